"""An exact host oracle for the training convolutions of csrc/conv_train.hip (no GPU, nothing of this library's kernels).

The kernels multiply and add in fp32 (v_mfma_f32_32x32x2_f32 and fmaf chains: "fp32 products, fp32 accumulation ... no operand is
narrowed", partial sums in a fixed order).  ``make_case`` builds DYADIC data -- inputs that are small integers or 0/1 spikes,
weights and biases that are small integers times 2^-SCALE_EXP, output gradients that are small integers -- so that every product is
an integer multiple of UNIT = 2^-SCALE_EXP, and it ASSERTS the condition that makes every answer unique: for each output element the
sum of the ABSOLUTE values of its products (the bias included; for the weight and bias gradients the sum runs over all N * Hv * Wv
positions), in units of UNIT, stays below 2^24.  Every partial sum of any subset of the products, in any order and any grouping, is
then an integer below 2^24 units: exactly representable in fp32, so no addition ever rounds and a correct kernel has ONE possible
fp32 result, whatever its order.  The oracle is torch's CPU fp64 conv2d / conv_transpose2d and its autograd, cast to fp32 (the cast
is exact by the same bound; checked).

``swapped`` is the oracle of the same BUFFERS read with H and W exchanged: what a kernel that took a row quantity for its column
twin would compute.  A case is only worth running if that differs from the true answer on every output tensor -- y, gi, gw and
the relu / masked forms (tests/test_conv_train_oracle_host.py checks it for every case of tests/_conv_train_cases.NONSQUARE_CASES
and MODULE_CASES; ``swapped_nchw_y`` serves the NCHW cases of the generic API convolution)."""
import zlib

import torch
import torch.nn.functional as F

SCALE_EXP = 4
UNIT = 2.0 ** -SCALE_EXP
EXACT_LIMIT = 2 ** 24
OUTPUTS = ("y", "gi", "gw", "gb")


def _operate(x, w, b, gy, stride, pad, transposed, out_pad):
    """(y, gi, gw, gb) of the layer in the dtype of its arguments: the framework's CPU operator and its autograd."""
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = None if b is None else b.clone().requires_grad_(True)
    y = F.conv_transpose2d(xr, wr, br, stride, pad, out_pad) if transposed else F.conv2d(xr, wr, br, stride, pad)
    gi, gw, *gb = torch.autograd.grad(y, (xr, wr) + (() if br is None else (br,)), gy)
    return y.detach(), gi, gw, (gb[0] if gb else None)


def _exact32(t, what):
    f = t.float()
    assert torch.equal(f.double(), t), f"{what}: the fp64 result is not an fp32 number"
    return f


def out_hw(geo):
    cin, cout, k, s, p, tr, op, H, W, N = geo
    size = (lambda n: (n - 1) * s - 2 * p + k + op) if tr else (lambda n: (n + 2 * p - k) // s + 1)
    return size(H), size(W)


def make_case(geo, seed, spikes=False, x_max=3, w_max=4, b_max=8, g_max=3):
    """geo = (Cin, Cout, k, stride, pad, transposed, out_pad, H, W, N).  Returns a dict of CPU tensors (logical NCHW; fp32 unless
    said otherwise): the data ``x`` (integers in [-x_max, x_max], or 0/1 ``spikes``), ``w`` and ``bias`` (integers in [-w_max, w_max] /
    [-b_max, b_max] times UNIT), ``gy`` (integers in [-g_max, g_max]); the oracle's ``y``, ``y_nobias``, ``relu_y``, ``gi``,
    ``gi_masked`` (x <= 0 ? 0 : gi -- the data gradient in front of a ReLU whose result x is), ``gw``, ``gb``; and ``abs_sums``: for
    each of y, gi, gw, gb the largest sum of absolute products of one output element in units of UNIT, each asserted below 2^24."""
    cin, cout, k, s, p, tr, op, H, W, N = geo
    g = torch.Generator().manual_seed(seed)

    def ints(shape, m):
        return torch.randint(-m, m + 1, shape, generator=g).double()

    x = (torch.rand(N, cin, H, W, generator=g) < 0.3).double() if spikes else ints((N, cin, H, W), x_max)
    w = ints((cin, cout, k, k) if tr else (cout, cin, k, k), w_max) * UNIT
    b = ints((cout,), b_max) * UNIT
    Ho, Wo = out_hw(geo)
    gy = ints((N, cout, Ho, Wo), g_max)
    y, gi, gw, gb = _operate(x, w, b, gy, s, p, tr, op)
    assert tuple(y.shape) == (N, cout, Ho, Wo)
    y_nb = (F.conv_transpose2d(x, w, None, s, p, op) if tr else F.conv2d(x, w, None, s, p))
    # the condition that makes the answers unique: the same operator on the absolute values bounds every partial sum
    ay, agi, agw, agb = _operate(x.abs(), w.abs(), b.abs(), gy.abs(), s, p, tr, op)
    abs_sums = {"y": float(ay.max()) / UNIT, "gi": float(agi.max()) / UNIT, "gw": float(agw.max()), "gb": float(agb.max())}
    for name, v in abs_sums.items():
        assert v < EXACT_LIMIT, f"{geo}: {name} sums {v} units of absolute products: fp32 partial sums could round"
    case = dict(geo=tuple(geo), abs_sums=abs_sums, x64=x, w64=w, b64=b, gy64=gy)
    for name, t in (("x", x), ("w", w), ("bias", b), ("gy", gy), ("y", y), ("y_nobias", y_nb), ("gi", gi), ("gw", gw), ("gb", gb)):
        case[name] = _exact32(t, name)
    case["relu_y"] = torch.relu(case["y"])
    case["gi_masked"] = torch.where(case["x"] <= 0, torch.zeros(()), case["gi"])
    return case


def cl_buffer(t):
    """The channels-last memory of a logical NCHW tensor, flat: what the kernels read and write."""
    return t.permute(0, 2, 3, 1).contiguous().flatten()


def nchw_buffer(t):
    return t.contiguous().flatten()


def swapped_nchw_y(case):
    """y of the same NCHW buffer of x read with H and W exchanged ([M][C][H][W] taken as [M][C][W][H]), flat: for the generic API
    convolution, whose tensors are NCHW."""
    cin, cout, k, s, p, tr, op, H, W, N = case["geo"]
    xs = case["x64"].contiguous().view(N, cin, W, H)
    y = F.conv_transpose2d(xs, case["w64"], case["b64"], s, p, op) if tr else F.conv2d(xs, case["w64"], case["b64"], s, p)
    return nchw_buffer(y).float()


def swapped(case):
    """{y, relu_y, gi, gi_masked, gw}: the oracle of the same buffers read with H and W exchanged -- x's memory [N][H][W][C] taken
    as [N][W][H][C], gy's likewise -- y and gi (and their epilogue forms; the mask is x's buffer, element for element) as flat
    channels-last buffers (compare with cl_buffer of the true ones), gw in the weight's shape."""
    cin, cout, k, s, p, tr, op, H, W, N = case["geo"]
    Ho, Wo = out_hw(case["geo"])
    xs = cl_buffer(case["x64"]).view(N, W, H, cin).permute(0, 3, 1, 2)
    gys = cl_buffer(case["gy64"]).view(N, Wo, Ho, cout).permute(0, 3, 1, 2)
    y, gi, gw, _ = _operate(xs, case["w64"], case["b64"], gys, s, p, tr, op)
    y, gi = cl_buffer(y).float(), cl_buffer(gi).float()
    return {"y": y, "relu_y": torch.relu(y), "gi": gi, "gi_masked": torch.where(cl_buffer(case["x"]) <= 0, torch.zeros(()), gi),
            "gw": gw.float()}


SWAP_CHECKED = ("y", "relu_y", "gi", "gi_masked", "gw")


_CASES = {}


def geo_of(c):
    layer = tuple(c["layer"])
    return layer[:8] + (layer[8] if len(layer) == 9 else layer[7], c["N"])


def for_case(c):
    """The data and oracle of a case of tests/_conv_train_cases.py: built once per process, shared, left unchanged.  Cases of one
    layer and image count share their data (the forward, the data gradient and the weight gradient of one layer)."""
    geo = geo_of(c)
    if geo not in _CASES:
        _CASES[geo] = make_case(geo, zlib.crc32(repr(geo).encode()), spikes=geo[0] >= 32)
    return _CASES[geo]


def outputs_of(c):
    """The oracle outputs the launch of case ``c`` is compared with."""
    if "T" in c:                                     # (a module case: forward and backward of the layer)
        return OUTPUTS
    return {"fwd": ("y",), "dgrad": ("gi",), "wgrad": ("gw", "gb") if c.get("bias", True) else ("gw",)}[c["op"]]
