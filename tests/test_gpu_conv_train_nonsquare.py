"""The training convolutions of csrc/conv_train.hip on NON-SQUARE maps, bit for bit against an exact host oracle.

Every other test of these kernels (tests/test_gpu_conv_train.py) builds (N, C, H, H) tensors and compares within a tolerance.  Here
every map has H != W -- one case per kernel and branch, tests/_conv_train_cases.NONSQUARE_CASES, each shown on the host to land where
it says and to change its answer when H and W are exchanged (tests/test_conv_train_oracle_host.py) -- and the data are dyadic
(tests/_conv_train_oracle.py): every fp32 partial sum is exact in any order, so each output has ONE correct fp32 value and every
comparison is ``torch.equal`` with torch's CPU fp64 operator, nothing excluded, no tolerance anywhere.

Direct C-ABI calls (spk_conv_train_gather, _gather_relu, _gather_masked, spk_conv_train_wgrad) are one launch into NaN-filled outputs
and a NaN-filled workspace, each allocated between two guard bands of a sentinel that must survive.  Above them: the autograd wrapper
(ops.NativeConvTrainFunction) in all four layout combinations, and the layer.Conv2d / layer.ConvTranspose2d modules in train() on a
[T, B, C, H, W] rectangular input, with the native entry points counted.  Last, the generic fp32 API convolution
(conv_nchw_kernel of csrc/conv_direct.hip, fp64 accumulation): non-square, with and without bias, and past its grid cap."""
import pytest
import torch

import _conv_train_cases as cases
import _conv_train_oracle as O
from parity_report import record as parity

pytestmark = pytest.mark.gpu

CL = torch.channels_last
NAN = float("nan")
GUARD = 256                  # floats on either side of an output (1 KiB: the payload stays 16-byte aligned)
SENTINEL = -12345.75
STATS = {}                   # family -> [case ids, elements compared, mismatches]
NS = {c["id"]: c for c in cases.NONSQUARE_CASES}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def _tally(fam, cid, got, want, what):
    """torch.equal with the mismatch pattern in the message; counts into the family's parity record."""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (cid, what, tuple(got.shape), tuple(want.shape), got.dtype)
    bad = ~(got == want)                                                     # (a NaN counts as a mismatch)
    n_bad = int(bad.sum())
    st = STATS.setdefault(fam, [set(), 0, 0])
    st[0].add(cid)
    st[1] += want.numel()
    st[2] += n_bad
    parity(f"conv_train_nonsquare_{fam}", cases=len(st[0]), elements=st[1], mismatches=st[2])
    assert n_bad == 0, (cid, what, f"{n_bad} of {want.numel()} differ; first at", bad.nonzero()[:8].tolist())


class Guarded:
    """``numel`` floats filled with ``fill`` between two guard bands of SENTINEL."""

    def __init__(self, dev, numel, fill=NAN):
        self.buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.payload = self.buf[GUARD:GUARD + numel]
        self.payload.fill_(fill)
        assert self.payload.data_ptr() % 16 == 0

    def nchw_view_of_cl(self, shape):
        """The payload as the channels-last memory of a logical [N, C, H, W] tensor."""
        N, C, H, W = shape
        return self.payload.view(N, H, W, C).permute(0, 3, 1, 2)

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all())


def _family(c):
    return cases.launch(c)["kernel"]


def _device_case(dev, c):
    case = O.for_case(c)
    d = {k: case[k].to(dev) for k in ("x", "w", "bias", "gy")}
    d["x"], d["gy"], d["w"] = (d[k].contiguous(memory_format=CL) for k in ("x", "gy", "w"))
    return case, d


def _gather(dev, ops, c, epi=None, bias=True):
    """One gather launch of case ``c`` ('fwd' or 'dgrad'; ``epi`` None / 'relu' / 'masked') -> (result, the oracle's tensor name)."""
    case, d = _device_case(dev, c)
    tr, op = c["layer"][5], c["op"]
    tap, s_ci, s_co = ops._conv_w_strides(d["w"], tr)
    lib, P, stream = ops.lib, ops._p, ops._stream(d["x"])
    geo = cases.gather_args(c["layer"], c["N"], op)
    if op == "fwd":
        src, b, strides, shape = d["x"], (d["bias"] if bias else None), (tap, s_ci, s_co), case["y"].shape
        name = {None: "y" if bias else "y_nobias", "relu": "relu_y"}[epi]
        assert bias or epi is None
    else:
        src, b, strides, shape = d["gy"], None, (tap, s_co, s_ci), case["x"].shape
        name = {None: "gi", "masked": "gi_masked"}[epi]
    assert tuple(shape) == (geo[0], geo[6], geo[4], geo[5])
    out = Guarded(dev, case[name].numel())
    if epi == "masked":
        ops.check(lib.spk_conv_train_gather_masked(P(src), P(d["w"]), P(b), P(d["x"]), P(out.payload), *geo, *strides, stream),
                  "spk_conv_train_gather_masked")
    else:
        fn = "spk_conv_train_gather_relu" if epi == "relu" else "spk_conv_train_gather"
        ops.check(getattr(lib, fn)(P(src), P(d["w"]), P(b), P(out.payload), *geo, *strides, stream), fn)
    torch.cuda.synchronize()
    assert out.intact(), f"{c['id']}: a guard band of the output was written"
    return out.nchw_view_of_cl(shape), case[name]


GATHER_CASES = [c for c in cases.NONSQUARE_CASES if c["op"] != "wgrad"]
WGRAD_CASES = [c for c in cases.NONSQUARE_CASES if c["op"] == "wgrad"]


@pytest.mark.parametrize("c", GATHER_CASES, ids=lambda c: c["id"])
def test_gather_on_non_square_maps_equals_the_oracle(dev, ops, c):
    assert c["claim"](cases.launch(c)), (c["why"], cases.launch(c))
    got, want = _gather(dev, ops, c)
    _tally(_family(c), c["id"], got, want, "y" if c["op"] == "fwd" else "gi")


@pytest.mark.parametrize("cid,epi", [
    ("gather_f0_s2_two_tiles_9x6", "relu"), ("gather_f1_outpad0_5x3", "relu"), ("gather_f1_k4_4x7", "relu"), ("c1in_3ch_16x10", "relu"),
    ("gather_f0_dgrad_convT_5x3", "masked"), ("gather_f1_dgrad_9x6", "masked"), ("c1in_dgrad_readout_6x10", "masked")])
def test_relu_and_masked_epilogues_on_non_square_maps(dev, ops, cid, epi):
    """relu(y) from the forward launch and the data gradient in front of a ReLU (x <= 0 ? 0 : gi) from the masked launch: on form 0
    and form 1 of the matrix kernel and on the few-channel input kernel (the instantiations the CNN VQ-VAE added)."""
    c = NS[cid]
    got, want = _gather(dev, ops, c, epi=epi)
    assert int((want == 0).sum()) > 0 and int((want != 0).sum()) > 0
    _tally(_family(c) + "_" + epi, cid, got, want, epi)


@pytest.mark.parametrize("cid", ["gather_f0_s1_ragged_5x9", "gather_f1_outpad1_5x3", "c1in_2ch_s1_7x5", "c1out_3ch_6x10"])
def test_gather_without_bias_on_non_square_maps(dev, ops, cid):
    """bias_or_null = NULL on each gather kernel."""
    c = NS[cid]
    got, want = _gather(dev, ops, c, bias=False)
    _tally(_family(c) + "_nobias", cid, got, want, "y without bias")


@pytest.mark.parametrize("c", WGRAD_CASES, ids=lambda c: c["id"])
def test_weight_and_bias_gradient_on_non_square_maps_equal_the_oracle(dev, ops, c):
    L = cases.launch(c)
    assert c["claim"](L), (c["why"], L)
    case, d = _device_case(dev, c)
    tr, k = c["layer"][5], c["layer"][2]
    lib, P, stream = ops.lib, ops._p, ops._stream(d["x"])
    n, Hu, Wu, Cu, Hv, Wv, Cv, k_, s, p, bias_from = cases.wgrad_args(c["layer"], c["N"])
    want_bias = c.get("bias", True)
    gw_g = Guarded(dev, d["w"].numel())
    gw = gw_g.payload.as_strided(d["w"].shape, d["w"].stride())              # dense: the channels-last weight's own strides
    gb_g = Guarded(dev, case["gb"].numel())
    g_tap, g_ci, g_co = ops._conv_w_strides(gw, tr)
    u, v, g_u, g_v = (d["gy"], d["x"], g_co, g_ci) if tr else (d["x"], d["gy"], g_ci, g_co)
    assert tuple(u.shape) == (n, Cu, Hu, Wu) and tuple(v.shape) == (n, Cv, Hv, Wv)
    nb = int(lib.spk_conv_train_wgrad_ws_bytes(n, Hv, Wv, Cu, Cv, k))
    assert nb == L["ws_bytes"] and nb % 4 == 0
    ws = Guarded(dev, nb // 4)
    ops.check(lib.spk_conv_train_wgrad(P(u), P(v), P(ws.payload), nb, P(gw_g.payload), P(gb_g.payload) if want_bias else None, n, Hu, Wu,
                                       Cu, Hv, Wv, Cv, k, s, p, g_tap, g_u, g_v, bias_from, stream), "spk_conv_train_wgrad")
    torch.cuda.synchronize()
    assert gw_g.intact() and gb_g.intact() and ws.intact(), f"{c['id']}: a guard band was written"
    _tally(_family(c), c["id"], gw, case["gw"], "gw")
    if want_bias:
        _tally(_family(c), c["id"], gb_g.payload, case["gb"], "gb")
    else:
        assert bool(torch.isnan(gb_g.payload).all()), "no bias gradient was asked for"


@pytest.mark.parametrize("cid", ["gather_f1_outpad0_5x3", "c1in_2ch_s1_7x5", "c1out_3ch_6x10"])
@pytest.mark.parametrize("w_cl", [True, False], ids=["wCL", "wNCHW"])
@pytest.mark.parametrize("x_cl", [True, False], ids=["xCL", "xNCHW"])
def test_autograd_wrapper_on_non_square_maps_equals_the_oracle(dev, ops, cid, w_cl, x_cl):
    """ops.NativeConvTrainFunction forward and backward, one layer per gather kernel (the matrix kernel, the few-channel input kernel,
    the few-channel output kernel; their data and weight gradients land on the other kernels), channels-last and NCHW weights,
    channels-last and NCHW x / gy: y, gi, gw and gb are the oracle's, bit for bit."""
    c = NS[cid]
    case = O.for_case(c)
    cin, cout, k, st, pd, tr, op = c["layer"][:7]
    fmt = (lambda t, cl: t.contiguous(memory_format=CL) if cl else t.contiguous())
    x = fmt(case["x"].to(dev), x_cl).requires_grad_(True)
    w = fmt(case["w"].to(dev), w_cl).requires_grad_(True)
    b = case["bias"].to(dev).requires_grad_(True)
    assert ops.conv_train_supported(x.shape, w, st, pd, tr, op, True, forward=True), "shape not taken by the native kernels"
    y = ops.NativeConvTrainFunction.apply(x, w, b, st, pd, tr, op)
    y.backward(fmt(case["gy"].to(dev), x_cl))
    torch.cuda.synchronize()
    assert w.grad.stride() == w.stride()
    for name, got in (("y", y), ("gi", x.grad), ("gw", w.grad), ("gb", b.grad)):
        _tally("wrapper", cid, got, case[name], name)


@pytest.mark.parametrize("c", cases.MODULE_CASES, ids=lambda c: c["id"])
def test_modules_in_train_mode_on_a_rectangular_sequence(dev, ops, monkeypatch, c):
    """layer.Conv2d / layer.ConvTranspose2d (step_mode 'm', train()) on [T, B, C, H, W] with H != W (tests/_conv_train_cases.
    MODULE_CASES: claim, bound and exchange checked on the host): the native entry points are the ones called (counted, as
    tests/_dispatch_recorders.py counts launches -- here the calls pass through), and y, x.grad, weight.grad and bias.grad equal the
    oracle bit for bit."""
    from spikingjelly.activation_based import layer
    assert c["claim"](cases.launch(c)), (c["why"], cases.launch(c))
    T, B = c["T"], c["B"]
    cin, cout, k, st, pd, tr, op, H, W, N = O.geo_of(c)
    case = O.for_case(c)
    calls = {}
    for name in ("conv_train_forward", "conv_train_backward", "conv2d", "conv_transpose2d"):
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    m = (layer.ConvTranspose2d(cin, cout, k, st, pd, op, step_mode='m') if tr else layer.Conv2d(cin, cout, k, st, pd, step_mode='m'))
    m = m.to(dev).train()
    with torch.no_grad():
        m.weight.copy_(case["w"].to(dev))
        m.bias.copy_(case["bias"].to(dev))
    x = case["x"].to(dev).view(T, B, cin, H, W).requires_grad_(True)
    y = m(x)
    assert tuple(y.shape) == (T, B) + tuple(case["y"].shape[1:])
    y.backward(case["gy"].to(dev).view(y.shape))
    torch.cuda.synchronize()
    assert calls == {"conv_train_forward": 1, "conv_train_backward": 1}, calls
    cid = c["id"]
    for name, got in (("y", y.flatten(0, 1)), ("gi", x.grad.flatten(0, 1)), ("gw", m.weight.grad), ("gb", m.bias.grad)):
        _tally("module", cid, got, case[name], name)


# ---- the generic fp32 API convolution (csrc/conv_direct.hip: conv_nchw_kernel behind spk_conv2d_fwd / spk_conv_transpose2d_fwd):
# NCHW, fp64 accumulation -- on dyadic data y equals the oracle everywhere
@pytest.mark.parametrize("c", [c for c in cases.API_CONV_CASES if c["layer"][2] > 1], ids=lambda c: c["id"])
def test_api_convolution_on_non_square_maps_with_and_without_bias(dev, ops, c):
    assert c["claim"](cases.launch(c)), (c["why"], cases.launch(c))
    cin, cout, k, s, p, transposed = c["layer"][:6]
    case = O.for_case(c)
    x, w, b = (case[n].to(dev) for n in ("x", "w", "bias"))
    for bias, name in ((b, "y"), (None, "y_nobias")):
        y = ops.conv_transpose2d(x, w, bias, s, p, 0) if transposed else ops.conv2d(x, w, bias, s, p)
        assert y.is_contiguous()
        _tally("api_conv", c["id"], y, case[name], name)


def test_api_convolution_walks_its_grid_a_second_time(dev, ops):
    """1x1, one input channel, 64 x 63 maps, 347 x 3 of them: just above GRID_CAP * 256 outputs (the case's claim), so the first
    threads of the capped grid take a second element -- into a NaN-filled output between guard bands."""
    c = next(c for c in cases.API_CONV_CASES if c["layer"][2] == 1)
    L = cases.launch(c)
    assert c["claim"](L), (c["why"], L)
    cin, cout, k, s, p, tr, op, H, W, M = O.geo_of(c)
    case = O.for_case(c)
    x, w, b = (case[n].to(dev).contiguous() for n in ("x", "w", "bias"))
    out = Guarded(dev, L["total"])
    ops.check(ops.lib.spk_conv2d_fwd(ops._p(x), ops._p(w), ops._p(b), ops._p(out.payload), M, cin, H, W, cout, k, s, p, ops._stream(x)),
              "spk_conv2d_fwd")
    torch.cuda.synchronize()
    assert out.intact()
    _tally("api_conv", c["id"], out.payload.view(case["y"].shape), case["y"], "y past the grid cap")
