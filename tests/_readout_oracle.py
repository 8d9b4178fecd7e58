"""Host oracle, case table and bounds of the collapsed read-out (spk_readout_collapsed_fwd, csrc/conv_mfma_gather.hip): the decoder's
last launch, out = conv(x) + bias * sum(coef) (tanh, u8) on x = sum_t coef[t] * spikes[t].  No GPU and nothing of the library here;
tests/test_readout_oracle_host.py checks this module on the CPU, tests/test_gpu_readout_oracle.py holds the kernels to it.

THE FORMS.  The launcher picks one of five kernels from the shape alone; readout_form() restates that arithmetic (and
tests/test_readout_oracle_host.py compares its constants with the source text):
    k3_r7_w28   readout_collapsed_k3_kernel<32,7,28>    k 3, Cin 32, Cout <= 8, H % 7 == 0, W == 28
    k3_r7       readout_collapsed_k3_kernel<32,7,0>     ... H % 7 == 0, any other W <= 32 with W % 4 == 0
    k3_r8_w32   readout_collapsed_k3_kernel<32,8,32>    ... H % 7 != 0, W == 32
    k3_r8       readout_collapsed_k3_kernel<32,8,0>     ... H % 7 != 0, any other such W
    generic     readout_collapsed_kernel                everything else the predicate takes
    refused     SPK_ERR_UNSUPPORTED

THE EXACT TIER (make_exact).  x holds multiples of 2^-6 in [0, 4), the weights multiples of 2^-8 with |w| <= 0.25 ("wide") or
|w| <= 2^-6 ("narrow"), the bias multiples of 2^-6 with |b| <= 1, coef 16 multiples of 2^-2 whose sum is at most 8.  Every product
x * w is a multiple of 2^-14, bias * sum(coef) a multiple of 2^-8, and the sum of the magnitudes of ALL terms of an output,
sum |x||w| + |bias * sum(coef)|, stays below 2^10 (k * k * Cin * 4 * 0.25 + 8 = 408 for the largest case, k 5 at Cin 16): every partial
sum of any subset of the terms is a multiple of 2^-14 below 2^10, 24 bits, an fp32 value.  So every fmaf, shuffle add and bias add of
the kernels is exact whatever the grouping, and the fp64 convolution cast to fp32 is the ONE correct answer: torch.equal, nothing
excluded.  The wide case saturates the u8 output without tanh (|m| of tens); the narrow one (bias within 2^-5, coef sum about 4) keeps at
least a third of the oracle's bytes strictly between 0 and 255.  No weight kernel equals its own 180-degree flip, and no two input
channels of an output channel carry equal weights: a kernel that reads a flipped tap or a neighbouring channel gives another number.

THE REAL-VALUED TIER (make_real).  x = collapse32(Bernoulli(0.15) spikes, 0.8^(15-t)), Gaussian weights and bias, the weights scaled
so that at least half of the pre-activations have |m| < 1 (tanh' > 0.42 there: an error before the tanh is not hidden behind it).

THE COEFFICIENT SUM.  ops.readout_collapsed adds the sixteen fp32 coefficients left to right in fp32 and hands the kernel that number;
coef_sum32() is that sum, and the oracle's bias term is bias * coef_sum32 (exactly sum(coef) in the exact tier)."""
from collections import namedtuple
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import _conv_bn_lif_oracle as O

# ------------------------------------------------------------------------------------------------ the dispatcher's mirror
RO_RB = 4                    # output rows per workgroup of the generic kernel
LDS_LIMIT = 64 * 1024        # bytes: the predicate's and the k3 branch's bound
K3_CIN = 32
K3_COUT_MAX = 8
K3_W_MAX = 32
K3_BANDS = (7, 8)            # rows per workgroup: H % 7 == 0 ? 7 : 8
K3_THREADS = 256             # (W / 4) * rb quads of four threads must fit one workgroup
WRAPPER_W = 64               # ops.readout_collapsed asks the predicate at this width and refuses wider images
FORMS = ("k3_r7_w28", "k3_r7", "k3_r8_w32", "k3_r8", "generic")


def generic_lds_bytes(Cin, Cout, k, W):
    """RO_RB + k - 1 input rows of W positions, channels padded by 4, and the whole weight (fp32)."""
    return ((RO_RB + k - 1) * W * (Cin + 4) + Cout * k * k * Cin) * 4


def k3_lds_bytes(Cout, W, rb):
    """rb + 2 input rows of W + 2 positions (one zero column on either side), 32 + 4 channels, and the weight."""
    return ((rb + 2) * (W + 2) * (K3_CIN + 4) + Cout * 9 * K3_CIN) * 4


def library_takes(Cin, Cout, k, W):
    """spk_readout_collapsed_supported at width W (W <= 0: at WRAPPER_W)."""
    if Cin <= 0 or Cout <= 0 or k <= 0:
        return False
    return k % 2 == 1 and Cin % 8 == 0 and generic_lds_bytes(Cin, Cout, k, W if W > 0 else WRAPPER_W) <= LDS_LIMIT


def wrapper_takes(W, Cin, Cout, k):
    """Does ops.readout_collapsed accept the shape?  It asks the predicate at width 64 whatever the image's width: (Cin 32, Cout 9,
    k 3) is refused at every width although the library takes it up to W = 63."""
    return W <= WRAPPER_W and library_takes(Cin, Cout, k, 0)


def readout_form(H, W, Cin, Cout, k):
    """The kernel spk_readout_collapsed_fwd launches for [B,H,W,Cin] -> [B,Cout,H,W] (pad == k / 2, any B below the grid cap)."""
    if not library_takes(Cin, Cout, k, W):
        return "refused"
    if k == 3 and Cin == K3_CIN and W % 4 == 0 and W <= K3_W_MAX and Cout <= K3_COUT_MAX:
        r7 = H % K3_BANDS[0] == 0
        rb = K3_BANDS[0] if r7 else K3_BANDS[1]
        if (W // 4) * rb * 4 <= K3_THREADS and k3_lds_bytes(Cout, W, rb) <= LDS_LIMIT:
            if r7:
                return "k3_r7_w28" if W == 28 else "k3_r7"
            return "k3_r8_w32" if W == 32 else "k3_r8"
    return "generic"


# ------------------------------------------------------------------------------------------------ the case table
# tr: the weight layouts a case runs with (True = ConvTranspose2d [Cin,Cout,k,k], read flipped); nobias: it ALSO runs with
# bias = None (one case of each form); note: what the case is there for
Case = namedtuple("Case", "form B H W Cin Cout k tr nobias note")
BOTH = (True, False)
CASES = [
    Case("k3_r7_w28", 2, 28, 28, 32, 1, 3, BOTH, True, "the MNIST decoder's own shape"),
    Case("k3_r7_w28", 1, 7, 28, 32, 8, 3, BOTH, False, "one band, Cout at the limit"),
    Case("k3_r7", 3, 14, 12, 32, 3, 3, BOTH, True, "runtime width, 21 of 64 thread groups"),
    Case("k3_r7", 1, 7, 4, 32, 1, 3, BOTH, False, "W = 4: one quad per row, 56 of 64 thread groups idle"),
    Case("k3_r7", 2, 21, 32, 32, 2, 3, BOTH, False, "W = 32 taken with the runtime width"),
    Case("k3_r8_w32", 2, 32, 32, 32, 3, 3, BOTH, True, "the CIFAR decoder's own shape"),
    Case("k3_r8_w32", 1, 9, 32, 32, 1, 3, BOTH, False, "second band of one row"),
    Case("k3_r8", 3, 20, 12, 32, 3, 3, BOTH, True, "last band of four rows"),
    Case("k3_r8", 2, 5, 28, 32, 1, 3, BOTH, False, "W = 28 with bands of eight: one ragged band"),
    Case("k3_r8", 1, 1, 4, 32, 1, 3, BOTH, False, "one row, one quad"),
    Case("generic", 2, 28, 28, 32, 9, 3, (True,), False, "Cout = 9: library entry only (the wrapper refuses it at every width)"),
    Case("generic", 2, 9, 30, 32, 2, 3, (False,), False, "W % 4 != 0 at Cin 32; ragged last band"),
    Case("generic", 2, 6, 36, 32, 1, 3, (True,), True, "W > 32"),
    Case("generic", 1, 6, 64, 32, 3, 3, (True,), False, "58 752 bytes of LDS: the widest image the wrapper takes"),
    Case("generic", 3, 5, 7, 8, 4, 1, (False,), False, "k = 1: four channels per thread"),
    Case("generic", 2, 9, 13, 16, 2, 5, (True,), False, "k = 5, transposed (pad' = k - 1 - pad = 2)"),
    Case("generic", 2, 3, 5, 24, 1, 3, (False,), False, "Cin = 24: 12 channels per thread"),
    Case("generic", 5, 1, 9, 32, 1, 3, (True,), False, "one row per image, five images"),
    Case("k3_r8", 5, 1, 8, 32, 1, 3, BOTH, False, "one row per image, two quads, five images (W % 4 == 0: not the generic kernel)"),
]
# shapes the library refuses (SPK_ERR_UNSUPPORTED): (H, W, Cin, Cout, k, why)
REFUSED = [
    (6, 64, 32, 9, 3, "65 664 bytes of LDS"),
    (28, 28, 32, 1, 4, "even k"),
    (28, 28, 30, 1, 3, "Cin % 8 != 0"),
    (8, 48, 64, 1, 5, "k 5 at Cin 64 and W 48: over the LDS limit"),
]
# one case per form plus the ragged-band and W = 4 cases: the guarded-buffer and locality tests
EDGE_CASES = [CASES[i] for i in (0, 2, 6, 7, 3, 9, 11, 15)]

Variant = namedtuple("Variant", "case tr bias")


def variants():
    """(case, transposed, with bias) of every run of the table."""
    out = []
    for c in CASES:
        out += [Variant(c, tr, True) for tr in c.tr]
        if c.nobias:
            out.append(Variant(c, c.tr[0], False))
    return out


def vid(v):
    c = v.case
    return f"{c.form}-B{c.B}-{c.H}x{c.W}-ci{c.Cin}-co{c.Cout}-k{c.k}-{'T' if v.tr else 'N'}" + ("" if v.bias else "-nobias")


def case_seed(c):
    return 4000 + (c.B * 7 + c.H * 131 + c.W * 17 + c.Cin * 3 + c.Cout * 1009 + c.k * 53) % 1000


# ------------------------------------------------------------------------------------------------ inputs
def _flip(w):
    return w.flip(-1).flip(-2)


def weights_distinct(w_oihw):
    """[Cout,Cin,k,k]: no kernel equals its own 180-degree flip (k > 1), and within an output channel no two input channels are equal."""
    Cout, Cin, k, _ = w_oihw.shape
    if k > 1 and bool((w_oihw == _flip(w_oihw)).flatten(2).all(2).any()):
        return False
    flat = w_oihw.flatten(2)
    same = (flat.unsqueeze(2) == flat.unsqueeze(1)).all(3)                 # [Cout,Cin,Cin]
    return int(same.sum()) == Cout * Cin


def dyadic_weights(Cout, Cin, k, g, n):
    """[Cout,Cin,k,k] integers in [-n, n] / 256 that pass weights_distinct (k = 1: drawn without replacement per output channel)."""
    if k == 1:
        assert 2 * n + 1 >= Cin
        q = torch.stack([torch.randperm(2 * n + 1, generator=g)[:Cin] - n for _ in range(Cout)]).view(Cout, Cin, 1, 1)
        w = q.float() / 256.0
    else:
        for _ in range(64):
            w = torch.randint(-n, n + 1, (Cout, Cin, k, k), generator=g).float() / 256.0
            if weights_distinct(w):
                break
    assert weights_distinct(w)
    return w


def as_layout(w_oihw, transposed):
    """The layer's own weight tensor whose CORRELATION kernel is w_oihw: Conv2d [Cout,Cin,k,k] as it is; ConvTranspose2d [Cin,Cout,k,k]
    holds the flipped taps (a stride-1 transposed convolution is the correlation with the flipped kernel)."""
    return _flip(w_oihw).transpose(0, 1).contiguous() if transposed else w_oihw.contiguous()


def make_exact(v, narrow=False):
    """The dyadic inputs of a variant (see the module docstring).  x [B,Cin,H,W]; w in the variant's layout; bias or None; coef [16]."""
    c = v.case
    g = torch.Generator().manual_seed(case_seed(c) + (500 if narrow else 0))
    x = torch.randint(0, 256, (c.B, c.Cin, c.H, c.W), generator=g).float() / 64.0
    w = dyadic_weights(c.Cout, c.Cin, c.k, g, 4 if narrow else 64)
    if narrow:
        bias = torch.randint(-2, 3, (c.Cout,), generator=g).float() / 64.0
        coef = torch.full((16,), 0.25)
        coef[torch.randperm(16, generator=g)[:3]] = 0.5                       # sum 4.75
    else:
        bias = torch.randint(-64, 65, (c.Cout,), generator=g).float() / 64.0
        coef = torch.randint(0, 3, (16,), generator=g).float() / 4.0
        coef[0] = 0.25                                                         # (never all zero)
    return SimpleNamespace(v=v, x=x, w=as_layout(w, v.tr), w_oihw=w, bias=bias if v.bias else None, coef=coef)


REAL_W_SCALE = 0.8           # std of the weighted sum before the bias, in units of the pre-activation
REAL_BIAS_STD = 0.05         # (times sum(coef) = 4.86: an offset of about a quarter)
X_SECOND_MOMENT = 0.88       # E[x^2] of x = sum_t 0.8^(15-t) * Bernoulli(0.15): 0.15 * 0.85 * 2.78 + (0.15 * 4.86)^2


def model_coef():
    return torch.pow(torch.tensor(0.8), torch.arange(15, -1, -1).float())


def make_real(v):
    """The real-valued inputs of a variant: collapsed Bernoulli(0.15) spikes under the model's coef, Gaussian weights and bias."""
    c = v.case
    g = torch.Generator().manual_seed(case_seed(c) + 250)
    coef = model_coef()
    spikes = (torch.rand((16, c.B, c.Cin, c.H, c.W), generator=g) < O.SPIKE_DENSITY).float()
    x = O.collapse32(spikes, coef)
    w = torch.randn((c.Cout, c.Cin, c.k, c.k), generator=g) * (REAL_W_SCALE / (X_SECOND_MOMENT * c.Cin * c.k * c.k) ** 0.5)
    bias = torch.randn((c.Cout,), generator=g) * REAL_BIAS_STD
    return SimpleNamespace(v=v, x=x, w=as_layout(w, v.tr), w_oihw=w, bias=bias if v.bias else None, coef=coef, spikes=spikes)


def to_bhwc(x_bchw):
    return x_bchw.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the oracle
def coef_sum32(coef):
    """The sixteen coefficients added in fp32 from the left: the number ops.readout_collapsed hands the kernel."""
    s = torch.zeros((), dtype=torch.float32)
    for cv in coef.float().reshape(-1):
        s = s + cv
    return float(s)


def conv64(x_bchw, w, k, transposed):
    """The layer's convolution in fp64 with the layer's own torch function (stride 1, pad k / 2), no bias."""
    if transposed:
        return F.conv_transpose2d(x_bchw.double(), w.double(), None, 1, k // 2)
    return F.conv2d(x_bchw.double(), w.double(), None, 1, k // 2)


def readout64(x_bchw, w, bias, coef, k, transposed):
    """(m, mag): the fp64 pre-activation conv(x) + bias * coef_sum32 [B,Cout,H,W] and the sum of the magnitudes of its terms,
    sum |x||w| + |bias * coef_sum32|."""
    m = conv64(x_bchw, w, k, transposed)
    mag = conv64(x_bchw.abs(), w.abs(), k, transposed)
    if bias is not None:
        bt = bias.double().view(1, -1, 1, 1) * coef_sum32(coef)
        m, mag = m + bt, mag + bt.abs()
    return m, mag


def oracle(case):
    """readout64 of a case built by make_exact / make_real."""
    return readout64(case.x, case.w, case.bias, case.coef, case.v.case.k, case.v.tr)


def conv32(case):
    """The same in plain fp32 torch (the reference that must pass the real-valued bar on its own)."""
    k = case.v.case.k
    y = F.conv_transpose2d(case.x, case.w, None, 1, k // 2) if case.v.tr else F.conv2d(case.x, case.w, None, 1, k // 2)
    if case.bias is not None:
        y = y + (case.bias * torch.tensor(coef_sum32(case.coef))).view(1, -1, 1, 1)
    return y


def fp32_bound(k, Cin, mag):
    """|fp32 evaluation - fp64 value| of one output of the read-out kernels, first order, in ANY grouping of the additions.

    An output is the sum of n = k * k * Cin products x * w and of bias * coef_sum.  The kernels split the n products over two or four
    threads; a thread adds its share with one fmaf per product (one rounding each, relative error <= 2^-24 of the partial sum it
    produces), the shares are joined by one or two shuffle additions, bias * coef_sum is rounded once as a product and the bias
    addition rounds once more (or the compiler contracts product and addition into one fmaf: one rounding fewer).  Every rounding
    acts on a partial sum whose magnitude is at most mag = sum |x||w| + |bias * coef_sum|, and no term passes through more than
    n + 4 roundings (at most n fmaf's, two shuffle additions, the bias product, the bias addition), so
        |error| <= (k * k * Cin + 4) * 2^-24 * mag
    to first order (the second-order terms are below 2^-24 of this).  Taps in the zero border add exact zeros."""
    return (k * k * Cin + 4) * 2.0 ** -24 * mag


def u8_rule(pv):
    """(uint8)(fminf(fmaxf(pv + 0.5f, 0), 1) * 255.0f) in fp32 torch: fmaxf(NaN, 0) = 0, the cast truncates."""
    assert pv.dtype == torch.float32
    q = (pv + torch.tensor(0.5, dtype=torch.float32))
    q = torch.where(torch.isnan(q), torch.zeros_like(q), q).clamp(0.0, 1.0) * torch.tensor(255.0, dtype=torch.float32)
    return q.to(torch.uint8)


def readout_check(what, got_f32, got_u8, want64, bound, tanh_err=0.0):
    """got fp32 [B,C,Ho,Wo] within ``bound`` (+ tanhf's own error) of the fp64 value; every u8 byte that differs from the oracle's
    differs by one AND has its oracle pre-truncation value within 255 x that bound of an integer."""
    tol = bound + tanh_err
    err = (got_f32.double() - want64).abs()
    worst = float((err - tol).max())
    assert worst <= 0.0, (what, "exceeds the read-out bound by", worst, "max err", float(err.max()), "at", int((err - tol).argmax()))
    if got_u8 is not None:
        q64 = torch.clamp(want64 + 0.5, 0.0, 1.0) * 255.0
        want_u8 = q64.floor().clamp(max=255.0)
        diff = got_u8.double() - want_u8
        off = diff != 0
        if bool(off.any()):
            assert float(diff[off].abs().max()) == 1.0, (what, "u8 differs by more than one")
            dist = (q64 - q64.round()).abs()
            assert bool((dist[off] <= 255.0 * tol[off]).all()), (what, "u8 differs away from a truncation boundary",
                                                                 float(dist[off].max()))
    return float(err.max())


def nan_reach(c, b, y, x):
    """bool [B,Cout,H,W]: the outputs one NaN at x[b, :, y, x] (any single channel) reaches: the k x k neighbourhood, every Cout."""
    m = torch.zeros((c.B, c.Cout, c.H, c.W), dtype=torch.bool)
    r = c.k // 2
    m[b, :, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
    return m


# ------------------------------------------------------------------------------------------------ the decoder chain
# (latent H, latent W, image channels, the read-out form of the 4H x 4W image, latent channels)
CHAIN_ROWS = [
    (7, 7, 1, "k3_r7_w28", 16),    # both stride-2 layers have an fp6 instance
    (8, 8, 3, "k3_r8_w32", 16),
    (5, 3, 3, "k3_r8", 16),        # no fp6 instance: the gather kernels all the way
    (7, 4, 1, "k3_r7", 16),
    (4, 9, 3, "generic", 16),      # W = 36
    (7, 7, 1, "k3_r7_w28", 32),    # 32 latent channels: only the second layer has an fp6 instance, the gather kernel hands it S32 records
]
CHAIN_B = 3


def chain_id(row):
    return f"{row[0]}x{row[1]}-D{row[4]}-C{row[2]}-{row[3]}"


def chain_seed(row):
    return 7100 + 10 * row[0] + row[1] + row[4]


def chain_geos(h, w, C, D=16, B=CHAIN_B):
    """The reference Decoder's three layers as geometry tuples of _conv_bn_lif_oracle (Cin, Cout, k, s, p, transposed, out_pad, H, W, B)."""
    return [(D, 64, 3, 2, 1, True, 1, h, w, B), (64, 32, 3, 2, 1, True, 1, 2 * h, 2 * w, B),
            (32, C, 3, 1, 1, True, 0, 4 * h, 4 * w, B)]


def chain_params(row):
    """Dyadic weights (O.make_case) and arbitrary BatchNorm statistics of the three layers, and two spike inputs [16,B,D,h,w].
    The stride-2 layers see k * k / 4 taps per output; their weights are doubled (still dyadic) to keep the layers firing.  The read-out
    layer's weights are an eighth and its bias a quarter of make_case's (drawn for one spike frame; it sees the sum of sixteen at twice
    the density), so that the image is not all saturated tanh."""
    h, w, C, _, D = row
    seed = chain_seed(row)
    g = torch.Generator().manual_seed(seed)
    layers = []
    for i, geo in enumerate(chain_geos(h, w, C, D)):
        cs = O.make_case(geo, seed + 10 * i)
        co = geo[1]
        bn = None
        if i < 2:
            bn = dict(weight=torch.rand(co, generator=g) + 1.0, bias=torch.rand(co, generator=g) * 0.8,
                      running_mean=torch.rand(co, generator=g) * 0.6 - 0.3, running_var=torch.rand(co, generator=g) * 0.5 + 0.5)
        layers.append(SimpleNamespace(geo=geo, w=cs.w * (2.0 if i < 2 else 0.125), bias=cs.bias * (1.0 if i < 2 else 0.25), bn=bn))
    xs = [(torch.rand((16, CHAIN_B, D, h, w), generator=g) < O.SPIKE_DENSITY).float() for _ in range(2)]
    return SimpleNamespace(layers=layers, xs=xs, coef=model_coef(), C=C, h=h, w=w, D=D)


def chain_oracle(p, terms):
    """The chain on the host, layer by layer (terms: the (a, b) BatchNorm terms of the two LIF layers): the reset-state run on input 0
    and the carried run on input 1 from the membrane potentials input 0 left.  Returns [(m64, mag, rates)] for the two runs, m64 the
    fp64 read-out of collapse32(second layer's oracle spikes)."""
    out, vs = [], [None, None]
    for x in p.xs:
        rates = []
        for i in range(2):
            L = p.layers[i]
            x, vs[i], _ = O.conv_bn_lif(x, L.w, L.bias, terms[i][0], terms[i][1], vs[i], L.geo)
            rates.append(float(x.mean()))
        L = p.layers[2]
        m, mag = readout64(O.collapse32(x, p.coef), L.w, L.bias, p.coef, 3, True)
        out.append((m, mag, rates))
    return out
