"""CPU checks of tests/_readout_oracle.py: the conditions on the inputs that make the exact tier exact and the real-valued tier
sensitive, the mirror of the read-out dispatcher against the source text and against the library's own predicate, the comparison's
power to reject three wrong kernels computed on the host, and the argument errors of spk_readout_collapsed_fwd (which need no device)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _conv_bn_lif_oracle as O
import _readout_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "spiking-diffusion_amd", "csrc", "conv_mfma_gather.hip")
VARIANTS = R.variants()
K3_VARIANTS = [v for v in VARIANTS if v.case.form != "generic"]


def _exact_cases():
    return [(v, narrow) for v in VARIANTS for narrow in (False, True)]


def _eid(p):
    return R.vid(p[0]) + ("-narrow" if p[1] else "-wide")


@pytest.mark.parametrize("p", _exact_cases(), ids=_eid)
def test_exact_tier_inputs_keep_the_dyadic_budget(p):
    """From the actual tensors: the grids of x, w, bias and coef; every product on the 2^-14 grid; the magnitudes of all terms of an
    output below 2^10; hence the fp64 value IS an fp32 value, and a plain fp32 convolution reproduces it bit for bit."""
    v, narrow = p
    c = R.make_exact(v, narrow)
    k = v.case.k

    def on_grid(t, bits):
        s = t.double() * 2.0 ** bits
        return bool((s == s.round()).all())

    assert on_grid(c.x, 6) and float(c.x.min()) >= 0.0 and float(c.x.max()) < 4.0
    assert on_grid(c.w, 8) and float(c.w.abs().max()) <= (2.0 ** -6 if narrow else 0.25)
    assert on_grid(c.coef, 2) and c.coef.numel() == 16 and 0.0 < float(c.coef.sum()) <= 8.0 and float(c.coef.min()) >= 0.0
    assert R.coef_sum32(c.coef) == float(c.coef.double().sum())
    if c.bias is not None:
        assert on_grid(c.bias, 6) and float(c.bias.abs().max()) <= 1.0
    assert R.weights_distinct(c.w_oihw)
    m, mag = R.oracle(c)
    assert float(mag.max()) < 2.0 ** 10
    assert on_grid(m, 14) and on_grid(mag, 14)
    assert torch.equal(m.float().double(), m)
    assert torch.equal(R.conv32(c), m.float()), "a plain fp32 convolution of dyadic inputs is exact"
    # the two layouts of a weight describe the same correlation
    corr = F.conv2d(c.x.double(), c.w_oihw.double(), None, 1, k // 2)
    assert torch.equal(corr, R.conv64(c.x, c.w, k, v.tr))
    byte = R.u8_rule(m.float())
    inside = float(((byte > 0) & (byte < 255)).float().mean())
    if narrow:
        assert inside >= 1.0 / 3.0, inside
    assert float(m.abs().max()) > 0.0


def test_collapsing_commutes_with_the_linear_layer():
    """conv(sum_t coef_t s_t) + bias * sum(coef) == sum_t coef_t (conv(s_t) + bias) in fp64 (to fp64 round-off), both layouts."""
    for v in (VARIANTS[0], VARIANTS[1], [v for v in VARIANTS if v.case.k == 5][0]):
        c = R.make_real(v)
        k = v.case.k
        coef = c.coef.double()
        x64 = (c.spikes.double() * coef.view(-1, 1, 1, 1, 1)).sum(0)
        lhs = R.conv64(x64, c.w, k, v.tr)
        rhs = sum(coef[t] * R.conv64(c.spikes[t], c.w, k, v.tr) for t in range(16))
        if c.bias is not None:
            lhs = lhs + c.bias.double().view(1, -1, 1, 1) * coef.sum()
            rhs = rhs + sum(coef[t] * c.bias.double().view(1, -1, 1, 1) for t in range(16))
        assert float((lhs - rhs).abs().max()) <= 1e-13 * max(1.0, float(rhs.abs().max()))
        # the fp32 collapse the producing kernels hand over is that tensor up to fp32 round-off of sixteen additions
        assert float((c.x.double() - x64).abs().max()) <= 16 * 2.0 ** -24 * float(x64.max())


def test_every_form_is_reached_and_refusals_are_named():
    forms = {f: 0 for f in R.FORMS}
    for c in R.CASES:
        got = R.readout_form(c.H, c.W, c.Cin, c.Cout, c.k)
        assert got == c.form, (c, got)
        forms[got] += 1
    assert all(n >= 2 for n in forms.values()), forms
    for f in R.FORMS:
        assert sum(1 for c in R.CASES if c.form == f and c.nobias) >= 1, f
        assert any(c.form == f for c in R.EDGE_CASES), f
    assert all(set(c.tr) == {True, False} for c in R.CASES if c.form != "generic")
    gen = [c for c in R.CASES if c.form == "generic"]
    assert {tr for c in gen for tr in c.tr} == {True, False}
    assert {c.k for c in gen} == {1, 3, 5} and {c.Cin for c in gen} == {8, 16, 24, 32}
    assert any(c.W % 4 and c.Cin == 32 for c in gen) and any(c.W > 32 for c in gen)
    assert len(R.REFUSED) >= 1
    for H, W, Cin, Cout, k, why in R.REFUSED:
        assert R.readout_form(H, W, Cin, Cout, k) == "refused", why
    # the wrapper asks at width 64: it refuses (32, 9, 3) although the library takes it at 28
    lib_only = [c for c in R.CASES if not R.wrapper_takes(c.W, c.Cin, c.Cout, c.k)]
    assert [(c.Cin, c.Cout, c.k, c.W) for c in lib_only] == [(32, 9, 3, 28)]
    assert R.library_takes(32, 9, 3, 63) and not R.library_takes(32, 9, 3, 64)
    assert R.generic_lds_bytes(32, 3, 3, 64) == 58752 and R.generic_lds_bytes(32, 9, 3, 64) == 65664


def test_mirror_agrees_with_the_library_predicate():
    from spkdiff import _lib, ops
    lib = _lib.lib
    for Cin in (8, 16, 24, 30, 32, 64):
        for Cout in (1, 3, 8, 9, 16):
            for k in (1, 2, 3, 5, 7):
                for W in (0, 4, 28, 32, 36, 63, 64, 65, 128):
                    assert bool(lib.spk_readout_collapsed_supported(Cin, Cout, k, W)) == R.library_takes(Cin, Cout, k, W), (Cin, Cout, k, W)
                assert ops.readout_collapsed_supported(Cin, Cout, k) == R.wrapper_takes(64, Cin, Cout, k)


def test_mirror_constants_are_those_of_the_source():
    """RO_RB, the 64 KB limits, the k3 branch's conditions, its bands, the thread test and the four instances, read from the text."""
    src = open(SRC).read()
    assert int(re.search(r"constexpr\s+int\s+RO_RB\s*=\s*(\d+)\s*;", src).group(1)) == R.RO_RB
    lds = re.search(r"static size_t readout_lds_bytes\(int Cin, int Cout, int k, int W\)\s*\{\s*return (.*?);\s*\}", src, re.S).group(1)
    assert re.sub(r"\s+", "", lds) == "((size_t)(RO_RB+k-1)*W*(Cin+4)+(size_t)Cout*k*k*Cin)*sizeof(float)"
    sup = re.search(r"int spk_readout_collapsed_supported\(.*?\)\s*\{(.*?)\n\}", src, re.S).group(1)
    m = re.search(r"\(k & 1\) == 1 && \(Cin % (\d+)\) == 0 && readout_lds_bytes\(Cin, Cout, k, W > 0 \? W : (\d+)\) <= (\d+) \* (\d+)", sup)
    assert m and int(m.group(1)) == 8 and int(m.group(2)) == R.WRAPPER_W and int(m.group(3)) * int(m.group(4)) == R.LDS_LIMIT
    fwd = re.search(r"int spk_readout_collapsed_fwd\(.*?\n\}", src, re.S).group(0)
    m = re.search(r"if \(k == 3 && Cin == (\d+) && \(W % 4\) == 0 && W <= (\d+) && Cout <= (\d+)\)", fwd)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (R.K3_CIN, R.K3_W_MAX, R.K3_COUT_MAX)
    m = re.search(r"const bool r7 = \(H % (\d+)\) == 0;.*?const int rb = r7 \? (\d+) : (\d+);", fwd, re.S)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (R.K3_BANDS[0],) + R.K3_BANDS
    m = re.search(r"if \(\(W / 4\) \* rb \* 4 <= (\d+)\)", fwd)
    assert m and int(m.group(1)) == R.K3_THREADS
    m = re.search(r"const size_t lds3 = (.*?);", fwd)
    assert re.sub(r"\s+", "", m.group(1)) == "((size_t)(rb+2)*(W+2)*(32+4)+(size_t)Cout*9*32)*sizeof(float)"
    m = re.search(r"if \(lds3 <= (\d+) \* (\d+) &&", fwd)
    assert m and int(m.group(1)) * int(m.group(2)) == R.LDS_LIMIT
    inst = re.findall(r"(if \(r7 && W == 28\)|else if \(r7\)|else if \(W == 32\)|else) hipLaunchKernelGGL\(\(readout_collapsed_k3_kernel<(\d+), (\d+), (\d+)>\)", fwd)
    assert inst == [("if (r7 && W == 28)", "32", "7", "28"), ("else if (r7)", "32", "7", "0"), ("else if (W == 32)", "32", "8", "32"),
                    ("else", "32", "8", "0")]
    assert len(re.findall(r"dim3\(256\)", fwd)) == 5 and "if (pad != k / 2) return SPK_ERR_UNSUPPORTED;" in fwd
    # ops.readout_collapsed: the width it refuses above and the width-free predicate
    ops_src = open(os.path.join(ROOT, "spiking-diffusion_amd", "spkdiff", "ops.py")).read()
    assert f"if W > {R.WRAPPER_W} or not readout_collapsed_supported(Cin, Cout, k):" in ops_src


@pytest.mark.parametrize("v", VARIANTS, ids=R.vid)
def test_real_tier_is_unsaturated_and_the_fp32_reference_passes_its_own_bar(v):
    c = R.make_real(v)
    m, mag = R.oracle(c)
    share = float((m.abs() < 1.0).float().mean())
    assert share >= 0.5, share
    bound = R.fp32_bound(v.case.k, v.case.Cin, mag)
    ref32 = R.conv32(c)
    worst = float(((ref32.double() - m).abs() / bound).max())
    assert worst <= 1.0, worst
    R.readout_check(R.vid(v), ref32, R.u8_rule(ref32), m, bound)
    t32 = torch.tanh(ref32)
    R.readout_check(R.vid(v), t32, R.u8_rule(t32), torch.tanh(m), bound, 2.0 ** -23)      # (torch's fp32 tanh: within two ulp of [0.5, 1))
    # the bound is a round-off bound, not a tolerance: far below the values it guards
    assert float(bound.max()) < 1e-3 and float((bound / mag).max()) < 3e-5
    byte = R.u8_rule(t32)
    assert float(((byte > 0) & (byte < 255)).float().mean()) >= 0.25


def test_u8_rule_is_monotone_and_reaches_both_ends():
    pv = torch.linspace(-0.75, 0.75, 400001, dtype=torch.float32)
    b = R.u8_rule(pv).int()
    assert int(b.min()) == 0 and int(b.max()) == 255 and bool((b[1:] >= b[:-1]).all())
    assert sorted(set(b.tolist())) == list(range(256))
    edge = torch.tensor([-0.5, -0.49, 0.5, 0.4999, float("nan"), float("inf"), -float("inf"), 0.0], dtype=torch.float32)
    assert R.u8_rule(edge).tolist() == [0, 2, 255, 254, 0, 255, 0, 127]
    # the rule is fp32: (pv + 0.5f) and the product by 255.0f each round once
    pv = torch.rand(100000, generator=torch.Generator().manual_seed(3)) - 0.5
    a = (pv.double() + 0.5).float()                                             # (exact in fp64, rounded once)
    want = (a.double() * 255.0).float().floor().to(torch.uint8)                 # (exact in fp64, rounded once)
    assert torch.equal(R.u8_rule(pv), want)


def _wrong_answers(c):
    """Three wrong kernels on the host (fp64): the un-flipped taps under transposed=True, one zeroed edge column of x, one dropped
    input channel."""
    cs, k = c.v.case, c.v.case.k
    bt = 0.0 if c.bias is None else c.bias.double().view(1, -1, 1, 1) * R.coef_sum32(c.coef)
    w_t = R.as_layout(c.w_oihw, True)                                           # the ConvTranspose2d tensor of this correlation
    unflipped = F.conv2d(c.x.double(), w_t.transpose(0, 1).double(), None, 1, k // 2) + bt
    x_edge = c.x.clone()
    x_edge[..., cs.W - 1] = 0.0
    x_chan = c.x.clone()
    x_chan[:, cs.Cin - 1] = 0.0
    return {"unflipped": unflipped, "edge column": R.conv64(x_edge, c.w, k, c.v.tr) + bt,
            "dropped channel": R.conv64(x_chan, c.w, k, c.v.tr) + bt}


@pytest.mark.parametrize("v", K3_VARIANTS, ids=R.vid)
def test_the_comparison_rejects_three_wrong_kernels(v):
    """Every k3 case, both tiers: the exact tier's torch.equal and the real-valued tier's bound (with and without tanh, f32 and u8 rule)
    must fail on each wrong answer.  Counts, per wrong answer, the outputs that differ."""
    for narrow in (False, True):
        c = R.make_exact(v, narrow)
        m, _ = R.oracle(c)
        for name, wrong in _wrong_answers(c).items():
            assert not torch.equal(wrong.float(), m.float()), (name, "exact tier", narrow)
            with pytest.raises(AssertionError):
                R.readout_check(name, torch.tanh(wrong).float(), None, torch.tanh(m), torch.zeros_like(m), 2.0 ** -22)
    c = R.make_real(v)
    m, mag = R.oracle(c)
    bound = R.fp32_bound(v.case.k, v.case.Cin, mag)
    for name, wrong in _wrong_answers(c).items():
        with pytest.raises(AssertionError):
            R.readout_check(name, wrong.float(), None, m, bound)
        with pytest.raises(AssertionError):
            R.readout_check(name, torch.tanh(wrong).float(), None, torch.tanh(m), bound, 2.0 ** -22)


def test_argument_errors_need_no_device():
    """spk_readout_collapsed_fwd returns before any launch on: both outputs NULL (argument error); even k, Cin % 8 != 0, pad != k / 2
    (unsupported).  The pointers are host addresses that are never read."""
    from spkdiff import _lib
    fwd = _lib.lib.spk_readout_collapsed_fwd
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    ARG, UNSUP = -1, -2
    assert fwd(p, p, None, 1.0, None, None, 0, 1, 28, 28, 32, 1, 3, 1, 1, None) == ARG            # both outputs NULL
    assert fwd(p, p, None, 1.0, p, None, 0, 1, 28, 28, 32, 1, 4, 2, 1, None) == UNSUP              # even k
    assert fwd(p, p, None, 1.0, p, None, 0, 1, 28, 28, 30, 1, 3, 1, 1, None) == UNSUP              # Cin % 8 != 0
    assert fwd(p, p, None, 1.0, p, None, 0, 1, 28, 28, 32, 1, 3, 0, 1, None) == UNSUP              # pad != k / 2
    assert fwd(p, p, None, 1.0, p, None, 0, 1, 28, 28, 32, 1, 5, 1, 0, None) == UNSUP              # ... k 5 with pad 1
    assert fwd(p, p, None, 1.0, p, None, 0, 1, 28, 28, 32, 1, 3, -1, 1, None) == ARG               # negative pad
    assert fwd(p, p, None, 1.0, p, None, 0, 0, 28, 28, 32, 1, 3, 1, 1, None) == ARG                # B = 0
    for H, W, Cin, Cout, k, why in R.REFUSED:
        assert fwd(p, p, None, 1.0, p, None, 0, 1, H, W, Cin, Cout, k, k // 2, 1, None) == UNSUP, why
    with pytest.raises(NotImplementedError):
        _lib.check(UNSUP, "spk_readout_collapsed_fwd")


def test_chain_rows_name_the_form_of_their_image():
    forms = set()
    for h, w, C, form, D in R.CHAIN_ROWS:
        assert R.readout_form(4 * h, 4 * w, 32, C, 3) == form
        assert R.wrapper_takes(4 * w, 32, C, 3)
        forms.add(form)
    assert forms == set(R.FORMS) and {r[4] for r in R.CHAIN_ROWS} == {16, 32}
    geos = R.chain_geos(7, 7, 1)
    assert [O.geo_out_hw(g) for g in geos] == [(14, 14), (28, 28), (28, 28)]


@pytest.mark.parametrize("row", R.CHAIN_ROWS[2:5], ids=R.chain_id)
def test_chain_inputs_fire_and_leave_the_image_unsaturated(row):
    """The three smallest chains on the host (the GPU test asserts the same on all five): both LIF layers fire between 0.02 and 0.6 in
    the reset-state and in the carried run, the two runs differ, and at least half of the image's pre-activations have |m| < 1."""
    from oracle import snn_ref as ref
    h, w, C, _, _ = row
    p = R.chain_params(row)
    terms = [ref.bn_affine_terms({"b." + k: t for k, t in L.bn.items()}, "b") for L in p.layers[:2]]
    (m0, mag0, r0), (m1, mag1, r1) = R.chain_oracle(p, terms)
    assert all(0.02 <= r <= 0.6 for r in r0 + r1), (r0, r1)
    assert m0.shape == (R.CHAIN_B, C, 4 * h, 4 * w) and not torch.equal(m0, m1)
    assert float((m0.abs() < 1.0).float().mean()) >= 0.5 and float((m1.abs() < 1.0).float().mean()) >= 0.5
    assert float((R.fp32_bound(3, 32, mag0) / mag0).max()) < 3e-5
