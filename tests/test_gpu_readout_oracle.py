"""The collapsed read-out (spk_readout_collapsed_fwd, csrc/conv_mfma_gather.hip: the generic kernel and the four 3x3 instances) and the
decoder chain that ends in it, against the host oracle of tests/_readout_oracle.py.

Exact tier: dyadic inputs, ONE correct fp32 answer, torch.equal on every output and every byte.  Real-valued tier: collapsed spikes
and Gaussian weights with half of the pre-activations unsaturated, inside the derived first-order bound (fp32_bound).  Then the stores
(guarded buffers, each output alone), locality (one NaN, one image of a batch), and FusedSequential.run(final='memout') over the
reference decoder's three layers at five latent sizes, one per read-out form, with the launches each size takes."""
import time

import pytest
import torch

import _conv_bn_lif_oracle as O
import _readout_oracle as R
import test_gpu_conv_bn_lif_oracle as CBL          # TANHF_ERR_ALLOWED: measured and documented there
from oracle import snn_ref as ref
from parity_report import record as parity

pytestmark = pytest.mark.gpu

TANHF_ERR_ALLOWED = CBL.TANHF_ERR_ALLOWED
VARIANTS = R.variants()
GUARD = 256
F32_SENTINEL, U8_SENTINEL = 7777.0, 0xA5

EXACT = {"values": 0, "mismatches": 0, "tanhf_own_err": 0.0, "max_err_tanh": 0.0, "host_oracle_s": 0.0}
REAL = {"worst_err_over_bound": 0.0, "worst_case": "", "tanhf_own_err": 0.0, "unsaturated_share_min": 1.0}
FORMS = {}
_CASES = {}
_HOST_S = [0.0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def _case(v, tier):
    """The inputs of a variant and their oracle, computed once per session and left unchanged."""
    key = (v, tier)
    if key not in _CASES:
        t0 = time.perf_counter()
        c = R.make_real(v) if tier == "real" else R.make_exact(v, narrow=tier == "narrow")
        c.m, c.mag = R.oracle(c)
        _HOST_S[0] += time.perf_counter() - t0
        EXACT["host_oracle_s"] = round(_HOST_S[0], 2)
        _CASES[key] = c
    return _CASES[key]


def _lib_call(ops, x, w, bias, csum, out_f, out_u, apply_tanh, B, H, W, Cin, Cout, k, transposed):
    """The library entry itself; out_f / out_u: device addresses (or None)."""
    ops.check(ops.lib.spk_readout_collapsed_fwd(ops._p(x), ops._p(w), ops._p(bias), float(csum), out_f, out_u, int(apply_tanh), B, H, W,
                                                Cin, Cout, k, k // 2, int(transposed), ops._stream(x)), "spk_readout_collapsed_fwd")


def _run(ops, dev, c, apply_tanh, x=None):
    """The variant through ops.readout_collapsed, or through the library entry where the wrapper refuses the shape.  x: another input
    [B',Cin,H,W] in place of the case's."""
    cs = c.v.case
    xb = R.to_bhwc(c.x if x is None else x).to(dev)
    w = c.w.to(dev)
    bias = None if c.bias is None else c.bias.to(dev)
    if R.wrapper_takes(cs.W, cs.Cin, cs.Cout, cs.k):
        r = ops.readout_collapsed(xb, w, bias, c.coef, apply_tanh=apply_tanh, want_u8=True, k=cs.k, pad=cs.k // 2, transposed=c.v.tr)
        return r["f32"].cpu(), r["u8"].cpu()
    with pytest.raises(NotImplementedError):
        ops.readout_collapsed(xb, w, bias, c.coef, apply_tanh=apply_tanh, want_u8=True, k=cs.k, pad=cs.k // 2, transposed=c.v.tr)
    Bn = xb.shape[0]
    out_f = torch.empty((Bn, cs.Cout, cs.H, cs.W), dtype=torch.float32, device=dev)
    out_u = torch.empty((Bn, cs.Cout, cs.H, cs.W), dtype=torch.uint8, device=dev)
    _lib_call(ops, xb, w, bias, R.coef_sum32(c.coef), out_f.data_ptr(), out_u.data_ptr(), apply_tanh, Bn, cs.H, cs.W, cs.Cin, cs.Cout,
              cs.k, c.v.tr)
    return out_f.cpu(), out_u.cpu()


def _equal(what, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    n_bad = int(bad.sum())
    EXACT["values"] += want.numel()
    EXACT["mismatches"] += n_bad
    parity("readout_oracle_exact", **EXACT)
    assert n_bad == 0, (what, f"{n_bad} of {want.numel()} differ; first at", bad.nonzero()[:8].tolist())


# ================================================================================================ a. exact tier
@pytest.mark.parametrize("v", VARIANTS, ids=R.vid)
def test_exact_tier_every_output_and_byte_equal(dev, ops, v):
    """Wide (|w| <= 0.25: bytes saturate) and narrow (|w| <= 2^-6: a third of the bytes inside) dyadic inputs.  Without tanh f32 equals the
    oracle and u8 equals the fp32 u8 rule, nothing excluded; with tanh f32 is within tanhf's own measured error of fp64 tanh."""
    cs = v.case
    form = R.readout_form(cs.H, cs.W, cs.Cin, cs.Cout, cs.k)
    assert form == cs.form
    FORMS[R.vid(v)] = form
    parity("readout_oracle_forms", cases=FORMS, forms=sorted(set(FORMS.values())))
    for tier in ("wide", "narrow"):
        c = _case(v, tier)
        want = c.m.float()
        assert torch.equal(want.double(), c.m)
        f32, u8 = _run(ops, dev, c, False)
        _equal((R.vid(v), tier, "f32"), f32, want)
        _equal((R.vid(v), tier, "u8"), u8, R.u8_rule(want))
        tf, tu = _run(ops, dev, c, True)
        own = float((tf.double() - torch.tanh(f32.double())).abs().max())
        EXACT["tanhf_own_err"] = max(EXACT["tanhf_own_err"], own)
        e = R.readout_check((R.vid(v), tier, "tanh"), tf, tu, torch.tanh(c.m), torch.zeros_like(c.m), TANHF_ERR_ALLOWED)
        EXACT["max_err_tanh"] = max(EXACT["max_err_tanh"], e)
        parity("readout_oracle_exact", tanhf_err_allowed=TANHF_ERR_ALLOWED, **EXACT)
        assert own <= TANHF_ERR_ALLOWED


# ================================================================================================ b. real-valued tier
@pytest.mark.parametrize("v", VARIANTS, ids=R.vid)
def test_real_tier_within_the_derived_bound(dev, ops, v):
    """f32 within fp32_bound of the fp64 value (+ tanhf's error with tanh), bytes by readout_check's rule; at least half of the
    pre-activations unsaturated.  Measured on an MI355X: error / bound 0.001 - 0.007 for the 3x3 and 5x5 cases, 0.13 for k = 1 at
    Cin = 8 (eight terms: the bound has little slack there); tanhf's own error 7.95e-8.  Share of outputs with |m| < 1 (the same for both
    weight layouts; in brackets without bias):
        k3_r7_w28   28x28 0.936 (0.828)   7x28 Cout 8 0.733
        k3_r7       14x12 0.954 (0.918)   7x4 0.964   21x32 0.844
        k3_r8_w32   32x32 0.640 (0.644)   9x32 0.847
        k3_r8       20x12 0.747 (0.717)   5x28 0.818   1x4 0.750   1x8 1.000
        generic     28x28 Cout 9 0.696   9x30 0.856   6x36 0.947 (0.884)   6x64 0.829   k 1 0.829   k 5 0.944   Cin 24 0.867   1x9 0.978"""
    cs = v.case
    c = _case(v, "real")
    share = float((c.m.abs() < 1.0).float().mean())
    assert share >= 0.5, share
    bound = R.fp32_bound(cs.k, cs.Cin, c.mag)
    f32, u8 = _run(ops, dev, c, False)
    ratio = float(((f32.double() - c.m).abs() / bound.clamp_min(1e-300)).max())
    print(f"readout real {R.vid(v)}: err / bound {ratio:.3f}; |m| < 1 at {share:.3f} of the outputs")
    if ratio > REAL["worst_err_over_bound"]:
        REAL["worst_err_over_bound"], REAL["worst_case"] = ratio, R.vid(v)
    REAL["unsaturated_share_min"] = min(REAL["unsaturated_share_min"], share)
    parity("readout_oracle_real", **REAL)
    R.readout_check((R.vid(v), "real"), f32, u8, c.m, bound)
    tf, tu = _run(ops, dev, c, True)
    own = float((tf.double() - torch.tanh(f32.double())).abs().max())
    REAL["tanhf_own_err"] = max(REAL["tanhf_own_err"], own)
    parity("readout_oracle_real", **REAL)
    R.readout_check((R.vid(v), "real", "tanh"), tf, tu, torch.tanh(c.m), bound, TANHF_ERR_ALLOWED)
    assert own <= TANHF_ERR_ALLOWED


# ================================================================================================ c. stores stay inside the tensor
def _guarded(n, dtype, sentinel, dev):
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=dev)
    return buf, buf.data_ptr() + GUARD * buf.element_size()


def _guards_intact(buf, sentinel):
    b = buf.cpu()
    return bool((b[:GUARD] == sentinel).all()) and bool((b[-GUARD:] == sentinel).all())


@pytest.mark.parametrize("cs", R.EDGE_CASES, ids=lambda c: R.vid(R.Variant(c, c.tr[0], True)))
@pytest.mark.parametrize("apply_tanh", [False, True], ids=["raw", "tanh"])
def test_stores_stay_inside_the_tensor(dev, ops, cs, apply_tanh):
    """The library entry on f32 and u8 buffers with 256 sentinel elements on either side: both outputs, u8 alone (out_f32 = NULL) and f32
    alone.  The sentinels come back untouched and the payload equals the wrapper's result."""
    v = R.Variant(cs, cs.tr[0], True)
    c = _case(v, "narrow")
    want_f, want_u = _run(ops, dev, c, apply_tanh)
    xb, w, bias = R.to_bhwc(c.x).to(dev), c.w.to(dev), c.bias.to(dev)
    n = want_f.numel()
    for use_f, use_u in ((True, True), (False, True), (True, False)):
        bf, pf = _guarded(n, torch.float32, F32_SENTINEL, dev)
        bu, pu = _guarded(n, torch.uint8, U8_SENTINEL, dev)
        _lib_call(ops, xb, w, bias, R.coef_sum32(c.coef), pf if use_f else None, pu if use_u else None, apply_tanh, cs.B, cs.H, cs.W,
                  cs.Cin, cs.Cout, cs.k, v.tr)
        torch.cuda.synchronize()
        assert _guards_intact(bf, F32_SENTINEL) and _guards_intact(bu, U8_SENTINEL), (R.vid(v), use_f, use_u)
        pay_f, pay_u = bf[GUARD:-GUARD].cpu().view(want_f.shape), bu[GUARD:-GUARD].cpu().view(want_u.shape)
        assert torch.equal(pay_f, want_f if use_f else torch.full_like(want_f, F32_SENTINEL)), (R.vid(v), use_f, use_u)
        assert torch.equal(pay_u, want_u if use_u else torch.full_like(want_u, U8_SENTINEL)), (R.vid(v), use_f, use_u)


# ================================================================================================ d. locality
@pytest.mark.parametrize("cs", R.EDGE_CASES, ids=lambda c: R.vid(R.Variant(c, c.tr[0], True)))
def test_one_nan_reaches_its_neighbourhood_and_images_are_independent(dev, ops, cs):
    """One NaN in x: f32 is NaN and u8 is 0 on the k x k neighbourhood x every Cout of that image, and every other output is
    bit-identical to the clean run.  Image i of the batch equals the B = 1 call on image i."""
    v = R.Variant(cs, cs.tr[0], True)
    c = _case(v, "wide")
    f0, u0 = _run(ops, dev, c, False)
    assert torch.equal(f0, c.m.float())
    for b, y, x, ci in ((cs.B - 1, cs.H - 1, cs.W - 1, cs.Cin - 1), (0, cs.H // 2, cs.W // 2, 0), (0, min(cs.H - 1, 7), 0, 5)):
        xn = c.x.clone()
        xn[b, ci, y, x] = float("nan")
        f1, u1 = _run(ops, dev, c, False, x=xn)
        reach = R.nan_reach(cs, b, y, x)
        assert torch.equal(torch.isnan(f1), reach), (R.vid(v), (b, y, x, ci), int(torch.isnan(f1).sum()), int(reach.sum()))
        assert int(u1[reach].max()) == 0
        assert torch.equal(f1[~reach].view(torch.int32), f0[~reach].view(torch.int32)) and torch.equal(u1[~reach], u0[~reach])
    for i in range(cs.B if cs.B > 1 else 0):
        fi, ui = _run(ops, dev, c, False, x=c.x[i:i + 1])
        assert torch.equal(fi[0], f0[i]) and torch.equal(ui[0], u0[i]), (R.vid(v), "image", i)


# ================================================================================================ e. the decoder chain
_PACK_GATHER = ["pack_conv_weight_i8(transposed)", "bn_prepare"]
_FP6_TAIL = ["bn_prepare", "vae_fp6_pack(transposed)", "vae_fp6_fwd(out_kind=COLLAPSED, transposed)", "readout_collapsed(transposed)"]
_STATEFUL = _PACK_GATHER + ["conv_mfma_fused(mode=LIF, transposed, v)"] + _PACK_GATHER + \
    ["conv_mfma_fused(mode=LIF, transposed, collapse_coef, v)", "readout_collapsed(transposed)"]
_ALL_GATHER = _PACK_GATHER + ["conv_mfma_fused(mode=LIF, transposed)"] + _PACK_GATHER + \
    ["conv_mfma_fused(mode=LIF, transposed, collapse_coef)", "readout_collapsed(transposed)"]


def _build_net(p):
    from spikingjelly.activation_based import functional, layer, neuron
    from spkdiff.fused import FusedSequential
    mods, bns = [], []
    for L in p.layers:
        Cin, Cout, k, s, pd, _, op = L.geo[:7]
        conv = layer.ConvTranspose2d(Cin, Cout, k, s, pd, op)
        with torch.no_grad():
            conv.weight.copy_(L.w); conv.bias.copy_(L.bias)
        mods.append(conv)
        if L.bn is not None:
            bn = layer.BatchNorm2d(Cout)
            with torch.no_grad():
                for name, val in L.bn.items():
                    getattr(bn, name).copy_(val)
            mods += [bn, neuron.LIFNode()]
            bns.append(bn)
    net = FusedSequential(*mods)
    functional.set_step_mode(net, "m")
    return net.eval(), bns


def _memout(net, ptc, coef, stateful):
    from spkdiff.ops import IN_PTC
    return net.run(ptc, IN_PTC, final="memout", coef=coef, apply_tanh=True, want_u8=True, stateful=stateful)


def _recorded_launches(monkeypatch, p):
    """The launches of a stateless and of a stateful call, logged on a CPU twin of the network by the dispatch recorders (no kernel
    runs; the real wrappers are back before this returns)."""
    from _dispatch_recorders import _install_recorders, _u8
    log = _install_recorders(monkeypatch)
    out = []
    try:
        with torch.no_grad():
            for stateful in (False, True):
                twin, _ = _build_net(p)                  # (a fresh one: the first call of a network packs its weights)
                del log[:]
                _memout(twin, _u8(R.CHAIN_B, p.h, p.w, 16, p.D), p.coef, stateful)
                out.append(list(log))
    finally:
        monkeypatch.undo()
    return out


# (latent h, w, channels) -> the launches of the stateless call: the fp6 kernels where the stride-2 layers have an instance (at 32
# latent channels only the second has one: the gather kernel writes the S32 records it reads)
_FP6_CHAIN = _PACK_GATHER + ["ptc_to_s32", "vae_fp6_pack(transposed)", "vae_fp6_fwd(out_kind=S32, transposed)"] + _FP6_TAIL
CHAIN_LAUNCHES = {
    (7, 7, 16): _FP6_CHAIN,
    (8, 8, 16): _FP6_CHAIN,
    (5, 3, 16): _ALL_GATHER,
    (7, 4, 16): _ALL_GATHER,
    (4, 9, 16): _ALL_GATHER,
    (7, 7, 32): _PACK_GATHER + ["conv_mfma_fused(mode=LIF, transposed, out_s32)"] + _FP6_TAIL,
}


@pytest.mark.parametrize("row", R.CHAIN_ROWS, ids=R.chain_id)
def test_decoder_chain_memout_against_the_chained_oracle(dev, ops, monkeypatch, row):
    """ConvT(16->64, s2) + BN + LIF, ConvT(64->32, s2) + BN + LIF, ConvT(32->C, s1) through FusedSequential.run(final='memout'): the
    image within the read-out bound + tanhf's error of tanh64 of the fp64 read-out of collapse32(the oracle's second-layer spikes), bytes
    by the u8 rule; stateless, stateful from the reset state (the same image), and a second stateful call on carried potentials."""
    from spikingjelly.activation_based import functional
    h, w, C, form, D = row
    assert R.readout_form(4 * h, 4 * w, 32, C, 3) == form
    p = R.chain_params(row)
    stateless, stateful = _recorded_launches(monkeypatch, p)
    assert stateless == CHAIN_LAUNCHES[(h, w, D)], stateless
    assert stateful == _STATEFUL, stateful
    net, bns = _build_net(p)
    terms = []
    for bn in bns:
        sd = {"b." + k: t.detach().clone() for k, t in bn.state_dict().items() if t.dtype == torch.float32}
        terms.append(ref.bn_affine_terms(sd, "b"))
    t0 = time.perf_counter()
    want = R.chain_oracle(p, terms)
    host_s = time.perf_counter() - t0
    for m, mag, rates in want:
        assert all(0.02 <= r <= 0.6 for r in rates), rates
    net = net.to(dev)
    for (a, b), bn in zip(terms, bns):
        ga, gb = ops.bn_prepare(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        assert torch.equal(ga.cpu(), a) and torch.equal(gb.cpu(), b), "ops.bn_prepare differs from ref.bn_affine_terms"
    coef = p.coef.to(dev)
    ptc = [O.to_ptc(x).to(dev) for x in p.xs]
    worst = 0.0

    def check(what, r, m, mag):
        bound = R.fp32_bound(3, 32, mag)
        f32, u8 = r["f32"].cpu(), r["u8"].cpu()
        assert f32.shape == (R.CHAIN_B, C, 4 * h, 4 * w)
        R.readout_check((what, row), f32, u8, torch.tanh(m), bound, TANHF_ERR_ALLOWED)
        return float(((f32.double() - torch.tanh(m)).abs() / (bound + TANHF_ERR_ALLOWED)).max())

    with torch.inference_mode():
        r0 = _memout(net, ptc[0], coef, False)
        worst = max(worst, check("stateless", r0, want[0][0], want[0][1]))
        functional.reset_net(net)
        r1 = _memout(net, ptc[0], coef, True)
        assert torch.equal(r1["f32"], r0["f32"]) and torch.equal(r1["u8"], r0["u8"]), "stateful from the reset state != stateless"
        r2 = _memout(net, ptc[1], coef, True)
        worst = max(worst, check("carried", r2, want[1][0], want[1][1]))
        functional.reset_net(net)
    share = float((want[0][0].abs() < 1.0).float().mean())
    parity(f"readout_oracle_chain_{h}x{w}_d{D}_c{C}", form=form, worst_err_over_tol=worst, rates=[round(r, 3) for r in want[0][2] + want[1][2]],
           unsaturated_share=round(share, 3), host_oracle_s=round(host_s, 2))
