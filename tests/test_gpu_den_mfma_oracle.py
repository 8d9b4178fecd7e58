"""The denoiser's 3x3 matrix-core kernels against an EXACT host oracle on FULL-WIDTH weights (tests/_conv_bn_lif_oracle.py,
make_case(weights="full")): csrc/den_mfma.hip (four int8 digit planes: LIF, carried state, MODE_MEAN, and the time-collapsed counts
form), csrc/den_mfma_fp6.hip (six fp6 planes: LIF, carried state, RAW) and csrc/den_mfma_fp6v2.hip (the sampler's kernel: certified
decisions, the exact repair tail, last-position launches, the half-image, listed and row-band forms).

Every weight is exact in the kernels' per-channel fixed point with ALL digits in play, every fp64 partial sum is exact in any order, and a
quarter of the output channels hold a neuron whose charged potential of step 0 is exactly 1.0 (a further eighth: the largest fp32 below
it), so the contract of DESIGN.md §2 -- exact dot product + bias -> one rounding to fp32 -> fmaf(y, a, b) -> fp32 LIF -- has ONE answer
per neuron: every spike, spike count, carried potential, RAW pre-activation and counts-form logit below is compared bit for bit, nothing
excluded.  Two read-outs carry the error bound of their fp32 evaluation (readout_bound): MODE_MEAN of the per-step int8 kernel, whose
epilogue adds sixteen rounded fp32 values, and -- besides its bit-equality with the counts oracle -- the logits of spk_den_step_tail.

Inputs are built and outputs decoded by the host builders of the oracle module, never by the device converters; those are compared with
the host builders once, in both directions (test_device_layout_converters_equal_the_host_builders)."""
import time

import pytest
import torch

import _conv_bn_lif_oracle as O
from oracle import snn_ref as ref
from parity_report import record as parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


FLAG_LIST = 1 << 20          # id-list entries of a certified kernel's workspace: [count, published count, ids..., bitmap, ticket]
STATS = {}                   # family -> [values compared, mismatches, host oracle seconds]
FLAGGED = {}                 # fp6v2: row -> {(form, cap): neurons the call flagged}
_ORACLE = {}


def _rid(r):
    return "-".join("cus" if v is None else str(int(v)) for v in r)


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _report(fam):
    st = STATS.setdefault(fam, [0, 0, 0.0])
    extra = {}
    if fam == "fp6v2":
        extra["flagged"] = sum(n for d in FLAGGED.values() for n in d.values())
        extra["flagged_per_row"] = {k: [min(d.values()), max(d.values())] for k, d in FLAGGED.items()}
    parity(f"den_oracle_{fam}", values=st[0], mismatches=st[1], host_oracle_s=round(st[2], 2), **extra)


def _tally(fam, got, want, what):
    """torch.equal with the mismatch pattern in the message; counts into the family's parity record."""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    bad = got != want
    n_bad = int(bad.sum())
    st = STATS.setdefault(fam, [0, 0, 0.0])
    st[0] += want.numel()
    st[1] += n_bad
    _report(fam)
    assert n_bad == 0, (what, f"{n_bad} of {want.numel()} differ; first at", bad.nonzero()[:8].tolist())


def _oracle(fam, row, carried=False):
    """The full-width case of a row and its oracle results, computed once per session and left unchanged: the reset-state run on input
    0 and (carried=True) the carried-state pair v0 -> input 0 -> v1 -> input 1 -> v2."""
    row = O.den_row(row, _cus())
    geo = O.den_geo(row)
    t0 = time.perf_counter()
    if geo not in _ORACLE:
        c = O.make_case(geo, O.full_seed(geo), weights="full", n_inputs=2)
        c.y0 = O.conv_fp32(c.xs[0], c.w, c.bias, geo)                        # MODE_RAW
        c.pre0 = O.bn32(c.y0, c.a, c.b)
        if fam != "counts":                                                  # (the counts rows use the convolution alone)
            c.s, c.v = ref.lif_multi_step(c.pre0)
            c.bits = O.spikes_to_bits(c.s)
            c.cnt = O.to_counts(c.s)
        _ORACLE[geo] = c
    c = _ORACLE[geo]
    c.row = row                                                              # (two families may share a geometry, not the input split)
    if carried and not hasattr(c, "s2"):
        c.s1, c.v1 = ref.lif_multi_step(c.pre0, c.v0.clone())
        pre1 = O.bn32(O.conv_fp32(c.xs[1], c.w, c.bias, geo), c.a, c.b)
        c.s2, c.v2 = ref.lif_multi_step(pre1, c.v1.clone())
    STATS.setdefault(fam, [0, 0, 0.0])[2] += time.perf_counter() - t0
    return c


def _u8(t):
    return t.view(torch.uint8) if t.dtype == torch.int8 else t


def _split(x, C0):
    """The two concatenated inputs of a row: channels [0, C0) and, if any, the rest."""
    return x[:, :, :C0].contiguous(), (x[:, :, C0:].contiguous() if x.shape[2] > C0 else None)


def _graze_check(c, spikes, what, n_img=None):
    """The constructed neurons by name (bit-equality implies it; this names the neuron): h == 1.0 fires at step 0, the largest fp32
    below does not."""
    for kind, ch, b, y, x in c.graze:
        if n_img is not None and b >= n_img:
            continue
        assert float(spikes[0, b, ch, y, x]) == (1.0 if kind == "fire" else 0.0), (what, kind, "channel", ch, "image", b, "at", (y, x))


def _readout_check(what, got, want64, bound):
    err = (got.double() - want64).abs()
    worst = float((err - bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, bound up to {float(bound.max()):.3e}")
    assert worst <= 0.0, (what, "exceeds the read-out bound by", worst, "max err", float(err.max()), "at", int((err - bound).argmax()))
    return float(err.max())


def _n_active(dev, B, n):
    """The device-side image count of the wrappers' active_set: (slot -> image list, [count, work word])."""
    return torch.arange(B, dtype=torch.int32, device=dev), torch.tensor([n, 0], dtype=torch.int32, device=dev)


# ================================================================================================ layouts
def test_device_layout_converters_equal_the_host_builders(dev, ops):
    """The converters the rest of the suite trusts on both sides of every comparison, against the plain-torch builders, both directions,
    on one ragged shape (15 positions, 3 images, 128 channels)."""
    g = torch.Generator().manual_seed(21)
    s = (torch.rand(16, 3, 128, 5, 3, generator=g) < 0.3).float()
    sd = s.to(dev)
    bits = O.spikes_to_bits(s)
    n = 0
    for chunk in (None, 32):
        host = O.to_ptc(s, chunk)
        assert torch.equal(ops.spikes_to_ptc(sd, chunk=chunk).cpu(), host)
        assert torch.equal(ops.ptc_to_spikes(host.to(dev)).cpu(), s)
        n += 2 * s.numel()
    for rec, to_dev, from_dev in ((64, ops.spikes_to_c4, ops.c4_to_spikes), (32, ops.spikes_to_s32, ops.s32_to_spikes)):
        host = O.bits_to_packed(bits, rec)
        got = to_dev(sd)
        assert got.dtype == ops.C4_DTYPE and torch.equal(_u8(got).cpu(), host)
        assert torch.equal(from_dev(host.view(torch.int8).to(dev)).cpu(), s)
        assert torch.equal(O.packed_to_spikes(host), s)
        n += 2 * s.numel()
    parity("den_oracle_layout_converters", values=n, mismatches=0)


# ================================================================================================ a. int8 digit planes
def _i8_in(ops, dev, c, i=0):
    C0 = c.row[0]
    x0, x1 = _split(c.xs[i], C0)
    return O.to_ptc(x0, 32).to(dev), None if x1 is None else O.to_ptc(x1, 32).to(dev)


@pytest.mark.parametrize("row", O.DEN_I8_ROWS, ids=_rid)
def test_int8_kernel_lif_from_reset_carried_state_and_counts(dev, ops, row):
    """spk_den_conv3x3_mfma, MODE_LIF: CPTC spikes and spike counts from the reset state, then v carried over two calls on different
    inputs from a non-zero v0 -- spikes and the returned v bit-equal after each."""
    c = _oracle("i8", row, carried=True)
    Cout, B = c.geo[1], c.geo[9]
    if row[5] is None:
        assert B * (Cout // 16) > _cus(), "one trip of the persistent grid takes every item"
    pk = ops.den_pack_weight_i8(c.w.to(dev), c.bias.to(dev))
    a, b = c.a.to(dev), c.b.to(dev)
    in0, in1 = _i8_in(ops, dev, c, 0)
    out, cnt = ops.den_conv3x3_mfma(in0, pk, Cout, mode=ops.MODE_LIF, in1=in1, bn_a=a, bn_b=b, want_counts=True)
    got = O.from_cptc(out.cpu())
    _graze_check(c, got, ("i8", row))
    _tally("i8", out.cpu(), O.to_ptc(c.s, 32), ("i8 spikes", row))
    _tally("i8", cnt.cpu(), c.cnt, ("i8 counts", row))
    v = c.v0.to(dev).clone()
    out1 = ops.den_conv3x3_mfma(in0, pk, Cout, mode=ops.MODE_LIF, in1=in1, bn_a=a, bn_b=b, v=v)
    _tally("i8", out1.cpu(), O.to_ptc(c.s1, 32), ("i8 call 1 spikes", row))
    _tally("i8", v.cpu(), c.v1, ("i8 call 1 v", row))
    in0b, in1b = _i8_in(ops, dev, c, 1)
    out2 = ops.den_conv3x3_mfma(in0b, pk, Cout, mode=ops.MODE_LIF, in1=in1b, bn_a=a, bn_b=b, v=v)
    _tally("i8", out2.cpu(), O.to_ptc(c.s2, 32), ("i8 call 2 spikes", row))
    _tally("i8", v.cpu(), c.v2, ("i8 call 2 v", row))
    assert 0.02 <= float(c.s.mean()) <= 0.6


def test_int8_kernel_time_mean_within_the_fp32_evaluation_bound(dev, ops):
    """MODE_MEAN of the per-step kernel.  Its epilogue (den_mfma.hip: `msum = msum + x[r]` over the sixteen pre-activations, each already
    rounded to fp32, then `/ 16.0f`) adds sixteen rounded fp32 values in fp32: it does NOT round once, so the comparison with the fp64
    mean of the oracle's per-step outputs carries readout_bound (the counts form, which does round once, is compared bit for bit)."""
    row = O.DEN_I8_MEAN_ROW
    c = _oracle("i8", row)
    in0, in1 = _i8_in(ops, dev, c, 0)
    pk = ops.den_pack_weight_i8(c.w.to(dev), c.bias.to(dev))
    got = ops.den_conv3x3_mfma(in0, pk, c.geo[1], mode=ops.MODE_MEAN, in1=in1).cpu()
    mean, mag = O.mean64(c.y0)
    err = _readout_check(("i8 mean", row), got, mean, O.readout_bound(16, mag))
    parity("den_oracle_i8_mean", max_err=err, bound_max=float(O.readout_bound(16, mag).max()))


# ================================================================================================ b. the counts form
def _counts_in(ops, dev, c):
    C0 = c.row[0]
    x0, x1 = _split(c.xs[0], C0)
    return O.to_counts(x0).to(dev), None if x1 is None else O.to_counts(x1).to(dev)


@pytest.mark.parametrize("row", O.DEN_COUNTS_ROWS, ids=_rid)
def test_counts_form_logits_bit_equal(dev, ops, row):
    """spk_den_conv3x3_counts_mfma on the spike counts of random spike trains: fp32(sum_t dot + T * bias) / T, rounded once -- bit-equal
    to the oracle on both kernels (K chunks split over the waves / LDS-shared) and through the zero-padded packing."""
    c = _oracle("counts", row)
    Cout, H, W, B = c.geo[1], c.geo[7], c.geo[8], c.geo[9]
    shared = B * H * W > 32 * 160 and 43 <= H * W <= 64
    assert shared == (row in O.DEN_COUNTS_ROWS[2:4]), "the row does not reach the kernel its comment names"
    cnt0, cnt1 = _counts_in(ops, dev, c)
    pk = ops.den_pack_weight_i8(c.w.to(dev), c.bias.to(dev), pad_cout=bool(Cout % 16))
    assert pk[1].numel() == (Cout + 15) // 16 * 16
    got = ops.den_conv3x3_counts(cnt0, pk, Cout, 16, cnt1=cnt1)
    t0 = time.perf_counter()
    want, _ = O.counts_logits(c.xs[0].sum(0), c.w, c.bias, c.geo)
    STATS["counts"][2] += time.perf_counter() - t0
    _tally("counts", got.cpu(), want, ("counts logits", row))
    assert float(want.abs().max()) > 0.1


def test_step_tail_logits(dev, ops):
    """The logits of spk_den_step_tail (its own copy of the counts epilogue: fma(s, scale, bias * T) rounded once, times 1 / T) within
    readout_bound of the fp64 mean of the per-step outputs, and bit-equal to the counts oracle."""
    row = O.STEP_TAIL_ROW
    c = _oracle("counts", row)
    K, H, W, B = c.geo[1], c.geo[7], c.geo[8], c.geo[9]
    cnt5, cnt1 = _counts_in(ops, dev, c)
    pk = ops.den_pack_weight_i8(c.w.to(dev), c.bias.to(dev), pad_cout=True)
    g = torch.Generator().manual_seed(5)
    x_t = torch.full((B, 1, H, W), K, dtype=torch.int64, device=dev)
    un = torch.zeros((B, 1, H, W), dtype=torch.bool, device=dev)
    u = torch.rand(B * H * W, generator=g).to(dev)
    q = torch.empty(B * H * W, K).exponential_(1, generator=g).to(dev)
    _, lg = ops.den_step_tail(cnt5, cnt1, pk, x_t, un, 5, 1.0, T=16, K=K, u=u, q=q, want_logits=True)
    want, want64 = O.counts_logits(c.xs[0].sum(0), c.w, c.bias, c.geo)
    mean, mag = O.mean64(c.y0)
    err = _readout_check(("step tail logits", row), lg.cpu(), mean, O.readout_bound(16, mag))
    parity("den_oracle_step_tail_logits", max_err_vs_per_step_mean=err)
    _tally("counts", lg.cpu(), want, ("step tail logits", row))
    assert int(x_t.max()) <= K and int((x_t < K).sum()) > 0, "the token update ran"


# ================================================================================================ c. six fp6 planes
def _c4(dev, x):
    return O.bits_to_packed(O.spikes_to_bits(x), 64).view(torch.int8).to(dev)


@pytest.mark.parametrize("row", O.DEN_FP6_ROWS, ids=_rid)
def test_fp6_kernel_lif_carried_state_counts_and_raw(dev, ops, row):
    """spk_den_conv3x3_mfma_fp6: C4 records and spike counts from the reset state, v carried over two calls with the returned v compared
    exactly (the last position of an odd map comes from the last-position kernel), and spk_den_conv3x3_fp6_raw == the convolution
    rounded once."""
    c = _oracle("fp6", row, carried=True)
    Cin, Cout, H, W, B = c.geo[0], c.geo[1], c.geo[7], c.geo[8], c.geo[9]
    assert ops.den_fp6_supported(Cout, Cin, 3, 1, 1, 16, H, W), row
    if row[5] is None:
        assert B * (Cout // 16) > _cus()
    pk = ops.den_pack_weight_fp6(c.w.to(dev), c.bias.to(dev))
    a, b = c.a.to(dev), c.b.to(dev)
    in0 = _c4(dev, c.xs[0])
    out, cnt = ops.den_conv3x3_mfma_fp6(in0, pk, Cout, bn_a=a, bn_b=b, want_counts=True)
    assert out.dtype == ops.C4_DTYPE
    _graze_check(c, O.packed_to_spikes(_u8(out).cpu()), ("fp6", row))
    _tally("fp6", _u8(out).cpu(), O.bits_to_packed(c.bits, 64), ("fp6 records", row))
    _tally("fp6", cnt.cpu(), c.cnt, ("fp6 counts", row))
    raw = ops.den_conv3x3_fp6_raw(in0, pk, Cout)
    _tally("fp6", raw.cpu().contiguous(), c.y0, ("fp6 raw", row))
    v = c.v0.to(dev).clone()
    out1 = ops.den_conv3x3_mfma_fp6(in0, pk, Cout, bn_a=a, bn_b=b, v=v)
    _tally("fp6", _u8(out1).cpu(), O.bits_to_packed(O.spikes_to_bits(c.s1), 64), ("fp6 call 1 records", row))
    _tally("fp6", v.cpu(), c.v1, ("fp6 call 1 v", row))
    out2 = ops.den_conv3x3_mfma_fp6(_c4(dev, c.xs[1]), pk, Cout, bn_a=a, bn_b=b, v=v)
    _tally("fp6", _u8(out2).cpu(), O.bits_to_packed(O.spikes_to_bits(c.s2), 64), ("fp6 call 2 records", row))
    _tally("fp6", v.cpu(), c.v2, ("fp6 call 2 v", row))
    assert 0.02 <= float(c.s.mean()) <= 0.6


def test_fp6_kernel_refuses_the_map_its_lds_cannot_hold(dev, ops):
    """7x8 (56 positions) would be the fullest seven-tile item, but its two zero-bordered LDS images and weight slabs take 167 936 B of
    the 163 840 B a workgroup may have: the support predicate says no and the launcher returns an error instead of launching."""
    C0, _, Cout, H, W, B = O.DEN_FP6_REFUSED
    assert not ops.den_fp6_supported(Cout, C0, 3, 1, 1, 16, H, W)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(16, B, C0, H, W, generator=g) < 0.1).float()
    pk = ops.den_pack_weight_fp6(torch.rand(Cout, C0, 3, 3, generator=g).to(dev) - 0.5, None)
    ones = torch.ones(Cout, device=dev)
    with pytest.raises(NotImplementedError, match="spk_den_conv3x3_mfma_fp6"):
        ops.den_conv3x3_mfma_fp6(_c4(dev, x), pk, Cout, bn_a=ones, bn_b=ones)


# ================================================================================================ d. fp6v2
def _s32(dev, x):
    return O.bits_to_packed(O.spikes_to_bits(x), 32).view(torch.int8).to(dev)


def _flag_ws(ops, dev, B, Cout, H, W):
    from spkdiff._lib import lib
    return ops._flag_bitmap(dev, lib.spk_den_fp6v2_flag_words(B, Cout, H, W))


def _flag_ws_clean(v):
    """The flag_ws_clean rule of tests/test_gpu_parity.py: live counter zero, overflow bitmap and hand-over ticket zero."""
    return int(v[0]) == 0 and int(v[2 + FLAG_LIST:].abs().sum()) == 0


def _graze_outside_tail(c, n_img=None, listed=None):
    """Constructed neurons the MAIN launch decides (the tail computes the last position of a 7x7 map itself): each must be flagged."""
    H, W = c.geo[7], c.geo[8]
    n = 0
    for kind, ch, b, y, x in c.graze:
        p = y * W + x
        if (H * W) % 2 and p == H * W - 1:
            continue
        if n_img is not None and b >= n_img:
            continue
        if listed is not None and not bool(listed[b, p]):
            continue
        n += 1
    return n


class _settings:
    """ops.FLAG_CAP / ops.FP6V2_FORM for one call, restored afterwards."""

    def __init__(self, ops, cap, form):
        self.ops, self.cap, self.form = ops, cap, form

    def __enter__(self):
        self.prev = (self.ops.FLAG_CAP, self.ops.FP6V2_FORM)
        self.ops.FLAG_CAP, self.ops.FP6V2_FORM = self.cap, self.form

    def __exit__(self, *exc):
        self.ops.FLAG_CAP, self.ops.FP6V2_FORM = self.prev
        return False


# (row, form): the automatic form and the whole-image form; the row bands of an 8x8 map have one form
FP6V2_CASES = [(r, f) for r in O.DEN_FP6V2_ROWS for f in (0, 1) if not (r[3:5] == (8, 8) and f == 1)]


@pytest.mark.parametrize("cap", [-1, 64, 0])
@pytest.mark.parametrize("row,form", FP6V2_CASES, ids=[f"{_rid(r)}-form{f}" for r, f in FP6V2_CASES])
def test_fp6v2_kernel_spikes_counts_flags_and_workspace(dev, ops, row, form, cap):
    """spk_den_conv3x3_mfma_fp6v2 under the automatic form (0: these batches take the half-image kernel on a 7x7 map wherever
    B * Cout / 32 * 2 <= the grid) and the whole-image form (1), with the whole id list (-1), 64 entries and none (the overflow bitmap):
    S32 records and spike counts equal the oracle; the call flagged at least the constructed threshold-grazing neurons (so the
    certification and the exact repair were entered); the workspace comes back clean."""
    c = _oracle("fp6v2", row)
    Cin, Cout, H, W, B = c.geo[0], c.geo[1], c.geo[7], c.geo[8], c.geo[9]
    assert ops.den_fp6v2_supported(Cout, Cin, 3, 1, 1, 16, H, W)
    pk = ops.den_pack_weight_fp6v2(c.w.to(dev), c.bias.to(dev))
    in0 = _s32(dev, c.xs[0])
    with _settings(ops, cap, form):
        out, cnt = ops.den_conv3x3_mfma_fp6v2(in0, pk, Cout, bn_a=c.a.to(dev), bn_b=c.b.to(dev), want_counts=True)
    torch.cuda.synchronize()
    ws = _flag_ws(ops, dev, B, Cout, H, W).cpu()
    flagged = int(ws[1])
    FLAGGED.setdefault(_rid(row), {})[(form, cap)] = flagged
    _graze_check(c, O.packed_to_spikes(_u8(out).cpu()), ("fp6v2", row, form, cap))
    _tally("fp6v2", _u8(out).cpu(), O.bits_to_packed(c.bits, 32), ("fp6v2 records", row, form, cap))
    _tally("fp6v2", cnt.cpu(), c.cnt, ("fp6v2 counts", row, form, cap))
    need = _graze_outside_tail(c)
    assert need >= 1 and flagged >= need, (row, form, cap, "flagged", flagged, "constructed neurons outside the tail's positions", need)
    assert _flag_ws_clean(ws), "live counter, overflow bitmap and hand-over ticket come back clean"
    print(f"fp6v2 {row} form {form} cap {cap}: flagged {flagged} of {B * Cout * H * W} neurons (constructed: {need})")


def _listed_call(ops, dev, c, in0, pk, out, cnt, act, need, radius, cap):
    """spk_den_conv3x3_mfma_fp6v2_listed into caller-owned (prefilled) buffers: the wrapper allocates its own."""
    from spkdiff._lib import lib
    Cout, H, W, B = c.geo[1], c.geo[7], c.geo[8], c.geo[9]
    wq, scale, bias_d, wl1, qtab = pk
    flags = _flag_ws(ops, dev, B, Cout, H, W)
    a, b = c.a.to(dev), c.b.to(dev)
    p = ops._p
    rc = lib.spk_den_conv3x3_mfma_fp6v2_listed(p(in0), in0.shape[1], p(wq), p(scale), p(bias_d), p(wl1), p(qtab), p(a), p(b), p(out),
                                               p(cnt), p(flags), 16, B, H, W, Cout, act[1].data_ptr(), p(need.buf), need.radii,
                                               int(radius), int(cap), ops._stream(in0))
    torch.cuda.synchronize()
    return rc, flags


@pytest.mark.parametrize("cap", [-1, 64, 0])
def test_fp6v2_listed_launch_against_the_oracle(dev, ops, cap):
    """conv3x3_fp6v2_listed_kernel through ops.active_set(..., need=NeedLists): every listed position and the 49th of every active slot
    equal the oracle (records and counts); a second call into prefilled buffers leaves every other byte untouched."""
    row = O.DEN_LISTED_ROW
    c = _oracle("fp6v2", row)
    Cout, H, W, B = c.geo[1], c.geo[7], c.geo[8], c.geo[9]
    t, radius = 2, 1
    # the step changes (u < 1 / t on a masked position) the positions of the first eight constructed neurons below position 48, so that
    # the lists of radius 1 hold them, and position 0 of every image that has none: every image is active, slot s is image s
    unmasked = torch.ones(B, 1, 7, 7, dtype=torch.bool)
    for kind, ch, b, y, x in [gz for gz in c.graze if gz[3] * 7 + gz[4] < 48][:8]:
        unmasked[b, 0, y, x] = False
    for b in range(B):
        if bool(unmasked[b].all()):
            unmasked[b, 0, 0, 0] = False
    u = unmasked.float()                                          # 0 where a change is wanted, 1 elsewhere
    um, ud = unmasked.to(dev), u.to(dev)
    act = ops.select_active(um, t, ud)
    need = ops.select_needed(um, t, act, ops.NeedLists(B, 4, dev), ud)
    n_act = int(act[1][0].item())
    assert n_act == B and act[0].cpu().tolist() == list(range(B))
    rec = need.records(radius).cpu().numpy()
    listed = torch.zeros(B, 49, dtype=torch.bool)
    for s in range(n_act):
        listed[s, rec[s, :rec[s, 48]].tolist()] = True
        listed[s, 48] = True
    assert 0 < int(listed[:n_act, :48].sum()) < n_act * 48, "the lists are neither empty nor everything"
    pk = ops.den_pack_weight_fp6v2(c.w.to(dev), c.bias.to(dev))
    in0 = _s32(dev, c.xs[0])
    want = O.bits_to_packed(c.bits, 32).view(B, Cout // 32, 49, 16, 16)
    want_c = c.cnt.view(B, Cout // 32, 49, 32)
    m = listed[:, None, :, None, None].expand_as(want)
    mc = listed[:, None, :, None].expand_as(want_c)
    with _settings(ops, cap, 0), ops.active_set(*act, need=need):
        out, cnt = ops.den_conv3x3_mfma_fp6v2(in0, pk, Cout, bn_a=c.a.to(dev), bn_b=c.b.to(dev), want_counts=True, need_radius=radius)
    torch.cuda.synchronize()
    _tally("fp6v2", _u8(out).cpu().view(want.shape)[m], want[m], ("listed records", cap))
    _tally("fp6v2", cnt.cpu().view(want_c.shape)[mc], want_c[mc], ("listed counts", cap))
    # ... and the launch itself into prefilled buffers (rc 0: the listed kernel ran, not the wrapper's unlisted stand-in)
    out2 = torch.full((B, Cout // 32, 7, 7, 16, 16), 0x11, dtype=torch.int8, device=dev)
    cnt2 = torch.full((B, Cout // 32, 7, 7, 32), 0xEE, dtype=torch.uint8, device=dev)
    rc, flags = _listed_call(ops, dev, c, in0, pk, out2, cnt2, act, need, radius, cap)
    assert rc == 0, f"spk_den_conv3x3_mfma_fp6v2_listed returned {rc}"
    ws = flags.cpu()
    o2, c2 = _u8(out2).cpu().view(want.shape), cnt2.cpu().view(want_c.shape)
    _tally("fp6v2", o2[m], want[m], ("listed records, prefilled", cap))
    _tally("fp6v2", c2[mc], want_c[mc], ("listed counts, prefilled", cap))
    _tally("fp6v2", o2[~m], torch.full_like(o2[~m], 0x11), ("unlisted record bytes untouched", cap))
    _tally("fp6v2", c2[~mc], torch.full_like(c2[~mc], 0xEE), ("unlisted count bytes untouched", cap))
    n_graze = _graze_outside_tail(c, n_img=n_act, listed=listed)
    flagged = int(ws[1])
    FLAGGED.setdefault("listed-" + _rid(row), {})[(1, cap)] = flagged
    assert n_graze >= 1 and flagged >= n_graze, ("flagged", flagged, "constructed neurons on listed positions", n_graze)
    assert _flag_ws_clean(ws)
    _report("fp6v2")


# ================================================================================================ e. device-side image count
def test_device_side_image_count_int8(dev, ops):
    """n_dyn = 3 of B = 5 through the wrapper's active_set: images below the count equal the oracle, the images beyond it keep the
    sentinel of the output buffer and their carried v."""
    row = O.DEN_NDYN_ROWS["i8"]
    c = _oracle("i8", row, carried=True)
    Cout, H, W, B = c.geo[1], c.geo[7], c.geo[8], c.geo[9]
    n = 3
    pk = ops.den_pack_weight_i8(c.w.to(dev), c.bias.to(dev))
    in0, in1 = _i8_in(ops, dev, c, 0)
    out = torch.full((B, Cout // 32, H, W, 16, 32), 0xAB, dtype=torch.uint8, device=dev)
    v = c.v0.to(dev).clone()
    with ops.active_set(*_n_active(dev, B, n)):
        got = ops.den_conv3x3_mfma(in0, pk, Cout, mode=ops.MODE_LIF, in1=in1, bn_a=c.a.to(dev), bn_b=c.b.to(dev), v=v, out=out)
    assert got.data_ptr() == out.data_ptr()
    _tally("i8", out[:n].cpu(), O.to_ptc(c.s1, 32)[:n], ("i8 n_dyn spikes", row))
    _tally("i8", v[:n].cpu(), c.v1[:n], ("i8 n_dyn v", row))
    _tally("i8", out[n:].cpu(), torch.full_like(out[n:].cpu(), 0xAB), ("i8 n_dyn sentinel", row))
    _tally("i8", v[n:].cpu(), c.v0[n:], ("i8 n_dyn untouched v", row))


def test_device_side_image_count_counts_form(dev, ops):
    row = O.DEN_NDYN_ROWS["counts"]
    c = _oracle("counts", row)
    B, n = c.geo[9], 3
    cnt0, cnt1 = _counts_in(ops, dev, c)
    pk = ops.den_pack_weight_i8(c.w.to(dev), c.bias.to(dev))
    with ops.active_set(*_n_active(dev, B, n)):
        got = ops.den_conv3x3_counts(cnt0, pk, c.geo[1], 16, cnt1=cnt1)
    want, _ = O.counts_logits(c.xs[0].sum(0), c.w, c.bias, c.geo)
    _tally("counts", got[:n].cpu(), want[:n], ("counts n_dyn", row))


def test_device_side_image_count_fp6(dev, ops):
    row = O.DEN_NDYN_ROWS["fp6"]
    c = _oracle("fp6", row, carried=True)
    Cout, B, n = c.geo[1], c.geo[9], 3
    pk = ops.den_pack_weight_fp6(c.w.to(dev), c.bias.to(dev))
    v = c.v0.to(dev).clone()
    with ops.active_set(*_n_active(dev, B, n)):
        out, cnt = ops.den_conv3x3_mfma_fp6(_c4(dev, c.xs[0]), pk, Cout, bn_a=c.a.to(dev), bn_b=c.b.to(dev), v=v, want_counts=True)
    _tally("fp6", _u8(out)[:n].cpu(), O.bits_to_packed(O.spikes_to_bits(c.s1), 64)[:n], ("fp6 n_dyn records", row))
    _tally("fp6", cnt[:n].cpu(), O.to_counts(c.s1)[:n], ("fp6 n_dyn counts", row))
    _tally("fp6", v[:n].cpu(), c.v1[:n], ("fp6 n_dyn v", row))
    _tally("fp6", v[n:].cpu(), c.v0[n:], ("fp6 n_dyn untouched v", row))


@pytest.mark.parametrize("cap", [-1, 0])
def test_device_side_image_count_fp6v2(dev, ops, cap):
    row = O.DEN_NDYN_ROWS["fp6v2"]
    c = _oracle("fp6v2", row)
    Cout, H, W, B, n = c.geo[1], c.geo[7], c.geo[8], c.geo[9], 3
    pk = ops.den_pack_weight_fp6v2(c.w.to(dev), c.bias.to(dev))
    with _settings(ops, cap, 0), ops.active_set(*_n_active(dev, B, n)):
        out, cnt = ops.den_conv3x3_mfma_fp6v2(_s32(dev, c.xs[0]), pk, Cout, bn_a=c.a.to(dev), bn_b=c.b.to(dev), want_counts=True)
    torch.cuda.synchronize()
    ws = _flag_ws(ops, dev, B, Cout, H, W).cpu()
    _tally("fp6v2", _u8(out)[:n].cpu(), O.bits_to_packed(c.bits, 32)[:n], ("fp6v2 n_dyn records", row, cap))
    _tally("fp6v2", cnt[:n].cpu(), c.cnt[:n], ("fp6v2 n_dyn counts", row, cap))
    need = _graze_outside_tail(c, n_img=n)
    FLAGGED.setdefault("ndyn-" + _rid(row), {})[(0, cap)] = int(ws[1])
    assert need >= 1 and int(ws[1]) >= need and _flag_ws_clean(ws), (int(ws[1]), need)
    _report("fp6v2")
