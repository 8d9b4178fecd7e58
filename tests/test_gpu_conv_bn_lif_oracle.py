"""The inference Conv + BN + LIF kernels against an EXACT host oracle (tests/_conv_bn_lif_oracle.py): the direct kernels of
csrc/conv_direct.hip (conv_fused_kernel, tinv_lif_kernel, tinv_lif_staged_kernel, conv_raw_steps_kernel), the int8 gather-MFMA kernels
of csrc/conv_mfma_gather.hip (the generic kernel and the five compile-time instances), csrc/vae_fp6.hip and the module path on top.

The inputs are dyadic, so the oracle's spikes and membrane potentials are the only correct answer (see the oracle module and
tests/test_conv_bn_lif_oracle_host.py, which checks the conditions on the inputs on the CPU): every spike, state, pre-activation and RAW
comparison below is torch.equal, with no fragile set and nothing excluded.  The read-outs that add T fp32 terms (MEMOUT, MEAN) carry the
error bound of that evaluation, derived in readout_bound()."""
import time

import pytest
import torch

import _conv_bn_lif_oracle as O
from _readout_oracle import readout_check
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


def _gid(g):
    return "-".join(str(int(v)) for v in g)


# tanhf's own error, measured on an MI355X as |kernel output with tanh - fp64 tanh of the kernel's fp32 read-out m| over the MEMOUT rows
# of this file (gather and IN_SEQ): between 5.0e-8 and 7.14e-8 per row (about one ulp of a value in [0.5, 1)).  Twice the largest value
# seen is allowed on top of the read-out bound, which passes through tanh unchanged (|tanh'| <= 1); the comparison itself is against
# fp64 tanh of the ORACLE's m.  Each run records its own measurement in PARITY_REPORT (tanhf_own_err).
TANHF_ERR_SEEN = 7.2e-8
TANHF_ERR_ALLOWED = 2 * TANHF_ERR_SEEN

STATS = {}           # family -> [neuron-steps compared, mismatches, host oracle seconds]
_ORACLE = {}


def _tally(fam, got, want, what):
    """torch.equal with the mismatch pattern in the message; counts into the family's parity record."""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    bad = got != want
    n_bad = int(bad.sum())
    st = STATS.setdefault(fam, [0, 0, 0.0])
    st[0] += want.numel()
    st[1] += n_bad
    parity(f"conv_bn_lif_oracle_{fam}", values=st[0], mismatches=st[1], host_oracle_s=round(st[2], 2))
    assert n_bad == 0, (what, f"{n_bad} of {want.numel()} differ; first at", bad.nonzero()[:8].tolist())


def _oracle(fam, geo, kind="spikes", T=16, weights="dyadic12"):
    """The case of a row and its oracle results, computed once per session and left unchanged: reset-state run on input 0, and the
    carried-state pair (v0 -> input 0 -> v1 -> input 1 -> v2).  weights="full": the row's full-width case (all digit planes of the MFMA
    kernels in play, threshold-grazing channels; see the oracle module)."""
    key = (geo, kind, T, weights)
    if key not in _ORACLE:
        t0 = time.perf_counter()
        seed = O.row_seed(geo, T) if weights == "dyadic12" else O.full_seed(geo)
        c = O.make_case(geo, seed, kind=kind, T=T, n_inputs=2, weights=weights)
        seqs = [x.unsqueeze(0).repeat(T, 1, 1, 1, 1) if kind == "pixels" else x for x in c.xs]
        c.y = [O.conv_fp32(x, c.w, c.bias, geo) for x in seqs]                 # MODE_RAW
        c.pre = [O.bn32(y, c.a, c.b) for y in c.y]                              # want_pre
        c.s, c.v = ref.lif_multi_step(c.pre[0])
        c.s1, c.v1 = ref.lif_multi_step(c.pre[0], c.v0.clone())
        c.s2, c.v2 = ref.lif_multi_step(c.pre[1], c.v1.clone())
        STATS.setdefault(fam, [0, 0, 0.0])[2] += time.perf_counter() - t0
        _ORACLE[key] = c
    return _ORACLE[key]


def _geo_kw(geo):
    return dict(k=geo[2], stride=geo[3], pad=geo[4], transposed=bool(geo[5]), out_pad=geo[6])


def _u8(t):
    return t.view(torch.uint8) if t.dtype == torch.int8 else t


def _readout_check(fam, what, got_f32, got_u8, want64, bound, tanh_err=0.0):
    """The rule of _readout_oracle.readout_check (shared with tests/test_gpu_readout_oracle.py); counts the bytes into the family's record."""
    worst = readout_check(what, got_f32, got_u8, want64, bound, tanh_err)
    if got_u8 is not None:
        st = STATS.setdefault(fam, [0, 0, 0.0])
        st[0] += got_u8.numel()
    return worst


# ================================================================================================ a. gather family
def _gather_in(ops, dev, c, i=0):
    geo = c.geo
    pk = ops.pack_conv_weight_i8(c.w.to(dev), c.bias.to(dev), bool(geo[5]))
    return O.to_ptc(c.xs[i]).to(dev), pk


@pytest.mark.parametrize("geo", O.GATHER_ROWS, ids=_gid)
def test_gather_lif_from_reset_state_all_output_forms(dev, ops, geo):
    """u8 PTC, S32 (Cout % 32 == 0) and the time-collapsed output of spk_conv_mfma_fused_fwd / _lif_s32 equal the oracle's spikes."""
    _gather_reset(dev, ops, geo, "dyadic12")


@pytest.mark.parametrize("geo", O.GATHER_FULL_ROWS, ids=_gid)
def test_gather_lif_from_reset_state_full_width_weights(dev, ops, geo):
    """The same on full-width weights: one spike-input row of each compile-time instance and one generic row, with all four int8 digit
    planes in play (multiples of 2^-12 leave the low planes zero) and neurons built to sit exactly on the threshold."""
    _gather_reset(dev, ops, geo, "full")


def _gather_reset(dev, ops, geo, weights):
    c = _oracle("gather", geo, weights=weights)
    Cout, kw = geo[1], _geo_kw(geo)
    ptc, pk = _gather_in(ops, dev, c)
    a, b = c.a.to(dev), c.b.to(dev)
    got = ops.conv_mfma_fused(ptc, pk, Cout, mode=ops.MODE_LIF, bn_a=a, bn_b=b, **kw)
    _tally("gather", got.cpu(), O.to_ptc(c.s), ("ptc", geo))
    if Cout % 32 == 0:
        s32 = ops.conv_mfma_fused(ptc, pk, Cout, mode=ops.MODE_LIF, bn_a=a, bn_b=b, out_s32=True, **kw)
        _tally("gather", _u8(s32).cpu(), O.bits_to_packed(O.spikes_to_bits(c.s), 32), ("s32 records", geo))
        _tally("gather", ops.s32_to_spikes(s32).cpu(), c.s, ("s32", geo))
    col = ops.conv_mfma_fused(ptc, pk, Cout, mode=ops.MODE_LIF, bn_a=a, bn_b=b, collapse_coef=c.coef.to(dev), **kw)
    _tally("gather", col.cpu(), O.collapse32(c.s, c.coef).permute(0, 2, 3, 1).contiguous(), ("collapsed", geo))
    assert 0.02 <= float(c.s.mean()) <= 0.6


@pytest.mark.parametrize("geo", O.GATHER_ROWS, ids=_gid)
def test_gather_lif_with_carried_membrane_state(dev, ops, geo):
    """v carried over two calls on different spike inputs, starting from a non-zero dyadic v0: spikes and v bit-equal after each."""
    _gather_carried(dev, ops, geo, "dyadic12")


@pytest.mark.parametrize("geo", O.GATHER_FULL_ROWS, ids=_gid)
def test_gather_lif_with_carried_membrane_state_full_width_weights(dev, ops, geo):
    _gather_carried(dev, ops, geo, "full")


def _gather_carried(dev, ops, geo, weights):
    c = _oracle("gather", geo, weights=weights)
    Cout, kw = geo[1], _geo_kw(geo)
    ptc0, pk = _gather_in(ops, dev, c, 0)
    ptc1 = O.to_ptc(c.xs[1]).to(dev)
    a, b = c.a.to(dev), c.b.to(dev)
    v = c.v0.to(dev).clone()
    got1 = ops.conv_mfma_fused(ptc0, pk, Cout, mode=ops.MODE_LIF, bn_a=a, bn_b=b, v=v, **kw)
    _tally("gather", got1.cpu(), O.to_ptc(c.s1), ("call 1 spikes", geo))
    _tally("gather", v.cpu(), c.v1, ("call 1 v", geo))
    got2 = ops.conv_mfma_fused(ptc1, pk, Cout, mode=ops.MODE_LIF, bn_a=a, bn_b=b, v=v, **kw)
    _tally("gather", got2.cpu(), O.to_ptc(c.s2), ("call 2 spikes", geo))
    _tally("gather", v.cpu(), c.v2, ("call 2 v", geo))
    if Cout % 32 == 0:                                       # the S32 entry point carries v too
        v = c.v0.to(dev).clone()
        s32 = ops.conv_mfma_fused(ptc0, pk, Cout, mode=ops.MODE_LIF, bn_a=a, bn_b=b, v=v, out_s32=True, **kw)
        _tally("gather", _u8(s32).cpu(), O.bits_to_packed(O.spikes_to_bits(c.s1), 32), ("s32 call 1", geo))
        _tally("gather", v.cpu(), c.v1, ("s32 call 1 v", geo))


@pytest.mark.parametrize("geo", O.MEMOUT_ROWS, ids=_gid)
def test_gather_memout_within_the_fp32_evaluation_bound(dev, ops, geo):
    """MODE_MEMOUT (no BN, no LIF): sum_t coef[t] * y[t] with y the exact convolution rounded once; with and without tanh, plus u8."""
    _gather_memout(dev, ops, geo, "dyadic12")


@pytest.mark.parametrize("geo", [g for g in O.GATHER_FULL_ROWS if g in O.MEMOUT_ROWS], ids=_gid)
def test_gather_memout_full_width_weights(dev, ops, geo):
    _gather_memout(dev, ops, geo, "full")


def _gather_memout(dev, ops, geo, weights):
    c = _oracle("gather", geo, weights=weights)
    Cout, kw = geo[1], _geo_kw(geo)
    ptc, pk = _gather_in(ops, dev, c)
    m64, mag = O.memout64(c.y[0], c.coef)
    bound = O.readout_bound(16, mag)
    coef = c.coef.to(dev)
    r = ops.conv_mfma_fused(ptc, pk, Cout, mode=ops.MODE_MEMOUT, coef=coef, apply_tanh=False, want_u8=True, **kw)
    e0 = _readout_check("gather", ("memout", geo), r["f32"].cpu(), r["u8"].cpu(), m64, bound)
    rt = ops.conv_mfma_fused(ptc, pk, Cout, mode=ops.MODE_MEMOUT, coef=coef, apply_tanh=True, want_u8=True, **kw)
    own = float((rt["f32"].cpu().double() - torch.tanh(r["f32"].cpu().double())).abs().max())      # tanhf alone
    print(f"gather memout {geo}: max err {e0:.3e} (bound up to {float(bound.max()):.3e}); tanhf own error {own:.3e}")
    e1 = _readout_check("gather", ("memout+tanh", geo), rt["f32"].cpu(), rt["u8"].cpu(), torch.tanh(m64), bound, TANHF_ERR_ALLOWED)
    parity(f"conv_bn_lif_oracle_gather_memout_{_gid(geo)}" + ("" if weights == "dyadic12" else "_full"), max_err=e0, max_err_tanh=e1, tanhf_own_err=own,
           tanhf_err_allowed=TANHF_ERR_ALLOWED)
    assert own <= TANHF_ERR_ALLOWED


# ================================================================================================ b. direct family
def _direct_w(ops, dev, c):
    return ops.pack_conv_weight(c.w.to(dev), bool(c.geo[5])), c.bias.to(dev)


def _direct(ops, dev, c, in0, **kw):
    wp, bias = _direct_w(ops, dev, c)
    args = dict(in_kind=ops.IN_PTC, T=c.T, mode=ops.MODE_LIF, bn_a=c.a.to(dev), bn_b=c.b.to(dev), **_geo_kw(c.geo))
    args.update(kw)
    if args["mode"] != ops.MODE_LIF:
        args.pop("bn_a"), args.pop("bn_b")
    return ops.conv_fused(in0, wp, bias, **args)


@pytest.mark.parametrize("geo", O.GATHER_ROWS + O.DIRECT_PTC_EXTRA, ids=_gid)
def test_direct_ptc_lif_raw_and_carried_state(dev, ops, geo):
    """conv_fused_kernel<IN_PTC> (and conv_raw_steps_kernel for RAW at Cout = 1, 3): spikes as u8 PTC and fp32, RAW == the
    convolution rounded once, and v carried over two calls."""
    c = _oracle("direct", geo)
    ptc0, ptc1 = O.to_ptc(c.xs[0]).to(dev), O.to_ptc(c.xs[1]).to(dev)
    r = _direct(ops, dev, c, ptc0, want_ptc=True, want_f32=True)
    _tally("direct", r["ptc"].cpu(), O.to_ptc(c.s), ("ptc", geo))
    _tally("direct", r["f32"].cpu(), c.s, ("f32", geo))
    raw = _direct(ops, dev, c, ptc0, mode=ops.MODE_RAW)
    _tally("direct", raw["f32"].cpu(), c.y[0], ("raw", geo))
    v = c.v0.to(dev).clone()
    r1 = _direct(ops, dev, c, ptc0, want_ptc=True, v=v)
    _tally("direct", r1["ptc"].cpu(), O.to_ptc(c.s1), ("call 1 spikes", geo))
    _tally("direct", v.cpu(), c.v1, ("call 1 v", geo))
    r2 = _direct(ops, dev, c, ptc1, want_ptc=True, v=v)
    _tally("direct", r2["ptc"].cpu(), O.to_ptc(c.s2), ("call 2 spikes", geo))
    _tally("direct", v.cpu(), c.v2, ("call 2 v", geo))


def test_direct_ptc_concatenated_chunked_inputs(dev, ops):
    """in1 concatenated after in0 along channels (C0 = 8, C1 = 4), both in the CPTC layout with chunks of 4."""
    c = _oracle("direct", O.CONCAT_ROW)
    x = c.xs[0]
    in0, in1 = O.to_ptc(x[:, :, :8].contiguous(), 4).to(dev), O.to_ptc(x[:, :, 8:].contiguous(), 4).to(dev)
    assert in0.shape[1] == 2 and in1.shape[1] == 1
    r = _direct(ops, dev, c, in0, in1=in1, want_ptc=True, want_pre=True)
    _tally("direct", r["ptc"].cpu(), O.to_ptc(c.s), ("concat ptc", c.geo))
    _tally("direct", r["pre"].cpu(), c.pre[0], ("concat pre", c.geo))
    # ... and plain PTC in0 with a chunked in1
    r = _direct(ops, dev, c, O.to_ptc(x[:, :, :8].contiguous()).to(dev), in1=in1, want_ptc=True)
    _tally("direct", r["ptc"].cpu(), O.to_ptc(c.s), ("concat plain + chunked", c.geo))


def test_direct_ptc_chunked_output(dev, ops):
    c = _oracle("direct", O.CHUNK_OUT_ROW)
    r = _direct(ops, dev, c, O.to_ptc(c.xs[0]).to(dev), want_ptc=True, chunk_out=4)
    _tally("direct", r["ptc"].cpu(), O.to_ptc(c.s, 4), ("chunk_out 4", c.geo))


def test_direct_ptc_s32_and_c4_packing_on_a_half_filled_wave(dev, ops):
    """Nibble-packed outputs: S32 at 15 positions x 32 channels (the last wave half filled), C4 at Cout = 64."""
    c = _oracle("direct", O.S32_ROW)
    r = _direct(ops, dev, c, O.to_ptc(c.xs[0]).to(dev), want_ptc=True, chunk_out=ops.CHUNK_S32)
    _tally("direct", _u8(r["ptc"]).cpu(), O.bits_to_packed(O.spikes_to_bits(c.s), 32), ("s32 records", c.geo))
    _tally("direct", ops.s32_to_spikes(r["ptc"]).cpu(), c.s, ("s32", c.geo))
    c = _oracle("direct", O.C4_ROW)
    r = _direct(ops, dev, c, O.to_ptc(c.xs[0]).to(dev), want_ptc=True, chunk_out=ops.CHUNK_C4)
    _tally("direct", _u8(r["ptc"]).cpu(), O.bits_to_packed(O.spikes_to_bits(c.s), 64), ("c4 records", c.geo))
    v = c.v0.to(dev).clone()
    r = _direct(ops, dev, c, O.to_ptc(c.xs[0]).to(dev), want_ptc=True, chunk_out=ops.CHUNK_C4, v=v)
    _tally("direct", _u8(r["ptc"]).cpu(), O.bits_to_packed(O.spikes_to_bits(c.s1), 64), ("c4 records, carried v", c.geo))
    _tally("direct", v.cpu(), c.v1, ("c4 v", c.geo))


def test_direct_ptc_spike_counts(dev, ops):
    c = _oracle("direct", O.COUNTS_ROW)
    B, Cout = c.geo[9], c.geo[1]
    want = c.s.sum(0).to(torch.uint8).view(B, Cout // 32, 32, c.Ho, c.Wo).permute(0, 1, 3, 4, 2).contiguous()
    for chunk_out in (None, ops.CHUNK_S32):
        r = _direct(ops, dev, c, O.to_ptc(c.xs[0]).to(dev), want_ptc=True, want_counts=True, chunk_out=chunk_out)
        _tally("direct", r["cnt"].cpu(), want, ("counts", chunk_out, c.geo))
    _tally("direct", _u8(r["ptc"]).cpu(), O.bits_to_packed(O.spikes_to_bits(c.s), 32), ("s32 with counts", c.geo))
    assert int(want.max()) > 1


@pytest.mark.parametrize("T", [4, 7])
def test_direct_ptc_short_time(dev, ops, T):
    """T < 16: the unrolled sixteen-step loops stop at T; S32 records of T steps at T = 4."""
    c = _oracle("direct", O.SHORT_T_ROW, T=T)
    ptc = O.to_ptc(c.xs[0]).to(dev)
    assert ptc.shape[3] == T
    r = _direct(ops, dev, c, ptc, want_ptc=True, want_f32=True, want_pre=True)
    _tally("direct", r["ptc"].cpu(), O.to_ptc(c.s), ("short ptc", T))
    _tally("direct", r["f32"].cpu(), c.s, ("short f32", T))
    _tally("direct", r["pre"].cpu(), c.pre[0], ("short pre", T))
    if T == 4:
        r = _direct(ops, dev, c, ptc, want_ptc=True, chunk_out=ops.CHUNK_S32)
        _tally("direct", _u8(r["ptc"]).cpu(), O.bits_to_packed(O.spikes_to_bits(c.s), 32, T), ("short s32", T))
    v = c.v0.to(dev).clone()
    r = _direct(ops, dev, c, ptc, want_ptc=True, v=v)
    _tally("direct", r["ptc"].cpu(), O.to_ptc(c.s1), ("short carried", T))
    _tally("direct", v.cpu(), c.v1, ("short v", T))


def test_direct_ptc_pre_activation(dev, ops):
    """want_pre: the BN output fmaf(y, a, b) of every step, bit-equal (transposed row)."""
    c = _oracle("direct", O.PRE_ROW)
    r = _direct(ops, dev, c, O.to_ptc(c.xs[0]).to(dev), want_ptc=True, want_pre=True)
    _tally("direct", r["pre"].cpu(), c.pre[0], ("pre", c.geo))
    _tally("direct", r["ptc"].cpu(), O.to_ptc(c.s), ("pre: ptc", c.geo))


@pytest.mark.parametrize("T", [3, 16])
@pytest.mark.parametrize("geo", O.SEQ_ROWS, ids=_gid)
def test_direct_seq_lif_raw_memout_mean(dev, ops, geo, T):
    """conv_fused_kernel<IN_SEQ> on dyadic real sequences: LIF (fresh and carried), RAW, MEMOUT (+ tanh, u8) and MEAN."""
    c = _oracle("direct", geo, kind="seq", T=T)
    x0, x1 = c.xs[0].to(dev), c.xs[1].to(dev)
    seq = dict(in_kind=ops.IN_SEQ)
    r = _direct(ops, dev, c, x0, want_ptc=True, want_f32=True, want_pre=True, **seq)
    _tally("direct", r["f32"].cpu(), c.s, ("seq f32", geo, T))
    _tally("direct", r["ptc"].cpu(), O.to_ptc(c.s), ("seq ptc", geo, T))
    _tally("direct", r["pre"].cpu(), c.pre[0], ("seq pre", geo, T))
    _tally("direct", _direct(ops, dev, c, x0, mode=ops.MODE_RAW, **seq)["f32"].cpu(), c.y[0], ("seq raw", geo, T))
    v = c.v0.to(dev).clone()
    _tally("direct", _direct(ops, dev, c, x0, want_f32=True, v=v, **seq)["f32"].cpu(), c.s1, ("seq call 1", geo, T))
    _tally("direct", v.cpu(), c.v1, ("seq call 1 v", geo, T))
    _tally("direct", _direct(ops, dev, c, x1, want_f32=True, v=v, **seq)["f32"].cpu(), c.s2, ("seq call 2", geo, T))
    _tally("direct", v.cpu(), c.v2, ("seq call 2 v", geo, T))
    m64, mag = O.memout64(c.y[0], c.coef)
    bound = O.readout_bound(T, mag)
    coef = c.coef.to(dev)
    rm = _direct(ops, dev, c, x0, mode=ops.MODE_MEMOUT, coef=coef, want_u8=True, **seq)
    e0 = _readout_check("direct", ("seq memout", geo, T), rm["f32"].cpu(), rm["u8"].cpu(), m64, bound)
    rt = _direct(ops, dev, c, x0, mode=ops.MODE_MEMOUT, coef=coef, apply_tanh=True, want_u8=True, **seq)
    own = float((rt["f32"].cpu().double() - torch.tanh(rm["f32"].cpu().double())).abs().max())
    e1 = _readout_check("direct", ("seq memout+tanh", geo, T), rt["f32"].cpu(), rt["u8"].cpu(), torch.tanh(m64), bound, TANHF_ERR_ALLOWED)
    mean, mmag = O.mean64(c.y[0])
    rmean = _direct(ops, dev, c, x0, mode=ops.MODE_MEAN, **seq)
    e2 = _readout_check("direct", ("seq mean", geo, T), rmean["f32"].cpu(), None, mean, O.readout_bound(T + 1, mmag))
    print(f"seq {geo} T={T}: memout err {e0:.3e}, +tanh {e1:.3e} (tanhf own {own:.3e}), mean err {e2:.3e}")
    parity(f"conv_bn_lif_oracle_seq_readouts_{_gid(geo)}_T{T}", memout_err=e0, memout_tanh_err=e1, tanhf_own_err=own, mean_err=e2)
    assert own <= TANHF_ERR_ALLOWED


@pytest.mark.parametrize("row", O.TINV_ROWS, ids=_gid)
def test_direct_tinv_stateless_carried_and_generic(dev, ops, row):
    """Time-invariant input: stateless (tinv_lif_staged_kernel, or tinv_lif_kernel<0,0> where no staged instance exists), carried v
    over two calls on different frames (tinv_lif_kernel<KS,KC>), and with want_f32 + want_pre (the generic conv_fused_kernel<TINV>).
    S32 output where Cout % 32 == 0, plain PTC otherwise."""
    geo = O.tinv_geo(row)
    c = _oracle("direct", geo, kind="pixels")
    Cout = geo[1]
    x0, x1 = c.xs[0].to(dev), c.xs[1].to(dev)
    s32 = Cout % 32 == 0
    tin = dict(in_kind=ops.IN_TINV, want_ptc=True, chunk_out=ops.CHUNK_S32 if s32 else None)

    def want(s):
        return O.bits_to_packed(O.spikes_to_bits(s), 32) if s32 else O.to_ptc(s)

    _tally("direct", _u8(_direct(ops, dev, c, x0, **tin)["ptc"]).cpu(), want(c.s), ("tinv stateless", row))
    v = c.v0.to(dev).clone()
    _tally("direct", _u8(_direct(ops, dev, c, x0, v=v, **tin)["ptc"]).cpu(), want(c.s1), ("tinv call 1", row))
    _tally("direct", v.cpu(), c.v1, ("tinv call 1 v", row))
    _tally("direct", _u8(_direct(ops, dev, c, x1, v=v, **tin)["ptc"]).cpu(), want(c.s2), ("tinv call 2", row))
    _tally("direct", v.cpu(), c.v2, ("tinv call 2 v", row))
    r = _direct(ops, dev, c, x0, want_f32=True, want_pre=True, **tin)
    _tally("direct", _u8(r["ptc"]).cpu(), want(c.s), ("tinv generic ptc", row))
    _tally("direct", r["f32"].cpu(), c.s, ("tinv generic f32", row))
    _tally("direct", r["pre"].cpu(), c.pre[0][0], ("tinv generic pre", row))
    if s32:                                                   # ... and the spike counts the lean kernels write with S32 records
        r = _direct(ops, dev, c, x0, want_counts=True, **tin)
        B = geo[9]
        cnt = c.s.sum(0).to(torch.uint8).view(B, Cout // 32, 32, c.Ho, c.Wo).permute(0, 1, 3, 4, 2).contiguous()
        _tally("direct", r["cnt"].cpu(), cnt, ("tinv counts", row))


def test_direct_second_trip_of_conv_fused_grid_stride_loop(dev, ops):
    """2 157 568 work items against grid_for's cap of 8192 blocks x 256: the tail runs in a second trip.  Compared as S32 records on the
    device (the oracle keeps one int32 of spike bits per neuron; no fp32 spike tensor is built on the host)."""
    geo = O.TRIP2_PTC_ROW
    Cin, Cout, k, s, p, tr, op, H, W, B = geo
    assert B * H * W * Cout > 8192 * 256
    t0 = time.perf_counter()
    c = O.make_case(geo, O.row_seed(geo))
    bits, _ = O.conv_bn_lif_bits(lambda t: c.x[t], c.w, c.bias, c.a, c.b, None, geo)
    STATS.setdefault("direct", [0, 0, 0.0])[2] += time.perf_counter() - t0
    r = _direct(ops, dev, c, O.to_ptc(c.x).to(dev), want_ptc=True, chunk_out=ops.CHUNK_S32)
    want = O.bits_to_packed(bits.to(dev), 32)
    n_bad = int((_u8(r["ptc"]) != want).sum())
    st = STATS["direct"]; st[0] += 16 * bits.numel(); st[1] += n_bad
    parity("conv_bn_lif_oracle_direct", values=st[0], mismatches=st[1], host_oracle_s=round(st[2], 2))
    assert n_bad == 0 and 0 < int(want.count_nonzero()) < want.numel()


def test_direct_second_trip_of_the_tinv_loops(dev, ops):
    """137 200 positions: past the staged kernel's 2048 chunks of 64 (stateless call) and past tinv_lif_kernel's 4096 block steps of
    16 positions (carried v).  Compared as u8 PTC on the device."""
    geo = O.tinv_geo(O.TRIP2_TINV_ROW)
    B, Ho, Wo = geo[9], *O.geo_out_hw(geo)
    assert B * Ho * Wo > 2048 * 64 and B * Ho * Wo > 4096 * 16
    t0 = time.perf_counter()
    c = O.make_case(geo, O.row_seed(geo), kind="pixels")
    bits, _ = O.conv_bn_lif_bits(c.x, c.w, c.bias, c.a, c.b, None, geo)
    bits1, v1 = O.conv_bn_lif_bits(c.x, c.w, c.bias, c.a, c.b, c.v0, geo)
    STATS.setdefault("direct", [0, 0, 0.0])[2] += time.perf_counter() - t0
    x = c.x.to(dev)
    got = _direct(ops, dev, c, x, in_kind=ops.IN_TINV, want_ptc=True)["ptc"]
    v = c.v0.to(dev).clone()
    got1 = _direct(ops, dev, c, x, in_kind=ops.IN_TINV, want_ptc=True, v=v)["ptc"]
    n_bad = int((got != O.bits_to_ptc(bits.to(dev))).sum()) + int((got1 != O.bits_to_ptc(bits1.to(dev))).sum())
    n_bad_v = int((v.cpu() != v1).sum())
    st = STATS["direct"]; st[0] += 2 * 16 * bits.numel() + v1.numel(); st[1] += n_bad + n_bad_v
    parity("conv_bn_lif_oracle_direct", values=st[0], mismatches=st[1], host_oracle_s=round(st[2], 2))
    assert n_bad == 0 and n_bad_v == 0
    assert 0.02 <= float(got.float().mean()) <= 0.6


# ================================================================================================ c. vae_fp6 against the oracle
FLAG_LIST = 1 << 20          # id-list entries of a certified kernel's workspace: [count, published count, ids..., bitmap, ticket]


def _flag_ws_clean(v):
    return int(v[0]) == 0 and int(v[2 + FLAG_LIST:].abs().sum()) == 0


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("row", O.VAE_FP6_ROWS, ids=lambda r: r[0])
def test_vae_fp6_against_the_oracle(dev, ops, row, B):
    """spk_vae_fp6_fwd in its three geometries, each with its own output kind, straight against the host oracle (no gather kernel in
    between); the flag workspace comes back clean."""
    _vae_fp6(dev, ops, row, B, "dyadic12")


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("row", O.VAE_FP6_ROWS, ids=lambda r: r[0])
def test_vae_fp6_against_the_oracle_full_width_weights(dev, ops, row, B):
    """The same on full-width weights: the fifth and sixth radix-32 digit, which the certification drops and bounds and only the exact
    repair reads, are non-zero, and the constructed threshold-grazing neurons must be flagged (word 1 of the workspace)."""
    c = _vae_fp6(dev, ops, row, B, "full")
    ws = [v for k, v in ops._FLAG_DEFAULT.items() if k[0] == "vae"]
    flagged = max(int(v[1]) for v in ws)
    print(f"vae_fp6 {row[0]} B={B} full-width: last calls flagged up to {flagged}; constructed neurons {len(c.graze)}")
    assert len(c.graze) >= 1


def _vae_fp6(dev, ops, row, B, weights):
    layer, Cin, Cout, tr, op, H = row
    geo = O.vae_fp6_geo(row, B)
    kind = {"enc2": ops.VAE_OUT_PTC, "dec1": ops.VAE_OUT_S32, "dec2": ops.VAE_OUT_COLLAPSED}[layer]
    assert ops.vae_fp6_kind(Cin, Cout, 3, 2, 1, op, tr, 16, H, H) == kind
    c = _oracle("vae_fp6", geo, weights=weights)
    x = c.xs[0]
    if Cin % 32:                                              # zero nibbles beyond Cin
        x = torch.cat([x, torch.zeros(x.shape[0], B, 32 - Cin % 32, H, H)], dim=2)
    s32 = O.bits_to_packed(O.spikes_to_bits(x), 32).view(torch.int8).to(dev)
    pk = ops.vae_fp6_pack(c.w.to(dev), c.bias.to(dev), tr)
    got = ops.vae_fp6_fwd(s32, pk, Cout, bn_a=c.a.to(dev), bn_b=c.b.to(dev), transposed=tr, out_kind=kind,
                          coef=c.coef.to(dev) if layer == "dec2" else None)
    if layer == "enc2":
        _tally("vae_fp6", got.cpu(), O.to_ptc(c.s), (layer, B))
    elif layer == "dec1":
        _tally("vae_fp6", _u8(got).cpu(), O.bits_to_packed(O.spikes_to_bits(c.s), 32), (layer, B))
    else:
        _tally("vae_fp6", got.cpu(), O.collapse32(c.s, c.coef).permute(0, 2, 3, 1).contiguous(), (layer, B))
    torch.cuda.synchronize()
    ws = [v for k, v in ops._FLAG_DEFAULT.items() if k[0] == "vae"]
    assert ws and all(_flag_ws_clean(v) for v in ws), "live counter, overflow bitmap and hand-over ticket come back clean"
    return c


# ================================================================================================ d. module path
@pytest.mark.parametrize("H,W", [(20, 12), (28, 28)], ids=["20x12-gather", "28x28-fp6"])
def test_fused_sequential_against_the_chained_oracle(dev, ops, H, W):
    """A FusedSequential of three Conv + BN + LIF triples (3x3 s2 1->32, 3x3 s2 32->64, 1x1 64->16) in eval mode on dyadic images:
    dyadic weights, arbitrary running statistics.  20x12 has no fp6 instance (direct, then the gather kernels); 28x28 takes the fp6
    encoder layer.  The BN terms equal ops.bn_prepare bit for bit, and the final PTC spikes equal the oracle chained layer by layer."""
    from spikingjelly.activation_based import functional, layer, neuron
    from spkdiff.fused import FusedSequential
    B, T = 3, 16
    g = torch.Generator().manual_seed(900 + H)
    chans = [(1, 32, 3, 2, 1), (32, 64, 3, 2, 1), (64, 16, 1, 1, 0)]
    mods, params = [], []
    h, w = H, W
    for i, (ci, co, k, s, p) in enumerate(chans):
        geo = (ci, co, k, s, p, False, 0, h, w, B)
        cs = O.make_case(geo, 900 + 10 * i + H, kind="pixels" if i == 0 else "spikes")
        conv, bn = layer.Conv2d(ci, co, k, s, p), layer.BatchNorm2d(co)
        if i:
            cs.w = cs.w * 2                                   # (still dyadic; these layers see spikes at 0.15 - 0.3)
        with torch.no_grad():
            conv.weight.copy_(cs.w); conv.bias.copy_(cs.bias)
            bn.weight.copy_(torch.rand(co, generator=g) + 1.0); bn.bias.copy_(torch.rand(co, generator=g) * 0.8)
            bn.running_mean.copy_(torch.rand(co, generator=g) * 0.6 - 0.3); bn.running_var.copy_(torch.rand(co, generator=g) * 0.5 + 0.5)
        mods += [conv, bn, neuron.LIFNode()]
        params.append((geo, cs.w, cs.bias, bn))
        h, w = O.geo_out_hw(geo)
    net = FusedSequential(*mods)
    functional.set_step_mode(net, "m")
    img = O.dyadic((B, 1, H, W), g, 8, 1.0)
    t0 = time.perf_counter()
    x = img.unsqueeze(0).repeat(T, 1, 1, 1, 1)
    terms = []
    for geo, wt, bias, bn in params:
        sd = {"b." + k: v.detach().clone() for k, v in bn.state_dict().items() if v.dtype == torch.float32}
        a, b = ref.bn_affine_terms(sd, "b")
        terms.append((a, b))
        x, _, _ = O.conv_bn_lif(x, wt, bias, a, b, None, geo)
        assert 0.02 <= float(x.mean()) <= 0.6, (geo, float(x.mean()))
    STATS.setdefault("module", [0, 0, 0.0])[2] += time.perf_counter() - t0
    net = net.to(dev).eval()
    for (a, b), (_, _, _, bn) in zip(terms, params):
        ga, gb = ops.bn_prepare(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        assert torch.equal(ga.cpu(), a) and torch.equal(gb.cpu(), b), "ops.bn_prepare differs from ref.bn_affine_terms"
    with torch.inference_mode():
        got = net.run(img.to(dev), ops.IN_TINV, T=T, final="ptc", stateful=False)["ptc"]
        _tally("module", got.cpu(), O.to_ptc(x), ("module stateless", H, W))
        seq = net(img.to(dev).unsqueeze(0).repeat(T, 1, 1, 1, 1))            # the module call: IN_SEQ first layer, stateful
        _tally("module", seq.cpu(), x, ("module forward", H, W))
