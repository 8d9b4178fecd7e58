"""GPU tests of the element-wise streaming kernels behind the module surface (csrc/lif.hip: spk_lif_fwd, spk_lif_fwd_ex,
spk_bn_eval_fwd, spk_memout_fwd; csrc/lif_train.hip: spk_lif_train_fwd / _bwd, spk_psp) against plain host oracles, at the
shapes the model-level tests do not reach (tests/_stream_cases.py names them and says which kernel and how many passes each is):
  * past every grid cap, where the grid-stride loops make a second, ragged pass;
  * contiguous views that start 4, 8 or 12 bytes into an allocation with N % 4 == 0, which must take the scalar kernels;
  * T across the SPK_LIF_TU chunk, the four forms of the eval neuron, both DIV forms, v_reset != 0;
  * membrane potentials exactly on the threshold and one ulp either side, NaN and infinite inputs;
  * spk_lif_fwd and spk_memout_fwd with (T - 1) * N past 2^31, where a 32-bit plane offset would wrap.
Forward arithmetic is IEEE fp32 operation by operation and must equal the oracle bit for bit (any NaN equal to any NaN).  The
two adjoints are held to an fp64 restatement run on the kernel's own h_seq by a counted round-off bound: per element
c * 2^-23 * M, c the fp32 roundings on the longest path times the steps feeding the element, M the recurrence on absolute
values (tests/_stream_cases.py has the count).  Outputs are allocated over NaN-filled blocks, so an element a kernel fails to
write is NaN."""
import numpy as np
import pytest
import torch

import _stream_cases as sc
from oracle import snn_ref as ref
from parity_report import record as parity
from spkdiff import ops

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
TALLY = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


def tally(name, **counts):
    """Accumulate the counts of one test function over its cases and keep its PARITY_REPORT line current ('max_' keys keep
    their maximum)."""
    t = TALLY.setdefault(name, {})
    for k, v in counts.items():
        t[k] = max(t.get(k, 0.0), v) if k.startswith("max_") else t.get(k, 0) + v
    parity("stream_" + name, **t)


def diff_bits(a, b):
    """Elements that differ bit for bit, any NaN equal to any NaN (the payload a NaN carries is not part of the contract)."""
    a, b = a.reshape(-1), b.reshape(-1)
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32
    na, nb = torch.isnan(a), torch.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(torch.int32) != b.view(torch.int32)))).sum())


def same_bits(a, b):
    return diff_bits(a, b) == 0


def poison(dev, *numels):
    """Leave NaN-filled blocks of these sizes in the caching allocator, so that outputs a kernel fails to write are NaN
    rather than whatever an earlier call left there."""
    bufs = [torch.full((int(n),), NAN, device=dev) for n in numels]
    del bufs


GUARD = 777.0


def view_at(t, dev, off):
    """``t`` on the device as a contiguous view ``off`` floats into a larger allocation (guard values around it)."""
    base = torch.full((t.numel() + 8,), GUARD, device=dev)
    w = base[off:off + t.numel()].view(t.shape)
    w.copy_(t)
    assert w.is_contiguous() and w.data_ptr() % 16 == (4 * off) % 16
    return w, base


def guards_intact(base, off, n):
    return bool((base[:off] == GUARD).all()) and bool((base[off + n:] == GUARD).all())


def rand_inputs(T, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, N, generator=g) * 1.5 + 0.7
    v0 = torch.rand(N, generator=g) - 0.5
    return x, v0


def unpack_words(words, N):
    """int64 [T, ceil(N / 64)] -> (spikes fp32 [T, N], number of set pad bits in the last word of every step)."""
    w = words.cpu().contiguous().numpy().view(np.uint64)
    bits = ((w[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(w.shape[0], -1)
    return torch.from_numpy(bits[:, :N].astype(np.float32)), int(bits[:, N:].sum())


def run_lif_fwd(dev, x, v0, tau, vth, vr, dt, want=None, xd=None, vd=None):
    """One spk_lif_fwd call against ref.lif_multi_step: (spike mismatches, v mismatches, set pad bits)."""
    T, N = x.shape
    if want is None:
        want = ref.lif_multi_step(x, v0.clone(), vth, vr, tau)
    xd = x.to(dev) if xd is None else xd
    vd = v0.clone().to(dev) if vd is None else vd
    poison(dev, T * N, T * N // 4 + 1, T * ((N + 63) // 64) * 2)
    s = ops.lif_fwd(xd, vd, tau, vth, vr, spike_dtype=dt)
    pad = 0
    if dt == ops.SPIKE_BITS:
        assert s.shape == (T, (N + 63) // 64) and s.dtype == torch.int64
        s, pad = unpack_words(s, N)
    else:
        assert s.dtype == (torch.float32 if dt == ops.SPIKE_F32 else torch.uint8)
        s = s.cpu().float()
    return int((s != want[0]).sum()), diff_bits(vd.cpu(), want[1]), pad


DTYPES = (ops.SPIKE_F32, ops.SPIKE_U8, ops.SPIKE_BITS)
LIF_PARAMS = ((2.0, 1.0, 0.0), (3.0, 1.0, -0.25), (0.5, 1.0, -0.25), (2.0, 0.5, -0.25))     # (tau, v_th, v_reset)


# ------------------------------------------------------------------------------------------------------------ (a) spk_lif_fwd
@pytest.mark.parametrize("N", sc.SMALL_N)
def test_lif_fwd_small_family(dev, N):
    """Three spike dtypes x T across the SPK_LIF_TU = 8 chunk x both DIV forms, v_reset != 0."""
    for T in (1, 7, 8, 9, 16, 17):
        x, v0 = rand_inputs(T, N, N * 31 + T)
        for tau, vth, vr in LIF_PARAMS:
            want = ref.lif_multi_step(x, v0.clone(), vth, vr, tau)
            for dt in DTYPES:
                bad_s, bad_v, pad = run_lif_fwd(dev, x, v0, tau, vth, vr, dt, want)
                tally("lif_fwd_small", neuron_steps=T * N, spike_mismatches=bad_s, v_mismatches=bad_v, pad_bits_set=pad)
                assert (bad_s, bad_v, pad) == (0, 0, 0), (N, T, tau, vth, vr, dt)


@pytest.mark.parametrize("cid", ["lif_fwd_f32_vec", "lif_fwd_u8_vec", "lif_fwd_f32_scalar", "lif_fwd_u8_scalar", "lif_fwd_bits"])
def test_lif_fwd_second_pass(dev, cid):
    a = sc.CASES[cid]["args"]
    N, T, dt = a["N"], a["T"], a["spike_dtype"]
    x, v0 = rand_inputs(T, N, 5)
    xd = x.to(dev)
    for tau, vth, vr in ((2.0, 1.0, 0.0), (3.0, 1.0, -0.25)):
        bad_s, bad_v, pad = run_lif_fwd(dev, x, v0, tau, vth, vr, dt, xd=xd)
        tally("lif_fwd_second_pass", neuron_steps=T * N, spike_mismatches=bad_s, v_mismatches=bad_v, pad_bits_set=pad)
        assert (bad_s, bad_v, pad) == (0, 0, 0), (cid, tau)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("which", ["x", "v"])
def test_lif_fwd_misaligned_view(dev, which, off):
    """N % 4 == 0 and x_seq or v a contiguous view 4 * off bytes into its allocation: the scalar kernel, the view itself updated,
    nothing written around it."""
    N, T = sc.MISALIGNED_N, 3
    assert sc.CASES[f"lif_fwd_{which}_plus{off}"]["args"]["N"] == N
    x, v0 = rand_inputs(T, N, 40 + off)
    for tau, vth, vr in ((2.0, 1.0, 0.0), (3.0, 1.0, -0.25)):
        for dt in DTYPES:
            xd, xb = view_at(x, dev, off) if which == "x" else (x.to(dev), None)
            vd, vb = view_at(v0, dev, off) if which == "v" else (v0.clone().to(dev), None)
            bad_s, bad_v, pad = run_lif_fwd(dev, x, v0, tau, vth, vr, dt, xd=xd, vd=vd)
            tally("lif_fwd_misaligned", neuron_steps=T * N, spike_mismatches=bad_s, v_mismatches=bad_v, pad_bits_set=pad)
            assert (bad_s, bad_v, pad) == (0, 0, 0), (which, off, tau, dt)
            assert vb is None or guards_intact(vb, off, N)
            assert xb is None or (guards_intact(xb, off, T * N) and torch.equal(xd.cpu(), x))


def test_lif_fwd_state_is_advanced_in_place_or_refused(dev):
    """A contiguous v is the tensor the kernel advances; a transposed one is refused (a copy would take the update)."""
    x, v0 = rand_inputs(4, 6 * 10, 3)
    want = ref.lif_multi_step(x, v0.clone())
    want_ex = ref.lif_multi_step_ex(x, v0.clone())
    for fn in (ops.lif_fwd, ops.lif_fwd_ex):
        v = v0.clone().to(dev).view(6, 10)
        ptr = v.data_ptr()
        fn(x.view(4, 6, 10).to(dev), v)
        assert v.data_ptr() == ptr and same_bits(v.cpu().flatten(), want[1]) and same_bits(want[1], want_ex[1])
        assert not torch.equal(v.cpu().flatten(), v0)
        vt = v0.clone().to(dev).view(10, 6).t()
        before = vt.clone()
        with pytest.raises(ValueError, match="in place.*contiguous"):
            fn(x.view(4, 6, 10).to(dev), vt)
        assert torch.equal(vt, before)


# ------------------------------------------------------------------------------------------ (b) threshold ties, non-finite inputs
def edge_inputs(N, tau, vr, seed=0):
    """[5, N] inputs and [N] initial states whose first columns put h exactly on v_th = 1 and just either side of it, in every
    form of the neuron, at step 0 and again later (a constant input after a reset; the same values at step 2 of a random
    column), and NaN / +inf / -inf at step 0 and at step 2."""
    T = 5
    x, v0 = rand_inputs(T, N, 900 + seed)
    one = torch.tensor(1.0)
    cols = []
    for start in (vr, 0.0):                                  # initial state: the reset potential, or 0 (the soft-reset forms)
        for xt in (tau * (1.0 - vr), 1.0 - vr, tau, 1.0):    # h == 1: hard+decay from v_reset; hard, no decay; soft+decay from 0; soft
            xt = torch.tensor(xt, dtype=torch.float32)
            for val in (xt, torch.nextafter(xt, 0 * one), torch.nextafter(xt, 1e9 * one)):
                cols.append((start, float(val)))
    k = 0
    for start, val in cols:                                  # the value at every step
        x[:, k] = val; v0[k] = start; k += 1
    for start, val in cols:                                  # the value at step 2 only
        x[2, k] = val; k += 1
    for t in (0, 2):
        for val in (NAN, INF, -INF):
            x[t, k] = val; k += 1
    assert k <= N
    return x, v0, k


@pytest.mark.parametrize("N", [64, 67])
@pytest.mark.parametrize("tau,vr", [(2.0, 0.0), (2.0, -0.25), (3.0, 0.0), (3.0, -0.25)])
def test_threshold_ties_and_nonfinite_inputs(dev, N, tau, vr):
    x, v0, k = edge_inputs(N, tau, vr)
    T = x.shape[0]
    # the inputs do what they are for: h lands on the threshold, and one ulp either side of it at tau = 2, v_reset = 0
    _, h, _ = sc.lif_train_fwd_f32(x, v0, 1.0, vr, tau)
    one = torch.tensor(1.0)
    assert int((h[:, :k] == 1.0).sum()) >= 3
    if (tau, vr) == (2.0, 0.0):
        assert bool((h[0, :k] == torch.nextafter(one, 0 * one)).any()) and bool((h[0, :k] == torch.nextafter(one, 2 * one)).any())
    xd = x.to(dev)
    # spk_lif_fwd, three dtypes
    want = ref.lif_multi_step(x, v0.clone(), 1.0, vr, tau)
    assert bool(torch.isnan(want[1]).any())
    for dt in DTYPES:
        bad_s, bad_v, pad = run_lif_fwd(dev, x, v0, tau, 1.0, vr, dt, want, xd=xd)
        tally("edges_lif_fwd", neuron_steps=T * N, spike_mismatches=bad_s, v_mismatches=bad_v, pad_bits_set=pad)
        assert (bad_s, bad_v, pad) == (0, 0, 0), dt
    # spk_lif_fwd_ex, four forms
    for soft in (False, True):
        for decay in (False, True):
            ws, wv, wvs = ref.lif_multi_step_ex(x, v0.clone(), 1.0, None if soft else vr, tau, decay)
            for want_v_seq in (False, True):
                vd = v0.clone().to(dev)
                poison(dev, T * N, T * N)
                s, v_seq = ops.lif_fwd_ex(xd, vd, tau, 1.0, vr, soft, decay, want_v_seq)
                bad = (int((s.cpu() != ws).sum()), diff_bits(vd.cpu(), wv), diff_bits(v_seq.cpu(), wvs) if want_v_seq else 0)
                tally("edges_lif_fwd_ex", neuron_steps=T * N, spike_mismatches=bad[0], v_mismatches=bad[1], v_seq_mismatches=bad[2])
                assert bad == (0, 0, 0), (soft, decay, want_v_seq)
    # spk_lif_train_fwd
    with torch.no_grad():
        so, vo = ref.lif_multi_step_train(x, v0.clone(), 1.0, vr, tau)
    ss, hs, vs = sc.lif_train_fwd_f32(x, v0, 1.0, vr, tau)
    assert torch.equal(ss, so) and same_bits(vs, vo)
    poison(dev, T * N, T * N, N)
    s, hd, vl = ops.lif_train_fwd(xd, v0.to(dev), tau, 1.0, vr)
    bad = (int((s.cpu() != so).sum()), diff_bits(hd.cpu(), hs), diff_bits(vl.cpu(), vo))
    tally("edges_lif_train_fwd", neuron_steps=T * N, spike_mismatches=bad[0], h_mismatches=bad[1], v_mismatches=bad[2])
    assert bad == (0, 0, 0)


# -------------------------------------------------------------------------------------------------------- (c) spk_lif_fwd_ex
def run_lif_fwd_ex(dev, x, v0, tau, vr, soft, decay, want_v_seq, xd=None, vd=None):
    T, N = x.shape
    ws, wv, wvs = ref.lif_multi_step_ex(x, v0.clone(), 1.0, None if soft else vr, tau, decay)
    xd = x.to(dev) if xd is None else xd
    vd = v0.clone().to(dev) if vd is None else vd
    poison(dev, T * N, T * N)
    s, v_seq = ops.lif_fwd_ex(xd, vd, tau, 1.0, vr, soft, decay, want_v_seq)
    assert (v_seq is None) == (not want_v_seq)
    bad = (int((s.cpu() != ws).sum()), diff_bits(vd.cpu(), wv), diff_bits(v_seq.cpu(), wvs) if want_v_seq else 0)
    return bad


FORMS = [(False, True), (False, False), (True, True), (True, False)]            # (soft_reset, decay_input)


@pytest.mark.parametrize("soft,decay", FORMS)
def test_lif_fwd_ex_small_family(dev, soft, decay):
    for N in sc.SMALL_N:
        for T in (1, 9):
            x, v0 = rand_inputs(T, N, N * 7 + T)
            for tau, vr in ((2.0, 0.0), (3.0, -0.25)):
                for want_v_seq in (False, True):
                    bad = run_lif_fwd_ex(dev, x, v0, tau, vr, soft, decay, want_v_seq)
                    tally("lif_fwd_ex_small", neuron_steps=T * N, spike_mismatches=bad[0], v_mismatches=bad[1], v_seq_mismatches=bad[2])
                    assert bad == (0, 0, 0), (N, T, tau, vr, want_v_seq)


@pytest.mark.parametrize("soft,decay", FORMS)
def test_lif_fwd_ex_second_pass_and_misaligned(dev, soft, decay):
    a = sc.CASES["lif_fwd_ex"]["args"]
    x, v0 = rand_inputs(a["T"], a["N"], 77)
    xd = x.to(dev)
    for tau, vr, want_v_seq in ((3.0, -0.25, True), (2.0, 0.0, False)):
        bad = run_lif_fwd_ex(dev, x, v0, tau, vr, soft, decay, want_v_seq, xd=xd)
        tally("lif_fwd_ex_second_pass", neuron_steps=x.numel(), spike_mismatches=bad[0], v_mismatches=bad[1], v_seq_mismatches=bad[2])
        assert bad == (0, 0, 0), (tau, vr, want_v_seq)
    x, v0 = rand_inputs(3, sc.MISALIGNED_N, 78)
    xd, xb = view_at(x, dev, 1)
    vd, vb = view_at(v0, dev, 2)
    bad = run_lif_fwd_ex(dev, x, v0, 3.0, -0.25, soft, decay, True, xd=xd, vd=vd)
    tally("lif_fwd_ex_misaligned", neuron_steps=x.numel(), spike_mismatches=bad[0], v_mismatches=bad[1], v_seq_mismatches=bad[2])
    assert bad == (0, 0, 0) and guards_intact(vb, 2, v0.numel()) and guards_intact(xb, 1, x.numel())


# ------------------------------------------------------------------------------ (d) spk_lif_train_fwd / spk_lif_train_bwd
ALPHA = 2.0


def sample_columns(cid):
    """The neurons of a second-pass case on which the fp64 recurrences are evaluated (the host takes seconds for all of them): the
    first 65 536, everything from 65 536 before the end of the first pass to N (the pass boundary and the whole second pass),
    and every 509th in between.  The fp32 forward outputs are compared on all N, and all N of an adjoint must be written."""
    c = sc.CASES[cid]
    L, N = sc.launch(c), c["args"]["N"]
    pe = L["per_pass"] * L["vec"]
    assert 2 * 65536 < pe < N
    return torch.cat([torch.arange(0, 65536), torch.arange(65536, pe - 65536, 509), torch.arange(pe - 65536, N)])


def run_lif_train(dev, T, N, tau, vr, seed, configs, x_off=0, v_off=0, gs_off=0, h_off=0, gv_off=0, name="lif_train_small",
                  cols=None):
    """Forward against the fp32 restatement bit for bit; then for every (detach_reset, with grad_v_last) of ``configs`` the
    backward on the kernel's own h_seq against the fp64 recurrence within the counted bound (on the neurons ``cols``; all of
    them by default), and once more with need_grad_v=False, which must leave grad_x as it was."""
    g = torch.Generator().manual_seed(seed)
    x, v0 = rand_inputs(T, N, seed)
    gs, gv = torch.randn(T, N, generator=g), torch.randn(N, generator=g)
    ss, hs, vs = sc.lif_train_fwd_f32(x, v0, 1.0, vr, tau)
    xd = view_at(x, dev, x_off)[0] if x_off else x.to(dev)
    vd = view_at(v0, dev, v_off)[0] if v_off else v0.to(dev)
    poison(dev, T * N, T * N, N)
    s, h, vl = ops.lif_train_fwd(xd, vd, tau, 1.0, vr)
    bad = (int((s.cpu() != ss).sum()), diff_bits(h.cpu(), hs), diff_bits(vl.cpu(), vs))
    tally(name, neuron_steps=T * N, spike_mismatches=bad[0], h_mismatches=bad[1], v_last_mismatches=bad[2])
    assert bad == (0, 0, 0), (T, N, tau, vr)
    assert T * N < 4096 or 0.02 < float(ss.mean()) < 0.98
    hb = None
    if h_off:
        h, hb = view_at(h.cpu(), dev, h_off)
    gsd = view_at(gs, dev, gs_off)[0] if gs_off else gs.to(dev)
    gvd = view_at(gv, dev, gv_off)[0] if gv_off else gv.to(dev)
    c = sc.BPTT_ROUNDINGS_PER_STEP
    steps = sc.steps_feeding(T, hs)
    sub = (lambda a: a) if cols is None else (lambda a: a[..., cols])
    gs_o, gv_o, hs_o = sub(gs), sub(gv), sub(hs)
    for det, with_gv in configs:
        poison(dev, T * N, N)
        gx, gv0 = ops.lif_train_bwd(gsd, gvd if with_gv else None, h, tau, 1.0, vr, ALPHA, det)
        wx, wv, Mx, Mv = sc.lif_bptt_f64(gs_o, gv_o if with_gv else None, hs_o, tau, 1.0, vr, ALPHA, det)
        gxc, gvc = gx.cpu(), gv0.cpu()
        assert not bool(torch.isnan(gvc).any())
        rx = sc.bound_ratio(sub(gxc), wx, c * steps * sc.EPS32 * Mx)
        rv = sc.bound_ratio(sub(gvc), wv, c * T * sc.EPS32 * Mv)
        print(f"lif_train_bwd T={T} N={N} tau={tau} vr={vr} detach={det} gv={with_gv}: err/bound grad_x {rx:.4f} grad_v {rv:.4f}")
        tally(name, max_grad_x_err_over_bound=rx, max_grad_v_err_over_bound=rv)
        assert rx <= 1.0 and rv <= 1.0, (T, N, tau, vr, det, with_gv, rx, rv)
        assert not bool(torch.isnan(gxc).any())
        poison(dev, T * N, N)
        gx2, none = ops.lif_train_bwd(gsd, gvd if with_gv else None, h, tau, 1.0, vr, ALPHA, det, need_grad_v=False)
        assert none is None and same_bits(gx2.cpu(), gxc)
    assert hb is None or guards_intact(hb, h_off, T * N)


ALL_BWD = [(False, True), (True, True), (False, False), (True, False)]         # (detach_reset, with grad_v_last)


@pytest.mark.parametrize("N", sc.SMALL_N)
def test_lif_train_small_family(dev, N):
    for T in (1, 9, 16):
        for tau, vr in ((2.0, 0.0), (3.0, -0.25), (2.0, -0.25), (3.0, 0.0)):
            run_lif_train(dev, T, N, tau, vr, N * 13 + T, ALL_BWD)


@pytest.mark.parametrize("cid", ["vec", "scalar"])
def test_lif_train_second_pass(dev, cid):
    a = sc.CASES["lif_train_fwd_" + cid]["args"]
    assert sc.CASES["lif_train_bwd_" + cid]["args"] == a
    run_lif_train(dev, a["T"], a["N"], 3.0, -0.25, 21, [(False, True), (True, False)], name="lif_train_second_pass",
                  cols=sample_columns("lif_train_bwd_" + cid))


@pytest.mark.parametrize("offs", [dict(x_off=1), dict(v_off=2), dict(gs_off=1), dict(h_off=3), dict(gv_off=2)],
                         ids=lambda d: "_".join(f"{k}{v}" for k, v in d.items()))
def test_lif_train_misaligned_view(dev, offs):
    run_lif_train(dev, 3, sc.MISALIGNED_N, 3.0, -0.25, 31, ALL_BWD, name="lif_train_misaligned", **offs)


# --------------------------------------------------------------------------------------------------------------- (e) spk_psp
def run_psp(dev, x, tau_s, name, xd=None, cols=None):
    T = x.shape[0]
    xd = x.to(dev) if xd is None else xd
    poison(dev, x.numel())
    y = ops.psp(xd, tau_s, False).cpu()
    bad = diff_bits(y.contiguous(), ref.psp_filter(x, tau_s).contiguous())
    poison(dev, x.numel())
    gx = ops.psp(xd, tau_s, True).cpu()
    assert not bool(torch.isnan(gx).any())
    if cols is not None:
        gx, x = gx[:, cols], x[:, cols]
    wx, Mx = sc.psp_adjoint_f64(x, tau_s)
    r = sc.bound_ratio(gx, wx, sc.PSP_ADJOINT_ROUNDINGS_PER_STEP * sc.steps_feeding(T, x) * sc.EPS32 * Mx)
    print(f"psp {tuple(x.shape)} tau_s={tau_s}: forward mismatches {bad}, adjoint err/bound {r:.4f}")
    tally(name, values=x.numel(), forward_mismatches=bad, max_adjoint_err_over_bound=r)
    assert bad == 0 and r <= 1.0, (tuple(x.shape), tau_s, bad, r)


@pytest.mark.parametrize("N", sc.SMALL_N)
def test_psp_small_family(dev, N):
    for T in (1, 7, 16):
        for tau_s in (2.0, 3.0):
            run_psp(dev, rand_inputs(T, N, N + T)[0], tau_s, "psp_small")


@pytest.mark.parametrize("cid", ["vec", "scalar"])
def test_psp_second_pass(dev, cid):
    a = sc.CASES["psp_fwd_" + cid]["args"]
    assert sc.CASES["psp_bwd_" + cid]["args"] == dict(a, backward=True)
    run_psp(dev, rand_inputs(a["T"], a["N"], 8)[0], 3.0, "psp_second_pass", cols=sample_columns("psp_bwd_" + cid))


def test_psp_misaligned_and_permuted(dev):
    x = rand_inputs(3, sc.MISALIGNED_N, 9)[0]
    for off in (1, 3):
        xd, xb = view_at(x, dev, off)
        run_psp(dev, x, 3.0, "psp_misaligned", xd=xd)
        assert guards_intact(xb, off, x.numel())
    # a dense permutation inside the planes goes to the kernel as it is (element-wise: any order inside a plane)
    x3 = rand_inputs(7, 60, 10)[0].view(7, 6, 10)
    xp, xd = x3.permute(0, 2, 1), x3.to(dev).permute(0, 2, 1)
    assert not xd.is_contiguous() and ops._dense_tn(xd, "inputs") is xd and torch.equal(xd.cpu(), xp)
    for tau_s in (2.0, 3.0):
        run_psp(dev, xp, tau_s, "psp_permuted", xd=xd)


# ------------------------------------------------------------------------------------------------------- (f) spk_bn_eval_fwd
def run_bn(dev, M, C, HW, seed, name, off=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, HW, generator=g) * 2
    a, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    want = ref.fma_f32(x, a.view(1, C, 1), b.view(1, C, 1))
    xd, xb = view_at(x, dev, off) if off else (x.to(dev), None)
    poison(dev, x.numel())
    y = ops.bn_eval(xd, a.to(dev), b.to(dev)).cpu()
    bad = diff_bits(y, want)
    tally(name, values=x.numel(), mismatches=bad)
    assert bad == 0, (M, C, HW, off, bad)
    assert xb is None or guards_intact(xb, off, x.numel())


@pytest.mark.parametrize("HW", [1, 3, 4, 49, 64])
def test_bn_eval_small_family(dev, HW):
    for C in (1, 3, 64):
        for M in (1, 5, 32):
            run_bn(dev, M, C, HW, HW * 100 + C + M, "bn_eval_small")


@pytest.mark.parametrize("cid", ["bn_eval_vec", "bn_eval_scalar"])
def test_bn_eval_second_pass(dev, cid):
    a = sc.CASES[cid]["args"]
    run_bn(dev, a["M"], a["C"], a["HW"], 6, "bn_eval_second_pass")


def test_bn_eval_misaligned_view(dev):
    a = sc.CASES["bn_eval_x_plus1"]["args"]
    for off in (1, 2, 3):
        run_bn(dev, a["M"], a["C"], a["HW"], 7 + off, "bn_eval_misaligned", off=off)


# -------------------------------------------------------------------------------------------------------- (g) spk_memout_fwd
def coef_of(T):
    return torch.pow(torch.tensor(0.8), torch.arange(T - 1, -1, -1).float())


def run_memout(dev, T, N, seed, name, off=0):
    x = rand_inputs(T, N, seed)[0]                      # products with 0.8^k are not representable: a fused multiply-add shows
    coef = coef_of(T)
    want = sc.memout_f32(x, coef)
    xd, xb = view_at(x, dev, off) if off else (x.to(dev), None)
    poison(dev, N)
    y = ops.memout(xd, coef.to(dev)).cpu()
    bad = diff_bits(y, want)
    tally(name, values=N, mismatches=bad)
    assert bad == 0, (T, N, off, bad)
    assert xb is None or guards_intact(xb, off, x.numel())


@pytest.mark.parametrize("T", [1, 16, 64])
def test_memout_small_family(dev, T):
    for N in sc.SMALL_N:
        run_memout(dev, T, N, T * 1000 + N, "memout_small")
    for off in (1, 2, 3):
        run_memout(dev, T, sc.MISALIGNED_N, T + off, "memout_misaligned", off=off)


def test_memout_refuses_more_than_64_steps(dev):
    assert sc.memout_launch(64, 65)["kernel"] == "refused"
    with pytest.raises(ValueError):
        ops.memout(torch.zeros(65, 64, device=dev), torch.ones(65, device=dev))


@pytest.mark.parametrize("cid", ["memout_vec", "memout_scalar"])
def test_memout_second_pass(dev, cid):
    a = sc.CASES[cid]["args"]
    run_memout(dev, a["T"], a["N"], 12, "memout_second_pass")


# ------------------------------------------------------------------------------------------- plane offsets past 2^31 elements
@pytest.fixture(scope="module")
def past_2g(dev):
    """sc.PAST_2G_T x sc.PAST_2G_N fp32 inputs generated on the device (the host oracle reads back blocks of columns)."""
    total, chunk = sc.PAST_2G_T * sc.PAST_2G_N, 1 << 28
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.empty(total, device=dev)
    for i in range(0, total, chunk):
        x[i:i + chunk].normal_(0.7, 1.5, generator=g)
    yield x
    del x
    torch.cuda.empty_cache()


def columns(t2d, blocks):
    return torch.cat([t2d[..., a:b].cpu() for a, b in blocks], dim=-1)


@pytest.mark.parametrize("dt", [ops.SPIKE_U8, ops.SPIKE_BITS], ids=["u8", "bits"])
def test_lif_fwd_plane_offset_past_2g(dev, past_2g, dt):
    """(T - 1) * N >= 2^31: the last planes of x_seq and of the spikes lie past what a 32-bit offset reaches."""
    T, N = sc.PAST_2G_T, sc.PAST_2G_N
    blocks = sc.past_2g_blocks(N)
    x = past_2g.view(T, N)
    g = torch.Generator(device=dev).manual_seed(2)
    v = torch.rand(N, generator=g, device=dev) - 0.5
    xs, v0 = columns(x, blocks), columns(v, blocks)
    want_s, want_v = ref.lif_multi_step(xs, v0.clone(), 1.0, -0.25, 3.0)
    s = ops.lif_fwd(x, v, 3.0, 1.0, -0.25, spike_dtype=dt)
    pad = 0
    if dt == ops.SPIKE_BITS:
        got = []
        for a, b in blocks:                                   # the words that hold columns a .. b-1
            w0, w1 = a // 64, (b + 63) // 64
            bits, _ = unpack_words(s[:, w0:w1], (w1 - w0) * 64)
            got.append(bits[:, a - w0 * 64:b - w0 * 64])
        got = torch.cat(got, dim=1)
        pad = unpack_words(s[:, -1:], N - (s.shape[1] - 1) * 64)[1]
    else:
        got = columns(s, blocks).float()
    bad = (int((got != want_s).sum()), diff_bits(columns(v, blocks), want_v), pad)
    tally("lif_fwd_past_2g", neuron_steps=want_s.numel(), spike_mismatches=bad[0], v_mismatches=bad[1], pad_bits_set=bad[2])
    assert bad == (0, 0, 0) and not bool(torch.isnan(v).any())
    assert 0.02 < float(want_s.mean()) < 0.98


def test_memout_plane_offset_past_2g(dev, past_2g):
    T, N = sc.PAST_2G_MEMOUT_T, sc.PAST_2G_MEMOUT_N
    blocks = sc.past_2g_blocks(N)
    x = past_2g.view(T, N)
    coef = coef_of(T)
    poison(dev, N)
    y = ops.memout(x, coef.to(dev))
    bad = diff_bits(columns(y, blocks), sc.memout_f32(columns(x, blocks), coef))
    tally("memout_past_2g", values=len(blocks) * sc.PAST_2G_BLOCK, mismatches=bad)
    assert bad == 0 and not bool(torch.isnan(y).any())
