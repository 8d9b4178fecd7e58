"""GPU tests of the plain-CNN VQVAE baseline's training step on HIP (run with ``-m gpu`` on an MI355X): the two
fused epilogues of csrc/conv_train.hip bit for bit against the plain gather launch, the quantiser and loss kernels of
csrc/ann_vqvae_train.hip against fp64 given the indices, the model's iteration against the fp64 oracle given the kernel's
decisions (tests/_ann_vqvae_train_oracle.py), the dispatch, the captured step and the loop of R/main.py:130-142.  Every
grid-stride loop of those kernels also runs past its first trip (the case tables derive the sizes from the caps in the sources;
tests/test_ann_vqvae_train_host.py checks that they are past them), the quantiser in its DC == 0 form at D != 16, and its own
arg min on ties, NaN and inf."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _ann_vqvae_oracle as orc             # noqa: E402
import _ann_vqvae_train_oracle as tor       # noqa: E402
import _conv_train_cases as ctc             # noqa: E402
from oracle import snn_ref                  # noqa: E402
from parity_report import record as parity  # noqa: E402
from spkdiff import synth                  # noqa: E402

NEW_ENTRY_POINTS = ("spk_conv_train_gather_relu", "spk_conv_train_gather_masked", "spk_ann_vqvae_train_vq_fwd",
                    "spk_ann_vqvae_train_vq_bwd", "spk_ann_vqvae_train_loss_fwd", "spk_ann_vqvae_train_loss_bwd")
POISON = 12345.0
SENTINEL = -7.5                             # what the guard bands around a workspace hold
GUARD = 4096
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ 1. epilogues
@pytest.mark.parametrize("cid,layer,N,op,epi", tor.epilogue_cases(), ids=[c[0] for c in tor.epilogue_cases()])
def test_epilogue_equals_the_plain_launch_bit_for_bit(dev, cid, layer, N, op, epi):
    from spkdiff import ops
    L = ops.lib
    cin, cout, k, stride, pad, tr = layer[:6]
    n, Hi, Wi, Cred, Ho, Wo, Cout, k, stride, pad, form = ctc.gather_args(layer, N, op)
    g = torch.Generator().manual_seed(1000 + N)
    x = torch.randn(n, Hi, Wi, Cred, generator=g)
    flat = x.reshape(-1)
    flat[1::97] = 0.0                                               # exact zeros among the operands
    flat[flat.numel() // 3] = float("nan")
    flat[flat.numel() // 2] = -0.0
    w = torch.randn((cin, cout, k, k) if tr else (cout, cin, k, k), generator=g) * 0.1
    tap, s_ci, s_co = ops._conv_w_strides(w, tr)
    w_red, w_out = (s_ci, s_co) if op == "fwd" else (s_co, s_ci)
    bias = torch.randn(Cout, generator=g) if op == "fwd" else None
    act = torch.randn(n, Ho, Wo, Cout, generator=g)
    act.reshape(-1)[::5] = 0.0                                      # entries that are exactly zero: cut, as threshold_backward cuts them
    act.reshape(-1)[2::11] = -0.0
    x, w, act = x.to(dev), w.to(dev), act.to(dev)
    bias = None if bias is None else bias.to(dev)
    numel = n * Ho * Wo * Cout
    geo = (n, Hi, Wi, Cred, Ho, Wo, Cout, k, stride, pad, form, tap, w_red, w_out)
    st = torch.cuda.current_stream().cuda_stream

    def run(name, *extra):
        buf = torch.full((numel + 2 * GUARD,), POISON, device=dev)
        out = buf[GUARD:GUARD + numel]
        rc = getattr(L, name)(x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), *extra, out.data_ptr(), *geo, st)
        assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + numel:] == POISON).all()), f"{name} wrote outside its tensor"
        return out.clone()

    y = run("spk_conv_train_gather")
    assert not bool((y == POISON).any()), "the plain launch left an output element unwritten"
    assert bool(torch.isnan(y).any()) and bool((y < 0).any()) and bool((y > 0).any())
    zero = torch.zeros((), device=dev)
    if epi == "relu":
        got = run("spk_conv_train_gather_relu")
        want = torch.where(y < 0, zero, y)                          # the issue's rule; a NaN stays NaN
        assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(torch.relu(y), nan=-7.0))      # torch.relu's values
    else:
        got = run("spk_conv_train_gather_masked", act.data_ptr())
        want = torch.where(act.reshape(-1) <= 0, zero, y)
        assert int((want == 0).sum()) >= numel // 5
    assert torch.equal(_bits(got), _bits(want)), f"{cid}: {int((_bits(got) != _bits(want)).sum())} of {numel} elements differ"


# ------------------------------------------------------------------------------------------------ 2. quantiser and loss kernels
def _vq_case(kind, N, K, g, D=tor.D):
    cb = torch.randn(K, D, generator=g)
    if kind == "one_code":                                          # one code owns every row
        z = cb[5] + 0.01 * torch.randn(N, D, generator=g)
    elif kind == "few_codes":                                       # most codes unused
        z = cb[torch.randint(0, 3, (N,), generator=g) * 7] + 0.01 * torch.randn(N, D, generator=g)
    else:
        z = torch.randn(N, D, generator=g)
    return z, cb


def _guarded(dev, n, dtype=torch.float32, fill=POISON):
    """(buffer, its n middle elements): GUARD elements of ``fill`` on either side of what a kernel is handed."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n, fill=POISON):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


def _same_bits(a, b):
    """Equal bit for bit, except that any NaN equals any NaN (the payload a NaN carries is not part of the contract)."""
    a, b = a.reshape(-1), b.reshape(-1)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(a[~na]), _bits(b[~nb]))


def _vq_fwd(dev, zd, cbd, beta):
    """spk_ann_vqvae_train_vq_fwd on poisoned, guarded outputs and a workspace of exactly the bytes the library asks for, itself
    between guard bands -> (idx, e, loss)."""
    from spkdiff import ops
    L = ops.lib
    (N, D), K = zd.shape, cbd.shape[0]
    nb = int(L.spk_ann_vqvae_train_ws_bytes(N, 0))
    assert nb == 8 * tor.vq_fwd_launch(N, D, K)["ws_doubles"]
    ibuf, idx = _guarded(dev, N, torch.int64, -1)
    ebuf, e = _guarded(dev, N * D)
    loss = torch.full((1,), POISON, device=dev)
    wbuf, ws = _guarded(dev, nb // 8, torch.float64, SENTINEL)
    ws.fill_(NAN)                                                   # scratch: nothing is expected of its contents
    assert L.spk_ann_vqvae_train_vq_fwd(zd.data_ptr(), cbd.data_ptr(), idx.data_ptr(), e.data_ptr(), loss.data_ptr(), beta,
                                        ws.data_ptr(), nb, N, D, K, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert _intact(wbuf, nb // 8, SENTINEL), "the forward wrote outside the workspace it asked for"
    assert _intact(ibuf, N, -1) and _intact(ebuf, N * D), "the forward wrote outside idx or e"
    assert bool(((idx >= 0) & (idx < K)).all()), "an index is unwritten or outside [0, K)"
    assert not bool((e == POISON).any()) and not bool((loss == POISON).any()), "the forward left an output unwritten"
    return idx.clone(), e.clone().view(N, D), loss


def _vq_bwd(dev, ged, gl, zd, idx, cbd, beta):
    """spk_ann_vqvae_train_vq_bwd on poisoned, guarded outputs -> (gz, gcodebook); ged and gl may be None."""
    from spkdiff import ops
    (N, D), K = zd.shape, cbd.shape[0]
    zbuf, gz = _guarded(dev, N * D)
    cbuf, gcb = _guarded(dev, K * D)
    assert ops.lib.spk_ann_vqvae_train_vq_bwd(None if ged is None else ged.data_ptr(), None if gl is None else gl.data_ptr(),
                                              zd.data_ptr(), idx.data_ptr(), cbd.data_ptr(), beta, gz.data_ptr(), gcb.data_ptr(),
                                              N, D, K, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert _intact(zbuf, N * D) and _intact(cbuf, K * D), "the backward wrote outside its gradients"
    assert not bool((gz == POISON).any()) and not bool((gcb == POISON).any()), "the backward left a gradient element unwritten"
    return gz.clone().view(N, D), gcb.clone().view(K, D)


@pytest.mark.parametrize("kind,N,D,K", [c[:4] for c in tor.VQ_CASES], ids=[tor.vq_case_id(c) for c in tor.VQ_CASES])
def test_vq_kernels_meet_fp64_given_the_indices(dev, kind, N, D, K):
    from spkdiff import ops
    L = ops.lib
    assert L.spk_ann_vqvae_train_supported(D, K)
    g = torch.Generator().manual_seed(N + K + (0 if D == tor.D else 1000 * D))
    z, cb = _vq_case(kind, N, K, g, D)
    g_e = torch.randn(N, D, generator=g)
    beta, g_loss = 0.25, 0.75
    zd, cbd, ged = z.to(dev), cb.to(dev), g_e.to(dev)
    gl = torch.tensor([g_loss], device=dev)

    def run():
        idx, e, loss = _vq_fwd(dev, zd, cbd, beta)
        return (idx, e, loss) + _vq_bwd(dev, ged, gl, zd, idx, cbd, beta)

    idx, e, loss, gz, gcb = run()
    try:
        want_idx = ops.vq_argmin(zd, cbd)
    except (NotImplementedError, ValueError):                       # a width spk_vq_argmin does not take: the fp64 distances decide
        want_idx = None
        orc.check_indices(snn_ref.vq_distances_f64(z, cb), idx, f"vq {kind} N={N} D={D} K={K}")
    assert want_idx is not None or D != tor.D
    if want_idx is not None:
        assert torch.equal(idx, want_idx), "the training kernel and spk_vq_argmin choose different codes"
    used = int(idx.unique().numel())
    assert used == 1 if kind == "one_code" else used <= 3 if kind == "few_codes" else used > min(8, K - 1)
    if N > tor.SMALL_N:                                             # a row's index and value depend on that row alone
        idx_s, e_s, _ = _vq_fwd(dev, zd[:tor.SMALL_N].contiguous(), cbd, beta)
        assert torch.equal(idx[:tor.SMALL_N], idx_s) and torch.equal(_bits(e[:tor.SMALL_N]), _bits(e_s)), \
            f"the first {tor.SMALL_N} of {N} rows differ from a call on those rows alone"
    q = cbd[idx]
    assert torch.equal(_bits(e), _bits(zd + (q - zd))), "e is not the fp32 value z + (q - z)"
    r = tor.vq_reference(z, cb, idx, beta, g_e, g_loss)
    worst = {"loss": abs(float(loss) - r["loss"]) / r["loss_bound"],
             "gz": float(((gz.cpu().double() - r["gz"]).abs() / r["gz_bound"].clamp_min(1e-300)).max()),
             "gcb": float(((gcb.cpu().double() - r["gcb"]).abs() / r["gcb_bound"].clamp_min(1e-300))[r["gcb_bound"] > 0].max())}
    print(f"vq {kind} N={N} D={D} K={K}: {used} codes used; worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    parity(f"ann_vqvae_train_vq[{tor.vq_case_id((kind, N, D, K))}]", **worst)
    assert max(worst.values()) <= 1.0, worst
    unused = torch.ones(K, dtype=torch.bool)
    unused[idx.cpu().unique()] = False
    assert bool((gcb.cpu()[unused] == 0).all()) and int(unused.sum()) == K - used        # the dense gradient of nn.Embedding
    again = run()
    for a, b in zip((idx, e, loss, gz, gcb), again):
        assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)
    # NULL gradients are zeros
    gz0, gcb0 = _vq_bwd(dev, None, None, zd, idx, cbd, beta)
    assert not bool(gz0.any()) and not bool(gcb0.any())


def test_vq_kernels_stop_at_the_lds_ceiling(dev):
    """K = 244 is the largest codebook of D = 64 that fits in 64 KB of LDS (it runs: VQ_CASES); K = 245 is refused by the predicate
    and by the forward, which touches nothing."""
    from spkdiff import _lib, ops
    L, UNS = ops.lib, _lib.CONSTANTS["SPK_ERR_UNSUPPORTED"]
    D = tor.MAX_D
    K = max(tor.DC0_K)
    assert L.spk_ann_vqvae_train_supported(D, K) and not L.spk_ann_vqvae_train_supported(D, K + 1)
    assert ("random", tor.SMALL_N, D, K) in [c[:4] for c in tor.VQ_CASES]
    N = 49
    zd, cbd = torch.randn(N, D, device=dev), torch.randn(K + 1, D, device=dev)
    idx = torch.full((N,), -1, dtype=torch.int64, device=dev)
    e = torch.full((N, D), POISON, device=dev)
    loss = torch.full((1,), POISON, device=dev)
    ws = torch.full((N,), SENTINEL, dtype=torch.float64, device=dev)
    assert L.spk_ann_vqvae_train_vq_fwd(zd.data_ptr(), cbd.data_ptr(), idx.data_ptr(), e.data_ptr(), loss.data_ptr(), 0.25,
                                        ws.data_ptr(), N * 8, N, D, K + 1, torch.cuda.current_stream().cuda_stream) == UNS
    torch.cuda.synchronize()
    assert bool((idx == -1).all()) and bool((e == POISON).all()) and bool((loss == POISON).all()) and bool((ws == SENTINEL).all())


# ---- the kernel's own arg min (its copy of vq_kernel's lane loop): ties, NaN and inf, as tests/test_gpu_vq_shapes.py pins them
# for spk_vq_argmin.  The index is torch.argmin's on the fp64 distances of oracle/snn_ref.py -- the first NaN, else the first
# minimum -- and always in [0, K); D = 16 is the DC form, D = 24 the DC == 0 form; K = 37 < 64 leaves lanes on the clamped code.
ARGMIN_FORMS = [(16, 128), (24, 128), (16, 37), (24, 37)]


def _argmin64(z, cb):
    return torch.argmin(snn_ref.vq_distances_f64(z, cb), dim=1)


@pytest.mark.parametrize("D,K", ARGMIN_FORMS)
def test_vq_fwd_ties_take_the_lower_index(dev, D, K):
    """Duplicate codes at (k, k + 1), (k, k + 64) (the same lane) and (k, K - 1), with rows placed on them: the lower index wins,
    the row's value is the row itself, and the twin that lost gets an exactly-zero gradient."""
    g = torch.Generator().manual_seed(77 + D + K)
    N = 3 * 49
    z, cb = torch.randn(N, D, generator=g), torch.randn(K, D, generator=g)
    pairs = [(3, 4), (20, K - 1)] + ([(10, 74)] if K > 74 else [])
    want = {}
    for j, (a, b) in enumerate(pairs):
        p = 5 + 11 * j
        cb[a] = cb[b] = z[p]
        want[p] = a
    zd, cbd = z.to(dev), cb.to(dev)
    idx, e, loss = _vq_fwd(dev, zd, cbd, 0.25)
    assert torch.equal(idx.cpu(), _argmin64(z, cb))
    for p, a in want.items():
        assert int(idx[p]) == a, (p, int(idx[p]), a)
        assert torch.equal(_bits(e[p]), _bits(zd[p]))
    gz, gcb = _vq_bwd(dev, None, torch.ones(1, device=dev), zd, idx, cbd, 0.25)
    for a, b in pairs:
        assert not bool(gcb[b].any()), f"code {b}, the twin of {a}, is no row's code and has a gradient"
    flat = torch.full((K, D), 0.25, device=dev)                     # every code equal: index 0 everywhere
    idx, e, loss = _vq_fwd(dev, zd, flat, 0.25)
    assert int(idx.abs().max()) == 0


@pytest.mark.parametrize("D,K,N", [(16, 100, tor.N_PAST_FWD[16]), (24, 37, tor.SMALL_N)])
def test_vq_nan_and_inf_rows_stay_in_their_rows(dev, D, K, N):
    """Rows with one NaN component, rows of NaN and rows of +-inf (generated; every index comes from the forward).  Forward: the
    index is torch.argmin's, e and the loss carry the NaN.  Backward: gz is non-finite exactly where z is, gcodebook exactly in
    the components of the chosen codes that a non-finite component fed, and every other entry is within its counted bound of
    the fp64 reference without those components' contribution (z = q there)."""
    g = torch.Generator().manual_seed(D + K)
    z = torch.randn(N, D, generator=g)
    z[::7, D // 2] = NAN
    z[3::11] = NAN
    z[5::13] = INF
    z[6::17] = -INF
    cb = torch.randn(K, D, generator=g)
    g_e = torch.randn(N, D, generator=g)
    beta, g_loss = 0.25, 0.75
    zd, cbd, ged = z.to(dev), cb.to(dev), g_e.to(dev)
    idx, e, loss = _vq_fwd(dev, zd, cbd, beta)
    want = _argmin64(z, cb)
    bad = (idx.cpu() != want).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {N} indices differ from torch.argmin's, first rows {bad[:8].tolist()}"
    assert int(idx[0]) == 0 and int(idx[3]) == 0 and idx.unique().numel() > 8       # every distance of a NaN row is NaN: code 0
    assert _same_bits(e, zd + (cbd[idx] - zd)), "e is not the fp32 value z + (q - z)"
    finite = torch.isfinite(z)
    assert torch.equal(torch.isnan(e).cpu(), ~finite) and bool(torch.isnan(loss).all())
    gz, gcb = _vq_bwd(dev, ged, torch.tensor([g_loss], device=dev), zd, idx, cbd, beta)
    gz, gcb, idx = gz.cpu(), gcb.cpu(), idx.cpu()
    assert torch.equal(~torch.isfinite(gz), ~finite), "gz is non-finite somewhere else than z"
    assert bool(torch.isnan(gz)[torch.isnan(z)].all())
    fed = torch.zeros(K, D).index_add_(0, idx, (~finite).float()) > 0
    assert torch.equal(~torch.isfinite(gcb), fed), "gcodebook is non-finite somewhere else than where a non-finite component went"
    assert set(fed.any(dim=1).nonzero().flatten().tolist()) == set(idx[~finite.all(dim=1)].unique().tolist())
    r = tor.vq_reference(torch.where(finite, z, cb[idx]), cb, idx, beta, g_e, g_loss)
    worst = {"gz": float(((gz.double() - r["gz"]).abs() / r["gz_bound"].clamp_min(1e-300))[finite].max()),
             "gcb": float(((gcb.double() - r["gcb"]).abs() / r["gcb_bound"].clamp_min(1e-300))[~fed & (r["gcb_bound"] > 0)].max())}
    print(f"vq nan rows N={N} D={D} K={K}: {int((~finite.all(dim=1)).sum())} bad rows, codes fed {int(fed.any(dim=1).sum())}; "
          "worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    parity(f"ann_vqvae_train_vq[nan_rows-{N}-{D}-{K}]", **worst)
    assert max(worst.values()) <= 1.0, worst
    unused = torch.ones(K, dtype=torch.bool)
    unused[idx.unique()] = False
    assert bool((gcb[unused] == 0).all())


@pytest.mark.parametrize("D,K", ARGMIN_FORMS)
def test_vq_fwd_nan_and_inf_codes(dev, D, K):
    """A NaN code row (every distance to it NaN: it is every row's code unless an earlier distance is NaN) and an inf row before
    it: its distance is NaN where the signs cancel inf against inf, and +inf for the rows whose every product with it is -inf
    (every third row is given those signs) -- those rows take the NaN code, or, once it is gone, a finite one."""
    g = torch.Generator().manual_seed(9 + D + K)
    N = 3 * 49
    z, cb = torch.randn(N, D, generator=g), torch.randn(K, D, generator=g)
    k_inf, k_nan = (40, 90) if K > 90 else (10, 30)
    cb[k_inf] = INF
    cb[k_inf, 1::2] = -INF
    cb[k_nan, 2] = NAN
    z[::3] = z[::3].abs() * torch.tensor([-1.0, 1.0]).repeat(D // 2)
    zd = z.to(dev)
    for book in (cb, torch.cat([cb[:k_nan], torch.full((1, D), 0.5), cb[k_nan + 1:]])):     # ... and the inf row alone
        cbd = book.to(dev)
        idx, e, loss = _vq_fwd(dev, zd, cbd, 0.25)
        assert torch.equal(idx.cpu(), _argmin64(z, book))
        chosen = set(idx.cpu().unique().tolist())
        assert chosen == {k_inf, k_nan} if book is cb else (k_inf in chosen and len(chosen) > 4)        # (the inputs' variety)
        assert bool((idx[1::3] == k_inf).all()) and not bool((idx[::3] == k_inf).any())
        assert _same_bits(e, zd + (cbd[idx] - zd)) and not bool(torch.isfinite(loss).any())


LOSS_CASES = [c[:3] for c in tor.LOSS_CASES]


@pytest.mark.parametrize("B,C,H", LOSS_CASES)
def test_loss_kernels_meet_fp64(dev, B, C, H):
    from spkdiff import ops
    L = ops.lib
    g = torch.Generator().manual_seed(B * 100 + C)
    x = torch.rand(B, C, H, H, generator=g) - 0.5
    xr = x + 0.3 * torch.randn(B, C, H, H, generator=g)             # logical NCHW
    dv, g_recon, g_real = 0.0625, 1.0, 0.5
    xd = x.to(dev)
    xr_cl = xr.to(dev).permute(0, 2, 3, 1).contiguous()              # the kernel's channels-last reconstruction
    dvd, grd, gld = (torch.tensor([v], device=dev) for v in (dv, g_recon, g_real))
    st = torch.cuda.current_stream().cuda_stream
    n = x.numel()
    nb = int(L.spk_ann_vqvae_train_ws_bytes(0, n))
    assert nb == 8 * tor.loss_fwd_launch(B, C, H)["ws_doubles"]

    def backward(g_recon_ptr, g_real_ptr):
        gbuf, gx = _guarded(dev, n)
        assert L.spk_ann_vqvae_train_loss_bwd(xr_cl.data_ptr(), xd.data_ptr(), g_recon_ptr, g_real_ptr, dvd.data_ptr(), gx.data_ptr(),
                                              B, C, H, H, st) == 0
        torch.cuda.synchronize()
        assert _intact(gbuf, n), "the backward wrote outside its gradient"
        assert not bool((gx == POISON).any()), "the backward left a gradient element unwritten"
        return gx.clone().view(B, H, H, C)

    def run():
        obuf, out = _guarded(dev, 2)
        wbuf, ws = _guarded(dev, nb // 8, torch.float64, SENTINEL)  # exactly the bytes the library asks for, between guard bands
        ws.fill_(NAN)
        assert L.spk_ann_vqvae_train_loss_fwd(xr_cl.data_ptr(), xd.data_ptr(), dvd.data_ptr(), out[0:].data_ptr(), out[1:].data_ptr(),
                                              ws.data_ptr(), nb, B, C, H, H, st) == 0
        torch.cuda.synchronize()
        assert _intact(wbuf, nb // 8, SENTINEL), "the forward wrote outside the workspace it asked for"
        assert _intact(obuf, 2) and not bool((out == POISON).any())
        return out.clone(), backward(grd.data_ptr(), gld.data_ptr())

    out, gx = run()
    # a gradient element depends on its own pair alone: the first image's, from the kernel's c in fp32 on the host
    c = (np.float32(g_recon) / np.float32(dv) + np.float32(g_real)) * (np.float32(2.0) / np.float32(n))
    want0 = torch.tensor(c) * (xr[0].permute(1, 2, 0).contiguous() - x[0].permute(1, 2, 0).contiguous())
    assert want0.dtype == torch.float32 and torch.equal(_bits(gx[0].cpu()), _bits(want0)), "the first image's gradient is not c (xr - x)"
    r = tor.loss_reference(xr, x, dv, g_recon, g_real)
    worst = {"recon": abs(float(out[0]) - r["recon"]) / r["recon_bound"], "real": abs(float(out[1]) - r["real"]) / r["bound"],
             "g": float(((gx.permute(0, 3, 1, 2).cpu().double() - r["g"]).abs() / r["g_bound"].clamp_min(1e-300)).max())}
    print(f"loss B={B} C={C} H={H}: worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    parity(f"ann_vqvae_train_loss[{B}-{C}-{H}]", **worst)
    assert max(worst.values()) <= 1.0, worst
    out2, gx2 = run()
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(gx), _bits(gx2))
    assert not bool(backward(None, None).any())                     # NULL gradients are zeros


# ---------------------------------------------------------------------------------------------------------------- 3. the model
def _build(case, dev, dtype=torch.float32, data_variance=None):
    from snn_model.vae_model import VQVAE
    sd, images, dv, K, in_dim = tor.model_inputs(case)
    m = VQVAE(in_dim, tor.D, K, torch.tensor(dv) if data_variance is None else data_variance)
    m.load_state_dict(sd)
    m.fused_train = True                                            # (whatever the class's default is)
    return m.to(dev).to(dtype).train(), sd, images, dv


def _tensor_errors(grads, grads64):
    """{name: (max |g - g64|, max |g64|)} per parameter, on the entries the fixture keeps for the large ones."""
    out = {}
    for n, g64 in grads64.items():
        a, b = tor.grad_entries(grads[n]).astype(np.float64), tor.grad_entries(g64)
        out[n] = (float(np.abs(a - b).max()), float(np.abs(g64.numpy()).max()))
    return out


@pytest.mark.parametrize("case", tor.MODEL_CASES, ids=[c[0] for c in tor.MODEL_CASES])
def test_training_iteration_meets_the_fp64_oracle_given_its_decisions(dev, case):
    from spkdiff import ops
    m, sd, images, dv = _build(case, dev)
    x = images.to(dev)
    assert m._train_fused(x), "the case does not take the HIP path"
    loss_eq, loss_rec, real = m(x)
    assert type(loss_eq.grad_fn).__name__.startswith("ANNVQVAETrainFunction")
    (loss_eq + loss_rec).backward()
    # the record of the same forward (the kernels are deterministic: the same values as the model's call)
    params = m._enc_params() + m._dec_params() + (m.vq_layer.embeddings.weight,)
    vals, rec = ops.ann_vqvae_train_forward(x, params[:6], params[6:12], params[12], m.vq_layer.commitment_cost, m.data_variance)
    for a, b in zip((loss_eq, loss_rec, real), vals):
        assert torch.equal(_bits(a.detach()), _bits(b))
    for k in ("a1", "a2", "z", "e", "d1", "d2", "x_recon"):
        assert rec[k].permute(0, 2, 3, 1).is_contiguous(), k                      # channels-last
    rep = tor.check_decisions(sd, rec, case[0])
    losses64, grads64 = tor.train64(sd, images, tor.masks_of(rec), rec["idx"], 0.25, dv)
    got = {"loss_eq": float(loss_eq.detach()), "loss_rec": float(loss_rec.detach()), "real_loss_rec": float(real.detach())}
    grads = {n: p.grad for n, p in m.named_parameters()}
    assert all(g is not None for g in grads.values())
    errs = _tensor_errors(grads, grads64)
    if case[0] == "f20":
        f = orc.fixture()
        lbound = {k: 8 * float(f["err_loss/" + k]) for k in got}
        gbound = {n: 8 * float(f["err_grad/" + n]) for n in grads}
    else:
        # the reference operators' own error, like with like: the CPU module path in fp32 against train64 given ITS decisions
        from snn_model.vae_model import VQVAE
        ref = VQVAE(m.in_dim, tor.D, m.num_embeddings, torch.tensor(dv))
        ref.load_state_dict(sd)
        ref.train()
        (r_eq, r_rec, r_real), r_masks, r_idx = tor.module_path_decisions(ref, images)
        (r_eq + r_rec).backward()
        r64, rg64 = tor.train64(sd, images, r_masks, r_idx, 0.25, dv)
        rl = {"loss_eq": float(r_eq.detach()), "loss_rec": float(r_rec.detach()), "real_loss_rec": float(r_real.detach())}
        lbound = {k: 8 * max(abs(rl[k] - r64[k]), tor.EPS * abs(r64[k])) for k in got}
        rerr = _tensor_errors({n: p.grad for n, p in ref.named_parameters()}, rg64)
        gbound = {n: 8 * max(rerr[n][0], tor.EPS * errs[n][1]) for n in grads}
    lines, worst = [], 0.0
    for k in got:
        ratio = abs(got[k] - losses64[k]) / lbound[k]
        lines.append(f"{k}: {got[k]:.9g} vs fp64 {losses64[k]:.9g}: err {abs(got[k] - losses64[k]):.3g}, bound {lbound[k]:.3g}")
        worst = max(worst, ratio)
    for n in grads:
        lines.append(f"grad {n}: err {errs[n][0]:.3g}, bound {gbound[n]:.3g} (max |g64| {errs[n][1]:.3g})")
        worst = max(worst, errs[n][0] / gbound[n])
    print(f"{case[0]}: decisions {rep}\n  " + "\n  ".join(lines))
    parity(f"ann_vqvae_train_model[{case[0]}]", worst_err_over_bound=worst, **rep)
    for k in got:
        assert abs(got[k] - losses64[k]) <= lbound[k], (k, lines)
    for n in grads:
        assert errs[n][0] <= gbound[n], (n, lines)
        if case[0] == "f20" and grads[n].numel() > orc.SUB:
            f = orc.fixture()
            assert abs(float(grads[n].double().norm()) - float(grads64[n].norm())) <= 8 * float(f["err_gradnorm/" + n]), n
    for n, p in m.named_parameters():
        assert p.grad.shape == p.shape and p.grad.stride() == p.stride(), n     # each weight's memory format
    with pytest.raises(RuntimeError):
        (loss_eq + loss_rec).backward()                             # the record was freed by the first backward
    with torch.no_grad():
        nvals = m(x)
    assert all(v.grad_fn is None and not v.requires_grad for v in nvals)
    for a, b in zip((loss_eq, loss_rec, real), nvals):
        assert torch.equal(_bits(a.detach()), _bits(b))


def test_gradients_keep_a_channels_last_weights_memory_format(dev):
    m, sd, images, dv = _build(tor.MODEL_CASES[2], dev)
    l = m(images.to(dev))
    (l[0] + l[1]).backward()
    ref_grads = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    for mod in (m.encoder.convs[2], m.decoder.convs[2]):
        mod.weight.data = mod.weight.data.contiguous(memory_format=torch.channels_last)
    l = m(images.to(dev))
    assert type(l[0].grad_fn).__name__.startswith("ANNVQVAETrainFunction")
    (l[0] + l[1]).backward()
    for n, p in m.named_parameters():
        assert p.grad.stride() == p.stride(), n
        assert torch.equal(_bits(p.grad.contiguous()), _bits(ref_grads[n].contiguous())), n


def test_data_variance_may_be_a_number_a_cpu_tensor_or_a_device_tensor(dev):
    case = tor.MODEL_CASES[2]
    vals = []
    for dv in (0.0625, torch.tensor(0.0625), torch.tensor(0.0625, device=dev), torch.tensor([0.0625], dtype=torch.float64)):
        m, sd, images, _ = _build(case, dev, data_variance=dv)
        l = m(images.to(dev))
        (l[0] + l[1]).backward()
        vals.append([v.detach().clone() for v in l] + [m.decoder.convs[4].weight.grad.clone()])
    for other in vals[1:]:
        for a, b in zip(vals[0], other):
            assert torch.equal(_bits(a), _bits(b))
    assert abs(float(vals[0][1]) - float(vals[0][2]) / 0.0625) <= 2 * tor.EPS * float(vals[0][1])


# ---------------------------------------------------------------------------------------------------------------- 4. dispatch
class _Recorder:
    """Stands in for ops.lib: every entry point stays real, its name is logged."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("spk_"):
            self.calls.append(name)
        return fn


def _recorded(monkeypatch, fn):
    """(result or the exception fn raised, entry points issued, framework convolutions issued)"""
    from torch.utils._python_dispatch import TorchDispatchMode
    from spkdiff import ops
    rec = _Recorder(ops._lib.lib)
    convs = []

    class Mode(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if "conv" in str(func):
                convs.append(str(func))
            return func(*args, **(kwargs or {}))

    with monkeypatch.context() as mp:
        mp.setattr(ops, "lib", rec)
        try:
            with Mode():
                out = fn()
        except Exception as exc:                                    # noqa: BLE001  (the test compares the outcomes)
            out = exc
    return out, rec.calls, convs


def _module_path(m, x):
    """The reference's operators in the reference's order (VQVAE.forward's module branch)."""
    z = m.encoder(x)
    e, e_q_loss = m.vq_layer(z)
    x_recon = m.decoder(e)
    return e_q_loss, F.mse_loss(x_recon, x) / m.data_variance, F.mse_loss(x_recon, x)


def test_train_mode_call_issues_the_new_entry_points_and_no_framework_convolution(dev, monkeypatch):
    m, sd, images, dv = _build(tor.MODEL_CASES[2], dev)
    x = images.to(dev)

    def step():
        l = m(x)
        (l[0] + l[1]).backward()
        return l

    out, calls, convs = _recorded(monkeypatch, step)
    assert not isinstance(out, Exception), out
    assert not convs, convs
    count = {n: calls.count(n) for n in set(calls)}
    print("entry points of one iteration:", count)
    assert count["spk_conv_train_gather_relu"] == 4 and count["spk_conv_train_gather_masked"] == 4
    assert count["spk_conv_train_gather"] == 3                      # Conv 1x1 and ConvT 32->C forward, ConvT D->64's data gradient
    assert count["spk_conv_train_wgrad"] == 6
    for n in NEW_ENTRY_POINTS[2:]:
        assert count[n] == 1, n
    with torch.no_grad():
        out, calls, convs = _recorded(monkeypatch, lambda: m(x))
    assert not convs and "spk_conv_train_wgrad" not in calls and "spk_ann_vqvae_train_loss_fwd" in calls


@pytest.mark.parametrize("how", ["hook_on_a_child", "fused_train_false", "fp64_parameters", "image_30x30", "codebook_1024",
                                 "image_requires_grad"])
def test_other_calls_take_the_module_path_bit_for_bit(dev, monkeypatch, how):
    dtype = torch.float64 if how == "fp64_parameters" else torch.float32
    m, sd, images, dv = _build(tor.MODEL_CASES[2], dev, dtype=dtype)
    x = images.to(dev).to(dtype)
    handle = None
    if how == "codebook_1024":
        # the eval kernels take K up to 1024 (the model's eval forward is fused), the training quantiser's LDS image ends at 862
        from snn_model.vae_model import VQVAE
        from spkdiff import ops
        torch.manual_seed(3)
        m = VQVAE(1, tor.D, 1024, torch.tensor(dv)).to(dev).train()
        m.fused_train = True
        assert m._images_fused(x) and not ops.lib.spk_ann_vqvae_train_supported(tor.D, 1024) and not m._train_fused(x)
        m862 = VQVAE(1, tor.D, 862, torch.tensor(dv)).to(dev).train()
        assert m862._train_fused(x)
        l = m862(x)                                                 # the largest codebook the kernels take runs on them
        assert type(l[0].grad_fn).__name__.startswith("ANNVQVAETrainFunction")
        (l[0] + l[1]).backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m862.parameters())
    elif how == "image_requires_grad":
        x = x.clone().requires_grad_(True)
    if how == "hook_on_a_child":
        handle = m.decoder.convs[2].register_forward_hook(lambda *_: None)
    elif how == "fused_train_false":
        m.fused_train = False
    elif how == "image_30x30":
        x = F.pad(x, (1, 1, 1, 1)).contiguous()
    out, calls, convs = _recorded(monkeypatch, lambda: m(x))
    assert not set(calls) & set(NEW_ENTRY_POINTS) and "spk_conv_train_gather" not in calls, calls
    assert convs, "the module path runs the framework's convolutions"
    try:
        want = _module_path(m, x)
    except Exception as exc:                                        # noqa: BLE001  (a 30 x 30 image fails in the reference as well)
        want = exc
    if handle is not None:
        handle.remove()
    if isinstance(want, Exception):
        assert type(out) is type(want) and how == "image_30x30"
        return
    assert not isinstance(out, Exception), out
    for a, b in zip(out, want):
        assert a.dtype == dtype and torch.equal(a.detach(), b.detach())
    assert type(out[2].grad_fn).__name__ == "MseLossBackward0"
    if how in ("codebook_1024", "image_requires_grad"):            # and the iteration completes as it did before the kernels came
        (out[0] + out[1]).backward()
        assert all(p.grad is not None for p in m.parameters())
        assert how != "image_requires_grad" or (x.grad is not None and bool(x.grad.abs().sum() > 0))


# ---------------------------------------------------------------------------------------------------------- 5. captured step
def test_three_replays_equal_three_eager_iterations_bit_for_bit(dev):
    from spkdiff.train import GraphedANNVQVAETrainStep
    case = tor.MODEL_CASES[2]
    all_images = synth.stroke_images(12, img=synth.MNIST.img, channels=1) - 0.5
    example, batches = all_images[:3].to(dev), [all_images[3 + 3 * i:6 + 3 * i].to(dev) for i in range(3)]
    warmup = 2

    def make():
        m, *_ = _build(case, dev)
        return m, torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)

    eager, opt_e = make()
    eager_losses = []
    for b in [example] * warmup + batches:
        opt_e.zero_grad(set_to_none=True)
        l = eager(b)
        (l[0] + l[1]).backward()
        opt_e.step()
        eager_losses.append([v.detach().clone() for v in l])
    graphed, opt_g = make()
    with pytest.raises(RuntimeError, match="capturable"):
        GraphedANNVQVAETrainStep(graphed, torch.optim.AdamW(graphed.parameters(), lr=1e-3), example)
    # a model on its module path is refused where the framework's embedding backward would sort (more than 3072 rows), before
    # anything runs; the HIP path of the same batch is not
    many = torch.zeros(GraphedANNVQVAETrainStep.MODULE_PATH_MAX_ROWS // 49 + 1, 1, 28, 28, device=dev)
    graphed.fused_train = False
    with pytest.raises(RuntimeError, match="module path"):
        GraphedANNVQVAETrainStep(graphed, opt_g, many)
    assert not opt_g.state, "the refused step ran an iteration"
    graphed.fused_train = True
    assert graphed._train_fused(many)
    step = GraphedANNVQVAETrainStep(graphed, opt_g, example, warmup=warmup)
    for i, b in enumerate(batches):
        l = step(b)
        for a, want in zip(l, eager_losses[warmup + i]):
            assert torch.equal(_bits(a), _bits(want)), f"replay {i}: a loss differs from the eager iteration's"
    torch.cuda.synchronize()
    start = orc.state("mnist_k128")
    for (n, p), (_, q) in zip(graphed.named_parameters(), eager.named_parameters()):
        assert torch.equal(_bits(p.detach()), _bits(q.detach())), n
        assert not torch.equal(p.detach().cpu(), start[n]), n       # the weights moved
    # eval after the step sees the new weights
    graphed.eval()
    eager.eval()
    fresh, *_ = _build(case, dev)
    fresh.eval()
    with torch.no_grad():
        a, b, c = graphed(example), eager(example), fresh(example)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], c[1])


# --------------------------------------------------------------------------------------------------------- 6. the real loop
def test_the_loop_of_main_py_runs_and_the_loss_falls(dev):
    """R/main.py:130-142: zero_grad, model(images), (loss_eq + loss_rec).backward(), step."""
    from snn_model.vae_model import VQVAE
    cfg = synth.MNIST
    images = (synth.stroke_images(32, img=cfg.img, channels=cfg.in_dim) - 0.5).to(dev)
    dv = torch.tensor(float(images.var()))                          # a CPU tensor, as R/main.py:91-107 passes
    torch.manual_seed(7)
    m = VQVAE(cfg.in_dim, tor.D, 128, dv).to(dev).train()
    m.fused_train = True
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3)
    hist = []
    for it in range(20):
        opt.zero_grad()
        loss_eq, loss_rec, real = m(images)
        assert type(real.grad_fn).__name__.startswith("ANNVQVAETrainFunction")
        loss = loss_eq + loss_rec
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
    print("loss over 20 iterations:", " ".join(f"{v:.4f}" for v in hist))
    assert all(np.isfinite(hist)) and hist[-1] < hist[0] and min(hist[-3:]) < 0.9 * hist[0]
