"""GPU tests of the VQ kernels (csrc/vq.hip, csrc/vq_train.hip) against the fp64 host oracle (oracle/snn_ref.py, "VQ kernels"
section, pinned by tests/test_oracle_vq.py) at the shapes the model-level tests do not reach:
  * every grid-stride loop past its first pass: vq16_kernel above 65 536 positions, vq_kernel above 8 192, the training /
    loss kernels above 65 536 elements, embedding_kernel above 4096 x 256 elements;
  * the two-level sums with more than 128 block partials (quant loss, alpha gradient, PSP and reconstruction losses);
  * each code-search form: vq16_kernel (D = T = 16, K <= 455), vq_kernel<16> (T != 16, or 456 <= K <= 862), vq_kernel<0>;
  * ties inside one lane and across lanes, the LDS ceiling, and NaN / inf inputs, where the index must be torch.argmin's:
    the first NaN, else the first minimum, and always in [0, K).
Indices must equal the oracle's on every row, read-outs and gathers bit for bit; fp32 arithmetic is held to the fp64 oracle
by per-element bounds of a few fp32 roundings."""
import pytest
import torch

from oracle import snn_ref as ref
from spkdiff import ops

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
EPS32 = 2.0 ** -23
ALPHA = 0.37


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


def coef_of(T):
    return torch.pow(torch.tensor(0.8), torch.arange(T - 1, -1, -1).float())


def spikes_ptc(B, H, W, T, D, seed, p=0.3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, H, W, T, D, generator=g) < p).to(torch.uint8)


def codebook(K, D, seed, scale=0.9):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(K, D, generator=g) * scale


def same_bits(a, b):
    """Equal bit for bit, except that any NaN equals any NaN (the payload a NaN carries is not part of the contract)."""
    a, b = a.reshape(-1), b.reshape(-1)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def poison(dev, *numels):
    """Leave NaN-filled blocks of these sizes in the caching allocator, so that outputs a kernel fails to write are NaN
    rather than whatever an earlier call left there."""
    bufs = [torch.full((int(n),), NAN, device=dev) for n in numels]
    del bufs


def assert_in_range(idx, K):
    idx = idx.cpu()
    assert bool(((idx >= 0) & (idx < K)).all()), f"index out of [0, {K}): {idx[(idx < 0) | (idx >= K)][:8].tolist()}"


def run_readout(dev, z, coef, alpha, cb):
    """spk_vq_readout_argmin, first without the gather (range checked), then with the gather and read-out; all against the
    oracle.  Returns the device indices."""
    K, D = cb.shape
    B, H, W, T, _ = z.shape
    zd, cd, ad, cbd = z.to(dev), coef.to(dev), alpha.to(dev), cb.to(dev)
    idx0, _, _ = ops.vq_readout_argmin(zd, cd, ad, cbd, want_zq=False)
    assert_in_range(idx0, K)
    poison(dev, B * H * W * D)
    idx, zq, xm = ops.vq_readout_argmin(zd, cd, ad, cbd, want_zq=True, want_xm=True)
    want_xm = ref.vq_readout_f32(z, coef, alpha)
    assert same_bits(xm.cpu(), want_xm)
    want = ref.vq_argmin_f64(want_xm, cb)
    got = idx.cpu()
    assert torch.equal(idx0.cpu(), got)
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {want.numel()} indices differ, first rows {bad[:8].tolist()}"
    assert same_bits(zq.cpu(), cb[want].view(B, H, W, D).permute(0, 3, 1, 2).contiguous())
    return idx


def run_argmin(dev, x, cb):
    K = cb.shape[0]
    idx = ops.vq_argmin(x.to(dev), cb.to(dev)).cpu()
    assert_in_range(idx, K)
    want = ref.vq_argmin_f64(x, cb)
    bad = (idx != want).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {want.numel()} indices differ, first rows {bad[:8].tolist()}"
    return idx


# ------------------------------------------------------------------------------------------------ read-out and code search
VQ16_SMALL = [(1, 1, 1), (1, 5, 3), (16, 1, 1), (17, 1, 1), (3, 7, 7), (2, 8, 8)]     # 1, 15, 16, 17, 147, 128 positions


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 128, 455])
@pytest.mark.parametrize("B,H,W", VQ16_SMALL)
def test_vq16_readout(dev, B, H, W, K):
    run_readout(dev, spikes_ptc(B, H, W, 16, 16, B * 31 + H * 7 + W), coef_of(16), torch.tensor(ALPHA), codebook(K, 16, K))


@pytest.mark.parametrize("K", [1, 64, 65, 128])
@pytest.mark.parametrize("B", [1024, 1400])
def test_vq16_readout_past_the_grid(dev, B, K):
    """B = 1400 at 7x7 is 68 600 positions: more than vq16_kernel's 4096 workgroups x 16 take in one pass."""
    z = spikes_ptc(B, 7, 7, 16, 16, B + K)
    idx = run_readout(dev, z, coef_of(16), torch.tensor(ALPHA), codebook(K, 16, K + 1))
    if K > 1:
        assert idx.unique().numel() > 1
    # the same x_m through spk_vq_argmin (vq_kernel<0>) gives the same indices
    xm = ref.vq_readout_f32(z, coef_of(16), torch.tensor(ALPHA))
    assert torch.equal(ops.vq_argmin(xm.to(dev), codebook(K, 16, K + 1).to(dev)).cpu(), idx.cpu())


@pytest.mark.parametrize("T,K,B", [(1, 456, 257), (4, 512, 200), (4, 862, 257), (16, 456, 257), (16, 862, 200),
                                   (20, 512, 257), (20, 862, 257)])
def test_vq_kernel16_readout(dev, T, K, B):
    """vq_kernel<16>: T != 16, or 456 <= K <= 862 at T = 16 (vq16_kernel's fp64 codebook no longer fits in 64 KB); B = 200 and
    257 at 7x7 are 9 800 and 12 593 positions, past the 2048 x 4 of one pass."""
    run_readout(dev, spikes_ptc(B, 7, 7, T, 16, T * 1000 + K), coef_of(T), torch.tensor(ALPHA), codebook(K, 16, K))


@pytest.mark.parametrize("D", [1, 3, 8, 17, 48, 64])
@pytest.mark.parametrize("T", [3, 16])
def test_vq_kernel0_readout(dev, D, T):
    run_readout(dev, spikes_ptc(200, 7, 7, T, D, D * 10 + T), coef_of(T), torch.tensor(ALPHA), codebook(100, D, D))


@pytest.mark.parametrize("N", [1, 8191, 8192, 8193, 65537])
@pytest.mark.parametrize("D", [1, 3, 8, 17, 48, 64])
def test_vq_argmin_signed(dev, D, N):
    g = torch.Generator().manual_seed(D * 7 + N)
    x = torch.randn(N, D, generator=g) * 2.0
    cb = torch.randn(100, D, generator=g)
    idx = run_argmin(dev, x, cb)
    if N > 1000:
        assert idx.unique().numel() > 20


def tied_codebook(xm, K, pairs, seed):
    """A codebook whose pairs (a, b) are both equal to the read-out of a distinct position: that position's nearest code is a."""
    cb = codebook(K, xm.shape[1], seed)
    want = {}
    for j, (a, b) in enumerate(pairs):
        p = 5 + 11 * j
        cb[a] = cb[b] = xm[p]
        want[p] = a
    return cb, want


@pytest.mark.parametrize("form", ["vq16", "vq_kernel16", "vq_argmin"])
def test_vq_ties(dev, form):
    """Duplicate codes at (k, k + 1), (k, k + 64) (the same lane) and (k, K - 1): the lower index wins."""
    K, T = 128, (4 if form == "vq_kernel16" else 16)
    z = spikes_ptc(3, 7, 7, T, 16, 77 + T)
    xm = ref.vq_readout_f32(z, coef_of(T), torch.tensor(ALPHA))
    cb, want = tied_codebook(xm, K, [(3, 4), (10, 74), (20, K - 1)], 5)
    idx = (run_argmin(dev, xm, cb) if form == "vq_argmin" else run_readout(dev, z, coef_of(T), torch.tensor(ALPHA), cb)).cpu()
    for p, a in want.items():
        assert int(idx[p]) == a, (p, int(idx[p]), a)
    flat = torch.ones(K, 16) * 0.25                            # every code equal: index 0 everywhere
    idx = (run_argmin(dev, xm, flat) if form == "vq_argmin" else run_readout(dev, z, coef_of(T), torch.tensor(ALPHA), flat))
    assert int(idx.abs().max()) == 0


def test_vq_lds_ceiling_and_width_limits(dev):
    z = spikes_ptc(2, 7, 7, 16, 16, 1)
    c, a = coef_of(16).to(dev), torch.tensor(ALPHA, device=dev)
    run_readout(dev, z, coef_of(16), torch.tensor(ALPHA), codebook(862, 16, 3))
    with pytest.raises(NotImplementedError):
        ops.vq_readout_argmin(z.to(dev), c, a, codebook(863, 16, 3).to(dev))
    with pytest.raises(NotImplementedError):
        ops.vq_argmin(torch.rand(10, 16, device=dev), codebook(863, 16, 3).to(dev))
    with pytest.raises(ValueError):
        ops.vq_readout_argmin(spikes_ptc(2, 7, 7, 16, 65, 1).to(dev), c, a, codebook(8, 65, 3).to(dev))
    with pytest.raises(ValueError):
        ops.vq_argmin(torch.rand(10, 65, device=dev), codebook(8, 65, 3).to(dev))


# ------------------------------------------------------------------------------------------------ NaN and inf
@pytest.mark.parametrize("D", [16, 5])
def test_vq_argmin_nan_rows(dev, D):
    """Rows with one NaN component, rows of NaN and rows of inf: index 0 where every distance is NaN, torch.argmin's elsewhere."""
    g = torch.Generator().manual_seed(D)
    N, K = 9000, 100
    x = torch.randn(N, D, generator=g)
    x[::7, D // 2] = NAN
    x[3::11] = NAN
    x[5::13] = INF
    x[6::17] = -INF
    cb = torch.randn(K, D, generator=g)
    idx = run_argmin(dev, x, cb)
    assert int(idx[0]) == 0 and int(idx[3]) == 0 and int(idx[7]) == 0


@pytest.mark.parametrize("form", ["vq16", "vq_kernel16", "vq_kernel0", "vq_argmin"])
def test_vq_nan_and_inf_codes(dev, form):
    """A NaN code row (every distance to it NaN: it is every row's code unless an earlier distance is NaN) and an inf row before
    it (NaN where x has a zero or the signs cancel inf against inf, inf elsewhere)."""
    D = 5 if form == "vq_kernel0" else 16
    T = 4 if form == "vq_kernel16" else 16
    K = 128
    z = spikes_ptc(3, 7, 7, T, D, 9)
    cb = codebook(K, D, 9)
    cb[40] = INF
    cb[40, 1::2] = -INF
    cb[90, 2] = NAN
    xm = ref.vq_readout_f32(z, coef_of(T), torch.tensor(ALPHA))
    if form == "vq_argmin":
        xs = torch.randn(xm.shape, generator=torch.Generator().manual_seed(4))
        idx = run_argmin(dev, xs, cb)
    else:
        idx = run_readout(dev, z, coef_of(T), torch.tensor(ALPHA), cb)
    assert set(idx.cpu().unique().tolist()) <= {40, 90}
    only_inf = cb.clone()
    only_inf[90] = 0.5
    if form == "vq_argmin":
        run_argmin(dev, xs, only_inf)
    else:
        run_readout(dev, z, coef_of(T), torch.tensor(ALPHA), only_inf)


@pytest.mark.parametrize("form", ["vq16", "vq_kernel16", "vq_kernel0", "vq_argmin"])
def test_vq_all_inf_distances(dev, form):
    """x_m = -inf against a positive codebook: every distance is +inf, none is below another, so every index is 0 (torch.argmin's
    first minimum) -- the read-out gets there through coef[0] = -inf with every spike of step 0 set."""
    D = 5 if form == "vq_kernel0" else 16
    T = 4 if form == "vq_kernel16" else 16
    cb = codebook(100, D, 6) + 0.05
    if form == "vq_argmin":
        x = torch.randn(300, D, generator=torch.Generator().manual_seed(6))
        x[::3] = -INF
        idx = run_argmin(dev, x, cb)
        assert int(idx[::3].abs().max()) == 0
        return
    z = spikes_ptc(40, 7, 7, T, D, 6)
    z[:, :, :, 0] = 1
    coef = coef_of(T)
    coef[0] = -INF
    idx = run_readout(dev, z, coef, torch.tensor(ALPHA), cb)
    assert int(idx.abs().max()) == 0


@pytest.mark.parametrize("form", ["vq16", "vq_kernel16", "vq_kernel0"])
def test_vq_readout_nan_alpha(dev, form):
    """alpha = NaN (a diverged step): every x_m is NaN, every index 0 -- never an index past the codebook."""
    D = 5 if form == "vq_kernel0" else 16
    T = 4 if form == "vq_kernel16" else 16
    idx = run_readout(dev, spikes_ptc(40, 7, 7, T, D, 3), coef_of(T), torch.tensor(NAN), codebook(100, D, 3))
    assert int(idx.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ training branch
def train_codebook(kind, K, D, seed):
    cb = codebook(K, D, seed, scale=1.2)
    if kind == "one_code":                                     # code 1 nearest to every row, the others far away
        cb[:] += 20.0
        cb[1] = 0.4
    elif kind == "half_unused":                                # codes K/2.. never nearest
        cb[K // 2:] += 50.0
    return cb


def run_train(dev, x, coef, alpha, cb, beta, g_out, g_loss):
    xs = x.to(dev).requires_grad_(True)
    a = alpha.to(dev).requires_grad_(True)
    E = cb.to(dev).requires_grad_(True)
    poison(dev, x.numel(), g_out.numel())
    q, loss = ops.VQTrainFunction.apply(xs, coef.to(dev), a, E, beta)
    idx = q.grad_fn.indices
    torch.autograd.backward((q, loss), (g_out.to(dev), torch.tensor(g_loss, device=dev)))
    return [t.detach().cpu() for t in (idx, q, loss, xs.grad, a.grad, E.grad)]


TRAIN_CASES = [  # (B, side, D, K, T, codebook)
    (1, 7, 16, 1, 16, "random"),
    (84, 7, 16, 37, 16, "random"),          # N * D = 65 856: the element-wise loops take a second pass
    (100, 7, 16, 128, 16, "one_code"),
    (300, 8, 16, 512, 16, "half_unused"),
    (33, 5, 3, 7, 5, "random"),             # D = 3: 85 row lanes of 3, one thread idle in the g_E workgroups
    (40, 7, 48, 64, 16, "half_unused"),     # D = 48: 5 row lanes, 16 threads idle
    (20, 7, 64, 130, 16, "random"),
]


@pytest.mark.parametrize("B,side,D,K,T,kind", TRAIN_CASES)
def test_vq_train_function_vs_fp64(dev, B, side, D, K, T, kind):
    g = torch.Generator().manual_seed(B * 13 + D * 7 + K)
    x = (torch.rand(T, B, D, side, side, generator=g) < 0.3).float()
    coef, alpha, beta = coef_of(T), torch.tensor(ALPHA), 0.25
    cb = train_codebook(kind, K, D, K + D)
    g_out = torch.randn(B, D, side, side, generator=g)
    g_loss = 1.7
    # the code search on this read-out is in range before anything gathers from the codebook
    want = ref.vq_train_f64(x, coef, alpha, cb, beta, g_out, g_loss)
    assert_in_range(ops.vq_argmin(want["xm"].to(dev), cb.to(dev)), K)
    idx, q, loss, gx, ga, gE = run_train(dev, x, coef, alpha, cb, beta, g_out, g_loss)
    assert torch.equal(idx, want["idx"])
    if kind == "one_code":
        assert bool((idx == 1).all())
    used = torch.bincount(want["idx"], minlength=K) > 0
    if kind == "half_unused":
        assert not bool(used[K // 2:].any())
    N = B * side * side
    xm = want["xm"].double().view(B, side, side, D).permute(0, 3, 1, 2)
    assert bool(((q.double() - want["q"]).abs() <= 2 * EPS32 * (want["q"].abs() + xm.abs())).all())
    assert abs(float(loss) - float(want["loss"])) <= 4 * EPS32 * float(want["loss"])
    # g_x: a few fp32 roundings of the operands (g_out and the commitment term may cancel in g_x_m)
    w_t = ((1 - ALPHA) * coef.double() + ALPHA / T).view(T, 1, 1, 1, 1)
    err = (gx.double() - want["g_x"]).abs()
    tol = 8 * EPS32 * (want["g_x"].abs() + g_out.double().abs() * w_t)
    assert bool((err <= tol).all()), f"g_x: worst error / bound {float((err / tol).max())}"
    assert abs(float(ga) - float(want["g_alpha"])) <= 1e-6 * abs(float(want["g_alpha"]))
    # g_E per row, against that row's fp64 norm plus the fp32 rounding of its (e_k - x_m) terms; unused rows exactly 0
    c = abs(g_loss * 2.0 / (N * D))
    absdiff = torch.zeros(K, D, dtype=torch.float64).index_add_(0, want["idx"], (cb.double()[want["idx"]] - want["xm"].double()).abs())
    row_err = (gE.double() - want["g_E"]).norm(dim=1)
    row_tol = 1e-6 * want["g_E"].norm(dim=1) + 4 * EPS32 * c * absdiff.norm(dim=1)
    assert bool((row_err[used] <= row_tol[used]).all()), f"g_E rows {(row_err > row_tol).nonzero().flatten()[:8].tolist()}"
    assert bool((gE[~used] == 0).all()) and not bool(torch.signbit(gE[~used]).any())
    # deterministic: a second call gives the same bits
    again = run_train(dev, x, coef, alpha, cb, beta, g_out, g_loss)
    assert torch.equal(again[0], idx)
    for a_, b_ in zip(again[1:], (q, loss, gx, ga, gE)):
        assert same_bits(a_, b_)


def test_vq_train_function_nan_alpha(dev):
    """A NaN alpha: every row's code is 0 (the first NaN distance) and the loss is NaN -- the gathers stay in the codebook."""
    B, D, K, T = 100, 16, 128, 16
    x = (torch.rand(T, B, D, 7, 7, generator=torch.Generator().manual_seed(8)) < 0.3).float()
    cb = codebook(K, D, 8)
    assert_in_range(ops.vq_argmin(torch.full((B * 49, D), NAN, device=dev), cb.to(dev)), K)
    idx, q, loss, gx, ga, gE = run_train(dev, x, coef_of(T), torch.tensor(NAN), cb, 0.25, torch.randn(B, D, 7, 7), 1.0)
    assert_in_range(idx, K)
    assert int(idx.abs().max()) == 0
    assert bool(torch.isnan(loss))


# ------------------------------------------------------------------------------------------------ loss kernels
@pytest.mark.parametrize("tau", [2.0, 3.0])
@pytest.mark.parametrize("T", [1, 2, 15, 16])
def test_psp_loss_vs_fp64(dev, T, tau):
    """[T, 5, 16, 30, 30]: 72 000 elements per step, past one pass of 256 x 256 and over 128 block partials."""
    g = torch.Generator().manual_seed(T * 10 + int(tau))
    shape = (T, 5, 16, 30, 30)
    q0 = (torch.rand(*shape, generator=g) < 0.2).float()
    x0 = (torch.rand(*shape, generator=g) < 0.3).float()
    beta, g_loss = 0.25, 1.3
    q, x = q0.to(dev).requires_grad_(True), x0.to(dev).requires_grad_(True)
    poison(dev, q0.numel(), q0.numel())
    loss = ops.PSPLossFunction.apply(q, x, beta, tau)
    (loss * g_loss).backward()
    wl, wq, wx = ref.psp_loss_f64(q0, x0, beta, tau, g_loss)
    assert abs(float(loss) - float(wl)) <= 4e-6 * float(wl)
    c = g_loss * 2.0 / q0.numel()
    for got, want in ((q.grad.cpu(), wq), (x.grad.cpu(), wx)):
        err = (got.double() - want).abs()
        assert bool((err <= 1e-6 * want.abs() + 4 * T * EPS32 * c).all()), f"worst abs error {float(err.max())}"


@pytest.mark.parametrize("T,B", [(16, 100), (1, 100), (5, 3)])
def test_recon_loss_vs_fp64(dev, T, B):
    g = torch.Generator().manual_seed(T * 100 + B)
    y0 = torch.randn(T, B, 1, 28, 28, generator=g) * 0.4
    img = torch.rand(B, 1, 28, 28, generator=g) - 0.5
    coef, g_loss = coef_of(T), 2.5
    y = y0.to(dev).requires_grad_(True)
    poison(dev, y0.numel())
    loss = ops.ReconLossFunction.apply(y, coef.to(dev), img.to(dev))
    (loss * g_loss).backward()
    wl, wy = ref.recon_loss_f64(y0, coef, img, g_loss)
    assert abs(float(loss) - float(wl)) <= 1e-5 * float(wl)
    # per element: the fp32 read-out's rounding carried through tanh and the difference with the image
    c = g_loss * 2.0 / img.numel()
    s = (y0.double().abs() * coef.double().view(T, 1, 1, 1, 1)).sum(0)
    tol = 1e-6 * wy.abs() + 4 * EPS32 * c * coef.double().view(T, 1, 1, 1, 1) * ((T + 4) * s + 4)
    err = (y.grad.cpu().double() - wy).abs()
    assert bool((err <= tol).all()), f"worst abs error {float(err.max())}"


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("nchw", [True, False])
def test_embedding_past_the_grid(dev, nchw):
    """1400 x 7 x 7 tokens x D = 16: 1 097 600 elements, past 4096 x 256; tokens -1 and K give NaN rows exactly there."""
    K, D, B = 128, 16, 1400
    g = torch.Generator().manual_seed(1 + nchw)
    tok = torch.randint(0, K, (B, 7, 7), generator=g)
    tok.view(-1)[::97] = -1
    tok.view(-1)[5::101] = K
    cb = torch.randn(K, D, generator=g)
    poison(dev, B * 49 * D)
    out = ops.embedding(tok.to(dev), cb.to(dev), nchw_hw=(7, 7) if nchw else None).cpu()
    bad = (tok < 0) | (tok >= K)
    want = cb[tok.clamp(0, K - 1)]
    want[bad] = NAN
    if nchw:
        want = want.permute(0, 3, 1, 2)
    assert same_bits(out, want.contiguous())


# ------------------------------------------------------------------------------------------------ streams and the model
def test_vq_train_launches_on_two_streams(dev):
    """Quant, backward, PSP and reconstruction losses of two problems interleaved on two streams give the serial results
    (each stream has its own block partials and last-block ticket)."""
    def problem(seed):
        g = torch.Generator().manual_seed(seed)
        T, B, D = 16, 100, 16
        return dict(x=(torch.rand(T, B, D, 7, 7, generator=g) < 0.3).float().to(dev), cb=codebook(128, D, seed).to(dev),
                    go=torch.randn(B, D, 7, 7, generator=g).to(dev), q=(torch.rand(T, B, D, 7, 7, generator=g) < 0.2).float().to(dev),
                    y=(torch.randn(T, B, 1, 28, 28, generator=g) * 0.4).to(dev), img=(torch.rand(B, 1, 28, 28, generator=g) - 0.5).to(dev))

    coef = coef_of(16).to(dev)

    def run(p):
        xs, E = p["x"].clone().requires_grad_(True), p["cb"].clone().requires_grad_(True)
        a = torch.tensor(ALPHA, device=dev, requires_grad=True)
        q, l1 = ops.VQTrainFunction.apply(xs, coef, a, E, 0.25)
        qs, ys = p["q"].clone().requires_grad_(True), p["y"].clone().requires_grad_(True)
        l2 = ops.PSPLossFunction.apply(qs, xs, 0.25, 2.0)
        l3 = ops.ReconLossFunction.apply(ys, coef, p["img"])
        ((q * p["go"]).sum() + l1 + l2 + l3).backward()
        return [t.detach() for t in (q, l1, l2, l3, xs.grad, a.grad, E.grad, qs.grad, ys.grad)]

    probs = [problem(1), problem(2)]
    serial = [[t.cpu() for t in run(p)] for p in probs]
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream(dev))
    outs = [[], []]
    for _ in range(4):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                outs[i].append(run(probs[i]))
    torch.cuda.synchronize()
    for i in (0, 1):
        for res in outs[i]:
            for got, want in zip(res, serial[i]):
                assert same_bits(got.cpu(), want)


def test_snn_vqvae_model_train_step_fused_and_op_by_op(dev):
    """One SNN_VQVAE training step at B = 100 (4 900 latent positions): the fused VQ / PSP / reconstruction operators and the
    reference's algebra op by op through autograd give the same code indices, losses and codebook / alpha gradients."""
    from snn_model.vae_model import SNN_VQVAE, functional
    from spkdiff import synth
    img = (synth.stroke_images(100, 21) - 0.5).to(dev)
    res = {}
    for fused in (True, False):
        m = SNN_VQVAE(1, 16, 128, 0.08).to(dev)
        functional.set_step_mode(net=m, step_mode='m')
        m.load_state_dict(synth.synth_vqvae_state(synth.MNIST))
        m.train()
        m.vq_layer.fused_train = fused
        seen = []
        inner = m.vq_layer._train_forward_idx

        def spy(x, inner=inner, seen=seen):
            r = inner(x)
            seen.append(r[2].detach().clone())
            return r

        m.vq_layer._train_forward_idx = spy
        a, b, c = m(img.unsqueeze(0).repeat(16, 1, 1, 1, 1), img)
        (a + b).backward()
        functional.reset_net(m)
        res[fused] = (seen[0].cpu(), float(a.detach()), float(b.detach()), m.vq_layer.embeddings.weight.grad.cpu(),
                      float(m.vq_layer.alpha.grad))
    (i1, a1, b1, e1, al1), (i0, a0, b0, e0, al0) = res[True], res[False]
    assert i1.numel() == 4900 and torch.equal(i1, i0)
    assert abs(a1 - a0) <= 4e-6 * abs(a0) and abs(b1 - b0) <= 3e-6 * abs(b0)
    assert float((e1 - e0).norm() / (e0.norm() + 1e-30)) <= 2e-6
    assert abs(al1 - al0) <= 2e-5 * (abs(al0) + 1e-3)
