"""GPU tests of the sample-quality arithmetic (run with ``-m gpu`` on an MI355X): ``spk_feature_moments_acc`` and
``spk_poly_kernel_sums`` against the exact host oracle of tests/_feature_stats_oracle.py (bit for bit on the dyadic cases, inside
the counted bounds on the real-valued ones), the chain contract, NaN containment, workspaces full of garbage, graph capture,
``FeatureStats`` / ``kernel_distance`` on the device against their CPU paths, ``encode_features`` and ``sample_quality_eval``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _feature_stats_oracle as orc          # noqa: E402
from spkdiff import synth                   # noqa: E402
from test_gpu_completion import build_den, build_vae, sampler      # noqa: E402  (the helpers, not the tests)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def _state(d, dev):
    return torch.zeros(d, dtype=torch.float64, device=dev), torch.zeros((d, d), dtype=torch.float64, device=dev)


def _moments(ops, dev, x, state=None):
    s, g = _state(x.shape[1], dev) if state is None else state
    ops.feature_moments(torch.from_numpy(np.ascontiguousarray(x)).to(dev), s, g)
    return s, g


# ------------------------------------------------------------------------------------------------- 1. moments
@pytest.mark.parametrize("n,d", orc.MOMENT_DYADIC)
def test_moments_exact(dev, ops, n, d):
    f = orc.dyadic_features(n, d, seed=100 + n + d)
    ssum, gram, _, _ = orc.moments_oracle(f)
    s, g = _moments(ops, dev, f.x)
    assert np.array_equal(s.cpu().numpy(), ssum), "sum"
    assert np.array_equal(g.cpu().numpy(), gram), "gram"
    assert torch.equal(g, g.T), "gram is bit-symmetric"
    # a strided view: the rows of a wider matrix (row stride > d), garbage beside them
    wide = torch.full((n, d + 24), 7.5, device=dev)
    wide[:, 3:3 + d] = torch.from_numpy(f.x).to(dev)
    s2, g2 = _state(d, dev)
    view = wide[:, 3:3 + d]
    assert view.stride(0) == d + 24 and (n == 1 or not view.is_contiguous())
    ops.feature_moments(view, s2, g2)
    assert torch.equal(s2, s) and torch.equal(g2, g)


@pytest.mark.parametrize("n,d", orc.MOMENT_REAL)
def test_moments_ragged_and_real_valued(dev, ops, n, d):
    f = orc.real_features(n, d, seed=200 + n + d)
    ssum, gram, abs_sum, abs_gram = orc.moments_oracle(f)
    s, g = _moments(ops, dev, f.x)
    es, eg = np.abs(s.cpu().numpy() - ssum), np.abs(g.cpu().numpy() - gram)
    bs, bg = orc.sum_bound(n, abs_sum), orc.gram_bound(n, abs_gram)
    print(f"MOMENTS n={n} d={d}: max gram err / bound {float((eg / bg).max()):.3f}, sum {float((es / bs).max()):.3f}, "
          f"inexact entries {float((eg > 0).mean()):.2f}")
    assert np.all(es <= bs) and np.all(eg <= bg)
    assert torch.equal(g, g.T)
    # padding rows and columns contribute nothing: the same features inside a larger, NaN-filled buffer give the same bits
    pad = torch.full((n + 7, d + 9), float("nan"), device=dev)
    pad[:n, :d] = torch.from_numpy(f.x).to(dev)
    s2, g2 = _state(d, dev)
    ops.feature_moments(pad[:n, :d], s2, g2)
    assert torch.equal(s2, s) and torch.equal(g2, g)


def test_moments_chain_contract(dev, ops):
    n, d = 150, 100
    f = orc.real_features(n, d, seed=31)
    _, _, _, abs_gram = orc.moments_oracle(f)
    whole = _moments(ops, dev, f.x)
    again = _moments(ops, dev, f.x)
    assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1]), "two identical calls"
    st = _moments(ops, dev, f.x[:64])                                   # 64 % 4 == 0: the chain continues where it stopped
    _moments(ops, dev, f.x[64:], st)
    assert torch.equal(st[0], whole[0]) and torch.equal(st[1], whole[1])
    st = _moments(ops, dev, f.x[:61])                                   # 61 % 4 != 0: other groups of four, inside the bound
    _moments(ops, dev, f.x[61:], st)
    assert torch.equal(st[0], whole[0]), "the sum is one sequential chain whatever the split"
    diff = (st[1] - whole[1]).abs().cpu().numpy()
    print(f"CHAIN split at 61: {int((diff > 0).sum())} of {diff.size} entries differ, max diff / bound "
          f"{float((diff / orc.chain_split_bound(61, n - 61, abs_gram)).max()):.3f}")
    assert np.all(diff <= orc.chain_split_bound(61, n - 61, abs_gram))
    keep = (st[0].clone(), st[1].clone())
    ops.feature_moments(torch.empty((0, d), device=dev), *st)            # n = 0: a no-op
    assert torch.equal(st[0], keep[0]) and torch.equal(st[1], keep[1])


def test_moments_nan_reaches_its_row_and_column_only(dev, ops):
    n, d, r, c = 37, 40, 21, 17
    x = orc.real_features(n, d, seed=32).x.copy()
    clean = _moments(ops, dev, x)
    x[r, c] = np.nan
    s, g = _moments(ops, dev, x)
    want = torch.zeros(d, dtype=torch.bool, device=dev)
    want[c] = True
    assert torch.equal(torch.isnan(s), want)
    assert torch.equal(torch.isnan(g), want[:, None] | want[None, :])
    ok = ~torch.isnan(g)
    assert torch.equal(g[ok], clean[1][ok]) and torch.equal(s[~want], clean[0][~want])


# ------------------------------------------------------------------------------------------------- 2. kernel sums
def _garbage_ws(ops, S, p, q, dev):
    ws = ops.poly_kernel_sums_ws(S, p, q, dev)
    ws.fill_(0x7FF8DEADBEEF0000)                                         # NaN bit patterns: a partial read before it is written shows
    return ws


@pytest.mark.parametrize("p,q", orc.KSUM_DYADIC_PQ)
@pytest.mark.parametrize("d", orc.KSUM_DYADIC_D)
def test_kernel_sums_exact(dev, ops, d, p, q):
    n_x, n_y, S = p + 5, q + 3, 5
    fx, fy = orc.dyadic_features(n_x, d, seed=300 + d + p), orc.dyadic_features(n_y, d, seed=400 + d + q)
    X, Y = torch.from_numpy(fx.x).to(dev), torch.from_numpy(fy.x).to(dev)
    ix, iy = orc.subset_tables(n_x, n_y, S, p, q, seed=d + p + q)         # rows repeat and come in any order
    ix[0, :] = ix[0, 0]                                                  # (one subset names a single row p times)
    gamma, coef = 1.0 / d, 1.0
    for degree in (1, 2, 3):
        # S = 1 without tables: rows 0 .. p - 1 against rows 0 .. q - 1
        got = ops.poly_kernel_sums(X, Y, p=p, q=q, degree=degree, ws=_garbage_ws(ops, 1, p, q, dev)).cpu().numpy()
        want = orc.dyadic_kernel_sums(fx.rows(range(p)), fy.rows(range(q)), gamma, coef, degree, False)
        assert got.shape == (1, 2) and (got[0, 0], got[0, 1]) == (want[0], 0.0), (degree, "no tables")
        got = ops.poly_kernel_sums(X, X, p=p, q=p, degree=degree, symmetric=True, ws=_garbage_ws(ops, 1, p, p, dev)).cpu().numpy()
        want = orc.dyadic_kernel_sums(fx.rows(range(p)), fx.rows(range(p)), gamma, coef, degree, True)
        assert (got[0, 0], got[0, 1]) == want, (degree, "no tables, symmetric")
        # S = 5 with tables
        got = ops.poly_kernel_sums(X, Y, torch.from_numpy(ix).to(dev), torch.from_numpy(iy).to(dev), degree=degree,
                                   ws=_garbage_ws(ops, S, p, q, dev)).cpu().numpy()
        for s in range(S):
            want = orc.dyadic_kernel_sums(fx.rows(ix[s]), fy.rows(iy[s]), gamma, coef, degree, False)
            assert (got[s, 0], got[s, 1]) == (want[0], 0.0), (degree, s)
        t = torch.from_numpy(ix)                                         # a host table: checked and uploaded by the wrapper
        got = ops.poly_kernel_sums(X, X, t, t, degree=degree, symmetric=True, ws=_garbage_ws(ops, S, p, p, dev)).cpu().numpy()
        for s in range(S):
            want = orc.dyadic_kernel_sums(fx.rows(ix[s]), fx.rows(ix[s]), gamma, coef, degree, True)
            assert (got[s, 0], got[s, 1]) == want, (degree, s, "symmetric")


@pytest.mark.parametrize("d,p,q", orc.KSUM_REAL)
def test_kernel_sums_real_valued(dev, ops, d, p, q):
    n_x, n_y, S = p + 9, q + 4, 3
    fx, fy = orc.real_features(n_x, d, seed=500 + d), orc.real_features(n_y, d, seed=501 + d)
    fy = orc.Feat(fy.g, fy.r, fx.s)                                      # (one column grid for both sets)
    X, Y = torch.from_numpy(fx.x).to(dev), torch.from_numpy(fy.x).to(dev)
    ix, iy = orc.subset_tables(n_x, n_y, S, p, q, seed=d)
    ix[ix == 2] = 3                                                      # row 2 of X is kept for the NaN below
    ix[1, 5] = 2
    dix, diy = torch.from_numpy(ix).to(dev), torch.from_numpy(iy).to(dev)
    gamma = 1.0 / d
    got = ops.poly_kernel_sums(X, Y, dix, diy, gamma=gamma, degree=3, ws=_garbage_ws(ops, S, p, q, dev)).cpu().numpy()
    sym = ops.poly_kernel_sums(X, X, dix, dix, gamma=gamma, degree=3, symmetric=True, ws=_garbage_ws(ops, S, p, p, dev)).cpu().numpy()
    for s in range(S):
        tot, _, b_tot, _ = orc.kernel_sums_oracle(fx.rows(ix[s]), fy.rows(iy[s]), gamma, 1.0, 3, False)
        stot, sdia, sb_tot, sb_dia = orc.kernel_sums_oracle(fx.rows(ix[s]), fx.rows(ix[s]), gamma, 1.0, 3, True)
        print(f"KSUM d={d} s={s}: err/bound total {abs(got[s, 0] - tot) / b_tot:.3f} sym {abs(sym[s, 0] - stot) / sb_tot:.3f} "
              f"diag {abs(sym[s, 1] - sdia) / sb_dia:.3f}")
        assert abs(got[s, 0] - tot) <= b_tot and got[s, 1] == 0.0
        assert abs(sym[s, 0] - stot) <= sb_tot and abs(sym[s, 1] - sdia) <= sb_dia
    # a NaN in a row: the subsets that name the row are NaN, the others keep their bits
    Xn = X.clone()
    Xn[2, d // 2] = float("nan")
    gn = ops.poly_kernel_sums(Xn, Y, dix, diy, gamma=gamma, degree=3, ws=_garbage_ws(ops, S, p, q, dev)).cpu().numpy()
    assert np.isnan(gn[1, 0]) and np.array_equal(gn[[0, 2]], got[[0, 2]])
    # a device table with an entry outside the matrix: no row is read, that subset is NaN
    bad = dix.clone()
    bad[2, 0] = n_x
    gb = ops.poly_kernel_sums(X, Y, bad, diy, gamma=gamma, degree=3).cpu().numpy()
    assert np.isnan(gb[2, 0]) and np.array_equal(gb[:2], got[:2])
    with pytest.raises(ValueError, match="outside"):                     # the same table on the host is refused
        ops.poly_kernel_sums(X, Y, bad.cpu(), diy, gamma=gamma, degree=3)


def test_capture_and_replay(dev, ops):
    n, d, p = 130, 100, 37
    f = orc.real_features(n, d, seed=61)
    X = torch.from_numpy(f.x).to(dev)
    ix = torch.from_numpy(orc.subset_tables(n, n, 3, p, p, seed=8)[0]).to(dev)
    eager_s, eager_g = _state(d, dev)
    ops.feature_moments(X, eager_s, eager_g)
    eager_k = ops.poly_kernel_sums(X, X, ix, ix, symmetric=True)
    s, g = _state(d, dev)
    ws, out = _garbage_ws(ops, 3, p, p, dev), torch.empty((3, 2), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            ops.feature_moments(X, s, g)
            ops.poly_kernel_sums(X, X, ix, ix, symmetric=True, ws=ws, out=out)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(2):                                                   # the state is an input too: reset it, replay
        s.zero_()
        g.zero_()
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s, eager_s) and torch.equal(g, eager_g) and torch.equal(out, eager_k)


# ------------------------------------------------------------------------------------------------- 3. the public interface
def test_device_distances_agree_with_the_cpu_paths(dev):
    from spkdiff.evaluate import FeatureStats, frechet_distance, kernel_distance, kernel_subsets
    n, d, S, m = 300, 784, 4, 128
    fx, fy = orc.real_features(n, d, seed=71), orc.real_features(n, d, seed=72)
    x, y = torch.from_numpy(fx.x), torch.from_numpy(fy.x) * 1.25 + 0.125
    cpu_a, cpu_b = FeatureStats(d).update(x), FeatureStats(d).update(y)
    dev_a, dev_b = FeatureStats(d, dev).update(x.to(dev)), FeatureStats(d, dev).update(y.to(dev))
    assert dev_a.n == n and dev_a.gram.is_cuda
    for c, g, t in ((cpu_a, dev_a, x), (cpu_b, dev_b, y)):
        ab = t.double().abs()
        abs_gram = (ab.T @ ab).numpy() * (1 + 1e-12)
        # device: the counted chain; CPU (any order): n roundings
        bound = orc.gram_bound(n, abs_gram) + n * orc.U * abs_gram
        assert np.all((c.gram - g.gram.cpu()).abs().numpy() <= bound)
        assert np.all((c.sum - g.sum.cpu()).abs().numpy() <= 2 * orc.sum_bound(n, ab.sum(0).numpy()))
    fd_c, fd_d = frechet_distance(cpu_a, cpu_b), frechet_distance(dev_a, dev_b)
    # n <= d: sqrt(C1) C2 sqrt(C1) has d - n + 1 zero eigenvalues, where a perturbation delta of the matrix (3 d^2 eps |C|^2, see
    # the self-distance test below) becomes sqrt(delta) = d sqrt(3 eps) |C| in the root: d of them, doubled, on either path
    tr = max(float(torch.trace(cpu_a.cov())), float(torch.trace(cpu_b.cov())))
    fd_bound = 4 * d * (d * np.sqrt(3 * orc.EPS)) * tr
    print(f"FD device {fd_d:.12e} cpu {fd_c:.12e} |diff| {abs(fd_d - fd_c):.2e} bound {fd_bound:.2e}")
    assert fd_c > 0 and abs(fd_c - fd_d) <= fd_bound
    mean_c, std_c = kernel_distance(x, y, subsets=S, subset_size=m, seed=5)
    mean_d, std_d = kernel_distance(x.to(dev), y.to(dev), subsets=S, subset_size=m, seed=5)
    ix, iy = kernel_subsets(n, n, S, m, seed=5)
    gamma, bound = 1.0 / d, 0.0
    for s in range(S):                                                   # both paths' term bounds through the formula
        xs, ys = x[ix[s].long()].numpy(), y[iy[s].long()].numpy()
        b = 0.0
        for a_, b_, div in ((xs, xs, m * (m - 1)), (ys, ys, m * (m - 1)), (xs, ys, m * m / 2)):
            dk = orc.kernel_term_bounds(a_, b_, gamma, 1.0, 3, orc.DOT_ROUNDINGS(d), orc.SUM_DEPTH(m, m)) + \
                orc.kernel_term_bounds(a_, b_, gamma, 1.0, 3, d, m * m)
            kk = np.abs(gamma * (a_.astype(np.float64) @ b_.astype(np.float64).T) + 1.0) ** 3
            b += (dk.sum() + 8 * orc.U * kk.sum()) / div
        bound = max(bound, b)
    print(f"KD device {mean_d:.12e} cpu {mean_c:.12e} |diff| {abs(mean_d - mean_c):.2e} bound {bound:.2e}")
    assert abs(mean_d - mean_c) <= bound and abs(std_d - std_c) <= 2 * bound * np.sqrt(S)
    assert bound < 1e-4 * abs(mean_c), "the bound is loose enough to pass anything"
    assert (mean_d, std_d) == kernel_distance(x.to(dev), y.to(dev), subsets=S, subset_size=m, seed=5)


def test_encode_features_is_the_read_out_the_quantiser_searches_on(dev):
    from snn_model.vae_model import IN_TINV
    model, _ = build_vae(synth.MNIST, dev)
    img = (torch.rand(3, 1, 28, 28, generator=torch.Generator().manual_seed(9)) - 0.5).to(dev)
    idx0 = model.encode_images(img, 16)
    feats = model.encode_features(img, 16)
    z_ptc = model.encoder.snn_convs.run(img, IN_TINV, final='ptc', T=16, stateful=False)['ptc']
    idx, _, xm = model.vq_layer._quantize_ptc(z_ptc, want_xm=True, want_zq=False)
    D = model.vq_layer.embedding_dim
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (3, 49 * D)
    assert torch.equal(feats, xm.reshape(3, -1)) and torch.equal(idx.reshape(3, 7, 7), idx0)
    assert torch.equal(model.encode_images(img, 16), idx0), "the indices of encode_images are unchanged by the new method"
    assert float(feats.std()) > 0


def _quality(dev, features, batch, kid, real=None, seed=77):
    from spkdiff.evaluate import sample_quality_eval
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    ab = sampler(den, True, True, True)
    if real is None:
        real = synth.stroke_images(64, seed=123)
    torch.manual_seed(seed)
    res = sample_quality_eval(model, ab, [real[i:i + batch] for i in range(0, 64, batch)], 64, features=features, batch=batch,
                              kid=kid, sample_steps=5)
    return res, model, ab


@pytest.mark.parametrize("features", ["pixels", "encoder"])
def test_sample_quality_eval_on_the_synthetic_checkpoint(dev, features):
    kid = dict(subsets=2, subset_size=32)
    r64, model, ab = _quality(dev, features, 64, kid)
    assert set(r64) == {"fd", "fd_reference_convention", "kd_mean", "kd_std", "n_real", "n_generated", "d"}
    assert (r64["n_real"], r64["n_generated"], r64["d"]) == (64, 64, 784 if features == "pixels" else 49 * model.vq_layer.embedding_dim)
    assert all(np.isfinite(r64[k]) for k in ("fd", "fd_reference_convention", "kd_mean", "kd_std")) and r64["fd"] > 0
    assert ab.n_samples == 3, "the sampler's own job size is restored"
    # batch 16: the images do not depend on it (one job, one key) and 16 % 4 == 0, so the chains continue bit for bit
    r16, _, _ = _quality(dev, features, 16, kid)
    assert r16 == r64
    assert _quality(dev, features, 64, None)[0]["kd_mean"] is None


def test_sample_quality_eval_of_a_set_against_itself(dev, ops):
    """The generated images, fed back as the real set: the two FeatureStats are equal, so the Frechet distance is what the two
    eigenproblems leave -- M = sqrt(C) C sqrt(C) has entry errors of about 3 d eps |C|^2, its eigenvalues move by d times that, and
    a zero eigenvalue (n <= d: most of them) turns a perturbation delta into sqrt(delta): at most 2 d (d sqrt(3 eps)) tr C.  The
    unbiased kernel estimate of a set against itself is not 0 but 2 (T - n D) / (n^2 (n - 1)) <= 0 (T: the sum of the Gram matrix,
    D: its trace): exactly that, from the same kernel."""
    from spkdiff.evaluate import sample_quality_eval
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    ab = sampler(den, True, True, True)
    ab.set_shard(0, 64)
    torch.manual_seed(78)
    tok = ab.sample(1.0, 5).reshape(64, 7, 7)
    real = model.decode_tokens(tok, 16, want_u8=True)[1].float() / 255
    seen = []

    def pixels(im):
        seen.append(im.reshape(im.shape[0], -1).contiguous())
        return seen[-1]
    res = sample_quality_eval(model, ab, [real], 64, draw=lambda s, b: tok, features=pixels, batch=64, kid=dict(subsets=None))
    assert len(seen) == 2 and torch.equal(seen[0], seen[1]), "the real side returns to the uint8 grid it came from"
    F = seen[0]
    n, d = F.shape
    tr = float(torch.trace(torch.cov(F.double().T)))
    bound = 2 * d * (d * np.sqrt(3 * orc.EPS)) * tr
    print(f"SELF fd {res['fd']:.3e} (bound {bound:.3e}, tr C {tr:.3f}) kd {res['kd_mean']:.6e}")
    assert abs(res["fd"]) <= bound
    T, D = ops.poly_kernel_sums(F, F, symmetric=True)[0].tolist()
    assert res["kd_mean"] == ((T - D) + (T - D)) / (n * (n - 1)) - 2 * T / (n * n) and res["kd_std"] == 0.0
    assert res["kd_mean"] <= 0 and res["kd_mean"] == pytest.approx(2 * (T - n * D) / (n * n * (n - 1)), rel=1e-9)
