"""CPU tests of the sample-quality arithmetic: the oracle against its own definition, ``FeatureStats`` on CPU
tensors, both conventions of ``frechet_distance`` against fixture F21 (tests/golden/f21_sample_quality.npz, written with the real
reference by tools/gen_golden_sample_quality.py), ``kernel_distance`` on its torch restatement, the argument errors and the
header's constants.  tests/_feature_stats_oracle.py has the bounds and their derivation."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _feature_stats_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F21 = os.path.join(ROOT, "tests", "golden", "f21_sample_quality.npz")


@pytest.fixture(scope="module")
def f21():
    return np.load(F21)


def test_oracle_integer_route_is_fsum_of_the_products():
    """The exact-integer sums equal math.fsum over the fp64 products term by term, and the exponent spread makes plain fp64
    accumulation round (else the 'real-valued' cases would test nothing)."""
    f = orc.real_features(37, 24, seed=5)
    ssum, gram, abs_sum, abs_gram = orc.moments_oracle(f)
    fs, fg = orc.gram_fsum(f.x)
    assert np.array_equal(ssum, fs) and np.array_equal(gram, fg) and np.array_equal(gram, gram.T)
    x = f.x.astype(np.float64)
    naive = np.zeros_like(gram)
    for k in range(x.shape[0]):
        naive += np.outer(x[k], x[k])
    assert (naive != gram).mean() > 0.2, "sequential fp64 accumulation is exact on these features: the bound is not exercised"
    assert np.all(np.abs(naive - gram) <= x.shape[0] * orc.U * abs_gram)
    dots, _ = orc.exact_dots(f.rows([0, 3]), f.rows([1, 3, 5]))
    assert float(dots[1, 2]) == pytest.approx(float(x[3] @ x[5]), rel=1e-13) and dots.shape == (2, 3)


def test_oracle_dyadic_budget_and_sums():
    f = orc.dyadic_features(33, 16, seed=2)
    assert set(np.unique(f.x * 4)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    tot, dia = orc.dyadic_kernel_sums(f, f, 1 / 16, 1.0, 3, True)
    x = f.x.astype(np.float64)
    k = (x @ x.T / 16 + 1) ** 3
    assert tot == k.sum() and dia == np.trace(k)                       # exact in any order, numpy's included
    t2, d2, b_t, b_d = orc.kernel_sums_oracle(f, f, 1 / 16, 1.0, 3, True)
    assert (t2, d2) == (tot, dia) and b_t > 0
    with pytest.raises(AssertionError):
        orc.dyadic_budget(1024, 4096, 4096, 8, 1 / 1024, 1.0)          # 8 (12 + log2 1.25) + 24 bits: not exact
    with pytest.raises(AssertionError):
        orc.dyadic_features(4, 24, seed=0)


def _stats(x, device="cpu", split=None):
    from spkdiff.evaluate import FeatureStats
    st = FeatureStats(x.shape[1], device)
    for part in ([x] if split is None else [x[:split], x[split:]]):
        st.update(torch.from_numpy(part).to(device))
    return st


@pytest.mark.parametrize("n,d", [(2, 16), (64, 16), (256, 64)])
def test_feature_stats_cpu_cov_is_np_cov_bit_for_bit(n, d):
    """Dyadic features and n a power of two: the mean, the centred values, their products and sums are exact, so np.cov's two-pass
    value and the one-pass (gram - sum sum^T / n) / (n - 1) must agree to the bit."""
    f = orc.dyadic_features(n, d, seed=n + d)
    st = _stats(f.x)
    ssum, gram, _, _ = orc.moments_oracle(f)
    assert st.n == n and np.array_equal(st.sum.numpy(), ssum) and np.array_equal(st.gram.numpy(), gram)
    assert np.array_equal(st.mean().numpy(), f.x.astype(np.float64).mean(axis=0))
    assert np.array_equal(st.cov().numpy(), np.cov(f.x.astype(np.float64), rowvar=False))
    assert st.cov().dtype == torch.float64


def test_feature_stats_merge_and_errors():
    from spkdiff.evaluate import FeatureStats
    f = orc.dyadic_features(96, 32, seed=9)
    one, a, b = _stats(f.x), _stats(f.x[:40]), _stats(f.x[40:])
    a.merge(b)
    assert a.n == one.n and torch.equal(a.sum, one.sum) and torch.equal(a.gram, one.gram) and torch.equal(a.cov(), one.cov())
    assert torch.equal(_stats(f.x, split=41).gram, one.gram)
    r = orc.real_features(50, 12, seed=3)
    assert np.allclose(_stats(r.x).cov().numpy(), np.cov(r.x.astype(np.float64), rowvar=False), rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError):
        FeatureStats(4).update(torch.zeros(3, 5))
    with pytest.raises(ValueError):
        FeatureStats(4).update(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        FeatureStats(4).update(torch.zeros(1, 4)).cov()
    with pytest.raises(ValueError):
        FeatureStats(4097)
    with pytest.raises(ValueError):
        a.merge(FeatureStats(16))
    assert FeatureStats(4).update(torch.zeros(0, 4)).n == 0


def _same_d_ref_err(f21, d):
    return max(float(f21[f"{n}/ref_err"]) for n in f21["commuting_names"] if f21[f"{n}/mu1"].shape[0] == d)


def test_frechet_exact_against_the_closed_form(f21):
    from spkdiff.evaluate import frechet_distance
    L_MIN, L_MAX = orc.F21_L_MIN, orc.F21_L_MAX
    for name in f21["commuting_names"]:
        g = {k: f21[f"{name}/{k}"] for k in ("mu1", "mu2", "sigma1", "sigma2", "l1", "l2", "closed")}
        d = g["mu1"].shape[0]
        assert L_MIN <= min(g["l1"].min(), g["l2"].min()) and max(g["l1"].max(), g["l2"].max()) <= L_MAX
        got = frechet_distance((g["mu1"], g["sigma1"]), (g["mu2"], g["sigma2"]))
        bound = orc.frechet_exact_bound(d, L_MIN, L_MAX, g["l1"].sum() + g["l2"].sum())
        print(f"F21 {name}: exact {got:.15g} closed {float(g['closed']):.15g} |diff| {abs(got - float(g['closed'])):.2e} bound {bound:.2e}")
        assert abs(got - float(g["closed"])) <= bound
        assert bound < 1e-7 * float(g["closed"])                       # (the bound is tight enough to mean something)


def test_frechet_reference_convention_against_the_reference(f21):
    from metric.Fid_score import calculate_frechet_distance
    from spkdiff.evaluate import FeatureStats, frechet_distance
    for name in f21["commuting_names"]:
        g = {k: f21[f"{name}/{k}"] for k in ("mu1", "mu2", "sigma1", "sigma2", "ref_fd")}
        d = g["mu1"].shape[0]
        tol = orc.frechet_reference_tol(d, np.trace(g["sigma1"]) + np.trace(g["sigma2"]), _same_d_ref_err(f21, d))
        got = frechet_distance((g["mu1"], g["sigma1"]), (g["mu2"], g["sigma2"]), "reference")
        got2 = calculate_frechet_distance(g["mu1"], g["sigma1"], g["mu2"], g["sigma2"])
        print(f"F21 {name}: reference convention {got:.15g} recorded {float(g['ref_fd']):.15g} tol {tol:.2e}")
        assert abs(got - float(g["ref_fd"])) <= tol and got2 == got
    for name in f21["feature_names"]:
        x, y, ref = f21[f"{name}/x"], f21[f"{name}/y"], float(f21[f"{name}/ref_fd"])
        d = x.shape[1]
        a, b = _stats(x), _stats(y)
        tol = orc.frechet_reference_tol(d, float(torch.trace(a.cov()) + torch.trace(b.cov())), _same_d_ref_err(f21, d))
        got = frechet_distance(a, b, "reference")
        got2 = calculate_frechet_distance(a.mean().numpy(), a.cov().numpy(), b.mean().numpy(), b.cov().numpy(), eps=1e-6)
        print(f"F21 {name}: reference convention {got:.15g} recorded {ref:.15g} tol {tol:.2e}")
        assert abs(got - ref) <= tol and got2 == got
        # through a FeatureStats on torch tensors given as (mu, sigma), too
        assert frechet_distance((a.mean(), a.cov()), (b.mean(), b.cov()), "reference") == got


def test_the_two_conventions_differ_where_the_covariances_do_not_commute(f21):
    """R/metric/Fid_score.py:15-18 takes U sqrt(S) V of the non-symmetric C1 C2 for its square root: on correlated features the
    value is off by more than 10 %; on commuting covariances the two agree."""
    from spkdiff.evaluate import frechet_distance
    name = "corr_n400_d40"
    a, b = _stats(f21[f"{name}/x"]), _stats(f21[f"{name}/y"])
    exact, ref = frechet_distance(a, b), frechet_distance(a, b, "reference")
    print(f"F21 {name}: exact {exact:.6f} reference convention {ref:.6f}")
    assert abs(ref - exact) > 0.1 * exact and 0 < exact < ref
    s1, s2 = a.cov().numpy(), b.cov().numpy()
    assert np.abs(s1 @ s2 - s2 @ s1).max() > 1e-3
    # the exact value by another route: the eigenvalues of C1 C2 (real and non-negative for SPD factors)
    lam = np.linalg.eigvals(s1 @ s2)
    other = float(((a.mean() - b.mean()) ** 2).sum()) + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.clip(lam.real, 0, None)).sum()
    assert abs(other - exact) < 1e-9 * exact
    g = {k: f21[f"rot_d40/{k}"] for k in ("mu1", "mu2", "sigma1", "sigma2")}
    e2 = frechet_distance((g["mu1"], g["sigma1"]), (g["mu2"], g["sigma2"]))
    r2 = frechet_distance((g["mu1"], g["sigma1"]), (g["mu2"], g["sigma2"]), "reference")
    assert abs(e2 - r2) < 1e-10 * e2


def test_frechet_argument_errors():
    from spkdiff.evaluate import FeatureStats, frechet_distance
    mu, s = np.zeros(3), np.eye(3)
    assert frechet_distance((mu, s), (mu, s)) == pytest.approx(0.0, abs=1e-12)
    bad = s.copy()
    bad[0, 1] = np.nan
    for a in ((mu, bad), (np.array([0, np.inf, 0]), s)):
        with pytest.raises(ValueError, match="non-finite"):
            frechet_distance(a, (mu, s))
    with pytest.raises(ValueError, match="n >= 2"):
        frechet_distance(FeatureStats(3).update(torch.zeros(1, 3)), (mu, s))
    with pytest.raises(ValueError):
        frechet_distance((mu, s), (np.zeros(4), np.eye(4)))
    with pytest.raises(ValueError, match="convention"):
        frechet_distance((mu, s), (mu, s), "scipy")
    assert "rank" in frechet_distance.__doc__ and "n <= d" in frechet_distance.__doc__


def test_kernel_distance_cpu():
    from spkdiff.evaluate import kernel_distance, kernel_subsets, mmd2_from_sums
    # every row the same: k is constant, sum k = m tr k, and the unbiased estimate of a set against itself is exactly 0
    row = orc.dyadic_features(1, 16, seed=4).x
    same = torch.from_numpy(np.repeat(row, 24, axis=0))
    assert kernel_distance(same, same, subsets=3, subset_size=8) == (0.0, 0.0)
    assert kernel_distance(same, same, subsets=None) == (0.0, 0.0)
    # a dyadic set against itself, full set: exactly the closed form 2 (T - n D) / (n^2 (n - 1)) <= 0 of the exact sums
    f = orc.dyadic_features(32, 16, seed=6)
    x = torch.from_numpy(f.x)
    T, D = orc.dyadic_kernel_sums(f, f, 1 / 16, 1.0, 3, True)
    mean, std = kernel_distance(x, x, subsets=None)
    assert std == 0.0 and mean == ((T - D) + (T - D)) / (32 * 31) - 2 * T / (32 * 32) and mean <= 0
    assert mean == pytest.approx(2 * (T - 32 * D) / (32 * 32 * 31), rel=1e-12)
    # subsets: a function of the seed alone; mean and unbiased std over the per-subset values
    g = orc.dyadic_features(40, 16, seed=7)
    y = torch.from_numpy(g.x)
    ix, iy = kernel_subsets(32, 40, 5, 12, seed=3)
    ix2, iy2 = kernel_subsets(32, 40, 5, 12, seed=3)
    assert torch.equal(ix, ix2) and torch.equal(iy, iy2) and ix.dtype == torch.int32 and tuple(iy.shape) == (5, 12)
    assert not torch.equal(ix, kernel_subsets(32, 40, 5, 12, seed=4)[0])
    assert all(len(set(r.tolist())) == 12 for r in ix) and int(ix.max()) < 32 and int(iy.max()) < 40
    vals = []
    for s in range(5):
        fx, fy = f.rows(ix[s].numpy()), g.rows(iy[s].numpy())
        sxx, syy = orc.dyadic_kernel_sums(fx, fx, 1 / 16, 1.0, 3, True), orc.dyadic_kernel_sums(fy, fy, 1 / 16, 1.0, 3, True)
        sxy = orc.dyadic_kernel_sums(fx, fy, 1 / 16, 1.0, 3, False)
        vals.append(((sxx[0] - sxx[1]) + (syy[0] - syy[1])) / (12 * 11) - 2 * sxy[0] / 144)
    mean, std = kernel_distance(x, y, subsets=5, subset_size=12, seed=3)
    want = torch.tensor(vals, dtype=torch.float64)
    assert mean == float(want.mean()) and std == float(want.std())
    t64 = lambda v: torch.tensor([v], dtype=torch.float64)      # noqa: E731
    assert mmd2_from_sums(t64([10., 2.]), t64([7., 1.]), t64([6., 0.]), 3, 3).item() == 14 / 6 - 12 / 9


def test_kernel_distance_argument_errors_need_no_device():
    from spkdiff.evaluate import kernel_distance
    x = torch.zeros(10, 8)
    for kw in (dict(degree=0), dict(degree=9), dict(degree=2.0), dict(subset_size=11, subsets=2), dict(subsets=0, subset_size=4)):
        with pytest.raises(ValueError):
            kernel_distance(x, x, **{"subsets": 2, "subset_size": 4, **kw})
    with pytest.raises(ValueError, match="d ="):
        kernel_distance(x, torch.zeros(10, 9), subsets=2, subset_size=4)
    with pytest.raises(ValueError, match="4096"):
        kernel_distance(torch.zeros(4, 4097), torch.zeros(4, 4097), subsets=1, subset_size=2)
    with pytest.raises(ValueError):
        kernel_distance(x.double(), x, subsets=2, subset_size=4)


def test_header_constants_entry_points_and_host_side_refusals():
    from spkdiff import _lib, ops
    L = _lib.lib
    assert _lib.CONSTANTS["SPK_FEATURE_MAX_D"] == ops.FEATURE_MAX_D == 4096
    assert _lib.CONSTANTS["SPK_POLY_KERNEL_MAX_DEGREE"] == ops.POLY_KERNEL_MAX_DEGREE == 8
    assert _lib.CONSTANTS["SPK_VERSION"] == 106
    for n in ("spk_feature_moments_acc", "spk_poly_kernel_sums_ws_bytes", "spk_poly_kernel_sums"):
        assert n in _lib.EXPORTS
    ARG, UNS = _lib.CONSTANTS["SPK_ERR_ARG"], _lib.CONSTANTS["SPK_ERR_UNSUPPORTED"]
    # workspace: one pair of fp64 partials per 16x16 tile and subset
    assert L.spk_poly_kernel_sums_ws_bytes(1, 1, 1) == 16 and L.spk_poly_kernel_sums_ws_bytes(5, 17, 33) == 16 * 5 * 2 * 3
    assert L.spk_poly_kernel_sums_ws_bytes(100, 1000, 1000) == 16 * 100 * 63 * 63
    assert L.spk_poly_kernel_sums_ws_bytes(0, 4, 4) == ARG and L.spk_poly_kernel_sums_ws_bytes(1, 0, 4) == ARG
    assert L.spk_poly_kernel_sums_ws_bytes(65536, 4, 4) == UNS
    # refusals come before any launch: they need no device (the pointers are never read)
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    assert L.spk_feature_moments_acc(p, 4, 0, 4, p, p, None) == ARG
    assert L.spk_feature_moments_acc(p, -1, 4, 4, p, p, None) == ARG
    assert L.spk_feature_moments_acc(p, 4, 8, 4, p, p, None) == ARG                # row stride below d
    assert L.spk_feature_moments_acc(p, 4, 4, 4, None, p, None) == ARG
    assert L.spk_feature_moments_acc(p, 4, 4097, 4097, p, p, None) == UNS
    assert L.spk_feature_moments_acc(None, 0, 4, 4, p, p, None) == 0               # n = 0: nothing to do, nothing launched
    gc = (ctypes.c_double * 2)(0.25, 1.0)
    g = ctypes.addressof(gc)

    def ks(d=4, ix=None, iy=None, S=1, pp=2, q=2, degree=3, ws_bytes=1 << 20, nx=4, ny=4):
        return L.spk_poly_kernel_sums(p, nx, p, ny, d, ix, iy, S, pp, q, g, degree, 0, p, p, ws_bytes, None)
    assert ks(degree=0) == ARG and ks(degree=9) == ARG
    assert ks(S=2) == ARG                                                          # no tables: one subset
    assert ks(pp=5) == ARG and ks(q=5) == ARG                                      # more rows than the matrix has
    assert ks(ws_bytes=8) == ARG
    assert ks(d=4097) == UNS and ks(d=0) == ARG
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.feature_moments(torch.zeros(4, 4), torch.zeros(4, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.poly_kernel_sums(torch.zeros(4, 4), torch.zeros(4, 4))


def test_fid_score_surface_keeps_raising_for_the_network_part():
    import inspect
    ns = {}
    exec("from metric.Fid_score import *", ns)
    with pytest.raises(NotImplementedError, match="inception_v3"):
        ns["calculate_fid"](None, None, use_multiprocessing=False, batch_size=4)
    assert list(inspect.signature(ns["calculate_frechet_distance"]).parameters) == ["mu1", "sigma1", "mu2", "sigma2", "eps"]
    assert inspect.signature(ns["calculate_frechet_distance"]).parameters["eps"].default == 1e-6


def test_sample_quality_eval_names_the_alternatives():
    from spkdiff.evaluate import _feature_fn

    class NoEncoder:
        pass
    with pytest.raises(ValueError, match="'pixels'.*callable"):
        _feature_fn(NoEncoder(), "encoder", 16)
    with pytest.raises(ValueError, match="'encoder', 'pixels'"):
        _feature_fn(NoEncoder(), "inception", 16)
    f = _feature_fn(NoEncoder(), "pixels", 16)
    assert tuple(f(torch.zeros(3, 1, 4, 5)).shape) == (3, 20)
