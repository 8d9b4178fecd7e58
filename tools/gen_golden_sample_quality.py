"""Fixture F21 (tests/golden/f21_sample_quality.npz): seeded feature sets and Gaussian moments with the value of the REAL
reference's ``calculate_frechet_distance`` (R/metric/Fid_score.py:116-172, imported by path with torchvision stubbed as
oracle/gen_golden.py does) for each, and commuting-covariance cases with their closed form.

    python tools/gen_golden_sample_quality.py [--out tests/golden/f21_sample_quality.npz]

Stored (data only):
  * feature cases ``<name>/``: ``x``, ``y`` fp32 [n, d] (random correlated features: x = z A + b with a seeded mixing matrix per
    set, so the two covariances do not commute), ``ref_fd`` = the reference's value on ``np.mean(axis=0)`` / ``np.cov(rowvar=False)``;
  * commuting cases ``<name>/``: ``mu1``, ``mu2``, ``sigma1``, ``sigma2`` fp64 (sigma_i = Q diag(l_i) Q^T with ONE orthogonal Q, or
    diagonal), ``l1``, ``l2``, ``closed`` = |mu1 - mu2|^2 + sum l1 + sum l2 - 2 sum sqrt(l1 l2) (math.fsum), ``ref_fd`` and
    ``ref_err`` = |ref_fd - closed|, the reference's own error;
  * ``feature_names``, ``commuting_names``, ``numpy_version``.
Reproducing it needs the reference tree; the tests only read the .npz."""
import argparse
import importlib.util
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import REF, _load  # noqa: E402

orc = _load(os.path.join(ROOT, "tests", "_feature_stats_oracle.py"), "feature_stats_oracle")

FEATURE_CASES = (("corr_n400_d40", 400, 40, 2101), ("corr_n200_d16", 200, 16, 2102))
COMMUTING_CASES = (("diag_d16", 16, False, 2111), ("rot_d16", 16, True, 2112), ("diag_d40", 40, False, 2113),
                   ("rot_d40", 40, True, 2114))
L_MIN, L_MAX = orc.F21_L_MIN, orc.F21_L_MAX                 # eigenvalue range of the commuting cases


def reference_fid():
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tvm.inception_v3 = None
    tv.models = tvm
    sys.modules.setdefault("torchvision", tv)
    sys.modules["torchvision.models"] = tvm
    spec = importlib.util.spec_from_file_location("ref_fid_score", os.path.join(REF, "metric", "Fid_score.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def feature_set(rng, n, d):
    mix = rng.standard_normal((d, d)) / math.sqrt(d) + 0.5 * np.eye(d)
    return (rng.standard_normal((n, d)) @ mix + 0.3 * rng.standard_normal(d)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "f21_sample_quality.npz"))
    args = ap.parse_args()
    ref = reference_fid()
    f = {}
    for name, n, d, seed in FEATURE_CASES:
        rng = np.random.default_rng(seed)
        x, y = feature_set(rng, n, d), feature_set(rng, n, d)
        xd, yd = x.astype(np.float64), y.astype(np.float64)
        f[f"{name}/x"], f[f"{name}/y"] = x, y
        f[f"{name}/ref_fd"] = np.array(ref.calculate_frechet_distance(np.mean(xd, axis=0), np.cov(xd, rowvar=False),
                                                                      np.mean(yd, axis=0), np.cov(yd, rowvar=False)))
        print(f"{name}: n {n} d {d}  reference {float(f[name + '/ref_fd']):.6f}")
    for name, d, rotate, seed in COMMUTING_CASES:
        rng = np.random.default_rng(seed)
        l1, l2 = rng.uniform(L_MIN, L_MAX, d), rng.uniform(L_MIN, L_MAX, d)
        q = np.linalg.qr(rng.standard_normal((d, d)))[0] if rotate else np.eye(d)
        s1, s2 = (q * l1) @ q.T, (q * l2) @ q.T
        s1, s2 = (s1 + s1.T) / 2, (s2 + s2.T) / 2
        mu1, mu2 = rng.standard_normal(d), rng.standard_normal(d)
        closed = math.fsum([float(v) ** 2 for v in mu1 - mu2] + list(l1) + list(l2) + [-2 * math.sqrt(a * b) for a, b in zip(l1, l2)])
        r = float(ref.calculate_frechet_distance(mu1, s1, mu2, s2))
        for k, v in (("mu1", mu1), ("mu2", mu2), ("sigma1", s1), ("sigma2", s2), ("l1", l1), ("l2", l2), ("closed", np.array(closed)),
                     ("ref_fd", np.array(r)), ("ref_err", np.array(abs(r - closed)))):
            f[f"{name}/{k}"] = v
        print(f"{name}: d {d}  closed {closed:.12f}  reference {r:.12f}  |r - c| {abs(r - closed):.2e}")
    f["feature_names"] = np.array([c[0] for c in FEATURE_CASES])
    f["commuting_names"] = np.array([c[0] for c in COMMUTING_CASES])
    f["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(args.out, **f)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
