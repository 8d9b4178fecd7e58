"""Host oracle of csrc/feature_stats.hip (spk_feature_moments_acc, spk_poly_kernel_sums) and of spkdiff.evaluate's distances.

Features are built on a grid so that EXACT sums are cheap: x[k, c] = g[k, c] * 2^-(G_BITS + r[k] + s[c]) with integers |g| < 2^23
and small per-row / per-column exponents r, s.  Every x is an fp32 number, every product an integer times a power of two, and a
sum over rows (the Gram matrix) or over columns (a dot product) is a sum of int64-exact matrix products, one per exponent of the
inner index, combined as Python integers: the exact value, rounded ONCE to fp64 (int -> float is correctly rounded) -- what
``math.fsum`` over the fp64 products returns, which the small cases check term by term (``gram_fsum``).  The spread of exponents is
what makes the device's fp64 partial sums round at all: on a single grid a few hundred 46-bit products add exactly.

"Dyadic" cases: g in {-2 .. 2}, x = g / 4, d a power of two, gamma = 1 / d, coef = 1.  Then products, sums, gamma * dot + coef and
its powers are exact in fp64 in ANY order, and the device must match bit for bit; ``dyadic_budget`` asserts the bit budget (worked
example: d = 16, gamma = 1 / 16: v = (G + 256) / 256 with |G| <= 64, so |v^3| < 2^25 in units of 2^-24 and 2^16 pairs sum below
2^41; the assert does this arithmetic for the case at hand).

Error bounds (u = 2^-53, the unit roundoff), from the contract in include/spkdiff.h:
  * gram[i, j]: products exact; one chain of ceil(n / 4) MFMAs from the stored value, each adding four exact products to the
    accumulator.  Counted as one rounding of a partial sum per MFMA plus three for the adds inside the first one:
    GRAM_ROUNDINGS(n) = ceil(n / 4) + 3, and every partial sum is at most S = sum_k |x_ki x_kj| (1 + small), so
    |err| <= GRAM_ROUNDINGS(n) u S (1 + 2^-40 for the second-order terms).
  * sum[c]: a sequential chain, n roundings: n u sum_k |x_kc|.
  * a kernel sum: dot_ij within DOT_ROUNDINGS(d) u sum_c |x_ic y_jc|; v = fl(fl(gamma dot) + coef) adds u |gamma dot| + u |v|; the
    power by repeated multiplication adds (deg - 1) u |v|^deg to deg |v|^(deg - 1) |dv|; the sums add SUM_DEPTH(tiles) u sum |k|
    (4 registers, 6 butterfly steps, ceil(tiles / 256) chain steps, 8 tree steps)."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
G_BITS = 21                                           # g * 2^-21: |x| < 4 on the coarsest grid
E_STEPS = (0, 5, 10)                                  # the exponents r[k] and s[c] are drawn from
E_MAX = max(E_STEPS)

# (n, d) of the GPU tests
MOMENT_DYADIC = ((1, 16), (3, 16), (4, 32), (257, 64), (130, 1024))
MOMENT_REAL = ((5, 40), (257, 100), (130, 784))
KSUM_DYADIC_D = (16, 64)
KSUM_DYADIC_PQ = ((1, 1), (17, 33), (257, 130))
KSUM_REAL = ((40, 37, 21), (784, 33, 18))             # (d, p, q)


class Feat:
    """g int64 [n, d], r int [n], s int [d]; x fp32 = g * 2^-(G_BITS + r[k] + s[c])."""

    def __init__(self, g, r, s):
        self.g, self.r, self.s = np.asarray(g, np.int64), np.asarray(r, np.int64), np.asarray(s, np.int64)
        x64 = np.ldexp(self.g.astype(np.float64), -(G_BITS + self.r[:, None] + self.s[None, :]))
        self.x = x64.astype(np.float32)
        assert np.array_equal(self.x.astype(np.float64), x64), "the grid value is not an fp32 number"

    def rows(self, idx):
        idx = np.asarray(idx, np.int64)
        return Feat(self.g[idx], self.r[idx], self.s)


def real_features(n, d, seed):
    rng = np.random.default_rng(seed)
    g = np.clip(np.rint(rng.standard_normal((n, d)) * 2 ** G_BITS), -(2 ** 23) + 1, 2 ** 23 - 1)
    return Feat(g, rng.choice(E_STEPS, n), rng.choice(E_STEPS, d))


def dyadic_features(n, d, seed):
    """x = g / 4, g in {-2 .. 2} (as a Feat: g * 2^19 on the coarse grid, no exponents)."""
    assert d & (d - 1) == 0, "dyadic cases take d a power of two (gamma = 1 / d exact)"
    rng = np.random.default_rng(seed)
    return Feat(rng.integers(-2, 3, (n, d)) * 2 ** (G_BITS - 2), np.zeros(n), np.zeros(d))


def _exact_inner(A, B, e):
    """T[i, j] = sum_k A[k, i] B[k, j] 2^(2 (E_MAX - e[k])) as Python integers (object array): int64-exact per exponent group."""
    T = np.zeros((A.shape[1], B.shape[1]), dtype=object)
    for ev in np.unique(e):
        sel = e == ev
        assert sel.sum() * 2 ** 46 < 2 ** 62, "an exponent group would overflow int64"
        T = T + (A[sel].T @ B[sel]).astype(object) * (1 << int(2 * (E_MAX - ev)))
    return T


def _round_scaled(T, exp2):
    """float(T[i, j]) (correctly rounded) * 2^exp2[i, j] (exact)."""
    f = np.array([[float(v) for v in row] for row in T], dtype=np.float64).reshape(T.shape)
    return np.ldexp(f, exp2)


def moments_oracle(f):
    """(sum fp64 [d], gram fp64 [d, d]): the exact sums rounded once; (abs_sum, abs_gram): sum |x|, sum |x_ki x_kj| for the bounds."""
    T = _exact_inner(f.g, f.g, f.r)
    gram = _round_scaled(T, -(2 * G_BITS + 2 * E_MAX) - (f.s[:, None] + f.s[None, :]))
    w = (1 << (E_MAX - f.r)).astype(np.int64)[:, None]
    ssum = np.ldexp((f.g * w).sum(axis=0).astype(np.float64), -(G_BITS + E_MAX) - f.s)       # < 2^53: exact
    assert np.abs((np.abs(f.g) * w).sum(axis=0)).max() < 2 ** 53
    ax = np.abs(f.x.astype(np.float64))
    return ssum, gram, ax.sum(axis=0) * (1 + 1e-12), (ax.T @ ax) * (1 + 1e-12)


def gram_fsum(x):
    """The definition, term by term: math.fsum over the fp64 products of the fp32 features (small cases only)."""
    x = x.astype(np.float64)
    d = x.shape[1]
    return (np.array([math.fsum(x[:, c]) for c in range(d)]),
            np.array([[math.fsum(x[:, i] * x[:, j]) for j in range(d)] for i in range(d)]))


def GRAM_ROUNDINGS(n):
    return (n + 3) // 4 + 3


def gram_bound(n, abs_gram):
    return GRAM_ROUNDINGS(n) * U * abs_gram * (1 + 2.0 ** -40)


def sum_bound(n, abs_sum):
    return n * U * abs_sum * (1 + 2.0 ** -40)


def chain_split_bound(n_a, n_b, abs_gram):
    """update(A); update(B) against update(cat(A, B)) when len(A) % 4 != 0: each is within its own counted bound of the exact sum."""
    return (GRAM_ROUNDINGS(n_a) + GRAM_ROUNDINGS(n_b) + GRAM_ROUNDINGS(n_a + n_b)) * U * abs_gram * (1 + 2.0 ** -40)


# ---- kernel sums -------------------------------------------------------------------------------------------------------------
def DOT_ROUNDINGS(d):
    return (d + 3) // 4 + 3


def SUM_DEPTH(p, q):
    tiles = ((p + 15) // 16) * ((q + 15) // 16)
    return 3 + 6 + (tiles + 255) // 256 + 8


def exact_dots(fx, fy):
    """dots[i, j] = <x_i, y_j> as Fractions (object array) and sum_c |x_ic y_jc| (fp64, inflated)."""
    assert np.array_equal(fx.s, fy.s)
    T = _exact_inner(fx.g.T.copy(), fy.g.T.copy(), fx.s)
    sh = 2 * G_BITS + 2 * E_MAX
    dots = np.empty(T.shape, dtype=object)
    for i in range(T.shape[0]):
        for j in range(T.shape[1]):
            dots[i, j] = Fraction(int(T[i, j]), 1 << int(sh + fx.r[i] + fy.r[j]))
    ax, ay = np.abs(fx.x.astype(np.float64)), np.abs(fy.x.astype(np.float64))
    return dots, (ax @ ay.T) * (1 + 1e-12)


def kernel_term_bounds(x, y, gamma, coef, degree, dot_roundings, depth):
    """fp64 [p, q]: the error bound of every term (gamma <x_i, y_j> + coef)^degree as it enters a sum (module docstring), for an
    implementation whose dot product rounds ``dot_roundings`` times and whose sums are ``depth`` deep.  x, y: fp32 / fp64 arrays."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    dots, adots = x @ y.T, (np.abs(x) @ np.abs(y).T) * (1 + 1e-12)
    av = (np.abs(gamma * dots + coef) + 4 * U * (abs(gamma) * adots + abs(coef))) * (1 + 1e-12)
    ak = av ** degree
    dv = abs(gamma) * dot_roundings * U * adots + U * abs(gamma) * adots + U * av
    return (degree * av ** (degree - 1) * dv + (degree - 1) * U * ak) * 1.01 + depth * U * ak


def kernel_sums_oracle(fx, fy, gamma, coef, degree, symmetric):
    """(total, diag, bound_total, bound_diag) of one subset whose rows are fx, fy in order: exact rationals rounded once, and the
    device's error bound derived in the module docstring."""
    dots, _ = exact_dots(fx, fy)
    g, c = Fraction(gamma), Fraction(coef)
    p, q = dots.shape
    tot, dia = Fraction(0), Fraction(0)
    for i in range(p):
        for j in range(q):
            k = (g * dots[i, j] + c) ** degree
            tot += k
            if symmetric and i == j:
                dia += k
    dk = kernel_term_bounds(fx.x, fy.x, gamma, coef, degree, DOT_ROUNDINGS(fx.x.shape[1]), SUM_DEPTH(p, q))
    return float(tot), float(dia), float(dk.sum()), float(np.trace(dk[:min(p, q), :min(p, q)])) if symmetric else 0.0


def dyadic_budget(d, p, q, degree, gamma, coef):
    """The bit budget that makes a dyadic kernel sum exact in fp64 in any order: asserts it and returns the unit exponent."""
    a = int(round(-math.log2(gamma)))
    assert gamma == 2.0 ** -a and a >= 0 and float(coef).is_integer(), "dyadic cases take gamma a power of two and an integer coef"
    unit = 4 + a                                        # dot = G / 16, gamma dot = G / 2^(4 + a)
    vmax = 4 * d + abs(int(coef)) * 2 ** unit           # |G| <= 4 d: products of {-2 .. 2}
    assert math.log2(vmax) * degree + math.log2(p * q) < 53, f"dyadic case d={d} p={p} q={q} degree={degree} is not exact in fp64"
    return unit


def dyadic_kernel_sums(fx, fy, gamma, coef, degree, symmetric):
    """Exact (total, diag) of a dyadic subset by integer arithmetic."""
    d = fx.x.shape[1]
    p, q = fx.x.shape[0], fy.x.shape[0]
    unit = dyadic_budget(d, p, q, degree, gamma, coef)
    gx, gy = fx.g >> (G_BITS - 2), fy.g >> (G_BITS - 2)          # back to {-2 .. 2}
    V = gx @ gy.T + int(coef) * (1 << unit)            # int64: the budget keeps every power and the sum below 2^53
    K = V ** degree
    tot = int(K.sum())
    dia = int(np.trace(K[:min(p, q), :min(p, q)])) if symmetric else 0
    scale = 1 << (unit * degree)
    assert abs(tot) < 2 ** 53 and tot / scale == Fraction(tot, scale)
    return tot / scale, dia / scale


def subset_tables(n_x, n_y, S, p, q, seed):
    """Tables that repeat and permute rows: int32 [S, p], [S, q]."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_x, (S, p)).astype(np.int32), rng.integers(0, n_y, (S, q)).astype(np.int32)


# ---- Frechet distance --------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -52
F21_L_MIN, F21_L_MAX = 0.25, 4.0                      # eigenvalue range of fixture F21's commuting cases (the generator reads these)


def frechet_exact_bound(d, l_min, l_max, tr):
    """|frechet_distance('exact') - closed form| on a commuting case with eigenvalues in [l_min, l_max]: the matrix
    M = sqrt(C1) C2 sqrt(C1) (norm <= l_max^2) is formed with an entry error of about 3 d eps l_max^2 (two products and the root),
    so its eigenvalues move by at most d times that; sqrt has slope 1 / (2 l_min) at the smallest eigenvalue l_min^2 of M; d of
    them are added and doubled.  The traces and |mu1 - mu2|^2 add d eps tr.  The stored sigmas are themselves Q diag(l) Q^T in
    fp64, a perturbation of the same order, covered by the factor 2."""
    return 2 * (2 * d * (3 * d * d * EPS * l_max ** 2) / (2 * l_min) + 4 * d * EPS * tr)


def frechet_reference_tol(d, tr, ref_err_same_d):
    """The allowance for the reference convention against the reference's recorded value: 10 x the reference's own error on the
    commuting cases of this d, floored at 8 d eps (tr C1 + tr C2) -- a dot product of length d has error d eps |terms|, the value
    is a sum of traces of such products, and another LAPACK build may order an SVD's roundings differently."""
    return max(10 * ref_err_same_d, 8 * d * EPS * tr)
