"""Host oracle of reveal schedules and annealed selection noise for confidence-ordered decoding (the rule:
csrc/psample_common.h): the count arithmetic in integers (``reveal_count``), the two named tables (``linear_weights``,
``cosine_weights``), the annealing (``noise_row``), the commit on scores as a literal sort (``commit_by_sort``) and as a mirror of the
kernel's key / rank arithmetic (``commit_by_rank``), the fp64 Gumbel and score (``gumbel_f64``, ``score_f64``) and the counted
round-off bound of the kernels' fp32 score against it (``score_bound``).  Everything here is written out again, not imported from the
package: tests/test_confident_sched_host.py compares the two.  Keys, confidences, their bound and the case table are those of
tests/_confident_oracle.py.  Host tensors only."""
import math

import numpy as np
import torch

import _confident_oracle as cfo

W_MAX = 1 << 24
U = cfo.U
LOGF_ULP = cfo.LOGF_ULP


# ---- how many ---------------------------------------------------------------------------------------------------------------
def reveal_count(m, w_prev, w_cur):
    """n of the rule: keep = w[t] == 0 ? 0 : min(m, (m * w[t - 1]) / w[t]); n = m - keep; m > 0 and n == 0: n = 1.  Python integers
    (the kernels: unsigned 64-bit; m <= 64 and w <= 2^24 keep the product below 2^31)."""
    m, w_prev, w_cur = int(m), int(w_prev), int(w_cur)
    assert 0 <= m and 0 <= w_prev <= W_MAX and 0 <= w_cur <= W_MAX and m * w_prev < (1 << 64)
    keep = 0 if w_cur == 0 else min(m, (m * w_prev) // w_cur)
    n = m - keep
    return 1 if (m > 0 and n == 0) else n


def linear_weights(e):
    return [t for t in range(e + 1)]


def cosine_weights(e):
    """rint(2^24 sin(pi t / (2 e))) in fp64 (np.rint: ties to even, as rint)."""
    return [int(np.rint(np.float64(W_MAX) * np.sin(np.float64(np.pi) * np.float64(t) / (2.0 * np.float64(e))))) for t in range(e + 1)]


def run_counts(m0, w):
    """The counts of a whole run from m0 masked positions: t = e .. 1."""
    m, out = int(m0), []
    for t in range(len(w) - 1, 0, -1):
        n = reveal_count(m, w[t - 1], w[t])
        out.append(n)
        m -= n
    return out


def noise_row(tau, e, S):
    """a[t] = fp32(tau * (t - 1) / e) for 1 <= t <= e, 0 elsewhere; the product and the quotient in fp64."""
    return [float(np.float32(np.float64(tau) * np.float64(t - 1) / np.float64(e))) if 1 <= t <= e else 0.0 for t in range(S + 1)]


# ---- in what order ----------------------------------------------------------------------------------------------------------
def commit_by_sort(masked, score32, n):
    """The definition on one image: sort the masked positions by (key of the score, -position), largest first, take the first n."""
    masked = np.asarray(masked, dtype=bool)
    keys = cfo.conf_key(score32)
    order = sorted((p for p in range(len(masked)) if masked[p]), key=lambda p: (-int(keys[p]), p))
    out = np.zeros(len(masked), dtype=bool)
    for p in order[:int(n)]:
        out[p] = True
    return out


def commit_by_rank(masked, score32, n):
    """The kernel's arithmetic (confident_reveal_n): rank[p] = the number of masked p' with key[p'] > key[p] or (equal and p' < p);
    revealed iff masked and rank < n, unsigned 32-bit."""
    masked = np.asarray(masked, dtype=bool)
    keys = cfo.conf_key(score32).astype(np.uint32)
    pos = np.arange(len(masked))
    above = (keys[None, :] > keys[:, None]) | ((keys[None, :] == keys[:, None]) & (pos[None, :] < pos[:, None]))
    rank = (above & masked[None, :]).sum(1).astype(np.uint32)
    return masked & (rank < np.uint32(n))


def commit_state(x, un, cand, score32, w_prev, w_cur, commit=commit_by_sort):
    """One step on host copies: x int64 [B, HW], un bool [B, HW], cand int64 [B, HW], score32 fp32 [B, HW]; w_prev / w_cur: B
    integers each (w[i][t - 1], w[i][t]) -> (x, un, revealed, counts)."""
    x, un = x.clone(), un.clone()
    rev = torch.zeros_like(un)
    counts = []
    for b in range(x.shape[0]):
        m = int((~un[b]).sum())
        n = reveal_count(m, w_prev[b], w_cur[b])
        r = torch.from_numpy(commit(~un[b].numpy(), score32[b].numpy(), n))
        rev[b] = r
        x[b][r] = cand[b][r]
        un[b] |= r
        counts.append(n)
    return x, un, rev, counts


def gumbel_f64(u):
    """g = -ln(-ln u) in fp64 for u in (0, 1) (fp32 uniforms, exact in fp64)."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return -np.log(-np.log(u))


def score_f64(conf64, a, u):
    return np.asarray(conf64, dtype=np.float64) + np.asarray(a, dtype=np.float64) * gumbel_f64(u)


# The counted bound of the fp32 score.  u = 2^-24 is the unit round-off, r = LOGF_ULP * 2u the relative error of one logf
# (LOGF_ULP = 2 units in the last place, as tests/_confident_oracle.py counts it; HIP documents 1).  With U in (0, 1) an fp32 uniform
# (exact on both sides), a the fp32 noise scale (exact on both sides) and conf the kernel's fp32 confidence, sched_score computes
#   L1    = logf(U)                 = ln U (1 + r1),  |r1| <= r;  x = -L1 is exact
#   L2    = logf(x)                 = ln x (1 + r2),  |r2| <= r;  ln x = ln(-ln U) + ln(1 + r1),  |ln(1 + r1)| <= r / (1 - r)
#   g     = -L2                     : |g - g64| <= Eg = r / (1 - r) + r (|g64| + r / (1 - r))
#   prod  = fl(a * g)               : |prod - a g64| <= Ep = |a| Eg + u |a| (|g64| + Eg)
#   score = fl(conf + prod)         : |score - s64| <= Ec + Ep + u (|s64| + Ec + Ep)
# with s64 = conf64 + a g64 and Ec = conf_bound, the counted bound of |conf - conf64| (tests/_confident_oracle.py), times (1 + 2^-10)
# for the fp64 reference's own roundings.  -ln U lies in [2^-24.0.., 17): both logf arguments are normal numbers.  Counted, not fitted.
def score_bound(K, mx, conf64, a, u):
    """The bound above: rows with truncated-row maximum ``mx``, reference confidence ``conf64``, noise scale ``a`` (fp32 value) and
    uniform ``u`` (arrays [N])."""
    conf64 = np.asarray(conf64, dtype=np.float64)
    s64 = np.abs(score_f64(conf64, a, u))
    a = np.abs(np.asarray(a, dtype=np.float64))
    g = np.abs(gumbel_f64(u))
    r = LOGF_ULP * 2 * U
    eg = r / (1 - r) + r * (g + r / (1 - r))
    ep = a * eg + U * a * (g + eg)
    ec = cfo.conf_bound(K, mx, conf64)
    return (ec + ep + U * (s64 + ec + ep)) * (1 + 2.0 ** -10)


# ---- the tables of the GPU case table --------------------------------------------------------------------------------------
def custom_tables(S):
    """Three custom tables of S + 1 weights: a zero weight in the middle (w[t] = 0 reveals everything at t, and w[t - 1] = 0 at the
    step above it), a non-monotone pair (w[t - 1] > w[t]: the min keeps all, the forced 1 reveals one) and a staircase with the
    largest weight."""
    zero = [t * 3 for t in range(S + 1)]
    zero[max(S // 2, 1)] = 0
    bump = [t * 5 + 1 for t in range(S + 1)]
    bump[0] = 0
    for t in range(2, S + 1, 3):
        bump[t - 1] = bump[t] + 7                    # (w[t - 1] > w[t])
    stair = [min(W_MAX, (t // 2) * (W_MAX // max(S // 2, 1))) for t in range(S + 1)]
    stair[S] = W_MAX
    return {"zero": zero, "bump": bump, "stair": stair}


def table_rows(S, B=cfo.B):
    """Per-image rows [B][S + 1] of the case table: linear, cosine and the three custom tables, one per image (cycled)."""
    tabs = [linear_weights(S), cosine_weights(S)] + list(custom_tables(S).values())
    return [tabs[b % len(tabs)] for b in range(B)]
