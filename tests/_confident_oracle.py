"""Host oracle of confidence-ordered decoding (the rule: csrc/psample_common.h): the schedule (``n_reveal``), the
commit rule as a literal sort loop (``commit_by_sort``) and as a mirror of the kernel's key / rank arithmetic (``commit_by_rank``),
the fp64 log-softmax of a candidate on its truncated row (``log_prob_f64``), the counted round-off bound of the kernels' fp32
confidence against it (``conf_bound``) and the seeded case table of tests/test_gpu_confident.py (``conf_inputs``).  Keys, truncation
and the fragile-cut rule are those of tests/_topk_oracle.py and tests/_topp_oracle.py.  Host tensors only."""
import math

import numpy as np
import torch

import _topk_oracle as tko
import _topp_oracle as tpo

NEG_INF = float("-inf")
KS = (2, 63, 64, 65, 128, 257, 512, 2048)
HWS = (1, 49, 64)
B = 5
TEMPS = (0.5, 1.0, 2.0, 0.25, 1.0)        # per image; powers of two: the kernel's fp32 division is exact, the host's rows are the device's
P_ROW = (1.0, 1.0, 0.5, 0.9, 1e-6)        # per image: untruncated, top-k only, nucleus only, both, p -> 0+ (a row maximum)


def k_row(K):
    return (0, 5, 0, K // 2, 0)


# ---- the schedule ---------------------------------------------------------------------------------------------------------
def n_reveal(m, t):
    """How many of the m positions still masked reverse step t reveals: ceil(m / t) in integer arithmetic, as the kernels write it."""
    return (int(m) + int(t) - 1) // int(t)


# ---- the commit rule ------------------------------------------------------------------------------------------------------
def conf_key(conf32):
    """uint32 order keys of fp32 confidences: the keys of truncate_top_k (tests/_topk_oracle.order_key); a NaN has key 0, orders last."""
    return tko.order_key(np.ascontiguousarray(conf32, dtype=np.float32))


def commit_by_sort(masked, conf32, t):
    """The definition on one image: bool [HW], the positions revealed.  Sort the masked positions by (key, -position), largest first --
    larger key first, equal keys to the lower position -- and take the first n = ceil(m / t)."""
    masked = np.asarray(masked, dtype=bool)
    keys = conf_key(conf32)
    order = sorted((p for p in range(len(masked)) if masked[p]), key=lambda p: (-int(keys[p]), p))
    out = np.zeros(len(masked), dtype=bool)
    for p in order[:n_reveal(len(order), t)]:
        out[p] = True
    return out


def commit_by_rank(masked, conf32, t):
    """The kernel's arithmetic (confident_reveal, csrc/psample_common.h) on one image: rank[p] = the number of masked p' with
    key[p'] > key[p] or (key[p'] == key[p] and p' < p); revealed iff masked and rank < n, n in unsigned 32-bit arithmetic."""
    masked = np.asarray(masked, dtype=bool)
    keys = conf_key(conf32).astype(np.uint32)
    m = np.uint32(masked.sum())
    n = (m + np.uint32(t) - np.uint32(1)) // np.uint32(t)
    pos = np.arange(len(masked))
    above = (keys[None, :] > keys[:, None]) | ((keys[None, :] == keys[:, None]) & (pos[None, :] < pos[:, None]))
    rank = (above & masked[None, :]).sum(1).astype(np.uint32)
    return masked & (rank < n)


def commit_state(x, un, cand, conf32, t, commit=commit_by_rank):
    """One reverse step on host copies of the state: x int64 [B, HW], un bool [B, HW], cand int64 [B, HW], conf32 fp32 [B, HW] (read
    at the masked positions only) -> (x, un, revealed) after the commit."""
    x, un = x.clone(), un.clone()
    rev = torch.zeros_like(un)
    for b in range(x.shape[0]):
        r = torch.from_numpy(commit(~un[b].numpy(), conf32[b].numpy(), t))
        rev[b] = r
        x[b][r] = cand[b][r]
        un[b] |= r
    return x, un, rev


# ---- the confidence -------------------------------------------------------------------------------------------------------
def log_prob_f64(zt, tok):
    """fp64 log-softmax of class tok [N] on rows zt fp32 [N, K] (already truncated: dropped classes at -inf): (z_tok - mx) - log sum
    exp(z - mx) with mx the row maximum; NaN for a row with a NaN or without a finite entry."""
    z = zt.double()
    mx = z.max(-1, keepdim=True).values
    with np.errstate(invalid="ignore"):
        lse = mx + torch.log(torch.exp(z - mx).sum(-1, keepdim=True))
    return (z.gather(1, tok[:, None]) - lse)[:, 0]


# The counted bound.  u = 2^-24 is the unit round-off of fp32 round-to-nearest.  On a truncated row l (fp32, the same bits on both
# sides: the division by a power of two is exact, the truncation is decided by exact comparisons) with maximum mx (exact), K classes
# of which nj sit in one lane, categorical_race computes
#   d_c   = fl(l_c - mx)                        one rounding: d_c (1 + a), |a| <= u
#   w_c   = expf(d_c)                           EXPF_ULP = 2 units in the last place (HIP documents 1): relative 2 * 2^-23 = 4u
#   se    = wave sum of the lane sums of w_c    nj adds in a lane, then 6 butterfly adds: every term passes nj + 6 roundings at most
#   lg    = logf(se)                            LOGF_ULP = 2 units in the last place (HIP documents 1): relative 4u of lg
#   lse   = fl(mx + lg)                         one rounding: u |lse|
#   conf  = fl(l_tok - lse)                     one rounding: u |conf|
# The subtraction's rounding moves w_c by the factor exp(a d_c), so se moves by at most u * sum |d_c| w_c; with p_c = w_c / se this is
# u * se * (H(p) - ln se) <= u * se * ln K, since se >= 1 (the maximum's term is expf(0) = 1).  A term below 2^-126 may be flushed to
# zero: K * 2^-126 in all, nothing beside u.  So se = se_true (1 + r) with |r| <= R = (1 + u ln K)(1 + 4u)(1 + u)^(nj + 6) - 1, and
#   |conf - conf_true| <= ln(1 + R) / (1 - R)  [se into its logarithm]  +  4u (ln K + R)  [logf, |lg| <= ln K + R]
#                         + u (|mx| + ln K + R)  [the add]  +  u |conf|  [the subtract],
# times (1 + 2^-10) for every product of two of these terms and for the fp64 reference's own rounding.  nj is the larger of the two
# kernels' (the sampling kernel's 4 / 8 / 16 / 32; the step tail holds 2 per 128 classes).  Counted, not fitted.
U = 2.0 ** -24
EXPF_ULP, LOGF_ULP = 2, 2


def classes_per_lane(K):
    return 4 if K <= 256 else 8 if K <= 512 else 16 if K <= 1024 else 32


def conf_bound(K, mx, conf):
    """The bound above for rows with maximum ``mx`` and (reference) confidence ``conf`` (arrays [N]); K = the row's class count."""
    mx, conf = np.abs(np.asarray(mx, dtype=np.float64)), np.abs(np.asarray(conf, dtype=np.float64))
    lnk = math.log(K)
    R = (1 + U * lnk) * (1 + EXPF_ULP * 2 * U) * (1 + U) ** (classes_per_lane(K) + 6) - 1
    e = math.log1p(R) / (1 - R) + LOGF_ULP * 2 * U * (lnk + R) + U * (mx + lnk + R) + U * conf
    return e * (1 + 2.0 ** -10)


# ---- the case table -------------------------------------------------------------------------------------------------------
def masked_counts(HW):
    """m per image of the table's start state: 0, 1, 2, HW - 1, HW, clamped to the latent."""
    return [min(max(v, 0), HW) for v in (0, 1, 2, HW - 1, HW)]


def steps_of(HW):
    """The t of the table's calls: 1, 2, 100 and m, m + 1 for every m > 0 of the start state -- t dividing m and not."""
    ts = {1, 2, 100}
    for m in masked_counts(HW):
        if m > 0:
            ts |= {m, m + 1}
    return sorted(ts)


def conf_inputs(K, HW):
    """The seeded case of (K, HW): B = 5 images, logits fp32 [B, K, HW, 1] of spread max(3, log2 K) (tests/_topp_oracle.logit_spread:
    a row's mass sits on a few classes at every K), q [B * HW, K], the start state x0 int64 / un0 bool [B, 1, HW, 1] with m = 0, 1, 2,
    HW - 1, HW masked positions at seeded places, and per image temperature, k and p."""
    g = torch.Generator().manual_seed(9000 + 7 * K + HW)
    logits = torch.randn(B, K, HW, 1, generator=g) * tpo.logit_spread(K)
    q = torch.empty(B * HW, K).exponential_(1, generator=g)
    un0 = torch.ones(B, HW, dtype=torch.bool)
    for b, m in enumerate(masked_counts(HW)):
        un0[b, torch.randperm(HW, generator=g)[:m]] = False
    x0 = torch.randint(0, K, (B, HW), generator=g)
    x0[~un0] = K
    temps = torch.tensor(TEMPS, dtype=torch.float32)
    ks = torch.tensor(k_row(K), dtype=torch.int32)
    ps = torch.tensor(P_ROW, dtype=torch.float32)
    return logits, q, x0.reshape(B, 1, HW, 1), un0.reshape(B, 1, HW, 1), temps, ks, ps


def reference_rows(logits, temps, ks, ps):
    """The host side of a case, computed once: z32 [N, K] = logits / temp per image, the rows after both truncations, the fragile-cut
    flags [N] and the nucleus-truncated flags [N] (tests/_topp_oracle.truncate)."""
    Bn, K, HW = logits.shape[0], logits.shape[1], logits[0, 0].numel()
    z32 = tpo.rows_of(logits.reshape(Bn, K, HW, 1)) / temps.repeat_interleave(HW)[:, None]
    zt, keep, fcut, on = tpo.truncate(z32.contiguous(), ks.long().repeat_interleave(HW), ps.repeat_interleave(HW).numpy())
    return z32, zt, fcut, on
