"""Host oracle of nucleus (top-p) truncated sampling: the integer masses (``masses``), the definition given those
masses as a per-row sort loop (``nucleus_by_sort``), a numpy mirror of the kernel's key, integer bit descent and fp64 compare
(``nucleus_by_bits``, csrc/psample_common.h ``truncate_top_p``), the fragility rule of the GPU tests (``fragile_cut``), the fp64 race
on the truncated row (``oracle_tokens``), the reference's reverse loop with the truncation lines in front of the categorical draw
(``run``) and the seeded case table of tests/test_gpu_topp.py (``topp_inputs``).  Host tensors only."""
import numpy as np
import torch

import _topk_oracle as tko
from oracle import snn_ref as ref

NEG_INF = float("-inf")
SCALE = float(1 << 20)                   # a class's weight expf(z - mx) in [0, 1] becomes an integer mass in [0, 2^20]
P_CYCLE = (1.0, 1e-6, 0.25, 0.5, 0.9, 0.999)
KS = (2, 63, 64, 65, 128, 257, 512, 2048)
KINDS = ("randn", "neg_inf", "ties")
TEMPS = (0.25, 0.5, 1.0)                 # the uniform temperatures of the kernel test (powers of two: the division is exact)
FRAGILE_SHARE_CAP = 0.10                 # of the nucleus-truncated rows of a case; a condition on the case table, not a measurement

# The fragility rule.  The host cannot reproduce the device's expf bit for bit, so its masses may differ from the device's.  With
# mt_c = 2^20 * exp(z_c - mx) in fp64 (z, mx and the subtraction in fp32, as the kernel makes them -- those are bit-identical on both
# sides) a device mass is m_c = rint(mt_c * (1 + d)), |d| <= EXPF_REL: |m_c - mt_c| <= 0.5 + EXPF_REL * mt_c, the 0.5 from the
# rounding to an integer, the other term from an expf that is off by at most EXPF_ULP units in the last place (an fp32 ulp is at most
# 2^-23 of the value; HIP documents 1 ulp for expf, 2 allows for it generously).  Where mt_c * (1 + EXPF_REL) < 0.5 both sides round
# to 0 and the deviation is mt_c itself (< 0.5; nothing for the classes at -inf), so the allowance per class is e_c = mt_c there and
# 0.5 + EXPF_REL * mt_c elsewhere: never more than 0.5 + EXPF_REL * mt_c.  A cut compares S = the sum over a prefix of the classes with P = p * total: the deviation of S is at most the sum
# over the prefix, that of P at most p < 1 times the sum over the row, so twice the row's sum bounds |(S - P) - (St - Pt)| (the fp64
# product's own rounding, 2^-53 * 2^31, is nothing beside it).  A row is fragile when some cut between distinct values has
# |St - Pt| <= E; on every other row the device's comparisons come out as the host's, and so does the kept set.
EXPF_ULP = 2
EXPF_REL = EXPF_ULP * 2.0 ** -23


def masses(z32):
    """uint32 [N, K] integer masses of fp32 rows z32 [N, K] (numpy; a row after its top-k truncation) and the fp32 row maximum:
    m_c = rint(2^20 * expf(z_c - mx)), ties to even, with expf correctly rounded from fp64; 0 for a NaN.  Rows whose maximum is not
    finite get zeros (they are not truncated)."""
    z32 = np.ascontiguousarray(z32, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.fmax.reduce(z32, axis=1, initial=np.float32(NEG_INF))            # fmaxf: NaNs ignored
        ok = np.isfinite(mx)
        d = (z32 - np.where(ok, mx, np.float32(0))[:, None]).astype(np.float32)  # the one fp32 subtraction
        w = np.exp(d.astype(np.float64)).astype(np.float32)                      # expf, correctly rounded
        m = np.rint((w * np.float32(SCALE)).astype(np.float32))                  # (exact scaling by a power of two)
    m = np.where(np.isnan(z32) | ~ok[:, None], 0.0, m).astype(np.uint32)
    return m, mx


def nucleus_by_sort(z_row, m_row, p):
    """The definition on one row, given its integer masses: bool [K], the classes that stay.  Sort the classes that count (not NaN)
    by key, largest first; walk down group by group of equal keys adding masses; stop at the first group where the sum reaches
    P = p * total in fp64; tau is that group's value and every class with z < tau (the float comparison) goes.  A p outside (0, 1)
    or a row maximum that is not finite: everything stays."""
    K = len(z_row)
    keep = np.ones(K, dtype=bool)
    p32 = np.float32(p)
    if not (p32 > 0 and p32 < 1):
        return keep
    vals = [float(v) for v in z_row if not np.isnan(v)]
    if not vals or not np.isfinite(max(vals)):
        return keep
    keys = tko.order_key(np.asarray(z_row, dtype=np.float32))
    total = int(sum(int(v) for v in m_row))
    P = float(np.float64(p32) * np.float64(total))
    order = sorted((c for c in range(K) if keys[c] != 0), key=lambda c: -int(keys[c]))
    s, i, tau = 0, 0, None
    while i < len(order):
        j = i
        while j < len(order) and keys[order[j]] == keys[order[i]]:
            s += int(m_row[order[j]])
            j += 1
        if float(s) >= P:
            tau = np.float32(z_row[order[i]])
            break
        i = j
    assert tau is not None                                   # (the whole row sums to total >= P)
    for c in range(K):
        if z_row[c] < tau:
            keep[c] = False
    return keep


def nucleus_by_bits(z32, m, p_rows):
    """tau fp32 [N] as the kernel finds it on rows z32 fp32 [N, K] with masses m uint32 [N, K] and p fp32 [N]: the largest key T with
    (double) S(T) >= (double) p * (double) total, built from bit 31 down, mapped back to its float; -inf (nothing is below it) for a
    row that is not truncated."""
    z32 = np.ascontiguousarray(z32, dtype=np.float32)
    p32 = np.asarray(p_rows, dtype=np.float32)
    key = tko.order_key(z32)
    m = m.astype(np.uint32)
    total = m.sum(1, dtype=np.uint32)                                             # uint32, as the kernel sums
    P = p32.astype(np.float64) * total.astype(np.float64)
    T = np.zeros(z32.shape[0], dtype=np.uint32)
    for bit in range(31, -1, -1):
        trial = T | np.uint32(1 << bit)
        s = np.where(key >= trial[:, None], m, np.uint32(0)).sum(1, dtype=np.uint32)
        T = np.where(s.astype(np.float64) >= P, trial, T).astype(np.uint32)
    bits = np.where(T & np.uint32(0x80000000), T & np.uint32(0x7FFFFFFF), ~T).astype(np.uint32)
    tau = bits.view(np.float32).copy()
    with np.errstate(invalid="ignore"):
        mx = np.fmax.reduce(z32, axis=1, initial=np.float32(NEG_INF))
    on = (p32 > 0) & (p32 < 1) & np.isfinite(mx)
    tau[~on] = np.float32(NEG_INF)
    return tau


def class_allowance(mt):
    """e_c of the rule above: how far a device mass may lie from the fp64 mass mt_c."""
    return np.where(mt * (1.0 + EXPF_REL) < 0.5, mt, 0.5 + EXPF_REL * mt)


def rows_of(logits):
    """[B, K, h, w] -> [B * h * w, K]: one row per position, in the kernels' position order."""
    return logits.flatten(2).permute(0, 2, 1).reshape(-1, logits.shape[1])


def truncated_rows(p_rows, mx):
    """bool [N]: the rows the nucleus truncation works on -- 0 < p < 1 (fp32) and a finite row maximum."""
    p32 = np.asarray(p_rows, dtype=np.float32)
    return (p32 > 0) & (p32 < 1) & np.isfinite(mx)


def fragile_cut(z32, p_rows):
    """bool [N]: rows (after top-k) with a cut between distinct values closer to P than E (the rule above); False for rows that are
    not nucleus-truncated.  Also returns E [N]."""
    z32 = np.ascontiguousarray(z32, dtype=np.float32)
    p32 = np.asarray(p_rows, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.fmax.reduce(z32, axis=1, initial=np.float32(NEG_INF))
        on = truncated_rows(p32, mx)
        d = (z32 - np.where(np.isfinite(mx), mx, np.float32(0))[:, None]).astype(np.float32)
        mt = SCALE * np.exp(d.astype(np.float64))
    mt = np.where(np.isnan(z32), 0.0, mt)
    E = 2.0 * class_allowance(mt).sum(1)
    zs = np.where(np.isnan(z32), np.float32(NEG_INF), z32)                        # (a NaN counts for nothing: below every cut)
    order = np.argsort(-zs, axis=1, kind="stable")
    zsrt = np.take_along_axis(zs, order, 1)
    S = np.cumsum(np.take_along_axis(mt, order, 1), axis=1)
    P = p32.astype(np.float64)[:, None] * S[:, -1:]
    cut = zsrt[:, :-1] != zsrt[:, 1:]                                              # a cut below sorted position i
    near = np.abs(S[:, :-1] - P) <= E[:, None]
    return (cut & near).any(1) & on, E


def truncate(z32, k_rows, p_rows):
    """Rows z32 (torch fp32 [N, K]) -> (the rows after top-k and nucleus truncation, kept bool [N, K], fragile_cut bool [N],
    nucleus-truncated bool [N]).  k_rows int [N], p_rows fp32 [N]."""
    zk = tko.truncate(z32, k_rows)
    zn = zk.numpy()
    m, mx = masses(zn)
    tau = torch.from_numpy(nucleus_by_bits(zn, m, np.asarray(p_rows, dtype=np.float32)))
    keep = ~(zk < tau[:, None]) & ~(z32 < tko._tau_rows(z32, k_rows))
    frag, _ = fragile_cut(zn, p_rows)
    return zk.masked_fill(zk < tau[:, None], NEG_INF), keep, torch.from_numpy(frag), torch.from_numpy(truncated_rows(p_rows, mx))


def oracle_tokens(z32, k_rows, p_rows, q, thr):
    """fp64 race on the truncated rows: (token [N] -- first index on a tie, 0 for a row without a comparable ratio --, fragile [N]:
    a fragile cut, or the two largest ratios closer than ``thr`` relative to the largest (the race oracle's rule), kept bool [N, K],
    fragile_cut [N], nucleus-truncated [N])."""
    zt, keep, fcut, on = truncate(z32, k_rows, p_rows)
    tok, fragile = race_tokens(zt, fcut, q, thr)
    return tok, fragile, keep, fcut, on


def race_tokens(zt, fcut, q, thr):
    """The fp64 race on rows already truncated (``truncate``): (token [N], fragile [N] = ``fcut`` or a fragile race)."""
    r = torch.softmax(zt.double(), -1) / q.double()
    allnan = torch.isnan(r).all(-1)
    r = torch.where(torch.isnan(r), torch.full_like(r, -1.0), r)
    tok = r.argmax(-1)
    tok[allnan] = 0
    if r.shape[1] < 2:
        return tok, fcut.clone()
    top = r.topk(2, -1).values
    frace = ((top[:, 0] - top[:, 1]) < thr * top[:, 0]) & ~allnan & ~torch.isinf(top[:, 0])
    return tok, frace | fcut


def topp_inputs(K, kind):
    """The seeded case table of tests/test_gpu_topp.py: HW = 49, B = 21 (11 at K = 2048), seed 7000 + K.  Logits of the three kinds
    (image 5 -- p = 0.999, no top-k -- holds a NaN at position 0 and is all -inf at position 1), then q, u, the state, p and k per image.  The spread of the logits grows with
    log K so that a row's mass sits on a few classes at every K, as a trained denoiser's does."""
    B = 11 if K == 2048 else 21
    g = torch.Generator().manual_seed(7000 + K)
    r = torch.randn(B, K, 7, 7, generator=g)
    hole = torch.rand(B, K, 7, 7, generator=g) < 0.3
    hole[:, K // 2] = False                                      # (every position keeps a finite class)
    s = logit_spread(K)
    if kind == "randn":
        logits = r * s
    elif kind == "neg_inf":
        logits = r * s
        logits[hole] = NEG_INF
    else:
        logits = torch.round(2 * r * s) / 2                      # "ties": half-integer logits, many rows tie at tau
    logits[5, K // 2, 0, 0] = float("nan")
    logits[5, :, 0, 1] = NEG_INF
    q = torch.empty(B * 49, K).exponential_(1, generator=g)
    u = torch.rand(B * 49, generator=g)
    un0 = torch.rand(B, 1, 7, 7, generator=g) < 0.4
    x0 = torch.randint(0, K, (B, 1, 7, 7), generator=g)
    x0[~un0] = K
    ps = torch.tensor([P_CYCLE[b % 6] for b in range(B)], dtype=torch.float32)
    kc = [0, 0, 5, K // 2, K - 1]
    ks = torch.tensor([kc[b % 5] for b in range(B)], dtype=torch.int32)
    return logits, q, u, x0, un0, ps, ks


def logit_spread(K):
    return max(3.0, float(np.log2(K)))


def run(sd, B, steps, noise, top_p, top_k=0, K=128, mask_id=None, temp=1.0, T=16, L=7, exact_conv=False, margins=None, cuts=None):
    """The reference's reverse loop (oracle/snn_ref.py: ``denoiser_forward`` + the body of ``p_sample_step``) from the all-masked
    state with the two truncations inserted between ``logits / temp`` and ``categorical_sample``.  ``noise``: t -> (u [B,1,L,L], q
    [B*L*L, K]); ``top_p`` / ``top_k``: one value for every image.  ``margins`` (a list) receives, per step, the relative gap of the
    two largest fp64 ratios at the positions that change; ``cuts`` (a list) the number of changing positions with a fragile cut.
    Returns x_t [B,1,L,L]."""
    mask_id = K if mask_id is None else mask_id
    x_t = torch.full((B, 1, L, L), mask_id, dtype=torch.long)
    unmasked = torch.zeros((B, 1, L, L), dtype=torch.bool)
    n = B * L * L
    for t in reversed(range(1, steps + 1)):
        u, q = noise(t)
        tt = torch.full((B,), t, dtype=torch.long)
        logits = ref.denoiser_forward(x_t.float(), tt, sd, T, exact_conv=exact_conv).permute(0, 2, 3, 1)     # [B,L,L,K]
        changes = (u < 1 / torch.full_like(u, float(t))) & ~unmasked
        unmasked = unmasked | changes
        z32 = (logits / temp).reshape(n, K).contiguous()
        zt, _, fcut, _ = truncate(z32, torch.full((n,), int(top_k)), np.full(n, top_p, dtype=np.float32))    # the new lines
        x_0_hat = ref.categorical_sample(zt.reshape(B, L, L, K), q).long().unsqueeze(dim=1)
        if margins is not None:
            r = torch.softmax(zt.double(), -1) / q.double()
            top = r.topk(2, -1).values
            margins.append(((top[:, 0] - top[:, 1]) / top[:, 0])[changes.flatten()])
        if cuts is not None:
            cuts.append(int(fcut[changes.flatten()].sum()))
        x_t = x_t.clone()
        x_t[changes] = x_0_hat[changes]
    return x_t
