"""Host oracle of top-k truncated sampling: the definition in torch (``truncate``), a numpy mirror of the kernel's
order-preserving key and bit-wise select (``kth_largest_by_bits``, csrc/psample_common.h ``truncate_top_k``), the fp64 race on the
truncated row (``oracle_tokens``) and the reference's reverse loop with the one truncation line in front of the categorical draw
(``run``).  Host tensors only."""
import numpy as np
import torch

from oracle import snn_ref as ref

NEG_INF = float("-inf")


def truncate(z, k):
    """The definition on rows z [..., K] (NaN-free): k <= 0 or k >= K leaves the row; otherwise every class below the k-th largest
    entry (counting multiplicity, IEEE comparison: classes equal to it stay) becomes -inf.  ``k``: an int, or one per row ([...])."""
    K = z.shape[-1]
    if torch.is_tensor(k):
        out = z.clone()
        for kv in k.unique().tolist():
            sel = k == kv
            out[sel] = truncate(z[sel], int(kv))
        return out
    if k <= 0 or k >= K:
        return z
    return z.masked_fill(z < z.topk(k, dim=-1).values[..., -1:], NEG_INF)


def kept(z, k):
    """bool [..., K]: the classes ``truncate`` keeps (all of them for k <= 0 or k >= K)."""
    K = z.shape[-1]
    if k <= 0 or k >= K:
        return torch.ones_like(z, dtype=torch.bool)
    return ~(z < z.topk(k, dim=-1).values[..., -1:])


def order_key(z32):
    """uint32 keys that order as the non-NaN fp32 values do: sign bit flipped for v >= 0, all bits for v < 0; 0 = does not count (NaN)."""
    b = np.ascontiguousarray(z32, dtype=np.float32).view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(z32), np.uint32(0), key)


def kth_largest_by_bits(z, k):
    """tau fp32 [N] of rows z fp32 [N, K] as the kernel finds it: the largest key T with at least k keys >= T, built from bit 31
    down, mapped back to its float (T = 0 -- fewer than k non-NaN entries -- maps to a NaN: nothing is below it)."""
    z32 = np.ascontiguousarray(z, dtype=np.float32)
    key = order_key(z32)
    T = np.zeros(z32.shape[0], dtype=np.uint32)
    for bit in range(31, -1, -1):
        trial = T | np.uint32(1 << bit)
        n = (key >= trial[:, None]).sum(1)
        T = np.where(n >= k, trial, T).astype(np.uint32)
    bits = np.where(T & np.uint32(0x80000000), T & np.uint32(0x7FFFFFFF), ~T).astype(np.uint32)
    return bits.view(np.float32)


def oracle_tokens(z32, k_rows, q, thr):
    """fp64 race on the truncated rows: z32 fp32 [N, K] are the temperature-scaled logits (the mask is decided on them), k_rows
    int [N], q [N, K].  Returns (token [N] -- first index on a tie, 0 for a row without a comparable ratio --, fragile [N]: the two
    largest ratios closer than ``thr`` relative to the largest, kept bool [N, K])."""
    keep = ~(z32 < _tau_rows(z32, k_rows))                     # {c : z_c >= tau}; tau = -inf where the row is not truncated
    zt = z32.masked_fill(~keep, NEG_INF)
    assert torch.equal(zt, truncate(z32, k_rows))
    r = torch.softmax(zt.double(), -1) / q.double()
    allnan = torch.isnan(r).all(-1)
    r = torch.where(torch.isnan(r), torch.full_like(r, -1.0), r)
    tok = r.argmax(-1)
    tok[allnan] = 0
    if r.shape[1] < 2:
        return tok, torch.zeros_like(tok, dtype=torch.bool), keep
    top = r.topk(2, -1).values
    fragile = ((top[:, 0] - top[:, 1]) < thr * top[:, 0]) & ~allnan & ~torch.isinf(top[:, 0])
    return tok, fragile, keep


def _tau_rows(z32, k_rows):
    K = z32.shape[-1]
    tau = torch.full((z32.shape[0], 1), NEG_INF)
    for kv in k_rows.unique().tolist():
        if 0 < kv < K:
            sel = k_rows == kv
            tau[sel] = z32[sel].topk(int(kv), dim=-1).values[:, -1:]
    return tau


def ratios_ref_f32(z32, k_rows, q):
    """ref.categorical_sample's fp32 expression on the truncated row, with the ratios kept."""
    zt = truncate(z32, k_rows)
    ln = zt - zt.logsumexp(dim=-1, keepdim=True)
    return torch.softmax(ln, dim=-1) / q


def measure_fp32_error(z32, k_rows, q):
    """Largest |r32 - r64| / max r64 over the two largest fp64 ratios of each row (tests/test_gpu_sampler_noise_shapes.py's measure)."""
    r64 = torch.softmax(truncate(z32, k_rows).double(), -1) / q.double()
    r32 = ratios_ref_f32(z32, k_rows, q)
    top = r64.topk(min(2, r64.shape[1]), -1)
    return float(((r32.double().gather(1, top.indices) - top.values).abs() / top.values[:, :1]).max())


def run(sd, B, steps, noise, top_k, K=128, mask_id=None, temp=1.0, T=16, L=7, exact_conv=False, margins=None):
    """The reference's reverse loop (oracle/snn_ref.py: ``denoiser_forward`` + the body of ``p_sample_step``) from the all-masked
    state with ``truncate`` inserted between ``logits / temp`` and ``categorical_sample``.  ``noise``: t -> (u [B,1,L,L], q [B*L*L,
    K]); ``top_k``: an int for every image.  ``margins`` (a list) receives, per step, the relative gap of the two largest fp64
    ratios at the positions that change.  Returns x_t [B,1,L,L]."""
    mask_id = K if mask_id is None else mask_id
    x_t = torch.full((B, 1, L, L), mask_id, dtype=torch.long)
    unmasked = torch.zeros((B, 1, L, L), dtype=torch.bool)
    for t in reversed(range(1, steps + 1)):
        u, q = noise(t)
        tt = torch.full((B,), t, dtype=torch.long)
        logits = ref.denoiser_forward(x_t.float(), tt, sd, T, exact_conv=exact_conv).permute(0, 2, 3, 1)     # [B,L,L,K]
        changes = (u < 1 / torch.full_like(u, float(t))) & ~unmasked
        unmasked = unmasked | changes
        z = truncate(logits / temp, int(top_k))                                                             # the one new line
        x_0_hat = ref.categorical_sample(z, q).long().unsqueeze(dim=1)
        if margins is not None:
            r = torch.softmax(z.reshape(-1, K).double(), -1) / q.double()
            top = r.topk(2, -1).values
            margins.append(((top[:, 0] - top[:, 1]) / top[:, 0])[changes.flatten()])
        x_t = x_t.clone()
        x_t[changes] = x_0_hat[changes]
    return x_t
