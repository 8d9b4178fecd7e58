"""Host restatement of the sampler's counter-based noise (test infrastructure only; the product never imports it).

Written from the public definition of Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
1, 2, 3", SC'11, and the Random123 library's philox.h), not from the device code, and pinned to the library's published
known answers by tests/test_oracle_philox.py.

One round of Philox4x32 maps the counter (c0, c1, c2, c3) under the round key (k0, k1) to

    (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0))

with M0 = 0xD2511F53, M1 = 0xCD9E8D57 and hi / lo the halves of the 64-bit product; ten rounds, the key bumped by the Weyl
constants (0x9E3779B9, 0xBB67AE85) between rounds.

The noise contract of one reverse step (include/spkdiff.h, spk_psample_step), B images x HW positions x K classes,
64-bit key ``seed`` and 64-bit counter ``offset``:

    position p (image-major) tests   u_p   = (r0 >> 8) * 2^-24           r = philox(counter offset + p*K,     stream 0)
    and races                        q_p,k = -log(((r0 >> 8) + 1) * 2^-24)  r = philox(counter offset + p*K + k, stream 1)

    counter words (index lo32, index hi32, stream, 0), key words (seed lo32, seed hi32); only output word 0 is used.

``state = (seed', base)`` is the 2-word device buffer of a captured graph: seed' REPLACES the seed and base is ADDED to the
offset, everything modulo 2^64.

u lies in [0, 1) and carries the 24 mantissa bits exactly.  q lies in [0, 24 ln 2 = 16.64]: q = 0 is reachable (mantissa all
ones, 2^-24 per draw).  The sampler's race is argmax_k softmax_k / q_k.  In the kernels a class with q = 0 and a positive
(not underflowed) probability has ratio +inf and wins (the lowest such class on a tie), which is also what torch.argmax does
with the reference expression; a class with q = 0 whose probability underflowed to 0 has ratio 0/0 = NaN, which the kernels'
`ratio > best` never selects (torch.argmax would select it).  If every ratio of a position is NaN (a NaN logit, or all
logits -inf) the kernels write token 0, which is torch.argmax's answer for an all-NaN row.
"""
from typing import NamedTuple

import numpy as np

M0 = np.uint64(0xD2511F53)
M1 = np.uint64(0xCD9E8D57)
W0 = 0x9E3779B9
W1 = 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
MASK64 = (1 << 64) - 1
S32 = np.uint64(32)


def philox4x32_10(counter4, key2):
    """Philox4x32-10.  counter4: integer array [..., 4] of 32-bit words, key2: 2 words (or [..., 2], broadcast against the
    counters) -> uint32 array [..., 4]."""
    c = np.asarray(counter4, dtype=np.uint64) & MASK32
    k = np.asarray(key2, dtype=np.uint64) & MASK32
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & MASK32
            k1 = (k1 + np.uint64(W1)) & MASK32
        p0 = M0 * c0                      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK32, (p0 >> S32) ^ c3 ^ k1, p0 & MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _word0(seed, index, stream):
    """Output word 0 at the 64-bit counters ``index`` (uint64 array) of one stream under the 64-bit key ``seed``."""
    index = np.asarray(index, dtype=np.uint64)
    ctr = np.stack([index & MASK32, index >> S32, np.full_like(index, stream), np.zeros_like(index)], axis=-1)
    seed = int(seed) & MASK64
    return philox4x32_10(ctr, [seed & 0xFFFFFFFF, seed >> 32])[..., 0]


def q_of_mantissa(n_q):
    """fp64 exponential variate of a 24-bit mantissa: -log((n + 1) * 2^-24)."""
    return -np.log((np.asarray(n_q, dtype=np.float64) + 1.0) * 2.0 ** -24)


class StepNoise(NamedTuple):
    u: np.ndarray        # fp32 [B*HW], exact
    q: np.ndarray        # fp32 [B*HW, K]: q64 rounded once (None when want_q is False)
    n_u: np.ndarray      # uint32 [B*HW] 24-bit mantissas
    n_q: np.ndarray      # uint32 [B*HW, K]
    q64: np.ndarray      # fp64 [B*HW, K]


def step_noise(seed, offset, B, HW, K, state=None, want_q=True, chunk=1 << 20):
    """The (u, q) of one Philox-mode reverse step; see the module docstring for the contract."""
    seed, offset = int(seed) & MASK64, int(offset) & MASK64
    if state is not None:
        seed = int(state[0]) & MASK64
        offset = (offset + int(state[1])) & MASK64
    npos = int(B) * int(HW)
    K = int(K)
    with np.errstate(over="ignore"):                                      # counters wrap modulo 2^64 by definition
        pos = np.arange(npos, dtype=np.uint64) * np.uint64(K) + np.uint64(offset)
        n_u = _word0(seed, pos, 0) >> np.uint32(8)
        u = (n_u.astype(np.float64) * 2.0 ** -24).astype(np.float32)
        if not want_q:
            return StepNoise(u, None, n_u, None, None)
        n_q = np.empty(npos * K, dtype=np.uint32)
        for a in range(0, npos * K, chunk):
            b = min(npos * K, a + chunk)
            n_q[a:b] = _word0(seed, np.arange(a, b, dtype=np.uint64) + np.uint64(offset), 1) >> np.uint32(8)
    n_q = n_q.reshape(npos, K)
    q64 = q_of_mantissa(n_q)
    return StepNoise(u, q64.astype(np.float32), n_u, n_q, q64)
