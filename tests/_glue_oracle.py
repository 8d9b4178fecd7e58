"""Host oracles and case tables of three kernels that sit between the models and the numbers they publish, for
tests/test_glue_oracle_host.py (CPU) and tests/test_gpu_glue_kernels.py (GPU):
  * the decoder's front end by token (csrc/conv_direct.hip: spk_spikegen_tokens_s32 = spikegen_table_kernel +
    spikegen_expand_kernel<16|32>; ops.spikegen_tokens_s32);
  * the content checksum of a tensor set (csrc/count.hip: spk_checksum_multi; ops.TensorChecksum);
  * the spike counter of the synaptic-operations report (csrc/count.hip: spk_count_spikes; ops.count_spikes).
No GPU and nothing of the library's arithmetic: fp64 matrix products of torch on the CPU, one rounding to fp32, the single-rounding
fma of tests/_conv_bn_lif_oracle.py, the reference's LIF recurrence (oracle/snn_ref.py lif_multi_step) and integer arithmetic.

The generator cases are DYADIC (codes multiples of 2^-8 in [-1, 1), weights multiples of 2^-12 in [-0.5, 0.5), biases multiples of 2^-10,
BN terms multiples of 2^-6): every product is a multiple of 2^-20 and every partial sum of a row stays far below 2^53 of them, so
the fp64 dot product is exact in any order and the contract  exact dot + bias -> ONE rounding to fp32 -> fmaf(y, a, b) -> sixteen
fp32 LIF steps from the reset state  has one answer per (code, channel), bit for bit.  The threshold case feeds the generator
pre-activations that sit exactly on, and one float below, each of the sixteen thresholds of the constant-input table
(csrc/spk_common.h), through a generator that passes code component 0 on unchanged.

The caps each "past the cap" case crosses are read from the sources (the launch lines are named where they are parsed)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import torch

import _conv_bn_lif_oracle as O
from oracle import snn_ref as ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spiking-diffusion_amd", "csrc")
T16 = 16
M64 = (1 << 64) - 1
MIX_J, MIX_W = 0x9E3779B97F4A7C15, 0xD1342543DE82EF95
CODE_BITS, WEIGHT_BITS, BIAS_BITS, BN_BITS = 8, 12, 10, 6
PRODUCT_GRID_BITS = CODE_BITS + WEIGHT_BITS                    # every term of a row's sum is a multiple of 2^-20
INT64_MIN = -(1 << 63)


def _match(src, pattern, what):
    m = re.search(pattern, open(os.path.join(CSRC, src)).read())
    assert m, f"{what} not found in {src}"
    return m


# ------------------------------------------------------------------------------------------------ the caps, from the sources
# conv_direct.hip, spk_spikegen_tokens_s32:  const dim3 g((unsigned)(blocks < 256 * 32 ? blocks : 256 * 32));  blocks of 256 threads,
# one thread per (position, step):  blocks = (n_positions * 16 + 255) / 256
_m = _match("conv_direct.hip", r"blocks\s*<\s*(\d+)\s*\*\s*(\d+)\s*\?\s*blocks\s*:\s*(\d+)\s*\*\s*(\d+)\)\);\s*\n\s*if \(Cout == 16\) "
            r"hipLaunchKernelGGL\(\(spikegen_expand_kernel<16>\)", "the expand kernel's grid cap")
assert (_m.group(1), _m.group(2)) == (_m.group(3), _m.group(4))
EXPAND_BLOCK_CAP = int(_m.group(1)) * int(_m.group(2))
EXPAND_BLOCK = int(_match("conv_direct.hip", r"n_positions\s*\*\s*16\s*\+\s*255\)\s*/\s*(\d+);", "the expand kernel's block").group(1))
EXPAND_POSITIONS_PER_PASS = EXPAND_BLOCK_CAP * EXPAND_BLOCK // T16
# count.hip, spk_checksum_multi:  dim3(128, n < 32 ? n : 32), dim3(256)
_m = _match("count.hip", r"checksum_multi_kernel,\s*dim3\((\d+),\s*n\s*<\s*(\d+)\s*\?\s*n\s*:\s*(\d+)\),\s*dim3\((\d+)\)", "the checksum's grid")
assert _m.group(2) == _m.group(3)
CHECKSUM_TENSORS_PER_PASS = int(_m.group(2))
CHECKSUM_WORDS_PER_PASS = int(_m.group(1)) * int(_m.group(4))
# count.hip, spk_count_spikes:  int blocks = spk_blocks(n_words, 256 * 8);  if (blocks > 4096) blocks = 4096;  dim3(256)
_m = _match("count.hip", r"blocks\s*=\s*spk_blocks\(n_words,\s*(\d+)\s*\*\s*(\d+)\);\s*\n\s*if \(blocks > (\d+)\) blocks = (\d+);", "the counter's grid")
assert _m.group(3) == _m.group(4)
COUNT_BLOCK, COUNT_WORDS_PER_THREAD, COUNT_BLOCK_CAP = int(_m.group(1)), int(_m.group(2)), int(_m.group(3))
COUNT_THREADS_PER_PASS = COUNT_BLOCK_CAP * COUNT_BLOCK
COUNT_WORDS_AT_CAP = COUNT_THREADS_PER_PASS * COUNT_WORDS_PER_THREAD       # more words: the grid stops growing with the tensor


# ------------------------------------------------------------------------------------------------ spike generator
def spikegen_preact(codebook, w, bias, a, b):
    """fp32 [K, Cout]: the exact fp64 dot product of every code row with every weight column, plus the bias, rounded ONCE to fp32,
    then fmaf(y, a[co], b[co]) with one rounding.  codebook [K, D], w [D, Cout], bias [Cout] or None, a / b [Cout]."""
    y64 = codebook.double() @ w.double()
    if bias is not None:
        y64 = y64 + bias.double().view(1, -1)
    return O.fma32(y64.float(), a.view(1, -1), b.view(1, -1))


def spikegen_bits(codebook, w, bias, a, b):
    """uint16 [K + 1, Cout] (numpy): bit t of entry (k, co) = the spike of step t of the default neuron, run for sixteen steps from the
    reset state on the constant input spikegen_preact(...)[k, co].  Row K (an out-of-range token) is silent.  The recurrence is
    run as it stands (ref.lif_multi_step): no threshold table."""
    z = spikegen_preact(codebook, w, bias, a, b)
    s, _ = ref.lif_multi_step(z.unsqueeze(0).expand(T16, -1, -1).contiguous(), 0.0)
    bits = np.zeros((z.shape[0] + 1, z.shape[1]), dtype=np.uint16)
    for t in range(T16):
        bits[:-1] |= (s[t].numpy() != 0).astype(np.uint16) << np.uint16(t)
    return bits


def token_rows(tokens, K):
    """The table row every token reads: its own inside [0, K), row K outside."""
    return torch.where((tokens >= 0) & (tokens < K), tokens, torch.full_like(tokens, K))


def spikegen_s32(tokens, bits, Cout):
    """tokens int64 [B, h, w] -> the S32 bytes u8 [B, 1, h, w, 16, 16] of the generator's spikes: one 16-byte record of 32 channel
    nibbles per (position, step); with 16 channels the upper 8 bytes of every record are zero.  The records of the K + 1 table
    rows come from O.bits_to_packed and every position takes its row's."""
    K = bits.shape[0] - 1
    assert Cout in (16, 32) and bits.shape[1] == Cout
    b32 = torch.zeros((K + 1, 32, 1, 1), dtype=torch.int32)
    b32[:, :Cout, 0, 0] = torch.from_numpy(bits.astype(np.int32))
    rec = O.bits_to_packed(b32, 32, T16).view(K + 1, T16, 16)           # [K+1, 1, 1, 1, 16, 16]
    B, h, w = tokens.shape
    return rec[token_rows(tokens, K).reshape(-1)].view(B, 1, h, w, T16, 16)


def gen_case(K, D, Cout, with_bias, map_shape, seed):
    """One dyadic generator case: codebook [K, D], weights [D, Cout] (the packed [1][D][Cout] form without its leading 1), bias,
    BN terms, and a token map that holds every code and the four out-of-range tokens K, -1, 2^40 and the most negative int64."""
    g = torch.Generator().manual_seed(seed)
    cb = O.dyadic((K, D), g, CODE_BITS, 1.0)
    amp = min(0.5, max(2.0 ** -6, 2.0 ** int(np.floor(np.log2(7.5 / np.sqrt(D))))))     # pre-activations spread by about one
    w = O.dyadic((D, Cout), g, WEIGHT_BITS, amp)
    bias = O.dyadic((Cout,), g, BIAS_BITS, 0.25) if with_bias else None
    a = O.dyadic((Cout,), g, BN_BITS, 2.0)
    b = O.dyadic((Cout,), g, BN_BITS, 1.0) + 0.75                       # (multiples of 2^-6 in [-0.25, 1.75): a fair share of neurons fire)
    tokens = gen_tokens(K, map_shape, g)
    return SimpleNamespace(K=K, D=D, Cout=Cout, cb=cb, w=w, bias=bias, a=a, b=b, tokens=tokens, seed=seed)


def special_tokens(K):
    return [K, -1, 1 << 40, INT64_MIN]


def gen_tokens(K, map_shape, g):
    B, h, w = map_shape
    n = B * h * w
    sp = special_tokens(K)
    assert n >= K + len(sp), "the map must hold every code and the out-of-range tokens"
    tok = torch.randint(0, K, (n,), generator=g)
    tok[:K] = torch.arange(K)
    tok[K:K + len(sp)] = torch.tensor(sp, dtype=torch.int64)
    return tok[torch.randperm(n, generator=g)].view(B, h, w).contiguous()


# (K, D, Cout, bias, token map): the rows of the GPU test, and what each is there for
GEN_ROWS = [
    (128, 16, 16, True, (3, 7, 7)),        # the models' shape
    (128, 16, 32, True, (3, 7, 7)),        # spikegen_expand_kernel<32>
    (7, 5, 16, False, (3, 5, 3)),          # D < 16 (the ci < D guards), null bias, K < 16
    (200, 24, 32, True, (5, 7, 7)),        # two chunks of sixteen components, the second ragged
    (512, 64, 32, True, (11, 7, 7)),       # four chunks
    (1, 16, 16, True, (3, 5, 3)),          # a single code
]
MODEL_ROW = GEN_ROWS[0]
LARGE_ROW = (128, 16, 32, True, (2676, 7, 7))       # 131 124 positions: just past one pass of the expand kernel's grid


def row_id(row):
    K, D, Cout, wb, shape = row
    return f"K{K}-D{D}-C{Cout}-{'bias' if wb else 'nobias'}-B{shape[0]}"


def row_seed(row):
    K, D, Cout, wb, shape = row
    return 4000 + K * 7 + D * 3 + Cout + int(wb)


def case_of(row):
    K, D, Cout, wb, shape = row
    return gen_case(K, D, Cout, wb, shape, row_seed(row))


def large_case():
    """LARGE_ROW: the (128, 16, 32, bias) parameters with a map of random codes; the out-of-range tokens sit at the first and the
    last position of the map and at the two positions either side of the end of the first pass."""
    K, D, Cout, wb, shape = LARGE_ROW
    c = gen_case(K, D, Cout, wb, GEN_ROWS[1][4], row_seed(GEN_ROWS[1]))
    g = torch.Generator().manual_seed(4999)
    n = shape[0] * shape[1] * shape[2]
    tok = torch.randint(0, K, (n,), generator=g)
    sp = special_tokens(K)
    P = EXPAND_POSITIONS_PER_PASS
    for pos, v in ((0, sp[0]), (P - 1, sp[1]), (P, sp[2]), (n - 1, sp[3])):
        tok[pos] = v
    c.tokens = tok.view(shape)
    return c


def dyadic_budget(c):
    """|sum| * 2^PRODUCT_GRID_BITS of the largest row sum a case can reach in ANY order of its terms (the sum of absolute values)."""
    s = c.cb.abs().double() @ c.w.abs().double()
    if c.bias is not None:
        s = s + c.bias.abs().double().view(1, -1)
    return float(s.max()) * 2.0 ** PRODUCT_GRID_BITS


def lif_const_thresholds():
    """The sixteen thresholds of the constant-input table, from the library's host function (no device needed)."""
    import ctypes
    from spkdiff import _lib
    th = np.zeros(16, dtype=np.float32)
    pat = np.zeros(18, dtype=np.uint32)
    assert _lib.lib.spk_lif_const_input_table(th.ctypes.data_as(ctypes.c_void_p), pat.ctypes.data_as(ctypes.c_void_p)) == 0
    return th, pat


def threshold_values(thetas):
    """The pre-activations of the threshold case: every theta_k and the float just below it, then the edges of the look-up's ranges
    and the values its arithmetic could trip on.  No infinities: the kernels' contract is finite pre-activations."""
    th = np.asarray(thetas, dtype=np.float32)
    one, two, inf = np.float32(1.0), np.float32(2.0), np.float32(np.inf)
    vals = []
    for t in th:
        vals += [t, np.nextafter(t, -inf)]
    vals += [one, np.nextafter(one, inf), two, np.nextafter(two, -inf), np.float32(0.0), np.float32(-0.0), np.float32(-3.0),
             np.finfo(np.float32).max, np.float32(1e-45), np.float32(np.nan), np.float32(-np.nan)]
    return np.array(vals, dtype=np.float32)


def threshold_case(Cout, thetas, D=16, map_shape=(3, 7, 7)):
    """A generator that hands code component 0 to every channel unchanged (weight column = the unit vector, no bias term, a = 1,
    b = 0) over a codebook whose row k holds threshold_values()[k] in component 0 and zeros elsewhere."""
    vals = threshold_values(thetas)
    K = len(vals)
    cb = torch.zeros((K, D))
    cb[:, 0] = torch.from_numpy(vals)
    w = torch.zeros((D, Cout))
    w[0, :] = 1.0
    g = torch.Generator().manual_seed(4100 + Cout)
    return SimpleNamespace(K=K, D=D, Cout=Cout, cb=cb, w=w, bias=torch.zeros(Cout), a=torch.ones(Cout), b=torch.zeros(Cout),
                           tokens=gen_tokens(K, map_shape, g), vals=vals)


def recurrence_bits(x):
    """The default neuron's fp32 recurrence on a constant input, sixteen steps from v = 0 (numpy; h = v + (x - v) / 2)."""
    x = np.asarray(x, dtype=np.float32)
    v = np.zeros_like(x)
    bits = np.zeros(x.shape, dtype=np.uint16)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T16):
            h = (v + (x - v) / np.float32(2.0)).astype(np.float32)
            s = h >= np.float32(1.0)
            bits |= s.astype(np.uint16) << np.uint16(t)
            v = np.where(s, np.float32(0.0), h)
    return bits


def table_bits(x, th, pat):
    """The device function's selection logic (csrc/spk_common.h: spk_lif_const_input_bits16) restated in numpy."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x - np.float32(1.0)
        _, e = np.frexp(t)
        k = np.clip(1 - e, 1, 16)
        p = np.where(x >= th[k - 1], k, k + 1)
        p = np.where(x >= np.float32(2.0), 1, p)
        p = np.where(x > np.float32(1.0), p, 17)
    return pat[p].astype(np.uint16)


# ------------------------------------------------------------------------------------------------ checksum
def words_of(t):
    """The little-endian 32-bit words of a tensor's elements in MEMORY order (numpy uint32): a channels-last 4-D tensor is read as
    the kernel reads it, channels innermost."""
    t = t.detach().cpu()
    if not t.is_contiguous():
        assert t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last), "dense tensors only"
        t = t.permute(0, 2, 3, 1)
    by = t.contiguous().reshape(-1).view(torch.uint8).numpy()
    assert by.size % 4 == 0
    return by.view("<u4")


def checksum_multi(arrays):
    """sum_j sum_w (word_w + 1) * ((((w + MIX_J * (j + 1)) * MIX_W) mod 2^64) | 1)  mod 2^64, as the int64 that holds those bits.
    arrays: one uint32 array of words per tensor, j = its place in the list."""
    total = 0
    for j, a in enumerate(arrays):
        a = np.asarray(a, dtype=np.uint32).reshape(-1)
        base = np.uint64((MIX_J * (j + 1)) & M64)
        with np.errstate(over="ignore"):
            m = ((np.arange(a.size, dtype=np.uint64) + base) * np.uint64(MIX_W)) | np.uint64(1)
            terms = (a.astype(np.uint64) + np.uint64(1)) * m
            total = (total + int(terms.sum(dtype=np.uint64))) & M64
    return total - (1 << 64) if total >> 63 else total


def random_words(n, g):
    """n random 32-bit words as an int32 tensor (every bit in play)."""
    return torch.randint(-(1 << 31), 1 << 31, (int(n),), generator=g).to(torch.int32)


def many_tensor_lengths(n):
    """Unequal small lengths (words) of a set of n tensors; tensors 0 and 1 are equally long (the content swap needs a pair)."""
    lens = [1 + (7 * j * j + 3 * j) % 61 for j in range(n)]
    lens[1] = lens[0] = 17
    return lens


def many_tensor_set(n, seed=5000):
    g = torch.Generator().manual_seed(seed + n)
    return [random_words(m, g) for m in many_tensor_lengths(n)]


MANY_TENSOR_COUNTS = (33, 64, 70)
LONG_WORDS = (CHECKSUM_WORDS_PER_PASS + 1, 3 * CHECKSUM_WORDS_PER_PASS + 5)


# ------------------------------------------------------------------------------------------------ spike counter
def count_spikes(words_u32, inner_words, T, kind):
    """(total, t0, ones) by the rules at the top of csrc/count.hip.  The tensor is a sequence of u32 words; word w belongs to
    time step (w // inner_words) % T.  kind 0: u8 {0, 1} bytes, a spike = bit 0 of a byte; kind 1: e2m1 nibbles, a spike = 0x2
    in a nibble; kind 2: fp32 words, nonzero = anything but +0.0 / -0.0 (NaN and denormals included), ones = words equal to 1.0f
    (0 for the other kinds)."""
    x = np.asarray(words_u32, dtype=np.uint32).reshape(-1)
    if kind == 0:
        c = sum(((x >> np.uint32(8 * i)) & np.uint32(1)).astype(np.int64) for i in range(4))
    elif kind == 1:
        c = sum(((x >> np.uint32(4 * i + 1)) & np.uint32(1)).astype(np.int64) for i in range(8))
    else:
        assert kind == 2
        c = ((x & np.uint32(0x7FFFFFFF)) != 0).astype(np.int64)
    ones = int((x == np.uint32(0x3F800000)).sum()) if kind == 2 else 0
    step = (np.arange(x.size, dtype=np.int64) // int(inner_words)) % int(T)
    return int(c.sum()), int(c[step == 0].sum()), ones


def sparse_spikes(shape, seed, density=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(tuple(shape), generator=g) < density).float()


def storage_forms(s):
    """fp32 spikes [T, B, C, H, W] (C a multiple of 64) -> the five storage forms, built on the host: name -> (tensor as the library
    tags it, inner_words, kind)."""
    T, B, C, H, W = s.shape
    bits = O.spikes_to_bits(s)
    return {
        "fp32": (s.clone(), s[0].numel(), 2),
        "ptc": (O.to_ptc(s), C // 4, 0),
        "cptc": (O.to_ptc(s, 32), 8, 0),
        "c4": (O.bits_to_packed(bits, 64, T).view(torch.int8), 8, 1),
        "s32": (O.bits_to_packed(bits, 32, T).view(torch.int8), 4, 1),
    }


# one tensor per kind with more words than COUNT_WORDS_AT_CAP; (kind, shape, T, inner_words): sparse, random, seeded
LARGE_COUNT_CASES = {
    "fp32": (2, (3, 2796211), 3, 2796211),                 # [T, N]: 8 388 633 words, an odd inner size
    "ptc": (0, (7, 1, 24967, 16, 12), 16, 3),              # PTC [B, H, W, T, C = 12]: 8 388 912 words
    "s32": (1, (3, 1, 1, 233019, 3, 16), 3, 4),            # S32 [B, 1, H, W, T = 3, 16]: 8 388 684 words
}


def large_count_words(name):
    kind, shape, T, inner = LARGE_COUNT_CASES[name]
    return int(np.prod(shape)) * (4 if kind == 2 else 1) // 4


def large_count_tensor(name):
    """The tensor of LARGE_COUNT_CASES[name] with the dtype the library tags it by (about 3 % of the channels fire)."""
    kind, shape, T, inner = LARGE_COUNT_CASES[name]
    g = torch.Generator().manual_seed(6000 + kind)
    n = int(np.prod(shape))
    r = torch.randint(0, 64, (n,), generator=g, dtype=torch.uint8)
    if kind == 2:
        return (r == 0).float().view(shape)
    if kind == 0:
        return (r < 2).to(torch.uint8).view(shape)
    lo, hi = (r == 0) | (r == 2), (r == 1) | (r == 2)
    return (lo.to(torch.uint8) * 0x02 + hi.to(torch.uint8) * 0x20).view(torch.int8).view(shape)


def placement_cases(inner_words, T, outer):
    """Word indices that hold the only spikes of a tensor of ``outer`` blocks of T steps of ``inner_words`` words: name -> (indices,
    how many of them lie in step 0).  Each set holds the very first and the very last word of its step, in the first and in the
    last outer block."""
    def step_words(t):
        idx = []
        for o in sorted({0, outer - 1}):
            base = (o * T + t) * inner_words
            idx += [base, base + inner_words - 1]
        return sorted(set(idx))
    cases = {"step0": (step_words(0), len(step_words(0)))}
    if T > 1:
        cases["step1"] = (step_words(1), 0)
        cases["last_step"] = (step_words(T - 1), 0)
    return cases
