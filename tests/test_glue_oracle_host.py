"""CPU tests of tests/_glue_oracle.py, the host side of tests/test_gpu_glue_kernels.py: the dyadic budget of every generator
case, the generator oracle against two independent formulations (torch's fp64 convolution through the Conv+BN+LIF oracle, and the
numpy restatement of the constant-input table), the checksum oracle against a literal triple loop, the spike-count oracle against
plain tensor sums, the caps every "past the cap" case claims to cross at the constants the sources have now, and the argument
errors of the three entry points that need no device."""
import ctypes

import numpy as np
import pytest
import torch

import _conv_bn_lif_oracle as O
import _glue_oracle as G

ALL_ROWS = G.GEN_ROWS + [G.LARGE_ROW]


# ------------------------------------------------------------------------------------------------ spike generator
@pytest.mark.parametrize("row", ALL_ROWS, ids=G.row_id)
def test_dyadic_budget_of_every_generator_case(row):
    """|sum| * 2^20 < 2^53 for the sum of ABSOLUTE values of every row: each fp64 partial sum is exact in any order."""
    c = G.large_case() if row is G.LARGE_ROW else G.case_of(row)
    for t, bits in ((c.cb, G.CODE_BITS), (c.w, G.WEIGHT_BITS), (c.bias, G.BIAS_BITS), (c.a, G.BN_BITS), (c.b, G.BN_BITS)):
        if t is not None:
            scaled = t.double() * 2.0 ** bits
            assert torch.equal(scaled, scaled.round()), "not on its dyadic grid"
    assert float(c.cb.abs().max()) <= 1.0 and float(c.w.abs().max()) <= 0.5
    assert G.dyadic_budget(c) < 2.0 ** 53
    # and BN's x * a + b: a product of a 24-bit and an 8-bit significand, exact in fp64 (fma32 then rounds the sum once)
    assert float(c.a.abs().max()) * 2 ** G.BN_BITS <= 2 ** 8


@pytest.mark.parametrize("row", G.GEN_ROWS, ids=G.row_id)
def test_every_generator_case_can_tell_a_wrong_kernel(row):
    """The token map holds every code and the four out-of-range tokens; the table has silent and firing entries of several
    periods, and its even and odd channels differ (a swap of the two halves of a channel pair would show)."""
    K, D, Cout, wb, shape = row
    c = G.case_of(row)
    tok = c.tokens.reshape(-1).tolist()
    assert set(range(K)) <= set(tok) and all(s in tok for s in G.special_tokens(K))
    assert c.tokens.shape == shape and (c.bias is None) == (not wb)
    bits = G.spikegen_bits(c.cb, c.w, c.bias, c.a, c.b)
    assert bits.shape == (K + 1, Cout) and bits.dtype == np.uint16 and not bits[K].any()
    assert not np.array_equal(bits[:K, 0::2], bits[:K, 1::2])
    assert (bits[:K] == 0).any() and (bits[:K] != 0).any()
    if K >= 7:
        assert len(np.unique(bits[:K])) >= 5, "too few distinct spike trains"
    if D % 16:
        # the components a chunk of sixteen reads beyond D must not matter: a codebook row of D + 1 components would differ
        assert c.cb.shape[1] == D and c.w.shape[0] == D


@pytest.mark.parametrize("row", G.GEN_ROWS, ids=G.row_id)
def test_generator_oracle_equals_the_conv_bn_lif_oracle(row):
    """torch.nn.functional.conv2d in fp64 -> fp32 -> fma32 -> lif_multi_step on a [T, K, D, 1, 1] input: the same spikes."""
    K, D, Cout, wb, shape = row
    c = G.case_of(row)
    x = c.cb.view(1, K, D, 1, 1).expand(16, -1, -1, -1, -1).contiguous()
    w4 = c.w.t().contiguous().view(Cout, D, 1, 1)
    s, _, _ = O.conv_bn_lif(x, w4, c.bias, c.a, c.b, None, (D, Cout, 1, 1, 0, False, 0, 1, 1, K))
    want = O.spikes_to_bits(s).view(K, Cout).numpy().astype(np.uint16)
    bits = G.spikegen_bits(c.cb, c.w, c.bias, c.a, c.b)
    assert np.array_equal(bits[:K], want)


def test_generator_oracle_equals_the_table_restatement_at_the_model_shape():
    th, pat = G.lif_const_thresholds()
    for row in (G.MODEL_ROW, G.GEN_ROWS[1]):
        c = G.case_of(row)
        z = G.spikegen_preact(c.cb, c.w, c.bias, c.a, c.b).numpy()
        assert np.array_equal(G.spikegen_bits(c.cb, c.w, c.bias, c.a, c.b)[:-1], G.table_bits(z, th, pat))


@pytest.mark.parametrize("Cout", [16, 32])
def test_threshold_case_is_the_fp32_recurrence_on_its_floats(Cout):
    th, pat = G.lif_const_thresholds()
    c = G.threshold_case(Cout, th)
    vals = c.vals
    assert len(vals) == 2 * 16 + 11 and not np.isinf(vals).any() and np.isnan(vals).sum() == 2
    assert np.signbit(vals[np.isnan(vals)]).tolist() == [False, True]
    z = G.spikegen_preact(c.cb, c.w, c.bias, c.a, c.b).numpy()
    # the generator hands component 0 on unchanged (fmaf(-0.0, 1, 0) is +0.0: the same neuron)
    same = (z.view(np.uint32) == vals.view(np.uint32)[:, None]) | (np.isnan(z) & np.isnan(vals)[:, None]) | ((z == 0) & (vals == 0)[:, None])
    assert same.all()
    bits = G.spikegen_bits(c.cb, c.w, c.bias, c.a, c.b)
    want = G.recurrence_bits(vals)
    assert np.array_equal(bits[:-1], np.repeat(want[:, None], Cout, axis=1))
    assert np.array_equal(want, G.table_bits(vals, th, pat))
    # theta_k is the smallest float whose first spike comes at step k or earlier: the float below fires later (or, below theta_16, never)
    first = [int(b & -b).bit_length() if b else 17 for b in want[:32].tolist()]
    assert first[0::2] == list(range(1, 17)) and first[1::2] == list(range(2, 18))
    # 1.0, the float above it, 2.0, the float below it, 0.0, -0.0, -3.0, the largest float, a denormal, NaN, -NaN
    assert want[32:].tolist() == [0, 0, 0xFFFF, 0xAAAA, 0, 0, 0, 0xFFFF, 0, 0, 0]


def test_s32_bytes_by_row_equal_the_direct_packing():
    """spikegen_s32 takes the records of the K + 1 table rows and deals them out by token; packing the per-position bits directly
    gives the same bytes.  With 16 channels the upper half of every record is zero."""
    for row in (G.GEN_ROWS[2], G.GEN_ROWS[1]):
        K, D, Cout, wb, (B, h, w) = row
        c = G.case_of(row)
        bits = G.spikegen_bits(c.cb, c.w, c.bias, c.a, c.b)
        got = G.spikegen_s32(c.tokens, bits, Cout)
        assert got.shape == (B, 1, h, w, 16, 16) and got.dtype == torch.uint8
        per_pos = torch.zeros((B, 32, h, w), dtype=torch.int32)
        per_pos[:, :Cout] = torch.from_numpy(bits.astype(np.int32))[G.token_rows(c.tokens, K)].permute(0, 3, 1, 2)
        assert torch.equal(got, O.bits_to_packed(per_pos, 32, 16))
        if Cout == 16:
            assert not got[..., 8:].any()
        sp = torch.isin(c.tokens, torch.tensor(G.special_tokens(K)))
        assert int(sp.sum()) == 4 and not got[:, 0][sp].any()
        assert int(O.packed_to_spikes(got).sum()) == int(sum(bin(int(v)).count("1") for v in bits[G.token_rows(c.tokens, K)].reshape(-1)))


# ------------------------------------------------------------------------------------------------ checksum
def test_checksum_oracle_against_a_literal_triple_loop():
    arrays = [np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32), np.array([0x80000000], dtype=np.uint32),
              np.array([7, 7, 0x12345678, 0, 0xFFFFFFFF], dtype=np.uint32)]
    total = 0
    for j, a in enumerate(arrays):
        by = a.tobytes()
        for w in range(len(by) // 4):
            word = 0
            for i in range(4):                                       # little-endian: byte i is bits 8 i .. 8 i + 7
                word += by[4 * w + i] << (8 * i)
            m = ((w + 0x9E3779B97F4A7C15 * (j + 1)) * 0xD1342543DE82EF95) % 2 ** 64
            total = (total + (word + 1) * (m | 1)) % 2 ** 64
    want = total - 2 ** 64 if total >= 2 ** 63 else total
    assert G.checksum_multi(arrays) == want
    assert -2 ** 63 <= want < 2 ** 63
    # the sum does not depend on the order its terms are added in: each word keeps its own index w, the terms are permuted
    terms = [((j, w, int(x))) for j, a in enumerate(arrays) for w, x in enumerate(a)]
    rng = np.random.default_rng(1)
    for _ in range(3):
        acc = 0
        for i in rng.permutation(len(terms)):
            j, w, x = terms[i]
            acc = (acc + (x + 1) * ((((w + G.MIX_J * (j + 1)) * G.MIX_W) & G.M64) | 1)) & G.M64
        assert acc == total
    # ... but on which tensor a word belongs to, and where in it
    assert G.checksum_multi([arrays[1], arrays[0], arrays[2]]) != want
    assert G.checksum_multi([arrays[0][::-1].copy(), arrays[1], arrays[2]]) != want
    assert G.checksum_multi([arrays[0]]) != G.checksum_multi([np.zeros(0, np.uint32), arrays[0]])
    # a zero word still counts (word + 1), so a longer tensor of zeros differs
    assert G.checksum_multi([np.zeros(3, np.uint32)]) != G.checksum_multi([np.zeros(4, np.uint32)])


def test_words_of_reads_memory_order():
    t = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).view(2, 3, 2, 2)
    cl = t.contiguous(memory_format=torch.channels_last)
    assert np.array_equal(G.words_of(t).view(np.float32), t.reshape(-1).numpy())
    assert np.array_equal(G.words_of(cl).view(np.float32), t.permute(0, 2, 3, 1).reshape(-1).numpy())
    assert G.words_of(torch.tensor([1, -1], dtype=torch.int64)).tolist() == [1, 0, 0xFFFFFFFF, 0xFFFFFFFF]
    assert G.words_of(torch.tensor([1, 2, 3, 4, 5, 6, 7, 8], dtype=torch.uint8)).tolist() == [0x04030201, 0x08070605]
    assert G.words_of(torch.tensor([1.0, -2.0], dtype=torch.bfloat16)).tolist() == [0xC0003F80]


def test_checksum_cases_cross_the_caps_they_claim():
    # count.hip, spk_checksum_multi: hipLaunchKernelGGL(checksum_multi_kernel, dim3(128, n < 32 ? n : 32), dim3(256), ...)
    assert G.CHECKSUM_TENSORS_PER_PASS == 32 and G.CHECKSUM_WORDS_PER_PASS == 32768
    assert min(G.MANY_TENSOR_COUNTS) == G.CHECKSUM_TENSORS_PER_PASS + 1               # the `j += gridDim.y` loop's second trip
    assert 2 * G.CHECKSUM_TENSORS_PER_PASS in G.MANY_TENSOR_COUNTS                    # ... a full second trip
    assert max(G.MANY_TENSOR_COUNTS) > 2 * G.CHECKSUM_TENSORS_PER_PASS                # ... and a ragged third
    assert G.LONG_WORDS[0] == G.CHECKSUM_WORDS_PER_PASS + 1                           # one word into the second pass of the word loop
    assert 3 * G.CHECKSUM_WORDS_PER_PASS < G.LONG_WORDS[1] < 4 * G.CHECKSUM_WORDS_PER_PASS
    for n in G.MANY_TENSOR_COUNTS:
        lens = G.many_tensor_lengths(n)
        assert lens[0] == lens[1] and len(set(lens)) > 20 and min(lens) >= 1
        ts = G.many_tensor_set(n)
        assert [t.numel() for t in ts] == lens and not torch.equal(ts[0], ts[1])


# ------------------------------------------------------------------------------------------------ spike counter
@pytest.mark.parametrize("T", [1, 3, 16])
def test_count_oracle_equals_plain_sums_on_every_storage_form(T):
    s = G.sparse_spikes((T, 2, 64, 3, 5), 70 + T)
    total, t0 = int(s.sum()), int(s[0].sum())
    assert 0 < t0 and (T == 1 or t0 < total)
    for name, (t, inner, kind) in G.storage_forms(s).items():
        got = G.count_spikes(G.words_of(t), inner, T, kind)
        assert got == (total, t0, total if kind == 2 else 0), name


def test_count_oracle_value_classes_and_placement():
    f = np.array([0.0, 1.0, -0.0, 0.5, 2.0, -1.0, np.nan, 1e-45, 1.0], dtype=np.float32)
    assert G.count_spikes(f.view(np.uint32), 3, 3, 2) == (7, 1, 2)                    # -0.0 is no spike; step 0 = words 0..2
    for inner, T, outer in ((70, 3, 1), (3, 16, 5), (4, 1, 3)):
        n = inner * T * outer
        for name, (idx, n0) in G.placement_cases(inner, T, outer).items():
            assert len(idx) == len(set(idx)) and 0 <= min(idx) and max(idx) < n
            steps = {(i // inner) % T for i in idx}
            assert steps == {{"step0": 0, "step1": 1, "last_step": T - 1}[name]}
            w = np.zeros(n, dtype=np.uint32)
            w[idx] = 0x01010101
            assert G.count_spikes(w, inner, T, 0) == (4 * len(idx), 4 * n0, 0)
    assert G.placement_cases(3, 16, 5)["step0"][0] == [0, 2, 192, 194]
    assert G.placement_cases(3, 16, 5)["last_step"][0] == [45, 47, 237, 239]


def test_large_count_cases_cross_the_block_cap():
    # count.hip, spk_count_spikes: int blocks = spk_blocks(n_words, 256 * 8); if (blocks > 4096) blocks = 4096;  blocks of 256 threads
    assert G.COUNT_BLOCK_CAP == 4096 and G.COUNT_BLOCK == 256 and G.COUNT_WORDS_PER_THREAD == 8
    assert G.COUNT_THREADS_PER_PASS == 1048576 and G.COUNT_WORDS_AT_CAP == 8388608
    for name, (kind, shape, T, inner) in G.LARGE_COUNT_CASES.items():
        n = G.large_count_words(name)
        assert n > G.COUNT_WORDS_AT_CAP, name                       # spk_blocks asks for more than 4096 blocks
        assert n > 8 * G.COUNT_THREADS_PER_PASS, name               # every thread makes more than eight passes, the last ragged
        assert n % G.COUNT_THREADS_PER_PASS != 0 and n < 2 ** 31 // 4 * 4
        assert n % (inner * T) == 0 and n // (inner * T) == (1 if kind == 2 else n // (inner * T))
        assert name == "s32" or inner & (inner - 1) != 0            # (an S32 record is four words whatever the shape)
        assert n * 4 < 36 * 2 ** 20


def test_large_generator_row_crosses_the_expand_grid_cap():
    # conv_direct.hip, spk_spikegen_tokens_s32: const dim3 g((unsigned)(blocks < 256 * 32 ? blocks : 256 * 32)), blocks of 256 threads,
    # one thread per (position, step)
    assert G.EXPAND_BLOCK_CAP == 8192 and G.EXPAND_BLOCK == 256 and G.EXPAND_POSITIONS_PER_PASS == 131072
    K, D, Cout, wb, (B, h, w) = G.LARGE_ROW
    n = B * h * w
    assert G.EXPAND_POSITIONS_PER_PASS < n == 131124 < G.EXPAND_POSITIONS_PER_PASS + 256
    assert all(Bs * hs * ws <= G.EXPAND_POSITIONS_PER_PASS for _, _, _, _, (Bs, hs, ws) in G.GEN_ROWS)
    c = G.large_case()
    flat = c.tokens.reshape(-1)
    P = G.EXPAND_POSITIONS_PER_PASS
    assert [int(flat[i]) for i in (0, P - 1, P, n - 1)] == G.special_tokens(K)
    small = G.case_of(G.GEN_ROWS[1])
    assert all(torch.equal(getattr(c, k), getattr(small, k)) for k in ("cb", "w", "bias", "a", "b"))


# ------------------------------------------------------------------------------------------------ argument errors, no device
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_checksum_and_counter_argument_errors():
    from spkdiff import _lib, ops
    lib, ERR_ARG = _lib.lib, _lib.CONSTANTS["SPK_ERR_ARG"]
    with pytest.raises(ValueError):
        ops.TensorChecksum([])
    with pytest.raises(ValueError):
        ops.TensorChecksum([None, torch.zeros(4)])                   # (host tensors are not covered: nothing is left)
    buf = np.zeros(8, dtype=np.uint64)
    assert lib.spk_checksum_multi(None, 1, _ptr(buf), None) == ERR_ARG
    assert lib.spk_checksum_multi(_ptr(buf), 1, None, None) == ERR_ARG
    assert lib.spk_checksum_multi(_ptr(buf), 0, _ptr(buf), None) == ERR_ARG
    assert lib.spk_checksum_multi(_ptr(buf), -3, _ptr(buf), None) == ERR_ARG
    assert lib.spk_count_spikes(None, 4, 1, 1, 0, _ptr(buf), None) == ERR_ARG
    assert lib.spk_count_spikes(_ptr(buf), 4, 1, 1, 0, None, None) == ERR_ARG
    for n, inner, T, kind in ((0, 1, 1, 0), (-4, 1, 1, 0), (4, 0, 1, 0), (4, 1, 0, 0), (4, 1, 1, -1), (4, 1, 1, 3)):
        assert lib.spk_count_spikes(_ptr(buf), n, inner, T, kind, _ptr(buf), None) == ERR_ARG
    with pytest.raises(RuntimeError):
        ops.count_spikes(torch.zeros(3, 4))


def test_spikegen_argument_errors_and_table_size():
    from spkdiff import _lib
    lib, C = _lib.lib, _lib.CONSTANTS
    for K, Cout in ((128, 16), (128, 32), (1, 16), (7, 16), (512, 32)):
        assert lib.spk_spikegen_table_bytes(K, Cout) == (K + 1) * Cout * 2
    for K, Cout in ((0, 16), (-1, 32), (128, 8), (128, 24), (128, 64), (128, 0)):
        assert lib.spk_spikegen_table_bytes(K, Cout) == -1
    b = np.zeros(64, dtype=np.uint64)
    p = _ptr(b)

    def call(tokens=p, cb=p, w=p, bias=p, a=p, bb=p, ws=p, out=p, T=16, n=1, K=1, D=1, Cout=16):
        return lib.spk_spikegen_tokens_s32(tokens, cb, w, bias, a, bb, ws, 1, out, T, n, K, D, Cout, None)

    for name in ("tokens", "cb", "w", "a", "bb", "ws", "out"):
        assert call(**{name: None}) == C["SPK_ERR_ARG"], name
    assert call(n=0) == call(n=-5) == call(K=0) == call(D=0) == call(D=-1) == C["SPK_ERR_ARG"]
    for T in (1, 4, 15, 17, 32):
        assert call(T=T) == C["SPK_ERR_UNSUPPORTED"]
    for Cout in (0, 8, 15, 17, 24, 48, 64):
        assert call(Cout=Cout) == C["SPK_ERR_UNSUPPORTED"]
