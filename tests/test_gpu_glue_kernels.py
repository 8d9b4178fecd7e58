"""GPU tests of three kernels that were reached only through whole models, each against the host oracles of tests/_glue_oracle.py
(tests/test_glue_oracle_host.py checks those, and the caps named below, without a GPU):
  (a) the decoder's front end by token (csrc/conv_direct.hip: spk_spikegen_tokens_s32 = spikegen_table_kernel +
      spikegen_expand_kernel<16|32>) through ops.spikegen_tokens_s32: both channel counts, D below and across the chunk of sixteen
      components, no bias, K from 1 to 512, out-of-range tokens, a token map past one pass of the expand kernel's grid,
      pre-activations exactly on every threshold of the constant-input table, the build_table flag and the wrapper's slot logic;
  (b) the content checksum of a tensor set (csrc/count.hip: spk_checksum_multi) through ops.TensorChecksum: the value itself, more
      than 32 tensors, tensors longer than one pass, every kind of tensor the selection keeps, single-bit and swap sensitivity;
  (c) the spike counter (csrc/count.hip: spk_count_spikes) through ops.count_spikes and the C-ABI: all five storage forms at
      T = 1, 3, 16, inner sizes that are no power of two, tensors past the block cap, spikes placed in one step only, the fp32
      value classes.
Every comparison is exact: bytes with torch.equal, integers with ==.  Outputs are allocated over blocks filled with 0xFF, so a
byte a kernel fails to write is not a valid record."""
import numpy as np
import pytest
import torch

import _glue_oracle as G
from parity_report import record as parity
from spkdiff import ops

pytestmark = pytest.mark.gpu

TALLY = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


def tally(name, **counts):
    """Accumulate the counts of one family over its cases and keep its PARITY_REPORT line current."""
    t = TALLY.setdefault(name, {})
    for k, v in counts.items():
        t[k] = t.get(k, 0) + int(v)
    parity("glue_" + name, **t)


def poison(dev, nbytes):
    """Leave a block of 0xFF bytes in the caching allocator: the next allocation of that size starts from it."""
    buf = torch.full((int(nbytes),), -1, dtype=torch.int8, device=dev)
    del buf


# =============================================================================================== (a) spike generator
def gen_args(c, dev):
    """The device tensors of a generator case: (tokens, codebook, packed weights [1][D][Cout], bias or None, a, b)."""
    return (c.tokens.to(dev), c.cb.to(dev), c.w.view(1, c.D, c.Cout).contiguous().to(dev), None if c.bias is None else c.bias.to(dev),
            c.a.to(dev), c.b.to(dev))


def run_generator(c, dev, **kw):
    """ops.spikegen_tokens_s32 on a case against the oracle's bytes: (bytes compared, bytes that differ)."""
    want = G.spikegen_s32(c.tokens, G.spikegen_bits(c.cb, c.w, c.bias, c.a, c.b), c.Cout)
    poison(dev, want.numel())
    out = ops.spikegen_tokens_s32(*gen_args(c, dev), **kw)
    B, h, w = c.tokens.shape
    assert out.dtype == torch.int8 and tuple(out.shape) == (B, 1, h, w, 16, 16) and out.is_contiguous()
    got = out.cpu().view(torch.uint8)
    return want.numel(), int((got != want).sum()), got, want


@pytest.mark.parametrize("row", G.GEN_ROWS, ids=G.row_id)
def test_spike_generator_rows(dev, row):
    """Every code, K, -1, 2^40 and the most negative int64 on a small map; the whole output against the oracle's bytes."""
    c = G.case_of(row)
    n, bad, got, want = run_generator(c, dev, table_slot=None)
    tally("spikegen_rows", bytes=n, mismatches=bad)
    assert torch.equal(got, want)


def test_spike_generator_past_one_pass_of_the_expand_grid(dev):
    """131 124 positions against 256 * 32 blocks of 256 threads, one thread per (position, step): 52 positions in the second pass."""
    c = G.large_case()
    assert c.tokens.numel() > G.EXPAND_POSITIONS_PER_PASS
    n, bad, got, want = run_generator(c, dev, table_slot=None)
    tally("spikegen_second_pass", bytes=n, mismatches=bad)
    assert torch.equal(got, want)


@pytest.mark.parametrize("Cout", [16, 32])
def test_spike_generator_on_the_thresholds_of_the_constant_input_table(dev, Cout):
    """Pre-activations exactly theta_k and the float below, for all sixteen thresholds, and 1.0, 1.0+, 2.0, 2.0-, 0.0, -0.0, -3.0,
    FLT_MAX, a denormal and both NaNs, through a generator that hands them on unchanged: the fp32 recurrence decides."""
    th, _ = G.lif_const_thresholds()
    c = G.threshold_case(Cout, th)
    assert np.array_equal(G.spikegen_bits(c.cb, c.w, c.bias, c.a, c.b)[:-1, 0], G.recurrence_bits(c.vals))
    n, bad, got, want = run_generator(c, dev, table_slot=None)
    tally("spikegen_thresholds", bytes=n, mismatches=bad)
    assert torch.equal(got, want)


def test_spike_generator_build_table_flag_through_the_c_abi(dev):
    """build_table = 0 reads the table the workspace holds (the codebook buffer may have changed since); 1 rebuilds it."""
    row = G.GEN_ROWS[3]
    c1 = G.case_of(row)
    c2 = G.gen_case(c1.K, c1.D, c1.Cout, True, row[4], G.row_seed(row) + 1)
    bits1 = G.spikegen_bits(c1.cb, c1.w, c1.bias, c1.a, c1.b)
    bits2 = G.spikegen_bits(c2.cb, c1.w, c1.bias, c1.a, c1.b)               # the second codebook under the first generator
    want1, want2 = G.spikegen_s32(c1.tokens, bits1, c1.Cout), G.spikegen_s32(c1.tokens, bits2, c1.Cout)
    assert not torch.equal(want1, want2)
    tokens, cb, wp, bias, a, b = gen_args(c1, dev)
    nbytes = ops.lib.spk_spikegen_table_bytes(c1.K, c1.Cout)
    assert nbytes == (c1.K + 1) * c1.Cout * 2
    ws = torch.full((nbytes // 2,), -1, dtype=torch.int16, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(build):
        out = torch.full(tuple(want1.shape), -1, dtype=torch.int8, device=dev)
        rc = ops.lib.spk_spikegen_tokens_s32(tokens.data_ptr(), cb.data_ptr(), wp.data_ptr(), bias.data_ptr(), a.data_ptr(), b.data_ptr(),
                                             ws.data_ptr(), build, out.data_ptr(), 16, tokens.numel(), c1.K, c1.D, c1.Cout, stream)
        assert rc == 0
        return out.cpu().view(torch.uint8)

    first = call(1)
    table = ws.cpu().numpy().view(np.uint16).reshape(c1.K + 1, c1.Cout)
    cb.copy_(c2.cb.to(dev))
    kept = call(0)
    rebuilt = call(1)
    bad = int((first != want1).sum()) + int((kept != want1).sum()) + int((rebuilt != want2).sum())
    bad += int((table != bits1).sum())
    tally("spikegen_build_flag", bytes=3 * want1.numel() + 2 * table.size, mismatches=bad)
    assert np.array_equal(table, bits1), "the table workspace is [K + 1][Cout] u16 patterns, bit t = step t"
    assert torch.equal(first, want1) and torch.equal(kept, want1) and torch.equal(rebuilt, want2)


def test_spike_generator_wrapper_slot_logic(dev):
    """ops.spikegen_tokens_s32 builds the table when it must and only then: same key and stream -> once; a changed key, no key or
    another stream -> again; two slots (two models) never share a buffer.  Every call's output is the oracle's."""
    c = G.case_of(G.MODEL_ROW)
    want = G.spikegen_s32(c.tokens, G.spikegen_bits(c.cb, c.w, c.bias, c.a, c.b), c.Cout)
    args = gen_args(c, dev)
    seen = []
    orig = ops.lib.spk_spikegen_tokens_s32

    def spy(tokens, cb, wp, bias, a, b, ws, build, *rest):
        seen.append((int(build), int(ws)))
        return orig(tokens, cb, wp, bias, a, b, ws, build, *rest)

    bad = calls = 0

    def run(**kw):
        nonlocal bad, calls
        got = ops.spikegen_tokens_s32(*args, **kw).cpu().view(torch.uint8)
        bad += int((got != want).sum())
        calls += 1
        return seen[-1]

    slot_a, slot_b = {}, {}
    ops.lib.spk_spikegen_tokens_s32 = spy
    try:
        b1, ws_a = run(table_key="k1", table_slot=slot_a)
        assert b1 == 1
        assert run(table_key="k1", table_slot=slot_a) == (0, ws_a)              # same key, same stream
        assert run(table_key="k2", table_slot=slot_a) == (1, ws_a)              # changed key
        assert run(table_key="k2", table_slot=slot_a) == (0, ws_a)
        assert run(table_key=None, table_slot=slot_a) == (1, ws_a)              # no key: always
        assert run(table_key=None, table_slot=slot_a) == (1, ws_a)
        assert run(table_key="k2", table_slot=slot_a) == (1, ws_a)              # (a keyless call leaves no key behind)
        assert run(table_key="k2", table_slot=slot_a) == (0, ws_a)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            assert run(table_key="k2", table_slot=slot_a) == (1, ws_a)          # another stream
            assert run(table_key="k2", table_slot=slot_a) == (0, ws_a)
        torch.cuda.current_stream(dev).wait_stream(side)
        assert run(table_key="k2", table_slot=slot_a) == (1, ws_a)              # ... and back
        b2, ws_b = run(table_key="k2", table_slot=slot_b)                       # a second slot: its own buffer, its own first build
        assert b2 == 1 and ws_b != ws_a
        assert run(table_key="k2", table_slot=slot_a) == (0, ws_a) and run(table_key="k2", table_slot=slot_b) == (0, ws_b)
        b3, ws_c = run(table_key="k2", table_slot=None)                         # no slot: a buffer of the call's own, always built
        assert b3 == 1 and ws_c not in (ws_a, ws_b)
    finally:
        ops.lib.spk_spikegen_tokens_s32 = orig
    assert len(slot_a) == len(slot_b) == 1 and len(seen) == calls
    tally("spikegen_slots", bytes=calls * want.numel(), mismatches=bad)
    assert bad == 0


# =============================================================================================== (b) checksum
def check_value(name, kept, tensors=None):
    """TensorChecksum(tensors).value() against the oracle on the host copies of ``kept`` (the tensors the selection keeps, in order)."""
    cs = ops.TensorChecksum(kept if tensors is None else tensors)
    assert cs.n == len(kept)
    got, want = cs.value(), G.checksum_multi([G.words_of(t) for t in kept])
    tally(name, values=1, mismatches=got != want)
    assert got == want, (name, got, want)
    return cs, got


def test_checksum_of_one_word(dev):
    for word in (0, 1, -1, 0x12345678):
        check_value("checksum_small", [torch.tensor([word], dtype=torch.int32, device=dev)])


def test_checksum_of_a_mixed_set(dev):
    """fp32, int64, eight uint8 bytes, bf16 with an even count and a channels-last 4-D fp32 are covered (as their words in memory
    order); a non-dense view and an empty tensor sit in the list and are skipped, so the tensors after them move up."""
    g = torch.Generator().manual_seed(5100)
    f32 = torch.randn(5, 7, generator=g).to(dev)
    i64 = torch.randint(-(1 << 62), 1 << 62, (3,), generator=g).to(dev)
    u8 = torch.randint(0, 256, (8,), generator=g, dtype=torch.uint8).to(dev)
    bf = torch.randn(3, 6, generator=g).to(torch.bfloat16).to(dev)
    cl = torch.randn(2, 3, 4, 5, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    view = torch.randn(6, 6, generator=g).to(dev)[:, ::2]
    empty = torch.zeros(0, device=dev)
    assert not view.is_contiguous() and not cl.is_contiguous()
    tensors = [f32, view, i64, empty, u8, None, bf, cl]
    kept = [f32, i64, u8, bf, cl]
    assert [t.data_ptr() for t in ops.TensorChecksum.select(tensors)] == [t.data_ptr() for t in kept]
    _, v = check_value("checksum_small", kept, tensors)
    # the channels-last tensor is read in memory order: the same values laid out contiguously give another value
    assert check_value("checksum_small", [f32, i64, u8, bf, cl.contiguous()])[1] != v
    with pytest.raises(NotImplementedError):
        ops.TensorChecksum([f32, torch.zeros(3, dtype=torch.uint8, device=dev)])


@pytest.mark.parametrize("n", G.MANY_TENSOR_COUNTS)
def test_checksum_of_more_tensors_than_one_pass(dev, n):
    assert n > G.CHECKSUM_TENSORS_PER_PASS
    check_value("checksum_many_tensors", [t.to(dev) for t in G.many_tensor_set(n)])


@pytest.mark.parametrize("n_words", G.LONG_WORDS)
def test_checksum_of_a_tensor_longer_than_one_pass(dev, n_words):
    assert n_words > G.CHECKSUM_WORDS_PER_PASS
    g = torch.Generator().manual_seed(5200 + n_words)
    check_value("checksum_long_tensor", [G.random_words(n_words, g).to(dev)])
    check_value("checksum_long_tensor", [G.random_words(3, g).to(dev), G.random_words(n_words, g).to(dev), G.random_words(5, g).to(dev)])


def test_checksum_of_the_denoisers_parameters_and_buffers(dev):
    from snn_model.vae_model import functional
    from snn_model.vq_diffusion import DummyModel
    from spkdiff import synth
    den = DummyModel(1, 128).to(dev)
    functional.set_step_mode(net=den, step_mode='m')
    den.load_state_dict(synth.synth_denoiser_state(synth.MNIST))
    ts = list(den.parameters()) + list(den.buffers())
    kept = ops.TensorChecksum.select(ts)
    assert len(kept) > G.CHECKSUM_TENSORS_PER_PASS and len(kept) == len([t for t in ts if t.numel()])
    assert max(t.numel() for t in kept) > G.CHECKSUM_WORDS_PER_PASS
    cs, v = check_value("checksum_denoiser", kept, ts)
    # one .data write to the last tensor's last element is noticed, and the value is the oracle's again
    last = kept[-1]
    last.data.view(-1)[-1] += 1
    v2, want2 = cs.value(), G.checksum_multi([G.words_of(t) for t in kept])
    tally("checksum_denoiser", values=1, mismatches=v2 != want2)
    assert v2 != v and v2 == want2


def flip(t, word, bit):
    t.view(-1)[word] ^= torch.tensor(-(1 << 31) if bit == 31 else 1 << bit, dtype=torch.int32)


def test_checksum_notices_every_single_bit(dev):
    """Bit 0 and bit 31 of a word in tensors 0, 31, 32 and the last of the 70-tensor set, and of words 0, 32 767, 32 768 and the
    last of the long tensor: each flip gives the oracle's value for the new content, and another value than before."""
    n = max(G.MANY_TENSOR_COUNTS)
    host = G.many_tensor_set(n)
    g = torch.Generator().manual_seed(5300)
    host.append(G.random_words(G.LONG_WORDS[1], g))
    ts = [t.to(dev) for t in host]
    cs, v = check_value("checksum_sensitivity", ts)
    P = G.CHECKSUM_WORDS_PER_PASS
    spots = [(j, host[j].numel() // 2) for j in (0, G.CHECKSUM_TENSORS_PER_PASS - 1, G.CHECKSUM_TENSORS_PER_PASS, n - 1)]
    spots += [(n, w) for w in (0, P - 1, P, G.LONG_WORDS[1] - 1)]
    seen = {v}
    for j, w in spots:
        for bit in (0, 31):
            flip(ts[j], w, bit)
            flip(host[j], w, bit)
            got, want = cs.value(), G.checksum_multi([G.words_of(t) for t in host])
            tally("checksum_sensitivity", values=1, mismatches=got != want)
            assert got == want, (j, w, bit)
            assert got not in seen, (j, w, bit)
            seen.add(got)
    assert torch.equal(ts[n].cpu(), host[n])


def test_checksum_notices_swaps_and_repeats_itself(dev):
    host = G.many_tensor_set(max(G.MANY_TENSOR_COUNTS))
    ts = [t.to(dev) for t in host]
    cs, v = check_value("checksum_sensitivity", ts)
    assert [cs.value() for _ in range(3)] == [v, v, v]              # (the memset per call; atomics landing in any order)
    # the contents of two equally long tensors change places (0 and 1); then the words tensor 32 has with the same words of
    # tensor 0, which the same row of the grid reads
    for i, k in ((0, 1), (0, G.CHECKSUM_TENSORS_PER_PASS)):
        m = min(host[i].numel(), host[k].numel())
        a, b = host[i][:m].clone(), host[k][:m].clone()
        assert not torch.equal(a, b)
        host[i][:m], host[k][:m] = b, a
        ts[i].copy_(host[i])
        ts[k].copy_(host[k])
        got, want = cs.value(), G.checksum_multi([G.words_of(t) for t in host])
        tally("checksum_sensitivity", values=1, mismatches=got != want)
        assert got == want and got != v
        v = got
    # two unequal words of one tensor change places
    t = host[5]
    assert t.numel() >= 2 and int(t[0]) != int(t[-1])
    t[0], t[-1] = int(t[-1]), int(t[0])
    ts[5].copy_(t)
    got, want = cs.value(), G.checksum_multi([G.words_of(t) for t in host])
    tally("checksum_sensitivity", values=1, mismatches=got != want)
    assert got == want and got != v
    assert [cs.value() for _ in range(3)] == [got, got, got]


# =============================================================================================== (c) spike counter
def counted(t):
    r = ops.count_spikes(t)
    return r["total"], r["t0"], r["numel"], r["numel_t0"], r["binary"]


def raw_count(words, inner, T, kind, dev):
    """spk_count_spikes on a raw word buffer: (total, t0, ones)."""
    d = torch.from_numpy(words.view(np.int32)).to(dev)
    out = torch.full((3,), -1, dtype=torch.int64, device=dev)
    rc = ops.lib.spk_count_spikes(d.data_ptr(), d.numel(), inner, T, kind, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    return tuple(int(v) for v in out.tolist())


@pytest.mark.parametrize("T", [1, 3, 16])
def test_count_spikes_of_every_storage_form(dev, T):
    s = G.sparse_spikes((T, 2, 64, 3, 5), 70 + T)
    total, t0 = int(s.sum()), int(s[0].sum())
    for name, (t, inner, kind) in G.storage_forms(s).items():
        assert G.count_spikes(G.words_of(t), inner, T, kind)[:2] == (total, t0)
        got = counted(t.to(dev))
        tally("count_forms", values=2, mismatches=(got[0] != total) + (got[1] != t0))
        assert got == (total, t0, s.numel(), s[0].numel(), True), (name, got)


def test_count_spikes_with_inner_sizes_that_are_no_power_of_two(dev):
    s = G.sparse_spikes((3, 2, 5, 7), 81, 0.2)                      # fp32 [T, ...]: 70 words per step
    got = counted(s.to(dev))
    want = (int(s.sum()), int(s[0].sum()), s.numel(), s[0].numel(), True)
    tally("count_forms", values=2, mismatches=(got[0] != want[0]) + (got[1] != want[1]))
    assert got == want
    for T in (1, 3, 16):
        p = G.sparse_spikes((T, 3, 12, 3, 5), 82 + T, 0.2)          # PTC with C = 12: three words per (position, step)
        ptc = p.permute(1, 3, 4, 0, 2).contiguous().to(torch.uint8)
        assert G.count_spikes(G.words_of(ptc), 3, T, 0)[:2] == (int(p.sum()), int(p[0].sum()))
        got = counted(ptc.to(dev))
        want = (int(p.sum()), int(p[0].sum()), p.numel(), p[0].numel(), True)
        tally("count_forms", values=2, mismatches=(got[0] != want[0]) + (got[1] != want[1]))
        assert got == want, T


@pytest.mark.parametrize("name", sorted(G.LARGE_COUNT_CASES))
def test_count_spikes_past_the_block_cap(dev, name):
    """More than 4096 blocks x 256 threads x 8 words: the grid is capped and every thread makes a ninth, ragged pass."""
    kind, shape, T, inner = G.LARGE_COUNT_CASES[name]
    t = G.large_count_tensor(name)
    words = G.words_of(t)
    assert words.size == G.large_count_words(name) > G.COUNT_WORDS_AT_CAP
    total, t0, ones = G.count_spikes(words, inner, T, kind)
    assert 0 < t0 < total
    r = ops.count_spikes(t.to(dev))
    tally("count_past_cap", values=2, mismatches=(r["total"] != total) + (r["t0"] != t0))
    assert (r["total"], r["t0"], r["binary"]) == (total, t0, True), (name, r)
    assert r["numel"] == t.numel() * (2 if kind == 1 else 1) and r["numel_t0"] == r["numel"] // T


@pytest.mark.parametrize("inner,T,outer,kind", [(70, 3, 1, 2), (3, 16, 5, 0), (4, 3, 7, 1), (8, 16, 2, 1), (5, 1, 3, 0)])
def test_count_spikes_attributes_step_zero_exactly(dev, inner, T, outer, kind):
    """Spikes only in step 0, only in step 1, only in step T - 1, on the very first and the very last word of the step in the first
    and the last outer block, through the C-ABI on raw words."""
    fill = {0: (0x01010101, 4), 1: (0x22222222, 8), 2: (0x3F800000, 1)}[kind]
    for name, (idx, n0) in G.placement_cases(inner, T, outer).items():
        w = np.zeros(inner * T * outer, dtype=np.uint32)
        w[idx] = fill[0]
        want = (fill[1] * len(idx), fill[1] * n0, len(idx) if kind == 2 else 0)
        assert G.count_spikes(w, inner, T, kind) == want
        got = raw_count(w, inner, T, kind, dev)
        tally("count_placement", values=3, mismatches=sum(a != b for a, b in zip(got, want)))
        assert got == want, (name, got, want)


def test_count_spikes_fp32_value_classes(dev):
    """{0, 1, -0.0} is a binary tensor and -0.0 is no spike; 0.5, 2.0, -1.0, NaN or a denormal each count as nonzero and make the
    tensor analogue."""
    base = torch.zeros(3, 10)
    base[0, 0] = base[1, 3] = base[2, 9] = base[0, 9] = 1.0
    base[0, 1] = base[2, 0] = -0.0
    assert int(torch.signbit(base).sum()) == 2
    got = counted(base.to(dev))
    tally("count_values", values=2, mismatches=(got[0] != 4) + (got[1] != 2))
    assert got == (4, 2, 30, 10, True)
    denormal = float(np.float32(1e-45))
    for v, step in ((0.5, 0), (2.0, 1), (-1.0, 2), (float("nan"), 0), (-float("nan"), 1), (denormal, 0), (-denormal, 2)):
        t = base.clone()
        t[step, 5] = v
        assert G.count_spikes(G.words_of(t), 10, 3, 2) == (5, 2 + (step == 0), 4)
        got = counted(t.to(dev))
        tally("count_values", values=2, mismatches=(got[0] != 5) + (got[1] != 2 + (step == 0)))
        assert got == (5, 2 + (step == 0), 30, 10, False), (v, got)
    with pytest.raises(RuntimeError):
        ops.count_spikes(base)


def test_count_spikes_of_a_sixteen_channel_generators_records(dev):
    """The S32 tensor of a 16-channel generator: total and t0 are the oracle's; ``numel`` counts record SLOTS, 32 per record (the
    upper sixteen are never set), so a rate taken against it is half the generator's."""
    c = G.case_of(G.MODEL_ROW)
    assert c.Cout == 16
    bits = G.spikegen_bits(c.cb, c.w, c.bias, c.a, c.b)
    rows = bits[G.token_rows(c.tokens, c.K).reshape(-1).numpy()].astype(np.uint32)       # [positions, 16]
    total = int(sum(((rows >> np.uint32(t)) & 1).sum() for t in range(16)))
    t0 = int((rows & 1).sum())
    assert 0 < t0 < total
    out = ops.spikegen_tokens_s32(*gen_args(c, dev), table_slot=None)
    r = ops.count_spikes(out)
    tally("count_generator_records", values=2, mismatches=(r["total"] != total) + (r["t0"] != t0))
    positions = c.tokens.numel()
    assert (r["total"], r["t0"], r["binary"]) == (total, t0, True)
    assert r["numel"] == positions * 16 * 32 and r["numel_t0"] == positions * 32
