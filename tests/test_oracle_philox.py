"""Pins the host restatement of the sampler's noise (oracle/philox_ref.py) without a device: Philox4x32-10 against the
Random123 library's published known answers, the counter layout of one reverse step against its own contract
(include/spkdiff.h, spk_psample_step), and the host arithmetic of AbsorbingDiffusion._step_offset (counter intervals of
the steps and shards of a job are disjoint in the 'global' layout, and a shard draws the unsplit job's counters)."""
import numpy as np
import pytest
import torch

from oracle import philox_ref as pr

# Random123 tests/kat_vectors, philox4x32 10 rounds: counter, key, expected output
KAT = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox4x32_10_known_answers(ctr, key, out):
    got = pr.philox4x32_10(words(ctr), words(key))
    assert got.dtype == np.uint32 and [int(v) for v in got] == words(out)


def test_philox4x32_10_is_vectorised_over_counters_and_keys():
    ctr = np.array([words(c) for c, _, _ in KAT], dtype=np.uint64)
    key = np.array([words(k) for _, k, _ in KAT], dtype=np.uint64)
    got = pr.philox4x32_10(ctr, key)
    assert got.shape == (3, 4) and got.tolist() == [words(o) for _, _, o in KAT]
    # one key broadcast over a [2, 3, 4] block of counters
    blk = np.stack([ctr, ctr + 1]) & 0xFFFFFFFF
    one = pr.philox4x32_10(blk, words(KAT[2][1]))
    assert one.shape == (2, 3, 4) and one[0, 2].tolist() == words(KAT[2][2])
    assert one[1, 2].tolist() != one[0, 2].tolist()


def direct(seed, index, stream):
    """Word 0 of one counter, spelled out word by word."""
    index &= (1 << 64) - 1
    return int(pr.philox4x32_10([index & 0xFFFFFFFF, index >> 32, stream, 0], [seed & 0xFFFFFFFF, seed >> 32])[0])


def test_step_noise_zero_key_zero_counter_is_the_first_known_answer():
    n = pr.step_noise(0, 0, 1, 1, 1)
    assert int(n.n_u[0]) == 0x6627e8 and float(n.u[0]) == 0x6627e8 / 2.0 ** 24
    # stream 1 differs from stream 0 at the same counter
    assert int(n.n_q[0, 0]) == direct(0, 0, 1) >> 8 != 0x6627e8


@pytest.mark.parametrize("seed", [0, 1, 1 << 32, (1 << 62) - 1, 0x1234567_89ABCDEF])
@pytest.mark.parametrize("offset", [0, (1 << 32) - 1000, 99 * (1 << 40) + 7 * 49 * 128, (1 << 63) + 5, (1 << 64) - 300])
def test_step_noise_counter_layout(seed, offset):
    B, HW, K = 3, 5, 100                      # 1500 counters: 2^32 - 1000 and 2^64 - 300 carry / wrap inside the call
    n = pr.step_noise(seed, offset, B, HW, K)
    assert n.u.shape == (15,) and n.q.shape == (15, 100) and n.u.dtype == np.float32 and n.q.dtype == np.float32
    for p in (0, 1, 9, 10, 14):
        assert int(n.n_u[p]) == direct(seed, offset + p * K, 0) >> 8
        for k in (0, 1, 50, 99):
            assert int(n.n_q[p, k]) == direct(seed, offset + p * K + k, 1) >> 8
    assert np.array_equal(n.u, (n.n_u * 2.0 ** -24).astype(np.float32))
    assert np.array_equal(n.q64, -np.log((n.n_q.astype(np.float64) + 1) / 2.0 ** 24))
    assert np.array_equal(n.q, n.q64.astype(np.float32))
    only_u = pr.step_noise(seed, offset, B, HW, K, want_q=False)
    assert np.array_equal(only_u.u, n.u) and only_u.q is None


def test_step_noise_depends_on_every_key_and_counter_word():
    base = pr.step_noise(5, 0, 2, 4, 8)
    for seed, off in ((5 + (1 << 32), 0), (5, 1 << 32), (5, 1 << 40), (5, 1), (6, 0)):
        other = pr.step_noise(seed, off, 2, 4, 8)
        assert not np.array_equal(other.n_u, base.n_u) and not np.array_equal(other.n_q, base.n_q)
    # offset + 1 shifts the q stream by one class; u of position p + 1 sits K counters on
    shifted = pr.step_noise(5, 8, 2, 4, 8)
    assert np.array_equal(shifted.n_u[:-1], base.n_u[1:]) and np.array_equal(shifted.n_q[:-1], base.n_q[1:])


def test_step_noise_state_replaces_the_seed_and_adds_to_the_offset_modulo_2_64():
    for seed, off, state in ((0, 12345, (991, 4096)), (77, (1 << 40) + 3, (1 << 61, (1 << 32) - 2)),
                             (1, (1 << 64) - 10, ((1 << 62) - 1, 500)), (3, 5, (8, (1 << 64) - 5))):
        a = pr.step_noise(seed, off, 2, 3, 7, state=state)
        b = pr.step_noise(state[0], (off + state[1]) % (1 << 64), 2, 3, 7)
        assert np.array_equal(a.n_u, b.n_u) and np.array_equal(a.n_q, b.n_q)


def test_step_noise_ranges_and_the_extreme_mantissas():
    n = pr.step_noise(42, 3 << 40, 64, 49, 128)           # 401 408 counters
    assert n.n_u.max() < 1 << 24 and n.n_q.max() < 1 << 24
    assert n.u.min() >= 0.0 and n.u.max() < 1.0
    assert n.q.min() >= 0.0 and n.q.max() <= 16.64 and n.q64.max() <= 24 * np.log(2.0)
    assert abs(float(n.u.mean()) - 0.5) < 0.03 and abs(float(n.q64.mean()) - 1.0) < 0.01
    # the ends of the mantissa range: q = 0 exactly at all ones, 24 ln 2 at zero
    assert pr.q_of_mantissa(np.array([(1 << 24) - 1]))[0] == 0.0
    assert pr.q_of_mantissa(np.array([0]))[0] == pytest.approx(16.6355323334, abs=1e-9)
    # the chunked q generation equals one pass
    small = pr.step_noise(42, 3 << 40, 64, 49, 128, chunk=1000)
    assert np.array_equal(small.n_q, n.n_q)


# ----------------------------------------------------------------------------------------------- AbsorbingDiffusion._step_offset
class _Den(torch.nn.Module):
    num_embeddings = 512


def _sampler(layout, first=None, count=None):
    from snn_model.vq_diffusion import AbsorbingDiffusion
    ab = AbsorbingDiffusion(_Den(), mask_id=512, latent_shape=(8, 8))
    ab.noise_layout = layout
    if first is not None:
        ab.set_shard(first, count)
    return ab


def _intervals(ab, b, steps=100, h=8, w=8, K=512):
    return [(ab._step_offset(s, b, h, w, K), ab._step_offset(s, b, h, w, K) + b * h * w * K) for s in range(steps)]


def _pairwise_disjoint(iv):
    iv = sorted(iv)
    return all(a[1] <= b[0] for a, b in zip(iv, iv[1:]))


@pytest.mark.parametrize("B", [256, 8192])
def test_step_offset_global_layout_steps_and_shards_are_disjoint_sub_intervals(B):
    h = w = 8
    K = 512
    whole = _intervals(_sampler('global'), B)
    assert whole[0][0] == 0 and all(lo == s << 40 for s, (lo, _) in enumerate(whole))
    assert all(0 <= lo < hi <= 1 << 64 for lo, hi in whole)               # the device adds in 64 bits: no wrap in a job
    assert _pairwise_disjoint(whole)
    shards = 8
    per = B // shards
    every = []
    for r in range(shards):
        ab = _sampler('global', r * per, per)
        assert ab.n_samples == per and ab.global_first == r * per
        iv = _intervals(ab, per)
        for s, (lo, hi) in enumerate(iv):
            # the counters the unsplit job gives images [r*per, (r+1)*per) at step s
            assert lo == whole[s][0] + r * per * h * w * K and hi == lo + per * h * w * K and hi <= whole[s][1]
        every += iv
    assert len(every) == shards * 100 and _pairwise_disjoint(every)
    # the shards of one step tile the unsplit job's interval exactly
    for s in range(100):
        step = sorted(every[r * 100 + s] for r in range(shards))
        assert step[0][0] == whole[s][0] and step[-1][1] == whole[s][1]
        assert all(a[1] == b[0] for a, b in zip(step, step[1:]))


def test_step_offset_global_layout_refuses_a_step_that_does_not_fit_its_stride():
    ab = _sampler('global', (1 << 40) // (64 * 512) - 10, 16)
    with pytest.raises(ValueError):
        ab._step_offset(0, 16, 8, 8, 512)
    ab = _sampler('global', (1 << 40) // (64 * 512) - 16, 16)            # the last 16 images that fit
    assert ab._step_offset(1, 16, 8, 8, 512) + 16 * 64 * 512 == 2 << 40


@pytest.mark.parametrize("B", [256, 1024])
def test_step_offset_rank_layout_steps_are_adjacent(B):
    """'rank' layout: local image index, step stride b*h*w*K; the shard does not enter the offset (the rank is folded into
    the key), so the steps of one sampler tile [0, steps * b*h*w*K)."""
    for first in (None, 3 * B):
        ab = _sampler('rank', first, None if first is None else B)
        iv = _intervals(ab, B)
        assert iv[0][0] == 0 and all(a[1] == b[0] for a, b in zip(iv, iv[1:])) and iv[-1][1] == 100 * B * 64 * 512
    with pytest.raises(ValueError):
        _sampler('neither')._step_offset(0, 4, 8, 8, 512)
