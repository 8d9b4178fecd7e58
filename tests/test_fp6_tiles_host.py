"""The host statement of the packed fp6 weight tiles (tests/_fp6_tiles_oracle.py), checked on the CPU: what it encodes decodes to the
quantised weights again, and the CONDITIONS ON THE INPUTS of tests/test_gpu_fp6_tiles.py hold in every case -- all six digit planes
carry non-zero digits of both signs, a leading digit reaches magnitude 16, one channel is all zero."""
import numpy as np
import pytest

import _fp6_tiles_oracle as T


@pytest.fixture(scope="module", params=T.CASES, ids=T.case_id)
def case(request):
    w, bias = T.case_weights(request.param)
    q, sh, scale = T.quantise(w.numpy(), request.param[3])
    return request.param, w, q, sh, scale


def test_digits_and_codes_round_trip():
    rng = np.random.default_rng(3)
    q = np.concatenate([rng.integers(-(1 << 29) + 1, 1 << 29, 4000), [0, 1, -1, 15, 16, -16, -17, (1 << 29) - 1, -(1 << 29) + 1,
                                                                      (1 << 29) - 32, 16 << 25, -(16 << 25)]])
    dg = T.digits(q)
    assert np.array_equal(T.undigits(dg), q)
    assert int(dg[1:].min()) >= -16 and int(dg[1:].max()) <= 15 and int(np.abs(dg[0]).max()) == 16
    assert np.array_equal(T.e2m3_digit(T.e2m3_code(dg)), dg)
    codes = rng.integers(0, 64, (50, 32)).astype(np.uint8)
    fr = T.fragment_bytes(codes)
    assert fr.shape == (50, 24) and np.array_equal(T.fragment_codes(fr), codes)
    # code k sits at bit 6 k of the little-endian stream
    one = np.zeros(32, dtype=np.uint8)
    one[5] = 0x21
    assert int.from_bytes(T.fragment_bytes(one).tobytes(), "little") == 0x21 << 30


def test_the_weights_are_exact_and_fill_every_digit_plane(case):
    (_, Cout, Cin, transposed), w, q, sh, scale = case
    wp = T.plain_view(w.numpy(), transposed)
    assert q.shape == (Cout, 9, Cin)
    assert np.array_equal(q.transpose(0, 2, 1).astype(np.float64) * scale[:, None, None], wp.astype(np.float64))   # packing is exact
    dg = T.digits(q)
    for p in range(6):
        assert int(dg[p].max()) > 0 and int(dg[p].min()) < 0, f"digit plane {p} lacks a sign"
    assert int(np.abs(dg[0]).max()) == 16
    zero = [co for co in range(Cout) if not q[co].any()]
    assert zero == [T.ZERO_CHANNEL] and sh[T.ZERO_CHANNEL] == 29
    live = np.delete(np.arange(Cout), T.ZERO_CHANNEL)
    assert (np.abs(q[live]).reshape(len(live), -1).max(axis=1) == (1 << 29) - 32).all()


def test_tiles_decode_to_the_quantised_weights(case):
    (kind, Cout, Cin, _), _, q, _, _ = case
    dg = T.digits(q)
    if kind == "v2":
        buf, mask = T.v2_slabs(q)
        assert buf.size == (Cout // 32) * (Cin // 32) * T.W_SLAB and int(mask.sum()) == (Cout // 32) * (Cin // 32) * T.V2_TILES * T.WT
        assert not mask.reshape(-1, T.W_SLAB)[:, T.V2_TILES * T.WT:].any()            # the padding is not defined
        got, have = T.v2_decode(buf, Cout, Cin)
        assert have[:5].all() and list(np.flatnonzero(have[5])) == [0, 1, 3, 4]
        assert np.array_equal(got[:5], dg[:5]) and np.array_equal(got[5][:, have[5]], dg[5][:, have[5]])
        taps = np.flatnonzero(have[5])
        assert np.array_equal(T.undigits(got[:, :, taps]), q[:, taps])
    else:
        buf, mask = T.vae_tiles(q)
        assert buf.size == (Cout // 32) * 9 * T.vae_tiles_per_tap(Cin) * T.WT and mask.all()
        got = T.vae_decode(buf, Cout, Cin)
        assert np.array_equal(got[:, :, :, :Cin], dg[:5]) and not got[:, :, :, Cin:].any()
        assert np.array_equal(T.undigits(np.concatenate([got[:, :, :, :Cin], dg[5:]])), q)
