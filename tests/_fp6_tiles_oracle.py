"""Host statement (numpy only) of the BYTE FORMAT of the certified kernels' packed weights: the slabs spk_den_pack_weight_fp6v2
writes and the tile array of spk_vae_fp6_pack.  Written from the format comments of csrc/den_mfma_fp6v2.hip ("weight packing"),
csrc/vae_fp6.hip (tiles_per_tap) and csrc/spk_common.h ("weight digits"), not from the kernels: the tiles are otherwise pinned only
through the spikes that come out of them (tests/test_fp6_tiles_host.py, tests/test_gpu_fp6_tiles.py).

Per output channel: m = max |w|, e its frexp exponent (m = f 2^e, f in [0.5, 1); 0 for an all-zero channel), sh = 29 - e,
q = rint(w 2^sh) (|q| < 2^29), scale = 2^-sh.  q = sum_p d_p 32^(5 - p): six balanced radix-32 digits, most significant first,
d_1..d_5 in [-16, 16), d_0 the rest (in [-16, 16]).  A digit travels as its 6-bit e2m3 code: sign bit 0x20 over the magnitude.

A FRAGMENT is 32 codes (32 consecutive input channels of one output channel, one tap, one digit) as a little-endian stream of 192
bits = 24 bytes.  A TILE is 1536 bytes = 64 lanes x 24: lane = K half * 32 + (output channel % 32); bytes 0..15 of a lane's fragment
at lane * 16, bytes 16..23 at 1024 + lane * 8.

fp6v2: one slab of W_SLAB bytes per (32-channel output group g, 32-channel input chunk c), at (g * chunks + c) * W_SLAB; 25 tiles:
  0..17   (tap, digit pair): tile 2 tap + pair, K half 0 = digit 2 pair, half 1 = digit 2 pair + 1
  18..22  fifth digit (p = 4), two taps per tile: K half 0 = tap 2 (tile - 18), half 1 = the next tap (tap 9: zeros)
  23, 24  sixth digit (p = 5) of taps (0, 1) and (3, 4)
  the 512 bytes behind the 25 tiles are padding: NOT defined.
vae_fp6: per group 9 x tiles_per_tap tiles, tile (g * 9 + tap) * tiles_per_tap + j; input channels beyond Cin are zero.
  two chunks (32 < Cin <= 64), tiles_per_tap 5: j = 0..3: chunk j / 2, digit pair j % 2 (K halves as above); j = 4: the fifth
      digit, K half 0 = chunk 0, half 1 = chunk 1
  one chunk (Cin <= 32), tiles_per_tap 3: j = 0, 1: digit pair j; j = 2: the fifth digit in K half 0, half 1 zeros.
  Weights: Conv2d [Cout][Cin][3][3], or ConvTranspose2d [Cin][Cout][3][3] (transposed)."""
import numpy as np

WT = 1536
V2_TILES = 25
W_SLAB = (V2_TILES * WT + 1023) // 1024 * 1024


def plain_view(w, transposed):
    """[Cout][Cin][9] float32 view of a Conv2d / ConvTranspose2d 3x3 weight."""
    w = np.asarray(w, dtype=np.float32)
    if transposed:
        w = w.transpose(1, 0, 2, 3)
    return w.reshape(w.shape[0], w.shape[1], 9)


def quantise(w, transposed=False):
    """-> q int64 [Cout][9][Cin] (the layout of the kernels' qtab), sh int [Cout], scale fp64 [Cout] = 2^-sh."""
    wp = plain_view(w, transposed)
    m = np.abs(wp).reshape(wp.shape[0], -1).max(axis=1)
    e = np.where(m > 0, np.frexp(m)[1], 0).astype(np.int64)
    sh = 29 - e
    q = np.rint(np.ldexp(wp.astype(np.float64), sh[:, None, None].astype(np.int32))).astype(np.int64)
    assert int(np.abs(q).max(initial=0)) < 1 << 29
    return np.ascontiguousarray(q.transpose(0, 2, 1)), sh, np.ldexp(1.0, (-sh).astype(np.int32))


def digits(q):
    """Balanced radix-32 digits of q, most significant first: int64 [6, *q.shape]."""
    q = np.asarray(q, dtype=np.int64).copy()
    dg = np.zeros((6,) + q.shape, dtype=np.int64)
    for p in range(5, 0, -1):
        r = ((q + 16) & 31) - 16
        dg[p] = r
        q = (q - r) >> 5
    dg[0] = q
    assert int(np.abs(dg[0]).max(initial=0)) <= 16
    return dg


def undigits(dg):
    q = np.zeros(dg.shape[1:], dtype=np.int64)
    for p in range(6):
        q = q * 32 + dg[p]
    return q


def e2m3_code(d):
    d = np.asarray(d, dtype=np.int64)
    return (np.where(d < 0, 0x20, 0) | np.abs(d)).astype(np.uint8)


def e2m3_digit(code):
    code = np.asarray(code, dtype=np.int64)
    return np.where(code & 0x20, -(code & 0x1f), code & 0x1f)


def fragment_bytes(codes):
    """[..., 32] codes -> [..., 24] bytes."""
    bits = np.unpackbits(np.asarray(codes, dtype=np.uint8)[..., None], axis=-1, bitorder="little")[..., :6]
    return np.packbits(bits.reshape(codes.shape[:-1] + (192,)), axis=-1, bitorder="little")


def fragment_codes(frag):
    """[..., 24] bytes -> [..., 32] codes."""
    bits = np.unpackbits(np.asarray(frag, dtype=np.uint8), axis=-1, bitorder="little").reshape(frag.shape[:-1] + (32, 6))
    return np.packbits(np.concatenate([bits, np.zeros(bits.shape[:-1] + (2,), np.uint8)], axis=-1), axis=-1,
                       bitorder="little")[..., 0]


def _put(buf, mask, tile_off, kh, frags):
    """The fragments [32][24] of the 32 output channels of a group into K half kh of the tile at tile_off."""
    for col in range(32):
        ln = kh * 32 + col
        buf[tile_off + ln * 16: tile_off + ln * 16 + 16] = frags[col, :16]
        buf[tile_off + 1024 + ln * 8: tile_off + 1024 + ln * 8 + 8] = frags[col, 16:]
    if mask is not None:
        mask[tile_off + kh * 512: tile_off + kh * 512 + 512] = True
        mask[tile_off + 1024 + kh * 256: tile_off + 1024 + kh * 256 + 256] = True


def _get(buf, tile_off, kh):
    out = np.zeros((32, 24), dtype=np.uint8)
    for col in range(32):
        ln = kh * 32 + col
        out[col, :16] = buf[tile_off + ln * 16: tile_off + ln * 16 + 16]
        out[col, 16:] = buf[tile_off + 1024 + ln * 8: tile_off + 1024 + ln * 8 + 8]
    return out


def v2_tile_content(tau, kh):
    """(tap, digit) of K half kh of slab tile tau, or None for the half that holds zeros."""
    if tau < 18:
        return tau >> 1, 2 * (tau & 1) + kh
    if tau < 23:
        tap = 2 * (tau - 18) + kh
        return (tap, 4) if tap < 9 else None
    return (0 if tau == 23 else 3) + kh, 5


def vae_tile_content(nch, j, kh):
    """(chunk, digit) of K half kh of tile j of a tap, or None for the half that holds zeros."""
    if nch == 2:
        return (j >> 1, 2 * (j & 1) + kh) if j < 4 else (kh, 4)
    if j < 2:
        return 0, 2 * j + kh
    return (0, 4) if kh == 0 else None


def _codes(q, cin_pad):
    """q [Cout][9][Cin] -> codes uint8 [6][Cout][9][cin_pad] (channels beyond Cin: digit 0)."""
    qp = np.zeros(q.shape[:2] + (cin_pad,), dtype=np.int64)
    qp[:, :, :q.shape[2]] = q
    return e2m3_code(digits(qp))


def v2_slabs(q):
    """q [Cout][9][Cin] -> (bytes uint8 [Cout/32 * Cin/32 * W_SLAB], mask of the defined bytes)."""
    Cout, _, Cin = q.shape
    assert Cout % 32 == 0 and Cin % 32 == 0
    G, nchunks = Cout // 32, Cin // 32
    codes = _codes(q, Cin)
    buf = np.zeros(G * nchunks * W_SLAB, dtype=np.uint8)
    mask = np.zeros(buf.shape, dtype=bool)
    zeros = np.zeros((32, 24), dtype=np.uint8)
    for g in range(G):
        for c in range(nchunks):
            for tau in range(V2_TILES):
                for kh in range(2):
                    what = v2_tile_content(tau, kh)
                    fr = zeros if what is None else fragment_bytes(
                        codes[what[1], g * 32:(g + 1) * 32, what[0], c * 32:(c + 1) * 32])
                    _put(buf, mask, (g * nchunks + c) * W_SLAB + tau * WT, kh, fr)
    return buf, mask


def vae_tiles_per_tap(Cin):
    return 5 if (Cin + 31) // 32 == 2 else 3


def vae_tiles(q):
    """q [Cout][9][Cin] -> (bytes uint8 [Cout/32 * 9 * tiles_per_tap * WT], mask of the defined bytes: all of them)."""
    Cout, _, Cin = q.shape
    assert Cout % 32 == 0 and 0 < Cin <= 64
    G, nch, tpt = Cout // 32, (Cin + 31) // 32, vae_tiles_per_tap(Cin)
    codes = _codes(q, nch * 32)
    buf = np.zeros(G * 9 * tpt * WT, dtype=np.uint8)
    mask = np.zeros(buf.shape, dtype=bool)
    zeros = np.zeros((32, 24), dtype=np.uint8)
    for g in range(G):
        for tap in range(9):
            for j in range(tpt):
                for kh in range(2):
                    what = vae_tile_content(nch, j, kh)
                    fr = zeros if what is None else fragment_bytes(
                        codes[what[1], g * 32:(g + 1) * 32, tap, what[0] * 32:(what[0] + 1) * 32])
                    _put(buf, mask, ((g * 9 + tap) * tpt + j) * WT, kh, fr)
    return buf, mask


def v2_decode(buf, Cout, Cin):
    """The digits a slab array holds: (dg int64 [6][Cout][9][Cin], have bool [6][9]: the sixth digit exists for taps 0, 1, 3, 4)."""
    G, nchunks = Cout // 32, Cin // 32
    dg = np.zeros((6, Cout, 9, Cin), dtype=np.int64)
    have = np.zeros((6, 9), dtype=bool)
    for g in range(G):
        for c in range(nchunks):
            for tau in range(V2_TILES):
                for kh in range(2):
                    what = v2_tile_content(tau, kh)
                    if what is None:
                        continue
                    fr = _get(buf, (g * nchunks + c) * W_SLAB + tau * WT, kh)
                    dg[what[1], g * 32:(g + 1) * 32, what[0], c * 32:(c + 1) * 32] = e2m3_digit(fragment_codes(fr))
                    have[what[1], what[0]] = True
    return dg, have


def vae_decode(buf, Cout, Cin):
    """The digits a tile array holds: dg int64 [5][Cout][9][nch * 32] (the sixth digit is not stored; channels beyond Cin: zero)."""
    G, nch, tpt = Cout // 32, (Cin + 31) // 32, vae_tiles_per_tap(Cin)
    dg = np.zeros((5, Cout, 9, nch * 32), dtype=np.int64)
    for g in range(G):
        for tap in range(9):
            for j in range(tpt):
                for kh in range(2):
                    what = vae_tile_content(nch, j, kh)
                    if what is None:
                        continue
                    fr = _get(buf, ((g * 9 + tap) * tpt + j) * WT, kh)
                    dg[what[1], g * 32:(g + 1) * 32, tap, what[0] * 32:(what[0] + 1) * 32] = e2m3_digit(fragment_codes(fr))
    return dg


# ------------------------------------------------------------------------------------------------ the cases of the two test files
# (packer, Cout, Cin, transposed): fp6v2 with one and with two groups and chunks; vae_fp6 with a half-filled chunk, with two chunks,
# and with the ConvTranspose2d indexing
CASES = (("v2", 32, 32, False), ("v2", 64, 64, False), ("vae", 32, 16, False), ("vae", 32, 64, False), ("vae", 64, 64, True))
ZERO_CHANNEL = 5


def case_id(case):
    return f"{case[0]}-{case[1]}x{case[2]}" + ("-T" if case[3] else "")


def case_weights(case):
    """Full-width weights (tests/_conv_bn_lif_oracle.py: integers q up to 2^29 - 2^5 times 2^(e-29), one tap per channel pinned to
    2^29 - 2^5) with channel ZERO_CHANNEL zeroed, and a bias.  -> (w as the packer takes it, bias, torch tensors)."""
    import torch

    import _conv_bn_lif_oracle as O
    _, Cout, Cin, transposed = case
    g = torch.Generator().manual_seed(1000 + 7 * Cout + Cin + (1 if transposed else 0))
    w, _ = O.full_width_weights(Cout, Cin, 3, g, -6, 1)
    w[ZERO_CHANNEL] = 0.0
    bias = torch.randn(Cout, generator=g)
    return (w.transpose(0, 1).contiguous() if transposed else w), bias
