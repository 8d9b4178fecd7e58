"""Cases with ONE correct answer for the denoiser's training gradient kernels (csrc/conv_wgrad.hip, csrc/conv_dgrad.hip,
csrc/conv_wgrad_small.hip), the conditions that make them so, and the launch forms those kernels pick.  No device code.

Oracle: ``torch.ops.aten.convolution_backward`` in fp64 on the CPU, on integer-valued data times powers of two: every sum stays
below 2^53, so the oracle is exact.

Exactness condition (``_settle``).  Every operand value is an integer multiple of its set's power-of-two unit, so every product
-- and every product of operand TERMS, the terms being integer multiples of the same units -- is an integer multiple of the
output's product unit u.  The builder computes, with the same fp64 operator on absolute values, S = sum over the output's terms
of |a| |b| and asserts S <= 2^24 u.  Then every partial sum of term products, in any order and any grouping, is an integer
multiple of u of magnitude <= 2^24 u: exactly representable in fp32.  That covers the MFMA chain, the two accumulators of the
data gradient and their final add, the split-K partial sums and their reduction, and the row sums of the bias gradient.  The
kernels' splits are exact and the products they drop are zero on these cases (asserted per case with the host emulations of the
splits below), so each output has one answer and is compared with ``torch.equal``.

What the budget of 2^24 allows.  A value of b significant bits times a spike count of 15 needs b + 4 bits: next to counts the
wide entries of the weight-gradient cases have 20 significant bits, next to binary spikes 20 to 24.  A 22-bit term of the data
gradient meets only factors of magnitude <= 3, a 24-bit one only factors of magnitude 1, and its receptive field holds no second
one unless both are shorter."""
import numpy as np
import torch

F32 = np.float32
U32 = np.uint32


def _cdiv(a, b):
    return -(-a // b)


# ================================================================================================ launch forms
def wgrad_ks0(Cout, Cin, cus):
    """wgrad_ksplit of csrc/conv_wgrad.hip before the cap by the image count."""
    tiles = (Cout // 128) * (Cin // 64)
    ks = cus // tiles
    if tiles == 1 and ks > 128:
        ks = 128
    return max(ks, 1)


def wgrad_form(TB, Cout, Cin, cus):
    """The slices of spk_conv3x3_wgrad_bf16: ``per`` images per slice, ``used`` slices that hold images, the image count of the
    ``last`` of them, ``empty`` slices behind it."""
    ks = max(1, min(wgrad_ks0(Cout, Cin, cus), TB))
    per = _cdiv(TB, ks)
    used = _cdiv(TB, per)
    return dict(tiles=(Cout // 128) * (Cin // 64), ksplit=ks, per=per, used=used, last=TB - (used - 1) * per, empty=ks - used)


def dgrad_nt(f16, N, Cin, cus):
    """dgrad_nt of csrc/conv_dgrad.hip: column tiles per wave."""
    if not f16 or Cin % 64:
        return 1
    groups = _cdiv(N, 8)
    r2 = _cdiv(groups * (Cin // 64), cus) * 2
    r1 = _cdiv(groups * (Cin // 32), cus)
    return 2 if r2 <= r1 else 1


def dgrad_form(form, N, Cout, Cin, cus):
    nt = dgrad_nt(form == "f16x2", N, Cin, cus)
    return dict(NT=nt, groups=_cdiv(N, 8), last_group=N - (_cdiv(N, 8) - 1) * 8, chunks=Cout // 16, col_tiles=Cin // (32 * nt))


def small_form(N, cus):
    """small_parts of csrc/conv_wgrad_small.hip and what follows from it: wave w of workgroup g takes images 4 g + w + 4 parts j."""
    parts = min(_cdiv(N, 4), cus)
    return dict(parts=parts, images_per_wave_max=_cdiv(N, 4 * parts), waves_with_a_second_image=max(0, min(N - 4 * parts, 4 * parts)),
                ragged=N % 4 != 0)


def wgrad_rows(cus):
    """(Cout, Cin, TB, claim) of the weight-gradient rows: TB follows from the device's slice count so that the row reaches the
    form it names on any CU count (at 256 CUs: 3 ks + 5 = 389, 2 ks + 1 = 257, 3 ks + 2 = 50)."""
    ks = wgrad_ks0(128, 64, cus)
    rows = [(128, 64, 4 * ((3 * ks + 4) // 4) + 1, lambda f: f["per"] == 4 and f["last"] == 1 and f["empty"] > 0)]
    ks = wgrad_ks0(256, 64, cus)
    rows.append((256, 64, 2 * ks + 1, lambda f: f["per"] == 3 and f["tiles"] == 2))
    ks = wgrad_ks0(512, 256, cus)
    rows.append((512, 256, 3 * ks + 2, lambda f: f["per"] >= 3 and f["tiles"] == 16))
    return rows


def dgrad_rows(cus):
    """(N, Cout, Cin, NT of the two-term form) of the data-gradient rows."""
    n2 = 8 * (cus // 4 + 1) - 5
    return [(n2, 16, 128, 2), (n2, 48, 128, 2), (3, 48, 96, 1), (13, 48, 96, 1), (11, 48, 128, 1)]


# (Cin, Cout, H, W, weight channels-last, bias gradient requested); N = 4 CUs + 7
SMALL_ROWS = [(2, 64, 7, 7, True, True), (1, 96, 8, 8, True, False), (3, 130, 5, 12, False, True), (4, 130, 2, 3, True, True),
              (4, 64, 8, 8, False, False), (2, 96, 5, 12, True, True), (3, 64, 7, 7, True, False), (1, 130, 2, 3, False, True)]


# ================================================================================================ host emulations of the splits
def split_bf16x3(x):
    """The kernels' three-term split (truncate, subtract, truncate, subtract): [hi, mid, lo] as fp32, hi + mid + lo == x."""
    x = np.ascontiguousarray(x, dtype=F32)
    h = (x.view(U32) & U32(0xFFFF0000)).view(F32)
    r = x - h
    m = (r.view(U32) & U32(0xFFFF0000)).view(F32)
    lo = r - m
    assert not (lo.view(U32) & U32(0xFFFF)).any(), "the third term is a bf16"
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + lo.astype(np.float64), x.astype(np.float64))
    return [h, m, lo]


def is_bf16(x):
    return not (np.ascontiguousarray(x, dtype=F32).view(U32) & U32(0xFFFF)).any()


def f16_scales(maxabs):
    """scale_of / inv_scale_of of csrc/conv_dgrad.hip for the largest magnitudes of sets (fp32 array)."""
    be = ((np.ascontiguousarray(maxabs, dtype=F32).view(U32) >> U32(23)) & U32(0xFF)).astype(np.int64)
    bc = np.maximum(be, 32)
    s = np.where(be == 0, 1.0, np.exp2(141.0 - bc)).astype(F32)
    inv = np.where(be == 0, 1.0, np.exp2(bc - 141.0)).astype(F32)
    return s, inv


def split_f16x2(x, scale):
    """x * scale = h + m + rest with h, m the nearest fp16: (h, m, rest) as fp32."""
    xs = np.ascontiguousarray(x, dtype=F32) * scale.astype(F32)
    h = xs.astype(np.float16).astype(F32)
    r = xs - h
    m = r.astype(np.float16).astype(F32)
    return h, m, r - m


# ================================================================================================ the fp64 operator
def _bwd(gy, x, w, mask):
    return torch.ops.aten.convolution_backward(gy, x, w, [w.shape[0]], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, mask)


def wgrad64(gy, x, bias=True):
    w = torch.zeros(gy.shape[1], x.shape[1], 3, 3, dtype=torch.float64)
    _, gw, gb = _bwd(gy.double(), x.double(), w, [False, True, bias])
    return gw, gb


def dgrad64(gy, w):
    x = torch.zeros(gy.shape[0], w.shape[1], gy.shape[2], gy.shape[3], dtype=torch.float64)
    return _bwd(gy.double(), x, w.double(), [True, False, False])[0]


class Case:
    """Operands (fp32, logical NCHW / [Cout,Cin,3,3]), the oracle's results as fp32 (exact), and what the builder proved."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _settle(what, val64, abs64, unit):
    """The exactness condition for one output tensor; returns the oracle's values as fp32 and the share of the 2^24 budget
    the fullest output uses."""
    unit = unit.double().expand_as(abs64)
    use = float((abs64 / unit).max()) / 2.0 ** 24
    assert use <= 1.0, (what, "sum of |terms| exceeds 2^24 product units:", use)
    q = val64 / unit
    assert torch.equal(q, q.round()), (what, "an output is not a whole number of product units")
    out = val64.float()
    assert torch.equal(out.double(), val64), (what, "an output is not an fp32")
    return out, use


def _f32(ints, exps):
    """integers (int64 array) times 2^exps -> fp32, exactly."""
    assert int(np.abs(ints).max()) < 2 ** 24
    v = ints.astype(np.float64) * np.exp2(exps.astype(np.float64))
    out = v.astype(F32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def _wide(rng, bits):
    """An odd integer of exactly ``bits`` significant bits below 2^(bits-1) + 2^(bits-2) whose remainder after the leading eight
    bits has more than eight significant bits (bit ``bits`` - 9 set): three bf16 terms; two fp16 terms once bits > 11."""
    top = 1 << (bits - 1)
    return top | (1 << (bits - 9)) | int(rng.randint(0, 1 << (bits - 2))) | 1


def _gapped(rng):
    """A 24-bit integer below 2^23 + 2^22 that is exactly two fp16 terms of 11 significant bits each: a 2^13 + b, b odd."""
    return (int(rng.randint(1024, 1536)) << 13) | int(rng.randint(1024, 2048)) | 1


def _signs(rng, shape):
    return rng.randint(0, 2, size=shape).astype(np.int64) * 2 - 1


# ================================================================================================ weight gradient
G_EXPS = np.array([-12, 0, 5, -3, 9, -20, 14])          # gy = m 2^e(co), e cycling over the output channels
COUNT_VALUES = np.array([0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 7, 8, 11, 13, 15, 16])


def make_wgrad(TB, Cout, Cin, HH, operand, seed=0):
    """gy [TB,Cout,HH,HH] and the operand x [TB,Cin,HH,HH] (``operand``: 'spikes' in {0,1} or 'counts' in 0..16).  gy = m 2^e(co):
    every entry non-zero and narrow (|m| in 1..7: one bf16 term), so every (image, row, column, channel) slot of the kernel's LDS
    images matters; on top, wide entries with all three bf16 terms populated -- next to spikes one of 24 significant bits in the
    even channels and three of 20, 22 and 23 in the odd ones, next to counts one of 20 per channel -- placed so that every map
    position (hence both k halves: the two image rows of a k group) carries one in some channel and image, the last image included."""
    rng = np.random.RandomState(1000 + seed)
    HW = HH * HH
    if operand == "spikes":
        x = (rng.rand(TB, Cin, HH, HH) < 0.3).astype(np.int64)
    else:
        x = COUNT_VALUES[rng.randint(0, len(COUNT_VALUES), size=(TB, Cin, HH, HH))]
        for v in (3, 5, 7, 11, 13, 15, 16):
            assert (x == v).any()
    m = rng.randint(1, 8, size=(TB, Cout, HH, HH)).astype(np.int64) * _signs(rng, (TB, Cout, HH, HH))
    wide = np.zeros(m.shape, dtype=bool)
    for co in range(Cout):
        bits = [20] if operand == "counts" else ([24] if co % 2 == 0 else [20, 22, 23])
        for j, b in enumerate(bits):
            pos = (co + 29 * j + 7 * (co // HW)) % HW
            img = (TB - 1 - 3 * co - 7 * j) % TB
            m[img, co, pos // HH, pos % HH] = _wide(rng, b) * (1 if (co + j) % 3 else -1)
            wide[img, co, pos // HH, pos % HH] = True
    e = G_EXPS[np.arange(Cout) % len(G_EXPS)]
    gy = _f32(m, np.broadcast_to(e.reshape(1, -1, 1, 1), m.shape))
    xf = x.astype(F32)
    # the kernel's operand forms: x by truncation to bf16, gy as three truncated bf16 terms
    assert is_bf16(xf), "the operand is exact in bf16"
    planes = split_bf16x3(gy)
    assert (planes[1][wide] != 0).all() and (planes[2][wide] != 0).all(), "wide entries populate all three term planes"
    assert not planes[1][~wide].any(), "narrow entries are one term"
    tg, tx = torch.from_numpy(gy), torch.from_numpy(xf)
    gw64, gb64 = wgrad64(tg, tx)
    aw64, ab64 = wgrad64(tg.abs(), tx)
    unit = torch.from_numpy(np.exp2(e.astype(np.float64)))
    gw, use_w = _settle("gw", gw64, aw64, unit.view(-1, 1, 1, 1))
    gb, use_b = _settle("gb", gb64, ab64, unit)
    return Case(kind="wgrad", gy=tg, x=tx, gw=gw, gb=gb, budget=max(use_w, use_b), wide=int(wide.sum()),
                wide_positions=int(wide.any(axis=(0, 1)).sum()), wide_in_last_image=bool(wide[TB - 1].any()), planes=planes)


# ================================================================================================ data gradient
N_EXPS = np.array([0, -20, 3, 1, 12, -2, 2])            # per image (gy) and per input channel (w): mixed binades, images at
C_EXPS = np.array([0, 2, -20, 1, -3, 12, 4, -1])        # 2^-20 and 2^+12 of the others
DGRAD_FAMILIES = {"bf16x3": ("g3w1", "g1w3", "g2w2"), "f16x2": ("g11w22", "g22w11")}


def _two_plane(rng, shape):
    return (rng.randint(2, 4, size=shape) * 256 + rng.randint(1, 4, size=shape)).astype(np.int64) * _signs(rng, shape)


def make_dgrad(form, family, N, Cout, Cin, HH, seed=0):
    """gy [N,Cout,HH,HH] = m 2^e(n) and w [Cout,Cin,3,3] = k 2^f(ci) (the scales sit on the axes that are not summed); the last
    image (N > 1) and input channel 5 are all zero.  Families (which side is wide):
      bf16x3  g3w1    gy narrow (|m| <= 3) plus two three-term entries per image, in output channels whose weights are small: 24
                      bits (the third term's eight bits all in play) where the weights are +-1, 17..22 bits where they are within
                      +-3; the other channels' weights have up to 8 significant bits: products (0,0) (1,0) (2,0)
              g1w3    the converse (wide weights: one of 24 or 22 bits, or two of <= 21, per input channel): (0,0) (0,1) (0,2)
              g2w2    +-(a 2^8 + b), a in {2,3}, b in {1,2,3}, on both sides, the weights sparse in (co, tap) (at most 16 per input
                      channel): (0,0) (0,1) (1,0) (1,1)
      f16x2   g11w22  gy of at most 11 significant bits x weights of up to 22 bits, and of two 11-bit terms with a gap between
                      them where bf16x3 has its 24-bit entries (two fp16 terms, no remainder): (h,h) (h,m)
              g22w11  the converse: (h,h) (m,h)
    The two wide entries of an image lie three or four rows apart: no output's 3x3 window holds both."""
    assert family in DGRAD_FAMILIES[form]
    rng = np.random.RandomState(2000 + seed)
    HW = HH * HH
    wide_side = {"g3w1": "g", "g22w11": "g", "g1w3": "w", "g11w22": "w", "g2w2": None}[family]
    other_max = 255 if form == "bf16x3" else 2047
    gshape, wshape = (N, Cout, HH, HH), (Cout, Cin, 3, 3)
    wide_ch = np.arange(Cout) % 5 == 2                      # the output channels that hold wide entries: both k halves of a chunk
    wch = np.nonzero(wide_ch)[0]
    unit_ch = wide_ch & ((np.arange(Cout) // 5) % 2 == 0)   # ... those of them whose other operand is +-1: room for 24 bits
    entry = lambda c, bits: (_wide(rng, 24) if form == "bf16x3" else _gapped(rng)) if unit_ch[c] else _wide(rng, bits)
    g_wide, w_wide = np.zeros(gshape, dtype=bool), np.zeros(wshape, dtype=bool)
    if wide_side is None:
        m = _two_plane(rng, gshape)
        k = _two_plane(rng, wshape)
        stride = max(1, Cout // 16)
        co, ci = np.arange(Cout).reshape(-1, 1), np.arange(Cin).reshape(1, -1)
        keep = ((co + ci) % stride == 0)[:, :, None] & (np.arange(9).reshape(1, 1, -1) == ((2 * co + ci) % 9)[:, :, None])
        k = k * keep.reshape(wshape)
    else:
        small = lambda shape: rng.randint(1, 4, size=shape).astype(np.int64) * _signs(rng, shape)
        big = lambda shape: rng.randint(1, other_max + 1, size=shape).astype(np.int64) * _signs(rng, shape)
        if wide_side == "g":
            m = small(gshape)
            k = big(wshape)
            k[0, 0, 0, 0] = other_max
            k[wide_ch] = small((len(wch), Cin, 3, 3))
            k[unit_ch] = _signs(rng, (int(unit_ch.sum()), Cin, 3, 3))
            for n in range(N):
                y, x = ((5 * n + 1) % HW) // HH, ((5 * n + 1) % HW) % HH
                for j, (yy, xx) in enumerate(((y, x), ((y + 4) % HH, (x + 3) % HH))):
                    c = wch[(n + j) % len(wch)]
                    m[n, c, yy, xx] = entry(c, 17 + (3 * n + 2 * j) % 6) * (1 if (n + j) % 2 else -1)
                    g_wide[n, c, yy, xx] = True
        else:
            k = small(wshape)
            m = big(gshape)
            m[0, 0, 0, 0] = other_max
            m[:, wide_ch] = small((N, len(wch), HH, HH))
            m[:, unit_ch] = _signs(rng, (N, int(unit_ch.sum()), HH, HH))
            for ci in range(Cin):
                bits = [22] if ci % 2 == 0 else [17 + ci % 5, 18 + ci % 4]
                for j, b in enumerate(bits):
                    c, tap = wch[(ci // 2 + j) % len(wch)], (ci + 4 * j) % 9
                    v = entry(c, b) if len(bits) == 1 else _wide(rng, b)
                    k[c, ci, tap // 3, tap % 3] = v * (1 if (ci + j) % 2 else -1)
                    w_wide[c, ci, tap // 3, tap % 3] = True
    if N > 1:
        m[N - 1] = 0
        g_wide[N - 1] = False
    k[:, 5] = 0
    w_wide[:, 5] = False
    en, fc = N_EXPS[np.arange(N) % len(N_EXPS)], C_EXPS[np.arange(Cin) % len(C_EXPS)]
    gy = _f32(m, np.broadcast_to(en.reshape(-1, 1, 1, 1), gshape))
    w = _f32(k, np.broadcast_to(fc.reshape(1, -1, 1, 1), wshape))
    # the kernel's operand terms, and the products it drops
    if form == "bf16x3":
        gt, wt = split_bf16x3(gy), split_bf16x3(w)
        dropped = [(1, 2), (2, 1), (2, 2)]
        if family == "g3w1":
            assert (gt[2][g_wide] != 0).all() and g_wide.any() and not wt[1].any()
        elif family == "g1w3":
            assert (wt[2][w_wide] != 0).all() and w_wide.any() and not gt[1].any()
        else:
            assert (gt[1][m != 0] != 0).all() and (wt[1][k != 0] != 0).all() and not gt[2].any() and not wt[2].any()
        scales = None
    else:
        gs, gi_ = f16_scales(np.abs(gy).reshape(N, -1).max(axis=1))
        ws_, wi_ = f16_scales(np.abs(w).transpose(1, 0, 2, 3).reshape(Cin, -1).max(axis=1))
        gh, gm, gr = split_f16x2(gy, gs.reshape(-1, 1, 1, 1))
        wh, wm, wr = split_f16x2(w, ws_.reshape(1, -1, 1, 1))
        assert not gr.any() and not wr.any(), "two fp16 terms reproduce every scaled value: no remainder, none subnormal"
        gt, wt, dropped = [gh, gm], [wh, wm], [(1, 1)]
        if wide_side == "g":
            assert (gm[g_wide] != 0).all() and g_wide.any() and not wm.any()
        else:
            assert (wm[w_wide] != 0).all() and w_wide.any() and not gm.any()
        scales = (gs, gi_, ws_, wi_)
    # entries whose LAST term uses its lowest mantissa bit (an error of one such bit is 2^-23 of the value)
    last = (gt if wide_side == "g" else wt)[-1]
    lsb = 0 if wide_side is None else int(((last.view(U32) >> U32(16)) & U32(1)).sum() if form == "bf16x3"
                                          else (last.astype(np.float16).view(np.uint16) & 1).sum())
    for a, b in dropped:                                     # (a term plane that is zero everywhere: every product with it is zero)
        assert not gt[a].any() or not wt[b].any(), ("a dropped product is not zero", family, a, b)
    tg, tw = torch.from_numpy(gy), torch.from_numpy(w)
    unit = torch.from_numpy(np.exp2(en.astype(np.float64))).view(-1, 1, 1, 1) * torch.from_numpy(np.exp2(fc.astype(np.float64))).view(1, -1, 1, 1)
    gi, use = _settle("gi", dgrad64(tg, tw), dgrad64(tg.abs(), tw.abs()), unit)
    if N > 1:
        assert not gi[N - 1].any()
    assert not gi[:, 5].any()
    return Case(kind="dgrad", form=form, family=family, gy=tg, w=tw, gi=gi, budget=use, gt=gt, wt=wt, scales=scales,
                wide=int(g_wide.sum() + w_wide.sum()), last_term_lsb=lsb)


# ================================================================================================ small-input weight gradient
def make_wgrad_small(N, Cin, Cout, H, W, seed=0):
    """gy [N,Cout,H,W] = m 2^e(co), |m| in 1..15, and the dense input x [N,Cin,H,W] = k 2^f(ci), |k| in 0..7."""
    rng = np.random.RandomState(3000 + seed)
    m = rng.randint(1, 16, size=(N, Cout, H, W)).astype(np.int64) * _signs(rng, (N, Cout, H, W))
    k = rng.randint(0, 8, size=(N, Cin, H, W)).astype(np.int64) * _signs(rng, (N, Cin, H, W))
    e, f = G_EXPS[np.arange(Cout) % len(G_EXPS)], np.array([0, -7, 5, 11])[np.arange(Cin)]
    gy = _f32(m, np.broadcast_to(e.reshape(1, -1, 1, 1), m.shape))
    x = _f32(k, np.broadcast_to(f.reshape(1, -1, 1, 1), k.shape))
    tg, tx = torch.from_numpy(gy), torch.from_numpy(x)
    gw64, gb64 = wgrad64(tg, tx)
    aw64, ab64 = wgrad64(tg.abs(), tx.abs())
    ue, uf = torch.from_numpy(np.exp2(e.astype(np.float64))), torch.from_numpy(np.exp2(f.astype(np.float64)))
    gw, use_w = _settle("gw", gw64, aw64, ue.view(-1, 1, 1, 1) * uf.view(1, -1, 1, 1))
    gb, use_b = _settle("gb", gb64, ab64, ue)
    return Case(kind="wgrad_small", gy=tg, x=tx, gw=gw, gb=gb, budget=max(use_w, use_b))


# ================================================================================================ the kernels' arithmetic on the host
def accumulate_f32(a_terms, b_terms, products, seed):
    """sum over k and over the (term of a, term of b) pairs of a_terms[ta][k, :, None] * b_terms[tb][k, None, :], every product
    and every addition in fp32, ONE accumulator, the (k, pair) steps in the order of a permutation drawn from ``seed``."""
    K = a_terms[0].shape[0]
    steps = [(kk, ta, tb) for kk in range(K) for ta, tb in products]
    order = np.random.RandomState(seed).permutation(len(steps))
    acc = np.zeros((a_terms[0].shape[1], b_terms[0].shape[1]), dtype=F32)
    for i in order:
        kk, ta, tb = steps[i]
        a, b = a_terms[ta][kk], b_terms[tb][kk]
        if a.any() and b.any():
            acc += a[:, None] * b[None, :]
    return acc


def _windows(x):
    """x [N,C,H,W] -> [N,H,W,C,3,3]: element (ky, kx) = x(y + ky - 1, x + kx - 1), zero outside."""
    N, C, H, W = x.shape
    p = np.zeros((N, C, H + 2, W + 2), dtype=x.dtype)
    p[:, :, 1:-1, 1:-1] = x
    out = np.empty((N, H, W, C, 3, 3), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out[:, :, :, :, ky, kx] = p[:, :, ky:ky + H, kx:kx + W].transpose(0, 2, 3, 1)
    return out


def emulate_wgrad(case, seed):
    """(gw, gb) as csrc/conv_wgrad.hip computes them: gy as three truncated bf16 terms times the bf16 operand, fp32 accumulation
    over (image, position, term); gb: the fp32 sum of gy over (image, position)."""
    gy, x = case.gy.numpy(), case.x.numpy()
    N, Cout, H, W = gy.shape
    Cin = x.shape[1]
    a = [t.transpose(0, 2, 3, 1).reshape(N * H * W, Cout) for t in split_bf16x3(gy)]
    b = [_windows(x).reshape(N * H * W, Cin * 9)]
    gw = accumulate_f32(a, b, [(0, 0), (1, 0), (2, 0)], seed).reshape(Cout, Cin, 3, 3)
    gb = accumulate_f32([gy.transpose(0, 2, 3, 1).reshape(N * H * W, Cout)], [np.ones((N * H * W, 1), dtype=F32)], [(0, 0)], seed + 1)
    return torch.from_numpy(gw), torch.from_numpy(gb[:, 0].copy())


def emulate_wgrad_small(case, seed):
    """csrc/conv_wgrad_small.hip: fp32 multiply-adds of the unsplit operands (its fp64 reduction of exact partial sums is exact)."""
    gy, x = case.gy.numpy(), case.x.numpy()
    N, Cout, H, W = gy.shape
    Cin = x.shape[1]
    a = [gy.transpose(0, 2, 3, 1).reshape(N * H * W, Cout)]
    gw = accumulate_f32(a, [_windows(x).reshape(N * H * W, Cin * 9)], [(0, 0)], seed).reshape(Cout, Cin, 3, 3)
    gb = accumulate_f32(a, [np.ones((N * H * W, 1), dtype=F32)], [(0, 0)], seed + 1)
    return torch.from_numpy(gw), torch.from_numpy(gb[:, 0].copy())


DGRAD_PRODUCTS = {"bf16x3": [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)], "f16x2": [(0, 0), (0, 1), (1, 0)]}


def emulate_dgrad(case, seed):
    """csrc/conv_dgrad.hip: the kept term products of the split operands accumulated in fp32 over (output channel, tap, product);
    the two-term form on the scaled operands, descaled by the two exact powers of two."""
    N, Cout, H, W = case.gy.shape
    Cin = case.w.shape[1]
    # gi(n, y, x, ci) = sum over (co, ky, kx) of gy(n, co, y + 1 - ky, x + 1 - kx) w(co, ci, ky, kx): windows with the taps flipped
    a = [_windows(t)[:, :, :, :, ::-1, ::-1].reshape(N * H * W, Cout * 9).T.copy() for t in case.gt]       # [k, rows]
    b = [t.transpose(0, 2, 3, 1).reshape(Cout * 9, Cin).copy() for t in case.wt]                             # [k, ci]
    acc = accumulate_f32(a, b, DGRAD_PRODUCTS[case.form], seed).reshape(N, H, W, Cin)
    if case.scales is not None:
        gs, g_inv, ws_, w_inv = case.scales
        acc = (acc * g_inv.reshape(-1, 1, 1, 1)) * w_inv.reshape(1, 1, 1, -1)
    return torch.from_numpy(acc.transpose(0, 3, 1, 2).copy())
