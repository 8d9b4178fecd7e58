"""The nine layout conversions of the C-ABI (fp32 spikes [T,B,C,H,W] <-> u8 PTC / CPTC, <-> the nibble-packed C4 / S32 records;
channels-last fp32 -> C4 with and without the spike counts; u8 PTC -> S32), each pinned BIT FOR BIT to the host builders of
tests/_conv_bn_lif_oracle.py, through the wrappers of ``spkdiff.ops``.  Shapes are the smallest at which these kernels can go wrong:
one and two records of channels, a 3x5 map and B = 3 (nothing a multiple of the wave size), T = 16 and T = 4, plus one shape per
grid-stride kernel whose work exceeds the launch's block cap, so that the stride loop runs a second time."""
import pytest
import torch

import _conv_bn_lif_oracle as O

pytestmark = pytest.mark.gpu

DENSITY = 0.1
REC = {"c4": 64, "s32": 32}                 # channels per nibble-packed record


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def spikes(seed, T, B, C, H, W):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((T, B, C, H, W), generator=g) < DENSITY).float()


def records(s, rec):
    """The host's nibble-packed records of fp32 spikes [T,B,C,H,W], channels zero-padded to whole records: u8 [B,ceil(C/rec),H,W,T,rec/2]."""
    T, B, C, H, W = s.shape
    pad = -C % rec
    if pad:
        s = torch.cat([s, s.new_zeros((T, B, pad, H, W))], dim=2)
    return O.bits_to_packed(O.spikes_to_bits(s), rec, T)


def as_u8(q):
    assert q.dtype == torch.int8, q.dtype                      # the tag that keeps C4 / S32 apart from u8 CPTC of the same shape
    return q.cpu().view(torch.uint8)


def cl5(s):
    """The same fp32 [T,B,C,H,W] values with channels-last memory."""
    return s.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)


# ------------------------------------------------------------------------------------------------ C4 / S32 <-> fp32
@pytest.mark.parametrize("T", [16, 4])
@pytest.mark.parametrize("nrec", [1, 2])
@pytest.mark.parametrize("form", ["c4", "s32"])
def test_nibble_records_both_directions(dev, ops, form, nrec, T):
    rec = REC[form]
    s = spikes(100 + rec + nrec + T, T, 3, nrec * rec, 3, 5)
    want = records(s, rec)
    to, back = (ops.spikes_to_c4, ops.c4_to_spikes) if form == "c4" else (ops.spikes_to_s32, ops.s32_to_spikes)
    q = to(s.to(dev))
    assert tuple(q.shape) == (3, nrec, 3, 5, T, rec // 2)
    assert torch.equal(as_u8(q), want)
    assert torch.equal(O.packed_to_spikes(as_u8(q)), s)        # (also: every nibble is 0x0 or 0x2)
    r = back(want.view(torch.int8).to(dev))
    assert r.dtype == torch.float32 and tuple(r.shape) == tuple(s.shape)
    assert torch.equal(r.cpu(), s)
    assert torch.equal(back(q).cpu(), s)


@pytest.mark.parametrize("form,C", [("c4", 96), ("s32", 48)])
def test_nibble_records_refuse_a_partial_record(dev, ops, form, C):
    to = ops.spikes_to_c4 if form == "c4" else ops.spikes_to_s32
    with pytest.raises(NotImplementedError):
        to(spikes(7, 16, 1, C, 3, 5).to(dev))
    torch.cuda.synchronize()


# More than 65536 x 256 = 16 777 216 work items: one per output BYTE into records (B C HW T / 2 > 2^24) and one per output ELEMENT on
# the way back (B C HW T > 2^24), so every thread of the capped grid takes a second trip through the stride loop.
def test_nibble_records_past_the_grid_cap_into_records(dev, ops):
    T, B, C, H, W = 16, 147, 64, 15, 15
    assert B * C * H * W * T // 2 > 65536 * 256
    s = spikes(31, T, B, C, H, W)
    q = ops.spikes_to_c4(s.to(dev))
    assert torch.equal(as_u8(q), records(s, 64))


def test_nibble_records_past_the_grid_cap_back_to_spikes(dev, ops):
    T, B, C, H, W = 16, 147, 32, 15, 15
    assert B * C * H * W * T > 65536 * 256
    s = spikes(32, T, B, C, H, W)
    q = records(s, 32).view(torch.int8).to(dev)
    assert torch.equal(ops.s32_to_spikes(q).cpu(), s)


# ------------------------------------------------------------------------------------------------ channels-last fp32 -> C4 (+ counts)
@pytest.mark.parametrize("T", [16, 4])
@pytest.mark.parametrize("C", [64, 128])
def test_channels_last_spikes_to_c4_and_counts(dev, ops, C, T):
    s = spikes(200 + C + T, T, 3, C, 3, 5)
    want = records(s, 64)
    x = cl5(s.to(dev))
    assert x.permute(0, 1, 3, 4, 2).is_contiguous()
    assert torch.equal(as_u8(ops.spikes_cl_to_c4(x)), want)
    q, cnt = ops.spikes_cl_to_c4_counts(x)
    assert torch.equal(as_u8(q), want)
    assert cnt.dtype == torch.float32 and tuple(cnt.shape) == (3, C, 3, 5)
    assert cnt.permute(0, 2, 3, 1).is_contiguous()             # channels-last memory
    assert torch.equal(cnt.cpu(), s.sum(0))
    assert torch.equal(O.from_counts(O.to_counts(s)), cnt.cpu())


def test_channels_last_spikes_to_c4_refuses_a_partial_record(dev, ops):
    x = cl5(spikes(8, 16, 1, 96, 3, 5).to(dev))
    with pytest.raises(NotImplementedError):
        ops.spikes_cl_to_c4(x)
    with pytest.raises(NotImplementedError):
        ops.spikes_cl_to_c4_counts(x)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ u8 PTC -> S32
# C % 16 == 0 takes the 16-byte loads; 8 and 40 take the byte loop and leave the last record partly filled (both accepted by the
# library before and after the move).  The expected records come from the channels zero-padded to the next multiple of 32: the
# nibbles beyond C are zero.
@pytest.mark.parametrize("C", [16, 32, 64, 8, 40])
def test_ptc_to_s32(dev, ops, C):
    T, B, H, W = 16, 2, 5, 3
    s = spikes(300 + C, T, B, C, H, W)
    q = ops.ptc_to_s32(O.to_ptc(s).to(dev))
    assert tuple(q.shape) == (B, (C + 31) // 32, H, W, T, 16)
    assert torch.equal(as_u8(q), records(s, 32))


def test_ptc_to_s32_is_the_sixteen_step_form_only(dev, ops):
    with pytest.raises(NotImplementedError):
        ops.ptc_to_s32(O.to_ptc(spikes(9, 4, 2, 32, 5, 3)).to(dev))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ u8 PTC / CPTC <-> fp32
PTC_SHAPES = [(T, 3, 64, 3, 5) for T in (16, 4)] + [(16, 48, 64, 7, 7)]     # the last: T B C HW > 8192 x 256 work items


@pytest.mark.parametrize("chunk", [None, 32, 4], ids=["plain", "chunk32", "chunk4"])
@pytest.mark.parametrize("shape", PTC_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_ptc_and_cptc_both_directions(dev, ops, shape, chunk):
    T, B, C, H, W = shape
    if (T, B) == (16, 48):
        assert T * B * C * H * W > 8192 * 256
    s = spikes(400 + T + B + (chunk or 0), *shape)
    want = O.to_ptc(s, chunk)
    p = ops.spikes_to_ptc(s.to(dev), chunk)
    assert p.dtype == torch.uint8 and torch.equal(p.cpu(), want)
    r = ops.ptc_to_spikes(want.to(dev))
    assert r.dtype == torch.float32
    assert torch.equal(r.cpu(), O.from_ptc(want) if chunk is None else O.from_cptc(want))
    assert torch.equal(r.cpu(), s)


def test_ptc_to_spikes_reads_the_nibble_records_too(dev, ops):
    """``ptc_to_spikes`` is the module boundary's decode: it tells C4 and S32 (int8-tagged) from u8 CPTC of the same shape."""
    s = spikes(41, 16, 2, 64, 3, 5)
    for q in (ops.spikes_to_c4(s.to(dev)), ops.spikes_to_s32(s.to(dev)), ops.spikes_to_ptc(s.to(dev), 32),
              ops.spikes_to_ptc(s.to(dev), 16), ops.spikes_to_ptc(s.to(dev))):
        assert torch.equal(ops.ptc_to_spikes(q).cpu(), s)


# ------------------------------------------------------------------------------------------------ count_spikes on every layout
def test_count_spikes_of_each_layout(dev, ops):
    T, B, C, H, W = 16, 3, 64, 3, 5
    s = spikes(51, T, B, C, H, W)
    total, t0 = int(s.sum()), int(s[0].sum())
    x = s.to(dev)
    forms = {"fp32": x, "ptc": ops.spikes_to_ptc(x), "cptc": ops.spikes_to_ptc(x, 32), "c4": ops.spikes_to_c4(x),
             "s32": ops.spikes_to_s32(x)}
    for name, t in forms.items():
        r = ops.count_spikes(t)
        assert (r["total"], r["t0"], r["numel"], r["numel_t0"], r["binary"]) == (total, t0, s.numel(), s[0].numel(), True), (name, r)
