"""The full-item form of spk_den_conv3x3_mfma_fp6v2 puts two adjacent TAPS of one weight digit into the K halves of an MFMA
(den_mfma_fp6v2.hip, "TAP PAIRS"): per-lane-half input cells, per-lane-half halves of two packed weight tiles, a scale that is uniform
over the lanes, four MFMAs per tap pair and row tile, tap 8 of the interior waves as a single tap.  What that can break, at the smallest
shapes that reach it (B = 3; Cout = 32, 64; Cin = 32, 64, 96: one, two and three chunks per item with the fragments carried over a chunk
boundary; plus one batch of more images than image lanes, so that a workgroup runs a second item) -- the inputs are described, and
shown on the host to be what they claim, in tests/_tap_pair_cases.py and tests/test_tap_pair_cases_host.py:

  a swapped lane half, a wrong tap distance          one tap at a time
  a wrong scale, the wrong half-tile slot            one weight digit at a time
  a pair of the wrong wave class, the single tap 8   border / interior / single-corner inputs, every input active

Every case forces the full-item form (`form` 1 of the C entry point, what ops.FP6V2_FORM = 1 passes) and is compared BIT FOR BIT, spikes and counts, with the six-plane kernel
(spk_den_conv3x3_mfma_fp6) and, on complete position lists, with the listed-position form, which keeps the digit-pair K loop: same
records, same counts, the SAME number of flagged neurons (flag_words[1]).  Outputs start as a sentinel: with a device-side image count
below B the images past it keep it.  After every call the live counter, the overflow bitmap and the ticket are clean.  The flagged
counts are printed per case (TAP_PAIR_FLAGS {json}) so that a run on another library (SPKDIFF_LIB) can be compared line by line."""
import json

import pytest
import torch

import _tap_pair_cases as C

pytestmark = pytest.mark.gpu

FLAG_LIST = 1 << 20          # id-list entries of the workspace (FLAG_CAP): [count, published count, ids..., bitmap, ticket]
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


_LISTS = {}


def _complete_lists(ops, dev, B):
    """Complete position lists: nothing unmasked, every position changes at t = 1 -> all 48 positions listed at every radius."""
    if B not in _LISTS:
        um = torch.zeros(B, 1, 7, 7, dtype=torch.bool, device=dev)
        ud = torch.zeros(B, 1, 7, 7, device=dev)
        act = ops.select_active(um, 1, ud)
        need = ops.select_needed(um, 1, act, ops.NeedLists(B, 4, dev), ud)
        assert int(act[1][0].item()) == B and bool((need.records(1).cpu()[:, 48] == 48).all())
        _LISTS[B] = (act, need)
    return _LISTS[B]


def _ws_clean(ws):
    return int(ws[0]) == 0 and int(ws[2 + FLAG_LIST:].abs().sum()) == 0


def _full_form(ops, lib, s32, pk2, Cout, ad, bd):
    """spk_den_conv3x3_mfma_fp6v2, form 1 (whole-image items), into sentinel-filled outputs (inside ops.active_set: its image count)."""
    B, nch, H, W, T, _ = s32.shape
    wq, scale, bias_d, wl1, qtab = pk2
    out = ops.empty_spikes(ops.S32, B, Cout, H, W, T, s32.device)
    out.view(torch.uint8).fill_(SENTINEL)
    cnt = torch.full((B, Cout // 32, H, W, 32), SENTINEL, dtype=torch.uint8, device=s32.device)
    flags = ops._flag_bitmap(s32.device, lib.spk_den_fp6v2_flag_words(B, Cout, H, W))
    ops.check(lib.spk_den_conv3x3_mfma_fp6v2(ops._p(s32), nch, ops._p(wq), ops._p(scale), ops._p(bias_d), ops._p(wl1), ops._p(qtab),
                                             ops._p(ad), ops._p(bd), ops._p(out), ops._p(cnt), ops._p(flags), T, B, H, W, Cout,
                                             ops._n_dyn(), int(ops.FLAG_CAP), 1, ops._stream(s32)), "spk_den_conv3x3_mfma_fp6v2")
    return out, cnt


def _check(ops, dev, spikes, layer, name, n_dyn=None):
    """One input [16, B, Cin, 7, 7] through the full-item form, the six-plane kernel and the listed form on complete lists."""
    from spkdiff._lib import lib
    _, B, Cin = spikes.shape[:3]
    w, bias, a, b = layer
    Cout = w.shape[0]
    wd, biasd, ad, bd = w.to(dev), bias.to(dev), a.to(dev), b.to(dev)
    # the six-plane kernel takes K chunks of 64 input channels: its copy of a Cin = 32 / 96 layer carries 32 more channels of zero
    # weights and zero spikes: exact zeros in an exact sum, the same quantisation scale (the row maximum).  It also takes output
    # channels by 64: its copy of a Cout = 32 layer carries 32 more output channels (zero weights, bias and BN: silent), dropped below
    # -- an output channel's quantisation, sums and LIF are its own
    pad = -Cout % 64
    w1 = torch.cat([torch.cat([w, torch.zeros(Cout, -Cin % 64, 3, 3)], 1), torch.zeros(pad, Cin + -Cin % 64, 3, 3)], 0).to(dev)
    zp = torch.zeros(pad, device=dev)
    pk2, pk1 = ops.den_pack_weight_fp6v2(wd, biasd), ops.den_pack_weight_fp6(w1, torch.cat([biasd, zp]))
    ws = ops._flag_bitmap(dev, lib.spk_den_fp6v2_flag_words(B, Cout, 7, 7))
    sd = spikes.to(dev)
    s32 = ops.spikes_to_s32(sd)
    sd1 = torch.cat([sd, torch.zeros(16, B, -Cin % 64, 7, 7, device=dev)], 2) if Cin % 64 else sd
    o1, c1 = ops.den_conv3x3_mfma_fp6(ops.spikes_to_c4(sd1), pk1, Cout + pad, bn_a=torch.cat([ad, zp]), bn_b=torch.cat([bd, zp]),
                                      want_counts=True)
    s1, c1 = ops.c4_to_spikes(o1)[:, :, :Cout], c1[:, :Cout // 32]
    n = B if n_dyn is None else n_dyn
    if n_dyn is not None:
        count = (torch.arange(B, dtype=torch.int32, device=dev), torch.tensor([n_dyn, 0], dtype=torch.int32, device=dev))
        with ops.active_set(*count):
            o2, c2 = _full_form(ops, lib, s32, pk2, Cout, ad, bd)
    else:
        o2, c2 = _full_form(ops, lib, s32, pk2, Cout, ad, bd)
    torch.cuda.synchronize()
    flagged = int(ws[1].item())
    assert _ws_clean(ws), (name, "live counter, overflow bitmap and ticket clean")
    firing = float(s1[:, :n].mean())
    line = {"B": B, "Cout": Cout, "Cin": Cin, "case": name, "flagged": flagged, "firing": round(firing, 6)}
    assert bool((o2[n:].view(torch.uint8) == SENTINEL).all()) and bool((c2[n:] == SENTINEL).all()), (name, "images past the count: untouched")
    s2 = ops.s32_to_spikes(o2[:n])
    assert torch.equal(s1[:, :n], s2), (B, Cout, Cin, name, int((s1[:, :n] != s2).sum()))
    assert torch.equal(c1[:n], c2[:n]), (B, Cout, Cin, name)
    assert 0.0 < firing < 1.0, "a case that fires nowhere or everywhere checks nothing"
    if n_dyn is None:
        act, need = _complete_lists(ops, dev, B)
        with ops.active_set(*act, need=need):
            o3, c3 = ops.den_conv3x3_mfma_fp6v2(s32, pk2, Cout, bn_a=ad, bn_b=bd, want_counts=True, need_radius=1)
        torch.cuda.synchronize()
        line["flagged_listed"] = int(ws[1].item())
        assert _ws_clean(ws), (name, "listed form: workspace clean")
        print("TAP_PAIR_FLAGS " + json.dumps(line))
        assert torch.equal(o3, o2) and torch.equal(c3, c2), (B, Cout, Cin, name, "listed form")
        assert line["flagged_listed"] == flagged, (B, Cout, Cin, name, "flagged: full-item form", flagged, "listed form", line["flagged_listed"])
        assert flagged < B * Cout * 49, "some neuron is decided by the matrix-core path"
    else:
        print("TAP_PAIR_FLAGS " + json.dumps(line))


@pytest.mark.parametrize("Cout,Cin", C.SHAPES)
def test_tap_pairs_one_tap_at_a_time(dev, ops, Cout, Cin):
    s = C.spikes_random(Cin, 0.30, Cin)
    for tap in range(9):
        _check(ops, dev, s, C.layer_one_tap(Cout, Cin, tap), f"tap{tap}")


@pytest.mark.parametrize("Cout,Cin", C.SHAPES)
def test_tap_pairs_one_digit_at_a_time(dev, ops, Cout, Cin):
    s = C.spikes_random(Cin, 0.30, 100 + Cin, silent0=True)
    for j in range(4):
        _check(ops, dev, s, C.layer_one_digit(Cout, Cin, j), f"digit{j}")


@pytest.mark.parametrize("Cout", C.COUTS)
def test_tap_pairs_border_interior_and_single_corner_inputs(dev, ops, Cout):
    layer = C.layer_random(Cout, 64)
    for k, (name, cells, rate, only) in enumerate(C.cell_cases()):
        _check(ops, dev, C.spikes_random(64, rate, 200 + k, cells=cells, only=only), layer, name)


@pytest.mark.parametrize("Cout", C.COUTS)
def test_tap_pairs_every_input_active(dev, ops, Cout):
    _check(ops, dev, torch.ones(16, C.B, 96, 7, 7), C.layer_random(Cout, 96), "all")


@pytest.mark.parametrize("Cout,Cin", C.SHAPES)
def test_tap_pairs_random_inputs(dev, ops, Cout, Cin):
    _check(ops, dev, C.spikes_random(Cin, 0.30, 400 + Cin), C.layer_random(Cout, Cin), "random30")


@pytest.mark.parametrize("Cout", C.COUTS)
def test_tap_pairs_image_count_on_the_device(dev, ops, Cout):
    """A device-side image count of 2 below B = 3: the third image's records and counts keep the sentinel."""
    _check(ops, dev, C.spikes_random(64, 0.30, 300), C.layer_random(Cout, 64), "n_dyn", n_dyn=2)


def test_tap_pairs_second_item_of_a_workgroup(dev, ops):
    """B = 3 leaves every workgroup one item.  Cout = 64 has cus / 2 image lanes: three more images than lanes give three workgroups a
    second item, whose first operands are read behind the first item's epilogue, at two chunks per item."""
    lanes = torch.cuda.get_device_properties(dev).multi_processor_count // 2
    g = torch.Generator().manual_seed(7500)
    s = (torch.rand(16, lanes + 3, 64, 7, 7, generator=g) < 0.30).float()
    _check(ops, dev, s, C.layer_random(64, 64), "second_item")
