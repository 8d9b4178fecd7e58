"""On full 7x7 items of spk_den_conv3x3_mfma_fp6v2 three of the eight waves of a workgroup -- the 18-step border waves top, right and
left -- issue ALL the LDS-DMA copies of a chunk (41 pieces: 14 image-row pieces, 27 weight pieces; 14 / 14 / 13 per wave, one per K-loop
step, the first chunk's weight pieces in front of the LDS zeroing); the bottom wave and the four interior waves copy nothing
(den_mfma_fp6v2.hip, "COPY ROLES").  The (cell, step) input records of an item are counted by all 512 threads, two each.  What the
roles can break, at the smallest shapes that reach it:

  a piece nobody copies, or copied into the wrong buffer   -> wrong spikes: compared BIT FOR BIT with the six-plane kernel
                                                              (spk_den_conv3x3_mfma_fp6) and, on complete position lists, with the
                                                              listed-position form, which keeps the symmetric roles
  chunks per item    Cin = 32 / 64 / 96: one chunk (the prologue's copies only), two (one steady-state copy and the read-ahead of the
                     next chunk), three (both buffers reused)
  items per group    Cout = 128 leaves cus / 4 image lanes per channel group (64 on 256 CUs): B = 1, 2, lanes + 6, 2 lanes + 2 are
                     1, 1, 2 and a ragged 3 items per workgroup -- the next item's first chunk is copied during the last chunk of the
                     current one
  device image count an image count below B (n_dyn): the workgroups past it copy nothing, the last chunk is copied once more
  a record counted twice or never -> the counts feed only the certification bound, so spikes rarely move; the number of neurons the
                     main launch flags (flag_words[1]) does.  Full-item form and listed form count the same n_t on complete lists, so
                     their flagged counts are compared (they agree at the parent commit too), with every input active (n_t at its
                     maximum of 9 Cin) and with ONE spike in one record: the ends of the rounds of a division among 512 threads
                     (0, 511, 512, 783) and among 256 (255, 256, 767, 768: the division that was measured and not kept).

Small batches take the half-image form by themselves: every call here forces the full-item form (ops.FP6V2_FORM = 1).  The flagged
counts are printed per case (COPY_ROLES_FLAGS {json}) so that a run on another library (SPKDIFF_LIB) can be compared line by line."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

FLAG_LIST = 1 << 20          # id-list entries of the workspace (FLAG_CAP): [count, published count, ids..., bitmap, ticket]
COUT = 128
SINGLE_RECORDS = (0, 255, 256, 511, 512, 767, 768, 783)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


@pytest.fixture(scope="module")
def lanes(dev):
    """Image lanes per channel group of a Cout = 128 launch: the host code walks one workgroup per CU, Cout / 32 groups."""
    n = torch.cuda.get_device_properties(dev).multi_processor_count // (COUT // 32)
    assert n >= 6
    return n


class _full_form:
    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        self.prev, self.ops.FP6V2_FORM = self.ops.FP6V2_FORM, 1

    def __exit__(self, *exc):
        self.ops.FP6V2_FORM = self.prev
        return False


_LAYERS = {}


def _layer(ops, dev, Cin):
    """Weights, BN and packed forms of one (COUT, Cin) layer: made once, shared by the cases."""
    if Cin not in _LAYERS:
        g = torch.Generator().manual_seed(9100 + Cin)
        w = (torch.rand(COUT, Cin, 3, 3, generator=g) - 0.5) * 0.05
        w[:, :, 1, 1] *= 3.0
        bias = (torch.rand(COUT, generator=g) - 0.5) * 0.2
        a = (torch.rand(COUT, generator=g) - 0.3) * 12.0                  # some negative BN scales
        b = (torch.rand(COUT, generator=g) - 0.4) * 1.5
        wd, biasd = w.to(dev), bias.to(dev)
        # the six-plane kernel takes K chunks of 64 input channels: its copy of a Cin = 32 / 96 layer carries 32 more channels of
        # zero weights (and zero spikes, _check): exact zeros in an exact sum, the same quantisation scale (the row maximum)
        w1 = torch.cat([w, torch.zeros(COUT, -Cin % 64, 3, 3)], 1).to(dev)
        _LAYERS[Cin] = (ops.den_pack_weight_fp6v2(wd, biasd), ops.den_pack_weight_fp6(w1, biasd), a.to(dev), b.to(dev))
    return _LAYERS[Cin]


def _ws_clean(ws):
    return int(ws[0]) == 0 and int(ws[2 + FLAG_LIST:].abs().sum()) == 0


def _check(ops, dev, spikes, name, n_dyn=None):
    """One input [16, B, Cin, 7, 7] through the full-item form, the six-plane kernel and the listed form on complete lists."""
    from spkdiff._lib import lib
    _, B, Cin = spikes.shape[:3]
    pk2, pk1, ad, bd = _layer(ops, dev, Cin)
    ws = ops._flag_bitmap(dev, lib.spk_den_fp6v2_flag_words(B, COUT, 7, 7))
    sd = spikes.to(dev)
    s32 = ops.spikes_to_s32(sd)
    sd1 = torch.cat([sd, torch.zeros(16, B, -Cin % 64, 7, 7, device=dev)], 2) if Cin % 64 else sd
    o1, c1 = ops.den_conv3x3_mfma_fp6(ops.spikes_to_c4(sd1), pk1, COUT, bn_a=ad, bn_b=bd, want_counts=True)
    s1 = ops.c4_to_spikes(o1)
    n = B if n_dyn is None else n_dyn
    if n_dyn is not None:
        count = (torch.arange(B, dtype=torch.int32, device=dev), torch.tensor([n_dyn, 0], dtype=torch.int32, device=dev))
        with _full_form(ops), ops.active_set(*count):
            o2, c2 = ops.den_conv3x3_mfma_fp6v2(s32, pk2, COUT, bn_a=ad, bn_b=bd, want_counts=True)
    else:
        with _full_form(ops):
            o2, c2 = ops.den_conv3x3_mfma_fp6v2(s32, pk2, COUT, bn_a=ad, bn_b=bd, want_counts=True)
    torch.cuda.synchronize()
    flagged = int(ws[1].item())
    assert _ws_clean(ws), (name, "live counter, overflow bitmap and ticket clean")
    s2 = ops.s32_to_spikes(o2)
    line = {"B": B, "Cin": Cin, "case": name, "flagged": flagged, "firing": round(float(s1[:, :n].mean()), 6)}
    assert torch.equal(s1[:, :n], s2[:, :n]), (B, Cin, name, int((s1[:, :n] != s2[:, :n]).sum()))
    assert torch.equal(c1[:n], c2[:n]), (B, Cin, name)
    assert 0.0 < float(s1[:, :n].mean()) < 1.0, "a case that fires nowhere or everywhere checks nothing"
    if n_dyn is None:
        # complete position lists: nothing unmasked, every position changes at t = 1 -> all 48 positions listed at every radius
        um = torch.zeros(B, 1, 7, 7, dtype=torch.bool, device=dev)
        ud = torch.zeros(B, 1, 7, 7, device=dev)
        act = ops.select_active(um, 1, ud)
        need = ops.select_needed(um, 1, act, ops.NeedLists(B, 4, dev), ud)
        assert int(act[1][0].item()) == B and bool((need.records(1).cpu()[:, 48] == 48).all())
        with ops.active_set(*act, need=need):
            o3, c3 = ops.den_conv3x3_mfma_fp6v2(s32, pk2, COUT, bn_a=ad, bn_b=bd, want_counts=True, need_radius=1)
        torch.cuda.synchronize()
        line["flagged_listed"] = int(ws[1].item())
        assert _ws_clean(ws), (name, "listed form: workspace clean")
        print("COPY_ROLES_FLAGS " + json.dumps(line))
        assert torch.equal(o3, o2) and torch.equal(c3, c2), (B, Cin, name, "listed form")
        assert line["flagged_listed"] == flagged, (B, Cin, name, "flagged: full-item form", flagged, "listed form", line["flagged_listed"])
    else:
        print("COPY_ROLES_FLAGS " + json.dumps(line))


def _random(g, B, Cin, rate):
    return (torch.rand(16, B, Cin, 7, 7, generator=g) < rate).float()


@pytest.mark.parametrize("Cin", [32, 64, 96])
def test_copy_roles_chunks_per_item(dev, ops, lanes, Cin):
    """One, two and three chunks per item at two items per workgroup: random inputs at 5 % and 30 %, and every input active."""
    B = lanes + 6
    g = torch.Generator().manual_seed(9200 + Cin)
    _check(ops, dev, _random(g, B, Cin, 0.05), "random5")
    _check(ops, dev, _random(g, B, Cin, 0.30), "random30")
    _check(ops, dev, torch.ones(16, B, Cin, 7, 7), "all")


@pytest.mark.parametrize("items", ["one_image", "two_images", "two_items", "ragged_three_items"])
def test_copy_roles_items_per_workgroup(dev, ops, lanes, items):
    """1, 1, 2 and a ragged 3 items per workgroup (B = 1, 2, lanes + 6, 2 lanes + 2) at two chunks per item."""
    B = {"one_image": 1, "two_images": 2, "two_items": lanes + 6, "ragged_three_items": 2 * lanes + 2}[items]
    g = torch.Generator().manual_seed(9300 + B)
    _check(ops, dev, _random(g, B, 64, 0.30), items)
    _check(ops, dev, torch.ones(16, B, 64, 7, 7), items + "_all")


def test_copy_roles_image_count_on_the_device(dev, ops, lanes):
    """B = lanes + 6 with a device-side image count of lanes + 1: one workgroup runs two items, the rest one, none the images beyond."""
    B = lanes + 6
    g = torch.Generator().manual_seed(9400)
    _check(ops, dev, _random(g, B, 64, 0.30), "n_dyn", n_dyn=lanes + 1)


@pytest.mark.parametrize("rec", SINGLE_RECORDS)
def test_copy_roles_one_spike_in_one_record(dev, ops, rec):
    """ONE input spike of the batch: image 1 of 2, channel 40 (the second chunk), record rec = cell * 16 + step."""
    spikes = torch.zeros(16, 2, 64, 7, 7)
    cell, t = rec >> 4, rec & 15
    spikes[t, 1, 40, cell // 7, cell % 7] = 1.0
    _check(ops, dev, spikes, f"record{rec}")
