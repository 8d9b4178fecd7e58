"""The full-item form of spk_den_conv3x3_mfma_fp6v2 skips the (tile, tap) steps that read only the zero border of a 7x7 latent
(den_mfma_fp6v2.hip, "BORDER SKIP"): its waves hold the border positions side by side and run K loops of 6 instead of 9 tap
blocks.  A tap that is wrongly omitted, or a position the new map sends to the wrong output record, changes spikes -- so every
case is compared BIT FOR BIT with the six-plane kernel (spk_den_conv3x3_mfma_fp6: all nine taps, its own position order), and,
through complete position lists, with the listed-position form, which keeps the old map and all nine taps.

Inputs put the weight on the border:
  border    spikes only in the 24 border cells
  interior  spikes only in the 25 interior cells
  all       every input active at every step (any omitted tap that touches the image would be missed); B = 64 only
  corner k  ONE image of the batch active, in the single corner cell k
The number of neurons the certification flags (flag_words[1]) depends on the counted active inputs, not on the map: it is printed
per case (BORDER_SKIP_FLAGS ...) so that a run on another library (SPKDIFF_LIB) can be compared line by line."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

FLAG_LIST = 1 << 20          # id-list entries of the workspace (FLAG_CAP): [count, published count, ids..., bitmap, ticket]
SHAPES = ((128, 64), (256, 128), (512, 256), (256, 512))          # (Cout, Cin) of den.conv2 .. conv5
CORNERS = ((0, 0), (0, 6), (6, 0), (6, 6))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def _cases(B):
    border = torch.zeros(7, 7, dtype=torch.bool)
    border[0, :] = border[6, :] = border[:, 0] = border[:, 6] = True
    out = [("border", border, 0.30, None), ("interior", ~border, 0.30, None)]
    if B == 64:
        out.append(("all", torch.ones(7, 7, dtype=torch.bool), 1.0, None))
    for k, (y, x) in enumerate(CORNERS):
        cell = torch.zeros(7, 7, dtype=torch.bool)
        cell[y, x] = True
        out.append((f"corner{k}", cell, 0.5, (k * (B - 1)) // 3))     # the one active image: first, two in between, last
    return out


@pytest.mark.parametrize("B,shapes", [(64, SHAPES), (256, (SHAPES[2],))])
def test_fp6v2_border_skip_bit_equal_to_the_six_plane_kernel(dev, ops, B, shapes):
    from spkdiff._lib import lib
    # complete position lists: nothing unmasked, every position changes at t = 1 -> all 48 positions listed at every radius
    um = torch.zeros(B, 1, 7, 7, dtype=torch.bool, device=dev)
    ud = torch.zeros(B, 1, 7, 7, device=dev)
    act = ops.select_active(um, 1, ud)
    need = ops.select_needed(um, 1, act, ops.NeedLists(B, 4, dev), ud)
    assert int(act[1][0].item()) == B and bool((need.records(1).cpu()[:, 48] == 48).all())
    g = torch.Generator().manual_seed(4200 + B)
    for Cout, Cin in shapes:
        w = (torch.rand(Cout, Cin, 3, 3, generator=g) - 0.5) * 0.05
        w[:, :, 1, 1] *= 3.0
        bias = (torch.rand(Cout, generator=g) - 0.5) * 0.2
        a = (torch.rand(Cout, generator=g) - 0.3) * 12.0                  # some negative BN scales
        b = (torch.rand(Cout, generator=g) - 0.4) * 1.5
        wd, biasd, ad, bd = w.to(dev), bias.to(dev), a.to(dev), b.to(dev)
        pk2, pk1 = ops.den_pack_weight_fp6v2(wd, biasd), ops.den_pack_weight_fp6(wd, biasd)
        ws = ops._flag_bitmap(dev, lib.spk_den_fp6v2_flag_words(B, Cout, 7, 7))
        for name, cells, rate, only in _cases(B):
            spikes = (torch.rand(16, B, Cin, 7, 7, generator=g) < rate).float() * cells.float()
            if only is not None:
                keep = torch.zeros(B)
                keep[only] = 1.0
                spikes = spikes * keep.view(1, B, 1, 1, 1)
            sd = spikes.to(dev)
            s32 = ops.spikes_to_s32(sd)
            o2, c2 = ops.den_conv3x3_mfma_fp6v2(s32, pk2, Cout, bn_a=ad, bn_b=bd, want_counts=True)
            torch.cuda.synchronize()
            flagged = int(ws[1].item())
            assert int(ws[0]) == 0 and int(ws[2 + FLAG_LIST:].abs().sum()) == 0, "live counter, overflow bitmap and ticket clean"
            o1, c1 = ops.den_conv3x3_mfma_fp6(ops.spikes_to_c4(sd), pk1, Cout, bn_a=ad, bn_b=bd, want_counts=True)
            s2, s1 = ops.s32_to_spikes(o2), ops.c4_to_spikes(o1)
            print("BORDER_SKIP_FLAGS " + json.dumps({"B": B, "Cout": Cout, "Cin": Cin, "case": name, "flagged": flagged,
                                                     "firing": round(float(s1.mean()), 6)}))
            assert torch.equal(s1, s2), (B, Cout, Cin, name, int((s1 != s2).sum()))
            assert torch.equal(c1, c2), (B, Cout, Cin, name)
            assert 0.0 < float(s1.mean()) < 1.0, "a case that fires nowhere or everywhere checks nothing"
            # the listed-position form on complete lists (old position order, all nine taps): the same records on positions 0 .. 48
            with ops.active_set(*act, need=need):
                o3, c3 = ops.den_conv3x3_mfma_fp6v2(s32, pk2, Cout, bn_a=ad, bn_b=bd, want_counts=True, need_radius=1)
            torch.cuda.synchronize()
            assert torch.equal(o3, o2) and torch.equal(c3, c2), (B, Cout, Cin, name, "listed form")
            assert int(ws[0]) == 0 and int(ws[2 + FLAG_LIST:].abs().sum()) == 0
