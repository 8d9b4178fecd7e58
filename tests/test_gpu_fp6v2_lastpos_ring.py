"""The LDS-shared last-position form of the dense tail launch (den_mfma_fp6v2.hip, fp6v2_lastpos_shared_body, "THE CHUNK PIPELINE"):
a workgroup of four waves takes eight images of one channel group; a chunk's thirteen weight tiles come in by LDS-DMA into one of two
buffers and its four spike fragments into one of two register sets, one chunk ahead, under the MFMAs of the chunk before; one wait and
one barrier per chunk.  What that can break -- a chunk read from the wrong buffer or before it is in, fragments of the wrong chunk,
the last chunk's clamped prefetch, a wave without an image -- at the smallest shapes that take the form (full batches of B >= 64
without a device-side count, Cin >= 64: tests/_image_count_cases.py restates the launcher's condition):

  B = 64, 65 (one image alone in its group of eight: three waves have no image), 71
  Cout = 32, 64 (one and two channel groups: the workgroup -> group map)
  Cin = 32 x nch, nch = 2, 3, 4, 5, 7, 16 (below, at and above every buffer count considered, odd and even, the denoiser's largest)

Inputs: random at the denoiser's ~5 % firing rate, every input active, none active, and ONE active cell (every image, last chunk) in
turn at the four cells that reach position 48 (40, 41, 47, 48) and at one that does not (39).  Weights: random (all six digits), and
one radix-32 digit of the six at a time -- the last position uses all six exactly.

Every case is compared BIT FOR BIT, spikes and counts, ALL 49 positions, with the six-plane kernel (spk_den_conv3x3_mfma_fp6); then
spk_den_conv3x3_mfma_fp6v2_part(part = 4) re-runs the NON-shared last-position form on the same workspace and output: the buffers
are the same byte for byte before and after.  Outputs start as a sentinel; the workspace is clean afterwards.  Per case a line
LASTPOS_RING_DIGEST {json} carries a digest of positions 0-47 (records and counts) and of the flag workspace (published count, sorted
ids), so that a run on another library (SPKDIFF_LIB) can be compared line by line.

On a library that reads a chunk from the other buffer all 46 cases fail; an explicit wait of vmcnt(5) in front of the barrier fails none
(the compiler's own wait for the fragment loads at the end of the step retires the copies too): profiles/lastpos_ring_ab.txt (5)."""
import hashlib
import json

import pytest
import torch

import _image_count_cases as ic

pytestmark = pytest.mark.gpu

FLAG_LIST = 1 << 20          # id-list entries of the workspace (FLAG_CAP): [count, published count, ids..., bitmap, ticket]
SENTINEL = 0x5A
BATCHES = (64, 65, 71)
COUTS = (32, 64)
NCHS = (2, 3, 4, 5, 7, 16)
LP_SIGNS = (1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0, 1.0, 1.0)      # taps 0, 1, 3, 4 reach position 48: three up, one down


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def layer_random(Cout, Cin, seed=0, fires_alone=False):
    """(w, bias, bn_a, bn_b).  fires_alone: BN offsets of 0.5 .. 2.5, so that part of the channels spike without any input."""
    g = torch.Generator().manual_seed(9100 + 7 * Cout + Cin + seed)
    w = (torch.rand(Cout, Cin, 3, 3, generator=g) - 0.5) * 0.05
    w[:, :, 1, 1] *= 3.0
    bias = (torch.rand(Cout, generator=g) - 0.5) * 0.2
    a = (torch.rand(Cout, generator=g) - 0.3) * 12.0                  # some negative BN scales
    b = (torch.rand(Cout, generator=g) - 0.4) * 1.5
    if fires_alone:
        b = 0.5 + 2.0 * torch.rand(Cout, generator=g)
    return w, bias, a, b


def layer_one_digit(Cout, Cin, j, rate):
    """Every weight of input channels 1.. is LP_SIGNS[tap] * d * 32^(5 - j) * 2^-29, d in 8 .. 15 by output channel: digit j of six alone.
    Input channel 0 carries one weight of 0.5 (digit 0 alone: the quantisation shift is 29) and never spikes.  BN scales the
    pre-activation of position 48 (rate x two taps net x (Cin - 1) inputs x d) to 1.5 .. 3; no bias."""
    d = 8.0 + (torch.arange(Cout) % 8).float()
    unit = float(32 ** (5 - j)) * 2.0 ** -29
    w = torch.tensor(LP_SIGNS).view(1, 1, 3, 3) * d.view(Cout, 1, 1, 1) * unit * torch.ones(Cout, Cin, 3, 3)
    w[:, 0] = 0.0
    w[:, 0, 1, 1] = 0.5
    est = rate * 2.0 * (Cin - 1) * d * unit
    a = (1.5 + 1.5 * ((torch.arange(Cout) * 5) % 7).float() / 6.0) / est
    return w, torch.zeros(Cout), a, torch.zeros(Cout)


def spikes_random(dev, B, Cin, rate, seed, silent0=False):
    g = torch.Generator(device=dev).manual_seed(9300 + seed)
    s = (torch.rand(16, B, Cin, 7, 7, generator=g, device=dev) < rate).float()
    if silent0:
        s[:, :, 0] = 0.0
    return s


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def _ws_clean(ws):
    return int(ws[0]) == 0 and int(ws[2 + FLAG_LIST:].abs().sum()) == 0


def _run(ops, dev, sd, layer, name):
    """One input [16, B, Cin, 7, 7] (on the device) through the dense call and the six-plane kernel; then part 4 on the same buffers.
    Returns the spikes of position 48 [16, B, Cout] and the number of flagged neurons."""
    from spkdiff._lib import lib
    _, B, Cin = sd.shape[:3]
    w, bias, a, b = layer
    Cout = w.shape[0]
    assert ic.fp6v2_tail(B, Cin, 7, False) == 3, "the shape takes the LDS-shared last-position form"
    wd, biasd, ad, bd = w.to(dev), bias.to(dev), a.to(dev), b.to(dev)
    # the six-plane kernel takes K chunks of 64 input channels and output channels by 64: its copy of the layer carries zero weights and
    # zero spikes in the padding (exact zeros in an exact sum, the same quantisation scale) and silent output channels, dropped below
    pad = -Cout % 64
    w1 = torch.cat([torch.cat([w, torch.zeros(Cout, -Cin % 64, 3, 3)], 1), torch.zeros(pad, Cin + -Cin % 64, 3, 3)], 0).to(dev)
    zp = torch.zeros(pad, device=dev)
    pk2, pk1 = ops.den_pack_weight_fp6v2(wd, biasd), ops.den_pack_weight_fp6(w1, torch.cat([biasd, zp]))
    ws = ops._flag_bitmap(dev, lib.spk_den_fp6v2_flag_words(B, Cout, 7, 7))
    s32 = ops.spikes_to_s32(sd)
    sd1 = torch.cat([sd, torch.zeros(16, B, -Cin % 64, 7, 7, device=dev)], 2) if Cin % 64 else sd
    o1, c1 = ops.den_conv3x3_mfma_fp6(ops.spikes_to_c4(sd1), pk1, Cout + pad, bn_a=torch.cat([ad, zp]), bn_b=torch.cat([bd, zp]),
                                      want_counts=True)
    s1, c1 = ops.c4_to_spikes(o1)[:, :, :Cout], c1[:, :Cout // 32]
    nch = Cin // 32
    wq, scale, bias_d, wl1, qtab = pk2
    out = ops.empty_spikes(ops.S32, B, Cout, 7, 7, 16, dev)
    out.view(torch.uint8).fill_(SENTINEL)
    cnt = torch.full((B, Cout // 32, 7, 7, 32), SENTINEL, dtype=torch.uint8, device=dev)
    head = (ops._p(s32), nch, ops._p(wq), ops._p(scale), ops._p(bias_d), ops._p(wl1), ops._p(qtab), ops._p(ad), ops._p(bd), ops._p(out),
            ops._p(cnt), ops._p(ws), 16, B, 7, 7, Cout, ops._n_dyn())
    ops.check(lib.spk_den_conv3x3_mfma_fp6v2(*head, int(ops.FLAG_CAP), int(ops.FP6V2_FORM), ops._stream(s32)), "spk_den_conv3x3_mfma_fp6v2")
    torch.cuda.synchronize()
    flagged = int(ws[1].item())
    ids = torch.sort(ws[2:2 + min(flagged, FLAG_LIST)]).values
    assert _ws_clean(ws), (name, "live counter, overflow bitmap and ticket clean")
    ob, cb = out.view(torch.uint8).reshape(B, Cout // 32, 49, -1), cnt.reshape(B, Cout // 32, 49, 32)
    line = {"B": B, "Cout": Cout, "Cin": Cin, "case": name, "flagged": flagged, "ids": _digest(ids),
            "pos0_47": _digest(ob[:, :, :48], cb[:, :, :48])}
    print("LASTPOS_RING_DIGEST " + json.dumps(line))
    s2 = ops.s32_to_spikes(out)
    p1, p2 = s1.flatten(3), s2.flatten(3)
    assert torch.equal(p1[..., 48], p2[..., 48]), (B, Cout, Cin, name, "position 48", int((p1[..., 48] != p2[..., 48]).sum()))
    assert torch.equal(c1.reshape(B, -1, 49, 32)[:, :, 48], cb[:, :, 48]), (B, Cout, Cin, name, "counts of position 48")
    assert torch.equal(s1, s2) and torch.equal(c1, cnt), (B, Cout, Cin, name, "positions 0-47", int((s1 != s2).sum()))
    # part 4: fp6v2_tail_kernel<7, 7, 2>, the last position of every image by the non-shared form, into the same buffers
    before_o, before_c = out.clone(), cnt.clone()
    ops.check(lib.spk_den_conv3x3_mfma_fp6v2_part(*head, 4, int(ops.FLAG_CAP), ops._stream(s32)), "spk_den_conv3x3_mfma_fp6v2_part")
    torch.cuda.synchronize()
    assert torch.equal(before_o.view(torch.uint8), out.view(torch.uint8)) and torch.equal(before_c, cnt), (B, Cout, Cin, name, "part 4 agrees")
    return p2[..., 48], flagged


@pytest.mark.parametrize("nch", NCHS)
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("B", BATCHES)
def test_lastpos_ring_random_inputs_every_shape(dev, ops, B, Cout, nch):
    Cin = 32 * nch
    p48, flagged = _run(ops, dev, spikes_random(dev, B, Cin, 0.05, 17 * B + nch), layer_random(Cout, Cin), "random05")
    assert flagged < B * Cout * 49, "some neuron is decided by the matrix-core path"
    assert 0.0 < float(p48.mean()) < 1.0, "a last position that fires nowhere or everywhere checks nothing"
    # every image of the batch, the single one of B = 65's last group too
    assert bool((p48.flatten(2).sum((0, 2)) > 0).all()), "every image fires somewhere at position 48"


@pytest.mark.parametrize("nch", NCHS)
def test_lastpos_ring_every_input_active_and_none(dev, ops, nch):
    Cin = 32 * nch
    layer = layer_random(64, Cin, seed=1, fires_alone=True)
    ones = _run(ops, dev, torch.ones(16, 65, Cin, 7, 7, device=dev), layer, "all")[0]
    zero = _run(ops, dev, torch.zeros(16, 65, Cin, 7, 7, device=dev), layer, "none")[0]
    assert 0.0 < float(ones.mean()) < 1.0 and 0.0 < float(zero.mean()) < 1.0
    assert not torch.equal(ones, zero)


@pytest.mark.parametrize("Cout", COUTS)
def test_lastpos_ring_one_active_cell(dev, ops, Cout):
    """Cells 40, 41, 47, 48 are taps 0, 1, 3, 4 of position 48; cell 39 (row 5, column 4) is not in its window: with spikes there and
    nowhere else position 48 answers as it does to no input at all."""
    B, nch = 65, 3
    Cin = 32 * nch
    layer = layer_random(Cout, Cin, seed=2, fires_alone=True)
    zero = _run(ops, dev, torch.zeros(16, B, Cin, 7, 7, device=dev), layer, "none")[0]
    assert 0.0 < float(zero.mean()) < 1.0
    seen = []
    for cell in (40, 41, 47, 48, 39):
        s = torch.zeros(16, B, Cin, 49, device=dev)
        s[:, :, Cin - 32:, cell] = spikes_random(dev, B, 32, 0.5, cell)[..., 0, 0]        # the last chunk alone
        p48 = _run(ops, dev, s.view(16, B, Cin, 7, 7), layer, f"cell{cell}")[0]
        if cell == 39:
            assert torch.equal(p48, zero), "cell 39 does not reach position 48"
        else:
            assert not torch.equal(p48, zero), (cell, "reaches position 48")
            assert all(not torch.equal(p48, q) for q in seen), (cell, "its own tap")
            seen.append(p48)


@pytest.mark.parametrize("B,Cout,nch", [(65, 32, 5), (64, 64, 2)])
def test_lastpos_ring_one_digit_at_a_time(dev, ops, B, Cout, nch):
    Cin = 32 * nch
    s = spikes_random(dev, B, Cin, 0.30, 500 + nch, silent0=True)
    for j in range(6):
        p48 = _run(ops, dev, s, layer_one_digit(Cout, Cin, j, 0.30), f"digit{j}")[0]
        assert 0.0 < float(p48.mean()) < 1.0, (j, "the digit decides spikes at position 48")
