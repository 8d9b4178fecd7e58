"""tests/_bn_lif_train_oracle.py checked on the CPU, with nothing of the library, before tests/test_gpu_bn_lif_train_denoiser.py
trusts it: the fp32 restatement of the forward against the free-running fp64 oracle, the given-decisions oracle against the
existing one, the C4 builder against its reader, the strided gradient against the tensor it was cut from, the slice counts
against DESIGN.md §4.5, and -- at a full-size case -- that the input distribution of the GPU tests keeps the fragile share
(neuron-steps within 1e-5 of the threshold) far below the 1e-4 cap those tests assert."""
import numpy as np
import pytest
import torch

import _bn_lif_train_oracle as O
from _conv_bn_lif_oracle import packed_to_spikes
from parity_report import record as parity

CPU = torch.device("cpu")
# (T, B, C, H, v_init, detach_reset)
SMALL = [(16, 3, 128, 7, False, False), (5, 2, 64, 8, False, False), (16, 2, 64, 7, True, False), (5, 3, 128, 8, True, True)]


def _case(T, B, C, H, with_v, seed):
    return O._inputs(CPU, B, C, H, with_v, seed, T=T)


def _restate_from_fp64_stats(inp, free):
    y, gamma, beta, _, _, v0 = inp[:6]
    return O.restate_fwd32(y, gamma, beta, free[2].float(), free[3].float(), v0)


@pytest.mark.parametrize("T,B,C,H,with_v,det", SMALL, ids=lambda v: str(int(v)))
def test_fp32_restatement_is_the_free_running_oracle_outside_the_fragile_set(T, B, C, H, with_v, det):
    inp = _case(T, B, C, H, with_v, seed=11 + C + H + T)
    free = O.oracle_given(*inp, det, None)
    s32, v32, h32 = _restate_from_fp64_stats(inp, free)
    own, v64, frag = free[0], free[1], free[10]
    assert s32.shape == own.shape == h32.shape == (T, B, C, H, H) and v32.shape == (B, C, H, H)
    assert set(np.unique(s32.numpy())) <= {0.0, 1.0} and 0.01 < float(s32.mean()) < 0.5
    assert int((s32.double() != own)[~frag].sum()) == 0
    clean = ~frag.any(dim=0)                                                           # neurons with no fragile step
    assert float((v32.double() - v64)[clean].abs().max()) <= 1e-5 and int(clean.sum()) > 0.99 * clean.numel()
    # h_t is the charge of step t: recomputing the spikes and the state from it gives the restatement's own outputs
    assert torch.equal((h32 - 1.0 >= 0).float(), s32) and torch.equal(((1 - s32[-1]) * h32[-1]), v32)


@pytest.mark.parametrize("T,B,C,H,with_v,det", SMALL, ids=lambda v: str(int(v)))
def test_given_decisions_oracle_reproduces_the_existing_oracle_on_its_own_spikes(T, B, C, H, with_v, det):
    inp = _case(T, B, C, H, with_v, seed=5 + C + H + T)
    free = O.oracle_given(*inp, det, None)
    given = O.oracle_given(*inp, det, free[0])
    old = O._oracle(*inp, det, free[0].float())
    assert torch.equal(given[0], free[0]) and torch.equal(old[0], free[0]) and torch.equal(given[10], old[10])
    for i in (1, 2, 3, 4, 5, 6, 7, 8, 9):
        if old[i] is None:
            assert given[i] is None and not with_v
            continue
        assert O._rel_l2(given[i], old[i]) <= 1e-12 and O._rel_l2(free[i], old[i]) <= 1e-12, i
    assert float(old[6].abs().max()) > 0


def test_given_decisions_oracle_takes_the_value_and_keeps_the_surrogate():
    """With every spike forced to 0 the state never resets: v_last is the plain leaky integration of z, and grad_y is non-zero
    although no spike depends on y in value (the ATan surrogate carries it)."""
    T, B, C, H = 5, 2, 64, 8
    inp = _case(T, B, C, H, False, seed=3)
    zeros = torch.zeros(T, B, C, H, H)
    out = O.oracle_given(*inp, False, zeros)
    y, gamma, beta = (t.double() for t in inp[:3])
    z = (y - out[2].view(1, 1, C, 1, 1)) * out[3].view(1, 1, C, 1, 1) * gamma.view(1, 1, C, 1, 1) + beta.view(1, 1, C, 1, 1)
    v = torch.zeros(B, C, H, H, dtype=torch.float64)
    for t in range(T):
        v = v + (z[t] - v) / 2.0
    assert float((out[1] - v).abs().max()) <= 1e-12
    assert float(out[6].abs().max()) > 0 and bool(out[0].any()), "own decisions are still reported"


@pytest.mark.parametrize("T,B,C,H", [(16, 3, 128, 7), (5, 2, 64, 8), (5, 2, 256, 7)])
def test_c4_builder_round_trips(T, B, C, H):
    g = torch.Generator().manual_seed(T + C)
    s = (torch.rand(T, B, C, H, H, generator=g) < 0.2).float()
    rec = O.c4_records(s)
    assert rec.dtype == torch.uint8 and rec.shape == (B, C // 64, H, H, T, 32)
    assert torch.equal(packed_to_spikes(rec), s)
    # one spike alone: channel c of image b at (h, w), step t sits in record c // 64, byte (c % 64) // 2, low nibble for even c
    one = torch.zeros(T, B, C, H, H)
    t, b, c, h, w = T - 1, B - 1, C - 63, H - 2, 1
    one[t, b, c, h, w] = 1.0
    rec = O.c4_records(one)
    assert int(rec[b, c // 64, h, w, t, (c % 64) // 2]) == (0x20 if c % 2 else 0x02) and int(rec.count_nonzero()) == 1


@pytest.mark.parametrize("B,C,H,T,pitch,offset,broadcast", [(3, 64, 7, 16, 320, 256, True), (2, 128, 8, 5, 192, 64, False),
                                                            (2, 256, 7, 16, 320, 0, True)])
def test_strided_gradient_is_the_slice_it_was_cut_from(B, C, H, T, pitch, offset, broadcast):
    gs = O.strided_grad(B, C, H, H, T, pitch, offset, broadcast, torch.Generator().manual_seed(9))
    shape = (B, pitch, H, H) if broadcast else (T, B, pitch, H, H)
    wide = torch.randn(shape, generator=torch.Generator().manual_seed(9))              # the same draw, in plain NCHW memory
    want = wide[:, offset:offset + C].unsqueeze(0).expand(T, B, C, H, H) if broadcast else wide[:, :, offset:offset + C]
    assert gs.shape == (T, B, C, H, H) and torch.equal(gs.contiguous(), want.contiguous())
    # the layout the wrapper's in-place path asks for: channels fastest, row pitch = the wide tensor's channels, step stride 0 or a
    # whole wide step
    assert gs.stride()[1:] == (H * H * pitch, 1, H * pitch, pitch)
    assert gs.stride(0) == (0 if broadcast else B * H * H * pitch)
    assert gs.storage_offset() == offset and not gs.is_contiguous()


def test_slice_counts_are_the_documented_geometry():
    """The geometry of DESIGN.md §4.5: at the reference batch C = 512 on 7x7 wraps the BPTT pass with one row per step while the
    forward does not wrap; on 8x8 the BPTT pass wraps exactly twice and the forward sits on the cap; C = 1024 leaves the BPTT
    pass to the scalar form."""
    g = O.slice_counts(32 * 49, 512)
    assert g == dict(fwd=784, bptt=1024, vec_fwd=4, vec_bptt=2, wraps_fwd=False, wraps_bptt=True)
    g = O.slice_counts(32 * 64, 512)
    assert (g["fwd"], g["bptt"], g["wraps_fwd"], g["wraps_bptt"]) == (1024, 1024, False, True) and 32 * 64 == 2 * 1024
    for B, C, H in ((335, 64, 7), (168, 128, 7), (84, 256, 7), (33, 512, 8)):
        R, rows = B * H * H, 1024 // C
        g = O.slice_counts(R, C)
        assert g["wraps_fwd"] and g["wraps_bptt"] and g["fwd"] == g["bptt"] == 1024
        assert (2 ** 20) // C < R < (2 ** 20) // C + 1024 and R % (1024 * rows) != 0, "just past the cap: a short second trip"
        assert 2 < R / (1024 * (512 // C)) <= 3, "the BPTT pass is on its third trip"
    g = O.slice_counts(3 * 49, 1024)
    assert g == dict(fwd=147, bptt=37, vec_fwd=4, vec_bptt=1, wraps_fwd=False, wraps_bptt=False)
    g = O.slice_counts(5 * 49, 128, aligned=False)
    assert (g["fwd"], g["bptt"], g["vec_fwd"], g["vec_bptt"]) == (62, 62, 1, 1)


def test_fragile_share_at_full_size_stays_far_below_the_cap():
    """(T, B, C, H) = (16, 8, 512, 7) with the GPU tests' input distribution (randn * 2 + 0.3, gamma = 1 + 0.3 randn,
    beta = 0.5 randn): the share of neuron-steps within 1e-5 of the threshold is of the order of 1e-5 (the density of h at the
    threshold times the 2e-5 window), an order below the 1e-4 cap, and outside that set the fp32 restatement decides every spike
    as the fp64 oracle does."""
    T, B, C, H = 16, 8, 512, 7
    inp = _case(T, B, C, H, False, seed=8512)
    free = O.oracle_given(*inp, False, None)
    s32, v32, _ = _restate_from_fp64_stats(inp, free)
    frag = free[10]
    steps, nfrag = frag.numel(), int(frag.sum())
    mism = int((s32.double() != free[0])[~frag].sum())
    clean = ~frag.any(dim=0)
    v_err = float((v32.double() - free[1])[clean].abs().max())
    parity("bn_lif_train_host_T16_B8_C512_7x7", neuron_steps=steps, fragile=nfrag, firing_rate=float(s32.mean()),
           spike_mismatches_outside_fragile=mism, v_last=v_err)
    assert steps == 3211264 and nfrag < 1e-4 * steps, (nfrag, steps)
    assert mism == 0 and v_err <= 1e-5
