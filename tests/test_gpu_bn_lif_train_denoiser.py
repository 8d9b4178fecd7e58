"""Training BatchNorm + LIF (csrc/bn_lif_train.hip through ops.BNLIFTrainFunction(..., want_c4=True)) at the DENOISER's block
tails: C = 64, 128, 256, 512, 256 on 7x7 or 8x8 maps at the reference's batch of 32, channels-last memory as the library's
convolutions leave it, and the sizes around them at which the vector kernels change behaviour: the forward and
the second backward pass walk 1024 / C rows per workgroup step and wrap their row loop past R = B * HW = 2^20 / C, the BPTT
pass 512 / C rows and wraps past 2^19 / C -- at C = 512 already at batch 32, with ONE row per step.  tests/
test_gpu_bn_lif_train_shapes.py has the VQ-VAE's shapes (C <= 64), where none of this happens.

Every case is held against independent statements of the operator (tests/_bn_lif_train_oracle.py, checked on the CPU by
tests/test_bn_lif_train_oracle_host.py):

  statistics   save_mean / save_invstd / running statistics against fp64;
  forward      spikes and v_last BIT-EQUAL to the fp32 restatement of the apply launch from the kernel's own statistics, over every
               neuron-step, nothing exempt; and, as a cross-check of the restatement, equal to the fp64 oracle's own decisions
               outside the fragile set (within 1e-5 of the threshold; fewer than 1e-4 of the neuron-steps);
  C4 records   bytewise the records built on the host from the restatement's spikes;
  backward     grad_y element-wise over ALL neurons, grad_gamma, grad_beta and grad_v_init against the fp64 autograd oracle that
               is given the kernel's spike decisions (so its trajectory is the kernel's at every neuron and nothing is left out);
  repeat run   bit-identical outputs and gradients (fixed-order reductions);
  workspace    spk_bn_lif_train_ws_bytes covers the largest slice count any launch of the case uses."""
import pytest
import torch

import _bn_lif_train_oracle as O
from parity_report import record as parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


# (T, B, C, H, v_init, detach_reset, strided gradient (pitch channels, offset, broadcast over T) or None, through the C-ABI misaligned)
CASES = [
    # the reference batch: every block tail.  C = 512 on 7x7: R = 1568, the BPTT pass wraps with one row per step; on 8x8:
    # R = 2048, the BPTT pass wraps exactly twice and the forward sits on the cap without wrapping
    (16, 32, 64, 7, False, False, None, False), (16, 32, 128, 7, False, False, None, False),
    (16, 32, 256, 7, False, False, None, False), (16, 32, 512, 7, False, False, None, False),
    (16, 32, 512, 8, False, False, None, False),
    # the forward wraps: R just above 2^20 / C (a short second trip); the BPTT pass is on its third trip
    (16, 335, 64, 7, False, False, None, False), (16, 168, 128, 7, False, False, None, False),
    (16, 84, 256, 7, False, False, None, False), (16, 33, 512, 8, False, False, None, False),
    # carried state in the wrapped loops
    (16, 32, 512, 7, True, False, None, False), (16, 84, 256, 7, False, True, None, False),
    # short T: the t < T guards and the record stride T * 32 of the C4 output
    (5, 4, 256, 7, False, False, None, False),
    # the BPTT pass takes the scalar kernel (C / 2 > 256), the forward and the second pass stay 4-wide: the finalize launch
    # has to read the scalar pass's slice count
    (16, 3, 1024, 7, False, False, None, False),
    # the gradient read in place: conv5's tail (broadcast over T, a slice of cat(x5, x1)'s 320 channels), conv1's half of the
    # same tensor, and a dense-over-T channel slice
    (16, 32, 256, 7, False, False, (320, 0, True), False), (16, 32, 64, 7, False, False, (320, 256, True), False),
    (16, 5, 128, 8, False, False, (192, 64, False), False),
    # every launch in its scalar form at a C the vector forms normally serve: tensors one float off a 16-byte boundary
    (16, 5, 128, 7, False, False, None, True),
]


def _id(case):
    T, B, C, H, with_v, det, strided, mis = case
    return (f"T{T}_B{B}_C{C}_{H}x{H}" + ("_v" if with_v else "") + ("_det" if det else "") +
            (f"_pitch{strided[0]}_off{strided[1]}" + ("_bcast" if strided[2] else "_dense") if strided else "") +
            ("_misaligned" if mis else ""))


def _channels_last(x):
    n = x.dim()
    return x.permute(*range(n - 3), n - 2, n - 1, n - 3).contiguous().permute(*range(n - 3), n - 1, n - 3, n - 2)


def _run_wrapper(ops, y, gamma, beta, rm, rv, v0, gs, gv, det):
    """_bn_lif_train_oracle._run_hip's tuple + the C4 records, with want_c4=True and the gradient of the spikes handed to autograd as
    the tensor `gs` itself (so a strided `gs` reaches the backward with its strides)."""
    yd, gd, bd = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    vd = None if v0 is None else v0.clone().requires_grad_(True)
    rmd, rvd = rm.clone(), rv.clone()
    assert yd.stride() == y.stride()
    s, vl, c4 = ops.BNLIFTrainFunction.apply(yd, gd, bd, vd, rmd, rvd, 0.1, 1e-5, 2.0, 1.0, 0.0, 2.0, det, True)
    mean, invstd = s.grad_fn.saved_tensors[3:5]
    torch.autograd.backward([s] + ([vl] if gv is not None else []), [gs] + ([gv] if gv is not None else []))
    torch.cuda.synchronize()
    return (s.detach(), vl.detach(), mean.clone(), invstd.clone(), rmd, rvd, yd.grad, gd.grad, bd.grad,
            None if vd is None else vd.grad, c4)


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bn_lif_train_at_the_denoiser_shapes(dev, ops, case):
    T, B, C, H, with_v, det, strided, mis = case
    HW, R = H * H, B * H * H
    seed = B * 1000 + C * 10 + H + 3 * with_v + 7 * det + 11 * T + (strided[1] + 13 if strided else 0) + 17 * mis
    y, gamma, beta, rm, rv, v0, gs, gv = O._inputs(dev, B, C, H, with_v, seed, T=T)
    y, gs = _channels_last(y), _channels_last(gs)
    v0, gv = (None, None) if not with_v else (_channels_last(v0), _channels_last(gv))
    want_strides = (R * C, C)
    if strided:
        pitch, offset, bcast = strided
        gs = O.strided_grad(B, C, H, H, T, pitch, offset, bcast, torch.Generator(device=dev).manual_seed(seed + 1))
        want_strides = (0 if bcast else R * pitch, pitch)
    inp = (y, gamma, beta, rm, rv, v0, gs, gv)

    # the workspace covers every launch of the case (the wrapped C = 512 BPTT pass, 1 024 slices, is the binding one)
    geo = O.slice_counts(R, C, aligned=not mis)
    ws_bytes = int(ops.lib.spk_bn_lif_train_ws_bytes(B, C, HW))
    assert ws_bytes >= C * max(geo["fwd"], geo["bptt"]) * 16, (ws_bytes, geo)

    if mis:
        a = O.run_cabi_misaligned(ops, *inp, det)
        b = O.run_cabi_misaligned(ops, *inp, det)
        for x in (a, b):
            assert x[10] == -2 and x[11], "spk_bn_lif_train_fwd_c4 on misaligned tensors: SPK_ERR_UNSUPPORTED, nothing launched"
        a, b = a[:10] + (None,), b[:10] + (None,)
    else:
        seen = []
        orig = ops.lib.spk_bn_lif_train_bwd_strided

        def spy(grad_s, step_stride, row_pitch, *rest):
            seen.append((int(step_stride), int(row_pitch)))
            return orig(grad_s, step_stride, row_pitch, *rest)

        ops.lib.spk_bn_lif_train_bwd_strided = spy
        try:
            a = _run_wrapper(ops, *inp, det)
            b = _run_wrapper(ops, *inp, det)
        finally:
            ops.lib.spk_bn_lif_train_bwd_strided = orig
        # a strided gradient was read where autograd left it (a silent expanded copy would arrive as (R * C, C))
        assert seen == [want_strides, want_strides], (seen, want_strides)
        assert a[10] is not None and a[10].shape == (B, C // 64, H, H, T, 32), "C4 records come with every denoiser shape"
    s, vl, mean, invstd, rmo_k, rvo_k, gy, gg, gb, gv0, c4 = a

    # ---- repeat run
    for x, x2 in zip(a, b):
        assert (x is None and x2 is None) or torch.equal(x, x2)

    # ---- forward, exact: the fp32 restatement from the kernel's own statistics
    s32, v32, _ = O.restate_fwd32(y, gamma, beta, mean, invstd, v0)
    steps = s32.numel()
    fwd_mism = int((_bits(s) != _bits(s32)).sum())
    v_mism = int((_bits(vl) != _bits(v32)).sum())
    c4_mism = -1 if c4 is None else int((c4.view(torch.uint8).cpu() != O.c4_records(s32)).sum())

    # ---- fp64: statistics, the oracle's own decisions, gradients on the kernel's trajectory
    own, _, mean_o, invstd_o, rmo, rvo, gyo, ggo, gbo, gv0o, frag = O.oracle_given(y, gamma, beta, rm, rv, v0, gs.contiguous(),
                                                                                   gv, det, s)
    nfrag = int(frag.sum())
    mism_out = int((s.double() != own)[~frag].sum())
    e = dict(
        save_mean=float((mean.double() - mean_o).abs().max()), save_invstd=float((invstd.double() - invstd_o).abs().max()),
        running_mean=float((rmo_k.double() - rmo).abs().max()), running_var=float((rvo_k.double() - rvo).abs().max()),
        grad_y_max_abs=float((gy.double() - gyo).abs().max()), grad_y_scale=1 + float(gyo.abs().max()),
        grad_y_rel_l2=O._rel_l2(gy, gyo), grad_gamma=O._rel_l2(gg, ggo), grad_beta=O._rel_l2(gb, gbo),
        grad_v_init=O._rel_l2(gv0, gv0o) if with_v else 0.0)
    parity("bn_lif_train_den_" + _id(case), neuron_steps=steps, firing_rate=float(s32.mean()), forward_mismatches=fwd_mism,
           v_last_mismatches=v_mism, c4_byte_mismatches=c4_mism, fragile=nfrag, spike_mismatches_outside_fragile=mism_out,
           slices_fwd=geo["fwd"], slices_bptt=geo["bptt"], ws_bytes=ws_bytes, **e)

    assert fwd_mism == 0 and v_mism == 0, (fwd_mism, v_mism)
    assert mis or c4_mism == 0, c4_mism
    assert nfrag < 1e-4 * steps, (nfrag, steps)
    assert mism_out == 0
    assert e["running_mean"] <= 1e-6 and e["save_mean"] <= 1e-6, e
    assert e["running_var"] <= 1e-5 and e["save_invstd"] <= 1e-5, e
    assert e["grad_y_max_abs"] <= 1e-5 * e["grad_y_scale"] and e["grad_y_rel_l2"] <= 2e-5, e
    assert max(e["grad_gamma"], e["grad_beta"], e["grad_v_init"]) <= 2e-5, e
    assert float(gyo.abs().max()) > 0 and gy.shape == y.shape
    if with_v:
        assert gv0 is not None and gv0.shape == (B, C, H, H)
