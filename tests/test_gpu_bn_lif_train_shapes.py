"""Training BatchNorm + LIF (csrc/bn_lif_train.hip through ops.BNLIFTrainFunction) at the VQ-VAE's training shapes: T = 16 steps,
B = 32 images (R/main.py:67,133), every block tail of the MNIST and the CIFAR-shaped model, and 32@28x28 at B = 64.  These are
the sizes where the row-slice loops of the vector kernels wrap (the BPTT pass from 1 024 row groups on, the forward past B = 41
on 28x28), which the small shapes of tests/test_gpu_parity.py never reach.

The oracle runs in fp64 on the device: F.batch_norm(training=True) followed by the per-step arithmetic of
oracle.snn_ref.lif_multi_step_train (charge v + (z - v) / tau, ATan surrogate spike, hard reset), with momentum 0.1, eps 1e-5,
tau 2, alpha 2.  At a neuron-step within 1e-5 of the threshold (the fragile set) the fp32 kernel and the fp64 oracle may
decide the spike differently; the oracle then takes the kernel's decision, so the steps that follow stay comparable and no
gradient check is skipped because such a step exists somewhere in the batch."""
import pytest
import torch

from _bn_lif_train_oracle import _inputs, _oracle, _rel_l2, _run_hip
from parity_report import record as parity

pytestmark = pytest.mark.gpu

T = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


# (B, C, H, v_init, detach_reset)
SHAPES = [
    (32, 32, 14, False, False), (32, 64, 7, False, False), (32, 16, 7, False, False), (32, 64, 14, False, False),
    (32, 32, 28, False, False),                                         # MNIST: enc1, enc2, enc3 / spike generator, dec1, dec2
    (32, 32, 16, False, False), (32, 64, 8, False, False), (32, 16, 8, False, False), (32, 64, 16, False, False),
    (32, 32, 32, False, False),                                         # CIFAR-shaped model
    (64, 32, 28, False, False),                                         # the forward's row slices wrap as well
    (32, 64, 14, True, False),                                          # a carried membrane state (and its gradient)
    (32, 32, 16, False, True),                                          # detach_reset
]


@pytest.mark.parametrize("B,C,H,with_v,det", SHAPES, ids=lambda v: str(int(v)))
def test_bn_lif_train_at_the_training_shapes_vs_fp64(dev, ops, B, C, H, with_v, det):
    """Spikes equal outside the fragile set (fewer than 1e-4 of the neuron-steps), the batch and running statistics to fp32
    round-off, grad_y element-wise at every neuron whose 16 steps hold no fragile value, grad_gamma / grad_beta / grad_v_init
    within 2e-5 relative L2."""
    inp = _inputs(dev, B, C, H, with_v, seed=B * 1000 + C * 10 + H + 3 * with_v + 7 * det)
    s, vl, mean, invstd, rm, rv, gy, gg, gb, gv0 = _run_hip(ops, *inp, det)
    so, vlo, mean_o, invstd_o, rmo, rvo, gyo, ggo, gbo, gv0o, frag = _oracle(*inp, det, s)
    steps = frag.numel()
    nfrag = int(frag.sum())
    clean = ~frag.any(dim=0)                                                     # [B, C, H, W]: neurons with no fragile step
    clean_cl = clean.unsqueeze(0).expand_as(frag)
    mism = int((s.double() != so)[~frag].sum())
    e = dict(
        v_last=float((vl.double() - vlo).abs().max()),
        save_mean=float((mean.double() - mean_o).abs().max()), save_invstd=float((invstd.double() - invstd_o).abs().max()),
        running_mean=float((rm.double() - rmo).abs().max()), running_var=float((rv.double() - rvo).abs().max()),
        grad_y_max_abs=float((gy.double() - gyo)[clean_cl].abs().max()), grad_y_scale=1 + float(gyo[clean_cl].abs().max()),
        grad_y_rel_l2=_rel_l2(gy[clean_cl], gyo[clean_cl]), grad_gamma=_rel_l2(gg, ggo), grad_beta=_rel_l2(gb, gbo),
        grad_v_init=_rel_l2(gv0, gv0o) if with_v else 0.0)
    parity(f"bn_lif_train_T{T}_B{B}_C{C}_{H}x{H}" + ("_v" if with_v else "") + ("_det" if det else ""), neuron_steps=steps,
           fragile=nfrag, spike_mismatches_outside_fragile=mism, **e)
    assert nfrag < 1e-4 * steps, (nfrag, steps)
    assert mism == 0
    assert e["v_last"] <= 1e-5
    assert e["running_mean"] <= 1e-6 and e["save_mean"] <= 1e-6, e
    assert e["running_var"] <= 1e-5 and e["save_invstd"] <= 1e-5, e
    assert e["grad_y_max_abs"] <= 1e-5 * e["grad_y_scale"] and e["grad_y_rel_l2"] <= 2e-5, e
    assert max(e["grad_gamma"], e["grad_beta"], e["grad_v_init"]) <= 2e-5, e
    if with_v:
        assert gv0 is not None and gv0.shape == (B, C, H, H)


@pytest.mark.parametrize("B,C,H,with_v,det", [(32, 32, 28, False, False), (64, 32, 28, False, True), (32, 64, 14, True, False)],
                         ids=lambda v: str(int(v)))
def test_bn_lif_train_is_bit_reproducible_at_the_training_shapes(dev, ops, B, C, H, with_v, det):
    """Fixed-order partial sums: two runs give bit-identical spikes, v_last, statistics and gradients."""
    inp = _inputs(dev, B, C, H, with_v, seed=B + C + H)
    a, b = _run_hip(ops, *inp, det), _run_hip(ops, *inp, det)
    for x, x2 in zip(a, b):
        assert (x is None and x2 is None) or torch.equal(x, x2)
