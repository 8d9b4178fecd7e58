"""CPU tests of the VQ oracle (oracle/snn_ref.py, "VQ kernels" section) that tests/test_gpu_vq_shapes.py holds csrc/vq.hip and
csrc/vq_train.hip to: its code search reproduces fixture F3's indices (captured from the real reference), its training algebra
is fp64 autograd of the reference's lines (R/snn_model/vae_model.py:61-84), and its NaN / inf / tie behaviour is
torch.argmin's."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import snn_ref as ref
from spkdiff import synth

NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("tag,cfg", [("mnist", synth.MNIST), ("cifar", synth.CIFAR)])
def test_vq_argmin_f64_reproduces_f3_indices(golden_dir, tag, cfg):
    d = np.load(os.path.join(golden_dir, f"f3_encode_{tag}.npz"), allow_pickle=False)
    sd = synth.synth_vqvae_state(cfg)
    x = torch.from_numpy(d["images"]).unsqueeze(0).repeat(16, 1, 1, 1, 1)
    z = ref.encoder_forward(x, sd)
    cb = sd["vq_layer.embeddings.weight"]
    want = torch.from_numpy(d["indices"]).flatten()
    flat, _ = ref.vq_readout(z, sd)
    assert torch.equal(ref.vq_argmin_f64(flat, cb), want)
    # the kernels' read-out order (t ascending, [B, h, w, T, D] spikes) gives the same indices
    flat32 = ref.vq_readout_f32(z.permute(1, 3, 4, 0, 2), sd["vq_layer.memout.coef"], sd["vq_layer.alpha"])
    assert torch.equal(ref.vq_argmin_f64(flat32, cb), want)
    assert torch.equal(ref.vq_argmin_f64(flat32, cb, chunk=7), want)


def test_vq_train_f64_is_fp64_autograd_of_the_reference_lines():
    """Dyadic coefficients and alpha make the fp32 read-out exact, so the oracle and fp64 autograd see the same x_m."""
    g = torch.Generator().manual_seed(11)
    T, B, D, h, w, K, beta = 8, 3, 5, 3, 2, 9, 0.25
    x = (torch.rand(T, B, D, h, w, generator=g) < 0.4).float()
    coef = torch.pow(0.5, torch.arange(T - 1, -1, -1).float())
    alpha = torch.tensor(0.375)
    E0 = torch.randn(K, D, generator=g)
    g_out = torch.randn(B, D, h, w, generator=g)
    g_loss = 1.7
    o = ref.vq_train_f64(x, coef, alpha, E0, beta, g_out, g_loss)

    xs = x.double().requires_grad_(True)
    a = alpha.double().requires_grad_(True)
    E = E0.double().requires_grad_(True)
    x_memout = (1 - a) * torch.sum(xs * coef.double().view(T, 1, 1, 1, 1), dim=0) + a * torch.sum(xs, dim=0) / T
    x_memout = x_memout.permute(0, 2, 3, 1).contiguous()
    flat_x = x_memout.reshape(-1, D)
    idx = torch.argmin(ref.vq_distances(flat_x.detach(), E.detach()), dim=1)
    quantized = F.embedding(idx, E).view_as(x_memout)
    loss = F.mse_loss(quantized, x_memout.detach()) + beta * F.mse_loss(x_memout, quantized.detach())
    q = (x_memout + (quantized - x_memout).detach()).permute(0, 3, 1, 2).contiguous()
    gx, ga, gE = torch.autograd.grad((q, loss), (xs, a, E), (g_out.double(), torch.tensor(g_loss, dtype=torch.float64)))

    assert torch.equal(o["xm"].double(), flat_x.detach())
    assert torch.equal(o["idx"], idx)
    assert idx.unique().numel() > 2
    assert torch.allclose(o["q"], q.detach(), rtol=1e-12, atol=0)
    assert abs(float(o["loss"]) - float(loss.detach())) <= 1e-12 * float(loss.detach())
    assert torch.allclose(o["g_x"], gx, rtol=1e-12, atol=1e-15)
    assert abs(float(o["g_alpha"]) - float(ga)) <= 1e-12 * abs(float(ga))
    assert torch.allclose(o["g_E"], gE, rtol=1e-12, atol=1e-15)
    assert bool((o["g_E"][torch.bincount(idx, minlength=K) == 0] == 0).all())


def test_psp_and_recon_loss_f64_are_the_reference_lines():
    g = torch.Generator().manual_seed(5)
    T = 6
    qs = (torch.rand(T, 2, 3, 4, generator=g) < 0.3).float()
    xs = (torch.rand(T, 2, 3, 4, generator=g) < 0.3).float()
    loss, gq, gx = ref.psp_loss_f64(qs, xs, 0.25, 3.0, 2.0)
    q, x = qs.double().requires_grad_(True), xs.double().requires_grad_(True)
    pq, px = ref.psp_filter(q, 3.0), ref.psp_filter(x, 3.0)
    want = torch.mean((pq - px.detach()) ** 2) + 0.25 * torch.mean((pq.detach() - px) ** 2)
    (2.0 * want).backward()
    assert abs(float(loss) - float(want.detach())) <= 1e-15 * float(want.detach())
    assert torch.allclose(gq, q.grad, rtol=1e-13, atol=0) and torch.allclose(gx, x.grad, rtol=1e-13, atol=0)
    assert float(gq.abs().max()) > 0 and float(gx.abs().max()) > 0

    y0 = torch.randn(T, 2, 1, 5, 3, generator=g)
    img = torch.rand(2, 1, 5, 3, generator=g) - 0.5
    coef = ref.memout_coef(T).flatten()
    loss, gy = ref.recon_loss_f64(y0, coef, img, 1.5)
    y = y0.double().requires_grad_(True)
    want = F.mse_loss(torch.tanh(ref.membrane_output(y, ref.memout_coef(T).double())), img.double())
    (1.5 * want).backward()
    assert abs(float(loss) - float(want.detach())) <= 1e-14 * float(want.detach())
    assert torch.allclose(gy, y.grad, rtol=1e-12, atol=0)


def test_vq_argmin_f64_nan_inf_and_ties_are_torch_argmin():
    """NaN is the minimum and the first NaN wins; ties go to the lowest index; every index is in [0, K)."""
    g = torch.Generator().manual_seed(2)
    K, D = 70, 4
    cb = torch.randn(K, D, generator=g)
    cb[66] = cb[2]                                      # a tie across one lane (k, k + 64)
    x = torch.randn(8, D, generator=g)
    x[1] = NAN                                          # all-NaN row
    x[2, 3] = NAN                                       # one NaN component: every distance NaN
    x[3] = cb[2]                                        # exactly on the tied pair
    x[4] = INF
    got = ref.vq_argmin_f64(x, cb)
    assert torch.equal(got, torch.argmin(ref.vq_distances_f64(x, cb), dim=1))
    assert int(got[1]) == 0 and int(got[2]) == 0 and int(got[3]) == 2
    assert bool(((got >= 0) & (got < K)).all())
    # a NaN code row: every distance to it is NaN, so it is every row's code (the first NaN)
    cbn = cb.clone()
    cbn[5, 1] = NAN
    assert torch.equal(ref.vq_argmin_f64(x[[0, 3, 5, 6, 7]], cbn), torch.full((5,), 5))
    # an inf code row before it: rows whose distance to the inf row is NaN take it, the others the NaN row
    cbi = cbn.clone()
    cbi[3] = torch.tensor([INF, -INF, INF, 0.0])
    xi = torch.tensor([[1.0, -1.0, 1.0, 0.5], [-1.0, 1.0, -1.0, 0.5], [0.0, 0.0, 0.0, 0.0]])
    d3 = ref.vq_distances_f64(xi, cbi)[:, 3]
    assert torch.equal(ref.vq_argmin_f64(xi, cbi), torch.where(torch.isnan(d3), 3, 5))
    assert bool(torch.isnan(d3).any()) and not bool(torch.isnan(d3).all())
    # every distance +inf (x = -inf against a positive codebook): none is below another, index 0
    pos = cb.abs() + 0.1
    assert torch.equal(ref.vq_distances_f64(-INF * torch.ones(2, D), pos), torch.full((2, K), INF, dtype=torch.float64))
    assert torch.equal(ref.vq_argmin_f64(-INF * torch.ones(2, D), pos), torch.zeros(2, dtype=torch.int64))
    # an all-equal codebook: index 0 everywhere
    assert torch.equal(ref.vq_argmin_f64(x[[0, 3, 5]], torch.ones(K, D)), torch.zeros(3, dtype=torch.int64))
