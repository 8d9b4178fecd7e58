"""The reconstruction evaluation of R/main.py:300-323 (per test batch: model forward, ``F.mse_loss`` and ``1 - SSIM``; at the
end ``round(sum / len, 3)`` of both lists) without a host synchronisation per batch.

The reference's loop reads two ``.item()`` per batch and builds the SSIM from ~20 launches.  Here a batch adds to the model's
own launches one ``ops.ssim_mse`` launch (fp64 sums per image) and one fixed-order sum of them into slot ``i`` of a device
buffer; after the last batch one vectorised epilogue rounds every slot to the fp32 values ``.item()`` would have returned
(``mse_i``, ``1 - ssim_i``) and ONE copy brings them to the host.

``token_nll_eval`` is the denoiser's counterpart, which the reference lacks: the test set's code indices scored under the sampler's
own reverse process (``AbsorbingDiffusion.score``), again with one read at the end."""
from __future__ import annotations

import math

import torch

from . import ops


def aggregate(per_batch_ssim_loss, per_batch_mse):
    """main.py:322-323 on the per-batch values ``.item()`` returned: Python-float ``sum(list) / len(list)`` and its
    ``round(..., 3)``."""
    loss_ssim = [float(v) for v in per_batch_ssim_loss]
    loss_mse = [float(v) for v in per_batch_mse]
    if not loss_ssim or len(loss_ssim) != len(loss_mse):
        raise ValueError("reconstruction_eval: needs one SSIM and one MSE value per batch, at least one batch")
    s, m = sum(loss_ssim) / len(loss_ssim), sum(loss_mse) / len(loss_mse)
    return {"loss_ssim": s, "loss_mse": m, "loss_ssim_rounded": round(s, 3), "loss_mse_rounded": round(m, 3),
            "n_batches": len(loss_ssim)}


def reconstruction_eval(model, batches, T=16, window_size=11):
    """``batches`` yields ``images`` in [0, 1] ([B,C,H,W]) or ``(images, labels)``; ``model`` is an eval-mode SNN_VQVAE,
    SNN_VQVAE_uni (three outputs) or SNN_VAE (two outputs) on a ROCm device.  Returns {"loss_ssim", "loss_mse" (unrounded
    means), "loss_ssim_rounded", "loss_mse_rounded" (what main.py prints), "n_batches"}.  The last batch may be smaller."""
    from metric.pytorch_ssim import create_window
    from spikingjelly.activation_based import functional

    device = next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("spkdiff: reconstruction_eval runs the model and the metrics on a ROCm device; there is no CPU path")
    window2d = create_window(window_size, 1)[0, 0].contiguous().to(device)
    chunks, denoms = [], []                             # device slots, 64 batches per buffer
    with torch.inference_mode():
        for batch in batches:
            images = batch[0] if isinstance(batch, (tuple, list)) else batch
            norm_images = (images - 0.5).to(device)
            images_spike = norm_images.unsqueeze(0).repeat(T, 1, 1, 1, 1)
            recon_images = model(images_spike, norm_images)[1]
            functional.reset_net(model)
            N, C, H, W = norm_images.shape
            i = len(denoms)
            if i % 64 == 0:
                chunks.append(torch.empty((64, 2), dtype=torch.float64, device=device))
            out = torch.empty((2, N), dtype=torch.float64, device=device)
            ops.ssim_mse(recon_images, norm_images, window2d, out=out)
            torch.sum(out, dim=1, out=chunks[-1][i % 64])     # {sum of the SSIM map, sum of squared differences} of the batch
            denoms.append((N * C * ops.ssim_mse_out_size(H, window_size) * ops.ssim_mse_out_size(W, window_size),
                           N * C * H * W))
        if not denoms:
            raise ValueError("reconstruction_eval: no batches")
        totals = torch.cat(chunks)[:len(denoms)]
        means = (totals / torch.tensor(denoms, dtype=torch.float64).to(device)).float()     # fp32 ssim_i, mse_i
        host = torch.stack((1 - means[:, 0], means[:, 1]), dim=1).cpu()                     # fp32 1 - ssim_i, as the script forms it
    return aggregate(host[:, 0].tolist(), host[:, 1].tolist())


def token_nll_eval(model, sampler, batches, temp=1.0, sample_steps=None, orders=1, T=16):
    """How well the denoiser models the VQ-VAE's codes, without a sample: every batch is encoded (``model.encode_images``) and its
    codes scored under the sampler's reverse process (``AbsorbingDiffusion.score``: a lower bound on log p(codes), ``orders``
    reveal orders per image -- DESIGN.md §4.10).  ``batches`` as for ``reconstruction_eval`` (images in [0, 1]; the last batch
    may be smaller).  The per-batch sums stay on the device and ONE copy at the end brings the total to the host.  Returns
    {"bits_per_dim": -mean(log_prob) / (ln 2 * h * w) -- the unit of the reference's training loss, lower is better --,
    "nats_per_image": -mean(log_prob), "n_images", "orders"}; the mean runs over images and orders."""
    device = next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("spkdiff: token_nll_eval runs the encoder and the denoiser on a ROCm device; there is no CPU path")
    total = torch.zeros((), dtype=torch.float64, device=device)
    n_images = 0
    # (no_grad, not inference_mode: the sampler keeps the buffers of a graph it captures here and writes them in later calls,
    #  which inference tensors would refuse outside this block)
    with torch.no_grad():
        for batch in batches:
            images = batch[0] if isinstance(batch, (tuple, list)) else batch
            codes = model.encode_images((images - 0.5).to(device).float().contiguous(), T)
            total += sampler.score(codes, temp=temp, sample_steps=sample_steps, orders=orders).log_prob.sum()
            n_images += int(images.shape[0])
        if not n_images:
            raise ValueError("token_nll_eval: no batches")
        nats = -float(total.item()) / (n_images * int(orders))
    h, w = sampler.shape
    return {"bits_per_dim": nats / (math.log(2) * h * w), "nats_per_image": nats, "n_images": n_images, "orders": int(orders)}
