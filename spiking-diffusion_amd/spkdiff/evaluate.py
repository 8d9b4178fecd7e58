"""The reconstruction evaluation of R/main.py:300-323 (per test batch: model forward, ``F.mse_loss`` and ``1 - SSIM``; at the
end ``round(sum / len, 3)`` of both lists) without a host synchronisation per batch.

The reference's loop reads two ``.item()`` per batch and builds the SSIM from ~20 launches.  Here a batch adds to the model's
own launches one ``ops.ssim_mse`` launch (fp64 sums per image) and one fixed-order sum of them into slot ``i`` of a device
buffer; after the last batch one vectorised epilogue rounds every slot to the fp32 values ``.item()`` would have returned
(``mse_i``, ``1 - ssim_i``) and ONE copy brings them to the host.

``token_nll_eval`` is the denoiser's counterpart, which the reference lacks: the test set's code indices scored under the sampler's
own reverse process (``AbsorbingDiffusion.score``), again with one read at the end.

``temperature_sweep`` is the sampling sweep of R/main.py:379-443 (per temperature: many ``abdiff.sample(temp=tem)`` calls of 16
images, decoded) run as ONE job with a per-image temperature; ``step_count_sweep`` is its counterpart over the
step count of confidence-ordered decoding, one job with a per-image step count."""
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
    SNN_VQVAE_uni (three outputs), SNN_VAE (two outputs) or the plain-CNN VQVAE (called with the images alone, R/main.py:311)
    on a ROCm device.  Returns {"loss_ssim", "loss_mse" (unrounded
    means), "loss_ssim_rounded", "loss_mse_rounded" (what main.py prints), "n_batches"}.  The last batch may be smaller."""
    from metric.pytorch_ssim import create_window
    from snn_model.vae_model import VQVAE
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
            if isinstance(model, VQVAE):                # (the ANN baseline: one argument, no neuron state to reset)
                recon_images = model(norm_images)[1]
            else:
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


def _sweep_temps(temps, n_per_temp):
    """fp32 [len(temps) * n_per_temp] on the host: image g * n_per_temp + j of the sweep job has temperature temps[g]."""
    tv = torch.as_tensor(temps, dtype=torch.float64).reshape(-1)
    n_per_temp = int(n_per_temp)
    if tv.numel() < 1 or n_per_temp < 1:
        raise ValueError("temperature_sweep: needs at least one temperature and n_per_temp >= 1")
    if not bool(torch.isfinite(tv).all()) or not bool((tv > 0).all()):
        raise ValueError("temperature_sweep: every temperature must be finite and > 0")
    return tv.to(torch.float32).repeat_interleave(n_per_temp)


def _sweep_top_k(top_k, n_temps, n_per_temp):
    """The ``top_k`` of a sweep, per image of the job as ``_sweep_temps`` expands the temperatures: None, or int32 [n_temps *
    n_per_temp] on the host from an int >= 0 (every image) or one k per temperature (image g * n_per_temp + j has top_k[g];
    0: that group is not truncated)."""
    if top_k is None:
        return None
    bad = ValueError(f"temperature_sweep: top_k must be None, an integer >= 0 or one per temperature ({n_temps}), got {top_k!r}")
    if isinstance(top_k, bool):
        raise bad
    try:
        kv = torch.as_tensor(top_k).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        raise bad from None
    if kv.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64) or kv.dim() > 1:
        raise bad
    kv = kv.reshape(-1).expand(n_temps) if kv.numel() == 1 else kv
    if kv.numel() != n_temps or bool((kv < 0).any()) or bool((kv > 0x7FFFFFFF).any()):
        raise bad
    return kv.to(torch.int32).repeat_interleave(int(n_per_temp))


def _sweep_top_p(top_p, n_temps, n_per_temp):
    """The ``top_p`` of a sweep, per image of the job as ``_sweep_temps`` expands the temperatures: None, or fp32 [n_temps *
    n_per_temp] on the host from a number in (0, 1] (every image) or one p per temperature (image g * n_per_temp + j has top_p[g];
    1: that group is not truncated)."""
    if top_p is None:
        return None
    bad = ValueError(f"temperature_sweep: top_p must be None, a number in (0, 1] or one per temperature ({n_temps}), got {top_p!r}")
    if isinstance(top_p, bool):
        raise bad
    try:
        pv = torch.as_tensor(top_p).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        raise bad from None
    if pv.dtype in (torch.bool, torch.complex64, torch.complex128) or pv.dim() > 1:
        raise bad
    pv = pv.to(torch.float64)
    pv = pv.reshape(-1).expand(n_temps) if pv.numel() == 1 else pv
    if pv.numel() != n_temps or not bool(torch.isfinite(pv).all()) or not bool(((pv.to(torch.float32) > 0) & (pv <= 1)).all()):
        raise bad
    return pv.to(torch.float32).repeat_interleave(int(n_per_temp))


@torch.no_grad()
def temperature_sweep_range(model, sampler, temps, n_per_temp, lo, hi, sample_steps=None, batch=256, T=16, top_k=None, top_p=None):
    """Images [lo, hi) of the job ``temperature_sweep`` describes -- what one rank of ``spkdiff.dist.temperature_sweep_sharded``
    runs: (uint8 [hi - lo, C, H, W], tokens int64 [hi - lo, h, w]).  Calls of at most ``batch`` images (None: one call), each a
    shard of the job (``set_shard(first, count)``) with its slice of the per-image temperature vector, all under ONE noise key
    (``AbsorbingDiffusion._one_key``: one draw from torch's CPU generator, broadcast from rank 0 inside a process group), so the
    images depend on neither ``batch`` nor the range.  ``n_samples`` / ``global_first`` of the sampler are restored.
    ``top_k``: None, an int or one k per temperature (``temperature_sweep_top_k``); every call takes its slice of the per-image
    vector through ``sample_top_k``.  ``top_p``: None, a number or one p per temperature (``temperature_sweep_top_p``), sliced in
    the same way and handed to ``sample_top_p``."""
    tv = _sweep_temps(temps, n_per_temp)
    kv = _sweep_top_k(top_k, len(temps), n_per_temp)
    pv = _sweep_top_p(top_p, len(temps), n_per_temp)
    lo, hi = int(lo), int(hi)
    if not 0 <= lo < hi <= tv.numel():
        raise ValueError(f"temperature_sweep: the range [{lo}, {hi}) is not inside the job's {tv.numel()} images")
    if getattr(sampler, "noise_source", "philox") != "philox":
        raise ValueError("temperature_sweep: one job in several calls needs the counter-based noise (noise_source = 'philox')")
    step = hi - lo if batch is None else int(batch)
    if step < 1:
        raise ValueError("temperature_sweep: batch must be >= 1 or None")
    tv = tv.to(next(model.parameters()).device)        # one copy: every call takes a slice
    kv = None if kv is None else kv.to(tv.device)
    pv = None if pv is None else pv.to(tv.device)
    keep = (sampler.n_samples, sampler.global_first)
    images, tokens = [], []
    try:
        sampler.set_shard(lo, min(step, hi - lo))       # (declares the shard before the key is drawn: the broadcast rule)
        with sampler._one_key():
            for first in range(lo, hi, step):
                count = min(step, hi - first)
                sampler.set_shard(first, count)
                if pv is not None:
                    tok = sampler.sample_top_p(pv[first:first + count], temp=tv[first:first + count], sample_steps=sample_steps,
                                               top_k=None if kv is None else kv[first:first + count])
                elif kv is None:
                    tok = sampler.sample(temp=tv[first:first + count], sample_steps=sample_steps)
                else:
                    tok = sampler.sample_top_k(kv[first:first + count], temp=tv[first:first + count], sample_steps=sample_steps)
                tok = tok.reshape(count, tok.shape[-2], tok.shape[-1])
                images.append(model.decode_tokens(tok, T, want_u8=True)[1])
                tokens.append(tok)
    finally:
        sampler.n_samples, sampler.global_first = keep
    return torch.cat(images), torch.cat(tokens)


@torch.no_grad()
def temperature_sweep(model, sampler, temps, n_per_temp, sample_steps=None, batch=256, T=16):
    """R/main.py's temperature sweep (:379-443: for every temperature, calls of ``abdiff.sample(temp=tem)`` at 16 images, each
    decoded to uint8) as ONE job of ``len(temps) * n_per_temp`` images: image ``g * n_per_temp + j`` has temperature
    ``temps[g]``.  Returns (uint8 images [len(temps), n_per_temp, C, H, W] -- main.py's ``all_images_list`` --, tokens int64
    [len(temps), n_per_temp, h, w]) on the device.  The job runs in calls of at most ``batch`` images whatever the group
    boundaries (``batch=None``: one call), see ``temperature_sweep_range``; one captured graph per call size serves every
    temperature, where the scalar protocol captures one per temperature.  Image (g, j) is the image ``sample(temps[g])`` gives at
    global index ``g * n_per_temp + j`` under the sweep's key."""
    return temperature_sweep_top_k(model, sampler, temps, n_per_temp, None, sample_steps=sample_steps, batch=batch, T=T)


@torch.no_grad()
def temperature_sweep_top_k(model, sampler, temps, n_per_temp, top_k, sample_steps=None, batch=256, T=16):
    """``temperature_sweep`` with top-k truncation: ``top_k`` is None (the plain sweep), an int for every image
    or one k per temperature -- image (g, j) is drawn at temperature ``temps[g]`` from its positions' ``top_k[g]`` likeliest codes
    (0: group g is not truncated).  Same job, same key rule, same result shapes; the images depend on neither ``batch`` nor the
    split, and one captured graph per call size serves every temperature and every k."""
    G, n = len(temps), int(n_per_temp)
    u8, tok = temperature_sweep_range(model, sampler, temps, n, 0, G * n, sample_steps=sample_steps, batch=batch, T=T, top_k=top_k)
    return u8.reshape((G, n) + tuple(u8.shape[1:])), tok.reshape((G, n) + tuple(tok.shape[1:]))


@torch.no_grad()
def temperature_sweep_top_p(model, sampler, temps, n_per_temp, top_p, sample_steps=None, batch=256, T=16, top_k=None):
    """``temperature_sweep`` with nucleus truncation: ``top_p`` is None (the sweep ``top_k`` describes), a number
    in (0, 1] for every image or one p per temperature -- image (g, j) is drawn at temperature ``temps[g]`` from the likeliest
    codes whose mass reaches ``top_p[g]`` (1: group g is not truncated), after the top-k truncation ``top_k`` asks for.  Same job,
    same key rule, same result shapes; the images depend on neither ``batch`` nor the split, and one captured graph per call size
    serves every temperature, every k and every p."""
    G, n = len(temps), int(n_per_temp)
    u8, tok = temperature_sweep_range(model, sampler, temps, n, 0, G * n, sample_steps=sample_steps, batch=batch, T=T, top_k=top_k,
                                      top_p=top_p)
    return u8.reshape((G, n) + tuple(u8.shape[1:])), tok.reshape((G, n) + tuple(tok.shape[1:]))


@torch.no_grad()
def step_count_sweep(model, sampler, steps, n_per_steps, batch=256, T=16, temp=1.0, top_k=None, top_p=None, schedule=None,
                     selection_noise=None, remask=None):
    """"How few steps are enough?" as ONE job: ``n_per_steps`` confidence-ordered samples for every entry of
    ``steps`` (integers >= 1) -- image ``g * n_per_steps + j`` of the job runs ``steps[g]`` steps -- through
    ``AbsorbingDiffusion.sample_confident`` with per-image step counts.  Returns (uint8 images [len(steps), n_per_steps, C, H, W],
    tokens int64 [len(steps), n_per_steps, h, w]) on the device.  The job runs in calls of at most ``batch`` images whatever the
    group boundaries (None: one call), each a shard of the job (``set_shard``) under ONE noise key (``_one_key``), every call at
    the largest count among its images; image (g, j) is the image ``sample_confident(steps[g])`` gives at global index
    ``g * n_per_steps + j`` under the sweep's key, so neither ``batch`` nor the grouping changes an image.  ``temp`` / ``top_k`` /
    ``top_p``: one value for the whole job, as sample_confident() takes a number.  ``schedule`` (None, 'linear' or 'cosine': every
    image gets the named table of its own step count) and ``selection_noise`` (one tau >= 0, annealed over each image's own steps):
    DESIGN.md §4.17, handed to every call; both None: the calls made before.  ``remask`` (None or one int r >= 0: up to r tokens
    per image return to the masked state at every step t >= 2 of the image's own run; a table fits one step count): DESIGN.md §4.18,
    handed to every call.  ``n_samples`` / ``global_first`` of the sampler are
    restored."""
    n = int(n_per_steps)
    try:
        sv = torch.as_tensor(steps)
        ok = sv.dim() == 1 and sv.numel() >= 1 and sv.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64) and \
            bool((sv >= 1).all())
    except (TypeError, ValueError, RuntimeError):
        ok = False
    if not ok or n < 1:
        raise ValueError(f"step_count_sweep: steps must be a sequence of integers >= 1 and n_per_steps >= 1, got {steps!r}, {n_per_steps!r}")
    if not (schedule is None or isinstance(schedule, str)):
        raise ValueError(f"step_count_sweep: schedule is None, 'linear' or 'cosine' (a table fits one step count), got {schedule!r}")
    sched = {} if schedule is None and selection_noise is None else {'schedule': schedule, 'selection_noise': selection_noise}
    if remask is not None:
        if isinstance(remask, bool) or not hasattr(remask, '__index__'):
            raise ValueError(f"step_count_sweep: remask is None or one integer >= 0 (a table fits one step count), got {remask!r}")
        sched['remask'] = remask
    if getattr(sampler, "noise_source", "philox") != "philox":
        raise ValueError("step_count_sweep: one job in several calls needs the counter-based noise (noise_source = 'philox')")
    sv = sv.to(torch.int32).cpu().repeat_interleave(n)
    total = int(sv.numel())
    step = total if batch is None else int(batch)
    if step < 1:
        raise ValueError("step_count_sweep: batch must be >= 1 or None")
    keep = (sampler.n_samples, sampler.global_first)
    images, tokens = [], []
    try:
        sampler.set_shard(0, min(step, total))          # (declares the shard before the key is drawn: the broadcast rule)
        with sampler._one_key():
            for first in range(0, total, step):
                count = min(step, total - first)
                sampler.set_shard(first, count)
                tok = sampler.sample_confident(sv[first:first + count], temp=temp, top_k=top_k, top_p=top_p, **sched)
                tok = tok.reshape(count, tok.shape[-2], tok.shape[-1])
                images.append(model.decode_tokens(tok, T, want_u8=True)[1])
                tokens.append(tok)
    finally:
        sampler.n_samples, sampler.global_first = keep
    u8, tok = torch.cat(images), torch.cat(tokens)
    G = total // n
    return u8.reshape((G, n) + tuple(u8.shape[1:])), tok.reshape((G, n) + tuple(tok.shape[1:]))


def token_nll_eval(model, sampler, batches, temp=1.0, sample_steps=None, orders=1, T=16, temps=None):
    """How well the denoiser models the VQ-VAE's codes, without a sample: every batch is encoded (``model.encode_images``) and its
    codes scored under the sampler's reverse process (``AbsorbingDiffusion.score``: a lower bound on log p(codes), ``orders``
    reveal orders per image -- DESIGN.md §4.10).  ``batches`` as for ``reconstruction_eval`` (images in [0, 1]; the last batch
    may be smaller).  The per-batch sums stay on the device and ONE copy at the end brings the total to the host.  Returns
    {"bits_per_dim": -mean(log_prob) / (ln 2 * h * w) -- the unit of the reference's training loss, lower is better --,
    "nats_per_image": -mean(log_prob), "n_images", "orders"}; the mean runs over images and orders.

    ``temps = [t_0, ...]`` (then ``temp`` is not read): the NLL-versus-temperature curve from one pass -- every batch is repeated
    ``len(temps)`` times and scored in ONE ``score()`` call with a per-image temperature (replica r of image i sits at index
    r * B + i of the call and has temperature temps[r]); "bits_per_dim" and "nats_per_image" are then lists with one figure per
    temperature and "temps" repeats the list.  The replicas of an image sit at different global image indices, so they see
    different reveal orders: each figure is an unbiased estimate of its own temperature's bound, not the same orders at another
    temperature."""
    device = next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("spkdiff: token_nll_eval runs the encoder and the denoiser on a ROCm device; there is no CPU path")
    G = None
    if temps is not None:
        tv = _sweep_temps(temps, 1).to(device)
        G = int(tv.numel())
    total = torch.zeros(() if G is None else (G,), dtype=torch.float64, device=device)
    n_images = 0
    # (no_grad, not inference_mode: the sampler keeps the buffers of a graph it captures here and writes them in later calls,
    #  which inference tensors would refuse outside this block)
    with torch.no_grad():
        for batch in batches:
            images = batch[0] if isinstance(batch, (tuple, list)) else batch
            codes = model.encode_images((images - 0.5).to(device).float().contiguous(), T)
            if G is None:
                total += sampler.score(codes, temp=temp, sample_steps=sample_steps, orders=orders).log_prob.sum()
            else:
                B = int(codes.shape[0])
                lp = sampler.score(codes.repeat(G, 1, 1), temp=tv.repeat_interleave(B), sample_steps=sample_steps,
                                   orders=orders).log_prob                       # [orders, G * B]
                total += lp.reshape(int(orders), G, B).sum(dim=(0, 2))
            n_images += int(images.shape[0])
        if not n_images:
            raise ValueError("token_nll_eval: no batches")
        host = total.cpu()
    h, w = sampler.shape
    if G is not None:
        nats = [-float(v) / (n_images * int(orders)) for v in host.tolist()]
        return {"bits_per_dim": [v / (math.log(2) * h * w) for v in nats], "nats_per_image": nats, "n_images": n_images,
                "orders": int(orders), "temps": [float(v) for v in tv.tolist()]}
    nats = -float(host.item()) / (n_images * int(orders))
    return {"bits_per_dim": nats / (math.log(2) * h * w), "nats_per_image": nats, "n_images": n_images, "orders": int(orders)}
