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
step count of confidence-ordered decoding, one job with a per-image step count.

``sample_quality_eval`` scores generated images against data: the Frechet distance between Gaussian fits (``FeatureStats``,
``frechet_distance``) and the kernel distance of KID (``kernel_distance``) -- the arithmetic of R/main.py:445-529 after its feature
network -- on a feature space of this project's own, in fp64 on the matrix cores."""
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


# ---- sample quality: Frechet and kernel distances on a feature space ----------------------------------------
class FeatureStats:
    """Streaming first and second moments of a feature set: ``n``, ``sum`` fp64 [d] and ``gram`` = sum of x x^T fp64 [d, d].  The
    state is additive -- ``merge`` adds another instance's, which is what a sharded job reduces -- and mean and covariance follow
    from it.  ``update`` takes fp32 [n, d]: a device tensor goes through ``ops.feature_moments`` (fp64 matrix cores: exact
    products, one accumulation chain per element, so the result depends on the row order and the split of the stream into
    updates only through the chain contract of DESIGN.md §4.19), a CPU tensor through torch's fp64 operators.  No host
    synchronisation inside ``update`` (``n`` is counted from shapes)."""

    def __init__(self, d, device="cpu"):
        d = int(d)
        if not 1 <= d <= ops.FEATURE_MAX_D:
            raise ValueError(f"FeatureStats: d must be in 1 .. {ops.FEATURE_MAX_D}, got {d}")
        self.d, self.device, self.n = d, torch.device(device), 0
        self.sum = torch.zeros(d, dtype=torch.float64, device=self.device)
        self.gram = torch.zeros((d, d), dtype=torch.float64, device=self.device)

    def update(self, features):
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[1] != self.d:
            raise ValueError(f"FeatureStats.update: features must be [n, {self.d}], got {tuple(getattr(features, 'shape', ()))}")
        if features.dtype != torch.float32:
            raise ValueError(f"FeatureStats.update: features must be fp32, got {features.dtype}")
        if features.device.type != self.device.type:
            raise ValueError(f"FeatureStats.update: features are on '{features.device}', the state on '{self.device}'")
        if self.device.type == "cuda":
            ops.feature_moments(features, self.sum, self.gram)
        elif features.shape[0]:
            f = features.double()
            self.sum += f.sum(dim=0)
            self.gram += f.T @ f
        self.n += int(features.shape[0])
        return self

    def merge(self, other):
        if not isinstance(other, FeatureStats) or other.d != self.d:
            raise ValueError("FeatureStats.merge: needs a FeatureStats of the same d")
        self.sum += other.sum.to(self.device)
        self.gram += other.gram.to(self.device)
        self.n += other.n
        return self

    def mean(self):
        """fp64 [d] on the state's device."""
        if self.n < 1:
            raise ValueError("FeatureStats.mean: no features yet")
        return self.sum / self.n

    def cov(self):
        """The unbiased covariance, fp64 [d, d] on the state's device: (gram - sum sum^T / n) * (1 / (n - 1)), the value
        ``np.cov(rowvar=False)`` gives (it, too, multiplies by the reciprocal).  One pass: the subtraction cancels
        (mean / std)^2 of the leading digits, which fp64 affords for features of order one."""
        if self.n < 2:
            raise ValueError(f"FeatureStats.cov: needs n >= 2, has {self.n}")
        return (self.gram - torch.outer(self.sum, self.sum) / self.n) * (1.0 / (self.n - 1))


def _moments_np(a, what):
    import numpy as np
    if isinstance(a, FeatureStats):
        if a.n < 2:
            raise ValueError(f"frechet_distance: {what} has n = {a.n}; a covariance needs n >= 2")
        mu, sigma = a.mean().cpu().numpy(), a.cov().cpu().numpy()
    else:
        mu, sigma = a
        mu = np.atleast_1d(np.asarray(mu.cpu() if isinstance(mu, torch.Tensor) else mu, dtype=np.float64))
        sigma = np.atleast_2d(np.asarray(sigma.cpu() if isinstance(sigma, torch.Tensor) else sigma, dtype=np.float64))
    if mu.ndim != 1 or sigma.shape != (mu.shape[0], mu.shape[0]):
        raise ValueError(f"frechet_distance: {what} must be (mu [d], sigma [d, d]), got {mu.shape} and {sigma.shape}")
    if not (np.isfinite(mu).all() and np.isfinite(sigma).all()):
        raise ValueError(f"frechet_distance: {what} has non-finite moments")
    return mu, sigma


def frechet_distance(a, b, convention="exact"):
    """The Frechet distance between the Gaussians fitted to two feature sets.  ``a``, ``b``: ``FeatureStats`` or ``(mu, sigma)``
    pairs.  The d x d eigenproblems run on the host in fp64 (numpy); they are not the hot path.

    ``'exact'``: |mu1 - mu2|^2 + tr C1 + tr C2 - 2 sum sqrt(lambda(sqrt(C1) C2 sqrt(C1))), eigenvalues clipped at 0 -- the
    distance itself (tr sqrt(C1 C2) by a symmetric eigenproblem).
    ``'reference'``: the formula of R/metric/Fid_score.py:116-172, whose own ``sqrtm(A) = U sqrt(S) V`` from an SVD is applied
    to the non-symmetric C1 C2; it equals the distance only when C1 and C2 commute and is kept for parity with
    what main.py would print.

    ValueError on non-finite moments or n < 2.  For n <= d the covariance has rank at most n - 1: sqrt(C1) C2 sqrt(C1) then has at
    most n - 1 non-zero eigenvalues, the cross term is under-estimated and the value is biased upwards by an amount that depends on
    n, so distances are comparable only between sets of the same size (the same holds, less visibly, for every finite n)."""
    import numpy as np
    mu1, s1 = _moments_np(a, "a")
    mu2, s2 = _moments_np(b, "b")
    if mu1.shape != mu2.shape:
        raise ValueError(f"frechet_distance: the two sets have d = {mu1.shape[0]} and {mu2.shape[0]}")
    diff = mu1 - mu2
    if convention == "exact":
        lam, V = np.linalg.eigh((s1 + s1.T) / 2)
        root = (V * np.sqrt(np.clip(lam, 0.0, None))) @ V.T
        M = root @ s2 @ root
        tr_covmean = float(np.sqrt(np.clip(np.linalg.eigvalsh((M + M.T) / 2), 0.0, None)).sum())
    elif convention == "reference":
        U, S, Vh = np.linalg.svd(s1.dot(s2))
        tr_covmean = float(np.trace(U.dot(np.diag(np.sqrt(S))).dot(Vh)))
    else:
        raise ValueError(f"frechet_distance: convention is 'exact' or 'reference', got {convention!r}")
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * tr_covmean)


def kernel_subsets(n_x, n_y, subsets, subset_size, seed=0):
    """The subset tables of ``kernel_distance``: (ix int32 [subsets, subset_size], iy likewise) on the host, a function of the
    arguments alone.  One seeded host generator; for s = 0, 1, ...: the first ``subset_size`` entries of a permutation of n_x, then
    of a permutation of n_y (without replacement, as torchmetrics' KernelInceptionDistance draws)."""
    subsets, m = int(subsets), int(subset_size)
    if subsets < 1 or m < 2:
        raise ValueError(f"kernel_distance: needs subsets >= 1 and subset_size >= 2, got {subsets}, {subset_size}")
    if m > min(n_x, n_y):
        raise ValueError(f"kernel_distance: subset_size {m} is larger than a set ({n_x} and {n_y} samples)")
    g = torch.Generator().manual_seed(int(seed))
    ix = torch.empty((subsets, m), dtype=torch.int32)
    iy = torch.empty((subsets, m), dtype=torch.int32)
    for s in range(subsets):
        ix[s] = torch.randperm(n_x, generator=g)[:m]
        iy[s] = torch.randperm(n_y, generator=g)[:m]
    return ix, iy


def _poly_sums_host(X, Y, ix, iy, gamma, coef, degree, symmetric):
    """``ops.poly_kernel_sums`` restated with torch's fp64 operators for CPU tensors (the materialised Gram matrix per subset)."""
    out = torch.zeros((1 if ix is None else ix.shape[0], 2), dtype=torch.float64)
    Xd, Yd = X.double(), Y.double()
    for s in range(out.shape[0]):
        v = gamma * ((Xd if ix is None else Xd[ix[s].long()]) @ (Yd if iy is None else Yd[iy[s].long()]).T) + coef
        k = v
        for _ in range(degree - 1):
            k = k * v
        out[s, 0] = k.sum()
        if symmetric:
            out[s, 1] = torch.diagonal(k).sum()
    return out


def kernel_distance(fx, fy, subsets=100, subset_size=1000, degree=3, gamma=None, coef=1.0, seed=0):
    """The kernel distance of KID on any feature space: (mean, std) over ``subsets`` random subsets of ``subset_size`` samples a
    side of the unbiased MMD^2 under k(a, b) = (gamma <a, b> + coef)^degree,
        (sum k_xx + sum k_yy - tr k_xx - tr k_yy) / (m (m - 1)) - 2 sum k_xy / m^2,
    with the defaults main.py's ``KernelInceptionDistance()`` runs with (gamma None: 1 / d); the std is the unbiased one
    (``torch.std``; 0 for a single value).  fx, fy fp32 [n, d].  Device tensors: the subset tables (``kernel_subsets``) are
    uploaded once and three ``ops.poly_kernel_sums`` calls serve all subsets, no Gram matrix is written, one host read at the end;
    CPU tensors: torch fp64 operators.  ``subsets=None``: the full-set estimate (each k_xx / k_yy term over its own n (n - 1),
    k_xy over n_x n_y), std 0.  ``subset_size`` larger than either set raises, as the torchmetrics class does.  The estimator is
    unbiased, not non-negative: a set against itself gives 2 (sum k - m tr k) / (m^2 (m - 1)) <= 0, not 0."""
    for t, name in ((fx, "fx"), (fy, "fy")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError(f"kernel_distance: {name} must be an fp32 [n, d] tensor")
    d = int(fx.shape[1])
    if fy.shape[1] != d:
        raise ValueError(f"kernel_distance: fx has d = {d} and fy d = {int(fy.shape[1])}")
    if not 1 <= d <= ops.FEATURE_MAX_D:
        raise ValueError(f"kernel_distance: d must be in 1 .. {ops.FEATURE_MAX_D}, got {d}")
    if isinstance(degree, bool) or not hasattr(degree, "__index__") or not 1 <= int(degree) <= ops.POLY_KERNEL_MAX_DEGREE:
        raise ValueError(f"kernel_distance: degree must be an integer in 1 .. {ops.POLY_KERNEL_MAX_DEGREE}, got {degree!r}")
    if fx.device != fy.device:
        raise ValueError("kernel_distance: fx and fy must be on one device")
    n_x, n_y = int(fx.shape[0]), int(fy.shape[0])
    degree, gamma, coef = int(degree), (1.0 / d if gamma is None else float(gamma)), float(coef)
    if subsets is None:
        if min(n_x, n_y) < 2:
            raise ValueError("kernel_distance: needs at least two samples a side")
        ix = iy = None
        mx, my = n_x, n_y
    else:
        ix, iy = kernel_subsets(n_x, n_y, subsets, subset_size, seed)
        mx = my = int(subset_size)
    if fx.is_cuda:
        if ix is not None:
            ix, iy = ix.to(fx.device), iy.to(fx.device)
        kw = dict(gamma=gamma, coef=coef, degree=degree)
        sxx = ops.poly_kernel_sums(fx, fx, ix, ix, symmetric=True, **kw)
        syy = ops.poly_kernel_sums(fy, fy, iy, iy, symmetric=True, **kw)
        sxy = ops.poly_kernel_sums(fx, fy, ix, iy, symmetric=False, **kw)
    else:
        sxx = _poly_sums_host(fx, fx, ix, ix, gamma, coef, degree, True)
        syy = _poly_sums_host(fy, fy, iy, iy, gamma, coef, degree, True)
        sxy = _poly_sums_host(fx, fy, ix, iy, gamma, coef, degree, False)
    vals = mmd2_from_sums(sxx, syy, sxy, mx, my)
    mean = vals.mean()
    std = vals.std() if vals.numel() > 1 else torch.zeros_like(mean)
    mean, std = torch.stack((mean, std)).cpu().tolist()
    return mean, std


def mmd2_from_sums(sxx, syy, sxy, mx, my):
    """fp64 [S]: the unbiased MMD^2 of every subset from the three [S, 2] results of ``ops.poly_kernel_sums`` (mx, my samples a
    side), in this order of operations: ((xx - tr_xx) / (mx (mx - 1)) + (yy - tr_yy) / (my (my - 1))) - 2 xy / (mx my) -- for
    mx = my the two quotients share the divisor, as in the formula above."""
    if mx == my:
        return ((sxx[:, 0] - sxx[:, 1]) + (syy[:, 0] - syy[:, 1])) / (mx * (mx - 1)) - 2 * sxy[:, 0] / (mx * mx)
    return (sxx[:, 0] - sxx[:, 1]) / (mx * (mx - 1)) + (syy[:, 0] - syy[:, 1]) / (my * (my - 1)) - 2 * sxy[:, 0] / (mx * my)


KID_DEFAULTS = dict(subsets=100, subset_size=1000, degree=3, gamma=None, coef=1.0, seed=0)


def _feature_fn(model, features, T):
    """images fp32 [B,C,H,W] in [0, 1] on the device -> fp32 [B, d]."""
    if callable(features):
        return features
    if features == "encoder":
        if not hasattr(model, "encode_features"):
            raise ValueError(f"sample_quality_eval: {type(model).__name__} has no encode_features (the 'encoder' feature space is "
                             "the SNN_VQVAE encoder's read-out); use features='pixels' or a callable images -> [B, d]")
        return lambda im: model.encode_features((im - 0.5).contiguous(), T)
    if features == "pixels":
        return lambda im: im.reshape(im.shape[0], -1).contiguous()
    raise ValueError(f"sample_quality_eval: features is 'encoder', 'pixels' or a callable images -> [B, d], got {features!r}")


def sample_quality_eval(model, sampler, real_batches, n_samples, draw=None, features="encoder", batch=256, T=16, kid=KID_DEFAULTS,
                        sample_steps=None):
    """How close are the sampler's images to data?  Frechet and kernel distances between ``real_batches`` (as for
    ``reconstruction_eval``: images in [0, 1] or (images, labels)) and ``n_samples`` generated images, on a feature space this
    project owns.  ``draw``: a callable (sampler, b) -> tokens of b images (any ``sample_*`` method fits in a
    lambda); None: ``sampler.sample(1.0, sample_steps)``.  The job runs in calls of at most ``batch`` images, each a shard of the
    job under ONE noise key, decoded with ``model.decode_tokens``.  ``features``: 'encoder' (``model.encode_features``: the
    read-out the quantiser searches on), 'pixels' (the uint8 image divided by 255, flattened; real images are rounded to the
    same grid) or a callable images in [0, 1] -> fp32 [B, d].  Both sides go through the uint8 image, so the real side sees the decoder's
    quantisation too.  One ``FeatureStats`` per side; the features themselves are kept only when ``kid`` is not None (a dict of
    ``kernel_distance`` arguments over ``KID_DEFAULTS``).  One host read per distance at the end.  Returns {"fd",
    "fd_reference_convention", "kd_mean", "kd_std" (None without kid), "n_real", "n_generated", "d"}."""
    device = next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("spkdiff: sample_quality_eval runs the sampler and the metrics on a ROCm device; there is no CPU path")
    fn = _feature_fn(model, features, T)
    n_samples, step = int(n_samples), int(batch)
    if n_samples < 2 or step < 1:
        raise ValueError("sample_quality_eval: needs n_samples >= 2 and batch >= 1")
    if getattr(sampler, "noise_source", "philox") != "philox":
        raise ValueError("sample_quality_eval: one job in several calls needs the counter-based noise (noise_source = 'philox')")
    if kid is not None:
        kid = {**KID_DEFAULTS, **kid}
    if draw is None:
        draw = lambda s, b: s.sample(1.0, sample_steps)      # noqa: E731
    stats, kept = {}, {"real": [], "generated": []}

    def take(side, u8):
        f = fn(u8.float() / 255)
        if f.dim() != 2 or f.dtype != torch.float32:
            raise ValueError(f"sample_quality_eval: the feature function must return fp32 [B, d], got {f.dtype} {tuple(f.shape)}")
        if side not in stats:
            stats[side] = FeatureStats(f.shape[1], device)
        stats[side].update(f)
        if kid is not None:
            kept[side].append(f)

    with torch.no_grad():
        for b in real_batches:
            images = (b[0] if isinstance(b, (tuple, list)) else b).to(device).float()
            take("real", (images.clamp(0, 1) * 255 + 0.5).to(torch.uint8))      # rounded: data that came from uint8 returns to it
        if "real" not in stats:
            raise ValueError("sample_quality_eval: no real batches")
        keep = (sampler.n_samples, sampler.global_first)
        try:
            sampler.set_shard(0, min(step, n_samples))
            with sampler._one_key():
                for first in range(0, n_samples, step):
                    count = min(step, n_samples - first)
                    sampler.set_shard(first, count)
                    tok = draw(sampler, count)
                    tok = tok.reshape(count, tok.shape[-2], tok.shape[-1])
                    take("generated", model.decode_tokens(tok, T, want_u8=True)[1])
        finally:
            sampler.n_samples, sampler.global_first = keep
        real, gen = stats["real"], stats["generated"]
        if real.d != gen.d:
            raise ValueError(f"sample_quality_eval: real features have d = {real.d}, generated d = {gen.d}")
        res = {"fd": frechet_distance(real, gen, "exact"), "fd_reference_convention": frechet_distance(real, gen, "reference"),
               "kd_mean": None, "kd_std": None, "n_real": real.n, "n_generated": gen.n, "d": real.d}
        if kid is not None:
            res["kd_mean"], res["kd_std"] = kernel_distance(torch.cat(kept["real"]), torch.cat(kept["generated"]), **kid)
    return res
