"""Multi-GPU sampling: one process per GPU, the sampling batch is sharded by rank, every rank runs the whole
reverse diffusion + decode locally, and ONE all-gather of the finished uint8 images is the only collective
(RCCL over xGMI when the backend is "nccl").  Samples are independent -- eval BN uses running
statistics, LIF / VQ are per position -- so there is no other exchange step on this path.
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist


def env_world():
    """(rank, local_rank, world_size) from the torchrun environment; (0, 0, 1) when not launched by it."""
    return (int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)))


def init(backend: str | None = None):
    """Initialise torch.distributed from the environment (MASTER_ADDR/PORT, RANK, WORLD_SIZE). Idempotent."""
    rank, local_rank, world = env_world()
    if world > 1 and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local_rank, world


def shard_range(total: int, rank: int, world: int):
    """Contiguous shard [lo, hi) of ``total`` samples for ``rank``; the first ``total % world`` ranks get one more."""
    q, r = divmod(total, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def gather_images(local_u8: torch.Tensor, total: int | None = None) -> torch.Tensor:
    """All-gather uint8 images [b_local, C, H, W] from every rank into [total, C, H, W] in rank order.

    Equal shards use a single ``all_gather_into_tensor``; ragged shards are padded to the largest shard so that
    it is still one collective.  With world_size == 1 (or no process group) it returns the input."""
    if not (dist.is_available() and dist.is_initialized()):
        return local_u8
    world = dist.get_world_size()
    if total is None:
        total = local_u8.shape[0] * world
    sizes = [shard_range(total, r, world) for r in range(world)]
    bmax = max(hi - lo for lo, hi in sizes)
    send = local_u8.contiguous()
    if send.shape[0] != bmax:
        pad = torch.zeros((bmax - send.shape[0],) + tuple(send.shape[1:]), dtype=send.dtype, device=send.device)
        send = torch.cat((send, pad), 0)
    if send.is_cuda and dist.get_backend() == 'gloo':
        # gloo (CPU tests; several ranks sharing ONE device as a testing aid: RCCL refuses that) stages device tensors itself, and with work
        # still pending on the stream that staging took SECONDS per call when two processes shared a device (measured: 6.1 s per bench step
        # against 0.2 s): hand it host tensors -- the images are 784 bytes each
        host = torch.empty((world * bmax,) + tuple(send.shape[1:]), dtype=send.dtype)
        dist.all_gather_into_tensor(host, send.cpu())
        out = host.to(send.device)
    else:
        out = torch.empty((world * bmax,) + tuple(send.shape[1:]), dtype=send.dtype, device=send.device)
        dist.all_gather_into_tensor(out, send)
    if all(hi - lo == bmax for lo, hi in sizes):
        return out
    parts = [out[r * bmax: r * bmax + (hi - lo)] for r, (lo, hi) in enumerate(sizes)]
    return torch.cat(parts, 0)


def sample_images_sharded(generate_local, total: int, sampler=None):
    """``generate_local(lo, hi)`` -> uint8 [hi-lo, C, H, W] on this rank's device; returns all ``total`` images
    on every rank (rank order == sample order).

    ``sampler``: the ``AbsorbingDiffusion`` that ``generate_local`` samples from.  When given, ``sampler.set_shard(lo, hi - lo)``
    is called here, which is what makes the ranks one job ('global' noise layout: shared key, counters on the GLOBAL image index --
    the images do not depend on the split).  Without it ``generate_local`` MUST call ``set_shard(lo, hi - lo)`` itself: a sampler
    that never did draws per-rank noise (and warns)."""
    rank, world = (dist.get_rank(), dist.get_world_size()) if (dist.is_available() and dist.is_initialized()) else (0, 1)
    lo, hi = shard_range(total, rank, world)
    if sampler is not None:
        sampler.set_shard(lo, hi - lo)
    return gather_images(generate_local(lo, hi), total)


def _per_image(v):
    """Is ``v`` one entry per image of a job (to be sliced by shard), not one value for all of them?"""
    return isinstance(v, (list, tuple)) or (getattr(v, 'ndim', 0) == 1 and len(v) > 1)


def complete_images_sharded(model, sampler, images, keep, temp=1.0, sample_steps=None, T=16, paste=True, top_k=None, top_p=None,
                            confident=False, positions_per_step=None, schedule=None, selection_noise=None, remask=None):
    """``spkdiff.complete.complete_images`` of one job over the ranks: every rank holds the whole job's ``images`` / ``keep``,
    completes its ``shard_range`` of them as a shard of the job (``set_shard``: shared key, counters on the global image index,
    so the images do not depend on the split) and one gather returns all uint8 images [total, C, H, W] on every rank.
    ``temp``: a number, or one temperature per image of the whole job (every rank passes the whole vector; a rank uses its
    shard's slice).  ``top_k``: None, an int >= 1 or one k per image of the whole job, sliced in the same way
    (``spkdiff.complete.complete_images_top_k``); ``top_p``: None, a number in (0, 1] or one p per image of the
    whole job, sliced likewise (``spkdiff.complete.complete_images_top_p``).  ``confident``: every shard reveals
    in the order of the denoiser's confidence (``spkdiff.complete.complete_images_confident`` with the same ``temp`` / ``top_k`` /
    ``top_p``); False: the calls made before.  With ``confident``, ``sample_steps`` may be one step count per image of the whole
    job, sliced like ``temp``, and ``positions_per_step`` is handed on; every shard runs its own maximum, and an
    image is completed as its own count alone completes it, so the images still do not depend on the split.  ``schedule`` /
    ``selection_noise`` (with ``confident``): as sample_confident() takes them -- one value for the job, or one per
    image of the whole job (a list of per-image schedules, a list of noise scales), sliced like ``temp``; an image's tables are its
    own, so the split still changes nothing.  ``remask`` (with ``confident``): as sample_confident() takes it -- one
    int or one table for the job, or one per image of the whole job (a list of B entries or a 2-D array), sliced like ``temp``;
    remasking draws no new noise, so the split still changes nothing."""
    from .complete import complete_images, complete_images_confident, complete_images_top_k, complete_images_top_p
    per_image, per_image_k, per_image_p = _per_image(temp), _per_image(top_k), _per_image(top_p)
    per_image_s = confident and (isinstance(sample_steps, (list, tuple)) or getattr(sample_steps, 'ndim', 0) == 1)
    if positions_per_step is not None and not confident:
        raise ValueError("complete_images_sharded: positions_per_step belongs to confident=True")
    if (schedule is not None or selection_noise is not None) and not confident:
        raise ValueError("complete_images_sharded: schedule / selection_noise belong to confident=True")
    # a list of per-image schedules (names, None or tables) or a 2-D array of rows is sliced; one name or one table is not
    per_image_w = getattr(schedule, 'ndim', 0) == 2 or (isinstance(schedule, (list, tuple)) and any(
        v is None or isinstance(v, (str, list, tuple)) or getattr(v, 'ndim', 0) >= 1 for v in schedule))
    per_image_n = _per_image(selection_noise)
    if remask is not None and not confident:
        raise ValueError("complete_images_sharded: remask belongs to confident=True")
    per_image_r = getattr(remask, 'ndim', 0) == 2 or (isinstance(remask, (list, tuple)) and any(
        v is None or isinstance(v, (list, tuple)) or getattr(v, 'ndim', 0) >= 1 for v in remask))

    def generate_local(lo, hi):
        tl = temp[lo:hi] if per_image else temp
        if confident:
            return complete_images_confident(model, sampler, images[lo:hi], keep[lo:hi],
                                             sample_steps=sample_steps[lo:hi] if per_image_s else sample_steps, temp=tl, T=T,
                                             paste=paste, top_k=top_k[lo:hi] if per_image_k else top_k,
                                             top_p=top_p[lo:hi] if per_image_p else top_p,
                                             positions_per_step=positions_per_step,
                                             **({} if schedule is None and selection_noise is None else
                                                {'schedule': schedule[lo:hi] if per_image_w else schedule,
                                                 'selection_noise': selection_noise[lo:hi] if per_image_n else selection_noise}),
                                             **({} if remask is None else {'remask': remask[lo:hi] if per_image_r else remask})
                                             ).images_u8
        if top_p is not None:
            return complete_images_top_p(model, sampler, images[lo:hi], keep[lo:hi], top_p[lo:hi] if per_image_p else top_p, temp=tl,
                                         sample_steps=sample_steps, T=T, paste=paste,
                                         top_k=top_k[lo:hi] if per_image_k else top_k).images_u8
        if top_k is None:
            return complete_images(model, sampler, images[lo:hi], keep[lo:hi], temp=tl, sample_steps=sample_steps, T=T,
                                   paste=paste).images_u8
        return complete_images_top_k(model, sampler, images[lo:hi], keep[lo:hi], top_k[lo:hi] if per_image_k else top_k, temp=tl,
                                     sample_steps=sample_steps, T=T, paste=paste).images_u8
    return sample_images_sharded(generate_local, int(images.shape[0]), sampler=sampler)


def temperature_sweep_sharded(model, sampler, temps, n_per_temp, sample_steps=None, batch=256, T=16, top_k=None, top_p=None):
    """``spkdiff.evaluate.temperature_sweep`` of one job over the ranks: every rank runs its ``shard_range`` of the job's
    ``len(temps) * n_per_temp`` images (``temperature_sweep_range``: calls of at most ``batch`` images, one key for the whole
    job, broadcast from rank 0) and one gather returns the uint8 images [len(temps), n_per_temp, C, H, W] on every rank -- the
    images of the one-rank sweep under the same key.  ``top_k``: None, an int or one k per temperature (``temperature_sweep_top_k``);
    ``top_p``: None, a number or one p per temperature (``temperature_sweep_top_p``)."""
    from .evaluate import temperature_sweep_range
    G, n = len(temps), int(n_per_temp)
    keep = (sampler.n_samples, sampler.global_first)

    def generate_local(lo, hi):
        return temperature_sweep_range(model, sampler, temps, n, lo, hi, sample_steps=sample_steps, batch=batch, T=T, top_k=top_k,
                                       **({} if top_p is None else {'top_p': top_p}))[0]
    try:
        u8 = sample_images_sharded(generate_local, G * n, sampler=sampler)
    finally:
        sampler.n_samples, sampler.global_first = keep
    return u8.reshape((G, n) + tuple(u8.shape[1:]))


def _mix64(x: torch.Tensor) -> torch.Tensor:
    """splitmix64 finaliser on int64 tensors (two's-complement wrap-around arithmetic)."""
    x = (x ^ ((x >> 30) & 0x3FFFFFFFF)) * -4658895280553007687        # 0xBF58476D1CE4E5B9
    x = (x ^ ((x >> 27) & 0x1FFFFFFFFF)) * -7723592293110705685       # 0x94D049BB133111EB
    return x ^ ((x >> 31) & 0x1FFFFFFFF)


def token_checksum(tokens: torch.Tensor, first: int = 0) -> int:
    """Checksum of the tokens of images [first, first + n) of a job, as a sum over images of a hash of (GLOBAL image index,
    tokens): the partial sums of any split of the job add up (mod 2^64) to the same number, so an N-rank run, a 1-rank run
    and the oracle can be compared by one integer.  ``tokens``: integer tensor [n, ...] on any device."""
    t = tokens.reshape(tokens.shape[0], -1).to(torch.int64)
    n, m = t.shape
    w = _mix64(torch.arange(1, m + 1, dtype=torch.int64, device=t.device)) | 1
    row = ((t + 1) * w).sum(1)
    idx = torch.arange(first, first + n, dtype=torch.int64, device=t.device)
    return int(_mix64(row ^ _mix64(idx + 0x1234567)).sum().item())


def global_token_checksum(tokens_local: torch.Tensor, first: int) -> int:
    """``token_checksum`` of the whole job: every rank contributes the partial sum of its shard (one int64 all-reduce, outside
    any timed region).  Reported as a non-negative 63-bit integer."""
    part = token_checksum(tokens_local, first)
    if dist.is_available() and dist.is_initialized():        # (also at one rank: the collective path is the tested path)
        dev = tokens_local.device if dist.get_backend() == "nccl" else "cpu"
        v = torch.tensor([part], dtype=torch.int64, device=dev)
        dist.all_reduce(v)          # int64 sums wrap: the sum mod 2^64 does not depend on the split
        part = int(v.item())
    return part & 0x7FFFFFFFFFFFFFFF
