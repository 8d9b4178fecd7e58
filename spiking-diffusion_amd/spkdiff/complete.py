"""Completion of partly given images (inpainting / outpainting): encode the image, keep the code indices
that no removed pixel reached, run the reverse process from that partly unmasked state, decode, paste the given pixels back.

A fixed launch sequence on the current stream; nothing is read back inside the call:

    model.encode_images -> spk_completion_state (4, 3) -> sampler.sample(x_init, known) -> model.decode_tokens
                        -> spk_completion_compose (``paste``)

The encoder is Conv 3x3 s2 p1, Conv 3x3 s2 p1, Conv 1x1 (R/snn_model/vae_model.py:101-129), so code (i, j) reads pixels
4i - 3 .. 4i + 3 in both directions (and the zero padding outside the image, which is given by definition).  A code is trusted
only if every pixel of that window is given: the result therefore does not depend on what the input holds inside the hole.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops

ENC_STRIDE, ENC_RADIUS = 4, 3          # the encoder's receptive field on the pixel grid: centre 4i, 3 pixels either side


class Completion(NamedTuple):
    images_u8: torch.Tensor            # uint8 [B,C,H,W]: the completed images
    tokens: torch.Tensor               # int64 [B,h,w]: the completed code indices
    known: torch.Tensor                # bool  [B,h,w]: the codes taken from the input
    n_known: torch.Tensor              # int32 [B]: their number per image


def _check_inputs(images, keep):
    if not isinstance(images, torch.Tensor) or not isinstance(keep, torch.Tensor):
        raise TypeError(f"images and keep must be torch.Tensors, got {type(images)} and {type(keep)}")
    if images.dim() != 4:
        raise ValueError(f"complete_images: images {tuple(images.shape)} must be [B,C,H,W]")
    B, C, H, W = (int(v) for v in images.shape)
    if keep.dim() == 4 and keep.shape[1] == 1:
        keep = keep[:, 0]
    if tuple(keep.shape) != (B, H, W):
        raise ValueError(f"complete_images: keep {tuple(keep.shape)} must be [{B},1,{H},{W}] or [{B},{H},{W}]")
    if keep.dtype not in (torch.bool, torch.uint8):
        raise NotImplementedError(f"spkdiff: keep must be bool or uint8, got {keep.dtype}")
    if H % 4 or W % 4:
        raise ValueError(f"complete_images: the encoder halves the image twice: H, W = {H}, {W} must be multiples of 4")
    images = ops._dev(images, "images", torch.float32)
    keep = ops._dev(keep, "keep")
    return images, keep


@torch.no_grad()
def complete_images(model, sampler, images, keep, temp=1.0, sample_steps=None, T=16, paste=True):
    """``images`` fp32 device tensor [B,C,H,W], normalised as everywhere (pixel - 0.5); ``keep`` bool / uint8 [B,1,H,W] or
    [B,H,W], true = the pixel is given.  ``model``: the SNN_VQVAE, ``sampler``: the AbsorbingDiffusion of its latent shape.
    Returns a ``Completion`` of device tensors.  ``paste``: the given pixels of ``images_u8`` are the input's
    (uint8(clip(image + 0.5, 0, 1) * 255), R/main.py:401), the rest the decoder's; False: the decoder's image everywhere.
    ``temp``: a number or one temperature per image, as ``sample()`` takes it.
    One key draw from torch's global CPU generator, as every ``sample()`` call.  Top-k truncation: ``complete_images_top_k``; nucleus
    truncation: ``complete_images_top_p``."""
    return _complete(model, sampler, images, keep, temp, sample_steps, T, paste, None)


@torch.no_grad()
def complete_images_top_k(model, sampler, images, keep, top_k, temp=1.0, sample_steps=None, T=16, paste=True):
    """``complete_images`` with the unknown tokens drawn under top-k truncation: ``top_k`` is None, an int >= 1
    or one k per image (0: that image is not truncated), as ``AbsorbingDiffusion.sample_top_k`` takes it.  The known tokens are
    never drawn, so they come back unchanged whatever k is."""
    return _complete(model, sampler, images, keep, temp, sample_steps, T, paste, top_k)


@torch.no_grad()
def complete_images_top_p(model, sampler, images, keep, top_p, temp=1.0, sample_steps=None, T=16, paste=True, top_k=None):
    """``complete_images`` with the unknown tokens drawn under nucleus truncation: ``top_p`` is None, a number in
    (0, 1] or one p per image (1: that image is not truncated), as ``AbsorbingDiffusion.sample_top_p`` takes it, ``top_k`` the
    top-k truncation that precedes it.  The known tokens are never drawn, so they come back unchanged whatever p is."""
    return _complete(model, sampler, images, keep, temp, sample_steps, T, paste, top_k, top_p)


@torch.no_grad()
def complete_images_confident(model, sampler, images, keep, sample_steps=None, temp=1.0, T=16, paste=True, top_k=None, top_p=None,
                              positions_per_step=None, schedule=None, selection_noise=None, remask=None):
    """``complete_images`` with the unknown tokens revealed in the order of the denoiser's confidence (DESIGN.md §4.15;
    ``AbsorbingDiffusion.sample_confident``): every step commits the ceil(m / t) surest candidates of each image, m counting the
    positions still unknown, so a few steps serve a small hole.  ``temp`` / ``top_k`` / ``top_p`` as sample_confident() takes them.
    The known tokens are never drawn, so they come back unchanged; with nothing known the tokens are sample_confident()'s under
    the same key.
    ``sample_steps`` may be one step count per image, as sample_confident() takes it: image i is completed as
    ``sample_steps=s_i`` alone completes it, and every step evaluates the pending images only.  ``positions_per_step = r`` (an int
    >= 1; not together with ``sample_steps``) chooses the counts from the holes: s_i = max(1, ceil(m_i / r)) with m_i = h * w -
    n_known_i the number of unknown codes of image i, so every step commits at most r tokens per image, a 4-token hole takes one
    step beside a full image's 13 (r = 4, 7 x 7), and an image with nothing to fill is never evaluated.  It costs ONE host read
    (the ``n_known`` vector, B int32) ahead of the sampler call -- the only synchronisation of this function.
    ``schedule`` / ``selection_noise``: handed to sample_confident() as given -- how many of the unknown tokens a
    step commits ('cosine': few at first, most at the end) and how much annealed Gumbel noise their order carries; both None:
    the call made before.  The known tokens come back unchanged under every schedule and noise scale.
    ``remask``: handed to sample_confident() as given -- how many of the tokens earlier steps filled in each step
    returns to the masked state; the known tokens are never remasked and come back unchanged.  None: the call made before."""
    if positions_per_step is not None:
        if sample_steps is not None:
            raise ValueError("complete_images_confident: give sample_steps or positions_per_step, not both")
        if isinstance(positions_per_step, bool) or not isinstance(positions_per_step, int) or positions_per_step < 1:
            raise ValueError(f"complete_images_confident: positions_per_step must be an int >= 1, got {positions_per_step!r}")
    return _complete(model, sampler, images, keep, temp, sample_steps, T, paste, top_k, top_p, confident=True,
                     positions_per_step=positions_per_step,
                     **({} if schedule is None and selection_noise is None else {'schedule': schedule, 'selection_noise': selection_noise}),
                     **({} if remask is None else {'remask': remask}))


def steps_for_holes(n_unknown, positions_per_step):
    """s_i = max(1, ceil(m_i / r)): the step counts ``positions_per_step = r`` gives holes of ``n_unknown`` = m_i positions (an
    integer tensor; the result has its dtype and device)."""
    r = int(positions_per_step)
    return ((n_unknown + (r - 1)) // r).clamp(min=1)


def _complete(model, sampler, images, keep, temp, sample_steps, T, paste, top_k, top_p=None, confident=False, positions_per_step=None,
              **sched):
    images, keep = _check_inputs(images, keep)
    B, C, H, W = (int(v) for v in images.shape)
    h, w = H // 4, W // 4
    if [h, w] != [int(v) for v in sampler.shape]:
        raise ValueError(f"complete_images: {H}x{W} images encode to {h}x{w} codes, the sampler's shape is {list(sampler.shape)}")
    codes = model.encode_images(images, T)
    x_init, known, n_known = ops.completion_state(codes, keep, int(sampler.num_classes), int(sampler.mask_id), ENC_STRIDE,
                                                  ENC_RADIUS, want_counts=True)
    if positions_per_step is not None:
        sample_steps = steps_for_holes(h * w - n_known.cpu().to(torch.int64), positions_per_step)     # (the one host read)
    if confident:
        tokens = sampler.sample_confident(sample_steps=sample_steps, temp=temp, x_init=x_init, known=known, top_k=top_k, top_p=top_p,
                                          **sched)
    elif top_p is not None:
        tokens = sampler.sample_top_p(top_p, temp=temp, sample_steps=sample_steps, x_init=x_init, known=known, top_k=top_k)
    elif top_k is None:
        tokens = sampler.sample(temp=temp, sample_steps=sample_steps, x_init=x_init, known=known)
    else:
        tokens = sampler.sample_top_k(top_k, temp=temp, sample_steps=sample_steps, x_init=x_init, known=known)
    tokens = tokens.reshape(B, h, w)
    _, u8 = model.decode_tokens(tokens, T)
    if paste:
        u8 = ops.completion_compose(images, keep, u8)
    return Completion(u8, tokens, known.reshape(B, h, w), n_known)
