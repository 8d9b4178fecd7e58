"""Oracle of the teacher-forced reverse process (``AbsorbingDiffusion.score``, spk_pscore_step): the reference's
loop (R/snn_model/vq_diffusion.py:110-140) with the token written at a revealed position taken from the given x_0 and its
log-probability under softmax(logits / temp) kept.  Host only, a checker: the step in numpy fp64 on the fp32 quotient
logits / temp (the value the sampler races with), the loop over any ``logits_fn`` and over ``oracle.snn_ref.denoiser_forward``.
The noise comes from the caller, as in tests/_completion_oracle.py; only u is read."""
import numpy as np
import torch

import _completion_oracle as corc
from oracle import snn_ref as ref


def log_prob(z32, tok):
    """log softmax(z)[tok] for one row z (fp32: logits / temp): (z_tok - m) - log sum_k exp(z_k - m) in fp64, m = max_k z_k with
    NaN entries passed over (they reach the result through the sum).  A token outside the row gives -inf."""
    K = z32.shape[0]
    if not 0 <= tok < K:
        return -np.inf
    with np.errstate(all='ignore'):
        m = np.float64(np.fmax.reduce(z32, initial=np.float32(-np.inf)))
        z = z32.astype(np.float64)
        return (z[tok] - m) - np.log(np.sum(np.exp(z - m)))


def pscore_step(logits, x0, x_t, unmasked, t, temp, u, logp, step, images=None):
    """spk_pscore_step in numpy, in place on x_t int64 / unmasked bool / logp fp64 / step int32 (each [B, HW] or any shape with
    B*HW entries, C order).  logits fp32 [B,K,...] indexed by IMAGE; ``images``: the only images the step may touch (the active
    list of the elimination forms; an image outside it has no change by construction).  Returns the ``changes`` mask [B,HW]."""
    B, K = logits.shape[0], logits.shape[1]
    lg = np.ascontiguousarray(logits, dtype=np.float32).reshape(B, K, -1)
    HW = lg.shape[2]
    x0, x_t, unmasked, logp, step = (a.reshape(B, HW) for a in (x0, x_t, unmasked, logp, step))
    inv_t = np.float32(1.0) / np.float32(t)                                     # the kernels' fp32 expression
    changes = (np.asarray(u, dtype=np.float32).reshape(B, HW) < inv_t) & ~unmasked.astype(bool)
    if images is not None:
        row = np.zeros(B, dtype=bool)
        row[np.asarray(images, dtype=np.int64)] = True
        changes &= row[:, None]
    with np.errstate(all='ignore'):
        for b, p in np.argwhere(changes):
            logp[b, p] = log_prob(lg[b, :, p] / np.float32(temp), int(x0[b, p]))
    step[changes] = t
    x_t[changes] = x0[changes]
    unmasked[changes] = True
    return changes


def run_fn(logits_fn, x_0, known, steps, noise, K, mask_id=None, temp=1.0, record=None):
    """The teacher-forced loop over ``logits_fn(x_t int64 [B,1,h,w] torch, t) -> [B,K,h,w]``.  ``known`` None: the all-masked
    start; else the completion start state.  ``noise``: t -> u or (u, q), u [B,1,h,w].  ``record`` receives (t, x_t, unmasked)
    after every step.  Returns (position_log_prob fp64 [B,h,w], reveal_step int32 [B,h,w], x_t, unmasked [B,1,h,w] torch)."""
    mask_id = K if mask_id is None else mask_id
    B, h, w = x_0.shape[0], x_0.shape[-2], x_0.shape[-1]
    x0 = x_0.reshape(B, 1, h, w).long()
    if known is None:
        x_t, unmasked = torch.full_like(x0, mask_id), torch.zeros_like(x0).bool()
    else:
        x_t, unmasked = corc.start_state(x0, known, K, mask_id)
    x_t, unmasked = x_t.clone().numpy(), unmasked.clone().numpy()
    logp = np.zeros((B, h, w), dtype=np.float64)
    step = np.zeros((B, h, w), dtype=np.int32)
    for t in reversed(range(1, steps + 1)):
        u = noise(t)
        u = u[0] if isinstance(u, (tuple, list)) else u
        # the logits are read only where a position changes: the denoiser runs on the images the step touches (what the
        # elimination forms of the device do; the rows of the others stay NaN and are never read)
        touched = ((np.asarray(u, dtype=np.float32).reshape(B, -1) < np.float32(1.0) / np.float32(t)) & ~unmasked.reshape(B, -1)).any(1)
        logits = np.full((B, K, h, w), np.nan, dtype=np.float32)
        if touched.any():
            logits[touched] = np.asarray(logits_fn(torch.from_numpy(x_t[touched]), t), dtype=np.float32)
        pscore_step(logits, x0.numpy(), x_t, unmasked, t, temp, np.asarray(u), logp, step)
        if record is not None:
            record.append((t, torch.from_numpy(x_t.copy()), torch.from_numpy(unmasked.copy())))
    return logp, step, torch.from_numpy(x_t), torch.from_numpy(unmasked)


def run(sd, x_0, known, steps, noise, K=128, mask_id=None, temp=1.0, T=16, record=None, exact_conv=False):
    """``run_fn`` over the oracle denoiser (oracle/snn_ref.denoiser_forward on the state dict ``sd``), in the shape of
    tests/_completion_oracle.run."""
    def logits_fn(x_t, t):
        tt = torch.full((x_t.shape[0],), t, dtype=torch.long)
        return ref.denoiser_forward(x_t.float(), tt, sd, T, exact_conv=exact_conv).numpy()
    return run_fn(logits_fn, x_0, known, steps, noise, K, mask_id, temp, record)
