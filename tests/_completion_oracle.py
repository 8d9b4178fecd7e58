"""Oracle of the conditional (partly known start) reverse process and of the two completion kernels: the reference's loop
(R/snn_model/vq_diffusion.py:110-140) as restated in oracle/snn_ref.py -- ``denoiser_forward`` + ``p_sample_step``, pinned to the
real reference by fixtures F5 / F6 / F13 -- started from

    unmasked = known & (0 <= x_init < K),   x_t = where(unmasked, x_init, mask_id)

instead of the all-masked state.  Host tensors only; the noise comes from the caller (``ops.philox_noise`` dumps on the GPU,
``oracle/philox_ref.step_noise`` on the CPU)."""
import numpy as np
import torch

from oracle import snn_ref as ref

STEP_STRIDE = 1 << 40          # Philox counters of one reverse step ('global' layout)


def start_state(x_init, known, K, mask_id):
    """(x_t, unmasked) [B,1,h,w] of a conditional call from x_init / known ([B,1,h,w] or [B,h,w])."""
    B, h, w = x_init.shape[0], x_init.shape[-2], x_init.shape[-1]
    x = x_init.reshape(B, 1, h, w).long()
    unmasked = known.reshape(B, 1, h, w).bool() & (x >= 0) & (x < K)
    return torch.where(unmasked, x, torch.full_like(x, mask_id)), unmasked


def state_from_mask(codes, keep, K, mask_id, stride, radius):
    """spk_completion_state in torch: token (i,j) is known iff every mask byte in rows stride*i - radius .. stride*i + radius and
    the same columns, clipped to the mask, is non-zero, and the code is inside [0, K).  codes [B,h,w], keep [B,Hm,Wm] ->
    (x_t int64 [B,1,h,w], unmasked bool [B,1,h,w], n_known int32 [B])."""
    B, h, w = codes.shape
    # a minimum over the clipped window == min-pool with the outside padded by "given"
    m = torch.nn.functional.pad((keep != 0).float(), (radius, radius, radius, radius), value=1.0)
    win = -torch.nn.functional.max_pool2d(-m.unsqueeze(1), 2 * radius + 1, stride=1)[:, 0]        # [B,Hm,Wm]: min over the window
    known = win[:, 0:stride * (h - 1) + 1:stride, 0:stride * (w - 1) + 1:stride] > 0.5
    x_t, unmasked = start_state(codes, known, K, mask_id)
    return x_t, unmasked, unmasked.flatten(1).sum(1).to(torch.int32)


def compose(images, keep, decoded_u8):
    """spk_completion_compose in numpy: R/main.py:401's conversion where the pixel is given, the decoder's uint8 elsewhere.
    images fp32 [B,C,H,W], keep [B,H,W], decoded uint8 [B,C,H,W] (numpy arrays)."""
    given = np.array(np.clip(images + np.float32(0.5), 0.0, 1.0) * 255, dtype=np.uint8)
    return np.where((keep != 0)[:, None], given, decoded_u8)


def issue_start(B, L=7, K=128):
    """The start state of the pinned job: tokens from one generator, per image (b % 4) the top three rows / the left four
    columns / a random half / only the centre 3x3 known."""
    g = torch.Generator().manual_seed(2024)
    x_init = torch.randint(0, K, (B, 1, L, L), generator=g)
    known = torch.zeros(B, 1, L, L, dtype=torch.bool)
    for b in range(B):
        m = b % 4
        if m == 0:
            known[b, :, :3] = True
        elif m == 1:
            known[b, :, :, :4] = True
        elif m == 2:
            known[b] = torch.rand(1, L, L, generator=g) < 0.5
        else:
            known[b, :, 2:5, 2:5] = True
    return x_init, known


def run(sd, x_init, known, steps, noise, K=128, mask_id=None, temp=1.0, T=16, record=None, exact_conv=False):
    """The conditional reverse process on the host.  ``noise``: callable t -> (u [B,1,h,w], q [B*h*w, K]) host tensors.
    ``record`` (a list) receives (t, x_t, unmasked) after every step.  Returns (x_t, unmasked)."""
    mask_id = K if mask_id is None else mask_id
    x_t, unmasked = start_state(x_init, known, K, mask_id)
    B = x_t.shape[0]
    for t in reversed(range(1, steps + 1)):
        u, q = noise(t)
        tt = torch.full((B,), t, dtype=torch.long)
        logits = ref.denoiser_forward(x_t.float(), tt, sd, T, exact_conv=exact_conv).permute(0, 2, 3, 1)
        x_t, unmasked = ref.p_sample_step(x_t, unmasked, logits, t, temp, u, q)
        if record is not None:
            record.append((t, x_t.clone(), unmasked.clone()))
    return x_t, unmasked


def host_philox_noise(key, steps, B, L, K, first=0):
    """Noise callable from oracle/philox_ref.step_noise at the sampler's counter offsets (CPU tests)."""
    from oracle import philox_ref

    def noise(t):
        n = philox_ref.step_noise(key, (steps - t) * STEP_STRIDE + first * L * L * K, B, L * L, K)
        return torch.from_numpy(n.u).view(B, 1, L, L), torch.from_numpy(n.q)
    return noise
