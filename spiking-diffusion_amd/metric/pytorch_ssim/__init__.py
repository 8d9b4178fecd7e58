"""Drop-in ``metric.pytorch_ssim`` of the MI355X build (the names of R/metric/pytorch_ssim/__init__.py: ``gaussian``,
``create_window``, ``SSIM``, ``ssim``).

fp32 tensors on a ROCm device, with autograd off or no input requiring grad -- main.py's evaluation loop -- take one HIP launch
(``spkdiff.ops.ssim_mse``: fp64 arithmetic, deterministic) and return the fp32 value.  Every other call (CPU tensors, other
dtypes, inputs that require grad, a window above ``ops.SSIM_MAX_WINDOW``) takes ``ssim_torch``, the same formula with the
framework's operators in the inputs' dtype; it is also the host path and the baseline tools/recon_eval_time.py times."""
from math import exp

import torch
import torch.nn.functional as F

C1 = 0.01 ** 2
C2 = 0.03 ** 2


def gaussian(window_size, sigma):
    """Normalised 1-D Gaussian, fp32 [window_size], centred on window_size // 2 (R/metric/pytorch_ssim/__init__.py:7-9): the
    taps are evaluated in Python floats, rounded to fp32 and divided by their fp32 sum."""
    centre, denom = window_size // 2, float(2 * sigma ** 2)
    taps = torch.tensor([exp(-((k - centre) ** 2) / denom) for k in range(window_size)], dtype=torch.float32)
    return taps / taps.sum()


def create_window(window_size, channel):
    """The depthwise window fp32 [channel, 1, ws, ws]: the fp32 outer product fl(g[i] g[j]) of gaussian(ws, 1.5) (:11-15)."""
    g = gaussian(window_size, 1.5)
    return torch.outer(g, g).expand(channel, 1, window_size, window_size).contiguous()


def ssim_torch(img1, img2, window, window_size, channel, size_average=True):
    """SSIM with the framework's operators, as the reference spells it (:17-39): five depthwise window convolutions with
    zero padding ws // 2, the map, its mean (over everything, or per image over (C, H', W'))."""
    pad = window_size // 2

    def blur(x):
        return F.conv2d(x, window, padding=pad, groups=channel)

    mu1, mu2 = blur(img1), blur(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = blur(img1 * img1) - mu1_sq
    sigma2_sq = blur(img2 * img2) - mu2_sq
    sigma12 = blur(img1 * img2) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    if size_average:
        return ssim_map.mean()
    return ssim_map.mean(1).mean(1).mean(1)


def _hip_path(img1, img2, window, window_size):
    from spkdiff import ops
    return (img1.dim() == 4 and img1.is_cuda and img2.is_cuda and window.is_cuda
            and img1.dtype == img2.dtype == window.dtype == torch.float32
            and img1.shape == img2.shape and img1.numel() > 0 and 1 <= window_size <= ops.SSIM_MAX_WINDOW
            and not (torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad or window.requires_grad)))


def _ssim(img1, img2, window, window_size, channel, size_average=True):
    if not _hip_path(img1, img2, window, window_size):
        return ssim_torch(img1, img2, window, window_size, channel, size_average)
    from spkdiff import ops
    N, C, H, W = img1.shape
    ssim_sum, _ = ops.ssim_mse(img1, img2, window[0, 0])
    per_image = C * ops.ssim_mse_out_size(H, window_size) * ops.ssim_mse_out_size(W, window_size)
    if size_average:
        return (ssim_sum.sum() / (N * per_image)).float()
    return (ssim_sum / per_image).float()


def _window_like(img, window_size, channel):
    """create_window on the input's device and in its dtype."""
    window = create_window(window_size, channel)
    if img.is_cuda:
        window = window.cuda(img.get_device())
    return window.type_as(img)


class SSIM(torch.nn.Module):
    """SSIM(window_size=11, size_average=True)(img1, img2): attributes window_size, size_average, channel, window.  The
    cached window follows the channel count and the tensor type (dtype, cpu / device) of the last input, as the reference's
    forward does (:50-60)."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        self.window_size = window_size
        self.size_average = size_average
        self.channel = 1
        self.window = create_window(window_size, self.channel)

    def forward(self, img1, img2):
        channel = img1.size(1)
        if channel != self.channel or self.window.data.type() != img1.data.type():
            self.window = _window_like(img1, self.window_size, channel)
            self.channel = channel
        return _ssim(img1, img2, self.window, self.window_size, channel, self.size_average)


def ssim(img1, img2, window_size=11, size_average=True):
    channel = img1.size(1)
    return _ssim(img1, img2, _window_like(img1, window_size, channel), window_size, channel, size_average)
