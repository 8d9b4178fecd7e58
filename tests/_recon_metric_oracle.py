"""fp64 oracle of the reconstruction metrics (tests/test_recon_metrics_host.py, tests/test_gpu_recon_metrics.py; fixture F19
is written with it by tools/gen_golden_recon_metrics.py): torch CPU fp64, the SSIM formula of R/metric/pytorch_ssim/__init__.py:17-39
and F.mse_loss on the fp32 inputs with the fp32 window values, both widened.  A test-side restatement, not the code under test.

Bounds (derived, not measured).  ``o``: the oracle value of a result, ``r``: the reference's fp32 value in F19.
  * HIP path:  |hip - o| <= 2^-23 |o| + 1e-10.  The kernel's fp64 window sums differ from the oracle's in order only (relative
    ~1e-13 per map); the SSIM denominator amplifies that by at most 0.25 / 9e-4 ~ 300, which stays below 1e-10; the final
    rounding to fp32 is 2^-24 relative.
  * against the reference (triangle inequality):  |hip - r| <= |r - o| + 2^-23 |o| + 1e-10.
  * the torch-op path on the CPU, fp32 like the reference:  |cpu - o| <= 2 |r - o| + 2^-23 |o|."""
import numpy as np
import torch
import torch.nn.functional as F

C1 = 0.01 ** 2
C2 = 0.03 ** 2
EPS32 = 2.0 ** -23

CASES = ("strokes_blur", "strokes_noise", "identical", "constant", "rgb32", "c2_19x23_w7", "even_w8", "small9_w11")


def from_u8(k):
    """uint8 k -> fp32 k / 255 - 0.5 (the fixture's inputs, rebuilt with these two fp32 operations)."""
    return torch.from_numpy(np.asarray(k).astype(np.float32)) / 255 - 0.5


def from_i16(k):
    """int16 k -> fp32 k / 4096 - 0.5 (the perturbed copies)."""
    return torch.from_numpy(np.asarray(k).astype(np.float32)) / 4096 - 0.5


def rebuild(k):
    return from_u8(k) if np.asarray(k).dtype == np.uint8 else from_i16(k)


def ssim_map64(a, b, window2d):
    """fp64 SSIM map [N,C,H',W'] of fp32 a, b [N,C,H,W] under the fp32 window [ws,ws]."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    C = a.shape[1]
    ws = window2d.shape[-1]
    w = window2d.detach().cpu().double().reshape(1, 1, ws, ws).expand(C, 1, ws, ws).contiguous()

    def win(x):
        return F.conv2d(x, w, padding=ws // 2, groups=C)

    mu1, mu2 = win(a), win(b)
    s11, s22, s12 = win(a * a) - mu1 * mu1, win(b * b) - mu2 * mu2, win(a * b) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))


def ssim64(a, b, window2d):
    """(mean over everything, per-image mean [N]) in fp64."""
    m = ssim_map64(a, b, window2d)
    return m.mean(), m.mean(dim=(1, 2, 3))


def mse64(a, b):
    d = a.detach().cpu().double() - b.detach().cpu().double()
    return (d * d).mean()


def sums64(a, b, window2d):
    """What ops.ssim_mse returns: (sum of the map per image, sum of squared differences per image), fp64 [N]."""
    d = a.detach().cpu().double() - b.detach().cpu().double()
    return ssim_map64(a, b, window2d).sum(dim=(1, 2, 3)), (d * d).sum(dim=(1, 2, 3))


def hip_bound(o):
    return EPS32 * np.abs(np.asarray(o, dtype=np.float64)) + 1e-10


def ref_bound(r, o):
    r, o = np.asarray(r, dtype=np.float64), np.asarray(o, dtype=np.float64)
    return np.abs(r - o) + hip_bound(o)


def cpu_bound(r, o):
    r, o = np.asarray(r, dtype=np.float64), np.asarray(o, dtype=np.float64)
    return 2 * np.abs(r - o) + EPS32 * np.abs(o)


def load_case(z, name):
    """One F19 case: inputs rebuilt to fp32 and its stored values."""
    g = lambda k: z[f"{name}/{k}"]     # noqa: E731
    return dict(a=rebuild(g("a")), b=rebuild(g("b")), ws=int(g("ws")),
                r_mean=g("ref_ssim_mean"), r_per=g("ref_ssim_per"), r_fn=g("ref_ssim_fn"), r_mse=g("ref_mse"),
                o_mean=g("o_ssim_mean"), o_per=g("o_ssim_per"), o_mse=g("o_mse"))
