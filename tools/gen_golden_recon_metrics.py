"""Fixture F19 (tests/golden/f19_recon_metrics.npz): the reconstruction metrics of R/main.py:318-320 computed by the REAL
reference module (R/metric/pytorch_ssim/__init__.py, imported by path) and torch's F.mse_loss on the CPU in fp32, next to the
fp64 oracle values of both (tests/_recon_metric_oracle.py).

    python tools/gen_golden_recon_metrics.py [--out tests/golden/f19_recon_metrics.npz]

Stored (data only):
  * ``gaussian_11_1p5``, ``window_11_c1``, ``window_11_c3``: the reference's gaussian(11, 1.5) and create_window(11, 1) / (11, 3);
  * per case ``<name>/``: the inputs as small integers (``a`` uint8: k / 255 - 0.5; ``b`` int16: k / 4096 - 0.5, or uint8), ``ws``,
    the reference's fp32 ``SSIM(ws)(a, b)`` (``ref_ssim_mean``), ``SSIM(ws, size_average=False)(a, b)`` (``ref_ssim_per``),
    ``ssim(a, b, ws)`` (``ref_ssim_fn``) and ``F.mse_loss(a, b)`` (``ref_mse``), and the fp64 oracle's ``o_ssim_mean``,
    ``o_ssim_per``, ``o_mse``;
  * ``names``, ``torch_version``.
Reproducing it needs the reference tree; the tests only read the .npz."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)          # (not the package directory: its metric would shadow the reference's)

from oracle.gen_golden import REF, _load  # noqa: E402

synth = _load(os.path.join(ROOT, "spiking-diffusion_amd", "spkdiff", "synth.py"), "spk_synth")
orc = _load(os.path.join(ROOT, "tests", "_recon_metric_oracle.py"), "recon_metric_oracle")


def reference_ssim():
    path = os.path.join(REF, "metric", "pytorch_ssim", "__init__.py")
    spec = importlib.util.spec_from_file_location("ref_pytorch_ssim", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def u8(x01):
    return (x01.clamp(0, 1) * 255).round().to(torch.uint8).numpy()


def i16(x01):
    return (x01.clamp(0, 1) * 4096).round().to(torch.int16).numpy()


def blur_noise(x01, g, sigma=0.04):
    """A reconstruction-like copy: 3x3 box blur mixed in, plus Gaussian noise."""
    C = x01.shape[1]
    k = torch.full((C, 1, 3, 3), 1 / 9.0)
    y = 0.5 * x01 + 0.5 * F.conv2d(x01, k, padding=1, groups=C)
    return y + sigma * torch.randn(x01.shape, generator=g)


def cases():
    g = torch.Generator().manual_seed(1907)
    s28 = synth.stroke_images(32, seed=77)
    out = {}
    out["strokes_blur"] = (u8(s28), i16(blur_noise(s28, g)), 11)
    out["strokes_noise"] = (u8(s28), i16(torch.rand(s28.shape, generator=g)), 11)
    out["identical"] = (u8(s28[:8]), u8(s28[:8]), 11)
    out["constant"] = (np.full((4, 1, 28, 28), 178, np.uint8), np.full((4, 1, 28, 28), 2300, np.int16), 11)
    s32 = synth.stroke_images(7, seed=78, img=32, channels=3)
    out["rgb32"] = (u8(s32), i16(blur_noise(s32, g)), 11)
    s23 = synth.stroke_images(5, seed=79, img=23, channels=2)[:, :, 2:21, :].contiguous()
    out["c2_19x23_w7"] = (u8(s23), i16(blur_noise(s23, g)), 7)
    out["even_w8"] = (u8(s28[8:11]), i16(blur_noise(s28[8:11], g)), 8)
    s9 = synth.stroke_images(2, seed=80, img=9)
    out["small9_w11"] = (u8(s9), i16(blur_noise(s9, g, 0.08)), 11)
    assert tuple(out) == orc.CASES
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "f19_recon_metrics.npz"))
    args = ap.parse_args()
    torch.manual_seed(0)
    ref = reference_ssim()
    f = {"gaussian_11_1p5": ref.gaussian(11, 1.5).numpy(), "window_11_c1": ref.create_window(11, 1).numpy(),
         "window_11_c3": ref.create_window(11, 3).numpy()}
    for name, (ka, kb, ws) in cases().items():
        a, b = orc.rebuild(ka), orc.rebuild(kb)
        w2d = ref.create_window(ws, 1)[0, 0]
        o_mean, o_per = orc.ssim64(a, b, w2d)
        with torch.no_grad():
            f[f"{name}/a"], f[f"{name}/b"], f[f"{name}/ws"] = ka, kb, np.array(ws)
            f[f"{name}/ref_ssim_mean"] = ref.SSIM(window_size=ws)(a, b).numpy()
            f[f"{name}/ref_ssim_per"] = ref.SSIM(window_size=ws, size_average=False)(a, b).numpy()
            f[f"{name}/ref_ssim_fn"] = ref.ssim(a, b, ws).numpy()
            f[f"{name}/ref_mse"] = F.mse_loss(a, b).numpy()
        f[f"{name}/o_ssim_mean"], f[f"{name}/o_ssim_per"] = o_mean.numpy(), o_per.numpy()
        f[f"{name}/o_mse"] = orc.mse64(a, b).numpy()
        print(f"{name}: {tuple(a.shape)} ws {ws}  ssim ref {float(f[name + '/ref_ssim_mean']):.9f} oracle {float(o_mean):.12f} "
              f"|r-o| {abs(float(f[name + '/ref_ssim_mean']) - float(o_mean)):.2e}  mse ref {float(f[name + '/ref_mse']):.9f} "
              f"|r-o| {abs(float(f[name + '/ref_mse']) - float(f[name + '/o_mse'])):.2e}")
    f["names"] = np.array(list(orc.CASES))
    f["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(args.out, **f)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
