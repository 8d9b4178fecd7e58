"""Time of the reconstruction metrics of R/main.py:300-323 on HIP next to the loop as the script writes it.

  * per batch at B = 32 and 256 (1x28x28, window 11): the ``ops.ssim_mse`` launch against the torch-op restatement
    (``metric.pytorch_ssim.ssim_torch`` + ``F.mse_loss``) on the same device, HIP events around each call, median of N;
  * the whole loop over 313 batches (10 000 = 312 x 32 + 16 ``synth.stroke_images``, trained checkpoint):
    ``spkdiff.evaluate.reconstruction_eval`` against the literal loop (torch-op SSIM with its window rebuilt per batch, two
    ``.item()`` per batch), wall clock with a synchronise at both ends, median of ``--loops``; and the model calls alone.

    python tools/recon_eval_time.py [--iters 50] [--loops 3] [--batches 313]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def time_gpu(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def time_wall(fn, loops):
    fn()
    ms = []
    for _ in range(loops):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--batches", type=int, default=313)
    args = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd")]
    import metric.pytorch_ssim as ps
    from spkdiff import evaluate, ops, synth
    from snn_model.vae_model import SNN_VQVAE, functional
    dev = torch.device("cuda:0")

    def row(**kw):
        print(json.dumps(kw), flush=True)

    row(device=torch.cuda.get_device_name(0), shader_clock_ghz=round(ops.clock_probe(dev)["ghz_median"], 3))
    window = ps.create_window(11, 1).to(dev)
    w2d = window[0, 0].contiguous()
    for B in (32, 256):
        a = (synth.stroke_images(B, seed=1) - 0.5).to(dev)
        b = (a + 0.05 * torch.randn_like(a)).clamp(-0.5, 0.5)
        buf = ops.ssim_mse_ws(B, 1, 28, 28, 11, dev)
        out = torch.empty((2, B), dtype=torch.float64, device=dev)

        def torch_ops():
            with torch.inference_mode():
                return F.mse_loss(a, b), 1 - ps.ssim_torch(a, b, window, 11, 1)

        def torch_ops_as_written():                 # SSIM(window_size=11) built per batch: the window rebuilt and uploaded
            with torch.inference_mode():
                return F.mse_loss(a, b), 1 - ps.ssim_torch(a, b, ps.create_window(11, 1).to(dev), 11, 1)

        row(call=f"metrics of one batch, B = {B}", form="ops.ssim_mse (one launch), buffers reused",
            ms=round(time_gpu(lambda: ops.ssim_mse(a, b, w2d, ws=buf, out=out), args.iters), 4))
        row(call=f"metrics of one batch, B = {B}", form="ops.ssim_mse, buffers from the allocator",
            ms=round(time_gpu(lambda: ops.ssim_mse(a, b, w2d), args.iters), 4))
        slot = torch.empty(2, dtype=torch.float64, device=dev)

        def eval_step():                            # what reconstruction_eval adds to the model call per batch
            o = torch.empty((2, B), dtype=torch.float64, device=dev)
            ops.ssim_mse(a, b, w2d, out=o)
            torch.sum(o, dim=1, out=slot)

        row(call=f"metrics of one batch, B = {B}", form="ops.ssim_mse + the sum into the slot (reconstruction_eval's step)",
            ms=round(time_gpu(eval_step, args.iters), 4))
        row(call=f"metrics of one batch, B = {B}", form="torch ops (ssim_torch + mse_loss), window on the device",
            ms=round(time_gpu(torch_ops, args.iters), 4))
        row(call=f"metrics of one batch, B = {B}", form="torch ops, window rebuilt per batch (as main.py writes it)",
            ms=round(time_gpu(torch_ops_as_written, args.iters), 4))
        row(call=f"metrics of one batch, B = {B}", form="torch ops as written + two .item()",
            ms=round(time_gpu(lambda: [v.item() for v in torch_ops_as_written()], args.iters), 4))

    # the whole loop
    model = SNN_VQVAE(1, 16, 128, torch.tensor(1.0))
    functional.set_step_mode(net=model, step_mode='m')
    model.load_state_dict(synth.trained_state("vqvae"))
    model = model.cuda(0).eval()
    n_img = (args.batches - 1) * 32 + 16
    images = torch.cat([synth.stroke_images(min(2000, n_img - i), seed=50 + i) for i in range(0, n_img, 2000)])
    batches = [(images[i:i + 32], None) for i in range(0, n_img, 32)]

    def literal():
        loss_mse, loss_ssim = [], []
        for imgs, _ in batches:
            norm_images = (imgs - 0.5).cuda(0)
            with torch.inference_mode():
                images_spike = norm_images.unsqueeze(0).repeat(16, 1, 1, 1, 1)
                recon_images = model(images_spike, norm_images)[1]
                functional.reset_net(model)
                loss_mse.append(F.mse_loss(recon_images, norm_images).item())
                win = ps.create_window(11, 1).to(dev)
                loss_ssim.append((1 - ps.ssim_torch(recon_images, norm_images, win, 11, 1)).item())
        return evaluate.aggregate(loss_ssim, loss_mse)

    def model_only():
        for imgs, _ in batches:
            norm_images = (imgs - 0.5).cuda(0)
            with torch.inference_mode():
                model(norm_images.unsqueeze(0).repeat(16, 1, 1, 1, 1), norm_images)
                functional.reset_net(model)

    ms, res = time_wall(lambda: evaluate.reconstruction_eval(model, batches), args.loops)
    row(call=f"evaluation loop, {len(batches)} batches ({n_img} images)", form="evaluate.reconstruction_eval", ms=round(ms, 2),
        per_batch_us=round(ms * 1e3 / len(batches), 1), result=res)
    ms, res = time_wall(literal, args.loops)
    row(call=f"evaluation loop, {len(batches)} batches ({n_img} images)", form="literal loop (torch-op SSIM, two .item() per batch)",
        ms=round(ms, 2), per_batch_us=round(ms * 1e3 / len(batches), 1), result=res)
    ms, _ = time_wall(model_only, args.loops)
    row(call=f"evaluation loop, {len(batches)} batches ({n_img} images)", form="the model calls alone (upload, forward, reset_net)",
        ms=round(ms, 2), per_batch_us=round(ms * 1e3 / len(batches), 1))


if __name__ == "__main__":
    main()
