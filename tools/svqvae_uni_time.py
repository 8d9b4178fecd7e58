"""Per-call time of the SNN_VQVAE_uni baseline on HIP next to SNN_VQVAE on the same (synthetic) weights: the eval forward at
B in {32, 256} with the statistic's prints on and off, one training iteration at B = 32, and the codebook-usage statistic
alone (spk_vq_code_usage against the same statistic spelled with torch ops, R/snn_model/vae_model.py:705-716).  HIP events
around each call after warm-up, median of N; the prints go to a string buffer.

    python tools/svqvae_uni_time.py [--iters 20]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def time_gpu(fn, iters, warmup=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd")]
    from spkdiff import ops, synth
    from snn_model.vae_model import SNN_VQVAE, SNN_VQVAE_uni, functional
    sd = synth.synth_vqvae_state(synth.MNIST)
    sink = io.StringIO()

    def build(cls, print_usage=None):
        m = cls(1, 16, 128, torch.tensor(1.0))
        functional.set_step_mode(net=m, step_mode='m')
        m = m.cuda(0)
        m.load_state_dict(sd)
        if print_usage is not None:
            m.vq_layer.print_usage = print_usage
        return m.eval()

    vq, uni_on, uni_off = build(SNN_VQVAE), build(SNN_VQVAE_uni, True), build(SNN_VQVAE_uni, False)

    def row(**kw):
        print(json.dumps(kw), flush=True)

    for B in (32, 256):
        img = (synth.stroke_images(B) - 0.5).cuda(0)
        x = img.unsqueeze(0).repeat(16, 1, 1, 1, 1).contiguous()

        def fwd(m, stat=None):
            def f():
                with torch.inference_mode(), contextlib.redirect_stdout(sink):
                    idx = m(x, img)[2]
                    if stat is not None:
                        stat(idx)
                functional.reset_net(m)
                sink.seek(0)
                sink.truncate()
            return f

        def torch_stat_printed(idx):          # what the reference does after the forward: torch ops, then its prints
            u = ops.vq_code_usage_torch(idx, 128)
            print(u.hist, float(u.fid_loss))

        cases = (("SNN_VQVAE", fwd(vq)), ("SNN_VQVAE + torch-op statistic, printed", fwd(vq, torch_stat_printed)),
                 ("SNN_VQVAE_uni print_usage=True", fwd(uni_on)), ("SNN_VQVAE_uni print_usage=False", fwd(uni_off)))
        for name, fn in cases:
            row(call=f"eval forward({B})", model=name, ms=round(time_gpu(fn, args.iters), 4))
        with torch.inference_mode():
            idx = vq(x, img)[2]
        functional.reset_net(vq)
        row(call=f"statistic alone, N = {idx.numel()}", form="spk_vq_code_usage (one launch + memset)",
            ms=round(time_gpu(lambda: ops.vq_code_usage(idx, 128), args.iters), 4))
        row(call=f"statistic alone, N = {idx.numel()}", form="torch ops (vq_code_usage_torch)",
            ms=round(time_gpu(lambda: ops.vq_code_usage_torch(idx, 128), args.iters), 4))
        row(call=f"statistic alone, N = {idx.numel()}", form="spk_vq_code_usage + one device-to-host copy",
            ms=round(time_gpu(lambda: ops.vq_code_usage(idx, 128).packed.cpu(), args.iters), 4))

    B = 32
    img = (synth.stroke_images(B) - 0.5).cuda(0)
    x = img.unsqueeze(0).repeat(16, 1, 1, 1, 1).contiguous()

    def train(m):
        def f():
            with contextlib.redirect_stdout(sink):
                a, b, _ = m(x, img)
            (a + b).backward()
            functional.reset_net(m)
            m.zero_grad(set_to_none=True)
            sink.seek(0)
            sink.truncate()
        return f

    for name, m in (("SNN_VQVAE", vq), ("SNN_VQVAE_uni print_usage=True", uni_on), ("SNN_VQVAE_uni print_usage=False", uni_off)):
        m.train()
        row(call=f"train iteration({B})", model=name, ms=round(time_gpu(train(m), args.iters), 4))
        m.load_state_dict(sd)
        m.eval()


if __name__ == "__main__":
    main()
