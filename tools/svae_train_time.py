"""Per-iteration time of the SNN_VAE baseline's training step on HIP: R/main.py:118-146 -- forward (train()), backward,
AdamW step, reset_net, host draws included -- at B in {32, 256} (synthetic weights, p = 0 as R/main.py runs, HIP events
around each iteration after warm-up, median of N), with the library entry points one iteration makes.  ``--reference`` times
the real reference's iteration on the CPU with 16 threads instead (needs the reference tree, ``--ref``).

    python tools/svae_train_time.py [--iters 20]
    python tools/svae_train_time.py --reference --ref /path/to/Spiking-Diffusion-release
    rocprofv3 --kernel-trace --stats -- python tools/svae_train_time.py --iters 5      (kernel launches per iteration)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_step(model, functional, x, img):
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-3)

    def step():
        opt.zero_grad()
        loss_mmd, loss_rec = model(x, img)
        (loss_mmd + loss_rec).backward()
        opt.step()
        functional.reset_net(model)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reference", action="store_true", help="time the reference on the CPU (16 threads) instead")
    ap.add_argument("--ref", default=None, help="reference release directory (with --reference)")
    args = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd")]
    from spkdiff import synth
    sd = synth.synth_svae_state()
    if not args.reference:
        from svae_time import count_entry_points
        from snn_model.vae_model import SNN_VAE, functional
        model = SNN_VAE()
        functional.set_step_mode(model, 'm')
        model = model.cuda(0)
        model.load_state_dict(sd)
        model.train()
        for B in (32, 256):
            img = (synth.stroke_images(B) - 0.5).cuda(0)
            x = img.unsqueeze(0).repeat(16, 1, 1, 1, 1).contiguous()
            step = make_step(model, functional, x, img)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            calls = count_entry_points(step)
            row = {"call": f"train iteration B={B}", "ms": round(statistics.median(times), 3),
                   "images_per_s": round(B / statistics.median(times) * 1e3, 1), "lib_calls": sum(calls.values()),
                   "ar_prefix_launches": calls.get("spk_svae_ar_prefix_fwd", 0), "entry_points": calls}
            print(json.dumps(row), flush=True)
        return
    torch.set_num_threads(16)
    sys.path.insert(0, ROOT)
    for m in [m for m in sys.modules if m.split(".")[0] in ("snn_model", "spikingjelly")]:
        del sys.modules[m]
    sys.path.remove(os.path.join(ROOT, "spiking-diffusion_amd"))
    import oracle.gen_golden as gg
    if args.ref:
        gg.REF = args.ref
    vm, _ = gg._import_reference()
    ref = vm.SNN_VAE()
    vm.functional.set_step_mode(ref, 'm')
    ref.load_state_dict(sd)
    ref.train()
    for B in (32, 256):
        img = synth.stroke_images(B) - 0.5
        x = img.unsqueeze(0).repeat(16, 1, 1, 1, 1)
        step = make_step(ref, vm.functional, x, img)
        step()
        times = []
        for _ in range(max(1, min(args.iters, 3))):
            t0 = time.perf_counter()
            step()
            times.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"call": f"reference CPU train iteration B={B}, 16 threads", "ms": round(statistics.median(times), 1),
                          "images_per_s": round(B / statistics.median(times) * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
