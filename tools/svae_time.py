"""Per-call time of the SNN_VAE baseline on HIP: ``sample(B)`` and the eval ``forward`` at B in {32, 256} (synthetic weights,
HIP events around each call after warm-up, median of N), the library entry points each call makes, and the reference's
CPU time at the same B on 16 threads when the reference tree is available.

    python tools/svae_time.py [--iters 20] [--ref /path/to/Spiking-Diffusion-release]
    rocprofv3 --kernel-trace --stats -- python tools/svae_time.py      (kernel launches per call)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def count_entry_points(fn):
    """Calls into libspkdiff made by fn() (each one enqueues one or more kernels)."""
    from spkdiff import _lib
    counts = {}
    saved = {n: getattr(_lib.lib, n) for n in _lib.EXPORTS}

    def wrap(n, f):
        def w(*a):
            counts[n] = counts.get(n, 0) + 1
            return f(*a)
        return w
    try:
        for n, f in saved.items():
            setattr(_lib.lib, n, wrap(n, f))
        fn()
    finally:
        for n, f in saved.items():
            setattr(_lib.lib, n, f)
    return counts


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
    ap.add_argument("--ref", default=None, help="reference release directory: also time its CPU forward / sample")
    args = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd")]
    from spkdiff import synth
    sd = synth.synth_svae_state()
    if torch.cuda.is_available():
        from snn_model.vae_model import SNN_VAE, functional
        model = SNN_VAE()
        functional.set_step_mode(model, 'm')
        model = model.cuda(0)
        model.load_state_dict(sd)
        model.eval()
        rows = []
        for B in (32, 256):
            img = (synth.stroke_images(B) - 0.5).cuda(0)
            x = img.unsqueeze(0).repeat(16, 1, 1, 1, 1).contiguous()

            def fwd():
                with torch.inference_mode():
                    model(x, img)
                functional.reset_net(model)

            def smp():
                with torch.inference_mode():
                    model.sample(B)
                functional.reset_net(model)

            for name, fn in (("forward", fwd), ("sample", smp)):
                ms = time_gpu(fn, args.iters)
                calls = count_entry_points(fn)
                rows.append({"call": f"{name}({B})", "ms": round(ms, 3), "images_per_s": round(B / ms * 1e3, 1),
                             "lib_calls": sum(calls.values()), "ar_launches": calls.get("spk_svae_ar_fwd", 0),
                             "entry_points": calls})
                print(json.dumps(rows[-1]), flush=True)
    if args.ref:
        torch.set_num_threads(16)
        sys.path.insert(0, ROOT)
        for m in [m for m in sys.modules if m.split(".")[0] in ("snn_model", "spikingjelly")]:
            del sys.modules[m]
        sys.path.remove(os.path.join(ROOT, "spiking-diffusion_amd"))
        import oracle.gen_golden as gg
        gg.REF = args.ref
        vm, _ = gg._import_reference()
        ref = vm.SNN_VAE()
        vm.functional.set_step_mode(ref, 'm')
        ref.load_state_dict(sd)
        ref.eval()
        for B in (32, 256):
            img = synth.stroke_images(B) - 0.5
            x = img.unsqueeze(0).repeat(16, 1, 1, 1, 1)
            for name, fn in (("forward", lambda: ref(x, img)), ("sample", lambda: ref.sample(B))):
                with torch.inference_mode():
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                vm.functional.reset_net(ref)
                print(json.dumps({"call": f"reference CPU {name}({B}), 16 threads", "ms": round(dt, 1),
                                  "images_per_s": round(B / dt * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
