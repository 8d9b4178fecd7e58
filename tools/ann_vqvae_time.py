"""Time of the plain-CNN VQVAE baseline's eval path: ``encode_images``, ``decode_tokens`` and ``model(x)`` on
csrc/ann_vqvae.hip against the SAME weights on the model's module path on the device -- the framework's operators, which a
forward hook on a child selects and which is what the class would run without the kernels.

Per case: AVT_CALLS (default 200) back-to-back calls between two HIP events, after a warm-up of the same length; the window is
repeated AVT_REPS (default 7) times, the two paths alternating, and the median microseconds per call is printed with its min and
max.  Launch counts come from one profiled call of each path (torch.profiler's device kernels).  The shader clock the device
holds (spk_clock_probe) is printed first and last.

usage: ann_vqvae_time.py            (AVT_BATCHES="32 256" AVT_SHAPE=mnist|cifar AVT_K=128)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd"), ROOT]


def window(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def launches(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    import torch
    from snn_model.vae_model import VQVAE
    from spkdiff import ops, synth
    assert torch.cuda.is_available(), "ann_vqvae_time.py needs a ROCm device"
    dev = torch.device("cuda", 0)
    cfg = {"mnist": synth.MNIST, "cifar": synth.CIFAR}[os.environ.get("AVT_SHAPE", "mnist")]
    K = int(os.environ.get("AVT_K", "128"))
    calls, reps = int(os.environ.get("AVT_CALLS", "200")), int(os.environ.get("AVT_REPS", "7"))
    model = VQVAE(cfg.in_dim, cfg.latent_dim, K, torch.tensor(1.0))
    model.load_state_dict(synth.synth_ann_vqvae_state(cfg, K=K))
    model = model.to(dev).eval()
    print("clock before: " + json.dumps(ops.clock_probe(dev)), flush=True)
    for B in (int(b) for b in os.environ.get("AVT_BATCHES", "32 256").split()):
        x = (synth.stroke_images(B, img=cfg.img, channels=cfg.in_dim) - 0.5).to(dev)
        with torch.inference_mode():
            tok = model.encode_images(x)
            work = {"encode_images": lambda: model.encode_images(x), "decode_tokens": lambda: model.decode_tokens(tok),
                    "model(x)": lambda: model(x)}
            for name, fn in work.items():
                us = {"hip": [], "module": []}
                n_launch = {}
                for path in us:
                    handle = model.encoder.register_forward_hook(lambda m, i, o: None) if path == "module" else None
                    try:
                        try:
                            n_launch[path] = launches(fn)
                        except Exception as e:          # noqa: BLE001  (a profiler that cannot start is not a timing failure)
                            n_launch[path] = f"not measured ({type(e).__name__})"
                        window(fn, calls)               # warm-up of this path at this shape
                    finally:
                        if handle is not None:
                            handle.remove()
                for _ in range(reps):
                    for path in us:                     # alternating: a drift of the device hits both paths alike
                        handle = model.encoder.register_forward_hook(lambda m, i, o: None) if path == "module" else None
                        try:
                            us[path].append(window(fn, calls))
                        finally:
                            if handle is not None:
                                handle.remove()
                med = {p: statistics.median(v) for p, v in us.items()}
                print(f"{os.environ.get('AVT_SHAPE', 'mnist')} K={K} B={B:4d} {name:14s} "
                      + "  ".join(f"{p}: {med[p]:8.1f} us/call (min {min(us[p]):.1f} max {max(us[p]):.1f}, {n_launch[p]} launches)"
                                  for p in us)
                      + f"  module/hip {med['module'] / med['hip']:.2f}x  n={reps}x{calls}", flush=True)
    print("clock after: " + json.dumps(ops.clock_probe(dev)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
