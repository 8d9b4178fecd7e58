"""Time of ONE training iteration of the plain-CNN VQVAE baseline (R/main.py:130-142: zero_grad, model(images), (loss_eq +
loss_rec).backward(), AdamW step) on csrc/conv_train.hip + csrc/ann_vqvae_train.hip against the SAME weights on
the model's module path on the device (``fused_train = False``: the framework's operators under autograd, which is what the
class ran before the kernels), eager and as one captured graph (spkdiff.train.GraphedANNVQVAETrainStep for both paths).

The method of tools/ann_vqvae_time.py.  Per case: AVTT_CALLS (default 50) back-to-back iterations between two HIP events,
after a warm-up of the same length; the window is repeated AVTT_REPS (default 7) times, the four (path, mode) pairs alternating,
and the median microseconds per iteration is printed with its min and max.  The shader clock the device holds
(spk_clock_probe) is printed first and last.  Shapes: B = 32 (the reference's batch) and 256, MNIST shape with K = 128 and
CIFAR shape with K = 256.

Launch counts come from a kernel trace of the tool in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/ann_vqvae_train_time.py --trace
    python tools/ann_vqvae_train_time.py --summarize <dir>/.../*_kernel_trace.csv
``--trace`` runs AVTT_TRACE_ITERS (default 10) eager iterations of each path at B = 32, MNIST shape, between clock-probe launches
(the markers the summary cuts at); ``--summarize`` prints launches and kernel time per iteration and the per-kernel table of
both paths.

usage: ann_vqvae_train_time.py [--trace | --summarize CSV]      (AVTT_BATCHES="32 256" AVTT_SHAPES="mnist:128 cifar:256")"""
import collections
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd"), ROOT]


# The module path is not captured where spkdiff.train.GraphedANNVQVAETrainStep refuses it: above this many quantiser rows the
# framework's embedding backward sorts its indices, and the replay of a graph captured over that form ended in a GPU memory fault
# on the MI355X (B = 256, 12544 rows).  The HIP path has no such launch.
def _sort_rows():
    from spkdiff.train import GraphedANNVQVAETrainStep
    return GraphedANNVQVAETrainStep.MODULE_PATH_MAX_ROWS


def window(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def make(cfg, K, dev, fused):
    import torch
    from snn_model.vae_model import VQVAE
    from spkdiff import synth
    m = VQVAE(cfg.in_dim, cfg.latent_dim, K, torch.tensor(0.0625))
    m.load_state_dict(synth.synth_ann_vqvae_state(cfg, K=K))
    m = m.to(dev).train()
    m.fused_train = fused
    return m, torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)


def eager_step(m, opt, x):
    def step():
        opt.zero_grad(set_to_none=True)
        loss_eq, loss_rec, _ = m(x)
        (loss_eq + loss_rec).backward()
        opt.step()
    return step


def time_main():
    import torch
    from spkdiff import ops, synth
    from spkdiff.train import GraphedANNVQVAETrainStep
    assert torch.cuda.is_available(), "ann_vqvae_train_time.py needs a ROCm device"
    dev = torch.device("cuda", 0)
    calls, reps = int(os.environ.get("AVTT_CALLS", "50")), int(os.environ.get("AVTT_REPS", "7"))
    print("clock before: " + json.dumps(ops.clock_probe(dev)), flush=True)
    for shape in os.environ.get("AVTT_SHAPES", "mnist:128 cifar:256").split():
        name, K = shape.split(":")
        cfg, K = {"mnist": synth.MNIST, "cifar": synth.CIFAR}[name], int(K)
        for B in (int(b) for b in os.environ.get("AVTT_BATCHES", "32 256").split()):
            x = (synth.stroke_images(B, img=cfg.img, channels=cfg.in_dim) - 0.5).to(dev)
            work, keep = {}, []
            for path, fused in (("hip", True), ("module", False)):
                m, opt = make(cfg, K, dev, fused)
                assert m._train_fused(x) is fused
                work[path, "eager"] = eager_step(m, opt, x)
                if path == "module" and B * cfg.latent * cfg.latent > _sort_rows():
                    continue                                        # (see _sort_rows)
                m2, opt2 = make(cfg, K, dev, fused)
                g = GraphedANNVQVAETrainStep(m2, opt2, x)
                keep.append(g)                                      # (the graph reads g's input, model and optimizer state)
                work[path, "captured"] = g.graph.replay
            us = {k: [] for k in work}
            for k, fn in work.items():
                window(fn, calls)                                   # warm-up of this path at this shape
            for _ in range(reps):
                for k, fn in work.items():                          # alternating: a drift of the device hits every pair alike
                    us[k].append(window(fn, calls))
            med = {k: statistics.median(v) for k, v in us.items()}
            for mode in ("eager", "captured"):
                both = ("module", mode) in med
                print(f"{name} K={K} B={B:4d} {mode:9s} "
                      + "  ".join(f"{p}: {med[p, mode]:8.1f} us/iteration (min {min(us[p, mode]):.1f} max {max(us[p, mode]):.1f})"
                                  for p in ("hip", "module") if (p, mode) in med)
                      + (f"  module/hip {med['module', mode] / med['hip', mode]:.2f}x" if both else
                         f"  module: not captured (its embedding backward sorts above {_sort_rows()} rows)")
                      + f"  n={reps}x{calls}", flush=True)
    print("clock after: " + json.dumps(ops.clock_probe(dev)), flush=True)
    return 0


def trace_main():
    import torch
    from spkdiff import ops, synth
    dev = torch.device("cuda", 0)
    cfg, K, B = synth.MNIST, 128, 32
    iters = int(os.environ.get("AVTT_TRACE_ITERS", "10"))
    x = (synth.stroke_images(B, img=cfg.img, channels=cfg.in_dim) - 0.5).to(dev)
    for path, fused in (("hip", True), ("module", False)):
        m, opt = make(cfg, K, dev, fused)
        step = eager_step(m, opt, x)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        ops.clock_probe(dev, target_ms=0.1)                         # marker: the iterations of this path start
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        ops.clock_probe(dev, target_ms=0.1)                         # marker: ... and end
        print(f"traced {iters} eager iterations of the {path} path (B = {B}, MNIST shape, K = {K})", flush=True)
    return 0


def summarize(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "clock_probe" in r["Kernel_Name"]]
    assert len(marks) == 4, f"expected four marker launches in {path}, found {len(marks)}"
    iters = int(os.environ.get("AVTT_TRACE_ITERS", "10"))

    def short(n):
        return n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:72]

    for name, (a, b) in (("hip", marks[0:2]), ("module", marks[2:4])):
        seg = rows[a + 1:b]
        d = collections.OrderedDict()
        for r in seg:
            d.setdefault(short(r["Kernel_Name"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        tot = sum(sum(v) for v in d.values())
        span = (int(seg[-1]["End_Timestamp"]) - int(seg[0]["Start_Timestamp"])) / 1e3
        print(f"{name} path: {len(seg) / iters:.1f} launches, {tot / iters:.1f} us of kernels, {span / iters:.1f} us from the first "
              f"launch to the last per iteration ({iters} eager iterations, B = 32, MNIST shape)")
        print("| kernel | launches / iteration | avg us | us / iteration | % |\n|---|---|---|---|---|")
        for k, v in sorted(d.items(), key=lambda kv: -sum(kv[1]))[:20]:
            print(f"| `{k}` | {len(v) / iters:.1f} | {sum(v) / len(v):.1f} | {sum(v) / iters:.1f} | {sum(v) / tot * 100:.1f} |")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        sys.exit(summarize(sys.argv[2]))
    sys.exit(trace_main() if "--trace" in sys.argv[1:] else time_main())
