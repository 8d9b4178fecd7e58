"""What a reveal schedule and annealed selection noise cost: B = 256, captured, dense form (the fused step tail
draws the tokens), trained checkpoint, 8 / 12 / 16 steps.

  default        ``sample_confident(S)`` -- the `_conf` kernels, the calls made before the schedules existed
  linear         ``sample_confident(S, schedule='linear')`` -- the `_sched` kernels with the counts of ``default``, no noise drawn (a = 0
                 everywhere): what the kernel family and its two table inputs cost
  cosine         ``sample_confident(S, schedule='cosine')`` -- few tokens early, so more positions stay masked and draw a candidate
                 at every step: what the schedule itself costs
  cosine+noise   ``sample_confident(S, schedule='cosine', selection_noise=4.5)`` -- one Philox block and two logf per masked position

A window is CST_CALLS (default 10) calls between two HIP events after a warm-up window; the configurations alternate over
CST_WINDOWS (default 7) windows and the median is reported with the spread (max - min) of the windows beside it.  CST_TREE names
another checkout of this repository to import the package and bench.py from (its library built): run there, a tree that has no
``schedule=`` argument measures ``default`` alone -- the same call on the parent's kernels, to be compared with this tree's
``default`` within the spread.

The measurement runs in a child process under a time limit (CST_LIMIT seconds, default 300).

usage: confident_schedule_time.py      (CST_CALLS=10 CST_WINDOWS=7 CST_TREE= CST_LIMIT=300)"""
import inspect
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.environ.get("CST_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEP_COUNTS, BATCH, TAU = (8, 12, 16), 256, 4.5


def timed_window(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def child():
    sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd"), ROOT]
    import torch
    sys.argv = ["bench.py"]
    import bench
    import snn_model.vq_diffusion as vqd
    calls, windows = int(os.environ.get("CST_CALLS", "10")), int(os.environ.get("CST_WINDOWS", "7"))
    dev = torch.device("cuda", 0)
    _, den, ab0 = bench.build_models(dev, 16, weights="trained")
    assert list(ab0.shape) == [7, 7]
    scheduled = "schedule" in inspect.signature(vqd.AbsorbingDiffusion.sample_confident).parameters

    def new_sampler():
        ab = vqd.AbsorbingDiffusion(den, mask_id=ab0.mask_id, latent_shape=tuple(ab0.shape))
        ab.n_samples, ab.skip_untouched = BATCH, False
        assert ab.form_for(BATCH, 7, 7) == "dense_step_tail"
        return ab
    configs = {"default": {}}
    if scheduled:
        configs["linear"] = dict(schedule="linear")
        configs["cosine"] = dict(schedule="cosine")
        configs["cosine+noise"] = dict(schedule="cosine", selection_noise=TAU)
    ways = {}
    for s in STEP_COUNTS:                                            # (a sampler each: a sampler keeps two graphs)
        for name, kw in configs.items():
            ways[f"{name}@{s}"] = (new_sampler(), s, lambda ab, s=s, kw=kw: ab.sample_confident(s, **kw))
    for ab, _, fn in ways.values():                                  # warm-up: capture + one window
        timed_window(lambda: fn(ab), calls)
        assert len(ab._graphs) == 1
    res = {name: [] for name in ways}
    for _ in range(windows):
        for name, (ab, _, fn) in ways.items():
            res[name].append(timed_window(lambda: fn(ab), calls))
    out = {}
    for name, (_, s, _) in ways.items():
        med = statistics.median(res[name])
        out[name] = dict(ms_per_sample=res[name], median=med, spread=max(res[name]) - min(res[name]), steps=s, ms_per_step=med / s)
        print(f"{name:16s} B = {BATCH}: median {med:7.3f} ms per sample of {windows} windows (max - min {out[name]['spread']:.3f}), "
              f"{med / s:.4f} ms per step", flush=True)
    if scheduled:
        for s in STEP_COUNTS:
            d, li, c, n = (out[f"{k}@{s}"]["median"] for k in ("default", "linear", "cosine", "cosine+noise"))
            print(f"{s:2d} steps: linear / default {li / d:.4f}, cosine / default {c / d:.4f}, cosine+noise / default {n / d:.4f}, "
                  f"cosine+noise / cosine {n / c:.4f}", flush=True)
    print("CST_RESULT " + json.dumps({"tree": "this" if not os.environ.get("CST_TREE") else "CST_TREE", "scheduled": scheduled,
                                      "results": out}), flush=True)
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    limit = float(os.environ.get("CST_LIMIT", "300"))
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=limit).returncode
    except subprocess.TimeoutExpired:
        print(f"confident_schedule_time: ran past its {limit:.0f} s limit", flush=True)
        return 124
    if rc != 0:
        print(f"confident_schedule_time: ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
