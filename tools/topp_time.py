"""Cost of nucleus (top-p) truncation in the sampler: the 49-step sample at B = 256, captured, dense form (the
fused step tail draws the tokens), on the synthetic and on the trained checkpoint, in two configurations

  (a) temps        ``sample(temp=<per-image vector>)``: the ``_temps`` kernels -- separate instantiations this feature leaves alone,
                   so the figure is comparable with the same run of a tree without the feature (which prints (a) only);
  (b) temps+top_p  ``sample_top_p(0.9, temp=<the same vector>)``: the ``_topp`` kernels.

Both replay one captured graph each; a timed pass is TP_CALLS (default 40) calls between two HIP events after a warm-up pass, and
the two configurations alternate TP_REPS (default 5) times so that (b) / (a) can be read against the spread of the repeats.  Before
the timing the tool checks that ``sample_top_p`` with every p = 1 gives the tokens of (a) under the same seed and that p = 0.9
changes them.

Every checkpoint runs in a child process of its own under a time limit (TP_LIMIT seconds, default 240); after a child that fails
or runs out of time nothing more is started.

usage: topp_time.py      (TP_CALLS=40 TP_REPS=5 TP_WEIGHTS=synthetic,trained TP_LIMIT=240)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, BATCH, TOP_P = 49, 256, 0.9


def timed_pass(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def child(weights):
    sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd"), ROOT]
    import torch
    sys.argv = ["bench.py"]
    import bench
    import snn_model.vq_diffusion as vqd
    calls, reps = int(os.environ.get("TP_CALLS", "40")), int(os.environ.get("TP_REPS", "5"))
    dev = torch.device("cuda", 0)
    _, den, ab0 = bench.build_models(dev, 16, weights=weights)
    assert list(ab0.shape) == [7, 7]

    def new_sampler():
        ab = vqd.AbsorbingDiffusion(den, mask_id=ab0.mask_id, latent_shape=tuple(ab0.shape))
        ab.n_samples, ab.skip_untouched = BATCH, False
        assert ab.form_for(BATCH, 7, 7) == "dense_step_tail"
        return ab
    g = torch.Generator().manual_seed(7)
    temps = (0.5 + torch.rand(BATCH, generator=g)).to(dev)           # per-image temperatures in [0.5, 1.5)
    ways = {"temps": (new_sampler(), lambda ab: ab.sample(temp=temps, sample_steps=STEPS))}
    if hasattr(vqd.AbsorbingDiffusion, "sample_top_p"):
        ways["temps+top_p"] = (new_sampler(), lambda ab: ab.sample_top_p(TOP_P, temp=temps, sample_steps=STEPS))
        torch.manual_seed(11)
        a = ways["temps"][1](ways["temps"][0])
        torch.manual_seed(11)
        z = ways["temps+top_p"][0].sample_top_p(torch.ones(BATCH, dtype=torch.float32, device=dev), temp=temps, sample_steps=STEPS)
        assert torch.equal(a, z), "p = 1 must give the untruncated tokens"
        torch.manual_seed(11)
        assert not torch.equal(a, ways["temps+top_p"][1](ways["temps+top_p"][0])), "top_p = 0.9 must change tokens"
    for ab, fn in ways.values():                                     # warm-up: capture + one pass
        timed_pass(lambda: fn(ab), calls)
        assert len(ab._graphs) == 1
    res = {name: [] for name in ways}
    for _ in range(reps):
        for name, (ab, fn) in ways.items():
            res[name].append(timed_pass(lambda: fn(ab), calls))
    out = {name: dict(ms_per_sample=v, median=statistics.median(v), spread=max(v) - min(v)) for name, v in res.items()}
    if "temps+top_p" in out:
        out["ratio_b_over_a"] = [b / a for a, b in zip(res["temps"], res["temps+top_p"])]
    for name in ways:
        print(f"{weights:9s} {name:12s} B = {BATCH} x {STEPS} steps: " + " ".join(f"{v:7.3f}" for v in res[name]) +
              f" ms per sample, median {out[name]['median']:.3f}, max - min {out[name]['spread']:.3f}", flush=True)
    if "ratio_b_over_a" in out:
        r = out["ratio_b_over_a"]
        print(f"{weights:9s} (b) / (a) per repeat: " + " ".join(f"{v:.4f}" for v in r) + f", median {statistics.median(r):.4f}", flush=True)
    print("TP_RESULT " + json.dumps({weights: out}), flush=True)
    return 0


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    limit = float(os.environ.get("TP_LIMIT", "240"))
    for weights in os.environ.get("TP_WEIGHTS", "synthetic,trained").split(","):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", weights], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f"topp_time: {weights} ran past its {limit:.0f} s limit; nothing more is started", flush=True)
            return 124
        if rc != 0:
            print(f"topp_time: {weights} ended with status {rc}; nothing more is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
