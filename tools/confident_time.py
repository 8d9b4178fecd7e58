"""The step-count trade of confidence-ordered decoding: B = 256, captured, dense form (the fused step tail draws
the tokens), on the synthetic and on the trained checkpoint.

  times     ``sample_confident`` at 8, 12, 16 and 49 steps against ``sample_top_p`` -- the coin's reveal, the same `_topp` kernel
            family -- at the same step counts, and against the 49-step ``sample()``; all with temperature 1, both truncating calls
            with top_p = CT_TOP_P (default 0.9) as a per-image vector.  A window is CT_CALLS (default 10) calls between two HIP
            events after a warm-up window; the configurations alternate over CT_WINDOWS (default 7) windows and the median is
            reported, with the spread of the windows beside it.
  per step  the same medians divided by the step count: the confident tail draws at EVERY masked position of a step, the coin's
            tail at the ones it reveals.
  bits/dim  ``score(tokens, sample_steps=49).bits_per_dim()`` of the tokens either rule generates at 8 steps without truncation
            (and of the 49-step ``sample()`` tokens), mean over CT_ORDERS (default 4) reveal orders.  This is the model's OWN
            likelihood bound of its samples under the 49-step coin process -- how typical the model finds them -- not a quality
            metric: no FID, IS or KID here.

Every checkpoint runs in a child process of its own under a time limit (CT_LIMIT seconds, default 300); after a child that fails
or runs out of time nothing more is started.

usage: confident_time.py      (CT_CALLS=10 CT_WINDOWS=7 CT_ORDERS=4 CT_TOP_P=0.9 CT_WEIGHTS=synthetic,trained CT_LIMIT=300)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_COUNTS, BATCH, FULL = (8, 12, 16, 49), 256, 49


def timed_window(fn, calls):
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
    calls, windows = int(os.environ.get("CT_CALLS", "10")), int(os.environ.get("CT_WINDOWS", "7"))
    orders, top_p = int(os.environ.get("CT_ORDERS", "4")), float(os.environ.get("CT_TOP_P", "0.9"))
    dev = torch.device("cuda", 0)
    _, den, ab0 = bench.build_models(dev, 16, weights=weights)
    assert list(ab0.shape) == [7, 7]

    def new_sampler():
        ab = vqd.AbsorbingDiffusion(den, mask_id=ab0.mask_id, latent_shape=tuple(ab0.shape))
        ab.n_samples, ab.skip_untouched = BATCH, False
        assert ab.form_for(BATCH, 7, 7) == "dense_step_tail"
        return ab
    pv = torch.full((BATCH,), top_p, dtype=torch.float32, device=dev)
    ways = {}
    for s in STEP_COUNTS:                                            # (a sampler each: a sampler keeps two graphs)
        ways[f"confident@{s}"] = (new_sampler(), s, lambda ab, s=s: ab.sample_confident(s, top_p=pv))
        ways[f"top_p@{s}"] = (new_sampler(), s, lambda ab, s=s: ab.sample_top_p(pv, sample_steps=s))
    ways[f"sample@{FULL}"] = (new_sampler(), FULL, lambda ab: ab.sample(sample_steps=FULL))
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
        print(f"{weights:9s} {name:13s} B = {BATCH}: median {med:7.3f} ms per sample of {windows} windows (max - min "
              f"{out[name]['spread']:.3f}), {med / s:.4f} ms per step", flush=True)
    base = out[f"sample@{FULL}"]["median"]
    for s in STEP_COUNTS:
        c, p = out[f"confident@{s}"], out[f"top_p@{s}"]
        print(f"{weights:9s} {s:2d} steps: confident / top_p at equal steps {c['median'] / p['median']:.3f} (per step "
              f"{c['ms_per_step']:.4f} / {p['ms_per_step']:.4f} ms), confident / {FULL}-step sample() {c['median'] / base:.3f}", flush=True)
    # the model's own likelihood of what either rule generates at 8 steps (untruncated draws), under the 49-step coin process
    scorer = new_sampler()
    bpd = {}
    gens = {"confident@8": lambda ab: ab.sample_confident(8), "coin@8": lambda ab: ab.sample(sample_steps=8),
            f"coin@{FULL}": lambda ab: ab.sample(sample_steps=FULL)}
    for name, gen in gens.items():
        torch.manual_seed(11)
        tok = gen(new_sampler())
        assert int(tok.max()) < int(ab0.mask_id)
        torch.manual_seed(12)
        bpd[name] = float(scorer.score(tok, sample_steps=FULL, orders=orders).bits_per_dim())
        print(f"{weights:9s} bits/dim of the {name} tokens under score(sample_steps={FULL}, orders={orders}): {bpd[name]:.4f}"
              "   (the model's own likelihood of its samples, not a quality metric)", flush=True)
    out["bits_per_dim"] = bpd
    print("CT_RESULT " + json.dumps({weights: out}), flush=True)
    return 0


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    limit = float(os.environ.get("CT_LIMIT", "300"))
    for weights in os.environ.get("CT_WEIGHTS", "synthetic,trained").split(","):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", weights], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f"confident_time: {weights} ran past its {limit:.0f} s limit; nothing more is started", flush=True)
            return 124
        if rc != 0:
            print(f"confident_time: {weights} ended with status {rc}; nothing more is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
