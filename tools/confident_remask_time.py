"""What remasking costs: B = 256, captured, dense form (the fused step tail draws the tokens), trained checkpoint,
8 / 12 / 16 steps.

  default        ``sample_confident(S)`` -- the `_conf` kernels, the calls made before the argument existed
  sched          ``sample_confident(S, schedule='linear')`` -- the `_sched` kernels, the family remasking sits on
  remask0        ``sample_confident(S, remask=0)`` -- the `_remask` kernels with a zero table: what the kernel family, its table input,
                 the commit_conf buffer and its one initialising launch cost
  remask2 / 4    ``sample_confident(S, remask=2)`` / ``remask=4`` -- up to 2 / 4 tokens per image return to the masked state at every
                 step t >= 2 and draw again: more masked positions at every later step

A window is CRT_CALLS (default 10) calls between two HIP events after a warm-up window; the configurations alternate over
CRT_WINDOWS (default 7) windows and the median is reported with the spread (max - min) of the windows beside it.  CRT_TREE names
another checkout of this repository to import the package and bench.py from (its library built): run there, a tree that has no
``remask=`` argument measures ``default`` (and ``sched``) alone -- the same calls on the parent's kernels, to be compared with this
tree's within the spread.

Beside the times: ``score(tokens, 49 steps, orders=4)`` in bits per dimension of 8-step samples with and without remasking (CRT_BPD=0
leaves it out).  It is the model's own likelihood bound of its own samples, not a quality metric.

The measurement runs in a child process under a time limit (CRT_LIMIT seconds, default 300).

usage: confident_remask_time.py      (CRT_CALLS=10 CRT_WINDOWS=7 CRT_TREE= CRT_LIMIT=300 CRT_BPD=1)"""
import inspect
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.environ.get("CRT_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEP_COUNTS, BATCH = (8, 12, 16), 256


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
    calls, windows = int(os.environ.get("CRT_CALLS", "10")), int(os.environ.get("CRT_WINDOWS", "7"))
    dev = torch.device("cuda", 0)
    _, den, ab0 = bench.build_models(dev, 16, weights="trained")
    assert list(ab0.shape) == [7, 7]
    remasking = "remask" in inspect.signature(vqd.AbsorbingDiffusion.sample_confident).parameters

    def new_sampler():
        ab = vqd.AbsorbingDiffusion(den, mask_id=ab0.mask_id, latent_shape=tuple(ab0.shape))
        ab.n_samples, ab.skip_untouched = BATCH, False
        assert ab.form_for(BATCH, 7, 7) == "dense_step_tail"
        return ab
    configs = {"default": {}, "sched": dict(schedule="linear")}
    if remasking:
        configs.update(remask0=dict(remask=0), remask2=dict(remask=2), remask4=dict(remask=4))
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
        print(f"{name:12s} B = {BATCH}: median {med:7.3f} ms per sample of {windows} windows (max - min {out[name]['spread']:.3f}), "
              f"{med / s:.4f} ms per step; windows {' '.join(f'{v:.3f}' for v in res[name])}", flush=True)
    if remasking:
        for s in STEP_COUNTS:
            d, sc, r0, r2, r4 = (out[f"{k}@{s}"]["median"] for k in ("default", "sched", "remask0", "remask2", "remask4"))
            print(f"{s:2d} steps: sched / default {sc / d:.4f}, remask0 / sched {r0 / sc:.4f}, remask2 / remask0 {r2 / r0:.4f}, "
                  f"remask4 / remask0 {r4 / r0:.4f}", flush=True)
    bpd = {}
    if remasking and os.environ.get("CRT_BPD", "1") != "0":
        # the model's own likelihood bound of its own 8-step samples: NOT a quality metric
        ab = new_sampler()
        for name, kw in (("remask=None", {}), ("remask=2", dict(remask=2)), ("remask=4", dict(remask=4))):
            torch.manual_seed(2026)
            tok = ab.sample_confident(8, **kw)
            torch.manual_seed(7)
            sc = ab.score(tok.reshape(BATCH, 7, 7), sample_steps=49, orders=4)
            bpd[name] = float(sc.bits_per_dim())
            print(f"score(8-step samples, 49 steps, orders = 4), {name}: {bpd[name]:.4f} bits per dimension (the model's own likelihood "
                  "bound, not a quality metric)", flush=True)
    print("CRT_RESULT " + json.dumps({"tree": "this" if not os.environ.get("CRT_TREE") else "CRT_TREE", "remasking": remasking,
                                      "results": out, "bits_per_dim": bpd}), flush=True)
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    limit = float(os.environ.get("CRT_LIMIT", "300"))
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=limit).returncode
    except subprocess.TimeoutExpired:
        print(f"confident_remask_time: ran past its {limit:.0f} s limit", flush=True)
        return 124
    if rc != 0:
        print(f"confident_remask_time: ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
