"""Time of one ``score()`` batch beside one ``sample()`` batch at the same (B, steps): per-call milliseconds of
one hipGraph replay in the default launch form between two HIP events, ``sample()`` and ``score()`` alternating call by call so that
a drift of the box hits both alike.  Warm-up first (three calls each: the captures), then ST_REPS (default 30) calls each; the
whole set is repeated in ST_PROCS (default 2) fresh processes and the spread of a case over ALL its repeats is printed next to
its median, so that the difference between the two can be read against it.  The expectation is parity: the same denoiser
launches, and a token update that skips the categorical race.

usage: score_time.py                              (ST_CASES="16x49,256x49,256x100": B x steps)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd"), ROOT]
    import torch
    sys.argv = ["bench.py"]
    import bench
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("ST_REPS", "30"))
    cases = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("ST_CASES", "16x49,256x49,256x100").split(",")]
    model, den, ab = bench.build_models(dev, 16)
    h, w = ab.shape
    out = {}
    for B, steps in cases:
        ab.n_samples = B
        x_0 = torch.randint(0, ab.num_classes, (B, 1, h, w), generator=torch.Generator().manual_seed(1)).to(dev)
        calls = {"sample": lambda: ab.sample(temp=1.0, sample_steps=steps), "score": lambda: ab.score(x_0, temp=1.0, sample_steps=steps)}
        torch.manual_seed(1)
        for _ in range(3):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(reps):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        assert len(ab._graphs) == 2                                    # sample()'s graph and the score graph, both kept
        sc = ab._form(B, h, w)._replace(tail=False, tail_act=False)
        out[f"{B}x{steps}"] = dict(ms=ms, sample_form=ab.form_for(B, h, w),
                                   score_form=("elimination_lists" if sc.lists else "elimination") if sc.skip else "dense")
    print("ST_RESULT " + json.dumps(out), flush=True)


def main():
    procs = int(os.environ.get("ST_PROCS", "2"))
    runs = {}
    for _ in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("ST_RESULT ")), None)
        if line is None:
            print(f"child failed (exit {r.returncode}): {r.stderr.strip()[-800:]}", flush=True)
            return 1
        for case, c in json.loads(line[len("ST_RESULT "):]).items():
            for name, ms in c["ms"].items():
                e = runs.setdefault((case, name), dict(ms=[], medians=[], form=c[f"{name}_form"]))
                e["ms"] += ms
                e["medians"].append(statistics.median(ms))
    for (case, name), c in runs.items():
        ms = sorted(c["ms"])
        B, steps = case.split("x")
        print(f"B={B} steps={steps} {name:6s} {c['form']:18s} median {statistics.median(ms):7.3f} ms  per-process medians "
              f"{' '.join(f'{m:.3f}' for m in c['medians'])}  min {ms[0]:.3f} p10 {ms[len(ms) // 10]:.3f} p90 {ms[len(ms) * 9 // 10]:.3f} "
              f"max {ms[-1]:.3f}  n={len(ms)}", flush=True)
    for case in dict.fromkeys(c for c, _ in runs):
        a, b = statistics.median(runs[(case, "sample")]["ms"]), statistics.median(runs[(case, "score")]["ms"])
        print(f"{case}: score / sample = {b / a:.3f}", flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    else:
        sys.exit(main())
