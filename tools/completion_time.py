"""Time of a conditional reverse process (sample(x_init=, known=)) against the unconditional one: per-batch
milliseconds of one sample() call -- one hipGraph replay, elimination + position lists -- between two HIP events, for the
unconditional call and for a start with a fraction 0, 1/4, 1/2, 3/4 of the tokens known (random positions) and with the
bottom half of the image removed (pixel rows >= H/2: the codes of rows 0..2 of 7 stay known).  Warm-up first, then the median
of CT_REPS (default 30) calls with their min / max; the whole set is repeated in CT_PROCS (default 2) fresh processes, and the
spread of a case over ALL its repeats is printed next to it, so that a difference between two cases can be read against it.

usage: completion_time.py [other_tree ...]      (CT_BATCH=256 CT_STEPS=100)
Every ``other_tree`` is the root of another checkout of this repository, built (the parent commit, say): its unconditional call
is timed in the same alternation, in processes of its own; a tree without the conditional start reports that line only."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(root):
    sys.path[:0] = [os.path.join(root, "spiking-diffusion_amd"), root]
    import inspect
    import torch
    sys.argv = ["bench.py"]
    import bench
    assert os.path.abspath(bench.__file__).startswith(os.path.abspath(root))
    dev = torch.device("cuda", 0)
    B, steps, reps = int(os.environ.get("CT_BATCH", "256")), int(os.environ.get("CT_STEPS", "100")), int(os.environ.get("CT_REPS", "30"))
    model, den, ab = bench.build_models(dev, 16)
    ab.n_samples = B
    h, w = ab.shape
    K = ab.num_classes
    g = torch.Generator().manual_seed(1)
    x_init = torch.randint(0, K, (B, 1, h, w), generator=g).to(dev)
    cases = {"unconditional": None}
    if "x_init" in inspect.signature(ab.sample).parameters:
        r = torch.rand(B, 1, h, w, generator=g)
        for name, frac in (("known 0", 0.0), ("known 1/4", 0.25), ("known 1/2", 0.5), ("known 3/4", 0.75)):
            cases[name] = (r < frac).to(dev)
        bottom = torch.zeros(B, 1, h, w, dtype=torch.bool)
        rows = [i for i in range(h) if 4 * i + 3 < 2 * h]                 # codes whose 7-pixel window ends above pixel row H/2
        bottom[:, :, rows] = True
        cases["bottom half removed"] = bottom.to(dev)
    out = {}
    for name, known in cases.items():
        kw = {} if known is None else dict(x_init=x_init, known=known)
        torch.manual_seed(1)
        for _ in range(3):
            ab.sample(temp=1.0, sample_steps=steps, **kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ab.sample(temp=1.0, sample_steps=steps, **kw)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[name] = dict(ms=ms, known_fraction=None if known is None else float(known.float().mean()))
    assert len(ab._graphs) <= 2
    print("CT_RESULT " + json.dumps(dict(form=ab.form_for(B, h, w), B=B, steps=steps, cases=out)), flush=True)


def main():
    trees = [ROOT] + [os.path.abspath(t) for t in sys.argv[1:]]
    procs = int(os.environ.get("CT_PROCS", "2"))
    runs = {}
    for rep in range(procs):
        for tree in trees:                                               # alternating: a drift of the box hits every tree alike
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], capture_output=True, text=True)
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("CT_RESULT ")), None)
            if line is None:
                print(f"{tree}: child failed (exit {r.returncode}): {r.stderr.strip()[-800:]}", flush=True)
                return 1
            res = json.loads(line[len("CT_RESULT "):])
            for name, c in res["cases"].items():
                runs.setdefault((tree, name), dict(ms=[], medians=[], frac=c["known_fraction"], cfg=res))
                runs[(tree, name)]["ms"] += c["ms"]
                runs[(tree, name)]["medians"].append(statistics.median(c["ms"]))
    for (tree, name), c in runs.items():
        ms, cfg = sorted(c["ms"]), c["cfg"]
        tag = "this tree" if tree == ROOT else tree
        frac = "" if c["frac"] is None else f" (known fraction {c['frac']:.3f})"
        print(f"{tag:14s} B={cfg['B']} steps={cfg['steps']} {cfg['form']:18s} {name:20s} median {statistics.median(ms):7.3f} ms  "
              f"per-process medians {' '.join(f'{m:.3f}' for m in c['medians'])}  min {ms[0]:.3f} p10 {ms[len(ms) // 10]:.3f} "
              f"p90 {ms[len(ms) * 9 // 10]:.3f} max {ms[-1]:.3f}  n={len(ms)}{frac}", flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(main())
