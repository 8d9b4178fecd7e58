"""How close are the sampler's images to data?    The trained checkpoint against procedurally generated stroke
images the training run never saw (tools/train_on_strokes.py::strokes with another seed), SQ_N (default 10 240) images a side,
'encoder' features (the read-out the quantiser searches on, d = 784): the Frechet distance in both conventions and the kernel
distance with main.py's KID defaults (100 subsets of 1000, cubic kernel), through ``spkdiff.evaluate.sample_quality_eval``.

Rows:
  noise floor      two disjoint halves of real images against each other (generated side replaced by real images): what the
                   estimators give for two samples of ONE distribution at this n
  sample 49        ``sample()`` at 49 steps (one token per step: the reference's sampler)
  confident S      ``sample_confident(S)`` at 8, 12 and 16 steps
  confident 8 cos  the 8-step call with ``schedule='cosine'``
  remask 2 / 4     the 8-step call with ``remask=2`` / ``remask=4``

Every row is measured against the SAME real set.  The numbers are reported as they come; lower is better for every column.
The measurement runs in a child process under a time limit (SQ_LIMIT seconds, default 900).

usage: sample_quality.py      (SQ_N=10240 SQ_BATCH=256 SQ_LIMIT=900 SQ_SEED=500000)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd"), ROOT, os.path.join(ROOT, "tools")]
    import torch
    sys.argv = ["bench.py"]
    import bench
    from spkdiff.evaluate import FeatureStats, frechet_distance, kernel_distance, sample_quality_eval
    from train_on_strokes import strokes
    n, batch, seed = int(os.environ.get("SQ_N", "10240")), int(os.environ.get("SQ_BATCH", "256")), int(os.environ.get("SQ_SEED", "500000"))
    dev = torch.device("cuda", 0)
    model, den, ab = bench.build_models(dev, 16, weights="trained")
    t0 = time.time()
    data = strokes(2 * n, seed)                                        # (the training run drew seeds 2024 .. 2024 + 8192)
    real, other = data[:n], data[n:]
    print(f"{2 * n} stroke images from seed {seed} in {time.time() - t0:.1f} s; sampler form at B = {batch}: {ab.form_for(batch, 7, 7)}",
          flush=True)
    batches = lambda x: [x[i:i + batch] for i in range(0, x.shape[0], batch)]      # noqa: E731

    # the noise floor: real against real, through the same feature path (uint8 grid, encoder read-out)
    with torch.no_grad():
        feats = [torch.cat([model.encode_features(((b.to(dev) * 255 + 0.5).to(torch.uint8).float() / 255 - 0.5).contiguous(), 16)
                            for b in batches(x)]) for x in (real, other)]
    sa, sb = (FeatureStats(f.shape[1], dev).update(f) for f in feats)
    kd = kernel_distance(feats[0], feats[1])
    rows = {"noise floor": {"fd": frechet_distance(sa, sb), "fd_reference_convention": frechet_distance(sa, sb, "reference"),
                            "kd_mean": kd[0], "kd_std": kd[1], "n_real": sa.n, "n_generated": sb.n, "d": sa.d}}
    draws = {"sample 49": lambda s, b: s.sample(1.0, 49),
             "confident 8": lambda s, b: s.sample_confident(8),
             "confident 12": lambda s, b: s.sample_confident(12),
             "confident 16": lambda s, b: s.sample_confident(16),
             "confident 8 cos": lambda s, b: s.sample_confident(8, schedule="cosine"),
             "remask 2": lambda s, b: s.sample_confident(8, remask=2),
             "remask 4": lambda s, b: s.sample_confident(8, remask=4)}
    print(f"{'row':16s} {'fd':>12s} {'fd (ref. conv.)':>16s} {'kd mean':>13s} {'kd std':>11s} {'seconds':>8s}", flush=True)
    r = rows["noise floor"]
    print(f"{'noise floor':16s} {r['fd']:12.5f} {r['fd_reference_convention']:16.5f} {r['kd_mean']:13.6e} {r['kd_std']:11.3e} {'':>8s}",
          flush=True)
    for name, draw in draws.items():
        torch.manual_seed(2027)
        t0 = time.time()
        r = rows[name] = sample_quality_eval(model, ab, batches(real), n, draw=draw, features="encoder", batch=batch)
        print(f"{name:16s} {r['fd']:12.5f} {r['fd_reference_convention']:16.5f} {r['kd_mean']:13.6e} {r['kd_std']:11.3e} "
              f"{time.time() - t0:8.1f}", flush=True)
    print("SQ_RESULT " + json.dumps({"n": n, "batch": batch, "seed": seed, "rows": rows}), flush=True)
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    limit = float(os.environ.get("SQ_LIMIT", "900"))
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=limit).returncode
    except subprocess.TimeoutExpired:
        print(f"sample_quality: ran past its {limit:.0f} s limit", flush=True)
        return 124
    if rc != 0:
        print(f"sample_quality: ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
