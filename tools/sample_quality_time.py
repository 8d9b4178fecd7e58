"""What the sample-quality metric stage costs, N = 10 240 'encoder' features a side (d = 784), against its
torch-operator restatement on the same device and against the sampling it follows.

  moments      ``ops.feature_moments`` over the set in updates of 256 rows (as ``sample_quality_eval`` makes them), both sides
  moments_t    the restatement: per update ``x.double().T @ x.double()`` and ``x.double().sum(0)`` added to the state (library dgemm)
  ksums        the three ``ops.poly_kernel_sums`` calls of ``kernel_distance`` -- 100 subsets of 1000, cubic kernel: no n x m buffer,
               all subsets in one launch each
  ksums_t      the restatement: per subset the gathered rows in fp64, a materialised 1000 x 1000 Gram matrix, its power, two sums
  sampling     what produces one side: 40 calls of ``sample_confident(8)`` at B = 256 (captured), decoded and encoded

A window is one pass of a configuration between two HIP events after a warm-up pass; the configurations alternate over SQT_WINDOWS
(default 5) windows; the median is reported with the spread (max - min) beside it.  No ratio is a pass condition: the numbers are
recorded as measured.  The measurement runs in a child process under a time limit (SQT_LIMIT seconds, default 600).

usage: sample_quality_time.py      (SQT_N=10240 SQT_WINDOWS=5 SQT_LIMIT=600)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, SUBSETS, SUBSET_SIZE = 256, 100, 1000


def window(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def child():
    sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd"), ROOT]
    import torch
    sys.argv = ["bench.py"]
    import bench
    from spkdiff import ops
    from spkdiff.evaluate import kernel_subsets
    n, windows = int(os.environ.get("SQT_N", "10240")), int(os.environ.get("SQT_WINDOWS", "5"))
    dev = torch.device("cuda", 0)
    model, den, ab = bench.build_models(dev, 16, weights="trained")
    ab.n_samples = BATCH
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                               # features with the encoder's statistics: encoded samples
        torch.manual_seed(3)
        sides = []
        for _ in range(2):
            f = [model.encode_features((model.decode_tokens(ab.sample_confident(8).reshape(BATCH, 7, 7), 16)[1].float() / 255 - 0.5)
                                       .contiguous(), 16) for _ in range(4)]
            f = torch.cat(f)
            sides.append(f[torch.randint(0, f.shape[0], (n,), generator=g).to(dev)] +
                         0.01 * torch.randn((n, f.shape[1]), generator=g).to(dev))
    X, Y = sides
    d = X.shape[1]
    ix, iy = (t.to(dev) for t in kernel_subsets(n, n, SUBSETS, SUBSET_SIZE, 0))
    state = [(torch.zeros(d, dtype=torch.float64, device=dev), torch.zeros((d, d), dtype=torch.float64, device=dev)) for _ in range(2)]
    ws = ops.poly_kernel_sums_ws(SUBSETS, SUBSET_SIZE, SUBSET_SIZE, dev)
    out = torch.empty((3, SUBSETS, 2), dtype=torch.float64, device=dev)

    def moments():
        for (s, gm), F in zip(state, (X, Y)):
            for i in range(0, n, BATCH):
                ops.feature_moments(F[i:i + BATCH], s, gm)

    def moments_t():
        for (s, gm), F in zip(state, (X, Y)):
            for i in range(0, n, BATCH):
                f = F[i:i + BATCH].double()
                gm.addmm_(f.T, f)
                s += f.sum(0)

    def ksums():
        ops.poly_kernel_sums(X, X, ix, ix, symmetric=True, ws=ws, out=out[0])
        ops.poly_kernel_sums(Y, Y, iy, iy, symmetric=True, ws=ws, out=out[1])
        ops.poly_kernel_sums(X, Y, ix, iy, ws=ws, out=out[2])

    def ksums_t():
        Xd, Yd = X.double(), Y.double()
        for k, (A, ia, B, ib, sym) in enumerate(((Xd, ix, Xd, ix, True), (Yd, iy, Yd, iy, True), (Xd, ix, Yd, iy, False))):
            for s in range(SUBSETS):
                v = (A[ia[s].long()] @ B[ib[s].long()].T) / d + 1.0
                kk = v * v * v
                out[k, s, 0] = kk.sum()
                if sym:
                    out[k, s, 1] = torch.diagonal(kk).sum()

    def sampling():
        with torch.no_grad():
            for _ in range(n // BATCH):
                tok = ab.sample_confident(8).reshape(BATCH, 7, 7)
                model.encode_features((model.decode_tokens(tok, 16)[1].float() / 255 - 0.5).contiguous(), 16)

    ways = {"moments": moments, "moments_t": moments_t, "ksums": ksums, "ksums_t": ksums_t, "sampling": sampling}
    for fn in ways.values():
        window(fn)
    res = {k: [] for k in ways}
    for _ in range(windows):
        for k, fn in ways.items():
            res[k].append(window(fn))
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        print(f"{k:10s} median {med[k]:10.3f} ms of {windows} windows (max - min {max(v) - min(v):.3f}); windows "
              f"{' '.join(f'{t:.3f}' for t in v)}", flush=True)
    print(f"N = {n} a side, d = {d}: moments / moments_t {med['moments'] / med['moments_t']:.3f}, ksums / ksums_t "
          f"{med['ksums'] / med['ksums_t']:.3f}, (moments + ksums) / sampling {(med['moments'] + med['ksums']) / med['sampling']:.4f}",
          flush=True)
    ksums()
    a = out.clone()
    ksums_t()
    print(f"ksums against the restatement: max relative difference {float(((a - out).abs() / out.abs().clamp_min(1e-300)).max()):.2e}",
          flush=True)
    print("SQT_RESULT " + json.dumps({"n": n, "d": d, "windows": res, "median": med}), flush=True)
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    limit = float(os.environ.get("SQT_LIMIT", "600"))
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=limit).returncode
    except subprocess.TimeoutExpired:
        print(f"sample_quality_time: ran past its {limit:.0f} s limit", flush=True)
        return 124
    if rc != 0:
        print(f"sample_quality_time: ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
