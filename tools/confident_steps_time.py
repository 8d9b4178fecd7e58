"""What per-image step counts buy confidence-ordered decoding: B = 256, captured, the trained checkpoint.

  mixed     seeded start states with a quarter of the images each at m = 4, 12, 24 and 49 unknown positions (interleaved over the
            batch).  ``sample_confident([s_i], x_init=, known=)`` with s_i = ceil(m_i / 4) -- what ``positions_per_step = 4`` chooses:
            1, 3, 6, 13 -- against ``sample_confident(13, x_init=, known=)`` on the same states: the dense call runs every image
            through the denoiser at each of the 13 steps, the per-image call only the pending ones.  The image-step ratio
            sum(s_i) / (B * 13) = 1472 / 3328 = 0.442 is the ideal; the time ratio is printed beside it.
  uniform   nothing known, every image at 13 steps: ``sample_confident([13] * B)`` (the list form: spk_select_pending, the denoiser on
            the active list, the counts kernel, spk_psample_step_conf_listed) against ``sample_confident(13)`` (the dense form with
            the fused step tail) -- the price of the list form when nothing can be skipped.

A window is CS_CALLS (default 10) calls between two HIP events after a warm-up window; the four configurations alternate over
CS_WINDOWS (default 7) windows; medians and the spread of the windows are printed, then a CS_RESULT line with every window.  The
measurement runs in a child process under a time limit (CS_LIMIT seconds, default 300).

usage: confident_steps_time.py      (CS_CALLS=10 CS_WINDOWS=7 CS_WEIGHTS=trained CS_LIMIT=300)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, HW, PER_STEP, HOLES = 256, 49, 4, (4, 12, 24, 49)


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
    calls, windows = int(os.environ.get("CS_CALLS", "10")), int(os.environ.get("CS_WINDOWS", "7"))
    dev = torch.device("cuda", 0)
    _, den, ab0 = bench.build_models(dev, 16, weights=weights)
    assert list(ab0.shape) == [7, 7]
    K = int(ab0.num_classes)

    def new_sampler():
        ab = vqd.AbsorbingDiffusion(den, mask_id=ab0.mask_id, latent_shape=tuple(ab0.shape))
        ab.n_samples = BATCH
        return ab
    g = torch.Generator().manual_seed(416)
    m = [HOLES[i % len(HOLES)] for i in range(BATCH)]
    known = torch.ones(BATCH, HW, dtype=torch.bool)
    for i, mi in enumerate(m):
        known[i, torch.randperm(HW, generator=g)[:mi]] = False
    x_init = torch.randint(0, K, (BATCH, 1, 7, 7), generator=g).to(dev)
    known = known.reshape(BATCH, 1, 7, 7).to(dev)
    steps = [max(1, -(-mi // PER_STEP)) for mi in m]
    S = max(steps)
    assert sorted(set(steps)) == [1, 3, 6, 13] and sum(steps) == 1472 and BATCH * S == 3328
    sv = torch.tensor(steps, dtype=torch.int32)
    full = torch.full((BATCH,), S, dtype=torch.int32)
    ways = {"mixed per-image": (new_sampler(), lambda ab: ab.sample_confident(sv, x_init=x_init, known=known)),
            "mixed dense@13": (new_sampler(), lambda ab: ab.sample_confident(S, x_init=x_init, known=known)),
            "uniform listed@13": (new_sampler(), lambda ab: ab.sample_confident(full)),
            "uniform dense@13": (new_sampler(), lambda ab: ab.sample_confident(S))}
    # the per-image call gives the dense call's tokens where the counts agree, and known tokens stay
    torch.manual_seed(5)
    a = ways["mixed per-image"][1](ways["mixed per-image"][0])
    torch.manual_seed(5)
    b = ways["mixed dense@13"][1](ways["mixed dense@13"][0])
    at13 = torch.tensor([s == S for s in steps], device=dev)
    assert torch.equal(a[at13], b[at13]) and torch.equal(a[known], x_init[known]) and int(a.max()) < K
    for ab, fn in ways.values():                                     # warm-up: capture + one window
        timed_window(lambda: fn(ab), calls)
        assert len(ab._graphs) == 1
    res = {name: [] for name in ways}
    for _ in range(windows):
        for name, (ab, fn) in ways.items():
            res[name].append(timed_window(lambda: fn(ab), calls))
    out = {}
    for name in ways:
        med = statistics.median(res[name])
        out[name] = dict(ms_per_call=res[name], median=med, spread=max(res[name]) - min(res[name]))
        print(f"{weights:9s} {name:18s} B = {BATCH}: median {med:7.3f} ms per call of {windows} windows (max - min "
              f"{out[name]['spread']:.3f})", flush=True)
    r_mixed = out["mixed per-image"]["median"] / out["mixed dense@13"]["median"]
    r_uni = out["uniform listed@13"]["median"] / out["uniform dense@13"]["median"]
    print(f"{weights:9s} mixed job (m = 4, 12, 24, 49 -> s = 1, 3, 6, 13): per-image / dense time {r_mixed:.3f}; image steps "
          f"{sum(steps)} / {BATCH * S} = {sum(steps) / (BATCH * S):.3f} is the ideal", flush=True)
    print(f"{weights:9s} uniform job (all m = 49, s = 13): listed / dense time {r_uni:.3f} -- the list form's price when nothing "
          "can be skipped", flush=True)
    out["ratios"] = dict(mixed=r_mixed, ideal=sum(steps) / (BATCH * S), uniform=r_uni)
    print("CS_RESULT " + json.dumps({weights: out}), flush=True)
    return 0


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    limit = float(os.environ.get("CS_LIMIT", "300"))
    for weights in os.environ.get("CS_WEIGHTS", "trained").split(","):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", weights], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f"confident_steps_time: {weights} ran past its {limit:.0f} s limit; nothing more is started", flush=True)
            return 124
        if rc != 0:
            print(f"confident_steps_time: {weights} ended with status {rc}; nothing more is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
