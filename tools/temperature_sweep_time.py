"""Time of R/main.py's second temperature sweep (:418-443: 12 temperatures x 80 calls of ``abdiff.sample(temp=tem,
sample_steps=49)`` at 16 images, each decoded to uint8) run two ways:

  as written   scalar calls at B = 16, every call a job of its own (fresh key, global image index 0), decode per call.  The sampler's
               graph key holds the temperature, so every temperature captures a new graph: the first call of a temperature (capture
               + replay, wall clock around a synchronised call) is reported apart from the steady-state replays (79 calls + their
               decodes between two HIP events per temperature).
  one job      ``spkdiff.evaluate.temperature_sweep(model, ab, temps, 1280, sample_steps=49, batch=256)``: per-image temperatures,
               60 calls of 256 images on one captured graph, between two HIP events (its capture happens in an untimed first pass,
               which is reported as well).

Both on the trained checkpoint and on the synthetic one.  Warm-up (weight packing, allocator pools; for the one-job way a whole
untimed pass) is excluded; the two ways alternate TS_REPS (default 3) times and every pass is printed, so that the ratio can be
read against the spread.  Before the timing the tool asserts that the two ways give EQUAL tokens under one shared key: the job's
960 scalar calls at B = 16, each on its shard of the job (``set_shard(16 * call, 16)``, launched eagerly), against the one-job
tokens.

usage: temperature_sweep_time.py      (TS_CALLS=80 TS_REPS=3 TS_WEIGHTS=trained,synthetic)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPS = [0.001, 0.01, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1]          # R/main.py:418
STEPS, CALL_B = 49, 16


def as_written(model, ab, calls, captures):
    """One pass of the loop as the script runs it.  Returns (ms of the first call per temperature, summed; ms of the other calls
    and all decodes, summed; graph captures)."""
    import torch
    ab.set_shard(0, CALL_B)
    first_ms = steady_ms = 0.0
    c0 = captures[0]
    for tem in TEMPS:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tok = ab.sample(temp=tem, sample_steps=STEPS).reshape(CALL_B, 7, 7)
        torch.cuda.synchronize()
        first_ms += (time.perf_counter() - t0) * 1e3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model.decode_tokens(tok, 16, want_u8=True)
        for _ in range(calls - 1):
            tok = ab.sample(temp=tem, sample_steps=STEPS).reshape(CALL_B, 7, 7)
            model.decode_tokens(tok, 16, want_u8=True)
        e1.record()
        e1.synchronize()
        steady_ms += e0.elapsed_time(e1)
    return first_ms, steady_ms, captures[0] - c0


def one_job(model, ab, calls, captures):
    import torch
    from spkdiff.evaluate import temperature_sweep
    c0 = captures[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    u8, tok = temperature_sweep(model, ab, TEMPS, calls * CALL_B, sample_steps=STEPS, batch=256)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), captures[0] - c0, tok


def main():
    sys.path[:0] = [os.path.join(ROOT, "spiking-diffusion_amd"), ROOT]
    import torch
    sys.argv = ["bench.py"]
    import bench
    import snn_model.vq_diffusion as vqd
    calls, reps = int(os.environ.get("TS_CALLS", "80")), int(os.environ.get("TS_REPS", "3"))
    captures = [0]
    init = vqd._SamplerGraph.__init__

    def counted(self, *a, **k):
        captures[0] += 1
        init(self, *a, **k)
    vqd._SamplerGraph.__init__ = counted
    dev = torch.device("cuda", 0)
    n = calls * CALL_B
    out = {}
    for weights in os.environ.get("TS_WEIGHTS", "trained,synthetic").split(","):
        model, den, ab = bench.build_models(dev, 16, weights=weights)
        assert list(ab.shape) == [7, 7]
        # (a sampler per way on the one denoiser: a sampler keeps at most two graphs, and the twelve captures of the scalar way
        #  would evict the one-job graph between the passes)
        ab1 = vqd.AbsorbingDiffusion(den, mask_id=ab.mask_id, latent_shape=tuple(ab.shape))
        # ---- equal tokens under one key: the job's scalar calls at B = 16 on their shards (eager) against the one job
        torch.manual_seed(2024)
        warm_ms, warm_caps, tok = one_job(model, ab1, calls, captures)      # (the one-job way's untimed first pass: its capture)
        key = int(ab1.last_key)
        ab.use_graph = False
        torch.manual_seed(2024)
        ab.set_shard(0, CALL_B)
        bad = 0
        with ab._one_key() as k2:
            assert k2 == key
            for g, tem in enumerate(TEMPS):
                for i in range(calls):
                    ab.set_shard(g * n + i * CALL_B, CALL_B)
                    got = ab.sample(temp=tem, sample_steps=STEPS).reshape(CALL_B, 7, 7)
                    bad += int((got != tok[g, i * CALL_B:(i + 1) * CALL_B]).sum())
        ab.use_graph = True
        assert bad == 0, f"{weights}: {bad} tokens differ between the scalar calls and the one job"
        # ---- warm-up of the as-written way (a temperature outside the list), then alternate
        ab.set_shard(0, CALL_B)
        for _ in range(3):
            model.decode_tokens(ab.sample(temp=0.95, sample_steps=STEPS).reshape(CALL_B, 7, 7), 16, want_u8=True)
        torch.cuda.synchronize()
        res = dict(as_written=[], one_job=[], one_job_warmup=dict(ms=warm_ms, captures=warm_caps), images=len(TEMPS) * n,
                   tokens_equal=True)
        for _ in range(reps):
            f, s, c = as_written(model, ab, calls, captures)
            res["as_written"].append(dict(first_calls_ms=f, steady_ms=s, total_ms=f + s, captures=c))
            ms, c, _ = one_job(model, ab1, calls, captures)
            res["one_job"].append(dict(ms=ms, captures=c))
        a_tot = statistics.median(r["total_ms"] for r in res["as_written"])
        a_steady = statistics.median(r["steady_ms"] for r in res["as_written"])
        b = statistics.median(r["ms"] for r in res["one_job"])
        res["median"] = dict(as_written_total_ms=a_tot, as_written_steady_ms=a_steady, one_job_ms=b, ratio_total=a_tot / b,
                             ratio_steady=a_steady / b)
        out[weights] = res
        print(f"{weights:9s} {len(TEMPS)} temperatures x {calls} calls x {CALL_B} images, {STEPS} steps + decode", flush=True)
        for r in res["as_written"]:
            print(f"  as written: first call of each temperature {r['first_calls_ms']:9.1f} ms ({r['captures']} captures), "
                  f"steady state {r['steady_ms']:9.1f} ms, total {r['total_ms']:9.1f} ms", flush=True)
        for r in res["one_job"]:
            print(f"  one job   : {r['ms']:9.1f} ms ({r['captures']} captures)", flush=True)
        print(f"  one-job first pass {warm_ms:.1f} ms ({warm_caps} captures); medians: as written {a_tot:.1f} ms "
              f"(steady {a_steady:.1f}), one job {b:.1f} ms: x{a_tot / b:.2f} (steady state alone x{a_steady / b:.2f}); "
              f"{res['images'] / a_tot * 1e3:.0f} -> {res['images'] / b * 1e3:.0f} images/s", flush=True)
    print("TS_RESULT " + json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
