"""GPU tests of per-image step counts for confidence-ordered decoding (run with ``-m gpu`` on an MI355X):
``spk_select_pending`` against the host mirror of tests/_confident_steps_oracle.py, ``spk_psample_step_conf_listed`` against
``spk_psample_step_conf`` bit for bit (full list, sub-list, shifted counters), ``AbsorbingDiffusion.sample_confident`` with a step
vector against its one-count calls row by row -- eager, captured, across shards --, ``complete_images_confident(positions_per_step=)``,
``step_count_sweep`` and what the wrappers refuse."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

import _confident_oracle as cfo             # noqa: E402
import _confident_steps_oracle as cso       # noqa: E402
from spkdiff import synth                  # noqa: E402
from test_gpu_completion import K as K128, build_den, build_vae, sampler      # noqa: E402  (the helpers, not the tests)
from test_gpu_confident import KLIST, PLIST, TLIST, conf_call      # noqa: E402

SIGMA = cso.STEP_STRIDE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


# ------------------------------------------------------------------------------------------------- 1. the list of pending images
@pytest.mark.parametrize("HW", [1, 49, 64])
@pytest.mark.parametrize("B", [1, 5, 64, 65, 300])
def test_select_pending_vs_oracle(dev, ops, B, HW):
    """One compaction chunk (B <= 64), a ragged second chunk (65), several workgroups (8 images each); images with m = 0, 1, HW and
    a seeded m; entries -3, 0, t - 1, t, t + 1, S + 5; t in {1, 2, S}; every call on ONE buffer pair.  The list equals the host
    mirror and is ascending, the count is its length, the work word is zero afterwards, ``unmasked`` is untouched."""
    S = 13
    out = (torch.full((B,), -7, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))
    bad = {}
    for i, t in enumerate((1, 2, S, 2)):                                  # (the fourth call: another state at a t already seen)
        un, steps = cso.select_case(B, HW, t, S, seed=1000 * B + 10 * HW + i)
        und, sd = un.to(dev), steps.to(dev)
        got = ops.select_pending(und, t, sd, out=out)
        assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
        want = cso.pending(un, t, steps.tolist())
        n, word = (int(v) for v in out[1].cpu())
        lst = out[0].cpu()[:max(n, 0)].tolist()
        bad[f"call{i}_t{t}"] = int(n != len(want)) + int(lst != want) + int(lst != sorted(lst)) + int(word != 0) + \
            int(not torch.equal(und.cpu(), un))
    # without ``out``: a fresh pair, the same list
    fresh = ops.select_pending(und, t, sd)
    assert int(fresh[1][0]) == len(want) and fresh[0].cpu()[:len(want)].tolist() == want and int(fresh[1][1]) == 0
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 2. the listed token update
def listed_call(ops, dev, logits, x0, un0, t, temp, top_k, top_p, steps, S, lst, **noise):
    """One listed update on copies of the state -> (x_t, unmasked, x0_hat, conf); ``lst``: the images of the list, in slot order.
    The outputs carry conf_call's sentinels; the slots past the list hold NaN logits, which nothing may read."""
    Bn = x0.shape[0]
    n = x0.numel()
    slots = torch.full_like(logits, float("nan"))
    slots[:len(lst)] = logits[torch.tensor(lst, dtype=torch.int64, device=dev)]
    act = torch.full((Bn,), -1, dtype=torch.int32, device=dev)
    act[:len(lst)] = torch.tensor(lst, dtype=torch.int32, device=dev)
    nact = torch.tensor([len(lst), 0], dtype=torch.int32, device=dev)
    x, un = x0.clone(), un0.clone()
    hat = torch.full((n,), -5, dtype=torch.int64, device=dev)
    conf = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    with ops.active_set(act, nact):
        ops.psample_step_conf_listed(slots, x, un, t, temp, steps, S, SIGMA, x0_hat=hat, conf=conf, top_k=top_k, top_p=top_p, **noise)
    return x, un, hat, conf


def _rows_differ(a, b, rows, HW):
    """How many of the four outputs differ on the given images (bitwise; conf compared as integers: a NaN equals itself)."""
    n = 0
    for u, v in zip(a[:4], b[:4]):
        u, v = u.reshape(-1, HW)[rows], v.reshape(-1, HW)[rows]
        if u.dtype == torch.float32:
            u, v = u.view(torch.int32), v.view(torch.int32)
        n += int((u != v).sum())
    return n


@pytest.mark.parametrize("HW", cfo.HWS)
@pytest.mark.parametrize("K", cfo.KS)
def test_psample_step_conf_listed_equals_the_dense_entry_point(dev, ops, K, HW):
    """The case table of tests/_confident_oracle.conf_inputs (B = 5, m = 0, 1, 2, HW - 1, HW, per-image temperature / k / p), injected
    q, Philox and philox_state.  Full list with steps_b = S: state, x0_hat and conf are spk_psample_step_conf's bit for bit.
    Sub-list [0, 2, 4] with the logits gathered by slot: listed images equal the dense call's, unlisted ones keep state and
    sentinels.  An image with e_i < S equals the dense call made at offset - (S - e_i) * sigma and (enough positions and classes to
    tell) differs from the unshifted one; steps_b > S behaves as S."""
    logits, q, x0, un0, temps, ks, ps = cfo.conf_inputs(K, HW)
    ld, x0d, un0d, tv, kd, pd = (v.to(dev) for v in (logits, x0, un0, temps, ks, ps))
    Bn, S, t, e = cfo.B, 6, 2, 3
    seed, off = 0x1234_5678_9ABC, 5 * SIGMA + 11 * HW * K
    state = torch.tensor([seed, 1 << 33], dtype=torch.int64, device=dev)
    noises = {"injected": dict(q=q.to(dev)), "philox": dict(seed=seed, offset=off),
              "philox_state": dict(seed=99, offset=off - (1 << 33), philox_state=state)}
    full = torch.full((Bn,), S, dtype=torch.int32, device=dev)
    mixed = torch.tensor([S, S, S + 7, e, e], dtype=torch.int32, device=dev)      # images 3 and 4 run e < S steps, image 2 "more"
    every = list(range(Bn))
    # untruncated rows at temperature 2: the draws show (the table's p -> 0+ / k rows are nearly deterministic)
    flat = (torch.full((Bn,), 2.0, device=dev), torch.zeros(Bn, dtype=torch.int32, device=dev), torch.ones(Bn, device=dev))
    bad, shift_shows = {}, 0
    for mode, kw in noises.items():
        dense = conf_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, **kw)
        got = listed_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, full, S, every, **kw)
        bad[f"{mode}_full"] = _rows_differ(got, dense, every, HW)
        # t = S, the first step of the loop, and t = 1, the last
        for tt in (S, 1):
            bad[f"{mode}_full_t{tt}"] = _rows_differ(listed_call(ops, dev, ld, x0d, un0d, tt, tv, kd, pd, full, S, every, **kw),
                                                     conf_call(ops, dev, ld, x0d, un0d, tt, tv, kd, pd, **kw), every, HW)
        sub = listed_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, full, S, [0, 2, 4], **kw)
        bad[f"{mode}_sub_listed"] = _rows_differ(sub, dense, [0, 2, 4], HW)
        untouched = (x0d, un0d, torch.full_like(sub[2], -5), torch.full_like(sub[3], 7.0))
        bad[f"{mode}_sub_unlisted"] = _rows_differ(sub, untouched, [1, 3], HW)
        # a list in another order serves the same images (slot s = image active[s])
        bad[f"{mode}_sub_permuted"] = _rows_differ(listed_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, full, S, [4, 0, 2], **kw), sub,
                                                   every, HW)
        mix = listed_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, mixed, S, every, **kw)
        bad[f"{mode}_above_S_is_S"] = _rows_differ(mix, dense, [0, 1, 2], HW)
        if mode == "injected":
            bad[f"{mode}_q_as_given"] = _rows_differ(mix, dense, [3, 4], HW)
            continue
        shifted = dict(kw, offset=kw["offset"] - (S - e) * SIGMA)
        assert shifted["offset"] >= 0
        bad[f"{mode}_shifted"] = _rows_differ(mix, conf_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, **shifted), [3, 4], HW)
        fm = listed_call(ops, dev, ld, x0d, un0d, t, *flat, mixed, S, every, **kw)
        bad[f"{mode}_flat_shifted"] = _rows_differ(fm, conf_call(ops, dev, ld, x0d, un0d, t, *flat, **shifted), [3, 4], HW)
        shift_shows += int(_rows_differ(fm, conf_call(ops, dev, ld, x0d, un0d, t, *flat, **kw), [3, 4], HW) > 0)
        # an image whose count is below t is not pending: left as it is even on the list
        low = torch.tensor([S, S, S, 1, S], dtype=torch.int32, device=dev)
        lo = listed_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, low, S, every, **kw)
        bad[f"{mode}_below_t"] = _rows_differ(lo, (x0d, un0d, torch.full_like(lo[2], -5), torch.full_like(lo[3], 7.0)), [3], HW) + \
            _rows_differ(lo, dense, [0, 1, 2, 4], HW)
    print(f"conf_listed K={K} HW={HW}: {bad}, shifted draws differ in {shift_shows} of 2 modes")
    assert all(v == 0 for v in bad.values()), bad
    if HW >= 49 and K >= 63:
        assert shift_shows == 2, "an image with e < S draws other counters than the loop's"


def test_listed_wrapper_refuses_before_launching(dev, ops):
    K, HW, Bn = 64, 49, 5
    logits, q, x0, un0, temps, ks, ps = cfo.conf_inputs(K, HW)
    ld, x0d, un0d, tv = (v.to(dev) for v in (logits, x0, un0, temps))
    steps = torch.full((Bn,), 4, dtype=torch.int32, device=dev)
    act, nact = torch.arange(Bn, dtype=torch.int32, device=dev), torch.tensor([Bn, 0], dtype=torch.int32, device=dev)
    x, un = x0d.clone(), un0d.clone()
    with pytest.raises(ValueError, match="active_set"):
        ops.psample_step_conf_listed(ld, x, un, 2, tv, steps, 4, SIGMA)                     # outside a scope
    with ops.active_set(act, nact):
        for kw in (dict(steps_b=steps[:4]), dict(steps_b=steps.long()), dict(steps_b=steps.cpu()), dict(steps_b=[4] * Bn), dict(t=5),
                   dict(t=0), dict(S=0), dict(temp=0.0), dict(top_k=3), dict(top_p=0.5)):
            a = dict(dict(t=2, temp=tv, steps_b=steps, S=4), **kw)
            with pytest.raises(ValueError):
                ops.psample_step_conf_listed(ld, x, un, a["t"], a["temp"], a["steps_b"], a["S"], SIGMA,
                                             **{k: v for k, v in a.items() if k in ("top_k", "top_p")})
        with pytest.raises(ValueError):
            ops.select_pending(un, 2, steps[:4])
    big = torch.zeros((2, 1, 65, 1), dtype=torch.bool, device=dev)
    with pytest.raises(NotImplementedError):
        ops.select_pending(big, 2, steps[:2].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(x, x0d) and torch.equal(un, un0d), "a refused call launched nothing"


# ------------------------------------------------------------------------------------------------- 3. the sampler
STEPS6 = [1, 3, 8, 8, 5, 12]
VARIANTS = {"plain": dict(), "vectors": dict(temp=TLIST, top_k=KLIST, top_p=PLIST)}
_REFS = {}


def _conf_sampler(den, graph):
    return sampler(den, True, True, graph)


def reference_rows(den, name, seed, steps=STEPS6, tail=True):
    """Row i of ``sample_confident(steps[i])`` at B = len(steps) under ``seed`` (eager, one call per distinct count), computed once."""
    key = (name, seed, tuple(steps), tail)
    if key not in _REFS:
        tail0 = den.use_step_tail
        den.use_step_tail = tail
        try:
            ab = _conf_sampler(den, False)
            ab.n_samples = len(steps)
            rows = {}
            for s in sorted(set(steps)):
                torch.manual_seed(seed)
                rows[s] = ab.sample_confident(s, **VARIANTS[name])
            _REFS[key] = torch.stack([rows[s][i] for i, s in enumerate(steps)])
        finally:
            den.use_step_tail = tail0
    return _REFS[key]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_sample_confident_with_a_step_vector_equals_the_one_count_calls_row_by_row(dev, name):
    den, _ = build_den(synth.MNIST, dev)
    Bn, seed = 6, 8100
    kw = VARIANTS[name]
    want = reference_rows(den, name, seed)
    assert torch.equal(want, reference_rows(den, name, seed, tail=False)), "the reference calls: fused step tail on and off"
    assert want.shape == (Bn, 1, 7, 7) and int(want.max()) < K128 and int(want.min()) >= 0
    bad = {}
    for graph in (False, True):
        ab = _conf_sampler(den, graph)
        ab.n_samples = Bn
        for rep in range(2 if graph else 1):                         # (a captured graph: a second replay)
            torch.manual_seed(seed)
            got = ab.sample_confident(STEPS6, **kw)
            bad[f"{'graph' if graph else 'eager'}_{rep}"] = int((got != want).sum())
            assert int(got.max()) < K128, "no mask_id is left"
        # every form of the argument: a tuple, a CPU tensor, a device tensor
        for form in (tuple(STEPS6), torch.tensor(STEPS6), torch.tensor(STEPS6, dtype=torch.int32, device=dev)):
            torch.manual_seed(seed)
            bad[f"{'graph' if graph else 'eager'}_{type(form).__name__}_{getattr(form, 'device', '')}"] = \
                int((ab.sample_confident(form, **kw) != want).sum())
        # all twelve: the one-count call
        torch.manual_seed(seed)
        all12 = ab.sample_confident([12] * Bn, **kw)
        twelve = _conf_sampler(den, False)
        twelve.n_samples = Bn
        torch.manual_seed(seed)
        bad[f"{'graph' if graph else 'eager'}_all12"] = int((all12 != twelve.sample_confident(12, **kw)).sum())
        assert len(ab._graphs) == (1 if graph else 0), "a second vector with the same maximum reuses the one graph"
        if graph:
            key, g = next(iter(ab._graphs.items()))
            assert "per-image-steps" in key and "confident" in key and 12 in key and g.steps is not None and g.confident
            # an int takes the existing path: a graph of its own, without the marker
            torch.manual_seed(seed)
            ab.sample_confident(12, **kw)
            assert len(ab._graphs) == 2 and sum("per-image-steps" in k for k in ab._graphs) == 1
    print(f"sample_confident per-image steps {name}: {bad}")
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 4. shards
def test_step_vector_on_two_shards_equals_the_whole_job(dev):
    den, _ = build_den(synth.MNIST, dev)
    Bn, seed = 6, 8100
    want = reference_rows(den, "vectors", seed)
    bad = {}
    for name, split in (("2+4", ((0, 2), (2, 6))), ("1+5", ((0, 1), (1, 6)))):
        for graph in (False, True):
            parts = []
            for lo, hi in split:
                sh = _conf_sampler(den, graph).set_shard(lo, hi - lo)
                torch.manual_seed(seed)
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    parts.append(sh.sample_confident(STEPS6[lo:hi], temp=TLIST[lo:hi], top_k=KLIST[lo:hi], top_p=PLIST[lo:hi]))
                assert not [str(w.message) for w in seen if "spkdiff" in str(w.message)], "no capture fall-back"
                assert sh.use_graph == graph and len(sh._graphs) == (1 if graph else 0)
            bad[f"{name}_{'graph' if graph else 'eager'}"] = int((torch.cat(parts) != want).sum())
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 5. completion
def test_complete_images_confident_positions_per_step(dev, ops):
    from spkdiff.complete import complete_images_confident
    from spkdiff.dist import complete_images_sharded
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    Bn, r, HW = 6, 4, 49
    images = (synth.stroke_images(Bn, seed=78, img=28, channels=1) - 0.5).to(dev)
    keep = torch.ones(Bn, 28, 28, dtype=torch.bool)
    keep[1, 12:14, 12:14] = False                # a 2 x 2 pixel hole: the four codes whose windows reach it
    keep[2, 14:] = False                         # the lower half
    keep[3] = False                              # nothing given
    keep[4, :, 20:] = False                      # the right columns
    keep[5, 0, 0] = False                        # one corner pixel: one code
    keep = keep.to(dev)
    ab = _conf_sampler(den, True)
    kw = dict(temp=0.9, top_p=0.95)
    torch.manual_seed(2031)
    res = complete_images_confident(model, ab, images, keep, positions_per_step=r, **kw)
    m = (HW - res.n_known.cpu().long()).tolist()
    assert m[0] == 0 and m[1] == 4 and m[3] == HW and m[5] == 1 and 4 < m[2] < HW and 4 < m[4] < HW, m
    steps = [cso.steps_for_hole(v, r) for v in m]
    assert steps[0] == steps[1] == steps[5] == 1 and steps[3] == 13 and len(set(steps)) >= 3
    codes = model.encode_images(images)
    assert int((res.tokens[res.known] != codes[res.known]).sum()) == 0, "known tokens come back unchanged"
    assert torch.equal(res.tokens[0], codes[0]), "nothing to fill: the image's own codes"
    assert int(res.tokens.max()) < K128 and int(res.tokens.min()) >= 0
    assert torch.equal((~res.known).flatten(1).sum(1).cpu(), torch.tensor(m))
    bad = {}
    ref = _conf_sampler(den, False)              # (the one-count references launch eagerly: no capture per count)
    for s in sorted(set(steps)):
        torch.manual_seed(2031)
        one = complete_images_confident(model, ref, images, keep, sample_steps=s, **kw)
        rows = [i for i in range(Bn) if steps[i] == s]
        bad[f"steps{s}_tokens"] = int((one.tokens[rows] != res.tokens[rows]).sum())
        bad[f"steps{s}_images"] = int((one.images_u8[rows] != res.images_u8[rows]).sum())
    # the step vector itself, as a list
    torch.manual_seed(2031)
    vec = complete_images_confident(model, ab, images, keep, sample_steps=steps, **kw)
    bad["vector"] = int((vec.tokens != res.tokens).sum())
    torch.manual_seed(2031)
    sh = complete_images_sharded(model, ab, images, keep, confident=True, positions_per_step=r, **kw)
    bad["sharded"] = int((sh != res.images_u8).sum())
    torch.manual_seed(2031)
    shv = complete_images_sharded(model, ab, images, keep, confident=True, sample_steps=steps, **kw)
    bad["sharded_vector"] = int((shv != res.images_u8).sum())
    print(f"positions_per_step={r}: m = {m}, steps = {steps}, {bad}")
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 6. the step-count sweep
def test_step_count_sweep_is_one_job(dev):
    from spkdiff.evaluate import step_count_sweep
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    ab = _conf_sampler(den, True)
    ab.n_samples, first0 = 3, ab.global_first
    steps, n = (2, 5), 3
    torch.manual_seed(2032)
    u4, t4 = step_count_sweep(model, ab, steps, n, batch=4, temp=0.9, top_k=30)
    torch.manual_seed(2032)
    u6, t6 = step_count_sweep(model, ab, steps, n, batch=6, temp=0.9, top_k=30)
    assert u4.shape == (2, 3, 1, 28, 28) and u4.dtype == torch.uint8 and t4.shape == (2, 3, 7, 7) and t4.dtype == torch.int64
    assert torch.equal(u4, u6) and torch.equal(t4, t6), "neither batch nor the grouping changes an image"
    assert (ab.n_samples, ab.global_first) == (3, first0)
    dense = _conf_sampler(den, False)
    for g, s in enumerate(steps):
        dense.set_shard(g * n, n)
        torch.manual_seed(2032)
        want = dense.sample_confident(s, temp=0.9, top_k=30).reshape(n, 7, 7)
        assert torch.equal(t4[g], want), f"group {g}: sample_confident({s}) at its global indices"
        assert torch.equal(u4[g], model.decode_tokens(want, 16, want_u8=True)[1])
    assert not torch.equal(t4[0], t4[1])
    with pytest.raises(ValueError):
        step_count_sweep(model, ab, (2, 0), n)


# ------------------------------------------------------------------------------------------------- 7. what the sampler refuses
def test_step_vector_refusals_leave_everything_untouched(dev):
    from spkdiff.complete import complete_images_confident
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    Bn = 5
    ab = _conf_sampler(den, True)
    ab.n_samples = Bn
    rank = _conf_sampler(den, True)
    rank.n_samples, rank.noise_layout = Bn, 'rank'
    big = sampler(den, True, True, True, latent=9)
    big.n_samples = Bn
    g = torch.Generator().manual_seed(3)
    x_init = torch.randint(0, K128, (Bn, 1, 7, 7), generator=g).to(dev)
    known = (torch.rand(Bn, 1, 7, 7, generator=g) < 0.5).to(dev)
    x0, k0 = x_init.clone(), known.clone()
    images = (synth.stroke_images(Bn, seed=79, img=28, channels=1) - 0.5).to(dev)
    keep = torch.ones(Bn, 28, 28, dtype=torch.bool, device=dev)
    good = [2, 3, 1, 4, 2]
    torch.manual_seed(5)
    state = torch.get_rng_state()
    cases = [(ValueError, lambda: ab.sample_confident(good, record=[], x_init=x_init, known=known)),
             (ValueError, lambda: rank.sample_confident(good, x_init=x_init, known=known)),
             (ValueError, lambda: ab.sample_confident(good[:4], x_init=x_init, known=known)),
             (ValueError, lambda: ab.sample_confident(good + [1])),
             (ValueError, lambda: ab.sample_confident([2, 0, 1, 4, 2], x_init=x_init, known=known)),
             (ValueError, lambda: ab.sample_confident(torch.tensor([2, 0, 1, 4, 2], device=dev))),
             (ValueError, lambda: complete_images_confident(model, ab, images, keep, sample_steps=3, positions_per_step=4)),
             (ValueError, lambda: complete_images_confident(model, ab, images, keep, positions_per_step=0)),
             (NotImplementedError, lambda: big.sample_confident(good))]
    for i, (exc, call) in enumerate(cases):
        with pytest.raises(exc):
            call()
        assert torch.equal(torch.get_rng_state(), state), f"case {i} drew from the generator"
    torch.cuda.synchronize()
    assert torch.equal(x_init, x0) and torch.equal(known, k0)
    assert len(ab._graphs) == 0 and len(rank._graphs) == 0 and len(big._graphs) == 0
    assert ab.last_key is None and rank.last_key is None and big.last_key is None
