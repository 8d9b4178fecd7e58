"""GPU tests of the likelihood-bound feature (run with ``-m gpu`` on an MI355X): spk_pscore_step against its
numpy fp64 restatement (tests/_score_oracle.py), ``AbsorbingDiffusion.score`` against the trajectory of ``sample()`` it forces,
against itself across launch forms, graph replays, splits and ``known=`` starts, against the host oracle on the dumped Philox
noise, its normalisation over a codebook, and ``spkdiff.evaluate.token_nll_eval`` end to end.

Tolerances.  Kernel against numpy: both sides evaluate the same fp64 formula on the same fp32 z = logits / temp, so they differ by
the summation order and libm ulps over at most 512 terms, ~1e-13: 1e-9 + 1e-12 |logp| leaves margin and is far below what a wrong
index or a wrong z gives.  Device against the host oracle's denoiser: 2 * 1e-5 / temp + 1e-9 -- 1e-5 is the absolute logit agreement
tests/test_gpu_parity.py holds the device to on synthetic weights, and a log-softmax moves by at most twice the largest logit
change.  Everything else is exact."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _completion_oracle as corc           # noqa: E402
import _score_oracle as sorc                # noqa: E402
from parity_report import record as parity  # noqa: E402
from spkdiff import synth                  # noqa: E402
from test_gpu_completion import FORMS, K, build_den, build_vae, sampler      # noqa: E402  (the helpers, not the tests)

SENT_LP, SENT_STEP = -12345.0, -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def _close(got, want):
    """|got - want| <= 1e-9 + 1e-12 |want| where finite; NaN and the infinities must sit at the same places.  Returns the largest
    finite difference."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), "infinite positions differ"
    fin = np.isfinite(want)
    d = np.abs(got[fin] - want[fin])
    assert np.all(d <= 1e-9 + 1e-12 * np.abs(want[fin])), f"max |d logp| {d.max():.3e}"
    return float(d.max()) if d.size else 0.0


# ------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("temp", [1.0, 0.7])
@pytest.mark.parametrize("t", [1, 2, 49])
@pytest.mark.parametrize("B,HW,Kc", [(1, 49, 1), (5, 49, 7), (257, 49, 128), (3, 64, 200), (2, 64, 512)])
def test_pscore_step_equals_the_numpy_step(dev, ops, B, HW, Kc, t, temp):
    h = int(math.isqrt(HW))
    g = torch.Generator().manual_seed(B * 1000 + Kc + t)
    logits = torch.randn(B, Kc, h, h, generator=g) * 3
    x0 = torch.randint(0, Kc, (B, HW), generator=g)
    prior = torch.rand(B, HW, generator=g) < 0.5
    x_start = torch.where(prior, torch.randint(0, Kc, (B, HW), generator=g), torch.full((B, HW), Kc))
    u_inj = torch.rand(B, HW, generator=g)
    # rows with special values, all forced to change (injected noise): a NaN logit, a -inf target logit, every logit -inf, a
    # target above / below the codebook
    lg3 = logits.view(B, Kc, HW)
    lg3[0, Kc // 2, 0] = float("nan")
    lg3[0, x0[0, 1], 1] = float("-inf")
    lg3[0, :, 2] = float("-inf")
    x0[0, 3], x0[0, 4] = Kc + 3, -1
    prior[0, :5], u_inj[0, :5] = False, 0.0
    x_start[0, :5] = Kc
    seed, off, base = 0x1234_5678_9ABC, 3 * (1 << 40) + 17 * HW * Kc, 1 << 33
    u_phi = ops.philox_noise(seed, off, B, HW, Kc, dev, want_q=False)[0]
    state = torch.tensor([seed, base], dtype=torch.int64, device=dev)
    u_state = ops.philox_noise(99, off - base, B, HW, Kc, dev, philox_state=state, want_q=False)[0]
    assert torch.equal(u_phi, u_state)
    # a shuffled partial active list; the slots beyond it hold NaN logits and must never be read
    n_act = max(1, (B + 1) // 2)
    perm = torch.randperm(B, generator=g)
    act = torch.zeros(B, dtype=torch.int32)
    act[:n_act] = perm[:n_act].to(torch.int32)
    slots = torch.full((B, Kc, h, h), float("nan"))
    slots[:n_act] = logits[perm[:n_act]]
    worst, n_changes = 0.0, 0
    for mode in ("injected", "philox", "philox_state", "active_injected", "active_philox"):
        u_dev = u_inj.to(dev) if mode.endswith("injected") else None
        u_host = (u_inj if u_dev is not None else u_phi.cpu()).numpy()
        x_t = x_start.clone().view(B, 1, h, h).to(dev)
        unmasked = prior.clone().view(B, 1, h, h).to(dev)
        logp = torch.full((B, h, h), SENT_LP, dtype=torch.float64, device=dev)
        step = torch.full((B, h, h), SENT_STEP, dtype=torch.int32, device=dev)
        kw = dict(u=u_dev, seed=seed, offset=off)
        if mode == "philox_state":
            kw = dict(u=None, seed=99, offset=off - base, philox_state=state)
        images = None
        if mode.startswith("active"):
            images = act[:n_act].numpy()
            with ops.active_set(act.to(dev), torch.tensor([n_act, 0], dtype=torch.int32, device=dev)):
                ops.pscore_step(slots.to(dev), x0.to(dev), x_t, unmasked, t, temp, logp, step, **kw)
        else:
            nxt = torch.full((B, 2, h, h), float("nan"), device=dev)
            ops.pscore_step(logits.to(dev), x0.to(dev), x_t, unmasked, t, temp, logp, step, next_input=nxt, **kw)
            assert torch.equal(nxt, ops.den_build_input(x_t, t - 1)), "next_input = the next step's denoiser input"
        wx, wu = x_start.clone().numpy(), prior.clone().numpy()
        wl = np.full((B, HW), SENT_LP, dtype=np.float64)
        ws = np.full((B, HW), SENT_STEP, dtype=np.int32)
        changes = sorc.pscore_step(logits.numpy(), x0.numpy(), wx, wu, t, temp, u_host, wl, ws, images=images)
        got_changes = (unmasked.cpu().view(B, HW) & ~prior).numpy()
        assert np.array_equal(got_changes, changes), mode
        assert np.array_equal(x_t.cpu().view(B, HW).numpy(), wx) and np.array_equal(unmasked.cpu().view(B, HW).numpy(), wu), mode
        assert np.array_equal(step.cpu().view(B, HW).numpy(), ws), mode
        got = logp.cpu().view(B, HW).numpy()
        assert np.all(got[~changes] == SENT_LP), "a position that does not change keeps the sentinel"
        worst = max(worst, _close(got[changes], wl[changes]))
        n_changes += int(changes.sum())
        if mode == "injected":
            sp = got[0, :5]
            assert changes[0, :5].all() and np.isnan(sp[2]) and sp[3] == -np.inf and sp[4] == -np.inf
            if Kc > 1:
                assert np.isnan(sp[0]) and sp[1] == -np.inf
    assert n_changes > 0
    parity(f"pscore_step_B{B}_HW{HW}_K{Kc}_t{t}_temp{temp}", changes=n_changes, max_abs_dlogp=worst)


def test_pscore_wrapper_refuses_bad_arguments(dev, ops):
    lg = torch.zeros(2, 8, 7, 7, device=dev)
    x0 = torch.zeros(2, 49, dtype=torch.int64, device=dev)
    x_t, un = torch.zeros(2, 1, 7, 7, dtype=torch.int64, device=dev), torch.zeros(2, 1, 7, 7, dtype=torch.bool, device=dev)
    lp, st = torch.zeros(2, 49, dtype=torch.float64, device=dev), torch.zeros(2, 49, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="spk_pscore_step"):
        ops.pscore_step(lg, x0, x_t, un, 0, 1.0, lp, st)
    with pytest.raises(ValueError, match="spk_pscore_step"):
        ops.pscore_step(lg, x0, x_t, un, 3, 0.0, lp, st)
    with pytest.raises(NotImplementedError, match="spk_pscore_step"):
        ops.pscore_step(torch.zeros(1, 513, 1, 1, device=dev), x0[:1, :1], x_t[:1, :, :1, :1], un[:1, :, :1, :1].contiguous(), 3, 1.0,
                        lp[:1, :1], st[:1, :1])
    with pytest.raises(ValueError):
        ops.pscore_step(lg, x0[:1], x_t, un, 3, 1.0, lp, st)
    with pytest.raises(ValueError):
        ops.pscore_step(lg, x0, x_t, un, 3, 1.0, lp.float(), st)
    with pytest.raises(ValueError):
        ops.pscore_step(lg, x0, x_t, un, 3, 1.0, lp, st.long())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pscore_step(lg, x0.cpu(), x_t, un, 3, 1.0, lp, st)
    assert not lp.any() and not st.any() and not un.any()


# ------------------------------------------------------------------------------------------------- 2. sample, then score
def test_score_forces_the_trajectory_of_the_sample(dev):
    den, _ = build_den(synth.MNIST, dev)
    B, steps, temp = 4, 49, 0.8
    g = torch.Generator().manual_seed(12)
    draws = {t: (torch.rand(B, 1, 7, 7, generator=g).to(dev), torch.empty(B * 49, K).exponential_(1, generator=g).to(dev))
             for t in range(1, steps + 1)}
    ab = sampler(den, False, False, False)
    ab.n_samples = B
    tail = den.use_step_tail
    den.use_step_tail = False                     # the form named 'dense': conv6, then the token update, as score() runs it
    try:
        assert ab.form_for(B, 7, 7) == "dense"
        rec_s, rec_c = [], []
        X = ab.sample(temp, steps, noise=lambda t: draws[t], record=rec_s)
    finally:
        den.use_step_tail = tail
    sc = ab.score(X, temp, steps, noise=lambda t: draws[t], record=rec_c)
    assert sc.position_log_prob.shape == (1, B, 7, 7) and sc.position_log_prob.dtype == torch.float64
    assert sc.reveal_step.shape == (1, B, 7, 7) and sc.reveal_step.dtype == torch.int32
    assert sc.log_prob.shape == (1, B) and sc.log_prob.dtype == torch.float64 and sc.log_prob.is_cuda
    assert len(rec_s) == len(rec_c) == steps
    state_bad = logits_bad = 0
    first_on = torch.zeros(B, 1, 7, 7, dtype=torch.int32)
    prev = torch.zeros(B, 1, 7, 7, dtype=torch.bool)
    want = np.zeros((B, 49))
    Xh = X.cpu().view(B, 49)
    for (ts, xs, us, ls), (tc, xc, uc, lc) in zip(rec_s, rec_c):
        assert ts == tc
        state_bad += int((xs != xc).sum()) + int((us != uc).sum())
        logits_bad += int((ls.view(torch.int32) != lc.view(torch.int32)).sum())
        new = us.cpu() & ~prev
        first_on[new] = ts
        prev = us.cpu()
        z = (ls.cpu().view(B, K, 49).numpy() / np.float32(temp))
        for b, p in np.argwhere(new.view(B, 49).numpy()):
            want[b, p] = sorc.log_prob(z[b, :, p], int(Xh[b, p]))
    assert state_bad == 0 and logits_bad == 0
    assert torch.equal(rec_c[-1][1], X) and bool(prev.all())
    step = sc.reveal_step[0].cpu()
    assert torch.equal(step.view(B, 1, 7, 7), first_on) and int(step.min()) >= 1 and int(step.max()) <= steps
    worst = _close(sc.position_log_prob[0].cpu().view(B, 49).numpy(), want)
    assert torch.equal(sc.log_prob, sc.position_log_prob.sum(dim=(2, 3)))
    assert abs(float(sc.bits_per_dim(49)) + float(sc.log_prob.mean()) / (math.log(2) * 49)) < 1e-12
    parity("score_forces_sample_trajectory", state_mismatches=state_bad, logits_bits_differing=logits_bad, max_abs_dlogp=worst,
           bits_per_dim=float(sc.bits_per_dim()))


# ------------------------------------------------------------------------------------------------- 3. the forms agree
@pytest.mark.parametrize("L,B,steps", [(7, 32, 49), (8, 3, 16)], ids=["7x7_B32", "8x8_B3"])
def test_forms_agree_and_x0_is_a_graph_input(dev, L, B, steps):
    cfg = synth.MNIST if L == 7 else synth.CIFAR
    den, _ = build_den(cfg, dev)
    g = torch.Generator().manual_seed(L)
    x_a = torch.randint(0, K, (B, 1, L, L), generator=g).to(dev)
    x_b = torch.randint(0, K, (B, L, L), generator=g).to(dev)
    out = {}
    for graph in (True, False):
        for name, skip, lists in FORMS:
            ab = sampler(den, skip, lists, graph, latent=L)
            f = ab._form(B, L, L)
            assert (f.skip, f.lists) == (skip, skip and lists and L == 7), "B is above list_min_batch: the lists really run"
            ab.n_samples = B
            torch.manual_seed(9)
            tok = ab.sample(0.9, steps)
            res = []
            for x, seed in ((x_a, 1), (x_a, 2), (x_b, 1), (x_a, 1)):          # seeds and inputs through ONE captured graph
                torch.manual_seed(seed)
                res.append(ab.score(x, 0.9, steps))
            assert len(ab._graphs) == (2 if graph else 0)                      # sample()'s graph and the score graph
            torch.manual_seed(9)
            assert torch.equal(ab.sample(0.9, steps), tok) and len(ab._graphs) == (2 if graph else 0)
            out[(name, graph)] = res
    first = out[("dense", False)]
    bad = 0
    for res in out.values():
        for a, b in zip(res, first):
            bad += int((a.position_log_prob.view(torch.int64) != b.position_log_prob.view(torch.int64)).sum())
            bad += int((a.reveal_step != b.reveal_step).sum()) + int((a.log_prob.view(torch.int64) != b.log_prob.view(torch.int64)).sum())
    s1, s2, s3, s4 = first
    assert not torch.equal(s1.reveal_step, s2.reveal_step) and not torch.equal(s1.position_log_prob, s2.position_log_prob)
    assert torch.equal(s1.reveal_step, s3.reveal_step) and not torch.equal(s1.position_log_prob, s3.position_log_prob)
    assert torch.equal(s1.position_log_prob, s4.position_log_prob) and torch.equal(s1.reveal_step, s4.reveal_step)
    assert int(s1.reveal_step.min()) >= 1 and bool(torch.isfinite(s1.position_log_prob).all()) and bool((s1.position_log_prob < 0).all())
    parity(f"score_forms_agree_{L}x{L}_B{B}", forms=len(out), calls=4, differing_values=bad, bits_per_dim=float(s1.bits_per_dim()))
    assert bad == 0


# ------------------------------------------------------------------------------------------------- 4. against the oracle
def _oracle_check(name, dev, ops, sd, ab, x_0, known, steps, temp, seed):
    """score() in the captured Philox form against tests/_score_oracle.run (exact convolutions) on the noise the device drew."""
    B, L = x_0.shape[0], x_0.shape[-1]
    torch.manual_seed(seed)
    key = ab._philox_key()
    torch.manual_seed(seed)
    sc = ab.score(x_0.to(dev), temp, steps, known=None if known is None else known.to(dev))
    assert int(ab.last_key) == key and len(ab._graphs) == 1, "replayed from a captured hipGraph"

    def noise(t):
        return ops.philox_noise(key, (steps - t) * corc.STEP_STRIDE, B, L * L, K, dev, want_q=False)[0].cpu().view(B, 1, L, L)
    wl, ws, wx, _ = sorc.run(sd, x_0, known, steps, noise, K=K, temp=temp, exact_conv=True)
    step_bad = int((sc.reveal_step[0].cpu().numpy() != ws).sum())
    got = sc.position_log_prob[0].cpu().numpy()
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(wl))
    err = float(np.abs(got - wl).max())
    print(f"{name}: reveal steps differing {step_bad} of {ws.size}, max |d position_log_prob| {err:.3e} (bound {2e-5 / temp + 1e-9:.3e})")
    parity(name, reveal_steps_differing=step_bad, max_abs_dlogp=err, bound=2e-5 / temp + 1e-9, nats_per_image=float(-wl.sum() / B))
    assert step_bad == 0
    assert err <= 2e-5 / temp + 1e-9
    return sc, wl, ws


@pytest.mark.parametrize("B,steps", [(4, 100), (256, 6)])
def test_score_philox_graph_vs_oracle_on_dumped_noise(dev, ops, B, steps):
    den, sd = build_den(synth.MNIST, dev)
    x_0 = corc.issue_start(B)[0]
    ab = sampler(den, True, True, True)
    _oracle_check(f"score_philox_graph_B{B}_{steps}steps", dev, ops, sd, ab, x_0, None, steps, 1.0, 777)


# ------------------------------------------------------------------------------------------------- 5. known=
def test_known_starts(dev, ops):
    den, sd = build_den(synth.MNIST, dev)
    B, steps = 8, 12
    x_0, known = corc.issue_start(B)
    none = torch.zeros(B, 1, 7, 7, dtype=torch.bool, device=dev)
    every = torch.ones(B, 7, 7, dtype=torch.uint8, device=dev)
    for graph in (True, False):
        ab = sampler(den, True, True, graph)
        torch.manual_seed(5)
        plain = ab.score(x_0.to(dev), 1.0, steps)
        torch.manual_seed(5)
        cond = ab.score(x_0.to(dev), 1.0, steps, known=none)
        assert torch.equal(plain.position_log_prob, cond.position_log_prob) and torch.equal(plain.reveal_step, cond.reveal_step)
        assert torch.equal(plain.log_prob, cond.log_prob) and ab.n_samples == 3
        full = ab.score(x_0[:, 0].to(dev), 1.0, steps, known=every)
        assert not full.log_prob.any() and not full.reveal_step.any() and not full.position_log_prob.any()
    rec = []
    ab = sampler(den, True, True, False)
    ab.score(x_0.to(dev), 1.0, 3, known=every.view(B, 1, 7, 7), record=rec)
    assert len(rec) == 3 and all(torch.equal(r[1].cpu(), x_0) and bool(r[2].all()) for r in rec), "the tokens are untouched"
    # mixed masks: known positions hold 0 / 0, the rest is the oracle's conditional score
    ab = sampler(den, True, True, True)
    sc, wl, ws = _oracle_check("score_known_mixed_masks", dev, ops, sd, ab, x_0, known, steps, 1.0, 31)
    kn = known[:, 0]
    assert not sc.position_log_prob[0].cpu()[kn].any() and not sc.reveal_step[0].cpu()[kn].any()
    assert bool((sc.reveal_step[0].cpu()[~kn] >= 1).all()) and not wl[kn.numpy()].any() and not ws[kn.numpy()].any()


# ------------------------------------------------------------------------------------------------- 6. normalisation
def test_one_open_position_is_a_normalised_distribution(dev):
    den, _ = build_den(synth.MNIST, dev)
    g = torch.Generator().manual_seed(6)
    row = torch.randint(0, K, (1, 1, 7, 7), generator=g)
    x_0 = row.repeat(K, 1, 1, 1)
    x_0[:, 0, 3, 4] = torch.arange(K)                      # the 128 images differ in this token only
    known = torch.ones(K, 1, 7, 7, dtype=torch.bool)
    known[:, 0, 3, 4] = False
    u = torch.full((K, 1, 7, 7), 0.03, device=dev)         # < 1/t from t = 33 down: one reveal step for all images
    for temp in (1.0, 0.7):
        for skip, lists in ((True, True), (False, False)):
            ab = sampler(den, skip, lists, True)
            sc = ab.score(x_0.to(dev), temp, 49, noise=lambda t: (u, None), known=known.to(dev))
            assert bool((sc.reveal_step[0, :, 3, 4] == 33).all()) and int(sc.reveal_step.sum()) == 33 * K
            total = float(torch.exp(sc.log_prob[0]).sum())
            parity(f"score_normalisation_temp{temp}_{'elim' if skip else 'dense'}", sum_of_probabilities=total)
            assert abs(total - 1.0) <= 1e-9


# ------------------------------------------------------------------------------------------------- 7. split independence
def test_score_does_not_depend_on_the_split(dev):
    den, _ = build_den(synth.MNIST, dev)
    steps = 20
    x_0, known = corc.issue_start(8)
    x_0, known = x_0.to(dev), known.to(dev)
    for kn in (None, known):
        ab = sampler(den, True, True, True)
        torch.manual_seed(606)
        whole = ab.score(x_0, 1.0, steps, known=kn)
        parts = []
        for lo, n in ((0, 5), (5, 3)):
            sh = sampler(den, True, True, True).set_shard(lo, n)
            torch.manual_seed(606)
            parts.append(sh.score(x_0[lo:lo + n], 1.0, steps, known=None if kn is None else kn[lo:lo + n]))
            assert sh.last_key == ab.last_key
        for f in ("position_log_prob", "reveal_step", "log_prob"):
            assert torch.equal(torch.cat([getattr(p, f) for p in parts], dim=1), getattr(whole, f)), f
        # the second part alone is NOT the first part's noise: the counters sit on the global image index
        un = sampler(den, True, True, True)
        torch.manual_seed(606)
        assert not torch.equal(un.score(x_0[5:], 1.0, steps, known=None if kn is None else kn[5:]).reveal_step, parts[1].reveal_step)


# ------------------------------------------------------------------------------------------------- 8. end to end
def test_token_nll_eval(dev):
    from spkdiff.evaluate import token_nll_eval
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    ab = sampler(den, True, True, True)
    images = synth.stroke_images(8, seed=41)
    batches = [images[:5], (images[5:], torch.zeros(3))]            # unequal sizes; bare images and (images, labels)
    steps, orders = 12, 2
    torch.manual_seed(8)
    res = token_nll_eval(model, ab, batches, temp=0.9, sample_steps=steps, orders=orders)
    torch.manual_seed(8)
    lps = []
    for im in (images[:5], images[5:]):
        codes = model.encode_images((im - 0.5).to(dev))
        assert codes.shape == (im.shape[0], 7, 7)
        lps.append(ab.score(codes, 0.9, steps, orders=orders).log_prob)
    lp = torch.cat(lps, dim=1)
    assert lp.shape == (orders, 8) and not torch.equal(lp[0], lp[1]), "every order draws a key of its own"
    assert res["n_images"] == 8 and res["orders"] == orders and set(res) == {"bits_per_dim", "nats_per_image", "n_images", "orders"}
    nats = -float(lp.mean())
    assert abs(res["nats_per_image"] - nats) <= 1e-12 * abs(nats)
    assert abs(res["bits_per_dim"] - nats / (math.log(2) * 49)) <= 1e-12 * abs(nats)
    assert math.isfinite(res["bits_per_dim"]) and res["bits_per_dim"] > 0
    parity("token_nll_eval", **res)
    with pytest.raises(ValueError):
        token_nll_eval(model, ab, [])
