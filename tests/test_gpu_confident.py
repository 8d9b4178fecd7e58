"""GPU tests of confidence-ordered decoding (run with ``-m gpu`` on an MI355X): ``spk_psample_step_conf`` against
the oracle of tests/_confident_oracle.py (candidates == the `_topp` entry point's x0_hat, the commit rule exactly, the fp32 confidence
within the counted bound of fp64), ties and non-finite rows, ``spk_den_step_tail_conf`` against the three-launch form bit for bit,
``AbsorbingDiffusion.sample_confident`` in every form, eager and captured, step by step from a record, greedy, across shards, the
completion wrapper, and what the wrappers refuse."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _confident_oracle as cfo             # noqa: E402
from spkdiff import synth                  # noqa: E402
from test_gpu_completion import K as K128, build_den, build_vae, sampler      # noqa: E402  (the helpers, not the tests)
from test_gpu_temps import _active, _den_k, _state      # noqa: E402

NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def conf_call(ops, dev, logits, x0, un0, t, temp, top_k, top_p, nxt=False, **noise):
    """One confidence-ordered token update on copies of the state -> (x_t, unmasked, x0_hat, conf, next_input or None); the two
    outputs are pre-filled with sentinels the kernel must leave where a position is not masked."""
    n = x0.numel()
    x, un = x0.clone(), un0.clone()
    hat = torch.full((n,), -5, dtype=torch.int64, device=dev)
    conf = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    ni = torch.full((x0.shape[0], 2) + tuple(logits.shape[2:]), float("nan"), device=dev) if nxt else None
    ops.psample_step_conf(logits, x, un, t, temp, x0_hat=hat, conf=conf, next_input=ni, top_k=top_k, top_p=top_p, **noise)
    return x, un, hat, conf, ni


def check_step(ops, dev, logits, x0, un0, t, temp, top_k, top_p, noise, ref=None, nxt=True):
    """The checks every confidence-ordered step must pass, on device tensors logits [B,K,..], x0 / un0 [B,1,..]; ``ref`` = the
    host rows of tests/_confident_oracle.reference_rows (None: no comparison with fp64).  Returns (x, un, stats, worst ratio of
    |conf - fp64| to the counted bound)."""
    Bn, K = logits.shape[0], logits.shape[1]
    HW = logits[0, 0].numel()
    x, un, hat, conf, ni = conf_call(ops, dev, logits, x0, un0, t, temp, top_k, top_p, nxt=nxt, **noise)
    # the candidates: the x0_hat spk_psample_step_topp reports for the same inputs (its coin is irrelevant to x0_hat)
    xs, uns = x0.clone(), un0.clone()
    sib = torch.full((Bn * HW,), -5, dtype=torch.int64, device=dev)
    ops.psample_step(logits, xs, uns, t, temp, x0_hat=sib, top_k=top_k, top_p=top_p, **noise)
    masked = ~un0.flatten().cpu()
    hat_c, conf_c, sib_c = hat.cpu(), conf.cpu(), sib.cpu()
    stats = dict(cand_differs=int((hat_c[masked] != sib_c[masked]).sum()),
                 touched_unmasked=int((hat_c[~masked] != -5).sum()) + int((conf_c[~masked] != 7.0).sum()))
    # the commit, given the kernel's own candidates and confidences: exactly the oracle's
    xh, unh = x0.cpu().reshape(Bn, HW), un0.cpu().reshape(Bn, HW).bool()
    wx, wun, rev = cfo.commit_state(xh, unh, hat_c.reshape(Bn, HW), conf_c.reshape(Bn, HW), t)
    stats["state_differs"] = int((x.cpu().reshape(Bn, HW) != wx).sum()) + int((un.cpu().reshape(Bn, HW).bool() != wun).sum())
    stats["count_differs"] = sum(int(rev[b].sum()) != cfo.n_reveal(int((~unh[b]).sum()), t) for b in range(Bn))
    if nxt:
        stats["next_input"] = int(not torch.equal(ni, ops.den_build_input(x, t - 1)))
    worst = 0.0
    if ref is not None:
        z32, zt, fcut, on = ref
        sel = masked & ~fcut & ~torch.isnan(z32).any(-1) & torch.isfinite(zt).any(-1)
        want = cfo.log_prob_f64(zt[sel], hat_c[sel])
        bound = cfo.conf_bound(K, zt[sel].max(-1).values.numpy(), want.numpy())
        err = (conf_c[sel].double() - want).abs().numpy()
        if err.size:
            worst = float((err / bound).max())
        stats["conf_outside_bound"] = int((err > bound).sum())
        stats["cand_not_kept"] = int((~torch.isfinite(zt[sel].gather(1, hat_c[sel][:, None])[:, 0])).sum())
    return x, un, stats, worst


# ------------------------------------------------------------------------------------------------- 1. the sampling kernel
@pytest.mark.parametrize("HW", cfo.HWS)
@pytest.mark.parametrize("K", cfo.KS)
def test_psample_step_conf_vs_oracle(dev, ops, K, HW):
    """The seeded case table (tests/_confident_oracle.conf_inputs): B = 5, start states with m = 0, 1, 2, HW - 1, HW masked positions
    in one batch, per-image temperature / k / p, t in {1, 2, m, m + 1, 100}; injected q, Philox and philox_state.  Candidates equal
    spk_psample_step_topp's x0_hat bit for bit; given the kernel's own conf_out and candidates the committed state is the oracle's
    exactly; ceil(m / t) positions per image are revealed; nothing is written where a position is not masked; conf_out is within the
    counted bound of the fp64 log-softmax on every row whose truncation the host can decide (tests/_topp_oracle.fragile_cut)."""
    logits, q, x0, un0, temps, ks, ps = cfo.conf_inputs(K, HW)
    ref = cfo.reference_rows(logits, temps, ks, ps)
    ld, x0d, un0d, tv, kd, pd = (v.to(dev) for v in (logits, x0, un0, temps, ks, ps))
    seed, off = 0x1234_5678_9ABC, 5 * (1 << 40) + 11 * HW * K
    state = torch.tensor([seed, 1 << 33], dtype=torch.int64, device=dev)
    noises = {"injected": dict(q=q.to(dev)), "philox": dict(seed=seed, offset=off),
              "philox_state": dict(seed=99, offset=off - (1 << 33), philox_state=state)}
    total, worst, seen = {}, 0.0, {}
    for t in cfo.steps_of(HW):
        for mode, kw in noises.items():
            x, un, stats, w = check_step(ops, dev, ld, x0d, un0d, t, tv, kd, pd, kw, ref=ref)
            worst = max(worst, w)
            for k, v in stats.items():
                total[k] = total.get(k, 0) + v
            seen[t, mode] = (x, un)
        # philox_state names the same counters: the same step
        total["state_form_differs"] = total.get("state_form_differs", 0) + sum(
            int(not torch.equal(a, b)) for a, b in zip(seen[t, "philox"], seen[t, "philox_state"]))
        # an injected u is ignored
        xu, unu, _, _, _ = conf_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, u=torch.zeros(cfo.B * HW, device=dev), **noises["philox"])
        total["u_matters"] = total.get("u_matters", 0) + int(not torch.equal(xu, seen[t, "philox"][0]))
    # t = 1 reveals everything
    assert bool(seen[1, "philox"][1].all()) and int(seen[1, "philox"][0].max()) < K
    print(f"conf K={K} HW={HW}: {total}, largest |conf - fp64| / bound {worst:.4f}")
    assert all(v == 0 for v in total.values()), total
    assert worst <= 1.0


def test_psample_step_conf_refuses_more_than_64_positions(dev, ops):
    g = torch.Generator().manual_seed(65)
    logits = torch.randn(2, 16, 65, 1, generator=g).to(dev)
    x0 = torch.full((2, 1, 65, 1), 16, dtype=torch.int64, device=dev)
    un0 = torch.zeros((2, 1, 65, 1), dtype=torch.bool, device=dev)
    x, un = x0.clone(), un0.clone()
    with pytest.raises(NotImplementedError):
        ops.psample_step_conf(logits, x, un, 2, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(un, un0), "a refused call launched nothing"


# ------------------------------------------------------------------------------------------------- 2. ties and non-finite rows
def test_ties_go_to_the_lower_position_and_non_finite_rows_order_last(dev, ops):
    K, HW, Bn = 64, 49, 3
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(Bn, K, HW, 1, generator=g) * 0.05                # flat rows: confidences near -ln 64
    q = torch.empty(Bn, HW, K).exponential_(1, generator=g)
    # image 0: one row and one q at every position -- 49 identical keys
    logits[0] = logits[0, :, :1].clone()
    q[0] = q[0, :1].clone()
    # image 1: a peaked row (and one q) at the positions of G -- five identical keys above every other
    G = [3, 10, 11, 30, 40]
    peaked = torch.randn(K, generator=g) * 0.05
    peaked[17] = 12.0
    logits[1][:, G, 0] = peaked[:, None]
    q[1, G] = q[1, G[0]].clone()
    # image 2: a NaN at position 0, every class at -inf at position 1
    logits[2, 5, 0, 0] = float("nan")
    logits[2, :, 1, 0] = NEG_INF
    ld, qd = logits.to(dev), q.reshape(Bn * HW, K).to(dev)
    x0 = torch.full((Bn, 1, HW, 1), K, dtype=torch.int64, device=dev)
    un0 = torch.zeros((Bn, 1, HW, 1), dtype=torch.bool, device=dev)
    # all masked, t = 17: n = 3
    x, un, hat, conf, _ = conf_call(ops, dev, ld, x0, un0, 17, 1.0, None, None, q=qd)
    unc, cc, hc = un.cpu().reshape(Bn, HW), conf.cpu().reshape(Bn, HW), hat.cpu().reshape(Bn, HW)
    assert cfo.n_reveal(49, 17) == 3
    assert len(set(cc[0].tolist())) == 1 and len(set(hc[0].tolist())) == 1, "identical rows and noise: identical candidates and keys"
    assert unc[0].nonzero().flatten().tolist() == [0, 1, 2]
    assert len(set(cc[1][G].tolist())) == 1 and float(cc[1][G[0]]) > float(np.delete(cc[1].numpy(), G).max())
    assert unc[1].nonzero().flatten().tolist() == G[:3], "the cut falls inside the tie group: the lower positions win"
    assert bool((hc[1][G] == 17).all())
    # the non-finite rows: confidence NaN, token 0, ordered last -- not among the 25 of t = 2, revealed at t = 1
    assert bool(torch.isnan(cc[2][:2]).all()) and hc[2][:2].tolist() == [0, 0] and not bool(torch.isnan(cc[2][2:]).any())
    x2, un2, _, _, _ = conf_call(ops, dev, ld, x0, un0, 2, 1.0, None, None, q=qd)
    u2 = un2.cpu().reshape(Bn, HW)
    assert int(u2[2].sum()) == 25 and not bool(u2[2][:2].any())
    x1, un1, _, _, _ = conf_call(ops, dev, ld, x0, un0, 1, 1.0, None, None, q=qd)
    assert bool(un1.all()) and x1.cpu().reshape(Bn, HW)[2][:2].tolist() == [0, 0]
    # between the two non-finite rows the lower position wins: masked = {0, 1, 5}, t = 2 -> n = 2 -> {5, 0}
    un3 = torch.ones((Bn, 1, HW, 1), dtype=torch.bool)
    un3[2, 0, [0, 1, 5], 0] = False
    x3 = torch.where(un3, torch.zeros((), dtype=torch.int64), torch.full((), K, dtype=torch.int64))
    xo, uno, _, _, _ = conf_call(ops, dev, ld, x3.to(dev), un3.to(dev), 2, 1.0, None, None, q=qd)
    assert (~uno.cpu().reshape(Bn, HW)[2]).nonzero().flatten().tolist() == [1]
    # greedy rows (top_k = 1): every confidence is exactly 0, so the lowest positions are revealed
    k1 = torch.ones(Bn, dtype=torch.int32, device=dev)
    xg, ung, hg, cg, _ = conf_call(ops, dev, ld[:2], x0[:2], un0[:2], 17, 1.0, k1[:2], None, q=qd[:2 * HW])
    assert bool((cg == 0).all()) and ung.cpu().reshape(2, HW)[1].nonzero().flatten().tolist() == [0, 1, 2]
    assert torch.equal(hg.cpu().reshape(2, HW), logits[:2, :, :, 0].argmax(1))


# ------------------------------------------------------------------------------------------------- 3. the fused step tail
@pytest.mark.parametrize("L", [7, 8])
@pytest.mark.parametrize("Kc", [100, 128, 256, 512])
def test_den_step_tail_conf_equals_the_three_launch_form(dev, ops, Kc, L):
    """spk_den_step_tail_conf == spk_den_conv3x3_counts_mfma, then spk_psample_step_conf, then the first-layer launch, bit for bit:
    tokens, ``unmasked``, x0_hat, conf_out, the logits and the next step's S32 spikes and counts -- at the first step (all masked),
    a middle step (half masked) and the last step (t = 1, no successor), Philox and injected noise."""
    from spkdiff.ops import IN_TINV
    den = _den_k(Kc, dev)
    assert den.tail_fusable(L, L)
    Bn, HW = 3, L * L
    g = torch.Generator().manual_seed(Kc * 10 + L)
    _, xh, unh, _, q = _state(Bn, Kc, L, g, dev)
    tv = torch.tensor((0.5, 1.0, 2.0), dtype=torch.float32, device=dev)
    kd = torch.tensor([0, 5, Kc // 2], dtype=torch.int32, device=dev)
    pd = torch.tensor([0.5, 1.0, 0.9], dtype=torch.float32, device=dev)
    den._trunk(ops.den_build_input(xh, 1), False)                        # (a first call derives the layers' packed weights)
    conv6, packed6 = den._conv6_params()
    conv1, bn1 = den.conv1[0], den.conv1[1]
    a1, b1 = bn1.affine_terms()
    c1 = (conv1._spk_params.get(conv1), conv1.bias.detach(), a1, b1)
    xfull = torch.where(unh, xh, (xh + 1) % 7)                           # (a valid token everywhere; the state masks it below)
    few = torch.ones_like(unh)
    few[:, :, 0, :3] = False
    cases = {"first": (xfull, torch.zeros_like(unh), 12), "middle": (xfull, unh, 5), "last": (xfull, few, 1)}
    bad = {}
    for name, (x0, un0, t) in cases.items():
        x0 = torch.where(un0, x0, torch.full_like(x0, Kc))
        _, cnt5, _, cnt1, which, _, collapse = den._trunk(ops.den_build_input(x0, t), False)
        assert which == 'mfma-fp6v2' and collapse
        nxt = c1 if t > 1 else None
        for mode, kw in {"philox": dict(seed=4242, offset=1000 * t), "injected": dict(q=q)}.items():
            x, un = x0.clone(), un0.clone()
            hat = torch.full((Bn * HW,), -5, dtype=torch.int64, device=dev)
            cf = torch.full((Bn * HW,), 7.0, device=dev)
            pre, lg = ops.den_step_tail_conf(cnt5, cnt1, packed6, x, un, t, tv, T=16, K=Kc, conv1=nxt, want_logits=True, top_k=kd,
                                             top_p=pd, x0_hat=hat, conf=cf, **kw)
            lr = ops.den_conv3x3_counts(cnt5, packed6, Kc, 16, cnt1=cnt1)
            xr, unr, hr, cr, _ = conf_call(ops, dev, lr, x0, un0, t, tv, kd, pd, **kw)
            n = int(not torch.equal(lg, lr)) + int((x != xr).sum()) + int((un != unr).sum()) + int((hat != hr).sum())
            n += int((cf.view(torch.int32) != cr.view(torch.int32)).sum())
            m = (~un0).flatten(1).sum(1)
            assert torch.equal((un & ~un0).flatten(1).sum(1), (m + t - 1) // t) and bool((m > 0).all())
            if t > 1:
                r1 = den.conv1.run(ops.den_build_input(xr, t - 1), IN_TINV, final='ptc', T=16, stateful=False,
                                   chunk_out=ops.S32.chunk, want_counts=True)
                n += int(not torch.equal(pre[0], r1['ptc'])) + int(not torch.equal(pre[1], r1['cnt']))
            else:
                assert pre is None and bool(un.all())
            # without the optional outputs: the same state
            x2, un2 = x0.clone(), un0.clone()
            ops.den_step_tail_conf(cnt5, cnt1, packed6, x2, un2, t, tv, T=16, K=Kc, conv1=None, top_k=kd, top_p=pd, **kw)
            n += int((x2 != x).sum()) + int((un2 != un).sum())
            bad[f"{name}_{mode}"] = n
    print(f"den_step_tail_conf K={Kc} {L}x{L}: {bad}")
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 4. every form
TLIST = [0.3, 1.0, 1.0, 0.65, 2.5, 0.8]
KLIST = [0, 4, 0, 0, 16, 200]
PLIST = [0.05, 0.5, 0.5, 1.0, 0.9, 0.999]


def _conf_sampler(den, graph, skip=True):
    ab = sampler(den, skip, skip, graph)          # (skip_untouched on: sample_confident takes the dense form whatever it says)
    return ab


@pytest.mark.parametrize("steps", [1, 5, 12, 49, 60])
def test_sample_confident_gives_the_same_tokens_in_every_form(dev, steps):
    den, _ = build_den(synth.MNIST, dev)
    Bn = 6
    variants = {"plain": dict(), "vectors": dict(temp=TLIST, top_k=KLIST, top_p=PLIST)}
    bad, want = {}, {}
    tail0 = den.use_step_tail
    try:
        for tail in (True, False):
            den.use_step_tail = tail
            for graph in (False, True):
                ab = _conf_sampler(den, graph)
                ab.n_samples = Bn
                for rep in range(2 if graph else 1):             # (a captured graph: a second replay of every variant)
                    for name, kw in variants.items():
                        torch.manual_seed(7100 + steps)
                        got = ab.sample_confident(steps, **kw)
                        ref = want.setdefault(name, got)          # (the first form run: fused tail, eager)
                        bad[f"{'tail' if tail else 'dense'}_{'graph' if graph else 'eager'}_{name}_{rep}"] = int((got != ref).sum())
                assert len(ab._graphs) == (1 if graph else 0), "one graph serves every temperature, k and p"
                if graph:
                    key = next(iter(ab._graphs))
                    assert "confident" in key and next(iter(ab._graphs.values())).confident
    finally:
        den.use_step_tail = tail0
    for w in want.values():
        assert w.shape == (Bn, 1, 7, 7) and int(w.max()) < K128 and int(w.min()) >= 0, "no mask_id is left"
    assert not torch.equal(want["plain"], want["vectors"])
    # another rule than the coin's: other tokens than sample() under the same key (more than one step)
    plain = sampler(den, False, False, False)
    plain.n_samples = Bn
    torch.manual_seed(7100 + steps)
    coin = plain.sample(1.0, steps)
    if steps > 1:
        assert not torch.equal(coin, want["plain"])
    else:
        assert torch.equal(coin, want["plain"]), "one step reveals everything under either rule: the same draws"
    print(f"sample_confident {steps} steps: {bad}")
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 5. a recorded run, step by step
def test_each_step_of_a_recorded_run_replays(dev, ops):
    den, _ = build_den(synth.MNIST, dev)
    Bn, steps, HW = 4, 12, 49
    ab = _conf_sampler(den, True)
    ab.n_samples = Bn
    tv = torch.tensor([0.5, 1.0, 2.0, 1.0], dtype=torch.float32, device=dev)
    kd = torch.tensor([0, 8, 0, 0], dtype=torch.int32, device=dev)
    pd = torch.tensor([1.0, 1.0, 0.9, 1.0], dtype=torch.float32, device=dev)
    rec = []
    torch.manual_seed(7200)
    out = ab.sample_confident(steps, temp=tv, top_k=kd, top_p=pd, record=rec)
    assert len(rec) == steps and torch.equal(rec[-1][1], out) and int(out.max()) < K128
    x = torch.full((Bn, 1, 7, 7), K128, dtype=torch.int64, device=dev)
    un = torch.zeros((Bn, 1, 7, 7), dtype=torch.bool, device=dev)
    total, worst, m = {}, 0.0, [HW] * Bn
    for i, (t, x_after, un_after, logits) in enumerate(rec):
        assert t == steps - i
        off = ab._step_offset(i, Bn, 7, 7, K128)
        ref = cfo.reference_rows(logits.cpu().reshape(Bn, K128, HW, 1), tv.cpu(), kd.cpu(), pd.cpu())
        xn, unn, stats, w = check_step(ops, dev, logits, x, un, t, tv, kd, pd, dict(seed=int(ab.last_key), offset=off), ref=ref)
        worst = max(worst, w)
        stats["replay_differs"] = int((xn != x_after).sum()) + int((unn != un_after).sum())
        n_new = (unn & ~un).flatten(1).sum(1).tolist()
        stats["schedule"] = sum(int(n_new[b] != cfo.n_reveal(m[b], t)) for b in range(Bn))
        m = [m[b] - n_new[b] for b in range(Bn)]
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
        x, un = x_after, un_after
    assert m == [0] * Bn
    print(f"recorded run: {total}, largest |conf - fp64| / bound {worst:.4f}")
    assert all(v == 0 for v in total.values()), total
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------- 6. greedy decoding
def test_greedy_decoding_does_not_depend_on_the_key(dev):
    den, _ = build_den(synth.MNIST, dev)
    ab = _conf_sampler(den, True)
    ab.n_samples = 4
    torch.manual_seed(1)
    a = ab.sample_confident(8, top_k=1)
    ka = ab.last_key
    torch.manual_seed(2)
    b = ab.sample_confident(8, top_k=1)
    assert ka != ab.last_key and torch.equal(a, b) and int(a.max()) < K128
    torch.manual_seed(2)
    assert not torch.equal(ab.sample_confident(8), b)


# ------------------------------------------------------------------------------------------------- 7. shards
def test_sample_confident_on_two_shards_equals_the_whole_job(dev):
    den, _ = build_den(synth.MNIST, dev)
    Bn, steps = 6, 8
    whole = _conf_sampler(den, True)
    whole.n_samples = Bn
    torch.manual_seed(31)
    want = whole.sample_confident(steps, temp=TLIST, top_k=KLIST, top_p=PLIST)
    bad = {}
    # (the second split has a shard of ONE image: its per-image arrays have one entry, which no wrapper may read back -- inside a
    #  capture that is refused, and the sampler would fall back to eager launches with a warning)
    for name, split in (("2+4", ((0, 2), (2, 6))), ("1+5", ((0, 1), (1, 6)))):
        for graph in (False, True):
            parts = []
            for lo, hi in split:
                sh = _conf_sampler(den, graph).set_shard(lo, hi - lo)
                torch.manual_seed(31)
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    parts.append(sh.sample_confident(steps, temp=TLIST[lo:hi], top_k=KLIST[lo:hi], top_p=PLIST[lo:hi]))
                assert not [str(w.message) for w in seen if "spkdiff" in str(w.message)], "no capture fall-back"
                assert sh.use_graph == graph and len(sh._graphs) == (1 if graph else 0), "captured stays captured, one live graph"
            bad[f"{name}_{'graph' if graph else 'eager'}"] = int((torch.cat(parts) != want).sum())
    # a batch of one with scalar arguments, captured: the same image as the job's first under the same key
    one = _conf_sampler(den, True)
    one.n_samples = 1
    torch.manual_seed(31)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = one.sample_confident(steps, temp=TLIST[0], top_p=PLIST[0])
    assert not [str(w.message) for w in seen if "spkdiff" in str(w.message)] and one.use_graph and len(one._graphs) == 1
    bad["one_image_scalars"] = int((got != want[:1]).sum())
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 8. completion
def test_complete_images_confident(dev, ops):
    from spkdiff.complete import complete_images_confident
    from spkdiff.dist import complete_images_sharded
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    Bn, steps = 6, 4
    images = (synth.stroke_images(Bn, seed=77, img=28, channels=1) - 0.5).to(dev)
    keep = torch.ones(Bn, 28, 28, dtype=torch.bool)
    keep[:, 14:] = False
    keep[1::2, :, 10:17] = False
    keep = keep.to(dev)
    ab = _conf_sampler(den, True)
    torch.manual_seed(2026)
    res = complete_images_confident(model, ab, images, keep, sample_steps=steps, temp=0.9, top_p=0.95)
    codes = model.encode_images(images)
    assert 0 < int(res.known.sum()) < res.known.numel()
    assert int((res.tokens[res.known] != codes[res.known]).sum()) == 0, "known tokens come back unchanged"
    assert int(res.tokens.max()) < K128 and int(res.tokens.min()) >= 0
    # the paste, as in complete_images: the given pixels are the input's, the rest the decoder's
    torch.manual_seed(2026)
    raw = complete_images_confident(model, ab, images, keep, sample_steps=steps, temp=0.9, top_p=0.95, paste=False)
    assert torch.equal(raw.tokens, res.tokens)
    assert torch.equal(ops.completion_compose(images, keep, raw.images_u8), res.images_u8)
    # nothing known: sample_confident under the same key
    none = torch.zeros_like(keep)
    torch.manual_seed(2027)
    free = complete_images_confident(model, ab, images, none, sample_steps=steps, temp=0.9, top_k=20)
    assert int(free.known.sum()) == 0
    ab.n_samples = Bn
    torch.manual_seed(2027)
    assert torch.equal(ab.sample_confident(steps, temp=0.9, top_k=20).reshape(Bn, 7, 7), free.tokens)
    # the sharded wrapper hands the flag on; its default is the coin's call
    torch.manual_seed(2026)
    sh = complete_images_sharded(model, ab, images, keep, temp=0.9, sample_steps=steps, top_p=0.95, confident=True)
    assert torch.equal(sh, res.images_u8)


# ------------------------------------------------------------------------------------------------- 9. what the wrappers refuse
def test_wrappers_refuse_bad_arguments_before_launching(dev, ops):
    Bn, h = 5, 7
    g = torch.Generator().manual_seed(1)
    logits, x0, un0, _, _ = _state(Bn, K128, h, g, dev)
    good_p = torch.full((Bn,), 0.5, device=dev)
    good_k = torch.full((Bn,), 4, dtype=torch.int32, device=dev)
    calls = [dict(temp=0.0), dict(temp=-1.0), dict(temp=float("nan")), dict(temp=torch.ones(4, device=dev)),
             dict(temp=torch.ones(Bn, dtype=torch.float64, device=dev)),
             dict(top_k=4), dict(top_k=torch.ones(Bn, device=dev)), dict(top_k=good_k[:4]), dict(top_k=good_k.cpu()),
             dict(top_p=0.5), dict(top_p=good_p[:4]), dict(top_p=good_p.double()), dict(top_p=good_p.cpu()),
             dict(conf=torch.zeros(Bn * h * h, dtype=torch.float64, device=dev)), dict(x0_hat=torch.zeros(3, dtype=torch.int64, device=dev))]
    for kw in calls:
        x, un = x0.clone(), un0.clone()
        with pytest.raises(ValueError):
            ops.psample_step_conf(logits, x, un, 2, **dict(dict(temp=1.0), **kw))
        torch.cuda.synchronize()
        assert torch.equal(x, x0) and torch.equal(un, un0), f"a refused call launched nothing: {kw}"
    # inside an active_set scope: no active-list form
    x, un = x0.clone(), un0.clone()
    den = _den_k(K128, dev)
    _, cnt5, _, cnt1, _, _, _ = den._trunk(ops.den_build_input(x0, 2), False)
    with ops.active_set(*_active(Bn, dev)):
        with pytest.raises(ValueError, match="active"):
            ops.psample_step_conf(logits, x, un, 2, 1.0, top_k=good_k, top_p=good_p)
        with pytest.raises(ValueError, match="active"):
            ops.den_step_tail_conf(cnt5, cnt1, den._conv6_params()[1], x, un, 2, 1.0, T=16, K=K128)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(un, un0)
    # scalars are broadcast: the call equals the one with the three vectors
    a, b = x0.clone(), x0.clone()
    ops.psample_step_conf(logits, a, un0.clone(), 2, 0.7, seed=3)
    ops.psample_step_conf(logits, b, un0.clone(), 2, torch.full((Bn,), 0.7, device=dev), seed=3, top_p=torch.ones(Bn, device=dev),
                          top_k=torch.zeros(Bn, dtype=torch.int32, device=dev))
    assert torch.equal(a, b)
    # the sampler: checked before a key is drawn or a graph captured
    build, _ = build_den(synth.MNIST, dev)
    ab = _conf_sampler(build, True)
    ab.n_samples = Bn
    torch.manual_seed(5)
    state = torch.get_rng_state()
    for kw in (dict(temp=0.0), dict(temp=[1.0] * 4), dict(temp=[1.0, -1.0, 1.0, 1.0, 1.0]), dict(top_k=0), dict(top_k=[1] * 4),
               dict(top_k=1.5), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=[0.5] * 4), dict(top_p=torch.ones(Bn, 1, device=dev))):
        with pytest.raises(ValueError):
            ab.sample_confident(3, **kw)
    big = sampler(build, True, True, True, latent=9)
    with pytest.raises(NotImplementedError):
        big.sample_confident(3)
    assert torch.equal(torch.get_rng_state(), state) and len(ab._graphs) == 0 and len(big._graphs) == 0
