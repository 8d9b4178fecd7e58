"""GPU tests of reveal schedules and annealed selection noise for confidence-ordered decoding (run with ``-m gpu`` on an MI355X;
DESIGN.md §4.17): the three ``_sched`` entry points against their ``_conf`` siblings bit for bit (linear table, no noise; the
candidates and confidences under any table), the counts against the host integers, the commit against a literal sort of the kernel's
own scores, the scores against fp64 within the counted bound of tests/_confident_sched_oracle.py, injected uniforms that decide the
order, ``AbsorbingDiffusion.sample_confident(schedule=, selection_noise=)`` in every form, and the one property the feature exists
for: greedy decoding of the trained denoiser depends on the key exactly when the selection noise is on."""
import math
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _confident_oracle as cfo             # noqa: E402
import _confident_sched_oracle as cso       # noqa: E402
import _confident_steps_oracle as cst       # noqa: E402
from spkdiff import schedules as sch        # noqa: E402
from spkdiff import synth                   # noqa: E402
from test_gpu_completion import K as K128, build_den, build_vae, sampler      # noqa: E402  (the helpers, not the tests)
from test_gpu_confident import conf_call    # noqa: E402
from test_gpu_temps import _den_k, _state   # noqa: E402

SIGMA = cst.STEP_STRIDE
KS = (2, 65, 128, 512, 2048)
S_TABLE = 100                                # the loop length of the kernel cases: t = 100 is one of the table's steps


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def sched_call(ops, dev, logits, x0, un0, t, temp, top_k, top_p, w, a, S, nxt=False, **noise):
    """One scheduled update on copies of the state -> (x_t, unmasked, x0_hat, conf, score, next_input or None); the three outputs are
    pre-filled with sentinels the kernel must leave where a position is not masked."""
    n = x0.numel()
    x, un = x0.clone(), un0.clone()
    hat = torch.full((n,), -5, dtype=torch.int64, device=dev)
    conf = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    score = torch.full((n,), 9.0, dtype=torch.float32, device=dev)
    ni = torch.full((x0.shape[0], 2) + tuple(logits.shape[2:]), float("nan"), device=dev) if nxt else None
    ops.psample_step_conf_sched(logits, x, un, t, temp, w, S, a, x0_hat=hat, conf=conf, score=score, next_input=ni, top_k=top_k,
                                top_p=top_p, **noise)
    return x, un, hat, conf, score, ni


def _bits(v):
    return v.view(torch.int32) if v.dtype == torch.float32 else v


def _differ(a, b):
    return sum(int((_bits(u) != _bits(v)).sum()) for u, v in zip(a, b) if u is not None)


def _tables(S, dev, B=cfo.B):
    w = torch.tensor(cso.table_rows(S, B), dtype=torch.int32)
    lin = torch.tensor([cso.linear_weights(S)] * B, dtype=torch.int32)
    cos = torch.tensor([cso.cosine_weights(S)] * B, dtype=torch.int32)
    # per image: no noise, a small scale, MaskGIT's 4.5 annealed over the S steps, a large scale, a negative one (legal at this level)
    taus = (0.0, 0.5, 4.5, 300.0, -2.0)
    a = torch.tensor([cso.noise_row(taus[b % 5], S, S) for b in range(B)], dtype=torch.float32)
    return w, lin, cos, a


# ------------------------------------------------------------------------------------------------- 1. the sampling kernel
@pytest.mark.parametrize("HW", cfo.HWS)
@pytest.mark.parametrize("K", KS)
def test_psample_step_conf_sched_vs_sibling_and_oracle(dev, ops, K, HW):
    """The case table of tests/_confident_oracle.conf_inputs (B = 5, m = 0, 1, 2, HW - 1, HW, per-image temperature / k / p), t in {1, 2,
    m, m + 1, 100} inside a loop of S = 100.  IDENTITY: the linear table with a null and with an all-zero noise table gives x_t,
    unmasked, x0_hat, conf and next_input bit-equal to spk_psample_step_conf; under the cosine and the per-image custom tables with
    tau > 0 the candidates and conf_out are still the sibling's.  COUNTS: the number revealed per image equals the host integers.
    ORDER: the committed state is the literal sort applied to the kernel's own score_out (no case excluded), score_out equals conf_out
    where a = 0 and lies within the counted bound of conf64 + a * g64 elsewhere (the uniforms: spk_philox_noise's, or the injected
    ones), and nothing is written where a position is not masked."""
    logits, q, x0, un0, temps, ks, ps = cfo.conf_inputs(K, HW)
    ref = cfo.reference_rows(logits, temps, ks, ps)
    z32, zt, fcut, on = ref
    ld, x0d, un0d, tv, kd, pd = (v.to(dev) for v in (logits, x0, un0, temps, ks, ps))
    Bn, S = cfo.B, S_TABLE
    w_mix, w_lin, w_cos, a_tab = _tables(S, dev)
    zero_a = torch.zeros_like(a_tab).to(dev)
    seed, off = 0x1234_5678_9ABC, 5 * SIGMA + 11 * HW * K
    state = torch.tensor([seed, 1 << 33], dtype=torch.int64, device=dev)
    gi = torch.Generator().manual_seed(K * 7 + HW)
    u_inj = torch.rand(Bn * HW, generator=gi).clamp_(min=2.0 ** -24)
    noises = {"philox": dict(seed=seed, offset=off), "philox_state": dict(seed=99, offset=off - (1 << 33), philox_state=state),
              "injected": dict(q=q.to(dev), u=u_inj.to(dev))}
    masked = ~un0.flatten()
    xh, unh = x0.reshape(Bn, HW), un0.reshape(Bn, HW).bool()
    total, worst = {}, 0.0

    def add(k, v):
        total[k] = total.get(k, 0) + int(v)

    for t in (tt for tt in cfo.steps_of(HW) if tt <= S):
        for mode, kw in noises.items():
            sib = conf_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, nxt=True, **{k: v for k, v in kw.items() if k != "u"})
            # identity: linear table, null / all-zero noise
            for name, a in (("null", None), ("zero", zero_a)):
                got = sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, w_lin.to(dev), a, S, nxt=True, **kw)
                add(f"identity_{name}", _differ((got[0], got[1], got[2], got[3], got[5]), sib))
                add(f"identity_{name}_score_is_conf", _differ((got[4],), (torch.where(un0d.flatten(), torch.full_like(got[4], 9.0), got[3]),)))
            # any table, tau > 0: the sibling's candidates and confidences; the commit and the counts from the kernel's own scores
            for name, w in (("cosine", w_cos), ("custom", w_mix)):
                x, un, hat, conf, score, ni = sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, w.to(dev), a_tab.to(dev), S, nxt=True, **kw)
                add(f"{name}_cand_or_conf_differs", _differ((hat, conf), (sib[2], sib[3])))
                sc = score.cpu()
                add(f"{name}_touched_unmasked", (sc[~masked] != 9.0).sum())
                wp, wc = w[:, t - 1].tolist(), w[:, t].tolist()
                wx, wun, rev, counts = cso.commit_state(xh, unh, hat.cpu().reshape(Bn, HW), sc.reshape(Bn, HW), wp, wc)
                add(f"{name}_state_differs", (x.cpu().reshape(Bn, HW) != wx).sum() + (un.cpu().reshape(Bn, HW).bool() != wun).sum())
                got_n = (un.cpu().reshape(Bn, HW).bool() & ~unh).sum(1).tolist()
                add(f"{name}_count_differs", sum(int(got_n[b] != cso.reveal_count(int((~unh[b]).sum()), wp[b], wc[b])) for b in range(Bn)))
                # (the rank mirror agrees with the sort on the kernel's scores)
                rx, run, _, _ = cso.commit_state(xh, unh, hat.cpu().reshape(Bn, HW), sc.reshape(Bn, HW), wp, wc, commit=cso.commit_by_rank)
                add(f"{name}_mirror_differs", (rx != wx).sum() + (run != wun).sum())
                add(f"{name}_next_input", not torch.equal(ni, ops.den_build_input(x, t - 1)))
                # the scores against fp64
                a_pos = a_tab[:, t].repeat_interleave(HW)
                add(f"{name}_score_not_conf_at_a0", (_bits(sc)[masked & (a_pos == 0)] != _bits(conf.cpu())[masked & (a_pos == 0)]).sum())
                u_used = u_inj if mode == "injected" else _philox_u(ops, dev, seed, off, Bn, HW, K)
                sel = masked & ~fcut & ~torch.isnan(z32).any(-1) & torch.isfinite(zt).any(-1) & (u_used > 0)
                c64 = cfo.log_prob_f64(zt[sel], hat.cpu()[sel]).numpy()
                want = cso.score_f64(c64, a_pos[sel].double().numpy(), u_used[sel].double().numpy())
                bound = cso.score_bound(K, zt[sel].max(-1).values.numpy(), c64, a_pos[sel].double().numpy(), u_used[sel].double().numpy())
                err = np.abs(sc[sel].double().numpy() - want)
                if err.size:
                    worst = max(worst, float((err / bound).max()))
                add(f"{name}_score_outside_bound", (err > bound).sum())
    print(f"conf_sched K={K} HW={HW}: {total}, largest |score - fp64| / bound {worst:.4f}")
    assert all(v == 0 for v in total.values()), total
    assert worst <= 1.0


_U = {}


def _philox_u(ops, dev, seed, off, Bn, HW, K):
    """The stream-0 uniforms of a step as spk_philox_noise writes them (host copy, computed once per case)."""
    key = (seed, off, Bn, HW, K)
    if key not in _U:
        _U.clear()
        _U[key] = ops.philox_noise(seed, off, Bn, HW, K, dev, want_q=False)[0].cpu()
    return _U[key]


# ------------------------------------------------------------------------------------------------- 2. injected uniforms decide
@pytest.mark.parametrize("HW", [49, 64])
def test_well_separated_uniforms_and_a_large_scale_decide_the_order(dev, ops, HW):
    """a = 2^20 and injected u on the grid (k + 1) / (HW + 2), permuted per image: the revealed set is exactly the n positions with
    the largest u.  The margin: g(u) = -ln(-ln u) has g' = 1 / (u (-ln u)) >= e on (0, 1), so two grid points differ by at least
    e / (HW + 2) in g and by a * e / (HW + 2) in a * g; a confidence lies in [-(range of the scaled row + ln K), 0], and the two
    fp32 roundings of a score of magnitude below 2^25 move it by at most 2 * 2 each."""
    K, Bn, S, t = 128, cfo.B, 8, 5
    logits, q, x0, un0, temps, ks, ps = cfo.conf_inputs(K, HW)
    z32 = cfo.reference_rows(logits, temps, ks, ps)[0]
    conf_abs = float((z32.max(-1).values - z32.min(-1).values).max()) + math.log(K)
    a_val = float(1 << 20)
    gap = a_val * math.e / (HW + 2)
    margin = gap - 2 * conf_abs - 8.0
    assert a_val * 17.0 < 2.0 ** 25 and margin > 1000.0, (gap, conf_abs)
    g = torch.Generator().manual_seed(HW)
    grid = (torch.arange(HW, dtype=torch.float64) + 1) / (HW + 2)
    u = torch.stack([grid[torch.randperm(HW, generator=g)] for _ in range(Bn)]).to(torch.float32)
    w = torch.tensor([cso.cosine_weights(S)] * Bn, dtype=torch.int32, device=dev)
    a = torch.zeros(Bn, S + 1)
    a[:, t] = a_val
    ld, x0d, un0d, tv, kd, pd = (v.to(dev) for v in (logits, x0, un0, temps, ks, ps))
    x, un, hat, conf, score, _ = sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, w, a.to(dev), S, q=q.to(dev), u=u.flatten().to(dev))
    unh, got = un0.reshape(Bn, HW).bool(), un.cpu().reshape(Bn, HW).bool()
    for b in range(Bn):
        m = int((~unh[b]).sum())
        n = cso.reveal_count(m, cso.cosine_weights(S)[t - 1], cso.cosine_weights(S)[t])
        pos = (~unh[b]).nonzero().flatten()
        want = set(pos[u[b][pos].argsort(descending=True)[:n]].tolist())
        assert set((got[b] & ~unh[b]).nonzero().flatten().tolist()) == want, b
    assert float(conf.cpu()[~un0.flatten()].abs().max()) <= conf_abs, "the stated bound of |conf| holds on the kernel's own values"


# ------------------------------------------------------------------------------------------------- 3. the listed form
def listed_sched_call(ops, dev, logits, x0, un0, t, temp, top_k, top_p, steps, S, lst, w, a, **noise):
    Bn, n = x0.shape[0], x0.numel()
    slots = torch.full_like(logits, float("nan"))
    slots[:len(lst)] = logits[torch.tensor(lst, dtype=torch.int64, device=dev)]
    act = torch.full((Bn,), -1, dtype=torch.int32, device=dev)
    act[:len(lst)] = torch.tensor(lst, dtype=torch.int32, device=dev)
    nact = torch.tensor([len(lst), 0], dtype=torch.int32, device=dev)
    x, un = x0.clone(), un0.clone()
    hat = torch.full((n,), -5, dtype=torch.int64, device=dev)
    conf = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    score = torch.full((n,), 9.0, dtype=torch.float32, device=dev)
    with ops.active_set(act, nact):
        if w is None:
            ops.psample_step_conf_listed(slots, x, un, t, temp, steps, S, SIGMA, x0_hat=hat, conf=conf, top_k=top_k, top_p=top_p, **noise)
        else:
            ops.psample_step_conf_listed_sched(slots, x, un, t, temp, steps, S, SIGMA, w, a, x0_hat=hat, conf=conf, score=score,
                                               top_k=top_k, top_p=top_p, **noise)
    return x, un, hat, conf, score


@pytest.mark.parametrize("HW", cfo.HWS)
@pytest.mark.parametrize("K", KS)
def test_listed_sched_equals_the_dense_sched_and_the_listed_sibling(dev, ops, K, HW):
    """Full list with all counts equal to S: state, x0_hat, conf and score are spk_psample_step_conf_sched's bit for bit.  The linear
    table without noise: spk_psample_step_conf_listed's.  A sub-list in another order: listed images as the dense call, the others
    untouched.  An image with e < S reads its own row at the loop's t and draws race noise AND Gumbel uniform at offset - (S - e) *
    sigma: it equals the dense call made there."""
    logits, q, x0, un0, temps, ks, ps = cfo.conf_inputs(K, HW)
    ld, x0d, un0d, tv, kd, pd = (v.to(dev) for v in (logits, x0, un0, temps, ks, ps))
    Bn, S, t, e = cfo.B, 6, 2, 3
    w = torch.tensor(cso.table_rows(S), dtype=torch.int32, device=dev)
    a = torch.tensor([cso.noise_row((0.0, 0.5, 4.5, 300.0, 2.0)[b], S, S) for b in range(Bn)], dtype=torch.float32, device=dev)
    lin = torch.tensor([cso.linear_weights(S)] * Bn, dtype=torch.int32, device=dev)
    seed, off = 0x1234_5678_9ABC, 5 * SIGMA + 11 * HW * K
    state = torch.tensor([seed, 1 << 33], dtype=torch.int64, device=dev)
    noises = {"philox": dict(seed=seed, offset=off), "philox_state": dict(seed=99, offset=off - (1 << 33), philox_state=state),
              "injected": dict(q=q.to(dev), u=torch.rand(Bn * HW, generator=torch.Generator().manual_seed(K + HW)).to(dev))}
    full = torch.full((Bn,), S, dtype=torch.int32, device=dev)
    mixed = torch.tensor([S, S, S + 7, e, e], dtype=torch.int32, device=dev)
    every = list(range(Bn))
    bad = {}

    def rows(a_, b_, which):
        n = 0
        for u_, v_ in zip(a_, b_):
            n += int((_bits(u_).reshape(Bn, HW)[which] != _bits(v_).reshape(Bn, HW)[which]).sum())
        return n

    for mode, kw in noises.items():
        for tt in (t, S, 1):
            dense = sched_call(ops, dev, ld, x0d, un0d, tt, tv, kd, pd, w, a, S, **kw)[:5]
            got = listed_sched_call(ops, dev, ld, x0d, un0d, tt, tv, kd, pd, full, S, every, w, a, **kw)
            bad[f"{mode}_full_t{tt}"] = rows(got, dense, every)
        dense = sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, w, a, S, **kw)[:5]
        noq = {k: v for k, v in kw.items() if k != "u"}
        sib = listed_sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, full, S, every, None, None, **noq)
        for name, aa in (("null", None), ("zero", torch.zeros_like(a))):
            got = listed_sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, full, S, every, lin, aa, **kw)
            bad[f"{mode}_identity_{name}"] = rows(got[:4], sib[:4], every)
        sub = listed_sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, full, S, [4, 0, 2], w, a, **kw)
        bad[f"{mode}_sub_listed"] = rows(sub, dense, [0, 2, 4])
        untouched = (x0d, un0d, torch.full_like(sub[2], -5), torch.full_like(sub[3], 7.0), torch.full_like(sub[4], 9.0))
        bad[f"{mode}_sub_unlisted"] = rows(sub, untouched, [1, 3])
        mix = listed_sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, mixed, S, every, w, a, **kw)
        bad[f"{mode}_above_S_is_S"] = rows(mix, dense, [0, 1, 2])
        if mode == "injected":
            bad[f"{mode}_noise_as_given"] = rows(mix, dense, [3, 4])
            continue
        shifted = dict(kw, offset=kw["offset"] - (S - e) * SIGMA)
        bad[f"{mode}_shifted"] = rows(mix, sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, w, a, S, **shifted)[:5], [3, 4])
        if HW >= 49:
            assert rows(mix[4:], dense[4:], [3, 4]) > 0, "an image with e < S draws its Gumbel uniform at other counters than the loop's"
    print(f"conf_listed_sched K={K} HW={HW}: {bad}")
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 4. the fused step tail
@pytest.mark.parametrize("L", [7, 8])
@pytest.mark.parametrize("Kc", [100, 128, 256, 512])
def test_den_step_tail_conf_sched_equals_the_three_launch_form(dev, ops, Kc, L):
    """spk_den_step_tail_conf_sched == spk_den_conv3x3_counts_mfma, then spk_psample_step_conf_sched, then the first-layer launch, bit
    for bit: tokens, ``unmasked``, x0_hat, conf, score, the logits and the next step's S32 spikes and counts -- first, middle and last
    step, Philox and injected noise; and with the linear table and no noise it is spk_den_step_tail_conf."""
    from spkdiff.ops import IN_TINV
    den = _den_k(Kc, dev)
    assert den.tail_fusable(L, L)
    Bn, HW, S = 3, L * L, 12
    g = torch.Generator().manual_seed(Kc * 10 + L)
    _, xh, unh, u, q = _state(Bn, Kc, L, g, dev)
    tv = torch.tensor((0.5, 1.0, 2.0), dtype=torch.float32, device=dev)
    kd = torch.tensor([0, 5, Kc // 2], dtype=torch.int32, device=dev)
    pd = torch.tensor([0.5, 1.0, 0.9], dtype=torch.float32, device=dev)
    rows = cso.table_rows(S, 5)
    w = torch.tensor([rows[1], rows[2], rows[3]], dtype=torch.int32, device=dev)          # cosine, a zero weight, a non-monotone pair
    a = torch.tensor([cso.noise_row(tau, S, S) for tau in (4.5, 0.0, 50.0)], dtype=torch.float32, device=dev)
    lin = torch.tensor([cso.linear_weights(S)] * Bn, dtype=torch.int32, device=dev)
    den._trunk(ops.den_build_input(xh, 1), False)                        # (a first call derives the layers' packed weights)
    conv6, packed6 = den._conv6_params()
    conv1, bn1 = den.conv1[0], den.conv1[1]
    a1, b1 = bn1.affine_terms()
    c1 = (conv1._spk_params.get(conv1), conv1.bias.detach(), a1, b1)
    xfull = torch.where(unh, xh, (xh + 1) % 7)
    few = torch.ones_like(unh)
    few[:, :, 0, :3] = False
    cases = {"first": (xfull, torch.zeros_like(unh), 12), "middle": (xfull, unh, 5), "last": (xfull, few, 1)}
    bad = {}
    for name, (x0, un0, t) in cases.items():
        x0 = torch.where(un0, x0, torch.full_like(x0, Kc))
        _, cnt5, _, cnt1, which, _, collapse = den._trunk(ops.den_build_input(x0, t), False)
        assert which == 'mfma-fp6v2' and collapse
        nxt = c1 if t > 1 else None
        for mode, kw in {"philox": dict(seed=4242, offset=1000 * t), "injected": dict(q=q, u=u)}.items():
            x, un = x0.clone(), un0.clone()
            hat = torch.full((Bn * HW,), -5, dtype=torch.int64, device=dev)
            cf = torch.full((Bn * HW,), 7.0, device=dev)
            sc = torch.full((Bn * HW,), 9.0, device=dev)
            pre, lg = ops.den_step_tail_conf_sched(cnt5, cnt1, packed6, x, un, t, tv, w, S, T=16, K=Kc, noise_a=a, conv1=nxt,
                                                   want_logits=True, top_k=kd, top_p=pd, x0_hat=hat, conf=cf, score=sc, **kw)
            lr = ops.den_conv3x3_counts(cnt5, packed6, Kc, 16, cnt1=cnt1)
            xr, unr, hr, cr, sr, _ = sched_call(ops, dev, lr, x0, un0, t, tv, kd, pd, w, a, S, **kw)
            n = int(not torch.equal(lg, lr)) + _differ((x, un, hat, cf, sc), (xr, unr, hr, cr, sr))
            m = (~un0).flatten(1).sum(1).tolist()
            wl = w.cpu()
            want_n = [cso.reveal_count(m[b], int(wl[b, t - 1]), int(wl[b, t])) for b in range(Bn)]
            assert (un & ~un0).flatten(1).sum(1).tolist() == want_n and min(m) > 0
            if t > 1:
                r1 = den.conv1.run(ops.den_build_input(xr, t - 1), IN_TINV, final='ptc', T=16, stateful=False,
                                   chunk_out=ops.S32.chunk, want_counts=True)
                n += int(not torch.equal(pre[0], r1['ptc'])) + int(not torch.equal(pre[1], r1['cnt']))
            else:
                assert pre is None
            # without the optional outputs: the same state
            x2, un2 = x0.clone(), un0.clone()
            ops.den_step_tail_conf_sched(cnt5, cnt1, packed6, x2, un2, t, tv, w, S, T=16, K=Kc, noise_a=a, top_k=kd, top_p=pd, **kw)
            n += int((x2 != x).sum()) + int((un2 != un).sum())
            bad[f"{name}_{mode}"] = n
            # identity: the linear table, null and all-zero noise == spk_den_step_tail_conf
            xs, uns = x0.clone(), un0.clone()
            hs, cs = torch.full_like(hat, -5), torch.full_like(cf, 7.0)
            noq = {k: v for k, v in kw.items() if k != "u"}
            ps_, ls = ops.den_step_tail_conf(cnt5, cnt1, packed6, xs, uns, t, tv, T=16, K=Kc, conv1=nxt, want_logits=True, top_k=kd,
                                            top_p=pd, x0_hat=hs, conf=cs, **noq)
            for iname, aa in (("null", None), ("zero", torch.zeros_like(a))):
                xi, uni = x0.clone(), un0.clone()
                hi, ci = torch.full_like(hat, -5), torch.full_like(cf, 7.0)
                pi, li = ops.den_step_tail_conf_sched(cnt5, cnt1, packed6, xi, uni, t, tv, lin, S, T=16, K=Kc, noise_a=aa, conv1=nxt,
                                                      want_logits=True, top_k=kd, top_p=pd, x0_hat=hi, conf=ci, **kw)
                k = _differ((xi, uni, hi, ci, li), (xs, uns, hs, cs, ls))
                if t > 1:
                    k += int(not torch.equal(pi[0], ps_[0])) + int(not torch.equal(pi[1], ps_[1]))
                bad[f"{name}_{mode}_identity_{iname}"] = k
    print(f"den_step_tail_conf_sched K={Kc} {L}x{L}: {bad}")
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 5. the sampler, every form
TAB12 = [0, 1, 1, 4, 4, 9, 9, 9, 30, 25, 40, 60, 61]        # 12 steps: repeats (forced 1) and a non-monotone pair
TAUS6 = [0.0, 4.5, 1.0, 0.0, 9.0, 2.5]
SCHED6 = ["cosine", None, "linear", TAB12, "cosine", TAB12]


def _variants(steps):
    v = {"linear": dict(schedule="linear"), "cosine": dict(schedule="cosine"), "cosine_noisy": dict(schedule="cosine", selection_noise=4.5),
         "noisy": dict(selection_noise=4.5)}
    if steps == 12:
        v["per_image"] = dict(schedule=SCHED6, selection_noise=TAUS6, temp=[0.3, 1.0, 1.0, 0.65, 2.5, 0.8], top_k=[0, 4, 0, 0, 16, 200],
                              top_p=[0.05, 0.5, 0.5, 1.0, 0.9, 0.999])
    return v


@pytest.mark.parametrize("steps", [5, 12])
def test_sample_confident_sched_gives_the_same_tokens_in_every_form(dev, steps):
    """Fused tail == three launches, eager == captured, ONE captured graph replayed with linear, cosine and noisy tables == the eager
    runs of each; the linear table without noise == sample_confident() without arguments; a recorded run commits the host's counts."""
    den, _ = build_den(synth.MNIST, dev)
    Bn = 6
    variants = _variants(steps)
    bad, want = {}, {}
    tail0 = den.use_step_tail
    try:
        for tail in (True, False):
            den.use_step_tail = tail
            for graph in (False, True):
                ab = sampler(den, True, True, graph)
                ab.n_samples = Bn
                for rep in range(2 if graph else 1):
                    for name, kw in variants.items():
                        torch.manual_seed(7300 + steps)
                        got = ab.sample_confident(steps, **kw)
                        ref = want.setdefault(name, got)
                        bad[f"{'tail' if tail else 'dense'}_{'graph' if graph else 'eager'}_{name}_{rep}"] = int((got != ref).sum())
                assert len(ab._graphs) == (1 if graph else 0), "one graph serves every schedule and every noise scale"
                if graph:
                    key, g = next(iter(ab._graphs.items()))
                    assert "scheduled" in key and "confident" in key and g.sched is not None and tuple(g.sched[0].shape) == (Bn, steps + 1)
                    with warnings.catch_warnings(record=True) as seen:
                        warnings.simplefilter("always")
                        torch.manual_seed(7300 + steps)
                        plain = ab.sample_confident(steps)
                    assert not [str(w.message) for w in seen if "spkdiff" in str(w.message)]
                    assert len(ab._graphs) == 2 and sum("scheduled" in k for k in ab._graphs) == 1, "the default call keeps its own graph"
                    bad[f"{'tail' if tail else 'dense'}_linear_is_the_default"] = int((plain != want["linear"]).sum())
    finally:
        den.use_step_tail = tail0
    for w in want.values():
        assert w.shape == (Bn, 1, 7, 7) and int(w.max()) < K128 and int(w.min()) >= 0, "no mask_id is left"
    assert not torch.equal(want["linear"], want["cosine"]) and not torch.equal(want["cosine"], want["cosine_noisy"])
    assert not torch.equal(want["linear"], want["noisy"])
    # the counts of a recorded run: the host integers
    ab = sampler(den, True, True, False)
    ab.n_samples = Bn
    for name, w in (("cosine", sch.cosine_weights(steps)), ("linear", sch.linear_weights(steps))):
        rec = []
        torch.manual_seed(7300 + steps)
        out = ab.sample_confident(steps, schedule=name, selection_noise=2.0, record=rec)
        left = torch.full((Bn,), 49)
        counts = []
        for _, _, un_after, _ in rec:
            now = (~un_after).flatten(1).sum(1).cpu()
            counts.append((left - now).tolist())
            left = now
        assert counts == [[n] * Bn for n in sch.reveal_counts(49, w)] and int(left.sum()) == 0, (name, counts)
    print(f"sample_confident sched {steps} steps: {bad}")
    assert all(v == 0 for v in bad.values()), bad


def test_a_batch_split_in_one_two_and_four_parts_gives_the_same_tokens(dev):
    den, _ = build_den(synth.MNIST, dev)
    Bn, steps = 8, 12
    scheds = (SCHED6 + ["cosine", TAB12])[:Bn]
    taus = (TAUS6 + [4.5, 0.5])[:Bn]
    temps = [0.3, 1.0, 1.0, 0.65, 2.5, 0.8, 1.0, 0.5]
    bad, want = {}, None
    for parts in (1, 2, 4):
        n = Bn // parts
        for graph in (False, True):
            out = []
            for i in range(parts):
                lo, hi = i * n, (i + 1) * n
                sh = sampler(den, True, True, graph).set_shard(lo, n)
                torch.manual_seed(41)
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    out.append(sh.sample_confident(steps, temp=temps[lo:hi], schedule=scheds[lo:hi], selection_noise=taus[lo:hi]))
                assert not [str(w.message) for w in seen if "spkdiff" in str(w.message)], "no capture fall-back"
            got = torch.cat(out)
            want = got if want is None else want
            bad[f"{parts}_{'graph' if graph else 'eager'}"] = int((got != want).sum())
    assert all(v == 0 for v in bad.values()), bad


def test_image_i_of_a_mixed_run_equals_its_own_run(dev):
    """Per-image steps, schedules and noise scales: image i equals image i of sample_confident(e_i, schedule=row_i,
    selection_noise=tau_i) at the same global index under the same key, bit for bit -- eager and captured."""
    den, _ = build_den(synth.MNIST, dev)
    steps = [1, 3, 8, 12, 5, 12]
    Bn = len(steps)
    rows = ["cosine", "cosine", None, TAB12, [0, 2, 2, 7, 3, 11], "cosine"]
    bad = {}
    solo = []
    for i, e in enumerate(steps):
        one = sampler(den, True, True, False).set_shard(i, 1)
        torch.manual_seed(55)
        solo.append(one.sample_confident(e, schedule=rows[i], selection_noise=TAUS6[i], temp=0.9, top_k=30))
    want = torch.cat(solo)
    for graph in (False, True):
        ab = sampler(den, True, True, graph)
        ab.n_samples = Bn
        for rep in range(2 if graph else 1):
            torch.manual_seed(55)
            got = ab.sample_confident(steps, schedule=rows, selection_noise=TAUS6, temp=0.9, top_k=30)
            bad[f"{'graph' if graph else 'eager'}_{rep}"] = (got != want).flatten(1).sum(1).tolist()
        if graph:
            key = next(iter(ab._graphs))
            assert len(ab._graphs) == 1 and "scheduled" in key and "per-image-steps" in key
            # another schedule and another noise: the same graph
            torch.manual_seed(55)
            ab.sample_confident(steps, schedule="linear", selection_noise=1.0)
            assert len(ab._graphs) == 1
    assert int(want.max()) < K128
    assert all(sum(v) == 0 for v in bad.values()), bad


def test_completion_keeps_the_known_tokens_under_a_schedule_and_noise(dev, ops):
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
    ab = sampler(den, True, True, True)
    torch.manual_seed(2026)
    res = complete_images_confident(model, ab, images, keep, sample_steps=steps, temp=0.9, schedule="cosine", selection_noise=4.5)
    codes = model.encode_images(images)
    assert 0 < int(res.known.sum()) < res.known.numel()
    assert int((res.tokens[res.known] != codes[res.known]).sum()) == 0, "known tokens come back unchanged"
    assert int(res.tokens.max()) < K128 and int(res.tokens.min()) >= 0
    torch.manual_seed(2026)
    plain = complete_images_confident(model, ab, images, keep, sample_steps=steps, temp=0.9)
    assert not torch.equal(plain.tokens, res.tokens) and torch.equal(plain.known, res.known)
    torch.manual_seed(2026)
    sh = complete_images_sharded(model, ab, images, keep, temp=0.9, sample_steps=steps, confident=True, schedule="cosine",
                                 selection_noise=4.5)
    assert torch.equal(sh, res.images_u8)
    with pytest.raises(ValueError):
        complete_images_sharded(model, ab, images, keep, schedule="cosine")


def test_step_count_sweep_hands_the_arguments_on(dev):
    from spkdiff.evaluate import step_count_sweep
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    ab = sampler(den, True, True, True)
    torch.manual_seed(9)
    _, tok = step_count_sweep(model, ab, [2, 6], 3, batch=4, schedule="cosine", selection_noise=3.0)
    want = []
    for g, s in enumerate((2, 6)):
        one = sampler(den, True, True, False).set_shard(3 * g, 3)
        torch.manual_seed(9)
        want.append(one.sample_confident(s, schedule="cosine", selection_noise=3.0).reshape(3, 7, 7))
    assert torch.equal(tok, torch.stack(want))
    with pytest.raises(ValueError):
        step_count_sweep(model, ab, [2, 6], 3, schedule=[0, 1, 2])


# ------------------------------------------------------------------------------------------------- 6. what the feature is for
def test_greedy_decoding_depends_on_the_key_exactly_when_the_noise_is_on(dev):
    """The trained checkpoint, 8 steps, top_k = 1, two keys: with tau = 0 the tokens of the two keys are identical -- greedy decoding
    plus a fixed order is deterministic --, with tau > 0 they differ in at least one image."""
    from snn_model.vq_diffusion import DummyModel, functional
    sd = synth.trained_state('denoiser')
    den = DummyModel(1, synth.MNIST.num_embeddings).to(dev)
    functional.set_step_mode(net=den, step_mode='m')
    den.load_state_dict(sd)
    ab = sampler(den.eval(), True, True, True)
    ab.n_samples = 8
    out = {}
    for tau in (0.0, 4.5):
        for seed in (1, 2):
            torch.manual_seed(seed)
            out[tau, seed] = ab.sample_confident(8, top_k=1, schedule="cosine", selection_noise=tau)
            out[tau, seed, "key"] = ab.last_key
    assert out[0.0, 1, "key"] != out[0.0, 2, "key"]
    assert torch.equal(out[0.0, 1], out[0.0, 2])
    differ = (out[4.5, 1] != out[4.5, 2]).flatten(1).any(1)
    print(f"greedy decoding, tau = 4.5: {int(differ.sum())} of 8 images differ between the two keys")
    assert int(differ.sum()) >= 1
    assert int(out[4.5, 1].max()) < K128


# ------------------------------------------------------------------------------------------------- 7. what the wrappers refuse
def test_wrappers_refuse_bad_tables_before_launching(dev, ops):
    Bn, h, S = 5, 7, 4
    g = torch.Generator().manual_seed(1)
    logits, x0, un0, _, _ = _state(Bn, K128, h, g, dev)
    w = torch.tensor([cso.linear_weights(S)] * Bn, dtype=torch.int32, device=dev)
    a = torch.zeros(Bn, S + 1, device=dev)
    calls = [dict(sched_w=None), dict(sched_w=w.cpu()), dict(sched_w=w.long()), dict(sched_w=w[:4].contiguous()), dict(sched_w=w[:, :4].contiguous()),
             dict(sched_w=w.float()), dict(noise_a=a.cpu()), dict(noise_a=a.double()), dict(noise_a=a[:, :4].contiguous()),
             dict(noise_a=1.0), dict(t=0), dict(t=5), dict(S=0), dict(S=3), dict(score=torch.zeros(3, device=dev)),
             dict(score=torch.zeros(Bn * h * h, dtype=torch.float64, device=dev)), dict(temp=0.0)]
    for kw in calls:
        x, un = x0.clone(), un0.clone()
        args = dict(dict(t=2, temp=1.0, sched_w=w, S=S, noise_a=a), **kw)
        with pytest.raises(ValueError):
            ops.psample_step_conf_sched(logits, x, un, args.pop("t"), args.pop("temp"), args.pop("sched_w"), args.pop("S"), **args)
        torch.cuda.synchronize()
        assert torch.equal(x, x0) and torch.equal(un, un0), f"a refused call launched nothing: {kw}"
    with pytest.raises(ValueError, match="active_set"):
        ops.psample_step_conf_listed_sched(logits, x0.clone(), un0.clone(), 2, 1.0, torch.full((Bn,), S, dtype=torch.int32, device=dev),
                                           S, SIGMA, w, a)
    big = torch.randn(2, 16, 65, 1, generator=g).to(dev)
    with pytest.raises(NotImplementedError):
        ops.psample_step_conf_sched(big, torch.full((2, 1, 65, 1), 16, dtype=torch.int64, device=dev),
                                    torch.zeros((2, 1, 65, 1), dtype=torch.bool, device=dev), 2, 1.0, w[:2].contiguous(), S)
