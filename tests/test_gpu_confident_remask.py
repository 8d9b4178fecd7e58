"""GPU tests of remasking for confidence-ordered decoding (run with ``-m gpu`` on an MI355X): the three ``_remask``
entry points against their ``_sched`` siblings bit for bit (zero table: everything; any table: the reveal and its three outputs), the
remasked set against a literal sort of the ``commit_conf`` handed in (tests/_confident_remask_oracle.py), ``commit_conf`` and
``remasked_out`` exactly, the edge cases of the rule one image each, the listed form, the fused step tail against its three launches,
and ``AbsorbingDiffusion.sample_confident(remask=)`` in every form.  No case needs a tolerance: every decision is compared on the
kernel's own fp32 outputs in integer order."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _confident_oracle as cfo             # noqa: E402
import _confident_remask_oracle as cro      # noqa: E402
import _confident_sched_oracle as cso       # noqa: E402
import _confident_steps_oracle as cst       # noqa: E402
from spkdiff import schedules as sch        # noqa: E402
from spkdiff import synth                   # noqa: E402
from test_gpu_completion import K as K128, build_den, build_vae, sampler      # noqa: E402  (the helpers, not the tests)
from test_gpu_confident_sched import _bits, _differ, listed_sched_call, sched_call      # noqa: E402
from test_gpu_temps import _den_k, _state   # noqa: E402

SIGMA = cst.STEP_STRIDE
KS = (2, 65, 128, 512, 2048)
S_TABLE = 100
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def remask_call(ops, dev, logits, x0, un0, cc0, t, temp, top_k, top_p, w, a, S, R, mask_id, nxt=False, **noise):
    """One remasking update on copies of the state -> (x_t, unmasked, x0_hat, conf, score, next_input or None, commit_conf, remasked);
    the outputs are pre-filled with sentinels the kernel must leave where nothing may be written."""
    n = x0.numel()
    x, un, cc = x0.clone(), un0.clone(), cc0.clone()
    hat = torch.full((n,), -5, dtype=torch.int64, device=dev)
    conf = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    score = torch.full((n,), 9.0, dtype=torch.float32, device=dev)
    rem = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    ni = torch.full((x0.shape[0], 2) + tuple(logits.shape[2:]), float("nan"), device=dev) if nxt else None
    ops.psample_step_conf_remask(logits, x, un, t, temp, w, S, R, cc, mask_id, noise_a=a, x0_hat=hat, conf=conf, score=score,
                                 remasked=rem, next_input=ni, top_k=top_k, top_p=top_p, **noise)
    return x, un, hat, conf, score, ni, cc, rem


def commit_conf_for(un, gen, specials=True):
    """A commit_conf for a state: random log-probabilities at the unmasked positions, among them -- per image, where it has enough
    of them -- a +inf (a known token), a NaN, a -inf and a tied pair; garbage at the masked positions (ignored)."""
    Bn, HW = un.shape
    cc = -torch.rand(Bn, HW, generator=gen) * 9
    cc[~un] = 123.0
    if specials:
        for b in range(Bn):
            pos = un[b].nonzero().flatten().tolist()
            if len(pos) >= 6:
                cc[b, pos[0]] = INF
                cc[b, pos[2]] = float("nan") if b % 2 else -INF
                cc[b, pos[3]] = cc[b, pos[5]]
                cc[b, pos[-1]] = INF
    return cc


def check_against_oracle(name, add, Bn, HW, t, mask_id, xh, unh, cch, w, R, got):
    """The kernel's state after a remasking step against the oracle run on the kernel's own candidates, confidences and scores."""
    x, un, hat, conf, score, ni, cc, rem = got
    wp, wc, rr = w[:, t - 1].tolist(), w[:, t].tolist(), R[:, t].tolist()
    wx, wun, wcc, rev, rmk, counts = cro.remask_state(xh, unh, cch, hat.cpu().reshape(Bn, HW), conf.cpu().reshape(Bn, HW),
                                                      score.cpu().reshape(Bn, HW), wp, wc, rr, t, mask_id)
    rx, run, rcc, _, _, _ = cro.remask_state(xh, unh, cch, hat.cpu().reshape(Bn, HW), conf.cpu().reshape(Bn, HW),
                                             score.cpu().reshape(Bn, HW), wp, wc, rr, t, mask_id, remask=cro.remask_by_rank)
    add(f"{name}_mirror_differs", (rx != wx).sum() + (run != wun).sum())
    add(f"{name}_state_differs", (x.cpu().reshape(Bn, HW) != wx).sum() + (un.cpu().reshape(Bn, HW).bool() != wun).sum())
    add(f"{name}_commit_conf_differs", (_bits(cc.cpu().reshape(Bn, HW)) != _bits(wcc)).sum())
    m = (~unh).sum(1)
    want_rem = torch.where((m > 0)[:, None], rmk.to(torch.uint8), torch.full((Bn, HW), 7, dtype=torch.uint8))
    add(f"{name}_remasked_out_differs", (rem.cpu().reshape(Bn, HW) != want_rem).sum())
    add(f"{name}_remasked_a_masked_or_revealed", (rmk & ~unh).sum() + (rmk & rev).sum())
    return counts, rmk


# ------------------------------------------------------------------------------------------------- 1. the sampling kernel
@pytest.mark.parametrize("HW", cfo.HWS)
@pytest.mark.parametrize("K", KS)
def test_psample_step_conf_remask_vs_sibling_and_oracle(dev, ops, K, HW):
    """The case table of tests/_confident_oracle.conf_inputs (B = 5 in one batch, m = 0, 1, 2, HW - 1, HW), t in {1, 2, 50, 100} inside
    a loop of S = 100, injected and Philox noise.  ZERO TABLE: tokens, unmasked, x0_hat, conf, score and next_input are bit for bit
    spk_psample_step_conf_sched's.  NON-ZERO TABLE: the three outputs are still the sibling's; the state, commit_conf and remasked_out
    are the oracle's on the kernel's own outputs and the commit_conf handed in; sentinels survive where nothing may be written."""
    logits, q, x0, un0, temps, ks, ps = cfo.conf_inputs(K, HW)
    ld, x0d, un0d, tv, kd, pd = (v.to(dev) for v in (logits, x0, un0, temps, ks, ps))
    Bn, S, mask_id = cfo.B, S_TABLE, K
    g = torch.Generator().manual_seed(K * 11 + HW)
    xh, unh = x0.reshape(Bn, HW), un0.reshape(Bn, HW).bool()
    cch = commit_conf_for(unh, g)
    ccd = cch.to(dev)
    w = torch.tensor(cso.table_rows(S, Bn), dtype=torch.int32)
    a = torch.tensor([cso.noise_row((0.0, 0.5, 4.5, 300.0, 2.0)[b], S, S) for b in range(Bn)], dtype=torch.float32).to(dev)
    R0 = torch.zeros(Bn, S + 1, dtype=torch.int32)
    R = torch.tensor([[(3, 64, 1, 2, 5)[b]] * (S + 1) for b in range(Bn)], dtype=torch.int32)
    seed, off = 0x1234_5678_9ABC, 5 * SIGMA + 11 * HW * K
    noises = {"philox": dict(seed=seed, offset=off),
              "injected": dict(q=q.to(dev), u=torch.rand(Bn * HW, generator=g).clamp_(min=2.0 ** -24).to(dev))}
    total = {}

    def add(k, v):
        total[k] = total.get(k, 0) + int(v)

    masked = ~un0.flatten()
    for t in (1, 2, 50, 100):
        for mode, kw in noises.items():
            sib = sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, w.to(dev), a, S, nxt=True, **kw)
            got = remask_call(ops, dev, ld, x0d, un0d, ccd, t, tv, kd, pd, w.to(dev), a, S, R0.to(dev), mask_id, nxt=True, **kw)
            add("zero_table_differs_from_sibling", _differ(got[:6], sib))
            check_against_oracle("zero", add, Bn, HW, t, mask_id, xh, unh, cch, w, R0, got)
            add("zero_table_remasked", (got[7].cpu() == 1).sum())
            got = remask_call(ops, dev, ld, x0d, un0d, ccd, t, tv, kd, pd, w.to(dev), a, S, R.to(dev), mask_id, nxt=True, **kw)
            add("outputs_differ_from_sibling", _differ(got[2:5], sib[2:5]))
            add("revealed_differ_from_sibling", ((got[1] & ~un0d) != (sib[1] & ~un0d)).sum() + (got[0] != sib[0])[sib[1] & ~un0d].sum())
            add("touched_unmasked_outputs", (got[2].cpu()[~masked] != -5).sum() + (got[3].cpu()[~masked] != 7.0).sum()
                + (got[4].cpu()[~masked] != 9.0).sum())
            counts, rmk = check_against_oracle("table", add, Bn, HW, t, mask_id, xh, unh, cch, w, R, got)
            add("next_input", not torch.equal(got[5], ops.den_build_input(got[0], t - 1)))
            if t == 1:
                add("remasked_at_t1", rmk.sum())
            elif HW >= 49:
                assert int(rmk.sum()) > 0, "the case remasks something"
            # without the optional outputs: the same state
            x2, un2, cc2 = x0d.clone(), un0d.clone(), ccd.clone()
            ops.psample_step_conf_remask(ld, x2, un2, t, tv, w.to(dev), S, R.to(dev), cc2, mask_id, noise_a=a, top_k=kd, top_p=pd, **kw)
            add("without_outputs", _differ((x2, un2, cc2), (got[0], got[1], got[6])))
    print(f"conf_remask K={K} HW={HW}: {total}")
    assert all(v == 0 for v in total.values()), total


# ------------------------------------------------------------------------------------------------- 2. the edge cases, one image each
@pytest.mark.parametrize("HW", [49, 64])
def test_edge_cases_one_image_each(dev, ops, HW):
    K, S, mask_id = 128, 8, 128
    h = 7 if HW == 49 else 8
    g = torch.Generator().manual_seed(HW)
    names = ["c0", "R_above_c", "tied", "nan_first", "inf_never", "m0", "all_lanes"]
    Bn = len(names)
    un = torch.zeros(Bn, HW, dtype=torch.bool)
    cc = torch.full((Bn, HW), 55.0)
    un[0, 10:30] = True; cc[0, 10:30] = INF                                # c = 0 with R > 0
    un[1, 5:25] = True; cc[1, 5:25] = INF; cc[1, [6, 11, 20]] = torch.tensor([-1.0, -2.0, -0.5])     # R > c: all three go
    un[2, 8:40] = True; cc[2, 8:40] = 0.0                                  # all keys tied (top_k = 1: every confidence is exactly 0)
    un[3, 0:20] = True; cc[3, 0:20] = -torch.rand(20, generator=g) - 1; cc[3, 13] = float("nan"); cc[3, 4] = -INF
    un[4, 2:44] = True; cc[4, 2:44] = INF; cc[4, 30:34] = torch.tensor([-3.0, -0.1, -7.0, -2.0])     # +inf never, R = 64
    un[5, :] = True; cc[5, :] = -torch.rand(HW, generator=g)               # m = 0 with revisable tokens: untouched
    un[6, 0::2] = True; cc[6, 0::2] = -torch.rand((HW + 1) // 2, generator=g)                        # every lane masked or revisable
    Rrow = [5, 64, 6, 1, 64, 9, 64]
    R = torch.tensor([[r] * (S + 1) for r in Rrow], dtype=torch.int32)
    w = torch.tensor([cso.linear_weights(S)] * Bn, dtype=torch.int32)
    x = torch.where(un, torch.randint(0, K, (Bn, HW), generator=g), torch.full((Bn, HW), mask_id))
    logits = torch.randn(Bn, K, h, h, generator=g) * 3
    q = torch.empty(Bn * HW, K).exponential_(1, generator=g)
    xd, und, ccd = x.reshape(Bn, 1, h, h).to(dev), un.reshape(Bn, 1, h, h).to(dev), cc.to(dev)
    total = {}

    def add(k, v):
        total[k] = total.get(k, 0) + int(v)

    for t in (3, 1):
        got = remask_call(ops, dev, logits.to(dev), xd, und, ccd, t, 1.0, None, None, w.to(dev), None, S, R.to(dev), mask_id, nxt=True,
                          q=q.to(dev))
        counts, rmk = check_against_oracle(f"t{t}", add, Bn, HW, t, mask_id, x, un, cc, w, R, got)
        if t == 1:
            assert int(rmk.sum()) == 0 and int((~got[1].cpu()).sum()) == 0, "t = 1 remasks nothing and leaves nothing masked"
            continue
        pos = lambda b: rmk[b].nonzero().flatten().tolist()          # noqa: E731
        assert pos(0) == [] and pos(1) == [6, 11, 20] and pos(2) == list(range(34, 40)), (pos(0), pos(1), pos(2))
        assert pos(3) == [13], "a NaN commit_conf goes first (before -inf)"
        assert pos(4) == [30, 31, 32, 33] and pos(5) == []
        assert pos(6) == list(range(0, HW, 2)), "all of the revisable half"
        # image 5 is untouched: state, commit_conf, remasked_out
        assert torch.equal(got[0].cpu().reshape(Bn, HW)[5], x[5]) and bool(got[1].cpu().reshape(Bn, HW)[5].all())
        assert bool((got[7].cpu().reshape(Bn, HW)[5] == 7).all()) and torch.equal(got[6].cpu()[5], cc[5])
        # all 64 lanes in play on 8 x 8: image 6 reveals among the odd positions and remasks the even ones
        assert int((got[1].cpu().reshape(Bn, HW)[6, 1::2]).sum()) == counts[6][0] and counts[6][1] == (HW + 1) // 2
    assert all(v == 0 for v in total.values()), total


# ------------------------------------------------------------------------------------------------- 3. the listed form
def listed_remask_call(ops, dev, logits, x0, un0, cc0, t, temp, top_k, top_p, steps, S, lst, w, a, R, mask_id, **noise):
    Bn, n = x0.shape[0], x0.numel()
    slots = torch.full_like(logits, float("nan"))
    slots[:len(lst)] = logits[torch.tensor(lst, dtype=torch.int64, device=dev)]
    act = torch.full((Bn,), -1, dtype=torch.int32, device=dev)
    act[:len(lst)] = torch.tensor(lst, dtype=torch.int32, device=dev)
    nact = torch.tensor([len(lst), 0], dtype=torch.int32, device=dev)
    x, un, cc = x0.clone(), un0.clone(), cc0.clone()
    hat = torch.full((n,), -5, dtype=torch.int64, device=dev)
    conf = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    score = torch.full((n,), 9.0, dtype=torch.float32, device=dev)
    rem = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    with ops.active_set(act, nact):
        ops.psample_step_conf_listed_remask(slots, x, un, t, temp, steps, S, SIGMA, w, R, cc, mask_id, noise_a=a, x0_hat=hat, conf=conf,
                                            score=score, remasked=rem, top_k=top_k, top_p=top_p, **noise)
    return x, un, hat, conf, score, cc, rem


@pytest.mark.parametrize("HW", cfo.HWS)
@pytest.mark.parametrize("K", KS)
def test_listed_remask_equals_the_dense_remask_and_leaves_the_rest_alone(dev, ops, K, HW):
    """Full list, all counts S: everything is the dense call's.  A sub-list in another order (slots != images): listed images as the
    dense call, the others untouched, commit_conf and remasked_out included.  An image with e < S at t <= e draws at the shifted
    counters, as the sibling does; one with t > e_i is untouched.  The zero table: the `_sched` listed sibling."""
    logits, q, x0, un0, temps, ks, ps = cfo.conf_inputs(K, HW)
    ld, x0d, un0d, tv, kd, pd = (v.to(dev) for v in (logits, x0, un0, temps, ks, ps))
    Bn, S, t, e, mask_id = cfo.B, 6, 2, 3, K
    g = torch.Generator().manual_seed(K * 13 + HW)
    ccd = commit_conf_for(un0.reshape(Bn, HW).bool(), g).to(dev)
    w = torch.tensor(cso.table_rows(S), dtype=torch.int32, device=dev)
    a = torch.tensor([cso.noise_row((0.0, 0.5, 4.5, 300.0, 2.0)[b], S, S) for b in range(Bn)], dtype=torch.float32, device=dev)
    R = torch.tensor([[(3, 64, 1, 2, 5)[b]] * (S + 1) for b in range(Bn)], dtype=torch.int32, device=dev)
    seed, off = 0x1234_5678_9ABC, 5 * SIGMA + 11 * HW * K
    noises = {"philox": dict(seed=seed, offset=off),
              "injected": dict(q=q.to(dev), u=torch.rand(Bn * HW, generator=g).clamp_(min=2.0 ** -24).to(dev))}
    full = torch.full((Bn,), S, dtype=torch.int32, device=dev)
    mixed = torch.tensor([S, S, S + 7, e, e], dtype=torch.int32, device=dev)
    every = list(range(Bn))
    bad = {}

    def rows(a_, b_, which):
        return sum(int((_bits(u_).reshape(Bn, HW)[which] != _bits(v_).reshape(Bn, HW)[which]).sum()) for u_, v_ in zip(a_, b_))

    def dense(tt, **kw):
        r = remask_call(ops, dev, ld, x0d, un0d, ccd, tt, tv, kd, pd, w, a, S, R, mask_id, **kw)
        return r[:5] + r[6:]

    untouched = (x0d, un0d, torch.full((Bn * HW,), -5, device=dev), torch.full((Bn * HW,), 7.0, device=dev),
                 torch.full((Bn * HW,), 9.0, device=dev), ccd, torch.full((Bn * HW,), 7, dtype=torch.uint8, device=dev))
    for mode, kw in noises.items():
        for tt in (t, S):
            got = listed_remask_call(ops, dev, ld, x0d, un0d, ccd, tt, tv, kd, pd, full, S, every, w, a, R, mask_id, **kw)
            bad[f"{mode}_full_t{tt}"] = rows(got, dense(tt, **kw), every)
        d = dense(t, **kw)
        sub = listed_remask_call(ops, dev, ld, x0d, un0d, ccd, t, tv, kd, pd, full, S, [4, 0, 2], w, a, R, mask_id, **kw)
        bad[f"{mode}_sub_listed"] = rows(sub, d, [0, 2, 4])
        bad[f"{mode}_sub_unlisted"] = rows(sub, untouched, [1, 3])
        mix = listed_remask_call(ops, dev, ld, x0d, un0d, ccd, t, tv, kd, pd, mixed, S, every, w, a, R, mask_id, **kw)
        bad[f"{mode}_above_S_is_S"] = rows(mix, d, [0, 1, 2])
        late = listed_remask_call(ops, dev, ld, x0d, un0d, ccd, e + 1, tv, kd, pd, mixed, S, every, w, a, R, mask_id, **kw)
        bad[f"{mode}_t_above_e_untouched"] = rows(late, untouched, [3, 4])
        zero = listed_remask_call(ops, dev, ld, x0d, un0d, ccd, t, tv, kd, pd, mixed, S, [3, 1, 0, 4, 2], w, a, torch.zeros_like(R), mask_id, **kw)
        sib = listed_sched_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, mixed, S, [3, 1, 0, 4, 2], w, a, **kw)
        bad[f"{mode}_zero_table_is_the_sibling"] = rows(zero[:5], sib, every)
        if mode == "philox":
            shifted = dict(kw, offset=kw["offset"] - (S - e) * SIGMA)
            bad[f"{mode}_shifted"] = rows(mix, dense(t, **shifted), [3, 4])
    print(f"conf_listed_remask K={K} HW={HW}: {bad}")
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 4. the fused step tail
@pytest.mark.parametrize("L", [7, 8])
@pytest.mark.parametrize("Kc", [100, 128, 256, 512])
def test_den_step_tail_conf_remask_equals_the_three_launch_form(dev, ops, Kc, L):
    """spk_den_step_tail_conf_remask == spk_den_conv3x3_counts_mfma, then spk_psample_step_conf_remask, then the first-layer launch, bit
    for bit: tokens, unmasked, commit_conf, remasked_out, x0_hat, conf, score, the logits and the next step's S32 spikes and counts --
    first, middle and last step.  In the middle case the corner position of every image holds the smallest commit_conf, so it is
    remasked and the fused first layer must read mask_id next to the border."""
    from spkdiff.ops import IN_TINV
    den = _den_k(Kc, dev)
    assert den.tail_fusable(L, L)
    Bn, HW, S, mask_id = 3, L * L, 12, Kc
    g = torch.Generator().manual_seed(Kc * 10 + L)
    _, xh, unh, u, q = _state(Bn, Kc, L, g, dev)
    unh[:, :, 0, 0] = True
    xh = torch.where(unh, xh.clamp(max=Kc - 1), torch.full_like(xh, Kc))
    tv = torch.tensor((0.5, 1.0, 2.0), dtype=torch.float32, device=dev)
    kd = torch.tensor([0, 5, Kc // 2], dtype=torch.int32, device=dev)
    pd = torch.tensor([0.5, 1.0, 0.9], dtype=torch.float32, device=dev)
    rows = cso.table_rows(S, 5)
    w = torch.tensor([rows[1], rows[0], rows[3]], dtype=torch.int32, device=dev)
    a = torch.tensor([cso.noise_row(tau, S, S) for tau in (4.5, 0.0, 50.0)], dtype=torch.float32, device=dev)
    R = torch.tensor([[2] * (S + 1), [64] * (S + 1), [5] * (S + 1)], dtype=torch.int32, device=dev)
    den._trunk(ops.den_build_input(xh, 1), False)
    conv6, packed6 = den._conv6_params()
    conv1, bn1 = den.conv1[0], den.conv1[1]
    a1, b1 = bn1.affine_terms()
    c1 = (conv1._spk_params.get(conv1), conv1.bias.detach(), a1, b1)
    xfull = torch.where(unh, xh, (xh + 1) % 7)
    few = torch.ones_like(unh)
    few[:, :, 0, 1:4] = False
    cases = {"first": (xfull, torch.zeros_like(unh), 12), "middle": (xfull, unh, 5), "last": (xfull, few, 1)}
    bad = {}
    for name, (x0, un0, t) in cases.items():
        x0 = torch.where(un0, x0, torch.full_like(x0, Kc))
        cc0 = commit_conf_for(un0.reshape(Bn, HW).cpu(), g).to(dev)
        cc0[:, 0] = -100.0                                                 # (the corner: the least trusted where it is unmasked)
        _, cnt5, _, cnt1, which, _, collapse = den._trunk(ops.den_build_input(x0, t), False)
        assert which == 'mfma-fp6v2' and collapse
        nxt = c1 if t > 1 else None
        for mode, kw in {"philox": dict(seed=4242, offset=1000 * t), "injected": dict(q=q, u=u)}.items():
            x, un, cc = x0.clone(), un0.clone(), cc0.clone()
            hat = torch.full((Bn * HW,), -5, dtype=torch.int64, device=dev)
            cf = torch.full((Bn * HW,), 7.0, device=dev)
            sc = torch.full((Bn * HW,), 9.0, device=dev)
            rem = torch.full((Bn * HW,), 7, dtype=torch.uint8, device=dev)
            pre, lg = ops.den_step_tail_conf_remask(cnt5, cnt1, packed6, x, un, t, tv, w, S, R, cc, mask_id, T=16, K=Kc, noise_a=a,
                                                    conv1=nxt, want_logits=True, top_k=kd, top_p=pd, x0_hat=hat, conf=cf, score=sc,
                                                    remasked=rem, **kw)
            lr = ops.den_conv3x3_counts(cnt5, packed6, Kc, 16, cnt1=cnt1)
            xr, unr, hr, cr, sr, _, ccr, remr = remask_call(ops, dev, lr, x0, un0, cc0, t, tv, kd, pd, w, a, S, R, mask_id, **kw)
            n = int(not torch.equal(lg, lr)) + _differ((x, un, hat, cf, sc, cc, rem), (xr, unr, hr, cr, sr, ccr, remr))
            if name == "middle":
                assert bool((rem.reshape(Bn, HW)[:, 0] == 1).all()) and bool((x.reshape(Bn, HW)[:, 0] == mask_id).all()), "the corner is remasked"
            else:
                assert int((rem == 1).sum()) == 0, "nothing revisable (first) / t = 1 (last)"
            if t > 1:
                r1 = den.conv1.run(ops.den_build_input(xr, t - 1), IN_TINV, final='ptc', T=16, stateful=False,
                                   chunk_out=ops.S32.chunk, want_counts=True)
                n += int(not torch.equal(pre[0], r1['ptc'])) + int(not torch.equal(pre[1], r1['cnt']))
            else:
                assert pre is None
            bad[f"{name}_{mode}"] = n
            # the zero table: spk_den_step_tail_conf_sched
            xs, uns = x0.clone(), un0.clone()
            hs, cs, ss = torch.full_like(hat, -5), torch.full_like(cf, 7.0), torch.full_like(sc, 9.0)
            ps_, ls = ops.den_step_tail_conf_sched(cnt5, cnt1, packed6, xs, uns, t, tv, w, S, T=16, K=Kc, noise_a=a, conv1=nxt,
                                                   want_logits=True, top_k=kd, top_p=pd, x0_hat=hs, conf=cs, score=ss, **kw)
            xi, uni, cci = x0.clone(), un0.clone(), cc0.clone()
            hi, ci, si = torch.full_like(hat, -5), torch.full_like(cf, 7.0), torch.full_like(sc, 9.0)
            pi, li = ops.den_step_tail_conf_remask(cnt5, cnt1, packed6, xi, uni, t, tv, w, S, torch.zeros_like(R), cci, mask_id, T=16,
                                                   K=Kc, noise_a=a, conv1=nxt, want_logits=True, top_k=kd, top_p=pd, x0_hat=hi, conf=ci,
                                                   score=si, **kw)
            k = _differ((xi, uni, hi, ci, si, li), (xs, uns, hs, cs, ss, ls))
            if t > 1:
                k += int(not torch.equal(pi[0], ps_[0])) + int(not torch.equal(pi[1], ps_[1]))
            bad[f"{name}_{mode}_zero_table"] = k
    print(f"den_step_tail_conf_remask K={Kc} {L}x{L}: {bad}")
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 5. the sampler, every form
def _known(Bn, seed, dev):
    g = torch.Generator().manual_seed(seed)
    known = torch.rand(Bn, 7, 7, generator=g) < 0.3
    known[0] = False
    x_init = torch.randint(0, K128, (Bn, 7, 7), generator=g)
    return x_init.to(dev), known.to(dev)


def _tables_for(steps):
    v = {"r2": 2}
    if steps < 60:                               # (the long run takes two of the four: every path is taken, in a quarter of the launches)
        v["r4_cosine_noisy"] = 4
    if 5 <= steps < 60:
        v["table"] = [0, 0] + [(3 * t) % 7 for t in range(2, steps + 1)]
    if steps >= 5:
        v["per_image"] = [0, 1, [0, 0] + [5] * (steps - 1), 64, 3, None]
    return v


@pytest.mark.parametrize("steps", [1, 5, 12, 60])
def test_sample_confident_remask_gives_the_same_tokens_in_every_form(dev, steps):
    """Fused tail == three launches == captured; ONE captured graph replayed with different remask tables and different ``known`` sets
    == the eager calls; no mask_id is left; known tokens come back unchanged; ``remask=0`` == the call without it under
    ``schedule='linear'``; a recorded run replayed through the oracle gives the (n_t, r_t) of run_counts_remask."""
    den, _ = build_den(synth.MNIST, dev)
    Bn = 6
    variants = _tables_for(steps)
    bad, want = {}, {}
    starts = {"free": (None, None), "known_a": _known(Bn, 1, dev), "known_b": _known(Bn, 2, dev)}
    tail0 = den.use_step_tail
    try:
        for tail in (True, False):
            den.use_step_tail = tail
            for graph in (False, True):
                ab = sampler(den, True, True, graph)
                ab.n_samples = Bn
                for sname, (xi, kn) in starts.items():
                    for name, rm in variants.items():
                        kw = dict(schedule="cosine", selection_noise=4.5) if "cosine" in name else {}
                        if xi is not None:
                            kw.update(x_init=xi, known=kn)
                        torch.manual_seed(8100 + steps)
                        with warnings.catch_warnings(record=True) as seen:
                            warnings.simplefilter("always")
                            got = ab.sample_confident(steps, remask=rm, **kw)
                        assert not [str(w.message) for w in seen if "spkdiff" in str(w.message)], "no capture fall-back"
                        ref = want.setdefault((sname, name), got)
                        bad[f"{'tail' if tail else 'dense'}_{'graph' if graph else 'eager'}_{sname}_{name}"] = int((got != ref).sum())
                        assert int(got.max()) < K128 and int(got.min()) >= 0, "no mask_id is left"
                        if xi is not None:
                            assert torch.equal(got.reshape(Bn, 7, 7)[kn], xi[kn]), "known tokens come back unchanged"
                if graph:
                    keys = [k for k in ab._graphs if "remask" in k]
                    assert keys and all("scheduled" in k and "confident" in k for k in keys)
                    assert len(keys) <= 2, "one graph per (batch, S, conditional) serves every remask table"
                    gr = ab._graphs[keys[0]]
                    assert tuple(gr.remask.shape) == (Bn, steps + 1) and gr.commit_conf is not None
        # remask = 0 == no remask under the linear schedule
        den.use_step_tail = tail0
        ab = sampler(den, True, True, False)
        ab.n_samples = Bn
        torch.manual_seed(8100 + steps)
        zero = ab.sample_confident(steps, remask=0)
        torch.manual_seed(8100 + steps)
        lin = ab.sample_confident(steps, schedule="linear")
        bad["remask0_is_linear"] = int((zero != lin).sum())
    finally:
        den.use_step_tail = tail0
    if steps >= 5:
        assert not torch.equal(want["free", "r2"], zero), "remasking changes the tokens"
    # a recorded run: the trajectory of the host integers
    ab = sampler(den, True, True, False)
    ab.n_samples = Bn
    for name, wt in (("cosine", sch.cosine_weights(steps)), ("linear", sch.linear_weights(steps))):
        rec = []
        torch.manual_seed(8100 + steps)
        ab.sample_confident(steps, schedule=name, selection_noise=2.0, remask=3, record=rec)
        prev = torch.zeros(Bn, 49, dtype=torch.bool)
        counts = []
        for _, _, un_after, _ in rec:
            now = un_after.flatten(1).cpu()
            counts.append(((now & ~prev).sum(1).tolist(), (prev & ~now).sum(1).tolist()))
            prev = now
        wantc = sch.run_counts_remask(49, wt, 3)
        assert counts == [([n] * Bn, [r] * Bn) for n, r in wantc] and bool(prev.all()), (name, counts, wantc)
        assert wantc == cro.run_counts_remask(49, wt, [0, 0] + [3] * (steps - 1))
    print(f"sample_confident remask {steps} steps: {bad}")
    assert all(v == 0 for v in bad.values()), bad


def test_image_i_of_a_mixed_run_equals_its_own_run(dev):
    """Per-image step counts: row i is built for e_i, and image i equals image i of the one-count call with its row -- eager and
    captured."""
    den, _ = build_den(synth.MNIST, dev)
    steps = [1, 3, 8, 12, 5, 12]
    Bn = len(steps)
    rms = [0, 2, [0, 0, 1, 2, 3, 4, 5, 6, 7], 64, None, 3]
    solo = []
    for i, e in enumerate(steps):
        one = sampler(den, True, True, False).set_shard(i, 1)
        torch.manual_seed(56)
        solo.append(one.sample_confident(e, remask=0 if rms[i] is None else rms[i], schedule="cosine", selection_noise=1.5, temp=0.9))
    want = torch.cat(solo)
    bad = {}
    for graph in (False, True):
        ab = sampler(den, True, True, graph)
        ab.n_samples = Bn
        for rep in range(2 if graph else 1):
            torch.manual_seed(56)
            got = ab.sample_confident(steps, remask=rms, schedule="cosine", selection_noise=1.5, temp=0.9)
            bad[f"{'graph' if graph else 'eager'}_{rep}"] = (got != want).flatten(1).sum(1).tolist()
        if graph:
            key = next(iter(ab._graphs))
            assert len(ab._graphs) == 1 and "remask" in key and "per-image-steps" in key
    assert int(want.max()) < K128
    assert all(sum(v) == 0 for v in bad.values()), bad


def test_shards_of_two_and_four_equal_the_whole_job(dev):
    den, _ = build_den(synth.MNIST, dev)
    Bn, steps = 8, 12
    rms = [[0, 0] + [i] * 11 for i in range(Bn)]                        # (one table per image: a slice of them stays per-image)
    bad, want = {}, None
    for parts in (1, 2, 4):
        n = Bn // parts
        for graph in (False, True):
            out = []
            for i in range(parts):
                lo, hi = i * n, (i + 1) * n
                sh = sampler(den, True, True, graph).set_shard(lo, n)
                torch.manual_seed(42)
                out.append(sh.sample_confident(steps, remask=rms[lo:hi], selection_noise=2.0))
            got = torch.cat(out)
            want = got if want is None else want
            bad[f"{parts}_{'graph' if graph else 'eager'}"] = int((got != want).sum())
    assert all(v == 0 for v in bad.values()), bad


def test_completion_keeps_the_known_tokens_under_remasking(dev):
    from spkdiff.complete import complete_images_confident
    from spkdiff.dist import complete_images_sharded
    from spkdiff.evaluate import step_count_sweep
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    Bn, steps = 6, 6
    images = (synth.stroke_images(Bn, seed=78, img=28, channels=1) - 0.5).to(dev)
    keep = torch.ones(Bn, 28, 28, dtype=torch.bool)
    keep[:, 14:] = False
    keep = keep.to(dev)
    ab = sampler(den, True, True, True)
    torch.manual_seed(2027)
    res = complete_images_confident(model, ab, images, keep, sample_steps=steps, temp=0.9, remask=4)
    codes = model.encode_images(images)
    assert 0 < int(res.known.sum()) < res.known.numel()
    assert int((res.tokens[res.known] != codes[res.known]).sum()) == 0, "known tokens come back unchanged"
    assert int(res.tokens.max()) < K128 and int(res.tokens.min()) >= 0
    torch.manual_seed(2027)
    plain = complete_images_confident(model, ab, images, keep, sample_steps=steps, temp=0.9)
    assert not torch.equal(plain.tokens, res.tokens) and torch.equal(plain.known, res.known)
    torch.manual_seed(2027)
    sh = complete_images_sharded(model, ab, images, keep, temp=0.9, sample_steps=steps, confident=True, remask=4)
    assert torch.equal(sh, res.images_u8)
    with pytest.raises(ValueError):
        complete_images_sharded(model, ab, images, keep, remask=4)
    torch.manual_seed(9)
    _, tok = step_count_sweep(model, ab, [2, 6], 3, batch=4, remask=2)
    wantt = []
    for gi, s in enumerate((2, 6)):
        one = sampler(den, True, True, False).set_shard(3 * gi, 3)
        torch.manual_seed(9)
        wantt.append(one.sample_confident(s, remask=2).reshape(3, 7, 7))
    assert torch.equal(tok, torch.stack(wantt))


# ------------------------------------------------------------------------------------------------- 6. what is refused
def test_refusals(dev, ops):
    den, _ = build_den(synth.MNIST, dev)
    ab = sampler(den, True, True, True)
    ab.n_samples = 3
    state = torch.get_rng_state()
    for rm in (-1, 1.5, [0, 0, 1], [0, 1, 1, 1, 1], [1, 0, 1, 1, 1], [0, 0, -1, 1, 1], [0, 0, 1.0, 1, 1], [[0, 0, 1, 1, 1]] * 2,
               torch.ones(3, 5), "two", True):
        with pytest.raises(ValueError):
            ab.sample_confident(4, remask=rm)
    assert torch.equal(torch.get_rng_state(), state) and len(ab._graphs) == 0, "refused before a key is drawn"
    Bn, h, S = 5, 7, 4
    g = torch.Generator().manual_seed(1)
    logits, x0, un0, _, _ = _state(Bn, K128, h, g, dev)
    w = torch.tensor([cso.linear_weights(S)] * Bn, dtype=torch.int32, device=dev)
    R = torch.ones(Bn, S + 1, dtype=torch.int32, device=dev)
    cc = torch.zeros(Bn * h * h, device=dev)
    for kw in (dict(remask_r=None), dict(remask_r=R.cpu()), dict(remask_r=R.long()), dict(remask_r=R[:, :4].contiguous()),
               dict(commit_conf=None), dict(commit_conf=cc.double()), dict(commit_conf=cc[:5]), dict(mask_id=0), dict(mask_id=127),
               dict(mask_id=1.0), dict(remasked=torch.zeros(3, dtype=torch.uint8, device=dev)), dict(t=5), dict(sched_w=None)):
        x, un, c = x0.clone(), un0.clone(), cc.clone()
        args = dict(dict(t=2, temp=1.0, sched_w=w, S=S, remask_r=R, commit_conf=c, mask_id=K128), **kw)
        with pytest.raises(ValueError):
            ops.psample_step_conf_remask(logits, x, un, args.pop("t"), args.pop("temp"), args.pop("sched_w"), args.pop("S"),
                                         args.pop("remask_r"), args.pop("commit_conf"), args.pop("mask_id"), **args)
        torch.cuda.synchronize()
        assert torch.equal(x, x0) and torch.equal(un, un0) and torch.equal(c, cc), f"a refused call launched nothing: {kw}"
    with pytest.raises(ValueError, match="active_set"):
        ops.psample_step_conf_listed_remask(logits, x0.clone(), un0.clone(), 2, 1.0, torch.full((Bn,), S, dtype=torch.int32, device=dev),
                                            S, SIGMA, w, R, cc, K128)
