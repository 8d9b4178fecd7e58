"""GPU tests of nucleus (top-p) truncated sampling (run with ``-m gpu`` on an MI355X): ``spk_psample_step_topp``
against the oracle of tests/_topp_oracle.py (integer masses, the cut, the fp64 race on the truncated row) and its exact properties,
``spk_den_step_tail_topp`` against the three-launch form bit for bit, ``AbsorbingDiffusion.sample_top_p`` in every launch form,
eager and captured, against the host oracle, as a graph input, across shards and splits, and the completion wrapper."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _completion_oracle as corc           # noqa: E402
import _topp_oracle as tpo                  # noqa: E402
from parity_report import record as parity  # noqa: E402
from spkdiff import synth                  # noqa: E402
from test_gpu_completion import K as K128, build_den, build_vae, sampler      # noqa: E402  (the helpers, not the tests)
from test_gpu_sampler_noise_shapes import FRAGILE_CAP, REG_THRESHOLD      # noqa: E402
from test_gpu_temps import ACTIVE, LAUNCH_FORMS, _active, _den_k, _form_sampler, _state      # noqa: E402
from test_topp_host import ORACLE_PS, ORACLE_SEED      # noqa: E402  (the seed the host test vetted)

NEG_INF = float("-inf")
TEMPS = tpo.TEMPS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def step_call(ops, dev, logits, x0, un0, t, temp, top_k, top_p, hat=False, nxt=False, active=None, **noise):
    """One token update on copies of the state -> (x_t, unmasked, x0_hat or None, next_input or None)."""
    B, K, h, w = logits.shape
    x, un = x0.clone(), un0.clone()
    x0h = torch.full((B * h * w,), -5, dtype=torch.int64, device=dev) if hat else None
    ni = torch.full((B, 2, h, w), float("nan"), device=dev) if nxt else None
    kw = dict(noise, **({} if top_k is None else {"top_k": top_k}), **({} if top_p is None else {"top_p": top_p}))
    if active is not None:
        slots = torch.full_like(logits, float("nan"))            # slots beyond the list hold NaN and must never be read
        slots[:len(ACTIVE)] = logits[list(ACTIVE)]
        with ops.active_set(*active):
            ops.psample_step(slots, x, un, t, temp, **kw)
    else:
        ops.psample_step(logits, x, un, t, temp, x0_hat=x0h, next_input=ni, **kw)
    return x, un, x0h, ni


# ------------------------------------------------------------------------------------------------- 1 + 2. the sampling kernel
@pytest.mark.parametrize("kind", tpo.KINDS)
@pytest.mark.parametrize("K", tpo.KS)
def test_psample_step_topp_vs_oracle_and_exact_properties(dev, ops, K, kind):
    """The seeded case table (tests/_topp_oracle.topp_inputs: HW = 49, t = 3, p per image cycling through 1, 1e-6, 0.25, 0.5, 0.9,
    0.999, k through 0, 0, 5, K/2, K - 1, one NaN row, one all -inf row).  One call per uniform temperature and form (dense with
    next_input, x0_hat, the active list; injected noise, Philox, philox_state).  On rows that are not fragile (a cut within E of P:
    tests/_topp_oracle.fragile_cut, at most 10 % of the nucleus-truncated rows, which tests/test_topp_host.py asserts of this table
    without a GPU; or the race's two largest ratios within REG_THRESHOLD): every x0_hat lies in the oracle's kept set and the token
    is the fp64 race's on the oracle-truncated row.  With no allowance: p and k all off == spk_psample_step_temps and p off with k
    on == spk_psample_step_topk, bit for bit; p = 1e-6 images land on a row maximum; the NaN row and the all -inf row get token
    0; a call with mixed temperatures equals the uniform calls image by image."""
    logits, q, u, x0, un0, ps, ks = tpo.topp_inputs(K, kind)
    B, HW, t = logits.shape[0], 49, 3
    k_rows, p_rows = ks.long().repeat_interleave(HW), ps.repeat_interleave(HW).numpy()
    ld, x0d, un0d, kd, pd = logits.to(dev), x0.to(dev), un0.to(dev), ks.to(dev), ps.to(dev)
    seed, off = 0x1234_5678_9ABC, 5 * (1 << 40) + 11 * HW * K
    state = torch.tensor([seed, 1 << 33], dtype=torch.int64, device=dev)
    up, qp = ops.philox_noise(seed, off, B, HW, K, dev)
    noises = {"injected": (dict(u=u.to(dev), q=q.to(dev)), u, q),
              "philox": (dict(seed=seed, offset=off), up.cpu(), qp.cpu()),
              "philox_state": (dict(seed=99, offset=off - (1 << 33), philox_state=state), up.cpu(), qp.cpu())}
    act = _active(B, dev)
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(t), dtype=torch.float32)
    stats = dict(wrong=0, outside_kept=0, tiny_p_not_max=0, off_differs_temps=0, p_off_differs_topk=0, active_differs=0,
                 mixed_differs=0, next_input=0, degenerate_rows=0)
    cut_share, race_share = 0.0, 0.0
    uniform = {}
    p_off, k_off = torch.ones_like(pd), torch.zeros_like(kd)
    tiny = torch.from_numpy(p_rows == np.float32(1e-6))
    for temp in TEMPS:
        z32 = tpo.rows_of(logits) / temp                             # the fp32 division the kernel makes (exact for these temperatures)
        tv = torch.full((B,), temp, dtype=torch.float32, device=dev)
        rowmax = torch.where(torch.isnan(z32), torch.full_like(z32, NEG_INF), z32).max(-1).values
        zt, keep, fcut, on = tpo.truncate(z32, k_rows, p_rows)       # the oracle's truncation: once per temperature
        for mode, (kw, uh, qh) in noises.items():
            if mode != "philox_state":
                tok, fragile = tpo.race_tokens(zt, fcut, qh, REG_THRESHOLD)
                cut_share = max(cut_share, float(fcut.sum()) / float(on.sum()))
                race_share = max(race_share, float((fragile & ~fcut).sum()) / (B * HW))
                changes = (uh < inv_t) & ~un0.flatten()
            dense = step_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, nxt=True, **kw)
            full = step_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, hat=True, **kw)
            uniform[temp, mode] = (dense, full)
            xa, una, hc = dense[0].cpu().flatten(), dense[1].cpu().flatten(), full[2].cpu()
            assert torch.equal(una, un0.flatten() | changes) and torch.equal(xa[~changes], x0.flatten()[~changes])
            assert torch.equal(full[0], dense[0]) and torch.equal(full[1], dense[1])
            assert bool(((hc >= 0) & (hc < K)).all())
            cmp = changes & ~fragile
            stats["wrong"] += int((xa[cmp] != tok[cmp]).sum()) + int((hc[~fragile] != tok[~fragile]).sum())
            stats["next_input"] += int(not torch.equal(dense[3], ops.den_build_input(dense[0], t - 1)))
            # the drawn class was kept (rows without a fragile cut; the NaN row's token 0 is not a draw)
            sure = ~fcut & ~torch.isnan(z32).any(-1)
            stats["outside_kept"] += int((~keep.gather(1, hc[:, None])[:, 0] & sure).sum())
            # exact, on all rows: p = 1e-6 draws a maximum of the row; a row without a comparable ratio gets token 0
            stats["tiny_p_not_max"] += int((z32[tiny].gather(1, hc[tiny][:, None])[:, 0] != rowmax[tiny]).sum())
            stats["degenerate_rows"] += int(hc[5 * HW] != 0) + int(hc[5 * HW + 1] != 0)
            # p off and k off: the `_temps` entry point; p off, k on: the `_topk` entry point -- whole calls and per image
            plain = step_call(ops, dev, ld, x0d, un0d, t, tv, None, None, hat=True, nxt=True, **kw)
            offs = step_call(ops, dev, ld, x0d, un0d, t, tv, k_off, p_off, hat=True, nxt=True, **kw)
            stats["off_differs_temps"] += sum(int(not torch.equal(a, b)) for a, b in zip(plain, offs))
            topk = step_call(ops, dev, ld, x0d, un0d, t, tv, kd, None, hat=True, nxt=True, **kw)
            for poff in (p_off, torch.zeros_like(pd), -p_off, p_off * float("nan"), p_off * 1.5):
                pk = step_call(ops, dev, ld, x0d, un0d, t, tv, kd, poff, hat=True, nxt=True, **kw)
                stats["p_off_differs_topk"] += sum(int(not torch.equal(a, b)) for a, b in zip(topk, pk))
            same = torch.from_numpy(~(p_rows < 1)).view(B, HW)
            stats["p_off_differs_topk"] += int((full[2].cpu().view(B, HW)[same] != topk[2].cpu().view(B, HW)[same]).sum())
            stats["p_off_differs_topk"] += int((dense[0].cpu().view(B, HW)[same] != topk[0].cpu().view(B, HW)[same]).sum())
            # the active list: slot s serves image ACTIVE[s] and reads topp_b[ACTIVE[s]]
            xl, unl, _, _ = step_call(ops, dev, ld, x0d, un0d, t, tv, kd, pd, active=act, **kw)
            for i in range(B):
                wx, wu = (dense[0][i], dense[1][i]) if i in ACTIVE else (x0d[i], un0d[i])
                stats["active_differs"] += int((xl[i] != wx).sum()) + int((unl[i] != wu).sum())
    # a mixed call: temperatures per image with the p and k cycles == the uniform calls, image by image
    tmix = torch.tensor([TEMPS[b % 3] for b in range(B)], dtype=torch.float32)
    for mode in ("injected", "philox"):
        dense = step_call(ops, dev, ld, x0d, un0d, t, tmix.to(dev), kd, pd, nxt=True, **noises[mode][0])
        full = step_call(ops, dev, ld, x0d, un0d, t, tmix.to(dev), kd, pd, hat=True, **noises[mode][0])
        for b in range(B):
            ud, uf = uniform[TEMPS[b % 3], mode]
            stats["mixed_differs"] += int((dense[0][b] != ud[0][b]).sum()) + int((dense[1][b] != ud[1][b]).sum())
            stats["mixed_differs"] += int(not torch.equal(dense[3][b], ud[3][b]))
            stats["mixed_differs"] += int((full[2].view(B, HW)[b] != uf[2].view(B, HW)[b]).sum())
    print(f"topp K={K} {kind}: {stats}, fragile cuts {cut_share:.4f} of the truncated rows, fragile races {race_share:.4f}")
    parity(f"psample_topp_K{K}_{kind}", positions=B * HW, fragile_cut_share=cut_share, fragile_race_share=race_share, **stats)
    assert cut_share <= tpo.FRAGILE_SHARE_CAP and race_share <= FRAGILE_CAP
    assert all(v == 0 for v in stats.values()), stats


# ------------------------------------------------------------------------------------------------- 3. the fused step tail
@pytest.mark.parametrize("L", [7, 8])
@pytest.mark.parametrize("Kc", [100, 128, 256, 512])
def test_den_step_tail_topp_equals_the_three_launch_form(dev, ops, Kc, L):
    """Tokens, ``unmasked``, the fused first layer's spikes and counts of spk_den_step_tail_topp == spk_psample_step_topp on the
    tail's own logits followed by the first-layer launch, bit for bit, dense and on the active list, Philox and injected noise;
    with every p off the launch equals spk_den_step_tail_topk."""
    from spkdiff.ops import IN_TINV
    den = _den_k(Kc, dev)
    assert den.tail_fusable(L, L)
    B, t = 5, 2
    g = torch.Generator().manual_seed(Kc * 10 + L)
    _, x0, un0, u, q = _state(B, Kc, L, g, dev)
    tv = torch.tensor((0.5, 1.0, 2.0, 0.65, 1.0), dtype=torch.float32, device=dev)
    kd = torch.tensor([0, 0, 5, Kc // 2, 0], dtype=torch.int32, device=dev)
    pd = torch.tensor([1e-6, 0.5, 0.9, 0.999, 1.0], dtype=torch.float32, device=dev)
    _, cnt5, _, cnt1, which, _, collapse = den._trunk(ops.den_build_input(x0, t), False)
    assert which == 'mfma-fp6v2' and collapse
    conv6, packed6 = den._conv6_params()
    conv1, bn1 = den.conv1[0], den.conv1[1]
    a1, b1 = bn1.affine_terms()
    c1 = (conv1._spk_params.get(conv1), conv1.bias.detach(), a1, b1)
    act = _active(B, dev)
    with ops.active_set(*act):
        _, cnt5a, _, cnt1a, _, _, _ = den._trunk(ops.den_build_input(x0, t), False)
    bad = {}
    for mode, kw in {"philox": dict(seed=4242, offset=1000 * t), "injected": dict(u=u, q=q)}.items():
        x, un = x0.clone(), un0.clone()
        pre, lg = ops.den_step_tail(cnt5, cnt1, packed6, x, un, t, tv, T=16, K=Kc, conv1=c1, want_logits=True, top_k=kd, top_p=pd, **kw)
        xr, unr = x0.clone(), un0.clone()
        ops.psample_step(lg, xr, unr, t, tv, top_k=kd, top_p=pd, **kw)
        r1 = den.conv1.run(ops.den_build_input(xr, t - 1), IN_TINV, final='ptc', T=16, stateful=False, chunk_out=ops.S32.chunk,
                           want_counts=True)
        n = int((x != xr).sum()) + int((un != unr).sum()) + int(not torch.equal(pre[0], r1['ptc'])) + int(not torch.equal(pre[1], r1['cnt']))
        assert bool((un & ~un0).flatten(1).any(1).all()), "every image has a position that changes"
        # p = 1e-6: the arg max of the tail's own logits at every changed position of image 0
        ch0 = (un & ~un0)[0, 0]
        n += int((x[0, 0][ch0] != (lg[0] / tv[0]).argmax(0)[ch0]).sum())
        # every p off: the `_topk` launch
        xz, unz = x0.clone(), un0.clone()
        prez, lgz = ops.den_step_tail(cnt5, cnt1, packed6, xz, unz, t, tv, T=16, K=Kc, conv1=c1, want_logits=True,
                                      top_k=kd, top_p=torch.ones_like(pd), **kw)
        xt, unt = x0.clone(), un0.clone()
        pret, lgt = ops.den_step_tail(cnt5, cnt1, packed6, xt, unt, t, tv, T=16, K=Kc, conv1=c1, want_logits=True, top_k=kd, **kw)
        n += sum(int(not torch.equal(a, b)) for a, b in ((xz, xt), (unz, unt), (lgz, lgt), (prez[0], pret[0]), (prez[1], pret[1])))
        n += int(not torch.equal(lg, lgt)) + int(torch.equal(x, xt))          # (same logits; the nucleus changes tokens)
        bad[mode] = n
        # the active list: slot s serves image ACTIVE[s]
        xa, una = x0.clone(), un0.clone()
        with ops.active_set(*act):
            prea, _ = ops.den_step_tail(cnt5a, cnt1a, packed6, xa, una, t, tv, T=16, K=Kc, conv1=None, want_logits=True, top_k=kd,
                                        top_p=pd, **kw)
        assert prea is None
        n = 0
        for i in range(B):
            wx, wu = (x[i], un[i]) if i in ACTIVE else (x0[i], un0[i])
            n += int((xa[i] != wx).sum()) + int((una[i] != wu).sum())
        bad["active_" + mode] = n
    parity(f"den_step_tail_topp_K{Kc}_{L}x{L}", mismatches=bad)
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 4. every launch form
PLIST = [0.05, 0.5, 0.5, 1.0, 0.9, 0.999]
KLIST = [0, 4, 0, 0, 16, 200]
TLIST = [0.3, 1.0, 1.0, 0.65, 2.5, 0.8]


def _variants(dev):
    """name -> (top_p, temp, top_k): a number, a list and a device tensor, scalar and per-image temperatures, with and without top_k."""
    pt = torch.tensor(PLIST, dtype=torch.float32, device=dev)
    return {"number_scalar": (0.5, 0.8, None), "list_vector": (PLIST, TLIST, None), "device_scalar_k": (pt, 0.8, KLIST),
            "list_vector_k": (PLIST, TLIST, 4)}


@pytest.mark.parametrize("steps", [12, 49])
def test_sample_top_p_gives_the_same_tokens_in_every_form(dev, steps):
    den, _ = build_den(synth.MNIST, dev)
    B = 6
    bad, want = {}, {}
    tail0 = den.use_step_tail
    try:
        for form in LAUNCH_FORMS:
            den.use_step_tail = form[3]
            for graph in (False, True):
                ab = _form_sampler(den, form, graph)
                ab.n_samples = B
                assert ab.form_for(B, 7, 7) == form[5] and ab._form(B, 7, 7).tail_act == (form[4] and form[1])
                for name, (tp, temp, tk) in _variants(dev).items():
                    torch.manual_seed(6100 + steps)
                    got = ab.sample_top_p(tp, temp, steps, top_k=tk)
                    ref = want.setdefault(name, got)                 # (the first form run: dense, eager)
                    bad[f"{form[0]}_{'graph' if graph else 'eager'}_{name}"] = int((got != ref).sum())
                assert len(ab._graphs) == (1 if graph else 0), "one graph serves every top_p, every top_k and every temperature"
    finally:
        den.use_step_tail = tail0
    for w in want.values():
        assert int(w.max()) < K128 and int(w.min()) >= 0
    # truncation matters, and p = 1 does not: the untruncated image of the list is sample()'s
    plain = _form_sampler(den, LAUNCH_FORMS[0], False)
    plain.n_samples = B
    torch.manual_seed(6100 + steps)
    p = plain.sample(TLIST, steps)
    assert torch.equal(p[3], want["list_vector"][3]) and not torch.equal(p, want["list_vector"])
    assert not torch.equal(want["list_vector_k"], want["list_vector"])
    # top_p = None is sample_top_k, and with all p = 1 the call is sample_top_k's result too
    torch.manual_seed(6100 + steps)
    k_only = plain.sample_top_k(KLIST, 0.8, steps)
    torch.manual_seed(6100 + steps)
    assert torch.equal(plain.sample_top_p(None, 0.8, steps, top_k=KLIST), k_only)
    torch.manual_seed(6100 + steps)
    assert torch.equal(plain.sample_top_p(1.0, 0.8, steps, top_k=KLIST), k_only)
    parity(f"topp_sample_forms_{steps}steps", token_mismatches=bad, tokens=B * 49)
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 5. the host oracle
def test_sample_top_p_vs_host_oracle_per_image(dev):
    """B = 4, 12 steps, p = (0.05, 0.5, 0.9, 1.0) at temperature 1, the captured dense and elimination forms against the host
    oracle (tests/_topp_oracle.run: the reference's loop with the truncation in front of the categorical draw) run once per IMAGE
    on the host's own Philox noise at the image's global index: zero differing tokens, no allowance.  The key is the draw after
    torch.manual_seed(ORACLE_SEED), vetted by tests/test_topp_host.py: on the whole host trajectory no drawn position has a
    fragile cut or a fragile race."""
    den, sd = build_den(synth.MNIST, dev)
    steps, B = 12, 4
    torch.manual_seed(ORACLE_SEED)
    key = sampler(den, True, True, True)._philox_key()
    want = torch.cat([tpo.run(sd, 1, steps, corc.host_philox_noise(key, steps, 1, 7, K128, first=i), ORACLE_PS[i]) for i in range(B)])
    bad = {}
    for form in (LAUNCH_FORMS[1], LAUNCH_FORMS[3]):
        ab = _form_sampler(den, form, True)
        ab.n_samples = B
        torch.manual_seed(ORACLE_SEED)
        got = ab.sample_top_p(list(ORACLE_PS), 1.0, steps).cpu()
        assert int(ab.last_key) == key and len(ab._graphs) == 1
        bad[form[0]] = int((got != want).sum())
    torch.manual_seed(ORACLE_SEED)
    plain = _form_sampler(den, LAUNCH_FORMS[1], False)
    plain.n_samples = B
    assert not torch.equal(plain.sample(1.0, steps).cpu(), want), "the case needs a truncation that changes tokens"
    print(f"top-p vs per-image host oracle: token mismatches {bad} of {want.numel()}")
    parity("topp_sample_vs_host_oracle", token_mismatches=bad, tokens=int(want.numel()))
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 6. a graph input
def test_top_p_is_a_graph_input(dev):
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 6, 12
    ab = sampler(den, True, True, True)
    eager = sampler(den, True, True, False)
    ab.n_samples = eager.n_samples = B
    pa, pb = PLIST, [0.9, 0.1, 1.0, 0.3, 0.3, 0.75]
    out = []
    for seed, pv, kv in ((1, pa, None), (2, pb, KLIST), (1, pa, None)):
        torch.manual_seed(seed)
        got = ab.sample_top_p(pv, TLIST, steps, top_k=kv)
        torch.manual_seed(seed)
        out.append((got, int((got != eager.sample_top_p(pv, TLIST, steps, top_k=kv)).sum())))
    assert len(ab._graphs) == 1, "one graph serves every top_p vector"
    torch.manual_seed(1)
    other = ab.sample_top_p(pb, TLIST, steps)                        # same key and temperatures, another p: other tokens
    assert torch.equal(out[0][0], out[2][0]) and not torch.equal(other, out[0][0]) and len(ab._graphs) == 1
    g = next(iter(ab._graphs.values()))
    assert g.topp is not None and g.topp.tolist() == torch.tensor(pb, dtype=torch.float32).tolist() and g.topk.tolist() == [0] * B
    assert "top-p" in next(iter(ab._graphs))
    # a top-k call adds its own graph and is today's result
    torch.manual_seed(3)
    s1 = ab.sample_top_k(KLIST, 0.65, steps)
    assert len(ab._graphs) == 2 and sum(gr.topp is not None for gr in ab._graphs.values()) == 1
    torch.manual_seed(3)
    plain_bad = int((s1 != eager.sample_top_k(KLIST, 0.65, steps)).sum())
    parity("topp_graph_input", token_mismatches_vs_eager=[o[1] for o in out], topk_vs_eager=plain_bad, graphs=len(ab._graphs))
    assert all(o[1] == 0 for o in out) and plain_bad == 0


# ------------------------------------------------------------------------------------------------- 7. shards and splits
def test_sample_top_p_on_two_shards_equals_the_whole_job(dev):
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 6, 12
    whole = sampler(den, True, True, True)
    whole.n_samples = B
    torch.manual_seed(31)
    want = whole.sample_top_p(PLIST, TLIST, steps, top_k=KLIST)
    bad = {}
    for graph in (False, True):
        parts = []
        for lo, hi in ((0, 2), (2, 6)):
            sh = sampler(den, True, True, graph).set_shard(lo, hi - lo)
            torch.manual_seed(31)
            parts.append(sh.sample_top_p(PLIST[lo:hi], TLIST[lo:hi], steps, top_k=KLIST[lo:hi]))
        bad["graph" if graph else "eager"] = int((torch.cat(parts) != want).sum())
    parity("topp_shards", token_mismatches=bad, tokens=int(want.numel()))
    assert all(v == 0 for v in bad.values()), bad


def test_nucleus_sweep_does_not_depend_on_batch_or_split(dev):
    from spkdiff import dist as sdist
    from spkdiff.evaluate import temperature_sweep_range, temperature_sweep_top_p
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    temps, pv, n, steps = (0.3, 1.0, 0.65), [0.5, 1.0, 0.9], 5, 12
    ab = sampler(den, True, True, True)
    ab.set_shard(3, 7)
    res = {}
    for name, batch in (("batch4", 4), ("batch256", 256)):
        torch.manual_seed(910)
        res[name] = temperature_sweep_top_p(model, ab, temps, n, pv, sample_steps=steps, batch=batch)
        assert (ab.n_samples, ab.global_first) == (7, 3), "the sampler's shard is restored"
    u8, tok = res["batch4"]
    assert u8.shape == (3, n, 1, 28, 28) and tok.shape == (3, n, 7, 7)
    halves = []
    for rank in range(2):
        lo, hi = sdist.shard_range(3 * n, rank, 2)
        torch.manual_seed(910)
        halves.append(temperature_sweep_range(model, sampler(den, True, True, True), temps, n, lo, hi, sample_steps=steps, batch=4, top_p=pv))
    split = (torch.cat([h[0] for h in halves]).reshape(u8.shape), torch.cat([h[1] for h in halves]).reshape(tok.shape))
    # group g is sample_top_p(pv[g], temps[g]) on the group's shard; the untruncated group is sample()'s
    s_tok = []
    for gi, (t, p) in enumerate(zip(temps, pv)):
        sh = sampler(den, True, True, False).set_shard(gi * n, n)
        torch.manual_seed(910)
        s_tok.append((sh.sample(t, steps) if p == 1.0 else sh.sample_top_p(p, t, steps)).reshape(n, 7, 7))
    bad = dict(batch256_tokens=int((res["batch256"][1] != tok).sum()), batch256_pixels=int((res["batch256"][0] != u8).sum()),
               split_tokens=int((split[1] != tok).sum()), split_pixels=int((split[0] != u8).sum()),
               per_group_tokens=int((torch.stack(s_tok) != tok).sum()))
    torch.manual_seed(910)
    bad["sharded_pixels"] = int((sdist.temperature_sweep_sharded(model, ab, temps, n, sample_steps=steps, batch=4, top_p=pv) != u8).sum())
    parity("topp_temperature_sweep", **bad, tokens=int(tok.numel()))
    assert all(v == 0 for v in bad.values()), bad


def test_complete_images_top_p(dev):
    from spkdiff.complete import complete_images, complete_images_top_p
    from spkdiff.dist import complete_images_sharded
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 8, 12
    pv = [0.05, 0.05, 0.5, 0.5, 1.0, 0.9, 0.25, 0.25]
    images = (synth.stroke_images(B, seed=77, img=28, channels=1) - 0.5).to(dev)
    keep = torch.ones(B, 28, 28, dtype=torch.bool)
    keep[:, 14:] = False
    keep[1::2, :, 10:17] = False
    keep = keep.to(dev)
    ab = sampler(den, True, True, True)
    torch.manual_seed(2026)
    res = complete_images_top_p(model, ab, images, keep, pv, temp=0.9, sample_steps=steps)
    codes = model.encode_images(images)
    assert 0 < int(res.known.sum()) < res.known.numel()
    kept_bad = int((res.tokens[res.known] != codes[res.known]).sum())
    torch.manual_seed(2026)
    plain = complete_images(model, ab, images, keep, temp=0.9, sample_steps=steps)
    torch.manual_seed(2026)
    ones = complete_images_top_p(model, ab, images, keep, [1.0] * B, temp=0.9, sample_steps=steps)
    one_bad = int((ones.tokens != plain.tokens).sum()) + int((ones.images_u8 != plain.images_u8).sum())
    torch.manual_seed(2026)
    shard_bad = int((complete_images_sharded(model, ab, images, keep, temp=0.9, sample_steps=steps, top_p=pv) != res.images_u8).sum())
    parity("complete_images_top_p", known_changed=kept_bad, all_one_vs_plain=one_bad, sharded_pixels=shard_bad)
    assert kept_bad == 0 and one_bad == 0 and shard_bad == 0 and int(res.tokens.max()) < K128
    assert torch.equal(res.tokens[4], plain.tokens[4]) and not torch.equal(res.tokens, plain.tokens)


# ------------------------------------------------------------------------------------------------- 8. what the wrappers refuse
def test_wrappers_refuse_a_bad_top_p(dev, ops):
    B, h = 5, 7
    g = torch.Generator().manual_seed(1)
    logits, x0, un0, _, _ = _state(B, K128, h, g, dev)
    good = torch.full((B,), 0.5, device=dev)
    bads = (torch.ones(4, device=dev), torch.ones(B, dtype=torch.float64, device=dev), torch.ones(B, dtype=torch.int32, device=dev),
            torch.ones(B), torch.ones(B, 2, device=dev)[:, 0], torch.ones(1, B, device=dev), [0.5] * B, 0.5)
    for bad in bads:
        x, un = x0.clone(), un0.clone()
        with pytest.raises(ValueError, match="top_p must be"):
            ops.psample_step(logits, x, un, 2, 1.0, top_p=bad)
        torch.cuda.synchronize()
        assert torch.equal(x, x0) and torch.equal(un, un0), "a refused call launched nothing"
    # a scalar temperature is broadcast and a missing top_k is zeros: the call equals the one with the vectors
    a, b = x0.clone(), x0.clone()
    ops.psample_step(logits, a, un0.clone(), 2, 0.7, seed=3, top_p=good)
    ops.psample_step(logits, b, un0.clone(), 2, torch.full((B,), 0.7, device=dev), seed=3, top_p=good,
                     top_k=torch.zeros(B, dtype=torch.int32, device=dev))
    assert torch.equal(a, b)
    den, _ = build_den(synth.MNIST, dev)
    ab = sampler(den, True, True, True)
    ab.n_samples = B
    torch.manual_seed(5)
    state = torch.get_rng_state()
    for bad in (torch.ones(B, dtype=torch.float64, device=dev), torch.ones(4, device=dev), torch.ones(B, dtype=torch.int32, device=dev),
                torch.ones(B, 1, device=dev)):
        with pytest.raises(ValueError, match="top_p"):
            ab.sample_top_p(bad, 1.0, 3)
    assert torch.equal(torch.get_rng_state(), state) and len(ab._graphs) == 0
