"""GPU tests of top-k truncated sampling (run with ``-m gpu`` on an MI355X): ``spk_psample_step_topk`` against
the fp64 oracle of tests/_topk_oracle.py and its exact properties, ``spk_den_step_tail_topk`` against the three-launch form bit
for bit, ``AbsorbingDiffusion.sample_top_k`` in every launch form, eager and captured, against the host oracle, as a graph input,
across shards and splits, and the wrappers' argument checks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _completion_oracle as corc           # noqa: E402
import _topk_oracle as tko                  # noqa: E402
from parity_report import record as parity  # noqa: E402
from spkdiff import synth                  # noqa: E402
from test_gpu_completion import K as K128, build_den, build_vae, sampler      # noqa: E402  (the helpers, not the tests)
from test_gpu_sampler_noise_shapes import FRAGILE_CAP, REG_MEASURED, REG_THRESHOLD, rows_of      # noqa: E402
from test_gpu_temps import ACTIVE, LAUNCH_FORMS, _active, _den_k, _form_sampler, _state      # noqa: E402

NEG_INF = float("-inf")
TEMPS = (0.5, 1.0, 2.0)
ORACLE_SEED = 2718                                   # see test_sample_top_k_vs_host_oracle_per_image


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def k_cycle(K):
    return [1, 2, 5, max(1, K // 2), max(1, K - 1), K, 0]


def topk_inputs(K, kind):
    """HW = 49, B = 21 (11 at K = 2048), seed 4000 + K: logits of the three kinds, then q, u, the state."""
    B = 11 if K == 2048 else 21
    g = torch.Generator().manual_seed(4000 + K)
    r = torch.randn(B, K, 7, 7, generator=g)
    hole = torch.rand(B, K, 7, 7, generator=g) < 0.3
    hole[:, K // 2] = False                                      # (every position keeps a finite class)
    if kind == "randn":
        logits = r * 3
    elif kind == "neg_inf":
        logits = r * 3
        logits[hole] = NEG_INF
    else:
        logits = torch.round(2 * r * 3) / 2                      # "ties": half-integer logits, many rows tie at tau
    q = torch.empty(B * 49, K).exponential_(1, generator=g)
    u = torch.rand(B * 49, generator=g)
    un0 = torch.rand(B, 1, 7, 7, generator=g) < 0.4
    x0 = torch.randint(0, K, (B, 1, 7, 7), generator=g)
    x0[~un0] = K
    return logits, q, u, x0, un0


def step_call(ops, dev, logits, x0, un0, t, temp, top_k, hat=False, nxt=False, active=None, **noise):
    """One token update on copies of the state -> (x_t, unmasked, x0_hat or None, next_input or None)."""
    B, K, h, w = logits.shape
    x, un = x0.clone(), un0.clone()
    x0h = torch.full((B * h * w,), -5, dtype=torch.int64, device=dev) if hat else None
    ni = torch.full((B, 2, h, w), float("nan"), device=dev) if nxt else None
    kw = dict(noise, **({} if top_k is None else {"top_k": top_k}))
    if active is not None:
        slots = torch.full_like(logits, float("nan"))            # slots beyond the list hold NaN and must never be read
        slots[:len(ACTIVE)] = logits[list(ACTIVE)]
        with ops.active_set(*active):
            ops.psample_step(slots, x, un, t, temp, **kw)
    else:
        ops.psample_step(logits, x, un, t, temp, x0_hat=x0h, next_input=ni, **kw)
    return x, un, x0h, ni


# ------------------------------------------------------------------------------------------------- 1 + 2. the sampling kernel
K_TOPK = [2, 63, 64, 65, 128, 256, 257, 512, 513, 2048]      # both sides of the 256 / 512 classes-per-lane switches, ragged last lanes


@pytest.mark.parametrize("kind", ["randn", "neg_inf", "ties"])
@pytest.mark.parametrize("K", K_TOPK)
def test_psample_step_topk_vs_fp64_oracle_and_exact_properties(dev, ops, K, kind):
    """One call per uniform temperature 0.5 / 1 / 2 and form (dense with next_input, x0_hat, the active list; injected noise,
    Philox, philox_state) against the fp64 race on the row truncated in fp32 (tests/_topk_oracle.oracle_tokens): changing,
    non-fragile positions token for token, x0_hat at every non-fragile position (REG_THRESHOLD; at most FRAGILE_CAP of the
    positions fragile; the fp32 reference expression re-measured against REG_MEASURED).  Then, with no fragile allowance: every
    x0_hat lies in the oracle's kept set, k = 1 images get a row maximum under both noise modes, k in {K, 0} images and an all-zero
    call equal spk_psample_step_temps bit for bit, and a call with mixed temperatures equals the uniform calls image by image."""
    logits, q, u, x0, un0 = topk_inputs(K, kind)
    B, HW, t = logits.shape[0], 49, 3
    ks = torch.tensor([k_cycle(K)[b % 7] for b in range(B)], dtype=torch.int32)
    k_rows = ks.long().repeat_interleave(HW)
    ld, x0d, un0d, kd = logits.to(dev), x0.to(dev), un0.to(dev), ks.to(dev)
    seed, off = 0x1234_5678_9ABC, 5 * (1 << 40) + 11 * HW * K
    state = torch.tensor([seed, 1 << 33], dtype=torch.int64, device=dev)
    up, qp = ops.philox_noise(seed, off, B, HW, K, dev)
    noises = {"injected": (dict(u=u.to(dev), q=q.to(dev)), u, q),
              "philox": (dict(seed=seed, offset=off), up.cpu(), qp.cpu()),
              "philox_state": (dict(seed=99, offset=off - (1 << 33), philox_state=state), up.cpu(), qp.cpu())}
    act = _active(B, dev)
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(t), dtype=torch.float32)
    stats = dict(wrong=0, outside_kept=0, k1_not_max=0, untruncated_differs=0, active_differs=0, mixed_differs=0, next_input=0)
    fragile_n, measured, more_than_k = 0, 0.0, []
    uniform = {}
    for temp in TEMPS:
        z32 = rows_of(logits) / temp                                 # the fp32 division the kernel makes (exact for these temperatures)
        tv = torch.full((B,), temp, dtype=torch.float32, device=dev)
        trunc_rows = (k_rows > 0) & (k_rows < K)
        for mode, (kw, uh, qh) in noises.items():
            if mode != "philox_state":
                tok, fragile, keep = tko.oracle_tokens(z32, k_rows, qh, REG_THRESHOLD)
                fragile_n = max(fragile_n, int(fragile.sum()))
                measured = max(measured, tko.measure_fp32_error(z32, k_rows, qh))
                changes = (uh < inv_t) & ~un0.flatten()
            dense = step_call(ops, dev, ld, x0d, un0d, t, tv, kd, nxt=True, **kw)
            full = step_call(ops, dev, ld, x0d, un0d, t, tv, kd, hat=True, **kw)
            uniform[temp, mode] = (dense, full)
            xa, una, hc = dense[0].cpu().flatten(), dense[1].cpu().flatten(), full[2].cpu()
            assert torch.equal(una, un0.flatten() | changes) and torch.equal(xa[~changes], x0.flatten()[~changes])
            assert torch.equal(full[0], dense[0]) and torch.equal(full[1], dense[1])
            cmp = changes & ~fragile
            stats["wrong"] += int((xa[cmp] != tok[cmp]).sum()) + int((hc[~fragile] != tok[~fragile]).sum())
            stats["next_input"] += int(not torch.equal(dense[3], ops.den_build_input(dense[0], t - 1)))
            # exact: the drawn class was kept; k = 1 draws a maximum of the row
            assert bool(((hc >= 0) & (hc < K)).all())
            stats["outside_kept"] += int((~keep.gather(1, hc[:, None])[:, 0]).sum())
            k1 = k_rows == 1
            stats["k1_not_max"] += int((z32[k1].gather(1, hc[k1][:, None])[:, 0] != z32[k1].max(-1).values).sum())
            # k in {K, 0}: the `_temps` entry point, bit for bit -- per image of this call and as a whole call of zeros
            plain = step_call(ops, dev, ld, x0d, un0d, t, tv, None, hat=True, nxt=True, **kw)
            zeros = step_call(ops, dev, ld, x0d, un0d, t, tv, torch.zeros_like(kd), hat=True, nxt=True, **kw)
            stats["untruncated_differs"] += sum(int(not torch.equal(a, b)) for a, b in zip(plain, zeros))
            same = (~trunc_rows).view(B, HW)
            stats["untruncated_differs"] += int((full[2].cpu().view(B, HW)[same] != plain[2].cpu().view(B, HW)[same]).sum())
            stats["untruncated_differs"] += int((dense[0].cpu().view(B, HW)[same] != plain[0].cpu().view(B, HW)[same]).sum())
            # the active list: slot s serves image ACTIVE[s] and reads topk_b[ACTIVE[s]]
            xl, unl, _, _ = step_call(ops, dev, ld, x0d, un0d, t, tv, kd, active=act, **kw)
            for i in range(B):
                wx, wu = (dense[0][i], dense[1][i]) if i in ACTIVE else (x0d[i], un0d[i])
                stats["active_differs"] += int((xl[i] != wx).sum()) + int((unl[i] != wu).sum())
        if kind == "ties":
            kept_n = tko.oracle_tokens(z32, k_rows, q, REG_THRESHOLD)[2][trunc_rows].sum(1)
            more_than_k.append(float((kept_n > k_rows[trunc_rows]).float().mean()))
    # a mixed call: temperatures from {0.5, 1, 2} per image with the k cycle == the uniform calls, image by image
    tmix = torch.tensor([TEMPS[b % 3] for b in range(B)], dtype=torch.float32)
    for mode in ("injected", "philox"):
        dense = step_call(ops, dev, ld, x0d, un0d, t, tmix.to(dev), kd, nxt=True, **noises[mode][0])
        full = step_call(ops, dev, ld, x0d, un0d, t, tmix.to(dev), kd, hat=True, **noises[mode][0])
        for b in range(B):
            ud, uf = uniform[TEMPS[b % 3], mode]
            stats["mixed_differs"] += int((dense[0][b] != ud[0][b]).sum()) + int((dense[1][b] != ud[1][b]).sum())
            stats["mixed_differs"] += int(not torch.equal(dense[3][b], ud[3][b]))
            stats["mixed_differs"] += int((full[2].view(B, HW)[b] != uf[2].view(B, HW)[b]).sum())
    share = fragile_n / (B * HW)
    print(f"topk K={K} {kind}: {stats}, fragile {fragile_n}, fp32 reference error {measured:.3e}, rows keeping more than k {more_than_k}")
    parity(f"psample_topk_K{K}_{kind}", positions=B * HW, fragile=fragile_n, fp32_reference_error_measured=measured,
           rows_keeping_more_than_k=more_than_k, **stats)
    assert measured <= REG_MEASURED, f"fp32 reference error {measured} above the value the threshold was derived from"
    assert share <= FRAGILE_CAP, f"{fragile_n} of {B * HW} positions fragile"
    assert all(v == 0 for v in stats.values()), stats
    if kind == "ties":
        assert min(more_than_k) > 0, "the case needs rows that tie at tau"


def test_psample_step_topk_one_class(dev, ops):
    """K = 1: no k truncates (k >= K or k <= 0) -- the `_temps` entry point bit for bit."""
    g = torch.Generator().manual_seed(1)
    logits, x0, un0, u, q = _state(7, 1, 7, g, dev)
    tv = torch.full((7,), 0.5, device=dev)
    kd = torch.tensor(k_cycle(1), dtype=torch.int32, device=dev)
    bad = 0
    for kw in (dict(u=u, q=q), dict(seed=5, offset=1 << 40)):
        a = step_call(ops, dev, logits, x0, un0, 2, tv, kd, hat=True, nxt=True, **kw)
        b = step_call(ops, dev, logits, x0, un0, 2, tv, None, hat=True, nxt=True, **kw)
        bad += sum(int(not torch.equal(p, r)) for p, r in zip(a, b))
    parity("psample_topk_K1", differing=bad)
    assert bad == 0 and not bool(a[1].all()) and bool((a[0][a[1]] == 0).all())


# ------------------------------------------------------------------------------------------------- 3. the fused step tail
@pytest.mark.parametrize("L", [7, 8])
@pytest.mark.parametrize("Kc", [100, 128, 256, 512])
def test_den_step_tail_topk_equals_the_three_launch_form(dev, ops, Kc, L):
    """Tokens, ``unmasked``, the fused first layer's spikes and counts of spk_den_step_tail_topk == spk_psample_step_topk on the
    tail's own logits followed by the first-layer launch, bit for bit, dense and on the active list, Philox and injected noise;
    with every k = 0 the launch equals spk_den_step_tail_temps."""
    from spkdiff.ops import IN_TINV
    den = _den_k(Kc, dev)
    assert den.tail_fusable(L, L)
    B, t = 5, 2
    g = torch.Generator().manual_seed(Kc * 10 + L)
    _, x0, un0, u, q = _state(B, Kc, L, g, dev)
    tv = torch.tensor((0.5, 1.0, 2.0, 0.65, 1.0), dtype=torch.float32, device=dev)
    kd = torch.tensor([1, 2, 5, Kc // 2, 0], dtype=torch.int32, device=dev)
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
        pre, lg = ops.den_step_tail(cnt5, cnt1, packed6, x, un, t, tv, T=16, K=Kc, conv1=c1, want_logits=True, top_k=kd, **kw)
        xr, unr = x0.clone(), un0.clone()
        ops.psample_step(lg, xr, unr, t, tv, top_k=kd, **kw)
        r1 = den.conv1.run(ops.den_build_input(xr, t - 1), IN_TINV, final='ptc', T=16, stateful=False, chunk_out=ops.S32.chunk,
                           want_counts=True)
        n = int((x != xr).sum()) + int((un != unr).sum()) + int(not torch.equal(pre[0], r1['ptc'])) + int(not torch.equal(pre[1], r1['cnt']))
        assert bool((un & ~un0).flatten(1).any(1).all()), "every image has a position that changes"
        # k = 1: the arg max of the tail's own logits at every changed position of image 0
        ch0 = (un & ~un0)[0, 0]
        n += int((x[0, 0][ch0] != (lg[0] / tv[0]).argmax(0)[ch0]).sum())
        # every k = 0: the `_temps` launch
        xz, unz = x0.clone(), un0.clone()
        prez, lgz = ops.den_step_tail(cnt5, cnt1, packed6, xz, unz, t, tv, T=16, K=Kc, conv1=c1, want_logits=True,
                                      top_k=torch.zeros_like(kd), **kw)
        xt, unt = x0.clone(), un0.clone()
        pret, lgt = ops.den_step_tail(cnt5, cnt1, packed6, xt, unt, t, tv, T=16, K=Kc, conv1=c1, want_logits=True, **kw)
        n += sum(int(not torch.equal(a, b)) for a, b in ((xz, xt), (unz, unt), (lgz, lgt), (prez[0], pret[0]), (prez[1], pret[1])))
        n += int(not torch.equal(lg, lgt)) + int(torch.equal(x, xt))          # (same logits; truncation changes tokens)
        bad[mode] = n
        # the active list: slot s serves image ACTIVE[s]
        xa, una = x0.clone(), un0.clone()
        with ops.active_set(*act):
            prea, _ = ops.den_step_tail(cnt5a, cnt1a, packed6, xa, una, t, tv, T=16, K=Kc, conv1=None, want_logits=True, top_k=kd, **kw)
        assert prea is None
        n = 0
        for i in range(B):
            wx, wu = (x[i], un[i]) if i in ACTIVE else (x0[i], un0[i])
            n += int((xa[i] != wx).sum()) + int((una[i] != wu).sum())
        bad["active_" + mode] = n
    parity(f"den_step_tail_topk_K{Kc}_{L}x{L}", mismatches=bad)
    assert all(v == 0 for v in bad.values()), bad


@pytest.mark.parametrize("what", ["nan", "neg_inf"])
def test_step_tail_topk_rows_without_a_comparable_ratio(dev, ops, what):
    """conv6's bias NaN for one class (a NaN is never replaced: the row has no comparable ratio) or -inf for all (fewer than k
    entries above -inf: nothing is dropped): every changing position gets token 0, as without truncation."""
    from snn_model.vq_diffusion import DummyModel, functional
    Kc, L, B = 17, 7, 5
    torch.manual_seed(Kc)
    den = DummyModel(1, Kc).to(dev)
    functional.set_step_mode(net=den, step_mode='m')
    with torch.no_grad():
        if what == "nan":
            den.conv6[0].bias[Kc // 2] = float("nan")
        else:
            den.conv6[0].bias.fill_(NEG_INF)
    den.eval()
    g = torch.Generator().manual_seed(Kc + L)
    _, x0, un0, _, _ = _state(B, Kc, L, g, dev)
    _, cnt5, _, cnt1, _, _, _ = den._trunk(ops.den_build_input(x0, 1), False)
    _, packed6 = den._conv6_params()
    tv = torch.ones(B, device=dev)
    kd = torch.tensor([1, 2, 5, 8, 16], dtype=torch.int32, device=dev)
    xa, una = x0.clone(), un0.clone()
    _, lg = ops.den_step_tail(cnt5, cnt1, packed6, xa, una, 1, tv, T=16, K=Kc, seed=5, offset=1 << 40, conv1=None, want_logits=True, top_k=kd)
    lr = rows_of(lg.cpu())
    assert bool(torch.isnan(lr[:, Kc // 2]).all()) if what == "nan" else bool((lr == NEG_INF).all())
    assert bool(una.all()) and bool((xa[~un0] == 0).all()) and torch.equal(xa[un0], x0[un0])
    xb, unb = x0.clone(), un0.clone()
    ops.psample_step(lg, xb, unb, 1, tv, seed=5, offset=1 << 40, top_k=kd)
    assert torch.equal(xb, xa) and torch.equal(unb, una)
    parity(f"step_tail_topk_degenerate_rows_{what}", tokens_not_zero=int((xa[~un0] != 0).sum()))


# ------------------------------------------------------------------------------------------------- 4. every launch form
KLIST = [1, 4, 4, 0, 16, 200]
TLIST = [0.3, 1.0, 1.0, 0.65, 2.5, 0.8]


def _variants(dev):
    """name -> (top_k, temp): an int, a list and a device tensor, with a scalar and with a per-image temperature."""
    return {"int_scalar": (4, 0.8), "list_vector": (KLIST, TLIST), "device_scalar": (torch.tensor(KLIST, dtype=torch.int32, device=dev), 0.8),
            "device_vector": (torch.tensor(KLIST, dtype=torch.int32, device=dev), torch.tensor(TLIST, dtype=torch.float32, device=dev))}


@pytest.mark.parametrize("steps", [12, 49])
def test_sample_top_k_gives_the_same_tokens_in_every_form(dev, steps):
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
                for name, (tk, temp) in _variants(dev).items():
                    torch.manual_seed(5100 + steps)
                    got = ab.sample_top_k(tk, temp, steps)
                    ref = want.setdefault(name, got)                 # (the first form run: dense, eager)
                    bad[f"{form[0]}_{'graph' if graph else 'eager'}_{name}"] = int((got != ref).sum())
                assert len(ab._graphs) == (1 if graph else 0), "one graph serves every top_k and every temperature"
    finally:
        den.use_step_tail = tail0
    for w in want.values():
        assert int(w.max()) < K128 and int(w.min()) >= 0
    # truncation matters, and k = 0 / k >= K do not: the untruncated images of the list are sample()'s
    plain = _form_sampler(den, LAUNCH_FORMS[0], False)
    plain.n_samples = B
    torch.manual_seed(5100 + steps)
    p = plain.sample(TLIST, steps)
    assert torch.equal(p[3], want["list_vector"][3]) and torch.equal(p[5], want["list_vector"][5]) and not torch.equal(p, want["list_vector"])
    assert torch.equal(want["device_vector"], want["list_vector"]) and not torch.equal(want["device_scalar"], want["int_scalar"])
    parity(f"topk_sample_forms_{steps}steps", token_mismatches=bad, tokens=B * 49)
    assert all(v == 0 for v in bad.values()), bad


def test_sample_top_k_on_the_8x8_model(dev):
    den, _ = build_den(synth.CIFAR, dev)
    B, steps = 6, 12
    got = {}
    for form, graph in ((LAUNCH_FORMS[1], True), (LAUNCH_FORMS[2], False)):
        ab = _form_sampler(den, form, graph, latent=8)
        ab.n_samples = B
        assert ab.form_for(B, 8, 8) == form[5]
        torch.manual_seed(89)
        got[form[0]] = ab.sample_top_k(KLIST, TLIST, steps)
    a, b = got.values()
    bad = int((a != b).sum())
    parity("topk_sample_8x8", token_mismatches=bad, tokens=int(a.numel()))
    assert bad == 0 and a.shape == (B, 1, 8, 8)


# ------------------------------------------------------------------------------------------------- 5. the host oracle
def test_sample_top_k_vs_host_oracle_per_image(dev):
    """B = 4, 12 steps, k = (1, 3, 8, 0) at temperature 1, the captured dense and elimination forms against the host oracle
    (tests/_topk_oracle.run: the reference's loop with the truncation line in front of the categorical draw) run once per IMAGE on
    the host's own Philox noise at the image's global index: zero differing tokens, no allowance for near-ties.  The key is the
    draw after torch.manual_seed(ORACLE_SEED = 2718), chosen on the host: for this job (synthetic MNIST denoiser) the fp32 oracle
    and the exact-convolution oracle give the same tokens for every image, and over the whole oracle run the two largest fp64
    ratios of every drawn position are further apart than REG_THRESHOLD relative to the larger (no fragile draw), so equality is
    a fair demand."""
    den, sd = build_den(synth.MNIST, dev)
    ks, steps, B = (1, 3, 8, 0), 12, 4
    torch.manual_seed(ORACLE_SEED)
    key = sampler(den, True, True, True)._philox_key()
    want = torch.cat([tko.run(sd, 1, steps, corc.host_philox_noise(key, steps, 1, 7, K128, first=i), ks[i]) for i in range(B)])
    bad = {}
    for form in (LAUNCH_FORMS[1], LAUNCH_FORMS[3]):
        ab = _form_sampler(den, form, True)
        ab.n_samples = B
        torch.manual_seed(ORACLE_SEED)
        got = ab.sample_top_k(list(ks), 1.0, steps).cpu()
        assert int(ab.last_key) == key and len(ab._graphs) == 1
        bad[form[0]] = int((got != want).sum())
    print(f"top-k vs per-image host oracle: token mismatches {bad} of {want.numel()}")
    parity("topk_sample_vs_host_oracle", token_mismatches=bad, tokens=int(want.numel()))
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 6. a graph input
def test_top_k_is_a_graph_input(dev):
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 6, 12
    ab = sampler(den, True, True, True)
    eager = sampler(den, True, True, False)
    ab.n_samples = eager.n_samples = B
    ka, kb = KLIST, [8, 1, 0, 2, 2, 64]
    ta, tb = TLIST, [1.0, 0.65, 0.001, 0.3, 2.0, 0.3]
    out = []
    for seed, kv, tv in ((1, ka, ta), (2, kb, tb), (1, ka, ta)):
        torch.manual_seed(seed)
        got = ab.sample_top_k(kv, tv, steps)
        torch.manual_seed(seed)
        out.append((got, int((got != eager.sample_top_k(kv, tv, steps)).sum())))
    assert len(ab._graphs) == 1, "one graph serves every top_k vector and every temperature vector"
    torch.manual_seed(1)
    other = ab.sample_top_k(kb, ta, steps)                           # same key and temperatures, another k: other tokens
    assert torch.equal(out[0][0], out[2][0]) and not torch.equal(other, out[0][0]) and len(ab._graphs) == 1
    g = next(iter(ab._graphs.values()))
    assert g.topk is not None and g.topk.tolist() == kb and g.temps.tolist() == torch.tensor(ta, dtype=torch.float32).tolist()
    assert "top-k" in next(iter(ab._graphs))
    # an untruncated call adds its own graph and is today's result
    torch.manual_seed(3)
    s1 = ab.sample(0.65, steps)
    assert len(ab._graphs) == 2 and sum(gr.topk is not None for gr in ab._graphs.values()) == 1
    torch.manual_seed(3)
    plain_bad = int((s1 != eager.sample(0.65, steps)).sum())
    torch.manual_seed(3)
    assert torch.equal(s1, ab.sample_top_k(None, 0.65, steps)) and len(ab._graphs) == 2
    parity("topk_graph_input", token_mismatches_vs_eager=[o[1] for o in out], untruncated_vs_eager=plain_bad, graphs=len(ab._graphs))
    assert all(o[1] == 0 for o in out) and plain_bad == 0


# ------------------------------------------------------------------------------------------------- 7. shards and splits
def test_sample_top_k_on_two_shards_equals_the_whole_job(dev):
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 6, 12
    whole = sampler(den, True, True, True)
    whole.n_samples = B
    torch.manual_seed(31)
    want = whole.sample_top_k(KLIST, TLIST, steps)
    bad = {}
    for graph in (False, True):
        parts = []
        for lo, hi in ((0, 2), (2, 6)):
            sh = sampler(den, True, True, graph).set_shard(lo, hi - lo)
            torch.manual_seed(31)
            parts.append(sh.sample_top_k(KLIST[lo:hi], TLIST[lo:hi], steps))
        bad["graph" if graph else "eager"] = int((torch.cat(parts) != want).sum())
    parity("topk_shards", token_mismatches=bad, tokens=int(want.numel()))
    assert all(v == 0 for v in bad.values()), bad


def test_truncated_sweep_does_not_depend_on_batch_or_split(dev):
    from spkdiff import dist as sdist
    from spkdiff.evaluate import temperature_sweep_range, temperature_sweep_top_k
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    temps, ks, n, steps = (0.3, 1.0, 0.65), [1, 0, 16], 5, 12
    ab = sampler(den, True, True, True)
    ab.set_shard(3, 7)
    res = {}
    for name, batch in (("batch4", 4), ("batch256", 256)):
        torch.manual_seed(910)
        res[name] = temperature_sweep_top_k(model, ab, temps, n, ks, sample_steps=steps, batch=batch)
        assert (ab.n_samples, ab.global_first) == (7, 3), "the sampler's shard is restored"
    u8, tok = res["batch4"]
    assert u8.shape == (3, n, 1, 28, 28) and tok.shape == (3, n, 7, 7)
    halves = []
    for rank in range(2):
        lo, hi = sdist.shard_range(3 * n, rank, 2)
        torch.manual_seed(910)
        halves.append(temperature_sweep_range(model, sampler(den, True, True, True), temps, n, lo, hi, sample_steps=steps, batch=4, top_k=ks))
    split = (torch.cat([h[0] for h in halves]).reshape(u8.shape), torch.cat([h[1] for h in halves]).reshape(tok.shape))
    # group g is sample_top_k(ks[g], temps[g]) on the group's shard; the untruncated group is sample()'s
    s_tok = []
    for gi, (t, k) in enumerate(zip(temps, ks)):
        sh = sampler(den, True, True, False).set_shard(gi * n, n)
        torch.manual_seed(910)
        s_tok.append((sh.sample(t, steps) if k == 0 else sh.sample_top_k(k, t, steps)).reshape(n, 7, 7))
    bad = dict(batch256_tokens=int((res["batch256"][1] != tok).sum()), batch256_pixels=int((res["batch256"][0] != u8).sum()),
               split_tokens=int((split[1] != tok).sum()), split_pixels=int((split[0] != u8).sum()),
               per_group_tokens=int((torch.stack(s_tok) != tok).sum()))
    torch.manual_seed(910)
    bad["sharded_pixels"] = int((sdist.temperature_sweep_sharded(model, ab, temps, n, sample_steps=steps, batch=4, top_k=ks) != u8).sum())
    parity("topk_temperature_sweep", **bad, tokens=int(tok.numel()))
    assert all(v == 0 for v in bad.values()), bad


def test_complete_images_top_k(dev):
    from spkdiff.complete import complete_images, complete_images_top_k
    from spkdiff.dist import complete_images_sharded
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 8, 12
    ks = [1, 1, 4, 4, 0, 16, 2, 2]
    images = (synth.stroke_images(B, seed=77, img=28, channels=1) - 0.5).to(dev)
    keep = torch.ones(B, 28, 28, dtype=torch.bool)
    keep[:, 14:] = False
    keep[1::2, :, 10:17] = False
    keep = keep.to(dev)
    ab = sampler(den, True, True, True)
    torch.manual_seed(2026)
    res = complete_images_top_k(model, ab, images, keep, ks, temp=0.9, sample_steps=steps)
    codes = model.encode_images(images)
    assert 0 < int(res.known.sum()) < res.known.numel()
    kept_bad = int((res.tokens[res.known] != codes[res.known]).sum())
    torch.manual_seed(2026)
    plain = complete_images(model, ab, images, keep, temp=0.9, sample_steps=steps)
    torch.manual_seed(2026)
    zeros = complete_images_top_k(model, ab, images, keep, [0] * B, temp=0.9, sample_steps=steps)
    zero_bad = int((zeros.tokens != plain.tokens).sum()) + int((zeros.images_u8 != plain.images_u8).sum())
    torch.manual_seed(2026)
    shard_bad = int((complete_images_sharded(model, ab, images, keep, temp=0.9, sample_steps=steps, top_k=ks) != res.images_u8).sum())
    parity("complete_images_top_k", known_changed=kept_bad, all_zero_vs_plain=zero_bad, sharded_pixels=shard_bad)
    assert kept_bad == 0 and zero_bad == 0 and shard_bad == 0 and int(res.tokens.max()) < K128
    assert torch.equal(res.tokens[4], plain.tokens[4]) and not torch.equal(res.tokens, plain.tokens)


# ------------------------------------------------------------------------------------------------- 8. what the wrappers refuse
def test_wrappers_refuse_a_bad_top_k(dev, ops):
    B, h = 5, 7
    g = torch.Generator().manual_seed(1)
    logits, x0, un0, _, _ = _state(B, K128, h, g, dev)
    good = torch.ones(B, dtype=torch.int32, device=dev)
    bads = (torch.ones(4, dtype=torch.int32, device=dev), torch.ones(B, dtype=torch.int64, device=dev), torch.ones(B, device=dev),
            torch.ones(B, dtype=torch.int32), torch.ones(B, 2, dtype=torch.int32, device=dev)[:, 0],
            torch.ones(1, B, dtype=torch.int32, device=dev), [1] * B, 3)
    cnt5 = torch.zeros(B, 8, h, h, 32, dtype=torch.uint8, device=dev)
    cnt1 = torch.zeros(B, 2, h, h, 32, dtype=torch.uint8, device=dev)
    packed6 = (torch.zeros(8 * 10 * 18432, dtype=torch.int8, device=dev), torch.zeros(128, dtype=torch.float64, device=dev),
               torch.zeros(128, dtype=torch.float64, device=dev))
    for bad in bads:
        x, un = x0.clone(), un0.clone()
        with pytest.raises(ValueError, match="top_k must be"):
            ops.psample_step(logits, x, un, 2, 1.0, top_k=bad)
        with pytest.raises(ValueError, match="top_k must be"):
            ops.den_step_tail(cnt5, cnt1, packed6, x, un, 2, 1.0, T=16, K=K128, top_k=bad)
        torch.cuda.synchronize()
        assert torch.equal(x, x0) and torch.equal(un, un0), "a refused call launched nothing"
    with pytest.raises(ValueError, match="per-image temp"):          # with top_k the temperature vector is checked as ever
        ops.psample_step(logits, x0.clone(), un0.clone(), 2, torch.ones(4, device=dev), top_k=good)
    # a scalar temperature is broadcast: the call equals the one with the vector
    a, b = x0.clone(), x0.clone()
    ops.psample_step(logits, a, un0.clone(), 2, 0.7, seed=3, top_k=good * 4)
    ops.psample_step(logits, b, un0.clone(), 2, torch.full((B,), 0.7, device=dev), seed=3, top_k=good * 4)
    assert torch.equal(a, b)
    # the sampler: a device tensor of the wrong dtype / length / device, and score() has no top_k
    den, _ = build_den(synth.MNIST, dev)
    ab = sampler(den, True, True, True)
    ab.n_samples = B
    torch.manual_seed(5)
    state = torch.get_rng_state()
    for bad in (torch.ones(B, dtype=torch.int64, device=dev), torch.ones(4, dtype=torch.int32, device=dev),
                torch.ones(B, dtype=torch.float32, device=dev), torch.ones(B, 1, dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError, match="top_k"):
            ab.sample_top_k(bad, 1.0, 3)
    with pytest.raises(TypeError):
        ab.score(torch.zeros(B, 1, h, h, dtype=torch.int64, device=dev), top_k=3)
    assert torch.equal(torch.get_rng_state(), state) and len(ab._graphs) == 0
