"""GPU tests of the per-image sampling temperature (run with ``-m gpu`` on an MI355X).  Everything here is exact:
the ``_temps`` entry points against their scalar siblings bit for bit (image i of a vector call == the scalar call at temp[i]),
``AbsorbingDiffusion.sample`` / ``.score`` with a vector against the scalar calls of every run of equal temperature (same key,
``set_shard`` on the run's first image) in every launch form, eager and captured, against the host oracle run per image, the
temperatures as a graph INPUT, and ``temperature_sweep`` / ``complete_images`` / ``token_nll_eval`` on top."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import _completion_oracle as corc           # noqa: E402
from parity_report import record as parity  # noqa: E402
from spkdiff import synth                  # noqa: E402
from test_gpu_completion import K, build_den, build_vae, sampler      # noqa: E402  (the helpers, not the tests)

TEMPS5 = (0.001, 0.3, 1.0, 0.65, 2.5)                 # kernel level: five images, five temperatures
TEMPS6 = (0.001, 0.3, 0.3, 1.0, 0.65, 1.0)           # sampler level
ACTIVE = (3, 0, 4)                                   # a short list that is not the identity: slot s != image active[s]
ORACLE_SEED = 777                                    # see test_vector_sample_vs_host_oracle_per_image


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def runs_of(temps):
    """Contiguous runs of equal temperature: [(first, count, temp)]."""
    out = []
    for i, t in enumerate(temps):
        if out and out[-1][2] == t:
            out[-1] = (out[-1][0], out[-1][1] + 1, t)
        else:
            out.append((i, 1, t))
    return out


def _state(B, Kc, h, g, dev):
    """A half-unmasked state and t = 2: every image has positions that change and positions that do not."""
    logits = torch.randn(B, Kc, h, h, generator=g) * 3
    un = torch.rand(B, 1, h, h, generator=g) < 0.5
    x = torch.where(un, torch.randint(0, Kc, (B, 1, h, h), generator=g), torch.full((B, 1, h, h), Kc))
    u = torch.rand(B * h * h, generator=g)
    q = torch.empty(B * h * h, Kc).exponential_(1, generator=g)
    return logits.to(dev), x.to(dev), un.to(dev), u.to(dev), q.to(dev)


def _active(B, dev):
    act = torch.zeros(B, dtype=torch.int32)
    act[:len(ACTIVE)] = torch.tensor(ACTIVE, dtype=torch.int32)
    return act.to(dev), torch.tensor([len(ACTIVE), 0], dtype=torch.int32, device=dev)


def _both_kinds(un0, un1):
    """Every image has changed and unchanged masked positions."""
    ch = (un1 & ~un0).flatten(1).sum(1)
    left = (~un1).flatten(1).sum(1)
    return bool((ch > 0).all()) and bool((left > 0).all())


# ------------------------------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("HW", [49, 64])
@pytest.mark.parametrize("Kc", [100, 128, 512])
def test_psample_step_temps_equals_the_scalar_entry_point_per_image(dev, ops, Kc, HW):
    B, h, t = 5, int(math.isqrt(HW)), 2
    g = torch.Generator().manual_seed(Kc * 100 + HW)
    logits, x0, un0, u, q = _state(B, Kc, h, g, dev)
    tv = torch.tensor(TEMPS5, dtype=torch.float32, device=dev)
    seed, off = 0x1234_5678_9ABC, 5 * (1 << 40) + 11 * HW * Kc
    state = torch.tensor([seed, 1 << 33], dtype=torch.int64, device=dev)
    modes = {"philox": dict(seed=seed, offset=off), "philox_state": dict(seed=99, offset=off - (1 << 33), philox_state=state),
             "injected": dict(u=u, q=q)}
    bad, both = {}, True

    def call(temp, active=None, **kw):
        x, un = x0.clone(), un0.clone()
        if active is not None:
            with ops.active_set(*active):
                ops.psample_step(slots, x, un, t, temp, **kw)
            return x, un, None, None
        x0h = torch.full((B, 1, h, h), -5, dtype=torch.int64, device=dev)
        nxt = torch.full((B, 2, h, h), float("nan"), device=dev)
        ops.psample_step(logits, x, un, t, temp, x0_hat=x0h, next_input=nxt, **kw)
        return x, un, x0h, nxt

    slots = torch.full_like(logits, float("nan"))        # slots beyond the list hold NaN and must never be read
    slots[:len(ACTIVE)] = logits[list(ACTIVE)]
    act = _active(B, dev)
    for mode, kw in modes.items():
        vec = call(tv, **kw)
        both = both and _both_kinds(un0, vec[1])
        n = 0
        for i, ti in enumerate(TEMPS5):
            sc = call(ti, **kw)
            n += sum(int((a[i] != b[i]).sum()) for a, b in zip(vec[:3], sc[:3])) + int(not torch.equal(vec[3][i], sc[3][i]))
        assert torch.equal(vec[3], ops.den_build_input(vec[0], t - 1))
        bad[mode] = n
        # active list: slot s serves image ACTIVE[s] and reads temp_b[ACTIVE[s]]
        veca = call(tv, active=act, **kw)
        n = 0
        for i in ACTIVE:
            sca = call(TEMPS5[i], active=act, **kw)
            n += int((veca[0][i] != sca[0][i]).sum()) + int((veca[1][i] != sca[1][i]).sum())
            n += int((veca[0][i] != vec[0][i]).sum())               # ... which is the dense call's image i
        for i in set(range(B)) - set(ACTIVE):
            n += int((veca[0][i] != x0[i]).sum()) + int((veca[1][i] != un0[i]).sum())
        bad["active_" + mode] = n
    # temperatures matter: the coldest image takes the arg max, a vector of another order gives other tokens
    swapped = call(tv.flip(0).contiguous(), **modes["philox"])
    assert not torch.equal(swapped[2], call(tv, **modes["philox"])[2])
    parity(f"psample_step_temps_K{Kc}_HW{HW}", mismatches=bad, both_kinds_of_position=both)
    assert both and all(v == 0 for v in bad.values()), bad


@pytest.mark.parametrize("HW", [49, 64])
@pytest.mark.parametrize("Kc", [100, 128, 512])
def test_pscore_step_temps_equals_the_scalar_entry_point_per_image(dev, ops, Kc, HW):
    B, h, t = 5, int(math.isqrt(HW)), 2
    g = torch.Generator().manual_seed(Kc * 100 + HW + 1)
    logits, x0, un0, u, _ = _state(B, Kc, h, g, dev)
    target = torch.randint(0, Kc, (B, h, h), generator=g).to(dev)
    tv = torch.tensor(TEMPS5, dtype=torch.float32, device=dev)
    seed, off = 0xABCDEF, 7 * (1 << 40) + 3 * HW * Kc
    state = torch.tensor([seed, 1 << 20], dtype=torch.int64, device=dev)
    modes = {"philox": dict(seed=seed, offset=off), "philox_state": dict(seed=1, offset=off - (1 << 20), philox_state=state),
             "injected": dict(u=u)}
    slots = torch.full_like(logits, float("nan"))
    slots[:len(ACTIVE)] = logits[list(ACTIVE)]
    act = _active(B, dev)

    def call(temp, active=None, **kw):
        x, un = x0.clone(), un0.clone()
        logp = torch.full((B, h, h), -12345.0, dtype=torch.float64, device=dev)
        step = torch.full((B, h, h), -7, dtype=torch.int32, device=dev)
        if active is not None:
            with ops.active_set(*active):
                ops.pscore_step(slots, target, x, un, t, temp, logp, step, **kw)
            return x, un, logp, step, None
        nxt = torch.full((B, 2, h, h), float("nan"), device=dev)
        ops.pscore_step(logits, target, x, un, t, temp, logp, step, next_input=nxt, **kw)
        return x, un, logp, step, nxt

    bad, both = {}, True
    for mode, kw in modes.items():
        vec = call(tv, **kw)
        both = both and _both_kinds(un0, vec[1])
        n = 0
        for i, ti in enumerate(TEMPS5):
            sc = call(ti, **kw)
            # (fp64 log-probabilities compared as bit patterns)
            n += sum(int((a[i] != b[i]).sum()) for a, b in ((vec[0], sc[0]), (vec[1], sc[1]), (vec[3], sc[3])))
            n += int((vec[2][i].view(torch.int64) != sc[2][i].view(torch.int64)).sum()) + int(not torch.equal(vec[4][i], sc[4][i]))
        bad[mode] = n
        veca = call(tv, active=act, **kw)
        n = 0
        for i in ACTIVE:
            sca = call(TEMPS5[i], active=act, **kw)
            n += int((veca[2][i].view(torch.int64) != sca[2][i].view(torch.int64)).sum()) + int((veca[3][i] != sca[3][i]).sum())
            n += int((veca[2][i].view(torch.int64) != vec[2][i].view(torch.int64)).sum()) + int((veca[1][i] != vec[1][i]).sum())
        for i in set(range(B)) - set(ACTIVE):
            n += int((veca[2][i] != -12345.0).sum()) + int((veca[1][i] != un0[i]).sum())
        bad["active_" + mode] = n
    vec = call(tv, **modes["philox"])
    ch = vec[1] & ~un0
    assert not torch.equal(vec[2][0][ch[0, 0]], call(1.0, **modes["philox"])[2][0][ch[0, 0]]), "the temperature reaches the score"
    parity(f"pscore_step_temps_K{Kc}_HW{HW}", mismatches=bad, both_kinds_of_position=both)
    assert both and all(v == 0 for v in bad.values()), bad


_DENS = {}


def _den_k(Kc, dev):
    """A denoiser with ``Kc`` classes (random init, logits widened so that the classes compete), as tests/test_gpu_parity.py makes it."""
    from snn_model.vq_diffusion import DummyModel, functional
    if Kc not in _DENS:
        torch.manual_seed(Kc)
        den = DummyModel(1, Kc).to(dev)
        functional.set_step_mode(net=den, step_mode='m')
        with torch.no_grad():
            den.conv6[0].weight.mul_(20.0)
        _DENS[Kc] = den.eval()
    return _DENS[Kc]


@pytest.mark.parametrize("L", [7, 8])
@pytest.mark.parametrize("Kc", [100, 128, 512])
def test_den_step_tail_temps_equals_the_scalar_entry_point_per_image(dev, ops, Kc, L):
    """Dense form with the fused next-step first layer (x1 / cnt1) and the optional logits; the active-list form; Philox and
    injected noise; one to four channel groups per wave (K = 100 / 128: one, 512: four)."""
    den = _den_k(Kc, dev)
    assert den.tail_fusable(L, L)
    B, HW, t = 5, L * L, 2
    g = torch.Generator().manual_seed(Kc * 10 + L)
    _, x0, un0, u, q = _state(B, Kc, L, g, dev)
    tv = torch.tensor(TEMPS5, dtype=torch.float32, device=dev)
    _, cnt5, _, cnt1, which, _, collapse = den._trunk(ops.den_build_input(x0, t), False)
    assert which == 'mfma-fp6v2' and collapse
    conv6, packed6 = den._conv6_params()
    conv1, bn1 = den.conv1[0], den.conv1[1]
    a1, b1 = bn1.affine_terms()
    c1 = (conv1._spk_params.get(conv1), conv1.bias.detach(), a1, b1)
    act = _active(B, dev)
    with ops.active_set(*act):
        _, cnt5a, _, cnt1a, _, _, _ = den._trunk(ops.den_build_input(x0, t), False)
    modes = {"philox": dict(seed=4242, offset=1000 * t), "injected": dict(u=u, q=q)}

    def call(temp, active=None, **kw):
        x, un = x0.clone(), un0.clone()
        if active is not None:
            with ops.active_set(*active):
                pre, lg = ops.den_step_tail(cnt5a, cnt1a, packed6, x, un, t, temp, T=16, K=Kc, conv1=None, want_logits=True, **kw)
            assert pre is None
            return x, un, lg[:len(ACTIVE)]
        pre, lg = ops.den_step_tail(cnt5, cnt1, packed6, x, un, t, temp, T=16, K=Kc, conv1=c1, want_logits=True, **kw)
        return x, un, lg, pre[0], pre[1]

    bad, both = {}, True
    for mode, kw in modes.items():
        vec = call(tv, **kw)
        both = both and _both_kinds(un0, vec[1])
        n = 0
        for i, ti in enumerate(TEMPS5):
            sc = call(ti, **kw)
            n += sum(int(not torch.equal(a[i], b[i])) for a, b in zip(vec, sc))
        bad[mode] = n
        veca = call(tv, active=act, **kw)
        n = 0
        for i in ACTIVE:
            sca = call(TEMPS5[i], active=act, **kw)
            n += int(not torch.equal(veca[0][i], sca[0][i])) + int(not torch.equal(veca[1][i], sca[1][i]))
            n += int(not torch.equal(veca[0][i], vec[0][i]))           # ... the dense call's image i
        n += int(not torch.equal(veca[2], call(1.0, active=act, **kw)[2]))   # (the logits do not see the temperature)
        for i in set(range(B)) - set(ACTIVE):
            n += int(not torch.equal(veca[0][i], x0[i])) + int(not torch.equal(veca[1][i], un0[i]))
        bad["active_" + mode] = n
    assert not torch.equal(call(tv.flip(0).contiguous(), **modes["philox"])[0], call(tv, **modes["philox"])[0])
    parity(f"den_step_tail_temps_K{Kc}_{L}x{L}", mismatches=bad, both_kinds_of_position=both)
    assert both and all(v == 0 for v in bad.values()), bad


def test_wrappers_refuse_a_bad_vector(dev, ops):
    B, h = 5, 7
    g = torch.Generator().manual_seed(1)
    logits, x0, un0, _, _ = _state(B, K, h, g, dev)
    for bad in (torch.ones(4, device=dev), torch.ones(B, dtype=torch.float64, device=dev), torch.ones(B), torch.ones(B, 2, device=dev)[:, 0],
                torch.ones(1, B, device=dev)):
        with pytest.raises(ValueError, match="per-image temp"):
            ops.psample_step(logits, x0.clone(), un0.clone(), 2, bad)
    # one-element tensors are the scalar call
    a, b = x0.clone(), x0.clone()
    ops.psample_step(logits, a, un0.clone(), 2, torch.tensor([0.7], device=dev), seed=3)
    ops.psample_step(logits, b, un0.clone(), 2, 0.7, seed=3)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 2. the sampler
LAUNCH_FORMS = (                  # name, skip, lists, use_step_tail, step_tail_in_elimination, form_for
    ("dense", False, False, False, False, "dense"),
    ("dense_tail", False, False, True, False, "dense_step_tail"),
    ("elim", True, False, True, False, "elimination"),
    ("elim_lists", True, True, True, False, "elimination_lists"),
    ("elim_tail", True, False, True, True, "elimination"),
    ("elim_lists_tail", True, True, True, True, "elimination_lists"),
)


def _form_sampler(den, form, graph, latent=7):
    name, skip, lists, tail, tail_elim, _ = form
    ab = sampler(den, skip, lists, graph, latent=latent)
    ab.list_min_batch = 0                      # (the lists at a batch of six)
    ab.step_tail_in_elimination = tail_elim
    return ab


def _scalar_runs(den, temps, fn, latent=7):
    """fn(sampler sharded on the run, first, count, temp) for every run of equal temperature, concatenated along the batch."""
    parts = []
    for first, count, t in runs_of(temps):
        sh = sampler(den, True, True, False, latent=latent).set_shard(first, count)
        parts.append(fn(sh, first, count, t))
    return parts


@pytest.mark.parametrize("steps", [12, 49])
def test_vector_sample_equals_the_scalar_calls_in_every_form(dev, steps):
    den, _ = build_den(synth.MNIST, dev)
    B = len(TEMPS6)

    def scalar(sh, first, count, t):
        torch.manual_seed(4100 + steps)
        return sh.sample(t, steps)
    want = torch.cat(_scalar_runs(den, TEMPS6, scalar))
    bad = {}
    tail0 = den.use_step_tail
    try:
        for form in LAUNCH_FORMS:
            den.use_step_tail = form[3]
            for graph in (False, True):
                ab = _form_sampler(den, form, graph)
                ab.n_samples = B
                assert ab.form_for(B, 7, 7) == form[5] and ab._form(B, 7, 7).tail_act == (form[4] and form[1])
                for kind, tv in (("list", list(TEMPS6)), ("device", torch.tensor(TEMPS6, dtype=torch.float32, device=dev))):
                    torch.manual_seed(4100 + steps)
                    got = ab.sample(tv, steps)
                    bad[f"{form[0]}_{'graph' if graph else 'eager'}_{kind}"] = int((got != want).sum())
                assert len(ab._graphs) == (1 if graph else 0)
    finally:
        den.use_step_tail = tail0
    assert int(want.max()) < K and int(want.min()) >= 0
    parity(f"temps_sample_forms_{steps}steps", token_mismatches=bad, tokens=int(want.numel()))
    assert all(v == 0 for v in bad.values()), bad


def test_vector_sample_on_the_8x8_model(dev):
    den, _ = build_den(synth.CIFAR, dev)
    B, steps = len(TEMPS6), 12

    def scalar(sh, first, count, t):
        torch.manual_seed(88)
        return sh.sample(t, steps)
    want = torch.cat(_scalar_runs(den, TEMPS6, scalar, latent=8))
    bad = {}
    for form, graph in ((LAUNCH_FORMS[1], True), (LAUNCH_FORMS[2], False)):
        ab = _form_sampler(den, form, graph, latent=8)
        ab.n_samples = B
        assert ab.form_for(B, 8, 8) == form[5]
        torch.manual_seed(88)
        bad[form[0]] = int((ab.sample(list(TEMPS6), steps) != want).sum())
    parity("temps_sample_8x8", token_mismatches=bad, tokens=int(want.numel()))
    assert all(v == 0 for v in bad.values()), bad


def test_vector_sample_vs_host_oracle_per_image(dev):
    """B = 4, 12 steps, the captured dense and elimination forms against the host oracle (tests/_completion_oracle.run, its default
    fp32 mode) run once per IMAGE with that image's scalar temperature and the host's own Philox noise at the image's global
    index: zero differing tokens, no allowance for near-ties.  The key is the draw after torch.manual_seed(ORACLE_SEED); for this
    job (synthetic MNIST denoiser) the fp32 oracle and the exact-convolution oracle were checked on the host to give the same
    tokens for every image, so no spike of the oracle hangs on a summation order and equality is a fair demand."""
    den, sd = build_den(synth.MNIST, dev)
    temps, steps, B = (0.001, 0.3, 1.0, 0.65), 12, 4
    none = torch.zeros(1, 1, 7, 7, dtype=torch.bool)
    torch.manual_seed(ORACLE_SEED)
    key = sampler(den, True, True, True)._philox_key()
    want = torch.cat([corc.run(sd, torch.zeros(1, 1, 7, 7, dtype=torch.int64), none, steps,
                               corc.host_philox_noise(key, steps, 1, 7, K, first=i), temp=temps[i])[0] for i in range(B)])
    bad = {}
    for form in (LAUNCH_FORMS[1], LAUNCH_FORMS[3]):
        ab = _form_sampler(den, form, True)
        ab.n_samples = B
        torch.manual_seed(ORACLE_SEED)
        got = ab.sample(list(temps), steps).cpu()
        assert int(ab.last_key) == key and len(ab._graphs) == 1
        bad[form[0]] = int((got != want).sum())
    print(f"vector temperatures vs per-image host oracle: token mismatches {bad} of {want.numel()}")
    parity("temps_sample_vs_host_oracle", token_mismatches=bad, tokens=int(want.numel()))
    assert all(v == 0 for v in bad.values()), bad


def test_temperatures_are_a_graph_input(dev):
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 6, 12
    ab = sampler(den, True, True, True)
    eager = sampler(den, True, True, False)
    ab.n_samples = eager.n_samples = B
    va, vb = list(TEMPS6), [1.0, 0.65, 0.001, 0.3, 2.0, 0.3]
    out = []
    for seed, tv in ((1, va), (2, vb), (1, va)):
        torch.manual_seed(seed)
        got = ab.sample(tv, steps)
        torch.manual_seed(seed)
        out.append((got, int((got != eager.sample(tv, steps)).sum())))
    assert len(ab._graphs) == 1, "one graph serves every temperature vector"
    torch.manual_seed(1)
    other = ab.sample(vb, steps)                                    # same key, other temperatures: other tokens
    assert torch.equal(out[0][0], out[2][0]) and not torch.equal(other, out[0][0]) and len(ab._graphs) == 1
    g = next(iter(ab._graphs.values()))
    assert g.temps is not None and g.temps.tolist() == torch.tensor(vb, dtype=torch.float32).tolist()
    assert "per-image" in next(iter(ab._graphs))
    # a scalar call adds its own graph, keyed by the value as ever
    torch.manual_seed(3)
    s1 = ab.sample(0.65, steps)
    assert len(ab._graphs) == 2 and any(0.65 in k for k in ab._graphs) and all(gr.temps is None for k, gr in ab._graphs.items() if 0.65 in k)
    torch.manual_seed(3)
    assert torch.equal(s1, eager.sample(0.65, steps))
    torch.manual_seed(3)
    assert torch.equal(s1, ab.sample([0.65] * B, steps)) and len(ab._graphs) == 2
    parity("temps_graph_input", token_mismatches_vs_eager=[o[1] for o in out], graphs=len(ab._graphs))
    assert all(o[1] == 0 for o in out)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("with_known", [False, True], ids=["all", "known"])
def test_vector_score_equals_the_scalar_calls(dev, graph, with_known):
    den, _ = build_den(synth.MNIST, dev)
    B, steps, orders = len(TEMPS6), 12, 2
    x_init, known = corc.issue_start(B)
    x0 = x_init.to(dev)
    kn = known.to(dev) if with_known else None

    def scalar(sh, first, count, t):
        torch.manual_seed(52)
        return sh.score(x0[first:first + count], temp=t, sample_steps=steps, orders=orders,
                        known=None if kn is None else kn[first:first + count])
    parts = _scalar_runs(den, TEMPS6, scalar)
    want_lp = torch.cat([p.position_log_prob for p in parts], dim=1)
    want_st = torch.cat([p.reveal_step for p in parts], dim=1)
    bad = {}
    for form in (LAUNCH_FORMS[0], LAUNCH_FORMS[2], LAUNCH_FORMS[3]):
        ab = _form_sampler(den, form, graph)
        for kind, tv in (("list", list(TEMPS6)), ("device", torch.tensor(TEMPS6, dtype=torch.float32, device=dev))):
            torch.manual_seed(52)
            sc = ab.score(x0, temp=tv, sample_steps=steps, orders=orders, known=kn)
            bad[f"{form[0]}_{kind}"] = (int((sc.position_log_prob.view(torch.int64) != want_lp.view(torch.int64)).sum()) +
                                        int((sc.reveal_step != want_st).sum()))
        assert len(ab._graphs) == (1 if graph else 0)
        assert sc.position_log_prob.shape == (orders, B, 7, 7) and sc.log_prob.shape == (orders, B)
    if with_known:
        kd = known[:, 0].to(dev)
        assert bool((want_lp[:, kd] == 0).all()) and bool((want_st[:, kd] == 0).all())
    assert bool(torch.isfinite(want_lp).all()) and not torch.equal(want_lp[0], want_lp[1])
    parity(f"temps_score_{'graph' if graph else 'eager'}_{'known' if with_known else 'all'}", mismatches=bad,
           positions=int(want_lp.numel()))
    assert all(v == 0 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------- 3. on top
def test_temperature_sweep_does_not_depend_on_batch_or_split(dev):
    from spkdiff import dist as sdist
    from spkdiff.evaluate import temperature_sweep, temperature_sweep_range
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    temps, n, steps = (0.3, 1.0, 0.65), 5, 12
    ab = sampler(den, True, True, True)
    ab.set_shard(3, 7)
    res = {}
    for name, batch in (("batch4", 4), ("one_call", None)):
        torch.manual_seed(909)
        res[name] = temperature_sweep(model, ab, temps, n, sample_steps=steps, batch=batch)
        key = int(ab.last_key)
        assert (ab.n_samples, ab.global_first) == (7, 3), "the sampler's shard is restored"
        # four calls (4 + 4 + 4 + 3 images) on two graphs, one per call size: the shard is a graph input as the temperatures are
        assert len(ab._graphs) == (2 if batch == 4 else 1)
    u8, tok = res["batch4"]
    assert u8.shape == (3, n, 1, 28, 28) and u8.dtype == torch.uint8 and tok.shape == (3, n, 7, 7) and tok.dtype == torch.int64
    halves = []
    for rank in range(2):                                            # two ranks of one job, in process: one key
        lo, hi = sdist.shard_range(3 * n, rank, 2)
        torch.manual_seed(909)
        halves.append(temperature_sweep_range(model, sampler(den, True, True, True), temps, n, lo, hi, sample_steps=steps, batch=4))
    split = (torch.cat([h[0] for h in halves]).reshape(u8.shape), torch.cat([h[1] for h in halves]).reshape(tok.shape))
    # the scalar protocol: per temperature, sample(temp) on the group's shard and decode
    s_tok, s_u8 = [], []
    for gi, t in enumerate(temps):
        sh = sampler(den, True, True, False).set_shard(gi * n, n)
        torch.manual_seed(909)
        tk = sh.sample(t, steps).reshape(n, 7, 7)
        assert int(sh.last_key) == key
        s_tok.append(tk)
        s_u8.append(model.decode_tokens(tk, 16, want_u8=True)[1])
    s_tok, s_u8 = torch.stack(s_tok), torch.stack(s_u8)
    bad = dict(one_call_tokens=int((res["one_call"][1] != tok).sum()), one_call_pixels=int((res["one_call"][0] != u8).sum()),
               split_tokens=int((split[1] != tok).sum()), split_pixels=int((split[0] != u8).sum()),
               scalar_tokens=int((s_tok != tok).sum()), scalar_pixels=int((s_u8 != u8).sum()))
    parity("temperature_sweep", **bad, tokens=int(tok.numel()))
    assert all(v == 0 for v in bad.values()), bad
    assert sdist.temperature_sweep_sharded.__module__ == "spkdiff.dist"
    torch.manual_seed(909)
    assert torch.equal(sdist.temperature_sweep_sharded(model, ab, temps, n, sample_steps=steps, batch=4), u8)


def test_complete_images_with_a_vector(dev):
    from spkdiff.complete import complete_images
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 8, 12
    temps = [0.3] * 3 + [1.0] * 3 + [0.65] * 2
    images = (synth.stroke_images(B, seed=77, img=28, channels=1) - 0.5).to(dev)
    keep = torch.ones(B, 28, 28, dtype=torch.bool)
    keep[:, 14:] = False
    keep[1::2, :, 10:17] = False
    keep = keep.to(dev)
    ab = sampler(den, True, True, True)
    torch.manual_seed(2025)
    res = complete_images(model, ab, images, keep, temp=temps, sample_steps=steps)
    codes = model.encode_images(images)
    assert 0 < int(res.known.sum()) < res.known.numel()
    kept_bad = int((res.tokens[res.known] != codes[res.known]).sum())

    def scalar(sh, first, count, t):
        torch.manual_seed(2025)
        return complete_images(model, sh, images[first:first + count], keep[first:first + count], temp=t, sample_steps=steps)
    parts = _scalar_runs(den, temps, scalar)
    tok_bad = int((torch.cat([p.tokens for p in parts]) != res.tokens).sum())
    px_bad = int((torch.cat([p.images_u8 for p in parts]) != res.images_u8).sum())
    parity("complete_images_temps", known_changed=kept_bad, token_mismatches=tok_bad, pixel_mismatches=px_bad)
    assert kept_bad == 0 and tok_bad == 0 and px_bad == 0 and int(res.tokens.max()) < K


def test_token_nll_eval_curve_from_one_pass(dev):
    from spkdiff.evaluate import token_nll_eval
    model, _ = build_vae(synth.MNIST, dev)
    den, _ = build_den(synth.MNIST, dev)
    B, steps, temps = 4, 12, [1.0, 0.5, 2.0]
    images = synth.stroke_images(B, seed=5, img=28, channels=1)
    ab = sampler(den, True, True, True)
    torch.manual_seed(64)
    r = token_nll_eval(model, ab, [images], sample_steps=steps, temps=temps)
    assert r["temps"] == temps and r["n_images"] == B and len(r["bits_per_dim"]) == 3 and len(ab._graphs) == 1
    codes = model.encode_images((images - 0.5).to(dev).float().contiguous(), 16)
    for gi, t in enumerate(temps):                                   # replica gi sits at global images gi * B ..
        sh = sampler(den, True, True, False).set_shard(gi * B)
        torch.manual_seed(64)
        nats = -float(sh.score(codes, temp=t, sample_steps=steps).log_prob.sum()) / B
        assert abs(nats - r["nats_per_image"][gi]) <= 1e-9 * max(1.0, abs(nats))
        assert abs(nats / (math.log(2) * 49) - r["bits_per_dim"][gi]) <= 1e-9
    torch.manual_seed(64)
    one = token_nll_eval(model, ab, [images], temp=1.0, sample_steps=steps)
    assert isinstance(one["bits_per_dim"], float) and abs(one["bits_per_dim"] - r["bits_per_dim"][0]) <= 1e-12
