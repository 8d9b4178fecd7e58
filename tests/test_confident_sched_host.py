"""CPU tests of reveal schedules and annealed selection noise for confidence-ordered decoding: the count arithmetic
(the linear identity, the cosine tables, the forced 1, zero and non-monotone weights), the literal-sort commit on scores against the
mirror of the kernel's rank arithmetic, the annealing table, the package's builders against the oracle of
tests/_confident_sched_oracle.py, what the three new C entry points and the Python arguments refuse before anything is launched, and
the launch sequence: with both arguments at their defaults the calls made before, with anything else the ``_sched`` family.  No device."""
import inspect
import math

import numpy as np
import pytest
import torch

import _confident_oracle as cfo
import _confident_sched_oracle as cso

W_MAX = 1 << 24


# ------------------------------------------------------------------------------------------------- the count arithmetic
def test_linear_table_gives_the_ceil_count_for_all_m_and_t():
    """w[t] = t: m - floor(m (t - 1) / t) == ceil(m / t), the count of the rule without a schedule, for all m, t <= 64."""
    for m in range(0, 65):
        for t in range(1, 65):
            assert cso.reveal_count(m, t - 1, t) == cfo.n_reveal(m, t) == -(-m // t), (m, t)
    for e in (1, 2, 13, 49, 64):
        w = cso.linear_weights(e)
        assert w == list(range(e + 1))
        for m0 in (0, 1, 48, 49, 64):
            m, want = m0, []
            for t in range(e, 0, -1):
                want.append(cfo.n_reveal(m, t))
                m -= want[-1]
            assert cso.run_counts(m0, w) == want and m == 0


def test_cosine_tables():
    """e = 1 .. 49: non-decreasing, at most 2^24, w[0] = 0, w[e] = 2^24, and the counts of a run sum to m for every m <= 64; at 8
    steps and 49 positions the first step commits the fewest tokens -- fewer than the linear table's 7 -- and the second half of the
    run more than the first."""
    for e in range(1, 50):
        w = cso.cosine_weights(e)
        assert len(w) == e + 1 and w[0] == 0 and w[e] == W_MAX and max(w) <= W_MAX
        assert all(w[t - 1] <= w[t] for t in range(1, e + 1))
        assert all(abs(w[t] - W_MAX * math.sin(math.pi * t / (2 * e))) <= 0.5 + 1e-6 for t in range(e + 1))
        for m0 in (0, 1, 2, 48, 49, 64):
            c = cso.run_counts(m0, w)
            assert len(c) == e and sum(c) == m0 and all(v >= 0 for v in c)
            left = m0
            for v in c:                                                   # (the forced 1: a step with something masked reveals)
                assert v >= 1 or left == 0
                left -= v
    c8 = cso.run_counts(49, cso.cosine_weights(8))
    assert c8[0] == min(c8) < 7 and sum(c8[4:]) > sum(c8[:4]) and max(c8) > 7, c8


def test_the_forced_one_zero_weights_and_non_monotone_pairs():
    # the forced 1: keep would be everything
    assert cso.reveal_count(5, 10, 10) == 1 and cso.reveal_count(1, W_MAX - 1, W_MAX) == 1 and cso.reveal_count(64, 999, 1000) == 1
    assert cso.reveal_count(0, 10, 10) == 0 and cso.reveal_count(0, 0, 0) == 0, "nothing masked: nothing revealed"
    # w[t] == 0: keep = 0, everything is revealed whatever w[t - 1] is; w[t - 1] == 0 too
    for m in (0, 1, 49, 64):
        assert cso.reveal_count(m, 123, 0) == m and cso.reveal_count(m, 0, 0) == m and cso.reveal_count(m, 0, 77) == m
    # w[t - 1] > w[t]: the quotient exceeds m, the min keeps all, the forced 1 reveals one
    for m in (1, 2, 49, 64):
        assert cso.reveal_count(m, 11, 10) == 1 and cso.reveal_count(m, W_MAX, 1) == 1
    # the largest operands stay far below 2^64 (and below 2^31)
    assert 64 * W_MAX < (1 << 31) and cso.reveal_count(64, W_MAX, W_MAX) == 1 and cso.reveal_count(64, W_MAX // 2, W_MAX) == 32
    # the custom tables of the GPU cases really hold a zero weight and a non-monotone pair, and every run ends with nothing masked
    # where its w[0] is 0
    for S in (1, 2, 8, 100):
        tabs = cso.custom_tables(S)
        assert 0 in tabs["zero"][1:] and (S < 2 or any(tabs["bump"][t - 1] > tabs["bump"][t] for t in range(1, S + 1)))
        for w in tabs.values():
            assert len(w) == S + 1 and w[0] == 0 and 0 <= min(w) and max(w) <= W_MAX
            assert sum(cso.run_counts(49, w)) == 49


def test_the_package_builds_the_oracles_tables():
    from spkdiff import schedules as sch
    assert sch.W_MAX == W_MAX
    for e in range(1, 50):
        assert sch.linear_weights(e) == cso.linear_weights(e) and sch.cosine_weights(e) == cso.cosine_weights(e)
    for m in range(0, 65):
        for wp, wc in ((0, 0), (0, 5), (5, 0), (3, 4), (4, 3), (W_MAX, W_MAX), (1, W_MAX), (11863283, 16777216)):
            assert sch.reveal_count(m, wp, wc) == cso.reveal_count(m, wp, wc)
    for e in (1, 8, 12, 16):
        for w in (cso.linear_weights(e), cso.cosine_weights(e)):
            assert sch.reveal_counts(49, w) == cso.run_counts(49, w)
    assert sch.reveal_counts(49, sch.linear_weights(8)) == [7, 6, 6, 6, 6, 6, 6, 6]
    # a row for an image of e < S steps: its own table in entries 0 .. e, the last entry repeated above
    row = sch.weights_row("cosine", 5, 8)
    assert row[:6] == cso.cosine_weights(5) and row[6:] == [W_MAX] * 3
    assert sch.weights_row(None, 3, 5) == [0, 1, 2, 3, 3, 3] == sch.weights_row("linear", 3, 5)
    assert sch.weights_row([0, 4, 4, 9], 3, 5) == [0, 4, 4, 9, 9, 9] and sch.weights_row([0, 1, 2, 3, 4, 5], 3, 5) == [0, 1, 2, 3, 4, 5]
    for bad in ("sine", [0, 1, 2], [0, 1, 2.0, 3], [0, 1, True, 3], [0, 1, -1, 3], [0, 1, W_MAX + 1, 3], 7, [[0, 1, 2, 3]]):
        with pytest.raises(ValueError):
            sch.weights_row(bad, 3, 5)
    with pytest.raises(ValueError):
        sch.weights_row("cosine", 6, 5)


def test_the_annealing_table():
    from spkdiff import schedules as sch
    for tau in (0.0, 0.5, 4.5, 1e3):
        for e, S in ((1, 1), (1, 5), (8, 8), (5, 8), (16, 16)):
            a = sch.noise_scales(tau, e, S)
            assert len(a) == S + 1 and a[0] == 0.0 and a[1] == 0.0, "the last step of every image is noise-free"
            assert all(v == 0.0 for v in a[e + 1:]) and all(a[t] == tau * (t - 1) / e for t in range(1, e + 1))
            assert [float(np.float32(v)) for v in a] == cso.noise_row(tau, e, S)
            assert tau == 0 or e == 1 or a[e] == tau * (e - 1) / e > 0
    for bad in (-1.0, float("nan"), float("inf"), -0.5, "x", None, True):
        with pytest.raises(ValueError):
            sch.noise_scales(bad, 4, 4)


# ------------------------------------------------------------------------------------------------- the commit on scores
def test_literal_sort_commit_equals_the_rank_mirror():
    """Seeded scores with ties, -inf (u = 0 under a > 0), +inf and NaN, every count n = 0 .. m + 1: the two commits agree, reveal
    min(n, m) positions, -inf orders last among the numbers and ahead of the NaNs, ties go to the lower position."""
    g = np.random.default_rng(17)
    for HW in (1, 2, 49, 64):
        for rep in range(20):
            masked = g.random(HW) < (0.0, 0.3, 0.7, 1.0)[rep % 4]
            score = g.standard_normal(HW).astype(np.float32) * 5
            score[g.random(HW) < 0.3] = np.float32(-1.25)                      # ties
            score[g.random(HW) < 0.1] = -np.inf
            score[g.random(HW) < 0.1] = np.nan
            score[g.random(HW) < 0.05] = np.inf
            m = int(masked.sum())
            for n in range(0, m + 2):
                a, b = cso.commit_by_sort(masked, score, n), cso.commit_by_rank(masked, score, n)
                assert np.array_equal(a, b) and int(a.sum()) == min(n, m) and not bool((a & ~masked).any())
    masked = np.ones(5, dtype=bool)
    score = np.array([np.nan, -np.inf, -3.0, -3.0, -np.inf], dtype=np.float32)
    order = [int(np.flatnonzero(cso.commit_by_sort(masked, score, n) & ~cso.commit_by_sort(masked, score, n - 1))[0]) for n in range(1, 6)]
    assert order == [2, 3, 1, 4, 0]
    # with the linear count and the confidence as the score it is the commit of the rule without a schedule
    for t in (1, 2, 3, 7):
        conf = g.standard_normal(49).astype(np.float32)
        masked = g.random(49) < 0.6
        n = cso.reveal_count(int(masked.sum()), t - 1, t)
        assert np.array_equal(cso.commit_by_sort(masked, conf, n), cfo.commit_by_sort(masked, conf, t))


def test_score_bound_is_counted_from_the_formats():
    """The bound grows with |a| and |g|, equals the confidence's bound (plus the unit round-off of the sum) at a = 0, and an fp32
    evaluation of the formula with correctly rounded logarithms lies inside it."""
    g = np.random.default_rng(3)
    u = (g.integers(1, 1 << 24, 4000).astype(np.float64)) / float(1 << 24)
    conf = -np.abs(g.standard_normal(4000)) * 3
    mx = np.abs(g.standard_normal(4000)) * 4
    for a in (0.0, 0.5, 4.5, float(1 << 20)):
        av = np.full(4000, np.float32(a), dtype=np.float64)
        b = cso.score_bound(128, mx, conf, av, u)
        u32, a32, c32 = u.astype(np.float32), av.astype(np.float32), conf.astype(np.float32)
        g32 = -np.log(-np.log(u32).astype(np.float32)).astype(np.float32)
        s32 = (c32 + (a32 * g32).astype(np.float32)).astype(np.float32) if a else c32
        err = np.abs(s32.astype(np.float64) - cso.score_f64(c32.astype(np.float64), av, u))
        assert bool((err <= b).all()) and bool((b >= cfo.conf_bound(128, mx, conf)).all())
    assert bool((cso.score_bound(128, mx, conf, np.full(4000, 9.0), u) > cso.score_bound(128, mx, conf, np.full(4000, 1.0), u)).all())


# ------------------------------------------------------------------------------------------------- the C entry points
def test_entry_points_are_declared_resolved_and_refuse_bad_arguments_without_a_device():
    from spkdiff import _lib
    C = _lib.CONSTANTS
    assert _lib.version() == 106 and C["SPK_VERSION"] == 106
    names = ("spk_psample_step_conf_sched", "spk_psample_step_conf_listed_sched", "spk_den_step_tail_conf_sched")
    for n in names:
        assert n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None
    sig = dict(zip(names, (len(getattr(_lib.lib, n).argtypes) for n in names)))
    assert sig == {"spk_psample_step_conf_sched": 23, "spk_psample_step_conf_listed_sched": 26, "spk_den_step_tail_conf_sched": 37}
    # the siblings plus four (the listed one has S already: plus three)
    assert len(_lib.lib.spk_psample_step_conf.argtypes) == 19 and len(_lib.lib.spk_psample_step_conf_listed.argtypes) == 23
    assert len(_lib.lib.spk_den_step_tail_conf.argtypes) == 33
    lib, P = _lib.lib, 0x1000                                        # (a non-null pointer: refused calls never touch it)
    ARG, UNS = C["SPK_ERR_ARG"], C["SPK_ERR_UNSUPPORTED"]
    # logits, x_t, unmasked, t, temp_b, topk_b, topp_b, u, q, seed, offset, state, x0_hat, conf, B, HW, K, next_input, sched_w,
    # noise_a, S, score_out, stream
    good = [P, P, P, 2, P, P, P, None, None, 1, 0, None, None, None, 4, 49, 128, None, P, None, 5, None, None]
    for i in (0, 1, 2, 4, 5, 6, 18):                                  # (18: a null sched_w)
        bad = list(good)
        bad[i] = None
        assert lib.spk_psample_step_conf_sched(*bad) == ARG, i
    for i, v in ((3, 0), (3, 6), (3, -1), (14, 0), (15, 0), (16, 0), (20, 0), (20, 1)):     # t < 1, t > S, B, HW, K, S < 1, S < t
        bad = list(good)
        bad[i] = v
        assert lib.spk_psample_step_conf_sched(*bad) == ARG, (i, v)
    for i, v in ((15, 65), (16, 2049)):
        bad = list(good)
        bad[i] = v
        assert lib.spk_psample_step_conf_sched(*bad) == UNS, (i, v)
    # the listed form: ... B, HW, K, steps_b, S, stride, active, n_active, sched_w, noise_a, score_out, stream
    good = [P, P, P, 2, P, P, P, None, None, 1, 0, None, None, None, 4, 49, 128, P, 5, 1 << 40, P, P, P, None, None, None]
    for i in (0, 1, 2, 4, 5, 6, 17, 20, 21, 22):
        bad = list(good)
        bad[i] = None
        assert lib.spk_psample_step_conf_listed_sched(*bad) == ARG, i
    for i, v in ((3, 0), (3, 6), (14, 0), (15, 0), (16, 0), (18, 0)):
        bad = list(good)
        bad[i] = v
        assert lib.spk_psample_step_conf_listed_sched(*bad) == ARG, (i, v)
    for i, v in ((15, 65), (16, 2049)):
        bad = list(good)
        bad[i] = v
        assert lib.spk_psample_step_conf_listed_sched(*bad) == UNS, (i, v)
    # the step tail: cnt5, nch5, cnt1, nch1, wq, scale, bias, logits, x_t, unmasked, t, temp_b, topk_b, topp_b, u, q, seed, offset,
    # state, w1, b1, bn_a, bn_b, x1, cnt1_out, T, B, H, W, K, x0_hat, conf, sched_w, noise_a, S, score_out, stream
    good = [P, 8, P, 2, P, P, P, None, P, P, 2, P, P, P, None, None, 1, 0, None, None, None, None, None, None, None, 16, 4, 7, 7, 128,
            None, None, P, None, 5, None, None]
    for i in (0, 2, 4, 5, 6, 8, 9, 11, 12, 13, 32):                    # (32: a null sched_w)
        bad = list(good)
        bad[i] = None
        assert lib.spk_den_step_tail_conf_sched(*bad) == ARG, i
    for i, v in ((10, 0), (10, 6), (34, 0), (34, 1), (26, 0)):          # t < 1, t > S, S < 1, S < t, B
        bad = list(good)
        bad[i] = v
        assert lib.spk_den_step_tail_conf_sched(*bad) == ARG, (i, v)
    for i, v in ((27, 9), (29, 513), (1, 7)):                          # a 9 x 7 latent (HW > 64 among them), K, nch5
        bad = list(good)
        bad[i] = v
        assert lib.spk_den_step_tail_conf_sched(*bad) == UNS, (i, v)


def test_wrappers_exist_with_the_siblings_arguments():
    from spkdiff import ops
    for name, sib in (("psample_step_conf_sched", "psample_step_conf"), ("psample_step_conf_listed_sched", "psample_step_conf_listed"),
                      ("den_step_tail_conf_sched", "den_step_tail_conf")):
        new, old = inspect.signature(getattr(ops, name)).parameters, inspect.signature(getattr(ops, sib)).parameters
        assert set(old) <= set(new) and set(new) - set(old) <= {"sched_w", "noise_a", "S", "score"}, name
        assert {"sched_w", "noise_a", "score"} <= set(new)


# ------------------------------------------------------------------------------------------------- the Python arguments
def test_sampler_builds_both_tables_on_the_host_and_refuses_bad_arguments():
    from snn_model.vq_diffusion import AbsorbingDiffusion as AD
    w, a = AD._sched_arg("cosine", 4.5, 3, [8, 8, 8], 8)
    assert w.dtype == torch.int32 and a.dtype == torch.float32 and tuple(w.shape) == tuple(a.shape) == (3, 9)
    assert w.tolist() == [cso.cosine_weights(8)] * 3 and a.tolist() == [cso.noise_row(4.5, 8, 8)] * 3
    assert bool((a[:, 1] == 0).all()) and bool((a[:, 0] == 0).all())
    # per-image steps: row i for e_i
    w, a = AD._sched_arg("cosine", [0.0, 1.0, 4.5], 3, [3, 8, 5], 8)
    for i, e in enumerate((3, 8, 5)):
        assert w[i, :e + 1].tolist() == cso.cosine_weights(e) and a[i].tolist() == cso.noise_row((0.0, 1.0, 4.5)[i], e, 8)
    # defaults inside a scheduled call: the linear table, no noise
    w, a = AD._sched_arg(None, None, 2, [4, 4], 4)
    assert w.tolist() == [[0, 1, 2, 3, 4]] * 2 and not bool(a.any())
    w, _ = AD._sched_arg("linear", 0, 2, [4, 2], 4)
    assert w.tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 2, 2]]
    # one table for every image, per-image entries, a 2-D array, a tensor
    tab = [0, 3, 3, 9, W_MAX]
    assert AD._sched_arg(tab, None, 2, [4, 4], 4)[0].tolist() == [tab] * 2
    assert AD._sched_arg(tuple(tab), None, 2, [4, 4], 4)[0].tolist() == [tab] * 2
    assert AD._sched_arg(torch.tensor(tab), None, 2, [4, 4], 4)[0].tolist() == [tab] * 2
    assert AD._sched_arg(np.array([tab, tab[::-1]]), None, 2, [4, 4], 4)[0].tolist() == [tab, tab[::-1]]
    mixed = AD._sched_arg(["cosine", None, tab], torch.tensor([1.0, 2.0, 3.0]), 3, [4, 4, 4], 4)
    assert mixed[0].tolist() == [cso.cosine_weights(4), cso.linear_weights(4), tab] and mixed[1][:, 4].tolist() == [0.75, 1.5, 2.25]
    for kw in (dict(selection_noise=-1.0), dict(selection_noise=float("nan")), dict(selection_noise=float("inf")),
               dict(selection_noise=[1.0, 2.0]), dict(selection_noise=[1.0, -2.0, 0.0]), dict(selection_noise="much"),
               dict(selection_noise=1e39), dict(schedule="sine"), dict(schedule=[0, 1, 2]), dict(schedule=[0, 1, 2, 3, 4, 5]),
               dict(schedule=[0, 1, 2, 3, W_MAX + 1]), dict(schedule=[0, 1, 2, 3, -4]), dict(schedule=[0.0, 1.0, 2.0, 3.0, 4.0]),
               dict(schedule=torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0])), dict(schedule=["cosine", "cosine"]),
               dict(schedule=["cosine", "linear", "sine"]), dict(schedule=[tab, tab]), dict(schedule=np.zeros((3, 4), dtype=np.int64)), dict(schedule=7),
               dict(schedule=np.zeros((3, 5), dtype=np.float32)), dict(schedule=torch.ones(5, dtype=torch.bool)), dict(schedule={0: 1})):
        with pytest.raises(ValueError):
            AD._sched_arg(kw.get("schedule"), kw.get("selection_noise"), 3, [4, 4, 4], 4)


def _sampler_on_cpu():
    from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel, functional
    torch.manual_seed(0)
    dn = DummyModel(1, 128).eval()
    functional.set_step_mode(dn, 'm')
    ab = AbsorbingDiffusion(dn, mask_id=128, latent_shape=(7, 7))
    ab.n_samples, ab.verify_weights = 2, False
    return ab


def test_sample_confident_refuses_bad_tables_before_a_key_is_drawn(monkeypatch):
    ab = _sampler_on_cpu()
    state = torch.get_rng_state()
    for kw in (dict(selection_noise=-1.0), dict(selection_noise=float("nan")), dict(schedule="sine"), dict(schedule=[0, 1, 2]),
               dict(schedule=[0, 1, 2, W_MAX + 1]), dict(schedule=["cosine"] * 3), dict(selection_noise=[1.0] * 3)):
        with pytest.raises(ValueError):
            ab.sample_confident(3, **kw)
    assert torch.equal(torch.get_rng_state(), state) and len(ab._graphs) == 0
    # score() takes neither
    assert not {"schedule", "selection_noise"} & set(inspect.signature(ab.score).parameters)
    assert {"schedule", "selection_noise"} <= set(inspect.signature(ab.sample_confident).parameters)


def test_pass_through_arguments_exist():
    from spkdiff.complete import complete_images_confident
    from spkdiff.dist import complete_images_sharded
    from spkdiff.evaluate import step_count_sweep
    for f in (complete_images_confident, complete_images_sharded, step_count_sweep):
        p = inspect.signature(f).parameters
        assert p["schedule"].default is None and p["selection_noise"].default is None, f.__name__


# ------------------------------------------------------------------------------------------------- the launch sequence
UPDATES = ("psample_step_conf", "psample_step_conf_listed", "den_step_tail_conf", "psample_step_conf_sched",
           "psample_step_conf_listed_sched", "den_step_tail_conf_sched")


def _record_updates(monkeypatch):
    """On top of the recorders of tests/_dispatch_recorders.py: the six confidence-ordered token updates and select_pending, logged
    with every argument they were given."""
    from spkdiff import ops
    calls = []

    def fake(name):
        sig = inspect.signature(getattr(ops, name))

        def rec(*args, **kwargs):
            a = sig.bind(*args, **kwargs)
            calls.append((name, dict(a.arguments)))
            if name.startswith("den_step_tail"):
                cnt5 = a.arguments["cnt5"]
                Bn, _, H, W, _ = cnt5.shape
                nxt = None if a.arguments.get("conv1") is None else (torch.zeros((Bn, 2, H, W, 16, 16), dtype=ops.C4_DTYPE),
                                                                    torch.zeros((Bn, 2, H, W, 32), dtype=torch.uint8))
                return nxt, None
            return a.arguments["x_t"], a.arguments["unmasked"]
        return rec
    for name in UPDATES:
        monkeypatch.setattr(ops, name, fake(name))
    monkeypatch.setattr(ops, "select_pending", lambda unmasked, t, steps_b, out=None: out if out is not None else (
        torch.zeros(unmasked.shape[0], dtype=torch.int32), torch.zeros(2, dtype=torch.int32)))
    return calls


def _same(a, b):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return a is b or (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a, b))
    return a == b


@pytest.mark.parametrize("tail", [True, False], ids=["tail", "three_launches"])
@pytest.mark.parametrize("per_image", [False, True], ids=["dense", "listed"])
@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph_body"])
def test_defaults_issue_the_calls_made_before_and_anything_else_the_sched_family(monkeypatch, tail, per_image, captured):
    """The step loop driven on CPU tensors through the recorders, three steps.  Without tables: psample_step_conf /
    psample_step_conf_listed / den_step_tail_conf and nothing else, with exactly the arguments of a loop that knows no schedule.
    With tables: their ``_sched`` siblings at the same places with the same arguments plus the two tables and S."""
    from _dispatch_recorders import _install_recorders
    from snn_model.vq_diffusion import SampleForm, _SamplerGraph
    Bn, S = 2, 3
    ab = _sampler_on_cpu()
    ab._denoise_fn.use_step_tail = tail
    cpu = torch.device("cpu")
    form = SampleForm(skip=per_image, lists=False, tail=tail and not per_image, tail_act=False)
    tv, kd, pd = torch.ones(Bn), torch.zeros(Bn, dtype=torch.int32), torch.ones(Bn)
    steps = torch.tensor([2, 3], dtype=torch.int32) if per_image else None
    sched = (torch.tensor([[0, 1, 2, 2], [0, 1, 2, 3]], dtype=torch.int32), torch.zeros(Bn, S + 1))
    logs = {}
    for name, sc in (("plain", None), ("sched", sched)):
        with monkeypatch.context() as mp:
            _install_recorders(mp, sampler=True)
            calls = _record_updates(mp)
            kw = dict(top_k=kd, top_p=pd, confident=True, **({} if steps is None else {"steps_b": steps}),
                      **({} if sc is None else {"sched": sc}))
            with torch.no_grad():
                if captured:
                    g = _SamplerGraph(cpu, Bn, 7, 7, form, int(ab.list_radii), False, top_p=True, confident=True,
                                      **({} if steps is None else {"per_image_steps": True}),
                                      **({} if sc is None else {"sched_steps": S}))
                    assert (g.sched is None) == (sc is None)
                    if sc is not None:
                        assert tuple(g.sched[0].shape) == tuple(g.sched[1].shape) == (Bn, S + 1)
                        assert g.sched[0].dtype == torch.int32 and g.sched[1].dtype == torch.float32
                    ab._graph_body(g, form, tv, S)
                else:
                    ab._sample_eager(cpu, Bn, 7, 7, form, tv, S, None, 5, None, None, **kw)
            logs[name] = calls
    want = "den_step_tail_conf" if form.tail else "psample_step_conf_listed" if per_image else "psample_step_conf"
    assert [c[0] for c in logs["plain"]] == [want] * S
    assert [c[0] for c in logs["sched"]] == [want + "_sched"] * S
    for (_, old), (_, new) in zip(logs["plain"], logs["sched"]):
        extra = set(new) - set(old)
        assert extra == {"sched_w", "noise_a", "S"} - set(old), extra
        assert int(new["S"]) == S and tuple(new["sched_w"].shape) == (Bn, S + 1) and tuple(new["noise_a"].shape) == (Bn, S + 1)
        if not captured:
            assert new["sched_w"] is sched[0] and new["noise_a"] is sched[1]
        for k, v in old.items():
            if k in ("cnt5", "cnt1", "packed6", "conv1", "logits", "x_t", "unmasked", "philox_state", "next_input", "temp", "top_k",
                     "top_p", "steps_b"):
                assert (v is None) == (new[k] is None), k                # (buffers of the two runs: given or not, alike)
            else:
                assert _same(v, new[k]), (k, v, new[k])
    # the arguments of the plain calls name no table: the loop hands on what it handed on before
    for _, old in logs["plain"]:
        assert not {"sched_w", "noise_a", "score"} & set(old)


def test_sample_confident_hands_its_defaults_on_unchanged(monkeypatch):
    ab = _sampler_on_cpu()
    seen = []
    monkeypatch.setattr(ab, "_sample_call", lambda *a, **kw: seen.append((a, kw)) or "tokens")
    assert ab.sample_confident(5, temp=0.7, top_k=3) == "tokens"
    assert seen[-1] == ((0.7, 5, None, None, None, None, 3, None), {"confident": True}), "the call made before, argument for argument"
    ab.sample_confident(5, schedule="cosine")
    assert seen[-1][1] == {"confident": True, "schedule": "cosine", "selection_noise": None, "scheduled": True}
    ab.sample_confident(5, selection_noise=4.5)
    assert seen[-1][1] == {"confident": True, "schedule": None, "selection_noise": 4.5, "scheduled": True}
    ab.sample_confident(5, schedule="linear")
    assert seen[-1][1]["scheduled"] is True
