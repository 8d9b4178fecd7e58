"""Host tests of remasking for confidence-ordered decoding (no device): the rule's oracle against itself (literal sort
== rank mirror), the count trajectory and its invariants, the package's host builders against the oracle, every refusal, and the three
C entry points -- declared, resolved and refusing bad arguments before any launch."""
import inspect

import numpy as np
import pytest
import torch

import _confident_oracle as cfo
import _confident_remask_oracle as cro
import _confident_sched_oracle as cso

INF = float("inf")


# ------------------------------------------------------------------------------------------------- the rule
def test_literal_sort_remask_equals_the_rank_mirror():
    g = np.random.default_rng(5)
    for trial in range(300):
        HW = int(g.choice([1, 2, 7, 49, 64]))
        rev = g.random(HW) < g.random()
        cc = (-g.random(HW) * 9).astype(np.float32)
        kind = trial % 4
        if kind == 1:                                              # heavy ties (top_k = 1: every confidence is exactly 0)
            cc = g.choice(np.array([0.0, -0.0, -1.5], dtype=np.float32), HW)
        elif kind == 2:                                            # specials: NaN first, then -inf; +inf orders last among these
            cc[g.random(HW) < 0.3] = np.nan
            cc[g.random(HW) < 0.2] = -np.inf
            cc[g.random(HW) < 0.1] = np.inf
        elif kind == 3:
            cc[:] = cc[0]
        for r in (0, 1, 2, int(rev.sum()) // 2, int(rev.sum()), 64):
            r = min(r, int(rev.sum()))
            a, b = cro.remask_by_sort(rev, cc, r), cro.remask_by_rank(rev, cc, r)
            assert (a == b).all() and int(a.sum()) == r and not (a & ~rev).any(), (trial, r)
    # ties go to the higher position, a NaN before everything, -0.0 and +0.0 are different keys (as in the reveal)
    rev = np.ones(8, dtype=bool)
    assert cro.remask_by_sort(rev, np.zeros(8, np.float32), 3).nonzero()[0].tolist() == [5, 6, 7]
    cc = np.array([-1, -2, np.nan, -np.inf, -2, 0, -3, -1], dtype=np.float32)
    assert cro.remask_by_sort(rev, cc, 1).nonzero()[0].tolist() == [2]
    assert cro.remask_by_sort(rev, cc, 2).nonzero()[0].tolist() == [2, 3]
    assert cro.remask_by_sort(rev, cc, 4).nonzero()[0].tolist() == [2, 3, 4, 6]
    # +inf is not revisable, a NaN is; a masked position is not
    un = np.array([1, 1, 1, 0], dtype=bool)
    assert cro.revisable_of(un, np.array([np.inf, np.nan, -1.0, -1.0], np.float32)).tolist() == [False, True, True, False]
    # the mirror image of the reveal: one total order serves both ends
    keys = cfo.conf_key(cc)
    order = sorted(range(8), key=lambda p: (int(keys[p]), -p))
    assert order == sorted(range(8), key=lambda p: (-int(keys[p]), p))[::-1]
    assert cro.remask_count(5, 3, 2, 4) == 3 and cro.remask_count(5, 3, 1, 4) == 0 and cro.remask_count(5, 3, 2, 0) == 0


def _tables(e):
    bump = [t * 5 + 1 for t in range(e + 1)]
    bump[0] = 0
    for t in range(2, e + 1, 3):
        bump[t - 1] = bump[t] + 7                                  # (non-monotone: w[t - 1] > w[t])
    return {"linear": cso.linear_weights(e), "cosine": cso.cosine_weights(e), "bump": bump}


@pytest.mark.parametrize("e", [1, 2, 5, 8, 12, 60])
def test_the_count_trajectory_and_its_invariants(e):
    from spkdiff import schedules as sch
    g = np.random.default_rng(e)
    for name, w in _tables(e).items():
        for m0 in (0, 1, 7, 49, 64):
            rows = [[0] * (e + 1), [0, 0] + [1] * (e - 1), [0, 0] + [64] * (e - 1), [0, 0] + g.integers(0, 65, max(e - 1, 0)).tolist()]
            for R in rows:
                R = R[:e + 1]
                traj = cro.run_counts_remask(m0, w, R)
                assert len(traj) == e
                m, sn, sr = m0, 0, 0
                for t, (n, r) in zip(range(e, 0, -1), traj):
                    assert n == cso.reveal_count(m, w[t - 1], w[t]) and 0 <= n <= m
                    assert r <= m0 - m and r <= R[t] and (t >= 2 or r == 0), "r_t <= m0 - m_t, and nothing at t = 1"
                    m = m - n + r
                    sn, sr = sn + n, sr + r
                assert m == 0, f"no masked position after t = 1 ({name}, m0 = {m0}, R = {R})"
                assert sn == m0 + sr, "sum n = m0 + sum r"
                assert traj == sch.run_counts_remask(m0, w, R), "the package's trajectory is the oracle's"
            assert [n for n, _ in cro.run_counts_remask(m0, w, [0] * (e + 1))] == cso.run_counts(m0, w), "a zero table: the `_sched` counts"
            if e >= 2:
                assert sch.run_counts_remask(m0, w, 3) == cro.run_counts_remask(m0, w, [0, 0] + [3] * (e - 1)), "an int is every t >= 2"


def test_a_step_on_host_copies_follows_the_rule():
    g = torch.Generator().manual_seed(3)
    Bn, HW, K, t = 4, 49, 16, 3
    un = torch.rand(Bn, HW, generator=g) < 0.5
    un[3] = True                                                   # m = 0: untouched, revisable tokens or not
    x = torch.where(un, torch.randint(0, K, (Bn, HW), generator=g), torch.full((Bn, HW), K))
    cc = -torch.rand(Bn, HW, generator=g)
    cc[0, un[0].nonzero().flatten()[:3]] = INF
    cand = torch.randint(0, K, (Bn, HW), generator=g)
    conf = -torch.rand(Bn, HW, generator=g)
    x1, un1, cc1, rev, rem, counts = cro.remask_state(x, un, cc, cand, conf, conf, [2] * Bn, [3] * Bn, [4, 64, 0, 9], t, K)
    for b in range(Bn):
        m = int((~un[b]).sum())
        assert counts[b][0] == cfo.n_reveal(m, t) == int(rev[b].sum())
        assert not bool((rev[b] & rem[b]).any()) and bool((rem[b] <= un[b]).all()), "a position revealed in the step is not remasked in it"
        assert bool((x1[b][rem[b]] == K).all()) and not bool(un1[b][rem[b]].any()) and torch.equal(cc1[b][rem[b]], cc[b][rem[b]])
        assert torch.equal(cc1[b][rev[b]], conf[b][rev[b]]) and torch.equal(cc1[b][~rev[b]], cc[b][~rev[b]])
        assert not bool((rem[b] & (cc[b] == INF)).any())
    assert counts[1][1] == int((un[1]).sum()) and counts[2][1] == 0 and counts[3] == (0, 0) and counts[0][1] == 4
    assert torch.equal(x1[3], x[3]) and bool(un1[3].all())
    _, _, _, _, rem1, c1 = cro.remask_state(x, un, cc, cand, conf, conf, [0] * Bn, [1] * Bn, [4, 64, 0, 9], 1, K)
    assert int(rem1.sum()) == 0 and all(r == 0 for _, r in c1), "t = 1 remasks nothing"


# ------------------------------------------------------------------------------------------------- the package's host side
def test_remask_row_placement_and_refusals():
    from spkdiff import schedules as sch
    assert sch.remask_row(None, 4, 4) == [0] * 5 and sch.remask_row(0, 4, 4) == [0] * 5
    assert sch.remask_row(3, 4, 4) == [0, 0, 3, 3, 3]
    assert sch.remask_row(3, 2, 6) == [0, 0, 3, 0, 0, 0, 0], "an image with e < S: its own row in entries 0 .. e, zeros above"
    assert sch.remask_row(3, 1, 3) == [0, 0, 0, 0]
    assert sch.remask_row([0, 0, 5, 1], 3, 6) == [0, 0, 5, 1, 0, 0, 0]
    assert sch.remask_row((0, 0, 5, 1, 0, 0, 0), 3, 6) == [0, 0, 5, 1, 0, 0, 0]
    assert sch.remask_row(np.array([0, 0, 2]), 2, 2) == [0, 0, 2] and sch.remask_row(np.int64(2), 3, 3) == [0, 0, 2, 2]
    for bad in (-1, 1.5, True, "2", [0, 0, 1], [0, 0, 1, 1, 1, 1], [0, 1, 1, 1], [1, 0, 1, 1], [0, 0, -1, 1], [0, 0, 1.0, 1], [0, 0, True, 1],
                [0, 0, 1, 1, 0, 0, 1], {0: 1}):
        with pytest.raises(ValueError):
            sch.remask_row(bad, 3, 6)
    with pytest.raises(ValueError):
        sch.remask_row(1, 7, 6)
    with pytest.raises(ValueError):
        sch.remask_row(1, 0, 6)


def test_sampler_builds_the_table_on_the_host_and_refuses_bad_arguments():
    from snn_model.vq_diffusion import AbsorbingDiffusion as AD
    r = AD._remask_arg(2, 3, [4, 4, 4], 4)
    assert r.dtype == torch.int32 and r.tolist() == [[0, 0, 2, 2, 2]] * 3
    assert AD._remask_arg(0, 2, [4, 4], 4).tolist() == [[0] * 5] * 2
    tab = [0, 0, 7, 1, 3]
    for form in (tab, tuple(tab), torch.tensor(tab), np.array(tab)):
        assert AD._remask_arg(form, 2, [4, 4], 4).tolist() == [tab] * 2
    assert AD._remask_arg([1, None, tab], 3, [4, 4, 4], 4).tolist() == [[0, 0, 1, 1, 1], [0] * 5, tab]
    assert AD._remask_arg(np.array([tab, tab[::-1][:0] + [0, 0, 1, 1, 1]]), 2, [4, 4], 4).tolist() == [tab, [0, 0, 1, 1, 1]]
    assert AD._remask_arg(torch.tensor(3), 1, [2], 2).tolist() == [[0, 0, 3]]
    # per-image step counts: row i for e_i, placed as a schedule row is
    assert AD._remask_arg(2, 3, [4, 2, 1], 4).tolist() == [[0, 0, 2, 2, 2], [0, 0, 2, 0, 0], [0] * 5]
    assert AD._remask_arg([[0, 0, 9], 1, [0, 0, 1, 2, 3]], 3, [2, 3, 4], 4).tolist() == [[0, 0, 9, 0, 0], [0, 0, 1, 1, 0], [0, 0, 1, 2, 3]]
    for bad in (-1, 1.5, True, "two", [0, 0, 1], [0, 1, 1, 1, 1], [1, 0, 1, 1, 1], [0, 0, -1, 1, 1], [0, 0, 1.0, 1, 1], [tab, tab],
                [tab] * 4, torch.ones(3, 5), np.zeros((3, 4), dtype=np.int64), np.zeros((2, 3, 5), dtype=np.int64),
                torch.ones(5, dtype=torch.bool), [2, None], {0: 1}):
        with pytest.raises(ValueError):
            AD._remask_arg(bad, 3, [4, 4, 4], 4)


def _sampler_on_cpu():
    from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel, functional
    torch.manual_seed(0)
    dn = DummyModel(1, 128).eval()
    functional.set_step_mode(dn, 'm')
    ab = AbsorbingDiffusion(dn, mask_id=128, latent_shape=(7, 7))
    ab.n_samples, ab.verify_weights = 2, False
    return ab


def test_sample_confident_refuses_bad_tables_before_a_key_is_drawn():
    ab = _sampler_on_cpu()
    state = torch.get_rng_state()
    for rm in (-1, 1.5, [0, 0, 1], [0, 1, 1, 1], [0, 0, -2, 1], [[0, 0, 1, 1]] * 3, "r"):
        with pytest.raises(ValueError):
            ab.sample_confident(3, remask=rm)
    assert torch.equal(torch.get_rng_state(), state) and len(ab._graphs) == 0
    assert "remask" not in inspect.signature(ab.score).parameters, "score() takes no such argument"
    assert inspect.signature(ab.sample_confident).parameters["remask"].default is None
    assert "remask" in inspect.signature(type(ab._denoise_fn).sample_step).parameters


def test_pass_through_arguments_exist():
    from spkdiff.complete import complete_images_confident
    from spkdiff.dist import complete_images_sharded
    from spkdiff.evaluate import step_count_sweep
    for f in (complete_images_confident, complete_images_sharded, step_count_sweep):
        assert inspect.signature(f).parameters["remask"].default is None, f.__name__


def test_wrappers_exist_with_the_siblings_arguments():
    from spkdiff import ops
    for name, sib in (("psample_step_conf_remask", "psample_step_conf_sched"),
                      ("psample_step_conf_listed_remask", "psample_step_conf_listed_sched"),
                      ("den_step_tail_conf_remask", "den_step_tail_conf_sched")):
        new, old = inspect.signature(getattr(ops, name)).parameters, inspect.signature(getattr(ops, sib)).parameters
        assert set(old) <= set(new) and set(new) - set(old) == {"remask_r", "commit_conf", "mask_id", "remasked"}, name


def test_none_issues_the_calls_made_before(monkeypatch):
    """``remask=None`` hands nothing new down: _sample_call sees the arguments it saw, launch for launch."""
    ab = _sampler_on_cpu()
    seen = []
    monkeypatch.setattr(type(ab), "_sample_call", lambda self, *a, **kw: seen.append((a, kw)))
    ab.sample_confident(4)
    ab.sample_confident(4, remask=None)
    ab.sample_confident(4, schedule="cosine")
    ab.sample_confident(4, schedule="cosine", remask=None)
    ab.sample_confident(4, remask=0)
    assert seen[0] == seen[1] and seen[2] == seen[3]
    assert "remask" not in seen[0][1] and "scheduled" not in seen[0][1] and "remask" not in seen[2][1]
    assert seen[4][1]["remask"] == 0 and seen[4][1]["scheduled"] is True and seen[4][1]["schedule"] is None


# ------------------------------------------------------------------------------------------------- the C entry points
def test_entry_points_are_declared_resolved_and_refuse_bad_arguments_without_a_device():
    from spkdiff import _lib
    C = _lib.CONSTANTS
    assert _lib.version() == 106 and C["SPK_VERSION"] == 106
    names = ("spk_psample_step_conf_remask", "spk_psample_step_conf_listed_remask", "spk_den_step_tail_conf_remask")
    for n in names:
        assert n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None
    sig = dict(zip(names, (len(getattr(_lib.lib, n).argtypes) for n in names)))
    # the `_sched` siblings plus four
    assert sig == {"spk_psample_step_conf_remask": 27, "spk_psample_step_conf_listed_remask": 30, "spk_den_step_tail_conf_remask": 41}
    assert len(_lib.lib.spk_psample_step_conf_sched.argtypes) == 23 and len(_lib.lib.spk_psample_step_conf_listed_sched.argtypes) == 26
    assert len(_lib.lib.spk_den_step_tail_conf_sched.argtypes) == 37
    lib, P = _lib.lib, 0x1000                                        # (a non-null pointer: refused calls never touch it)
    ARG, UNS = C["SPK_ERR_ARG"], C["SPK_ERR_UNSUPPORTED"]
    # logits, x_t, unmasked, t, temp_b, topk_b, topp_b, u, q, seed, offset, state, x0_hat, conf, B, HW, K, next_input, sched_w,
    # noise_a, S, score_out, remask_r, commit_conf, mask_id, remasked_out, stream
    good = [P, P, P, 2, P, P, P, None, None, 1, 0, None, None, None, 4, 49, 128, None, P, None, 5, None, P, P, 128, None, None]
    for i in (0, 1, 2, 4, 5, 6, 18, 22, 23):                          # (18: a null sched_w; 22: a null table; 23: a null commit_conf)
        bad = list(good)
        bad[i] = None
        assert lib.spk_psample_step_conf_remask(*bad) == ARG, i
    for i, v in ((3, 0), (3, 6), (14, 0), (15, 0), (16, 0), (20, 0), (20, 1), (24, 0), (24, 127), (24, 64)):   # .., t > S, .., mask_id in [0, K)
        bad = list(good)
        bad[i] = v
        assert lib.spk_psample_step_conf_remask(*bad) == ARG, (i, v)
    for i, v in ((15, 65), (16, 2049)):
        bad = list(good)
        bad[i] = v
        bad[24] = 4096
        assert lib.spk_psample_step_conf_remask(*bad) == UNS, (i, v)
    # the listed form: ... B, HW, K, steps_b, S, stride, active, n_active, sched_w, noise_a, score_out, remask_r, commit_conf, mask_id,
    # remasked_out, stream
    good = [P, P, P, 2, P, P, P, None, None, 1, 0, None, None, None, 4, 49, 128, P, 5, 1 << 40, P, P, P, None, None, P, P, -1, None, None]
    for i in (0, 1, 2, 4, 5, 6, 17, 20, 21, 22, 25, 26):
        bad = list(good)
        bad[i] = None
        assert lib.spk_psample_step_conf_listed_remask(*bad) == ARG, i
    for i, v in ((3, 0), (3, 6), (14, 0), (15, 0), (16, 0), (18, 0), (27, 0), (27, 127)):
        bad = list(good)
        bad[i] = v
        assert lib.spk_psample_step_conf_listed_remask(*bad) == ARG, (i, v)
    for i, v in ((15, 65), (16, 2049)):
        bad = list(good)
        bad[i] = v
        assert lib.spk_psample_step_conf_listed_remask(*bad) == UNS, (i, v)
    # the step tail: cnt5, nch5, cnt1, nch1, wq, scale, bias, logits, x_t, unmasked, t, temp_b, topk_b, topp_b, u, q, seed, offset,
    # state, w1, b1, bn_a, bn_b, x1, cnt1_out, T, B, H, W, K, x0_hat, conf, sched_w, noise_a, S, score_out, remask_r, commit_conf,
    # mask_id, remasked_out, stream
    good = [P, 8, P, 2, P, P, P, None, P, P, 2, P, P, P, None, None, 1, 0, None, None, None, None, None, None, None, 16, 4, 7, 7, 128,
            None, None, P, None, 5, None, P, P, 128, None, None]
    for i in (0, 2, 4, 5, 6, 8, 9, 11, 12, 13, 32, 36, 37):
        bad = list(good)
        bad[i] = None
        assert lib.spk_den_step_tail_conf_remask(*bad) == ARG, i
    for i, v in ((10, 0), (10, 6), (34, 0), (34, 1), (26, 0), (38, 0), (38, 127)):     # t < 1, t > S, S < 1, S < t, B, mask_id in [0, K)
        bad = list(good)
        bad[i] = v
        assert lib.spk_den_step_tail_conf_remask(*bad) == ARG, (i, v)
    for i, v in ((27, 9), (29, 513), (1, 7)):
        bad = list(good)
        bad[i] = v
        bad[38] = 4096
        assert lib.spk_den_step_tail_conf_remask(*bad) == UNS, (i, v)
