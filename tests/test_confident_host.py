"""CPU tests of confidence-ordered decoding: the oracle of tests/_confident_oracle.py against itself -- the literal
sort loop against the mirror of the kernel's key / rank arithmetic on the whole case table --, the schedule, tie and NaN ordering, the
arithmetic of the counted bound, and the condition the GPU test puts on the table's top-p rows.  No device."""
import math

import numpy as np
import pytest
import torch

import _confident_oracle as cfo
import _topp_oracle as tpo


def _host_conf(zt, g):
    """A host stand-in for the kernel's outputs on truncated rows: a candidate drawn from the kept classes and its fp32 confidence."""
    kept = torch.isfinite(zt)
    w = torch.where(kept, torch.rand(zt.shape, generator=g), torch.full_like(zt, -1.0))
    tok = w.argmax(-1)
    return tok, cfo.log_prob_f64(zt, tok).float()


@pytest.mark.parametrize("HW", cfo.HWS)
@pytest.mark.parametrize("K", cfo.KS)
def test_sort_loop_equals_the_rank_mirror_on_the_whole_table(K, HW):
    logits, q, x0, un0, temps, ks, ps = cfo.conf_inputs(K, HW)
    z32, zt, fcut, on = cfo.reference_rows(logits, temps, ks, ps)
    g = torch.Generator().manual_seed(K + HW)
    tok, conf = _host_conf(zt, g)
    x, un = x0.reshape(cfo.B, HW), un0.reshape(cfo.B, HW)
    assert [int((~un[b]).sum()) for b in range(cfo.B)] == cfo.masked_counts(HW)
    for t in cfo.steps_of(HW):
        a = cfo.commit_state(x, un, tok.reshape(cfo.B, HW), conf.reshape(cfo.B, HW), t, commit=cfo.commit_by_sort)
        b = cfo.commit_state(x, un, tok.reshape(cfo.B, HW), conf.reshape(cfo.B, HW), t, commit=cfo.commit_by_rank)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), (K, HW, t)
        rev = a[2]
        for i, m in enumerate(cfo.masked_counts(HW)):
            assert int(rev[i].sum()) == cfo.n_reveal(m, t) and not bool((rev[i] & un[i]).any())
        # what is not revealed keeps its state
        assert torch.equal(a[0][~rev], x[~rev]) and torch.equal(a[1], un | rev)


def test_schedule():
    assert [cfo.n_reveal(49, t) for t in (1, 49, 50, 100)] == [49, 1, 1, 1] and cfo.n_reveal(0, 5) == 0
    for steps in (1, 2, 5, 8, 12, 16, 48, 49, 50, 60, 100):
        for m0 in (0, 1, 2, 7, 48, 49, 63, 64):
            m, ns = m0, []
            for t in range(steps, 0, -1):
                n = cfo.n_reveal(m, t)
                assert 0 <= n <= m and (n >= 1 or m == 0)
                if t >= m > 0:
                    assert n == 1                                # t >= m: one per step
                ns.append(n)
                m -= n
            assert m == 0 and sum(ns) == m0                      # t = 1 reveals what is left: the counts sum to m
    seq, m = [], 49
    for t in range(8, 0, -1):
        seq.append(cfo.n_reveal(m, t))
        m -= seq[-1]
    assert seq == [7, 6, 6, 6, 6, 6, 6, 6]
    seq, m = [], 49
    for t in range(49, 0, -1):
        seq.append(cfo.n_reveal(m, t))
        m -= seq[-1]
    assert seq == [1] * 49


def test_ties_go_to_the_lower_position_and_nan_orders_last():
    nan, inf = float("nan"), float("inf")
    conf = np.array([-1.0, -0.5, -0.5, nan, -0.5, -inf, -0.0, 0.0, nan, -2.0], dtype=np.float32)
    masked = np.ones(10, dtype=bool)
    # keys: +0.0 above -0.0 (the keys of truncate_top_k order the bit patterns), then -0.5 three times, -1, -2, -inf, the NaNs
    want = [7, 6, 1, 2, 4, 0, 9, 5, 3, 8]
    key = cfo.conf_key(conf)
    assert key[3] == key[8] == 0 and key[5] > 0 and key[7] > key[6] > key[1] == key[2] == key[4]
    for n in range(1, 11):
        # m = 10, t chosen so that ceil(10 / t) = n where such a t exists
        ts = [t for t in range(1, 11) if cfo.n_reveal(10, t) == n]
        for t in ts:
            for commit in (cfo.commit_by_sort, cfo.commit_by_rank):
                assert sorted(np.flatnonzero(commit(masked, conf, t))) == sorted(want[:n]), (n, t)
    # the cut inside a tie group: n = 4 takes positions 1 and 2 of the three at -0.5, not 4
    assert cfo.n_reveal(10, 3) == 4 and list(np.flatnonzero(cfo.commit_by_rank(masked, conf, 3))) == [1, 2, 6, 7]
    # unmasked positions neither count nor compete, whatever their (unread) confidence holds
    masked[[7, 6]] = False
    assert list(np.flatnonzero(cfo.commit_by_rank(masked, conf, 4))) == [1, 2] and cfo.n_reveal(8, 4) == 2
    # all NaN: the lowest positions
    allnan = np.full(6, nan, dtype=np.float32)
    assert list(np.flatnonzero(cfo.commit_by_sort(np.ones(6, dtype=bool), allnan, 2))) == [0, 1, 2]
    assert list(np.flatnonzero(cfo.commit_by_rank(np.ones(6, dtype=bool), allnan, 2))) == [0, 1, 2]
    # t = 1 reveals the NaN positions too
    assert cfo.commit_by_rank(np.ones(10, dtype=bool), conf, 1).all()


def test_bound_arithmetic():
    u = 2.0 ** -24
    assert cfo.U == u and [cfo.classes_per_lane(K) for K in (2, 256, 257, 512, 513, 1024, 1025, 2048)] == [4, 4, 8, 8, 16, 16, 32, 32]
    for K in cfo.KS:
        nj, lnk = cfo.classes_per_lane(K), math.log(K)
        # first order: (ln K + 4 + nj + 6) u into the logarithm, 4 ln K u from logf, (|mx| + ln K) u and |conf| u from the add and the subtract
        first = ((lnk + 4 + nj + 6) + 4 * lnk + (3.0 + lnk) + 5.0) * u
        got = float(cfo.conf_bound(K, np.array([-3.0]), np.array([-5.0]))[0])
        assert first < got < first * 1.01, (K, first, got)
        # grows with |mx| and |conf| by u each, and nowhere else
        d = float(cfo.conf_bound(K, np.array([103.0]), np.array([-5.0]))[0]) - got
        assert abs(d - 100 * u * (1 + 2.0 ** -10)) < 1e-12
    # the largest case of the table stays a few hundred ulps of 1: the test can tell a wrong class from a rounding
    assert float(cfo.conf_bound(2048, np.array([40.0]), np.array([-30.0]))[0]) < 1e-5
    # the fp64 reference itself: log-softmax of a two-class row
    zt = torch.tensor([[0.0, math.log(3.0)], [1.0, float("-inf")]], dtype=torch.float32)
    lp = cfo.log_prob_f64(zt, torch.tensor([0, 0]))
    assert abs(float(lp[0]) - math.log(0.25)) < 1e-7 and float(lp[1]) == 0.0
    assert math.isnan(float(cfo.log_prob_f64(torch.full((1, 4), float("-inf")), torch.tensor([0]))[0]))


@pytest.mark.parametrize("K", cfo.KS)
def test_top_p_rows_of_the_table_are_rarely_fragile(K):
    """What tests/test_gpu_confident.py relies on: at most FRAGILE_SHARE_CAP (tests/_topp_oracle.py) of a case's nucleus-truncated
    rows have a cut the host cannot decide (those rows are left out of the confidence comparison, nothing else)."""
    for HW in cfo.HWS:
        logits, q, x0, un0, temps, ks, ps = cfo.conf_inputs(K, HW)
        _, _, fcut, on = cfo.reference_rows(logits, temps, ks, ps)
        assert int(on.sum()) == 3 * HW                           # images 2, 3 and 4 are nucleus-truncated
        assert float(fcut.sum()) <= tpo.FRAGILE_SHARE_CAP * float(on.sum()), (K, HW, int(fcut.sum()), int(on.sum()))
