"""CPU tests of per-image step counts for confidence-ordered decoding: the step counts ``positions_per_step``
chooses against the schedule of tests/_confident_oracle.py, the counter arithmetic of the listed kernel, the host mirror of the
pending list, and what the two new C entry points refuse before any launch.  No device."""
import pytest
import torch

import _confident_oracle as cfo
import _confident_steps_oracle as cso


def test_positions_per_step_bounds_every_commit():
    """For all m <= 64 and r <= 64: s = max(1, ceil(m / r)) steps, every step of the ceil(m / t) schedule commits <= r, the total is m."""
    for m0 in range(0, 65):
        for r in range(1, 65):
            s = cso.steps_for_hole(m0, r)
            assert s == max(1, -(-m0 // r)) and (s - 1) * r < max(m0, 1) <= s * r
            m, total = m0, 0
            for t in range(s, 0, -1):
                n = cfo.n_reveal(m, t)
                assert n <= r, (m0, r, t, n)
                m -= n
                total += n
            assert m == 0 and total == m0


def test_the_package_chooses_the_same_step_counts():
    from spkdiff.complete import steps_for_holes
    m = torch.arange(0, 65)
    for r in (1, 3, 4, 7, 49, 64):
        assert steps_for_holes(m, r).tolist() == [cso.steps_for_hole(int(v), r) for v in m]
    assert steps_for_holes(torch.tensor([0, 4, 12, 24, 49]), 4).tolist() == [1, 1, 3, 6, 13]


def test_offset_arithmetic_never_underflows_for_a_pending_image():
    """A pending image (t <= e_i) draws at base + (e_i - t) * stride: the step index of its own run, never below the shard's base --
    for every S, every count (also > S: e_i = S) and every t; a non-pending t > e_i would wrap, and is never drawn."""
    base = 5 * 49 * 128
    for S in (1, 2, 13, 49, 100):
        for sb in (1, 2, S - 1, S, S + 1, S + 5):
            if sb < 1:
                continue
            (e,) = cso.effective_steps([sb], S)
            assert e == min(sb, S)
            for t in range(S, 0, -1):
                off = cso.image_offset(cso.loop_offset(S, t, base), S, e)
                if t <= e:
                    assert off == base + (e - t) * cso.STEP_STRIDE == cso.loop_offset(e, t, base)      # the run of e steps alone
                else:
                    assert off > (1 << 63)                                                          # (wrapped: not pending)
    assert cso.effective_steps([-3, 0, 7, 20], 13) == [-3, 0, 7, 13]


def test_pending_list_mirror():
    un = torch.ones(6, 1, 7, 7, dtype=torch.bool)
    un[1, 0, 3, 3] = False
    un[2] = False
    un[3, 0, 0, :2] = False
    un[4] = False
    un[5, 0, 6, 6] = False
    steps = [5, 5, 2, 0, -3, 9]
    assert cso.pending(un, 5, steps) == [1, 5]                     # image 0: nothing masked; 2: t > s; 3, 4: counts < 1
    assert cso.pending(un, 2, steps) == [1, 2, 5]
    assert cso.pending(un, 9, steps) == [5] and cso.pending(un, 10, steps) == []
    for B, HW, t, S in ((5, 49, 2, 13), (65, 64, 13, 13), (300, 1, 1, 4)):
        un, sb = cso.select_case(B, HW, t, S, seed=B + HW)
        want = cso.pending(un, t, sb.tolist())
        assert want == sorted(want) and all(int(sb[b]) >= t and not bool(un[b].all()) for b in want)
        assert set(sb.tolist()) <= {-3, 0, t - 1, t, t + 1, S + 5}


def test_entry_points_refuse_bad_arguments_without_a_device():
    from spkdiff import _lib
    C = _lib.CONSTANTS
    assert _lib.version() == 106 and C["SPK_VERSION"] == 106
    assert "spk_select_pending" in _lib.EXPORTS and "spk_psample_step_conf_listed" in _lib.EXPORTS
    lib, P = _lib.lib, 0x1000                                        # (a non-null pointer: refused calls never touch it)
    ARG, UNS = C["SPK_ERR_ARG"], C["SPK_ERR_UNSUPPORTED"]
    good = [P, 2, P, P, P, 4, 49, None]                              # unmasked, t, steps_b, active_out, n_active_out, B, HW, stream
    for i in (0, 2, 3, 4):
        bad = list(good)
        bad[i] = None
        assert lib.spk_select_pending(*bad) == ARG, i
    for i, v in ((1, 0), (5, 0), (6, 0)):
        bad = list(good)
        bad[i] = v
        assert lib.spk_select_pending(*bad) == ARG, i
    assert lib.spk_select_pending(*(good[:6] + [65, None])) == UNS
    # logits, x_t, unmasked, t, temp_b, topk_b, topp_b, u, q, seed, offset, state, x0_hat, conf, B, HW, K, steps_b, S, stride, active,
    # n_active, stream
    good = [P, P, P, 2, P, P, P, None, None, 1, 0, None, None, None, 4, 49, 128, P, 5, 1 << 40, P, P, None]
    for i in (0, 1, 2, 4, 5, 6, 17, 20, 21):
        bad = list(good)
        bad[i] = None
        assert lib.spk_psample_step_conf_listed(*bad) == ARG, i
    for i, v in ((3, 0), (3, 6), (14, 0), (15, 0), (16, 0), (18, 0)):      # t < 1, t > S, B, HW, K, S
        bad = list(good)
        bad[i] = v
        assert lib.spk_psample_step_conf_listed(*bad) == ARG, (i, v)
    for i, v in ((15, 65), (16, 2049)):
        bad = list(good)
        bad[i] = v
        assert lib.spk_psample_step_conf_listed(*bad) == UNS, (i, v)


def test_sampler_reads_the_step_argument_before_anything_else():
    from snn_model.vq_diffusion import AbsorbingDiffusion as AD
    assert AD._steps_arg(None, 4) is None and AD._steps_arg(7, 4) == 7 and int(AD._steps_arg(torch.tensor(7), 4)) == 7
    v = AD._steps_arg([1, 3, 8, 2], 4)
    assert v.dtype == torch.int32 and v.tolist() == [1, 3, 8, 2]
    assert AD._steps_arg(torch.tensor([5]), 1).tolist() == [5]
    for bad in ([1, 2, 3], [1, 0, 2, 2], [1, -1, 2, 2], [1.0, 2.0, 3.0, 4.0], torch.ones(2, 2, dtype=torch.int64), [True] * 4,
                [1, 2, 3, 1 << 31]):
        with pytest.raises(ValueError):
            AD._steps_arg(bad, 4)
