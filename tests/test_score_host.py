"""CPU tests of the likelihood-bound feature (no device): the host oracle of the teacher-forced reverse process
(tests/_score_oracle.py) against an exhaustive enumeration on a latent small enough to enumerate -- which is also the check of
the documented claim that one pass is a lower bound in expectation on the log of a NORMALISED probability --, the argument
checks of spk_pscore_step and of ``AbsorbingDiffusion.score``, and the unchanged C-ABI version."""
import itertools

import numpy as np
import pytest
import torch

import _score_oracle as sorc


def _toy_logits(x_t, t):
    """A hand-written 'denoiser' on a 1x2 latent with K = 3: the logits of a position depend on the OTHER position's token
    (3 = still masked) and on the step."""
    x = x_t.numpy().reshape(-1, 2).astype(np.float64)
    k = np.arange(3, dtype=np.float64)[None, :, None]
    j = np.arange(2, dtype=np.float64)[None, None, :]
    other = x[:, ::-1][:, None, :]
    return np.sin(1.3 * k + 0.7 * other + 0.31 * t + j + 0.2 * k * other).astype(np.float32).reshape(-1, 3, 1, 2)


def test_every_schedule_enumerated_bound_and_normalisation():
    S, K = 2, 3
    maps = torch.tensor(list(itertools.product(range(K), repeat=2))).reshape(9, 1, 1, 2)          # all 9 token maps, one image each
    # position i is revealed at step 2 when u_i < 1/2 (probability 1/2), else at step 1 (u < 1 always): four schedules of 1/4
    scores, p_rho = [], []
    for rho in itertools.product((2, 1), repeat=2):
        u2 = torch.tensor([0.25 if r == 2 else 0.75 for r in rho]).reshape(1, 1, 1, 2).expand(9, 1, 1, 2)
        noise = {2: u2, 1: torch.full((9, 1, 1, 2), 0.75)}
        logp, step, x_t, unmasked = sorc.run_fn(_toy_logits, maps, None, S, lambda t: noise[t], K)
        assert np.array_equal(step.reshape(9, 2), np.broadcast_to(np.array(rho, dtype=np.int32), (9, 2)))
        assert torch.equal(x_t, maps) and bool(unmasked.all())
        scores.append(logp.reshape(9, 2).sum(1))
        p_rho.append(0.25)
    scores, p_rho = np.stack(scores), np.array(p_rho)[:, None]                                     # [4 schedules, 9 maps]
    assert np.ptp(scores, axis=0).min() > 1e-3, "the schedules must disagree, or Jensen's inequality checks nothing"
    bound = (p_rho * scores).sum(0)                              # E_rho[score]: what score() estimates
    marginal = (p_rho * np.exp(scores)).sum(0)                   # p(x_0) of the sampler: schedule marginalised
    assert np.all(bound <= np.log(marginal)) and np.all(bound < np.log(marginal) - 1e-6)
    assert abs(marginal.sum() - 1.0) <= 1e-12                    # a probability over the 9 maps
    # every single schedule is a normalised autoregressive model too
    assert np.allclose(np.exp(scores).sum(1), 1.0, rtol=0, atol=1e-12)


def test_oracle_known_positions_and_special_values():
    K = 3
    x0 = torch.tensor([[[[2, 1]]], [[[5, 0]]]])                  # image 1: a target outside the codebook
    known = torch.tensor([[[[True, False]]], [[[False, False]]]])
    u = torch.full((2, 1, 1, 2), 0.75)
    logp, step, x_t, unmasked = sorc.run_fn(_toy_logits, x0, known, 2, lambda t: u, K)
    assert logp[0, 0, 0] == 0 and step[0, 0, 0] == 0 and step[0, 0, 1] == 1 and logp[0, 0, 1] < 0
    assert logp[1, 0, 0] == -np.inf and np.isfinite(logp[1, 0, 1]) and int(x_t[1, 0, 0, 0]) == 5
    inf = np.float32(np.inf)
    assert np.isnan(sorc.log_prob(np.array([0.0, np.nan, 1.0], dtype=np.float32), 0))
    assert sorc.log_prob(np.array([0.0, -inf, 1.0], dtype=np.float32), 1) == -np.inf
    assert np.isnan(sorc.log_prob(np.array([-inf, -inf, -inf], dtype=np.float32), 2))
    assert sorc.log_prob(np.array([0.0, 1.0], dtype=np.float32), -1) == -np.inf
    assert abs(sorc.log_prob(np.array([0.0, 0.0], dtype=np.float32), 1) + np.log(2.0)) < 1e-15


def test_pscore_step_rejects_bad_arguments_on_the_host():
    from spkdiff import _lib
    f = _lib.lib.spk_pscore_step
    # (fake non-null addresses: every call below is refused before any launch)
    lg, x0, xt, um, lp, st, act, nact = (0x1000 * (i + 1) for i in range(8))
    ok = dict(logits=lg, x0=x0, x_t=xt, unmasked=um, t=3, temp=1.0, u=None, seed=1, offset=0, state=None, logp=lp, step=st, B=2,
              HW=49, K=128, active=None, n_active=None, next_input=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*a.values())
    for name in ('logits', 'x0', 'x_t', 'unmasked', 'logp'):
        assert call(**{name: None}) == -1, name
    for kw in (dict(t=0), dict(t=-2), dict(temp=0.0), dict(temp=-1.0), dict(temp=float('nan')), dict(K=0), dict(K=-3), dict(B=0),
               dict(HW=0), dict(active=act), dict(n_active=nact), dict(active=act, n_active=nact, next_input=0x9000)):
        assert call(**kw) == -1, kw
    assert call(K=513) == -2 and call(K=4096) == -2
    with pytest.raises(ValueError, match='spk_pscore_step'):
        _lib.check(call(t=0), 'spk_pscore_step')


def test_score_refuses_cpu_tensors_and_bad_arguments():
    from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel, Score, functional
    dn = DummyModel(1, 128).eval()
    functional.set_step_mode(dn, 'm')
    ab = AbsorbingDiffusion(dn, mask_id=128)
    ab.n_samples = 5
    state = torch.random.get_rng_state()
    with pytest.raises(RuntimeError, match='no CPU path'):
        ab.score(torch.zeros(2, 1, 7, 7, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ab.score(torch.zeros(2, 7, 7, dtype=torch.int32), known=torch.zeros(2, 7, 7, dtype=torch.bool))
    with pytest.raises(ValueError):
        ab.score(torch.zeros(2, 1, 8, 8, dtype=torch.int64))
    with pytest.raises(ValueError):
        ab.score(torch.zeros(2, 1, 7, 7, dtype=torch.int64), known=torch.zeros(2, 7, 7, dtype=torch.bool))
    with pytest.raises(ValueError):
        ab.score(None)
    with pytest.raises(NotImplementedError):
        ab.score(torch.zeros(2, 1, 7, 7))
    with pytest.raises(NotImplementedError):
        ab.score(torch.zeros(2, 1, 7, 7, dtype=torch.int64), known=torch.zeros(2, 1, 7, 7))
    with pytest.raises(TypeError):
        ab.score([[0] * 7] * 7)
    assert torch.equal(torch.random.get_rng_state(), state) and ab.last_key is None and ab.n_samples == 5, "nothing drawn"
    assert Score._fields == ('position_log_prob', 'reveal_step', 'log_prob')
    s = Score(torch.zeros(2, 3, 7, 7, dtype=torch.float64), torch.zeros(2, 3, 7, 7, dtype=torch.int32),
              torch.tensor([[-49.0, -98.0, -49.0], [-98.0, -49.0, -98.0]], dtype=torch.float64))
    assert abs(float(s.bits_per_dim(49)) - 1.5 / np.log(2.0)) < 1e-15 and float(s.bits_per_dim()) == float(s.bits_per_dim(49))


def test_the_entry_point_is_additive():
    from spkdiff import _lib
    assert _lib.version() == 106 and 'spk_pscore_step' in _lib.EXPORTS
