"""Which launches ``AbsorbingDiffusion.score()`` makes in each form, eager and captured (CPU, no kernel runs; the recorders of
tests/test_sampler_dispatch.py plus one for ``ops.pscore_step``): the loop of sample() with spk_pscore_step in the place of
spk_psample_step, never a fused-tail launch, ``next_input`` in the captured dense form, the outputs zeroed inside the graph."""
import pytest
import torch

from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel, _SamplerGraph, functional

from _dispatch_recorders import B, _install_recorders
from test_sampler_dispatch import CONV1, TRUNK

STEPS = 2
BODY = ['den_conv3x3_counts']


def _sampler(hw=7, **switches):
    torch.manual_seed(0)
    dn = DummyModel(1, 128).eval()
    functional.set_step_mode(dn, 'm')
    ab = AbsorbingDiffusion(dn, mask_id=128, latent_shape=(hw, hw))
    ab.n_samples, ab.list_min_batch, ab.verify_weights = B, 1, False
    for k, v in switches.items():
        setattr(ab, k, v)
    return ab


def _record_pscore(monkeypatch, log):
    from spkdiff import ops

    def rec(logits, x0, x_t, unmasked, t, temp, logp, step=None, u=None, seed=0, offset=0, philox_state=None, next_input=None):
        assert x0.dtype == torch.int64 and logp.dtype == torch.float64 and step.dtype == torch.int32
        assert x0.numel() == x_t.numel() == logp.numel() == step.numel()
        given = [n for n, v in (('u', u), ('philox_state', philox_state), ('next_input', next_input)) if v is not None]
        log.append(f'pscore_step({", ".join(given)})' if given else 'pscore_step')
        return logp, step
    monkeypatch.setattr(ops, 'pscore_step', rec)


CASES = {
    # name: (sampler switches, known, captured, expected launches of the two steps)
    'eager_dense': (dict(skip_untouched=False), False, False,
                    ['den_build_input', CONV1] + TRUNK + BODY + ['pscore_step', 'den_build_input', CONV1] + TRUNK + BODY + ['pscore_step']),
    'eager_elim_lists_known': (dict(), True, False,
                               ['completion_state(out)', 'select_active', 'select_needed', 'den_build_input', CONV1] + TRUNK + BODY +
                               ['pscore_step', 'select_active(out)', 'select_needed', 'den_build_input', CONV1] + TRUNK + BODY + ['pscore_step']),
    'graph_dense': (dict(skip_untouched=False), False, True,
                    ['den_build_input(out)', CONV1] + TRUNK + BODY + ['pscore_step(philox_state, next_input)', CONV1] + TRUNK + BODY +
                    ['pscore_step(philox_state)']),
    'graph_elim': (dict(list_positions=False), False, True,
                   ['select_active(philox_state, out)', 'den_build_input', CONV1] + TRUNK + BODY +
                   ['pscore_step(philox_state)', 'select_active(philox_state, out)', 'den_build_input', CONV1] + TRUNK + BODY +
                   ['pscore_step(philox_state)']),
    'graph_elim_lists_known': (dict(), True, True,
                               ['completion_state(out)', 'select_active(philox_state, out)', 'select_needed(philox_state)', 'den_build_input', CONV1] +
                               TRUNK + BODY +
                               ['pscore_step(philox_state)', 'select_active(philox_state, out)', 'select_needed(philox_state)', 'den_build_input', CONV1] +
                               TRUNK + BODY + ['pscore_step(philox_state)']),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_score_launches(monkeypatch, name):
    switches, known, captured, want = CASES[name]
    ab = _sampler(**switches)
    cpu = torch.device('cpu')
    log = _install_recorders(monkeypatch, sampler=True)
    _record_pscore(monkeypatch, log)
    # the form score() takes: the step-tail switches of the denoiser are on (their default) and must not matter
    assert ab._denoise_fn.use_step_tail
    form = ab._form(B, 7, 7)._replace(tail=False, tail_act=False)
    x0 = torch.zeros((B, 7, 7), dtype=torch.int64)
    start = (x0, torch.zeros((B, 7, 7), dtype=torch.uint8)) if known else None
    with torch.no_grad():
        if captured:
            g = _SamplerGraph(cpu, B, 7, 7, form, int(ab.list_radii), known, True)
            assert (g.target[0] is g.start_in[0]) if known else (g.start_in is None)
            g.target[1].fill_(7.0)
            g.target[2].fill_(7)
            ab._graph_body(g, form, 1.0, STEPS)
            assert not g.target[1].any() and not g.target[2].any(), "the outputs are zeroed inside the graph"
        else:
            tgt = (x0, torch.zeros((B, 7, 7), dtype=torch.float64), torch.zeros((B, 7, 7), dtype=torch.int32))
            ab._sample_eager(cpu, B, 7, 7, form, 1.0, STEPS, None, 5, start, None, tgt)
    launches = [c for c in log if not c.startswith(('bn_prepare', 'pack_', 'den_pack_'))]
    assert launches == want


def test_score_graph_has_a_key_of_its_own_and_leaves_the_sample_keys_alone():
    ab = _sampler()
    form = ab._form(16, 7, 7)
    plain = ab._graph_key('cpu', 16, 7, 7, 1.0, 5, form, False)
    assert plain == ab._graph_key('cpu', 16, 7, 7, 1.0, 5, form, False, False)
    keys = {plain, ab._graph_key('cpu', 16, 7, 7, 1.0, 5, form, True),
            ab._graph_key('cpu', 16, 7, 7, 1.0, 5, form, False, True), ab._graph_key('cpu', 16, 7, 7, 1.0, 5, form, True, True)}
    assert len(keys) == 4
