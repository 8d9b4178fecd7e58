"""Which launches each form of ``AbsorbingDiffusion.sample()`` makes, eager and captured (CPU, no kernel runs).

Every launch form of the sampler gives the same tokens, so a step loop that sends a call to the wrong form, drops
``next_input`` or builds the denoiser input every step fails no parity test -- it only gets slower.  As in
tests/test_fused_dispatch.py the ``spkdiff.ops`` wrappers are replaced by recorders (tests/_dispatch_recorders.py, here with
the sampler's own launches and noise arguments logged too); the eager entry (``_sample_eager``) and the body a graph captures
(``_graph_body``) are driven with CPU tensors, B = 2, two steps.  Weight-pack and ``bn_prepare`` calls are left out of the
comparison.  The lists below were recorded from the loops as they stood before they became one (eager: ``sample()`` with its
device check bypassed; captured: the ``body()`` closure called directly); the one difference is that the eager conditional
call now hands spk_completion_state the buffers to fill (``completion_state(out)``, the same single launch).
"""
import itertools

import pytest
import torch

from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel, SampleForm, _SamplerGraph, functional

from _dispatch_recorders import B, _install_recorders

STEPS = 2
# name -> sampler switches (ab), denoiser switches (dn), latent side (hw), and what the call is given
CASES = {
    'eager_dense_tail_philox': dict(ab=dict(skip_untouched=False)),
    'eager_dense_tail_host': dict(ab=dict(skip_untouched=False, noise_source='host')),
    'eager_record_host': dict(ab=dict(noise_source='host'), record=True),
    'eager_dense': dict(ab=dict(skip_untouched=False), dn=dict(use_step_tail=False)),
    'eager_dense_injected': dict(ab=dict(skip_untouched=False), dn=dict(use_step_tail=False), inject=True),
    'eager_elim': dict(ab=dict(list_positions=False)),
    'eager_elim_host': dict(ab=dict(list_positions=False, noise_source='host')),
    'eager_elim_lists': dict(),
    'eager_elim_lists_tail': dict(ab=dict(step_tail_in_elimination=True)),
    'eager_elim_lists_known': dict(known=True),
    'eager_dense_tail_known': dict(ab=dict(skip_untouched=False), known=True),
    'eager_8x8_lists_asked': dict(hw=8),
    'graph_dense_tail': dict(ab=dict(skip_untouched=False)),
    'graph_dense': dict(ab=dict(skip_untouched=False), dn=dict(use_step_tail=False)),
    'graph_elim': dict(ab=dict(list_positions=False)),
    'graph_elim_lists': dict(),
    'graph_elim_lists_tail': dict(ab=dict(step_tail_in_elimination=True)),
    'graph_elim_lists_known': dict(known=True),
    'graph_dense_known': dict(ab=dict(skip_untouched=False), dn=dict(use_step_tail=False), known=True),
    'graph_8x8_lists_asked': dict(hw=8),
}


CONV1 = 'conv_fused(mode=LIF, in_kind=TINV, chunk_out=S32, want_counts, want_ptc)'
TRUNK = ['den_conv3x3_mfma_fp6v2(need_radius=4)', 'den_conv3x3_mfma_fp6v2(need_radius=3)',
         'den_conv3x3_mfma_fp6v2(need_radius=2)', 'den_conv3x3_mfma_fp6v2(want_counts, need_radius=1)']
# name -> (what form_for says, the launches of the first step ... the last step)
EXPECTED = {
    'eager_dense_tail_philox': ('dense_step_tail',
        ['den_build_input', CONV1] + TRUNK + ['den_step_tail(conv1)'] + TRUNK + ['den_step_tail'],
    ),
    'eager_dense_tail_host': ('dense_step_tail',
        ['den_build_input', CONV1] + TRUNK + ['den_step_tail(conv1, u, q)'] + TRUNK +
        ['den_step_tail(u, q)'],
    ),
    'eager_record_host': ('elimination_lists',
        ['den_build_input', CONV1] + TRUNK + ['den_step_tail(conv1, want_logits, u, q)'] + TRUNK +
        ['den_step_tail(want_logits, u, q)'],
    ),
    'eager_dense': ('dense',
        ['den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step'],
    ),
    'eager_dense_injected': ('dense',
        ['den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step(u, q)', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step(u, q)'],
    ),
    'eager_elim': ('elimination',
        ['select_active', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step', 'select_active(out)', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step'],
    ),
    'eager_elim_host': ('elimination',
        ['select_active(u)', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step(u, q)', 'select_active(u, out)', 'den_build_input', CONV1] +
        TRUNK + ['den_conv3x3_counts', 'psample_step(u, q)'],
    ),
    'eager_elim_lists': ('elimination_lists',
        ['select_active', 'select_needed', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step', 'select_active(out)', 'select_needed', 'den_build_input', CONV1] +
        TRUNK + ['den_conv3x3_counts', 'psample_step'],
    ),
    'eager_elim_lists_tail': ('elimination_lists',
        ['select_active', 'select_needed', 'den_build_input', CONV1] + TRUNK +
        ['den_step_tail', 'select_active(out)', 'select_needed', 'den_build_input', CONV1] + TRUNK +
        ['den_step_tail'],
    ),
    'eager_elim_lists_known': ('elimination_lists',
        ['completion_state(out)', 'select_active', 'select_needed', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step', 'select_active(out)', 'select_needed', 'den_build_input', CONV1] +
        TRUNK + ['den_conv3x3_counts', 'psample_step'],
    ),
    'eager_dense_tail_known': ('dense_step_tail',
        ['completion_state(out)', 'den_build_input', CONV1] + TRUNK + ['den_step_tail(conv1)'] + TRUNK +
        ['den_step_tail'],
    ),
    'eager_8x8_lists_asked': ('elimination',
        ['select_active', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step', 'select_active(out)', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step'],
    ),
    'graph_dense_tail': ('dense_step_tail',
        ['den_build_input', CONV1] + TRUNK + ['den_step_tail(conv1, philox_state)'] + TRUNK +
        ['den_step_tail(philox_state)'],
    ),
    'graph_dense': ('dense',
        ['den_build_input(out)', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step(philox_state, next_input)', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step(philox_state)'],
    ),
    'graph_elim': ('elimination',
        ['select_active(philox_state, out)', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step(philox_state)', 'select_active(philox_state, out)', 'den_build_input', CONV1] +
        TRUNK + ['den_conv3x3_counts', 'psample_step(philox_state)'],
    ),
    'graph_elim_lists': ('elimination_lists',
        ['select_active(philox_state, out)', 'select_needed(philox_state)', 'den_build_input', CONV1] +
        TRUNK +
        ['den_conv3x3_counts', 'psample_step(philox_state)', 'select_active(philox_state, out)', 'select_needed(philox_state)', 'den_build_input', CONV1] +
        TRUNK + ['den_conv3x3_counts', 'psample_step(philox_state)'],
    ),
    'graph_elim_lists_tail': ('elimination_lists',
        ['select_active(philox_state, out)', 'select_needed(philox_state)', 'den_build_input', CONV1] +
        TRUNK +
        ['den_step_tail(philox_state)', 'select_active(philox_state, out)', 'select_needed(philox_state)', 'den_build_input', CONV1] +
        TRUNK + ['den_step_tail(philox_state)'],
    ),
    'graph_elim_lists_known': ('elimination_lists',
        ['completion_state(out)', 'select_active(philox_state, out)', 'select_needed(philox_state)', 'den_build_input', CONV1] +
        TRUNK +
        ['den_conv3x3_counts', 'psample_step(philox_state)', 'select_active(philox_state, out)', 'select_needed(philox_state)', 'den_build_input', CONV1] +
        TRUNK + ['den_conv3x3_counts', 'psample_step(philox_state)'],
    ),
    'graph_dense_known': ('dense',
        ['completion_state(out)', 'den_build_input(out)', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step(philox_state, next_input)', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step(philox_state)'],
    ),
    'graph_8x8_lists_asked': ('elimination',
        ['select_active(philox_state, out)', 'den_build_input', CONV1] + TRUNK +
        ['den_conv3x3_counts', 'psample_step(philox_state)', 'select_active(philox_state, out)', 'den_build_input', CONV1] +
        TRUNK + ['den_conv3x3_counts', 'psample_step(philox_state)'],
    ),
}


def _sampler(case, hw=7):
    torch.manual_seed(0)
    dn = DummyModel(1, 128).eval()
    functional.set_step_mode(dn, 'm')
    ab = AbsorbingDiffusion(dn, mask_id=128, latent_shape=(hw, hw))
    ab.n_samples, ab.list_min_batch, ab.verify_weights = B, 1, False
    for obj, values in ((dn, case.get('dn', {})), (ab, case.get('ab', {}))):
        for k, v in values.items():
            setattr(obj, k, v)
    return ab


@pytest.mark.parametrize('name', sorted(CASES))
def test_sampler_launches(monkeypatch, name):
    case = CASES[name]
    hw = case.get('hw', 7)
    ab = _sampler(case, hw)
    cpu = torch.device('cpu')
    start = (torch.zeros((B, hw, hw), dtype=torch.int64), torch.zeros((B, hw, hw), dtype=torch.uint8)) if case.get('known') else None
    record = [] if case.get('record') else None
    noise = (lambda t: (torch.zeros(B, 1, hw, hw), torch.zeros(B * hw * hw, 128))) if case.get('inject') else None
    log = _install_recorders(monkeypatch, sampler=True)
    form = ab._form(B, hw, hw, record is not None)
    with torch.no_grad():
        if name.startswith('graph'):
            ab._graph_body(_SamplerGraph(cpu, B, hw, hw, form, int(ab.list_radii), start is not None), form, 1.0, STEPS)
        else:
            seed = 5 if noise is None and ab.noise_source == 'philox' else 0
            ab._sample_eager(cpu, B, hw, hw, form, 1.0, STEPS, noise, seed, start, record)
    launches = [c for c in log if not c.startswith(('bn_prepare', 'pack_', 'den_pack_'))]
    assert (ab.form_for(B, hw, hw), launches) == EXPECTED[name]
    if record is not None:
        assert [r[0] for r in record] == [2, 1] and not form.skip


# ---- the form table -------------------------------------------------------------------------------------------------------
_SWITCHES = list(itertools.product((False, True), (False, True), (False, True), ((7, 7), (8, 8)), (16, 24)))


def _set(ab, skip, lists, tail):
    ab.skip_untouched, ab.list_positions, ab._denoise_fn.use_step_tail = skip, lists, tail


@pytest.mark.parametrize('skip,lists,tail,hw,b', _SWITCHES)
def test_form_for_agrees_with_the_form_record(skip, lists, tail, hw, b):
    ab = _sampler({}, hw[0])
    ab.list_min_batch = 24
    _set(ab, skip, lists, tail)
    form = ab._form(b, *hw)
    listed = skip and lists and hw == (7, 7) and b >= 24
    assert form == SampleForm(skip=skip, lists=listed, tail=tail and not skip, tail_act=False)
    name = ('elimination_lists' if listed else 'elimination') if skip else ('dense_step_tail' if tail else 'dense')
    assert ab.form_for(b, *hw) == name
    # record= wants every image's logits at every step: always the dense form
    rec = ab._form(b, *hw, True)
    assert rec == SampleForm(skip=False, lists=False, tail=tail, tail_act=False)
    ab.step_tail_in_elimination = True
    assert ab._form(b, *hw) == form._replace(tail_act=skip and tail) and ab._form(b, *hw, True) == rec


def test_graph_key_changes_with_every_input_of_the_key():
    """The key as it was spelled before the form record existed, against the key built from the record, over the switches
    and the call's arguments: two settings with different old keys must have different new keys -- the new key determines
    the old one."""
    ab = _sampler({})
    ab.list_min_batch = 24
    dn = ab._denoise_fn
    old_of = {}
    for (skip, lists, tail, hw, b), tail_elim, radii, layout, first, steps, temp, cond in itertools.product(
            _SWITCHES, (False, True), (2, 3), ('global', 'rank'), (0, 16), (5, 49), (1.0, 0.9), (False, True)):
        _set(ab, skip, lists, tail)
        ab.step_tail_in_elimination, ab.list_radii, ab.noise_layout, ab.global_first = tail_elim, radii, layout, first
        listed = skip and ab._list_ok(*hw, b)
        old = ('cpu', b, *hw, 128, temp, steps, 128, skip, listed, radii, tail, tail_elim, layout, first, cond)
        new = ab._graph_key('cpu', b, *hw, temp, steps, ab._form(b, *hw), cond)
        assert old_of.setdefault(new, old) == old, "two settings that differed in the old key share a key now"
    assert len(set(old_of.values())) == 2304          # (of 4096 settings: list_positions does not count where no lists are taken)
    # ... and with the weights: a new version of a parameter, an invalidation of the derived forms
    k0 = ab._graph_key('cpu', 16, 7, 7, 1.0, 5, ab._form(16, 7, 7), False)
    with torch.no_grad():
        next(dn.parameters()).add_(1.0)
    k1 = ab._graph_key('cpu', 16, 7, 7, 1.0, 5, ab._form(16, 7, 7), False)
    dn.invalidate()
    k2 = ab._graph_key('cpu', 16, 7, 7, 1.0, 5, ab._form(16, 7, 7), False)
    assert len({k0, k1, k2}) == 3
