"""Which launches each configuration makes (CPU, no kernel runs).

Every kernel form of ``FusedSequential.run`` and the denoiser is bit-exact, so sending a layer to the wrong form changes no
number a parity test could see -- only the speed.  Here the ``spkdiff.ops`` wrappers that pack weights or launch kernels are
replaced by recorders that log the call with the arguments that pick its form and return zero tensors of the shape and dtype
the real wrapper returns (the next block dispatches on those); the pure-Python predicates stay real.  Each configuration's
call list, the pack calls included, is pinned as a literal below.
"""
import re

import pytest
import torch

from spkdiff import ops
from spkdiff.fused import FusedSequential
from spkdiff.ops import IN_PTC, IN_SEQ, IN_TINV
from snn_model.vae_model import SNN_VQVAE
from snn_model.vq_diffusion import DummyModel, functional

from _dispatch_recorders import B, _f32, _install_recorders, _s4, _u8


@pytest.fixture
def calls(monkeypatch):
    """Replace the packing / launching wrappers of spkdiff.ops by recorders; returns the call log."""
    return _install_recorders(monkeypatch)


def _ready(m):
    m.eval()
    functional.set_step_mode(m, 'm')
    return m


def _vqvae(in_dim=1, embedding_dim=16):
    torch.manual_seed(0)
    return _ready(SNN_VQVAE(in_dim, embedding_dim, 128, torch.tensor(1.0)))


def _den():
    torch.manual_seed(0)
    return _ready(DummyModel(1, 128))


def _img(m, hw):
    c = m.encoder.snn_convs[0].in_channels
    return _f32(B, c, hw, hw)


def _tokens(h):
    return torch.zeros((B, 1, h, h))


# ---- the configurations -----------------------------------------------------------------------------------------------
def enc_tinv_28():
    m = _vqvae(1)
    m.encoder.snn_convs.run(_img(m, 28), IN_TINV, final='ptc', T=16, stateful=False)


def enc_tinv_32():
    m = _vqvae(3)
    m.encoder.snn_convs.run(_img(m, 32), IN_TINV, final='ptc', T=16, stateful=False)


def enc_seq_stateful():
    m = _vqvae(1)
    m.encoder.snn_convs.run(_f32(16, B, 1, 28, 28), IN_SEQ, final='ptc')


def enc_seq_f32():
    m = _vqvae(1)
    m.encoder.snn_convs.run(_f32(16, B, 1, 28, 28), IN_SEQ, final='f32')


def enc_direct():
    m = _vqvae(1)
    m.encoder.snn_convs.run(_img(m, 28), IN_TINV, final='ptc', T=16, stateful=False, impl='direct')


def poisson_tinv():
    m = _vqvae(1)
    m.vq_layer.poisson.run(_f32(B, 16, 7, 7), IN_TINV, final='ptc', T=16, stateful=False)


def tokens_to_s32_none():
    m = _vqvae(1)
    cb = m.vq_layer.embeddings.weight
    assert m.vq_layer.poisson.tokens_to_s32(torch.zeros((B, 7, 7), dtype=torch.int64), cb) is None     # CPU tokens
    assert m.encoder.snn_convs.tokens_to_s32(torch.zeros((B, 7, 7), dtype=torch.int64), cb) is None    # not a generator


def decode_tokens_7():
    m = _vqvae(1)
    m.decode_tokens(torch.zeros((B, 7, 7), dtype=torch.int64))


def _memout(m, x, **kw):
    return m.decoder.snn_convs.run(x, IN_PTC, final='memout', coef=m.memout.coef.flatten(), apply_tanh=True, want_u8=True,
                                   **kw)


def dec_s32_7():
    m = _vqvae(1)
    _memout(m, _s4(B, 1, 7, 7, 16, 16), stateful=False)


def dec_s32_8():
    m = _vqvae(3)
    _memout(m, _s4(B, 1, 8, 8, 16, 16), stateful=False)


def dec_ptc_7():
    m = _vqvae(1)
    _memout(m, _u8(B, 7, 7, 16, 16), stateful=False)


def dec_ptc_8():
    m = _vqvae(3)
    _memout(m, _u8(B, 8, 8, 16, 16), stateful=False)


def dec_ptc_d32():
    m = _vqvae(1, embedding_dim=32)
    _memout(m, _u8(B, 7, 7, 16, 32), stateful=False)


def dec_memout_stateful():
    m = _vqvae(1)
    _memout(m, _u8(B, 7, 7, 16, 16))


def dec_f32_ptc():
    m = _vqvae(1)
    m.decoder.snn_convs.run(_u8(B, 7, 7, 16, 16), IN_PTC, final='f32', stateful=False)


def dec_f32_seq():
    m = _vqvae(1)
    m.decoder.snn_convs.run(_f32(16, B, 16, 7, 7), IN_SEQ, final='f32')


def dec_direct():
    m = _vqvae(1)
    _memout(m, _u8(B, 7, 7, 16, 16), stateful=False, impl='direct')


def den_logits_7():
    _den().logits_from_tokens(_tokens(7), 5)


def den_logits_8():
    _den().logits_from_tokens(_tokens(8), 5)


def den_forward_stateful():
    _den()(_tokens(7), torch.full((B,), 5))


def den_i8():
    m = _den()
    m.conv_impl_request = 'i8'
    m.logits_from_tokens(_tokens(7), 5)


def den_direct():
    m = _den()
    m.conv_impl_request = 'direct'
    m.logits_from_tokens(_tokens(7), 5)


def den_no_collapse():
    m = _den()
    m.collapse_conv6 = False
    m.logits_from_tokens(_tokens(7), 5)


def den_no_fp6v2():
    m = _den()
    m.use_fp6v2 = False
    m.logits_from_tokens(_tokens(7), 5)


def den_sample_step():
    m = _den()
    x_t, unmasked = torch.zeros((B, 1, 7, 7), dtype=torch.int64), torch.zeros((B, 1, 7, 7), dtype=torch.bool)
    pre1, _ = m.sample_step(x_t, unmasked, 5, 1.0)
    m.sample_step(x_t, unmasked, 4, 1.0, pre1=pre1, want_next=False, want_logits=True)


def den_conv6_mean():
    m = _den()
    m.conv6.run(_u8(B, 8, 7, 7, 16, 32), IN_PTC, final='mean', in1=_u8(B, 2, 7, 7, 16, 32))


def want_pre_tinv():
    m = _vqvae(1)
    blk = FusedSequential(*list(m.encoder.snn_convs)[0:3])
    blk.run(_img(m, 28), IN_TINV, final='both', T=16, stateful=False, want_pre=True)


def want_pre_ptc():
    m = _vqvae(1)
    blk = FusedSequential(*list(m.encoder.snn_convs)[3:6])
    blk.run(_u8(B, 14, 14, 16, 32), IN_PTC, final='both', stateful=False, want_pre=True)


EXPECTED = {
    'dec_direct': [
        'pack_conv_weight(transposed)',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=PTC, transposed, want_ptc)',
        'pack_conv_weight(transposed)',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=PTC, transposed, want_ptc)',
        'pack_conv_weight(transposed)',
        'conv_fused(mode=MEMOUT, in_kind=PTC, transposed)',
    ],
    'dec_f32_ptc': [
        'pack_conv_weight_i8(transposed)',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF, transposed)',
        'pack_conv_weight_i8(transposed)',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF, transposed)',
        'pack_conv_weight(transposed)',
        'conv_fused(mode=RAW, in_kind=PTC, transposed)',
    ],
    'dec_f32_seq': [
        'pack_conv_weight(transposed)',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=SEQ, transposed, v, want_ptc)',
        'pack_conv_weight_i8(transposed)',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF, transposed, v)',
        'pack_conv_weight(transposed)',
        'conv_fused(mode=RAW, in_kind=PTC, transposed)',
    ],
    'dec_memout_stateful': [
        'pack_conv_weight_i8(transposed)',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF, transposed, v)',
        'pack_conv_weight_i8(transposed)',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF, transposed, collapse_coef, v)',
        'readout_collapsed(transposed)',
    ],
    'dec_ptc_7': [
        'pack_conv_weight_i8(transposed)',
        'bn_prepare',
        'ptc_to_s32',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=S32, transposed)',
        'bn_prepare',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=COLLAPSED, transposed)',
        'readout_collapsed(transposed)',
    ],
    'dec_ptc_8': [
        'pack_conv_weight_i8(transposed)',
        'bn_prepare',
        'ptc_to_s32',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=S32, transposed)',
        'bn_prepare',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=COLLAPSED, transposed)',
        'readout_collapsed(transposed)',
    ],
    'dec_ptc_d32': [
        'pack_conv_weight_i8(transposed)',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF, transposed, out_s32)',
        'bn_prepare',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=COLLAPSED, transposed)',
        'readout_collapsed(transposed)',
    ],
    'dec_s32_7': [
        'bn_prepare',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=S32, transposed)',
        'bn_prepare',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=COLLAPSED, transposed)',
        'readout_collapsed(transposed)',
    ],
    'dec_s32_8': [
        'bn_prepare',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=S32, transposed)',
        'bn_prepare',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=COLLAPSED, transposed)',
        'readout_collapsed(transposed)',
    ],
    'decode_tokens_7': [
        'embedding',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, want_ptc)',
        'pack_conv_weight_i8(transposed)',
        'bn_prepare',
        'ptc_to_s32',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=S32, transposed)',
        'bn_prepare',
        'vae_fp6_pack(transposed)',
        'vae_fp6_fwd(out_kind=COLLAPSED, transposed)',
        'readout_collapsed(transposed)',
    ],
    'den_conv6_mean': [
        'den_pack_weight_i8',
        'den_conv3x3_mfma(mode=MEAN)',
    ],
    'den_direct': [
        'den_build_input',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, chunk_out=32, want_ptc)',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=PTC, chunk_out=32, want_ptc)',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=PTC, chunk_out=32, want_ptc)',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=PTC, chunk_out=32, want_ptc)',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=PTC, chunk_out=32, want_ptc)',
        'pack_conv_weight',
        'conv_fused(mode=MEAN, in_kind=PTC)',
    ],
    'den_forward_stateful': [
        'den_build_input',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, chunk_out=C4, want_counts, v, want_ptc)',
        'bn_prepare',
        'den_pack_weight_fp6',
        'den_conv3x3_mfma_fp6(v)',
        'bn_prepare',
        'den_pack_weight_fp6',
        'den_conv3x3_mfma_fp6(v)',
        'bn_prepare',
        'den_pack_weight_fp6',
        'den_conv3x3_mfma_fp6(v)',
        'bn_prepare',
        'den_pack_weight_fp6',
        'den_conv3x3_mfma_fp6(want_counts, v)',
        'den_pack_weight_i8(pad_cout)',
        'den_conv3x3_counts',
    ],
    'den_i8': [
        'den_build_input',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, chunk_out=32, want_counts, want_ptc)',
        'den_pack_weight_i8',
        'bn_prepare',
        'den_conv3x3_mfma(mode=LIF)',
        'den_pack_weight_i8',
        'bn_prepare',
        'den_conv3x3_mfma(mode=LIF)',
        'den_pack_weight_i8',
        'bn_prepare',
        'den_conv3x3_mfma(mode=LIF)',
        'den_pack_weight_i8',
        'bn_prepare',
        'den_conv3x3_mfma(mode=LIF, want_counts)',
        'den_pack_weight_i8(pad_cout)',
        'den_conv3x3_counts',
    ],
    'den_logits_7': [
        'den_build_input',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, chunk_out=S32, want_counts, want_ptc)',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2(want_counts)',
        'den_pack_weight_i8(pad_cout)',
        'den_conv3x3_counts',
    ],
    'den_logits_8': [
        'den_build_input',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, chunk_out=S32, want_counts, want_ptc)',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2(want_counts)',
        'den_pack_weight_i8(pad_cout)',
        'den_conv3x3_counts',
    ],
    'den_no_collapse': [
        'den_build_input',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, chunk_out=32, want_ptc)',
        'den_pack_weight_i8',
        'bn_prepare',
        'den_conv3x3_mfma(mode=LIF)',
        'den_pack_weight_i8',
        'bn_prepare',
        'den_conv3x3_mfma(mode=LIF)',
        'den_pack_weight_i8',
        'bn_prepare',
        'den_conv3x3_mfma(mode=LIF)',
        'den_pack_weight_i8',
        'bn_prepare',
        'den_conv3x3_mfma(mode=LIF)',
        'den_pack_weight_i8',
        'den_conv3x3_mfma(mode=MEAN)',
    ],
    'den_no_fp6v2': [
        'den_build_input',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, chunk_out=C4, want_counts, want_ptc)',
        'bn_prepare',
        'den_pack_weight_fp6',
        'den_conv3x3_mfma_fp6',
        'bn_prepare',
        'den_pack_weight_fp6',
        'den_conv3x3_mfma_fp6',
        'bn_prepare',
        'den_pack_weight_fp6',
        'den_conv3x3_mfma_fp6',
        'bn_prepare',
        'den_pack_weight_fp6',
        'den_conv3x3_mfma_fp6(want_counts)',
        'den_pack_weight_i8(pad_cout)',
        'den_conv3x3_counts',
    ],
    'den_sample_step': [
        'den_build_input',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, chunk_out=S32, want_counts, want_ptc)',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'bn_prepare',
        'den_pack_weight_fp6v2',
        'den_conv3x3_mfma_fp6v2(want_counts)',
        'den_pack_weight_i8(pad_cout)',
        'den_step_tail',
        'den_conv3x3_mfma_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'den_conv3x3_mfma_fp6v2',
        'den_conv3x3_mfma_fp6v2(want_counts)',
        'den_step_tail',
    ],
    'enc_direct': [
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, want_ptc)',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=PTC, want_ptc)',
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=PTC, want_ptc)',
    ],
    'enc_seq_f32': [
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=SEQ, v, want_ptc)',
        'pack_conv_weight_i8',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF, v)',
        'pack_conv_weight_i8',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF, v)',
        'ptc_to_spikes',
    ],
    'enc_seq_stateful': [
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=SEQ, v, want_ptc)',
        'pack_conv_weight_i8',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF, v)',
        'pack_conv_weight_i8',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF, v)',
    ],
    'enc_tinv_28': [
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, chunk_out=S32, want_ptc)',
        'bn_prepare',
        'vae_fp6_pack',
        'vae_fp6_fwd(out_kind=PTC)',
        'pack_conv_weight_i8',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF)',
    ],
    'enc_tinv_32': [
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, chunk_out=S32, want_ptc)',
        'bn_prepare',
        'vae_fp6_pack',
        'vae_fp6_fwd(out_kind=PTC)',
        'pack_conv_weight_i8',
        'bn_prepare',
        'conv_mfma_fused(mode=LIF)',
    ],
    'poisson_tinv': [
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, want_ptc)',
    ],
    'tokens_to_s32_none': [],
    'want_pre_ptc': [
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=PTC, want_ptc, want_f32, want_pre)',
    ],
    'want_pre_tinv': [
        'pack_conv_weight',
        'bn_prepare',
        'conv_fused(mode=LIF, in_kind=TINV, want_ptc, want_f32, want_pre)',
    ],
}


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_dispatch(calls, name):
    with torch.no_grad():
        globals()[name]()
    assert calls == EXPECTED[name]


# ---- error paths: type and message stay ---------------------------------------------------------------------------------
_S32_MSG = ('spkdiff: S32 spikes are only consumed by the fp6v2 MFMA conv (3x3/s1/p1 + BN + LIF, T=16, 7x7, fresh LIF '
            'state, S32 output)')
_C4_MSG = 'spkdiff: fp4-packed (C4) spikes are only consumed by the fp6 MFMA conv (3x3/s1/p1 + BN + LIF, T=16, C4 output)'


def test_s32_input_without_kernel(calls):
    with pytest.raises(NotImplementedError, match=re.escape(_S32_MSG)):
        _den().conv2.run(_s4(B, 2, 7, 7, 16, 16), IN_PTC, final='ptc', chunk_out=ops.CHUNK_S32)       # stateful


def test_c4_input_without_kernel(calls):
    with pytest.raises(NotImplementedError, match=re.escape(_C4_MSG)):
        _den().conv2.run(_s4(B, 1, 7, 7, 16, 32), IN_PTC, final='ptc', chunk_out=ops.CHUNK_C4, impl='direct')


def _stale(blk, shape):
    blk[2].v = _f32(*shape)
    return re.escape(f'LIFNode state has shape {tuple(shape)} but the input implies ')


@pytest.mark.parametrize('form', ['fp6', 'i8', 'gather', 'direct'])
def test_stale_membrane_shape(calls, form):
    if form in ('fp6', 'i8'):
        blk = _den().conv2
        x = _s4(B, 1, 7, 7, 16, 32) if form == 'fp6' else _u8(B, 2, 7, 7, 16, 32)
        msg = _stale(blk, (B, 128, 8, 8)) + re.escape(f'{(B, 128, 7, 7)}; call functional.reset_net first')
        args = dict(chunk_out=ops.CHUNK_C4 if form == 'fp6' else 32)
    else:
        blk = _vqvae(1).decoder.snn_convs
        x = _u8(B, 7, 7, 16, 16)
        msg = _stale(blk, (B, 64, 7, 7)) + re.escape(f'{(B, 64, 14, 14)}; call functional.reset_net first')
        args = dict(impl='direct') if form == 'direct' else {}
    with pytest.raises(RuntimeError, match='^' + msg + '$'):
        blk.run(x, IN_PTC, final='ptc', **args)
