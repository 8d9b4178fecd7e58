"""Which launches each configuration makes (CPU, no kernel runs).

Every kernel form of ``FusedSequential.run`` and the denoiser is bit-exact, so sending a layer to the wrong form changes no
number a parity test could see -- only the speed.  Here the ``spkdiff.ops`` wrappers that pack weights or launch kernels are
replaced by recorders that log the call with the arguments that pick its form and return zero tensors of the shape and dtype
the real wrapper returns (the next block dispatches on those); the pure-Python predicates stay real.  Each configuration's
call list, the pack calls included, is pinned as a literal below.
"""
import inspect
import re

import pytest
import torch

from spkdiff import ops
from spkdiff.fused import FusedSequential
from spkdiff.ops import IN_PTC, IN_SEQ, IN_TINV
from snn_model.vae_model import SNN_VQVAE
from snn_model.vq_diffusion import DummyModel, functional

B = 2
_MODES = {ops.MODE_LIF: 'LIF', ops.MODE_RAW: 'RAW', ops.MODE_MEMOUT: 'MEMOUT', ops.MODE_MEAN: 'MEAN'}
_KINDS = {IN_PTC: 'PTC', IN_TINV: 'TINV', IN_SEQ: 'SEQ'}
_VAE_OUT = {ops.VAE_OUT_COLLAPSED: 'COLLAPSED', ops.VAE_OUT_S32: 'S32', ops.VAE_OUT_PTC: 'PTC'}
_CHUNK = {ops.CHUNK_C4: 'C4', ops.CHUNK_S32: 'S32'}
# the arguments that pick a kernel form, as logged: a flag by its name when set, a choice as name=value when given
_FORM_ARGS = {
    'mode': _MODES.get, 'in_kind': _KINDS.get, 'out_kind': _VAE_OUT.get,
    'chunk_out': lambda c: _CHUNK.get(c, c), 'transposed': bool, 'want_counts': bool, 'out_s32': bool,
    'collapse_coef': lambda c: c is not None, 'v': lambda v: v is not None, 'pad_cout': bool,
    'want_ptc': bool, 'want_f32': bool, 'want_pre': bool,
}


def _u8(*s):
    return torch.zeros(s, dtype=torch.uint8)


def _f32(*s):
    return torch.zeros(s, dtype=torch.float32)


def _s4(*s):
    return torch.zeros(s, dtype=ops.C4_DTYPE)


def _hw(H, W, a):
    return (ops.conv_out_size(H, a['k'], a['stride'], a['pad'], a['transposed'], a['out_pad']),
            ops.conv_out_size(W, a['k'], a['stride'], a['pad'], a['transposed'], a['out_pad']))


def _conv_fused(a):
    in0, T, in_kind, mode = a['in0'], a['T'], a['in_kind'], a['mode']
    if in_kind == IN_PTC:
        Bn, H, W = (in0.shape[0], in0.shape[2], in0.shape[3]) if in0.dim() == 6 else in0.shape[:3]
    elif in_kind == IN_TINV:
        Bn, H, W = in0.shape[0], in0.shape[2], in0.shape[3]
    else:
        Bn, H, W = in0.shape[1], in0.shape[3], in0.shape[4]
    Cout = a['w_packed'].shape[2]
    Ho, Wo = _hw(H, W, a)
    res = {'ptc': None, 'f32': None, 'pre': None, 'u8': None, 'cnt': None}
    if mode == ops.MODE_LIF:
        co = a['chunk_out']
        if a['want_counts']:
            res['cnt'] = _u8(Bn, Cout // 32, Ho, Wo, 32)
        if a['want_ptc']:
            res['ptc'] = (_s4(Bn, Cout // 64, Ho, Wo, T, 32) if co == ops.CHUNK_C4 else
                          _s4(Bn, Cout // 32, Ho, Wo, T, 16) if co == ops.CHUNK_S32 else
                          _u8(Bn, Cout // co, Ho, Wo, T, co) if co else _u8(Bn, Ho, Wo, T, Cout))
        if a['want_f32']:
            res['f32'] = _f32(T, Bn, Cout, Ho, Wo)
        if a['want_pre']:
            res['pre'] = _f32(Bn, Cout, Ho, Wo) if in_kind == IN_TINV else _f32(T, Bn, Cout, Ho, Wo)
    elif mode == ops.MODE_RAW:
        res['f32'] = _f32(T, Bn, Cout, Ho, Wo)
    else:
        res['f32'] = _f32(Bn, Cout, Ho, Wo)
        res['u8'] = _u8(Bn, Cout, Ho, Wo) if a['want_u8'] else None
    return res


def _with_counts(out, a, cshape):
    return (out, _u8(*cshape)) if a['want_counts'] else out


def _den_mfma(a):
    Bn, _, H, W, T, _ = a['in0'].shape
    Cout = a['Cout']
    if a['mode'] == ops.MODE_LIF:
        return _with_counts(_u8(Bn, Cout // 32, H, W, T, 32), a, (Bn, Cout // 32, H, W, 32))
    return _f32(Bn, Cout, H, W)


def _den_fp6(a):
    Bn, _, H, W, T, _ = a['in0'].shape
    return _with_counts(_s4(Bn, a['Cout'] // 64, H, W, T, 32), a, (Bn, a['Cout'] // 32, H, W, 32))


def _den_fp6v2(a):
    Bn, _, H, W, T, _ = a['in0'].shape
    return _with_counts(_s4(Bn, a['Cout'] // 32, H, W, T, 16), a, (Bn, a['Cout'] // 32, H, W, 32))


def _vae_fp6_fwd(a):
    Bn, _, H, W, T, _ = a['in_s32'].shape
    Cout, kind = a['Cout'], a['out_kind']
    Ho, Wo = (2 * H, 2 * W) if a['transposed'] else (H // 2, W // 2)
    if kind == ops.VAE_OUT_COLLAPSED:
        return _f32(Bn, Ho, Wo, Cout)
    return _s4(Bn, Cout // 32, Ho, Wo, T, 16) if kind == ops.VAE_OUT_S32 else _u8(Bn, Ho, Wo, T, Cout)


def _conv_mfma_fused(a):
    Bn, H, W, T, _ = a['in_ptc'].shape
    Cout = a['Cout']
    Ho, Wo = _hw(H, W, a)
    if a['mode'] == ops.MODE_LIF:
        if a['out_s32']:
            return _s4(Bn, Cout // 32, Ho, Wo, T, 16)
        return _f32(Bn, Ho, Wo, Cout) if a['collapse_coef'] is not None else _u8(Bn, Ho, Wo, T, Cout)
    return {'f32': _f32(Bn, Cout, Ho, Wo), 'u8': _u8(Bn, Cout, Ho, Wo) if a['want_u8'] else None}


def _readout(a):
    Bn, H, W, _ = a['x_bhwc'].shape
    w = a['weight']
    Cout = w.shape[1] if a['transposed'] else w.shape[0]
    return {'f32': _f32(Bn, Cout, H, W), 'u8': _u8(Bn, Cout, H, W) if a['want_u8'] else None}


def _ptc_to_spikes(a):
    p = a['p']
    if p.dim() == 6:
        Bn, nch, H, W, T, rec = p.shape
        C = nch * (64 if p.dtype == ops.C4_DTYPE and rec == 32 else 32 if p.dtype == ops.C4_DTYPE else rec)
    else:
        Bn, H, W, T, C = p.shape
    return _f32(T, Bn, C, H, W)


def _ptc_to_s32(a):
    Bn, H, W, T, C = a['ptc'].shape
    return _s4(Bn, (C + 31) // 32, H, W, T, 16)


def _build_input(a):
    x = a['x']
    return a['out'] if a['out'] is not None else _f32(x.shape[0], 2, x.shape[-2], x.shape[-1])


def _step_tail(a):
    Bn, _, H, W, _ = a['cnt5'].shape
    nxt = None if a['conv1'] is None else (_s4(Bn, 2, H, W, a['T'], 16), _u8(Bn, 2, H, W, 32))
    return nxt, (_f32(Bn, a['K'], H, W) if a['want_logits'] else None)


def _embedding(a):
    tok, cb = a['tokens'], a['codebook']
    if a['nchw_hw'] is None:
        return _f32(*tok.shape, cb.shape[1])
    h, w = a['nchw_hw']
    return _f32(tok.numel() // (h * w), cb.shape[1], h, w)


def _wshape(a):
    w = a['w']
    return (w.shape[1], w.shape[0]) if a.get('transposed') else (w.shape[0], w.shape[1])      # (Cout, Cin)


_FAKES = {
    'bn_prepare': lambda a: (_f32(a['mean'].numel()), _f32(a['mean'].numel())),
    'pack_conv_weight': lambda a: _f32(a['w'].shape[2] * a['w'].shape[3], _wshape(a)[1], _wshape(a)[0]),
    'den_pack_weight_i8': lambda a: (torch.zeros(1, dtype=torch.int8), torch.zeros(1, dtype=torch.float64),
                                     torch.zeros(1, dtype=torch.float64)),
    'den_pack_weight_fp6': lambda a: (_u8(1), torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)),
    'den_pack_weight_fp6v2': lambda a: (_u8(1),) + (torch.zeros(1, dtype=torch.float64),) * 2 + (_f32(1), _f32(1)),
    'vae_fp6_pack': lambda a: (_u8(1),) + (torch.zeros(1, dtype=torch.float64),) * 2 + (_f32(1), _wshape(a)[1]),
    'pack_conv_weight_i8': lambda a: (torch.zeros(1, dtype=torch.int8), torch.zeros(1, dtype=torch.float64),
                                      torch.zeros(1, dtype=torch.float64)),
    'conv_fused': _conv_fused,
    'den_conv3x3_mfma': _den_mfma,
    'den_conv3x3_mfma_fp6': _den_fp6,
    'den_conv3x3_mfma_fp6v2': _den_fp6v2,
    'den_conv3x3_counts': lambda a: _f32(a['cnt0'].shape[0], a['Cout'], a['cnt0'].shape[2], a['cnt0'].shape[3]),
    'vae_fp6_fwd': _vae_fp6_fwd,
    'conv_mfma_fused': _conv_mfma_fused,
    'readout_collapsed': _readout,
    'ptc_to_s32': _ptc_to_s32,
    'ptc_to_spikes': _ptc_to_spikes,
    'den_build_input': _build_input,
    'den_step_tail': _step_tail,
    'spikegen_tokens_s32': lambda a: _s4(a['tokens'].shape[0], 1, a['tokens'].shape[1], a['tokens'].shape[2], a['T'], 16),
    'embedding': _embedding,
}


def _install_recorders(monkeypatch):
    log = []
    for name, fake in _FAKES.items():
        sig = inspect.signature(getattr(ops, name))

        def rec(*args, _name=name, _fake=fake, _sig=sig, **kwargs):
            bound = _sig.bind(*args, **kwargs)
            bound.apply_defaults()
            a = bound.arguments
            vals = [(k, f(a[k])) for k, f in _FORM_ARGS.items() if k in a]
            form = ', '.join(k if v is True else f'{k}={v}' for k, v in vals if v is not None and v is not False)
            log.append(f'{_name}({form})' if form else _name)
            return _fake(a)
        monkeypatch.setattr(ops, name, rec)
    return log


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
