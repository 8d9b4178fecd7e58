"""Recorders for the launch-sequence tests (tests/test_fused_dispatch.py, tests/test_sampler_dispatch.py).

The ``spkdiff.ops`` wrappers that pack weights or launch kernels are replaced by recorders that log the call with the
arguments that pick its form and return zero tensors of the shape and dtype the real wrapper returns (the next block
dispatches on those); the pure-Python predicates stay real.
"""
import inspect

import torch

from spkdiff import ops
from spkdiff.ops import IN_PTC, IN_SEQ, IN_TINV

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


def _given(v):
    return v is not None


def _pair_or(out, make):
    return out if out is not None else make()


# the sampler's own launches (tests/test_sampler_dispatch.py) and the further arguments that test logs
_SAMPLER_FAKES = {
    'select_active': lambda a: _pair_or(a['out'], lambda: (torch.zeros(a['unmasked'].shape[0], dtype=torch.int32),
                                                           torch.zeros(2, dtype=torch.int32))),
    'select_needed': lambda a: a['need'],
    'psample_step': lambda a: (a['x_t'], a['unmasked']),
    'completion_state': lambda a: _pair_or(a['out'], lambda: (
        torch.zeros((a['codes'].shape[0], 1) + tuple(a['codes'].shape[-2:]), dtype=torch.int64),
        torch.zeros((a['codes'].shape[0], 1) + tuple(a['codes'].shape[-2:]), dtype=torch.bool))) + (None,),
}
_SAMPLER_FORM_ARGS = {
    'need_radius': lambda r: r, 'conv1': _given, 'want_logits': bool, 'u': _given, 'q': _given, 'philox_state': _given,
    'next_input': _given, 'out': _given,
}


def _install_recorders(monkeypatch, sampler=False):
    log = []
    fakes = dict(_FAKES, **_SAMPLER_FAKES) if sampler else _FAKES
    form_args = dict(_FORM_ARGS, **_SAMPLER_FORM_ARGS) if sampler else _FORM_ARGS
    for name, fake in fakes.items():
        sig = inspect.signature(getattr(ops, name))

        def rec(*args, _name=name, _fake=fake, _sig=sig, **kwargs):
            bound = _sig.bind(*args, **kwargs)
            bound.apply_defaults()
            a = bound.arguments
            vals = [(k, f(a[k])) for k, f in form_args.items() if k in a]
            form = ', '.join(k if v is True else f'{k}={v}' for k, v in vals if v is not None and v is not False)
            log.append(f'{_name}({form})' if form else _name)
            return _fake(a)
        monkeypatch.setattr(ops, name, rec)
    return log
