"""Tensor-level wrappers over the C-ABI: validate, allocate outputs with torch, launch on torch's current stream.

PyTorch is plumbing here (device memory, streams); every operation is executed by ``libspkdiff.so``.
All tensors must live on a ROCm device ("cuda"); CPU tensors are rejected -- there is no fallback.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, lib

# The C-ABI's enumerations and limits keep their Python names here; include/spkdiff.h defines each one (SPK_<name>).
_C = _lib.CONSTANTS
MODE_LIF, MODE_RAW, MODE_MEMOUT, MODE_MEAN = (_C["SPK_MODE_" + n] for n in ("LIF", "RAW", "MEMOUT", "MEAN"))
SPIKE_F32, SPIKE_U8, SPIKE_BITS = (_C["SPK_SPIKE_" + n] for n in ("F32", "U8", "BITS"))
MAX_T = 16


# ---------------------------------------------------------------------------------------------- active-set batch
# Set by the sampler around one denoiser call (``with ops.active_set(active, n_active)``): the per-step kernels then
# process only the images listed by spk_select_active -- ``active`` int32 [B] (slot -> image), ``n_active`` int32 [2] (count, work word),
# both on the device, so that a captured hipGraph replays with fresh lists.  None = every image (dense).
# ``need`` (optional, spk_select_needed): the positions of each active image the step will read, per layer depth; the
# layers that take position lists then compute only those.
ACTIVE = None
NEED = None


class active_set:
    def __init__(self, active, n_active, need=None):
        self.pair = None if active is None else (active, n_active)
        self.need = need if active is not None else None

    def __enter__(self):
        global ACTIVE, NEED
        self.prev, ACTIVE = ACTIVE, self.pair
        self.prev_need, NEED = NEED, self.need
        return self

    def __exit__(self, *exc):
        global ACTIVE, NEED
        ACTIVE = self.prev
        NEED = self.prev_need
        return False


def _n_dyn():
    return None if ACTIVE is None else ACTIVE[1].data_ptr()


# ---------------------------------------------------------------------------------------------- in-situ kernel timing
# bench.py switches this on to bracket named launches with HIP events recorded on the SAME stream the kernels
# are enqueued on (torch's current stream): TIMERS[tag] = [(start_event, end_event), ...].
TIMERS = None


class timed:
    __slots__ = ("tag", "e1")

    def __init__(self, tag):
        self.tag = tag

    def __enter__(self):
        if TIMERS is not None and self.tag is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            TIMERS.setdefault(self.tag, []).append((e0, self.e1))
        return self

    def __exit__(self, *exc):
        if TIMERS is not None and self.tag is not None:
            self.e1.record()
        return False


def _stream(t: torch.Tensor):
    """HIP stream the launch goes to: torch's current stream of the tensor's device.  A launch is issued in the calling
    thread's current device context, so a tensor on another GPU is refused rather than launched into the wrong context
    (this package runs one process per GPU; ``with torch.cuda.device(t.device):`` around the call is the way to address
    a second device from one process)."""
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        raise RuntimeError(f"spkdiff: tensor on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                           "wrap the call in `with torch.cuda.device(tensor.device):`")
    return torch.cuda.current_stream(t.device).cuda_stream


def _dev(t: torch.Tensor, name: str, dtype=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"spkdiff: {name} is on '{t.device}'. The HIP kernels are the implementation; "
                           "there is no CPU path (move the module / tensors to a ROCm device).")
    if dtype is not None and t.dtype != dtype:
        raise NotImplementedError(f"spkdiff: {name} must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _state(t: torch.Tensor, name: str):
    """A tensor the kernel updates in place.  ``_dev`` would hand the kernel a contiguous COPY of a non-contiguous one and the
    caller's tensor would silently keep its old values, so such a tensor is refused."""
    if isinstance(t, torch.Tensor) and not t.is_contiguous():
        raise ValueError(f"spkdiff: {name} is updated in place and must be contiguous (shape {tuple(t.shape)}, strides "
                         f"{tuple(t.stride())}); a copy would take the update and {name} itself would not advance. "
                         f"Pass {name}.contiguous() and keep that tensor as the state.")
    return _dev(t, name, torch.float32)


def _p(t):
    return None if t is None else t.data_ptr()


def conv_out_size(n, k, stride, pad, transposed=False, out_pad=0):
    return lib.spk_conv_out_size(n, k, stride, pad, int(transposed), out_pad)


def clock_probe(device, target_ms: float = 4.0):
    """Shader clock [GHz] this device holds under a block-scaled fp6 x fp4 MFMA load (spk_clock_probe): median over
    the workgroups of d(s_memtime) / d(s_memrealtime) * 0.1.  Synchronises.  Measurement aid for bench.py."""
    nblk = torch.cuda.get_device_properties(device).multi_processor_count
    out = torch.zeros((nblk, 4), dtype=torch.int64, device=device)
    iters = max(1000, int(target_ms * 1e-3 / (4 * 33 / 2.0e9)))
    check(lib.spk_clock_probe(_p(out), nblk, iters, _stream(out)), "spk_clock_probe")
    o = out.cpu().double()
    ghz = (o[:, 0] / o[:, 1].clamp(min=1)) * 0.1
    cyc_per_mfma = o[:, 0] / o[:, 2].clamp(min=1)
    return {"ghz_median": float(ghz.median()), "ghz_min": float(ghz.min()), "ghz_max": float(ghz.max()),
            "cycles_per_mfma": float(cyc_per_mfma.median()), "workgroups": int(nblk), "mfma_per_wave": int(4 * iters)}


# ---------------------------------------------------------------------------------------------- neuron
def lif_fwd(x_seq: torch.Tensor, v: torch.Tensor, tau=2.0, v_threshold=1.0, v_reset=0.0, spike_dtype=SPIKE_F32):
    """x_seq [T, ...] fp32, v [...] fp32 contiguous (updated in place; a non-contiguous v is a ValueError) -> spikes. Mirrors the cupy-plugin contract
    SJ/activation_based/neuron.py:954-966 (x_seq.flatten(1), v.flatten(0))."""
    v = _state(v, "v")
    x_seq = _dev(x_seq, "x_seq", torch.float32)
    T = x_seq.shape[0]
    N = x_seq[0].numel()
    if v.numel() != N:
        raise ValueError(f"v has {v.numel()} elements, x_seq[0] has {N}")
    if spike_dtype == SPIKE_F32:
        out = torch.empty_like(x_seq)
    elif spike_dtype == SPIKE_U8:
        out = torch.empty(x_seq.shape, dtype=torch.uint8, device=x_seq.device)
    elif spike_dtype == SPIKE_BITS:
        out = torch.empty((T, (N + 63) // 64), dtype=torch.int64, device=x_seq.device)
    else:
        raise NotImplementedError(spike_dtype)
    check(lib.spk_lif_fwd(_p(x_seq), _p(v), _p(out), T, N, float(tau), float(v_threshold), float(v_reset),
                          spike_dtype, _stream(x_seq)), "spk_lif_fwd")
    return out


def lif_fwd_ex(x_seq: torch.Tensor, v: torch.Tensor, tau=2.0, v_threshold=1.0, v_reset=0.0, soft_reset=False, decay_input=True,
               want_v_seq=False):
    """The reference neuron's other eval forms (spk_lif_fwd_ex): soft reset, decay_input=False, v_seq.  Returns
    (spikes fp32 like x_seq, v_seq or None); v (contiguous, else ValueError) updated in place."""
    v = _state(v, "v")
    x_seq = _dev(x_seq, "x_seq", torch.float32)
    T, N = x_seq.shape[0], x_seq[0].numel()
    if v.numel() != N:
        raise ValueError(f"v has {v.numel()} elements, x_seq[0] has {N}")
    out = torch.empty_like(x_seq)
    v_seq = torch.empty_like(x_seq) if want_v_seq else None
    check(lib.spk_lif_fwd_ex(_p(x_seq), _p(v), _p(out), _p(v_seq), T, N, float(tau), float(v_threshold),
                             0.0 if v_reset is None else float(v_reset), int(bool(soft_reset)), int(bool(decay_input)),
                             _stream(x_seq)), "spk_lif_fwd_ex")
    return out, v_seq


# ---------------------------------------------------------------------------------------------- stateless layers
def lif_train_fwd(x_seq: torch.Tensor, v_init: torch.Tensor, tau=2.0, v_threshold=1.0, v_reset=0.0):
    """Training-mode multi-step LIF (hard reset, decay_input). Returns (spike_seq, h_seq, v_last), all fp32."""
    x = _dev(x_seq, "x_seq", torch.float32)
    v0 = _dev(v_init, "v", torch.float32)
    T = x.shape[0]
    N = x[0].numel()
    if v0.numel() != N:
        raise ValueError(f"v has {v0.numel()} elements, x_seq[0] has {N}")
    h = torch.empty_like(x)
    s = torch.empty_like(x)
    v_last = torch.empty_like(v0)
    check(lib.spk_lif_train_fwd(_p(x), _p(v0), _p(h), _p(s), _p(v_last), T, N, float(tau), float(v_threshold),
                                float(v_reset), _stream(x)), "spk_lif_train_fwd")
    return s, h, v_last


def lif_train_bwd(grad_spike_seq, grad_v_last, h_seq, tau=2.0, v_threshold=1.0, v_reset=0.0, alpha=2.0,
                  detach_reset=False, need_grad_v=True):
    """BPTT of lif_train_fwd with the ATan surrogate. Returns (grad_x_seq, grad_v_init or None)."""
    gs = _dev(grad_spike_seq, "grad_spike_seq", torch.float32)
    h = _dev(h_seq, "h_seq", torch.float32)
    gv = None if grad_v_last is None else _dev(grad_v_last, "grad_v_last", torch.float32)
    T = h.shape[0]
    N = h[0].numel()
    gx = torch.empty_like(h)
    gv0 = torch.empty(h.shape[1:], dtype=torch.float32, device=h.device) if need_grad_v else None
    check(lib.spk_lif_train_bwd(_p(gs), _p(gv), _p(h), _p(gx), _p(gv0), T, N, float(tau), float(v_threshold),
                                float(v_reset), float(alpha), int(bool(detach_reset)), _stream(h)), "spk_lif_train_bwd")
    return gx, gv0


class LIFTrainFunction(torch.autograd.Function):
    """spike_seq, v_last = f(x_seq, v_init): the HIP counterpart of the reference's LIFNodeATGF
    (SJ/activation_based/auto_cuda/neuron_kernel.py:496-540), ATan surrogate."""

    @staticmethod
    def forward(ctx, x_seq, v_init, tau, v_threshold, v_reset, alpha, detach_reset):
        s, h, v_last = lif_train_fwd(x_seq, v_init, tau, v_threshold, v_reset)
        ctx.save_for_backward(h)
        ctx.cfg = (tau, v_threshold, v_reset, alpha, detach_reset)
        return s, v_last

    @staticmethod
    def backward(ctx, grad_s, grad_v_last):
        (h,) = ctx.saved_tensors
        tau, v_threshold, v_reset, alpha, detach_reset = ctx.cfg
        gs = grad_s if grad_s is not None else torch.zeros_like(h)
        gx, gv0 = lif_train_bwd(gs.contiguous(), None if grad_v_last is None else grad_v_last.contiguous(), h, tau,
                                v_threshold, v_reset, alpha, detach_reset, need_grad_v=ctx.needs_input_grad[1])
        return gx, gv0, None, None, None, None, None


def _cl5(x, name):
    """[T,B,C,H,W] fp32 device tensor -> the same values with channels-last memory ([T][B][H][W][C]); no copy if it
    already is (the output of a channels-last library convolution viewed as [T,B,...])."""
    if not x.is_cuda:
        raise RuntimeError(f"spkdiff: {name} is on '{x.device}'; there is no CPU path")
    if x.dtype != torch.float32:
        raise NotImplementedError(f"spkdiff: {name} must be float32, got {x.dtype}")
    if x.permute(0, 1, 3, 4, 2).is_contiguous():
        return x
    return x.flatten(0, 1).contiguous(memory_format=torch.channels_last).view(x.shape)


def _cl4(x, name):
    if x is None:
        return None
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError(f"spkdiff: {name} must be a float32 device tensor")
    return x if x.permute(0, 2, 3, 1).is_contiguous() else x.contiguous(memory_format=torch.channels_last)


def _empty_cl(shape, device):
    """Uninitialised fp32 [..., C, H, W] tensor whose memory is [...][H][W][C]."""
    perm = tuple(range(len(shape) - 3)) + (len(shape) - 2, len(shape) - 1, len(shape) - 3)
    inv = tuple(range(len(shape) - 3)) + (len(shape) - 1, len(shape) - 3, len(shape) - 2)
    return torch.empty(tuple(shape[i] for i in perm), dtype=torch.float32, device=device).permute(inv)


class BNLIFTrainFunction(torch.autograd.Function):
    """spike_seq, v_last = f(y_seq, gamma, beta, v_init): training-mode BatchNorm2d (batch statistics over T*B*H*W,
    running statistics updated in place) fused with the surrogate-gradient LIF -- the tail of one denoiser block in
    train() mode (SJ/activation_based/layer.py:458-465 + neuron.py:739-749,133-135).  y_seq [T,B,C,H,W] fp32.
    Only y and the two per-channel statistics are kept for the backward, which recomputes the membrane potentials.
    The kernels work on channels-last memory ([T][B][H][W][C]): inputs in another layout are converted, outputs and
    gradients are returned channels-last (what the library's NHWC convolutions consume without a transpose)."""

    @staticmethod
    def forward(ctx, y_seq, gamma, beta, v_init, running_mean, running_var, momentum, eps, tau, v_threshold, v_reset,
                alpha, detach_reset, want_c4=False):
        # want_c4: a THIRD output, the spikes as C4 records (the next block's exact MFMA forward reads them: no conversion launch)
        if y_seq.dim() != 5:
            raise ValueError(f'expected y_seq with shape [T, N, C, H, W], but got {tuple(y_seq.shape)}')
        y = _cl5(y_seq, "y_seq")
        T, B, C = int(y.shape[0]), int(y.shape[1]), int(y.shape[2])
        HW = int(y.shape[3] * y.shape[4])
        g = None if gamma is None else _dev(gamma, "gamma", torch.float32)
        b = None if beta is None else _dev(beta, "beta", torch.float32)
        v0 = _cl4(v_init, "v")
        if v0 is not None and tuple(v0.shape) != tuple(y.shape[1:]):
            raise RuntimeError(f"LIFNode state has shape {tuple(v0.shape)} but the input implies {tuple(y.shape[1:])}; "
                               "call functional.reset_net first")
        for name, r in (("running_mean", running_mean), ("running_var", running_var)):
            if r is not None and (not r.is_cuda or r.dtype != torch.float32 or not r.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous fp32 device tensor (updated in place)")
        ws = torch.empty(int(lib.spk_bn_lif_train_ws_bytes(B, C, HW)), dtype=torch.uint8, device=y.device)
        s = _empty_cl(y.shape, y.device)
        v_last = _empty_cl(y.shape[1:], y.device)
        mean = torch.empty(C, dtype=torch.float32, device=y.device)
        invstd = torch.empty(C, dtype=torch.float32, device=y.device)
        c4 = None
        if want_c4 and C % 64 == 0 and C // 4 <= 256 and 256 % (C // 4) == 0 and all(
                t is None or t.data_ptr() % 16 == 0 for t in (y, s, v0, v_last)):
            c4 = empty_spikes(C4, B, C, int(y.shape[3]), int(y.shape[4]), T, y.device)
        with timed("train.bn_lif_fwd"):
            check(lib.spk_bn_lif_train_fwd_c4(_p(y), _p(g), _p(b), _p(running_mean), _p(running_var), float(momentum),
                                              float(eps), _p(v0), _p(s), _p(v_last), _p(mean), _p(invstd), _p(c4), _p(ws),
                                              ws.numel(), T, B, C, HW, float(tau), float(v_threshold), float(v_reset),
                                              _stream(y)), "spk_bn_lif_train_fwd_c4")
        ctx.save_for_backward(y, g, b, mean, invstd, v0)
        ctx.cfg = (tau, v_threshold, v_reset, alpha, detach_reset)
        # v_last usually ends in lif.v and nowhere in the loss: without this autograd materialises a zero gradient for it on every
        # backward (a fill + a layout copy per block and iteration); the kernel takes a null pointer for "no gradient"
        ctx.set_materialize_grads(False)
        if not want_c4:
            return s, v_last
        if c4 is not None:
            ctx.mark_non_differentiable(c4)
        return s, v_last, c4

    @staticmethod
    def backward(ctx, grad_s, grad_v_last, *_):
        y, g, b, mean, invstd, v0 = ctx.saved_tensors
        tau, v_threshold, v_reset, alpha, detach_reset = ctx.cfg
        T, B, C = int(y.shape[0]), int(y.shape[1]), int(y.shape[2])
        HW = int(y.shape[3] * y.shape[4])
        # grad_s as autograd left it: a dense channels-last tensor, or -- in front of the denoiser's last layer -- ONE [B,C,H,W]
        # gradient broadcast over T (stride 0) and / or a channel slice of a wider channels-last tensor (cat(x5, x1) backward):
        # the kernel takes the step stride and the row pitch instead of an expanded copy (25.7 MB for conv5's spikes at B = 32)
        gs_ts, gs_pitch = B * HW * C, C
        gs = None
        if grad_s is None and grad_v_last is None:
            return (None,) * 14
        if grad_s is not None and grad_s.is_cuda and grad_s.dtype == torch.float32 and grad_s.dim() == 5:
            st = grad_s.stride()
            Hh, Ww = int(y.shape[3]), int(y.shape[4])
            pitch = st[4]
            if (st[2] == 1 and st[3] == Ww * pitch and st[1] == Hh * Ww * pitch and pitch >= C and pitch % 4 == 0 and
                    st[0] in (0, B * Hh * Ww * pitch) and st[0] % 4 == 0 and grad_s.data_ptr() % 16 == 0 and
                    (st[0] == 0 or pitch != C)):
                gs, gs_ts, gs_pitch = grad_s, int(st[0]), int(pitch)
        if gs is None:
            gs = _empty_cl(y.shape, y.device).zero_() if grad_s is None else _cl5(grad_s, "grad_spike_seq")
        gv = _cl4(grad_v_last, "grad_v_last")
        ws = torch.empty(int(lib.spk_bn_lif_train_ws_bytes(B, C, HW)), dtype=torch.uint8, device=y.device)
        gy = _empty_cl(y.shape, y.device)
        gg = torch.empty(C, dtype=torch.float32, device=y.device)
        gb = torch.empty(C, dtype=torch.float32, device=y.device)
        gv0 = _empty_cl(y.shape[1:], y.device) if (v0 is not None and ctx.needs_input_grad[3]) else None
        with timed("train.bn_lif_bwd"):
            check(lib.spk_bn_lif_train_bwd_strided(_p(gs), int(gs_ts), int(gs_pitch), _p(gv), _p(y), _p(g), _p(b), _p(mean),
                                                   _p(invstd), _p(v0), _p(gy), _p(gg), _p(gb), _p(gv0), _p(ws), ws.numel(), T, B,
                                                   C, HW, float(tau), float(v_threshold), float(v_reset), float(alpha),
                                                   int(bool(detach_reset)), _stream(y)), "spk_bn_lif_train_bwd_strided")
        return (gy, gg if g is not None else None, gb if b is not None else None, gv0) + (None,) * 10


class MaskedCEFunction(torch.autograd.Function):
    """loss = sum_b coef_b * sum_p ce[b, p] with ce the masked cross-entropy of R/snn_model/vq_diffusion.py:85-88
    (ignore_index = -1).  logits [B,K,h,w] fp32, target [B,1,h,w] (or [B,h,w]) fp32 token ids, coef [B] fp32.
    Forward and gradient come from one spk_masked_ce launch; the weighted sum over [B, hw] is a tiny torch reduction."""

    @staticmethod
    def forward(ctx, logits, target, coef):
        lg = _dev(logits, "logits", torch.float32)
        B, K = int(lg.shape[0]), int(lg.shape[1])
        HW = lg[0, 0].numel()
        tg = _dev(target, "target", torch.float32)
        cf = _dev(coef, "coef", torch.float32)
        if tg.numel() != B * HW or cf.numel() != B:
            raise ValueError("target must have B*h*w entries and coef B entries")
        ce = torch.empty((B, HW), dtype=torch.float32, device=lg.device)
        dl = torch.empty_like(lg) if ctx.needs_input_grad[0] else None
        check(lib.spk_masked_ce(_p(lg), _p(tg), _p(cf), _p(ce), _p(dl), B, K, HW, _stream(lg)), "spk_masked_ce")
        ctx.has_dl = dl is not None
        if dl is not None:
            ctx.save_for_backward(dl)          # survives retain_graph / a second backward like any saved tensor
        return (ce.sum(1) * cf).sum()

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.has_dl:
            return None, None, None
        (dl,) = ctx.saved_tensors
        return dl * grad_out, None, None


def masked_ce(logits, target):
    """Per-position masked cross-entropy [B, hw] (no gradient): the forward half of spk_masked_ce."""
    lg = _dev(logits, "logits", torch.float32)
    B, K = int(lg.shape[0]), int(lg.shape[1])
    HW = lg[0, 0].numel()
    tg = _dev(target, "target", torch.float32)
    ce = torch.empty((B, HW), dtype=torch.float32, device=lg.device)
    check(lib.spk_masked_ce(_p(lg), _p(tg), None, _p(ce), None, B, K, HW, _stream(lg)), "spk_masked_ce")
    return ce


def bn_prepare(gamma, beta, mean, var, eps):
    mean = _dev(mean, "running_mean", torch.float32)
    var = _dev(var, "running_var", torch.float32)
    C = mean.numel()
    a = torch.empty(C, dtype=torch.float32, device=mean.device)
    b = torch.empty_like(a)
    g = None if gamma is None else _dev(gamma.detach(), "bn.weight", torch.float32)
    be = None if beta is None else _dev(beta.detach(), "bn.bias", torch.float32)
    check(lib.spk_bn_prepare(_p(g), _p(be), _p(mean), _p(var), float(eps), _p(a), _p(b), C, _stream(mean)),
          "spk_bn_prepare")
    return a, b


def bn_eval(x, a, b):
    """x [M, C, H, W] (or [M, C, HW]) fp32."""
    x = _dev(x, "x", torch.float32)
    M, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    y = torch.empty_like(x)
    check(lib.spk_bn_eval_fwd(_p(x), _p(a), _p(b), _p(y), M, C, HW, _stream(x)), "spk_bn_eval_fwd")
    return y


def conv2d(x, w, bias, stride, pad):
    x = _dev(x, "x", torch.float32)
    w = _dev(w.detach(), "weight", torch.float32)
    b = None if bias is None else _dev(bias.detach(), "bias", torch.float32)
    M, Cin, H, W = x.shape
    Cout, Cin_w, k, k2 = w.shape
    if Cin_w != Cin or k != k2:
        raise ValueError(f"weight {tuple(w.shape)} does not match input channels {Cin} / square kernels only")
    Ho, Wo = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    y = torch.empty((M, Cout, Ho, Wo), dtype=torch.float32, device=x.device)
    check(lib.spk_conv2d_fwd(_p(x), _p(w), _p(b), _p(y), M, Cin, H, W, Cout, k, stride, pad, _stream(x)),
          "spk_conv2d_fwd")
    return y


def conv_transpose2d(x, w, bias, stride, pad, out_pad):
    x = _dev(x, "x", torch.float32)
    w = _dev(w.detach(), "weight", torch.float32)
    b = None if bias is None else _dev(bias.detach(), "bias", torch.float32)
    M, Cin, H, W = x.shape
    Cin_w, Cout, k, k2 = w.shape
    if Cin_w != Cin or k != k2:
        raise ValueError(f"weight {tuple(w.shape)} does not match input channels {Cin} / square kernels only")
    Ho, Wo = conv_out_size(H, k, stride, pad, True, out_pad), conv_out_size(W, k, stride, pad, True, out_pad)
    y = torch.empty((M, Cout, Ho, Wo), dtype=torch.float32, device=x.device)
    check(lib.spk_conv_transpose2d_fwd(_p(x), _p(w), _p(b), _p(y), M, Cin, H, W, Cout, k, stride, pad, out_pad,
                                       _stream(x)), "spk_conv_transpose2d_fwd")
    return y


class ExactConvTrainFunction(torch.autograd.Function):
    """y = conv2d / conv_transpose2d(x, weight) + bias in training: the forward is this library's direct kernel (fp64
    accumulation: the correctly rounded exact result, the same numbers as the inference path and -- up to the reference's
    own fp32 round-off -- the reference's), the backward is the framework's convolution backward.  Used for the small
    layers (VQ-VAE, the denoiser's first convolution); the denoiser's spike-input layers use SpikeConvTrainFunction."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, transposed, out_pad):
        if transposed:
            y = conv_transpose2d(x, weight, bias, stride, pad, out_pad)
        else:
            y = conv2d(x, weight, bias, stride, pad)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (int(stride), int(pad), bool(transposed), int(out_pad), bias is not None)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        stride, pad, transposed, out_pad, has_bias = ctx.cfg
        cout = int(weight.shape[1] if transposed else weight.shape[0])
        if (NATIVE_WGRAD and not transposed and not ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and stride == 1 and
                pad == 1 and tuple(weight.shape[2:]) == (3, 3) and int(weight.shape[1]) <= 4 and x.dim() == 4 and
                lib.spk_conv3x3_wgrad_small_ws_bytes(int(x.shape[0]), int(x.shape[2]), int(x.shape[3]), cout,
                                                     int(weight.shape[1])) > 0):
            # few input channels, dense input, no input gradient wanted: the denoiser's first layer (spk_conv3x3_wgrad_small:
            # maps up to 8x8 -- larger ones answer the workspace query with -1 and take the framework's operator below)
            return (None,) + conv3x3_wgrad_small(grad_y, x, weight, has_bias and ctx.needs_input_grad[2]) + (None,) * 4
        needs = (bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1]), bool(has_bias and ctx.needs_input_grad[2]))
        if conv_train_supported(x.shape, weight, stride, pad, transposed, out_pad, needs[0]):
            # the native data / weight gradients of csrc/conv_train.hip (the VQ-VAE's stride-2, 1x1 and transposed layers)
            return conv_train_backward(grad_y, x, weight, stride, pad, transposed, out_pad, needs) + (None,) * 4
        gi, gw, gb = torch.ops.aten.convolution_backward(
            grad_y.contiguous(), x.contiguous(), weight, [cout], [stride, stride], [pad, pad], [1, 1], transposed,
            [out_pad, out_pad], 1, list(needs))
        return gi, gw, gb, None, None, None, None


# ---- native training convolutions (csrc/conv_train.hip): the VQ-VAE's stride-2 / 1x1 / transposed layers ---------------------
NATIVE_TRAIN_CONV = True        # False: the framework's (library) convolution backward, as in rounds 3-4
NATIVE_TRAIN_FORWARD = True     # False: exact direct kernel / library forward by ops.EXACT_TRAIN_FORWARD_MACS (the parity runs)


def _conv_w_strides(weight, transposed):
    """(tap, cin, cout) element strides of a convolution weight as stored ([Cout,Cin,k,k] / [Cin,Cout,k,k], contiguous or
    channels-last), or None when the taps are not k*k equally spaced elements."""
    st, k = weight.stride(), int(weight.shape[2])
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or (k > 1 and st[2] != k * st[3]):
        return None
    tap = int(st[3]) if k > 1 else 0
    return (tap, int(st[0]), int(st[1])) if transposed else (tap, int(st[1]), int(st[0]))


def _conv_train_geometry(xshape, weight, stride, pad, transposed, out_pad):
    N, Cin, Hi, Wi = (int(v) for v in xshape)
    k = int(weight.shape[2])
    Cout = int(weight.shape[1] if transposed else weight.shape[0])
    Ho, Wo = (conv_out_size(Hi, k, stride, pad, transposed, out_pad), conv_out_size(Wi, k, stride, pad, transposed, out_pad))
    return N, Cin, Hi, Wi, Cout, Ho, Wo, k


def conv_train_supported(xshape, weight, stride, pad, transposed, out_pad, need_gi=True, forward=False):
    """Do the native training kernels take this layer (backward: data gradient if wanted + weight gradient; forward=True: the
    forward as well)?"""
    if not NATIVE_TRAIN_CONV or len(xshape) != 4 or weight.dim() != 4 or not weight.is_cuda or weight.dtype != torch.float32:
        return False
    if _conv_w_strides(weight, transposed) is None or int(weight.shape[1 if not transposed else 0]) != int(xshape[1]):
        return False
    N, Cin, Hi, Wi, Cout, Ho, Wo, k = _conv_train_geometry(xshape, weight, stride, pad, transposed, out_pad)
    if transposed and (out_pad >= stride or (Hi - 1) * stride - 2 * pad + k + out_pad != Ho):
        return False
    f_fwd, f_bwd = (1, 0) if transposed else (0, 1)
    if forward and not lib.spk_conv_train_gather_supported(Cin, Cout, k, stride, f_fwd):
        return False
    if need_gi and not lib.spk_conv_train_gather_supported(Cout, Cin, k, stride, f_bwd):
        return False
    if transposed:          # u = gy (finer grid), v = the input
        return lib.spk_conv_train_wgrad_ws_bytes(N, Hi, Wi, Cout, Cin, k) > 0
    return lib.spk_conv_train_wgrad_ws_bytes(N, Ho, Wo, Cin, Cout, k) > 0


def conv_train_forward(x, weight, bias, stride, pad, transposed, out_pad, relu=False):
    """y [N,Cout,Ho,Wo] (channels-last memory) = conv2d / conv_transpose2d(x, weight) + bias on the fp32 matrix cores
    (spk_conv_train_gather); ``relu``: relu(y) from the same launch (spk_conv_train_gather_relu)."""
    xin = _cl4(x.detach(), "x")
    w = weight.detach()
    N, Cin, Hi, Wi, Cout, Ho, Wo, k = _conv_train_geometry(xin.shape, w, stride, pad, transposed, out_pad)
    tap, s_ci, s_co = _conv_w_strides(w, transposed)
    y = _empty_cl((N, Cout, Ho, Wo), xin.device)
    b = None if bias is None else _dev(bias.detach(), "bias", torch.float32)
    name = "spk_conv_train_gather_relu" if relu else "spk_conv_train_gather"
    with timed("train.conv_fwd"):
        check(getattr(lib, name)(_p(xin), _p(w), _p(b), _p(y), N, Hi, Wi, Cin, Ho, Wo, Cout, k, stride, pad,
                                 1 if transposed else 0, tap, s_ci, s_co, _stream(xin)), name)
    return y


def conv_train_backward(grad_y, x, weight, stride, pad, transposed, out_pad, needs, relu_input=False):
    """(gi, gw, gb) of a convolution layer from gy (any layout; converted to channels-last if it is not), the saved input and
    the weight: spk_conv_train_gather in the transposed role + spk_conv_train_wgrad.  gw in the memory format of ``weight``.
    ``relu_input``: ``x`` is the result of a ReLU and gi is the gradient in front of it (zero where x <= 0), from the same launch
    (spk_conv_train_gather_masked)."""
    gy = _cl4(grad_y, "grad_y")
    xin = _cl4(x.detach(), "x")
    w = weight.detach()
    N, Cin, Hi, Wi, Cout, Ho, Wo, k = _conv_train_geometry(xin.shape, w, stride, pad, transposed, out_pad)
    tap, s_ci, s_co = _conv_w_strides(w, transposed)
    st = _stream(gy)
    gi = gw = gb = None
    if needs[0]:
        gi = _empty_cl((N, Cin, Hi, Wi), gy.device)
        geo = (N, Ho, Wo, Cout, Hi, Wi, Cin, k, stride, pad, 0 if transposed else 1, tap, s_co, s_ci, st)
        with timed("train.conv_bwd_data"):
            if relu_input:
                check(lib.spk_conv_train_gather_masked(_p(gy), _p(w), None, _p(xin), _p(gi), *geo), "spk_conv_train_gather_masked")
            else:
                check(lib.spk_conv_train_gather(_p(gy), _p(w), None, _p(gi), *geo), "spk_conv_train_gather")
    if needs[1] or needs[2]:
        gw = torch.empty_like(w)                     # (the memory format of a dense weight is preserved; the kernel takes gw's own strides)
        g_tap, g_ci, g_co = _conv_w_strides(gw, transposed)
        gb = torch.empty(Cout, dtype=torch.float32, device=gy.device) if needs[2] else None
        if transposed:
            u, v, Hu, Wu, Cu, Hv, Wv, Cv, g_u, g_v, bf = gy, xin, Ho, Wo, Cout, Hi, Wi, Cin, g_co, g_ci, 2
        else:
            u, v, Hu, Wu, Cu, Hv, Wv, Cv, g_u, g_v, bf = xin, gy, Hi, Wi, Cin, Ho, Wo, Cout, g_ci, g_co, 1
        nb = int(lib.spk_conv_train_wgrad_ws_bytes(N, Hv, Wv, Cu, Cv, k))
        ws = torch.empty(nb, dtype=torch.uint8, device=gy.device)
        with timed("train.conv_bwd_weight"):
            check(lib.spk_conv_train_wgrad(_p(u), _p(v), _p(ws), nb, _p(gw), _p(gb), N, Hu, Wu, Cu, Hv, Wv, Cv, k, stride, pad,
                                           g_tap, g_u, g_v, bf if gb is not None else 0, st), "spk_conv_train_wgrad")
        if not needs[1]:
            gw = None
    return gi, gw, gb


class NativeConvTrainFunction(torch.autograd.Function):
    """y = conv2d / conv_transpose2d(x, weight) + bias in training, forward and backward on this library's fp32 matrix-core
    kernels (csrc/conv_train.hip): the stride-2, 1x1 and transposed layers of the spiking VQ-VAE
    (R/snn_model/vae_model.py:101-159; cuDNN in the reference).  Tensors are channels-last in memory (what the BatchNorm+LIF
    block tails produce and consume); another layout is converted."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, transposed, out_pad):
        y = conv_train_forward(x, weight, bias, stride, pad, transposed, out_pad)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (int(stride), int(pad), bool(transposed), int(out_pad), bias is not None)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        stride, pad, transposed, out_pad, has_bias = ctx.cfg
        needs = (bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1]), bool(has_bias and ctx.needs_input_grad[2]))
        return conv_train_backward(grad_y, x, weight, stride, pad, transposed, out_pad, needs) + (None,) * 4


def conv3x3_wgrad_small(grad_y, x, weight, want_bias):
    """(gw, gb) of a 3x3 / s1 / p1 convolution with <= 4 input channels from gy [N,Cout,H,W] and the dense input x [N,Cin,H,W]
    (spk_conv3x3_wgrad_small); gw comes in the memory format of ``weight`` (channels-last while training)."""
    N, Cout, H, W = (int(v) for v in grad_y.shape)
    Cin = int(x.shape[1])
    gy = grad_y if grad_y.is_contiguous(memory_format=torch.channels_last) else grad_y.contiguous(memory_format=torch.channels_last)
    xin = _dev(x.detach(), "x", torch.float32)
    cl = weight.dim() == 4 and weight.is_contiguous(memory_format=torch.channels_last) and not weight.is_contiguous()
    gw = torch.empty_like(weight, memory_format=torch.channels_last if cl else torch.contiguous_format)
    gb = torch.empty(Cout, dtype=torch.float32, device=gy.device) if want_bias else None
    nb = int(lib.spk_conv3x3_wgrad_small_ws_bytes(N, H, W, Cout, Cin))
    if nb <= 0:
        raise NotImplementedError(f"spk_conv3x3_wgrad_small: unsupported shape N={N} H={H} W={W} Cout={Cout} Cin={Cin} "
                                  "(maps of at most 64 positions, at most 4 input channels)")
    ws = torch.empty(nb, dtype=torch.uint8, device=gy.device)
    with timed("train.conv_bwd_weight"):
        check(lib.spk_conv3x3_wgrad_small(_p(gy), _p(xin), _p(ws), nb, _p(gw), _p(gb), N, H, W, Cout, Cin, int(cl), _stream(gy)),
              "spk_conv3x3_wgrad_small")
    return gw, gb


# Training forward of a stand-alone convolution: exact direct kernel up to this many multiply-accumulates per call (its fp64
# accumulation is not a matrix-core kernel), the library operator beyond.  Round 4: 4e9 -> 1e8 -- at the reference's batch of 32
# the VQ-VAE's 64 -> 32 transposed convolution (1.85e9) took 2.4 ms of a 5.4 ms training iteration in the exact kernel, the
# 16 -> 64 one (2.3e8) 0.33 ms (profiles/r4_train_vqvae.md)
EXACT_TRAIN_FORWARD_MACS = 100_000_000


def memout(x_seq, coef):
    x_seq = _dev(x_seq, "x_seq", torch.float32)
    coef = _dev(coef, "coef", torch.float32)
    T = x_seq.shape[0]
    if coef.numel() != T:
        raise RuntimeError(f"The size of tensor a ({T}) must match the size of tensor b ({coef.numel()}) at "
                           "non-singleton dimension 0")      # what torch raises for x*coef in the reference
    out = torch.empty(x_seq.shape[1:], dtype=torch.float32, device=x_seq.device)
    check(lib.spk_memout_fwd(_p(x_seq), _p(coef), _p(out), T, out.numel(), _stream(x_seq)), "spk_memout_fwd")
    return out


class MemoutFunction(torch.autograd.Function):
    """Differentiable MembraneOutputLayer (training path): forward = spk_memout_fwd, backward dL/dx[t] = dL/dout * coef[t]
    (one broadcast multiply)."""

    @staticmethod
    def forward(ctx, x_seq, coef):
        ctx.save_for_backward(coef)
        return memout(x_seq, coef)

    @staticmethod
    def backward(ctx, grad_out):
        (coef,) = ctx.saved_tensors
        return grad_out.unsqueeze(0) * coef.view((-1,) + (1,) * grad_out.dim()), None


def _dense_tn(x, name):
    """[T, ...] fp32 device tensor whose memory is T dense planes (any element order inside a plane)."""
    if not x.is_cuda:
        raise RuntimeError(f"spkdiff: {name} is on '{x.device}'; there is no CPU path")
    if x.dtype != torch.float32:
        raise NotImplementedError(f"spkdiff: {name} must be float32, got {x.dtype}")
    n = x[0].numel()
    if x.shape[0] > 1 and x.stride(0) != n:
        return x.contiguous()
    if not torch.empty_like(x).stride() == x.stride():       # not a dense permutation: copy
        return x.contiguous()
    return x


def psp(x_seq, tau_s=2.0, backward=False):
    x = _dense_tn(x_seq, "inputs")
    out = torch.empty_like(x)
    check(lib.spk_psp(_p(x), _p(out), int(x.shape[0]), x[0].numel(), float(tau_s), int(backward), _stream(x)), "spk_psp")
    return out


class PSPFunction(torch.autograd.Function):
    """syns = PSP(inputs) (R/snn_model/snn_layers.py:12-26) with its adjoint as the backward, both spk_psp."""

    @staticmethod
    def forward(ctx, x_seq, tau_s):
        ctx.tau_s = tau_s
        return psp(x_seq, tau_s, False)

    @staticmethod
    def backward(ctx, grad_out):
        return psp(grad_out, ctx.tau_s, True), None


# ---------------------------------------------------------------------------------------------- layouts
# The storage forms of a spike tensor between layers (the kernels' side of the same table: csrc/layouts.hip).  A record
# is the channels of one (position, step) that lie together in memory:
#   PTC   u8 [B,H,W,T,C]                  one byte per channel, all C of them in one record
#   CPTC  u8 [B,C/chunk,H,W,T,chunk]      the same bytes in records of `chunk` channels (32: the int8 MFMA kernel's K chunk)
#   C4    int8 [B,C/64,H,W,T,32]          e2m1 nibbles (a spike = 0x2, even channel = low nibble), 64 channels per 32-byte record
#   S32   int8 [B,C/32,H,W,T,16]          the same nibbles, 32 channels per 16-byte record (fp6v2 and the VQ-VAE's fp6 kernel)
# The nibble records carry dtype int8 so that they cannot be mistaken for the u8 CPTC of the same shape.
C4_DTYPE = torch.int8
CHUNK_C4, CHUNK_S32 = _C["SPK_CHUNK_C4"], _C["SPK_CHUNK_S32"]      # chunk_out values of spk_conv_fused_fwd


class SpikeLayout(NamedTuple):
    name: str
    dtype: torch.dtype
    rec_channels: int        # channels per record (PTC: 0 = all C of the tensor)
    rec_bytes: int           # bytes per record (PTC: 0 = C)
    chunk: int               # the C-ABI's `chunk` / `chunk_out` argument that names this layout


PTC = SpikeLayout("PTC", torch.uint8, 0, 0, 0)
C4 = SpikeLayout("C4", C4_DTYPE, 64, 32, CHUNK_C4)
S32 = SpikeLayout("S32", C4_DTYPE, 32, 16, CHUNK_S32)


def cptc(chunk):
    """The CPTC layout with records of ``chunk`` channels."""
    return SpikeLayout("CPTC", torch.uint8, int(chunk), int(chunk), int(chunk))


LAYOUTS = (PTC, cptc(32), C4, S32)      # (CPTC at the int8 MFMA kernel's chunk; cptc(n) for another)


def layout_of(t):
    """(layout, (B, C, H, W, T)) of a stored spike tensor: the place that tells the four layouts apart, by dtype, rank and record
    size (PTC, cptc(chunk), C4 or S32; compare by ``.name``).  Any device."""
    if t.dtype == torch.uint8 and t.dim() == 5:
        B, H, W, T, C = (int(v) for v in t.shape)
        return PTC, (B, C, H, W, T)
    if t.dtype == torch.uint8 and t.dim() == 6:
        B, nrec, H, W, T, chunk = (int(v) for v in t.shape)
        return cptc(chunk), (B, nrec * chunk, H, W, T)
    if t.dtype == C4_DTYPE and t.dim() == 6:
        B, nrec, H, W, T, rb = (int(v) for v in t.shape)
        for lay in (S32, C4):
            if rb == lay.rec_bytes:
                return lay, (B, nrec * lay.rec_channels, H, W, T)
    if t.dtype not in (torch.uint8, C4_DTYPE):
        raise NotImplementedError(f"spkdiff: stored spikes are torch.uint8 (PTC / CPTC) or int8-tagged C4 / S32 records, got {t.dtype}")
    raise ValueError(f"spkdiff: a {t.dtype} tensor of shape {tuple(t.shape)} is none of the spike layouts (PTC [B,H,W,T,C], CPTC "
                     "[B,C/chunk,H,W,T,chunk], C4 [B,C/64,H,W,T,32], S32 [B,C/32,H,W,T,16])")


def empty_spikes(layout, B, C, H, W, T, device):
    """Uninitialised spike tensor of C channels in ``layout`` (PTC, cptc(chunk), C4, S32): the one place that spells a record shape.
    ceil(C / record) records: the channels of a partly filled last record belong to whoever writes the tensor."""
    if layout.name == "PTC":
        shape = (B, H, W, T, C)
    else:
        shape = (B, (C + layout.rec_channels - 1) // layout.rec_channels, H, W, T, layout.rec_bytes)
    return torch.empty(shape, dtype=layout.dtype, device=device)


def spikes_to_layout(s, layout):
    """fp32 [T,B,C,H,W] -> the same spikes stored in ``layout`` (PTC, cptc(chunk), C4, S32)."""
    s = _dev(s, "spikes", torch.float32)
    T, B, C, H, W = s.shape
    o = empty_spikes(layout, B, C, H, W, T, s.device)
    if layout.dtype == torch.uint8:
        check(lib.spk_spikes_to_ptc(_p(s), _p(o), T, B, C, H * W, layout.rec_channels or C, _stream(s)), "spk_spikes_to_ptc")
    elif layout.name == "C4":
        check(lib.spk_spikes_to_fp4(_p(s), _p(o), T, B, C, H * W, _stream(s)), "spk_spikes_to_fp4")
    else:
        check(lib.spk_spikes_to_s32(_p(s), _p(o), T, B, C, H * W, _stream(s)), "spk_spikes_to_s32")
    return o


def layout_to_spikes(q, expect=None):
    """A stored spike tensor of any of the four layouts (``expect``: of that one) -> fp32 [T,B,C,H,W]."""
    q = _dev(q, "stored spikes" if expect is None else expect.name)
    lay, (B, C, H, W, T) = layout_of(q)
    if expect is not None and lay.name != expect.name:
        raise NotImplementedError(f"spkdiff: {expect.name} spikes expected, got {lay.name} ({q.dtype} {tuple(q.shape)})")
    o = torch.empty((T, B, C, H, W), dtype=torch.float32, device=q.device)
    if lay.dtype == torch.uint8:
        check(lib.spk_ptc_to_spikes(_p(q), _p(o), T, B, C, H * W, lay.rec_channels or C, _stream(q)), "spk_ptc_to_spikes")
    elif lay.name == "C4":
        check(lib.spk_fp4_to_spikes(_p(q), _p(o), T, B, C, H * W, _stream(q)), "spk_fp4_to_spikes")
    else:
        check(lib.spk_s32_to_spikes(_p(q), _p(o), T, B, C, H * W, _stream(q)), "spk_s32_to_spikes")
    return o


# The names the layers, tests and tools call: fp32 [T,B,C,H,W] <-> u8 [B,H,W,T,C] (plain PTC) or, with ``chunk``, CPTC
# [B,C/chunk,H,W,T,chunk]; <-> C4 [B,C/64,H,W,T,32]; <-> S32 [B,C/32,H,W,T,16].  ptc_to_spikes decodes any of the four.
def spikes_to_ptc(s, chunk=None):
    return spikes_to_layout(s, PTC if chunk is None else cptc(chunk))


def ptc_to_spikes(p):
    return layout_to_spikes(p)


def spikes_to_c4(s):
    return spikes_to_layout(s, C4)


def c4_to_spikes(q):
    return layout_to_spikes(q, C4)


def spikes_to_s32(s):
    return spikes_to_layout(s, S32)


def s32_to_spikes(q):
    return layout_to_spikes(q, S32)


def count_spikes(t: torch.Tensor):
    """Spike statistics of a tensor in any storage format of this library, counted on the device (spk_count_spikes):
    dict(total, t0, numel, numel_t0, binary).  fp32 [T, ...] (the reference interface; ``binary`` = every nonzero entry is
    exactly 1.0), u8 PTC [B,H,W,T,C] / CPTC [B,C/ch,H,W,T,ch], int8-tagged C4 / S32 [B,C/rec_ch,H,W,T,rec].
    ``numel`` is the tensor's CAPACITY: for C4 / S32 it counts record slots (64 / 32 per record), not channels that a layer
    drives -- the S32 spikes of a 16-channel spike generator report 32 slots per (position, step), half of them never set, so
    ``total / numel`` there is half the generator's firing rate.  Divide by the channel count you know, not by ``numel``, when
    a record is partly filled.  -0.0 is no spike in an fp32 tensor; NaN and denormals are (and make ``binary`` False)."""
    if not t.is_cuda:
        raise RuntimeError(f"spkdiff: tensor on '{t.device}'; there is no CPU path")
    t = t if t.is_contiguous() else t.contiguous()
    out = torch.empty(3, dtype=torch.int64, device=t.device)
    if t.dtype == torch.float32:
        T = int(t.shape[0])
        n = t.numel()
        inner, kind, numel = n // T, 2, n
    else:
        lay, (_, C, _, _, T) = layout_of(t)
        rec = lay.rec_bytes or C
        if rec % 4:
            raise NotImplementedError("count_spikes: PTC records must be a multiple of 4 bytes")
        nibbles = lay.dtype == C4_DTYPE                          # spk_count_spikes' kind 1: two channels per byte
        n, inner, kind, numel = t.numel() // 4, rec // 4, int(nibbles), t.numel() * (2 if nibbles else 1)
    check(lib.spk_count_spikes(_p(t), n, inner, T, kind, _p(out), _stream(t)), "spk_count_spikes")
    tot, t0, ones = (int(v) for v in out.tolist())
    return {"total": tot, "t0": t0, "numel": numel, "numel_t0": numel // T, "binary": kind != 2 or tot == ones}


# ---------------------------------------------------------------------------------------------- fused conv
def pack_conv_weight(w, transposed):
    w = _dev(w.detach(), "weight", torch.float32)
    if transposed:
        Cin, Cout, k, k2 = w.shape
    else:
        Cout, Cin, k, k2 = w.shape
    if k != k2:
        raise NotImplementedError("square kernels only")
    out = torch.empty((k * k, Cin, Cout), dtype=torch.float32, device=w.device)
    check(lib.spk_pack_conv_weight(_p(w), _p(out), Cout, Cin, k, int(transposed), _stream(w)), "spk_pack_conv_weight")
    return out


IN_PTC, IN_TINV, IN_SEQ = (_C["SPK_IN_" + n] for n in ("PTC", "TINV", "SEQ"))
STEP_TAIL_MAX_K = _C["SPK_STEP_TAIL_MAX_K"]   # classes the fused reverse-step tail takes (four 16-channel groups per wave)
VQ_TRAIN_MAX_D = _C["SPK_VQ_TRAIN_MAX_D"]     # the fused VQ training operators keep one code vector per thread


def conv_fused(in0, w_packed, bias, *, in_kind, T, mode, k, stride, pad, transposed=False, out_pad=0, in1=None,
               bn_a=None, bn_b=None, v=None, want_ptc=False, want_f32=False, want_pre=False, want_u8=False,
               coef=None, apply_tanh=False, out_ptc=None, out_f32=None, chunk_out=None, want_counts=False):
    """Launch spk_conv_fused_fwd. Returns dict(ptc=, f32=, pre=, u8=).

    in_kind IN_PTC: in0 u8 [B,H,W,T,C0] (+ in1 [B,H,W,T,C1]);  IN_TINV: in0 fp32 [B,C0,H,W];
    IN_SEQ: in0 fp32 [T,B,C0,H,W] (any values)."""
    dev = in0.device
    chunk0 = chunk1 = 0
    if in_kind == IN_PTC:
        in0 = _dev(in0, "in0", torch.uint8)
        lay0, (B, C0, H, W, T_in) = layout_of(in0)
        chunk0 = lay0.chunk
        if T_in != T:
            raise ValueError("T mismatch")
    elif in_kind == IN_TINV:
        in0 = _dev(in0, "in0", torch.float32)
        B, C0, H, W = in0.shape
    else:
        in0 = _dev(in0, "in0", torch.float32)
        T_in, B, C0, H, W = in0.shape
        if T_in != T:
            raise ValueError("T mismatch")
    if T > MAX_T:
        raise NotImplementedError(f"fused kernels keep T <= {MAX_T} steps in registers, got T={T}")
    C1 = 0
    if in1 is not None:
        in1 = _dev(in1, "in1", torch.uint8)
        lay1, (_, C1, _, _, _) = layout_of(in1)
        chunk1 = lay1.chunk
    kk, Cin, Cout = w_packed.shape
    if Cin != C0 + C1 or kk != k * k:
        raise ValueError(f"packed weight {tuple(w_packed.shape)} does not match Cin={C0 + C1}, k={k}")
    Ho, Wo = conv_out_size(H, k, stride, pad, transposed, out_pad), conv_out_size(W, k, stride, pad, transposed, out_pad)
    res = {"ptc": None, "f32": None, "pre": None, "u8": None, "cnt": None}
    if mode == MODE_LIF:
        if want_counts:
            res["cnt"] = torch.empty((B, Cout // 32, Ho, Wo, 32), dtype=torch.uint8, device=dev)
        if want_ptc:
            lay = C4 if chunk_out == C4.chunk else S32 if chunk_out == S32.chunk else cptc(chunk_out) if chunk_out else PTC
            given = out_ptc if lay.dtype == torch.uint8 else None
            res["ptc"] = given if given is not None else empty_spikes(lay, B, Cout, Ho, Wo, T, dev)
        if want_f32:
            res["f32"] = out_f32 if out_f32 is not None else torch.empty((T, B, Cout, Ho, Wo), dtype=torch.float32, device=dev)
        if want_pre:
            shape = (B, Cout, Ho, Wo) if in_kind == IN_TINV else (T, B, Cout, Ho, Wo)
            res["pre"] = torch.empty(shape, dtype=torch.float32, device=dev)
    elif mode == MODE_RAW:
        res["f32"] = out_f32 if out_f32 is not None else torch.empty((T, B, Cout, Ho, Wo), dtype=torch.float32, device=dev)
    else:
        res["f32"] = out_f32 if out_f32 is not None else torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=dev)
        if want_u8:
            res["u8"] = torch.empty((B, Cout, Ho, Wo), dtype=torch.uint8, device=dev)
    if v is not None:
        v = _dev(v, "v", torch.float32)
        if v.numel() != B * Cout * Ho * Wo:
            raise ValueError("membrane potential tensor has the wrong size")
    check(lib.spk_conv_fused_fwd(
        _p(in0), _p(in1), C0, C1, in_kind, _p(w_packed), _p(bias), _p(bn_a), _p(bn_b), _p(v), _p(res["ptc"]),
        _p(res["f32"]), _p(res["pre"]), _p(res["u8"]), _p(coef), int(apply_tanh), mode, T, B, H, W, Cout, k, stride,
        pad, int(transposed), out_pad, chunk0, chunk1, chunk_out or 0, _p(res["cnt"]), _n_dyn(), _stream(in0)),
        "spk_conv_fused_fwd")
    return res


# ---------------------------------------------------------------------------------------------- MFMA denoiser convs
# Which shapes a kernel family takes is answered by the library (spk_*_supported / spk_vae_fp6_kind: host functions its entry points
# call themselves); what is added to an answer here is policy -- which of the supported shapes this package sends there.
def den_mfma_supported(Cout, Cin, k, stride, pad, T, H, W):
    return bool(lib.spk_den_conv3x3_mfma_supported(Cout, Cin, k, stride, pad, T, H, W))


def _pack_weight(w, bias, nbytes, n_scale, plane_dtype, pack, what, unsupported, extra=()):
    """The part every weight packer shares.  w: the fp32 weight on its device; nbytes: the library's size answer for the digit
    planes (negative / zero: NotImplementedError(unsupported)); n_scale: entries of the fp64 scale and bias vectors; extra:
    (shape, dtype) of further outputs.  pack(w, bias, planes, scale, bias_d, *extra outputs) makes the library call.
    Returns (planes, scale, bias_d, *extra outputs)."""
    if nbytes <= 0:
        raise NotImplementedError(unsupported)
    wq = torch.empty(nbytes, dtype=plane_dtype, device=w.device)
    scale = torch.empty(n_scale, dtype=torch.float64, device=w.device)
    bias_d = torch.empty(n_scale, dtype=torch.float64, device=w.device)
    more = tuple(torch.empty(shape, dtype=dtype, device=w.device) for shape, dtype in extra)
    b = None if bias is None else _dev(bias.detach(), "bias", torch.float32)
    check(pack(_p(w), _p(b), _p(wq), _p(scale), _p(bias_d), *(_p(t) for t in more)), what)
    return (wq, scale, bias_d) + more


def den_pack_weight_i8(w, bias, pad_cout=False):
    """[Cout,Cin,3,3] fp32 -> (int8 digit planes, fp64 scale [Cout], fp64 bias [Cout]).  pad_cout: output channels are
    zero-padded to the next multiple of 16 first (the logits layer for any --codebook_size, R/main.py:58: the kernels that read
    these planes take 16-channel column groups; scale / bias then have ceil16(Cout) entries, the extra ones are never read back)."""
    w = _dev(w.detach(), "weight", torch.float32)
    Cout, Cin = w.shape[0], w.shape[1]
    if pad_cout and Cout % 16:
        kp = (Cout + 15) // 16 * 16
        w = torch.cat([w, w.new_zeros((kp - Cout,) + tuple(w.shape[1:]))], 0).contiguous()
        if bias is not None:
            bias = torch.cat([bias.detach(), bias.detach().new_zeros(kp - Cout)], 0)
        Cout = kp
    return _pack_weight(w, bias, lib.spk_den_packed_weight_bytes(Cout, Cin), Cout, torch.int8,
                        lambda *t: lib.spk_den_pack_weight_i8(*t, Cout, Cin, _stream(w)), "spk_den_pack_weight_i8",
                        "spkdiff: MFMA conv needs Cout % 16 == 0 and Cin % 32 == 0")


def den_conv3x3_mfma(in0, packed, Cout, *, mode, in1=None, bn_a=None, bn_b=None, v=None, out=None, want_counts=False):
    """in0/in1: CPTC u8 [B, C/32, H, W, 16, 32]. mode LIF -> CPTC spikes [B, Cout/32, H, W, 16, 32]
    (or (spikes, counts u8 [B, Cout/32, H, W, 32]) with want_counts); mode MEAN -> fp32 [B, Cout, H, W]."""
    in0 = _dev(in0, "in0", torch.uint8)
    B, nch0, H, W, T, chunk = in0.shape
    if chunk != 32:
        raise ValueError("MFMA conv reads 32-channel chunked spikes")
    nch1 = 0
    if in1 is not None:
        in1 = _dev(in1, "in1", torch.uint8)
        nch1 = in1.shape[1]
    wq, scale, bias_d = packed
    out_c = out_f = None
    if mode == MODE_LIF:
        out_c = out if out is not None else empty_spikes(cptc(32), B, Cout, H, W, T, in0.device)
    else:
        out_f = out if out is not None else torch.empty((B, Cout, H, W), dtype=torch.float32, device=in0.device)
    cnt = None
    if want_counts and mode == MODE_LIF:
        cnt = torch.empty((B, Cout // 32, H, W, 32), dtype=torch.uint8, device=in0.device)
    check(lib.spk_den_conv3x3_mfma(_p(in0), nch0, _p(in1), nch1, _p(wq), _p(scale), _p(bias_d), _p(bn_a), _p(bn_b),
                                   _p(v), _p(out_c), _p(cnt), _p(out_f), mode, T, B, H, W, Cout, _n_dyn(),
                                   _stream(in0)), "spk_den_conv3x3_mfma")
    if mode == MODE_LIF:
        return (out_c, cnt) if want_counts else out_c
    return out_f


def den_conv3x3_counts(cnt0, packed, Cout, T, cnt1=None):
    """Time-collapsed conv6: cnt0/cnt1 u8 spike counts [B, C/32, H, W, 32] -> logits fp32 [B, Cout, H, W].  ``packed`` may hold
    more (zero-padded) output channels than Cout (den_pack_weight_i8(pad_cout=True)): the kernel computes all of them and the
    first Cout are returned."""
    cnt0 = _dev(cnt0, "cnt0", torch.uint8)
    B, nch0, H, W, ck = cnt0.shape
    if ck != 32:
        raise ValueError("counts are 32-channel chunked")
    nch1 = 0
    if cnt1 is not None:
        cnt1 = _dev(cnt1, "cnt1", torch.uint8)
        nch1 = cnt1.shape[1]
    wq, scale, bias_d = packed
    kp = int(scale.numel())
    if kp < Cout or kp - Cout >= 16:
        raise ValueError("packed logits weights do not belong to a layer of Cout output channels")
    out = torch.empty((B, kp, H, W), dtype=torch.float32, device=cnt0.device)
    check(lib.spk_den_conv3x3_counts_mfma(_p(cnt0), nch0, _p(cnt1), nch1, _p(wq), _p(scale), _p(bias_d), _p(out), T, B,
                                          H, W, kp, _n_dyn(), _stream(cnt0)), "spk_den_conv3x3_counts_mfma")
    return out if kp == Cout else out[:, :Cout].contiguous()


# ------------------------------------------------------------------------------- fp6/fp4 block-scaled MFMA denoiser convs
def den_fp6_supported(Cout, Cin, k, stride, pad, T, H, W):
    return bool(lib.spk_den_conv3x3_mfma_fp6_supported(Cout, Cin, k, stride, pad, T, H, W))


def den_pack_weight_fp6(w, bias):
    """[Cout,Cin,3,3] fp32 -> (e2m3 digit planes u8, fp64 scale [Cout], fp64 bias [Cout])."""
    wd = w.detach()
    # a channels-last weight (the training path's parameter format) is packed as stored: no layout copy per layer and iteration
    cl = (wd.is_cuda and wd.dtype == torch.float32 and wd.dim() == 4 and tuple(wd.shape[2:]) == (3, 3) and not wd.is_contiguous()
          and wd.is_contiguous(memory_format=torch.channels_last))
    w = wd if cl else _dev(wd, "weight", torch.float32)
    Cout, Cin = w.shape[0], w.shape[1]
    pack = lib.spk_den_pack_weight_fp6_cl if cl else lib.spk_den_pack_weight_fp6
    return _pack_weight(w, bias, lib.spk_den_packed_weight_fp6_bytes(Cout, Cin), Cout, torch.uint8,
                        lambda *t: pack(*t, Cout, Cin, _stream(w)), "spk_den_pack_weight_fp6",
                        "spkdiff: fp6 MFMA conv needs Cout % 16 == 0 and Cin % 64 == 0")


def den_conv3x3_mfma_fp6(in0, packed, Cout, *, bn_a, bn_b, v=None, want_counts=False):
    """in0: C4 spikes [B, C/64, H, W, 16, 32] (int8-tagged). Returns C4 spikes [B, Cout/64, H, W, 16, 32]
    (or (spikes, counts u8 [B, Cout/32, H, W, 32]) with want_counts)."""
    in0 = _dev(in0, "in0", C4_DTYPE)
    B, nch, H, W, T, rec = in0.shape
    if rec != 32:
        raise ValueError("C4 spike records are 32 bytes (64 channels)")
    wq, scale, bias_d = packed
    out = empty_spikes(C4, B, Cout, H, W, T, in0.device)
    cnt = torch.empty((B, Cout // 32, H, W, 32), dtype=torch.uint8, device=in0.device) if want_counts else None
    check(lib.spk_den_conv3x3_mfma_fp6(_p(in0), nch, _p(wq), _p(scale), _p(bias_d), _p(bn_a), _p(bn_b), _p(v), _p(out),
                                       _p(cnt), T, B, H, W, Cout, _n_dyn(), _stream(in0)), "spk_den_conv3x3_mfma_fp6")
    return (out, cnt) if want_counts else out


def spikes_cl_to_c4(s):
    """fp32 spikes [T,B,C,H,W] with channels-last memory -> C4 [B, C/64, H, W, T, 32]."""
    s = _cl5(s, "spikes")
    T, B, C, H, W = s.shape
    o = empty_spikes(C4, B, C, H, W, T, s.device)
    check(lib.spk_spikes_nhwc_to_fp4(_p(s), _p(o), T, B, C, H * W, _stream(s)), "spk_spikes_nhwc_to_fp4")
    return o


def spikes_cl_to_c4_counts(s):
    """spikes_cl_to_c4 + the spike counts over T, fp32 [B,C,H,W] (channels-last memory), from the same pass."""
    s = _cl5(s, "spikes")
    T, B, C, H, W = s.shape
    o = empty_spikes(C4, B, C, H, W, T, s.device)
    cnt = _empty_cl((B, C, H, W), s.device)
    check(lib.spk_spikes_nhwc_to_fp4_counts(_p(s), _p(o), _p(cnt), T, B, C, H * W, _stream(s)), "spk_spikes_nhwc_to_fp4_counts")
    return o, cnt


def den_conv3x3_fp6_raw(in0, packed, Cout):
    """in0: C4 spikes [B, C/64, H, W, 16, 32] -> exact pre-activations fp32 [T,B,Cout,H,W], channels-last memory."""
    in0 = _dev(in0, "in0", C4_DTYPE)
    B, nch, H, W, T, rec = in0.shape
    wq, scale, bias_d = packed
    y = _empty_cl((T, B, Cout, H, W), in0.device)
    check(lib.spk_den_conv3x3_fp6_raw(_p(in0), nch, _p(wq), _p(scale), _p(bias_d), _p(y), T, B, H, W, Cout, _stream(in0)),
          "spk_den_conv3x3_fp6_raw")
    return y


def conv3x3_wgrad_supported(Cout, Cin, H, W):
    return bool(lib.spk_conv3x3_wgrad_supported(Cout, Cin, H, W))


# False: the weight gradient of the spike-input convolutions comes from the framework's operator (as in rounds 1-2)
NATIVE_WGRAD = True


def conv3x3_wgrad(gy_cl, spikes_cl, Cout, Cin, want_bias=False):
    """gw [Cout,Cin,3,3] (channels-last memory) of a 3x3 / s1 / p1 convolution from gy [N,Cout,H,W] and an operand [N,Cin,H,W]
    whose values are exact in bf16 -- binary spikes, or integers up to 256 such as the spike counts the time-collapsed last layer
    passes (the kernel truncates the operand to bf16) -- on 7x7 or 8x8 maps, both channels-last fp32 (spk_conv3x3_wgrad_bf16: bf16
    matrix cores, exact three-term split of gy)."""
    N, H, W = int(gy_cl.shape[0]), int(gy_cl.shape[2]), int(gy_cl.shape[3])
    nb = int(lib.spk_conv3x3_wgrad_ws_bytes(N, int(Cout), int(Cin)))
    if nb <= 0:
        raise NotImplementedError("spk_conv3x3_wgrad_bf16: unsupported shape")
    ws = torch.empty(nb // 4, dtype=torch.float32, device=gy_cl.device)
    gw = torch.empty((Cout, 3, 3, Cin), dtype=torch.float32, device=gy_cl.device)
    gb = torch.empty(Cout, dtype=torch.float32, device=gy_cl.device) if want_bias else None
    with timed("train.conv_wrw"):
        check(lib.spk_conv3x3_wgrad_bf16(_p(gy_cl), _p(spikes_cl), _p(ws), nb, _p(gw), _p(gb), N, H, W, int(Cout), int(Cin),
                                         _stream(gy_cl)), "spk_conv3x3_wgrad_bf16")
    return (gw.permute(0, 3, 1, 2), gb) if want_bias else gw.permute(0, 3, 1, 2)


def conv3x3_dgrad_supported(Cout, Cin, H, W, N):
    # policy (small layers and small batches: the framework's operator is as fast)
    return bool(lib.spk_conv3x3_dgrad_supported(Cout, Cin, H, W, N)) and Cout * Cin >= 8192 and N >= 64


# False: the data gradient of the spike-input convolutions comes from the framework's operator (as in rounds 1-2)
NATIVE_DGRAD = True


# "bf16x3": three bf16 terms per operand, six products (exact splits); "f16x2": two scaled fp16 terms, three products
DGRAD_FORM = "f16x2"


class WeightPrep:
    """What one optimizer step's worth of a spike-input convolution's weight is turned into ONCE per training iteration by
    ``train_weight_prep``: ``fp6`` = (digit planes, scale, bias) of the exact MFMA forward, ``dg`` = (workspace, bytes, N) of the
    two-term fp16 data gradient, or None where that layer's backward does not take it."""
    __slots__ = ("fp6", "dg", "key")

    def __init__(self, fp6, dg, key):
        self.fp6, self.dg, self.key = fp6, dg, key

    def matches(self, weight):
        return self.key == (weight.data_ptr(), weight._version, tuple(weight.shape))


def _ptr_array(ctype, values):
    return (ctype * len(values))(*values)


def train_weight_prep(layers):
    """layers: [(weight [Cout,Cin,3,3] channels-last fp32 parameter, bias or None, N_dgrad, (H, W))], at most eight.  TWO launches
    for all of them -- spk_den_pack_weight_fp6_cl_multi and spk_conv3x3_dgrad_f16x2_pack_multi -- instead of one fp6 pack per
    layer in the forward and a fill + maximum + pack per layer in the backward (20 launches, ~130 us of a 2.0 ms iteration at the
    reference's batch).  N_dgrad: the image count that layer's data gradient will be called with (T * B; B for the collapsed last
    layer; 0: that layer's backward does not take the native two-term data gradient).  Returns one WeightPrep per layer, or None when a layer does not fit (callers then pack per
    layer as before)."""
    import ctypes
    if not layers or len(layers) > 8:
        return None
    dev = layers[0][0].device
    for w, b, n_dg, hw in layers:
        if not (w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3)
                and w.is_contiguous(memory_format=torch.channels_last) and w.shape[0] % 16 == 0 and w.shape[1] % 64 == 0):
            return None
    n = len(layers)
    wd = [w.detach() for w, _, _, _ in layers]
    couts, cins = [int(w.shape[0]) for w in wd], [int(w.shape[1]) for w in wd]
    wq = [torch.empty(int(lib.spk_den_packed_weight_fp6_bytes(co, ci)), dtype=torch.uint8, device=dev) for co, ci in zip(couts, cins)]
    scale = [torch.empty(co, dtype=torch.float64, device=dev) for co in couts]
    bias_d = [torch.empty(co, dtype=torch.float64, device=dev) for co in couts]
    bs = [None if b is None else _dev(b.detach(), "bias", torch.float32) for _, b, _, _ in layers]
    vp = ctypes.c_void_p
    ia = lambda v: _ptr_array(ctypes.c_int, [int(x) for x in v])
    pa = lambda ts: _ptr_array(vp, [None if t is None else t.data_ptr() for t in ts])
    check(lib.spk_den_pack_weight_fp6_cl_multi(pa(wd), pa(bs), pa(wq), pa(scale), pa(bias_d), ia(couts), ia(cins), n, _stream(wd[0])),
          "spk_den_pack_weight_fp6_cl_multi")
    dg = [None] * n
    sel = [i for i, (w, _, n_dg, hw) in enumerate(layers)
           if NATIVE_DGRAD and DGRAD_FORM == "f16x2" and n_dg > 0 and tuple(hw) in ((7, 7), (8, 8))
           and n_dg * hw[0] * hw[1] * couts[i] < 2 ** 31]
    if sel:
        nbs = [int(lib.spk_conv3x3_dgrad_ws_bytes(couts[i], cins[i])) for i in sel]
        wss = [torch.empty(nb, dtype=torch.uint8, device=dev) for nb in nbs]
        check(lib.spk_conv3x3_dgrad_f16x2_pack_multi(pa([wd[i] for i in sel]), pa(wss), _ptr_array(ctypes.c_longlong, nbs),
                                                     ia([layers[i][2] for i in sel]), ia([couts[i] for i in sel]),
                                                     ia([cins[i] for i in sel]), len(sel), _stream(wd[0])),
              "spk_conv3x3_dgrad_f16x2_pack_multi")
        for i, ws, nb in zip(sel, wss, nbs):
            dg[i] = (ws, nb, int(layers[i][2]))
    return [WeightPrep((wq[i], scale[i], bias_d[i]), dg[i], (layers[i][0].data_ptr(), layers[i][0]._version, tuple(wd[i].shape)))
            for i in range(n)]


def conv3x3_dgrad(gy_cl, weight, Cin, form=None, prep=None):
    """gi [N,Cin,H,W] (channels-last memory) of a 3x3 / s1 / p1 convolution from gy [N,Cout,H,W] (channels-last fp32; 7x7 or
    8x8 maps) and the weight [Cout,Cin,3,3]: spk_conv3x3_dgrad_f16x2 (two scaled fp16 terms per operand, three products) or
    spk_conv3x3_dgrad_bf16 (three exact bf16 terms, six products).  Both measure 2-4e-7 relative L2 against fp64 on the training
    shapes (an fp32 operator: 2-6e-7).  Per ELEMENT they differ: the bf16 form splits every value exactly, whatever its
    magnitude; the fp16 form scales each image's gy / each input channel's weights by one power of two and keeps fp32-like
    relative precision only within ~17 binades of that set's maximum (below: an absolute 2^-40 of the maximum) -- choose
    ``form='bf16x3'`` where a gradient map's magnitudes span more than that inside one image."""
    N, Cout, H, W = int(gy_cl.shape[0]), int(gy_cl.shape[1]), int(gy_cl.shape[2]), int(gy_cl.shape[3])
    nb = int(lib.spk_conv3x3_dgrad_ws_bytes(Cout, int(Cin)))
    if nb <= 0:
        raise NotImplementedError("spk_conv3x3_dgrad_bf16: unsupported shape")
    form = form or DGRAD_FORM
    gi = torch.empty((N, H, W, Cin), dtype=torch.float32, device=gy_cl.device)
    if prep is not None and prep.dg is not None and form == "f16x2" and prep.dg[2] == N and prep.matches(weight):
        # the weight half was packed with the other layers' at the start of the iteration (train_weight_prep)
        with timed("train.conv_bwd_data"):
            check(lib.spk_conv3x3_dgrad_f16x2_prepacked(_p(gy_cl), _p(prep.dg[0]), prep.dg[1], _p(gi), N, H, W, Cout, int(Cin),
                                                        _stream(gy_cl)), "spk_conv3x3_dgrad_f16x2_prepacked")
        return gi.permute(0, 3, 1, 2)
    w_cl = weight.detach().contiguous(memory_format=torch.channels_last)        # storage [Cout][3][3][Cin]
    ws = torch.empty(nb, dtype=torch.uint8, device=gy_cl.device)
    fn, name = ((lib.spk_conv3x3_dgrad_f16x2, "spk_conv3x3_dgrad_f16x2") if form == "f16x2"
                else (lib.spk_conv3x3_dgrad_bf16, "spk_conv3x3_dgrad_bf16"))
    with timed("train.conv_bwd_data"):
        check(fn(_p(gy_cl), _p(w_cl), _p(ws), nb, _p(gi), N, H, W, Cout, int(Cin), _stream(gy_cl)), name)
    return gi.permute(0, 3, 1, 2)


class SpikeConvTrainFunction(torch.autograd.Function):
    """y = conv3x3(spikes, weight) + bias for BINARY input spikes in training: the forward is the exact
    fp6 x fp4 MFMA convolution (weights re-packed into six radix-32 digit planes each call -- they change every optimizer
    step -- spikes packed to C4); the backward of the 7x7 layers is native where the shape fits -- weight (+ bias) gradient
    on the bf16 MFMA with an exact three-term split of gy (spk_conv3x3_wgrad_bf16), data gradient on the fp16 MFMA with both
    operands as two scaled terms (spk_conv3x3_dgrad_f16x2; DGRAD_FORM selects the three-term bf16 form) -- and the
    framework's operator otherwise.  spikes [T,B,Cin,H,W] in {0,1}; returns channels-last [T,B,Cout,H,W]."""

    @staticmethod
    def forward(ctx, spikes, weight, bias, prep=None, c4=None):
        # prep: this layer's WeightPrep of the iteration (ops.train_weight_prep), c4: the spikes as C4 records where the producing
        # BatchNorm+LIF launch wrote them -- either spares a launch here; both are optional and checked
        s = _cl5(spikes, "spikes")
        Cout = int(weight.shape[0])
        if prep is not None and not prep.matches(weight):
            prep = None
        T, B, C, H, W = (int(v) for v in s.shape)
        try:
            if c4 is not None and (c4.device != s.device or layout_of(c4) != (C4, (B, C, H, W, T))):
                c4 = None
        except (ValueError, NotImplementedError):               # (no spike tensor at all: dropped like any other mismatch)
            c4 = None
        with timed("train.conv_fwd_fp6"):
            y = den_conv3x3_fp6_raw(c4 if c4 is not None else spikes_cl_to_c4(s),
                                    prep.fp6 if prep is not None else den_pack_weight_fp6(weight, bias), Cout)
        ctx.save_for_backward(s, weight)
        ctx.has_bias = bias is not None
        ctx.prep = prep
        return y

    @staticmethod
    def backward(ctx, grad_y):
        s, weight = ctx.saved_tensors
        gy = _cl5(grad_y, "grad_y").flatten(0, 1)
        s4 = s.flatten(0, 1)
        Cout, Cin = int(weight.shape[0]), int(weight.shape[1])
        need_gi, need_gw = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])
        need_gb = bool(ctx.has_bias and ctx.needs_input_grad[2])
        gw_native = None
        if (NATIVE_WGRAD and need_gw and tuple(weight.shape[2:]) == (3, 3) and
                conv3x3_wgrad_supported(Cout, Cin, int(s.shape[3]), int(s.shape[4]))):
            # the weight gradient multiplies gy by SPIKES: native on the bf16 matrix cores (the data gradient has no spike operand)
            gw_native = conv3x3_wgrad(gy, s4, Cout, Cin, want_bias=need_gb)      # (+ the bias gradient from the same pass)
            if need_gb:
                gw_native, gb_native = gw_native
            need_gw = False
        gi_native = None
        if (NATIVE_DGRAD and need_gi and tuple(weight.shape[2:]) == (3, 3) and
                conv3x3_dgrad_supported(Cout, Cin, int(s.shape[3]), int(s.shape[4]), int(gy.shape[0]))):
            gi_native = conv3x3_dgrad(gy, weight, Cin, prep=ctx.prep)
            need_gi = False
        gi = gw = gb = None
        if need_gi or need_gw or (need_gb and gw_native is None):
            gi, gw, gb = torch.ops.aten.convolution_backward(
                gy, s4, weight, [Cout], [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                [need_gi, need_gw, need_gb and gw_native is None])
        if gw_native is not None:
            gw = gw_native
            if need_gb:
                gb = gb_native
        if gi_native is not None:
            gi = gi_native
        if gi is not None:
            gi = gi.reshape(s.shape) if gi_native is None else gi.unflatten(0, (s.shape[0], s.shape[1]))
        return gi, gw, gb, None, None


class CatChannelsFunction(torch.autograd.Function):
    """cat((a, b), dim=2) of two [T,B,C,H,W] spike trains (R/snn_model/vq_diffusion.py:205).  Forward: the framework's cat, on the
    4-D views when both operands are channels-last (so that the layout survives).  Backward: two channel SLICES of the incoming
    gradient, as views -- the gradient in front of the last layer is one [B,C,H,W] tensor broadcast over T (stride 0), which the
    reshape in the framework's own backward of flatten + cat + view had to expand and copy (32 MB at B = 32) before slicing."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.ca = int(a.shape[2])
        T = int(a.shape[0])
        if a.permute(0, 1, 3, 4, 2).is_contiguous() and b.permute(0, 1, 3, 4, 2).is_contiguous():
            cat = torch.cat((a.flatten(0, 1), b.flatten(0, 1)), dim=1)
            return cat.view((T, a.shape[1]) + tuple(cat.shape[1:]))
        return torch.cat((a, b), dim=2)

    @staticmethod
    def backward(ctx, g):
        return g[:, :, :ctx.ca], g[:, :, ctx.ca:]


class SpikeConvMeanTrainFunction(torch.autograd.Function):
    """mean over T of conv3x3(spikes_t, weight) + bias -- the denoiser's last layer and its time mean
    (R/snn_model/vq_diffusion.py:185-187, 205-206) as ONE differentiable operator.  Forward: the exact fp6 x fp4 MFMA convolution
    of every step and `sum(0) / T`, the operations of the two-operator form.  Backward: every step receives the SAME output
    gradient g / T, so the weight gradient is sum_b (g_b / T) (x) COUNTS_b (counts = sum_t s_t, 0..T: exact in bf16) and the
    data gradient is one transposed convolution of g / T repeated over T -- 1/T of the matrix work of the per-step backward and
    no [T,B,Cout,H,W] gradient tensor.  spikes [T,B,Cin,H,W] in {0,1}; returns [B,Cout,H,W]."""

    @staticmethod
    def forward(ctx, spikes, weight, bias, prep=None):
        s = _cl5(spikes, "spikes")
        T, Cout = int(s.shape[0]), int(weight.shape[0])
        if prep is not None and not prep.matches(weight):
            prep = None
        with timed("train.conv_fwd_fp6"):
            c4, counts = spikes_cl_to_c4_counts(s)             # counts [B,Cin,H,W], channels-last like s: same pass as the packing
            y = den_conv3x3_fp6_raw(c4, prep.fp6 if prep is not None else den_pack_weight_fp6(weight, bias), Cout)
        ctx.save_for_backward(counts, weight)
        ctx.has_bias, ctx.T = bias is not None, T
        ctx.prep = prep
        return torch.sum(y, dim=0) / T

    @staticmethod
    def backward(ctx, grad_out):
        counts, weight = ctx.saved_tensors
        T, Cout, Cin = ctx.T, int(weight.shape[0]), int(weight.shape[1])
        B, H, W = int(counts.shape[0]), int(counts.shape[2]), int(counts.shape[3])
        g = (grad_out / T).contiguous(memory_format=torch.channels_last)     # the gradient of every step's output
        c = counts.contiguous(memory_format=torch.channels_last)
        need_gi, need_gw = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])
        need_gb = bool(ctx.has_bias and ctx.needs_input_grad[2])
        gi = gw = gb = None
        native = tuple(weight.shape[2:]) == (3, 3) and (H, W) in ((7, 7), (8, 8))
        if need_gw and native and NATIVE_WGRAD and Cout % 128 == 0 and Cin % 64 == 0:
            gw = conv3x3_wgrad(g, c, Cout, Cin)
            need_gw = False
        if need_gi and native and NATIVE_DGRAD and Cout % 16 == 0 and Cin % 32 == 0:
            gi = conv3x3_dgrad(g, weight, Cin, prep=ctx.prep)
            need_gi = False
        if need_gi or need_gw:
            gi2, gw2, _ = torch.ops.aten.convolution_backward(g, c, weight, [Cout], [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                              [need_gi, need_gw, False])
            gi = gi2 if need_gi else gi
            gw = gw2 if need_gw else gw
        if need_gb:
            gb = grad_out.sum(dim=(0, 2, 3))                   # sum over T of g / T
        if gi is not None:
            gi = gi.unsqueeze(0).expand((T,) + tuple(gi.shape))
        return gi, gw, gb, None


# ------------------------------------------------------------------------------- fp6v2: the sampler's denoiser convolutions
def den_fp6v2_supported(Cout, Cin, k, stride, pad, T, H, W):
    return bool(lib.spk_den_conv3x3_mfma_fp6v2_supported(Cout, Cin, k, stride, pad, T, H, W))


def den_pack_weight_fp6v2(w, bias):
    """[Cout,Cin,3,3] fp32 -> (digit tiles u8, fp64 scale [Cout], fp64 bias [Cout], fp32 L1 norms [Cout], the quantised
    weights as int32 [Cout, 9, Cin]: the exact recomputation of flagged neurons reads them)."""
    w = _dev(w.detach(), "weight", torch.float32)
    Cout, Cin = w.shape[0], w.shape[1]
    return _pack_weight(w, bias, lib.spk_den_packed_weight_fp6v2_bytes(Cout, Cin), Cout, torch.uint8,
                        lambda *t: lib.spk_den_pack_weight_fp6v2(*t, Cout, Cin, _stream(w)), "spk_den_pack_weight_fp6v2",
                        "spkdiff: fp6v2 MFMA conv needs Cout % 32 == 0 and Cin % 32 == 0",
                        extra=(((Cout,), torch.float32), ((Cout, 9, Cin), torch.int32)))          # wl1, qtab


# Flagged-neuron workspaces of the certified kernels (fp6v2 / vae_fp6: live counter, id list, overflow bitmap, hand-over
# ticket; zero-initialised, every call leaves them clean).  A workspace must never be shared by launches that can run
# concurrently: outside a ``flag_scope`` it is keyed by (kind, device, STREAM, words); inside one it belongs to the scope's
# owner -- a captured graph keeps its scope dict in its cache entry, so the buffers its launches address live as long as the
# graph and no eager call ever touches them.  Nothing here is ever dropped while a graph may address it.
_FLAG_DEFAULT = {}
# (thread-local: the sampler captures with capture_error_mode='thread_local' precisely so that OTHER threads may use the device
#  meanwhile -- their certified-kernel calls must keep their own per-stream workspaces, never the capturing thread's scope)
import threading as _threading
_FLAG_TLS = _threading.local()


class flag_scope:
    """``with ops.flag_scope(store):`` -- certified kernels launched inside take their flag workspaces from ``store`` (a dict
    owned by the caller: one per captured graph / call site)."""

    def __init__(self, store):
        self.store = store

    def __enter__(self):
        self.prev = getattr(_FLAG_TLS, "store", None)
        _FLAG_TLS.store = self.store
        return self.store

    def __exit__(self, *exc):
        _FLAG_TLS.store = self.prev
        return False


def _flag_ws(kind, device, words):
    store = getattr(_FLAG_TLS, "store", None)
    if store is None:
        key = (kind, str(device), int(torch.cuda.current_stream(device).cuda_stream), int(words))
        buf = _FLAG_DEFAULT.get(key)
        if buf is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("spkdiff: first use of a certified-kernel shape during hipGraph capture outside an "
                                   "ops.flag_scope (its workspace would live in the graph's pool and be shared with eager calls)")
            buf = _FLAG_DEFAULT[key] = torch.zeros(int(words), dtype=torch.int32, device=device)
        return buf
    key = (kind, str(device), int(words))
    buf = store.get(key)
    if buf is None:
        # (inside a capture the memset is captured with it: replays re-zero a buffer the kernels already left clean)
        buf = store[key] = torch.zeros(int(words), dtype=torch.int32, device=device)
    return buf


def _flag_bitmap(device, words):
    return _flag_ws("den", device, words)


# How many flagged neurons the id list of a certified-kernel call takes before the rest go to the overflow bitmap (the `flag_cap`
# argument of spk_den_conv3x3_mfma_fp6v2* / spk_vae_fp6_fwd).  -1 = the whole list (2^20 entries): every product call.  The parity
# suite sets 64 and 0 so that whole samplers / decoders run on the overflow path (tests: test_flag_overflow_*).
FLAG_CAP = -1
# `form` argument of spk_den_conv3x3_mfma_fp6v2: 0 = automatic (small batches: two half-image items per image), 1 = whole-image items
# always (tests: the split form against it)
FP6V2_FORM = 0


def den_conv3x3_mfma_fp6v2(in0, packed, Cout, *, bn_a, bn_b, want_counts=False, need_radius=None):
    """in0: S32 spikes [B, C/32, 7, 7, 16, 16] (int8-tagged). Returns S32 spikes [B, Cout/32, 7, 7, 16, 16]
    (or (spikes, counts u8 [B, Cout/32, 7, 7, 32]) with want_counts).  Fresh LIF state, none written back.
    need_radius: inside ``active_set(..., need=NeedLists)`` the layer computes only the positions listed for that radius
    (1 = the layer the logits convolution reads, 2 = the one below, ...); every other position of the result is
    unspecified."""
    in0 = _dev(in0, "in0", C4_DTYPE)
    B, nch, H, W, T, rec = in0.shape
    if rec != 16:
        raise ValueError("S32 spike records are 16 bytes (32 channels)")
    wq, scale, bias_d, wl1, qtab = packed
    out = empty_spikes(S32, B, Cout, H, W, T, in0.device)
    cnt = torch.empty((B, Cout // 32, H, W, 32), dtype=torch.uint8, device=in0.device) if want_counts else None
    flags = _flag_bitmap(in0.device, lib.spk_den_fp6v2_flag_words(B, Cout, H, W))
    if (need_radius is not None and NEED is not None and ACTIVE is not None and (H, W) == (7, 7) and
            need_radius <= NEED.radii and NEED.batch == B):
        rc = lib.spk_den_conv3x3_mfma_fp6v2_listed(_p(in0), nch, _p(wq), _p(scale), _p(bias_d), _p(wl1), _p(qtab), _p(bn_a),
                                                   _p(bn_b), _p(out), _p(cnt), _p(flags), T, B, H, W, Cout, _n_dyn(),
                                                   _p(NEED.buf), NEED.radii, int(need_radius), int(FLAG_CAP), _stream(in0))
        if rc != _C["SPK_ERR_UNSUPPORTED"]:
            check(rc, "spk_den_conv3x3_mfma_fp6v2_listed")
            return (out, cnt) if want_counts else out
        # SPK_ERR_UNSUPPORTED: this device / partition has too few CUs for the per-class division of the listed launch (e.g.
        # a 32-CU partition with Cout = 512).  The unlisted launch computes a superset of the listed positions: same tokens.
    check(lib.spk_den_conv3x3_mfma_fp6v2(_p(in0), nch, _p(wq), _p(scale), _p(bias_d), _p(wl1), _p(qtab), _p(bn_a), _p(bn_b),
                                         _p(out), _p(cnt), _p(flags), T, B, H, W, Cout, _n_dyn(), int(FLAG_CAP), int(FP6V2_FORM),
                                         _stream(in0)),
          "spk_den_conv3x3_mfma_fp6v2")
    if FP6V2_STATS is not None:
        _fp6v2_stats(in0, packed, Cout, bn_a, bn_b, out, cnt, flags)
    return (out, cnt) if want_counts else out


# bench.py's instrumented pass sets this to a list: every fp6v2 layer call then appends (Cout, Cin, flagged neurons,
# neurons, repair ms, last-position ms) -- the tail parts re-run and timed on their own (spk_den_conv3x3_mfma_fp6v2_part)
FP6V2_STATS = None


def _fp6v2_stats(in0, packed, Cout, bn_a, bn_b, out, cnt, flags):
    B, nch, H, W, T, _ = in0.shape
    wq, scale, bias_d, wl1, qtab = packed
    ms = {}
    for part in (2, 4):
        if part == 4 and (H * W) % 2 == 0:
            ms[part] = 0.0
            continue
        evs = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(lib.spk_den_conv3x3_mfma_fp6v2_part(_p(in0), nch, _p(wq), _p(scale), _p(bias_d), _p(wl1), _p(qtab), _p(bn_a),
                                                      _p(bn_b), _p(out), _p(cnt), _p(flags), T, B, H, W, Cout, _n_dyn(), part,
                                                      int(FLAG_CAP), _stream(in0)), "spk_den_conv3x3_mfma_fp6v2_part")
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ms[part] = sorted(a.elapsed_time(b) for a, b in evs)[1]
    FP6V2_STATS.append({"Cout": int(Cout), "Cin": int(nch * 32), "flagged": int(flags[1].item()),
                        "neurons": int(B * Cout * H * W), "repair_ms": ms[2], "last_position_ms": ms[4]})


# ---------------------------------------------------------------------------------------------- MFMA VQ-VAE layers
def conv_mfma_supported(Cin, Cout, T, mode):
    # policy: a spiking layer goes there only with whole 16-channel groups of output (the kernel itself pads any Cout)
    return bool(lib.spk_conv_mfma_fused_supported(Cin, Cout, T, mode)) and (mode == MODE_MEMOUT or Cout % 16 == 0)


def pack_conv_weight_i8(w, bias, transposed):
    """Conv2d [Cout,Cin,k,k] / ConvTranspose2d [Cin,Cout,k,k] fp32 -> (int8 digit planes, scale, bias) (padded to 16)."""
    w = _dev(w.detach(), "weight", torch.float32)
    if transposed:
        Cin, Cout, k, k2 = w.shape
    else:
        Cout, Cin, k, k2 = w.shape
    if k != k2:
        raise NotImplementedError("square kernels only")
    return _pack_weight(w, bias, lib.spk_conv_packed_weight_i8_bytes(Cout, Cin, k), (Cout + 15) // 16 * 16, torch.int8,
                        lambda *t: lib.spk_pack_conv_weight_i8(*t, Cout, Cin, k, int(transposed), _stream(w)),
                        "spk_pack_conv_weight_i8", "spk_pack_conv_weight_i8: unsupported shape")


def conv_mfma_fused(in_ptc, packed, Cout, *, mode, k, stride, pad, transposed=False, out_pad=0, bn_a=None, bn_b=None,
                    v=None, coef=None, apply_tanh=False, want_u8=False, collapse_coef=None, out_s32=False):
    """in_ptc u8 [B,H,W,16,Cin] -> LIF: spikes u8 [B,Ho,Wo,16,Cout]; MEMOUT: dict(f32=[B,Cout,Ho,Wo], u8=...).
    LIF with collapse_coef [16]: returns sum_t collapse_coef[t] * spikes[t] as fp32 [B,Ho,Wo,Cout] instead of the spikes
    (input of readout_collapsed)."""
    in_ptc = _dev(in_ptc, "in_ptc", torch.uint8)
    B, H, W, T, Cin = in_ptc.shape
    Ho, Wo = conv_out_size(H, k, stride, pad, transposed, out_pad), conv_out_size(W, k, stride, pad, transposed, out_pad)
    wq, scale, bias_d = packed
    out_p = out_f = out_u = None
    if mode == MODE_LIF and out_s32:
        # nibble-packed "S32" spikes [B, Cout/32, Ho, Wo, 16, 16]: the input layout of the fp6 kernels
        o = empty_spikes(S32, B, Cout, Ho, Wo, T, in_ptc.device)
        check(lib.spk_conv_mfma_fused_lif_s32(_p(in_ptc), _p(wq), _p(scale), _p(bias_d), _p(bn_a), _p(bn_b), _p(v), _p(o), T, B,
                                              H, W, Cin, Cout, k, stride, pad, int(transposed), out_pad, _stream(in_ptc)),
              "spk_conv_mfma_fused_lif_s32")
        return o
    if mode == MODE_LIF and collapse_coef is not None:
        coef = _dev(collapse_coef, "collapse_coef", torch.float32)
        if coef.numel() != T:
            raise ValueError("collapse_coef must hold one coefficient per time step")
        out_f = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=in_ptc.device)
    elif mode == MODE_LIF:
        coef = None
        out_p = empty_spikes(PTC, B, Cout, Ho, Wo, T, in_ptc.device)
    else:
        out_f = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=in_ptc.device)
        if want_u8:
            out_u = torch.empty((B, Cout, Ho, Wo), dtype=torch.uint8, device=in_ptc.device)
    check(lib.spk_conv_mfma_fused_fwd(_p(in_ptc), _p(wq), _p(scale), _p(bias_d), _p(bn_a), _p(bn_b), _p(v), _p(out_p),
                                      _p(coef), _p(out_f), _p(out_u), int(apply_tanh), mode, T, B, H, W, Cin, Cout, k,
                                      stride, pad, int(transposed), out_pad, _stream(in_ptc)), "spk_conv_mfma_fused_fwd")
    if mode == MODE_LIF:
        return out_f if collapse_coef is not None else out_p
    return {"f32": out_f, "u8": out_u}


VAE_OUT_COLLAPSED, VAE_OUT_S32, VAE_OUT_PTC = (_C["SPK_VAE_OUT_" + n] for n in ("COLLAPSED", "S32", "PTC"))


def vae_fp6_kind(Cin, Cout, k, stride, pad, out_pad, transposed, T, H, W):
    """Which output form of the fp6 VQ-VAE kernel (csrc/vae_fp6.hip) exists for this 3x3 stride-2 layer on an H x W input:
    VAE_OUT_COLLAPSED (decoder convT2), VAE_OUT_S32 (decoder convT1), VAE_OUT_PTC (encoder conv2), or None."""
    kind = lib.spk_vae_fp6_kind(Cin, Cout, k, stride, pad, out_pad, int(bool(transposed)), T, H, W)
    return None if kind < 0 else kind


def convT_fp6_supported(Cin, Cout, k, stride, pad, out_pad, transposed, T, H, W):
    return vae_fp6_kind(Cin, Cout, k, stride, pad, out_pad, transposed, T, H, W) == VAE_OUT_COLLAPSED


def vae_fp6_pack(w, bias, transposed):
    """Conv2d [Cout,Cin,3,3] / ConvTranspose2d [Cin,Cout,3,3] fp32 (+bias) -> (digit tiles, scale f64, bias f64, qtab int32)."""
    w = _dev(w.detach(), "weight", torch.float32)
    Cin, Cout = (int(w.shape[0]), int(w.shape[1])) if transposed else (int(w.shape[1]), int(w.shape[0]))
    return _pack_weight(w, bias, lib.spk_vae_fp6_packed_bytes(Cout, Cin), Cout, torch.uint8,
                        lambda *t: lib.spk_vae_fp6_pack(*t, Cout, Cin, int(transposed), _stream(w)), "spk_vae_fp6_pack",
                        "spk_vae_fp6_pack: unsupported shape", extra=(((Cout, 9, Cin), torch.int32),)) + (Cin,)


def convT_fp6_pack(w, bias):
    return vae_fp6_pack(w, bias, True)


def ptc_to_s32(ptc):
    """u8 PTC spikes [B,H,W,16,C] -> S32 [B, ceil(C/32), H, W, 16, 16] (zero nibbles beyond C)."""
    ptc = _dev(ptc, "ptc", torch.uint8)
    B, H, W, T, C = ptc.shape
    o = empty_spikes(S32, B, C, H, W, T, ptc.device)
    check(lib.spk_ptc_to_s32(_p(ptc), _p(o), T, B, H * W, C, _stream(ptc)), "spk_ptc_to_s32")
    return o


def vae_fp6_fwd(in_s32, packed, Cout, *, bn_a, bn_b, transposed, out_kind, coef=None):
    """One spike-input 3x3 stride-2 VQ-VAE layer + BN + LIF from the reset state on the fp6 MFMA (see vae_fp6_kind).
    in_s32: S32 spikes [B, nch, H, W, 16, 16].  Returns fp32 [B,Ho,Wo,Cout] (collapsed), S32 [B,Cout/32,Ho,Wo,16,16] or u8 PTC
    [B,Ho,Wo,16,Cout]."""
    in_s32 = _dev(in_s32, "in_s32", C4_DTYPE)
    B, nch, H, W, T, rec = in_s32.shape
    wq, scale, bias_d, qtab, Cin = packed
    if rec != 16 or nch != (Cin + 31) // 32:
        raise ValueError("S32 spikes with ceil(Cin / 32) chunks expected")
    Ho, Wo = (2 * H, 2 * W) if transposed else (H // 2, W // 2)
    if out_kind == VAE_OUT_COLLAPSED:
        coef = _dev(coef, "coef", torch.float32)
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=in_s32.device)
    elif out_kind == VAE_OUT_S32:
        out = empty_spikes(S32, B, Cout, Ho, Wo, T, in_s32.device)
    else:
        out = empty_spikes(PTC, B, Cout, Ho, Wo, T, in_s32.device)
    flags = _flag_ws("vae", in_s32.device, lib.spk_vae_fp6_flag_words(B, Cout, Ho, Wo))
    check(lib.spk_vae_fp6_fwd(_p(in_s32), _p(wq), _p(scale), _p(bias_d), _p(qtab), _p(bn_a), _p(bn_b), _p(coef), _p(out),
                              int(out_kind), _p(flags), T, B, H, W, Cin, Cout, int(transposed), int(FLAG_CAP), _stream(in_s32)),
          "spk_vae_fp6_fwd")
    return out


def convT_fp6_collapsed(in_s32, packed, Cout, *, bn_a, bn_b, coef):
    """Decoder convT2: S32 spikes [B, 2, H, W, 16, 16] -> fp32 [B, 2H, 2W, Cout] = sum_t coef[t] * spikes[t]."""
    return vae_fp6_fwd(in_s32, packed, Cout, bn_a=bn_a, bn_b=bn_b, transposed=True, out_kind=VAE_OUT_COLLAPSED, coef=coef)


_COEF_SUMS = {}      # (data_ptr, _version, numel) of a coefficient tensor -> (its fp32 sum, an alias of the tensor)


def readout_collapsed_supported(Cin, Cout, k):
    """At any image width up to 64 (the library's W <= 0); readout_collapsed refuses wider images."""
    return bool(lib.spk_readout_collapsed_supported(Cin, Cout, k, 0))


def readout_collapsed(x_bhwc, weight, bias, coef, *, apply_tanh=False, want_u8=False, k=3, pad=1, transposed=True):
    """Linear read-out layer on time-collapsed spikes: x_bhwc fp32 [B,H,W,Cin] = sum_t coef[t] * spikes[t] (conv_mfma_fused
    with collapse_coef) -> dict(f32=[B,Cout,H,W] = conv(x) + bias * sum(coef) (tanh), u8=...).  Stride 1, 'same' padding.
    Refused here although the library takes them: the library's predicate depends on the image width (the kernel keeps
    4 + k - 1 rows of W positions in LDS), and this wrapper asks it at width 64 whatever W is, so that a layer's answer does
    not change with the image.  (Cin, Cout, k) that fit only narrower images -- e.g. (32, 9, 3), which
    spk_readout_collapsed_fwd runs up to W = 63 -- raise NotImplementedError at every width, as does any W > 64."""
    x = _dev(x_bhwc, "x", torch.float32)
    B, H, W, Cin = x.shape
    w = _dev(weight, "weight", torch.float32)
    Cout = w.shape[1] if transposed else w.shape[0]
    if W > 64 or not readout_collapsed_supported(Cin, Cout, k):
        raise NotImplementedError("spk_readout_collapsed_fwd: unsupported geometry")
    if bias is not None:
        bias = _dev(bias, "bias", torch.float32)
    out_f = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    out_u = torch.empty((B, Cout, H, W), dtype=torch.uint8, device=x.device) if want_u8 else None
    ckey = (coef.data_ptr(), coef._version, coef.numel())
    ent = _COEF_SUMS.get(ckey)
    csum = None if ent is None else ent[0]
    if csum is None:                    # (a device -> host copy: once per coefficient tensor, not per call)
        csum = 0.0
        for c in coef.detach().reshape(-1).float().cpu().tolist():      # fp32 left-to-right, as torch.sum over T would add
            csum = float(torch.tensor(csum, dtype=torch.float32) + torch.tensor(c, dtype=torch.float32))
        if len(_COEF_SUMS) > 16:
            _COEF_SUMS.clear()
        _COEF_SUMS[ckey] = (csum, coef.detach())    # (the alias keeps the storage: no other tensor gets this address under this key)
    check(lib.spk_readout_collapsed_fwd(_p(x), _p(w), _p(bias), float(csum), _p(out_f), _p(out_u), int(apply_tanh), B, H, W,
                                        Cin, Cout, int(k), int(pad), int(transposed), _stream(x)), "spk_readout_collapsed_fwd")
    return {"f32": out_f, "u8": out_u}


# ---------------------------------------------------------------------------------------------- VQ
def vq_readout_argmin(z_ptc, coef, alpha, codebook, want_zq=True, want_xm=False):
    z_ptc = _dev(z_ptc, "z_ptc", torch.uint8)
    B, H, W, T, D = z_ptc.shape
    codebook = _dev(codebook.detach(), "codebook", torch.float32)
    K = codebook.shape[0]
    coef = _dev(coef, "coef", torch.float32)
    if coef.numel() != T:
        raise RuntimeError(f"The size of tensor a ({T}) must match the size of tensor b ({coef.numel()}) at "
                           "non-singleton dimension 0")
    alpha = _dev(alpha.detach().reshape(1), "alpha", torch.float32)
    idx = torch.empty(B * H * W, dtype=torch.int64, device=z_ptc.device)
    zq = torch.empty((B, D, H, W), dtype=torch.float32, device=z_ptc.device) if want_zq else None
    xm = torch.empty((B * H * W, D), dtype=torch.float32, device=z_ptc.device) if want_xm else None
    check(lib.spk_vq_readout_argmin(_p(z_ptc), _p(coef), _p(alpha), _p(codebook), _p(idx), _p(zq), _p(xm), T, B, D,
                                    H * W, K, _stream(z_ptc)), "spk_vq_readout_argmin")
    return idx, zq, xm


def vq_argmin(flat_x, codebook):
    flat_x = _dev(flat_x, "flat_x", torch.float32)
    codebook = _dev(codebook.detach(), "codebook", torch.float32)
    N, D = flat_x.shape
    idx = torch.empty(N, dtype=torch.int64, device=flat_x.device)
    check(lib.spk_vq_argmin(_p(flat_x), _p(codebook), _p(idx), N, D, codebook.shape[0], _stream(flat_x)),
          "spk_vq_argmin")
    return idx


VQ_USAGE_MAX_K = _C["SPK_VQ_USAGE_MAX_K"]     # spk_vq_code_usage keeps the histogram in LDS: larger codebooks take the torch ops below


class CodeUsage(NamedTuple):
    """Codebook-usage statistic of VectorQuantizer_uni (R/snn_model/vae_model.py:705-718), device tensors.  hist, used,
    max_index and fid_loss are views of ``packed`` (int64 [K + 3] = hist, used, max_index, fp32 bits of fid_loss), so one
    device-to-host copy of ``packed`` carries all of it."""
    hist: torch.Tensor           # int64 [K]   bincount(idx, minlength=K)
    used: torch.Tensor           # int64 []    len(unique(idx))
    max_index: torch.Tensor      # int64 []    argmax(hist), first maximum
    fid_loss: torch.Tensor       # fp32 []     0.001 * mse_loss(hist without max_index, N / K)
    packed: torch.Tensor


def _code_usage_views(packed, K):
    return CodeUsage(packed[:K], packed[K], packed[K + 1], packed[K + 2:K + 3].view(torch.float32)[0], packed)


def unpack_code_usage(packed_host):
    """Host copy of CodeUsage.packed -> (hist int64 [K], used, max_index, fid_loss as a Python float)."""
    K = packed_host.numel() - 3
    return (packed_host[:K], int(packed_host[K]), int(packed_host[K + 1]),
            float(packed_host[K + 2:K + 3].view(torch.float32)[0]))


def vq_code_usage_torch(idx, K):
    """The statistic with the framework's operators, as the reference spells it (the fallback for K > VQ_USAGE_MAX_K)."""
    N = idx.numel()
    packed = torch.zeros(K + 3, dtype=torch.int64, device=idx.device)
    hist = torch.bincount(idx.reshape(-1), minlength=K)
    packed[:K] = hist
    packed[K] = (hist > 0).sum()
    m = torch.argmax(hist)
    packed[K + 1] = m
    mask = torch.ne(torch.arange(K, device=idx.device), m)
    targets = (torch.ones(K) * N / K).to(idx.device)
    fid = 0.001 * F.mse_loss(torch.masked_select(hist, mask), torch.masked_select(targets, mask))
    packed[K + 2:K + 3].view(torch.float32)[0] = fid
    return _code_usage_views(packed, K)


def vq_code_usage(idx, K):
    """idx int64 [N] (device) -> CodeUsage: the histogram, the number of used codes, the first maximum and FID_loss of
    R/snn_model/vae_model.py:705-718, one launch (spk_vq_code_usage) and no host synchronisation.  Integer results are
    exact, the whole result deterministic.  K > VQ_USAGE_MAX_K takes vq_code_usage_torch."""
    idx = _dev(idx.reshape(-1), "idx", torch.int64)
    K = int(K)
    if K < 1:
        raise ValueError(f"vq_code_usage: K must be positive, got {K}")
    packed = torch.empty(K + 3, dtype=torch.int64, device=idx.device)
    ws = torch.empty(K + 1, dtype=torch.int64, device=idx.device)
    rc = lib.spk_vq_code_usage(_p(idx), idx.numel(), K, _p(packed), _p(packed[K:]), _p(ws), _stream(idx))
    if rc == _C["SPK_ERR_UNSUPPORTED"] and K > VQ_USAGE_MAX_K:
        return vq_code_usage_torch(idx, K)
    check(rc, "spk_vq_code_usage")
    return _code_usage_views(packed, K)


SSIM_MAX_WINDOW = _C["SPK_SSIM_MAX_WINDOW"]   # spk_ssim_mse stages a 32x32 tile plus the window's halo in LDS


def ssim_mse_out_size(n, window_size):
    """H' of the SSIM map: F.conv2d(padding=window_size // 2) of an n-pixel side (n for an odd window, n + 1 for an even one)."""
    return n + 2 * (window_size // 2) - window_size + 1


def ssim_mse(img1, img2, window2d, ws=None, out=None):
    """img1, img2 fp32 [N,C,H,W] and the 2-D window fp32 [ws,ws] of metric.pytorch_ssim.create_window (device) ->
    (ssim_sum fp64 [N], sq_sum fp64 [N]): per image the sum of the SSIM map over (C, H', W') and the sum of (img1 - img2)^2
    over (C, H, W), fp64 arithmetic, one launch (spk_ssim_mse), deterministic, no host synchronisation.  ``ws``: a workspace
    of ``ssim_mse_ws(...)`` to reuse (this call's alone while it is in flight); ``out``: fp64 [2, N] to write (rows ssim_sum,
    sq_sum)."""
    img1 = _dev(img1, "img1", torch.float32)
    img2 = _dev(img2, "img2", torch.float32)
    window2d = _dev(window2d, "window2d", torch.float32)
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise ValueError(f"ssim_mse: img1 {tuple(img1.shape)} and img2 {tuple(img2.shape)} must be equal [N,C,H,W] shapes")
    if img2.device != img1.device or window2d.device != img1.device:
        raise ValueError("ssim_mse: img1, img2 and window2d must be on one device")
    if window2d.dim() != 2 or window2d.shape[0] != window2d.shape[1]:
        raise ValueError(f"ssim_mse: window2d must be [ws, ws], got {tuple(window2d.shape)}")
    N, C, H, W = img1.shape
    wsz = int(window2d.shape[0])
    nbytes = int(lib.spk_ssim_mse_ws_bytes(N, C, H, W, wsz))
    if nbytes < 0:
        check(nbytes, "spk_ssim_mse_ws_bytes")
    if ws is None:
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=img1.device)
    elif not (ws.is_cuda and ws.device == img1.device and ws.is_contiguous() and ws.data_ptr() % 8 == 0
              and ws.numel() * ws.element_size() >= nbytes):
        raise ValueError(f"ssim_mse: ws must be a contiguous 8-byte aligned device buffer of at least {nbytes} bytes")
    if out is None:
        out = torch.empty((2, N), dtype=torch.float64, device=img1.device)
    elif not (out.is_cuda and out.device == img1.device and out.dtype == torch.float64 and out.is_contiguous()
              and out.shape == (2, N)):
        raise ValueError(f"ssim_mse: out must be a contiguous fp64 [2, {N}] device tensor")
    check(lib.spk_ssim_mse(_p(img1), _p(img2), _p(window2d), _p(out[0]), _p(out[1]), _p(ws), N, C, H, W, wsz, _stream(img1)),
          "spk_ssim_mse")
    return out[0], out[1]


def ssim_mse_ws(N, C, H, W, window_size, device):
    """A workspace for ssim_mse calls of this shape."""
    nbytes = int(lib.spk_ssim_mse_ws_bytes(N, C, H, W, window_size))
    if nbytes < 0:
        check(nbytes, "spk_ssim_mse_ws_bytes")
    return torch.empty(nbytes // 8, dtype=torch.int64, device=device)


FEATURE_MAX_D = _C["SPK_FEATURE_MAX_D"]                    # widest feature matrix of feature_moments / poly_kernel_sums
POLY_KERNEL_MAX_DEGREE = _C["SPK_POLY_KERNEL_MAX_DEGREE"]


def feature_moments(x, sum, gram):
    """x fp32 [n, d] (device; rows may be strided, the columns of a row are contiguous), ``sum`` fp64 [d] and ``gram`` fp64 [d, d]
    (contiguous device state, updated in place): sum += x.sum(0), gram += x^T x on the fp64 matrix cores
    (spk_feature_moments_acc: exact products, one accumulation chain per element, deterministic, no host synchronisation).
    n = 0 is a no-op.  Returns (sum, gram)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"spkdiff: feature_moments: x is on '{getattr(x, 'device', type(x))}'; there is no CPU path")
    if x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError(f"feature_moments: x must be fp32 [n, d], got {x.dtype} {tuple(x.shape)}")
    n, d = int(x.shape[0]), int(x.shape[1])
    if d < 1:
        raise ValueError("feature_moments: d must be >= 1")
    if n > 1 and (x.stride(1) != 1 or x.stride(0) < d):
        x = x.contiguous()
    elif n <= 1 and d > 1 and x.stride(1) != 1:
        x = x.contiguous()
    stride = int(x.stride(0)) if n > 1 else d
    for t, name, shape in ((sum, "sum", (d,)), (gram, "gram", (d, d))):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == x.device and t.dtype == torch.float64
                and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"feature_moments: {name} must be a contiguous fp64 {list(shape)} tensor on {x.device} (it is the "
                             f"state the call updates in place)")
    check(lib.spk_feature_moments_acc(_p(x), n, d, stride, _p(sum), _p(gram), _stream(x)), "spk_feature_moments_acc")
    return sum, gram


def _index_table(t, name, rows, device):
    """An index table of poly_kernel_sums as a contiguous int32 [S, count] device tensor.  A table still on the host is checked
    here (every entry in [0, rows)) and uploaded; a device table is the caller's contract (the kernel reads no row for a bad
    entry and that subset's sums are NaN)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"poly_kernel_sums: {name} must be an int32 [S, count] tensor")
    if not t.is_cuda:
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= rows):
            raise ValueError(f"poly_kernel_sums: {name} names a row outside [0, {rows})")
        t = t.to(torch.int32).to(device)
    elif t.dtype != torch.int32:
        raise ValueError(f"poly_kernel_sums: a device {name} must be int32")
    return t if t.is_contiguous() else t.contiguous()


def poly_kernel_sums_ws(S, p, q, device):
    """A workspace for poly_kernel_sums calls of this shape (one pair of fp64 partials per 16x16 tile and subset)."""
    nbytes = int(lib.spk_poly_kernel_sums_ws_bytes(S, p, q))
    if nbytes < 0:
        check(nbytes, "spk_poly_kernel_sums_ws_bytes")
    return torch.empty(nbytes // 8, dtype=torch.int64, device=device)


def poly_kernel_sums(X, Y, ix=None, iy=None, p=None, q=None, gamma=None, coef=1.0, degree=3, symmetric=False, ws=None, out=None):
    """X fp32 [n_x, d], Y fp32 [n_y, d] (device); ``ix`` int32 [S, p] / ``iy`` int32 [S, q] tables of row numbers (None: rows
    0 .. p - 1 / 0 .. q - 1, one subset; p / q default to all rows) -> out fp64 [S, 2]:
    out[s, 0] = sum_{i, j} (gamma <X[ix[s, i]], Y[iy[s, j]]> + coef)^degree, out[s, 1] = the sum of the (i, i) terms when
    ``symmetric`` (pass Y = X and iy = ix), else 0.  gamma None: 1 / d.  One call serves all S subsets; the p x q Gram matrix is
    never written (spk_poly_kernel_sums: fp64 matrix cores, fixed-order sums, deterministic, no host synchronisation).  ``ws``: a
    workspace of ``poly_kernel_sums_ws`` to reuse (this call's alone while it is in flight)."""
    for t, name in ((X, "X"), (Y, "Y")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"spkdiff: poly_kernel_sums: {name} is on '{getattr(t, 'device', type(t))}'; there is no CPU path")
        if t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"poly_kernel_sums: {name} must be fp32 [n, d], got {t.dtype} {tuple(t.shape)}")
    if X.shape[1] != Y.shape[1] or X.device != Y.device:
        raise ValueError(f"poly_kernel_sums: X {tuple(X.shape)} and Y {tuple(Y.shape)} must share d and the device")
    X = X if X.is_contiguous() else X.contiguous()
    Y = Y if Y.is_contiguous() else Y.contiguous()
    n_x, n_y, d = int(X.shape[0]), int(Y.shape[0]), int(X.shape[1])
    if ix is not None:
        ix = _index_table(ix, "ix", n_x, X.device)
    if iy is not None:
        iy = _index_table(iy, "iy", n_y, X.device)
    if (ix is None) != (iy is None) and (ix if ix is not None else iy).shape[0] != 1:
        raise ValueError("poly_kernel_sums: one table alone needs S = 1")
    if ix is not None and iy is not None and ix.shape[0] != iy.shape[0]:
        raise ValueError(f"poly_kernel_sums: ix has {ix.shape[0]} subsets and iy {iy.shape[0]}")
    S = int(ix.shape[0]) if ix is not None else int(iy.shape[0]) if iy is not None else 1
    p = int(ix.shape[1]) if ix is not None else n_x if p is None else int(p)
    q = int(iy.shape[1]) if iy is not None else n_y if q is None else int(q)
    gc = (ctypes.c_double * 2)(1.0 / d if gamma is None else float(gamma), float(coef))
    nbytes = int(lib.spk_poly_kernel_sums_ws_bytes(S, p, q))
    if nbytes < 0:
        check(nbytes, "spk_poly_kernel_sums_ws_bytes")
    if ws is None:
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=X.device)
    elif not (ws.is_cuda and ws.device == X.device and ws.is_contiguous() and ws.data_ptr() % 8 == 0
              and ws.numel() * ws.element_size() >= nbytes):
        raise ValueError(f"poly_kernel_sums: ws must be a contiguous 8-byte aligned device buffer of at least {nbytes} bytes")
    if out is None:
        out = torch.empty((S, 2), dtype=torch.float64, device=X.device)
    elif not (out.is_cuda and out.device == X.device and out.dtype == torch.float64 and out.is_contiguous()
              and tuple(out.shape) == (S, 2)):
        raise ValueError(f"poly_kernel_sums: out must be a contiguous fp64 [{S}, 2] device tensor")
    check(lib.spk_poly_kernel_sums(_p(X), n_x, _p(Y), n_y, d, _p(ix), _p(iy), S, p, q, ctypes.addressof(gc), int(degree),
                                   int(bool(symmetric)), _p(out), _p(ws), ws.numel() * ws.element_size(), _stream(X)),
          "spk_poly_kernel_sums")
    return out


def _vq_train_ws(device):
    """Block partials and the last-block ticket of spk_vq_train_quant / _bwd, spk_psp_loss_fwd and spk_recon_loss_fwd.  The
    ticket protocol needs the buffer to itself while a launch is in flight, so it is one buffer per (device, stream) -- or per
    ops.flag_scope store under capture -- with _flag_ws's rule against a first use during capture."""
    return _flag_ws("vq_train", device, (int(lib.spk_vq_train_ws_bytes()) + 3) // 4)


class VQTrainFunction(torch.autograd.Function):
    """Training branch of VectorQuantizer.forward up to the spike generator (R/snn_model/vae_model.py:61-78): read-out, code
    search, VQ + commitment loss and the straight-through value as three launches (spk_vq_train_readout, spk_vq_argmin,
    spk_vq_train_quant); the backward -- gradients of the encoder spikes, of alpha and of the codebook -- is one
    (spk_vq_train_bwd: the codebook rows are summed by one workgroup per code in a fixed order).
    apply(x_seq [T,B,D,h,w], coef [T], alpha [] , codebook [K,D], beta) -> (quantized [B,D,h,w], loss_1 [])."""

    @staticmethod
    def forward(ctx, x_seq, coef, alpha, codebook, beta):
        x = _dev(x_seq.detach(), "x_seq", torch.float32)
        T, B, D, h, w = x.shape
        HW, N = h * w, B * h * w
        cf = _dev(coef.detach().flatten(), "coef", torch.float32)
        al = _dev(alpha.detach().reshape(1), "alpha", torch.float32)
        E = _dev(codebook.detach(), "codebook", torch.float32)
        xm = torch.empty((N, D), dtype=torch.float32, device=x.device)
        dxa = torch.empty_like(xm)
        check(lib.spk_vq_train_readout(_p(x), _p(cf), _p(al), _p(xm), _p(dxa), T, B, D, HW, _stream(x)), "spk_vq_train_readout")
        idx = vq_argmin(xm, E)
        out = torch.empty((B, D, h, w), dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ws = _vq_train_ws(x.device)
        check(lib.spk_vq_train_quant(_p(xm), _p(idx), _p(E), _p(out), _p(loss), float(beta), _p(ws), N, D, HW, _stream(x)),
              "spk_vq_train_quant")
        ctx.save_for_backward(xm, idx, E, dxa, cf, al)
        # (the backward runs on this stream, but in autograd's own thread, which sees neither this thread's flag_scope nor,
        #  under capture, a workspace of its own: it takes the forward's)
        ctx.ws = ws
        ctx.cfg = (T, B, D, h, w, float(beta), tuple(alpha.shape))
        ctx.mark_non_differentiable(idx)
        ctx.indices = idx
        return out, loss

    @staticmethod
    def backward(ctx, g_out, g_loss):
        xm, idx, E, dxa, cf, al = ctx.saved_tensors
        T, B, D, h, w, beta, ashape = ctx.cfg
        N, K = B * h * w, E.shape[0]
        go = torch.zeros((B, D, h, w), dtype=torch.float32, device=xm.device) if g_out is None else g_out.contiguous()
        gl = None if g_loss is None else g_loss.reshape(1).contiguous()
        gx = torch.empty((T, B, D, h, w), dtype=torch.float32, device=xm.device)
        ga = torch.empty(1, dtype=torch.float32, device=xm.device)
        gE = torch.empty_like(E)
        with timed("train.vq_bwd"):
            check(lib.spk_vq_train_bwd(_p(go), _p(gl), _p(xm), _p(idx), _p(E), _p(dxa), _p(cf), _p(al), beta, _p(gx), _p(ga), _p(gE),
                                       _p(ctx.ws), T, N, D, h * w, K, _stream(xm)), "spk_vq_train_bwd")
        return gx, None, ga.reshape(ashape), gE, None


class PSPLossFunction(torch.autograd.Function):
    """loss_2 of VectorQuantizer.forward (R/snn_model/vae_model.py:79-84): mean((psp(q) - sg(psp(x)))^2) + beta * mean((sg(psp(q)) -
    psp(x))^2) over spike tensors [T, ...] -- one launch forward (spk_psp_loss_fwd: both filters in registers), one backward
    (spk_psp_loss_bwd: both adjoint filters) instead of four filter launches and ~16 element-wise / reduce launches.
    apply(q_seq, x_seq, beta, tau_s) -> loss []."""

    @staticmethod
    def forward(ctx, q_seq, x_seq, beta, tau_s):
        q = _dev(q_seq.detach(), "q_seq", torch.float32)
        x = _dev(x_seq.detach(), "x_seq", torch.float32)
        if q.shape != x.shape:
            raise ValueError(f"PSP loss: shapes {tuple(q.shape)} and {tuple(x.shape)} differ")
        T, N = q.shape[0], q[0].numel()
        if T > 16:
            raise NotImplementedError("spk_psp_loss: at most 16 time steps")
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        check(lib.spk_psp_loss_fwd(_p(q), _p(x), _p(loss), float(beta), float(tau_s), _p(_vq_train_ws(q.device)), T, N, _stream(q)),
              "spk_psp_loss_fwd")
        ctx.save_for_backward(q, x)
        ctx.cfg = (float(beta), float(tau_s))
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        q, x = ctx.saved_tensors
        beta, tau_s = ctx.cfg
        T, N = q.shape[0], q[0].numel()
        gq, gx = torch.empty_like(q), torch.empty_like(x)
        with timed("train.psp_loss_bwd"):
            check(lib.spk_psp_loss_bwd(_p(q), _p(x), _p(g_loss.reshape(1).contiguous()), _p(gq), _p(gx), beta, tau_s, T, N, _stream(q)),
                  "spk_psp_loss_bwd")
        return gq, gx, None, None


class ReconLossFunction(torch.autograd.Function):
    """mse_loss(tanh(memout(y)), image) of SNN_VQVAE.forward in training (R/snn_model/vae_model.py:189-196): read-out, tanh and the
    mean square as one launch, the gradient of the decoder's output as another (spk_recon_loss_fwd / _bwd).
    apply(y_seq [T,B,C,H,W], coef [T], image [B,C,H,W]) -> loss []."""

    @staticmethod
    def forward(ctx, y_seq, coef, image):
        y = _dev(y_seq.detach(), "y_seq", torch.float32)
        img = _dev(image.detach(), "image", torch.float32)
        cf = _dev(coef.detach().flatten(), "coef", torch.float32)
        T, N = y.shape[0], y[0].numel()
        if img.numel() != N or cf.numel() != T:
            raise ValueError(f"recon loss: y {tuple(y.shape)}, image {tuple(img.shape)}, coef {tuple(cf.shape)}")
        xr = torch.empty_like(img)
        loss = torch.empty((), dtype=torch.float32, device=y.device)
        check(lib.spk_recon_loss_fwd(_p(y), _p(cf), _p(img), _p(xr), _p(loss), _p(_vq_train_ws(y.device)), T, N, _stream(y)),
              "spk_recon_loss_fwd")
        ctx.save_for_backward(xr, img, cf)
        ctx.shape = tuple(y.shape)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        xr, img, cf = ctx.saved_tensors
        gy = torch.empty(ctx.shape, dtype=torch.float32, device=xr.device)
        with timed("train.recon_loss_bwd"):
            check(lib.spk_recon_loss_bwd(_p(xr), _p(img), _p(cf), _p(g_loss.reshape(1).contiguous()), _p(gy), ctx.shape[0], xr.numel(),
                                         _stream(xr)), "spk_recon_loss_bwd")
        return gy, None, None


def embedding(tokens, codebook, nchw_hw=None):
    """nn.Embedding lookup; nchw_hw=(h,w) writes [B,D,h,w] for tokens [B,h,w]."""
    tokens = _dev(tokens, "tokens", torch.int64)
    codebook = _dev(codebook.detach(), "codebook", torch.float32)
    K, D = codebook.shape
    N = tokens.numel()
    if nchw_hw is None:
        out = torch.empty(tuple(tokens.shape) + (D,), dtype=torch.float32, device=tokens.device)
        HW, nchw = 1, 0
    else:
        h, w = nchw_hw
        HW, nchw = h * w, 1
        out = torch.empty((N // HW, D, h, w), dtype=torch.float32, device=tokens.device)
    check(lib.spk_embedding_fwd(_p(tokens), _p(codebook), _p(out), N, D, K, HW, nchw, _stream(tokens)),
          "spk_embedding_fwd")
    return out


def spikegen_tokens_s32(tokens, codebook, w_packed, bias, bn_a, bn_b, T=16, table_key=None, table_slot=None, table_hold=None):
    """tokens int64 [B,h,w] -> S32 spikes [B,1,h,w,16,16] of the spike generator (embedding + 1x1 conv + BN + LIF from the reset state on
    the repeated code vector), by a per-token pattern table (spk_spikegen_tokens_s32).  w_packed: [1][D][Cout], Cout 16 or 32.
    table_slot: a dict OWNED BY THE CALLER's module (one per spike generator: no table is shared between models) that keeps the table
    buffer per (device, K, Cout) with the key and the stream of its last eager build.  table_key: anything that changes whenever
    codebook, weights or BN terms do (parameter versions + the owner's invalidation epoch); the slot's table is reused while the key
    AND the stream are equal.  table_hold: aliases of the tensors the key names, kept with it (their storage cannot be recycled under an
    equal key).  A call under stream capture always builds, into a buffer of its own (the graph's pool), and never touches
    the slot: a replay bakes the derived inputs of capture time and must not leave its table behind an eager call's key."""
    tokens = _dev(tokens, "tokens", torch.int64)
    codebook = _dev(codebook.detach(), "codebook", torch.float32)
    K, D = codebook.shape
    kk, Cin, Cout = w_packed.shape
    if kk != 1 or Cin != D:
        raise ValueError("a 1x1 generator over the code vector expected")
    nbytes = lib.spk_spikegen_table_bytes(K, Cout)
    if nbytes < 0 or T != 16:
        raise NotImplementedError("spikegen_tokens_s32: Cout 16 or 32, T = 16")
    stream = _stream(tokens)
    capturing = torch.cuda.is_current_stream_capturing()
    ent = None
    if table_slot is not None and not capturing:    # (a captured call builds into a buffer of its own, from the graph's pool: replays
        skey = (tokens.device, K, Cout)             #  -- which bake the derived inputs of capture time -- never write the eager slot)
        ent = table_slot.get(skey)
        if ent is None:
            ent = table_slot[skey] = [torch.empty(nbytes // 2, dtype=torch.int16, device=tokens.device), None, None, None]
    if ent is None:
        ws, build = torch.empty(nbytes // 2, dtype=torch.int16, device=tokens.device), True
    else:
        ws = ent[0]
        build = table_key is None or ent[1] != table_key or ent[2] != stream
        ent[1:] = (None, None, None) if table_key is None else (table_key, stream, table_hold)
    B, h, w = tokens.shape
    out = empty_spikes(S32, B, Cout, h, w, T, tokens.device)
    check(lib.spk_spikegen_tokens_s32(_p(tokens), _p(codebook), _p(w_packed), _p(bias), _p(bn_a), _p(bn_b), _p(ws), int(build), _p(out),
                                      T, tokens.numel(), K, D, Cout, stream), "spk_spikegen_tokens_s32")
    return out


# ---------------------------------------------------------------------------------------------- sampler
def den_build_input(x, t, out=None):
    """x: float [B,1,h,w] or int64 tokens; t: int64 [B] tensor or python int -> fp32 [B,2,h,w]."""
    xf = xi = None
    if x.dtype == torch.int64:
        xi = _dev(x, "x_t", torch.int64)
    else:
        xf = _dev(x, "x", torch.float32)
    B = x.shape[0]
    HW = x[0].numel()
    h, w = x.shape[-2], x.shape[-1]
    if out is None:
        out = torch.empty((B, 2, h, w), dtype=torch.float32, device=x.device)
    tv, ts = None, 0
    if torch.is_tensor(t):
        tv = _dev(t, "t", torch.int64)
        if tv.numel() != B:
            raise ValueError("t must have one entry per sample")
    else:
        ts = int(t)
    act, nact = (None, None) if ACTIVE is None else ACTIVE
    check(lib.spk_den_build_input(_p(xf), _p(xi), _p(tv), ts, _p(out), B, HW, _p(act), _p(nact), _stream(x)),
          "spk_den_build_input")
    return out


def _temp_arg(temp, B, what):
    """The temperature of a token update: (fp32 device tensor [B], None) for a per-image vector -- the ``_temps`` entry point --
    or (None, float) for anything ``float()`` takes (a number, a 0-dim or one-element tensor): the scalar entry point, unchanged.
    A vector is taken as given: contiguous fp32 on the device, one entry per image of the call (index = image, also inside an
    ``active_set`` scope); its values are the caller's (the kernels divide by whatever is there)."""
    if not (isinstance(temp, torch.Tensor) and temp.numel() > 1):
        return None, float(temp)
    if temp.dtype != torch.float32 or not temp.is_cuda or not temp.is_contiguous() or temp.dim() != 1 or temp.numel() != int(B):
        raise ValueError(f"{what}: a per-image temp must be a contiguous fp32 device tensor of B = {int(B)} entries, got "
                         f"{temp.dtype} {tuple(temp.shape)} on '{temp.device}'")
    return temp, None


def _token_state(x_t, unmasked, n, what):
    """The state a token update writes in place: contiguous device tensors of ``n`` entries (``what``: the messages' description)."""
    if x_t.dtype != torch.int64 or not x_t.is_cuda or not x_t.is_contiguous():
        raise ValueError(f"x_t must be a contiguous int64 device tensor {what}")
    if unmasked.dtype not in (torch.bool, torch.uint8) or not unmasked.is_cuda or not unmasked.is_contiguous():
        raise ValueError(f"unmasked must be a contiguous bool/uint8 device tensor {what}")
    if x_t.numel() != n or unmasked.numel() != n:
        raise ValueError("x_t / unmasked size mismatch")


def _step_noise(u, q, philox_state, n, K):
    """The noise arguments of a token update, each optional: u fp32 [n], q fp32 [n * K] (device), philox_state int64 [2] -> (u, q)."""
    if u is not None:
        u = _dev(u, "u", torch.float32)
        if u.numel() != n:
            raise ValueError("u must have B*HW entries")
    if q is not None:
        q = _dev(q, "q", torch.float32)
        if q.numel() != n * K:
            raise ValueError("q must have B*HW*K entries")
    if philox_state is not None and (philox_state.dtype != torch.int64 or philox_state.numel() != 2):
        raise ValueError("philox_state must be an int64 device tensor {seed, base offset}")
    return u, q


def _next_input_arg(next_input, n):
    """The optional buffer for the next reverse step's denoiser input cat(x_t, t - 1): fp32 [B,2,h,w], contiguous."""
    if next_input is not None:
        next_input = _dev(next_input, "next_input", torch.float32)
        if next_input.numel() != 2 * n or not next_input.is_contiguous():
            raise ValueError("next_input must be a contiguous fp32 [B,2,h,w] tensor")
    return next_input


def _topk_arg(top_k, temp, B, what, device):
    """``top_k`` of a token update: None -- the call as it always was, (None, temp) -- or an int32 device tensor
    [B], one k per image of the call (index = image, also inside an ``active_set`` scope; k <= 0 or k >= K: that image is not
    truncated), taken as given: returns (top_k, temp_b).  The ``_topk`` entry points take their temperatures per image too: a
    vector goes through as it is (fp32 [B] on the device), a number is broadcast."""
    if top_k is None:
        return None, temp
    B = int(B)
    if (not isinstance(top_k, torch.Tensor) or top_k.dtype != torch.int32 or not top_k.is_cuda or not top_k.is_contiguous() or
            top_k.dim() != 1 or top_k.numel() != B):
        got = f"{top_k.dtype} {tuple(top_k.shape)} on '{top_k.device}'" if isinstance(top_k, torch.Tensor) else repr(type(top_k))
        raise ValueError(f"{what}: top_k must be a contiguous int32 device tensor of B = {B} entries, got {got}")
    if isinstance(temp, torch.Tensor) and temp.is_cuda and temp.dtype == torch.float32 and temp.dim() == 1 and temp.numel() == B:
        return top_k, temp.contiguous()
    temp_b, temp = _temp_arg(temp, B, what)
    return top_k, temp_b if temp_b is not None else torch.full((B,), temp, dtype=torch.float32, device=device)


def _topp_arg(top_p, top_k, temp, B, what, device):
    """``top_p`` of a token update: None -- the call as it was, (None, top_k, temp) -- or a contiguous fp32 device
    tensor [B], one p per image of the call (index = image, also inside an ``active_set`` scope; a p outside (0, 1): that image is
    not nucleus-truncated), taken as given: returns (top_p, top_k, temp).  The ``_topp`` entry points take all three per image: a
    missing ``top_k`` becomes zeros (no top-k truncation), and a scalar ``temp`` is broadcast by ``_topk_arg``."""
    if top_p is None:
        return None, top_k, temp
    B = int(B)
    if (not isinstance(top_p, torch.Tensor) or top_p.dtype != torch.float32 or not top_p.is_cuda or not top_p.is_contiguous() or
            top_p.dim() != 1 or top_p.numel() != B):
        got = f"{top_p.dtype} {tuple(top_p.shape)} on '{top_p.device}'" if isinstance(top_p, torch.Tensor) else repr(type(top_p))
        raise ValueError(f"{what}: top_p must be a contiguous fp32 device tensor of B = {B} entries, got {got}")
    if top_k is None:
        top_k = torch.zeros(B, dtype=torch.int32, device=device)
    return top_p, top_k, temp


def _launch_by_temp(name, temp_b, temp, head, tail, top_k=None, top_p=None):
    """Launch ``name(*head, temp, *tail)`` or, ``temp_b`` given, its ``_temps`` sibling with the vector (looked up per call);
    ``top_k`` given (then with ``temp_b``): its ``_topk`` sibling with both vectors; ``top_p`` given (then with both): its
    ``_topp`` sibling with the three."""
    if top_p is not None:
        name = name + "_topp"
        check(getattr(lib, name)(*head, _p(temp_b), _p(top_k), _p(top_p), *tail), name)
        return
    if top_k is not None:
        name = name + "_topk"
        check(getattr(lib, name)(*head, _p(temp_b), _p(top_k), *tail), name)
        return
    if temp_b is not None:
        name, temp = name + "_temps", _p(temp_b)
    check(getattr(lib, name)(*head, temp, *tail), name)


def psample_step(logits, x_t, unmasked, t, temp=1.0, u=None, q=None, seed=0, offset=0, x0_hat=None, philox_state=None,
                 next_input=None, top_k=None, top_p=None):
    """In-place update of x_t (int64) and unmasked (bool/u8) from logits [B,K,h,w].  next_input (dense form only): fp32
    [B,2,h,w] that receives the denoiser input of the next reverse step, cat(x_t, t - 1).  ``temp``: a number, or a contiguous
    fp32 device tensor with one temperature per image (spk_psample_step_temps).  ``top_k``: int32 device tensor with one k per
    image -- every drawn token comes from its position's k likeliest classes (spk_psample_step_topk; 0: not truncated).
    ``top_p``: fp32 device tensor with one p per image -- nucleus truncation after the top-k one (spk_psample_step_topp; a p
    outside (0, 1): none); a scalar ``temp`` is then broadcast and a missing ``top_k`` becomes zeros."""
    logits = _dev(logits, "logits", torch.float32)
    B, K = logits.shape[0], logits.shape[1]
    HW = logits[0, 0].numel()
    n = B * HW
    top_p, top_k, temp = _topp_arg(top_p, top_k, temp, x_t.numel() // HW, "psample_step", logits.device)
    top_k, temp = _topk_arg(top_k, temp, x_t.numel() // HW, "psample_step", logits.device)
    temp_b, temp = (temp, None) if top_k is not None else _temp_arg(temp, x_t.numel() // HW, "psample_step")
    _token_state(x_t, unmasked, n, "(updated in place)")
    u, q = _step_noise(u, q, philox_state, n, K)
    act, nact = (None, None) if ACTIVE is None else ACTIVE
    next_input = _next_input_arg(next_input, n)
    _launch_by_temp("spk_psample_step", temp_b, temp, (_p(logits), _p(x_t), _p(unmasked), int(t)),
                    (_p(u), _p(q), int(seed), int(offset), _p(philox_state), _p(x0_hat), B, HW, K, _p(act), _p(nact), _p(next_input),
                     _stream(logits)), top_k=top_k, top_p=top_p)
    return x_t, unmasked


def pscore_step(logits, x0, x_t, unmasked, t, temp, logp, step=None, u=None, seed=0, offset=0, philox_state=None,
                next_input=None):
    """``psample_step`` run teacher-forced (spk_pscore_step): the positions reverse step ``t`` reveals -- the same u / Philox
    arguments, the same test -- take the GIVEN token ``x0`` (int64, one per position) instead of a sampled one, and its
    log-probability under softmax(logits / temp) goes to ``logp`` (fp64, nats) and ``t`` to ``step`` (int32, optional); the other
    positions of ``logp`` / ``step`` are not written.  x_t / unmasked in place; ``next_input`` and the ``active_set`` scope as
    for psample_step; ``temp`` a number or a per-image fp32 device tensor (spk_pscore_step_temps)."""
    logits = _dev(logits, "logits", torch.float32)
    B, K = logits.shape[0], logits.shape[1]
    HW = logits[0, 0].numel()
    n = B * HW
    temp_b, temp = _temp_arg(temp, B, "pscore_step")
    x0 = _dev(x0, "x0", torch.int64)
    _token_state(x_t, unmasked, n, "(updated in place)")
    if not isinstance(logp, torch.Tensor) or logp.dtype != torch.float64 or not logp.is_cuda or not logp.is_contiguous():
        raise ValueError("logp must be a contiguous fp64 device tensor (written where a position is revealed)")
    if step is not None and (step.dtype != torch.int32 or not step.is_cuda or not step.is_contiguous()):
        raise ValueError("step must be a contiguous int32 device tensor (written where a position is revealed)")
    if x0.numel() != n or logp.numel() != n or (step is not None and step.numel() != n):
        raise ValueError("x0 / x_t / unmasked / logp / step size mismatch: one entry per position of the logits' batch")
    u, _ = _step_noise(u, None, philox_state, n, K)
    act, nact = (None, None) if ACTIVE is None else ACTIVE
    next_input = _next_input_arg(next_input, n)
    _launch_by_temp("spk_pscore_step", temp_b, temp, (_p(logits), _p(x0), _p(x_t), _p(unmasked), int(t)),
                    (_p(u), int(seed), int(offset), _p(philox_state), _p(logp), _p(step), B, HW, K, _p(act), _p(nact),
                     _p(next_input), _stream(logits)))
    return logp, step


def _den_step_tail(what, cnt5, cnt1, packed6, x_t, unmasked, t, temp, T, K, u, q, seed, offset, philox_state, conv1, want_logits,
                   top_k, top_p, conf_outs=None, sched=None, remask=None):
    """The body of ``den_step_tail`` and its three confidence-ordered siblings (``what``: the caller's name; its entry point is
    ``spk_`` + that).  ``conf_outs``: None -- the plain family, launched by the form of its temperature, inside an ``active_set``
    scope too -- or the (x0_hat, conf) of a confidence-ordered tail; ``sched``: None or its (sched_w, S, noise_a, score);
    ``remask``: None or, with ``sched``, its (remask_r, commit_conf, mask_id, remasked)."""
    cnt5 = _dev(cnt5, "cnt5", torch.uint8)
    cnt1 = _dev(cnt1, "cnt1", torch.uint8)
    B, nch5, H, W, _ = cnt5.shape
    n = B * H * W
    images = x_t.numel() // (H * W)
    act = nact = None
    if conf_outs is None:
        top_p, top_k, temp = _topp_arg(top_p, top_k, temp, images, what, cnt5.device)
        top_k, temp = _topk_arg(top_k, temp, images, what, cnt5.device)
        temp_b, temp = (temp, None) if top_k is not None else _temp_arg(temp, images, what)
        act, nact = (None, None) if ACTIVE is None else ACTIVE
    else:
        temp_b, top_k, top_p, _ = _conf_args(temp, top_k, top_p, images, what, cnt5.device)
    if sched is not None:
        sched_w, S, noise_a, score = sched
        sched_w, noise_a, score = _sched_args(sched_w, noise_a, score, images, S, t, n, what)
    if remask is not None:
        remask = _remask_args(*remask, images, S, n, int(K), what)
    wq, scale, bias_d = packed6
    _token_state(x_t, unmasked, n, "[B,1,h,w]")
    u, q = _step_noise(u, q, philox_state, n, int(K))
    logits = torch.empty((B, K, H, W), dtype=torch.float32, device=cnt5.device) if want_logits else None
    if act is not None and conv1 is not None:
        raise ValueError(f"{what}: the fused first layer is the dense form's (inside an active_set scope pass conv1=None)")
    x1 = c1o = w1 = b1 = a1 = bb1 = None
    if conv1 is not None and int(T) != 16:
        raise NotImplementedError(f"spk_{what}: the fused first layer is the T = 16, LIFNode(tau=2, v_threshold=1, "
                                  "v_reset=0) form; run conv1 as its own launch for other step counts")
    if conv1 is not None:
        w1, b1, a1, bb1 = conv1
        x1 = empty_spikes(S32, B, 64, H, W, T, cnt5.device)
        c1o = torch.empty((B, 2, H, W, 32), dtype=torch.uint8, device=cnt5.device)
    name = "spk_" + what
    head = (_p(cnt5), int(nch5), _p(cnt1), int(cnt1.shape[1]), _p(wq), _p(scale), _p(bias_d), _p(logits), _p(x_t), _p(unmasked), int(t))
    tail = (_p(u), _p(q), int(seed), int(offset), _p(philox_state), _p(w1), _p(b1), _p(a1), _p(bb1), _p(x1), _p(c1o), int(T), B, H, W,
            int(K))
    if conf_outs is None:
        _launch_by_temp(name, temp_b, temp, head, tail + (_p(act), _p(nact), _stream(cnt5)), top_k=top_k, top_p=top_p)
    else:
        tail += (_p(_x0_hat_out(conf_outs[0], n)), _p(_conf_out(conf_outs[1], n)))
        if sched is not None:
            tail += (_p(sched_w), _p(noise_a), int(S), _p(score))
        if remask is not None:
            tail += (_p(remask[0]), _p(remask[1]), remask[2], _p(remask[3]))
        check(getattr(lib, name)(*head, _p(temp_b), _p(top_k), _p(top_p), *tail, _stream(cnt5)), name)
    return (None if x1 is None else (x1, c1o)), logits


def den_step_tail(cnt5, cnt1, packed6, x_t, unmasked, t, temp, *, T, K, u=None, q=None, seed=0, offset=0, philox_state=None,
                  conv1=None, want_logits=False, top_k=None, top_p=None):
    """The tail of one dense reverse step as one launch (spk_den_step_tail): conv6 on the spike counts + time mean, the token
    update of ``psample_step`` (x_t / unmasked in place, same noise arguments) and -- with ``conv1 = (w_packed [9,2,64], bias,
    bn_a, bn_b)`` -- the first denoiser layer of the next step.  Returns (x1 S32 [B,2,h,w,16,16], cnt1 u8 [B,2,h,w,32]) or None,
    and the logits fp32 [B,K,h,w] when asked for.  Inside an ``active_set`` scope (the untouched-image elimination) cnt5 / cnt1 / logits
    are per SLOT of the active list and x_t / unmasked / the noise per image; ``conv1`` must be None there (the next step's first layer
    belongs to the next step's active set).  ``temp``: a number or a per-image fp32 device tensor (spk_den_step_tail_temps);
    ``top_k``: int32 device tensor, one k per image, as for psample_step (spk_den_step_tail_topk); ``top_p``: fp32 device tensor,
    one p per image, as for psample_step (spk_den_step_tail_topp)."""
    return _den_step_tail("den_step_tail", cnt5, cnt1, packed6, x_t, unmasked, t, temp, T, K, u, q, seed, offset, philox_state, conv1,
                          want_logits, top_k, top_p)


def _conf_args(temp, top_k, top_p, B, what, device, listed=False):
    """The three per-image arrays of a confidence-ordered token update after the checks of the ``_topp`` siblings
    (``_topp_arg`` / ``_topk_arg``: ``top_k`` / ``top_p``, where given, are device tensors of B entries -- a number is refused as
    the siblings refuse it): a missing ``top_p`` becomes ones and a missing ``top_k`` zeros (neither truncates), a scalar ``temp``
    (> 0) is broadcast, a per-image ``temp`` is taken as given -> (temp_b, top_k, top_p, pair).  ``listed`` false: there is no
    active-list form, so inside an ``active_set`` scope the call is refused before anything is launched, and ``pair`` is None.
    ``listed`` true: the call is refused OUTSIDE a scope, and ``pair`` is the scope's (active, n_active), which
    must hold B slots and two count words."""
    if not listed and ACTIVE is not None:
        raise ValueError(f"{what}: this entry point has no active-list form (which positions change depends on the logits): call it "
                         "outside an active_set scope; the list of pending images is psample_step_conf_listed's")
    if listed and ACTIVE is None:
        raise ValueError(f"{what}: the list of pending images comes from the enclosing active_set scope "
                         f"(ops.select_pending); outside one call {what.replace('_listed', '')}")
    if listed and (ACTIVE[0].numel() < int(B) or ACTIVE[1].numel() < 2):
        raise ValueError(f"{what}: the active_set pair must hold B slots and two count words")
    B = int(B)
    # scalar or vector as ``_topk_arg`` decides it: a device tensor of B entries is per-image and never read back (B = 1 too: the
    # sampler hands its graph's one-entry buffer down, and a read-back is refused inside a capture)
    per_image = isinstance(temp, torch.Tensor) and (temp.numel() > 1 or (temp.is_cuda and temp.dim() == 1 and temp.numel() == B))
    if not per_image and not float(temp) > 0:
        raise ValueError(f"{what}: temp must be > 0 (what the scalar entry points check), got {float(temp)}")
    if top_p is None:
        top_p = torch.ones(B, dtype=torch.float32, device=device)
    top_p, top_k, temp = _topp_arg(top_p, top_k, temp, B, what, device)
    top_k, temp_b = _topk_arg(top_k, temp, B, what, device)
    return temp_b, top_k, top_p, (ACTIVE if listed else None)


def _conf_out(conf, n):
    if conf is not None and (not isinstance(conf, torch.Tensor) or conf.dtype != torch.float32 or not conf.is_cuda or
                             not conf.is_contiguous() or conf.numel() != n):
        raise ValueError("conf must be a contiguous fp32 device tensor with one entry per position (written where a position is masked)")
    return conf


def _x0_hat_out(x0_hat, n):
    if x0_hat is not None and (not isinstance(x0_hat, torch.Tensor) or x0_hat.dtype != torch.int64 or not x0_hat.is_cuda or
                               not x0_hat.is_contiguous() or x0_hat.numel() != n):
        raise ValueError("x0_hat must be a contiguous int64 device tensor with one entry per position (written where a position is masked)")
    return x0_hat


def _psample_conf(what, logits, x_t, unmasked, t, temp, u, q, seed, offset, x0_hat, conf, philox_state, top_k, top_p, next_input=None,
                  listed=None, sched=None, remask=None):
    """The body of the six ``psample_step_conf*`` wrappers (``what``: the caller's name; its entry point is ``spk_`` + that).
    ``listed``: None -- the dense form, which may write ``next_input`` -- or the (steps_b, S, step_stride) of the update on the list
    of the enclosing ``active_set`` scope, whose logits lie by slot; ``sched``: None or (sched_w, S, noise_a, score); ``remask``:
    None or, with ``sched``, (remask_r, commit_conf, mask_id, remasked)."""
    logits = _dev(logits, "logits", torch.float32)
    B, K = logits.shape[0], logits.shape[1]
    HW = logits[0, 0].numel()
    n = B * HW
    images = x_t.numel() // HW
    temp_b, top_k, top_p, pair = _conf_args(temp, top_k, top_p, images, what, logits.device, listed=listed is not None)
    if listed is None:
        offset, tail = int(offset), (_p(_next_input_arg(next_input, n)),)
    else:
        if B != images:
            raise ValueError(f"{what}: logits hold one slot per image of the batch ({images}), got {B}")
        steps_b, S, step_stride = _steps_arg(listed[0], B, what), int(listed[1]), int(listed[2])
        if not 1 <= int(t) <= S or step_stride < 0:
            raise ValueError(f"{what}: 1 <= t <= S and step_stride >= 0, got t = {int(t)}, S = {S}, stride {step_stride}")
        offset, tail = int(offset) & 0xFFFFFFFFFFFFFFFF, (_p(steps_b), S, step_stride, _p(pair[0]), _p(pair[1]))
    if sched is not None:
        sched_w, S, noise_a, score = sched
        sched_w, noise_a, score = _sched_args(sched_w, noise_a, score, images, S, t, n, what)
    if remask is not None:
        remask = _remask_args(*remask, images, S, n, K, what)
    _token_state(x_t, unmasked, n, "(updated in place)")
    u, q = _step_noise(u, q, philox_state, n, K)
    if sched is not None:                           # (the listed form has its S among the list's arguments)
        tail += (_p(sched_w), _p(noise_a), int(S), _p(score)) if listed is None else (_p(sched_w), _p(noise_a), _p(score))
    if remask is not None:
        tail += (_p(remask[0]), _p(remask[1]), remask[2], _p(remask[3]))
    name = "spk_" + what
    check(getattr(lib, name)(_p(logits), _p(x_t), _p(unmasked), int(t), _p(temp_b), _p(top_k), _p(top_p), _p(u), _p(q), int(seed),
                             offset, _p(philox_state), _p(_x0_hat_out(x0_hat, n)), _p(_conf_out(conf, n)), B, HW, K, *tail,
                             _stream(logits)), name)
    return x_t, unmasked


def psample_step_conf(logits, x_t, unmasked, t, temp=1.0, u=None, q=None, seed=0, offset=0, x0_hat=None, conf=None,
                      philox_state=None, next_input=None, top_k=None, top_p=None):
    """``psample_step`` under the confidence-ordered reveal (spk_psample_step_conf): every position masked at entry
    draws the candidate ``psample_step(..., top_k, top_p, x0_hat=)`` reports for it, and the ceil(m / t) candidates of each image
    with the largest log-probability (ties to the lower position) are committed; x_t / unmasked in place.  ``x0_hat`` (int64) /
    ``conf`` (fp32): optional outputs, written at the masked positions only.  ``u`` is accepted and ignored (the coin is not part
    of the rule).  ``temp`` / ``top_k`` / ``top_p`` as for psample_step: ``top_k`` (int32) and ``top_p`` (fp32) are device
    tensors with one entry per image or None, ``temp`` a number or such a tensor.  The entry point takes all three per image, so a
    scalar ``temp`` is broadcast and a missing truncation becomes k = 0 / p = 1 everywhere.  Not inside an ``active_set`` scope; h * w <= 64."""
    return _psample_conf("psample_step_conf", logits, x_t, unmasked, t, temp, u, q, seed, offset, x0_hat, conf, philox_state, top_k,
                         top_p, next_input)


def _steps_arg(steps_b, B, what):
    """``steps_b`` of the per-image confidence-ordered calls: a contiguous int32 device tensor with one step count
    per image of the call (index = image), taken as given."""
    B = int(B)
    if (not isinstance(steps_b, torch.Tensor) or steps_b.dtype != torch.int32 or not steps_b.is_cuda or not steps_b.is_contiguous() or
            steps_b.dim() != 1 or steps_b.numel() != B):
        got = f"{steps_b.dtype} {tuple(steps_b.shape)} on '{steps_b.device}'" if isinstance(steps_b, torch.Tensor) else repr(type(steps_b))
        raise ValueError(f"{what}: steps_b must be a contiguous int32 device tensor of B = {B} entries, got {got}")
    return steps_b


def select_pending(unmasked, t, steps_b, out=None):
    """Images PENDING at reverse step t of per-image confidence-ordered decoding (spk_select_pending): those with
    t <= steps_b[i] and at least one masked position.  Returns select_active's pair (active int32 [B] ascending image list, n_active
    int32 [2]: count and a work word) on the device -- a drop-in for ``active_set``; no noise is drawn.  h * w <= 64."""
    if unmasked.dtype not in (torch.bool, torch.uint8) or not unmasked.is_cuda or not unmasked.is_contiguous():
        raise ValueError("unmasked must be a contiguous bool/uint8 device tensor")
    B = unmasked.shape[0]
    HW = unmasked[0].numel()
    steps_b = _steps_arg(steps_b, B, "select_pending")
    if out is None:
        out = (torch.empty(B, dtype=torch.int32, device=unmasked.device),
               torch.zeros(2, dtype=torch.int32, device=unmasked.device))     # [count, work word (zero between calls)]
    elif out[0].numel() < B or out[1].numel() < 2:
        raise ValueError("out = (active int32 [B], n_active int32 [2]: count, work word (zero before the first call))")
    check(lib.spk_select_pending(_p(unmasked), int(t), _p(steps_b), _p(out[0]), _p(out[1]), B, HW, _stream(unmasked)),
          "spk_select_pending")
    return out


def psample_step_conf_listed(logits, x_t, unmasked, t, temp, steps_b, S, step_stride, u=None, q=None, seed=0, offset=0, x0_hat=None,
                             conf=None, philox_state=None, top_k=None, top_p=None):
    """``psample_step_conf`` on the list of the enclosing ``active_set`` scope (spk_psample_step_conf_listed; refused
    outside one): ``logits`` [B,K,h,w] hold one SLOT per listed image, everything else -- x_t / unmasked, ``temp`` / ``top_k`` /
    ``top_p``, ``steps_b`` (int32 device tensor, one step count per image), the noise, ``x0_hat`` / ``conf`` -- is indexed by image.
    A listed image takes psample_step_conf's update at this ``t`` with the noise of its own run of e = min(steps_b[i], S) steps:
    counters at ``offset - (S - e) * step_stride`` (``S``: the loop's step count, ``step_stride``: its counters per step);
    images off the list keep their state.  No ``next_input``: the listed form gathers its denoiser input by slot."""
    return _psample_conf("psample_step_conf_listed", logits, x_t, unmasked, t, temp, u, q, seed, offset, x0_hat, conf, philox_state,
                         top_k, top_p, listed=(steps_b, S, step_stride))


def den_step_tail_conf(cnt5, cnt1, packed6, x_t, unmasked, t, temp, *, T, K, u=None, q=None, seed=0, offset=0, philox_state=None,
                       conv1=None, want_logits=False, top_k=None, top_p=None, x0_hat=None, conf=None):
    """``den_step_tail`` under the confidence-ordered reveal (spk_den_step_tail_conf): conv6 on the counts, the token update of
    ``psample_step_conf`` and -- with ``conv1`` -- the next step's first layer on the committed tokens, one launch.  Same
    arguments, checks and results as den_step_tail, plus the optional outputs ``x0_hat`` / ``conf`` of psample_step_conf; not
    inside an ``active_set`` scope."""
    return _den_step_tail("den_step_tail_conf", cnt5, cnt1, packed6, x_t, unmasked, t, temp, T, K, u, q, seed, offset, philox_state,
                          conv1, want_logits, top_k, top_p, conf_outs=(x0_hat, conf))


def _sched_args(sched_w, noise_a, score, B, S, t, n, what):
    """The tables of a ``_sched`` token update: ``sched_w`` a contiguous int32 device tensor [B, S + 1]
    (the entry points read uint32: weights 0 .. 2^24 have the same bits in both), ``noise_a`` None or contiguous fp32 [B, S + 1] on the
    device, both taken as given; ``score`` None or fp32 with one entry per position; 1 <= t <= S."""
    B, S = int(B), int(S)
    if S < 1 or not 1 <= int(t) <= S:
        raise ValueError(f"{what}: 1 <= t <= S, got t = {int(t)}, S = {S}")
    if (not isinstance(sched_w, torch.Tensor) or sched_w.dtype != torch.int32 or not sched_w.is_cuda or
            not sched_w.is_contiguous() or tuple(sched_w.shape) != (B, S + 1)):
        got = f"{sched_w.dtype} {tuple(sched_w.shape)} on '{sched_w.device}'" if isinstance(sched_w, torch.Tensor) else repr(type(sched_w))
        raise ValueError(f"{what}: sched_w must be a contiguous int32 device tensor [B = {B}, S + 1 = {S + 1}], got {got}")
    if noise_a is not None and (not isinstance(noise_a, torch.Tensor) or noise_a.dtype != torch.float32 or not noise_a.is_cuda or
                                not noise_a.is_contiguous() or tuple(noise_a.shape) != (B, S + 1)):
        got = f"{noise_a.dtype} {tuple(noise_a.shape)} on '{noise_a.device}'" if isinstance(noise_a, torch.Tensor) else repr(type(noise_a))
        raise ValueError(f"{what}: noise_a must be None or a contiguous fp32 device tensor [B = {B}, S + 1 = {S + 1}], got {got}")
    if score is not None and (not isinstance(score, torch.Tensor) or score.dtype != torch.float32 or not score.is_cuda or
                              not score.is_contiguous() or score.numel() != n):
        raise ValueError(f"{what}: score must be a contiguous fp32 device tensor with one entry per position (written where a position is masked)")
    return sched_w, noise_a, score


def psample_step_conf_sched(logits, x_t, unmasked, t, temp, sched_w, S, noise_a=None, u=None, q=None, seed=0, offset=0, x0_hat=None,
                            conf=None, score=None, philox_state=None, next_input=None, top_k=None, top_p=None):
    """``psample_step_conf`` under a reveal schedule and annealed selection noise (spk_psample_step_conf_sched):
    the count of image i at step ``t`` comes from row i of ``sched_w`` (int32 [B, S + 1] on the device; spkdiff.schedules
    builds rows), the order from score = conf + noise_a[i][t] * g with g the Gumbel of the position's stream-0 uniform (``noise_a``:
    fp32 [B, S + 1] on the device or None = no noise; ``u``, where injected, IS that uniform).  ``score``: optional fp32 output, at
    the masked positions.  Candidates, ``x0_hat`` and ``conf`` are psample_step_conf's bit for bit.  Every other argument is the
    sibling's."""
    return _psample_conf("psample_step_conf_sched", logits, x_t, unmasked, t, temp, u, q, seed, offset, x0_hat, conf, philox_state,
                         top_k, top_p, next_input, sched=(sched_w, S, noise_a, score))


def psample_step_conf_listed_sched(logits, x_t, unmasked, t, temp, steps_b, S, step_stride, sched_w, noise_a=None, u=None, q=None,
                                   seed=0, offset=0, x0_hat=None, conf=None, score=None, philox_state=None, top_k=None, top_p=None):
    """``psample_step_conf_listed`` under a reveal schedule and annealed selection noise (spk_psample_step_conf_listed_sched;
    DESIGN.md §4.17): the tables of psample_step_conf_sched, indexed by image and by the loop's ``t``; a listed image draws its
    Gumbel uniform at its own shifted counters, as it draws its race noise.  Every other argument is the sibling's."""
    return _psample_conf("psample_step_conf_listed_sched", logits, x_t, unmasked, t, temp, u, q, seed, offset, x0_hat, conf,
                         philox_state, top_k, top_p, listed=(steps_b, S, step_stride), sched=(sched_w, S, noise_a, score))


def den_step_tail_conf_sched(cnt5, cnt1, packed6, x_t, unmasked, t, temp, sched_w, S, *, T, K, noise_a=None, u=None, q=None, seed=0,
                             offset=0, philox_state=None, conv1=None, want_logits=False, top_k=None, top_p=None, x0_hat=None,
                             conf=None, score=None):
    """``den_step_tail_conf`` under a reveal schedule and annealed selection noise (spk_den_step_tail_conf_sched):
    conv6 on the counts, the token update of ``psample_step_conf_sched`` and -- with ``conv1`` -- the next step's first layer, one
    launch.  The sibling's arguments, checks and results plus the tables and the optional ``score`` of psample_step_conf_sched."""
    return _den_step_tail("den_step_tail_conf_sched", cnt5, cnt1, packed6, x_t, unmasked, t, temp, T, K, u, q, seed, offset,
                          philox_state, conv1, want_logits, top_k, top_p, conf_outs=(x0_hat, conf), sched=(sched_w, S, noise_a, score))


def _remask_args(remask_r, commit_conf, mask_id, remasked, B, S, n, K, what):
    """The added arguments of a ``_remask`` token update: ``remask_r`` a contiguous int32 device tensor [B, S + 1]
    (the entry points read uint32: counts >= 0 have the same bits in both), ``commit_conf`` a contiguous fp32 device tensor with one
    entry per position (read and written in place), both taken as given; ``mask_id`` an integer outside [0, K); ``remasked`` None
    or a contiguous uint8 / bool device tensor with one entry per position."""
    B, S = int(B), int(S)
    if (not isinstance(remask_r, torch.Tensor) or remask_r.dtype != torch.int32 or not remask_r.is_cuda or
            not remask_r.is_contiguous() or tuple(remask_r.shape) != (B, S + 1)):
        got = f"{remask_r.dtype} {tuple(remask_r.shape)} on '{remask_r.device}'" if isinstance(remask_r, torch.Tensor) else repr(type(remask_r))
        raise ValueError(f"{what}: remask_r must be a contiguous int32 device tensor [B = {B}, S + 1 = {S + 1}], got {got}")
    if (not isinstance(commit_conf, torch.Tensor) or commit_conf.dtype != torch.float32 or not commit_conf.is_cuda or
            not commit_conf.is_contiguous() or commit_conf.numel() != n):
        raise ValueError(f"{what}: commit_conf must be a contiguous fp32 device tensor with one entry per position (updated in place)")
    if isinstance(mask_id, bool) or not hasattr(mask_id, "__index__") or 0 <= mask_id.__index__() < int(K):
        raise ValueError(f"{what}: mask_id is an integer outside the classes 0 .. K - 1 = {int(K) - 1}, got {mask_id!r}")
    if remasked is not None and (not isinstance(remasked, torch.Tensor) or remasked.dtype not in (torch.uint8, torch.bool) or
                                 not remasked.is_cuda or not remasked.is_contiguous() or remasked.numel() != n):
        raise ValueError(f"{what}: remasked must be a contiguous uint8 / bool device tensor with one entry per position")
    return remask_r, commit_conf, mask_id.__index__(), remasked


def psample_step_conf_remask(logits, x_t, unmasked, t, temp, sched_w, S, remask_r, commit_conf, mask_id, noise_a=None, u=None, q=None,
                             seed=0, offset=0, x0_hat=None, conf=None, score=None, remasked=None, philox_state=None, next_input=None,
                             top_k=None, top_p=None):
    """``psample_step_conf_sched`` with remasking (spk_psample_step_conf_remask): after the reveal, the
    min(remask_r[i][t], c) least trusted of image i's c earlier commits -- those with the smallest ``commit_conf``, ties to the higher
    position; positions holding +inf, the tokens the run started with, are never revisited -- return to the masked state (x_t =
    ``mask_id``, unmasked = 0) and draw again at the next step; nothing is remasked at t = 1.  ``commit_conf`` (fp32, one entry per
    position, in place) receives the confidence of every position this step reveals; ``remask_r``: int32 [B, S + 1] on the device
    (spkdiff.schedules.remask_row builds rows); ``remasked``: optional uint8 output, 1 where this step remasked (written for the
    images with a masked position at entry).  The reveal and ``x0_hat`` / ``conf`` / ``score`` are the sibling's bit for bit."""
    return _psample_conf("psample_step_conf_remask", logits, x_t, unmasked, t, temp, u, q, seed, offset, x0_hat, conf, philox_state,
                         top_k, top_p, next_input, sched=(sched_w, S, noise_a, score), remask=(remask_r, commit_conf, mask_id, remasked))


def psample_step_conf_listed_remask(logits, x_t, unmasked, t, temp, steps_b, S, step_stride, sched_w, remask_r, commit_conf, mask_id,
                                    noise_a=None, u=None, q=None, seed=0, offset=0, x0_hat=None, conf=None, score=None, remasked=None,
                                    philox_state=None, top_k=None, top_p=None):
    """``psample_step_conf_listed_sched`` with remasking (spk_psample_step_conf_listed_remask): the added arguments
    of psample_step_conf_remask, all indexed by image; an image off the list, or with t above its own step count, is left as it is,
    ``commit_conf`` included."""
    return _psample_conf("psample_step_conf_listed_remask", logits, x_t, unmasked, t, temp, u, q, seed, offset, x0_hat, conf,
                         philox_state, top_k, top_p, listed=(steps_b, S, step_stride), sched=(sched_w, S, noise_a, score),
                         remask=(remask_r, commit_conf, mask_id, remasked))


def den_step_tail_conf_remask(cnt5, cnt1, packed6, x_t, unmasked, t, temp, sched_w, S, remask_r, commit_conf, mask_id, *, T, K,
                              noise_a=None, u=None, q=None, seed=0, offset=0, philox_state=None, conv1=None, want_logits=False,
                              top_k=None, top_p=None, x0_hat=None, conf=None, score=None, remasked=None):
    """``den_step_tail_conf_sched`` with remasking (spk_den_step_tail_conf_remask): conv6 on the counts, the token
    update of ``psample_step_conf_remask`` and -- with ``conv1`` -- the next step's first layer, which reads ``mask_id`` at a
    remasked position; one launch.  The sibling's arguments, checks and results plus the added ones of psample_step_conf_remask."""
    return _den_step_tail("den_step_tail_conf_remask", cnt5, cnt1, packed6, x_t, unmasked, t, temp, T, K, u, q, seed, offset,
                          philox_state, conv1, want_logits, top_k, top_p, conf_outs=(x0_hat, conf), sched=(sched_w, S, noise_a, score),
                          remask=(remask_r, commit_conf, mask_id, remasked))


def q_sample(x_0, t, u, num_timesteps, mask_id):
    """(x_t, x_0_ignore, mask) of R/snn_model/vq_diffusion.py:61-75 from x_0 fp32 [B,1,h,w], t int64 [B] and the uniforms u
    (spk_q_sample: one launch)."""
    x0 = _dev(x_0, "x_0", torch.float32)
    uu = _dev(u, "u", torch.float32)
    tt = t.contiguous()
    if tt.dtype != torch.int64 or not tt.is_cuda:
        raise ValueError("t must be an int64 device tensor")
    B = int(x0.shape[0])
    HW = x0[0].numel()
    x_t, ign = torch.empty_like(x0), torch.empty_like(x0)
    mask = torch.empty(x0.shape, dtype=torch.bool, device=x0.device)
    check(lib.spk_q_sample(_p(x0), _p(tt), _p(uu), _p(x_t), _p(ign), _p(mask), B, HW, int(num_timesteps), float(mask_id),
                           _stream(x0)), "spk_q_sample")
    return x_t, ign, mask


def philox_noise(seed, offset, B, HW, K, device, philox_state=None, want_q=True):
    """The (u [B*HW], q [B*HW, K]) a Philox-mode reverse step with these (seed, offset, philox_state) arguments draws
    (spk_philox_noise): parity aid -- the oracle run on the dumped noise must reproduce the Philox-mode tokens."""
    u = torch.empty(B * HW, dtype=torch.float32, device=device)
    q = torch.empty((B * HW, K), dtype=torch.float32, device=device) if want_q else None
    check(lib.spk_philox_noise(int(seed), int(offset), _p(philox_state), _p(u), _p(q), int(B), int(HW), int(K), _stream(u)),
          "spk_philox_noise")
    return u, q


def _keep_u8(keep, name):
    """A bool / uint8 device mask as the contiguous uint8 bytes the kernels read (a view: no copy for a contiguous mask)."""
    if not isinstance(keep, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(keep)}")
    if keep.dtype not in (torch.bool, torch.uint8):
        raise NotImplementedError(f"spkdiff: {name} must be bool or uint8, got {keep.dtype}")
    keep = _dev(keep, name)
    return keep.view(torch.uint8) if keep.dtype == torch.bool else keep


def completion_state(codes, keep, K, mask_id, stride=1, radius=0, out=None, want_counts=False):
    """Start state of a conditional reverse process (spk_completion_state): ``codes`` int64 [B,h,w] or [B,1,h,w], ``keep``
    bool / uint8 [B,Hm,Wm] or [B,1,Hm,Wm] (true = given) -> (x_t int64 [B,1,h,w], unmasked bool [B,1,h,w], n_known int32 [B] or
    None).  Token (i,j) is known iff every mask byte within ``radius`` of (stride*i, stride*j), clipped to the mask, is set and
    the code is inside [0, K); x_t holds ``mask_id`` elsewhere.  (1, 0): a latent-resolution mask; (4, 3): a pixel mask seen
    through the encoder's receptive field.  ``out``: (x_t, unmasked) buffers to write (a captured graph's)."""
    if not isinstance(codes, torch.Tensor) or not isinstance(keep, torch.Tensor):
        raise TypeError(f"codes and keep must be torch.Tensors, got {type(codes)} and {type(keep)}")
    if keep.dtype not in (torch.bool, torch.uint8):
        raise NotImplementedError(f"spkdiff: keep must be bool or uint8, got {keep.dtype}")
    codes = _dev(codes, "codes", torch.int64)
    keep = _keep_u8(keep, "keep")
    if codes.dim() == 4 and codes.shape[1] == 1:
        codes = codes[:, 0]
    if keep.dim() == 4 and keep.shape[1] == 1:
        keep = keep[:, 0]
    if codes.dim() != 3 or keep.dim() != 3 or keep.shape[0] != codes.shape[0]:
        raise ValueError(f"completion_state: codes {tuple(codes.shape)} must be [B,h,w] and keep {tuple(keep.shape)} [B,Hm,Wm] "
                         "with the same B")
    if keep.device != codes.device:
        raise ValueError("completion_state: codes and keep must be on one device")
    B, h, w = (int(v) for v in codes.shape)
    Hm, Wm = int(keep.shape[1]), int(keep.shape[2])
    if out is None:
        x_t = torch.empty((B, 1, h, w), dtype=torch.int64, device=codes.device)
        unmasked = torch.empty((B, 1, h, w), dtype=torch.bool, device=codes.device)
    else:
        x_t, unmasked = out
        if not (x_t.is_cuda and x_t.device == codes.device and x_t.dtype == torch.int64 and x_t.is_contiguous()
                and x_t.numel() == B * h * w):
            raise ValueError("completion_state: out[0] must be a contiguous int64 device tensor [B,1,h,w]")
        if not (unmasked.is_cuda and unmasked.device == codes.device and unmasked.dtype in (torch.bool, torch.uint8)
                and unmasked.is_contiguous() and unmasked.numel() == B * h * w):
            raise ValueError("completion_state: out[1] must be a contiguous bool/uint8 device tensor [B,1,h,w]")
    n_known = torch.empty(B, dtype=torch.int32, device=codes.device) if want_counts else None
    check(lib.spk_completion_state(_p(codes.contiguous()), _p(keep.contiguous()), _p(x_t), _p(unmasked), _p(n_known), B, h, w,
                                   Hm, Wm, int(stride), int(radius), int(K), int(mask_id), _stream(codes)), "spk_completion_state")
    return x_t, unmasked, n_known


def completion_compose(images, keep, decoded_u8):
    """Given pixels pasted over a decoded image (spk_completion_compose): ``images`` fp32 [B,C,H,W] normalised (pixel - 0.5),
    ``keep`` bool / uint8 [B,H,W] or [B,1,H,W], ``decoded_u8`` uint8 [B,C,H,W] -> uint8 [B,C,H,W]:
    keep ? uint8(clip(image + 0.5, 0, 1) * 255) : decoded_u8."""
    images = _dev(images, "images", torch.float32)
    keep = _keep_u8(keep, "keep")
    decoded_u8 = _dev(decoded_u8, "decoded_u8", torch.uint8)
    if keep.dim() == 4 and keep.shape[1] == 1:
        keep = keep[:, 0]
    if images.dim() != 4 or decoded_u8.shape != images.shape:
        raise ValueError(f"completion_compose: images {tuple(images.shape)} and decoded_u8 {tuple(decoded_u8.shape)} must be "
                         "equal [B,C,H,W] shapes")
    B, C, H, W = (int(v) for v in images.shape)
    if tuple(keep.shape) != (B, H, W):
        raise ValueError(f"completion_compose: keep {tuple(keep.shape)} must be [{B},{H},{W}] (or [B,1,H,W])")
    if keep.device != images.device or decoded_u8.device != images.device:
        raise ValueError("completion_compose: images, keep and decoded_u8 must be on one device")
    out = torch.empty((B, C, H, W), dtype=torch.uint8, device=images.device)
    check(lib.spk_completion_compose(_p(images), _p(keep.contiguous()), _p(decoded_u8), _p(out), B, C, H, W, _stream(images)),
          "spk_completion_compose")
    return out


class TensorChecksum:
    """Content checksum of a fixed set of device tensors in one launch (spk_checksum_multi): ``value()`` synchronises."""

    @staticmethod
    def select(tensors):
        """The tensors a checksum covers: device tensors whose numel * itemsize bytes from data_ptr are exactly their
        elements in SOME order (default or channels-last memory: the sum does not depend on the order)."""
        out = []
        for t in tensors:
            if t is None or not t.is_cuda or t.numel() == 0:
                continue
            dense = t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))
            if dense:
                out.append(t)
        return out

    @staticmethod
    def key_of(tensors):
        return tuple((t.data_ptr(), t.numel() * t.element_size()) for t in TensorChecksum.select(tensors))

    def __init__(self, tensors):
        ts = self.select(tensors)
        if not ts:
            raise ValueError("TensorChecksum: no device tensors")
        self.key = tuple((t.data_ptr(), t.numel() * t.element_size()) for t in ts)
        dev = ts[0].device
        tab = []
        for t in ts:
            nb = t.numel() * t.element_size()
            if nb % 4 or t.data_ptr() % 4:
                raise NotImplementedError("TensorChecksum: tensors must be whole 4-byte words")
            tab += [t.data_ptr(), nb // 4]
        self.table = torch.tensor(tab, dtype=torch.int64).to(dev)
        self.out = torch.zeros(1, dtype=torch.int64, device=dev)
        self.n = len(ts)
        self._keep = ts

    def value(self):
        check(lib.spk_checksum_multi(_p(self.table), self.n, _p(self.out), _stream(self.out)), "spk_checksum_multi")
        return int(self.out.item())


class NeedLists:
    """Device buffer of spk_select_needed for ``batch`` image slots and ``radii`` layer depths (zero-initialised once)."""
    __slots__ = ("buf", "batch", "radii")

    def __init__(self, batch, radii, device):
        n = lib.spk_select_needed_bytes(int(batch), int(radii))
        if n <= 0:
            raise ValueError("spk_select_needed_bytes: bad (batch, radii)")
        self.buf = torch.zeros(n, dtype=torch.uint8, device=device)
        self.batch, self.radii = int(batch), int(radii)

    def records(self, radius):
        """uint8 [B, 64] view of the records of one radius (tests)."""
        R, B = self.radii, self.batch
        lists = 64 + R * 64 + R * 6 * B * 4
        off = (lists + 63) // 64 * 64 + (radius - 1) * B * 64
        return self.buf[off:off + B * 64].view(B, 64)


def select_needed(unmasked, t, active, need, u=None, seed=0, offset=0, philox_state=None, K=128):
    """Positions each active image needs from the layers below the logits at reverse step t (spk_select_needed); ``active``
    = the pair returned by select_active for the same step, ``need`` a NeedLists for the same batch.  7x7 latents.  ``K``:
    the class count of the step's psample_step call (the stride of the Philox counter layout; unused with injected u)."""
    B = unmasked.shape[0]
    H, W = int(unmasked.shape[-2]), int(unmasked.shape[-1])
    if need.batch != B:
        raise ValueError("NeedLists was sized for another batch")
    if u is not None:
        u = _dev(u, "u", torch.float32)
    check(lib.spk_select_needed(_p(unmasked), int(t), _p(u), int(seed), int(offset), _p(philox_state), _p(active[0]),
                                _p(active[1]), _p(need.buf), B, H, W, need.radii, int(K), _stream(unmasked)), "spk_select_needed")
    return need


def select_active(unmasked, t, u=None, seed=0, offset=0, philox_state=None, out=None, K=128):
    """Images that reverse step t touches (at least one position with u < 1/t still masked): returns (active int32 [B]
    ascending image list, n_active int32 [2]: count and a work word) on the device; same u / Philox arguments as psample_step
    (``K``: that call's class count, the stride of the Philox counter layout; unused with injected u)."""
    if unmasked.dtype not in (torch.bool, torch.uint8) or not unmasked.is_cuda or not unmasked.is_contiguous():
        raise ValueError("unmasked must be a contiguous bool/uint8 device tensor")
    B = unmasked.shape[0]
    HW = unmasked[0].numel()
    if u is not None:
        u = _dev(u, "u", torch.float32)
    if out is None:
        out = (torch.empty(B, dtype=torch.int32, device=unmasked.device),
               torch.zeros(2, dtype=torch.int32, device=unmasked.device))     # [count, work word (zero between calls)]
    elif out[1].numel() < 2:
        raise ValueError("n_active needs two int32 words: [count, work word (zero before the first call)]")
    check(lib.spk_select_active(_p(unmasked), int(t), _p(u), int(seed), int(offset), _p(philox_state), _p(out[0]),
                                _p(out[1]), B, HW, int(K), _stream(unmasked)), "spk_select_active")
    return out


# ---------------------------------------------------------------------------------------------- SNN_VAE spiking MLP
LIN_IN_F32, LIN_IN_U8, LIN_IN_PTC = (_C["SPK_LIN_IN_" + n] for n in ("F32", "U8", "PTC"))
LIN_OUT_F32, LIN_OUT_U8, LIN_OUT_PTC = (_C["SPK_LIN_OUT_" + n] for n in ("F32", "U8", "PTC"))


def _linear_params(weight, bias, n_in):
    w = _dev(weight, "weight", torch.float32)
    if w.dim() != 2 or w.shape[1] != n_in:
        raise ValueError(f"weight must be [out, {n_in}], got {tuple(w.shape)}")
    b = None if bias is None else _dev(bias, "bias", torch.float32)
    if b is not None and b.shape != (w.shape[0],):
        raise ValueError(f"bias must be [{w.shape[0]}], got {tuple(b.shape)}")
    return w, b


def linear(x: torch.Tensor, weight: torch.Tensor, bias=None):
    """layer.Linear's currents: x fp32 [N, in] -> fp32 [N, out] = x @ weight.T + bias (spk_linear_lif_fwd, LIN_OUT_F32);
    each output an fp32 sum over the inputs in ascending order, then + bias."""
    x = _dev(x, "x", torch.float32)
    if x.dim() != 2:
        raise ValueError(f"x must be [N, in], got {tuple(x.shape)}")
    w, b = _linear_params(weight, bias, x.shape[1])
    out = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
    if x.shape[0] == 0:
        return out
    check(lib.spk_linear_lif_fwd(_p(x), LIN_IN_F32, _p(w), _p(b), None, _p(out), LIN_OUT_F32, 1, x.shape[0], x.shape[1],
                                 w.shape[0], 0, 0, 0, _stream(x)), "spk_linear_lif_fwd")
    return out


def linear_lif(x: torch.Tensor, weight: torch.Tensor, bias, v: torch.Tensor, out_ptc=None, want_out=True):
    """Multi-step Linear + default LIFNode (tau 2, v_th 1, hard reset 0), spk_linear_lif_fwd.

    x: fp32 [T,B,in] (any values), u8/bool [T,B,in] (spikes), or u8 PTC [B,H,W,T,C] (spikes, in = C*H*W read in
    flatten(C,H,W) order).  v: fp32 [B,out], updated in place.  Returns u8 spikes [T,B,out], or with ``out_ptc=(C,H,W)``
    u8 PTC [B,H,W,T,C] (out = C*H*W); ``want_out=False``: state-only pass, returns None."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    x = _dev(x, "x")
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    if x.dtype == torch.float32 and x.dim() == 3:
        in_kind, (T, B, n_in), pc = LIN_IN_F32, x.shape, (0, 0, 0)
    elif x.dtype == torch.uint8 and x.dim() == 3:
        in_kind, (T, B, n_in), pc = LIN_IN_U8, x.shape, (0, 0, 0)
    elif x.dtype == torch.uint8 and x.dim() == 5:
        B, H, W, T, C = x.shape
        in_kind, n_in, pc = LIN_IN_PTC, C * H * W, (C, H, W)
    else:
        raise ValueError(f"x must be fp32/u8 [T,B,in] or u8 PTC [B,H,W,T,C], got {x.dtype} {tuple(x.shape)}")
    w, b = _linear_params(weight, bias, n_in)
    n_out = w.shape[0]
    v = _dev(v, "v", torch.float32)
    if v.shape != (B, n_out):
        raise ValueError(f"v must be [{B}, {n_out}], got {tuple(v.shape)}")
    out = None
    if out_ptc is not None:
        if in_kind == LIN_IN_PTC:
            raise NotImplementedError("spkdiff: PTC input and PTC output in one call")
        C, H, W = out_ptc
        if C * H * W != n_out:
            raise ValueError(f"out_ptc {tuple(out_ptc)} does not hold {n_out} outputs")
        out_kind, pc = LIN_OUT_PTC, (C, H, W)
        out = empty_spikes(PTC, B, C, H, W, T, x.device)
    else:
        out_kind = LIN_OUT_U8
        if want_out:
            out = torch.empty((T, B, n_out), dtype=torch.uint8, device=x.device)
    check(lib.spk_linear_lif_fwd(_p(x), in_kind, _p(w), _p(b), _p(v), _p(out), out_kind, T, B, n_in, n_out, *pc,
                                 _stream(x)), "spk_linear_lif_fwd")
    return out


def svae_ar(x, z0, layers, vs, idx, want_q_z=False):
    """One autoregressive loop of the SNN_VAE latent model in one launch (spk_svae_ar_fwd).

    x: u8/bool spikes [T,B,cx] -> PosteriorBernoulliSTBP.forward; None -> PriorBernoulliSTBP.sample (B from idx).
    z0: initial_input ([1,1,cz] or [cz]); layers: ((w1, b1), (w2, b2), (w3, b3)) with w3 [cz*k, h2]; vs: the three layers'
    v, fp32 [B,h], updated in place; idx: [T,B,cz] integer draws in [0,k).  Returns (sampled_z fp32 [T,B,cz],
    q_z u8 [T,B,cz*k] of the final posterior pass, or None)."""
    idx = _dev(idx, "idx")
    if idx.dim() != 3 or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"idx must be an integer [T,B,cz] tensor, got {idx.dtype} {tuple(idx.shape)}")
    T, B, cz = idx.shape
    if x is not None:
        x = _dev(x, "x")
        if x.dtype == torch.bool:
            x = x.view(torch.uint8)
        if x.dtype != torch.uint8 or x.dim() != 3 or x.shape[:2] != (T, B):
            raise ValueError(f"x must be u8 spikes [{T}, {B}, cx], got {x.dtype} {tuple(x.shape)}")
        cx = x.shape[2]
    else:
        cx = 0
        if want_q_z:
            raise ValueError("q_z belongs to the posterior (x given)")
    z0 = _dev(z0, "initial_input", torch.float32)
    if z0.numel() != cz:
        raise ValueError(f"initial_input has {z0.numel()} elements, expected {cz}")
    (w1, b1), (w2, b2), (w3, b3) = layers
    w1, b1 = _linear_params(w1, b1, cx + cz)
    h1 = w1.shape[0]
    w2, b2 = _linear_params(w2, b2, h1)
    h2 = w2.shape[0]
    w3, b3 = _linear_params(w3, b3, h2)
    h3 = w3.shape[0]
    if h3 % cz:
        raise ValueError(f"last layer has {h3} outputs, not a multiple of {cz} channels")
    k = h3 // cz
    bs = [torch.zeros(w.shape[0], dtype=torch.float32, device=w.device) if bb is None else bb
          for w, bb in ((w1, b1), (w2, b2), (w3, b3))]
    v1, v2, v3 = (_dev(v, "v", torch.float32) for v in vs)
    for v, h in ((v1, h1), (v2, h2), (v3, h3)):
        if v.shape != (B, h):
            raise ValueError(f"v must be [{B}, {h}], got {tuple(v.shape)}")
    idx32 = idx if idx.dtype == torch.int32 else idx.to(torch.int32)
    z = torch.empty((T, B, cz), dtype=torch.float32, device=idx.device)
    q = torch.empty((T, B, h3), dtype=torch.uint8, device=idx.device) if want_q_z else None
    check(lib.spk_svae_ar_fwd(_p(x), _p(z0), _p(w1), _p(bs[0]), _p(w2), _p(bs[1]), _p(w3), _p(bs[2]), _p(v1), _p(v2), _p(v3),
                              _p(idx32), _p(z), _p(q), T, B, cx, cz, h1, h2, k, _stream(idx)), "spk_svae_ar_fwd")
    return z, q


# ---------------------------------------------------------------------------------------------- SNN_VAE training path
def _lin_train_input(x, name, T, B):
    """fp32 / u8 / bool [T,B,n] -> (contiguous tensor, kind, n)."""
    x = _dev(x, name)
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    if x.dim() != 3 or x.shape[:2] != (T, B) or x.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{name} must be fp32/u8 [{T}, {B}, n], got {x.dtype} {tuple(x.shape)}")
    return x, (LIN_IN_F32 if x.dtype == torch.float32 else LIN_IN_U8), x.shape[2]


def linear_lif_train_fwd(x, weight, bias, v=None, x2=None, lif=True):
    """Multi-step Linear (+ the LIFNode's training forward), spk_linear_lif_train_fwd.

    x: fp32/u8 [T,B,in1]; x2: optional second input [T,B,in2] read as the concat [x | x2] (weight [out, in1+in2]).
    lif=True: returns (spikes fp32 [T,B,out], h_seq fp32 [T,B,out]); v fp32 [B,out] (None: zeros) is the state before and,
    updated in place, after.  lif=False: returns (currents fp32 [T,B,out], None)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError(f"x must be [T, B, in], got {getattr(x, 'shape', None)}")
    T, B = x.shape[0], x.shape[1]
    x, k1, n1 = _lin_train_input(x, "x", T, B)
    if x2 is not None:
        x2, k2, n2 = _lin_train_input(x2, "x2", T, B)
    else:
        k2, n2 = LIN_IN_F32, 0
    w, b = _linear_params(weight, bias, n1 + n2)
    n_out = w.shape[0]
    out = torch.empty((T, B, n_out), dtype=torch.float32, device=x.device)
    h = None
    if lif:
        h = torch.empty_like(out)
        if v is None:
            raise ValueError("lif=True needs the neuron state v [B, out]")
        if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
                and v.shape == (B, n_out)):
            raise ValueError(f"v must be a contiguous fp32 [{B}, {n_out}] device tensor")
    check(lib.spk_linear_lif_train_fwd(_p(x), k1, n1, _p(x2), k2, n2, _p(w), _p(b), _p(v) if lif else None, _p(out), _p(h),
                                       _p(v) if lif else None, int(bool(lif)), T, B, n_out, _stream(x)),
          "spk_linear_lif_train_fwd")
    return out, h


def linear_lif_train_bwd(grad_out, h_seq, x, weight, x2=None, grad_x_cols=0, want_bias=True):
    """Backward of linear_lif_train_fwd (spk_linear_lif_train_bwd): (grad_x fp32 [T,B,grad_x_cols] or None, grad_w, grad_b)."""
    g = _dev(grad_out, "grad_out", torch.float32)
    if g.dim() != 3:
        raise ValueError(f"grad_out must be [T, B, out], got {tuple(g.shape)}")
    T, B, n_out = g.shape
    x, k1, n1 = _lin_train_input(x, "x", T, B)
    if x2 is not None:
        x2, k2, n2 = _lin_train_input(x2, "x2", T, B)
    else:
        k2, n2 = LIN_IN_F32, 0
    w, _ = _linear_params(weight, None, n1 + n2)
    if w.shape[0] != n_out:
        raise ValueError(f"weight has {w.shape[0]} outputs, grad_out {n_out}")
    ws = None
    if h_seq is not None:
        h_seq = _dev(h_seq, "h_seq", torch.float32)
        if h_seq.shape != g.shape:
            raise ValueError(f"h_seq {tuple(h_seq.shape)} != grad_out {tuple(g.shape)}")
        ws = torch.empty_like(g)
    if not 0 <= grad_x_cols <= n1 + n2:
        raise ValueError(f"grad_x_cols {grad_x_cols} outside [0, {n1 + n2}]")
    gx = torch.empty((T, B, grad_x_cols), dtype=torch.float32, device=g.device) if grad_x_cols else None
    gw = torch.empty_like(w)
    gb = torch.empty(n_out, dtype=torch.float32, device=g.device) if want_bias else None
    check(lib.spk_linear_lif_train_bwd(_p(g), _p(h_seq), _p(ws), _p(x), k1, n1, _p(x2), k2, n2, _p(w), _p(gx), grad_x_cols,
                                       _p(gw), _p(gb), T, B, n_out, _stream(g)), "spk_linear_lif_train_bwd")
    return gx, gw, gb


class LinearLIFTrainFunction(torch.autograd.Function):
    """layer.Linear + LIFNode (or layer.Linear alone, lif=False) in training, R/snn_model/vae_model.py:212-228,306-546:
    one launch forward (spk_linear_lif_train_fwd), the BPTT and the three gradient GEMMs backward (spk_linear_lif_train_bwd).
    apply(x [T,B,in1], x2 [T,B,in2] or None, weight, bias, v [B,out] or None, lif) -> spikes / currents fp32 [T,B,out].
    v (no gradient: every state a grad pass starts from was made without grad or is the reset value) is updated in place."""

    @staticmethod
    def forward(ctx, x, x2, weight, bias, v, lif):
        out, h = linear_lif_train_fwd(x.detach(), weight.detach(), None if bias is None else bias.detach(), v,
                                      None if x2 is None else x2.detach(), lif)
        ctx.save_for_backward(x.detach(), None if x2 is None else x2.detach(), weight.detach(), h)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, x2, w, h = ctx.saved_tensors
        n1 = x.shape[2]
        need_x, need_x2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        cols = n1 + x2.shape[2] if need_x2 else (n1 if need_x else 0)
        gx, gw, gb = linear_lif_train_bwd(g_out.contiguous(), h, x, w, x2, cols, ctx.has_bias)
        gx1 = gx[..., :n1] if need_x else None
        gx2 = gx[..., n1:] if need_x2 else None
        return gx1, gx2, gw, gb if ctx.needs_input_grad[3] else None, None, None


def svae_ar_prefix(x, z0, layers, vs, idx=None, sched=None, noise=None, z_teacher=None):
    """The no-grad prefix passes of one training Bernoulli loop in one launch (spk_svae_ar_prefix_fwd).

    Posterior: x u8/bool [T,B,cx] and idx [T,B,cz].  Prior: x None, sched bool/u8 [T-1], noise fp32 [n_sched,B,cz] (n_sched =
    scheduled steps; with none, [0,B,cz] and the result is [z0, z_teacher[:-1]]), z_teacher fp32 [T,B,cz].  vs: the three
    layers' v fp32 [B,h], updated in place.
    Returns z_t_minus fp32 [T,B,cz]."""
    (w1, b1), (w2, b2), (w3, b3) = layers
    if x is not None:
        x = _dev(x, "x")
        if x.dtype == torch.bool:
            x = x.view(torch.uint8)
        if x.dtype != torch.uint8 or x.dim() != 3:
            raise ValueError(f"x must be u8 spikes [T, B, cx], got {x.dtype} {tuple(x.shape)}")
        T, B, cx = x.shape
        if idx is None:
            raise ValueError("the posterior's prefix needs idx")
        idx = _dev(idx, "idx")
        if idx.dim() != 3 or idx.shape[:2] != (T, B) or idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"idx must be an integer [{T}, {B}, cz] tensor, got {idx.dtype} {tuple(idx.shape)}")
        cz = idx.shape[2]
        idx = idx if idx.dtype == torch.int32 else idx.to(torch.int32)
        dev = x.device
    else:
        if sched is None or noise is None or z_teacher is None:
            raise ValueError("the prior's prefix needs sched, noise and z_teacher")
        z_teacher = _dev(z_teacher, "z_teacher", torch.float32)
        if z_teacher.dim() != 3:
            raise ValueError(f"z_teacher must be [T, B, cz], got {tuple(z_teacher.shape)}")
        T, B, cz = z_teacher.shape
        cx = 0
        sched = _dev(sched, "sched")
        if sched.dtype == torch.bool:
            sched = sched.view(torch.uint8)
        if sched.dtype != torch.uint8 or sched.shape != (T - 1,):
            raise ValueError(f"sched must be bool/u8 [{T - 1}], got {sched.dtype} {tuple(sched.shape)}")
        n_sched = int(sched.count_nonzero())
        noise = _dev(noise, "noise", torch.float32)
        if noise.shape != (n_sched, B, cz):
            raise ValueError(f"noise must be [{n_sched}, {B}, {cz}], got {tuple(noise.shape)}")
        dev = z_teacher.device
    if T < 2:
        raise ValueError("the prefix passes need T >= 2")
    z0 = _dev(z0, "initial_input", torch.float32)
    if z0.numel() != cz:
        raise ValueError(f"initial_input has {z0.numel()} elements, expected {cz}")
    w1, b1 = _linear_params(w1, b1, cx + cz)
    h1 = w1.shape[0]
    w2, b2 = _linear_params(w2, b2, h1)
    h2 = w2.shape[0]
    w3, b3 = _linear_params(w3, b3, h2)
    if w3.shape[0] % cz:
        raise ValueError(f"last layer has {w3.shape[0]} outputs, not a multiple of {cz} channels")
    k = w3.shape[0] // cz
    bs = [torch.zeros(w.shape[0], dtype=torch.float32, device=w.device) if bb is None else bb
          for w, bb in ((w1, b1), (w2, b2), (w3, b3))]
    v1, v2, v3 = vs
    for v, hh in ((v1, h1), (v2, h2), (v3, w3.shape[0])):
        if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.shape == (B, hh)):
            raise ValueError(f"v must be a contiguous fp32 [{B}, {hh}] device tensor")
    zm = torch.empty((T, B, cz), dtype=torch.float32, device=dev)
    if x is None and noise.numel() == 0:
        noise = z_teacher     # no scheduled step: the kernel never reads noise, but the entry point wants a non-null pointer
    check(lib.spk_svae_ar_prefix_fwd(_p(x), _p(z0), _p(w1), _p(bs[0]), _p(w2), _p(bs[1]), _p(w3), _p(bs[2]), _p(v1), _p(v2),
                                     _p(v3), _p(idx), _p(sched), _p(noise), _p(z_teacher), _p(zm), T, B, cx, cz, h1, h2, k,
                                     _stream(zm)), "spk_svae_ar_prefix_fwd")
    return zm


def _latent_args(q_z, p_z, idx):
    q = _dev(q_z.detach(), "q_z", torch.float32)
    idx = _dev(idx, "idx")
    if idx.dim() != 3 or idx.dtype != torch.int32:
        raise ValueError(f"idx must be int32 [T, B, cz], got {idx.dtype} {tuple(idx.shape)}")
    T, B, cz = idx.shape
    if q.dim() != 3 or q.shape[:2] != (T, B) or q.shape[2] % cz:
        raise ValueError(f"q_z must be [{T}, {B}, {cz}*k], got {tuple(q.shape)}")
    if T > MAX_T:
        raise NotImplementedError(f"spkdiff: the latent loss keeps at most {MAX_T} steps")
    p = None
    if p_z is not None:
        p = _dev(p_z.detach(), "p_z", torch.float32)
        if p.shape != q.shape:
            raise ValueError(f"p_z {tuple(p.shape)} != q_z {tuple(q.shape)}")
    return q, p, idx, T, B, cz, q.shape[2] // cz


class LatentLossFunction(torch.autograd.Function):
    """The posterior's gather sampled_z[t] = q_z[t].view(-1)[idx_t] (R/snn_model/vae_model.py:531-541) and, with p_z, the MMD
    loss mean((PSP(mean_k q_z) - PSP(mean_k p_z))^2) (:273-285), fused (spk_svae_latent_loss_fwd / _bwd).
    apply(q_z [T,B,cz*k], p_z [T,B,cz*k] or None, idx int32 [T,B,cz], tau_s) -> (sampled_z [T,B,cz], loss [] (zero without p_z))."""

    @staticmethod
    def forward(ctx, q_z, p_z, idx, tau_s):
        q, p, idx, T, B, cz, k = _latent_args(q_z, p_z, idx)
        sz = torch.empty((T, B, cz), dtype=torch.float32, device=q.device)
        loss = torch.zeros((), dtype=torch.float32, device=q.device)
        ws = None
        if p is not None:
            ws = torch.empty(lib.spk_svae_latent_loss_ws_floats(B, cz), dtype=torch.float32, device=q.device)
        check(lib.spk_svae_latent_loss_fwd(_p(q), _p(p), _p(idx), _p(sz), _p(loss) if p is not None else None, _p(ws), T, B, cz,
                                           k, float(tau_s), _stream(q)), "spk_svae_latent_loss_fwd")
        ctx.save_for_backward(q, p, idx)
        ctx.tau_s = float(tau_s)
        if p is None:
            ctx.mark_non_differentiable(loss)
        return sz, loss

    @staticmethod
    def backward(ctx, g_sz, g_loss):
        q, p, idx = ctx.saved_tensors
        T, B, cz = idx.shape
        k = q.shape[2] // cz
        gl = g_loss.reshape(1).contiguous() if (g_loss is not None and p is not None) else None
        gs = g_sz.contiguous() if g_sz is not None else None
        gq = torch.empty_like(q)
        gp = torch.empty_like(p) if (p is not None and ctx.needs_input_grad[1]) else None
        with timed("train.latent_loss_bwd"):
            check(lib.spk_svae_latent_loss_bwd(_p(q), _p(p), _p(idx), _p(gl), _p(gs), _p(gq), _p(gp), T, B, cz, k, ctx.tau_s,
                                               _stream(q)), "spk_svae_latent_loss_bwd")
        return gq, gp, None, None


# ---------------------------------------------------------------------------------------------- the plain-CNN VQVAE baseline
# csrc/ann_vqvae.hip: the encoder + code search in one launch, the decoder in two.  A workgroup takes one image and a launch has
# at most ANN_VQVAE_GRID_CAP workgroups, which loop over the images beyond that (the batch sizes the tests make special).
ANN_VQVAE_D = _C["SPK_ANN_VQVAE_D"]
ANN_VQVAE_MAX_K = _C["SPK_ANN_VQVAE_MAX_K"]
ANN_VQVAE_GRID_CAP = _C["SPK_ANN_VQVAE_GRID_CAP"]
ANN_VQVAE_GROUP = 1                # images a workgroup works on at a time


def ann_vqvae_supported(C, H, W, D, K):
    """Do spk_ann_vqvae_encode / _decode take images [*,C,H,W], embedding_dim D and K codes?  Host-only: no device needed."""
    return bool(lib.spk_ann_vqvae_supported(int(C), int(H), int(W), int(D), int(K)))


def _ann_params(params, n, what):
    if len(params) != n:
        raise ValueError(f"{what}: expected {n} weight / bias tensors, got {len(params)}")
    return [_dev(p.detach(), f"{what} parameter {i}", torch.float32) for i, p in enumerate(params)]


def ann_vqvae_encode(images, enc_params, codebook, want_z=False, want_e=False):
    """images fp32 [B,C,H,W]; enc_params = (w1, b1, w2, b2, w3, b3) of CNN_Encoder.convs.{0,2,4}; codebook [K,D] ->
    (indices int64 [B*h*w], z fp32 [B,D,h,w] or None, e fp32 [B,D,h,w] or None), h = H / 4.  One launch."""
    images = _dev(images, "images", torch.float32)
    if images.dim() != 4:
        raise ValueError(f"ann_vqvae_encode: images must be [B,C,H,W], got {tuple(images.shape)}")
    w1, b1, w2, b2, w3, b3 = _ann_params(enc_params, 6, "ann_vqvae_encode")
    codebook = _dev(codebook.detach(), "codebook", torch.float32)
    B, C, H, W = images.shape
    K, D = codebook.shape
    if (tuple(w1.shape), tuple(w2.shape), tuple(w3.shape)) != ((32, C, 3, 3), (64, 32, 3, 3), (D, 64, 1, 1)):
        raise ValueError("ann_vqvae_encode: the weights are not CNN_Encoder's for these images and this codebook")
    h, w = H // 4, W // 4
    idx = torch.empty(B * h * w, dtype=torch.int64, device=images.device)
    z = torch.empty((B, D, h, w), dtype=torch.float32, device=images.device) if want_z else None
    e = torch.empty((B, D, h, w), dtype=torch.float32, device=images.device) if want_e else None
    check(lib.spk_ann_vqvae_encode(_p(images), _p(w1), _p(b1), _p(w2), _p(b2), _p(w3), _p(b3), _p(codebook), _p(idx), _p(z),
                                   _p(e), B, C, H, W, D, K, _stream(images)), "spk_ann_vqvae_encode")
    return idx, z, e


def ann_vqvae_decode_ws(B, H, W, device):
    """A workspace for ann_vqvae_decode calls of this shape (the second layer's output)."""
    nbytes = int(lib.spk_ann_vqvae_decode_ws_bytes(int(B), int(H), int(W)))
    if nbytes < 0:
        check(nbytes, "spk_ann_vqvae_decode_ws_bytes")
    return torch.empty(nbytes // 8, dtype=torch.int64, device=device)


def ann_vqvae_decode(code, dec_params, codebook, want_u8=False, ws=None):
    """code: tokens int64 [B,h,w] (the embedding gather folded in; a token outside [0, K) gives NaN pixels where it reaches)
    or e fp32 [B,D,h,w]; dec_params = (wt1, bt1, wt2, bt2, wt3, bt3) of CNN_Decoder.convs.{0,2,4}; codebook [K,D] ->
    (x_recon fp32 [B,C,H,W], uint8(clip(x_recon + 0.5, 0, 1) * 255) or None).  Two launches.  ``ws``: a workspace of
    ``ann_vqvae_decode_ws`` to reuse (this call's alone while it is in flight)."""
    wt1, bt1, wt2, bt2, wt3, bt3 = _ann_params(dec_params, 6, "ann_vqvae_decode")
    codebook = _dev(codebook.detach(), "codebook", torch.float32)
    K, D = codebook.shape
    C = wt3.shape[1]
    if (tuple(wt1.shape), tuple(wt2.shape), tuple(wt3.shape)) != ((D, 64, 3, 3), (64, 32, 3, 3), (32, C, 3, 3)):
        raise ValueError("ann_vqvae_decode: the weights are not CNN_Decoder's for this codebook")
    if code.dtype == torch.int64:
        code = _dev(code, "tokens", torch.int64)
        if code.dim() != 3:
            raise ValueError(f"ann_vqvae_decode: tokens must be [B,h,w], got {tuple(code.shape)}")
        tokens, e = code, None
        B, h, w = code.shape
    else:
        code = _dev(code, "e", torch.float32)
        if code.dim() != 4 or code.shape[1] != D:
            raise ValueError(f"ann_vqvae_decode: e must be [B,{D},h,w], got {tuple(code.shape)}")
        tokens, e = None, code
        B, _, h, w = code.shape
    H, W = 4 * h, 4 * w
    nbytes = int(lib.spk_ann_vqvae_decode_ws_bytes(B, H, W))
    if ws is None:
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=code.device)
    elif not (ws.is_cuda and ws.device == code.device and ws.is_contiguous() and ws.data_ptr() % 8 == 0
              and ws.numel() * ws.element_size() >= nbytes):
        raise ValueError(f"ann_vqvae_decode: ws must be a contiguous 8-byte aligned device buffer of at least {nbytes} bytes")
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=code.device)
    u8 = torch.empty((B, C, H, W), dtype=torch.uint8, device=code.device) if want_u8 else None
    check(lib.spk_ann_vqvae_decode(_p(tokens), _p(e), _p(codebook), _p(wt1), _p(bt1), _p(wt2), _p(bt2), _p(wt3), _p(bt3), _p(ws),
                                   ws.numel() * ws.element_size(), _p(out), _p(u8), B, C, H, W, D, K, _stream(code)),
          "spk_ann_vqvae_decode")
    return out, u8


# ---------------------------------------------------------------------------------------------- the plain-CNN VQVAE baseline, training
# VQVAE.forward in train() mode (R/snn_model/vae_model.py:660-672) on csrc/conv_train.hip (the six convolutions, the ReLU as
# an epilogue of the launch in front of it and of the data-gradient launch behind it) and csrc/ann_vqvae_train.hip (the
# time-free vector quantiser and the mean-squared-error loss).  Everything between the caller's image and the three loss
# scalars is channels-last: Conv 1x1's output IS the reference's flat_x [B*h*w, D].
# (stride, pad, transposed, out_pad, ReLU behind it) of CNN_Encoder.convs.{0,2,4} and CNN_Decoder.convs.{0,2,4}
ANN_TRAIN_LAYERS = ((2, 1, False, 0, True), (2, 1, False, 0, True), (1, 0, False, 0, False),
                    (2, 1, True, 1, True), (2, 1, True, 1, True), (1, 1, True, 0, False))


def ann_vqvae_train_supported(xshape, enc_params, dec_params, codebook):
    """Do the training kernels take the quantiser (spk_ann_vqvae_train_supported: D and the codebook's LDS image) and every layer
    of the network (forward, the data gradients the backward needs, weight gradient) for images of this shape?"""
    K, D = (int(v) for v in codebook.shape)
    if not lib.spk_ann_vqvae_train_supported(D, K):
        return False
    shape = tuple(int(v) for v in xshape)
    for i, (w, (stride, pad, tr, op, _)) in enumerate(zip(tuple(enc_params[0::2]) + tuple(dec_params[0::2]), ANN_TRAIN_LAYERS)):
        if not conv_train_supported(shape, w, stride, pad, tr, op, need_gi=i > 0, forward=True):
            return False
        _, _, _, _, Cout, Ho, Wo, _ = _conv_train_geometry(shape, w, stride, pad, tr, op)
        shape = (shape[0], Cout, Ho, Wo)
    return True


def ann_data_variance(data_variance, device):
    """data_variance as a float32 device tensor [1]: an fp32 device tensor is taken as it is, anything else (a Python number, a CPU
    tensor as R/main.py:91-107 passes, another dtype) is converted -- one small launch and no read-back.  VQVAE keeps the
    result per model, so its iterations convert nothing."""
    if isinstance(data_variance, torch.Tensor) and data_variance.is_cuda:
        return _dev(data_variance.detach().reshape(1).to(torch.float32), "data_variance", torch.float32)
    return torch.full((1,), float(data_variance), dtype=torch.float32, device=device)


def _ann_train_ws(rows, elems, device):
    """Scratch of the two mean-square reductions (the partial sums; no state).  Per (device, stream), or per ops.flag_scope
    store under capture, like the other loss kernels' workspaces."""
    return _flag_ws("ann_vqvae_train", device, (int(lib.spk_ann_vqvae_train_ws_bytes(int(rows), int(elems))) + 7) // 8 * 2)


def ann_vqvae_train_forward(x, enc_params, dec_params, codebook, beta, data_variance):
    """images x fp32 [B,C,H,W]; enc_params / dec_params as for ann_vqvae_encode / _decode; codebook [K,D] ->
    ((e_q_loss, recon_loss, real_loss_rec) fp32 scalars on the device, record): the record holds what the backward needs, all
    channels-last -- x, a1, a2 (post-ReLU), z [B,D,h,w], idx int64 [B*h*w], e, d1, d2 (post-ReLU), x_recon and data_variance [1].
    Ten launches (plus one layout copy of an RGB image)."""
    x = _dev(x.detach(), "x", torch.float32)
    if x.dim() != 4:
        raise ValueError(f"ann_vqvae_train_forward: images must be [B,C,H,W], got {tuple(x.shape)}")
    enc = _ann_params(enc_params, 6, "ann_vqvae_train_forward")
    dec = _ann_params(dec_params, 6, "ann_vqvae_train_forward")
    cb = _dev(codebook.detach(), "codebook", torch.float32)
    B, C, H, W = x.shape
    K, D = cb.shape
    if (tuple(tuple(w.shape) for w in enc[0::2] + dec[0::2])
            != ((32, C, 3, 3), (64, 32, 3, 3), (D, 64, 1, 1), (D, 64, 3, 3), (64, 32, 3, 3), (32, C, 3, 3))):
        raise ValueError("ann_vqvae_train_forward: the weights are not CNN_Encoder's / CNN_Decoder's for these images and this codebook")
    dv = ann_data_variance(data_variance, x.device)
    L = ANN_TRAIN_LAYERS
    a1 = conv_train_forward(x, enc[0], enc[1], *L[0][:4], relu=True)
    a2 = conv_train_forward(a1, enc[2], enc[3], *L[1][:4], relu=True)
    z = conv_train_forward(a2, enc[4], enc[5], *L[2][:4])
    N = z.shape[0] * z.shape[2] * z.shape[3]
    idx = torch.empty(N, dtype=torch.int64, device=x.device)
    e = _empty_cl(tuple(z.shape), x.device)
    l_eq, l_rec, l_real = (torch.empty((), dtype=torch.float32, device=x.device) for _ in range(3))
    ws = _ann_train_ws(N, x.numel(), x.device)
    nb = ws.numel() * ws.element_size()
    st = _stream(x)
    with timed("train.ann_vq_fwd"):
        check(lib.spk_ann_vqvae_train_vq_fwd(_p(z), _p(cb), _p(idx), _p(e), _p(l_eq), float(beta), _p(ws), nb, N, D, K, st),
              "spk_ann_vqvae_train_vq_fwd")
    d1 = conv_train_forward(e, dec[0], dec[1], *L[3][:4], relu=True)
    d2 = conv_train_forward(d1, dec[2], dec[3], *L[4][:4], relu=True)
    x_recon = conv_train_forward(d2, dec[4], dec[5], *L[5][:4])
    with timed("train.ann_loss_fwd"):
        check(lib.spk_ann_vqvae_train_loss_fwd(_p(x_recon), _p(x), _p(dv), _p(l_rec), _p(l_real), _p(ws), nb, B, C, H, W, st), "spk_ann_vqvae_train_loss_fwd")
    rec = dict(x=x, a1=a1, a2=a2, z=z, idx=idx, e=e, d1=d1, d2=d2, x_recon=x_recon, data_variance=dv)
    return (l_eq, l_rec, l_real), rec


def ann_vqvae_train_backward(rec, enc_params, dec_params, codebook, beta, g_eq, g_recon, g_real):
    """Gradients of the thirteen parameters, in (enc_params, dec_params, codebook) order and each in its parameter's memory
    format, from the record of ann_vqvae_train_forward and the gradients of the three losses (device scalars or None): the loss
    backward, five data-gradient launches (four masked by the saved post-ReLU activation; ConvT D->64's is not: the quantiser
    is behind it), the quantiser's backward and six weight gradients with their bias gradients."""
    enc = _ann_params(enc_params, 6, "ann_vqvae_train_backward")
    dec = _ann_params(dec_params, 6, "ann_vqvae_train_backward")
    cb = _dev(codebook.detach(), "codebook", torch.float32)
    x, xr, z = rec["x"], rec["x_recon"], rec["z"]
    B, C, H, W = x.shape
    K, D = cb.shape
    N = rec["idx"].numel()
    st = _stream(x)

    def scalar(g):
        return None if g is None else _dev(g.detach().reshape(1), "loss gradient", torch.float32)

    g_eq, g_recon, g_real = scalar(g_eq), scalar(g_recon), scalar(g_real)
    L, all3 = ANN_TRAIN_LAYERS, (True, True, True)
    g = _empty_cl(tuple(xr.shape), x.device)
    with timed("train.ann_loss_bwd"):
        check(lib.spk_ann_vqvae_train_loss_bwd(_p(xr), _p(x), _p(g_recon), _p(g_real), _p(rec["data_variance"]), _p(g), B, C, H, W,
                                               st), "spk_ann_vqvae_train_loss_bwd")
    g, gw6, gb6 = conv_train_backward(g, rec["d2"], dec[4], *L[5][:4], all3, relu_input=True)
    g, gw5, gb5 = conv_train_backward(g, rec["d1"], dec[2], *L[4][:4], all3, relu_input=True)
    g_e, gw4, gb4 = conv_train_backward(g, rec["e"], dec[0], *L[3][:4], all3)
    g_z = _empty_cl(tuple(z.shape), x.device)
    g_cb = torch.empty_like(cb)
    with timed("train.ann_vq_bwd"):
        check(lib.spk_ann_vqvae_train_vq_bwd(_p(g_e), _p(g_eq), _p(z), _p(rec["idx"]), _p(cb), float(beta), _p(g_z), _p(g_cb), N, D,
                                             K, st), "spk_ann_vqvae_train_vq_bwd")
    g, gw3, gb3 = conv_train_backward(g_z, rec["a2"], enc[4], *L[2][:4], all3, relu_input=True)
    g, gw2, gb2 = conv_train_backward(g, rec["a1"], enc[2], *L[1][:4], all3, relu_input=True)
    _, gw1, gb1 = conv_train_backward(g, x, enc[0], *L[0][:4], (False, True, True))
    return gw1, gb1, gw2, gb2, gw3, gb3, gw4, gb4, gw5, gb5, gw6, gb6, g_cb


class ANNVQVAETrainFunction(torch.autograd.Function):
    """VQVAE.forward in train() mode as one autograd node: apply(x, beta, data_variance, *enc_params, *dec_params, codebook) ->
    (e_q_loss, recon_loss, real_loss_rec).  The image gets no gradient."""

    @staticmethod
    def forward(ctx, x, beta, data_variance, *params):
        enc, dec, cb = params[:6], params[6:12], params[12]
        losses, rec = ann_vqvae_train_forward(x, enc, dec, cb, beta, data_variance)
        ctx.keys = tuple(rec)
        ctx.save_for_backward(*params, *rec.values())
        ctx.beta = float(beta)
        return losses

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_eq, g_recon, g_real):
        saved = ctx.saved_tensors
        params, rec = saved[:13], dict(zip(ctx.keys, saved[13:]))
        grads = ann_vqvae_train_backward(rec, params[:6], params[6:12], params[12], ctx.beta, g_eq, g_recon, g_real)
        return (None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:]))
