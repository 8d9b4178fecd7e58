"""Oracles of the training BatchNorm + LIF operator (csrc/bn_lif_train.hip through ops.BNLIFTrainFunction), shared by
tests/test_gpu_bn_lif_train_shapes.py (the VQ-VAE's shapes), tests/test_gpu_bn_lif_train_denoiser.py (the denoiser's) and
tests/test_bn_lif_train_oracle_host.py (which checks this file on the CPU before a GPU test trusts it).

Three independent statements of the operator:

  _oracle          fp64 F.batch_norm(training=True) + the per-step arithmetic of oracle.snn_ref.lif_multi_step_train with autograd;
                   at a neuron-step within FRAGILE of the threshold the spike value is the kernel's.
  oracle_given     the same with the spike VALUE of every neuron-step supplied (the ATan surrogate still carries the gradient): fed
                   the kernel's spikes, its gradients are those of the kernel's own trajectory at every neuron, so a gradient check
                   excludes nothing.  It also returns what it would have decided itself, and the fragile mask.
  restate_fwd32    the apply launch in fp32, operation by operation (the library is built with -ffp-contract=off, so the launch is
                   these operations and nothing else): from the kernel's save_mean / save_invstd there is ONE answer per
                   neuron-step, bit for bit.

plus the layouts the operator writes and reads: the C4 spike records from host spikes, a gradient that is broadcast over T and / or
a channel slice of a wider channels-last tensor, and the launch geometry (rows per workgroup step, slice counts) restated from
DESIGN.md §4.5 for the workspace bound."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from oracle import snn_ref as ref
from _conv_bn_lif_oracle import bits_to_packed, fma32, spikes_to_bits

T = 16
FRAGILE = 1e-5


def _rel_l2(got, want):
    return float((got.double() - want.double()).norm() / (want.double().norm() + 1e-30))


def _inputs(dev, B, C, H, with_v, seed, T=T):
    g = torch.Generator(device=dev).manual_seed(seed)
    shape = (T, B, C, H, H)
    y = torch.randn(shape, generator=g, device=dev) * 2 + 0.3
    gamma = 1 + 0.3 * torch.randn(C, generator=g, device=dev)
    beta = 0.5 * torch.randn(C, generator=g, device=dev)
    rm, rv = torch.randn(C, generator=g, device=dev), torch.rand(C, generator=g, device=dev) + 0.5
    v0 = torch.rand(B, C, H, H, generator=g, device=dev) - 0.5 if with_v else None
    gs = torch.randn(shape, generator=g, device=dev)
    gv = torch.randn(B, C, H, H, generator=g, device=dev) if with_v else None
    return y, gamma, beta, rm, rv, v0, gs, gv


def _run_hip(ops, y, gamma, beta, rm, rv, v0, gs, gv, det):
    """(spikes, v_last, save_mean, save_invstd, running mean, running var, grad_y, grad_gamma, grad_beta, grad_v_init)."""
    yd, gd, bd = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    vd = None if v0 is None else v0.clone().requires_grad_(True)
    rmd, rvd = rm.clone(), rv.clone()
    s, vl = ops.BNLIFTrainFunction.apply(yd, gd, bd, vd, rmd, rvd, 0.1, 1e-5, 2.0, 1.0, 0.0, 2.0, det)
    mean, invstd = s.grad_fn.saved_tensors[3:5]
    loss = (s * gs).sum() + ((vl * gv).sum() if gv is not None else 0)
    loss.backward()
    torch.cuda.synchronize()
    return (s.detach(), vl.detach(), mean.clone(), invstd.clone(), rmd, rvd, yd.grad, gd.grad, bd.grad,
            None if vd is None else vd.grad)


def _oracle(y, gamma, beta, rm, rv, v0, gs, gv, det, s_hip):
    """fp64 BatchNorm (batch statistics) + LIF with autograd; at fragile neuron-steps the spike is the kernel's."""
    shape = y.shape
    yo, go, bo = (t.double().requires_grad_(True) for t in (y, gamma, beta))
    vo = None if v0 is None else v0.double().requires_grad_(True)
    rmo, rvo = rm.double(), rv.double()
    z = F.batch_norm(yo.flatten(0, 1), rmo, rvo, go, bo, True, 0.1, 1e-5).view(shape)
    v = torch.zeros(shape[1:], dtype=torch.float64, device=y.device) if vo is None else vo
    spikes, fragile = [], []
    for t in range(shape[0]):
        h = v + (z[t] - v) / 2.0
        fr = (h.detach() - 1.0).abs() < FRAGILE
        sp = ref._ATanSpike.apply(h - 1.0, 2.0)
        sp = sp + (torch.where(fr, s_hip[t].double(), sp.detach()) - sp).detach()      # (value: the kernel's decision where fragile)
        sd = sp.detach() if det else sp
        v = (1.0 - sd) * h
        spikes.append(sp)
        fragile.append(fr)
    so = torch.stack(spikes)
    ((so * gs.double()).sum() + ((v * gv.double()).sum() if gv is not None else 0)).backward()
    yd = yo.detach()
    mean = yd.mean(dim=(0, 1, 3, 4))
    invstd = 1.0 / torch.sqrt(yd.var(dim=(0, 1, 3, 4), unbiased=False) + 1e-5)
    return (so.detach(), v.detach(), mean, invstd, rmo, rvo, yo.grad, go.grad, bo.grad, None if vo is None else vo.grad,
            torch.stack(fragile))


def oracle_given(y, gamma, beta, rm, rv, v0, gs, gv, det, s_given):
    """_oracle with the spike value of EVERY neuron-step taken from s_given [T,B,C,H,W] (None: the oracle's own decisions, the
    free-running trajectory).  The gradient still flows through the ATan surrogate at h - 1.  Returns _oracle's tuple with the
    spikes the oracle would have decided itself (h >= 1 on the trajectory it was given) in place of the spikes it used, so
    `own == s_given outside fragile` says that the given trajectory is the oracle's own up to threshold round-off."""
    shape = y.shape
    yo, go, bo = (t.double().requires_grad_(True) for t in (y, gamma, beta))
    vo = None if v0 is None else v0.double().requires_grad_(True)
    rmo, rvo = rm.double(), rv.double()
    z = F.batch_norm(yo.flatten(0, 1), rmo, rvo, go, bo, True, 0.1, 1e-5).view(shape)
    v = torch.zeros(shape[1:], dtype=torch.float64, device=y.device) if vo is None else vo
    used, own, fragile = [], [], []
    for t in range(shape[0]):
        h = v + (z[t] - v) / 2.0
        sp = ref._ATanSpike.apply(h - 1.0, 2.0)
        own.append(sp.detach())
        fragile.append((h.detach() - 1.0).abs() < FRAGILE)
        if s_given is not None:
            sp = sp + (s_given[t].double() - sp).detach()                              # (value: given; gradient: the surrogate's)
        sd = sp.detach() if det else sp
        v = (1.0 - sd) * h
        used.append(sp)
    so = torch.stack(used)
    ((so * gs.double()).sum() + ((v * gv.double()).sum() if gv is not None else 0)).backward()
    yd = yo.detach()
    mean = yd.mean(dim=(0, 1, 3, 4))
    invstd = 1.0 / torch.sqrt(yd.var(dim=(0, 1, 3, 4), unbiased=False) + 1e-5)
    return (torch.stack(own), v.detach(), mean, invstd, rmo, rvo, yo.grad, go.grad, bo.grad, None if vo is None else vo.grad,
            torch.stack(fragile))


def restate_fwd32(y, gamma, beta, mean, invstd, v0, tau=2.0, v_th=1.0, v_reset=0.0):
    """The apply launch on the host in fp32 numpy, one rounding per operation:  a = gamma * invstd;  b = beta - mean * a (a product,
    then a difference);  z = fma(y, a, b) (ONE rounding: fma32);  h = v + (z - (v - v_reset)) / tau;  s = (h - v_th >= 0);
    v = (1 - s) * h + s * v_reset.  mean / invstd are the kernel's own save_mean / save_invstd (or fp64 statistics rounded to
    fp32).  Returns CPU fp32 tensors (spikes [T,B,C,H,W], v_last [B,C,H,W], h [T,B,C,H,W])."""
    f32 = np.float32
    yn = y.detach().cpu().numpy().astype(f32, copy=False)
    Tn, B, C, H, W = yn.shape
    g_, b_, m_, i_ = (np.asarray(t.detach().cpu().numpy(), dtype=f32) for t in (gamma, beta, mean, invstd))
    a = (g_ * i_).astype(f32)
    prod = (m_ * a).astype(f32)
    b = (b_ - prod).astype(f32)
    a, b = a.reshape(1, C, 1, 1), b.reshape(1, C, 1, 1)
    tau, v_th, v_reset, one = f32(tau), f32(v_th), f32(v_reset), f32(1.0)
    v = np.full((B, C, H, W), v_reset, dtype=f32) if v0 is None else np.ascontiguousarray(v0.detach().cpu().numpy(), dtype=f32)
    spikes, hs = np.empty(yn.shape, dtype=f32), np.empty(yn.shape, dtype=f32)
    for t in range(Tn):
        z = fma32(yn[t], a, b)
        h = v + (z - (v - v_reset)) / tau
        s = ((h - v_th) >= f32(0.0)).astype(f32)
        v = (one - s) * h + s * v_reset
        assert h.dtype == f32 and v.dtype == f32
        spikes[t], hs[t] = s, h
    return torch.from_numpy(spikes), torch.from_numpy(v), torch.from_numpy(hs)


def c4_records(spikes):
    """CPU fp32 spikes [T,B,C,H,W] (C % 64 == 0) -> the C4 records u8 [B, C/64, H, W, T, 32] the forward writes next to them: 64
    channels per record as e2m1 nibbles (1.0 = 0x2, even channel in the low nibble)."""
    Tn, B, C, H, W = spikes.shape
    return bits_to_packed(spikes_to_bits(spikes), 64, T=Tn).reshape(B, C // 64, H, W, Tn, 32)


def strided_grad(B, C, H, W, T, pitch_channels, offset, broadcast, gen):
    """The gradient of the spikes as autograd leaves it in front of the denoiser's last layer: a channel slice
    [offset, offset + C) of a wider channels-last tensor -- [B, pitch_channels, H, W] expanded over T (step stride 0) when
    `broadcast`, else [T, B, pitch_channels, H, W].  Drawn with randn from `gen` (on gen's device); a view, nothing is copied."""
    shape = (B, pitch_channels, H, W) if broadcast else (T, B, pitch_channels, H, W)
    wide = torch.randn(shape, generator=gen, device=gen.device)
    nd = len(shape)
    to_cl = tuple(range(nd - 3)) + (nd - 2, nd - 1, nd - 3)
    from_cl = tuple(range(nd - 3)) + (nd - 1, nd - 3, nd - 2)
    wide = wide.permute(to_cl).contiguous().permute(from_cl)                           # channels-last memory
    sl = wide.narrow(nd - 3, offset, C)
    return sl.unsqueeze(0).expand(T, B, C, H, W) if broadcast else sl


# ---------------------------------------------------------------------------------------------------- launch geometry
def slice_counts(R, C, aligned=True):
    """Slice counts S (partial-sum rows of the workspace [S][C][2] doubles) of the launches of one forward + backward over
    R = B * HW rows, restated from DESIGN.md §4.5: the vector forms walk 256 * VEC / C rows per workgroup step on at most 1 024
    workgroups (VEC = 4: statistics, apply, second backward pass; VEC = 2: the BPTT pass), the scalar forms one row per wave on
    at most 8 192 / (4 * ceil(C / 64)) row slices.  dict(fwd=, bptt=, wraps_fwd=, wraps_bptt=)."""
    def vec(v):
        while v >= 2:
            if C % v == 0 and C // v <= 256 and 256 % (C // v) == 0:
                return v
            v //= 2
        return 1

    def count(v):
        if v == 1:
            return max(1, min(8192 // (4 * ((C + 63) // 64)), -(-R // 4)))
        rows = 256 * v // C
        return max(1, min(1024, -(-R // rows)))

    v4, v2 = (vec(4), vec(2)) if aligned else (1, 1)
    return dict(fwd=count(v4), bptt=count(v2), vec_fwd=v4, vec_bptt=v2,
                wraps_fwd=v4 > 1 and R > 1024 * (256 * v4 // C), wraps_bptt=v2 > 1 and R > 1024 * (256 * v2 // C))


# ---------------------------------------------------------------------------------------------------- the C-ABI, misaligned
def _off1(shape, dev, fill=None):
    """A contiguous fp32 tensor of `shape` that starts ONE float into a larger buffer: 4-byte, not 16-byte aligned."""
    n = int(np.prod(shape))
    buf = torch.empty(n + 8, dtype=torch.float32, device=dev)
    if fill is not None:
        buf.fill_(fill)
    view = buf[1:1 + n].view(shape)
    assert view.data_ptr() % 16 == 4
    return view


def run_cabi_misaligned(ops, y, gamma, beta, rm, rv, v0, gs, gv, det):
    """_run_hip's tuple from spk_bn_lif_train_fwd / spk_bn_lif_train_bwd called directly with y, spikes, v_out and grad_y as
    channels-last views that start one float into their buffers: every launch then takes its scalar form.  Before that,
    spk_bn_lif_train_fwd_c4 with a record pointer on the same tensors: SPK_ERR_UNSUPPORTED (-2) and no output touched (returned
    as the 11th and 12th entries: the code, and whether the NaN-filled outputs were left alone)."""
    dev = y.device
    Tn, B, C, H, W = y.shape
    HW = H * W
    cf, st = ctypes.c_float, torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    cl = lambda t: t.permute(*range(t.dim() - 3), t.dim() - 2, t.dim() - 1, t.dim() - 3)   # logical NCHW -> [..., H, W, C]
    nchw = lambda t: t.permute(*range(t.dim() - 3), t.dim() - 1, t.dim() - 3, t.dim() - 2)
    y1 = _off1((Tn, B, H, W, C), dev)
    y1.copy_(cl(y))
    s1, v1, gy1 = _off1((Tn, B, H, W, C), dev, float("nan")), _off1((B, H, W, C), dev, float("nan")), _off1((Tn, B, H, W, C), dev)
    v0c = None if v0 is None else cl(v0).contiguous()
    gsc, gvc = cl(gs).contiguous(), None if gv is None else cl(gv).contiguous()
    mean, invstd = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
    rmd, rvd = rm.clone(), rv.clone()
    gg, gb = torch.empty(C, device=dev), torch.empty(C, device=dev)
    gv0 = None if v0 is None else torch.empty((B, H, W, C), device=dev)
    nb = int(ops.lib.spk_bn_lif_train_ws_bytes(B, C, HW))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    rec = torch.zeros((B, C // 64, H, W, Tn, 32), dtype=torch.uint8, device=dev)
    rc_c4 = ops.lib.spk_bn_lif_train_fwd_c4(p(y1), p(gamma), p(beta), p(rmd), p(rvd), cf(0.1), cf(1e-5), p(v0c), p(s1), p(v1), p(mean),
                                            p(invstd), p(rec), p(ws), nb, Tn, B, C, HW, cf(2.0), cf(1.0), cf(0.0), st)
    torch.cuda.synchronize()
    untouched = bool(torch.isnan(s1).all() and torch.isnan(v1).all() and torch.isnan(mean).all() and torch.isnan(invstd).all()
                     and torch.equal(rmd, rm) and torch.equal(rvd, rv) and not bool(rec.any()))
    ops.check(ops.lib.spk_bn_lif_train_fwd(p(y1), p(gamma), p(beta), p(rmd), p(rvd), cf(0.1), cf(1e-5), p(v0c), p(s1), p(v1), p(mean),
                                           p(invstd), p(ws), nb, Tn, B, C, HW, cf(2.0), cf(1.0), cf(0.0), st), "spk_bn_lif_train_fwd")
    ops.check(ops.lib.spk_bn_lif_train_bwd(p(gsc), p(gvc), p(y1), p(gamma), p(beta), p(mean), p(invstd), p(v0c), p(gy1), p(gg), p(gb),
                                           p(gv0), p(ws), nb, Tn, B, C, HW, cf(2.0), cf(1.0), cf(0.0), cf(2.0), int(bool(det)), st),
              "spk_bn_lif_train_bwd")
    torch.cuda.synchronize()
    return (nchw(s1), nchw(v1), mean, invstd, rmd, rvd, nchw(gy1), gg, gb, None if gv0 is None else nchw(gv0), rc_c4, untouched)
