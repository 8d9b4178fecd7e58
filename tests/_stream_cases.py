"""The launch forms csrc/lif.hip and csrc/lif_train.hip pick for the element-wise streaming kernels (spk_lif_fwd, spk_lif_fwd_ex,
spk_bn_eval_fwd, spk_memout_fwd, spk_lif_train_fwd / _bwd, spk_psp), mirrored on the host, the sizes that sit past each of their
grid caps, and the host oracles of the kernels that ``oracle/snn_ref.py`` states only through autograd.

Each ``*_launch`` function restates one entry point: which kernel the call picks (4 elements per thread or 1, division or
multiplication by 1 / tau, the template form), with which grid, and how many grid-stride passes the kernel makes.  The constants
(SPK_LIF_GRID_PER_CU, SPK_LIF_BLOCK, LIF_GRID_CAP, SPK_LIF_TU, GRID_CAP, the 256-thread rounding of spk_grid) are read from the
sources.  Every case of SECOND_PASS_CASES / MISALIGNED_CASES carries the side it claims (``claim``): the GPU test
(tests/test_gpu_stream_kernels.py) runs the shape with poisoned outputs and the CPU test (tests/test_stream_cases_host.py)
checks the claim, so a retune of a cap that moves a case off its boundary fails on a machine without a GPU too."""
import math
import os
import re

import numpy as np
import torch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spiking-diffusion_amd", "csrc")
SPIKE_F32, SPIKE_U8, SPIKE_BITS = 0, 1, 2


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _constant(src, name):
    """``constexpr int NAME = a * b * ...;`` of source file ``src``: the product."""
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+(?:\s*\*\s*\d+)*)\s*;", _src(src))
    assert m, f"{name} not found in {src}"
    return math.prod(int(f) for f in m.group(1).split("*"))


def _match(src, pattern, what):
    m = re.search(pattern, _src(src))
    assert m, f"{what} not found in {src}"
    return m


SPK_LIF_TU = _constant("lif.hip", "SPK_LIF_TU")
SPK_LIF_BLOCK = _constant("lif.hip", "SPK_LIF_BLOCK")
SPK_LIF_GRID_PER_CU = _constant("lif.hip", "SPK_LIF_GRID_PER_CU")
LIF_GRID_CAP = _constant("lif.hip", "LIF_GRID_CAP")
GRID_CAP = _constant("lif_train.hip", "GRID_CAP")
# lif_grid:  cap = 256ll * SPK_LIF_GRID_PER_CU
LIF_GRID_CUS = int(_match("lif.hip", r"cap\s*=\s*(\d+)ll\s*\*\s*SPK_LIF_GRID_PER_CU", "lif_grid's cap").group(1))
# spk_grid:  g = (work_items + 255) / 256
_m = _match("spk_common.h", r"g\s*=\s*\(work_items\s*\+\s*(\d+)\)\s*/\s*(\d+)\s*;", "spk_grid's rounding")
SPK_GRID_BLOCK = int(_m.group(2))
assert int(_m.group(1)) == SPK_GRID_BLOCK - 1
MEMOUT_MAX_T = 64                      # spk_memout_fwd: the coefficients' LDS array

SMALL_N = (1, 3, 4, 63, 64, 65, 1000, 1001)


def _cdiv(a, b):
    return -(-a // b)


def spk_grid(work_items, cap):
    return max(1, min(_cdiv(work_items, SPK_GRID_BLOCK), cap))


def lif_grid(work_items):
    return max(1, min(_cdiv(work_items, SPK_LIF_BLOCK), LIF_GRID_CUS * SPK_LIF_GRID_PER_CU))


def pow2(tau):
    """frexpf(tau).mantissa == 0.5: the launchers multiply by 1 / tau instead of dividing."""
    return math.frexp(float(np.float32(tau)))[0] == 0.5


def _aligned(*byte_offsets):
    """Every pointer is a fresh allocation (16-byte aligned) plus its offset."""
    return all(o % 16 == 0 for o in byte_offsets)


def _passes(items, grid, block, **more):
    """``items`` work items (one per thread and pass) on ``grid`` x ``block`` threads: passes of the grid-stride loop, and how the
    last pass ends (threads of it that find no item; whether its last workgroup is partly filled)."""
    per_pass = grid * block
    passes = _cdiv(items, per_pass)
    last = items - (passes - 1) * per_pass
    return dict(items=items, grid=grid, block=block, per_pass=per_pass, passes=passes, last_pass_items=last,
                idle_threads=per_pass - last, partial_workgroup=last % block != 0, **more)


def lif_fwd_launch(N, T, spike_dtype=SPIKE_F32, tau=2.0, x_off=0, v_off=0):
    """spk_lif_fwd; x_off / v_off: bytes from a 16-byte boundary of x_seq / v (the spikes are a fresh allocation)."""
    div = not pow2(tau)
    if spike_dtype == SPIKE_BITS:
        words = _cdiv(N, 64)
        grid = spk_grid(words * 64, LIF_GRID_CAP)
        L = _passes(words, grid * 256 // 64, 1, kernel="lif_fwd_bits", vec=1, div=div, words=words, pad_bits=words * 64 - N)
        L.update(grid=grid, block=256)                  # items are waves: one word per wave and pass
        return L
    vec = 4 if (N % 4 == 0 and _aligned(x_off, v_off)) else 1
    groups = _cdiv(N, vec)
    return _passes(groups, lif_grid(groups), SPK_LIF_BLOCK, kernel="lif_fwd", vec=vec, div=div, out=spike_dtype,
                   chunks=_cdiv(T, SPK_LIF_TU), pass_elems=lif_grid(groups) * SPK_LIF_BLOCK * vec)


def lif_fwd_ex_launch(N, T, tau=2.0, soft_reset=False, decay_input=True, want_v_seq=False):
    """spk_lif_fwd_ex: one neuron per thread; the soft reset without decay_input multiplies by (1 - 1 / tau) and has no DIV form."""
    div = (not pow2(tau)) and (decay_input or not soft_reset)
    return _passes(N, spk_grid(N, LIF_GRID_CAP), 256, kernel="lif_fwd_ex", vec=1, div=div, soft=bool(soft_reset),
                   decay=bool(decay_input), v_seq=bool(want_v_seq))


def bn_eval_launch(M, C, HW, x_off=0):
    total = M * C * HW
    vec = 4 if (HW % 4 == 0 and _aligned(x_off)) else 1
    L = _passes(total // vec, spk_grid(total // vec, LIF_GRID_CAP), 256, kernel="bn_eval", vec=vec, total=total)
    L["pass_elems"] = L["per_pass"] * vec
    # the channel and the offset inside its row at which a thread's second pass starts (0, 0: the pass length is whole images)
    L["pass_start_channel"] = (L["pass_elems"] // HW) % C
    L["pass_start_in_row"] = L["pass_elems"] % HW
    return L


def memout_launch(N, T, x_off=0):
    if T <= 0 or T > MEMOUT_MAX_T:
        return dict(kernel="refused")
    vec = 4 if (N % 4 == 0 and _aligned(x_off)) else 1
    return _passes(N // vec, spk_grid(N // vec, LIF_GRID_CAP), 256, kernel="memout", vec=vec)


def _train_launch(kernel, N, offs, **more):
    vec = 4 if (N % 4 == 0 and _aligned(*offs)) else 1
    groups = _cdiv(N, vec)
    return _passes(groups, spk_grid(groups, GRID_CAP), 256, kernel=kernel, vec=vec, **more)


def lif_train_fwd_launch(N, T, x_off=0, v_off=0):
    return _train_launch("lif_train_fwd", N, (x_off, v_off))


def lif_train_bwd_launch(N, T, detach_reset=False, gs_off=0, gv_off=0, h_off=0):
    return _train_launch("lif_train_bwd", N, (gs_off, gv_off, h_off), detach=bool(detach_reset))


def psp_launch(N, T, backward=False, x_off=0):
    return _train_launch("psp", N, (x_off,), backward=bool(backward))


LAUNCH = dict(lif_fwd=lif_fwd_launch, lif_fwd_ex=lif_fwd_ex_launch, bn_eval=bn_eval_launch, memout=memout_launch,
              lif_train_fwd=lif_train_fwd_launch, lif_train_bwd=lif_train_bwd_launch, psp=psp_launch)


def _case(id_, entry, args, claim, why):
    return dict(id=id_, entry=entry, args=args, claim=claim, why=why)


def _second(vec, **more):
    """vector or scalar kernel, exactly two passes, the second one ragged: a few hundred items, so most of its threads are idle
    and its last workgroup is partly filled."""
    def claim(L):
        return (L["vec"] == vec and L["passes"] == 2 and 0 < L["last_pass_items"] < 512 and L["partial_workgroup"]
                and all(L[k] == v for k, v in more.items()))
    return claim


# Sizes one full pass plus a ragged remainder above each cap.  T = 2 keeps the streams under a second.
N_LIF_VEC, N_LIF_SCALAR, N_LIF_WAVES = 8_388_608 + 1_212, 2_097_152 + 301, 2_097_152 + 333
N_TRAIN_VEC, N_TRAIN_SCALAR = 16_777_216 + 1_212, 4_194_304 + 301
BN_VEC, BN_SCALAR = dict(M=699_080, C=3, HW=4), dict(M=99_880, C=7, HW=3)

SECOND_PASS_CASES = [
    _case("lif_fwd_f32_vec", "lif_fwd", dict(N=N_LIF_VEC, T=2, spike_dtype=SPIKE_F32), _second(4, kernel="lif_fwd"),
          "vector kernel, 2 passes, ragged last pass"),
    _case("lif_fwd_u8_vec", "lif_fwd", dict(N=N_LIF_VEC, T=2, spike_dtype=SPIKE_U8), _second(4, kernel="lif_fwd"),
          "vector kernel, u8 spikes, 2 passes, ragged last pass"),
    _case("lif_fwd_f32_scalar", "lif_fwd", dict(N=N_LIF_SCALAR, T=2, spike_dtype=SPIKE_F32), _second(1, kernel="lif_fwd"),
          "scalar kernel (odd N), 2 passes, ragged last pass"),
    _case("lif_fwd_u8_scalar", "lif_fwd", dict(N=N_LIF_SCALAR, T=2, spike_dtype=SPIKE_U8), _second(1, kernel="lif_fwd"),
          "scalar kernel (odd N), u8 spikes, 2 passes, ragged last pass"),
    _case("lif_fwd_bits", "lif_fwd", dict(N=N_LIF_WAVES, T=2, spike_dtype=SPIKE_BITS),
          lambda L: (L["kernel"] == "lif_fwd_bits" and L["passes"] == 2 and 0 < L["last_pass_items"] < 8 and 0 < L["pad_bits"] < 64
                     and L["last_pass_items"] % 4 != 0),
          "ballot kernel: a few words on the second pass, the last one partly live, the last workgroup partly filled"),
    _case("lif_fwd_ex", "lif_fwd_ex", dict(N=N_LIF_WAVES, T=2), _second(1, kernel="lif_fwd_ex"),
          "one neuron per thread, 2 passes, N % 64 != 0"),
    _case("bn_eval_vec", "bn_eval", BN_VEC,
          lambda L: _second(4)(L) and L["pass_start_channel"] != 0,
          "vector kernel, 2 passes; the second pass starts at channel 2 of 3"),
    _case("bn_eval_scalar", "bn_eval", BN_SCALAR,
          lambda L: _second(1)(L) and L["pass_start_channel"] != 0 and L["pass_start_in_row"] != 0,
          "scalar kernel (HW = 3), 2 passes; the second pass starts inside a row of channel 2 of 7"),
    _case("memout_vec", "memout", dict(N=N_LIF_VEC, T=2), _second(4, kernel="memout"), "vector kernel, 2 passes"),
    _case("memout_scalar", "memout", dict(N=N_LIF_SCALAR, T=2), _second(1, kernel="memout"), "scalar kernel (odd N), 2 passes"),
    _case("lif_train_fwd_vec", "lif_train_fwd", dict(N=N_TRAIN_VEC, T=2), _second(4), "vector kernel, 2 passes"),
    _case("lif_train_fwd_scalar", "lif_train_fwd", dict(N=N_TRAIN_SCALAR, T=2), _second(1), "scalar kernel (odd N), 2 passes"),
    _case("lif_train_bwd_vec", "lif_train_bwd", dict(N=N_TRAIN_VEC, T=2), _second(4), "vector kernel, 2 passes"),
    _case("lif_train_bwd_scalar", "lif_train_bwd", dict(N=N_TRAIN_SCALAR, T=2), _second(1), "scalar kernel (odd N), 2 passes"),
    _case("psp_fwd_vec", "psp", dict(N=N_TRAIN_VEC, T=2), _second(4), "vector kernel, 2 passes"),
    _case("psp_fwd_scalar", "psp", dict(N=N_TRAIN_SCALAR, T=2), _second(1), "scalar kernel (odd N), 2 passes"),
    _case("psp_bwd_vec", "psp", dict(N=N_TRAIN_VEC, T=2, backward=True), _second(4, backward=True), "adjoint, vector, 2 passes"),
    _case("psp_bwd_scalar", "psp", dict(N=N_TRAIN_SCALAR, T=2, backward=True), _second(1, backward=True),
          "adjoint, scalar, 2 passes"),
]

# One full pass exactly: the largest size on the near side of each cap (host-checked only; the mirror must put it at one pass).
ONE_PASS_CASES = [
    _case("lif_fwd_vec_at_cap", "lif_fwd", dict(N=8_388_608, T=2), lambda L: L["vec"] == 4 and L["passes"] == 1
          and L["idle_threads"] == 0, "vector kernel: every thread of the capped grid has one group"),
    _case("lif_fwd_scalar_at_cap", "lif_fwd", dict(N=2_097_151, T=2), lambda L: L["vec"] == 1 and L["passes"] == 1
          and L["idle_threads"] == 1, "scalar kernel: odd N one short of the capped grid"),
    _case("lif_fwd_bits_at_cap", "lif_fwd", dict(N=2_097_152, T=2, spike_dtype=SPIKE_BITS),
          lambda L: L["passes"] == 1 and L["idle_threads"] == 0, "ballot kernel: one word per wave of the capped grid"),
    _case("lif_fwd_ex_at_cap", "lif_fwd_ex", dict(N=2_097_152, T=2), lambda L: L["passes"] == 1 and L["idle_threads"] == 0, ""),
    _case("bn_eval_vec_at_cap", "bn_eval", dict(M=524_288, C=4, HW=4), lambda L: L["vec"] == 4 and L["passes"] == 1
          and L["idle_threads"] == 0, ""),
    _case("memout_scalar_at_cap", "memout", dict(N=2_097_151, T=2), lambda L: L["vec"] == 1 and L["passes"] == 1, ""),
    _case("lif_train_fwd_vec_at_cap", "lif_train_fwd", dict(N=16_777_216, T=2), lambda L: L["vec"] == 4 and L["passes"] == 1
          and L["idle_threads"] == 0, ""),
    _case("lif_train_bwd_scalar_at_cap", "lif_train_bwd", dict(N=4_194_303, T=2), lambda L: L["vec"] == 1 and L["passes"] == 1, ""),
    _case("psp_vec_at_cap", "psp", dict(N=16_777_216, T=2), lambda L: L["vec"] == 4 and L["passes"] == 1, ""),
]


def _scalar_although_n4(L):
    return L["vec"] == 1 and L["passes"] == 1


# A contiguous view 1, 2 or 3 floats into a larger allocation, N % 4 == 0: the float4 kernels must not be picked.
MISALIGNED_N = 1000
MISALIGNED_CASES = (
    [_case(f"lif_fwd_x_plus{k}", "lif_fwd", dict(N=MISALIGNED_N, T=3, x_off=4 * k), _scalar_although_n4, "x_seq misaligned")
     for k in (1, 2, 3)] +
    [_case(f"lif_fwd_v_plus{k}", "lif_fwd", dict(N=MISALIGNED_N, T=3, v_off=4 * k), _scalar_although_n4, "v misaligned")
     for k in (1, 2, 3)] +
    [_case("bn_eval_x_plus1", "bn_eval", dict(M=5, C=3, HW=64, x_off=4), _scalar_although_n4, "x misaligned, HW % 4 == 0"),
     _case("memout_x_plus1", "memout", dict(N=MISALIGNED_N, T=16, x_off=4), _scalar_although_n4, "x_seq misaligned"),
     _case("lif_train_fwd_x_plus1", "lif_train_fwd", dict(N=MISALIGNED_N, T=3, x_off=4), _scalar_although_n4, "x_seq misaligned"),
     _case("lif_train_fwd_v_plus2", "lif_train_fwd", dict(N=MISALIGNED_N, T=3, v_off=8), _scalar_although_n4, "v_init misaligned"),
     _case("lif_train_bwd_gs_plus1", "lif_train_bwd", dict(N=MISALIGNED_N, T=3, gs_off=4), _scalar_although_n4,
           "grad_spike_seq misaligned"),
     _case("lif_train_bwd_h_plus3", "lif_train_bwd", dict(N=MISALIGNED_N, T=3, h_off=12), _scalar_although_n4, "h_seq misaligned"),
     _case("lif_train_bwd_gv_plus2", "lif_train_bwd", dict(N=MISALIGNED_N, T=3, gv_off=8), _scalar_although_n4,
           "grad_v_last misaligned"),
     _case("psp_x_plus1", "psp", dict(N=MISALIGNED_N, T=3, x_off=4), _scalar_although_n4, "inputs misaligned"),
     _case("psp_bwd_x_plus3", "psp", dict(N=MISALIGNED_N, T=3, backward=True, x_off=12), _scalar_although_n4, "gradient misaligned")])

# Past 2^31: (T - 1) * N, the offset of the last time step's plane, no longer fits a 32-bit int.  One buffer serves spk_lif_fwd as
# [16, N] and spk_memout_fwd as [64, N / 4] (9.2 GB of fp32 generated on the device; the host oracle runs on blocks of columns).
PAST_2G_T, PAST_2G_N = 16, 143_166_000
PAST_2G_MEMOUT_T, PAST_2G_MEMOUT_N = 64, PAST_2G_N // 4
PAST_2G_BLOCK = 4096


def past_2g_blocks(N):
    """Eight blocks of PAST_2G_BLOCK columns: the first, the last (ragged end included) and six in between."""
    starts = [0] + [(N * k // 7) // 4 * 4 + 3 for k in range(1, 7)] + [N - PAST_2G_BLOCK]
    return [(a, a + PAST_2G_BLOCK) for a in starts]


CASES = {c["id"]: c for c in SECOND_PASS_CASES + ONE_PASS_CASES + MISALIGNED_CASES}


def launch(case):
    return LAUNCH[case["entry"]](**case["args"])


def check_claims(cases):
    """[(id, launch description)] of the cases whose shape does not land where the case says it does."""
    return [(c["id"], launch(c)) for c in cases if not c["claim"](launch(c))]


# ------------------------------------------------------------------------------------------------------------- host oracles
EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52


def lif_train_fwd_f32(x_seq, v, v_threshold=1.0, v_reset=0.0, tau=2.0):
    """The loop of ``ref.lif_multi_step_train`` in fp32 without autograd, also returning the charged potential h of every step:
    (spike_seq, h_seq, v_last)."""
    v = v.clone()
    hs, ss = [], []
    for t in range(x_seq.shape[0]):
        if v_reset == 0.0:
            h = v + (x_seq[t] - v) / tau
        else:
            h = v + (x_seq[t] - (v - v_reset)) / tau
        s = ((h - v_threshold) >= 0).to(h)
        v = (1.0 - s) * h + s * v_reset
        hs.append(h)
        ss.append(s)
    return torch.stack(ss), torch.stack(hs), v


# fp32 roundings, to first order, on the longest path through one spk_atan_bptt_step (csrc/spk_common.h), line by line:
#   over = h - v_th                                   1
#   ax   = 1.5707964f * alpha * over                  over 1 + the rounded pi/2 constant 1 + two products 2        =  4
#   ax * ax                                           2 x 4 (both factors carry ax's error) + 1                    =  9
#   1.0f + ax * ax                                    + 1 (both terms positive: no amplification)                  = 10
#   g_s  = alpha / 2.0f / (...)                       alpha / 2 is exact; the division + 1                         = 11
#   (v_reset - h) * g_s                               the difference 1, the product 1                              = 13
#   dv_dh = ... + (1.0f - s)                          1.0f - s is exact; the sum + 1                               = 14
#   G * dv_dh                                         + 1                                                          = 15
#   gh = G * dv_dh + grad_s * g_s                     (the other term has 11 + 1 = 12)  the sum + 1                = 16
#   gx = gh * inv_tau                                 inv_tau = 1.0f / tau 1, the product 1                        = 18
#   G  = gh * carry                                   carry = 1.0f - inv_tau: 2 (inv_tau's error weighs inv_tau / carry <= 1
#                                                     for tau >= 2), the product 1                                 = 19
# Each term's error is relative to its own magnitude, so the error of an element is bounded by the count times 2^-24 times the
# same recurrence run on absolute values (M); 2^-23 in the bound leaves the second-order terms a factor of two.
BPTT_ROUNDINGS_PER_STEP = 19
# psp_kernel<BWD>:  G = acc + x 1;  ov = G * inv_tau 1 + 1;  acc = G * carry 2 + 1: four on the longer path
PSP_ADJOINT_ROUNDINGS_PER_STEP = 4


def lif_bptt_f64(grad_s, grad_v_last, h_seq, tau=2.0, v_threshold=1.0, v_reset=0.0, alpha=2.0, detach_reset=False):
    """The recurrence in the header of csrc/lif_train.hip in fp64 on a recorded h_seq (the parameters as the fp32 values the
    kernel receives).  Returns (grad_x, grad_v_init, M_x, M_v): the gradients, and the same recurrence on absolute values, the
    magnitude of the terms that enter each element."""
    f = lambda a: float(np.float32(a))
    tau, v_th, v_reset, alpha = f(tau), f(v_threshold), f(v_reset), f(alpha)
    gs, h = grad_s.double(), h_seq.double()
    T = h.shape[0]
    G = torch.zeros_like(h[0]) if grad_v_last is None else grad_v_last.double().reshape(h[0].shape).clone()
    MG = G.abs()
    gx, Mx = torch.empty_like(h), torch.empty_like(h)
    carry = 1.0 - 1.0 / tau
    for t in range(T - 1, -1, -1):
        over = h[t] - v_th
        s = (over >= 0).double()
        g = alpha / 2.0 / (1.0 + (math.pi / 2.0 * alpha * over) ** 2)
        dv, Mdv = 1.0 - s, 1.0 - s
        if not detach_reset:
            dv = dv + (v_reset - h[t]) * g
            Mdv = Mdv + (v_reset - h[t]).abs() * g
        gh = G * dv + gs[t] * g
        Mgh = MG * Mdv + gs[t].abs() * g
        gx[t], Mx[t] = gh / tau, Mgh / tau
        G, MG = gh * carry, Mgh * carry
    return gx, G, Mx, MG


def psp_adjoint_f64(grad_syn, tau_s=2.0):
    """The adjoint of the PSP filter (csrc/lif_train.hip) in fp64: (grad_x, M_x)."""
    tau = float(np.float32(tau_s))
    g = grad_syn.double()
    G, MG = torch.zeros_like(g[0]), torch.zeros_like(g[0])
    gx, Mx = torch.empty_like(g), torch.empty_like(g)
    for t in range(g.shape[0] - 1, -1, -1):
        G, MG = G + g[t], MG + g[t].abs()
        gx[t], Mx[t] = G / tau, MG / tau
        G, MG = G * (1.0 - 1.0 / tau), MG * (1.0 - 1.0 / tau)
    return gx, Mx


def steps_feeding(T, like):
    """[T, 1, ...]: element t of a reverse scan is fed by the steps T-1 .. t."""
    return torch.arange(T, 0, -1, dtype=torch.float64).view((T,) + (1,) * (like.dim() - 1))


def bound_ratio(got, want, bound):
    """max over the elements of |got - want| / bound, with 0 / 0 = 0 and x / 0 = inf."""
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


def memout_f32(x_seq, coef):
    """acc = acc + x[t] * coef[t] in t order, multiply and add as separate fp32 operations."""
    acc = torch.zeros_like(x_seq[0])
    c = coef.reshape(-1)
    for t in range(x_seq.shape[0]):
        p = x_seq[t] * c[t]
        acc = acc + p
    return acc
