"""CPU tests of tests/_stream_cases.py: every case of its tables sits on the side of the grid cap (or of the alignment test) it
claims at the constants csrc/lif.hip and csrc/lif_train.hip have now, and the host oracles the GPU tests
(tests/test_gpu_stream_kernels.py) hold the kernels to agree with ``oracle/snn_ref.py``: the fp32 training forward bit for bit,
the fp64 BPTT and PSP-adjoint restatements with fp64 autograd through ``ref.lif_multi_step_train`` / ``ref.psp_filter`` within
fp64 round-off.  Also the part of the in-place contract of ops.lif_fwd / ops.lif_fwd_ex that needs no device."""
import pytest
import torch

import _stream_cases as sc
from oracle import snn_ref as ref


def test_constants_are_read_from_the_sources():
    assert sc.SPK_LIF_BLOCK == 256 == sc.SPK_GRID_BLOCK and sc.LIF_GRID_CUS == 256
    assert sc.SPK_LIF_TU >= 1 and sc.SPK_LIF_GRID_PER_CU >= 1 and sc.LIF_GRID_CAP >= 1 and sc.GRID_CAP >= 1
    # the products are evaluated, not their first factor
    assert sc.LIF_GRID_CAP % 256 == 0 and sc.LIF_GRID_CAP > 256 and sc.GRID_CAP % 256 == 0 and sc.GRID_CAP > 256


@pytest.mark.parametrize("table", ["SECOND_PASS_CASES", "ONE_PASS_CASES", "MISALIGNED_CASES"])
def test_every_case_lands_where_it_claims(table):
    cases = getattr(sc, table)
    assert len({c["id"] for c in cases}) == len(cases)
    bad = sc.check_claims(cases)
    assert not bad, f"cases off their boundary (retuned cap? move the case with it): {bad}"


def test_case_tables_cover_every_kernel_and_form():
    second = {(c["entry"], sc.launch(c)["vec"]) for c in sc.SECOND_PASS_CASES}
    for entry in ("lif_fwd", "bn_eval", "memout", "lif_train_fwd", "lif_train_bwd", "psp"):
        assert (entry, 4) in second and (entry, 1) in second, entry
    assert ("lif_fwd_ex", 1) in second
    assert any(sc.launch(c)["kernel"] == "lif_fwd_bits" for c in sc.SECOND_PASS_CASES)
    assert {sc.launch(c).get("out") for c in sc.SECOND_PASS_CASES if c["entry"] == "lif_fwd"} >= {sc.SPIKE_F32, sc.SPIKE_U8}
    assert {(c["args"].get("backward", False)) for c in sc.SECOND_PASS_CASES if c["entry"] == "psp"} == {False, True}


def test_small_family_kernel_choice():
    """N % 4 decides the kernel of the small family; tau decides the DIV form; T crosses the SPK_LIF_TU chunk."""
    for N in sc.SMALL_N:
        L = sc.lif_fwd_launch(N, 9, sc.SPIKE_F32, 3.0)
        assert L["vec"] == (4 if N % 4 == 0 else 1) and L["div"] and L["passes"] == 1 and L["chunks"] == 2
        assert sc.lif_train_fwd_launch(N, 1)["vec"] == L["vec"] == sc.psp_launch(N, 1)["vec"] == sc.memout_launch(N, 1)["vec"]
    assert not sc.lif_fwd_launch(64, 8, tau=2.0)["div"] and not sc.lif_fwd_launch(64, 8, tau=0.5)["div"]
    assert [sc.lif_fwd_launch(64, T)["chunks"] for T in (1, 7, 8, 9, 16, 17)] == [1, 1, 1, 2, 2, 3]
    assert sc.lif_fwd_launch(65, 2, sc.SPIKE_BITS)["pad_bits"] == 63 and sc.lif_fwd_launch(64, 2, sc.SPIKE_BITS)["pad_bits"] == 0
    # the soft reset without decay_input multiplies by (1 - 1 / tau): no division whatever tau is
    assert not sc.lif_fwd_ex_launch(64, 2, 3.0, soft_reset=True, decay_input=False)["div"]
    assert sc.lif_fwd_ex_launch(64, 2, 3.0, soft_reset=False, decay_input=False)["div"]
    assert sc.memout_launch(64, 64)["kernel"] == "memout" and sc.memout_launch(64, 65)["kernel"] == "refused"
    assert sc.bn_eval_launch(2, 3, 49)["vec"] == 1 and sc.bn_eval_launch(2, 3, 64)["vec"] == 4


def test_past_2g_sizes_overflow_a_32_bit_plane_offset():
    for T, N in ((sc.PAST_2G_T, sc.PAST_2G_N), (sc.PAST_2G_MEMOUT_T, sc.PAST_2G_MEMOUT_N)):
        assert (T - 1) * N >= 2 ** 31 and N % 4 == 0 and T * N == sc.PAST_2G_T * sc.PAST_2G_N
        blocks = sc.past_2g_blocks(N)
        assert blocks[0][0] == 0 and blocks[-1][1] == N and all(0 <= a < b <= N for a, b in blocks)
        assert all(b0 <= a1 for (_, b0), (a1, _) in zip(blocks, blocks[1:]))
    assert sc.memout_launch(sc.PAST_2G_MEMOUT_N, sc.PAST_2G_MEMOUT_T)["vec"] == 4 and sc.PAST_2G_MEMOUT_T == sc.MEMOUT_MAX_T
    L = sc.lif_fwd_launch(sc.PAST_2G_N, sc.PAST_2G_T, sc.SPIKE_U8)
    assert L["vec"] == 4 and L["passes"] > 2 and L["chunks"] == 2
    assert sc.lif_fwd_launch(sc.PAST_2G_N, sc.PAST_2G_T, sc.SPIKE_BITS)["pad_bits"] > 0


def _inputs(T, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, N, generator=g) * 1.5 + 0.7
    v0 = torch.rand(N, generator=g) - 0.5
    gs = torch.randn(T, N, generator=g)
    gv = torch.randn(N, generator=g)
    return x, v0, gs, gv


@pytest.mark.parametrize("tau,vr", [(2.0, 0.0), (3.0, -0.25), (2.0, -0.25)])
def test_fp32_training_forward_is_the_oracles(tau, vr):
    x, v0, _, _ = _inputs(9, 257, 3)
    s, h, v = sc.lif_train_fwd_f32(x, v0, 1.0, vr, tau)
    so, vo = ref.lif_multi_step_train(x, v0.clone(), 1.0, vr, tau)
    assert torch.equal(s, so) and torch.equal(v.view(torch.int32), vo.view(torch.int32))
    assert 0.05 < float(s.mean()) < 0.95
    # h is the potential the spikes were decided on, and the one the next step starts from where it did not fire
    assert torch.equal(s, ((h - 1.0) >= 0).float())
    assert torch.equal(torch.where(s[-1] == 0, h[-1], torch.full_like(v, vr)), v)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("tau,vr", [(2.0, 0.0), (3.0, -0.25)])
@pytest.mark.parametrize("with_gv", [True, False])
def test_fp64_bptt_restatement_is_fp64_autograd(det, tau, vr, with_gv):
    T, N = 9, 203
    x, v0, gs, gv = _inputs(T, N, 11)
    x, v0, gs, gv = x.double(), v0.double(), gs.double(), gv.double()
    xo, vo = x.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    so, vlast = ref.lif_multi_step_train(xo, vo, 1.0, vr, tau, 2.0, det)
    loss = (so * gs).sum() + ((vlast * gv).sum() if with_gv else 0.0)
    loss.backward()
    _, h, _ = sc.lif_train_fwd_f32(x, v0, 1.0, vr, tau)                  # (fp64 here: the loop keeps its argument's type)
    gx, gv0, Mx, Mv = sc.lif_bptt_f64(gs, gv if with_gv else None, h, tau, 1.0, vr, 2.0, det)
    c = sc.BPTT_ROUNDINGS_PER_STEP
    assert sc.bound_ratio(gx, xo.grad, c * sc.steps_feeding(T, gx) * sc.EPS64 * Mx) <= 1.0
    assert sc.bound_ratio(gv0, vo.grad, c * T * sc.EPS64 * Mv) <= 1.0
    assert float(xo.grad.abs().max()) > 0.1 and float(vo.grad.abs().max()) > 1e-3     # not a comparison of zeros
    if det:                                                              # and the two forms differ by far more than the bound
        gx2 = sc.lif_bptt_f64(gs, gv if with_gv else None, h, tau, 1.0, vr, 2.0, False)[0]
        assert float((gx2 - gx).abs().max()) > 1e-3


@pytest.mark.parametrize("tau_s", [2.0, 3.0])
def test_fp64_psp_adjoint_is_fp64_autograd(tau_s):
    T, N = 7, 101
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, N, generator=g, dtype=torch.float64).requires_grad_(True)
    gy = torch.randn(T, N, generator=g, dtype=torch.float64)
    (ref.psp_filter(x, tau_s) * gy).sum().backward()
    gx, Mx = sc.psp_adjoint_f64(gy, tau_s)
    assert sc.bound_ratio(gx, x.grad, sc.PSP_ADJOINT_ROUNDINGS_PER_STEP * sc.steps_feeding(T, gx) * sc.EPS64 * Mx) <= 1.0
    assert float(x.grad.abs().max()) > 0.1


def test_memout_oracle_is_separate_multiply_and_add():
    """The fp32 loop differs from a fused multiply-add on these inputs (so a contracted kernel would show), and agrees with the
    reference's ``torch.sum(x * coef, 0)`` to round-off."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(16, 4096, generator=g)
    coef = torch.pow(torch.tensor(0.8), torch.arange(15, -1, -1).float())
    want = sc.memout_f32(x, coef)
    fused = torch.zeros(4096)
    for t in range(16):
        fused = ref.fma_f32(x[t], coef[t], fused)
    assert int((fused != want).sum()) > 100
    assert float((want - ref.membrane_output(x.view(16, 1, 1, 64, 64)).flatten()).abs().max()) <= 2e-6


@pytest.mark.parametrize("fn", ["lif_fwd", "lif_fwd_ex"])
def test_in_place_state_must_be_contiguous(fn):
    """ops.lif_fwd / ops.lif_fwd_ex update v in place: a non-contiguous v is refused (before anything is asked of a device)
    rather than copied, which would leave the caller's state where it was."""
    from spkdiff import ops
    x = torch.zeros(2, 3, 5)
    v = torch.zeros(5, 3).t()
    assert not v.is_contiguous()
    with pytest.raises(ValueError, match="in place.*contiguous"):
        getattr(ops, fn)(x, v)
    with pytest.raises(RuntimeError, match="no CPU path"):               # a contiguous one gets as far as the device check
        getattr(ops, fn)(x, v.contiguous())
