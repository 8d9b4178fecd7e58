"""CPU tests (no GPU): which shapes each matrix-core kernel family takes is answered by the library -- one host predicate per family,
called by that family's entry point itself -- and ``spkdiff.ops`` asks it.  The formulas ``ops`` computed on its own before are kept
here, frozen, and every answer is compared with them over a grid of shapes; the one place where the two had drifted apart is
listed literally."""
import itertools

import pytest
import torch

from spkdiff import _lib, ops

lib = _lib.lib

HW = range(1, 65)
TS = (4, 16)
GEOS = ((3, 1, 1), (3, 2, 1), (1, 1, 0), (5, 1, 2))           # (k, stride, pad)
CH = (16, 30, 32, 48, 64, 96, 128, 256, 320)
DGRAD_N = (1, 63, 64, 784, 2 ** 31 // (49 * 16))

# The latents on which the int8 launch refused what the Python copy of its rule accepted: the input-slab copy pieces per wave,
# (H * ceil(W / 2) + 3) / 4, exceed the eight the kernel is instantiated for while the tiles per wave do not.
DRIFT_HW = {(3, 21), (7, 9), (9, 7), (11, 5), (12, 5),
            (17, 3), (18, 3), (19, 3), (20, 3), (21, 3),
            (33, 1), (34, 1), (35, 1), (36, 1), (37, 1), (38, 1), (39, 1)}


# ---- the formulas of spkdiff/ops.py before the library answered (frozen copies) --------------------------------------------------
def frozen_den_mfma(Cout, Cin, k, stride, pad, T, H, W):
    ntiles = (H * W + 1) // 2
    nt = (ntiles + 3) // 4
    lds = 2 * ((H + 2) * (W + 2) * 512 + 18432)
    return (k == 3 and stride == 1 and pad == 1 and T == 16 and Cout % 32 == 0 and Cin % 32 == 0
            and nt <= 8 and lds <= 160 * 1024)


def frozen_den_fp6(Cout, Cin, k, stride, pad, T, H, W):
    ntiles = (H * W + 1) // 2
    bands = (ntiles + 3) // 4 > 7 and H % 2 == 0 and (H // 2) * W <= 32 and H >= 4
    Hin = H // 2 + 1 if bands else H
    npa = (Hin * ((W + 1) // 2) + 3) // 4
    lds = 2 * (((Hin + 2) * (W + 1) + 1) * 512 + 41984)
    return (k == 3 and stride == 1 and pad == 1 and T == 16 and Cout % 64 == 0 and Cin % 64 == 0
            and (bands or (ntiles + 3) // 4 <= 7) and npa <= 7 and lds <= 160 * 1024)


def frozen_den_fp6v2(Cout, Cin, k, stride, pad, T, H, W):
    return (k == 3 and stride == 1 and pad == 1 and T == 16 and (H, W) in ((7, 7), (8, 8)) and Cout % 32 == 0 and
            Cin % 32 == 0)


def frozen_conv_mfma(Cin, Cout, T, mode):
    return T == 16 and Cin % 16 == 0 and (mode == ops.MODE_MEMOUT or Cout % 16 == 0)


def frozen_vae_fp6_kind(Cin, Cout, k, stride, pad, out_pad, transposed, T, H, W):
    if k != 3 or stride != 2 or pad != 1 or T != 16 or Cout % 32:
        return None
    if transposed and out_pad == 1 and Cin == 64 and (H, W) in ((14, 14), (16, 16)):
        return ops.VAE_OUT_COLLAPSED
    if transposed and out_pad == 1 and Cin == 16 and (H, W) in ((7, 7), (8, 8)):
        return ops.VAE_OUT_S32
    if not transposed and Cin == 32 and (H, W) in ((14, 14), (16, 16)):
        return ops.VAE_OUT_PTC
    return None


def frozen_readout_collapsed(Cin, Cout, k):
    return Cin % 8 == 0 and k % 2 == 1 and ((4 + k - 1) * 64 * (Cin + 4) + Cout * k * k * Cin) * 4 <= 64 * 1024


def frozen_wgrad(Cout, Cin, H, W):
    return (H, W) in ((7, 7), (8, 8)) and Cout % 128 == 0 and Cin % 64 == 0


def frozen_dgrad(Cout, Cin, H, W, N):
    return ((H, W) in ((7, 7), (8, 8)) and Cout % 16 == 0 and Cin % 32 == 0 and Cout * Cin >= 8192 and N >= 64
            and N * H * W * Cout < 2 ** 31)


def _den_grid():
    return itertools.product(CH, CH, GEOS, TS, HW, HW)


def test_den_mfma_supported_equals_the_frozen_formula_except_on_the_drift_latents():
    differ, accepted_drift = set(), 0
    for Cout, Cin, (k, s, p), T, H, W in _den_grid():
        got, was = ops.den_mfma_supported(Cout, Cin, k, s, p, T, H, W), frozen_den_mfma(Cout, Cin, k, s, p, T, H, W)
        assert isinstance(got, bool)
        if got != was:
            differ.add((H, W))
            assert was and not got, (Cout, Cin, k, s, p, T, H, W)         # only ever: accepted before, refused now
        if (H, W) in DRIFT_HW:
            accepted_drift += got
    assert differ == DRIFT_HW
    assert accepted_drift == 0
    # ... and on those latents every channel pair that passes the modulus rules WAS accepted: the whole difference is the latent
    for (H, W), Cout, Cin in itertools.product(sorted(DRIFT_HW), CH, CH):
        assert frozen_den_mfma(Cout, Cin, 3, 1, 1, 16, H, W) == (Cout % 32 == 0 and Cin % 32 == 0)


@pytest.mark.parametrize("name", ["den_fp6_supported", "den_fp6v2_supported"])
def test_fp6_predicates_equal_the_frozen_formulas(name):
    got_f, was_f = getattr(ops, name), {"den_fp6_supported": frozen_den_fp6, "den_fp6v2_supported": frozen_den_fp6v2}[name]
    n_true = 0
    for Cout, Cin, (k, s, p), T, H, W in _den_grid():
        got = got_f(Cout, Cin, k, s, p, T, H, W)
        assert got is bool(was_f(Cout, Cin, k, s, p, T, H, W)), (Cout, Cin, k, s, p, T, H, W)
        n_true += got
    assert n_true > 0


def test_vae_fp6_kind_equals_the_frozen_dispatch_table():
    seen = set()
    kind, was = ops.vae_fp6_kind, frozen_vae_fp6_kind
    for Cin, Cout, (k, s, p), T, H, W in itertools.product(CH, CH, GEOS, TS, HW, HW):
        for tr, op in ((False, 0), (False, 1), (True, 0), (True, 1)):
            got = kind(Cin, Cout, k, s, p, op, tr, T, H, W)
            assert got == was(Cin, Cout, k, s, p, op, tr, T, H, W), (Cin, Cout, k, s, p, op, tr, T, H, W)
            if got is not None:
                seen.add(got)
    assert seen == {ops.VAE_OUT_COLLAPSED, ops.VAE_OUT_S32, ops.VAE_OUT_PTC}
    for Cin, Cout, H, tr in itertools.product(CH, (32, 48), (7, 8, 12, 14, 16), (False, True)):
        assert ops.convT_fp6_supported(Cin, Cout, 3, 2, 1, 1, tr, 16, H, H) == (was(Cin, Cout, 3, 2, 1, 1, tr, 16, H, H) == ops.VAE_OUT_COLLAPSED)


def test_gather_readout_and_gradient_predicates_equal_the_frozen_formulas():
    for Cin, Cout, T, mode in itertools.product(CH, CH, TS, (ops.MODE_LIF, ops.MODE_MEMOUT)):
        assert ops.conv_mfma_supported(Cin, Cout, T, mode) is bool(frozen_conv_mfma(Cin, Cout, T, mode)), (Cin, Cout, T, mode)
    # the kernel itself takes any Cout in both modes (the 16-channel rule is this package's policy), and no other mode
    assert lib.spk_conv_mfma_fused_supported(16, 40, 16, ops.MODE_LIF) == 1
    assert lib.spk_conv_mfma_fused_supported(16, 32, 16, ops.MODE_RAW) == 0 == lib.spk_conv_mfma_fused_supported(16, 32, 16, ops.MODE_MEAN)
    for Cin, Cout, (k, _, _) in itertools.product(CH + (8, 1), CH + (1, 3, 8), GEOS + ((2, 1, 1), (7, 1, 3))):
        want = bool(frozen_readout_collapsed(Cin, Cout, k))
        assert ops.readout_collapsed_supported(Cin, Cout, k) is want, (Cin, Cout, k)
        # "any width up to 64" is the answer at width 64, and a narrower image never fits worse
        assert lib.spk_readout_collapsed_supported(Cin, Cout, k, 64) == want == lib.spk_readout_collapsed_supported(Cin, Cout, k, -1)
        assert lib.spk_readout_collapsed_supported(Cin, Cout, k, 28) >= want
    for Cout, Cin, H, W in itertools.product(CH, CH, HW, HW):
        assert ops.conv3x3_wgrad_supported(Cout, Cin, H, W) is bool(frozen_wgrad(Cout, Cin, H, W)), (Cout, Cin, H, W)
        for N in DGRAD_N:
            assert ops.conv3x3_dgrad_supported(Cout, Cin, H, W, N) is bool(frozen_dgrad(Cout, Cin, H, W, N)), (Cout, Cin, H, W, N)
    # the library's part of the data-gradient answer is capability alone: no layer-size or batch cut
    assert lib.spk_conv3x3_dgrad_supported(16, 32, 7, 7, 1) == 1 and not ops.conv3x3_dgrad_supported(16, 32, 7, 7, 1)
    n_edge = 2 ** 31 // (49 * 16)
    assert lib.spk_conv3x3_dgrad_supported(16, 32, 7, 7, n_edge) == 1 and lib.spk_conv3x3_dgrad_supported(16, 32, 7, 7, n_edge + 1) == 0


def test_denoiser_on_a_drift_latent_runs_the_direct_kernels(monkeypatch):
    """9x7: the fp6 family is out (H odd, 8 tiles per wave) and the int8 launch refuses (9 copy pieces per wave).  The automatic choice
    is the fp64 direct kernels, and the container launches nothing else."""
    from snn_model.vq_diffusion import DummyModel, functional
    from _dispatch_recorders import B, _install_recorders
    torch.manual_seed(0)
    m = DummyModel(1, 128).eval()
    functional.set_step_mode(m, 'm')
    assert m.conv_impl_request == 'auto'
    assert m.impl_for(9, 7) == 'direct-f64' == m.impl_for(7, 9)
    assert m.impl_for(7, 7) != 'direct-f64' and m.impl_for(8, 8) != 'direct-f64'
    calls = _install_recorders(monkeypatch)
    with torch.no_grad():
        m.logits_from_tokens(torch.zeros((B, 1, 9, 7)), 5)
    launches = [c for c in calls if not re_pack(c)]
    assert len(launches) == 7 and launches[0] == 'den_build_input', calls
    assert all(c.startswith('conv_fused(') for c in launches[1:]), calls


def re_pack(call):
    return call.split('(')[0] in ('pack_conv_weight', 'bn_prepare')
