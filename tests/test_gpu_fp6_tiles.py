"""The packed weights of the two certified kernels, byte for byte: spk_den_pack_weight_fp6v2 (csrc/den_mfma_fp6v2.hip) and
spk_vae_fp6_pack (csrc/vae_fp6.hip) against the host statement of the format (tests/_fp6_tiles_oracle.py; its own checks and the
conditions on the weights: tests/test_fp6_tiles_host.py).  Every other test sees the tiles only through the spikes computed from them.

Cases: fp6v2 at (Cout, Cin) = (32, 32) and (64, 64) -- the second has two channel groups and two chunks; vae_fp6 at (32, 16) plain (one
half-filled chunk), (32, 64) plain (two chunks) and (64, 64) ConvTranspose2d.  Per case, torch.equal on the defined bytes of the tiles
(the slab padding of fp6v2 is not defined), the int32 quantised weights, the fp64 scales and the fp64 biases; both packers give the same
quantised weights for the same plain weight; fp6v2's L1 norm lies in [exact, exact (1 + 2e-6)] (exact: the fp64 L1 norm of q 2^-sh; the
bound: the kernel's factor 1.000001 and one fp32 rounding)."""
import numpy as np
import pytest
import torch

import _fp6_tiles_oracle as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def _pack(ops, dev, kind, w, bias, transposed):
    """-> (wq, scale, bias_d, qtab, wl1 or None) on the host."""
    if kind == "v2":
        wq, scale, bias_d, wl1, qtab = ops.den_pack_weight_fp6v2(w.to(dev), None if bias is None else bias.to(dev))
    else:
        wq, scale, bias_d, qtab = ops.vae_fp6_pack(w.to(dev), None if bias is None else bias.to(dev), transposed)[:4]
        wl1 = None
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in (wq, scale, bias_d, qtab, wl1))


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_packed_tiles_are_the_format(ops, dev, case):
    kind, Cout, Cin, transposed = case
    w, bias = T.case_weights(case)
    q, sh, scale = T.quantise(w.numpy(), transposed)
    want, mask = (T.v2_slabs if kind == "v2" else T.vae_tiles)(q)
    wq, g_scale, g_bias, qtab, wl1 = _pack(ops, dev, kind, w, bias, transposed)
    assert wq.dtype == torch.uint8 and wq.numel() == want.size
    tmask = torch.from_numpy(mask)
    n_bad = int((wq[tmask] != torch.from_numpy(want)[tmask]).sum())
    print(f"FP6_TILES {T.case_id(case)}: {int(mask.sum())} defined bytes of {want.size}, {n_bad} differ")
    assert torch.equal(wq[tmask], torch.from_numpy(want)[tmask])
    assert qtab.dtype == torch.int32 and torch.equal(qtab, torch.from_numpy(q.astype(np.int32)))
    assert g_scale.dtype == torch.float64 and torch.equal(g_scale, torch.from_numpy(scale))
    assert g_bias.dtype == torch.float64 and torch.equal(g_bias, bias.double())
    if kind == "v2":
        exact = torch.from_numpy(np.abs(q).reshape(Cout, -1).sum(axis=1).astype(np.float64) * scale)
        lo, hi = wl1.double() - exact, exact * (1.0 + 2e-6) - wl1.double()
        print(f"FP6_TILES {T.case_id(case)}: wl1 / exact - 1 in [{float((wl1.double() / exact.clamp_min(1e-300) - 1)[exact > 0].min()):.3e}, "
              f"{float((wl1.double() / exact.clamp_min(1e-300) - 1)[exact > 0].max()):.3e}]")
        assert wl1.dtype == torch.float32 and bool((lo >= 0).all()) and bool((hi >= 0).all())
        # the same plain weight through the other packer: the same quantised weights (and no bias: zeros)
        if Cin <= 64:
            _, v_scale, v_bias, v_qtab, _ = _pack(ops, dev, "vae", w, None, False)
            assert torch.equal(v_qtab, qtab) and torch.equal(v_scale, g_scale) and torch.equal(v_bias, torch.zeros(Cout, dtype=torch.float64))
