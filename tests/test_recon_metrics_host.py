"""CPU tests of the reconstruction metrics (R/main.py:300-323): the ``metric`` module surface, the window values against
fixture F19 (tests/golden/f19_recon_metrics.npz, written with the real reference by tools/gen_golden_recon_metrics.py), the
torch-op path against the fp64 oracle (tests/_recon_metric_oracle.py has the bounds and their derivation), the two C-ABI
entry points and their host-side argument checks, and the aggregation of spkdiff.evaluate."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _recon_metric_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F19 = os.path.join(ROOT, "tests", "golden", "f19_recon_metrics.npz")


@pytest.fixture(scope="module")
def f19():
    return np.load(F19)


def test_metric_surface_and_signatures():
    import metric
    import metric.pytorch_ssim as ps
    assert metric.pytorch_ssim is ps
    for name in ("gaussian", "create_window", "SSIM", "ssim"):
        assert hasattr(ps, name), name
    assert list(inspect.signature(ps.gaussian).parameters) == ["window_size", "sigma"]
    assert list(inspect.signature(ps.create_window).parameters) == ["window_size", "channel"]
    sig = inspect.signature(ps.SSIM.__init__).parameters
    assert list(sig) == ["self", "window_size", "size_average"]
    assert sig["window_size"].default == 11 and sig["size_average"].default is True
    sig = inspect.signature(ps.ssim).parameters
    assert list(sig) == ["img1", "img2", "window_size", "size_average"]
    assert sig["window_size"].default == 11 and sig["size_average"].default is True
    m = ps.SSIM()
    assert isinstance(m, torch.nn.Module)
    assert (m.window_size, m.size_average, m.channel) == (11, True, 1)
    assert m.window.shape == (1, 1, 11, 11) and m.window.dtype == torch.float32
    # the cached window follows the channel count and the dtype of the input
    a = torch.rand(2, 3, 16, 16)
    m(a, a)
    assert m.channel == 3 and m.window.shape == (3, 1, 11, 11)
    m(a.double(), a.double())
    assert m.window.dtype == torch.float64 and m.channel == 3
    w = m.window
    m(a.double(), a.double())
    assert m.window is w


def test_window_values_bit_equal_to_the_reference(f19):
    import metric.pytorch_ssim as ps
    assert np.array_equal(ps.gaussian(11, 1.5).numpy(), f19["gaussian_11_1p5"])
    assert np.array_equal(ps.create_window(11, 1).numpy(), f19["window_11_c1"])
    assert np.array_equal(ps.create_window(11, 3).numpy(), f19["window_11_c3"])
    assert ps.create_window(11, 3).is_contiguous()


def test_fixture_holds_the_cases_and_its_oracle_values(f19):
    """F19 lists the eight cases, and its stored fp64 values are what the test-side oracle computes from its inputs."""
    import metric.pytorch_ssim as ps
    assert tuple(str(n) for n in f19["names"]) == orc.CASES
    shapes = {"strokes_blur": ((32, 1, 28, 28), 11), "strokes_noise": ((32, 1, 28, 28), 11), "rgb32": ((7, 3, 32, 32), 11),
              "c2_19x23_w7": ((5, 2, 19, 23), 7), "even_w8": ((3, 1, 28, 28), 8), "small9_w11": ((2, 1, 9, 9), 11)}
    for name in orc.CASES:
        c = orc.load_case(f19, name)
        assert c["a"].dtype == torch.float32 and c["a"].shape == c["b"].shape
        if name in shapes:
            assert (tuple(c["a"].shape), c["ws"]) == shapes[name]
        o_mean, o_per = orc.ssim64(c["a"], c["b"], ps.create_window(c["ws"], 1)[0, 0])
        assert abs(float(o_mean) - float(c["o_mean"])) <= 1e-12
        assert np.abs(o_per.numpy() - c["o_per"]).max() <= 1e-12
        assert abs(float(orc.mse64(c["a"], c["b"])) - float(c["o_mse"])) <= 1e-14
    assert torch.equal(orc.load_case(f19, "identical")["a"], orc.load_case(f19, "identical")["b"])


@pytest.mark.parametrize("name", orc.CASES)
def test_torch_path_on_cpu_within_the_bound(f19, name):
    """|cpu - o| <= 2 |r - o| + 2^-23 |o| on every F19 case, through SSIM (both forms) and ssim."""
    import metric.pytorch_ssim as ps
    c = orc.load_case(f19, name)
    a, b, ws = c["a"], c["b"], c["ws"]
    with torch.no_grad():
        got_mean = ps.SSIM(window_size=ws)(a, b)
        got_per = ps.SSIM(window_size=ws, size_average=False)(a, b)
        got_fn = ps.ssim(a, b, ws)
    assert got_mean.dtype == torch.float32 and got_mean.dim() == 0 and got_per.shape == (a.shape[0],)
    e_mean = abs(float(got_mean) - float(c["o_mean"]))
    e_fn = abs(float(got_fn) - float(c["o_mean"]))
    e_per = np.abs(got_per.double().numpy() - c["o_per"])
    print(f"{name}: cpu |mean - o| {e_mean:.3e} (bound {float(orc.cpu_bound(c['r_mean'], c['o_mean'])):.3e}), "
          f"max |per - o| {e_per.max():.3e}")
    assert e_mean <= orc.cpu_bound(c["r_mean"], c["o_mean"])
    assert e_fn <= orc.cpu_bound(c["r_fn"], c["o_mean"])
    assert (e_per <= orc.cpu_bound(c["r_per"], c["o_per"])).all()


def test_torch_path_identical_images_and_gradients():
    import metric.pytorch_ssim as ps
    from spkdiff import synth
    a = synth.stroke_images(4, seed=5) - 0.5
    assert float(ps.SSIM()(a, a.clone())) == 1.0
    assert float(ps.ssim(a, a.clone())) == 1.0
    assert torch.equal(ps.SSIM(size_average=False)(a, a.clone()), torch.ones(4))
    x = (a + 0.05 * torch.randn(a.shape, generator=torch.Generator().manual_seed(1))).requires_grad_(True)
    loss = 1 - ps.SSIM()(x, a)
    loss.backward()
    assert x.grad is not None and x.grad.shape == x.shape and torch.isfinite(x.grad).all() and float(x.grad.abs().sum()) > 0


def test_entry_points_declared_exported_and_bound():
    from spkdiff import _lib
    txt = open(os.path.join(ROOT, "include", "spkdiff.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("spk_ssim_mse_ws_bytes", "spk_ssim_mse"):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/spkdiff.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libspkdiff.so"
        assert name in _lib.EXPORTS
    assert _lib.lib.spk_ssim_mse_ws_bytes.restype is ctypes.c_longlong
    assert len(_lib.lib.spk_ssim_mse.argtypes) == 12
    assert _lib.version() == _lib.EXPECTED_VERSION == 106


def test_host_rejection_before_any_launch():
    """Null pointers and non-positive sizes: SPK_ERR_ARG (-1); a window above 31 or 2^31 tiles and more: SPK_ERR_UNSUPPORTED
    (-2).  Decided on the host before any launch: no GPU is needed (the non-null pointers here are host addresses)."""
    from spkdiff import _lib
    lib = _lib.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ok = [p, p, p, p, p, p]
    for k in range(6):
        args = list(ok)
        args[k] = None
        assert lib.spk_ssim_mse(*args, 1, 1, 8, 8, 3, None) == -1, f"null pointer argument {k}"
    assert lib.spk_ssim_mse(*ok, 1, 1, 8, 8, 0, None) == -1
    assert lib.spk_ssim_mse(*ok, 1, 1, 8, 8, -3, None) == -1
    assert lib.spk_ssim_mse(*ok, 1, 1, 8, 8, 32, None) == -2
    for sizes in ((0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (-1, 1, 8, 8)):
        assert lib.spk_ssim_mse(*ok, *sizes, 11, None) == -1, sizes
        assert lib.spk_ssim_mse_ws_bytes(*sizes, 11) == -1, sizes
    assert lib.spk_ssim_mse_ws_bytes(1, 1, 8, 8, 0) == -1
    assert lib.spk_ssim_mse_ws_bytes(1, 1, 8, 8, 32) == -2
    # planes x tiles must stay below 2^31
    assert lib.spk_ssim_mse(*ok, 2 ** 20, 2 ** 11, 8, 8, 11, None) == -2
    assert lib.spk_ssim_mse_ws_bytes(2 ** 20, 2 ** 11, 8, 8, 11) == -2
    assert lib.spk_ssim_mse_ws_bytes(2 ** 17, 1, 2 ** 12, 2 ** 12, 11) == -2       # 2^17 planes x 128 x 128 tiles = 2^31
    assert lib.spk_ssim_mse_ws_bytes(2 ** 16, 1, 2 ** 12, 2 ** 12, 11) == 16 * 2 ** 30
    # two fp64 partials per 32x32 tile of every output plane
    assert lib.spk_ssim_mse_ws_bytes(32, 1, 28, 28, 11) == 16 * 32
    assert lib.spk_ssim_mse_ws_bytes(7, 3, 32, 32, 11) == 16 * 21
    assert lib.spk_ssim_mse_ws_bytes(3, 1, 32, 32, 8) == 16 * 3 * 4          # a 33x33 map: four tiles
    assert lib.spk_ssim_mse_ws_bytes(2, 1, 300, 200, 31) == 16 * 2 * 10 * 7
    assert lib.spk_ssim_mse_ws_bytes(2, 1, 9, 9, 11) == 16 * 2               # a window larger than the image is legal


def test_ops_wrapper_refuses_cpu_tensors():
    from spkdiff import ops
    import metric.pytorch_ssim as ps
    a = torch.zeros(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ssim_mse(a, a, ps.create_window(3, 1)[0, 0])
    assert ops.ssim_mse_out_size(28, 11) == 28 and ops.ssim_mse_out_size(28, 8) == 29 and ops.ssim_mse_out_size(9, 11) == 9


def test_metric_stubs_raise():
    ns = {}
    exec("from metric.IS_score import *\nfrom metric.Fid_score import *", ns)
    with pytest.raises(NotImplementedError, match="inception_v3"):
        ns["inception_score"](None, cuda=True, batch_size=32, resize=True, splits=1)
    with pytest.raises(NotImplementedError, match="inception_v3"):
        ns["calculate_fid"](None, None, False, 32)


def test_aggregation_is_the_scripts_arithmetic():
    from spkdiff import evaluate
    g = torch.Generator().manual_seed(9)
    ssim_items = (0.05 + 0.1 * torch.rand(313, generator=g)).float().tolist()      # what .item() returns: fp32 as Python floats
    mse_items = (0.002 + 0.004 * torch.rand(313, generator=g)).float().tolist()
    res = evaluate.aggregate(ssim_items, mse_items)
    assert res["n_batches"] == 313
    assert res["loss_ssim"] == sum(ssim_items) / len(ssim_items) and res["loss_mse"] == sum(mse_items) / len(mse_items)
    assert res["loss_ssim_rounded"] == round(sum(ssim_items) / len(ssim_items), 3)
    assert res["loss_mse_rounded"] == round(sum(mse_items) / len(mse_items), 3)
    assert set(res) == {"loss_ssim", "loss_mse", "loss_ssim_rounded", "loss_mse_rounded", "n_batches"}
    with pytest.raises(ValueError):
        evaluate.aggregate([], [])
    sig = inspect.signature(evaluate.reconstruction_eval).parameters
    assert list(sig) == ["model", "batches", "T", "window_size"] and sig["T"].default == 16 and sig["window_size"].default == 11
