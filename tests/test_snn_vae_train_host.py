"""Host-side tests of the SNN_VAE training path (no GPU): the new entry points are declared and exported, reject bad arguments
before any launch, the ops wrappers check shapes, fixture F17 belongs to ``synth.synth_svae_state`` and has the reference's
shapes, and train() without autograd stays out of scope."""
import os
import re

import numpy as np
import pytest
import torch

from spkdiff import _lib, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F17 = os.path.join(ROOT, "tests", "golden", "f17_snn_vae_train.npz")
NEW = ("spk_svae_ar_prefix_fwd", "spk_linear_lif_train_fwd", "spk_linear_lif_train_bwd", "spk_svae_latent_loss_ws_floats",
       "spk_svae_latent_loss_fwd", "spk_svae_latent_loss_bwd")


def test_new_symbols_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "spkdiff.h")) as f:
        header = f.read()
    for n in NEW:
        assert re.search(r"\b" + n + r"\(", header), n
        assert n in _lib.EXPORTS and hasattr(_lib.lib, n), n


def test_entry_points_reject_bad_arguments_on_the_host():
    L = _lib.lib
    d = ctypes_dummy = 4096           # any non-null address: every call below is rejected before a launch
    assert L.spk_linear_lif_train_fwd(None, 0, 4, None, 0, 0, d, None, None, d, d, d, 1, 2, 2, 4, None) == -1
    assert L.spk_linear_lif_train_fwd(d, 0, 4, None, 0, 0, d, None, None, d, None, None, 1, 2, 2, 4, None) == -1   # lif: no h
    assert L.spk_linear_lif_train_fwd(d, 0, 4, None, 0, 0, d, None, None, d, d, d, 1, 0, 2, 4, None) == -1        # T = 0
    assert L.spk_linear_lif_train_fwd(d, 3, 4, None, 0, 0, d, None, None, d, d, d, 1, 2, 2, 4, None) == -1        # bad kind
    assert L.spk_linear_lif_train_fwd(d, 0, 4, None, 0, 5, d, None, None, d, d, d, 1, 2, 2, 4, None) == -1        # x2 size, no x2
    assert L.spk_linear_lif_train_bwd(None, None, None, d, 0, 4, None, 0, 0, d, None, 0, d, None, 2, 2, 4, None) == -1
    assert L.spk_linear_lif_train_bwd(d, d, None, d, 0, 4, None, 0, 0, d, None, 0, d, None, 2, 2, 4, None) == -1  # h, no ws
    assert L.spk_linear_lif_train_bwd(d, None, None, d, 0, 4, None, 0, 0, d, d, 5, d, None, 2, 2, 4, None) == -1   # cols > in
    assert L.spk_svae_latent_loss_ws_floats(0, 56) == -1
    assert L.spk_svae_latent_loss_fwd(None, None, d, d, None, None, 16, 2, 56, 20, 2.0, None) == -1
    assert L.spk_svae_latent_loss_fwd(d, d, d, d, None, None, 16, 2, 56, 20, 2.0, None) == -1                     # p_z, no loss
    assert L.spk_svae_latent_loss_fwd(d, None, d, d, None, None, 17, 2, 56, 20, 2.0, None) == -1                  # T > 16
    assert L.spk_svae_latent_loss_bwd(d, None, d, d, None, d, None, 16, 2, 56, 20, 2.0, None) == -1               # g_loss, no p_z
    assert L.spk_svae_latent_loss_bwd(d, d, d, None, None, None, None, 16, 2, 56, 20, 2.0, None) == -1            # no grad_q_z
    args = [d] * 11
    assert L.spk_svae_ar_prefix_fwd(*args, None, None, None, None, d, 16, 2, 56, 56, 112, 224, 20, None) == -1   # post: no idx
    assert L.spk_svae_ar_prefix_fwd(None, *args[1:], None, d, None, d, d, 16, 2, 0, 56, 112, 224, 20, None) == -1  # prior: noise
    assert L.spk_svae_ar_prefix_fwd(None, *args[1:], None, d, d, d, d, 1, 2, 0, 56, 112, 224, 20, None) == -1     # T < 2
    del ctypes_dummy


def test_ops_wrappers_check_shapes_before_the_device():
    meta = torch.device("meta")
    with pytest.raises(ValueError):
        ops.linear_lif_train_fwd(torch.zeros(4, 3), torch.zeros(5, 3), None)         # not [T,B,in]
    with pytest.raises(ValueError):
        ops.svae_ar_prefix(None, torch.zeros(56), [(None, None)] * 3, [None] * 3)      # prior without its schedule
    with pytest.raises((ValueError, RuntimeError)):
        ops.LatentLossFunction.apply(torch.zeros(16, 2, 1120, device=meta), None, torch.zeros(16, 2, 56, dtype=torch.int32), 2.0)
    # CPU tensors are refused: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linear_lif_train_fwd(torch.zeros(2, 2, 4), torch.zeros(3, 4), None, lif=False)


def test_f17_belongs_to_the_synthetic_state_and_has_the_reference_shapes():
    assert os.path.getsize(F17) < 600_000, "F17 must stay a small test vector"
    f = np.load(F17)
    sd = synth.synth_svae_state()
    assert str(f["state_checksum"]) == synth.state_checksum(sd)
    T, B, C, k = 16, 8, 56, 20
    for key, shape in (("latent_x", (T, B, C)), ("sampled_z", (T, B, C)), ("q_z", (T, B, C * k)), ("p_z", (T, B, C * k)),
                       ("z_t_minus", (T, B, C)), ("p3/z_t_minus", (T, B, C)), ("p3/p_z", (T, B, C * k))):
        assert tuple(int(s) for s in f[key + "_shape"]) == shape, key
    assert f["dl_dlatent_x"].shape == (T, B, C) and f["dl_dsampled_z"].shape == (T, B, C)
    assert f["idx"].shape == (T, B, C) and f["idx"].min() >= 0 and f["idx"].max() < k
    sched = f["p3/sched"]
    assert sched.shape == (T - 1,) and not sched[:5].any() and f["p3/noise"].shape == (int(sched.sum()), B, C)
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    params = dict(ns["SNN_VAE"]().named_parameters())
    for n, v in sd.items():
        if n not in params:                     # buffers carry no gradient
            continue
        if "grad/" + n in f.files:
            assert f["grad/" + n].shape == tuple(v.shape), n
        else:                                   # large gradients: norm + a fixed-stride sample (gen_golden_svae_train.py)
            assert tuple(f["grad/" + n + "/shape"]) == tuple(v.shape) and f["grad/" + n + "/sub"].size < v.numel(), n
            assert float(f["grad/" + n + "/norm"]) > 0, n
    assert all(0.05 <= r <= 0.5 for r in f["rates"])


def test_train_mode_without_autograd_is_out_of_scope():
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    model = ns["SNN_VAE"]()
    ns["functional"].set_step_mode(net=model, step_mode='m')
    model.train()
    img = synth.stroke_images(2) - 0.5
    with torch.no_grad(), pytest.raises(NotImplementedError):
        model(img.unsqueeze(0).repeat(16, 1, 1, 1, 1), img)
    with pytest.raises(NotImplementedError, match="SNN_VAE.forward in train"):
        model(img.unsqueeze(0).repeat(16, 1, 1, 1, 1), img)
