"""CPU tests of the plain-CNN VQVAE baseline (no GPU): the class constructs with the reference's children and
state_dict keys (fixture F20, built from the real reference), its module path -- the reference's operators, which CPU tensors
take -- meets F20 in eval and over one training iteration, the fp64 oracle the GPU tests use meets F20, the new entry points
are declared and bound, and every case of the GPU table satisfies the condition under which the index rule is meaningful."""
import inspect

import numpy as np
import pytest
import torch

import _ann_vqvae_oracle as orc
from spkdiff import synth


def _ns():
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    return ns


def _model(train=False):
    f = orc.fixture()
    m = _ns()["VQVAE"](1, 16, 128, torch.tensor(float(f["data_variance"])))
    m.load_state_dict(orc.state("mnist_k128"))
    return m.train() if train else m.eval()


def test_vqvae_constructs_with_the_reference_surface():
    ns = _ns()
    for name in ("VQVAE", "CNN_Encoder", "CNN_Decoder", "CNN_VectorQuantizer"):
        assert name in ns, name
    m = ns["VQVAE"](1, 16, 128, torch.tensor(1.0))
    assert isinstance(m, torch.nn.Module)
    sig = inspect.signature(ns["VQVAE"].__init__)
    assert list(sig.parameters) == ["self", "in_dim", "embedding_dim", "num_embeddings", "data_variance", "commitment_cost"]
    assert sig.parameters["commitment_cost"].default == 0.25
    assert list(inspect.signature(ns["VQVAE"].forward).parameters) == ["self", "x"]
    assert list(inspect.signature(ns["CNN_VectorQuantizer"].__init__).parameters) == [
        "self", "embedding_dim", "num_embeddings", "commitment_cost"]
    assert inspect.signature(ns["CNN_Encoder"].__init__).parameters["in_dim"].default == 3
    assert inspect.signature(ns["CNN_Decoder"].__init__).parameters["out_dim"].default == 1
    assert (m.in_dim, m.embedding_dim, m.num_embeddings) == (1, 16, 128)
    with pytest.raises(TypeError, match="data_variance"):           # the reference's error for the three-argument call
        ns["VQVAE"](1, 16, 128)
    assert (m.vq_layer.embedding_dim, m.vq_layer.num_embeddings, m.vq_layer.commitment_cost) == (16, 128, 0.25)
    for name in ("encode_images", "decode_tokens"):
        assert callable(getattr(m, name)), name


def test_state_dict_keys_equal_f20_and_take_the_synthetic_state():
    f = orc.fixture()
    m = _ns()["VQVAE"](1, 16, 128, torch.tensor(1.0))
    assert list(m.state_dict()) == [str(k) for k in f["state_keys"]]
    sd = orc.state("mnist_k128")
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict(sd)
    assert str(f["state_checksum"]) == synth.state_checksum(sd)      # the fixture's reference run used these weights
    assert {k[5:].split("/")[0] for k in f if k.startswith("grad/")} == {n for n, _ in m.named_parameters()}


def test_f20_satisfies_the_index_rules_condition():
    f = orc.fixture()
    d64 = orc.distances64(torch.from_numpy(f["z64"]), orc.state("mnist_k128"))
    assert torch.equal(torch.argmin(d64, dim=1), torch.from_numpy(f["indices64"]))
    assert orc.fragile_share(d64) <= orc.MAX_FRAGILE_SHARE
    assert abs(orc.fragile_share(d64) - float(f["fragile_share"])) < 1e-12
    assert 1e-7 < float(f["err_rel_dist"]) < 1e-5 and 0 < orc.pixel_bound() <= 1e-4        # fp32 round-off sized: a sanity bracket


def test_module_path_on_cpu_meets_f20_in_eval():
    f = orc.fixture()
    m = _model()
    images = torch.from_numpy(f["images"])
    with torch.inference_mode():
        e, x_recon, enco = m(images)
        tok = m.encode_images(images)
        pred, u8 = m.decode_tokens(torch.from_numpy(f["indices64"]).view(8, 7, 7))
    assert e.shape == (8, 16, 7, 7) and x_recon.shape == (8, 1, 28, 28) and enco.shape == (392,) and enco.dtype == torch.int64
    assert torch.equal(tok.reshape(-1), enco) and tok.shape == (8, 7, 7)
    d64 = orc.distances64(torch.from_numpy(f["z64"]), orc.state("mnist_k128"))
    n_diff, worst = orc.check_indices(d64, enco, "module path")
    err = float((pred.double() - torch.from_numpy(f["x_recon64"])).abs().max())
    print(f"module path: {int((enco != torch.from_numpy(f['indices'])).sum())} indices differ from the fp32 reference's, {n_diff} "
          f"from the fp64 one's (worst slack {worst:.3g} tau); pixel err {err:.3g} (bound {orc.pixel_bound():.3g})")
    assert err <= orc.pixel_bound()
    assert u8.dtype == torch.uint8 and torch.equal(u8, orc.uint8_rule(pred))
    assert torch.equal(e, m.vq_layer.embeddings.weight.detach()[enco].view(8, 7, 7, 16).permute(0, 3, 1, 2))


def _grad_entries(g):
    g = g.detach().numpy().reshape(-1)
    return g[orc.sub_index(g.size)] if g.size > orc.SUB else g


def test_module_path_training_iteration_meets_f20():
    """R/main.py:139-142: (loss_eq + loss_rec).backward() on a fresh model; losses and gradients against the fixture's fp64
    values within 8 x the fp32 reference's own error for that tensor."""
    f = orc.fixture()
    m = _model(train=True)
    images = torch.from_numpy(f["images"])
    loss_eq, loss_rec, real = m(images)
    (loss_eq + loss_rec).backward()
    for name, v in (("loss_eq", loss_eq), ("loss_rec", loss_rec), ("real_loss_rec", real)):
        err, bound = abs(float(v.detach()) - float(f["loss64/" + name])), 8 * float(f["err_loss/" + name])
        print(f"{name}: {float(v.detach()):.9g} vs fp64 {float(f['loss64/' + name]):.9g}: err {err:.3g}, bound {bound:.3g}")
        assert err <= bound, name
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        big = p.numel() > orc.SUB
        want = f["grad64/" + n + "/sub"] if big else f["grad64/" + n].reshape(-1)
        err, bound = float(np.abs(_grad_entries(p.grad).astype(np.float64) - want).max()), 8 * float(f["err_grad/" + n])
        print(f"grad {n}: err {err:.3g}, bound {bound:.3g}")
        assert err <= bound, n
        if big:
            nerr = abs(float(p.grad.double().norm()) - float(f["grad64/" + n + "/norm"]))
            assert nerr <= 8 * float(f["err_gradnorm/" + n]), n
            assert tuple(f["grad64/" + n + "/shape"]) == tuple(p.shape)


def test_oracle_meets_f20():
    f = orc.fixture()
    r = orc.forward64(orc.state("mnist_k128"), torch.from_numpy(f["images"]))
    assert torch.equal(r["idx"], torch.from_numpy(f["indices64"]))
    assert torch.equal(r["e"], torch.from_numpy(f["e64"]))
    # the same fp64 operators on the same values; only the library's blocking may differ between two machines
    assert float((r["z"] - torch.from_numpy(f["z64"])).abs().max()) <= 1e-12
    assert float((r["x_recon"] - torch.from_numpy(f["x_recon64"])).abs().max()) <= 1e-12
    tok = r["idx"].view(8, 7, 7).clone()
    tok[0, 0, 0], tok[1, 6, 6] = 128, -1                             # the mask id and a negative token embed as NaN
    e = orc.embed64(orc.state("mnist_k128"), tok)
    assert bool(torch.isnan(e[0, :, 0, 0]).all()) and bool(torch.isnan(e[1, :, 6, 6]).all()) and int(torch.isnan(e).sum()) == 32
    assert torch.equal(orc.uint8_rule(torch.tensor([-0.6, -0.5, 0.0, 0.4999, 0.5, 0.7])),
                       torch.tensor([0, 0, 127, 254, 255, 255], dtype=torch.uint8))


def test_header_declares_and_binds_the_new_entry_points():
    from spkdiff import _lib, ops
    for name in ("spk_ann_vqvae_supported", "spk_ann_vqvae_encode", "spk_ann_vqvae_decode", "spk_ann_vqvae_decode_ws_bytes"):
        assert name in _lib.EXPORTS, name
        assert getattr(_lib.lib, name).argtypes is not None
    assert _lib.version() == _lib.EXPECTED_VERSION == 106
    for C, H, K, want in ((1, 28, 128, True), (3, 32, 256, True), (1, 28, 100, True), (3, 28, 2, True), (1, 32, 512, True),
                          (1, 32, 513, True), (2, 28, 128, False), (1, 30, 128, False), (1, 28, 1, False),
                          (1, 28, ops.ANN_VQVAE_MAX_K + 1, False)):
        assert ops.ann_vqvae_supported(C, H, H, 16, K) is want, (C, H, K)
    assert not ops.ann_vqvae_supported(1, 28, 32, 16, 128) and not ops.ann_vqvae_supported(1, 28, 28, 32, 128)
    assert ops.ANN_VQVAE_D == 16 and ops.ANN_VQVAE_MAX_K >= 512 and ops.ANN_VQVAE_GROUP >= 1 and ops.ANN_VQVAE_GRID_CAP >= 1
    assert _lib.lib.spk_ann_vqvae_decode_ws_bytes(3, 28, 28) == 3 * 32 * 28 * 28 * 4
    with pytest.raises(RuntimeError, match="no CPU path"):          # the wrappers refuse CPU tensors; the MODEL routes them
        ops.ann_vqvae_encode(torch.zeros(1, 1, 28, 28), [torch.zeros(1)] * 6, torch.zeros(128, 16))


def test_every_gpu_case_satisfies_the_fragile_share_condition():
    from spkdiff import ops
    table = orc.cases(ops.ANN_VQVAE_GROUP, ops.ANN_VQVAE_GRID_CAP)
    n_ref = orc.batch_sizes(ops.ANN_VQVAE_GROUP, ops.ANN_VQVAE_GRID_CAP)[-1]
    assert {b for _, _, _, b in table} >= {1, 3, 33, ops.ANN_VQVAE_GROUP + 1, ops.ANN_VQVAE_GROUP * ops.ANN_VQVAE_GRID_CAP + 1}
    assert {(cfg.in_dim, cfg.img, K) for _, cfg, K, _ in table} == {(1, 28, 128), (3, 32, 256), (1, 28, 100)}
    for name, cfg, K, B in table:
        _, r = orc.reference(name, n_ref)
        d = r["d"][:B * cfg.tokens]
        share = orc.fragile_share(d)
        print(f"{name} B={B}: fragile share {share:.5f}, {int(r['idx'][:B * cfg.tokens].unique().numel())} of {K} codes used")
        assert share <= orc.MAX_FRAGILE_SHARE, (name, B)
        assert r["idx"][:B * cfg.tokens].unique().numel() >= (2 if B == 1 else 8)      # (not a collapsed codebook)
