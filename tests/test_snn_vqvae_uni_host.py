"""CPU tests of the SNN_VQVAE_uni baseline's surface (no GPU): the star import exposes it and VectorQuantizer_uni, they take the
reference's constructor signatures (R/snn_model/vae_model.py:674-801) and attributes, SNN_VQVAE_uni has SNN_VQVAE's children and
state_dict keys (fixture F18, built from the real reference), the product path refuses CPU tensors as SNN_VQVAE's does, and
VQVAE stays out of scope."""
import inspect
import os

import numpy as np
import pytest
import torch

from spkdiff import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F18 = os.path.join(ROOT, "tests", "golden", "f18_snn_vqvae_uni.npz")


def _ns():
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    return ns


def _model(ns, name="SNN_VQVAE_uni"):
    model = ns[name](1, 16, 128, torch.tensor(1.0))
    ns["functional"].set_step_mode(net=model, step_mode='m')
    return model


def test_star_import_exposes_both_classes():
    ns = _ns()
    for name in ("SNN_VQVAE_uni", "VectorQuantizer_uni", "SNN_VQVAE", "functional"):
        assert name in ns, name
    assert isinstance(_model(ns), torch.nn.Module)


def test_signatures_and_attributes_match_the_reference():
    ns = _ns()
    sig = inspect.signature(ns["SNN_VQVAE_uni"].__init__)
    assert list(sig.parameters) == ["self", "in_dim", "embedding_dim", "num_embeddings", "data_variance", "commitment_cost"]
    assert sig.parameters["commitment_cost"].default == 0.25
    assert list(inspect.signature(ns["SNN_VQVAE_uni"].forward).parameters) == ["self", "x", "image"]
    assert list(inspect.signature(ns["VectorQuantizer_uni"].__init__).parameters) == [
        "self", "embedding_dim", "num_embeddings", "commitment_cost"]
    model = _model(ns)
    assert (model.in_dim, model.embedding_dim, model.num_embeddings) == (1, 16, 128)
    vq = model.vq_layer
    assert type(vq).__name__ == "VectorQuantizer_uni"
    assert (vq.embedding_dim, vq.num_embeddings, vq.commitment_cost, vq.num_step) == (16, 128, 0.25, 16)
    for name in ("memout", "psp", "alpha", "embeddings", "poisson", "get_code_indices", "quantize"):
        assert hasattr(vq, name), name
    for name in ("encoder", "decoder", "memout", "encode_images", "decode_tokens"):
        assert hasattr(model, name), name
    assert vq.print_usage is True and vq.usage is None          # (not in the reference: the print switch, the last statistic)


def test_state_dict_keys_and_shapes_equal_snn_vqvae_and_f18():
    ns = _ns()
    sd_uni, sd_vq = _model(ns).state_dict(), _model(ns, "SNN_VQVAE").state_dict()
    assert list(sd_uni) == list(sd_vq)
    assert {k: tuple(v.shape) for k, v in sd_uni.items()} == {k: tuple(v.shape) for k, v in sd_vq.items()}
    synth_sd = synth.synth_vqvae_state(synth.MNIST)
    model = _model(ns)
    model.load_state_dict(synth_sd)
    f = np.load(F18)
    assert str(f["state_checksum"]) == synth.state_checksum(synth_sd)      # the fixture's reference run used these weights
    params = {k[5:].split("/")[0] for k in f.files if k.startswith("grad/")}
    assert params == {n for n, _ in model.named_parameters()}


def _errors(model, x, img):
    try:
        model(x, img)
    except Exception as e:          # noqa: BLE001  (the type and message are what is compared)
        return type(e), str(e)
    return None


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_cpu_tensors_raise_the_snn_vqvae_errors(mode):
    ns = _ns()
    sd = synth.synth_vqvae_state(synth.MNIST)
    img = synth.stroke_images(2) - 0.5
    x = img.unsqueeze(0).repeat(16, 1, 1, 1, 1)
    got = []
    for name in ("SNN_VQVAE", "SNN_VQVAE_uni"):
        model = _model(ns, name)
        model.load_state_dict(sd)
        getattr(model, mode)()
        got.append(_errors(model, x, img))
    assert got[0] is not None and got[0] == got[1], got
    assert got[1][0] is RuntimeError and "no CPU path" in got[1][1]


def test_vqvae_still_raises():
    ns = _ns()
    with pytest.raises(NotImplementedError, match="SNN_VQVAE_uni"):
        ns["VQVAE"](1, 16, 128)
