"""CPU tests of the SNN_VAE baseline's surface (no GPU): the star import exposes it, it constructs with the reference's
children and state_dict keys (fixture F16, built from the real reference), the product path refuses CPU tensors and the
training branch, and the synthetic weights sit on the exact 2^-12 grid the bit-exact GPU tests rely on."""
import os

import numpy as np
import pytest
import torch

from spkdiff import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = os.path.join(ROOT, "tests", "golden", "f16_snn_vae.npz")


def _model():
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    model = ns["SNN_VAE"]()
    ns["functional"].set_step_mode(net=model, step_mode='m')
    return model, ns


def test_star_import_exposes_a_constructible_snn_vae():
    model, ns = _model()
    for name in ("SNN_VAE", "PriorBernoulliSTBP", "PosteriorBernoulliSTBP", "functional"):
        assert name in ns, name
    assert model.latent_dim == 56 and model.n_steps == 16 and model.k == 20 and model.p == 0
    for meth in ("encode", "decode", "sample", "forward", "loss_function_mmd", "weight_clipper", "update_p"):
        assert callable(getattr(model, meth)), meth
    assert model.prior.k == 20 and model.posterior.k == 20
    with pytest.raises(NotImplementedError):
        ns["VQVAE"](1, 16, 128)          # the other baselines stay out of scope


def test_state_dict_keys_and_shapes_equal_the_reference():
    model, _ = _model()
    sd = model.state_dict()
    assert len(sd) == 56
    for k in ("prior.initial_input", "posterior.initial_input", "membrane_output_layer.coef"):
        assert k in sd, k
    synth_sd = synth.synth_svae_state()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in synth_sd.items()}
    model.load_state_dict(synth_sd)
    f = np.load(F16)
    assert str(f["state_checksum"]) == synth.state_checksum(synth_sd)      # the fixture's reference run used these weights
    # the fixture stores the state of every LIFNode of the reference module tree but the decoder's
    nodes = {n for n, m in model.named_modules() if type(m).__name__ == "LIFNode" and not n.startswith("decoder.")}
    assert nodes == {k[2:] for k in f.files if k.startswith("v/")}


def test_cpu_forward_and_sample_refuse_instead_of_falling_back():
    model, _ = _model()
    model.load_state_dict(synth.synth_svae_state())
    model.eval()
    img = synth.stroke_images(2) - 0.5
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(img.unsqueeze(0).repeat(16, 1, 1, 1, 1), img)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.sample(2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.before_latent_layer[0](torch.zeros(4, 784))


def test_train_mode_forward_is_out_of_scope():
    model, _ = _model()
    model.train()
    img = synth.stroke_images(2) - 0.5
    with pytest.raises(NotImplementedError, match="SNN_VAE.forward in train"):
        model(img.unsqueeze(0).repeat(16, 1, 1, 1, 1), img)


def test_plain_torch_helpers():
    model, _ = _model()
    model.update_p(5, 10)
    assert abs(model.p - 0.2) < 1e-12
    with torch.no_grad():
        model.prior.layers[0].weight.fill_(7.0)
    model.weight_clipper()
    assert float(model.prior.layers[0].weight.detach().max()) == 4.0


def test_synth_svae_state_is_on_the_dyadic_grid():
    sd = synth.synth_svae_state()
    lin = [k for k in sd if k.startswith(("before_latent_layer.", "decoder_input.", "prior.layers.", "posterior.layers."))]
    assert len(lin) == 16
    for k in lin:
        v = sd[k].double()
        assert bool(((v * 4096).round() == v * 4096).all()), k
        if k.endswith("weight"):
            assert float(v.abs().max()) <= 0.25, k
            # largest fan-in 784: every spike-weighted sum plus bias stays below 2^8 (exact in fp32)
            assert v.shape[1] * 0.25 + float(sd[k[:-6] + "bias"].abs().max()) < 256, k
    a, b = synth.synth_svae_state(), synth.synth_svae_state()
    assert all(torch.equal(a[k], b[k]) for k in a)
