"""GPU tests of the SNN_VAE baseline (spk_linear_lif_fwd, spk_svae_ar_fwd, snn_model.vae_model.SNN_VAE) against fixture F16,
which the real reference computed on the CPU with ``synth.synth_svae_state`` weights (tools/gen_golden_svae.py).  On those
dyadic weights every Linear sum is exact in fp32, so spikes, sampled z and the MLP layers' membrane potentials must match bit
for bit; decoded pixels are held to the 1e-4 max-abs bar of the F3/F4 decode tests."""
import os

import numpy as np
import pytest
import torch

from spkdiff import ops, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = os.path.join(ROOT, "tests", "golden", "f16_snn_vae.npz")
SEED_FWD, SEED_SAMPLE = 16, 1616          # tools/gen_golden_svae.py
PIX_TOL = 1e-4
MLP_NODES = ("before_latent_layer.1", "posterior.layers.1", "posterior.layers.3", "posterior.layers.5", "prior.layers.1",
             "prior.layers.3", "prior.layers.5", "decoder_input.1")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def f16():
    return np.load(F16)


@pytest.fixture(scope="module")
def sd():
    return synth.synth_svae_state()


def unpack(f, key):
    shape = tuple(int(s) for s in f[key + "_shape"])
    return torch.from_numpy(np.unpackbits(f[key], axis=-1, count=shape[-1]).reshape(shape)).float()


def make_model(sd, dev):
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    model = ns["SNN_VAE"]()
    ns["functional"].set_step_mode(net=model, step_mode='m')
    model = model.cuda(0)
    model.load_state_dict(sd)
    return model.eval(), ns["functional"]


def lif_ref(cur, v):
    """The reference neuron's fp32 eval update (SJ/activation_based/neuron.py:799-811, tau 2, v_th 1, hard reset 0)."""
    out = torch.empty_like(cur)
    for t in range(cur.shape[0]):
        v = v + (cur[t] - v) / 2.0
        s = (v >= 1.0).float()
        v = 0.0 * s + (1.0 - s) * v
        out[t] = s
    return out, v


def dyadic(shape, units, g):
    return torch.randint(-units, units + 1, shape, generator=g).float() * 2.0 ** -12


@pytest.mark.parametrize("n_in", [56, 112, 224, 784])
@pytest.mark.parametrize("n_out", [56, 112, 224, 784, 1120])
def test_linear_lif_kernel_bit_exact(dev, n_in, n_out):
    """Kernel a on u8 spikes with carried state, T in {1, 5, 16}: spikes and v equal an fp64-accumulating torch reference."""
    g = torch.Generator().manual_seed(n_in * 10007 + n_out)
    for T in (1, 5, 16):
        B = 7
        w = dyadic((n_out, n_in), 1024, g)
        b = dyadic((n_out,), 256, g) + 1.0
        x = (torch.rand(T, B, n_in, generator=g) < 0.3).to(torch.uint8)
        v0 = dyadic((B, n_out), 2048, g)
        v = v0.to(dev).contiguous()
        wd, bd = w.to(dev), b.to(dev)
        s1 = ops.linear_lif(x.to(dev), wd, bd, v)
        s2 = ops.linear_lif(x.flip(0).to(dev), wd, bd, v)           # second call: v carried in
        cur = lambda xx: ((xx.double() @ w.double().t()) + b.double()).float()
        r1, rv = lif_ref(cur(x), v0)
        r2, rv = lif_ref(cur(x.flip(0)), rv)
        assert torch.equal(s1.cpu().float(), r1) and torch.equal(s2.cpu().float(), r2), (T, n_in, n_out)
        assert torch.equal(v.cpu(), rv), (T, n_in, n_out)
        # fp32 input and layer.Linear's plain currents
        xf = x.float() * 0.5
        vf = v0.to(dev).contiguous()
        sf = ops.linear_lif(xf.to(dev), wd, bd, vf)
        rf, rvf = lif_ref(cur(xf), v0)
        assert torch.equal(sf.cpu().float(), rf) and torch.equal(vf.cpu(), rvf)
        y = ops.linear(xf.flatten(0, 1).to(dev), wd, bd)
        assert torch.equal(y.cpu(), cur(xf).flatten(0, 1))


def test_linear_lif_ptc_layouts(dev):
    """before_latent_layer reads the encoder's u8 PTC [B,7,7,T,16] in flatten(C,H,W) order; decoder_input writes it."""
    g = torch.Generator().manual_seed(5)
    B, T = 5, 16
    spikes = (torch.rand(T, B, 16, 7, 7, generator=g) < 0.3).to(torch.uint8)
    ptc = spikes.permute(1, 3, 4, 0, 2).contiguous()                       # [B,H,W,T,C]
    w, b = dyadic((56, 784), 1024, g), dyadic((56,), 256, g) + 1.0
    v = torch.zeros(B, 56, device=dev)
    s = ops.linear_lif(ptc.to(dev), w.to(dev), b.to(dev), v)
    r, rv = lif_ref(((spikes.flatten(2).double() @ w.double().t()) + b.double()).float(), torch.zeros(B, 56))
    assert torch.equal(s.cpu().float(), r) and torch.equal(v.cpu(), rv)
    z = (torch.rand(T, B, 56, generator=g) < 0.3).float()
    w2, b2 = dyadic((784, 56), 1024, g), dyadic((784,), 256, g) + 1.0
    v2 = torch.zeros(B, 784, device=dev)
    out = ops.linear_lif(z.to(dev), w2.to(dev), b2.to(dev), v2, out_ptc=(16, 7, 7))
    r2, _ = lif_ref(((z.double() @ w2.double().t()) + b2.double()).float(), torch.zeros(B, 784))
    assert torch.equal(out.cpu().float(), r2.view(T, B, 16, 7, 7).permute(1, 3, 4, 0, 2))


def test_layer_linear_step_modes(dev):
    from spikingjelly.activation_based import layer
    g = torch.Generator().manual_seed(9)
    lin = layer.Linear(112, 224).to(dev).eval()
    with torch.no_grad():
        lin.weight.copy_(dyadic((224, 112), 1024, g))
        lin.bias.copy_(dyadic((224,), 1024, g))
    x = torch.randint(-8, 9, (4, 3, 112), generator=g).float() * 0.125     # products on 2^-15, |sum| < 2^5: exact
    ref = ((x.double() @ lin.weight.detach().cpu().double().t()) + lin.bias.detach().cpu().double()).float()
    for mode in ('s', 'm'):
        lin.step_mode = mode
        with torch.no_grad():
            assert torch.equal(lin(x.to(dev)).cpu(), ref), mode


def test_posterior_loop_teacher_forced_from_f16(dev, f16, sd):
    model, _ = make_model(sd, dev)
    latent_x = unpack(f16, "latent_x").to(torch.uint8).to(dev)
    torch.manual_seed(SEED_FWD)
    with torch.inference_mode():
        z, q = model.posterior(latent_x, want_q_z=False)
    torch.cuda.synchronize()
    assert q is None
    assert torch.equal(z.cpu(), unpack(f16, "sampled_z"))
    for i in (1, 3, 5):
        assert torch.equal(model.posterior.layers[i].v.cpu(), torch.from_numpy(f16[f"v/posterior.layers.{i}"])), i


def test_eval_forward_end_to_end_f16(dev, f16, sd):
    model, functional = make_model(sd, dev)
    images = torch.from_numpy(f16["images"])
    x = images.unsqueeze(0).repeat(16, 1, 1, 1, 1).to(dev)
    from spkdiff.ops import IN_SEQ
    with torch.inference_mode():
        enc = model.encoder.snn_convs.run(x, IN_SEQ, final='ptc', stateful=False)['ptc']       # [B,7,7,T,16]
    enc = enc.permute(3, 0, 4, 1, 2).float().cpu()
    want = unpack(f16, "enc_spikes")
    same = (enc == want).flatten(2).all(-1).all(0)
    print(f"F16 encoder spikes equal on {int(same.sum())}/{len(same)} images")
    assert bool(same.all())
    torch.manual_seed(SEED_FWD)
    with torch.inference_mode():
        z, xr = model(x, images.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(z.cpu(), unpack(f16, "sampled_z"))
    for n in MLP_NODES:
        node = model.get_submodule(n)
        assert torch.equal(node.v.cpu(), torch.from_numpy(f16["v/" + n])), n
    for n in ("encoder.snn_convs.2", "encoder.snn_convs.5", "encoder.snn_convs.8"):
        assert float((model.get_submodule(n).v.cpu() - torch.from_numpy(f16["v/" + n])).abs().max()) <= 1e-5, n
    err = float((xr.cpu() - torch.from_numpy(f16["x_recon"])).abs().max())
    print(f"F16 x_recon max-abs err {err:.2e}, sampled_z equal")
    assert xr.shape == (8, 1, 28, 28) and err <= PIX_TOL
    functional.reset_net(model)
    assert all(isinstance(m.v, float) and m.v == 0.0 for m in model.modules() if hasattr(m, 'v_threshold'))


def test_two_samples_without_reset_f16(dev, f16, sd):
    model, functional = make_model(sd, dev)
    functional.reset_net(model)
    torch.manual_seed(SEED_SAMPLE)
    with torch.inference_mode():
        for c in range(2):
            sx, sz = model.sample(32)
            torch.cuda.synchronize()
            assert torch.equal(sz.cpu(), unpack(f16, f"sample{c}_z")), c
            for n in ("prior.layers.1", "prior.layers.3", "prior.layers.5", "decoder_input.1"):
                assert torch.equal(model.get_submodule(n).v.cpu(), torch.from_numpy(f16[f"sample{c}_v/{n}"])), (c, n)
            err = float((sx.cpu() - torch.from_numpy(f16[f"sample{c}_x"])).abs().max())
            print(f"F16 sample {c}: z equal, image max-abs err {err:.2e}")
            assert sx.shape == (32, 1, 28, 28) and err <= PIX_TOL


def test_main_py_snn_vae_call_sequence(dev, sd):
    """R/main.py:97-108,288-314,345-376 for --model snn-vae on synthetic weights."""
    ns = {}
    exec("from snn_model.snn_layers import *\nfrom snn_model.vae_model import *", ns)
    model = ns["SNN_VAE"]()
    ns["functional"].set_step_mode(net=model, step_mode='m')
    model = model.cuda(0)
    model.load_state_dict(sd)
    model.eval()
    norm_images = (synth.stroke_images(16) - 0.5).cuda(0)
    with torch.inference_mode():
        images_spike = norm_images.unsqueeze(0).repeat(16, 1, 1, 1, 1)
        e, recon_images = model(images_spike, norm_images)
        ns["functional"].reset_net(model)
        assert e.shape == (16, 16, 56) and recon_images.shape == norm_images.shape
        assert torch.nn.functional.mse_loss(recon_images, norm_images).item() >= 0
    sampled_x, sampled_z = model.sample(32)
    ns["functional"].reset_net(model)
    assert sampled_x.shape == (32, 1, 28, 28) and sampled_z.shape == (16, 32, 56)
    imgs = []
    for _ in range(3):
        sampled_x, sampled_z = model.sample(32)
        imgs.append(np.array(np.clip((sampled_x + 0.5).detach().cpu().numpy(), 0., 1.) * 255, dtype=np.uint8))
    assert np.concatenate(imgs).shape == (96, 1, 28, 28)
    assert isinstance(model.prior.layers[5].v, torch.Tensor)              # state carried across the repeated samples


def test_product_path_calls_no_framework_gemm(dev, sd, monkeypatch):
    model, functional = make_model(sd, dev)
    img = (synth.stroke_images(4) - 0.5).to(dev)

    def refuse(*a, **k):
        raise AssertionError("framework GEMM on the product path")

    for mod, name in ((torch.nn.functional, "linear"), (torch, "matmul"), (torch, "addmm"), (torch.Tensor, "matmul"),
                      (torch.Tensor, "__matmul__")):
        monkeypatch.setattr(mod, name, refuse)
    with torch.inference_mode():
        z, xr = model(img.unsqueeze(0).repeat(16, 1, 1, 1, 1), img)
        sx, sz = model.sample(4)
    torch.cuda.synchronize()
    assert z.shape == (16, 4, 56) and xr.shape == (4, 1, 28, 28) and sx.shape == (4, 1, 28, 28)
