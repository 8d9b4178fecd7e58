"""GPU tests of the SNN_VAE baseline's training step (csrc/svae_train.hip, spk_svae_ar_prefix_fwd, the train() branches of
snn_model.vae_model.SNN_VAE) against fp64 autograd restatements and fixture F17, which the real reference computed on the CPU
with ``synth.synth_svae_state`` weights (tools/gen_golden_svae_train.py)."""
import math
import os
import random

import numpy as np
import pytest
import torch

from spkdiff import ops, synth

from parity_report import record as parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F17 = os.path.join(ROOT, "tests", "golden", "f17_snn_vae_train.npz")
SEED0, SEED1 = 17, 1717                   # tools/gen_golden_svae_train.py
KERNEL_GRAD_TOL = 1e-5
STAGE_TOL = 1e-5
LOSS_TOL, GRAD_TOL, BN_TOL = 0.02, 0.05, 1e-4     # F10's bars for a whole iteration
PRE_BN_BIASES = ("encoder.snn_convs.0.bias", "encoder.snn_convs.3.bias", "encoder.snn_convs.6.bias",
                 "decoder.snn_convs.0.bias", "decoder.snn_convs.3.bias")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def f17():
    return np.load(F17)


@pytest.fixture(scope="module")
def sd():
    return synth.synth_svae_state()


def unpack(f, key):
    shape = tuple(int(s) for s in f[key + "_shape"])
    return torch.from_numpy(np.unpackbits(f[key], axis=-1, count=shape[-1]).reshape(shape)).float()


def rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), torch.as_tensor(b).double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def grad_rel(grad, f, key):
    """Rel L2 of a gradient against F17: whole, or for the large ones (tools/gen_golden_svae_train.py:put_grad) the worse of
    the stored entries' rel L2 and the norm's relative error."""
    if key in f.files:
        return rel_l2(grad, f[key])
    g = grad.detach().double().cpu().flatten()
    assert tuple(int(d) for d in f[key + "/shape"]) == tuple(grad.shape), key
    sub = f[key + "/sub"]
    step = g.numel() // sub.size
    idx = torch.arange(sub.size, dtype=torch.int64) * step + step // 2
    ref_norm = float(f[key + "/norm"])
    return max(rel_l2(g[idx], sub), abs(float(g.norm()) - ref_norm) / ref_norm)


def make_model(sd, dev):
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    model = ns["SNN_VAE"]()
    ns["functional"].set_step_mode(net=model, step_mode='m')
    model = model.cuda(0)
    model.load_state_dict(sd)
    return model.train(), ns["functional"]


def dyadic(shape, scale, g):
    return torch.randint(-64, 65, shape, generator=g).float() / scale


# ---------------------------------------------------------------------------------------------- 1. Linear + LIF kernels
class _Spike(torch.autograd.Function):
    """Heaviside whose value is the fp32 forward's spike, with the ATan(alpha 2) surrogate at h - 1."""

    @staticmethod
    def forward(ctx, h, s):
        ctx.save_for_backward(h)
        return s.clone()

    @staticmethod
    def backward(ctx, g):
        h, = ctx.saved_tensors
        x = h - 1.0
        return g * (1.0 / (1.0 + (math.pi / 2 * 2.0 * x) ** 2)), None


def lif_fp32(cur, v):
    """The reference's fp32 training forward (neuron.py charge / fire / hard reset, tau 2, v_th 1): spikes, h, v."""
    s_all, h_all = [], []
    for t in range(cur.shape[0]):
        h = v + (cur[t] - (v - 0.0)) / 2.0
        s = (h - 1.0 >= 0).float()
        v = (1.0 - s) * h + s * 0.0
        s_all.append(s)
        h_all.append(h)
    return torch.stack(s_all), torch.stack(h_all), v


def lif_fp64(cur, v, spikes):
    out = []
    for t in range(cur.shape[0]):
        h = v + (cur[t] - v) / 2.0
        s = _Spike.apply(h, spikes[t])
        v = (1.0 - s) * h
        out.append(s)
    return torch.stack(out)


@pytest.mark.parametrize("n_in,n_out,split,lif", [(784, 56, 0, True), (112, 112, 56, True), (224, 1120, 0, True),
                                                   (56, 784, 0, True), (112, 224, 0, False)])
def test_linear_lif_train_vs_fp64_autograd(dev, n_in, n_out, split, lif):
    g = torch.Generator().manual_seed(n_in * 7 + n_out)
    T, B = 16, 8
    x = (torch.rand(T, B, n_in, generator=g) < 0.3).float()
    w = dyadic((n_out, n_in), 4096 if n_in > 200 else 1024, g)
    b = dyadic((n_out,), 256, g) + (1.0 if lif else 0.0)
    v0 = torch.randint(0, 200, (B, n_out), generator=g).float() / 256
    gout = torch.randn(T, B, n_out, generator=g)
    xs = [x[..., :split], x[..., split:]] if split else [x]
    xd = [t.to(dev).requires_grad_() for t in xs]
    wd, bd = w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    vd = v0.to(dev).clone() if lif else None
    out = ops.LinearLIFTrainFunction.apply(xd[0], xd[1] if split else None, wd, bd, vd, lif)
    (out * gout.to(dev)).sum().backward()
    torch.cuda.synchronize()
    cur = (x.double() @ w.double().t() + b.double()).float()          # exact: dyadic products, |sum| < 2^8
    if lif:
        s_ref, h_ref, v_ref = lif_fp32(cur, v0)
        _, h_dev = ops.linear_lif_train_fwd(x.to(dev), w.to(dev), b.to(dev), v0.to(dev).clone())
        assert torch.equal(out.detach().cpu(), s_ref)
        assert torch.equal(h_dev.cpu(), h_ref)
        assert torch.equal(vd.cpu(), v_ref)
        rate = float(s_ref.mean())
        assert 0.02 < rate < 0.9, rate
    else:
        assert torch.equal(out.detach().cpu(), cur)
    x64 = x.double().requires_grad_()
    w64, b64 = w.double().requires_grad_(), b.double().requires_grad_()
    c64 = x64 @ w64.t() + b64
    o64 = lif_fp64(c64, v0.double(), s_ref.double()) if lif else c64
    (o64 * gout.double()).sum().backward()
    gx = torch.cat([t.grad.cpu() for t in xd], -1)
    errs = {"dx": rel_l2(gx, x64.grad), "dw": rel_l2(wd.grad, w64.grad), "db": rel_l2(bd.grad, b64.grad)}
    print(f"linear_lif_train {n_in}->{n_out} lif={lif}: rel L2 {errs}")
    parity(f"svae_train_linear_{n_in}x{n_out}_{'lif' if lif else 'cur'}", **errs)
    assert max(errs.values()) <= KERNEL_GRAD_TOL, errs


def test_layer_linear_trains_through_the_kernels(dev):
    from spikingjelly.activation_based import layer
    g = torch.Generator().manual_seed(3)
    lin = layer.Linear(112, 224, step_mode='m').to(dev).train()
    x = torch.randn(4, 3, 112, generator=g)
    xd = x.to(dev).requires_grad_()
    y = lin(xd)
    gy = torch.randn(4, 3, 224, generator=g)
    (y * gy.to(dev)).sum().backward()
    w64, b64 = lin.weight.detach().cpu().double().requires_grad_(), lin.bias.detach().cpu().double().requires_grad_()
    x64 = x.double().requires_grad_()
    y64 = x64 @ w64.t() + b64
    (y64 * gy.double()).sum().backward()
    assert rel_l2(y, y64) < 1e-6
    for a, r in ((xd.grad, x64.grad), (lin.weight.grad, w64.grad), (lin.bias.grad, b64.grad)):
        assert rel_l2(a, r) < KERNEL_GRAD_TOL


# ---------------------------------------------------------------------------------------------- 2. latent loss
def test_latent_loss_vs_autograd(dev):
    g = torch.Generator().manual_seed(11)
    T, B, C, k = 16, 8, 56, 20
    q = (torch.rand(T, B, C * k, generator=g) < 0.3).float()
    p = (torch.rand(T, B, C * k, generator=g) < 0.3).float()
    idx = torch.randint(0, k, (T, B, C), generator=g, dtype=torch.int32)
    gsz = torch.randn(T, B, C, generator=g)
    qd, pd = q.to(dev).requires_grad_(), p.to(dev).requires_grad_()
    sz, loss = ops.LatentLossFunction.apply(qd, pd, idx.to(dev), 2.0)
    (loss * 3.0 + (sz * gsz.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    q64, p64 = q.double().requires_grad_(), p.double().requires_grad_()
    sz64 = torch.gather(q64.view(T, B, C, k), 3, idx.long().unsqueeze(-1)).squeeze(-1)

    def psp(x):
        syn, out = torch.zeros_like(x[0]), []
        for t in range(T):
            syn = syn + (x[t] - syn) / 2.0
            out.append(syn)
        return torch.stack(out)

    l64 = torch.mean((psp(q64.view(T, B, C, k).mean(-1)) - psp(p64.view(T, B, C, k).mean(-1))) ** 2)
    (l64 * 3.0 + (sz64 * gsz.double()).sum()).backward()
    assert torch.equal(sz.detach().cpu(), sz64.detach().float())
    errs = {"loss": abs(float(loss) - float(l64)) / float(l64), "dq": rel_l2(qd.grad, q64.grad), "dp": rel_l2(pd.grad, p64.grad)}
    print("latent loss rel errors", errs)
    parity("svae_train_latent_loss", **errs)
    assert max(errs.values()) <= KERNEL_GRAD_TOL, errs


# ---------------------------------------------------------------------------------------------- 3. stage test against F17
def _stage(model, f17, dev, prefix, seed, p, monkeypatch=None):
    model.p = p
    latent_x = unpack(f17, "latent_x").to(dev).requires_grad_()
    noise = None
    if prefix:
        noise = list(torch.from_numpy(f17[prefix + "noise"]).to(dev))
        monkeypatch.setattr(torch, "randn_like", lambda t, *a, **k: noise.pop(0).clone())
    torch.manual_seed(seed)
    random.seed(seed)
    sampled_z, mmd, q_z, p_z, z_t_minus = model._latent_from(latent_x)
    gsz = torch.from_numpy(f17[prefix + "dl_dsampled_z"]).to(dev)
    (mmd + (sampled_z * gsz).sum()).backward()
    torch.cuda.synchronize()
    if noise is not None:
        assert noise == [], "every recorded randn_like draw consumed"
    return latent_x, sampled_z, mmd, q_z, p_z, z_t_minus


def test_latent_stage_matches_f17_p0(dev, f17, sd):
    model, _ = make_model(sd, dev)
    latent_x, sampled_z, mmd, q_z, p_z, z_t_minus = _stage(model, f17, dev, "", SEED0, 0)
    assert torch.equal(sampled_z.detach().cpu(), unpack(f17, "sampled_z"))
    assert torch.equal(q_z.detach().cpu(), unpack(f17, "q_z"))
    assert torch.equal(p_z.detach().cpu(), unpack(f17, "p_z"))
    assert torch.equal(z_t_minus.cpu(), unpack(f17, "z_t_minus"))
    for n in ("posterior.layers.1", "posterior.layers.3", "posterior.layers.5", "prior.layers.1", "prior.layers.3",
              "prior.layers.5"):
        assert torch.equal(dict(model.named_modules())[n].v.cpu(), torch.from_numpy(f17["v/" + n])), n
    errs = {"mmd": abs(float(mmd) - float(f17["loss_mmd"])) / float(f17["loss_mmd"]),
            "dl_dlatent_x": rel_l2(latent_x.grad, f17["dl_dlatent_x"])}
    for n, prm in model.named_parameters():
        if n.startswith(("posterior.", "prior.")):
            errs["grad/" + n] = grad_rel(prm.grad, f17, "grad/" + n)
    print("F17 stage (p = 0) rel errors", errs)
    parity("svae_train_stage_p0", max_rel=max(errs.values()), **{k: v for k, v in errs.items() if "/" not in k})
    assert max(errs.values()) <= STAGE_TOL, errs


def test_latent_stage_matches_f17_scheduled(dev, f17, sd, monkeypatch):
    model, _ = make_model(sd, dev)
    latent_x, sampled_z, mmd, q_z, p_z, z_t_minus = _stage(model, f17, dev, "p3/", SEED1, float(f17["p_sched"]), monkeypatch)
    assert torch.equal(sampled_z.detach().cpu(), unpack(f17, "p3/sampled_z"))
    assert torch.equal(z_t_minus.cpu(), unpack(f17, "p3/z_t_minus"))
    assert torch.equal(p_z.detach().cpu(), unpack(f17, "p3/p_z"))
    for n in ("prior.layers.1", "prior.layers.3", "prior.layers.5"):
        assert torch.equal(dict(model.named_modules())[n].v.cpu(), torch.from_numpy(f17["p3/v/" + n])), n
    errs = {"mmd": abs(float(mmd) - float(f17["p3/loss_mmd"])) / float(f17["p3/loss_mmd"])}
    params = dict(model.named_parameters())
    for n, prm in params.items():
        if n.startswith(("posterior.", "prior.")):
            ref = float(f17["p3/gnorm/" + n])
            errs["gnorm/" + n] = abs(float(prm.grad.norm()) - ref) / ref
    for n in ("prior.layers.0.weight", "prior.layers.0.bias", "prior.layers.2.weight", "prior.layers.2.bias",
              "prior.layers.4.bias"):
        errs["p3/grad/" + n] = grad_rel(params[n].grad, f17, "p3/grad/" + n)
    print("F17 stage (p = 0.3) rel errors", errs)
    parity("svae_train_stage_p03", max_rel=max(errs.values()), mmd=errs["mmd"])
    assert max(errs.values()) <= STAGE_TOL, errs


# ---------------------------------------------------------------------------------------------- 4. whole iteration
def _iteration(model, images, seed, capture=None):
    if capture is not None:
        inner = model._latent_from

        def spy(latent_x, scheduled=True):
            capture.append(latent_x.detach())
            return inner(latent_x, scheduled)
        model._latent_from = spy
    torch.manual_seed(seed)
    random.seed(seed)
    x = images.unsqueeze(0).repeat(16, 1, 1, 1, 1)
    loss_mmd, loss_rec = model(x, images)
    (loss_mmd + loss_rec).backward()
    torch.cuda.synchronize()
    if capture is not None:
        del model._latent_from
    return float(loss_mmd), float(loss_rec)


@pytest.mark.parametrize("exact", [True, False], ids=["exact_forward", "default"])
def test_training_iteration_matches_f17(dev, f17, sd, exact):
    keep = ops.EXACT_TRAIN_FORWARD_MACS, ops.NATIVE_TRAIN_FORWARD
    if exact:
        ops.EXACT_TRAIN_FORWARD_MACS, ops.NATIVE_TRAIN_FORWARD = 1 << 62, False
    try:
        model, _ = make_model(sd, dev)
        images = torch.from_numpy(f17["images"]).to(dev)
        cap = []
        l_mmd, l_rec = _iteration(model, images, SEED0, cap)
    finally:
        ops.EXACT_TRAIN_FORWARD_MACS, ops.NATIVE_TRAIN_FORWARD = keep
    lx_ref = unpack(f17, "latent_x")
    lx_diff = int((cap[0].cpu() != lx_ref).sum())
    res = {"loss_mmd": abs(l_mmd - float(f17["loss_mmd"])) / float(f17["loss_mmd"]),
           "loss_rec": abs(l_rec - float(f17["loss_rec"])) / float(f17["loss_rec"]), "latent_x_diff": lx_diff}
    grad_err, zero_grad = {}, {}
    for n, prm in model.named_parameters():
        if n in PRE_BN_BIASES:                    # conv biases in front of a batch-statistics BN: zero gradient (as F10);
            zero_grad[n] = float(prm.grad.norm())  # the reference's are rounding noise (1e-9 .. 1e-5)
        else:
            grad_err[n] = grad_rel(prm.grad, f17, "grad/" + n)
    bn_err = {n: float((b.detach().cpu() - torch.from_numpy(f17["bn/" + n])).abs().max())
              for n, b in model.named_buffers() if "bn/" + n in f17.files}
    res["max_grad_rel_l2"] = max(grad_err.values())
    res["max_bn_abs"] = max(bn_err.values())
    print(f"F17 whole iteration ({'exact' if exact else 'default'} forward): {res}")
    print("  worst gradients:", sorted(grad_err.items(), key=lambda kv: -kv[1])[:4])
    parity(f"svae_train_iteration_{'exact' if exact else 'default'}", **res)
    assert res["loss_mmd"] <= LOSS_TOL and res["loss_rec"] <= LOSS_TOL, res
    assert res["max_grad_rel_l2"] <= GRAD_TOL, sorted(grad_err.items(), key=lambda kv: -kv[1])[:4]
    assert res["max_bn_abs"] <= BN_TOL, bn_err
    assert all(v <= 1e-4 for v in zero_grad.values()), zero_grad
    if lx_diff == 0:
        # the same latent spikes and draws: the latent model's outputs are the reference's bit for bit
        for n in ("posterior.layers.5", "prior.layers.5"):
            assert torch.equal(dict(model.named_modules())[n].v.cpu(), torch.from_numpy(f17["v/" + n])), n


# ---------------------------------------------------------------------------------------------- 5. determinism
def test_training_iteration_is_deterministic(dev, sd):
    images = (synth.stroke_images(8, seed=5) - 0.5).to(dev)
    grads = []
    for _ in range(2):
        model, functional = make_model(sd, dev)
        model.p = 0.3
        _iteration(model, images, 99)
        grads.append({n: prm.grad.clone() for n, prm in model.named_parameters()})
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n


# ---------------------------------------------------------------------------------------------- 6. no framework GEMM
def test_training_calls_no_framework_gemm_or_convolution(dev, sd, monkeypatch):
    model, _ = make_model(sd, dev)
    images = (synth.stroke_images(4) - 0.5).to(dev)

    def refuse(*a, **k):
        raise AssertionError("framework GEMM / convolution on the training path")

    for mod, name in ((torch.nn.functional, "linear"), (torch, "matmul"), (torch, "mm"), (torch, "addmm"), (torch, "bmm"),
                      (torch.Tensor, "matmul"), (torch.Tensor, "__matmul__"), (torch.nn.functional, "conv2d"),
                      (torch.nn.functional, "conv_transpose2d")):
        monkeypatch.setattr(mod, name, refuse)
    model.p = 0.3
    _iteration(model, images, 5)
    assert all(prm.grad is not None and bool(torch.isfinite(prm.grad).all()) for prm in model.parameters())


# ---------------------------------------------------------------------------------------------- 7. the R/main.py loop
def test_main_py_training_loop_for_snn_vae(dev):
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    functional = ns["functional"]
    torch.manual_seed(0)
    model = ns["SNN_VAE"]()
    functional.set_step_mode(net=model, step_mode='m')
    model = model.cuda(0)
    keys = list(model.state_dict().keys())
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-3)
    images_all = (synth.stroke_images(48, seed=7) - 0.5).to(dev)
    model.train()
    for it in range(3):
        images = images_all[it * 16:(it + 1) * 16]
        images_spike = images.unsqueeze(0).repeat(16, 1, 1, 1, 1)
        optimizer.zero_grad()
        loss_eq, loss_rec = model(images_spike, images)
        loss = loss_eq + loss_rec
        loss.backward()
        optimizer.step()
        functional.reset_net(model)
        assert math.isfinite(float(loss_eq)) and math.isfinite(float(loss_rec)), (it, float(loss_eq), float(loss_rec))
    moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(moved) >= len(before) - 2, sorted(set(before) - set(moved))
    model.eval()
    with torch.no_grad():
        images = images_all[:16]
        sampled_z, x_recon = model(images.unsqueeze(0).repeat(16, 1, 1, 1, 1), images)
        functional.reset_net(model)
        sx, sz = model.sample(16)
        functional.reset_net(model)
    torch.cuda.synchronize()
    assert x_recon.shape == (16, 1, 28, 28) and sx.shape == (16, 1, 28, 28) and sz.shape == (16, 16, 56)
    assert bool(torch.isfinite(x_recon).all()) and bool(torch.isfinite(sx).all())
    assert list(model.state_dict().keys()) == keys
