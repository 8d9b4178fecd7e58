"""GPU tests of the SNN_VAE kernels (csrc/svae.hip, csrc/svae_train.hip) at the shapes fixtures F16/F17 do not reach, against
the host oracle (oracle/snn_ref.py, SNN_VAE section, pinned to F16/F17 by tests/test_oracle_svae.py) or fp64 autograd:
  * the autoregressive loops above B = 256, where ar_tile() switches to 4 images per workgroup, with ragged last tiles;
  * loop geometries other than the model's: odd cx + cz, h1/h2 > 256, k = 1 and 3, T = 1 / 2 / 5, v carried in;
  * the training GEMMs' ragged K and row tiles, the bias column in its own tile, grad_x_cols < nin, u8 input, no bias;
  * the latent loss with more partials than one reduction workgroup, T < 16, k = 1, tau_s != 2 and the gather alone.
The Linear weights are dyadic (synth._linear_lif_calibrated: multiples of 2^-12, |w| <= 0.25), so every sum is exact in fp32
and spikes, z, q_z and every membrane potential must equal the oracle's bit for bit."""
import functools
import random

import pytest
import torch

from oracle import snn_ref as ref
from spkdiff import ops, synth

from test_gpu_snn_vae_train import lif_fp32, lif_fp64, rel_l2

pytestmark = pytest.mark.gpu

BS = (1, 3, 256, 257, 259, 260, 513)      # 256 -> 257 crosses the 4-image tile; last tiles of 1, 3 and 4 images
GEOMS = {                                 # (cx, cz, h1, h2, k); the prior form drops cx
    "model": (56, 56, 112, 224, 20),
    "odd": (20, 13, 40, 72, 3),           # cx + cz and cz odd: w1 rows alternate between the float4 and scalar sv_dot
    "wide_k1": (12, 8, 300, 264, 1),      # h1, h2 > 256: the o += 256 thread loop wraps
    "wide_k3": (8, 6, 260, 520, 3),
}
KERNEL_GRAD_TOL = 1e-5
LDS_MAX = 64 * 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def mlp(geom, post):
    """Dyadic (w, b) of the three layers, biases calibrated to ~25 % firing on Bernoulli inputs, and a 0/1 z0.
    geom: a key of GEOMS or a (cx, cz, h1, h2, k) tuple."""
    cx, cz, h1, h2, k = GEOMS.get(geom, geom)
    nin = (cx if post else 0) + cz
    seed = cx + 3 * cz + 5 * h1 + 7 * h2 + 11 * k + 1000 * post
    g = torch.Generator().manual_seed(seed)
    sd = {}
    h = synth._linear_lif_calibrated(sd, "l0", (torch.rand(16, 16, nin, generator=g) < 0.25).float(), h1, seed)
    h = synth._linear_lif_calibrated(sd, "l2", h, h2, seed)
    synth._linear_lif_calibrated(sd, "l4", h, cz * k, seed)
    z0 = (torch.rand(cz, generator=g) < 0.5).float()
    return [(sd[f"l{i}.weight"], sd[f"l{i}.bias"]) for i in (0, 2, 4)], z0


def v_init(B, layers, g):
    """Non-zero dyadic membrane potentials in [0, 1), one per neuron and image."""
    return [torch.randint(0, 4096, (B, w.shape[0]), generator=g).float() / 4096 for w, _ in layers]


def to_dev(layers, dev):
    return [(w.to(dev), b.to(dev)) for w, b in layers]


def spikes(shape, g, rate=0.3):
    return (torch.rand(shape, generator=g) < rate).to(torch.uint8)


def assert_v(vd, vr, what):
    for i, (a, b) in enumerate(zip(vd, vr)):
        assert torch.equal(a.cpu(), b), f"{what}: v of layer {i} differs"


# ---------------------------------------------------------------------------------------------- 1. the eval loops
@pytest.mark.parametrize("post", [True, False], ids=["posterior", "prior"])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_svae_ar_vs_oracle(dev, geom, B, post):
    """ops.svae_ar, T in {1, 5, 16}: two calls in a row with v carried from a non-zero start; z, q_z and every v exact."""
    cx, cz, h1, h2, k = GEOMS[geom]
    layers, z0 = mlp(geom, post)
    ld = to_dev(layers, dev)
    g = torch.Generator().manual_seed(B * 31 + len(geom))
    for T in (1, 5, 16):
        vr = v_init(B, layers, g)
        vd = [v.to(dev) for v in vr]
        for call in range(2):
            idx = torch.randint(0, k, (T, B, cz), generator=g, dtype=torch.int32)
            x = spikes((T, B, cx), g) if post else None
            z, q = ops.svae_ar(None if x is None else x.to(dev), z0.to(dev), ld, vd, idx.to(dev), want_q_z=post)
            torch.cuda.synchronize()
            what = f"{geom} B={B} T={T} call {call}"
            if post:
                zr, qr = ref.svae_posterior(x, z0, layers, vr, idx)
                assert torch.equal(q.cpu().float(), qr), what + ": q_z"
            else:
                zr = ref.svae_prior_sample(z0, layers, vr, idx)
            assert torch.equal(z.cpu(), zr), what + ": z"
            assert_v(vd, vr, what)
        if T == 16:
            rate = float(zr.mean())
            assert 0.02 < rate < 0.98, (what, rate)          # the loop is not degenerate


SCHED = {                                 # name -> sched [T-1] as a function of T
    "first": lambda n: [i == 0 for i in range(n)],
    "last": lambda n: [i == n - 1 for i in range(n)],
    "every": lambda n: [True] * n,
    "none": lambda n: [False] * n,
}


@pytest.mark.parametrize("post", [True, False], ids=["posterior", "prior"])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_svae_ar_prefix_vs_oracle(dev, geom, B, post):
    """ops.svae_ar_prefix, T in {2, 16}, from a non-zero v; the prior under every schedule of SCHED.  noise (scaled so
    that it decides many steps) and z_teacher differ per image, so a wrong image index shows."""
    cx, cz, h1, h2, k = GEOMS[geom]
    layers, z0 = mlp(geom, post)
    ld = to_dev(layers, dev)
    g = torch.Generator().manual_seed(B * 37 + len(geom))
    for T in (2, 16):
        for sname, sfn in (SCHED.items() if not post else [("post", None)]):
            vr = v_init(B, layers, g)
            vd = [v.to(dev) for v in vr]
            what = f"{geom} B={B} T={T} {sname}"
            if post:
                x = spikes((T, B, cx), g)
                idx = torch.randint(0, k, (T, B, cz), generator=g, dtype=torch.int32)
                zm = ops.svae_ar_prefix(x.to(dev), z0.to(dev), ld, vd, idx=idx.to(dev))
                zr = ref.svae_posterior_prefix(x, z0, layers, vr, idx)
            else:
                sched = torch.tensor(sfn(T - 1), dtype=torch.bool)
                noise = torch.randn(int(sched.sum()), B, cz, generator=g) * 300
                zt = spikes((T, B, cz), g, 0.5).float()
                zm = ops.svae_ar_prefix(None, z0.to(dev), ld, vd, sched=sched.to(dev), noise=noise.to(dev),
                                        z_teacher=zt.to(dev))
                zr = ref.svae_prior_prefix(z0, layers, vr, sched, noise, zt)
                if sname == "none":       # all teacher: [z0, z_teacher[:-1]], no layer runs
                    assert torch.equal(zr, torch.cat([z0.view(1, 1, cz).expand(1, B, cz), zt[:-1]], 0))
            torch.cuda.synchronize()
            assert torch.equal(zm.cpu(), zr), what + ": z_t_minus"
            assert_v(vd, vr, what)


def test_all_teacher_prefix_leaves_v_unchanged(dev):
    """sched all zero: noise is [0, B, cz]; the op returns the teacher rows and no neuron moves (both tile sizes)."""
    layers, z0 = mlp("model", False)
    ld = to_dev(layers, dev)
    g = torch.Generator().manual_seed(7)
    for B in (8, 300):
        vr = v_init(B, layers, g)
        vd = [v.to(dev) for v in vr]
        zt = spikes((16, B, 56), g, 0.5).float()
        zm = ops.svae_ar_prefix(None, z0.to(dev), ld, vd, sched=torch.zeros(15, dtype=torch.uint8, device=dev),
                                noise=torch.empty(0, B, 56, device=dev), z_teacher=zt.to(dev))
        torch.cuda.synchronize()
        assert torch.equal(zm.cpu(), torch.cat([z0.view(1, 1, 56).expand(1, B, 56), zt[:-1]], 0)), B
        assert_v(vd, vr, f"B={B}")


@pytest.mark.parametrize("post", [True, False], ids=["posterior", "prior"])
def test_svae_ar_tile_sizes_agree(dev, post):
    """svae_ar at B = 300 (4-image tiles) equals the same images run as slices of at most 256 (1-image tiles)."""
    cx, cz, h1, h2, k = GEOMS["model"]
    layers, z0 = mlp("model", post)
    ld = to_dev(layers, dev)
    g = torch.Generator().manual_seed(300)
    B, T = 300, 16
    v0 = v_init(B, layers, g)
    idx = torch.randint(0, k, (T, B, cz), generator=g, dtype=torch.int32).to(dev)
    x = spikes((T, B, cx), g).to(dev) if post else None
    vd = [v.to(dev) for v in v0]
    z, q = ops.svae_ar(x, z0.to(dev), ld, vd, idx, want_q_z=post)
    parts = []
    for lo, hi in ((0, 256), (256, 300)):
        vs = [v[lo:hi].contiguous().to(dev) for v in v0]
        zs, qs = ops.svae_ar(None if x is None else x[:, lo:hi].contiguous(), z0.to(dev), ld, vs,
                             idx[:, lo:hi].contiguous(), want_q_z=post)
        parts.append((zs, qs, vs))
    torch.cuda.synchronize()
    assert torch.equal(z, torch.cat([p[0] for p in parts], 1))
    if post:
        assert torch.equal(q, torch.cat([p[1] for p in parts], 1))
    for i in range(3):
        assert torch.equal(vd[i], torch.cat([p[2][i] for p in parts], 0)), i


def test_ar_lds_limit(dev):
    """The model's posterior with k = 30: 4200 floats per image, 67 200 bytes at 4 images.  B > 256 raises
    NotImplementedError (eval loop and prefix); B = 256 runs with 1-image tiles and matches the oracle."""
    cx, cz, h1, h2, k, T = 56, 56, 112, 224, 30, 16
    per_image = T * cx + (T + 1) * cz + 2 * h1 + 2 * h2 + cz * k
    assert 4 * 4 * per_image > LDS_MAX >= 4 * per_image
    layers, z0 = mlp((cx, cz, h1, h2, k), True)
    ld = to_dev(layers, dev)
    g = torch.Generator().manual_seed(30)
    for B in (257, 513):
        vd = [torch.zeros(B, w.shape[0], device=dev) for w, _ in layers]
        x = spikes((T, B, cx), g).to(dev)
        idx = torch.randint(0, k, (T, B, cz), generator=g, dtype=torch.int32).to(dev)
        with pytest.raises(NotImplementedError):
            ops.svae_ar(x, z0.to(dev), ld, vd, idx, want_q_z=True)
        with pytest.raises(NotImplementedError):
            ops.svae_ar_prefix(x, z0.to(dev), ld, vd, idx=idx)
    B = 256
    vr = v_init(B, layers, g)
    vd = [v.to(dev) for v in vr]
    x = spikes((T, B, cx), g)
    idx = torch.randint(0, k, (T, B, cz), generator=g, dtype=torch.int32)
    z, q = ops.svae_ar(x.to(dev), z0.to(dev), ld, vd, idx.to(dev), want_q_z=True)
    torch.cuda.synchronize()
    zr, qr = ref.svae_posterior(x, z0, layers, vr, idx)
    assert torch.equal(z.cpu(), zr) and torch.equal(q.cpu().float(), qr)
    assert_v(vd, vr, "B=256 k=30")


# ---------------------------------------------------------------------------------------------- 2. the model at B > 256
def make_model(dev, train=False):
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    model = ns["SNN_VAE"]()
    ns["functional"].set_step_mode(net=model, step_mode='m')
    model = model.cuda(0)
    model.load_state_dict(synth.synth_svae_state())
    return model.train() if train else model.eval()


def sd_layers(model, name):
    return [(model.get_submodule(f"{name}.layers.{i}").weight.detach().cpu(),
             model.get_submodule(f"{name}.layers.{i}").bias.detach().cpu()) for i in (0, 2, 4)]


def node_v(model, names):
    return [model.get_submodule(n).v.cpu() for n in names]


PRIOR_NODES = ("prior.layers.1", "prior.layers.3", "prior.layers.5")
POST_NODES = ("posterior.layers.1", "posterior.layers.3", "posterior.layers.5")


def decoder_input_ref(model, z):
    lin = model.decoder_input[0]
    _, v = ref.svae_linear_lif(z, lin.weight.detach().cpu(), lin.bias.detach().cpu(), torch.zeros(z.shape[1], 784))
    return v


def test_model_sample_300_vs_oracle(dev):
    model = make_model(dev)
    torch.manual_seed(300)
    with torch.inference_mode():
        sx, sz = model.sample(300)
    torch.cuda.synchronize()
    torch.manual_seed(300)
    idx = ref.svae_draw_indices(16, 300, 56, 20)
    vr = [torch.zeros(300, n) for n in (112, 224, 1120)]
    zr = ref.svae_prior_sample(model.prior.initial_input.cpu(), sd_layers(model, "prior"), vr, idx)
    assert sx.shape == (300, 1, 28, 28)
    assert torch.equal(sz.cpu(), zr)
    assert_v(node_v(model, PRIOR_NODES), vr, "prior")
    assert torch.equal(model.decoder_input[1].v.cpu(), decoder_input_ref(model, zr))


def test_model_eval_forward_260_vs_oracle(dev):
    model = make_model(dev)
    B = 260
    images = (synth.stroke_images(B, seed=11) - 0.5).to(dev)
    cap = []
    inner = model.posterior.forward

    def spy(x, want_q_z=True):
        cap.append(x.detach().cpu())
        return inner(x, want_q_z)
    model.posterior.forward = spy
    torch.manual_seed(260)
    with torch.inference_mode():
        z, xr = model(images.unsqueeze(0).repeat(16, 1, 1, 1, 1), images)
    torch.cuda.synchronize()
    latent_x = cap[0].float()
    torch.manual_seed(260)
    idx = ref.svae_draw_indices(16, B, 56, 20)
    vp = [torch.zeros(B, n) for n in (112, 224, 1120)]
    zr, _ = ref.svae_posterior(latent_x, model.posterior.initial_input.cpu(), sd_layers(model, "posterior"), vp, idx)
    vq = [torch.zeros(B, n) for n in (112, 224, 1120)]
    z0 = model.prior.initial_input.cpu().expand(1, B, 56)
    ref.svae_mlp(torch.cat([z0, zr[:-1]], 0), sd_layers(model, "prior"), vq)      # the prior's teacher-forced pass
    assert xr.shape == (B, 1, 28, 28)
    assert torch.equal(z.cpu(), zr)
    assert_v(node_v(model, POST_NODES), vp, "posterior")
    assert_v(node_v(model, PRIOR_NODES), vq, "prior")
    assert torch.equal(model.decoder_input[1].v.cpu(), decoder_input_ref(model, zr))


def test_model_train_latent_260_scheduled_vs_oracle(dev, monkeypatch):
    """_latent_from in train() at B = 260, p = 0.3: the posterior prefix + grad pass and the prior's scheduled prefix
    (random.seed draws the schedule, the randn_like draws are recorded) against the oracle."""
    model = make_model(dev, train=True)
    model.p = 0.3
    B, seed = 260, 26
    g = torch.Generator().manual_seed(seed)
    latent_x = (torch.rand(16, B, 56, generator=g) < 0.3).float()
    drawn = []
    real = torch.randn_like

    def rec(t, *a, **k):
        r = real(t, *a, **k)
        drawn.append(r.detach().cpu().clone())
        return r
    monkeypatch.setattr(torch, "randn_like", rec)
    torch.manual_seed(seed)
    random.seed(seed)
    sampled_z, mmd, q_z, p_z, z_t_minus = model._latent_from(latent_x.to(dev).requires_grad_())
    torch.cuda.synchronize()
    monkeypatch.undo()
    random.seed(seed)
    sched = torch.tensor([t >= 5 and random.random() < 0.3 for t in range(15)])
    assert int(sched.sum()) == len(drawn) > 0
    torch.manual_seed(seed)
    idx = ref.svae_draw_indices(16, B, 56, 20)
    vp = [torch.zeros(B, n) for n in (112, 224, 1120)]
    szr, qr = ref.svae_posterior(latent_x, model.posterior.initial_input.cpu(), sd_layers(model, "posterior"), vp, idx)
    vq = [torch.zeros(B, n) for n in (112, 224, 1120)]
    zmr = ref.svae_prior_prefix(model.prior.initial_input.cpu(), sd_layers(model, "prior"), vq, sched, torch.stack(drawn), szr)
    pr = ref.svae_mlp(zmr, sd_layers(model, "prior"), vq)                         # the prior's grad pass
    assert torch.equal(q_z.detach().cpu(), qr)
    assert torch.equal(sampled_z.detach().cpu(), szr)
    assert torch.equal(z_t_minus.cpu(), zmr)
    assert torch.equal(p_z.detach().cpu(), pr)
    assert_v(node_v(model, POST_NODES), vp, "posterior")
    assert_v(node_v(model, PRIOR_NODES), vq, "prior")


# ---------------------------------------------------------------------------------------------- 3. training GEMM tails
def dyadic(shape, scale, g):
    return torch.randint(-64, 65, shape, generator=g).float() / scale


def lif_offset(cur, v0, rate=0.25):
    """The constant on the 2^-12 grid that, added to every current of cur [T,B,out], makes the fp32 LIF fire at ~rate."""
    lo, hi = -16.0, 16.0
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if float(lif_fp32(cur + mid, v0)[0].mean()) < rate else (lo, mid)
    return round(0.5 * (lo + hi) * 4096) / 4096


def check_linear_train(dev, T, B, n1, n_out, g, n2=0, lif=True, bias=True, x_u8=False, x2_grad=True):
    """LinearLIFTrainFunction against fp64 autograd: forward spikes, h and v (or the currents) exact, dX / dW / db within
    KERNEL_GRAD_TOL.  x [T,B,n1] (u8 or fp32 with grad) and optional x2 [T,B,n2] (fp32, with or without grad).  With the
    LIF, a calibrated offset (in the bias, or without one spread over the weights) makes the layer fire at ~25 %."""
    nin = n1 + n2
    x = (torch.rand(T, B, nin, generator=g) < 0.3).float()
    w = dyadic((n_out, nin), 4096 if nin > 200 else 1024, g)
    b = dyadic((n_out,), 256, g) if bias else None
    v0 = torch.randint(0, 200, (B, n_out), generator=g).float() / 256
    if lif:
        cur = x @ w.t() + (b if bias else 0.0)                       # exact: dyadic products, small sums
        off = lif_offset(cur, v0)
        if bias:
            b = b + off
        else:
            w = w + round(off / (0.3 * nin) * 4096) / 4096
    gout = torch.randn(T, B, n_out, generator=g)
    x1d = x[..., :n1].to(torch.uint8).to(dev) if x_u8 else x[..., :n1].to(dev).requires_grad_()
    x2d = x[..., n1:].to(dev).requires_grad_(x2_grad) if n2 else None
    wd = w.to(dev).requires_grad_()
    bd = b.to(dev).requires_grad_() if bias else None
    vd = v0.to(dev).clone() if lif else None
    out = ops.LinearLIFTrainFunction.apply(x1d, x2d, wd, bd, vd, lif)
    (out * gout.to(dev)).sum().backward()
    torch.cuda.synchronize()
    cur = x.double() @ w.double().t()
    cur = (cur + b.double() if bias else cur).float()                       # exact: dyadic products, small sums
    what = f"T={T} B={B} {n1}+{n2}->{n_out} lif={lif} bias={bias} u8={x_u8}"
    if lif:
        s_ref, h_ref, v_ref = lif_fp32(cur, v0)
        _, h_dev = ops.linear_lif_train_fwd(x1d.detach(), w.to(dev), None if b is None else b.to(dev),
                                            v0.to(dev).clone(), None if x2d is None else x2d.detach())
        assert torch.equal(out.detach().cpu(), s_ref), what
        assert torch.equal(h_dev.cpu(), h_ref), what
        assert torch.equal(vd.cpu(), v_ref), what
        if s_ref.numel() >= 4096:
            assert 0.02 < float(s_ref.mean()) < 0.9, what
    else:
        assert torch.equal(out.detach().cpu(), cur), what
    x64 = x.double().requires_grad_()
    w64 = w.double().requires_grad_()
    b64 = b.double().requires_grad_() if bias else None
    c64 = x64 @ w64.t() + (b64 if bias else 0.0)
    o64 = lif_fp64(c64, v0.double(), s_ref.double()) if lif else c64
    (o64 * gout.double()).sum().backward()
    errs = {"dw": rel_l2(wd.grad, w64.grad)}
    if bias:
        errs["db"] = rel_l2(bd.grad, b64.grad)
    if not x_u8:
        errs["dx1"] = rel_l2(x1d.grad, x64.grad[..., :n1])
    else:
        assert x1d.grad is None
    if n2:
        if x2_grad:
            errs["dx2"] = rel_l2(x2d.grad, x64.grad[..., n1:])
        else:
            assert x2d.grad is None
    assert max(errs.values()) <= KERNEL_GRAD_TOL, (what, errs)


@pytest.mark.parametrize("n_out", [1, 65, 257])
@pytest.mark.parametrize("n_in", [63, 64, 65, 784])
@pytest.mark.parametrize("T,B", [(3, 5), (16, 257)])
def test_linear_lif_train_tails(dev, T, B, n_in, n_out):
    """M = T*B in {15, 4112}: a ragged 16-deep K tile in WGRAD and a ragged 64-row DGRAD tile; nin = 64: the bias column
    is a tile of its own; nout = 1 / 65 / 257: ragged output tiles."""
    check_linear_train(dev, T, B, n_in, n_out, torch.Generator().manual_seed(T * B * 1009 + n_in * 31 + n_out))


@pytest.mark.parametrize("T", [1, 3, 16])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_linear_lif_train_row_counts(dev, T, B):
    """Every M = T*B of B in {1, 5, 257} x T in {1, 3, 16}, LIF and plain currents."""
    g = torch.Generator().manual_seed(T * 7 + B)
    check_linear_train(dev, T, B, 65, 65, g)
    check_linear_train(dev, T, B, 64, 257, g, lif=False)


@pytest.mark.parametrize("T,B", [(16, 5), (3, 257)])
def test_linear_lif_train_concat_u8_and_no_bias(dev, T, B):
    g = torch.Generator().manual_seed(T + B)
    check_linear_train(dev, T, B, 56, 112, g, n2=56, x2_grad=False)     # the posterior's [x | z_t_minus]: grad_x_cols = n1
    check_linear_train(dev, T, B, 65, 63, g, n2=64, x2_grad=True)      # both inputs: grad_x_cols = nin
    check_linear_train(dev, T, B, 65, 65, g, x_u8=True)                # u8 input: dW and db only
    check_linear_train(dev, T, B, 64, 65, g, bias=False)               # no bias column
    check_linear_train(dev, T, B, 63, 65, g, x_u8=True, bias=False, lif=False)
    check_linear_train(dev, T, B, 40, 65, g, n2=24, x_u8=True, x2_grad=True, bias=False)


# ---------------------------------------------------------------------------------------------- 4. the latent loss
def latent_case(dev, T, B, cz, k, tau, with_p, g):
    q = (torch.rand(T, B, cz * k, generator=g) < 0.3).float()
    p = (torch.rand(T, B, cz * k, generator=g) < 0.3).float()
    idx = torch.randint(0, k, (T, B, cz), generator=g, dtype=torch.int32)
    gsz = torch.randn(T, B, cz, generator=g)
    qd = q.to(dev).requires_grad_()
    pd = p.to(dev).requires_grad_() if with_p else None
    return q, p, idx, gsz, qd, pd


@pytest.mark.parametrize("with_p", [True, False], ids=["mmd", "gather_only"])
@pytest.mark.parametrize("tau", [2.0, 3.0])
@pytest.mark.parametrize("T,B,cz,k", [(1, 5, 56, 20), (7, 3, 13, 1), (2, 1200, 56, 3)])
def test_latent_loss_shapes_vs_autograd(dev, T, B, cz, k, tau, with_p):
    """(2, 1200, 56, 3): 67 200 columns, 263 partial sums for the one 256-thread reduction workgroup."""
    g = torch.Generator().manual_seed(T * 100 + B + cz + k)
    q, p, idx, gsz, qd, pd = latent_case(dev, T, B, cz, k, tau, with_p, g)
    sz, loss = ops.LatentLossFunction.apply(qd, pd, idx.to(dev), tau)
    if with_p:
        (loss * 3.0 + (sz * gsz.to(dev)).sum()).backward()
    else:
        (sz * gsz.to(dev)).sum().backward()
    torch.cuda.synchronize()
    q64, p64 = q.double().requires_grad_(), p.double().requires_grad_()
    sz64 = torch.gather(q64.view(T, B, cz, k), 3, idx.long().unsqueeze(-1)).squeeze(-1)
    assert torch.equal(sz.detach().cpu(), sz64.detach().float())
    if not with_p:
        assert float(loss) == 0.0
        (sz64 * gsz.double()).sum().backward()
        assert rel_l2(qd.grad, q64.grad) <= KERNEL_GRAD_TOL
        return
    l64 = torch.mean((ref.psp_filter(q64.view(T, B, cz, k).mean(-1), tau) -
                      ref.psp_filter(p64.view(T, B, cz, k).mean(-1), tau)) ** 2)
    (l64 * 3.0 + (sz64 * gsz.double()).sum()).backward()
    errs = {"loss": abs(float(loss) - float(l64)) / float(l64), "dq": rel_l2(qd.grad, q64.grad),
            "dp": rel_l2(pd.grad, p64.grad)}
    assert max(errs.values()) <= KERNEL_GRAD_TOL, errs


# ---------------------------------------------------------------------------------------------- 5. determinism
def test_backward_is_bitwise_deterministic_at_ragged_shapes(dev):
    g = torch.Generator().manual_seed(5)
    T, B, n1, n2, n_out = 3, 257, 65, 56, 257
    x = (torch.rand(T, B, n1 + n2, generator=g) < 0.3).float().to(dev)
    w, b = dyadic((n_out, n1 + n2), 1024, g).to(dev), (dyadic((n_out,), 256, g) + 1.0).to(dev)
    v0 = (torch.randint(0, 200, (B, n_out), generator=g).float() / 256).to(dev)
    gout = torch.randn(T, B, n_out, generator=g).to(dev)
    grads = []
    for _ in range(2):
        xd, wd, bd = x[..., :n1].clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        out = ops.LinearLIFTrainFunction.apply(xd, x[..., n1:].contiguous(), wd, bd, v0.clone(), True)
        (out * gout).sum().backward()
        grads.append((xd.grad, wd.grad, bd.grad))
    T2, B2, cz, k = 2, 1200, 56, 3
    q, p, idx, gsz, _, _ = latent_case(dev, T2, B2, cz, k, 2.0, True, g)
    for _ in range(2):
        qd, pd = q.to(dev).requires_grad_(), p.to(dev).requires_grad_()
        sz, loss = ops.LatentLossFunction.apply(qd, pd, idx.to(dev), 2.0)
        (loss + (sz * gsz.to(dev)).sum()).backward()
        grads.append((qd.grad, pd.grad, loss.detach()))
    torch.cuda.synchronize()
    for a, c in ((grads[0], grads[1]), (grads[2], grads[3])):
        for i, (u, v) in enumerate(zip(a, c)):
            assert torch.equal(u, v), i
