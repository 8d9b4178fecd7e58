"""fp64 restatement of ONE training iteration of the plain-CNN VQVAE baseline (R/snn_model/vae_model.py:548-672 in train() mode,
R/main.py:130-142) GIVEN the decisions, the teacher-forced layer check that justifies those decisions, the counted round-off
bounds of the quantiser / loss kernels, and the case tables the host and the GPU tests share.  No device code.

ReLU is a discontinuity of the gradient and the arg min a discontinuity of everything, so an fp64 run that makes its own
decisions measures the decisions of the path under test and not its round-off.  ``train64`` is therefore handed the decisions of
the path it judges (which units the four ReLUs pass, which code every row takes) -- tests/_bn_lif_train_oracle.py does the
same with the kernel's spike decisions -- and ``check_decisions`` shows that every decision it was handed is one an exact run
could not tell from its own: each saved activation is recomputed in fp64 from the saved activation below it, must lie within
the counted forward bound of an fp32 dot product, a mask may differ from ``preact64 > 0`` only where |preact64| is within that
bound, and an index must satisfy F20's tau rule.
"""
import numpy as np
import torch
import torch.nn.functional as F

import _ann_vqvae_oracle as orc
import _conv_train_cases as ctc
from spkdiff import synth

EPS = 2.0 ** -24                  # unit round-off of fp32
D = 16                            # embedding_dim of every case (SPK_ANN_VQVAE_D)
PARAMS = ("encoder.convs.0", "encoder.convs.2", "encoder.convs.4", "decoder.convs.0", "decoder.convs.2", "decoder.convs.4")
# (transposed, stride, pad, out_pad, ReLU behind it) of the six layers, in PARAMS order
LAYERS = ((False, 2, 1, 0, True), (False, 2, 1, 0, True), (False, 1, 0, 0, False),
          (True, 2, 1, 1, True), (True, 2, 1, 1, True), (True, 1, 1, 0, False))
MASKS = ("a1", "a2", "d1", "d2")  # the saved post-ReLU activations, in forward order


def _conv(x, w, b, layer):
    tr, s, p, op, _ = layer
    return F.conv_transpose2d(x, w, b, s, p, op) if tr else F.conv2d(x, w, b, s, p)


def train64(sd, images, relu_masks, idx, beta, data_variance):
    """One iteration in fp64 given the decisions.  sd: state dict (any float dtype); images [B,C,H,W]; relu_masks: four bool
    tensors [B,C,h,w] (a1, a2, d1, d2: True where the ReLU passes its input); idx int64 [B*h*w] -> ({"loss_eq", "loss_rec",
    "real_loss_rec"} floats, {parameter name: fp64 gradient} of (loss_eq + loss_rec), thirteen tensors)."""
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    m = [t.cpu().bool() for t in relu_masks]
    x = images.detach().cpu().double()

    def layer(i, h, mask=None):
        y = _conv(h, p[PARAMS[i] + ".weight"], p[PARAMS[i] + ".bias"], LAYERS[i])
        return y if mask is None else torch.where(mask, y, torch.zeros((), dtype=torch.float64))

    z = layer(2, layer(1, layer(0, x, m[0]), m[1]))
    zl = z.permute(0, 2, 3, 1)
    q = p["vq_layer.embeddings.weight"][idx.cpu().reshape(-1)].view_as(zl)
    loss_eq = F.mse_loss(q, zl.detach()) + beta * F.mse_loss(zl, q.detach())
    e = (zl + (q - zl).detach()).permute(0, 3, 1, 2)
    xr = layer(5, layer(4, layer(3, e, m[2]), m[3]))
    real = F.mse_loss(xr, x)
    loss_rec = real / float(data_variance)
    (loss_eq + loss_rec).backward()
    return ({"loss_eq": float(loss_eq.detach()), "loss_rec": float(loss_rec.detach()), "real_loss_rec": float(real.detach())},
            {k: v.grad for k, v in p.items()})


def check_decisions(sd, rec, what=""):
    """The teacher-forced layer check.  rec: {"x", "a1", "a2", "z", "idx", "e", "d1", "d2", "x_recon"} (logical NCHW, fp32; any
    device).  Asserts the bounds and returns {"mask_diff": units whose mask differs from preact64 > 0 (all within the bound),
    "idx_diff": rows whose index differs from the fp64 arg min (all within tau), "worst_act": largest |saved - fp64| / bound,
    "worst_slack": largest index slack / tau}."""
    r = {k: v.detach().cpu() for k, v in rec.items() if isinstance(v, torch.Tensor)}
    chain = (("x", "a1"), ("a1", "a2"), ("a2", "z"), ("e", "d1"), ("d1", "d2"), ("d2", "x_recon"))
    mask_diff, worst = 0, 0.0
    for i, (src, dst) in enumerate(chain):
        w, b = sd[PARAMS[i] + ".weight"].double(), sd[PARAMS[i] + ".bias"].double()
        h = r[src].double()
        pre = _conv(h, w, b, LAYERS[i])
        n = w.shape[2] * w.shape[3] * (w.shape[0] if LAYERS[i][0] else w.shape[1])      # taps x input channels (at most)
        bound = (n + 2) * EPS * _conv(h.abs(), w.abs(), b.abs(), LAYERS[i])
        got = r[dst].double()
        want = pre.clamp_min(0) if LAYERS[i][4] else pre
        ok = torch.isfinite(want)
        ratio = float(((got - want).abs()[ok] / bound[ok].clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{what}: {dst} is {ratio:.3g} x the forward bound from its fp64 value"
        if LAYERS[i][4]:
            differ = (r[dst] > 0) != (pre > 0)
            assert bool((pre.abs()[differ] <= bound[differ]).all()), f"{what}: a ReLU decision of {dst} differs outside the bound"
            mask_diff += int(differ.sum())
    d64 = orc.distances64(r["z"], sd)
    idx_diff, slack = orc.check_indices(d64, r["idx"], what)
    zl = r["z"].permute(0, 2, 3, 1)
    q = sd["vq_layer.embeddings.weight"][r["idx"].reshape(-1)].view_as(zl)
    assert torch.equal(r["e"].permute(0, 2, 3, 1), zl + (q - zl)), f"{what}: e is not the fp32 value z + (q - z)"
    return {"mask_diff": mask_diff, "idx_diff": idx_diff, "worst_act": worst, "worst_slack": slack}


def masks_of(rec):
    return [rec[k].detach().cpu() > 0 for k in MASKS]


def module_path_decisions(model, images):
    """(losses, masks, idx) of one forward of ``model``'s MODULE path (train() mode, hooks on the four nn.ReLU modules -- which
    also keep the HIP path away); the caller runs backward on the losses."""
    got, handles = {}, []
    relus = (model.encoder.convs[1], model.encoder.convs[3], model.decoder.convs[1], model.decoder.convs[3])
    for name, mod in zip(MASKS, relus):
        handles.append(mod.register_forward_hook(lambda _m, _i, out, name=name: got.__setitem__(name, out.detach().cpu() > 0)))
    handles.append(model.encoder.register_forward_hook(lambda _m, _i, out: got.__setitem__("z", out.detach())))
    try:
        losses = model(images)
    finally:
        for h in handles:
            h.remove()
    flat = got["z"].permute(0, 2, 3, 1).reshape(-1, model.embedding_dim)
    idx = model.vq_layer.get_code_indices(flat).cpu()
    return losses, [got[k] for k in MASKS], idx


# ---- counted bounds of the quantiser and loss kernels against fp64 given the indices (tests/test_gpu_ann_vqvae_train.py) ----
# Every bound is (number of fp32 roundings on the path, rounded up to 8) x 2^-24 x the magnitude the roundings act on.
def vq_reference(z, cb, idx, beta, g_e, g_loss):
    """fp64 values and bounds of spk_ann_vqvae_train_vq_fwd / _bwd for z [N,D], cb [K,D] fp32, idx [N], g_e [N,D], g_loss float."""
    z64, cb64, g64 = z.double().cpu(), cb.double().cpu(), g_e.double().cpu()
    idx = idx.cpu()
    q = cb64[idx]
    n = z64.numel()
    m = float(((q - z64) ** 2).mean())
    loss = m + beta * m                                   # roundings: q - z, its square, the mean, beta * m, the sum
    t = g_loss * beta * 2.0 * (z64 - q) / n               # roundings: gl * beta, 2 / n, their product, z - q, the product, the sum
    gz = g64 + t
    gcb = torch.zeros_like(cb64)
    gcb.index_add_(0, idx, q - z64)
    mag = torch.zeros_like(cb64)
    mag.index_add_(0, idx, (q - z64).abs())
    scale = abs(g_loss) * 2.0 / n                         # roundings: every q - z, the sum's cast, 2 / n, two products
    return {"loss": loss, "loss_bound": 8 * EPS * abs(loss), "gz": gz, "gz_bound": 8 * EPS * (g64.abs() + t.abs()),
            "gcb": g_loss * 2.0 / n * gcb, "gcb_bound": 8 * EPS * scale * mag}


def loss_reference(xr_nchw, x, dv, g_recon, g_real):
    """fp64 values and bounds of spk_ann_vqvae_train_loss_fwd / _bwd (xr_nchw: the reconstruction, logical NCHW)."""
    d = xr_nchw.double().cpu() - x.double().cpu()
    mse = float((d ** 2).mean())                          # roundings: the difference, its square, the mean, the division
    g = (g_recon / dv + g_real) * 2.0 * d / d.numel()     # roundings: g / dv, the sum, 2 / n, the product, the difference, the product
    return {"real": mse, "recon": mse / dv, "bound": 8 * EPS * mse, "recon_bound": 8 * EPS * mse / dv, "g": g,
            "g_bound": 8 * EPS * g.abs()}


# ---- the epilogue cases ---------------------------------------------------------------------------------------------------
def vqvae_layers(C, H):
    """The launches of one training iteration that carry an epilogue, as (name, layer tuple of _conv_train_cases, op, epilogue):
    layer = (Cin, Cout, k, stride, pad, transposed, out_pad, input size)."""
    return (
        ("enc0.fwd", (C, 32, 3, 2, 1, False, 0, H), "fwd", "relu"),
        ("enc2.fwd", (32, 64, 3, 2, 1, False, 0, H // 2), "fwd", "relu"),
        ("enc2.dgrad", (32, 64, 3, 2, 1, False, 0, H // 2), "dgrad", "masked"),
        ("enc4.dgrad", (64, D, 1, 1, 0, False, 0, H // 4), "dgrad", "masked"),
        ("dec0.fwd", (D, 64, 3, 2, 1, True, 1, H // 4), "fwd", "relu"),
        ("dec2.fwd", (64, 32, 3, 2, 1, True, 1, H // 2), "fwd", "relu"),
        ("dec2.dgrad", (64, 32, 3, 2, 1, True, 1, H // 2), "dgrad", "masked"),
        ("dec4.dgrad", (32, C, 3, 1, 1, True, 0, H), "dgrad", "masked"),
    )


def big_threshold(layer, op):
    """Smallest N at which the gather launch of (layer, op) has CT_BIG_ITEMS items or more (two column tiles per wave)."""
    n = 1
    while ctc.gather_launch(*ctc.gather_args(layer, n, op))["items"] < ctc.CT_BIG_ITEMS:
        n += 1
    return n


# 64-output-channel launches on either side of CT_BIG_ITEMS: a ReLU launch of each gather form and a masked one
BIG_LAYERS = tuple((name, layer, op, epi) for name, layer, op, epi in vqvae_layers(1, 28)
                   if name in ("enc2.fwd", "dec0.fwd", "dec2.dgrad"))


def epilogue_cases():
    """[(id, layer, N, op, epilogue)]: every layer at H = 28 (grey) and 32 (RGB), N = 1 and 3, and the CT_BIG_ITEMS pairs."""
    out = []
    for C, H in ((1, 28), (3, 32)):
        for name, layer, op, epi in vqvae_layers(C, H):
            for N in (1, 3):
                out.append((f"{name}-H{H}-N{N}", layer, N, op, epi))
    for name, layer, op, epi in BIG_LAYERS:
        n = big_threshold(layer, op)
        out += [(f"{name}-below_big-N{n - 1}", layer, n - 1, op, epi), (f"{name}-at_big-N{n}", layer, n, op, epi)]
    return out


# ---- the model cases: (id, shape name of _ann_vqvae_oracle.SHAPES, B); "f20" = the fixture's images and state -------------------
MODEL_CASES = (("f20", "mnist_k128", 8), ("mnist_k128-B1", "mnist_k128", 1), ("mnist_k128-B3", "mnist_k128", 3),
               ("mnist_k128-B33", "mnist_k128", 33), ("cifar_k256-B3", "cifar_k256", 3), ("mnist_k100-B3", "mnist_k100", 3))


def model_inputs(case):
    """(state dict, images fp32 [B,C,H,W], data_variance float, K, in_dim) of a model case."""
    cid, shape, B = case
    _, cfg, K = next(s for s in orc.SHAPES if s[0] == shape)
    sd = orc.state(shape)
    if cid == "f20":
        f = orc.fixture()
        return sd, torch.from_numpy(f["images"]), float(f["data_variance"]), K, cfg.in_dim
    images = synth.stroke_images(B, img=cfg.img, channels=cfg.in_dim) - 0.5
    return sd, images, 0.0625, K, cfg.in_dim


def grad_entries(g):
    g = g.detach().cpu().numpy().reshape(-1)
    return g[orc.sub_index(g.size)] if g.size > orc.SUB else g
