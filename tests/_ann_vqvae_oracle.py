"""fp64 restatement of the plain-CNN VQVAE baseline (R/snn_model/vae_model.py:548-672) in plain torch, the tolerance rules of
its tests, and the case table the host and the GPU tests share.  No device code.

Tolerances come from fixture F20 (tests/golden/f20_ann_vqvae.npz, tools/gen_golden_ann_vqvae.py), which records how far the
fp32 reference itself is from its own fp64 run:

* indices -- for every position, the fp64 distance of the chosen code may exceed the fp64 minimum by at most
  tau * max_k |d64|, tau = 8 x the recorded relative distance error (another summation order over the same <= 576-term sums
  and the same three-term distance moves that error by a small multiple).  Where the fp64 top-2 gap exceeds the bound this
  forces the exact index; at most 1 % of a case's positions may have a smaller gap (``fragile_share``).
* pixels -- decode of GIVEN indices against the fp64 reconstruction: 16 x the recorded pixel error, at most 1e-4.
* training -- losses and gradients against fp64: 8 x the recorded error of that tensor.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from spkdiff import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F20 = os.path.join(ROOT, "tests", "golden", "f20_ann_vqvae.npz")
SUB = 2048                        # entries a large gradient keeps in the fixture (as fixtures F17 / F18)
MAX_FRAGILE_SHARE = 0.01
PIXEL_BOUND_CAP = 1e-4            # the project's standing pixel bound


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(F20) as f:
        return {k: f[k] for k in f.files}


def tau():
    """Relative slack of the index rule."""
    return 8.0 * float(fixture()["err_rel_dist"])


def pixel_bound():
    return min(16.0 * float(fixture()["err_pixel"]), PIXEL_BOUND_CAP)


def sub_index(n):
    """The flat indices a large gradient keeps in the fixture (tools/gen_golden_ann_vqvae.py repeats it)."""
    step = n // SUB
    return np.arange(SUB, dtype=np.int64) * step + step // 2


def _d(sd):
    return {k: v.double() for k, v in sd.items()}


def encode64(sd, images):
    """images [B,C,H,W] -> z fp64 [B,D,h,w] with the fp64 copies of the weights."""
    sd, p = _d(sd), "encoder.convs."
    x = F.relu(F.conv2d(images.double(), sd[p + "0.weight"], sd[p + "0.bias"], 2, 1))
    x = F.relu(F.conv2d(x, sd[p + "2.weight"], sd[p + "2.bias"], 2, 1))
    return F.conv2d(x, sd[p + "4.weight"], sd[p + "4.bias"])


def distances64(z, sd):
    """z [B,D,h,w] (any float dtype) -> fp64 distances [B*h*w, K], the reference's expression."""
    cb = sd["vq_layer.embeddings.weight"].double()
    flat = z.double().permute(0, 2, 3, 1).reshape(-1, cb.shape[1])
    return torch.sum(flat ** 2, dim=1, keepdim=True) + torch.sum(cb ** 2, dim=1) - 2.0 * torch.matmul(flat, cb.t())


def decode64(sd, e):
    """e [B,D,h,w] (NaN rows allowed) -> x_recon fp64 [B,C,H,W]."""
    sd, p = _d(sd), "decoder.convs."
    y = F.relu(F.conv_transpose2d(e.double(), sd[p + "0.weight"], sd[p + "0.bias"], 2, 1, 1))
    y = F.relu(F.conv_transpose2d(y, sd[p + "2.weight"], sd[p + "2.bias"], 2, 1, 1))
    return F.conv_transpose2d(y, sd[p + "4.weight"], sd[p + "4.bias"], 1, 1)


def embed64(sd, tokens):
    """tokens int64 [B,h,w] -> e fp64 [B,D,h,w]; a token outside [0, K) embeds as NaN (spk_embedding_fwd's rule)."""
    cb = sd["vq_layer.embeddings.weight"].double()
    ok = (tokens >= 0) & (tokens < cb.shape[0])
    e = cb[tokens.clamp(0, cb.shape[0] - 1)]
    e[~ok] = float("nan")
    return e.permute(0, 3, 1, 2).contiguous()


def forward64(sd, images):
    """The eval forward in fp64: {"z", "d" [N,K], "idx" [N], "e", "x_recon"}."""
    z = encode64(sd, images)
    d = distances64(z, sd)
    idx = torch.argmin(d, dim=1)
    B, _, h, w = z.shape
    e = embed64(sd, idx.view(B, h, w))
    return {"z": z, "d": d, "idx": idx, "e": e, "x_recon": decode64(sd, e)}


def uint8_rule(pred):
    """R/main.py:400 on an fp32 tensor: np.array(np.clip(pred + 0.5, 0, 1) * 255, dtype=np.uint8) (truncating cast)."""
    return ((pred + 0.5).clamp(0, 1) * 255).to(torch.uint8)


def index_slack(d64, idx):
    """Per position: (d64[chosen] - min d64) / max_k |d64|, fp64 [N]; the index rule is ``index_slack <= tau()``."""
    chosen = d64.gather(1, idx.reshape(-1, 1).to(torch.int64))[:, 0]
    return (chosen - d64.min(dim=1).values) / d64.abs().max(dim=1).values


def fragile_share(d64, t=None):
    """Share of positions whose fp64 top-2 gap is below the index rule's bound (there the rule does not force the index)."""
    t = tau() if t is None else t
    s = torch.topk(d64, 2, dim=1, largest=False).values
    return float(((s[:, 1] - s[:, 0]) < t * d64.abs().max(dim=1).values).double().mean())


def check_indices(d64, idx, what=""):
    """The index rule; returns (positions that differ from the fp64 arg min, largest slack / tau)."""
    slack = index_slack(d64, idx.cpu())
    worst = float(slack.max()) / tau()
    n_diff = int((idx.cpu().reshape(-1) != torch.argmin(d64, dim=1)).sum())
    assert worst <= 1.0, f"{what}: a chosen code is {worst:.3g} x the allowed slack above the fp64 minimum"
    return n_diff, worst


# ---- the cases the GPU tests run; the host test checks the fragile-share condition for each ------------------------
SHAPES = (("mnist_k128", synth.MNIST, 128), ("cifar_k256", synth.CIFAR, 256), ("mnist_k100", synth.MNIST, 100))


def batch_sizes(group, grid_cap):
    """B = 1, 3, 33 and the sizes the kernel's grouping makes special: one less and one more than the images a workgroup
    takes at a time, and one more than a full grid of workgroups."""
    return sorted({b for b in (1, 3, 33, group - 1, group + 1, group * grid_cap + 1) if b >= 1})


def cases(group, grid_cap):
    """[(shape name, cfg, K, B)]: every batch size at the MNIST shape, the ends and the wrap-around at the others."""
    sizes = batch_sizes(group, grid_cap)
    out = [(SHAPES[0][0], SHAPES[0][1], SHAPES[0][2], b) for b in sizes]
    for name, cfg, K in SHAPES[1:]:
        out += [(name, cfg, K, b) for b in (3, 33, sizes[-1])]
    return out


@functools.lru_cache(maxsize=None)
def state(name):
    _, cfg, K = next(s for s in SHAPES if s[0] == name)
    return synth.synth_ann_vqvae_state(cfg, K=K)


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """(images fp32 [n,C,H,W], forward64 of them) of a shape: computed once for the largest batch, every case takes a prefix
    (the fp64 convolutions treat every image alone).  Not to be modified."""
    _, cfg, _ = next(s for s in SHAPES if s[0] == name)
    images = synth.stroke_images(n, img=cfg.img, channels=cfg.in_dim) - 0.5
    return images, forward64(state(name), images)
