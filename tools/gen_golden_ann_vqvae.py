"""Fixture F20 (tests/golden/f20_ann_vqvae.npz): the plain-CNN VQVAE baseline (R/snn_model/vae_model.py:548-672, main.py
--model vq-vae) computed by the REAL reference on the CPU with ``synth.synth_ann_vqvae_state(synth.MNIST)`` weights on
``synth.stroke_images(8) - 0.5``, in fp32 and -- the same modules after ``.double()`` -- in fp64.

    python tools/gen_golden_ann_vqvae.py [--out tests/golden/f20_ann_vqvae.npz]

Stored:
  * ``state_keys`` (the reference model's state_dict keys, in order), ``state_checksum``, ``images``, ``data_variance``;
  * eval forward: ``indices``, ``z``, ``e``, ``x_recon`` (fp32) and ``indices64``, ``z64``, ``e64``, ``x_recon64``;
  * one training iteration, ``(loss_eq + loss_rec).backward()`` (R/main.py:139-142) on a fresh model: ``loss_eq``,
    ``loss_rec``, ``real_loss_rec`` and every parameter's gradient (``grad/<name>``; more than SUB entries: ``/norm`` +
    ``/sub`` at a fixed stride + ``/shape``, as fixtures F17 / F18 store them), and the same under ``loss64/`` / ``grad64/``;
  * the errors of the fp32 reference against its own fp64 run, from which the tests derive their bounds:
    ``err_rel_dist`` = max over rows of max_k |d32 - d64| / max_k |d64| (d: the code distances, each from its own z),
    ``err_pixel`` = max |x_recon32(decoder on e64's fp32 values) - x_recon64| -- no index decision enters --,
    ``err_loss/<name>``, ``err_grad/<name>`` (max over the stored entries; the norm's under ``err_gradnorm/<name>``);
  * ``fragile_share``: the share of positions whose fp64 top-2 distance gap is below 8 * err_rel_dist * max_k |d64| (asserted
    <= 1 % here).
Reproducing it needs the reference tree; the tests only read the .npz."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)          # (not the package directory: its snn_model would shadow the reference's)

from oracle.gen_golden import _import_reference, _load  # noqa: E402

synth = _load(os.path.join(ROOT, "spiking-diffusion_amd", "spkdiff", "synth.py"), "spk_synth")

B = 8
K = 128
SUB = 2048


def sub_index(n):
    """The flat indices a large gradient keeps: SUB entries at a fixed stride (tests/_ann_vqvae_oracle.py repeats it)."""
    step = n // SUB
    return np.arange(SUB, dtype=np.int64) * step + step // 2


def put_grad(f, key, g):
    g = g.detach().numpy()
    if g.size <= SUB:
        f[key] = g
    else:
        f[key + "/norm"] = np.array(float(np.linalg.norm(g.astype(np.float64))))
        f[key + "/sub"] = g.reshape(-1)[sub_index(g.size)]
        f[key + "/shape"] = np.array(g.shape)


def distances(vq, z):
    """The reference's distance expression (CNN_VectorQuantizer.get_code_indices, :595-599) on z [B,D,h,w]."""
    flat_x = z.permute(0, 2, 3, 1).contiguous().reshape(-1, vq.embedding_dim)
    return (torch.sum(flat_x ** 2, dim=1, keepdim=True) + torch.sum(vq.embeddings.weight ** 2, dim=1)
            - 2. * torch.matmul(flat_x, vq.embeddings.weight.t()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "f20_ann_vqvae.npz"))
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    vm, _ = _import_reference()
    sd = synth.synth_ann_vqvae_state(synth.MNIST, K=K)
    images = synth.stroke_images(B) - 0.5
    var = torch.tensor(float(images.var()))

    def model_for(double):
        m = vm.VQVAE(1, 16, K, var.double() if double else var)
        m.load_state_dict(sd)
        return m.double() if double else m

    f = {"state_keys": np.array(list(model_for(False).state_dict())), "state_checksum": np.array(synth.state_checksum(sd)),
         "images": images.numpy(), "data_variance": var.numpy()}

    # ---- eval forward, fp32 and fp64
    m32, m64 = model_for(False).eval(), model_for(True).eval()
    with torch.no_grad():
        z32, z64 = m32.encoder(images), m64.encoder(images.double())
        e32, x32, i32 = m32(images)
        e64, x64, i64 = m64(images.double())
        d32, d64 = distances(m32.vq_layer, z32), distances(m64.vq_layer, z64)
        x32_at64 = m32.decoder(e64.float())            # (e64 holds codebook rows: fp32 values)
    assert torch.equal(e64.float().double(), e64)
    f["indices"], f["z"], f["e"], f["x_recon"] = i32.numpy(), z32.numpy(), e32.numpy(), x32.numpy()
    f["indices64"], f["z64"], f["e64"], f["x_recon64"] = i64.numpy(), z64.numpy(), e64.numpy(), x64.numpy()
    dmax = d64.abs().max(dim=1).values
    err_rel = float(((d32.double() - d64).abs().max(dim=1).values / dmax).max())
    err_pix = float((x32_at64.double() - x64).abs().max())
    f["err_rel_dist"], f["err_pixel"] = np.array(err_rel), np.array(err_pix)
    top2 = torch.topk(d64, 2, dim=1, largest=False).values
    fragile = float(((top2[:, 1] - top2[:, 0]) < 8 * err_rel * dmax).double().mean())
    f["fragile_share"] = np.array(fragile)
    assert fragile <= 0.01, fragile
    print(f"eval: {int(torch.unique(i64).numel())} codes used, indices32 != indices64 at {int((i32 != i64).sum())} of {i64.numel()}, "
          f"err_rel_dist {err_rel:.3g} (tau {8 * err_rel:.3g}), err_pixel {err_pix:.3g}, fragile share {fragile:.4f}, "
          f"x_recon in [{float(x64.min()):.3f}, {float(x64.max()):.3f}]")

    # ---- one training iteration on fresh models
    got = {}
    for double in (False, True):
        model = model_for(double).train()
        x = images.double() if double else images
        loss_eq, loss_rec, real = model(x)
        (loss_eq + loss_rec).backward()
        got[double] = ({"loss_eq": loss_eq, "loss_rec": loss_rec, "real_loss_rec": real},
                       {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in model.named_parameters()})
    for name in got[False][0]:
        v32, v64 = float(got[False][0][name].detach()), float(got[True][0][name].detach())
        f[name], f["loss64/" + name], f["err_loss/" + name] = np.array(v32), np.array(v64), np.array(abs(v32 - v64))
    for n in got[False][1]:
        g32, g64 = got[False][1][n], got[True][1][n]
        put_grad(f, "grad/" + n, g32)
        put_grad(f, "grad64/" + n, g64)
        keep = sub_index(g32.numel()) if g32.numel() > SUB else np.arange(g32.numel())
        f["err_grad/" + n] = np.array(float((g32.double() - g64).reshape(-1)[keep].abs().max()))
        f["err_gradnorm/" + n] = np.array(abs(float(g32.double().norm()) - float(g64.norm())))
        print(f"  grad {n}: |g64| {float(g64.norm()):.4g}, err {float(f['err_grad/' + n]):.3g}, norm err {float(f['err_gradnorm/' + n]):.3g}")
    print("train: " + ", ".join(f"{k} {float(f[k]):.8g} (err {float(f['err_loss/' + k]):.2g})" for k in got[False][0]))
    np.savez_compressed(args.out, **f)
    print(f"wrote {args.out} ({os.path.getsize(args.out) / 1e3:.0f} kB), state {f['state_checksum']}")


if __name__ == "__main__":
    main()
