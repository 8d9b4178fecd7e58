"""GPU tests of the plain-CNN VQVAE baseline (run with ``-m gpu`` on an MI355X): the three launches of
csrc/ann_vqvae.hip against the fp64 oracle (tests/_ann_vqvae_oracle.py) on the same weights and against fixture F20, at the
batch sizes the kernel's grouping makes special, and the model, its entry points and its callers on top of them.  The bounds are
F20's: what the fp32 reference itself loses against its own fp64 run, times the factors _ann_vqvae_oracle states."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ann_vqvae_oracle as orc             # noqa: E402
from parity_report import record as parity  # noqa: E402
from spkdiff import synth                  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def _cases():
    from spkdiff import ops as o
    return orc.cases(o.ANN_VQVAE_GROUP, o.ANN_VQVAE_GRID_CAP)


def _n_ref():
    from spkdiff import ops as o
    return orc.batch_sizes(o.ANN_VQVAE_GROUP, o.ANN_VQVAE_GRID_CAP)[-1]


_MODELS = {}


def build(name, dev):
    from snn_model.vae_model import VQVAE
    if name not in _MODELS:
        _, cfg, K = next(s for s in orc.SHAPES if s[0] == name)
        m = VQVAE(cfg.in_dim, cfg.latent_dim, K, torch.tensor(1.0))
        m.load_state_dict(orc.state(name))
        _MODELS[name] = m.to(dev).eval()
    return _MODELS[name]


def case(name, B):
    """(images fp32 [B,...], the fp64 reference's tensors of those images) -- views of the shared reference."""
    images, r = orc.reference(name, _n_ref())
    h = images.shape[-1] // 4
    return images[:B], {"z": r["z"][:B], "d": r["d"][:B * h * h], "idx": r["idx"][:B * h * h], "x_recon": r["x_recon"][:B]}


# ----------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("name,B", [(n, b) for n, _, _, b in _cases()])
def test_forward_meets_the_fp64_oracle(dev, name, B):
    model = build(name, dev)
    _, cfg, K = next(s for s in orc.SHAPES if s[0] == name)
    images, r = case(name, B)
    assert orc.fragile_share(r["d"]) <= orc.MAX_FRAGILE_SHARE
    with torch.inference_mode():
        e, x_recon, enco = model(images.to(dev))
        tok = model.encode_images(images.to(dev))
        pred, u8 = model.decode_tokens(r["idx"].view(B, cfg.latent, cfg.latent).to(dev))     # the ORACLE's indices: no index decision
        pred_own, _ = model.decode_tokens(tok)
    h = cfg.latent
    assert e.shape == (B, 16, h, h) and e.dtype == torch.float32
    assert x_recon.shape == (B, cfg.in_dim, cfg.img, cfg.img) and x_recon.dtype == torch.float32
    assert enco.shape == (B * h * h,) and enco.dtype == torch.int64
    assert tok.shape == (B, h, h) and torch.equal(tok.reshape(-1), enco)
    cb = orc.state(name)["vq_layer.embeddings.weight"]
    assert torch.equal(e.cpu(), cb[enco.cpu()].view(B, h, h, 16).permute(0, 3, 1, 2))
    assert torch.equal(pred_own, x_recon)                              # decode_tokens(enco) is the forward's decoder, bit for bit
    n_diff, worst = orc.check_indices(r["d"], enco, f"{name} B={B}")
    err = float((pred.cpu().double() - r["x_recon"]).abs().max())
    print(f"{name} B={B}: {n_diff}/{enco.numel()} indices differ from the fp64 arg min, worst slack {worst:.3g} of tau "
          f"{orc.tau():.3g}; pixel err {err:.3g} (bound {orc.pixel_bound():.3g}); {int(enco.unique().numel())} codes used")
    parity(f"ann_vqvae_{name}_B{B}", index_diffs=n_diff, worst_slack_over_tau=worst, pixel_err=err)
    assert err <= orc.pixel_bound()
    assert torch.equal(u8, orc.uint8_rule(pred)) and u8.dtype == torch.uint8
    if B >= 33:                                                        # (the synthetic decoder spans past both ends: the cast clips)
        assert float(r["x_recon"].min()) < -0.5 and float(r["x_recon"].max()) > 0.5 and int(u8.min()) == 0 and int(u8.max()) == 255


def test_f20(dev, ops):
    """The fixture of the real reference: B = 8, MNIST shape."""
    f = orc.fixture()
    model = build("mnist_k128", dev)
    assert str(f["state_checksum"]) == synth.state_checksum(orc.state("mnist_k128"))
    images = torch.from_numpy(f["images"])
    d64 = orc.distances64(torch.from_numpy(f["z64"]), orc.state("mnist_k128"))
    with torch.inference_mode():
        e, x_recon, enco = model(images.to(dev))
        pred, _ = model.decode_tokens(torch.from_numpy(f["indices64"]).view(8, 7, 7).to(dev))
        _, z, _ = ops.ann_vqvae_encode(images.to(dev), model._enc_params(), model.vq_layer.embeddings.weight, want_z=True)
    n_diff, worst = orc.check_indices(d64, enco, "F20")
    n32 = int((enco.cpu() != torch.from_numpy(f["indices"])).sum())
    err = float((pred.cpu().double() - torch.from_numpy(f["x_recon64"])).abs().max())
    zerr = float((z.cpu().double() - torch.from_numpy(f["z64"])).abs().max())
    print(f"F20: {n32} indices differ from the fp32 reference's, {n_diff} from the fp64 one's, worst slack {worst:.3g} tau; pixel "
          f"err {err:.3g} (bound {orc.pixel_bound():.3g}); z err {zerr:.3g}")
    assert err <= orc.pixel_bound()


# ----------------------------------------------------------------------------------------------- 2. properties
@pytest.mark.parametrize("name", [s[0] for s in orc.SHAPES[:2]])
def test_rows_do_not_depend_on_the_batch(dev, name):
    model = build(name, dev)
    images, _ = case(name, 33)
    with torch.inference_mode():
        e33, x33, i33 = model(images.to(dev))
        e3, x3, i3 = model(images[:3].contiguous().to(dev))
        t33 = model.encode_images(images.to(dev))
        p33, u33 = model.decode_tokens(t33)
        p3, u3 = model.decode_tokens(t33[:3].contiguous())
    n = i3.numel()
    assert torch.equal(i33[:n], i3) and torch.equal(e33[:3], e3) and torch.equal(x33[:3], x3)
    assert torch.equal(p33[:3], p3) and torch.equal(u33[:3], u3)


@pytest.mark.parametrize("name", [s[0] for s in orc.SHAPES])
def test_out_of_range_tokens_give_nan_where_they_reach(dev, name):
    model = build(name, dev)
    _, cfg, K = next(s for s in orc.SHAPES if s[0] == name)
    _, r = case(name, 3)
    h = cfg.latent
    tok = r["idx"].view(3, h, h).clone()
    good, _ = model.decode_tokens(tok.to(dev))
    tok[0, 0, 0], tok[1, h - 1, 2], tok[2, 3, h - 1], tok[2, 4, 4] = K, -1, K, K + 1000
    with torch.inference_mode():
        pred, u8 = model.decode_tokens(tok.to(dev))
    want = orc.decode64(orc.state(name), orc.embed64(orc.state(name), tok))
    nan = torch.isnan(want)
    assert bool(nan.any()) and not bool(nan.all())
    assert torch.equal(torch.isnan(pred.cpu()), nan)
    assert torch.equal(pred.cpu()[~nan], good.cpu()[~nan])               # the rest: unchanged, bit for bit
    assert float((pred.cpu().double() - want)[~nan].abs().max()) <= orc.pixel_bound()


def test_a_nan_pixel_reaches_only_its_codes(dev):
    name = "mnist_k128"
    model = build(name, dev)
    images, r = case(name, 3)
    images = images.clone()
    images[1, 0, 13, 9] = float("nan")
    want = orc.forward64(orc.state(name), images)
    with torch.inference_mode():
        _, x_recon, enco = model(images.to(dev))
    hit = torch.isnan(want["d"]).any(dim=1)
    assert 1 <= int(hit.sum()) <= 4 and bool(hit[49:98].any()) and not bool(hit[:49].any()) and not bool(hit[98:].any())
    assert torch.equal(enco.cpu()[hit], want["idx"][hit])                # torch.argmin on the NaN rows
    clean = model(case(name, 3)[0].to(dev))[2]
    assert torch.equal(enco.cpu()[~hit], clean.cpu()[~hit])
    assert not bool(torch.isnan(x_recon).any())                          # (every index is a code: the decoder saw no NaN)


def test_graph_capture_replays_on_new_input(dev, ops):
    name = "mnist_k128"
    model = build(name, dev)
    images, _ = case(name, 33)
    a, b = images[:16].contiguous().to(dev), images[16:32].contiguous().to(dev)
    buf = a.clone()
    enc, dec, cb = model._enc_params(), model._dec_params(), model.vq_layer.embeddings.weight
    ws = ops.ann_vqvae_decode_ws(16, 28, 28, dev)
    with torch.inference_mode():
        idx_w, _, _ = ops.ann_vqvae_encode(buf, enc, cb)                # warm-up ahead of the capture
        ops.ann_vqvae_decode(idx_w.view(16, 7, 7), dec, cb, want_u8=True, ws=ws)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            idx_g, _, _ = ops.ann_vqvae_encode(buf, enc, cb)
            pred_g, u8_g = ops.ann_vqvae_decode(idx_g.view(16, 7, 7), dec, cb, want_u8=True, ws=ws)
        buf.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        tok = model.encode_images(b)
        pred, u8 = model.decode_tokens(tok)
    assert torch.equal(idx_g.view(16, 7, 7), tok) and torch.equal(pred_g, pred) and torch.equal(u8_g, u8)
    assert not torch.equal(tok, model.encode_images(a))


def test_a_hook_sends_the_call_down_the_module_path(dev, monkeypatch):
    name = "mnist_k128"
    model = build(name, dev)
    images, r = case(name, 3)
    x = images.to(dev)
    from spkdiff import ops as o
    calls = []
    real = o.ann_vqvae_encode
    monkeypatch.setattr(o, "ann_vqvae_encode", lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.inference_mode():
        e, x_recon, enco = model(x)
        assert calls == [1]
        seen = []
        handle = model.encoder.convs[2].register_forward_hook(lambda m, i, out: seen.append(tuple(out.shape)))
        try:
            e_m, x_m, enco_m = model(x)
            tok_m = model.encode_images(x)
            pred_m, u8_m = model.decode_tokens(tok_m)
        finally:
            handle.remove()
    assert calls == [1] and seen == [(3, 64, 7, 7)] * 2                 # the library was not called; the hook saw its layer
    assert enco_m.dtype == torch.int64 and x_m.shape == x_recon.shape and e_m.shape == e.shape
    orc.check_indices(r["d"], enco_m, "module path")
    assert torch.equal(tok_m.reshape(-1), enco_m) and u8_m.dtype == torch.uint8
    same = (enco_m == enco).view(3, 49).all(dim=1).cpu()
    assert bool(same.any())
    assert float((x_m - x_recon)[same.to(dev)].abs().max()) <= 2 * orc.pixel_bound()      # each within the bound of the fp64 image


# ----------------------------------------------------------------------------------------------- 3. the callers, each once
def test_reconstruction_eval_takes_the_model(dev):
    from metric import pytorch_ssim as ps
    from spkdiff import evaluate
    model = build("mnist_k128", dev)
    images = synth.stroke_images(40, seed=31)
    batches = [(images[:32], torch.zeros(32, dtype=torch.int64)), images[32:]]
    res = evaluate.reconstruction_eval(model, batches)
    mse, loss = [], []
    for b in (images[:32], images[32:]):
        x = (b - 0.5).to(dev)
        with torch.inference_mode():
            xr = model(x)[1]
        mse.append(torch.nn.functional.mse_loss(xr.double(), x.double()).item())
        loss.append(1 - ps.ssim(xr.double().cpu(), x.double().cpu()).item())
    lit = evaluate.aggregate(loss, mse)
    print(f"reconstruction_eval {res}; from x_recon {lit}")
    assert res["n_batches"] == 2
    # reconstruction_eval rounds each batch's two values (<= 1) to fp32 as .item() would: 2^-24 each; 1e-6 is 16 of those
    assert abs(res["loss_mse"] - lit["loss_mse"]) <= 1e-6 and abs(res["loss_ssim"] - lit["loss_ssim"]) <= 1e-6


def test_complete_images_with_everything_kept(dev):
    from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel, functional
    from spkdiff import complete
    model = build("mnist_k128", dev)
    den = DummyModel(1, 128).to(dev)
    functional.set_step_mode(net=den, step_mode='m')
    den.load_state_dict(synth.synth_denoiser_state(synth.MNIST))
    ab = AbsorbingDiffusion(den.eval(), mask_id=128)
    images = (synth.stroke_images(3, seed=5) - 0.5).to(dev)
    keep = torch.ones(3, 28, 28, dtype=torch.bool, device=dev)
    tok = model.encode_images(images)
    r = complete.complete_images(model, ab, images, keep, sample_steps=3, paste=False)
    assert torch.equal(r.tokens, tok) and bool(r.known.all()) and r.n_known.tolist() == [49] * 3
    assert torch.equal(r.images_u8, model.decode_tokens(tok)[1])        # the input's own reconstruction
    pasted = complete.complete_images(model, ab, images, keep, sample_steps=3)
    assert torch.equal(pasted.images_u8, orc.uint8_rule(images))        # ... pasted over by the given pixels


def test_get_data_for_diff_returns_encode_images(dev):
    from snn_model.vq_diffusion import get_data_for_diff
    model = build("mnist_k128", dev)
    images = synth.stroke_images(5, seed=9)
    loader = [(images[:3], torch.zeros(3)), (images[3:], torch.zeros(2))]
    got = get_data_for_diff(loader, model)
    assert len(got) == 2 and got[0].shape == (3, 7, 7) and got[1].shape == (2, 7, 7) and got[0].device.type == "cpu"
    want = model.encode_images((images - 0.5).to(dev)).cpu()
    assert torch.equal(torch.cat(got), want)
