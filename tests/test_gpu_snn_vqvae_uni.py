"""GPU tests of the SNN_VQVAE_uni baseline (spk_vq_code_usage, ops.vq_code_usage, snn_model.vae_model.SNN_VQVAE_uni) against
fixture F18, which the real reference computed on the CPU with ``synth.synth_vqvae_state(synth.MNIST)`` weights
(tools/gen_golden_svqvae_uni.py), against SNN_VQVAE on the same weights, and against the statistic spelled with torch ops."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from spkdiff import _lib, ops, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F18 = os.path.join(ROOT, "tests", "golden", "f18_snn_vqvae_uni.npz")
SUB = 2048


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def f18():
    return np.load(F18)


@pytest.fixture(scope="module")
def sd():
    return synth.synth_vqvae_state(synth.MNIST)


def make_model(sd, name="SNN_VQVAE_uni", data_variance=1.0, print_usage=True):
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    model = ns[name](1, 16, 128, torch.tensor(float(data_variance)))
    ns["functional"].set_step_mode(net=model, step_mode='m')
    model = model.cuda(0)
    model.load_state_dict(sd)
    if name == "SNN_VQVAE_uni":
        model.vq_layer.print_usage = print_usage
    return model.eval(), ns["functional"]


def unpack(f, key):
    shape = tuple(int(s) for s in f[key + "_shape"])
    return torch.from_numpy(np.unpackbits(f[key], axis=-1, count=shape[-1]).reshape(shape)).float()


def parse_usage(text):
    """The four prints of R/snn_model/vae_model.py:714-718 -> (N, valid counts, targets, used, FID_loss); the tensor reprs are
    read as numbers (a device tensor's repr carries a device suffix, the reference's CPU run's does not)."""
    lines = text.strip().splitlines()
    tensors = re.findall(r"tensor\(\[(.*?)\]", text, flags=re.S)
    assert len(tensors) == 2, text
    valid, targets = ([float(v) for v in t.replace("\n", " ").split(",") if v.strip()] for t in tensors)
    m = re.fullmatch(r"torch\.Size\(\[(\d+)\]\) (\S+)", lines[-1])
    assert m, lines[-1]
    return int(lines[0]), valid, targets, int(m.group(1)), float(m.group(2))


def usage_torch(idx, K):
    """The statistic as the reference spells it (R/snn_model/vae_model.py:705-716), on the device."""
    N = len(idx)
    hist = torch.bincount(idx, minlength=K)
    m = torch.argmax(hist)
    mask = torch.ne(torch.arange(K).cuda(), m)
    targets = torch.ones(K) * N / K
    fid = 0.001 * F.mse_loss(torch.masked_select(hist, mask), torch.masked_select(targets.cuda(), mask))
    return hist, int(torch.unique(idx).numel()), int(m), float(fid)


def check_usage(u, idx, K, rtol):
    hist, used, m, fid = usage_torch(idx, K)
    assert torch.equal(u.hist, hist)
    assert (int(u.used), int(u.max_index)) == (used, m)
    if np.isnan(fid):
        assert np.isnan(float(u.fid_loss))
    else:
        assert abs(float(u.fid_loss) - fid) <= rtol * abs(fid) + 1e-30, (float(u.fid_loss), fid)


# ------------------------------------------------------------------------------------------------------------- F18 eval
def test_f18_eval_forward_and_printed_statistic(f18, sd, dev, capsys):
    from snn_model.vae_model import functional
    model, _ = make_model(sd)
    img = torch.from_numpy(f18["images"]).to(dev)
    capsys.readouterr()
    with torch.inference_mode():
        e, x_recon, idx = model(img.unsqueeze(0).repeat(16, 1, 1, 1, 1), img)
    functional.reset_net(model)
    printed = capsys.readouterr().out
    assert torch.equal(idx.cpu(), torch.from_numpy(f18["indices"]))
    assert float((x_recon.cpu() - torch.from_numpy(f18["x_recon"])).abs().max()) <= 1e-4
    assert torch.equal(e.cpu(), unpack(f18, "e"))
    u = model.vq_layer.usage
    assert torch.equal(u.hist.cpu(), torch.from_numpy(f18["hist"]))
    assert int(u.used) == int(f18["used"]) and int(u.max_index) == int(f18["max_index"])
    want_fid = float(f18["fid_loss"])
    assert abs(float(u.fid_loss) - want_fid) <= 1e-6 * want_fid
    n, valid, targets, used, fid = parse_usage(printed)
    rn, rvalid, rtargets, rused, rfid = parse_usage(str(f18["eval_stdout"]))
    assert (n, valid, targets, used) == (rn, rvalid, rtargets, rused)
    assert abs(fid - rfid) <= 1e-6 * rfid
    assert "device='cuda:0'" in printed


def test_uni_eval_equals_snn_vqvae_on_the_same_weights(sd, dev):
    g = torch.Generator().manual_seed(77)
    img = (torch.rand(12, 1, 28, 28, generator=g) - 0.5).to(dev)
    outs = []
    for name in ("SNN_VQVAE", "SNN_VQVAE_uni"):
        model, functional = make_model(sd, name, print_usage=False)
        with torch.inference_mode():
            outs.append(model(img.unsqueeze(0).repeat(16, 1, 1, 1, 1), img))
            functional.reset_net(model)
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ F18 train
def sub_index(n):
    step = n // SUB
    return np.arange(SUB, dtype=np.int64) * step + step // 2


def test_f18_train_iteration(f18, sd, dev, capsys):
    img = torch.from_numpy(f18["images"]).to(dev)
    x = img.unsqueeze(0).repeat(16, 1, 1, 1, 1)
    var = float(f18["data_variance"])
    model, functional = make_model(sd, data_variance=var)
    model.train()
    capsys.readouterr()
    leq, lrec, lreal = model(x, img)
    (leq + lrec).backward()
    printed = capsys.readouterr().out
    rel = {k: abs(float(v.detach()) - float(f18[k])) / float(f18[k]) for k, v in
           (("loss_eq", leq), ("loss_rec", lrec), ("real_loss_rec", lreal))}
    gerr, norms = {}, {}
    params = dict(model.named_parameters())
    # a convolution bias in front of a batch-statistics BatchNorm has a zero gradient: both sides hold only round-off
    before_bn = set()
    for prefix, seq in (("encoder.snn_convs", model.encoder.snn_convs), ("decoder.snn_convs", model.decoder.snn_convs),
                        ("vq_layer.poisson", model.vq_layer.poisson)):
        kids = list(seq)
        before_bn |= {f"{prefix}.{i}.bias" for i in range(len(kids) - 1) if "BatchNorm" in type(kids[i + 1]).__name__}
    for k in f18.files:
        if not k.startswith("grad/") or k.endswith(("/shape", "/norm")):
            continue
        name = k[5:].split("/")[0]
        g = params[name].grad.detach().cpu().reshape(-1) if params[name].grad is not None else torch.zeros(params[name].numel())
        want = torch.from_numpy(f18[k]).reshape(-1)
        norms[name] = (float(g.double().norm()), float(f18[f"grad/{name}/norm"]) if k.endswith("/sub") else float(want.norm()))
        if k.endswith("/sub"):
            got_norm, want_norm = norms[name]
            assert abs(got_norm - want_norm) <= 5e-2 * want_norm + 5e-5, (name, got_norm, want_norm)
            g = g[torch.from_numpy(sub_index(g.numel()))]
        if float(want.norm()) > 1e-6 and name not in before_bn:
            gerr[name] = float((g - want).norm() / want.norm())
    print("F18 train measured: loss rel err", rel, "grad rel L2", gerr)
    assert max(rel.values()) <= 2e-2, rel
    assert max(gerr.values()) <= 5e-2, gerr
    top = max(max(v) for v in norms.values())
    for name in before_bn:
        assert max(norms[name]) <= 1e-3 * top, (name, norms[name], top)
    assert leq.dtype == torch.float32 and leq.is_cuda
    n, valid, targets, used, fid = parse_usage(printed)          # train() mode prints the statistic too
    assert n == 392 and len(valid) == 127 and used == int(model.vq_layer.usage.used)
    functional.reset_net(model)
    # the returned loss_eq is SNN_VQVAE's loss on the same run (FID_loss is a CPU int64 zero in train() mode)
    plain, functional = make_model(sd, "SNN_VQVAE", data_variance=var)
    plain.train()
    model.load_state_dict(sd)
    outs = []
    for m in (plain, model):
        outs.append(m(x, img))
        functional.reset_net(m)
    assert torch.equal(outs[0][0].detach(), outs[1][0].detach())
    assert torch.equal(outs[0][1].detach(), outs[1][1].detach())


# ------------------------------------------------------------------------------------------------ kernel against torch
@pytest.mark.parametrize("K", [1, 2, 16, 127, 128, 129, 512, 4096])
@pytest.mark.parametrize("N", [1, 49, 392, 65539, 401408])
def test_vq_code_usage_matches_torch(N, K, dev):
    g = torch.Generator().manual_seed(N * 7919 + K)
    idx = torch.randint(0, K, (N,), generator=g).to(dev)
    u = ops.vq_code_usage(idx, K)
    check_usage(u, idx, K, 1e-5)
    again = ops.vq_code_usage(idx, K)
    assert torch.equal(u.packed, again.packed)            # bitwise-equal repeat (fid_loss bits included)


@pytest.mark.parametrize("K", [2, 128, 4096])
def test_vq_code_usage_special_distributions(K, dev):
    # tied maxima: codes K-1 and 1 hold the same largest count; the smaller code wins
    idx = torch.tensor([K - 1] * 5 + [1] * 5 + [0] * 3, device=dev)
    u = ops.vq_code_usage(idx, K)
    check_usage(u, idx, K, 1e-5)
    assert int(u.max_index) == 1
    # every index on one code
    idx = torch.full((40000,), K // 2, dtype=torch.int64, device=dev)
    u = ops.vq_code_usage(idx, K)
    check_usage(u, idx, K, 1e-5)
    assert int(u.used) == 1 and int(u.max_index) == K // 2
    # one index per code: every count ties, code 0 wins, the loss is 0
    idx = torch.randperm(K).to(dev)
    u = ops.vq_code_usage(idx, K)
    check_usage(u, idx, K, 1e-5)
    assert int(u.used) == K and int(u.max_index) == 0 and float(u.fid_loss) == 0.0


def test_vq_code_usage_above_the_lds_limit_takes_the_fallback(dev):
    K = ops.VQ_USAGE_MAX_K + 1
    idx = torch.randint(0, K, (9000,), generator=torch.Generator().manual_seed(5)).to(dev)
    packed = torch.empty(K + 3, dtype=torch.int64, device=dev)
    ws = torch.empty(K + 1, dtype=torch.int64, device=dev)
    rc = _lib.lib.spk_vq_code_usage(idx.data_ptr(), idx.numel(), K, packed.data_ptr(), packed[K:].data_ptr(), ws.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == -2                                     # SPK_ERR_UNSUPPORTED: nothing launched
    u = ops.vq_code_usage(idx, K)
    check_usage(u, idx, K, 1e-5)
    assert u.hist.is_cuda and u.fid_loss.dtype == torch.float32


# ------------------------------------------------------------------------------------------------------ print_usage off
def test_print_usage_off_is_silent_and_capturable(sd, dev, capsys):
    g = torch.Generator().manual_seed(91)
    img = (torch.rand(8, 1, 28, 28, generator=g) - 0.5).to(dev)
    x = img.unsqueeze(0).repeat(16, 1, 1, 1, 1)
    loud, functional = make_model(sd, print_usage=True)
    quiet, _ = make_model(sd, print_usage=False)
    capsys.readouterr()
    with torch.inference_mode():
        ref = loud(x, img)
        functional.reset_net(loud)
        assert capsys.readouterr().out != ""
        got = quiet(x, img)
        functional.reset_net(quiet)
    assert capsys.readouterr().out == ""
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    assert torch.equal(loud.vq_layer.usage.packed, quiet.vq_layer.usage.packed)
    # an eval forward captured in a hipGraph and replayed gives the eager outputs and statistic
    store = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.inference_mode():
        with torch.cuda.stream(side), ops.flag_scope(store):
            quiet(x, img)
            functional.reset_net(quiet)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), ops.flag_scope(store):
            out_g = quiet(x, img)
        usage_g = quiet.vq_layer.usage
        functional.reset_net(quiet)
        graph.replay()
        torch.cuda.synchronize()
    assert capsys.readouterr().out == ""
    for a, b in zip(ref, out_g):
        assert torch.equal(a, b)
    assert torch.equal(usage_g.packed, loud.vq_layer.usage.packed)


# ------------------------------------------------------------------------------------------ R/main.py snn-vq-vae-uni replay
def test_main_py_snn_vq_vae_uni_replay(sd, dev, capsys):
    """R/main.py --model snn-vq-vae-uni on synthetic tensors: the training step with AdamW (:126-146), the per-epoch
    reconstruction (:175-178), get_data_for_diff over two batches and one diffusion training iteration on its codes
    (:202-252), the decode glue (:264-273)."""
    ns = {}
    exec("from snn_model.snn_layers import *\nfrom snn_model.vae_model import *\nfrom snn_model.vq_diffusion import *", ns)
    functional = ns["functional"]
    model = ns["SNN_VQVAE_uni"](1, 16, 128, torch.tensor(0.09))
    functional.set_step_mode(net=model, step_mode='m')
    model = model.cuda(0)
    model.load_state_dict(sd)
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.001)
    g = torch.Generator().manual_seed(2026)
    before = model.vq_layer.embeddings.weight.detach().clone()
    model.train()
    for _ in range(2):
        images = (torch.rand(8, 1, 28, 28, generator=g) - 0.5).cuda(0)
        images_spike = images.unsqueeze(0).repeat(16, 1, 1, 1, 1)
        loss_eq, loss_rec, real_loss_rec = model(images_spike, images)
        optimizer.zero_grad()
        (loss_eq + loss_rec).backward()
        optimizer.step()
        functional.reset_net(model)
        line = "loss {:.3f} loss_eq {:.3f} loss_rec {:.3f}".format((loss_eq + loss_rec).item(), float(loss_eq), float(real_loss_rec))
        assert "nan" not in line
    assert not torch.equal(before, model.vq_layer.embeddings.weight.detach())
    model.eval()
    norm_images = (torch.rand(32, 1, 28, 28, generator=g) - 0.5).cuda(0)
    with torch.inference_mode():
        images_spike = norm_images.unsqueeze(0).repeat(16, 1, 1, 1, 1)
        e, recon_images, _ = model(images_spike, norm_images)
        functional.reset_net(model)
    recon = np.array(np.clip((recon_images + 0.5).cpu().numpy(), 0., 1.) * 255, dtype=np.uint8)
    assert recon.shape == (32, 1, 28, 28) and e.shape == (16, 32, 16, 7, 7)
    capsys.readouterr()
    loader = [(torch.rand(32, 1, 28, 28, generator=g), torch.zeros(32)) for _ in range(2)]
    train_indices = ns["get_data_for_diff"](loader, model)
    printed = capsys.readouterr().out
    assert printed.count("torch.Size([") == 2                     # the statistic, once per batch, as in the reference
    assert len(train_indices) == 2 and train_indices[0].shape == (32, 7, 7) and train_indices[0].dtype == torch.int64
    denoise_fn = ns["DummyModel"](1, 128).cuda(0)
    functional.set_step_mode(net=denoise_fn, step_mode='m')
    denoise_fn.load_state_dict(synth.synth_denoiser_state(synth.MNIST))
    abdiff = ns["AbsorbingDiffusion"](denoise_fn, mask_id=128)
    opt_d = torch.optim.AdamW(denoise_fn.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.001)
    denoise_fn.train()
    indices = train_indices[0].float().cuda(0).unsqueeze(dim=1)
    loss = abdiff.train_iter(indices)['loss']
    opt_d.zero_grad()
    loss.backward()
    opt_d.step()
    functional.reset_net(net=denoise_fn)
    assert np.isfinite(loss.item())
    denoise_fn.eval()
    sample = torch.cat([train_indices[0][:16], train_indices[1][:16]], dim=0).reshape(32, 7, 7)

    def glue():
        with torch.inference_mode():
            z = model.vq_layer.quantize(sample.cuda(0))
            z = z.permute(0, 3, 1, 2).contiguous()
            quantized = torch.unsqueeze(z, dim=0).repeat(16, 1, 1, 1, 1)
            quantized = model.vq_layer.poisson(quantized)
            pred = model.decoder(quantized)
            return torch.tanh(model.memout(pred))

    pred = glue()                 # (as in R/main.py, on the membrane state get_data_for_diff's batches of 32 left behind)
    generated = np.array(np.clip((pred + 0.5).cpu().numpy(), 0., 1.) * 255, dtype=np.uint8)
    assert generated.shape == (32, 1, 28, 28)
    functional.reset_net(model)
    pred = glue()
    functional.reset_net(model)
    fast, _ = model.decode_tokens(sample.cuda(0))
    assert float((fast - pred).abs().max()) <= 1e-4
