"""GPU tests of the reconstruction metrics of R/main.py:300-323 (spk_ssim_mse, ops.ssim_mse, metric.pytorch_ssim,
spkdiff.evaluate) against fixture F19 (the real reference's fp32 values, tools/gen_golden_recon_metrics.py) and against the fp64
oracle tests/_recon_metric_oracle.py, which also holds the bounds and their derivation:
    |hip - o| <= 2^-23 |o| + 1e-10          and          |hip - r| <= |r - o| + 2^-23 |o| + 1e-10."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _recon_metric_oracle as orc
import parity_report
from spkdiff import evaluate, ops, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F19 = os.path.join(ROOT, "tests", "golden", "f19_recon_metrics.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def f19():
    return np.load(F19)


@pytest.fixture(scope="module")
def ps():
    import metric.pytorch_ssim as m
    return m


def win2d(ps, ws, dev=None):
    w = ps.create_window(ws, 1)[0, 0].contiguous()
    return w if dev is None else w.to(dev)


def hip_values(ps, a, b, ws, dev):
    """Every public route on the device: SSIM (both forms), ssim, and ops.ssim_mse -> fp32 results."""
    ad, bd = a.to(dev), b.to(dev)
    N, C, H, W = a.shape
    with torch.no_grad():
        mean = ps.SSIM(window_size=ws)(ad, bd)
        per = ps.SSIM(window_size=ws, size_average=False)(ad, bd)
        fn = ps.ssim(ad, bd, ws)
        fn_per = ps.ssim(ad, bd, ws, False)
    ssim_sum, sq_sum = ops.ssim_mse(ad, bd, win2d(ps, ws, dev))
    assert ssim_sum.dtype == sq_sum.dtype == torch.float64 and ssim_sum.shape == sq_sum.shape == (N,)
    assert mean.dtype == per.dtype == torch.float32 and mean.dim() == 0 and per.shape == (N,) and mean.is_cuda
    cnt = C * ops.ssim_mse_out_size(H, ws) * ops.ssim_mse_out_size(W, ws)
    return dict(mean=float(mean), per=per.cpu().double().numpy(), fn=float(fn), fn_per=fn_per.cpu().double().numpy(),
                ops_mean=float((ssim_sum.sum() / (N * cnt)).float()), ops_per=(ssim_sum / cnt).float().cpu().double().numpy(),
                mse=float((sq_sum.sum() / a.numel()).float()), ssim_sum=ssim_sum.cpu(), sq_sum=sq_sum.cpu())


def check_against_oracle(got, o_mean, o_per, o_mse, what):
    """The first bound on every route; returns the largest |hip - o| seen."""
    worst = 0.0
    for key, o in (("mean", o_mean), ("fn", o_mean), ("ops_mean", o_mean), ("mse", o_mse)):
        err = abs(got[key] - float(o))
        print(f"{what}: {key} hip {got[key]:.9g} oracle {float(o):.12g} |hip - o| {err:.3e} bound {float(orc.hip_bound(o)):.3e}")
        assert err <= orc.hip_bound(o), (what, key, err)
        worst = max(worst, err)
    for key in ("per", "fn_per", "ops_per"):
        err = np.abs(got[key] - np.asarray(o_per))
        print(f"{what}: {key} max |hip - o| {err.max():.3e}")
        assert (err <= orc.hip_bound(o_per)).all(), (what, key, err.max())
        worst = max(worst, float(err.max()))
    return worst


# ------------------------------------------------------------------------------------------------- F19
@pytest.mark.parametrize("name", orc.CASES)
def test_f19_both_bounds(f19, ps, dev, name):
    c = orc.load_case(f19, name)
    got = hip_values(ps, c["a"], c["b"], c["ws"], dev)
    worst = check_against_oracle(got, c["o_mean"], c["o_per"], c["o_mse"], name)
    # against the reference's fp32 values: the triangle inequality
    for key, r, o in (("mean", c["r_mean"], c["o_mean"]), ("fn", c["r_fn"], c["o_mean"]), ("ops_mean", c["r_mean"], c["o_mean"]),
                      ("mse", c["r_mse"], c["o_mse"])):
        err = abs(got[key] - float(r))
        print(f"{name}: {key} |hip - r| {err:.3e} bound {float(orc.ref_bound(r, o)):.3e}")
        assert err <= orc.ref_bound(r, o), (name, key, err)
    for key in ("per", "fn_per", "ops_per"):
        err = np.abs(got[key] - c["r_per"].astype(np.float64))
        assert (err <= orc.ref_bound(c["r_per"], c["o_per"])).all(), (name, key, err.max())
    r_o = max(abs(float(c["r_mean"]) - float(c["o_mean"])), float(np.abs(c["r_per"].astype(np.float64) - c["o_per"]).max()),
              abs(float(c["r_mse"]) - float(c["o_mse"])))
    parity_report.record(f"recon_metrics_f19_{name}", max_abs_hip_minus_oracle=worst, max_abs_reference_minus_oracle=r_o)


# ------------------------------------------------------------------------------------------------- live shapes
def live_pair(shape, seed):
    """A smooth image in [-0.5, 0.5] and a noisy, slightly blurred copy (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    if (C, H, W) == (1, 28, 28):
        a = synth.stroke_images(N, seed=seed)
    else:
        a = F.avg_pool2d(torch.rand(N, C, H + 2, W + 2, generator=g), 3, stride=1)
    b = (0.7 * a + 0.3 * F.avg_pool2d(F.pad(a, (1, 1, 1, 1), mode="replicate"), 3, stride=1)
         + 0.05 * torch.randn(a.shape, generator=g)).clamp(0, 1)
    return (a - 0.5).contiguous(), (b - 0.5).contiguous()


LIVE = [((1, 1, 28, 28), 11), ((31, 1, 28, 28), 11), ((32, 1, 28, 28), 11), ((256, 1, 28, 28), 11), ((1000, 1, 28, 28), 11),
        ((6, 3, 32, 32), 11), ((5, 2, 19, 23), 7), ((4, 1, 28, 28), 1), ((4, 1, 28, 28), 8), ((3, 2, 32, 32), 8),
        ((4, 1, 28, 28), 31), ((2, 1, 9, 9), 11), ((4, 1, 64, 48), 11), ((2, 1, 300, 200), 11), ((2, 1, 70, 45), 30)]


@pytest.mark.parametrize("shape,ws", LIVE, ids=[f"{'x'.join(map(str, s))}_w{w}" for s, w in LIVE])
def test_live_shapes_against_the_oracle(ps, dev, shape, ws):
    a, b = live_pair(shape, seed=100 + ws + shape[0])
    got = hip_values(ps, a, b, ws, dev)
    w = win2d(ps, ws)
    o_mean, o_per = orc.ssim64(a, b, w)
    worst = check_against_oracle(got, o_mean, o_per.numpy(), orc.mse64(a, b), f"{shape} ws {ws}")
    # the raw per-image sums
    o_ssum, o_qsum = orc.sums64(a, b, w)
    assert torch.allclose(got["ssim_sum"], o_ssum, rtol=2.0 ** -23, atol=1e-10 * o_ssum.numel())
    assert torch.allclose(got["sq_sum"], o_qsum, rtol=2.0 ** -23, atol=1e-10)
    parity_report.record(f"recon_metrics_live_{'x'.join(map(str, shape))}_w{ws}", max_abs_hip_minus_oracle=worst)


# ------------------------------------------------------------------------------------------------- edge values
def test_identical_inputs_are_exact(ps, dev):
    for shape, ws in (((32, 1, 28, 28), 11), ((3, 3, 32, 32), 8), ((2, 1, 100, 70), 11)):
        a, _ = live_pair(shape, seed=7)
        ad = a.to(dev)
        assert float(ps.SSIM(window_size=ws)(ad, ad.clone())) == 1.0
        assert torch.equal(ps.SSIM(window_size=ws, size_average=False)(ad, ad.clone()).cpu(), torch.ones(shape[0]))
        _, sq = ops.ssim_mse(ad, ad.clone(), win2d(ps, ws, dev))
        assert torch.equal(sq.cpu(), torch.zeros(shape[0], dtype=torch.float64))


def test_one_nan_pixel_stays_in_its_image(ps, dev):
    a, b = live_pair((8, 1, 28, 28), seed=21)
    w = win2d(ps, 11, dev)
    s0, q0 = (t.cpu() for t in ops.ssim_mse(a.to(dev), b.to(dev), w))
    for which in ("a", "b"):
        a2, b2 = a.clone(), b.clone()
        (a2 if which == "a" else b2)[5, 0, 13, 2] = float("nan")
        s1, q1 = (t.cpu() for t in ops.ssim_mse(a2.to(dev), b2.to(dev), w))
        keep = torch.arange(8) != 5
        assert torch.isnan(s1[5]) and torch.isnan(q1[5])
        assert torch.equal(s1[keep], s0[keep]) and torch.equal(q1[keep], q0[keep])
        per = ps.SSIM(size_average=False)(a2.to(dev), b2.to(dev)).cpu()
        assert torch.isnan(per[5]) and not torch.isnan(per[keep]).any()
        assert torch.isnan(ps.SSIM()(a2.to(dev), b2.to(dev)))


# ------------------------------------------------------------------------------------------------- determinism, workspace
def test_two_calls_bit_equal_and_workspace_contents_do_not_matter(ps, dev):
    for shape, ws in (((32, 1, 28, 28), 11), ((2, 1, 300, 200), 11), ((5, 2, 19, 23), 7)):
        a, b = (t.to(dev) for t in live_pair(shape, seed=3))
        w = win2d(ps, ws, dev)
        s0, q0 = ops.ssim_mse(a, b, w)
        s1, q1 = ops.ssim_mse(a, b, w)
        assert torch.equal(s0, s1) and torch.equal(q0, q1)
        buf = ops.ssim_mse_ws(*shape, ws, dev)
        assert buf.numel() * 8 == ops.lib.spk_ssim_mse_ws_bytes(*shape, ws)
        for _ in range(2):
            buf.fill_(-1)                                   # every byte 0xFF
            s2, q2 = ops.ssim_mse(a, b, w, ws=buf)
            assert torch.equal(s0, s2) and torch.equal(q0, q2)


def test_interleaved_calls_on_one_workspace_each(ps, dev):
    """Two evaluations (two models' loops) alternate on the same stream, each with a workspace and an output of its own."""
    w = win2d(ps, 11, dev)
    pairs = [tuple(t.to(dev) for t in live_pair((32, 1, 28, 28), seed=s)) for s in (31, 32)]
    want = [tuple(t.clone() for t in ops.ssim_mse(a, b, w)) for a, b in pairs]
    bufs = [ops.ssim_mse_ws(32, 1, 28, 28, 11, dev) for _ in pairs]
    outs = [torch.empty((2, 32), dtype=torch.float64, device=dev) for _ in pairs]
    for _ in range(5):
        for k, (a, b) in enumerate(pairs):
            ops.ssim_mse(a, b, w, ws=bufs[k], out=outs[k])
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(outs[k][0], want[k][0]) and torch.equal(outs[k][1], want[k][1])
    assert not torch.equal(want[0][0], want[1][0])


# ------------------------------------------------------------------------------------------------- input forms, launch context
def test_non_contiguous_inputs_and_inference_mode_tensors(ps, dev):
    a, b = (t.to(dev) for t in live_pair((6, 3, 32, 32), seed=11))
    want = ps.SSIM()(a, b)
    want_per = ps.SSIM(size_average=False)(a, b)
    a_cl, b_cl = a.contiguous(memory_format=torch.channels_last), b.contiguous(memory_format=torch.channels_last)
    assert not a_cl.is_contiguous()
    assert torch.equal(ps.SSIM()(a_cl, b_cl), want) and torch.equal(ps.ssim(a_cl, b), want)
    big_a, big_b = torch.zeros(6, 3, 40, 36, device=dev), torch.zeros(6, 3, 40, 36, device=dev)
    big_a[:, :, 4:36, 2:34], big_b[:, :, 4:36, 2:34] = a, b
    sa, sb = big_a[:, :, 4:36, 2:34], big_b[:, :, 4:36, 2:34]
    assert not sa.is_contiguous()
    assert torch.equal(ps.SSIM(size_average=False)(sa, sb), want_per)
    s_ref, q_ref = ops.ssim_mse(a, b, win2d(ps, 11, dev))
    s_sl, q_sl = ops.ssim_mse(sa, sb, win2d(ps, 11, dev))
    assert torch.equal(s_ref, s_sl) and torch.equal(q_ref, q_sl)
    with torch.inference_mode():
        ai, bi = a * 1.0, b * 1.0
        got = ps.SSIM()(ai, bi)
    assert ai.is_inference() and torch.equal(got, want)
    assert torch.equal(ps.SSIM()(ai, bi), want)             # inference tensors used outside the mode


def test_inputs_that_require_grad_take_the_torch_path(ps, dev, monkeypatch):
    a, b = (t.to(dev) for t in live_pair((4, 1, 28, 28), seed=12))
    calls = []
    real = ops.ssim_mse
    monkeypatch.setattr(ops, "ssim_mse", lambda *x, **k: calls.append(1) or real(*x, **k))
    x = a.clone().requires_grad_(True)
    loss = 1 - ps.SSIM()(x, b)
    assert not calls
    loss.backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    with torch.no_grad():
        ps.SSIM()(x, b)
    assert len(calls) == 1
    ps.SSIM()(a.double(), b.double())                       # other dtypes: the torch path
    ps.SSIM(window_size=33)(a, b)                           # a window above the kernel's limit too
    assert len(calls) == 1


def test_non_default_stream(ps, dev):
    a, b = (t.to(dev) for t in live_pair((32, 1, 28, 28), seed=13))
    w = win2d(ps, 11, dev)
    want = tuple(t.clone() for t in ops.ssim_mse(a, b, w))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = ops.ssim_mse(a, b, w)
        val = ps.SSIM()(a, b)
    st.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(val, ps.SSIM()(a, b))


def test_graph_capture_and_three_replays(ps, dev):
    """One capture, then three replays, each after the static inputs were overwritten with another batch on the same stream:
    every replay equals the eager result of its batch bit for bit (a kernel that depended on the cache maintenance of the
    replayed dispatch returned the first batch's result from the second replay on: DESIGN 4.8)."""
    w = win2d(ps, 11, dev)
    data = [tuple(t.to(dev) for t in live_pair((32, 1, 28, 28), seed=40 + k)) for k in range(3)]
    eager = [tuple(t.clone() for t in ops.ssim_mse(a, b, w)) for a, b in data]
    sa, sb = data[0][0].clone(), data[0][1].clone()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.ssim_mse(sa, sb, w)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gs, gq = ops.ssim_mse(sa, sb, w)
    for k, (a, b) in enumerate(data):
        sa.copy_(a)
        sb.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gs, eager[k][0]) and torch.equal(gq, eager[k][1]), f"replay {k}"


# ------------------------------------------------------------------------------------------------- end to end
E2E_SEED = {"SNN_VQVAE": 2034, "SNN_VAE": 2034}        # see the assertion on the rounding boundary below


def e2e_model(kind, dev):
    ns = {}
    exec("from snn_model.vae_model import *", ns)
    if kind == "SNN_VQVAE":
        model, sd = ns["SNN_VQVAE"](1, 16, 128, torch.tensor(1.0)), synth.trained_state("vqvae")
    else:
        model, sd = ns["SNN_VAE"](), synth.synth_svae_state()
    ns["functional"].set_step_mode(net=model, step_mode='m')
    model.load_state_dict(sd)
    return model.cuda(0).eval(), ns["functional"]


def e2e_figures(kind, seed, dev, ps):
    """reconstruction_eval and the literal loop of R/main.py:304-323 (the torch-op SSIM, two .item() per batch) on five batches
    of 32 and one of 16 stroke images; per batch the fp64 oracle on the literal loop's reconstruction."""
    model, functional = e2e_model(kind, dev)
    images = synth.stroke_images(5 * 32 + 16, seed=seed)
    batches = [(images[i:i + 32], torch.zeros(len(images[i:i + 32]), dtype=torch.int64)) for i in range(0, len(images), 32)]
    assert [len(b[0]) for b in batches] == [32] * 5 + [16]
    torch.manual_seed(seed)
    res = evaluate.reconstruction_eval(model, batches)
    # the script's loop, as written
    torch.manual_seed(seed)
    loss_mse, loss_ssim, b_ssim, b_mse, o_loss, o_mse = [], [], [], [], [], []
    w2 = win2d(ps, 11)
    for i, (imgs, labels) in enumerate(batches):
        norm_images = (imgs - 0.5).cuda(0)
        with torch.inference_mode():
            images_spike = norm_images.unsqueeze(0).repeat(16, 1, 1, 1, 1)
            recon_images = model(images_spike, norm_images)[1]
            functional.reset_net(model)
            loss_mse.append(F.mse_loss(recon_images, norm_images).item())
            window = ps.create_window(11, 1).to(dev)
            loss_ssim.append((1 - ps.ssim_torch(recon_images, norm_images, window, 11, 1)).item())
        o_s, _ = orc.ssim64(recon_images.cpu(), norm_images.cpu(), w2)
        o_m = orc.mse64(recon_images.cpu(), norm_images.cpu())
        o_s, o_m = float(o_s), float(o_m)
        o_loss.append(1 - o_s)
        o_mse.append(o_m)
        # per batch: |hip - lit| <= |lit - o| + 2^-23 |o| + 1e-10; the loss adds the fp32 rounding of 1 - ssim on both sides
        b_ssim.append(abs((1 - o_s) - loss_ssim[-1]) + float(orc.hip_bound(o_s)) + orc.EPS32 * abs(1 - o_s))
        b_mse.append(abs(o_m - loss_mse[-1]) + float(orc.hip_bound(o_m)))
    lit = evaluate.aggregate(loss_ssim, loss_mse)

    def edge(x):                                            # distance of x to the nearest boundary of round(x, 3)
        return abs((x * 1000 - 0.5) - round(x * 1000 - 0.5)) / 1000

    return dict(res=res, lit=lit, bound_ssim=sum(b_ssim) / len(b_ssim), bound_mse=sum(b_mse) / len(b_mse),
                o_loss=sum(o_loss) / len(o_loss), o_mse=sum(o_mse) / len(o_mse),
                edge_ssim=edge(sum(o_loss) / len(o_loss)), edge_mse=edge(sum(o_mse) / len(o_mse)))


@pytest.mark.parametrize("kind", ["SNN_VQVAE", "SNN_VAE"])
def test_reconstruction_eval_end_to_end(ps, dev, kind, monkeypatch):
    calls = []
    real = ops.ssim_mse
    monkeypatch.setattr(ops, "ssim_mse", lambda *x, **k: calls.append(1) or real(*x, **k))
    f = e2e_figures(kind, E2E_SEED[kind], dev, ps)
    res, lit = f["res"], f["lit"]
    print(f"{kind}: eval {res} literal {lit} bounds ssim {f['bound_ssim']:.3e} mse {f['bound_mse']:.3e} oracle means "
          f"{f['o_loss']:.9f} {f['o_mse']:.9f} distance to a rounding boundary {f['edge_ssim']:.3e} {f['edge_mse']:.3e}")
    assert len(calls) == 6 == res["n_batches"] == lit["n_batches"]      # one metric launch per batch (the literal loop makes none)
    assert abs(res["loss_ssim"] - lit["loss_ssim"]) <= f["bound_ssim"]
    assert abs(res["loss_mse"] - lit["loss_mse"]) <= f["bound_mse"]
    # the seed keeps the oracle means further from a boundary of round(., 3) than the bounds: the printed values must agree
    assert f["edge_ssim"] > f["bound_ssim"] and f["edge_mse"] > f["bound_mse"]
    assert res["loss_ssim_rounded"] == lit["loss_ssim_rounded"] and res["loss_mse_rounded"] == lit["loss_mse_rounded"]
    parity_report.record(f"recon_eval_{kind}", loss_ssim=res["loss_ssim"], loss_mse=res["loss_mse"],
                         abs_diff_ssim=abs(res["loss_ssim"] - lit["loss_ssim"]), abs_diff_mse=abs(res["loss_mse"] - lit["loss_mse"]),
                         bound_ssim=f["bound_ssim"], bound_mse=f["bound_mse"])
