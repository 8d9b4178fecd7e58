"""GPU tests of the completion feature (run with ``-m gpu`` on an MI355X): the two kernels of
csrc/completion.hip against their torch / numpy restatements, ``AbsorbingDiffusion.sample(x_init=, known=)`` in every launch form
against the unconditional call, against itself across forms and graph replays, and against the host oracle
(tests/_completion_oracle.py: the reference's step from the other start state) on the dumped Philox noise, and
``spkdiff.complete.complete_images`` end to end.  Everything is exact (integers) except the one decode check, which takes the
1e-4 the project uses for decoded pixels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _completion_oracle as corc           # noqa: E402
from oracle import snn_ref as ref           # noqa: E402  (checker only)
from parity_report import record as parity  # noqa: E402
from spkdiff import synth                  # noqa: E402

K = 128
FORMS = (("dense", False, False), ("elim", True, False), ("elim+lists", True, True))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


_MODELS = {}


def build_den(cfg, dev):
    from snn_model.vq_diffusion import DummyModel, functional
    if ("den", cfg.img) not in _MODELS:
        sd = synth.synth_denoiser_state(cfg)
        d = DummyModel(1, cfg.num_embeddings).to(dev)
        functional.set_step_mode(net=d, step_mode='m')
        d.load_state_dict(sd)
        _MODELS[("den", cfg.img)] = (d.eval(), sd)
    return _MODELS[("den", cfg.img)]


def build_vae(cfg, dev):
    from snn_model.vae_model import SNN_VQVAE, functional
    if ("vae", cfg.img) not in _MODELS:
        sd = synth.synth_vqvae_state(cfg)
        m = SNN_VQVAE(cfg.in_dim, cfg.latent_dim, cfg.num_embeddings, torch.tensor(1.0))
        functional.set_step_mode(net=m, step_mode='m')
        m.load_state_dict(sd)
        _MODELS[("vae", cfg.img)] = (m.to(dev).eval(), sd)
    return _MODELS[("vae", cfg.img)]


def sampler(den, skip, lists, graph, latent=7):
    from snn_model.vq_diffusion import AbsorbingDiffusion
    ab = AbsorbingDiffusion(den, mask_id=K, latent_shape=(latent, latent))
    ab.skip_untouched, ab.list_positions, ab.use_graph = skip, lists, graph
    ab.n_samples = 3                        # (a conditional call neither reads nor changes it)
    return ab


# ------------------------------------------------------------------------------------------------- 1. the two kernels
@pytest.mark.parametrize("H,h,stride,radius", [(28, 7, 4, 3), (32, 8, 4, 3), (7, 7, 1, 0), (8, 8, 1, 0)])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_completion_state_equals_the_torch_expression(dev, ops, B, H, h, stride, radius):
    g = torch.Generator().manual_seed(B * 100 + H)
    inside = torch.randint(0, K, (B, h, h), generator=g)
    wild = torch.randint(-5, K + 12, (B, h, h), generator=g)          # out-of-range and negative values among them
    wild[0, 0, 0], wild[-1, -1, -1] = -1, K                          # (K is the mask id: never known)
    masks = {"all": torch.ones(B, H, H, dtype=torch.bool), "none": torch.zeros(B, H, H, dtype=torch.bool)}
    for dens in (0.5, 0.9, 0.99, 0.999):
        masks[f"random{dens}"] = torch.rand(B, H, H, generator=g) < dens
    one = torch.ones(B, H, H, dtype=torch.bool)
    py, px = torch.randint(0, H, (B,), generator=g), torch.randint(0, H, (B,), generator=g)
    one[torch.arange(B), py, px] = False
    masks["one_pixel"] = one
    bad = 0
    for name, keep in masks.items():
        for codes in (inside, wild):
            for mk in (keep, keep.to(torch.uint8) * 3):              # bool and uint8 (any non-zero byte = given)
                x_t, un, n = ops.completion_state(codes.to(dev), mk.to(dev), K, K, stride, radius, want_counts=True)
                wx, wu, wn = corc.state_from_mask(codes, keep, K, K, stride, radius)
                assert x_t.shape == (B, 1, h, h) and x_t.dtype == torch.int64 and un.dtype == torch.bool and n.dtype == torch.int32
                bad += int((x_t.cpu() != wx).sum()) + int((un.cpu() != wu).sum()) + int((n.cpu() != wn).sum())
    # one removed pixel: exactly the (at most four) codes whose windows hold it drop out
    _, un, n = ops.completion_state(inside.to(dev), one.to(dev), K, K, stride, radius, want_counts=True)
    un = un.cpu()[:, 0]
    for b in range(B):
        y, x = int(py[b]), int(px[b])
        want = {(i, j) for i in range(h) for j in range(h) if abs(stride * i - y) <= radius and abs(stride * j - x) <= radius}
        got = {(int(i), int(j)) for i, j in torch.nonzero(~un[b]).tolist()}
        assert got == want and len(got) <= 4 and int(n[b]) == h * h - len(got)
        assert radius == 0 or len(got) >= 1
    # a [B,1,h,w] / [B,1,H,W] pair and caller-provided outputs
    xo = torch.empty(B, 1, h, h, dtype=torch.int64, device=dev)
    uo = torch.empty(B, 1, h, h, dtype=torch.bool, device=dev)
    keep = masks["random0.99"]
    r = ops.completion_state(wild.unsqueeze(1).to(dev), keep.unsqueeze(1).to(dev), K, K, stride, radius, out=(xo, uo))
    wx, wu, _ = corc.state_from_mask(wild, keep, K, K, stride, radius)
    assert r[0] is xo and r[1] is uo and r[2] is None
    bad += int((xo.cpu() != wx).sum()) + int((uo.cpu() != wu).sum())
    parity(f"completion_state_B{B}_{H}to{h}_s{stride}r{radius}", cases=len(masks) * 4 + 1, mismatches=bad)
    assert bad == 0


@pytest.mark.parametrize("B,C,H", [(1, 1, 28), (5, 3, 32), (257, 1, 28), (3, 2, 19)])
def test_completion_compose_equals_the_numpy_expression(dev, ops, B, C, H):
    g = torch.Generator().manual_seed(B + H)
    img = torch.rand(B, C, H, H, generator=g) * 1.6 - 0.8              # beyond [-0.5, 0.5] on both sides
    img[0, 0, 0, :8] = torch.tensor([-0.5, 0.5, 0.0, -0.50001, 0.49999, 1e9, -1e9, 0.25])
    k255 = torch.arange(256, dtype=torch.float32) / 255 - 0.5           # every uint8 level's own pre-image
    img.view(-1)[8:8 + min(256, img.numel() - 8)] = k255[:min(256, img.numel() - 8)]
    dec = torch.randint(0, 256, (B, C, H, H), generator=g, dtype=torch.uint8)
    bad = 0
    for dens in (0.0, 0.5, 1.0):
        keep = torch.rand(B, H, H, generator=g) < dens
        want = corc.compose(img.numpy(), keep.numpy(), dec.numpy())
        for kk in (keep, keep.unsqueeze(1).to(torch.uint8)):
            got = ops.completion_compose(img.to(dev), kk.to(dev), dec.to(dev))
            assert got.dtype == torch.uint8 and got.shape == dec.shape
            bad += int((got.cpu().numpy() != want).sum())
    parity(f"completion_compose_B{B}_C{C}_{H}", pixels=int(img.numel()), mismatches=bad)
    assert bad == 0


def test_wrappers_refuse_bad_arguments(dev, ops):
    codes = torch.zeros(2, 7, 7, dtype=torch.int64, device=dev)
    keep = torch.ones(2, 28, 28, dtype=torch.bool, device=dev)
    with pytest.raises(ValueError):
        ops.completion_state(codes, keep[:1], K, K, 4, 3)
    with pytest.raises(ValueError, match="spk_completion_state"):
        ops.completion_state(codes, keep[:, :21], K, K, 4, 3)           # a window that misses the mask
    with pytest.raises(ValueError, match="spk_completion_state"):
        ops.completion_state(codes, keep, 0, K, 4, 3)
    with pytest.raises(NotImplementedError):
        ops.completion_state(codes.int(), keep, K, K, 4, 3)
    with pytest.raises(ValueError):
        ops.completion_compose(torch.zeros(2, 1, 28, 28, device=dev), keep[:, :14], torch.zeros(2, 1, 28, 28, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        ops.completion_compose(torch.zeros(2, 1, 28, 28, device=dev), keep, torch.zeros(2, 3, 28, 28, dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------------------------------------- 2. the two trivial starts
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_nothing_known_is_the_unconditional_call_and_everything_known_comes_back(dev, graph):
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 24, 16
    g = torch.Generator().manual_seed(31)
    x_any = torch.randint(-3, K + 3, (B, 1, 7, 7), generator=g).to(dev)
    x_in = torch.randint(0, K, (B, 7, 7), generator=g).to(dev)
    none = torch.zeros(B, 1, 7, 7, dtype=torch.bool, device=dev)
    every = torch.ones(B, 7, 7, dtype=torch.uint8, device=dev)
    rep = {}
    base = None
    for name, skip, lists in FORMS:
        ab = sampler(den, skip, lists, graph)
        assert ab.form_for(B, 7, 7) in {"dense": ("dense_step_tail", "dense"), "elim": ("elimination",),
                                        "elim+lists": ("elimination_lists",)}[name]
        ab.n_samples = B
        torch.manual_seed(99)
        uncond = ab.sample(1.0, steps)
        ab.n_samples = 3
        torch.manual_seed(99)
        cond = ab.sample(1.0, steps, x_init=x_any, known=none)
        assert cond.shape == (B, 1, 7, 7) and cond.dtype == torch.int64 and ab.n_samples == 3
        base = uncond if base is None else base
        back = ab.sample(1.0, steps, x_init=x_in, known=every)
        rep[name] = dict(vs_unconditional=int((cond != uncond).sum()), vs_dense=int((uncond != base).sum()),
                         all_known_changed=int((back != x_in.unsqueeze(1)).sum()))
        assert len(ab._graphs) == (2 if graph else 0)              # the unconditional graph and the conditional one
        if graph:
            torch.manual_seed(99)
            assert torch.equal(ab.sample(1.0, steps, x_init=x_any, known=none), uncond) and len(ab._graphs) == 2
    parity(f"completion_trivial_starts_{'graph' if graph else 'eager'}", **rep)
    assert all(v == 0 for r in rep.values() for v in r.values()), rep


# ------------------------------------------------------------------------------------------------- 3. the forms agree
def test_forms_agree_and_the_start_state_is_a_graph_input(dev):
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 24, 49
    x_a, k_a = corc.issue_start(B)
    g = torch.Generator().manual_seed(5)
    x_b = torch.randint(0, K, (B, 1, 7, 7), generator=g)
    k_b = torch.rand(B, 1, 7, 7, generator=g) < 0.3
    x_b[0, 0, 3, 3], k_b[0, 0, 3, 3] = K + 7, True                   # a "known" token outside the codebook is resampled
    jobs = [(x_a, k_a, 1), (x_b, k_b, 2), (x_a, k_a, 3), (x_a, k_a, 1)]
    out = {}
    for graph in (True, False):
        for name, skip, lists in FORMS:
            ab = sampler(den, skip, lists, graph)
            res = []
            for x, k, seed in jobs:                                   # different inputs through ONE captured graph
                torch.manual_seed(seed)
                res.append(ab.sample(1.0, steps, x_init=x.to(dev), known=k.to(dev)).cpu())
            assert len(ab._graphs) == (1 if graph else 0)
            out[(name, graph)] = res
    first = out[("dense", False)]
    bad = sum(int((a != b).sum()) for res in out.values() for a, b in zip(res, first))
    kept_bad = masks_left = 0
    for (x, k, _), tok in zip(jobs, first):
        kept = k & (x >= 0) & (x < K)
        kept_bad += int((tok[kept] != x[kept]).sum())
        masks_left += int((tok == K).sum()) + int((tok < 0).sum()) + int((tok > K).sum())
    assert torch.equal(first[0], first[3]) and not torch.equal(first[0], first[2])       # the seed decides, nothing lingers
    assert int(first[1][0, 0, 3, 3]) < K
    parity("completion_forms_agree", forms=len(out), calls=len(jobs), token_mismatches=bad, known_changed=kept_bad,
           mask_ids_left=masks_left)
    assert bad == 0 and kept_bad == 0 and masks_left == 0


# ------------------------------------------------------------------------------------------------- 4. against the oracle
@pytest.mark.parametrize("B,steps", [(4, 100), (256, 6)])
def test_conditional_philox_graph_vs_oracle_on_dumped_noise(dev, ops, B, steps):
    """The timed configuration (Philox noise, the whole reverse process one hipGraph replay; dense and both elimination forms)
    started from known tokens, against the host oracle on the noise the device drew: ZERO differing tokens.  The job is the
    issue's own (synthetic MNIST denoiser, key = the draw after torch.manual_seed(777), start state
    ``_completion_oracle.issue_start``: per image b % 4 the top three rows / the left four columns / a random half / only the
    centre 3x3 known; temp 1.0).  On this job the fp32 oracle and the exact-convolution oracle were checked to give the same
    tokens on the host (0 of 196 and 0 of 12 544 differing, noise from oracle/philox_ref.py), so no spike of the oracle is
    decided by summation order and equality is a fair demand."""
    den, sd = build_den(synth.MNIST, dev)
    x_init, known = corc.issue_start(B)
    got, key = {}, None
    for name, skip, lists in FORMS:
        ab = sampler(den, skip, lists, True)
        assert ab.noise_source == 'philox' and ab.use_graph
        torch.manual_seed(777)
        k = ab._philox_key()
        assert key is None or k == key
        key = k
        torch.manual_seed(777)
        got[name] = ab.sample(temp=1.0, sample_steps=steps, x_init=x_init.to(dev), known=known.to(dev)).cpu()
        assert int(ab.last_key) == key and len(ab._graphs) == 1, "replayed from a captured hipGraph"

    def noise(t):
        u, q = ops.philox_noise(key, (steps - t) * corc.STEP_STRIDE, B, 49, K, dev)
        return u.cpu().view(B, 1, 7, 7), q.cpu()
    want, un = corc.run(sd, x_init, known, steps, noise)
    bad = {n: int((t != want).sum()) for n, t in got.items()}
    print(f"conditional philox+graph B={B} steps={steps}: token mismatches vs oracle on dumped noise {bad} of {want.numel()}")
    parity(f"completion_philox_graph_B{B}_{steps}steps", token_mismatches=bad, tokens=int(want.numel()),
           known_tokens=int(known.sum()))
    assert torch.equal(want[known], x_init[known])
    assert all(v == 0 for v in bad.values()), bad


def test_conditional_host_noise_eager_trajectory_vs_oracle(dev):
    """noise_source = 'host' (u and q from torch's CPU generator in the reference's order), eager, ``record=``: (x_t, unmasked)
    after EVERY step equal to the oracle's under the same seed."""
    den, sd = build_den(synth.MNIST, dev)
    B, steps = 4, 24
    x_init, known = corc.issue_start(B)
    ab = sampler(den, True, True, True)
    ab.noise_source = 'host'
    rec = []
    torch.manual_seed(4242)
    tok = ab.sample(1.0, steps, record=rec, x_init=x_init.to(dev), known=known.to(dev)).cpu()

    def noise(t):
        return torch.rand(B, 1, 7, 7), torch.empty(B * 49, K).exponential_(1)
    rec_o = []
    torch.manual_seed(4242)
    want, _ = corc.run(sd, x_init, known, steps, noise, record=rec_o)
    assert len(rec) == len(rec_o) == steps
    bad = sum(int((r[1].cpu() != o[1]).sum()) + int((r[2].cpu() != o[2]).sum()) for r, o in zip(rec, rec_o))
    assert all(r[0] == o[0] for r, o in zip(rec, rec_o))
    parity("completion_host_noise_trajectory", steps=steps, state_mismatches=bad, token_mismatches=int((tok != want).sum()))
    assert bad == 0 and torch.equal(tok, want)
    # noise= injection: the same call on the dumped host draws, through the elimination loop
    draws = {}
    torch.manual_seed(4242)
    for t in reversed(range(1, steps + 1)):
        draws[t] = noise(t)
    ab2 = sampler(den, True, False, False)
    tok2 = ab2.sample(1.0, steps, noise=lambda t: (draws[t][0].to(dev), draws[t][1].to(dev)), x_init=x_init.to(dev),
                      known=known.to(dev)).cpu()
    assert torch.equal(tok2, want)


# ------------------------------------------------------------------------------------------------- 5. end to end
def _holes(B, H, g):
    """Per image: the bottom half removed / a square hole / a vertical band / scattered 3x3 holes."""
    keep = torch.ones(B, H, H, dtype=torch.bool)
    for b in range(B):
        m = b % 4
        if m == 0:
            keep[b, H // 2:] = False
        elif m == 1:
            keep[b, 8:19, 6:17] = False
        elif m == 2:
            keep[b, :, 10:17] = False
        else:
            for _ in range(4):
                y, x = (int(v) for v in torch.randint(0, H - 3, (2,), generator=g))
                keep[b, y:y + 3, x:x + 3] = False
    return keep


@pytest.mark.parametrize("cfg", [synth.MNIST, synth.CIFAR], ids=["mnist28", "cifar32"])
def test_complete_images_end_to_end(dev, ops, cfg):
    from spkdiff.complete import complete_images
    model, sd_v = build_vae(cfg, dev)
    den, sd_d = build_den(cfg, dev)
    L, H, C, B, steps = cfg.latent, cfg.img, cfg.in_dim, 8, 12
    ab = sampler(den, True, True, True, latent=L)
    g = torch.Generator().manual_seed(H)
    images = synth.stroke_images(B, seed=77, img=H, channels=C) - 0.5
    keep = _holes(B, H, g)
    k4 = keep.unsqueeze(1)
    img_a = torch.where(k4, images, torch.rand(B, C, H, H, generator=g) - 0.5)
    img_b = torch.where(k4, images, torch.rand(B, C, H, H, generator=g) * 4 - 2)
    res = []
    for im, kk in ((img_a, keep), (img_b, k4.to(torch.uint8))):
        torch.manual_seed(2025)
        res.append(complete_images(model, ab, im.to(dev), kk.to(dev), sample_steps=steps))
    ra, rb = res
    assert ra.images_u8.shape == (B, C, H, H) and ra.images_u8.dtype == torch.uint8
    assert ra.tokens.shape == (B, L, L) and ra.tokens.dtype == torch.int64
    assert ra.known.shape == (B, L, L) and ra.known.dtype == torch.bool and ra.n_known.dtype == torch.int32
    hole_dep = sum(int((getattr(ra, f) != getattr(rb, f)).sum()) for f in ("images_u8", "tokens", "known", "n_known"))
    # the codes kept are those the rule says, and they come back unchanged; nothing stays masked
    codes = model.encode_images(img_a.to(dev)).cpu()
    wx, wu, wn = corc.state_from_mask(codes, keep, K, K, 4, 3)
    known = ra.known.cpu()
    tokens = ra.tokens.cpu()
    assert torch.equal(known, wu[:, 0]) and torch.equal(ra.n_known.cpu(), wn)
    assert 0 < int(known.sum()) < known.numel()
    assert torch.equal(tokens[known], codes[known]) and int(tokens.min()) >= 0 and int(tokens.max()) < K
    # the given pixels are the input's, in main.py's conversion
    given = np.array(np.clip(img_a.numpy() + np.float32(0.5), 0.0, 1.0) * 255, dtype=np.uint8)
    u8 = ra.images_u8.cpu().numpy()
    kk = np.broadcast_to(k4.numpy(), u8.shape)
    paste_bad = int((u8[kk] != given[kk]).sum())
    # ... and the rest is the decoder's image of the completed tokens (paste=False: everywhere)
    pred, dec_u8 = model.decode_tokens(ra.tokens)
    assert np.array_equal(u8[~kk], dec_u8.cpu().numpy()[~kk])
    torch.manual_seed(2025)
    rn = complete_images(model, ab, img_a.to(dev), keep.to(dev), sample_steps=steps, paste=False)
    assert torch.equal(rn.tokens, ra.tokens) and torch.equal(rn.images_u8, dec_u8)
    # everything kept: the tokens are the encoder's, the image decode_tokens(encode_images(x))'s
    full = complete_images(model, ab, images.to(dev), torch.ones(B, H, H, dtype=torch.bool, device=dev), sample_steps=steps,
                           paste=False)
    enc = model.encode_images(images.to(dev))
    assert torch.equal(full.tokens, enc) and bool(full.known.all()) and torch.equal(full.n_known.cpu(), torch.full((B,), L * L, dtype=torch.int32))
    assert torch.equal(full.images_u8, model.decode_tokens(enc)[1])
    # the oracle from the same start state on the dumped noise: same tokens, decode within 1e-4
    torch.manual_seed(2025)
    key = ab._philox_key()

    def noise(t):
        u, q = ops.philox_noise(key, (steps - t) * corc.STEP_STRIDE, B, L * L, K, dev)
        return u.cpu().view(B, 1, L, L), q.cpu()
    want, _ = corc.run(sd_d, wx, wu, steps, noise)
    tok_bad = int((tokens != want[:, 0]).sum())
    opred = ref.decode_tokens(want[:, 0], sd_v, 16)
    err = float((pred.cpu() - opred).abs().max())
    print(f"complete_images {H}x{H}: hole dependence {hole_dep}, pasted pixels differing {paste_bad}, tokens vs oracle {tok_bad} of "
          f"{want.numel()}, decode max-abs err {err:.3e}")
    parity(f"complete_images_{H}x{H}", hole_dependent_values=hole_dep, pasted_pixels_differing=paste_bad,
           token_mismatches_vs_oracle=tok_bad, tokens=int(want.numel()), known_tokens=int(known.sum()), decode_max_abs_err=err)
    assert hole_dep == 0 and paste_bad == 0 and tok_bad == 0
    assert err <= 1e-4


# ------------------------------------------------------------------------------------------------- 6. split independence
def test_conditional_job_does_not_depend_on_the_split(dev):
    from spkdiff import dist as sdist
    den, _ = build_den(synth.MNIST, dev)
    B, steps = 48, 20
    x_init, known = corc.issue_start(B)
    x_init, known = x_init.to(dev), known.to(dev)
    ab = sampler(den, True, True, True)
    torch.manual_seed(606)
    whole = ab.sample(1.0, steps, x_init=x_init, known=known)
    parts = []
    for lo, hi in ((0, 24), (24, 48)):
        sh = sampler(den, True, True, True).set_shard(lo, hi - lo)
        torch.manual_seed(606)
        parts.append(sh.sample(1.0, steps, x_init=x_init[lo:hi], known=known[lo:hi]))
    bad = int((torch.cat(parts) != whole).sum())
    cs_whole = sdist.token_checksum(whole, 0)
    cs_parts = (sdist.token_checksum(parts[0], 0) + sdist.token_checksum(parts[1], 24) + 2 ** 63) % 2 ** 64 - 2 ** 63
    parity("completion_split_independence", token_mismatches=bad, checksum_equal=bool(cs_whole == cs_parts))
    assert bad == 0 and cs_whole == cs_parts
    # the second half alone is NOT the first half's noise: the counters sit on the global image index
    un = sampler(den, True, True, True)
    torch.manual_seed(606)
    assert not torch.equal(un.sample(1.0, steps, x_init=x_init[24:], known=known[24:]), parts[1])
