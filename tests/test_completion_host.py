"""CPU tests of the completion feature: the two C-ABI entry points of csrc/completion.hip are declared,
exported and bound and reject bad arguments on the host; ``AbsorbingDiffusion.sample(x_init=, known=)`` keeps the existing
signature in front and checks its new arguments before anything is drawn or launched; the test-side oracle's state and
compose rules; the host oracle of the conditional reverse process keeps the known tokens."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _completion_oracle as corc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_exported_and_bound():
    from spkdiff import _lib
    txt = open(os.path.join(ROOT, "include", "spkdiff.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("spk_completion_state", "spk_completion_compose"):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/spkdiff.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libspkdiff.so"
        assert name in _lib.EXPORTS
    assert len(_lib.lib.spk_completion_state.argtypes) == 15
    assert _lib.lib.spk_completion_state.argtypes[13] is ctypes.c_longlong          # mask_id
    assert len(_lib.lib.spk_completion_compose.argtypes) == 9
    assert _lib.lib.spk_completion_state.restype is ctypes.c_int and _lib.lib.spk_completion_compose.restype is ctypes.c_int
    assert _lib.version() == _lib.EXPECTED_VERSION == 106           # additive: the ABI version stays
    assert os.path.exists(os.path.join(ROOT, "spiking-diffusion_amd", "csrc", "completion.hip"))


def test_host_rejection_before_any_launch():
    """Null pointers and bad sizes: SPK_ERR_ARG (-1), decided on the host before any launch -- no GPU is needed (the non-null
    pointers here are host addresses)."""
    from spkdiff import _lib
    lib = _lib.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ok = [p, p, p, p, None]                               # (the per-image count is optional)
    good = (2, 7, 7, 28, 28, 4, 3, 128, 128)              # B, h, w, Hm, Wm, stride, radius, K, mask_id
    for k in range(4):
        args = list(ok)
        args[k] = None
        assert lib.spk_completion_state(*args, *good, None) == -1, f"null pointer argument {k}"
    for k, bad in ((0, 0), (0, -1), (1, 0), (2, 0), (3, 0), (4, -2), (5, 0), (5, -1), (6, -1), (7, 0), (7, -5)):
        sizes = list(good)
        sizes[k] = bad
        assert lib.spk_completion_state(*ok, *sizes, None) == -1, (k, bad)
    # a token whose window misses the mask altogether: 7 tokens at stride 4 and radius 3 need 22 mask rows at least
    assert lib.spk_completion_state(*ok, 2, 7, 7, 21, 28, 4, 3, 128, 128, None) == -1
    assert lib.spk_completion_state(*ok, 2, 7, 7, 28, 21, 4, 3, 128, 128, None) == -1
    assert lib.spk_completion_state(*ok, 2, 7, 7, 6, 7, 1, 0, 128, 128, None) == -1
    assert lib.spk_completion_state(*ok, 1 << 20, 1 << 6, 1 << 6, 1 << 6, 1 << 6, 1, 0, 128, 128, None) == -1      # 2^32 tokens

    okc = [p, p, p, p]
    for k in range(4):
        args = list(okc)
        args[k] = None
        assert lib.spk_completion_compose(*args, 1, 1, 8, 8, None) == -1, f"null pointer argument {k}"
    for sizes in ((0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (-1, 1, 8, 8), (1, 1, 1 << 16, 1 << 16)):
        assert lib.spk_completion_compose(*okc, *sizes, None) == -1, sizes


def test_ops_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from spkdiff import ops
    codes = torch.zeros(2, 7, 7, dtype=torch.int64)
    keep = torch.ones(2, 7, 7, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.completion_state(codes, keep, 128, 128)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.completion_compose(torch.zeros(2, 1, 28, 28), torch.ones(2, 28, 28, dtype=torch.bool),
                               torch.zeros(2, 1, 28, 28, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        ops.completion_state(codes, keep.float(), 128, 128)
    with pytest.raises(TypeError):
        ops.completion_state(codes, None, 128, 128)
    sig = inspect.signature(ops.completion_state).parameters
    assert list(sig)[:4] == ["codes", "keep", "K", "mask_id"] and sig["stride"].default == 1 and sig["radius"].default == 0


def _sampler(latent=(7, 7)):
    from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel
    return AbsorbingDiffusion(DummyModel(1, 128), mask_id=128, latent_shape=latent)


def test_sample_signature_keeps_the_existing_arguments_first():
    from snn_model.vq_diffusion import AbsorbingDiffusion
    sig = inspect.signature(AbsorbingDiffusion.sample).parameters
    assert list(sig) == ["self", "temp", "sample_steps", "noise", "record", "x_init", "known"]
    assert sig["temp"].default == 1.0
    for name in ("sample_steps", "noise", "record", "x_init", "known"):
        assert sig[name].default is None, name


def test_sample_checks_the_start_arguments_before_anything_else():
    """Both or neither, equal shapes, the sampler's shape, integer / bool types, device tensors -- raised before the key draw
    (the global generator is left where it was) and before the device is looked at (so: on a machine without a GPU too)."""
    ab = _sampler()
    ab.n_samples = 5
    x = torch.zeros(3, 1, 7, 7, dtype=torch.int64)
    k = torch.ones(3, 1, 7, 7, dtype=torch.bool)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="both or neither"):
        ab.sample(x_init=x)
    with pytest.raises(ValueError, match="both or neither"):
        ab.sample(known=k)
    with pytest.raises(ValueError, match="same shape"):
        ab.sample(x_init=x, known=k[:, 0])
    with pytest.raises(ValueError, match="same shape"):
        ab.sample(x_init=x, known=k[:2])
    with pytest.raises(ValueError, match="sampler's shape"):
        ab.sample(x_init=torch.zeros(3, 1, 8, 8, dtype=torch.int64), known=torch.ones(3, 1, 8, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match="sampler's shape"):
        ab.sample(x_init=torch.zeros(3, 2, 7, 7, dtype=torch.int64), known=torch.ones(3, 2, 7, 7, dtype=torch.bool))
    with pytest.raises(ValueError, match="sampler's shape"):
        ab.sample(x_init=torch.zeros(3, 49, dtype=torch.int64), known=torch.ones(3, 49, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="integer"):
        ab.sample(x_init=x.float(), known=k)
    with pytest.raises(NotImplementedError, match="bool or uint8"):
        ab.sample(x_init=x, known=k.long())
    with pytest.raises(TypeError):
        ab.sample(x_init=x.numpy(), known=k)
    for xi, kn in ((x, k), (x[:, 0], k[:, 0]), (x.int(), k.to(torch.uint8))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ab.sample(x_init=xi, known=kn)
    assert torch.equal(torch.get_rng_state(), state), "no key was drawn by a refused call"
    assert ab.n_samples == 5
    ab8 = _sampler((8, 8))
    with pytest.raises(ValueError, match="sampler's shape"):
        ab8.sample(x_init=x, known=k)


def test_complete_images_surface_and_argument_checks():
    from spkdiff import complete, dist
    sig = inspect.signature(complete.complete_images).parameters
    assert list(sig) == ["model", "sampler", "images", "keep", "temp", "sample_steps", "T", "paste"]
    assert (sig["temp"].default, sig["sample_steps"].default, sig["T"].default, sig["paste"].default) == (1.0, None, 16, True)
    assert complete.Completion._fields == ("images_u8", "tokens", "known", "n_known")
    assert (complete.ENC_STRIDE, complete.ENC_RADIUS) == (4, 3)
    sig = inspect.signature(dist.complete_images_sharded).parameters
    assert list(sig)[:4] == ["model", "sampler", "images", "keep"]
    ab = _sampler()
    img = torch.zeros(2, 1, 28, 28)
    with pytest.raises(ValueError, match="keep"):
        complete.complete_images(None, ab, img, torch.ones(2, 1, 14, 14, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        complete.complete_images(None, ab, img[0], torch.ones(1, 28, 28, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="bool or uint8"):
        complete.complete_images(None, ab, img, torch.ones(2, 28, 28))
    with pytest.raises(ValueError, match="multiples of 4"):
        complete.complete_images(None, ab, torch.zeros(2, 1, 30, 30), torch.ones(2, 30, 30, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        complete.complete_images(None, ab, img, torch.ones(2, 28, 28, dtype=torch.bool))


def test_oracle_state_rule_receptive_field():
    """The torch restatement the GPU test compares the kernel with, against the rule spelled out as loops; and the rule against
    the encoder itself: a code's value depends on exactly the pixels 4i-3 .. 4i+3 (Conv 3x3 s2 p1 twice, then 1x1)."""
    g = torch.Generator().manual_seed(7)
    for (B, H, h, stride, radius) in ((3, 28, 7, 4, 3), (2, 32, 8, 4, 3), (3, 7, 7, 1, 0)):
        codes = torch.randint(-3, 140, (B, h, h), generator=g)
        keep = torch.rand(B, H, H, generator=g) < 0.97
        x_t, un, n = corc.state_from_mask(codes, keep, 128, 128, stride, radius)
        for b in range(B):
            for i in range(h):
                for j in range(h):
                    win = keep[b, max(0, stride * i - radius):stride * i + radius + 1, max(0, stride * j - radius):stride * j + radius + 1]
                    want = bool(win.all()) and 0 <= int(codes[b, i, j]) < 128
                    assert bool(un[b, 0, i, j]) == want
                    assert int(x_t[b, 0, i, j]) == (int(codes[b, i, j]) if want else 128)
        assert torch.equal(n, un.flatten(1).sum(1).to(torch.int32))
    # the window is the encoder's receptive field: the gradient of a code's pre-quantisation feature reaches those pixels only
    import torch.nn.functional as F
    w1, w2, w3 = torch.rand(4, 1, 3, 3, generator=g) + 0.1, torch.rand(4, 4, 3, 3, generator=g) + 0.1, torch.rand(2, 4, 1, 1, generator=g) + 0.1
    x = torch.rand(1, 1, 28, 28, generator=g).requires_grad_(True)
    z = F.conv2d(F.conv2d(F.conv2d(x, w1, None, 2, 1), w2, None, 2, 1), w3)
    assert z.shape[-2:] == (7, 7)
    for (i, j) in ((0, 0), (3, 2), (6, 6)):
        gr, = torch.autograd.grad(z[0, :, i, j].sum(), x, retain_graph=True)
        nz = torch.nonzero(gr[0, 0])
        assert int(nz[:, 0].min()) == max(0, 4 * i - 3) and int(nz[:, 0].max()) == min(27, 4 * i + 3)
        assert int(nz[:, 1].min()) == max(0, 4 * j - 3) and int(nz[:, 1].max()) == min(27, 4 * j + 3)


def test_oracle_compose_rule():
    img = np.array([[[[-0.7, -0.5, -0.25, 0.0]], [[0.25, 0.4999, 0.5, 3.0]]]], dtype=np.float32).reshape(1, 2, 1, 4)
    dec = np.full((1, 2, 1, 4), 7, dtype=np.uint8)
    keep = np.array([[[1, 0, 1, 1]]], dtype=np.uint8)
    out = corc.compose(img, keep, dec)
    assert out.tolist() == [[[[0, 7, 63, 127]], [[191, 7, 255, 255]]]]


def test_host_oracle_keeps_known_tokens_and_leaves_no_mask():
    """The conditional loop on the host (2 images, 49 steps, noise from oracle/philox_ref.py): every known token is returned
    unchanged, nothing stays masked, and with nothing known the tokens are ref.absorbing_sample's on the same noise."""
    from oracle import snn_ref as ref
    from spkdiff import synth
    torch.set_num_threads(min(8, torch.get_num_threads()))
    sd = synth.synth_denoiser_state(synth.MNIST)
    B, steps, K = 2, 49, 128
    x_init, known = corc.issue_start(4)
    x_init, known = x_init[2:], known[2:]                      # a random half / only the centre
    x_init[0, 0, 0, 0], known[0, 0, 0, 0] = 200, True           # outside the codebook under a true mask: not known
    noise = corc.host_philox_noise(12345, steps, B, 7, K)
    x, un = corc.run(sd, x_init, known, steps, noise)
    kept = known & (x_init < K)
    assert bool(un.all()) and int((x == K).sum()) == 0 and int(x.max()) < K
    assert torch.equal(x[kept], x_init[kept])
    assert not bool(kept[0, 0, 0, 0])
    none = torch.zeros_like(known)
    x0, _ = corc.run(sd, x_init, none, 6, corc.host_philox_noise(12345, 6, B, 7, K))
    assert torch.equal(x0, ref.absorbing_sample(sd, B, K, 1.0, 6, 7, 16, noise=corc.host_philox_noise(12345, 6, B, 7, K)))
