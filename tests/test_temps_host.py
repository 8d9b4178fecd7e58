"""CPU tests of the per-image sampling temperature: the three ``_temps`` entry points are declared, exported and
bound and refuse a null temperature array on the host; ``AbsorbingDiffusion.sample`` / ``.score`` check a host vector before
anything is drawn or launched; ``spkdiff.evaluate.temperature_sweep`` maps the job's image indices to temperatures and shards the
job as specified (a stub sampler records what every call was given)."""
import contextlib
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spk_psample_step_temps", "spk_pscore_step_temps", "spk_den_step_tail_temps")


def test_entry_points_declared_exported_and_bound():
    from spkdiff import _lib
    txt = open(os.path.join(ROOT, "include", "spkdiff.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/spkdiff.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libspkdiff.so"
        assert name in _lib.EXPORTS
        sib = getattr(_lib.lib, name[:-len("_temps")])
        fn = getattr(_lib.lib, name)
        # the sibling's arguments with `float temp` replaced by a pointer, nothing else
        diff = [i for i, (a, b) in enumerate(zip(sib.argtypes, fn.argtypes)) if a is not b]
        assert len(sib.argtypes) == len(fn.argtypes) and len(diff) == 1
        assert sib.argtypes[diff[0]] is ctypes.c_float and fn.argtypes[diff[0]] is ctypes.c_void_p
        assert fn.restype is ctypes.c_int
    assert _lib.version() == _lib.EXPECTED_VERSION == 106           # additive: the ABI version stays
    m = re.search(r"#define\s+SPK_VERSION\s+(\d+)", txt)
    assert m and int(m.group(1)) == 106


def test_null_temperature_array_is_refused_before_any_launch():
    """SPK_ERR_ARG (-1) on the host, as for the other pointers -- no GPU is needed (the non-null pointers are host addresses and
    never dereferenced)."""
    from spkdiff import _lib
    lib = _lib.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    # logits, x_t, unmasked, t, temp_b, u, q, seed, offset, state, x0_hat, B, HW, K, active, n_active, next_input, stream
    assert lib.spk_psample_step_temps(p, p, p, 3, None, None, None, 1, 0, None, None, 2, 49, 128, None, None, None, None) == -1
    assert lib.spk_psample_step_temps(None, p, p, 3, p, None, None, 1, 0, None, None, 2, 49, 128, None, None, None, None) == -1
    assert lib.spk_psample_step_temps(p, p, p, 0, p, None, None, 1, 0, None, None, 2, 49, 128, None, None, None, None) == -1
    assert lib.spk_psample_step_temps(p, p, p, 3, p, None, None, 1, 0, None, None, 2, 49, 4096, None, None, None, None) == -2
    # logits, x0, x_t, unmasked, t, temp_b, u, seed, offset, state, logp, step, B, HW, K, active, n_active, next_input, stream
    assert lib.spk_pscore_step_temps(p, p, p, p, 3, None, None, 1, 0, None, p, None, 2, 49, 128, None, None, None, None) == -1
    assert lib.spk_pscore_step_temps(p, p, p, p, 3, p, None, 1, 0, None, None, None, 2, 49, 128, None, None, None, None) == -1
    assert lib.spk_pscore_step_temps(p, p, p, p, 3, p, None, 1, 0, None, p, None, 2, 49, 513, None, None, None, None) == -2
    # cnt5, 8, cnt1, 2, wq, scale, bias, logits, x_t, unmasked, t, temp_b, u, q, seed, offset, state, w1, b1, a1, bb1, x1, c1, T, B, H, W,
    # K, active, n_active, stream
    tail = lambda temp, H=7: lib.spk_den_step_tail_temps(p, 8, p, 2, p, p, p, None, p, p, 3, temp, None, None, 1, 0, None,      # noqa: E731
                                                         None, None, None, None, None, None, 16, 2, H, H, 128, None, None, None)
    assert tail(None) == -1
    assert tail(p, H=9) == -2
    # the scalar siblings keep their own check of the value
    assert lib.spk_psample_step(p, p, p, 3, 0.0, None, None, 1, 0, None, None, 2, 49, 128, None, None, None, None) == -1
    assert lib.spk_pscore_step(p, p, p, p, 3, -1.0, None, 1, 0, None, p, None, 2, 49, 128, None, None, None, None) == -1


def _sampler():
    from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel
    return AbsorbingDiffusion(DummyModel(1, 128), mask_id=128)


def test_sample_and_score_check_a_host_vector_before_anything_else():
    ab = _sampler()
    ab.n_samples = 4
    x0 = torch.zeros(4, 1, 7, 7, dtype=torch.int64)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    bad_len = ([1.0, 0.5, 0.3], [1.0] * 5, np.ones(3, dtype=np.float32), torch.ones(5), torch.ones(2, 2), (0.5, 0.5))
    bad_val = ([1.0, 0.0, 0.5, 0.5], [1.0, -0.5, 0.5, 0.5], [1.0, float("inf"), 0.5, 0.5], [1.0, float("nan"), 0.5, 0.5],
               np.array([0.5, 0.5, 0.5, 0.0]), torch.tensor([0.5, float("nan"), 1.0, 1.0]), torch.tensor([-1.0, 1.0, 1.0, 1.0]))
    for t in bad_len:
        with pytest.raises(ValueError, match="one entry per image"):
            ab.sample(temp=t, sample_steps=3)
        with pytest.raises(ValueError, match="one entry per image"):
            ab.score(x0, temp=t, sample_steps=3)
    for t in bad_val:
        with pytest.raises(ValueError, match="finite and > 0"):
            ab.sample(temp=t, sample_steps=3)
        with pytest.raises(ValueError, match="finite and > 0"):
            ab.score(x0, temp=t, sample_steps=3)
    assert torch.equal(torch.get_rng_state(), state), "no key was drawn by a refused call"
    assert ab.n_samples == 4
    # a good vector and every scalar form get past the temperature check: the next refusal is the device's
    for t in ([1.0, 0.5, 0.3, 0.001], np.full(4, 0.5), torch.full((4,), 0.7), 0.5, 1, np.float32(0.5), torch.tensor(0.5),
              torch.tensor([0.5])):
        with pytest.raises(RuntimeError, match="ROCm device"):
            ab.sample(temp=t, sample_steps=3)
    v = ab._temp_arg([1.0, 0.5, 0.3, 0.001], 4)
    assert v.dtype == torch.float32 and v.tolist() == torch.tensor([1.0, 0.5, 0.3, 0.001]).tolist()
    assert ab._temp_arg(torch.tensor([0.25]), 4) == 0.25 and ab._temp_arg(0.9, 4) == 0.9
    # the graph key: a marker in place of the value for a vector, the value for a scalar
    form = ab._form(4, 7, 7)
    k1 = ab._graph_key("cuda:0", 4, 7, 7, torch.tensor([1.0, 0.5, 0.3, 0.2]), 12, form, False)
    k2 = ab._graph_key("cuda:0", 4, 7, 7, torch.tensor([0.1, 0.1, 0.1, 0.1]), 12, form, False)
    k3, k4 = (ab._graph_key("cuda:0", 4, 7, 7, t, 12, form, False) for t in (0.1, 0.2))
    assert k1 == k2 and "per-image" in k1 and k3 != k4 and k3 != k1 and 0.1 in k3
    # ... and for the shard: a sweep's calls share the vector graph, scalar calls keep the shard in the key
    ab.set_shard(8)
    assert ab._graph_key("cuda:0", 4, 7, 7, torch.tensor([1.0, 0.5, 0.3, 0.2]), 12, form, False) == k1
    assert ab._graph_key("cuda:0", 4, 7, 7, 0.1, 12, form, False) != k3


def test_ops_wrappers_take_the_vector_only_as_a_device_tensor():
    from spkdiff import ops
    t, x = ops._temp_arg(0.9, 5, "x")
    assert t is None and x == 0.9
    assert ops._temp_arg(torch.tensor(0.5), 5, "x") == (None, 0.5) and ops._temp_arg(torch.tensor([0.5]), 5, "x") == (None, 0.5)
    with pytest.raises(ValueError, match="fp32 device tensor"):
        ops._temp_arg(torch.ones(5), 5, "psample_step")             # a host tensor
    for name in ("psample_step", "pscore_step", "den_step_tail"):
        assert "temp" in inspect.signature(getattr(ops, name)).parameters


class _StubSampler:
    """What temperature_sweep touches of an AbsorbingDiffusion; records (global_first, n_samples, temps, key) per call."""
    noise_source = 'philox'

    def __init__(self):
        self.n_samples, self.global_first, self.shape = 16, 7, [2, 2]
        self.calls, self.keys_drawn, self._pinned_key = [], 0, None

    def set_shard(self, first, count=None):
        self.global_first = int(first)
        if count is not None:
            self.n_samples = int(count)
        return self

    @contextlib.contextmanager
    def _one_key(self):
        self.keys_drawn += 1
        self._pinned_key = 1000 + self.keys_drawn
        try:
            yield self._pinned_key
        finally:
            self._pinned_key = None

    def sample(self, temp=1.0, sample_steps=None):
        self.calls.append((self.global_first, self.n_samples, [round(float(v), 6) for v in temp], self._pinned_key, sample_steps))
        # token = the image's global index everywhere
        idx = torch.arange(self.global_first, self.global_first + self.n_samples)
        return idx.reshape(-1, 1, 1, 1).expand(-1, 1, 2, 2).contiguous()


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def decode_tokens(self, tokens, T=16, want_u8=True):
        assert want_u8
        u8 = tokens.to(torch.uint8).reshape(-1, 1, 2, 2).repeat(1, 1, 2, 2)
        return None, u8


def test_temperature_sweep_maps_indices_to_temperatures_and_shards_the_job():
    from spkdiff import evaluate, dist
    sig = inspect.signature(evaluate.temperature_sweep).parameters
    assert list(sig) == ["model", "sampler", "temps", "n_per_temp", "sample_steps", "batch", "T"]
    assert (sig["sample_steps"].default, sig["batch"].default, sig["T"].default) == (None, 256, 16)
    assert list(inspect.signature(dist.temperature_sweep_sharded).parameters)[:4] == ["model", "sampler", "temps", "n_per_temp"]
    temps, n = [0.3, 1.0, 0.65], 5
    per_image = [0.3] * 5 + [1.0] * 5 + [0.65] * 5
    sm, md = _StubSampler(), _StubModel()
    u8, tok = evaluate.temperature_sweep(md, sm, temps, n, sample_steps=12, batch=4)
    assert u8.shape == (3, 5, 1, 4, 4) and u8.dtype == torch.uint8 and tok.shape == (3, 5, 2, 2) and tok.dtype == torch.int64
    # chunks of four straddle the group boundaries at 5 and 10
    assert [(c[0], c[1]) for c in sm.calls] == [(0, 4), (4, 4), (8, 4), (12, 3)]
    for first, count, tv, key, steps in sm.calls:
        assert tv == [round(v, 6) for v in per_image[first:first + count]] and steps == 12
    assert sm.keys_drawn == 1 and {c[3] for c in sm.calls} == {1001}, "all calls of one sweep use one key"
    assert (sm.n_samples, sm.global_first) == (16, 7), "the sampler's shard is restored"
    # image (g, j) of the result is image g * n + j of the job
    assert torch.equal(tok[:, :, 0, 0], torch.arange(15).reshape(3, 5)) and torch.equal(u8[:, :, 0, 0, 0], torch.arange(15).reshape(3, 5).to(torch.uint8))
    # one call
    sm2 = _StubSampler()
    u8b, tokb = evaluate.temperature_sweep(md, sm2, temps, n, batch=None)
    assert [(c[0], c[1]) for c in sm2.calls] == [(0, 15)] and sm2.calls[0][2] == [round(v, 6) for v in per_image]
    assert torch.equal(u8b, u8) and torch.equal(tokb, tok)
    # a rank's range of the job
    sm3 = _StubSampler()
    lo, hi = dist.shard_range(15, 1, 2)
    u8c, tokc = evaluate.temperature_sweep_range(md, sm3, temps, n, lo, hi, batch=4)
    assert (lo, hi) == (8, 15) and [(c[0], c[1]) for c in sm3.calls] == [(8, 4), (12, 3)]
    assert torch.equal(tokc, tok.reshape(15, 2, 2)[lo:hi]) and (sm3.n_samples, sm3.global_first) == (16, 7)
    # (no process group: the sharded form is the whole job on this rank)
    sm4 = _StubSampler()
    assert torch.equal(dist.temperature_sweep_sharded(md, sm4, temps, n, batch=4), u8) and (sm4.n_samples, sm4.global_first) == (16, 7)
    for bad in ([], [0.5, 0.0], [0.5, float("nan")], [-1.0]):
        with pytest.raises(ValueError):
            evaluate.temperature_sweep(md, _StubSampler(), bad, n)
    with pytest.raises(ValueError):
        evaluate.temperature_sweep(md, _StubSampler(), temps, 0)
    with pytest.raises(ValueError):
        evaluate.temperature_sweep_range(md, _StubSampler(), temps, n, 8, 16)
    host = _StubSampler()
    host.noise_source = 'host'
    with pytest.raises(ValueError, match="philox"):
        evaluate.temperature_sweep(md, host, temps, n)


def test_the_pinned_key_is_one_ordinary_draw():
    """``_one_key``: one draw from torch's CPU generator -- the key sample() would have drawn -- and no draw by the calls inside."""
    ab = _sampler()
    torch.manual_seed(77)
    want = ab._philox_key()
    second = ab._philox_key()
    torch.manual_seed(77)
    with ab._one_key() as key:
        assert key == want and ab._philox_key() == want and ab._philox_key() == want
        with pytest.raises(RuntimeError):
            with ab._one_key():
                pass
    assert ab._pinned_key is None and ab._philox_key() == second and second != want


def test_token_nll_eval_and_complete_images_keep_their_signatures():
    from spkdiff import evaluate, complete
    sig = inspect.signature(evaluate.token_nll_eval).parameters
    assert list(sig) == ["model", "sampler", "batches", "temp", "sample_steps", "orders", "T", "temps"] and sig["temps"].default is None
    assert list(inspect.signature(complete.complete_images).parameters)[:5] == ["model", "sampler", "images", "keep", "temp"]
