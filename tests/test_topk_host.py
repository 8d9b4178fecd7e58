"""CPU tests of top-k truncated sampling: the host oracle against a plain sort, the numpy mirror of the kernel's
bit-wise select on rows with signed zeros, infinities, denormals, repeats and a NaN; the two ``_topk`` entry points declared,
exported, bound and refusing null arrays on the host; ``AbsorbingDiffusion.sample_top_k`` checking ``top_k`` before anything is
drawn or launched; and the launch sequence of every form, which is today's with the ``top_k`` tensor on every token update and on
nothing else (the recorders of tests/_dispatch_recorders.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _topk_oracle as tko
from _dispatch_recorders import B, _install_recorders
from test_sampler_dispatch import CASES, EXPECTED, STEPS, _sampler as dispatch_sampler      # (the helpers, not the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spk_psample_step_topk", "spk_den_step_tail_topk")
INF = float("inf")


# ------------------------------------------------------------------------------------------------- the oracle itself
def _sort_loop(z, k):
    """Per row: sort descending, take entry k - 1, drop what is below it."""
    out = z.clone()
    K = z.shape[-1]
    if k <= 0 or k >= K:
        return out
    for r in range(z.shape[0]):
        tau = sorted(z[r].tolist(), reverse=True)[k - 1]
        for c in range(K):
            if z[r, c].item() < tau:
                out[r, c] = -INF
    return out


@pytest.mark.parametrize("K", [1, 2, 5, 64, 130])
def test_truncate_is_the_sort_definition(K):
    g = torch.Generator().manual_seed(K)
    z = torch.randn(12, K, generator=g) * 3
    z[1::3] = torch.round(z[1::3] * 2) / 2                          # rows with ties
    z[2, K // 2] = -INF
    if K > 2:
        z[3, :2] = torch.tensor([0.0, -0.0])
    for k in sorted({-1, 0, 1, 2, K // 2, K - 1, K, K + 3}):
        got = tko.truncate(z, k)
        assert torch.equal(got, _sort_loop(z, k)), (K, k)
        assert torch.equal(z.masked_fill(~tko.kept(z, k), -INF), got), (K, k)
        if 0 < k < K:
            assert int((got > -INF).sum(1).min()) >= min(k, int((z > -INF).sum(1).min()))
    ks = torch.tensor([0, 1, 2, K, K + 1, 1, 0, 2, 1, 3, K - 1, 1])
    per_row = tko.truncate(z, ks)
    for r in range(12):
        assert torch.equal(per_row[r], tko.truncate(z[r:r + 1], int(ks[r]))[0])


def _special_rows(K, seed):
    """fp32 rows [N, K] holding +-0, +-inf, denormals, repeated values and (last row block) a NaN."""
    g = np.random.default_rng(seed)
    rows = []
    base = (g.standard_normal((6, K)) * 3).astype(np.float32)
    rows.append(base)
    rows.append(np.round(base * 2) / 2)                                                  # repeats
    pool = np.array([0.0, -0.0, INF, -INF, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0, 3.5, 3.5], dtype=np.float32)
    rows.append(pool[g.integers(0, len(pool), (8, K))])                                  # only special values
    mixed = base.copy()
    hit = g.random((6, K)) < 0.4
    mixed[hit] = pool[g.integers(0, len(pool), int(hit.sum()))]
    rows.append(mixed)
    rows.append(np.zeros((1, K), dtype=np.float32))                                      # all equal
    rows.append(np.full((1, K), -INF, dtype=np.float32))                                 # nothing above -inf
    nan = mixed.copy()
    nan[np.arange(6), g.integers(0, K, 6)] = np.nan
    rows.append(nan)
    return np.concatenate(rows).astype(np.float32)


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 257])
def test_bit_select_equals_the_sort(K):
    z = _special_rows(K, 100 + K)
    assert np.isnan(z).any() and (z == 0).any() and np.isinf(z).any()
    for k in sorted({1, 2, K - 1} - {0}):
        tau = tko.kth_largest_by_bits(z, k)
        for r in range(z.shape[0]):
            vals = sorted((float(v) for v in z[r] if not np.isnan(v)), reverse=True)
            if len(vals) < k:
                assert np.isnan(tau[r]), (K, k, r)                   # fewer than k entries that count: nothing is dropped
                assert not (z[r] < tau[r]).any()
                continue
            assert float(tau[r]) == vals[k - 1], (K, k, r, float(tau[r]), vals[k - 1])      # (-0.0 == +0.0)
            drop = z[r] < tau[r]
            assert not drop[np.isnan(z[r])].any()
            assert int((~drop & ~np.isnan(z[r])).sum()) >= k
            # on a NaN-free row the mask is the definition's
            if not np.isnan(z[r]).any() and k < K:
                want = tko.truncate(torch.from_numpy(z[r:r + 1]), k)[0].numpy()
                got = np.where(drop, np.float32(-INF), z[r])
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (K, k, r)
    # the keys order as the floats do
    flat = z[~np.isnan(z)]
    order = np.argsort(tko.order_key(flat), kind="stable")
    assert np.all(flat[order][1:] >= flat[order][:-1])


# ------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_declared_exported_and_bound():
    from spkdiff import _lib
    txt = open(os.path.join(ROOT, "include", "spkdiff.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/spkdiff.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libspkdiff.so"
        assert name in _lib.EXPORTS
        sib = getattr(_lib.lib, name[:-len("_topk")] + "_temps")
        fn = getattr(_lib.lib, name)
        # the `_temps` sibling's arguments with one more pointer right after temp_b, nothing else
        i = [a is ctypes.c_float for a in getattr(_lib.lib, name[:-len("_topk")]).argtypes].index(True)
        assert list(fn.argtypes) == list(sib.argtypes[:i + 1]) + [ctypes.c_void_p] + list(sib.argtypes[i + 1:])
        assert fn.restype is ctypes.c_int
    assert _lib.version() == _lib.EXPECTED_VERSION == 106           # additive: the ABI version stays
    m = re.search(r"#define\s+SPK_VERSION\s+(\d+)", txt)
    assert m and int(m.group(1)) == 106


def test_null_arrays_are_refused_before_any_launch():
    """SPK_ERR_ARG (-1) on the host for a NULL temp_b or topk_b; the other checks are the siblings' (no GPU is needed: the non-null
    pointers are host addresses and never dereferenced)."""
    from spkdiff import _lib
    lib = _lib.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    # logits, x_t, unmasked, t, temp_b, topk_b, u, q, seed, offset, state, x0_hat, B, HW, K, active, n_active, next_input, stream
    ps = lambda tb, kb, t=3, K=128, lg=p: lib.spk_psample_step_topk(lg, p, p, t, tb, kb, None, None, 1, 0, None, None, 2, 49, K,      # noqa: E731
                                                                    None, None, None, None)
    assert ps(None, p) == -1 and ps(p, None) == -1 and ps(None, None) == -1
    assert ps(p, p, lg=None) == -1 and ps(p, p, t=0) == -1
    assert ps(p, p, K=2049) == -2 and ps(p, p, K=4096) == -2
    tail = lambda tb, kb, H=7, K=128: lib.spk_den_step_tail_topk(p, 8, p, 2, p, p, p, None, p, p, 3, tb, kb, None, None, 1, 0, None,   # noqa: E731
                                                                 None, None, None, None, None, None, 16, 2, H, H, K, None, None, None)
    assert tail(None, p) == -1 and tail(p, None) == -1
    assert tail(p, p, H=9) == -2 and tail(p, p, K=513) == -2 and tail(p, p, K=0) == -2


# ------------------------------------------------------------------------------------------------- sample_top_k's argument
def _sampler():
    from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel
    return AbsorbingDiffusion(DummyModel(1, 128), mask_id=128)


def test_topk_arg_accepts_and_refuses():
    ab = _sampler()
    assert ab._topk_arg(None, 4) is None
    for k in (1, 8, 500, np.int64(8), np.int32(3), torch.tensor(8), np.array(8)):
        got = ab._topk_arg(k, 4)
        assert isinstance(got, int) and got == int(k)
    for v in ([1, 4, 0, 200], (1, 4, 0, 200), np.array([1, 4, 0, 200]), np.array([1, 4, 0, 200], dtype=np.int32),
              torch.tensor([1, 4, 0, 200]), torch.tensor([1, 4, 0, 200], dtype=torch.int32)):
        got = ab._topk_arg(v, 4)
        assert got.dtype == torch.int32 and got.device.type == "cpu" and got.tolist() == [1, 4, 0, 200]
    assert ab._topk_arg([3], 1).tolist() == [3]
    bad = ([1, 2, 3], [1] * 5, np.ones(3, dtype=np.int64), torch.ones(5, dtype=torch.int64), torch.ones(2, 2, dtype=torch.int64),   # length
           [1, -1, 2, 2], np.array([1, 2, 3, -4]), torch.tensor([-1, 1, 1, 1]), -1, 0, np.int64(0),                                   # negative
           [1.0, 2.0, 3.0, 4.0], 2.0, 2.5, np.float32(2.0), torch.tensor([1.0, 2.0, 3.0, 4.0]), np.ones(4),                           # not integers
           True, False, [True, False, True, True], np.array([True] * 4), torch.ones(4, dtype=torch.bool), "8", [1, 2, None, 4])      # bools, others
    for v in bad:
        with pytest.raises(ValueError, match="top_k"):
            ab._topk_arg(v, 4)


def test_sample_top_k_checks_top_k_before_anything_else():
    ab = _sampler()
    ab.n_samples = 4
    sig = inspect.signature(ab.sample_top_k).parameters
    assert list(sig) == ["top_k", "temp", "sample_steps", "noise", "record", "x_init", "known"]
    assert list(inspect.signature(ab.sample).parameters) == list(sig)[1:]
    assert "top_k" not in inspect.signature(ab.score).parameters
    with pytest.raises(TypeError):
        ab.score(torch.zeros(4, 1, 7, 7, dtype=torch.int64), top_k=3)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    for v in ([1, 2, 3], [1, -1, 2, 2], [1.0, 2.0, 3.0, 4.0], True, 0, 2.5):
        with pytest.raises(ValueError, match="top_k"):
            ab.sample_top_k(v, sample_steps=3)
        with pytest.raises(ValueError, match="top_k"):
            ab.sample_top_k(v, temp=[1.0, 0.5, 0.3, 0.2], sample_steps=3)
    with pytest.raises(ValueError, match="one entry per image"):      # the temperature's own check comes first, as in sample()
        ab.sample_top_k(3, temp=[1.0, 0.5], sample_steps=3)
    assert torch.equal(torch.get_rng_state(), state), "no key was drawn by a refused call"
    # a good top_k gets past the check: the next refusal is the device's
    for v in (None, 1, 8, [1, 4, 0, 200], np.array([1, 4, 0, 200]), torch.tensor([1, 4, 0, 200])):
        with pytest.raises(RuntimeError, match="ROCm device"):
            ab.sample_top_k(v, sample_steps=3)
    assert torch.equal(torch.get_rng_state(), state) and ab.n_samples == 4
    # the graph key: one marker for every top_k and every temperature; untruncated calls keep their keys
    form = ab._form(4, 7, 7)
    tv = torch.tensor([1.0, 0.5, 0.3, 0.2])
    k1 = ab._graph_key("cuda:0", 4, 7, 7, tv, 12, form, False, top_k=torch.tensor([1, 2, 3, 4], dtype=torch.int32))
    k2 = ab._graph_key("cuda:0", 4, 7, 7, tv * 2, 12, form, False, top_k=torch.tensor([8, 8, 0, 8], dtype=torch.int32))
    plain_v, plain_s = ab._graph_key("cuda:0", 4, 7, 7, tv, 12, form, False), ab._graph_key("cuda:0", 4, 7, 7, 0.5, 12, form, False)
    assert k1 == k2 and "top-k" in k1 and "per-image" in k1
    assert "top-k" not in plain_v and "top-k" not in plain_s and len({k1, plain_v, plain_s}) == 3
    assert plain_v == ab._graph_key("cuda:0", 4, 7, 7, tv, 12, form, False, top_k=None)
    ab.set_shard(8)
    assert ab._graph_key("cuda:0", 4, 7, 7, tv, 12, form, False, top_k=torch.zeros(4, dtype=torch.int32)) == k1


def test_ops_wrappers_take_top_k_only_as_an_int32_device_tensor():
    from spkdiff import ops
    assert ops._topk_arg(None, 0.9, 5, "x", "cpu") == (None, 0.9)
    for bad in (torch.ones(5, dtype=torch.int32), [1, 2, 3, 4, 5], 3):      # a host tensor, a list, an int
        with pytest.raises(ValueError, match="int32 device tensor"):
            ops._topk_arg(bad, 1.0, 5, "psample_step", "cpu")
    for name in ("psample_step", "den_step_tail"):
        assert inspect.signature(getattr(ops, name)).parameters["top_k"].default is None
    assert "top_k" not in inspect.signature(ops.pscore_step).parameters


def test_sweep_and_completion_surfaces():
    from spkdiff import complete, dist, evaluate
    assert list(inspect.signature(evaluate.temperature_sweep_top_k).parameters) == [
        "model", "sampler", "temps", "n_per_temp", "top_k", "sample_steps", "batch", "T"]
    assert inspect.signature(evaluate.temperature_sweep_range).parameters["top_k"].default is None
    assert inspect.signature(dist.temperature_sweep_sharded).parameters["top_k"].default is None
    assert inspect.signature(dist.complete_images_sharded).parameters["top_k"].default is None
    assert list(inspect.signature(complete.complete_images_top_k).parameters)[:6] == ["model", "sampler", "images", "keep", "top_k", "temp"]
    assert evaluate._sweep_top_k(None, 3, 5) is None
    assert evaluate._sweep_top_k(8, 3, 2).tolist() == [8] * 6 and evaluate._sweep_top_k(0, 2, 2).tolist() == [0] * 4
    kv = evaluate._sweep_top_k([1, 0, 16], 3, 2)
    assert kv.dtype == torch.int32 and kv.tolist() == [1, 1, 0, 0, 16, 16]
    for bad in ([1, 2], [1, 2, 3, 4], [1, -2, 3], [1.0, 2.0, 3.0], 2.5, True, -1):
        with pytest.raises(ValueError, match="top_k"):
            evaluate._sweep_top_k(bad, 3, 2)


class _StubSampler:
    """What temperature_sweep touches of an AbsorbingDiffusion; records which method every call took and what it was given."""
    noise_source = 'philox'

    def __init__(self):
        import contextlib
        self.n_samples, self.global_first, self.shape, self.calls = 16, 7, [2, 2], []
        self._one_key = contextlib.nullcontext

    def set_shard(self, first, count=None):
        self.global_first, self.n_samples = int(first), self.n_samples if count is None else int(count)
        return self

    def _tokens(self):
        idx = torch.arange(self.global_first, self.global_first + self.n_samples)
        return idx.reshape(-1, 1, 1, 1).expand(-1, 1, 2, 2).contiguous()

    def sample(self, temp=1.0, sample_steps=None):
        self.calls.append(("sample", self.global_first, None))
        return self._tokens()

    def sample_top_k(self, top_k, temp=1.0, sample_steps=None):
        assert len(top_k) == len(temp) == self.n_samples and top_k.dtype == torch.int32
        self.calls.append(("sample_top_k", self.global_first, top_k.tolist()))
        return self._tokens()


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def decode_tokens(self, tokens, T=16, want_u8=True):
        return None, tokens.to(torch.uint8).reshape(-1, 1, 2, 2)


def test_sweep_slices_top_k_with_the_temperatures():
    from spkdiff import evaluate
    temps, n, ks = [0.3, 1.0, 0.65], 5, [1, 0, 16]
    per_image = [1] * 5 + [0] * 5 + [16] * 5
    sm = _StubSampler()
    u8, tok = evaluate.temperature_sweep_top_k(_StubModel(), sm, temps, n, ks, batch=4)
    assert [(c[0], c[1]) for c in sm.calls] == [("sample_top_k", f) for f in (0, 4, 8, 12)]
    assert [c[2] for c in sm.calls] == [per_image[f:f + 4] for f in (0, 4, 8, 12)]
    assert tok.shape == (3, 5, 2, 2) and (sm.n_samples, sm.global_first) == (16, 7)
    # without top_k the sweep calls sample() with today's arguments
    sm2 = _StubSampler()
    evaluate.temperature_sweep(_StubModel(), sm2, temps, n, batch=4)
    evaluate.temperature_sweep_top_k(_StubModel(), sm2, temps, n, None, batch=4)
    assert [c[0] for c in sm2.calls] == ["sample"] * 8


# ------------------------------------------------------------------------------------------------- the launch sequence
def _watch_top_k(monkeypatch):
    """On top of the installed recorders: note every wrapper call that carries a ``top_k`` keyword."""
    from spkdiff import ops
    seen = []
    for name in ("psample_step", "den_step_tail", "pscore_step", "select_active", "select_needed", "den_build_input", "completion_state"):
        inner = getattr(ops, name)

        def shim(*a, _inner=inner, _name=name, **kw):
            if "top_k" in kw:
                seen.append((_name, kw["top_k"]))
            return _inner(*a, **kw)
        monkeypatch.setattr(ops, name, shim)
    return seen


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("given", [False, True], ids=["none", "top_k"])
def test_launch_sequence_with_and_without_top_k(monkeypatch, name, given):
    """Every case of tests/test_sampler_dispatch.py driven through the same entries with ``top_k`` None and with a tensor: the
    recorded launches are EXPECTED's either way; with None no call carries the keyword, with a tensor every token-update call
    (psample_step / den_step_tail) carries that very tensor and nothing else does."""
    from snn_model.vq_diffusion import _SamplerGraph
    case = CASES[name]
    hw = case.get('hw', 7)
    ab = dispatch_sampler(case, hw)
    cpu = torch.device('cpu')
    start = (torch.zeros((B, hw, hw), dtype=torch.int64), torch.zeros((B, hw, hw), dtype=torch.uint8)) if case.get('known') else None
    record = [] if case.get('record') else None
    noise = (lambda t: (torch.zeros(B, 1, hw, hw), torch.zeros(B * hw * hw, 128))) if case.get('inject') else None
    log = _install_recorders(monkeypatch, sampler=True)
    seen = _watch_top_k(monkeypatch)
    form = ab._form(B, hw, hw, record is not None)
    tk = torch.tensor([3, 0], dtype=torch.int32) if given else None
    with torch.no_grad():
        if name.startswith('graph'):
            g = _SamplerGraph(cpu, B, hw, hw, form, int(ab.list_radii), start is not None, top_k=given)
            assert (g.topk is not None) == given and (g.temps is not None) == given
            tk = g.topk
            ab._graph_body(g, form, 1.0, STEPS)
        else:
            seed = 5 if noise is None and ab.noise_source == 'philox' else 0
            ab._sample_eager(cpu, B, hw, hw, form, 1.0, STEPS, noise, seed, start, record, top_k=tk)
    launches = [c for c in log if not c.startswith(('bn_prepare', 'pack_', 'den_pack_'))]
    assert (ab.form_for(B, hw, hw), launches) == EXPECTED[name]
    updates = [c.split('(')[0] for c in launches if c.startswith(('psample_step', 'den_step_tail'))]
    assert len(updates) == STEPS
    if given:
        assert [s[0] for s in seen] == updates and all(s[1] is tk for s in seen)
    else:
        assert seen == []
