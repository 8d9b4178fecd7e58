"""CPU tests of nucleus (top-p) truncated sampling: the numpy mirror of the kernel's integer bit descent against
the definition as a sort loop, on rows with signed zeros, infinities, denormals, repeats and a NaN, with and without a preceding
top-k and under a permutation of the classes; the fragility rule and the 10 % cap on the seeded case table of
tests/test_gpu_topp.py; the end-to-end case's seed; the two ``_topp`` entry points declared, exported, bound and refusing null
arrays on the host; ``AbsorbingDiffusion.sample_top_p`` checking ``top_p`` before anything is drawn or launched; and the launch
sequence of every form, which is today's with the ``top_p`` tensor on every token update and on nothing else."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _completion_oracle as corc
import _topk_oracle as tko
import _topp_oracle as tpo
from _dispatch_recorders import B, _install_recorders
from test_sampler_dispatch import CASES, EXPECTED, STEPS, _sampler as dispatch_sampler      # (the helpers, not the tests)
from test_topk_host import _special_rows                                                     # (the helper, not the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spk_psample_step_topp", "spk_den_step_tail_topp")
INF = float("inf")
PS = (1e-6, 0.25, 0.5, 0.9, 0.999)
REG_THRESHOLD = 8 * 9.4e-7               # the race oracle's fragile rule (tests/test_gpu_sampler_noise_shapes.py; that module needs a GPU)
ORACLE_SEED = 3143                       # see test_end_to_end_case_has_no_fragile_cut_and_no_fragile_draw
ORACLE_PS = (0.05, 0.5, 0.9, 1.0)


# ------------------------------------------------------------------------------------------------- the oracle itself
def _rows(K, seed):
    z = _special_rows(K, seed)
    g = np.random.default_rng(seed + 1)
    big = z[:6].copy()
    big[np.arange(6), g.integers(0, K, 6)] = INF                                        # mx = +inf: the row is not truncated
    return np.concatenate([z, big]).astype(np.float32)


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 257])
def test_bit_descent_equals_the_sort_definition(K):
    z = _rows(K, 300 + K)
    assert np.isnan(z).any() and (z == 0).any() and np.isinf(z).any() and (z == INF).any()
    assert (z == -INF).all(1).any(), "a row of -inf only"
    N = z.shape[0]
    g = np.random.default_rng(K)
    perm = g.permutation(K)
    for k in sorted({0, 2, K - 1}):
        k_rows = torch.full((N,), k)
        # (tko.truncate is defined on NaN-free rows: the rows with a NaN take no top-k here)
        has_nan = np.isnan(z).any(1)
        k_rows[torch.from_numpy(has_nan)] = 0
        zk = tko.truncate(torch.from_numpy(z), k_rows).numpy()
        m, mx = tpo.masses(zk)
        assert m.dtype == np.uint32 and int(m.max()) == 1 << 20
        assert (m[np.isnan(zk)] == 0).all() and (m[zk == -INF] == 0).all()
        fin = np.isfinite(mx)
        assert ((zk == mx[:, None]) & fin[:, None] <= (m == 1 << 20)).all(), "a row maximum weighs 2^20"
        for p in PS + (1.0, 0.0, -0.5, float("nan"), 1.5):
            p_rows = np.full(N, p, dtype=np.float32)
            tau = tpo.nucleus_by_bits(zk, m, p_rows)
            on = tpo.truncated_rows(p_rows, mx)
            if not (0 < p < 1):
                assert not on.any() and (tau == -INF).all()
            with np.errstate(invalid="ignore"):
                keep = ~(zk < tau[:, None])
            for r in range(N):
                want = tpo.nucleus_by_sort(zk[r], m[r], p)
                assert np.array_equal(keep[r], want), (K, k, p, r)
                if on[r]:
                    assert keep[r][zk[r] == mx[r]].all(), "the row maximum always stays"
                    assert keep[r][np.isnan(zk[r])].all(), "a NaN is never replaced"
                    if p == 1e-6:
                        assert np.array_equal(keep[r] & ~np.isnan(zk[r]), zk[r] == mx[r]), "p -> 0+: only the maxima"
                    # the smallest set of top classes, closed under ties, that reaches p of the total
                    P = float(np.float64(np.float32(p)) * np.float64(int(m[r].sum())))
                    cnt = ~np.isnan(zk[r])
                    assert float(int(m[r][keep[r] & cnt].sum())) >= P
                    tv = zk[r][keep[r] & cnt].min()
                    with np.errstate(invalid="ignore"):
                        above = cnt & (zk[r] > tv)
                    # (+0.0 and -0.0 are one value for the keep test and two keys for the sums: the mass above tau's KEY is short of P)
                    if tv != 0 and above.any():
                        assert float(int(m[r][above].sum())) < P, (K, k, p, r)
                else:
                    assert keep[r].all()
            # a permutation of the classes permutes the kept set: the integer sums do not depend on their order
            tau_p = tpo.nucleus_by_bits(zk[:, perm], m[:, perm], p_rows)
            assert np.array_equal(tau_p.view(np.uint32), tau.view(np.uint32)), (K, k, p)


def test_mirror_sums_in_uint32_and_compares_in_fp64():
    """K = 2048 classes that all tie: total = 2^31, which a signed or fp32 sum would not hold; every class stays for every p."""
    z = np.zeros((2, 2048), dtype=np.float32)
    z[1, 5] = -1.0
    m, mx = tpo.masses(z)
    assert int(m[0].sum(dtype=np.uint64)) == 1 << 31 and m.sum(1, dtype=np.uint32)[0] == np.uint32(1 << 31)
    for p in PS:
        tau = tpo.nucleus_by_bits(z, m, np.full(2, p, dtype=np.float32))
        assert tau[0] == 0.0 and tau[1] == 0.0                       # the 2047 tied classes reach p = 0.999 of the total on their own
    # the compare is S >= p * total in fp64: neighbouring fp32 values of p on either side of 2/3 decide it either way
    z = np.array([[0.0, np.log(np.float32(0.5)), -30.0]], dtype=np.float32)
    m, _ = tpo.masses(z)
    assert m.tolist() == [[1 << 20, 1 << 19, 0]]
    p_lo, p_hi = np.nextafter(np.float32(2 / 3), np.float32(0)), np.float32(2 / 3)
    assert float(np.float64(p_lo) * (3 << 19)) < float(1 << 20) < float(np.float64(p_hi) * (3 << 19))
    assert tpo.nucleus_by_bits(z, m, np.array([p_lo]))[0] == 0.0
    assert tpo.nucleus_by_bits(z, m, np.array([p_hi]))[0] == z[0, 1]


# ------------------------------------------------------------------------------------------------- the fragility rule
def test_fragile_rule_flags_what_an_expf_off_by_two_ulp_could_move():
    """Masses from an expf pushed one ulp off the correctly rounded value, up or down (at most 1.5 ulp off the true value: inside
    the rule's EXPF_ULP = 2), lie within the rule's per-class allowance of the fp64 mass, and a row the rule clears keeps its kept
    set under them."""
    g = np.random.default_rng(9)
    z = (g.standard_normal((400, 65)) * 4).astype(np.float32)
    p_rows = np.asarray([tpo.P_CYCLE[1:][i % 5] for i in range(400)], dtype=np.float32)
    frag, E = tpo.fragile_cut(z, p_rows)
    m, mx = tpo.masses(z)
    d = (z - mx[:, None]).astype(np.float32)
    w = np.exp(d.astype(np.float64)).astype(np.float32)
    base = ~(z < tpo.nucleus_by_bits(z, m, p_rows)[:, None])
    moved = 0
    for sign in (-1, 1):
        w2 = w.copy()
        w2 = np.nextafter(w2, np.float32(2 if sign > 0 else -1))
        m2 = np.rint((w2 * np.float32(tpo.SCALE)).astype(np.float32)).astype(np.uint32)
        mt = tpo.SCALE * np.exp(d.astype(np.float64))
        assert (np.abs(m2.astype(np.float64) - mt) <= tpo.class_allowance(mt) + 1e-9).all()
        keep2 = ~(z < tpo.nucleus_by_bits(z, m2, p_rows)[:, None])
        diff = (keep2 != base).any(1)
        moved += int(diff.sum())
        assert not (diff & ~frag).any(), "a row the rule clears kept another set"
    assert 0 < int(frag.sum()) < 400 * tpo.FRAGILE_SHARE_CAP
    assert (E > 0).all()


@pytest.mark.parametrize("K", tpo.KS)
def test_case_table_stays_under_the_fragile_cap(K):
    """The seeded case table of tests/test_gpu_topp.py on the oracle alone: at every temperature the GPU test calls with, at most
    FRAGILE_SHARE_CAP of the nucleus-truncated rows of a case have a fragile cut (a condition on the table, checked without a
    GPU); the table holds the rows the GPU test needs."""
    TEMPS, rows_of = tpo.TEMPS, tpo.rows_of
    for kind in tpo.KINDS:
        logits, q, u, x0, un0, ps, ks = tpo.topp_inputs(K, kind)
        Bn = logits.shape[0]
        assert Bn == (11 if K == 2048 else 21) and ps.tolist()[:6] == [np.float32(p) for p in tpo.P_CYCLE]
        assert ks.tolist()[:5] == [0, 0, 5, K // 2, K - 1]
        k_rows, p_rows = ks.long().repeat_interleave(49), ps.repeat_interleave(49).numpy()
        rows = rows_of(logits)
        assert bool(torch.isnan(rows[5 * 49]).any()) and bool((rows[5 * 49 + 1] == -INF).all()) and float(ps[5]) < 1
        for temp in TEMPS:
            _, _, keep, fcut, on = tpo.oracle_tokens(rows / temp, k_rows, p_rows, q, REG_THRESHOLD)
            share = float(fcut.sum()) / float(on.sum())
            assert int(on.sum()) >= 0.7 * rows.shape[0]
            assert share <= tpo.FRAGILE_SHARE_CAP, (K, kind, temp, share)
            if kind == "ties" and K > 2:
                n_tau = ((rows / temp) == (rows / temp).masked_fill(~keep, INF).min(-1, keepdim=True).values).sum(-1)
                assert int((n_tau[on] > 1).sum()) > 0, "the case needs rows that tie at tau"


def test_end_to_end_case_has_no_fragile_cut_and_no_fragile_draw():
    """The end-to-end case of tests/test_gpu_topp.py (B = 4, 12 steps, p = ORACLE_PS, the key drawn after
    torch.manual_seed(ORACLE_SEED)): over the whole host trajectory of every image no drawn position has a fragile cut, and the two
    largest fp64 ratios of every drawn position are further apart than the race oracle's threshold -- equality with the device is a
    fair demand.  (ORACLE_SEED was picked on the host among 3141 .. 3143 as the seed with the widest smallest margin.)"""
    from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel
    from spkdiff import synth
    sd = synth.synth_denoiser_state(synth.MNIST)
    torch.manual_seed(ORACLE_SEED)
    key = AbsorbingDiffusion(DummyModel(1, 128), mask_id=128)._philox_key()
    for i, p in enumerate(ORACLE_PS):
        margins, cuts = [], []
        tok = tpo.run(sd, 1, 12, corc.host_philox_noise(key, 12, 1, 7, 128, first=i), p, margins=margins, cuts=cuts)
        assert sum(cuts) == 0, (i, p, cuts)
        assert min(float(m.min()) for m in margins if m.numel()) > REG_THRESHOLD
        assert int(tok.max()) < 128 and int(tok.min()) >= 0


# ------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_declared_exported_and_bound():
    from spkdiff import _lib
    txt = open(os.path.join(ROOT, "include", "spkdiff.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, f"{name} is not declared in include/spkdiff.h"
        args = [a.strip() for a in m.group(1).split(",")]
        i = args.index("const int* topk_b")
        assert args[i + 1] == "const float* topp_b" and args[i - 1] == "const float* temp_b"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libspkdiff.so"
        assert name in _lib.EXPORTS
        sib = getattr(_lib.lib, name[:-len("_topp")] + "_topk")
        fn = getattr(_lib.lib, name)
        # the `_topk` sibling's arguments with one more pointer right after topk_b, nothing else
        j = [a is ctypes.c_float for a in getattr(_lib.lib, name[:-len("_topp")]).argtypes].index(True) + 1
        assert list(fn.argtypes) == list(sib.argtypes[:j + 1]) + [ctypes.c_void_p] + list(sib.argtypes[j + 1:])
        assert fn.restype is ctypes.c_int
    assert _lib.version() == _lib.EXPECTED_VERSION == 106           # additive: the ABI version stays
    m = re.search(r"#define\s+SPK_VERSION\s+(\d+)", txt)
    assert m and int(m.group(1)) == 106


def test_null_arrays_are_refused_before_any_launch():
    """SPK_ERR_ARG (-1) on the host for a NULL temp_b, topk_b or topp_b; the other checks are the siblings' (no GPU is needed: the
    non-null pointers are host addresses and never dereferenced)."""
    from spkdiff import _lib
    lib = _lib.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ps = lambda tb, kb, pb, t=3, K=128, lg=p: lib.spk_psample_step_topp(lg, p, p, t, tb, kb, pb, None, None, 1, 0, None, None, 2, 49, K,      # noqa: E731
                                                                        None, None, None, None)
    assert ps(None, p, p) == -1 and ps(p, None, p) == -1 and ps(p, p, None) == -1 and ps(None, None, None) == -1
    assert ps(p, p, p, lg=None) == -1 and ps(p, p, p, t=0) == -1
    assert ps(p, p, p, K=2049) == -2 and ps(p, p, p, K=4096) == -2
    tail = lambda tb, kb, pb, H=7, K=128: lib.spk_den_step_tail_topp(p, 8, p, 2, p, p, p, None, p, p, 3, tb, kb, pb, None, None, 1, 0,       # noqa: E731
                                                                     None, None, None, None, None, None, None, 16, 2, H, H, K, None, None,
                                                                     None)
    assert tail(None, p, p) == -1 and tail(p, None, p) == -1 and tail(p, p, None) == -1
    assert tail(p, p, p, H=9) == -2 and tail(p, p, p, K=513) == -2 and tail(p, p, p, K=0) == -2


# ------------------------------------------------------------------------------------------------- sample_top_p's argument
def _sampler():
    from snn_model.vq_diffusion import AbsorbingDiffusion, DummyModel
    return AbsorbingDiffusion(DummyModel(1, 128), mask_id=128)


def test_topp_arg_accepts_and_refuses():
    ab = _sampler()
    assert ab._topp_arg(None, 4) is None
    for p in (0.9, 1.0, 1, 1e-6, np.float32(0.5), np.float64(0.25), torch.tensor(0.9), np.array(0.9)):
        got = ab._topp_arg(p, 4)
        assert isinstance(got, float) and got == float(p)
    for v in ([0.9, 1.0, 0.25, 1e-6], (0.9, 1.0, 0.25, 1e-6), np.array([0.9, 1.0, 0.25, 1e-6]), np.array([0.9, 1.0, 0.25, 1e-6], dtype=np.float32),
              torch.tensor([0.9, 1.0, 0.25, 1e-6]), torch.tensor([0.9, 1.0, 0.25, 1e-6], dtype=torch.float64)):
        got = ab._topp_arg(v, 4)
        assert got.dtype == torch.float32 and got.device.type == "cpu" and got.tolist() == torch.tensor([0.9, 1.0, 0.25, 1e-6]).tolist()
    assert ab._topp_arg([0.5], 1).tolist() == [0.5] and ab._topp_arg([1, 1, 1, 1], 4).tolist() == [1.0] * 4
    nan = float("nan")
    bad = ([0.9, 0.5, 0.1], [0.5] * 5, np.full(3, 0.5), torch.full((5,), 0.5), torch.full((2, 2), 0.5),                 # length / shape
           0.0, -0.1, 1.5, 2, [0.5, 0.0, 0.5, 0.5], [0.5, 1.0001, 0.5, 0.5], np.array([0.5, -1e-9, 0.5, 0.5]), 1e-60,    # outside (0, 1]
           nan, INF, [0.5, nan, 0.5, 0.5], torch.tensor([0.5, INF, 0.5, 0.5]),                                           # not finite
           True, False, [True, False, True, True], np.array([True] * 4), torch.ones(4, dtype=torch.bool), "0.9", [0.5, 0.5, None, 0.5])
    for v in bad:
        with pytest.raises(ValueError, match="top_p"):
            ab._topp_arg(v, 4)


def test_sample_top_p_checks_top_p_before_anything_else():
    ab = _sampler()
    ab.n_samples = 4
    sig = inspect.signature(ab.sample_top_p).parameters
    assert list(sig) == ["top_p", "temp", "sample_steps", "noise", "record", "x_init", "known", "top_k"]
    assert list(inspect.signature(ab.sample).parameters) == list(sig)[1:-1]
    assert list(inspect.signature(ab.sample_top_k).parameters) == ["top_k"] + list(sig)[1:-1]
    assert "top_p" not in inspect.signature(ab.score).parameters
    with pytest.raises(TypeError):
        ab.score(torch.zeros(4, 1, 7, 7, dtype=torch.int64), top_p=0.9)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    for v in ([0.9, 0.5, 0.1], [0.5, 0.0, 0.5, 0.5], True, 0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            ab.sample_top_p(v, sample_steps=3)
        with pytest.raises(ValueError, match="top_p"):
            ab.sample_top_p(v, temp=[1.0, 0.5, 0.3, 0.2], sample_steps=3, top_k=4)
    with pytest.raises(ValueError, match="one entry per image"):      # the temperature's own check comes first, as in sample()
        ab.sample_top_p(0.9, temp=[1.0, 0.5], sample_steps=3)
    with pytest.raises(ValueError, match="top_k"):
        ab.sample_top_p(0.9, sample_steps=3, top_k=[1, 2])
    assert torch.equal(torch.get_rng_state(), state), "no key was drawn by a refused call"
    # a good top_p gets past the check: the next refusal is the device's
    for v in (None, 1, 0.9, [0.9, 1.0, 0.25, 1e-6], np.array([0.9, 1.0, 0.25, 1e-6]), torch.tensor([0.9, 1.0, 0.25, 1e-6])):
        with pytest.raises(RuntimeError, match="ROCm device"):
            ab.sample_top_p(v, sample_steps=3)
    assert torch.equal(torch.get_rng_state(), state) and ab.n_samples == 4
    # the graph key: one marker for every top_p, every top_k and every temperature; the other calls keep their keys
    form = ab._form(4, 7, 7)
    tv = torch.tensor([1.0, 0.5, 0.3, 0.2])
    kv = torch.tensor([1, 2, 3, 4], dtype=torch.int32)
    k1 = ab._graph_key("cuda:0", 4, 7, 7, tv, 12, form, False, top_k=kv, top_p=torch.tensor([0.9, 0.5, 1.0, 0.1]))
    k2 = ab._graph_key("cuda:0", 4, 7, 7, tv * 2, 12, form, False, top_k=kv * 0, top_p=torch.tensor([0.1, 0.1, 0.1, 0.1]))
    topk = ab._graph_key("cuda:0", 4, 7, 7, tv, 12, form, False, top_k=kv)
    plain_v, plain_s = ab._graph_key("cuda:0", 4, 7, 7, tv, 12, form, False), ab._graph_key("cuda:0", 4, 7, 7, 0.5, 12, form, False)
    assert k1 == k2 and "top-p" in k1 and "top-k" in k1 and "per-image" in k1
    assert all("top-p" not in k for k in (topk, plain_v, plain_s)) and len({k1, topk, plain_v, plain_s}) == 4
    assert topk == ab._graph_key("cuda:0", 4, 7, 7, tv, 12, form, False, top_k=kv, top_p=None)
    assert plain_v == ab._graph_key("cuda:0", 4, 7, 7, tv, 12, form, False, top_k=None, top_p=None)


def test_ops_wrappers_take_top_p_only_as_an_fp32_device_tensor():
    from spkdiff import ops
    assert ops._topp_arg(None, None, 0.9, 5, "x", "cpu") == (None, None, 0.9)
    for bad in (torch.ones(5), torch.ones(5, dtype=torch.float64), [0.5] * 5, 0.9):      # host tensors, a list, a number
        with pytest.raises(ValueError, match="fp32 device tensor"):
            ops._topp_arg(bad, None, 1.0, 5, "psample_step", "cpu")
    for name in ("psample_step", "den_step_tail"):
        assert inspect.signature(getattr(ops, name)).parameters["top_p"].default is None
    assert "top_p" not in inspect.signature(ops.pscore_step).parameters
    from snn_model.vq_diffusion import DummyModel
    assert inspect.signature(DummyModel.sample_step).parameters["top_p"].default is None


def test_sweep_and_completion_surfaces():
    from spkdiff import complete, dist, evaluate
    assert list(inspect.signature(evaluate.temperature_sweep_top_p).parameters) == [
        "model", "sampler", "temps", "n_per_temp", "top_p", "sample_steps", "batch", "T", "top_k"]
    assert inspect.signature(evaluate.temperature_sweep_range).parameters["top_p"].default is None
    assert inspect.signature(dist.temperature_sweep_sharded).parameters["top_p"].default is None
    assert inspect.signature(dist.complete_images_sharded).parameters["top_p"].default is None
    assert list(inspect.signature(complete.complete_images_top_p).parameters)[:6] == ["model", "sampler", "images", "keep", "top_p", "temp"]
    assert evaluate._sweep_top_p(None, 3, 5) is None
    assert evaluate._sweep_top_p(0.5, 3, 2).tolist() == [0.5] * 6 and evaluate._sweep_top_p(1, 2, 2).tolist() == [1.0] * 4
    pv = evaluate._sweep_top_p([0.25, 1.0, 0.5], 3, 2)
    assert pv.dtype == torch.float32 and pv.tolist() == [0.25, 0.25, 1.0, 1.0, 0.5, 0.5]
    for bad in ([0.5, 0.5], [0.5] * 4, [0.5, -0.5, 0.5], [0.5, 0.0, 0.5], 1.5, 0, True, float("nan"), "0.9"):
        with pytest.raises(ValueError, match="top_p"):
            evaluate._sweep_top_p(bad, 3, 2)


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
        self.calls.append(("sample", self.global_first, None, None))
        return self._tokens()

    def sample_top_k(self, top_k, temp=1.0, sample_steps=None):
        self.calls.append(("sample_top_k", self.global_first, None, top_k.tolist()))
        return self._tokens()

    def sample_top_p(self, top_p, temp=1.0, sample_steps=None, top_k=None):
        assert len(top_p) == len(temp) == self.n_samples and top_p.dtype == torch.float32
        assert top_k is None or (len(top_k) == self.n_samples and top_k.dtype == torch.int32)
        self.calls.append(("sample_top_p", self.global_first, top_p.tolist(), None if top_k is None else top_k.tolist()))
        return self._tokens()


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def decode_tokens(self, tokens, T=16, want_u8=True):
        return None, tokens.to(torch.uint8).reshape(-1, 1, 2, 2)


def test_sweep_slices_top_p_with_the_temperatures():
    from spkdiff import evaluate
    temps, n, ps, ks = [0.3, 1.0, 0.65], 5, [0.5, 1.0, 0.25], [1, 0, 16]
    per_image = [0.5] * 5 + [1.0] * 5 + [0.25] * 5
    per_image_k = [1] * 5 + [0] * 5 + [16] * 5
    sm = _StubSampler()
    u8, tok = evaluate.temperature_sweep_top_p(_StubModel(), sm, temps, n, ps, batch=4)
    assert [(c[0], c[1]) for c in sm.calls] == [("sample_top_p", f) for f in (0, 4, 8, 12)]
    assert [c[2] for c in sm.calls] == [per_image[f:f + 4] for f in (0, 4, 8, 12)] and all(c[3] is None for c in sm.calls)
    assert tok.shape == (3, 5, 2, 2) and (sm.n_samples, sm.global_first) == (16, 7)
    sm = _StubSampler()
    evaluate.temperature_sweep_top_p(_StubModel(), sm, temps, n, 0.5, batch=4, top_k=ks)
    assert [c[3] for c in sm.calls] == [per_image_k[f:f + 4] for f in (0, 4, 8, 12)] and sm.calls[0][2] == [0.5] * 4
    # without top_p the sweep makes today's calls
    sm2 = _StubSampler()
    evaluate.temperature_sweep(_StubModel(), sm2, temps, n, batch=4)
    evaluate.temperature_sweep_top_p(_StubModel(), sm2, temps, n, None, batch=4)
    evaluate.temperature_sweep_top_p(_StubModel(), sm2, temps, n, None, batch=4, top_k=ks)
    assert [c[0] for c in sm2.calls] == ["sample"] * 8 + ["sample_top_k"] * 4


def test_sample_top_p_none_is_sample_top_k_call_for_call(monkeypatch):
    ab = _sampler()
    seen = []
    monkeypatch.setattr(ab, "_sample_call", lambda *a, **kw: seen.append((a, kw)))
    ab.sample_top_k([1, 2, 3, 4], 0.7, 12, None, None, None, None)
    ab.sample_top_p(None, 0.7, 12, top_k=[1, 2, 3, 4])
    ab.sample(0.7, 12)
    ab.sample_top_p(None, 0.7, 12)
    norm = lambda c: (c[0] + (None,) * (8 - len(c[0])), c[1])       # noqa: E731  (top_p: not passed, or None)
    assert norm(seen[0]) == norm(seen[1]) and norm(seen[2]) == norm(seen[3])


# ------------------------------------------------------------------------------------------------- the launch sequence
def _watch(monkeypatch, key):
    """On top of the installed recorders: note every wrapper call that carries the keyword ``key``."""
    from spkdiff import ops
    seen = []
    for name in ("psample_step", "den_step_tail", "pscore_step", "select_active", "select_needed", "den_build_input", "completion_state"):
        inner = getattr(ops, name)

        def shim(*a, _inner=inner, _name=name, **kw):
            if key in kw:
                seen.append((_name, kw[key]))
            return _inner(*a, **kw)
        monkeypatch.setattr(ops, name, shim)
    return seen


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("given", [False, True], ids=["none", "top_p"])
def test_launch_sequence_with_and_without_top_p(monkeypatch, name, given):
    """Every case of tests/test_sampler_dispatch.py driven through the same entries with ``top_p`` None and with a tensor: the
    recorded launches are EXPECTED's either way; with None no call carries the keyword (nor ``top_k``), with a tensor every
    token-update call (psample_step / den_step_tail) carries that very tensor, and the ``top_k`` one, and nothing else does."""
    from snn_model.vq_diffusion import _SamplerGraph
    assert len(CASES) == 20
    case = CASES[name]
    hw = case.get('hw', 7)
    ab = dispatch_sampler(case, hw)
    cpu = torch.device('cpu')
    start = (torch.zeros((B, hw, hw), dtype=torch.int64), torch.zeros((B, hw, hw), dtype=torch.uint8)) if case.get('known') else None
    record = [] if case.get('record') else None
    noise = (lambda t: (torch.zeros(B, 1, hw, hw), torch.zeros(B * hw * hw, 128))) if case.get('inject') else None
    log = _install_recorders(monkeypatch, sampler=True)
    seen = _watch(monkeypatch, "top_p")
    seen_k = _watch(monkeypatch, "top_k")
    form = ab._form(B, hw, hw, record is not None)
    tp = torch.tensor([0.9, 1.0], dtype=torch.float32) if given else None
    tk = torch.tensor([0, 3], dtype=torch.int32) if given else None
    with torch.no_grad():
        if name.startswith('graph'):
            g = _SamplerGraph(cpu, B, hw, hw, form, int(ab.list_radii), start is not None, top_p=given)
            assert (g.topp is not None) == given and (g.topk is not None) == given and (g.temps is not None) == given
            tp, tk = g.topp, g.topk
            ab._graph_body(g, form, 1.0, STEPS)
        else:
            seed = 5 if noise is None and ab.noise_source == 'philox' else 0
            kw = dict(top_k=tk, top_p=tp) if given else {}
            ab._sample_eager(cpu, B, hw, hw, form, 1.0, STEPS, noise, seed, start, record, **kw)
    launches = [c for c in log if not c.startswith(('bn_prepare', 'pack_', 'den_pack_'))]
    assert (ab.form_for(B, hw, hw), launches) == EXPECTED[name]
    updates = [c.split('(')[0] for c in launches if c.startswith(('psample_step', 'den_step_tail'))]
    assert len(updates) == STEPS
    if given:
        assert [s[0] for s in seen] == updates and all(s[1] is tp for s in seen)
        assert [s[0] for s in seen_k] == updates and all(s[1] is tk for s in seen_k)
    else:
        assert seen == [] and seen_k == []
