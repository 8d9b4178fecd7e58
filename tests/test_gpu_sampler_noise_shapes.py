"""GPU tests of the sampler's glue kernels (csrc/psample.hip, csrc/psample_common.h, the token update of csrc/step_tail.hip,
csrc/masked_ce.hip) against host oracles, at the values and shapes the model-level tests do not reach:
  * the Philox noise itself against the host restatement of Philox4x32-10 (oracle/philox_ref.py, pinned to the Random123
    known answers by tests/test_oracle_philox.py): every key and counter word, carries, the philox_state indirection, more
    than one pass of the grid -- and every consumer of the noise, and the timed sampler configuration, on HOST-made noise;
  * spk_psample_step against an fp64 oracle on both sides of every classes-per-lane switch up to K = 2048, other latent
    sizes, temperatures, -inf / dominant / underflowing logits, the active-list form, the u == 1/t edge for every t;
  * spk_select_active beyond 64 positions and at ragged batches, spk_den_build_input, spk_q_sample, both spk_masked_ce kernels
    against fp64 per element, and the in-range rule for rows without a comparable ratio (NaN logits, all -inf).
Tokens, flags and lists must be exact; tokens of the categorical race are compared outside a stated fragile set."""
import math

import numpy as np
import pytest
import torch

from oracle import philox_ref as pr
from oracle import snn_ref as ref
from parity_report import record as parity
from spkdiff import ops, synth

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
STEP = 1 << 40                       # AbsorbingDiffusion.STEP_STRIDE: counters per reverse step in the 'global' layout
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


def s64(v):
    """A 64-bit unsigned value as the int64 that holds the same bits (the philox_state buffer is an int64 tensor)."""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def state_tensor(dev, seed, base):
    return torch.tensor([s64(seed), s64(base)], dtype=torch.int64, device=dev)


def host_noise(dev, seed, offset, B, HW, K, state=None):
    """(u, q) device tensors of one reverse step made by the HOST generator."""
    n = pr.step_noise(seed, offset, B, HW, K, state=state)
    return torch.from_numpy(n.u).to(dev), torch.from_numpy(n.q).to(dev)


def ulp32(x64):
    """Spacing of fp32 at |x| (x given in fp64)."""
    return np.spacing(np.abs(x64).astype(np.float32)).astype(np.float64)


# =============================================================================================== a. the noise itself
KEY_MIXED = 0x2BADC0DE_0000F00D          # different high and low halves, below 2^62
NOISE_CASES = [
    # name, seed, offset, B, HW, K, state
    ("zero_key_zero_counter", 0, 0, 4, 49, 128, None),
    ("seed1_carry_inside_the_call", 1, (1 << 32) - 1000, 2, 64, 100, None),
    ("seed_2_32_step1_first256", 1 << 32, 1 * STEP + 256 * 49 * 128, 8, 49, 128, None),
    ("seed_2_62m1_step2_first3", (1 << 62) - 1, 2 * STEP + 3 * 64 * 512, 4, 64, 512, None),
    ("mixed_key_step99_first1024_K2048", KEY_MIXED, 99 * STEP + 1024 * 64 * 2048, 2, 64, 2048, None),
    ("mixed_key_offset_2_63_K1", KEY_MIXED, (1 << 63) + 5, 3, 49, 1, None),
    ("seed0_step99_K100", 0, 99 * STEP + 7 * 49 * 100, 5, 49, 100, None),
    ("state_base_carries", 12345, (1 << 32) - 500, 3, 64, 128, (KEY_MIXED, 7 * STEP + (1 << 32) - 100)),
    ("state_wraps_2_64", 0, (1 << 64) - 4096, 2, 49, 100, ((1 << 62) - 1, 1000)),
    ("past_one_grid_pass", (1 << 32) + 1, 1 * STEP + 512 * 49 * 128, 340, 49, 128, None),     # 2 132 480 > 8192 * 256
]


@pytest.mark.parametrize("name,seed,offset,B,HW,K,state", NOISE_CASES, ids=[c[0] for c in NOISE_CASES])
def test_philox_noise_equals_the_host_generator(dev, name, seed, offset, B, HW, K, state):
    """spk_philox_noise against oracle/philox_ref.step_noise.  u carries the top 24 bits of the stream-0 word: bit for bit.
    q = -logf(x): x = (n + 1) * 2^-24 is exact in fp32 (n + 1 <= 2^24), so the rounding of the argument contributes nothing and
    the bound is twice the 1 ulp HIP documents for logf without fast-math (csrc/Makefile sets none): |q - q64| <= 2 ulp32(q64).
    The largest observed error in ulp goes to the parity report."""
    want = pr.step_noise(seed, offset, B, HW, K, state=state)
    st = None if state is None else state_tensor(dev, *state)
    u, q = ops.philox_noise(seed, offset, B, HW, K, dev, philox_state=st)
    assert u.shape == (B * HW,) and q.shape == (B * HW, K)
    got_u = u.cpu().numpy()
    bad_u = int((got_u.view(np.uint32) != want.u.view(np.uint32)).sum())
    err = np.abs(q.cpu().numpy().astype(np.float64) - want.q64) / ulp32(want.q64)
    worst = float(err.max())
    parity(f"philox_noise_{name}", u_mismatches=bad_u, positions=B * HW, q_max_err_ulp=round(worst, 4),
           q_differs_from_rounded_fp64=int((q.cpu().numpy() != want.q).sum()), q_bound_ulp=2.0)
    assert bad_u == 0, f"{bad_u} of {B * HW} uniforms differ, first {np.nonzero(got_u != want.u)[0][:8].tolist()}"
    if name == "zero_key_zero_counter":
        assert float(got_u[0]) == 0x6627e8 / 2.0 ** 24          # Random123 known answer 6627e8d5, top 24 bits
    assert worst <= 2.0, f"q off by {worst} ulp at {np.unravel_index(int(err.argmax()), err.shape)}"
    assert float(q.min()) >= 0.0 and float(q.max()) <= 16.64 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    # u alone is the same u
    u_only, none = ops.philox_noise(seed, offset, B, HW, K, dev, philox_state=st, want_q=False)
    assert none is None and torch.equal(u_only, u)


# =============================================================================================== b. the consumers
def build_den(dev, cfg=synth.MNIST):
    from snn_model.vq_diffusion import DummyModel, functional
    sd = synth.synth_denoiser_state(cfg)
    d = DummyModel(1, cfg.num_embeddings).cuda(0)
    functional.set_step_mode(net=d, step_mode='m')
    d.load_state_dict(sd)
    return d.eval(), sd


KEY_B = (1 << 45) + 12345            # a key above 2^32
FIRST_B = 512                        # first image of the shard


def philox_forms(dev, s, HW, K):
    """(seed, offset, philox_state) of reverse step number s of a shard starting at image FIRST_B, stated directly and through
    the philox_state indirection (as the captured graph passes it: per-step offset baked in, {key, base} in the buffer)."""
    off = s * STEP + FIRST_B * HW * K
    return [("direct", KEY_B, off, None),
            ("state", 99, off, state_tensor(dev, KEY_B, 0)),
            ("state_with_base", 99, FIRST_B * HW * K, state_tensor(dev, KEY_B, s * STEP))]


@pytest.mark.parametrize("K,L,B,s", [(128, 7, 64, 1), (512, 8, 9, 37), (1000, 7, 5, 99)])
def test_psample_and_select_active_draw_the_host_noise(dev, K, L, B, s):
    """spk_psample_step and spk_select_active in Philox mode == the same calls with the host-made (u, q) injected, bit for bit,
    at counters s * 2^40 + first * HW * K under a key above 2^32."""
    HW = L * L
    g = torch.Generator().manual_seed(K + s)
    logits = (torch.randn(B, K, L, L, generator=g) * 2).to(dev)
    un0 = (torch.rand(B, 1, L, L, generator=g) < 0.4).to(dev)
    x0 = torch.randint(0, K, (B, 1, L, L), generator=g).to(dev)
    u, q = host_noise(dev, KEY_B, s * STEP + FIRST_B * HW * K, B, HW, K)
    diffs = 0
    for t in (1, 4, 60):
        xb, unb, hb = x0.clone(), un0.clone(), torch.full((B * HW,), -7, dtype=torch.int64, device=dev)
        ops.psample_step(logits, xb, unb, t, 0.9, u, q, x0_hat=hb)
        a2, n2 = ops.select_active(un0, t, u)
        want_n = int(((u.view(B, HW) < float(np.float32(1.0) / np.float32(t))) & ~un0.view(B, HW)).any(1).sum())
        assert int(n2[0]) == want_n
        for form, seed, off, st in philox_forms(dev, s, HW, K):
            xa, una, ha = x0.clone(), un0.clone(), torch.full((B * HW,), -7, dtype=torch.int64, device=dev)
            ops.psample_step(logits, xa, una, t, 0.9, None, None, seed, off, philox_state=st, x0_hat=ha)
            d = int((xa != xb).sum()) + int((una != unb).sum()) + int((ha != hb).sum())
            # ... and the form that skips unchanged positions before the softmax
            xc, unc = x0.clone(), un0.clone()
            ops.psample_step(logits, xc, unc, t, 0.9, None, None, seed, off, philox_state=st)
            d += int((xc != xb).sum()) + int((unc != unb).sum())
            a1, n1 = ops.select_active(un0, t, None, seed, off, philox_state=st, K=K)
            d += int(int(n1[0]) != int(n2[0])) + int(not torch.equal(a1[:int(n1[0])], a2[:int(n2[0])]))
            assert d == 0, (form, t, d)
            diffs += d
    parity(f"consumers_on_host_noise_psample_K{K}_{L}x{L}", differing=diffs)


@pytest.mark.parametrize("s", [1, 99])
def test_select_needed_and_step_tail_draw_the_host_noise(dev, s):
    """spk_select_needed and spk_den_step_tail (7x7, K = 128) in Philox mode == the same calls on injected host-made noise."""
    den, _ = build_den(dev)
    B, L, K = 37, 7, 128
    HW = L * L
    g = torch.Generator().manual_seed(900 + s)
    u, q = host_noise(dev, KEY_B, s * STEP + FIRST_B * HW * K, B, HW, K)
    for t in (30, 2):
        x0 = torch.randint(0, K, (B, 1, L, L), generator=g)
        un0 = torch.rand(B, 1, L, L, generator=g) < 0.5
        x0[~un0] = K
        x0, un0 = x0.to(dev), un0.to(dev)
        x5, cnt5, x1, cnt1, which, impl, collapse = den._trunk(ops.den_build_input(x0, t), False)
        conv6, packed6 = den._conv6_params()
        xb, unb = x0.clone(), un0.clone()
        _, lgb = ops.den_step_tail(cnt5, cnt1, packed6, xb, unb, t, 0.9, T=16, K=K, u=u, q=q, conv1=None, want_logits=True)
        assert int(unb.sum()) > int(un0.sum())
        act_b = ops.select_active(un0, t, u)
        nb = int(act_b[1][0])
        need_b = ops.select_needed(un0, t, act_b, ops.NeedLists(B, 3, dev), u)
        for form, seed, off, st in philox_forms(dev, s, HW, K):
            xa, una = x0.clone(), un0.clone()
            _, lga = ops.den_step_tail(cnt5, cnt1, packed6, xa, una, t, 0.9, T=16, K=K, seed=seed, offset=off, philox_state=st,
                                       conv1=None, want_logits=True)
            assert torch.equal(lga, lgb) and torch.equal(xa, xb) and torch.equal(una, unb), (form, t)
            act_a = ops.select_active(un0, t, None, seed, off, philox_state=st, K=K)
            assert int(act_a[1][0]) == nb and torch.equal(act_a[0][:nb], act_b[0][:nb])
            need_a = ops.select_needed(un0, t, act_a, ops.NeedLists(B, 3, dev), None, seed, off, philox_state=st, K=K)
            for r in (1, 2, 3):
                assert torch.equal(need_a.records(r)[:nb, :51], need_b.records(r)[:nb, :51]), (form, t, r)
    parity(f"consumers_on_host_noise_step_tail_step{s}", differing=0)


# =============================================================================================== c. the timed configuration
def test_timed_configuration_philox_graph_vs_oracle_on_host_made_noise(dev):
    """The configuration bench.py times (Philox noise, the reverse process replayed from one hipGraph), dense and with the
    untouched-image elimination + lists, token-identical to the CPU oracle run on noise the HOST generator made from the
    sampler's key and the 'global' counter layout (step s at s * 2^40): nothing in the chain comes from the device's own
    generator, so a lost counter or key word shows.  sample() runs twice per sampler: the second replay takes its key through
    the philox_state buffer.  B = 4 x 100 steps x 2 keys: twice the host time of the dumped-noise case next to it."""
    from snn_model.vq_diffusion import AbsorbingDiffusion
    den, sd = build_den(dev)
    B, steps, L, K = 4, 100, 7, 128
    probe = AbsorbingDiffusion(den, mask_id=K)
    torch.manual_seed(777)
    keys = [probe._philox_key(), probe._philox_key()]
    assert keys[0] != keys[1] and min(keys) > 1 << 32
    got = {}
    for name, skip, lists in (("dense", False, False), ("elim+lists", True, True)):
        ab = AbsorbingDiffusion(den, mask_id=K)
        ab.n_samples, ab.skip_untouched, ab.list_positions, ab.list_min_batch = B, skip, lists, 1
        assert ab.noise_source == 'philox' and ab.use_graph and ab.noise_layout == 'global'
        torch.manual_seed(777)
        for i in range(2):
            got[name, i] = ab.sample(temp=1.0, sample_steps=steps).cpu()
            assert ab.last_key == keys[i]
        assert len(ab._graphs) == 1, "both runs replayed one captured hipGraph"
    bad = {}
    for i, key in enumerate(keys):
        def noise(t):
            n = pr.step_noise(key, (steps - t) * STEP, B, L * L, K)
            return torch.from_numpy(n.u).view(B, 1, L, L), torch.from_numpy(n.q)
        want = ref.absorbing_sample(sd, B, K, 1.0, steps, L, 16, noise=noise)
        for name in ("dense", "elim+lists"):
            bad[f"{name}_run{i}"] = int((got[name, i] != want).sum())
    assert not torch.equal(got["dense", 0], got["dense", 1])
    parity("timed_configuration_philox_graph_on_host_made_noise", token_mismatches=bad, tokens=B * L * L)
    assert all(v == 0 for v in bad.values()), bad


LOOP_FORMS = [
    # name, skip_untouched, list_positions, use_step_tail, step_tail_in_elimination, what form_for says
    ("dense", False, False, False, False, "dense"),
    ("dense+tail", False, False, True, False, "dense_step_tail"),
    ("elim", True, False, True, False, "elimination"),
    ("elim+lists", True, True, True, False, "elimination_lists"),
    ("elim+lists+tail", True, True, True, True, "elimination_lists"),
]


def test_one_step_loop_eager_and_captured_in_every_form(dev):
    """The one step loop behind sample(), driven captured (capture + replay, then a second replay) and eagerly (twice) under the
    same seed, in each launch form: B = 3 on 7x7 (one image below and above ``list_min_batch = 1``), 5 steps (first step != a
    middle step != last step).  First calls equal, second calls equal, first != second (a fresh key per call), and every
    form equal to the dense eager result."""
    from snn_model.vq_diffusion import AbsorbingDiffusion
    den, _ = build_den(dev)
    B, steps, K = 3, 5, 128
    got = {}
    for name, skip, lists, tail, tail_elim, form_name in LOOP_FORMS:
        den.use_step_tail = tail
        ab = AbsorbingDiffusion(den, mask_id=K)
        ab.n_samples, ab.list_min_batch = B, 1
        ab.skip_untouched, ab.list_positions, ab.step_tail_in_elimination = skip, lists, tail_elim
        form = ab._form(B, 7, 7)
        assert ab.form_for(B, 7, 7) == form_name and form.tail == (tail and not skip) and form.tail_act == tail_elim
        for graph in (True, False):
            ab.use_graph = graph
            torch.manual_seed(4242)
            for i in range(2):
                got[name, graph, i] = ab.sample(temp=1.0, sample_steps=steps).cpu()
            # (a failed capture would have switched use_graph off; the eager calls capture nothing more)
            assert ab.use_graph is graph and len(ab._graphs) == 1
    want = [got["dense", False, i] for i in range(2)]
    assert not torch.equal(want[0], want[1]) and bool(((want[0] >= 0) & (want[0] < K)).all())
    bad = {f"{name}_{'graph' if graph else 'eager'}_call{i}": int((tok != want[i]).sum()) for (name, graph, i), tok in got.items()}
    parity("one_step_loop_eager_and_captured_forms", token_mismatches=bad, tokens=B * 49)
    assert all(v == 0 for v in bad.values()), bad


# =============================================================================================== d. spk_psample_step vs fp64
# Fragile set.  A position's token is argmax_k r_k, r_k = softmax(l / temp)_k / q_k.  MEASURED on the CPU over the inputs of
# the cases below (measure_fp32_error; tests/test_gpu_sampler_noise_shapes.py run on the host): the fp32 reference expression
# (ref.categorical_sample's, on logits / temp) differs from the fp64 ratios, at the two largest ratios of a row and relative
# to the largest, by at most
#     temp 0.5 / 1 / 2 (also -inf entries, a +80 class, spreads that underflow expf)   9.39e-7  (K = 2048, temp 2)  -> REG_MEASURED
#     temp 1e-3 ("wide": the fp32 rounding of logits / temp ~ 1e4 alone is ~ 5e-4)     2.96e-4  (K = 1500)          -> WIDE_MEASURED
# A position is fragile if its two largest fp64 ratios are closer than 8x that, relative to the largest (two fp32 evaluation
# orders may each be off by the measured amount, with margin): 7.52e-6 and 2.4e-3.  Fragile positions are left out of the token
# comparison only; at most 0.1 % of the positions of a case may be fragile (on the host no case below has a fragile position).
# Every case re-measures its inputs and fails if they exceed the recorded value.
REG_MEASURED, WIDE_MEASURED = 9.4e-7, 3.0e-4
REG_THRESHOLD, WIDE_THRESHOLD = 8 * REG_MEASURED, 8 * WIDE_MEASURED
FRAGILE_CAP = 1e-3


def rows_of(logits):
    B, K = logits.shape[:2]
    return logits.flatten(2).permute(0, 2, 1).reshape(-1, K)


def ratios_f64(logits, temp, q):
    l = rows_of(logits).double() / float(np.float32(temp))
    return torch.softmax(l, -1) / q.double()


def ratios_ref_f32(logits, temp, q):
    """ref.categorical_sample's expression with the ratios kept."""
    l = rows_of(logits) / temp
    ln = l - l.logsumexp(dim=-1, keepdim=True)
    return torch.softmax(ln, dim=-1) / q


def measure_fp32_error(logits, temp, q):
    """Largest |r32 - r64| / max_k r64 over the two largest (fp64) ratios of each row."""
    r64, r32 = ratios_f64(logits, temp, q), ratios_ref_f32(logits, temp, q)
    assert torch.equal(r32.argmax(-1), ref.categorical_sample(rows_of(logits) / temp, q))
    top = r64.topk(min(2, r64.shape[1]), -1)
    return float(((r32.double().gather(1, top.indices) - top.values).abs() / top.values[:, :1]).max())


def oracle_tokens(logits, temp, q, thr):
    """fp64 tokens (first index on a tie; a NaN ratio never wins unless the row has nothing else, then 0) and the fragile mask."""
    r = ratios_f64(logits, temp, q)
    allnan = torch.isnan(r).all(-1)
    r = torch.where(torch.isnan(r), torch.full_like(r, -1.0), r)
    tok = r.argmax(-1)
    tok[allnan] = 0
    if r.shape[1] < 2:
        return tok, torch.zeros_like(tok, dtype=torch.bool)
    top = r.topk(2, -1).values
    fragile = ((top[:, 0] - top[:, 1]) < thr * top[:, 0]) & ~allnan & ~torch.isinf(top[:, 0])
    return tok, fragile


def psample_inputs(B, K, H, W, seed, kind="randn"):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, K, H, W, generator=g) * 3
    if kind == "neg_inf":
        hole = torch.rand(B, K, H, W, generator=g) < 0.3
        hole[:, K // 2] = False                                  # (every position keeps a finite class)
        logits[hole] = -INF
    elif kind == "dominant":
        logits.scatter_(1, torch.randint(0, K, (B, 1, H, W), generator=g), 80.0)
    elif kind == "spread":
        logits *= 40.0                                           # (expf(l - max) underflows for most classes)
    HW = H * W
    q = torch.empty(B * HW, K).exponential_(1, generator=g)
    u = torch.rand(B * HW, generator=g)
    un0 = torch.rand(B, 1, H, W, generator=g) < 0.4
    x0 = torch.randint(0, K, (B, 1, H, W), generator=g)
    x0[~un0] = K                                                 # the mask id
    return logits, q, u, x0, un0


def check_psample(dev, name, inp, t, temp, wide=False, active=None):
    """One spk_psample_step call per form against the fp64 oracle.  ``active``: list of images (the active-list form)."""
    logits, q, u, x0, un0 = inp
    B, K, H, W = logits.shape
    HW = H * W
    measured_cap, thr = (WIDE_MEASURED, WIDE_THRESHOLD) if wide else (REG_MEASURED, REG_THRESHOLD)
    measured = measure_fp32_error(logits, temp, q)
    tok, fragile = oracle_tokens(logits, temp, q, thr)
    share = float(fragile.float().mean())
    changes = (u < torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(t), dtype=torch.float32)) & ~un0.flatten()
    if active is not None:
        on = torch.zeros(B, dtype=torch.bool)
        on[torch.tensor(active, dtype=torch.long)] = True
        changes &= on.repeat_interleave(HW)
    want_un = un0.flatten() | changes
    ld, qd, ud = logits.to(dev), q.to(dev), u.to(dev)
    wrong = 0
    forms = ["skip", "x0_hat"] if active is None else ["active"]
    for form in forms:
        xa, una = x0.to(dev), un0.to(dev)
        hat = torch.full((B * HW,), -7, dtype=torch.int64, device=dev) if form == "x0_hat" else None
        nxt = torch.full((B, 2, H, W), NAN, device=dev) if active is None else None
        if active is None:
            ops.psample_step(ld, xa, una, t, temp, ud, qd, x0_hat=hat, next_input=nxt)
        else:
            slots = torch.zeros_like(ld)
            if active:
                slots[:len(active)] = ld[torch.tensor(active, dtype=torch.long, device=dev)]
            act = torch.full((B,), 0, dtype=torch.int32, device=dev)
            act[:len(active)] = torch.tensor(active, dtype=torch.int32)
            n_act = torch.tensor([len(active), 0], dtype=torch.int32, device=dev)
            with ops.active_set(act, n_act):
                ops.psample_step(slots, xa, una, t, temp, ud, qd)
        xa_c, una_c = xa.cpu().flatten(), una.cpu().flatten()
        assert torch.equal(una_c, want_un), f"{name}/{form}: unmasked differs at {(una_c != want_un).nonzero().flatten()[:8].tolist()}"
        assert torch.equal(xa_c[~changes], x0.flatten()[~changes]), f"{name}/{form}: a token that does not change was written"
        assert bool(((xa_c[changes] >= 0) & (xa_c[changes] < K)).all()), f"{name}/{form}: token out of [0, {K})"
        cmp = changes & ~fragile
        bad = (xa_c[cmp] != tok[cmp]).nonzero().flatten()
        wrong += bad.numel()
        assert bad.numel() == 0, f"{name}/{form}: {bad.numel()} of {int(cmp.sum())} tokens differ from the fp64 oracle"
        if hat is not None:
            hc = hat.cpu()
            assert bool(((hc >= 0) & (hc < K)).all()), f"{name}: x0_hat unwritten or out of range"
            assert torch.equal(hc[~fragile], tok[~fragile]), f"{name}: x0_hat differs from the fp64 oracle"
            assert torch.equal(hc[changes], xa_c[changes])
        if nxt is not None:
            want_nxt = torch.cat([xa.float(), torch.full_like(xa, t - 1).float()], 1)
            assert torch.equal(nxt, want_nxt), f"{name}/{form}: next_input is not cat(x_t, t - 1)"
    parity(f"psample_fp64_{name}", positions=B * HW, fragile=int(fragile.sum()), fragile_share=share, threshold=thr,
           fp32_reference_error_measured=measured, wrong_tokens=wrong)
    assert measured <= measured_cap, f"{name}: fp32 reference error {measured} above the value the threshold was derived from"
    assert share <= FRAGILE_CAP, f"{name}: {int(fragile.sum())} of {B * HW} positions fragile"


K_EDGES = [1, 2, 63, 64, 65, 256, 257, 512, 513, 1000, 1024, 1025, 2048]      # both sides of every classes-per-lane switch


@pytest.mark.parametrize("temp", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("K", K_EDGES)
def test_psample_step_vs_fp64_codebook_sizes(dev, K, temp):
    B = 21 if K <= 1025 else 11
    check_psample(dev, f"K{K}_temp{temp}", psample_inputs(B, K, 7, 7, 1000 + K), 3, temp)


@pytest.mark.parametrize("K", [65, 513, 2048])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 8), (9, 9)])
def test_psample_step_vs_fp64_latent_sizes(dev, H, W, K):
    B = 300 if H * W == 1 else 9
    check_psample(dev, f"K{K}_{H}x{W}", psample_inputs(B, K, H, W, 2000 + K + H), 2, 1.0)


def test_psample_step_vs_fp64_past_one_grid_pass(dev):
    """340 x 49 = 16 660 positions: more waves than the 4096 workgroups x 4 hold in one pass."""
    check_psample(dev, "B340_K8", psample_inputs(340, 8, 7, 7, 31), 2, 1.0)
    check_psample(dev, "B270_8x8_K5", psample_inputs(270, 5, 8, 8, 32), 5, 2.0)


@pytest.mark.parametrize("K", [100, 300, 600, 1500])
@pytest.mark.parametrize("kind,temp,wide", [("neg_inf", 1.0, False), ("neg_inf", 0.5, False), ("dominant", 1.0, False),
                                            ("spread", 1.0, False), ("spread", 2.0, False), ("randn", 1e-3, True)])
def test_psample_step_vs_fp64_hard_logits(dev, K, kind, temp, wide):
    check_psample(dev, f"{kind}_K{K}_temp{temp}", psample_inputs(9, K, 7, 7, 3000 + K, kind), 2, temp, wide=wide)


@pytest.mark.parametrize("K", [128, 700])
@pytest.mark.parametrize("t", [1, 1000])
def test_psample_step_first_and_late_steps(dev, K, t):
    """t = 1: u < 1 always, every masked position changes; t = 1000: almost none does."""
    inp = psample_inputs(40, K, 7, 7, 4000 + K + t)
    check_psample(dev, f"K{K}_t{t}", inp, t, 1.0)
    u, un0 = inp[2], inp[4].flatten()
    n = int(((u < float(np.float32(1.0) / np.float32(t))) & ~un0).sum())
    assert n == int((~un0).sum()) if t == 1 else n < 20


@pytest.mark.parametrize("K,L", [(128, 7), (600, 8), (1100, 7)])
def test_psample_step_active_list_form(dev, K, L):
    """Lists of length 0, 1, some and B: images that are not listed keep x_t / unmasked bit for bit."""
    B = 12
    inp = psample_inputs(B, K, L, L, 5000 + K)
    for active in ([], [7], [0, 3, 4, 11], list(range(B))):
        check_psample(dev, f"active{len(active)}_K{K}_{L}x{L}", inp, 2, 1.0, active=active)


def test_psample_step_refuses_more_than_2048_classes(dev):
    B, K = 1, 2049
    x0 = torch.full((B, 1, 2, 2), K, dtype=torch.int64, device=dev)
    un0 = torch.zeros((B, 1, 2, 2), dtype=torch.bool, device=dev)
    hat = torch.full((4,), -7, dtype=torch.int64, device=dev)
    with pytest.raises(NotImplementedError):
        ops.psample_step(torch.zeros(B, K, 2, 2, device=dev), x0, un0, 1, 1.0, torch.zeros(4, device=dev),
                         torch.ones(4, K, device=dev), x0_hat=hat)
    torch.cuda.synchronize()
    assert bool((x0 == K).all()) and not bool(un0.any()) and bool((hat == -7).all())


def test_psample_step_exponential_of_zero(dev):
    """q = 0 (reachable in Philox mode: a 24-bit mantissa of all ones).  A class with q = 0 and a probability above zero has
    ratio +inf and wins, the lowest such class on a tie; with a probability of zero (logit -inf) the ratio is 0 / 0 = NaN and
    the class never wins (oracle/philox_ref.py states this contract)."""
    for K in (7, 300, 600, 1100, 2048):
        logits, q, u, x0, un0 = psample_inputs(4, K, 3, 3, 6000 + K)
        rows = q.shape[0]
        want, _ = oracle_tokens(logits, 1.0, q, REG_THRESHOLD)
        a, b, c = K // 3, K // 2, K - 1
        q[0, c] = 0.0; want[0] = c                                # one zero
        q[1, b] = 0.0; q[1, c] = 0.0; want[1] = b                 # two zeros: the lower class
        q[2, a] = 0.0; q[2, b] = 0.0
        lr = rows_of(logits)                                      # (a copy)
        lr[2, a] = -INF; want[2] = b                              # 0 / 0 at class a never wins
        lr[3, a] = -INF; q[3, a] = 0.0                            # ... and leaves the rest of the race alone
        logits = lr.reshape(4, 9, K).permute(0, 2, 1).reshape(4, K, 3, 3).contiguous()
        want[3] = oracle_tokens(logits, 1.0, q, REG_THRESHOLD)[0][3]
        assert want[3] != a
        hat = torch.full((rows,), -7, dtype=torch.int64, device=dev)
        ops.psample_step(logits.to(dev), x0.to(dev), un0.to(dev), 1, 1.0, u.to(dev), q.to(dev), x0_hat=hat)
        _, fragile = oracle_tokens(logits, 1.0, q, REG_THRESHOLD)
        fragile[:4] = False
        assert int(fragile.sum()) == 0
        assert torch.equal(hat.cpu(), want), (K, hat.cpu()[:4].tolist(), want[:4].tolist())


def next_f32(x, up):
    return np.nextafter(np.float32(x), np.float32(2.0 if up else -1.0), dtype=np.float32)


def test_change_threshold_edges_every_t(dev):
    """changes = u < fp32(1 / t): for t = 1..100, u on the threshold (no change), one fp32 below (change), one above (none) --
    in spk_psample_step, spk_select_active (an image whose only candidate sits on the threshold is not listed) and
    spk_select_needed (positions on the threshold do not enter the lists).  1.0f / (float)t equals torch's fp32 1 / t and the
    double-rounded value for every t here, so one host expression serves."""
    K = 4
    logits = torch.zeros(3, K, 7, 7)
    logits[:, 2] = 5.0
    q = torch.ones(3 * 49, K)
    ld, qd = logits.to(dev), q.to(dev)
    need = ops.NeedLists(3, 1, dev)
    act = None
    for t in range(1, 101):
        thr = np.float32(1.0) / np.float32(t)
        assert float(thr) == float(torch.tensor(1.0) / torch.tensor(float(t))) == float(np.float32(1.0 / t))
        u = torch.full((3, 49), 0.999)
        un0 = torch.ones(3, 1, 7, 7, dtype=torch.bool)
        un0.view(3, 49)[:, [10, 24, 40]] = False                 # candidates: still masked
        u[0, [10, 24, 40]] = torch.tensor([float(thr), float(next_f32(thr, True)), 0.999])      # image 0: on / above: nothing
        u[1, [10, 24, 40]] = torch.tensor([float(thr), float(next_f32(thr, False)), float(next_f32(thr, True))])   # image 1: 24 changes
        u[2, [10, 24, 40]] = float(thr)                          # image 2: all on the threshold
        if t == 1:
            u[u == 0.999] = 1.0
        x0 = torch.full((3, 1, 7, 7), 1, dtype=torch.int64)
        x0[~un0] = K
        xa, una, ud = x0.to(dev), un0.to(dev), u.reshape(-1).to(dev)
        act = ops.select_active(una, t, ud, out=act)
        assert act[1].cpu().tolist() == [1, 0] and int(act[0][0]) == 1, t
        ops.select_needed(una, t, act, need, ud)
        rec = need.records(1)[0].cpu().tolist()
        assert rec[48] == 9 and rec[:9] == [16, 17, 18, 23, 24, 25, 30, 31, 32] and rec[50] == 0, (t, rec[:12])
        ops.psample_step(ld, xa, una, t, 1.0, ud, qd)
        want_un, want_x = un0.clone(), x0.clone()
        want_un.view(3, 49)[1, 24] = True
        want_x.view(3, 49)[1, 24] = 2
        assert torch.equal(una.cpu(), want_un) and torch.equal(xa.cpu(), want_x), t


# =============================================================================================== e. select_active, build_input
@pytest.mark.parametrize("HW", [1, 7, 49, 64, 65, 81, 200])
def test_select_active_latent_and_batch_sizes(dev, HW):
    """spk_select_active against the torch `changes` expression on injected u and, in Philox mode, on the host generator's u:
    latents beyond 64 positions (the kernel's second loop), ragged batches, empty and full lists, the work word back at zero
    (two calls per buffer)."""
    g = torch.Generator().manual_seed(HW)
    K = 16
    for B in (1, 7, 8, 9, 63, 64, 65, 300):
        out = None
        for t, p_un in ((max(2, HW // 2), 0.5), (HW + 3, 0.9), (1, 0.0), (5, 1.0)):
            un = torch.rand(B, HW, generator=g) < p_un
            u = torch.rand(B, HW, generator=g)
            want = torch.nonzero(((u < 1.0 / t) & ~un).any(1)).flatten().int()
            if p_un == 1.0:
                assert want.numel() == 0
            if t == 1:
                assert want.numel() == B
            und = un.view(B, 1, 1, HW).to(dev)
            out = ops.select_active(und, t, u.to(dev), out=out)
            n = out[1].cpu().tolist()
            assert n == [want.numel(), 0], (B, t, n)
            assert torch.equal(out[0][:n[0]].cpu(), want), (B, t)
            off = 5 * STEP + 77 * HW * K
            hu = torch.from_numpy(pr.step_noise(KEY_B, off, B, HW, K, want_q=False).u).view(B, HW)
            want_p = torch.nonzero(((hu < 1.0 / t) & ~un).any(1)).flatten().int()
            out = ops.select_active(und, t, None, KEY_B, off, out=out, K=K)
            n = out[1].cpu().tolist()
            assert n == [want_p.numel(), 0] and torch.equal(out[0][:n[0]].cpu(), want_p), (B, t, "philox")


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (5, 7, 7), (37, 8, 8), (300, 3, 5)])
def test_den_build_input_forms(dev, B, H, W):
    """spk_den_build_input == cat(x, t): float and token inputs, t as a vector and as a scalar, with and without the active list."""
    g = torch.Generator().manual_seed(B + H)
    tok = torch.randint(0, 2049, (B, 1, H, W), generator=g)
    tv = torch.randint(1, 1000, (B,), generator=g)
    listed = sorted(set(torch.randint(0, B, (max(1, B // 2),), generator=g).tolist()))
    for x in (tok, tok.float() + 0.25):
        for t in (tv, 17):
            tt = t if torch.is_tensor(t) else torch.full((B,), t)
            want = torch.cat([x.float(), tt.float().view(B, 1, 1, 1).expand(B, 1, H, W)], 1)
            td = t.to(dev) if torch.is_tensor(t) else t
            assert torch.equal(ops.den_build_input(x.to(dev), td).cpu(), want)
            for lst in ([], listed, list(range(B))):
                act = torch.zeros(B, dtype=torch.int32, device=dev)
                act[:len(lst)] = torch.tensor(lst, dtype=torch.int32)
                out = torch.full((B, 2, H, W), NAN, device=dev)
                with ops.active_set(act, torch.tensor([len(lst), 0], dtype=torch.int32, device=dev)):
                    ops.den_build_input(x.to(dev), td, out=out)
                oc = out.cpu()
                assert torch.equal(oc[:len(lst)], want[lst]) and bool(torch.isnan(oc[len(lst):]).all())


# =============================================================================================== f. spk_q_sample
def run_q_sample(dev, x0, t, u, T, mask_id):
    want = ref.q_sample(x0, t, T, mask_id, u=u)
    got = ops.q_sample(x0.to(dev), t.to(dev), u.to(dev), T, mask_id)
    for name, g_, w_ in zip(("x_t", "x_0_ignore", "mask"), got, want):
        assert g_.shape == w_.shape and g_.dtype == w_.dtype
        assert torch.equal(g_.cpu(), w_), f"{name}: {int((g_.cpu() != w_).sum())} differ"
    return want


@pytest.mark.parametrize("B,H,W,T", [(1, 1, 1, 49), (5, 7, 7, 49), (1341, 7, 7, 49), (1025, 8, 8, 100), (3, 3, 5, 100)])
def test_q_sample_vs_reference(dev, B, H, W, T):
    """spk_q_sample against ref.q_sample on injected u; 1341 x 49 = 65 709 and 1025 x 64 = 65 600 elements: not multiples of
    256, above 65 536; t covers 0 (nothing masked) and T (everything)."""
    g = torch.Generator().manual_seed(B * T)
    x0 = torch.randint(0, 512, (B, 1, H, W), generator=g).float()
    t = torch.randint(0, T + 1, (B,), generator=g)
    t[0] = T
    t[-1] = 0 if B > 1 else T
    u = torch.rand(B, 1, H, W, generator=g)
    x_t, ign, mask = run_q_sample(dev, x0, t, u, T, 512.0)
    assert bool(mask[0].all()) and (B == 1 or not bool(mask[-1].any()))
    assert 0 < int(mask.sum()) <= mask.numel()


@pytest.mark.parametrize("T", [49, 100])
def test_q_sample_threshold_edges(dev, T):
    """mask = u < fp32(t) / fp32(T): u on the threshold (kept), one fp32 below (masked), one above (kept), for every t in 1..T
    (and t = 0: nothing below zero).  fp32(t) / fp32(T) equals the double-rounded t / T for these T."""
    t = torch.arange(0, T + 1)
    thr = (t.float() / T).numpy()
    assert np.array_equal(thr, (t.double() / T).float().numpy())
    u = torch.empty(T + 1, 1, 2, 2)
    u[:, 0, 0, 0] = torch.from_numpy(thr)
    u[:, 0, 0, 1] = torch.from_numpy(np.nextafter(thr, np.float32(-1.0)).clip(min=0))
    u[:, 0, 1, 0] = torch.from_numpy(np.nextafter(thr, np.float32(2.0)))
    u[:, 0, 1, 1] = 0.0
    x0 = torch.arange(4 * (T + 1)).float().view(T + 1, 1, 2, 2)
    _, _, mask = run_q_sample(dev, x0, t, u, T, 999.0)
    want = torch.zeros(T + 1, 1, 2, 2, dtype=torch.bool)
    want[1:, 0, 0, 1] = True
    want[1:, 0, 1, 1] = True
    assert torch.equal(mask, want)


def test_q_sample_without_the_mask_output(dev):
    from spkdiff._lib import check, lib
    g = torch.Generator().manual_seed(8)
    B, HW, T = 9, 49, 49
    x0 = torch.randint(0, 128, (B, 1, 7, 7), generator=g).float()
    t = torch.randint(1, T + 1, (B,), generator=g)
    u = torch.rand(B, 1, 7, 7, generator=g)
    want = ref.q_sample(x0, t, T, 128.0, u=u)
    xd, td, ud = x0.to(dev), t.to(dev), u.to(dev)
    x_t, ign = torch.full_like(xd, NAN), torch.full_like(xd, NAN)
    check(lib.spk_q_sample(xd.data_ptr(), td.data_ptr(), ud.data_ptr(), x_t.data_ptr(), ign.data_ptr(), None, B, HW, T, 128.0,
                           torch.cuda.current_stream().cuda_stream), "spk_q_sample")
    assert torch.equal(x_t.cpu(), want[0]) and torch.equal(ign.cpu(), want[1])


# =============================================================================================== g. spk_masked_ce
EPS32 = 2.0 ** -23
CE_TILE = 16384                      # floats of LDS: K*HW + 2*HW above it takes the kernel without the tile


def ce_oracle(logits, target, coef):
    """fp64: F.cross_entropy(ignore_index = -1, reduction = 'none') and the closed-form gradient coef * (softmax - onehot);
    targets truncated towards zero, targets outside [0, K) ignored (what the kernel documents)."""
    import torch.nn.functional as F
    B, K = logits.shape[:2]
    l = logits.double().flatten(2)
    tg = torch.where((target >= 0) & (target < K), target.double().floor(), torch.full_like(target, -1).double()).long().view(B, -1)
    ce = F.cross_entropy(l, tg, ignore_index=-1, reduction='none')
    sm = torch.softmax(l, 1)
    onehot = torch.zeros_like(sm).scatter_(1, tg.clamp(min=0).unsqueeze(1), 1.0)
    grad = coef.double().view(B, 1, 1) * (sm - onehot)
    grad = torch.where((tg >= 0).unsqueeze(1), grad, torch.zeros_like(grad))
    return ce, grad, tg, sm


def check_masked_ce(dev, name, logits, target, coef):
    """Per-element bounds in fp32 roundings.  With m the row maximum and S = sum exp(l - m) in [1, K]:
      ce  = log S - (l_t - m): the subtraction l - m (1 rounding of a value up to |l_t - m|), K expf at <= 2 ulp each feeding a
            K-term serial fp32 sum (relative error <= (K + 2) eps/2 of S, the same absolute error in log S), logf (<= 2 ulp of
            log S <= log K) and the final subtraction (1 rounding of ce):
               |err| <= eps * (|l_t - m| + (K + 2) / 2 + 2 log K + |ce|) + eps
      grad = coef * (exp(l - off) - [k = t]), off = m + log S rounded (a value up to |m| + log K): the argument l - off carries the
            error of log S, the rounding of off and its own (a value up to |l - m| + log K); expf 2 ulp, the difference and the
            product 1 rounding each; one more eps absolute for probabilities that underflow in fp32:
               |err| <= |coef| * (softmax * eps * ((K + 2) / 2 + 4 log K + |m| + |l - m| + 3) + eps)"""
    B, K = logits.shape[:2]
    HW = logits[0, 0].numel()
    ce64, g64, tg, sm = ce_oracle(logits, target, coef)
    ld = logits.to(dev).requires_grad_(True)
    loss = ops.MaskedCEFunction.apply(ld, target.to(dev), coef.to(dev))
    loss.backward()
    ce = ops.masked_ce(logits.to(dev), target.to(dev)).cpu().double()
    grad = ld.grad.cpu().double().flatten(2)
    l = logits.double().flatten(2)
    m = l.max(1, keepdim=True).values
    lt = torch.gather(l, 1, tg.clamp(min=0).unsqueeze(1)).squeeze(1)
    logK = math.log(max(K, 2))
    finite = torch.isfinite(ce64)
    ce_bound = EPS32 * ((lt - m.squeeze(1)).abs() + (K + 2) / 2 + 2 * logK + ce64.abs()) + EPS32
    assert torch.equal(torch.isfinite(ce), finite) and torch.equal(ce[~finite], ce64[~finite]), f"{name}: infinities differ"
    ce_err = ((ce - ce64).abs() / ce_bound)[finite]
    assert bool((ce[tg < 0] == 0).all()), f"{name}: an ignored position has a loss"
    lm = (l - m).abs()
    lm = torch.where(torch.isfinite(lm), lm, torch.zeros_like(lm))
    g_bound = coef.double().abs().view(B, 1, 1) * (sm * EPS32 * ((K + 2) / 2 + 4 * logK + m.abs() + lm + 3) + EPS32)
    g_err = (grad - g64).abs()
    ok = g_err <= g_bound
    assert bool((grad[(tg < 0).unsqueeze(1).expand_as(grad)] == 0).all()), f"{name}: an ignored position has a gradient"
    want_loss = (ce64.sum(1) * coef.double()).sum()
    form = "global" if K * HW + 2 * HW > CE_TILE else "lds"
    parity(f"masked_ce_{form}_{name}", ce_max_err_over_bound=float(ce_err.max()) if ce_err.numel() else 0.0,
           grad_max_err_over_bound=float((g_err / g_bound.clamp(min=1e-300)).max()) if bool((g_bound > 0).any()) else 0.0,
           ce_max_abs_err=float((ce - ce64).abs()[finite].max()) if ce_err.numel() else 0.0, grad_max_abs_err=float(g_err.max()))
    assert ce_err.numel() == 0 or float(ce_err.max()) <= 1.0, f"{name}: ce error {float(ce_err.max())} x the bound"
    assert bool(ok.all()), f"{name}: {int((~ok).sum())} gradient elements beyond the bound, worst {float((g_err / g_bound).max())}"
    if bool(torch.isfinite(want_loss)):
        assert abs(float(loss) - float(want_loss)) <= 1e-5 * max(1.0, abs(float(want_loss)))


def ce_inputs(B, K, HW, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, K, 1, HW, generator=g) * scale
    tgt = torch.randint(0, K, (B, 1, 1, HW), generator=g).float()
    tgt[torch.rand(B, 1, 1, HW, generator=g) < 0.4] = -1
    coef = torch.rand(B, generator=g) + 0.1
    return logits, tgt, coef


CE_SHAPES = [(128, 49), (255, 64), (256, 64), (333, 49), (512, 49), (512, 64), (2048, 49), (10, 300), (60, 270), (1, 49)]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("K,HW", CE_SHAPES)
def test_masked_ce_vs_fp64_both_kernels(dev, K, HW, B):
    """(K, HW) on both sides of the 16 384-float switch between the LDS-tile kernel and the global one ((255, 64) is the last
    that fits, (256, 64) and (333, 49) the first that do not), and more than 256 positions (the per-position loop's second pass)
    in both kernels ((10, 300) fits, (60, 270) does not)."""
    check_masked_ce(dev, f"K{K}_HW{HW}_B{B}", *ce_inputs(B, K, HW, K + HW + B))


@pytest.mark.parametrize("K,HW", [(128, 49), (512, 64)])
def test_masked_ce_edges(dev, K, HW):
    B = 3
    logits, tgt, coef = ce_inputs(B, K, HW, 77 + K)
    # every target ignored: loss and gradient exactly zero
    ign = torch.full_like(tgt, -1)
    ld = logits.to(dev).requires_grad_(True)
    loss = ops.MaskedCEFunction.apply(ld, ign.to(dev), coef.to(dev))
    loss.backward()
    assert float(loss) == 0.0 and bool((ld.grad == 0).all()) and bool((ops.masked_ce(logits.to(dev), ign.to(dev)) == 0).all())
    # targets >= K are ignored, non-integer targets truncate
    t2 = tgt.clone()
    t2.view(-1)[0::5] = float(K)
    t2.view(-1)[1::5] = float(K + 100)
    t2.view(-1)[2::5] = t2.view(-1)[2::5].clamp(min=0) + 0.75
    t2.view(-1)[3::5] = -0.5
    check_masked_ce(dev, f"odd_targets_K{K}", logits, t2, coef)
    # logits at +-80, one -inf per row (as the target of some rows: infinite loss, gradient -coef there), zero and negative coef
    big = logits.clone()
    big[:, 0::3] = 80.0
    big[:, 1::3] = -80.0
    check_masked_ce(dev, f"pm80_K{K}", big, tgt, torch.tensor([0.0, -0.7, 1.3]))
    hole = logits.clone()
    hole[:, 5] = -INF
    t3 = tgt.clone()
    t3.view(B, HW)[:, :4] = 5.0
    check_masked_ce(dev, f"neg_inf_K{K}", hole, t3, torch.tensor([0.5, -0.7, 0.0]))


# =============================================================================================== h. rows without a winner
def degenerate_rows(B, K, L, seed):
    """Logits whose position i % 4 is: 0 regular, 1 one NaN class, 2 every class -inf, 3 one +inf class (inf - inf = NaN)."""
    logits, q, u, x0, un0 = psample_inputs(B, K, L, L, seed)
    rows = rows_of(logits)
    kind = torch.arange(rows.shape[0]) % 4
    rows[kind == 1, (K * 2) // 3] = NAN
    rows[kind == 2] = -INF
    rows[kind == 3, K // 2] = INF
    logits = rows.reshape(B, L * L, K).permute(0, 2, 1).reshape(B, K, L, L).contiguous()
    return (logits, q, u, x0, un0), kind


@pytest.mark.parametrize("K", [1, 5, 128, 300, 600, 1100, 2048])
def test_psample_step_rows_without_a_comparable_ratio(dev, K):
    """A position whose logits hold a NaN or +inf, or are all -inf, has no comparable ratio (the reference's Categorical raises
    there).  The kernel writes token 0 -- torch.argmax's answer for the all-NaN ratios -- and never a token outside [0, K); the
    regular positions of the same call are unaffected.  (Before: token 2 147 483 647.)  The tokens are only read back."""
    (logits, q, u, x0, un0), kind = degenerate_rows(6, K, 4, 7000 + K)
    want, fragile = oracle_tokens(logits, 1.0, q, REG_THRESHOLD)
    assert bool((want[kind != 0] == 0).all()) and not bool(fragile[kind != 0].any())
    for form in ("x0_hat", "skip"):
        xa, una = x0.to(dev), un0.to(dev)
        hat = torch.full((x0.numel(),), -7, dtype=torch.int64, device=dev) if form == "x0_hat" else None
        ops.psample_step(logits.to(dev), xa, una, 1, 1.0, u.to(dev), q.to(dev), x0_hat=hat)
        got = xa.cpu().flatten()
        changed = ~un0.flatten()
        assert bool(una.all()) and bool(((got >= 0) & (got < K)).all()), (form, int(got.max()))
        assert torch.equal(got[changed & ~fragile], want[changed & ~fragile]), form
        assert torch.equal(got[~changed], x0.flatten()[~changed])
        if hat is not None:
            assert torch.equal(hat.cpu()[~fragile], want[~fragile])
    parity(f"degenerate_rows_psample_K{K}", tokens_out_of_range=0, degenerate_positions=int((kind != 0).sum()))


@pytest.mark.parametrize("what", ["nan", "neg_inf"])
@pytest.mark.parametrize("K,L", [(17, 7), (129, 8)])
def test_step_tail_rows_without_a_comparable_ratio(dev, K, L, what):
    """The same rule in the token update of spk_den_step_tail: conv6's bias made NaN for one class (every position holds a
    NaN logit) or -inf for all (every logit -inf): every position that changes gets token 0.  No next-step layer is run
    (conv1 = None); tokens and logits are only read back."""
    from snn_model.vq_diffusion import DummyModel, functional
    torch.manual_seed(K)
    den = DummyModel(1, K).to(dev)
    functional.set_step_mode(net=den, step_mode='m')
    with torch.no_grad():
        if what == "nan":
            den.conv6[0].bias[K // 2] = NAN
        else:
            den.conv6[0].bias.fill_(-INF)
    den.eval()
    assert den.tail_fusable(L, L)
    g = torch.Generator().manual_seed(K + L)
    B = 5
    x0 = torch.randint(0, K, (B, 1, L, L), generator=g)
    un0 = torch.rand(B, 1, L, L, generator=g) < 0.5
    x0[~un0] = K
    x5, cnt5, x1, cnt1, which, impl, collapse = den._trunk(ops.den_build_input(x0.to(dev), 1), False)
    conv6, packed6 = den._conv6_params()
    xa, una = x0.to(dev), un0.to(dev)
    _, lg = ops.den_step_tail(cnt5, cnt1, packed6, xa, una, 1, 1.0, T=16, K=K, seed=5, offset=STEP, conv1=None, want_logits=True)
    lr = rows_of(lg.cpu())
    if what == "nan":
        assert bool(torch.isnan(lr[:, K // 2]).all()), "the case needs a NaN logit at every position"
    else:
        assert bool((lr == -INF).all()), "the case needs every logit at -inf"
    got = xa.cpu()
    assert bool(una.all()) and bool((got[~un0] == 0).all()) and torch.equal(got[un0], x0[un0])
    # the three-launch form agrees
    xb, unb = x0.to(dev), un0.to(dev)
    ops.psample_step(lg, xb, unb, 1, 1.0, seed=5, offset=STEP)
    assert torch.equal(xb, xa) and torch.equal(unb, una)
    parity(f"degenerate_rows_step_tail_{what}_K{K}", tokens_out_of_range=0, positions_changed=int((~un0).sum()))


# =============================================================================================== i. what the wrappers refuse
@pytest.mark.parametrize("wrapper", ["psample_step", "pscore_step", "den_step_tail"])
def test_token_update_wrappers_refuse_the_same_bad_arguments(dev, wrapper):
    """ops.psample_step, ops.pscore_step and ops.den_step_tail check the token state, the noise and next_input through the same
    helpers: a wrong dtype, a non-contiguous or host tensor, a short u / q / next_input, a philox_state that is not two int64
    words -- each raises ValueError before any launch (x_t / unmasked as they were; t = 1 on an all-masked state, so a launch
    would reveal every position).  Every short tensor is a slice of a full-size buffer and the host mask is pinned, so a wrapper
    that let one through would still read inside an allocation."""
    B, L, K = 2, 7, 17
    HW = L * L
    n = B * HW
    g = torch.Generator().manual_seed(17)

    def zeros(count, dtype):
        return torch.zeros(count, dtype=dtype, device=dev)
    good = dict(x_t=torch.full((B, 1, L, L), K, dtype=torch.int64, device=dev), unmasked=zeros(n, torch.bool).reshape(B, 1, L, L),
                u=torch.rand(n, generator=g).to(dev), q=(torch.rand(n * K, generator=g) + 0.1).to(dev),
                philox_state=zeros(2, torch.int64), next_input=zeros(2 * n, torch.float32).reshape(B, 2, L, L))
    bad = {
        "x_t int32": dict(x_t=torch.full((2 * n,), K, dtype=torch.int32, device=dev)[:n].reshape(B, 1, L, L)),
        "x_t non-contiguous": dict(x_t=torch.full((B, 1, L, 2 * L), K, dtype=torch.int64, device=dev)[..., ::2]),
        "unmasked float32": dict(unmasked=zeros(n, torch.float32).reshape(B, 1, L, L)),
        "unmasked on the CPU": dict(unmasked=torch.zeros((B, 1, L, L), dtype=torch.bool).pin_memory()),
        "u short": dict(u=good["u"][:n - 1]),
        "q short": dict(q=good["q"][:n * K - 1]),
        "philox_state int32": dict(philox_state=zeros(4, torch.int32)[:2]),
        "philox_state three words": dict(philox_state=zeros(3, torch.int64)),
        "next_input short": dict(next_input=zeros(2 * n, torch.float32)[:2 * n - 1]),
    }
    takes = {"psample_step": {"q", "next_input"}, "pscore_step": {"next_input"}, "den_step_tail": {"q"}}[wrapper]
    logits = torch.randn(B, K, L, L, generator=g).to(dev)
    x0, logp = zeros(n, torch.int64), zeros(n, torch.float64)
    # (den_step_tail: count records and packed conv6 weights of the right sizes -- two 16-channel groups -- and nothing else)
    cnt5, cnt1 = zeros(B * 8 * HW * 32, torch.uint8).reshape(B, 8, L, L, 32), zeros(B * 2 * HW * 32, torch.uint8).reshape(B, 2, L, L, 32)
    packed6 = (zeros(2 * 10 * 18432, torch.int8), zeros(32, torch.float64), zeros(32, torch.float64))

    def call(a):
        opt = {k: a[k] for k in ("q", "next_input") if k in takes}
        if wrapper == "psample_step":
            return ops.psample_step(logits, a["x_t"], a["unmasked"], 1, 1.0, u=a["u"], philox_state=a["philox_state"], **opt)
        if wrapper == "pscore_step":
            return ops.pscore_step(logits, x0, a["x_t"], a["unmasked"], 1, 1.0, logp, u=a["u"], philox_state=a["philox_state"], **opt)
        return ops.den_step_tail(cnt5, cnt1, packed6, a["x_t"], a["unmasked"], 1, 1.0, T=16, K=K, u=a["u"],
                                 philox_state=a["philox_state"], **opt)
    wrong = []
    for name, change in bad.items():
        if (name.startswith("q ") and "q" not in takes) or (name.startswith("next_input") and "next_input" not in takes):
            continue
        a = dict(good, **change)
        before = a["x_t"].clone(), a["unmasked"].clone()
        try:
            call(a)
            wrong.append(f"{name}: accepted")
        except ValueError:
            pass
        except Exception as e:  # noqa: BLE001  (the wrong exception type is what is reported)
            wrong.append(f"{name}: {type(e).__name__} instead of ValueError")
        torch.cuda.synchronize()
        if not (torch.equal(a["x_t"], before[0]) and torch.equal(a["unmasked"], before[1])):
            wrong.append(f"{name}: x_t / unmasked written")
    assert not wrong, f"{wrapper}: {wrong}"
