"""The host oracle of tests/test_gpu_conv_bn_lif_oracle.py, checked on the CPU: its single-rounding fma against exact rational
arithmetic, and the CONDITIONS ON THE INPUTS that let the GPU tests demand bit-equality with nothing excluded -- every row's fp64
convolution is the same bits in any summation order, its spike rate is in a useful band, and the tables hold neuron-steps whose
charged potential equals the threshold exactly.  The FULL-WIDTH rows (the denoiser's matrix-core family and the second pass over the
gather / vae_fp6 rows) add: the weights are exact in both fixed-point formats with the low digits in play, and the threshold-grazing
neurons are what they were built to be."""
import numpy as np
import pytest
import torch

import _conv_bn_lif_oracle as O
from oracle import snn_ref as ref

ROWS = O.all_spike_rows()


def _rid(r):
    return f"{r[0]}-" + "-".join(str(int(v)) for v in r[1]) + f"-T{r[3]}"


def test_fma32_is_the_single_rounding_fma_where_double_rounding_is_not():
    """4000 triples on the ties of the naive form's second rounding: fma32 (and the oracle module's torch form) equal exact
    rational arithmetic everywhere; the naive double-rounding form does not (the set is adversarial)."""
    x, a, b = O.fma_tie_set(4000, seed=1)
    want = O.fma32_exact(x, a, b)
    got = O.fma32(x, a, b)
    naive = O.fma32_naive(x, a, b)
    assert int((got.view(np.uint32) != want.view(np.uint32)).sum()) == 0
    n_naive = int((naive.view(np.uint32) != want.view(np.uint32)).sum())
    assert n_naive >= 100, f"the tie set does not defeat double rounding ({n_naive} of 4000)"
    tx, ta, tb = (torch.from_numpy(v) for v in (x, a, b))
    assert torch.equal(ref.fma_f32(tx, ta, tb), torch.from_numpy(want))
    assert torch.equal(O.fma32(tx, ta, tb), torch.from_numpy(want))


def test_fma32_on_random_triples():
    rng = np.random.default_rng(2)
    n = 3000
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-6, 6, n))).astype(np.float32)
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-3, 3, n))).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-6, 6, n))).astype(np.float32)
    b[::7] = (-x[::7].astype(np.float64) * a[::7].astype(np.float64)).astype(np.float32)       # cancellation
    want = O.fma32_exact(x, a, b)
    assert int((O.fma32(x, a, b).view(np.uint32) != want.view(np.uint32)).sum()) == 0
    assert torch.equal(ref.fma_f32(torch.from_numpy(x), torch.from_numpy(a), torch.from_numpy(b)), torch.from_numpy(want))


def _frames(c):
    """[N,Cin,H,W] frames of a case (all steps of a sequence, or the one frame of a time-invariant row)."""
    return c.x if c.kind == "pixels" else c.x.flatten(0, 1)


@pytest.mark.parametrize("row", ROWS, ids=_rid)
def test_row_is_exact_in_any_order_and_fires_at_a_useful_rate(row):
    name, geo, kind, T = row
    c = O.make_case(geo, O.row_seed(geo, T), kind=kind, T=T)
    Cin, tr = geo[0], geo[5]
    x = _frames(c)
    y = O.conv64(x, c.w, c.bias, geo)
    # a channel permutation and a flip of the tap order change the order of every partial sum, not the sum
    perm = torch.randperm(Cin, generator=torch.Generator().manual_seed(7))
    wp = c.w[perm] if tr else c.w[:, perm]
    assert torch.equal(O.conv64(x[:, perm], wp, c.bias, geo), y), "fp64 convolution depends on the channel order"
    # the taps added one by one from the last to the first (each tap's channel sum by torch, the taps' sum here)
    assert torch.equal(_conv_taps_reversed(x, c.w, c.bias, geo), y), "fp64 convolution depends on the tap order"
    assert torch.equal(y.float().double(), y) or kind == "seq"      # (spike / pixel rows: even the fp32 rounding is exact)
    xs = c.x if kind != "pixels" else c.x.unsqueeze(0).repeat(T, 1, 1, 1, 1)
    spk, _, _ = O.conv_bn_lif(xs, c.w, c.bias, c.a, c.b, None, geo)
    rate = float(spk.mean())
    assert 0.02 <= rate <= 0.6, rate
    assert bool((c.a < 0).any()) or geo[1] < 8


def _conv_taps_reversed(x, w, bias, geo):
    """The convolution as the sum of its k * k single-tap convolutions, added from the LAST tap to the first, bias last."""
    k = geo[2]
    acc = None
    for ky in reversed(range(k)):
        for kx in reversed(range(k)):
            wt = torch.zeros_like(w)
            wt[:, :, ky, kx] = w[:, :, ky, kx]
            term = O.conv64(x, wt, None, geo)
            acc = term if acc is None else acc + term
    return acc + bias.double().view(1, -1, 1, 1)


def test_tables_hold_potentials_exactly_on_the_threshold():
    """h == 1.0 fires (>=): a kernel that tested > would differ exactly there.  Each row of O.TIE_ROWS (one per gather kernel shape:
    three compile-time instances and two generic geometries) holds such a neuron-step from the reset state."""
    for geo in O.TIE_ROWS:
        c = O.make_case(geo, O.row_seed(geo))
        n = O.threshold_ties(O.bn32(O.conv_fp32(c.x, c.w, c.bias, geo), c.a, c.b))
        assert n >= 1, geo


@pytest.mark.parametrize("geo", [O.GATHER_ROWS[0], O.GATHER_ROWS[10]], ids=["enc2", "3x3s1"])
def test_agrees_with_conv_bn_lif_exact_on_plain_rows(geo):
    """The new oracle against ref.conv_bn_lif_exact (BN terms from running statistics through ref.bn_affine_terms)."""
    c = O.make_case(geo, O.row_seed(geo))
    Cout = geo[1]
    g = torch.Generator().manual_seed(5)
    sd = {"c.weight": c.w, "c.bias": c.bias, "b.weight": torch.rand(Cout, generator=g) + 0.5, "b.bias": torch.rand(Cout, generator=g) - 0.3,
          "b.running_mean": torch.rand(Cout, generator=g) - 0.5, "b.running_var": torch.rand(Cout, generator=g) + 0.5}
    a, b = ref.bn_affine_terms(sd, "b")
    want_s, want_y = ref.conv_bn_lif_exact(c.x, sd, "c", "b", geo[3], geo[4])
    s, _, y = O.conv_bn_lif(c.x, c.w, c.bias, a, b, None, geo)
    assert torch.equal(s, want_s) and torch.equal(O.bn32(y, a, b), want_y)
    assert 0.0 < float(s.mean()) < 1.0


def test_packed_layout_helpers_round_trip():
    g = torch.Generator().manual_seed(3)
    s = (torch.rand(16, 2, 64, 3, 5, generator=g) < 0.3).float()
    bits = O.spikes_to_bits(s)
    assert torch.equal(O.bits_to_ptc(bits), O.to_ptc(s)) and torch.equal(O.from_ptc(O.to_ptc(s)), s)
    s32 = O.bits_to_packed(bits, 32)
    assert s32.shape == (2, 2, 3, 5, 16, 16)
    # record (b, chunk 1, y 2, x 4, t 5): byte j holds channels 32 + 2j (low nibble) and 32 + 2j + 1 (high nibble), 1.0 = 0x2
    want = [int(s[5, 1, 32 + 2 * j, 2, 4]) * 2 + int(s[5, 1, 33 + 2 * j, 2, 4]) * 32 for j in range(16)]
    assert s32[1, 1, 2, 4, 5].tolist() == want
    assert O.bits_to_packed(bits, 64).shape == (2, 1, 3, 5, 16, 32)
    assert torch.equal(O.to_ptc(s, 4)[1, 3, 2, 4, 5], s[5, 1, 12:16, 2, 4].to(torch.uint8))


def test_bn_scale_of_the_oracle_is_correctly_rounded():
    """ref.bn_affine_terms evaluates a = (1 / sqrt(var + eps)) * gamma with every operation correctly rounded (exact rational checks of
    the root's and the quotient's rounding intervals), whatever the tensor library's fp32 sqrt does."""
    from fractions import Fraction
    g = torch.Generator().manual_seed(4)
    var = torch.rand(2000, generator=g) * 0.5 + 0.5
    r = np.sqrt(var.numpy().astype(np.float64)).astype(np.float32)
    inv = ref._inv_sqrt_f32(var).numpy()
    for x, ri, qi in zip(var.numpy(), r, inv):
        lo = (Fraction(float(ri)) + Fraction(float(np.nextafter(ri, np.float32(0))))) / 2
        hi = (Fraction(float(ri)) + Fraction(float(np.nextafter(ri, np.float32(2))))) / 2
        assert lo * lo <= Fraction(float(x)) <= hi * hi
        assert qi == O.round_fraction_f32(1 / Fraction(float(ri)))
    sd = {"b.weight": torch.rand(2000, generator=g) + 1.0, "b.bias": torch.rand(2000, generator=g), "b.running_var": var - ref.BN_EPS,
          "b.running_mean": torch.rand(2000, generator=g) - 0.5}
    a, b = ref.bn_affine_terms(sd, "b")
    assert torch.equal(a, ref._inv_sqrt_f32(sd["b.running_var"] + ref.BN_EPS) * sd["b.weight"])
    want_b = O.fma32_exact((-sd["b.running_mean"]).numpy(), a.numpy(), sd["b.bias"].numpy())
    assert torch.equal(b, torch.from_numpy(want_b))


# ================================================================================================ full-width rows
FULL_ROWS = [(f"den_{fam}", O.den_geo(r)) for fam, r in O.all_den_rows()]
FULL_ROWS += [("gather_full", g) for g in O.GATHER_FULL_ROWS] + [("vae_fp6_full", O.vae_fp6_geo(r, B)) for r in O.VAE_FP6_ROWS for B in (1, 5)]
_FULL = {}


def _full(geo):
    if geo not in _FULL:
        c = O.make_case(geo, O.full_seed(geo), weights="full")
        c.y = O.conv_fp32(c.x, c.w, c.bias, geo)
        c.z = O.bn32(c.y, c.a, c.b)
        c.s, _ = ref.lif_multi_step(c.z)
        _FULL[geo] = c
    return _FULL[geo]


def _fid(r):
    return f"{r[0]}-" + "-".join(str(int(v)) for v in r[1])


def test_full_width_weights_are_refused_for_real_valued_inputs():
    for kind in ("seq", "pixels"):
        with pytest.raises(ValueError):
            O.make_case(O.SEQ_ROWS[0], 1, kind=kind, weights="full")


def test_default_scheme_is_unchanged_by_the_weights_option():
    geo = O.GATHER_ROWS[0]
    c0, c1 = O.make_case(geo, 5), O.make_case(geo, 5, weights="dyadic12")
    assert all(torch.equal(getattr(c0, k), getattr(c1, k)) for k in ("w", "bias", "a", "b", "v0", "x"))
    assert torch.equal(c0.w * 4096, (c0.w * 4096).round()) and float(c0.w.abs().max()) < 0.5


@pytest.mark.parametrize("row", FULL_ROWS, ids=_fid)
def test_full_width_row_fills_every_digit_and_is_exact_in_any_order(row):
    name, geo = row
    Cin, Cout, tr = geo[0], geo[1], geo[5]
    c = _full(geo)
    w_oc = (c.w.transpose(0, 1) if tr else c.w).double()                    # [Cout, Cin, k, k]
    e = O.channel_exponent(c.w, tr)
    assert torch.equal(e, c.e), "the pack kernels' frexp exponent is the exponent the channel was drawn with"
    q29 = w_oc * torch.exp2((29 - e).double()).view(-1, 1, 1, 1)
    q30 = w_oc * torch.exp2((30 - e).double()).view(-1, 1, 1, 1)
    assert torch.equal(q29, torch.round(q29)) and torch.equal(q30, torch.round(q30)), "a weight is not exact in the kernels' fixed point"
    assert float(q29.abs().max()) < 2.0 ** 29 and float(q29.abs().min()) >= 16.0
    low5 = float((torch.remainder(q29.abs(), 32.0) != 0).double().mean())
    assert low5 >= 0.5, low5                                                # the sixth radix-32 digit (and the low int8 digit) is in play
    assert float((torch.remainder(q30.abs(), 256.0) != 0).double().mean()) >= 0.5
    x = c.x.flatten(0, 1)
    y = O.conv64(x, c.w, c.bias, geo)
    perm = torch.randperm(Cin, generator=torch.Generator().manual_seed(7))
    wp = c.w[perm] if tr else c.w[:, perm]
    assert torch.equal(O.conv64(x[:, perm], wp, c.bias, geo), y), "fp64 convolution depends on the channel order"
    assert torch.equal(_conv_taps_reversed(x, c.w, c.bias, geo), y), "fp64 convolution depends on the tap order"
    rate = float(c.s.mean())
    assert 0.02 <= rate <= 0.6, rate
    assert bool((c.a < 0).any()) or Cout < 8
    assert float((y.float().double() != y).double().mean()) > 0.5, "the one rounding to fp32 has nothing to round"


@pytest.mark.parametrize("row", FULL_ROWS, ids=_fid)
def test_full_width_row_grazes_the_threshold_where_it_was_built_to(row):
    name, geo = row
    c = _full(geo)
    fire = [g for g in c.graze if g[0] == "fire"]
    below = [g for g in c.graze if g[0] == "below"]
    assert O.threshold_ties(c.z) >= len(fire)
    h0 = O.lif_h0(c.z[0])
    for _, ch, b, y, x in fire:
        assert float(c.a[ch]) == 1.0 and float(h0[b, ch, y, x]) == 1.0 and float(c.s[0, b, ch, y, x]) == 1.0
    one = torch.ones(1)
    for _, ch, b, y, x in below:
        yv = c.y[0, b, ch, y, x].reshape(1)
        h = float(O.lif_h0(O.fma32(yv, one, c.b[ch].reshape(1))))
        b_up = torch.from_numpy(np.nextafter(c.b[ch].reshape(1).numpy(), np.float32(np.inf)))
        assert h < 1.0 and float(c.s[0, b, ch, y, x]) == 0.0 and float(h0[b, ch, y, x]) == h
        assert float(O.lif_h0(O.fma32(yv, one, b_up))) >= 1.0, "a larger b stays below the threshold"
        assert h == float(np.nextafter(np.float32(1.0), np.float32(0.0))), h     # z is the largest fp32 below 2
    if name.startswith("den_") and geo[9] * c.Ho * c.Wo >= 49:           # (the few-tap transposed rows of the second pass have fewer)
        assert len(fire) >= geo[1] // 8 and len(below) >= 1, (len(fire), len(below))
    assert len(fire) >= 1 or geo[1] < 4


@pytest.mark.parametrize("row", [r for r in FULL_ROWS if r[0].startswith("den_")], ids=_fid)
def test_denoiser_rows_spread_the_built_neurons_over_the_launch_forms(row):
    """Position H*W - 1 of an odd map (the last-position launches) and positions below it, rows H/2 - 1 and H/2 of an even-height map
    (both row bands), image 0 and the last image."""
    name, geo = row
    H, W, B = geo[7], geo[8], geo[9]
    c = _full(geo)
    pos = {y * W + x for _, _, _, y, x in c.graze}
    rows_hit = {y for _, _, _, y, _ in c.graze}
    imgs = {b for _, _, b, _, _ in c.graze}
    if H * W >= 25:
        assert min(pos) < H * W - 1 and 0 in imgs and B - 1 in imgs
        if H % 2 == 0:
            assert H // 2 - 1 in rows_hit and H // 2 in rows_hit
        if (H * W) % 2:                                                  # an odd map: its last position has launches of its own
            assert any(g[0] == "fire" and g[3] * W + g[4] == H * W - 1 for g in c.graze)


@pytest.mark.parametrize("row", O.DEN_COUNTS_ROWS + [O.STEP_TAIL_ROW], ids=lambda r: "-".join(str(v) for v in r))
def test_counts_oracle_against_the_mean_of_the_per_step_outputs(row):
    """fp32(sum_t dot + T * bias) / T from the convolution of the COUNT tensor against the fp64 mean of the per-step conv_fp32 outputs.
    The two round differently: the counts form rounds the exact sum ONCE, the per-step outputs are rounded one by one, so a mean that
    happens to be representable can still sit one ulp from the rounding of the exact mean.  They must be EQUAL wherever no per-step
    output was rounded and the mean is representable -- every such element of the full-width case, and nearly every element of the same
    row on 2^-12 weights, whose per-step outputs are all exact -- and within readout_bound everywhere."""
    geo = O.den_geo(row)
    for weights in ("full", "dyadic12"):
        c = _full(geo) if weights == "full" else O.make_case(geo, O.row_seed(geo))
        y = O.conv_fp32(c.x, c.w, c.bias, geo)
        cnt = O.from_counts(O.to_counts(c.x))
        assert torch.equal(cnt, c.x.sum(0)) and int(cnt.max()) > 1
        got, got64 = O.counts_logits(cnt, c.w, c.bias, geo)
        y64 = O.conv64(c.x.flatten(0, 1), c.w, c.bias, geo).view(16, *got.shape)
        assert torch.equal(got64, y64.sum(0) / 16), "the convolution of the counts is the sum of the per-step convolutions"
        mean, mag = O.mean64(y)
        rep = (mean.float().double() == mean) & (y64 == y.double()).all(0)
        print(f"counts oracle {row} {weights}: no step rounded and the mean representable at {int(rep.sum())} of {rep.numel()}; "
              f"max |diff| {float((got.double() - mean).abs().max()):.3e}")
        assert bool(((got.double() - mean).abs() <= O.readout_bound(16, mag)).all())
        assert torch.equal(got.double()[rep], mean[rep])
        if weights == "dyadic12":
            assert int(rep.sum()) >= 0.9 * rep.numel(), int(rep.sum())


def test_host_builders_of_the_denoiser_layouts_round_trip():
    g = torch.Generator().manual_seed(11)
    s = (torch.rand(16, 3, 128, 3, 5, generator=g) < 0.3).float()
    cp = O.to_ptc(s, 32)
    assert cp.shape == (3, 4, 3, 5, 16, 32) and torch.equal(O.from_cptc(cp), s)
    assert torch.equal(cp[2, 3, 1, 4, 9], s[9, 2, 96:128, 1, 4].to(torch.uint8))
    bits = O.spikes_to_bits(s)
    for rec in (32, 64):
        assert torch.equal(O.packed_to_spikes(O.bits_to_packed(bits, rec)), s)
    cnt = O.to_counts(s)
    assert cnt.shape == (3, 4, 3, 5, 32) and int(cnt[1, 2, 2, 3, 7]) == int(s[:, 1, 71, 2, 3].sum())
    assert torch.equal(O.from_counts(cnt), s.sum(0))
    bad = O.bits_to_packed(bits, 32).clone()
    bad[0, 0, 0, 0, 0, 0] = 0x01
    with pytest.raises(AssertionError):
        O.packed_to_spikes(bad)
