"""The host oracle of tests/test_gpu_conv_bn_lif_oracle.py, checked on the CPU: its single-rounding fma against exact rational
arithmetic, and the CONDITIONS ON THE INPUTS that let the GPU tests demand bit-equality with nothing excluded -- every row's fp64
convolution is the same bits in any summation order, its spike rate is in a useful band, and the tables hold neuron-steps whose
charged potential equals the threshold exactly."""
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
