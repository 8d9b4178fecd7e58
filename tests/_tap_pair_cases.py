"""Inputs of tests/test_gpu_fp6v2_tap_pairs.py (CPU only: torch tensors on the host), and a host restatement of the layer
(conv 3x3 + BN + LIF from a fresh state, fp64) that tests/test_tap_pair_cases_host.py uses to show that every generator yields what its
name says and a firing rate strictly between 0 and 1 -- a case that fires nowhere or everywhere checks nothing.

The full-item form of spk_den_conv3x3_mfma_fp6v2 puts two adjacent TAPS of one weight digit into the K halves of an MFMA
(den_mfma_fp6v2.hip, "TAP PAIRS"): lanes 0-31 read the input cell of tap a, lanes 32-63 that of tap a + 1; the B operand is one half of
the packed tile (a, pair) and one half of tile (a + 1, pair); the scale is 2^8 for digits 0 and 2, 2^3 for digits 1 and 3.
  one tap      weights non-zero in a single tap: a swapped lane half or a wrong tap distance reads the neighbouring tap
  one digit    every weight a single non-zero radix-32 digit j of the 29-bit fixed-point value (tests/_fp6_tiles_oracle.py: quantise,
               digits), signs by tap: a wrong scale or the wrong half-tile slot (even / odd digit) moves every pre-activation.  The
               quantisation scale follows the largest weight of an output channel, so input channel 0 carries one weight of 0.5 (digit 0
               alone, sh = 29) in every output channel and never spikes.
  cells        spikes only on the border, only in the interior, in ONE corner cell of ONE image, everywhere."""
import torch

B = 3
COUTS = (32, 64)
CINS = (32, 64, 96)          # one, two and three K chunks per item
SHAPES = tuple((co, ci) for co in COUTS for ci in CINS)
CORNERS = ((0, 0), (0, 6), (6, 0), (6, 6))
TAP_SIGNS = (1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0, 1.0)      # six taps up, three down: every tap pair but (7, 8) is mixed or not


def layer_random(Cout, Cin, seed=0):
    """(w, bias, bn_a, bn_b): the layer of the border-skip and copy-roles tests."""
    g = torch.Generator().manual_seed(7100 + 7 * Cout + Cin + seed)
    w = (torch.rand(Cout, Cin, 3, 3, generator=g) - 0.5) * 0.05
    w[:, :, 1, 1] *= 3.0
    bias = (torch.rand(Cout, generator=g) - 0.5) * 0.2
    a = (torch.rand(Cout, generator=g) - 0.3) * 12.0                  # some negative BN scales
    b = (torch.rand(Cout, generator=g) - 0.4) * 1.5
    return w, bias, a, b


def layer_one_tap(Cout, Cin, tap):
    """Weights in tap `tap` alone, nine times as large as layer_random's (one tap carries the pre-activation of nine)."""
    w, bias, a, b = layer_random(Cout, Cin, seed=tap + 1)
    keep = torch.zeros(9)
    keep[tap] = 9.0
    return w * keep.view(1, 1, 3, 3), bias, a, b


def layer_one_digit(Cout, Cin, j):
    """Every weight of input channels 1.. is TAP_SIGNS[tap] * d * 32^(5 - j) * 2^-29 with d in 8 .. 15 by output channel: digit j alone.
    BN scales the pre-activation of the interior (0.3 x 6 - 3 taps x (Cin - 1) inputs x d) to 1.5 .. 3; no bias."""
    assert 0 <= j <= 3
    d = 8.0 + (torch.arange(Cout) % 8).float()
    unit = float(32 ** (5 - j)) * 2.0 ** -29
    w = torch.tensor(TAP_SIGNS).view(1, 1, 3, 3) * d.view(Cout, 1, 1, 1) * unit * torch.ones(Cout, Cin, 3, 3)
    w[:, 0] = 0.0
    w[:, 0, 1, 1] = 0.5
    est = 0.3 * 3.0 * (Cin - 1) * d * unit
    a = (1.5 + 1.5 * ((torch.arange(Cout) * 5) % 7).float() / 6.0) / est
    return w, torch.zeros(Cout), a, torch.zeros(Cout)


def border_mask():
    m = torch.zeros(7, 7, dtype=torch.bool)
    m[0, :] = m[6, :] = m[:, 0] = m[:, 6] = True
    return m


def spikes_random(Cin, rate, seed, cells=None, only=None, silent0=False):
    """[16, B, Cin, 7, 7] 0/1 at `rate`, on `cells` (bool [7, 7]) of image `only` (or of all); silent0: input channel 0 never spikes."""
    g = torch.Generator().manual_seed(7300 + seed)
    s = (torch.rand(16, B, Cin, 7, 7, generator=g) < rate).float()
    if cells is not None:
        s = s * cells.float()
    if only is not None:
        keep = torch.zeros(B)
        keep[only] = 1.0
        s = s * keep.view(1, B, 1, 1, 1)
    if silent0:
        s[:, :, 0] = 0.0
    return s


def cell_cases():
    """(name, cells, rate, the one active image or None): border / interior / one corner cell of one image (first, first, middle, last)."""
    border = border_mask()
    out = [("border", border, 0.30, None), ("interior", ~border, 0.30, None)]
    for k, (y, x) in enumerate(CORNERS):
        cell = torch.zeros(7, 7, dtype=torch.bool)
        cell[y, x] = True
        out.append((f"corner{k}", cell, 0.5, (k * (B - 1)) // 3))
    return out


def host_layer(spikes, layer):
    """fp64 restatement: spikes [16, B, Cin, 7, 7] -> output spikes [16, B, Cout, 7, 7] (h = v + (z - v) / 2, spike and reset at h >= 1)."""
    w, bias, a, b = (t.double() for t in layer)
    T, Bn = spikes.shape[:2]
    z = torch.nn.functional.conv2d(spikes.double().flatten(0, 1), w, bias, padding=1)
    z = (z * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)).view(T, Bn, -1, 7, 7)
    v = torch.zeros_like(z[0])
    out = []
    for t in range(T):
        h = v + (z[t] - v) / 2
        s = h >= 1.0
        v = torch.where(s, torch.zeros_like(h), h)
        out.append(s.float())
    return torch.stack(out)
