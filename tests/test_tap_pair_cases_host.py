"""The generators of tests/_tap_pair_cases.py yield what tests/test_gpu_fp6v2_tap_pairs.py relies on (no GPU): single taps, single
radix-32 digits under the packer's quantisation (tests/_fp6_tiles_oracle.py), border / interior / corner cells, and -- through the
fp64 restatement of the layer -- a firing rate strictly between 0 and 1 for every case the GPU test runs."""
import numpy as np
import pytest
import torch

import _fp6_tiles_oracle as F
import _tap_pair_cases as C


def _rate(spikes, layer):
    return float(C.host_layer(spikes, layer).mean())


@pytest.mark.parametrize("Cout,Cin", C.SHAPES)
def test_one_tap_layers_hold_one_tap_and_fire(Cout, Cin):
    s = C.spikes_random(Cin, 0.30, Cin)
    for tap in range(9):
        layer = C.layer_one_tap(Cout, Cin, tap)
        w = layer[0].reshape(Cout, Cin, 9)
        assert bool((w[:, :, tap] != 0).all()) and int((w != 0).sum()) == Cout * Cin
        assert 0.0 < _rate(s, layer) < 1.0, tap


@pytest.mark.parametrize("Cout,Cin", C.SHAPES)
def test_one_digit_layers_hold_one_digit_and_fire(Cout, Cin):
    s = C.spikes_random(Cin, 0.30, 100 + Cin, silent0=True)
    assert float(s[:, :, 0].sum()) == 0.0
    for j in range(4):
        layer = C.layer_one_digit(Cout, Cin, j)
        q, sh, _ = F.quantise(layer[0].numpy())
        assert (sh == 29).all()
        dg = F.digits(q)                                           # [6][Cout][9][Cin]
        rest = np.delete(dg[:, :, :, 1:], j, axis=0)
        assert not rest.any() and (dg[j, :, :, 1:] != 0).all(), "input channels 1..: digit j alone, everywhere"
        assert (np.sign(dg[j, :, :, 1]) == np.sign(np.array(C.TAP_SIGNS))[None, :]).all() and len(set(C.TAP_SIGNS)) == 2
        assert (np.abs(dg[j, :, 0, 1]) == 8 + np.arange(Cout) % 8).all()
        assert 0.0 < _rate(s, layer) < 1.0, j


def test_cell_cases_cover_border_interior_and_the_four_corners():
    cases = C.cell_cases()
    assert [c[0] for c in cases] == ["border", "interior", "corner0", "corner1", "corner2", "corner3"]
    assert int(cases[0][1].sum()) == 24 and int(cases[1][1].sum()) == 25 and not bool((cases[0][1] & cases[1][1]).any())
    assert [c[3] for c in cases[2:]] == [0, 0, 1, 2]
    for Cout in C.COUTS:
        layer = C.layer_random(Cout, 64)
        for k, (name, cells, rate, only) in enumerate(cases):
            s = C.spikes_random(64, rate, 200 + k, cells=cells, only=only)
            assert float((s * (~cells).float()).sum()) == 0.0 and float(s.sum()) > 0.0
            if only is not None:
                assert float(s.sum()) == float(s[:, only].sum()) and int(cells.sum()) == 1
            assert 0.0 < _rate(s, layer) < 1.0, (Cout, name)


@pytest.mark.parametrize("Cout", C.COUTS)
def test_remaining_cases_fire(Cout):
    assert 0.0 < _rate(torch.ones(16, C.B, 96, 7, 7), C.layer_random(Cout, 96)) < 1.0          # every input active
    layer = C.layer_random(Cout, 64)
    s = C.spikes_random(64, 0.30, 300)
    assert 0.0 < float(C.host_layer(s, layer)[:, :2].mean()) < 1.0                               # image count 2 of 3
    for Cin in C.CINS:
        assert 0.0 < _rate(C.spikes_random(Cin, 0.30, 400 + Cin), C.layer_random(Cout, Cin)) < 1.0
