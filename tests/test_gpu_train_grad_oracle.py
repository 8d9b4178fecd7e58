"""The denoiser's training gradient kernels against an EXACT host oracle (tests/_train_grad_oracle.py): csrc/conv_wgrad.hip
(spk_conv3x3_wgrad_bf16), csrc/conv_dgrad.hip (spk_conv3x3_dgrad_bf16, spk_conv3x3_dgrad_f16x2, spk_conv3x3_dgrad_f16x2_pack_multi
+ spk_conv3x3_dgrad_f16x2_prepacked) and csrc/conv_wgrad_small.hip (spk_conv3x3_wgrad_small).

These kernels promise a result that is exact up to fp32 accumulation: every operand split is exact, every product is exact, the
dropped cross products are stated in the source.  The cases are integer-valued data times powers of two whose every fp32 partial
sum is exact in any order and on which the dropped products are zero (the builders assert both; tests/test_train_grad_oracle_host.py
proves it with the reference alone), so every output has one answer: every comparison below is ``torch.equal`` with the fp64
operator's result, nothing excluded.

Image counts follow from the device's CU count through the launch-form predictors of the oracle module, so that each row reaches
the form it names on any device -- several images per split-K slice with a one-image last slice and empty slices behind it, two
column tiles per wave with a ragged last image group, a second image per wave of the small-input kernel -- and each predicted
form is checked against what the library itself reports (workspace sizes, the tile width recorded by the multi-layer pack)."""
import ctypes

import pytest
import torch

import _train_grad_oracle as O
from parity_report import record as parity

pytestmark = pytest.mark.gpu

CL = torch.channels_last
STATS = {}                   # family -> [values compared, mismatches, {row: predicted form}]
_CASES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from spkdiff._lib import lib as l
    return l


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _case(builder, *args):
    """A case and its oracle results: built once per session, shared, left unchanged."""
    key = (builder.__name__,) + args
    if key not in _CASES:
        _CASES[key] = builder(*args)
    return _CASES[key]


def _report(fam):
    st = STATS.setdefault(fam, [0, 0, {}])
    parity(f"train_grad_oracle_{fam}", values=st[0], mismatches=st[1], forms=st[2])


def _form(fam, row, form):
    STATS.setdefault(fam, [0, 0, {}])[2][row] = form
    _report(fam)


def _tally(fam, got, want, what):
    """torch.equal with the mismatch pattern in the message; counts into the family's parity record."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, tuple(got.shape), tuple(want.shape), got.dtype)
    bad = ~(got == want)                                                     # (a NaN counts as a mismatch)
    n_bad = int(bad.sum())
    st = STATS.setdefault(fam, [0, 0, {}])
    st[0] += want.numel()
    st[1] += n_bad
    _report(fam)
    assert n_bad == 0, (what, f"{n_bad} of {want.numel()} differ; first at", bad.nonzero()[:8].tolist())


# ================================================================================================ weight gradient
WGRAD_CASES = [(r, hh, op) for r in range(3) for hh in (7, 8) for op in ("spikes", "counts") if op == "spikes" or r != 1]


@pytest.mark.parametrize("row,HH,operand", WGRAD_CASES)
def test_weight_gradient_and_bias_gradient_bit_equal(dev, ops, lib, row, HH, operand):
    """spk_conv3x3_wgrad_bf16 with several images per slice (the second LDS buffer, the deposits between the k steps, the prefetch),
    a short last slice and empty slices: gw and gb equal the oracle on binary spikes and on spike counts 0..16; a second call into
    a workspace and outputs pre-filled with NaN gives the same bits (no stale partial sum is read)."""
    Cout, Cin, TB, claim = O.wgrad_rows(_cus())[row]
    form = O.wgrad_form(TB, Cout, Cin, _cus())
    assert claim(form), ("the row does not reach the form it names", form)
    n = Cout * 9 * Cin
    nb = int(lib.spk_conv3x3_wgrad_ws_bytes(TB, Cout, Cin))
    assert nb == form["ksplit"] * (n + Cout) * 4, "the library's slice count is the predicted one"
    _form("wgrad", f"{Cout}x{Cin}-TB{TB}-{HH}x{HH}-{operand}", form)
    c = _case(O.make_wgrad, TB, Cout, Cin, HH, operand)
    gy = c.gy.to(dev).contiguous(memory_format=CL)
    x = c.x.to(dev).contiguous(memory_format=CL)
    gw, gb = ops.conv3x3_wgrad(gy, x, Cout, Cin, want_bias=True)
    _tally("wgrad", gw, c.gw, ("gw", row, HH, operand))
    _tally("wgrad", gb, c.gb, ("gb", row, HH, operand))
    ws = torch.full((nb // 4,), float("nan"), device=dev)
    gw2 = torch.full((Cout, 3, 3, Cin), float("nan"), device=dev)
    gb2 = torch.full((Cout,), float("nan"), device=dev)
    rc = lib.spk_conv3x3_wgrad_bf16(gy.data_ptr(), x.data_ptr(), ws.data_ptr(), nb, gw2.data_ptr(), gb2.data_ptr(), TB, HH, HH, Cout,
                                    Cin, ops._stream(gy))
    assert rc == 0
    _tally("wgrad", gw2.permute(0, 3, 1, 2), c.gw, ("gw into a NaN workspace", row, HH, operand))
    _tally("wgrad", gb2, c.gb, ("gb into a NaN workspace", row, HH, operand))
    gw3 = ops.conv3x3_wgrad(gy, x, Cout, Cin)                                # (no bias gradient requested)
    _tally("wgrad", gw3, c.gw, ("gw alone", row, HH, operand))


# ================================================================================================ data gradient
def _pack_multi(lib, ops, w_cl, N, Cout, Cin):
    """spk_conv3x3_dgrad_f16x2_pack_multi for one layer: (workspace, bytes, the tile width it recorded)."""
    nb = int(lib.spk_conv3x3_dgrad_ws_bytes(Cout, Cin))
    ws = torch.zeros(nb, dtype=torch.uint8, device=w_cl.device)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    rc = lib.spk_conv3x3_dgrad_f16x2_pack_multi((vp * 1)(w_cl.data_ptr()), (vp * 1)(ws.data_ptr()), (ctypes.c_longlong * 1)(nb),
                                                (ci * 1)(N), (ci * 1)(Cout), (ci * 1)(Cin), 1, ops._stream(w_cl))
    assert rc == 0
    torch.cuda.synchronize()
    off = Cout * 9 * Cin * 6 + Cin * 4
    tag = int(ws[off:off + 4].cpu().view(torch.int32)[0])
    return ws, nb, tag


DGRAD_CASES = [(r, hh, form, fam) for r in range(5) for hh in (7, 8) for form, fams in O.DGRAD_FAMILIES.items() for fam in fams]


@pytest.mark.parametrize("row,HH,form,family", DGRAD_CASES)
def test_data_gradient_bit_equal(dev, ops, lib, row, HH, form, family):
    """spk_conv3x3_dgrad_bf16 (products (0,0) (0,1) (1,0) (0,2) (2,0) (1,1) over the three families that populate them) and
    spk_conv3x3_dgrad_f16x2 (products (h,h) (h,m) (m,h); images and input channels spread over 32 binades, one all-zero image, one
    all-zero input channel), the two-term form also through the multi-layer pack + prepacked entry: gi equals the oracle.  Rows:
    two column tiles per wave with a ragged last group of images (one and three chunks of output channels), one column tile with
    three and two-plus-ragged groups."""
    N, Cout, Cin, nt = O.dgrad_rows(_cus())[row]
    f = O.dgrad_form(form, N, Cout, Cin, _cus())
    assert f["NT"] == (nt if form == "f16x2" else 1) and (f["NT"] == 1 or f["last_group"] < 8), f
    fam = f"dgrad_{form}"
    _form(fam, f"N{N}-{Cout}x{Cin}-{HH}x{HH}", f)
    c = _case(O.make_dgrad, form, family, N, Cout, Cin, HH)
    gy = c.gy.to(dev).contiguous(memory_format=CL)
    w = c.w.to(dev)
    gi = ops.conv3x3_dgrad(gy, w, Cin, form=form)
    _tally(fam, gi, c.gi, (form, family, row, HH))
    if form == "f16x2":
        ws, nb, tag = _pack_multi(lib, ops, w.contiguous(memory_format=CL), N, Cout, Cin)
        assert tag == 32 * f["NT"], "the library packed for the predicted number of column tiles"
        out = torch.full((N, HH, HH, Cin), float("nan"), device=dev)
        rc = lib.spk_conv3x3_dgrad_f16x2_prepacked(gy.data_ptr(), ws.data_ptr(), nb, out.data_ptr(), N, HH, HH, Cout, Cin, ops._stream(gy))
        assert rc == 0
        _tally("dgrad_prepacked", out.permute(0, 3, 1, 2), c.gi, ("prepacked", family, row, HH))


def _impulse_launches(cus):
    # (form, N): the three-term form, the two-term form with one column tile per wave and with two
    return [("bf16x3", 69), ("f16x2", 69), ("f16x2", 8 * (cus // 4 + 1) - 5)]


@pytest.mark.parametrize("HH", [7, 8])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["bf16x3", "f16x2-nt1", "f16x2-nt2"])
def test_data_gradient_impulses(dev, ops, which, HH):
    """One unit weight (co, ci, tap) and, in every image, one unit gy element of channel co at map position (image index mod
    positions): gi of that image is a single one at (y - 1 + ky, x - 1 + kx) of channel ci -- or nothing where that falls off the
    map -- and exact zeros elsewhere.  Every position (corners, edges, centre, the column next to the 7x7 padding column) under
    all nine taps; output channels on both k halves and in a later chunk, input channels in both column tiles of a wave and in
    the last workgroup column."""
    form, N = _impulse_launches(_cus())[which]
    Cout, Cin, HW = 48, 128, HH * HH
    f = O.dgrad_form(form, N, Cout, Cin, _cus())
    assert f["NT"] == (2 if which == 2 else 1) and f["last_group"] < 8
    n = torch.arange(N, device=dev)
    yg, xg = (n % HW) // HH, (n % HW) % HH
    fam = "dgrad_impulses"
    for co, ci in ((3, 1), (12, 40), (25, 127), (40, 70)):
        gy = torch.zeros(N, Cout, HH, HH, device=dev)
        gy[n, co, yg, xg] = 1.0
        gy = gy.contiguous(memory_format=CL)
        for tap in range(9):
            ky, kx = tap // 3, tap % 3
            w = torch.zeros(Cout, Cin, 3, 3, device=dev)
            w[co, ci, ky, kx] = 1.0
            got = ops.conv3x3_dgrad(gy, w, Cin, form=form)
            yo, xo = yg - 1 + ky, xg - 1 + kx
            ok = (yo >= 0) & (yo < HH) & (xo >= 0) & (xo < HH)
            want = torch.zeros(N, Cin, HH, HH, device=dev)
            want[n[ok], ci, yo[ok], xo[ok]] = 1.0
            n_bad = int((got != want).sum())
            st = STATS.setdefault(fam, [0, 0, {}])
            st[0] += want.numel()
            st[1] += n_bad
            assert n_bad == 0, (form, HH, "co", co, "ci", ci, "tap", (ky, kx), n_bad, (got != want).nonzero()[:8].tolist())
    _form(fam, f"{form}-N{N}-{HH}x{HH}", f)


@pytest.mark.parametrize("form", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("row,HH", [(1, 7), (3, 8)])
def test_data_gradient_contains_a_nan_to_its_image(dev, ops, form, row, HH):
    """One element of image 1's gy is NaN: every OTHER image's gi -- images of the same workgroup included -- equals, bit for bit,
    the run without the NaN (= the oracle).  What the poisoned image itself returns is recorded, not asserted: in the two-term
    form the NaN is the image's largest bit pattern and sets the image's scale (2^-114), so its finite outputs differ from an
    fp32 operator's, which would keep the outputs outside the NaN's 3x3 window intact."""
    N, Cout, Cin, _ = O.dgrad_rows(_cus())[row]
    family = O.DGRAD_FAMILIES[form][0]
    c = _case(O.make_dgrad, form, family, N, Cout, Cin, HH)
    gy = c.gy.clone()
    gy[1, Cout // 2, HH // 2, 2] = float("nan")
    gi = ops.conv3x3_dgrad(gy.to(dev).contiguous(memory_format=CL), c.w.to(dev), Cin, form=form).cpu()
    keep = torch.arange(N) != 1
    _tally("dgrad_containment", gi[keep], c.gi[keep], ("images beside the poisoned one", form, row, HH))
    p = gi[1]
    STATS["dgrad_containment"][2][f"{form}-N{N}-{HH}x{HH}"] = dict(poisoned_image_nan=int(torch.isnan(p).sum()),
                                                                    poisoned_image_equal_to_clean=int((p == c.gi[1]).sum()),
                                                                    poisoned_image_values=p.numel())
    _report("dgrad_containment")


# ================================================================================================ small-input weight gradient
@pytest.mark.parametrize("row", range(len(O.SMALL_ROWS)))
def test_small_input_weight_gradient_bit_equal(dev, ops, lib, row):
    """spk_conv3x3_wgrad_small at N = 4 CUs + 7: seven waves take a second image (the rewrite of the padded LDS image) and the last
    workgroup of the first round is ragged; Cin 1..4, Cout that is and is not a multiple of 32 and 64, square and non-square maps,
    both weight memory formats, the bias gradient requested and not."""
    Cin, Cout, H, W, cl, want_gb = O.SMALL_ROWS[row]
    N = 4 * _cus() + 7
    f = O.small_form(N, _cus())
    assert f["images_per_wave_max"] == 2 and f["waves_with_a_second_image"] == 7 and f["ragged"], f
    assert int(lib.spk_conv3x3_wgrad_small_ws_bytes(N, H, W, Cout, Cin)) == f["parts"] * ((Cout + 63) // 64) * (Cin * 9 + 1) * 64 * 4, \
        "the library's workgroup count is the predicted one"
    _form("wgrad_small", f"N{N}-{Cin}->{Cout}-{H}x{W}-{'cl' if cl else 'nchw'}-{'gb' if want_gb else 'nogb'}", f)
    c = _case(O.make_wgrad_small, N, Cin, Cout, H, W)
    wd = torch.zeros(Cout, Cin, 3, 3, device=dev)
    if cl:
        wd = wd.contiguous(memory_format=CL)
    gw, gb = ops.conv3x3_wgrad_small(c.gy.to(dev), c.x.to(dev), wd, want_gb)
    assert gw.shape == (Cout, Cin, 3, 3) and (gw.is_contiguous(memory_format=CL) if cl else gw.is_contiguous())
    _tally("wgrad_small", gw, c.gw, ("gw", row))
    if want_gb:
        _tally("wgrad_small", gb, c.gb, ("gb", row))
    else:
        assert gb is None
