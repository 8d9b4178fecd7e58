"""CPU tests of the non-square cases of the training convolutions (tests/_conv_train_cases.NONSQUARE_CASES) and of their exact
oracle (tests/_conv_train_oracle.py); the GPU runs are tests/test_gpu_conv_train_nonsquare.py.

Shown here, without a device: every case lands on the kernel and branch it names (its ``claim`` on the mirrored launch, and the
library's own support queries and workspace sizes agree with the mirror); the table as a whole covers what it is meant to cover;
every case meets the exactness bound; on the reference operator alone the fp32 sum of an output's products does not depend on the
order; and every case can tell an H / W exchange: the oracle of the same buffers read with H and W swapped differs from the true one
on every output tensor of the case -- y, gi and gw, and their relu / masked forms (the bias gradient, a plain sum, is exempt) -- the
host-side stand-in for breaking the kernel and watching the test fail.  The module-level cases (MODULE_CASES) are held to all of
it, the generic API convolution's cases (API_CONV_CASES; fp64 accumulation, NCHW) to their claims, the bound and the exchange."""
import pytest
import torch
import torch.nn.functional as F

import _conv_train_cases as cases
import _conv_train_oracle as O

NS = cases.NONSQUARE_CASES
MODULES = cases.MODULE_CASES
APIS = cases.API_CONV_CASES
_id = lambda c: c["id"]                                                       # noqa: E731


def test_every_nonsquare_case_lands_on_the_kernel_it_names():
    from spkdiff import _lib
    lib = _lib.lib
    assert cases.check_claims(NS + MODULES + APIS) == []
    assert len({c["id"] for c in NS + MODULES + APIS}) == len(NS + MODULES + APIS)
    assert all(c["N"] == c["T"] * c["B"] and cases.map_size(c["layer"])[0] != cases.map_size(c["layer"])[1] for c in MODULES)
    for c in NS + MODULES:
        if c["op"] == "wgrad":
            n, hu, wu, cu, hv, wv, cv, k, s, p, bf = cases.wgrad_args(c["layer"], c["N"])
            assert lib.spk_conv_train_wgrad_ws_bytes(n, hv, wv, cu, cv, k) == cases.launch(c)["ws_bytes"], c["id"]
        else:
            n, hi, wi, cred, ho, wo, cout, k, s, p, form = cases.gather_args(c["layer"], c["N"], c["op"])
            assert lib.spk_conv_train_gather_supported(cred, cout, k, s, form) == 1, c["id"]


def test_an_eight_field_layer_still_means_a_square_map():
    for c in cases.BOUNDARY_CASES + cases.REGISTER_WGRAD_CASES:
        layer = c["layer"]
        assert len(layer) == 8 and cases.map_size(layer) == (layer[7], layer[7])
        wide = layer + (layer[7],)
        assert cases.launch(c) == cases.launch(dict(c, layer=wide))
        assert cases.wgrad_args(layer, c["N"]) == cases.wgrad_args(wide, c["N"])
        for op in ("fwd", "dgrad"):
            a = cases.gather_args(layer, c["N"], op)
            assert a == cases.gather_args(wide, c["N"], op) and a[1] == a[2] and a[4] == a[5]
    # and a separate W reaches the width arguments alone
    assert cases.gather_args((8, 24, 3, 2, 1, False, 0, 9, 6), 2, "fwd") == (2, 9, 6, 8, 5, 3, 24, 3, 2, 1, 0)
    assert cases.gather_args((8, 24, 3, 2, 1, False, 0, 9, 6), 2, "dgrad") == (2, 5, 3, 24, 9, 6, 8, 3, 2, 1, 1)
    assert cases.wgrad_args((8, 24, 3, 2, 1, True, 1, 9, 6), 2) == (2, 18, 12, 24, 9, 6, 8, 3, 2, 1, 2)
    assert cases.wgrad_args((8, 24, 3, 2, 1, False, 0, 9, 6), 2) == (2, 9, 6, 8, 5, 3, 24, 3, 2, 1, 1)


def test_the_table_covers_every_kernel_and_branch_on_maps_of_both_orientations():
    L = {c["id"]: cases.launch(c) for c in NS}
    by_kernel = {}
    for c in NS:
        H, W = cases.map_size(c["layer"])
        assert H != W, c["id"]
        # the input and the output map of the launch are both non-square
        a = cases.wgrad_args(c["layer"], c["N"]) if c["op"] == "wgrad" else cases.gather_args(c["layer"], c["N"], c["op"])
        assert a[1] != a[2] and a[4] != a[5], (c["id"], a)
        by_kernel.setdefault(L[c["id"]]["kernel"], []).append(c)
    assert set(by_kernel) == {"gather", "c1in", "c1out", "wgrad_lds", "wgrad_reg", "c1_wgrad"}
    tall = lambda cs: any(cases.map_size(c["layer"])[0] > cases.map_size(c["layer"])[1] for c in cs)     # noqa: E731
    wide = lambda cs: any(cases.map_size(c["layer"])[0] < cases.map_size(c["layer"])[1] for c in cs)     # noqa: E731
    gathers = by_kernel["gather"] + by_kernel["c1in"] + by_kernel["c1out"]
    wgrads = by_kernel["wgrad_lds"] + by_kernel["wgrad_reg"] + by_kernel["c1_wgrad"]
    assert tall(gathers) and wide(gathers) and tall(wgrads) and wide(wgrads)
    g = [L[c["id"]] for c in by_kernel["gather"]]
    assert {(x["form"], x["CN"]) for x in g} >= {(0, 1), (1, 1), (0, 2)}
    assert any(x["form"] == 1 and len(set(x["class_rows"])) == 4 for x in g), "no form-1 case with four different classes"
    assert any(x["class_rows"][0] % 32 for x in g if x["form"] == 0)
    strides = {(x["form"], c["layer"][3]) for c, x in zip(by_kernel["gather"], g)}
    assert strides >= {(0, 1), (0, 2), (1, 1), (1, 2)}
    assert {c["layer"][2] for c, x in zip(by_kernel["gather"], g) if x["form"] == 1} >= {2, 3, 4}
    reduced = lambda c: cases.gather_args(c["layer"], c["N"], c["op"])[3]                                # noqa: E731
    outch = lambda c: cases.gather_args(c["layer"], c["N"], c["op"])[6]                                  # noqa: E731
    assert {reduced(c) for c in by_kernel["c1in"]} >= {1, 2, 3} and {outch(c) for c in by_kernel["c1out"]} >= {1, 2, 3}
    for k in ("c1in", "c1out"):
        assert any(L[c["id"]]["rows"] == cases.CT_C1_ROWS_CAP + 1 for c in by_kernel[k]), k
    lds = [L[c["id"]] for c in by_kernel["wgrad_lds"]]
    assert sorted(x["RB"] for x in lds) == [1, 2, 3, 4]
    bias_from = lambda c: cases.wgrad_args(c["layer"], c["N"])[-1] if c.get("bias", True) else 0         # noqa: E731
    assert {(bias_from(c), L[c["id"]]["fuse_bias"]) for c in by_kernel["wgrad_lds"]} == {(1, True), (2, True), (2, False), (0, False)}
    assert {bias_from(c) for c in by_kernel["wgrad_reg"]} == {1, 2}
    assert {c["layer"][0] for c in by_kernel["c1_wgrad"]} == {1, 3}


@pytest.mark.parametrize("c", NS + MODULES + APIS, ids=_id)
def test_every_case_meets_the_exactness_bound(c):
    """make_case asserts it while it builds; restated: each output's absolute products sum to less than 2^24 units of 2^-4, the bias
    and the N * Hv * Wv positions of the weight and bias gradients included -- also on 0/1 input (the cases of 32+ input channels)."""
    case = O.for_case(c)
    assert set(case["abs_sums"]) == set(O.OUTPUTS)
    assert all(0 < v < O.EXACT_LIMIT for v in case["abs_sums"].values()), case["abs_sums"]
    assert all(float(v) == int(v) for v in case["abs_sums"].values())
    for name in ("x", "gy"):
        assert torch.equal(case[name], case[name].round())
    for name in ("w", "bias"):
        assert torch.equal(case[name] / O.UNIT, (case[name] / O.UNIT).round())
    assert int(case["x"].abs().max()) >= 1 and int(case["gy"].abs().max()) >= 1 and float(case["w"].abs().max()) > 0
    assert torch.equal(case["y"], (case["y_nobias"].double() + case["b64"].view(1, -1, 1, 1)).float())


def _terms(case, name, images):
    """[J, ...]: output ``name`` of the first ``images`` images split into its single products by the reference operator alone -- the
    operator is linear, so the operator with all but ONE weight position (y: one (ci, ky, kx); gi: one (co, ky, kx)) or all but one
    position of gy (gw, gb) zeroed yields, for every output element at once, the one product that position contributes."""
    cin, cout, k, s, p, tr, op, H, W, N = case["geo"]
    x, w, gy = case["x64"][:images], case["w64"], case["gy64"][:images]
    conv = (lambda a, b: F.conv_transpose2d(a, b, None, s, p, op)) if tr else (lambda a, b: F.conv2d(a, b, None, s, p))
    terms = []
    if name in ("y", "gi"):
        kept = 0 if (name == "y") == tr else 1                  # the weight dimension that holds the reduced channel
        for c in range(w.shape[kept]):
            for t in range(k * k):
                m = torch.zeros_like(w)
                m.select(kept, c)[:, t // k, t % k] = 1
                if name == "y":
                    terms.append(conv(x, w * m))
                else:
                    xr = x.clone().requires_grad_(True)
                    terms.append(torch.autograd.grad(conv(xr, w * m), xr, gy)[0])
        if name == "y":
            terms.append(case["b64"].view(1, -1, 1, 1).expand_as(terms[0]))
    else:
        wr = w.clone().requires_grad_(True)
        y = conv(x, wr)
        flat = torch.zeros(gy.numel() // cout, dtype=torch.float64)
        for pos in range(flat.numel()):
            flat.zero_()
            flat[pos] = 1
            gm = gy * flat.view(gy.shape[0], 1, gy.shape[2], gy.shape[3])
            terms.append(torch.autograd.grad(y, wr, gm, retain_graph=True)[0] if name == "gw" else gm.sum((0, 2, 3)))
    T = torch.stack(terms)
    assert torch.equal(T.float().double(), T)                  # every product is an fp32 number
    return T.float()


@pytest.mark.parametrize("c", NS + MODULES, ids=_id)
def test_fp32_sums_of_the_products_do_not_depend_on_the_order(c):
    """Each output's products, from the reference operator alone, added in fp32 one by one in three orders (as listed, reversed,
    shuffled; the bias wherever the order puts it): the fp64 oracle's value every time.  y and gi of the cases with many images are
    taken on the first four (their sums do not cross images); gw and gb run over all N * Hv * Wv positions."""
    case = O.for_case(c)
    for name in O.outputs_of(c):
        images = case["geo"][9] if name in ("gw", "gb") else min(case["geo"][9], 4)
        T = _terms(case, name, images)
        want = case[name] if name in ("gw", "gb") else case[name][:images]
        g = torch.Generator().manual_seed(len(c["id"]))
        J = T.shape[0]
        assert J >= 3
        for order in (range(J), range(J - 1, -1, -1), torch.randperm(J, generator=g).tolist()):
            acc = torch.zeros_like(T[0])
            for j in order:
                acc += T[j]
            assert torch.equal(acc, want), (c["id"], name)


@pytest.mark.parametrize("c", NS + MODULES, ids=_id)
def test_every_case_can_tell_an_exchange_of_h_and_w(c):
    """Whatever launch a case names, its data serve every direction (the wrapper and module tests run forward and backward on them,
    the epilogue tests the relu / masked forms): the exchanged oracle differs from the true one on EVERY output tensor -- y, gi and gw
    on at least a quarter of their elements; relu(y) and the masked gi, whose structural zeros cannot differ, on at least a quarter
    of the elements that are non-zero on either side.  The bias gradient, a plain sum, is exempt."""
    case = O.for_case(c)
    sw = O.swapped(case)
    for name in O.SWAP_CHECKED:
        true = case[name] if name == "gw" else O.cl_buffer(case[name])
        assert true.shape == sw[name].shape
        differ = int((true != sw[name]).sum())
        live = true.numel() if name in ("y", "gi", "gw") else int(((true != 0) | (sw[name] != 0)).sum())
        assert live * 4 >= true.numel() // 4, (c["id"], name, live)          # (the epilogue leaves enough to compare)
        assert differ * 4 >= live, (c["id"], name, differ, live, true.numel())


@pytest.mark.parametrize("c", APIS, ids=_id)
def test_the_api_convolution_cases_can_tell_an_exchange_of_h_and_w(c):
    """The generic API convolution reads and writes NCHW: the same x buffer taken as [M][C][W][H] gives another y on at least a
    quarter of the elements -- except for the grid-cap case, whose 1x1 one-channel layer is element-wise (y's buffer is the same
    function of x's buffer in either reading: no exchange can show there; that case is about the second grid-stride trip)."""
    case = O.for_case(c)
    true, sw = O.nchw_buffer(case["y"]), O.swapped_nchw_y(case)
    assert true.shape == sw.shape
    if c["layer"][2] == 1:
        assert c["id"] == "api_conv_1x1_past_grid_cap" and torch.equal(true, sw)
    else:
        assert int((true != sw).sum()) * 4 >= true.numel(), c["id"]
