"""The proof, made with the reference alone, that the cases of tests/test_gpu_train_grad_oracle.py have ONE answer each and that
nothing has to be excluded from their bit-for-bit comparison (tests/_train_grad_oracle.py).

For every case the GPU file runs, at full shape and for a 256-CU device: the builder's assertions hold -- the sum of |terms| of
every output stays within 2^24 product units, the term planes the case names are populated, the products the kernel drops are
zero.  At reduced shapes (the emulation walks one rank-1 update per term product) a numpy emulation of each kernel's arithmetic --
the operands split as the kernel splits them, the kept term products accumulated in fp32 -- gives the fp64 oracle bit for bit in
two different shuffled orders."""
import numpy as np
import pytest
import torch

import _train_grad_oracle as O

CUS = 256


# ================================================================================================ launch forms
def test_rows_reach_the_forms_they_name_on_a_256_cu_device():
    rows = O.wgrad_rows(CUS)
    assert [(co, ci, tb) for co, ci, tb, _ in rows] == [(128, 64, 389), (256, 64, 257), (512, 256, 50)]
    forms = [O.wgrad_form(tb, co, ci, CUS) for co, ci, tb, _ in rows]
    assert all(claim(f) for (_, _, _, claim), f in zip(rows, forms)), forms
    assert forms[0] == dict(tiles=1, ksplit=128, per=4, used=98, last=1, empty=30)
    assert (forms[1]["ksplit"], forms[1]["per"]) == (128, 3) and (forms[2]["ksplit"], forms[2]["per"], forms[2]["last"]) == (16, 4, 2)
    for N, Cout, Cin, nt in O.dgrad_rows(CUS):
        f = O.dgrad_form("f16x2", N, Cout, Cin, CUS)
        assert f["NT"] == nt and O.dgrad_form("bf16x3", N, Cout, Cin, CUS)["NT"] == 1
        if nt == 2:
            assert N == 515 and f["last_group"] == 3, "NT = 2 with a ragged last group"
    assert {f["chunks"] for f in (O.dgrad_form("f16x2", *r[:3], CUS) for r in O.dgrad_rows(CUS))} == {1, 3}
    s = O.small_form(4 * CUS + 7, CUS)
    assert s == dict(parts=CUS, images_per_wave_max=2, waves_with_a_second_image=7, ragged=True)
    assert O.small_form(512, CUS)["images_per_wave_max"] == 1, "the largest N of the tolerance tests stays at one image per wave"


@pytest.mark.parametrize("cus", [64, 80, 104, 228, 256, 304])
def test_rows_reach_their_forms_on_other_cu_counts(cus):
    for co, ci, tb, claim in O.wgrad_rows(cus):
        assert claim(O.wgrad_form(tb, co, ci, cus)), (cus, co, ci, tb, O.wgrad_form(tb, co, ci, cus))
    for N, Cout, Cin, nt in O.dgrad_rows(cus):
        f = O.dgrad_form("f16x2", N, Cout, Cin, cus)
        assert f["NT"] == nt and (nt == 1 or f["last_group"] == 3), (cus, N, f)
    assert O.small_form(4 * cus + 7, cus)["waves_with_a_second_image"] == 7


# ================================================================================================ the splits
def test_split_emulations():
    """Three truncated bf16 terms reproduce any fp32; a 2^8 + b has exactly two terms; at most 8 significant bits: one term;
    22-bit integers below 2^15 (in units of 2^-7) split into two fp16 terms with no remainder."""
    rng = np.random.RandomState(1)
    x = (rng.standard_normal(4096) * np.exp2(rng.randint(-30, 30, size=4096))).astype(np.float32)
    h, m, lo = O.split_bf16x3(x)                                           # (asserts h + m + lo == x and that lo is a bf16)
    assert O.is_bf16(h) and O.is_bf16(m)
    two = np.array([a * 256 + b for a in (2, 3) for b in (1, 2, 3)], dtype=np.float32)
    h, m, lo = O.split_bf16x3(np.concatenate([two, -two]))
    assert h.all() and m.all() and not lo.any()
    h, m, lo = O.split_bf16x3(np.arange(1, 256, dtype=np.float32) * np.float32(2.0 ** -9))
    assert h.all() and not m.any() and not lo.any()
    v = (rng.randint(1 << 21, 1 << 22, size=4096) | 1).astype(np.float32)
    s, inv = O.f16_scales(v)
    assert (v * s >= 2.0 ** 14).all() and (v * s < 2.0 ** 15).all() and (s * inv == 1.0).all()
    h, m, r = O.split_f16x2(v, s)
    assert m.all() and not r.any()
    assert O.f16_scales(np.zeros(1, dtype=np.float32))[0][0] == 1.0


# ================================================================================================ conditions at full shape
WGRAD_FULL = [(r, hh, op) for r in range(3) for hh in (7, 8) for op in ("spikes", "counts") if op == "spikes" or r != 1]


@pytest.mark.parametrize("row,HH,operand", WGRAD_FULL)
def test_weight_gradient_cases_have_one_answer(row, HH, operand):
    Cout, Cin, TB, _ = O.wgrad_rows(CUS)[row]
    c = O.make_wgrad(TB, Cout, Cin, HH, operand)                            # (the builder asserts the budget and the planes)
    assert c.budget <= 1.0 and c.wide_positions == HH * HH and c.wide_in_last_image
    assert c.gw.abs().max() > 0 and (c.gw != 0).float().mean() > 0.9


DGRAD_FULL = [(r, hh, form, fam) for r in range(5) for hh in (7, 8) for form, fams in O.DGRAD_FAMILIES.items() for fam in fams]


@pytest.mark.parametrize("row,HH,form,family", DGRAD_FULL)
def test_data_gradient_cases_have_one_answer(row, HH, form, family):
    N, Cout, Cin, _ = O.dgrad_rows(CUS)[row]
    c = O.make_dgrad(form, family, N, Cout, Cin, HH)                        # (budget, populated planes, dropped products == 0)
    assert c.budget <= 1.0 and (family == "g2w2" or c.wide > 0)
    if family != "g2w2" and N >= 11:
        assert c.last_term_lsb > 0, "some wide entry reaches the lowest mantissa bit of the operand's last term"
    live = c.gi[:max(N - 1, 1)]
    assert (live != 0).float().mean() > 0.5


@pytest.mark.parametrize("row", range(len(O.SMALL_ROWS)))
def test_small_input_cases_have_one_answer(row):
    Cin, Cout, H, W, _, _ = O.SMALL_ROWS[row]
    assert H * W <= 64 and (H + 2) * (W + 2) <= 100 and Cin <= 4, "what the entry point admits"
    c = O.make_wgrad_small(4 * CUS + 7, Cin, Cout, H, W)
    assert c.budget <= 1.0 and c.gw.abs().max() > 0


def test_small_input_rows_cover_what_the_issue_lists():
    rows = O.SMALL_ROWS
    assert {r[0] for r in rows} == {1, 2, 3, 4} and {r[1] for r in rows} == {64, 96, 130}
    assert {r[2:4] for r in rows} == {(7, 7), (8, 8), (5, 12), (2, 3)}
    assert {r[4] for r in rows} == {True, False} and {r[5] for r in rows} == {True, False}


# ================================================================================================ the kernels' arithmetic, emulated
def _two_orders(emulate, case, want):
    a, b = emulate(case, 11), emulate(case, 12)
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    for x, y, w in zip(a, b, want):
        assert x.dtype == torch.float32 and torch.equal(x, y), "the two shuffled orders disagree"
        assert torch.equal(x, w), "the emulated kernel arithmetic is not the fp64 oracle"


@pytest.mark.parametrize("operand", ["spikes", "counts"])
@pytest.mark.parametrize("HH", [7, 8])
def test_weight_gradient_arithmetic_gives_the_oracle_in_any_order(HH, operand):
    c = O.make_wgrad(7, 12, 6, HH, operand, seed=HH)
    _two_orders(O.emulate_wgrad, c, (c.gw, c.gb))


@pytest.mark.parametrize("form,family", [(f, fam) for f, fams in O.DGRAD_FAMILIES.items() for fam in fams])
@pytest.mark.parametrize("HH,Cout", [(7, 48), (8, 16)])
def test_data_gradient_arithmetic_gives_the_oracle_in_any_order(HH, Cout, form, family):
    c = O.make_dgrad(form, family, 4, Cout, 32, HH, seed=HH)
    _two_orders(O.emulate_dgrad, c, (c.gi,))


@pytest.mark.parametrize("Cin,H,W", [(2, 7, 7), (4, 5, 12), (3, 2, 3)])
def test_small_input_arithmetic_gives_the_oracle_in_any_order(Cin, H, W):
    c = O.make_wgrad_small(9, Cin, 10, H, W, seed=Cin)
    _two_orders(O.emulate_wgrad_small, c, (c.gw, c.gb))


def test_a_dropped_product_would_be_seen():
    """The emulation is not blind: without the (1,1) product the two-plane family misses the oracle, without (m, h) the wide-gy
    two-term family does."""
    c = O.make_dgrad("bf16x3", "g2w2", 4, 16, 32, 7)
    full = O.DGRAD_PRODUCTS["bf16x3"]
    try:
        O.DGRAD_PRODUCTS["bf16x3"] = [p for p in full if p != (1, 1)]
        assert not torch.equal(O.emulate_dgrad(c, 3), c.gi)
    finally:
        O.DGRAD_PRODUCTS["bf16x3"] = full
    c = O.make_dgrad("f16x2", "g22w11", 4, 16, 32, 7)
    full = O.DGRAD_PRODUCTS["f16x2"]
    try:
        O.DGRAD_PRODUCTS["f16x2"] = [p for p in full if p != (1, 0)]
        assert not torch.equal(O.emulate_dgrad(c, 3), c.gi)
    finally:
        O.DGRAD_PRODUCTS["f16x2"] = full
