"""CPU tests of tests/_image_count_cases.py, the case table of tests/test_gpu_image_count.py: the census of the kernels that read the
device-side image count equals the sources, every case reaches the sites it names at the constants the launchers have now, and the
sentinels the GPU test prefills its output buffers with can never be a legal output -- checked on the oracle's own tensors, for every
case and every image, so that "still the sentinel" can only mean "not written"."""
import pytest
import torch

import _conv_bn_lif_oracle as O
import _image_count_cases as ic

RECORD_BYTES = (0x00, 0x02, 0x20, 0x22)      # two e2m1 nibbles, each 0.0 or 1.0


def test_census_of_the_image_count_reads_equals_the_sources():
    """Every spk_batch_count( call of csrc/*.hip and the written-out copy, by file and enclosing function, is a site of the table --
    no more, no fewer -- and every site names at least one case."""
    found = ic.count_sites()
    table = {}
    for (f, fn), ids in ic.SITES.items():
        table.setdefault(f, []).append(fn)
        assert ids, f"{f}: {fn} reads the image count and no case of tests/_image_count_cases.py reaches it"
        assert all(i in ic.BY_ID for i in ids)
    assert {f: len(v) for f, v in found.items()} == {f: len(v) for f, v in table.items()}, (found, "against the table", table)
    assert {f: sorted(v) for f, v in found.items()} == {f: sorted(v) for f, v in table.items()}
    assert sum(len(v) for v in found.values()) == 14
    written_out = [ln for ln in ic._src("den_mfma_fp6v2.hip").splitlines() if ic.WRITTEN_OUT in ln]
    assert len(written_out) == 1 and "spk_batch_count(" not in written_out[0]


def test_the_written_out_copy_runs_only_without_a_count():
    """fp6v2_lastpos_shared_body (fp6v2_tail_kernel<7, 7, 3>) is launched under `!n_dyn_or_null && ...`: with a count every 7x7 call
    takes the merged tail, whatever its batch.  Its case is therefore the dense call; the launcher's condition is held to the source."""
    src = ic._src("den_mfma_fp6v2.hip")
    i = src.index("fp6v2_tail_kernel<7, 7, 3>), dim3(n_lps")
    cond = src.rfind("if (!n_dyn_or_null && nch >= 2 && B >= SPK_V2_LPS_MIN_B", 0, i)
    assert cond >= 0 and "else" not in src[cond:i] and src.count("fp6v2_tail_kernel<7, 7, 3>), dim3(") == 1
    for B in (5, 64, 256):
        assert ic.fp6v2_tail(B, 64, 7, True) == 0 and ic.fp6v2_tail(B, 64, 8, True) == 1
    assert ic.fp6v2_tail(64, 64, 7, False) == 3 and ic.fp6v2_tail(63, 64, 7, False) == 0 and ic.fp6v2_tail(64, 32, 7, False) == 0


@pytest.mark.parametrize("cid", ic.case_ids())
def test_every_case_reaches_the_sites_it_names(cid):
    case = ic.BY_ID[cid]
    for cus in (O.HOST_CUS, 304, 64):
        reach = case["reach"](cus)
        assert {fn for _, fn in case["sites"]} == set(reach), (cid, reach)
        if cus == O.HOST_CUS or cus == 304:
            assert all(reach.values()), (cid, cus, reach)
    B = case["geo"][9]
    assert all(n is None or 0 <= n <= B for n in case["counts"])
    if case["counts"] != (None,):
        assert 0 in case["counts"] and B in case["counts"] and any(n % 2 for n in case["counts"]) and any(n and n % 2 == 0 for n in case["counts"])
        assert B == (105 if cid == "i8-counts-shared" else ic.B5)
        assert max(case["geo"][0], case["geo"][1]) <= 128 and case["geo"][7] * case["geo"][8] <= 64


def test_the_table_reaches_every_family_and_form_of_the_issue():
    forms = {(c["family"], c["form"]) for c in ic.CASES}
    assert forms >= {("direct", "ptc-lif"), ("direct", "ptc-mean"), ("direct", "seq-raw"), ("direct", "tinv"), ("i8", "i8-lif"),
                     ("i8", "i8-counts"), ("fp6", "fp6-lif"), ("fp6v2", "fp6v2"), ("fp6v2", "fp6v2-listed"), ("fp6v2", "fp6v2-part4")}
    v2 = [c for c in ic.CASES if c["form"] == "fp6v2" and c["counts"] != (None,)]
    assert {(c["v2_form"], c["cap"]) for c in v2 if c["geo"][7] == 7} == {(0, -1), (0, 0), (1, -1), (1, 0)}
    assert {c["cap"] for c in v2 if c["geo"][7] == 8} == {-1, 0}
    assert {c["has_v"] for c in ic.CASES if c["form"] == "tinv"} == {True, False}
    assert any("cnt" in ic.expected(c) for c in ic.CASES if c["form"] == "ptc-lif")
    # one, two and three K chunks under the merged tail (its four waves split them: a wave without a chunk adds nothing)
    assert {c["geo"][0] // 32 for c in v2 if c["geo"][7] == 7} == {1, 2, 3}


def test_count_zero_forms_no_address_from_an_empty_range():
    """What the GPU test's n = 0 runs rely on, read from the sources and held to them: every kernel leaves before it forms an
    address from `Bn - 1` or from an empty unit range.  conv3x3_counts_mfma_shared_kernel returns at `R0 >= nrows` (nrows = 0: every
    workgroup) ABOVE the `Bn - 1` clamp of its staging index; fp6v2_lastpos_body has n_units = 0, so unit = its workgroup index,
    b0 = (unit / G) * 2 * NP >= 0 = Bn and it returns at `b0 >= Bn` before any load; the persistent kernels' item loops have
    `total = Bn * G = 0` items and the direct kernels' loops `npos = Bn * plane = 0` positions (`npos - 1` is formed inside them)."""
    shared = ic._src("den_mfma.hip")
    shared = shared[shared.index("void conv3x3_counts_mfma_shared_kernel"):]
    assert 0 < shared.index("if (R0 >= nrows) return;") < shared.index("Bn - 1")
    lp = ic._src("den_mfma_fp6v2.hip")
    lp = lp[lp.index("void fp6v2_lastpos_body"):lp.index("void fixup_neuron")]
    assert 0 < lp.index("if (b0 >= Bn) return;") < lp.index("a.in0 +") and lp.index("if (b0 >= Bn) return;") < lp.index("a.wq +")
    assert ic.lastpos_units(0, 64) == (0, True)
    direct = ic._src("conv_direct.hip")
    for fn, loop in (("void tinv_lif_kernel", "p0 < npos"), ("void tinv_lif_staged_kernel", "c0 < npos")):
        body = direct[direct.index(fn):]
        assert 0 < body.index(loop) < body.index("npos - 1"), fn


@pytest.mark.parametrize("cid", ic.case_ids())
def test_no_sentinel_is_a_legal_output(cid):
    """On the oracle's own tensors, for every image of the case: record bytes are two nibbles of 0.0 / 1.0, spike bytes 0 / 1,
    spike counts at most 16 -- none is 0xAB; fp32 outputs are finite -- none is NaN; the carried potential moves somewhere in the
    image; and the image's output is not all zero (a zero-filled buffer would tell as little)."""
    case = ic.BY_ID[cid]
    B = case["geo"][9]
    exp = ic.expected(case)
    assert exp
    c = ic.oracle(case)
    for name, e in exp.items():
        w = e.want.movedim(e.axis, 0)
        assert w.shape[0] == B
        if e.kind == "rec":
            assert w.dtype == torch.uint8 and bool(torch.isin(w, torch.tensor(RECORD_BYTES, dtype=torch.uint8)).all())
        elif e.kind == "ptc":
            assert w.dtype == torch.uint8 and int(w.max()) <= 1
        elif e.kind == "cnt":
            assert w.dtype == torch.uint8 and int(w.max()) <= 16
        elif e.kind in ("f32", "mean"):
            assert bool(torch.isfinite(w).all())
            if e.kind == "mean":
                assert bool(torch.isfinite(e.bound).all()) and float(e.bound.max()) < 1e-4
        else:
            assert e.kind == "v" and w.dtype == torch.float32 and bool(torch.isfinite(w).all())
            moved = (w != c.v0).flatten(1).any(1)
            assert bool(moved.all()), (cid, "images whose carried potential does not move:", (~moved).nonzero().flatten().tolist())
        if w.dtype == torch.uint8:
            assert not bool((w == ic.U8_SENTINEL).any())
        nz = (w != 0).flatten(1).any(1)
        assert bool(nz.all()), (cid, name, "images whose output is all zero:", (~nz).nonzero().flatten().tolist())


def test_listed_case_lists_every_image_and_not_every_position():
    case = ic.BY_ID["fp6v2-listed"]
    um = ic.listed_unmasked(case)
    B = case["geo"][9]
    assert all(not bool(um[b].all()) for b in range(B)), "every image is active"
    listed = ic.listed_positions(case)
    assert listed.shape == (B, 49) and bool(listed[:, 48].all())
    per_image = listed[:, :48].sum(1)
    assert int(per_image.min()) >= 1 and int(per_image.max()) < 48, "the lists are neither empty nor everything"
