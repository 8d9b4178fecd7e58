"""The device-side image count (``n_dyn_or_null`` of include/spkdiff.h: "only images [0, *n_dyn) are computed; buffers stay sized by
B"), pinned from BOTH sides: the case table of tests/test_image_count_cases_host.py (CPU) and tests/test_gpu_image_count.py.

Every kernel that obeys the count reads it through ``spk_batch_count`` (csrc/spk_common.h) -- or, once, through a written-out copy of
it.  SITES is the census of those reads, by source file and enclosing function; the CPU test counts the calls in the sources and holds
the census to them, so a new read of the count without a case here fails on a machine without a GPU.  Each case names the entry point it
calls, the sites it reaches and -- ``reach`` -- the launcher's shape arithmetic, restated on the host, that proves it reaches them.

A case runs ONE call at every count of ``counts`` into caller-owned buffers prefilled with a sentinel that is never a legal output
(0xAB for spike bytes, records and counts, NaN for fp32, the carried v0 for membrane potentials).  The inputs of ALL B images are the
oracle's real inputs (the listed launch builds its position lists with every image active and only then lowers the count): a kernel
that ignores the count computes real, detectable results past it from valid memory, never a fault.  Counts above B or below 0 are the
caller's duty (the header) and are not cases.

Geometries are those of the oracle module's rows (tests/_conv_bn_lif_oracle.py: DEN_NDYN_ROWS, DEN_FP6V2_ROWS, DEN_COUNTS_ROWS,
DEN_LISTED_ROW, TINV_ROWS, DIRECT_PTC_EXTRA, SEQ_ROWS) at batch 5 -- one image pair, one odd image out, so that a count of 1 or 3
leaves the partner of the last pair past the count -- except the LDS-shared counts kernel, which needs B * HW > 5120 and keeps its
B = 105 row, and the LDS-shared last-position tail, which the launcher picks only WITHOUT a count (B >= 64)."""
import os
import re
from types import SimpleNamespace

import torch

import _conv_bn_lif_oracle as O
from oracle import snn_ref as ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spiking-diffusion_amd", "csrc")
B5 = 5
COUNTS_B5 = (0, 1, 3, 4, 5)            # nothing, odd (the pair partner is past the count), odd, even, the whole batch
COUNTS_B105 = (0, 52, 53, 105)
U8_SENTINEL = 0xAB
WRITTEN_OUT = "spk_batch_count of spk_common.h, written out"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _constant(src, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", _src(src))
    assert m, f"{name} not found in {src}"
    return int(m.group(1))


SPK_V2_HALF_FILL = _constant("den_mfma_fp6v2.hip", "SPK_V2_HALF_FILL")
SPK_V2_LPS_MIN_B = _constant("den_mfma_fp6v2.hip", "SPK_V2_LPS_MIN_B")
SPK_V2_LP_PAIRS = _constant("den_mfma_fp6v2.hip", "SPK_V2_LP_PAIRS")
SPK_V2_LP_SPLIT_MAX = _constant("den_mfma_fp6v2.hip", "SPK_V2_LP_SPLIT_MAX")
# spk_den_conv3x3_counts_mfma:  if ((long long)B * H * W > 32 * 160 && H * W >= 43 && H * W <= 64)  -> the LDS-shared kernel
_m = re.search(r"B \* H \* W > (\d+) \* (\d+) && H \* W >= (\d+) && H \* W <= (\d+)", _src("den_mfma.hip"))
assert _m, "the counts launcher's choice of kernel not found in den_mfma.hip"
COUNTS_SHARED_ROWS, COUNTS_SHARED_HW_MIN, COUNTS_SHARED_HW_MAX = int(_m.group(1)) * int(_m.group(2)), int(_m.group(3)), int(_m.group(4))


# ------------------------------------------------------------------------------------------------ census
def count_sites():
    """{file: [enclosing function of every read of the device-side image count, in source order]} from csrc/*.hip: the calls of
    spk_batch_count( and the lines that carry the written-out copy's comment."""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith(".hip"):
            continue
        fn, names = None, []
        for ln in _src(f).splitlines():
            m = re.search(r"\bvoid\s+(\w+)\s*\(", ln)
            if m:
                fn = m.group(1)
            if "spk_batch_count(" in ln or WRITTEN_OUT in ln:
                names.append(fn)
        if names:
            out[f] = names
    return out


# (file, enclosing function): ids of the cases that reach it.  Filled by _case() below.
SITES = {
    ("conv_direct.hip", "conv_fused_kernel"): [],
    ("conv_direct.hip", "tinv_lif_kernel"): [],
    ("conv_direct.hip", "tinv_lif_staged_kernel"): [],
    ("den_mfma.hip", "conv3x3_mfma_kernel"): [],
    ("den_mfma.hip", "conv3x3_counts_mfma_kernel"): [],
    ("den_mfma.hip", "conv3x3_counts_mfma_shared_kernel"): [],
    ("den_mfma_fp6.hip", "conv3x3_fp6_kernel"): [],
    ("den_mfma_fp6.hip", "conv3x3_fp6_lastpos_kernel"): [],
    ("den_mfma_fp6v2.hip", "conv3x3_fp6v2_kernel"): [],
    ("den_mfma_fp6v2.hip", "conv3x3_fp6v2_half_kernel"): [],
    ("den_mfma_fp6v2.hip", "conv3x3_fp6v2_listed_kernel"): [],
    ("den_mfma_fp6v2.hip", "fp6v2_lastpos_body"): [],
    ("den_mfma_fp6v2.hip", "fp6v2_fixup_body"): [],
    # the written-out copy.  fp6v2_launch takes the tail that runs it (fp6v2_tail_kernel<7, 7, 3>) only when the call has NO count
    # (`!n_dyn_or_null && nch >= 2 && B >= SPK_V2_LPS_MIN_B`): there the count is B by definition, and its case is the dense call
    ("den_mfma_fp6v2.hip", "fp6v2_lastpos_shared_body"): [],
}


# ------------------------------------------------------------------------------------------------ the launchers, restated
def direct_kernel(in_kind, mode, Cout, k, C0, has_v, T=16, f32=False, pre=False):
    """Which kernel spk_conv_fused_fwd launches under a count (conv_raw_steps_kernel is taken only without one)."""
    if in_kind == "tinv" and mode == "lif" and T == 16 and not f32 and not pre and Cout % 16 == 0 and 256 % Cout == 0:
        if not has_v and (k, C0) in ((3, 1), (3, 3), (3, 2), (1, 16)):
            return f"tinv_lif_staged_kernel<{k},{C0}>"
        if k == 3 and C0 in (1, 2, 3):
            return f"tinv_lif_kernel<3,{C0}>"
        return "tinv_lif_kernel<0,0>"
    return "conv_fused_kernel"


def i8_tiles(H, W):
    """(row tiles, input copy pieces) per wave of conv3x3_mfma_kernel: <7,7> up to 7 of both, else <8,8>."""
    return ((H * W + 1) // 2 + 3) // 4, (H * ((W + 1) // 2) + 3) // 4


def counts_shared(B, H, W):
    return B * H * W > COUNTS_SHARED_ROWS and COUNTS_SHARED_HW_MIN <= H * W <= COUNTS_SHARED_HW_MAX


def fp6_form(H, W):
    """fp6_plan + launch_fp6: 'bands', '6+lastpos' (odd map of at most 24 full tiles) or '7'."""
    ntiles = (H * W + 1) // 2
    if (ntiles + 3) // 4 > 7 and H % 2 == 0 and (H // 2) * W <= 32 and H >= 4:
        return "bands"
    if (H * W) % 2 and (H * W) // 2 <= 24 and H >= 2 and W >= 2:
        return "6+lastpos"
    return "7"


def fp6v2_main(B, Cout, H, form, cus, listed=False):
    """fp6v2_launch's main kernel.  The grid is cus (XCD-aware walk) or the flat walk's (cus / G) * G: the smaller decides."""
    G = Cout // 32
    grid = (cus // G) * G if cus >= G else G
    if H == 8:
        return "conv3x3_fp6v2_kernel"              # <8, 8, 8, SPLIT>
    if listed:
        return "conv3x3_fp6v2_listed_kernel"
    return "conv3x3_fp6v2_half_kernel" if form == 0 and B * G * SPK_V2_HALF_FILL <= grid else "conv3x3_fp6v2_kernel"


def fp6v2_tail(B, Cin, H, has_count):
    """fp6v2_tail_kernel's PART: 1 repair only (8x8), 3 LDS-shared last positions + repair, 0 the merged tail."""
    if H == 8:
        return 1
    return 3 if (not has_count and Cin // 32 >= 2 and B >= SPK_V2_LPS_MIN_B) else 0


def lastpos_units(n, Cout):
    """n_units of fp6v2_lastpos_body at count n (0 at n = 0: every workgroup returns at `b0 >= Bn`) and whether the waves split K."""
    u = ((n + 2 * SPK_V2_LP_PAIRS - 1) // (2 * SPK_V2_LP_PAIRS)) * (Cout // 32)
    return u, u <= SPK_V2_LP_SPLIT_MAX


# ------------------------------------------------------------------------------------------------ cases
CASES = []


def _den(row, B=B5):
    return row[:5] + (B,)


def _case(id, family, row, entry, sites, reach, kind, counts=COUNTS_B5, **kw):
    """row: the oracle module's row with this table's batch; kind: the oracle the case needs ('den' full-width spikes, 'counts'
    full-width count tensor, 'spikes' / 'seq' / 'pixels' the 2^-12 scheme); reach(cus) -> {site: bool}."""
    geo = O.den_geo(row) if kind in ("den", "counts") else (O.tinv_geo(row) if kind == "pixels" else row)
    c = dict(id=id, family=family, row=row, geo=geo, entry=entry, sites=sites, reach=reach, kind=kind, counts=counts, **kw)
    for s in sites:
        SITES[s].append(id)
    CASES.append(c)
    return c


_D, _I8, _F6, _V2 = "conv_direct.hip", "den_mfma.hip", "den_mfma_fp6.hip", "den_mfma_fp6v2.hip"

# ---- direct
_r = _den(O.DEN_NDYN_ROWS["i8"])
_case("direct-ptc-lif", "direct", _r, "spk_conv_fused_fwd", [(_D, "conv_fused_kernel")],
      lambda cus: {"conv_fused_kernel": direct_kernel("ptc", "lif", 32, 3, 32, True, f32=True, pre=True) == "conv_fused_kernel"},
      "den", form="ptc-lif")                       # carried v, out_ptc + out_f32 + out_pre + out_counts together (Cout % 32 == 0)
for _i, _r in enumerate(O.DIRECT_PTC_EXTRA):
    _r = _r[:9] + (B5,)
    _case(f"direct-ptc-lif-extra{_i}", "direct", _r, "spk_conv_fused_fwd", [(_D, "conv_fused_kernel")],
          lambda cus, r=_r: {"conv_fused_kernel": direct_kernel("ptc", "lif", r[1], r[2], r[0], True, f32=True, pre=True) == "conv_fused_kernel"},
          "spikes", form="ptc-lif")                # odd Cout (5, 7: an image ends inside a wave), one of them transposed; no counts
_r = _den(O.DEN_NDYN_ROWS["counts"])
_case("direct-ptc-mean", "direct", _r, "spk_conv_fused_fwd", [(_D, "conv_fused_kernel")],
      lambda cus: {"conv_fused_kernel": direct_kernel("ptc", "mean", 16, 3, 96, False) == "conv_fused_kernel"},
      "den", form="ptc-mean")                      # conv6's form under the direct implementation: in1 concatenated, MODE_MEAN
for _i, _r in enumerate(O.SEQ_ROWS):
    _r = _r[:9] + (B5,)
    _case(f"direct-seq-raw{_i}", "direct", _r, "spk_conv_fused_fwd", [(_D, "conv_fused_kernel")],
          lambda cus, r=_r: {"conv_fused_kernel": direct_kernel("seq", "raw", r[1], r[2], r[0], False) == "conv_fused_kernel"},
          "seq", form="seq-raw")                   # out_f32 is [T,B,...]: the untouched part is [:, n:]
_r = O.TINV_ROWS[2][:7] + (B5,)                     # denoiser conv1's shape: 2 -> 64 channels, 3x3, 7x7
_case("direct-tinv-carried", "direct", _r, "spk_conv_fused_fwd", [(_D, "tinv_lif_kernel")],
      lambda cus, r=_r: {"tinv_lif_kernel": direct_kernel("tinv", "lif", r[1], r[2], r[0], True) == "tinv_lif_kernel<3,2>"},
      "pixels", form="tinv", has_v=True)
_case("direct-tinv-staged", "direct", _r, "spk_conv_fused_fwd", [(_D, "tinv_lif_staged_kernel")],
      lambda cus, r=_r: {"tinv_lif_staged_kernel": direct_kernel("tinv", "lif", r[1], r[2], r[0], False) == "tinv_lif_staged_kernel<3,2>"},
      "pixels", form="tinv", has_v=False)

# ---- int8 digit planes
_r = _den(O.DEN_NDYN_ROWS["i8"])
_case("i8-lif", "i8", _r, "spk_den_conv3x3_mfma", [(_I8, "conv3x3_mfma_kernel")],
      lambda cus, r=_r: {"conv3x3_mfma_kernel": max(i8_tiles(r[3], r[4])) <= 7},                # <7, 7, MODE_LIF>
      "den", form="i8-lif")
_r = _den(O.DEN_NDYN_ROWS["counts"])
assert _r == _den(O.DEN_COUNTS_ROWS[0])
_case("i8-counts-split", "i8", _r, "spk_den_conv3x3_counts_mfma", [(_I8, "conv3x3_counts_mfma_kernel")],
      lambda cus, r=_r: {"conv3x3_counts_mfma_kernel": not counts_shared(r[5], r[3], r[4]) and r[5] * r[3] * r[4] <= COUNTS_SHARED_ROWS},
      "counts", form="i8-counts")                  # 245 rows <= 5120: the four waves split the K chunks
_r = O.DEN_COUNTS_ROWS[2]
_case("i8-counts-shared", "i8", _r, "spk_den_conv3x3_counts_mfma", [(_I8, "conv3x3_counts_mfma_shared_kernel")],
      lambda cus, r=_r: {"conv3x3_counts_mfma_shared_kernel": counts_shared(r[5], r[3], r[4])},
      "counts", counts=COUNTS_B105, form="i8-counts")      # 52 / 53 of 105: the last workgroup's 128 rows end inside / on an image

# ---- six fp6 planes
_r = _den(O.DEN_NDYN_ROWS["fp6"])
_case("fp6-lif", "fp6", _r, "spk_den_conv3x3_mfma_fp6", [(_F6, "conv3x3_fp6_kernel"), (_F6, "conv3x3_fp6_lastpos_kernel")],
      lambda cus, r=_r: {"conv3x3_fp6_kernel": True, "conv3x3_fp6_lastpos_kernel": fp6_form(r[3], r[4]) == "6+lastpos"},
      "den", form="fp6-lif")                       # the last-position kernel's tiles hold image PAIRS

# ---- fp6v2
V2_ROWS = [_den(O.DEN_NDYN_ROWS["fp6v2"]), _den(O.DEN_FP6V2_ROWS[1]), _den(O.DEN_FP6V2_ROWS[2]), _den(O.DEN_FP6V2_ROWS[4])]
assert _den(O.DEN_FP6V2_ROWS[0]) == V2_ROWS[0] and _den(O.DEN_FP6V2_ROWS[3]) == V2_ROWS[2]
for _r in V2_ROWS:
    for _form in ((0,) if _r[3] == 8 else (0, 1)):
        for _cap in (-1, 0):
            _main = "conv3x3_fp6v2_kernel" if (_r[3] == 8 or _form == 1) else "conv3x3_fp6v2_half_kernel"
            _sites = [(_V2, _main), (_V2, "fp6v2_fixup_body")] + ([] if _r[3] == 8 else [(_V2, "fp6v2_lastpos_body")])

            def _reach(cus, r=_r, form=_form, main=_main):
                d = {main: fp6v2_main(r[5], r[2], r[3], form, cus) == main,
                     "fp6v2_fixup_body": fp6v2_tail(r[5], r[0], r[3], True) in (0, 1)}
                if r[3] == 7:                       # the merged tail <7, 7, 0>: every call with a count takes it
                    d["fp6v2_lastpos_body"] = fp6v2_tail(r[5], r[0], r[3], True) == 0 and lastpos_units(r[5], r[2])[1]
                return d
            _case(f"fp6v2-{O.den_geo(_r)[0]}-{_r[2]}-{_r[3]}x{_r[4]}-form{_form}-cap{_cap}", "fp6v2", _r, "spk_den_conv3x3_mfma_fp6v2",
                  _sites, _reach, "den", form="fp6v2", v2_form=_form, cap=_cap)
_r = _den(O.DEN_LISTED_ROW)
_case("fp6v2-listed", "fp6v2", _r, "spk_den_conv3x3_mfma_fp6v2_listed",
      [(_V2, "conv3x3_fp6v2_listed_kernel"), (_V2, "fp6v2_lastpos_body"), (_V2, "fp6v2_fixup_body")],
      lambda cus, r=_r: {"conv3x3_fp6v2_listed_kernel": fp6v2_main(r[5], r[2], r[3], 1, cus, listed=True) == "conv3x3_fp6v2_listed_kernel"
                         and (cus // (r[2] // 32)) >= 6,
                         "fp6v2_lastpos_body": fp6v2_tail(r[5], r[0], r[3], True) == 0, "fp6v2_fixup_body": True},
      "den", form="fp6v2-listed", cap=-1)
_r = V2_ROWS[1]
_case("fp6v2-part4", "fp6v2", _r, "spk_den_conv3x3_mfma_fp6v2_part", [(_V2, "fp6v2_lastpos_body")],
      lambda cus, r=_r: {"fp6v2_lastpos_body": r[3] == 7 and lastpos_units(r[5], r[2])[1]},      # fp6v2_tail_kernel<7, 7, 2>
      "den", form="fp6v2-part4", cap=-1)
_r = O.DEN_FP6V2_ROWS[2]
_case("fp6v2-dense-lds-shared-tail", "fp6v2", _r, "spk_den_conv3x3_mfma_fp6v2", [(_V2, "fp6v2_lastpos_shared_body")],
      lambda cus, r=_r: {"fp6v2_lastpos_shared_body": fp6v2_tail(r[5], r[0], r[3], False) == 3 and fp6v2_tail(r[5], r[0], r[3], True) == 0},
      "den", counts=(None,), form="fp6v2", v2_form=0, cap=-1)      # no count tensor: all B = 64 images are written

BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def case_ids():
    return [c["id"] for c in CASES]


def runs():
    """(case id, count) of every GPU run."""
    return [(c["id"], n) for c in CASES for n in c["counts"]]


# ------------------------------------------------------------------------------------------------ the oracle, once per geometry
_ORACLE = {}


def oracle(case):
    """The case's inputs and the exact results of tests/_conv_bn_lif_oracle.py, computed once per (kind, geometry) and left
    unchanged: y (the convolution rounded once), pre (after BN), (s, v) from the reset state, (s1, v1) from the carried v0; for the
    counts form the logits."""
    kind, geo = case["kind"], case["geo"]
    key = (kind, geo)
    if key not in _ORACLE:
        if kind in ("den", "counts"):
            c = O.make_case(geo, O.full_seed(geo), weights="full", n_inputs=1)
        else:
            c = O.make_case(geo, O.row_seed(geo), kind=kind, n_inputs=1)
        if kind == "counts":
            c.logits, _ = O.counts_logits(c.x.sum(0), c.w, c.bias, geo)
        else:
            x = c.x.unsqueeze(0).repeat(c.T, 1, 1, 1, 1) if kind == "pixels" else c.x
            c.y = O.conv_fp32(x, c.w, c.bias, geo)
            c.pre = O.bn32(c.y, c.a, c.b)
            c.s, c.v = ref.lif_multi_step(c.pre)
            c.s1, c.v1 = ref.lif_multi_step(c.pre, c.v0.clone())
        _ORACLE[key] = c
    return _ORACLE[key]


def _cnt(s):
    return O.to_counts(s)


def expected(case):
    """{output name: SimpleNamespace(want, axis, kind)} of the case's call on ALL B images.  axis: the image axis of the buffer.
    kind: 'ptc' u8 spike bytes, 'rec' nibble-packed records, 'cnt' u8 spike counts, 'f32' fp32 compared bit for bit, 'mean' fp32
    within O.readout_bound (want = the fp64 mean, bound beside it), 'v' the carried potential (sentinel: v0)."""
    c, form = oracle(case), case["form"]
    N = SimpleNamespace
    Cout = case["geo"][1]
    if form == "ptc-lif":
        out = dict(ptc=N(want=O.to_ptc(c.s1), axis=0, kind="ptc"), f32=N(want=c.s1, axis=1, kind="f32"),
                   pre=N(want=c.pre, axis=1, kind="f32"), v=N(want=c.v1, axis=0, kind="v"))
        if Cout % 32 == 0:
            out["cnt"] = N(want=_cnt(c.s1), axis=0, kind="cnt")
        return out
    if form == "ptc-mean":
        mean, mag = O.mean64(c.y)
        return dict(f32=N(want=mean, bound=O.readout_bound(16, mag), axis=0, kind="mean"))
    if form == "seq-raw":
        return dict(f32=N(want=c.y, axis=1, kind="f32"))
    if form == "tinv":
        s, v = (c.s1, c.v1) if case["has_v"] else (c.s, None)
        out = dict(rec=N(want=O.bits_to_packed(O.spikes_to_bits(s), 32), axis=0, kind="rec"), cnt=N(want=_cnt(s), axis=0, kind="cnt"))
        if v is not None:
            out["v"] = N(want=v, axis=0, kind="v")
        return out
    if form == "i8-lif":
        return dict(ptc=N(want=O.to_ptc(c.s1, 32), axis=0, kind="ptc"), cnt=N(want=_cnt(c.s1), axis=0, kind="cnt"),
                    v=N(want=c.v1, axis=0, kind="v"))
    if form == "i8-counts":
        return dict(f32=N(want=c.logits, axis=0, kind="f32"))
    if form == "fp6-lif":
        return dict(rec=N(want=O.bits_to_packed(O.spikes_to_bits(c.s1), 64), axis=0, kind="rec"), cnt=N(want=_cnt(c.s1), axis=0, kind="cnt"),
                    v=N(want=c.v1, axis=0, kind="v"))
    assert form.startswith("fp6v2"), form         # fresh LIF state, none written back
    return dict(rec=N(want=O.bits_to_packed(O.spikes_to_bits(c.s), 32), axis=0, kind="rec"), cnt=N(want=_cnt(c.s), axis=0, kind="cnt"))


# ------------------------------------------------------------------------------------------------ the listed launch's lists
def listed_unmasked(case):
    """The token state the listed case selects from: u = unmasked, t = 2, so a masked position changes (u = 0 < 1 / t) and an
    unmasked one does not (the rule of tests/test_gpu_den_mfma_oracle.py's listed test).  Masked: the positions of the first eight
    constructed threshold-grazing neurons below position 48, and position 0 of every image that has none -- EVERY image is active
    (slot s is image s), whatever count the call is then given."""
    c = oracle(case)
    B, H, W = case["geo"][9], case["geo"][7], case["geo"][8]
    unmasked = torch.ones(B, 1, H, W, dtype=torch.bool)
    for kind, ch, b, y, x in [gz for gz in c.graze if gz[3] * W + gz[4] < H * W - 1][:8]:
        unmasked[b, 0, y, x] = False
    for b in range(B):
        if bool(unmasked[b].all()):
            unmasked[b, 0, 0, 0] = False
    return unmasked


def listed_positions(case, radius=1):
    """bool [B, 49]: the positions the lists of ``radius`` hold (the masked positions dilated ``radius`` times, below position 48)
    plus the 49th, which the tail launch computes for every image below the count -- select_needed_kernel's rule on the host."""
    um = listed_unmasked(case)
    m = (~um).float()
    for _ in range(radius):
        m = torch.nn.functional.max_pool2d(m, 3, 1, 1)
    listed = m.flatten(1).bool()
    listed[:, -1] = True
    return listed
