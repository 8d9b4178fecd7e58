"""The launch forms csrc/conv_train.hip picks, mirrored on the host, and the shapes that sit on either side of each of its
thresholds.

``gather_launch`` restates gather_kind and the items / big / CN / grid arithmetic of spk_conv_train_gather; ``wgrad_launch``
restates wgrad_kind, wgrad_nwg and the LDS-form test of spk_conv_train_wgrad.  CT_BIG_ITEMS, CT_C1_ROWS_CAP and CT_C1W_CAP are
read from the source.  Every case of BOUNDARY_CASES / REGISTER_WGRAD_CASES carries the side it claims (``claim``); the GPU test
(tests/test_gpu_conv_train.py) runs the shape with poisoned outputs and the CPU test (tests/test_cabi_and_host.py) checks the
claim, so a retune of a threshold that moves a case off its boundary fails on a machine without a GPU too."""
import os
import re

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spiking-diffusion_amd", "csrc",
                   "conv_train.hip")


def _constant(name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", open(SRC).read())
    assert m, f"{name} not found in {SRC}"
    return int(m.group(1))


CT_BIG_ITEMS = _constant("CT_BIG_ITEMS")
CT_C1_ROWS_CAP = _constant("CT_C1_ROWS_CAP")
CT_C1W_CAP = _constant("CT_C1W_CAP")
GATHER_LDS_MAX = 150 * 1024
WGRAD_NWG_CAP = 256                          # (kind 1: wgrad_nwg)


def _cdiv(a, b):
    return -(-a // b)


def out_size(H, layer):
    cin, cout, k, s, p, tr, op, _ = layer
    return (H - 1) * s - 2 * p + k + op if tr else (H + 2 * p - k) // s + 1


def gather_kind(Cred, Cout, k, stride, form):
    if k < 1 or k * k > 16 or stride < 1 or Cred < 1 or Cout < 1:
        return 0
    if Cred <= 4:
        return 3 if (not form and Cout % 4 == 0 and k * k * Cred * Cout * 4 <= 64 * 1024) else 0
    if Cout <= 4:
        if form and stride != 1:
            return 0
        return 2 if Cred in (8, 16, 32, 64) else 0
    if Cred % 8 or Cred > 64 or Cout > 64:
        return 0
    if stride > 4 or (form and stride > 2) or k * k * Cred * 32 * 4 > GATHER_LDS_MAX:
        return 0
    return 1


def gather_args(layer, N, op):
    """(N, Hi, Wi, Cred, Ho, Wo, Cout, k, stride, pad, form) of the gather launch of ``op`` ('fwd' or 'dgrad') of ``layer`` =
    (Cin, Cout, k, stride, pad, transposed, out_pad, H) on N images: the argument order of ops.conv_train_forward / _backward."""
    cin, cout, k, s, p, tr, _, H = layer
    Ho = out_size(H, layer)
    if op == "fwd":
        return N, H, H, cin, Ho, Ho, cout, k, s, p, 1 if tr else 0
    return N, Ho, Ho, cout, H, H, cin, k, s, p, 0 if tr else 1


def gather_launch(N, Hi, Wi, Cred, Ho, Wo, Cout, k, stride, pad, form):
    kind = gather_kind(Cred, Cout, k, stride, form)
    if kind in (2, 3):
        rows = N * Ho
        return dict(kernel="c1in" if kind == 3 else "c1out", rows=rows, grid=min(rows, CT_C1_ROWS_CAP))
    assert kind == 1, "shape not taken by the gather kernels"
    cs = stride if form else 1
    CNT = _cdiv(Cout, 32)
    items = sum(_cdiv(N * _cdiv(Ho - c // cs, cs) * _cdiv(Wo - c % cs, cs), 32) for c in range(cs * cs))
    big = CNT == 1 or (items >= CT_BIG_ITEMS and k * k * Cred * CNT * 32 * 4 <= GATHER_LDS_MAX)
    CN = CNT if big else 1
    gy = 1 if big else CNT
    lds = k * k * Cred * CN * 32 * 4
    per_cu = 1 if lds > 76 * 1024 else 2
    gx = min(_cdiv(items, 8), max(256 * per_cu // gy, 1))
    return dict(kernel="gather", items=items, CNT=CNT, CN=CN, gx=gx, gy=gy, lds=lds, passes=_cdiv(items, gx * 8))


def wgrad_kind(Cu, Cv, k):
    if k < 1 or k * k > 16 or Cu < 1 or Cv < 1:
        return 0
    if Cu <= 4:
        CQ = Cv // 4
        cq_ok = Cv % 4 == 0 and CQ in (1, 2, 4, 8, 16)
        return 2 if (cq_ok and (Cu == 1 or k <= 3) and 4 * (k * k * Cu + 1) * Cv * 4 <= 64 * 1024) else 0
    if Cu > 64 or Cv > 64:
        return 0
    return 1 if k * k * _cdiv(Cu, 32) * _cdiv(Cv, 32) <= 36 else 0


def wgrad_args(layer, N):
    """(N, Hu, Wu, Cu, Hv, Wv, Cv, k, stride, pad, bias_from) of ``layer``'s weight gradient, as ops.conv_train_backward
    assigns the roles (u = the tensor on the finer grid)."""
    cin, cout, k, s, p, tr, _, H = layer
    Ho = out_size(H, layer)
    if tr:
        return N, Ho, Ho, cout, H, H, cin, k, s, p, 2
    return N, H, H, cin, Ho, Ho, cout, k, s, p, 1


def wgrad_launch(N, Hu, Wu, Cu, Hv, Wv, Cv, k, stride, pad, bias_from, aligned=True):
    kind = wgrad_kind(Cu, Cv, k)
    assert kind, "shape not taken by the weight-gradient kernels"
    Ms = N * Hv * Wv
    want = _cdiv(Ms, 64) if kind == 1 else _cdiv(Ms, 256)
    nwg = max(1, min(want, WGRAD_NWG_CAP if kind == 1 else CT_C1W_CAP))
    if kind == 2:
        return dict(kernel="c1_wgrad", nwg=nwg, nwg_wanted=want, per_wg=_cdiv(Ms, nwg),
                    ws_bytes=nwg * ((k * k * Cu + 1) * Cv + 8) * 4)
    ntile = k * k * _cdiv(Cu, 32) * _cdiv(Cv, 32)
    ntw = _cdiv(ntile, 4)
    lds_form = False
    if ntw <= 5 and Cu % 4 == 0 and Cv % 4 == 0 and aligned and Wv * stride + k >= Wu + pad:
        WP = Wv * stride + k
        for RB in (4, 3, 2, 1):
            if RB > 1 and (RB - 1) * Wv >= 24:
                continue
            need = 4 * (RB * (Wv + 1) * Cv + RB * k * WP * Cu) * 4
            if need <= 150 * 1024 and RB * Wv * Cv // 4 + RB * k * Wu * Cu // 4 <= 256 * 8:
                lds_form = True
                break
    split = 2 if ntw <= 5 else 1                     # (the LDS form: two halves of four waves as well)
    NR, parts = N * Hv, nwg * split
    rows_per = _cdiv(NR, parts)
    full = NR // rows_per
    short = 1 if NR % rows_per else 0
    bias_c = 0 if not bias_from else (Cv if bias_from == 1 else Cu)
    return dict(kernel="wgrad_lds" if lds_form else "wgrad_reg", ntw=ntw, split=split, nwg=nwg, nwg_wanted=want,
                rows_per=rows_per, full_parts=full, short_parts=short, empty_parts=parts - full - short,
                bias_c=bias_c, bias_vec4=bias_c > 0 and bias_c % 4 == 0, ws_bytes=nwg * (ntile * 1024 + 64) * 4)


def launch(case):
    layer, N, op = case["layer"], case["N"], case["op"]
    if op == "wgrad":
        return wgrad_launch(*wgrad_args(layer, N))
    return gather_launch(*gather_args(layer, N, op))


# (Cin, Cout, k, stride, pad, transposed, out_pad, H)
ENC_CONV2 = (32, 64, 3, 2, 1, False, 0, 14)
DEC_CONVT1 = (16, 64, 3, 2, 1, True, 1, 7)
DEC_CONVT2 = (64, 32, 3, 2, 1, True, 1, 14)


def _case(id_, layer, N, op, claim, why):
    return dict(id=id_, layer=layer, N=N, op=op, claim=claim, why=why)


# shapes on both sides of the thresholds of spk_conv_train_gather / spk_conv_train_wgrad
BOUNDARY_CASES = [
    _case("form0_items_below_big", (32, 64, 3, 2, 1, False, 0, 10), 2620, "fwd",
          lambda L: L["items"] == CT_BIG_ITEMS - 1 and L["CN"] == 1 and L["gy"] == 2,
          "regular gather, 5x5 map: items = CT_BIG_ITEMS - 1, one column tile per workgroup, two column workgroups"),
    _case("form0_items_at_big", (32, 64, 3, 2, 1, False, 0, 10), 2621, "fwd",
          lambda L: L["items"] == CT_BIG_ITEMS and L["CN"] == 2 and L["gy"] == 1,
          "regular gather: items = CT_BIG_ITEMS, both column tiles in one wave"),
    _case("form1_items_below_big", DEC_CONVT1, 333, "fwd",
          lambda L: L["items"] < CT_BIG_ITEMS and L["CN"] == 1 and L["gy"] == 2,
          "sub-pixel gather (dec.convT1 forward): items = CT_BIG_ITEMS - 8 (four equal classes), the largest count below"),
    _case("form1_items_at_big", DEC_CONVT1, 334, "fwd",
          lambda L: L["items"] == CT_BIG_ITEMS and L["CN"] == 2 and L["gy"] == 1,
          "sub-pixel gather (dec.convT1 forward): items = CT_BIG_ITEMS"),
    _case("cn2_147KB_weights", (64, 64, 3, 1, 1, False, 0, 14), 336, "fwd",
          lambda L: L["CN"] == 2 and L["lds"] == 147456 and L["gx"] == 256 and L["passes"] == 2,
          "CN = 2 with all 9 x 64 x 64 taps in LDS: one workgroup per CU, grid capped at 256, some waves walk two items"),
    _case("gather_two_passes", DEC_CONVT2, 200, "fwd",
          lambda L: L["CN"] == 1 and L["gx"] == 512 and L["passes"] == 2,
          "dec.convT2 forward: more items than waves on the 512-workgroup grid"),
    _case("c1in_rows_at_cap", (1, 32, 3, 2, 1, False, 0, 32), 256, "fwd",
          lambda L: L["kernel"] == "c1in" and L["rows"] == CT_C1_ROWS_CAP == L["grid"],
          "one-channel input gather: rows = CT_C1_ROWS_CAP, one row per workgroup"),
    _case("c1in_rows_above_cap", (1, 32, 3, 2, 1, False, 0, 34), 241, "fwd",
          lambda L: L["kernel"] == "c1in" and L["rows"] == CT_C1_ROWS_CAP + 1 and L["grid"] == CT_C1_ROWS_CAP,
          "one-channel input gather: rows = CT_C1_ROWS_CAP + 1, workgroup 0 walks a second row"),
    _case("c1out_rows_at_cap", (32, 1, 3, 1, 1, True, 0, 16), 256, "fwd",
          lambda L: L["kernel"] == "c1out" and L["rows"] == CT_C1_ROWS_CAP == L["grid"],
          "one-channel output gather (read-out forward): rows = CT_C1_ROWS_CAP"),
    _case("c1out_rows_above_cap", (32, 1, 3, 1, 1, True, 0, 17), 241, "fwd",
          lambda L: L["kernel"] == "c1out" and L["rows"] == CT_C1_ROWS_CAP + 1 and L["grid"] == CT_C1_ROWS_CAP,
          "one-channel output gather: rows = CT_C1_ROWS_CAP + 1"),
    _case("c1_wgrad_below_cap", (1, 32, 3, 2, 1, False, 0, 32), CT_C1W_CAP - 1, "wgrad",
          lambda L: L["kernel"] == "c1_wgrad" and L["nwg"] == L["nwg_wanted"] == CT_C1W_CAP - 1,
          "few-channel weight gradient: one workgroup short of CT_C1W_CAP"),
    _case("c1_wgrad_above_cap", (1, 32, 3, 2, 1, False, 0, 32), CT_C1W_CAP + 1, "wgrad",
          lambda L: L["kernel"] == "c1_wgrad" and L["nwg_wanted"] == CT_C1W_CAP + 1 and L["nwg"] == CT_C1W_CAP,
          "few-channel weight gradient: one workgroup more than CT_C1W_CAP wanted"),
    _case("wgrad_lds_cap_ragged_enc_conv2", ENC_CONV2, 600, "wgrad",
          lambda L: L["kernel"] == "wgrad_lds" and L["nwg"] == 256 and L["short_parts"] == 1 and L["empty_parts"] > 0,
          "LDS-staged weight gradient at the 256-workgroup cap: one part short, the last parts empty"),
    _case("wgrad_lds_cap_ragged_dec_convT2", DEC_CONVT2, 600, "wgrad",
          lambda L: L["kernel"] == "wgrad_lds" and L["nwg"] == 256 and L["short_parts"] == 1 and L["empty_parts"] > 0,
          "LDS-staged weight gradient (u = gy on the finer grid) at the cap with short and empty parts"),
]

# conv_train_wgrad_kernel<NTW, 2> (the register form): Cu or Cv not a multiple of 4 keeps a shape off the LDS form; each NTW
# 1..5, both bias sources (1: column sums of v = gy of a Conv2d, 2: of u = gy of a ConvTranspose2d), scalar (C % 4 != 0) and
# 16-byte (C % 4 == 0) bias loops
REGISTER_WGRAD_CASES = [
    _case("ntw1_conv_bias_scalar", (24, 18, 1, 1, 0, False, 0, 14), 64, "wgrad",
          lambda L: (L["ntw"], L["bias_c"], L["bias_vec4"]) == (1, 18, False), "k = 1, one tile"),
    _case("ntw2_convT_bias_vec4", (22, 36, 2, 2, 0, True, 0, 7), 64, "wgrad",
          lambda L: (L["ntw"], L["bias_c"], L["bias_vec4"]) == (2, 36, True), "k = 2, two u tiles"),
    _case("ntw3_conv_bias_vec4", (18, 24, 3, 2, 1, False, 0, 14), 64, "wgrad",
          lambda L: (L["ntw"], L["bias_c"], L["bias_vec4"]) == (3, 24, True), "k = 3, one tile"),
    _case("ntw3_convT_bias_scalar", (24, 18, 3, 2, 1, True, 1, 7), 64, "wgrad",
          lambda L: (L["ntw"], L["bias_c"], L["bias_vec4"]) == (3, 18, False), "k = 3, one tile"),
    _case("ntw4_convT_bias_vec4", (18, 24, 4, 2, 1, True, 0, 7), 64, "wgrad",
          lambda L: (L["ntw"], L["bias_c"], L["bias_vec4"]) == (4, 24, True), "k = 4, one tile"),
    _case("ntw5_conv_bias_scalar_cap", (40, 22, 3, 1, 1, False, 0, 9), 600, "wgrad",
          lambda L: ((L["ntw"], L["bias_c"], L["bias_vec4"], L["nwg"]) == (5, 22, False, 256) and L["short_parts"] == 1
                     and L["empty_parts"] > 0), "k = 3, two u tiles, at the workgroup cap with short and empty parts"),
]
for _c in REGISTER_WGRAD_CASES:
    _c["claim"] = (lambda f: lambda L: L["kernel"] == "wgrad_reg" and L["split"] == 2 and f(L))(_c["claim"])


def check_claims(cases):
    """[(id, launch description)] of the cases whose shape does not land where the case says it does."""
    return [(c["id"], launch(c)) for c in cases if not c["claim"](launch(c))]
