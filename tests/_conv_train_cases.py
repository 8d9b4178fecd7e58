"""The launch forms csrc/conv_train.hip picks, mirrored on the host, and the shapes that sit on either side of each of its
thresholds.

``gather_launch`` restates gather_kind and the items / big / CN / grid arithmetic of spk_conv_train_gather; ``wgrad_launch``
restates wgrad_kind, wgrad_nwg and the LDS-form test of spk_conv_train_wgrad.  CT_BIG_ITEMS, CT_C1_ROWS_CAP and CT_C1W_CAP are
read from the source.  Every case of BOUNDARY_CASES / REGISTER_WGRAD_CASES carries the side it claims (``claim``); the GPU test
(tests/test_gpu_conv_train.py) runs the shape with poisoned outputs and the CPU test (tests/test_cabi_and_host.py) checks the
claim, so a retune of a threshold that moves a case off its boundary fails on a machine without a GPU too.

A layer tuple is (Cin, Cout, k, stride, pad, transposed, out_pad, H) for a square map or (..., H, W).  NONSQUARE_CASES: one case
per kernel and branch on maps with H != W (tests/test_gpu_conv_train_nonsquare.py, bit for bit against tests/_conv_train_oracle.py;
claims and coverage checked in tests/test_conv_train_oracle_host.py)."""
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
    cin, cout, k, s, p, tr, op = layer[:7]
    return (H - 1) * s - 2 * p + k + op if tr else (H + 2 * p - k) // s + 1


def map_size(layer):
    """(H, W) of a layer tuple (Cin, Cout, k, stride, pad, transposed, out_pad, H[, W]): eight fields mean a square map."""
    assert len(layer) in (8, 9), layer
    return layer[7], layer[8] if len(layer) == 9 else layer[7]


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
    (Cin, Cout, k, stride, pad, transposed, out_pad, H[, W]) on N images: the argument order of ops.conv_train_forward /
    _backward."""
    cin, cout, k, s, p, tr = layer[:6]
    H, W = map_size(layer)
    Ho, Wo = out_size(H, layer), out_size(W, layer)
    if op == "fwd":
        return N, H, W, cin, Ho, Wo, cout, k, s, p, 1 if tr else 0
    return N, Ho, Wo, cout, H, W, cin, k, s, p, 0 if tr else 1


def gather_launch(N, Hi, Wi, Cred, Ho, Wo, Cout, k, stride, pad, form):
    kind = gather_kind(Cred, Cout, k, stride, form)
    if kind in (2, 3):
        rows = N * Ho
        return dict(kernel="c1in" if kind == 3 else "c1out", form=form, rows=rows, grid=min(rows, CT_C1_ROWS_CAP))
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
    class_rows = [N * _cdiv(Ho - c // cs, cs) * _cdiv(Wo - c % cs, cs) for c in range(cs * cs)]
    return dict(kernel="gather", form=form, class_rows=class_rows, items=items, CNT=CNT, CN=CN, gx=gx, gy=gy, lds=lds,
                passes=_cdiv(items, gx * 8))


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
    cin, cout, k, s, p, tr = layer[:6]
    H, W = map_size(layer)
    Ho, Wo = out_size(H, layer), out_size(W, layer)
    if tr:
        return N, Ho, Wo, cout, H, W, cin, k, s, p, 2
    return N, H, W, cin, Ho, Wo, cout, k, s, p, 1


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
    lds_form, RB = False, 0
    if ntw <= 5 and Cu % 4 == 0 and Cv % 4 == 0 and aligned and Wv * stride + k >= Wu + pad:
        WP = Wv * stride + k
        for rb in (4, 3, 2, 1):
            if rb > 1 and (rb - 1) * Wv >= 24:
                continue
            need = 4 * (rb * (Wv + 1) * Cv + rb * k * WP * Cu) * 4
            if need <= 150 * 1024 and rb * Wv * Cv // 4 + rb * k * Wu * Cu // 4 <= 256 * 8:
                lds_form, RB = True, rb
                break
    split = 2 if ntw <= 5 else 1                     # (the LDS form: two halves of four waves as well)
    NR, parts = N * Hv, nwg * split
    rows_per = _cdiv(NR, parts)
    full = NR // rows_per
    short = 1 if NR % rows_per else 0
    bias_c = 0 if not bias_from else (Cv if bias_from == 1 else Cu)
    # conv_train_wgrad_lds_kernel's fuse_bias: the bias gradient summed from the staged rows (every gy row passes through LDS
    # once) instead of a second pass over gy; RB = the block height the launcher settled on (0: not the LDS form)
    fuse_bias = (lds_form and bias_from != 0 and 256 % bias_c == 0 and
                 (bias_from == 1 or (k >= pad + stride and Hu == stride * Hv)))
    return dict(kernel="wgrad_lds" if lds_form else "wgrad_reg", ntw=ntw, split=split, nwg=nwg, nwg_wanted=want, RB=RB,
                fuse_bias=fuse_bias, NR=NR, parts=parts, rows_per=rows_per, full_parts=full, short_parts=short,
                empty_parts=parts - full - short, bias_c=bias_c, bias_vec4=bias_c > 0 and bias_c % 4 == 0,
                ws_bytes=nwg * (ntile * 1024 + 64) * 4)


def launch(case):
    layer, N, op = case["layer"], case["N"], case["op"]
    if case.get("api"):                              # (the generic API convolution, not a kernel of conv_train.hip)
        return api_conv_launch(case)
    if op == "wgrad":
        args = wgrad_args(layer, N)
        if not case.get("bias", True):               # (gb_out_or_null = NULL: the entry point clears bias_from)
            args = args[:-1] + (0,)
        return wgrad_launch(*args)
    return gather_launch(*gather_args(layer, N, op))


# (Cin, Cout, k, stride, pad, transposed, out_pad, H) or (..., H, W)
ENC_CONV2 = (32, 64, 3, 2, 1, False, 0, 14)
DEC_CONVT1 = (16, 64, 3, 2, 1, True, 1, 7)
DEC_CONVT2 = (64, 32, 3, 2, 1, True, 1, 14)


def _case(id_, layer, N, op, claim, why, **extra):
    return dict(id=id_, layer=layer, N=N, op=op, claim=claim, why=why, **extra)


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


# Non-square maps (H != W), one case per kernel / branch of csrc/conv_train.hip at the smallest shape that still takes it: every
# row quantity of the kernels (Qh, Hi, Ho, Hu, Hv, N * Hv rows, the class rows) differs from its column twin here, so an exchanged
# pair changes the result (tests/test_conv_train_oracle_host.py shows that for every case on the host; the GPU runs are
# tests/test_gpu_conv_train_nonsquare.py, bit for bit against tests/_conv_train_oracle.py).  ``claim`` is on the launch the mirror
# predicts; ``bias`` False: the weight gradient without a bias gradient (gb_out_or_null = NULL).
def _gather(form, CNT, CN, class_rows):
    return lambda L: (L["kernel"], L["form"], L["CNT"], L["CN"], L["class_rows"]) == ("gather", form, CNT, CN, class_rows)


def _c1(kernel, rows):
    return lambda L: (L["kernel"], L["rows"], L["grid"]) == (kernel, rows, min(rows, CT_C1_ROWS_CAP))


def _lds(RB, bias_c, fused):
    """The LDS-staged weight gradient at block height RB: N * Hv rows that RB * parts does not divide (a ragged last block and a
    short or empty last part), the bias gradient from ``bias_c`` channels (0: none), fused or in the separate pass."""
    return lambda L: ((L["kernel"], L["RB"], L["bias_c"], L["fuse_bias"]) == ("wgrad_lds", RB, bias_c, fused) and
                      L["NR"] % (RB * L["parts"]) != 0 and L["rows_per"] > RB)


N_CN2 = (CT_BIG_ITEMS - 1) * 32 // 15 + 1            # 5x3 output maps: the first image count with CT_BIG_ITEMS items
N_ROWS_ABOVE_CAP = CT_C1_ROWS_CAP // 17 + 1          # 17 output rows per image: N * Ho = CT_C1_ROWS_CAP + 1

NONSQUARE_CASES = [
    # ---- conv_train_gather_kernel
    _case("gather_f0_s1_ragged_5x9", (8, 24, 3, 1, 1, False, 0, 5, 9), 3, "fwd", _gather(0, 1, 1, [135]),
          "form 0, stride 1, 24 of 32 columns: 135 rows, a ragged last 32-row item"),
    _case("gather_f0_s2_two_tiles_9x6", (16, 40, 3, 2, 1, False, 0, 9, 6), 5, "fwd", _gather(0, 2, 1, [75]),
          "form 0, stride 2, 9x6 -> 5x3: two column tiles (the second ragged), one per workgroup"),
    _case("gather_f1_outpad1_5x3", (16, 16, 3, 2, 1, True, 1, 5, 3), 3, "fwd", _gather(1, 1, 1, [45, 45, 45, 45]),
          "form 1 (ConvTranspose2d forward), 5x3 -> 10x6: four equal classes"),
    _case("gather_f1_outpad0_5x3", (16, 16, 3, 2, 1, True, 0, 5, 3), 3, "fwd", _gather(1, 1, 1, [45, 30, 36, 24]),
          "form 1, 5x3 -> 9x5: the odd classes one row short (5 -> 4) in one axis and one column short (3 -> 2) in the other"),
    _case("gather_f1_k2_6x4", (40, 8, 2, 2, 0, True, 0, 6, 4), 2, "fwd", _gather(1, 1, 1, [48] * 4),
          "form 1, k 2 / s 2 / p 0, 6x4 -> 12x8: one tap per class"),
    _case("gather_f1_k4_4x7", (16, 24, 4, 2, 1, True, 0, 4, 7), 2, "fwd", _gather(1, 1, 1, [56] * 4),
          "form 1, k 4 / s 2 / p 1, 4x7 -> 8x14: four taps per class"),
    _case("gather_f1_dgrad_9x6", (24, 40, 3, 2, 1, False, 0, 9, 6), 2, "dgrad", _gather(1, 1, 1, [30, 30, 24, 24]),
          "form 1 as the data gradient of a stride-2 Conv2d: gy 5x3 -> gi 9x6, classes of 5x3 and 4x3"),
    _case("gather_f0_dgrad_convT_5x3", (16, 16, 3, 2, 1, True, 1, 5, 3), 3, "dgrad", _gather(0, 1, 1, [45]),
          "form 0 at stride 2 as the data gradient of a ConvTranspose2d: gy 10x6 -> gi 5x3"),
    _case("gather_f1_s1_6x4", (16, 32, 3, 1, 1, True, 0, 6, 4), 5, "fwd", _gather(1, 1, 1, [120]),
          "form 1 with stride 1: one class"),
    _case("gather_cn2_10x6", (32, 64, 3, 2, 1, False, 0, 10, 6), N_CN2, "fwd",
          lambda L: _gather(0, 2, 2, [N_CN2 * 15])(L) and L["items"] == CT_BIG_ITEMS and L["gy"] == 1,
          "items = CT_BIG_ITEMS on 5x3 output maps: both column tiles in one wave"),
    # ---- conv_train_c1in_kernel
    _case("c1in_1ch_12x20", (1, 32, 3, 2, 1, False, 0, 12, 20), 3, "fwd", _c1("c1in", 18), "one reduced channel, 12x20 -> 6x10"),
    _case("c1in_3ch_16x10", (3, 32, 3, 2, 1, False, 0, 16, 10), 2, "fwd", _c1("c1in", 16), "three reduced channels, 16x10 -> 8x5"),
    _case("c1in_2ch_s1_7x5", (2, 16, 3, 1, 1, False, 0, 7, 5), 3, "fwd", _c1("c1in", 21), "two reduced channels at stride 1"),
    _case("c1in_dgrad_readout_6x10", (32, 3, 3, 1, 1, True, 0, 6, 10), 3, "dgrad", _c1("c1in", 18),
          "the read-out layer's data gradient: three reduced channels, form 0"),
    _case("c1in_rows_above_cap_34x20", (1, 32, 3, 2, 1, False, 0, 34, 20), N_ROWS_ABOVE_CAP, "fwd",
          _c1("c1in", CT_C1_ROWS_CAP + 1), "rows = N * Ho = CT_C1_ROWS_CAP + 1 on 17x10 output maps: workgroup 0 walks a second row"),
    # ---- conv_train_c1out_kernel
    _case("c1out_1ch_6x10", (32, 1, 3, 1, 1, True, 0, 6, 10), 3, "fwd", _c1("c1out", 18), "one output channel"),
    _case("c1out_3ch_6x10", (32, 3, 3, 1, 1, True, 0, 6, 10), 3, "fwd", _c1("c1out", 18), "three output channels"),
    _case("c1out_dgrad_2ch_7x5", (2, 16, 3, 1, 1, False, 0, 7, 5), 3, "dgrad", _c1("c1out", 21),
          "two output channels, form 1 at stride 1: the data gradient of the denoiser's first layer shape"),
    _case("c1out_rows_above_cap_17x9", (32, 1, 3, 1, 1, True, 0, 17, 9), N_ROWS_ABOVE_CAP, "fwd",
          _c1("c1out", CT_C1_ROWS_CAP + 1), "rows = CT_C1_ROWS_CAP + 1 on 17x9 maps"),
    # ---- conv_train_wgrad_lds_kernel, one case per block height
    _case("wgrad_lds_rb4_bias_v_7x5", (32, 64, 3, 2, 1, False, 0, 14, 10), 5, "wgrad", _lds(4, 64, True),
          "Wv = 5 (Hv = 7): four rows per block; bias_from = 1, fused (column sums of the staged v rows)"),
    _case("wgrad_lds_rb3_bias_u_fused_4x10", (16, 32, 3, 2, 1, True, 1, 4, 10), 20, "wgrad", _lds(3, 32, True),
          "Wv = 10 (Hv = 4), u = gy on 8x20: three rows per block; bias_from = 2 with Hu == 2 Hv, fused"),
    _case("wgrad_lds_rb2_bias_u_pass_5x14", (16, 32, 3, 2, 1, True, 0, 5, 14), 13, "wgrad", _lds(2, 32, False),
          "Wv = 14 (Hv = 5), u = gy on 9x27 (out_pad 0: Hu != 2 Hv): two rows per block; bias_from = 2 from the separate pass"),
    _case("wgrad_lds_rb1_no_bias_5x28", (8, 16, 3, 1, 1, False, 0, 5, 28), 11, "wgrad", _lds(1, 0, False),
          "Wv = 28 (Hv = 5): one row per block; no bias gradient", bias=False),
    # ---- conv_train_wgrad_kernel<NTW, 2>
    _case("wgrad_reg_bias_v_14x9", (18, 24, 3, 2, 1, False, 0, 14, 9), 5, "wgrad",
          lambda L: (L["kernel"], L["ntw"], L["bias_c"], L["bias_vec4"], L["rows_per"]) == ("wgrad_reg", 3, 24, True, 6),
          "register form (Cu = 18), v = gy on 7x5, six rows per part (parts start inside an image); bias_from = 1, 16-byte loop"),
    _case("wgrad_reg_bias_u_7x4", (24, 18, 3, 2, 1, True, 1, 7, 4), 5, "wgrad",
          lambda L: (L["kernel"], L["ntw"], L["bias_c"], L["bias_vec4"], L["rows_per"]) == ("wgrad_reg", 3, 18, False, 6),
          "register form (Cu = 18), u = gy on 14x8, v on 7x4; bias_from = 2 through the scalar loop"),
    # ---- conv_train_c1_wgrad_kernel
    _case("c1_wgrad_1ch_12x20", (1, 32, 3, 2, 1, False, 0, 12, 20), 13, "wgrad",
          lambda L: L["kernel"] == "c1_wgrad" and L["nwg"] == 4 and L["per_wg"] % 10 != 0,
          "Cu = 1, v = gy on 6x10: four workgroups whose position ranges start inside a row"),
    _case("c1_wgrad_3ch_12x20", (3, 32, 3, 2, 1, False, 0, 12, 20), 13, "wgrad",
          lambda L: L["kernel"] == "c1_wgrad" and L["nwg"] == 4 and L["per_wg"] % 10 != 0, "Cu = 3"),
]


# The layer.Conv2d / layer.ConvTranspose2d modules in train() on a [T, B, C, H, W] rectangular sequence (N = T * B images): the
# forward launch carries the claim; the host file holds these to the same bound and swap conditions as the table above.
MODULE_CASES = [
    _case("module_conv2d_9x6", (16, 40, 3, 2, 1, False, 0, 9, 6), 6, "fwd", _gather(0, 2, 1, [90]),
          "layer.Conv2d 16 -> 40, k 3 / s 2 / p 1 on [3, 2, 16, 9, 6]", T=3, B=2),
    _case("module_convT2d_5x3", (16, 16, 3, 2, 1, True, 0, 5, 3), 6, "fwd", _gather(1, 1, 1, [90, 60, 72, 48]),
          "layer.ConvTranspose2d 16 -> 16, k 3 / s 2 / p 1, out_pad 0 on [3, 2, 16, 5, 3]", T=3, B=2),
]


# ---- the generic fp32 API convolution (csrc/conv_direct.hip: conv_nchw_kernel behind spk_conv2d_fwd / spk_conv_transpose2d_fwd):
# one thread per output element on a grid capped at GRID_CAP workgroups of 256 threads, grid-stride beyond
def _api_grid_cap():
    src = open(os.path.join(os.path.dirname(SRC), "conv_direct.hip")).read()
    m = re.search(r"constexpr\s+int\s+GRID_CAP\s*=\s*([\d\s*]+);", src)
    assert m, "GRID_CAP not found in conv_direct.hip"
    cap = 1
    for f in m.group(1).split("*"):
        cap *= int(f)
    return cap


API_GRID_CAP = _api_grid_cap()


def api_conv_launch(case):
    """Outputs, workgroups and grid-stride trips of the API convolution of ``case`` (spk_grid(total, GRID_CAP))."""
    layer, N = case["layer"], case["N"]
    H, W = map_size(layer)
    total = N * layer[1] * out_size(H, layer) * out_size(W, layer)
    grid = max(1, min(_cdiv(total, 256), API_GRID_CAP))
    return dict(kernel="api_conv", total=total, grid=grid, passes=_cdiv(total, grid * 256), map=(H, W))


def _api(transposed, k, s, p):
    layer = (5, 3, k, s, p, True, 0, 4, 7) if transposed else (3, 5, k, s, p, False, 0, 7, 10)
    return _case(f"api_{'convT' if transposed else 'conv'}_k{k}s{s}p{p}", layer, 2, "fwd",
                 lambda L: L["passes"] == 1 and L["map"][0] != L["map"][1], "non-square, one trip; run with and without bias", api=True)


API_CONV_CASES = [_api(tr, k, s, p) for tr in (False, True) for k, s, p in ((3, 2, 1), (2, 2, 0), (4, 2, 1))] + [
    _case("api_conv_1x1_past_grid_cap", (1, 3, 1, 1, 0, False, 0, 64, 63), 347, "fwd",
          lambda L: L["grid"] == API_GRID_CAP and L["passes"] == 2 and 0 < L["total"] - API_GRID_CAP * 256 <= 64 * 63,
          "1x1, one input channel, 64 x 63 maps: just above GRID_CAP * 256 outputs, the first threads take a second element", api=True),
]


def check_claims(cases):
    """[(id, launch description)] of the cases whose shape does not land where the case says it does."""
    return [(c["id"], launch(c)) for c in cases if not c["claim"](launch(c))]
