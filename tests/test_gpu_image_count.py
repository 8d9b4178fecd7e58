"""The device-side image count (``n_dyn_or_null``) from BOTH sides, on every kernel that reads it (the census and the case table of
tests/_image_count_cases.py; tests/test_image_count_cases_host.py holds both to the sources and shows that no sentinel is a legal
output).  Each run is ONE call of the C-ABI into caller-owned buffers prefilled with a sentinel, with the real inputs of ALL B images
in place and the count in device memory.  After it:

  (a) the images below the count equal the exact host oracle bit for bit -- spikes or records, spike counts, the carried v, the BN
      output where the entry has one (MODE_MEAN: within the oracle module's derived read-out bound);
  (b) every byte of every output of the images at or past the count is still the sentinel;
  (c) their carried v is still v0;
  (d) fp6v2: the flag workspace comes back clean and word 1 counts at least the constructed threshold-grazing neurons of the images
      below the count.

csrc/cert_common.h leaves the id of a flagged neuron to the caller (it states no id -> image map), so no test reads the id list.
A count of 0 writes nothing at all: (a) is empty and (b) covers the whole buffer."""
import pytest
import torch

import _conv_bn_lif_oracle as O
import _image_count_cases as ic

pytestmark = pytest.mark.gpu

FLAG_LIST = 1 << 20          # id-list entries of a certified kernel's workspace: [count, published count, ids..., bitmap, ticket]
_DEV = {}                    # case id -> its device-side inputs (built once)
_WS = {}                     # (B, Cout, H, W) -> flag workspace of the fp6v2 calls (one stream: one workspace per shape)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _same(got, want, what):
    """torch.equal with the mismatch pattern in the message."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    if not torch.equal(got, want):
        bad = got != want
        raise AssertionError((what, f"{int(bad.sum())} of {want.numel()} differ; first at", bad.nonzero()[:8].tolist()))


def _bits(t):
    """fp32 compared as its bits (the sentinel is NaN); bytes as they are."""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _u8(t):
    return t.view(torch.uint8) if t.dtype == torch.int8 else t


def _count(dev, n):
    """[count, work word] as ops.active_set carries it; None: the call has no count."""
    return None if n is None else torch.tensor([n, 0], dtype=torch.int32, device=dev)


def _flag_ws(dev, case):
    from spkdiff._lib import lib
    Cout, H, W, B = case["geo"][1], case["geo"][7], case["geo"][8], case["geo"][9]
    key = (B, Cout, H, W)
    if key not in _WS:
        _WS[key] = torch.zeros(lib.spk_den_fp6v2_flag_words(B, Cout, H, W), dtype=torch.int32, device=dev)
    return _WS[key]


def _flag_ws_clean(v):
    """Live counter zero, overflow bitmap and hand-over ticket zero (the rule of tests/test_gpu_parity.py)."""
    return int(v[0]) == 0 and int(v[2 + FLAG_LIST:].abs().sum()) == 0


def _graze_outside_tail(c, n_img, listed=None):
    """Constructed threshold-grazing neurons of the images below the count that the MAIN launch decides (the tail computes the last
    position of a 7x7 map itself): each must be flagged."""
    H, W = c.geo[7], c.geo[8]
    n = 0
    for kind, ch, b, y, x in c.graze:
        p = y * W + x
        if ((H * W) % 2 and p == H * W - 1) or b >= n_img or (listed is not None and not bool(listed[b, p])):
            continue
        n += 1
    return n


def _prefill(dev, case):
    """{name: (device buffer, its host copy)} -- every output of the call, sentinel-filled (the carried v: v0)."""
    c = ic.oracle(case)
    bufs = {}
    for name, e in ic.expected(case).items():
        if e.kind == "v":
            host = c.v0.clone()
        elif e.want.dtype == torch.uint8:
            host = torch.full(e.want.shape, ic.U8_SENTINEL, dtype=torch.uint8)
        else:
            host = torch.full(e.want.shape, float("nan"), dtype=torch.float32)
        bufs[name] = (host.to(dev), host)
    return bufs


def _inputs(ops, dev, case):
    """The case's inputs and packed weights on the device, all B images real."""
    if case["id"] in _DEV:
        return _DEV[case["id"]]
    c, form, geo = ic.oracle(case), case["form"], case["geo"]
    d = dict(a=c.a.to(dev), b=c.b.to(dev))
    if form in ("ptc-lif", "ptc-mean", "seq-raw", "tinv"):
        d["wp"], d["bias"] = ops.pack_conv_weight(c.w.to(dev), bool(geo[5])), c.bias.to(dev)
        C0 = case["row"][0] if form == "ptc-mean" else geo[0]
        if form == "seq-raw" or form == "tinv":
            d["in0"], d["in1"] = c.x.to(dev), None
        else:
            d["in0"] = O.to_ptc(c.x[:, :, :C0].contiguous()).to(dev)
            d["in1"] = O.to_ptc(c.x[:, :, C0:].contiguous()).to(dev) if C0 < geo[0] else None
        d["C0"], d["C1"] = C0, geo[0] - C0
    elif form == "i8-lif":
        d["pk"] = ops.den_pack_weight_i8(c.w.to(dev), c.bias.to(dev))
        d["in0"] = O.to_ptc(c.x, 32).to(dev)
    elif form == "i8-counts":
        C0 = case["row"][0]
        d["pk"] = ops.den_pack_weight_i8(c.w.to(dev), c.bias.to(dev))
        d["in0"] = O.to_counts(c.x[:, :, :C0].contiguous()).to(dev)
        d["in1"] = O.to_counts(c.x[:, :, C0:].contiguous()).to(dev) if C0 < geo[0] else None
    elif form == "fp6-lif":
        d["pk"] = ops.den_pack_weight_fp6(c.w.to(dev), c.bias.to(dev))
        d["in0"] = O.bits_to_packed(O.spikes_to_bits(c.x), 64).to(dev)
    else:
        d["pk"] = ops.den_pack_weight_fp6v2(c.w.to(dev), c.bias.to(dev))
        d["in0"] = O.bits_to_packed(O.spikes_to_bits(c.x), 32).to(dev)
    torch.cuda.synchronize()
    _DEV[case["id"]] = d
    return d


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(ops, dev, case, d, bufs, cnt, part=None):
    """The case's one call of the C-ABI on torch's current stream; returns its status."""
    from spkdiff._lib import lib
    form, geo = case["form"], case["geo"]
    Cin, Cout, k, s, pad, tr, op, H, W, B = geo
    p, n_ptr, st = _ptr, _ptr(cnt), ops._stream(d["in0"])
    o = {name: b[0] for name, b in bufs.items()}
    if form in ("ptc-lif", "ptc-mean", "seq-raw", "tinv"):
        in_kind = {"ptc-lif": ops.IN_PTC, "ptc-mean": ops.IN_PTC, "seq-raw": ops.IN_SEQ, "tinv": ops.IN_TINV}[form]
        mode = {"ptc-lif": ops.MODE_LIF, "ptc-mean": ops.MODE_MEAN, "seq-raw": ops.MODE_RAW, "tinv": ops.MODE_LIF}[form]
        lif = mode == ops.MODE_LIF
        out_ptc = o.get("ptc") if form == "ptc-lif" else o.get("rec")
        return lib.spk_conv_fused_fwd(p(d["in0"]), p(d["in1"]), d["C0"], d["C1"], in_kind, p(d["wp"]), p(d["bias"]),
                                      p(d["a"]) if lif else None, p(d["b"]) if lif else None, p(o.get("v")), p(out_ptc), p(o.get("f32")),
                                      p(o.get("pre")), None, None, 0, mode, 16, B, H, W, Cout, k, s, pad, int(tr), op, 0, 0,
                                      ops.CHUNK_S32 if form == "tinv" else 0, p(o.get("cnt")), n_ptr, st)
    if form == "i8-lif":
        wq, scale, bias_d = d["pk"]
        return lib.spk_den_conv3x3_mfma(p(d["in0"]), Cin // 32, None, 0, p(wq), p(scale), p(bias_d), p(d["a"]), p(d["b"]), p(o["v"]),
                                        p(o["ptc"]), p(o["cnt"]), None, ops.MODE_LIF, 16, B, H, W, Cout, n_ptr, st)
    if form == "i8-counts":
        wq, scale, bias_d = d["pk"]
        C0 = d["in0"].shape[1]
        return lib.spk_den_conv3x3_counts_mfma(p(d["in0"]), C0, p(d["in1"]), Cin // 32 - C0, p(wq), p(scale), p(bias_d), p(o["f32"]), 16,
                                               B, H, W, Cout, n_ptr, st)
    if form == "fp6-lif":
        wq, scale, bias_d = d["pk"]
        return lib.spk_den_conv3x3_mfma_fp6(p(d["in0"]), Cin // 64, p(wq), p(scale), p(bias_d), p(d["a"]), p(d["b"]), p(o["v"]),
                                            p(o["rec"]), p(o["cnt"]), 16, B, H, W, Cout, n_ptr, st)
    wq, scale, bias_d, wl1, qtab = d["pk"]
    head = (p(d["in0"]), Cin // 32, p(wq), p(scale), p(bias_d), p(wl1), p(qtab), p(d["a"]), p(d["b"]), p(o["rec"]), p(o["cnt"]),
            p(_flag_ws(dev, case)), 16, B, H, W, Cout, n_ptr)
    if part is not None:
        return lib.spk_den_conv3x3_mfma_fp6v2_part(*head, int(part), int(case["cap"]), st)
    if form == "fp6v2-listed":
        need = d["need"]
        return lib.spk_den_conv3x3_mfma_fp6v2_listed(*head, p(need.buf), need.radii, 1, int(case["cap"]), st)
    return lib.spk_den_conv3x3_mfma_fp6v2(*head, int(case["cap"]), int(case.get("v2_form", 0)), st)


def _check(case, n, bufs, mask=None):
    """(a), (b), (c) on every output.  mask: bool [B, positions] of the positions the call computes (the listed launch); the other
    positions of the images below the count stay the sentinel as well."""
    B = case["geo"][9]
    n = B if n is None else n
    for name, e in ic.expected(case).items():
        got = bufs[name][0].cpu().movedim(e.axis, 0)
        fill = bufs[name][1].movedim(e.axis, 0)
        want = e.want.movedim(e.axis, 0)
        what = (case["id"], "count", n, name)
        if e.kind == "mean":
            err = (got[:n].double() - want[:n]).abs()
            print(f"{what}: max err {float(err.max()) if n else 0.0:.3e}, bound up to {float(e.bound.max()):.3e}")
            assert bool((err <= e.bound[:n]).all()), (what, "exceeds the read-out bound", float((err - e.bound[:n]).max()))
        elif mask is None:
            _same(got[:n], want[:n], what + ("below the count",))
        else:                                      # records [B,G,H,W,16,16] / counts [B,G,H,W,32]: positions on axes 2, 3
            m = mask.view(B, 1, *want.shape[2:4], *([1] * (want.dim() - 4))).expand_as(want)
            _same(got[:n][m[:n]], want[:n][m[:n]], what + ("listed positions below the count",))
            _same(got[:n][~m[:n]], fill[:n][~m[:n]], what + ("unlisted positions below the count: untouched",))
        _same(_bits(got[n:]), _bits(fill[n:]), what + ("at or past the count: untouched",))


RUNS = [r for r in ic.runs() if ic.BY_ID[r[0]]["form"] not in ("fp6v2-listed", "fp6v2-part4")]


@pytest.mark.parametrize("cid,n", RUNS, ids=[f"{c}-n{n}" for c, n in RUNS])
def test_images_past_the_count_stay_untouched(dev, ops, cid, n):
    case = ic.BY_ID[cid]
    assert all(case["reach"](_cus()).values()), ("the case does not reach the sites it names on this device", case["reach"](_cus()))
    d = _inputs(ops, dev, case)
    bufs = _prefill(dev, case)
    cnt = _count(dev, n)
    rc = _call(ops, dev, case, d, bufs, cnt)
    torch.cuda.synchronize()
    assert rc == 0, f"{case['entry']} returned {rc}"
    if cnt is not None:
        assert cnt.cpu().tolist() == [n, 0], "the count tensor is read, never written"
    _check(case, n, bufs)
    if case["family"] == "fp6v2":
        ws = _flag_ws(dev, case).cpu()
        B = case["geo"][9]
        need = _graze_outside_tail(ic.oracle(case), B if n is None else n)
        assert _flag_ws_clean(ws), "live counter, overflow bitmap and hand-over ticket come back clean"
        assert int(ws[1]) >= need, ("flagged", int(ws[1]), "constructed neurons below the count", need)
        assert need >= 1 or n not in (None, B), "the whole batch holds constructed neurons"
        assert n != 0 or int(ws[1]) == 0, "a count of 0 flags nothing"


@pytest.mark.parametrize("n", ic.COUNTS_B5)
def test_listed_launch_follows_a_count_lowered_after_its_lists_were_built(dev, ops, n):
    """spk_den_conv3x3_mfma_fp6v2_listed: the position lists are built with all five images active (slot s is image s), THEN the
    count is lowered.  Listed positions and the 49th of the images below the count equal the oracle; their unlisted positions and
    every byte of the images at or past the count stay the sentinel -- the main launch walks the lists, which still name all five."""
    case = ic.BY_ID["fp6v2-listed"]
    assert all(case["reach"](_cus()).values())
    B = case["geo"][9]
    d = _inputs(ops, dev, case)
    um = ic.listed_unmasked(case).to(dev)
    ud = um.float()                                               # 0 where a change is wanted, 1 elsewhere
    act = ops.select_active(um, 2, ud)
    need = d["need"] = ops.select_needed(um, 2, act, ops.NeedLists(B, 4, dev), ud)
    assert act[1].cpu().tolist() == [B, 0] and act[0].cpu().tolist() == list(range(B)), "every image is active"
    listed = ic.listed_positions(case)
    rec = need.records(1).cpu()
    for s in range(B):
        got = torch.zeros(49, dtype=torch.bool)
        got[rec[s, :int(rec[s, 48])].long()] = True
        got[48] = True
        assert torch.equal(got, listed[s]), ("the device's lists differ from the host rule", s)
    act[1][:1].fill_(n)                                           # ... and only now the count
    bufs = _prefill(dev, case)
    rc = _call(ops, dev, case, d, bufs, act[1])
    torch.cuda.synchronize()
    assert rc == 0, f"spk_den_conv3x3_mfma_fp6v2_listed returned {rc}"
    _check(case, n, bufs, mask=listed)
    ws = _flag_ws(dev, case).cpu()
    n_graze = _graze_outside_tail(ic.oracle(case), n, listed=listed)
    assert _flag_ws_clean(ws) and int(ws[1]) >= n_graze, ("flagged", int(ws[1]), "constructed neurons on listed positions", n_graze)
    assert n < B or n_graze >= 1, "the whole batch holds constructed neurons on listed positions"
    assert n != 0 or int(ws[1]) == 0, "a count of 0 flags nothing"


@pytest.mark.parametrize("n", ic.COUNTS_B5)
def test_last_position_part_follows_the_count(dev, ops, n):
    """spk_den_conv3x3_mfma_fp6v2_part, part 4 (fp6v2_tail_kernel<7, 7, 2>: the wide form of the last-position body): after a main
    call, the last position of ALL images is re-filled with the sentinel and part 4 re-run under the same count -- the images below
    the count get it back, the others keep the sentinel."""
    case = ic.BY_ID["fp6v2-part4"]
    assert all(case["reach"](_cus()).values())
    d = _inputs(ops, dev, case)
    bufs = _prefill(dev, case)
    cnt = _count(dev, n)
    main = dict(case, form="fp6v2", v2_form=0)
    assert _call(ops, dev, main, d, bufs, cnt) == 0
    torch.cuda.synchronize()
    _check(case, n, bufs)
    for name in ("rec", "cnt"):
        bufs[name][0][:, :, 6, 6] = ic.U8_SENTINEL
        got = bufs[name][0].cpu()
        assert bool((got[:, :, 6, 6] == ic.U8_SENTINEL).all()) and (n == 0 or not torch.equal(got[:n], ic.expected(case)[name].want[:n]))
    rc = _call(ops, dev, case, d, bufs, cnt, part=4)
    torch.cuda.synchronize()
    assert rc == 0, f"spk_den_conv3x3_mfma_fp6v2_part returned {rc}"
    _check(case, n, bufs)
    assert _flag_ws_clean(_flag_ws(dev, case).cpu())


def test_a_captured_graph_reads_the_count_at_replay(dev, ops):
    """One fp6v2 call and one int8 call captured (single stream, after a warm-up) with the count tensor holding 4.  Outputs re-filled
    with the sentinel, 1 written into the count tensor, replay: exactly image 0 is written and equals the oracle.  5, replay: all
    five.  The count lives in device memory and is read when the kernels run, not when they were captured."""
    v2, i8 = ic.BY_ID["fp6v2-96-64-7x7-form0-cap-1"], ic.BY_ID["i8-lif"]
    cnt = _count(dev, 4)
    runs = [(c, _inputs(ops, dev, c), _prefill(dev, c)) for c in (v2, i8)]
    _flag_ws(dev, v2)                                             # (allocated ahead of the capture)
    for c, d, bufs in runs:                                       # warm-up
        assert _call(ops, dev, c, d, bufs, cnt) == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c, d, bufs in runs:
            assert _call(ops, dev, c, d, bufs, cnt) == 0
    for n in (1, 5, 0, 4):
        for c, d, bufs in runs:
            for dbuf, host in bufs.values():
                dbuf.copy_(host)
        cnt[:1].fill_(n)
        g.replay()
        torch.cuda.synchronize()
        for c, d, bufs in runs:
            _check(c, n, bufs)
        assert _flag_ws_clean(_flag_ws(dev, v2).cpu())
