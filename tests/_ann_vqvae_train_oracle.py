"""fp64 restatement of ONE training iteration of the plain-CNN VQVAE baseline (R/snn_model/vae_model.py:548-672 in train() mode,
R/main.py:130-142) GIVEN the decisions, the teacher-forced layer check that justifies those decisions, the counted round-off
bounds of the quantiser / loss kernels, and the case tables the host and the GPU tests share.  No device code.

ReLU is a discontinuity of the gradient and the arg min a discontinuity of everything, so an fp64 run that makes its own
decisions measures the decisions of the path under test and not its round-off.  ``train64`` is therefore handed the decisions of
the path it judges (which units the four ReLUs pass, which code every row takes) -- tests/_bn_lif_train_oracle.py does the
same with the kernel's spike decisions -- and ``check_decisions`` shows that every decision it was handed is one an exact run
could not tell from its own: each saved activation is recomputed in fp64 from the saved activation below it, must lie within
the counted forward bound of an fp32 dot product, a mask may differ from ``preact64 > 0`` only where |preact64| is within that
bound, and an index must satisfy F20's tau rule.
"""
import functools
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import _ann_vqvae_oracle as orc
import _conv_train_cases as ctc
from spkdiff import _lib, synth

SRC = os.path.join(os.path.dirname(ctc.SRC), "ann_vqvae_train.hip")

EPS = 2.0 ** -24                  # unit round-off of fp32
D = 16                            # embedding_dim of every case (SPK_ANN_VQVAE_D)
PARAMS = ("encoder.convs.0", "encoder.convs.2", "encoder.convs.4", "decoder.convs.0", "decoder.convs.2", "decoder.convs.4")
# (transposed, stride, pad, out_pad, ReLU behind it) of the six layers, in PARAMS order
LAYERS = ((False, 2, 1, 0, True), (False, 2, 1, 0, True), (False, 1, 0, 0, False),
          (True, 2, 1, 1, True), (True, 2, 1, 1, True), (True, 1, 1, 0, False))
MASKS = ("a1", "a2", "d1", "d2")  # the saved post-ReLU activations, in forward order


def _conv(x, w, b, layer):
    tr, s, p, op, _ = layer
    return F.conv_transpose2d(x, w, b, s, p, op) if tr else F.conv2d(x, w, b, s, p)


def train64(sd, images, relu_masks, idx, beta, data_variance):
    """One iteration in fp64 given the decisions.  sd: state dict (any float dtype); images [B,C,H,W]; relu_masks: four bool
    tensors [B,C,h,w] (a1, a2, d1, d2: True where the ReLU passes its input); idx int64 [B*h*w] -> ({"loss_eq", "loss_rec",
    "real_loss_rec"} floats, {parameter name: fp64 gradient} of (loss_eq + loss_rec), thirteen tensors)."""
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    m = [t.cpu().bool() for t in relu_masks]
    x = images.detach().cpu().double()

    def layer(i, h, mask=None):
        y = _conv(h, p[PARAMS[i] + ".weight"], p[PARAMS[i] + ".bias"], LAYERS[i])
        return y if mask is None else torch.where(mask, y, torch.zeros((), dtype=torch.float64))

    z = layer(2, layer(1, layer(0, x, m[0]), m[1]))
    zl = z.permute(0, 2, 3, 1)
    q = p["vq_layer.embeddings.weight"][idx.cpu().reshape(-1)].view_as(zl)
    loss_eq = F.mse_loss(q, zl.detach()) + beta * F.mse_loss(zl, q.detach())
    e = (zl + (q - zl).detach()).permute(0, 3, 1, 2)
    xr = layer(5, layer(4, layer(3, e, m[2]), m[3]))
    real = F.mse_loss(xr, x)
    loss_rec = real / float(data_variance)
    (loss_eq + loss_rec).backward()
    return ({"loss_eq": float(loss_eq.detach()), "loss_rec": float(loss_rec.detach()), "real_loss_rec": float(real.detach())},
            {k: v.grad for k, v in p.items()})


def check_decisions(sd, rec, what=""):
    """The teacher-forced layer check.  rec: {"x", "a1", "a2", "z", "idx", "e", "d1", "d2", "x_recon"} (logical NCHW, fp32; any
    device).  Asserts the bounds and returns {"mask_diff": units whose mask differs from preact64 > 0 (all within the bound),
    "idx_diff": rows whose index differs from the fp64 arg min (all within tau), "worst_act": largest |saved - fp64| / bound,
    "worst_slack": largest index slack / tau}."""
    r = {k: v.detach().cpu() for k, v in rec.items() if isinstance(v, torch.Tensor)}
    chain = (("x", "a1"), ("a1", "a2"), ("a2", "z"), ("e", "d1"), ("d1", "d2"), ("d2", "x_recon"))
    mask_diff, worst = 0, 0.0
    for i, (src, dst) in enumerate(chain):
        w, b = sd[PARAMS[i] + ".weight"].double(), sd[PARAMS[i] + ".bias"].double()
        h = r[src].double()
        pre = _conv(h, w, b, LAYERS[i])
        n = w.shape[2] * w.shape[3] * (w.shape[0] if LAYERS[i][0] else w.shape[1])      # taps x input channels (at most)
        bound = (n + 2) * EPS * _conv(h.abs(), w.abs(), b.abs(), LAYERS[i])
        got = r[dst].double()
        want = pre.clamp_min(0) if LAYERS[i][4] else pre
        ok = torch.isfinite(want)
        ratio = float(((got - want).abs()[ok] / bound[ok].clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{what}: {dst} is {ratio:.3g} x the forward bound from its fp64 value"
        if LAYERS[i][4]:
            differ = (r[dst] > 0) != (pre > 0)
            assert bool((pre.abs()[differ] <= bound[differ]).all()), f"{what}: a ReLU decision of {dst} differs outside the bound"
            mask_diff += int(differ.sum())
    d64 = orc.distances64(r["z"], sd)
    idx_diff, slack = orc.check_indices(d64, r["idx"], what)
    zl = r["z"].permute(0, 2, 3, 1)
    q = sd["vq_layer.embeddings.weight"][r["idx"].reshape(-1)].view_as(zl)
    assert torch.equal(r["e"].permute(0, 2, 3, 1), zl + (q - zl)), f"{what}: e is not the fp32 value z + (q - z)"
    return {"mask_diff": mask_diff, "idx_diff": idx_diff, "worst_act": worst, "worst_slack": slack}


def masks_of(rec):
    return [rec[k].detach().cpu() > 0 for k in MASKS]


def module_path_decisions(model, images):
    """(losses, masks, idx) of one forward of ``model``'s MODULE path (train() mode, hooks on the four nn.ReLU modules -- which
    also keep the HIP path away); the caller runs backward on the losses."""
    got, handles = {}, []
    relus = (model.encoder.convs[1], model.encoder.convs[3], model.decoder.convs[1], model.decoder.convs[3])
    for name, mod in zip(MASKS, relus):
        handles.append(mod.register_forward_hook(lambda _m, _i, out, name=name: got.__setitem__(name, out.detach().cpu() > 0)))
    handles.append(model.encoder.register_forward_hook(lambda _m, _i, out: got.__setitem__("z", out.detach())))
    try:
        losses = model(images)
    finally:
        for h in handles:
            h.remove()
    flat = got["z"].permute(0, 2, 3, 1).reshape(-1, model.embedding_dim)
    idx = model.vq_layer.get_code_indices(flat).cpu()
    return losses, [got[k] for k in MASKS], idx


# ---- counted bounds of the quantiser and loss kernels against fp64 given the indices (tests/test_gpu_ann_vqvae_train.py) ----
# Every bound is (number of fp32 roundings on the path, rounded up to 8) x 2^-24 x the magnitude the roundings act on.
def vq_reference(z, cb, idx, beta, g_e, g_loss):
    """fp64 values and bounds of spk_ann_vqvae_train_vq_fwd / _bwd for z [N,D], cb [K,D] fp32, idx [N], g_e [N,D], g_loss float."""
    z64, cb64, g64 = z.double().cpu(), cb.double().cpu(), g_e.double().cpu()
    idx = idx.cpu()
    q = cb64[idx]
    n = z64.numel()
    m = float(((q - z64) ** 2).mean())
    loss = m + beta * m                                   # roundings: q - z, its square, the mean, beta * m, the sum
    t = g_loss * beta * 2.0 * (z64 - q) / n               # roundings: gl * beta, 2 / n, their product, z - q, the product, the sum
    gz = g64 + t
    gcb = torch.zeros_like(cb64)
    gcb.index_add_(0, idx, q - z64)
    mag = torch.zeros_like(cb64)
    mag.index_add_(0, idx, (q - z64).abs())
    scale = abs(g_loss) * 2.0 / n                         # roundings: every q - z, the sum's cast, 2 / n, two products
    return {"loss": loss, "loss_bound": 8 * EPS * abs(loss), "gz": gz, "gz_bound": 8 * EPS * (g64.abs() + t.abs()),
            "gcb": g_loss * 2.0 / n * gcb, "gcb_bound": 8 * EPS * scale * mag}


def loss_reference(xr_nchw, x, dv, g_recon, g_real):
    """fp64 values and bounds of spk_ann_vqvae_train_loss_fwd / _bwd (xr_nchw: the reconstruction, logical NCHW)."""
    d = xr_nchw.double().cpu() - x.double().cpu()
    mse = float((d ** 2).mean())                          # roundings: the difference, its square, the mean, the division
    g = (g_recon / dv + g_real) * 2.0 * d / d.numel()     # roundings: g / dv, the sum, 2 / n, the product, the difference, the product
    return {"real": mse, "recon": mse / dv, "bound": 8 * EPS * mse, "recon_bound": 8 * EPS * mse / dv, "g": g,
            "g_bound": 8 * EPS * g.abs()}


# ---- the epilogue cases ---------------------------------------------------------------------------------------------------
def vqvae_layers(C, H):
    """The launches of one training iteration that carry an epilogue, as (name, layer tuple of _conv_train_cases, op, epilogue):
    layer = (Cin, Cout, k, stride, pad, transposed, out_pad, input size)."""
    return (
        ("enc0.fwd", (C, 32, 3, 2, 1, False, 0, H), "fwd", "relu"),
        ("enc2.fwd", (32, 64, 3, 2, 1, False, 0, H // 2), "fwd", "relu"),
        ("enc2.dgrad", (32, 64, 3, 2, 1, False, 0, H // 2), "dgrad", "masked"),
        ("enc4.dgrad", (64, D, 1, 1, 0, False, 0, H // 4), "dgrad", "masked"),
        ("dec0.fwd", (D, 64, 3, 2, 1, True, 1, H // 4), "fwd", "relu"),
        ("dec2.fwd", (64, 32, 3, 2, 1, True, 1, H // 2), "fwd", "relu"),
        ("dec2.dgrad", (64, 32, 3, 2, 1, True, 1, H // 2), "dgrad", "masked"),
        ("dec4.dgrad", (32, C, 3, 1, 1, True, 0, H), "dgrad", "masked"),
    )


def big_threshold(layer, op):
    """Smallest N at which the gather launch of (layer, op) has CT_BIG_ITEMS items or more (two column tiles per wave)."""
    n = 1
    while ctc.gather_launch(*ctc.gather_args(layer, n, op))["items"] < ctc.CT_BIG_ITEMS:
        n += 1
    return n


# 64-output-channel launches on either side of CT_BIG_ITEMS: a ReLU launch of each gather form and a masked one
BIG_LAYERS = tuple((name, layer, op, epi) for name, layer, op, epi in vqvae_layers(1, 28)
                   if name in ("enc2.fwd", "dec0.fwd", "dec2.dgrad"))


def second_trip(L):
    """Whether a launch of ctc.gather_launch walks its loop a second time: a workgroup of the few-channel kernels takes a second
    row (rows > CT_C1_ROWS_CAP), a wave of the main gather kernel a second item (passes >= 2)."""
    return L["rows"] > L["grid"] if L["kernel"] in ("c1in", "c1out") else L["passes"] >= 2


def second_trip_threshold(layer, op):
    """Smallest N at which the gather launch of (layer, op) takes a second trip."""
    n = 1
    while not second_trip(ctc.gather_launch(*ctc.gather_args(layer, n, op))):
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def second_trip_cases():
    """[(id, layer, N, op, epilogue)]: the smallest N with a second trip of each of the eight epilogue launches at H = 28 (grey)
    and of the RGB few-channel pair at H = 32."""
    out = []
    for name, layer, op, epi in vqvae_layers(1, 28):
        n = second_trip_threshold(layer, op)
        out.append((f"{name}-H28-second_trip-N{n}", layer, n, op, epi))
    for name, layer, op, epi in vqvae_layers(3, 32):
        if name in ("enc0.fwd", "dec4.dgrad"):
            n = second_trip_threshold(layer, op)
            out.append((f"{name}-H32-second_trip-N{n}", layer, n, op, epi))
    return tuple(out)


def epilogue_cases():
    """[(id, layer, N, op, epilogue)]: every layer at H = 28 (grey) and 32 (RGB), N = 1 and 3, the CT_BIG_ITEMS pairs, and the
    second-trip cases."""
    out = []
    for C, H in ((1, 28), (3, 32)):
        for name, layer, op, epi in vqvae_layers(C, H):
            for N in (1, 3):
                out.append((f"{name}-H{H}-N{N}", layer, N, op, epi))
    for name, layer, op, epi in BIG_LAYERS:
        n = big_threshold(layer, op)
        out += [(f"{name}-below_big-N{n - 1}", layer, n - 1, op, epi), (f"{name}-at_big-N{n}", layer, n, op, epi)]
    return out + list(second_trip_cases())


# ---- the launch arithmetic of the quantiser and loss entry points (csrc/ann_vqvae_train.hip), mirrored on the host ---------------
# The caps are read from the source and the chunk from the header, so a retuned cap moves the cases below with it; every case
# carries the side of the cap it claims, and tests/test_ann_vqvae_train_host.py checks the claim on a machine without a GPU.
def _cap(name):
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)\s*[,;]", open(SRC).read())
    assert m, f"{name} not found in {SRC}"
    return int(m.group(1))


AT_VQ_GRID, AT_EW_GRID, AT_LOSS_GRID = _cap("AT_VQ_GRID"), _cap("AT_EW_GRID"), _cap("AT_LOSS_GRID")
CHUNK = _lib.CONSTANTS["SPK_ANN_VQVAE_TRAIN_CHUNK"]
MAX_D = _lib.CONSTANTS["SPK_VQ_TRAIN_MAX_D"]
VQ_WAVES = 4                      # rows a workgroup of ann_vq_fwd_kernel takes per trip (a wave each)
SCAN = 256                        # rows the per-code workgroups of ann_vq_bwd_kernel scan at a time
SMALL_N = 33 * 64                 # the largest row count of the one-trip cases: the prefix the row-independence checks repeat


def _cdiv(a, b):
    return -(-a // b)


def _ew_grid(elems):
    """spk_grid(elems, AT_EW_GRID): one thread per element, 256 to a workgroup, capped."""
    return max(1, min(_cdiv(elems, 256), AT_EW_GRID))


def ws_doubles(rows, elems):
    """spk_ann_vqvae_train_ws_bytes / 8: a partial per row or per chunk, whichever is more (at least one)."""
    return max(rows, _cdiv(elems, CHUNK), 1)


def vq_fwd_launch(N, D, K):
    grid = min(_cdiv(N, VQ_WAVES), AT_VQ_GRID)
    return dict(kernel="vq_fwd<16>" if D == 16 else "vq_fwd<0>", grid=grid, second_trip=N > grid * VQ_WAVES, partials=N, nb_x=0,
                last_trip_rows=N % (grid * VQ_WAVES), ws_doubles=ws_doubles(N, 0))


def vq_bwd_launch(N, D, K):
    nb_x = _ew_grid(N * D)
    return dict(kernel="vq_bwd", grid=nb_x + K, second_trip=N * D > nb_x * 256, partials=0, nb_x=nb_x,
                last_trip_elems=(N * D) % (nb_x * 256), scans=_cdiv(N, SCAN), last_scan_rows=N % SCAN, RL=256 // D)


def loss_fwd_launch(B, C, H):
    n = B * C * H * H
    chunks = _cdiv(n, CHUNK)
    grid = min(chunks, AT_LOSS_GRID)
    return dict(kernel="loss_fwd", n=n, grid=grid, second_trip=chunks > grid, partials=chunks, nb_x=0, last_chunk_elems=n % CHUNK,
                last_trip_chunks=chunks % grid, ws_doubles=ws_doubles(0, n))


def loss_bwd_launch(B, C, H):
    n = B * C * H * H
    nb_x = _ew_grid(n)
    return dict(kernel="loss_bwd", n=n, grid=nb_x, second_trip=n > nb_x * 256, partials=0, nb_x=nb_x,
                last_trip_elems=n % (nb_x * 256), last_block_elems=n % 256)


def _first(pred, start=1):
    n = start
    while not pred(n):
        n += 1
    return n


# The quantiser cases: (kind, N, D, K, claim, why).  Each past-the-cap size is the smallest with a second trip plus a ragged
# remainder (the forward's second trip is 37 rows: nine whole workgroups and one wave of a tenth, and a partial 256-row scan of
# the backward; the backward's is 19 rows: one partial workgroup at D = 16, five at D = 64).
FWD_RAGGED, BWD_RAGGED = 36, 18
N_PAST_FWD = {D: _first(lambda n, D=D: vq_fwd_launch(n, D, 1)["second_trip"]) + FWD_RAGGED for D in (16, 24)}
N_PAST_BWD = {D: _first(lambda n, D=D: vq_bwd_launch(n, D, 1)["second_trip"], (AT_EW_GRID * 256) // D - 2) + BWD_RAGGED
              for D in (16, 64)}


def _past_fwd(N, D, K):
    f, b = vq_fwd_launch(N, D, K), vq_bwd_launch(N, D, K)
    return (f["second_trip"] and f["grid"] == AT_VQ_GRID and 0 < f["last_trip_rows"] < f["grid"] * VQ_WAVES
            and f["last_trip_rows"] % VQ_WAVES != 0 and b["last_scan_rows"] != 0 and N > SMALL_N)


def _past_bwd(N, D, K):
    b = vq_bwd_launch(N, D, K)
    return (b["second_trip"] and b["nb_x"] == AT_EW_GRID and 0 < b["last_trip_elems"] < b["nb_x"] * 256
            and b["last_trip_elems"] % 256 != 0 and b["last_scan_rows"] != 0 and b["scans"] >= 2 and N > SMALL_N)


def _one_trip(N, D, K):
    f, b = vq_fwd_launch(N, D, K), vq_bwd_launch(N, D, K)
    return not f["second_trip"] and not b["second_trip"] and b["nb_x"] < AT_EW_GRID


def _dc0(claim):
    return lambda N, D, K: D != 16 and 1 <= D <= MAX_D and vq_fwd_launch(N, D, K)["kernel"] == "vq_fwd<0>" and claim(N, D, K)


DC0_D, DC0_K, DC0_N = (1, 3, 8, 24, 33, 64), (1, 63, 65, 244), (3 * 49, SMALL_N)
VQ_CASES = (
    [(kind, N, D, K, _one_trip, "one trip of every loop") for kind, N, K in
     (("random", 49, 100), ("random", 3 * 49, 128), ("random", SMALL_N, 256), ("one_code", 3 * 49, 128), ("few_codes", SMALL_N, 256))]
    + [(kind, N_PAST_FWD[16], 16, 128, _past_fwd, "ann_vq_fwd_kernel<16>: some waves walk a second row") for kind in ("random", "few_codes")]
    + [("random", N_PAST_BWD[16], 16, 100, _past_bwd, "ann_vq_bwd_kernel: the element-wise blocks walk a second element (and the forward "
        "a third row)"),
       ("random", N_PAST_BWD[64], 64, 64, _dc0(_past_bwd), "the same with a row per wave-width: D = 64"),
       ("random", N_PAST_FWD[24], 24, 65, _dc0(_past_fwd), "ann_vq_fwd_kernel<0> past the forward's cap")]
    + [("random", N, D, K, _dc0(_one_trip), "the DC == 0 form") for D in DC0_D for K in DC0_K for N in DC0_N]
)


def vq_case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" if c[2] != D else f"{c[0]}-{c[1]}-{c[3]}"


# The loss cases: (B, C, H, claim).  Forward: the smallest B with more chunks than AT_LOSS_GRID and a partial last chunk.
# Backward: the smallest B with more than 256 AT_EW_GRID elements and a second trip that covers part of the grid (a CIFAR image
# is twelve whole workgroups, so there the ragged end is a partial trip; at 28 x 28 the last workgroup is partial as well).
def _loss_one_trip(B, C, H):
    return not loss_fwd_launch(B, C, H)["second_trip"] and not loss_bwd_launch(B, C, H)["second_trip"]


def _loss_past_fwd(B, C, H):
    f = loss_fwd_launch(B, C, H)
    return (f["second_trip"] and f["grid"] == AT_LOSS_GRID and f["last_chunk_elems"] != 0 and f["last_trip_chunks"] != 0
            and loss_bwd_launch(B, C, H)["second_trip"])


def _loss_past_bwd(B, C, H):
    b = loss_bwd_launch(B, C, H)
    return (b["second_trip"] and b["grid"] == AT_EW_GRID and 0 < b["last_trip_elems"] < b["grid"] * 256
            and (b["last_block_elems"] != 0 or (C * H * H) % 256 == 0) and not loss_bwd_launch(B - 1, C, H)["second_trip"])


LOSS_CASES = (
    [(B, C, H, _loss_one_trip) for B, C, H in ((1, 1, 28), (3, 3, 32), (33, 1, 28), (5, 3, 28))]
    + [(_first(lambda b: loss_bwd_launch(b, C, H)["second_trip"]), C, H, _loss_past_bwd) for C, H in ((1, 28), (3, 32))]
    + [(_first(lambda b: loss_fwd_launch(b, C, H)["second_trip"] and loss_fwd_launch(b, C, H)["last_chunk_elems"] != 0), C, H,
        _loss_past_fwd) for C, H in ((3, 32), (1, 28))]
)


# ---- the model cases: (id, shape name of _ann_vqvae_oracle.SHAPES, B); "f20" = the fixture's images and state -------------------
MODEL_CASES = (("f20", "mnist_k128", 8), ("mnist_k128-B1", "mnist_k128", 1), ("mnist_k128-B3", "mnist_k128", 3),
               ("mnist_k128-B33", "mnist_k128", 33), ("cifar_k256-B3", "cifar_k256", 3), ("mnist_k100-B3", "mnist_k100", 3),
               # past the quantiser's forward cap (8232 and 8320 rows) and the read-out kernels' row cap (4704 and 4160 rows)
               ("mnist_k128-B168", "mnist_k128", 168), ("cifar_k256-B130", "cifar_k256", 130))


def model_inputs(case):
    """(state dict, images fp32 [B,C,H,W], data_variance float, K, in_dim) of a model case."""
    cid, shape, B = case
    _, cfg, K = next(s for s in orc.SHAPES if s[0] == shape)
    sd = orc.state(shape)
    if cid == "f20":
        f = orc.fixture()
        return sd, torch.from_numpy(f["images"]), float(f["data_variance"]), K, cfg.in_dim
    images = synth.stroke_images(B, img=cfg.img, channels=cfg.in_dim) - 0.5
    return sd, images, 0.0625, K, cfg.in_dim


def grad_entries(g):
    g = g.detach().cpu().numpy().reshape(-1)
    return g[orc.sub_index(g.size)] if g.size > orc.SUB else g
