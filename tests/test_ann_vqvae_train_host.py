"""CPU tests of the plain-CNN VQVAE baseline's training step on HIP (no GPU): the fp64 oracle of the GPU tests
meets fixture F20 when it is given the module path's decisions, the new entry points are declared, bound and exported and
refuse bad arguments before they touch a device, the epilogue case table lands on the launch forms it claims, every
past-the-cap case of the quantiser, loss and epilogue tables really is past its cap with a ragged remainder (the launch
arithmetic restated on the host, the caps read from the sources), the workspace size is the launch model's, and on the CPU
VQVAE.train() still takes the module path."""
import numpy as np
import pytest
import torch

import _ann_vqvae_oracle as orc
import _ann_vqvae_train_oracle as tor
import _conv_train_cases as ctc

NEW_ENTRY_POINTS = ("spk_conv_train_gather_relu", "spk_conv_train_gather_masked", "spk_ann_vqvae_train_supported",
                    "spk_ann_vqvae_train_ws_bytes",
                    "spk_ann_vqvae_train_vq_fwd", "spk_ann_vqvae_train_vq_bwd", "spk_ann_vqvae_train_loss_fwd",
                    "spk_ann_vqvae_train_loss_bwd")


def _model(train=True):
    from snn_model.vae_model import VQVAE
    f = orc.fixture()
    m = VQVAE(1, 16, 128, torch.tensor(float(f["data_variance"])))
    m.load_state_dict(orc.state("mnist_k128"))
    return m.train() if train else m.eval()


def test_train64_given_the_module_paths_decisions_meets_f20():
    """The oracle against the real reference's fp64 run: train64 is handed the decisions of the CPU module path (forward hooks on
    the four nn.ReLU modules, and the indices) and must meet F20's loss64/* and grad64/* within 8 x the fp32 reference's own
    error, the rule of test_module_path_training_iteration_meets_f20."""
    f = orc.fixture()
    m = _model()
    images = torch.from_numpy(f["images"])
    _, masks, idx = tor.module_path_decisions(m, images)
    assert torch.equal(idx, torch.from_numpy(f["indices64"]))
    losses, grads = tor.train64(orc.state("mnist_k128"), images, masks, idx, 0.25, float(f["data_variance"]))
    for name, v in losses.items():
        err, bound = abs(v - float(f["loss64/" + name])), 8 * float(f["err_loss/" + name])
        print(f"{name}: {v:.12g} vs F20 {float(f['loss64/' + name]):.12g}: err {err:.3g}, bound {bound:.3g}")
        assert err <= bound, name
    assert set(grads) == {n for n, _ in m.named_parameters()}
    for n, g in grads.items():
        big = g.numel() > orc.SUB
        want = f["grad64/" + n + "/sub"] if big else f["grad64/" + n].reshape(-1)
        err, bound = float(np.abs(tor.grad_entries(g) - want).max()), 8 * float(f["err_grad/" + n])
        print(f"grad {n}: err {err:.3g}, bound {bound:.3g}")
        assert err <= bound, n
        if big:
            assert abs(float(g.norm()) - float(f["grad64/" + n + "/norm"])) <= 8 * float(f["err_gradnorm/" + n]), n


def test_teacher_forced_check_accepts_the_module_path_and_refuses_a_wrong_decision():
    f = orc.fixture()
    sd = orc.state("mnist_k128")
    m = _model()
    images = torch.from_numpy(f["images"])
    saved = {}
    convs = {"a1": m.encoder.convs[1], "a2": m.encoder.convs[3], "z": m.encoder.convs[4], "d1": m.decoder.convs[1],
             "d2": m.decoder.convs[3], "x_recon": m.decoder.convs[4]}
    hs = [mod.register_forward_hook(lambda _m, _i, out, k=k: saved.__setitem__(k, out.detach().clone())) for k, mod in convs.items()]
    hs.append(m.vq_layer.register_forward_hook(lambda _m, _i, out: saved.__setitem__("e", out[0].detach().clone())))
    m(images)
    for h in hs:
        h.remove()
    flat = saved["z"].permute(0, 2, 3, 1).reshape(-1, 16)
    rec = dict(saved, x=images, idx=m.vq_layer.get_code_indices(flat))
    rep = tor.check_decisions(sd, rec, "module path")
    print("PARITY_REPORT ann_vqvae_train cpu_module_path " + " ".join(f"{k}={v:.3g}" for k, v in rep.items()))
    assert rep["worst_act"] <= 1.0 and rep["worst_slack"] <= 1.0
    bad = dict(rec, a2=rec["a2"].clone())
    big = int(bad["a2"].reshape(-1).argmax())
    bad["a2"].reshape(-1)[big] = 0.0                                # a unit far above zero, recorded as cut
    with pytest.raises(AssertionError):
        tor.check_decisions(sd, bad, "tampered")
    bad = dict(rec, idx=(rec["idx"] + 1) % 128)
    with pytest.raises(AssertionError):
        tor.check_decisions(sd, bad, "tampered")


def test_header_declares_binds_and_exports_the_entry_points():
    from spkdiff import _lib, ops
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.EXPORTS, name
        assert getattr(_lib.lib, name).argtypes is not None
    assert _lib.version() == _lib.EXPECTED_VERSION == 106
    relu, masked, plain = (getattr(_lib.lib, n).argtypes for n in NEW_ENTRY_POINTS[:2] + ("spk_conv_train_gather",))
    assert list(relu) == list(plain) and len(masked) == len(plain) + 1
    assert _lib.CONSTANTS["SPK_ANN_VQVAE_TRAIN_CHUNK"] == 2048
    for name in ("ann_vqvae_train_forward", "ann_vqvae_train_backward", "ann_vqvae_train_supported", "ANNVQVAETrainFunction"):
        assert hasattr(ops, name), name
    from spkdiff import train
    assert hasattr(train, "GraphedANNVQVAETrainStep")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ann_vqvae_train_forward(torch.zeros(1, 1, 28, 28), [torch.zeros(1)] * 6, [torch.zeros(1)] * 6, torch.zeros(128, 16),
                                    0.25, 1.0)


def test_argument_errors_come_back_without_a_device():
    from spkdiff import _lib
    L, C = _lib.lib, _lib.CONSTANTS
    ARG, UNS = C["SPK_ERR_ARG"], C["SPK_ERR_UNSUPPORTED"]
    p = 4096                                                        # a non-null, 8-byte aligned address nothing dereferences
    geo = (1, 14, 14, 32, 7, 7, 64, 3, 2, 1, 0, 9, 1, 288)          # enc.conv2 forward
    assert L.spk_conv_train_gather_relu(None, p, None, p, *geo, None) == ARG
    assert L.spk_conv_train_gather_relu(p, None, None, p, *geo, None) == ARG
    assert L.spk_conv_train_gather_relu(p, p, None, None, *geo, None) == ARG
    assert L.spk_conv_train_gather_masked(p, p, None, None, p, *geo, None) == ARG          # the mask is not optional
    assert L.spk_conv_train_gather_masked(p, p, None, p, None, *geo, None) == ARG
    for i in (0, 1, 2, 4, 5):                                       # N, Hi, Wi, Ho, Wo
        bad = list(geo)
        bad[i] = 0
        assert L.spk_conv_train_gather_relu(p, p, None, p, *bad, None) == ARG, i
        assert L.spk_conv_train_gather_masked(p, p, None, p, p, *bad, None) == ARG, i
    # the shapes spk_conv_train_gather_supported refuses, and the few-output-channel kernel, which has no epilogue
    for Cred, Cout, k, stride, form in ((32, 64, 5, 1, 0), (12, 64, 3, 2, 0), (32, 96, 3, 2, 0), (3, 30, 3, 2, 0), (32, 64, 3, 3, 1)):
        assert not L.spk_conv_train_gather_supported(Cred, Cout, k, stride, form)
        g = (1, 14, 14, Cred, 7, 7, Cout, k, stride, 1, form, 1, 1, 1)
        assert L.spk_conv_train_gather_relu(p, p, None, p, *g, None) == UNS
        assert L.spk_conv_train_gather_masked(p, p, None, p, p, *g, None) == UNS
    assert L.spk_conv_train_gather_supported(32, 1, 3, 1, 1)
    g = (1, 28, 28, 32, 28, 28, 1, 3, 1, 1, 1, 1, 1, 1)
    assert L.spk_conv_train_gather_relu(p, p, None, p, *g, None) == UNS
    assert L.spk_conv_train_gather_masked(p, p, None, p, p, *g, None) == UNS

    assert L.spk_ann_vqvae_train_ws_bytes(49, 784) == 49 * 8 and L.spk_ann_vqvae_train_ws_bytes(1, 4097) == 3 * 8
    assert L.spk_ann_vqvae_train_ws_bytes(-1, 0) == ARG
    ws = 49 * 8
    ok = dict(z=p, cb=p, idx=p, e=p, loss=p, ws=p)
    for missing in ok:
        a = dict(ok, **{missing: None})
        assert L.spk_ann_vqvae_train_vq_fwd(a["z"], a["cb"], a["idx"], a["e"], a["loss"], 0.25, a["ws"], ws, 49, 16, 128, None) == ARG
    assert L.spk_ann_vqvae_train_vq_fwd(p, p, p, p, p, 0.25, p, ws - 8, 49, 16, 128, None) == ARG        # workspace too small
    assert L.spk_ann_vqvae_train_vq_fwd(p, p, p, p, p, 0.25, p + 4, ws, 49, 16, 128, None) == ARG        # ... or misaligned
    for N, D, K in ((0, 16, 128), (49, 0, 128), (49, 16, 0), (-3, 16, 128)):
        assert L.spk_ann_vqvae_train_vq_fwd(p, p, p, p, p, 0.25, p, ws, N, D, K, None) == ARG
        assert L.spk_ann_vqvae_train_vq_bwd(p, p, p, p, p, 0.25, p, p, N, D, K, None) == ARG
    assert L.spk_ann_vqvae_train_vq_fwd(p, p, p, p, p, 0.25, p, ws, 49, C["SPK_VQ_TRAIN_MAX_D"] + 1, 128, None) == UNS
    assert L.spk_ann_vqvae_train_vq_bwd(p, p, p, p, p, 0.25, p, p, 49, C["SPK_VQ_TRAIN_MAX_D"] + 1, 128, None) == UNS
    assert L.spk_ann_vqvae_train_vq_fwd(p, p, p, p, p, 0.25, p, ws, 49, 64, 512, None) == UNS            # codebook beyond 64 KB of LDS
    for i in range(2, 7):                                           # z, idx, codebook, gz, gcodebook (g_e and g_loss may be NULL)
        a = [p] * 5 + [0.25, p, p]
        a[i if i < 5 else i + 1] = None
        assert L.spk_ann_vqvae_train_vq_bwd(*a, 49, 16, 128, None) == ARG, i
    lw = 8
    for i in range(6):                                              # x_recon, x, data_variance, recon, real, ws
        a = [p] * 6
        a[i] = None
        assert L.spk_ann_vqvae_train_loss_fwd(*a, lw, 1, 1, 28, 28, None) == ARG, i
    assert L.spk_ann_vqvae_train_loss_fwd(p, p, p, p, p, p, 0, 8, 1, 28, 28, None) == ARG
    for dims in ((0, 1, 28, 28), (1, 0, 28, 28), (1, 1, 0, 28), (1, 1, 28, 0)):
        assert L.spk_ann_vqvae_train_loss_fwd(p, p, p, p, p, p, 1 << 20, *dims, None) == ARG
        assert L.spk_ann_vqvae_train_loss_bwd(p, p, p, p, p, p, *dims, None) == ARG
    for i in (0, 1, 4, 5):                                          # x_recon, x, data_variance, gx (the two loss gradients may be NULL)
        a = [p] * 6
        a[i] = None
        assert L.spk_ann_vqvae_train_loss_bwd(*a, 1, 1, 28, 28, None) == ARG, i


def test_epilogue_cases_land_on_the_launch_forms_they_claim():
    cases = tor.epilogue_cases()
    ids = [c[0] for c in cases]
    assert len(set(ids)) == len(ids)
    kernels = {}
    for cid, layer, N, op, epi in cases:
        a = ctc.gather_args(layer, N, op)
        assert ctc.gather_kind(a[3], a[6], a[7], a[8], a[10]), cid
        kernels.setdefault(ctc.gather_launch(*a)["kernel"], set()).add(epi)
    assert kernels == {"gather": {"relu", "masked"}, "c1in": {"relu", "masked"}}        # both epilogues in both kernels
    # which N puts the 64-output-channel launches on either side of CT_BIG_ITEMS
    for name, layer, op, _ in tor.BIG_LAYERS:
        n = tor.big_threshold(layer, op)
        below, at = (ctc.gather_launch(*ctc.gather_args(layer, m, op)) for m in (n - 1, n))
        print(f"{name}: N = {n - 1}: {below['items']} items, CN {below['CN']}, gy {below['gy']};  N = {n}: {at['items']} items, "
              f"CN {at['CN']}, gy {at['gy']}")
        assert below["items"] < ctc.CT_BIG_ITEMS <= at["items"]
        assert (below["CNT"], below["CN"], below["gy"]) == (2, 1, 2) and (at["CNT"], at["CN"], at["gy"]) == (2, 2, 1)
        assert f"{name}-below_big-N{n - 1}" in ids and f"{name}-at_big-N{n}" in ids
    # ConvT D->64 forward changes form where the existing boundary cases of conv_train.hip say it does; Conv 32->64 forward where
    # 49 N / 32 output rows reach CT_BIG_ITEMS items
    assert tor.big_threshold(ctc.DEC_CONVT1, "fwd") == next(c["N"] for c in ctc.BOUNDARY_CASES if c["id"] == "form1_items_at_big")
    assert tor.big_threshold((32, 64, 3, 2, 1, False, 0, 14), "fwd") == (ctc.CT_BIG_ITEMS - 1) * 32 // 49 + 1
    # every reference-batch launch (B = 32, both shapes) is a small one: one column tile per workgroup
    for C, H in ((1, 28), (3, 32)):
        for name, layer, op, _ in tor.vqvae_layers(C, H):
            L = ctc.gather_launch(*ctc.gather_args(layer, 32, op))
            assert L["kernel"] == "c1in" or L["CN"] == 1 or L["CNT"] == 1, name


def test_second_trip_epilogue_cases_take_a_second_trip():
    """The smallest N at which each epilogue launch walks its loop again: a second row per workgroup in the few-channel kernels
    (rows > CT_C1_ROWS_CAP), a second item per wave in the main gather kernel (passes >= 2) -- and one image fewer does not."""
    cases = tor.second_trip_cases()
    ids = [c[0] for c in tor.epilogue_cases()]
    names = [n for n, *_ in tor.vqvae_layers(1, 28)]
    assert [c[0].split("-")[0] for c in cases] == names + ["enc0.fwd", "dec4.dgrad"] and len(names) == 8
    seen = set()
    for cid, layer, N, op, epi in cases:
        assert cid in ids, cid
        at, below = (ctc.gather_launch(*ctc.gather_args(layer, n, op)) for n in (N, N - 1))
        print(f"{cid}: {at}")
        assert tor.second_trip(at) and not tor.second_trip(below), cid
        if at["kernel"] == "c1in":
            assert ctc.CT_C1_ROWS_CAP < at["rows"] < 2 * ctc.CT_C1_ROWS_CAP and at["grid"] == ctc.CT_C1_ROWS_CAP, cid
        else:
            assert at["kernel"] == "gather" and at["passes"] == 2 and at["gx"] * 8 < at["items"] < at["gx"] * 16, cid
        seen.add((at["kernel"], epi))
    assert seen == {("gather", "relu"), ("gather", "masked"), ("c1in", "relu"), ("c1in", "masked")}
    dec4 = next(c for c in cases if c[0].startswith("dec4.dgrad-H28"))
    assert dec4[2] == ctc.CT_C1_ROWS_CAP // 28 + 1                  # (147 at a cap of 4096 rows)


def test_quantiser_and_loss_cases_sit_past_the_caps_they_claim():
    """The launch arithmetic of csrc/ann_vqvae_train.hip on the host (the caps read from the source): every case lands on the side
    of its cap it claims -- past it with a ragged remainder, or within one trip -- so a retuned cap cannot leave the GPU tests
    below it unnoticed."""
    assert (tor.AT_VQ_GRID, tor.AT_EW_GRID, tor.AT_LOSS_GRID) == (2048, 1024, 1024) and tor.CHUNK == 2048     # today's values
    ids = [tor.vq_case_id(c) for c in tor.VQ_CASES]
    assert len(set(ids)) == len(ids)
    for kind, N, D, K, claim, why in tor.VQ_CASES:
        f, b = tor.vq_fwd_launch(N, D, K), tor.vq_bwd_launch(N, D, K)
        assert claim(N, D, K), (kind, N, D, K, why, f, b)
        assert f["partials"] == N and f["grid"] <= tor.AT_VQ_GRID and b["grid"] == b["nb_x"] + K and b["nb_x"] <= tor.AT_EW_GRID
    by = {(N, D, K): (tor.vq_fwd_launch(N, D, K), tor.vq_bwd_launch(N, D, K)) for _, N, D, K, *_ in tor.VQ_CASES}
    # the sizes the cases were derived to be
    f, b = by[(4 * tor.AT_VQ_GRID + 37, 16, 128)]
    assert f["second_trip"] and f["last_trip_rows"] == 37 and not b["second_trip"] and b["last_scan_rows"] != 0
    f, b = by[(256 * tor.AT_EW_GRID // 16 + 19, 16, 100)]
    assert b["second_trip"] and b["last_trip_elems"] == 19 * 16 and b["last_scan_rows"] == 19 and f["second_trip"]
    f, b = by[(256 * tor.AT_EW_GRID // 64 + 19, 64, 64)]
    assert b["second_trip"] and b["last_trip_elems"] == 19 * 64 and b["last_scan_rows"] == 19 and b["RL"] == 4 and not f["second_trip"]
    f, b = by[(4 * tor.AT_VQ_GRID + 37, 24, 65)]
    assert f["kernel"] == "vq_fwd<0>" and f["second_trip"] and b["RL"] == 10 and 256 % 24
    # at the cap itself nothing walks twice: the cases are the first sizes that do, plus their remainders
    assert not tor.vq_fwd_launch(4 * tor.AT_VQ_GRID, 16, 128)["second_trip"]
    assert not tor.vq_bwd_launch(256 * tor.AT_EW_GRID // 16, 16, 100)["second_trip"]
    # every width and codebook size of the DC == 0 form, at both row counts, and the LDS ceiling of D = 64
    from spkdiff import _lib
    L = _lib.lib
    for D in tor.DC0_D:
        for K in tor.DC0_K:
            for N in tor.DC0_N:
                assert (N, D, K) in by and L.spk_ann_vqvae_train_supported(D, K), (N, D, K)
    assert tor.DC0_D == (1, 3, 8, 24, 33, 64) and tor.DC0_K == (1, 63, 65, 244) and tor.DC0_N == (147, 2112)
    assert not L.spk_ann_vqvae_train_supported(64, 245)
    for B, C, H, claim in tor.LOSS_CASES:
        assert claim(B, C, H), (B, C, H, tor.loss_fwd_launch(B, C, H), tor.loss_bwd_launch(B, C, H))
    shapes = [c[:3] for c in tor.LOSS_CASES]
    assert len(set(shapes)) == len(shapes)
    past_fwd = [c[:3] for c in tor.LOSS_CASES if c[3] is tor._loss_past_fwd]
    past_bwd = [c[:3] for c in tor.LOSS_CASES if c[3] is tor._loss_past_bwd]
    assert past_fwd == [(683, 3, 32), (2675, 1, 28)] and past_bwd == [(335, 1, 28), (86, 3, 32)]           # at today's caps
    for B, C, H in past_fwd:
        f = tor.loss_fwd_launch(B, C, H)
        assert f["partials"] == tor.AT_LOSS_GRID + 1 and 0 < f["last_chunk_elems"] < tor.CHUNK
    assert tor.loss_bwd_launch(335, 1, 28)["last_block_elems"] != 0


def test_ws_bytes_is_what_the_launch_model_says():
    """spk_ann_vqvae_train_ws_bytes is max(rows, chunks) doubles, exactly: the GPU tests hand the kernels that many and guard the
    bytes behind them."""
    from spkdiff import _lib
    L = _lib.lib
    for _, N, D, K, *_ in tor.VQ_CASES:
        assert L.spk_ann_vqvae_train_ws_bytes(N, 0) == 8 * tor.vq_fwd_launch(N, D, K)["ws_doubles"] == 8 * N
    for B, C, H, _ in tor.LOSS_CASES:
        f = tor.loss_fwd_launch(B, C, H)
        assert L.spk_ann_vqvae_train_ws_bytes(0, f["n"]) == 8 * f["ws_doubles"] == 8 * f["partials"]
    for rows, elems in ((0, 0), (1, 0), (0, 1), (0, tor.CHUNK), (0, tor.CHUNK + 1), (49, 784), (1, 4097), (8232, 168 * 784),
                        (8320, 130 * 3072), (3, 1 << 33), ((1 << 31) - 1, 5)):
        want = max(rows, -(-elems // tor.CHUNK), 1)
        assert tor.ws_doubles(rows, elems) == want and L.spk_ann_vqvae_train_ws_bytes(rows, elems) == 8 * want, (rows, elems)
    # the two model cases past the caps: the quantiser's rows outnumber the loss's chunks, and both loops walk twice
    for case, rows, readout_rows in (("mnist_k128-B168", 8232, 4704), ("cifar_k256-B130", 8320, 4160)):
        cid, shape, B = next(c for c in tor.MODEL_CASES if c[0] == case)
        _, cfg, K = next(s for s in orc.SHAPES if s[0] == shape)
        assert B * (cfg.img // 4) ** 2 == rows and B * cfg.img == readout_rows > ctc.CT_C1_ROWS_CAP
        assert tor.vq_fwd_launch(rows, tor.D, K)["second_trip"]
        for name, layer, op, _ in tor.vqvae_layers(cfg.in_dim, cfg.img):
            if name == "dec4.dgrad":
                assert tor.second_trip(ctc.gather_launch(*ctc.gather_args(layer, B, op)))


def test_vqvae_train_on_the_cpu_still_takes_the_module_path(monkeypatch):
    from spkdiff import ops
    calls = []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(ops._lib.lib, name)
            if name in NEW_ENTRY_POINTS:
                calls.append(name)
            return fn

    monkeypatch.setattr(ops, "lib", Recorder())
    m = _model()
    assert m.fused_train in (True, False)
    images = torch.from_numpy(orc.fixture()["images"])
    for flag in (True, False):
        m.fused_train = flag
        loss_eq, loss_rec, real = m(images)
        assert not calls
        assert type(real.grad_fn).__name__ == "MseLossBackward0" and loss_eq.grad_fn is not None and loss_rec.grad_fn is not None
    with torch.no_grad():
        vals = m(images)
    assert not calls and all(v.grad_fn is None for v in vals)


def test_a_codebook_beyond_the_quantiser_kernel_falls_back(monkeypatch):
    """The eval kernels take K <= SPK_ANN_VQVAE_MAX_K = 1024; the training quantiser stages the codebook in 64 KB of LDS ((D + 1)
    floats and a double per code): K <= 862 at D = 16.  The predicate the model asks says so, agrees with the entry point, and
    decides before any convolution is looked at -- a model with K = 1024 keeps the module path in train() mode."""
    from spkdiff import _lib, ops
    L, C = _lib.lib, _lib.CONSTANTS
    p = 4096

    def lds(D, K):
        return ((K * (D + 1) + 1) & ~1) * 4 + K * 8

    for D, K in ((16, 128), (16, 256), (16, 862), (16, 863), (16, 1024), (64, 244), (64, 245), (65, 8), (0, 8), (16, 0)):
        want = 1 <= D <= C["SPK_VQ_TRAIN_MAX_D"] and K >= 1 and lds(D, K) <= 64 * 1024
        assert bool(L.spk_ann_vqvae_train_supported(D, K)) is want, (D, K)
        if not want and D > 0 and K > 0:                            # (a supported call would launch)
            assert L.spk_ann_vqvae_train_vq_fwd(p, p, p, p, p, 0.25, p, 1 << 20, 49, D, K, None) == C["SPK_ERR_UNSUPPORTED"]
    assert ops.ann_vqvae_supported(1, 28, 28, 16, 1024) and not L.spk_ann_vqvae_train_supported(16, 1024)
    monkeypatch.setattr(ops, "conv_train_supported", lambda *a, **k: True)       # the convolutions are not what decides
    from snn_model.vae_model import VQVAE
    for K, want in ((862, True), (863, False), (1024, False)):
        m = VQVAE(1, 16, K, torch.tensor(1.0)).train()
        got = ops.ann_vqvae_train_supported((3, 1, 28, 28), m._enc_params(), m._dec_params(), m.vq_layer.embeddings.weight)
        assert got is want, K
    m = VQVAE(1, 16, 1024, torch.tensor(1.0)).train()
    l = m(torch.rand(2, 1, 28, 28) - 0.5)
    assert type(l[2].grad_fn).__name__ == "MseLossBackward0"
    x = (torch.rand(2, 1, 28, 28) - 0.5).requires_grad_(True)       # an image that wants a gradient gets one
    l = m(x)
    (l[0] + l[1]).backward()
    assert x.grad is not None and bool(x.grad.abs().sum() > 0)
