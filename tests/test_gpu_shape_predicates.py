"""The latents on which the int8 matrix-core launch refuses what ``ops.den_mfma_supported`` used to accept (9x7, 7x9: nine input-slab
copy pieces per wave) run through the containers on the direct kernels, bit-equal to the host oracle; and each denoiser entry point
refuses, before any launch, a shape its predicate refuses."""
import pytest
import torch

import _conv_bn_lif_oracle as O
from oracle import snn_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from spkdiff import ops as o
    return o


@pytest.mark.parametrize("H,W", [(9, 7), (7, 9)], ids=["9x7", "7x9"])
def test_fused_sequential_on_a_drift_latent(dev, ops, H, W):
    """Conv2d(32, 32, 3, 1, 1) + BN + LIF in eval mode on random CPTC spikes [1, 1, H, W, 16, 32]: impl='auto' does not raise and
    equals impl='direct' and the host oracle bit for bit."""
    from spikingjelly.activation_based import functional, layer, neuron
    from spkdiff.fused import FusedSequential
    assert not ops.den_mfma_supported(32, 32, 3, 1, 1, 16, H, W) and not ops.den_fp6_supported(64, 64, 3, 1, 1, 16, H, W)
    geo = (32, 32, 3, 1, 1, False, 0, H, W, 1)
    c = O.make_case(geo, 4100 + H, kind="spikes")
    g = torch.Generator().manual_seed(4200 + H)
    conv, bn = layer.Conv2d(32, 32, 3, 1, 1), layer.BatchNorm2d(32)
    with torch.no_grad():
        conv.weight.copy_(c.w); conv.bias.copy_(c.bias)
        bn.weight.copy_(torch.rand(32, generator=g) + 1.0); bn.bias.copy_(torch.rand(32, generator=g) * 0.8)
        bn.running_mean.copy_(torch.rand(32, generator=g) * 0.6 - 0.3); bn.running_var.copy_(torch.rand(32, generator=g) * 0.5 + 0.5)
    sd = {"b." + k: v.detach().clone() for k, v in bn.state_dict().items() if v.dtype == torch.float32}
    a, b = ref.bn_affine_terms(sd, "b")
    want, _, _ = O.conv_bn_lif(c.x, c.w, c.bias, a, b, None, geo)
    assert 0.02 <= float(want.mean()) <= 0.6, float(want.mean())
    net = FusedSequential(conv, bn, neuron.LIFNode())
    functional.set_step_mode(net, "m")
    net = net.to(dev).eval()
    x = O.to_ptc(c.x, 32).to(dev)
    assert tuple(x.shape) == (1, 1, H, W, 16, 32)
    with torch.inference_mode():
        auto = net.run(x, ops.IN_PTC, final="ptc", chunk_out=32, impl="auto", stateful=False)["ptc"]
        direct = net.run(x, ops.IN_PTC, final="ptc", chunk_out=32, impl="direct", stateful=False)["ptc"]
    assert torch.equal(auto, direct)
    assert torch.equal(auto.cpu(), O.to_ptc(want, 32))


def test_denoiser_forward_on_a_drift_latent_equals_the_direct_request(dev):
    from spkdiff import synth
    from snn_model.vq_diffusion import DummyModel, functional
    den = DummyModel(1, 128).to(dev)
    functional.set_step_mode(net=den, step_mode='m')
    den.load_state_dict(synth.synth_denoiser_state(synth.MNIST))
    den.eval()
    assert den.impl_for(9, 7) == 'direct-f64'
    tok = torch.randint(0, 129, (1, 1, 9, 7), generator=torch.Generator().manual_seed(5)).float().to(dev)
    t = torch.full((1,), 5, device=dev)
    with torch.inference_mode():
        auto = den(tok, t)
        functional.reset_net(den)
        den.conv_impl_request = 'direct'
        direct = den(tok, t)
        functional.reset_net(den)
    assert tuple(auto.shape)[-2:] == (9, 7) and bool(torch.isfinite(auto).all())
    assert torch.equal(auto, direct)


def _bn(dev, C):
    return torch.ones(C, device=dev), torch.zeros(C, device=dev)


@pytest.mark.parametrize("family", ["i8", "fp6", "fp6v2"])
def test_entry_point_refuses_what_its_predicate_refuses(dev, ops, family):
    """SPK_ERR_UNSUPPORTED (-2 -> NotImplementedError): an error return before any launch."""
    if family == "i8":
        H, W, C = 9, 7, 32
        assert not ops.den_mfma_supported(C, C, 3, 1, 1, 16, H, W)
        packed = ops.den_pack_weight_i8(torch.zeros(C, C, 3, 3, device=dev), None)
        x = torch.zeros((1, 1, H, W, 16, 32), dtype=torch.uint8, device=dev)
        a, b = _bn(dev, C)
        with pytest.raises(NotImplementedError, match="spk_den_conv3x3_mfma"):
            ops.den_conv3x3_mfma(x, packed, C, mode=ops.MODE_LIF, bn_a=a, bn_b=b)
    elif family == "fp6":
        H, W, C = 9, 7, 64
        assert not ops.den_fp6_supported(C, C, 3, 1, 1, 16, H, W)
        packed = ops.den_pack_weight_fp6(torch.zeros(C, C, 3, 3, device=dev), None)
        x = torch.zeros((1, 1, H, W, 16, 32), dtype=ops.C4_DTYPE, device=dev)
        a, b = _bn(dev, C)
        with pytest.raises(NotImplementedError, match="spk_den_conv3x3_mfma_fp6"):
            ops.den_conv3x3_mfma_fp6(x, packed, C, bn_a=a, bn_b=b)
    else:
        H, W, C = 9, 9, 32
        assert not ops.den_fp6v2_supported(C, C, 3, 1, 1, 16, H, W)
        packed = ops.den_pack_weight_fp6v2(torch.zeros(C, C, 3, 3, device=dev), None)
        x = torch.zeros((1, 1, H, W, 16, 16), dtype=ops.C4_DTYPE, device=dev)
        a, b = _bn(dev, C)
        with pytest.raises(NotImplementedError, match="spk_den_conv3x3_mfma_fp6v2"):
            ops.den_conv3x3_mfma_fp6v2(x, packed, C, bn_a=a, bn_b=b)
    torch.cuda.synchronize()
