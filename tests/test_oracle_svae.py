"""CPU tests: the SNN_VAE loops of the oracle (oracle/snn_ref.py, SNN_VAE section) against fixtures F16 and F17, which the
real reference computed with ``synth.synth_svae_state`` weights (tools/gen_golden_svae.py, tools/gen_golden_svae_train.py).
Every comparison is bit for bit.  These pin the oracle that tests/test_gpu_snn_vae_shapes.py uses at the shapes the fixtures cannot reach."""
import os

import numpy as np
import pytest
import torch

from oracle import snn_ref as ref
from spkdiff import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = os.path.join(ROOT, "tests", "golden", "f16_snn_vae.npz")
F17 = os.path.join(ROOT, "tests", "golden", "f17_snn_vae_train.npz")
SEED_FWD, SEED_SAMPLE = 16, 1616          # tools/gen_golden_svae.py
C, K = 56, 20


@pytest.fixture(scope="module")
def sd():
    return synth.synth_svae_state()


def unpack(f, key):
    shape = tuple(int(s) for s in f[key + "_shape"])
    return torch.from_numpy(np.unpackbits(f[key], axis=-1, count=shape[-1]).reshape(shape)).float()


def layers(sd, name):
    return [(sd[f"{name}.layers.{i}.weight"], sd[f"{name}.layers.{i}.bias"]) for i in (0, 2, 4)]


def zero_state(sd, name, B):
    return [torch.zeros(B, sd[f"{name}.layers.{i}.weight"].shape[0]) for i in (0, 2, 4)]


def test_posterior_matches_f16(sd):
    f = np.load(F16)
    x = unpack(f, "latent_x")
    T, B = x.shape[0], x.shape[1]
    torch.manual_seed(SEED_FWD)
    idx = ref.svae_draw_indices(T, B, C, K)
    vs = zero_state(sd, "posterior", B)
    z, q = ref.svae_posterior(x, sd["posterior.initial_input"], layers(sd, "posterior"), vs, idx)
    assert torch.equal(z, unpack(f, "sampled_z"))
    assert q.shape == (T, B, C * K)
    for i, v in zip((1, 3, 5), vs):
        assert torch.equal(v, torch.from_numpy(f[f"v/posterior.layers.{i}"])), i


def test_two_prior_samples_without_reset_match_f16(sd):
    f = np.load(F16)
    vs = zero_state(sd, "prior", 32)
    torch.manual_seed(SEED_SAMPLE)
    for c in range(2):
        idx = ref.svae_draw_indices(16, 32, C, K)
        z = ref.svae_prior_sample(sd["prior.initial_input"], layers(sd, "prior"), vs, idx)
        assert torch.equal(z, unpack(f, f"sample{c}_z")), c
        for i, v in zip((1, 3, 5), vs):
            assert torch.equal(v, torch.from_numpy(f[f"sample{c}_v/prior.layers.{i}"])), (c, i)


def test_posterior_matches_f17(sd):
    f = np.load(F17)
    x = unpack(f, "latent_x")
    idx = torch.from_numpy(f["idx"])
    vs = zero_state(sd, "posterior", x.shape[1])
    z, q = ref.svae_posterior(x, sd["posterior.initial_input"], layers(sd, "posterior"), vs, idx)
    assert torch.equal(z, unpack(f, "sampled_z"))
    assert torch.equal(q, unpack(f, "q_z"))
    for i, v in zip((1, 3, 5), vs):                # the training loop's grad pass is the same fp32 update as the eval pass
        assert torch.equal(v, torch.from_numpy(f[f"v/posterior.layers.{i}"])), i


@pytest.mark.parametrize("prefix", ["", "p3/"], ids=["p0", "p03"])
def test_prior_scheduled_prefix_matches_f17(sd, prefix):
    """The p = 0.3 run schedules steps (p3/sched, its recorded randn_like draws in p3/noise); the p = 0 run schedules none,
    so its z_t_minus is the teacher [z0, sampled_z[:-1]]."""
    f = np.load(F17)
    zt = unpack(f, prefix + "sampled_z")
    T, B = zt.shape[0], zt.shape[1]
    if prefix:
        sched, noise = torch.from_numpy(f[prefix + "sched"]), torch.from_numpy(f[prefix + "noise"])
        assert int(sched.sum()) == noise.shape[0] > 0
    else:
        sched, noise = torch.zeros(T - 1, dtype=torch.bool), torch.zeros(0, B, C)
    vs = zero_state(sd, "prior", B)
    zm = ref.svae_prior_prefix(sd["prior.initial_input"], layers(sd, "prior"), vs, sched, noise, zt)
    assert torch.equal(zm, unpack(f, prefix + "z_t_minus"))
    p_z = ref.svae_mlp(zm, layers(sd, "prior"), vs)             # the grad pass over z_t_minus
    assert torch.equal(p_z, unpack(f, prefix + "p_z"))
    for i, v in zip((1, 3, 5), vs):
        key = f"{prefix}v/prior.layers.{i}"
        assert torch.equal(v, torch.from_numpy(f[key])), key
