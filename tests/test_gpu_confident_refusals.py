"""The return codes of the four confidence-ordered token updates of csrc/psample.hip -- spk_psample_step_conf, `_conf_listed`,
`_conf_sched` and `_conf_listed_sched` -- called through the ctypes binding itself, one broken argument at a time: which code each
refusal gives, that a bad argument is decided before an unsupported shape, and that a refused call leaves x_t / unmasked as they
were.  Every case is a refusal ahead of any launch: no kernel runs here (what the kernels compute is pinned by
test_gpu_confident.py, test_gpu_confident_steps.py and test_gpu_confident_sched.py)."""
import pytest
import torch

from spkdiff._lib import CONSTANTS, lib

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED = CONSTANTS["SPK_ERR_ARG"], CONSTANTS["SPK_ERR_UNSUPPORTED"]
B, HW, K, S, T_STEP = 2, 4, 8, 3, 2

# the arguments by name, in the order of include/spkdiff.h: the head all four share, then each form's tail (the stream is last)
HEAD = ("logits", "x_t", "unmasked", "t", "temp_b", "topk_b", "topp_b", "u", "q", "seed", "offset", "philox_state", "x0_hat", "conf",
        "B", "HW", "K")
TAILS = {
    "spk_psample_step_conf": ("next_input",),
    "spk_psample_step_conf_listed": ("steps_b", "S", "step_stride", "active", "n_active"),
    "spk_psample_step_conf_sched": ("next_input", "sched_w", "noise_a", "S", "score"),
    "spk_psample_step_conf_listed_sched": ("steps_b", "S", "step_stride", "active", "n_active", "sched_w", "noise_a", "score"),
}
ALL = tuple(TAILS)
WITH_S = ALL[1:]
LISTED = (ALL[1], ALL[3])
SCHED = (ALL[2], ALL[3])

# (what is broken, the forms that take it, the code)
CASES = [({name: None}, ALL, ARG) for name in ("logits", "x_t", "unmasked", "temp_b", "topk_b", "topp_b")]
CASES += [({name: 0}, ALL, ARG) for name in ("t", "B", "HW", "K")]
CASES += [({"t": S + 1}, WITH_S, ARG), ({"S": 0}, WITH_S, ARG)]
CASES += [({name: None}, LISTED, ARG) for name in ("steps_b", "active", "n_active")]
CASES += [({"sched_w": None}, SCHED, ARG)]
CASES += [({"HW": 65}, ALL, UNSUPPORTED), ({"K": 2049}, ALL, UNSUPPORTED)]
CASES += [({"t": 0, "HW": 65}, ALL, ARG)]                                       # a bad argument is decided first
PARAMS = [pytest.param(entry, broken, code, id=f"{entry[len('spk_psample_step_'):]}-" + "-".join(f"{k}={v}" for k, v in broken.items()))
          for broken, forms, code in CASES for entry in forms]


@pytest.fixture(scope="module")
def valid():
    """Every argument of a call all four forms accept, by name: buffers of B = 2, HW = 4, K = 8 (S = 3, t = 2), every optional
    one present.  No test writes them."""
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    n = B * HW
    x_t = torch.tensor([K, 3, K, K, 1, K, 7, K], dtype=torch.int64)
    return dict(
        logits=torch.randn(B, K, HW, generator=g).to(dev), x_t=x_t.to(dev), unmasked=(x_t != K).to(torch.uint8).to(dev), t=T_STEP,
        temp_b=torch.ones(B, device=dev), topk_b=torch.zeros(B, dtype=torch.int32, device=dev), topp_b=torch.ones(B, device=dev),
        u=torch.rand(n, generator=g).to(dev), q=torch.rand(n * K, generator=g).to(dev), seed=11, offset=0,
        philox_state=torch.tensor([11, 0], dtype=torch.int64, device=dev), x0_hat=torch.zeros(n, dtype=torch.int64, device=dev),
        conf=torch.zeros(n, device=dev), B=B, HW=HW, K=K, next_input=torch.zeros(B, 2, 2, 2, device=dev),
        steps_b=torch.full((B,), S, dtype=torch.int32, device=dev), S=S, step_stride=1 << 40,
        active=torch.arange(B, dtype=torch.int32, device=dev), n_active=torch.tensor([B, 0], dtype=torch.int32, device=dev),
        sched_w=torch.arange(S + 1, dtype=torch.int32).repeat(B, 1).contiguous().to(dev),
        noise_a=torch.zeros(B, S + 1, device=dev), score=torch.zeros(n, device=dev))


@pytest.mark.parametrize("entry,broken,code", PARAMS)
def test_refusal_code_and_state_untouched(valid, entry, broken, code):
    args = dict(valid, **broken)
    x_t0, unmasked0 = valid["x_t"].clone(), valid["unmasked"].clone()
    call = [args[name].data_ptr() if isinstance(args[name], torch.Tensor) else args[name] for name in HEAD + TAILS[entry]]
    rc = getattr(lib, entry)(*call, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == code, f"{entry} with {broken}: return code {rc}, expected {code}"
    assert torch.equal(valid["x_t"], x_t0) and torch.equal(valid["unmasked"], unmasked0), f"{entry} with {broken} wrote the state"
