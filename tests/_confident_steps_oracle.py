"""Host oracle of per-image step counts for confidence-ordered decoding (the rule: include/spkdiff.h): the steps an
image really runs (``effective_steps``), the list of pending images a reverse step works on (``pending``), the step counts
``positions_per_step`` chooses (``steps_for_hole``) and the counter offset the listed kernel draws image i at (``image_offset``).
The schedule ceil(m / t) is tests/_confident_oracle.n_reveal.  Host integers and tensors only."""
import torch

STEP_STRIDE = 1 << 40                     # the 'global' noise layout: counters per reverse step (AbsorbingDiffusion.STEP_STRIDE)
U64 = (1 << 64) - 1


def effective_steps(steps_b, S):
    """e_i = min(steps_b[i], S) for every image: the steps image i runs inside a loop of S (an entry < 1 stays < 1: never pending)."""
    return [min(int(s), int(S)) for s in steps_b]


def pending(unmasked, t, steps_b):
    """The ascending list of images pending at reverse step t: 1 <= t <= steps_b[i] and at least one position masked.
    ``unmasked``: bool [B, ...] host tensor (true = revealed); ``steps_b``: B integers.  (t <= S always inside a loop of S, so
    t <= steps_b[i] is t <= e_i.)"""
    un = unmasked.reshape(unmasked.shape[0], -1).bool()
    return [b for b in range(un.shape[0]) if 1 <= int(t) <= int(steps_b[b]) and not bool(un[b].all())]


def steps_for_hole(m, r):
    """s = max(1, ceil(m / r)): the step count ``positions_per_step = r`` gives an image with m unknown positions."""
    return max(1, (int(m) + int(r) - 1) // int(r))


def image_offset(offset, S, e, stride=STEP_STRIDE):
    """The counter offset of image i at a loop step whose own offset is ``offset``: offset - (S - e_i) * stride in unsigned 64-bit
    arithmetic, as the kernel computes it."""
    return (int(offset) - (int(S) - int(e)) * int(stride)) & U64


def loop_offset(S, t, base=0, stride=STEP_STRIDE):
    """The offset the sampler hands to loop step t of S: step index S - t, plus the shard's counter base."""
    return (int(S) - int(t)) * int(stride) + int(base)


def select_case(B, HW, t, S, seed):
    """The seeded case of the spk_select_pending test: ``unmasked`` bool [B, 1, HW, 1] whose images cycle through m = 0, 1, HW and
    a seeded count of masked positions at seeded places, and ``steps_b`` int32 [B] cycling through -3, 0, t - 1, t, t + 1, S + 5 with
    a period coprime to the first, so that every (m, entry) pair with m in {0, 1, HW} occurs from B = 24 on and a ragged batch
    still mixes them."""
    g = torch.Generator().manual_seed(seed)
    un = torch.ones(B, HW, dtype=torch.bool)
    entries = (-3, 0, t - 1, t, t + 1, S + 5)
    steps = torch.empty(B, dtype=torch.int32)
    for b in range(B):
        m = (0, 1, HW, int(torch.randint(0, HW + 1, (1,), generator=g)))[b % 4]
        un[b, torch.randperm(HW, generator=g)[:m]] = False
        steps[b] = entries[(b // 4 + b) % 6]
    return un.reshape(B, 1, HW, 1), steps
