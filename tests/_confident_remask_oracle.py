"""Host oracle of remasking for confidence-ordered decoding (the rule: csrc/psample_common.h): the remask on one
image as a literal sort by (key, -position) (``remask_by_sort``) and as a mirror of the kernel's rank arithmetic
(``remask_by_rank``), one whole step on host copies (``remask_state``) and the count trajectory of a run (``run_counts_remask``).
Everything here is written out again, not imported from the package: tests/test_confident_remask_host.py compares the two.  The
order key is that of tests/_confident_oracle.py, the reveal count and commit those of tests/_confident_sched_oracle.py.  Host
tensors only."""
import numpy as np
import torch

import _confident_oracle as cfo
import _confident_sched_oracle as sco


def revisable_of(unmasked, commit_conf):
    """Unmasked at entry and commit_conf != +inf (a NaN is revisable: NaN != +inf)."""
    cc = np.asarray(commit_conf, dtype=np.float32)
    return np.asarray(unmasked, dtype=bool) & ~(cc == np.float32(np.inf))


def remask_count(R, c, t, m):
    """r of the rule: min(R, c); 0 at t = 1 and for an image with nothing masked at entry."""
    return 0 if (int(t) <= 1 or int(m) == 0) else min(int(R), int(c))


def remask_by_sort(revisable, commit_conf, r):
    """The definition on one image: sort the revisable positions by (key, -position), smallest first, take the first r."""
    revisable = np.asarray(revisable, dtype=bool)
    keys = cfo.conf_key(np.asarray(commit_conf, dtype=np.float32))
    order = sorted((p for p in range(len(revisable)) if revisable[p]), key=lambda p: (int(keys[p]), -p))
    out = np.zeros(len(revisable), dtype=bool)
    for p in order[:int(r)]:
        out[p] = True
    return out


def remask_by_rank(revisable, commit_conf, r):
    """The kernel's arithmetic (confident_remask): rank[p] = the number of revisable p' with key[p'] < key[p] or (equal and
    p' > p); remasked iff revisable and rank < r, unsigned 32-bit."""
    revisable = np.asarray(revisable, dtype=bool)
    keys = cfo.conf_key(np.asarray(commit_conf, dtype=np.float32)).astype(np.uint32)
    pos = np.arange(len(revisable))
    below = (keys[None, :] < keys[:, None]) | ((keys[None, :] == keys[:, None]) & (pos[None, :] > pos[:, None]))
    rank = (below & revisable[None, :]).sum(1).astype(np.uint32)
    return revisable & (rank < np.uint32(r))


def remask_state(x, un, cc, cand, conf32, score32, w_prev, w_cur, R, t, mask_id, remask=remask_by_sort):
    """One step on host copies.  x int64 [B, HW], un bool [B, HW], cc fp32 [B, HW] (commit_conf), cand int64 / conf32 fp32 / score32
    fp32 [B, HW] (the kernel's own outputs at the masked positions), w_prev / w_cur / R: B integers each (w[i][t - 1], w[i][t],
    remask_r[i][t]) -> (x, un, cc, revealed, remasked, [(n, r)])."""
    x, un, cc = x.clone(), un.clone(), cc.clone()
    rev = torch.zeros_like(un)
    rem = torch.zeros_like(un)
    counts = []
    for b in range(x.shape[0]):
        masked = ~un[b].numpy()
        m = int(masked.sum())
        n = sco.reveal_count(m, w_prev[b], w_cur[b])
        rv = revisable_of(un[b].numpy(), cc[b].numpy())
        r = remask_count(R[b], int(rv.sum()), t, m)
        revealed = torch.from_numpy(sco.commit_by_sort(masked, score32[b].numpy(), n))
        remasked = torch.from_numpy(remask(rv, cc[b].numpy(), r))
        assert not bool((revealed & remasked).any())
        x[b][revealed] = cand[b][revealed]
        un[b] |= revealed
        cc[b][revealed] = conf32[b][revealed]
        x[b][remasked] = int(mask_id)
        un[b] &= ~remasked
        rev[b], rem[b] = revealed, remasked
        counts.append((n, r))
    return x, un, cc, rev, rem, counts


def run_counts_remask(m0, w, R):
    """The (n_t, r_t) of a whole run of e = len(w) - 1 steps from m0 masked positions, t = e .. 1: the revisable count at entry of
    step t is m0 - m_t; an image with nothing masked does nothing."""
    m, out = int(m0), []
    for t in range(len(w) - 1, 0, -1):
        n = sco.reveal_count(m, w[t - 1], w[t])
        r = min(int(R[t]), int(m0) - m) if (t >= 2 and m > 0) else 0
        out.append((n, r))
        m = m - n + r
    return out
