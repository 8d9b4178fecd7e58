"""Reveal schedules and annealed selection noise of confidence-ordered decoding (the rule: csrc/psample_common.h):
the host-side builders of the two per-image tables the ``_sched`` entry points read, and the count arithmetic of the kernels as
integers.  Nothing here touches a device; ``AbsorbingDiffusion.sample_confident(schedule=, selection_noise=)`` calls these and
uploads the result.

A table row belongs to one image and is indexed by the loop's t = 0 .. S.  An image that runs e <= S steps of its own joins the
loop at t = e, so its row is the table of a run of e steps in entries 0 .. e; the entries above e are never read and repeat the
last one.

Remasking adds a third table of the same shape, the per-step remask counts (``remask_row``: zeros above e), and the
count trajectory of a run that reveals and remasks (``run_counts_remask``)."""
import math

W_MAX = 1 << 24                # the largest weight a schedule may hold (the kernels multiply it by m <= 64 in 64-bit arithmetic)


def linear_weights(e):
    """w[t] = t, t = 0 .. e: the count is m - floor(m (t - 1) / t) = ceil(m / t), the rule without a schedule."""
    e = _steps(e)
    return list(range(e + 1))


def cosine_weights(e):
    """w[t] = rint(2^24 sin(pi t / (2 e))) in fp64, t = 0 .. e: after progress r = (e - t) / e of the run the masked fraction is
    sin(pi t / (2 e)) = cos(pi r / 2).  w[0] = 0 (the last step reveals what is left), w[e] = 2^24."""
    e = _steps(e)
    return [int(round(W_MAX * math.sin(math.pi * t / (2.0 * e)))) for t in range(e + 1)]


def check_weights(w, what="schedule"):
    """A custom table: a sequence of integers in 0 .. 2^24 -> list of int (ValueError otherwise; a bool or a float is refused)."""
    try:
        w = list(w)
    except TypeError:
        raise ValueError(f"{what}: a weight table is a sequence of integers, got {w!r}") from None
    out = []
    for v in w:
        if isinstance(v, bool) or not hasattr(v, "__index__"):
            raise ValueError(f"{what}: a weight is an integer in 0 .. 2^24, got {v!r}")
        v = v.__index__()
        if not 0 <= v <= W_MAX:
            raise ValueError(f"{what}: a weight is an integer in 0 .. 2^24, got {v}")
        out.append(v)
    return out


def weights_row(schedule, e, S, what="schedule"):
    """Row of S + 1 weights for an image that runs e = min(its steps, S) steps: ``schedule`` is None / 'linear', 'cosine' or a
    custom table of e + 1 weights (S + 1 is taken too: entries above e are not read)."""
    e, S = _steps(e), _steps(S)
    if e > S:
        raise ValueError(f"{what}: an image runs at most the loop's S = {S} steps, got {e}")
    if schedule is None or (isinstance(schedule, str) and schedule == "linear"):
        w = linear_weights(e)
    elif isinstance(schedule, str) and schedule == "cosine":
        w = cosine_weights(e)
    elif isinstance(schedule, str):
        raise ValueError(f"{what}: a named schedule is 'linear' or 'cosine', got {schedule!r}")
    else:
        w = check_weights(schedule, what)
        if len(w) not in (e + 1, S + 1):
            raise ValueError(f"{what}: a table for {e} steps holds {e + 1} weights (t = 0 .. {e}), got {len(w)}")
    w = w[:S + 1]
    return w + [w[-1]] * (S + 1 - len(w))


def noise_scales(tau, e, S):
    """Row of S + 1 fp64 noise scales of one image: a[t] = tau * (t - 1) / e for 1 <= t <= e (MaskGIT's linear decay: the last step,
    t = 1, is noise-free), 0 elsewhere.  The caller rounds to fp32.  tau >= 0 and finite."""
    e, S = _steps(e), _steps(S)
    tau = check_tau(tau)
    return [tau * (t - 1) / e if 1 <= t <= e else 0.0 for t in range(S + 1)]


def check_tau(tau, what="selection_noise"):
    if isinstance(tau, bool):
        raise ValueError(f"{what}: a number >= 0, got {tau!r}")
    try:
        v = float(tau)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a number >= 0, got {tau!r}") from None
    if not (math.isfinite(v) and v >= 0):
        raise ValueError(f"{what}: finite and >= 0, got {tau!r}")
    return v


def reveal_count(m, w_prev, w_cur):
    """The kernels' count (sched_reveal_count): how many of m masked positions a step with weights w[t - 1], w[t] reveals."""
    m, w_prev, w_cur = int(m), int(w_prev), int(w_cur)
    keep = 0 if w_cur == 0 else min(m, (m * w_prev) // w_cur)
    n = m - keep
    return 1 if m > 0 and n == 0 else n


def reveal_counts(m0, w):
    """How many tokens each step of a run commits: ``w`` a table of e + 1 weights, ``m0`` the positions masked at the start ->
    list of e counts, for t = e, e - 1, .. 1."""
    w = check_weights(w)
    if len(w) < 2:
        raise ValueError("reveal_counts: a table holds at least two weights (t = 0, 1)")
    m, out = int(m0), []
    for t in range(len(w) - 1, 0, -1):
        n = reveal_count(m, w[t - 1], w[t])
        out.append(n)
        m -= n
    return out


def remask_row(remask, e, S, what="remask"):
    """Row of S + 1 remask counts for an image that runs e = min(its steps, S) steps, placed as ``weights_row``
    places a schedule row: ``remask`` is None / 0 (nothing), an integer r >= 0 (up to r tokens at every step 2 <= t <= e) or a
    sequence of e + 1 non-negative integers indexed by t whose entries 0 and 1 are 0 (S + 1 is taken too: entries above e must be
    0, they are never read).  Entries above e are 0."""
    e, S = _steps(e), _steps(S)
    if e > S:
        raise ValueError(f"{what}: an image runs at most the loop's S = {S} steps, got {e}")
    if remask is None:
        remask = 0
    if isinstance(remask, bool) or isinstance(remask, (str, float)):
        raise ValueError(f"{what}: an integer >= 0 or a table of e + 1 integers >= 0, got {remask!r}")
    if hasattr(remask, "__index__") and getattr(remask, "ndim", 0) == 0:
        r = remask.__index__()
        if not 0 <= r <= 0x7FFFFFFF:
            raise ValueError(f"{what}: a count is an integer >= 0, got {r}")
        row = [0, 0] + [r] * (e - 1)
    else:
        try:
            row = list(remask)
        except TypeError:
            raise ValueError(f"{what}: an integer >= 0 or a table of e + 1 integers >= 0, got {remask!r}") from None
        for v in row:
            if isinstance(v, bool) or not hasattr(v, "__index__") or not 0 <= v.__index__() <= 0x7FFFFFFF:
                raise ValueError(f"{what}: a count is an integer >= 0, got {v!r}")
        row = [v.__index__() for v in row]
        if len(row) not in (e + 1, S + 1):
            raise ValueError(f"{what}: a table for {e} steps holds {e + 1} counts (t = 0 .. {e}), got {len(row)}")
        if any(row[:2]) or any(row[e + 1:]):
            raise ValueError(f"{what}: the entries at t = 0 and t = 1 are 0 (the last step reveals what is left and remasks nothing), "
                             f"and so are those above the image's {e} steps, got {row}")
        row = row[:e + 1]
    return row + [0] * (S + 1 - len(row))


def run_counts_remask(m0, w, r):
    """The counts of a whole run with remasking: ``w`` a table of e + 1 weights, ``r`` one of e + 1 remask counts,
    ``m0`` the positions masked at the start -> list of e pairs (n_t, r_t) for t = e .. 1.  The revisable count at entry of step t
    is m0 - m_t, so n_t = reveal_count(m_t, w[t - 1], w[t]), r_t = min(r[t], m0 - m_t) for t >= 2 and m_t > 0, else 0, and
    m_(t-1) = m_t - n_t + r_t: the n sum to m0 plus the sum of the r."""
    w = check_weights(w)
    r = remask_row(r, len(w) - 1, len(w) - 1) if len(w) >= 2 else []
    if len(w) < 2:
        raise ValueError("run_counts_remask: a table holds at least two weights (t = 0, 1)")
    m0 = int(m0)
    m, out = m0, []
    for t in range(len(w) - 1, 0, -1):
        n = reveal_count(m, w[t - 1], w[t])
        rt = min(r[t], m0 - m) if (t >= 2 and m > 0) else 0
        out.append((n, rt))
        m = m - n + rt
    return out


def _steps(e):
    if isinstance(e, bool) or not hasattr(e, "__index__") or e.__index__() < 1:
        raise ValueError(f"a step count is an integer >= 1, got {e!r}")
    return e.__index__()
