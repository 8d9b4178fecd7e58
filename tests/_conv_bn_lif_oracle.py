"""Host oracle of the inference Conv + BN + LIF kernels (csrc/conv_direct.hip, csrc/conv_mfma_gather.hip, csrc/vae_fp6.hip) on DYADIC
inputs, and the case tables of tests/test_conv_bn_lif_oracle_host.py / tests/test_gpu_conv_bn_lif_oracle.py.  No GPU, nothing of the
library: torch's fp64 convolution on the CPU, one rounding to fp32, a single-rounding fp32 fma and the reference's LIF step
(oracle/snn_ref.py lif_multi_step).

Why dyadic: the kernels' contract is  exact dot product + bias -> ONE rounding to fp32 -> fmaf(y, a, b) -> fp32 LIF.
With spikes / pixels that are multiples of 2^-8, weights multiples of 2^-12 (|w| < 1), biases multiples of 2^-10 and BN terms
multiples of 2^-6, every fp64 partial sum of the convolution is exact IN ANY ORDER (products are multiples of 2^-20 below 2^14: 34
bits of 53), the gather kernel's 2^-30 fixed point holds the weights exactly, and x * a + b needs fewer than 53 bits.  So there is one
correct spike train per neuron, bit for bit: no fragile set, no tolerance, nothing to exclude.

FULL-WIDTH weights (make_case(weights="full"); the denoiser's matrix-core kernels of csrc/den_mfma.hip, den_mfma_fp6.hip and
den_mfma_fp6v2.hip, and a second pass over the gather and vae_fp6 rows).  Multiples of 2^-12 below 0.5 fill only the top ~12 bits of the
kernels' per-channel fixed point (shift 29 - e for six radix-32 digits, 30 - e for four radix-256 digits, e = the frexp exponent of the
channel maximum): the two or three lowest digit planes of every MFMA kernel are zero on them.  The full-width scheme draws, per output
channel, an exponent e and integers q of log-uniform magnitude in [2^4, 2^29), rounded to fp32 (24 significant bits, still an integer),
and sets w = q * 2^(e-29); one tap per channel is 2^29 - 2^5, so the channel maximum lies in [2^(e-1), 2^e).  Then w * 2^(29-e) and
w * 2^(30-e) are integers (the packing is exact, all six / four digits in play), and with BINARY inputs (or spike counts <= 16) every
fp64 partial sum is an integer multiple of 2^(e-29) below 2^46: exact in any order.  The contract again has ONE answer per neuron."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import snn_ref as ref

T16 = 16
SPIKE_DENSITY = 0.15


# ------------------------------------------------------------------------------------------------ single-rounding fp32 fma
def fma32(x, a, b):
    """fmaf(x, a, b) on fp32 numpy arrays or torch tensors (broadcast), rounded ONCE.  The product of two fp32 values is exact in
    fp64; the sum p + b is not, and rounding it to fp64 and then to fp32 rounds twice.  TwoSum gives the residual err of
    p + b = s + err exactly; the second rounding goes wrong only where s sits exactly midway between two fp32 values (there
    round-to-nearest-even decides without knowing err), and there the sign of err decides."""
    is_torch = torch.is_tensor(x)
    xs = [np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float32) for t in (x, a, b)]
    p = xs[0].astype(np.float64) * xs[1].astype(np.float64)
    b64 = xs[2].astype(np.float64)
    s = p + b64
    bb = s - p
    err = (p - (s - bb)) + (b64 - bb)                          # TwoSum (Knuth): p + b == s + err exactly
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)                               # exact (Sterbenz)
    with np.errstate(over="ignore", invalid="ignore"):
        up = np.nextafter(r, np.float32(np.inf)).astype(np.float64)
        dn = np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
        tie_up = (d > 0) & ((up - s) == d) & (err > 0)         # s is the midpoint (r, up) and the true sum lies above it
        tie_dn = (d < 0) & ((s - dn) == -d) & (err < 0)
    r = np.where(tie_up, up.astype(np.float32), np.where(tie_dn, dn.astype(np.float32), r)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(r)) if is_torch else r


def fma32_naive(x, a, b):
    """The double-rounding form fma32 replaces (kept for the host test that shows the tie set is adversarial)."""
    x, a, b = (np.asarray(t, dtype=np.float32) for t in (x, a, b))
    return (x.astype(np.float64) * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)


def round_fraction_f32(q):
    """A rational number -> the nearest fp32 value, ties to even (exact arithmetic; normal range)."""
    c = np.float32(float(q))
    cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - q), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def fma32_exact(x, a, b):
    """Element-wise fma by exact rational arithmetic (slow; the reference of the host test)."""
    return np.array([round_fraction_f32(Fraction(float(xi)) * Fraction(float(ai)) + Fraction(float(bi)))
                     for xi, ai, bi in zip(x, a, b)], dtype=np.float32)


def fma_tie_set(n, seed):
    """Triples built to land on the ties of the SECOND rounding of the naive form: b = t in [0.5, 4), x = ulp(t)/2 * (1 + 2^-23),
    a = 1 -/+ 2^-23.  x * a is half an ulp of t minus / plus a part far below fp64's last bit of t + x * a."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.5, 4.0, n).astype(np.float32)
    ulp = (np.nextafter(t, np.float32(np.inf)) - t).astype(np.float32)
    x = (ulp * np.float32(0.5) * np.float32(1.0 + 2.0 ** -23)).astype(np.float32)
    a = np.where(rng.integers(0, 2, n) == 0, np.float32(1.0 - 2.0 ** -23), np.float32(1.0 + 2.0 ** -23)).astype(np.float32)
    return x, a, t


# ------------------------------------------------------------------------------------------------ inputs
def dyadic(shape, gen, bits, amp):
    """Random multiples of 2^-bits in [-amp, amp) as fp32 (amp * 2^bits must be an integer >= 1)."""
    n = int(round(amp * 2 ** bits))
    assert n >= 1 and n == amp * 2 ** bits
    return torch.randint(-n, n, tuple(shape), generator=gen).float() * 2.0 ** -bits


def out_size(n, k, s, p, transposed, out_pad):
    return (n - 1) * s - 2 * p + k + out_pad if transposed else (n + 2 * p - k) // s + 1


def geo_out_hw(geo):
    Cin, Cout, k, s, p, tr, op, H, W, B = geo
    return out_size(H, k, s, p, tr, op), out_size(W, k, s, p, tr, op)


def tinv_geo(row):
    """(Cin, Cout, k, s, p, H, W, B) of a time-invariant row -> the ten-field geometry tuple (plain convolution)."""
    Cin, Cout, k, s, p, H, W, B = row
    return (Cin, Cout, k, s, p, False, 0, H, W, B)


def _pow2_floor(v):
    return 2.0 ** int(np.floor(np.log2(v)))


def make_case(geo, seed, kind="spikes", T=T16, n_inputs=1, weights="dyadic12"):
    """Inputs of one row.  kind 'spikes': binary [T,B,Cin,H,W] at density 0.15; 'seq': dyadic reals (multiples of 2^-8, |x| < 4);
    'pixels': ONE dyadic frame [B,Cin,H,W] (multiples of 2^-8, |x| < 1; the time-invariant layers).  Weights are multiples of 2^-12
    scaled (by a power of two) so that the pre-activation has a spread of about one; bias multiples of 2^-10; BN scale a = multiples
    of 2^-6 with 0.5 <= |a| < 2, a quarter of them negative; BN shift b multiples of 2^-6 in [-0.5, 1); v0 multiples of 2^-8 in
    [-1, 1) (below the threshold, as a carried membrane potential is).  ``xs`` holds n_inputs independent inputs (carried-state
    tests call the layer twice); they are drawn last, so the parameters and input 0 do not depend on n_inputs.
    weights="full": the full-width scheme of make_full_case (spike inputs only); the default leaves every draw as it was."""
    if weights == "full":
        if kind != "spikes":
            raise ValueError("full-width weights need binary inputs: with 'seq' / 'pixels' inputs the partial sums take 52 bits")
        return make_full_case(geo, seed, T=T, n_inputs=n_inputs)
    if weights != "dyadic12":
        raise ValueError(weights)
    Cin, Cout, k, s, p, tr, op, H, W, B = geo
    g = torch.Generator().manual_seed(seed)
    taps = Cin * k * k / (s * s if tr else 1)                 # taps that reach one output of a transposed layer: k*k / s*s
    power = {"spikes": SPIKE_DENSITY, "seq": 16.0 / 3.0, "pixels": 1.0 / 3.0}[kind]
    amp = min(0.5, max(2.0 ** -6, _pow2_floor(2.5 / np.sqrt(power * taps))))
    w = dyadic((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), g, 12, amp)
    bias = dyadic((Cout,), g, 10, 0.25)
    a = (torch.randint(32, 128, (Cout,), generator=g).float() / 64.0) * torch.where(torch.rand(Cout, generator=g) < 0.25, -1.0, 1.0)
    b = torch.randint(-32, 64, (Cout,), generator=g).float() / 64.0
    Ho, Wo = geo_out_hw(geo)
    v0 = dyadic((B, Cout, Ho, Wo), g, 8, 1.0)
    xs = []
    for _ in range(n_inputs):
        if kind == "spikes":
            xs.append((torch.rand((T, B, Cin, H, W), generator=g) < SPIKE_DENSITY).float())
        elif kind == "seq":
            xs.append(dyadic((T, B, Cin, H, W), g, 8, 4.0))
        else:
            xs.append(dyadic((B, Cin, H, W), g, 8, 1.0))
    coef = torch.pow(torch.tensor(0.8), torch.arange(T - 1, -1, -1).float())      # the model's membrane read-out weights
    return SimpleNamespace(geo=geo, kind=kind, T=T, xs=xs, x=xs[0], w=w, bias=bias, a=a, b=b, v0=v0, coef=coef, Ho=Ho, Wo=Wo,
                           weights=weights, graze=[])


# ------------------------------------------------------------------------------------------------ full-width weights
FULL_STD = 0.17            # sqrt(E[w^2]) / 2^e of the scheme: |q| = 2^u, u uniform in [4, 29):  E[4^(u-29)] = 1 / (50 ln 2) = 0.0289
Q_PIN = 2.0 ** 29 - 2.0 ** 5


def full_width_weights(Cout, Cin, k, g, e_lo, e_hi):
    """[Cout,Cin,k,k] fp32 weights w = q * 2^(e-29) and the int64 exponents e [Cout] (uniform in [e_lo, e_hi])."""
    e = torch.randint(e_lo, e_hi + 1, (Cout,), generator=g)
    bits = 4.0 + 25.0 * torch.rand((Cout, Cin, k, k), generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand((Cout, Cin, k, k), generator=g) < 0.5, -1.0, 1.0).double()
    q = (torch.floor(torch.exp2(bits)) * sign).float().double()         # 24 significant bits: still an integer, |q| <= 2^29 - 2^5
    q[:, 0, k // 2, k // 2] = Q_PIN                                      # pins the channel maximum into [2^(e-1), 2^e)
    w = (q * torch.exp2((e - 29).double()).view(-1, 1, 1, 1)).float()
    assert torch.equal(w.double(), q * torch.exp2((e - 29).double()).view(-1, 1, 1, 1))
    return w, e


def channel_exponent(w, transposed=False):
    """The frexp exponent of every output channel's largest magnitude, as the pack kernels take it (m = f * 2^e, f in [0.5, 1))."""
    m = (w.transpose(0, 1) if transposed else w).flatten(1).abs().amax(1).double().numpy()
    return torch.from_numpy(np.frexp(m)[1].astype(np.int64))


def lif_h0(z0):
    """The charged potential of step 0 from the reset state, as ref.lif_multi_step computes it: h = v + (z - v) / 2 with v = 0."""
    v = torch.zeros_like(z0)
    return v + (z0 - v) / 2.0


def _graze_pref(shape, pref):
    """The neurons [B,H,W] a constructed channel should sit on, by preference: 0 the last position (the last-position launches of an
    odd map), 1 a position below it in the last image, 2 row H/2 - 1 in image 0, 3 row H/2 in the last image (the two row bands
    of an 8x8 map)."""
    B, H, W = shape
    m = torch.zeros(shape, dtype=torch.bool)
    if pref == 0:
        m[:, H - 1, W - 1] = True
    elif pref == 1:
        m[B - 1] = True
        m[B - 1, H - 1, W - 1] = False
    elif pref == 2:
        m[0, max(H // 2 - 1, 0)] = True
    else:
        m[B - 1, H // 2] = True
    return m


def _graze_pick(cand, order, pref):
    """(channel, image, y, x): the first channel of ``order`` with a candidate neuron on the preferred set; failing that, the first
    channel with any candidate; None if no channel has one.  cand: bool [B,C,H,W]."""
    m = _graze_pref(cand[:, 0].shape, pref)
    for mask in (m, torch.ones_like(m)):
        for c in order:
            idx = (cand[:, c] & mask).nonzero()
            if len(idx):
                return (c,) + tuple(int(v) for v in idx[0])
    return None


def make_full_case(geo, seed, T=T16, n_inputs=1):
    """make_case(weights="full").  Bias multiples of 2^-10; ordinary channels carry BN terms as in the 2^-12 scheme; v0 likewise.
    The channel exponents lie in [e_hi - 3, e_hi] (clamped to [-6, 0]) with e_hi chosen so that the pre-activation of the widest
    channels has a spread of about 2.5.

    THRESHOLD-GRAZING CHANNELS.  A random draw no longer lands on h == 1.0, so it is built: in a quarter of the output channels
    a = 1 and b = 2 - y32 for one neuron whose oracle pre-activation y32 of step 0 (input 0, reset state) lies in [1, 2): the
    difference is exact, z = fma(y32, 1, b) = 2 and h = 1.0 exactly -- the neuron fires (>=).  In a further eighth b is the LARGEST
    fp32 value for which the oracle's h at that neuron stays below 1, found by stepping down with nextafter (y32 + b may round
    back up to 2).  ``graze`` lists them: (kind 'fire' | 'below', channel, image, y, x).  The channels are taken in a seeded order,
    each slot preferring a channel that has such a neuron where _graze_pref wants one; a channel with no y32 in [1, 2) stays ordinary."""
    Cin, Cout, k, s, p, tr, op, H, W, B = geo
    g = torch.Generator().manual_seed(seed)
    taps = Cin * k * k / (s * s if tr else 1)
    e_hi = int(np.clip(np.round(np.log2(2.5 / (FULL_STD * np.sqrt(SPIKE_DENSITY * taps)))), -3, 0))
    w, e = full_width_weights(Cout, Cin, k, g, max(e_hi - 3, -6), e_hi)
    if tr:
        w = w.transpose(0, 1).contiguous()
    bias = dyadic((Cout,), g, 10, 0.25)
    a = (torch.randint(32, 128, (Cout,), generator=g).float() / 64.0) * torch.where(torch.rand(Cout, generator=g) < 0.25, -1.0, 1.0)
    b = torch.randint(-32, 64, (Cout,), generator=g).float() / 64.0
    Ho, Wo = geo_out_hw(geo)
    v0 = dyadic((B, Cout, Ho, Wo), g, 8, 1.0)
    order = torch.randperm(Cout, generator=g).tolist()                   # which channels graze: a function of the seed alone
    xs = [(torch.rand((T, B, Cin, H, W), generator=g) < SPIKE_DENSITY).float() for _ in range(n_inputs)]
    y0 = conv64(xs[0][0], w, bias, geo).float()                          # [B,Cout,Ho,Wo]: the oracle's y32 of step 0
    n_fire, n_below = Cout // 4, Cout // 8
    cand = (y0 >= 1.0) & (y0 < 2.0)
    graze = []
    one = torch.ones(1)
    for j in range(n_fire + n_below):
        pick = _graze_pick(cand, order, j % 4)
        if pick is None:
            break
        c = pick[0]
        order.remove(c)
        yv = y0[pick[1], c, pick[2], pick[3]].reshape(1)
        bc = (2.0 - yv.double()).float()
        assert float(bc.double() + yv.double()) == 2.0                    # exact: y32 in [1, 2), b in (0, 1] on a finer grid
        kind = "fire" if j < n_fire else "below"
        while kind == "below" and float(lif_h0(fma32(yv, one, bc))) >= 1.0:
            bc = torch.from_numpy(np.nextafter(bc.numpy(), np.float32(-np.inf)))
        a[c], b[c] = 1.0, float(bc)
        graze.append((kind,) + pick)
    coef = torch.pow(torch.tensor(0.8), torch.arange(T - 1, -1, -1).float())
    return SimpleNamespace(geo=geo, kind="spikes", T=T, xs=xs, x=xs[0], w=w, bias=bias, a=a, b=b, v0=v0, coef=coef, Ho=Ho, Wo=Wo,
                           weights="full", e=e, graze=graze)


# ------------------------------------------------------------------------------------------------ the oracle
def conv64(x_nchw, w, bias, geo):
    """torch's fp64 convolution of a batch [N,Cin,H,W] (exact on dyadic inputs, in any order)."""
    Cin, Cout, k, s, p, tr, op, H, W, B = geo
    bd = None if bias is None else bias.double()
    if tr:
        return F.conv_transpose2d(x_nchw.double(), w.double(), bd, s, p, op)
    return F.conv2d(x_nchw.double(), w.double(), bd, s, p)


def conv_fp32(x_seq, w, bias, geo):
    """[T,B,Cin,H,W] -> the convolution + bias in fp64, rounded ONCE to fp32: [T,B,Cout,Ho,Wo] (MODE_RAW)."""
    T, B = x_seq.shape[:2]
    y = conv64(x_seq.flatten(0, 1), w, bias, geo).float()
    return y.view(T, B, *y.shape[1:])


def bn32(y_seq, a, b):
    """fmaf(y, a[c], b[c]) over [..., C, H, W] with one rounding."""
    return fma32(y_seq, a.view(-1, 1, 1), b.view(-1, 1, 1))


def conv_bn_lif(x_seq, w, bias, a, b, v0, geo):
    """The kernels' contract on the host: returns (spikes [T,B,Cout,Ho,Wo], v_last [B,Cout,Ho,Wo], y_fp32 = the convolution output
    before BN).  v0: None (reset state) or a membrane potential tensor."""
    y = conv_fp32(x_seq, w, bias, geo)
    s, v = ref.lif_multi_step(bn32(y, a, b), 0.0 if v0 is None else v0.clone())
    return s, v, y


def conv_bn_lif_bits(frames, w, bias, a, b, v0, geo, T=T16):
    """The same, one step at a time and without the [T, ...] tensors (the rows sized past a grid-stride cap): ``frames`` is a
    callable t -> [B,Cin,H,W] (or one tensor: a time-invariant input).  Returns (bits int32 [B,Cout,Ho,Wo], bit t = spike at step t;
    v_last)."""
    const = torch.is_tensor(frames)
    y = bn32(conv64(frames, w, bias, geo).float(), a, b) if const else None
    v = torch.zeros(1) if v0 is None else v0.clone()
    bits = None
    for t in range(T):
        if not const:
            y = bn32(conv64(frames(t), w, bias, geo).float(), a, b)
        if t == 0 and v0 is None:
            v = torch.zeros_like(y)
        s, v = ref.lif_multi_step(y.unsqueeze(0), v)
        sb = s[0].to(torch.int32) << t
        bits = sb if bits is None else bits | sb
    return bits, v


def threshold_ties(x_bn_seq, v0=None):
    """Neuron-steps whose charged potential h equals the threshold 1.0 EXACTLY (they fire: >=, not >)."""
    v = torch.zeros_like(x_bn_seq[0]) if v0 is None else v0.clone()
    n = 0
    for t in range(x_bn_seq.shape[0]):
        h = v + (x_bn_seq[t] - v) / 2.0
        n += int((h == 1.0).sum())
        v = torch.where(h >= 1.0, torch.zeros_like(h), h)
    return n


def memout64(y_seq, coef):
    """sum_t coef[t] * y[t] in fp64 and sum_t |coef[t] * y[t]| (the scale of the fp32 evaluation's error bound)."""
    c = coef.double().view(-1, 1, 1, 1, 1)
    prod = y_seq.double() * c
    return prod.sum(0), prod.abs().sum(0)


def mean64(y_seq):
    return y_seq.double().sum(0) / y_seq.shape[0], y_seq.double().abs().sum(0) / y_seq.shape[0]


def readout_bound(T, mag):
    """|fp32 evaluation - fp64 value| of sum_t coef[t] * y[t]: T products and T additions (and, for the mean, one division), each
    within one rounding whether or not the compiler contracts them: (T + 2) * 2^-24 * sum_t |coef[t] * y[t]| (first order; the
    +2 covers the division and the second-order terms)."""
    return (T + 2) * 2.0 ** -24 * mag


def collapse32(spikes, coef):
    """sum_t coef[t] * spike[t] added in fp32 in the order t = 0..T-1: [B,Cout,Ho,Wo]."""
    m = torch.zeros_like(spikes[0])
    for t in range(spikes.shape[0]):
        m = m + spikes[t] * coef[t]
    return m


# ------------------------------------------------------------------------------------------------ layouts (plain torch; any device)
def to_ptc(s, chunk=None):
    """[T,B,C,H,W] 0/1 -> u8 PTC [B,H,W,T,C], or CPTC [B,C/chunk,H,W,T,chunk]."""
    T, B, C, H, W = s.shape
    if chunk is None:
        return s.permute(1, 3, 4, 0, 2).contiguous().to(torch.uint8)
    return s.view(T, B, C // chunk, chunk, H, W).permute(1, 2, 4, 5, 0, 3).contiguous().to(torch.uint8)


def from_ptc(p):
    """u8 PTC [B,H,W,T,C] -> fp32 [T,B,C,H,W]."""
    return p.permute(3, 0, 4, 1, 2).contiguous().float()


def bits_to_ptc(bits, T=T16):
    """int32 [B,C,H,W] (bit t = spike at step t) -> u8 PTC [B,H,W,T,C]."""
    sh = torch.arange(T, device=bits.device, dtype=torch.int32).view(1, 1, 1, T, 1)
    return ((bits.permute(0, 2, 3, 1).unsqueeze(3) >> sh) & 1).to(torch.uint8)


def bits_to_packed(bits, rec, T=T16):
    """int32 [B,C,H,W] -> the nibble-packed e2m1 records (1.0 = 0x2; even channel = low nibble) as u8 [B,C/rec,H,W,T,rec/2]:
    rec = 32 "S32", rec = 64 "C4"."""
    B, C, H, W = bits.shape
    ptc = bits_to_ptc(bits, T)                                           # [B,H,W,T,C]
    pr = ptc.view(B, H, W, T, C // rec, rec // 2, 2)
    by = (pr[..., 0] * 2 + pr[..., 1] * 32).to(torch.uint8)               # [B,H,W,T,C/rec,rec/2]
    return by.permute(0, 4, 1, 2, 3, 5).contiguous()


def from_cptc(p):
    """u8 CPTC [B,C/chunk,H,W,T,chunk] -> fp32 [T,B,C,H,W]."""
    B, nch, H, W, T, chunk = p.shape
    return p.permute(4, 0, 1, 5, 2, 3).reshape(T, B, nch * chunk, H, W).contiguous().float()


def packed_to_spikes(q):
    """Nibble-packed records u8 [B,C/rec,H,W,T,rec/2] (S32: rec = 32, C4: rec = 64) -> fp32 [T,B,C,H,W]; a non-zero nibble is a spike,
    and every nibble is 0x0 or 0x2 (checked: a record holds e2m1 codes of 0.0 and 1.0 only)."""
    B, nrec, H, W, T, half = q.shape
    lo, hi = q & 0xF, q >> 4
    assert bool(((lo == 0) | (lo == 2)).all()) and bool(((hi == 0) | (hi == 2)).all()), "a nibble that is neither 0.0 nor 1.0"
    ch = torch.stack([lo, hi], dim=-1).reshape(B, nrec, H, W, T, 2 * half)
    return (ch != 0).permute(4, 0, 1, 5, 2, 3).reshape(T, B, nrec * 2 * half, H, W).contiguous().float()


def to_counts(s):
    """fp32 spikes [T,B,C,H,W] -> the spike-count record u8 [B,C/32,H,W,32] (the A operand of the time-collapsed logits layer)."""
    T, B, C, H, W = s.shape
    return s.sum(0).to(torch.uint8).view(B, C // 32, 32, H, W).permute(0, 1, 3, 4, 2).contiguous()


def from_counts(cnt):
    """u8 [B,C/32,H,W,32] -> fp32 counts [B,C,H,W]."""
    B, nch, H, W, _ = cnt.shape
    return cnt.permute(0, 1, 4, 2, 3).reshape(B, nch * 32, H, W).contiguous().float()


def counts_logits(cnt_bchw, w, bias, geo, T=T16):
    """The time-collapsed logits layer on the host: fp32(sum_t dot + T * bias) / T from the fp64 convolution of the COUNT tensor.
    One rounding (the kernel rounds fma(s, scale, bias * T) once) and an exact division for T = 16.  Also returns the fp64 value."""
    y64 = conv64(cnt_bchw, w, None, geo) + float(T) * bias.double().view(1, -1, 1, 1)
    return y64.float() * (1.0 / T), y64 / T


def spikes_to_bits(s):
    """fp32 [T,B,C,H,W] -> int32 [B,C,H,W]."""
    sh = torch.arange(s.shape[0], dtype=torch.int32).view(-1, 1, 1, 1, 1)
    return (s.to(torch.int32) << sh).sum(0).to(torch.int32)


# ------------------------------------------------------------------------------------------------ case tables
# rows: (Cin, Cout, k, stride, pad, transposed, out_pad, H, W, B); the comment names the kernel or branch a row reaches
GATHER_ROWS = [
    (32, 64, 3, 2, 1, False, 0, 14, 14, 3),      # gather2 <3,2,plain,1 chunk>: encoder conv2's own shape
    (16, 40, 3, 2, 1, False, 0, 9, 13, 2),       # ... 5x7 = 35 positions (ragged group of 4), Cout % 16 = 8 (byte stores), Cin = 16 (half K chunk)
    (64, 16, 1, 1, 0, False, 0, 7, 7, 5),        # gather2 <1,1,plain,2>: encoder conv3 (49 positions: ragged)
    (48, 24, 1, 1, 0, False, 0, 5, 3, 2),        # ... Cin = 48: the second chunk half filled; Cout = 24: ragged second group
    (16, 64, 3, 2, 1, True, 1, 7, 7, 3),         # gather2 <3,2,T,1>: decoder convT1
    (16, 32, 3, 2, 1, True, 0, 5, 6, 2),         # ... out_pad = 0: 9x11 output, sub-pixel classes of unequal size
    (64, 32, 3, 2, 1, True, 1, 14, 14, 2),       # gather2 <3,2,T,2>: decoder convT2
    (48, 8, 3, 2, 1, True, 0, 6, 5, 2),          # ... Cin = 48, Cout = 8 (one ragged group), unequal classes (11x9)
    (32, 1, 3, 1, 1, True, 0, 28, 28, 2),        # gather2 <3,1,T,1>: decoder convT3 (one output channel)
    (32, 3, 3, 1, 1, True, 0, 9, 11, 3),         # ... three output channels, 99 positions
    (32, 32, 3, 1, 1, False, 0, 7, 7, 2),        # generic kernel: 3x3 stride 1
    (96, 16, 3, 2, 1, False, 0, 10, 10, 2),      # generic kernel: three K chunks
    (16, 16, 5, 1, 2, False, 0, 6, 6, 2),        # generic kernel: k = 5
    (32, 32, 3, 2, 0, False, 0, 9, 9, 2),        # generic kernel: pad != k / 2
    (16, 16, 4, 2, 1, True, 0, 5, 5, 3),         # generic kernel: k = 4 transposed (10x10 output, two taps per class and axis)
    (32, 24, 3, 1, 1, False, 0, 5, 5, 2),        # generic kernel: Cout = 24, its own ragged last channel group (byte stores); 25 positions
]
GATHER2_T31 = [r for r in GATHER_ROWS if r[5] and r[3] == 1]          # the <3,1,T,1> rows
MEMOUT_ROWS = GATHER2_T31 + [GATHER_ROWS[11]]                         # ... plus one generic row
DIRECT_PTC_EXTRA = [
    (4, 5, 3, 1, 1, False, 0, 5, 7, 3),          # conv_fused_kernel<PTC>: one u32 of input channels, odd Cout
    (12, 7, 3, 2, 1, True, 1, 4, 5, 2),          # conv_fused_kernel<PTC, transposed>: Cout = 7
]
CONCAT_ROW = (12, 16, 3, 1, 1, False, 0, 5, 4, 2)      # in1 concatenation: C0 = 8 + C1 = 4, both CPTC with chunk 4
CHUNK_OUT_ROW = (8, 8, 3, 1, 1, False, 0, 4, 5, 2)     # chunk_out = 4 at Cout = 8
S32_ROW = (8, 32, 3, 1, 1, False, 0, 3, 5, 1)          # S32 packing: 15 positions x 32 channels = 7.5 waves
C4_ROW = (8, 64, 3, 1, 1, False, 0, 3, 3, 1)           # C4 packing at Cout = 64: 9 positions = 9 waves, one 64-channel record each
COUNTS_ROW = (8, 32, 3, 2, 1, False, 0, 5, 5, 2)       # want_counts
SHORT_T_ROW = (8, 32, 3, 1, 1, False, 0, 3, 5, 2)      # T = 4 (S32 and PTC) and T = 7
PRE_ROW = (8, 12, 3, 1, 1, True, 0, 4, 3, 2)           # want_pre
SEQ_ROWS = [
    (5, 6, 3, 2, 1, False, 0, 7, 6, 2),          # conv_fused_kernel<SEQ>
    (6, 5, 3, 2, 1, True, 1, 4, 3, 2),           # conv_fused_kernel<SEQ, transposed>
]
# (Cin, Cout, k, stride, pad, H, W, B)
TINV_ROWS = [
    (1, 32, 3, 2, 1, 10, 9, 3),                  # staged<3,1> / tinv<3,1>: 75 positions = one full chunk of 64 + 11
    (3, 16, 3, 2, 1, 9, 9, 2),                   # staged<3,3> / tinv<3,3>
    (2, 64, 3, 1, 1, 7, 7, 3),                   # staged<3,2> / tinv<3,2>
    (16, 16, 1, 1, 0, 7, 7, 3),                  # staged<1,16> / tinv<0,0> with carried v (the spike generator)
    (1, 256, 3, 1, 1, 5, 5, 1),                  # one position per block step
    (1, 128, 3, 1, 1, 5, 5, 2),                  # two positions per block step
    (4, 48, 3, 1, 1, 6, 5, 2),                   # 256 % 48 != 0: the generic conv_fused_kernel<TINV>
    (4, 16, 3, 1, 1, 6, 5, 2),                   # Cin = 4: tinv_lif_kernel<0,0> stateless
]
# one row per grid-stride loop, sized just past its cap
TRIP2_PTC_ROW = (4, 64, 1, 1, 0, False, 0, 28, 28, 43)     # conv_fused_kernel: 2 157 568 work items against 8192 x 256 = 2 097 152
TRIP2_TINV_ROW = (1, 16, 3, 2, 1, 28, 28, 700)             # staged: 137 200 positions against 2048 x 64; tinv: against 4096 x 16
# csrc/vae_fp6.hip: (layer, Cin, Cout, transposed, out_pad, H)
VAE_FP6_ROWS = [
    ("enc2", 32, 64, False, 0, 14),              # u8 PTC output
    ("dec1", 16, 64, True, 1, 7),                # S32 output
    ("dec2", 64, 32, True, 1, 14),               # time-collapsed output
]


# ---- the denoiser's 3x3 matrix-core family (stride 1, pad 1, T = 16): (Cin0, Cin1, Cout, H, W, B); full-width weights.
# B = None: computed from the CU count at run time (den_rows(cus)); the host test takes 256 CUs.
DEN_I8_ROWS = [
    (32, 0, 32, 7, 7, 3),          # conv3x3_mfma_kernel<7,7>: the smallest
    (64, 32, 64, 7, 7, 5),         # in1 concatenation, three K chunks (also MODE_MEAN)
    (32, 0, 32, 8, 8, 2),          # <8,8>
    (96, 0, 32, 5, 6, 2),          # <7,7> at 30 positions: 15 tiles, the fourth wave's last tile absent
    (32, 0, 32, 3, 3, 1),          # <7,7> at 9 positions: the last tile half filled
    (32, 0, 64, 7, 7, None),       # B = CUs / 4 + 1: CUs + 4 items on a persistent grid of CUs workgroups, the second trip
]
DEN_I8_MEAN_ROW = DEN_I8_ROWS[1]
DEN_COUNTS_ROWS = [
    (64, 32, 16, 7, 7, 3),         # conv3x3_counts_mfma_kernel (K chunks split over the four waves), with cnt1
    (32, 0, 40, 7, 7, 2),          # through den_pack_weight_i8(pad_cout=True): 48 packed channels
    (32, 0, 48, 7, 7, 105),        # B * HW = 5145 > 5120: conv3x3_counts_mfma_shared_kernel at HW = 49
    (32, 0, 16, 8, 8, 81),         # ... at HW = 64 (5184 rows)
    (32, 0, 16, 6, 7, 123),        # 5166 rows but HW = 42 < 43: the first kernel, one tile per wave (no K split)
]
STEP_TAIL_ROW = (256, 64, 16, 7, 7, 3)      # spk_den_step_tail's logits (cnt5 of 256 channels, cnt1 of 64)
DEN_FP6_ROWS = [
    (64, 0, 64, 7, 7, 3),          # conv3x3_fp6_kernel<6> + conv3x3_fp6_lastpos_kernel
    (128, 0, 64, 9, 6, 2),         # <7>: 54 positions = 27 tiles, two K chunks (the largest even map the launcher's LDS check takes:
                                   # 7x8, 56 positions, asks for 164 KB and is refused -- DEN_FP6_REFUSED)
    (64, 0, 64, 8, 8, 3),          # <4, SPLIT>: two row bands per image
    (64, 0, 64, 10, 6, 2),         # <4, SPLIT> away from 8x8: bands of 5 rows
    (64, 0, 64, 5, 5, 2),          # <6> + last-position kernel with 12 full tiles
    (64, 0, 64, 2, 2, 1),          # <7> with two tiles (4 positions: an even count has no last-position launch)
    (64, 0, 128, 7, 7, 8),         # XCD-aware walk (64 workgroups, gx = 8)
    (64, 0, 128, 7, 7, 7),         # ... 56 workgroups: S % gx != 0, image-major walk
    (64, 0, 64, 7, 7, None),       # B = CUs / 4 + 1: second trip; the last-position grid's last workgroup half filled
]
DEN_FP6_REFUSED = (128, 0, 64, 7, 8, 2)
DEN_FP6V2_ROWS = [
    (32, 0, 32, 7, 7, 2),          # half-image kernel (form 0) / whole-image kernel (form 1); one K chunk: merged tail <7,7,0>
    (96, 0, 64, 7, 7, 5),          # three K chunks (odd), merged tail <7,7,0>
    (64, 0, 64, 7, 7, 64),         # B >= 64 and two K chunks: the LDS-shared last-position tail <7,7,3>
    (64, 0, 64, 7, 7, 63),         # ... one image fewer: the merged tail
    (32, 0, 64, 8, 8, 3),          # row bands <8,8,8,SPLIT>, repair-only tail <8,8,1>
    (512, 0, 256, 7, 7, 5),        # conv5's own shape: 16 K chunks
]
DEN_LISTED_ROW = (64, 0, 64, 7, 7, 6)       # the listed launch (conv3x3_fp6v2_listed_kernel), through ops.active_set(need=...)
DEN_NDYN_ROWS = {"i8": (32, 0, 32, 7, 7, 5), "counts": (64, 32, 16, 7, 7, 5), "fp6": (64, 0, 64, 7, 7, 5), "fp6v2": (32, 0, 32, 7, 7, 5)}
HOST_CUS = 256


def den_row(row, cus=HOST_CUS):
    return row if row[5] is not None else row[:5] + (cus // 4 + 1,)


def den_geo(row, cus=HOST_CUS):
    """(Cin0, Cin1, Cout, H, W, B) -> the ten-field geometry tuple (Cin = Cin0 + Cin1)."""
    C0, C1, Cout, H, W, B = den_row(row, cus)
    return (C0 + C1, Cout, 3, 1, 1, False, 0, H, W, B)


def all_den_rows(cus=HOST_CUS):
    """(family, row) of every denoiser row, B resolved."""
    rows = [("i8", r) for r in DEN_I8_ROWS] + [("counts", r) for r in DEN_COUNTS_ROWS + [STEP_TAIL_ROW]]
    rows += [("fp6", r) for r in DEN_FP6_ROWS] + [("fp6v2", r) for r in DEN_FP6V2_ROWS + [DEN_LISTED_ROW]]
    rows += [(f, r) for f, r in DEN_NDYN_ROWS.items()]
    seen, out = set(), []
    for f, r in rows:
        r = den_row(r, cus)
        if den_geo(r) not in seen:
            seen.add(den_geo(r))
            out.append((f, r))
    return out


# the rows of the 2^-12 tables that run a second time on full-width weights (tests/test_gpu_conv_bn_lif_oracle.py)
GATHER_FULL_ROWS = [GATHER_ROWS[i] for i in (0, 2, 4, 6, 8, 11)]


def full_seed(geo):
    """The seed of a row's full-width case (its own stream: a row of the 2^-12 tables keeps its seed there)."""
    return 7000 + row_seed(geo) % 1000


def vae_fp6_geo(row, B):
    _, Cin, Cout, tr, op, H = row
    return (Cin, Cout, 3, 2, 1, tr, op, H, H, B)


def all_spike_rows():
    """(name, geo, kind, T) of every row of every table (the host test checks the input conditions on each)."""
    rows = [("gather", r, "spikes", 16) for r in GATHER_ROWS]
    rows += [("direct", r, "spikes", 16) for r in DIRECT_PTC_EXTRA + [CONCAT_ROW, CHUNK_OUT_ROW, S32_ROW, C4_ROW, COUNTS_ROW, PRE_ROW]]
    rows += [("short", SHORT_T_ROW, "spikes", 4), ("short", SHORT_T_ROW, "spikes", 7)]
    rows += [("seq", r, "seq", T) for r in SEQ_ROWS for T in (3, 16)]
    rows += [("tinv", tinv_geo(r), "pixels", 16) for r in TINV_ROWS]
    rows += [("vae_fp6", vae_fp6_geo(r, B), "spikes", 16) for r in VAE_FP6_ROWS for B in (1, 5)]
    return rows


# Seeds chosen on the CPU (tests/test_conv_bn_lif_oracle_host.py checks what they were chosen for): the first five give their
# row at least one neuron-step whose charged potential equals the threshold exactly (one row of each gather kernel shape), the last
# two put the two smallest rows' spike rate inside the band.
ROW_SEEDS = {
    (GATHER_ROWS[0], 16): 25, (GATHER_ROWS[4], 16): 9, (GATHER_ROWS[6], 16): 3, (GATHER_ROWS[10], 16): 20, (GATHER_ROWS[14], 16): 38,
    (DIRECT_PTC_EXTRA[0], 16): 2, (DIRECT_PTC_EXTRA[1], 16): 3,
}
TIE_ROWS = [GATHER_ROWS[i] for i in (0, 4, 6, 10, 14)]


def row_seed(geo, T=16):
    """The seed of a row's case: a function of the row alone, so that every test of a row sees the same inputs."""
    if (geo, T) in ROW_SEEDS:
        return ROW_SEEDS[(geo, T)]
    return 1000 + (sum((i + 1) * int(v) for i, v in enumerate(geo)) * 31 + T) % 100000
