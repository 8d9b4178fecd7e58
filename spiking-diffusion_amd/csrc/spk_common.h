// Shared helpers for the libspkdiff HIP kernels (gfx950 / MI355X only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>

#define SPK_OK 0              // the negative return codes SPK_ERR_* and the spike dtypes SPK_SPIKE_*: include/spkdiff.h

#define SPK_MAX_T 16          // time steps kept in registers by the fused kernels

#define SPK_LAUNCH_CHECK()                                   \
  do {                                                       \
    hipError_t e__ = hipGetLastError();                      \
    if (e__ != hipSuccess) return (int)e__;                  \
  } while (0)

static inline int spk_blocks(long long n, int threads) { return (int)((n + threads - 1) / threads); }
// Blocks of 256 threads of a grid-stride launch over `work_items`: ceil(work_items / 256), at least 1, at most `cap` (the loop
// covers the rest).  The cap is the call site's: how many blocks keep its kernel's memory pipeline full.
static inline int spk_grid(long long work_items, int cap) {
  const long long g = (work_items + 255) / 256;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// Images a kernel processes: the optional device-side count, at most B.  Buffers and strides stay sized by B.
__device__ __forceinline__ int spk_batch_count(const int* n_dyn, int B) { return n_dyn ? (*n_dyn < B ? *n_dyn : B) : B; }

// One LIF step, exactly the arithmetic of
// SJ/activation_based/neuron.py:799-811 with v_reset as a parameter:
//   v = v + (x - (v - v_reset)) / tau ; s = v >= v_th ; v = v_reset * s + (1 - s) * v
// DIV=false multiplies by inv_tau instead of dividing: bit-identical when tau is a power of two
// (the default tau = 2); DIV=true performs the correctly rounded fp32 division for any other tau.
template <bool DIV>
__device__ __forceinline__ bool spk_lif_step(float& v, float x, float tau, float inv_tau, float v_th, float v_reset) {
  float d = x - (v - v_reset);
  float h = v + (DIV ? d / tau : d * inv_tau);
  bool s = h >= v_th;
  // v_reset*1 + 0*h  |  v_reset*0 + 1*h : the reference's arithmetic maps -0.0 to +0.0 via the add
  v = s ? (v_reset + 0.0f * h) : (v_reset * 0.0f + h);
  return s;
}

// Default neuron of the models (tau 2, v_th 1, v_reset 0: R/snn_model/vae_model.py:37,112,...), lean form for the
// fused epilogues:  h = v + (x - v)/2 ; s = h >= 1 ; v = s ? 0 : h.  Same spikes and the same v as the reference's
// arithmetic except that a zero membrane potential may keep its sign (-0.0 instead of +0.0), which no later
// operation can observe (x - (-0) == x - (+0), and torch.equal(-0., +0.) is True), and that an INFINITE h resets to 0 here
// and to NaN there ((1 - s) * h): pre-activations are finite.
__device__ __forceinline__ bool spk_lif_step_default(float& v, float x) {
  const float h = v + (x - v) * 0.5f;
  const bool s = h >= 1.0f;
  v = s ? 0.0f : h;
  return s;
}

// The default neuron under a CONSTANT input x from v = 0 (the layers whose input is the same frame at every step: encoder
// conv1, the spike generator, the denoiser's conv1).  After a spike the state is v = 0 again, so the train is periodic with
// the step p(x) of the first spike, and p is a step function of x: p(x) <= k  <=>  x >= theta_k.  The sixteen thresholds
// below are those of the fp32 recurrence above (h = v + (x - v) * 0.5f, three roundings), found by running it on EVERY float
// in [0.5, 4) (tests/test_cabi_and_host.py repeats that, 25 M values; x <= 1 and NaN never fire, x >= 2 fires every step):
// theta_k is the smallest float whose first spike comes at step k or earlier (~ 1 / (1 - 2^-k)).  Sixteen LIF steps become
// one table look-up: with t = x - 1 (exact in [1, 2]) and k = -ilogb(t), theta_{k+1} - 1 <= 2^-k <= t, so p is k or k + 1.
#define SPK_LIF_CONST_TH_BITS {0x40000000u, 0x3faaaaabu, 0x3f924925u, 0x3f888889u, 0x3f842108u, 0x3f820821u, 0x3f810204u, \
                               0x3f808081u, 0x3f804020u, 0x3f802008u, 0x3f801002u, 0x3f800801u, 0x3f800400u, 0x3f800200u, \
                               0x3f800100u, 0x3f800080u}
// spike bits (bit t = step t) of a train with period p = 1 .. 16; p = 17: no spike within sixteen steps; entry 0 unused
#define SPK_LIF_CONST_PATTERNS {0u, 0xffffu, 0xaaaau, 0x4924u, 0x8888u, 0x4210u, 0x0820u, 0x2040u, 0x8080u, 0x0100u, 0x0200u, \
                                0x0400u, 0x0800u, 0x1000u, 0x2000u, 0x4000u, 0x8000u, 0u}
// s_th[k - 1] = theta_k (16 floats), s_pat[p] (18 words): LDS copies of the two tables
__device__ __forceinline__ unsigned spk_lif_const_input_bits16(float x, const float* s_th, const unsigned* s_pat) {
  const float t = x - 1.0f;
  int k = 1 - __builtin_amdgcn_frexp_expf(t);              // t = m * 2^e, m in [0.5, 1): ilogb(t) = e - 1
  k = k < 1 ? 1 : (k > 16 ? 16 : k);
  int p = x >= s_th[k - 1] ? k : k + 1;
  p = x >= 2.0f ? 1 : p;
  p = x > 1.0f ? p : 17;                                    // (also NaN)
  return s_pat[p];
}

// ------------------------------------------------------------------------------------------------ surrogate-gradient training
// One step of the training forward (the autograd-recorded LIF of the reference trainers):
//   h = v + (x - (v - v_reset)) / tau ; s = h - v_th >= 0 ; v = (1 - s) h + s v_reset.   Returns {h, s}, s = 0 or 1.
struct SpkLifHS { float h, s; };
__device__ __forceinline__ SpkLifHS spk_lif_train_step(float& v, float x, float tau, float v_th, float v_reset) {
  const float h = v + (x - (v - v_reset)) / tau;
  const float s = (h - v_th >= 0.0f) ? 1.0f : 0.0f;
  v = (1.0f - s) * h + s * v_reset;
  return {h, s};
}

// One reverse step of that forward under the ATan surrogate (g(x) = alpha / 2 / (1 + (pi / 2 alpha x)^2) for ds/dh).
// G: gradient of the loss w.r.t. the potential v after the step (updated to the one before it); grad_s: w.r.t. the spike;
// h: the recorded charged potential.  DETACH drops the reset's path through s.  Returns the gradient w.r.t. the input x.
// inv_tau = 1 / tau, carry = 1 - inv_tau.
template <bool DETACH>
__device__ __forceinline__ float spk_atan_bptt_step(float& G, float grad_s, float h, float v_th, float v_reset, float alpha,
                                                    float inv_tau, float carry) {
  const float over = h - v_th;
  const float s = over >= 0.0f ? 1.0f : 0.0f;
  const float ax = 1.57079632679489661923f * alpha * over;
  const float g_s = alpha / 2.0f / (1.0f + ax * ax);
  float dv_dh = 1.0f - s;
  if (!DETACH) dv_dh = (v_reset - h) * g_s + dv_dh;
  const float gh = G * dv_dh + grad_s * g_s;
  const float gx = gh * inv_tau;
  G = gh * carry;
  return gx;
}

// ------------------------------------------------------------------------------------------------ spike records
// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>).  The K loop must be straight-line
// code with constant accumulator indices (a runtime index would send the accumulators through scratch); this does not
// depend on the unroller's size heuristics.
template <typename F, int... S>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, S...>) {
  (f(std::integral_constant<int, S>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

// 16x16 bit-matrix transpose inside every 16-lane row (lane = row, bit = column) with DPP lane exchanges:
// lane^8 = row_mirror o row_half_mirror, lane^4 = row_half_mirror o quad-reverse, lane^2 / lane^1 = quad_perm.
// Round s (8, 4, 2, 1) swaps the off-diagonal s-bit blocks with lane ^ s.  Both lane parities run the SAME two instructions on
// per-lane constants -- the partner's word rotated by s towards the block it lands in (v_alignbit: right by s for the lanes with
// bit s set, right by 32 - s = left by s for the others) and merged under the keep mask (v_bfi) -- instead of a select between
// two shift-and-mask expressions, which hipcc compiled as two exec-masked branches per round (45 vector + 24 scalar
// instructions per transpose; now 14).  Bits 16..31 of the result are garbage (rotated-out blocks): callers use the low half.
__device__ __forceinline__ unsigned spk_transpose16_rows(unsigned x, int lane) {
  unsigned y;
  // (opaque copy of the lane id: the three per-lane constants of a round are recomputed here -- three vector instructions --
  //  instead of being hoisted out of the caller's loops, where eight of them stayed live across the K loop: 256 registers + spills)
  int ln = lane;
  asm volatile("" : "+v"(ln));
#define SPK_TR16_ROUND(S, LOW)                                                                       \
  do {                                                                                               \
    const unsigned sh = (unsigned)ln & (unsigned)(S);            /* 0 or S */                         \
    const unsigned keep = (unsigned)(LOW) << sh;                                                     \
    const unsigned amt = (32u - (unsigned)(S)) + 2u * sh;        /* 32 - S, or 32 + S = S (mod 32) */ \
    const unsigned yr = __builtin_amdgcn_alignbit(y, y, amt);                                        \
    x = (x & keep) | (yr & ~keep);                                                                   \
  } while (0)
  y = __builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp(x, 0x140, 0xF, 0xF, true), 0x141, 0xF, 0xF, true);
  SPK_TR16_ROUND(8, 0x00FFu);
  y = __builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp(x, 0x141, 0xF, 0xF, true), 0x1B, 0xF, 0xF, true);
  SPK_TR16_ROUND(4, 0x0F0Fu);
  y = __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true);
  SPK_TR16_ROUND(2, 0x3333u);
  y = __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true);
  SPK_TR16_ROUND(1, 0x5555u);
#undef SPK_TR16_ROUND
  return x;
}

// uint32 sum over the 64 lanes of a fully active wave with the same DPP lane exchanges (integers: any order gives the same sum): a
// butterfly inside each row of 16 lanes (lane ^ 1, lane ^ 2, then the mirror of each half row and of each row: every lane of a row
// ends with the row's sum), then the four rows' sums through the scalar unit.  The nucleus truncation of the sampler makes 32 such
// sums in a row per drawn token (truncate_top_p, psample_common.h): as six __shfl_xor steps each was six dependent ds_bpermute round
// trips, and top_p = 0.9 cost 2.1 - 2.3 % of the B = 256 dense sample where this form costs 0.8 - 1.2 %.
__device__ __forceinline__ unsigned spk_wave_sum_u32(unsigned v) {
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);    // quad_perm [1, 0, 3, 2]
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2, 3, 0, 1]
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);   // row_half_mirror
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);   // row_mirror
  return (unsigned)__builtin_amdgcn_readlane((int)v, 0) + (unsigned)__builtin_amdgcn_readlane((int)v, 16) +
         (unsigned)__builtin_amdgcn_readlane((int)v, 32) + (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}

// e2m1 spike records: 16 channels of one (position, step) as 16 nibbles = 8 bytes, channel k in nibble k, a spike as the
// e2m1 code of 1.0 (0x2).  spk_spread8: bit k -> nibble k of eight channel bits.
__device__ __forceinline__ unsigned spk_spread8(unsigned x) {
  x = (x | (x << 12)) & 0x000f000fu;
  x = (x | (x << 6)) & 0x03030303u;
  x = (x | (x << 3)) & 0x11111111u;
  return x << 1;
}
// the record of a row of spk_transpose16_rows (the 16 channel bits of one step in bits 0..15)
__device__ __forceinline__ uint2 spk_e2m1_record(unsigned bits16) {
  uint2 o;
  o.x = spk_spread8(bits16 & 0xffu);
  o.y = spk_spread8((bits16 >> 8) & 0xffu);
  return o;
}
// byte spike records ("PTC" / "CPTC" u8): the same 16 channels as 16 bytes of 0 or 1, channel k in byte k.
// spk_spread4_u8: bit k -> byte k of four channel bits (the multiply puts a copy of the nibble at bit offsets 0, 7, 14, 21).
constexpr unsigned spk_spread4_u8(unsigned nib) { return ((nib & 0xfu) * 0x00204081u) & 0x01010101u; }
static_assert(spk_spread4_u8(0x0u) == 0x00000000u && spk_spread4_u8(0xFu) == 0x01010101u, "byte spike record");
static_assert(spk_spread4_u8(0xAu) == 0x01000100u && spk_spread4_u8(0x1u) == 0x00000001u, "byte spike record");
static_assert(spk_spread4_u8(0x38u) == 0x01000000u, "byte spike record: only the low nibble counts");
// the record of a row of spk_transpose16_rows
__device__ __forceinline__ uint4 spk_u8_record(unsigned bits16) {
  uint4 o;
  o.x = spk_spread4_u8(bits16);
  o.y = spk_spread4_u8(bits16 >> 4);
  o.z = spk_spread4_u8(bits16 >> 8);
  o.w = spk_spread4_u8(bits16 >> 12);
  return o;
}
// four fp32 spikes (zero / nonzero) of consecutive channels -> their 16-bit quarter of a record
__device__ __forceinline__ unsigned spk_e2m1_nibbles4(float a, float b, float c, float d) {
  return (a != 0.f ? 0x2u : 0u) | (b != 0.f ? 0x20u : 0u) | (c != 0.f ? 0x200u : 0u) | (d != 0.f ? 0x2000u : 0u);
}

// ------------------------------------------------------------------------------------------------ weight digits
// The MFMA layers quantise a conv weight channel exactly: w -> q = rint(w 2^sh), split into balanced digits (int8 planes:
// base 256; fp6 planes: radix 32, each digit an e2m3 sign-magnitude code), and the digit products are summed exactly.
//
// Maximum of m over the 256 threads of the block (smax: 256 floats of the caller's LDS), returned as e with max < 2^e
// (0 for an all-zero channel).  The caller's shift is sh = 30 - e (int8) or 29 - e (fp6): |w| 2^sh < 2^30 or 2^29.
__device__ __forceinline__ int spk_channel_exponent(float* smax, float m) {
  smax[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + s]);
    __syncthreads();
  }
  m = smax[0];
  int e = 0;
  if (m > 0.f) frexpf(m, &e);                 // m = f * 2^e, f in [0.5, 1)  ->  m < 2^e
  return e;
}

// q = sum_d dg[d] 2^(BITS (N - 1 - d)), most significant digit first: dg[1 .. N-1] in [-2^(BITS-1), 2^(BITS-1)), dg[0] the
// rest (|q| < 2^30 for base 256 x 4 and |q| < 2^29 for radix 32 x 6 keep it in [-2^(BITS-1), 2^(BITS-1)]).
template <int BITS, int N>
__device__ __forceinline__ void spk_balanced_digits(long long q, int (&dg)[N]) {
#pragma unroll
  for (int d = N - 1; d >= 1; --d) {
    const int r = (int)(((q + (1 << (BITS - 1))) & ((1 << BITS) - 1)) - (1 << (BITS - 1)));
    dg[d] = r;
    q = (q - r) >> BITS;
  }
  dg[0] = (int)q;
}

// a radix-32 digit in [-16, 16] as its 6-bit e2m3 code: sign bit 0x20 over the magnitude's bits (read as e2m3: |d| / 8, exact)
__device__ __forceinline__ unsigned spk_e2m3_code(int d) { return (d < 0 ? 0x20u : 0u) | (unsigned)(d < 0 ? -d : d); }
