// What the two CERTIFIED kernels share (den_mfma_fp6v2.hip: the denoiser's conv2..5; vae_fp6.hip: the VQ-VAE's stride-2 layers): both
// multiply four of the six radix-32 weight digits on the matrix cores, bound the error of every spike decision, FLAG the neurons that
// come within the bound of the threshold in a workspace, and recompute exactly those in a tail launch.  Here, once: the workspace and
// its protocol (flag, hand-over, scan), the pieces of the exact repair, and the weight tile format of the pack kernels.  What stays in
// the two files is what differs: geometry, the repair's work decomposition (a workgroup per flagged neuron in fp6v2, a wave in
// vae_fp6) and which (tap, digit, chunk) a weight tile holds.
#pragma once
#include "den_common.h"
#include <math.h>

typedef int v6i __attribute__((ext_vector_type(6)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int T16 = 16;
constexpr int POSB = 256;                    // bytes of an S32 spike record group: one position, 32 channels, 16 steps x 16 B
constexpr int WT = 64 * 24;                  // one B tile: 64 lanes x 32 six-bit codes
constexpr float CERT_4EPS = 4.0f * 2.38418579e-07f;   // (den_mfma_fp6v2.hip, "Certification")

// ------------------------------------------------------------------------------------------------ the flag workspace
// u32 words of a layer of n neurons: ws[0] the LIVE count of flagged neurons (zero between launches), ws[1] the count PUBLISHED for
// the tail launch, ws[2 .. 2 + FLAG_CAP) their ids, then the overflow BITMAP (one bit per neuron of the layer), then the TICKET of the
// hand-over.  The id list holds the first `flag_cap` <= FLAG_CAP flagged neurons of a launch (a per-call argument: the parity suite
// runs the overflow path with 64 and 0); every further one sets its bit in the bitmap, which the tail launch scans and clears.  The
// LAYOUT never depends on flag_cap.
constexpr unsigned FLAG_CAP = 1u << 20;
static inline long long spk_cert_bitmap_words(long long n) { return (n + 31) / 32; }
static inline long long spk_cert_ticket_idx(long long n) { return 2 + (long long)FLAG_CAP + spk_cert_bitmap_words(n); }
static inline long long spk_cert_flag_words(long long n) { return spk_cert_ticket_idx(n) + 1; }
// What the kernels get of it (a member `ws` of their argument structs).  flag_cap argument of a call: id-list entries used (< 0, or
// more than there are: all)
struct CertWs { unsigned* flags; unsigned flag_cap; long long ticket_idx; };
static inline CertWs spk_cert_ws(unsigned* flag_words, int flag_cap, long long n) {
  return CertWs{flag_words, flag_cap < 0 || (unsigned)flag_cap > FLAG_CAP ? FLAG_CAP : (unsigned)flag_cap, spk_cert_ticket_idx(n)};
}

__device__ __forceinline__ unsigned* spk_cert_bitmap(const CertWs& ws) { return ws.flags + 2 + FLAG_CAP; }

// main launch: neuron n came within its bound of the threshold (ws[0] also serves statistics and tests).  flagged: for the caller
// that has n at hand whether flagged or not
__device__ __forceinline__ void spk_cert_flag(const CertWs& ws, long long n, bool flagged = true) {
  if (flagged) {
    const unsigned idx = atomicAdd(ws.flags, 1u);
    if (idx < ws.flag_cap) ws.flags[2 + idx] = (unsigned)n;
    else atomicOr(spk_cert_bitmap(ws) + (n >> 5), 1u << (n & 31));
  }
}

// Hand-over to the tail launch, by ONE thread of every workgroup of the main launch behind a __syncthreads() of the caller's: the
// workgroup that finishes last publishes the count and re-arms the live counter for the next main launch.  The workgroups finish at
// different times, so the ticket costs nothing (a ticket in the tail launch, whose workgroups all arrive at once, cost 16 us, a
// separate reset launch 5).  No fence: every atomicAdd on the counter has RETURNED before its wave reaches the barrier, the count is
// read back with an atomic, and list entries are plain stores read by the next launch (a __threadfence cost 4.5 us per launch).
__device__ __forceinline__ void spk_cert_handover(const CertWs& ws) {
  if (atomicAdd(ws.flags + ws.ticket_idx, 1u) == gridDim.x - 1) {
    ws.flags[1] = atomicAdd(ws.flags, 0u);
    ws.flags[0] = 0u;
    ws.flags[ws.ticket_idx] = 0u;
  }
}

// Tail launch: fix(id) for every flagged neuron -- the listed ones, then (only if more than flag_cap were flagged) the set bits of the
// bitmap, cleared as it goes.  Unit `unit` of `n_units` (I: the caller's index type) is a WORKGROUP (WG: every thread calls with the
// same arguments; it takes a contiguous share of the n_words bitmap words, and all threads have read a word before `clearer` clears
// it) or a WAVE striding over the words.  clearer: the one thread of the unit that clears.
template <bool WG, class I, class Fix>
__device__ __forceinline__ void spk_cert_scan(const CertWs& ws, unsigned count, I unit, I n_units, long long n_words, bool clearer,
                                              Fix&& fix) {
  const unsigned nlist = count < ws.flag_cap ? count : ws.flag_cap;
  for (I e = unit; e < nlist; e += n_units) fix((long long)ws.flags[2 + e]);
  if (count > ws.flag_cap) {
    unsigned* bm = spk_cert_bitmap(ws);
    long long w0 = unit, w1 = n_words, step = n_units;
    if (WG) {
      const long long per = (n_words + n_units - 1) / n_units;
      w0 = (long long)unit * per;
      w1 = w0 + per < n_words ? w0 + per : n_words;
      step = 1;
    }
    for (long long wi = w0; wi < w1; wi += step) {
      unsigned wd = bm[wi];
      if (WG) __syncthreads();
      if (wd && clearer) bm[wi] = 0u;
      while (wd) {
        const int bit = __ffs((int)wd) - 1;
        wd &= wd - 1;
        fix(wi * 32 + bit);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ the exact repair
// part += the quantised weights (int32, eight consecutive input channels) under the set nibbles of one word of a spike record
__device__ __forceinline__ void spk_cert_add_active8(long long& part, unsigned nib, const int4& q0, const int4& q1) {
  part += (nib & 0x0000000fu) ? (long long)q0.x : 0ll;
  part += (nib & 0x000000f0u) ? (long long)q0.y : 0ll;
  part += (nib & 0x00000f00u) ? (long long)q0.z : 0ll;
  part += (nib & 0x0000f000u) ? (long long)q0.w : 0ll;
  part += (nib & 0x000f0000u) ? (long long)q1.x : 0ll;
  part += (nib & 0x00f00000u) ? (long long)q1.y : 0ll;
  part += (nib & 0x0f000000u) ? (long long)q1.z : 0ll;
  part += (nib & 0xf0000000u) ? (long long)q1.w : 0ll;
}
__device__ __forceinline__ long long spk_join64(int lo, int hi) {
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// the 64-bit value of lane `src`
__device__ __forceinline__ long long spk_shfl64(long long v, int src) {
  return spk_join64(__shfl((int)(unsigned)(v & 0xffffffffll), src), __shfl((int)(v >> 32), src));
}
// lanes l, l + 16, l + 32, l + 48 of a wave hold partial sums of the same time step: afterwards every one of them holds their sum
__device__ __forceinline__ long long spk_cert_sum_quarters(long long part) {
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1)
    part += spk_join64(__shfl_xor((int)(unsigned)(part & 0xffffffffll), off), __shfl_xor((int)(part >> 32), off));
  return part;
}
// the exact pre-activation: fp64 recombination of the exact integer sum, the ONE rounding to fp32
__device__ __forceinline__ float exact_preact(double s, double sc, double bi) { return (float)fma(s, sc, bi); }
// rewrite channel co's nibble in the 16-byte S32 record (one position, one step) of its channel group
__device__ __forceinline__ void spk_cert_patch_nibble(uint8_t* rec, int co, bool spike) {
  const int byte = (co & 31) >> 1;
  unsigned* wp = reinterpret_cast<unsigned*>(rec + (byte & ~3));
  const unsigned shw = 8u * (byte & 3) + 4u * (co & 1);
  atomicAnd(wp, ~(0xFu << shw));
  if (spike) atomicOr(wp, 0x2u << shw);
}

// ------------------------------------------------------------------------------------------------ weight packing
// A channel's weights as 29-bit fixed point: q = rint(w 2^sh), sh = 29 - spk_channel_exponent: |q| < 2^29 <= 16.5 * 32^5
__device__ __forceinline__ double spk_cert_quantise(float w, int sh) { return rint(ldexp((double)w, sh)); }
__device__ __forceinline__ void spk_cert_scale_bias(double* scale, double* bias_d, const float* bias, int co, int sh) {
  scale[co] = ldexp(1.0, -sh);
  bias_d[co] = bias ? (double)bias[co] : 0.0;
}
// One B fragment of a tile: digit `digit` (0 = most significant of six balanced radix-32 digits) of the 32 quantised weights
// q(0 .. 31) (the fragment's input channels; all zero unless live) as 32 six-bit e2m3 codes, little-endian, stored as lane ln's
// (= K half * 32 + output channel within the group of 32) 16 bytes in the ds_read_b128 part of the tile and 8 in its ds_read_b64 part.
template <class Q>
__device__ __forceinline__ void spk_cert_emit_fragment(uint8_t* tile, int ln, int digit, bool live, Q&& q) {
  unsigned bits[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 32 && live; ++k) {
    int dg[6];
    spk_balanced_digits<5>(q(k), dg);
    int d = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) d = (p == digit) ? dg[p] : d;
    const unsigned code = spk_e2m3_code(d);
    const int bit = 6 * k, wd = bit >> 5, sft = bit & 31;
#pragma unroll
    for (int q2 = 0; q2 < 6; ++q2) {         // static register indexing
      if (q2 == wd) bits[q2] |= code << sft;
      if (q2 == wd + 1 && sft > 26) bits[q2] |= code >> (32 - sft);
    }
  }
  unsigned* d16 = reinterpret_cast<unsigned*>(tile + ln * 16);
  unsigned* d8 = reinterpret_cast<unsigned*>(tile + 1024 + ln * 8);
  d16[0] = bits[0]; d16[1] = bits[1]; d16[2] = bits[2]; d16[3] = bits[3];
  d8[0] = bits[4]; d8[1] = bits[5];
}
