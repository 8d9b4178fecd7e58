// The spike-input layers of the spiking VQ-VAE on the block-scaled fp6 x fp4 MFMA (R/snn_model/vae_model.py:115-118 Encoder
// conv2, :139-150 Decoder convT1 / convT2), for calls that start from the reset state.  Same arithmetic
// contract as den_mfma_fp6v2.hip: 29-bit per-channel fixed-point weights as radix-32 digits, adjacent digits sharing an fp32
// accumulator through the per-block scales, every spike decision certified against an error bound, the few neurons that come
// within the bound of the threshold recomputed exactly (all six digits, 64-bit sums, fp64 recombination, one rounding) by a
// tail launch (the flag workspace and its protocol, the pieces of the exact repair and the weight tile format: cert_common.h, shared
// with that kernel).  Unflagged neurons provably emit the exact path's spikes; the result is the one spk_conv_mfma_fused_fwd (int8
// gather kernel) produces for the same layer.  Round 4: FOUR digits on the matrix cores (two accumulators per tile,
// 4 / 2 instead of 5 / 3 MFMAs and weight-tile reads per tap and chunk) behind the COUNTED bound of den_mfma_fp6v2.hip -- the
// active inputs of every input record are popcounted once per item, then per class and output position the maximum over the
// steps of the sum over the class's taps multiplies the per-input bound of the two dropped digits.  Measured at B = 1024 (same
// box, alternating): convT2 0.246-0.249 -> 0.222-0.228 ms, conv2 (nine taps; no longer spills) 0.118-0.127 -> 0.075-0.084 ms,
// encode -> decode 1.41-1.43 -> 1.57-1.58 M images/s; 0 mismatches against the int8 gather kernel over 7.2e8 neuron-steps.
//
// What differs from the denoiser kernel is the geometry: K is small (16 .. 64 input channels = 1 or 2 chunks of 32) and the
// spatial extent large, so ALL weight tiles of a 32-channel output group stay in LDS for the whole launch (9 taps x [pair 01,
// pair 23] per chunk: 27 / 54 KB; the fifth-digit tiles of the packed format stay in memory) next to the input rows of one item.
//   GEO 0  ConvTranspose2d(k3, s2, p1, op1): four sub-pixel classes (oy % 2, ox % 2) with 1 / 2 / 2 / 4 contributing taps; the
//          rows of a 32-row MFMA tile are two consecutive positions of ONE class x 16 time steps, so a tile's tap list is
//          compile-time.  Item = an image (or its upper / lower half) : class rows + one more input row, zero column on the right.
//   GEO 1  Conv2d(k3, s2, p1): rows = two consecutive OUTPUT positions; item = an image with a zero row above and a zero column left.
// The eight waves of a workgroup (two per SIMD) take passes of two tiles -- a weight tile read from LDS serves both -- and the
// pass list of an item (class-major) is dealt round-robin, so every wave gets a mix of cheap and expensive classes.  These
// layers are bound by the vector work of the LIF scan (16 steps x ~11 instructions per neuron), not by the matrix pipe or memory.
//
// Spikes in: "S32" [B][Cin/32 (rounded up)][H*W][16][16 B] (fp4 nibbles; channels beyond Cin must be zero).  Out: S32, plain u8
// PTC [B][Ho*Wo][16][Cout], or -- for the layer in front of the linear read-out -- the time-collapsed tensor
// m = sum_t coef[t] * s_t (fp32 [B][Ho*Wo][Cout], spk_readout_collapsed_fwd): the spike frames are then never stored.
#include "cert_common.h"
#include "../../include/spkdiff.h"
#include <type_traits>
#include <utility>

namespace {

__host__ __device__ constexpr int tiles_per_tap(int nch) { return nch == 2 ? 5 : 3; }
// tile (tap, j): NCH = 2: j = 0..3: chunk j / 2, digit pair j % 2; j = 4: fifth digit, K half 0 = chunk 0, half 1 = chunk 1.
//                NCH = 1: j = 0, 1: digit pair j; j = 2: fifth digit in K half 0 (half 1 zero).

struct TArgs {
  const uint8_t* in;                         // S32 [B][NCH][H*W][16][16 B]
  const uint8_t* wq; const double* scale; const double* bias; const float* bn_a; const float* bn_b; const float* coef;
  void* out;
  CertWs ws;                                 // the flag workspace (cert_common.h)
  const int* qtab;                           // int32 [Cout][9][Cin]
  int B, Cout, Cin;
};

constexpr int SPK_VT_NWV = 16;          // waves per workgroup.  Round 4: SIXTEEN (four per SIMD) with one tile per pass: the four-digit form needs ~100
                                        // registers at one tile per pass, four waves issue vector instructions at 2.0 instead of 3.1 cycles each
                                        // (tools/coexec_probe.hip) and overlap one another's multiply phases: encode -> decode at B = 1024
                                        // 1.577 -> 1.632-1.640 M images/s, convT2 0.225 -> 0.213 ms (same box; 12 waves: 1.61 M).  Round 3 (five
                                        // digits): 16 waves x 1 tile 253-255 us against 259-267 for convT2 and spills in the nine-tap layer
constexpr int SPK_VT_TPP = 1;           // row tiles per pass (a weight tile read from LDS serves all of them)
// FOUR digits on the matrix cores (two accumulators per tile, 4 / 2 MFMAs and weight-tile reads per tap) behind the COUNTED certification
// bound of den_mfma_fp6v2.hip: the two dropped digits move a pre-activation by at most 528 units of 2^-s per ACTIVE input, and the active
// inputs of every output row are counted once per item (popcounts of the input records, then per class and position the maximum over the
// steps of the sum over the class's taps).  Spike-bit outputs: the sixteen bits of a lane shifted in from the sign of h - 1 (as in
// den_mfma_fp6v2.hip).  The weight fragments of a class's leading SPK_VT_NHOLD taps stay in registers over the wave's passes of that class
// within an item: the multiply phase of these layers is bound by LDS reads, 1.5 KB of weight fragments per MFMA
// (profiles/r4_ab_kernel_variants.txt (11)).
// (Measured and dropped: software-pipelined LDS reads in the multiply phase, 264-267 against 267 us; a 512-2048-cycle s_sleep stagger of
//  waves 4..7, 270-275 against 266-267 us on convT2.)
constexpr int SPK_VT_NHOLD = 1;         // held taps per class.  All four taps of the four-tap class need 96 registers with two chunks: twelve waves
                                        // (168 registers each) hold three, sixteen (128) hold one

template <int GEO, int H, int W>
struct Geo {
  static constexpr int Ho = GEO == 0 ? 2 * H : H / 2, Wo = GEO == 0 ? 2 * W : W / 2;
  static constexpr int KMAX = GEO == 0 ? 4 : 9;                       // taps that can reach one output
};

// the taps that reach an output of sub-pixel class CLS (transposed convolution: 1 / 2 / 2 / 4 of nine; plain stride 2: all)
template <int GEO, int CLS>
__host__ __device__ constexpr bool tap_is_on(int tap) {
  const int ky = tap / 3, kx = tap % 3, py = CLS >> 1, px = CLS & 1;
  return GEO == 1 || ((py == 0 ? ky == 1 : ky != 1) && (px == 0 ? kx == 1 : kx != 1));
}
template <int GEO, int CLS>
__host__ __device__ constexpr int n_on_taps() {
  int n = 0;
  for (int t = 0; t < 9; ++t) n += tap_is_on<GEO, CLS>(t) ? 1 : 0;
  return n;
}
template <int GEO, int CLS>
__host__ __device__ constexpr int on_tap(int k) {
  for (int t = 0; t < 9; ++t)
    if (tap_is_on<GEO, CLS>(t) && k-- == 0) return t;
  return 0;
}

// The passes of an item are HANDED OUT (an LDS counter, class-major order kept) instead of dealt round-robin: of the four waves of a SIMD
// the oldest issues its scan's vector instructions first -- waves 0-3 scan a pass in 1 280 cycles, waves 12-15 in 2 410 -- so with equal
// shares the first four waited 31 % of the launch at the item's end barrier (mean over the waves: 19 %).
// (A wave recomputing the neurons IT flags right behind the tile's stores, instead of the id list + repair launch, measured slower:
//  convT2 198.8 -> 209.8, conv2 65.3 -> 79.7 us, profiles/r6_ab_kernel_variants.txt (3).)
template <int GEO, int H, int W, int NCH, int OUT, int SPLIT, bool DB>
__global__ __launch_bounds__(SPK_VT_NWV * 64, 1) void vae_fp6_kernel(TArgs a) {
  constexpr int TPT = tiles_per_tap(NCH), W_BYTES = 9 * TPT * WT;
  constexpr int TPL = TPT - 1;                              // tiles per tap kept in LDS (the fifth-digit tile stays in memory)
  constexpr int WL_BYTES = 9 * TPL * WT;
  constexpr int RQ = GEO == 0 ? H / SPLIT : H / 2;          // rows of positions per item (class rows / output rows)
  constexpr int CW = GEO == 0 ? W : W / 2;                  // positions per row
  constexpr int NPOS = RQ * CW, NTC = (NPOS + 1) / 2, TPP = SPK_VT_TPP, NPASS = (NTC + TPP - 1) / TPP,
                NCLS = GEO == 0 ? 4 : 1;
  constexpr int SROWS = GEO == 0 ? RQ + 1 : H + 1, SCOLS = W + 1;
  constexpr int A_CH = SROWS * SCOLS * POSB, A_BYTES = NCH * A_CH, NBUF = DB ? 2 : 1;
  constexpr int PPR = (W + 3) / 4;                          // 1 KiB DMA pieces per image row
  constexpr int DROWS = GEO == 0 ? SROWS : H;               // image rows copied per item
  constexpr int Ho = Geo<GEO, H, W>::Ho, Wo = Geo<GEO, H, W>::Wo;
  static_assert(GEO == 0 ? (H % SPLIT) == 0 : ((H % 2) == 0 && (W % 2) == 0 && SPLIT == 1), "item geometry");
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint8_t* const sA = lds;
  uint8_t* const sW = lds + NBUF * A_BYTES;
  // active inputs per input cell and step (u8, borders zero) and, per class and position, their maximum over
  // the steps of the sum over the class's taps
  constexpr int NCELL = SROWS * SCOLS;
  uint8_t* const s_cin = lds + NBUF * A_BYTES + WL_BYTES;                       // [NCELL][16]
  int* const s_nmax = reinterpret_cast<int*>(s_cin + ((NCELL * 16 + 15) & ~15));   // [NCLS][NPOS]
  constexpr bool DYN = GEO == 0;                           // (the 25 passes of the plain stride-2 layer's item: dealt; handed out it measured 3 us slower)
  int* const s_ctr = s_nmax + NCLS * NPOS;                  // the item's next pass (DYN)
  const unsigned sA_addr = spk_lds_addr(sA);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = a.Cout >> 5;
  const int g = blockIdx.x % G, il = blockIdx.x / G, lanes = gridDim.x / G;

  {  // the group's weight tiles and zeroed input slabs (their borders stay zero for the whole launch)
    const uint4* src = reinterpret_cast<const uint4*>(a.wq + (long long)g * W_BYTES);
    for (int i = tid; i < WL_BYTES / 16; i += SPK_VT_NWV * 64) {
      const int tile = i / (WT / 16), o = i - tile * (WT / 16);
      reinterpret_cast<uint4*>(sW)[i] = src[((tile / TPL) * TPT + tile % TPL) * (WT / 16) + o];
    }
    for (int i = tid; i < NBUF * A_BYTES / 16; i += SPK_VT_NWV * 64) reinterpret_cast<uint4*>(sA)[i] = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();

  const int co = g * 32 + (lane & 31);
  const float scale_f = (float)a.scale[co], bias_f = (float)a.bias[co];
  const float bna = a.bn_a[co], bnb = a.bn_b[co];
  const float Bc = fmaf(bias_f, bna, bnb);
  const float cE = 2.0f * 2.38418579e-07f * (fabsf(bnb) + fabsf(Bc)) + 1e-30f;
  // certification (den_mfma_fp6v2.hip, "Certification"): z = Q4 * Ac4 + Bc, Q4 = P01 * 2^10 + P23; the dropped digits move z_t by at
  // most cT * n_t (|32 d4 + d5| <= 528 units of 2^-s per active input), every fp32 rounding is inside the eps terms
  const float cT = 528.0f * scale_f * fabsf(bna) * 1.000001f;
  const float Ac4 = 1024.0f * scale_f * bna;
  float coef[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) coef[r] = OUT == SPK_VAE_OUT_COLLAPSED ? a.coef[r] : 0.f;

  const int row = lane & 31, half = lane >> 5;
  const int hsel = (row >> 2) & 1, tt = (row & 3) + 4 * (row >> 3);
  const int sc_a = 0x7f7f7f7f;
  const int sc_p = half ? (int)0x82828282u : (int)0x87878787u;     // even digit (K half 0) x 2^8, odd digit x 2^3
  const unsigned lane16 = (unsigned)lane * 16u;
  const int nitems = SPLIT * a.B;

  // copy the input rows of item `itm` into slab `buf` (asynchronous; spk_dma_wait_all + barrier before use)
  auto stage = [&](int itm, int buf) {
    const int b = itm / SPLIT, part = itm - b * SPLIT;
    const unsigned dst0 = sA_addr + buf * A_BYTES;
    for (int id = wave; id < NCH * DROWS * PPR; id += SPK_VT_NWV) {
      const int c = id / (DROWS * PPR), rr = (id / PPR) % DROWS, px4 = id % PPR;
      const int iy = GEO == 0 ? part * RQ + rr : rr;
      if (iy < H) {
        const int np = (W - 4 * px4) < 4 ? (W - 4 * px4) : 4;
        const unsigned long long mask = np == 4 ? ~0ull : ((1ull << (16 * np)) - 1ull);
        const uint8_t* src = a.in + (((long long)b * NCH + c) * H * W + iy * W + 4 * px4) * POSB;
        const int cell = GEO == 0 ? rr * SCOLS + 4 * px4 : (rr + 1) * SCOLS + 1 + 4 * px4;
        spk_dma16s_masked(src, lane16, dst0 + c * A_CH + cell * POSB, mask);
      }
    }
    if (GEO == 0 && part * RQ + SROWS - 1 >= H) {           // the row below the image: zeros
      for (int i = tid; i < NCH * W * POSB / 16; i += SPK_VT_NWV * 64) {
        const int c = i / (W * POSB / 16), o = i % (W * POSB / 16);
        reinterpret_cast<uint4*>(sA + buf * A_BYTES + c * A_CH + (SROWS - 1) * SCOLS * POSB)[o] = make_uint4(0, 0, 0, 0);
      }
    }
  };

  if (DB && il < nitems) stage(il, 0);
  int n = 0;
  for (int itm = il; itm < nitems; itm += lanes, ++n) {
    const int b = itm / SPLIT, part = itm - b * SPLIT;
    const int buf = DB ? (n & 1) : 0;
    if (!DB) stage(itm, 0);
    spk_dma_wait_all();
    __syncthreads();
    if (DB && itm + lanes < nitems) stage(itm + lanes, buf ^ 1);
    if constexpr (DYN) {
      // (every wave took its last pass number of the previous item before the barrier above; the first one of this item is taken
      //  behind the barriers of the counting phases below)
      if (tid == 0) *s_ctr = SPK_VT_NWV;
    }
    const uint8_t* const A0 = sA + buf * A_BYTES;

    // (A) active inputs of every input record (cell, step), summed over the chunks: a spike is the nibble 0x2 = one set bit
    for (int r = tid; r < NCELL * 16; r += SPK_VT_NWV * 64) {
      int n = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const v4i q = *reinterpret_cast<const v4i*>(A0 + c * A_CH + r * 16);
        n += __builtin_popcount((unsigned)q[0]) + __builtin_popcount((unsigned)q[1]) + __builtin_popcount((unsigned)q[2]) +
             __builtin_popcount((unsigned)q[3]);
      }
      s_cin[r] = (uint8_t)n;                                 // <= 64
    }
    __syncthreads();
    // (B) per class and output position: max over the steps of the sum over the class's taps (what the bound multiplies cT by)
    for (int e = tid; e < NCLS * NPOS; e += SPK_VT_NWV * 64) {
      const int cls = e / NPOS, p = e - cls * NPOS, ry = p / CW, rx = p - ry * CW;
      const int cell0 = GEO == 0 ? ry * SCOLS + rx : 2 * ry * SCOLS + 2 * rx;
      const int py = cls >> 1, px = cls & 1;
      unsigned lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};   // sixteen 16-bit sums (even / odd bytes of the four words)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap % 3;
        const bool on = GEO == 1 || ((py == 0 ? ky == 1 : ky != 1) && (px == 0 ? kx == 1 : kx != 1));
        const int dy = GEO == 1 ? ky : ((py == 1 && ky == 0) ? 1 : 0), dx = GEO == 1 ? kx : ((px == 1 && kx == 0) ? 1 : 0);
        if (on) {
          const v4i q = *reinterpret_cast<const v4i*>(s_cin + (cell0 + dy * SCOLS + dx) * 16);
#pragma unroll
          for (int w4 = 0; w4 < 4; ++w4) {
            lo[w4] += (unsigned)q[w4] & 0x00ff00ffu;
            hi[w4] += ((unsigned)q[w4] >> 8) & 0x00ff00ffu;
          }
        }
      }
      unsigned mx = 0;
#pragma unroll
      for (int w4 = 0; w4 < 4; ++w4) {
        mx = max(mx, max(lo[w4] & 0xffffu, lo[w4] >> 16));
        mx = max(mx, max(hi[w4] & 0xffffu, hi[w4] >> 16));
      }
      s_nmax[e] = (int)mx;
    }
    __syncthreads();

    // hb: the weight fragments of the class's first tap, read once per class by the caller
    auto run_pass = [&](auto cls_tag, int k, const v6i (&hb)[SPK_VT_NHOLD][NCH * 2]) __attribute__((always_inline)) {
      constexpr int CLS = decltype(cls_tag)::value, PY = CLS >> 1, PX = CLS & 1;
      constexpr int NHELD = n_on_taps<GEO, CLS>() < SPK_VT_NHOLD ? n_on_taps<GEO, CLS>() : SPK_VT_NHOLD;
      auto held_slot = [](int tap) constexpr {                // which held set carries this tap's fragments (-1: none)
        for (int h = 0; h < NHELD; ++h)
          if (on_tap<GEO, CLS>(h) == tap) return h;
        return -1;
      };
      int tl[TPP];                                         // tiles of the pass; one past the end repeats the first (computed, dropped)
      bool tv[TPP];
#pragma unroll
      for (int i = 0; i < TPP; ++i) {
        tv[i] = TPP * k + i < NTC;
        tl[i] = tv[i] ? TPP * k + i : TPP * k;
      }
      int base[TPP];
#pragma unroll
      for (int i = 0; i < TPP; ++i) {
        int p = 2 * tl[i] + hsel;
        p = p < NPOS ? p : NPOS - 1;
        const int ry = p / CW, rx = p - ry * CW;
        base[i] = (GEO == 0 ? ry * SCOLS + rx : 2 * ry * SCOLS + 2 * rx) * POSB + tt * 16;
      }
      constexpr int NACC = 2;
      v16f acc[TPP][NACC];
#pragma unroll
      for (int i = 0; i < TPP; ++i)
#pragma unroll
        for (int j = 0; j < NACC; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
      auto ldb = [&](int tile) -> v6i {
        const uint8_t* p = sW + tile * WT;
        const v4i x = *reinterpret_cast<const v4i*>(p + lane * 16);
        const v2i y = *reinterpret_cast<const v2i*>(p + 1024 + lane * 8);
        return v6i{x[0], x[1], x[2], x[3], y[0], y[1]};
      };
      // (the builtin, not inline assembly: hipcc then places the hazard wait states between an MFMA and the reads of its
      //  accumulator itself -- an asm form measured slower and raced)
      auto mm = [&](v16f& d, const v4i& av, const v6i& bv, int sb) {
        const v8i a8 = {av[0], av[1], av[2], av[3], 0, 0, 0, 0};
        const v8i b8 = {bv[0], bv[1], bv[2], bv[3], bv[4], bv[5], 0, 0};
        d = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, d, 4, 2, 0, sc_a, 0, sb);
      };
      static_for<9>([&](auto tap_tag) {
        constexpr int TAP = decltype(tap_tag)::value, KY = TAP / 3, KX = TAP % 3;
        // GEO 0: oy = 2 iy - 1 + ky: class parity PY takes ky = 1 (iy = qy) when even, ky = 0 (iy = qy + 1) and ky = 2 (iy = qy) when odd
        constexpr bool ON = GEO == 1 || ((PY == 0 ? KY == 1 : KY != 1) && (PX == 0 ? KX == 1 : KX != 1));
        if constexpr (ON) {
          constexpr int DY = GEO == 1 ? KY : ((PY == 1 && KY == 0) ? 1 : 0), DX = GEO == 1 ? KX : ((PX == 1 && KX == 0) ? 1 : 0);
          constexpr int TOFF = (DY * SCOLS + DX) * POSB;
          if constexpr (NCH == 2) {
            v4i av[TPP][2];
#pragma unroll
            for (int i = 0; i < TPP; ++i) {
              av[i][0] = *reinterpret_cast<const v4i*>(A0 + base[i] + TOFF);
              av[i][1] = *reinterpret_cast<const v4i*>(A0 + A_CH + base[i] + TOFF);
            }
            constexpr int HS = held_slot(TAP);
            constexpr bool HB = HS >= 0;
            constexpr int HQ = HB ? HS : 0;
            const v6i b0 = HB ? hb[HQ][0] : ldb(TAP * TPL + 0), b1 = HB ? hb[HQ][1] : ldb(TAP * TPL + 1),
                      b2 = HB ? hb[HQ][2] : ldb(TAP * TPL + 2), b3 = HB ? hb[HQ][3] : ldb(TAP * TPL + 3);
#pragma unroll
            for (int i = 0; i < TPP; ++i) {
              mm(acc[i][0], av[i][0], b0, sc_p);
              mm(acc[i][1], av[i][0], b1, sc_p);
              mm(acc[i][0], av[i][1], b2, sc_p);
              mm(acc[i][1], av[i][1], b3, sc_p);
            }
          } else {
            v4i av[TPP];
#pragma unroll
            for (int i = 0; i < TPP; ++i) av[i] = *reinterpret_cast<const v4i*>(A0 + base[i] + TOFF);
            constexpr int HS = held_slot(TAP);
            constexpr bool HB = HS >= 0;
            constexpr int HQ = HB ? HS : 0;
            const v6i b0 = HB ? hb[HQ][0] : ldb(TAP * TPL + 0), b1 = HB ? hb[HQ][1] : ldb(TAP * TPL + 1);
#pragma unroll
            for (int i = 0; i < TPP; ++i) {
              mm(acc[i][0], av[i], b0, sc_p);
              mm(acc[i][1], av[i], b1, sc_p);
            }
          }
        }
      });
      // ---- epilogue: fp32 recombination, BN, LIF scan with certification, output
#pragma unroll
      for (int i = 0; i < TPP; ++i) {
        // D_t = D_{t-1} / 2 + cE + 4 eps (|z_t| + |v_{t-1}|) and |v| <= max |z|, so D_t <= 2 cE + 16 eps max_t |z_t| for every t:
        // track max |z| and min |h - 1| (two instructions per step instead of five) and compare once
        float v = 0.f, m = 0.f, zmax = 0.f, dmin = 3.0e38f;
        unsigned mybits = 0;
#pragma unroll
        for (int r2 = 0; r2 < 16; r2 += 2) {
          // the recombination of two steps at a time on the packed fp32 pipe (adjacent accumulator registers)
          const v2f p0 = {acc[i][0][r2], acc[i][0][r2 + 1]}, p1 = {acc[i][1][r2], acc[i][1][r2 + 1]};
          const v2f q4 = __builtin_elementwise_fma(p0, (v2f){1024.0f, 1024.0f}, p1);
          const v2f z2 = __builtin_elementwise_fma(q4, (v2f){Ac4, Ac4}, (v2f){Bc, Bc});
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int r = r2 + e;
            const float z = z2[e];
            zmax = fmaxf(zmax, fabsf(z));
            const float h = fmaf(z - v, 0.5f, v);            // == v + (z - v) * 0.5f: the product is exact
            const float hm = h - 1.0f;
            dmin = fminf(dmin, fabsf(hm));
            if constexpr (OUT == SPK_VAE_OUT_COLLAPSED) {
              // spike = h >= 1: reset v and add the step's coefficient UNDER THE SPIKE MASK (v_cmpx narrows exec, two plain
              // instructions, exec restored): three vector instructions instead of compare + two selects + add (convT2 -5 %;
              // the spike-bit outputs measured slower in this form -- hipcc keeps their sixteen masks in SGPRs -- and keep the C form)
              v = h;
              unsigned long long exec_sv;
              asm volatile("s_mov_b64 %[sv], exec\n\tv_cmpx_le_f32_e32 1.0, %[v]\n\tv_mov_b32_e32 %[v], 0\n\t"
                           "v_add_f32_e32 %[m], %[c], %[m]\n\ts_mov_b64 exec, %[sv]"
                           : [v] "+v"(v), [m] "+v"(m), [sv] "=&s"(exec_sv) : [c] "s"(coef[r]) : "vcc");
            } else {
              const bool s = h >= 1.0f;
              v = s ? 0.0f : h;
              mybits = __builtin_amdgcn_alignbit(mybits, __float_as_uint(hm), 31);   // (mybits << 1) | sign(h - 1)
            }
          }
        }
        if constexpr (OUT != SPK_VAE_OUT_COLLAPSED) mybits = ~(__builtin_bitreverse32(mybits) >> 16) & 0xffffu;   // bit r = NOT sign(h_r - 1)
        const int p = 2 * tl[i] + half;                       // accumulator lane half == position within the tile
        const bool ok = tv[i] && p < NPOS;
        const int pc = p < NPOS ? p : NPOS - 1;
        // dh <= c + 8 eps max |z| (10 eps: a little to spare); c = cE + cT max_t n_t
        const float cb = fmaf((float)s_nmax[CLS * NPOS + pc], cT, cE);
        const bool flg = dmin <= fmaf(zmax, 2.5f * CERT_4EPS, cb);
        const int ry = pc / CW, rx = pc - ry * CW;
        const int oy = GEO == 0 ? 2 * (part * RQ + ry) + PY : ry, ox = GEO == 0 ? 2 * rx + PX : rx;
        const long long pos = ((long long)b * Ho + oy) * Wo + ox;
        const long long nid_f = pos * a.Cout + co;
        spk_cert_flag(a.ws, nid_f, flg && ok);
        if (OUT == SPK_VAE_OUT_COLLAPSED) {
          if (ok) reinterpret_cast<float*>(a.out)[pos * a.Cout + co] = m;
        } else {
          // a 16x16 bit transpose per 16-lane row gives lane t the 16 channel bits of step t (den_mfma_fp6v2.hip)
          const unsigned bitsv = spk_transpose16_rows(mybits, lane);
          const int t = lane & 15, hi = (lane >> 4) & 1;
          if (ok && OUT == SPK_VAE_OUT_S32) {
            const uint2 o = spk_e2m1_record(bitsv);
            uint8_t* rec = reinterpret_cast<uint8_t*>(a.out) + ((((long long)b * G + g) * Ho * Wo + oy * Wo + ox) * T16 + t) * 16;
            *reinterpret_cast<uint2*>(rec + 8 * hi) = o;
          }
          if (ok && OUT == SPK_VAE_OUT_PTC)
            *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(a.out) + (pos * T16 + t) * a.Cout + g * 32 + 16 * hi) = spk_u8_record(bitsv);
        }
      }
    };

    // the item's passes, class-major, dealt round-robin over the waves (every wave gets a mix of cheap and expensive classes); a
    // wave's passes of one class follow one another, so the class's first-tap weight fragments are read once for all of them
    [[maybe_unused]] int Pdyn = wave;                          // (DYN) the wave's pass: the first NWV are dealt, the rest handed out
    static_for<NCLS>([&](auto cls_tag) {
      constexpr int CLS = decltype(cls_tag)::value;
      constexpr int NHELD = n_on_taps<GEO, CLS>() < SPK_VT_NHOLD ? n_on_taps<GEO, CLS>() : SPK_VT_NHOLD;
      int P = DYN ? Pdyn : CLS * NPASS + ((wave - CLS * NPASS) % SPK_VT_NWV + SPK_VT_NWV) % SPK_VT_NWV;   // static: first P >= CLS * NPASS with P = wave (mod NWV)
      if (P < (CLS + 1) * NPASS) {
        v6i hb[SPK_VT_NHOLD][NCH * 2];
#pragma unroll
        for (int h = 0; h < SPK_VT_NHOLD; ++h)
#pragma unroll
          for (int j = 0; j < NCH * 2; ++j) hb[h][j] = v6i{0, 0, 0, 0, 0, 0};
        static_for<NHELD>([&](auto h_tag) {
          constexpr int h = decltype(h_tag)::value, TAPH = on_tap<GEO, CLS>(h);
#pragma unroll
          for (int j = 0; j < NCH * 2; ++j) {
            const uint8_t* p = sW + (TAPH * TPL + j) * WT;
            const v4i x = *reinterpret_cast<const v4i*>(p + lane * 16);
            const v2i y = *reinterpret_cast<const v2i*>(p + 1024 + lane * 8);
            hb[h][j] = v6i{x[0], x[1], x[2], x[3], y[0], y[1]};
          }
        });
        if constexpr (DYN) {
          while (P < (CLS + 1) * NPASS) {
            int nxt = 0;
            if (lane == 0) nxt = atomicAdd(s_ctr, 1);          // (requested before the pass, read behind it)
            run_pass(cls_tag, P - CLS * NPASS, hb);
            P = __builtin_amdgcn_readfirstlane(nxt);
          }
          Pdyn = P;
        } else {
          for (; P < (CLS + 1) * NPASS; P += SPK_VT_NWV) run_pass(cls_tag, P - CLS * NPASS, hb);
        }
      }
    });
    if (!DB) __syncthreads();                                  // everyone is done with the slab before the next copy lands
  }
  spk_dma_wait_all();
  __syncthreads();
  if (tid == 0) spk_cert_handover(a.ws);   // to the repair launch
}

// One flagged neuron, exactly, by one wave: lane = (time step t, quarter of a 32-channel chunk); every contributing tap and
// chunk costs one 4-byte read of the spike record and eight quantised weights (spk_cert_add_active8); 64-bit sums meet through two
// shuffles, then the reference's BN and LIF steps run on the correctly rounded pre-activations and the neuron's output is rewritten.
template <int GEO, int H, int W, int NCH, int OUT>
__device__ __forceinline__ void vae_fix_neuron(const TArgs& a, long long nid, int lane) {
  constexpr int Ho = Geo<GEO, H, W>::Ho, Wo = Geo<GEO, H, W>::Wo;
  const int co = (int)(nid % a.Cout);
  const long long pos = nid / a.Cout;
  const int ox = (int)(pos % Wo), oy = (int)((pos / Wo) % Ho), b = (int)(pos / ((long long)Wo * Ho));
  const int t = lane & 15, q = lane >> 4;
  long long part = 0;
  for (int ky = 0; ky < 3; ++ky) {
    int iy;
    if (GEO == 0) {
      const int ty = oy + 1 - ky;
      if (ty < 0 || (ty & 1) || (ty >> 1) >= H) continue;
      iy = ty >> 1;
    } else {
      iy = 2 * oy - 1 + ky;
      if (iy < 0 || iy >= H) continue;
    }
    for (int kx = 0; kx < 3; ++kx) {
      int ix;
      if (GEO == 0) {
        const int tx = ox + 1 - kx;
        if (tx < 0 || (tx & 1) || (tx >> 1) >= W) continue;
        ix = tx >> 1;
      } else {
        ix = 2 * ox - 1 + kx;
        if (ix < 0 || ix >= W) continue;
      }
      const int tap = ky * 3 + kx;
      for (int c = 0; c < NCH; ++c) {
        if (c * 32 + 8 * q >= a.Cin) continue;                // (padding channels of the last chunk carry no weights)
        const unsigned nib = *reinterpret_cast<const unsigned*>(a.in + ((((long long)b * NCH + c) * H * W + iy * W + ix) * T16 + t) * 16 + 4 * q);
        const int4* qp = reinterpret_cast<const int4*>(a.qtab + ((long long)co * 9 + tap) * a.Cin + c * 32 + 8 * q);
        spk_cert_add_active8(part, nib, qp[0], qp[1]);
      }
    }
  }
  part = spk_cert_sum_quarters(part);
  const double sc = a.scale[co], bi = a.bias[co];
  const float bna = a.bn_a[co], bnb = a.bn_b[co];
  float v = 0.f, m = 0.f;
  unsigned bits = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float y = exact_preact((double)spk_shfl64(part, r), sc, bi);
    const bool s = spk_lif_step_default(v, fmaf(y, bna, bnb));
    if (OUT == SPK_VAE_OUT_COLLAPSED) m = m + (s ? a.coef[r] : 0.f);
    bits |= s ? (1u << r) : 0u;
  }
  if (OUT == SPK_VAE_OUT_COLLAPSED) {
    if (lane == 0) reinterpret_cast<float*>(a.out)[nid] = m;
  } else if (OUT == SPK_VAE_OUT_S32) {
    if (lane < 16) {                                          // lane = time step: one nibble of the (position, t) record
      const int g = co >> 5, G = a.Cout >> 5;
      uint8_t* rec = reinterpret_cast<uint8_t*>(a.out) + ((((long long)b * G + g) * Ho * Wo + oy * Wo + ox) * T16 + lane) * 16;
      spk_cert_patch_nibble(rec, co, (bits >> lane) & 1u);
    }
  } else {
    if (lane < 16) reinterpret_cast<uint8_t*>(a.out)[(pos * T16 + lane) * a.Cout + co] = (uint8_t)((bits >> lane) & 1u);
  }
}

template <int GEO, int H, int W, int NCH, int OUT>
__global__ __launch_bounds__(256) void vae_fp6_fixup_kernel(TArgs a, long long n_words) {
  const int lane = threadIdx.x & 63;
  const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwv = (long long)gridDim.x * 4;
  spk_cert_scan<false>(a.ws, a.ws.flags[1], wv, nwv, n_words, lane == 0,
                       [&](long long nid) __attribute__((always_inline)) { vae_fix_neuron<GEO, H, W, NCH, OUT>(a, nid, lane); });
}

// one block per output channel: channel maximum -> shift s, every weight -> six balanced radix-32 digits, written as the
// per-lane 24-byte B fragments (spk_cert_emit_fragment) of the tiles listed at tiles_per_tap; also the quantised weights
// themselves (int32 [Cout][9][Cin]) for the exact recomputation.  w: Conv2d [Cout][Cin][3][3] or ConvTranspose2d [Cin][Cout][3][3].
__global__ __launch_bounds__(256) void pack_vae_fp6_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                           uint8_t* __restrict__ wq, double* __restrict__ scale,
                                                           double* __restrict__ bias_d, int* __restrict__ qtab, int Cout,
                                                           int Cin, int transposed) {
  __shared__ float smax[256];
  const int co = blockIdx.x, n = Cin * 9;
  const int NCH = (Cin + 31) / 32, TPT = tiles_per_tap(NCH);
  auto wat = [&](int ci, int tap) -> float {
    return transposed ? w[((long long)ci * Cout + co) * 9 + tap] : w[((long long)co * Cin + ci) * 9 + tap];
  };
  float m = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(wat(i / 9, i % 9)));
  const int sh = 29 - spk_channel_exponent(smax, m);     // |w| * 2^sh < 2^29 <= 16.5 * 32^5
  for (int i = threadIdx.x; i < n; i += 256) {
    const int ci = i / 9, tap = i - 9 * ci;
    qtab[((long long)co * 9 + tap) * Cin + ci] = (int)spk_cert_quantise(wat(ci, tap), sh);
  }
  if (threadIdx.x == 0) spk_cert_scale_bias(scale, bias_d, bias, co, sh);
  const int g = co >> 5, col = co & 31;
  for (int rec = threadIdx.x; rec < 9 * TPT * 2; rec += 256) {
    const int kh = rec & 1, tau = rec >> 1, tap = tau / TPT, j = tau % TPT;
    int chunk, digit;
    bool live = true;
    if (NCH == 2) { chunk = j < 4 ? (j >> 1) : kh; digit = j < 4 ? 2 * (j & 1) + kh : 4; }
    else { chunk = 0; digit = j < 2 ? 2 * j + kh : 4; live = j < 2 || kh == 0; }
    spk_cert_emit_fragment(wq + ((long long)g * 9 * TPT + tau) * WT, kh * 32 + col, digit, live, [&](int k) {
      const int ci = chunk * 32 + k;
      return ci < Cin ? (long long)spk_cert_quantise(wat(ci, tap), sh) : 0ll;
    });
  }
}

template <int GEO, int H, int W, int NCH, int OUT, int SPLIT, bool DB>
int launch_vae(const TArgs& a, long long n_words, hipStream_t stream) {
  constexpr int TPT = tiles_per_tap(NCH), TPL = TPT - 1;
  constexpr int SROWS = GEO == 0 ? H / SPLIT + 1 : H + 1;
  constexpr int NPOS = GEO == 0 ? (H / SPLIT) * W : (H / 2) * (W / 2), NCLS = GEO == 0 ? 4 : 1;
  // (+ the four-digit form's counters: u8 [cells][16] and int [classes][positions])
  constexpr size_t lds = (size_t)(DB ? 2 : 1) * NCH * SROWS * (W + 1) * POSB + 9 * TPL * WT +
                         (size_t)((SROWS * (W + 1) * 16 + 15) & ~15) + (size_t)NCLS * NPOS * 4 + 16;
  static_assert(lds <= (size_t)SPK_CU_LDS_BYTES, "this instance's LDS plan does not fit a compute unit");
  const int cus = spk_cu_count(), G = a.Cout / 32;
  const int grid = cus >= G ? (cus / G) * G : G;
  hipLaunchKernelGGL((vae_fp6_kernel<GEO, H, W, NCH, OUT, SPLIT, DB>), dim3(grid), dim3(SPK_VT_NWV * 64), lds, stream, a);
  SPK_LAUNCH_CHECK();
  hipLaunchKernelGGL((vae_fp6_fixup_kernel<GEO, H, W, NCH, OUT>), dim3(4 * cus), dim3(256), 0, stream, a, n_words);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

}  // namespace

extern "C" long long spk_vae_fp6_packed_bytes(int Cout, int Cin) {
  if (Cout <= 0 || Cin <= 0 || Cin > 64 || (Cin % 8) || (Cout % 32)) return -1;
  return (long long)(Cout / 32) * 9 * tiles_per_tap((Cin + 31) / 32) * WT;
}

extern "C" int spk_vae_fp6_pack(const float* w, const float* bias, uint8_t* wq, double* scale, double* bias_d, int* qtab,
                                int Cout, int Cin, int transposed, hipStream_t stream) {
  if (!w || !wq || !scale || !bias_d || !qtab || Cout <= 0 || Cin <= 0) return SPK_ERR_ARG;
  if (Cin > 64 || (Cin % 8) || (Cout % 32)) return SPK_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pack_vae_fp6_kernel, dim3(Cout), dim3(256), 0, stream, w, bias, wq, scale, bias_d, qtab, Cout, Cin,
                     transposed);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" long long spk_vae_fp6_flag_words(int B, int Cout, int Ho, int Wo) {
  if (B <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0) return -1;
  return spk_cert_flag_words((long long)B * Cout * Ho * Wo);
}

extern "C" int spk_vae_fp6_fwd(const uint8_t* in_s32, const uint8_t* wq, const double* scale, const double* bias_d,
                               const int* qtab, const float* bn_a, const float* bn_b, const float* coef_or_null, void* out,
                               int out_kind, unsigned* flag_words, int T, int B, int H, int W, int Cin, int Cout, int transposed,
                               int flag_cap, hipStream_t stream) {
  if (!in_s32 || !wq || !scale || !bias_d || !qtab || !bn_a || !bn_b || !out || !flag_words || B <= 0) return SPK_ERR_ARG;
  if (out_kind == SPK_VAE_OUT_COLLAPSED && !coef_or_null) return SPK_ERR_ARG;
  const int kind = spk_vae_fp6_kind(Cin, Cout, 3, 2, 1, transposed ? 1 : 0, transposed, T, H, W);
  if (kind < 0 || kind != out_kind) return SPK_ERR_UNSUPPORTED;
  if (B > (1 << 22)) return SPK_ERR_UNSUPPORTED;             // (not in the predicate: the batch is no part of the layer's shape)
  TArgs a;
  a.in = in_s32; a.wq = wq; a.scale = scale; a.bias = bias_d; a.bn_a = bn_a; a.bn_b = bn_b; a.coef = coef_or_null; a.out = out;
  a.qtab = qtab; a.B = B; a.Cout = Cout; a.Cin = Cin;
  const int Ho = transposed ? 2 * H : H / 2, Wo = transposed ? 2 * W : W / 2;
  const long long neurons = (long long)B * Cout * Ho * Wo;
  if (neurons >= (1ll << 32)) return SPK_ERR_UNSUPPORTED;          // neuron ids are 32-bit (not in the predicate: grows with the batch)
  const long long n_words = spk_cert_bitmap_words(neurons);
  a.ws = spk_cert_ws(flag_words, flag_cap, neurons);
  // one instance per (kind, H): spk_vae_fp6_kind has checked that this one exists
  if (kind == SPK_VAE_OUT_COLLAPSED) {                                                        // decoder convT2
    // half images per item, one input slab (two do not fit beside the weights); two class rows per item with two slabs measured
    // 231 against 195 us (profiles/r5_ab_kernel_variants.txt (7))
    return H == 14 ? launch_vae<0, 14, 14, 2, SPK_VAE_OUT_COLLAPSED, 2, false>(a, n_words, stream)
                   : launch_vae<0, 16, 16, 2, SPK_VAE_OUT_COLLAPSED, 2, false>(a, n_words, stream);
  }
  if (kind == SPK_VAE_OUT_S32) {                                                              // decoder convT1
    return H == 7 ? launch_vae<0, 7, 7, 1, SPK_VAE_OUT_S32, 1, true>(a, n_words, stream)
                  : launch_vae<0, 8, 8, 1, SPK_VAE_OUT_S32, 1, true>(a, n_words, stream);
  }
  return H == 14 ? launch_vae<1, 14, 14, 1, SPK_VAE_OUT_PTC, 1, true>(a, n_words, stream)     // encoder conv2
                 : launch_vae<1, 16, 16, 1, SPK_VAE_OUT_PTC, 1, false>(a, n_words, stream);   // (two slabs do not fit)
}

// Which instance exists for a layer: its output form, or -1.  The whole dispatch table of spk_vae_fp6_fwd.
extern "C" int spk_vae_fp6_kind(int Cin, int Cout, int k, int stride, int pad, int out_pad, int transposed, int T, int H, int W) {
  if (k != 3 || stride != 2 || pad != 1 || T != T16 || Cout <= 0 || (Cout % 32) || H != W) return -1;
  const bool mid = H == 14 || H == 16, small = H == 7 || H == 8;
  if (transposed && out_pad == 1 && Cin == 64 && mid) return SPK_VAE_OUT_COLLAPSED;   // decoder convT2
  if (transposed && out_pad == 1 && Cin == 16 && small) return SPK_VAE_OUT_S32;       // decoder convT1
  if (!transposed && Cin == 32 && mid) return SPK_VAE_OUT_PTC;                        // encoder conv2
  return -1;
}
