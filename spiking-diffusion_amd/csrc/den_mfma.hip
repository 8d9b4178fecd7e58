// 3x3 convolution over binary spike tensors on the MI355X matrix cores, with the BN + LIF scan (or the time-mean
// read-out) fused into the accumulator epilogue.  This is the denoiser's conv2..conv6
// (R/snn_model/vq_diffusion.py:166-187,201-206): >99.9 % of the sampling FLOPs.
//
// EXACT INTEGER FORMULATION.  The A operand is spikes (0/1, exact in int8).  Each fp32 weight is re-encoded once
// (spk_den_pack_weight_i8) as a 30-bit fixed-point number relative to its output channel's largest magnitude and
// split into four balanced base-256 digits D0..D3 in [-128,127]:  w_q = 2^-s * sum_d D_d * 256^(3-d).  Weights within
// 2^7 of the channel maximum are represented exactly (w_q == w); smaller ones are rounded at 2^-30 of that maximum
// (orders of magnitude below one fp32 ulp of any sum they take part in).  The four digit planes are four int8 GEMMs
// sharing the A operand, accumulated EXACTLY in int32 by v_mfma_i32_32x32x32_i8 (2x the bf16 MFMA rate), recombined
// exactly in fp64 and rounded ONCE to fp32: the pre-activation is the correctly rounded value of sum(w_q) + bias --
// independent of accumulation order and bit-reproducible.
//
// MAPPING.  GEMM rows = (position, time step), columns = output channels x digit planes, K = 9 taps x Cin.
//   * A work item = one image x 16 output channels.  The kernel is PERSISTENT: one workgroup (4 waves, one per
//     SIMD, 512 registers each) per CU walks items image-major, so consecutive items reuse the image from L2.
//     All accumulators of an item stay in registers over the whole K loop (7 row tiles x 2 column tiles x 16).
//   * A 32x32 row tile = 2 latent positions x 16 time steps, ordered so that lane-half h of the accumulator holds
//     position h with t = register index: the LIF scan over T is a 16-step in-register loop, no cross-lane traffic.
//   * A 32-wide column tile = 16 channels x 2 digit planes (digit parity = lane bit 4); v_permlane16_swap hands each
//     partner lane both digits of 8 of the 16 time steps, they recombine in fp64 and swap the fp32 results.
//   * Spikes are stored channel-chunked ("CPTC": [B][C/32][HW][T][32] u8) so that the 32-channel slab of one image
//     needed per K chunk is ONE contiguous 25 KB block.  It is copied by LDS-DMA (global_load_lds_dwordx4, no
//     staging registers) into a zero-bordered LDS image [(H+2)(W+2)][T][32]; all 9 taps read it with a constant
//     address offset (no im2col, no 9x re-fetch).  Packed weights are laid out exactly in LDS order (18 KB linear).
//   * LDS is double buffered: the DMA of chunk i+1 (also across item boundaries) is in flight while the 126 MFMAs
//     per wave of chunk i run, and the epilogue of an item overlaps the first DMA of the next one.  One barrier per
//     chunk.  LDS fragment reads are software pipelined two fragments ahead of the MFMA that consumes them.
//   * LDS images are XOR-swizzled at 16-B granularity (A: by t >= 8 through the DMA source lane; W: by column >= 16,
//     baked into the packed weights) so that every ds_read_b128 of a fragment is bank-conflict free.
//   * Spike emission: every lane collects the 16 spike bits of its neuron; a 16x16 bit-matrix transpose inside each
//     16-lane row (4 DPP exchange rounds) hands lane t the 16 channel bits of step t, which it expands to 16 bytes and
//     writes as ONE 16-byte store per (position, time step).
#include "den_common.h"
#include "../../include/spkdiff.h"
#include <stdlib.h>
#include <type_traits>

namespace {


constexpr int T16 = 16;
constexpr int CK = 32;                           // channels per K chunk
constexpr int POS_BYTES = T16 * CK;              // 512 B per latent position per chunk
constexpr int W_CHUNK_BYTES = 9 * 2 * 32 * CK;   // 18432 B per (channel group, chunk)
constexpr int W_PIECES = W_CHUNK_BYTES / 1024;   // 18 one-KiB DMA pieces

struct MfmaArgs {
  const uint8_t* in0; const uint8_t* in1; int nch0, nch1;
  const int8_t* wq; const double* scale; const double* bias; const float* bn_a; const float* bn_b;
  uint8_t* out; float* out_f32; float* v_io;
  uint8_t* out_cnt;   // optional per-neuron spike counts over T, [B][Cout/32][HW][32] (input of the time-collapsed conv6)
  int B, H, W, Cout, mode;
  const int* n_dyn;   // optional device-side batch count (<= B): only images [0, *n_dyn) are processed
};

// NT = row tiles per wave (7 for 7x7 latents, 8 for 8x8); NPA = A-slab DMA pieces per wave (H*ceil(W/2)/4, rounded up).
template <int NT, int NPA, int MODE>
__global__ __launch_bounds__(256, 1) void conv3x3_mfma_kernel(MfmaArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int HW = a.H * a.W, PW = a.W + 2;
  const int npp = (a.H + 2) * PW;
  const int A_BYTES = npp * POS_BYTES;
  // LDS: [A buf0][A buf1][W buf0][W buf1]
  uint8_t* const sA = lds;
  uint8_t* const sW = lds + 2 * A_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunks = a.nch0 + a.nch1;
  const int G = a.Cout >> 4;
  const int Bn = spk_batch_count(a.n_dyn, a.B);
  const int total = Bn * G;

  // zero both A images once: the borders stay zero for the whole kernel, interiors are overwritten by DMA
  for (int i = tid; i < 2 * A_BYTES / 16; i += 256) reinterpret_cast<uint4*>(sA)[i] = make_uint4(0, 0, 0, 0);

  // per-lane LDS byte offsets of this wave's A fragments (tile ti = wave + 4*i); absent tiles read the zero border
  const int row = lane & 31, half = lane >> 5;
  const int hsel = (row >> 2) & 1, tt = (row & 3) + 4 * (row >> 3);
  int a_off[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int p = 2 * (wave + 4 * i) + hsel;
    const int pp = p < HW ? (p / a.W + 1) * PW + (p % a.W) + 1 : 0;
    a_off[i] = pp * POS_BYTES + tt * CK + 16 * (half ^ (tt >> 3));   // 16-B halves swapped for t >= 8: bank-conflict-free
  }
  const int b_off = (lane & 31) * CK + 16 * (half ^ ((lane >> 4) & 1));   // same swizzle, baked into the packed weights

  // DMA piece table, built ONCE per wave with wave-uniform (scalar) values, one packed word per A piece (bits 0..14
  // source byte offset in the slab, 15..30 LDS byte offset in the image, bit 31 = full piece): the A slab of a chunk is
  // H image rows x ceil(W/2) pieces of two positions (1 KiB, the last piece of an odd-width row covers one position =
  // lanes 0..31), wave w copies pieces [w*NPA, (w+1)*NPA); the W slab is 18 one-KiB pieces, wave w copies pieces w,
  // w+4, ...  Pieces beyond the slab repeat an earlier one (a harmless duplicate) so that the K loop issues
  // unconditionally.  The copies are issued from inline assembly with a scalar base (den_common.h: hipcc then keeps
  // counted lgkmcnt waits for the fragment prefetch instead of lgkmcnt(0) while a copy is in flight).
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const int pprow = (a.W + 1) >> 1;
  const int nA = a.H * pprow;
  unsigned pa_pk[NPA];
#pragma unroll
  for (int j = 0; j < NPA; ++j) {
    int id = wave_s * NPA + j;
    id = id < nA ? id : nA - 1;
    const int y = id / pprow, px = id - y * pprow;
    const unsigned src = (unsigned)((y * a.W + 2 * px) * POS_BYTES), dst = (unsigned)(((y + 1) * PW + 1 + 2 * px) * POS_BYTES);
    pa_pk[j] = src | (dst << 15) | ((2 * px + 1 < a.W) ? 0x80000000u : 0u);
  }
  const unsigned lane_a = (unsigned)(lane ^ ((lane >> 4) & 1)) * 16u;     // swizzled source lane (see a_off)
  const unsigned lane_w = (unsigned)lane * 16u;
  const unsigned wave_k = (unsigned)wave_s * 1024u;
  const unsigned sA_addr = spk_lds_addr(sA), sW_addr = sA_addr + 2 * A_BYTES;

  // piece q of this wave: q < NPA -> A piece q, else W piece wave + 4 * (q - NPA)
  constexpr int NPW = (W_PIECES + 3) / 4;
  auto issue_piece = [&](int q, const uint8_t* aslab, const int8_t* wslab, unsigned dA, unsigned dW) {
    if (q < NPA) {
      const unsigned pk = pa_pk[q];
      const unsigned long long mask = (pk >> 31) ? ~0ull : 0xffffffffull;
      spk_dma16s_masked(aslab + (pk & 0x7fffu), lane_a, dA + ((pk >> 15) & 0xffffu), mask);
    } else {
      unsigned ko = wave_k + 4096u * (unsigned)(q - NPA);
      if (4 * (q - NPA) + 3 >= W_PIECES) ko = ko < (unsigned)W_PIECES * 1024u ? ko : ko - 4096u;
      spk_dma16s(wslab + ko, lane_w, dW + ko);
    }
  };
  auto slabs = [&](int item, int c, const uint8_t*& aslab, const int8_t*& wslab) {
    const int b = item / G, g = item - b * G;
    aslab = c < a.nch0 ? a.in0 + ((long long)b * a.nch0 + c) * HW * POS_BYTES
                       : a.in1 + ((long long)b * a.nch1 + (c - a.nch0)) * HW * POS_BYTES;
    wslab = a.wq + ((long long)g * nchunks + c) * W_CHUNK_BYTES;
  };

  const int col = lane & 31, ch = col & 15, odd = col >> 4;

  int it = 0;                                      // running chunk counter: LDS buffer = it & 1
  if ((int)blockIdx.x < total) {
    const uint8_t* as0; const int8_t* ws0;
    slabs(blockIdx.x, 0, as0, ws0);
#pragma unroll
    for (int q = 0; q < NPA + NPW; ++q) issue_piece(q, as0, ws0, sA_addr, sW_addr);
  }
  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    v16i acc[NT][2];      // written (not accumulated) by tap 0 of the first chunk: no explicit zeroing
    // epilogue constants of this item's channel: loaded now, their latency hides under the K loop
    const int b = item / G, g = item - b * G;
    const int co = g * 16 + ch;
    const double sc = a.scale[co], bi = a.bias[co];
    float bn_a = 1.f, bn_b = 0.f;
    if (MODE == SPK_MODE_LIF) { bn_a = a.bn_a[co]; bn_b = a.bn_b[co]; }
    for (int c = 0; c < nchunks; ++c, ++it) {
    const int buf = it & 1;
    spk_dma_wait_all();  // this wave's share of the chunk's DMA has landed ...
    __syncthreads();     // ... and so has everyone else's; everyone is done with the other buffer
    // next chunk (possibly of the next item): its DMA pieces are issued between the MFMA groups below
    int nitem = item, nc = c + 1;
    if (nc == nchunks) { nc = 0; nitem = item + gridDim.x; }
    const bool have_next = nitem < total;      // otherwise the same chunk is copied once more (never read)
    const uint8_t* n_aslab; const int8_t* n_wslab;
    slabs(have_next ? nitem : item, have_next ? nc : c, n_aslab, n_wslab);
    const unsigned n_dA = sA_addr + (buf ^ 1) * A_BYTES;            // LDS byte addresses of the DMA destinations
    const unsigned n_dW = sW_addr + (buf ^ 1) * W_CHUNK_BYTES;

    // ---------------- 9 taps x NT row tiles x 2 column tiles, fragments read four steps ahead ------------------
    // FIRST (the first K chunk of an item): tap 0 starts every accumulator from a zero C operand instead of zeroing
    // 224 accumulator registers by hand before the loop.
    auto compute = [&](auto first_tag) {
      constexpr bool FIRST = decltype(first_tag)::value;
      const uint8_t* A = sA + buf * A_BYTES;
      const uint8_t* Wb = sW + buf * W_CHUNK_BYTES + b_off;
      auto lda = [&](int s) -> v4i {
        const int tap = s / NT, i = s % NT;
        const int toff = ((tap / 3 - 1) * PW + (tap % 3 - 1)) * POS_BYTES;
        return *reinterpret_cast<const v4i*>(A + a_off[i] + toff);
      };
      v4i bc0 = *reinterpret_cast<const v4i*>(Wb), bc1 = *reinterpret_cast<const v4i*>(Wb + 32 * CK);
      v4i bn0 = bc0, bn1 = bc1;
      constexpr int PF = 4;                      // A fragments in flight ahead of the MFMA that consumes them
      v4i af[PF];
#pragma unroll
      for (int s = 0; s < PF; ++s) af[s] = lda(s);
#pragma unroll
      for (int s = 0; s < 9 * NT; ++s) {
        const int tap = s / NT, i = s % NT;
        const v4i av = af[s % PF];
        if (s + PF < 9 * NT) af[s % PF] = lda(s + PF);
        if (i == 0 && tap + 1 < 9) {
          bn0 = *reinterpret_cast<const v4i*>(Wb + ((tap + 1) * 2 + 0) * 32 * CK);
          bn1 = *reinterpret_cast<const v4i*>(Wb + ((tap + 1) * 2 + 1) * 32 * CK);
        }
        if (FIRST && tap == 0) {
          const v16i z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
          acc[i][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bc0, z, 0, 0, 0);
          acc[i][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bc1, z, 0, 0, 0);
        } else {
          acc[i][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bc0, acc[i][0], 0, 0, 0);
          acc[i][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bc1, acc[i][1], 0, 0, 0);
        }
        if (i == NT - 1) { bc0 = bn0; bc1 = bn1; }
        // DMA schedule: NPA + NPW pieces spread over the 9*NT steps (every DMA_EVERY-th step issues one piece)
        {
          constexpr int NPIECES = NPA + NPW;
          constexpr int DMA_EVERY = (9 * NT) / NPIECES;
          if (s % DMA_EVERY == 0 && s / DMA_EVERY < NPIECES) {
            issue_piece(s / DMA_EVERY, n_aslab, n_wslab, n_dA, n_dW);
          }
        }
        __builtin_amdgcn_sched_barrier(0);     // keep the read-ahead distance: hipcc otherwise sinks every ds_read
      }                                         // to just before its MFMA (one exposed LDS latency per tile)
    };
    if (c == 0) compute(std::true_type{}); else compute(std::false_type{});

    }   // chunks
    // ---------------- epilogue: exact recombination, BN, LIF scan over the 16 accumulator registers ----------
    // recombine(i, x): spk_digits_recombine (den_common.h) on the words of t = r and t = r + 8 -- the even lane recombines ITS
    // time step t = r, the odd lane t = r + 8 -- and a third swap hands both lanes all 16 fp32 values.
    auto recombine = [&](int i, float (&x)[16]) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const double s = spk_digits_recombine<int>(acc[i][0][r], acc[i][0][r + 8], acc[i][1][r], acc[i][1][r + 8]);
        const float xm = (float)fma(s, sc, bi);                        // the one rounding to fp32 (s*sc is exact)
        const v2u xx = __builtin_amdgcn_permlane16_swap(__float_as_uint(xm), __float_as_uint(xm), false, false);
        x[r] = __uint_as_float(xx[0]);                                 // t = r     (computed by the even lane)
        x[r + 8] = __uint_as_float(xx[1]);                             // t = r + 8 (computed by the odd lane)
      }
    };
    if (MODE == SPK_MODE_LIF) {
      // The LIF scan runs on TWO row tiles at once: even lanes scan tile ip, odd lanes tile ip + 1.  Each lane collects
      // its neuron's 16 spike bits; a DPP bit-matrix
      // transpose inside every 16-lane row (= 16 channels of one position) turns them into per-time-step channel masks.
#pragma unroll
      for (int ip = 0; ip < NT; ip += 2) {
        // Pairwise exchange: spk_digits_recombine on the words of tiles ip and ip + 1 gives the even lane all four digits
        // of ONE neuron of tile ip and the odd lane those of tile ip + 1, for all 16 steps; the odd tile out of an odd NT
        // is split over the lane parities by time steps (recombine()).
        float xa[16];
        const bool paired = ip + 1 < NT;
        // keep this pair's accumulators in their AGPR tuples up to here: hipcc otherwise copies 16-register tuples
        // to VGPRs at the top of the epilogue and spills (den_mfma_fp6.hip)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          asm volatile("" : "+a"(acc[ip][ct]));
          if (paired) asm volatile("" : "+a"(acc[ip + 1][ct]));
        }
        if (paired) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            // spk_digits_recombine<int> of den_common.h, written out: the call reorders this launch's accumulator reads
            const v2u p01 = __builtin_amdgcn_permlane16_swap((unsigned)acc[ip][0][r], (unsigned)acc[paired ? ip + 1 : ip][0][r], false, false);
            const v2u p23 = __builtin_amdgcn_permlane16_swap((unsigned)acc[ip][1][r], (unsigned)acc[paired ? ip + 1 : ip][1][r], false, false);
            const int hi = (int)p01[0] * 256 + (int)p01[1], lo = (int)p23[0] * 256 + (int)p23[1];
            const double s = fma((double)hi, 65536.0, (double)lo);        // exact
            xa[r] = (float)fma(s, sc, bi);                                // the one rounding to fp32
          }
        } else {
          recombine(ip, xa);
        }
        const int ti = wave + 4 * (ip + (paired ? odd : 0));
        const int p = 2 * ti + half;                  // accumulator lane-half == position within the tile
        const bool pos_ok = p < HW && (paired || !odd);
        const long long vidx = ((long long)b * a.Cout + co) * HW + (pos_ok ? p : 0);
        float v = a.v_io ? a.v_io[vidx] : 0.f;
        unsigned mybits = 0;                    // bit r = this lane's neuron fired at t = r
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool s = spk_lif_step_default(v, fmaf(xa[r], bn_a, bn_b)) && pos_ok;
          mybits |= s ? (1u << r) : 0u;
        }
        const unsigned cnt = __popc(mybits);
        // lanes of a 16-lane row are the 16 channels of one (tile, position): transposing the 16x16 bit matrix gives
        // lane t the 16 channel bits of time step t -- the 16 bytes it stores
        const unsigned bitsv = spk_transpose16_rows(mybits, lane);
        if (a.v_io && pos_ok) a.v_io[vidx] = v;
        if (a.out_cnt && pos_ok)
          a.out_cnt[(((long long)b * (a.Cout >> 5) + (co >> 5)) * HW + p) * CK + (co & 31)] = (uint8_t)cnt;
        // every lane stores one (position, time step): 16 channels = 16 bytes
        if (pos_ok) {
          const uint4 o = spk_u8_record(bitsv);
          const int co0 = g * 16;
          uint8_t* dst = a.out + ((((long long)b * (a.Cout >> 5) + (co0 >> 5)) * HW + p) * T16 + (lane & 15)) * CK +
                         (co0 & 31);
          *reinterpret_cast<uint4*>(dst) = o;
        }
        __builtin_amdgcn_sched_barrier(0);        // keep the tile pairs from being interleaved (VGPR pressure)
      }
    } else {
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        float x[16];
        asm volatile("" : "+a"(acc[i][0]));
        asm volatile("" : "+a"(acc[i][1]));
        recombine(i, x);
        const int p = 2 * (wave + 4 * i) + half;
        float msum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) msum = msum + x[r];                // torch.sum(x6, dim=0), t order
        if (!odd && p < HW) a.out_f32[((long long)b * a.Cout + co) * HW + p] = msum / 16.0f;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }   // items
  spk_dma_wait_all();     // the copy issued during the very last chunk must not outlive the workgroup's LDS allocation
}

// ------------------------------------------------------------------------------------------------ time-collapsed conv6
// conv6 has no BN / LIF: logits = (sum_t conv6(s_t)) / T = (conv6_linear(sum_t s_t) + T*bias) / T.  The A operand
// becomes the per-neuron spike COUNT over T (0..16, exact in int8) and the GEMM loses its factor T in M: rows are
// (image, position) pairs only.  The work is tiny (~0.6 M MFMAs for B = 256), so the kernel is deliberately simple:
// one workgroup per 32-row tile x 16 output channels, operands straight from L2 (counts 4 MB, weights 3.7 MB).
// Numerics: sum first, round once -- at least as accurate as the reference's per-step rounding (|diff| <~ 1 ulp).
struct CntArgs {
  const uint8_t* c0; const uint8_t* c1; int nch0, nch1;
  const int8_t* wq; const double* scale; const double* bias; float* out;
  int B, H, W, Cout, T;
  const int* n_dyn;     // optional device-side batch count (<= B)
};

// A wave = one 32-row tile x 16 output channels.  With few rows (the sampler's active set) the launch is bound by the
// latency of a wave's chain of dependent gathers, not by throughput: the four waves of a workgroup then SPLIT the K chunks
// of one tile (wave w: chunks w, w + 4, ...) and add their int32 partial sums in LDS (30 -> 17 us at ~100 active images).
__global__ __launch_bounds__(256) void conv3x3_counts_mfma_kernel(CntArgs a) {
  __shared__ int red[2][16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int HW = a.H * a.W;
  const int Bn = spk_batch_count(a.n_dyn, a.B);
  const long long nrows = (long long)Bn * HW;
  const bool split = nrows <= 32 * 160;                     // (uniform over the launch)
  const long long tile = split ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + wave;
  if (tile * 32 >= nrows) return;
  const int g = blockIdx.y;
  const int nchunks = a.nch0 + a.nch1;
  const int row = lane & 31, half = lane >> 5;
  const long long R = tile * 32 + row;
  const bool rvalid = R < nrows;
  const int b = rvalid ? (int)(R / HW) : 0, p = rvalid ? (int)(R % HW) : 0;
  const int y = p / a.W, x = p % a.W;
  const int boff = (lane & 31) * CK + 16 * (half ^ ((lane >> 4) & 1));
  if (split) {
    for (int i = threadIdx.x; i < 2 * 16 * 64; i += 256) (&red[0][0][0])[i] = 0;
    __syncthreads();
  }
  v16i acc0 = {0}, acc1 = {0};
  for (int c = split ? wave : 0; c < nchunks; c += split ? 4 : 1) {
    const uint8_t* src = c < a.nch0 ? a.c0 + ((long long)b * a.nch0 + c) * HW * CK
                                    : a.c1 + ((long long)b * a.nch1 + (c - a.nch0)) * HW * CK;
    const int8_t* wsrc = a.wq + ((long long)g * nchunks + c) * W_CHUNK_BYTES + boff;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
      const bool ok = rvalid && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
      // unconditional load from a clamped address + select: a load under a per-lane condition makes hipcc branch around
      // it and drain vmcnt(0) per tap, which serialises the nine gathers of a chunk (36 -> 2x faster launch)
      const v4i ld = *reinterpret_cast<const v4i*>(src + (ok ? (long long)(yy * a.W + xx) * CK + 16 * half : 0));
      const v4i av = ok ? ld : (v4i){0, 0, 0, 0};
      const v4i b0 = *reinterpret_cast<const v4i*>(wsrc + (tap * 2 + 0) * 32 * CK);
      const v4i b1 = *reinterpret_cast<const v4i*>(wsrc + (tap * 2 + 1) * 32 * CK);
      acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b1, acc1, 0, 0, 0);
    }
  }
  if (split) {
    if (wave != 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        atomicAdd(&red[0][r][lane], acc0[r]);
        atomicAdd(&red[1][r][lane], acc1[r]);
      }
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] += red[0][r][lane]; acc1[r] += red[1][r][lane]; }
  }
  const int col = lane & 31, ch = col & 15, odd = col >> 4;
  const int co = g * 16 + ch;
  const double sc = a.scale[co], bT = a.bias[co] * (double)a.T;
  const float invT = 1.0f / (float)a.T;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const double s = spk_digits_recombine<long long>(acc0[r], acc0[r + 8], acc1[r], acc1[r + 8]);
    const float xsum = (float)fma(s, sc, bT);                       // sum over T of the pre-activations, rounded once
    const int rr = r + 8 * odd;                                     // (the even lane recombined register r, the odd lane r + 8)
    const int orow = (rr & 3) + 8 * (rr >> 2) + 4 * half;           // spk_acc_row(rr, half) of den_common.h, written out
    const long long Ro = tile * 32 + orow;
    if (Ro < nrows) {
      const int ob = (int)(Ro / HW), op = (int)(Ro % HW);
      a.out[((long long)ob * a.Cout + co) * HW + op] = xsum * invT;
    }
  }
}

// Full batches: the launch above moves 1.35 GB through the L2 (every wave fetches the 18 KB of weight tiles of each chunk
// itself: 0.9 GB, and its 9 x 1 KB of count fragments: 0.45 GB) in 40 us -- the L2's 34 TB/s.  The four waves of a workgroup
// are four row tiles of the SAME channel group: here they share each chunk's weight tiles AND the count records of the (at most
// four) images their 128 rows lie in through LDS (fetched once per workgroup into registers while the previous chunk is
// multiplied, written to the other buffer, one barrier per chunk; the nine taps of a row are nine LDS reads).  Same sums, same
// epilogue.
__global__ __launch_bounds__(256) void conv3x3_counts_mfma_shared_kernel(CntArgs a) {
  constexpr int MAXP = 64;                                   // positions per image (the launcher checks H * W <= 64)
  // (both arrays are padded to whole 256-thread passes so that every staging store is unconditional, and s_a carries one
  //  all-zero vector, A_ZERO, that the taps outside the image read: conditional LDS accesses become branches with a wait each)
  constexpr int A_ZERO = 4 * MAXP * 2;
  __shared__ v4i s_w[2][5 * 256];
  __shared__ v4i s_a[2][4 * MAXP * 2 + 8];                   // the count records of the (up to) four images the 128 rows lie in
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int HW = a.H * a.W;
  const int Bn = spk_batch_count(a.n_dyn, a.B);
  const long long nrows = (long long)Bn * HW;
  const long long tile = (long long)blockIdx.x * 4 + wave;
  const long long R0 = (long long)blockIdx.x * 128;
  if (R0 >= nrows) return;                                   // (uniform over the workgroup)
  const int g = blockIdx.y;
  const int nchunks = a.nch0 + a.nch1;
  const int row = lane & 31, half = lane >> 5;
  const long long R = tile * 32 + row;
  const bool rvalid = R < nrows;
  const int b = rvalid ? (int)(R / HW) : 0, p = rvalid ? (int)(R % HW) : 0;
  const int y = p / a.W, x = p % a.W;
  const int b_lo = (int)(R0 / HW);                           // 128 rows span at most 4 images (H * W >= 43) -- checked by the launcher
  const int boff16 = ((lane & 31) * CK + 16 * (half ^ ((lane >> 4) & 1))) >> 4;
  constexpr int NV = W_CHUNK_BYTES / 16, NPRE = (NV + 255) / 256;      // 1152 16-byte vectors per chunk, 5 per thread
  const v4i* wg = reinterpret_cast<const v4i*>(a.wq + (long long)g * nchunks * W_CHUNK_BYTES);
  const int na = 4 * HW * 2;                                 // 16-byte vectors of the four images' records per chunk (<= 512)
  // vector e of the staged records: image b_lo + e / (2 HW), position (e / 2) % HW, half e & 1 (this thread's two vectors:
  // image and byte offset are worked out once, not per chunk)
  int a_img[2], a_rem[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int e = threadIdx.x + 256 * j;
    e = e < na ? e : na - 1;
    int bi = b_lo + e / (2 * HW);
    a_img[j] = bi < Bn ? bi : Bn - 1;
    a_rem[j] = (e % (2 * HW)) * 16;
  }
  auto a_src = [&](int c, int j) -> const v4i* {
    const uint8_t* base = c < a.nch0 ? a.c0 + ((long long)a_img[j] * a.nch0 + c) * HW * CK
                                     : a.c1 + ((long long)a_img[j] * a.nch1 + (c - a.nch0)) * HW * CK;
    return reinterpret_cast<const v4i*>(base + a_rem[j]);
  };
  // Register sets S[k & 1] carry chunk k from memory to LDS buffer k & 1: chunk c + 2 is requested while chunk c is multiplied
  // and chunk c + 1 (requested one iteration earlier) is written to the other buffer -- two chunks in flight per workgroup (a
  // chunk is 26 KB and an L2 round trip under this load ~1.5 us: one chunk in flight streams the 16 chunks in 24 us).
  v4i pre[2][NPRE], prea[2][2];
  auto request = [&](int c, auto s_tag) {
    constexpr int S = decltype(s_tag)::value;
#pragma unroll
    for (int j = 0; j < NPRE; ++j) {
      const int e = threadIdx.x + 256 * j;
      pre[S][j] = wg[(long long)c * NV + (e < NV ? e : NV - 1)];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) prea[S][j] = *a_src(c, j);
  };
  auto deposit = [&](auto s_tag) {
    constexpr int S = decltype(s_tag)::value;
#pragma unroll
    for (int j = 0; j < NPRE; ++j) s_w[S][threadIdx.x + 256 * j] = pre[S][j];
#pragma unroll
    for (int j = 0; j < 2; ++j) s_a[S][threadIdx.x + 256 * j] = prea[S][j];
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  static_assert(NPRE == 5, "s_w padding");
  if (threadIdx.x < 2) s_a[threadIdx.x][A_ZERO] = (v4i){0, 0, 0, 0};
  request(0, P0{});
  if (nchunks > 1) request(1, P1{});
  deposit(P0{});
  __syncthreads();
  // LDS vector index of this lane's fragment for tap (0, 0) shifted by (-1, -1), and the taps that lie inside the image
  const int a_base = ((b - b_lo) * HW + p) * 2 + half;
  bool okt[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    okt[tap] = rvalid && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
  }
  v16i acc0 = {0}, acc1 = {0};
  auto step = [&](int c, auto s_tag) {
    constexpr int S = decltype(s_tag)::value;                // c & 1
    if (c + 2 < nchunks) request(c + 2, s_tag);              // (set S is free: chunk c sits in LDS buffer S)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int d = ((tap / 3 - 1) * a.W + (tap % 3 - 1)) * 2;
      const v4i av = s_a[S][okt[tap] ? a_base + d : A_ZERO];
      const v4i b0 = s_w[S][(tap * 2 + 0) * 64 + boff16];
      const v4i b1 = s_w[S][(tap * 2 + 1) * 64 + boff16];
      acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b1, acc1, 0, 0, 0);
    }
    if (c + 1 < nchunks) deposit(std::integral_constant<int, 1 - S>{});
    __syncthreads();     // the next chunk's tiles and records are in place; everyone is done with this chunk's
  };
  for (int c = 0; c < nchunks; c += 2) {
    step(c, P0{});
    if (c + 1 < nchunks) step(c + 1, P1{});
  }
  // (the epilogue of conv3x3_counts_mfma_kernel, the definition, written out: as a shared function both kernels compile differently)
  const int col = lane & 31, ch = col & 15, odd = col >> 4;
  const int co = g * 16 + ch;
  const double sc = a.scale[co], bT = a.bias[co] * (double)a.T;
  const float invT = 1.0f / (float)a.T;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const double s = spk_digits_recombine<long long>(acc0[r], acc0[r + 8], acc1[r], acc1[r + 8]);
    const float xsum = (float)fma(s, sc, bT);                       // sum over T of the pre-activations, rounded once
    const int rr = r + 8 * odd;                                     // (the even lane recombined register r, the odd lane r + 8)
    const int orow = (rr & 3) + 8 * (rr >> 2) + 4 * half;           // spk_acc_row(rr, half) of den_common.h, written out
    const long long Ro = tile * 32 + orow;
    if (Ro < nrows) {
      const int ob = (int)(Ro / HW), op = (int)(Ro % HW);
      a.out[((long long)ob * a.Cout + co) * HW + op] = xsum * invT;
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight packing
// one block per output channel: channel maximum -> shift s, then every weight -> 4 balanced base-256 digits
__global__ __launch_bounds__(256) void pack_i8_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                      int8_t* __restrict__ wq, double* __restrict__ scale,
                                                      double* __restrict__ bias_d, int Cout, int Cin) {
  __shared__ float smax[256];
  const int co = blockIdx.x, n = Cin * 9;
  const float* wc = w + (long long)co * n;
  float m = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(wc[i]));
  const int sh = 30 - spk_channel_exponent(smax, m);     // |w| * 2^sh < 2^30
  if (threadIdx.x == 0) { scale[co] = ldexp(1.0, -sh); bias_d[co] = bias ? (double)bias[co] : 0.0; }
  const int nchunks = Cin / CK, g = co >> 4, ch = co & 15;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int ci = i / 9, tap = i % 9;
    int dg[4];
    spk_balanced_digits<8>((long long)rint(ldexp((double)wc[i], sh)), dg);
    const int c = ci / CK, k = ci % CK;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int ct = d >> 1, colw = (d & 1) * 16 + ch;
      wq[((((long long)(g * nchunks + c) * 9 + tap) * 2 + ct) * 32 + colw) * CK + (k ^ (colw & 16))] = (int8_t)dg[d];
    }
  }
}

// tiles (pairs of latent positions) and input-slab copy pieces per wave: the kernel is instantiated for up to 7 and up to 8 of both
inline int tiles_per_wave(int H, int W) { return ((H * W + 1) / 2 + 3) / 4; }
inline int pieces_per_wave(int H, int W) { return (H * ((W + 1) / 2) + 3) / 4; }
inline size_t lds_bytes(int H, int W) { return 2 * ((size_t)(H + 2) * (W + 2) * POS_BYTES + W_CHUNK_BYTES); }

template <int MODE>
int launch(const MfmaArgs& a, hipStream_t stream) {
  const int cus = spk_cu_count();
  const int total = a.B * (a.Cout / 16);
  dim3 grid(total < cus ? total : cus), blk(256);          // persistent: one workgroup per CU
  if (tiles_per_wave(a.H, a.W) <= 7 && pieces_per_wave(a.H, a.W) <= 7) {
    hipLaunchKernelGGL((conv3x3_mfma_kernel<7, 7, MODE>), grid, blk, lds_bytes(a.H, a.W), stream, a);
  } else {                                                 // (spk_den_conv3x3_mfma_supported: at most 8 of both)
    hipLaunchKernelGGL((conv3x3_mfma_kernel<8, 8, MODE>), grid, blk, lds_bytes(a.H, a.W), stream, a);
  }
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

}  // namespace

extern "C" int spk_den_conv3x3_mfma_supported(int Cout, int Cin, int k, int stride, int pad, int T, int H, int W) {
  if (Cout <= 0 || Cin <= 0 || H <= 0 || W <= 0) return 0;
  // (the LDS plan first: it bounds H * W, so the int products behind it cannot overflow)
  return k == 3 && stride == 1 && pad == 1 && T == T16 && (Cout % 32) == 0 && (Cin % CK) == 0 &&
         lds_bytes(H, W) <= (size_t)SPK_CU_LDS_BYTES && tiles_per_wave(H, W) <= 8 && pieces_per_wave(H, W) <= 8;
}

extern "C" long long spk_den_packed_weight_bytes(int Cout, int Cin) {
  if (Cout <= 0 || Cin <= 0 || (Cout % 16) || (Cin % CK)) return -1;
  return (long long)(Cout / 16) * (Cin / CK) * W_CHUNK_BYTES;
}

extern "C" int spk_den_pack_weight_i8(const float* w, const float* bias, int8_t* wq, double* scale, double* bias_d,
                                      int Cout, int Cin, hipStream_t stream) {
  if (!w || !wq || !scale || !bias_d || Cout <= 0 || Cin <= 0) return SPK_ERR_ARG;
  if ((Cout % 16) || (Cin % CK)) return SPK_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pack_i8_kernel, dim3(Cout), dim3(256), 0, stream, w, bias, wq, scale, bias_d, Cout, Cin);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_den_conv3x3_counts_mfma(const uint8_t* cnt0, int nch0, const uint8_t* cnt1, int nch1,
                                           const int8_t* wq, const double* scale, const double* bias_d, float* out_f32,
                                           int T, int B, int H, int W, int Cout, const int* n_dyn_or_null,
                                           hipStream_t stream) {
  if (!cnt0 || nch0 <= 0 || nch1 < 0 || (nch1 > 0 && !cnt1) || !wq || !scale || !bias_d || !out_f32 || B <= 0 ||
      H <= 0 || W <= 0 || Cout <= 0 || T <= 0)
    return SPK_ERR_ARG;
  if (T > 127 || (Cout % 16)) return SPK_ERR_UNSUPPORTED;      // counts must fit the signed int8 A operand
  CntArgs a;
  a.c0 = cnt0; a.c1 = cnt1; a.nch0 = nch0; a.nch1 = nch1; a.wq = wq; a.scale = scale; a.bias = bias_d; a.out = out_f32;
  a.B = B; a.H = H; a.W = W; a.Cout = Cout; a.T = T; a.n_dyn = n_dyn_or_null;
  const long long tiles = ((long long)B * H * W + 31) / 32;
  dim3 grid((unsigned)tiles, Cout / 16), blk(256);
  // batches of more than 160 row tiles: shared weight tiles and count records
  // (also the sampler's active-set calls: its register-staged stream of two chunks beats the K split of the first kernel even at
  //  a few dozen images -- elimination + position lists 35.4 -> 34.4 ms)
  if ((long long)B * H * W > 32 * 160 && H * W >= 43 && H * W <= 64) {
    hipLaunchKernelGGL(conv3x3_counts_mfma_shared_kernel, dim3((unsigned)((tiles + 3) / 4), Cout / 16), blk, 0, stream, a);
    SPK_LAUNCH_CHECK();
    return SPK_OK;
  }
  hipLaunchKernelGGL(conv3x3_counts_mfma_kernel, grid, blk, 0, stream, a);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_den_conv3x3_mfma(const uint8_t* in0_cptc, int nch0, const uint8_t* in1_cptc, int nch1,
                                    const int8_t* wq, const double* scale, const double* bias_d, const float* bn_a,
                                    const float* bn_b, float* v_inout, uint8_t* out_cptc, uint8_t* out_counts,
                                    float* out_f32, int mode, int T, int B, int H, int W, int Cout,
                                    const int* n_dyn_or_null, hipStream_t stream) {
  if (!in0_cptc || nch0 <= 0 || nch1 < 0 || (nch1 > 0 && !in1_cptc) || !wq || !scale || !bias_d || B <= 0 || H <= 0 ||
      W <= 0 || Cout <= 0)
    return SPK_ERR_ARG;
  if (!spk_den_conv3x3_mfma_supported(Cout, (nch0 + nch1) * CK, 3, 1, 1, T, H, W)) return SPK_ERR_UNSUPPORTED;
  MfmaArgs a;
  a.in0 = in0_cptc; a.in1 = in1_cptc; a.nch0 = nch0; a.nch1 = nch1; a.wq = wq; a.scale = scale; a.bias = bias_d;
  a.bn_a = bn_a; a.bn_b = bn_b; a.out = out_cptc; a.out_f32 = out_f32; a.v_io = v_inout; a.out_cnt = out_counts; a.B = B; a.H = H; a.W = W;
  a.Cout = Cout; a.mode = mode; a.n_dyn = n_dyn_or_null;
  if (mode == SPK_MODE_LIF) {
    if (!bn_a || !bn_b || !out_cptc) return SPK_ERR_ARG;
    return launch<SPK_MODE_LIF>(a, stream);
  }
  if (mode == SPK_MODE_MEAN) {
    if (!out_f32) return SPK_ERR_ARG;
    return launch<SPK_MODE_MEAN>(a, stream);
  }
  return SPK_ERR_UNSUPPORTED;
}
