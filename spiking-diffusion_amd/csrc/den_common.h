// Helpers shared by the matrix-core kernels: the denoiser convolutions (den_mfma.hip: int8 digit planes, den_mfma_fp6.hip and
// den_mfma_fp6v2.hip: fp6), the VQ-VAE layers (vae_fp6.hip) and the training gradients (conv_wgrad.hip, conv_dgrad.hip).
#pragma once
#include "spk_common.h"

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

// LDS of one gfx950 compute unit: what the LDS plan of a one-workgroup-per-CU kernel may add up to.  A constant of the target, not
// a device query: the shape predicates (spk_*_supported) answer on a machine without a GPU.
constexpr int SPK_CU_LDS_BYTES = 160 * 1024;

#define SPK_LDS(p) ((__attribute__((address_space(3))) void*)(p))
#define SPK_GLB(p) ((const __attribute__((address_space(1))) void*)(p))

// CU count of the current device, queried once (a constant of the machine; keeps device queries out of hipGraph capture)
static inline int spk_cu_count() {
  static const int cus = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      return v;
    return 256;
  }();
  return cus;
}

// LDS a workgroup of the current device may allocate (queried once, like the CU count): launches that ask for more than the
// 64 KB every device grants check it first and return SPK_ERR_UNSUPPORTED instead of failing inside the launch
static inline long long spk_lds_limit() {
  static const long long lim = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && v > 0)
      return (long long)v;
    return 65536ll;
  }();
  return lim;
}

// LDS-DMA of 16 bytes per lane: LDS[lds_base + lane * 16] = *(gsrc of this lane); lds_base is wave-uniform.
// Issued as inline assembly on purpose: hipcc treats the builtin (__builtin_amdgcn_global_load_lds) as a FLAT access
// that may touch LDS, and while one is in flight every LDS wait it inserts degrades to s_waitcnt lgkmcnt(0) -- which
// exposes the latency of the most recent fragment prefetch at every fourth MFMA group.  Hidden from the compiler the
// copy only moves the VM counter, so the caller MUST drain it itself (spk_dma_wait_all) before the barrier that
// publishes the data.
__device__ __forceinline__ void spk_dma16(const void* gsrc, unsigned lds_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
               : : "v"(gsrc), "s"(__builtin_amdgcn_readfirstlane(lds_base)) : "memory", "m0");
}
// The same copy with the source given as a wave-uniform base (SGPR pair) + a 32-bit per-lane byte offset: no vector
// address arithmetic per piece.
__device__ __forceinline__ void spk_dma16s(const void* sbase, unsigned voff, unsigned lds_base) {
  const unsigned long long b = (unsigned long long)sbase;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  const unsigned long long bs = ((unsigned long long)hi << 32) | lo;
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               : : "v"(voff), "s"(bs), "s"(__builtin_amdgcn_readfirstlane(lds_base)) : "memory", "m0");
}
// ... and with an explicit EXEC mask for the copy (all lanes must be active around the call: EXEC is restored to -1).
// A piece that covers only lanes 0..31 costs two scalar moves instead of a saveexec / branch / restore sequence.
__device__ __forceinline__ void spk_dma16s_masked(const void* sbase, unsigned voff, unsigned lds_base, unsigned long long mask) {
  const unsigned long long b = (unsigned long long)sbase;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  const unsigned long long bs = ((unsigned long long)hi << 32) | lo;
  const unsigned mlo = __builtin_amdgcn_readfirstlane((unsigned)mask), mhi = __builtin_amdgcn_readfirstlane((unsigned)(mask >> 32));
  const unsigned long long ms = ((unsigned long long)mhi << 32) | mlo;
  asm volatile("s_mov_b32 m0, %2\n\ts_mov_b64 exec, %3\n\tglobal_load_lds_dwordx4 %0, %1\n\ts_mov_b64 exec, -1"
               : : "v"(voff), "s"(bs), "s"(__builtin_amdgcn_readfirstlane(lds_base)), "s"(ms) : "memory", "m0");
}
__device__ __forceinline__ void spk_dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ unsigned spk_lds_addr(const void* p) { return (unsigned)(size_t)SPK_LDS(p); }

// ------------------------------------------------------------------------------------------------ int8 digit planes
// The exact value of one output of the int8 digit-plane kernels (den_mfma.hip, conv_mfma_gather.hip, step_tail.hip) from its
// four base-256 digit sums.  Lane contract: a 32-wide column tile is 16 channels x 2 digit planes, digit parity = lane bit 4,
// so partner lanes col and col ^ 16 hold planes {0, 2} and {1, 3} of one channel (column tiles 0 and 1).  The caller passes
// two accumulator words A, B per column tile; v_permlane16_swap(A, B) returns {even row: A.even, odd row: B.even} and
// {even row: A.odd, odd row: B.odd}, so the even lane of a pair gets all four digits of word A and the odd lane those of
// word B, and each returns (((d0 256 + d1) 256 + d2) 256 + d3) of ITS word.  WIDE is the integer the digit pairs are joined
// in: a digit sum over K 0/1 spikes is at most 128 K, so `int` holds 257 x that for any layer (K < 65 000); the counts forms
// multiply spike COUNTS of up to 127 and need `long long`.  The fp64 fma is exact (|value| < 2^53).
template <typename WIDE>
__device__ __forceinline__ double spk_digits_recombine(int a01, int b01, int a23, int b23) {
  const v2u p01 = __builtin_amdgcn_permlane16_swap((unsigned)a01, (unsigned)b01, false, false);
  const v2u p23 = __builtin_amdgcn_permlane16_swap((unsigned)a23, (unsigned)b23, false, false);
  const WIDE hi = (WIDE)(int)p01[0] * 256 + (int)p01[1], lo = (WIDE)(int)p23[0] * 256 + (int)p23[1];
  return fma((double)hi, 65536.0, (double)lo);
}

// Row of a 32x32 MFMA accumulator tile that register `reg` (0 .. 15) of a lane in lane-half `half` (lane >> 5) holds.
constexpr int spk_acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }
static_assert(spk_acc_row(0, 1) == 4 && spk_acc_row(4, 0) == 8 && spk_acc_row(15, 1) == 31, "32x32 accumulator layout");

// The block-scaled fp4 x fp6 MFMA of den_mfma_fp6.hip and den_mfma_fp6v2.hip as inline assembly (explicit register classes):
// D = A(32 x 64 fp4) * B(64 x 32 fp6) + C, accumulator in AGPRs ("a") or VGPRs ("v"); *_Z: C = 0 (first MFMA of an item).
// s_nop 1: the two wait states between a VALU write of an operand register (the B fragment hand-over is v_mov) and
// the MFMA that reads it, which hipcc's hazard recognizer cannot insert around inline assembly.
#define SPK_FP6_PRE "s_nop 1\n\t"
#define SPK_MFMA_FP6(CLS, acc, av, bv, sa, sb)                                                                       \
  asm volatile(SPK_FP6_PRE "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:4 blgp:2"  \
               : "+" CLS(acc) : "v"(av), "v"(bv), "v"(sa), "v"(sb))
#define SPK_MFMA_FP6_Z(CLS, acc, av, bv, sa, sb)                                                                     \
  asm volatile(SPK_FP6_PRE "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, 0, %3, %4 op_sel_hi:[0,0,0] cbsz:4 blgp:2"   \
               : "=&" CLS(acc) : "v"(av), "v"(bv), "v"(sa), "v"(sb))

// Layout of the position-list buffer written by spk_select_needed (psample.hip) and read by the listed form of the fp6v2
// kernel, for B image slots and R radii.  Bytes: [0, 64) header (u32 ticket of the list-building pass); per radius 16 int32
// (slots per tile-count class 1..6); per radius 6 x B int32 (the slots of each class); per radius B 64-byte records.
__host__ __device__ inline long long spk_need_off_cnt(int r) { return 64 + (long long)r * 64; }
__host__ __device__ inline long long spk_need_off_list(int B, int R, int r) {
  return 64 + (long long)R * 64 + (long long)r * 6 * B * 4;
}
__host__ __device__ inline long long spk_need_off_rec(int B, int R, int r) {
  const long long lists = 64 + (long long)R * 64 + (long long)R * 6 * B * 4;
  return (lists + 63) / 64 * 64 + (long long)r * B * 64;
}
