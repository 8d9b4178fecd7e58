// Codebook-usage statistic of VectorQuantizer_uni.forward (R/snn_model/vae_model.py:705-718), which the reference computes with
// unique / bincount / argmax / masked_select / mse_loss (~12 launches and a sync at its print) on every call:
//   hist[k]   = #{i : idx[i] = k}                                   (bincount, minlength K)
//   used      = #{k : hist[k] > 0}                                  (len(unique(idx)))
//   m         = first k with hist[k] = max hist                     (argmax)
//   t         = (float)N / (float)K                                 (ones(K) * N / K)
//   FID_loss  = 0.001f * (sum_{k != m} ((float)hist[k] - t)^2) / (K - 1)     (mse_loss of int64 against fp32, fp32 arithmetic)
// One launch: every workgroup counts its slice of idx into an LDS histogram and adds each non-zero bin to a global int64 bin
// (integer atomics: exact and order-free); the last workgroup to take a ticket (Guideline 16 counter hand-off: release fence
// before the ticket, acquire fence in the last arriver) writes the histogram and the statistics.  The fp32 sum runs in a fixed
// order (per-thread strided partials, then an LDS tree), so the whole result is deterministic.
#include <limits.h>

#include "spk_common.h"
#include "../../include/spkdiff.h"

namespace {

constexpr int VU_MAX_K = SPK_VQ_USAGE_MAX_K, VU_THREADS = 256, VU_MAX_BLOCKS = 128, VU_PER_BLOCK = 4096;

__global__ __launch_bounds__(VU_THREADS) void vq_usage_kernel(const long long* __restrict__ idx, long long N, int K,
                                                              long long per_block, unsigned* ticket,
                                                              unsigned long long* acc, long long* __restrict__ hist_out,
                                                              long long* __restrict__ stats_out) {
  // the one LDS array of the kernel: the block's histogram, then the "last workgroup" flag, then the final reductions
  __shared__ unsigned lds[VU_MAX_K];
  const int tid = threadIdx.x;
  for (int k = tid; k < K; k += VU_THREADS) lds[k] = 0u;
  __syncthreads();
  const long long lo = (long long)blockIdx.x * per_block;
  const long long hi = lo + per_block < N ? lo + per_block : N;
  for (long long i = lo + tid; i < hi; i += VU_THREADS) {
    const long long c = idx[i];
    if (c >= 0 && c < K) atomicAdd(&lds[c], 1u);       // (an index outside [0, K) is not counted)
  }
  __syncthreads();
  for (int k = tid; k < K; k += VU_THREADS) {
    const unsigned v = lds[k];
    if (v) atomicAdd(&acc[k], (unsigned long long)v);
  }
  // publish the bins, take a ticket (release fence, then the wait, then the relaxed agent-scope add)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = t == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    lds[0] = last ? 1u : 0u;
  }
  __syncthreads();
  if (!lds[0]) return;
  __syncthreads();

  // last workgroup: histogram out, used codes, first maximum
  int* cnt = reinterpret_cast<int*>(lds);              // [256] best count (N < 2^31), -1: none
  int* arg = cnt + VU_THREADS;                         // [256] its code
  unsigned* nz = lds + 2 * VU_THREADS;                 // [256] used codes
  float* red = reinterpret_cast<float*>(lds + 3 * VU_THREADS);   // [256] fp32 partial sums
  int best_c = -1, best_k = K;
  unsigned used = 0;
  for (int k = tid; k < K; k += VU_THREADS) {          // k ascending: strict '>' keeps the first maximum
    const unsigned long long v = __hip_atomic_load(&acc[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    hist_out[k] = (long long)v;
    used += v != 0ull;
    if ((int)v > best_c) { best_c = (int)v; best_k = k; }
  }
  cnt[tid] = best_c;
  arg[tid] = best_k;
  nz[tid] = used;
  __syncthreads();
  for (int s = VU_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const int c2 = cnt[tid + s], k2 = arg[tid + s];
      if (c2 > cnt[tid] || (c2 == cnt[tid] && k2 < arg[tid])) { cnt[tid] = c2; arg[tid] = k2; }
      nz[tid] += nz[tid + s];
    }
    __syncthreads();
  }
  const int m = arg[0];
  // FID_loss over the K - 1 codes other than m
  const float t = (float)N / (float)K;
  float part = 0.f;
  for (int k = tid; k < K; k += VU_THREADS) {
    if (k == m) continue;
    const float d = (float)hist_out[k] - t;
    part = part + d * d;
  }
  red[tid] = part;
  __syncthreads();
  for (int s = VU_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const float mse = red[0] / (float)(K - 1);         // K = 1: 0 / 0 = NaN, as mse_loss of empty tensors
    stats_out[0] = (long long)nz[0];
    stats_out[1] = (long long)m;
    const float fid = 0.001f * mse;
    stats_out[2] = (long long)(unsigned long long)__float_as_uint(fid);   // fp32 bits in the low word
  }
}

}  // namespace

extern "C" int spk_vq_code_usage(const long long* idx, long long N, int K, long long* hist_out, long long* stats_out, void* ws,
                                 hipStream_t stream) {
  if ((N > 0 && !idx) || !hist_out || !stats_out || !ws || N < 0 || K <= 0) return SPK_ERR_ARG;
  if (K > VU_MAX_K || N > (long long)INT_MAX) return SPK_ERR_UNSUPPORTED;
  long long nb = (N + VU_PER_BLOCK - 1) / VU_PER_BLOCK;
  if (nb < 1) nb = 1;
  if (nb > VU_MAX_BLOCKS) nb = VU_MAX_BLOCKS;
  const long long per_block = (N + nb - 1) / nb;
  // ws = {ticket, pad} + K int64 bins, zeroed here for every call
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)(K + 1) * sizeof(long long), stream);
  if (e != hipSuccess) return (int)e;
  unsigned* ticket = reinterpret_cast<unsigned*>(ws);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(ws) + 1;
  hipLaunchKernelGGL(vq_usage_kernel, dim3((unsigned)nb), dim3(VU_THREADS), 0, stream, idx, N, K, per_block, ticket, acc,
                     hist_out, stats_out);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
