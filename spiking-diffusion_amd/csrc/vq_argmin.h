// torch.argmin over a row of fp64 code distances, shared by the VectorQuantizer kernels (vq.hip) and the fused ANN encoder
// (ann_vqvae.hip): a NaN is below every number (the first NaN wins), ties go to the lowest index, and the index is always in
// [0, K) -- also for rows of NaN or inf.
#pragma once

constexpr int VQ_NONE = 0x7fffffff;                                // "no candidate yet": loses to every real code

// The argmin in three parts.  A lane sees its codes in ascending order and starts from (+inf, VQ_NONE): it keeps a candidate
// while its best is not NaN and the candidate is NaN or strictly smaller (vq_lane_takes), so it holds its first NaN, else its
// first minimum, else -- every distance +inf -- nothing.  The lanes are combined in torch.argmin's order (vq_better: NaN first,
// then ascending distance, then ascending index), and a row left with VQ_NONE had only +inf distances: code 0 (vq_index).
__device__ __forceinline__ bool vq_lane_takes(double d, double b) { return b == b && !(d >= b); }
__device__ __forceinline__ bool vq_better(double d, int k, double b, int i) {
  if (b != b) return d != d && k < i;
  return d != d || d < b || (d == b && k < i);
}
__device__ __forceinline__ int vq_index(int besti) { return besti == VQ_NONE ? 0 : besti; }

// the wave's 64 (best, besti) pairs combined into every lane
__device__ __forceinline__ void vq_wave_combine(double& best, int& besti) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(besti, off);
    if (vq_better(ob, oi, best, besti)) { best = ob; besti = oi; }
  }
}
