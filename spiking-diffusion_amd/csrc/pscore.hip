// One reverse step of the absorbing-state sampler run TEACHER-FORCED: the counterpart of spk_psample_step (psample.hip) that
// scores given tokens x0 under the sampler instead of drawing tokens.
//
//   changes  = (u < 1/t) & ~unmasked ;  unmasked |= changes                 (R/snn_model/vq_diffusion.py:113-124: the same draw,
//                                                                             reveal_u of psample_common.h, the same fp32 test)
//   logp[changes]  = log softmax(logits / temp)[x0]                          (the Categorical of :134-138 evaluated at x0)
//   x_t[changes]   = x0[changes]                                             (:140 with the given token in place of the sample)
//
// z_k = logits_k / temp is the fp32 value the sampler races with (psample.hip); from there fp64, max-subtracted:
// logp = (z_x0 - m) - log sum_k exp(z_k - m).  One wave per latent position, lanes stride over the K classes, each lane adds its
// classes in ascending order and the 64 partial sums meet in a fixed butterfly: the result does not depend on the launch.  Only
// the positions that change (about one per image and step) evaluate the softmax; the q stream of the sampler is not drawn.
#include "spk_common.h"
#include "psample_common.h"
#include "../../include/spkdiff.h"
#include <math.h>

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// PT = per-image temperature (spk_pscore_step_temps): `temp` is a device array indexed by IMAGE, read once per revealed position
// (psample_common.h); a separate instantiation, the scalar kernel's code does not change
template <bool PT>
__global__ __launch_bounds__(256) void pscore_kernel(const float* __restrict__ logits, const long long* __restrict__ x0,
                                                     long long* __restrict__ x_t, uint8_t* __restrict__ unmasked, int t,
                                                     spk_temp_arg_t<PT> temp_arg, const float* __restrict__ u_in, unsigned long long seed,
                                                     unsigned long long offset,
                                                     const unsigned long long* __restrict__ philox_state,
                                                     double* __restrict__ logp_out, int* __restrict__ step_out,
                                                     const int* __restrict__ active, const int* __restrict__ n_active, int B,
                                                     int HW, int K, float* __restrict__ next_input, float t_next) {
  philox_base(philox_state, seed, offset);
  const int lane = threadIdx.x & 63;
  // active-set form: logits hold one slot per ACTIVE image; noise, x0, x_t, unmasked and the outputs stay indexed by image
  const int Bn = spk_active_count(active, n_active, B);
  const long long npos = (long long)Bn * HW;
  const float inv_t = 1.0f / (float)t;
  for (long long ps = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); ps < npos; ps += (long long)gridDim.x * 4) {
    const int b = (int)(ps / HW), hw = (int)(ps % HW);            // b = logits slot
    const long long p = active ? (long long)active[b] * HW + hw : ps;
    const float u = reveal_u(u_in, seed, offset, p, K);
    if (!((u < inv_t) && !unmasked[p])) {                           // (wave-uniform)
      if (next_input && lane == 0) write_next_input(next_input, b, hw, HW, (float)x_t[p], t_next);   // keeps its token
      continue;
    }
    const float temp = spk_temp_of<PT>(temp_arg, active ? active[b] : b);
    const float* row = logits + (long long)b * K * HW + hw;         // class k at row[k * HW]
    float mx = -INFINITY;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, row[(long long)k * HW] / temp);
    mx = wave_max(mx);
    double se = 0.0;
    for (int k = lane; k < K; k += 64) se += exp((double)(row[(long long)k * HW] / temp) - (double)mx);
    se = wave_sum_f64(se);
    if (lane == 0) {
      const long long tok = x0[p];
      double lp = -INFINITY;                                        // a target outside the codebook has probability 0
      if (tok >= 0 && tok < K) lp = ((double)(row[tok * HW] / temp) - (double)mx) - log(se);
      logp_out[p] = lp;
      if (step_out) step_out[p] = t;
      x_t[p] = tok;
      unmasked[p] = 1;
      if (next_input) write_next_input(next_input, b, hw, HW, (float)tok, t_next);
    }
  }
}

}  // namespace

namespace {
template <bool PT>
int pscore_launch(const float* logits_bkhw, const long long* x0, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                  spk_temp_arg_t<PT> temp, const float* u_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                  const unsigned long long* philox_state_or_null, double* logp_out, int* step_out_or_null, int B, int HW, int K,
                  const int* active_or_null, const int* n_active_or_null, float* next_input_b2hw_or_null, hipStream_t stream) {
  if (!logits_bkhw || !x0 || !x_t_inout || !unmasked_inout || !logp_out || t <= 0 || !spk_temp_arg_ok<PT>(temp) || B <= 0 || HW <= 0 ||
      K <= 0)
    return SPK_ERR_ARG;
  if ((active_or_null == nullptr) != (n_active_or_null == nullptr)) return SPK_ERR_ARG;
  if (next_input_b2hw_or_null && active_or_null) return SPK_ERR_ARG;      // (the active-set form gathers its input by slot)
  if (K > 512) return SPK_ERR_UNSUPPORTED;
  const long long npos = (long long)B * HW;
  const int grid = npos > 4 * 4096 ? 4096 : (int)((npos + 3) / 4);    // four positions (waves) per workgroup, grid-stride beyond
  hipLaunchKernelGGL(pscore_kernel<PT>, dim3(grid), dim3(256), 0, stream, logits_bkhw, x0, x_t_inout, unmasked_inout, t, temp,
                     u_or_null, philox_seed, philox_offset, philox_state_or_null, logp_out, step_out_or_null, active_or_null,
                     n_active_or_null, B, HW, K, next_input_b2hw_or_null, (float)(t - 1));
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
}  // namespace

extern "C" int spk_pscore_step(const float* logits_bkhw, const long long* x0, long long* x_t_inout, uint8_t* unmasked_inout,
                               int t, float temp, const float* u_or_null, unsigned long long philox_seed,
                               unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                               double* logp_out, int* step_out_or_null, int B, int HW, int K, const int* active_or_null,
                               const int* n_active_or_null, float* next_input_b2hw_or_null, hipStream_t stream) {
  return pscore_launch<false>(logits_bkhw, x0, x_t_inout, unmasked_inout, t, temp, u_or_null, philox_seed, philox_offset,
                              philox_state_or_null, logp_out, step_out_or_null, B, HW, K, active_or_null, n_active_or_null,
                              next_input_b2hw_or_null, stream);
}

// The same step with one temperature per IMAGE: temp_b fp32 [B] on the device (include/spkdiff.h).
extern "C" int spk_pscore_step_temps(const float* logits_bkhw, const long long* x0, long long* x_t_inout, uint8_t* unmasked_inout,
                                     int t, const float* temp_b, const float* u_or_null, unsigned long long philox_seed,
                                     unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                                     double* logp_out, int* step_out_or_null, int B, int HW, int K, const int* active_or_null,
                                     const int* n_active_or_null, float* next_input_b2hw_or_null, hipStream_t stream) {
  return pscore_launch<true>(logits_bkhw, x0, x_t_inout, unmasked_inout, t, temp_b, u_or_null, philox_seed, philox_offset,
                             philox_state_or_null, logp_out, step_out_or_null, B, HW, K, active_or_null, n_active_or_null,
                             next_input_b2hw_or_null, stream);
}
