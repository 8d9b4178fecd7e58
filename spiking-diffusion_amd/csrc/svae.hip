// Spiking-MLP kernels of the SNN_VAE baseline (R/snn_model/vae_model.py:198-305, :306-546), eval path:
//   spk_linear_lif_fwd   multi-step layer.Linear (+ the default LIFNode): before_latent_layer, decoder_input, the prior's
//                        teacher-forced pass, and layer.Linear's plain currents
//   spk_svae_ar_fwd      one whole autoregressive Bernoulli loop (PosteriorBernoulliSTBP.forward :470-546 or
//                        PriorBernoulliSTBP.sample :405-423) in ONE launch: each workgroup owns a tile of BT images and runs
//                        every pass of the loop for them, so no state crosses workgroups and there is no grid-wide barrier.
//
// Numerics: every Linear output is an fp32 sum over the inputs in ascending index order (one multiply and one add per term,
// -ffp-contract=off), then + bias, then the reference neuron's fp32 update (spk_lif_step: tau 2, v_th 1, hard reset to 0,
// decay_input).  When the weights and biases are multiples of 2^-12 with small magnitude (spkdiff/synth.py:synth_svae_state)
// every sum is exact in fp32, so spikes and membrane potentials equal the reference's bit for bit whatever order it summed in.
//
// Activations in LDS are stored input-major, image-minor ([n][BT]): the BT images' values of input i are one LDS read, and a
// weight is loaded once for the BT images of the tile.
#include "spk_common.h"
#include "../../include/spkdiff.h"

namespace {

constexpr int SV_THREADS = 256;
constexpr int SV_LDS_MAX = 64 * 1024;

__device__ __forceinline__ bool sv_lif(float& v, float x) { return spk_lif_step<false>(v, x, 2.0f, 0.5f, 1.0f, 0.0f); }

// acc[j] += sum_{i < n} act[i][j] * w[i], i ascending.  act: LDS [n][BT]; w: one weight row.
template <int BT>
__device__ __forceinline__ void sv_dot(float (&acc)[BT], const float* __restrict__ act, const float* __restrict__ w, int n) {
  int i = 0;
  if ((((uintptr_t)w) & 15) == 0) {
    for (; i + 4 <= n; i += 4) {
      const float4 w4 = *reinterpret_cast<const float4*>(w + i);
      const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int j = 0; j < BT; ++j) acc[j] += act[(i + q) * BT + j] * wv[q];
      }
    }
  }
  for (; i < n; ++i) {
    const float wi = w[i];
#pragma unroll
    for (int j = 0; j < BT; ++j) acc[j] += act[i * BT + j] * wi;
  }
}

// ------------------------------------------------------------------------------------------ multi-step Linear (+ LIF)
// Grid (ceil(out/256), ceil(B/BT)); thread = one output neuron for the BT images of its tile, its membrane potentials in
// registers across the T steps.  Per step the tile's inputs are staged in LDS (converted from the input layout).
template <int BT>
__global__ __launch_bounds__(SV_THREADS) void linear_lif_kernel(const void* __restrict__ x, int in_kind,
                                                                const float* __restrict__ w, const float* __restrict__ bias,
                                                                float* __restrict__ v_io, void* __restrict__ out, int out_kind,
                                                                int T, int B, int nin, int nout, int pc, int ph, int pw) {
  extern __shared__ float s_act[];  // [nin][BT]
  const int o = blockIdx.x * SV_THREADS + threadIdx.x;
  const int b0 = blockIdx.y * BT;
  const int nb = min(BT, B - b0);
  const bool live = o < nout;
  const bool lif = out_kind != SPK_LIN_OUT_F32;
  float v[BT];
#pragma unroll
  for (int j = 0; j < BT; ++j) v[j] = (live && lif && j < nb) ? v_io[(long long)(b0 + j) * nout + o] : 0.0f;
  const float bo = (live && bias) ? bias[o] : 0.0f;
  const int phw = ph * pw;
  for (int t = 0; t < T; ++t) {
    __syncthreads();
    for (int e = threadIdx.x; e < nin * BT; e += SV_THREADS) {
      const int i = e / BT, j = e - i * BT;
      float val = 0.0f;
      if (j < nb) {
        const long long b = b0 + j;
        if (in_kind == SPK_LIN_IN_F32) {
          val = reinterpret_cast<const float*>(x)[((long long)t * B + b) * nin + i];
        } else if (in_kind == SPK_LIN_IN_U8) {
          val = reinterpret_cast<const uint8_t*>(x)[((long long)t * B + b) * nin + i] ? 1.0f : 0.0f;
        } else {  // PTC [B,H,W,T,C], i = c*H*W + h*W + w (the reference's flatten(C,H,W))
          const int c = i / phw, hw = i - c * phw;
          val = reinterpret_cast<const uint8_t*>(x)[((b * phw + hw) * T + t) * pc + c] ? 1.0f : 0.0f;
        }
      }
      s_act[e] = val;
    }
    __syncthreads();
    if (!live) continue;
    float acc[BT];
#pragma unroll
    for (int j = 0; j < BT; ++j) acc[j] = 0.0f;
    sv_dot<BT>(acc, s_act, w + (long long)o * nin, nin);
#pragma unroll
    for (int j = 0; j < BT; ++j) {
      if (j >= nb) break;
      const long long b = b0 + j;
      const float cur = acc[j] + bo;
      if (!lif) {
        reinterpret_cast<float*>(out)[((long long)t * B + b) * nout + o] = cur;
        continue;
      }
      const bool s = sv_lif(v[j], cur);
      if (out_kind == SPK_LIN_OUT_U8) {
        if (out) reinterpret_cast<uint8_t*>(out)[((long long)t * B + b) * nout + o] = s ? 1 : 0;
      } else {  // PTC [B,H,W,T,C], o = c*H*W + h*W + w
        const int c = o / phw, hw = o - c * phw;
        reinterpret_cast<uint8_t*>(out)[((b * phw + hw) * T + t) * pc + c] = s ? 1 : 0;
      }
    }
  }
  if (live && lif) {
#pragma unroll
    for (int j = 0; j < BT; ++j)
      if (j < nb) v_io[(long long)(b0 + j) * nout + o] = v[j];
  }
}

// ------------------------------------------------------------------------------------------ autoregressive loop
struct ArLayout {  // float offsets into dynamic LDS
  int xs, zs, s1, s2, v1, v2, v3, total;
};

__host__ __device__ inline ArLayout ar_layout(int bt, int T, int cx, int cz, int h1, int h2, int h3) {
  ArLayout L;
  int off = 0;
  L.xs = off; off += T * cx * bt;         // x_0..x_{T-1}      [T][cx][BT]
  L.zs = off; off += (T + 1) * cz * bt;   // z_0..z_T          [T+1][cz][BT]
  L.s1 = off; off += h1 * bt;             // layer-1 spikes    [h1][BT]
  L.s2 = off; off += h2 * bt;             // layer-2 spikes    [h2][BT]
  L.v1 = off; off += h1 * bt;             // membrane potentials, [n][BT]
  L.v2 = off; off += h2 * bt;
  L.v3 = off; off += h3 * bt;
  L.total = off;
  return L;
}

// Posterior (x != NULL): passes p = 0..T-2 run the MLP over the prefix rows 0..p of [x_s, z_s] and set
// z_{p+1} = spike[last row][c*k + idx[p][b][c]]; the final pass runs all T rows of [x, z_0..z_{T-1}] and sampled_z[s] takes
// the spike at idx[s] of row s (R/snn_model/vae_model.py:491-541).  Prior (x == NULL): passes p = 0..T-1 over z_0..z_p, and
// sampled_z[p] = z_{p+1} (:405-423).  No pass resets a neuron: v runs on through every row of every pass.
// MODE (AR_*): the eval loop above, or only the no-grad prefix passes of one training loop (spk_svae_ar_prefix_fwd).
// AR_POST_PREFIX: passes p = 0..T-2 of the posterior.  AR_PRIOR_PREFIX: the prior's scheduled sampling
// (R/snn_model/vae_model.py:365-390): for p = 0..T-2, a scheduled step (sched[p] != 0) runs the MLP over the prefix rows
// 0..p and sets z_{p+1} = (count_k(last-row spikes) / k + 0.001f * noise > 0.5), any other step copies the teacher row
// zt[p].  Both write z_0..z_{T-1} to zout ([T,B,cz], the z_t_minus of the grad pass) and leave v1..v3 after the passes.
enum { AR_EVAL = 0, AR_POST_PREFIX = 1, AR_PRIOR_PREFIX = 2 };

template <int BT, int MODE>
__global__ __launch_bounds__(SV_THREADS) void svae_ar_kernel(const uint8_t* __restrict__ x, const float* __restrict__ z0,
                                                             const float* __restrict__ w1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2, const float* __restrict__ b2,
                                                             const float* __restrict__ w3, const float* __restrict__ b3,
                                                             float* __restrict__ v1g, float* __restrict__ v2g,
                                                             float* __restrict__ v3g, const int* __restrict__ idx,
                                                             float* __restrict__ zout, uint8_t* __restrict__ qz, int T, int B,
                                                             int cx, int cz, int h1, int h2, int k,
                                                             const uint8_t* __restrict__ sched, const float* __restrict__ noise,
                                                             const float* __restrict__ zt) {
  extern __shared__ float lds[];
  const int h3 = cz * k;
  const ArLayout L = ar_layout(BT, T, cx, cz, h1, h2, h3);
  float* xs = lds + L.xs;
  float* zs = lds + L.zs;
  float* s1 = lds + L.s1;
  float* s2 = lds + L.s2;
  float* v1 = lds + L.v1;
  float* v2 = lds + L.v2;
  float* v3 = lds + L.v3;
  const int b0 = blockIdx.x * BT;
  const int nb = min(BT, B - b0);
  const int tid = threadIdx.x;

  for (int e = tid; e < T * cx * BT; e += SV_THREADS) {
    const int j = e % BT, i = (e / BT) % cx, t = e / (BT * cx);
    xs[e] = (j < nb) ? (x[((long long)t * B + b0 + j) * cx + i] ? 1.0f : 0.0f) : 0.0f;
  }
  for (int e = tid; e < (T + 1) * cz * BT; e += SV_THREADS) zs[e] = (e < cz * BT) ? z0[e / BT] : 0.0f;
  for (int e = tid; e < h1 * BT; e += SV_THREADS) {
    const int j = e % BT;
    v1[e] = (j < nb) ? v1g[(long long)(b0 + j) * h1 + e / BT] : 0.0f;
  }
  for (int e = tid; e < h2 * BT; e += SV_THREADS) {
    const int j = e % BT;
    v2[e] = (j < nb) ? v2g[(long long)(b0 + j) * h2 + e / BT] : 0.0f;
  }
  for (int e = tid; e < h3 * BT; e += SV_THREADS) {
    const int j = e % BT;
    v3[e] = (j < nb) ? v3g[(long long)(b0 + j) * h3 + e / BT] : 0.0f;
  }
  __syncthreads();

  const bool post = cx > 0;
  const int nin1 = cx + cz;
  const int npass = MODE == AR_EVAL ? T : T - 1;
  int n_sched = 0;                       // prior prefix: scheduled steps so far (row of noise)
  for (int p = 0; p < npass; ++p) {
    const bool last_pass = MODE == AR_EVAL && post && p == T - 1;
    const int len = last_pass ? T : p + 1;
    if (MODE == AR_PRIOR_PREFIX) {
      if (!sched[p]) {                   // teacher step: z_{p+1} = z[p], no layer runs
        for (int e = tid; e < cz * BT; e += SV_THREADS) {
          const int j = e % BT;
          zs[(p + 1) * cz * BT + e] = (j < nb) ? zt[((long long)p * B + b0 + j) * cz + e / BT] : 0.0f;
        }
        __syncthreads();
        continue;
      }
      for (int e = tid; e < cz * BT; e += SV_THREADS) zs[(p + 1) * cz * BT + e] = 0.0f;   // spike counts of row p
      __syncthreads();
    }
    for (int s = 0; s < len; ++s) {
      // layer 1: input row s = [x_s, z_s]
      for (int o = tid; o < h1; o += SV_THREADS) {
        float acc[BT];
#pragma unroll
        for (int j = 0; j < BT; ++j) acc[j] = 0.0f;
        const float* wr = w1 + (long long)o * nin1;
        if (post) sv_dot<BT>(acc, xs + s * cx * BT, wr, cx);
        sv_dot<BT>(acc, zs + s * cz * BT, wr + cx, cz);
        const float bo = b1[o];
#pragma unroll
        for (int j = 0; j < BT; ++j) s1[o * BT + j] = sv_lif(v1[o * BT + j], acc[j] + bo) ? 1.0f : 0.0f;
      }
      __syncthreads();
      for (int o = tid; o < h2; o += SV_THREADS) {
        float acc[BT];
#pragma unroll
        for (int j = 0; j < BT; ++j) acc[j] = 0.0f;
        sv_dot<BT>(acc, s1, w2 + (long long)o * h1, h1);
        const float bo = b2[o];
#pragma unroll
        for (int j = 0; j < BT; ++j) s2[o * BT + j] = sv_lif(v2[o * BT + j], acc[j] + bo) ? 1.0f : 0.0f;
      }
      __syncthreads();
      const bool pick_row = last_pass || s == len - 1;
      const int irow = last_pass ? s : p;  // which draw of idx this row's pick uses
      for (int o = tid; o < h3; o += SV_THREADS) {
        float acc[BT];
#pragma unroll
        for (int j = 0; j < BT; ++j) acc[j] = 0.0f;
        sv_dot<BT>(acc, s2, w3 + (long long)o * h2, h2);
        const float bo = b3[o];
        const int c = o / k, r = o - c * k;
#pragma unroll
        for (int j = 0; j < BT; ++j) {
          const bool spk = sv_lif(v3[o * BT + j], acc[j] + bo);
          if (j >= nb) continue;
          if (MODE == AR_PRIOR_PREFIX) {   // count the last row's spikes per channel (integer-valued: exact in any order)
            if (s == len - 1 && spk) atomicAdd(&zs[((p + 1) * cz + c) * BT + j], 1.0f);
            continue;
          }
          const long long b = b0 + j;
          if (MODE == AR_EVAL && last_pass && qz) qz[((long long)s * B + b) * h3 + o] = spk ? 1 : 0;
          if (!pick_row || idx[((long long)irow * B + b) * cz + c] != r) continue;
          const float zv = spk ? 1.0f : 0.0f;
          if (last_pass) {
            zout[((long long)s * B + b) * cz + c] = zv;
          } else {
            zs[((p + 1) * cz + c) * BT + j] = zv;
            if (MODE == AR_EVAL && !post) zout[((long long)p * B + b) * cz + c] = zv;
          }
        }
      }
      __syncthreads();
    }
    if (MODE == AR_PRIOR_PREFIX) {       // prob1 = mean_k + 1e-3 * randn (fp32, as the reference), z = prob1 > 0.5
      for (int e = tid; e < cz * BT; e += SV_THREADS) {
        const int j = e % BT, c = e / BT;
        float* zc = &zs[(p + 1) * cz * BT + e];
        const float nz = (j < nb) ? noise[((long long)n_sched * B + b0 + j) * cz + c] : 0.0f;
        const float prob = *zc / (float)k + 0.001f * nz;
        *zc = (j < nb && prob > 0.5f) ? 1.0f : 0.0f;
      }
      ++n_sched;
      __syncthreads();
    }
  }

  if (MODE != AR_EVAL) {
    for (int e = tid; e < T * cz * BT; e += SV_THREADS) {
      const int j = e % BT, c = (e / BT) % cz, t = e / (BT * cz);
      if (j < nb) zout[((long long)t * B + b0 + j) * cz + c] = zs[e];
    }
  }

  for (int e = tid; e < h1 * BT; e += SV_THREADS) {
    const int j = e % BT;
    if (j < nb) v1g[(long long)(b0 + j) * h1 + e / BT] = v1[e];
  }
  for (int e = tid; e < h2 * BT; e += SV_THREADS) {
    const int j = e % BT;
    if (j < nb) v2g[(long long)(b0 + j) * h2 + e / BT] = v2[e];
  }
  for (int e = tid; e < h3 * BT; e += SV_THREADS) {
    const int j = e % BT;
    if (j < nb) v3g[(long long)(b0 + j) * h3 + e / BT] = v3[e];
  }
}

constexpr int SV_LIN_BT = 4;

int ar_tile(int B) { return B > 256 ? 4 : 1; }   // one image per workgroup while the grid does not exceed the CU count

long long ar_lds_bytes(int T, int B, int cx, int cz, int h1, int h2, int k) {
  return (long long)ar_layout(ar_tile(B), T, cx, cz, h1, h2, cz * k).total * (long long)sizeof(float);
}

}  // namespace

extern "C" int spk_linear_lif_fwd(const void* x, int in_kind, const float* w, const float* bias_or_null, float* v_inout_or_null,
                                  void* out_or_null, int out_kind, int T, int B, int in_features, int out_features, int ptc_c,
                                  int ptc_h, int ptc_w, hipStream_t stream) {
  if (!x || !w || T <= 0 || B <= 0 || in_features <= 0 || out_features <= 0) return SPK_ERR_ARG;
  if (in_kind < SPK_LIN_IN_F32 || in_kind > SPK_LIN_IN_PTC || out_kind < SPK_LIN_OUT_F32 || out_kind > SPK_LIN_OUT_PTC)
    return SPK_ERR_ARG;
  if (in_kind == SPK_LIN_IN_PTC && out_kind == SPK_LIN_OUT_PTC) return SPK_ERR_UNSUPPORTED;
  if (in_kind == SPK_LIN_IN_PTC || out_kind == SPK_LIN_OUT_PTC) {
    const long long n = (long long)ptc_c * ptc_h * ptc_w;
    if (ptc_c <= 0 || ptc_h <= 0 || ptc_w <= 0) return SPK_ERR_ARG;
    if (n != (in_kind == SPK_LIN_IN_PTC ? in_features : out_features)) return SPK_ERR_ARG;
  }
  if (out_kind != SPK_LIN_OUT_U8 && !out_or_null) return SPK_ERR_ARG;   // only LIF spikes may be dropped (state-only pass)
  if (out_kind != SPK_LIN_OUT_F32 && !v_inout_or_null) return SPK_ERR_ARG;
  const size_t lds = (size_t)in_features * SV_LIN_BT * sizeof(float);
  if (lds > SV_LDS_MAX) return SPK_ERR_UNSUPPORTED;
  const long long gy = (B + SV_LIN_BT - 1) / SV_LIN_BT;
  if (gy > 65535) return SPK_ERR_UNSUPPORTED;
  const dim3 grid((out_features + SV_THREADS - 1) / SV_THREADS, (unsigned)gy);
  hipLaunchKernelGGL(linear_lif_kernel<SV_LIN_BT>, grid, dim3(SV_THREADS), lds, stream, x, in_kind, w, bias_or_null,
                     v_inout_or_null, out_or_null, out_kind, T, B, in_features, out_features, ptc_c, ptc_h, ptc_w);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_svae_ar_fwd(const uint8_t* x_or_null, const float* z0, const float* w1, const float* b1, const float* w2,
                               const float* b2, const float* w3, const float* b3, float* v1_inout, float* v2_inout,
                               float* v3_inout, const int* idx, float* sampled_z_out, uint8_t* q_z_out_or_null, int T, int B,
                               int cx, int cz, int h1, int h2, int k, hipStream_t stream) {
  if (!z0 || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !v1_inout || !v2_inout || !v3_inout || !idx || !sampled_z_out)
    return SPK_ERR_ARG;
  if (T <= 0 || T > SPK_MAX_T || B <= 0 || cz <= 0 || h1 <= 0 || h2 <= 0 || k <= 0) return SPK_ERR_ARG;
  if ((x_or_null != nullptr) != (cx > 0) || cx < 0) return SPK_ERR_ARG;
  if (q_z_out_or_null && !x_or_null) return SPK_ERR_ARG;          // q_z belongs to the posterior
  const long long lds = ar_lds_bytes(T, B, cx, cz, h1, h2, k);
  if (lds > SV_LDS_MAX) return SPK_ERR_UNSUPPORTED;
  const int bt = ar_tile(B);
  const dim3 grid((B + bt - 1) / bt);
  if (bt == 4)
    hipLaunchKernelGGL((svae_ar_kernel<4, AR_EVAL>), grid, dim3(SV_THREADS), (size_t)lds, stream, x_or_null, z0, w1, b1, w2, b2,
                       w3, b3, v1_inout, v2_inout, v3_inout, idx, sampled_z_out, q_z_out_or_null, T, B, cx, cz, h1, h2, k,
                       nullptr, nullptr, nullptr);
  else
    hipLaunchKernelGGL((svae_ar_kernel<1, AR_EVAL>), grid, dim3(SV_THREADS), (size_t)lds, stream, x_or_null, z0, w1, b1, w2, b2,
                       w3, b3, v1_inout, v2_inout, v3_inout, idx, sampled_z_out, q_z_out_or_null, T, B, cx, cz, h1, h2, k,
                       nullptr, nullptr, nullptr);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_svae_ar_prefix_fwd(const uint8_t* x_or_null, const float* z0, const float* w1, const float* b1,
                                      const float* w2, const float* b2, const float* w3, const float* b3, float* v1_inout,
                                      float* v2_inout, float* v3_inout, const int* idx_or_null, const uint8_t* sched_or_null,
                                      const float* noise_or_null, const float* z_teacher_or_null, float* z_t_minus_out, int T,
                                      int B, int cx, int cz, int h1, int h2, int k, hipStream_t stream) {
  if (!z0 || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !v1_inout || !v2_inout || !v3_inout || !z_t_minus_out)
    return SPK_ERR_ARG;
  if (T < 2 || T > SPK_MAX_T || B <= 0 || cz <= 0 || h1 <= 0 || h2 <= 0 || k <= 0 || cx < 0) return SPK_ERR_ARG;
  const bool post = x_or_null != nullptr;
  if (post != (cx > 0)) return SPK_ERR_ARG;
  if (post && !idx_or_null) return SPK_ERR_ARG;                                                      // posterior: the draws
  if (!post && (!sched_or_null || !noise_or_null || !z_teacher_or_null)) return SPK_ERR_ARG;         // prior: the schedule
  const long long lds = ar_lds_bytes(T, B, cx, cz, h1, h2, k);
  if (lds > SV_LDS_MAX) return SPK_ERR_UNSUPPORTED;
  const int bt = ar_tile(B);
  const dim3 grid((B + bt - 1) / bt);
#define SV_PREFIX(BT, MODE)                                                                                               \
  hipLaunchKernelGGL((svae_ar_kernel<BT, MODE>), grid, dim3(SV_THREADS), (size_t)lds, stream, x_or_null, z0, w1, b1, w2, b2, \
                     w3, b3, v1_inout, v2_inout, v3_inout, idx_or_null, z_t_minus_out, nullptr, T, B, cx, cz, h1, h2, k,    \
                     sched_or_null, noise_or_null, z_teacher_or_null)
  if (post) { if (bt == 4) SV_PREFIX(4, AR_POST_PREFIX); else SV_PREFIX(1, AR_POST_PREFIX); }
  else      { if (bt == 4) SV_PREFIX(4, AR_PRIOR_PREFIX); else SV_PREFIX(1, AR_PRIOR_PREFIX); }
#undef SV_PREFIX
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
