// Training path of the SNN_VAE baseline's spiking MLP (R/snn_model/vae_model.py:198-546 in train() mode):
//   spk_linear_lif_train_fwd   multi-step Linear + the surrogate-gradient LIF forward (keeps h, the membrane before reset),
//                              or the Linear's plain currents (layer.Linear in training); optional second input for the
//                              posterior's [x | z_t_minus] concat
//   spk_linear_lif_train_bwd   LIF BPTT (spk_lif_train_bwd, lif_train.hip), then dX = dI W, dW = dI^T X and db = sum dI as
//                              tiled fp32 GEMMs
//   spk_svae_latent_loss_fwd/bwd  the posterior's idx gather (sampled_z) and the MMD loss mean((PSP(mean_k q) - PSP(mean_k p))^2)
//                              with its backward, fused
// (The no-grad prefix passes of the two Bernoulli loops are spk_svae_ar_prefix_fwd in svae.hip: they share its kernel.)
//
// Numerics: the forward sums are those of spk_linear_lif_fwd (fp32, ascending input index, then + bias; the concat's
// second input continues the same sum), so on dyadic weights spikes and h are exact.  Every reduction of the backward has
// a fixed order (one thread owns one output and walks K ascending; the loss is a fixed tree over fixed partials), so two
// identical calls give bitwise-equal results; there are no float atomics.
#include "spk_common.h"
#include "../../include/spkdiff.h"

extern "C" int spk_lif_train_bwd(const float* grad_spike_seq, const float* grad_v_last, const float* h_seq,
                                 float* grad_x_seq, float* grad_v_init, int T, long long N, float tau, float v_threshold,
                                 float v_reset, float alpha, int detach_reset, hipStream_t stream);

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_BT = 4;               // images per workgroup of the forward
constexpr int ST_LDS_MAX = 64 * 1024;

// One input of the forward / weight gradient: fp32 or u8 {0,1}, [M, n] row-major.
__device__ __forceinline__ float st_load(const void* p, int kind, long long off) {
  return kind == SPK_LIN_IN_U8 ? (reinterpret_cast<const uint8_t*>(p)[off] ? 1.0f : 0.0f) : reinterpret_cast<const float*>(p)[off];
}

// ------------------------------------------------------------------------------------------ forward
// Grid (ceil(out/256), ceil(B/BT)); thread = one output neuron for the BT images of its tile, v in registers over T.
__global__ __launch_bounds__(ST_THREADS) void linear_lif_train_fwd_kernel(
    const void* __restrict__ x1, int k1, int n1, const void* __restrict__ x2, int k2, int n2, const float* __restrict__ w,
    const float* __restrict__ bias, const float* __restrict__ v_init, float* __restrict__ out, float* __restrict__ h_seq,
    float* __restrict__ v_out, int lif, int T, int B, int nout) {
  extern __shared__ float s_act[];  // [nin][BT]
  const int nin = n1 + n2;
  const int o = blockIdx.x * ST_THREADS + threadIdx.x;
  const int b0 = blockIdx.y * ST_BT;
  const int nb = min(ST_BT, B - b0);
  const bool live = o < nout;
  float v[ST_BT];
#pragma unroll
  for (int j = 0; j < ST_BT; ++j) v[j] = (live && lif && v_init && j < nb) ? v_init[(long long)(b0 + j) * nout + o] : 0.0f;
  const float bo = (live && bias) ? bias[o] : 0.0f;
  for (int t = 0; t < T; ++t) {
    __syncthreads();
    for (int e = threadIdx.x; e < nin * ST_BT; e += ST_THREADS) {
      const int i = e / ST_BT, j = e - i * ST_BT;
      float val = 0.0f;
      if (j < nb) {
        const long long m = (long long)t * B + b0 + j;
        val = i < n1 ? st_load(x1, k1, m * n1 + i) : st_load(x2, k2, m * n2 + (i - n1));
      }
      s_act[e] = val;
    }
    __syncthreads();
    if (!live) continue;
    float acc[ST_BT];
#pragma unroll
    for (int j = 0; j < ST_BT; ++j) acc[j] = 0.0f;
    const float* wr = w + (long long)o * nin;
    for (int i = 0; i < nin; ++i) {
      const float wi = wr[i];
#pragma unroll
      for (int j = 0; j < ST_BT; ++j) acc[j] += s_act[i * ST_BT + j] * wi;
    }
#pragma unroll
    for (int j = 0; j < ST_BT; ++j) {
      if (j >= nb) break;
      const long long r = ((long long)t * B + b0 + j) * nout + o;
      const float cur = acc[j] + bo;
      if (!lif) {
        out[r] = cur;
        continue;
      }
      // the reference's charge / fire / hard reset (neuron.py:739-749, :133-135), v_reset 0, tau 2 (as spk_lif_step)
      const float h = v[j] + (cur - (v[j] - 0.0f)) * 0.5f;
      const bool s = h >= 1.0f;
      v[j] = s ? (0.0f + 0.0f * h) : (0.0f * 0.0f + h);
      h_seq[r] = h;
      out[r] = s ? 1.0f : 0.0f;
    }
  }
  if (live && lif) {
#pragma unroll
    for (int j = 0; j < ST_BT; ++j)
      if (j < nb) v_out[(long long)(b0 + j) * nout + o] = v[j];
  }
}

// ------------------------------------------------------------------------------------------ backward GEMMs
// C[r][c] = sum_{q < K} A(r, q) * B(q, c), q ascending, one thread per 4x4 outputs of a 64x64 tile (K staged 16 at a time).
//   DGRAD: r = row m of [T*B], c = input column i < ncol, q = output o:  A = dI[m][o], B = W[o][i]        -> dX[m][i]
//   WGRAD: r = output o, c = input column i <= nin (i == nin: the bias, B = 1), q = row m: A = dI[m][o], B = X[m][i]
//          -> dW[o][i], db[o]
constexpr int GT = 64, GK = 16;

template <bool WGRAD>
__global__ __launch_bounds__(ST_THREADS) void linear_grad_kernel(const float* __restrict__ dI, const float* __restrict__ w,
                                                                 const void* __restrict__ x1, int k1, int n1,
                                                                 const void* __restrict__ x2, int k2, int n2,
                                                                 float* __restrict__ c_out, int ldc, float* __restrict__ db,
                                                                 int R, int C, int K, int nout) {
  __shared__ float As[GK][GT + 1];
  __shared__ float Bs[GK][GT + 1];
  const int nin = n1 + n2;
  const int r0 = blockIdx.y * GT, c0 = blockIdx.x * GT;
  const int tr = threadIdx.x / 16, tc = threadIdx.x % 16;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
  for (int q0 = 0; q0 < K; q0 += GK) {
    for (int e = threadIdx.x; e < GK * GT; e += ST_THREADS) {
      int qq, rr;
      if (WGRAD) { rr = e % GT; qq = e / GT; }        // A(o, m) = dI[m][o]: consecutive o are consecutive addresses
      else       { qq = e % GK; rr = e / GK; }        // A(m, o) = dI[m][o]
      const int r = r0 + rr, q = q0 + qq;
      float a = 0.0f;
      if (r < R && q < K) a = WGRAD ? dI[(long long)q * nout + r] : dI[(long long)r * nout + q];
      As[qq][rr] = a;
    }
    for (int e = threadIdx.x; e < GK * GT; e += ST_THREADS) {
      const int cc = e % GT, qq = e / GT;
      const int c = c0 + cc, q = q0 + qq;
      float bv = 0.0f;
      if (c < C && q < K) {
        if (!WGRAD) bv = w[(long long)q * nin + c];
        else if (c == nin) bv = 1.0f;
        else bv = c < n1 ? st_load(x1, k1, (long long)q * n1 + c) : st_load(x2, k2, (long long)q * n2 + (c - n1));
      }
      Bs[qq][cc] = bv;
    }
    __syncthreads();
    const int qn = min(GK, K - q0);
    for (int qq = 0; qq < qn; ++qq) {
      float av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = As[qq][tr + 16 * a];
#pragma unroll
      for (int b = 0; b < 4; ++b) bv[b] = Bs[qq][tc + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] += av[a] * bv[b];
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int r = r0 + tr + 16 * a;
    if (r >= R) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int c = c0 + tc + 16 * b;
      if (c >= C) continue;
      if (WGRAD && c == nin) { if (db) db[r] = acc[a][b]; }
      else c_out[(long long)r * ldc + c] = acc[a][b];
    }
  }
}

// ------------------------------------------------------------------------------------------ latent loss
// Thread = one (b, c) column over the T steps.  PSP (snn_layers.PSP): syn_t = syn_{t-1} + (x_t - syn_{t-1}) / tau_s.
constexpr int LL_MAX_T = SPK_MAX_T;

__device__ __forceinline__ float ll_mean_k(const float* __restrict__ p, int k) {
  float s = 0.0f;
  for (int j = 0; j < k; ++j) s += p[j];
  return s / (float)k;
}

__global__ __launch_bounds__(ST_THREADS) void latent_loss_fwd_kernel(const float* __restrict__ q, const float* __restrict__ pz,
                                                                     const int* __restrict__ idx, float* __restrict__ sz,
                                                                     float* __restrict__ partial, int T, int B, int cz, int k,
                                                                     float tau_s) {
  __shared__ float red[ST_THREADS];
  const long long ncol = (long long)B * cz;
  const long long n = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  float acc = 0.0f;
  if (n < ncol) {
    float sq = 0.0f, sp = 0.0f;
    for (int t = 0; t < T; ++t) {
      const long long row = (long long)t * ncol + n;        // (t, b, c) with n = b*cz + c
      const float* qr = q + row * k;
      const int i = idx[row];
      if (sz) sz[row] = (i >= 0 && i < k) ? qr[i] : 0.0f;
      if (partial) {
        sq = sq + (ll_mean_k(qr, k) - sq) / tau_s;
        sp = sp + (ll_mean_k(pz + row * k, k) - sp) / tau_s;
        const float d = sq - sp;
        acc += d * d;
      }
    }
  }
  if (!partial) return;
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(ST_THREADS) void latent_loss_reduce_kernel(const float* __restrict__ partial, int n,
                                                                        float* __restrict__ loss, float inv_count) {
  __shared__ float red[ST_THREADS];
  float acc = 0.0f;
  for (int i = threadIdx.x; i < n; i += ST_THREADS) acc += partial[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = red[0] * inv_count;
}

// dL/dq[t,b,c,j] = PSP^T(2 d g / N)_t / k + [j == idx] dL/dsampled_z[t,b,c];  dL/dp = -PSP^T(2 d g / N)_t / k.
__global__ __launch_bounds__(ST_THREADS) void latent_loss_bwd_kernel(const float* __restrict__ q, const float* __restrict__ pz,
                                                                     const int* __restrict__ idx, const float* __restrict__ g_loss,
                                                                     const float* __restrict__ g_sz, float* __restrict__ gq,
                                                                     float* __restrict__ gp, int T, int B, int cz, int k,
                                                                     float tau_s) {
  const long long ncol = (long long)B * cz;
  const long long n = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (n >= ncol) return;
  float d[LL_MAX_T];
  const bool mmd = pz != nullptr && g_loss != nullptr;
  const float g = mmd ? *g_loss * 2.0f / (float)((long long)T * ncol) : 0.0f;
  if (mmd) {
    float sq = 0.0f, sp = 0.0f;
#pragma unroll
    for (int t = 0; t < LL_MAX_T; ++t) {
      if (t >= T) break;
      const long long row = (long long)t * ncol + n;
      sq = sq + (ll_mean_k(q + row * k, k) - sq) / tau_s;
      sp = sp + (ll_mean_k(pz + row * k, k) - sp) / tau_s;
      d[t] = sq - sp;
    }
  }
  const float carry = 1.0f - 1.0f / tau_s;
  float G = 0.0f;
  for (int t = T - 1; t >= 0; --t) {
    const long long row = (long long)t * ncol + n;
    float gx = 0.0f;
    if (mmd) {
      G = g * d[t] + carry * G;
      gx = G / tau_s / (float)k;
    }
    const int i = idx[row];
    const float gs = g_sz ? g_sz[row] : 0.0f;
    for (int j = 0; j < k; ++j) {
      gq[row * k + j] = gx + (j == i ? gs : 0.0f);
      if (gp) gp[row * k + j] = -gx;
    }
  }
}

int ll_blocks(int B, int cz) { return (int)(((long long)B * cz + ST_THREADS - 1) / ST_THREADS); }

bool lin_kind_ok(int k) { return k == SPK_LIN_IN_F32 || k == SPK_LIN_IN_U8; }

}  // namespace

extern "C" int spk_linear_lif_train_fwd(const void* x, int x_kind, int x_features, const void* x2_or_null, int x2_kind,
                                        int x2_features, const float* w, const float* bias_or_null,
                                        const float* v_init_or_null, float* out, float* h_seq_or_null, float* v_out_or_null,
                                        int lif, int T, int B, int out_features, hipStream_t stream) {
  if (!x || !w || !out || T <= 0 || B <= 0 || x_features <= 0 || out_features <= 0 || x2_features < 0) return SPK_ERR_ARG;
  if (!lin_kind_ok(x_kind) || (x2_or_null && !lin_kind_ok(x2_kind))) return SPK_ERR_ARG;
  if ((x2_or_null != nullptr) != (x2_features > 0)) return SPK_ERR_ARG;
  if (lif != 0 && lif != 1) return SPK_ERR_ARG;
  if (lif && (!h_seq_or_null || !v_out_or_null)) return SPK_ERR_ARG;
  const long long nin = (long long)x_features + x2_features;
  const size_t lds = (size_t)nin * ST_BT * sizeof(float);
  if (lds > ST_LDS_MAX) return SPK_ERR_UNSUPPORTED;
  const long long gy = (B + ST_BT - 1) / ST_BT;
  if (gy > 65535) return SPK_ERR_UNSUPPORTED;
  const dim3 grid((out_features + ST_THREADS - 1) / ST_THREADS, (unsigned)gy);
  hipLaunchKernelGGL(linear_lif_train_fwd_kernel, grid, dim3(ST_THREADS), lds, stream, x, x_kind, x_features, x2_or_null,
                     x2_kind, x2_features, w, bias_or_null, v_init_or_null, out, h_seq_or_null, v_out_or_null, lif, T, B,
                     out_features);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_linear_lif_train_bwd(const float* grad_out, const float* h_seq_or_null, float* dI_ws_or_null,
                                        const void* x, int x_kind, int x_features, const void* x2_or_null, int x2_kind,
                                        int x2_features, const float* w, float* grad_x_or_null, int grad_x_cols,
                                        float* grad_w, float* grad_b_or_null, int T, int B, int out_features,
                                        hipStream_t stream) {
  if (!grad_out || !x || !w || !grad_w || T <= 0 || B <= 0 || x_features <= 0 || out_features <= 0 || x2_features < 0)
    return SPK_ERR_ARG;
  if (!lin_kind_ok(x_kind) || (x2_or_null && !lin_kind_ok(x2_kind))) return SPK_ERR_ARG;
  if ((x2_or_null != nullptr) != (x2_features > 0)) return SPK_ERR_ARG;
  const int nin = x_features + x2_features;
  if (grad_x_or_null && (grad_x_cols <= 0 || grad_x_cols > nin)) return SPK_ERR_ARG;
  if (h_seq_or_null && !dI_ws_or_null) return SPK_ERR_ARG;     // LIF mode: the current gradient needs a buffer
  const long long M = (long long)T * B;
  if (M > 0x7fffffffLL || (M + GT - 1) / GT > 65535) return SPK_ERR_UNSUPPORTED;
  const float* dI = grad_out;                                  // plain currents: dL/dI is the incoming gradient
  if (h_seq_or_null) {
    // BPTT of the default LIFNode (tau 2, v_th 1, v_reset 0, ATan alpha 2, detach_reset False); v_init carries no gradient
    const int rc = spk_lif_train_bwd(grad_out, nullptr, h_seq_or_null, dI_ws_or_null, nullptr, T, (long long)B * out_features, 2.0f,
                                     1.0f, 0.0f, 2.0f, 0, stream);
    if (rc != SPK_OK) return rc;
    dI = dI_ws_or_null;
  }
  if (grad_x_or_null) {
    const dim3 grid((grad_x_cols + GT - 1) / GT, (unsigned)((M + GT - 1) / GT));
    hipLaunchKernelGGL(linear_grad_kernel<false>, grid, dim3(ST_THREADS), 0, stream, dI, w, x, x_kind, x_features, x2_or_null,
                       x2_kind, x2_features, grad_x_or_null, grad_x_cols, nullptr, (int)M, grad_x_cols, out_features,
                       out_features);
    SPK_LAUNCH_CHECK();
  }
  const int C = nin + (grad_b_or_null ? 1 : 0);
  const dim3 grid((C + GT - 1) / GT, (out_features + GT - 1) / GT);
  hipLaunchKernelGGL(linear_grad_kernel<true>, grid, dim3(ST_THREADS), 0, stream, dI, w, x, x_kind, x_features, x2_or_null,
                     x2_kind, x2_features, grad_w, nin, grad_b_or_null, out_features, C, (int)M, out_features);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_svae_latent_loss_ws_floats(int B, int cz) {
  if (B <= 0 || cz <= 0) return SPK_ERR_ARG;
  return ll_blocks(B, cz);
}

extern "C" int spk_svae_latent_loss_fwd(const float* q_z, const float* p_z_or_null, const int* idx, float* sampled_z_or_null,
                                        float* loss_or_null, float* ws, int T, int B, int cz, int k, float tau_s,
                                        hipStream_t stream) {
  if (!q_z || !idx || T <= 0 || T > LL_MAX_T || B <= 0 || cz <= 0 || k <= 0 || !(tau_s > 0.f)) return SPK_ERR_ARG;
  if ((p_z_or_null != nullptr) != (loss_or_null != nullptr)) return SPK_ERR_ARG;
  if (loss_or_null && !ws) return SPK_ERR_ARG;
  if (!sampled_z_or_null && !loss_or_null) return SPK_ERR_ARG;
  const int nblk = ll_blocks(B, cz);
  hipLaunchKernelGGL(latent_loss_fwd_kernel, dim3(nblk), dim3(ST_THREADS), 0, stream, q_z, p_z_or_null, idx, sampled_z_or_null,
                     loss_or_null ? ws : nullptr, T, B, cz, k, tau_s);
  SPK_LAUNCH_CHECK();
  if (loss_or_null) {
    hipLaunchKernelGGL(latent_loss_reduce_kernel, dim3(1), dim3(ST_THREADS), 0, stream, ws, nblk, loss_or_null,
                       1.0f / (float)((long long)T * B * cz));
    SPK_LAUNCH_CHECK();
  }
  return SPK_OK;
}

extern "C" int spk_svae_latent_loss_bwd(const float* q_z, const float* p_z_or_null, const int* idx, const float* g_loss_or_null,
                                        const float* g_sampled_z_or_null, float* grad_q_z, float* grad_p_z_or_null, int T,
                                        int B, int cz, int k, float tau_s, hipStream_t stream) {
  if (!q_z || !idx || !grad_q_z || T <= 0 || T > LL_MAX_T || B <= 0 || cz <= 0 || k <= 0 || !(tau_s > 0.f))
    return SPK_ERR_ARG;
  if (g_loss_or_null && !p_z_or_null) return SPK_ERR_ARG;
  if (grad_p_z_or_null && !p_z_or_null) return SPK_ERR_ARG;
  hipLaunchKernelGGL(latent_loss_bwd_kernel, dim3(ll_blocks(B, cz)), dim3(ST_THREADS), 0, stream, q_z, p_z_or_null, idx,
                     g_loss_or_null, g_sampled_z_or_null, grad_q_z, grad_p_z_or_null, T, B, cz, k, tau_s);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
