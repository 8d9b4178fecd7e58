// Training branch of the plain-CNN VQVAE baseline (R/snn_model/vae_model.py:575-591 CNN_VectorQuantizer.forward, :660-672
// VQVAE.forward; main.py --model vq-vae in train() mode): the time-free vector quantiser and the mean-squared-error loss, forward
// and backward, on channels-last fp32 tensors.  The six convolutions around them are csrc/conv_train.hip's.
//   idx  = argmin_k |z - e_k|^2                         (vq_argmin.h: fp64 distances x2 + e2 - 2 dot on the fp32 z, spk_vq_argmin's order)
//   q    = E[idx];  e = z + (q - z)                     (the straight-through value: two fp32 roundings, not q)
//   loss = m + beta * m,  m = mean((q - z)^2)           (q_latent_loss + commitment_cost * e_latent_loss: both have this value)
//   g_z  = g_e + g_loss * beta * 2 (z - q) / (N D)
//   g_E[k] = g_loss * 2 / (N D) * sum over the rows with idx = k, ascending, of (q - z)
//   mse  = mean((x_recon - x)^2);  recon_loss = mse / data_variance;  g_x_recon = (g_recon / data_variance + g_real) * 2 (x_recon - x) / n
// fp32 element-wise arithmetic in the reference's order (-ffp-contract=off).  The mean squares are fp64 sums whose shape depends
// on the sizes alone -- one partial per row (VQ) or per AT_CHUNK elements (loss), each formed in a fixed order, and a
// single-workgroup launch that adds the partials in index order -- so a result depends neither on the grid nor on timing.  No
// atomics; the workspace carries no state from call to call.
#include "spk_common.h"
#include "vq_argmin.h"
#include "../../include/spkdiff.h"

namespace {

constexpr int AT_MAX_D = SPK_VQ_TRAIN_MAX_D;
constexpr int AT_CHUNK = SPK_ANN_VQVAE_TRAIN_CHUNK;                // elements per partial of the loss (256 threads x 8)
constexpr int AT_VQ_GRID = 2048, AT_EW_GRID = 1024, AT_LOSS_GRID = 1024;

// the 256 values of a workgroup added in a fixed order (a tree over the thread index); the sum arrives in thread 0
__device__ __forceinline__ double at_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// A wave per row, a lane per code (64 at a time), the codebook and its squared norms in LDS: vq_kernel's arithmetic (vq.hip).
// DC > 0: D == DC at compile time (the row sits in DC scalar-broadcast registers).
template <int DC>
__global__ __launch_bounds__(256) void ann_vq_fwd_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                         long long* __restrict__ idx_out, float* __restrict__ e_out,
                                                         double* __restrict__ row_part, long long N, int D_rt, int K) {
  const int D = DC > 0 ? DC : D_rt;
  extern __shared__ float lds[];
  float* s_cb = lds;                                               // [K][D + 1]
  double* s_e2 = reinterpret_cast<double*>(s_cb + ((K * (D + 1) + 1) & ~1));   // [K]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < K * D; i += blockDim.x) s_cb[(i / D) * (D + 1) + (i % D)] = cb[i];
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    double e2 = 0.0;
    for (int d = 0; d < D; ++d) { const double e = s_cb[k * (D + 1) + d]; e2 = fma(e, e, e2); }
    s_e2[k] = e2;
  }
  __syncthreads();
  for (long long p = (long long)blockIdx.x * 4 + wave; p < N; p += (long long)gridDim.x * 4) {
    const float xl = lane < D ? z[p * D + lane] : 0.f;             // lane d < D holds z[p][d]
    double best = __builtin_inf();
    int besti = VQ_NONE;
    double x2 = 0.0;
    // (products of two fp32 values are exact in fp64: fma(a, b, s) == s + a * b bit for bit)
    if constexpr (DC > 0) {
      double xr[DC];
#pragma unroll
      for (int d = 0; d < DC; ++d) { xr[d] = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(xl), d)); x2 = fma(xr[d], xr[d], x2); }
      for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const int kc = k < K ? k : K - 1;
        double dot = 0.0;
#pragma unroll
        for (int d = 0; d < DC; ++d) dot = fma(xr[d], (double)s_cb[kc * (DC + 1) + d], dot);
        const double dist = x2 + s_e2[kc] - 2.0 * dot;
        if (k < K && vq_lane_takes(dist, best)) { best = dist; besti = k; }
      }
    } else {
      for (int d = 0; d < D; ++d) { const double xv = (double)__shfl(xl, d); x2 = fma(xv, xv, x2); }
      for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const int kc = k < K ? k : K - 1;
        double dot = 0.0;
        for (int d = 0; d < D; ++d) dot = fma((double)__shfl(xl, d), (double)s_cb[kc * (D + 1) + d], dot);
        const double dist = x2 + s_e2[kc] - 2.0 * dot;
        if (k < K && vq_lane_takes(dist, best)) { best = dist; besti = k; }
      }
    }
    vq_wave_combine(best, besti);
    besti = vq_index(besti);
    double sq = 0.0;
    if (lane < D) {
      const float q = s_cb[besti * (D + 1) + lane];
      const float df = q - xl;
      e_out[p * D + lane] = xl + df;                               // z + (q - z)
      sq = (double)(df * df);
    }
    // the row's sum of squares: a butterfly over the lanes (the same order for every row)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
    if (lane == 0) { idx_out[p] = (long long)besti; row_part[p] = sq; }
  }
}

// adds n partials in a fixed order (thread t: t, t + 256, ...; then the tree) and writes the loss values.
// MODE 0: out0[0] = m + beta * m.  MODE 1: out0[0] = m / dv[0] (recon_loss), out1[0] = m (real_loss_rec); m = (float)(sum / count).
template <int MODE>
__global__ __launch_bounds__(256) void ann_mean_kernel(const double* __restrict__ part, long long n, double count, float beta,
                                                       const float* __restrict__ dv, float* __restrict__ out0,
                                                       float* __restrict__ out1) {
  __shared__ double red[256];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) s += part[i];
  const double tot = at_block_sum(s, red);
  if (threadIdx.x == 0) {
    const float m = (float)(tot / count);
    if (MODE == 0) out0[0] = m + beta * m;
    else { out0[0] = m / dv[0]; out1[0] = m; }
  }
}

// blocks [0, nb_x): g_z, element-wise; blocks [nb_x, nb_x + K): one codebook row each.  A code's rows are found 256 at a time
// (an ordered compaction through LDS), their differences fetched 256 / D rows at a time by all threads, and added by D threads
// in ascending row order.
__global__ __launch_bounds__(256) void ann_vq_bwd_kernel(const float* __restrict__ g_e, const float* __restrict__ gloss,
                                                         const float* __restrict__ z, const long long* __restrict__ idx,
                                                         const float* __restrict__ E, float beta, float* __restrict__ gz,
                                                         float* __restrict__ gE, int nb_x, long long N, int D, int K) {
  const float gl = gloss ? gloss[0] : 0.f;
  const long long total = N * D;
  const float inv = 2.0f / (float)total;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= nb_x) {
    __shared__ int s_list[256];
    __shared__ int s_wcnt[4];
    __shared__ float s_val[256];
    const int k = (int)blockIdx.x - nb_x, lane = tid & 63, wave = tid >> 6;
    const int RL = 256 / D, d = tid % D, rl = tid / D;             // RL rows are fetched at a time, D values each (D <= 64: RL >= 4)
    const float ek = E[(long long)k * D + d];
    double acc = 0.0;                                              // (threads tid < D: element tid of the row's sum)
    for (long long r0 = 0; r0 < N; r0 += 256) {
      const long long r = r0 + tid;
      const bool m = r < N && idx[r] == (long long)k;
      const unsigned long long b = __ballot(m);
      if (lane == 0) s_wcnt[wave] = __popcll(b);
      __syncthreads();
      int base = 0, cnt = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) { base += w < wave ? s_wcnt[w] : 0; cnt += s_wcnt[w]; }
      if (m) s_list[base + __popcll(b & ((1ull << lane) - 1ull))] = tid;
      __syncthreads();
      // the chunk's rows of this code, ascending: every thread fetches one difference, then D threads add them in row order
      for (int j0 = 0; j0 < cnt; j0 += RL) {
        if (rl < RL && j0 + rl < cnt) s_val[rl * D + d] = ek - z[(r0 + s_list[j0 + rl]) * D + d];
        __syncthreads();
        if (tid < D) {
          const int nj = cnt - j0 < RL ? cnt - j0 : RL;
          for (int j = 0; j < nj; ++j) acc += (double)s_val[j * D + tid];
        }
        __syncthreads();
      }
    }
    if (tid < D) gE[(long long)k * D + tid] = gl * inv * (float)acc;
    return;
  }
  const float c = gl * beta * inv;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < total; i += (long long)nb_x * 256) {
    const long long row = i / D;
    const int d = (int)(i - row * D);
    const float v = z[i], q = E[idx[row] * D + d];
    const float t = c * (v - q);
    gz[i] = g_e ? g_e[i] + t : t;
  }
}

// element i of the channels-last x_recon [B][H][W][C] and its partner in the NCHW image
__device__ __forceinline__ long long at_nchw_index(long long i, int C, int HW) {
  if (C == 1) return i;
  const int c = (int)(i % C);
  const long long pos = i / C, b = pos / HW, p = pos - b * HW;
  return (b * C + c) * HW + p;
}

// chunk ch = elements [ch * AT_CHUNK, (ch + 1) * AT_CHUNK): thread t adds ch * AT_CHUNK + t + 256 * j, j ascending, then the tree
__global__ __launch_bounds__(256) void ann_loss_fwd_kernel(const float* __restrict__ xr, const float* __restrict__ x,
                                                           double* __restrict__ part, long long n, long long nchunk, int C, int HW) {
  __shared__ double red[256];
  for (long long ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < AT_CHUNK / 256; ++j) {
      const long long i = ch * AT_CHUNK + threadIdx.x + 256 * j;
      if (i < n) {
        const float d = xr[i] - x[at_nchw_index(i, C, HW)];
        s += (double)(d * d);
      }
    }
    const double tot = at_block_sum(s, red);
    if (threadIdx.x == 0) part[ch] = tot;
    __syncthreads();                                               // (red is written again by the next chunk)
  }
}

__global__ __launch_bounds__(256) void ann_loss_bwd_kernel(const float* __restrict__ xr, const float* __restrict__ x,
                                                           const float* __restrict__ g_recon, const float* __restrict__ g_real,
                                                           const float* __restrict__ dv, float* __restrict__ gxr, long long n, int C,
                                                           int HW) {
  const float s = (g_recon ? g_recon[0] / dv[0] : 0.f) + (g_real ? g_real[0] : 0.f);
  const float c = s * (2.0f / (float)n);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    gxr[i] = c * (xr[i] - x[at_nchw_index(i, C, HW)]);
}

size_t at_vq_lds(int D, int K) { return (size_t)(((K * (D + 1) + 1) & ~1)) * sizeof(float) + (size_t)K * sizeof(double); }

long long at_chunks(long long elems) { return (elems + AT_CHUNK - 1) / AT_CHUNK; }

}  // namespace

extern "C" int spk_ann_vqvae_train_supported(int D, int K) {
  return D >= 1 && D <= AT_MAX_D && K >= 1 && K <= (1 << 20) && at_vq_lds(D, K) <= 64 * 1024;
}

extern "C" long long spk_ann_vqvae_train_ws_bytes(long long rows, long long elems) {
  if (rows < 0 || elems < 0) return SPK_ERR_ARG;
  const long long c = at_chunks(elems);
  const long long n = rows > c ? rows : c;
  return (n > 0 ? n : 1) * (long long)sizeof(double);
}

extern "C" int spk_ann_vqvae_train_vq_fwd(const float* z, const float* codebook, long long* idx_out, float* e_out, float* loss_out,
                                          float beta, void* ws, long long ws_bytes, long long N, int D, int K, spk_stream_t stream) {
  if (!z || !codebook || !idx_out || !e_out || !loss_out || !ws || N <= 0 || N > 0x7fffffff || D <= 0 || K <= 0 ||
      (reinterpret_cast<uintptr_t>(ws) & 7) != 0 || ws_bytes < spk_ann_vqvae_train_ws_bytes(N, 0))
    return SPK_ERR_ARG;
  if (!spk_ann_vqvae_train_supported(D, K)) return SPK_ERR_UNSUPPORTED;
  const size_t lds = at_vq_lds(D, K);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(ws);
  long long g = (N + 3) / 4;
  const int grid = (int)(g > AT_VQ_GRID ? AT_VQ_GRID : g);
  if (D == 16) hipLaunchKernelGGL(ann_vq_fwd_kernel<16>, dim3(grid), dim3(256), lds, s, z, codebook, idx_out, e_out, part, N, D, K);
  else hipLaunchKernelGGL(ann_vq_fwd_kernel<0>, dim3(grid), dim3(256), lds, s, z, codebook, idx_out, e_out, part, N, D, K);
  SPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(ann_mean_kernel<0>, dim3(1), dim3(256), 0, s, part, N, (double)N * (double)D, beta, (const float*)nullptr, loss_out,
                     (float*)nullptr);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_ann_vqvae_train_vq_bwd(const float* g_e_or_null, const float* g_loss_or_null, const float* z, const long long* idx,
                                          const float* codebook, float beta, float* gz_out, float* gcodebook_out, long long N, int D,
                                          int K, spk_stream_t stream) {
  if (!z || !idx || !codebook || !gz_out || !gcodebook_out || N <= 0 || N > 0x7fffffff || D <= 0 || K <= 0) return SPK_ERR_ARG;
  if (D > AT_MAX_D || K > (1 << 20)) return SPK_ERR_UNSUPPORTED;
  const int nb_x = spk_grid(N * D, AT_EW_GRID);
  hipLaunchKernelGGL(ann_vq_bwd_kernel, dim3(nb_x + K), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g_e_or_null,
                     g_loss_or_null, z, idx, codebook, beta, gz_out, gcodebook_out, nb_x, N, D, K);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_ann_vqvae_train_loss_fwd(const float* x_recon_cl, const float* x_nchw, const float* data_variance,
                                            float* recon_out, float* real_out, void* ws, long long ws_bytes, int B, int C, int H,
                                            int W, spk_stream_t stream) {
  if (!x_recon_cl || !x_nchw || !data_variance || !recon_out || !real_out || !ws || B <= 0 || C <= 0 || H <= 0 || W <= 0 ||
      (reinterpret_cast<uintptr_t>(ws) & 7) != 0)
    return SPK_ERR_ARG;
  const long long n = (long long)B * C * H * W;
  if ((long long)H * W > 0x7fffffff) return SPK_ERR_UNSUPPORTED;
  if (ws_bytes < spk_ann_vqvae_train_ws_bytes(0, n)) return SPK_ERR_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(ws);
  const long long nchunk = at_chunks(n);
  const int grid = (int)(nchunk > AT_LOSS_GRID ? AT_LOSS_GRID : nchunk);
  hipLaunchKernelGGL(ann_loss_fwd_kernel, dim3(grid), dim3(256), 0, s, x_recon_cl, x_nchw, part, n, nchunk, C, H * W);
  SPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(ann_mean_kernel<1>, dim3(1), dim3(256), 0, s, part, nchunk, (double)n, 0.f, data_variance, recon_out, real_out);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_ann_vqvae_train_loss_bwd(const float* x_recon_cl, const float* x_nchw, const float* g_recon_or_null,
                                            const float* g_real_or_null, const float* data_variance, float* gx_recon_cl, int B, int C,
                                            int H, int W, spk_stream_t stream) {
  if (!x_recon_cl || !x_nchw || !data_variance || !gx_recon_cl || B <= 0 || C <= 0 || H <= 0 || W <= 0) return SPK_ERR_ARG;
  if ((long long)H * W > 0x7fffffff) return SPK_ERR_UNSUPPORTED;
  const long long n = (long long)B * C * H * W;
  hipLaunchKernelGGL(ann_loss_bwd_kernel, dim3(spk_grid(n, AT_EW_GRID)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     x_recon_cl, x_nchw, g_recon_or_null, g_real_or_null, data_variance, gx_recon_cl, n, C, H * W);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
