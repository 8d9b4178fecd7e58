// Reconstruction metrics of R/main.py:318-320: SSIM (R/metric/pytorch_ssim/__init__.py:17-39, the five depthwise window
// convolutions, ~15 element-wise launches and the mean) and the squared error of F.mse_loss, as one launch with fp64 arithmetic:
//   mu1 = sum_w w a, mu2 = sum_w w b, s11 = sum_w w a^2, s22 = sum_w w b^2, s12 = sum_w w a b   (zero padding ws / 2, direct 2-D window)
//   map = ((2 mu1 mu2 + C1)(2 (s12 - mu1 mu2) + C2)) / ((mu1^2 + mu2^2 + C1)((s11 - mu1^2) + (s22 - mu2^2) + C2))
//   ssim_sum[n] = sum of map over (C, H', W'),  sq_sum[n] = sum of (a - b)^2 over (C, H, W);  H' = H + 2 (ws / 2) - ws + 1.
// The fp32 inputs and the fp32 window values are widened to fp64; a^2, b^2 and a b are exact there, so the only roundings are
// those of the window sums, the map and the reductions (the fp32 form cancels in s11 - mu1^2 next to the 9e-4 of C2).
// One work item = one 32x32 tile of one output plane: both planes' tile + halo staged in LDS as fp32, each thread sums its
// outputs in ascending order, the workgroup an LDS tree.  An image of one item (C = 1 and a map of at most 32x32: the 28x28
// batches of main.py) is finished there; otherwise the item's two partials go to the workspace and a second small launch adds
// each image's partials in item order.  No floating-point atomics and no hand-off between workgroups: the result does not
// depend on the order workgroups run in.
#include <limits.h>

#include "spk_common.h"
#include "../../include/spkdiff.h"

namespace {

constexpr int SS_THREADS = 256, SS_TILE = 32, SS_MAX_WS = SPK_SSIM_MAX_WINDOW;
constexpr int SS_SPAN = SS_TILE + SS_MAX_WS - 1;                 // 62: tile + halo, per side
constexpr int SS_W_DOUBLES = SS_MAX_WS * SS_MAX_WS;              // 961 window values (fp64)
constexpr int SS_TILE_FLOATS = SS_SPAN * SS_SPAN;                // 3844 per image
constexpr unsigned SS_MAX_BLOCKS = 1u << 20;                     // work beyond that is walked with a grid stride
constexpr int SS_THREAD_PER_IMAGE_PARTS = 32;                    // second launch: one thread per image up to this many partials, else a wave

// Inputs are read and results written at agent scope (sc1 loads past, sc1 stores through, the XCD's L2), so that the values do
// not depend on the cache maintenance of the launch that carries the kernel (replays of a captured graph).
__device__ __forceinline__ float ss_ld(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ss_ld(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ss_st(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// WS > 0: the window size as a constant (the reference's default 11); WS = 0: ws_rt.  part = NULL: one item per image.
template <int WS>
__global__ __launch_bounds__(SS_THREADS) void ssim_mse_kernel(const float* img1, const float* img2, const float* window, int H,
                                                              int W, int ws_rt, int Ho, int Wo, int tiles_x, int tiles,
                                                              unsigned items, double* part, double* ssim_out, double* sq_out) {
  // the one LDS array of the kernel: window (fp64), both tiles (fp32); the tile area is reused by the reduction
  __shared__ double lds[SS_W_DOUBLES + SS_TILE_FLOATS];
  double* sw = lds;
  float* sa = reinterpret_cast<float*>(lds + SS_W_DOUBLES);
  float* sb = sa + SS_TILE_FLOATS;
  double* red = lds + SS_W_DOUBLES;                              // [2][256] after the item's last tile read
  const int ws = WS ? WS : ws_rt;
  const int tid = threadIdx.x, pad = ws / 2;
  const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;

  for (int i = tid; i < ws * ws; i += SS_THREADS) sw[i] = (double)ss_ld(window + i);

  for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
    const int tile = (int)(item % (unsigned)tiles);
    const size_t plane = item / (unsigned)tiles;
    const int ty0 = (tile / tiles_x) * SS_TILE, tx0 = (tile % tiles_x) * SS_TILE;
    const int th = Ho - ty0 < SS_TILE ? Ho - ty0 : SS_TILE, tw = Wo - tx0 < SS_TILE ? Wo - tx0 : SS_TILE;
    const int span_h = th + ws - 1, span_w = tw + ws - 1;        // <= SS_SPAN
    const float* p1 = img1 + plane * (size_t)H * W;
    const float* p2 = img2 + plane * (size_t)H * W;
    __syncthreads();                                             // the previous item's reduction has left the tile area
    for (int i = tid; i < span_h * span_w; i += SS_THREADS) {
      const int r = i / span_w, c = i - r * span_w;
      const int y = ty0 + r - pad, x = tx0 + c - pad;
      const bool in = y >= 0 && y < H && x >= 0 && x < W;
      sa[i] = in ? ss_ld(p1 + (size_t)y * W + x) : 0.f;
      sb[i] = in ? ss_ld(p2 + (size_t)y * W + x) : 0.f;
    }
    __syncthreads();
    double acc_s = 0.0, acc_q = 0.0;
    for (int o = tid; o < th * tw; o += SS_THREADS) {
      const int oy = o / tw, ox = o - oy * tw;
      double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
      for (int dy = 0; dy < ws; ++dy) {
        const float* ra = sa + (oy + dy) * span_w + ox;
        const float* rb = sb + (oy + dy) * span_w + ox;
        const double* wr = sw + dy * ws;
#pragma unroll
        for (int dx = 0; dx < ws; ++dx) {
          const double a = (double)ra[dx], b = (double)rb[dx], w = wr[dx];
          m1 = fma(w, a, m1);
          m2 = fma(w, b, m2);
          s11 = fma(w, a * a, s11);
          s22 = fma(w, b * b, s22);
          s12 = fma(w, a * b, s12);
        }
      }
      const double mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu12 = m1 * m2;
      const double sig1 = s11 - mu1_sq, sig2 = s22 - mu2_sq, sig12 = s12 - mu12;
      acc_s += ((2.0 * mu12 + C1) * (2.0 * sig12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sig1 + sig2 + C2));
      if (ty0 + oy < H && tx0 + ox < W) {                        // this output's own pixel (H' >= H, W' >= W: every pixel once)
        const int c = (oy + pad) * span_w + ox + pad;
        const double d = (double)sa[c] - (double)sb[c];
        acc_q += d * d;
      }
    }
    __syncthreads();
    red[tid] = acc_s;
    red[SS_THREADS + tid] = acc_q;
    __syncthreads();
    for (int s = SS_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) {
        red[tid] += red[tid + s];
        red[SS_THREADS + tid] += red[SS_THREADS + tid + s];
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (part) {
        ss_st(part + 2 * (size_t)item, red[0]);
        ss_st(part + 2 * (size_t)item + 1, red[SS_THREADS]);
      } else {
        ss_st(ssim_out + item, red[0]);
        ss_st(sq_out + item, red[SS_THREADS]);
      }
    }
  }
}

// each image's partials in item order: one thread per image up to SS_THREAD_PER_IMAGE_PARTS partials, else one wave
__global__ __launch_bounds__(SS_THREADS) void ssim_mse_sum_kernel(const double* part, int N, long long parts, double* ssim_out,
                                                                  double* sq_out) {
  const int tid = threadIdx.x;
  if (parts <= SS_THREAD_PER_IMAGE_PARTS) {
    for (long long n = (long long)blockIdx.x * SS_THREADS + tid; n < N; n += (long long)gridDim.x * SS_THREADS) {
      const double* p = part + 2 * (size_t)n * parts;
      double s = 0.0, q = 0.0;
      for (int k = 0; k < (int)parts; ++k) {
        s += ss_ld(p + 2 * k);
        q += ss_ld(p + 2 * k + 1);
      }
      ss_st(ssim_out + n, s);
      ss_st(sq_out + n, q);
    }
  } else {
    constexpr int WAVES = SS_THREADS / 64;
    const int lane = tid & 63;
    for (long long n = (long long)blockIdx.x * WAVES + (tid >> 6); n < N; n += (long long)gridDim.x * WAVES) {   // wave-uniform
      const double* p = part + 2 * (size_t)n * parts;
      double s = 0.0, q = 0.0;
      for (long long k = lane; k < parts; k += 64) {
        s += ss_ld(p + 2 * k);
        q += ss_ld(p + 2 * k + 1);
      }
      for (int off = 32; off > 0; off >>= 1) {                   // butterfly: both partners add the same two values
        s += __shfl_xor(s, off, 64);
        q += __shfl_xor(q, off, 64);
      }
      if (lane == 0) {
        ss_st(ssim_out + n, s);
        ss_st(sq_out + n, q);
      }
    }
  }
}

struct SsShape { int Ho, Wo, tiles_x, tiles; long long items, parts; };

// SPK_OK and the launch shape, or the error the arguments earn
int ss_shape(int N, int C, int H, int W, int ws, SsShape* o) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || ws <= 0) return SPK_ERR_ARG;
  if (ws > SS_MAX_WS) return SPK_ERR_UNSUPPORTED;
  const long long Ho = (long long)H + 2 * (ws / 2) - ws + 1, Wo = (long long)W + 2 * (ws / 2) - ws + 1;
  const long long tx = (Wo + SS_TILE - 1) / SS_TILE, ty = (Ho + SS_TILE - 1) / SS_TILE;
  const long long tiles = tx * ty, planes = (long long)N * C;      // tx, ty < 2^27; planes < 2^62
  if (Ho > INT_MAX || Wo > INT_MAX || tiles > (long long)INT_MAX || planes > (long long)INT_MAX / tiles)
    return SPK_ERR_UNSUPPORTED;
  o->Ho = (int)Ho;
  o->Wo = (int)Wo;
  o->tiles_x = (int)tx;
  o->tiles = (int)tiles;
  o->items = planes * tiles;
  o->parts = (long long)C * tiles;                                 // work items per image
  return SPK_OK;
}

}  // namespace

extern "C" long long spk_ssim_mse_ws_bytes(int N, int C, int H, int W, int window_size) {
  SsShape sh;
  const int rc = ss_shape(N, C, H, W, window_size, &sh);
  if (rc != SPK_OK) return rc;
  return 16 * sh.items;                                            // two fp64 partials per work item
}

extern "C" int spk_ssim_mse(const float* img1, const float* img2, const float* window2d, double* ssim_sum_out,
                            double* sq_sum_out, void* ws_buf, int N, int C, int H, int W, int window_size,
                            hipStream_t stream) {
  if (!img1 || !img2 || !window2d || !ssim_sum_out || !sq_sum_out || !ws_buf) return SPK_ERR_ARG;
  SsShape sh;
  const int rc = ss_shape(N, C, H, W, window_size, &sh);
  if (rc != SPK_OK) return rc;
  const unsigned items = (unsigned)sh.items;
  const unsigned nb = items < SS_MAX_BLOCKS ? items : SS_MAX_BLOCKS;
  double* part = sh.parts == 1 ? nullptr : reinterpret_cast<double*>(ws_buf);
  if (window_size == 11)
    hipLaunchKernelGGL(ssim_mse_kernel<11>, dim3(nb), dim3(SS_THREADS), 0, stream, img1, img2, window2d, H, W, window_size,
                       sh.Ho, sh.Wo, sh.tiles_x, sh.tiles, items, part, ssim_sum_out, sq_sum_out);
  else
    hipLaunchKernelGGL(ssim_mse_kernel<0>, dim3(nb), dim3(SS_THREADS), 0, stream, img1, img2, window2d, H, W, window_size,
                       sh.Ho, sh.Wo, sh.tiles_x, sh.tiles, items, part, ssim_sum_out, sq_sum_out);
  SPK_LAUNCH_CHECK();
  if (part) {
    const long long per_block = sh.parts <= SS_THREAD_PER_IMAGE_PARTS ? SS_THREADS : SS_THREADS / 64;
    const long long want = (N + per_block - 1) / per_block;
    const unsigned nb2 = want < (long long)SS_MAX_BLOCKS ? (unsigned)want : SS_MAX_BLOCKS;
    hipLaunchKernelGGL(ssim_mse_sum_kernel, dim3(nb2), dim3(SS_THREADS), 0, stream, part, N, sh.parts, ssim_sum_out, sq_sum_out);
    SPK_LAUNCH_CHECK();
  }
  return SPK_OK;
}
