// Sample-quality arithmetic on a feature matrix: what R/main.py's last stage does after its feature network.
//   spk_feature_moments_acc: sum += sum_rows x, gram += x^T x  (the Gaussian fit of R/metric/Fid_score.py: mean and covariance)
//   spk_poly_kernel_sums:    sum_{i,j} (gamma <X_i, Y_j> + coef)^degree per subset (the polynomial-kernel MMD of KID)
// Both run on v_mfma_f64_16x16x4_f64.  Lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], one fp64 each;
// result register r of lane l is D[row = (l >> 4) + 4 r][col = l & 15] (the f64 form's own map, not the f32 one).  The fp32
// features are widened in registers, so every product is exact in fp64 and only the accumulation rounds.
//
// Moments: one wave owns one upper 16x16 tile of gram for the whole call -- acc = gram_in, then one MFMA per four rows in row
// order, rows at or beyond n as zeros -- and writes it and its mirror image.  Nothing is split over n and nothing depends on
// the grid, so two updates chain exactly like one update of the concatenation (when the first has a multiple of 4 rows).
// Kernel sums: a workgroup stages 32 rows of X and 32 of Y (gathered through the index tables, 64 features at a time, each row
// segment one coalesced read) in LDS; each of its four waves runs the MFMA chain of one 16x16 tile over d, raises the tile to
// the power in registers and reduces it with a fixed butterfly to one pair of partials; a second launch adds each subset's
// partials in a fixed order.  No floating-point atomics, no hand-off between workgroups.
#include <limits.h>

#include "spk_common.h"
#include "../../include/spkdiff.h"

namespace {

using fs_d4 = __attribute__((ext_vector_type(4))) double;

constexpr int FS_THREADS = 256, FS_WAVES = FS_THREADS / 64;
constexpr int FS_ROWS_AHEAD = 8;                  // MFMA steps (of 4 rows) whose loads are issued together
constexpr int FS_SUM_AHEAD = 32;                  // rows of the sum chain whose loads are issued together
constexpr int PK_M = 32;                          // rows of X and of Y per workgroup (2 x 2 tiles, one per wave)
constexpr int PK_KC = 64;                         // features staged per pass
constexpr int PK_LD = PK_KC + 4;                  // LDS row pitch in floats: lane (c, g) reads word 68 c + g -> 64 distinct banks
constexpr long long PK_ROW_PAD = -1, PK_ROW_BAD = -2;

// Inputs are read and results written at agent scope (values must not depend on the cache maintenance of the launch
// that carries the kernel, e.g. in a replayed graph).
__device__ __forceinline__ float fs_ld(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int fs_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double fs_ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void fs_st(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ fs_d4 fs_mfma(double a, double b, fs_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// grid (Td, ceil(Td / 4)): wave (blockIdx.y * 4 + wave, blockIdx.x) = tile (ti, tj); the waves below the diagonal leave at once
__global__ __launch_bounds__(FS_THREADS) void fs_gram_kernel(const float* x, long long n, int d, long long stride, double* gram) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int tj = blockIdx.x, ti = blockIdx.y * FS_WAVES + (threadIdx.x >> 6);
  if (ti > tj) return;                                            // wave-uniform; no barrier in this kernel
  const int ca = ti * 16 + c, cb = tj * 16 + c;                   // this lane's column of x as the A / B operand
  const bool va = ca < d, vb = cb < d;
  const float* pa = x + (va ? ca : d - 1);                        // a padding column reads a valid address and feeds zero
  const float* pb = x + (vb ? cb : d - 1);
  fs_d4 acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = ti * 16 + g + 4 * r;
    acc[r] = (row < d && vb) ? fs_ld(gram + (size_t)row * d + cb) : 0.0;
  }
  long long k0 = 0;
  for (; k0 + 4 * FS_ROWS_AHEAD <= n; k0 += 4 * FS_ROWS_AHEAD) {  // whole steps: no row test
    float fa[FS_ROWS_AHEAD], fb[FS_ROWS_AHEAD];
#pragma unroll
    for (int s = 0; s < FS_ROWS_AHEAD; ++s) {
      const long long off = (k0 + 4 * s + g) * stride;
      fa[s] = fs_ld(pa + off);
      fb[s] = fs_ld(pb + off);
    }
#pragma unroll
    for (int s = 0; s < FS_ROWS_AHEAD; ++s) acc = fs_mfma(va ? (double)fa[s] : 0.0, vb ? (double)fb[s] : 0.0, acc);
  }
  for (; k0 < n; k0 += 4) {                                       // the last steps: rows at or beyond n are zeros
    const long long k = k0 + g;
    const bool in = k < n;
    const long long off = (in ? k : 0) * stride;
    const float a = fs_ld(pa + off), b = fs_ld(pb + off);
    acc = fs_mfma(in && va ? (double)a : 0.0, in && vb ? (double)b : 0.0, acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = ti * 16 + g + 4 * r;
    if (row < d && vb) {
      fs_st(gram + (size_t)row * d + cb, acc[r]);
      if (ti != tj) fs_st(gram + (size_t)cb * d + row, acc[r]);   // the mirror image: gram stays bit-symmetric
    }
  }
}

// one thread per column: sum[c] += x[0][c], x[1][c], ... in row order
__global__ __launch_bounds__(64) void fs_sum_kernel(const float* x, long long n, int d, long long stride, double* sum) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= d) return;
  const float* p = x + c;
  double s = fs_ld(sum + c);
  long long k = 0;
  for (; k + FS_SUM_AHEAD <= n; k += FS_SUM_AHEAD) {
    float v[FS_SUM_AHEAD];
#pragma unroll
    for (int i = 0; i < FS_SUM_AHEAD; ++i) v[i] = fs_ld(p + (k + i) * stride);
#pragma unroll
    for (int i = 0; i < FS_SUM_AHEAD; ++i) s += (double)v[i];
  }
  for (; k < n; ++k) s += (double)fs_ld(p + k * stride);
  fs_st(sum + c, s);
}

// grid (macro tiles of 32 x 32, S).  part: [S][ntp][ntq][2] = {sum, diagonal sum} of every 16x16 tile.
__global__ __launch_bounds__(FS_THREADS) void pk_tile_kernel(const float* X, long long nx, const float* Y, long long ny, int d,
                                                             const int* ix, const int* iy, int p, int q, int mq, int ntp, int ntq,
                                                             double gamma, double coef, int degree, int symmetric, double* part) {
  __shared__ float sx[PK_M * PK_LD], sy[PK_M * PK_LD];
  __shared__ long long rx[PK_M], ry[PK_M];                        // row of X / Y, PK_ROW_PAD beyond p / q, PK_ROW_BAD outside the matrix
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int s = blockIdx.y, mi = blockIdx.x / mq, mj = blockIdx.x % mq;
  if (tid < 2 * PK_M) {
    const bool isx = tid < PK_M;
    const int t = isx ? tid : tid - PK_M;
    const int i = (isx ? mi : mj) * PK_M + t, cnt = isx ? p : q;
    const int* tab = isx ? ix : iy;
    const long long rows = isx ? nx : ny;
    long long r = PK_ROW_PAD;
    if (i < cnt) {
      r = tab ? (long long)fs_ld(tab + (size_t)s * cnt + i) : (long long)i;
      if (r < 0 || r >= rows) r = PK_ROW_BAD;
    }
    (isx ? rx : ry)[t] = r;
  }
  __syncthreads();
  const int wi = wave >> 1, wj = wave & 1;
  const float* ax = sx + (wi * 16 + c) * PK_LD + g;
  const float* by = sy + (wj * 16 + c) * PK_LD + g;
  fs_d4 acc = {0.0, 0.0, 0.0, 0.0};
  const int kk = tid & (PK_KC - 1);
  for (int k0 = 0; k0 < d; k0 += PK_KC) {
    if (k0) __syncthreads();                                      // the previous pass has been read
    const int k = k0 + kk;
    for (int rr = tid / PK_KC; rr < PK_M; rr += FS_THREADS / PK_KC) {
      const long long r1 = rx[rr], r2 = ry[rr];
      float v1 = r1 == PK_ROW_BAD ? __builtin_nanf("") : 0.f, v2 = r2 == PK_ROW_BAD ? __builtin_nanf("") : 0.f;
      if (k < d) {
        if (r1 >= 0) v1 = fs_ld(X + (size_t)r1 * d + k);
        if (r2 >= 0) v2 = fs_ld(Y + (size_t)r2 * d + k);
      }
      sx[rr * PK_LD + kk] = v1;
      sy[rr * PK_LD + kk] = v2;
    }
    __syncthreads();
    const int left = d - k0, kend = left < PK_KC ? (left + 3) & ~3 : PK_KC;   // (features beyond d are staged as zeros)
    for (int ks = 0; ks < kend; ks += 4) acc = fs_mfma((double)ax[ks], (double)by[ks], acc);
  }
  double tsum = 0.0, dsum = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = mi * PK_M + wi * 16 + g + 4 * r, j = mj * PK_M + wj * 16 + c;
    if (i < p && j < q) {
      const double v = gamma * acc[r] + coef;
      double pw = v;
      for (int e = 1; e < degree; ++e) pw = pw * v;
      tsum += pw;
      if (symmetric && i == j) dsum += pw;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {                        // butterfly: both partners add the same two values
    tsum += __shfl_xor(tsum, off, 64);
    dsum += __shfl_xor(dsum, off, 64);
  }
  const int t16 = mi * 2 + wi, u16 = mj * 2 + wj;
  if (lane == 0 && t16 < ntp && u16 < ntq) {
    double* o = part + 2 * (((size_t)s * ntp + t16) * ntq + u16);
    fs_st(o, tsum);
    fs_st(o + 1, dsum);
  }
}

// one workgroup per subset: thread t adds partials t, t + 256, ... in ascending order, then a binary tree over the threads
__global__ __launch_bounds__(FS_THREADS) void pk_sum_kernel(const double* part, long long tiles, double* out) {
  __shared__ double red[2 * FS_THREADS];
  const int tid = threadIdx.x;
  const double* p = part + 2 * (size_t)blockIdx.x * tiles;
  double a = 0.0, b = 0.0;
  for (long long t = tid; t < tiles; t += FS_THREADS) {
    a += fs_ld(p + 2 * t);
    b += fs_ld(p + 2 * t + 1);
  }
  red[tid] = a;
  red[FS_THREADS + tid] = b;
  __syncthreads();
  for (int s = FS_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      red[FS_THREADS + tid] += red[FS_THREADS + tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    fs_st(out + 2 * (size_t)blockIdx.x, red[0]);
    fs_st(out + 2 * (size_t)blockIdx.x + 1, red[FS_THREADS]);
  }
}

struct PkShape { int mp, mq, ntp, ntq; long long tiles; };

int pk_shape(int S, int p, int q, PkShape* o) {
  if (S < 1 || p < 1 || q < 1) return SPK_ERR_ARG;
  if (S > 65535) return SPK_ERR_UNSUPPORTED;
  const long long mp = ((long long)p + PK_M - 1) / PK_M, mq = ((long long)q + PK_M - 1) / PK_M;
  if (mp * mq > (long long)INT_MAX) return SPK_ERR_UNSUPPORTED;
  o->mp = (int)mp;
  o->mq = (int)mq;
  o->ntp = (int)(((long long)p + 15) / 16);
  o->ntq = (int)(((long long)q + 15) / 16);
  o->tiles = (long long)o->ntp * o->ntq;
  return SPK_OK;
}

}  // namespace

extern "C" int spk_feature_moments_acc(const float* x, long long n, int d, long long row_stride, double* sum_inout,
                                       double* gram_inout, hipStream_t stream) {
  if (!sum_inout || !gram_inout || n < 0 || d < 1 || row_stride < d || (n > 0 && !x)) return SPK_ERR_ARG;
  if (d > SPK_FEATURE_MAX_D) return SPK_ERR_UNSUPPORTED;
  if (n == 0) return SPK_OK;
  const int Td = (d + 15) / 16;
  hipLaunchKernelGGL(fs_gram_kernel, dim3(Td, (Td + FS_WAVES - 1) / FS_WAVES), dim3(FS_THREADS), 0, stream, x, n, d, row_stride,
                     gram_inout);
  SPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(fs_sum_kernel, dim3((d + 63) / 64), dim3(64), 0, stream, x, n, d, row_stride, sum_inout);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" long long spk_poly_kernel_sums_ws_bytes(int S, int p, int q) {
  PkShape sh;
  const int rc = pk_shape(S, p, q, &sh);
  if (rc != SPK_OK) return rc;
  return 16 * (long long)S * sh.tiles;
}

extern "C" int spk_poly_kernel_sums(const float* X, long long n_x, const float* Y, long long n_y, int d, const int* ix_or_null,
                                    const int* iy_or_null, int S, int p, int q, const double* gamma_coef_host, int degree,
                                    int symmetric, double* out, void* ws, long long ws_bytes, hipStream_t stream) {
  if (!X || !Y || !out || !ws || !gamma_coef_host || n_x < 1 || n_y < 1 || d < 1) return SPK_ERR_ARG;
  PkShape sh;
  const int rc = pk_shape(S, p, q, &sh);
  if (rc != SPK_OK) return rc;
  if (degree < 1 || degree > SPK_POLY_KERNEL_MAX_DEGREE) return SPK_ERR_ARG;
  if ((!ix_or_null || !iy_or_null) && S != 1) return SPK_ERR_ARG;
  if ((!ix_or_null && p > n_x) || (!iy_or_null && q > n_y)) return SPK_ERR_ARG;
  if (ws_bytes < 16 * (long long)S * sh.tiles) return SPK_ERR_ARG;
  if (d > SPK_FEATURE_MAX_D) return SPK_ERR_UNSUPPORTED;
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(pk_tile_kernel, dim3((unsigned)(sh.mp * sh.mq), S), dim3(FS_THREADS), 0, stream, X, n_x, Y, n_y, d,
                     ix_or_null, iy_or_null, p, q, sh.mq, sh.ntp, sh.ntq, gamma_coef_host[0], gamma_coef_host[1], degree,
                     symmetric ? 1 : 0, part);
  SPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(pk_sum_kernel, dim3(S), dim3(FS_THREADS), 0, stream, part, sh.tiles, out);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
