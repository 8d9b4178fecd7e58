// The plain-CNN VQVAE baseline (R/snn_model/vae_model.py:548-672, main.py --model vq-vae), eval path.
//   spk_ann_vqvae_encode   Conv 3x3 s2 p1 C->32 + ReLU, Conv 3x3 s2 p1 32->64 + ReLU, Conv 1x1 64->D, L2 arg min over the
//                          K codes (+ optional z and the gathered e): ONE launch, one workgroup per image, every
//                          intermediate in LDS
//   spk_ann_vqvae_decode   embedding gather (or a given e), ConvT 3x3 s2 p1 op1 D->64 + ReLU, ConvT 3x3 s2 p1 op1 64->32 + ReLU
//                          (launch 1, its output planar [B,32,H,W] in the caller's workspace), ConvT 3x3 s1 p1 32->C + the uint8
//                          image (launch 2)
//
// Arithmetic: fp32 products and fp32 accumulation, every multiply-add an fmaf, each output's sum in one fixed order (from the
// bias, input channels ascending, taps ascending), so an image's result depends on nothing but that image and the weights.  The
// weights are read with wave-uniform addresses straight from global memory (scalar loads, operands of the vector fmaf): no
// weight ever occupies LDS or a vector register.  The stride-2 transposed convolutions run by sub-pixel class: a thread owns
// one input position's 2x2 output block and issues the block's nine taps per channel pair -- 1 + 2 + 2 + 4 -- and none of the
// 27 structural zeros.  ReLU keeps a NaN (v < 0 ? 0 : v), as torch.relu does.  The code distances |z|^2 + |e_k|^2 - 2 z.e_k are
// fp64 on the fp32 z (exact products), the arg min is torch.argmin's (vq_argmin.h).  A token outside [0, K) embeds as NaN and
// is never used as an index.
#include <mutex>

#include "spk_common.h"
#include "vq_argmin.h"
#include "../../include/spkdiff.h"

namespace {

constexpr int AV_D = SPK_ANN_VQVAE_D, AV_C1 = 32, AV_C2 = 64;
constexpr int AV_CBS = AV_D + 1;                                   // LDS row stride of a code / a z vector (bank spread)
// 16 waves per workgroup, four per SIMD: a wave's wait for its next weights (scalar loads served by L2: a layer's weights are
// larger than the scalar cache) is covered by the other waves' arithmetic.  The waves split the output channels, so the work
// does not grow with their number (DESIGN.md 4.13 has the 4-wave A/B).
constexpr int AV_THREADS = 1024, AV_WAVES = AV_THREADS / 64;

__device__ __forceinline__ float av_relu(float v) { return v < 0.0f ? 0.0f : v; }

// LDS floats of the encoder at image side H and K codes: image | conv1 output | conv2 output | z | codebook | |e_k|^2 (fp64)
__host__ __device__ constexpr int av_enc_img(int C, int H) { return C * H * H; }
__host__ __device__ constexpr int av_enc_h1(int H) { return AV_C1 * (H / 2) * (H / 2); }
__host__ __device__ constexpr int av_enc_h2(int H) { return AV_C2 * (H / 4) * (H / 4); }
__host__ __device__ constexpr int av_enc_z(int H) { return (H / 4) * (H / 4) * AV_CBS; }
static size_t av_enc_lds_bytes(int C, int H, int K) {
  const size_t f = (size_t)av_enc_img(C, H) + av_enc_h1(H) + av_enc_h2(H) + av_enc_z(H) + (size_t)K * AV_CBS;
  return ((f + 1) & ~(size_t)1) * sizeof(float) + (size_t)K * sizeof(double);
}

template <int C>
__global__ __launch_bounds__(AV_THREADS) void ann_encode_kernel(
    const float* __restrict__ g_img, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3, const float* __restrict__ cb,
    long long* __restrict__ idx_out, float* __restrict__ z_out, float* __restrict__ e_out, int B, int H, int K) {
  extern __shared__ float lds[];
  const int H1 = H / 2, H2 = H / 4, HW1 = H1 * H1, HW2 = H2 * H2;
  float* s_img = lds;
  float* s_h1 = s_img + av_enc_img(C, H);
  float* s_h2 = s_h1 + av_enc_h1(H);
  float* s_z = s_h2 + av_enc_h2(H);
  float* s_cb = s_z + av_enc_z(H);
  double* s_e2 = reinterpret_cast<double*>(lds + ((av_enc_img(C, H) + av_enc_h1(H) + av_enc_h2(H) + av_enc_z(H) + K * AV_CBS + 1) & ~1));
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  for (int i = tid; i < K * AV_D; i += AV_THREADS) s_cb[(i / AV_D) * AV_CBS + (i % AV_D)] = cb[i];
  __syncthreads();
  for (int k = tid; k < K; k += AV_THREADS) {
    double e2 = 0.0;
#pragma unroll
    for (int d = 0; d < AV_D; ++d) { const double e = s_cb[k * AV_CBS + d]; e2 = fma(e, e, e2); }
    s_e2[k] = e2;
  }

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();                                               // (the previous image's LDS is read no more; s_e2 is written)
    const float* img = g_img + (long long)b * C * H * H;
    for (int i = tid; i < C * H * H; i += AV_THREADS) s_img[i] = img[i];
    __syncthreads();

    // Every layer: a wave owns a group of output channels -- its weight addresses are wave-uniform --, a lane one output position.
    // conv1: 2 channels per wave
    {
      constexpr int NJ = AV_C1 / AV_WAVES;
      const int co0 = wave * NJ;
      for (int p = lane; p < HW1; p += 64) {
        const int oy = p / H1, ox = p - oy * H1;
        float acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = b1[co0 + j];
#pragma unroll
        for (int ci = 0; ci < C; ++ci)
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
              const int ix = 2 * ox - 1 + kx;
              const bool in = iy >= 0 && iy < H && ix >= 0 && ix < H;
              const float v = in ? s_img[(ci * H + iy) * H + ix] : 0.0f;        // (a border tap adds nothing)
#pragma unroll
              for (int j = 0; j < NJ; ++j) acc[j] = fmaf(v, w1[(((co0 + j) * C + ci) * 3 + ky) * 3 + kx], acc[j]);
            }
          }
#pragma unroll
        for (int j = 0; j < NJ; ++j) s_h1[(co0 + j) * HW1 + p] = av_relu(acc[j]);
      }
    }
    __syncthreads();

    // conv2: 4 channels per wave
    {
      constexpr int NJ = AV_C2 / AV_WAVES;
      const int co0 = wave * NJ;
      for (int p = lane; p < HW2; p += 64) {
        const int oy = p / H2, ox = p - oy * H2;
        float acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = b2[co0 + j];
#pragma unroll 2
        for (int ci = 0; ci < AV_C1; ++ci) {
          const float* wp = w2 + ((long long)co0 * AV_C1 + ci) * 9;
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
              const int ix = 2 * ox - 1 + kx;
              const bool in = iy >= 0 && iy < H1 && ix >= 0 && ix < H1;
              const float v = in ? s_h1[(ci * H1 + iy) * H1 + ix] : 0.0f;
#pragma unroll
              for (int j = 0; j < NJ; ++j) acc[j] = fmaf(v, wp[j * AV_C1 * 9 + ky * 3 + kx], acc[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) s_h2[(co0 + j) * HW2 + p] = av_relu(acc[j]);
      }
    }
    __syncthreads();

    // conv3 (1x1): one channel per wave
    {
      static_assert(AV_D == AV_WAVES, "one latent channel per wave");
      const int d = wave;
      for (int p = lane; p < HW2; p += 64) {
        float acc = b3[d];
#pragma unroll 8
        for (int ci = 0; ci < AV_C2; ++ci) acc = fmaf(s_h2[ci * HW2 + p], w3[d * AV_C2 + ci], acc);
        s_z[p * AV_CBS + d] = acc;
        if (z_out) z_out[((long long)b * AV_D + d) * HW2 + p] = acc;
      }
    }
    __syncthreads();

    // arg min: a wave per position, a lane per code (spk_vq_argmin's arithmetic: x2 + e2 - 2 dot in fp64, d ascending)
    for (int p = wave; p < HW2; p += AV_WAVES) {
      double xr[AV_D], x2 = 0.0;
#pragma unroll
      for (int d = 0; d < AV_D; ++d) { xr[d] = (double)s_z[p * AV_CBS + d]; x2 = fma(xr[d], xr[d], x2); }
      double best = __builtin_inf();
      int besti = VQ_NONE;
      for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const int kc = k < K ? k : K - 1;
        double dot = 0.0;
#pragma unroll
        for (int d = 0; d < AV_D; ++d) dot = fma(xr[d], (double)s_cb[kc * AV_CBS + d], dot);
        const double dist = x2 + s_e2[kc] - 2.0 * dot;
        if (k < K && vq_lane_takes(dist, best)) { best = dist; besti = k; }
      }
      vq_wave_combine(best, besti);
      besti = vq_index(besti);
      if (lane == 0) idx_out[(long long)b * HW2 + p] = (long long)besti;
      if (e_out && lane < AV_D) e_out[((long long)b * AV_D + lane) * HW2 + p] = s_cb[besti * AV_CBS + lane];
    }
  }
}

// e | first layer's output | one row + 2 floats that the edge positions' unconditional neighbour reads may touch
static size_t av_dec_lds_bytes(int H) {
  return ((size_t)AV_D * (H / 4) * (H / 4) + (size_t)AV_C2 * (H / 2) * (H / 2) + H / 2 + 2) * sizeof(float);
}

// The 2x2 output block of input position (iy, ix) of a stride-2, pad-1, output-pad-1 3x3 transposed convolution, one channel
// pair: x00 = in(iy, ix), x01 = in(iy, ix + 1), x10 = in(iy + 1, ix), x11 = in(iy + 1, ix + 1) (0 past the edge), w the pair's
// [3][3] taps.  Output (y, x) takes in(i, j) * w[y + 1 - 2 i][x + 1 - 2 j]: the even rows and columns see the centre tap only.
__device__ __forceinline__ void av_convt_block(float (&o)[4], float x00, float x01, float x10, float x11, const float* w) {
  o[0] = fmaf(x00, w[4], o[0]);
  o[1] = fmaf(x01, w[3], o[1]);
  o[1] = fmaf(x00, w[5], o[1]);
  o[2] = fmaf(x10, w[1], o[2]);
  o[2] = fmaf(x00, w[7], o[2]);
  o[3] = fmaf(x11, w[0], o[3]);
  o[3] = fmaf(x10, w[2], o[3]);
  o[3] = fmaf(x01, w[6], o[3]);
  o[3] = fmaf(x00, w[8], o[3]);
}

// h2: [B][32][H][H], the second layer's output
__global__ __launch_bounds__(AV_THREADS) void ann_decode_front_kernel(
    const long long* __restrict__ tok, const float* __restrict__ e_in, const float* __restrict__ cb, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ h2, int B, int H,
    int K) {
  extern __shared__ float lds[];
  const int H0 = H / 4, H1 = H / 2, HW0 = H0 * H0, HW1 = H1 * H1, HW = H * H;
  float* s_e = lds;                                                // [16][H0][H0]
  float* s_h1 = s_e + AV_D * HW0;                                  // [64][H1][H1]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();
    for (int i = tid; i < AV_D * HW0; i += AV_THREADS) {
      const int d = i / HW0, p = i - d * HW0;
      float v;
      if (tok) {
        const long long k = tok[(long long)b * HW0 + p];
        v = (k >= 0 && k < K) ? cb[k * AV_D + d] : __builtin_nanf("");
      } else {
        v = e_in[(long long)b * AV_D * HW0 + i];
      }
      s_e[i] = v;
    }
    __syncthreads();

    // convT1 16 -> 64: a wave owns 4 output channels, a lane one input position
    {
      constexpr int NJ = AV_C2 / AV_WAVES;
      const int co0 = wave * NJ;
      for (int p = lane; p < HW0; p += 64) {
        const int iy = p / H0, ix = p - iy * H0;
        const bool rx = ix + 1 < H0, ry = iy + 1 < H0;
        float o[NJ][4];
#pragma unroll
        for (int j = 0; j < NJ; ++j) { const float bv = b1[co0 + j]; o[j][0] = o[j][1] = o[j][2] = o[j][3] = bv; }
#pragma unroll 2
        for (int ci = 0; ci < AV_D; ++ci) {
          const float* sp = s_e + ci * HW0 + p;
          const float l01 = sp[1], l10 = sp[H0], l11 = sp[H0 + 1];      // (unconditional reads, inside the LDS image)
          const float x00 = sp[0], x01 = rx ? l01 : 0.0f, x10 = ry ? l10 : 0.0f, x11 = (rx && ry) ? l11 : 0.0f;
          const float* wp = w1 + ((long long)ci * AV_C2 + co0) * 9;
#pragma unroll
          for (int j = 0; j < NJ; ++j) av_convt_block(o[j], x00, x01, x10, x11, wp + j * 9);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          float* hp = s_h1 + (co0 + j) * HW1 + (2 * iy) * H1 + 2 * ix;
          hp[0] = av_relu(o[j][0]);
          hp[1] = av_relu(o[j][1]);
          hp[H1] = av_relu(o[j][2]);
          hp[H1 + 1] = av_relu(o[j][3]);
        }
      }
    }
    __syncthreads();

    // convT2 64 -> 32: a wave owns 8 output channels (cg) and a quarter of the positions (pq, rotated with cg so that every
    // SIMD gets each quarter once: at 14 x 14 the last quarter holds 4 positions), a lane one input position
    {
      constexpr int NJ = 8;
      static_assert(AV_WAVES == 4 * (AV_C1 / NJ), "four position quarters x four channel groups");
      const int cg = wave >> 2, pq = (wave + cg) & 3, co0 = cg * NJ;
      for (int p = pq * 64 + lane; p < HW1; p += 4 * 64) {
        const int iy = p / H1, ix = p - iy * H1;
        const bool rx = ix + 1 < H1, ry = iy + 1 < H1;
        float o[NJ][4];
#pragma unroll
        for (int j = 0; j < NJ; ++j) { const float bv = b2[co0 + j]; o[j][0] = o[j][1] = o[j][2] = o[j][3] = bv; }
        for (int ci = 0; ci < AV_C2; ++ci) {
          const float* sp = s_h1 + ci * HW1 + p;
          const float l01 = sp[1], l10 = sp[H1], l11 = sp[H1 + 1];
          const float x00 = sp[0], x01 = rx ? l01 : 0.0f, x10 = ry ? l10 : 0.0f, x11 = (rx && ry) ? l11 : 0.0f;
          const float* wp = w2 + ((long long)ci * AV_C1 + co0) * 9;
#pragma unroll
          for (int j = 0; j < NJ; ++j) av_convt_block(o[j], x00, x01, x10, x11, wp + j * 9);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          float* gp = h2 + ((long long)b * AV_C1 + co0 + j) * HW + (2 * iy) * H + 2 * ix;
          *reinterpret_cast<float2*>(gp) = make_float2(av_relu(o[j][0]), av_relu(o[j][1]));
          *reinterpret_cast<float2*>(gp + H) = make_float2(av_relu(o[j][2]), av_relu(o[j][3]));
        }
      }
    }
  }
}

// convT3 32 -> C, stride 1, pad 1 (out(y, x) = sum in(y + 1 - ky, x + 1 - kx) w[ky][kx]) + the uint8 image of R/main.py:400
// (np.clip(pred + 0.5, 0, 1) * 255, truncating cast; a NaN pixel gives 0).  One thread per output pixel, all C channels.
constexpr int AV_BACK_THREADS = 128;
template <int C>
__global__ __launch_bounds__(AV_BACK_THREADS) void ann_decode_back_kernel(const float* __restrict__ h2, const float* __restrict__ w,
                                                                          const float* __restrict__ bias, float* __restrict__ out,
                                                                          uint8_t* __restrict__ out_u8, int H) {
  const int HW = H * H, b = blockIdx.y;
  const int p = blockIdx.x * AV_BACK_THREADS + threadIdx.x;
  if (p >= HW) return;
  const int y = p / H, x = p - y * H;
  // the nine taps' offsets (clamped into the plane: the loads are unconditional and a channel's nine are in flight together)
  int off[9];
  bool in[9];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = y + 1 - ky, ix = x + 1 - kx;
      in[ky * 3 + kx] = iy >= 0 && iy < H && ix >= 0 && ix < H;
      off[ky * 3 + kx] = min(max(iy, 0), H - 1) * H + min(max(ix, 0), H - 1);
    }
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = bias[c];
  const float* hb = h2 + (long long)b * AV_C1 * HW;
#pragma unroll 4
  for (int ci = 0; ci < AV_C1; ++ci) {
    const float* wp = w + (long long)ci * C * 9;
    float v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) v[t] = hb[(long long)ci * HW + off[t]];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float vt = in[t] ? v[t] : 0.0f;
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = fmaf(vt, wp[c * 9 + t], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const long long o = ((long long)b * C + c) * HW + p;
    out[o] = acc[c];
    if (out_u8) {
      const float f = fminf(fmaxf(acc[c] + 0.5f, 0.0f), 1.0f);
      out_u8[o] = (uint8_t)(int)(f * 255.0f);
    }
  }
}

template <typename KernelT>
void av_allow_lds(KernelT kernel) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
}

}  // namespace

extern "C" int spk_ann_vqvae_supported(int C, int H, int W, int D, int K) {
  if (!(C == 1 || C == 3) || H != W || !(H == 28 || H == 32) || D != SPK_ANN_VQVAE_D) return 0;
  return K >= 2 && K <= SPK_ANN_VQVAE_MAX_K && av_enc_lds_bytes(C, H, K) <= 152 * 1024;
}

extern "C" long long spk_ann_vqvae_decode_ws_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return SPK_ERR_ARG;
  return (long long)B * AV_C1 * H * W * (long long)sizeof(float);
}

extern "C" int spk_ann_vqvae_encode(const float* images, const float* w1, const float* b1, const float* w2, const float* b2,
                                    const float* w3, const float* b3, const float* codebook, long long* idx_out,
                                    float* z_out_or_null, float* e_out_or_null, int B, int C, int H, int W, int D, int K,
                                    hipStream_t stream) {
  if (!images || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !codebook || !idx_out || B <= 0) return SPK_ERR_ARG;
  if (!spk_ann_vqvae_supported(C, H, W, D, K)) return SPK_ERR_UNSUPPORTED;
  // (the attribute is set once per process, ahead of any capture: the first call of a kernel is never a captured one --
  //  a warm-up iteration runs in front of a capture)
  static std::once_flag once;
  std::call_once(once, [] { av_allow_lds(ann_encode_kernel<1>); av_allow_lds(ann_encode_kernel<3>); });
  const int grid = B < SPK_ANN_VQVAE_GRID_CAP ? B : SPK_ANN_VQVAE_GRID_CAP;
  const size_t lds = av_enc_lds_bytes(C, H, K);
  if (C == 1)
    hipLaunchKernelGGL(ann_encode_kernel<1>, dim3(grid), dim3(AV_THREADS), lds, stream, images, w1, b1, w2, b2, w3, b3, codebook, idx_out,
                       z_out_or_null, e_out_or_null, B, H, K);
  else
    hipLaunchKernelGGL(ann_encode_kernel<3>, dim3(grid), dim3(AV_THREADS), lds, stream, images, w1, b1, w2, b2, w3, b3, codebook, idx_out,
                       z_out_or_null, e_out_or_null, B, H, K);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_ann_vqvae_decode(const long long* tokens_or_null, const float* e_or_null, const float* codebook,
                                    const float* wt1, const float* bt1, const float* wt2, const float* bt2, const float* wt3,
                                    const float* bt3, void* ws, long long ws_bytes, float* x_recon_out, uint8_t* u8_out_or_null,
                                    int B, int C, int H, int W, int D, int K, hipStream_t stream) {
  if ((!tokens_or_null) == (!e_or_null) || (tokens_or_null && !codebook) || !wt1 || !bt1 || !wt2 || !bt2 || !wt3 || !bt3 ||
      !ws || !x_recon_out || B <= 0 || B > 65535)
    return SPK_ERR_ARG;
  if (!spk_ann_vqvae_supported(C, H, W, D, K)) return SPK_ERR_UNSUPPORTED;
  if (ws_bytes < spk_ann_vqvae_decode_ws_bytes(B, H, W) || ((uintptr_t)ws & 7)) return SPK_ERR_ARG;
  static std::once_flag once;
  std::call_once(once, [] { av_allow_lds(ann_decode_front_kernel); });
  const int grid = B < SPK_ANN_VQVAE_GRID_CAP ? B : SPK_ANN_VQVAE_GRID_CAP;
  hipLaunchKernelGGL(ann_decode_front_kernel, dim3(grid), dim3(AV_THREADS), av_dec_lds_bytes(H), stream, tokens_or_null, e_or_null, codebook,
                     wt1, bt1, wt2, bt2, static_cast<float*>(ws), B, H, K);
  SPK_LAUNCH_CHECK();
  const dim3 g2((H * W + AV_BACK_THREADS - 1) / AV_BACK_THREADS, B);
  if (C == 1)
    hipLaunchKernelGGL(ann_decode_back_kernel<1>, g2, dim3(AV_BACK_THREADS), 0, stream, static_cast<const float*>(ws), wt3, bt3, x_recon_out,
                       u8_out_or_null, H);
  else
    hipLaunchKernelGGL(ann_decode_back_kernel<3>, g2, dim3(AV_BACK_THREADS), 0, stream, static_cast<const float*>(ws), wt3, bt3, x_recon_out,
                       u8_out_or_null, H);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
