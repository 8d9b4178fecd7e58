// Completion of partly given images: the two elementwise steps around the conditional reverse process, as
// launches of their own so that the whole call is a fixed launch sequence without a host round trip and the start state can
// be the first node of the sampler's captured graph.
//
//   spk_completion_state    code indices + keep mask -> the sampler's start state (x_t, unmasked) [+ known tokens per image]
//   spk_completion_compose  given pixels (main.py's uint8 conversion, R/main.py:401) pasted over the decoder's uint8 image
//
// The reverse process itself (R/snn_model/vq_diffusion.py:110-140) is unchanged: it runs from
//   unmasked = known & (0 <= x_init < K),  x_t = where(unmasked, x_init, mask_id)
// instead of the all-masked state.  Plain kernels: the denoiser is where the time goes.
#include "spk_common.h"
#include "../../include/spkdiff.h"

namespace {

// One thread per token.  Token (i, j) of image b is known iff every mask byte in rows stride*i - radius .. stride*i + radius and
// columns stride*j - radius .. stride*j + radius, clipped to the mask, is non-zero (what lies outside the mask is the encoder's
// zero padding: given) and the code index is inside [0, K).
__global__ __launch_bounds__(256) void completion_state_kernel(const long long* __restrict__ codes, const uint8_t* __restrict__ keep,
                                                               long long* __restrict__ x_t, uint8_t* __restrict__ unmasked, int B,
                                                               int h, int w, int Hm, int Wm, int stride, int radius, int K,
                                                               long long mask_id) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * h * w) return;
  const int b = i / (h * w), r = i % (h * w);
  const int ty = r / w, tx = r % w;
  int y0 = stride * ty - radius, y1 = stride * ty + radius;
  int x0 = stride * tx - radius, x1 = stride * tx + radius;
  y0 = y0 < 0 ? 0 : y0;
  x0 = x0 < 0 ? 0 : x0;
  y1 = y1 > Hm - 1 ? Hm - 1 : y1;
  x1 = x1 > Wm - 1 ? Wm - 1 : x1;
  const uint8_t* m = keep + (long long)b * Hm * Wm;
  bool known = true;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) known = known && (m[y * Wm + x] != 0);
  const long long c = codes[i];
  known = known && c >= 0 && c < (long long)K;
  x_t[i] = known ? c : mask_id;
  unmasked[i] = known ? 1 : 0;
}

// Known tokens per image (reports): one thread per image over its HW bytes -- no atomics, nothing to zero beforehand.
__global__ __launch_bounds__(256) void completion_count_kernel(const uint8_t* __restrict__ unmasked, int* __restrict__ n_known, int B,
                                                               int HW) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int n = 0;
  for (int p = 0; p < HW; ++p) n += unmasked[(long long)b * HW + p] ? 1 : 0;
  n_known[b] = n;
}

// out = keep ? uint8(clip(image + 0.5, 0, 1) * 255) : decoded_u8; fp32 operations in numpy's order, truncating cast (a NaN pixel
// gives 0).
__global__ __launch_bounds__(256) void completion_compose_kernel(const float* __restrict__ image, const uint8_t* __restrict__ keep,
                                                                 const uint8_t* __restrict__ decoded, uint8_t* __restrict__ out,
                                                                 long long total, int C, int HW) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / ((long long)C * HW);
    const int p = (int)(i % HW);
    uint8_t v = decoded[i];
    if (keep[b * HW + p]) {
      float f = image[i] + 0.5f;
      f = fminf(fmaxf(f, 0.0f), 1.0f);
      v = (uint8_t)(int)(f * 255.0f);
    }
    out[i] = v;
  }
}

}  // namespace

extern "C" int spk_completion_state(const long long* codes_bhw, const uint8_t* keep_mask, long long* x_t_out, uint8_t* unmasked_out,
                                    int* n_known_out_or_null, int B, int h, int w, int Hm, int Wm, int stride, int radius, int K,
                                    long long mask_id, hipStream_t stream) {
  if (!codes_bhw || !keep_mask || !x_t_out || !unmasked_out || B <= 0 || h <= 0 || w <= 0 || Hm <= 0 || Wm <= 0 || stride <= 0 ||
      radius < 0 || K <= 0)
    return SPK_ERR_ARG;
  // every token's window must meet the mask, and the token count must fit the 32-bit thread index
  if ((long long)stride * (h - 1) - radius > Hm - 1 || (long long)stride * (w - 1) - radius > Wm - 1) return SPK_ERR_ARG;
  if ((long long)B * h * w > 0x7fffffffLL - 255 || (long long)Hm * Wm > 0x7fffffffLL) return SPK_ERR_ARG;
  const int total = B * h * w;
  hipLaunchKernelGGL(completion_state_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, codes_bhw, keep_mask, x_t_out,
                     unmasked_out, B, h, w, Hm, Wm, stride, radius, K, mask_id);
  SPK_LAUNCH_CHECK();
  if (n_known_out_or_null) {
    hipLaunchKernelGGL(completion_count_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, unmasked_out, n_known_out_or_null, B,
                       h * w);
    SPK_LAUNCH_CHECK();
  }
  return SPK_OK;
}

extern "C" int spk_completion_compose(const float* image_bchw, const uint8_t* keep_bhw, const uint8_t* decoded_u8_bchw,
                                      uint8_t* out_u8_bchw, int B, int C, int H, int W, hipStream_t stream) {
  if (!image_bchw || !keep_bhw || !decoded_u8_bchw || !out_u8_bchw || B <= 0 || C <= 0 || H <= 0 || W <= 0) return SPK_ERR_ARG;
  if ((long long)H * W > 0x7fffffffLL) return SPK_ERR_ARG;
  const long long total = (long long)B * C * H * W;
  long long grid = (total + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(completion_compose_kernel, dim3((int)grid), dim3(256), 0, stream, image_bchw, keep_bhw, decoded_u8_bchw,
                     out_u8_bchw, total, C, H * W);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
