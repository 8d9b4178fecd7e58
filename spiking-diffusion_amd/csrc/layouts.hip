// The spike storage layouts and the conversions between them (DESIGN.md §3 "Data layout in HBM"; include/spkdiff.h "spike layouts").
// The interface tensor is fp32 [T,B,C,H,W] (1.0 = spike); between layers a spike tensor is stored in one of four forms, a RECORD
// being the channels of one (position, step) that lie together in memory:
//   PTC   u8            [B][HW][T][C]                one byte per channel (0 / 1), all C channels in one record
//   CPTC  u8            [B][C/chunk][HW][T][chunk]   the same bytes in records of `chunk` channels
//   C4    e2m1 nibbles  [B][C/64][HW][T][32 B]       64 channels per record
//   S32   e2m1 nibbles  [B][C/32][HW][T][16 B]       32 channels per record
// (nibble records: channel k in nibble k, even channel = low nibble; a spike is the e2m1 code of 1.0 (0x2), silence 0x0)
// The fused kernels write these records themselves (spk_e2m1_record / spk_spread8 / spk_e2m1_nibbles4 of spk_common.h); this file
// holds what converts at a module boundary.  The Python side's copy of the table: spkdiff/ops.py LAYOUTS, layout_of, empty_spikes.
#include "spk_common.h"
#include "../../include/spkdiff.h"

namespace {

constexpr int T16 = 16;
constexpr int PTC_GRID_CAP = 256 * 8 * 4;      // 256 CUs x 8 blocks, x4 for tail balance; grid-stride the rest
constexpr int REC_GRID_CAP = 65536;

// ------------------------------------------------------------------------------------------ fp32 <-> PTC / CPTC
// fp32 spikes [T,B,C,H,W]  ->  u8 [B,H,W,T,C]   (one thread per (b, hw, t, c); reads strided, writes coalesced)
__global__ __launch_bounds__(256) void spikes_to_ptc_kernel(const float* __restrict__ s, uint8_t* __restrict__ o,
                                                            int T, int B, int C, int HW, int chunk) {
  // output memory order: [B][C/chunk][HW][T][chunk]  (chunk == C: plain PTC [B][HW][T][C])
  long long total = (long long)T * B * C * HW;
  const int nch = C / chunk;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int cc = (int)(i % chunk);
    long long r = i / chunk;
    int t = (int)(r % T); r /= T;
    int hw = (int)(r % HW); r /= HW;
    int c = (int)(r % nch) * chunk + cc;
    int b = (int)(r / nch);
    float f = s[(((long long)t * B + b) * C + c) * HW + hw];
    o[i] = f != 0.0f ? 1 : 0;
  }
}

// u8 [B,H,W,T,C] -> fp32 [T,B,C,H,W]   (one thread per output element)
__global__ __launch_bounds__(256) void ptc_to_spikes_kernel(const uint8_t* __restrict__ s, float* __restrict__ o,
                                                            int T, int B, int C, int HW, int chunk) {
  long long total = (long long)T * B * C * HW;
  const int nch = C / chunk;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int hw = (int)(i % HW);
    long long r = i / HW;
    int c = (int)(r % C); r /= C;
    int b = (int)(r % B);
    int t = (int)(r / B);
    o[i] = (float)s[((((long long)b * nch + c / chunk) * HW + hw) * T + t) * chunk + c % chunk];
  }
}

// ------------------------------------------------------------------------------------------ fp32 <-> C4 / S32
// fp32 spikes [T,B,C,HW] <-> nibble-packed records of RC channels [B][C/RC][HW][T][RC/2 B] (tests, module boundaries): one thread
// per record byte on the way in, per fp32 element on the way back
template <int RC>
__global__ void spikes_to_records_kernel(const float* __restrict__ s, uint8_t* __restrict__ o, int T, int B, int C, int HW) {
  constexpr int RB = RC / 2;
  const long long total = (long long)B * (C / RC) * HW * T * RB;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int byte = (int)(i % RB);
    long long r = i / RB;
    const int t = (int)(r % T); r /= T;
    const int p = (int)(r % HW); r /= HW;
    const int cc = (int)(r % (C / RC));
    const int b = (int)(r / (C / RC));
    const int c0 = cc * RC + 2 * byte;
    const float s0 = s[(((long long)t * B + b) * C + c0) * HW + p], s1 = s[(((long long)t * B + b) * C + c0 + 1) * HW + p];
    o[i] = (uint8_t)((s0 != 0.f ? 0x02 : 0) | (s1 != 0.f ? 0x20 : 0));
  }
}
template <int RC>
__global__ void records_to_spikes_kernel(const uint8_t* __restrict__ q, float* __restrict__ s, int T, int B, int C, int HW) {
  const long long total = (long long)T * B * C * HW;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW);
    long long r = i / HW;
    const int c = (int)(r % C); r /= C;
    const int b = (int)(r % B);
    const int t = (int)(r / B);
    const uint8_t by = q[((((long long)b * (C / RC) + c / RC) * HW + p) * T + t) * (RC / 2) + (c % RC) / 2];
    s[i] = ((by >> (4 * (c & 1))) & 0xf) ? 1.0f : 0.0f;
  }
}

template <int RC>
int spikes_to_records(const float* spikes, uint8_t* out, int T, int B, int C, int HW, hipStream_t stream) {
  static_assert(RC == 64 || RC == 32, "C4 and S32 records");
  if (!spikes || !out || T <= 0 || B <= 0 || C <= 0 || HW <= 0) return SPK_ERR_ARG;
  if (C % RC) return SPK_ERR_UNSUPPORTED;
  const long long total = (long long)B * (C / RC) * HW * T * (RC / 2);
  hipLaunchKernelGGL(spikes_to_records_kernel<RC>, dim3(spk_grid(total, REC_GRID_CAP)), dim3(256), 0, stream, spikes, out, T, B,
                     C, HW);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

template <int RC>
int records_to_spikes(const uint8_t* in, float* spikes, int T, int B, int C, int HW, hipStream_t stream) {
  static_assert(RC == 64 || RC == 32, "C4 and S32 records");
  if (!spikes || !in || T <= 0 || B <= 0 || C <= 0 || HW <= 0) return SPK_ERR_ARG;
  if (C % RC) return SPK_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(records_to_spikes_kernel<RC>, dim3(spk_grid((long long)T * B * C * HW, REC_GRID_CAP)), dim3(256), 0, stream,
                     in, spikes, T, B, C, HW);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

// ------------------------------------------------------------------------------------------ channels-last fp32 -> C4
// channels-last fp32 spikes [T][B][HW][C] -> C4: one thread = 4 consecutive channels of one (t, b, hw) = one 16-bit word
__global__ void spikes_nhwc_to_fp4_kernel(const float* __restrict__ s, uint8_t* __restrict__ o, int T, int B, int C, int HW) {
  const long long total = (long long)T * B * HW * (C / 4);
  const int Q = C / 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(i % Q);
    const long long row = i / Q;                       // (t * B + b) * HW + hw
    const int hw = (int)(row % HW);
    const long long tb = row / HW;
    const int b = (int)(tb % B), t = (int)(tb / B);
    const float4 v = reinterpret_cast<const float4*>(s)[i];
    const unsigned w = spk_e2m1_nibbles4(v.x, v.y, v.z, v.w);
    const int c = q * 4;
    uint8_t* dst = o + ((((long long)b * (C >> 6) + (c >> 6)) * HW + hw) * T + t) * 32 + ((c & 63) >> 1);
    *reinterpret_cast<uint16_t*>(dst) = (uint16_t)w;
  }
}

// the same conversion with the per-neuron spike COUNTS over T as a by-product (fp32 [B][HW][C], channels-last): one thread = 4
// consecutive channels of one (b, hw) for all T steps.  The training step's last layer convolves its weight gradient with these
// counts (ops.SpikeConvMeanTrainFunction); they were a separate reduction over the [T,B,320,7,7] spike tensor (32 us at B = 32).
__global__ void spikes_nhwc_to_fp4_counts_kernel(const float* __restrict__ s, uint8_t* __restrict__ o, float* __restrict__ cnt,
                                                 int T, int B, int C, int HW) {
  const int Q = C / 4;
  const long long total = (long long)B * HW * Q, plane = (long long)B * HW * Q;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(i % Q);
    const long long row = i / Q;                       // b * HW + hw
    const int hw = (int)(row % HW), b = (int)(row / HW);
    const int c = q * 4;
    uint8_t* dst = o + (((long long)b * (C >> 6) + (c >> 6)) * HW + hw) * T * 32 + ((c & 63) >> 1);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < T; ++t) {
      const float4 v = reinterpret_cast<const float4*>(s)[t * plane + i];
      const unsigned w = spk_e2m1_nibbles4(v.x, v.y, v.z, v.w);
      acc.x += v.x != 0.f ? 1.f : 0.f; acc.y += v.y != 0.f ? 1.f : 0.f;
      acc.z += v.z != 0.f ? 1.f : 0.f; acc.w += v.w != 0.f ? 1.f : 0.f;
      *reinterpret_cast<uint16_t*>(dst + t * 32) = (uint16_t)w;
    }
    reinterpret_cast<float4*>(cnt)[i] = acc;
  }
}

// ------------------------------------------------------------------------------------------ PTC -> S32
// u8 PTC [B][HW][16][C] -> S32 [B][ceil(C/32)][HW][16][16 B] (channels beyond C: zero nibbles); one thread per 16-byte record
__global__ void ptc_to_s32_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int B, int HW, int C) {
  const int nch = (C + 31) / 32;
  const long long total = (long long)B * nch * HW * T16;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i;
    const int t = (int)(r % T16); r /= T16;
    const int p = (int)(r % HW); r /= HW;
    const int cc = (int)(r % nch);
    const int b = (int)(r / nch);
    const uint8_t* src = in + (((long long)b * HW + p) * T16 + t) * C + cc * 32;
    const int nc = C - cc * 32 < 32 ? C - cc * 32 : 32;
    unsigned w[4] = {0, 0, 0, 0};
    if ((C & 15) == 0) {                                    // 16 or 32 channels: vector loads
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (16 * h < nc) {
          const uint4 v = *reinterpret_cast<const uint4*>(src + 16 * h);
          const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {                     // four bytes (0 / 1) -> four nibbles (0 / 2)
            const unsigned x = q[k] & 0x01010101u;
            const unsigned n4 = ((x | (x >> 4)) & 0x00ff00ffu);
            const unsigned n16 = (n4 | (n4 >> 8)) & 0xffffu;
            w[2 * h + (k >> 1)] |= (n16 << 1) << (16 * (k & 1));
          }
        }
      }
    } else {
      for (int c = 0; c < nc; ++c) w[c >> 3] |= (src[c] ? 2u : 0u) << (4 * (c & 7));
    }
    *reinterpret_cast<uint4*>(out + i * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace

extern "C" int spk_spikes_to_ptc(const float* spikes_tbchw, uint8_t* out_bhwtc, int T, int B, int C, int HW,
                                 int chunk, hipStream_t stream) {
  if (!spikes_tbchw || !out_bhwtc || T <= 0 || B <= 0 || C <= 0 || HW <= 0 || chunk <= 0 || C % chunk)
    return SPK_ERR_ARG;
  hipLaunchKernelGGL(spikes_to_ptc_kernel, dim3(spk_grid((long long)T * B * C * HW, PTC_GRID_CAP)), dim3(256), 0, stream,
                     spikes_tbchw, out_bhwtc, T, B, C, HW, chunk);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_ptc_to_spikes(const uint8_t* in_bhwtc, float* spikes_tbchw, int T, int B, int C, int HW,
                                 int chunk, hipStream_t stream) {
  if (!in_bhwtc || !spikes_tbchw || T <= 0 || B <= 0 || C <= 0 || HW <= 0 || chunk <= 0 || C % chunk)
    return SPK_ERR_ARG;
  hipLaunchKernelGGL(ptc_to_spikes_kernel, dim3(spk_grid((long long)T * B * C * HW, PTC_GRID_CAP)), dim3(256), 0, stream,
                     in_bhwtc, spikes_tbchw, T, B, C, HW, chunk);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_spikes_to_fp4(const float* spikes, uint8_t* out_c4, int T, int B, int C, int HW, hipStream_t stream) {
  return spikes_to_records<64>(spikes, out_c4, T, B, C, HW, stream);
}

extern "C" int spk_fp4_to_spikes(const uint8_t* in_c4, float* spikes, int T, int B, int C, int HW, hipStream_t stream) {
  return records_to_spikes<64>(in_c4, spikes, T, B, C, HW, stream);
}

extern "C" int spk_spikes_to_s32(const float* spikes, uint8_t* out_s32, int T, int B, int C, int HW, hipStream_t stream) {
  return spikes_to_records<32>(spikes, out_s32, T, B, C, HW, stream);
}

extern "C" int spk_s32_to_spikes(const uint8_t* in_s32, float* spikes, int T, int B, int C, int HW, hipStream_t stream) {
  return records_to_spikes<32>(in_s32, spikes, T, B, C, HW, stream);
}

extern "C" int spk_spikes_nhwc_to_fp4(const float* spikes_nhwc, uint8_t* out_c4, int T, int B, int C, int HW,
                                      hipStream_t stream) {
  if (!spikes_nhwc || !out_c4 || T <= 0 || B <= 0 || C <= 0 || HW <= 0) return SPK_ERR_ARG;
  if (C % 64) return SPK_ERR_UNSUPPORTED;
  const long long total = (long long)T * B * HW * (C / 4);
  hipLaunchKernelGGL(spikes_nhwc_to_fp4_kernel, dim3(spk_grid(total, REC_GRID_CAP)), dim3(256), 0, stream, spikes_nhwc, out_c4, T,
                     B, C, HW);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_spikes_nhwc_to_fp4_counts(const float* spikes_nhwc, uint8_t* out_c4, float* counts_nhwc, int T, int B, int C,
                                             int HW, hipStream_t stream) {
  if (!spikes_nhwc || !out_c4 || !counts_nhwc || T <= 0 || B <= 0 || C <= 0 || HW <= 0) return SPK_ERR_ARG;
  if (C % 64) return SPK_ERR_UNSUPPORTED;
  const long long total = (long long)B * HW * (C / 4);
  hipLaunchKernelGGL(spikes_nhwc_to_fp4_counts_kernel, dim3(spk_grid(total, REC_GRID_CAP)), dim3(256), 0, stream, spikes_nhwc,
                     out_c4, counts_nhwc, T, B, C, HW);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_ptc_to_s32(const uint8_t* in_ptc, uint8_t* out_s32, int T, int B, int HW, int C, hipStream_t stream) {
  if (!in_ptc || !out_s32 || B <= 0 || HW <= 0 || C <= 0) return SPK_ERR_ARG;
  if (T != T16) return SPK_ERR_UNSUPPORTED;
  const long long total = (long long)B * ((C + 31) / 32) * HW * T16;
  hipLaunchKernelGGL(ptc_to_s32_kernel, dim3(spk_grid(total, REC_GRID_CAP)), dim3(256), 0, stream, in_ptc, out_s32, B, HW, C);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
