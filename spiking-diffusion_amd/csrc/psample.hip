// One reverse step of the absorbing-state discrete diffusion sampler, after the denoiser produced the logits:
//   R/snn_model/vq_diffusion.py:113-124 (where to unmask), :134-140 (temperature, Categorical sample, scatter).
//
//   changes  = (u < 1/t) & ~unmasked ;  unmasked |= changes
//   x0_hat   = Categorical(logits = logits/temp).sample()
//            = argmax_k softmax(l - logsumexp l)_k / q_k ,  q ~ Exp(1)      (torch.multinomial one-draw fast path)
//   x_t[changes] = x0_hat[changes]
//
// Noise sources: (a) injected u [B*HW] and q [B*HW*K] (parity mode: the host draws them with the reference's CPU
// generator in the reference's order), or (b) on-device Philox4x32-10 keyed by (seed, offset)
// (throughput mode).  One wave per latent position; lanes stride over the K classes; wave reductions by DPP shuffles.
#include "spk_common.h"
#include "den_common.h"
#include "psample_common.h"
#include "../../include/spkdiff.h"
#include <math.h>

namespace {

__device__ __forceinline__ bool __any_sync_quad(bool v) {      // OR over the 4 lanes of a quad
  int x = v ? 1 : 0;
  x |= __shfl_xor(x, 1);
  x |= __shfl_xor(x, 2);
  return x != 0;
}

// KPL = classes per lane (K <= 64 * KPL): 4 covers the reference's default codebook (--codebook_size 128, R/main.py:58);
// 8 / 16 / 32 are instantiated for larger codebooks (K <= 2048).
// PT = per-image temperature (spk_psample_step_temps): `temp` is then a device array indexed by IMAGE (active[slot] in the
// active-set form, like x_t / unmasked / the noise), read once per position; the division below is the same fp32 division.  A
// separate instantiation: the scalar kernel's code does not change.
// TK = top-k truncation (spk_psample_step_topk; always with PT): `temp` is then the pair of per-image arrays {temperatures, k}, and
// a position whose token is drawn has its scaled logits truncated (truncate_top_k, psample_common.h) ahead of the unchanged race.
// TP = nucleus truncation after the top-k one (spk_psample_step_topp; always with PT and TK): the triple {temperatures, k, p} and
// truncate_top_p between truncate_top_k and the race.
template <int KPL, bool PT = false, bool TK = false, bool TP = false>
__global__ __launch_bounds__(256) void psample_kernel(const float* __restrict__ logits, long long* __restrict__ x_t,
                                                      uint8_t* __restrict__ unmasked, int t, spk_temp_arg_t<PT, TK, TP> temp,
                                                      const float* __restrict__ u_in, const float* __restrict__ q_in,
                                                      unsigned long long seed, unsigned long long offset,
                                                      const unsigned long long* __restrict__ philox_state,
                                                      long long* __restrict__ x0_hat_out,
                                                      const int* __restrict__ active, const int* __restrict__ n_active,
                                                      int B, int HW, int K, float* __restrict__ next_input, float t_next) {
  philox_base(philox_state, seed, offset);
  const int lane = threadIdx.x & 63;
  // active-set form (spk_select_active): logits hold one slot per ACTIVE image (slot s = image active[s]); noise, x_t
  // and unmasked stay indexed by image, so the draws are those of the dense form
  const int Bn = spk_active_count(active, n_active, B);
  const long long npos = (long long)Bn * HW;
  const float inv_t = 1.0f / (float)t;
  for (long long ps = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); ps < npos; ps += (long long)gridDim.x * 4) {
    const int b = (int)(ps / HW), hw = (int)(ps % HW);            // b = logits slot
    const long long p = active ? (long long)active[b] * HW + hw : ps;   // image position: noise / state index
    if (!x0_hat_out) {
      // only positions that change consume the sample (:140): skip the rest before the softmax (wave-uniform test;
      // the noise is counter-based / injected per position, so skipping a draw does not move any other)
      const float u = reveal_u(u_in, seed, offset, p, K);
      if (!((u < inv_t) && !unmasked[p])) {
        if (next_input && lane == 0) write_next_input(next_input, b, hw, HW, (float)x_t[p], t_next);   // keeps its token
        continue;
      }
    }
    float l[KPL];
    const float tp = spk_temp_of<PT, TK, TP>(temp, active ? active[b] : b);
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int k = lane + 64 * j;
      // (unconditional load from a clamped index + select: hipcc waits for a conditional load on its own)
      const float lg = logits[((long long)b * K + (k < K ? k : K - 1)) * HW + hw];
      l[j] = k < K ? lg / tp : -INFINITY;
    }
    if constexpr (TK) truncate_top_k<KPL>(l, lane, K, temp.topk[active ? active[b] : b]);
    if constexpr (TP) truncate_top_p<KPL>(l, lane, K, temp.topp[active ? active[b] : b]);
    const int besti = categorical_race<KPL>(l, lane, K, q_in, seed, offset, p);
    if (lane == 0) {
      const float u = reveal_u(u_in, seed, offset, p, K);
      bool ch = (u < inv_t) && !unmasked[p];
      if (ch) { unmasked[p] = 1; x_t[p] = (long long)besti; }
      if (x0_hat_out) x0_hat_out[p] = (long long)besti;
      if (next_input) write_next_input(next_input, b, hw, HW, ch ? (float)besti : (float)x_t[p], t_next);
    }
  }
}

// The same step under the confidence-ordered reveal (psample_common.h, "THE rule"; spk_psample_step_conf): one workgroup per
// image, no global workspace.  The four waves stride over the image's positions and run the `_topp` family's draw at every
// position masked at entry (candidate -> x0_hat_out, confidence -> conf_out, candidate and order key -> LDS); behind a barrier
// wave 0 -- lane = position -- ranks the keys, commits the n surest candidates and writes the next step's input from the
// committed state.  HW <= 64 (the host checks).  The stream-0 uniform is not drawn.  Which POSITIONS change depends on the
// logits, so there are no position lists; which IMAGES have nothing to do does not (psample_conf_listed_kernel below).
template <int KPL>
__global__ __launch_bounds__(256) void psample_conf_kernel(const float* __restrict__ logits, long long* __restrict__ x_t,
                                                           uint8_t* __restrict__ unmasked, int t, spk_temp_topp temp,
                                                           const float* __restrict__ q_in, unsigned long long seed,
                                                           unsigned long long offset,
                                                           const unsigned long long* __restrict__ philox_state,
                                                           long long* __restrict__ x0_hat_out, float* __restrict__ conf_out,
                                                           int HW, int K, float* __restrict__ next_input, float t_next) {
  __shared__ int s_cand[64];
  __shared__ uint32_t s_key[64];
  philox_base(philox_state, seed, offset);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const float tp = temp.temp[b];
  const int topk = temp.topk[b];
  const float topp = temp.topp[b];
  for (int hw = wave; hw < HW; hw += 4) {
    const long long p = (long long)b * HW + hw;
    if (unmasked[p]) continue;                                      // (wave-uniform)
    float l[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int k = lane + 64 * j;
      const float lg = logits[((long long)b * K + (k < K ? k : K - 1)) * HW + hw];
      l[j] = k < K ? lg / tp : -INFINITY;
    }
    truncate_top_k<KPL>(l, lane, K, topk);
    truncate_top_p<KPL>(l, lane, K, topp);
    float conf;
    const int besti = categorical_race<KPL, true>(l, lane, K, q_in, seed, offset, p, &conf);
    if (lane == 0) {
      s_cand[hw] = besti;
      s_key[hw] = spk_conf_key(conf);
      if (x0_hat_out) x0_hat_out[p] = (long long)besti;
      if (conf_out) conf_out[p] = conf;
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const long long p = (long long)b * HW + (lane < HW ? lane : 0);
  const bool masked = lane < HW && !unmasked[p];
  const bool reveal = confident_reveal(masked, lane, HW, t, s_key);
  if (reveal) { unmasked[p] = 1; x_t[p] = (long long)s_cand[lane]; }
  if (next_input && lane < HW) write_next_input(next_input, b, lane, HW, reveal ? (float)s_cand[lane] : (float)x_t[p], t_next);
}

// The same update on the list of PENDING images (spk_psample_step_conf_listed; the rule: include/spkdiff.h):
// workgroup s serves slot s of the list spk_select_pending wrote and returns at once past its length.  The logits lie by slot;
// state, noise, the per-image arrays and the two outputs by image b = active[s].  Image b runs e = min(steps_b[b], S) steps of
// its own inside a loop of S, so its step index at loop step t is e - t, not S - t: it draws at offset - (S - e) * step_stride,
// the counters it would draw alone in a run of e steps.  An image with t > e is not pending and is left as it is whatever the
// list says.  No next_input: the listed form gathers its denoiser input by slot.
// The body is the dense kernel's with the two indices apart, and psample_conf_sched_kernel below repeats the candidate draw a third
// time, line for line.  The copies are deliberate: drawing through one shared __forceinline__ helper changed the instruction
// stream of all 16 instances of the three kernels (profiles/conf_launcher_resources.txt has the numbers).  Only the host side is
// shared (psample_conf_launch).
template <int KPL>
__global__ __launch_bounds__(256) void psample_conf_listed_kernel(const float* __restrict__ logits, long long* __restrict__ x_t,
                                                                  uint8_t* __restrict__ unmasked, int t, spk_temp_topp temp,
                                                                  const float* __restrict__ q_in, unsigned long long seed,
                                                                  unsigned long long offset,
                                                                  const unsigned long long* __restrict__ philox_state,
                                                                  long long* __restrict__ x0_hat_out, float* __restrict__ conf_out,
                                                                  const int* __restrict__ steps_b, int S,
                                                                  unsigned long long step_stride, const int* __restrict__ active,
                                                                  const int* __restrict__ n_active, int B, int HW, int K) {
  __shared__ int s_cand[64];
  __shared__ uint32_t s_key[64];
  const int s = blockIdx.x;                                         // the logits' slot
  if (s >= spk_active_count(active, n_active, B)) return;          // (workgroup-uniform, ahead of the barrier)
  const int b = active[s];                                          // the image: state, noise, per-image arrays, outputs
  const int sb = steps_b[b];
  const int e = sb < S ? sb : S;
  if (t > e) return;
  philox_base(philox_state, seed, offset);
  offset -= (unsigned long long)(S - e) * step_stride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float tp = temp.temp[b];
  const int topk = temp.topk[b];
  const float topp = temp.topp[b];
  for (int hw = wave; hw < HW; hw += 4) {
    const long long p = (long long)b * HW + hw;
    if (unmasked[p]) continue;                                      // (wave-uniform)
    float l[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int k = lane + 64 * j;
      const float lg = logits[((long long)s * K + (k < K ? k : K - 1)) * HW + hw];
      l[j] = k < K ? lg / tp : -INFINITY;
    }
    truncate_top_k<KPL>(l, lane, K, topk);
    truncate_top_p<KPL>(l, lane, K, topp);
    float conf;
    const int besti = categorical_race<KPL, true>(l, lane, K, q_in, seed, offset, p, &conf);
    if (lane == 0) {
      s_cand[hw] = besti;
      s_key[hw] = spk_conf_key(conf);
      if (x0_hat_out) x0_hat_out[p] = (long long)besti;
      if (conf_out) conf_out[p] = conf;
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const long long p = (long long)b * HW + (lane < HW ? lane : 0);
  const bool masked = lane < HW && !unmasked[p];
  const bool reveal = confident_reveal(masked, lane, HW, t, s_key);
  if (reveal) { unmasked[p] = 1; x_t[p] = (long long)s_cand[lane]; }
}

// The confidence-ordered update under a reveal schedule and annealed selection noise (spk_psample_step_conf_sched and, LISTED,
// spk_psample_step_conf_listed_sched; the rule: psample_common.h): the two kernels above with the count read from
// the image's row of sched_w and the order key taken from score = conf + a * g, which wave 0 computes for all positions at once
// between the draw and the rank.  x0_hat_out and conf_out are the sibling's.
// LISTED: workgroup = slot of the pending list, logits by slot, everything else -- the two tables too -- by image active[s], the
// counters (those of the Gumbel uniform included) shifted to the image's own run of e steps; no next_input.
// RM: remasking on top of it (spk_psample_step_conf_remask and, LISTED, spk_psample_step_conf_listed_remask; the rule:
// psample_common.h): wave 0 -- the wave that commits -- reads the image's commit_conf with its `unmasked` bytes,
// parks the keys of the revisable positions in the free entries of s_key (the reveal's keys sit at the masked ones), and after the
// reveal ranks them once more from the other end.  Its four arguments are a base of the argument block, empty without the flag.
template <bool RM> struct spk_remask_arg_t {};
template <> struct spk_remask_arg_t<true> {
  const uint32_t* r;                              // [B][S + 1]
  float* commit_conf;                             // [B*HW], in place
  uint8_t* remasked_out;                          // [B*HW] or null
  long long mask_id;
};
template <bool RM = false> struct spk_sched_arg_t : spk_remask_arg_t<RM> {
  const uint32_t* w;                              // [B][S + 1]
  const float* a;                                 // [B][S + 1] or null
  const float* u_in;                              // injected uniforms [B*HW] or null
  float* score_out;                               // [B*HW] or null
  int S;
};
template <int KPL, bool LISTED, bool RM = false>
__global__ __launch_bounds__(256) void psample_conf_sched_kernel(const float* __restrict__ logits, long long* __restrict__ x_t,
                                                                 uint8_t* __restrict__ unmasked, int t, spk_temp_topp temp,
                                                                 const float* __restrict__ q_in, unsigned long long seed,
                                                                 unsigned long long offset,
                                                                 const unsigned long long* __restrict__ philox_state,
                                                                 long long* __restrict__ x0_hat_out, float* __restrict__ conf_out,
                                                                 spk_sched_arg_t<RM> sc, const int* __restrict__ steps_b,
                                                                 unsigned long long step_stride, const int* __restrict__ active,
                                                                 const int* __restrict__ n_active, int B, int HW, int K,
                                                                 float* __restrict__ next_input, float t_next) {
  __shared__ int s_cand[64];
  __shared__ uint32_t s_key[64];
  const int s = blockIdx.x;                                         // the logits' slot
  int b = s;                                                        // the image: state, noise, per-image arrays, tables, outputs
  int e = sc.S;
  if constexpr (LISTED) {
    if (s >= spk_active_count(active, n_active, B)) return;        // (workgroup-uniform, ahead of the barrier)
    b = active[s];
    const int sb = steps_b[b];
    e = sb < sc.S ? sb : sc.S;
    if (t > e) return;
  }
  philox_base(philox_state, seed, offset);
  if constexpr (LISTED) offset -= (unsigned long long)(sc.S - e) * step_stride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float tp = temp.temp[b];
  const int topk = temp.topk[b];
  const float topp = temp.topp[b];
  for (int hw = wave; hw < HW; hw += 4) {
    const long long p = (long long)b * HW + hw;
    if (unmasked[p]) continue;                                      // (wave-uniform)
    float l[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int k = lane + 64 * j;
      const float lg = logits[((long long)s * K + (k < K ? k : K - 1)) * HW + hw];
      l[j] = k < K ? lg / tp : -INFINITY;
    }
    truncate_top_k<KPL>(l, lane, K, topk);
    truncate_top_p<KPL>(l, lane, K, topp);
    float conf;
    const int besti = categorical_race<KPL, true>(l, lane, K, q_in, seed, offset, p, &conf);
    if (lane == 0) {
      s_cand[hw] = besti;
      s_key[hw] = __float_as_uint(conf);                            // (the confidence itself: its key is taken below)
      if (x0_hat_out) x0_hat_out[p] = (long long)besti;
      if (conf_out) conf_out[p] = conf;
    }
  }
  __syncthreads();
  // the scores, by the wave that ranks them -- lane = position, so the Gumbel draws of an image run side by side, once
  const long long p = (long long)b * HW + (lane < HW ? lane : 0);
  const bool masked = lane < HW && !unmasked[p];
  const long long row = (long long)b * (sc.S + 1);
  float conf_l = 0.f;                                               // RM: this lane's confidence, kept for commit_conf
  bool revisable = false;
  if (wave == 0 && masked) {
    conf_l = __uint_as_float(s_key[lane]);
    const float score = sched_score(conf_l, sc.a ? sc.a[row + t] : 0.f, sc.u_in, seed, offset, p, K);
    s_key[lane] = spk_conf_key(score);
    if (sc.score_out) sc.score_out[p] = score;
  }
  if constexpr (RM) {
    if (wave == 0 && lane < HW && !masked) {
      const float cc = sc.commit_conf[p];
      revisable = cc != INFINITY;
      s_key[lane] = spk_conf_key(cc);                               // (an entry the reveal does not read: it reads the masked ones)
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const bool reveal = confident_reveal_sched(masked, lane, HW, sc.w[row + t - 1], sc.w[row + t], s_key);
  if (reveal) { unmasked[p] = 1; x_t[p] = (long long)s_cand[lane]; }
  if constexpr (RM) {
    const bool any_masked = __ballot(masked) != 0ull;               // (m == 0: no remask, nothing written)
    const bool remask = confident_remask(revisable, lane, HW, (t > 1 && any_masked) ? sc.r[row + t] : 0u, s_key);
    if (reveal) sc.commit_conf[p] = conf_l;
    if (remask) { unmasked[p] = 0; x_t[p] = sc.mask_id; }
    if (sc.remasked_out && any_masked && lane < HW) sc.remasked_out[p] = remask ? 1 : 0;
  }
  if constexpr (!LISTED) {
    // (RM: read after this lane's own writes -- a remasked position shows mask_id)
    if (next_input && lane < HW) write_next_input(next_input, b, lane, HW, reveal ? (float)s_cand[lane] : (float)x_t[p], t_next);
  }
}

// Denoiser input map, R/snn_model/vq_diffusion.py:195-197:  cat(x, ones_like(x) * t[:,None,None,None]) -> [B,2,h,w]
// x comes either as float [B,1,h,w] (the module API) or as the int64 token state x_t of the sampler.
__global__ void den_input_kernel(const float* __restrict__ xf, const long long* __restrict__ xi,
                                 const long long* __restrict__ t_vec, long long t_scalar, float* __restrict__ out,
                                 const int* __restrict__ active, const int* __restrict__ n_active, int B, int HW) {
  const int Bn = spk_active_count(active, n_active, B);
  const int total = Bn * HW;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / HW, hw = i % HW;                            // output slot
    const int src = active ? active[b] * HW + hw : i;             // active-set form: slot b holds image active[b]
    const float x = xf ? xf[src] : (float)xi[src];
    const float tv = (float)(t_vec ? t_vec[active ? active[b] : b] : t_scalar);
    write_next_input(out, b, hw, HW, x, 1.0f * tv);
  }
}

// Which images does reverse step t touch?  R/snn_model/vq_diffusion.py:113-124 computes `changes` BEFORE the denoiser
// call and scatters x_0_hat only there (:140): for an image without a change at this step the denoiser output is never
// read and x_t / unmasked stay as they are.  This kernel evaluates the same test (same u: injected or the same Philox
// counters as spk_psample_step) per image and writes the ascending list of images with at least one change plus its
// length; the per-step kernels then run on that list only.  The list is ordered (deterministic slots).
// Eight threads per image (positions q, q + 8, ...: a Philox depth of HW / 8; the `unmasked` bytes of a thread are requested
// together), one-wave workgroups spread over the CUs; every image's flag goes to active[b], and the workgroup that finishes last
// (ticket) compacts the flags in place into the ordered list: slots are deterministic.  (The first form ran as ONE 1024-thread
// workgroup with a chain of conditional loads per thread: 10.7 us per reverse step.)  The ticket is n_active[1]: zero before the
// first call, left zero by every call (the caller's buffer, so calls on different streams with different buffers do not meet).

// The end of a select kernel (spk_select_active, spk_select_pending): every one-wave workgroup has written its images' flags to
// active[b]; the workgroup that finishes last (ticket n_active[1]) compacts them in place into the ascending list, writes its
// length to n_active[0] and re-arms the ticket.  Called by every lane of every workgroup.
__device__ __forceinline__ void compact_flags_by_last(int* __restrict__ active, int* __restrict__ n_active, int B, int lane) {
  __threadfence();
  int last = 0;
  if (lane == 0) last = atomicAdd(reinterpret_cast<unsigned*>(n_active + 1), 1u) == gridDim.x - 1 ? 1 : 0;
  last = __shfl(last, 0);
  if (!last) return;
  __threadfence();
  int base = 0;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int bi = b0 + lane;
    const int fl = bi < B ? __hip_atomic_load(&active[bi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    const unsigned long long m = __ballot(fl != 0);
    // (every lane of the wave has read its flag before any lane writes: list entries land at or below b0 + lane)
    if (fl) active[base + __popcll(m & ((1ull << lane) - 1ull))] = bi;
    base += __popcll(m);
  }
  if (lane == 0) { n_active[0] = base; n_active[1] = 0; }
}

__global__ __launch_bounds__(64) void select_active_kernel(const uint8_t* __restrict__ unmasked, int t,
                                                           const float* __restrict__ u_in, unsigned long long seed,
                                                           unsigned long long offset,
                                                           const unsigned long long* __restrict__ philox_state,
                                                           int* __restrict__ active, int* __restrict__ n_active, int B, int HW, int K) {
  philox_base(philox_state, seed, offset);
  const float inv_t = 1.0f / (float)t;
  const int lane = threadIdx.x;
  const int gid = blockIdx.x * 64 + lane;
  const int b = gid >> 3, q = gid & 7;
  bool any = false;
  if (b < B) {
    uint8_t um[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int hw = q + 8 * k;
      const uint8_t ld = unmasked[(long long)b * HW + (hw < HW ? hw : 0)];
      um[k] = hw < HW ? ld : (uint8_t)1;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (!um[k]) {
        const long long p = (long long)b * HW + q + 8 * k;
        const float u = reveal_u(u_in, seed, offset, p, K);
        any = any || (u < inv_t);
      }
    }
    for (int hw = q + 64; hw < HW; hw += 8) {                   // (latents beyond 64 positions)
      const long long p = (long long)b * HW + hw;
      if (unmasked[p]) continue;
      const float u = reveal_u(u_in, seed, offset, p, K);
      any = any || (u < inv_t);
    }
  }
  int f = any ? 1 : 0;
  f |= __shfl_xor(f, 1); f |= __shfl_xor(f, 2); f |= __shfl_xor(f, 4);
  if (q == 0 && b < B) active[b] = f;
  compact_flags_by_last(active, n_active, B, lane);
}

// Which images are PENDING at reverse step t of per-image confidence-ordered decoding (spk_select_pending)?
// Image b is pending iff 1 <= t <= steps_b[b] and at least one of its positions is masked -- no noise, no logits: the ceil(m / t)
// rule needs nothing but t, so a non-pending image can be left out of the step exactly.  The launch shape of select_active_kernel:
// eight threads per image over its `unmasked` bytes (h*w <= 64), flags, the shared compaction.
__global__ __launch_bounds__(64) void select_pending_kernel(const uint8_t* __restrict__ unmasked, int t,
                                                            const int* __restrict__ steps_b, int* __restrict__ active,
                                                            int* __restrict__ n_active, int B, int HW) {
  const int lane = threadIdx.x;
  const int gid = blockIdx.x * 64 + lane;
  const int b = gid >> 3, q = gid & 7;
  bool any = false;
  if (b < B) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int hw = q + 8 * k;
      const uint8_t ld = unmasked[(long long)b * HW + (hw < HW ? hw : 0)];
      any = any || (hw < HW && !ld);
    }
    any = any && t <= steps_b[b];
  }
  int f = any ? 1 : 0;
  f |= __shfl_xor(f, 1); f |= __shfl_xor(f, 2); f |= __shfl_xor(f, 4);
  if (q == 0 && b < B) active[b] = f;
  compact_flags_by_last(active, n_active, B, lane);
}

// Which POSITIONS of an active image does reverse step t need from each denoiser layer?  The sampler reads the logits only
// at the image's `changes` positions C (:134-140); conv6 is 3x3, so the last spiking layer is needed on dilate(C, 1), the
// one before it on dilate(C, 2), ... (3x3 convolutions, zero padding).  One wave per active slot; record (r - 1, slot)
// (64 bytes) describes radius r: bytes 0..47 the ascending list of needed positions below 48 (padded with its last entry),
// byte 48 the list length n, byte 49 its tile-count class ceil(n / 8) (1..6; a 32-row tile is two positions x 16 steps, four
// waves), byte 50 whether position 48 is needed.  (The last position of an odd latent is computed by the tail launch of the
// MFMA kernel either way.)  The workgroup that finishes last groups the slots of every radius by class (the MFMA kernel
// runs one item loop per class) and re-arms the ticket.  Buffer layout: den_common.h.
__global__ __launch_bounds__(256) void select_needed_kernel(const uint8_t* __restrict__ unmasked, int t,
                                                            const float* __restrict__ u_in, unsigned long long seed,
                                                            unsigned long long offset,
                                                            const unsigned long long* __restrict__ philox_state,
                                                            const int* __restrict__ active, const int* __restrict__ n_active,
                                                            uint8_t* __restrict__ need, int B, int H, int W, int R, int K) {
  __shared__ int s_cnt[8][8];
  __shared__ int s_last;
  philox_base(philox_state, seed, offset);
  const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int Bn = spk_active_count(active, n_active, B);
  const int HW = H * W;
  if (slot < Bn) {
    const int b = active[slot];
    bool ch = false;
    if (lane < HW) {
      const long long p = (long long)b * HW + lane;
      if (!unmasked[p]) {
        const float u = reveal_u(u_in, seed, offset, p, K);
        ch = u < 1.0f / (float)t;
      }
    }
    unsigned long long m = __ballot(ch);
    unsigned long long col0 = 0;
    const unsigned long long all = HW >= 64 ? ~0ull : ((1ull << HW) - 1ull);
    for (int y = 0; y < H; ++y) col0 |= 1ull << (y * W);
    const unsigned long long colL = col0 << (W - 1);
    for (int r = 1; r <= R; ++r) {
      const unsigned long long hdil = (m | ((m << 1) & ~col0) | ((m >> 1) & ~colL)) & all;
      m = (hdil | (hdil << W) | (hdil >> W)) & all;
      const unsigned long long ml = m & ((1ull << 48) - 1ull);            // listed: positions 0..47
      const int n = __popcll(ml);
      uint8_t* rec = need + spk_need_off_rec(B, R, r - 1) + (long long)slot * 64;
      if (lane < 48) {
        if ((ml >> lane) & 1ull) rec[__popcll(ml & ((1ull << lane) - 1ull))] = (uint8_t)lane;
        const int last = ml ? 63 - __clzll((long long)ml) : 0;
        if (lane >= n) rec[lane] = (uint8_t)last;
      }
      if (lane == 48) rec[48] = (uint8_t)n;
      if (lane == 49) rec[49] = (uint8_t)(n ? (n + 7) >> 3 : 1);
      if (lane == 50) rec[50] = (uint8_t)((m >> 48) & 1ull);
    }
  }
  // last workgroup to arrive: slots by class, per radius
  __threadfence();
  __syncthreads();
  unsigned* ticket = reinterpret_cast<unsigned*>(need);
  if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1 : 0;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  if (threadIdx.x < 64) s_cnt[threadIdx.x >> 3][threadIdx.x & 7] = 0;
  __syncthreads();
  for (int r = 0; r < R; ++r) {
    const uint8_t* recs = need + spk_need_off_rec(B, R, r);
    int* list = reinterpret_cast<int*>(need + spk_need_off_list(B, R, r));
    for (int s = threadIdx.x; s < Bn; s += blockDim.x) {
      int k = (int)__builtin_nontemporal_load(recs + (long long)s * 64 + 49) - 1;
      k = k < 0 ? 0 : (k > 5 ? 5 : k);
      list[k * B + atomicAdd(&s_cnt[r][k], 1)] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < 8 * R) {
    const int r = threadIdx.x >> 3, k = threadIdx.x & 7;
    reinterpret_cast<int*>(need + spk_need_off_cnt(r))[k] = k < 6 ? s_cnt[r][k] : 0;
  }
  if (threadIdx.x == 0) *ticket = 0u;
}

// The noise of one reverse step exactly as psample_kernel / select_active_kernel / select_needed_kernel draw it, written
// out: u[p] (stream 0, counter offset + p*K) and q[p*K + k] (stream 1, counter offset + p*K + k).  A debug / parity entry:
// the oracle is run on the dumped noise and must give the tokens of the Philox-mode sampler (the timed configuration).
__global__ __launch_bounds__(256) void philox_noise_kernel(unsigned long long seed, unsigned long long offset,
                                                           const unsigned long long* __restrict__ philox_state,
                                                           float* __restrict__ u_out, float* __restrict__ q_out,
                                                           long long npos, int K) {
  philox_base(philox_state, seed, offset);
  const long long nq = q_out ? npos * K : 0;
  const long long total = nq > npos ? nq : npos;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    if (u_out && i < npos) u_out[i] = reveal_u(nullptr, seed, offset, i, K);
    if (i < nq) q_out[i] = race_q(nullptr, seed, offset, i, 1, 0);     // (q_out is flat: i = p * K + k)
  }
}

}  // namespace

namespace {
// q_sample of the training step (R/snn_model/vq_diffusion.py:61-75): mask = u < t[b] / num_timesteps; x_t = mask ? mask_id : x_0;
// x_0_ignore = mask ? x_0 : -1.  One launch for what the module sequence spends eight on (expand, float, divide, compare, two
// fills, two selects); the uniforms u stay the framework's draw (rand_like), so the RNG stream is the reference's.
__global__ void q_sample_kernel(const float* __restrict__ x0, const long long* __restrict__ t, const float* __restrict__ u,
                                float* __restrict__ x_t, float* __restrict__ x0_ignore, uint8_t* __restrict__ mask, int B, int HW,
                                float num_timesteps, float mask_id) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * HW) return;
  const int b = i / HW;
  const bool m = u[i] < (float)t[b] / num_timesteps;
  const float x = x0[i];
  x_t[i] = m ? mask_id : x;
  x0_ignore[i] = m ? x : -1.0f;
  if (mask) mask[i] = m ? 1 : 0;
}
}  // namespace

extern "C" int spk_q_sample(const float* x0, const long long* t, const float* u, float* x_t_out, float* x0_ignore_out,
                            uint8_t* mask_out_or_null, int B, int HW, int num_timesteps, float mask_id, hipStream_t stream) {
  if (!x0 || !t || !u || !x_t_out || !x0_ignore_out || B <= 0 || HW <= 0 || num_timesteps <= 0) return SPK_ERR_ARG;
  hipLaunchKernelGGL(q_sample_kernel, dim3((B * HW + 255) / 256), dim3(256), 0, stream, x0, t, u, x_t_out, x0_ignore_out,
                     mask_out_or_null, B, HW, (float)num_timesteps, mask_id);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_philox_noise(unsigned long long philox_seed, unsigned long long philox_offset,
                                const unsigned long long* philox_state_or_null, float* u_out_or_null, float* q_out_or_null,
                                int B, int HW, int K, hipStream_t stream) {
  if ((!u_out_or_null && !q_out_or_null) || B <= 0 || HW <= 0 || K <= 0) return SPK_ERR_ARG;
  const long long npos = (long long)B * HW;
  const long long total = q_out_or_null ? npos * K : npos;
  long long grid = (total + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(philox_noise_kernel, dim3((int)grid), dim3(256), 0, stream, philox_seed, philox_offset,
                     philox_state_or_null, u_out_or_null, q_out_or_null, npos, K);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" long long spk_select_needed_bytes(int B, int R) {
  if (B <= 0 || R <= 0 || R > 8) return -1;
  return spk_need_off_rec(B, R, R);
}

extern "C" int spk_select_needed(const uint8_t* unmasked, int t, const float* u_or_null, unsigned long long philox_seed,
                                 unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                                 const int* active, const int* n_active, uint8_t* need_out, int B, int H, int W, int R,
                                 int K, hipStream_t stream) {
  if (!unmasked || !active || !n_active || !need_out || t <= 0 || B <= 0 || R <= 0 || R > 8 || K <= 0) return SPK_ERR_ARG;
  if (H != 7 || W != 7) return SPK_ERR_UNSUPPORTED;        // the record format lists positions 0..47 of a 49-position latent
  hipLaunchKernelGGL(select_needed_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, unmasked, t, u_or_null, philox_seed,
                     philox_offset, philox_state_or_null, active, n_active, need_out, B, H, W, R, K);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_select_active(const uint8_t* unmasked, int t, const float* u_or_null, unsigned long long philox_seed,
                                 unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                                 int* active_out, int* n_active_out, int B, int HW, int K, hipStream_t stream) {
  if (!unmasked || !active_out || !n_active_out || t <= 0 || B <= 0 || HW <= 0 || K <= 0) return SPK_ERR_ARG;
  hipLaunchKernelGGL(select_active_kernel, dim3((B * 8 + 63) / 64), dim3(64), 0, stream, unmasked, t, u_or_null, philox_seed,
                     philox_offset, philox_state_or_null, active_out, n_active_out, B, HW, K);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_select_pending(const uint8_t* unmasked, int t, const int* steps_b, int* active_out, int* n_active_out, int B,
                                  int HW, hipStream_t stream) {
  if (!unmasked || !steps_b || !active_out || !n_active_out || t <= 0 || B <= 0 || HW <= 0) return SPK_ERR_ARG;
  if (HW > 64) return SPK_ERR_UNSUPPORTED;                      // (eight threads x eight positions; the listed update's own limit)
  hipLaunchKernelGGL(select_pending_kernel, dim3((B * 8 + 63) / 64), dim3(64), 0, stream, unmasked, t, steps_b, active_out,
                     n_active_out, B, HW);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_den_build_input(const float* x_float_or_null, const long long* x_tokens_or_null,
                                   const long long* t_vec_or_null, long long t_scalar, float* out_b2hw, int B, int HW,
                                   const int* active_or_null, const int* n_active_or_null, hipStream_t stream) {
  if ((!x_float_or_null && !x_tokens_or_null) || !out_b2hw || B <= 0 || HW <= 0) return SPK_ERR_ARG;
  if ((active_or_null == nullptr) != (n_active_or_null == nullptr)) return SPK_ERR_ARG;
  int total = B * HW;
  hipLaunchKernelGGL(den_input_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, x_float_or_null,
                     x_tokens_or_null, t_vec_or_null, t_scalar, out_b2hw, active_or_null, n_active_or_null, B, HW);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

namespace {
template <bool PT, bool TK = false, bool TP = false>
int psample_launch(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t, spk_temp_arg_t<PT, TK, TP> temp,
                   const float* u_or_null, const float* q_or_null, unsigned long long philox_seed,
                   unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                   long long* x0_hat_out_or_null, int B, int HW, int K, const int* active_or_null, const int* n_active_or_null,
                   float* next_input_b2hw_or_null, hipStream_t stream) {
  if (!logits_bkhw || !x_t_inout || !unmasked_inout || t <= 0 || !spk_temp_arg_ok<PT, TK, TP>(temp) || B <= 0 || HW <= 0 || K <= 0)
    return SPK_ERR_ARG;
  if (next_input_b2hw_or_null && active_or_null) return SPK_ERR_ARG;      // (the active-set form gathers its input by slot)
  if ((active_or_null == nullptr) != (n_active_or_null == nullptr) || (active_or_null && x0_hat_out_or_null))
    return SPK_ERR_ARG;
  if (K > 64 * 32) return SPK_ERR_UNSUPPORTED;
  long long npos = (long long)B * HW;
  int grid = (int)((npos + 3) / 4);
  if (grid > 4096) grid = 4096;
#define SPK_PSAMPLE_LAUNCH(KPL)                                                                                          \
  hipLaunchKernelGGL((psample_kernel<KPL, PT, TK, TP>), dim3(grid), dim3(256), 0, stream, logits_bkhw, x_t_inout, unmasked_inout, \
                     t, temp, u_or_null, q_or_null, philox_seed, philox_offset, philox_state_or_null, x0_hat_out_or_null, \
                     active_or_null, n_active_or_null, B, HW, K, next_input_b2hw_or_null, (float)(t - 1))
  if (K <= 256) SPK_PSAMPLE_LAUNCH(4);
  else if (K <= 512) SPK_PSAMPLE_LAUNCH(8);
  else if (K <= 1024) SPK_PSAMPLE_LAUNCH(16);
  else SPK_PSAMPLE_LAUNCH(32);
#undef SPK_PSAMPLE_LAUNCH
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
}  // namespace

extern "C" int spk_psample_step(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                float temp, const float* u_or_null, const float* q_or_null,
                                unsigned long long philox_seed, unsigned long long philox_offset,
                                const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null, int B,
                                int HW, int K, const int* active_or_null, const int* n_active_or_null,
                                float* next_input_b2hw_or_null, hipStream_t stream) {
  return psample_launch<false>(logits_bkhw, x_t_inout, unmasked_inout, t, temp, u_or_null, q_or_null, philox_seed, philox_offset,
                               philox_state_or_null, x0_hat_out_or_null, B, HW, K, active_or_null, n_active_or_null,
                               next_input_b2hw_or_null, stream);
}

// The same step with one temperature per IMAGE: temp_b fp32 [B] on the device (include/spkdiff.h).
extern "C" int spk_psample_step_temps(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                      const float* temp_b, const float* u_or_null, const float* q_or_null,
                                      unsigned long long philox_seed, unsigned long long philox_offset,
                                      const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null, int B,
                                      int HW, int K, const int* active_or_null, const int* n_active_or_null,
                                      float* next_input_b2hw_or_null, hipStream_t stream) {
  return psample_launch<true>(logits_bkhw, x_t_inout, unmasked_inout, t, temp_b, u_or_null, q_or_null, philox_seed, philox_offset,
                              philox_state_or_null, x0_hat_out_or_null, B, HW, K, active_or_null, n_active_or_null,
                              next_input_b2hw_or_null, stream);
}

// The same step with top-k truncation: per IMAGE a temperature (temp_b fp32 [B]) and a k (topk_b int32 [B]; k <= 0 or k >= K: that
// image is not truncated) on the device (include/spkdiff.h).
extern "C" int spk_psample_step_topk(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                     const float* temp_b, const int* topk_b, const float* u_or_null, const float* q_or_null,
                                     unsigned long long philox_seed, unsigned long long philox_offset,
                                     const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null, int B,
                                     int HW, int K, const int* active_or_null, const int* n_active_or_null,
                                     float* next_input_b2hw_or_null, hipStream_t stream) {
  return psample_launch<true, true>(logits_bkhw, x_t_inout, unmasked_inout, t, spk_temp_topk{temp_b, topk_b}, u_or_null, q_or_null,
                                    philox_seed, philox_offset, philox_state_or_null, x0_hat_out_or_null, B, HW, K, active_or_null,
                                    n_active_or_null, next_input_b2hw_or_null, stream);
}

// The same step with nucleus (top-p) truncation after the top-k one: per IMAGE a temperature, a k and a p (topp_b fp32 [B]; !(0 < p
// < 1): that image is not nucleus-truncated) on the device (include/spkdiff.h).
extern "C" int spk_psample_step_topp(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                     const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                                     const float* q_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                                     const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null, int B,
                                     int HW, int K, const int* active_or_null, const int* n_active_or_null,
                                     float* next_input_b2hw_or_null, hipStream_t stream) {
  return psample_launch<true, true, true>(logits_bkhw, x_t_inout, unmasked_inout, t, spk_temp_topp{temp_b, topk_b, topp_b}, u_or_null,
                                          q_or_null, philox_seed, philox_offset, philox_state_or_null, x0_hat_out_or_null, B, HW, K,
                                          active_or_null, n_active_or_null, next_input_b2hw_or_null, stream);
}

// The confidence-ordered updates (include/spkdiff.h; the rule: psample_common.h): one launcher for the four
// entry points.  LISTED: on the list of pending images, each at its own step count (steps_b / active / n_active required, no
// next_input); SCHED: under a reveal schedule and annealed selection noise (sched_w required; u_or_null is the Gumbel uniform --
// without a schedule it is accepted and ignored: the coin is not part of the rule).  1 <= t <= S wherever the form has an S.
// REMASK (on top of SCHED only): remask_r and commit_conf_inout required, mask_id outside [0, K).
namespace {
template <bool LISTED, bool SCHED, bool REMASK = false>
int psample_conf_launch(const float* logits, long long* x_t_inout, uint8_t* unmasked_inout, int t, spk_temp_topp temp,
                        const float* u_or_null, const float* q_or_null, unsigned long long philox_seed,
                        unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                        long long* x0_hat_out_or_null, float* conf_out_or_null, int B, int HW, int K, const int* steps_b, int S,
                        unsigned long long step_stride, const int* active, const int* n_active, float* next_input_or_null,
                        const uint32_t* sched_w, const float* noise_a_or_null, float* score_out_or_null, hipStream_t stream,
                        const uint32_t* remask_r = nullptr, float* commit_conf_inout = nullptr, long long mask_id = -1,
                        uint8_t* remasked_out_or_null = nullptr) {
  static_assert(!REMASK || SCHED, "remasking exists on top of the scheduled form only");
  if (!logits || !x_t_inout || !unmasked_inout || t <= 0 || !spk_temp_arg_ok<true, true, true>(temp) || B <= 0 || HW <= 0 || K <= 0)
    return SPK_ERR_ARG;
  if ((LISTED || SCHED) && (S <= 0 || t > S)) return SPK_ERR_ARG;
  if (LISTED && (!steps_b || !active || !n_active)) return SPK_ERR_ARG;
  if (SCHED && !sched_w) return SPK_ERR_ARG;
  if (REMASK && (!remask_r || !commit_conf_inout || (mask_id >= 0 && mask_id < K))) return SPK_ERR_ARG;
  if (HW > 64 || K > 64 * 32) return SPK_ERR_UNSUPPORTED;      // (one wave ranks an image: lane = position)
  spk_sched_arg_t<REMASK> sc;
  sc.w = sched_w; sc.a = noise_a_or_null; sc.u_in = u_or_null; sc.score_out = score_out_or_null; sc.S = S;
  if constexpr (REMASK) { sc.r = remask_r; sc.commit_conf = commit_conf_inout; sc.remasked_out = remasked_out_or_null; sc.mask_id = mask_id; }
#define SPK_PSAMPLE_CONF_LAUNCH(KPL)                                                                                     \
  if constexpr (SCHED)                                                                                                   \
    hipLaunchKernelGGL((psample_conf_sched_kernel<KPL, LISTED, REMASK>), dim3(B), dim3(256), 0, stream, logits, x_t_inout,      \
                       unmasked_inout, t, temp, q_or_null, philox_seed, philox_offset, philox_state_or_null, x0_hat_out_or_null, \
                       conf_out_or_null, sc, steps_b, step_stride, active, n_active, B, HW, K, next_input_or_null,       \
                       (float)(t - 1));                                                                                  \
  else if constexpr (LISTED)                                                                                             \
    hipLaunchKernelGGL((psample_conf_listed_kernel<KPL>), dim3(B), dim3(256), 0, stream, logits, x_t_inout, unmasked_inout, t, temp, \
                       q_or_null, philox_seed, philox_offset, philox_state_or_null, x0_hat_out_or_null, conf_out_or_null, steps_b, S, \
                       step_stride, active, n_active, B, HW, K);                                                         \
  else                                                                                                                   \
    hipLaunchKernelGGL((psample_conf_kernel<KPL>), dim3(B), dim3(256), 0, stream, logits, x_t_inout, unmasked_inout, t, temp, \
                       q_or_null, philox_seed, philox_offset, philox_state_or_null, x0_hat_out_or_null, conf_out_or_null, HW, K, \
                       next_input_or_null, (float)(t - 1))
  if (K <= 256) { SPK_PSAMPLE_CONF_LAUNCH(4); }
  else if (K <= 512) { SPK_PSAMPLE_CONF_LAUNCH(8); }
  else if (K <= 1024) { SPK_PSAMPLE_CONF_LAUNCH(16); }
  else { SPK_PSAMPLE_CONF_LAUNCH(32); }
#undef SPK_PSAMPLE_CONF_LAUNCH
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
}  // namespace

extern "C" int spk_psample_step_conf(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                     const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                                     const float* q_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                                     const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null,
                                     float* conf_out_or_null, int B, int HW, int K, float* next_input_b2hw_or_null,
                                     hipStream_t stream) {
  return psample_conf_launch<false, false>(logits_bkhw, x_t_inout, unmasked_inout, t, spk_temp_topp{temp_b, topk_b, topp_b}, u_or_null,
                                           q_or_null, philox_seed, philox_offset, philox_state_or_null, x0_hat_out_or_null,
                                           conf_out_or_null, B, HW, K, nullptr, 0, 0ull, nullptr, nullptr, next_input_b2hw_or_null,
                                           nullptr, nullptr, nullptr, stream);
}

// The confidence-ordered update on the list of pending images, each at its own step count (include/spkdiff.h).
extern "C" int spk_psample_step_conf_listed(const float* logits_skhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                            const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                                            const float* q_or_null, unsigned long long philox_seed,
                                            unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                                            long long* x0_hat_out_or_null, float* conf_out_or_null, int B, int HW, int K,
                                            const int* steps_b, int S, unsigned long long step_stride, const int* active,
                                            const int* n_active, hipStream_t stream) {
  return psample_conf_launch<true, false>(logits_skhw, x_t_inout, unmasked_inout, t, spk_temp_topp{temp_b, topk_b, topp_b}, u_or_null,
                                          q_or_null, philox_seed, philox_offset, philox_state_or_null, x0_hat_out_or_null,
                                          conf_out_or_null, B, HW, K, steps_b, S, step_stride, active, n_active, nullptr, nullptr,
                                          nullptr, nullptr, stream);
}

extern "C" int spk_psample_step_conf_sched(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                           const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                                           const float* q_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                                           const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null,
                                           float* conf_out_or_null, int B, int HW, int K, float* next_input_b2hw_or_null,
                                           const uint32_t* sched_w, const float* noise_a_or_null, int S, float* score_out_or_null,
                                           hipStream_t stream) {
  return psample_conf_launch<false, true>(logits_bkhw, x_t_inout, unmasked_inout, t, spk_temp_topp{temp_b, topk_b, topp_b}, u_or_null,
                                          q_or_null, philox_seed, philox_offset, philox_state_or_null, x0_hat_out_or_null,
                                          conf_out_or_null, B, HW, K, nullptr, S, 0ull, nullptr, nullptr, next_input_b2hw_or_null,
                                          sched_w, noise_a_or_null, score_out_or_null, stream);
}

extern "C" int spk_psample_step_conf_listed_sched(const float* logits_skhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                                  const float* temp_b, const int* topk_b, const float* topp_b,
                                                  const float* u_or_null, const float* q_or_null, unsigned long long philox_seed,
                                                  unsigned long long philox_offset,
                                                  const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null,
                                                  float* conf_out_or_null, int B, int HW, int K, const int* steps_b, int S,
                                                  unsigned long long step_stride, const int* active, const int* n_active,
                                                  const uint32_t* sched_w, const float* noise_a_or_null,
                                                  float* score_out_or_null, hipStream_t stream) {
  return psample_conf_launch<true, true>(logits_skhw, x_t_inout, unmasked_inout, t, spk_temp_topp{temp_b, topk_b, topp_b}, u_or_null,
                                         q_or_null, philox_seed, philox_offset, philox_state_or_null, x0_hat_out_or_null,
                                         conf_out_or_null, B, HW, K, steps_b, S, step_stride, active, n_active, nullptr, sched_w,
                                         noise_a_or_null, score_out_or_null, stream);
}

// The two scheduled updates with remasking (include/spkdiff.h; the rule: psample_common.h): the `_sched` siblings'
// arguments plus the remask table, the commit confidences (in place), mask_id and the optional record of what was remasked.
extern "C" int spk_psample_step_conf_remask(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                            const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                                            const float* q_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                                            const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null,
                                            float* conf_out_or_null, int B, int HW, int K, float* next_input_b2hw_or_null,
                                            const uint32_t* sched_w, const float* noise_a_or_null, int S, float* score_out_or_null,
                                            const uint32_t* remask_r, float* commit_conf_inout, long long mask_id,
                                            uint8_t* remasked_out_or_null, hipStream_t stream) {
  return psample_conf_launch<false, true, true>(logits_bkhw, x_t_inout, unmasked_inout, t, spk_temp_topp{temp_b, topk_b, topp_b},
                                                u_or_null, q_or_null, philox_seed, philox_offset, philox_state_or_null,
                                                x0_hat_out_or_null, conf_out_or_null, B, HW, K, nullptr, S, 0ull, nullptr, nullptr,
                                                next_input_b2hw_or_null, sched_w, noise_a_or_null, score_out_or_null, stream, remask_r,
                                                commit_conf_inout, mask_id, remasked_out_or_null);
}

extern "C" int spk_psample_step_conf_listed_remask(const float* logits_skhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                                   const float* temp_b, const int* topk_b, const float* topp_b,
                                                   const float* u_or_null, const float* q_or_null, unsigned long long philox_seed,
                                                   unsigned long long philox_offset,
                                                   const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null,
                                                   float* conf_out_or_null, int B, int HW, int K, const int* steps_b, int S,
                                                   unsigned long long step_stride, const int* active, const int* n_active,
                                                   const uint32_t* sched_w, const float* noise_a_or_null,
                                                   float* score_out_or_null, const uint32_t* remask_r, float* commit_conf_inout,
                                                   long long mask_id, uint8_t* remasked_out_or_null, hipStream_t stream) {
  return psample_conf_launch<true, true, true>(logits_skhw, x_t_inout, unmasked_inout, t, spk_temp_topp{temp_b, topk_b, topp_b},
                                               u_or_null, q_or_null, philox_seed, philox_offset, philox_state_or_null,
                                               x0_hat_out_or_null, conf_out_or_null, B, HW, K, steps_b, S, step_stride, active,
                                               n_active, nullptr, sched_w, noise_a_or_null, score_out_or_null, stream, remask_r,
                                               commit_conf_inout, mask_id, remasked_out_or_null);
}
