// The token update of a reverse step, defined once for the sampler kernels (psample.hip, pscore.hip, step_tail.hip): the Philox4x32-10
// counter scheme of spk_psample_step behind reveal_u (u: stream 0, counter offset + position * K) and race_q (q: stream 1, counter
// offset + position * K + class), the categorical draw categorical_race, the top-k and nucleus truncations truncate_top_k /
// truncate_top_p that may precede it, the confidence-ordered reveal rule confident_reveal (what a step commits when it does not toss
// the coin) with its scheduled form (sched_reveal_count, sched_score, confident_reveal_sched) and the remask that returns the least trusted commits to the masked state
// (confident_remask), the 64-lane max / sum and the prologues every kernel shares.
// Every kernel that draws noise goes through these: every launch form and spk_philox_noise see the same draws.
#pragma once
#include "spk_common.h"
#include <math.h>

namespace {

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
  uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
  uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// Philox4x32-10: counter (index, stream) , key = seed
__device__ __forceinline__ void philox4x32(unsigned long long seed, unsigned long long index, uint32_t stream,
                                            uint32_t (&out)[4]) {
  uint32_t c[4] = {(uint32_t)index, (uint32_t)(index >> 32), stream, 0u};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}

__device__ __forceinline__ float u01_open_left(uint32_t r) {   // (0, 1]
  return ((float)(r >> 8) + 1.0f) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float u01_open_right(uint32_t r) {  // [0, 1)
  return (float)(r >> 8) * (1.0f / 16777216.0f);
}

// The uniform of the `changes` test of a reverse step at image position p (R/snn_model/vq_diffusion.py:116): injected, or stream 0
// at counter offset + p * K.  changes = (u < 1.0f / (float)t) & ~unmasked in fp32; the sampling kernel, the scoring kernel
// (pscore.hip), the fused step tail and the two select kernels all take their u from here.
__device__ __forceinline__ float reveal_u(const float* __restrict__ u_in, unsigned long long seed, unsigned long long offset,
                                          long long p, int K) {
  if (u_in) return u_in[p];
  uint32_t r[4];
  philox4x32(seed, offset + (unsigned long long)p * (unsigned long long)K, 0u, r);
  return u01_open_right(r[0]);
}

// The exponential of the race for class k at image position p: injected, or -log of a (0, 1] uniform, stream 1 at offset + p * K + k.
__device__ __forceinline__ float race_q(const float* __restrict__ q_in, unsigned long long seed, unsigned long long offset,
                                        long long p, int K, int k) {
  if (q_in) return q_in[p * K + k];
  uint32_t r[4];
  philox4x32(seed, offset + (unsigned long long)(p * K + k), 1u, r);
  return -logf(u01_open_left(r[0]));
}

// A captured (hipGraph) launch bakes its arguments: its Philox key / base come from {seed, base offset} the host updates per replay.
__device__ __forceinline__ void philox_base(const unsigned long long* __restrict__ state, unsigned long long& seed, unsigned long long& offset) {
  if (state) { seed = state[0]; offset += state[1]; }
}
// Active-set form (spk_select_active): how many slots of the list a launch sized for B images works on; B without a list.
__device__ __forceinline__ int spk_active_count(const int* __restrict__ active, const int* __restrict__ n_active, int B) {
  return active ? (*n_active < B ? *n_active : B) : B;
}
// (dense form) the denoiser input of the next reverse step, cat(x_t, t - 1), at position hw of logits slot b
__device__ __forceinline__ void write_next_input(float* __restrict__ next_input, int b, int hw, int HW, float token, float t_next) {
  float* dst = next_input + (long long)b * 2 * HW + hw;         // [B][2][HW]: plane 0 the token, plane 1 the step
  dst[0] = token;
  dst[HW] = t_next;
}

// The temperature argument of the token-update kernels (psample.hip, pscore.hip, step_tail.hip): one fp32 value for the call, or --
// PT, the `_temps` entry points -- a device array fp32 [B] indexed by IMAGE (the index of x_t / unmasked / the noise, not the slot of
// an active list).  Both forms divide the logit by the value in the same fp32 division, so an image whose entry equals the scalar
// gets the scalar call's results bit for bit.  The host can check a value (> 0), of an array only the pointer.
// TK, the `_topk` entry points (top-k truncation, below): the argument is the pair of per-image arrays, temperatures fp32 [B] and k
// int32 [B], both indexed by IMAGE.  The scalar and `_temps` kernels keep the argument they always had.
// TP, the `_topp` entry points (nucleus truncation after the top-k one, below; always with PT and TK): the triple of per-image arrays,
// temperatures fp32 [B], k int32 [B] and p fp32 [B].  One family serves top-k and top-p together.
struct spk_temp_topk { const float* temp; const int* topk; };
struct spk_temp_topp { const float* temp; const int* topk; const float* topp; };
template <bool PT, bool TK = false, bool TP = false> struct spk_temp_arg { using type = float; };
template <> struct spk_temp_arg<true, false, false> { using type = const float*; };
template <> struct spk_temp_arg<true, true, false> { using type = spk_temp_topk; };
template <> struct spk_temp_arg<true, true, true> { using type = spk_temp_topp; };
template <bool PT, bool TK = false, bool TP = false> using spk_temp_arg_t = typename spk_temp_arg<PT, TK, TP>::type;

template <bool PT, bool TK = false, bool TP = false>
__device__ __forceinline__ float spk_temp_of(spk_temp_arg_t<PT, TK, TP> temp, int image) {
  static_assert(PT || !TK, "the truncating kernels take per-image arrays");
  static_assert(TK || !TP, "the nucleus kernels take the top-k array too");
  if constexpr (TK) return temp.temp[image];
  else if constexpr (PT) return temp[image];
  else return temp;
}
template <bool PT, bool TK = false, bool TP = false>
inline bool spk_temp_arg_ok(spk_temp_arg_t<PT, TK, TP> temp) {
  if constexpr (TP) return temp.temp != nullptr && temp.topk != nullptr && temp.topp != nullptr;
  else if constexpr (TK) return temp.temp != nullptr && temp.topk != nullptr;
  else if constexpr (PT) return temp != nullptr;
  else return temp > 0.f;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// The entry of l (class lane + 64 * j in l[j]) for class `cls`, in every lane: cls is wave-uniform.
template <int NJ>
__device__ __forceinline__ float spk_race_conf(const float (&l)[NJ], int cls) {
  float c = l[0];
#pragma unroll
  for (int j = 1; j < NJ; ++j) c = (cls >> 6) == j ? l[j] : c;
  return __shfl(c, cls & 63);
}

// x0_hat = Categorical(logits = l).sample() of one position, by one wave: l[j] is the temperature-scaled logit of class lane + 64 * j
// (-inf for a class >= K; overwritten).  probs = softmax(l - logsumexp l), the draw argmax_k probs_k / q_k (torch.multinomial's one-draw
// path), ties to the lower class; every lane returns it.  These fp32 operations in this order are the definition (-ffp-contract=off).
// CONF (the confidence-ordered reveal, below): *conf also receives, in every lane, the value l holds for the drawn class after the
// `l[j] = l[j] - lse` line -- the log-probability of the token under the row as it was raced.  Nothing new is computed.
template <int NJ, bool CONF = false>
__device__ __forceinline__ int categorical_race(float (&l)[NJ], int lane, int K, const float* __restrict__ q_in,
                                                unsigned long long seed, unsigned long long offset, long long p,
                                                float* conf = nullptr) {
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < NJ; ++j) mx = fmaxf(mx, l[j]);
  mx = wave_max(mx);
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) se += (lane + 64 * j < K) ? expf(l[j] - mx) : 0.f;
  se = wave_sum(se);
  const float lse = mx + logf(se);
  float e[NJ];
  float mx2 = -INFINITY;
#pragma unroll
  for (int j = 0; j < NJ; ++j) { l[j] = l[j] - lse; mx2 = fmaxf(mx2, l[j]); }
  mx2 = wave_max(mx2);
  float se2 = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) { e[j] = (lane + 64 * j < K) ? expf(l[j] - mx2) : 0.f; se2 += e[j]; }
  se2 = wave_sum(se2);
  float best = -INFINITY;
  // a position without a single comparable ratio (a NaN logit, or every logit -inf: all ratios NaN) gets token 0 --
  // torch.argmax's answer for an all-NaN row; a valid ratio is >= 0 and always beats this start
  int besti = 0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int k = lane + 64 * j;
    if (k < K) {
      const float ratio = (e[j] / se2) / race_q(q_in, seed, offset, p, K, k);
      if (ratio > best) { best = ratio; besti = k; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(besti, off);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  if constexpr (CONF) *conf = spk_race_conf<NJ>(l, besti);
  return besti;
}

// Top-k truncation of one position's temperature-scaled logits, ahead of categorical_race: tau = the k-th
// largest of the row's non-NaN l (classes < K, counting multiplicity), every class with l < tau becomes -inf; classes equal to
// tau all stay, a NaN is never replaced, and k <= 0 or k >= K leaves the row as it is.  An exact order statistic, no sort and no
// LDS: every fp32 maps to a 32-bit key that orders as the floats do (sign bit flipped for v >= 0, all bits for v < 0), and tau's
// key is built from its top bit down -- the largest key T with at least k candidates >= T, counted over the wave by ballot.  Key 0
// is the bit pattern of a NaN, so it marks what does not count (a NaN, a class >= K); fewer than k candidates leave T = 0, whose
// float is a NaN: nothing is below it.  The keep test is the float comparison (-0.0 and +0.0 are equal), not a key comparison.
// Wave-uniform arguments K, k; every lane ends with the same tau.
template <int NJ>
__device__ __forceinline__ void truncate_top_k(float (&l)[NJ], int lane, int K, int k) {
  if (k <= 0 || k >= K) return;
  uint32_t key[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const uint32_t b = __float_as_uint(l[j]);
    const bool counts = (lane + 64 * j < K) && !(l[j] != l[j]);
    key[j] = counts ? ((b & 0x80000000u) ? ~b : (b | 0x80000000u)) : 0u;
  }
  uint32_t T = 0u;
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t trial = T | (1u << bit);
    int n = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) n += __popcll(__ballot(key[j] >= trial));
    if (n >= k) T = trial;
  }
  const float tau = __uint_as_float((T & 0x80000000u) ? (T & 0x7FFFFFFFu) : ~T);
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (l[j] < tau) l[j] = -INFINITY;
}

// Nucleus (top-p) truncation of one position's temperature-scaled logits, after truncate_top_k and ahead of categorical_race
// (DESIGN.md §4.14): the smallest set of top classes, closed under ties, whose probability mass reaches p of the row's.  The cut is
// exact integer arithmetic after one expf per class: with mx the row maximum (fmaxf: NaNs ignored), class c weighs
// m_c = (uint32) rint(expf(l_c - mx) * 2^20) (0 for a NaN, a class >= K and a class at -inf, top-k's among them), total = sum m_c
// <= 2048 * 2^20 = 2^31, P = (double)p * (double)total (one fp64 product), and tau's key is the largest key T -- the keys of
// truncate_top_k -- with (double)S(T) >= P, S(T) = the sum of m_c over the classes with key_c >= T, built from bit 31 down with one
// compare and one add per held class and a uint32 wave sum (spk_wave_sum_u32, spk_common.h) per step.  S falls as T rises, so the bit descent finds that T, and
// T is the key of a class with m_c > 0 (the maximum's 2^20 makes S(smallest key) = total > P).  Every class with l < tau (the float
// comparison) becomes -inf: classes equal to tau all stay, the row maximum always stays, a NaN is never replaced.  !(0 < p < 1) --
// 1, 0, a negative, a NaN -- and a row whose maximum is not finite leave the row as it is.  No LDS, no sort, no data-dependent loop;
// integer sums do not depend on their order, so a permutation of lanes or classes cannot move tau.  Wave-uniform arguments K, p.
template <int NJ>
__device__ __forceinline__ void truncate_top_p(float (&l)[NJ], int lane, int K, float p) {
  if (!(p > 0.f && p < 1.f)) return;
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < NJ; ++j) mx = fmaxf(mx, (lane + 64 * j < K) ? l[j] : -INFINITY);
  mx = wave_max(mx);
  if (!(fabsf(mx) < INFINITY)) return;
  uint32_t key[NJ], m[NJ];
  uint32_t total = 0u;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const uint32_t b = __float_as_uint(l[j]);
    const bool counts = (lane + 64 * j < K) && !(l[j] != l[j]);
    key[j] = counts ? ((b & 0x80000000u) ? ~b : (b | 0x80000000u)) : 0u;
    m[j] = counts ? (uint32_t)rintf(expf(l[j] - mx) * 1048576.0f) : 0u;
    total += m[j];
  }
  total = spk_wave_sum_u32(total);
  const double P = (double)p * (double)total;
  uint32_t T = 0u;
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t trial = T | (1u << bit);
    uint32_t s = 0u;
#pragma unroll
    for (int j = 0; j < NJ; ++j) s += key[j] >= trial ? m[j] : 0u;
    s = spk_wave_sum_u32(s);
    if ((double)s >= P) T = trial;
  }
  const float tau = __uint_as_float((T & 0x80000000u) ? (T & 0x7FFFFFFFu) : ~T);
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (l[j] < tau) l[j] = -INFINITY;
}

// The confidence-ordered reveal (spk_psample_step_conf, spk_den_step_tail_conf) -- THE rule, stated once.  At
// reverse step t, for each image on its own:
//   1. m = the number of positions masked at entry, n = (m + t - 1) / t in integer arithmetic (ceil(m / t): everything at t = 1);
//   2. every masked position p gets a candidate: the unchanged race on the temperature-scaled logits after truncate_top_k and
//      truncate_top_p, noise of stream 1 at offset + p * K + class -- bit for bit the x0_hat of the `_topp` entry points.  The
//      stream-0 uniform of reveal_u is neither drawn nor read (its counter stays free), an injected u is ignored;
//   3. the confidence of p is the fp32 value categorical_race holds for the drawn class after `l[j] = l[j] - lse` (CONF above);
//      its order key is the 32-bit key of truncate_top_k (spk_conf_key: a NaN has key 0 and orders last);
//   4. p is revealed iff fewer than n masked positions p' of the image have (key, -p') above (key, -p): larger key first, equal
//      keys to the lower position.  A revealed position takes its candidate and unmasked = 1, every other keeps its state.
// confident_reveal is step 4 for one image by ONE wave, lane = position (h*w <= 64): `masked` = this lane's position is masked at
// entry (false for lane >= h*w), s_key = the image's keys in LDS (read at masked positions only; the writes are behind a barrier).
__device__ __forceinline__ uint32_t spk_conf_key(float conf) {
  const uint32_t b = __float_as_uint(conf);
  return (conf != conf) ? 0u : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
}
__device__ __forceinline__ bool confident_reveal(bool masked, int lane, int HW, int t, const uint32_t* s_key) {
  const unsigned long long mm = __ballot(masked);
  const unsigned m = (unsigned)__popcll(mm);
  const unsigned n = (m + (unsigned)t - 1u) / (unsigned)t;
  const uint32_t key = masked ? s_key[lane] : 0u;
  unsigned rank = 0;
  for (int q = 0; q < HW; ++q) {
    if (!((mm >> q) & 1ull)) continue;                            // (wave-uniform)
    const uint32_t kq = s_key[q];                                 // (one address for the wave: a broadcast read)
    rank += (kq > key || (kq == key && q < lane)) ? 1u : 0u;
  }
  return masked && rank < n;
}

// Reveal schedules and annealed selection noise (the `_sched` entry points spk_psample_step_conf_sched,
// spk_psample_step_conf_listed_sched, spk_den_step_tail_conf_sched) -- THE rule, stated once.  Steps 2 and 3 above stay as they
// are (the candidates, their stream-1 counters, the truncation, the fp32 confidence: x0_hat_out and conf_out are bit for bit the
// `_conf` sibling's whatever the tables hold); steps 1 and 4 take two per-image tables indexed [image][t], t = 0 .. S:
//   1'. HOW MANY.  w = row i of sched_w (uint32 [B][S + 1], entries <= 2^24).  In unsigned 64-bit arithmetic
//         keep = w[t] == 0 ? 0 : min(m, (m * w[t - 1]) / w[t]);   n = m - keep;   m > 0 and n == 0: n = 1
//       (sched_reveal_count: m <= 64 and w <= 2^24, so the product is below 2^31).  w[t - 1] == 0 reveals everything -- t = 1 under
//       w[0] = 0 --, w[t] = t gives m - floor(m (t - 1) / t) = ceil(m / t), the `_conf` count, and a non-monotone table is legal:
//       the min and the forced 1 are what it means.
//   4'. IN WHAT ORDER.  a = noise_a[i][t] (fp32 [B][S + 1]; a null table: a = 0).  a == 0: nothing is drawn, score = conf.  Else
//       u = reveal_u of the position -- the injected u, or stream 0 at offset + p * K, the coin's own counter that the `_conf`
//       kernels leave undrawn, a value in [0, 1) -- and, every operation one fp32 rounding (-ffp-contract=off):
//         g = -logf(-logf(u));   score = conf + a * g      (sched_score)
//       u = 0 gives g = -inf, so score = -inf under a > 0: such a position orders last among the numbers, ahead of the NaNs (key 0).
//       The order key is spk_conf_key(score), the rank rule is confident_reveal's: (key, -position), ties to the lower position.
//       score_out receives the score at the positions masked at entry.
__device__ __forceinline__ unsigned sched_reveal_count(unsigned m, uint32_t w_prev, uint32_t w_cur) {   // w[t - 1], w[t]
  const unsigned long long wp = w_prev, wc = w_cur, mu = m;
  unsigned long long keep = 0ull;
  if (wc != 0ull) { keep = (mu * wp) / wc; keep = keep < mu ? keep : mu; }
  unsigned n = (unsigned)(mu - keep);
  if (m > 0u && n == 0u) n = 1u;
  return n;
}
__device__ __forceinline__ float sched_score(float conf, float a, const float* __restrict__ u_in, unsigned long long seed,
                                             unsigned long long offset, long long p, int K) {
  if (a == 0.f) return conf;
  const float u = reveal_u(u_in, seed, offset, p, K);
  const float g = -logf(-logf(u));
  const float ag = a * g;
  return conf + ag;
}
__device__ __forceinline__ bool confident_reveal_sched(bool masked, int lane, int HW, uint32_t w_prev, uint32_t w_cur,
                                                       const uint32_t* s_key) {
  // (confident_reveal with the count from the table: a copy of its eight lines, so that the `_conf` kernels keep the text they have)
  const unsigned long long mm = __ballot(masked);
  const unsigned n = sched_reveal_count((unsigned)__popcll(mm), w_prev, w_cur);
  const uint32_t key = masked ? s_key[lane] : 0u;
  unsigned rank = 0;
  for (int q = 0; q < HW; ++q) {
    if (!((mm >> q) & 1ull)) continue;                            // (wave-uniform)
    const uint32_t kq = s_key[q];                                 // (one address for the wave: a broadcast read)
    rank += (kq > key || (kq == key && q < lane)) ? 1u : 0u;
  }
  return masked && rank < n;
}

// Remasking (the `_remask` entry points spk_psample_step_conf_remask, spk_psample_step_conf_listed_remask,
// spk_den_step_tail_conf_remask) -- THE rule, stated once.  On top of the `_sched` rule only; a null noise_a is a = 0, w[t] = t gives
// the ceil(m / t) counts.  One more piece of per-position state, commit_conf (fp32 [B*HW], in place like x_t / unmasked): +inf at the
// positions unmasked when the run started (the `known` tokens, never revisited -- a committed log-probability is <= 0, so +inf
// cannot arise otherwise), the confidence of its reveal at a position a step revealed, anything (ignored) at a masked position.  The
// denoiser is not trained at unmasked positions (the loss ignores them), so a committed token is never re-scored from the current
// logits: its trust IS the confidence it was committed with.  At reverse step t, for each image on its own:
//   1. m = positions masked at entry.  m == 0: the image is left as the `_sched` sibling leaves it -- no remask either.
//   2. candidates, confidences, scores, the count n and the revealed set are the `_sched` rule's: x0_hat_out, conf_out, score_out and
//      the revealed positions are bit for bit the sibling's on the same state and tables.
//   3. REMASK.  p is revisable iff it was unmasked at entry and commit_conf[p] != +inf (a position revealed in this step is not).
//      c = the number of revisable positions, r = min(remask_r[i][t], c), and r = 0 at t = 1 whatever the table holds: a run never
//      ends with a masked position.  Order key = spk_conf_key(commit_conf[p]) (a NaN: key 0).  A revisable p is remasked iff fewer
//      than r revisable p' have (key, -p') below (key, -p): smaller key first, equal keys to the HIGHER position -- the mirror image
//      of the reveal, so one total order (key, -position) serves both ends.  A remasked p gets x_t = mask_id, unmasked = 0; its
//      commit_conf stays.  It draws again at the NEXT step, after a denoiser call has seen it masked.
//   4. every revealed p gets commit_conf[p] = its confidence -- conf_out's value, not the Gumbel-perturbed score.
//   5. next_input and the fused first layer of the next step read the state after 3 and 4: a remasked position shows mask_id.
// confident_remask is step 3 for one image by ONE wave, lane = position: `revisable` as above (false for lane >= h*w), r_tab the
// table entry (the caller zeroes it at t = 1 and for m == 0), s_key = the image's keys in LDS (read at revisable positions only).
__device__ __forceinline__ bool confident_remask(bool revisable, int lane, int HW, uint32_t r_tab, const uint32_t* s_key) {
  const unsigned long long rv = __ballot(revisable);
  const unsigned c = (unsigned)__popcll(rv);
  const unsigned r = r_tab < c ? r_tab : c;
  if (r == 0u) return false;                                      // (wave-uniform)
  const uint32_t key = revisable ? s_key[lane] : 0u;
  unsigned rank = 0;
  for (int q = 0; q < HW; ++q) {
    if (!((rv >> q) & 1ull)) continue;                            // (wave-uniform)
    const uint32_t kq = s_key[q];                                 // (one address for the wave: a broadcast read)
    rank += (kq < key || (kq == key && q > lane)) ? 1u : 0u;
  }
  return revisable && rank < r;
}

}  // namespace
