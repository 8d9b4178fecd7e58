// Second-generation 3x3 spike convolution for the denoiser's conv2..conv5 (R/snn_model/vq_diffusion.py:166-184,201-204;
// SURVEY.md §8 a8) on the CDNA4 block-scaled MFMA -- the sampler's fast path (7x7 latents, fresh LIF state).  Same results,
// bit for bit, as den_mfma_fp6.hip (the correctly rounded value of the exact 29-bit fixed-point dot product, then the
// reference's fp32 BN and LIF arithmetic); what changes is how much matrix and vector work it takes to get there.
//
// 1. DIGIT PAIRS SHARE AN ACCUMULATOR.  v_mfma_scale_f32_32x32x64_f8f6f4 takes one E8M0 scale per operand row / column and
//    32-wide K block, i.e. per lane.  The two K halves of an instruction carry the SAME 32 input channels with two
//    adjacent radix-32 digits of the weights, the even digit scaled by 2^8 and the odd one by 2^3 (e2m3 holds d/8): the
//    fp32 accumulator then holds 32 * D_even + D_odd directly -- an integer below 4608 * 528 < 2^24, still exact.  The
//    column tile is 32 output channels of one digit pair, so the three values of a neuron-step (pairs 01, 23 and the
//    fifth digit) sit in ONE lane: no cross-lane exchange in the epilogue, and all 64 lanes scan their own neuron.
// 2. FOUR DIGITS ON THE MATRIX CORES, THE LAST TWO ONLY WHERE THEY MATTER.  The fifth and sixth digit move a pre-activation by
//    at most 528 units of 2^-s per ACTIVE input.  The main kernel multiplies the four leading digits (18 instead of 27 MFMAs
//    per row tile and 32-channel chunk: two digit pairs per tap; 15.25 on average on full 7x7 items, whose border tiles leave
//    out the taps that read only the zero border: "BORDER SKIP" below), counts the active inputs of every row while their fragments
//    pass through its registers (four v_bcnt per fragment), recombines in fp32, and CERTIFIES every spike decision: every
//    neuron carries a running bound D_t on |h_approx - h_exact| (the dropped digits for the counted inputs of each step, the
//    fp32 recombination and every rounding of BN / LIF on either path, see "Certification" below) and is flagged when its
//    membrane potential ever comes within D_t of the threshold (1 - 6e-4 of the neurons at the denoiser's firing rates of
//    3 - 7 %).  The fixup launch recomputes the flagged neurons EXACTLY (all six digits as the pack kernel's int32 quantised
//    weights, 64-bit sums, fp64 recombination, one rounding: the arithmetic of den_mfma_fp6.hip) and patches their spikes.
//    The flag workspace with its protocol (flag, hand-over, scan), the pieces of that recomputation and the weight tile format are
//    shared with vae_fp6.hip: cert_common.h.
//    Unflagged neurons provably emit the spikes the exact arithmetic would; flagged ones are the exact arithmetic.  Membrane
//    potentials are not an output here (fresh state in, nothing written back): callers that carry LIF state, and the
//    training forward, use den_mfma_fp6.hip.  (The earlier form, five digits on the matrix cores -- 23 MFMAs, the fifth
//    pairing two taps per instruction -- and a bound that takes every input as active, flagged 2 - 3x fewer neurons and was
//    8 - 10 % slower end to end.)
// 3. A WORK ITEM = one image x 32 output channels, K chunk = 32 input channels: the spike slab of an image is fetched half
//    as often, a workgroup keeps ONE channel group for the whole launch (its BN / margin constants are loaded once, its
//    weight slabs stay L2-hot), and two images + two 35 KB weight slabs need 107 KB of LDS.
//
// Spike layout "S32": [B][C/32][H*W][T = 16][16 B], channel c of a group in byte (c % 32) / 2, low nibble first, e2m1 codes
// 0x0 / 0x2.  The last position of a 7x7 latent (the 49th: 24 full 32-row tiles + 1) is computed exactly by the tail
// launch from the same packed weights plus two sixth-digit tiles stored for its four taps.
#include "cert_common.h"
#include "../../include/spkdiff.h"
#include <stdlib.h>
#include <type_traits>
#include <utility>

namespace {

constexpr int CK = 32;                                   // input channels per K chunk: POSB = T16 * CK / 2 bytes per latent position
constexpr int N_PAIR = 18;                               // tiles 0..17: (tap, digit pair 01 | 23)
constexpr int N_D4 = 5;                                  // tiles 18..22: fifth digit, taps (0,1) (2,3) (4,5) (6,7) (8,-)
constexpr int N_MAIN = N_PAIR + N_D4;
constexpr int N_L5 = 2;                                  // tiles 23, 24: sixth digit of taps (0,1) and (3,4), last position only
constexpr int NACC = 2;                                  // accumulators per row tile: digit pairs 01 and 23
constexpr int W_PIECES = (N_PAIR * WT + 1023) / 1024;    // one-KiB DMA pieces per chunk: the main launch multiplies tiles 0..17 (27)
constexpr int W_LDS = W_PIECES * 1024;
constexpr int W_SLAB = ((N_MAIN + N_L5) * WT + 1023) / 1024 * 1024;   // bytes per (channel group, chunk) in memory

struct V2Args {
  const uint8_t* in0; int nch;               // S32 spikes, nch = Cin / 32
  const uint8_t* wq; const double* scale; const double* bias; const float* wl1;
  const float* bn_a; const float* bn_b;
  uint8_t* out; uint8_t* out_cnt;
  CertWs ws;                                 // the flag workspace (cert_common.h, spk_den_fp6v2_flag_words)
  int handover;                              // 1: the main launch publishes the count (fp6v2_handover); 0: the tail launches read
                                             //    ws[0] and the last-position launch, which follows the repair launch, re-arms it
  const int* qtab;                           // quantised weights int32 [Cout][9][Cin] (exact recomputation)
  const int* n_dyn;
  // position lists (spk_select_needed, one radius): 64-byte record per image slot; the slots by tile count (classes
  // 1..6 tiles per wave): cls_cnt[k - 1] slots listed in cls_list[(k - 1) * B ..]
  const uint8_t* need; const int* cls_cnt; const int* cls_list;
  int B, Cout, Cin;
  int gx, nsets;                             // XCD-aware walk (gx > 0) or flat walk (gx == 0)
};

constexpr int SPK_V2_KMIN = 2;          // listed positions: an item of fewer tiles per wave still costs about this many (operand copies)
constexpr float SPK_V2_SPARE = 1.0f;    // factor on the certification bound (2.0f = the first builds' spare factor)
constexpr int SPK_V2_REC_STEP = 13;     // the K-loop step (= two MFMAs) whose gap takes the record popcounts (the reads are issued at step 1; 7: no gain, 13: +0.4 %)
// Accumulators of the two-waves-per-SIMD kernels stay in VGPRs (243 registers, no scratch; the round-2/3 form with eight tiles in AGPRs:
// dense reverse process 91.2 / 92.4 against 90.6 / 90.2 ms, profiles/r4_ab_kernel_variants.txt).
// Full 7x7 batches run repair + last position as ONE tail launch (hand-over by the main launch): 1.6 % faster than two launches
// (90.3 / 90.2 against 91.2 / 92.4 ms).
// (Spike decisions kept as 64-bit lane masks and stored through v_writelane: 0.2 % slower, round 4: 90.47 / 90.73 / 90.46 against
//  90.41 / 90.35 / 90.15 ms per dense reverse process.)
// (The exact repair staging a neuron's weights in LDS: den.conv5 376.5 against 355.5 us, profiles/r5_ab_kernel_variants.txt (8).)
// The sixteen spike bits of a lane are shifted in from the sign of h - 1 (one v_alignbit per step, one bit reversal per tile):
// dense reverse process 88.84 -> 88.33 ms against sixteen selects (profiles/r4_ab_kernel_variants.txt (13)).
constexpr int SPK_V2_LP_PAIRS = 1;      // last-position part of the tail launch: image pairs (32-row tiles) per unit.  2 halves the weight-tile
                                        // reads and needs 146 + 96 registers: +1.8 % on the dense reverse process (86.8 -> 88.4 ms,
                                        // profiles/r4_ab_kernel_variants.txt) -- the launch is bound by chains of dependent reads, not L2 bandwidth
constexpr int SPK_V2_GX_KB = 2560;      // XCD-aware walk: packed weights of the channel groups one XCD keeps (its L2 is 4 MB).  Round 6, same box
                                        // (profiles/r6_ab_kernel_variants.txt (2)): 1536 (rounds 2-5: four sets of 2 / 4 groups for conv5 / conv4, every
                                        // image slab fetched by four XCDs) -> 2560 (two sets of 4 / 8 groups, 2.4 MB of weights per L2): L2-miss traffic
                                        // of the conv5 / conv4 launches 320 / 194 -> 214 / 150 MB at the SAME time (88.2 ms per batch either way);
                                        // 6144 (one set, 4.9 MB of weights per L2): 312 / 346 MB -- the weights no longer stay resident
constexpr int SPK_V2_HALF_FILL = 2;     // the small-batch split is taken while B x Cout / 32 x this <= workgroups (2: the halves still fit one per CU)
constexpr int SPK_V2_LPS_MIN_B = 64;    // full batches below this take the merged tail launch of the active-set calls (last position per image
                                        // pair from L2 + repairs): the LDS-shared form puts eight images on a workgroup, i.e. B / 8 x Cout / 32
                                        // workgroups -- at R/main.py's own B = 16 that is 2 x G serial chains (12.3 us per launch against 7.4)
constexpr int SPK_V2_LP_SPLIT_MAX = 512;   // last-position part: up to this many units the four waves of a workgroup split a unit's K chunks
                                           // (1024 until round 4; same box, dense / elimination / lists, ms per 100-step sample at B = 256:
                                           //  1024: 88.0 / 43.5 / 34.2, 512: 87.4 / 43.3 / 34.1, 256 and 0: 87.4 / 44.3 / 35.2)
constexpr int SPK_V2_PF = 6;            // four-wave items: A fragments requested this many steps ahead of the MFMA that consumes them
// Full 7x7 items (tap pairs, v2p_sched): register sets of the A-fragment ring per wave class.  The ring must close over a chunk (the
// fragment count -- 15 interior, 9 top / right / left, 11 bottom -- a multiple of the ring, or the ring's last owners dead in time):
// 5 / 3 / 4 sets request a fragment 4-12 / 2 / 2-3 MFMAs ahead of its first use.  The border waves reach the chunk barrier 12-18 MFMAs
// before the interior waves of their SIMD: their shorter distance costs nothing.  (Interior waves on 3 sets, two MFMAs ahead
// everywhere: profiles/tap_pair_ab.txt.)
constexpr int SPK_V2_TP_SLOTS_INT = 5;
constexpr int v2_tp_slots(int cls) { return cls == 0 ? SPK_V2_TP_SLOTS_INT : (cls == 4 ? 4 : 3); }
constexpr int SPK_V2_TP_PFD = 12;       // ... and at most this many MFMAs ahead (one pair block)
constexpr int SPK_V2_TP_TAIL = 6;       // the chunk barrier sits this many MFMAs before the end of the chunk

// Certification.  The approximate path (the leading digits, fp32 recombination, folded constants) and the exact path (six
// digits, fp64 recombination, the reference's BN / LIF operations) run the same LIF recursion on pre-activations that differ by
//   |z~_t - z_t| <= c_t + 2 eps |z_t|
//   c_t = |a| * 528 * 2^-s * n_t + 2 eps (|b| + |Bc|),   n_t = active inputs of the row at step t (counted),
//   |32 d4 + d5| <= 528 per input;
// with eps = 2^-22 (each of the handful of fp32 roundings on either path is <= 2^-24 relative to a quantity bounded by
// |z|, |b| or |Bc|).  One LIF step h = v + (z - v) / 2 halves the carried difference and adds its own roundings:
//   dh_t <= dh_{t-1} / 2 + c_t / 2 + 2 eps (|z_t| + |v_{t-1}|)
// as long as the spike decisions agreed so far (after a spike both paths restart from v = 0; the bound is simply kept).
// The epilogue uses the closed form of the same recursion, dh_t <= max c + 8 eps max |z| (|v| <= max |z|), WITHOUT the spare factor --
// the digit term of c_t is exact (528 is the largest residue there is), eps already holds every rounding 2.5-4 times over, and
// the number of flagged neurons (the repair launch: 7 % of a dense reverse step) is proportional to the bound.  Every
// unflagged neuron provably emits the exact path's spikes; flagged ones are recomputed exactly.  (CERT_4EPS = 4 eps: cert_common.h)

// Store the spikes of one 32-row tile: every lane holds the 16 step bits of its neuron (channel = lane & 31 of the group,
// position = its lane half); a 16x16 bit transpose per 16-lane row gives lane t the 16 channel bits of step t = 8 bytes of
// the (position, t) record.
__device__ __forceinline__ void store_tile_spikes(uint8_t* out, uint8_t* out_cnt, unsigned mybits, int lane, long long rec_base,
                                                  long long cnt_base, bool ok) {
  const unsigned bitsv = spk_transpose16_rows(mybits, lane);
  if (out_cnt && ok) out_cnt[cnt_base + (lane & 31)] = (uint8_t)__popc(mybits);
  if (ok) *reinterpret_cast<uint2*>(out + rec_base + (lane & 15) * 16 + 8 * ((lane >> 4) & 1)) = spk_e2m1_record(bitsv);
}

// NWV = waves per workgroup: 8 (two per SIMD, 3 row tiles each, 256 registers: the partner wave's MFMAs run under this wave's copy
// issue, fragment waits and epilogue, and two waves scanning at once get the SIMD's full vector rate) on full items, 4 (one per
// SIMD) on the half-image items of small batches.
// SPLIT (latents too large for one item, 8x8): an item is one of the two ROW BANDS of an image -- H / 2 output rows, H / 2 + 1
// input rows (one halo row from the other band).  Both bands sit in LDS rows 1 .. H/2 + 1 of a padded image whose rows 0 and
// H/2 + 2 stay zero; the top band's outputs are centred on LDS rows 1.., the bottom band's on rows 2.. (one row offset added
// to the fragment addresses per item).  An even position count needs no last-position launch.
// NTP > 0 (7x7, one wave per SIMD): the row tiles of an item are the positions LISTED for the image (a.need: what the
// sampler will read at this reverse step, dilated by the layers in between) instead of all 48 -- tile k = list entries 2k,
// 2k + 1, round-robin over the waves, NTP = ceil(entries / 8) tiles per wave; `slots` are the image slots with that tile
// count.  Positions outside the list keep whatever the output buffer held: nothing downstream of a listed position reads them.
// Small batches (round 6; R/main.py's own call is B = 16): an image x 32 output channels is ONE item, so a layer with B x Cout / 32
// items below the CU count leaves CUs idle (B = 16: conv2 64, conv3 / conv5 128 items on 256 CUs).  HALF = the listed-positions
// form (NTP = 3 tiles per wave of four) on two FIXED lists per image -- positions 0..23 and 24..47 -- i.e. two items per image, one
// wave per SIMD.  Same arithmetic per position as every other form (bit-equal: test_fp6v2_small_batch_split_...).
__device__ const uint8_t V2_HALF_REC[2][64] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23,
     23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 23, 24},
    {24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47,
     47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 24}};

// BORDER SKIP (full 7x7 items).  A tap that reads only the zero border of the LDS image multiplies nothing: its MFMAs add exactly +0 to
// an exact integer accumulation.  24 of the 49 positions lie on the border and miss 3 of their 9 taps (5 at a corner).  Position 48 is the
// tail launch's; the other 23 are gathered by SIDE, one wave per side, so that both positions of a tile miss the same three taps and the
// whole tap BLOCK -- its MFMAs, its two weight tiles, its fragment reads -- drops out of that wave's K loop:
//   top    0 1 | 2 3 | 4 5            6 taps x 3 tiles   (no taps 0 1 2)
//   right  6 13 | 20 27 | 34 41       6 taps x 3 tiles   (no taps 2 5 8)
//   left   7 14 | 21 28 | 35 42       6 taps x 3 tiles   (no taps 0 3 6)
//   bottom 43 44 | 45 46 | 47 40      6 taps x 3 tiles + taps 6 7 8 on the third tile alone (40 is interior)
//   four interior waves               9 taps x 3 tiles
// i.e. 11 x 6 + 13 x 9 = 183 (tile, tap) steps per chunk instead of 216: 15.25 MFMAs per row tile and chunk on average instead of 18.
// A K loop follows its class's block list: blocks in issue order, each on the LAST nt tiles of the wave.  The bottom wave's one-tile
// blocks come second, not last: behind the chunk barrier nothing may read the current buffers.
//
// TAP PAIRS (full 7x7 items).  A digit-pair MFMA carries the SAME 32 input channels in both K halves, so lanes r and r + 32 read the
// same 16 bytes of the spike record: 1 KB of LDS return traffic per A fragment for 512 distinct bytes.  A PAIR block puts two adjacent
// TAPS (a, a + 1) of ONE digit into the K halves instead: lanes 0-31 read the cell of tap a, lanes 32-63 the cell of tap a + 1, and the
// block issues four MFMAs per row tile -- digit 0 at 2^8 and digit 1 at 2^3 into acc[i][0], digit 2 at 2^8 and digit 3 at 2^3 into
// acc[i][1] -- where two single-tap blocks issued 2 x 2.  The scale is uniform over the lanes; the accumulators hold the same exact
// integers 32 D_even + D_odd (sums of exact products below 2^24: the order is free), so every pre-activation, spike, count and flag is
// bit for bit what the digit-pair form gives.  One A fragment now feeds four MFMAs: 98 fragment reads per chunk instead of 183.  The
// packed weights are untouched: a tile (tap, pair) keeps the even digit in the slots of lanes 0-31 and the odd digit in those of lanes
// 32-63 (16 bytes at lane * 16, 8 bytes at 1024 + lane * 8), so the operand "(tap a | tap a + 1), digit d" is the matching half of tile
// (a, pair) for lanes 0-31 and of tile (a + 1, pair) for lanes 32-63 -- 2 WT further on, ONE constant: two per-lane base registers
// (16-byte and 8-byte part; the odd digit is 512 / 256 bytes behind the even one), every 16-lane group still reading 256 contiguous
// bytes.  A class with an odd number of taps keeps its last tap (8) as a SINGLE block: the two digit-pair MFMAs per tile of every other form.
// Same box, three alternating passes, B = 256 (profiles/tap_pair_ab.txt): dense reverse process 77.79-77.99 -> 76.14-76.66 ms, den.conv4 /
// conv5 main + tail 320-323 / 309 -> 311-313 / 301-304 us; SQ_INSTS_MFMA per den.conv4 launch unchanged, SQ_INSTS_LDS 15.3 M -> 12.6 M,
// SQ_LDS_IDX_ACTIVE 54.2 M -> 43.0 M.
enum : int { V2_INT = 0, V2_TOP, V2_RIGHT, V2_LEFT, V2_BOTTOM, V2_NCLS };
struct V2Plan { int nblk; int tap[9]; int nt[9]; int pair[9]; };   // pair[b] = 1: taps (tap[b], tap[b] + 1) in the K halves
constexpr int V2_FT = 3;                                 // row tiles per wave of a full item
constexpr V2Plan V2_PLAN[V2_NCLS] = {
    {5, {0, 2, 4, 6, 8}, {3, 3, 3, 3, 3}, {1, 1, 1, 1, 0}},
    {3, {3, 5, 7}, {3, 3, 3}, {1, 1, 1}},
    {3, {0, 3, 6}, {3, 3, 3}, {1, 1, 1}},
    {3, {1, 4, 7}, {3, 3, 3}, {1, 1, 1}},
    {5, {0, 6, 8, 2, 4}, {3, 1, 1, 3, 3}, {1, 1, 0, 1, 1}}};
constexpr V2Plan v2_uniform_plan(int nt) {               // every other form: all nine taps on all tiles, one tap per block
  V2Plan p = {9, {0, 1, 2, 3, 4, 5, 6, 7, 8}, {}, {}};
  for (int b = 0; b < 9; ++b) p.nt[b] = nt;
  return p;
}
constexpr int v2_plan_start(const V2Plan& p, int blk) {  // first step (one A fragment: a block x one of its tiles) of a block (blk == nblk: their number)
  int n = 0;
  for (int b = 0; b < blk; ++b) n += p.nt[b];
  return n;
}
constexpr int v2_plan_blk(const V2Plan& p, int s) {      // block of a step
  int b = 0;
  while (s >= p.nt[b]) s -= p.nt[b++];
  return b;
}
constexpr bool v2_plan_has(const V2Plan& p, int b, int tap) { return p.tap[b] == tap || (p.pair[b] && p.tap[b] + 1 == tap); }
// The MFMAs ("ops") of a tap-pair K loop.  A block issues nd = 4 (pair) or 2 (single) B operands on each of its nt tiles, operand
// outer and tile inner: a B operand serves nt consecutive MFMAs and dies, and nt = 3 MFMAs lie between two that accumulate into the
// same register.  Operand `sel` of a pair block is digit sel (accumulator sel >> 1, scale 2^8 / 2^3 for even / odd), of a single
// block the digit-pair tile sel.  A one-tile pair block runs its digits 0 2 1 3 (accumulators 0 1 0 1, as the single blocks do).
constexpr int v2p_nd(const V2Plan& p, int b) { return p.pair[b] ? 4 : 2; }
constexpr int v2p_op_start(const V2Plan& p, int blk) {   // first op of a block (blk == nblk: the number of ops)
  int n = 0;
  for (int b = 0; b < blk; ++b) n += v2p_nd(p, b) * p.nt[b];
  return n;
}
constexpr int v2p_op_blk(const V2Plan& p, int m) {
  int b = 0;
  while (m >= v2p_op_start(p, b + 1)) ++b;
  return b;
}
constexpr int v2p_swap(int q) { return ((q & 1) << 1) | (q >> 1); }   // 0 2 1 3 (its own inverse)
constexpr int v2p_op_sel(const V2Plan& p, int b, int q) { return p.nt[b] > 1 ? q / p.nt[b] : (p.pair[b] ? v2p_swap(q) : q); }
constexpr int v2p_op_tile(const V2Plan& p, int b, int q) { return V2_FT - p.nt[b] + (p.nt[b] > 1 ? q % p.nt[b] : 0); }
constexpr int v2p_b_start(const V2Plan& p, int blk) {    // first B operand of a block (blk == nblk: their number)
  int n = 0;
  for (int b = 0; b < blk; ++b) n += v2p_nd(p, b);
  return n;
}
constexpr int v2p_b_blk(const V2Plan& p, int g) {
  int b = 0;
  while (g >= v2p_b_start(p, b + 1)) ++b;
  return b;
}
// first and last op that reads A fragment f (= step f) / B operand g
constexpr int v2p_a_first(const V2Plan& p, int f) { return v2p_op_start(p, v2_plan_blk(p, f)) + f - v2_plan_start(p, v2_plan_blk(p, f)); }
constexpr int v2p_a_last(const V2Plan& p, int f) { return v2p_a_first(p, f) + (v2p_nd(p, v2_plan_blk(p, f)) - 1) * p.nt[v2_plan_blk(p, f)]; }
constexpr int v2p_b_first(const V2Plan& p, int g) {
  const int b = v2p_b_blk(p, g), sel = g - v2p_b_start(p, b);
  return v2p_op_start(p, b) + (p.nt[b] > 1 ? sel * p.nt[b] : (p.pair[b] ? v2p_swap(sel) : sel));
}
constexpr int v2p_b_last(const V2Plan& p, int g) { return v2p_b_first(p, g) + p.nt[v2p_b_blk(p, g)] - 1; }
// WHEN the reads are issued.  A fragments live in a ring of `nslot` register sets (fragment f in set f % nslot), B operands in four
// (operand sel of a block in set sel).  A read is issued in front of op `at`: as soon as its set is free (the op after the last use
// of the set's previous owner, the previous chunk's if need be: the loop is periodic over the chunks of an item), the A reads not
// more than `pfd` ops ahead of their first use.  at < 0: the read belongs to the previous chunk's tail, at op nm + at, BEHIND that
// chunk's barrier at op mb = nm - tail (in front of it the next chunk's buffers are still being copied) -- or to the prologue of an
// item's first chunk.  ok: every read in front of its first use and behind the last use of its set's previous owner, every read of the
// current buffers in front of the chunk barrier (the reads scheduled AT op mb are issued first, then the barrier).
struct V2Sched { int nf, nb, nm, mb; int a_at[27]; int b_at[36]; int a_dist, b_dist; bool ok; };   // *_dist: fewest ops between a read and its first use
constexpr V2Sched v2p_sched(const V2Plan& p, int nslot, int pfd, int tail) {
  V2Sched s = {};
  s.nf = v2_plan_start(p, p.nblk); s.nb = v2p_b_start(p, p.nblk); s.nm = v2p_op_start(p, p.nblk); s.mb = s.nm - tail;
  s.ok = s.nf <= 27 && s.nb <= 36 && s.nf >= nslot && tail > 0 && s.mb > 0;
  s.a_dist = s.b_dist = s.nm;
  for (int f = 0; f < s.nf && s.ok; ++f) {
    int free_at = -s.nm;
    for (int k = 1; k <= s.nf; ++k) {
      const int g = f - k, gg = g < 0 ? g + s.nf : g;
      if (gg % nslot == f % nslot) { free_at = v2p_a_last(p, gg) + 1 - (g < 0 ? s.nm : 0); break; }
    }
    const int first = v2p_a_first(p, f);
    int at = free_at > first - pfd ? free_at : first - pfd;
    if (at < 0 && at < s.mb - s.nm) at = s.mb - s.nm;
    s.a_at[f] = at;
    s.a_dist = first - at < s.a_dist ? first - at : s.a_dist;
    s.ok = s.ok && at >= free_at && at <= first && (at < 0 ? at + s.nm >= s.mb : at <= s.mb);
  }
  for (int g = 0; g < s.nb && s.ok; ++g) {
    const int sel = g - v2p_b_start(p, v2p_b_blk(p, g));
    int free_at = -s.nm;
    for (int k = 1; k <= s.nb; ++k) {
      const int h = g - k, hh = h < 0 ? h + s.nb : h;
      if (hh - v2p_b_start(p, v2p_b_blk(p, hh)) == sel) { free_at = v2p_b_last(p, hh) + 1 - (h < 0 ? s.nm : 0); break; }
    }
    const int first = v2p_b_first(p, g);
    int at = free_at;
    if (at < 0 && at < s.mb - s.nm) at = s.mb - s.nm;
    s.b_at[g] = at;
    s.b_dist = first - at < s.b_dist ? first - at : s.b_dist;
    s.ok = s.ok && at >= free_at && at <= first && (at < 0 ? at + s.nm >= s.mb : at <= s.mb);
  }
  return s;
}
// [wave][tile][half] -> position; waves w and w + 4 share a SIMD: one border wave beside one interior wave, i.e. 45 / 45 / 45 / 48
// steps per SIMD and chunk instead of 54.  Same box, three alternating passes, B = 256 (profiles/border_skip_ab.txt): den.conv4 /
// conv5 launches 359-373 / 344-351 -> 334 / 312-314 us, dense reverse process 85.4-86.2 -> 77.5-77.8 ms.  Border waves 0 2 4 6
// (two border waves on one SIMD, two interior waves on the next: the chunk again lasts 54 steps, only its LDS traffic falls):
// 351-359 / 319-321 us, 79.4-79.7 ms.
__device__ constexpr uint8_t V2_FULL_POS[8][V2_FT][2] = {
    {{0, 1}, {2, 3}, {4, 5}},       {{6, 13}, {20, 27}, {34, 41}},  {{7, 14}, {21, 28}, {35, 42}},  {{43, 44}, {45, 46}, {47, 40}},
    {{8, 9}, {10, 11}, {12, 15}},   {{16, 17}, {18, 19}, {22, 23}}, {{24, 25}, {26, 29}, {30, 31}}, {{32, 33}, {36, 37}, {38, 39}}};
__device__ constexpr uint8_t V2_WAVE_CLS[8] = {V2_TOP, V2_RIGHT, V2_LEFT, V2_BOTTOM, V2_INT, V2_INT, V2_INT, V2_INT};
// the table is a permutation of 0 .. 47, no (tile, tap) step is issued twice, and every step a wave omits lies outside the image for
// BOTH positions of its tile
constexpr bool v2_full_map_ok() {
  bool seen[48] = {};
  for (int w = 0; w < 8; ++w)
    for (int i = 0; i < V2_FT; ++i)
      for (int h = 0; h < 2; ++h) {
        const int p = V2_FULL_POS[w][i][h];
        if (p >= 48 || seen[p]) return false;
        seen[p] = true;
      }
  int steps = 0;                                         // (tile, tap) steps issued: the 183 the border skip leaves, none of them beside the image
  for (int w = 0; w < 8; ++w) {
    const V2Plan& pl = V2_PLAN[V2_WAVE_CLS[w]];
    for (int b = 0; b < pl.nblk; ++b)
      if (pl.tap[b] + pl.pair[b] > 8 || pl.nt[b] < 1 || pl.nt[b] > V2_FT) return false;   // a pair is (a, a + 1)
    for (int i = 0; i < V2_FT; ++i)
      for (int tap = 0; tap < 9; ++tap) {
        int n = 0;
        for (int b = 0; b < pl.nblk; ++b) n += v2_plan_has(pl, b, tap) && i >= V2_FT - pl.nt[b];
        if (n > 1) return false;
        steps += n;
        for (int h = 0; h < 2 && n == 0; ++h) {
          const int y = V2_FULL_POS[w][i][h] / 7 + tap / 3 - 1, x = V2_FULL_POS[w][i][h] % 7 + tap % 3 - 1;
          if (y >= 0 && y < 7 && x >= 0 && x < 7) return false;
        }
      }
  }
  return steps == 11 * 6 + 13 * 9;
}
static_assert(v2_full_map_ok(), "full 7x7 items: position table and block lists");

// COPY ROLES.  A chunk's LDS-DMA pieces (14 image-row pieces "A", then the 27 weight pieces "W") are divided among the first nca / ncww
// waves of a workgroup: wave w owns A pieces w * npa + j (j < npa = ceil(14 / nca)) and W pieces w + ncww * q.  Every form but the full
// 7x7 one uses all its waves.  On full 7x7 items the interior waves (27 steps per chunk) set the length of the chunk and the border wave
// of their SIMD reaches the chunk barrier 9 steps (bottom: 6) before them: the three 18-step waves -- top, right, left -- issue ALL the
// copies, 14 / 14 / 13 pieces, one per step (= two MFMAs) from the chunk's first; the bottom wave and the interior waves issue none.  A border class
// is ONE wave, so its piece table is a compile-time constant (scalar instructions of a den.conv4 launch 20.3 M -> 15.0 M).  Same box,
// three alternating passes, B = 256 (profiles/copy_roles_ab.txt): dense reverse process 78.55-78.63 -> 77.11-77.35 ms, den.conv4 / conv5
// main + tail 322-327 / 311-313 -> 317-321 / 306-307 us.  The same file has what paid less or not at all: the four border waves copying
// (11 / 11 / 11 / 8 pieces) -0.8 ms where three waves give -1.2; two pieces per step, or the first piece at step 2, 0.1-0.4 ms slower
// than one per step from step 0; and the input-record COUNTING moved to the border waves as well (four records per thread of 256):
// +0.4 ms on its own, and the copies' gain gone when both move -- the counting keeps its symmetric form, thread tid of 512 counts
// records tid and tid + 512.
constexpr int V2_FULL_NCA = 3, V2_FULL_NCWW = 3;         // full 7x7 items: waves that copy A pieces / W pieces
constexpr int v2_ceil_div(int a, int b) { return (a + b - 1) / b; }
constexpr int v2_copy_na(int na, int ncw, int w) {       // A pieces wave w really has (the table repeats the last one beyond them)
  const int npa = v2_ceil_div(na, ncw), left = na - w * npa;
  return w >= ncw || left <= 0 ? 0 : (left < npa ? left : npa);
}
constexpr int v2_copy_nw(int nw, int ncw, int w) {       // W pieces wave w really has
  return w >= ncw || w >= nw ? 0 : (nw - w + ncw - 1) / ncw;
}
// LDS byte offset of record r = (cell, step) inside a slab of width w; a thread without a record reads cell 0, a border cell (always
// zero): an unconditional read (a conditional one is a branch with an LDS wait of its own, twice per chunk)
constexpr int v2_rec_off(int r, int nrec, int w) {
  const int cl = r >> 4, t = r & 15;
  return r < nrec ? (((cl / w) + 1) * (w + 1) + 1 + (cl % w)) * POSB + t * 16 : 0;
}
// every piece of a chunk is issued by exactly one wave; every record of an item is counted by exactly one thread, inside the image;
// a thread's slot without a record reads the zero cell
constexpr bool v2_roles_ok(int nwv, int nca, int ncww, int na, int nw, int nrec, int w) {
  int pa[64] = {}, pw[64] = {};
  if (na > 64 || nw > 64 || nca > nwv || ncww > nwv) return false;
  for (int wv = 0; wv < nwv; ++wv) {
    for (int j = 0; j < v2_copy_na(na, nca, wv); ++j) ++pa[wv * v2_ceil_div(na, nca) + j];
    for (int q = 0; q < v2_copy_nw(nw, ncww, wv); ++q) ++pw[wv + ncww * q];
  }
  for (int i = 0; i < na; ++i) if (pa[i] != 1) return false;
  for (int i = 0; i < nw; ++i) if (pw[i] != 1) return false;
  const int nct = 64 * nwv, nr = v2_ceil_div(nrec, nct);
  int seen[1024] = {};
  if (nrec > 1024) return false;
  for (int tid = 0; tid < nct; ++tid)
    for (int k = 0; k < nr; ++k) {
      const int r = tid + k * nct, off = v2_rec_off(r, nrec, w);
      if (r < nrec) {
        const int cell = off / POSB, y = cell / (w + 1), x = cell % (w + 1);
        if (y < 1 || x < 1 || x > w || (y - 1) * w + (x - 1) != (r >> 4) || (off % POSB) != (r & 15) * 16) return false;
        ++seen[r];
      } else if (off != 0) return false;
    }
  for (int r = 0; r < nrec; ++r) if (seen[r] != 1) return false;
  return true;
}
static_assert(v2_roles_ok(8, V2_FULL_NCA, V2_FULL_NCWW, 7 * 2, W_PIECES, 7 * 7 * 16, 7), "full 7x7 items: 41 pieces, 784 records, one owner each");

// CLS (full 7x7 items): the wave class this instance serves; the kernel branches once per wave, so that a class's K loop, scan and
// register allocation are its own (one body whose chunk loops alone were per class spilled 109 registers at the joins).
template <int H, int W, int NWV, bool SPLIT, int NTP, bool HALF = false, int CLS = V2_INT>
__device__ __forceinline__ void fp6v2_body(const V2Args& a, const int g, const int il, const int lanes, const int n_images,
                                           const int* __restrict__ slots, const int n_live = 0) {
  constexpr bool PRUNE = NTP > 0;
  constexpr bool LIVE = PRUNE && !HALF;                // listed slots: one at or past the image count n_live is computed and dropped
  static_assert(!HALF || (PRUNE && !SPLIT && H == 7 && W == 7 && NWV == 4 && NTP == 3), "half-image items: 7x7, four waves x three tiles");
  // how the four-digit form counts the active inputs of a row: REC: once per input record and chunk for the whole workgroup
  // (full items: the per-fragment popcounts were 29 % of the launch's vector issue), else per A fragment in the K loop
  // (listed positions: an item has few fragments, and the per-item passes of REC cost more than they save there: -2.5 %)
  constexpr bool REC = !PRUNE;
  // AH (round 5): the chunk barrier sits four steps BEFORE the end of the chunk instead of at its start.  Every read of the
  // current buffers has been issued by then (the last spike fragment at step NSTEP - 5, the last weight tile at the first step of
  // the last block but one), so that barrier both publishes the next chunk's copies and releases the current buffers -- and the
  // four steps behind it read the next chunk's first fragments: no LDS round trip in front of a chunk's first MFMA any more.  The
  // first chunk of an item still starts with its reads (the fragment registers must not live through the epilogue).
  // (Three slab buffers, the copies issued two chunks ahead, measured 1 % slower: conv4 376 against 373 us,
  //  profiles/r5_ab_kernel_variants.txt (4), (5).)
  constexpr int HW = H * W, PW = W + 1;
  constexpr int Hb = SPLIT ? H / 2 : H;                // output rows of an item
  constexpr int Hin = SPLIT ? Hb + 1 : H;              // input rows staged per item
  constexpr int HWb = Hb * W;                          // output positions of an item
  static_assert(SPLIT ? ((H % 2) == 0 && (HWb % (2 * NWV)) == 0)
                      : ((HW & 1) == 1 && ((HW / 2) % NWV) == 0), "whole 32-row tiles on every wave (+ one odd position)");
  static_assert(!PRUNE || (!SPLIT && (NWV == 4 || NWV == 8) && NTP <= (HWb / 2) / NWV), "position lists: 7x7 items");
  constexpr int NT = PRUNE ? NTP : (HWb / 2) / NWV;    // row tiles per wave (7x7: 6 or 3; 8x8 bands: 4)
  constexpr int N_AGPR = NWV == 4 ? (NACC * NT < 16 ? NACC * NT : 16) : 0;   // (two waves per SIMD: with any accumulator in AGPRs hipcc splits 256 registers 128 / 128)
  constexpr int NPP = (Hin + 2) * PW + 1;              // cells of the zero-bordered LDS image (pitch W + 1: the zero
  constexpr int A_BYTES = NPP * POSB;                  //  column is shared by x = -1 of a row and x = W of the previous)
  constexpr int PPR = (W + 3) / 4;                     // DMA pieces per image row (4 positions per KiB piece)
  constexpr int NA = Hin * PPR;
  constexpr bool BSKIP = NWV == 8 && !PRUNE && !SPLIT;  // full 7x7 items: per-wave block lists without the pure-border taps (V2_PLAN)
  static_assert(!BSKIP || (H == 7 && W == 7 && NT == V2_FT), "border skip: the position table is for 7x7 items of three tiles per wave");
  static_assert(BSKIP || CLS == V2_INT, "wave classes: full 7x7 items only");
  // copy roles (v2_roles_ok): full 7x7 items give the copies to border waves, whose class fixes the wave
  constexpr int NCA = BSKIP ? V2_FULL_NCA : NWV, NCWW = BSKIP ? V2_FULL_NCWW : NWV;
  constexpr bool KNOWN = BSKIP && CLS != V2_INT;       // a border class is ONE wave: its piece table is a constant
  constexpr int CWV = KNOWN ? CLS - 1 : 0;
  static_assert(!KNOWN || V2_WAVE_CLS[CWV] == CLS, "border class k is wave k - 1");
  static_assert(!BSKIP || v2_roles_ok(NWV, NCA, NCWW, NA, W_PIECES, Hin * W * 16, W), "copy roles, record counting");
  constexpr int NPA_T = (NA + NCA - 1) / NCA;          // A pieces per copying wave (the table's stride) ...
  constexpr int NPA = KNOWN ? v2_copy_na(NA, NCA, CWV) : ((!BSKIP || NCA == NWV) ? NPA_T : 0);   // ... and what this body issues
  constexpr int NPW = KNOWN ? v2_copy_nw(W_PIECES, NCWW, CWV) : ((!BSKIP || NCWW == NWV) ? (W_PIECES + NCWW - 1) / NCWW : 0);
  static_assert(NWV >= 8 || NACC * NT <= 16 || (NT - 1) * NACC <= N_AGPR + 2, "only the last tile may straddle the register files");
  constexpr bool AH = NWV == 8 && !PRUNE;                // (two waves per SIMD on full items)
  constexpr int NBUF = 2;                              // slab buffers: the copies of chunk c + 1 are issued during chunk c
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint8_t* const sA = lds;
  uint8_t* const sW = lds + NBUF * A_BYTES;
  // active inputs per input cell and step (s_cin, borders stay zero) and per output position and step (s_row)
  int* const s_cin = reinterpret_cast<int*>(lds + NBUF * A_BYTES + NBUF * W_LDS);    // [NPP][16]
  int* const s_row = s_cin + NPP * 16;                                               // [HWb + 1][16]
  int* const s_nmax = s_row + (HWb + 1) * 16;                                        // [HWb + 1]: max over the steps of s_row[p][.]
  const unsigned sA_addr = spk_lds_addr(sA), sW_addr = sA_addr + NBUF * A_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nch = a.nch;
  const int G = a.Cout >> 5;
  const int wave_s = KNOWN ? CWV : __builtin_amdgcn_readfirstlane(wave);
  const unsigned lane16 = (unsigned)lane * 16u;
  const unsigned wave_k = (unsigned)wave_s * 1024u;
  const uint8_t* const wbase = a.wq + (long long)g * nch * W_SLAB;
  const int nitems = (SPLIT || HALF) ? 2 * n_images : n_images;
  auto issue_w = [&](int qw, const uint8_t* wslab, unsigned dW) {   // W piece qw of this wave (a table slot beyond the slab repeats the last)
    unsigned ko = wave_k + 1024u * NCWW * (unsigned)qw;
    if (NCWW * qw + NCWW - 1 >= W_PIECES) ko = ko < (unsigned)W_PIECES * 1024u ? ko : ko - 1024u * NCWW;
    spk_dma16s(wslab + ko, lane16, dW + ko);
  };
  if constexpr (BSKIP && NPW > 0) {
    // the first chunk's weight pieces do not land in anything the zeroing below touches: issued in front of it and of its barrier
    if (il < nitems) {
#pragma unroll
      for (int q = 0; q < NPW; ++q) issue_w(q, wbase, sW_addr);
    }
  }
  // zero the A images once: the borders stay zero for the whole kernel, interiors are overwritten by DMA
  for (int i = tid; i < NBUF * A_BYTES / 16; i += NWV * 64) reinterpret_cast<uint4*>(sA)[i] = make_uint4(0, 0, 0, 0);
  if (REC)
    for (int i = tid; i < NPP * 16; i += NWV * 64) s_cin[i] = 0;
  __syncthreads();         // no wave's first DMA piece may land in a cell another wave has yet to zero

  // per-lane LDS byte offsets of this wave's A fragments (tile ti = wave + NWV * i; full 7x7 items: the positions of V2_FULL_POS),
  // relative to tap (0, 0): the same cell for both K halves (digit-pair instructions); a tap-pair block adds the second tap's distance,
  // one cell or PW - 2 cells, in the upper lane half (a_hd1, a_hd2)
  const int row = lane & 31, half = lane >> 5;
  const int a_hd1 = half * POSB, a_hd2 = half * (PW - 2) * POSB;
  // tap-pair B operands: lanes 0-31 read their half of tile (a, pair), lanes 32-63 theirs of tile (a + 1, pair), 2 WT further on
  const int b_o16 = lane * 16 + half * (2 * WT - 512), b_o8 = 1024 + lane * 8 + half * (2 * WT - 256);
  const int hsel = (row >> 2) & 1, tt = (row & 3) + 4 * (row >> 3);
  int a_off[NT];
  int p_out[NT];                                          // output position of this lane's accumulator rows
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int p = BSKIP ? (int)V2_FULL_POS[wave & 7][i % V2_FT][hsel] : 2 * (wave + NWV * i) + hsel;
    a_off[i] = ((p / W) * PW + (p % W)) * POSB + tt * 16;
    p_out[i] = BSKIP ? (int)V2_FULL_POS[wave & 7][i % V2_FT][half] : 2 * (wave + NWV * i) + half;
  }

  // DMA piece table (wave-uniform): bits 0..13 source byte offset in the slab, 14..28 LDS byte offset in the image,
  // 29..30 positions in the piece - 1.  Pieces beyond the slab repeat the last one so that the K loop issues unconditionally.
  unsigned pa_pk[NPA > 0 ? NPA : 1];
#pragma unroll
  for (int j = 0; j < NPA; ++j) {
    int id = wave_s * NPA_T + j;
    id = id < NA ? id : NA - 1;
    const int y = id / PPR, px = id - y * PPR;
    const int np = (W - 4 * px) < 4 ? (W - 4 * px) : 4;
    const unsigned src = (unsigned)((y * W + 4 * px) * POSB), dst = (unsigned)(((y + 1) * PW + 1 + 4 * px) * POSB);
    pa_pk[j] = src | (dst << 14) | ((unsigned)(np - 1) << 29);
  }
  auto issue_piece = [&](int q, const uint8_t* aslab, const uint8_t* wslab, unsigned dA, unsigned dW) {
    if (q < NPA) {
      const unsigned pk = pa_pk[q];
      const unsigned np = ((pk >> 29) & 3u) + 1u;
      const unsigned long long mask = np == 4 ? ~0ull : ((1ull << (16 * np)) - 1ull);
      spk_dma16s_masked(aslab + (pk & 0x3fffu), lane16, dA + ((pk >> 14) & 0x7fffu), mask);
    } else issue_w(q - NPA, wslab, dW);
  };
  // item index -> (image, band); the slab of a band starts (H/2 - 1) rows into the image for the bottom band
  auto aslab_of = [&](int itm, int c) -> const uint8_t* {
    const int b = HALF ? itm >> 1 : (PRUNE ? slots[itm] : (SPLIT ? itm >> 1 : itm)), band = SPLIT ? itm & 1 : 0;
    return a.in0 + ((long long)b * nch + c) * HW * POSB + band * (Hb - 1) * W * POSB;
  };

  // per-channel constants (the group is fixed: loaded once)
  const int co = g * 32 + (lane & 31);
  const float scale_f = (float)a.scale[co], bias_f = (float)a.bias[co];
  const float bna = a.bn_a[co], bnb = a.bn_b[co];
  const float Bc = fmaf(bias_f, bna, bnb);
  // certification constants: cE holds the rounding terms and cT the dropped digits PER ACTIVE INPUT (|32 d4 + d5| <= 528 units
  // of 2^-s each, rounded up), multiplied in the epilogue by the number of active inputs of the row -- 5-7x tighter than "every
  // input active" at the firing rates of the denoiser, which is what lets the fifth digit leave the matrix cores
  const float cE = 2.0f * 2.38418579e-07f * (fabsf(bnb) + fabsf(Bc)) + 1e-30f;
  const float cT = 528.0f * scale_f * fabsf(bna) * 1.000001f;
  const float Ac4 = 1024.0f * scale_f * bna;               // z = fma(Q4, Ac4, Bc),  Q4 = P01 * 2^10 + P23

  const int sc_a = 0x7f7f7f7f;                            // e8m0 block scales: spikes x 1
  const int sc_p = half ? (int)0x82828282u : (int)0x87878787u;   // digit pairs: even digit (K half 0) x 2^8, odd digit x 2^3
  const int sc_hi = (int)0x87878787u, sc_lo = (int)0x82828282u;  // tap pairs: one digit in both K halves

  int it = 0;                                             // running chunk counter: LDS buffer = it & 1
  if (il < nitems) {
    const uint8_t* as0 = aslab_of(il, 0);
#pragma unroll
    for (int q = 0; q < (BSKIP ? NPA : NPA + NPW); ++q) issue_piece(q, as0, wbase, sA_addr, sW_addr);
    if constexpr (AH) {                                   // (the only chunks whose copies no chunk barrier has waited for)
      spk_dma_wait_all();
      __syncthreads();
    }
  }
  for (int itm = il; itm < nitems; itm += lanes) {
    const int b = HALF ? itm >> 1 : (PRUNE ? slots[itm] : (SPLIT ? itm >> 1 : itm)), band = SPLIT ? itm & 1 : 0;
    const int band_off = band * PW * POSB;                // bottom band: fragment addresses one LDS row further down
    int n_list = 2 * NT * NWV;
    if constexpr (PRUNE) {
      const uint8_t* rec = HALF ? &V2_HALF_REC[itm & 1][0] : a.need + (long long)b * 64;
      n_list = __builtin_amdgcn_readfirstlane((int)rec[48]);
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int k2 = 2 * (wave + NWV * i);
        const int p = rec[k2 + hsel];
        a_off[i] = ((p / W) * PW + (p % W)) * POSB + tt * 16;
        p_out[i] = rec[k2 + half];
      }
    }
    v16f acc[NT][NACC];   // [i][0]: pair 01, [i][1]: pair 23; written (not accumulated) by the first MFMA
    int cnt[NT];          // !REC: active inputs of this lane's A row (position, step) over all taps and chunks
#pragma unroll
    for (int i = 0; i < NT; ++i) cnt[i] = 0;
    // REC: every thread counts the active inputs of NR input records (cell, step) of the item, chunk by chunk
    constexpr int NREC = Hin * W * 16, NR = (NREC + NWV * 64 - 1) / (NWV * 64);
    int creg[NR];
    int rec_off[NR];                                      // LDS byte offset of the record inside a slab; threads without one read
    bool rec_ok[NR];                                      //  the zero cell (v2_rec_off)
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      creg[k] = 0;
      const int r = tid + k * NWV * 64;
      rec_ok[k] = r < NREC;
      rec_off[k] = v2_rec_off(r, NREC, W);
    }
    constexpr int PFX = BSKIP ? v2_tp_slots(CLS) : (NWV == 4 ? SPK_V2_PF : 4);
    v6i bp[2][2];                                         // digit-pair tiles of block parity [blk & 1][pair]  (AH: carried over the
    v4i af[PFX];                                          //  chunks of an item: a chunk's last steps fill them for the next one)
                                                          // (tap pairs: B operand sel in bp[sel >> 1][sel & 1], A fragment f in af[f % PFX])
    for (int c = 0; c < nch; ++c, ++it) {
      const int buf = it & 1, buf1 = buf ^ 1;             // this chunk's buffers, the next chunk's (where this chunk's copies go)
      if constexpr (!AH) {
        spk_dma_wait_all();  // this wave's share of the chunk's DMA has landed ...
        __syncthreads();     // ... and so has everyone else's; everyone is done with the other buffer
      }
      int nb = itm, nc = c + 1;
      if (nc == nch) { nc = 0; nb = itm + lanes; }
      const bool have_next = nb < nitems;                 // otherwise the last chunk is copied once more (never read)
      const uint8_t* n_aslab = aslab_of(have_next ? nb : itm, have_next ? nc : c);
      const uint8_t* n_wslab = wbase + (long long)(have_next ? nc : c) * W_SLAB;
      const unsigned n_dA = sA_addr + buf1 * A_BYTES;
      const unsigned n_dW = sW_addr + buf1 * W_LDS;

      // REC: the chunk's record counts.  The two LDS reads are issued after the chunk's first MFMA step and their popcounts a few
      // steps later, inside the MFMA stream (in front of it they held the chunk's first MFMA back by an LDS round trip at every
      // chunk barrier).
      v4i rvq[NR];
      // Full 7x7 items: the K loop of the class's tap-pair plan ("TAP PAIRS" above), one op = one MFMA.  Every read is issued in front
      // of the op its schedule names (v2p_sched), the reads of the NEXT chunk's first operands behind the chunk barrier at op MB.
      auto compute_tap_pairs = [&](auto first_tag, const uint8_t* A, const uint8_t* Wb) {
        constexpr bool FIRST = decltype(first_tag)::value;
        constexpr V2Plan P = V2_PLAN[BSKIP ? CLS : V2_INT];
        constexpr V2Sched S = v2p_sched(P, PFX, SPK_V2_TP_PFD, SPK_V2_TP_TAIL);
        constexpr int NM = S.nm, MB = S.mb, NF = S.nf, NB = S.nb, NPIECES = NPA + NPW;
        static_assert(S.ok, "tap pairs: every read in front of its first use, behind its register set's last use, on the right side of the chunk barrier");
        // (the bottom wave's one-tile blocks take a new B operand with every MFMA: four sets leave one MFMA between read and use there,
        //  as the digit-pair loop did -- that wave is 12 MFMAs per chunk shorter than the interior wave of its SIMD)
        static_assert(S.a_dist >= 2 && S.b_dist >= (CLS == V2_BOTTOM ? 1 : 3), "no read right in front of the MFMA that needs it");
        static_assert(P.pair[0] && P.nt[0] == NT, "the first block writes (not accumulates) every accumulator: digits 0 and 2 of a pair block");
        // one copy slot per MFMA pair from the chunk's first (a wave's 14 pieces are out by op 26), the record counts at ops 2 and
        // 2 x SPK_V2_REC_STEP: all in front of the chunk barrier
        static_assert((NPIECES == 0 || 2 * (NPIECES - 1) < MB) && 2 * SPK_V2_REC_STEP < MB, "copy slots and record-count ops in front of the chunk barrier");
        auto toff = [](int tap) constexpr -> int { return ((tap / 3) * PW + (tap % 3)) * POSB; };
        auto lda = [&](const uint8_t* base, auto f_tag) -> v4i {
          constexpr int f = decltype(f_tag)::value, blk = v2_plan_blk(P, f), i = NT - P.nt[blk] + (f - v2_plan_start(P, blk));
          constexpr int t0 = toff(P.tap[blk]), dl = P.pair[blk] ? toff(P.tap[blk] + 1) - t0 : 0;
          static_assert(dl == 0 || dl == POSB || dl == (PW - 2) * POSB, "a pair's second tap: the next cell, or the first of the next row");
          const int o = dl == 0 ? a_off[i] : a_off[i] + (dl == POSB ? a_hd1 : a_hd2);
          return *reinterpret_cast<const v4i*>(base + o + t0);
        };
        auto ldb = [&](const uint8_t* base, auto g_tag) -> v6i {
          // 16 + 8 bytes per lane; the 8-byte read is volatile so that hipcc does not pair the tails of two operands
          constexpr int g = decltype(g_tag)::value, blk = v2p_b_blk(P, g), sel = g - v2p_b_start(P, blk);
          constexpr int tile = 2 * P.tap[blk] + (P.pair[blk] ? sel >> 1 : sel), odd = P.pair[blk] ? sel & 1 : 0;
          const uint8_t* p = base + tile * WT;
          const int o16 = P.pair[blk] ? b_o16 + 512 * odd : lane * 16, o8 = P.pair[blk] ? b_o8 + 256 * odd : 1024 + lane * 8;
          const v4i x = *reinterpret_cast<const v4i*>(p + o16);
          typedef const volatile __attribute__((address_space(3))) v2i* lds_v2i_ptr;
          const v2i y = *(lds_v2i_ptr)SPK_LDS(p + o8);
          const v6i r = {x[0], x[1], x[2], x[3], y[0], y[1]};
          return r;
        };
        if constexpr (FIRST) {
          static_for<NB>([&](auto g_tag) {
            constexpr int g = decltype(g_tag)::value, sel = g - v2p_b_start(P, v2p_b_blk(P, g));
            if constexpr (S.b_at[g] < 0) bp[sel >> 1][sel & 1] = ldb(Wb, g_tag);
          });
          static_for<NF>([&](auto f_tag) {
            constexpr int f = decltype(f_tag)::value;
            if constexpr (S.a_at[f] < 0) af[f % PFX] = lda(A, f_tag);
          });
        }
        const uint8_t* An = sA + buf1 * A_BYTES + band_off;
        const uint8_t* Wn = sW + buf1 * W_LDS;
        const bool ahead = c + 1 < nch;                     // (the last chunk of an item reads nothing ahead)
        static_for<NM>([&](auto m_tag) {
          constexpr int m = decltype(m_tag)::value, blk = v2p_op_blk(P, m), q = m - v2p_op_start(P, blk);
          constexpr int sel = v2p_op_sel(P, blk, q), i = v2p_op_tile(P, blk, q);
          constexpr int f = v2_plan_start(P, blk) + i - (NT - P.nt[blk]);
          // this chunk's reads ...
          static_for<NB>([&](auto g_tag) {
            constexpr int g = decltype(g_tag)::value, gs = g - v2p_b_start(P, v2p_b_blk(P, g));
            if constexpr (S.b_at[g] == m) bp[gs >> 1][gs & 1] = ldb(Wb, g_tag);
          });
          static_for<NF>([&](auto f_tag) {
            if constexpr (S.a_at[decltype(f_tag)::value] == m) af[decltype(f_tag)::value % PFX] = lda(A, f_tag);
          });
          if constexpr (m == MB) {
            // every read of this chunk's buffers is issued; this wave's copies of the next chunk have landed: the chunk barrier
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
          }
          // ... and, behind the barrier, the next chunk's first ones
          if constexpr (m >= MB) {
            if (ahead) {
              static_for<NB>([&](auto g_tag) {
                constexpr int g = decltype(g_tag)::value, gs = g - v2p_b_start(P, v2p_b_blk(P, g));
                if constexpr (S.b_at[g] + NM == m) bp[gs >> 1][gs & 1] = ldb(Wn, g_tag);
              });
              static_for<NF>([&](auto f_tag) {
                if constexpr (S.a_at[decltype(f_tag)::value] + NM == m) af[decltype(f_tag)::value % PFX] = lda(An, f_tag);
              });
            }
          }
          if constexpr (!P.pair[blk]) {
            SPK_MFMA_FP6("v", acc[i][sel], af[f % PFX], bp[0][sel], sc_a, sc_p);
          } else if constexpr (FIRST && blk == 0 && (sel & 1) == 0) {
            SPK_MFMA_FP6_Z("v", acc[i][sel >> 1], af[f % PFX], bp[sel >> 1][0], sc_a, sc_hi);
          } else if constexpr ((sel & 1) == 0) {
            SPK_MFMA_FP6("v", acc[i][sel >> 1], af[f % PFX], bp[sel >> 1][0], sc_a, sc_hi);
          } else {
            SPK_MFMA_FP6("v", acc[i][sel >> 1], af[f % PFX], bp[sel >> 1][1], sc_a, sc_lo);
          }
          __builtin_amdgcn_sched_barrier(0);
          if constexpr ((m & 1) == 0 && m / 2 < NPIECES) issue_piece(m / 2, n_aslab, n_wslab, n_dA, n_dW);
          if constexpr (m == 2) {
#pragma unroll
            for (int k = 0; k < NR; ++k) rvq[k] = *reinterpret_cast<const v4i*>(sA + buf * A_BYTES + rec_off[k]);
          }
          if constexpr (m == 2 * SPK_V2_REC_STEP) {
#pragma unroll
            for (int k = 0; k < NR; ++k)
              creg[k] += __builtin_popcount((unsigned)rvq[k][0]) + __builtin_popcount((unsigned)rvq[k][1]) +
                         __builtin_popcount((unsigned)rvq[k][2]) + __builtin_popcount((unsigned)rvq[k][3]);
          }
        });
      };
      auto compute = [&](auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const uint8_t* A = sA + buf * A_BYTES + band_off;
        const uint8_t* Wb = sW + buf * W_LDS;
        auto toff = [](int tap) constexpr -> int { return ((tap / 3) * PW + (tap % 3)) * POSB; };
        if constexpr (BSKIP) {
          compute_tap_pairs(first_tag, A, Wb);
          return;
        }
        // Step order: nine blocks, one tap per block, one step per row tile of the block; a step issues the two digit-pair MFMAs
        constexpr V2Plan P = v2_uniform_plan(NT);
        constexpr int NBLK = P.nblk, NSTEP = v2_plan_start(P, NBLK);
        constexpr int PF = PFX;
        constexpr int NPIECES = NPA + NPW;
        // what the schedule below relies on:
        static_assert(P.nt[0] == NT, "the first block writes (not accumulates) every accumulator");
        // copy slots: two per block (its first step and its middle step)
        static_assert(2 * NBLK >= NPIECES, "two copy slots per block: every DMA piece of the wave gets one");
        static_assert((!AH || NSTEP >= 2 * PF) && (!REC || NSTEP > SPK_V2_REC_STEP), "look-ahead slots; the record-count steps exist");
        // AH, the chunk barrier at step NSTEP - PF: the copies are issued in front of it (it waits for them), and so is every read of
        // the current buffers -- the last fragment at step NSTEP - PF - 1 by construction, the last weight tiles at the first step of
        // the last block but one (8x8 bands, two tiles per wave: in the step that opens with the barrier; the first copy into these
        // buffers is PF steps behind it)
        static_assert(!AH || (v2_plan_start(P, (NPIECES + 1) / 2) <= NSTEP - PF && v2_plan_start(P, NBLK - 2) <= NSTEP - PF),
                      "chunk barrier behind the copies and the last weight-tile read");
        auto lda_at = [&](const uint8_t* base, auto s_tag) -> v4i {
          constexpr int s = decltype(s_tag)::value;
          constexpr int blk = v2_plan_blk(P, s), i = NT - P.nt[blk] + (s - v2_plan_start(P, blk));
          return *reinterpret_cast<const v4i*>(base + a_off[i] + toff(P.tap[blk]));
        };
        auto lda = [&](auto s_tag) -> v4i { return lda_at(A, s_tag); };
        auto ldb = [&](int tile) -> v6i {
          // 16 + 8 bytes per lane; the 8-byte read is volatile so that hipcc does not pair the tails of two tiles
          const uint8_t* p = Wb + tile * WT;
          const v4i x = *reinterpret_cast<const v4i*>(p + lane * 16);
          typedef const volatile __attribute__((address_space(3))) v2i* lds_v2i_ptr;
          const v2i y = *(lds_v2i_ptr)SPK_LDS(p + 1024 + lane * 8);
          const v6i r = {x[0], x[1], x[2], x[3], y[0], y[1]};
          return r;
        };
        if constexpr (!AH || FIRST) {
          bp[0][0] = ldb(2 * P.tap[0]); bp[0][1] = ldb(2 * P.tap[0] + 1);
          static_for<PF>([&](auto s_tag) { af[decltype(s_tag)::value] = lda(s_tag); });
        }
        // AH: the next chunk's buffers (this item's; the last chunk of an item reads nothing ahead)
        const uint8_t* An = sA + buf1 * A_BYTES + band_off;
        const uint8_t* Wn = sW + buf1 * W_LDS;
        const bool ahead = AH && c + 1 < nch;
        static_for<NSTEP>([&](auto s_tag) {
          constexpr int s = decltype(s_tag)::value;
          constexpr int blk = v2_plan_blk(P, s), nt = P.nt[blk], j = s - v2_plan_start(P, blk);   // step j of a block of nt tiles
          constexpr int i = NT - nt + j;
          if constexpr (AH && s == NSTEP - PF) {
            // every read of this chunk's buffers is issued; this wave's copies of the next chunk have landed: the chunk barrier
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
          }
          const v4i av = af[s % PF];
          if constexpr (s + PF < NSTEP) af[s % PF] = lda(std::integral_constant<int, s + PF>{});
          else if constexpr (AH) {
            // the slot just consumed takes the next chunk's step with the same slot number: steps NSTEP - 4 .. NSTEP - 1 free slots
            // (NSTEP - 4) % 4 ..., i.e. the next chunk's steps s' with s' % 4 == s % 4
            constexpr int k = s % PF;                         // (PF == 4: next step k lives in slot k)
            if (ahead) af[k] = lda_at(An, std::integral_constant<int, k>{});
          }
          // (two per block: 18 slots for the 11 pieces of a wave of four)
#define V2_DMA_SLOT()                                                                              \
  do {                                                                                             \
    if constexpr (j == 0 && 2 * blk < NPIECES) issue_piece(2 * blk, n_aslab, n_wslab, n_dA, n_dW);                \
    if constexpr (j == (nt > 1 ? nt / 2 : 0) && 2 * blk + 1 < NPIECES)                             \
      issue_piece(2 * blk + 1, n_aslab, n_wslab, n_dA, n_dW);                                      \
  } while (0)
          // the next block's weight tiles are requested at the first step of this block
#define V2_NEXT_TILES()                                                                            \
  do {                                                                                             \
    if constexpr (j == 0 && blk + 1 < NBLK) {                                                      \
      bp[(blk + 1) & 1][0] = ldb(2 * P.tap[(blk + 1) % 9]);                                        \
      bp[(blk + 1) & 1][1] = ldb(2 * P.tap[(blk + 1) % 9] + 1);                                    \
    }                                                                                              \
  } while (0)
          if constexpr (!REC) {
            // (volatile: left to itself hipcc defers the pure popcounts and keeps every fragment of the chunk alive)
            asm volatile("v_bcnt_u32_b32 %0, %1, %0\n\tv_bcnt_u32_b32 %0, %2, %0\n\tv_bcnt_u32_b32 %0, %3, %0\n\t"
                         "v_bcnt_u32_b32 %0, %4, %0" : "+v"(cnt[i]) : "v"(av[0]), "v"(av[1]), "v"(av[2]), "v"(av[3]));
          }
#define V2_PAIR_MFMA(J)                                                                                      \
do {                                                                                                        \
  if constexpr (FIRST && blk == 0) {                                                                        \
    if constexpr (NACC * i + (J) < N_AGPR) SPK_MFMA_FP6_Z("a", acc[i][J], av, bp[0][J], sc_a, sc_p);              \
    else SPK_MFMA_FP6_Z("v", acc[i][J], av, bp[0][J], sc_a, sc_p);                                             \
  } else {                                                                                                  \
    if constexpr (NACC * i + (J) < N_AGPR) SPK_MFMA_FP6("a", acc[i][J], av, bp[blk & 1][J], sc_a, sc_p);          \
    else SPK_MFMA_FP6("v", acc[i][J], av, bp[blk & 1][J], sc_a, sc_p);                                         \
  }                                                                                                         \
} while (0)
          V2_PAIR_MFMA(0);
          __builtin_amdgcn_sched_barrier(0);
          V2_DMA_SLOT();
          V2_NEXT_TILES();
          if constexpr (REC) {
            if constexpr (s == 1) {
#pragma unroll
              for (int k = 0; k < NR; ++k) rvq[k] = *reinterpret_cast<const v4i*>(sA + buf * A_BYTES + rec_off[k]);
            }
            if constexpr (s == SPK_V2_REC_STEP) {
#pragma unroll
              for (int k = 0; k < NR; ++k)
                creg[k] += __builtin_popcount((unsigned)rvq[k][0]) + __builtin_popcount((unsigned)rvq[k][1]) +
                           __builtin_popcount((unsigned)rvq[k][2]) + __builtin_popcount((unsigned)rvq[k][3]);
            }
          }
          V2_PAIR_MFMA(1);
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (AH && s == NSTEP - 1) {
            if (ahead) {
              auto ldb_n = [&](int tile) -> v6i {
                const uint8_t* p = Wn + tile * WT;
                const v4i x = *reinterpret_cast<const v4i*>(p + lane * 16);
                typedef const volatile __attribute__((address_space(3))) v2i* lds_v2i_ptr;
                const v2i y = *(lds_v2i_ptr)SPK_LDS(p + 1024 + lane * 8);
                const v6i r = {x[0], x[1], x[2], x[3], y[0], y[1]};
                return r;
              };
              bp[0][0] = ldb_n(2 * P.tap[0]); bp[0][1] = ldb_n(2 * P.tap[0] + 1);
            }
          }
        });
      };
      if (c == 0) compute(std::true_type{}); else compute(std::false_type{});
    }   // chunks

    if constexpr (REC) {
      // publish the record counts, then add the nine taps of every output position: s_row[p][t] = active inputs of row (p, t)
#pragma unroll
      for (int k = 0; k < NR; ++k)
        if (rec_ok[k]) s_cin[(rec_off[k] / POSB) * 16 + ((rec_off[k] % POSB) >> 4)] = creg[k];
      if (tid <= HWb) s_nmax[tid] = 0;
      __syncthreads();
      for (int e = tid; e < HWb * 16; e += NWV * 64) {
        const int pp = e >> 4, t = e & 15;
        const int* c0 = s_cin + (((pp / W) + band) * PW + (pp % W)) * 16 + t;
        int sum = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) sum += c0[(dy * PW + dx) * 16];
        s_row[e] = sum;
        // the certification's first stage only needs max_t n_t of a position: one LDS atomic here instead of four 16-byte reads
        // and twelve v_max per tile and lane in the scan (the second stage, a few percent of the tiles, reads the sixteen counts)
        atomicMax(&s_nmax[pp], sum);
      }
      __syncthreads();
    }
    // The MFMAs are opaque to hipcc's hazard recognizer: an accumulator may be read 18 wait states after the (16-pass)
    // MFMA that wrote it was issued.
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");

    // ---------------- epilogue: fp32 recombination, BN, LIF scan, certification -------------------------------------
    // The tile that holds the VGPR-resident accumulators goes first (frees their registers for the scan temporaries).
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int i = k == 0 ? NT - 1 : k - 1;
#pragma unroll
      for (int j = 0; j < NACC; ++j)
        if (NACC * i + j < N_AGPR) asm volatile("" : "+a"(acc[i][j]));
      float v = 0.f;
      unsigned mybits = 0;
      bool flg = false;
      int cntv[16];                                       // active inputs of this lane's rows (its position, step r)
      if constexpr (!REC) {
        // the count of accumulator row r sits in the A-layout lane (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rowA = spk_acc_row(r, 0);
          const int c0 = __builtin_amdgcn_readlane(cnt[i], rowA), c1 = __builtin_amdgcn_readlane(cnt[i], rowA + 4);
          cntv[r] = half ? c1 : c0;
        }
      }
      int nmax_rec = 0;
      if constexpr (REC) nmax_rec = s_nmax[BSKIP ? p_out[i] : 2 * (wave + NWV * i) + half];     // (position within the item)
      // z = Q4 * Ac4 + Bc, Q4 = P01 * 2^10 + P23 (two steps at a time on the packed fp32 pipe); the dropped
      // digits move z_t by at most c_t = cE + cT n_t (n_t active inputs of the row).  D_t = D_{t-1} / 2 + c_t + 4 eps (|z_t| +
      // |v_{t-1}|) and |v| <= max |z| give D_t <= 2 (cE + cT max_t n_t) + 16 eps max_t |z_t| for every t: track max |z|,
      // max n and min |h - 1| (three instructions per step instead of eight) and compare once, against dh = D / 2
      float zmax = 0.f, dmin = 3.0e38f;
      int nmax = nmax_rec;
#pragma unroll
      for (int r2 = 0; r2 < 16; r2 += 2) {
        const v2f p0 = {acc[i][0][r2], acc[i][0][r2 + 1]}, p1 = {acc[i][1][r2], acc[i][1][r2 + 1]};
        const v2f q4 = __builtin_elementwise_fma(p0, (v2f){1024.0f, 1024.0f}, p1);
        const v2f z2 = __builtin_elementwise_fma(q4, (v2f){Ac4, Ac4}, (v2f){Bc, Bc});
        if constexpr (!REC) nmax = max(nmax, max(cntv[r2], cntv[r2 + 1]));
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float z = z2[e];
          zmax = fmaxf(zmax, fabsf(z));
          const float h = fmaf(z - v, 0.5f, v);            // == v + (z - v) * 0.5f: the product is exact (v is not an output here)
          const float hm = h - 1.0f;
          dmin = fminf(dmin, fabsf(hm));
          const bool s = h >= 1.0f;
          v = s ? 0.0f : h;
          mybits = __builtin_amdgcn_alignbit(mybits, __float_as_uint(hm), 31);   // (mybits << 1) | sign(h - 1)
        }
      }
      mybits = ~(__builtin_bitreverse32(mybits) >> 16) & 0xffffu;   // bit r = NOT sign(h_r - 1)
      flg = dmin <= SPK_V2_SPARE * fmaf(zmax, 2.5f * CERT_4EPS, fmaf((float)nmax, cT, cE));   // (10 eps for 8: a little to spare)
      if (__builtin_amdgcn_ballot_w64(flg) != 0ull) {
        // SECOND STAGE (a wave with a flagged lane: a few percent of the tiles).  The closed form above compares the closest
        // approach of ANY step with the bound of the WORST step.  The recursion it was derived from is tighter twice over: the
        // bound of step t only carries the counts of the steps before it, halved once per step (dh_t <= dh_{t-1} / 2 + c_t / 2
        // + 2 eps (|z_t| + |v_{t-1}|), c_t = cE + cT n_t; 2.5 eps for 2 as above), and each step's |h_t - 1| is compared with
        // ITS bound.  Flagged only if both stages flag: about half the exact recomputations (the repair launch's time is
        // proportional to them).  Every lane re-scans (the branch is wave-uniform); accumulators and counts are still live.
        float v2 = 0.f, dh = 0.f;
        bool f2 = false;
        if constexpr (REC) {
          const v4i* rp = reinterpret_cast<const v4i*>(s_row + (BSKIP ? p_out[i] : 2 * (wave + NWV * i) + half) * 16);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const v4i c4 = rp[q];
            cntv[4 * q] = c4[0]; cntv[4 * q + 1] = c4[1]; cntv[4 * q + 2] = c4[2]; cntv[4 * q + 3] = c4[3];
          }
        }
#pragma unroll
        for (int r2 = 0; r2 < 16; r2 += 2) {
          const v2f p0 = {acc[i][0][r2], acc[i][0][r2 + 1]}, p1 = {acc[i][1][r2], acc[i][1][r2 + 1]};
          const v2f q4 = __builtin_elementwise_fma(p0, (v2f){1024.0f, 1024.0f}, p1);
          const v2f z2 = __builtin_elementwise_fma(q4, (v2f){Ac4, Ac4}, (v2f){Bc, Bc});
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const float z = z2[e];
            const float ct = fmaf((float)cntv[r2 + e], cT, cE);
            dh = fmaf(fabsf(z) + fabsf(v2), 0.625f * CERT_4EPS, fmaf(dh, 0.5f, 0.5f * ct));
            const float h = fmaf(z - v2, 0.5f, v2);
            f2 = f2 || (fabsf(h - 1.0f) <= SPK_V2_SPARE * dh);
            v2 = h >= 1.0f ? 0.0f : h;
          }
        }
        flg = flg && f2;
      }
      const int ti = wave + NWV * i;
      // accumulator lane half == position within the tile; a list that does not fill its last tiles repeats its last
      // position there: computed and dropped
      const int p = (PRUNE || BSKIP) ? p_out[i] : 2 * ti + half + band * HWb;
      const bool listed = (!PRUNE || 2 * ti + half < n_list) && (!LIVE || b < n_live);
      if (flg && listed) spk_cert_flag(a.ws, ((long long)b * a.Cout + co) * HW + p);
      const long long rec = (((long long)b * G + g) * HW + p) * POSB;
      store_tile_spikes(a.out, a.out_cnt, mybits, lane, rec, (((long long)b * G + g) * HW + p) * 32, listed);
      __builtin_amdgcn_sched_barrier(0);
    }
  }   // images
  spk_dma_wait_all();     // the copy issued during the very last chunk must not outlive the workgroup's LDS allocation
}

// workgroup -> (channel group g, image lane il, lanes): the group is FIXED for the whole launch.  XCD-aware form:
// workgroups k and k + 8 share an XCD and its L2; XCD x owns channel-group set x % nsets (gx consecutive groups, chosen
// by the host so that their packed weights stay L2-resident) and image partition x / nsets.
__device__ __forceinline__ void fp6v2_wg_map(const V2Args& a, int& g, int& il, int& lanes) {
  const int k = blockIdx.x, G = a.Cout >> 5;
  if (a.gx > 0) {
    const int S = gridDim.x >> 3, x = k & 7, slot = k >> 3;
    const int npart = 8 / a.nsets, set = x % a.nsets, xi = x / a.nsets, lanes_x = S / a.gx;
    g = set * a.gx + slot % a.gx;
    il = xi * lanes_x + slot / a.gx;
    lanes = npart * lanes_x;
  } else {
    g = k % G;
    il = k / G;
    lanes = gridDim.x / G;
  }
}

// Hand-over to the tail launch (spk_cert_handover): the tail launch then needs no ordering between its repair part (which reads the
// count) and anything that resets it: repair and last position run as ONE launch.
__device__ __forceinline__ void fp6v2_handover(const V2Args& a) {
  if (!a.handover) return;
  __syncthreads();
  if (threadIdx.x == 0) spk_cert_handover(a.ws);
}

template <int H, int W, int NWV, bool SPLIT = false>
__global__ __launch_bounds__(NWV * 64, 1) void conv3x3_fp6v2_kernel(V2Args a) {
  const int Bn = spk_batch_count(a.n_dyn, a.B);
  int g, il, lanes;
  fp6v2_wg_map(a, g, il, lanes);
  if constexpr (NWV == 8 && !SPLIT) {
    // full 7x7 items: every wave runs the body of its class (wave-uniform; the eight waves meet at the same barriers whichever
    // body they are in: the zeroing, one per chunk, two per item, the hand-over).  Five bodies are 68 KB of code against 15 KB for
    // one (217 registers, no scratch: profiles/tap_pair_resources.txt).  Top, right and left sharing ONE body whose tap offsets and weight-tile offsets
    // sit in SGPRs (one address add per LDS read, 43 KB) measured the same: 77.5-78.1 against 77.5-77.8 ms per dense reverse
    // process (profiles/border_skip_ab.txt) -- the compile-time form is kept, it needs no second addressing path.
    switch (__builtin_amdgcn_readfirstlane((int)V2_WAVE_CLS[(threadIdx.x >> 6) & 7])) {
      case V2_TOP: fp6v2_body<H, W, NWV, false, 0, false, V2_TOP>(a, g, il, lanes, Bn, nullptr); break;
      case V2_RIGHT: fp6v2_body<H, W, NWV, false, 0, false, V2_RIGHT>(a, g, il, lanes, Bn, nullptr); break;
      case V2_LEFT: fp6v2_body<H, W, NWV, false, 0, false, V2_LEFT>(a, g, il, lanes, Bn, nullptr); break;
      case V2_BOTTOM: fp6v2_body<H, W, NWV, false, 0, false, V2_BOTTOM>(a, g, il, lanes, Bn, nullptr); break;
      default: fp6v2_body<H, W, NWV, false, 0, false, V2_INT>(a, g, il, lanes, Bn, nullptr); break;
    }
  } else fp6v2_body<H, W, NWV, SPLIT, 0>(a, g, il, lanes, Bn, nullptr);
  fp6v2_handover(a);
}

// Small batches: two half-image items per image (fp6v2_body HALF), four waves
template <int H, int W>
__global__ __launch_bounds__(256, 1) void conv3x3_fp6v2_half_kernel(V2Args a) {
  const int Bn = spk_batch_count(a.n_dyn, a.B);
  int g, il, lanes;
  fp6v2_wg_map(a, g, il, lanes);
  fp6v2_body<H, W, 4, false, 3, true>(a, g, il, lanes, Bn, nullptr);
  fp6v2_handover(a);
}

// Listed positions: the image lanes of every channel group are divided among the six tile-count classes in proportion to
// their work (slots x tiles, with a floor for the copy-bound small classes); a workgroup then runs the item loop
// instantiated for its class on that class's slots.  Every workgroup derives the same division from cls_cnt.
// (two waves per SIMD: a class of k tiles per wave of four becomes ceil(k / 2) tiles per wave of eight)
template <int H, int W, int NWV>
__global__ __launch_bounds__(NWV * 64, 1) void conv3x3_fp6v2_listed_kernel(V2Args a) {
  constexpr int NC = (H * W / 2) / 4;                    // classes: 1 .. NC tiles per wave
  // (the lists carry the image count of the spk_select_needed call that wrote them; a.n_dyn may have been lowered since: the tail
  //  launch follows it, and so must every store and flag of this one)
  const int Bn = spk_batch_count(a.n_dyn, a.B);
  int g, il, lanes;
  fp6v2_wg_map(a, g, il, lanes);
  int cnt[NC], work[NC], u[NC];
  int total = 0, nonempty = 0;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    cnt[k] = a.cls_cnt[k];
    work[k] = cnt[k] * (k + 1 < SPK_V2_KMIN ? SPK_V2_KMIN : k + 1);
    total += work[k];
    nonempty += cnt[k] > 0;
  }
  if (total == 0) { fp6v2_handover(a); return; }
  // one lane per non-empty class, the rest in proportion, leftovers to the class with the most work per lane
  int rem = lanes - nonempty, used = 0;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    u[k] = cnt[k] > 0 ? 1 + (int)((long long)rem * work[k] / total) : 0;
    used += u[k];
  }
  for (int left = lanes - used; left > 0; --left) {
    int best = 0;
    long long bw = -1, bu = 1;
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (cnt[k] > 0 && (long long)work[k] * bu > bw * u[k]) { bw = work[k]; bu = u[k]; best = k; }
#pragma unroll
    for (int k = 0; k < NC; ++k) u[k] += (k == best);
  }
  int start = 0, cls = -1, il_c = 0, lanes_c = 1;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    if (il >= start && il < start + u[k]) { cls = k; il_c = il - start; lanes_c = u[k]; }
    start += u[k];
  }
  const int* slots = a.cls_list + (long long)(cls < 0 ? 0 : cls) * a.B;
  static_assert(NWV == 8, "listed positions: two waves per SIMD");
  switch (cls) {
    case 0: case 1: fp6v2_body<H, W, 8, false, 1>(a, g, il_c, lanes_c, cnt[cls], slots, Bn); break;
    case 2: case 3: fp6v2_body<H, W, 8, false, 2>(a, g, il_c, lanes_c, cnt[cls], slots, Bn); break;
    case 4: case 5: fp6v2_body<H, W, 8, false, 3>(a, g, il_c, lanes_c, cnt[cls], slots, Bn); break;
    default: break;
  }
  fp6v2_handover(a);
}

// ------------------------------------------------------------------------------------------------ tail launches
// (1) the last position of every image, exactly: one workgroup = two images x one channel group (a 32-row tile whose lane
//     halves are the images), its waves splitting the K chunks; the four taps that reach position (H-1, W-1) from inside
//     the image; operands straight from L2; all six digits (the two sixth-digit tiles of the slab), fp64 recombination.
// (2) the flagged neurons of the main launch, exactly (fixup_neuron / fp6v2_fixup_kernel below).

// red: ONE [3][16][64] buffer (the partial sums of waves 1 .. 3 pass through it one after the other: the merged tail launch
// keeps eight workgroups on a CU) or, WIDE, three of them (one barrier: the stand-alone launch of full batches)
template <int H, int W, bool WIDE>
__device__ __forceinline__ void fp6v2_lastpos_body(const V2Args& a, const int bid, float (*red)[16][64]) {
  constexpr int HW = H * W, NP = SPK_V2_LP_PAIRS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = a.nch, G = a.Cout >> 5;
  const int Bn = spk_batch_count(a.n_dyn, a.B);
  // (without the hand-over this launch follows the repair launch on the stream and re-arms the flag counter)
  if (!a.handover && bid == 0 && threadIdx.x == 0) { a.ws.flags[1] = a.ws.flags[0]; a.ws.flags[0] = 0u; }
  // one unit = NP 32-row tiles = NP image pairs (the lane halves of a tile are the two images) x one channel group: the
  // weight tiles of a chunk are read ONCE for all of them (with one pair per unit the launch moved 327 MB of weight tiles
  // through L2 for the 256 -> 512 layer at B = 256: bound by that).  The four waves of a workgroup split the K chunks
  // (wave w: chunks w, w + 4, ...) and add their partial sums -- exact integers below 2^24 in fp32, so the order of the
  // additions does not matter -- in LDS: few units are bound by the latency of a wave's chain of dependent gathers
  // (with many units the launch is bound by throughput instead: then every wave takes a unit of its own)
  const int n_units = ((Bn + 2 * NP - 1) / (2 * NP)) * G;
  const bool split = n_units <= SPK_V2_LP_SPLIT_MAX;        // (uniform over the launch)
  const int unit = split ? bid : bid * 4 + wave;
  const int g = unit % G, b0 = (unit / G) * 2 * NP;
  if (b0 >= Bn) return;
  const int row = lane & 31, half = lane >> 5;
  const int hsel = (row >> 2) & 1, tt = (row & 3) + 4 * (row >> 3);
  const int sc_a = 0x7f7f7f7f;
  const int sc_p = half ? (int)0x82828282u : (int)0x87878787u;
  const int sc_hi = (int)0x87878787u, sc_lo = (int)0x82828282u;
  v16f acc[NP][3];
#pragma unroll
  for (int q = 0; q < NP; ++q)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][j][r] = 0.f;
  const int py = H - 1, px = W - 1;
  for (int c = split ? wave : 0; c < nch; c += split ? 4 : 1) {
    const uint8_t* wslab = a.wq + ((long long)g * nch + c) * W_SLAB;
    auto ldb = [&](int tile) -> v8i {
      const uint8_t* wt = wslab + tile * WT;
      const v4i bx = *reinterpret_cast<const v4i*>(wt + lane * 16);
      const v2i by = *reinterpret_cast<const v2i*>(wt + 1024 + lane * 8);
      return v8i{bx[0], bx[1], bx[2], bx[3], by[0], by[1], 0, 0};
    };
    // spikes of the four contributing taps (0, 1, 3, 4)
    v4i sp[NP][4];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int bA = b0 + 2 * q + hsel;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int tap = (u >> 1) * 3 + (u & 1);
        const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
        sp[q][u] = v4i{0, 0, 0, 0};
        if (bA < Bn)
          sp[q][u] = *reinterpret_cast<const v4i*>(a.in0 + (((long long)bA * nch + c) * HW + yy * W + xx) * POSB + tt * 16);
      }
    }
    // all thirteen weight tiles of the chunk are requested before the first MFMA waits
    v8i bt[8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int tap = (u >> 1) * 3 + (u & 1);
      bt[2 * u] = ldb(2 * tap); bt[2 * u + 1] = ldb(2 * tap + 1);
    }
    const v8i t18 = ldb(N_PAIR), t19 = ldb(N_PAIR + 1), t20 = ldb(N_PAIR + 2), t23 = ldb(N_MAIN), t24 = ldb(N_MAIN + 1);
    auto mm = [&](v16f& d, const v4i& av, const v8i& bv, int sb) {
      const v8i a8 = {av[0], av[1], av[2], av[3], 0, 0, 0, 0};
      d = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, bv, d, 4, 2, 0, sc_a, 0, sb);
    };
    const v4i zero = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < NP; ++q) {
#pragma unroll
      for (int u = 0; u < 4; ++u) { mm(acc[q][0], sp[q][u], bt[2 * u], sc_p); mm(acc[q][1], sp[q][u], bt[2 * u + 1], sc_p); }   // digit pairs 01, 23
      // fifth digit (x 32) and sixth digit into acc[2] = 32 * D4 + D5: tiles 18 (taps 0|1), 19 (2|3), 20 (4|5) and the
      // sixth-digit tiles 23 (taps 0|1), 24 (taps 3|4); taps 2 and 5 lie outside the image: zero spikes
      const v4i a01 = half ? sp[q][1] : sp[q][0];
      const v4i az3 = half ? sp[q][2] : zero;
      const v4i a4z = half ? zero : sp[q][3];
      const v4i a34 = half ? sp[q][3] : sp[q][2];
      mm(acc[q][2], a01, t18, sc_hi); mm(acc[q][2], az3, t19, sc_hi); mm(acc[q][2], a4z, t20, sc_hi);
      mm(acc[q][2], a01, t23, sc_lo); mm(acc[q][2], a34, t24, sc_lo);
    }
  }
  if (split) {
    const int nw = nch < 4 ? nch : 4;                       // waves that had a chunk
    if constexpr (WIDE) {
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        if (q) __syncthreads();
        if (wave != 0 && wave < nw) {
#pragma unroll
          for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) red[3 * (wave - 1) + j][r][lane] = acc[q][j][r];
        }
        __syncthreads();
        if (wave == 0) {
          for (int w = 1; w < nw; ++w)
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
              for (int r = 0; r < 16; ++r) acc[q][j][r] += red[3 * (w - 1) + j][r][lane];
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < NP; ++q)
        for (int w = 1; w < 4; ++w) {
          if (wave == w && w < nw) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
              for (int r = 0; r < 16; ++r) red[j][r][lane] = acc[q][j][r];
          }
          __syncthreads();
          if (wave == 0 && w < nw) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
              for (int r = 0; r < 16; ++r) acc[q][j][r] += red[j][r][lane];
          }
          __syncthreads();
        }
    }
    if (wave != 0) return;
  }
  const int co = g * 32 + (lane & 31);
  const double sc = a.scale[co], bi = a.bias[co];
  const float bna = a.bn_a[co], bnb = a.bn_b[co];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int b = b0 + 2 * q + half;                        // accumulator lane half == image within the tile's pair
    const bool ok = b < Bn;
    if (__builtin_amdgcn_ballot_w64(ok) == 0ull) continue;  // (a ragged last unit: no image in this pair)
    float v = 0.f;
    unsigned mybits = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const double s1 = fma((double)acc[q][0][r], 1024.0, (double)acc[q][1][r]);    // exact
      const double s = fma(s1, 1024.0, (double)acc[q][2][r]);                       // exact: |s| < 2^43
      const float y = exact_preact(s, sc, bi);                                      // the one rounding to fp32
      const bool sp1 = spk_lif_step_default(v, fmaf(y, bna, bnb)) && ok;
      mybits |= sp1 ? (1u << r) : 0u;
    }
    const long long cell = ((long long)(ok ? b : 0) * G + g) * HW + (HW - 1);
    store_tile_spikes(a.out, a.out_cnt, mybits, lane, cell * POSB, cell * 32, ok);
  }
}

// (2) One flagged neuron, exactly, by a 256-thread workgroup: thread unit (tap, 32-channel chunk, t) reads ONE 16-byte spike
// record and the 32 quantised weights of its (channel, tap, chunk) from the int32 table the pack kernel wrote (the same
// rint(w * 2^s) as the digit tiles) and sums the active ones in 64 bits; partial sums meet per time step through two lane
// shuffles and 16 LDS atomics per wave; then the first wave runs the exact epilogue in every lane (fp64 recombination of the
// exact sum -- the arithmetic of den_mfma_fp6.hip -- the reference's BN and LIF steps) and lane t patches the nibble of step t.
// Eight such workgroups fit a CU: a few thousand flagged neurons are one or two rounds, bound by the L2 reads (18 - 55 KB a neuron).
template <int H, int W>
__device__ __forceinline__ void fixup_neuron(const V2Args& a, long long n, unsigned long long* sS, int Bn) {
  constexpr int HW = H * W;
  const int tid = threadIdx.x, lane = tid & 63;
  const int nch = a.nch, Cin = a.Cin;
  const int p = (int)(n % HW);
  const long long r0 = n / HW;
  const int co = (int)(r0 % a.Cout), b = (int)(r0 / a.Cout);
  if (b >= Bn) return;                                     // (uniform over the workgroup)
  const int py = p / W, px = p % W;
  if (tid < 16) sS[tid] = 0ull;
  long long part = 0;
  __syncthreads();
  const int units = 9 * nch * 16;
  for (int u = tid; u < units; u += (int)blockDim.x) {
    const int t = u & 15, cc = (u >> 4) % nch, tap = (u >> 4) / nch;
    const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
    const uint4 sp = *reinterpret_cast<const uint4*>(a.in0 + (((long long)b * nch + cc) * HW + yy * W + xx) * POSB + t * 16);
    const int4* qp = reinterpret_cast<const int4*>(a.qtab + ((long long)co * 9 + tap) * Cin + cc * 32);
    const unsigned w4[4] = {sp.x, sp.y, sp.z, sp.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) spk_cert_add_active8(part, w4[j], qp[2 * j], qp[2 * j + 1]);     // channels 8j .. 8j + 7
  }
  // lanes l, l + 16, l + 32, l + 48 of a wave hold the same time step (t = u & 15; the block size is a multiple of 64)
  part = spk_cert_sum_quarters(part);
  if (lane < 16 && part != 0) atomicAdd(&sS[lane], (unsigned long long)part);
  __syncthreads();
  if (tid < 64) {
    const double sc = a.scale[co], bi = a.bias[co];
    const float bna = a.bn_a[co], bnb = a.bn_b[co];
    float v = 0.f;
    unsigned bits = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const float y = exact_preact((double)(long long)sS[t], sc, bi);
      bits |= spk_lif_step_default(v, fmaf(y, bna, bnb)) ? (1u << t) : 0u;
    }
    const int g = co >> 5;
    if (lane < 16) {
      uint8_t* rec = a.out + ((((long long)b * (a.Cout >> 5) + g) * HW + p) * POSB);
      spk_cert_patch_nibble(rec + lane * 16, co, (bits >> lane) & 1u);
    }
    if (a.out_cnt && lane == 0) a.out_cnt[(((long long)b * (a.Cout >> 5) + g) * HW + p) * 32 + (co & 31)] = (uint8_t)__popc(bits);
  }
  __syncthreads();
}

template <int H, int W>
__device__ __forceinline__ void fp6v2_fixup_body(const V2Args& a, long long n_words, const unsigned bid, const unsigned nb,
                                                 unsigned long long* sS) {
  const int Bn = spk_batch_count(a.n_dyn, a.B);
  const unsigned count = a.ws.flags[a.handover ? 1 : 0];       // published by the main launch (fp6v2_handover), or live
  spk_cert_scan<true>(a.ws, count, bid, nb, n_words, threadIdx.x == 0,
                      [&](long long n) __attribute__((always_inline)) { fixup_neuron<H, W>(a, n, sS, Bn); });
}

// (1b) Round 5: the last position with the weight tiles SHARED through LDS.  fp6v2_lastpos_body reads the thirteen tiles of every
// chunk straight from L2 per image pair: 320 MB per launch for the 256 -> 512 layer at B = 256, which is what its ~20 us are.
// Here a workgroup takes FOUR image pairs of one channel group -- a wave each, every wave walks all the chunks -- and a chunk's
// thirteen tiles (19.5 KB: the four contributing taps' digit pairs, three fifth-digit tiles, two sixth-digit tiles; four runs
// of the slab) come in ONCE per workgroup by LDS-DMA, double-buffered (39 KB), one barrier per chunk: 80 MB.  No partial sums
// cross waves; the epilogue is the exact one of fp6v2_lastpos_body.
// THE CHUNK PIPELINE.  A wave's chain is nch chunks of thirteen MFMAs (~0.25 us each); what it can wait for is the L2 -> LDS round trip
// of a chunk's tiles and the L2 -> register round trip of its four spike fragments.  Step c issues the fragment loads of chunk c + 1,
// then the wave's five tile pieces of chunk c + 1 into the other buffer, then runs chunk c's thirteen MFMAs, and only THEN waits --
// once, for both: both round trips lie under the MFMAs.  What that takes, with copies the compiler cannot see and loads it can:
//   - the fragment loads are unconditional (a wave whose image pair lies past the batch reads the last image's fragments: its rows
//     are never stored).  Zero-filled registers with a load under `if (image < Bn)` made hipcc protect the zero moves with a
//     vmcnt(0) right BEHIND the copies of chunk c + 1: that round trip was fully exposed;
//   - the step ends in an empty asm that takes the next fragments as in/out operands: hipcc waits for them there (vmcnt(0): it
//     counts only the loads it can see, so the wait also retires the copies, which barrier c + 1 needs anyway) and the registers
//     the next step's MFMAs read carry no pending load.  Before, a vmcnt(1) in front of the step's first MFMA stood BEHIND the
//     fragment loads just issued for chunk c + 1 and retired three of the four: the second exposed round trip.  Together ~1.2 us
//     per chunk, 16 / 8 / 4 / 2 chunks.
// Deeper (profiles/lastpos_ring_ab.txt): a ring of three tile buffers and a counted wait need the fragments out of the compiler's
// sight as well (its own vmcnt in front of a visible fragment's use drains the copies issued behind it).  Assembly loads into
// registers are moved by hipcc while in flight (loop copies in front of the wait that names them); through LDS-DMA into two
// wave-private sets the ring of three (76 KB) and the same form with two buffers (56 KB) are bit-equal and measured
// den.conv4 / conv5 +5 us per launch: the dynamic LDS of a launch is every workgroup's, the repair workgroups' too, and over 40 KB
// only two of them are resident per CU, not four.  The repair half sets the length of these launches once the last positions are
// short; a ring of four needs a third fragment set on top (the in-order counter retires chunk c + 2's tiles with chunk c + 1's
// fragments): 82.5 KB, one workgroup per CU.
constexpr int LPS_TILES = 13, LPS_BUF = LPS_TILES * WT;                  // 19 968 B per chunk
constexpr int LPS_RING = 2;             // chunk buffers
constexpr size_t LPS_LDS = LPS_RING * (size_t)LPS_BUF;
static_assert(LPS_RING == 2 && 4 * (LPS_LDS + 128) <= 160 * 1024,
              "barrier c releases buffer (c + 1) % 2, the one chunk c - 1 was read from, never chunk c's; four workgroups per CU (128 B static each)");
template <int H, int W>
__device__ __forceinline__ void fp6v2_lastpos_shared_body(const V2Args& a, const int bid) {
  constexpr int HW = H * W;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = a.nch, G = a.Cout >> 5;
  const int Bn = a.n_dyn ? (*a.n_dyn < a.B ? *a.n_dyn : a.B) : a.B;     // spk_batch_count of spk_common.h, written out
  const int g = bid % G, b0 = (bid / G) * 8;
  if (b0 >= Bn) return;                                     // (uniform over the workgroup)
  const int row = lane & 31, half = lane >> 5;
  const int hsel = (row >> 2) & 1, tt = (row & 3) + 4 * (row >> 3);
  const int sc_a = 0x7f7f7f7f;
  const int sc_p = half ? (int)0x82828282u : (int)0x87878787u;
  const int sc_hi = (int)0x87878787u, sc_lo = (int)0x82828282u;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const unsigned lds_addr = spk_lds_addr(lds), lane16 = (unsigned)lane * 16u;
  // the slab's four runs -> twenty pieces (one of them half a piece), five per wave: piece k of the wave = 5 * wave + k
  auto issue_chunk = [&](int c, int buf) {
    const uint8_t* slab = a.wq + ((long long)g * nch + c) * W_SLAB;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int pc = 5 * wave_s + k;                        // 0..19
      // pieces 0..5: tiles 0..3; 6..11: tiles 6..9; 12..16: tiles 18..20 (16 = the half piece); 17..19: tiles 23, 24
      const int src = pc < 6 ? pc * 1024 : pc < 12 ? 6 * WT + (pc - 6) * 1024 : pc < 17 ? 18 * WT + (pc - 12) * 1024
                                                                                        : 23 * WT + (pc - 17) * 1024;
      const int dst = pc < 6 ? pc * 1024 : pc < 12 ? 4 * WT + (pc - 6) * 1024 : pc < 17 ? 8 * WT + (pc - 12) * 1024
                                                                                        : 11 * WT + (pc - 17) * 1024;
      const unsigned long long mask = pc == 16 ? 0xffffffffull : ~0ull;
      spk_dma16s_masked(slab + src, lane16, lds_addr + (unsigned)(buf * LPS_BUF + dst), mask);
    }
  };
  const int py = H - 1, px = W - 1;
  // the image whose rows this lane feeds (A layout); past the batch: the last image's (loaded, multiplied, never stored)
  const int bA = b0 + 2 * wave + hsel, bAc = bA < Bn ? bA : Bn - 1;
  auto load_spikes = [&](int c, v4i (&sp)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int tap = (u >> 1) * 3 + (u & 1);
      const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
      sp[u] = *reinterpret_cast<const v4i*>(a.in0 + (((long long)bAc * nch + c) * HW + yy * W + xx) * POSB + tt * 16);
    }
  };
  v16f acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  v4i sp[4], spn[4];
  load_spikes(0, sp);
  issue_chunk(0, 0);
  asm volatile("" : "+v"(sp[0]), "+v"(sp[1]), "+v"(sp[2]), "+v"(sp[3]));
  for (int c = 0; c < nch; ++c) {
    const int buf = c & (LPS_RING - 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's pieces of chunk c are in (with the fragments, at the end of step c - 1)
    __syncthreads();                                        // everyone's are; everyone is done with the other buffer
    // (clamped, not skipped: the loads of the last step re-read chunk nch - 1's fragments -- no branch, no moves into spn)
    load_spikes(c + 1 < nch ? c + 1 : c, spn);
    if (c + 1 < nch) issue_chunk(c + 1, buf ^ 1);
    const uint8_t* Wb = lds + buf * LPS_BUF;
    // (the assembly form of the main kernel: four- and six-register operands; the builtin wants eight-register tuples padded
    //  with zeros for both, which is what pushed this body past 168 registers)
    auto ldb = [&](int tile) -> v6i {
      const uint8_t* wt = Wb + tile * WT;
      const v4i bx = *reinterpret_cast<const v4i*>(wt + lane * 16);
      const v2i by = *reinterpret_cast<const v2i*>(wt + 1024 + lane * 8);
      return v6i{bx[0], bx[1], bx[2], bx[3], by[0], by[1]};
    };
    auto mm = [&](v16f& d, const v4i& av, const v6i& bv, int sb) { SPK_MFMA_FP6("v", d, av, bv, sc_a, sb); };
    // (fences: at most four tiles in flight -- left alone hipcc requests all thirteen first: 188 registers, two workgroups per CU)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const v6i t0 = ldb(2 * u), t1 = ldb(2 * u + 1);
      mm(acc[0], sp[u], t0, sc_p); mm(acc[1], sp[u], t1, sc_p);
      if (u & 1) __builtin_amdgcn_sched_barrier(0);
    }
    const v4i zero = {0, 0, 0, 0};
    const v4i a01 = half ? sp[1] : sp[0];
    const v4i az3 = half ? sp[2] : zero;
    const v4i a4z = half ? zero : sp[3];
    const v4i a34 = half ? sp[3] : sp[2];
    {
      const v6i t8 = ldb(8), t9 = ldb(9), t10 = ldb(10);
      mm(acc[2], a01, t8, sc_hi); mm(acc[2], az3, t9, sc_hi); mm(acc[2], a4z, t10, sc_hi);
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      const v6i t11 = ldb(11), t12 = ldb(12);
      mm(acc[2], a01, t11, sc_lo); mm(acc[2], a34, t12, sc_lo);
    }
    __builtin_amdgcn_sched_barrier(0);
    // the one wait of the step: hipcc waits for the visible fragment loads in front of this statement
    asm volatile("" : "+v"(spn[0]), "+v"(spn[1]), "+v"(spn[2]), "+v"(spn[3]));
#pragma unroll
    for (int u = 0; u < 4; ++u) sp[u] = spn[u];
  }
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");        // (the MFMAs are opaque to the hazard recognizer: accumulator reads below)
  const int co = g * 32 + (lane & 31);
  const double sc = a.scale[co], bi = a.bias[co];
  const float bna = a.bn_a[co], bnb = a.bn_b[co];
  const int b = b0 + 2 * wave + half;                       // accumulator lane half == image within the pair
  const bool ok = b < Bn;
  if (__builtin_amdgcn_ballot_w64(ok) == 0ull) return;
  float v = 0.f;
  unsigned mybits = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const double s1 = fma((double)acc[0][r], 1024.0, (double)acc[1][r]);
    const double s2 = fma(s1, 1024.0, (double)acc[2][r]);
    const float y = exact_preact(s2, sc, bi);
    const bool sp1 = spk_lif_step_default(v, fmaf(y, bna, bnb)) && ok;
    mybits |= sp1 ? (1u << r) : 0u;
  }
  const long long cell = ((long long)(ok ? b : 0) * G + g) * HW + (HW - 1);
  store_tile_spikes(a.out, a.out_cnt, mybits, lane, cell * POSB, cell * 32, ok);
}

// The tail launches.  PART 0: workgroups [0, n_lp) compute last positions, the rest repair flagged neurons -- independent work
// (disjoint outputs, both read only the layer's input), each a chain of dependent L2 reads: in one launch they overlap (the
// sampler's active-set calls).  PART 1 / 2: repair only / last positions only, each with its own register and LDS budget (full
// batches, where either part fills the device by itself: the merged form measured 1.3 % slower there).
// PART 3 (round 5): PART 0 with the last positions of fp6v2_lastpos_shared_body (39 KB of dynamic LDS per workgroup: four per CU).
// (HIP's second launch-bound argument = waves per SIMD the kernel must leave room for: four workgroups of PART 3 per CU -> 128 registers;
//  123 used, no scratch: profiles/lastpos_ring_resources.txt)
template <int H, int W, int PART>
__global__ __launch_bounds__(256, PART == 3 ? 4 : 1) void fp6v2_tail_kernel(V2Args a, long long n_words, int n_lp) {
  __shared__ float red[(PART == 1 || PART == 3) ? 1 : (PART == 2 ? 9 : 3)][16][64];
  __shared__ unsigned long long sS[16];
  if constexpr (PART == 3) {
    if ((int)blockIdx.x < n_lp) { if constexpr ((H * W) & 1) fp6v2_lastpos_shared_body<H, W>(a, (int)blockIdx.x); }
    else fp6v2_fixup_body<H, W>(a, n_words, blockIdx.x - (unsigned)n_lp, gridDim.x - (unsigned)n_lp, sS);
    (void)red;
  } else {
    if (PART == 2 || (PART == 0 && (int)blockIdx.x < n_lp)) fp6v2_lastpos_body<H, W, PART == 2>(a, (int)blockIdx.x, red);
    else fp6v2_fixup_body<H, W>(a, n_words, blockIdx.x - (unsigned)n_lp, gridDim.x - (unsigned)n_lp, sS);
  }
}

// ------------------------------------------------------------------------------------------------ weight packing
// one block per output channel: channel maximum -> shift s, every weight -> six balanced radix-32 digits, written as the
// per-lane 24-byte B fragments (spk_cert_emit_fragment: lane = K half * 32 + channel within the group of 32).  Tile order per
// (group, 32-channel chunk): (tap, pair) x 18 [K half 0: even digit, half 1: odd digit, same 32 input channels], fifth digit
// x 5 [K half 0: tap 2q, half 1: tap 2q + 1], sixth digit x 2 [taps (0, 1) and (3, 4)].  Also the L1 norm of the quantised weights.
__global__ __launch_bounds__(256) void pack_fp6v2_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                         uint8_t* __restrict__ wq, double* __restrict__ scale,
                                                         double* __restrict__ bias_d, float* __restrict__ wl1,
                                                         int* __restrict__ qtab, int Cout, int Cin) {
  __shared__ float smax[256];
  __shared__ double ssum[256];
  const int co = blockIdx.x, n = Cin * 9;
  const float* wc = w + (long long)co * n;
  float m = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(wc[i]));
  const int sh = 29 - spk_channel_exponent(smax, m);     // |w| * 2^sh < 2^29 <= 16.5 * 32^5
  double l1 = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double q = spk_cert_quantise(wc[i], sh);
    l1 += fabs(q);
    const int ci = i / 9, tap = i - 9 * ci;
    qtab[((long long)co * 9 + tap) * Cin + ci] = (int)q;          // |q| < 2^29
  }
  ssum[threadIdx.x] = l1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) ssum[threadIdx.x] += ssum[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    spk_cert_scale_bias(scale, bias_d, bias, co, sh);
    wl1[co] = (float)(ldexp(ssum[0], -sh) * 1.000001);      // rounded up: it feeds an upper bound
  }
  const int nchunks = Cin / CK, g = co >> 5, col = co & 31;
  constexpr int NTILE = N_MAIN + N_L5;
  for (int rec = threadIdx.x; rec < nchunks * NTILE * 2; rec += 256) {
    const int kh = rec & 1, tau = (rec >> 1) % NTILE, c = rec / (2 * NTILE);
    int tap, digit;
    bool valid = true;
    if (tau < N_PAIR) { tap = tau >> 1; digit = 2 * (tau & 1) + kh; }
    else if (tau < N_MAIN) { tap = 2 * (tau - N_PAIR) + kh; digit = 4; valid = tap < 9; }
    else { tap = (tau == N_MAIN ? 0 : 3) + kh; digit = 5; }
    spk_cert_emit_fragment(wq + (long long)(g * nchunks + c) * W_SLAB + tau * WT, kh * 32 + col, digit, valid,
                           [&](int j) { return (long long)spk_cert_quantise(wc[(c * CK + j) * 9 + tap], sh); });
  }
}

}  // namespace

extern "C" long long spk_den_packed_weight_fp6v2_bytes(int Cout, int Cin) {
  if (Cout <= 0 || Cin <= 0 || (Cout % 32) || (Cin % CK)) return -1;
  return (long long)(Cout / 32) * (Cin / CK) * W_SLAB;
}

extern "C" int spk_den_pack_weight_fp6v2(const float* w, const float* bias, uint8_t* wq, double* scale, double* bias_d,
                                         float* wl1, int* qtab, int Cout, int Cin, hipStream_t stream) {
  if (!w || !wq || !scale || !bias_d || !wl1 || !qtab || Cout <= 0 || Cin <= 0) return SPK_ERR_ARG;
  if ((Cout % 32) || (Cin % CK)) return SPK_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pack_fp6v2_kernel, dim3(Cout), dim3(256), 0, stream, w, bias, wq, scale, bias_d, wl1, qtab, Cout, Cin);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" long long spk_den_fp6v2_flag_words(int B, int Cout, int H, int W) {
  if (B <= 0 || Cout <= 0 || H <= 0 || W <= 0) return -1;
  return spk_cert_flag_words((long long)B * Cout * H * W);
}

extern "C" int spk_den_conv3x3_mfma_fp6v2_supported(int Cout, int Cin, int k, int stride, int pad, int T, int H, int W) {
  return k == 3 && stride == 1 && pad == 1 && T == T16 && H == W && (H == 7 || H == 8) && Cout > 0 && Cin > 0 &&
         (Cout % 32) == 0 && (Cin % CK) == 0;
}

static int fp6v2_launch(const uint8_t* in_s32, int nch, const uint8_t* wq, const double* scale, const double* bias_d,
                        const float* wl1, const int* qtab, const float* bn_a, const float* bn_b, uint8_t* out_s32,
                        uint8_t* out_counts, unsigned* flag_words, int T, int B, int H, int W, int Cout,
                        const int* n_dyn_or_null, const uint8_t* need, int need_R, int need_r, int flag_cap, int form,
                        hipStream_t stream, int parts = 7) {
  const bool split_small = form == 0;                        // (form 1: whole-image items at any batch size)
  if (!in_s32 || nch <= 0 || !wq || !scale || !bias_d || !wl1 || !qtab || !bn_a || !bn_b || !out_s32 || !flag_words ||
      B <= 0 || H <= 0 || W <= 0 || Cout <= 0)
    return SPK_ERR_ARG;
  if (!spk_den_conv3x3_mfma_fp6v2_supported(Cout, nch * CK, 3, 1, 1, T, H, W)) return SPK_ERR_UNSUPPORTED;
  const bool bands = H == 8;                                 // (8x8: two row bands per image; else 7x7)
  if (need && (bands || !n_dyn_or_null)) return SPK_ERR_UNSUPPORTED;   // (not in the predicate: a property of the call's lists, not of the shape)
  V2Args a;
  a.in0 = in_s32; a.nch = nch; a.wq = wq; a.scale = scale; a.bias = bias_d; a.wl1 = wl1; a.qtab = qtab;
  a.bn_a = bn_a; a.bn_b = bn_b; a.out = out_s32; a.out_cnt = out_counts;
  a.ws = spk_cert_ws(flag_words, flag_cap, (long long)B * Cout * H * W);
  a.n_dyn = n_dyn_or_null;
  a.need = nullptr; a.cls_cnt = nullptr; a.cls_list = nullptr;
  if (need) {
    a.need = need + spk_need_off_rec(B, need_R, need_r);
    a.cls_cnt = reinterpret_cast<const int*>(need + spk_need_off_cnt(need_r));
    a.cls_list = reinterpret_cast<const int*>(need + spk_need_off_list(B, need_R, need_r));
  }
  a.B = B; a.Cout = Cout; a.Cin = nch * CK;
  const int cus = spk_cu_count();
  const int G = Cout / 32;
  // XCD-aware walk: the largest power-of-two group count per XCD whose packed weights fit ~1.5 MB of its 4 MB L2
  int grid = 0;
  a.gx = 0; a.nsets = 1;
  // (wgs: workgroups of the launch; returns the grid, 0 if the XCD-aware walk does not fit)
  // (the sampler's active-set and listed calls keep the rounds 2-5 bound: with few image lanes per channel group two sets measured 1.2 %
  //  slower there -- elimination + lists 34.37 against 33.96 ms, three alternating passes -- while full batches are indifferent in time and
  //  fetch a third less: profiles/r6_ab_kernel_variants.txt (2))
  const long long gx_kb = (n_dyn_or_null || need) ? 1536 : SPK_V2_GX_KB;
  auto xcd_walk = [&](V2Args& v, int wgs) -> int {
    v.gx = 0; v.nsets = 1;
    if ((wgs & 7) != 0) return 0;
    const int S = wgs / 8;
    int gx = 1;
    while (gx * 2 <= G && gx * 2 <= S && (long long)gx * 2 * nch * W_SLAB <= gx_kb * 1024) gx *= 2;
    while (G / gx > 8 && gx * 2 <= G && gx * 2 <= S) gx *= 2;
    const int nsets = G / gx;
    if (G % gx == 0 && nsets <= 8 && 8 % nsets == 0 && S % gx == 0) { v.gx = gx; v.nsets = nsets; return wgs; }
    return 0;
  };
  grid = xcd_walk(a, cus);
  if (a.gx == 0) grid = cus >= G ? (cus / G) * G : G;         // flat walk: workgroup k -> group k % G
  const int a_bytes = bands ? ((8 / 2 + 1 + 2) * 9 + 1) * POSB : ((7 + 2) * 8 + 1) * POSB;
  // (+ the active-input counters of the four-digit form: s_cin [cells][16], s_row [positions + 1][16])
  const size_t lds = 2 * ((size_t)a_bytes + W_LDS) + (size_t)((a_bytes / POSB) + (bands ? 32 : 49) + 1) * 64 + 256;   // (+ s_nmax)
  const long long n_words = spk_cert_bitmap_words((long long)B * Cout * H * W);
  // every main launch publishes the count for a merged tail launch (repair + last position as ONE launch: 1.6 % faster than two)
  a.handover = 1;
  if (parts != 7) {
    // measurement / debugging: re-run one tail part of the LAST launch on this workspace.  2 = the exact recomputation of
    // the neurons that launch flagged (count in ws[1], ids still listed: idempotent), 4 = the last position of every image.
    if (parts == 2) {
      if (bands) hipLaunchKernelGGL((fp6v2_tail_kernel<8, 8, 1>), dim3(8 * cus), dim3(256), 0, stream, a, n_words, 0);
      else hipLaunchKernelGGL((fp6v2_tail_kernel<7, 7, 1>), dim3(8 * cus), dim3(256), 0, stream, a, n_words, 0);
    } else if (parts == 4 && !bands) {
      const int n_lp4 = ((B + 2 * SPK_V2_LP_PAIRS - 1) / (2 * SPK_V2_LP_PAIRS)) * G;
      hipLaunchKernelGGL((fp6v2_tail_kernel<7, 7, 2>), dim3(n_lp4), dim3(256), 0, stream, a, n_words, n_lp4);
    } else return SPK_ERR_UNSUPPORTED;
    SPK_LAUNCH_CHECK();
    return SPK_OK;
  }
  if (bands) {
    hipLaunchKernelGGL((conv3x3_fp6v2_kernel<8, 8, 8, true>), dim3(grid), dim3(512), lds, stream, a);   // (eight waves: +4 % over four)
    SPK_LAUNCH_CHECK();
    hipLaunchKernelGGL((fp6v2_tail_kernel<8, 8, 1>), dim3(8 * cus), dim3(256), 0, stream, a, n_words, 0);   // (even latent: repair only)
    SPK_LAUNCH_CHECK();
    return SPK_OK;
  }
  // Two waves per SIMD since the four-digit form: the second wave is worth 8 % of the reverse process.  (Three, twelve waves of two
  // tiles, lose 11 %: den.conv4 launch 417-466 against 383-387 us, round 3; the staggered, duo and deferred-scan forms of round 5
  // are 4 - 40 % slower: profiles/r5_ab_duo_*.txt, profiles/r5_ab_defer_builds.txt.)
  if (need) {
    if (grid / G < 6) return SPK_ERR_UNSUPPORTED;           // one image lane per tile-count class at least (not in the predicate: the device's CU count)
    hipLaunchKernelGGL((conv3x3_fp6v2_listed_kernel<7, 7, 8>), dim3(grid), dim3(512), lds, stream, a);
  } else if (split_small && (long long)B * G * SPK_V2_HALF_FILL <= grid) {
    // fewer items than workgroups: two half-image items per image on four-wave workgroups (B = 16: conv2 / conv3 / conv5)
    hipLaunchKernelGGL((conv3x3_fp6v2_half_kernel<7, 7>), dim3(grid), dim3(256), lds, stream, a);
  } else hipLaunchKernelGGL((conv3x3_fp6v2_kernel<7, 7, 8>), dim3(grid), dim3(512), lds, stream, a);
  SPK_LAUNCH_CHECK();
  const int n_lp = ((B + 2 * SPK_V2_LP_PAIRS - 1) / (2 * SPK_V2_LP_PAIRS)) * G;
  if (!n_dyn_or_null && nch >= 2 && B >= SPK_V2_LPS_MIN_B &&
      (long long)LPS_LDS + 4096 <= spk_lds_limit()) {
    // round 5, full batches: last positions with LDS-shared weight tiles (eight images per workgroup), repairs beside them (four
    // workgroups per CU).  Same box, B = 256: den.conv4 / conv5 launches 386 / 373 -> 380 / 369 us, dense reverse process 91.6 -> 90.9 ms
    // (profiles/r5_ab_kernel_variants.txt (3)).  The sampler's active-set calls keep the form below: with few images the shared
    // form has too few units (elimination + lists 33.6 -> 34.7 ms)
    const int n_lps = ((B + 7) / 8) * G;
    hipLaunchKernelGGL((fp6v2_tail_kernel<7, 7, 3>), dim3(n_lps + 4 * cus), dim3(256), LPS_LDS, stream, a, n_words, n_lps);
    SPK_LAUNCH_CHECK();
  } else {
    // the sampler's active-set calls: few images, both parts are latency bound -- one launch (-17 us per reverse step)
    hipLaunchKernelGGL((fp6v2_tail_kernel<7, 7, 0>), dim3(n_lp + 8 * cus), dim3(256), 0, stream, a, n_words, n_lp);
    SPK_LAUNCH_CHECK();
  }
  return SPK_OK;
}

extern "C" int spk_den_conv3x3_mfma_fp6v2(const uint8_t* in_s32, int nch, const uint8_t* wq, const double* scale,
                                          const double* bias_d, const float* wl1, const int* qtab, const float* bn_a,
                                          const float* bn_b, uint8_t* out_s32, uint8_t* out_counts, unsigned* flag_words,
                                          int T, int B, int H, int W, int Cout, const int* n_dyn_or_null, int flag_cap,
                                          int form, hipStream_t stream) {
  if (form != 0 && form != 1) return SPK_ERR_ARG;
  return fp6v2_launch(in_s32, nch, wq, scale, bias_d, wl1, qtab, bn_a, bn_b, out_s32, out_counts, flag_words, T, B, H, W, Cout,
                      n_dyn_or_null, nullptr, 0, 0, flag_cap, form, stream);
}

extern "C" int spk_den_conv3x3_mfma_fp6v2_part(const uint8_t* in_s32, int nch, const uint8_t* wq, const double* scale,
                                               const double* bias_d, const float* wl1, const int* qtab, const float* bn_a,
                                               const float* bn_b, uint8_t* out_s32, uint8_t* out_counts, unsigned* flag_words,
                                               int T, int B, int H, int W, int Cout, const int* n_dyn_or_null, int part,
                                               int flag_cap, hipStream_t stream) {
  if (part != 2 && part != 4) return SPK_ERR_ARG;
  return fp6v2_launch(in_s32, nch, wq, scale, bias_d, wl1, qtab, bn_a, bn_b, out_s32, out_counts, flag_words, T, B, H, W, Cout,
                      n_dyn_or_null, nullptr, 0, 0, flag_cap, 1, stream, part);
}

extern "C" int spk_den_conv3x3_mfma_fp6v2_listed(const uint8_t* in_s32, int nch, const uint8_t* wq, const double* scale,
                                                 const double* bias_d, const float* wl1, const int* qtab, const float* bn_a,
                                                 const float* bn_b, uint8_t* out_s32, uint8_t* out_counts,
                                                 unsigned* flag_words, int T, int B, int H, int W, int Cout,
                                                 const int* n_dyn, const uint8_t* need, int need_radii, int radius,
                                                 int flag_cap, hipStream_t stream) {
  if (!need || !n_dyn || need_radii <= 0 || need_radii > 8 || radius < 1 || radius > need_radii) return SPK_ERR_ARG;
  return fp6v2_launch(in_s32, nch, wq, scale, bias_d, wl1, qtab, bn_a, bn_b, out_s32, out_counts, flag_words, T, B, H, W, Cout,
                      n_dyn, need, need_radii, radius - 1, flag_cap, 1, stream);
}
