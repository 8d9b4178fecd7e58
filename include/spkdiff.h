/* libspkdiff -- C-ABI of the MI355X-native (gfx950) Spiking-Diffusion inference kernels.
 *
 * This is the drop-in boundary for the reference's time-stepped SNN inference path.  The reference has no
 * FFI of its own for this path: its operator-plugin point is spikingjelly's ``backend`` switch
 * (SJ/activation_based/base.py:199-208, functional.py:109-149), whose only native plugin is the CuPy one with the
 * call contract  LIFNodeATGF.apply(x_seq[T,N], v[N], v_th, v_reset, 1/tau, ...)  (SJ/activation_based/neuron.py:954-966,
 * auto_cuda/neuron_kernel.py:496-522).  Every entry point below names the reference interface it replaces
 * (R/ = Spiking-Diffusion-release/, SJ/ = member of R/spikingjelly.zip).  INTEGRATION.md shows the ctypes stub.
 *
 * Contract (all functions):
 *   - plain C types only; every pointer is a DEVICE pointer owned by the caller (PyTorch); the library never
 *     allocates or frees device memory, reads no environment variable and keeps no mutable global state (the launch-shape
 *     choices of earlier rounds are fixed in the sources);
 *   - work is enqueued asynchronously on ``stream`` (a hipStream_t; pass torch.cuda.current_stream().cuda_stream);
 *   - returns 0 on success, SPK_ERR_* (< 0) for argument errors, a positive hipError_t for launch failures;
 *   - reentrant across streams and host threads.
 *
 * Layouts: "TBCHW" = fp32 [T,B,C,H,W] contiguous (the reference's tensors); "PTC" = u8 {0,1} [B,H,W,T,C]
 * (the library's compact inter-layer spike format); packed conv weights = fp32 [k*k][Cin][Cout].
 */
#ifndef SPKDIFF_H
#define SPKDIFF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* spk_stream_t; /* == hipStream_t */

#define SPK_VERSION 106 /* 0.1.6 -- bumped whenever an exported signature changes or entry points are added (round 4 inserted `int K`
                           * before the stream of spk_select_active / spk_select_needed: 101; round 5 added the VectorQuantizer's
                           * training branch and the training convolutions: 102, the token-table spike generator: 103; round 6: `int flag_cap` (and `int form` for spk_den_conv3x3_mfma_fp6v2) in front of the
                           * stream of the four certified-kernel entry points, spk_set_option / spk_get_option left the shipped library: 104;
                           * `active` / `n_active` of spk_den_step_tail: 105; the host-side shape
                           * predicates spk_*_supported / spk_vae_fp6_kind: 106); spkdiff/_lib.py reads its signatures from this header and
                           * refuses a library whose spk_version() differs.  Purely additive entry points (the SNN_VAE
                           * kernels spk_linear_lif_fwd / spk_svae_ar_fwd) keep the version: _lib.py resolves every declared
                           * symbol at import, so a library that lacks one fails there; so do spk_select_pending /
                           * spk_psample_step_conf_listed, DESIGN.md §4.16, the three `_sched` entry points, §4.17, and the three `_remask` entry points, §4.18: additive, still 106) */

/* return codes below zero (0: success; above zero: a hipError_t) */
#define SPK_ERR_ARG (-1)         /* bad argument: null pointer, non-positive size, contradictory combination */
#define SPK_ERR_UNSUPPORTED (-2) /* a shape or option this entry point has no kernel for; nothing was launched */

/* spike storage dtypes (spk_lif_fwd) */
#define SPK_SPIKE_F32 0
#define SPK_SPIKE_U8 1
#define SPK_SPIKE_BITS 2 /* one bit per neuron-step, 64 neurons per u64 word (wave ballot) */

/* fused-kernel epilogue modes (spk_conv_fused_fwd) */
#define SPK_CHUNK_C4 (-64) /* chunk_out value: fp4 nibble-packed output, 64 channels per chunk */
#define SPK_CHUNK_S32 (-32) /* chunk_out value: fp4 nibble-packed output, 32 channels per chunk ("S32", fp6v2 kernel) */
#define SPK_MODE_LIF 0    /* BN + LIF -> spikes                                    */
#define SPK_MODE_RAW 1    /* conv output per time step, fp32 TBCHW                 */
#define SPK_MODE_MEMOUT 2 /* sum_t x[t]*coef[t] (+tanh, +uint8)  -> [B,C,H,W]      */
#define SPK_MODE_MEAN 3   /* sum_t x[t] / T                      -> [B,C,H,W]      */

/* input kinds of spk_conv_fused_fwd */
#define SPK_IN_PTC 0  /* u8 spikes [B,H,W,T,C]                                               */
#define SPK_IN_TINV 1 /* fp32 [B,C,H,W], the same frame at every time step                  */
#define SPK_IN_SEQ 2  /* fp32 [T,B,C,H,W], arbitrary values (the reference's tensor format) */

int spk_version(void);
/* Returns a static string for an SPK_ERR_* / hipError_t code. */
const char* spk_error_string(int code);


/* ---- neuron surface -------------------------------------------------------------------------------------- */

/* Multi-step eval LIF (hard reset, decay_input): replaces LIFNode.multi_step_forward eval branch
 * SJ/activation_based/neuron.py:971-1011 -> jit_eval_multi_step_forward_hard_reset_decay_input :799-811, and mirrors the
 * cupy plugin contract :954-966.  x_seq [T,N] fp32; v_inout [N] fp32 (state before / after); spike_out [T,N] as
 * spike_dtype SPK_SPIKE_F32 = fp32, SPK_SPIKE_U8 = u8, SPK_SPIKE_BITS = bit-packed u64 words [T, ceil(N/64)] (bit l of word w =
 * neuron 64w+l). */
int spk_lif_fwd(const float* x_seq, float* v_inout, void* spike_out, int T, long long N, float tau, float v_threshold,
                float v_reset, int spike_dtype, spk_stream_t stream);
/* The other eval forms of the reference neuron, SJ/activation_based/neuron.py:827-900 (dispatch :971-1011): soft reset
 * (v_reset = None there; `v_reset` is ignored), decay_input = False, and -- v_seq_out non-NULL -- the `..._with_v_seq` variants
 * (membrane potential after every step, fp32 [T, N]).  fp32 spikes; v [N] updated in place. */
int spk_lif_fwd_ex(const float* x_seq, float* v_inout, float* spike_out_f32, float* v_seq_out_or_null, int T, long long N,
                   float tau, float v_threshold, float v_reset, int soft_reset, int decay_input, spk_stream_t stream);


/* The table behind the time-invariant-input layers (spk_conv_fused_fwd with SPK_IN_TINV and no carried state): the default
 * neuron (tau 2, v_th 1, v_reset 0: SJ/activation_based/neuron.py:799-811 with the models' constructor arguments,
 * R/snn_model/vae_model.py:112) driven by a CONSTANT input from v = 0 fires with period p(x); thresholds16[k-1] is the
 * smallest fp32 input whose first spike comes at step k or earlier, patterns18[p] the sixteen spike bits of period p
 * (p = 17: none).  Host-side copy-out, no GPU needed: the CPU tests check it against the fp32 recurrence on every float. */
int spk_lif_const_input_table(float* thresholds16, unsigned* patterns18);

/* ---- stateless step-mode layers ---------------------------------------------------------------------------- */

/* Eval BatchNorm as PyTorch evaluates it (pinned by fixture F7): a = (1/sqrt(var+eps))*gamma, b = fma(-mean,a,beta). */
int spk_bn_prepare(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                   float eps, float* a_out, float* b_out, int C, spk_stream_t stream);
/* y = fma(x, a[c], b[c]) over x [M,C,HW]: layer.BatchNorm2d 'm' mode, SJ/activation_based/layer.py:458-465. */
int spk_bn_eval_fwd(const float* x, const float* a, const float* b, float* y, long long M, int C, int HW,
                    spk_stream_t stream);
/* layer.Conv2d 'm' mode body (T folded into M), SJ/activation_based/layer.py:164-173. w [Cout,Cin,k,k]. */
int spk_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, long long M, int Cin, int H, int W,
                   int Cout, int k, int stride, int pad, spk_stream_t stream);
/* layer.ConvTranspose2d 'm' mode body, SJ/activation_based/layer.py:316-325. w [Cin,Cout,k,k]. */
int spk_conv_transpose2d_fwd(const float* x, const float* w, const float* bias, float* y, long long M, int Cin, int H,
                             int W, int Cout, int k, int stride, int pad, int out_pad, spk_stream_t stream);
/* MembraneOutputLayer.forward, R/snn_model/snn_layers.py:36-41: out[N] = sum_t x_seq[t][N]*coef[t]. */
int spk_memout_fwd(const float* x_seq, const float* coef, float* out, int T, long long N, spk_stream_t stream);

/* ---- surrogate-gradient LIF (training path) ---------------------------------------------- */
/* LIFNode training forward (hard reset, decay_input): SJ/activation_based/neuron.py:739-749,133-135; the native pair it
 * mirrors: LIFNodeFPTTKernel / LIFNodeBPTTKernel, SJ/activation_based/auto_cuda/neuron_kernel.py:102-225,479-540.
 * h_seq [T,N] (membrane potential before reset, kept for the backward), spike_seq [T,N] fp32, v_out [N] final state. */
int spk_lif_train_fwd(const float* x_seq, const float* v_init, float* h_seq, float* spike_seq, float* v_out, int T,
                      long long N, float tau, float v_threshold, float v_reset, spk_stream_t stream);
/* BPTT with the ATan surrogate g'(x) = alpha/2 / (1 + (pi/2 alpha x)^2) (SJ/activation_based/surrogate.py:664-678).
 * grad_v_last [N] (gradient of the final state) and grad_v_init [N] may be NULL.  detach_reset as in the reference. */
int spk_lif_train_bwd(const float* grad_spike_seq, const float* grad_v_last, const float* h_seq, float* grad_x_seq,
                      float* grad_v_init, int T, long long N, float tau, float v_threshold, float v_reset, float alpha,
                      int detach_reset, spk_stream_t stream);

/* Training-mode BatchNorm2d ('m' mode, batch statistics: SJ/activation_based/layer.py:458-465 -> F.batch_norm(training=True))
 * fused with the surrogate-gradient LIF above -- one denoiser block tail of DummyModel.forward in train() mode
 * (R/snn_model/vq_diffusion.py:163-183,199-203).  CHANNELS-LAST memory: y, spike_seq, grad_* are [T][B][HW][C] fp32
 * (what the library's NHWC convolutions read and write), v_init / v_out / grad_v_* [B][HW][C]; gamma/beta/running_* /
 * save_* [C]  (v_init NULL = reset state, v_out / running_* / grad_v_* may be NULL).
 * running_mean / running_var are updated in place with `momentum` (unbiased variance), save_mean / save_invstd receive
 * the batch statistics the backward needs.  ws: caller-allocated scratch of spk_bn_lif_train_ws_bytes(B, C, HW) bytes.
 * The backward recomputes the membrane potentials from y (only y and the two statistics vectors are kept). */
long long spk_bn_lif_train_ws_bytes(int B, int C, int HW);
int spk_bn_lif_train_fwd(const float* y, const float* gamma, const float* beta, float* running_mean, float* running_var,
                         float momentum, float eps, const float* v_init, float* spike_seq, float* v_out, float* save_mean,
                         float* save_invstd, void* ws, long long ws_bytes, int T, int B, int C, int HW, float tau,
                         float v_threshold, float v_reset, spk_stream_t stream);
int spk_bn_lif_train_bwd(const float* grad_spike_seq, const float* grad_v_last, const float* y, const float* gamma,
                         const float* beta, const float* save_mean, const float* save_invstd, const float* v_init,
                         float* grad_y, float* grad_gamma, float* grad_beta, float* grad_v_init, void* ws,
                         long long ws_bytes, int T, int B, int C, int HW, float tau, float v_threshold, float v_reset,
                         float alpha, int detach_reset, spk_stream_t stream);
/* The same backward with the layout of grad_spike_seq spelled out (in floats): grad_step_stride = 0 when every step receives
 * the SAME gradient -- the spikes in front of the denoiser's last layer do: its time mean hands g / T to every step
 * (R/snn_model/vq_diffusion.py:205-206) -- and grad_row_pitch >= C for a channel slice of a wider channels-last tensor (the x5 / x1
 * halves of cat(x5, x1), :205).  The gradient is read where autograd left it instead of being expanded and copied first.
 * spk_bn_lif_train_bwd == grad_step_stride B*HW*C, grad_row_pitch C. */
int spk_bn_lif_train_bwd_strided(const float* grad_spike_seq, long long grad_step_stride, long long grad_row_pitch,
                                 const float* grad_v_last, const float* y, const float* gamma, const float* beta,
                                 const float* save_mean, const float* save_invstd, const float* v_init, float* grad_y,
                                 float* grad_gamma, float* grad_beta, float* grad_v_init, void* ws, long long ws_bytes, int T,
                                 int B, int C, int HW, float tau, float v_threshold, float v_reset, float alpha,
                                 int detach_reset, spk_stream_t stream);
/* The same forward, also leaving the spikes as "C4" records [B][C/64][HW][T][32 bytes = 64 channels x e2m1] (spikes_c4_out, or
 * NULL) -- the input format of spk_den_conv3x3_fp6_raw, i.e. of the NEXT block's convolution in the training forward; the apply
 * launch writes them next to the fp32 spikes.  Needs C % 64 == 0 and 16-byte aligned tensors (SPK_ERR_UNSUPPORTED otherwise,
 * nothing launched). */
int spk_bn_lif_train_fwd_c4(const float* y, const float* gamma, const float* beta, float* running_mean, float* running_var,
                            float momentum, float eps, const float* v_init, float* spike_seq, float* v_out, float* save_mean,
                            float* save_invstd, uint8_t* spikes_c4_out, void* ws, long long ws_bytes, int T, int B, int C,
                            int HW, float tau, float v_threshold, float v_reset, spk_stream_t stream);
/* Training forward of a denoiser convolution on spike input (layer.Conv2d 'm' mode in train(), SJ/activation_based/layer.py:164-173,
 * for conv2..conv5 of DummyModel, R/snn_model/vq_diffusion.py:166-184): the exact fp6 x fp4 MFMA convolution of
 * spk_den_conv3x3_mfma_fp6 with the pre-activations (conv + bias, correctly rounded fp32 of the exact dot product) written
 * out instead of the fused BN + LIF -- batch-statistics BN needs all of them first.  in_c4 as for the inference kernel;
 * pre_nhwc fp32 channels-last [T][B][H*W][Cout].  spk_spikes_nhwc_to_fp4 (spike layouts, below) packs the output of
 * spk_bn_lif_train_fwd into the C4 input layout. */
int spk_den_conv3x3_fp6_raw(const uint8_t* in_c4, int nch, const uint8_t* wq, const double* scale, const double* bias_d,
                            float* pre_nhwc, int T, int B, int H, int W, int Cout, spk_stream_t stream);

/* Masked cross-entropy of AbsorbingDiffusion._train_loss (R/snn_model/vq_diffusion.py:85-88: F.cross_entropy with
 * ignore_index=-1, reduction='none') and its gradient in one pass.  logits / dlogits [B,K,HW] fp32; target [B,HW] fp32
 * token ids (-1 = ignored, as x_0_ignore); coef [B] per-sample gradient factor; ce_out [B,HW] (0 where ignored).
 * dlogits (and coef) may be NULL for the forward alone. */
int spk_masked_ce(const float* logits, const float* target, const float* coef, float* ce_out, float* dlogits, int B, int K,
                  int HW, spk_stream_t stream);

/* PSP filter of the VQ-VAE training losses (R/snn_model/snn_layers.py:6-26; used at R/snn_model/vae_model.py:81-82):
 * out[t] = syn_t, syn_t = syn_{t-1} + (in[t] - syn_{t-1}) / tau_s, syn_{-1} = 0, over a dense [T][N] fp32 tensor.
 * backward != 0 runs the adjoint instead (in = dL/dsyn, out = dL/dx). */
int spk_psp(const float* in, float* out, int T, long long N, float tau_s, int backward, spk_stream_t stream);

/* ---- spike layouts (csrc/layouts.hip) ------------------------------------------------------------------------ */
/* The interface tensor is fp32 [T,B,C,HW] (1.0 = spike).  Between layers a spike tensor is stored in one of four record forms, a
 * record being the channels of one (position, step) that lie together in memory:
 *   PTC   u8           [B][HW][T][C]               one byte per channel (0 / 1), all C channels in one record
 *   CPTC  u8           [B][C/chunk][HW][T][chunk]  the same bytes in records of `chunk` channels (32: the K chunk of the int8 MFMA
 *                                                  kernel, one contiguous slab per image and chunk)
 *   C4    e2m1 nibbles [B][C/64][HW][T][32 B]      64 channels per record
 *   S32   e2m1 nibbles [B][C/32][HW][T][16 B]      32 channels per record
 * In a nibble record channel k lies in nibble k (even channel = low nibble); a spike is 0x2, the e2m1 code of 1.0, silence 0x0.
 * C4 is read by spk_den_conv3x3_mfma_fp6 / spk_den_conv3x3_fp6_raw, S32 by spk_den_conv3x3_mfma_fp6v2 and spk_vae_fp6_fwd; the fused
 * kernels write all four themselves (chunk_out of spk_conv_fused_fwd: 0, a chunk, SPK_CHUNK_C4, SPK_CHUNK_S32).  The entry points
 * below convert at module boundaries and in tests.
 * fp32 <-> PTC (chunk = C) / CPTC (chunk < C); SPK_ERR_ARG unless C % chunk == 0: */
int spk_spikes_to_ptc(const float* spikes_tbchw, uint8_t* out_bhwtc, int T, int B, int C, int HW, int chunk,
                      spk_stream_t stream);
int spk_ptc_to_spikes(const uint8_t* in_bhwtc, float* spikes_tbchw, int T, int B, int C, int HW, int chunk,
                      spk_stream_t stream);
/* fp32 <-> C4 (C % 64 == 0) and S32 (C % 32 == 0; SPK_ERR_UNSUPPORTED otherwise): */
int spk_spikes_to_fp4(const float* spikes, uint8_t* out_c4, int T, int B, int C, int HW, spk_stream_t stream);
int spk_fp4_to_spikes(const uint8_t* in_c4, float* spikes, int T, int B, int C, int HW, spk_stream_t stream);
int spk_spikes_to_s32(const float* spikes, uint8_t* out_s32, int T, int B, int C, int HW, spk_stream_t stream);
int spk_s32_to_spikes(const uint8_t* in_s32, float* spikes, int T, int B, int C, int HW, spk_stream_t stream);
/* channels-last fp32 spikes [T][B][HW][C] (the output of spk_bn_lif_train_fwd) -> C4 (C % 64 == 0), the training forward's
 * conversion; _counts: with the per-neuron spike counts over T as a by-product, counts_nhwc fp32 [B][HW][C] (channels-last) -- what
 * the last layer's weight gradient is convolved with in the training step (its time mean hands every step the same gradient). */
int spk_spikes_nhwc_to_fp4(const float* spikes_nhwc, uint8_t* out_c4, int T, int B, int C, int HW, spk_stream_t stream);
int spk_spikes_nhwc_to_fp4_counts(const float* spikes_nhwc, uint8_t* out_c4, float* counts_nhwc, int T, int B, int C, int HW,
                                  spk_stream_t stream);
/* u8 PTC -> S32 [B][ceil(C/32)][HW][16][16 B], zero nibbles in the channels beyond C (any C; T = 16 only: SPK_ERR_UNSUPPORTED
 * otherwise): what the decoder's spike generator hands spk_vae_fp6_fwd. */
int spk_ptc_to_s32(const uint8_t* in_ptc, uint8_t* out_s32, int T, int B, int HW, int C, spk_stream_t stream);

/* ---- fused (Conv|ConvT) [+BN+LIF] --------------------------------------------------------------------------- */
int spk_conv_out_size(int in, int k, int stride, int pad, int transposed, int out_pad);
/* [Cout,Cin,k,k] (Conv2d) or [Cin,Cout,k,k] (ConvTranspose2d) -> packed [k*k][Cin][Cout]. */
int spk_pack_conv_weight(const float* w, float* packed, int Cout, int Cin, int k, int transposed, spk_stream_t stream);
/* One Conv|ConvT block of Encoder / poisson / Decoder / DummyModel with its BN + LIF (or read-out) fused:
 * R/snn_model/vae_model.py:34-38,109-124,139-155; R/snn_model/vq_diffusion.py:161-187,200-206.
 *   in0: per in_kind -- SPK_IN_TINV fp32 [B,C0,H,W] (same frame every step: R/main.py:309, vae_model.py:54-56,
 *        vq_diffusion.py:198), SPK_IN_PTC u8 [B,H,W,T,C0], SPK_IN_SEQ fp32 [T,B,C0,H,W];
 *   in1: optional second PTC source [B,H,W,T,C1] (channel concat of conv6, vq_diffusion.py:205).
 *   mode LIF:    bn_a/bn_b required; v_inout [B,Cout,Ho,Wo] or NULL (fresh state, not written back);
 *                out_ptc u8 PTC and/or out_f32 fp32 TBCHW spikes; out_pre optional BN output.
 *   mode RAW:    out_f32 TBCHW conv output.    mode MEMOUT: coef [T]; out_f32 [B,Cout,Ho,Wo] (tanh if apply_tanh),
 *                out_u8 = uint8(clip(p+0.5,0,1)*255) (R/main.py:401).   mode MEAN: out_f32 = sum_t x[t] / T.
 *   chunk0 / chunk1 / chunk_out: channel chunking of in0 / in1 / out_ptc (0: plain PTC); chunk_out = SPK_CHUNK_C4:
 *                out_ptc is written as nibble-packed fp4 "C4" (see spk_den_conv3x3_mfma_fp6; Cout % 64 == 0);
 *                SPK_CHUNK_S32: as "S32" (see spk_den_conv3x3_mfma_fp6v2; Cout % 32 == 0).
 *   out_counts (mode LIF, optional): per-neuron spike counts over T, u8 [B,Cout/32,Ho*Wo,32].
 *   n_dyn_or_null: optional device-side image count (0 <= *n_dyn <= B: the caller's duty; see spk_select_active): only images
 *                [0, *n_dyn) are computed; buffers stay sized by B.  For an image at or past the count NOTHING is written: no byte
 *                of any output (spikes, fp32 values, BN outputs, spike counts) and not its v_inout, which keeps the value it
 *                came with; a count of 0 writes nothing at all.  The count is read on the device when the kernel runs, so a
 *                captured graph follows the value its tensor holds at each replay.  The same holds for every n_dyn_or_null /
 *                n_dyn below (tests/test_gpu_image_count.py). */
int spk_conv_fused_fwd(const void* in0, const uint8_t* in1, int C0, int C1, int in_kind, const float* w_packed,
                       const float* bias, const float* bn_a, const float* bn_b, float* v_inout, uint8_t* out_ptc,
                       float* out_f32, float* out_pre, uint8_t* out_u8, const float* coef, int apply_tanh, int mode,
                       int T, int B, int H, int W, int Cout, int k, int stride, int pad, int transposed, int out_pad,
                       int chunk0, int chunk1, int chunk_out, uint8_t* out_counts, const int* n_dyn_or_null,
                       spk_stream_t stream);

/* ---- denoiser convolutions on the matrix cores ------------------------------------------------------------------ */
/* Shape predicates.  Every matrix-core kernel family answers which layer shapes it takes through one host function -- 1 / 0
 * (spk_vae_fp6_kind: the output form, or -1) from integers alone, no device needed -- and its entry point refuses exactly the shapes
 * the predicate refuses (SPK_ERR_UNSUPPORTED, nothing launched).  What an entry point refuses beyond that depends on the call or the
 * device, not on the shape: the batch size (grid and id widths), the device's LDS grant and CU count, the list arguments.
 * The three denoiser forms (k, stride, pad: the layer's geometry, only 3 / 1 / 1 is taken; T: time steps; H x W: the latent): */
int spk_den_conv3x3_mfma_supported(int Cout, int Cin, int k, int stride, int pad, int T, int H, int W);
int spk_den_conv3x3_mfma_fp6_supported(int Cout, int Cin, int k, int stride, int pad, int T, int H, int W);
int spk_den_conv3x3_mfma_fp6v2_supported(int Cout, int Cin, int k, int stride, int pad, int T, int H, int W);
/* Bytes of the packed int8 digit-plane weights of one 3x3 layer ([Cout/16][Cin/32][9][2][32][32]); -1 if unsupported. */
long long spk_den_packed_weight_bytes(int Cout, int Cin);
/* fp32 conv weight [Cout,Cin,3,3] (+bias) -> four balanced base-256 int8 digit planes + per-channel 2^-s scale and
 * fp64 bias.  One-time weight preparation for spk_den_conv3x3_mfma. */
int spk_den_pack_weight_i8(const float* w, const float* bias, int8_t* wq, double* scale, double* bias_d, int Cout,
                           int Cin, spk_stream_t stream);
/* 3x3 / stride 1 / pad 1 convolution over binary spikes (CPTC u8, T = 16) + BN + LIF (mode SPK_MODE_LIF -> out_cptc)
 * or + time mean (mode SPK_MODE_MEAN -> out_f32 [B,Cout,h,w]): DummyModel conv2..conv6,
 * R/snn_model/vq_diffusion.py:166-187,201-206.  in1 (nch1 chunks) is concatenated after in0 along channels.
 * v_inout [B,Cout,h,w] or NULL (fresh LIF state, nothing written back).  out_counts (LIF mode, optional): per-neuron
 * spike counts over T as u8 [B,Cout/32,h*w,32], the input format of spk_den_conv3x3_counts_mfma.
 * n_dyn_or_null as in spk_conv_fused_fwd.  SPK_ERR_UNSUPPORTED unless spk_den_conv3x3_mfma_supported (Cin = 32 * (nch0 + nch1)). */
int spk_den_conv3x3_mfma(const uint8_t* in0_cptc, int nch0, const uint8_t* in1_cptc, int nch1, const int8_t* wq,
                         const double* scale, const double* bias_d, const float* bn_a, const float* bn_b,
                         float* v_inout, uint8_t* out_cptc, uint8_t* out_counts, float* out_f32, int mode, int T, int B,
                         int H, int W, int Cout, const int* n_dyn_or_null, spk_stream_t stream);
/* conv6 + time mean of DummyModel (R/snn_model/vq_diffusion.py:185-187,205-206) in its time-collapsed form:
 * (sum_t conv(s_t)) / T = (conv_linear(sum_t s_t) + T*bias) / T.  cnt0 / cnt1: spike counts u8 [B,nch,h*w,32]
 * (channel concat: cnt1 after cnt0); same packed weights as spk_den_conv3x3_mfma; out_f32 [B,Cout,h,w].
 * n_dyn_or_null as in spk_conv_fused_fwd. */
int spk_den_conv3x3_counts_mfma(const uint8_t* cnt0, int nch0, const uint8_t* cnt1, int nch1, const int8_t* wq,
                                const double* scale, const double* bias_d, float* out_f32, int T, int B, int H, int W,
                                int Cout, const int* n_dyn_or_null, spk_stream_t stream);

/* ---- denoiser convolutions on the block-scaled fp6/fp4 MFMA (CDNA4 v_mfma_scale_f32_32x32x64_f8f6f4) -------------- */
/* Same operator and numerics contract as spk_den_conv3x3_mfma (LIF mode: DummyModel conv2..conv5,
 * R/snn_model/vq_diffusion.py:166-184,201-204) at 3/4 of its matrix-core time: weights as six radix-32 fp6 (e2m3)
 * digit planes, spikes as fp4 (e2m1) nibbles.  Spike tensors are "C4": [B][C/64][h*w][16][32 B], channel c of a
 * 64-channel chunk in byte c/2 (low nibble first), nibble = 0x2 for a spike.
 * Bytes of the packed weights of one layer ([Cout/16][Cin/64] slabs of [9][3][64 lanes x 24 B], each padded to 41 KiB);
 * -1 if unsupported. */
long long spk_den_packed_weight_fp6_bytes(int Cout, int Cin);
/* fp32 conv weight [Cout,Cin,3,3] (+bias) -> six balanced radix-32 digit planes as e2m3 codes + per-channel 2^-s
 * scale and fp64 bias. */
int spk_den_pack_weight_fp6(const float* w, const float* bias, uint8_t* wq, double* scale, double* bias_d, int Cout,
                            int Cin, spk_stream_t stream);
/* The same packing of a weight stored in the channels-last memory format, [Cout][3][3][Cin] (how the training path keeps its
 * convolution parameters, R/main.py:226-252 with NHWC library kernels): no layout copy in front of the per-iteration packing. */
int spk_den_pack_weight_fp6_cl(const float* w_channels_last, const float* bias, uint8_t* wq, double* scale, double* bias_d,
                               int Cout, int Cin, spk_stream_t stream);
/* The channels-last packing of n <= 8 layers in ONE launch (a training iteration re-packs every spike-input layer once per
 * optimizer step, R/main.py:243-252).  HOST arrays of n entries (bias may be NULL, or hold NULL entries); per layer the result
 * is spk_den_pack_weight_fp6_cl's byte for byte. */
int spk_den_pack_weight_fp6_cl_multi(const float* const* w_channels_last, const float* const* bias, uint8_t* const* wq,
                                     double* const* scale, double* const* bias_d, const int* Cout, const int* Cin, int n,
                                     spk_stream_t stream);
/* in_c4: nch chunks of 64 channels; out_c4 [B][Cout/64][h*w][16][32]; v_inout / out_counts as in spk_den_conv3x3_mfma.
 * SPK_ERR_UNSUPPORTED unless spk_den_conv3x3_mfma_fp6_supported (Cin = 64 * nch): a latent runs as one item per image and channel
 * group where that fits the kernel's LDS plan, 8x8 as two row bands.
 * n_dyn_or_null as in spk_conv_fused_fwd (the work items are then walked image-major). */
int spk_den_conv3x3_mfma_fp6(const uint8_t* in_c4, int nch, const uint8_t* wq, const double* scale, const double* bias_d,
                             const float* bn_a, const float* bn_b, float* v_inout, uint8_t* out_c4, uint8_t* out_counts,
                             int T, int B, int H, int W, int Cout, const int* n_dyn_or_null, spk_stream_t stream);
/* Second-generation form of spk_den_conv3x3_mfma_fp6 for the sampler (7x7 latents, fresh LIF state in, no state out):
 * the SAME spikes bit for bit -- the four leading digits on the matrix cores with adjacent digits sharing an accumulator through
 * the per-block scales, fp32 recombination, every spike decision certified against a bound on the dropped digits (per counted
 * active input of the row; tiles with a flagged lane are re-examined with the per-step running bound), and the ~1e-4 of neurons
 * that come closer to the threshold recomputed exactly (all six digits, int64 / fp64) by a tail launch; another finishes the 49th
 * position (csrc/den_mfma_fp6v2.hip).  DummyModel conv2..conv5, R/snn_model/vq_diffusion.py:166-184,201-204.
 * Spikes travel as "S32": [B][C/32][H*W][16][16 B] (fp4 nibbles, channel c of a group in byte (c % 32) / 2, low nibble first).
 * spk_den_pack_weight_fp6v2: fp32 [Cout,Cin,3,3] (+bias) -> packed digit tiles (spk_den_packed_weight_fp6v2_bytes), fp64
 * scale / bias [Cout] as for the fp6 kernel, wl1 [Cout] = L1 norm of each channel's quantised weights, and qtab = the
 * quantised weights themselves as int32 [Cout][9][Cin] (read by the exact recomputation).  flag_words: zero-initialised
 * u32 workspace of spk_den_fp6v2_flag_words(B, Cout, H, W) words (counter, ticket, id list, overflow bitmap); it is clean
 * again when the call's launches have run (word 1 keeps the number of neurons the call flagged, for statistics).  One
 * workspace per stream: two calls in flight at once must not share it.
 * flag_cap: how many flagged neurons the id list takes before the rest go to the overflow bitmap, which the tail launch scans and
 * clears (< 0 or > 2^20: the whole list of 2^20 entries -- what every product call passes).  The workspace layout does not depend on
 * it; the parity suite passes 64 and 0 so that the overflow path runs (tests/test_gpu_parity.py::test_flag_overflow_*).
 * form: 0 = automatic (7x7 latents with fewer items -- B x Cout / 32 -- than half the CUs run two half-image items per image on
 * four-wave workgroups: R/main.py's own n_samples = 16 leaves half the chip idle otherwise), 1 = whole-image items always (the
 * reference form for the bit-equality test of the split).  Same spikes bit for bit either way.
 * n_dyn_or_null as in spk_conv_fused_fwd, in every launch of the call: an image at or past the count gets no record, no spike
 * count and no flag entry (neither id nor bitmap bit), its last position included; with a count of 0 the workspace still comes back
 * clean and word 1 is 0.
 * SPK_ERR_UNSUPPORTED unless spk_den_conv3x3_mfma_fp6v2_supported (Cin = 32 * nch). */
long long spk_den_packed_weight_fp6v2_bytes(int Cout, int Cin);
int spk_den_pack_weight_fp6v2(const float* w, const float* bias, uint8_t* wq, double* scale, double* bias_d, float* wl1,
                              int* qtab, int Cout, int Cin, spk_stream_t stream);
long long spk_den_fp6v2_flag_words(int B, int Cout, int H, int W);
int spk_den_conv3x3_mfma_fp6v2(const uint8_t* in_s32, int nch, const uint8_t* wq, const double* scale, const double* bias_d,
                               const float* wl1, const int* qtab, const float* bn_a, const float* bn_b, uint8_t* out_s32,
                               uint8_t* out_counts, unsigned* flag_words, int T, int B, int H, int W, int Cout,
                               const int* n_dyn_or_null, int flag_cap, int form, spk_stream_t stream);
/* Measurement aid: re-run ONE tail part of the last spk_den_conv3x3_mfma_fp6v2 call on the same arguments and workspace --
 * part 2: the exact recomputation of the neurons that call flagged (flag_words[1] holds their number, the id list is intact;
 * recomputing them again writes the same spikes), part 4: the last position of every image (7x7) below the count
 * (n_dyn_or_null as in spk_den_conv3x3_mfma_fp6v2: the last position of an image at or past it is left as it was).  bench.py times
 * these to report `repair_ms` / `last_position_ms` per layer; flag_words[1] / (B * Cout * H * W) is the flagged fraction. */
int spk_den_conv3x3_mfma_fp6v2_part(const uint8_t* in_s32, int nch, const uint8_t* wq, const double* scale,
                                    const double* bias_d, const float* wl1, const int* qtab, const float* bn_a,
                                    const float* bn_b, uint8_t* out_s32, uint8_t* out_counts_or_null, unsigned* flag_words,
                                    int T, int B, int H, int W, int Cout, const int* n_dyn_or_null, int part,
                                    int flag_cap, spk_stream_t stream);
/* The same layer restricted to the positions the sampler will read (7x7 only): need = the buffer written by
 * spk_select_needed(..., R = need_radii) for the same B; radius (1..need_radii) selects the lists this layer computes --
 * 1 for the layer whose output the logits convolution reads, 2 for the one below it, ...  Listed positions (and the 49th)
 * receive exactly the spikes of the full call; the other positions of out_s32 / out_counts are left as they were.
 * n_dyn (required) as n_dyn_or_null of spk_den_conv3x3_mfma_fp6v2.  The lists carry the slot count of the spk_select_needed call
 * that wrote them; *n_dyn may be lower by the time of this call, and then it decides: a listed slot at or past it is written
 * nowhere -- no record, count or flag entry. */
int spk_den_conv3x3_mfma_fp6v2_listed(const uint8_t* in_s32, int nch, const uint8_t* wq, const double* scale,
                                      const double* bias_d, const float* wl1, const int* qtab, const float* bn_a,
                                      const float* bn_b, uint8_t* out_s32, uint8_t* out_counts, unsigned* flag_words, int T,
                                      int B, int H, int W, int Cout, const int* n_dyn, const uint8_t* need, int need_radii,
                                      int radius, int flag_cap, spk_stream_t stream);

/* ---- spiking VQ-VAE layers on the matrix cores ------------------------------------------------------------------- */
/* Bytes of the packed int8 digit planes of a k x k (transposed) conv: [ceil(Cout/16)][ceil(Cin/32)][k*k][2][32][32]. */
long long spk_conv_packed_weight_i8_bytes(int Cout, int Cin, int k);
/* Conv2d [Cout,Cin,k,k] or ConvTranspose2d [Cin,Cout,k,k] weight (+bias) -> int8 digit planes; scale / bias_d have
 * ceil(Cout/16)*16 entries (padding channels are zero). */
int spk_pack_conv_weight_i8(const float* w, const float* bias, int8_t* wq, double* scale, double* bias_d, int Cout,
                            int Cin, int k, int transposed, spk_stream_t stream);
/* (Conv2d | ConvTranspose2d) over binary spikes (plain PTC u8 [B,H*W,16,Cin]; spk_conv_mfma_fused_supported) with exact int8
 * MFMA accumulation, fused with BN + LIF (mode SPK_MODE_LIF -> out_ptc [B,Ho*Wo,16,Cout]) or with the membrane
 * read-out (mode SPK_MODE_MEMOUT: coef[16] -> out_f32 [B,Cout,Ho,Wo] (+tanh), out_u8): Encoder conv2/conv3, Decoder
 * convT1/convT2/convT3 of R/snn_model/vae_model.py:115-124,139-155,186.
 * SPK_MODE_LIF with coef AND out_f32 given: out_f32 [B,Ho*Wo,Cout] also receives sum_t coef[t] * spike[t] (the input of
 * spk_readout_collapsed_fwd); out_ptc may then be NULL (the spike frames are not stored). */
int spk_conv_mfma_fused_supported(int Cin, int Cout, int T, int mode);
int spk_conv_mfma_fused_fwd(const uint8_t* in_ptc, const int8_t* wq, const double* scale, const double* bias_d,
                            const float* bn_a, const float* bn_b, float* v_inout, uint8_t* out_ptc, const float* coef,
                            float* out_f32, uint8_t* out_u8, int apply_tanh, int mode, int T, int B, int H, int W, int Cin,
                            int Cout, int k, int stride, int pad, int transposed, int out_pad, spk_stream_t stream);
/* The decoder's linear last layer + membrane read-out (R/snn_model/vae_model.py:152-154,186, R/snn_model/snn_layers.py:36-41)
 * on time-collapsed spikes:  sum_t coef[t] * (W * s_t + bias) = W * (sum_t coef[t] * s_t) + bias * sum_t coef[t].
 * x_bpc fp32 [B,H*W,Cin] = sum_t coef[t] * s_t (see spk_conv_mfma_fused_fwd); w = the layer's fp32 weight, Conv2d
 * [Cout,Cin,k,k] or ConvTranspose2d [Cin,Cout,k,k] (transposed = 1); coef_sum = sum_t coef[t]; stride 1, pad == k / 2.
 * out_f32 [B,Cout,H,W] (tanh if apply_tanh), out_u8 = uint8(clip(p + 0.5, 0, 1) * 255) (R/main.py:401).  fp32 arithmetic:
 * equal to the frame-by-frame sum up to fp32 round-off.  spk_readout_collapsed_supported: whether (Cin, Cout, k) fits the kernel at
 * image width W; W <= 0 asks for every width up to 64. */
int spk_readout_collapsed_supported(int Cin, int Cout, int k, int W);
int spk_readout_collapsed_fwd(const float* x_bpc, const float* w, const float* bias_or_null, float coef_sum, float* out_f32,
                              uint8_t* out_u8, int apply_tanh, int B, int H, int W, int Cin, int Cout, int k, int pad,
                              int transposed, spk_stream_t stream);
/* spk_conv_mfma_fused_fwd in SPK_MODE_LIF writing nibble-packed "S32" spikes [B][Cout/32][Ho*Wo][16][16 B] (Cout % 32 == 0):
 * the input layout of the fp6 kernels. */
int spk_conv_mfma_fused_lif_s32(const uint8_t* in_ptc, const int8_t* wq, const double* scale, const double* bias_d,
                                const float* bn_a, const float* bn_b, float* v_inout, uint8_t* out_s32, int T, int B, int H,
                                int W, int Cin, int Cout, int k, int stride, int pad, int transposed, int out_pad,
                                spk_stream_t stream);
/* The spike-input 3x3 stride-2 layers of the spiking VQ-VAE from the reset state on the block-scaled fp6 x fp4 MFMA
 * (csrc/vae_fp6.hip): the same spikes as spk_conv_mfma_fused_fwd -- five digit planes on the matrix cores, certified decisions,
 * exact recomputation of the flagged neurons.  spk_vae_fp6_kind answers which instance exists for a layer -- its out_kind, or -1:
 *   SPK_VAE_OUT_COLLAPSED: Decoder convT2 (R/snn_model/vae_model.py:146-150) -> out = fp32 [B][4*H*W][Cout] = sum_t coef[t] * spike[t], the input
 *       of spk_readout_collapsed_fwd (the spike frames are not stored);
 *   SPK_VAE_OUT_S32: Decoder convT1 (:139-144) -> out = S32 spikes [B][Cout/32][4*H*W][16][16 B];
 *   SPK_VAE_OUT_PTC: Encoder conv2 (:115-118) -> out = u8 PTC [B][H*W/4][16][Cout].
 * spk_vae_fp6_fwd takes the out_kind that spk_vae_fp6_kind names for its layer (k 3, stride 2, pad 1; out_pad 1 if transposed).
 * in_s32: S32 spikes [B][ceil(Cin/32)][H*W][16][16 B] with zero nibbles in the channels beyond Cin (spk_ptc_to_s32 converts u8
 * PTC spikes).  spk_vae_fp6_pack: fp32 weight (Conv2d [Cout][Cin][3][3] / ConvTranspose2d [Cin][Cout][3][3]) (+bias) -> digit
 * tiles (spk_vae_fp6_packed_bytes), fp64 scale / bias [Cout], qtab int32 [Cout][9][Cin].  flag_words: zero-initialised u32
 * workspace of spk_vae_fp6_flag_words(B, Cout, Ho, Wo) words, clean again after the call; flag_cap as for
 * spk_den_conv3x3_mfma_fp6v2 (< 0: the whole id list). */
#define SPK_VAE_OUT_COLLAPSED 0
#define SPK_VAE_OUT_S32 1
#define SPK_VAE_OUT_PTC 2
int spk_vae_fp6_kind(int Cin, int Cout, int k, int stride, int pad, int out_pad, int transposed, int T, int H, int W);
long long spk_vae_fp6_packed_bytes(int Cout, int Cin);
int spk_vae_fp6_pack(const float* w, const float* bias, uint8_t* wq, double* scale, double* bias_d, int* qtab, int Cout, int Cin,
                     int transposed, spk_stream_t stream);
long long spk_vae_fp6_flag_words(int B, int Cout, int Ho, int Wo);
/* The decoder's front end by token (R/main.py:388-392, R/snn_model/vae_model.py:54-56,66-71: embedding look-up, repeat(T), the 'poisson'
 * spike generator = 1x1 Conv2d + BN + LIF from the reset state): the generator's input at a position is one of the K codebook rows, so
 * its spike train is one of K patterns per output channel.  One call = a K-row pattern table (the arithmetic of spk_conv_fused_fwd's
 * time-invariant form: fp64 dot product from the bias, BN fma, sixteen LIF steps; an out-of-range token embeds as NaN: no spikes) and
 * the S32 spikes [n_positions][16][16 B] of the positions' tokens -- the input layout of spk_vae_fp6_fwd (Cout 16 or 32, T == 16).
 * w_packed: [1][D][Cout] (spk_pack_conv_weight); table_ws: spk_spikegen_table_bytes(K, Cout) bytes, written when build_table != 0 and
 * only read otherwise (the caller keeps it while codebook, weights and BN terms are unchanged). */
long long spk_spikegen_table_bytes(int K, int Cout);
int spk_spikegen_tokens_s32(const long long* tokens, const float* codebook, const float* w_packed, const float* bias, const float* bn_a,
                            const float* bn_b, unsigned short* table_ws, int build_table, uint8_t* out_s32, int T, long long n_positions,
                            int K, int D, int Cout, spk_stream_t stream);
int spk_vae_fp6_fwd(const uint8_t* in_s32, const uint8_t* wq, const double* scale, const double* bias_d, const int* qtab,
                    const float* bn_a, const float* bn_b, const float* coef_or_null, void* out, int out_kind, unsigned* flag_words,
                    int T, int B, int H, int W, int Cin, int Cout, int transposed, int flag_cap, spk_stream_t stream);

/* ---- vector quantizer ----------------------------------------------------------------------------------------- */
/* VectorQuantizer.forward eval up to the codebook gather, R/snn_model/vae_model.py:40-52,87-99.
 * z_ptc u8 [B,h,w,T,D]; coef [T]; alpha [1] (device); codebook [K,D]; idx_out int64 [B*HW];
 * zq_out_bdhw fp32 [B,D,h,w] or NULL; xm_out fp32 [B*HW,D] or NULL (the read-out, for tests). */
int spk_vq_readout_argmin(const uint8_t* z_ptc, const float* coef, const float* alpha, const float* codebook,
                          long long* idx_out, float* zq_out_bdhw, float* xm_out, int T, int B, int D, int HW, int K,
                          spk_stream_t stream);
/* VectorQuantizer.get_code_indices on explicit rows flat_x [N,D], R/snn_model/vae_model.py:87-95. */
int spk_vq_argmin(const float* flat_x, const float* codebook, long long* idx_out, long long N, int D, int K,
                  spk_stream_t stream);
/* VectorQuantizer.quantize (nn.Embedding), R/snn_model/vae_model.py:97-99; nchw=1 also applies the
 * permute(0,3,1,2) of R/main.py:391 and writes [B,D,h,w].  Out-of-range tokens give NaN rows. */
int spk_embedding_fwd(const long long* tokens, const float* codebook, float* out, long long N, int D, int K, int HW,
                      int nchw, spk_stream_t stream);

/* Training branch of VectorQuantizer.forward, R/snn_model/vae_model.py:61-85 (through autograd in the reference: ~40 element-wise,
 * reduce and embedding-backward launches), csrc/vq_train.hip.  Rows are the NHWC positions (N = B * HW).
 * spk_vq_train_readout: x_seq fp32 [T,B,D,HW] -> xm [N,D] = (1 - alpha) * sum_t x[t] * coef[t] + alpha * sum_t x[t] / T and
 *   dxa [N,D] = d xm / d alpha.  (The code search on xm is spk_vq_argmin.)
 * spk_vq_train_quant: out_bdhw fp32 [B,D,HW] = xm + (E[idx] - xm) (the straight-through value) and loss_out[0] =
 *   mse(q, xm) + beta * mse(xm, q).  ws: spk_vq_train_ws_bytes() bytes, zero-initialised once, clean again after every call.
 * spk_vq_train_bwd: gout_bdhw = dL/d out, gloss_or_null [1] = dL/d loss (device) -> gx_seq [T,B,D,HW], galpha_out [1],
 *   gcodebook_out [K,D] (one workgroup per code, fixed summation order).  SPK_ERR_UNSUPPORTED for D > SPK_VQ_TRAIN_MAX_D. */
#define SPK_VQ_TRAIN_MAX_D 64
long long spk_vq_train_ws_bytes(void);
int spk_vq_train_readout(const float* x_seq, const float* coef, const float* alpha, float* xm_out, float* dxa_out, int T, int B,
                         int D, int HW, spk_stream_t stream);
int spk_vq_train_quant(const float* xm, const long long* idx, const float* codebook, float* out_bdhw, float* loss_out, float beta,
                       void* ws, long long N, int D, int HW, spk_stream_t stream);
/* The PSP losses of the same branch, R/snn_model/vae_model.py:79-84: loss_out[0] = mean((psp(q) - psp(x))^2) * (1 + beta) over dense
 * [T][N] fp32 tensors (both filters in registers, nothing stored), and its backward: gq_seq = dL/dq, gx_seq = dL/dx (the commitment
 * factor beta on x) from gloss [1] (device) through the adjoint filters -- one launch each.  ws as for spk_vq_train_quant.
 * spk_psp_loss_bwd: SPK_ERR_UNSUPPORTED for T > 16. */
int spk_psp_loss_fwd(const float* q_seq, const float* x_seq, float* loss_out, float beta, float tau_s, void* ws, int T, long long N,
                     spk_stream_t stream);
int spk_psp_loss_bwd(const float* q_seq, const float* x_seq, const float* gloss, float* gq_seq, float* gx_seq, float beta,
                     float tau_s, int T, long long N, spk_stream_t stream);
/* Reconstruction loss of SNN_VQVAE.forward in training, R/snn_model/vae_model.py:189-196: xr_out [N] = tanh(sum_t y[t] * coef[t]),
 * loss_out[0] = mean((xr - image)^2) over N = B*C*H*W elements (one launch), and gy_seq [T][N] = dL/dy from gloss [1] (one launch). */
int spk_recon_loss_fwd(const float* y_seq, const float* coef, const float* image, float* xr_out, float* loss_out, void* ws, int T,
                       long long N, spk_stream_t stream);
int spk_recon_loss_bwd(const float* xr, const float* image, const float* coef, const float* gloss, float* gy_seq, int T, long long N,
                       spk_stream_t stream);
int spk_vq_train_bwd(const float* gout_bdhw, const float* gloss_or_null, const float* xm, const long long* idx,
                     const float* codebook, const float* dxa, const float* coef, const float* alpha, float beta, float* gx_seq,
                     float* galpha_out, float* gcodebook_out, void* ws, int T, long long N, int D, int HW, int K,
                     spk_stream_t stream);

/* Weight gradient of a 3x3 / stride 1 / pad 1 convolution over a SPIKE input (training step of the denoiser's conv2..conv6,
 * R/snn_model/vq_diffusion.py:166-187 through autograd; the reference runs the library's fp32 kernels):
 * gw[co][ky][kx][ci] = sum_{n,y,x} gy[n,co,y,x] * s[n,ci,y+ky-1,x+kx-1] on the bf16 matrix cores -- the spikes are exact in bf16,
 * the fp32 output gradient is split into three bf16 terms exactly, so only the fp32 accumulation rounds.  gy_cl / spikes_cl:
 * channels-last fp32 [N = T*B][H*W][C]; gw_out fp32 [Cout][3][3][Cin] (= a channels-last [Cout,Cin,3,3] tensor); ws: scratch of
 * spk_conv3x3_wgrad_ws_bytes (split-K partial sums, added in a fixed order: deterministic).  Shapes:
 * spk_conv3x3_wgrad_supported; otherwise SPK_ERR_UNSUPPORTED (use the framework's operator).
 * The spike operand may also hold small non-negative integers (spike counts up to 256: exact in bf16) -- the time-collapsed
 * backward of the denoiser's last layer.
 * gb_out_or_null [Cout]: the bias gradient (sum of gy over images and positions), from the same pass over gy. */
int spk_conv3x3_wgrad_supported(int Cout, int Cin, int H, int W);
long long spk_conv3x3_wgrad_ws_bytes(int N, int Cout, int Cin);
int spk_conv3x3_wgrad_bf16(const float* gy_cl, const float* spikes_cl, float* ws, long long ws_bytes, float* gw_out,
                           float* gb_out_or_null, int N, int H, int W, int Cout, int Cin, spk_stream_t stream);

/* Data gradient of the same convolution (autograd of layer.Conv2d in the training step, R/snn_model/vq_diffusion.py:166-187;
 * cuDNN's data-gradient kernels in the reference): gi[n][y][x][ci] = sum over (co, ky, kx) of gy[n][y+1-ky][x+1-kx][co] *
 * w[co][ky][kx][ci], channels-last fp32 tensors (gy [N][49][Cout], w [Cout][3][3][Cin], gi [N][49][Cin]).  Both operands are
 * split into three bf16 terms exactly and six cross products run on the bf16 matrix cores with fp32 accumulation (what is
 * dropped is below 2^-24 of a product): an fp32 GEMM's accuracy.  ws: spk_conv3x3_dgrad_ws_bytes(Cout, Cin) bytes (the packed
 * weight terms, rewritten by every call).  Deterministic.  Shapes (49 -> H * W on the other map size) and image counts N:
 * spk_conv3x3_dgrad_supported; otherwise SPK_ERR_UNSUPPORTED (use the framework's operator). */
int spk_conv3x3_dgrad_supported(int Cout, int Cin, int H, int W, int N);
long long spk_conv3x3_dgrad_ws_bytes(int Cout, int Cin);
int spk_conv3x3_dgrad_bf16(const float* gy_cl, const float* w_cl, uint8_t* ws, long long ws_bytes, float* gi_out, int N, int H,
                           int W, int Cout, int Cin, spk_stream_t stream);
/* The same data gradient with TWO fp16 terms per operand and three cross products (half the matrix work): every image's gy
 * and every input channel's weights are scaled by a power of two that puts their largest magnitude into [2^14, 2^15), x 2^s =
 * h + m to 2^-23 (h, m: nearest fp16 of the value and of the exact remainder), products (h,h) (h,m) (m,h), fp32 accumulation,
 * exact descaling.  Values more than 28 binades below their image's / channel's maximum lose relative (not absolute)
 * precision.  Same arguments, workspace and shapes as spk_conv3x3_dgrad_bf16. */
int spk_conv3x3_dgrad_f16x2(const float* gy_cl, const float* w_cl, uint8_t* ws, long long ws_bytes, float* gi_out, int N, int H,
                            int W, int Cout, int Cin, spk_stream_t stream);
/* spk_conv3x3_dgrad_f16x2 in two halves.  pack_multi: the weight half (per-channel maxima + the two fp16 term planes) of
 * n <= 8 layers in ONE launch -- inside a training iteration each layer's backward otherwise spends a fill, a maximum and a pack
 * launch on weights that change once per optimizer step.  HOST arrays of n entries; ws[i]: spk_conv3x3_dgrad_ws_bytes(Cout[i],
 * Cin[i]) bytes; N[i]: the image count the data half will be called with (the packed tile width depends on it).  prepacked: the
 * data half on such a workspace, bit-identical to the one-call form.  A workspace packed for another tile width (another N)
 * yields NaN, not a permuted result. */
int spk_conv3x3_dgrad_f16x2_pack_multi(const float* const* w_cl, uint8_t* const* ws, const long long* ws_bytes, const int* N,
                                       const int* Cout, const int* Cin, int n, spk_stream_t stream);
int spk_conv3x3_dgrad_f16x2_prepacked(const float* gy_cl, const uint8_t* ws, long long ws_bytes, float* gi_out, int N, int H,
                                      int W, int Cout, int Cin, spk_stream_t stream);

/* Weight and bias gradient of a 3x3 / stride 1 / pad 1 convolution with FEW input channels (Cin <= 4) and a dense fp32 input: the
 * denoiser's first layer in the training step (cat(x_t, t): two channels, R/snn_model/vq_diffusion.py:161-165,195-201; what
 * loss.backward() computes through layer.Conv2d, R/main.py:226-252).  gy_cl channels-last [N][H*W][Cout], in_nchw [N][Cin][H][W];
 * gw_out [Cout][3][3][Cin] (weight_channels_last = 1, the storage the training path keeps its weights in) or [Cout][Cin][3][3];
 * gb_out optional [Cout].  ws: spk_conv3x3_wgrad_small_ws_bytes(...) bytes; deterministic (fixed-order partial sums, fp64). */
long long spk_conv3x3_wgrad_small_ws_bytes(int N, int H, int W, int Cout, int Cin);
int spk_conv3x3_wgrad_small(const float* gy_cl, const float* in_nchw, float* ws, long long ws_bytes, float* gw_out,
                            float* gb_out_or_null, int N, int H, int W, int Cout, int Cin, int weight_channels_last,
                            spk_stream_t stream);

/* Training convolutions of the spiking VQ-VAE (R/snn_model/vae_model.py:101-159 under loss.backward(), R/main.py:118-146; cuDNN's
 * forward / data-gradient / weight-gradient kernels in the reference): channels-last fp32 tensors ([N][H][W][C]) on the fp32 matrix
 * cores (v_mfma_f32_32x32x2_f32: fp32 products and accumulation, no operand narrowed).  csrc/conv_train.hip.
 *
 * spk_conv_train_gather: out[N][Ho][Wo][Cout] (+ bias) from in[N][Hi][Wi][Cred] and a k x k weight tensor addressed through three
 * element strides, W(tap, c, co) = w[tap * w_tap + c * w_red + co * w_out]:
 *   form 0: out[n, o, co] = sum over (tap, c) of in[n, o * stride + k - pad, c] * W(tap, c, co)       -- layer.Conv2d forward
 *           (SJ/activation_based/layer.py:164-173), the data gradient of layer.ConvTranspose2d;
 *   form 1: out[n, o, co] = sum over the taps with (o + pad - k) % stride == 0 and c of in[n, (o + pad - k) / stride, c] *
 *           W(tap, c, co)  -- layer.ConvTranspose2d forward (layer.py:316-325), the data gradient of layer.Conv2d; sub-pixel
 *           classes are separate tile rows, structural zeros are not multiplied.
 * Matrix path: Cred % 8 == 0, Cred <= 64, 2 <= Cout <= 64, stride <= 4 (form 1: <= 2), the k * k weight taps of one 32-channel column
 * tile within 150 KB of LDS; vector kernels for Cred <= 4 (form 0, Cout % 4 == 0: the first layer on grey or RGB images, the read-out
 * layer's data gradient) and Cout <= 4 (Cred 8 / 16 / 32 / 64; form 1 only with stride 1: the read-out layer).  N * Ho * Wo and N * Hi * Wi * Cred below 2^31.  spk_conv_train_gather_supported answers 1 / 0; an unsupported call returns
 * SPK_ERR_UNSUPPORTED (the host then takes the framework's operator).  Deterministic; capturable in a hipGraph. */
int spk_conv_train_gather_supported(int Cred, int Cout, int k, int stride, int form);
int spk_conv_train_gather(const float* in_cl, const float* w, const float* bias_or_null, float* out_cl, int N, int Hi, int Wi,
                          int Cred, int Ho, int Wo, int Cout, int k, int stride, int pad, int form, long long w_tap,
                          long long w_red, long long w_out, spk_stream_t stream);
/* spk_conv_train_gather with a fused epilogue, for the plain-CNN VQVAE baseline in training (the ReLU between its layers,
 * R/snn_model/vae_model.py:607-658): separate instantiations of the same kernels, same arguments, shapes, launch forms and error
 * codes; spk_conv_train_gather itself is unchanged.  v = acc + bias is spk_conv_train_gather's value, bit for bit.
 *   _relu:   out = v < 0 ? 0 : v            (a NaN stays NaN, -0.0 stays -0.0: torch.relu's values)
 *   _masked: out = act <= 0 ? 0 : v         act_cl: a channels-last tensor of the output's shape -- threshold_backward's rule on the
 *            SAVED post-ReLU activation (nn.ReLU(inplace=True) keeps only its result): the data gradient through a ReLU.
 * Matrix path and the Cred <= 4 vector kernel; the Cout <= 4 vector kernel (no VQVAE layer needs an epilogue there) returns
 * SPK_ERR_UNSUPPORTED. */
int spk_conv_train_gather_relu(const float* in_cl, const float* w, const float* bias_or_null, float* out_cl, int N, int Hi, int Wi,
                               int Cred, int Ho, int Wo, int Cout, int k, int stride, int pad, int form, long long w_tap,
                               long long w_red, long long w_out, spk_stream_t stream);
int spk_conv_train_gather_masked(const float* in_cl, const float* w, const float* bias_or_null, const float* act_cl, float* out_cl,
                                 int N, int Hi, int Wi, int Cred, int Ho, int Wo, int Cout, int k, int stride, int pad, int form,
                                 long long w_tap, long long w_red, long long w_out, spk_stream_t stream);
/* Weight (and bias) gradient of the same layers: D(tap, cu, cv) = sum over (n, q) of u[n, q * stride - pad + k, cu] * v[n, q, cv],
 * written to gw_out[tap * g_tap + cu * g_u + cv * g_v].  layer.Conv2d: u = the layer's input, v = gy; layer.ConvTranspose2d:
 * u = gy, v = the layer's input (u is the tensor on the finer grid).  bias_from: 0 none, 1: gb_out[cv] = column sums of v, 2:
 * gb_out[cu] = column sums of u.  Every workgroup owns a range of positions; a second launch adds the partial tiles in index order
 * (deterministic).  5 <= Cu <= 64, Cv <= 64 (k * k * ceil(Cu / 32) * ceil(Cv / 32) <= 36 tiles), or Cu <= 4 with Cv in {4, 8, 16, 32, 64}
 * (vector kernel; k <= 3 unless Cu == 1).  ws: spk_conv_train_wgrad_ws_bytes(...) bytes (-1: unsupported shape). */
long long spk_conv_train_wgrad_ws_bytes(int N, int Hv, int Wv, int Cu, int Cv, int k);
int spk_conv_train_wgrad(const float* u_cl, const float* v_cl, float* ws, long long ws_bytes, float* gw_out, float* gb_out_or_null,
                         int N, int Hu, int Wu, int Cu, int Hv, int Wv, int Cv, int k, int stride, int pad, long long g_tap,
                         long long g_u, long long g_v, int bias_from, spk_stream_t stream);

/* ---- sampler ---------------------------------------------------------------------------------------------------- */
/* Images touched by reverse step t.  R/snn_model/vq_diffusion.py:113-124 computes `changes = (u < 1/t) & ~unmasked`
 * BEFORE the denoiser call and only scatters the sample there (:140): for an image without a change at step t the
 * denoiser output is never read.  Writes the ascending list of images with >= 1 change (active_out [B] int32) and its
 * length (n_active_out [2] int32: [0] the length, [1] a work word that must be ZERO before the first call and is left zero);
 * u / Philox arguments exactly as spk_psample_step (same draws; K = the class count of that call: it is the stride of the
 * counter layout, see spk_psample_step).  With sample_steps = 100
 * and 49 positions an image is touched by 39 % of the steps on average: the per-step kernels take the list / count as
 * `active` / `n_dyn` arguments and skip the rest -- the same tokens as the dense loop, fewer evaluations. */
int spk_select_active(const uint8_t* unmasked, int t, const float* u_or_null, unsigned long long philox_seed,
                      unsigned long long philox_offset, const unsigned long long* philox_state_or_null, int* active_out,
                      int* n_active_out, int B, int HW, int K, spk_stream_t stream);
/* Positions of the active images that reverse step t needs from each denoiser layer (same `changes` test as above, per
 * position; R/snn_model/vq_diffusion.py:134-140 reads the denoiser output only there).  need_out: a ZERO-INITIALISED buffer of
 * spk_select_needed_bytes(B, R) bytes (it stays consistent from call to call); for every radius r = 1..R it receives, per
 * active slot, the positions within Chebyshev distance r of a change of image active[slot] -- what a stack of r 3x3
 * convolutions below the logits has to provide (64-byte records: bytes 0..47 ascending positions below 48, padded with the
 * last entry; byte 48 their number n; byte 49 ceil(n / 8); byte 50 whether position 48 is among them) -- and the slots
 * grouped by ceil(n / 8), the form spk_den_conv3x3_mfma_fp6v2_listed walks.  7x7 latents, R <= 8. */
long long spk_select_needed_bytes(int B, int R);
int spk_select_needed(const uint8_t* unmasked, int t, const float* u_or_null, unsigned long long philox_seed,
                      unsigned long long philox_offset, const unsigned long long* philox_state_or_null, const int* active,
                      const int* n_active, uint8_t* need_out, int B, int H, int W, int R, int K, spk_stream_t stream);
/* cat(x, ones_like(x)*t) of DummyModel.forward, R/snn_model/vq_diffusion.py:195-197 -> fp32 [B,2,h,w].
 * active / n_active (both or neither): slot s of the output is image active[s], s < *n_active. */
int spk_den_build_input(const float* x_float_or_null, const long long* x_tokens_or_null, const long long* t_vec_or_null,
                        long long t_scalar, float* out_b2hw, int B, int HW, const int* active_or_null,
                        const int* n_active_or_null, spk_stream_t stream);
/* Loop body of AbsorbingDiffusion.sample after the denoiser call, R/snn_model/vq_diffusion.py:113-124,134-140.
 * logits [B,K,h,w] fp32; x_t int64 [B*HW]; unmasked u8/bool [B*HW]; u [B*HW] / q [B*HW*K] injected noise or NULL
 * (then Philox4x32-10 keyed by seed: position p = image * HW + hw draws u from counter offset + p * K of stream 0 and q_k
 * from counter offset + p * K + k of stream 1 -- ONE rule for both, so a shard that starts at image b0 of a larger job
 * passes offset + b0 * HW * K and draws exactly what the whole job would draw for its images: the sample does not depend
 * on how a batch is split over devices); philox_state optional device {seed, base offset} pair that overrides
 * the seed and is added to the offset (lets a captured hipGraph draw fresh noise on every replay);
 * x0_hat_out optional int64 [B*HW].  The token of a position is argmax_k softmax(logits / temp)_k / q_k, lowest k on a tie;
 * a NaN ratio never wins, and a position without a comparable ratio (a NaN logit, or every logit -inf, where the reference's
 * Categorical raises) gets token 0: the token is always in [0, K).  active / n_active (both or neither; not with x0_hat_out): logits hold one slot
 * per active image (slot s = image active[s]); noise, x_t and unmasked stay indexed by image.
 * next_input_b2hw_or_null (not with active): also writes cat(x_t, t - 1) fp32 [B,2,h,w] -- what spk_den_build_input would
 * produce for the NEXT reverse step (:195-197 with the updated tokens): one launch less per step. */
int spk_psample_step(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t, float temp,
                     const float* u_or_null, const float* q_or_null, unsigned long long philox_seed,
                     unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                     long long* x0_hat_out_or_null, int B, int HW, int K, const int* active_or_null,
                     const int* n_active_or_null, float* next_input_b2hw_or_null, spk_stream_t stream);
/* Per-image temperature: spk_psample_step_temps, spk_pscore_step_temps and spk_den_step_tail_temps take the
 * arguments of spk_psample_step / spk_pscore_step / spk_den_step_tail with `float temp` replaced by `const float* temp_b`, a device
 * array of B fp32 values -- the reference's `x_0_logits / temp` (R/snn_model/vq_diffusion.py:134) with a [B,1,1,1] tensor in place
 * of the scalar.  temp_b is indexed by IMAGE, never by slot of the active list: in the active-set forms slot s reads
 * temp_b[active[s]], as it reads x_t, unmasked and the noise.  The logit is divided by the entry in the same single fp32 division
 * the scalar entry point makes, so for an image whose entry equals the scalar every output (token, unmasked, x0_hat, fp64 logp,
 * step, next_input, the fused first layer's spikes and counts) is bit for bit the scalar entry point's.  The host cannot see
 * device values: the only check on temp_b is for NULL (SPK_ERR_ARG before any launch, as for the other pointers); a non-positive,
 * infinite or NaN entry gives whatever the IEEE division gives, and the kernels' rules for special values then apply -- the token
 * is always in [0, K), the score is the formula evaluated in IEEE fp64.  Every other argument, check and property (all codebook
 * sizes, active lists, philox_state, injected u / q, hipGraph capture) is the sibling's. */
int spk_psample_step_temps(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t, const float* temp_b,
                           const float* u_or_null, const float* q_or_null, unsigned long long philox_seed,
                           unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                           long long* x0_hat_out_or_null, int B, int HW, int K, const int* active_or_null,
                           const int* n_active_or_null, float* next_input_b2hw_or_null, spk_stream_t stream);
/* Top-k truncated sampling: spk_psample_step_topk and spk_den_step_tail_topk take the arguments, checks and
 * properties of spk_psample_step_temps / spk_den_step_tail_temps plus `const int* topk_b`, a device array of B int32 values placed
 * after temp_b and indexed by IMAGE like it (slot s of an active list reads topk_b[active[s]]).  For a position of image i let
 * z_c = logits_c / temp_b[i] (the one fp32 division, classes c < K) and k = topk_b[i]:
 *   - k <= 0 or k >= K: the image is not truncated -- every output is bit for bit the `_temps` entry point's;
 *   - otherwise tau = the k-th largest of the row's non-NaN z_c, counting multiplicity, and every class with z_c < tau (IEEE
 *     comparison) is replaced by -inf before the unchanged race (same operations, same order, same noise counters: the host form is
 *     z.masked_fill(z < z.topk(k).values[..., -1:], -inf)).  Classes equal to tau all stay, so more than k classes may remain;
 *     -0.0 and +0.0 compare equal; a row with fewer than k entries above -inf loses nothing; a NaN is never replaced, so a row
 *     that holds one still gets token 0.  With k = 1 and a unique maximum the token is the arg max whatever the noise.
 * Only positions whose token is drawn are truncated (the changing ones; all of them with x0_hat_out).  The noise of a dropped
 * class is simply not used: no other draw moves, so split independence, philox_state and hipGraph capture hold as before.  tau is
 * an exact order statistic (a bit-wise select over order-preserving keys, csrc/psample_common.h): deterministic, no sort.  The only
 * check on temp_b / topk_b is for NULL (SPK_ERR_ARG before any launch).  There is no truncating score entry point: a token
 * outside the kept set would score -inf. */
int spk_psample_step_topk(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t, const float* temp_b,
                          const int* topk_b, const float* u_or_null, const float* q_or_null, unsigned long long philox_seed,
                          unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                          long long* x0_hat_out_or_null, int B, int HW, int K, const int* active_or_null,
                          const int* n_active_or_null, float* next_input_b2hw_or_null, spk_stream_t stream);
/* Nucleus (top-p) truncated sampling: spk_psample_step_topp and spk_den_step_tail_topp take the arguments, checks
 * and properties of their `_topk` siblings plus `const float* topp_b`, a device array of B fp32 values placed after topk_b and
 * indexed by IMAGE like it.  For a position of image i whose token is drawn let z_c = logits_c / temp_b[i] (the one fp32 division,
 * classes c < K), k = topk_b[i] and p = topp_b[i]:
 *   1. the top-k truncation with k, exactly as spk_psample_step_topk makes it (k <= 0 or k >= K: none);
 *   2. !(p > 0 && p < 1) -- 1, 0, a negative, a NaN: the row is not nucleus-truncated; every output is then bit for bit the `_topk`
 *      entry point's, and with k off too the `_temps` entry point's;
 *   3. otherwise mx = the row maximum of z_c by fmaxf (NaNs ignored); mx not finite: the row stays as it is;
 *   4. integer masses: w_c = expf(z_c - mx) (one fp32 subtraction, one expf, no contraction), m_c = (uint32) rint(w_c * 2^20), round
 *      to nearest even; m_c = 0 for a NaN z_c and for the classes top-k set to -inf; total = sum m_c in uint32 (K <= 2048: <= 2^31);
 *   5. P = (double)p * (double)total, one IEEE fp64 multiplication;
 *   6. with the order-preserving 32-bit keys of the top-k select (a NaN does not count), S(T) = the sum of m_c over the classes with
 *      key_c >= T; tau's key is the largest T with (double)S(T) >= P (built from bit 31 down, 32 integer wave sums);
 *   7. every class with z_c < tau (IEEE comparison) becomes -inf, and the row goes through the unchanged race: same operations, same
 *      order, same noise counters.
 * The kept set is the smallest set of top classes, closed under ties with tau, whose mass reaches p of the total: the row maximum
 * always stays, p -> 0+ leaves only the maxima (a unique maximum: the arg max whatever the noise), classes tying with tau all stay,
 * a NaN is never replaced (such a row still gets token 0).  After the expf everything is integer or single-rounded IEEE arithmetic:
 * no permutation of lanes or classes changes tau, and every launch form computes the same one.  A dropped class's draw is simply
 * not used: no other draw moves, so split independence, philox_state and hipGraph capture hold as before.  The only check on
 * temp_b / topk_b / topp_b is for NULL (SPK_ERR_ARG before any launch).  There is no nucleus score entry point. */
int spk_psample_step_topp(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t, const float* temp_b,
                          const int* topk_b, const float* topp_b, const float* u_or_null, const float* q_or_null,
                          unsigned long long philox_seed, unsigned long long philox_offset,
                          const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null, int B, int HW, int K,
                          const int* active_or_null, const int* n_active_or_null, float* next_input_b2hw_or_null,
                          spk_stream_t stream);
/* Confidence-ordered decoding: spk_psample_step_conf and spk_den_step_tail_conf take the arguments, checks and
 * truncation of their `_topp` siblings WITHOUT active / n_active, plus `float* conf_out_or_null` (fp32 [B*HW]; the step tail: also
 * `long long* x0_hat_out_or_null`).  What changes is WHERE a step reveals.  At reverse step t, for each image i on its own:
 *   1. m = the number of positions masked at entry; n = (m + t - 1) / t in integer arithmetic, ceil(m / t): everything at t = 1,
 *      one per step at m = 49 and 49 steps, 7, 6, 6, 6, 6, 6, 6, 6 at 8 steps;
 *   2. every masked position p gets a candidate token: the unchanged race on logits / temp_b[i] after the top-k and the nucleus
 *      truncation, noise of stream 1 at counter offset + p * K + class (or the injected q) -- bit for bit the x0_hat_out of
 *      spk_psample_step_topp for the same inputs.  The stream-0 uniform of the coin is neither drawn nor read (its per-position
 *      counter stays free), and u_or_null is ignored;
 *   3. the confidence of p is the fp32 log-probability the race itself holds for the drawn class under the truncated, renormalised
 *      row -- z_c - (mx + logf(sum expf(z - mx))) as csrc/psample_common.h computes it, no new arithmetic -- and its order key is
 *      the 32-bit key of the top-k select, under which a NaN (a row with a NaN logit, or all at -inf) has key 0 and orders last;
 *   4. p is revealed iff fewer than n masked positions p' of image i have (key, -p') above (key, -p): larger key first, equal keys
 *      to the lower position.  A revealed position takes its candidate and unmasked = 1; every other position keeps its state and
 *      its candidate is discarded.
 * x0_hat_out (the candidates) and conf_out (the confidences) are written at the positions masked at entry and nowhere else.
 * next_input_b2hw_or_null is written from the committed state.  One workgroup per image, no global workspace, no selection noise;
 * HW > 64: SPK_ERR_UNSUPPORTED with nothing launched; K <= 2048.  There is no active-list form -- which positions change depends
 * on the logits, so no position can be ruled out ahead of the denoiser, and with one step count for the batch no image either
 * (per-image step counts: spk_psample_step_conf_listed below) -- and no score form.  Deterministic, split
 * independent (the draws are the sibling's), capturable in a hipGraph; allocates nothing. */
int spk_psample_step_conf(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t, const float* temp_b,
                          const int* topk_b, const float* topp_b, const float* u_or_null, const float* q_or_null,
                          unsigned long long philox_seed, unsigned long long philox_offset,
                          const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null, float* conf_out_or_null,
                          int B, int HW, int K, float* next_input_b2hw_or_null, spk_stream_t stream);
/* Per-image step counts for confidence-ordered decoding: spk_select_pending and spk_psample_step_conf_listed.
 * THE rule.  Let S be the step count of the loop (t = S .. 1), steps_b[i] (int32 [B], device, indexed by IMAGE) the count of image
 * i and e_i = min(steps_b[i], S).  At reverse step t image i is PENDING iff 1 <= t <= e_i and at least one of its positions is
 * masked; steps_b[i] < 1: never.  A pending image takes exactly the update of spk_psample_step_conf with this t -- a candidate at
 * every masked position, then the commit of the ceil(m / t) surest; a non-pending image is not read, not evaluated and not written.
 * Noise: image i draws the counters it would draw ALONE in a run of e_i steps -- its step index at loop step t is e_i - t, not
 * S - t -- so with the caller's per-step counter stride step_stride (2^40 in the sampler's 'global' layout) the kernel uses
 * philox_offset - (S - e_i) * step_stride for image i, in unsigned 64-bit arithmetic, plus the philox_state base as before; for a
 * pending image that is philox_offset's shard base + (e_i - t) * step_stride and never wraps.  An injected q is used as given.
 * Hence image i of a per-image run equals, bit for bit, image i of a run of e_i steps with the same key, global index, temperature /
 * k / p and start state, whatever S and the other images' counts are.
 *
 * spk_select_pending writes the ascending list of pending images and its length in spk_select_active's output contract
 * (active_out [B] int32; n_active_out [2] int32: [0] the length, [1] a work word ZERO before the first call and left zero;
 * deterministic slots), from `unmasked` and steps_b alone: it draws no noise.  HW > 64: SPK_ERR_UNSUPPORTED.
 *
 * spk_psample_step_conf_listed takes the arguments of spk_psample_step_conf without next_input_b2hw, plus steps_b, S, step_stride
 * and the list (all four pointers required; 1 <= t <= S).  Workgroup s serves slot s and returns at once past *n_active (clamped to
 * B).  logits_skhw hold one slot per listed image (slot s = image active[s]); x_t, unmasked, temp_b / topk_b / topp_b, steps_b, the
 * noise and x0_hat_out / conf_out are indexed by image active[s].  A listed image with t > e_i is left as it is.  A separate
 * kernel: spk_psample_step_conf and spk_den_step_tail_conf keep their code paths, signatures and results.  HW <= 64, K <= 2048;
 * argument errors before any launch; capturable; allocates nothing.  There is no fused step tail on the list. */
int spk_select_pending(const uint8_t* unmasked, int t, const int* steps_b, int* active_out, int* n_active_out, int B, int HW,
                       spk_stream_t stream);
int spk_psample_step_conf_listed(const float* logits_skhw, long long* x_t_inout, uint8_t* unmasked_inout, int t, const float* temp_b,
                                 const int* topk_b, const float* topp_b, const float* u_or_null, const float* q_or_null,
                                 unsigned long long philox_seed, unsigned long long philox_offset,
                                 const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null,
                                 float* conf_out_or_null, int B, int HW, int K, const int* steps_b, int S,
                                 unsigned long long step_stride, const int* active, const int* n_active, spk_stream_t stream);
/* Reveal schedules and annealed selection noise for confidence-ordered decoding (the rule: csrc/psample_common.h):
 * spk_psample_step_conf_sched, spk_psample_step_conf_listed_sched and spk_den_step_tail_conf_sched take the arguments of their
 * `_conf` siblings plus `const uint32_t* sched_w` (required), `const float* noise_a_or_null`, `int S` (where the sibling has none)
 * and `float* score_out_or_null` (fp32 [B*HW], written at the positions masked at entry).  Everything of the `_conf` rule stays --
 * the candidates, their stream-1 counters, the truncation, the fp32 confidence: x0_hat_out and conf_out are bit for bit the
 * sibling's whatever the tables hold -- and two things become inputs, both device tables [B][S + 1] whose row i belongs to IMAGE i
 * and is indexed by the loop's t (1 <= t <= S; entry 0 is read as w[t - 1] at t = 1):
 *   1. HOW MANY.  w = row i of sched_w, entries at most 2^24.  With m positions masked at entry, in unsigned 64-bit arithmetic
 *        keep = w[t] == 0 ? 0 : min(m, (m * w[t - 1]) / w[t]);   n = m - keep;   if m > 0 and n == 0 then n = 1.
 *      Everything is revealed where w[t - 1] == 0, in particular at t = 1 under w[0] = 0.  The linear table w[t] = t gives
 *      m - floor(m (t - 1) / t) = ceil(m / t), the `_conf` count for every m and t; the cosine table of a run of e steps is
 *      w[t] = rint(2^24 sin(pi t / (2 e))), computed in fp64 on the host (masked fraction cos(pi r / 2) after progress r).  A
 *      non-monotone or arbitrary table is legal: the min and the forced 1 define what it means.
 *   2. IN WHAT ORDER.  a = noise_a[i][t]; a null table or a == 0: nothing is drawn and the order key is that of the confidence,
 *      exactly as in the sibling.  Otherwise u is the uniform of the position -- u_or_null[p], which these entry points READ, or
 *      stream 0 at counter offset + p * K, the coin's own counter that the `_conf` kernels leave undrawn, a value in [0, 1) -- and,
 *      each operation rounded once to fp32 (no contraction),
 *        g = -logf(-logf(u));   score = conf + a * g;   key = the 32-bit order key of score.
 *      u = 0 gives g = -inf and (a > 0) score = -inf: the position orders last among the numbers, ahead of the NaNs (key 0).  The
 *      rank rule does not change: (key, -position), larger key first, ties to the lower position.  The noise touches stream 0 only.
 * In the listed form image i draws the Gumbel uniform at its own shifted offset, exactly as its race noise is shifted, and reads
 * row i of both tables at the loop's t (the caller builds row i for e_i = min(steps_b[i], S) steps).  Argument errors before any
 * launch: a null sched_w, S < 1, t outside 1 .. S (SPK_ERR_ARG); HW > 64 (SPK_ERR_UNSUPPORTED).  A family of kernels of its own:
 * the `_conf` entry points keep their code paths, signatures and results.  Capturable; allocates nothing. */
int spk_psample_step_conf_sched(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t, const float* temp_b,
                                const int* topk_b, const float* topp_b, const float* u_or_null, const float* q_or_null,
                                unsigned long long philox_seed, unsigned long long philox_offset,
                                const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null,
                                float* conf_out_or_null, int B, int HW, int K, float* next_input_b2hw_or_null,
                                const uint32_t* sched_w, const float* noise_a_or_null, int S, float* score_out_or_null,
                                spk_stream_t stream);
int spk_psample_step_conf_listed_sched(const float* logits_skhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                       const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                                       const float* q_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                                       const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null,
                                       float* conf_out_or_null, int B, int HW, int K, const int* steps_b, int S,
                                       unsigned long long step_stride, const int* active, const int* n_active,
                                       const uint32_t* sched_w, const float* noise_a_or_null, float* score_out_or_null,
                                       spk_stream_t stream);
/* Remasking for confidence-ordered decoding (the rule: csrc/psample_common.h): spk_psample_step_conf_remask,
 * spk_psample_step_conf_listed_remask and spk_den_step_tail_conf_remask take the arguments of their `_sched` siblings plus
 *   const uint32_t* remask_r        [B][S + 1], required, indexed [image][t] like the two `_sched` tables;
 *   float* commit_conf_inout        fp32 [B*HW], required, read and written in place like x_t / unmasked;
 *   long long mask_id               the token a remasked position takes; a value inside [0, K) is SPK_ERR_ARG;
 *   uint8_t* remasked_out_or_null   [B*HW]: for an image with m > 0, 1 at the positions this step remasked and 0 at its others;
 *                                   untouched for an image with m = 0 or, in the listed form, with t > e_i.
 * The family sits on top of the `_sched` family only (a null noise_a is a = 0; the linear table w[t] = t gives the ceil(m / t)
 * counts).  commit_conf is one more piece of per-position state: +inf at the positions unmasked when the run started -- the known
 * tokens, never revisited; a committed log-probability is <= 0, so +inf cannot arise otherwise --, the confidence of its reveal at a
 * position a step revealed, anything (ignored) at a masked position.  The denoiser's logits at an unmasked position are untrained (the
 * loss ignores those positions), so a committed token is never re-scored: its trust is the confidence it was committed with, and a
 * remasked position draws again only at the NEXT step, after a denoiser call has seen it masked.  At reverse step t, per image:
 *   1. m = positions masked at entry.  m == 0: the image is left as the sibling leaves it, and nothing is remasked.
 *   2. Candidates, confidences, scores, the count n and the revealed set follow the `_sched` rule exactly: x0_hat_out, conf_out,
 *      score_out and the revealed positions are bit for bit the sibling's on the same state and tables.
 *   3. A position is revisable iff it was unmasked at entry and commit_conf != +inf (one revealed in this step is not).  c = their
 *      number, r = min(remask_r[i][t], c); the kernel forces r = 0 at t = 1, so a run never ends with a masked position.  Order key =
 *      the 32-bit key of commit_conf (a NaN: key 0).  A revisable p is remasked iff fewer than r revisable p' have (key, -p') below
 *      (key, -p): smaller key first, equal keys to the HIGHER position -- the reveal's order from the other end.  A remasked p gets
 *      x_t = mask_id and unmasked = 0; its commit_conf stays.
 *   4. Every revealed p gets commit_conf[p] = its confidence (conf_out's value, not the noise-perturbed score).
 *   5. next_input_b2hw and the fused first layer of the step tail read the state after 3 and 4.
 * From m0 masked positions the revisable count at entry of step t is m0 - m_t, so the counts of a run are host integers: n_t = the
 * `_sched` count of m_t, r_t = t >= 2 ? min(R[t], m0 - m_t) : 0, m_(t-1) = m_t - n_t + r_t.  Listed form: commit_conf, remask_r and
 * remasked_out are indexed by image active[s].  Argument errors before any launch: the siblings', a null remask_r or
 * commit_conf_inout, mask_id inside [0, K) (SPK_ERR_ARG).  The `_sched` and `_conf` entry points keep their code paths, signatures
 * and results.  Capturable; allocates nothing. */
int spk_psample_step_conf_remask(const float* logits_bkhw, long long* x_t_inout, uint8_t* unmasked_inout, int t, const float* temp_b,
                                 const int* topk_b, const float* topp_b, const float* u_or_null, const float* q_or_null,
                                 unsigned long long philox_seed, unsigned long long philox_offset,
                                 const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null,
                                 float* conf_out_or_null, int B, int HW, int K, float* next_input_b2hw_or_null,
                                 const uint32_t* sched_w, const float* noise_a_or_null, int S, float* score_out_or_null,
                                 const uint32_t* remask_r, float* commit_conf_inout, long long mask_id,
                                 uint8_t* remasked_out_or_null, spk_stream_t stream);
int spk_psample_step_conf_listed_remask(const float* logits_skhw, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                                        const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                                        const float* q_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                                        const unsigned long long* philox_state_or_null, long long* x0_hat_out_or_null,
                                        float* conf_out_or_null, int B, int HW, int K, const int* steps_b, int S,
                                        unsigned long long step_stride, const int* active, const int* n_active,
                                        const uint32_t* sched_w, const float* noise_a_or_null, float* score_out_or_null,
                                        const uint32_t* remask_r, float* commit_conf_inout, long long mask_id,
                                        uint8_t* remasked_out_or_null, spk_stream_t stream);
/* The same loop body run TEACHER-FORCED (csrc/pscore.hip): the reverse process scores given tokens x0 int64
 * [B*HW] instead of drawing tokens.  changes = (u < 1/t) & ~unmasked with the u of spk_psample_step (injected, or the same Philox
 * counters: stream 0 at offset + p * K; the q stream is not drawn), and at a changing position p
 *   logp_out[p] = log softmax(logits / temp)[x0[p]]   fp64, in nats: z_k = logits_k / temp in fp32 (the value the sampler races
 *                 with), then (z_x0 - m) - log sum_k exp(z_k - m) in fp64 with m = max_k z_k, summed in a fixed order;
 *   step_out[p] = t (optional int32);   x_t[p] = x0[p];   unmasked[p] = 1.
 * Every other position writes nothing to logp_out / step_out and evaluates no softmax.  Special values are what the formula gives
 * in IEEE fp64 (a NaN logit: NaN; target logit -inf: -inf; every logit -inf: NaN); a target outside [0, K) scores -inf, and x_t
 * still takes it as given (nothing gathers through x_t: the denoiser reads the token as a float).  Summed over the positions
 * after steps t = S .. 1 from the all-masked (or a partly known, spk_completion_state) start this is a one-sample estimate of the
 * sampler's likelihood bound E_order[sum_i log p(x0_i | x0 at the positions revealed before i)] <= log p(x0).
 * active / n_active, philox_state, next_input_b2hw_or_null (not with active): as spk_psample_step.  K <= 512
 * (SPK_ERR_UNSUPPORTED beyond).  Deterministic; capturable in a hipGraph; allocates nothing. */
int spk_pscore_step(const float* logits_bkhw, const long long* x0, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                    float temp, const float* u_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                    const unsigned long long* philox_state_or_null, double* logp_out, int* step_out_or_null, int B, int HW,
                    int K, const int* active_or_null, const int* n_active_or_null, float* next_input_b2hw_or_null,
                    spk_stream_t stream);
/* spk_pscore_step with one temperature per image: see spk_psample_step_temps. */
int spk_pscore_step_temps(const float* logits_bkhw, const long long* x0, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                          const float* temp_b, const float* u_or_null, unsigned long long philox_seed,
                          unsigned long long philox_offset, const unsigned long long* philox_state_or_null, double* logp_out,
                          int* step_out_or_null, int B, int HW, int K, const int* active_or_null, const int* n_active_or_null,
                          float* next_input_b2hw_or_null, spk_stream_t stream);

/* The tail of one DENSE reverse step as one launch per image: conv6 on the spike counts + mean over T (as
 * spk_den_conv3x3_counts_mfma; R/snn_model/vq_diffusion.py:185-187,205-206), the token update (as spk_psample_step: :113-124,
 * 134-140, same u / q / Philox arguments and draws) and -- unless x1_s32_out is NULL (last step) -- the first denoiser layer of
 * the NEXT step on cat(x_t, t - 1) (as spk_conv_fused_fwd on a time-invariant input: :161-165,195-201): S32 spikes
 * [B][2][HW][16][16 B] and spike counts u8 [B][2][HW][32].  cnt5 [B][8][HW][32] / cnt1 [B][2][HW][32]: spike counts of conv5 /
 * conv1 of THIS step; wq / scale / bias_d: conv6 packed by spk_den_pack_weight_i8 with its output channels zero-padded to
 * ceil16(K) (any --codebook_size, R/main.py:58: classes >= K are masked in the sampling exactly as spk_psample_step masks them);
 * conv1_w_packed: spk_pack_conv_weight of the first layer ([9][2][64]); bn1_a / bn1_b: its folded BatchNorm.  logits_out optional
 * fp32 [B][K][H][W].  1 <= K <= 512, 7x7 or 8x8 latents, 256 + 64 input channels (the reference's architecture); anything
 * else: SPK_ERR_UNSUPPORTED (use the three launches).
 * The fused first layer is the time-invariant-input form with the module defaults baked in: T = 16 steps and
 * LIFNode(tau = 2, v_threshold = 1, v_reset = 0) (R/snn_model/vq_diffusion.py:161-165); with x1_s32_out set any other T is
 * SPK_ERR_UNSUPPORTED (conv6 alone takes T <= 127).
 * active / n_active (round 6, both or neither): the active-set form of the untouched-image elimination (spk_select_active) -- workgroup s
 * serves slot s of the list: cnt5 / cnt1 / logits_out are indexed by slot (what the active-set denoiser launches produced), x_t / unmasked /
 * the noise by image active[s], so the draws are those of the dense form; x1_s32_out must be NULL there (the next step's first layer is
 * the next step's active set's). */
#define SPK_STEP_TAIL_MAX_K 512 /* the largest K spk_den_step_tail and its _temps / _topk / _topp / _conf forms take */
int spk_den_step_tail(const uint8_t* cnt5, int nch5, const uint8_t* cnt1, int nch1, const int8_t* wq, const double* scale,
                      const double* bias_d, float* logits_out_or_null, long long* x_t_inout, uint8_t* unmasked_inout, int t,
                      float temp, const float* u_or_null, const float* q_or_null, unsigned long long philox_seed,
                      unsigned long long philox_offset, const unsigned long long* philox_state_or_null,
                      const float* conv1_w_packed_or_null, const float* conv1_bias_or_null, const float* bn1_a,
                      const float* bn1_b, uint8_t* x1_s32_out_or_null, uint8_t* cnt1_out_or_null, int T, int B, int H, int W,
                      int K, const int* active_or_null, const int* n_active_or_null, spk_stream_t stream);
/* spk_den_step_tail with one temperature per image (workgroup s of the active-set form reads temp_b[active[s]]): see
 * spk_psample_step_temps. */
int spk_den_step_tail_temps(const uint8_t* cnt5, int nch5, const uint8_t* cnt1, int nch1, const int8_t* wq, const double* scale,
                            const double* bias_d, float* logits_out_or_null, long long* x_t_inout, uint8_t* unmasked_inout,
                            int t, const float* temp_b, const float* u_or_null, const float* q_or_null,
                            unsigned long long philox_seed, unsigned long long philox_offset,
                            const unsigned long long* philox_state_or_null, const float* conv1_w_packed_or_null,
                            const float* conv1_bias_or_null, const float* bn1_a, const float* bn1_b,
                            uint8_t* x1_s32_out_or_null, uint8_t* cnt1_out_or_null, int T, int B, int H, int W, int K,
                            const int* active_or_null, const int* n_active_or_null, spk_stream_t stream);
/* spk_den_step_tail with top-k truncation (1 <= K <= 512; workgroup s of the active-set form reads temp_b[active[s]] and
 * topk_b[active[s]]): see spk_psample_step_topk. */
int spk_den_step_tail_topk(const uint8_t* cnt5, int nch5, const uint8_t* cnt1, int nch1, const int8_t* wq, const double* scale,
                           const double* bias_d, float* logits_out_or_null, long long* x_t_inout, uint8_t* unmasked_inout,
                           int t, const float* temp_b, const int* topk_b, const float* u_or_null, const float* q_or_null,
                           unsigned long long philox_seed, unsigned long long philox_offset,
                           const unsigned long long* philox_state_or_null, const float* conv1_w_packed_or_null,
                           const float* conv1_bias_or_null, const float* bn1_a, const float* bn1_b,
                           uint8_t* x1_s32_out_or_null, uint8_t* cnt1_out_or_null, int T, int B, int H, int W, int K,
                           const int* active_or_null, const int* n_active_or_null, spk_stream_t stream);
/* spk_den_step_tail with top-k and nucleus truncation (1 <= K <= 512; workgroup s of the active-set form reads temp_b[active[s]],
 * topk_b[active[s]] and topp_b[active[s]]): see spk_psample_step_topp. */
int spk_den_step_tail_topp(const uint8_t* cnt5, int nch5, const uint8_t* cnt1, int nch1, const int8_t* wq, const double* scale,
                           const double* bias_d, float* logits_out_or_null, long long* x_t_inout, uint8_t* unmasked_inout,
                           int t, const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                           const float* q_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                           const unsigned long long* philox_state_or_null, const float* conv1_w_packed_or_null,
                           const float* conv1_bias_or_null, const float* bn1_a, const float* bn1_b,
                           uint8_t* x1_s32_out_or_null, uint8_t* cnt1_out_or_null, int T, int B, int H, int W, int K,
                           const int* active_or_null, const int* n_active_or_null, spk_stream_t stream);
/* spk_den_step_tail under the confidence-ordered reveal (1 <= K <= 512, 7x7 or 8x8; no active list): conv6 on the counts, a
 * candidate at every masked position, the commit of the n = ceil(m / t) surest by one wave, then the fused first layer on the
 * committed tokens -- bit for bit spk_den_conv3x3_counts_mfma, spk_psample_step_conf and the first layer as three launches: see
 * spk_psample_step_conf.  x0_hat_out / conf_out optional, written at the positions masked at entry. */
int spk_den_step_tail_conf(const uint8_t* cnt5, int nch5, const uint8_t* cnt1, int nch1, const int8_t* wq, const double* scale,
                           const double* bias_d, float* logits_out_or_null, long long* x_t_inout, uint8_t* unmasked_inout,
                           int t, const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                           const float* q_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                           const unsigned long long* philox_state_or_null, const float* conv1_w_packed_or_null,
                           const float* conv1_bias_or_null, const float* bn1_a, const float* bn1_b,
                           uint8_t* x1_s32_out_or_null, uint8_t* cnt1_out_or_null, int T, int B, int H, int W, int K,
                           long long* x0_hat_out_or_null, float* conf_out_or_null, spk_stream_t stream);
/* spk_den_step_tail_conf under a reveal schedule and annealed selection noise (the rule and the four added
 * arguments: spk_psample_step_conf_sched): bit for bit spk_den_conv3x3_counts_mfma, spk_psample_step_conf_sched and the first
 * layer as three launches.  u_or_null is read (the Gumbel uniform).  A null sched_w, S < 1 or t outside 1 .. S: SPK_ERR_ARG. */
int spk_den_step_tail_conf_sched(const uint8_t* cnt5, int nch5, const uint8_t* cnt1, int nch1, const int8_t* wq, const double* scale,
                                 const double* bias_d, float* logits_out_or_null, long long* x_t_inout, uint8_t* unmasked_inout,
                                 int t, const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                                 const float* q_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                                 const unsigned long long* philox_state_or_null, const float* conv1_w_packed_or_null,
                                 const float* conv1_bias_or_null, const float* bn1_a, const float* bn1_b,
                                 uint8_t* x1_s32_out_or_null, uint8_t* cnt1_out_or_null, int T, int B, int H, int W, int K,
                                 long long* x0_hat_out_or_null, float* conf_out_or_null, const uint32_t* sched_w,
                                 const float* noise_a_or_null, int S, float* score_out_or_null, spk_stream_t stream);
/* spk_den_step_tail_conf_sched with remasking (the rule and the four added arguments:
 * spk_psample_step_conf_remask): bit for bit spk_den_conv3x3_counts_mfma, spk_psample_step_conf_remask and the first layer as three
 * launches -- a remasked position enters the fused first layer as mask_id.  A null remask_r or commit_conf_inout, or mask_id
 * inside [0, K): SPK_ERR_ARG. */
int spk_den_step_tail_conf_remask(const uint8_t* cnt5, int nch5, const uint8_t* cnt1, int nch1, const int8_t* wq, const double* scale,
                                  const double* bias_d, float* logits_out_or_null, long long* x_t_inout, uint8_t* unmasked_inout,
                                  int t, const float* temp_b, const int* topk_b, const float* topp_b, const float* u_or_null,
                                  const float* q_or_null, unsigned long long philox_seed, unsigned long long philox_offset,
                                  const unsigned long long* philox_state_or_null, const float* conv1_w_packed_or_null,
                                  const float* conv1_bias_or_null, const float* bn1_a, const float* bn1_b,
                                  uint8_t* x1_s32_out_or_null, uint8_t* cnt1_out_or_null, int T, int B, int H, int W, int K,
                                  long long* x0_hat_out_or_null, float* conf_out_or_null, const uint32_t* sched_w,
                                  const float* noise_a_or_null, int S, float* score_out_or_null, const uint32_t* remask_r,
                                  float* commit_conf_inout, long long mask_id, uint8_t* remasked_out_or_null, spk_stream_t stream);
/* q_sample of the diffusion training step, R/snn_model/vq_diffusion.py:61-75: mask = u < t[b] / num_timesteps (fp32, as there);
 * x_t = mask ? mask_id : x_0;  x_0_ignore = mask ? x_0 : -1 (the loss's ignore index).  x0 / u / outputs fp32 [B*HW], t int64 [B],
 * mask_out optional u8.  u is the caller's draw (torch.rand_like in the reference's order). */
int spk_q_sample(const float* x0, const long long* t, const float* u, float* x_t_out, float* x0_ignore_out,
                 uint8_t* mask_out_or_null, int B, int HW, int num_timesteps, float mask_id, spk_stream_t stream);
/* The noise of one reverse step as spk_psample_step / spk_select_active / spk_select_needed draw it in Philox mode, written
 * out (parity aid: R/snn_model/vq_diffusion.py:116 `rand_like` -> u, :138 `Categorical.sample()` -> q ~ Exp(1)): u_out [B*HW] =
 * the uniforms of the `changes` test, q_out [B*HW*K] = the exponentials of the categorical race; same (seed, offset,
 * philox_state) arguments as the step they belong to.  The oracle run on these must reproduce the Philox-mode tokens. */
int spk_philox_noise(unsigned long long philox_seed, unsigned long long philox_offset,
                     const unsigned long long* philox_state_or_null, float* u_out_or_null, float* q_out_or_null, int B, int HW,
                     int K, spk_stream_t stream);

/* ---- completion of partly given images (csrc/completion.hip) ---------------------------------------- */
/* Start state of a conditional reverse process: the loop of R/snn_model/vq_diffusion.py:110-140 run from
 *   unmasked = known & (0 <= code < K),   x_t = unmasked ? code : mask_id
 * instead of the all-masked state (:106-107).  codes int64 [B,h,w]; keep_mask u8 [B,Hm,Wm] (non-zero = given) at a resolution
 * related to the tokens by (stride, radius): token (i,j) is known iff every mask byte in rows stride*i - radius .. stride*i +
 * radius and columns stride*j - radius .. stride*j + radius, clipped to the mask, is non-zero.  (1, 0): a mask at latent
 * resolution.  (4, 3): a pixel mask seen through the encoder's receptive field (Conv 3x3 s2 p1 twice, then 1x1,
 * R/snn_model/vae_model.py:101-129: code (i,j) reads pixels 4i-3 .. 4i+3; the zero padding outside the image counts as given).
 * A code outside [0, K) is never known, so no out-of-range index reaches an embedding gather later.  x_t_out int64 [B,1,h,w],
 * unmasked_out u8 [B,1,h,w], n_known_out (optional) int32 [B] = known tokens per image (a second small launch).  One thread per
 * token; deterministic; capturable in a hipGraph.  SPK_ERR_ARG also when a token's window misses the mask altogether
 * (stride * (h - 1) - radius > Hm - 1, likewise for the columns). */
int spk_completion_state(const long long* codes_bhw, const uint8_t* keep_mask, long long* x_t_out, uint8_t* unmasked_out,
                         int* n_known_out_or_null, int B, int h, int w, int Hm, int Wm, int stride, int radius, int K,
                         long long mask_id, spk_stream_t stream);
/* The given pixels pasted over a decoded image: out[b,c,y,x] = keep[b,y,x] ? uint8(clip(image[b,c,y,x] + 0.5, 0, 1) * 255)
 * : decoded_u8[b,c,y,x] -- the image conversion of R/main.py:401 (fp32, truncating cast; a NaN pixel gives 0) where the pixel
 * is given, the decoder's uint8 elsewhere.  image fp32 [B,C,H,W] normalised (pixel - 0.5), keep u8 [B,H,W], decoded / out u8
 * [B,C,H,W] (out is a buffer of its own). */
int spk_completion_compose(const float* image_bchw, const uint8_t* keep_bhw, const uint8_t* decoded_u8_bchw, uint8_t* out_u8_bchw,
                           int B, int C, int H, int W, spk_stream_t stream);

/* Content checksum of n device tensors in one launch (host-side cache validation; no reference counterpart: the reference
 * re-reads its weights on every call, this library keeps derived forms of them).  table_dev: device array of n pairs
 * {address, number of 32-bit words}; out1: one device word.  Order-independent 64-bit sum. */
int spk_checksum_multi(const unsigned long long* table_dev, int n, unsigned long long* out1, spk_stream_t stream);

/* ---- spike counts (syops report) -------------------------------------------------------------------------------- */
/* Spikes in a tensor the library emitted, all time steps and time step 0 alone -- the firing rates R/syops/ops.py:14-24
 * (`spike_rate`) and :69-75 (the LIF hook reads output[0]) feed into the ACs / MACs report.  The tensor is read as
 * n_words u32 words; word w belongs to time step (w / inner_words) % T.  kind 0: u8 {0,1} bytes (PTC / CPTC), 1: fp4
 * nibbles (C4 / S32), 2: fp32 ([T][N]).  out3 (device, 3 x u64): spikes, spikes at t = 0, fp32 words equal to 1.0f (kind 2:
 * nonzero == ones  <=>  the tensor is binary). */
int spk_count_spikes(const void* data, long long n_words, long long inner_words, int T, int kind, unsigned long long* out3,
                     spk_stream_t stream);

/* ---- SNN_VAE baseline: spiking MLP layers and the autoregressive Bernoulli loops (eval) ------------------------------ */
/* input / output layouts of spk_linear_lif_fwd */
#define SPK_LIN_IN_F32 0  /* fp32 [T,B,in], any values                                                   */
#define SPK_LIN_IN_U8 1   /* u8 {0,1} spikes [T,B,in]                                                    */
#define SPK_LIN_IN_PTC 2  /* u8 PTC spikes [B,H,W,T,C], in = C*H*W read in flatten(C,H,W) order (c*H*W + h*W + w) */
#define SPK_LIN_OUT_F32 0 /* the Linear's currents, fp32 [T,B,out]; no neuron, v unused                  */
#define SPK_LIN_OUT_U8 1  /* LIF spikes u8 [T,B,out]; out may be NULL (state-only pass)                  */
#define SPK_LIN_OUT_PTC 2 /* LIF spikes u8 PTC [B,H,W,T,C], out = C*H*W in flatten(C,H,W) order          */

/* Multi-step layer.Linear followed by the models' LIFNode (tau 2, v_th 1, hard reset to 0, decay_input): replaces
 * SJ/activation_based/layer.py Linear (nn.Linear over seq_to_ann_forward) + the eval LIF of neuron.py:799-811 for
 * R/snn_model/vae_model.py:212-216 (before_latent_layer: PTC in), :224-228 (decoder_input: PTC out, consumed by the fused
 * decoder, :256-260) and the prior's teacher-forced eval pass :365-403.  out = SPK_LIN_OUT_F32 is layer.Linear alone.
 * w [out,in], bias [out] (may be NULL) fp32; v_inout [B,out] fp32, the neuron state before / after (LIF outputs only);
 * ptc_c/h/w describe the PTC side.  Each output is an fp32 sum over the inputs in ascending order, then + bias. */
int spk_linear_lif_fwd(const void* x, int in_kind, const float* w, const float* bias_or_null, float* v_inout_or_null,
                       void* out_or_null, int out_kind, int T, int B, int in_features, int out_features, int ptc_c, int ptc_h,
                       int ptc_w, spk_stream_t stream);
/* One whole autoregressive loop of the SNN_VAE's Bernoulli latent model, every pass in one launch: with x (u8 spikes
 * [T,B,cx]) PosteriorBernoulliSTBP.forward (R/snn_model/vae_model.py:470-546: T-1 passes over the prefixes of [x, z],
 * then one full pass), with x NULL (cx 0) PriorBernoulliSTBP.sample (:405-423: T passes over the prefixes of z).  The MLP is
 * w1 [h1, cx+cz], w2 [h2,h1], w3 [cz*k, h2] with biases, each layer followed by the LIF of spk_linear_lif_fwd with state
 * v1/v2/v3 [B,h] carried in and out (no pass resets it); z0 = initial_input [cz].  idx int32 [T,B,cz] in [0,k): the host's
 * draws (torch.randint(0, k, (B*cz,)) in the reference's order), z_t = spike[c*k + idx].  sampled_z_out fp32 [T,B,cz];
 * q_z_out (posterior only, may be NULL) u8 [T,B,cz*k], the spikes of the final pass.  T <= 16. */
int spk_svae_ar_fwd(const uint8_t* x_or_null, const float* z0, const float* w1, const float* b1, const float* w2,
                    const float* b2, const float* w3, const float* b3, float* v1_inout, float* v2_inout, float* v3_inout,
                    const int* idx, float* sampled_z_out, uint8_t* q_z_out_or_null, int T, int B, int cx, int cz, int h1,
                    int h2, int k, spk_stream_t stream);

/* ---- SNN_VAE baseline: training path (R/snn_model/vae_model.py:198-546 in train() mode) ------------------------------ */
/* The no-grad prefix passes of one training Bernoulli loop in ONE launch (the kernel of spk_svae_ar_fwd in a prefix mode).
 * Posterior (x u8 [T,B,cx], idx [T,B,cz] as in spk_svae_ar_fwd): the T-1 passes over the prefixes of [x, z] (:491-513).
 * Prior (x NULL, cx 0; :365-390 with self.training): sched u8 [T-1] (step t scheduled: t >= 5 and random.random() < p),
 * noise fp32 [n_sched,B,cz] (the torch.randn_like draws of the scheduled steps, in order), z_teacher fp32 [T,B,cz] (the
 * posterior's z): a scheduled step runs the MLP over the prefix and sets z_{t+1} = (count_k / k + 0.001f * noise > 0.5), any
 * other step appends z_teacher[t].  Both write z_t_minus_out fp32 [T,B,cz] (z_0 = z0, the input of the grad pass) and
 * leave v1..v3 as the reference leaves them.  2 <= T <= 16. */
int spk_svae_ar_prefix_fwd(const uint8_t* x_or_null, const float* z0, const float* w1, const float* b1, const float* w2,
                           const float* b2, const float* w3, const float* b3, float* v1_inout, float* v2_inout,
                           float* v3_inout, const int* idx_or_null, const uint8_t* sched_or_null, const float* noise_or_null,
                           const float* z_teacher_or_null, float* z_t_minus_out, int T, int B, int cx, int cz, int h1, int h2,
                           int k, spk_stream_t stream);
/* Multi-step layer.Linear + the LIFNode's surrogate-gradient training forward.  Input [x | x2] (x2 may be NULL), each fp32
 * or u8 {0,1} (SPK_LIN_IN_F32 / SPK_LIN_IN_U8) [T,B,n], w [out, x_features + x2_features], bias may be NULL.  lif = 1:
 * out fp32 spikes [T,B,out], h_seq fp32 [T,B,out] (membrane before reset), v_out [B,out] from v_init (NULL: zeros; may
 * alias v_out).  lif = 0: out = the Linear's currents, h / v unused.  Same sums as spk_linear_lif_fwd. */
int spk_linear_lif_train_fwd(const void* x, int x_kind, int x_features, const void* x2_or_null, int x2_kind, int x2_features,
                             const float* w, const float* bias_or_null, const float* v_init_or_null, float* out,
                             float* h_seq_or_null, float* v_out_or_null, int lif, int T, int B, int out_features,
                             spk_stream_t stream);
/* Backward of spk_linear_lif_train_fwd.  h_seq given: LIF BPTT first (tau 2, v_th 1, v_reset 0, ATan alpha 2,
 * detach_reset off, no gradient into v_init) into dI_ws [T,B,out]; h_seq NULL: grad_out is dL/dcurrents.  Then
 * grad_x [T*B, grad_x_cols] = dI W[:, :grad_x_cols] (may be NULL), grad_w [out, in] = dI^T [x | x2], grad_b [out] = sum dI
 * (may be NULL).  Fixed-order fp32 sums: deterministic. */
int spk_linear_lif_train_bwd(const float* grad_out, const float* h_seq_or_null, float* dI_ws_or_null, const void* x,
                             int x_kind, int x_features, const void* x2_or_null, int x2_kind, int x2_features, const float* w,
                             float* grad_x_or_null, int grad_x_cols, float* grad_w, float* grad_b_or_null, int T, int B,
                             int out_features, spk_stream_t stream);
/* Workspace (floats) of spk_svae_latent_loss_fwd's loss reduction. */
int spk_svae_latent_loss_ws_floats(int B, int cz);
/* The posterior's gather and the latent MMD loss (:273-285, :531-541).  q_z, p_z fp32 [T,B,cz*k] (layer-3 spikes of the
 * grad passes), idx int32 [T,B,cz]: sampled_z [T,B,cz] = q_z[.., c*k + idx] (may be NULL); loss [1] =
 * mean((PSP(mean_k q) - PSP(mean_k p))^2), PSP at tau_s (p_z and loss both given or both NULL).  Fixed-order reduction. */
int spk_svae_latent_loss_fwd(const float* q_z, const float* p_z_or_null, const int* idx, float* sampled_z_or_null,
                             float* loss_or_null, float* ws, int T, int B, int cz, int k, float tau_s, spk_stream_t stream);
/* Its backward: grad_q_z = the MMD term (g_loss, device [1], may be NULL) spread over k plus the scatter of
 * g_sampled_z [T,B,cz] (may be NULL) at idx; grad_p_z (may be NULL) = minus the MMD term. */
int spk_svae_latent_loss_bwd(const float* q_z, const float* p_z_or_null, const int* idx, const float* g_loss_or_null,
                             const float* g_sampled_z_or_null, float* grad_q_z, float* grad_p_z_or_null, int T, int B, int cz,
                             int k, float tau_s, spk_stream_t stream);

/* ---- SNN_VQVAE_uni: codebook-usage statistic (csrc/vq_usage.hip) ---------------------------------------------------- */
/* The statistic VectorQuantizer_uni.forward computes on every call, R/snn_model/vae_model.py:705-718 (unique, bincount, argmax,
 * masked_select, mse_loss), in one launch.  idx int64 [N] (entries outside [0, K) are not counted) ->
 *   hist_out int64 [K] = bincount(idx, minlength=K);
 *   stats_out int64 [3] = {number of used codes, max_index (first maximum of hist), FID_loss};
 * FID_loss is fp32, stored as its bit pattern in the low 32 bits of stats_out[2]: 0.001f * sum_{k != max_index}
 * ((float)hist[k] - (float)N / K)^2 / (K - 1), fp32 arithmetic, fixed summation order (K = 1: NaN, as mse_loss of empty
 * tensors).  Integer results are exact; the whole result is deterministic.  ws: at least 8 * (K + 1) bytes, zeroed by the call
 * (one hipMemsetAsync ahead of the launch); capturable in a hipGraph.  SPK_ERR_UNSUPPORTED for K > SPK_VQ_USAGE_MAX_K (the LDS histogram) or
 * N > 2^31 - 1. */
#define SPK_VQ_USAGE_MAX_K 4096
int spk_vq_code_usage(const long long* idx, long long N, int K, long long* hist_out, long long* stats_out, void* ws,
                      spk_stream_t stream);

/* ---- reconstruction metrics of main.py: SSIM and MSE (csrc/ssim.hip) ------------------------------------------------ */
/* Workspace of spk_ssim_mse in bytes (two fp64 partials per 32x32 tile of every output plane), or the SPK_ERR_* code
 * spk_ssim_mse would return for these sizes. */
long long spk_ssim_mse_ws_bytes(int N, int C, int H, int W, int window_size);
/* The per-batch metrics of R/main.py:318-320 in one launch (two when an image has several channels or tiles): _ssim of R/metric/pytorch_ssim/__init__.py:17-39 (five depthwise
 * window convolutions with zero padding window_size / 2, the SSIM map, its mean) and the squared error of F.mse_loss.  img1,
 * img2 fp32 [N,C,H,W] contiguous; window2d fp32 [window_size, window_size], the values of create_window (:11-15).  Inputs and
 * window are widened to fp64 and every product, window sum (direct 2-D form), map value and reduction is fp64:
 *   ssim_sum_out fp64 [N] = sum of the SSIM map of image n over (C, H', W'), H' = H + 2 (window_size / 2) - window_size + 1
 *                           (H for an odd window, H + 1 for an even one; a window larger than the image is legal);
 *   sq_sum_out   fp64 [N] = sum of (img1 - img2)^2 of image n over (C, H, W).
 * SSIM(size_average=True) = sum(ssim_sum) / (N C H' W'), size_average=False = ssim_sum / (C H' W'), mse = sum(sq_sum) / (N C H W).
 * A NaN in an image makes that image's two sums NaN and no other's.  Fixed-order reductions, no floating-point atomics: two
 * calls give bit-equal results.  ws_buf: spk_ssim_mse_ws_bytes bytes, 8-byte aligned, this call's alone while it is in flight;
 * nothing is expected of its contents (the per-tile partials are written before the second launch reads them); capturable in a
 * hipGraph.  SPK_ERR_UNSUPPORTED for window_size > SPK_SSIM_MAX_WINDOW or 2^31 tiles and more. */
#define SPK_SSIM_MAX_WINDOW 31
int spk_ssim_mse(const float* img1, const float* img2, const float* window2d, double* ssim_sum_out, double* sq_sum_out,
                 void* ws_buf, int N, int C, int H, int W, int window_size, spk_stream_t stream);

/* ---- sample quality: feature moments and polynomial-kernel sums (csrc/feature_stats.hip) ----------------------------- */
/* The arithmetic R/main.py's last stage runs after its feature network (R/metric/Fid_score.py: mean and covariance for the
 * Frechet distance; torchmetrics' KernelInceptionDistance: a polynomial-kernel MMD), on any fp32 feature matrix, on the fp64
 * matrix cores (v_mfma_f64_16x16x4_f64).  The fp32 features are widened to fp64 in registers: every product is exact and
 * only the accumulation rounds.  No allocation, no synchronisation, fixed-order reductions, no floating-point atomics;
 * capturable in a hipGraph; two calls give bit-equal results.
 *
 * spk_feature_moments_acc: x fp32 [n, d] with row_stride >= d elements between rows; sum_inout fp64 [d] and gram_inout fp64
 *   [d, d] (contiguous) are updated in place:  sum += sum over rows of x,  gram += x^T x.
 *   Every element of gram is ONE chain owned by one wave: acc = gram_in; for k0 = 0, 4, 8, ...: acc = mfma(rows k0 .. k0 + 3,
 *   acc); rows at or beyond n are fed as zeros.  No split over n, no dependence on the grid: update(A); update(B) is bit-equal
 *   to update(cat(A, B)) when A has a multiple of 4 rows.  Every element of sum is a sequential fp64 chain over the rows in
 *   order.  The upper 16x16 tiles are computed and mirrored: gram is written as a full, bit-symmetric matrix (and is read as
 *   one: the state is this entry point's own).  A non-finite x[r, c] reaches sum[c] and row and column c of gram, nothing
 *   else.  1 <= d <= SPK_FEATURE_MAX_D (SPK_ERR_UNSUPPORTED beyond), any n >= 0; n = 0 launches nothing.  Two launches.
 *
 * spk_poly_kernel_sums: X fp32 [n_x, d], Y fp32 [n_y, d] (contiguous); ix int32 [S, p] and iy int32 [S, q] DEVICE tables of
 *   row numbers (rows may repeat); a NULL ix / iy means rows 0 .. p - 1 / 0 .. q - 1 and needs S = 1.  For every subset s
 *     out[2 s]     = sum_{i < p, j < q} (gamma * <X[ix[s, i]], Y[iy[s, j]]> + coef)^degree
 *     out[2 s + 1] = sum_{i < min(p, q)} of the terms (i, i) when `symmetric` is set (the caller passes Y = X, iy = ix: the
 *                    diagonal of the Gram matrix), else 0.
 *   gamma_coef_host: HOST fp64 [2] = {gamma, coef}, read before the call returns (the binding passes no fp64 by value).
 *   v = gamma * dot + coef is one fp64 product and one sum; the power is r = v; r = r * v (degree - 1 times).  The dot product
 *   is a chain of fp64 MFMAs over d in steps of 4 from zero.  The p x q Gram matrix is never written: each 16x16 tile is
 *   raised to the power in registers and reduced (fixed butterfly) to one pair of fp64 partials in ws; a second launch adds each
 *   subset's partials in a fixed order.  A non-finite feature reaches the subsets that name its row and no other.  A table is
 *   device memory, so the host cannot check it: an entry outside [0, n) is the caller's error; the kernel reads no row for it
 *   and that subset's results are NaN.  (spkdiff.ops checks a table that is still on the host: ValueError.)
 *   ws: spk_poly_kernel_sums_ws_bytes(S, p, q) bytes (or the SPK_ERR_* code the call would return), 8-byte aligned, this call's
 *   alone while it is in flight; nothing is expected of its contents.  SPK_ERR_ARG: null X / Y / out / ws, S < 1, p < 1, q < 1,
 *   p > n_x or q > n_y without a table, a NULL table with S > 1, degree outside 1 .. SPK_POLY_KERNEL_MAX_DEGREE, a short ws;
 *   SPK_ERR_UNSUPPORTED: d outside 1 .. SPK_FEATURE_MAX_D, S > 65535 or 2^31 macro tiles and more. */
#define SPK_FEATURE_MAX_D 4096
#define SPK_POLY_KERNEL_MAX_DEGREE 8
int spk_feature_moments_acc(const float* x, long long n, int d, long long row_stride, double* sum_inout, double* gram_inout,
                            spk_stream_t stream);
long long spk_poly_kernel_sums_ws_bytes(int S, int p, int q);
int spk_poly_kernel_sums(const float* X, long long n_x, const float* Y, long long n_y, int d, const int* ix_or_null,
                         const int* iy_or_null, int S, int p, int q, const double* gamma_coef_host, int degree, int symmetric,
                         double* out, void* ws, long long ws_bytes, spk_stream_t stream);

/* ---- the plain-CNN VQVAE baseline, eval path (csrc/ann_vqvae.hip) ---------------------------------------------------- */
/* R/snn_model/vae_model.py:548-672 (main.py --model vq-vae).  fp32 products and accumulation (fmaf, one fixed order per
 * output), deterministic, image i's result independent of B; no allocation, no synchronisation, capturable in a hipGraph.
 * Weights in the reference modules' layouts: Conv2d [Cout,Cin,k,k], ConvTranspose2d [Cin,Cout,k,k]; codebook [K,D].
 * spk_ann_vqvae_supported: 1 for C in {1, 3}, H == W in {28, 32}, D == SPK_ANN_VQVAE_D and 2 <= K <= SPK_ANN_VQVAE_MAX_K, else
 * 0; the two entry points return SPK_ERR_UNSUPPORTED for every other shape.  A workgroup takes one image; a launch has at most
 * SPK_ANN_VQVAE_GRID_CAP workgroups, which loop over the images beyond that. */
#define SPK_ANN_VQVAE_D 16
#define SPK_ANN_VQVAE_MAX_K 1024
#define SPK_ANN_VQVAE_GRID_CAP 256
int spk_ann_vqvae_supported(int C, int H, int W, int D, int K);
/* CNN_Encoder + CNN_VectorQuantizer.get_code_indices (+ quantize) in ONE launch: images fp32 [B,C,H,W] -> idx_out int64
 * [B*h*w] (h = H / 4), z_out fp32 [B,D,h,w] (the encoder's output) or NULL, e_out fp32 [B,D,h,w] (the chosen codebook rows) or
 * NULL.  Conv 3x3 s2 p1 C->32 + ReLU (w1, b1), Conv 3x3 s2 p1 32->64 + ReLU (w2, b2), Conv 1x1 64->D (w3, b3); the
 * distances are fp64 on the fp32 z and the arg min is spk_vq_argmin's (first index on ties, a NaN row gives torch.argmin's
 * index, always in [0, K)). */
int spk_ann_vqvae_encode(const float* images, const float* w1, const float* b1, const float* w2, const float* b2,
                         const float* w3, const float* b3, const float* codebook, long long* idx_out, float* z_out_or_null,
                         float* e_out_or_null, int B, int C, int H, int W, int D, int K, spk_stream_t stream);
/* CNN_Decoder in two launches from tokens int64 [B,h,w] (the embedding gather folded in; a token outside [0, K) embeds as
 * NaN, as in spk_embedding_fwd, and reads nothing) or from e fp32 [B,D,h,w] -- exactly one of the two is non-NULL:
 * ConvT 3x3 s2 p1 op1 D->64 + ReLU (wt1, bt1), ConvT 3x3 s2 p1 op1 64->32 + ReLU (wt2, bt2), ConvT 3x3 s1 p1 32->C (wt3, bt3)
 * -> x_recon_out fp32 [B,C,H,W] and, unless NULL, u8_out = uint8(clip(x_recon + 0.5, 0, 1) * 255), truncated (R/main.py:400; a
 * NaN pixel gives 0).  ws: spk_ann_vqvae_decode_ws_bytes(B, H, W) bytes, 8-byte aligned, this call's alone while it is in
 * flight (the second layer's output; nothing is expected of its contents).  B <= 65535. */
long long spk_ann_vqvae_decode_ws_bytes(int B, int H, int W);
int spk_ann_vqvae_decode(const long long* tokens_or_null, const float* e_or_null, const float* codebook, const float* wt1,
                         const float* bt1, const float* wt2, const float* bt2, const float* wt3, const float* bt3, void* ws,
                         long long ws_bytes, float* x_recon_out, uint8_t* u8_out_or_null, int B, int C, int H, int W, int D,
                         int K, spk_stream_t stream);

/* ---- the plain-CNN VQVAE baseline, training (csrc/ann_vqvae_train.hip) -------------------------------------------------- */
/* Vector quantiser and loss of VQVAE.forward in train() mode (R/snn_model/vae_model.py:575-591, 660-672) on channels-last fp32
 * tensors; the convolutions are spk_conv_train_gather(_relu / _masked) and spk_conv_train_wgrad.  fp32 element-wise arithmetic in
 * the reference's order; the two mean squares are fp64 sums of a fixed shape that depends on the sizes only (per row / per
 * SPK_ANN_VQVAE_TRAIN_CHUNK elements, then one single-workgroup launch in index order): deterministic, independent of the grid.
 * No atomics, no state: ws is scratch (spk_ann_vqvae_train_ws_bytes(rows, elems) bytes, 8-byte aligned, this call's alone while it is
 * in flight), nothing is expected of its contents.  Capturable in a hipGraph; nothing is read back to the host.
 *
 * spk_ann_vqvae_train_vq_fwd: z fp32 [N,D] (the rows of Conv 1x1's channels-last output), codebook [K,D] -> idx_out int64 [N]
 *   (spk_vq_argmin's arithmetic and rule: what spk_ann_vqvae_encode chooses for the same z), e_out [N,D] = z + (q - z) with
 *   q = codebook[idx] (two fp32 roundings, the straight-through value), loss_out [1] = m + beta * m, m = mean((q - z)^2).
 *   D <= SPK_VQ_TRAIN_MAX_D and the codebook ((D + 1) floats and a double per code) within 64 KB of LDS:
 *   spk_ann_vqvae_train_supported(D, K); SPK_ERR_UNSUPPORTED beyond.  Two launches.
 * spk_ann_vqvae_train_vq_bwd: gz_out [N,D] = g_e + g_loss * beta * 2 (z - q) / (N D); gcodebook_out [K,D]: row k = g_loss * 2 / (N D) *
 *   sum over the rows with idx = k, in ascending row order, of (q - z) (fp64 sum; one workgroup per code; an unused code's row is
 *   zero).  g_e_or_null NULL = zero, g_loss_or_null [1] (device) NULL = zero.  One launch.
 * spk_ann_vqvae_train_loss_fwd: x_recon_cl fp32 [B,H,W,C], x_nchw fp32 [B,C,H,W] (the caller's image), data_variance [1] (device) ->
 *   real_out [1] = mse = mean((x_recon - x)^2), recon_out [1] = mse / data_variance.  Two launches.
 * spk_ann_vqvae_train_loss_bwd: gx_recon_cl [B,H,W,C] = s * 2 (x_recon - x) / n with s = g_recon / data_variance + g_real (device
 *   scalars, NULL = zero).  One launch. */
#define SPK_ANN_VQVAE_TRAIN_CHUNK 2048
/* 1 where spk_ann_vqvae_train_vq_fwd takes embedding_dim D and K codes (host-only; D = 16: K <= 862), else 0. */
int spk_ann_vqvae_train_supported(int D, int K);
long long spk_ann_vqvae_train_ws_bytes(long long rows, long long elems);
int spk_ann_vqvae_train_vq_fwd(const float* z, const float* codebook, long long* idx_out, float* e_out, float* loss_out, float beta,
                               void* ws, long long ws_bytes, long long N, int D, int K, spk_stream_t stream);
int spk_ann_vqvae_train_vq_bwd(const float* g_e_or_null, const float* g_loss_or_null, const float* z, const long long* idx,
                               const float* codebook, float beta, float* gz_out, float* gcodebook_out, long long N, int D, int K,
                               spk_stream_t stream);
int spk_ann_vqvae_train_loss_fwd(const float* x_recon_cl, const float* x_nchw, const float* data_variance, float* recon_out,
                                 float* real_out, void* ws, long long ws_bytes, int B, int C, int H, int W, spk_stream_t stream);
int spk_ann_vqvae_train_loss_bwd(const float* x_recon_cl, const float* x_nchw, const float* g_recon_or_null,
                                 const float* g_real_or_null, const float* data_variance, float* gx_recon_cl, int B, int C, int H,
                                 int W, spk_stream_t stream);

/* ---- measurement aid ------------------------------------------------------------------------------------------ */
/* Shader clock this device holds under a block-scaled fp6 x fp4 MFMA load (bench.py records it next to every
 * matrix-core number: devices of one pool differ by ~10 %).  nblocks workgroups of 256 threads issue 4*iters MFMAs per
 * wave between two {s_memtime, s_memrealtime} stamps; out [nblocks][4] u64 = {shader cycles, 100 MHz ticks, MFMAs
 * per wave, 0}.  No counterpart in the reference (it has no timing hooks on this path). */
int spk_clock_probe(unsigned long long* out, int nblocks, int iters, spk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SPKDIFF_H */
