/*
 * cmgan_hip.h - C ABI of libcmgan_hip.so: the CMGAN generator forward path
 * (waveform -> STFT -> power-compress -> TSCNet -> power-uncompress -> ISTFT)
 * as hand-written HIP kernels for MI355X (gfx950 / CDNA4).
 *
 * The reference (ruizhecao96/CMGAN) is pure Python and has no operator / FFI
 * boundary; the seam this library sits behind is the Python module boundary
 * (SURVEY.md section 8b).  Each entry point cites the reference code it replaces
 * (paths relative to the reference tree).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - plain C types only; every pointer named *_dev is a device pointer owned by
 *    the caller (e.g. torch.Tensor.data_ptr()); fp32 everywhere.
 *  - every call returns 0 (CMGAN_OK) or a negative CMGAN_E_* code; the message is
 *    available from cmgan_last_error().  Nothing throws across the ABI.
 *  - all kernels are enqueued on the caller's `stream` (a hipStream_t passed as
 *    void*; NULL = the legacy default stream) and return without synchronising.
 *    No allocation, free or synchronisation happens inside forward calls, so they
 *    can be captured into a hipGraph.
 *  - a handle is bound to the device that was current at cmgan_create() and is
 *    not re-entrant; use one handle per GPU / per process.
 */
#ifndef CMGAN_HIP_H
#define CMGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMGAN_OK             0
#define CMGAN_E_BADARG      -1   /* null pointer / non-positive size               */
#define CMGAN_E_BADSHAPE    -2   /* shape incompatible with the handle's config    */
#define CMGAN_E_UNSUPPORTED -3   /* config outside what the kernels are built for  */
#define CMGAN_E_WEIGHTS     -4   /* blob malformed / tensor missing / wrong size   */
#define CMGAN_E_WORKSPACE   -5   /* workspace too small or misaligned              */
#define CMGAN_E_HIP         -6   /* a HIP runtime call failed (see last_error)     */

#define CMGAN_ABI_VERSION 23

typedef struct cmgan_handle cmgan_handle;

/* Hyper-parameters that are constructor arguments or literals in the reference:
 * TSCNet(num_channel=64, num_features=n_fft/2+1)  src/models/generator.py:160-172
 * n_fft=400, hop=100                               src/evaluation.py:62,78
 * heads=4, dim_head=16, conv kernel 31             src/models/generator.py:75-90
 * max_pos_emb=512                                  src/models/conformer.py:76      */
typedef struct cmgan_config {
    int32_t n_fft;         /* 400 (16 kHz) or 1200 (48 kHz); multiple of 16.  Also
                            * bounded by the device's LDS per block: cmgan_create
                            * returns CMGAN_E_UNSUPPORTED when the dense DFT kernels
                            * would need more than it, (15 hop + n_fft) x 4 B forward
                            * or 16 (32 ceil(F / 16) + 4) x 4 B inverse; at the
                            * MI355X's 160 KiB that is n_fft <= 2512                */
    int32_t hop;           /* 100 / 300; multiple of 4, must divide n_fft           */
    int32_t num_features;  /* F = n_fft/2 + 1                                       */
    int32_t num_channel;   /* 64 (the only value the kernels are specialised for)   */
    int32_t num_tscb;      /* 4                                                     */
    int32_t heads;         /* 4                                                     */
    int32_t dim_head;      /* 16                                                    */
    int32_t conv_kernel;   /* 31                                                    */
    int32_t max_pos_emb;   /* 512                                                   */
    int32_t mfma_mode;     /* CMGAN_MFMA_F32, CMGAN_MFMA_F16X3 (default), _F16X1 or _F16MIX */
    int32_t single_mask;   /* CMGAN_MFMA_F16MIX only: CMGAN_MIX_* bits = the kernel families that run ONE fp16 product */
} cmgan_config;

/* How the dense contractions (convs, linears, attention) are evaluated.  Three modes; all keep fp32 storage and
 * fp32 accumulation.  The first two are fp32-class and meet the 1e-3 parity gate by >2 decades; the third (F16X1,
 * below) is an opt-in reduced-precision mode that sits inside the gate without margin:
 *   F32   : v_mfma_f32_16x16x4_f32, bit-exact fp32 products (157 TF peak)
 *   F16X3 : every operand split x = hi + lo in fp16 and the product evaluated as
 *           hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16 (~2^-21 relative product error,
 *           ~5x the fp32 matrix rate; gfx950 has no TF32).  At n_fft 400 / hop 100 the STFT / ISTFT
 *           use folded split-f16 DFT kernels too; other sizes (48 kHz: 1200 / 300) run the
 *           dense fp32 DFT kernels in either mode.                                          */
#define CMGAN_MFMA_F32   0
#define CMGAN_MFMA_F16X3 1
/* F16X1 - REDUCED precision, opt-in, never the default: the TSCNet body (dense convs, conformers) on ONE fp16 product
 * per contraction (operands rounded to nearest fp16, fp32 accumulation): the "half-precision" throughput mode
 * BASELINE configs[1] names (fp16 carries 3 more mantissa bits than bf16).  ~1.3x the F16X3 rate; error vs the fp32
 * reference 6e-4 .. 9e-4 of the peak on synthetic clips and real recordings alike
 * (tests/test_gpu_parity.py::test_f16x1_mode_error_bands pins the measured bands): inside the 1e-3 gate without
 * margin, 200x the error of the other two modes - not fp32-class.  STFT / ISTFT run as in F16X3 (|X|^-0.7 on
 * near-silent bins is what a single-product front end gets wrong by several 1e-2). */
#define CMGAN_MFMA_F16X1 2
/* F16MIX - REDUCED precision, opt-in: the F16X3 library with the kernel families named in cmgan_config.single_mask
 * switched to their single-product (F16X1) build, every other family on three split products.  What each family
 * costs in accuracy when it alone is single is tabulated in DESIGN.md (tools/mix_ablation.py); the shipped "f16mix"
 * preset of the Python host (cmgan_amd.engine.F16MIX_PRESET) takes every family whose own contribution stays below
 * 1e-4 of the peak, for an end-to-end error <= 2e-4 (5 x margin to the 1e-3 gate, asserted two-sidedly by
 * tests/test_gpu_parity.py::test_f16mix_mode_error_band).  single_mask = 0 is F16X3, all bits = F16X1.            */
#define CMGAN_MFMA_F16MIX 3
#define CMGAN_MIX_CONV   1    /* dilated dense convs, conv_2, sub-pixel convs   src/models/generator.py:39-47,60,107-118 */
#define CMGAN_MIX_FF1    2    /* ff1 (LN -> W1 -> Swish -> W2)                  src/models/conformer.py:136-148, 216     */
#define CMGAN_MIX_FF2    4    /* ff2 + post norm                                src/models/conformer.py:220-221          */
#define CMGAN_MIX_QKV    8    /* LN -> to_q / to_kv                             src/models/conformer.py:100-101          */
#define CMGAN_MIX_ATTN  16    /* q k^T, q E^T, P V, to_out                      src/models/conformer.py:103-133          */
#define CMGAN_MIX_PW1   32    /* conv module: LN -> pointwise 64 -> 256 -> GLU  src/models/conformer.py:161-164          */
#define CMGAN_MIX_DWPW2 64    /* depthwise k = 31 -> Swish -> pointwise 128 -> 64   src/models/conformer.py:165-170      */
#define CMGAN_MIX_ALL  127
/* Plane widths and conv kernels.  In the three split-f16 modes the encoder / decoder convs run on the f16 matrix pipe only
 * where the plane is wide enough for that kernel's row walk (conv_x3.hip, conv3x_walkable); a narrower plane takes the
 * fp32 conv kernel of the F32 mode, conv by conv, with the same weights.  F = n_fft / 2 + 1, F' = (F + 1) / 2:
 *   encoder dense block, conv_2   (plane F)    split-f16 for F  >= 63 (n_fft >= 124), else fp32
 *   decoder dense blocks          (plane F')   split-f16 for F' >= 63 (n_fft >= 248), else fp32
 *   complex decoder sub-pixel conv (plane F')  split-f16 for F' >= 31 (n_fft >= 120), else fp32
 * The conformers, conv_1, the mask head and the tails do not depend on the width.  The default 16 kHz (F 201 / F' 101)
 * and 48 kHz (601 / 301) models are far above every limit; small n_fft is at least as accurate as before, not faster. */

/* Fills *cfg with the reference's 16 kHz defaults (above). */
void cmgan_default_config(cmgan_config* cfg);

int  cmgan_abi_version(void);

/* Creates a handle on the current device; builds the window / DFT tables
 * (replaces the torch.hamming_window + cuFFT plan of src/evaluation.py:36-38,44-50). */
int  cmgan_create(cmgan_handle** out, const cmgan_config* cfg);
void cmgan_destroy(cmgan_handle* h);

/* Last error message for this handle (or for a failed cmgan_create when h == NULL). */
const char* cmgan_last_error(const cmgan_handle* h);

/* Uploads packed weights.  `blob` is the host buffer produced by
 * cmgan_amd.packer.pack_state_dict() from the reference generator state_dict
 * (the 359-entry dict loaded at src/evaluation.py:63-64).  Layout: see
 * cmgan_amd/csrc/weights.h.  May be called again to swap weights (synchronises the
 * device).  The swap is atomic: on any failure the previously loaded weights stay in
 * place.  Device buffers are re-allocated, so hipGraphs captured before the call hold
 * stale pointers: re-capture when cmgan_weights_generation() has changed.          */
int  cmgan_load_weights(cmgan_handle* h, const void* blob, size_t bytes);
/* Number of successful cmgan_load_weights calls on this handle (-1 for NULL).      */
int  cmgan_weights_generation(const cmgan_handle* h);

/* Bytes of scratch the forward calls need for a batch of B spectrograms of T
 * frames (0 on bad arguments).  The caller allocates it once (256-byte aligned). */
size_t cmgan_workspace_bytes(const cmgan_handle* h, int B, int T);

/* c[b] = sqrt(L / sum_l wav[b,l]^2)            src/evaluation.py:21, src/train.py:75-79 */
int cmgan_rms_scale(cmgan_handle* h, const float* wav_dev, int B, int L,
                    float* scale_dev, void* stream);

/* Frames of an L-sample row: L / hop + 1 (torch.stft, center=True). */
int cmgan_num_frames(const cmgan_handle* h, int L);

/* wav[B,L] (optionally scaled by scale_dev[B]; NULL = 1) -> power-compressed
 * spectrogram spec[B,2,T,F] = the tensor fed to TSCNet.forward.
 * Replaces torch.stft + utils.power_compress + permute
 * (src/evaluation.py:36-39, src/utils.py:20-29).  Any L > n_fft/2 (reflect padding):
 * T = L / hop + 1 frames, exactly torch.stft(center=True).                      */
int cmgan_stft_compress(cmgan_handle* h, const float* wav_dev, const float* scale_dev,
                        int B, int L, float* spec_dev, void* stream);

/* TSCNet.forward (src/models/generator.py:174-196):
 * spec[B,2,T,F] -> out_real[B,1,T,F], out_imag[B,1,T,F].                       */
int cmgan_tscnet_forward(cmgan_handle* h, const float* spec_dev, int B, int T,
                         float* out_real_dev, float* out_imag_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* The mask decoder's head on its own (tests).  The forward evaluates sub_pixel (1,3) conv 64 -> 128, the pixel shuffle
 * and conv_1 (1,2) 64 -> 1 (src/models/generator.py:133-136, no non-linearity in between) as ONE linear map whose
 * weights cmgan_load_weights derives in double and rounds once to fp32:
 *   G[k][ci][r][kf] = sum_c conv_1.weight[0][c][0][kf] * sub_pixel.conv.weight[r * 64 + c][ci][0][k]
 *   g0[r][kf]       = sum_c conv_1.weight[0][c][0][kf] * sub_pixel.conv.bias[r * 64 + c]
 * cmgan_mask_head_weights copies them to HOST memory: out776 = G [3][64][2][2] then g0 as [2][4] (entries 2, 3 of a
 * row are zero).  cmgan_mask_head_forward runs the kernel on caller tensors with the handle's weights:
 * y [B, T, Fe, 64] = the mask dense block's last raw output, scale / shift [B][64] = its InstanceNorm as a per-clip
 * affine pair; with v = PReLU(scale * y + shift) (dense block prelu 4), zero outside [0, Fe),
 *   dm[((b * T + t) * 2Fe + 2f + r) * 4 + kf] = g0[r][kf] + sum_k sum_ci G[k][ci][r][kf] * v[b, t, f + k - 1, ci]
 * for kf = 0, 1 and 0 for kf = 2, 3; dm holds B * T * 2Fe * 4 floats.  B, T, Fe >= 1, B * T * Fe < 2^31.            */
int cmgan_mask_head_weights(cmgan_handle* h, float* out776);
int cmgan_mask_head_forward(cmgan_handle* h, const float* y_dev, const float* scale_dev, const float* shift_dev,
                            int B, int T, int Fe, float* dm_dev, void* stream);

/* est_real/est_imag [B,1,T,F] -> waveform wav_out[B, hop*(T-1)], divided by
 * scale_dev[B] when it is not NULL.  Replaces permute + utils.power_uncompress +
 * torch.istft + '/ c'  (src/evaluation.py:41-51, src/utils.py:32-39).          */
int cmgan_uncompress_istft(cmgan_handle* h, const float* real_dev, const float* imag_dev,
                           const float* scale_dev, int B, int T, float* wav_out_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* The whole device pipeline of enhance_one_track (src/evaluation.py:21-51) for a
 * batch of equal-length rows: per-row RMS scale, STFT, TSCNet, ISTFT, un-scale.
 * wav[B,L] -> wav_out[B,L];  L % hop == 0.                                      */
int cmgan_enhance(cmgan_handle* h, const float* wav_dev, int B, int L, float* wav_out_dev,
                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* cmgan_enhance as `branches` (1..8) part-batch branches: rows split evenly, branch 0 on `stream`,
 * the others on streams the handle owns, forked and joined with events so that a stream capture
 * of `stream` records them as parallel paths of one hipGraph.  Branch i + 1 starts once branch i
 * has issued `offset_launches` kernels (0 = all together).  Utterances are independent in eval
 * mode (src/models/generator.py:35, src/models/conformer.py:168; src/evaluation.py:30-34 batches
 * rows the same way) and each branch runs the unchanged per-row arithmetic: the result equals
 * cmgan_enhance bit for bit.  Workspace: cmgan_workspace_bytes_branched(B, T, branches).
 * The first call creates the side streams and events - make it outside a capture.            */
size_t cmgan_workspace_bytes_branched(const cmgan_handle* h, int B, int T, int branches);
int cmgan_enhance_branched(cmgan_handle* h, const float* wav_dev, int B, int L, float* wav_out_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream,
                           int branches, int offset_launches);

/* The non-adversarial terms of Trainer.calculate_generator_loss (src/train.py:124-151)
 * as deterministic device reductions, out4_dev = {loss_ri, loss_mag, time_loss, time_mse}:
 *   loss_ri   = mse(est_real, clean_real) + mse(est_imag, clean_imag)      train.py:135-137
 *   loss_mag  = mse(|est|, |clean|)                                         train.py:132-134
 *   time_loss = mean |est_audio - clean_audio|                              train.py:139-141
 *   time_mse  = mean (est_audio - clean_audio)^2   (logging only, not in the reference)
 * est_real/est_imag [B,1,T,F] are the TSCNet outputs, clean_spec [B,2,T,F] the
 * power-compressed clean spectrogram in the model layout (cmgan_stft_compress of the
 * clean rows; the reference's permutes do not change an elementwise mean), est/clean
 * audio [B,L_audio].  Either group may be all-NULL (its terms are then 0).  These are
 * the per-rank scalars the data-parallel step all-reduces (one RCCL call).          */
int cmgan_loss_terms(cmgan_handle* h, const float* est_real_dev, const float* est_imag_dev,
                     const float* clean_spec_dev, int B, int T, const float* est_audio_dev,
                     const float* clean_audio_dev, int L_audio, float* out4_dev, void* stream);

/* Training-mode FeedForward branch of a ConformerBlock with its backward - the first slice of the training
 * step:  y = Scale(0.5, PreNorm(64, FeedForward(64, mult=4, dropout)))(x)
 *                         = 0.5 * m2 * (W2 (m1 * Swish(W1 LayerNorm(x) + b1)) + b2)
 * (src/models/conformer.py:54-72, 136-148, 211-212).  The residual add of :216/:219 is fused on request:
 * residual_dev [M,64] (NULL = none) is added to y in the final store, dresidual_dev [M,64] (NULL = none; usually dy
 * itself) to dx, so that `x = ff(x) + x` and its backward cost no extra pass over the sequence.  The same pair of
 * optional pointers exists on the conv-module and attention entry points below.
 * Parameters are the RAW tensors of the reference state_dict for one ff{1,2} branch (row-major, device):
 *   ln_weight/ln_bias [64] = ff.fn.norm.{weight,bias};  w1 [256,64], b1 [256] = ff.fn.fn.net.0;
 *   w2 [64,256], b2 [64] = ff.fn.fn.net.3.
 * x, y, dy, dx are [M,64].  mask1 [M,256] / mask2 [M,64] are the keep-masks of the two nn.Dropout layers as BYTES
 * (non-zero = keep; a kept value is multiplied by mask_scale = 1/(1-p)); NULL = no dropout (p = 0 or eval) - bytes
 * because the masks are the largest per-token traffic of the step.  The backward recomputes the hidden activations from x,
 * writes dL/dx to dx and dL/dparam to the six tensors of *grads (overwritten, not accumulated), with
 * fixed-order reductions (bit-reproducible).  Workspace: cmgan_ffn_train_workspace_bytes(h, M).            */
typedef struct cmgan_ffn_params {
    float *ln_weight, *ln_bias, *w1, *b1, *w2, *b2;
} cmgan_ffn_params;
size_t cmgan_ffn_train_workspace_bytes(const cmgan_handle* h, long long M);
int cmgan_ffn_train_forward(cmgan_handle* h, const float* x_dev, long long M, const cmgan_ffn_params* params,
                            const unsigned char* mask1_dev, const unsigned char* mask2_dev, float mask_scale,
                            const float* residual_dev, float* y_dev, void* workspace_dev, size_t workspace_bytes,
                            void* stream);
int cmgan_ffn_train_backward(cmgan_handle* h, const float* x_dev, const float* dy_dev, long long M,
                             const cmgan_ffn_params* params, const unsigned char* mask1_dev,
                             const unsigned char* mask2_dev, float mask_scale, const float* dresidual_dev,
                             float* dx_dev, const cmgan_ffn_params* grads,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/* Training-mode ConformerConvModule with its backward - second slice of the training step:
 *   y = Conv1d(128,64,1)(Swish(BatchNorm1d(DepthWiseConv1d_31(GLU(Conv1d(64,256,1)(LayerNorm(x)))))))
 * (src/models/conformer.py:151-176; residual_dev / dresidual_dev fuse the residual add of :218; the module's Dropout has
 * p = conv_dropout = 0).  TRAIN semantics: BatchNorm1d normalises with the statistics of this batch (biased
 * variance over all N*L positions, eps 1e-5) and updates running_mean / running_var in place (momentum 0.1, unbiased
 * variance) when both pointers are non-NULL.  x, y, dy, dx: contiguous sequences [N, L, 64].  Parameters are the
 * RAW tensors of the reference state_dict (conv.net.{0,2,4.conv,5,7}.{weight,bias}; the [256,64,1], [128,1,31] and
 * [64,128,1] conv weights are used as [256,64], [128,31], [64,128]).  The forward keeps its GLU output, depthwise
 * output and batch statistics in the workspace; the backward must be given the SAME workspace, untouched in
 * between, and writes dL/dx and the ten parameter gradients (overwritten, fixed-order reductions).               */
typedef struct cmgan_convmod_params {
    float *ln_weight, *ln_bias, *pw1_weight, *pw1_bias, *dw_weight, *dw_bias, *bn_weight, *bn_bias,
          *pw2_weight, *pw2_bias;
} cmgan_convmod_params;
size_t cmgan_convmod_train_workspace_bytes(const cmgan_handle* h, int N, int L);
int cmgan_convmod_train_forward(cmgan_handle* h, const float* x_dev, int N, int L, const cmgan_convmod_params* params,
                                float* running_mean_dev, float* running_var_dev, const float* residual_dev,
                                float* y_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int cmgan_convmod_train_backward(cmgan_handle* h, const float* x_dev, const float* dy_dev, int N, int L,
                                 const cmgan_convmod_params* params, const float* dresidual_dev, float* dx_dev,
                                 const cmgan_convmod_params* grads,
                                 void* workspace_dev, size_t workspace_bytes, void* stream);

/* Training-mode PreNorm(Attention) with its backward - third slice of the training step:
 *   y = mask * to_out(softmax((q k^T + q E[clamp(i - j, +-max_pos)]^T) / 4) v),  q = to_q(LN(x)), k|v = to_kv(LN(x))
 * (src/models/conformer.py:54-72, 75-133; 4 heads of 16; residual_dev / dresidual_dev fuse the residual add of :217).  `mask`
 * [N,L,64] is the byte keep-mask (non-zero = keep, kept values x mask_scale) of the nn.Dropout on the to_out output
 * (conformer.py:133; NULL = none).  Parameters are
 * the RAW tensors attn.norm.{weight,bias}, attn.fn.to_q.weight [64,64], attn.fn.to_kv.weight [128,64],
 * attn.fn.to_out.{weight [64,64], bias}, attn.fn.rel_pos_emb.weight [2 max_pos + 1, 16].  L <= 4096
 * (CMGAN_E_UNSUPPORTED beyond; distances past +-max_pos share the table's end rows, as in the reference).  The forward keeps q|k|v, the attention output and the row log-sum-exp in the
 * workspace; the backward needs the SAME workspace untouched and writes dL/dx and the seven parameter gradients
 * (the embedding-table gradient is dense [2 max_pos + 1, 16], rows of unused distances are zero).                 */
typedef struct cmgan_attn_params {
    float *ln_weight, *ln_bias, *to_q_weight, *to_kv_weight, *to_out_weight, *to_out_bias, *rel_pos_emb;
} cmgan_attn_params;
size_t cmgan_attn_train_workspace_bytes(const cmgan_handle* h, int N, int L);
int cmgan_attn_train_forward(cmgan_handle* h, const float* x_dev, int N, int L, const cmgan_attn_params* params,
                             const unsigned char* mask_dev, float mask_scale, const float* residual_dev,
                             float* y_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int cmgan_attn_train_backward(cmgan_handle* h, const float* x_dev, const float* dy_dev, int N, int L,
                              const cmgan_attn_params* params, const unsigned char* mask_dev, float mask_scale,
                              const float* dresidual_dev, float* dx_dev, const cmgan_attn_params* grads,
                              void* workspace_dev, size_t workspace_bytes, void* stream);

/* Glue of ConformerBlock.forward in train mode (src/models/conformer.py:216-222): out = a + b over n floats (the
 * residual adds; n % 4 == 0), and the closing post_norm = nn.LayerNorm(64) (eps 1e-5) on [M,64] rows with its backward
 * (dL/dx, dL/dweight, dL/dbias; fixed-order reductions).                                                          */
/* in [B, A, C, 64] -> out [B, C, A, 64] (out != in): the time-axis <-> frequency-axis layout flip of a TSCB on
 * channels-last activations (src/models/generator.py:94,96 permute + contiguous).  add_dev (optional, laid out like
 * in_dev; NULL = none) is summed in before the flip: out = flip(in + add), which carries the residual add of
 * generator.py:95 (and of the backward) without a pass of its own.  cmgan_layernorm_train_forward's residual_dev
 * [M,64] (NULL = none) does the same for generator.py:97: y = LayerNorm(x) + residual.                            */
int cmgan_swap_axes(cmgan_handle* h, const float* in_dev, const float* add_dev, float* out_dev, int B, int A, int C,
                    void* stream);
int cmgan_add(cmgan_handle* h, const float* a_dev, const float* b_dev, float* out_dev, long long n, void* stream);
/* Keep-masks of nn.Dropout(p) layers (src/models/conformer.py:64,70,98,172) as bytes, 1 = keep with probability
 * keep_prob = 1 - p (compared at 16-bit resolution), for the mask_dev arguments of the training functions above: the
 * reference draws them inside F.dropout with torch's Philox stream, here one launch fills ALL masks of a step.
 * state_dev: two 64-bit words in device memory {seed, offset}; Philox4x32-10 counters offset .. offset + nbytes / 16 are
 * consumed and the offset is advanced on the device, so the call is replayable inside a captured graph.  nbytes must be
 * a positive multiple of 16.                                                                                        */
int cmgan_dropout_masks(cmgan_handle* h, unsigned char* masks_dev, long long nbytes, float keep_prob,
                        unsigned long long* state_dev, void* stream);
size_t cmgan_layernorm_train_workspace_bytes(const cmgan_handle* h, long long M);
int cmgan_layernorm_train_forward(cmgan_handle* h, const float* x_dev, long long M, const float* weight_dev,
                                  const float* bias_dev, const float* residual_dev, float* y_dev, void* stream);
int cmgan_layernorm_train_backward(cmgan_handle* h, const float* x_dev, const float* dy_dev, long long M,
                                   const float* weight_dev, const float* bias_dev, float* dx_dev,
                                   float* dweight_dev, float* dbias_dev,
                                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* Training-mode DilatedDenseNet with its backward - fourth slice of the training step:
 * four layers of  pad(top = 2^i, l/r = 1) -> Conv2d(64 (i+1) -> 64, (2,3), dilation (2^i, 1)) -> InstanceNorm2d(affine)
 * -> PReLU(64) -> cat([out, skip]) (newest first), returning the last layer's output (src/models/generator.py:6-47;
 * used by the encoder and both decoders).  Activations are channels-last [B, T, F, 64] (the reference's NCHW tensor
 * is x.permute(0, 2, 3, 1)).  Parameters are the RAW tensors conv{i}.weight [64, 64 i, 2, 3], conv{i}.bias,
 * norm{i}.weight/bias, prelu{i}.weight for i = 1..4 (index i-1 below).  The forward keeps the layer outputs, the raw
 * conv outputs and the InstanceNorm statistics in the workspace; the backward needs the SAME workspace untouched and
 * writes dL/dx and the twenty parameter gradients (the conv biases sit in front of an InstanceNorm, so their
 * gradients are zero up to rounding).  dx_dev is accumulated in place while the backward runs: it must not alias
 * x_dev or dy_dev (dy_dev is read, never written).                                                               */
typedef struct cmgan_dense_params {
    float *conv_weight[4], *conv_bias[4], *norm_weight[4], *norm_bias[4], *prelu_weight[4];
} cmgan_dense_params;
size_t cmgan_dense_train_workspace_bytes(const cmgan_handle* h, int B, int T, int F);
int cmgan_dense_train_forward(cmgan_handle* h, const float* x_dev, int B, int T, int F,
                              const cmgan_dense_params* params, float* y_dev,
                              void* workspace_dev, size_t workspace_bytes, void* stream);
int cmgan_dense_train_backward(cmgan_handle* h, const float* x_dev, const float* dy_dev, int B, int T, int F,
                               const cmgan_dense_params* params, float* dx_dev, const cmgan_dense_params* grads,
                               void* workspace_dev, size_t workspace_bytes, void* stream);

/* Training-mode DenseEncoder with its backward (src/models/generator.py:50-69): conv_1 (1x1, 3 -> 64) +
 * InstanceNorm2d(affine) + PReLU(64), the DilatedDenseNet above, conv_2 ((1,3), stride (1,2), padding (0,1)) +
 * InstanceNorm2d(affine) + PReLU(64).  xin [B,T,F,3] is the channels-last x_in of TSCNet.forward
 * (cmgan_tscnet_prologue); y [B,T,F',64] with F' = (F - 1) / 2 + 1.  x_in carries no gradient, so the backward only
 * writes the thirty parameter gradients.  Same workspace contract as the dense block.                            */
typedef struct cmgan_encoder_params {
    float *conv1_weight, *conv1_bias, *norm1_weight, *norm1_bias, *prelu1_weight;   /* conv_1.{0.weight [64,3,1,1], 0.bias, 1.weight, 1.bias, 2.weight} */
    cmgan_dense_params dense;                                                       /* dilated_dense.* */
    float *conv2_weight, *conv2_bias, *norm2_weight, *norm2_bias, *prelu2_weight;   /* conv_2.{0.weight [64,64,1,3], ...} */
} cmgan_encoder_params;
size_t cmgan_encoder_train_workspace_bytes(const cmgan_handle* h, int B, int T, int F);
int cmgan_encoder_train_forward(cmgan_handle* h, const float* xin_dev, int B, int T, int F,
                                const cmgan_encoder_params* params, float* y_dev,
                                void* workspace_dev, size_t workspace_bytes, void* stream);
int cmgan_encoder_train_backward(cmgan_handle* h, const float* xin_dev, const float* dy_dev, int B, int T, int F,
                                 const cmgan_encoder_params* params, const cmgan_encoder_params* grads,
                                 void* workspace_dev, size_t workspace_bytes, void* stream);

/* Training-mode MaskDecoder (kind CMGAN_DECODER_MASK, generator.py:121-138) and ComplexDecoder (kind
 * CMGAN_DECODER_COMPLEX, generator.py:141-156) with their backward.  Both: DilatedDenseNet -> SPConvTranspose2d
 * (pad 1/1, Conv2d(64 -> 128, (1,3)), pixel shuffle x2 along frequency, generator.py:102-119) -> head.
 *   mask head:    conv_1 (1,2) 64 -> 1, InstanceNorm2d(1, affine), PReLU(1), final_conv 1x1, PReLU(num_features);
 *                 out [B,T,F] (= the reference's [B,1,T,F])
 *   complex head: InstanceNorm2d(64, affine), PReLU(64), conv (1,2) 64 -> 2;  out [B,T,F,2] (reference: [B,2,T,F])
 * x [B,T,Fe,64] channels-last, F = 2 Fe - 1.  final_* / prelu_out_weight are ignored for the complex head.        */
enum { CMGAN_DECODER_MASK = 0, CMGAN_DECODER_COMPLEX = 1 };
typedef struct cmgan_decoder_params {
    cmgan_dense_params dense;                         /* dense_block.* */
    float *sub_pixel_weight, *sub_pixel_bias;         /* sub_pixel.conv.{weight [128,64,1,3], bias [128]} */
    float *conv_weight, *conv_bias;                   /* conv_1 (mask) / conv (complex): [NO,64,1,2], [NO] */
    float *norm_weight, *norm_bias, *prelu_weight;    /* norm.{weight,bias}, prelu.weight: [1] (mask) or [64] */
    float *final_weight, *final_bias;                 /* mask only: final_conv.{weight [1,1,1,1], bias [1]} */
    float *prelu_out_weight;                          /* mask only: prelu_out.weight [num_features] */
} cmgan_decoder_params;
size_t cmgan_decoder_train_workspace_bytes(const cmgan_handle* h, int B, int T, int Fe);
int cmgan_decoder_train_forward(cmgan_handle* h, int kind, const float* x_dev, int B, int T, int Fe,
                                const cmgan_decoder_params* params, float* out_dev,
                                void* workspace_dev, size_t workspace_bytes, void* stream);
int cmgan_decoder_train_backward(cmgan_handle* h, int kind, const float* x_dev, const float* dout_dev, int B, int T,
                                 int Fe, const cmgan_decoder_params* params, float* dx_dev,
                                 const cmgan_decoder_params* grads,
                                 void* workspace_dev, size_t workspace_bytes, void* stream);

/* The glue of TSCNet.forward (generator.py:176-201) for the training step, F = num_features of the handle:
 *   prologue:  spec [B,2,T,F] -> xin [B,T,F,3] = (|spec|, re, im)                       generator.py:177-181
 *   epilogue:  est = mask * |spec| * (cos, sin)(angle spec) + complex_out = mask * spec + complex_out
 *              (mask [B,T,F], complex_out [B,T,F,2] -> est_real, est_imag [B,T,F])      generator.py:188-199
 *   backward:  dmask = d_real re + d_imag im,  dcomplex = (d_real, d_imag); the noisy spectrogram is data.       */
int cmgan_tscnet_prologue(cmgan_handle* h, const float* spec_dev, int B, int T, float* xin_dev, void* stream);
int cmgan_tscnet_epilogue_forward(cmgan_handle* h, const float* spec_dev, const float* mask_dev,
                                  const float* complex_dev, int B, int T, float* est_real_dev, float* est_imag_dev,
                                  void* stream);
int cmgan_tscnet_epilogue_backward(cmgan_handle* h, const float* spec_dev, const float* d_real_dev,
                                   const float* d_imag_dev, int B, int T, float* dmask_dev, float* dcomplex_dev,
                                   void* stream);

/* Gradient of  w_ri * loss_ri + w_mag * loss_mag + w_time * time_loss  (the non-adversarial part of
 * Trainer.calculate_generator_loss, src/train.py:133-148; same arguments as cmgan_loss_terms) with respect to
 * est_real / est_imag [B,T,F].  The time term runs the adjoint of torch.istft (window, overlap-add, envelope
 * division, centre trim; train.py:106-112) and of utils.power_uncompress (utils.py:32-39) in one kernel; est_audio /
 * clean_audio [B, hop (T-1)] may both be NULL when w_time = 0.  n_fft / hop / F are the handle's.                 */
int cmgan_loss_backward(cmgan_handle* h, const float* est_real_dev, const float* est_imag_dev,
                        const float* clean_spec_dev, int B, int T, const float* est_audio_dev,
                        const float* clean_audio_dev, float w_ri, float w_mag, float w_time,
                        float* d_real_dev, float* d_imag_dev, void* stream);

/* The metric discriminator Discriminator(ndf=16) of the reference trainer (src/models/discriminator.py:29-64) with its
 * backward: four spectral-norm Conv2d(4x4, stride 2, pad 1, no bias) + InstanceNorm2d(affine) + PReLU stages
 * (2 -> 16 -> 32 -> 64 -> 128), global max pool, spectral-norm Linear(128,64), Dropout(0.3), PReLU(64), spectral-norm
 * Linear(64,1), LearnableSigmoid(1).  Parameters are the RAW state_dict tensors (weight_orig + the power-iteration
 * buffers weight_u / weight_v of torch.nn.utils.spectral_norm).  xy [B,T,F,2] = (|clean|, |est|) channels-last is the
 * reference's cat([clean_mag, est_mag], 1) [B,2,F,T] (cmgan_mag_pair builds it from the model-layout tensors);
 * T, F >= 16.  update_uv != 0 is train mode: one power iteration per spectral norm before use, written back to the
 * u / v buffers; mask [B,64] is the Dropout keep-mask (0 or 1/0.7) or NULL.  The backward needs the forward's workspace
 * untouched (it holds the u, v, sigma that forward used), writes dL/dxy when dxy is not NULL and the 22 parameter
 * gradients (the u / v fields of `grads` are ignored).                                                            */
typedef struct cmgan_disc_params {
    float *conv_weight_orig[4], *conv_u[4], *conv_v[4];   /* layers.{0,3,6,9}.weight_orig / weight_u / weight_v */
    float *norm_weight[4], *norm_bias[4], *prelu_weight[4]; /* layers.{1,4,7,10}.{weight,bias}, layers.{2,5,8,11}.weight */
    float *fc1_weight_orig, *fc1_bias, *fc1_u, *fc1_v;    /* layers.14.* */
    float *prelu5_weight;                                 /* layers.16.weight */
    float *fc2_weight_orig, *fc2_bias, *fc2_u, *fc2_v;    /* layers.17.* */
    float *slope;                                         /* layers.18.slope */
} cmgan_disc_params;
size_t cmgan_disc_workspace_bytes(const cmgan_handle* h, int B, int T);
int cmgan_disc_forward(cmgan_handle* h, const float* xy_dev, int B, int T, const cmgan_disc_params* params,
                       const float* mask_dev, int update_uv, float* score_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream);
int cmgan_disc_backward(cmgan_handle* h, const float* xy_dev, const float* dscore_dev, int B, int T,
                        const cmgan_disc_params* params, const float* mask_dev, float* dxy_dev,
                        const cmgan_disc_params* grads, void* workspace_dev, size_t workspace_bytes, void* stream);
/* xy [B,T,F,2] = (|clean_spec|, |est|) (train.py:102-103); est_* NULL -> (|clean|, |clean|) (train.py:166).
 * Backward: d_real / d_imag += scale * dxy[...,1] * est / |est|  (the path of gen_loss_GAN into the generator).   */
int cmgan_mag_pair(cmgan_handle* h, const float* clean_spec_dev, const float* est_real_dev, const float* est_imag_dev,
                   int B, int T, float* xy_dev, void* stream);
int cmgan_mag_pair_backward(cmgan_handle* h, const float* est_real_dev, const float* est_imag_dev,
                            const float* dxy_dev, int B, int T, float scale, float* d_real_dev, float* d_imag_dev,
                            void* stream);
/* loss = mean((score - target)^2) with target = 1 when NULL (train.py:129-131, 168-170); dscore (may be NULL) =
 * scale * d loss / d score.                                                                                       */
int cmgan_score_mse(cmgan_handle* h, const float* score_dev, const float* target_dev, int B, float scale,
                    float* loss_dev, float* dscore_dev, void* stream);

/* One torch.optim.AdamW step (src/train.py:63-66, 192-193; defaults betas (0.9, 0.999), eps 1e-8, weight_decay
 * 0.01) over a FLAT fp32 bucket of n parameters: params, grads and the two moment buffers are parallel device
 * arrays (the bucket the gradient all-reduce runs over), `step` = 1, 2, ... is the update count for the bias
 * corrections, `lr` the scheduled learning rate (StepLR(30, 0.5) is host arithmetic, train.py:248-253).          */
int cmgan_adamw_step(cmgan_handle* h, float* params_dev, const float* grads_dev, float* exp_avg_dev,
                     float* exp_avg_sq_dev, long long n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, void* stream);

/* The same update with the optimiser's scalars in device memory: state_dev[0] = learning rate, state_dev[1] = update
 * count (a float, advanced by one by this call before it is used for the bias corrections).  Nothing in the launch
 * depends on host values that change from step to step, so it can be captured in a hipGraph and replayed; a learning
 * rate schedule writes state_dev[0] between replays.                                                               */
int cmgan_adamw_step_dev(cmgan_handle* h, float* params_dev, const float* grads_dev, float* exp_avg_dev,
                         float* exp_avg_sq_dev, long long n, float* state_dev, float beta1, float beta2, float eps,
                         float weight_decay, void* stream);

/* utils.power_compress (src/utils.py:20-29): x[B,F,T,2] -> y[B,2,F,T].          */
int cmgan_power_compress(cmgan_handle* h, const float* x_dev, int B, int F, int T,
                         float* y_dev, void* stream);
/* utils.power_uncompress (src/utils.py:32-39): real,imag[B,1,F,T] -> y[B,1,F,T,2]. */
int cmgan_power_uncompress(cmgan_handle* h, const float* real_dev, const float* imag_dev,
                           int B, int F, int T, float* y_dev, void* stream);

/* ConformerBlock.forward (src/models/conformer.py:216-222), eval mode, for the
 * conformer stored in slot `index` of the loaded weights (2*(k-1) = TSCB_k.time,
 * 2*(k-1)+1 = TSCB_k.freq; a standalone block is packed into slot 0).
 * x[N,L,64] contiguous -> y[N,L,64].  `taps_dev` (may be NULL) receives the
 * residual stream after ff1 / attn / conv / ff2 as 4 consecutive [N,L,64] tensors
 * (test hook).  Workspace: cmgan_conformer_workspace_bytes(h, N, L).            */
size_t cmgan_conformer_workspace_bytes(const cmgan_handle* h, int N, int L);
int cmgan_conformer_forward(cmgan_handle* h, int index, const float* x_dev, int N, int L,
                            float* y_dev, float* taps_dev,
                            void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same with the attention mask of ConformerBlock.forward(x, mask) (conformer.py:113-126, 217):
 * mask_dev [N, L] bytes, non-zero = keep.  A (query i, key j) pair keeps its score only when both are kept; every
 * other score is the reference's -finfo.max, i.e. kept queries ignore masked keys and a masked query attends
 * uniformly to all L keys.  Only the attention uses the mask (feed-forward, conv module and norms see every row),
 * exactly like the reference.  CMGAN itself never passes one (generator.py:95,97).                              */
int cmgan_conformer_forward_masked(cmgan_handle* h, int index, const float* x_dev, int N, int L,
                                   const unsigned char* mask_dev, float* y_dev, float* taps_dev,
                                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* Stage taps of TSCNet.forward for parity tests (NCHW like the reference so the
 * tests read like the reference's module outputs); any pointer may be NULL:
 *   encoder[B,64,T,F']  = dense_encoder(x_in)        generator.py:181
 *   tscb[4][B,64,T,F']  = TSCB_1..4 outputs          generator.py:182-185
 *   mask[B,1,T,F], complex_out[B,2,T,F]              generator.py:187,190
 * Runs the same kernels as cmgan_tscnet_forward.                                */
typedef struct cmgan_taps {
    float* encoder_dev;
    float* tscb_dev[4];
    float* mask_dev;
    float* complex_dev;
} cmgan_taps;
int cmgan_tscnet_forward_taps(cmgan_handle* h, const float* spec_dev, int B, int T,
                              float* out_real_dev, float* out_imag_dev, const cmgan_taps* taps,
                              void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Streaming with carried state (BASELINE.json configs[4]) --------------------------
 * The reference has no streaming mode; the hooks it leaves are its already-causal dilated convs (generator.py:16-20,
 * 39-47) and the unused `causal` flag of the conv module (conformer.py:153,158,168).  What makes the encoder and the
 * decoders non-causal in the reference is ONLY InstanceNorm2d's statistics over all of T (generator.py:35,55,61,
 * 128,148).  With the statistics FROZEN (taken from a calibration pass and then held, like BatchNorm in eval mode) the
 * dense encoder and both decoders are exactly time-causal with a receptive field of 1 + 2 + 4 + 8 = 15 frames back:
 * frame t of their output is a function of frames t - 15 .. t of their input.  So their state CAN be carried across
 * windows exactly: 15 frames of input history in front of the new frames, first 15 output frames dropped.  The four
 * TSCBs attend over the whole window (bidirectional, no exact cache exists): they run on [context | window |
 * look-ahead] frames of cached / fresh encoder outputs, as before.
 *
 *   cmgan_stats_floats(h, B)        floats of one statistics blob: the (scale, shift) pairs of the 15 InstanceNorms
 *                                   per row + the mask head's one-channel norm.  Opaque; valid for that B.
 *   cmgan_tscnet_forward_stats      cmgan_tscnet_forward with `frozen_stats` (may be NULL = the tensor's own
 *                                   statistics, i.e. the reference's arithmetic) and `stats_out` (may be NULL): the blob
 *                                   of the statistics this call used.  A call with frozen_stats = its own stats_out
 *                                   reproduces the unfrozen call bit for bit.
 *   cmgan_stream_encoder            spec[B,2,T,F] -> x[B,T,F',64] (channels-last, the layout the TSCBs and decoders
 *                                   share) = dense_encoder (generator.py:65-69) under frozen statistics
 *   cmgan_stream_tscb               x[B,T,F',64] in place = TSCB_1..4 (generator.py:92-99, 182-185)
 *   cmgan_stream_decoder            x[B,T,F',64] + spec[B,2,T,F] -> est_real / est_imag [B,1,T,F] = mask + complex decoder
 *                                   + recombination (generator.py:187-194) under frozen statistics
 * Exactness (tests/test_gpu_parity.py::test_stream_*): frames t >= 15 of cmgan_stream_encoder on ANY slice of a clip's
 * spectrogram equal the same frames of the whole-clip call bit for bit; likewise the decoder.  Workspace:
 * cmgan_workspace_bytes(h, B, T) of the call's own T.                                                           */
size_t cmgan_stats_floats(const cmgan_handle* h, int B);
int cmgan_tscnet_forward_stats(cmgan_handle* h, const float* spec_dev, int B, int T, float* out_real_dev,
                               float* out_imag_dev, const float* frozen_stats_dev, float* stats_out_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream);
int cmgan_stream_encoder(cmgan_handle* h, const float* spec_dev, int B, int T, const float* frozen_stats_dev,
                         float* x_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int cmgan_stream_tscb(cmgan_handle* h, float* x_dev, int B, int T, void* workspace_dev, size_t workspace_bytes,
                      void* stream);
int cmgan_stream_decoder(cmgan_handle* h, const float* x_dev, const float* spec_dev, int B, int T,
                         const float* frozen_stats_dev, float* out_real_dev, float* out_imag_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* Running statistics (opt-in; the frozen blob above stays the default).  A running stream needs no calibration: each
 * row carries, for each of the 15 64-channel InstanceNorms and the mask head's one-channel norm, three fp64 numbers per
 * channel - n, sum x, sum x^2 - where x is that norm's INPUT (the conv output, bias included).  A call on T frames whose
 * first `hist` (0 <= hist < T) are history does, for every norm in network order:
 *   1. add the norm input over frames [hist, T), all frequency bins, to the carried sums (history is not counted again);
 *   2. mean = sum x / n, var = max(sum x^2 / n - mean^2, 0) (in_finalize's arithmetic), eps 1e-5 and the affine
 *      weights give the (scale, shift) pair; the sub-pixel norm folds channels c and c + 64 like the frozen path;
 *   3. normalise ALL T frames of the call, history included, with that pair.
 * Frames of earlier calls are not recomputed.  With hist = 0 on fresh (zero) sums the call is the reference arithmetic
 * on its frames, to fp64 summation order.  The sums are reduced in a fixed order (no atomics): replays of a captured
 * call give the same bits as eager calls.
 *   cmgan_stream_sums_doubles(h, B)  doubles of one sums blob, [norm j < 15][B][64][3] then the mask head's [B][3], in
 *                                    that order (n, sum x, sum x^2); 0 for a null h or B <= 0.  Zero it to start a stream.
 *   cmgan_stream_encoder_running     cmgan_stream_encoder with running statistics: updates norms 0..5 of sums_io
 *   cmgan_stream_decoder_running     cmgan_stream_decoder with running statistics: updates norms 6..15 of sums_io
 * The two touch disjoint parts of one blob, so the encoder of step k + 1 may run beside the decoders of step k.
 * `stats_out` (may be NULL) receives the statistics blob (cmgan_stats_floats layout) the call used: the encoder writes
 * its part (norms 0..5), the decoder the rest.  A null or out-of-range argument returns CMGAN_E_BADARG before anything
 * is enqueued.  Workspace: cmgan_workspace_bytes(h, B, T) of the call's own T.                                         */
size_t cmgan_stream_sums_doubles(const cmgan_handle* h, int B);
int cmgan_stream_encoder_running(cmgan_handle* h, const float* spec_dev, int B, int T, int hist, double* sums_io_dev,
                                 float* stats_out_dev, float* x_out_dev, void* workspace_dev, size_t workspace_bytes,
                                 void* stream);
int cmgan_stream_decoder_running(cmgan_handle* h, const float* x_dev, const float* spec_dev, int B, int T, int hist,
                                 double* sums_io_dev, float* stats_out_dev, float* out_real_dev, float* out_imag_dev,
                                 void* workspace_dev, size_t workspace_bytes, void* stream);

/* Self-test of the MFMA fragment conventions every kernel relies on: computes
 * D = A(16xK) * B(Kx16) with the f32 16x16x4 MFMA and the library's fragment
 * packing; returns max |D - reference| through *max_err_host (synchronises).   */
int cmgan_selftest_mfma(cmgan_handle* h, float* max_err_host);
/* Same for the f16 16x16x32 MFMA + split-product images of the F16X3 mode. */
int cmgan_selftest_mfma_x3(cmgan_handle* h, float* max_err_host);

/* ---- Objective speech metrics (src/tools/compute_metrics.py; host twin: cmgan_amd/metrics.py) --------------------
 * Scores B equal-length float32 pairs [B, L] (clean, enhanced) in float64: per row
 *   scores_dev[b][9] = pesq csig cbak covl ssnr stoi wss llr snr
 * (wss / llr: the 95 % trimmed means; snr: the overall SNR in dB; csig / cbak / covl from the caller's PESQ,
 * pesq_dev[b], or NaN when pesq_dev is NULL - PESQ itself is not computed here).  frames_dev, when not NULL, receives
 * [B][3][nf] per-frame WSS, LLR and clipped segmental SNR, nf = max(nf_wss, nf_llr) with
 * nf_wss = int(L / hop - win / hop), nf_llr = int((L - win) / hop) (win / hop = 480 / 120 at 16 kHz, 240 / 60 at
 * 8 kHz); entries past a measure's own count are NaN.  `offset` is added to every widened sample (the reference adds
 * eps to both signals when it trims unequal lengths; 0 otherwise).  fs = 16000 or 8000, else CMGAN_E_UNSUPPORTED.
 * CMGAN_E_BADSHAPE when L < win or L is too short for one 30-frame STOI window (at least 31 frames of 256 samples at
 * 10 kHz).  Difference from the host: a row whose STOI silence removal keeps fewer than 31 frames (so no 30-frame
 * window) gets stoi = NaN where the host tool raises.  Workspace: cmgan_metrics_workspace_bytes (h may be NULL; 0 for
 * an invalid shape), 256-byte aligned.  No synchronisation; graph-capturable.                                   */
size_t cmgan_metrics_workspace_bytes(const cmgan_handle* h, int B, int L, int fs);
int cmgan_metrics(cmgan_handle* h, const float* clean_dev, const float* enh_dev, int B, int L, int fs,
                  const double* pesq_dev, double offset, double* scores_dev, double* frames_dev,
                  void* workspace_dev, size_t workspace_bytes, void* stream);
/* Host-side export of the tables the metric kernels build (same C++ code), for tests: which = 0 analysis taper [win],
 * 1 WSS bank [25 first bins, 25 counts, 25 x 64 weights], 2 STOI bands [kept, then (first, end) bin pairs],
 * 3 STOI inner Hann window [256], 4 resample_poly FIR to 10 kHz [zero pre-pad + taps].  out_host NULL: returns the
 * count; otherwise writes it (cap >= count) and returns it.  Negative CMGAN_E_* on error.                          */
int cmgan_metrics_table(int fs, int which, double* out_host, size_t cap);

/* ---- Sample-rate conversion (the reference asserts sr == 16000, src/evaluation.py:19, and leaves it to the user) ------
 * Rational-rate polyphase FIR resampling of a float32 batch: the arithmetic of scipy.signal.resample_poly(x, up, down)
 * with its default window ('kaiser', 5.0) and padtype='constant'.  With g = gcd(fs_in, fs_out), up = fs_out / g,
 * down = fs_in / g, m = max(up, down), half_len = 10 m:
 *   taps        h = firwin(2 half_len + 1, 1 / m, window=('kaiser', 5.0)) * up in float64, with
 *               pre = down - half_len % down zeros in front (n_taps counts them)
 *   pre_remove  (half_len + pre) / down
 *   length      N = ceil(L up / down)
 *   output      y[n] = sum_i x[i] h[(n + pre_remove) down - i up], 0 <= n < N, over the i whose tap index lies in
 *               [0, n_taps), with x[i] = 0 outside [0, L)
 * Products and sums are float64, the taps of one output are added in ascending tap index, and the sum is rounded to
 * float32 once.  Supported: positive rates whose reduced max(up, down) <= 640 (a table of at most 13 441 doubles), else
 * CMGAN_E_UNSUPPORTED.  fs_in == fs_out is a copy.
 * cmgan_resample_geometry / _out_len are host arithmetic (no handle, no GPU; out_len returns a negative code on error);
 * cmgan_resample_table exports the taps (same C++ code as the table kernel; tap-major, pre-pad included) with the
 * calling convention of cmgan_metrics_table.
 * cmgan_resample serves whole signals and chunks: it writes outputs [n0_out, n0_out + n_out) of every row to
 * y_dev[b * ld_out + (n - n0_out)], reading a buffer x_dev[b * ld_in + q] that holds samples [pos_in, pos_in + n_buf) of
 * the signal; samples outside the buffer count as zero.  A whole signal is pos_in = n0_out = 0, n_buf = L, n_out = N.
 * A zero sample leaves the float64 sum unchanged, so a chunked call whose buffer holds every sample its outputs reach -
 * inputs ceil(((n0_out + pre_remove) down - (n_taps - 1)) / up) .. floor((n0_out + n_out - 1 + pre_remove) down / up),
 * those inside the signal - gives the SAME BITS as the whole-signal call.  The caller keeps n0_out + n_out <= N.
 * Workspace: cmgan_resample_workspace_bytes (h may be NULL; 0 for an unsupported pair), 256-byte aligned; it receives
 * the phase-major tap table, rebuilt by every call.  No synchronisation, no allocation, no atomics; graph-capturable. */
int cmgan_resample_geometry(int fs_in, int fs_out, int* up, int* down, int* n_taps, int* pre_remove);
long long cmgan_resample_out_len(int fs_in, int fs_out, long long n_in);
int cmgan_resample_table(int fs_in, int fs_out, double* out_host, size_t cap);
size_t cmgan_resample_workspace_bytes(const cmgan_handle* h, int fs_in, int fs_out);
int cmgan_resample(cmgan_handle* h, const float* x_dev, int B, int n_buf, long long ld_in, long long pos_in,
                   int fs_in, int fs_out, long long n0_out, int n_out, float* y_dev, long long ld_out,
                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Dynamic mixing (the reference replays pairs mixed beforehand: src/data/dataloader.py:13-50 reads clean/x.wav and
 * noisy/x.wav; its --cut_len help names "denoise and dereverberation") ------------------------------------------------
 * Turns B rows of clean speech, clean_dev[b * ld + i], 0 <= i < L, into a (noisy, target) training pair per row.  Every
 * per-row draw is read from DEVICE memory by the kernels, never by the host:
 *   noise   a flat float32 bank of bank_len samples; row b uses the segment noise_start[b] .. + noise_len[b] from
 *           offset noise_off[b] (int64 [B] each)
 *   RIR     optional: a float32 bank [R, Kmax], rows zero-padded, with rir_index[b] and rir_len[b] (int32 [B]);
 *           rir_bank_dev == NULL means no reverberation (R, Kmax, rir_index_dev, rir_len_dev are then ignored)
 *   snr_db  float32 [B], the requested speech-to-noise ratio
 *   peak    host float, the peak limit;  early  host int, the samples of early reflections kept in the target, -1 for a
 *           dry target
 * With h = rir[rir_index[b], 0:K], K = rir_len[b] (without a bank h = [1]):
 *   direct path  d = the FIRST index at which |h| is largest (without a bank d = 0)
 *   speech       speech[i] = sum_{k = 0 .. K-1} h[k] clean[b, i + d - k], 0 <= i < L, with clean = 0 outside [0, L):
 *                the direct-path delay is removed, so speech stays aligned with the dry clip
 *   target       early == -1: target = clean, a copy of its bits.  Otherwise the same sum over the taps k <= d + early:
 *                early >= K gives the reverberant speech itself, early = 0 everything up to and including the direct path
 *   noise        n[i] = bank[noise_start[b] + (noise_off[b] + i) mod noise_len[b]]: a short item wraps as often as needed
 *   gain         Ps = mean(speech^2), Pn = mean(n^2), g = sqrt(Ps / (Pn 10^(snr_db[b] / 10))); g = 0 when Ps == 0 or Pn == 0
 *   mix          v = speech + g n, m = max_i |v[i]|, s = peak / m if m > peak, else exactly 1
 *   outputs      noisy_dev[b * ld_out + i] = f32(v[i] s), target_dev[b * ld_out + i] = f32(target[i] s); with s == 1 and
 *                early == -1 the target is bit-identical to clean.  g_dev, scale_dev (= s), ps_dev, pn_dev: float64 [B]
 * Every product and sum is float64 and every output sample is rounded to float32 exactly once.  Ps, Pn and m are two-stage
 * reductions in a fixed order that depends on L alone (one partial per tile of cmgan_mix_tile() samples, then the
 * partials in ascending order): no atomics, the same bits from run to run, and row b's outputs depend neither on B nor on
 * the other rows.  Both sums of the target variant come from one pass over the same loads.
 * Supported: 1 <= B <= 65535, 1 <= L <= 2^31 - 1 - cmgan_mix_tile(), 1 <= Kmax <= 65536 (K may exceed L), else
 * CMGAN_E_BADARG / CMGAN_E_UNSUPPORTED before any launch.  Every argument is checked before the handle is, and the message
 * of a call with h == NULL is read with cmgan_last_error(NULL).  Table entries cannot be checked by the host without a
 * synchronisation, so the kernels never follow one outside its bank: a noise segment that is empty or leaves
 * [0, bank_len) counts as silence, rir_index is clamped to [0, R) and rir_len to [1, Kmax]; noise_off may be any int64.
 * Workspace: cmgan_mix_workspace_bytes (h may be NULL; 0 for an unsupported shape; non-decreasing in B, L and Kmax),
 * 256-byte aligned; it holds the float64 speech and target rows between the launches.  Six launches (five without a
 * bank), no synchronisation, no allocation; graph-capturable, and a replay reads the tables' current contents.  The call
 * is cmgan_scene (below) without located sources: the same checks, kernels and workspace layout, under this name.       */
int cmgan_mix_tile(void);
size_t cmgan_mix_workspace_bytes(const cmgan_handle* h, int B, int L, int Kmax);
int cmgan_mix(cmgan_handle* h, const float* clean_dev, int B, int L, long long ld, const float* noise_bank_dev,
              long long bank_len, const long long* noise_start_dev, const long long* noise_len_dev,
              const long long* noise_off_dev, const float* rir_bank_dev, int R, int Kmax, const int* rir_index_dev,
              const int* rir_len_dev, const float* snr_db_dev, float peak, int early, float* noisy_dev,
              float* target_dev, long long ld_out, double* g_dev, double* scale_dev, double* ps_dev, double* pn_dev,
              void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Scenes: located noise sources and interfering talkers (no counterpart in the reference, see "Dynamic mixing") ------
 * cmgan_mix with up to S <= cmgan_scene_max_sources() = 4 further sources per row, each INSIDE the room: convolved with a
 * response of its own and mixed in at an SNR of its own.  speech, target and d are exactly those of cmgan_mix, and so is
 * the dry noise n0 with its tables; noise_bank_dev == NULL drops the n0 term (its four tables are then ignored).  The
 * sources read ONE flat float32 bank src_bank_dev of src_bank_len samples - the noise bank again, or any other: a bank of
 * speech gives interfering talkers - through tables in DEVICE memory, row-major [B, S]: src_start, src_len, src_off
 * (int64), src_snr_db (float32), src_rir_index, src_rir_len (int32, rows of the SAME rir_bank_dev as the talker; without
 * a bank every source is dry, h_j = [1]), and n_src int32 [B].  With S == 0 all of these are ignored.  For row b, with
 * S_b = n_src[b] clamped to [0, S], and for j = 1 .. S_b (table column j - 1):
 *   segment   seg_j[m] = src_bank[src_start + ((src_off + m) mod src_len)] for EVERY integer m: it loops both ways
 *   source    c_j[i] = sum_{k = 0 .. K_j - 1} h_j[k] seg_j[i - k], 0 <= i < L, h_j = rir[src_rir_index], K_j = src_rir_len.
 *             The direct-path delay is NOT removed: a source further from the microphone than the talker arrives later
 *   gain      P_j = mean(c_j^2), g_j = sqrt(Ps / (P_j 10^(src_snr_db / 10))); g_j = 0 when Ps == 0 or P_j == 0
 *   mix       v = speech + g0 n0 + g_1 c_1 + ... + g_{S_b} c_{S_b}, one fused multiply-add per term in this order; m, s and
 *             the outputs as in cmgan_mix
 *   outputs   noisy_dev, target_dev as in cmgan_mix; g_dev float64 [B, 1 + S] = g0, g_1 .. g_S and p_dev float64
 *             [B, 1 + S] = Pn, P_1 .. P_S (both 0 in the columns beyond S_b, and in column 0 without a dry-noise bank);
 *             ps_dev, scale_dev float64 [B]
 * Arithmetic, reductions and guarantees are those of cmgan_mix: float64 products and sums, taps in ascending k, one rounding
 * to float32; two-stage reductions in a fixed order that depends on L alone; no atomics.  Row b's outputs depend neither
 * on B, nor on the other rows or their n_src, nor on the table columns beyond S_b, which are never read.  With S == 0 and a
 * dry-noise bank every output has the bits of cmgan_mix: cmgan_mix IS that call (one implementation; it only insists on
 * the dry noise and on all four of its [B] outputs, and cmgan_mix_workspace_bytes(h, B, L, Kmax) equals
 * cmgan_scene_workspace_bytes(h, B, L, Kmax, 0)).  Untrusted tables as there: a source segment that is empty or
 * leaves [0, src_bank_len) is silence (c_j = 0, P_j = 0, g_j = 0), RIR indices are clamped to [0, R), lengths to [1, Kmax];
 * offsets may be any int64.
 * Method.  The source index is a grid axis of the convolution kernel: slice 0 is the talker's convolution of cmgan_mix,
 * slice j source j over the same tiles of cmgan_mix_tile() outputs; a block stages a chunk of taps and the LOOPED span
 * they reach on chip in float64, the modulo taken once per thread and chunk and advanced by a conditional subtraction per
 * staged sample, so src_len = 1 and src_len >> L cost the same.
 * Supported: the shapes of cmgan_mix and 0 <= S <= 4.  Every argument is checked before the handle is (cmgan_last_error(NULL)
 * reads the message of a call with h == NULL): CMGAN_E_BADARG / CMGAN_E_UNSUPPORTED before any launch.
 * Workspace: cmgan_scene_workspace_bytes (h may be NULL; 0 for an unsupported shape; non-decreasing in B, L, Kmax and S),
 * 256-byte aligned; it holds the float64 speech, target and c_j rows between the launches.  Six launches (five without a
 * RIR bank), no synchronisation, no allocation; graph-capturable, and a replay reads the tables' current contents.     */
int cmgan_scene_max_sources(void);
size_t cmgan_scene_workspace_bytes(const cmgan_handle* h, int B, int L, int Kmax, int S);
int cmgan_scene(cmgan_handle* h, const float* clean_dev, int B, int L, long long ld, const float* noise_bank_dev,
                long long bank_len, const long long* noise_start_dev, const long long* noise_len_dev,
                const long long* noise_off_dev, const float* snr_db_dev, const float* src_bank_dev, long long src_bank_len,
                int S, const int* n_src_dev, const long long* src_start_dev, const long long* src_len_dev,
                const long long* src_off_dev, const float* src_snr_db_dev, const float* rir_bank_dev, int R, int Kmax,
                const int* rir_index_dev, const int* rir_len_dev, const int* src_rir_index_dev, const int* src_rir_len_dev,
                float peak, int early, float* noisy_dev, float* target_dev, long long ld_out, double* g_dev, double* p_dev,
                double* ps_dev, double* scale_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Paths: a talker and sources that MOVE through the room (no counterpart in the reference, see "Scenes") ------------
 * cmgan_scene with a path of responses instead of one: P waypoint columns per row and per source, waypoint p at input
 * sample p H (host ints, 1 <= P <= cmgan_scene_max_waypoints() = 64, 1 <= H <= 2^30).  rir_index_dev / rir_len_dev are
 * int32 [B, P], src_rir_index_dev / src_rir_len_dev int32 [B, S, P], n_path_dev int32 [B] and src_n_path_dev int32 [B, S]
 * say how many of the columns a row / a source uses: Pb = the entry clamped to [1, P], read on the device; the columns
 * beyond Pb are never read.  A RIR bank is required (without one there is nothing to move through: CMGAN_E_BADARG).  All
 * other arguments, the outputs and the untrusted-table rules (indices clamped to [0, R), lengths to [1, Kmax]) are
 * cmgan_scene's.
 *   weights  for any integer input index m:  u_p[m] = (double)(H - |m - p H|) / (double)H where that is positive, else 0 -
 *            an exact integer numerator and one IEEE division; u_0[m] = 1 for m <= 0, u_{Pb-1}[m] = 1 for m >= (Pb - 1) H
 *            (Pb = 1: u_0 = 1 everywhere).  Neighbouring waypoints cross-fade linearly by EMISSION time.
 *   talker   h_p the response of waypoint p, d_p ITS OWN first-argmax direct index.
 *            speech[i] = sum over p ascending, then k ascending, of h_p[k] xw,  xw = u_p[m] (double)clean[b, m] rounded
 *            once to float64,  m = i + d_p - k; only the terms with 0 <= m < L and u_p[m] > 0 count.  One fused
 *            multiply-add per term into ONE accumulator from 0, across the waypoints.  Every waypoint's own delay is
 *            removed: the speech stays aligned with the dry clip wherever the talker is, and the direct peaks of
 *            neighbouring responses coincide, so the cross-fade does not comb them.
 *   target   early >= 0: the same sum over the taps k <= d_p + early of each waypoint, from the same loads; early == -1:
 *            the clean row's bits, as in cmgan_mix.
 *   sources  c_j[i] = the same sum with m = i - k (the delay stays) over seg_j[m], which loops both ways; EVERY integer m
 *            is weighted by u_p[m], m < 0 included.  Silence rules as in cmgan_scene.
 *   the rest powers, gains, the fma chain over the sources, the peak guard, the stores and the outputs g, p, ps, scale
 *            are cmgan_scene's, by the same kernels.
 * NOT modelled: Doppler shift.  The responses are cross-faded at the emitted sample; no sample is resampled in time, so a
 * fast source changes colour and level but not pitch.
 * Contract: a row with Pb = 1 whose sources all have one waypoint has the bits of cmgan_scene called with column 0 of the
 * tables.  Guarantees as there: no atomics, reductions in an order that depends on L alone, the same bits from run to
 * run; a row's bits depend neither on B, nor on the other rows or their n_path, nor on padding, nor on unread columns.
 * Whether a zero-weight term of a non-finite tap shows in the output is unspecified.
 * Method.  scene_direct_path, grid (P, B), finds d_p.  scene_conv_path has scene_conv's grid: a block owns
 * cmgan_mix_tile() outputs of one (row, source) slice and, for every waypoint whose window can reach the tile, walks only
 * the taps that meet a non-zero weight - at most cnt + 2 H - 2, inside [0, K_p) and, for the talker, inside the clip - in
 * the chunks of scene_conv, with the span staged on chip ALREADY weighted (one product per staged sample, not per term).
 * Expected cost: about 2 + cmgan_mix_tile() / H times cmgan_scene's convolution.
 * Every argument is checked before the handle is (cmgan_last_error(NULL) reads the message of a call with h == NULL):
 * CMGAN_E_BADARG / CMGAN_E_UNSUPPORTED before any launch, a short or misaligned workspace included.
 * Workspace: cmgan_scene_path_workspace_bytes (h may be NULL; 0 for an unsupported shape; non-decreasing in every
 * argument): cmgan_scene's plus d [B, P].  Six launches, no synchronisation, no allocation; graph-capturable, and a replay
 * reads the tables' current contents.                                                                                  */
int cmgan_scene_max_waypoints(void);
size_t cmgan_scene_path_workspace_bytes(const cmgan_handle* h, int B, int L, int Kmax, int S, int P);
int cmgan_scene_path(cmgan_handle* h, const float* clean_dev, int B, int L, long long ld, const float* noise_bank_dev,
                     long long bank_len, const long long* noise_start_dev, const long long* noise_len_dev,
                     const long long* noise_off_dev, const float* snr_db_dev, const float* src_bank_dev,
                     long long src_bank_len, int S, const int* n_src_dev, const long long* src_start_dev,
                     const long long* src_len_dev, const long long* src_off_dev, const float* src_snr_db_dev,
                     const float* rir_bank_dev, int R, int Kmax, int P, int H, const int* n_path_dev,
                     const int* rir_index_dev, const int* rir_len_dev, const int* src_n_path_dev,
                     const int* src_rir_index_dev, const int* src_rir_len_dev, float peak, int early, float* noisy_dev,
                     float* target_dev, long long ld_out, double* g_dev, double* p_dev, double* ps_dev, double* scale_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Room impulse responses (the reference ships no impulse responses and no simulator; its --cut_len help names
 * "denoise and dereverberation", src/data/dataloader.py:13-50 replays pairs mixed beforehand) --------------------------
 * Simulates R shoe-box rooms by the image-source method (Allen & Berkley 1979) with Peterson's Hann-windowed sinc for the
 * fractional delays, into the float32 [R, K] bank + int32 [R] lengths that cmgan_mix takes as rir_bank_dev / rir_len.
 * Per-row inputs are read from DEVICE memory by the kernels, never by the host:
 *   rooms_dev   float64 [R, 15]: room size Lx Ly Lz (m), source sx sy sz, receiver mx my mz, reflection coefficients
 *               bx0 bx1 by0 by1 bz0 bz1 (wall at 0 and wall at L, per axis)
 *   n_taps_dev  int32 [R], the length of row r's response
 * Host arguments: fs (Hz), c (speed of sound, m/s), tw (half-width of the fractional-delay filter in samples),
 * Nx Ny Nz (image index range per axis), K (taps per row of the bank), ld (floats between rows, >= K).
 * For row r, with k_r = clamp(n_taps[r], 1, K), the sum runs over n = (nx, ny, nz), |n_axis| <= N_axis, and over
 * p = (px, py, pz) in {0, 1}^3:
 *   offset   per axis (1 - 2 p) s + 2 n L - m;  d = its Euclidean length;  tau = d fs / c
 *   a        prod_axis b_axis0^|n - p| b_axis1^|n| / (4 pi max(d, CMGAN_RIR_DMIN))                      (0^0 = 1)
 *   taps     h[k] = sum_images a w(k - tau) sinc(k - tau), 0 <= k < k_r, with w(t) = (1 + cos(pi t / tw)) / 2 for
 *            |t| < tw, else 0, and sinc(t) = sin(pi t) / (pi t), sinc(0) = 1; images with tau - tw >= K add nothing
 *   outputs  rir_dev[r * ld + k] = f32(h[k]) for k < k_r and exactly 0.0f for k_r <= k < K;  len_dev[r] = k_r
 * Not modelled: a high-pass filter; air absorption and frequency-dependent walls are cmgan_rir_bands, directional sources
 * and receivers cmgan_rir_dir / cmgan_rir_bands_dir, both below.
 * All arithmetic is float64 and each tap is rounded to
 * float32 exactly once.  A block owns cmgan_rir_tile() consecutive taps of one row and adds the images that reach them in
 * one fixed enumeration order (nx, ny, p, nz ascending), staged cmgan_rir_list_capacity() at a time in an on-chip list by
 * an order-preserving compaction: no atomics, the same bits from run to run, row r's bits depend neither on R nor on the
 * other rows, and an N larger than the response needs changes no bit.
 * Table entries cannot be checked by the host without a synchronisation: a row with a non-finite entry, a room size <= 0
 * or a coefficient outside [0, 1] is written as all zeros with len = 1, n_taps is clamped to [1, K], and no entry is ever
 * turned into an address.  Checked before any launch and before the handle is looked at (the message of a call with
 * h == NULL is read with cmgan_last_error(NULL)): null or misaligned pointers, 1 <= R <= 65535, 1 <= K <= 65536, ld >= K,
 * fs > 0, c > 0 and finite, 1 <= tw <= 64, 0 <= N_axis <= 255 and 8 (2Nx+1)(2Ny+1)(2Nz+1) < 2^31; otherwise
 * CMGAN_E_BADARG / CMGAN_E_UNSUPPORTED.  Workspace: cmgan_rir_workspace_bytes (h may be NULL; 0 when unsupported;
 * non-decreasing in R, K and tw), 256-byte aligned; it holds each row's verdict and the powers of its coefficients between
 * the two launches.  No synchronisation, no allocation; graph-capturable, and a replay reads the tables' current contents. */
#define CMGAN_RIR_DMIN 0.01   /* metres: the distance below which 1 / (4 pi d) stops growing */
int cmgan_rir_tile(void);
int cmgan_rir_list_capacity(void);
size_t cmgan_rir_workspace_bytes(const cmgan_handle* h, int R, int K, int tw);
int cmgan_rir(cmgan_handle* h, const double* rooms_dev, const int* n_taps_dev, int R, int K, int fs, double c, int tw,
              int Nx, int Ny, int Nz, float* rir_dev, long long ld, int* len_dev, void* workspace_dev,
              size_t workspace_bytes, void* stream);

/* ---- Room impulse responses in frequency bands: walls whose absorption depends on frequency, and air absorption ------
 * cmgan_rir simulated in NB frequency bands at once and joined by a caller-supplied FIR filterbank.  An image's position,
 * delay, window and sinc are the same in every band and only its amplitude differs, so the image list is built once and
 * every tap carries one accumulator per band; NB calls of cmgan_rir would walk the list NB times.
 *   rooms_dev   float64 [R, 15], the table of cmgan_rir: columns 0 - 8 (size, source, receiver) are used, columns 9 - 14
 *               are never read
 *   bands_dev   float64 [R, NB, 7]: per band the six reflection coefficients in cmgan_rir's order, then m, the amplitude
 *               attenuation of air in nepers per metre (m >= 0)
 *   n_taps_dev  int32 [R], the length of row r's response
 *   filt_dev    float64 [NB, NF], NF odd, D = (NF - 1) / 2: one FIR per band, shared by all rows.  A caller-supplied
 *               table whose values are not judged: a NaN in it propagates to the taps and is never an address
 * For row r, with k_r = clamp(n_taps[r], 1, K) and the images (n, p), d, tau, w and sinc of cmgan_rir:
 *   a_b      prod_axis b_{b,axis0}^|n - p| b_{b,axis1}^|n| exp(-m_b d) / (4 pi max(d, CMGAN_RIR_DMIN))          (0^0 = 1)
 *   bands    h_b[q] = sum_images a_b w(q - tau) sinc(q - tau) for 0 <= q < k_r + D, and 0 outside that range
 *   join     h[k] = sum_{b ascending} sum_{j ascending} g_b[j] h_b[k + D - j], one fused multiply-add per term in that
 *            order: the filterbank's delay D is taken out, and the bands are simulated D taps past the row's end, so the
 *            join truncates nothing there.  The caller's image ranges must cover K + D taps
 *   outputs  rir_dev[r * ld + k] = f32(h[k]) for k < k_r and exactly 0.0f for k_r <= k < K;  len_dev[r] = k_r
 * Still not modelled: a material per wall beyond what the caller writes into the band table (directivity:
 * cmgan_rir_bands_dir, below).  The
 * guarantees are those of cmgan_rir: float64 throughout and one rounding to float32; per (tap, band) the images are added
 * in the one fixed enumeration order of cmgan_rir; no atomics; the same bits from run to run; row r's bits depend neither
 * on R nor on the other rows, and an N larger than needed changes no bit; nothing read from a table becomes an address.
 * A row with a non-finite entry in columns 0 - 8 or in its band table, a size <= 0, a coefficient outside [0, 1] or a
 * negative m is written as all zeros with len = 1.  Checked before any launch and before the handle is looked at (the
 * message of a call with h == NULL is read with cmgan_last_error(NULL)): everything cmgan_rir checks, 1 <= NB <=
 * cmgan_rir_max_bands() (8), NF odd in [1, cmgan_rir_max_filter()] (1023), 8-byte alignment of the band and filter
 * tables; otherwise CMGAN_E_BADARG / CMGAN_E_UNSUPPORTED.  Workspace: cmgan_rir_bands_workspace_bytes (h may be NULL; 0
 * when unsupported; non-decreasing in every argument), 256-byte aligned; it holds the row records (verdict, m_b, powers
 * of the 6 NB coefficients) and the float64 band responses [R, NB, K + D] between the three launches.  No
 * synchronisation, no allocation; graph-capturable, and a replay reads the tables' current contents. */
int cmgan_rir_max_bands(void);
int cmgan_rir_max_filter(void);
size_t cmgan_rir_bands_workspace_bytes(const cmgan_handle* h, int R, int K, int tw, int NB, int NF);
int cmgan_rir_bands(cmgan_handle* h, const double* rooms_dev, const double* bands_dev, const int* n_taps_dev, int R, int K,
                    int NB, const double* filt_dev, int NF, int fs, double c, int tw, int Nx, int Ny, int Nz,
                    float* rir_dev, long long ld, int* len_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Room impulse responses of directional sources and receivers: first-order patterns, per band ---------------------
 * cmgan_rir and cmgan_rir_bands treat both ends as points that radiate and hear equally in all directions.  These two
 * calls give each end a facing vector and a first-order pattern alpha + (1 - alpha) cos(theta), per band.  Two more tables
 * per call, float64, on the device, read by the kernels only:
 *   orient_dev   [R, 6]: the source's facing vector u, then the receiver's v.  Any length: the kernels normalise them, with
 *                |x| = sqrt(fma(z, z, fma(y, y, x x))) and three divisions, to the unit vectors u^ and v^
 *   pattern_dev  [R, NB, 2]: per band alpha_s, alpha_m in [0, 1] - 1 omni, 0.75 sub-cardioid, 0.5 cardioid, 0.25
 *                hyper-cardioid, 0 figure-of-eight, and anything between.  NB = 1 for cmgan_rir_dir
 * For the image (n, p) of cmgan_rir, with its offset o = (1 - 2 p) s + 2 n L - m per axis and d = |o|: the image of the
 * source looks along the mirrored vector u^_p = ((1 - 2 p_x) u^_x, (1 - 2 p_y) u^_y, (1 - 2 p_z) u^_z) - a reflection in
 * a wall normal to an axis flips that component; n does not enter - and
 *   cos_m = (o . v^) / d        cos_s = -(o . u^_p) / d        (both 0 when d == 0; o . w = fma(o_z, w_z, fma(o_y, w_y, o_x w_x)),
 *                                                               and the kernels multiply by one shared reciprocal 1 / d)
 *   g_b   = fma(1 - alpha_s,b, cos_s, alpha_s,b) * fma(1 - alpha_m,b, cos_m, alpha_m,b)      (signed: rear lobes are negative)
 *   a_b   = (the amplitude of cmgan_rir, or of band b of cmgan_rir_bands) * g_b
 * Everything else - the enumeration order, delay, window, sinc, CMGAN_RIR_DMIN, float64 with one rounding to float32, the
 * join of the band call - is what the plain calls do, and so are their guarantees: no atomics, the same bits from run to
 * run, row r independent of R and of the other rows, an N larger than needed changes no bit, nothing read from a table
 * becomes an address.  The gain depends on the image and not on the tap: it is computed where an image enters the
 * on-chip list, and the per-(image, tap) loop is the plain calls'.
 *   - With every alpha of a row exactly 1, g_b == 1.0 exactly: the row has the bits of cmgan_rir / cmgan_rir_bands.  For
 *     an end whose alphas are all 1 the vector may be anything finite, zero included.
 *   - Swapping source and receiver together with their vectors and patterns maps the image set onto itself with the
 *     same a_b (reciprocity).
 *   - A row is invalid (zeros, len = 1, like the invalid rows of the plain calls) when, beyond their rules, an orient or
 *     pattern entry is non-finite, an alpha is outside [0, 1], a vector component has |.| > 1e100, or an end that has
 *     some alpha < 1 has a vector whose length (as computed above) is zero.
 * Checked before any launch and before the handle is looked at: everything the plain call checks, and null or misaligned
 * (8 bytes) orient_dev / pattern_dev.  Workspace: cmgan_rir_dir_workspace_bytes / cmgan_rir_bands_dir_workspace_bytes
 * (h may be NULL; 0 when unsupported; non-decreasing in every argument; a little more than the plain calls': a row's
 * record also holds u^, v^ and the alphas).  No synchronisation, no allocation; graph-capturable, and a replay reads the
 * tables' current contents. */
size_t cmgan_rir_dir_workspace_bytes(const cmgan_handle* h, int R, int K, int tw);
int cmgan_rir_dir(cmgan_handle* h, const double* rooms_dev, const double* orient_dev, const double* pattern_dev,
                  const int* n_taps_dev, int R, int K, int fs, double c, int tw, int Nx, int Ny, int Nz, float* rir_dev,
                  long long ld, int* len_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
size_t cmgan_rir_bands_dir_workspace_bytes(const cmgan_handle* h, int R, int K, int tw, int NB, int NF);
int cmgan_rir_bands_dir(cmgan_handle* h, const double* rooms_dev, const double* bands_dev, const double* orient_dev,
                        const double* pattern_dev, const int* n_taps_dev, int R, int K, int NB, const double* filt_dev, int NF,
                        int fs, double c, int tw, int Nx, int Ny, int Nz, float* rir_dev, long long ld, int* len_dev,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- What a room impulse response measures as: decay curve, EDT / T20 / T30, DRR, C50 / C80, D50, Ts ------------------
 * (the reference ships no impulse responses and no meter: src/data/dataloader.py:13-50 replays pairs mixed beforehand)
 * The room-acoustic parameters of ISO 3382-1 as its published description gives them, broad-band and in the bands of a
 * caller-supplied FIR filterbank, for the R rows rir_dev[r * ld + k] of a float32 [R, K] bank such as cmgan_rir makes.  No
 * other program is claimed as the yardstick: the definition below is the contract.
 *   len_dev     int32 [R] in DEVICE memory, read by the kernels only, or NULL for n = K; n = clamp(len[r], 1, K).  Samples at
 *               k >= n and the padding between rows are never read
 *   filt_dev    float64 [NB, NF], the layout and limits of cmgan_rir_bands: NF odd, D = (NF - 1) / 2, one FIR per band, shared
 *               by all rows; its values are not judged (a NaN propagates to that band's columns and is never an address).
 *               NULL with NB = 0: the broad-band analysis only (NF must still be odd; 1 will do)
 *   stats_dev   float64 [R, NB + 1, P], P = cmgan_rir_stats_columns() = 10.  Slice 0 is broad-band, slice 1 + b is band b
 *   status_dev  int32 [R, NB + 1], may be NULL: the CMGAN_RIR_STATS_* bits below
 *   edc_dev     float64 [R, NB + 1, K], may be NULL: the decay curve EDC[k] for k < n and zeros from n on
 * fs (Hz) and direct_ms are host numbers.  round(x) is floor(x + 1/2).  For row r and slice s:
 *   band signal   s >= 1, b = s - 1:  y_s[k] = sum_j filt[b][j] h[k + D - j] for 0 <= k < n, with h = 0 outside [0, n); float64,
 *                 j ascending, one fused multiply-add per term, from 0.  y_0[k] = h[k]
 *   energy        e[k] = y_s[k]^2
 *   direct        k0 = the smallest k < n that maximises |h[k]| of the BROAD-BAND row: the same for every slice.
 *                 w = round(direct_ms fs / 1000),  k50 = min(k0 + round(0.050 fs), n),  k80 = min(k0 + round(0.080 fs), n)
 *   decay curve   EDC[k] = sum_{j >= k} e[j] (Schroeder's backward integral),  E = EDC[0]
 *   thresholds    ka(x) = the smallest k < n with EDC[k] <= c_x E, compared in the linear domain with the float64 constants
 *                 CMGAN_RIR_STATS_DOWN_x below (c_x = 10^(-x/10), x = 5, 10, 25, 35).  Without such a k, ka(x) does not exist
 *   decay times   T30 on [ka(5), ka(35)), T20 on [ka(5), ka(25)), EDT on [0, ka(10)).  With L[k] = 10 log10(EDC[k] / E), m the
 *                 number of samples in the range and kbar their mean index:
 *                     slope = fs sum_k (k - kbar) L[k] / (m (m^2 - 1) / 12)  dB/s,      time = -60 / slope  seconds
 *                 (the least-squares line through the curve, extrapolated to 60 dB).  If the range's end does not exist,
 *                 m < 2 or the slope is not negative, the time is NaN and its status bit is set
 *   ratios        A = sum e[k] over max(k0 - w, 0) <= k <= min(k0 + w, n - 1);  DRR = 10 log10(A / (before + after)), the
 *                 denominator the sum of the energies before and after that window, added as such and not E - A
 *                 C50 = 10 log10(sum_{k < k50} e / EDC[k50]),  C80 alike with k80;  D50 = sum_{k < k50} e / E
 *                 Ts = sum_k max(k - k0, 0) e[k] / (fs E)  seconds
 *                 an empty denominator (nothing outside the window; k50 = n or nothing after it) gives +inf dB
 *   columns       0 E, 1 k0 (as a double), 2 DRR dB, 3 C50 dB, 4 C80 dB, 5 D50, 6 Ts s, 7 EDT s, 8 T20 s, 9 T30 s
 *   status        CMGAN_RIR_STATS_NONFINITE: a sample within n is NaN or inf; every column of every slice of the row is NaN
 *                 (and its curve is NaN below n).  CMGAN_RIR_STATS_ZERO: E == 0; the slice's columns are NaN except E = 0.
 *                 CMGAN_RIR_STATS_NO_EDT / _NO_T20 / _NO_T30: that time is NaN (always set with the two bits before)
 * Not done: noise-floor compensation (Lundeby's truncation and correction) - a response with less than 35 dB of decay range
 * above its floor gets a T30 that includes the floor, the curve of a response cut at n bends down towards n (the integral
 * stops there) and a range that reaches into that bend shortens the time, and a response whose curve never falls 35 dB
 * below E gets NaN rather than a guess; ISO's own octave filters are not supplied - the caller's filterbank is used,
 * typically mixing.octave_filterbank, whose bands are wider than ISO's.
 * All arithmetic is float64 on the VALU.  A block of the first launch owns cmgan_rir_stats_tile() consecutive samples of one
 * (row, slice): it runs the band filter from on-chip copies of the span and the taps and leaves e[k] and the tile's total
 * (a fixed tree) in the workspace.  One block per (row, slice) of the second launch folds the totals in descending tile
 * order into entry sums, suffix-scans tile after tile from them, finds every ka as an integer minimum and k0 by a
 * max-reduction under a total order (larger |h|, then smaller index), and adds the ratio and regression sums per thread in
 * ascending k and then by the same fixed tree.  No atomics; every reduction runs in an order that depends on n and the tile
 * grid alone: the same bits from run to run, row r's bits depend neither on R nor on the other rows, nor on ld, nor on K
 * beyond n, and slice 0 does not depend on NB.  No value read from device memory is turned into an address except k0, which
 * the kernel computed itself as an index below n.
 * Checked before any launch and before the handle is looked at (the message of a call with h == NULL is read with
 * cmgan_last_error(NULL)): null rir_dev / stats_dev, misaligned pointers (4 bytes for rir, len and status, 8 for filt, stats
 * and edc), 1 <= R <= 65535, 1 <= K <= 65536, ld >= K, 0 <= NB <= cmgan_rir_max_bands(), filt_dev NULL exactly when NB = 0,
 * NF odd in [1, cmgan_rir_max_filter()], fs > 0, direct_ms finite and >= 0, a workspace that is null, not 256-byte aligned
 * or smaller than cmgan_rir_stats_workspace_bytes (h may be NULL; 0 for unsupported arguments; non-decreasing in each);
 * otherwise CMGAN_E_BADARG / CMGAN_E_UNSUPPORTED.  Two launches, no synchronisation, no allocation; graph-capturable, and a
 * replay reads the current contents of rir_dev, len_dev and filt_dev. */
#define CMGAN_RIR_STATS_NONFINITE 1
#define CMGAN_RIR_STATS_ZERO 2
#define CMGAN_RIR_STATS_NO_EDT 4
#define CMGAN_RIR_STATS_NO_T20 8
#define CMGAN_RIR_STATS_NO_T30 16
#define CMGAN_RIR_STATS_DOWN_5 0.31622776601683794     /* 10^-0.5 */
#define CMGAN_RIR_STATS_DOWN_10 0.1                     /* 10^-1   */
#define CMGAN_RIR_STATS_DOWN_25 0.0031622776601683794   /* 10^-2.5 */
#define CMGAN_RIR_STATS_DOWN_35 0.00031622776601683794  /* 10^-3.5 */
int cmgan_rir_stats_tile(void);
int cmgan_rir_stats_columns(void);
size_t cmgan_rir_stats_workspace_bytes(const cmgan_handle* h, int R, int K, int NB, int NF);
int cmgan_rir_stats(cmgan_handle* h, const float* rir_dev, int R, int K, long long ld, const int* len_dev,
                    const double* filt_dev, int NB, int NF, int fs, double direct_ms, double* stats_dev, int* status_dev,
                    double* edc_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- The diffuse reverberant tail behind the early part of a room impulse response ------------------------------------
 * (the reference ships no impulse responses and no simulator: src/data/dataloader.py:13-50 replays pairs mixed beforehand)
 * The image-source method costs the cube of the response length; after the mixing time the reflections are dense and
 * indistinguishable from decaying noise.  As gpuRIR does after its Tdiff, this call extends every row of a float32 [R, K]
 * bank IN PLACE from its junction with noise under an exponential envelope that follows a GIVEN 60 dB decay time, band by
 * band, the level fitted to one window in front of the junction.  It reads no room geometry: a recorded bank will do.
 * All tables are in DEVICE memory and read by the kernels only:
 *   rir_dev     float32 [R, K], row stride ld: row r holds valid taps below k_x; taps below k_x are never written
 *   len_dev     int32 [R], in / out.  In: the junction, k_x = clamp(len[r], 1, K).  Out: max(k_x, k_end)
 *   n_taps_dev  int32 [R]: the wanted total length, k_end = clamp(n_taps[r], 1, K)
 *   decay_dev   float64 [R, NB'], NB' = max(NB, 1): the 60 dB decay time of band b in seconds
 *   seed_dev    int64 [R]: one Philox key per row
 *   filt_dev    float64 [NB, NF], NF odd, D = (NF - 1) / 2: the filterbank cmgan_rir_bands joins with (its values are not
 *               judged), or NULL with NB = 0: broad-band, one band with g = {1}, NF = 1, D = 0 (the NF given is then only
 *               checked to be odd)
 *   status_dev  int32 [R], out: 0, or the CMGAN_RIR_TAIL_* bits of the reasons the row was left untouched
 *   gain_dev    float64 [R, NB'], out: A_b below; 0 for an untouched row
 * window (W samples) and fs (Hz) are host numbers.  For row r:
 *   noise    nu[q] = (w0 + w1 + w2 + w3 - 2 (2^32 - 1)) / CMGAN_RIR_TAIL_NOISE_DIV for q >= 0 and 0 for q < 0, with (w0 .. w3) the
 *            four 32-bit words of Philox4x32-10 at the counter words (q, 0, 0, 0) under the key (low, high 32 bits of
 *            seed[r]).  The numerator is an integer below 2^34, exact in float64; the divisor is sqrt((2^64 - 1) / 3), the
 *            standard deviation of the sum; the division is IEEE's.  Mean 0, variance 1, kurtosis 2.7 (four uniforms)
 *   rate     delta_b = CMGAN_RIR_TAIL_3LN10 / (decay[r][b] fs): amplitude nepers per sample
 *   band     z_b[k] = sum_j g_b[j] h[k + D - j] for k_x - D - W <= k < k_x - D: j ascending, one fused multiply-add per term
 *            from 0, h the row's float32 values widened and 0 outside [0, k_x)
 *   fit      E_b = sum_k z_b[k]^2,  G_b = sum_j g_b[j]^2,  S_b = sum_k exp(-2 delta_b (k - k_x)) over that window;
 *            A_b = sqrt(E_b / (G_b S_b)), and 0 where E_b = 0 (a silent band is no error).  Each sum: thread t of 256 adds its
 *            terms t, t + 256, ... in ascending order (squares by one fma each), thread 0 adds the 256 partials in ascending t
 *   tail     y[k] = sum_b sum_j g_b[j] e_b[k + D - j],  e_b[q] = (A_b exp(-delta_b (q - k_x))) nu[q] rounded in that bracketing,
 *            for k_x <= k < k_end: b ascending, then j ascending, one fused multiply-add per term into one accumulator
 *            from 0, as the join of cmgan_rir_bands sums
 *   outputs  rir_dev[r * ld + k] = f32(y[k]) for k_x <= k < k_end and exactly 0.0f for k_end <= k < K;  len[r] = k_end
 * A row is left untouched - its taps and its len unchanged, gain 0 - with one status bit per reason:
 *   CMGAN_RIR_TAIL_NOTHING    k_end <= k_x: nothing to add
 *   CMGAN_RIR_TAIL_WINDOW     k_x - D - W < 0: the window does not fit
 *   CMGAN_RIR_TAIL_DECAY      a decay time of the row is NaN, infinite or <= 0
 *   CMGAN_RIR_TAIL_NONFINITE  a sample the fit reads - h[k], max(k_x - W - 2 D, 0) <= k < k_x - is NaN or infinite (judged
 *                             only where the window fits)
 * Not done: no fit of the decay rate (the early part of a shoe-box response is too sparse for one: the time is an input),
 * no cross-fade (a hard switch at k_x), no Gaussian noise (kurtosis 2.7), nothing correlated between rows or channels.  A
 * decay time so short that exp overflows within the window (far below a sample) gives non-finite taps, never an address.
 * All arithmetic is float64 on the VALU and each tap is rounded to float32 exactly once.  The first launch has one block
 * per (band, row) for the fit; a block of the second owns cmgan_rir_tail_tile() consecutive taps of one row, computes nu
 * once for the span they reach and then, band after band, stages e_b on chip with one exp per element.  No atomics; the
 * same bits from run to run; row r's bits depend neither on R nor on the other rows (their samples, band tables or
 * seeds), nor on ld, nor on K beyond k_end.  Nothing read from a table becomes an address without a clamp.
 * Checked before any launch and before the handle is looked at (the message of a call with h == NULL is read with
 * cmgan_last_error(NULL)): null pointers (only filt_dev may be NULL), misaligned pointers (4 bytes for rir, len, n_taps and
 * status, 8 for decay, seed, filt and gain), 1 <= R <= 65535, 1 <= K <= 65536, ld >= K, 0 <= NB <= cmgan_rir_max_bands(),
 * filt_dev NULL exactly when NB = 0, NF odd in [1, cmgan_rir_max_filter()], 1 <= window <= cmgan_rir_tail_max_window()
 * (4096), fs > 0, a workspace that is null, not 256-byte aligned or smaller than cmgan_rir_tail_workspace_bytes (h may be
 * NULL; 0 for unsupported arguments; non-decreasing in each); otherwise CMGAN_E_BADARG / CMGAN_E_UNSUPPORTED.  The
 * workspace holds each row's junction between the two launches.  No synchronisation, no allocation; graph-capturable, and
 * a replay reads the tables' current contents - len_dev among them, which the call before it has rewritten. */
#define CMGAN_RIR_TAIL_NOTHING 1
#define CMGAN_RIR_TAIL_WINDOW 2
#define CMGAN_RIR_TAIL_DECAY 4
#define CMGAN_RIR_TAIL_NONFINITE 8
#define CMGAN_RIR_TAIL_3LN10 6.907755278982137       /* 3 ln 10 */
#define CMGAN_RIR_TAIL_NOISE_DIV 2479700524.506239   /* sqrt((2^64 - 1) / 3) */
int cmgan_rir_tail_tile(void);
int cmgan_rir_tail_max_window(void);
size_t cmgan_rir_tail_workspace_bytes(const cmgan_handle* h, int R, int K, int NB, int NF);
int cmgan_rir_tail(cmgan_handle* h, float* rir_dev, int R, int K, long long ld, int* len_dev, const int* n_taps_dev,
                   const double* decay_dev, const long long* seed_dev, const double* filt_dev, int NB, int NF, int window,
                   int fs, int* status_dev, double* gain_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Active speech level (the reference has no level handling: src/data/dataloader.py:13-50 replays pairs mixed
 * beforehand) ---------------------------------------------------------------------------------------------------------
 * The level meter of ITU-T P.56, method B, as its published description gives it, for B rows x_dev[b * ld + i] of float32
 * samples.  ITU's own program was not available to compare with: the definition below is the contract, and equality with
 * that program is neither claimed nor tested.  lengths_dev is int32 [B] in DEVICE memory, read by the kernels only, or NULL
 * for n = L; n = clamp(lengths[b], 0, L), and samples at i >= n are never read.  fs is a host int.  For row b:
 *   g   = exp(-1 / (0.03 fs))              I = ceil(0.2 fs)              c_j = 2^(j-15), j = 0..14
 *   p_i = g p_{i-1} + (1-g) |x_i|,  q_i = g q_{i-1} + (1-g) p_i,          p_{-1} = q_{-1} = 0
 *   a_j = #{ i < n : q_i' >= c_j for some i' in [i-I, i] }                (activity with a hangover of I samples;
 *                                                                          a_j is non-increasing in j)
 *   sq  = sum_{i < n} x_i^2,  ms = sq / n
 *   J   = #{ j : a_j > 0 };  A_j = 10 log10(sq / a_j),  C_j = 20 log10(c_j),  D_j = A_j - C_j,  M = 15.9
 *   A*  = A_0                                      if D_0 <= M
 *       = A_{j-1} + t (A_j - A_{j-1}),  t = (D_{j-1} - M) / (D_{j-1} - D_j)   for the first j in 1..J-1 with D_j <= M
 *       = A_{J-1}                                  if there is none
 *   active_ms = 10^(A* / 10),  activity = ms / active_ms
 *   outputs   level_dev[b * 3 + 0..2] = {ms, active_ms, activity} (float64);  counts_dev (int64 [B][16], may be NULL)
 *             = {a_0 .. a_14, n}
 * n == 0, sq == 0 or J == 0: all three outputs are 0.  sq not finite: all three are NaN (and the row's a_j mean nothing).
 * All arithmetic is float64 on the VALU.  A block owns a tile of cmgan_speech_level_tile() samples: the recurrence is run
 * per tile from zero state, the tiles' end states are folded in ascending order (a segment of m samples acts on an incoming
 * state as p' = g^m p + P, q' = g^m q + m (1-g) g^m p + Q), every tile reports the first and last crossing of each threshold,
 * and a_j is an integer fold over the tiles.  No atomics; every reduction runs in an order that depends on the tile grid
 * alone, so the same bits come out from run to run, row b's bits depend neither on B nor on the other rows, and a row of
 * length n gives the same bits at every L >= n.
 * Checked before any launch and before the handle is looked at (the message of a call with h == NULL is read with
 * cmgan_last_error(NULL)): null or misaligned pointers (4 bytes for x and lengths, 8 for level and counts), 1 <= B <= 65535,
 * 1 <= L <= 2^31 - 1 - cmgan_speech_level_tile(), ld >= L, 8000 <= fs <= 192000, a workspace that is null, not 256-byte
 * aligned or smaller than cmgan_speech_level_workspace_bytes(B, L) (0 for an unsupported shape; non-decreasing in B and L);
 * each is CMGAN_E_BADARG.  Four launches, no synchronisation, no allocation; graph-capturable, and a replay reads the
 * current contents of x_dev and lengths_dev.                                                                            */
int cmgan_speech_level_tile(void);
size_t cmgan_speech_level_workspace_bytes(int B, int L);
int cmgan_speech_level(cmgan_handle* h, const float* x_dev, int B, int L, long long ld, const int* lengths_dev, int fs,
                       double* level_dev, long long* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Recording channel (the reference has no augmentation: src/data/dataloader.py:13-50 replays pairs mixed beforehand) -
 * Per row a cascade of biquads (microphone / equaliser response, band limit) and a clipping level, for B rows
 * x_dev[b * ldx + i] of float32 samples, written to y_dev[b * ldy + i].  All per-row tables are in DEVICE memory and read by
 * the kernels only: lengths_dev int32 [B] (NULL: n = L), sos_dev float64 [B][S][6] in scipy's layout b0 b1 b2 a0 a1 a2,
 * n_sections_dev int32 [B] (NULL: S for every row), clip_dev float64 [B] (NULL: no clipping; +inf: none for that row),
 * status_dev int32 [B] (may be NULL).  S is a host int in 1 .. cmgan_channel_max_sections() = 8.  For row b, with
 * n = clamp(lengths[b], 0, L) and m = n_sections[b]:
 *   sections 0 .. m-1 in order, each from zero state in float64 (transposed direct form II, scipy.signal.sosfilt's loop):
 *       y_i = b0 u_i + z1,   z1 <- b1 u_i - a1 y_i + z2,   z2 <- b2 u_i - a2 y_i
 *   the result limited to [-clip[b], clip[b]], rounded ONCE to float32, stored for i < n;  y[b, i] = 0 for n <= i < L.
 * m = 0 copies the row (and clips it).  Samples of x at i >= n are never read.  A row is INVALID - status 1 (else 0) and
 * L zeros - when a coefficient of a section it uses is not finite, a0 != 1, a section lies outside the stability triangle
 * (|a2| < 1 and |a1| < 1 + a2), m is outside [0, S], or clip[b] is NaN or <= 0.  A non-finite sample at position i leaves
 * the samples before i as defined; from i on the row is not specified (with a recursive section: non-finite).
 * Method.  The cascade is one linear system in the 2 m states z; a segment of k samples run from zero state, ending in Z,
 * acts on an incoming state as z' = A^k z + Z.  A block owns a tile of cmgan_channel_tile() samples, a thread 8 of them:
 * a prepare launch judges every row and tabulates the powers of A the scans need by repeated squaring, the tiles' end
 * states are found per tile and folded in ascending order, and every thread then runs its samples from its entry state.
 * All arithmetic is float64 on the VALU; no atomics; every reduction runs in an order that depends on the tile grid alone,
 * so the same bits come out from run to run, and row b's bits depend neither on B, nor on the other rows, nor on L beyond
 * n, nor on S beyond the row's own m.
 * y_dev == x_dev with ldy == ldx (in place) is allowed; any other intersection of [x, x + (B-1) ldx + L) with y's span is
 * CMGAN_E_BADARG.  Checked before any launch and before the handle is looked at (the message of a call with h == NULL is
 * read with cmgan_last_error(NULL)): null x / sos / y, misaligned pointers (4 bytes for float32 / int32, 8 for float64),
 * 1 <= B <= 65535, 1 <= L <= 2^31 - 1 - cmgan_channel_tile(), ldx >= L, ldy >= L, 1 <= S <= 8, the overlap above, a
 * workspace that is null, not 256-byte aligned or smaller than cmgan_channel_workspace_bytes(B, L, S) (0 for an unsupported
 * shape; non-decreasing in B, L and S); each is CMGAN_E_BADARG.  Four launches, no synchronisation, no allocation;
 * graph-capturable, and a replay reads the current contents of every device table.                                    */
int cmgan_channel_tile(void);
int cmgan_channel_max_sections(void);
size_t cmgan_channel_workspace_bytes(int B, int L, int S);
int cmgan_channel(cmgan_handle* h, const float* x_dev, int B, int L, long long ldx, const int* lengths_dev,
                  const double* sos_dev, const int* n_sections_dev, int S, const double* clip_dev, float* y_dev,
                  long long ldy, int* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Dynamics: compressor, limiter, automatic gain control (the reference has no augmentation, as above) ---------------
 * Per row a feed-forward gain control in the log domain, the level detector after the gain computer, with the smooth
 * branching peak detector (Giannoulis, Massberg and Reiss, JAES 60 (6), 2012), for B rows wav_dev[b * ldw + i] of float32
 * samples, written to out_dev[b * ldo + i].  The level is taken from key_dev[b * ldk + i] (NULL: from wav itself).  All
 * per-row tables are in DEVICE memory and read by the kernels only: lengths_dev int32 [B] (NULL: n = L), dyn_dev float64
 * [B][6] = (thr_db, slope, knee_db, a_att, a_rel, makeup_db) with slope = 1 - 1 / ratio (1: a limiter) and a = exp(-1 /
 * (t fs)) for a time constant of t seconds; status_dev int32 [B] and peak_reduction_db_dev float64 [B] (each may be NULL).
 * In float64, for row b with n = lengths[b] and the key row k:
 *   xg   = 20 log10(max(|k_i|, 1e-6))                   (a key sample that is not finite counts as silence: c_i = 0)
 *   c_i  = 0                                            if 2 (xg - thr) < -knee
 *        = slope t (t / (2 knee)), t = xg - thr + knee / 2   if 2 |xg - thr| <= knee and knee > 0
 *        = slope (xg - thr)                             otherwise                     (the wanted reduction in dB, >= 0)
 *   y_i  = a_att y_(i-1) + (1 - a_att) c_i  if c_i > y_(i-1)  else  a_rel y_(i-1) + (1 - a_rel) c_i,      y_(-1) = 0
 *   out_i = wav_i 10^((makeup - y_i) / 20), rounded ONCE to float32, for i < n;  out[b, i] = 0 for n <= i < L.
 * peak_reduction_db[b] is the largest y_i of the row (0 for an empty or invalid row).  Samples at i >= n are never read.
 * A row is INVALID - status 1 (else 0) and L zeros - when an entry of its table is not finite, slope is outside [0, 1],
 * knee < 0, a_att or a_rel is outside [0, 1), or lengths[b] is outside [0, L].  A row with slope 0, or with every sample
 * under the knee, and makeup 0 is copied bit for bit; a non-finite wav sample stays at its own index and touches no other.
 * Method.  With a_att <= a_rel a step is y -> max(a_att y + (1 - a_att) c_i, a_rel y + (1 - a_rel) c_i), two increasing
 * affine maps (with a_att > a_rel the same on -y and -c).  Increasing maps distribute over max, so a tile of T =
 * cmgan_dynamics_tile() steps is y -> max over k = 0 .. T of (a_att^k a_rel^(T-k) y + b_k), one offset per number of attack
 * steps, and the offsets follow from a (max, +) recurrence over the tile.  A wave owns a tile and a lane an offset; the
 * tiles' maps are folded per row in ascending order (a serial chain of n / T steps, a fused multiply-add per lane and a
 * wave maximum each), and every tile is then run from its entry state in the branching form above.  Float64 on the VALU;
 * no atomics; the same bits come out from run to run, and row b's bits depend neither on B, nor on the other rows, nor on
 * the strides, nor on L beyond n.  Against the serial loop the detector differs by float64 roundings that depend on T.
 * out_dev == wav_dev with ldo == ldw (in place) is allowed, and so is out_dev == key_dev with ldo == ldk; any other
 * intersection of out's span [out, out + (B-1) ldo + L) with wav's or key's is CMGAN_E_BADARG.  Checked before any launch
 * and before the handle is looked at (the message of a call with h == NULL is read with cmgan_last_error(NULL)): null wav /
 * dyn / out, misaligned pointers (4 bytes for float32 / int32, 8 for float64), 1 <= B <= 65535, 1 <= L <= 2^31 - 1 - 64 x
 * cmgan_dynamics_tile(), ldw >= L, ldo >= L, ldk >= L with a key, the overlaps above, a workspace that is null, not
 * 256-byte aligned or smaller than cmgan_dynamics_workspace_bytes(B, L) (0 for an unsupported shape; non-decreasing in B
 * and L); each is CMGAN_E_BADARG.  Three launches, four with peak_reduction_db; no synchronisation, no allocation;
 * graph-capturable, and a replay reads the current contents of every device table.                                     */
int cmgan_dynamics_tile(void);
size_t cmgan_dynamics_workspace_bytes(int B, int L);
int cmgan_dynamics(cmgan_handle* h, const float* wav_dev, int B, int L, long long ldw, const float* key_dev, long long ldk,
                   const int* lengths_dev, const double* dyn_dev, float* out_dev, long long ldo, int* status_dev,
                   double* peak_reduction_db_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Synthetic noise (the reference has no noise source of its own: its data path replays pairs mixed beforehand) -------
 * out_dev is a float32 [N, K] array, row r at out_dev[r * ld]: a noise of its own colour, modulation, hum and clicks per
 * row, made from a seed and small per-row tables.  All tables are in DEVICE memory and read by the kernels only: seed_dev
 * int64 [N] (the Philox key: low word, high word), start_dev int64 [N] (NULL: 0), len_dev int32 [N] (NULL: K), fir_dev
 * float64 [N][NF], env_dev float64 [N][P] (NULL: no envelope, then P = H = 0), tones_dev float64 [N][M][3] = (nu, amp, phi)
 * with nu in cycles per sample and phi in cycles (NULL exactly when M = 0), n_tones_dev int32 [N] (NULL: M for every row;
 * only with tones_dev), imp_dev float64 [N][2] = (thr, amp), thr a whole number in [0, 2^32) (NULL: no clicks),
 * status_dev int32 [N], written.  In float64, for row r, 0 <= k < len[r] and the absolute sample index n = start[r] + k:
 *   nu[q]  = (w0 + w1 + w2 + w3 - 2 (2^32 - 1)) / CMGAN_RIR_TAIL_NOISE_DIV, (w0 .. w3) = Philox4x32-10 at the counter (q mod
 *            2^32, q div 2^32, 0, 0) under the key seed[r] - for q < 2^32 the nu of cmgan_rir_tail; unit variance; the
 *            numerator is an exact integer, the division is IEEE's
 *   imp[q] = amp ((double)((int64)v1 - 2^31) / 2^31) if v0 < thr, else 0, (v0, v1, ..) = Philox at the counter (q mod 2^32,
 *            q div 2^32, 1, 0); thr = 0: no clicks, and the second block is not computed
 *   e[q]   = nu[q] + imp[q] for q >= 0, 0 for q < 0
 *   s[n]   = sum_{j = 0 .. NF-1} fir[r][j] e[n - j], j ascending, one fma per term into one accumulator from 0
 *   g[n]   = fma(env[r][p1] - env[r][p0], (double)(n - p0 H) / (double)H, env[r][p0]), p0 = min(n div H, P - 1),
 *            p1 = min(p0 + 1, P - 1): the envelope's points lie H samples apart and the last one holds; g = 1 without env
 *   t[n]   = sum_{m < n_tones[r]} amp_m sinpi(2 frac(fma(nu_m, (double)n, phi_m))), m ascending, one fma per term from 0,
 *            frac(x) = x - floor(x), which is exact
 *   out[r, k] = (float) fma(g[n], s[n], t[n]), ONE rounding to float32;  out[r, k] = 0 for len[r] <= k < K.
 * A row is INVALID - status 1 (else 0) and K zeros - when an entry of fir, env or imp of the row, or of the tones it uses,
 * is not finite, len[r] is outside [0, K], n_tones[r] is outside [0, M], a nu_m is outside [0, 0.5], thr is no whole number
 * in [0, 2^32), start[r] < 0 or start[r] + K > 2^40.  Tone columns from n_tones[r] on are never read.
 * Every sample is a pure function of the row's tables and n, so a row made whole and the same row made in pieces, start
 * advanced by the samples already made, have the same bits.  Float64 on the VALU; no atomics; the same bits come out from
 * run to run, and row r's bits depend neither on N, nor on the other rows, nor on ld, nor on K beyond len[r].  Two launches:
 * a judge (one block per row, the verdict goes to the workspace) and the rows on a grid (tile of cmgan_noise_tile() = 256
 * outputs, row), a thread per output: the block computes e once for the 256 + NF - 1 indices its outputs reach and stages
 * it in LDS as float64 (10.2 KB at NF = 1023); the taps, the same for the whole block, come through scalar loads.  With
 * K = 0 only the judge runs (out_dev may be NULL).
 * Checked before any launch and before the handle is looked at (the message of a call with h == NULL is read with
 * cmgan_last_error(NULL)): null out (K > 0) / seed / fir / status, misaligned pointers (4 bytes for float32 / int32, 8 for
 * float64 / int64), 1 <= N <= 65535, 0 <= K <= 2^31 - 1 - cmgan_noise_tile(), ld >= K, 1 <= NF <= cmgan_noise_max_filter()
 * (1023), with env 1 <= P <= cmgan_noise_max_points() (4096) and H >= 1 and without it P = H = 0, 0 <= M <=
 * cmgan_noise_max_tones() (8) with tones NULL exactly when M = 0 and n_tones only beside tones, a workspace that is null, not
 * 256-byte aligned or smaller than cmgan_noise_workspace_bytes(N) (0 for an unsupported N); each is CMGAN_E_BADARG.  No
 * synchronisation, no allocation; graph-capturable, and a replay reads the current contents of every device table.      */
int cmgan_noise_tile(void);
int cmgan_noise_max_filter(void);
int cmgan_noise_max_tones(void);
int cmgan_noise_max_points(void);
size_t cmgan_noise_workspace_bytes(int N);
int cmgan_noise(cmgan_handle* h, float* out_dev, int N, int K, long long ld, const long long* seed_dev,
                const long long* start_dev, const int* len_dev, const double* fir_dev, int NF, const double* env_dev, int P, int H,
                const double* tones_dev, const int* n_tones_dev, int M, const double* imp_dev, int* status_dev,
                void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Speed perturbation (the reference has no counterpart: its data path replays fixed pairs, src/data/dataloader.py) ---
 * Every row of a [B, L] float32 batch x_dev[b * ldx + k] is resampled by its OWN rate into N outputs y_dev[b * ldy + i]:
 * band-limited interpolation with a Hann-windowed sinc.  rate_dev float64 [B] (input samples per output sample: > 1 is
 * faster and higher), lengths_dev int32 [B] (NULL: n = L), out_len_dev and status_dev int32 [B] (each may be NULL) are in
 * DEVICE memory and read / written by the kernel only; zeros (4 .. cmgan_warp_max_zeros() = 64 zero crossings on either
 * side) and rolloff (0.5 .. 1, the cutoff as a fraction of the lower Nyquist rate) are host values.  In float64, for row
 * b with n = lengths[b] and r = rate[b]:
 *   t_i  = fl(i r)                                 the time of output i: ONE rounded product
 *   M    = min(N, #{i >= 0 : t_i < n})             out_len[b]; what cmgan_warp_out_len(n, r) returns before the min
 *   fc   = rolloff (r > 1 ? 1 / r : 1),  W = zeros / fc
 *   h(d) = fc sinc(fc d) (0.5 + 0.5 cospi(d / W)) for |d| < W, else 0;   sinc(z) = sinpi(z) / (pi z), sinc(0) = 1
 *   y[b, i] = f32( sum_k x[b, k] h(t_i - k) )      over the integers k with |t_i - k| < W and 0 <= k < n, ascending;
 *                                                  ONE rounding to float32;  y[b, i] = 0 for M <= i < N
 * Samples of x at k >= n are never read.  r = 1 with rolloff = 1 copies the row bit for bit.  A row is INVALID - status 1
 * (else 0), out_len 0 and N zeros - when its rate is not a finite number in [1 / cmgan_warp_max_rate(),
 * cmgan_warp_max_rate()] = [1/4, 4] or its length lies outside [0, L].  An output whose support holds a non-finite sample
 * is non-finite; the others are not affected.
 * Method.  A block owns cmgan_warp_tile() consecutive outputs of one row, a thread one of them; the input span of the
 * tile is staged on chip.  The sine of the sinc and the cosine of the window fall by a constant angle from tap to tap: a
 * thread evaluates sinpi / cospi at its first tap and turns the two (sin, cos) pairs by the angle-addition identities
 * from there; the taps with |d| < 1 take sinpi(fc d) and cospi(d / W) directly.  With fc = 1 the turn is exactly
 * (-1, 0), so integer times keep an exact zero sine.  No atomics, no workspace; row b's bits depend neither on B, nor
 * on the other rows, nor on the padding behind ldx / ldy, nor on L beyond n.
 * cmgan_warp_out_len is pure host arithmetic: ceil(n / r) corrected by single steps until fl((M - 1) r) < n <= fl(M r);
 * -1 for n < 0, n > 2^50 or a rate outside [1/4, 4].
 * Checked before the launch and before the handle is looked at (the message of a call with h == NULL is read with
 * cmgan_last_error(NULL)): null x / rate / y, misaligned pointers (4 bytes for float32 / int32, 8 for the rates),
 * 1 <= B <= 65535, L >= 1, N >= 1, ldx >= L, ldy >= N, 4 <= zeros <= 64, 0.5 <= rolloff <= 1, any intersection of
 * [x, x + (B-1) ldx + L) with [y, y + (B-1) ldy + N); each is CMGAN_E_BADARG.  One launch, no synchronisation, no
 * allocation; graph-capturable, and a replay reads the current contents of x, the rates and the lengths.            */
int cmgan_warp_tile(void);
double cmgan_warp_max_rate(void);
int cmgan_warp_max_zeros(void);
long long cmgan_warp_out_len(long long n, double rate);
int cmgan_warp(cmgan_handle* h, const float* x_dev, int B, int L, long long ldx, const int* lengths_dev,
               const double* rate_dev, int zeros, double rolloff, float* y_dev, int N, long long ldy, int* out_len_dev,
               int* status_dev, void* stream);

/* ---- Tempo perturbation (the reference has no counterpart: its data path replays fixed pairs, src/data/dataloader.py) ---
 * Every row of a [B, L] float32 batch x_dev[b * ldx + k] is time-stretched by its OWN rate into N outputs
 * y_dev[b * ldy + i] with the pitch kept: WSOLA (waveform-similarity overlap-add, Verhelst & Roelands 1993), the
 * time-domain method that splices the waveform at pitch-synchronous points.  rate_dev float64 [B] (input time per output
 * time: > 1 is faster, the sense of cmgan_warp), lengths_dev int32 [B] (NULL: n = L), out_len_dev, status_dev and
 * searched_dev int32 [B] and pos_dev int32 [B][ceil(N / hop)] (each may be NULL) are in DEVICE memory and read / written
 * by the kernel only; hop = H (16 .. cmgan_stretch_max_hop() = 1024) and search = D (0 .. cmgan_stretch_max_search() =
 * 1024) are host values.  For row b with n = lengths[b] and r = rate[b]; x[k] reads as 0 for every k outside [0, n):
 *   M    = min(N, #{i >= 0 : fl(i r) < n})         out_len[b]: cmgan_warp's count, so stretch and warp agree on lengths;
 *                                                  K = ceil(M / H) frames, the last one may be partial
 *   p_k  = floor(fl((k H) r))                      the nominal position: k H is an exact integer, ONE rounded float64
 *                                                  product per frame; k H < M gives 0 <= p_k < n
 *   q_0  = c_0 = 0;   c_k = q_{k-1} + H            the natural continuation of the previous segment, for k >= 1
 *   q_k  = c_k                                     if |c_k - p_k| <= D and 0 <= c_k < n: no search, the frame is a copy
 *   q_k  = the candidate q = p_k + d, |d| <= D, 0 <= q < n (d = 0 is always one), with the largest score otherwise:
 *          s(d) = 2 C - E,   C = sum_{i=0}^{H-1} x[q + i] x[c_k + i],   E = sum_{i=0}^{H-1} x[q + i]^2,
 *          each a float64 sum in ascending i (maximising 2 C - E minimises the squared difference to the continuation);
 *          a NaN score counts as -inf; among equal maxima the earliest in the order d = 0, -1, +1, -2, +2, ... wins, so
 *          silence, a constant row and an all-NaN row take d = 0
 *   f[i] = 0.5 - 0.5 cospi(i / H),   g[i] = fl(1 - f[i])          float64: a 50 % Hann overlap-add of x[q_k .. q_k + 2 H)
 *   y[b, k H + i] = f32( f[i] x[q_k + i] + g[i] x[c_k + i] )      for 0 <= i < H and k H + i < M;   y[b, i] = 0 for M <= i < N
 *   pos[b, k] = q_k for k < K and -1 for K <= k < ceil(N / H);   searched[b] = the frames that were searched
 * Where q_k = c_k the frame is the input bit for bit (finite samples): r = 1 copies the row, r = 1.0001 copies long runs and
 * splices rarely.  A product of two float32 values is exact in float64, so fused and unfused multiply-adds give the same
 * sums in ascending order and the positions q_k are exactly reproducible: a host model finds the same ones.  Only the
 * cross-fade line depends on the contraction of multiply-adds and on the device's cospi.  Samples of x at k >= n are never
 * read.  A row is INVALID - status 1 (else 0), out_len 0, N zeros, every pos -1, searched 0 - when its rate is not a finite
 * number in [1 / cmgan_warp_max_rate(), cmgan_warp_max_rate()] = [1/4, 4] or its length lies outside [0, L]; n = 0 is
 * valid with out_len 0.  Non-finite samples are no error: the rules above stay defined (a NaN score counts as -inf), the
 * outputs follow IEEE arithmetic, and no other row is affected.
 * Method.  The frames of a row form a serial chain, so one block owns a row and walks its frames: a batch of B rows keeps B
 * compute units busy.  A searched frame stages the candidate span and the continuation on chip; every candidate has a
 * thread of its own, which runs both sums in one ascending chain; the best (score, visiting rank) is reduced by wave
 * shuffles and one step through LDS, in an order that cannot change the winner because the order on that key is total.
 * No atomics, no workspace; row b's bits depend neither on B, nor on the other rows, nor on the padding behind ldx / ldy,
 * nor on L beyond n.
 * Checked before the launch and before the handle is looked at (the message of a call with h == NULL is read with
 * cmgan_last_error(NULL)): null x / rate / y, misaligned pointers (4 bytes for float32 / int32, 8 for the rates),
 * 1 <= B <= 65535, L >= 1, N >= 1, ldx >= L, ldy >= N, 16 <= hop <= 1024, 0 <= search <= 1024, any intersection of
 * [x, x + (B-1) ldx + L) with [y, y + (B-1) ldy + N); each is CMGAN_E_BADARG.  One launch, no synchronisation, no
 * allocation; graph-capturable, and a replay reads the current contents of x, the rates and the lengths.            */
int cmgan_stretch_max_hop(void);
int cmgan_stretch_max_search(void);
int cmgan_stretch(cmgan_handle* h, const float* x_dev, int B, int L, long long ldx, const int* lengths_dev,
                  const double* rate_dev, int hop, int search, float* y_dev, int N, long long ldy, int* out_len_dev,
                  int* status_dev, int* pos_dev, int* searched_dev, void* stream);

/* ---- Transmission: codec, packet loss and concealment (the reference has no counterpart: its data path replays fixed
 * pairs, src/data/dataloader.py, so the enhancer never meets speech that came over a telephone or VoIP link) -----------
 * Every row of a [B, L] float32 batch x_dev[b * ldx + k] is companded by its OWN codec, loses its OWN frames and has the
 * holes covered by repeating the last pitch period (after ITU-T G.711 Appendix I, simplified so that every step is
 * stated) or left as gaps; the result is y_dev[b * ldy + k].  lengths_dev int32 [B] (NULL: n = L), lost_dev uint8
 * [B][ldl] (non-zero: the frame is lost), codec_dev and plc_dev int32 [B], status_dev int32 [B] and lag_dev int32 [B][ldl]
 * (the last two may be NULL) are in DEVICE memory and read / written by the kernels only; frame = F (16 .. 4096), pmin and
 * pmax (the lag range, 16 <= pmin <= pmax <= cmgan_transmit_max_lag() = 1024), window = W (the matching window, 16 ..
 * cmgan_transmit_max_window() = 1024) and fade = A (the fade unit, >= 1) are host values.  For row b with n = lengths[b]
 * and K = ceil(n / F); table columns k >= K and samples at i >= n are never read:
 *   1. Codec.  z[i] = codec(x[i]) for 0 <= i < n.
 *        0  none: z is x bit for bit, NaN included
 *        1, 2, 3 start from q = sat16(rint(x[i] * 32768)): round half to even, NaN -> 0, +-inf saturate
 *        1  16-bit PCM: z = q / 32768
 *        2  G.711 mu-law: z = ulaw2lin(lin2ulaw(q)) / 32768
 *        3  G.711 A-law:  z = alaw2lin(lin2alaw(q)) / 32768        (both maps exactly those of Python's audioop at width 2)
 *   2. Loss.  y starts as z.  A run is a maximal set of consecutive lost frames k0 .. k1 - 1, s = k0 F, e = min(k1 F, n);
 *      runs are handled in ascending order; h(i) = y[i] as it stands for 0 <= i < s, earlier concealment included, and 0
 *      for i < 0.
 *        plc = 0:  y[s .. e) = 0; nothing else changes.
 *        plc = 1:
 *          lag     P = the pmin <= P <= pmax with the largest 2 C - E,  C = sum_{i<W} h(s-W+i) h(s-W-P+i),  E = sum_{i<W}
 *                  h(s-W-P+i)^2, float64 sums in ascending i (the score and the arithmetic of cmgan_stretch; products of
 *                  float32 values are exact); a NaN score counts as -inf; among equal maxima the smallest P wins, so
 *                  silence, and a run at the start of the row, take pmin
 *          period  Q = floor(P / 4);  v[i] = h(s-P+i) for 0 <= i < P - Q;  v[i] = fl(1-t) h(s-P+i) + t h(s-2P+i) with t =
 *                  (i - (P-Q) + 1) / (Q + 1) for P - Q <= i < P: the buffer ends where it begins
 *          gain    g(j) = min(1, max(0, (6A - j) / (5A))): an exact integer numerator and one IEEE division; 1 for the
 *                  first A samples, then falling by 20 % per A, 0 from 6A on
 *          fill    y[s+j] = f32(g(j) v[j mod P]) for 0 <= j < e - s; where g = 1 and j mod P < P - Q the sample is a bit
 *                  copy of the history
 *          fade back (if e < n)  R = min(Q, F, n - e), M = e - s, and for 0 <= i < R with t = (i + 1) / (R + 1):
 *                  y[e+i] = f32(fl(1-t) g(M+i) v[(M+i) mod P] + t z[e+i]); frame k1 is good, so the fade stays inside it
 *        Float64 arithmetic with one rounding to float32 per stored sample.
 *   y[i] = 0 for n <= i < L;  status[b] = 0;  lag[b, k] = P at the frame that starts a concealed run, 0 at every other
 *   frame k < K, -1 for K <= k < ldl.
 * A row is INVALID - status 1, L zeros, every lag -1 - when its codec lies outside 0 .. 3, its plc outside 0 .. 1 or its
 * length outside [0, L].  codec = 0 with no lost frame copies the row bit for bit.  Non-finite samples are no error.
 * Method.  Step 1 is one elementwise launch over the batch, 8 bytes per sample.  The concealment is a serial chain along
 * a row (a later loss conceals from a history that may itself be concealed), so in step 2 one block owns a row and walks
 * its runs: a batch of B rows keeps B compute units busy.  A run stages W + pmax history samples and v on chip as float64
 * (24 KB at most); every lag has a thread of its own, which runs both sums in one ascending chain; the best (score, P)
 * is reduced by wave shuffles and one step through LDS, in an order that cannot change the winner because the order on
 * that key is total; the block reads its own earlier writes to y back behind a barrier.  No atomics, no workspace; row
 * b's bits depend neither on B, nor on the other rows, nor on the padding behind ldx / ldy, nor on table columns from K
 * on, nor on L beyond n.
 * Checked before the launch and before the handle is looked at (the message of a call with h == NULL is read with
 * cmgan_last_error(NULL)): null x / lost / codec / plc / y, pointers to float32 / int32 that are not 4-byte aligned,
 * 1 <= B <= 65535, L >= 1, ldx >= L, ldy >= L, 16 <= frame <= 4096, 16 <= pmin <= pmax <= 1024, 16 <= window <= 1024,
 * fade >= 1, ldl >= ceil(L / frame), and any intersection of [x, x + (B-1) ldx + L) with [y, y + (B-1) ldy + L) other than
 * y == x with ldy == ldx (in place); each is CMGAN_E_BADARG.  Two launches, no synchronisation, no allocation;
 * graph-capturable, and a replay reads the current contents of x, the tables and the lengths.                      */
int cmgan_transmit_max_lag(void);
int cmgan_transmit_max_window(void);
int cmgan_transmit(cmgan_handle* h, const float* x_dev, int B, int L, long long ldx, const int* lengths_dev,
                   const unsigned char* lost_dev, long long ldl, const int* codec_dev, const int* plc_dev, int frame,
                   int pmin, int pmax, int window, int fade, float* y_dev, long long ldy, int* status_dev, int* lag_dev,
                   void* stream);

/* ---- Suppression: the recording device's own noise suppressor (the reference has no counterpart: its data path replays
 * fixed pairs, src/data/dataloader.py, so the enhancer never meets what a phone's or a headset's suppressor leaves behind;
 * the same call is the classical baseline - Wiener, spectral subtraction, Ephraim and Malah's log-MMSE) -----------------
 * Every row of a [B, L] float32 batch x_dev[b * ldx + k] goes through a short-time spectral gain of its OWN; the result is
 * y_dev[b * ldy + k].  key_dev (NULL: the key is x) is a batch of the same shape whose spectrum drives the gains.
 * lengths_dev int32 [B] (NULL: n = L), table_dev float64 [B][7], status_dev int32 [B] and gain_dev float64 [B][T][F] (the
 * last two may be NULL) are in DEVICE memory and read / written by the kernels only.  n_fft = N is a host value, 256, 512
 * or 1024; h = N / 2 (the hop), F = N / 2 + 1, T = ceil(L / h) + 1.  A table row is
 *   0 rule    0 off, 1 Wiener, 2 power spectral subtraction, 3 log-MMSE            an integer 0 .. 3
 *   1 a_dd    decision-directed smoothing                                          [0, 1)
 *   2 a_n     periodogram smoothing                                                [0, 1)
 *   3 D       minimum-search window in frames                                      an integer 1 .. cmgan_suppress_max_window() = 128
 *   4 bias    noise over-estimation                                                (0, 16]
 *   5 g_min   gain floor                                                           (0, 1]
 *   6 xi_min                                                                       [0, 1]
 * For row b with n = lengths[b], T_b = ceil(n / h) + 1 (0 when n = 0) and w[k] = sin(pi k / N), the square root of the
 * periodic Hann window (w[k]^2 + w[k + h]^2 = 1):
 *   1. Analysis.  Frame t holds s_t[k] = x~[(t - 1) h + k] w[k], k = 0 .. N-1, with x~ the row as float64 inside [0, n) and 0
 *      outside; Y_t[f] = sum_k s_t[k] e^{-2 pi i f k / N}, K_t the same from the key, A_t[f] = Re(K_t[f])^2 + Im(K_t[f])^2.
 *   2. Gain, per bin f, t ascending:
 *        P_t   = a_n P_{t-1} + (1 - a_n) A_t,  P_{-1} = A_0
 *        lam_t = max(bias min_{max(0, t-D+1) <= u <= t} P_u, 2^-60)
 *        gam_t = min(A_t / lam_t, 40)
 *        xi_t  = max(a_dd G_{t-1}^2 gam_{t-1} + (1 - a_dd) max(gam_t - 1, 0), xi_min)        (t = 0: without the first term)
 *        q     = xi_t / (1 + xi_t)
 *        G     = q (rule 1);  sqrt(q) (rule 2);  min(q exp(E1(max(q gam_t, 2^-30)) / 2), 1) (rule 3);   G_t = max(G, g_min)
 *      E1 is the exponential integral, by two fixed formulas:
 *        x < 2:   E1(x) = (-gamma - ln x) + x s_1,  s_K = c_K,  s_k = fma(s_{k+1}, x, c_k),  c_k = (-1)^(k+1) / (k k!), K = 26 (k!
 *                 a running float64 product, gamma = 0.5772156649015329);
 *        x >= 2:  E1(x) = e^-x d / n from the continued fraction e^-x / (x + 1 - 1 / (x + 3 - 4 / (x + 5 - 9 / ...))) cut at
 *                 depth 40 and run backwards: (n, d) = (x + 81, 1), then for k = 40 .. 1: (n, d) <- ((x + 2 k - 1) n - k^2 d, n).
 *      Both are within 1e-15 (absolute) of E1 on [2^-30, 45]; only the absolute error reaches G.
 *   3. Synthesis.  Z_t = G_t Y_t, z_t its real inverse transform with the factor 1 / N; for 0 <= i < n, t = floor(i / h), r =
 *      i mod h:   y[i] = f32(z_t[r + h] w[r + h] + z_{t+1}[r] w[r]),  the earlier frame first.
 *   y[i] = 0 for n <= i < L (samples from n on are never read);  status[b] = 0;  gain[b, t, f] = G_t[f] for t < T_b, 0 for T_b
 *   <= t < T.
 * Rule 0 copies the row's n samples bit for bit, NaN included, computes nothing and reports gains of 1.  A row is INVALID
 * - status 1, L zeros, gains 0 - when a table entry is not finite or outside its range, rule or D is no integer, or the
 * length lies outside [0, L]; the other entries are judged at rule 0 too.  Non-finite samples are no error: they stay in
 * their row.  Float64 arithmetic with one rounding to float32 per sample; every step is a continuous function of its
 * inputs, so a float64 model agrees to rounding.
 * Method.  Three launches.  A block per (row, frame) windows the frame into LDS as complex float64, runs a radix-2 transform
 * there and writes bins 0 .. N / 2 to the workspace (complex128 [B][T][F]) and A to a float64 [B][T][F] plane; with a key the
 * same code runs again on the key's frame, so a key that is x gives the bits of no key.  The gain is a serial chain along
 * t per (row, bin): a thread per bin, a wave per 64 consecutive bins, G written over A; the sliding minimum is exact (a
 * ring of D values per thread in LDS, suffix minima of the last block of D frames and a running prefix of this one).  A
 * block per (row, h outputs) then rebuilds the two frames its span needs and adds them in the stated order.  No atomics;
 * row b's bits depend neither on B, nor on the other rows, nor on the padding behind ldx / ldk / ldy, nor on L beyond n.
 * cmgan_suppress_workspace_bytes(B, L, n_fft) is what ws must hold (256-byte aligned; 24 B T F bytes, each plane rounded
 * up to 256; 0 for a shape the kernels do not take).
 * Checked before the launch and before the handle is looked at (the message of a call with h == NULL is read with
 * cmgan_last_error(NULL)): null x / table / y, pointers to float32 / int32 that are not 4-byte aligned, float64 pointers
 * that are not 8-byte aligned, n_fft other than 256 / 512 / 1024, 1 <= B <= 65535, 1 <= L <= 2^31 - 1 - 2048, ldx >= L, ldy
 * >= L, ldk >= L with a key, any intersection of y's span with x's other than y == x with ldy == ldx (in place) and with the
 * key's other than y == key with ldy == ldk, and the workspace; each is CMGAN_E_BADARG.  No synchronisation, no
 * allocation; graph-capturable, and a replay reads the current contents of x, the key, the table and the lengths.   */
int cmgan_suppress_max_window(void);
size_t cmgan_suppress_workspace_bytes(int B, int L, int n_fft);
int cmgan_suppress(cmgan_handle* h, const float* x_dev, int B, int L, long long ldx, const float* key_dev, long long ldk,
                   const int* lengths_dev, const double* table_dev, int n_fft, float* y_dev, long long ldy, int* status_dev,
                   double* gain_dev, void* ws, size_t ws_bytes, void* stream);

/* ---- Auxiliary losses: multi-resolution STFT loss and negative SI-SDR with their gradient (the reference has no
 * counterpart: its generator loss sees one 400-point resolution and a sample-wise L1, src/train.py:124-151) ------------
 * est, ref float32 [B, L], contiguous.  n_fft_host: n_res (1 .. cmgan_aux_loss_max_resolutions() = 4) DISTINCT values from
 * {256, 512, 1024, 2048}, a HOST array read at call time.  All arithmetic is float64; every float32 output is rounded once.
 * Per resolution n: hop h = n / 4, periodic Hann window w[k] = 0.5 - 0.5 cos(2 pi k / n), frames centred with reflect
 * padding of n / 2 as torch.stft(center=True, pad_mode="reflect") (so L > max n / 2), T = 1 + L / h frames (integer
 * division), F = n / 2 + 1 bins, and with X_x[t, f] the windowed frame's DFT of x in {e = est, r = ref}:
 *   m_x = sqrt(max(|X_x|^2, 1e-7))      (below the clamp the derivative with respect to X is 0)
 *   N = sum (m_r - m_e)^2,  D = sum m_r^2 over (t, f);   sc = sqrt(N) / sqrt(D), sc = 0 with a zero derivative where N == 0
 *   lm = mean over (t, f) of |ln m_r - ln m_e|, sign(0) = 0 in its derivative
 * Per row b: MR_b = mean over the resolutions of (sc + lm), and with x' = x - mean(x):
 *   a = <e', r'> / (<r', r'> + 1e-8),  s = a r',  q = e' - s,  SISDR_b = 10 log10((<s, s> + 1e-8) / (<q, q> + 1e-8))  [dB]
 *   (the five sums of e, r, e e, r r, e r are formed in one pass and centred afterwards)
 *   dSISDR / de = (10 / ln 10) (ce e' + cr r'),  ce = -2 / Q,  cr = 2 a R / ((R + 1e-8) S) + (2 a / Q) (1 + 1e-8 / (R + 1e-8)),
 *   R = <r', r'>, S = <s, s> + 1e-8, Q = <q, q> + 1e-8
 * Total A = sum over b ascending of (k_mr MR_b - k_si SISDR_b); the caller passes k_mr = w_mr / B and k_si = w_si / B, so a
 * row's outputs depend on its own samples and the two scalars only.  A term whose weight is exactly 0 is left out of A and
 * of the gradient (its values are still written).  Outputs:
 *   rows_dev     float64 [B, 2 n_res + 1]: (sc, lm) per resolution in the caller's order, then SISDR_b
 *   total_dev    float32 [3]: A, its multi-resolution part, its SI-SDR part
 *   g_audio_dev  float32 [B, L] = dA / de, with the adjoint of the reflect padding (margin samples fold back onto the
 *                interior; per sample: the resolutions in the caller's order, in each the sample's own position, then its
 *                mirror in the left margin, then in the right one, each over its up to four frames ascending; then the
 *                SI-SDR term), or NULL for the values alone (rows and total then have the bits they have with a gradient).
 *                It may not overlap est or ref: the gradient is not formed in place.  ref is data and gets no gradient.
 * A row with est == ref bit for bit has sc = lm = 0 exactly in every resolution (both signals pass through one loop
 * body), and with k_si = 0 a gradient of exact zeros; an all-zero est row has a gradient of exact zeros.  Fixed-order
 * reductions, no atomics: bit-reproducible, row-independent (a non-finite sample stays in its row's outputs and in the
 * total).  The workspace (256-byte aligned) holds, per resolution, the estimate's spectra as complex128 [B, T, F] (the
 * frame gradients overwrite them), m_r as float64 [B, T, F] and three partial sums per frame, then the SI-SDR tiles.
 * cmgan_aux_loss_workspace_bytes returns 0 for arguments cmgan_aux_loss rejects (its handle is not read and may be
 * NULL).  CMGAN_E_BADARG before anything is launched: a null est / ref / rows / total, a resolution outside the set, a
 * duplicate, n_res outside 1 .. 4, L <= max n / 2, B outside 1 .. 65535, a NaN weight, g_audio over est or ref, a
 * workspace that is too small or misaligned.  n_res + 3 launches without a gradient, up to 2 n_res + 4 with one; no host
 * synchronisation, no allocation; graph-capturable, and a replay reads the current contents of est and ref.           */
int cmgan_aux_loss_max_resolutions(void);
size_t cmgan_aux_loss_workspace_bytes(cmgan_handle* h, int B, int L, int n_res, const int* n_fft_host);
int cmgan_aux_loss(cmgan_handle* h, const float* est_dev, const float* ref_dev, int B, int L, int n_res,
                   const int* n_fft_host, double k_mr, double k_si, double* rows_dev, float* total_dev, float* g_audio_dev,
                   void* ws, size_t ws_bytes, void* stream);

/* cmgan_loss_backward with a caller's waveform gradient: g_audio [B, hop (T-1)] float32 (the gradient of any further
 * audio-domain term with respect to est_audio, cmgan_aux_loss's for one) is added to the time term's per-sample gradient
 * w_time sign(est - clean) / (B La) before the window and envelope step of the istft adjoint.  With w_time = 0 and a
 * g_audio, est_audio and clean_audio may be NULL.  g_audio = NULL is cmgan_loss_backward itself: the same launch, the
 * same bits.                                                                                                        */
int cmgan_loss_backward_aux(cmgan_handle* h, const float* est_real_dev, const float* est_imag_dev,
                            const float* clean_spec_dev, int B, int T, const float* est_audio_dev,
                            const float* clean_audio_dev, float w_ri, float w_mag, float w_time,
                            const float* g_audio_dev, float* d_real_dev, float* d_imag_dev, void* stream);

/* ---- Intelligibility loss: negative STOI / ESTOI of an estimate against a reference, with its gradient ----------------
 * est, ref float32 [B, L], contiguous, fs = 16000 only.  The forward is cmgan_metrics' STOI sum for sum (Taal et al. 2011 as
 * the reference's compute_metrics.py has it, quirks included); extended = 1 is ESTOI (Jensen and Taal 2016) on the same
 * envelopes.  All arithmetic is float64; every float32 output is rounded once.  Per row, for x in {e = est, r = ref}:
 *   x10[n] = sum over i ascending of x[i] h[(n + 11) 8 - 5 i]: scipy.signal.resample_poly(x, 5, 8), h = table 4 of
 *            cmgan_metrics_table(16000, ...) (169 taps with the pre-pad), N10 = ceil(5 L / 8) samples
 *   level[s] = 20 log10(sqrt(sum_m (r10[128 s - 1 + m] hann[m])^2) / 16), m < 256 (read ONE SAMPLE EARLY, index -1 wraps to
 *            N10 - 1), s < nS = ceil((N10 - 256) / 128), hann = table 3; frame s is KEPT iff ((level[s] - max level) + 40) > 0,
 *            decided from the reference alone; K kept frames src[0] < .. < src[K - 1]
 *   xs[t] = sum over p in (t / 128 - 1, t / 128) with 0 <= p < K, earlier first, of x10[128 src[p] + o] hann[o], o = t - 128 p
 *   X_k[j] = sum_n xs[128 j + n] hann[n] e^{-2 pi i k n / 512}, n < 256, envelope frames j < K - 1 (one radix-2 loop for both
 *            signals); env_x[band, j] = sqrt(sum over the band's bins k ascending of |X_k / ws|^2), ws = sum hann, the 15
 *            one-third-octave bands of table 2
 *   window w < K - 30 covers frames w .. w + 29; with X = env_r, Y = env_e there, sums over the frames i ascending:
 *     extended = 0: per band alpha = sqrt(sum X^2 / sum Y^2), y'_i = min(Y_i alpha, X_i (1 + 10^(15/20))),
 *            xn = (X - mean X) / |X - mean X|, yn = (y' - mean y') / |y' - mean y'|, s_band = sum_i xn_i yn_i;
 *            d_w = (sum over the bands ascending of s_band) / 15
 *     extended = 1: both 15 x 30 matrices get every row (band) minus its mean over the 30 frames and divided by its norm,
 *            then every column (frame) minus its mean over the 15 bands and divided by its norm (cx, cy); no clipping, no
 *            alpha; d_w = (sum over the frames ascending of (sum over the bands ascending of cx cy)) / 30
 *   STOI_b = (sum of d_w, the block's tree of metrics_finalize) / (K - 30)
 * Total A = sum over b ascending of (-k STOI_b) over the rows WITHOUT a status; the caller passes k = w / B, so a row's
 * outputs depend on its own samples and k only.  Outputs:
 *   rows_dev     float64 [B, 2]: (STOI_b, K)
 *   total_dev    float32 [1]: A
 *   status_dev   int32 [B]: bit 0 = fewer than 31 kept frames (no window), bit 1 = the value is not finite (an all-zero est
 *                gives sum Y^2 = 0).  A row with a status has NaN for its value, is left out of A and gets a gradient of
 *                exact zeros: one silent clip does not put NaN into a training step
 *   g_audio_dev  float32 [B, L] = dA / de, or NULL for the values alone (rows, total and status then have the bits they have
 *                with a gradient).  It may not overlap est or ref.  ref, the keep mask and all that is made of ref are
 *                constants.  Every stage is a gather in ascending order (no atomics), c_b = -k / (K - 30):
 *     D_w[band, i] = d d_w / d Y[band, w + i]:
 *       extended = 0: u_i = (xn_i - yn_i s_band) / |y' - mean y'|, q_i = u_i - mean u, m_i = 1 where Y_i alpha <= X_i (1 + c)
 *            (the derivative of min follows the selected branch, the estimate's at a tie), T = sum_i m_i q_i Y_i,
 *            D_w[band, i] = (m_i q_i alpha - (alpha / sum Y^2) T Y_i) / 15
 *       extended = 1: dc = cx / 30; per frame over the bands: u = (dc - cy (cy . dc)) / nu, da = u - mean u; per band over
 *            the frames: v = (da - ya (ya . da)) / n, D_w[band, .] = v - mean v   (ya the row-normalised estimate, n its row
 *            norm, nu the column norm of the second step)
 *     1. g[band, j] = c_b (sum over w = max(0, j - 29) .. min(j, K - 31) ascending of D_w[band, j - w])
 *     2. G_k = g[band, j] Y_k[j] / (ws^2 env_e[band, j]) on the band's bins (0 where env_e == 0) and 0 on all others;
 *        z[j, n] = hann[n] Re sum_k G_k e^{+2 pi i k n / 512}, n < 256: one conjugate 512-point transform per frame
 *     3. g10[n] = sum over s in (n / 128 - 1, n / 128) with 0 <= s < nS and s kept as src[p], earlier first, of
 *        hann[o] (sum over j in (t / 128 - 1, t / 128) with 0 <= j < K - 1, earlier first, of z[j, t - 128 j]),
 *        o = n - 128 s, t = 128 p + o
 *     4. g_audio[i] = (float) sum over n ascending of g10[n] h[(n + 11) 8 - 5 i] over the taps that exist
 * A row with est == ref bit for bit has STOI_b (extended = 0) equal to what cmgan_metrics gives it.  Fixed-order
 * reductions: bit-reproducible, row-independent, never in place.  The workspace (256-byte aligned) holds the tables, both
 * 10 kHz signals, levels, the keep maps, both envelopes, the estimate's bins 0 .. 255 per frame (the backward reads them
 * and does not transform twice), d_w, D_w, the frame gradients and g10; the kept-frame counts are read from it and the
 * grids are sized for the worst case.  cmgan_stoi_loss_workspace_bytes returns 0 for a shape cmgan_stoi_loss rejects (its
 * handle is not read and may be NULL).  Before anything is launched: CMGAN_E_UNSUPPORTED for fs != 16000; CMGAN_E_BADARG
 * for a null est / ref / rows / total / status, a misaligned buffer, B outside 1 .. 65535, an L too short for 31 frames at
 * 10 kHz (L < 6554), extended outside {0, 1}, a NaN k, g_audio over est or ref, a workspace that is too small or
 * misaligned.  8 launches without a gradient, 11 with one; no host synchronisation, no allocation; graph-capturable, and
 * a replay reads the current contents of est and ref.                                                                */
size_t cmgan_stoi_loss_workspace_bytes(cmgan_handle* h, int B, int L, int fs);
int cmgan_stoi_loss(cmgan_handle* h, const float* est_dev, const float* ref_dev, int B, int L, int fs, int extended, double k,
                    double* rows_dev, float* total_dev, int* status_dev, float* g_audio_dev, void* ws, size_t ws_bytes,
                    void* stream);

/* ---- Phase loss: the anti-wrapping phase terms of MP-SENet (Lu, Ai, Ling 2023) on the emitted spectrum, with their gradient --
 * est_real, est_imag float32 [B, T, F] (the [B, 1, T, F] TSCNet outputs), clean_spec float32 [B, 2, T, F], contiguous; F is
 * the handle's num_features (1 .. 1024).  The power compression keeps the angle, so the angle of est_real + i est_imag against
 * the angle of clean_spec is the phase error in the model's own domain.  All arithmetic is float64; every float32 output is
 * rounded once.  Per cell (t, f) of row b:
 *   p = atan2(est_imag, est_real),  q = atan2(clean_im, clean_re)
 *   r(x) = remainder(x, TWO_PI), the IEEE operation (exact), TWO_PI the double nearest 2 pi;  AW(x) = |r(x)|;
 *   s(x) = the sign of r(x), 0 at r = 0
 *   the cell is VOID when re^2 + im^2 of the estimate or of the clean cell (exact float64 squares, their sum rounded once)
 *   is 0 or below floor * floor, or one of its four inputs is not finite; a void cell makes void every term it is part of
 * Per row b, over the row's own non-void terms only:
 *   ip_b  = (sum of AW(p - q) over the cells) / N_ip
 *   gd_b  = (sum of AW((p[t,f] - p[t,f-1]) - (q[t,f] - q[t,f-1])) over the pairs with f >= 1) / N_gd
 *   iaf_b = (sum of AW((p[t,f] - p[t-1,f]) - (q[t,f] - q[t-1,f])) over the pairs with t >= 1) / N_iaf
 * N_ip, N_gd, N_iaf count the non-void terms: integers, constants of the gradient.  A term with count 0 has value 0, no
 * gradient and a status bit (T = 1 has no IAF pair).  MP-SENet's matrix form of the group delay also carries a boundary
 * column for f = 0; it is LEFT OUT here: only differences of neighbours enter.
 * Order of summation: a row is cut into tiles of cmgan_phase_loss_tile_frames() = 8 frames; a pair belongs to the tile of
 * its later cell.  Thread j of the tile's 256 adds the terms of its bins f = j, j + 256, .. over the tile's frames ascending,
 * bins ascending within a frame; the 256 threads are added by halving (j += j + 128, then + 64, .. + 1); the tiles of a row
 * are added ascending.  Total: x_i = k_i value_i (left out, 0, where k_i == 0 exactly), A = sum over b ascending of
 * (x_ip + x_gd) + x_iaf, each part the sum over b ascending of its x.  The caller passes k = w / B, so a row's outputs
 * depend on its own cells and k only.  Outputs:
 *   rows_dev    float64 [B, 3]: (ip_b, gd_b, iaf_b)
 *   counts_dev  int32 [B, 3]: (N_ip, N_gd, N_iaf)
 *   total_dev   float32 [4]: (A, its IP part, its GD part, its IAF part)
 *   status_dev  int32 [B]: bit 0 = N_ip is 0, bit 1 = N_gd is 0, bit 2 = N_iaf is 0 (whatever the k)
 *   g_real_dev, g_imag_dev  float32 [B, T, F] = dA / d est_real, dA / d est_imag, or BOTH NULL for the values alone (rows,
 *               counts, total and status then have the bits they have with a gradient).  A gather per cell, no atomics:
 *     D = c_ip s_ip[t,f];  D += c_gd (s_gd[t,f] - s_gd[t,f+1]);  D += c_iaf (s_iaf[t,f] - s_iaf[t+1,f])
 *     with c_i = k_i / N_i (0 where k_i == 0 or N_i == 0; N_i is read from counts_dev), s_gd[t,f] the sign of the pair whose
 *     later cell is (t, f), and terms that do not exist or are void contributing 0;
 *     g_real = (float)(D (-im / |z|^2)),  g_imag = (float)(D (re / |z|^2)),  |z|^2 = re^2 + im^2 as above.
 *     A void cell, and a cell with D == 0, gets exact (positive) zeros.  clean_spec, the void map and the counts are constants.
 * A row with est == clean bit for bit, and one with est = 2 clean, has values of exact zeros (and a gradient of exact
 * zeros).  Fixed-order reductions: bit-reproducible, row-independent (a NaN stays in its own row, whose cells are void),
 * never in place.  The workspace (256-byte aligned) holds six float64 per tile.  cmgan_phase_loss_workspace_bytes returns 0
 * for B outside 1 .. 65535 or T outside 1 .. 1000000; its size does not depend on F, so its handle is not read and may be
 * NULL.  CMGAN_E_BADARG before anything is launched, and before the handle is looked at: a null est / clean / rows / counts /
 * total / status, a misaligned buffer, B or T outside their ranges, a NaN k, a NaN or negative floor, only one of the two
 * gradient buffers, a workspace that is too small or misaligned; then a null handle; then, with the handle's F: F above
 * 1024, a gradient buffer over an input or over the other.  3 launches for the values, 4 with the gradient; no host
 * synchronisation, no allocation; graph-capturable, and a replay reads the current contents of the inputs.              */
int cmgan_phase_loss_tile_frames(void);
size_t cmgan_phase_loss_workspace_bytes(cmgan_handle* h, int B, int T);
int cmgan_phase_loss(cmgan_handle* h, const float* est_real_dev, const float* est_imag_dev, const float* clean_spec_dev, int B,
                     int T, double k_ip, double k_gd, double k_iaf, double floor, double* rows_dev, int* counts_dev,
                     float* total_dev, int* status_dev, float* g_real_dev, float* g_imag_dev, void* ws, size_t ws_bytes,
                     void* stream);

/* Names + durations (ms) of the kernels of the most recent forward when
 * profiling is enabled with cmgan_set_profiling(h, 1): HIP events are recorded
 * around every launch on the caller's stream.  cmgan_profile_read synchronises
 * the events, writes up to `cap` entries and returns the count.  bench.py uses it
 * for the live per-kernel roofline figure.                                      */
typedef struct cmgan_kernel_time { const char* name; float ms; } cmgan_kernel_time;
int cmgan_set_profiling(cmgan_handle* h, int enabled);
int cmgan_profile_read(cmgan_handle* h, cmgan_kernel_time* out, int cap);

/* ---- Environment ---------------------------------------------------------------------------------------------------
 * Launch-shape / kernel-choice overrides, read ONCE per process on first use (same-session A/B sweeps,
 * tools/knob_sweep.sh).  None changes a result beyond the last bits: each selects between kernels / launch shapes that
 * are parity-tested on their own.  Values outside the range shown (or not a number) are ignored - the built-in default
 * applies, so no setting can produce an invalid launch (kernels.h, env_knob):
 *   CMGAN_FFN32=0|1            FeedForward on 32x32x16 MFMAs (1, default) or the 16x16x32 kernel (0)
 *   CMGAN_STFT_BSPLIT=1..13    bin blocks per thread block of the small-batch STFT
 *   CMGAN_ASP_TPB_LONG=1..64, CMGAN_ASP_GROUP_LONG=1..4096, CMGAN_ASP_GROUP_SHORT=1..4096, CMGAN_ASP_ALIGN_SHORT=0|1,
 *   CMGAN_ASP_SLOTS=8..65536, CMGAN_ASP_TAILK=0|1    tile order / block shape of the attention kernel
 *   CMGAN_STFT_FFT=0|1         front / back end as 16 x 25 real FFTs (1, default) or the folded DFT products (0)
 *   CMGAN_FFN_BWD_FUSED=0|1, CMGAN_CM_BWD1_FUSED=0|1, CMGAN_CM_BWD2_FUSED=0|1
 *                              training: FeedForward backward / conv-module backward parts 1 and 2 with their weight gradients
 *                              contracted on the chip (1, default) or the un-fused kernels + token-contraction launches (0)
 *   CMGAN_RC_FWD_X3=0|1, CMGAN_RC_WGRAD_X3=0|1, CMGAN_RC_DGRAD_X3=0|1
 *                              training: forward (through the inference kernels), weight gradient and data gradient of the
 *                              encoder's stride-2 conv and the decoders' sub-pixel conv on split-f16 products (1, default)
 *                              or the fp32-MFMA row-conv kernels (0)
 *   CMGAN_ATTN_BWD=cores       training: the three attention backward cores instead of the fused kernel (read per launch)
 *   CMGAN_ATF_SLOTS_SHORT=1|2  training: wrapped diagonals per wave of the fused attention backward at L <= 128 (2, default:
 *                              4-wave blocks, three per CU; 1: 7-wave blocks, one per CU)
 * (The Python host adds CMGAN_BRANCHES=1|2 and CMGAN_BRANCH_OFFSET=n for Engine.enhance_graphed; CMGAN_HIP_LIB selects
 * the library file.)                                                                                                  */

#ifdef __cplusplus
}
#endif
#endif /* CMGAN_HIP_H */
