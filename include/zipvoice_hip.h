/*
 * zipvoice_hip.h — C ABI of the MI355X-native ZipVoice inference engine
 * (libzipvoice_hip.so, gfx950).
 *
 * Plain pointers and sizes only.  Every tensor argument is a DEVICE pointer
 * (caller-owned, row-major, contiguous) unless the parameter name says host_.
 * All work is enqueued on `stream` (a hipStream_t, NULL = default stream); no
 * call synchronises the host except zv_finalize (weight upload).
 * Return value: 0 on success, nonzero on error; zv_last_error() then returns
 * a thread-local message (the Python layer raises it as RuntimeError /
 * ValueError, mirroring the reference's exceptions).
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * reference repository winlaic/ZipVoice):
 *   zv_create / zv_set_weight / zv_finalize
 *       ZipVoice*.__init__ + load_checkpoint(strict=True)
 *       (zipvoice/models/zipvoice.py:38-133, zipvoice/utils/checkpoint.py:108-146,
 *        zipvoice/bin/infer_zipvoice.py:549-566)
 *   zv_fm_decoder      ZipVoice.forward_fm_decoder (zipvoice/models/zipvoice.py:135-185)
 *                      == TTSZipformer.forward (zipvoice/models/modules/zipformer.py:242-293)
 *   zv_velocity        DiffusionModel.forward / DistillDiffusionModel.forward
 *                      (zipvoice/models/modules/solver.py:40-165)
 *   zv_euler_sample    EulerSolver.sample (zipvoice/models/modules/solver.py:182-240)
 *   zv_euler_sample_sched  EulerSolver.sample run per row with that row's own scalars (defined below)
 *   zv_session_*       the same as a long-lived session that rows enter and leave between steps
 *                      (continuous batching; defined below)
 *   zv_text_encode     ZipVoice.forward_text_embed (zipvoice/models/zipvoice.py:187-212,
 *                      ZipVoiceDialog override zipvoice/models/zipvoice_dialog.py:127-159)
 *   zv_text_condition  ZipVoice.forward_text_condition (zipvoice/models/zipvoice.py:214-251)
 *   zv_speech_condition  speech-condition padding in ZipVoice.sample (zipvoice.py:441-451)
 *   Reference per-step ONNX operator with the same contract as zv_velocity:
 *       fm_decoder.onnx (zipvoice/bin/onnx_export.py:157-204)
 *   zv_vocoder_*       the vocoder the reference loads and calls after sampling:
 *                      get_vocoder (zipvoice/bin/infer_zipvoice.py:249-273) ->
 *                      Vocos.from_hparams + load_state_dict, and
 *                      `vocoder.decode(pred_features).squeeze(1).clamp(-1, 1)` with the
 *                      feature post-processing of infer_zipvoice.py:374-378
 *                      (third-party vocos 0.1.0: Vocos.decode = VocosBackbone + ISTFTHead)
 *   zv_fbank_*         VocosFbank.extract (zipvoice/utils/feature.py:36-120) and
 *                      BigVGANFbank.extract (:133-204, _bigvgan_mel_feature.py:42-111): the prompt
 *                      log-mel front end feeding prompt_features (infer_zipvoice.py:328-337)
 *   zv_resample_*      torchaudio.transforms.Resample on the loaded prompt
 *                      (infer_zipvoice.py:332-338, infer_zipvoice_dialog.py:270-277, :417-422)
 *   zv_wavjoin_*       no reference counterpart (long-form join, defined below)
 */
#ifndef ZIPVOICE_HIP_H
#define ZIPVOICE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zv_engine* zv_handle;

enum zv_variant { ZV_ZIPVOICE = 0, ZV_DISTILL = 1, ZV_DIALOG = 2, ZV_DIALOG_STEREO = 3 };
/* ZV_FP32: fp32-accurate mode (GEMMs as split products hi*hi + hi*lo + lo*hi of 16-bit
 *          operands, fp32 everything else);
 * ZV_BF16: 16-bit MFMA operands, fp32 accumulation / residual stream / softmax;
 * ZV_MIXED: ZV_BF16 for the decoder layers, the split products for the decoder's input /
 *          output projections, the layers' attention-score projections and the whole text
 *          encoder (the cheap linears that carry most of the 16-bit rounding error into the
 *          output).
 * The 16-bit operand format is the library's: bf16 in libzipvoice_hip.so, IEEE fp16 in
 * libzipvoice_hip_f16.so (same entry points, built from the same sources with
 * -DZV_OPERAND_F16).  ZV_MIXED in the fp16 library is the parity-grade fast mode.
 * ZV_FP8: ZV_BF16 with the decoder layers' feed-forward, convolution-module and
 *          NonlinAttention output linears on block-scaled MX-fp8 MFMA (e4m3 weights and
 *          activations, one power-of-two scale per 32 K elements; bf16 library only).  The
 *          BASELINE C5 "fp8 MFMA weights" mode, with its own tolerance. */
enum zv_precision { ZV_FP32 = 0, ZV_BF16 = 1, ZV_MIXED = 2, ZV_FP8 = 3 };

#define ZV_MAX_STACKS 8

/* Mirrors the "model" block of model.json (egs/zipvoice/conf/zipvoice_base.json:2-25). */
typedef struct {
  int variant;                 /* zv_variant */
  int precision;               /* zv_precision */
  int feat_dim;                /* 100 */
  int num_stacks;              /* len(fm_decoder_downsampling_factor) */
  int downsampling_factor[ZV_MAX_STACKS];
  int num_layers[ZV_MAX_STACKS];
  int cnn_module_kernel[ZV_MAX_STACKS];
  int fm_decoder_dim, fm_decoder_feedforward_dim, fm_decoder_num_heads;
  int text_encoder_num_layers, text_encoder_feedforward_dim, text_encoder_cnn_module_kernel;
  int text_encoder_num_heads, text_encoder_dim;
  int time_embed_dim, text_embed_dim;
  int query_head_dim, value_head_dim, pos_head_dim, pos_dim;
  int vocab_size, pad_id, spk_a_id, spk_b_id;
} zv_config;

const char* zv_last_error(void);
const char* zv_version(void);

zv_handle zv_create(const zv_config* cfg);
void zv_destroy(zv_handle h);

/* Stage one state-dict tensor (host fp32, reference key name, e.g.
 * "fm_decoder.encoders.1.encoder.layers.0.feed_forward2.in_proj.weight"). */
int zv_set_weight(zv_handle h, const char* name, const float* host_data, int64_t numel);
/* Check that every tensor of the config's state dict was staged (strict=True),
 * convert/pad to the device layout and upload.  Synchronous. */
int zv_finalize(zv_handle h);
/* Pre-size the decoder workspace for guided calls of up to max_batch utterances of
 * max_frames frames (runs one uncaptured guided velocity on zeros and synchronises).
 * Optional: forward calls grow it on demand, which synchronises; after a reservation
 * no call up to that shape allocates device memory. */
int zv_reserve(zv_handle h, int max_batch, int max_frames);
/* Total bytes of device memory held (weights + workspace). */
int64_t zv_device_bytes(zv_handle h);

/* Padding mode of the flow-matching decoder (no reference counterpart: the reference has the first
 * behaviour only).  A decoder stack with downsampling factor ds > 1 sums groups of ds frames and
 * right-pads the last group (SimpleDownsample, zipformer.py:887-913).
 *   ZV_PAD_BATCH (default)  the group is padded as the reference pads the batch tensor: a masked
 *                           row's last group takes in the frames past the row's end, so a row whose
 *                           length is no multiple of ds depends on the padded length and on what
 *                           lies there.
 *   ZV_PAD_ROW              every row is downsampled as the reference downsamples it alone: with
 *                           n_b = 1 + the last unmasked frame of row b (T for a fully masked row),
 *                           out[b, i] = sum_k w[k] in[b, min(i ds + k, n_b - 1)] for every i < dL.
 *                           A row's valid frames are then a function of its own valid frames only,
 *                           and equal the reference's result for the row alone at T = n_b to rounding
 *                           (not bitwise: kernel choices may still follow the batch's shape).
 * The lengths come from the padding mask each decoder call receives, so every entry point that
 * passes a mask follows the mode (zv_fm_decoder, zv_velocity, zv_euler_sample*, zv_session_step, the
 * editing solves); a call without a mask, the text encoder (factor 1) and the vocoders are not
 * affected.  zv_set_padding fails, changing nothing, for any other mode and while a session of the
 * engine has an occupied slot (a row's solve never changes mode midway).  zv_get_padding returns the
 * mode, -1 for a null handle. */
enum zv_padding { ZV_PAD_BATCH = 0, ZV_PAD_ROW = 1 };
int zv_set_padding(zv_handle h, int mode);
int zv_get_padding(zv_handle h);

/* Launch profiler (process-wide): when enabled, every GEMM / attention launch is
 * bracketed by HIP events on its stream.  zv_profile(0/1) also clears the log
 * (2 = on, with GEMM records keyed by shape);
 * zv_profile_report writes a JSON object {kernel: {launches, flops, bytes, ms}}
 * (synchronises on the recorded events). */
int zv_profile(int enable);
int zv_profile_report(char* buf, int buflen);

/* Number of host-blocking HIP runtime calls the library has issued since load (process-wide:
 * allocations, frees, synchronous copies / memsets, device / stream / event synchronisation,
 * stream / event / graph creation and destruction).  A warm zv_euler_sample /
 * zv_vocoder_decode at an already-seen shape adds none: the per-rank step never waits on the
 * GPU inside the Euler loop (no reference counterpart: the reference's solver loop,
 * zipvoice/models/modules/solver.py:213-240, runs eagerly on the caller's stream). */
int64_t zv_host_block_count(void);

/* Exact-path counters of the second-generation attention consumers of the bf16 / fp8 engines
 * (csrc/zv_flash2.inc).  Those kernels take p = 2^s without subtracting a row maximum; a
 * SelfAttention wave or NonlinAttention block whose range check fails redoes its queries with the
 * maximum subtracted (the reference's softmax, zipformer.py:1257-1306).  host_counts[0]: runs with
 * a query denominator under 2^-60, [1]: over 2^100 or a non-finite accumulator, [2]: every run
 * (including those forced by ZV_ATTN2_EXACT=1, test infrastructure).  Synchronises the device;
 * reset = 1 zeroes the counters.  No reference counterpart (the reference materialises softmax). */
int zv_attn_fallbacks(zv_handle h, int reset, int64_t* host_counts);

/* The second-generation attention consumers alone, on host arrays (test infrastructure: pins
 * csrc/zv_flash2.inc against a float64 softmax in tests/test_gpu_attn2.py).  Inputs are rounded to
 * the operand format as the engine's producers round them.  qkp (B, L, 2*32*H + 4*H) fp32 rows
 * [q | k | p] in base-2 units (the engine folds log2(e) into the k / p weights); P (2L-1, 4*H) the
 * positional projection (base 2); key_pad (B, L) 1 = padded, or NULL (masked_fill(-1000) of
 * zipformer.py:1281-1289 in base 2).  kernel 0 = SelfAttention (zipformer.py:1359-1396): v (B, L,
 * H*nv), nv <= 12, out (B, L, H*nv); kernel 1 = NonlinAttention (zipformer.py:1499-1544, head 0):
 * v, y, out (B, L, nv), out = y * (W0 . v).  form 0 = the engine's choice for L (SelfAttention 1 / 2:
 * register-fed with 2 / 3 query tiles per wave, 3 / 4 / 5: LDS-ring with 2 / 3 / 4; NonlinAttention
 * 1 / 2: 4 / 8 query tiles per block).  force_exact = 1 sends every wave / block through the exact
 * path; counts (or NULL) receives the three zv_attn_fallbacks counters of this launch.  Operands
 * are the library's (bf16; fp16 in libzipvoice_hip_f16.so, whose kernels take p = 2^(s - o) with a
 * per-query offset o); synchronous. */
int zv_attn2_check(int kernel, int form, int B, int L, int H, int nv, const float* qkp, const float* P,
                   const uint8_t* key_pad, const float* v, const float* y, int force_exact, float* out,
                   int64_t* counts);
/* The same with columns [L, Lpad) of V^T (Lpad = L rounded up to 64, the engine's row stride) holding
 * +stale / -stale (finite, alternating) instead of zeros: the engine's transposed value stores write
 * frames below L only, so in a reused workspace those columns hold whatever an earlier, longer
 * pass left there.  A key past L must weigh exactly 0 whatever its value. */
int zv_attn2_check_stale(int kernel, int form, int B, int L, int H, int nv, const float* qkp, const float* P,
                         const uint8_t* key_pad, const float* v, const float* y, int force_exact, float stale,
                         float* out, int64_t* counts);

/* One first-generation attention kernel (csrc/zv_flash.inc) or the materialising softmax
 * (csrc/zv_attn.inc) alone, through the launch function the engine launches it through (test
 * infrastructure: pins them against a float64 softmax in tests/test_gpu_attn_ref.py; synchronous).
 * They are the fp32 mode's kernels (split 3), the fp16 parity mode's text encoder, the over-length /
 * ZV_ATTN_MATERIALIZE fallback and the ZV_ATTN2=0 / ZV_SA_TP=0 arms.  qkp (B, L, 2*32*H + 4*H)
 * fp32 rows [q | k | p] and P (2L-1, 4*H) in natural units (these kernels fold log2(e) themselves;
 * SOFTMAX with b2 = 1 takes base-2 scores and exponentiates with exp2); qkp is rounded to the operand
 * format (split 1) or split into its hi / lo pair (split 3) as the engine's producers do; key_pad
 * (B, L) 1 = padded, or NULL.
 *   ZV_ATTN_STATS    head 0's row statistics.  form 0: positional term on VALU (split 1 / 3), 1: the
 *                    Toeplitz MFMA form (split 1).  stats (guard + B*L + guard, 2) fp32 = (m, r): the
 *                    base-2 row maximum estimate and 1 / sum_j 2^(u_j - m).
 *   ZV_ATTN_NA       NonlinAttention (head 0): the matching STATS launch into a private buffer, then
 *                    the consumer chosen by width as the engine chooses it (nv <= 384, a multiple
 *                    of 4).  v, y (B, L, nv); oh (/ ol with split 3) (guard + B*L + guard, ldo),
 *                    ldo % 4 == 0: out = y * (W0 . v).
 *   ZV_ATTN_SA       SelfAttention.  form 0: zv_attn_sa_kernel<split>, 1: zv_attn_sa_tp_kernel<0, 2>,
 *                    2: <0, 1> (forms 1 / 2: split 1).  v (B, L, H*nv), nv <= 12; oh (/ ol with split
 *                    3) (guard + B*L + guard, ldo), column h * nv + d.  Forms 1 / 2 also write the
 *                    output's lo half to ol and a second hi copy to oh2 when both are given (the fp16
 *                    parity mode's [o_hi | o_lo | o_hi] operand).
 *   ZV_ATTN_SOFTMAX  the weights W = softmax(s) of every head: Wh (/ Wl with split 3)
 *                    (guard + H*B*L + guard, ldw), ldw = L rounded up to 64, row (h * B + b) * L + i;
 *                    columns [L, ldw) are written as zeros.
 * V^T is laid out as the engine's transposed linears leave it: rows of L rounded up to 64 frames
 * (SA: nv rows per head -- these kernels make the ones row of the softmax denominator in registers;
 * NA: nv rows), frames below L written, columns past L holding +stale / -stale (finite).  Every
 * output is canary-filled by the caller, goes to the device as it is and comes back whole.
 * vrows (SA): V^T rows per head, 0 = nv, or up to 16: the layout of a value projection built padded for
 * the second-generation kernels, which the engine's fallback and ZV_ATTN2=0 arms hand to these kernels
 * with a 16-row head stride; rows nv..15 of a head then hold +-stale.
 * launch (out), written by the kind's launch function itself: {kernel (0 stats, 1 NonlinAttention,
 * 2 SelfAttention, 3 SelfAttention Toeplitz, 4 softmax), SPLIT, NA value tiles per wave (DTW) / Toeplitz
 * SA PLO, NA query tiles per block / Toeplitz SA MINW, TPM, grid x, grid y, grid z}. */
enum zv_attn_kind { ZV_ATTN_STATS = 0, ZV_ATTN_NA = 1, ZV_ATTN_SA = 2, ZV_ATTN_SOFTMAX = 3 };
typedef struct {
  int kind, B, L, H, nv, split, form, b2, guard, vrows;
  float stale;
  const float* qkp; const float* P; const uint8_t* key_pad;
  const float* v; const float* y;
  float* stats;
  uint16_t* oh; uint16_t* ol; uint16_t* oh2; int64_t ldo;
  uint16_t* Wh; uint16_t* Wl; int64_t ldw;
  int launch[8];
} zv_attn_check_args;
int zv_attn_check(zv_attn_check_args* a);

/* GEMM microbenchmark (random bf16 operands): average ms per launch of the 128x128 kernel for
 * C(M,N) = A(M,K) W(N,K)^T.  variant 0 = the general epilogue (any out_mode), 70 = the counted
 * residual epilogue (out_mode 5 / 6), 72 = the counted plain epilogue (out_mode 7); +100: one tile
 * per block instead of the persistent grid; any other value is rejected.  out_mode 0 = fp32 C,
 * 1 = bf16 C, 2 = residual (C += ..., fp32, plus a bf16 copy), 3 = SwooshL -> bf16, 4 = no output,
 * 5 = bias + residual (a residual linear's epilogue), 6 = 5 + bypass original and scale, 7 = bias +
 * SwooshL -> bf16 (a plain linear's). */
int zv_bench_gemm(int M, int N, int K, int variant, int iters, int out_mode, float* ms_out);

/* Microbenchmark of the NonlinAttention in-projection (form ZV_LIN_NA = 7, N % 48 == 0) or the
 * SelfAttention value projection (ZV_LIN_TRANS = 6) alone: average ms per launch of the 16-bit
 * product through the engine's launch choice (ZV_TRANS_ALIGNED as the engine reads it), random
 * operands, M rows in utterances of rpb rows, V^T rows of rpb rounded up to 64 frames. */
int zv_bench_fused_linear(int form, int M, int N, int K, int rpb, int iters, float* ms_out);

/* GEMM self-check (test infrastructure): variant 70 / 71 / 72 = the counted residual / residual +
 * bypass / plain epilogue of the 128x128 kernel (any other value is rejected) against its general
 * epilogue on the same random operands; mode 0 plain, 1 SwooshL (variant 72), 2 residual (70 / 71).
 * Writes max |diff| and max |ref|. */
int zv_gemm_selftest(int M, int N, int K, int variant, int mode, float* maxdiff, float* maxref);

/* One linear through the engine's own dispatch, on host arrays (test infrastructure: pins
 * csrc/zv_gemm.inc and zv_gemm256.inc against a float64 reference in tests/test_gpu_linear_ref.py;
 * no reference counterpart; synchronous).  The weight W (N, K) and bias (N) are in the reference's
 * layout and become a device linear exactly as the engine's weights do (hi / lo halves, rows padded
 * to 128, columns to 64, zero fill; the NA / GLU forms permute the rows as the engine does).  A
 * (M, K) is laid out as the engine lays out an activation: rounded to the operand format (bf16, or
 * fp16 in libzipvoice_hip_f16.so), with its lo half when split = 3, row stride K rounded up to 64,
 * zero beyond K.  split: 1 = 16-bit product, 3 = hi/lo split products of both operands, 2 = the
 * weight-split product (ZV_LIN_PLAIN without activation, and ZV_LIN_TRANS).  The launch is the one
 * the engine would make for that shape and form, not a chosen instantiation; `launch` receives which
 * one it was: {BM, BN, SPLIT, EPI, ROLE, 256x256 kernel, grid blocks, STAGES * 16 + OCC (+ 256 when
 * the TRANS / NA launch ran utterance-aligned tiles: B * ceil(rpb / BM) * ceil(N / BN) of them)}.
 *
 * Outputs keep their padding: the caller passes every output buffer it wants with guard rows before
 * row 0 and after the last row and a row stride larger than the width (ldc % 4 == 0, ldch % 8 == 0),
 * pre-filled with a canary; the buffer goes to the device as it is (the residual forms place resid
 * in the interior of C, which is updated in place as the engine updates its stream), comes back
 * whole, and the caller checks that nothing outside the output changed.
 *   C   fp32 (guard + M + guard, ldc);  Ch / Cl  16-bit hi / lo (guard + M + guard, ldch)
 *   Cth / Ctl  transposed 16-bit output of ZV_LIN_TRANS / ZV_LIN_NA:
 *              (guard + B * rows_t + guard, ldct), B = ceil(M / rpb), rows_t = N (TRANS) or N / 3
 *              (NA); element [b][n][l] is row b * rpb + l, column n. */
enum zv_linear_form {
  ZV_LIN_PLAIN = 0,        /* bias (+ SwooshL when act = 1) -> Ch (/ Cl) */
  ZV_LIN_PLAIN_F32 = 1,    /* bias (+ SwooshL) -> C */
  ZV_LIN_RESID = 2,        /* C = resid + (A W^T + bias), and its copy Ch (/ Cl) when given */
  ZV_LIN_RESID_BYP = 3,    /* ... then C = orig + (C - orig) * byp */
  ZV_LIN_RESID_RV = 4,     /* C = resid + (A W^T + bias) + rowvec[row / rows_per_group] */
  ZV_LIN_RESID_RV_COPY = 5,/* the same value to Ch only (no fp32 output; resid read from `resid`) */
  ZV_LIN_TRANS = 6,        /* bias -> Cth (/ Ctl), transposed per utterance of rpb rows */
  ZV_LIN_NA = 7,           /* W rows [s | x | y] (chunk(3)): x * tanh(s) -> Cth, y -> Ch, N / 3 wide */
  ZV_LIN_GLU = 8,          /* W rows [x | s] (chunk(2)): x * sigmoid(s), 0 where rowmask -> Ch, N / 2 wide */
  ZV_LIN_GLU_DW = 9        /* the ConvolutionModule's fused launch (zv_gemm256.inc g256_epi_glu_dw): GLU as above,
                              rounded to the operand format, then the depthwise conv of dw_ks taps ("same" zero
                              padding per utterance of dw_L rows) + SwooshR -> Ch, N / 2 wide.  split 1, N = 1024,
                              dw_ks 7 / 15 / 31, M % dw_L == 0, ldch % 8 == 0: the engine's own conditions for this
                              launch; anything else is rejected, never replaced by the unfused pair */
};
typedef struct {
  int M, N, K, split, form, act;
  int rows_per_group;      /* row-vector forms */
  int rpb;                 /* TRANS / NA: rows per utterance */
  int guard;               /* guard rows on each side of every output */
  const float* A; const float* W; const float* bias;
  const float* resid;      /* (M, N) */
  const float* orig;       /* (M, N) */
  const float* byp;        /* (N) */
  const float* rowvec;     /* (ceil(M / rows_per_group), N) */
  const uint8_t* rowmask;  /* (M) or NULL */
  const float* dw_w;       /* GLU_DW: the conv's taps (N / 2, dw_ks) */
  const float* dw_b;       /* GLU_DW: the conv's bias (N / 2) */
  int dw_ks, dw_L;         /* GLU_DW: kernel size, rows per utterance */
  float* C; int64_t ldc;
  uint16_t* Ch; uint16_t* Cl; int64_t ldch;
  uint16_t* Cth; uint16_t* Ctl; int64_t ldct;
  int launch[8];           /* out */
  int num_cus;             /* out: the CU count the dispatch thresholds used */
} zv_linear_check_args;
int zv_linear_check(zv_linear_check_args* a);

/* The fused FeedForward kernel alone, on host arrays (test infrastructure: pins csrc/zv_ffn.inc
 * against float64 in tests/test_gpu_ffn_ref.py; no reference counterpart; synchronous).  x (M, 512)
 * is rounded to the operand format; W1 (H, 512), b1, W2 (512, H), b2 are in the reference's layout
 * and are packed as the engine packs them.  form 0: C = resid + FF(x) (in place: resid starts in the
 * interior of C), with the 16-bit copy Ch when given; 1: + rowvec[row / rows_per_group] (Ch
 * required); 2: then the bypass C = orig + (C - orig) * byp (Ch required); 3: the BiasNorm epilogue,
 * v = resid + FF(x); out = orig + (v * rsqrt(mean((v - nb)^2)) * exp(log_scale) - orig) * byp -> C
 * (in place over orig, which starts in the interior of C), Ch (required), Cl, and out (+ rowvec
 * when given) -> C2h / C2l where given.  part_slots 0: one row block per block; > 0: the
 * persistent line schedule on that many blocks (at most the CU count).  Output buffers as
 * zv_linear_check: (guard + M + guard) rows of ldc (fp32) / ldch (16-bit) elements, canary-filled by
 * the caller.  launch: {128, 512, 1, RV | ORIG << 1 | COPY << 2 | TP << 3, NORM, 0, blocks, chunk
 * steps per block}.  Fails if the device error word is set after the launch. */
typedef struct {
  int M, H, form, rows_per_group, part_slots, guard;
  float log_scale;
  const float* x; const float* W1; const float* b1; const float* W2; const float* b2;
  const float* resid;      /* (M, 512) */
  const float* rowvec;     /* (ceil(M / rows_per_group), 512) or NULL */
  const float* orig;       /* (M, 512) */
  const float* byp;        /* (512) */
  const float* nb;         /* (512) */
  float* C; int64_t ldc;
  uint16_t* Ch; uint16_t* Cl; uint16_t* C2h; uint16_t* C2l; int64_t ldch;
  int launch[8];
  int num_cus;
  /* the pre-projection form (forms 2 and 3; K = 0: off): cur1 = resid + (A . Wp^T + bp) [+ rowvec]
   * replaces resid, x = round16(cur1) replaces the x argument (ignored); with form 2 the row vector
   * belongs to the pre-projection, with form 3 it is added there and to C2h / C2l.  launch[3] has
   * bit 4 (PRE) set. */
  int K;
  const float* A;          /* (M, K) */
  const float* Wp;         /* (512, K) */
  const float* bp;         /* (512) */
} zv_ffn_check_args;
int zv_ffn_check(zv_ffn_check_args* a);

/* The ConvolutionModule's depthwise conv + SwooshR alone, through the engine's launch_dwconv (test
 * infrastructure: pins csrc/zv_elem.inc's four kernels against float64 in tests/test_gpu_dwconv_ref.py;
 * no reference counterpart; synchronous).  g (B * L, C) is rounded to the operand format (with its lo
 * half when split = 3) into rows of ldin elements; w (C, ks) and bias (C) are fp32.  The kernel is the
 * one the engine would launch for these sizes, strides and operands; ZV_DWCONV_PIPE (0, 1 = automatic
 * chunk, n = chunks of n 64-frame tiles) and ZV_DWCONV_LDS=0 are read per launch and select the other
 * arms.  Oh / Ol: (guard + B * L + guard, ldout) 16-bit, canary-filled by the caller (Ol with split 3
 * only); q / qs (or NULL): the output's MX-fp8 copy, (guard + B * L + guard, ldq) codes and
 * (..., ldq / 32) scale bytes, canary-filled.  launch: {kernel (0 generic, 1 register-window, 2 LDS,
 * 3 pipe), ks, 3 with lo halves else 1, fp8 copy, grid x, grid y, grid z, 64-frame tiles per pipe
 * chunk (0 for the other kernels)}. */
typedef struct {
  int B, L, C, ks, split, guard;
  const float* g; const float* w; const float* bias;
  int64_t ldin;
  uint16_t* Oh; uint16_t* Ol; int64_t ldout;
  uint8_t* q; uint8_t* qs; int64_t ldq;
  int launch[8];
  int num_cus;
} zv_dwconv_check_args;
int zv_dwconv_check(zv_dwconv_check_args* a);

/* The kernels at the stack boundaries, each launched as zv_engine launches it (test infrastructure:
 * pins them against float64 in tests/test_gpu_stackedge_ref.py; synchronous).  M = B * L rows,
 * dL = ceil(L / ds).  fp32 outputs have guard rows only (their row stride is C); 16-bit outputs have
 * guard rows and a row stride ldact (a multiple of 4); all are canary-filled by the caller.
 *   ZV_SE_DOWNSAMPLE  x (M, C), w (ds) -> out (guard + B * dL + guard, C)
 *   ZV_SE_UPSAMPLE    x = the downsampled stream (B * dL, C), w = the combiner scale (C), orig (M, C)
 *                     -> out (guard + M + guard, C), updated in place over orig; the row-blocked kernel
 *                     where 256 % (C / 4) == 0, else the grid-stride one (launch[1] = 0 / 1)
 *   ZV_SE_MASK        mask (B, L) -> mout (guard + B * dL + guard) bytes
 *   ZV_SE_ENTRY       x = src (M, C), rowvec (or NULL) -> h / l = src, h2 / l2 = src + rowvec[row /
 *                     rows_per_group] (l, l2 optional), and the fp32 sum -> out where given
 *   ZV_SE_BIASNORM    x (M, C), nb (C), log_scale, w = bypass scale (C), orig (M, C) -> out in place
 *                     over orig, h (/ l); h2 (/ l2) = out + rowvec where given, and its MX-fp8 copy
 *                     q2 (guard + M + guard, ldq) / qs2 (..., ldq / 32); zv_biasnorm_bypass_v_kernel<2>
 *                     at C = 512, else the generic kernel (launch[1] = 1 / 0)
 * launch: {kind, kernel form, grid blocks, block threads, 0...}. */
enum zv_stackedge_kind { ZV_SE_DOWNSAMPLE = 0, ZV_SE_UPSAMPLE = 1, ZV_SE_MASK = 2, ZV_SE_ENTRY = 3, ZV_SE_BIASNORM = 4 };
typedef struct {
  int kind, B, L, C, ds, guard, rows_per_group;
  float log_scale;
  const float* x; const float* w; const float* nb; const float* orig; const float* rowvec;
  const uint8_t* mask;
  float* out;
  uint8_t* mout;
  uint16_t* h; uint16_t* l; uint16_t* h2; uint16_t* l2; int64_t ldact;
  uint8_t* q2; uint8_t* qs2; int64_t ldq;
  int launch[8];
  int num_cus;
} zv_stackedge_check_args;
int zv_stackedge_check(zv_stackedge_check_args* a);

/* The row padding mode's kernels as zv_engine launches them (test infrastructure: pins them against
 * float64 in tests/test_gpu_padrow_ref.py; synchronous).  mask (B, L) bytes -> lens (guard + B + guard)
 * int32, the rows' lengths (zv_row_len_kernel); x (B * L, C), w (ds) and those lengths -> out
 * (guard + B * dL + guard, C), dL = ceil(L / ds) (zv_downsample_row_kernel).  lens and out are
 * canary-filled by the caller.  launch: {0, length-kernel blocks, length-kernel threads, downsample
 * blocks, downsample threads, 0...}. */
typedef struct {
  int B, L, C, ds, guard;
  const uint8_t* mask; const float* x; const float* w;
  int32_t* lens;
  float* out;
  int launch[8];
  int num_cus;
} zv_padrow_check_args;
int zv_padrow_check(zv_padrow_check_args* a);

/* The BigVGAN kernels one at a time, and one AMP step, through the launches and weight relayouts that
 * zv_bigvgan's finalize / decode use (test infrastructure: pins csrc/zv_bigvgan.inc, the implicit-conv
 * GEMM and the conv_pre im2col against float64 in tests/test_gpu_bigvgan_ref.py; builds no zv_bigvgan;
 * synchronous).  split 1 / 3: 16-bit operands without / with their lo halves.  A stage stream holds
 * utterance b in rows b * Lp + [0, Lmax), Lp = round_up(Lmax + halo, 8); halo is a positive multiple
 * of 8.  lens (B) or NULL; an utterance's length is min(lens[b] * scale, Lmax).  fp32 outputs have
 * guard rows only, 16-bit ones the row stride stated; all are canary-filled by the caller, and what
 * the caller puts in rows / columns the kernel leaves alone comes back as it was.  Everything the
 * call allocates besides (16-bit operands, their padding columns and halo rows, fp32 scratch) starts
 * from a finite, non-zero pattern seeded by `stale`, never zeros: a result that depends on unwritten
 * memory changes with the seed.  Non-finite stale data is outside the kernels' contract.
 *   ZV_BV_FILTER  out = the BvFilter (up_even[6], up_odd[6], down[12]) of the 12 taps `taps`, or of
 *                 the kaiser-sinc filter when taps is NULL
 *   ZV_BV_ACT     zv_bv_act_kernel<mode> (0 / 2): x (B * Lp, C), alpha, ibeta (C), taps or NULL ->
 *                 mode 0: out (guard + B * Lp + guard, C); mode 2: oh / ol (guard + halo + B * Lp +
 *                 halo + guard, round_up(C, 32)): the operand as decode allocates it, both outer halos
 *                 included (the kernel never writes the trailing one)
 *   ZV_BV_CONV    w (Cout, C, ks), bias, dilation d; ah / al (halo + B * Lp + halo, round_up(C, 32)):
 *                 the operand with its halos; resid (B * Lp, Cout) or NULL -> out (guard + B * Lp +
 *                 guard, Cout), through the Conv1d relayout and the implicit-conv dispatch
 *   ZV_BV_CONVT   ConvTranspose1d (k = ks, stride u, padding (k - u) / 2) of utterances of Lmax frames
 *                 at rows b * Ls: flag 1: x (B * Ls, C), w (C, Cout, k) through the relayout and the
 *                 plain GEMM; flag 0: x = P (B * Ls, k * Cout), the gather alone; bias (Cout), scale =
 *                 the input lengths' scale -> out (guard + B * Lo + guard, Cout), Lo = round_up(Lmax *
 *                 u + halo, 8)
 *   ZV_BV_AVG     (x + x1 + x2) / n over M = B * Lmax rows of C -> out (guard + M + guard, C) and
 *                 oh / ol (guard + M + guard, ld) where given
 *   ZV_BV_POST    conv_post + clamp (flag 0) / tanh (flag 1): x (B * Ls, C), w (C, 7), bias0 -> out
 *                 (guard + B * Lmax + guard); fails when the LDS window exceeds 64 KiB
 *   ZV_BV_IM2COL  zv_voc_im2col_kernel: x (B, C, Lmax) (layout 0) or (B, Lmax, C) (1), div, sub ->
 *                 oh / ol (guard + B * Lmax + guard, round_up(C * ks, 64)); flag 1: then conv_pre's
 *                 GEMM with w (Cout, C, ks), bias -> out (guard + B * Lmax + guard, Cout)
 *   ZV_BV_STEP    one AMP step as decode runs it: out = x + conv2(act2(conv1_d(act1(x)))), x (B * Lp, C),
 *                 alpha / ibeta, w / bias (conv1, dilation d), alpha2 / ibeta2, w2 / bias2 (conv2)
 *                 -> out (guard + B * Lp + guard, C); rows outside [0, len) are unspecified
 * launch: the last GEMM's record as zv_linear_check's, with launch[5] = its K step (0: no GEMM). */
enum zv_bigvgan_check_kind { ZV_BV_FILTER = 0, ZV_BV_ACT = 1, ZV_BV_CONV = 2, ZV_BV_CONVT = 3, ZV_BV_AVG = 4,
                             ZV_BV_POST = 5, ZV_BV_IM2COL = 6, ZV_BV_STEP = 7 };
typedef struct {
  int kind, split, mode, guard;
  int B, Lmax, Ls, halo, scale;
  int C, Cout, ks, d, u, n, layout, flag;
  float div, sub, bias0;
  unsigned stale;
  const int* lens;
  const float* x; const float* x1; const float* x2;
  const float* w; const float* bias; const float* alpha; const float* ibeta;
  const float* w2; const float* bias2; const float* alpha2; const float* ibeta2;
  const float* taps; const float* resid;
  const uint16_t* ah; const uint16_t* al;
  float* out; uint16_t* oh; uint16_t* ol; int64_t ld;
  int launch[8];
  int num_cus;
} zv_bigvgan_check_args;
int zv_bigvgan_check(zv_bigvgan_check_args* a);

/* The kernels around the decoder, one launch at a time through the launch functions zv_engine calls
 * (test infrastructure: pins csrc/zv_elem.inc's solve-boundary kernels against float64 in
 * tests/test_gpu_solve_ref.py; builds no engine, needs no weights; synchronous).  Every output is
 * canary-filled by the caller and has `guard` guard rows at both ends (flat outputs: guard elements);
 * what the kernel leaves alone comes back as it was.
 *   ZV_SV_BUILD_INPUT   x (B * T, Fx), tc (B * T, Ft), sc (B * T, Fs), copies 1 / 2, zero_speech ->
 *                       oh / ol (guard + copies * B * T + guard, ld), ld >= Fx + Ft + Fs; ol NULL: no lo
 *                       half.  Rows [0, B T) of two copies are the unconditional ones.  launch[1]: 1 the
 *                       quad kernel (Fx, Ft, Fs, ld multiples of 4), 0 the scalar one
 *   ZV_SV_EULER         x (n), v (n, or 2 n with cfg = 1: unconditional then conditional), g, dt; grows (B)
 *                       or NULL with gmul and per_row (n = B * per_row) -> out (guard + n + guard), updated
 *                       in place over x
 *   ZV_SV_CFG_COMBINE   v (2 n), g / grows, gmul, per_row -> out (guard + n + guard)
 *   ZV_SV_MASK_COPY     mask (n) -> mout (guard + copies * n + guard) bytes
 *   ZV_SV_FILL          value -> out (guard + n + guard)
 *   ZV_SV_TEMB          x = t (M), W = freqs (N / 2) -> out (guard + M + guard, N): cos | sin | 0 (odd N)
 *   ZV_SV_SMALL_LINEAR  x (M, ldin), W (N, ldw), bias (N) or NULL, add (M, N) or NULL, pre 0 / 1 (SwooshR
 *                       on the input) -> out (guard + M + guard, ld); inplace 1: add is placed in out and
 *                       read from there.  form -1: the engine's policy (the row-staged kernel where
 *                       K <= 8192), 0 / 1: the row-staged / the per-output kernel; launch[1] says which
 *   ZV_SV_POSP          W (M * N, K): M layers' linear_pos weights (N = heads * pos_head_dim, K = pos_dim
 *                       <= 64), sequence length T -> out (guard + M * (2 T - 1) + guard, N)
 *   ZV_SV_EMBED         tok (n) int64 in [0, N), W = table (N, C) -> oh / ol (guard + n + guard, ld)
 *   ZV_SV_SPK_ADD       x (n, C), spk (n) in {-1, 0, 1}, W = table (2, C) -> out (guard + n + guard, C), in
 *                       place over x
 *   ZV_SV_TEXT_COND     x = embed (B, S, C), lens = tok_lens, lens2 = feat_lens (0 < tok_lens < S,
 *                       feat_lens >= 0: checked here on the host) -> out (guard + B * T + guard, C)
 *   ZV_SV_SPEECH_COND   x = prompt (B, S = Tp, C), lens = prompt_lens -> out (guard + B * T + guard, C)
 * launch: {kind, kernel form, grid blocks, block threads, 0...}. */
enum zv_solve_kind { ZV_SV_BUILD_INPUT = 0, ZV_SV_EULER = 1, ZV_SV_CFG_COMBINE = 2, ZV_SV_MASK_COPY = 3,
                     ZV_SV_FILL = 4, ZV_SV_TEMB = 5, ZV_SV_SMALL_LINEAR = 6, ZV_SV_POSP = 7, ZV_SV_EMBED = 8,
                     ZV_SV_SPK_ADD = 9, ZV_SV_TEXT_COND = 10, ZV_SV_SPEECH_COND = 11 };
typedef struct {
  int kind, guard, form;
  int B, T, S, C;
  int Fx, Ft, Fs, copies, zero_speech, cfg;
  int M, N, K, pre, inplace;
  float g, dt, gmul, value;
  int64_t n, per_row, ld, ldin, ldw;
  const float* x; const float* tc; const float* sc; const float* v; const float* grows;
  const float* W; const float* bias; const float* add;
  const int32_t* lens; const int32_t* lens2; const int64_t* tok; const int8_t* spk; const uint8_t* mask;
  float* out; uint16_t* oh; uint16_t* ol; uint8_t* mout;
  int launch[8];
  int num_cus;
} zv_solve_check_args;
int zv_solve_check(zv_solve_check_args* a);

/* The solve's host decisions (host only, no GPU; test infrastructure, tests/test_solve_plan.py).
 * zv_time_steps: the Euler grid zv_euler_sample integrates over, out[0 .. num_step] =
 * t_shift u / (1 + (t_shift - 1) u), u = torch.linspace(t_start, t_end, num_step + 1) in float32.
 * zv_cfg_plan: DiffusionModel.forward's branches (solver.py:71-98) for one velocity call at time t:
 * copies 2 when the rows are doubled (guidance_scale != 0, or per-row scales (has_rows) of which
 * some are nonzero (rows_nonzero); never in distill), zero_speech 1 when the unconditional copy's
 * speech condition is zeroed (t > 0.5), else the scale doubled: g = 2 guidance_scale, gmul = 2 (the
 * factor on per-row scales). */
int zv_time_steps(float t_start, float t_end, int num_step, float t_shift, float* out);
int zv_cfg_plan(float t, float guidance_scale, int has_rows, int rows_nonzero, int distill, int* copies,
                int* zero_speech, float* g, float* gmul);

/* The scheduled solve's host plan (host only, no GPU; what zv_euler_sample_sched itself runs;
 * tests/test_sched_plan.py).  Row b of a schedule integrates its own grid ts_b = zv_time_steps(t_start,
 * t_end, num_step, t_shift) with its own guidance scale, as EulerSolver.sample (solver.py:182-240)
 * would on that row alone.  The solve runs steps = max_b num_step steps; row b is active at step k iff
 * k < num_step_b, and a step's active list keeps the input order.  Not distilled: an active row has an
 * unconditional copy iff its scale is nonzero (solver.py:71 per row), with zv_cfg_plan's branch at the
 * row's own t (t > 0.5: the copy's speech zeroed and the scale g, else the speech kept and the scale
 * 2 g).  The step's decoder batch is the `copies` unconditional copies, in active order, then the
 * `active` conditional rows, in active order (every row active and guided: [uncond B | cond B]).
 * Distilled: no copies; the row's scale feeds the guidance embedding (act_scale).
 * zv_sched_plan fills `steps` and `total_rows` (the sum over the steps of copies + active: the decoder
 * rows of the whole solve) and, for step `step` in [0, steps), `active`, `copies` and every array that
 * is not NULL: dec_* take copies + active (at most 2 B) entries, act_* take active (at most B).
 * Rejected: B < 1 (or above 32767), num_step < 1, a non-finite field, t_shift <= 0, step outside
 * [0, steps). */
typedef struct { int32_t num_step; float t_start, t_end, t_shift, guidance_scale; } zv_row_sched;
typedef struct {
  int32_t steps;             /* K */
  int32_t active, copies;    /* A, U of the step */
  int64_t total_rows;
  int32_t* dec_src;          /* per decoder row: its input row */
  uint8_t* dec_zero_text;    /* ... 1: text condition zeroed (an unconditional copy) */
  uint8_t* dec_zero_speech;  /* ... 1: speech condition zeroed */
  float* dec_t;              /* ... its time */
  int32_t* act_row;          /* per active row: its input row */
  float* act_dt;             /* ... ts[k + 1] - ts[k] in float32 */
  float* act_scale;          /* ... the scale of the update (g or 2 g; 0 without a copy); distill: g */
  int32_t* act_cond;         /* ... the decoder row of its conditional velocity */
  int32_t* act_uncond;       /* ... of its unconditional velocity, or -1 */
} zv_sched_plan_out;
int zv_sched_plan(const zv_row_sched* rows, int B, int distill, int step, zv_sched_plan_out* out);

/* The scheduled solve's three kernels, one launch at a time through the launch functions zv_engine
 * calls (test infrastructure: tests/test_gpu_sched_ref.py; builds no engine; synchronous).  Outputs are
 * canary-filled by the caller with `guard` guard rows (flat outputs: elements) at both ends, as
 * zv_solve_check's.  Every index is checked on the host before the launch.
 *   ZV_SC_BUILD_INPUT  x (B * T, Fx), tc (B * T, Ft), sc (B * T, Fs); src / zero_text / zero_speech (N):
 *                      decoder row j = cat[x, tc, sc] of input row src[j], text / speech zeroed by its
 *                      flags -> oh / ol (guard + N * T + guard, ld); ol NULL: no lo half.  launch[1]: 1
 *                      the quad kernel (Fx, Ft, Fs, ld multiples of 4), 0 the scalar one
 *   ZV_SC_MASK_GATHER  mask (B * T), src (N) -> mout (guard + N * T + guard) bytes
 *   ZV_SC_EULER        x (B * per_row), v (N * per_row); row / dt / scale / cond / uncond (A, rows
 *                      distinct): x[row] += ((1 + g) v[cond] - g v[uncond]) dt, or v[cond] dt where
 *                      uncond < 0 -> out (guard + B * per_row + guard), in place over x
 * launch: {kind, kernel form, grid.x, block threads, grid.y, 0...}. */
enum zv_sched_kind { ZV_SC_BUILD_INPUT = 0, ZV_SC_MASK_GATHER = 1, ZV_SC_EULER = 2 };
typedef struct {
  int kind, guard;
  int B, T, N, A;
  int Fx, Ft, Fs;
  int64_t ld, per_row;
  const int32_t* src; const uint8_t* zero_text; const uint8_t* zero_speech;
  const float* x; const float* tc; const float* sc; const uint8_t* mask; const float* v;
  const int32_t* row; const float* dt; const float* scale; const int32_t* cond; const int32_t* uncond;
  float* out; uint16_t* oh; uint16_t* ol; uint8_t* mout;
  int launch[8];
  int num_cus;
} zv_sched_check_args;
int zv_sched_check(zv_sched_check_args* a);

/* A session tick's host plan (host only, no GPU; what zv_session_step itself runs;
 * tests/test_session_plan.py).  Slot b holds a row when rows[b].num_step > 0 (0 marks a free slot)
 * and is active while done[b] < num_step.  The tick is zv_sched_plan's step rule over the active
 * slots, in slot order, with slot b at its own index k = done[b] of its own grid: dec_t = ts_b[k],
 * act_dt = ts_b[k + 1] - ts_b[k], the copy rule at the row's own t, the copies first; act_row and
 * dec_src name slots.  *T_k = the longest lens[b] over the active slots (0 with none).  out as
 * zv_sched_plan's: active, copies and the arrays of this tick; steps = the ticks left until every
 * slot is done and total_rows = the decoder rows of those ticks, if nothing is admitted (with
 * every done[b] = 0: zv_sched_plan's).  Rejected: slots outside [1, 32767], an occupied slot with
 * done outside [0, num_step], lens outside [1, 2^30) or a schedule zv_sched_plan would reject. */
int zv_session_plan(const zv_row_sched* rows, const int32_t* done, const int32_t* lens, int slots,
                    int distill, zv_sched_plan_out* out, int32_t* T_k);

/* The session's kernels, one launch at a time through the launch functions the engine calls (test
 * infrastructure: tests/test_gpu_session_kernels.py; builds no engine; synchronous).  Outputs are
 * canary-filled by the caller with `guard` guard rows (flat outputs: elements) at both ends.  Every
 * index is checked on the host before the launch.  The slot buffers are (slots, max_frames, F).
 *   ZV_SS_ADMIT   x, tc, sc: the request rows (n, T_io, Fx / Ft / Fs = Fx); slot / len (n) -> out, out_tc,
 *                 out_sc (guard + slots * max_frames * F + guard) and mout (guard + slots * max_frames
 *                 + guard): the named slots written whole, the others left
 *   ZV_SS_RETIRE  x: the slot buffer; slot / len (n) -> out (guard + n * T_io * Fx + guard)
 *   ZV_SS_BUILD_INPUT  x, tc, sc: the slot buffers; src / zero_text / zero_speech (N) -> oh / ol (guard +
 *                 N * T_k + guard, ld); ol NULL: no lo half
 *   ZV_SS_MASK_GATHER  mask: the slot buffer; src (N) -> mout (guard + N * T_k + guard)
 *   ZV_SS_EULER   x: the slot buffer, v (N * T_k * Fx); row / dt / scale / cond / uncond (A, rows distinct)
 *                 -> out (guard + slots * max_frames * Fx + guard), in place over x
 * launch: {kind, kernel form (1: the quad kernel), grid.x, block threads, grid.y, 0...}. */
enum zv_session_kind { ZV_SS_ADMIT = 0, ZV_SS_RETIRE = 1, ZV_SS_BUILD_INPUT = 2, ZV_SS_MASK_GATHER = 3,
                       ZV_SS_EULER = 4 };
typedef struct {
  int kind, guard;
  int slots, max_frames, n, T_io, T_k, N, A;
  int Fx, Ft, Fs;
  int64_t ld;
  const int32_t* slot; const int32_t* len;
  const int32_t* src; const uint8_t* zero_text; const uint8_t* zero_speech;
  const float* x; const float* tc; const float* sc; const uint8_t* mask; const float* v;
  const int32_t* row; const float* dt; const float* scale; const int32_t* cond; const int32_t* uncond;
  float* out; float* out_tc; float* out_sc; uint16_t* oh; uint16_t* ol; uint8_t* mout;
  int launch[8];
  int num_cus;
} zv_session_check_args;
int zv_session_check(zv_session_check_args* a);

/* The edit rows' two kernels (zv_session_admit_edit / zv_session_retire_edit below), one launch at a
 * time through the rules, the table layout and the launch functions the engine runs (test
 * infrastructure: tests/test_gpu_session_edit_kernels.py; builds no engine; synchronous).  Outputs are
 * canary-filled by the caller with `guard` guard elements at both ends.  The session's host state is
 * the caller's: state_left [slots] the steps each slot has left (-1: free), state_len [slots] its row's
 * length; a call that succeeds updates both as the engine would (admit: num_step and T_i, retire: -1
 * and 0), a rejected call (return 1) leaves them and every output as they were and launches nothing.
 * slot / offsets / lens (n), table, row_ptr (n + 1) and pool (pool_rows, Fx) as in the entries.
 *   ZV_SE_ADMIT   x, tc: the request rows (n, T_io, Fx / Ft); rows (n) the schedules -> out, out_tc,
 *                 out_sc (guard + slots * max_frames * F + guard) and mout (guard + slots * max_frames
 *                 + guard): the named slots written whole, the others left
 *   ZV_SE_RETIRE  x: the slot buffer (slots, max_frames, Fx); keep_original -> out (guard + n * T_io *
 *                 Fx + guard) and mout (guard + n * T_io + guard, or NULL)
 * launch: {kind, kernel form (1: the quad kernel), grid.x, block threads, grid.y, 0...}. */
enum zv_session_edit_kind { ZV_SE_ADMIT = 0, ZV_SE_RETIRE = 1 };
typedef struct {
  int kind, guard;
  int slots, max_frames, n, T_io, Fx, Ft, pool_rows, keep_original;
  const int32_t* slot; const int32_t* offsets; const int32_t* lens; const int32_t* table; const int32_t* row_ptr;
  const zv_row_sched* rows;
  int32_t* state_left; int32_t* state_len;
  const float* x; const float* tc; const float* pool;
  float* out; float* out_tc; float* out_sc; uint8_t* mout;
  int launch[8];
  int num_cus;
} zv_session_edit_check_args;
int zv_session_edit_check(zv_session_edit_check_args* a);

/* Attention plan (host only, no GPU; test infrastructure): the LDS bytes of the fused
 * attention consumers a layer of sequence length L would launch — SelfAttention (sa_plo < 0:
 * the plain kernel, 0 / 1: the Toeplitz kernel without / with the table's lo half),
 * NonlinAttention of value width nv_na with scoring form tpm, the head-0 statistics — and
 * whether the fused path is taken (fits = 1) or the W-materialising fallback (0).
 * tpm = 3: the second-generation set of the bf16 / fp8 engines (zv_flash2.inc: base-2 scores,
 * no statistics pass, lds_stats = 0; sa_plo ignored).
 * split: 1 (16-bit operands) or 3 (fp32-accurate hi/lo). */
int zv_attn_plan(int split, int sa_plo, int tpm, int L, int nv_na, int64_t* lds_sa, int64_t* lds_na,
                 int64_t* lds_stats, int* fits);

/* MX-fp8 operand format of the fp8 mode (csrc/zv_mx8.inc): e4m3 values, one E8M0 scale byte per
 * 32 consecutive K elements.  zv_mx8_quantize: the host quantiser the engine applies to the
 * fp8 weights (host pointers, no GPU: x (rows, K) fp32 -> q (rows, ldq), s (rows, ldq / 32),
 * ldq = K rounded up to 128).  zv_mx8_gemm_check: the fp8 GEMM end to end on the device (host
 * pointers in and out): A (M, K) is rounded to bf16 and quantised by the device producer kernel
 * (zv_mx8_pack_kernel; its output returned in Aq / As), W (N, K) by the host quantiser, and
 * C = A8 . W8^T through the block-scaled MFMA GEMM with the residual epilogue (zero residual
 * and bias), K a multiple of 128.  Both replace no reference interface: they pin the fp8
 * mode's operand format and GEMM against tests/ (numpy). */
int zv_mx8_quantize(const float* x, int rows, int K, uint8_t* q, uint8_t* s);
int zv_mx8_gemm_check(int M, int N, int K, const float* A, const float* W, float* C, uint8_t* Aq,
                      uint8_t* As);

/* Raw decoder: v = fm_decoder(cat[xt, text_c, speech_c], t, pad, g).
 *  t:      [N] timesteps;  guidance: [N] (distill only, else NULL)
 *  xt, speech_c: [N, T, Fx]; text_c: [N, T, feat_dim]; pad: [N, T] uint8 (1 = padded) or NULL
 *  v_out:  [N, T, Fout] with Fout = Fx (stereo: stream chosen by input width). */
int zv_fm_decoder(zv_handle h, const float* t, const float* guidance, const float* xt,
                  const float* text_c, const float* speech_c, const uint8_t* pad, int N,
                  int T, int Fx, float* v_out, void* stream);

/* One guided velocity evaluation (solver.py:40-165): CFG doubling inside,
 * x/text_c/speech_c/pad are the B un-doubled rows; v_out [B, T, Fx]. */
int zv_velocity(zv_handle h, float t, float guidance_scale, const float* x,
                const float* text_c, const float* speech_c, const uint8_t* pad, int B, int T,
                float* v_out, void* stream);

/* Full Euler ODE solve (solver.py:182-240), in place: x holds x0 on entry and
 * x(t_end) on return.  Time grid: t_shift*u/(1+(t_shift-1)u), u = linspace. */
int zv_euler_sample(zv_handle h, float* x, const float* text_c, const float* speech_c,
                    const uint8_t* pad, int B, int T, int num_step, float guidance_scale,
                    float t_start, float t_end, float t_shift, void* stream);

/* Per-utterance guidance scales (the reference's guidance_scale tensor of shape
 * (batch, 1, 1), solver.py:61-62): guidance_rows is a device array of B floats.
 * (guidance_rows == 0).all() selects the unguided branch (solver.py:71-79; one small
 * device-to-host read at entry, as the reference's host predicate); otherwise CFG with
 * g_b per row, doubled where t <= 0.5 (:95).  Distill: the rows feed the guidance
 * embedding (solver.py:127-165). */
int zv_velocity_rows(zv_handle h, float t, const float* guidance_rows, const float* x,
                     const float* text_c, const float* speech_c, const uint8_t* pad, int B,
                     int T, float* v_out, void* stream);
int zv_euler_sample_rows(zv_handle h, float* x, const float* text_c, const float* speech_c,
                         const uint8_t* pad, int B, int T, int num_step,
                         const float* guidance_rows, float t_start, float t_end,
                         float t_shift, void* stream);

/* Scheduled solve: one call integrates B rows, each over its own Euler grid with its own guidance
 * scale (rows: HOST array of B zv_row_sched, read before the call returns).  Row b ends as
 * EulerSolver.sample (solver.py:182-240) would leave it when run on that row alone with that row's
 * scalars; the reference has no batched counterpart (its solver takes one num_step / t_shift per
 * call).  In place over x like zv_euler_sample; a row is neither read into the decoder nor written
 * once its steps are done, and a row with scale 0 has no unconditional copy, so the decoder runs
 * zv_sched_plan's total_rows rows instead of 2 B max(num_step).  The padded length T is the
 * batch's for every step.  Plain launches on `stream` (no graph); the step tables go up once per
 * solve from pinned staging owned by the engine, and a warm call makes no host-blocking runtime call
 * and no device-to-host read (the all-zero-scale question is answered from the host schedule).
 * zv_sched_stats: out[0] the decoder rows launched, out[1] the steps run by the handle's last
 * scheduled solve. */
int zv_euler_sample_sched(zv_handle h, float* x, const float* text_c, const float* speech_c,
                          const uint8_t* pad, int B, int T, const zv_row_sched* rows, void* stream);
int zv_sched_stats(zv_handle h, int64_t* out);

/* Solve session: continuous batching.  The scheduled solve as a long-lived object with `slots` row
 * slots of `max_frames` frames: between any two decoder steps finished rows are taken out and waiting
 * rows put into the free slots, and every row still integrates its own grid from its own step 0 with
 * its own scalars, as EulerSolver.sample (solver.py:182-240) would integrate that row inside a padded
 * batch: in a step it is padded with zeros to T_k, the longest row active in that step.  A row whose
 * length is a multiple of every downsampling factor ends exactly as it would alone; any other row's
 * last valid frames see the frames just past its end (SimpleDownsample groups ds frames, as the
 * reference's), so its result depends on T_k, i.e. on which rows are in flight beside it, as a row of
 * any padded batch depends on its padding.  The reference has no counterpart.  A row stays in its
 * slot from admit to retire (the step's row map gathers the active slots into the decoder batch).
 * Every entry is queued on `stream`; the host arrays are read before the call returns.  Use one
 * stream per ENGINE: all sessions of an engine and its other entries (zv_euler_sample_sched, the
 * velocity and solve calls) share the decoder workspace and one device table, and are ordered only
 * by the stream.  The tables go up from the engine's pinned staging, and a warm admit / step / retire
 * makes no host-blocking runtime call and no device-to-host read (the host knows which rows finish
 * from the schedules alone) while at most 8 uploads (one per admit, step or retire) are queued and
 * not yet run by the GPU; a host that runs further ahead makes the engine allocate one more pinned
 * staging slot per upload in flight (a blocking hipHostMalloc, kept until the engine is destroyed).
 *   create   the session owns x (slots, max_frames, Fx), text and speech conditions and the padding
 *            mask, all zero, and sizes the decoder workspace for 2 * slots rows of max_frames (as
 *            zv_reserve), so a step never moves it.  slots in [1, 32767].  The engine must outlive the
 *            session: every entry of a session whose engine is gone returns an error.
 *   admit    row i of x0 / speech_c (n, T_in, Fx) and text_c (n, T_in, feat_dim) (device) goes into
 *            slot host_slots[i] with the schedule host_rows[i]: frames [0, len) copied, [len,
 *            max_frames) zero in all three, pad[t] = t >= len.  One launch.  Rejected, with nothing
 *            queued or changed: n < 1; a slot outside [0, slots), not free or named twice; len < 1, len
 *            > T_in or len > max_frames; a schedule zv_sched_plan would reject.
 *   step     one tick: every occupied slot with steps left runs one Euler step at its own step index
 *            on its own grid (zv_session_plan below), at the decoder length T_k = the longest active
 *            row, exactly; frames >= T_k of a slot and the other slots are not touched.  A session
 *            whose rows were all admitted before the first tick runs zv_euler_sample_sched's decoder
 *            batches at T = max len.  No active slot: nothing is launched.
 *   retire   frames [0, len) of slot host_slots[i]'s x go to row i of out (n, T_out, Fx) (device), [len,
 *            T_out) zero; the slot is then free and may be admitted again at once.  One launch.
 *            Rejected: n < 1, a slot outside [0, slots), free, with steps left or named twice, T_out
 *            shorter than a row.
 *   state    host_steps_left [slots]: the steps each slot still has to run, -1 for a free slot; stats
 *            [4]: ticks run, decoder rows launched, the sum over the ticks of decoder rows x T_k, the
 *            last tick's T_k.  Either may be NULL. */
typedef struct zv_session* zv_session_handle;
zv_session_handle zv_session_create(zv_handle h, int slots, int max_frames);
void zv_session_destroy(zv_session_handle s);
int zv_session_admit(zv_session_handle s, int n, const int32_t* host_slots, const int32_t* host_lens,
                     const zv_row_sched* host_rows, const float* x0, const float* text_c,
                     const float* speech_c, int T_in, void* stream);
int zv_session_step(zv_session_handle s, void* stream);
int zv_session_retire(zv_session_handle s, int n, const int32_t* host_slots, float* out, int T_out,
                      void* stream);
int zv_session_state(zv_session_handle s, int32_t* host_steps_left, int64_t* stats);

/* Edit rows: a row of a speech edit (zv_edit_gather's frame tables) enters and leaves a slot straight
 * from a pool of stored feature frames, pool [pool_rows, Fx] device fp32 (the voice store's arena); no
 * (n, T, Fx) speech condition is built and nothing is read back.  NO reference counterpart.  Row i is
 * described by host_offsets[i] and host_lens[i] = L_i: its original frame f is pool row
 * host_offsets[i] + f (a plain (B, Lmax, Fx) tensor is the case offset_i = i * Lmax), and by segments
 * [host_row_ptr[i], host_row_ptr[i + 1]) of host_table, rows (dst, src, len) int32 with src == -1 a
 * generated segment, exactly as zv_edit_gather defines them; T_i is the length they tile.  The same
 * pool range may be named by several rows.  All of it is validated on the host before anything is
 * queued, the error names the row, and a rejected call changes no state and launches nothing:
 *   the table   row_ptr[0] == 0 and not falling; len > 0; the segments of a row tile [0, T_i) in
 *               order; a kept segment lies in [0, L_i); L_i >= 0, offset_i >= 0 and offset_i + L_i <=
 *               pool_rows (so the pool is never read outside [offset_i, offset_i + L_i));
 *   admit       zv_session_admit's rules with len = T_i: n < 1, a slot outside [0, slots), not free or
 *               named twice, T_i < 1, T_i > T_in or T_i > max_frames, a schedule zv_sched_plan rejects;
 *   retire      zv_session_retire's rules: n < 1, a slot outside [0, slots), free, with steps left or
 *               named twice, T_out shorter than a row; and a table whose T_i is not the slot's length.
 * The checked table then goes up through the engine's pinned staging as the other tables of a session
 * (one upload per call; the warm-path promise of zv_session_admit holds).
 *   admit_edit  one launch, one row per blockIdx.y, into the free slot host_slots[i] with the schedule
 *               host_rows[i] (t_start / t_end as zv_session_admit): x <- x0[i, :T_i], text <- text_c[i,
 *               :T_i], both zero up to max_frames (x0 (n, T_in, Fx), text_c (n, T_in, feat_dim) device);
 *               speech[t] = the pool frame on a kept segment, 0 on a generated one and for t >= T_i;
 *               pad[t] = t >= T_i.  The slot is then as zv_session_admit leaves it after
 *               zv_edit_gather(fill = NULL) built its speech condition, bit for bit.
 *   retire_edit one launch: out[i, t] (n, T_out, Fx) = the pool frame on a kept segment (bitwise the
 *               original), the slot's x on a generated one, 0 for T_i <= t < T_out; keep_original == 0
 *               takes the slot's x on every frame below T_i (sample_edit(keep_original=False));
 *               mask_out (n, T_out) uint8 or NULL: 1 exactly on generated frames.  The slot is free
 *               afterwards.  What zv_session_retire followed by zv_edit_gather(fill = the retired rows)
 *               leaves, bit for bit.
 * Both find a frame's segment by bisection in the row's table once per frame, move four features per
 * thread (16-byte loads and stores) when Fx % 4 == 0 (admit: and feat_dim % 4 == 0) and every base is
 * 16-byte aligned, one otherwise; no atomics, every output element is written exactly once by one
 * thread, and the results do not depend on the launch geometry. */
int zv_session_admit_edit(zv_session_handle s, int n, const int32_t* host_slots, const zv_row_sched* host_rows,
                          const float* x0, const float* text_c, int T_in, const float* pool, int pool_rows,
                          const int32_t* host_offsets, const int32_t* host_lens, const int32_t* host_table,
                          const int32_t* host_row_ptr, void* stream);
int zv_session_retire_edit(zv_session_handle s, int n, const int32_t* host_slots, const float* pool, int pool_rows,
                           const int32_t* host_offsets, const int32_t* host_lens, const int32_t* host_table,
                           const int32_t* host_row_ptr, int keep_original, float* out, uint8_t* mask_out, int T_out,
                           void* stream);

/* Text encoder (+ dialog speaker-turn embeddings).
 *  tokens: [B, S] int64 (already padded with pad_id, one extra pad per row);
 *  pad: [B, S] uint8; spk: [B, S] int8 in {-1,0,1} (dialog only, else NULL);
 *  out: [B, S, feat_dim]. */
int zv_text_encode(zv_handle h, const int64_t* tokens, const uint8_t* pad,
                   const int8_t* spk, int B, int S, float* out, void* stream);

/* Frame-rate text condition: out[b, f] = embed[b, min(f / (T_b / S_b), S_b)].
 *  tok_lens, feat_lens: [B] int32 device; out: [B, T, feat_dim].
 *  Preconditions: embed is [B, S, feat_dim] (the engine's own feat_dim: the call takes no width
 *  and cannot check the embedding's), with the pad slot, so 0 < tok_lens[b] < S (the kernel divides
 *  by tok_lens[b] and reads token tok_lens[b] for the frames past the last whole duration), and
 *  feat_lens[b] >= 0.  The lengths are device values and are not checked (that would take a
 *  device round trip); B, T > 0 and S > 1 are. */
int zv_text_condition(zv_handle h, const float* embed, int B, int S, const int32_t* tok_lens,
                      const int32_t* feat_lens, int T, float* out, void* stream);

/* Speech condition: prompt features [B, Tp, F] padded/zeroed to [B, T, F]. */
int zv_speech_condition(zv_handle h, const float* prompt, int B, int Tp, int F,
                        const int32_t* prompt_lens, int T, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Vocoder (Vocos, mel-24khz configuration: n_mels 100, dim 512, intermediate 1536,
 * 8 ConvNeXt blocks, ISTFT head n_fft 1024 / hop 256 / padding "same").
 * ---------------------------------------------------------------------- */
typedef struct zv_vocoder* zv_vocoder_handle;

/* Mirrors the vocos config.yaml backbone / head init_args. */
typedef struct {
  int precision;          /* zv_precision (ZV_FP32 = split-bf16x3 GEMMs, the parity mode) */
  int n_mels;             /* backbone.input_channels (100) */
  int dim;                /* backbone.dim (512) */
  int intermediate_dim;   /* backbone.intermediate_dim (1536) */
  int num_layers;         /* backbone.num_layers (8) */
  int n_fft;              /* head.n_fft (1024) */
  int hop;                /* head.hop_length (256) */
  int embed_kernel;       /* backbone.embed kernel size (7) */
  int dw_kernel;          /* ConvNeXt depthwise kernel size (7) */
} zv_vocoder_config;

zv_vocoder_handle zv_vocoder_create(const zv_vocoder_config* cfg);
void zv_vocoder_destroy(zv_vocoder_handle v);
/* Stage one vocos state-dict tensor (e.g. "backbone.convnext.3.pwconv1.weight",
 * "head.istft.window"); "feature_extractor.*" buffers are accepted and ignored. */
int zv_vocoder_set_weight(zv_vocoder_handle v, const char* name, const float* host_data,
                          int64_t numel);
int zv_vocoder_finalize(zv_vocoder_handle v);
/* wav[b, :T*hop] = decode(mel_b) for B utterances of up to T frames.
 *  layout 0: mel [B, n_mels, T] (Vocos.decode input, used as is: pass feat_scale 1, feat_bias 0);
 *  layout 1: model output [B, T, n_mels], post-processed as x / feat_scale - feat_bias
 *            (infer_zipvoice.py:374) inside the first kernel.
 *  lens: [B] int32 device frame counts (NULL = all T): utterance b is decoded on its own
 *        first lens[b] frames, exactly as a separate call would, and samples from
 *        lens[b]*hop on are 0.
 *  clamp: 1 applies clamp(-1, 1) (infer_zipvoice.py:378).  wav: [B, T*hop] fp32. */
int zv_vocoder_decode(zv_vocoder_handle v, const float* mel, int layout, float feat_scale,
                      float feat_bias, const int32_t* lens, int B, int T, float* wav, int clamp,
                      void* stream);
int64_t zv_vocoder_device_bytes(zv_vocoder_handle v);

/* ------------------------------------------------------------------------
 * Vocoder (BigVGAN-v2, bigvgan_v2_24khz_100band_256x), the one the reference loads for
 * feature.type "bigvgan_v2" (zipvoice/bin/infer_zipvoice.py:261-269: third-party
 * bigvgan.BigVGAN.from_pretrained(..., use_cuda_kernel=False) + remove_weight_norm();
 * decode(mel) = forward(mel)).  Weights are the weight-norm-removed state dict.
 * ---------------------------------------------------------------------- */
typedef struct zv_bigvgan* zv_bigvgan_handle;

/* Mirrors the bigvgan config.json fields the generator reads. */
typedef struct {
  int precision;                    /* zv_precision (ZV_FP32 = split-bf16x3 GEMMs) */
  int num_mels;                     /* 100 */
  int upsample_initial_channel;     /* 1536 */
  int num_upsamples;                /* len(upsample_rates) (6), <= 8 */
  int upsample_rates[8];            /* 4 4 2 2 2 2 */
  int upsample_kernel_sizes[8];     /* 8 8 4 4 4 4 */
  int num_kernels;                  /* len(resblock_kernel_sizes) (3), <= 3 */
  int resblock_kernel_sizes[3];     /* 3 7 11 */
  int resblock_dilation_sizes[3][3];/* (1 3 5) x 3; resblock "1" (AMPBlock1) */
  int snake_logscale;               /* 1 */
  int use_tanh_at_final;            /* 0: clamp(-1, 1) */
  int use_bias_at_final;            /* 0 */
} zv_bigvgan_config;

zv_bigvgan_handle zv_bigvgan_create(const zv_bigvgan_config* cfg);
void zv_bigvgan_destroy(zv_bigvgan_handle v);
/* Stage one generator tensor ("conv_pre.weight", "ups.0.0.weight",
 * "resblocks.4.convs1.2.bias", "resblocks.4.activations.3.act.alpha",
 * "activation_post.act.beta", "conv_post.weight", ...); the alias-free filter buffers
 * (*.upsample.filter, *.downsample.lowpass.filter) are accepted and checked. */
int zv_bigvgan_set_weight(zv_bigvgan_handle v, const char* name, const float* host_data,
                          int64_t numel);
int zv_bigvgan_finalize(zv_bigvgan_handle v);
/* wav[b, :T*hop] = forward(mel_b), hop = prod(upsample_rates); arguments as
 * zv_vocoder_decode (layout 0 [B, num_mels, T] / 1 [B, T, num_mels] with
 * x / feat_scale - feat_bias; lens [B] device frame counts or NULL).  The final
 * clamp (or tanh) is part of the network. */
int zv_bigvgan_decode(zv_bigvgan_handle v, const float* mel, int layout, float feat_scale,
                      float feat_bias, const int32_t* lens, int B, int T, float* wav,
                      void* stream);
int64_t zv_bigvgan_device_bytes(zv_bigvgan_handle v);

/* ------------------------------------------------------------------------
 * Prompt feature extractor (VocosFbank: centred reflect-padded STFT, power 1,
 * mel projection, log(clamp(1e-7)); fp32 arithmetic throughout).
 * ---------------------------------------------------------------------- */
typedef struct zv_fbank* zv_fbank_handle;
/* host_window: [n_fft] analysis window (torch.hann_window, periodic);
 * host_fb: [n_fft/2 + 1, n_mels] mel filterbank (torchaudio melscale_fbanks layout). */
zv_fbank_handle zv_fbank_create(int n_fft, int hop, int n_mels, const float* host_window,
                                const float* host_fb);
void zv_fbank_destroy(zv_fbank_handle f);
/* wav: [B, wav_ld] fp32 device samples, lens: [B] int32 sample counts (> n_fft/2);
 * out: [B, T_out, out_ld] log-mel rows (columns [0, n_mels)); utterance b fills its
 * first (lens[b] + hop/2) / hop rows (lhotse compute_num_frames), later rows are 0. */
/* Front-end variant (defaults: VocosFbank).  frame_offset = sample offset of frame
 * 0 (n_fft/2: centred STFT; (n_fft - hop)/2: BigVGANFbank's explicit reflect pad +
 * center=False), mag_eps added under the magnitude's square root (BigVGAN 1e-9),
 * log_floor the clamp before the log (Vocos 1e-7, BigVGAN 1e-5).  Frames past the
 * last STFT frame replicate it (BigVGANFbank's replicate pad to the lhotse count).
 * Reference: zipvoice/utils/feature.py:133-204, _bigvgan_mel_feature.py:42-111. */
int zv_fbank_configure(zv_fbank_handle f, int frame_offset, float mag_eps, float log_floor);
int zv_fbank_extract(zv_fbank_handle f, const float* wav, int64_t wav_ld, const int32_t* lens,
                     int B, int T_out, float* out, int64_t out_ld, void* stream);

/* ------------------------------------------------------------------------
 * Prompt resampler: torchaudio.transforms.Resample(orig_freq, new_freq) with its
 * defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), the step the
 * reference applies to a loaded prompt whose rate is not the model's
 * (zipvoice/bin/infer_zipvoice.py:332-338; zipvoice/bin/infer_zipvoice_dialog.py:270-277
 * and :417-422).  fp32 arithmetic, taps summed in ascending order.
 *
 * The filter comes from the host in compact form (zipvoice_amd/feature.py resample_plan):
 * o = orig / gcd, n = new / gcd; output i*n + j = sum_{k < S} host_table[j, k] *
 * x[i*o + host_start[j] + k], samples outside [0, len) counting as 0.  host_start [n]
 * must be non-decreasing with host_start[n-1] - host_start[0] <= o; host_table is [n, S].
 * create rejects o == n (equal rates: use the input), non-positive sizes, S > 512,
 * n * S > 16 Mi entries, and o / n so large that the input span of 256 outputs exceeds
 * 64 KiB.  Device memory is the compact table only (zv_resample_device_bytes).
 * ---------------------------------------------------------------------- */
typedef struct zv_resample* zv_resample_handle;
zv_resample_handle zv_resample_create(int o, int n, int S, const int32_t* host_start,
                                      const float* host_table);
void zv_resample_destroy(zv_resample_handle h);
/* wav: [R, wav_ld] fp32 device samples, lens: [R] int32 device sample counts (<= wav_ld);
 * out: [R, out_ld], columns [0, out_cols): row r receives ceil(n * lens[r] / o) samples
 * (at most out_cols), then zeros.  A row's result does not depend on the other rows. */
int zv_resample_apply(zv_resample_handle h, const float* wav, int64_t wav_ld, const int32_t* lens,
                      int R, float* out, int64_t out_ld, int64_t out_cols, void* stream);
int64_t zv_resample_device_bytes(zv_resample_handle h);

/* ------------------------------------------------------------------------
 * Long-form join: trim the pauses of a batch of chunk waveforms and glue the trimmed
 * chunks into one waveform with linear cross-fades (zipvoice_amd/longform.py WavJoiner,
 * generate_long).  These entry points have NO reference counterpart: the reference has no
 * long-form path, so the behaviour is defined here (tests/wavjoin_ref.py restates it in
 * float64).  fp32 arithmetic, no atomics; results are bitwise reproducible and do not
 * depend on the launch geometry.
 *
 * Frames.  Chunk b has nf = ceil(lens[b] / frame) frames; frame f covers samples
 * [f * frame, min((f + 1) * frame, lens[b])) of every channel.  Its energy e is the fp32
 * sum of squares over those samples and all C channels, in a fixed order; the frame is
 * quiet iff e < thr^2 * (samples in the frame * C), loud otherwise.
 * Kept frames.  A chunk without a loud frame is empty (m_b = 0).  Otherwise, with first /
 * last its first / last loud frame, the frames in [max(0, first - keep_edge),
 * min(nf - 1, last + keep_edge)] are kept, except that every maximal run of r > max_gap
 * quiet frames strictly between first and last keeps only its first ceil(max_gap / 2) and
 * last floor(max_gap / 2) frames.  The kept frames' samples, in order, are the trimmed
 * chunk y_b of length m_b.
 * Join.  Over the non-empty chunks in order: the first has F = 0 and off = 0; a chunk b
 * after the non-empty chunk p overlaps it by F_b = min(fade, m_p / 2, m_b / 2) (integer
 * halves) and starts at off_b = off_p + m_p - F_b; an empty chunk reports off = -1, F = 0.
 * N = off_last + m_last (0 if every chunk is empty).  For j in [0, F_b), with
 * w = (j + 1) / (F_b + 1):
 *   out[off_b + j] = g_p * y_p[m_p - F_b + j] * (1 - w) + g_b * y_b[j] * w;
 * everywhere else out = g_b * y_b, and with a gain of exactly 1 the sample is a bitwise
 * copy of its input.  Columns [N, out_cap) are zero-filled; nothing is written at or past
 * out_cap even when N > out_cap, and out_len always receives the true N.
 *
 * create rejects frame < 1 and negative thr, keep_edge, max_gap or fade.  The handle owns
 * the scratch (frame flags, per-frame destinations, the per-chunk plan), which grows on
 * demand (zv_wavjoin_device_bytes); a warm call at an already-seen size makes no
 * host-blocking runtime call.
 * ---------------------------------------------------------------------- */
typedef struct zv_wavjoin* zv_wavjoin_handle;
zv_wavjoin_handle zv_wavjoin_create(int frame, float thr, int keep_edge, int max_gap, int fade);
void zv_wavjoin_destroy(zv_wavjoin_handle h);
/* wav: [B, C, wav_ld] fp32 device samples, C in {1, 2}; lens: [B] int32 device sample
 * counts, 0 <= lens[b] <= wav_ld; gains: [B] fp32 device, or NULL for 1; out: [C, out_ld],
 * of which columns [0, out_cap) may be written (out_cap <= out_ld); out_len: one device
 * int64 (N); spans: [B, 3] device int32 {m_b, off_b, F_b}, or NULL.  B >= 0. */
int zv_wavjoin_apply(zv_wavjoin_handle h, const float* wav, int64_t wav_ld, const int32_t* lens,
                     const float* gains, int B, int C, float* out, int64_t out_ld, int64_t out_cap,
                     int64_t* out_len, int32_t* spans, void* stream);
/* The segmented join: the B chunks form D documents, and every document is joined on its
 * own into its own output row, so chunks of several texts share one batch (D == B: a
 * per-row pause trim).
 *
 * Documents.  doc_ptr is a device array of D + 1 int32 with doc_ptr[0] = 0, doc_ptr[D] = B,
 * non-decreasing; document d owns the consecutive chunks [doc_ptr[d], doc_ptr[d + 1]), a
 * range that may be empty.  Frames, kept frames and the trimmed chunks y_b are as above.
 * Join.  The rule above is applied to each document's chunks on their own, as a separate
 * zv_wavjoin_apply over just those chunks would apply it: the first non-empty chunk of a
 * document has F = 0 and off = 0, whatever precedes it in the batch, and the last
 * non-empty chunk of a document gives up no tail.
 * Output.  out: [D, C, out_ld]; row d may be written in columns [0, out_cap) only
 * (out_cap <= out_ld).  out_len: D device int64 and always receives the true N_d.
 * Columns [N_d, out_cap) of every row d are zero-filled; an empty document has N_d = 0 and
 * an all-zero row.  spans: [B, 3] device int32 {m_b, off_b, F_b}, or NULL, with off_b
 * relative to the chunk's own document row and -1 for an empty chunk.
 * doc_ptr == NULL is allowed with D == 1 only and means one document of all B chunks:
 * zv_wavjoin_apply(...) is zv_wavjoin_apply_docs(..., NULL, 1, ...).
 *
 * Rejected: a null handle, C not 1 or 2, B < 0, D < 0, D == 0 with B > 0, doc_ptr NULL
 * with D != 1, out_cap > out_ld.  B == 0 (any D >= 0) succeeds and writes out_len[d] = 0
 * and zero rows.  The contents of doc_ptr are a precondition (the library cannot read them
 * without a host wait, so the caller checks them): the kernels read every bound clamped
 * into [0, B] with hi >= lo and keep every store inside columns [0, out_cap) of a row < D
 * and inside the scratch, whatever the array holds; the result is then unspecified.
 * The properties of zv_wavjoin_apply hold: no atomics, every output column written exactly
 * once, bitwise reproducible results that do not depend on the launch geometry, bit copies
 * outside overlaps at gain 1, 64-bit positions, scratch owned by the handle (4 more bytes
 * per chunk for its document), no host-blocking runtime call in a warm call. */
int zv_wavjoin_apply_docs(zv_wavjoin_handle h, const float* wav, int64_t wav_ld, const int32_t* lens,
                          const float* gains, int B, int C, const int32_t* doc_ptr, int D,
                          float* out, int64_t out_ld, int64_t out_cap, int64_t* out_len,
                          int32_t* spans, void* stream);
int64_t zv_wavjoin_device_bytes(zv_wavjoin_handle h);

/* The stateful join: the same join handed over push by push (zipvoice_amd/longform.py
 * WavJoiner.stream, generate_long_stream; tests/wavjoin_stream_ref.py restates it in
 * float64).  A stream owns D independent slots; a slot is one open document, as in
 * zv_wavjoin_apply_docs, and D = 1 is the single-text case.  The stream borrows the joiner's
 * parameters and scratch: the joiner must outlive it, and calls on a joiner and its streams
 * are ordered by the caller (one device stream, or events), as calls on the joiner alone are.
 *
 * State.  After any push a slot holds on the device, for its last non-empty chunk p so far:
 * m_p, g_p, the raw (ungained) last H_p = min(fade, m_p / 2) trimmed samples
 * y_p[m_p - H_p, m_p) of every channel, and its stream position (the samples it has emitted).
 * A fresh or reset slot holds nothing and is at position 0.  The storage, C * fade floats and
 * a few words per slot, is allocated at create (zv_wavjoin_stream_device_bytes); a push
 * allocates nothing for it.
 *
 * A push gives slot d the consecutive chunks [doc_ptr[d], doc_ptr[d + 1]) of its B chunks,
 * a range that may be empty.  Frames, kept frames and the trimmed chunks y_b are as above.
 * The chain of non-empty chunks starts at the slot's held chunk p, if it holds one: the
 * first non-empty chunk b of the push then has F_b = min(fade, m_p / 2, m_b / 2) <= H_p, as
 * if p had come in the same call; without a held chunk it has F_b = 0.  Column 0 of row d is
 * the slot's position, so the held chunk starts at off_p = H_p - m_p (negative, never
 * reported) and off_b = off_p + m_p - F_b = H_p - F_b >= 0.  The push writes to row d, in
 * this order,
 *   1. the held samples that are now final, g_p * y_p[m_p - H_p, m_p - F_b);
 *   2. the F_b cross-faded samples, out[off_b + j] = g_p * y_p[m_p - F_b + j] * (1 - w)
 *      + g_b * y_b[j] * w with w = (j + 1) / (F_b + 1): the fp32 expression of
 *      zv_wavjoin_apply, on the raw held samples with g_p beside them;
 *   3. its chunks, as zv_wavjoin_apply writes them,
 *   4. except the last H = min(fade, m / 2) samples of its last non-empty chunk, which
 *      become the slot's new held tail, raw, with that chunk's m and gain.
 * A slot that gets no non-empty chunk writes nothing and keeps its state.  With
 * host_final[d] != 0 the tail (the new one, or without a non-empty chunk the held one,
 * g_p * y_p[m_p - H_p, m_p)) is written too, the slot then holds nothing, and it is closed: a
 * closed slot takes no chunks and no second final until zv_wavjoin_stream_reset, which also
 * puts its position back to 0.  Open or closed is host state, as host_final is.
 *
 * Invariant.  For any split of a chunk sequence into pushes, the last one final, the pieces
 * of a row in push order are bitwise the row zv_wavjoin_apply (zv_wavjoin_apply_docs) writes
 * for the whole sequence: pushes with B = 0, pushes whose chunks are all empty, a closing
 * push without chunks and a predecessor several pushes back included.  spans and positions
 * agree as well: off_b + pos_d is the chunk's off_b in the one-shot row.
 *
 * wav, lens, gains, spans: as for zv_wavjoin_apply, with spans[b] = {m_b, off_b, F_b} and
 * off_b relative to column 0 of this push's row (-1 for an empty chunk).  doc_ptr: D + 1
 * HOST int32, rising from doc_ptr[0] = 0 to doc_ptr[D] = B, or NULL with D == 1 (one slot of
 * all B chunks); being a host array it is checked, and its values travel as launch
 * arguments.  host_final: D host bytes, or NULL for none.  out: [D, C, out_ld]; out_len:
 * device int64 [D, 2], {n_d, pos_d}: the samples this push wrote to row d and the samples the
 * slot had emitted before it.  Columns [n_d, out_cap) are zero-filled, nothing is stored at
 * or past out_cap, and the state advances whatever out_cap is; a slot loses nothing when
 * out_cap >= fade + the sum of its chunks' lens in the push.
 *
 * Rejected: null handles, C not 1 or 2 or D < 1 at create, B < 0, doc_ptr NULL with D != 1,
 * a doc_ptr that does not rise from 0 to B, out_cap > out_ld, chunks or a final for a closed
 * slot, reset of a d outside [-1, D) (-1: every slot).  A rejected push changes nothing.
 * The properties of zv_wavjoin_apply hold: no atomics, every output column written exactly
 * once, results independent of the launch geometry, 64-bit positions, bit copies at gain 1
 * outside overlaps; a warm push makes no host-blocking runtime call, and reset is ordered on
 * its stream and does not block.  zv_wavjoin_apply and zv_wavjoin_apply_docs are unchanged. */
typedef struct zv_wavjoin_stream* zv_wavjoin_stream_handle;
zv_wavjoin_stream_handle zv_wavjoin_stream_create(zv_wavjoin_handle joiner, int C, int D);
void zv_wavjoin_stream_destroy(zv_wavjoin_stream_handle s);
int zv_wavjoin_stream_reset(zv_wavjoin_stream_handle s, int d, void* stream);
int zv_wavjoin_stream_push(zv_wavjoin_stream_handle s, const float* wav, int64_t wav_ld,
                           const int32_t* lens, const float* gains, int B, const int32_t* doc_ptr,
                           const uint8_t* host_final, float* out, int64_t out_ld, int64_t out_cap,
                           int64_t* out_len, int32_t* spans, void* stream);
int64_t zv_wavjoin_stream_device_bytes(zv_wavjoin_stream_handle s);

/* ------------------------------------------------------------------------
 * Speech editing: the two assembly passes around the solve of an edit, which regenerates
 * marked spans of a recording and keeps the rest (zipvoice_amd/edit.py, ZipVoice.sample_edit /
 * sample_intermediate).  NO reference counterpart: the reference's sample_intermediate
 * (zipvoice/models/zipvoice.py:488-534) takes a ready speech condition and returns features,
 * so the tables and the junction rule are defined here (tests/edit_ref.py restates them in
 * numpy).  fp32, no atomics, every output element written exactly once: results are bitwise
 * reproducible and do not depend on the launch geometry.
 *
 * Tables.  Both calls take, as HOST arrays, the segments of all rows one row after the other
 * and row_ptr [B + 1] int32 rising from 0: row b owns segments [row_ptr[b], row_ptr[b + 1]),
 * a range that may be empty (an empty row).  Being host arrays they are validated completely
 * before anything is queued; a bad table is an error string (it names the row) and launches
 * nothing.  The checked table is written into pinned staging owned by the handle and copied to
 * the handle's device table on `stream`; a staging buffer is taken again only once the GPU has
 * marked its copy done, so calls queued back to back on a handle each keep their own table
 * until it has been read.  Calls on one handle are ordered by the caller (one device stream, or
 * events).  The device table grows on demand (zv_edit_device_bytes, 0 before the first call); a
 * warm call makes no host-blocking runtime call.
 *
 * zv_edit_gather.  A frame table has rows (dst, src, len) int32: output frames
 * [dst, dst + len) of the row are original frames [src, src + len) (a kept segment), or
 * generated when src == -1.  Required: len > 0; the segments of a row tile [0, T_b) in order
 * (dst of the first is 0, dst of each next is dst + len of the one before) with T_b <= T; a
 * kept segment lies in [0, lens[b]); 0 <= lens[b] <= Lmax.
 *   feat [B, Lmax, F] device, fill [B, T, F] device or NULL, out [B, T, F] device, mask
 *   [B, T] device uint8 or NULL, lens [B] host int32.
 *   out[b, t] = feat[b, src + (t - dst)] on a kept segment, fill[b, t] (0 without fill) on a
 *   generated one, 0 for t >= T_b, all bitwise copies; mask[b, t] = 1 exactly on generated
 *   frames.  One call with fill == NULL builds the speech condition of an edit; one with the
 *   solver's output as fill puts the original frames back over it.  out may be fill itself; it
 *   must not overlap feat.  F % 4 == 0 with 16-byte aligned feat / fill / out moves four
 *   features per thread as 16-byte loads and stores, anything else one feature per thread.
 *   Rejected: a null handle, feat, lens, row_ptr or out, B outside [1, 65535], Lmax, F or
 *   T < 1, a table that breaks a rule above.
 *
 * zv_edit_splice.  A sample table has rows (out, src, len, kind) int32: output samples
 * [out, out + len) of the row are samples [src, src + len) of the row's original waveform
 * (kind 0) or of its generated waveform (kind 1).  Required: len > 0; the segments of a row
 * tile [0, N_b) in order with N_b <= out_cols; a segment lies inside its source's valid samples
 * [0, lens[b]) or [0, gen_lens[b]); lens[b] <= ld, gen_lens[b] <= ldg.
 *   orig [B, C, ld] device, gen [B, C, ldg] device, out [B, C, out_ld] device, C in {1, 2};
 *   lens, gen_lens [B] host int32; gains [B] host fp32, the factor on row b's generated
 *   samples; fade >= 0 samples.
 *   Away from the junctions out is the table's gather: original samples bitwise, generated
 *   samples times the row's gain (bitwise at a gain of exactly 1).  At the junction at output
 *   position p between consecutive segments i and i + 1 of a row, with lim the valid samples of
 *   a segment's source,
 *     h = min(fade, len_i / 2, len_{i+1} / 2, lim_i - (src_i + len_i), src_{i+1})
 *   (integer halves; the last two keep both reads below inside their buffers), and for
 *   j in [0, 2h), q = p - h + j, w = (j + 0.5) / (2h):
 *     out[q] = g_i * x_i[src_i + (q - out_i)] * (1 - w) + g_{i+1} * x_{i+1}[src_{i+1} + (q - p)] * w
 *   in fp32: segment i read on past its end, segment i + 1 read from before its start, g = 1
 *   for an original segment and the row's gain for a generated one.  The rule is the same for
 *   kept | generated, generated | kept and the kept | kept junction a deletion leaves; the
 *   len / 2 clamps keep the windows of neighbouring junctions apart.  Columns [N_b, out_cols)
 *   are zero-filled and nothing is stored at or past out_cols.
 *   Rejected: a null handle or array, B < 1, C not 1 or 2, fade < 0, ld, ldg or out_cols
 *   outside [1, 2^31), out_cols > out_ld, a table that breaks a rule above.
 * ---------------------------------------------------------------------- */
typedef struct zv_edit* zv_edit_handle;
zv_edit_handle zv_edit_create(void);
void zv_edit_destroy(zv_edit_handle h);
int64_t zv_edit_device_bytes(zv_edit_handle h);
int zv_edit_gather(zv_edit_handle h, const float* feat, int B, int Lmax, int F, const int32_t* host_lens,
                   const float* fill, const int32_t* host_table, const int32_t* host_row_ptr, int T,
                   float* out, uint8_t* mask, void* stream);
int zv_edit_splice(zv_edit_handle h, const float* orig, int64_t ld, const int32_t* host_lens, const float* gen,
                   int64_t ldg, const int32_t* host_gen_lens, int B, int C, const int32_t* host_table,
                   const int32_t* host_row_ptr, const float* host_gains, int fade, float* out, int64_t out_ld,
                   int64_t out_cols, void* stream);

/* ------------------------------------------------------------------------
 * Voice store: a prompt prepared once and kept on the device (zipvoice_amd/voices.py VoiceStore;
 * the (tokens, Voice) items of generate_batch and ContinuousBatcher.submit(voice=...)).  NO
 * reference counterpart: the reference normalises the prompt of every sentence on the host
 * (zipvoice/bin/infer_zipvoice.py:340-342) and restores the level on the host (:399-400), so
 * the behaviour is defined here (tests/voice_ref.py restates it in numpy).  fp32 data, no
 * atomics, every output element written exactly once: results are bitwise reproducible.
 *
 * zv_prompt_rms.  wav [B, ld] device fp32, lens [B] device int32, host_lens [B] the same
 * lengths as a HOST array (checked before the launch: each in [1, ld]; the kernel reads the
 * device copy, cut to [0, ld]).  Row b: one workgroup of 256 lanes; lane j adds
 * (double)x[i] * (double)x[i] for i = j, j + 256, ... < len in rising i, starting from 0; the
 * 256 partial sums p are folded in place, for w = 128, 64, ..., 1: p[j] += p[j + w] for every
 * j < w; then
 *   rms[b] = (float) sqrt(p[0] / (double)len)
 * in float64 with one rounding to fp32 at the end.  The order depends on len alone: a row's
 * bits do not depend on B, on ld, or on what columns [len, ld) hold (they are not read).  With
 * t = target as fp32 and IEEE fp32 divisions,
 *   gain_in[b]  = rms[b] < t ? t / rms[b] : 1      (the factor of :340-342)
 *   gain_out[b] = rms[b] < t ? rms[b] / t : 1      (the factor of :399-400)
 * rms, gain_in and gain_out are [B] device fp32; nothing comes back to the host.  Stateless, one
 * launch on `stream`, no host-blocking runtime call.  Rejected: B outside [1, 65535], ld
 * outside [1, 2^31), target <= 0, a null array, a length outside [1, ld] (so a row of length 0).
 *
 * zv_prompt_scale.  out [B, ld] device (may be wav itself), rms [B] device as written by
 * zv_prompt_rms.  For rows with rms[b] < t: out[b, i] = (wav[b, i] * t) / rms[b] for i < len,
 * two fp32 operations with an IEEE division: the expression infer._prompt_rms_normalise
 * evaluates, so for the same fp32 rms the samples are bitwise the host path's.  Other rows are
 * bitwise copies.  Columns [len, ld) are written as zeros (wav is not read there).  ld % 4 == 0
 * with 16-byte aligned wav and out moves four samples per thread as 16-byte loads and stores,
 * anything else one sample per thread.  Rejections as zv_prompt_rms.
 *
 * zv_voice_gather.  pool [pool_rows, F] device fp32 holds the stored features of the voices,
 * each a range of whole rows; host_table [n, 2] int32 HOST rows {offset, frames}; out
 * [n, T, F] device.  Row r of out receives pool rows [offset_r, offset_r + frames_r) as one
 * flat bitwise copy of frames_r * F values, then zeros up to T * F: what zv_speech_condition
 * produces from the padded prompt batch, without the padded batch.  The same range may be named
 * by several rows.  With gains_pool [pool_rows] and gains_out [n] (both or neither),
 * gains_out[r] = gains_pool[offset_r]: a voice's gain lives at the index of its first row.  F % 4
 * == 0 with 16-byte aligned pool and out moves four values per thread (16-byte loads and
 * stores), anything else one value per thread.  The table is validated completely before
 * anything is queued (0 <= offset, 1 <= frames <= T, offset + frames <= pool_rows; the error
 * names the row and launches nothing), then travels through the handle's pinned staging to the
 * handle's device table on `stream`, as the tables of zv_edit_*: calls queued back to back
 * each keep their own table until it has been read, calls on one handle are ordered by the
 * caller, and a warm call neither allocates nor makes a host-blocking runtime call
 * (zv_voice_device_bytes: the device table, 0 before the first call).  Rejected: a null handle,
 * pool, table or out, n outside [1, 65535], pool_rows, F or T < 1, T * F >= 2^30, one of the
 * gains arrays without the other, a table that breaks a rule above.
 * ---------------------------------------------------------------------- */
int zv_prompt_rms(const float* wav, int64_t ld, const int32_t* lens, const int32_t* host_lens, int B, float target,
                  float* rms, float* gain_in, float* gain_out, void* stream);
int zv_prompt_scale(const float* wav, int64_t ld, const int32_t* lens, const int32_t* host_lens, const float* rms, int B,
                    float target, float* out, void* stream);
typedef struct zv_voice* zv_voice_handle;
zv_voice_handle zv_voice_create(void);
void zv_voice_destroy(zv_voice_handle h);
int64_t zv_voice_device_bytes(zv_voice_handle h);
int zv_voice_gather(zv_voice_handle h, const float* pool, int pool_rows, int F, const int32_t* host_table, int n, int T,
                    float* out, const float* gains_pool, float* gains_out, void* stream);

/* ------------------------------------------------------------------------
 * Seeded noise: standard normals that are a pure function of (seed, stream, element
 * index), drawn on the device (zipvoice_amd/noise.py seeded_normal; the seeds / seed
 * arguments of sample, generate_sentence, generate_batch, generate_long and
 * generate_long_batch).  NO reference counterpart beyond --seed
 * (zipvoice/bin/infer_zipvoice.py:240, fix_random_seed): the reference speaks one sentence
 * per call, so there one global seed fixes a request's audio; here a request's noise must
 * not depend on the batch it is drawn in, so the behaviour is defined here
 * (tests/noise_ref.py restates it in numpy).
 *
 * The noise function.  For a row with unsigned 64-bit seed and 32-bit stream, element
 * index e (64-bit; e = f * F + c when the row is a (T, F) feature plane):
 *   block j = e / 4, lane i = e % 4;
 *   (x0, x1, x2, x3) = Philox4x32-10(counter = (j & 0xffffffff, j >> 32, stream, 0),
 *                                    key = (seed & 0xffffffff, seed >> 32)),
 *     with the standard constants: multipliers 0xD2511F53 (on counter word 0) and
 *     0xCD9E8D57 (on counter word 2), key increments 0x9E3779B9 and 0xBB67AE85, ten rounds;
 *   u(x) = fl32(fl32(x) * 2^-32 + 2^-33), which lies in (0, 1]; a u that rounds to 1.0 is
 *     allowed and gives a radius of 0;
 *   r(u) = sqrt(-2 ln u);
 *   z0 = r(u(x0)) * sin(2 pi u(x1)), z1 = r(u(x0)) * cos(2 pi u(x1)),
 *   z2 = r(u(x2)) * sin(2 pi u(x3)), z3 = r(u(x2)) * cos(2 pi u(x3));
 *   element e is z_i.
 * The uint32 words are specified bit-exactly (the Random123 known answers hold).  The
 * normals are specified to a tolerance, because log, sin and cos differ between math
 * libraries: |z - z_ref| <= 16 * 2^-24 * (1 + r) against a float64 evaluation of the rules
 * above on the fp32 u.  What the device computes is bitwise the same for the same
 * (seed, stream, e): it does not depend on B, the row stride, pointer alignment, launch
 * geometry, or on which operand build (bf16 / fp16) of the library is loaded.  A row's first
 * len * F elements therefore do not depend on the batch's frame count.
 * ---------------------------------------------------------------------- */
/* seeds: [B] device int64, the bit pattern is the unsigned 64-bit seed; streams: [B] device
 * int32 (the bit pattern is the unsigned 32-bit stream), or NULL for all zero; n elements
 * per row, ld >= n the row stride in floats.  Writes out[b * ld + e] for b < B, e < n and
 * nothing else: columns [n, ld) are not touched.  Stateless (no handle, no allocation) and
 * without a host-blocking runtime call; one launch on `stream`.  Rejected: B <= 0 or
 * B > 65535, n < 0 or n > 2^40, ld < n, null seeds / out with n > 0.  n == 0 succeeds and
 * launches nothing. */
int zv_noise_normal(const int64_t* seeds, const int32_t* streams, int B, int64_t n, int64_t ld,
                    float* out, void* stream);

/* The two layers of the noise function on their own (test infrastructure;
 * tests/test_noise_spec.py, tests/test_gpu_noise.py).  Host pointers throughout; where 0
 * runs the library's host functions (no GPU needed), where 1 the same source as device
 * functions in a one-off kernel, copied back.
 * ZV_NOISE_BITS: bits[4 * count] receives Philox4x32-10(counter + k, key) for
 *   k = 0 .. count - 1, where k is added to the 64-bit number formed by counter[0] (low)
 *   and counter[1] (high), so the carry from word 0 into word 1 can be reached; counter[2]
 *   and counter[3] stay.
 * ZV_NOISE_NORMALS: words[4 * count] caller-chosen uint32 go in as `count` quadruples
 *   (x0, x1, x2, x3); normals[4 * count] receives their (z0, z1, z2, z3).
 * count is in [0, 2^26]; 0 succeeds and does nothing. */
enum { ZV_NOISE_BITS = 0, ZV_NOISE_NORMALS = 1 };
typedef struct {
  int mode;                 /* ZV_NOISE_BITS / ZV_NOISE_NORMALS */
  int where;                /* 0 host, 1 device */
  uint32_t counter[4];      /* BITS: the start counter */
  uint32_t key[2];          /* BITS: the key */
  int64_t count;            /* BITS: blocks; NORMALS: word quadruples */
  const uint32_t* words;    /* NORMALS in */
  uint32_t* bits;           /* BITS out */
  float* normals;           /* NORMALS out */
} zv_noise_check_args;
int zv_noise_check(zv_noise_check_args* a);

#ifdef __cplusplus
}
#endif
#endif /* ZIPVOICE_HIP_H */
