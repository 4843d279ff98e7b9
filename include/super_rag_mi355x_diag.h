/* super_rag_mi355x_diag.h -- the diagnostic surface of the MI355X hot-path library.
 *
 * Exported by libsrmi_diag.so only (make -C super-rag_amd: the product sources built again with
 * SR_WITH_DIAG=1), never by the product library libsrmi.so.  These entry points drive ONE kernel
 * on device buffers for single-kernel parity tests (tests/test_gpu_gemm.py, test_gpu_attention.py,
 * test_gpu_ffn1_epilogue.py, test_gpu_ffn1_gelu_sweep.py, test_gpu_gemm_f8_fold.py,
 * test_gpu_fold_helpers.py, test_gpu_qkv_attention.py, test_gpu_attention_exact.py,
 * test_gpu_cls_attn_fold.py), microbenchmarks (tools/) and the measured peaks of bench.py; the
 * timing-only variants return wrong results by design.  The diagnostic library also honours the
 * A/B environment knobs of DESIGN.md §4 (SR_GEMM_GROUP_M, SR_GEMM_STAGGER, SR_SCAN_CHUNK,
 * SR_SCAN_GROWTH, SR_SCAN_LEGACY, SR_SCAN_DIAG_NOEPI, SR_QA_DIAG, SR_FFN1_DIAG_WALKERS), which the
 * product library ignores.  No reference counterpart (the reference has no kernels).
 */
#ifndef SUPER_RAG_MI355X_DIAG_H
#define SUPER_RAG_MI355X_DIAG_H

#include "super_rag_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* ------------------------------------------------------------------------------------------------
 * Diagnostics (microbenchmarks / parity tests of a single kernel; not used by the product path)
 * ---------------------------------------------------------------------------------------------- */
/* One encoder GEMM Y = epi(X W^T + bias (+R)) on device buffers: X M x K fp16 (row stride lda),
 * W N x K fp16, bias N fp32, R residual (epi 2: fp32, epi 4: fp16, row stride ldr), Y row stride
 * ldy (fp16 for epi 0/1/4, fp32 for 2/3).  epi: 0 bias, 1 bias+GELU, 2 bias+residual fp32,
 * 3 bias+tanh (fp32 out), 4 bias+residual fp16.  variant: -1 auto, 0 128x128, 1 256x256 (8 waves,
 * 2-stage), 4 pipelined 256x256, 5 persistent pipelined 256x256 (6 / 7: timing-only diagnostics
 * with wrong results); variant | 0x100 = split weights: W is [hi | lo] (N x K) over an X of K / 2
 * columns (the embedders' precision mode). */
int sr_diag_gemm(int variant, int epi, const void* X, int64_t lda, const void* W, const float* bias,
                 const void* R, int64_t ldr, void* Y, int64_t ldy, int M, int N, int K, int device,
                 void* stream);

/* Diagnostic: sr_diag_gemm on the 128x128 kernel the way the embedders call it (Encoder::forward's
 * lin): with a lent workspace ws of ws_bytes on the device, so the K-steps are summed in chunks of
 * 6 and, when the host heuristic of launch_gemm_variant splits (>= 2 chunks, <= 128 tiles,
 * chunks x tiles x 64 KiB <= ws_bytes), the chunk groups run in separate workgroups that store
 * partial tiles to ws and gemm_chunk_reduce_kernel finishes the tile.  Arguments and epilogues as
 * sr_diag_gemm; variant is ignored apart from | 0x100 (split weights): the 128x128 kernel always. */
int sr_diag_gemm_chunked(int variant, int epi, const void* X, int64_t lda, const void* W,
                         const float* bias, const void* R, int64_t ldr, void* Y, int64_t ldy, int M,
                         int N, int K, void* ws, int64_t ws_bytes, int device, void* stream);

/* Diagnostic: the LayerNorm-folded FFN1 GEMM Y = 2 GELU(rstd_m (X W^T - mu_m colsum) + bias) on
 * device buffers (the cross-encoders' FFN1 epilogue), fp16 (f8 = 0: X M x K, W N x K fp16, Y fp16)
 * or fp8 (f8 = 1: X, W OCP e4m3 bytes, wexp the E8M0 exponent byte of each W row, Y e4m3 bytes);
 * mr = (mu, rstd) per X row, colsum / bias N fp32.  diag: 0 the product kernel, 2 the main loop
 * without an epilogue, 5 the epilogue math without its stores, 6 the stores of the raw
 * accumulators without the math, 7 the product epilogue with every tile's stores folded onto the
 * first tile (L2-resident) (2 / 5 / 6 / 7: timing only, wrong results). */
int sr_diag_ffn1(int diag, int f8, const void* X, int64_t lda, const void* W, const uint8_t* wexp,
                 const float* bias, const float* colsum, const float* mr, void* Y, int64_t ldy, int M,
                 int N, int K, int device, void* stream);

/* Diagnostic: the residual + row-statistics GEMM epilogue (EPI_RES16_STATS, the encoders'
 * O-projection / FFN2 of layer 0) on device buffers: Y = fp16(X W^T + bias + R) (X M x K fp16, W
 * N x K fp16, bias N fp32, R / Y M x N fp16, row strides ldr / ldy, N % 256 == 0) and per row m and
 * 128-column span s the partials stat_out[(m * N / 128 + s) * 2 + {0, 1}] = (sum, M2) of the fp16
 * outputs of that span (the LayerNorm statistics ln_stats_finalize combines). */
int sr_diag_gemm_stats(const void* X, int64_t lda, const void* W, const float* bias, const void* R,
                       int64_t ldr, void* Y, int64_t ldy, int M, int N, int K, float* stat_out,
                       int device, void* stream);

/* Diagnostic: the FFN2 / O-projection GEMM of the LN-folded encoders, EPI_LNR16_STATS:
 * Y = X W^T + bias + ((R - mu) rstd) gamma per row (R un-normalised, mr = (mu, rstd) per row,
 * consecutive), fp16 Y, and the (sum, M2) partials of every 128-column span of Y as
 * sr_diag_gemm_stats. */
int sr_diag_gemm_lnr_stats(const void* X, int64_t lda, const void* W, const float* bias, const void* R,
                           int64_t ldr, const float* mr, const float* gamma, void* Y, int64_t ldy, int M,
                           int N, int K, float* stat_out, int device, void* stream);

/* Diagnostic: the e4m3-copy statistics epilogues (fp8 mode 3's O-projection: EPI_LNR16_STATS_Y8
 * when lnr != 0, as sr_diag_gemm_lnr_stats; EPI_RES16_STATS_Y8 otherwise, as sr_diag_gemm_stats,
 * mr / gamma unused): fp16 Y, its e4m3 copy y8 (bytes, row stride ldy) and the (sum, M2) partials. */
int sr_diag_gemm_stats_y8(int lnr, const void* X, int64_t lda, const void* W, const float* bias,
                          const void* R, int64_t ldr, const float* mr, const float* gamma, void* Y,
                          int64_t ldy, uint8_t* y8, int M, int N, int K, float* stat_out, int device,
                          void* stream);

/* Diagnostic: one LayerNorm-folded encoder GEMM the way the product launches it (launch_gemm /
 * launch_gemm_f8w with the automatic kernel choice, no forced variant), every LnFold field and row
 * stride from the arguments.  f8 = 0: X M x K, W N x K fp16; f8 = 1: X, W OCP e4m3 bytes (K % 128
 * == 0, K >= 256) and wexp the E8M0 exponent byte of each W row (W = W8 2^(wexp - 127)).  epi (the
 * Epilogue codes): 5 EPI_LNF_F16 Y = rstd_m (X W^T - mu_m colsum) + bias; 7 EPI_RES16_STATS Y =
 * X W^T + bias + R; 8 EPI_LNR16_STATS Y = X W^T + bias + ((R - mu_m) rstd_m) gamma; 12 / 13 = 7 / 8
 * that also store e4m3(Y) bytes to y8 (row stride ldy).  (mu_m, rstd_m) = mr[2 m stat_ld + {0, 1}]
 * (row m of the operand reads statistics row m x stat_ld); R / Y fp16 with row strides ldr / ldy
 * (Y may alias R); stat_out [M][N / 128][2] the (sum, M2) partials of the fp16 Y (epi 7, 8, 12,
 * 13).  Buffers an epilogue does not read may be null.  N % 256 == 0, M > 0. */
int sr_diag_gemm_fold(int f8, int epi, const void* X, int64_t lda, const void* W, const uint8_t* wexp,
                      const float* bias, const float* colsum, const void* R, int64_t ldr, const float* mr,
                      int64_t stat_ld, const float* gamma, void* Y, int64_t ldy, uint8_t* y8,
                      float* stat_out, int M, int N, int K, int device, void* stream);

/* Diagnostic: the weight-side helpers of the LayerNorm fold and the fp8 plan, one kernel each on
 * device buffers.  quantize_rows_fp8: W N x K fp16 -> W8 e4m3(W 2^e_n) bytes with e_n the largest
 * power of two keeping max|W_n| 2^e_n <= 448 (0 for a zero row), wexp[n] = 127 - e_n.  colsum_fp8:
 * colsum[n] = sum_k W8[n][k] 2^(wexp[n] - 127).  fold_ln_weight: w16 = fp16(w32 . diag(gamma)),
 * colsum[n] = sum_k float(w16[n][k]), bias_out[n] = sum_k w32[n][k] beta[k] + bias[n].
 * ln_stats_finalize: mr[m] = (mu, rstd = 1 / sqrt(var + eps)) of row m from its nparts (1..16)
 * (sum, M2) partials over 128-column spans, stat [M][nparts][2]. */
int sr_diag_quantize_rows_fp8(const void* W, int N, int K, uint8_t* W8, uint8_t* wexp, int device,
                              void* stream);
int sr_diag_colsum_fp8(const uint8_t* W8, const uint8_t* wexp, int N, int K, float* colsum, int device,
                       void* stream);
int sr_diag_fold_ln_weight(const float* w32, const float* gamma, const float* beta, const float* bias,
                           int N, int K, void* w16, float* colsum, float* bias_out, int device,
                           void* stream);
int sr_diag_ln_stats_finalize(const float* stat, int nparts, float eps, int M, float* mr, int device,
                              void* stream);

/* Diagnostic: the MFMA issue-rate peak on this box (k_diag.hip).  blocks workgroups of 8 waves,
 * each wave 8 independent accumulator chains x iters of the product's MFMA (f8 = 0: f16
 * 16x16x32; f8 = 1: block-scaled fp8 16x16x128) on random operands; FLOP = blocks x 8 x iters x 8 x
 * 16 x 16 x K x 2 (K = 32 / 128).  sink: device float [blocks x 512]; stamps: device uint64
 * [blocks x 2] = (d s_memtime, d s_memrealtime) of each block's loop (clock = ratio x 100 MHz). */
int sr_diag_mfma_rate(int f8, int blocks, int iters, float* sink, uint64_t* stamps, int device, void* stream);

/* Diagnostic: sr_diag_gemm_lnr_stats's persistent kernel with in-kernel s_memtime phase stamps
 * (stamps: device uint64 [grid x 8 waves x 8], sr_diag_ffn1_stamps' layout; grid = 8 x min(32,
 * ceil(tiles / 8))). */
int sr_diag_gemm_lnr_stats_stamps(const void* X, int64_t lda, const void* W, const float* bias, const void* R,
                                  int64_t ldr, const float* mr, const float* gamma, void* Y, int64_t ldy, int M,
                                  int N, int K, float* stat_out, uint64_t* stamps, int device, void* stream);

/* Diagnostic: K5c (fused QKV projection + attention, LN-folded: X un-normalised rows, W the folded
 * [Q; K; V] weight (3d x d), bias the folded bias, colsum its row sums, mr (mu, rstd) per row; S ==
 * 128, head dim 64) with in-kernel s_memtime phase stamps.  stamps: device uint64 [grid x 8 waves
 * x 8] = per wave [tiles, cycles of: the K-loop, the epilogue into the LDS images, the attention,
 * the tile transition, 0, 0, 0]; grid = 8 x min(32, ceil(B S / 256 x heads / 8)). */
int sr_diag_qkv_attention_stamps(const void* X, int64_t lda, const void* W, const float* bias,
                                 const float* colsum, const float* mr, const int32_t* mask, void* ctx, int B,
                                 int S, int d, int heads, uint64_t* stamps, int device, void* stream);

/* Diagnostic: K5c the way the encoder launches it (launch_qkv_attention without stamps, fp16 ctx):
 * the product instantiations qkv_attn_kernel<false> (epi 0, EPI_BIAS_F16: Q | K | V = X W^T + bias;
 * colsum / mr may be null) and qkv_attn_kernel<true> (epi 5, EPI_LNF_F16: rstd_m (X W^T - mu_m
 * colsum) + bias, mr = (mu, rstd) per row).  X [B*S, lda] fp16 (lda >= d, lda % 8 == 0), W [3d, d]
 * fp16, bias / colsum [3d] fp32, mask [B, S] int32, ctx [B*S, d] fp16; S == 128, d == 64 heads.
 * The e4m3 ctx form (fp8 mode 5) is left out: that mode was rejected and exists only in the
 * diagnostic library. */
int sr_diag_qkv_attention(int epi, const void* X, int64_t lda, const void* W, const float* bias,
                          const float* colsum, const float* mr, const int32_t* mask, void* ctx, int B, int S,
                          int d, int heads, int device, void* stream);

/* Diagnostic: the K/V-free CLS-only last layer's attention (launch_cls_attn_fold): w [B, H, D] fp16
 * (the CLS query folded through W'_k per head), U [B*S, D] fp16 un-normalised rows, mr (mu, rstd)
 * per row, mask [B, S] int32 -> z [B, 2 H D] fp16 = [hi(H D) | lo(H D)] of z'_h = sum_j p_j rstd_j
 * (u_j - mu_j), p = softmax_j(rstd_j (w_h . u_j - mu_j sum(w_h)) / 8) over the live tokens.  D / H in
 * {768 / 12, 1024 / 16}, S % 16 == 0, 16 <= S <= 512; every sequence needs a live token.  S <= 128
 * runs the single-read form unless SR_CLS_FOLD_1READ=0 (read per launch). */
int sr_diag_cls_attn_fold(const void* w, const void* U, const float* mr, const int32_t* mask, int B, int S,
                          int D, int H, void* z, int device, void* stream);

/* Diagnostic: the block-diagonal weights of that layer (launch_kv_blockdiag) from the folded QKV
 * weight wqkv_f [3D, D] fp16: wk_bd [H D, D], wv_bd [D, 2 H D] fp16. */
int sr_diag_kv_blockdiag(const void* wqkv_f, int D, int H, void* wk_bd, void* wv_bd, int device,
                         void* stream);

/* Diagnostic: the fp16 FFN1 of sr_diag_ffn1 with in-kernel s_memtime phase stamps (diag 9: the
 * product epilogue, 10: its math without the global stores, 11: the product epilogue without the
 * next tile's staging in its shadow -- timing only, wrong results).  stamps: device uint64 [grid x 8
 * waves x 8] = per wave [tile transitions, cycles of: K-step 0 (tile start -> its barrier),
 * K-step 1, the rest of the K-loop, the epilogue, the transition wait + barrier, K-steps per
 * tile, 0] (grid = 8 x min(32, tiles / 8) persistent workgroups). */
int sr_diag_ffn1_stamps(int diag, const void* X, int64_t lda, const void* W, const float* bias,
                        const float* colsum, const float* mr, void* Y, int64_t ldy, int M, int N,
                        int K, uint64_t* stamps, int device, void* stream);

/* Diagnostic: device-to-device copy of `bytes` (multiple of 16) with 16-byte lanes, the HBM
 * yardstick bench.py reports beside the spec peak (no reference counterpart). */
int sr_diag_copy(const void* src, void* dst, int64_t bytes, int device, void* stream);

/* Diagnostic: one attention launch (K5) on device pointers.  qkv: [B*S, 3d] fp16 (Q | K | V),
 * mask: [B, S] int32 (0 = padding key), ctx: [B*Sq, d] fp16 (first Sq query rows of every
 * sequence).  variant: -1 auto, 0 the 64-key-tile kernel, 1 the whole-head-in-LDS kernel with 4
 * waves per workgroup, 2 the same with 8 waves, 3 auto but the per-workgroup K5b STREAM form instead
 * of the persistent K5d at S_pad = 512 (variants 1-3: d/heads must be 64 and S <= 512). */
int sr_diag_attention(int variant, const void* qkv, const int32_t* mask, void* ctx, int B, int S,
                      int Sq, int d, int heads, int device, void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif

#endif /* SUPER_RAG_MI355X_DIAG_H */
