// Host-side launchers of the HIP kernels (one declaration per kernel family).
#pragma once

#include "sr_common.h"
#include "sr_gemm_plan.h"  // Epilogue, GemmVariant

namespace sr {

// Per-row statistics hand-over between GEMMs (Chan-combinable partials over 128-column spans):
// stat[row][part] = (sum, M2 = sum (x - sum/128)^2) of the fp16-rounded outputs in that span.
// launch_ln_stats_finalize turns them into mr[row] = (mu, rstd), which the folded epilogues read.
struct LnFold {
  const float* mr = nullptr;       // (mu, rstd) of the A rows (LNF) / residual rows (LNR)
  int64_t stat_ld = 1;             // row r of the operand reads mr row r * stat_ld
  const float* colsum = nullptr;   // LNF: c[n] = sum_k W'[n][k] (fp32 sum of the fp16 W')
  const float* gamma = nullptr;    // LNR: LayerNorm weight of the residual rows (its beta is
                                   //      pre-added to the GEMM bias)
  float* stat_out = nullptr;       // *_STATS: [M][N / 128] partials of the output rows
  const uint8_t* wexp = nullptr;   // fp8 operands (launch_gemm_f8w): E8M0 exponent per weight row
  uint8_t* y8 = nullptr;           // *_STATS: optional e4m3 copy of the fp16 output (row stride
                                   //          ldy bytes), the next fp8 GEMM's A operand
  int group_m = 0;                 // pipelined kernels: tile t walks groups of group_m m-panels
                                   // (m fastest inside a group); 0 / 1 = n fastest
  int stagger = 0;                 // persistent pipelined kernels (diagnostic): > 0: walker w of
                                   // an XCD starts (w & 7) x stagger x 512 cycles late; < 0: the
                                   // walkers of XCD x start x |stagger| x 512 cycles late
                                   // (de-phasing the epilogue store bursts)
  int x_k = 0;                     // split weights: X has x_k columns and K = 2 x_k; the K-steps
                                   // past x_k re-read X from k = 0, so W = [W_hi | W_lo] (N x 2 x_k)
                                   // gives X W_hi^T + X W_lo^T in one fp32 accumulation (0 = K)
  float* chunk_ws = nullptr;        // GEMM_SMALL (128 x 128, short M): workspace for split-K
  int64_t chunk_ws_bytes = 0;      // partial tiles (sr_gemm_plan.h KCHUNK); null: never split
  // EPI_SCAN(8) re-uses the fields (kernel-argument SGPRs are scarce in the persistent kernels):
  // stat_out = per-query candidate counts (int*), stat_ld = global row id of the chunk's first
  // row; bias = tau[B], R = live flags of the chunk, Y = candidate keys [B][cap] (ldy = cap).
};

// k_gemm.hip — Y = epi(X . W^T + bias (+ R)); K % 64 == 0, N % 128 == 0.
void launch_gemm(int epi, const half_t* X, int64_t lda, const half_t* W, const float* bias,
                 const void* R, int64_t ldr, void* Y, int64_t ldy, int M, int N, int K,
                 hipStream_t stream, const LnFold* lf = nullptr);
void launch_gemm_variant(int variant, int epi, const half_t* X, int64_t lda, const half_t* W,
                         const float* bias, const void* R, int64_t ldr, void* Y, int64_t ldy,
                         int M, int N, int K, hipStream_t stream, const LnFold* lf = nullptr);
void gemm_force_tile(int t);  // test hook: -1 auto, else a GemmVariant
#if SR_WITH_DIAG
// Diagnostic FFN1 launches (sr_diag_ffn1): diag 0 product, 2 no epilogue, 5 math only, 6 stores only.
void launch_ffn1_diag(int diag, bool f8, const void* X, int64_t lda, const void* W, const uint8_t* wexp,
                      const float* bias, const float* colsum, const float* mr, void* Y, int64_t ldy,
                      int M, int N, int K, hipStream_t stream, uint64_t* stamps = nullptr);
// MFMA issue-rate peak (k_diag.hip): blocks x 8 waves x iters x 8 independent MFMAs of the
// product's f16 (f8 = 0) or block-scaled fp8 (f8 = 1) shape on random operands; stamps[2 b] /
// [2 b + 1] = d(s_memtime) / d(s_memrealtime) of block b's wave 0 around its loop.
void launch_mfma_rate(int f8, int blocks, int iters, float* sink, uint64_t* stamps, hipStream_t st);
// The persistent EPI_LNR16_STATS GEMM with in-kernel phase stamps (k_gemm.hip; diagnostic)
void launch_lnr_stats_stamps(const half_t* X, int64_t lda, const half_t* W, const float* bias, const void* R,
                             int64_t ldr, const float* mr, const float* gamma, void* Y, int64_t ldy, int M,
                             int N, int K, float* stat_out, uint64_t* stamps, hipStream_t stream);
#endif
// Y = epi(X8 . W8^T) on OCP e4m3 operands: X8 [M][K] bytes (lda bytes), W8 [N][K] bytes with
// per-row E8M0 exponents lf->wexp[N] (W = W8 * 2^(wexp - 127)); K % 128 == 0, K >= 256,
// N % 256 == 0, lda % 16 == 0, ldy % 8 == 0, ldr % 8 == 0;
// epi in {EPI_LNF_F16, EPI_LNF_GELU_F8, EPI_RES16_STATS(_Y8), EPI_LNR16_STATS(_Y8)}.
void launch_gemm_f8w(int epi, const uint8_t* X8, int64_t lda, const uint8_t* W8, const float* bias,
                     const void* R, int64_t ldr, void* Y, int64_t ldy, int M, int N, int K,
                     hipStream_t stream, const LnFold* lf);
// colsum[n] = sum_k W8[n][k] * 2^(wexp[n] - 127) (the LN fold's column sums of an e4m3 weight)
void launch_colsum_fp8(const uint8_t* W8, const uint8_t* wexp, int N, int K, float* colsum,
                       hipStream_t s);
// W [N][K] fp16 -> W8 [N][K] e4m3 of W * 2^e_n (largest power of two with max|W_n| 2^e_n <= 448),
// wexp[n] = 127 - e_n
void launch_quantize_rows_fp8(const half_t* W, int N, int K, uint8_t* W8, uint8_t* wexp,
                              hipStream_t s);
// fp8 rows e4m3(256 x) (ld8 bytes, a multiple of 128, >= 256) of unit vectors; sims are cosines.
void launch_cosine_scan_gemm8(const uint8_t* corpus8, int64_t ld8, const uint8_t* live, int64_t r0,
                              int64_t r1, const uint8_t* Q8, int B, const float* tau, uint64_t* cand,
                              int* cnt, int cap, hipStream_t s);
// fp8 K1 for B <= 64 (k_search.hip): the small-block scan kernel on e4m3 rows (ld8 bytes each)
void launch_cosine_scan8(bool dense, const uint8_t* corpus8, int64_t ld8, const uint8_t* live,
                         int64_t r0, int64_t r1, const uint8_t* Q8, int B, const float* tau,
                         uint64_t* cand, int* cnt, int cap, hipStream_t s);
// K1 for large query blocks (B in (128, 256]) on the pipelined GEMM: rows [r0, r1) of the corpus
// against B queries; non-dense threshold mode only (same contract as launch_cosine_scan).
void launch_cosine_scan_gemm(const half_t* corpus, int64_t ldc, const uint8_t* live, int64_t r0,
                             int64_t r1, const half_t* Q, int B, const float* tau, uint64_t* cand,
                             int* cnt, int cap, hipStream_t s);

// k_attention.hip — ctx = MHA(qkv, key padding mask) for the first Sq query rows of each
// sequence; ctx rows are laid out [B][Sq][d].
// K5c (k_attention.hip): ctx = attention(epi(X . Wqkv^T)) without the QKV activation in HBM;
// epi = EPI_BIAS_F16 or EPI_LNF_F16 (lf: row statistics mr, column sums colsum).  S == 128, d_h == 64.
// ctx8 != nullptr: ctx is written there as OCP e4m3 bytes instead ([B*S, d], fp8 mode 5).
bool qkv_attention_supported(int S, int d, int heads);
void launch_qkv_attention(int epi, const half_t* X, int64_t lda, const half_t* W, const float* bias,
                          const LnFold* lf, const int32_t* mask, half_t* ctx, int B, int S, int d,
                          int heads, hipStream_t stream, uint8_t* ctx8 = nullptr,
                          uint64_t* stamps = nullptr);
void launch_attention(const half_t* qkv, const int32_t* mask, half_t* ctx, int B, int S, int Sq,
                      int d, int heads, hipStream_t stream);
void attention_force_variant(int v);  // test hook: -1 auto, 0 = 64-key-tile kernel, 1 = K5b, 2 = K5b with 8 waves

// k_encoder_misc.hip
void launch_positions(const int32_t* ids, int32_t* pos, int B, int S, int offset, hipStream_t s);
// h32 may be null (fp16 residual stream): then only the fp16 copy is written.
void launch_embed_ln(const int32_t* ids, const int32_t* pos, const int32_t* types,
                     const half_t* wemb, const half_t* pemb, const half_t* temb,
                     const float* gamma, const float* beta, float eps, int M, int d, int vocab,
                     int max_pos, int type_vocab, half_t* h16, float* h32, hipStream_t s);
// y is fp32 (y_f16 = false) or fp16; h32 may be null.
void launch_layernorm(const void* y, bool y_f16, const float* gamma, const float* beta, float eps,
                      int M, int d, half_t* h16, float* h32, hipStream_t s);
void launch_pool_l2(const void* h, bool h_f16, const int32_t* mask, int B, int S, int d, int pool,
                    void* out, int out_dtype, int ld_out, hipStream_t s);
// sparse head: tw[t] = max(0, h[t] . w + bias) where mask[t] != 0, else 0 (h: M x d final states)
void launch_sparse_token_weights(const void* h, bool h_f16, const int32_t* mask, const float* w,
                                 const float* bias, int M, int d, float* tw, hipStream_t s);
// token -> term collapse of B sequences of S tokens (device ids / mask / tw, host special_ids):
// out_terms / out_weights B x S (-1 / 0 past the count), out_count B
void sparse_terms_check_args(int B, int S, int n_special);
void launch_sparse_terms(const int32_t* ids, const int32_t* mask, const float* tw, int B, int S,
                         const int32_t* special_ids, int n_special, int32_t* out_terms,
                         float* out_weights, int32_t* out_count, hipStream_t s);
// multi-vector head (k_encoder_misc.hip colbert_pack): v [B][S][dc] fp16 (the head's GEMM output) ->
// out [B][S][dc]: the rows of the positions s >= 1 with mask != 0, L2-normalised in fp32
// (v / max(||v||, 1e-12)) and compacted in position order, zero rows behind them; out_len [B]
void colbert_pack_check_args(int B, int S, int dc);
void launch_colbert_pack(const half_t* v, const int32_t* mask, int B, int S, int dc, half_t* out,
                         int32_t* out_len, hipStream_t s);
void launch_cls_logits(const float* t, const float* w, const float* bias, int P, int d,
                       int labels, float* out, hipStream_t s);
void launch_normalize_rows(const void* x, int dtype, int64_t n, int dim, half_t* out, int ld,
                           hipStream_t s);
void launch_convert_f32_f16(const float* in, half_t* out, int64_t n, hipStream_t s);
// LayerNorm folding of a [N][K] fp32 weight behind LN(gamma, beta): w16 = fp16(W . diag(gamma)),
// colsum[n] = sum_k float(w16[n][k]), bias_out[n] = sum_k W[n][k] beta[k] + bias[n].
void launch_fold_ln_weight(const float* w32, const float* gamma, const float* beta,
                           const float* bias, int N, int K, half_t* w16, float* colsum,
                           float* bias_out, hipStream_t s);
// mr[r] = (mu, rstd) of row r from its nparts Chan partials (n = 128 each), rstd = 1/sqrt(var+eps).
void launch_ln_stats_finalize(const float* stat, int nparts, float eps, int M, float* mr,
                              hipStream_t s);
// h16 = LayerNorm(u) with (mu, rstd) from mr (no re-reduction).
void launch_ln_apply(const half_t* u, int64_t ldu, const float* mr, const float* gamma,
                     const float* beta, int M, int d, half_t* h16, hipStream_t s);
void launch_vec_add(const float* a, const float* b, float* out, int n, hipStream_t s);
// fp8 mode 4: e4m3 copy of the normalised rows (u - mu) rstd (k_encoder_misc.hip)
void launch_quantize_norm_fp8(const half_t* u, int64_t ldu, const float* mr, int M, int d, uint8_t* x8,
                              hipStream_t s);
// K/V-free CLS-only last layer (k_encoder_misc.hip): block-diagonal K / V weights from the folded
// QKV weight, and per sequence scores + softmax + z' = sum_j p_j rstd_j (u_j - mu_j).
// Contract: every sequence has at least one live token (the encoder's CLS token is always live);
// an all-masked sequence divides by a zero softmax sum and is outside it.  U rows and mr entries
// of masked tokens may hold any finite values (they meet a weight of exactly 0).
bool cls_attn_fold_supported(int S, int D, int H);
void launch_kv_blockdiag(const half_t* wqkv_f, int D, int H, half_t* wk_bd, half_t* wv_bd,
                         hipStream_t s);
void launch_cls_attn_fold(const half_t* w, const half_t* U, const float* mr, const int32_t* mask,
                          int B, int S, int D, int H, half_t* z, hipStream_t s);
void launch_scale_f16(const half_t* in, float scale, half_t* out, int64_t n, hipStream_t s);

// k_search.hip
int scan_query_tiles(int B);
int select_capacity();
void launch_cosine_scan(bool dense, const half_t* corpus, int64_t ldc, const uint8_t* live,
                        int64_t r0, int64_t r1, const half_t* Q, int B, const float* tau,
                        uint64_t* cand, int* cnt, int cap, hipStream_t s);
void launch_topk_select(uint64_t* cand, int* cnt, int cap, float* tau, int B, int k,
                        int* overflow, bool final_pass, float* out_sim, int64_t* out_rows,
                        int64_t row_offset, hipStream_t s,
                        const uint8_t* live = nullptr);
void launch_topk_merge(const float* sims, const int64_t* rows, int P, int B, int k, int k_out,
                       float* out_sim, int64_t* out_rows, hipStream_t s);
void launch_fill_int(int* p, int n, int v, hipStream_t s);
void launch_copy16(const void* src, void* dst, int64_t bytes, hipStream_t s);  // diagnostic
void launch_fill_float(float* p, int n, float v, hipStream_t s);
void launch_build_pairs(const int32_t* q_tok, const int32_t* q_len, int lq_max,
                        const int32_t* p_tok, const int32_t* p_len, int lp_max,
                        const int64_t* cand_rows, int B, int K, int S, int style, int bos, int eos,
                        int pad, int32_t* out_ids, int32_t* out_mask, int32_t* out_type,
                        hipStream_t s);
void launch_rerank_select(const float* logits, int B, int K, int k_out, int32_t* out_index,
                          hipStream_t s);

// k_mmr.hip — MMR diversification of K <= SR_MMR_MAX_CAND candidates per query (one workgroup
// each).  Candidate i of query b is row cand_rows[b K + i] - row_offset of `rows` (cand_rows < 0 or a
// row outside [0, n_rows): missing), or, with cand_rows null, row b K + i for i < n_cand[b] (null:
// K).  rel [B][K] = cos(query, candidate), or null: computed from the normalised queries qn
// [B][ld].  Outputs B x k_out in MMR order (-inf / -inf / -1 / -1 past the end): MMR score, rel of
// the kept candidate (null: skipped), its position (null: skipped), its cand_rows entry (null:
// skipped).  mmr_check_args throws SR_ERR_INVALID for arguments outside the documented limits.
void mmr_check_args(int B, int K, int k_out, float lambda, int mode);
void launch_mmr_rerank(const half_t* rows, int64_t ld, int64_t n_rows, const int64_t* cand_rows,
                       int64_t row_offset, const int32_t* n_cand, const float* rel,
                       const half_t* qn, int B, int K, float lambda, int mode, float min_score,
                       int k_out, float* out_score, float* out_sim, int32_t* out_index,
                       int64_t* out_rows, hipStream_t s);

// k_subset.hip — scores of per-query row lists as keys in the per-query candidate lists (K2
// launch_topk_select finishes).  Lists: CSR list_off / list_rows (device).  Groups: grp_q [G][16]
// query indices of the block (-1: none) that share list grp_list[g].  items [n_items][2] =
// (group, first list position of a SR_SUBSET_CHUNK-row chunk, relative to pass0), ordered
// [list][chunk][group].  A pass covers list positions [pass0, pass0 + pass_rows); position i's key
// goes to slot head + (i - pass0) (zero key for a row outside [0, n_rows)).  launch_subset_prep
// (before every pass; q_list [B] = list of each query of the block) sets cnt and, for pass0 > 0,
// zeroes the slots between the kept winners and k.  query_rows / group_rows: rows of the pass
// summed over queries / groups (profiling only).
constexpr int SR_SUBSET_CHUNK = 512;
void launch_subset_prep(const int32_t* q_list, const int64_t* list_off, int64_t pass0,
                        int pass_rows, int B, int k, uint64_t* cand, int cap, int* cnt,
                        hipStream_t s);
void launch_subset_scan(const half_t* corpus, int ld, int64_t n_rows, const half_t* Q,
                        const int32_t* items, int n_items, const int32_t* grp_q,
                        const int32_t* grp_list, const int64_t* list_off, const int64_t* list_rows,
                        int64_t pass0, int pass_rows, int head, uint64_t* cand, int cap,
                        double query_rows, double group_rows, hipStream_t s);

// k_group.hip — grouped search: the k best distinct groups of a query with the group_size best rows
// of each.  launch_group_collapse (one workgroup per query) walks the K candidates search_dev wrote
// (cand_rows carry row_offset, -1 past the end) together with C rows carried from earlier rounds
// (same form; C == 0: none); group [n_rows] int32: >= 0 a group, -1 a group of its own.  Outputs:
// B x k x group_size similarity / row (-inf / -1 unfilled), B x k group id (-1), per query n_groups,
// complete (the result is already exact) and found [B][k]: ascending (group key << 1 | full), the
// state launch_group_mask reads; next_sims / next_rows (or null) receive the rows of the full
// groups in the output layout, the next round's carried rows.  launch_group_mask (one query):
// out[row] = base[row] && the row's group can still take rows (not full; not found counts only
// while fewer than k groups are found).  group_check_args throws SR_ERR_INVALID outside the limits.
void group_check_args(int B, int K, int k, int group_size);
void launch_group_collapse(const float* cand_sims, const int64_t* cand_rows, int B, int K,
                           const float* carry_sims, const int64_t* carry_rows, int C,
                           int64_t row_offset, const int32_t* group, int64_t n_rows, int k,
                           int group_size, float* out_sim, int64_t* out_rows, int32_t* out_group,
                           int32_t* n_groups, int32_t* complete, uint64_t* found, float* next_sims,
                           int64_t* next_rows, hipStream_t s);
void launch_group_mask(const uint8_t* base, const int32_t* group, int64_t n_rows,
                       const uint64_t* found, const int32_t* n_groups, int k, uint8_t* out,
                       hipStream_t s);

// k_fuse.hip — score fusion of two scored row lists per query (one workgroup each; the function is
// stated in include/super_rag_mi355x.h): lists (score, rows) of ka / kb entries, row < 0 absent,
// side_a [B][kb] optional a-scores of the b rows, side_b [B][ka] optional b-scores of the a rows; outputs B x k_out by (fused desc, row asc),
// -inf / -1 unfilled, out_a / out_b optional components.  fuse_check_args throws SR_ERR_INVALID
// outside the documented limits (allow_full: SR_FUSE_FLOOR_FULL passes, for sr_hybrid_search_fused).  launch_score_rows: out[b][j] = qn_b . row (rows[b][j] - row_offset)
// over the fp16 rows (qn [B][ld] normalised, zero padded), -inf for a row outside [0, n_rows) or with
// live == 0; one wave per pair.
void fuse_check_args(int B, int ka, int kb, int mode, float alpha, int k_out, bool allow_full = false);
void launch_score_fuse(const float* score_a, const int64_t* rows_a, int ka, const float* score_b,
                       const int64_t* rows_b, int kb, const float* side_a, int B, int mode,
                       float alpha, float floor_a, float floor_b, float min_score, int k_out,
                       float* out_score, int64_t* out_rows, float* out_a, float* out_b,
                       hipStream_t s, const float* side_b = nullptr);
void launch_score_rows(const half_t* corpus, int ld, int64_t n_rows, const uint8_t* live,
                       const half_t* qn, const int64_t* rows, int B, int K, int64_t row_offset,
                       float* out, hipStream_t s);

// k_multivec.hip — MaxSim of (query, row) pairs over a multi-vector token pool (the function is
// stated in include/super_rag_mi355x.h): pool [n_tokens][dim] fp16, off [n_rows + 1], live [n_rows];
// q [B][ld_q][dim] fp16, q_len [B] (clamped to ld_q and 512), rows [B][K]; out [B][K], -inf for a row outside
// [0, n_rows), dead or empty and for an empty query.  tokens_hint: candidate tokens, profiling only.
// maxsim_check_args throws SR_ERR_INVALID outside the limits.  launch_mv_pack copies row i of src
// [n][ld_tok][dim] (off[i + 1] - off[i] tokens) to pool + off[i] * dim.
// dtype SR_DTYPE_FP8_E4M3: pool [n_tokens][dim] bytes e4m3(256 x), scored as the fp16 values d^ =
// e4m3_value / 256 (the query stays fp16); launch_mv_pack_fp8 is launch_mv_pack into such a pool.
void maxsim_check_args(int dim, int B, int ld_q, int K);
void launch_maxsim(const void* pool, int dtype, const int64_t* off, const uint8_t* live, int64_t n_rows,
                   int dim, const half_t* q, const int32_t* q_len, int B, int ld_q,
                   const int64_t* rows, int K, float* out, double tokens_hint, hipStream_t s);
// K9s (k_mvscan.hip, plan in sr_mv_plan.h): MaxSim of every query against the rows [row0, row1) of the
// pool (tokens [T0, T1)) into score [B][ld_s], column row - row0, bit for bit launch_maxsim's value of
// the pair; -inf for a row that is dead, empty or not allowed (allow [n_rows] bytes, may be null) and for
// an empty query.  launch_mv_topk folds the slab's scores into the running list run_keys [B][k] /
// run_n [B] (`first`: the list starts empty) and, on the `last` slab, writes out_score / out_rows [B][k]
// ordered (score desc, row asc), -inf / -1 past the eligible rows, row_offset added to the rows.
void launch_maxsim_scan(const void* pool, int dtype, const int64_t* off, const uint8_t* live,
                        const uint8_t* allow, int dim, const half_t* q, const int32_t* q_len, int B, int ld_q,
                        int64_t row0, int64_t row1, int64_t T0, int64_t T1, float* score, int64_t ld_s,
                        hipStream_t s);
void launch_mv_topk(const float* score, int64_t ld_s, int64_t row0, int64_t nrows, int B, int k, bool first,
                    bool last, uint64_t* run_keys, int* run_n, float* out_score, int64_t* out_rows,
                    int64_t row_offset, hipStream_t s);
void launch_mv_pack(const half_t* src, const int64_t* off, int64_t n, int ld_tok, int dim,
                    half_t* pool, hipStream_t s);
void launch_mv_pack_fp8(const half_t* src, const int64_t* off, int64_t n, int64_t ld_tok, int dim,
                        uint8_t* pool, hipStream_t s);
// compaction move: the kept tokens [t0, t1) of the compacted order from their old pool positions to
// dst + (t - dst_t0) * row_bytes; old_off / new_off [m] (+ new_off[m]): the kept rows' first tokens
// before and after (device), new_off[0] <= t0, t1 <= new_off[m].  Sources and [t0, t1) must not overlap
// when dst is the pool.
void launch_mv_move(const void* pool, void* dst, int64_t dst_t0, const int64_t* old_off,
                    const int64_t* new_off, int64_t m, int64_t t0, int64_t t1, int row_bytes,
                    hipStream_t s);

// k_lex.hip — reciprocal-rank fusion of two ranked row lists per query (-1 padded), fp64 scores.
void launch_rrf_fuse(const int64_t* rows_a, int ka, const int64_t* rows_b, int kb, int B,
                     int rank_const, double min_score, int k_out, double* out_score,
                     int64_t* out_rows, hipStream_t s);

}  // namespace sr
