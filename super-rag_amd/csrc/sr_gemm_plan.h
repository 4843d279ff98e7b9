// Launch decisions of the GEMM launchers (k_gemm.hip, launch_qkv_attention): which kernel family, whether
// persistent, grid, tile walk, profile name and booked flops / bytes.  Pure functions of scalars: no HIP
// call or header, plain host C++17, constexpr (gemm_pipe_kernel static_asserts its own constants against
// the predicates here; tests/native/gemm_plan_test.cpp pins every rule on the CPU).
#pragma once

#include <cstdint>

namespace sr {

enum Epilogue {
  EPI_BIAS_F16 = 0,       // y = acc + b                 -> fp16
  EPI_BIAS_GELU_F16 = 1,  // y = gelu_erf(acc + b)       -> fp16
  EPI_BIAS_RES_F32 = 2,   // y = acc + b + R (fp32)      -> fp32
  EPI_BIAS_TANH_F32 = 3,  // y = tanh(acc + b)           -> fp32 (classifier head)
  EPI_BIAS_RES_F16 = 4,   // y = acc + b + R (fp16)      -> fp16
  // LayerNorm folded into the GEMMs around it (fp16 residual stream; pipelined 256x256 kernels,
  // N % 256 == 0).  The A operand / residual is the UN-normalised row u with LN(u) =
  // (u - mu) * rstd * gamma + beta; mu / rstd come from per-row partial statistics written by the
  // producing GEMM's epilogue (LnFold, sr_kernels.h).
  EPI_LNF_F16 = 5,        // y = rstd * (acc - mu * c[n]) + b'[n], W' = W . diag(gamma) -> fp16
  EPI_LNF_GELU_F16 = 6,   // y = 2 gelu(same) (the FFN2 weight carries the 0.5)          -> fp16
  EPI_RES16_STATS = 7,    // y = acc + b + R (fp16, already normalised) -> fp16 + row statistics
  EPI_LNR16_STATS = 8,    // y = acc + b + LN(R) (R un-normalised)      -> fp16 + row statistics
  // K1 on the GEMM main loop (internal: launch_cosine_scan_gemm): W = corpus rows, X = queries,
  // epilogue = threshold filter appending (sim, row) keys to per-query candidate lists
  EPI_SCAN = 9,
  // the same on OCP fp8-e4m3 operands e4m3(256 x) of unit vectors (block-scaled MFMA
  // v_mfma_scale_f32_16x16x128_f8f6f4, E8M0 block scales 2^-8 undo the factor)
  EPI_SCAN8 = 10,
  // EPI_LNF_GELU_F16 storing OCP e4m3(2 GELU) bytes (the fp8 FFN1; its consumer runs fp8)
  EPI_LNF_GELU_F8 = 11,
  // EPI_RES16_STATS / EPI_LNR16_STATS that also store an e4m3 copy of their fp16 output to
  // LnFold.y8 (the next fp8 GEMM's A operand; separate codes keep the fp16 kernels' registers)
  EPI_RES16_STATS_Y8 = 12,
  EPI_LNR16_STATS_Y8 = 13
};
enum GemmVariant { GEMM_SMALL = 0, GEMM_BIG = 1, GEMM_PIPE = 4, GEMM_PIPE_PERSIST = 5,
                   GEMM_DIAG_NOLOAD = 6, GEMM_DIAG_NOEPI = 7 /* timing only */, GEMM_PP = 8,
                   GEMM_DIAG_P_NOEPI = 9, GEMM_DIAG_P_MATHONLY = 10, GEMM_DIAG_P_STOREONLY = 11 };

constexpr int GBK = 64;                  // k per stage (2-byte units)
constexpr int KCHUNK = 6;                // K-steps per chunk of the 128 x 128 kernel's chunked sums
constexpr int64_t kSplitMaxTiles = 128;  // split-K only below half a workgroup per CU slot pair

// One row per Epilogue code: what the launchers and kernels ask about an epilogue.
struct EpiTraits {
  bool valid;
  bool fold, lnf, gelu_fold, stats, lnr, y8, out32, scan;
  int out_bytes, res_bytes;  // per element: output 4 / 2 / 1, residual 4 / 2 / 0
  bool need_mr, need_colsum, need_gamma, need_stat_out, need_y8, need_stat_ld1;  // LnFold fields
  bool tile, pp, pipe, f8, k5c;  // families: 128 / 256 tile kernels, pp, pipe, fp8 operands, K5c
  const char* name_f16;  // profile names (null: the family does not carry it)
  const char* name_f8;
};
constexpr EpiTraits epi_traits(int epi) {
  constexpr bool T = true, F = false;
  switch (epi) {  //                    val fold lnf gelu stat lnr y8 o32 scan ob rb  mr col gam so  y8 ld1 tile pp pipe f8 k5c
    case EPI_BIAS_F16:       return {T, F, F, F, F, F, F, F, F, 2, 0, F, F, F, F, F, F, T, T, T, F, T, "gemm_f16_bias", nullptr};
    case EPI_BIAS_GELU_F16:  return {T, F, F, F, F, F, F, F, F, 2, 0, F, F, F, F, F, F, T, T, T, F, F, "gemm_f16_bias_gelu", nullptr};
    case EPI_BIAS_RES_F32:   return {T, F, F, F, F, F, F, T, F, 4, 4, F, F, F, F, F, F, T, T, T, F, F, "gemm_f16_bias_residual", nullptr};
    case EPI_BIAS_TANH_F32:  return {T, F, F, F, F, F, F, T, F, 4, 0, F, F, F, F, F, F, T, T, T, F, F, "gemm_f16_bias_tanh", nullptr};
    case EPI_BIAS_RES_F16:   return {T, F, F, F, F, F, F, F, F, 2, 2, F, F, F, F, F, F, T, T, T, F, F, "gemm_f16_bias_residual16", nullptr};
    case EPI_LNF_F16:        return {T, T, T, F, F, F, F, F, F, 2, 0, T, T, F, F, F, F, F, T, T, T, T, "gemm_f16_lnfold", "gemm_f8_lnfold"};
    case EPI_LNF_GELU_F16:   return {T, T, T, T, F, F, F, F, F, 2, 0, T, T, F, F, F, T, F, T, T, F, F, "gemm_f16_lnfold_gelu", nullptr};
    case EPI_RES16_STATS:    return {T, T, F, F, T, F, F, F, F, 2, 2, F, F, F, T, F, F, F, T, T, T, F, "gemm_f16_residual16_stats", "gemm_f8_residual16_stats"};
    case EPI_LNR16_STATS:    return {T, T, F, F, T, T, F, F, F, 2, 2, T, F, T, T, F, F, F, T, T, T, F, "gemm_f16_lnres16_stats", "gemm_f8_lnres16_stats"};
    case EPI_SCAN:           return {T, F, F, F, F, F, F, F, T, 0, 0, F, F, F, F, F, F, F, F, F, F, F, "cosine_scan", nullptr};
    case EPI_SCAN8:          return {T, F, F, F, F, F, F, F, T, 0, 0, F, F, F, F, F, F, F, F, F, F, F, nullptr, "cosine_scan8"};
    case EPI_LNF_GELU_F8:    return {T, T, T, T, F, F, F, F, F, 1, 0, T, T, F, F, F, T, F, F, T, T, F, "gemm_f16_lnfold_gelu_out8", "gemm_f8_lnfold_gelu_out8"};
    case EPI_RES16_STATS_Y8: return {T, T, F, F, T, F, T, F, F, 2, 2, F, F, F, T, T, F, F, F, T, T, F, "gemm_f16_residual16_stats_y8", "gemm_f8_residual16_stats_y8"};
    case EPI_LNR16_STATS_Y8: return {T, T, F, F, T, T, T, F, F, 2, 2, T, F, T, T, T, F, F, F, T, T, F, "gemm_f16_lnres16_stats_y8", "gemm_f8_lnres16_stats_y8"};
    default:                 return {F, F, F, F, F, F, F, F, F, 0, 0, F, F, F, F, F, F, F, F, F, F, F, nullptr, nullptr};
  }
}

constexpr int64_t plan_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Persistent kernels: 8 XCD groups x G walkers (one 8-wave workgroup per CU), G <= walkers.  The
// kernels' XCD split needs a multiple of 8, >= 8 (gemm_pipe_kernel: "grid = 8 x G"): true by construction.
constexpr unsigned walker_grid(int64_t tiles, int64_t walkers = 32) {
  const int64_t g = plan_ceil_div(tiles, 8);
  return (unsigned)(8 * (g < walkers ? g : walkers));
}
static_assert(walker_grid(1) == 8 && walker_grid(2049) == 256 && walker_grid(1ll << 40) == 256, "8 x G, G >= 1");
constexpr unsigned scan_grid(int64_t rows) { return walker_grid(plan_ceil_div(rows, 256)); }
// The product tile walk: short-K GEMMs (K <= 1024: QKV, FFN1, O-proj) walk groups of 8 (N >= 2048) or 4
// m-panels; FFN2 (K = 3072) stays n fastest.  Same-box A/B of the full bench: 422.8 / 424.0 -> 429.8 /
// 431.0 q/s (profiles/r01_gemm_group_m.log).
constexpr int product_group_m(int N, int K) { return K <= 1024 ? (N >= 2048 ? 8 : 4) : 0; }
// De-phasing of the persistent walkers (SR_GEMM_STAGGER = env, units of 512 cycles per phase at K = 768;
// 0 = off): phase step ~1/16 of a tile (K / 96 x 512 cycles), never rounded to "off".
constexpr int stagger_phase(int env, int K) {
  const int s = env * K / 768;
  return env > 0 ? (s > 1 ? s : 1) : env < 0 ? (s < -1 ? s : -1) : 0;
}
// K5c head groups of the tile walk (hg | heads): an XCD's ~32 concurrent tiles need ~32 / hg X panels
// (256 x d fp16) and hg W slices (192 x d fp16) in its 4 MiB L2: the divisor of heads that minimises
// 32 * 256 / hg + 192 hg, the larger on a tie (hg = 6 of 12 heads: 1,011 -> 1,033 TF/s and +0.9 % end to
// end against hg = heads; hg = 4 -5 %, profiles/r05_k5c_hgroup/)
constexpr int qkv_head_group(int heads) {
  int hg = heads;
  for (int v = 1; v <= heads; ++v)
    if (heads % v == 0 && 8192.0 / v + 192.0 * v <= 8192.0 / hg + 192.0 * hg) hg = v;
  return hg;
}
constexpr int64_t qkv_tiles(int64_t M, int heads) { return plan_ceil_div(M, 256) * heads; }
// Split-K of the 128 x 128 kernel over its K chunks when the tiles alone leave the CUs idle and the
// caller lent a workspace for the partial tiles (64 KiB per tile and chunk; ws_bytes 0: none): chunk
// groups of cpg chunks, about 512 workgroups in all.  cpg 0: no split.
struct SplitK { int64_t cpg, groups; };
constexpr SplitK split_k(int64_t nchunk, int64_t tiles, int64_t ws_bytes) {
  if (nchunk < 2 || tiles > kSplitMaxTiles || ws_bytes <= 0 || nchunk * tiles * 65536 > ws_bytes) return {0, 1};
  const int64_t want = plan_ceil_div(512, tiles);
  const int64_t cpg = plan_ceil_div(nchunk, nchunk < want ? nchunk : want);
  return {cpg, plan_ceil_div(nchunk, cpg)};
}

// The host images of two gemm_pipe_kernel constants (static_asserted there):
// CSTL: the FFN1 epilogues stage their constants during K-step 3 of a persistent tile.
constexpr int persist_min_ksteps(int epi) { return epi_traits(epi).gelu_fold ? 4 : 2; }
// RHALF: the persistent EPI_LNR16_STATS on fp16 operands stages CONSECUTIVE row statistics, so it runs
// only at stat_ld 1.  As the code stands, neither the _Y8 form (it stays persistent at stat_ld != 1)
// nor the fp8-operand kernels (launch_gemm_f8w never had a stat_ld clause) take that epilogue.
constexpr bool persist_stages_row_stats(int epi, bool f8_operands) { return epi == EPI_LNR16_STATS && !f8_operands; }

struct GemmAsk {
  bool f8 = false;          // fp8 operands (launch_gemm_f8w: K, lda in bytes); else launch_gemm_variant
  bool diag_build = false;  // SR_WITH_DIAG
  int variant = -1;         // requested GemmVariant, or -1 (fp16 operands only)
  int forced_tile = -1;     // gemm_force_tile / SR_GEMM_TILE, or -1
  int epi = 0, M = 0, N = 0, K = 0;
  int64_t lda = 0, ldr = 0, ldy = 0;
  // the LnFold fields the rules read (has_lf false: the caller passed none)
  bool has_lf = false, mr = false, colsum = false, gamma = false, stat_out = false, y8 = false, wexp = false;
  int64_t stat_ld = 1;
  int x_k = 0;              // LnFold.x_k
  int64_t ws_bytes = -1;    // split-K workspace: -1 none, else LnFold.chunk_ws_bytes
  int group_m = 0, stagger = 0;  // fp8 operands: as the caller passed them (LnFold)
  bool group_m_override = false; // fp16 operands: SR_GEMM_GROUP_M matched this N ...
  int group_m_env = 0;           // ... with this value
  int stagger_env = 0;           // fp16 operands: SR_GEMM_STAGGER
};
enum GemmFamily { FAM_TILE128, FAM_TILE256, FAM_PP, FAM_PIPE, FAM_PIPE_DIAG };
struct GemmPlan {
  const char* error = nullptr;  // the failed check's message: only name, flops and bytes are then set (the
                                // launcher books the rejected call in the profile table before it throws)
  int family = FAM_TILE128, variant = GEMM_SMALL;  // variant: as resolved (FAM_PIPE_DIAG picks its kernel by it)
  bool persist = false;
  unsigned grid_x = 0, grid_y = 1, block = 0;
  int group_m = 0, stagger = 0, x_k = 0;  // LnFold fields of the launch (x_k 0: plain K)
  int kxs = 0, cpg = 0, kchunk = 0;       // tile kernels: K-steps of X, chunks per group, chunk length
  const char* name = nullptr;
  double flops = 0.0, bytes = 0.0;
};
constexpr GemmPlan plan_reject(GemmPlan p, const char* msg) {
  p.error = msg;
  return p;
}

// The launchers' argument checks (they run before the M <= 0 return): null, or the failed check's message.
constexpr const char* check_gemm_args(const GemmAsk& a) {
  const EpiTraits t = epi_traits(a.epi);
  if (a.f8) {
    if (!t.f8) return "gemm_f8w: unsupported epilogue";
    if (!(a.K % 128 == 0 && a.K >= 256)) return "gemm_f8w: K must be a multiple of 128, >= 256";
    if (a.N % 256 != 0) return "gemm_f8w: N must be a multiple of 256";
    if (!(a.lda % 16 == 0 && a.ldy % 8 == 0 && a.ldr % 8 == 0)) return "gemm_f8w: 16-byte rows";
    if (!(a.has_lf && a.wexp)) return "gemm_f8w: the weight rows' exponents (LnFold.wexp)";
  } else {
    if (a.K % GBK != 0) return "gemm: K must be a multiple of 64";
    if (a.N % 128 != 0) return "gemm: N must be a multiple of 128";
    if (!(a.lda % 8 == 0 && a.ldy % 4 == 0)) return "gemm: leading dimensions must keep 16-byte rows";
    if (!t.valid || t.scan) return "gemm: unknown epilogue";
    if (t.need_y8 && !(a.has_lf && a.y8)) return "gemm: the e4m3-copy epilogues need LnFold.y8";  // (first here)
    if (t.fold && !(a.has_lf && a.N % 256 == 0)) return "gemm: LayerNorm-folded epilogues need LnFold, N % 256";
  }
  if (t.need_mr && !a.mr) return a.f8 ? "gemm_f8w: LN-folded operand needs its row statistics" : "gemm: LN-folded operand needs its row statistics";
  if (t.need_colsum && !a.colsum) return a.f8 ? "gemm_f8w: LNF needs colsum" : "gemm: LNF needs colsum";
  if (t.need_stat_ld1 && a.stat_ld != 1)
    return a.f8 ? "gemm_f8w: FFN1 reads consecutive row statistics" : "gemm: the FFN1 epilogues read consecutive row statistics (stat_ld 1)";
  if (t.need_gamma && !a.gamma) return a.f8 ? "gemm_f8w: LNR needs the LayerNorm weight" : "gemm: LNR needs the LayerNorm weight";
  if (t.need_stat_out && !a.stat_out) return a.f8 ? "gemm_f8w: stat_out" : "gemm: *_STATS epilogue needs stat_out";
  if (t.need_y8 && !a.y8) return "gemm_f8w: the e4m3-copy epilogues need LnFold.y8";  // (fp16 operands: checked above)
  const int x_k = a.x_k > 0 ? a.x_k : a.K;  // (split weights: fp16 operands and outputs, the pp epilogues)
  if (!a.f8 && !(x_k == a.K || (a.K == 2 * x_k && x_k % GBK == 0 && t.pp)))
    return "gemm: split weights need K == 2 x_k (x_k % 64 == 0, fp16 operands)";
  return nullptr;
}

// The launch of a checked GEMM with M > 0.  Every rule in the order the launchers applied them.
constexpr GemmPlan plan_gemm(const GemmAsk& a) {
  const EpiTraits t = epi_traits(a.epi);
  const int M = a.M, N = a.N, K = a.K;
  GemmPlan p;
  p.flops = 2.0 * M * (double)N * K;
  p.block = 512;
  const int64_t big_tiles = (N % 256 == 0) ? (int64_t)(N / 256) * plan_ceil_div(M, 256) : 0;
  if (a.f8) {
    // fp8 operands: always the pipe kernels, on K / 2 two-byte units.  group_m / stagger stay as the caller
    // passed them (today's callers pass 0: the fp8 GEMMs walk n fastest, the fp16 ones grouped), and the
    // bytes count the e4m3 copy, which the fp16 launcher's do not.
    p.name = t.name_f8;
    p.bytes = (double)M * K + (double)N * K + (double)(t.out_bytes + t.res_bytes + (t.y8 ? 1 : 0)) * (double)M * N;
    p.family = FAM_PIPE;
    p.persist = big_tiles >= 512 && K / 2 / GBK >= persist_min_ksteps(a.epi) &&
                !(persist_stages_row_stats(a.epi, true) && a.stat_ld != 1);
    p.variant = p.persist ? GEMM_PIPE_PERSIST : GEMM_PIPE;
    p.grid_x = p.persist ? walker_grid(big_tiles) : (unsigned)big_tiles;
    p.group_m = a.group_m;
    p.stagger = a.stagger;
    return p;
  }
  const int x_k = a.x_k > 0 ? a.x_k : K;
  p.name = t.name_f16;
  p.bytes = 2.0 * ((double)M * x_k + (double)N * K) + (double)(t.out_bytes + t.res_bytes) * (double)M * N;
  if (big_tiles >= (1ll << 31)) return plan_reject(p, "gemm: too many tiles");
  int v = a.variant >= 0 ? a.variant : a.forced_tile;
  if (v < 0) v = big_tiles >= 512 ? GEMM_PIPE_PERSIST : GEMM_SMALL;
  if (v != GEMM_SMALL && N % 256 != 0) v = GEMM_SMALL;
  if (v == GEMM_PP && (K % 32 != 0 || !t.pp || x_k != K)) v = GEMM_PIPE;
  if (x_k != K && v >= GEMM_DIAG_NOLOAD && v != GEMM_PP) v = GEMM_PIPE;  // diagnostics: plain K
  const bool timing = v == GEMM_DIAG_NOLOAD || v == GEMM_DIAG_NOEPI || (v >= GEMM_DIAG_P_NOEPI && v <= GEMM_DIAG_P_STOREONLY);
  if (timing && !a.diag_build) return plan_reject(p, "gemm: timing-only variants are in the diagnostic library (libsrmi_diag.so)");
  if (t.fold && (v == GEMM_SMALL || v == GEMM_BIG)) v = big_tiles >= 512 ? GEMM_PIPE_PERSIST : GEMM_PIPE;
  const bool wide = (v == GEMM_PIPE || v == GEMM_PIPE_PERSIST || v == GEMM_PP) && !t.out32;
  if (wide && !(a.ldy % 8 == 0 && a.ldr % 8 == 0)) return plan_reject(p, "gemm: fp16 outputs need ldy, ldr % 8 == 0");
  if (!t.pp && !(v == GEMM_PIPE || v == GEMM_PIPE_PERSIST)) return plan_reject(p, "gemm: the e4m3-output epilogues run on the pipelined kernels");
  p.group_m = a.group_m_override ? a.group_m_env : product_group_m(N, K);
  p.x_k = x_k == K ? 0 : x_k;
  p.stagger = stagger_phase(a.stagger_env, K);
  p.variant = v;
  p.kxs = x_k / GBK;
  if (v == GEMM_BIG) {
    p.family = FAM_TILE256;
    p.grid_x = (unsigned)big_tiles;
  } else if (timing) {  // (always EPI_BIAS_F16 kernels: timing only)
    p.family = FAM_PIPE_DIAG;
    p.persist = v >= GEMM_DIAG_P_NOEPI;
    p.grid_x = p.persist ? walker_grid(big_tiles) : (unsigned)big_tiles;
  } else if (v == GEMM_PP) {
    p.family = FAM_PP;
    p.grid_x = (unsigned)((int64_t)(N / 256) * plan_ceil_div(M, 128));
    p.block = 256;
  } else if (v == GEMM_PIPE || v == GEMM_PIPE_PERSIST) {
    p.family = FAM_PIPE;
    p.persist = v == GEMM_PIPE_PERSIST && K / GBK >= persist_min_ksteps(a.epi) &&
                !(persist_stages_row_stats(a.epi, false) && a.stat_ld != 1);
    p.grid_x = p.persist ? walker_grid(big_tiles) : (unsigned)big_tiles;
  } else {
    const int64_t tiles = (int64_t)(N / 128) * plan_ceil_div(M, 128);
    if (tiles >= (1ll << 31)) return plan_reject(p, "gemm: too many tiles");
    // (chunked sums only for the callers that lent a workspace: the same chunks split or not)
    const SplitK s = split_k(plan_ceil_div(K / GBK, KCHUNK), tiles, a.ws_bytes);
    p.family = FAM_TILE128;
    p.grid_x = (unsigned)tiles;
    p.grid_y = (unsigned)s.groups;
    p.block = 256;
    p.cpg = (int)s.cpg;
    p.kchunk = a.ws_bytes >= 0 ? KCHUNK : 0;
  }
  return p;
}

}  // namespace sr
