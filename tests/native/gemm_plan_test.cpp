// Host test of csrc/sr_gemm_plan.h (tests/test_gemm_plan.py builds it with AddressSanitizer + UBSan and
// runs it; no GPU, no HIP).  Every expected value is a literal read off the launchers as they were before
// the plan header existed (product build, no environment overrides unless a case says so); nothing here
// is computed by the functions under test.  Prints "gemm_plan_test: N checks, 0 failures" and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "sr_gemm_plan.h"

namespace {

using namespace sr;

int g_failures = 0;
int g_checks = 0;

#define EXPECT(cond)                                             \
  do {                                                           \
    ++g_checks;                                                  \
    if (!(cond)) {                                               \
      ++g_failures;                                              \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                            \
  } while (0)

bool same(const char* a, const char* b) { return (!a && !b) || (a && b && std::strcmp(a, b) == 0); }

// fp16 operands, 16-byte rows, every LnFold field present, stat_ld 1, no workspace
GemmAsk ask(int epi, int M, int N, int K, int variant = -1) {
  GemmAsk a;
  a.variant = variant;
  a.epi = epi, a.M = M, a.N = N, a.K = K;
  a.lda = K, a.ldr = N, a.ldy = N;
  a.has_lf = a.mr = a.colsum = a.gamma = a.stat_out = a.y8 = a.wexp = true;
  return a;
}
GemmAsk ask8(int epi, int M, int N, int K) {
  GemmAsk a = ask(epi, M, N, K);
  a.f8 = true;
  return a;
}
GemmPlan plan(const GemmAsk& a) {
  EXPECT(check_gemm_args(a) == nullptr);
  const GemmPlan p = plan_gemm(a);
  EXPECT(p.error == nullptr);
  return p;
}

struct Row {  // the literal traits table
  int epi;
  bool fold, lnf, gelu_fold, stats, lnr, y8, out32, scan;
  int out_bytes, res_bytes;
  bool mr, colsum, gamma, stat_out, need_y8, stat_ld1;
  bool tile, pp, pipe, f8, k5c;
  const char *f16, *f8name;
};
const Row kRows[] = {
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 1, "gemm_f16_bias", nullptr},
    {1, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, "gemm_f16_bias_gelu", nullptr},
    {2, 0, 0, 0, 0, 0, 0, 1, 0, 4, 4, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, "gemm_f16_bias_residual", nullptr},
    {3, 0, 0, 0, 0, 0, 0, 1, 0, 4, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, "gemm_f16_bias_tanh", nullptr},
    {4, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, "gemm_f16_bias_residual16", nullptr},
    {5, 1, 1, 0, 0, 0, 0, 0, 0, 2, 0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, "gemm_f16_lnfold", "gemm_f8_lnfold"},
    {6, 1, 1, 1, 0, 0, 0, 0, 0, 2, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 0, 0, "gemm_f16_lnfold_gelu", nullptr},
    {7, 1, 0, 0, 1, 0, 0, 0, 0, 2, 2, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 0, "gemm_f16_residual16_stats",
     "gemm_f8_residual16_stats"},
    {8, 1, 0, 0, 1, 1, 0, 0, 0, 2, 2, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 0, "gemm_f16_lnres16_stats",
     "gemm_f8_lnres16_stats"},
    {9, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, "cosine_scan", nullptr},
    {10, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, nullptr, "cosine_scan8"},
    {11, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 0, 1, 1, 0, "gemm_f16_lnfold_gelu_out8",
     "gemm_f8_lnfold_gelu_out8"},
    {12, 1, 0, 0, 1, 0, 1, 0, 0, 2, 2, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 0, "gemm_f16_residual16_stats_y8",
     "gemm_f8_residual16_stats_y8"},
    {13, 1, 0, 0, 1, 1, 1, 0, 0, 2, 2, 1, 0, 1, 1, 1, 0, 0, 0, 1, 1, 0, "gemm_f16_lnres16_stats_y8",
     "gemm_f8_lnres16_stats_y8"},
};

void test_traits() {
  for (const Row& r : kRows) {
    const EpiTraits t = epi_traits(r.epi);
    EXPECT(t.valid);
    EXPECT(t.fold == r.fold && t.lnf == r.lnf && t.gelu_fold == r.gelu_fold && t.stats == r.stats);
    EXPECT(t.lnr == r.lnr && t.y8 == r.y8 && t.out32 == r.out32 && t.scan == r.scan);
    EXPECT(t.out_bytes == r.out_bytes && t.res_bytes == r.res_bytes);
    EXPECT(t.need_mr == r.mr && t.need_colsum == r.colsum && t.need_gamma == r.gamma);
    EXPECT(t.need_stat_out == r.stat_out && t.need_y8 == r.need_y8 && t.need_stat_ld1 == r.stat_ld1);
    EXPECT(t.tile == r.tile && t.pp == r.pp && t.pipe == r.pipe && t.f8 == r.f8 && t.k5c == r.k5c);
    EXPECT(same(t.name_f16, r.f16));
    EXPECT(same(t.name_f8, r.f8name));
  }
  EXPECT(!epi_traits(-1).valid && !epi_traits(14).valid);
  static_assert(epi_traits(EPI_LNR16_STATS_Y8).y8 && !epi_traits(EPI_LNR16_STATS).y8, "usable in constexpr");
  static_assert(EPI_BIAS_TANH_F32 == 3 && EPI_BIAS_RES_F16 == 4 && EPI_SCAN == 9 && EPI_LNR16_STATS_Y8 == 13, "");
  static_assert(GEMM_SMALL == 0 && GEMM_BIG == 1 && GEMM_PIPE == 4 && GEMM_PIPE_PERSIST == 5 && GEMM_PP == 8, "");
  static_assert(GBK == 64 && KCHUNK == 6 && kSplitMaxTiles == 128, "");
}

void test_small_rules() {
  // scan: rows -> grid
  EXPECT(scan_grid(300) == 8 && scan_grid(2048) == 8 && scan_grid(2049) == 16);
  EXPECT(scan_grid(65536) == 256 && scan_grid(1000000) == 256);
  EXPECT(walker_grid(100, 4) == 32 && walker_grid(9, 4) == 16);  // the FFN1 diagnostic's walkers
  // K5c
  EXPECT(qkv_head_group(1) == 1 && qkv_head_group(4) == 4 && qkv_head_group(8) == 8);
  EXPECT(qkv_head_group(12) == 6 && qkv_head_group(16) == 8);
  EXPECT(walker_grid(qkv_tiles(2 * 128, 12)) == 16);
  // stagger
  EXPECT(stagger_phase(0, 768) == 0 && stagger_phase(2, 768) == 2 && stagger_phase(2, 3072) == 8);
  EXPECT(stagger_phase(1, 64) == 1 && stagger_phase(-1, 64) == -1);
  // the product walk
  EXPECT(product_group_m(3072, 768) == 8 && product_group_m(768, 768) == 4 && product_group_m(768, 1024) == 4);
  EXPECT(product_group_m(768, 3072) == 0 && product_group_m(2048, 1024) == 8);
  // split-K
  EXPECT(split_k(8, 6, 3145728).cpg == 1 && split_k(8, 6, 3145728).groups == 8);
  EXPECT(split_k(8, 6, 3145727).cpg == 0 && split_k(8, 6, 3145727).groups == 1);
  EXPECT(split_k(1, 6, 1 << 30).cpg == 0 && split_k(8, 129, 1ll << 40).cpg == 0 && split_k(8, 6, 0).cpg == 0);
  // the kernels' constants
  EXPECT(persist_min_ksteps(6) == 4 && persist_min_ksteps(11) == 4 && persist_min_ksteps(0) == 2);
  EXPECT(persist_min_ksteps(8) == 2 && persist_min_ksteps(13) == 2);
  EXPECT(persist_stages_row_stats(8, false) && !persist_stages_row_stats(8, true));
  EXPECT(!persist_stages_row_stats(13, false) && !persist_stages_row_stats(7, false));
}

void test_fp16_plans() {
  {  // small tiles
    const GemmPlan p = plan(ask(EPI_BIAS_F16, 64, 768, 768));
    EXPECT(p.family == FAM_TILE128 && p.grid_x == 6 && p.grid_y == 1 && p.block == 256);
    EXPECT(p.cpg == 0 && p.kchunk == 0 && p.kxs == 12 && !p.persist);
    EXPECT(same(p.name, "gemm_f16_bias"));
    EXPECT(p.bytes == 2.0 * (64.0 * 768 + 768.0 * 768) + 2.0 * 64 * 768);
    EXPECT(p.flops == 2.0 * 64 * 768 * 768);
  }
  {  // split-K
    GemmAsk a = ask(EPI_BIAS_F16, 64, 768, 3072);
    a.ws_bytes = 3145728;
    GemmPlan p = plan(a);
    EXPECT(p.grid_x == 6 && p.grid_y == 8 && p.cpg == 1 && p.kchunk == 6);
    a.ws_bytes = 3145727;
    p = plan(a);
    EXPECT(p.grid_x == 6 && p.grid_y == 1 && p.cpg == 0 && p.kchunk == 6);
    a = ask(EPI_BIAS_F16, 2048, 1024, 3072);
    a.ws_bytes = 64ll << 20;
    p = plan(a);
    EXPECT(p.grid_x == 128 && p.grid_y == 4 && p.cpg == 2);
    a.M = 2049;  // 136 tiles
    p = plan(a);
    EXPECT(p.grid_x == 136 && p.grid_y == 1 && p.cpg == 0 && p.kchunk == 6);
  }
  {  // the automatic threshold: 511 / 512 big tiles
    GemmPlan p = plan(ask(EPI_BIAS_F16, 130816, 256, 128));
    EXPECT(p.family == FAM_TILE128 && p.grid_x == 2044 && p.grid_y == 1 && !p.persist);
    p = plan(ask(EPI_BIAS_F16, 130817, 256, 128));
    EXPECT(p.family == FAM_PIPE && p.persist && p.grid_x == 256 && p.block == 512);
  }
  {  // FFN1
    GemmPlan p = plan(ask(EPI_LNF_GELU_F16, 131072, 3072, 768));
    EXPECT(p.family == FAM_PIPE && p.persist && p.grid_x == 256 && p.group_m == 8 && p.stagger == 0 && p.x_k == 0);
    p = plan(ask(EPI_LNF_GELU_F16, 131072, 3072, 192, GEMM_PIPE_PERSIST));
    EXPECT(p.family == FAM_PIPE && !p.persist && p.grid_x == 6144);
    p = plan(ask(EPI_LNF_GELU_F16, 131072, 3072, 256, GEMM_PIPE_PERSIST));
    EXPECT(p.persist && p.grid_x == 256);
    p = plan(ask(EPI_LNF_GELU_F8, 131072, 3072, 192, GEMM_PIPE_PERSIST));  // (fp16 operands, e4m3 output)
    EXPECT(!p.persist && same(p.name, "gemm_f16_lnfold_gelu_out8"));
  }
  {  // a fold epilogue at short M leaves the tile kernels
    const GemmPlan p = plan(ask(EPI_LNF_F16, 64, 768, 768));
    EXPECT(p.family == FAM_PIPE && !p.persist && p.grid_x == 3 && p.block == 512 && p.group_m == 4);
    const GemmPlan q = plan(ask(EPI_LNF_F16, 64, 768, 768, GEMM_BIG));
    EXPECT(q.family == FAM_PIPE && !q.persist && q.grid_x == 3);
  }
  {  // FFN2 / O-projection
    GemmAsk a = ask(EPI_LNR16_STATS, 131072, 768, 3072);
    GemmPlan p = plan(a);
    EXPECT(p.family == FAM_PIPE && p.persist && p.grid_x == 256 && p.group_m == 0);
    EXPECT(p.bytes == 2.0 * (131072.0 * 3072 + 768.0 * 3072) + 4.0 * 131072 * 768);
    a.stat_ld = 128;
    p = plan(a);
    EXPECT(!p.persist && p.grid_x == 1536);
    a.epi = EPI_LNR16_STATS_Y8;  // as the code stands: stays persistent, and books no byte for the copy
    p = plan(a);
    EXPECT(p.persist && p.grid_x == 256);
    EXPECT(p.bytes == 2.0 * (131072.0 * 3072 + 768.0 * 3072) + 4.0 * 131072 * 768);
  }
  {  // the K-step floor of the persistent kernels
    GemmPlan p = plan(ask(EPI_BIAS_F16, 300, 256, 64, GEMM_PIPE_PERSIST));
    EXPECT(p.family == FAM_PIPE && !p.persist && p.grid_x == 2);
    p = plan(ask(EPI_BIAS_F16, 300, 256, 128, GEMM_PIPE_PERSIST));
    EXPECT(p.persist && p.grid_x == 8);
  }
  {  // fallbacks
    GemmPlan p = plan(ask(EPI_BIAS_F16, 300, 640, 128, GEMM_PIPE));
    EXPECT(p.family == FAM_TILE128 && p.grid_x == 15);
    p = plan(ask(EPI_BIAS_F16, 300, 256, 128, GEMM_PP));
    EXPECT(p.family == FAM_PP && p.grid_x == 3 && p.block == 256);
    p = plan(ask(EPI_RES16_STATS_Y8, 300, 256, 128, GEMM_PP));
    EXPECT(p.family == FAM_PIPE && !p.persist);
    GemmAsk a = ask(EPI_BIAS_F16, 300, 256, 256, GEMM_PP);
    a.x_k = 128;
    a.lda = 128;
    p = plan(a);
    EXPECT(p.family == FAM_PIPE && p.x_k == 128 && p.kxs == 2);
    EXPECT(p.bytes == 2.0 * (300.0 * 128 + 256.0 * 256) + 2.0 * 300 * 256);
    a = ask(EPI_BIAS_F16, 300, 256, 128, GEMM_BIG);
    p = plan(a);
    EXPECT(p.family == FAM_TILE256 && p.grid_x == 2 && p.block == 512 && p.cpg == 0 && p.kchunk == 0);
    for (int v : {GEMM_DIAG_NOLOAD, GEMM_DIAG_NOEPI, GEMM_DIAG_P_NOEPI, GEMM_DIAG_P_MATHONLY, GEMM_DIAG_P_STOREONLY}) {
      a = ask(EPI_BIAS_F16, 300, 256, 128, v);
      EXPECT(check_gemm_args(a) == nullptr);
      EXPECT(same(plan_gemm(a).error, "gemm: timing-only variants are in the diagnostic library (libsrmi_diag.so)"));
      a.diag_build = true;
      p = plan_gemm(a);
      EXPECT(p.error == nullptr && p.family == FAM_PIPE_DIAG && p.grid_x == (v >= GEMM_DIAG_P_NOEPI ? 8u : 2u));
    }
    a = ask(EPI_BIAS_F16, 300, 256, 128, GEMM_PIPE);
    a.ldy = 260;
    EXPECT(check_gemm_args(a) == nullptr);
    EXPECT(same(plan_gemm(a).error, "gemm: fp16 outputs need ldy, ldr % 8 == 0"));
    a.variant = GEMM_SMALL;
    EXPECT(plan_gemm(a).error == nullptr && plan_gemm(a).family == FAM_TILE128);
    a = ask(EPI_BIAS_RES_F32, 300, 256, 128, GEMM_PIPE);
    a.ldy = 260;
    EXPECT(plan_gemm(a).error == nullptr && plan_gemm(a).family == FAM_PIPE);
    a = ask(EPI_BIAS_F16, 300, 256, 128);
    a.forced_tile = GEMM_PIPE;  // SR_GEMM_TILE / gemm_force_tile, only without a requested variant
    EXPECT(plan_gemm(a).family == FAM_PIPE);
    a.variant = GEMM_SMALL;
    EXPECT(plan_gemm(a).family == FAM_TILE128);
  }
  {  // environment overrides
    GemmAsk a = ask(EPI_LNF_GELU_F16, 131072, 3072, 768);
    a.group_m_override = true;
    a.group_m_env = 2;
    a.stagger_env = 2;
    const GemmPlan p = plan(a);
    EXPECT(p.group_m == 2 && p.stagger == 2);
  }
  {  // argument checks
    GemmAsk a = ask(EPI_SCAN, 64, 256, 128);
    EXPECT(same(check_gemm_args(a), "gemm: unknown epilogue"));
    a.epi = 14;
    EXPECT(same(check_gemm_args(a), "gemm: unknown epilogue"));
    a = ask(EPI_LNF_F16, 64, 256, 128);
    a.has_lf = a.mr = a.colsum = false;
    EXPECT(same(check_gemm_args(a), "gemm: LayerNorm-folded epilogues need LnFold, N % 256"));
    a = ask(EPI_LNF_GELU_F16, 64, 256, 128);
    a.stat_ld = 2;
    EXPECT(same(check_gemm_args(a), "gemm: the FFN1 epilogues read consecutive row statistics (stat_ld 1)"));
    a = ask(EPI_LNR16_STATS_Y8, 64, 256, 128);
    a.y8 = false;
    EXPECT(same(check_gemm_args(a), "gemm: the e4m3-copy epilogues need LnFold.y8"));
    a = ask(EPI_LNR16_STATS_Y8, 64, 256, 128);  // no LnFold at all: the y8 check comes before the fold check
    a.has_lf = a.mr = a.colsum = a.gamma = a.stat_out = a.y8 = a.wexp = false;
    EXPECT(same(check_gemm_args(a), "gemm: the e4m3-copy epilogues need LnFold.y8"));
    a = ask(EPI_BIAS_F16, 300, 256, 128, GEMM_PIPE);  // a rejected plan still carries what the launcher books
    a.ldy = 260;
    EXPECT(same(plan_gemm(a).name, "gemm_f16_bias") && plan_gemm(a).flops == 2.0 * 300 * 256 * 128);
    EXPECT(plan_gemm(a).bytes == 2.0 * (300.0 * 128 + 256.0 * 128) + 2.0 * 300 * 256);
    a = ask(EPI_RES16_STATS_Y8, 64, 256, 256);
    a.x_k = 128;
    EXPECT(same(check_gemm_args(a), "gemm: split weights need K == 2 x_k (x_k % 64 == 0, fp16 operands)"));
    a = ask(EPI_BIAS_F16, 64, 256, 96);
    EXPECT(same(check_gemm_args(a), "gemm: K must be a multiple of 64"));
  }
}

void test_fp8_plans() {
  GemmPlan p = plan(ask8(EPI_LNF_GELU_F8, 131072, 3072, 768));
  EXPECT(p.family == FAM_PIPE && p.persist && p.grid_x == 256 && p.block == 512 && p.group_m == 0 && p.stagger == 0);
  EXPECT(same(p.name, "gemm_f8_lnfold_gelu_out8"));
  EXPECT(p.bytes == 131072.0 * 768 + 3072.0 * 768 + 131072.0 * 3072);
  p = plan(ask8(EPI_LNF_GELU_F8, 131072, 3072, 256));
  EXPECT(!p.persist && p.grid_x == 6144);
  p = plan(ask8(EPI_RES16_STATS_Y8, 300, 256, 256));
  EXPECT(same(p.name, "gemm_f8_residual16_stats_y8") && !p.persist && p.grid_x == 2);
  EXPECT(p.bytes == 300.0 * 256 + 256.0 * 256 + 5.0 * 300 * 256);
  GemmAsk a = ask8(EPI_LNR16_STATS, 131072, 768, 3072);
  a.stat_ld = 128;  // as the code stands: no stat_ld clause on fp8 operands
  a.group_m = 3;
  a.stagger = -2;   // as the caller passed them
  p = plan(a);
  EXPECT(p.persist && p.grid_x == 256 && p.group_m == 3 && p.stagger == -2);
  for (int epi = -1; epi <= 14; ++epi) {
    const bool ok = epi == 5 || epi == 7 || epi == 8 || epi == 11 || epi == 12 || epi == 13;
    EXPECT(same(check_gemm_args(ask8(epi, 64, 256, 256)), ok ? nullptr : "gemm_f8w: unsupported epilogue"));
  }
  a = ask8(EPI_LNF_F16, 64, 256, 128);
  EXPECT(same(check_gemm_args(a), "gemm_f8w: K must be a multiple of 128, >= 256"));
  a = ask8(EPI_LNF_GELU_F8, 64, 256, 256);
  a.stat_ld = 2;
  EXPECT(same(check_gemm_args(a), "gemm_f8w: FFN1 reads consecutive row statistics"));
  a = ask8(EPI_RES16_STATS, 64, 256, 256);
  a.stat_out = false;
  EXPECT(same(check_gemm_args(a), "gemm_f8w: stat_out"));
  a = ask8(EPI_RES16_STATS, 64, 256, 256);
  a.wexp = false;
  EXPECT(same(check_gemm_args(a), "gemm_f8w: the weight rows' exponents (LnFold.wexp)"));
}

}  // namespace

int main() {
  test_traits();
  test_small_rules();
  test_fp16_plans();
  test_fp8_plans();
  std::printf("gemm_plan_test: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
