// The whole-corpus MaxSim scan's plan (super-rag_amd/csrc/sr_mv_plan.h) as a program of its own, built
// with -fsanitize=address,undefined by tests/test_mv_plan.py: slabs, windows and spans tile the rows,
// the edge cases of the span rule, Q and the LDS bytes for every dim, the default slab.
#include <cstdio>
#include <vector>

#include "sr_mv_plan.h"

using namespace sr;

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      ++failures;                                                         \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
    }                                                                     \
  } while (0)

static std::vector<int64_t> offsets(const std::vector<int64_t>& len) {
  std::vector<int64_t> off(1, 0);  // exactly n + 1 entries: a read past the end is an ASan report
  for (int64_t l : len) off.push_back(off.back() + l);
  return off;
}

// every row of [0, n) in exactly one slab, one window of it and one span of that, in order; spans obey
// the rule (a long row alone, at most max_rows rows, no long row inside a longer span)
static void check_tiling(const std::vector<int64_t>& len, int64_t slab_rows, int B, int64_t target,
                         int max_rows) {
  const std::vector<int64_t> off = offsets(len);
  const int64_t n = (int64_t)len.size();
  const int64_t slab = mv_slab_rows(slab_rows, B);
  CHECK(slab >= 1);
  const int64_t ns = mv_slab_count(n, slab);
  int64_t next = 0;
  for (int64_t i = 0; i < ns; ++i) {
    int64_t r0, r1;
    mv_slab(n, slab, i, &r0, &r1);
    CHECK(r0 == next && r1 > r0 && r1 - r0 <= slab && r1 <= n);
    const int64_t nw = mv_windows(off[r0], off[r1], target);
    CHECK(nw >= 1);
    CHECK(mv_scan_grid(off[r0], off[r1], target, 5, 2) == nw * 3);
    int64_t at = r0;
    for (int64_t w = 0; w < nw; ++w) {
      int64_t ra, rb;
      mv_window(off.data(), r0, r1, target, w, &ra, &rb);
      CHECK(ra == at && rb >= ra && rb <= r1);
      // the window owns the rows that START in its tokens
      for (int64_t r = ra; r < rb; ++r) {
        CHECK(off[r] >= off[r0] + w * target && off[r] < off[r0] + (w + 1) * target);
      }
      for (int64_t rs = ra; rs < rb;) {
        const int64_t re = mv_span_end(off.data(), rs, rb, target, max_rows);
        CHECK(re > rs && re <= rb && re - rs <= max_rows);
        if (len[rs] > target) CHECK(re == rs + 1);
        for (int64_t r = rs; r < re; ++r) CHECK(re - rs == 1 || len[r] <= target);
        // maximal: the span stops only at the window's end, the row limit or before a long row
        if (len[rs] <= target && re < rb) CHECK(re - rs == max_rows || len[re] > target);
        rs = re;
      }
      at = rb;
    }
    CHECK(at == r1);  // the windows tile the slab
    next = r1;
  }
  CHECK(next == n);  // the slabs tile the rows
}

int main() {
  // -- slabs and spans over hand-made rows ---------------------------------------------------------------
  const std::vector<std::vector<int64_t>> corpora = {
      {},                                              // n_rows == 0
      {0},                                             // one row without tokens
      {0, 0, 0, 0, 0, 0, 0},                           // an all-empty slab
      {5},                                             //
      {0, 0, 3, 1, 0, 9, 2, 0, 0},                     // empty rows at either end
      {3, 1, 40, 2, 2},                                // one row longer than the target (8)
      {40},                                            // only a long row
      {0, 40, 0},                                      // a long row between empty ones
      {8, 8, 8, 8},                                    // rows of exactly the target
      {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},   // more rows than a span holds (max_rows 4)
      {9, 9, 0, 0, 0, 0, 0, 0, 9, 1, 0},               //
  };
  for (const auto& len : corpora) {
    const int64_t n = (int64_t)len.size();
    for (int64_t sr : {int64_t(1), int64_t(7), n - 1, n, n + 1, int64_t(0)}) {
      if (sr < 0) continue;
      for (int64_t target : {int64_t(1), int64_t(8), int64_t(2048)})
        for (int max_rows : {1, 4, 256}) check_tiling(len, sr, 3, target, max_rows);
    }
  }
  // a longer pseudo-random corpus (LCG), lengths 0 .. 4099 with many empty rows
  {
    std::vector<int64_t> len;
    uint64_t s = 12345;
    for (int i = 0; i < 3000; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const uint64_t r = s >> 33;
      len.push_back(r % 5 == 0 ? 0 : r % 97 == 0 ? (int64_t)(r % 4100) : (int64_t)(r % 40));
    }
    const int64_t n = (int64_t)len.size();
    for (int64_t sr : {int64_t(1), int64_t(7), n - 1, n, n + 1, int64_t(0)})
      check_tiling(len, sr, 32, kMvSpanTokens, kMvSpanRows);
    check_tiling(len, 0, 32, 64, 16);
  }
  // hand-made windows: rows 3 | 1 | 40 | 2 | 2, target 8: the long row starts in window 0 and takes the
  // windows 1 .. 4 with it (they own no row); the last two rows start at tokens 44 and 46
  {
    const std::vector<int64_t> off = offsets({3, 1, 40, 2, 2});
    CHECK(mv_windows(0, 48, 8) == 7);
    int64_t ra, rb;
    mv_window(off.data(), 0, 5, 8, 0, &ra, &rb);
    CHECK(ra == 0 && rb == 3);
    CHECK(mv_span_end(off.data(), 0, 3, 8, 256) == 2);   // the two short rows
    CHECK(mv_span_end(off.data(), 2, 3, 8, 256) == 3);   // the long row alone
    for (int64_t w = 1; w <= 4; ++w) {
      mv_window(off.data(), 0, 5, 8, w, &ra, &rb);
      CHECK(ra == 3 && rb == 3);
    }
    mv_window(off.data(), 0, 5, 8, 5, &ra, &rb);
    CHECK(ra == 3 && rb == 5);
    mv_window(off.data(), 0, 5, 8, 6, &ra, &rb);
    CHECK(ra == 5 && rb == 5);
    // a slab that starts inside the corpus: rows [3, 5), tokens [44, 48)
    CHECK(mv_windows(off[3], off[5], 8) == 1);
    mv_window(off.data(), 3, 5, 8, 0, &ra, &rb);
    CHECK(ra == 3 && rb == 5);
  }
  // trailing rows without tokens sit at T1 and still have a window
  {
    const std::vector<int64_t> off = offsets({8, 8, 0, 0});
    CHECK(mv_windows(0, 16, 8) == 3);
    int64_t ra, rb;
    mv_window(off.data(), 0, 4, 8, 2, &ra, &rb);
    CHECK(ra == 2 && rb == 4);
  }

  // -- Q and LDS for every dim ---------------------------------------------------------------------------
  for (int dim = 64; dim <= 1024; dim += 64) {
    const int Q = mv_group_queries(dim);
    CHECK(Q >= 1 && Q <= kMvMaxQ);
    CHECK(mv_block_bytes(dim) == 64 * ((dim + 127) / 128 * 128) * 2);
    CHECK(mv_scan_lds_bytes(dim) == Q * mv_block_bytes(dim));
    CHECK(mv_scan_lds_bytes(dim) <= kMvLdsBytes - kMvStaticLds);
    // as many as fit, up to the cap
    CHECK(Q == kMvMaxQ || (Q + 1) * mv_block_bytes(dim) > kMvLdsBytes - kMvStaticLds);
  }
  CHECK(mv_block_bytes(128) == 16 * 1024 && mv_block_bytes(1024) == 128 * 1024);
  CHECK(mv_group_queries(64) == 3 && mv_group_queries(128) == 3 && mv_group_queries(256) == 3);
  CHECK(mv_group_queries(320) == 3 && mv_group_queries(384) == 3);
  CHECK(mv_group_queries(448) == 2 && mv_group_queries(512) == 2);
  CHECK(mv_group_queries(576) == 1 && mv_group_queries(1024) == 1);
  CHECK(kMvLdsBytes == 160 * 1024);

  // -- the default slab ----------------------------------------------------------------------------------
  CHECK(mv_slab_rows(0, 1) == (int64_t(64) << 20) / 4);
  CHECK(mv_slab_rows(0, 32) == (int64_t(64) << 20) / 128);
  CHECK(mv_slab_rows(0, 1024) == 16384);
  CHECK(mv_slab_rows(0, 1 << 20) == 1024);  // never below 1024 rows
  CHECK(mv_slab_rows(0, 0) == mv_slab_rows(0, 1));
  CHECK(mv_slab_rows(7, 1024) == 7);
  for (int B : {1, 32, 1024})
    CHECK(mv_slab_rows(0, B) * 4 * B <= (int64_t(64) << 20) || mv_slab_rows(0, B) == 1024);
  CHECK(mv_slab_count(0, 5) == 0 && mv_slab_count(5, 5) == 1 && mv_slab_count(6, 5) == 2);

  std::printf("mv_plan_test: %d failures\n", failures);
  return failures ? 1 : 0;
}
