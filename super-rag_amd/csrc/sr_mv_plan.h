// Plan of the whole-corpus MaxSim scan (sr_mv_search*; k_mvscan.hip, multivec.hip; DESIGN.md
// "Whole-corpus MaxSim search").  Plain C++: no HIP call or header, so tests/native/mv_plan_test.cpp
// builds it as a program of its own under the sanitizers.  The functions marked SR_MV_HD are device
// code as well: the scan kernel finds its window with mv_window / mv_first_row_at; mv_span_end states the
// span rule that the kernel applies to 256 rows at a time (a row table in LDS and one atomicMin).
//
//   slabs    the rows [0, n_rows) in runs of at most slab_rows consecutive rows; the score scratch
//            [B][slab rows] fp32 is the only memory that grows with the slab.
//   windows  a slab's tokens [T0, T1) in runs of `target` tokens: window w owns the rows whose FIRST
//            token position lies in [T0 + w target, T0 + (w + 1) target), found by two binary searches
//            in the offsets (mv_window).  A row belongs to exactly one window, whatever its length; the
//            rows without tokens share their successor's position and go with it (those at the very end
//            of the slab sit at T1, hence the "+ 1" of mv_windows).  One workgroup per (window, query
//            group).
//   spans    a window's rows are walked in spans (mv_span_end): a row longer than `target` is a span of
//            its own (its tiles spread over the workgroup's waves); the other rows go in runs of at most
//            kMvSpanRows (what the kernel's LDS row table holds), one row per wave at a time.
//   Q        query blocks (64 tokens x round_up(dim, 128) fp16) a workgroup keeps in LDS next to its
//            static state, capped where the accumulators (16 fp32 per query and lane) would spill.
#pragma once

#include <stdint.h>

#include <algorithm>

#if defined(__HIPCC__)
#define SR_MV_HD __host__ __device__ inline
#else
#define SR_MV_HD inline
#endif

namespace sr {

constexpr int64_t kMvScratchBytes = int64_t(64) << 20;  // the default slab's score scratch (B x rows x 4)
constexpr int64_t kMvMinSlabRows = 1024;
constexpr int kMvSpanRows = 256;            // rows of one span (the kernel's LDS row table)
constexpr int64_t kMvSpanTokens = 2048;     // token target of a window
constexpr int kMvLdsBytes = 160 * 1024;     // LDS of a CU
constexpr int kMvStaticLds = 16 * 1024;     // kept free for the kernel's static state (it uses < 12 KiB)
constexpr int kMvMaxQ = 3;                  // accumulators: 16 VGPRs per query; 4 queries spill

// rows of a slab: the caller's slab_rows, or (0) as many as keep B x rows x 4 bytes within 64 MiB, at
// least 1024
inline int64_t mv_slab_rows(int64_t slab_rows, int B) {
  if (slab_rows > 0) return slab_rows;
  return std::max<int64_t>(kMvMinSlabRows, kMvScratchBytes / (4 * (int64_t)std::max(B, 1)));
}

inline int64_t mv_slab_count(int64_t n_rows, int64_t slab) { return n_rows <= 0 ? 0 : (n_rows + slab - 1) / slab; }

// slab i of mv_slab_count(n_rows, slab): rows [r0, r1)
inline void mv_slab(int64_t n_rows, int64_t slab, int64_t i, int64_t* r0, int64_t* r1) {
  *r0 = i * slab;
  *r1 = std::min(n_rows, *r0 + slab);
}

// bytes of one query block in LDS
inline int mv_block_bytes(int dim) { return 64 * ((dim + 127) / 128 * 128) * 2; }

// queries per workgroup and the dynamic LDS they take
inline int mv_group_queries(int dim) {
  return std::max(1, std::min(kMvMaxQ, (kMvLdsBytes - kMvStaticLds) / mv_block_bytes(dim)));
}
inline int mv_scan_lds_bytes(int dim) { return mv_group_queries(dim) * mv_block_bytes(dim); }

// windows of a slab holding the tokens [T0, T1)
inline int64_t mv_windows(int64_t T0, int64_t T1, int64_t target) { return (T1 - T0) / target + 1; }

// workgroups of a slab's scan: windows x query groups
inline int64_t mv_scan_grid(int64_t T0, int64_t T1, int64_t target, int B, int Q) {
  return mv_windows(T0, T1, target) * ((B + Q - 1) / Q);
}

// the first row r of [r0, r1] with off[r] >= t (r1 when there is none below it); off ascending
SR_MV_HD int64_t mv_first_row_at(const int64_t* off, int64_t r0, int64_t r1, int64_t t) {
  int64_t lo = r0, hi = r1;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] >= t)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// rows [*ra, *rb) of window w of the slab [r0, r1)
SR_MV_HD void mv_window(const int64_t* off, int64_t r0, int64_t r1, int64_t target, int64_t w, int64_t* ra,
                        int64_t* rb) {
  const int64_t lo = off[r0] + w * target;
  *ra = mv_first_row_at(off, r0, r1, lo);
  *rb = mv_first_row_at(off, r0, r1, lo + target);
}

// end of the span that starts at row rs of a window ending at rb (rs < rb): rs + 1 when the row holds
// more than `target` tokens, else the rows up to the next such row, max_rows at the most
SR_MV_HD int64_t mv_span_end(const int64_t* off, int64_t rs, int64_t rb, int64_t target, int max_rows) {
  if (off[rs + 1] - off[rs] > target) return rs + 1;
  int64_t re = rs + 1;
  while (re < rb && re - rs < max_rows && off[re + 1] - off[re] <= target) ++re;
  return re;
}

}  // namespace sr
