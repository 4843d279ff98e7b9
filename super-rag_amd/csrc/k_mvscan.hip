// K9s maxsim_scan: exact MaxSim top-k over the WHOLE token pool of a MultiVecIndex (sr_mv_search*;
// plan in sr_mv_plan.h, host side in multivec.hip, DESIGN.md "Whole-corpus MaxSim search").
//
// maxsim_scan_kernel<FP8, Q>: one workgroup (8 waves) per (window of consecutive rows of the slab,
// group of Q queries).  Against maxsim_kernel (k_multivec.hip), which scores gathered candidates of ONE
// query: the rows are consecutive, so the pool streams in order; the Q query blocks of the group sit
// side by side in LDS (the same rows of round_up(dim, 128) halfs and chunk swizzle chunk ^ (row & 15)),
// and every document fragment a lane loads is multiplied against all of them before it is dropped, so
// the pool is read ceil(B / Q) times per 64-token query block, not B times; the scores go to the slab's
// scratch [B][slab rows], from which mv_topk_kernel keeps the best k.
//   1. the window's rows come from two binary searches in the offsets (mv_window) and are walked in
//      spans (mv_span_end): up to 256 rows whose offsets, lengths and eligibility (live, allowed, not
//      empty) go to an LDS table with one coalesced read.  Ineligible rows get -inf here and none of
//      their tokens is loaded.
//   2. a span of short rows: wave w owns rows w, w + 8, ... whole, so nothing crosses waves and the
//      span needs no barrier; a row longer than the window's token target is a span of its own and its
//      16-token tiles w, w + 8, ... go to wave w as in maxsim_kernel, the token maxima folded through
//      LDS.  Loads are maxsim_kernel's: 16 bytes, four lanes per 128-byte line, groups of four column
//      steps in two register buffers, the next group (across tiles and rows of the span) in flight
//      while the current one multiplies; fp8 bytes become fp16 operands by v_cvt_scalef32_pk_f16_fp8.
//   3. a pair's arithmetic is maxsim_kernel's, step for step, so its bits are those of
//      sr_mv_score_rows: per (document token, query token) the same chain of v_mfma_f32_16x16x32_f16
//      from a zero accumulator (fp16: steps ascending, the chunks 2 g and 2 g + 1; fp8: chunk, + 1,
//      + 2, + 3 of each step), max over the document tokens (exact: which wave or lane group sees a
//      token is free), the 64-lane butterfly wave_sum over the query tokens of a block (lane = token,
//      lanes past the block's tokens add 0), blocks added in block order starting from 0.f, one
//      division by Lq, and for fp8 the factor 2^-8 last.  Queries of a group may differ in Lq: the
//      group walks to its longest query; a query without the current block is neither staged, nor
//      multiplied, nor written.  The partial sum of a longer query waits in the score scratch between
//      blocks (written and read back by the same lane).  No atomics on scores.
// Static LDS: the row table (3 KiB) + the cross-wave maxima [8][Q][64] fp32 (6 KiB at Q = 3).
//
// mv_topk_kernel: one workgroup per query keeps the running top-k of the scan as sorted 64-bit keys
// (ordered score << 32 | ~row: descending key order is (score desc, row asc), keys unique and
// non-zero).  It streams the slab's scores, leaves out -inf (ineligible) rows and everything not above
// the current k-th key, collects the rest in LDS and compresses with block_topk (sr_topk.h) whenever
// the LDS list would overflow and at the end.  The running list [B][k] is the only state between slabs.
#include <algorithm>
#include <type_traits>

#include "sr_common.h"
#include "sr_kernels.h"
#include "sr_mv_plan.h"
#include "sr_topk.h"

namespace sr {

namespace {

constexpr int MVS_THREADS = 512;
constexpr int MVS_WAVES = MVS_THREADS / 64;
constexpr int MVS_QT = 64;  // query tokens per LDS block

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct MvScanArgs {
  const void* pool;       // [n_tokens][dim] fp16, or e4m3 bytes
  const int64_t* off;     // [n_rows + 1]
  const uint8_t* live;    // [n_rows]
  const uint8_t* allow;   // [n_rows] or null
  const half_t* q;        // [B][ld_q][dim]
  const int32_t* q_len;   // [B]
  float* score;           // [B][ld_s], column = row - row0
  int64_t row0, row1, ld_s, target;
  int B, ld_q, dim, ngroups;
};

// eight e4m3 bytes -> the fp16 values of the same numbers, in byte order (as in k_multivec.hip)
__device__ __forceinline__ half8 mvs_e4m3x8_to_f16(uint32_t w0, uint32_t w1) {
  const half2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w0, 1.f, false);
  const half2_t b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w0, 1.f, true);
  const half2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w1, 1.f, false);
  const half2_t d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w1, 1.f, true);
  return half8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

template <bool FP8, int Q>
__global__ __launch_bounds__(MVS_THREADS) void maxsim_scan_kernel(MvScanArgs a) {
  using Buf = std::conditional_t<FP8, u32x4, half8>;  // one 16-byte load
  extern __shared__ __attribute__((aligned(16))) unsigned char mvs_smem[];
  __shared__ int64_t c_off[kMvSpanRows];
  __shared__ int c_len[kMvSpanRows];  // 0 for a row that is dead, not allowed or empty
  __shared__ float red[MVS_WAVES][Q][MVS_QT];
  __shared__ int first_long;
  half_t* qtile = reinterpret_cast<half_t*>(mvs_smem);

  const int tid = threadIdx.x, lane = tid & 63, gl = lane >> 4, r16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dim = a.dim;
  const int b0 = (int)(blockIdx.x % (unsigned)a.ngroups) * Q;
  const int64_t win = (int64_t)(blockIdx.x / (unsigned)a.ngroups);
  int64_t ra, rb;
  mv_window(a.off, a.row0, a.row1, a.target, win, &ra, &rb);
  if (ra >= rb) return;

  // (never more query tokens than the caller's rows hold, nor than the documented limit)
  int Lq[Q], maxLq = 0;
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    Lq[j] = b0 + j < a.B ? max(0, min(min(a.q_len[b0 + j], a.ld_q), SR_MV_MAX_QUERY_TOKENS)) : 0;
    maxLq = max(maxLq, Lq[j]);
  }

  // steps of one token row: 64 columns (fp16) or 128 columns plus, at dim % 128 == 64, a half step
  const int nfull = dim >> 7, nk = FP8 ? (dim + 127) >> 7 : dim >> 6, ng = (nk + 3) >> 2, nchunk = dim >> 3;
  const int lds_ld = (dim + 127) & ~127;
  const int blk = MVS_QT * lds_ld;  // halfs of one query's block
  const int nqb = max(1, (maxLq + MVS_QT - 1) / MVS_QT);

  for (int qb = 0; qb < nqb; ++qb) {
    int rows_q[Q], nqt[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      rows_q[j] = max(0, min(MVS_QT, Lq[j] - qb * MVS_QT));
      nqt[j] = (rows_q[j] + 15) >> 4;
    }
    __syncthreads();  // every wave is past its last read of the previous blocks
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      if (nqt[j] > 0) {
        const half_t* qsrc = a.q + ((int64_t)(b0 + j) * a.ld_q + (int64_t)qb * MVS_QT) * dim;
        half_t* qt = qtile + j * blk;
        const int total = nqt[j] * 16 * nchunk;
        for (int p = tid; p < total; p += MVS_THREADS) {
          const int row = p / nchunk, ch = p - row * nchunk;
          half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
          if (row < rows_q[j]) v = *reinterpret_cast<const half8*>(qsrc + (int64_t)row * dim + ch * 8);
          *reinterpret_cast<half8*>(qt + row * lds_ld + ((ch ^ (row & 15)) << 3)) = v;
        }
      }
    }

    for (int64_t rs = ra; rs < rb;) {
      // 1. the span's row table
      __syncthreads();  // the previous span's table and maxima are read (and the query blocks staged)
      if (tid == 0) first_long = kMvSpanRows;
      __syncthreads();
      const int nload = (int)min((int64_t)kMvSpanRows, rb - rs);
      if (tid < nload) {
        const int64_t row = rs + tid;
        const int64_t o = a.off[row], raw = a.off[row + 1] - o;
        const bool ok = a.live[row] != 0 && (a.allow == nullptr || a.allow[row] != 0);
        c_off[tid] = o;
        c_len[tid] = ok ? (int)raw : 0;
        if (raw > a.target) atomicMin(&first_long, tid);
      }
      __syncthreads();
      const int fl = first_long;
      const bool split = fl == 0;  // one long row, its tiles over the waves
      const int R = split ? 1 : min(nload, fl);
      if (qb == 0 && tid < R) {
#pragma unroll
        for (int j = 0; j < Q; ++j)
          if (b0 + j < a.B && (c_len[tid] == 0 || Lq[j] == 0))
            a.score[(int64_t)(b0 + j) * a.ld_s + (rs + tid - a.row0)] = -INFINITY;
      }
      const int64_t col0 = rs - a.row0;
      rs += R;
      if (maxLq == 0) continue;

      auto tiles_of = [&](int c) { return (__builtin_amdgcn_readfirstlane(c_len[c]) + 15) >> 4; };
      // 16-byte loads of group g of tile t of row c of the span (maxsim_kernel's)
      auto load = [&](Buf (&buf)[8], int c, int t, int g) {
        const int len = __builtin_amdgcn_readfirstlane(c_len[c]);
        const int tok = min(t * 16 + r16, len - 1);
        if constexpr (FP8) {
          const uint8_t* p = static_cast<const uint8_t*>(a.pool) + (c_off[c] + tok) * dim;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int ks = g * 4 + u;
            const bool full = ks < nfull;
            if (ks < nk) {
              buf[2 * u] = *reinterpret_cast<const u32x4*>(p + ks * 128 + gl * (full ? 32 : 16));
              if (full) buf[2 * u + 1] = *reinterpret_cast<const u32x4*>(p + ks * 128 + gl * 32 + 16);
            }
          }
        } else {
          const half_t* p = static_cast<const half_t*>(a.pool) + (c_off[c] + tok) * dim + gl * 16;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int ks = g * 4 + u;
            if (ks < nk) {
              buf[2 * u] = *reinterpret_cast<const half8*>(p + ks * 64);
              buf[2 * u + 1] = *reinterpret_cast<const half8*>(p + ks * 64 + 8);
            }
          }
        }
      };
      float4v acc[Q][4];
#pragma unroll
      for (int j = 0; j < Q; ++j)
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) acc[j][qi] = float4v{0.f, 0.f, 0.f, 0.f};
      // one MFMA k-step: 8 columns per lane, every query's fragment at the same chunk of its row
      auto mfma_chunk = [&](const half8 da, int chunk) {
        const half_t* f = qtile + r16 * lds_ld + ((chunk ^ r16) << 3);
#pragma unroll
        for (int j = 0; j < Q; ++j) {
#pragma unroll
          for (int qi = 0; qi < 4; ++qi) {
            if (qi < nqt[j]) {
              const half8 fb = *reinterpret_cast<const half8*>(f + j * blk + qi * 16 * lds_ld);
              acc[j][qi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(da, fb, acc[j][qi], 0, 0, 0);
            }
          }
        }
      };
      auto compute = [&](const Buf (&buf)[8], int g) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int ks = g * 4 + u;
          if constexpr (FP8) {
            const bool full = ks < nfull;
            if (ks < nk) {  // chunks 4 gl .. 4 gl + 3 of a step's 16, 2 gl and 2 gl + 1 of a half step's 8
              const int chunk = ks * 16 + gl * (full ? 4 : 2);
              const u32x4 w0 = buf[2 * u];
              mfma_chunk(mvs_e4m3x8_to_f16(w0[0], w0[1]), chunk);
              mfma_chunk(mvs_e4m3x8_to_f16(w0[2], w0[3]), chunk + 1);
              if (full) {
                const u32x4 w1 = buf[2 * u + 1];
                mfma_chunk(mvs_e4m3x8_to_f16(w1[0], w1[1]), chunk + 2);
                mfma_chunk(mvs_e4m3x8_to_f16(w1[2], w1[3]), chunk + 3);
              }
            }
          } else {
            if (ks < nk) {
              mfma_chunk(buf[2 * u], ks * 8 + 2 * gl);
              mfma_chunk(buf[2 * u + 1], ks * 8 + 2 * gl + 1);
            }
          }
        }
      };

      // 2. this wave's work list: (row, tile, group), the next item always one ahead
      const int r_first = split ? 0 : wave, r_step = split ? 1 : MVS_WAVES;
      const int t_first = split ? wave : 0, t_step = split ? MVS_WAVES : 1;
      int nc = r_first, nt = t_first, ngi = 0;
      while (nc < R && nt >= tiles_of(nc)) {
        nc += r_step;
        nt = t_first;
      }
      Buf bufA[8], bufB[8];
      int par = 0;
      if (nc < R) load(bufA, nc, nt, ngi);

      for (int c = r_first; c < R; c += r_step) {
        const int len = __builtin_amdgcn_readfirstlane(c_len[c]);
        if (len == 0) continue;  // (-inf above; the same for every wave of a split row)
        float m[Q][4];
#pragma unroll
        for (int j = 0; j < Q; ++j)
#pragma unroll
          for (int qi = 0; qi < 4; ++qi) m[j][qi] = -INFINITY;
        while (nc == c) {
          const int ct = nt, cg = ngi;
          // advance the look-ahead
          if (++ngi == ng) {
            ngi = 0;
            nt += t_step;
            while (nc < R && nt >= tiles_of(nc)) {
              nc += r_step;
              nt = t_first;
            }
          }
          if (par == 0) {
            if (nc < R) load(bufB, nc, nt, ngi);
            compute(bufA, cg);
          } else {
            if (nc < R) load(bufA, nc, nt, ngi);
            compute(bufB, cg);
          }
          par ^= 1;
          if (cg == ng - 1) {  // the tile is complete: acc[j][qi][r] = d_{16 ct + 4 gl + r} . q^j_{16 qi + r16}
#pragma unroll
            for (int j = 0; j < Q; ++j) {
#pragma unroll
              for (int qi = 0; qi < 4; ++qi) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const float v = (ct * 16 + 4 * gl + r < len) ? acc[j][qi][r] : -INFINITY;
                  m[j][qi] = fmaxf(m[j][qi], v);
                }
                acc[j][qi] = float4v{0.f, 0.f, 0.f, 0.f};
              }
            }
          }
        }
        // 3. fold over the lane groups; lane l then takes the maximum of query token l of the block
        float tokmax[Q];
#pragma unroll
        for (int j = 0; j < Q; ++j) {
#pragma unroll
          for (int qi = 0; qi < 4; ++qi) {
            float v = m[j][qi];
            v = fmaxf(v, __shfl_xor(v, 16, 64));
            v = fmaxf(v, __shfl_xor(v, 32, 64));
            m[j][qi] = v;
          }
          tokmax[j] = gl == 0 ? m[j][0] : gl == 1 ? m[j][1] : gl == 2 ? m[j][2] : m[j][3];
        }
        if (split) {  // over the waves through LDS; wave j finishes query j
#pragma unroll
          for (int j = 0; j < Q; ++j) red[wave][j][lane] = tokmax[j];
          __syncthreads();
#pragma unroll
          for (int j = 0; j < Q; ++j) {
            float v = -INFINITY;
#pragma unroll
            for (int w = 0; w < MVS_WAVES; ++w) v = fmaxf(v, red[w][j][lane]);
            tokmax[j] = v;
          }
        }
        // 4. the token maxima of this block, summed in maxsim_kernel's order
#pragma unroll
        for (int j = 0; j < Q; ++j) {
          if (nqt[j] > 0 && (!split || wave == j)) {
            const float s = wave_sum(lane < rows_q[j] ? tokmax[j] : 0.f);
            if (lane == 0) {
              float* dst = a.score + (int64_t)(b0 + j) * a.ld_s + (col0 + c);
              const float tot = (qb ? *dst : 0.f) + s;
              const bool last = qb == (Lq[j] + MVS_QT - 1) / MVS_QT - 1;
              if constexpr (FP8) {  // the operands were 256 d; 2^-8 is exact
                *dst = last ? tot / (float)Lq[j] * 0.00390625f : tot;
              } else {
                *dst = last ? tot / (float)Lq[j] : tot;
              }
            }
          }
        }
      }
    }
  }
}

// ---- selection -------------------------------------------------------------------------------------
constexpr int MVT_BATCH = 8 * SEL_THREADS;  // scores looked at between two capacity checks

struct MvTopkSmem {
  uint64_t keys[SEL_CAP];
  SelShared sh;
  int cnt;
};

// score [B][ld_s]: the slab's columns [0, nrows) are the rows row0 ..; run_keys [B][k] / run_n [B]: the
// running list, sorted descending (read unless `first`, always written); `last`: out_score / out_rows
// [B][k] as well, -inf / -1 past the list, row_offset added to the real rows
__global__ __launch_bounds__(SEL_THREADS, 1) void mv_topk_kernel(
    const float* __restrict__ score, int64_t ld_s, int64_t row0, int64_t nrows, int k, int first, int last,
    uint64_t* __restrict__ run_keys, int* __restrict__ run_n, float* __restrict__ out_score,
    int64_t* __restrict__ out_rows, int64_t row_offset) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mvt_smem[];
  MvTopkSmem& S = *reinterpret_cast<MvTopkSmem*>(mvt_smem);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n0 = first ? 0 : run_n[b];
  for (int i = tid; i < n0; i += SEL_THREADS) S.keys[i] = run_keys[(int64_t)b * k + i];
  if (tid == 0) S.cnt = n0;
  __syncthreads();
  uint64_t tau = n0 == k ? S.keys[k - 1] : 0ull;  // a key has to be above it to enter
  int n = n0;
  auto compress = [&]() {  // S.keys[0 .. n) -> the best min(n, k), sorted; block-uniform
    const int m = block_topk([&](int i) { return S.keys[i]; }, n, k, S.sh);
    for (int i = tid; i < m; i += SEL_THREADS) S.keys[i] = S.sh.sel[i];
    if (tid == 0) S.cnt = m;
    if (m == k) tau = S.sh.sel[k - 1];
    n = m;
    __syncthreads();
  };
  const float* src = score + (int64_t)b * ld_s;
  for (int64_t base = 0; base < nrows; base += MVT_BATCH) {
    if (n + MVT_BATCH > SEL_CAP) compress();
    const int64_t end = min(nrows, base + MVT_BATCH);
    for (int64_t i = base + tid; i < end; i += SEL_THREADS) {
      const float s = src[i];
      if (s != -INFINITY) {  // (an ineligible row never enters; the key is built from the position)
        const uint64_t key = make_key(s, (uint32_t)(row0 + i));
        if (key > tau) S.keys[atomicAdd(&S.cnt, 1)] = key;
      }
    }
    __syncthreads();
    n = S.cnt;
    __syncthreads();
  }
  compress();
  for (int i = tid; i < n; i += SEL_THREADS) run_keys[(int64_t)b * k + i] = S.keys[i];
  if (tid == 0) run_n[b] = n;
  if (last) {
    for (int i = tid; i < k; i += SEL_THREADS) {
      const bool ok = i < n;
      out_score[(int64_t)b * k + i] = ok ? key_sim(S.keys[i]) : -INFINITY;
      out_rows[(int64_t)b * k + i] = ok ? (int64_t)key_row(S.keys[i]) + row_offset : -1;
    }
  }
}

template <bool FP8>
void scan_q(int Q, dim3 grid, size_t smem, hipStream_t s, const MvScanArgs& a) {
  auto go = [&](auto kernel) {
    // (per launch: the attribute belongs to the current device's copy of the kernel)
    SR_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kernel, grid, dim3(MVS_THREADS), smem, s, a);
  };
  switch (Q) {
    case 1: go(maxsim_scan_kernel<FP8, 1>); break;
    case 2: go(maxsim_scan_kernel<FP8, 2>); break;
    default: go(maxsim_scan_kernel<FP8, 3>); break;
  }
}

}  // namespace

void launch_maxsim_scan(const void* pool, int dtype, const int64_t* off, const uint8_t* live,
                        const uint8_t* allow, int dim, const half_t* q, const int32_t* q_len, int B, int ld_q,
                        int64_t row0, int64_t row1, int64_t T0, int64_t T1, float* score, int64_t ld_s,
                        hipStream_t s) {
  SR_CHECK(dim >= 64 && dim <= 1024 && dim % 64 == 0, "mv: dim must be a multiple of 64, <= 1024");
  SR_CHECK(dtype == SR_DTYPE_F16 || dtype == SR_DTYPE_FP8_E4M3, "mv.search: pool dtype");
  if (B <= 0 || row1 <= row0) return;
  SR_CHECK(row1 - row0 <= ld_s && T1 >= T0, "mv.search: slab arguments");
  const bool fp8 = dtype == SR_DTYPE_FP8_E4M3;
  const int Q = mv_group_queries(dim);
  SR_CHECK(Q >= 1 && Q <= 3, "mv.search: queries per workgroup");
  const int64_t grid = mv_scan_grid(T0, T1, kMvSpanTokens, B, Q);
  SR_CHECK(grid < (1ll << 31), "mv.search: too many workgroups in one slab (use smaller slab_rows)");
  MvScanArgs a;
  a.pool = pool;
  a.off = off;
  a.live = live;
  a.allow = allow;
  a.q = q;
  a.q_len = q_len;
  a.score = score;
  a.row0 = row0;
  a.row1 = row1;
  a.ld_s = ld_s;
  a.target = kMvSpanTokens;
  a.B = B;
  a.ld_q = ld_q;
  a.dim = dim;
  a.ngroups = (int)ceil_div(B, Q);
  // (profiling only: 32 query tokens assumed, one query block)
  const double tokens = (double)(T1 - T0);
  ProfScope prof(fp8 ? "maxsim_scan_fp8" : "maxsim_scan", s, 2.0 * tokens * dim * 32.0 * B,
                 tokens * dim * (fp8 ? 1.0 : 2.0) * a.ngroups + (double)B * (double)(row1 - row0) * 4.0);
  if (fp8)
    scan_q<true>(Q, dim3((unsigned)grid), (size_t)mv_scan_lds_bytes(dim), s, a);
  else
    scan_q<false>(Q, dim3((unsigned)grid), (size_t)mv_scan_lds_bytes(dim), s, a);
  SR_LAUNCH_CHECK();
}

void launch_mv_topk(const float* score, int64_t ld_s, int64_t row0, int64_t nrows, int B, int k, bool first,
                    bool last, uint64_t* run_keys, int* run_n, float* out_score, int64_t* out_rows,
                    int64_t row_offset, hipStream_t s) {
  SR_CHECK(k >= 1 && k <= SR_MAX_TOPK, "mv.search: k must be in [1, 1024]");
  SR_CHECK(row0 >= 0 && nrows >= 0 && row0 + nrows < 0xffffffffll, "mv.search: rows do not fit a 32-bit key");
  if (B <= 0) return;
  SR_HIP(hipFuncSetAttribute((const void*)mv_topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)sizeof(MvTopkSmem)));
  ProfScope prof("mv_topk", s, 0.0, (double)B * (double)nrows * 4.0 + (double)B * k * 28.0);
  hipLaunchKernelGGL(mv_topk_kernel, dim3((unsigned)B), dim3(SEL_THREADS), sizeof(MvTopkSmem), s, score, ld_s,
                     row0, nrows, k, first ? 1 : 0, last ? 1 : 0, run_keys, run_n, out_score, out_rows,
                     row_offset);
  SR_LAUNCH_CHECK();
}

}  // namespace sr
