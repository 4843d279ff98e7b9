// K2f score_fuse / score_rows: score-based hybrid fusion (Weaviate relativeScoreFusion, Milvus
// WeightedRanker, linear combination with min-max normalisation; Bruch et al. 2023, "An Analysis of
// Fusion Functions for Hybrid Retrieval": SR_FUSE_FLOOR is their theoretical-minimum variant).
//
// score_fuse, one workgroup (8 waves) per query, fuses two scored row lists a [ka] and b [kb]
// (row < 0: an absent entry, anywhere; a row at most once per list; no order assumed) with the
// optional a-metric scores side_a [kb] of the b rows and, its mirror, the optional b-metric scores
// side_b [ka] of the a rows (include/super_rag_mi355x.h states the function):
//   1. hi / lo of each list: block reduction over its valid scores (side scores never enter)
//   2. slot -> join key (row + 1) << 13 | list << 12 | index, list a = 1, 0 for an absent entry;
//      bitonic_sort_desc: the entries of one row are adjacent, list a's first
//   3. the first entry of a row (its head) takes the row's a and b scores: the a entry's score or,
//      for a row of list b alone, side_a; the b score from the entry itself or the one behind the
//      head or, for a row of list a alone, side_b.  fused = alpha norm_a + (1 - alpha) norm_b, every operation rounded once (no contraction)
//   4. the head's slot becomes ordered_bits(fused) << 32 | position + 1 (0: not a head, or below
//      min_score) while src[position] keeps (index in a + 1) | (index in b + 1) << 12.  The join order
//      is row DESCENDING, so on equal fused scores the larger position is the smaller row: the second
//      bitonic_sort_desc gives (fused desc, row asc), the store's tie rule
//   5. output slot i re-reads row and scores of key i through src[] (the lists are in L2)
// LDS: 4096 x 8 B keys + 4096 x 4 B src + 128 B partials = 49,280 B.  Nothing is indexed by a row id.
//
// score_rows, one wave per (query, row) pair: out = q . x_row over the fp16 rows, fp32 accumulation,
// 16-byte loads; -inf for a row outside [0, n_rows) or tombstoned (checked before the row is read).
#include <algorithm>

#include "sr_common.h"
#include "sr_kernels.h"
#include "sr_topk.h"

namespace sr {

namespace {

constexpr int FTHREADS = 512;                   // 8 waves
constexpr int FMAXL = 2 * SR_MAX_TOPK;          // entries per list
constexpr int FMAXN = 2 * FMAXL;                // slots
constexpr int FPER = FMAXN / FTHREADS;          // slots per thread
constexpr int FIDX_BITS = 12;                   // index + 1 <= 2048
constexpr uint32_t FIDX_MASK = (1u << FIDX_BITS) - 1;

struct FuseArgs {
  const float* score_a;     // [B][ka]
  const int64_t* rows_a;    // [B][ka]
  int ka;
  const float* score_b;     // [B][kb]
  const int64_t* rows_b;    // [B][kb]
  int kb;
  const float* side_a;      // [B][kb] or null
  const float* side_b;      // [B][ka] or null
  int N;                    // power of two >= ka + kb, in [64, FMAXN]
  int mode;
  float alpha, one_minus_alpha, floor_a, floor_b, min_score;
  int k_out;
  float* out_score;         // [B][k_out]
  int64_t* out_rows;        // [B][k_out]
  float* out_a;             // [B][k_out] or null
  float* out_b;             // [B][k_out] or null
};

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// (no FMA contraction below: tests/fuse_ref.py restates the function in numpy, which rounds every
// operation)
#pragma clang fp contract(off)
__device__ __forceinline__ float fuse_norm(float s, float hi, float lo) {
  return hi > lo ? fmaxf(0.f, __fdiv_rn(s - lo, hi - lo)) : 1.f;
}

__global__ __launch_bounds__(FTHREADS, 1) void score_fuse_kernel(FuseArgs a) {
  __shared__ uint64_t key[FMAXN];
  __shared__ uint32_t src[FMAXN];
  __shared__ float red[4][FTHREADS / 64];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ka = a.ka, kb = a.kb, N = a.N;
  const float* sa = a.score_a + (int64_t)b * ka;
  const int64_t* ra = a.rows_a + (int64_t)b * ka;
  const float* sb = a.score_b + (int64_t)b * kb;
  const int64_t* rb = a.rows_b + (int64_t)b * kb;
  const float* side = a.side_a ? a.side_a + (int64_t)b * kb : nullptr;
  const float* sideb = a.side_b ? a.side_b + (int64_t)b * ka : nullptr;

  // 1. + 2. join keys, and the extremes of each list's valid scores
  float hia = -INFINITY, loa = INFINITY, hib = -INFINITY, lob = INFINITY;
  for (int i = tid; i < N; i += FTHREADS) {
    uint64_t v = 0ull;
    if (i < ka) {
      const int64_t r = ra[i];
      if (r >= 0) {
        const float s = sa[i];
        hia = fmaxf(hia, s);
        loa = fminf(loa, s);
        v = ((uint64_t)((uint32_t)r + 1u) << 13) | (1ull << 12) | (uint64_t)i;
      }
    } else if (i < ka + kb) {
      const int j = i - ka;
      const int64_t r = rb[j];
      if (r >= 0) {
        const float s = sb[j];
        hib = fmaxf(hib, s);
        lob = fminf(lob, s);
        v = ((uint64_t)((uint32_t)r + 1u) << 13) | (uint64_t)j;
      }
    }
    key[i] = v;
  }
  hia = wave_max(hia);
  loa = wave_min(loa);
  hib = wave_max(hib);
  lob = wave_min(lob);
  if (lane == 0) {
    red[0][wave] = hia;
    red[1][wave] = loa;
    red[2][wave] = hib;
    red[3][wave] = lob;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < FTHREADS / 64; ++w) {
    hia = fmaxf(hia, red[0][w]);
    loa = fminf(loa, red[1][w]);
    hib = fmaxf(hib, red[2][w]);
    lob = fminf(lob, red[3][w]);
  }
  if (a.mode == SR_FUSE_FLOOR) {
    loa = a.floor_a;
    lob = a.floor_b;
  }
  bitonic_sort_desc(key, N);

  // 3. + 4. heads -> fused keys (kept in registers until every neighbour has been read)
  uint64_t k2[FPER];
#pragma unroll
  for (int e = 0; e < FPER; ++e) {
    const int p = tid + e * FTHREADS;
    k2[e] = 0ull;
    if (p >= N) continue;
    const uint64_t cur = key[p];
    if (cur == 0ull) continue;
    const uint64_t row1 = cur >> 13;
    if (p > 0 && (key[p - 1] >> 13) == row1) continue;   // not the row's first entry
    const int idx = (int)(cur & 0xfffu);
    int ia = -1, ib = -1;
    if ((cur >> 12) & 1ull) {
      ia = idx;
      const uint64_t nxt = p + 1 < N ? key[p + 1] : 0ull;
      if ((nxt >> 13) == row1 && ((nxt >> 12) & 1ull) == 0ull) ib = (int)(nxt & 0xfffu);
    } else {
      ib = idx;
    }
    float xa = -INFINITY, xb = -INFINITY;
    if (ia >= 0) xa = sa[ia];
    else if (side) xa = side[ib];
    if (ib >= 0) xb = sb[ib];
    else if (sideb) xb = sideb[ia];
    const float na = xa > -INFINITY ? fuse_norm(xa, hia, loa) : 0.f;
    const float nb = xb > -INFINITY ? fuse_norm(xb, hib, lob) : 0.f;
    const float fused = (a.alpha * na) + (a.one_minus_alpha * nb);
    src[p] = (uint32_t)(ia + 1) | ((uint32_t)(ib + 1) << FIDX_BITS);
    if (!(fused < a.min_score)) k2[e] = ((uint64_t)ordered_bits(fused) << 32) | (uint64_t)(p + 1);
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < FPER; ++e) {
    const int p = tid + e * FTHREADS;
    if (p < N) key[p] = k2[e];
  }
  __syncthreads();
  bitonic_sort_desc(key, N);

  // 5. outputs
  const int64_t ob = (int64_t)b * a.k_out;
  for (int i = tid; i < a.k_out; i += FTHREADS) {
    const uint64_t kk = i < N ? key[i] : 0ull;
    float fs = -INFINITY, xa = -INFINITY, xb = -INFINITY;
    int64_t row = -1;
    if (kk != 0ull) {
      const uint32_t s = src[(uint32_t)kk - 1u];
      const int ia = (int)(s & FIDX_MASK) - 1, ib = (int)(s >> FIDX_BITS) - 1;
      fs = unordered_bits((uint32_t)(kk >> 32));
      row = ia >= 0 ? ra[ia] : rb[ib];
      if (ia >= 0) xa = sa[ia];
      else if (side) xa = side[ib];
      if (ib >= 0) xb = sb[ib];
      else if (sideb) xb = sideb[ia];
    }
    a.out_score[ob + i] = fs;
    a.out_rows[ob + i] = row;
    if (a.out_a) a.out_a[ob + i] = xa;
    if (a.out_b) a.out_b[ob + i] = xb;
  }
}

constexpr int RTHREADS = 256;   // 4 waves = 4 pairs

__global__ __launch_bounds__(RTHREADS) void score_rows_kernel(
    const half_t* __restrict__ corpus, int ld, int64_t n_rows, const uint8_t* __restrict__ live,
    const half_t* __restrict__ qn, const int64_t* __restrict__ rows, int B, int K,
    int64_t row_offset, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * (RTHREADS / 64) + (threadIdx.x >> 6);
  if (j >= K) return;   // (wave-uniform)
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int64_t raw = rows[(int64_t)b * K + j];
    const int64_t r = raw - row_offset;
    const bool ok = raw >= 0 && r >= 0 && r < n_rows && live[r] != 0;
    float acc = 0.f;
    if (ok) {
      // rows and queries are zero padded to ld, a multiple of 64 halfs
      const half8* x = reinterpret_cast<const half8*>(corpus + r * ld);
      const half8* q = reinterpret_cast<const half8*>(qn + (int64_t)b * ld);
      for (int c = lane; c < ld / 8; c += 64) {
        const half8 xv = x[c], qv = q[c];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf((float)qv[e], (float)xv[e], acc);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) out[(int64_t)b * K + j] = ok ? acc : -INFINITY;
  }
}

}  // namespace

void fuse_check_args(int B, int ka, int kb, int mode, float alpha, int k_out, bool allow_full) {
  SR_CHECK(B >= 0, "score_fuse: negative batch");
  SR_CHECK(ka >= 0 && ka <= FMAXL && kb >= 0 && kb <= FMAXL, "score_fuse: list length must be in [0, 2048]");
  SR_CHECK(k_out >= 1 && k_out <= FMAXL, "score_fuse: k_out must be in [1, 2048]");
  SR_CHECK(mode == SR_FUSE_MINMAX || mode == SR_FUSE_FLOOR || (allow_full && mode == SR_FUSE_FLOOR_FULL),
           "score_fuse: mode must be SR_FUSE_MINMAX or SR_FUSE_FLOOR");
  SR_CHECK(alpha >= 0.f && alpha <= 1.f, "score_fuse: alpha must be in [0, 1]");   // (false for NaN)
}

void launch_score_fuse(const float* score_a, const int64_t* rows_a, int ka, const float* score_b,
                       const int64_t* rows_b, int kb, const float* side_a, int B, int mode,
                       float alpha, float floor_a, float floor_b, float min_score, int k_out,
                       float* out_score, int64_t* out_rows, float* out_a, float* out_b,
                       hipStream_t s, const float* side_b) {
  fuse_check_args(B, ka, kb, mode, alpha, k_out);
  if (B == 0) return;
  int N = 64;
  while (N < ka + kb) N <<= 1;
  FuseArgs a;
  a.score_a = score_a;
  a.rows_a = rows_a;
  a.ka = ka;
  a.score_b = score_b;
  a.rows_b = rows_b;
  a.kb = kb;
  a.side_a = kb ? side_a : nullptr;
  a.side_b = ka ? side_b : nullptr;
  a.N = N;
  a.mode = mode;
  a.alpha = alpha;
  a.one_minus_alpha = 1.0f - alpha;
  a.floor_a = floor_a;
  a.floor_b = floor_b;
  a.min_score = min_score;
  a.k_out = k_out;
  a.out_score = out_score;
  a.out_rows = out_rows;
  a.out_a = out_a;
  a.out_b = out_b;
  ProfScope prof("score_fuse", s, 0.0,
                 (double)B * ((double)(ka + kb) * 12.0 + (side_a ? kb * 4.0 : 0.0) + (side_b ? ka * 4.0 : 0.0) + k_out * 20.0));
  hipLaunchKernelGGL(score_fuse_kernel, dim3((unsigned)B), dim3(FTHREADS), 0, s, a);
  SR_LAUNCH_CHECK();
}

void launch_score_rows(const half_t* corpus, int ld, int64_t n_rows, const uint8_t* live,
                       const half_t* qn, const int64_t* rows, int B, int K, int64_t row_offset,
                       float* out, hipStream_t s) {
  SR_CHECK(B >= 0 && K >= 0, "score_rows: negative shape");
  SR_CHECK(ld > 0 && ld % 64 == 0, "score_rows: row stride must be a multiple of 64");
  if (B == 0 || K == 0) return;
  SR_CHECK(corpus && live && qn && rows && out, "score_rows: null buffer");
  ProfScope prof("score_rows", s, 2.0 * B * K * ld, (double)B * K * (ld * 2.0 + 12.0));
  hipLaunchKernelGGL(score_rows_kernel, dim3((unsigned)ceil_div(K, RTHREADS / 64), (unsigned)std::min(B, 65535)),
                     dim3(RTHREADS), 0, s, corpus, ld, n_rows, live, qn, rows, B, K, row_offset, out);
  SR_LAUNCH_CHECK();
}

}  // namespace sr
