// K6 mmr_rerank: maximal-marginal-relevance diversification of a query's top-K candidates
// (graphiti maximal_marginal_relevance, graphiti_core/search/search_utils.py:1884-1922, plus the
// classical greedy form).  One workgroup (8 waves) per query:
//   1. resolve the K <= 128 candidate rows through an index (the store's rows, or an explicit
//      B x K x ld buffer); an index < 0 or >= n_rows is a missing candidate: never dereferenced,
//      staged as a zero row, masked out of every maximum and never output
//   2. Gram matrix G = C . C^T (fp32 accumulate, v_mfma_f32_16x16x32_f16) over K padded up to a
//      multiple of 16: the rows are gathered from HBM in 64-column stages (KP x 64 fp16, 128-byte
//      LDS rows with k_search.hip's 16-byte chunk swizzle, two buffers: the loads of stage t + 1
//      are in flight while stage t multiplies); wave w owns the 16-row block w and all KP / 16
//      column blocks (<= 8 accumulators)
//   3. G stays in LDS (row stride KP + 1 floats: row- and column-wise walks are conflict-free)
//   4. SR_MMR_ONEPASS: m_i = max(0, max_{j != i} G_ij), score_i = lambda rel_i + (lambda - 1) m_i,
//      rank by counting on the key (score desc, position asc), keep score >= min_score, rank < k_out
//      SR_MMR_GREEDY: wave 0 runs the selection loop over G in LDS (running maxima in registers,
//      64-bit key argmax by wave shuffles: ties go to the lower position)
// LDS at K = 128: G 128 x 129 x 4 = 66,048 B + 2 stages x 16 KiB + ~3 KiB of per-candidate state
// = ~102 KB of the CU's 160 KB.  rel comes from the caller (the scan's similarities) or, with a
// query row, from an fp32 dot of the fp16 rows (one wave per candidate).
#include "sr_common.h"
#include "sr_kernels.h"

namespace sr {

namespace {

constexpr int MTHREADS = 512;  // 8 waves
constexpr int MBK = 64;        // columns (fp16) per stage
constexpr int MMAXK = SR_MMR_MAX_CAND;

__device__ __forceinline__ int mmr_swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

__device__ __forceinline__ half8 mmr_frag(const half_t* tile, int row, int chunk) {
  return *reinterpret_cast<const half8*>(tile + row * MBK + mmr_swz(row, chunk) * 8);
}

struct MmrArgs {
  const half_t* rows;       // candidate rows (fp16, ld halfs each)
  int64_t ld, n_rows;
  const int64_t* cand_rows; // [B][K] row ids (+ row_offset, < 0 missing) or null: row b K + i
  int64_t row_offset;
  const int32_t* n_cand;    // explicit buffer: valid candidates per query (null = K)
  const float* rel;         // [B][K] relevance, or null: computed from qn
  const half_t* qn;         // [B][ld] normalised queries (rel == null)
  int K, k_out, mode;
  float lambda, min_score;
  float* out_score;         // [B][k_out]
  float* out_sim;           // [B][k_out] or null
  int32_t* out_index;       // [B][k_out] candidate positions, or null
  int64_t* out_rows;        // [B][k_out] cand_rows of the kept candidates, or null
};

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(MTHREADS, 1) void mmr_rerank_kernel(MmrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mmr_smem[];
  __shared__ int64_t ridx[MMAXK];   // resolved row (valid candidates only)
  __shared__ float relv[MMAXK], score[MMAXK];
  __shared__ int valid[MMAXK], slot[MMAXK];

  const int K = a.K, KP = (K + 15) & ~15, T = KP >> 4, GLD = KP + 1;
  float* G = reinterpret_cast<float*>(mmr_smem);
  // (G's KP * GLD floats rounded up to 16 bytes, then the two stage buffers)
  half_t* stage = reinterpret_cast<half_t*>(mmr_smem + ((KP * GLD * 4 + 15) & ~15));

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ld = a.ld;

  // 1. candidate index
  if (tid < MMAXK) {
    bool ok = false;
    int64_t r = 0;
    if (tid < K) {
      if (a.cand_rows) {
        const int64_t raw = a.cand_rows[(int64_t)b * K + tid];
        r = raw - a.row_offset;
        ok = raw >= 0 && r >= 0 && r < a.n_rows;
      } else {
        const int nc = a.n_cand ? a.n_cand[b] : K;
        r = (int64_t)b * K + tid;
        ok = tid < nc && r < a.n_rows;
      }
    }
    valid[tid] = ok ? 1 : 0;
    ridx[tid] = ok ? r : 0;
    relv[tid] = (ok && a.rel) ? a.rel[(int64_t)b * K + tid] : 0.f;
    slot[tid] = -1;
  }
  __syncthreads();

  // relevance from the query row: fp32 dot of the fp16 rows, one wave per candidate
  if (!a.rel) {
    const half_t* q = a.qn + (int64_t)b * ld;
    for (int i = wave; i < K; i += MTHREADS / 64) {
      if (!valid[i]) continue;
      const half_t* x = a.rows + ridx[i] * ld;
      float acc = 0.f;
      for (int64_t c = lane * 8; c < ld; c += 64 * 8) {
        const half8 xv = *reinterpret_cast<const half8*>(x + c);
        const half8 qv = *reinterpret_cast<const half8*>(q + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf((float)qv[e], (float)xv[e], acc);
      }
      acc = wave_sum(acc);
      if (lane == 0) relv[i] = acc;
    }
  }

  // 2. Gram matrix.  A stage is KP rows x 8 chunks of 16 bytes: <= 2 chunks per thread.
  const int nk = (int)(ld / MBK);
  const int npiece = KP * 8;
  half8 st[2];
  auto load = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = tid + i * MTHREADS;
      half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (p < npiece) {
        const int row = p >> 3, c = p & 7;
        if (valid[row])
          v = *reinterpret_cast<const half8*>(a.rows + ridx[row] * ld + (int64_t)kt * MBK + c * 8);
      }
      st[i] = v;
    }
  };
  auto store = [&](int buf) {
    half_t* tile = stage + buf * (KP * MBK);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = tid + i * MTHREADS;
      if (p < npiece) {
        const int row = p >> 3, c = p & 7;
        *reinterpret_cast<half8*>(tile + row * MBK + mmr_swz(row, c) * 8) = st[i];
      }
    }
  };

  float4v acc[8];
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) acc[ct] = float4v{0.f, 0.f, 0.f, 0.f};

  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load(kt + 1);
    if (wave < T) {
      const half_t* tile = stage + cur * (KP * MBK);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int chunk = (lane >> 4) + 4 * s;
        const half8 fa = mmr_frag(tile, wave * 16 + (lane & 15), chunk);
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {
          if (ct < T) {
            const half8 fb = mmr_frag(tile, ct * 16 + (lane & 15), chunk);
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, fb, acc[ct], 0, 0, 0);
          }
        }
      }
    }
    // (buffer cur ^ 1 was last read in iteration kt - 1, before that iteration's barrier)
    if (kt + 1 < nk) store(cur ^ 1);
    __syncthreads();
  }

  // 3. acc[ct][r] = G[16 wave + 4 (lane >> 4) + r][16 ct + (lane & 15)]
  if (wave < T) {
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) {
      if (ct < T) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          G[(wave * 16 + 4 * (lane >> 4) + r) * GLD + ct * 16 + (lane & 15)] = acc[ct][r];
      }
    }
  }
  __syncthreads();

  const float lam = a.lambda, lam1 = a.lambda - 1.f;
  const int k_out = a.k_out;
  const int64_t ob = (int64_t)b * k_out;

  if (a.mode == SR_MMR_ONEPASS) {
    // 4a. row maxima without the diagonal, clamped at 0 (a wave per row), then the scores
    for (int i = wave; i < K; i += MTHREADS / 64) {
      float m = 0.f;
      for (int j = lane; j < K; j += 64)
        if (j != i && valid[j]) m = fmaxf(m, G[i * GLD + j]);
      m = wave_max(m);
      if (lane == 0) score[i] = lam * relv[i] + lam1 * m;
    }
    __syncthreads();
    // rank by counting on (score desc, position asc); the kept candidates are a prefix of that order
    if (tid < K && valid[tid]) {
      const float s = score[tid];
      int rank = 0;
      for (int j = 0; j < K; ++j) {
        const float sj = score[j];
        rank += (valid[j] && (sj > s || (sj == s && j < tid))) ? 1 : 0;
      }
      if (s >= a.min_score && rank < k_out) slot[rank] = tid;
    }
    __syncthreads();
    if (tid < k_out) {
      const int i = slot[tid];
      a.out_score[ob + tid] = i >= 0 ? score[i] : -INFINITY;
      if (a.out_sim) a.out_sim[ob + tid] = i >= 0 ? relv[i] : -INFINITY;
      if (a.out_index) a.out_index[ob + tid] = i;
      if (a.out_rows) a.out_rows[ob + tid] = i >= 0 ? a.cand_rows[(int64_t)b * K + i] : -1;
    }
    return;
  }

  // 4b. greedy selection, wave 0: lane owns candidates lane and lane + 64
  if (wave != 0) return;
  float cur[2] = {0.f, 0.f}, rl[2];
  bool open[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = lane + 64 * h;
    open[h] = i < K && valid[i];
    rl[h] = i < K ? relv[i] : 0.f;
  }
  int t = 0;
  for (; t < k_out; ++t) {
    uint64_t best = 0ull;  // (ordered value << 32 | ~position); 0 = no candidate left
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (open[h]) {
        // (+ 0: a -0 value orders as +0 in the key, so equal values tie by position)
        const uint64_t key = make_key(lam * rl[h] + lam1 * cur[h] + 0.f, (uint32_t)(lane + 64 * h));
        best = key > best ? key : best;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t other = shfl_xor_u64(best, o);
      best = other > best ? other : best;
    }
    if (best == 0ull) break;
    const float val = key_sim(best);
    if (!(val >= a.min_score)) break;
    const int p = (int)key_row(best);
    if (lane == 0) {
      a.out_score[ob + t] = val;
      if (a.out_sim) a.out_sim[ob + t] = relv[p];
      if (a.out_index) a.out_index[ob + t] = p;
      if (a.out_rows) a.out_rows[ob + t] = a.cand_rows[(int64_t)b * K + p];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i == p) open[h] = false;
      if (open[h]) cur[h] = fmaxf(cur[h], G[p * GLD + i]);
    }
  }
  for (int i = t + lane; i < k_out; i += 64) {
    a.out_score[ob + i] = -INFINITY;
    if (a.out_sim) a.out_sim[ob + i] = -INFINITY;
    if (a.out_index) a.out_index[ob + i] = -1;
    if (a.out_rows) a.out_rows[ob + i] = -1;
  }
}

}  // namespace

void mmr_check_args(int B, int K, int k_out, float lambda, int mode) {
  SR_CHECK(B >= 0, "mmr: negative batch");
  SR_CHECK(mode == SR_MMR_ONEPASS || mode == SR_MMR_GREEDY,
           "mmr: mode must be SR_MMR_ONEPASS (0) or SR_MMR_GREEDY (1)");
  SR_CHECK(lambda >= 0.f && lambda <= 1.f, "mmr: lambda must be in [0, 1]");
  SR_CHECK(K >= 1 && K <= SR_MMR_MAX_CAND, "mmr: candidates per query must be in [1, 128]");
  SR_CHECK(k_out >= 1 && k_out <= K, "mmr: k_out must be in [1, candidates per query]");
}

void launch_mmr_rerank(const half_t* rows, int64_t ld, int64_t n_rows, const int64_t* cand_rows,
                       int64_t row_offset, const int32_t* n_cand, const float* rel,
                       const half_t* qn, int B, int K, float lambda, int mode, float min_score,
                       int k_out, float* out_score, float* out_sim, int32_t* out_index,
                       int64_t* out_rows, hipStream_t s) {
  mmr_check_args(B, K, k_out, lambda, mode);
  SR_CHECK(ld > 0 && ld % MBK == 0, "mmr: padded dim must be a multiple of 64");
  SR_CHECK(rel != nullptr || qn != nullptr, "mmr: relevance or query rows required");
  SR_CHECK(out_rows == nullptr || cand_rows != nullptr, "mmr: out_rows needs cand_rows");
  if (B == 0) return;
  const int KP = (K + 15) & ~15;
  const size_t smem = (size_t)((KP * (KP + 1) * 4 + 15) & ~15) + (size_t)2 * KP * MBK * sizeof(half_t);
  // (per launch: the attribute belongs to the current device's copy of the kernel)
  SR_HIP(hipFuncSetAttribute((const void*)mmr_rerank_kernel,
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             MMAXK * (MMAXK + 1) * 4 + 2 * MMAXK * MBK * 2));
  MmrArgs a;
  a.rows = rows;
  a.ld = ld;
  a.n_rows = n_rows;
  a.cand_rows = cand_rows;
  a.row_offset = row_offset;
  a.n_cand = n_cand;
  a.rel = rel;
  a.qn = qn;
  a.K = K;
  a.k_out = k_out;
  a.mode = mode;
  a.lambda = lambda;
  a.min_score = min_score;
  a.out_score = out_score;
  a.out_sim = out_sim;
  a.out_index = out_index;
  a.out_rows = out_rows;
  const double rows_b = (double)B * K * (double)ld;
  ProfScope prof("mmr_rerank", s, 2.0 * rows_b * K + (rel ? 0.0 : 2.0 * rows_b),
                 rows_b * 2.0 + (double)B * K * 12.0 + (double)B * k_out * 16.0);
  hipLaunchKernelGGL(mmr_rerank_kernel, dim3((unsigned)B), dim3(MTHREADS), smem, s, a);
  SR_LAUNCH_CHECK();
}

}  // namespace sr
