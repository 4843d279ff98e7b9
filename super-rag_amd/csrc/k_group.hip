// K2g group_collapse / group_mask: grouped search (Qdrant search_groups, Milvus group_by_field): the
// k best DISTINCT groups of a query with the group_size best rows of each, exact.
//
// The walk (include/super_rag_mi355x.h): over the eligible rows in (similarity desc, row asc) order a
// row is kept when its group holds fewer than group_size kept rows and the group is already kept or
// fewer than k groups are.  The kept groups are therefore the first k groups by the position of
// their best row, and the kept rows the first group_size rows of each: no sequential pass is needed.
//
// group_collapse, one workgroup (8 waves) per query, over N <= 2048 slots (the k_cand list that
// search_dev / topk_select wrote plus, in a continuation round, the rows carried from earlier rounds):
//   1. slot -> make_key(sim, row), 0 for a missing entry (row < 0 or outside [0, n_rows): never
//      dereferenced); bitonic_sort_desc: position p = rank in the walk order, the zeros at the end
//   2. second sort on ~(group key << 11 | position): ascending (group key, position); the group key
//      is the id for g >= 0 and 2^32 | row for an ungrouped row (g == -1), a group of its own
//   3. in that order a row's rank inside its group is the length of the run before it (looked back
//      over at most SR_GROUP_MAX_SIZE entries) and rank 0 marks the group's best row
//   4. block prefix sum of the rank-0 flags in POSITION order = the group's ordinal; a row is kept
//      when its rank < group_size and its group's ordinal < k, and goes to slot ordinal group_size + rank
//   5. block prefix sum of the kept groups in GROUP KEY order compacts the found list
//      (group key << 1 | full), ascending: the state group_mask searches
// A group is full when it holds group_size kept rows or is an ungrouped row (it cannot grow).
// complete = the candidate list was not full (the eligible rows are exhausted) or k groups were
// found and every one is full.  LDS: 2 x 2048 x 8 B keys + 2 x 2048 x 2 B + 2 x 2048 B = 44 KiB.
//
// group_mask, grid over the rows, one query: out[row] = base[row] && keep(group key of row), keep
// by binary search of the found list staged in LDS (<= 1024 x 8 B): a found group keeps its rows
// while it is not full; a group not found keeps them in open mode (fewer than k groups found) only.
#include <algorithm>

#include "sr_common.h"
#include "sr_kernels.h"
#include "sr_topk.h"

namespace sr {

namespace {

constexpr int GTHREADS = 512;             // 8 waves
constexpr int GMAXN = 2 * SR_MAX_TOPK;    // slots: candidate list + carried rows
constexpr int GPOS_BITS = 11;             // position < 2048
constexpr uint64_t GPOS_MASK = (1ull << GPOS_BITS) - 1;

struct GroupArgs {
  const float* cand_sims;     // [B][K]
  const int64_t* cand_rows;   // [B][K] row + row_offset, -1 past the end
  int K;
  const float* carry_sims;    // [B][C] rows kept by earlier rounds (same form), or null
  const int64_t* carry_rows;
  int C;
  int N;                      // power of two >= K + C, <= GMAXN
  int64_t row_offset, n_rows;
  const int32_t* group;       // [n_rows]
  int k, gs;
  float* out_sim;             // [B][k gs]
  int64_t* out_rows;          // [B][k gs]
  int32_t* out_group;         // [B][k]
  int32_t* n_groups;          // [B]
  int32_t* complete;          // [B]
  uint64_t* found;            // [B][k] ascending (group key << 1 | full), ~0 past n_groups
  float* next_sims;           // [B][k gs] the rows of full groups (-1 elsewhere), or null
  int64_t* next_rows;
};

__device__ __forceinline__ uint64_t group_key_of(int32_t g, uint32_t row) {
  return g >= 0 ? (uint64_t)(uint32_t)g : ((1ull << 32) | (uint64_t)row);
}

// out[i] = flag[0] + .. + flag[i - 1] for i < n (n <= 4 blockDim.x); returns the total
__device__ int block_scan_excl(const uint8_t* flag, uint16_t* out, int n, int* wsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int f[4], s = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = 4 * tid + e;
    f[e] = i < n ? (int)flag[i] : 0;
    s += f[e];
  }
  int inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < GTHREADS / 64; ++w) {
    base += w < wave ? wsum[w] : 0;
    total += wsum[w];
  }
  int run = base + inc - s;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = 4 * tid + e;
    if (i < n) out[i] = (uint16_t)run;
    run += f[e];
  }
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(GTHREADS, 1) void group_collapse_kernel(GroupArgs a) {
  __shared__ uint64_t pos_key[GMAXN];   // walk order: make_key(sim, row) descending
  __shared__ uint64_t grp_ord[GMAXN];   // ~(group key << 11 | position) descending
  __shared__ uint16_t ord[GMAXN];       // position -> rank-0 flags before it (group ordinal)
  __shared__ uint16_t fidx[GMAXN];      // group order -> kept groups before it
  __shared__ uint8_t rnk[GMAXN];        // position -> rank inside the group (capped)
  __shared__ uint8_t flg[GMAXN];
  __shared__ int wsum[GTHREADS / 64];
  __shared__ int nvalid, nfull;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = a.K, C = a.C, N = a.N, k = a.k, gs = a.gs;

  // 1. keys in walk order
  for (int i = tid; i < N; i += GTHREADS) {
    int64_t raw = -1;
    float sim = 0.f;
    if (i < K) {
      raw = a.cand_rows[(int64_t)b * K + i];
      sim = a.cand_sims[(int64_t)b * K + i];
    } else if (i < K + C) {
      raw = a.carry_rows[(int64_t)b * C + (i - K)];
      sim = a.carry_sims[(int64_t)b * C + (i - K)];
    }
    const int64_t r = raw - a.row_offset;
    const bool ok = raw >= 0 && r >= 0 && r < a.n_rows;
    pos_key[i] = ok ? make_key(sim, (uint32_t)r) : 0ull;
  }
  if (tid == 0) {
    nvalid = 0;
    nfull = 0;
  }
  __syncthreads();
  bitonic_sort_desc(pos_key, N);

  // 2. (group key, position) ascending
  for (int i = tid; i < N; i += GTHREADS) {
    const uint64_t key = pos_key[i];
    uint64_t v = 0ull;
    if (key != 0ull) {
      const uint32_t row = key_row(key);   // < n_rows: checked when the key was formed
      v = ~((group_key_of(a.group[row], row) << GPOS_BITS) | (uint64_t)i);
      if (i == N - 1 || pos_key[i + 1] == 0ull) nvalid = i + 1;
    }
    grp_ord[i] = v;
  }
  __syncthreads();
  bitonic_sort_desc(grp_ord, N);
  const int nv = nvalid;

  // 3. rank inside the group
  for (int j = tid; j < N; j += GTHREADS) {
    if (j < nv) {
      const uint64_t e = ~grp_ord[j];
      const uint64_t gk = e >> GPOS_BITS;
      int r = 0;
      while (r < SR_GROUP_MAX_SIZE && j - r - 1 >= 0 && ((~grp_ord[j - r - 1]) >> GPOS_BITS) == gk) ++r;
      const int p = (int)(e & GPOS_MASK);
      rnk[p] = (uint8_t)r;
      flg[p] = r == 0 ? 1 : 0;
    } else {
      flg[j] = 0;   // positions nv .. N - 1 hold no candidate
    }
  }
  __syncthreads();

  // 4. group ordinals, outputs
  const int total = block_scan_excl(flg, ord, N, wsum);
  const int ng = min(total, k);
  const int64_t ob = (int64_t)b * k * gs;
  for (int i = tid; i < k * gs; i += GTHREADS) {
    a.out_sim[ob + i] = -INFINITY;
    a.out_rows[ob + i] = -1;
    if (a.next_rows) {
      a.next_sims[ob + i] = -INFINITY;
      a.next_rows[ob + i] = -1;
    }
  }
  for (int i = tid; i < k; i += GTHREADS) {
    a.out_group[(int64_t)b * k + i] = -1;
    a.found[(int64_t)b * k + i] = ~0ull;
  }
  __syncthreads();   // (the fills above and the scattered stores below hit the same addresses)
  for (int j = tid; j < N; j += GTHREADS) {
    uint8_t kept_first = 0;
    if (j < nv) {
      const uint64_t e = ~grp_ord[j];
      const uint64_t gk = e >> GPOS_BITS;
      const int p = (int)(e & GPOS_MASK);
      const int r = rnk[p];
      if (r < gs) {
        const int j0 = j - r;   // the group's best row
        const int o = ord[(int)((~grp_ord[j0]) & GPOS_MASK)];
        if (o < k) {
          const bool full = (gk >> 32) != 0 ||
                            (j0 + gs - 1 < nv && ((~grp_ord[j0 + gs - 1]) >> GPOS_BITS) == gk);
          const uint64_t key = pos_key[p];
          const int64_t row = (int64_t)key_row(key) + a.row_offset;
          const int64_t at = ob + (int64_t)o * gs + r;
          a.out_sim[at] = key_sim(key);
          a.out_rows[at] = row;
          if (a.next_rows && full) {
            a.next_sims[at] = key_sim(key);
            a.next_rows[at] = row;
          }
          if (r == 0) {
            a.out_group[(int64_t)b * k + o] = (gk >> 32) != 0 ? -1 : (int32_t)(uint32_t)gk;
            kept_first = 1;
            if (full) atomicAdd(&nfull, 1);
          }
        }
      }
    }
    flg[j] = kept_first;
  }
  __syncthreads();

  // 5. the found list, ascending by group key
  (void)block_scan_excl(flg, fidx, N, wsum);
  for (int j = tid; j < nv; j += GTHREADS) {
    if (flg[j]) {
      const uint64_t gk = (~grp_ord[j]) >> GPOS_BITS;
      const bool full = (gk >> 32) != 0 ||
                        (j + gs - 1 < nv && ((~grp_ord[j + gs - 1]) >> GPOS_BITS) == gk);
      a.found[(int64_t)b * k + fidx[j]] = (gk << 1) | (full ? 1ull : 0ull);
    }
  }
  if (tid == 0) {
    const bool list_full = a.cand_rows[(int64_t)b * K + K - 1] >= 0;
    a.n_groups[b] = ng;
    a.complete[b] = (!list_full || (ng == k && nfull == k)) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void group_mask_kernel(
    const uint8_t* __restrict__ base, const int32_t* __restrict__ group, int64_t n_rows,
    const uint64_t* __restrict__ found, const int32_t* __restrict__ n_groups, int k,
    uint8_t* __restrict__ out) {
  __shared__ uint64_t f[SR_MAX_TOPK];
  const int nf = max(0, min(*n_groups, k));
  for (int i = threadIdx.x; i < nf; i += blockDim.x) f[i] = found[i];
  __syncthreads();
  const bool open = nf < k;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows;
       row += (int64_t)gridDim.x * blockDim.x) {
    uint8_t m = 0;
    if (base[row]) {
      const uint64_t gk = group_key_of(group[row], (uint32_t)row);
      int lo = 0, hi = nf;   // first entry with key >= gk
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((f[mid] >> 1) < gk) lo = mid + 1; else hi = mid;
      }
      const bool hit = lo < nf && (f[lo] >> 1) == gk;
      m = (hit ? (f[lo] & 1ull) == 0 : open) ? 1 : 0;
    }
    out[row] = m;
  }
}

}  // namespace

void group_check_args(int B, int K, int k, int group_size) {
  SR_CHECK(B >= 0, "group: negative batch");
  SR_CHECK(k >= 1 && k <= SR_MAX_TOPK, "group: k (groups) must be in [1, 1024]");
  SR_CHECK(group_size >= 1 && group_size <= SR_GROUP_MAX_SIZE, "group: group_size must be in [1, 8]");
  SR_CHECK(K >= k * group_size && K <= SR_MAX_TOPK,
           "group: candidates per query must be in [k * group_size, 1024]");
}

void launch_group_collapse(const float* cand_sims, const int64_t* cand_rows, int B, int K,
                           const float* carry_sims, const int64_t* carry_rows, int C,
                           int64_t row_offset, const int32_t* group, int64_t n_rows, int k,
                           int group_size, float* out_sim, int64_t* out_rows, int32_t* out_group,
                           int32_t* n_groups, int32_t* complete, uint64_t* found, float* next_sims,
                           int64_t* next_rows, hipStream_t s) {
  group_check_args(B, K, k, group_size);
  SR_CHECK(C >= 0 && C <= SR_MAX_TOPK && (C == 0 || (carry_sims && carry_rows)),
           "group: at most 1024 carried rows");
  SR_CHECK((next_sims == nullptr) == (next_rows == nullptr), "group: next_sims and next_rows go together");
  SR_CHECK(n_rows >= 0 && n_rows <= 0xffffffffLL, "group: row ids must fit 32 bits");
  if (B == 0) return;
  int N = 64;
  while (N < K + C) N <<= 1;
  GroupArgs a;
  a.cand_sims = cand_sims;
  a.cand_rows = cand_rows;
  a.K = K;
  a.carry_sims = C ? carry_sims : nullptr;
  a.carry_rows = C ? carry_rows : nullptr;
  a.C = C;
  a.N = N;
  a.row_offset = row_offset;
  a.n_rows = n_rows;
  a.group = group;
  a.k = k;
  a.gs = group_size;
  a.out_sim = out_sim;
  a.out_rows = out_rows;
  a.out_group = out_group;
  a.n_groups = n_groups;
  a.complete = complete;
  a.found = found;
  a.next_sims = next_sims;
  a.next_rows = next_rows;
  ProfScope prof("group_collapse", s, 0.0,
                 (double)B * ((double)(K + C) * 16.0 + (double)k * group_size * 24.0 + k * 12.0));
  hipLaunchKernelGGL(group_collapse_kernel, dim3((unsigned)B), dim3(GTHREADS), 0, s, a);
  SR_LAUNCH_CHECK();
}

void launch_group_mask(const uint8_t* base, const int32_t* group, int64_t n_rows,
                       const uint64_t* found, const int32_t* n_groups, int k, uint8_t* out,
                       hipStream_t s) {
  SR_CHECK(k >= 1 && k <= SR_MAX_TOPK, "group: k (groups) must be in [1, 1024]");
  if (n_rows <= 0) return;
  const int64_t blocks = std::min<int64_t>(ceil_div(n_rows, 256 * 4), 1024);
  ProfScope prof("group_mask", s, 0.0, (double)n_rows * 6.0);
  hipLaunchKernelGGL(group_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, s, base, group, n_rows,
                     found, n_groups, k, out);
  SR_LAUNCH_CHECK();
}

}  // namespace sr
