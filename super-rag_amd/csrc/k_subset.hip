// K1g subset_scan: exact cosine scores of per-query ROW LISTS (pre-filtered search: the chat_id /
// indexer filters of context/context.py:74-111 resolved to posting lists on the host), written as
// top-k keys into the store's per-query candidate lists; the unchanged K2 (topk_select) finishes.
//
//   * a GROUP is up to 16 queries of one query block that name the same list (16 = one MFMA column
//     tile); a work item is (group, 512-row chunk of the group's list), one 512-thread workgroup:
//     wave w owns 64 of the chunk's rows as 4 blocks of 16 in the A-fragment layout of
//     v_mfma_f32_16x16x32_f16 (lane (c, g) holds row c, dims 32 j + 8 g .. + 8 of slice j: the
//     layout cosine_stream uses), loaded by per-lane global_load_dwordx4 straight from the gathered
//     rows, one slice ahead of the MFMAs; the same 32-dim slices in the same order as cosine_scan,
//     fp32 accumulation
//   * the group's queries sit in LDS for the whole item (16 x ld fp16, 16-byte chunks XOR-swizzled
//     by the query's low 3 bits) while that is at most 64 KiB (ld <= 2048); wider rows read their B
//     fragments from the L2-resident query block instead
//   * key positions are deterministic: list position i of a pass that covers positions
//     [pass0, pass0 + pass_rows) goes to slot head + (i - pass0) of every query of the group (head =
//     0 in the first pass, k afterwards: the k winners so far stay at the head, subset_prep zeroes
//     what is left of the head and sets cnt).  No atomics, no dependence on scheduling
//   * a lane past the end of the list or the pass neither reads a row nor writes a key; a row id
//     outside [0, n_rows) is never turned into an address and leaves a zero key
//   * items are laid out [list][chunk][group of the list] and item = (block % 8) * (grid / 8) +
//     block / 8, so the groups that share a chunk run side by side on ONE XCD and all but the first
//     read the chunk's rows from that XCD's L2
#include "sr_common.h"
#include "sr_kernels.h"

namespace sr {

namespace {

constexpr int SUB_RB = 4;                       // 16-row blocks per wave
constexpr int SUB_THREADS = 512;                // 8 waves
constexpr int SUB_CHUNK = 8 * SUB_RB * 16;      // list rows per work item (512)
constexpr int SUB_QLDS_MAX_LD = 2048;           // 16 x ld fp16 <= 64 KiB
constexpr uint32_t SUB_NOROW = 0xffffffffu;

static_assert(SUB_CHUNK == SR_SUBSET_CHUNK, "sr_kernels.h names the chunk size the host cuts lists by");

// per query of the block: rows of its list inside the pass; first pass: cnt = that; later passes:
// a query with rows in the pass keeps its winners, gets zero keys up to slot k and cnt = k + rows
__global__ void subset_prep_kernel(const int32_t* __restrict__ q_list,
                                   const int64_t* __restrict__ list_off, int64_t pass0,
                                   int pass_rows, int k, uint64_t* __restrict__ cand, int cap,
                                   int* __restrict__ cnt) {
  const int q = blockIdx.x;
  const int l = q_list[q];
  const int64_t len = list_off[l + 1] - list_off[l];
  int64_t n = len - pass0;
  n = n < 0 ? 0 : (n > pass_rows ? pass_rows : n);
  if (pass0 == 0) {
    if (threadIdx.x == 0) cnt[q] = (int)n;
    return;
  }
  if (n == 0) return;
  const int have = min(max(cnt[q], 0), k);
  __syncthreads();  // (every thread has read cnt[q] before thread 0 replaces it)
  for (int i = have + threadIdx.x; i < k; i += blockDim.x) cand[(int64_t)q * cap + i] = 0ull;
  if (threadIdx.x == 0) cnt[q] = k + (int)n;
}

template <bool QLDS>
__global__ __launch_bounds__(SUB_THREADS, 1) void subset_scan_kernel(
    const half_t* __restrict__ corpus, int ld, int64_t n_rows, const half_t* __restrict__ Q,
    const int32_t* __restrict__ items, int n_items, const int32_t* __restrict__ grp_q,
    const int32_t* __restrict__ grp_list, const int64_t* __restrict__ list_off,
    const int64_t* __restrict__ list_rows, int64_t pass0, int pass_rows, int head,
    uint64_t* __restrict__ cand, int cap) {
  extern __shared__ __attribute__((aligned(16))) half_t qlds[];  // QLDS: 16 x ld halfs

  const int per_xcd = (int)(gridDim.x >> 3);
  const int item = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
  if (item >= n_items) return;  // (whole workgroup)
  const int grp = items[2 * item];
  const int64_t i0 = pass0 + items[2 * item + 1];  // list position of the chunk's first row
  const int l = grp_list[grp];
  const int64_t off = list_off[l];
  const int64_t len = list_off[l + 1] - off;
  const int64_t pend = len < pass0 + pass_rows ? len : pass0 + pass_rows;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int NS = ld >> 5;
  const int qi = grp_q[grp * 16 + c];  // the lane's query column (-1: none)

  if constexpr (QLDS) {
    const int chunks = ld >> 3;
    for (int i = tid; i < 16 * chunks; i += SUB_THREADS) {
      const int q = i / chunks, ch = i - q * chunks;
      const int src = grp_q[grp * 16 + q];
      half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (src >= 0) v = *reinterpret_cast<const half8*>(Q + (int64_t)src * ld + ch * 8);
      *reinterpret_cast<half8*>(qlds + q * ld + ((ch ^ (q & 7)) * 8)) = v;
    }
    __syncthreads();
  }
  const int64_t iw = i0 + wave * 64;  // the wave's first list position
  if (iw >= pend) return;             // (after the only barrier)

  // the lane's rows: block rb, row c -> list position iw + 16 rb + c
  const half_t* rp[SUB_RB];
  uint32_t rrow[SUB_RB];
#pragma unroll
  for (int rb = 0; rb < SUB_RB; ++rb) {
    const int64_t i = iw + 16 * rb + c;
    int64_t r = -1;
    if (i < pend) r = list_rows[off + i];
    const bool ok = r >= 0 && r < n_rows && r < (int64_t)SUB_NOROW;
    rrow[rb] = ok ? (uint32_t)r : SUB_NOROW;
    rp[rb] = ok ? corpus + r * ld + 8 * g : nullptr;
  }
  const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  auto load_a = [&](int rb, int j) {
    return rp[rb] ? *reinterpret_cast<const half8*>(rp[rb] + 32 * j) : zero;
  };
  auto load_b = [&](int j) {
    if constexpr (QLDS) {
      return *reinterpret_cast<const half8*>(qlds + c * ld + (((4 * j + g) ^ (c & 7)) * 8));
    } else {
      return qi >= 0 ? *reinterpret_cast<const half8*>(Q + (int64_t)qi * ld + 32 * j + 8 * g) : zero;
    }
  };

  float4v acc[SUB_RB];
  half8 a[SUB_RB], an[SUB_RB];
#pragma unroll
  for (int rb = 0; rb < SUB_RB; ++rb) {
    acc[rb] = float4v{0.f, 0.f, 0.f, 0.f};
    a[rb] = load_a(rb, 0);
  }
  half8 b = load_b(0);
  for (int j = 0; j < NS; ++j) {
    const int jn = j + 1 < NS ? j + 1 : j;  // (the last step re-reads its own slice: in bounds)
    const half8 bn = load_b(jn);
#pragma unroll
    for (int rb = 0; rb < SUB_RB; ++rb) an[rb] = load_a(rb, jn);
#pragma unroll
    for (int rb = 0; rb < SUB_RB; ++rb)
      acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[rb], b, acc[rb], 0, 0, 0);
#pragma unroll
    for (int rb = 0; rb < SUB_RB; ++rb) a[rb] = an[rb];
    b = bn;
  }

  // acc[rb][r] = sim(list position iw + 16 rb + 4 g + r, query column c); that position's row id
  // is held by lane 4 g + r
#pragma unroll
  for (int rb = 0; rb < SUB_RB; ++rb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t row = (uint32_t)__shfl((int)rrow[rb], 4 * g + r, 64);
      const int64_t i = iw + 16 * rb + 4 * g + r;
      if (qi >= 0 && i < pend)
        cand[(int64_t)qi * cap + head + (i - pass0)] =
            row != SUB_NOROW ? make_key(acc[rb][r], row) : 0ull;
    }
}

}  // namespace

void launch_subset_prep(const int32_t* q_list, const int64_t* list_off, int64_t pass0,
                        int pass_rows, int B, int k, uint64_t* cand, int cap, int* cnt,
                        hipStream_t s) {
  if (B <= 0) return;
  hipLaunchKernelGGL(subset_prep_kernel, dim3(B), dim3(256), 0, s, q_list, list_off, pass0,
                     pass_rows, k, cand, cap, cnt);
  SR_LAUNCH_CHECK();
}

void launch_subset_scan(const half_t* corpus, int ld, int64_t n_rows, const half_t* Q,
                        const int32_t* items, int n_items, const int32_t* grp_q,
                        const int32_t* grp_list, const int64_t* list_off, const int64_t* list_rows,
                        int64_t pass0, int pass_rows, int head, uint64_t* cand, int cap,
                        double query_rows, double group_rows, hipStream_t s) {
  SR_CHECK(ld > 0 && ld % 64 == 0, "subset_scan: padded dim must be a multiple of 64");
  SR_CHECK(pass_rows > 0 && head >= 0 && head + pass_rows <= cap,
           "subset_scan: a pass must fit the candidate list");
  if (n_items <= 0) return;
  const dim3 grid((unsigned)round_up(n_items, 8));
  // algorithmic: one dot product per (query, row of its list); every group gathers its rows once
  ProfScope prof("subset_scan", s, 2.0 * query_rows * ld,
                 group_rows * (ld * 2.0 + 8.0) + query_rows * 8.0);
  if (ld <= SUB_QLDS_MAX_LD)
    hipLaunchKernelGGL((subset_scan_kernel<true>), grid, dim3(SUB_THREADS),
                       (size_t)16 * ld * sizeof(half_t), s, corpus, ld, n_rows, Q, items, n_items,
                       grp_q, grp_list, list_off, list_rows, pass0, pass_rows, head, cand, cap);
  else
    hipLaunchKernelGGL((subset_scan_kernel<false>), grid, dim3(SUB_THREADS), 0, s, corpus, ld,
                       n_rows, Q, items, n_items, grp_q, grp_list, list_off, list_rows, pass0,
                       pass_rows, head, cand, cap);
  SR_LAUNCH_CHECK();
}

}  // namespace sr
