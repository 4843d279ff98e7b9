// K9 maxsim: late-interaction (ColBERT / bge-m3 multi-vector) scores of (query, row) pairs over the
// token pool of a MultiVecIndex (multivec.hip; DESIGN.md "Multi-vector retrieval"):
//   score = (1 / Lq) sum_i max_j q_i . d_j      (fp16 operands as stored, fp32 accumulation)
// One workgroup (8 waves) per (query, group of <= 32 candidates of that query):
//   1. the query block (<= 64 tokens x dim fp16) is staged ONCE in LDS, rows of round_up(dim, 128)
//      halfs with the 16-byte chunk swizzle chunk ^ (row & 15) (conflict-free ds_read_b128 of an MFMA
//      fragment: 16 rows x one chunk column land in 16 different bank quads), rows past Lq zero and
//      never read from the caller's buffer
//   2. every candidate's tokens stream from HBM straight into MFMA A operands, 16-byte loads, each
//      token once per query block: wave w owns the 16-token tiles w, w + 8, ... of the candidate; a
//      lane loads chunks 2 g and 2 g + 1 (g = lane >> 4) of every 64-column step of its token, so
//      four lanes cover one 128-byte line, and the query fragment is read with the same column
//      order (a dot product does not care which 8 columns a lane group multiplies, as long as both
//      operands agree).  Four steps (8 loads per lane) form a group; the next group's loads, across
//      tile and candidate boundaries, are in flight while the current one multiplies (two register
//      buffers).  Slots past Ld in the last tile load the last token again (in bounds) and enter
//      the maximum as -inf.
//   3. v_mfma_f32_16x16x32_f16 with A = document tile, B = query sub-tile (<= 4 of 16 tokens):
//      acc[r] = d_{4 g + r} . q_{lane & 15}; the running maximum per query token stays in registers
//      (4 floats per lane), is folded over g by two shuffles at the end of the candidate and over
//      the waves through LDS (two buffers, one barrier per candidate)
//   4. wave 0 sums the <= 64 token maxima by a fixed butterfly, adds the blocks of a longer query
//      in block order and divides by Lq once.  No atomics.
// A pair's arithmetic depends on (Lq, Ld, dim) and the values only: the tile -> wave map, the column
// order and the summation tree are fixed, so its bits do not depend on B, K, the grouping or the
// other candidates.  Queries longer than 64 tokens re-stream the candidates once per 64-token block.
// LDS: 64 x round_up(dim, 128) x 2 B (128 KiB at dim 1024) + 4.5 KiB of static state.
//
// maxsim_kernel<true> is the same kernel over an fp8 pool (SR_DTYPE_FP8_E4M3: a token element x is the
// byte e4m3(256 fp16(x)), a pool row is dim bytes).  Only the candidate loads, their conversion and
// the last scale differ:
//   - a 16-byte load carries 16 columns.  A step is 128 columns: lane group g loads bytes [32 g,
//     32 g + 32) of the step (two loads), so the four lanes of a token still cover one whole 128-byte
//     line; the 8 columns of MFMA m (0 .. 3) of the step are chunk 16 ks + 4 g + m of the row, and the
//     query fragment is read at that chunk.  dim % 128 == 64 ends on a half step of 64 columns: one
//     load of bytes [16 g, 16 g + 16), chunks 16 ks + 2 g + m, m < 2.  Four steps (8 loads per lane,
//     the fp16 kernel's bytes in flight, twice its columns) form a group.
//   - the bytes become MFMA operands in registers by v_cvt_scalef32_pk_f16_fp8 with scale 1: the fp16
//     value of 256 x, exact (every e4m3 value is a normal fp16: the smallest is 2^-9), eight packed
//     conversions per load.  The query stays the caller's fp16.
//   - the factor 2^-8 is applied once, in fp32, to the finished sum (a power of two: exact).
// Everything else, the fp16 instantiation included, is the code above unchanged.
//
// mv_move_kernel, at the end, is the byte mover of the index's in-place compaction (its own comment).
#include <algorithm>
#include <type_traits>

#include "sr_common.h"
#include "sr_kernels.h"

namespace sr {

namespace {

constexpr int MV_THREADS = 512;
constexpr int MV_WAVES = MV_THREADS / 64;
constexpr int MV_QT = 64;     // query tokens per LDS block
constexpr int MV_MAXC = 32;   // candidates per workgroup

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct MvArgs {
  const void* pool;       // [n_tokens][dim] fp16, or e4m3 bytes (maxsim_kernel<true>)
  const int64_t* off;     // [n_rows + 1] first token of each row
  const uint8_t* live;    // [n_rows]
  int64_t n_rows;
  const half_t* q;        // [B][ld_q][dim]
  const int32_t* q_len;   // [B]
  const int64_t* rows;    // [B][K]
  float* out;             // [B][K]
  int ld_q, dim, K, cpw;
};

// eight e4m3 bytes -> the fp16 values of the same numbers, in byte order
__device__ __forceinline__ half8 e4m3x8_to_f16(uint32_t w0, uint32_t w1) {
  const half2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w0, 1.f, false);
  const half2_t b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w0, 1.f, true);
  const half2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w1, 1.f, false);
  const half2_t d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w1, 1.f, true);
  return half8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

template <bool FP8>
__global__ __launch_bounds__(MV_THREADS) void maxsim_kernel(MvArgs a) {
  using Buf = std::conditional_t<FP8, u32x4, half8>;  // one 16-byte load
  extern __shared__ __attribute__((aligned(16))) unsigned char mv_smem[];
  __shared__ int64_t c_off[MV_MAXC];
  __shared__ int c_len[MV_MAXC];
  __shared__ float psum[MV_MAXC];
  __shared__ float red[2][MV_WAVES][MV_QT];
  half_t* qtile = reinterpret_cast<half_t*>(mv_smem);

  const int tid = threadIdx.x, lane = tid & 63, gl = lane >> 4, r16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = a.K, dim = a.dim;
  const int ngrp = (K + a.cpw - 1) / a.cpw;
  const int b = (int)(blockIdx.x / (unsigned)ngrp);
  const int c0 = (int)(blockIdx.x % (unsigned)ngrp) * a.cpw;
  const int C = min(a.cpw, K - c0);
  // (never more query tokens than the caller's rows hold, nor than the documented limit)
  const int Lq = min(min(a.q_len[b], a.ld_q), SR_MV_MAX_QUERY_TOKENS);
  const int64_t ob = (int64_t)b * K + c0;

  if (Lq <= 0) {
    if (tid < C) a.out[ob + tid] = -INFINITY;
    return;
  }
  if (tid < C) {
    const int64_t row = a.rows[ob + tid];
    const bool ok = row >= 0 && row < a.n_rows && a.live[row] != 0;
    const int64_t o = ok ? a.off[row] : 0;
    c_off[tid] = o;
    c_len[tid] = ok ? (int)(a.off[row + 1] - o) : 0;
  }
  __syncthreads();

  // steps of one token row: 64 columns (fp16) or 128 columns plus, at dim % 128 == 64, a half step
  const int nfull = dim >> 7, nk = FP8 ? (dim + 127) >> 7 : dim >> 6, ng = (nk + 3) >> 2, nchunk = dim >> 3;
  const int lds_ld = (dim + 127) & ~127;
  const int nqb = (Lq + MV_QT - 1) / MV_QT;
  int epoch = 0;  // candidates reduced so far: picks the red buffer

  for (int qb = 0; qb < nqb; ++qb) {
    const int rows_q = min(MV_QT, Lq - qb * MV_QT);
    const int nqt = (rows_q + 15) >> 4;
    // 1. stage the query block (every wave is past its last read of the previous one: the barrier
    //    of the previous block's last candidate)
    {
      const half_t* qsrc = a.q + ((int64_t)b * a.ld_q + (int64_t)qb * MV_QT) * dim;
      const int total = nqt * 16 * nchunk;
      for (int p = tid; p < total; p += MV_THREADS) {
        const int row = p / nchunk, ch = p - row * nchunk;
        half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < rows_q) v = *reinterpret_cast<const half8*>(qsrc + (int64_t)row * dim + ch * 8);
        *reinterpret_cast<half8*>(qtile + row * lds_ld + ((ch ^ (row & 15)) << 3)) = v;
      }
    }
    __syncthreads();

    auto tiles_of = [&](int c) { return (__builtin_amdgcn_readfirstlane(c_len[c]) + 15) >> 4; };
    // 16-byte loads of group g of tile t of candidate c: this lane's token, chunks 2 gl, 2 gl + 1
    // of the (<= 4) 64-column steps of the group
    auto load = [&](Buf (&buf)[8], int c, int t, int g) {
      const int len = __builtin_amdgcn_readfirstlane(c_len[c]);
      const int tok = min(t * 16 + r16, len - 1);
      if constexpr (FP8) {
        // bytes [32 gl, 32 gl + 32) of every 128-column step, [16 gl, 16 gl + 16) of a last half step
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
    float4v acc[4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) acc[qi] = float4v{0.f, 0.f, 0.f, 0.f};
    // one MFMA k-step: 8 columns per lane, the query fragment at the same chunk of its row
    auto mfma_chunk = [&](const half8 da, int chunk) {
      const half_t* f = qtile + r16 * lds_ld + ((chunk ^ r16) << 3);
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        if (qi < nqt) {
          const half8 fb = *reinterpret_cast<const half8*>(f + qi * 16 * lds_ld);
          acc[qi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(da, fb, acc[qi], 0, 0, 0);
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
            mfma_chunk(e4m3x8_to_f16(w0[0], w0[1]), chunk);
            mfma_chunk(e4m3x8_to_f16(w0[2], w0[3]), chunk + 1);
            if (full) {
              const u32x4 w1 = buf[2 * u + 1];
              mfma_chunk(e4m3x8_to_f16(w1[0], w1[1]), chunk + 2);
              mfma_chunk(e4m3x8_to_f16(w1[2], w1[3]), chunk + 3);
            }
          }
        } else {
          if (ks < nk) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
              const int chunk = ks * 8 + 2 * gl + s;
              const half_t* f = qtile + r16 * lds_ld + ((chunk ^ r16) << 3);
#pragma unroll
              for (int qi = 0; qi < 4; ++qi) {
                if (qi < nqt) {
                  const half8 fb = *reinterpret_cast<const half8*>(f + qi * 16 * lds_ld);
                  acc[qi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(buf[2 * u + s], fb, acc[qi], 0, 0, 0);
                }
              }
            }
          }
        }
      }
    };

    // this wave's work list: (candidate, tile, group), the next item always one ahead
    int nc = 0, nt = wave, ngi = 0;
    while (nc < C && nt >= tiles_of(nc)) {
      ++nc;
      nt = wave;
    }
    Buf bufA[8], bufB[8];
    int par = 0;
    if (nc < C) load(bufA, nc, nt, ngi);

    for (int c = 0; c < C; ++c, ++epoch) {
      const int len = __builtin_amdgcn_readfirstlane(c_len[c]);
      float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      while (nc == c) {
        const int ct = nt, cg = ngi;
        // advance the look-ahead
        if (++ngi == ng) {
          ngi = 0;
          nt += MV_WAVES;
          while (nc < C && nt >= tiles_of(nc)) {
            ++nc;
            nt = wave;
          }
        }
        if (par == 0) {
          if (nc < C) load(bufB, nc, nt, ngi);
          compute(bufA, cg);
        } else {
          if (nc < C) load(bufA, nc, nt, ngi);
          compute(bufB, cg);
        }
        par ^= 1;
        if (cg == ng - 1) {  // the tile is complete: acc[qi][r] = d_{16 ct + 4 gl + r} . q_{16 qi + r16}
#pragma unroll
          for (int qi = 0; qi < 4; ++qi) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float v = (ct * 16 + 4 * gl + r < len) ? acc[qi][r] : -INFINITY;
              m[qi] = fmaxf(m[qi], v);
            }
            acc[qi] = float4v{0.f, 0.f, 0.f, 0.f};
          }
        }
      }
      // 3. fold over the lane groups, then over the waves through LDS
      float* rb = &red[epoch & 1][0][0];
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        float v = m[qi];
        v = fmaxf(v, __shfl_xor(v, 16, 64));
        v = fmaxf(v, __shfl_xor(v, 32, 64));
        if (gl == 0) rb[wave * MV_QT + qi * 16 + r16] = v;
      }
      __syncthreads();
      // 4. wave 0: the token maxima of this block, summed in a fixed order
      if (wave == 0) {
        float v = -INFINITY;
#pragma unroll
        for (int w = 0; w < MV_WAVES; ++w) v = fmaxf(v, rb[w * MV_QT + lane]);
        const float s = wave_sum(lane < rows_q ? v : 0.f);
        if (lane == 0) {
          const float tot = (qb ? psum[c] : 0.f) + s;
          psum[c] = tot;
          if constexpr (FP8) {  // the operands were 256 d; 2^-8 is exact
            if (qb == nqb - 1) a.out[ob + c] = len > 0 ? tot / (float)Lq * 0.00390625f : -INFINITY;
          } else {
            if (qb == nqb - 1) a.out[ob + c] = len > 0 ? tot / (float)Lq : -INFINITY;
          }
        }
      }
    }
  }
}

// rows of src [n][ld_tok][dim] (len[i] tokens each) -> the pool at off[i] (16-byte copies)
__global__ __launch_bounds__(256) void mv_pack_kernel(const half_t* __restrict__ src,
                                                      const int64_t* __restrict__ off, int ld_tok,
                                                      int dim, half_t* __restrict__ pool) {
  const int64_t i = blockIdx.x;
  const int64_t o = off[i];
  const int64_t nch = (off[i + 1] - o) * (int64_t)(dim >> 3);
  const half8* s = reinterpret_cast<const half8*>(src + i * (int64_t)ld_tok * dim);
  half8* d = reinterpret_cast<half8*>(pool + o * dim);
  for (int64_t p = (int64_t)blockIdx.y * 256 + threadIdx.x; p < nch; p += (int64_t)gridDim.y * 256)
    d[p] = s[p];
}

// the same into an fp8 pool: 16 fp16 values (two 16-byte loads) -> 16 bytes e4m3(256 x), one 16-byte
// store.  |x| > 1.75 saturates at +-448 (e4m3x4 clamps).
__global__ __launch_bounds__(256) void mv_pack_fp8_kernel(const half_t* __restrict__ src,
                                                          const int64_t* __restrict__ off, int64_t ld_tok,
                                                          int dim, uint8_t* __restrict__ pool) {
  const int64_t i = blockIdx.x;
  const int64_t o = off[i];
  const int64_t nch = (off[i + 1] - o) * (int64_t)(dim >> 4);
  const half8* s = reinterpret_cast<const half8*>(src + i * ld_tok * dim);
  u32x4* d = reinterpret_cast<u32x4*>(pool + o * dim);
  for (int64_t p = (int64_t)blockIdx.y * 256 + threadIdx.x; p < nch; p += (int64_t)gridDim.y * 256) {
    const half8 lo = s[2 * p], hi = s[2 * p + 1];
    auto q4 = [](const half8& v, int k) {
      return e4m3x4(256.f * (float)v[k], 256.f * (float)v[k + 1], 256.f * (float)v[k + 2], 256.f * (float)v[k + 3]);
    };
    d[p] = u32x4{q4(lo, 0), q4(lo, 4), q4(hi, 0), q4(hi, 4)};
  }
}

// Compaction move (multivec.hip MultiVecIndex::compact): the kept tokens [t0, t1) of the compacted
// order, each copied from its old pool position to dst + (t - dst_t0) * row_bytes (dst: the pool
// itself with dst_t0 = 0, or a staging buffer with dst_t0 = t0).  old_off / new_off [m] and new_off[m]:
// the first token of every kept row before and after, new_off[0] <= t0 and t1 <= new_off[m].  A wave
// owns whole tokens (grid-stride): one binary search in new_off per token, on wave-uniform values,
// for the last kept row k with new_off[k] <= t (rows without tokens share their successor's offset
// and are passed over), then row_bytes of 16-byte loads and stores, two per lane in flight.  Bytes
// move as they are, whatever the dtype.  The caller guarantees that no source of the launch lies in
// the range it writes.
__global__ __launch_bounds__(256) void mv_move_kernel(const uint8_t* pool, uint8_t* dst, int64_t dst_t0,
                                                      const int64_t* __restrict__ old_off,
                                                      const int64_t* __restrict__ new_off, int64_t m,
                                                      int64_t t0, int64_t t1, int row_bytes) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
  const int nwaves = (int)gridDim.x * 4;
  const int units = row_bytes >> 4;
  for (int64_t t = t0 + wave; t < t1; t += nwaves) {
    int64_t lo = 0, hi = m;  // new_off[lo] <= t < new_off[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (new_off[mid] <= t)
        lo = mid;
      else
        hi = mid;
    }
    const u32x4* s = reinterpret_cast<const u32x4*>(pool + (old_off[lo] + (t - new_off[lo])) * row_bytes);
    u32x4* d = reinterpret_cast<u32x4*>(dst + (t - dst_t0) * row_bytes);
    for (int u = lane; u < units; u += 128) {
      const bool two = u + 64 < units;
      const u32x4 a = s[u];
      u32x4 b = a;
      if (two) b = s[u + 64];
      d[u] = a;
      if (two) d[u + 64] = b;
    }
  }
}

}  // namespace

void maxsim_check_args(int dim, int B, int ld_q, int K) {
  SR_CHECK(dim >= 64 && dim <= 1024 && dim % 64 == 0, "mv: dim must be a multiple of 64, <= 1024");
  SR_CHECK(B >= 0, "mv.score_rows: negative batch");
  SR_CHECK(K >= 1 && K <= SR_MAX_TOPK, "mv.score_rows: K must be in [1, 1024]");
  SR_CHECK(ld_q >= 1, "mv.score_rows: ld_q must be >= 1");
}

void launch_maxsim(const void* pool, int dtype, const int64_t* off, const uint8_t* live, int64_t n_rows,
                   int dim, const half_t* q, const int32_t* q_len, int B, int ld_q,
                   const int64_t* rows, int K, float* out, double tokens_hint, hipStream_t s) {
  maxsim_check_args(dim, B, ld_q, K);
  SR_CHECK(dtype == SR_DTYPE_F16 || dtype == SR_DTYPE_FP8_E4M3, "mv.score_rows: pool dtype");
  if (B == 0) return;
  const bool fp8 = dtype == SR_DTYPE_FP8_E4M3;
  const void* kernel = fp8 ? (const void*)maxsim_kernel<true> : (const void*)maxsim_kernel<false>;
  // candidates per workgroup: about 2048 workgroups (8 per CU) once there are that many pairs
  const int64_t pairs = (int64_t)B * K;
  const int cpw = (int)std::min<int64_t>(std::min<int64_t>(MV_MAXC, K), std::max<int64_t>(1, ceil_div(pairs, 2048)));
  const int64_t grid = (int64_t)B * ceil_div(K, cpw);
  SR_CHECK(grid < (1ll << 31), "mv.score_rows: too many pairs");
  const size_t smem = (size_t)MV_QT * round_up(dim, 128) * sizeof(half_t);
  // (per launch: the attribute belongs to the current device's copy of the kernel)
  SR_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             MV_QT * 1024 * (int)sizeof(half_t)));
  MvArgs a;
  a.pool = pool;
  a.off = off;
  a.live = live;
  a.n_rows = n_rows;
  a.q = q;
  a.q_len = q_len;
  a.rows = rows;
  a.out = out;
  a.ld_q = ld_q;
  a.dim = dim;
  a.K = K;
  a.cpw = cpw;
  // (profiling only: the caller's estimate of the candidate tokens, 32 query tokens assumed)
  ProfScope prof(fp8 ? "maxsim_fp8" : "maxsim", s, 2.0 * tokens_hint * dim * 32.0,
                 tokens_hint * dim * (fp8 ? 1.0 : 2.0) + (double)pairs * 12.0);
  if (fp8)
    hipLaunchKernelGGL(maxsim_kernel<true>, dim3((unsigned)grid), dim3(MV_THREADS), smem, s, a);
  else
    hipLaunchKernelGGL(maxsim_kernel<false>, dim3((unsigned)grid), dim3(MV_THREADS), smem, s, a);
  SR_LAUNCH_CHECK();
}

void launch_mv_pack(const half_t* src, const int64_t* off, int64_t n, int ld_tok, int dim,
                    half_t* pool, hipStream_t s) {
  if (n <= 0) return;
  SR_CHECK(n < (1ll << 31), "mv.add: too many rows in one call");
  const int by = (int)std::min<int64_t>(64, std::max<int64_t>(1, ceil_div((int64_t)ld_tok * (dim >> 3), 256)));
  ProfScope prof("mv_pack", s, 0.0, (double)n * ld_tok * dim * 4.0);
  hipLaunchKernelGGL(mv_pack_kernel, dim3((unsigned)n, (unsigned)by), dim3(256), 0, s, src, off, ld_tok,
                     dim, pool);
  SR_LAUNCH_CHECK();
}

void launch_mv_pack_fp8(const half_t* src, const int64_t* off, int64_t n, int64_t ld_tok, int dim,
                        uint8_t* pool, hipStream_t s) {
  if (n <= 0) return;
  SR_CHECK(n < (1ll << 31), "mv.add: too many rows in one call");
  const int by = (int)std::min<int64_t>(1024, std::max<int64_t>(1, ceil_div(ld_tok * (dim >> 4), 256)));
  ProfScope prof("mv_pack_fp8", s, 0.0, (double)n * ld_tok * dim * 3.0);
  hipLaunchKernelGGL(mv_pack_fp8_kernel, dim3((unsigned)n, (unsigned)by), dim3(256), 0, s, src, off, ld_tok,
                     dim, pool);
  SR_LAUNCH_CHECK();
}

void launch_mv_move(const void* pool, void* dst, int64_t dst_t0, const int64_t* old_off,
                    const int64_t* new_off, int64_t m, int64_t t0, int64_t t1, int row_bytes,
                    hipStream_t s) {
  if (t1 <= t0) return;
  SR_CHECK(m >= 1 && row_bytes >= 64 && row_bytes % 64 == 0, "mv.compact: move arguments");
  int dev = 0, cus = 0;
  SR_HIP(hipGetDevice(&dev));
  SR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  // four tokens per workgroup and pass, eight workgroups per CU at the most
  const int64_t grid = std::min<int64_t>(ceil_div(t1 - t0, 4), (int64_t)std::max(cus, 1) * 8);
  ProfScope prof("mv_move", s, 0.0, (double)(t1 - t0) * row_bytes * 2.0);
  hipLaunchKernelGGL(mv_move_kernel, dim3((unsigned)grid), dim3(256), 0, s,
                     static_cast<const uint8_t*>(pool), static_cast<uint8_t*>(dst), dst_t0, old_off, new_off,
                     m, t0, t1, row_bytes);
  SR_LAUNCH_CHECK();
}

}  // namespace sr
