// Multi-vector index (sr_mv_*; DESIGN.md "Multi-vector retrieval"): the per-token unit vectors of
// every row of a collection (bge-m3's multi-vector / ColBERT output), row-aligned with the store
// like sr_lex.  One token pool [n_tokens][dim] in HBM, fp16 or (SR_DTYPE_FP8_E4M3) the bytes
// e4m3(256 fp16(x)), an int64 offsets array (device copy and host mirror) and live flags; both the
// pool and the per-row arrays grow by doubling.  Every way into an fp8 pool goes through the one
// quantising kernel (launch_mv_pack_fp8), so the stored bytes do not depend on it.  Appends and
// removals finish before they return; scoring (k_multivec.hip) is asynchronous on the caller's
// stream and ordered against them by the completion event, as in the store.  compact() drops the
// tombstoned rows in place, with bounded staging; save() / load() write and read the whole state.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sr_kernels.h"
#include "sr_mv_plan.h"
#include "sr_runtime.h"

namespace sr {

MultiVecIndex::MultiVecIndex(int dim, int device, int dtype) : dim_(dim), device_(device), dtype_(dtype) {
  SR_CHECK(dim >= 64 && dim <= 1024 && dim % 64 == 0, "mv: dim must be a multiple of 64, <= 1024");
  SR_CHECK(dtype == SR_DTYPE_F16 || dtype == SR_DTYPE_FP8_E4M3, "mv: dtype must be SR_DTYPE_F16 or SR_DTYPE_FP8_E4M3");
  DeviceGuard g(device_);
  SR_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  SR_HIP(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
}

MultiVecIndex::~MultiVecIndex() {
  (void)hipSetDevice(device_);
  if (done_) {
    (void)hipEventSynchronize(done_);
    (void)hipEventDestroy(done_);
  }
  if (stream_) {
    (void)hipStreamSynchronize(stream_);
    (void)hipStreamDestroy(stream_);
  }
}

void MultiVecIndex::ensure_capacity(int64_t rows, int64_t tokens, hipStream_t s) {
  if (tokens > cap_tokens_) {
    const int64_t cap = round_up(std::max<int64_t>(tokens, 2 * cap_tokens_), 1024);
    DevBuf np;
    np.reserve((size_t)cap * row_bytes());
    if (n_tokens_ > 0)
      SR_HIP(hipMemcpyAsync(np.p, pool_.p, (size_t)n_tokens_ * row_bytes(), hipMemcpyDeviceToDevice, s));
    SR_HIP(hipStreamSynchronize(s));
    std::swap(pool_.p, np.p);
    std::swap(pool_.bytes, np.bytes);
    cap_tokens_ = cap;
  }
  if (rows > cap_rows_) {
    const int64_t cap = round_up(std::max<int64_t>(rows, 2 * cap_rows_), 256);
    DevBuf no, nl;
    no.reserve((size_t)(cap + 1) * sizeof(int64_t));
    nl.reserve((size_t)cap);
    SR_HIP(hipMemsetAsync(nl.p, 0, (size_t)cap, s));
    SR_HIP(hipMemcpyAsync(no.p, off_host_.data(), (size_t)(n_rows_ + 1) * sizeof(int64_t),
                          hipMemcpyHostToDevice, s));
    if (n_rows_ > 0) SR_HIP(hipMemcpyAsync(nl.p, live_.p, (size_t)n_rows_, hipMemcpyDeviceToDevice, s));
    SR_HIP(hipStreamSynchronize(s));
    std::swap(off_.p, no.p);
    std::swap(off_.bytes, no.bytes);
    std::swap(live_.p, nl.p);
    std::swap(live_.bytes, nl.bytes);
    cap_rows_ = cap;
  }
}

void MultiVecIndex::commit(const std::vector<int64_t>& len, hipStream_t s) {
  const int64_t n = (int64_t)len.size();
  for (int64_t i = 0; i < n; ++i) off_host_.push_back(off_host_.back() + len[i]);
  live_host_.insert(live_host_.end(), (size_t)n, 1);
  SR_HIP(hipMemcpyAsync(off_.as<int64_t>() + n_rows_, off_host_.data() + n_rows_,
                        (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  SR_HIP(hipMemsetAsync(live_.as<uint8_t>() + n_rows_, 1, (size_t)n, s));
  end(s);
  SR_HIP(hipStreamSynchronize(s));
  n_rows_ += n;
  n_live_ += n;
  n_tokens_ = off_host_.back();
}

void MultiVecIndex::add_host(const int64_t* off, const float* vecs, int64_t n, int64_t* first_row) {
  SR_CHECK(n >= 0, "mv.add: negative row count");
  if (first_row) *first_row = n_rows_;
  if (n == 0) return;
  SR_CHECK(off != nullptr, "mv.add: null offsets");
  SR_CHECK(off[0] == 0, "mv.add: off[0] must be 0");
  std::vector<int64_t> len((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    SR_CHECK(off[i + 1] >= off[i], "mv.add: offsets must not decrease");
    len[i] = off[i + 1] - off[i];
    SR_CHECK(len[i] < (1ll << 31), "mv.add: a row holds too many tokens");
  }
  const int64_t T = off[n];
  SR_CHECK(T == 0 || vecs != nullptr, "mv.add: null vectors");
  DeviceGuard g(device_);
  begin(stream_);
  ensure_capacity(n_rows_ + n, n_tokens_ + T, stream_);
  if (T > 0) {
    float* stage;
    half_t* h16;
    int64_t* doff;
    Carve c;
    c.part((size_t)T * dim_, &stage);
    c.part(fp8() ? (size_t)T * dim_ : 0, &h16);
    c.part(fp8() ? 2 : 0, &doff);
    hostio_.carve(c);
    SR_HIP(hipMemcpyAsync(stage, vecs, (size_t)T * dim_ * sizeof(float), hipMemcpyHostToDevice, stream_));
    if (fp8()) {
      // fp32 -> fp16 as the fp16 pool stores it, then add_dev's quantiser over the T tokens as one row
      const int64_t span[2] = {n_tokens_, n_tokens_ + T};
      SR_HIP(hipMemcpyAsync(doff, span, sizeof(span), hipMemcpyHostToDevice, stream_));
      launch_convert_f32_f16(stage, h16, T * dim_, stream_);
      launch_mv_pack_fp8(h16, doff, 1, T, dim_, pool_.as<uint8_t>(), stream_);
      SR_HIP(hipStreamSynchronize(stream_));  // `span` leaves scope
    } else {
      launch_convert_f32_f16(stage, pool_.as<half_t>() + n_tokens_ * dim_, T * dim_, stream_);
    }
  }
  commit(len, stream_);
}

void MultiVecIndex::add_dev(const half_t* vecs, const int32_t* len, int64_t n, int ld_tok,
                            int64_t* first_row, hipStream_t s) {
  SR_CHECK(n >= 0, "mv.add: negative row count");
  SR_CHECK(ld_tok >= 1, "mv.add: ld_tok must be >= 1");
  if (first_row) *first_row = n_rows_;
  if (n == 0) return;
  SR_CHECK(vecs != nullptr && len != nullptr, "mv.add: null buffer");
  DeviceGuard g(device_);
  begin(s);
  std::vector<int32_t> l32((size_t)n);
  SR_HIP(hipMemcpyAsync(l32.data(), len, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  SR_HIP(hipStreamSynchronize(s));
  std::vector<int64_t> l64((size_t)n), off((size_t)n + 1);
  off[0] = n_tokens_;
  for (int64_t i = 0; i < n; ++i) {
    SR_CHECK(l32[i] >= 0 && l32[i] <= ld_tok, "mv.add: a length outside [0, ld_tok]");
    l64[i] = l32[i];
    off[i + 1] = off[i] + l64[i];
  }
  ensure_capacity(n_rows_ + n, off[n], s);
  // the new rows' offsets first: the copy kernel reads them from the device array
  SR_HIP(hipMemcpyAsync(off_.as<int64_t>() + n_rows_, off.data(), (size_t)(n + 1) * sizeof(int64_t),
                        hipMemcpyHostToDevice, s));
  if (fp8())
    launch_mv_pack_fp8(vecs, off_.as<int64_t>() + n_rows_, n, ld_tok, dim_, pool_.as<uint8_t>(), s);
  else
    launch_mv_pack(vecs, off_.as<int64_t>() + n_rows_, n, ld_tok, dim_, pool_.as<half_t>(), s);
  SR_HIP(hipStreamSynchronize(s));  // `off` leaves scope
  commit(l64, s);
}

void MultiVecIndex::remove(const int64_t* rows, int64_t n) {
  SR_CHECK(n >= 0, "mv.remove: negative count");
  if (n == 0) return;
  SR_CHECK(rows != nullptr, "mv.remove: null rows");
  for (int64_t i = 0; i < n; ++i)
    SR_CHECK(rows[i] >= 0 && rows[i] < n_rows_, "mv.remove: row out of range");
  DeviceGuard g(device_);
  begin(stream_);
  for (int64_t i = 0; i < n; ++i) {
    if (!live_host_[(size_t)rows[i]]) continue;
    live_host_[(size_t)rows[i]] = 0;
    --n_live_;
    SR_HIP(hipMemsetAsync(live_.as<uint8_t>() + rows[i], 0, 1, stream_));
  }
  end(stream_);
  SR_HIP(hipStreamSynchronize(stream_));
}

void MultiVecIndex::stats(int64_t* n_rows, int64_t* n_live, int64_t* n_tokens) const {
  if (n_rows) *n_rows = n_rows_;
  if (n_live) *n_live = n_live_;
  if (n_tokens) *n_tokens = n_tokens_;
}

void MultiVecIndex::info(int* dtype, int64_t* pool_bytes) const {
  if (dtype) *dtype = dtype_;
  if (pool_bytes) *pool_bytes = n_tokens_ * (int64_t)row_bytes();
}

// value of an OCP e4m3fn byte (the pool never holds the NaN codes: the quantiser saturates)
static float e4m3_value(uint8_t c) {
  const int e = (c >> 3) & 15, m = c & 7;
  const float a = e == 0 ? std::ldexp((float)m, -9) : std::ldexp((float)(8 + m), e - 10);
  return (c & 0x80) ? -a : a;
}

void MultiVecIndex::get(int64_t row, float* out, int64_t cap, int64_t* n_tok) {
  SR_CHECK(row >= 0 && row < n_rows_, "mv.get: row out of range");
  const int64_t o = off_host_[(size_t)row], T = off_host_[(size_t)row + 1] - o;
  if (n_tok) *n_tok = T;
  SR_CHECK(cap >= 0, "mv.get: negative capacity");
  const int64_t m = std::min(T, cap);
  if (m == 0) return;
  SR_CHECK(out != nullptr, "mv.get: null output");
  DeviceGuard g(device_);
  begin(stream_);
  if (fp8()) {  // the dequantised values e4m3_value / 256, exact in fp32
    std::vector<uint8_t> h((size_t)m * dim_);
    SR_HIP(hipMemcpyAsync(h.data(), pool_.as<uint8_t>() + o * dim_, h.size(), hipMemcpyDeviceToHost, stream_));
    SR_HIP(hipStreamSynchronize(stream_));
    for (size_t i = 0; i < h.size(); ++i) out[i] = e4m3_value(h[i]) * 0.00390625f;
    return;
  }
  std::vector<half_t> h((size_t)m * dim_);
  SR_HIP(hipMemcpyAsync(h.data(), pool_.as<half_t>() + o * dim_, h.size() * sizeof(half_t),
                        hipMemcpyDeviceToHost, stream_));
  SR_HIP(hipStreamSynchronize(stream_));
  for (size_t i = 0; i < h.size(); ++i) out[i] = (float)h[i];
}

void MultiVecIndex::score_rows_dev(const half_t* q, const int32_t* q_len, int B, int ld_q,
                                   const int64_t* rows, int K, float* out, hipStream_t s) {
  maxsim_check_args(dim_, B, ld_q, K);
  if (B == 0) return;
  SR_CHECK(q && q_len && rows && out, "mv.score_rows: null buffer");
  SR_CHECK((int64_t)B * K < (1ll << 31), "mv.score_rows: too many pairs");
  DeviceGuard g(device_);
  begin(s);
  if (n_rows_ == 0) {
    launch_fill_float(out, B * K, -INFINITY, s);
  } else {
    const double avg = (double)n_tokens_ / (double)n_rows_;
    launch_maxsim(pool_.p, dtype_, off_.as<int64_t>(), live_.as<uint8_t>(), n_rows_, dim_, q, q_len, B,
                  ld_q, rows, K, out, avg * B * K, s);
  }
  end(s);
}

void MultiVecIndex::score_rows_host(const float* q, const int32_t* q_len, int B, int ld_q,
                                    const int64_t* rows, int K, float* out) {
  maxsim_check_args(dim_, B, ld_q, K);
  if (B == 0) return;
  SR_CHECK(q && q_len && rows && out, "mv.score_rows: null buffer");
  for (int b = 0; b < B; ++b)
    SR_CHECK(q_len[b] >= 0 && q_len[b] <= SR_MV_MAX_QUERY_TOKENS && q_len[b] <= ld_q,
             "mv.score_rows: q_len must be in [0, min(ld_q, 512)]");
  DeviceGuard g(device_);
  const size_t nq = (size_t)B * ld_q * dim_, no = (size_t)B * K;
  float *dq32, *dout;
  half_t* dq;
  int32_t* dlen;
  int64_t* drows;
  Carve c;
  c.part(nq, &dq32, &dq);
  c.part((size_t)B, &dlen);
  c.part(no, &drows, &dout);
  hostio_.carve(c);
  begin(stream_);
  // only the rows below q_len travel: the rest of the caller's buffer is never read
  SR_HIP(hipMemsetAsync(dq32, 0, nq * sizeof(float), stream_));
  for (int b = 0; b < B; ++b)
    if (q_len[b] > 0)
      SR_HIP(hipMemcpyAsync(dq32 + (size_t)b * ld_q * dim_, q + (size_t)b * ld_q * dim_,
                            (size_t)q_len[b] * dim_ * sizeof(float), hipMemcpyHostToDevice, stream_));
  launch_convert_f32_f16(dq32, dq, (int64_t)nq, stream_);
  SR_HIP(hipMemcpyAsync(dlen, q_len, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
  SR_HIP(hipMemcpyAsync(drows, rows, no * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
  score_rows_dev(dq, dlen, B, ld_q, drows, K, dout, stream_);
  SR_HIP(hipMemcpyAsync(out, dout, no * sizeof(float), hipMemcpyDeviceToHost, stream_));
  SR_HIP(hipStreamSynchronize(stream_));
}

// ---- whole-corpus search ---------------------------------------------------------------------------
// The rows in slabs (sr_mv_plan.h): per slab one scan launch (k_mvscan.hip) into the score scratch
// [B][slab rows] and one selection launch that folds the slab into the running [B, k] list; the last
// selection writes the caller's outputs.  Planning needs the offsets' host mirror only (the tokens of a
// slab size its grid), so nothing is read back.  scan_ holds the scratch and the list; calls on the
// index are ordered by the completion event, so one buffer serves them all.
static void search_check_args(int B, int ld_q, int k, int64_t slab_rows, int64_t row_offset) {
  SR_CHECK(B >= 0, "mv.search: negative batch");
  SR_CHECK(k >= 1 && k <= SR_MAX_TOPK, "mv.search: k must be in [1, 1024]");
  SR_CHECK(ld_q >= 1, "mv.search: ld_q must be >= 1");
  SR_CHECK(slab_rows >= 0, "mv.search: slab_rows must be >= 0 (0: the default)");
  SR_CHECK(row_offset >= 0, "mv.search: row_offset must be >= 0");
}

void MultiVecIndex::search_dev(const half_t* q, const int32_t* q_len, int B, int ld_q, int k,
                               const uint8_t* allow, int64_t slab_rows, int64_t row_offset, float* out_score,
                               int64_t* out_rows, hipStream_t s) {
  search_check_args(B, ld_q, k, slab_rows, row_offset);
  if (B == 0) return;
  SR_CHECK(q && q_len && out_score && out_rows, "mv.search: null buffer");
  SR_CHECK(n_rows_ < 0xffffffffll, "mv.search: the index holds too many rows for a 32-bit key");
  const int64_t slab = std::min(mv_slab_rows(slab_rows, B), std::max<int64_t>(n_rows_, 1));
  DeviceGuard g(device_);
  float* score;
  uint64_t* run_keys;
  int* run_n;
  Carve c;
  c.part((size_t)B * (size_t)slab, &score);
  c.part((size_t)B * k, &run_keys);
  c.part((size_t)B, &run_n);
  scan_.carve(c);
  begin(s);
  const int64_t ns = mv_slab_count(n_rows_, slab);
  for (int64_t i = 0; i < ns; ++i) {
    int64_t r0, r1;
    mv_slab(n_rows_, slab, i, &r0, &r1);
    launch_maxsim_scan(pool_.p, dtype_, off_.as<int64_t>(), live_.as<uint8_t>(), allow, dim_, q, q_len, B, ld_q,
                       r0, r1, off_host_[(size_t)r0], off_host_[(size_t)r1], score, slab, s);
    launch_mv_topk(score, slab, r0, r1 - r0, B, k, i == 0, i == ns - 1, run_keys, run_n, out_score, out_rows,
                   row_offset, s);
  }
  if (ns == 0)  // an empty index: -inf / -1
    launch_mv_topk(score, slab, 0, 0, B, k, true, true, run_keys, run_n, out_score, out_rows, row_offset, s);
  end(s);
}

void MultiVecIndex::search_host(const float* q, const int32_t* q_len, int B, int ld_q, int k,
                                const uint8_t* allow, int64_t slab_rows, float* out_score, int64_t* out_rows) {
  search_check_args(B, ld_q, k, slab_rows, 0);
  if (B == 0) return;
  SR_CHECK(q && q_len && out_score && out_rows, "mv.search: null buffer");
  for (int b = 0; b < B; ++b)
    SR_CHECK(q_len[b] >= 0 && q_len[b] <= SR_MV_MAX_QUERY_TOKENS && q_len[b] <= ld_q,
             "mv.search: q_len must be in [0, min(ld_q, 512)]");
  DeviceGuard g(device_);
  const size_t nq = (size_t)B * ld_q * dim_, no = (size_t)B * k;
  float *dq32, *dscore;
  half_t* dq;
  int32_t* dlen;
  uint8_t* dallow;
  int64_t* drows;
  Carve c;
  c.part(nq, &dq32, &dq);
  c.part((size_t)B, &dlen);
  c.part(allow ? (size_t)n_rows_ : 0, &dallow);
  c.part(no, &dscore, &drows);
  hostio_.carve(c);
  begin(stream_);
  // only the rows below q_len travel: the rest of the caller's buffer is never read
  SR_HIP(hipMemsetAsync(dq32, 0, nq * sizeof(float), stream_));
  for (int b = 0; b < B; ++b)
    if (q_len[b] > 0)
      SR_HIP(hipMemcpyAsync(dq32 + (size_t)b * ld_q * dim_, q + (size_t)b * ld_q * dim_,
                            (size_t)q_len[b] * dim_ * sizeof(float), hipMemcpyHostToDevice, stream_));
  launch_convert_f32_f16(dq32, dq, (int64_t)nq, stream_);
  SR_HIP(hipMemcpyAsync(dlen, q_len, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
  if (allow && n_rows_ > 0)
    SR_HIP(hipMemcpyAsync(dallow, allow, (size_t)n_rows_, hipMemcpyHostToDevice, stream_));
  search_dev(dq, dlen, B, ld_q, k, allow ? dallow : nullptr, slab_rows, 0, dscore, drows, stream_);
  SR_HIP(hipMemcpyAsync(out_score, dscore, no * sizeof(float), hipMemcpyDeviceToHost, stream_));
  SR_HIP(hipMemcpyAsync(out_rows, drows, no * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  SR_HIP(hipStreamSynchronize(stream_));
}

// ---- compaction ----------------------------------------------------------------------------------
// In place: the pool is never duplicated (an index sized to fill the card could not be compacted
// otherwise).  Let t number the kept tokens in their order, which is also their position after the
// compaction, and src(t) >= t be the pool position the token holds now; src(t) - t, the tokens dropped
// before it, never decreases with t.  Tokens with src(t) == t stay where they are: everything before
// the first dropped token.  The rest is cut into chunks [t0, t1) in ascending order; with gap =
// src(t0) - t0, left = the tokens still to place and D = min(stage tokens, kDirectMinBytes of tokens):
//   direct  (gap >= min(D, left))  t1 = t0 + min(gap, left): one launch of the move kernel, pool ->
//           pool.  Every source of the chunk is >= src(t0) = t0 + gap >= t1, so the launch reads
//           nothing it writes, whatever the order of its waves.
//   staged  (otherwise)  t1 = t0 + min(stage tokens, left): the same kernel gathers the chunk into the
//           staging buffer, then a device-to-device copy puts it at [t0, t1).  The gather writes no
//           pool byte, and the copy starts after it in stream order.
// A direct chunk moves its bytes once but is only as long as the gap, a staged one moves them twice
// but is as long as the stage: below kDirectMinBytes per launch the launches of the direct path cost
// more than the second pass of the staged one (an estimate, DESIGN.md: the stage was swept, this
// threshold was not).
// Between chunks the stream order is the only synchronisation, and it is enough: chunk c writes only
// [t0, t1) of the pool, chunk c + 1 reads only src(t) >= t >= t1 for its own t >= t1, positions that
// chunk c (and every earlier one, which wrote below t0) never wrote; they still hold the old bytes.
// The staging buffer is rewritten by a gather only after the copy that read it, again by stream order.
// Chunks are cut by tokens, so a row longer than the stage spans several; the kernel finds a token's
// row in the kept rows' new offsets.
namespace {
struct MoveChunk {
  int64_t t0, t1;
  bool staged;
};

// old_off / new_off: the first token of every kept row before / after (new_off has one more entry, the
// kept tokens), from the first kept row that moves (k0) on
std::vector<MoveChunk> plan_moves(const std::vector<int64_t>& old_off, const std::vector<int64_t>& new_off,
                                  int64_t stage_tok, int64_t direct_tok) {
  std::vector<MoveChunk> plan;
  if (old_off.empty()) return plan;
  const int64_t T = new_off.back();
  size_t k = 0;
  for (int64_t t = new_off[0]; t < T; t = plan.back().t1) {
    while (new_off[k + 1] <= t) ++k;  // the kept row of token t (t < T: k stays in range)
    const int64_t gap = old_off[k] - new_off[k];
    if (gap >= std::min(std::min(stage_tok, direct_tok), T - t))
      plan.push_back({t, t + std::min(gap, T - t), false});
    else
      plan.push_back({t, t + std::min(stage_tok, T - t), true});
  }
  return plan;
}
}  // namespace

void MultiVecIndex::compact(int64_t stage_bytes, int64_t* old_to_new) {
  SR_CHECK(stage_bytes == 0 || stage_bytes >= (int64_t)row_bytes(),
           "mv.compact: stage_bytes must be 0 (the default) or at least one token's bytes");
  const int64_t stage_tok = (stage_bytes ? stage_bytes : kDefaultStageBytes) / (int64_t)row_bytes();
  // the kept rows, the map and the offsets after the compaction
  std::vector<int64_t> keep, noff{0};
  keep.reserve((size_t)n_live_);
  noff.reserve((size_t)n_live_ + 1);
  for (int64_t r = 0; r < n_rows_; ++r) {
    if (live_host_[(size_t)r]) {
      if (old_to_new) old_to_new[r] = (int64_t)keep.size();
      keep.push_back(r);
      noff.push_back(noff.back() + (off_host_[(size_t)r + 1] - off_host_[(size_t)r]));
    } else if (old_to_new) {
      old_to_new[r] = -1;
    }
  }
  const int64_t m = (int64_t)keep.size();
  if (m == n_rows_) return;  // nothing is tombstoned: the identity
  // from the first kept row whose tokens move
  int64_t k0 = 0;
  while (k0 < m && off_host_[(size_t)keep[(size_t)k0]] == noff[(size_t)k0]) ++k0;
  std::vector<int64_t> mold, mnew;
  for (int64_t k = k0; k < m; ++k) mold.push_back(off_host_[(size_t)keep[(size_t)k]]);
  mnew.assign(noff.begin() + k0, noff.end());
  const std::vector<MoveChunk> plan =
      plan_moves(mold, mnew, stage_tok, std::max<int64_t>(1, kDirectMinBytes / (int64_t)row_bytes()));
  int64_t stage_need = 0;
  for (const MoveChunk& c : plan)
    if (c.staged) stage_need = std::max(stage_need, c.t1 - c.t0);

  DeviceGuard g(device_);
  // every allocation before the first byte moves
  DevBuf stage;
  stage.reserve((size_t)stage_need * row_bytes());
  int64_t *dold = nullptr, *dnew = nullptr;
  if (!plan.empty()) {
    Carve c;
    c.part(mold.size(), &dold);
    c.part(mnew.size(), &dnew);
    hostio_.carve(c);
  }
  begin(stream_);
  if (!plan.empty()) {
    const int64_t mm = (int64_t)mold.size();
    const int rb = (int)row_bytes();
    SR_HIP(hipMemcpyAsync(dold, mold.data(), mold.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
    SR_HIP(hipMemcpyAsync(dnew, mnew.data(), mnew.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
    uint8_t* pool = pool_.as<uint8_t>();
    for (const MoveChunk& ch : plan) {
      if (ch.staged) {
        launch_mv_move(pool, stage.p, ch.t0, dold, dnew, mm, ch.t0, ch.t1, rb, stream_);
        SR_HIP(hipMemcpyAsync(pool + ch.t0 * rb, stage.p, (size_t)(ch.t1 - ch.t0) * rb,
                              hipMemcpyDeviceToDevice, stream_));
      } else {
        launch_mv_move(pool, pool, 0, dold, dnew, mm, ch.t0, ch.t1, rb, stream_);
      }
    }
  }
  SR_HIP(hipMemcpyAsync(off_.p, noff.data(), noff.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
  if (m > 0) SR_HIP(hipMemsetAsync(live_.p, 1, (size_t)m, stream_));
  SR_HIP(hipMemsetAsync(live_.as<uint8_t>() + m, 0, (size_t)(n_rows_ - m), stream_));
  end(stream_);
  SR_HIP(hipStreamSynchronize(stream_));  // finished on return; the host vectors leave scope
  off_host_ = noff;
  live_host_.assign((size_t)m, 1);
  n_rows_ = m;
  n_live_ = m;
  n_tokens_ = noff.back();
}

// ---- snapshots -----------------------------------------------------------------------------------
// Snapshot format (little endian): "SRMIMVX1", int32 dim, int32 dtype (SR_DTYPE_F16 or
// SR_DTYPE_FP8_E4M3), int64 n_rows, int64 n_tokens, (n_rows + 1) int64 offsets, n_rows bytes of live
// flags, n_tokens x row_bytes pool bytes exactly as held in HBM (fp16 values, or e4m3 bytes; the
// tokens of tombstoned rows included: the snapshot is the state).  Written to "<path>.tmp", fsync'd
// and renamed over <path>, so a crash mid-save leaves the previous snapshot intact.
static constexpr size_t kSnapshotChunkBytes = size_t(16) << 20;  // host buffer the pool streams through

void MultiVecIndex::save(const char* path) {
  DeviceGuard g(device_);
  begin(stream_);
  SR_HIP(hipStreamSynchronize(stream_));
  const std::string tmp = std::string(path) + ".tmp";
  std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
  if (!f) throw Error(SR_ERR_IO, std::string("mv.save: cannot open ") + tmp);
  f.write("SRMIMVX1", 8);
  const int32_t d = dim_, dt = dtype_;
  f.write(reinterpret_cast<const char*>(&d), 4);
  f.write(reinterpret_cast<const char*>(&dt), 4);
  f.write(reinterpret_cast<const char*>(&n_rows_), 8);
  f.write(reinterpret_cast<const char*>(&n_tokens_), 8);
  f.write(reinterpret_cast<const char*>(off_host_.data()), (std::streamsize)((n_rows_ + 1) * sizeof(int64_t)));
  f.write(reinterpret_cast<const char*>(live_host_.data()), (std::streamsize)n_rows_);
  const int64_t step = std::max<int64_t>(1, (int64_t)(kSnapshotChunkBytes / row_bytes()));
  std::vector<uint8_t> buf;
  for (int64_t t = 0; t < n_tokens_ && f; t += step) {
    const int64_t n = std::min(step, n_tokens_ - t);
    buf.resize((size_t)n * row_bytes());
    SR_HIP(hipMemcpyAsync(buf.data(), pool_.as<uint8_t>() + t * row_bytes(), buf.size(),
                          hipMemcpyDeviceToHost, stream_));
    SR_HIP(hipStreamSynchronize(stream_));
    f.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)buf.size());
  }
  f.flush();
  if (!f) {
    f.close();
    (void)std::remove(tmp.c_str());
    throw Error(SR_ERR_IO, std::string("mv.save: write failed for ") + tmp);
  }
  f.close();
  if (!fsync_path(tmp)) throw Error(SR_ERR_IO, std::string("mv.save: fsync failed for ") + tmp);
  if (std::rename(tmp.c_str(), path) != 0)
    throw Error(SR_ERR_IO, std::string("mv.save: cannot rename ") + tmp + " to " + path);
}

// Everything the file says is checked on the host before a device is touched, and no buffer is sized
// by a header field before the file's real size has confirmed it.
MultiVecIndex* MultiVecIndex::load(const char* path, int device) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error(SR_ERR_IO, std::string("mv.load: cannot open ") + path);
  char magic[8];
  f.read(magic, 8);
  if (!f || std::memcmp(magic, "SRMIMVX1", 8) != 0)
    throw Error(SR_ERR_IO, std::string("mv.load: not a multi-vector snapshot: ") + path);
  int32_t d = 0, dt = 0;
  int64_t n = 0, T = 0;
  f.read(reinterpret_cast<char*>(&d), 4);
  f.read(reinterpret_cast<char*>(&dt), 4);
  f.read(reinterpret_cast<char*>(&n), 8);
  f.read(reinterpret_cast<char*>(&T), 8);
  const int64_t lim = int64_t(1) << 40;
  if (!f || d < 64 || d > 1024 || d % 64 != 0 || (dt != SR_DTYPE_F16 && dt != SR_DTYPE_FP8_E4M3) ||
      n < 0 || n > lim || T < 0 || T > lim)
    throw Error(SR_ERR_IO, "mv.load: corrupt header");
  const bool f8 = dt == SR_DTYPE_FP8_E4M3;
  const int64_t rb = (int64_t)d * (f8 ? 1 : 2);
  f.seekg(0, std::ios::end);
  const std::streamoff size = f.tellg();
  const int64_t pool_at = 32 + 8 * (n + 1) + n;
  if (!f || size != (std::streamoff)(pool_at + T * rb))  // (< 2^52: the limits above)
    throw Error(SR_ERR_IO, "mv.load: file size does not match the header (truncated or corrupt)");
  f.seekg(32);
  std::vector<int64_t> off((size_t)n + 1);
  std::vector<uint8_t> live((size_t)n);
  f.read(reinterpret_cast<char*>(off.data()), (std::streamsize)(off.size() * sizeof(int64_t)));
  f.read(reinterpret_cast<char*>(live.data()), (std::streamsize)n);
  if (!f) throw Error(SR_ERR_IO, "mv.load: truncated offsets or live flags");
  if (off[0] != 0 || off[(size_t)n] != T) throw Error(SR_ERR_IO, "mv.load: offsets do not span the pool");
  int64_t n_live = 0;
  for (int64_t i = 0; i < n; ++i) {
    // (as unsigned: a difference of two corrupt offsets must not overflow)
    const uint64_t len = (uint64_t)off[(size_t)i + 1] - (uint64_t)off[(size_t)i];
    if (off[(size_t)i + 1] < off[(size_t)i] || len >= (uint64_t(1) << 31))
      throw Error(SR_ERR_IO, "mv.load: offsets decrease or a row holds 2^31 tokens or more");
    if (live[(size_t)i] > 1) throw Error(SR_ERR_IO, "mv.load: a live flag is neither 0 nor 1");
    n_live += live[(size_t)i];
  }
  const int64_t step = std::max<int64_t>(1, (int64_t)kSnapshotChunkBytes / rb);
  std::vector<uint8_t> buf;
  if (f8) {  // the quantiser saturates and never writes a NaN code; get() and the kernel rely on it
    for (int64_t t = 0; t < T; t += step) {
      buf.resize((size_t)(std::min(step, T - t) * rb));
      f.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)buf.size());
      if (!f) throw Error(SR_ERR_IO, "mv.load: truncated pool");
      for (uint8_t c : buf)
        if ((c & 0x7f) == 0x7f) throw Error(SR_ERR_IO, "mv.load: an fp8 pool holds a NaN code");
    }
    f.seekg((std::streamoff)pool_at);
  }
  MultiVecIndex* x = new MultiVecIndex(d, device, dt);
  try {
    DeviceGuard g(device);
    x->ensure_capacity(n, T, x->stream_);
    for (int64_t t = 0; t < T; t += step) {
      buf.resize((size_t)(std::min(step, T - t) * rb));
      f.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)buf.size());
      if (!f) throw Error(SR_ERR_IO, "mv.load: truncated pool");
      SR_HIP(hipMemcpyAsync(x->pool_.as<uint8_t>() + t * rb, buf.data(), buf.size(), hipMemcpyHostToDevice,
                            x->stream_));
      SR_HIP(hipStreamSynchronize(x->stream_));  // `buf` is refilled
    }
    if (n > 0) {
      SR_HIP(hipMemcpyAsync(x->off_.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice,
                            x->stream_));
      SR_HIP(hipMemcpyAsync(x->live_.p, live.data(), (size_t)n, hipMemcpyHostToDevice, x->stream_));
    }
    x->end(x->stream_);
    SR_HIP(hipStreamSynchronize(x->stream_));
    x->off_host_ = std::move(off);
    x->live_host_ = std::move(live);
    x->n_rows_ = n;
    x->n_live_ = n_live;
    x->n_tokens_ = T;
  } catch (...) {
    delete x;
    throw;
  }
  return x;
}

}  // namespace sr
