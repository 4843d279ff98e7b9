// Multi-vector index (sr_mv_*; DESIGN.md "Multi-vector retrieval"): the per-token unit vectors of
// every row of a collection (bge-m3's multi-vector / ColBERT output), row-aligned with the store
// like sr_lex.  One token pool [n_tokens][dim] in HBM, fp16 or (SR_DTYPE_FP8_E4M3) the bytes
// e4m3(256 fp16(x)), an int64 offsets array (device copy and host mirror) and live flags; both the
// pool and the per-row arrays grow by doubling.  Every way into an fp8 pool goes through the one
// quantising kernel (launch_mv_pack_fp8), so the stored bytes do not depend on it.  Appends and
// removals finish before they return; scoring (k_multivec.hip) is asynchronous on the caller's
// stream and ordered against them by the completion event, as in the store.
#include <algorithm>
#include <cmath>
#include <vector>

#include "sr_kernels.h"
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

}  // namespace sr
