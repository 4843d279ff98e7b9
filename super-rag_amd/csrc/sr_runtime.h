// Host runtime objects behind the C-ABI: the in-HBM vector store and the transformer encoder.
#pragma once

#include <memory>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

#include "sr_carve.h"
#include "sr_common.h"

namespace sr {

// Flush a written file's data to stable storage before it is renamed into place (snapshot
// writers: a commit must never name a base whose bytes are still only in the page cache).
inline bool fsync_path(const std::string& path) {
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) return false;
  const bool ok = ::fsync(fd) == 0;
  return (::close(fd) == 0) && ok;
}

// RAII device allocation.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
    o.p = nullptr;
    o.bytes = 0;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // Grow to at least n bytes (contents are NOT preserved).
  void reserve(size_t n) {
    if (n <= bytes) return;
    release();
    SR_HIP(hipMalloc(&p, n));
    bytes = n;
  }
  // Grow to the carver's total and point its parts into the buffer (sr_carve.h).
  void carve(const Carve& c) { reserve(c.bytes()); c.bind(p); }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

// A non-blocking stream of the current device for the length of one call: synchronised and
// destroyed on every way out of the scope, an exception included (errors of either are ignored).
struct ScopedStream {
  hipStream_t s = nullptr;
  ScopedStream() { SR_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ScopedStream(const ScopedStream&) = delete;
  ScopedStream& operator=(const ScopedStream&) = delete;
  ~ScopedStream() {
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
};

// Scoped device selection (restores the caller's current device).
struct DeviceGuard {
  int prev = 0;
  explicit DeviceGuard(int dev) {
    SR_HIP(hipGetDevice(&prev));
    if (prev != dev) SR_HIP(hipSetDevice(dev));
  }
  ~DeviceGuard() { (void)hipSetDevice(prev); }
};

// ------------------------------------------------------------------------------------------------
class Store {
 public:
  Store(int dim, int device, int64_t capacity);
  ~Store();

  int dim() const { return dim_; }
  int ld() const { return ld_; }
  int device() const { return device_; }
  int64_t rows() const { return n_rows_; }
  int64_t live() const { return n_live_; }

  void add_host(const float* vecs, int64_t n, int64_t* out_rows);
  int64_t add_dev(const void* vecs, int dtype, int64_t n, hipStream_t s);
  void remove(const int64_t* rows, int64_t n);
  void get(const int64_t* rows, int64_t n, float* out);
  // allow: optional host eligibility mask (n_rows bytes), cached on the device per mask_key
  // raw_sim: out_dist receives the similarities (descending) instead of 1 - sim, for callers
  // that merge lists (1 - sim in fp32 can merge two neighbouring similarities into one distance)
  void search_host(const float* q, int B, int k, float* out_dist, int64_t* out_rows,
                   const uint8_t* allow = nullptr, int64_t mask_key = 0, bool raw_sim = false);
  void search_dev(const void* q, int q_dtype, int B, int k, float* out_sim, int64_t* out_rows,
                  int64_t row_offset, hipStream_t s, const uint8_t* elig = nullptr);
  // MMR over candidates as search_dev wrote them (k_mmr.hip); asynchronous on s
  void mmr_dev(const int64_t* cand_rows, const float* cand_sims, int B, int K, int64_t row_offset,
               float lambda, int mode, float min_score, int k_out, float* out_score,
               float* out_sim, int64_t* out_rows, hipStream_t s);
  // search_host for the top k_cand, then MMR, keep k (out_dist = 1 - cos of the kept rows)
  void search_mmr_host(const float* q, int B, int k, int k_cand, float lambda, int mode,
                       float min_score, const uint8_t* allow, int64_t mask_key, float* out_score,
                       float* out_dist, int64_t* out_rows);
  // every query b searches only the rows of list q_list[b] (CSR list_off / list_rows, host; local
  // row ids strictly ascending inside a list; lists may be shared or empty); out_sim descending,
  // -inf / -1 past the eligible rows; reads the fp16 rows in either scan mode (k_subset.hip)
  void search_subset_host(const float* q, int B, int k, const int32_t* q_list, int n_lists,
                          const int64_t* list_off, const int64_t* list_rows, float* out_sim,
                          int64_t* out_rows);
  // grouped search (k_group.hip): the k best distinct groups with the group_size best rows of each,
  // exact: search_dev for the top k_cand, group_collapse, and continuation rounds for the queries
  // whose list did not settle the answer.  group: host int32 [n_rows] (>= 0 a group, -1 a group of
  // its own), cached on the device per group_key like the allow mask.  out_sim: similarities.
  void search_grouped_host(const float* q, int B, int k, int group_size, int k_cand,
                           const int32_t* group, int64_t group_key, const uint8_t* allow,
                           int64_t mask_key, float* out_sim, int64_t* out_rows, int32_t* out_group);
  // group_collapse over candidates as search_dev wrote them; no continuation; asynchronous on s
  void group_dev(const int64_t* cand_rows, const float* cand_sims, int B, int K, int64_t row_offset,
                 int k, int group_size, const int32_t* group, int64_t group_key, float* out_sim,
                 int64_t* out_rows, int32_t* out_group, int32_t* out_complete, hipStream_t s);
  // device copy of a host group array (validated; cached per group_key and store version)
  const int32_t* group_array(const int32_t* group, int64_t group_key);
  // exact cosines of (query, row) pairs on the fp16 rows (k_fuse.hip score_rows): rows [B][K] carry
  // row_offset; -inf for a row outside the store or tombstoned; asynchronous on s
  void score_rows_dev(const void* q, int q_dtype, int B, const int64_t* rows, int K,
                      int64_t row_offset, float* out_sim, hipStream_t s);
  void score_rows_host(const float* q, int B, const int64_t* rows, int K, float* out_sim);
  // device eligibility mask live & allow (cached per mask_key and store version); null for null
  const uint8_t* eligibility(const uint8_t* allow, int64_t mask_key);
  // scan dtype: SR_DTYPE_F16 (default) or SR_DTYPE_FP8_E4M3 (fp8 copy + exact fp16 re-scoring)
  void set_scan_dtype(int dtype);
  int scan_dtype() const { return fp8_ ? SR_DTYPE_FP8_E4M3 : SR_DTYPE_F16; }
  void save(const char* path);
  static Store* load(const char* path, int device);
  void compact(int64_t* old_to_new);

  std::mutex mu;

 private:
  // Cross-stream ordering: every operation first makes its stream wait for the previous
  // operation's completion event, and records the event when it has enqueued its work, so calls
  // on different streams (the object's own stream, torch's stream, the null stream) never race
  // on the corpus or the shared workspaces.
  void begin(hipStream_t s) { SR_HIP(hipStreamWaitEvent(s, done_, 0)); }
  void end(hipStream_t s) { SR_HIP(hipEventRecord(done_, s)); }
  void ensure_capacity(int64_t rows);
  void ensure_query_ws(int B);
  // Runs the chunked scan/select schedule for one block of <= 256 normalised queries.
  void search_block(const half_t* qn, int B, int k, float* out_sim, int64_t* out_rows,
                    int64_t row_offset, hipStream_t s, bool safe, const uint8_t* live);
  void search_block8(const half_t* qn, int B, int k, float* out_sim, int64_t* out_rows,
                     int64_t row_offset, hipStream_t s, bool safe, const uint8_t* live);
  int ld8() const;
  void grow_fp8();
  void quantize_rows(int64_t r0, int64_t n, hipStream_t s);

  int dim_, ld_, device_;
  int64_t n_rows_ = 0, n_live_ = 0, capacity_ = 0;
  DevBuf corpus_, live_;
  std::vector<uint8_t> live_host_;
  hipStream_t stream_ = nullptr;
  hipEvent_t done_ = nullptr;
  // search workspace
  DevBuf qbuf_, qstage_, cand_, cnt_, tau_, overflow_, scratch_;
  int ws_queries_ = 0;
  // fp8 scan: e4m3(256 x) copy of the rows (ld8 bytes each), query staging, fp8-stage candidates
  bool fp8_ = false;
  DevBuf corpus8_, q8_, approx_;
  // filtered search: device eligibility mask (live & allow) and what it was built from
  DevBuf mask_;
  int64_t version_ = 0, mask_key_ = 0, mask_version_ = -1, mask_rows_ = -1;
  // subset search: list offsets | list rows | query lists, groups and work items of one call
  DevBuf subset_;
  // grouped search: the group array and what it was built from, the continuation rounds'
  // eligibility mask (never the cached mask_), staging of one call, group_dev's per-query state
  DevBuf group_, gmask_, gstage_, gstate_;
  int64_t group_key_ = 0, group_version_ = -1, group_rows_ = -1;
};

// One collection row-sharded over several devices (store_set.cpp; C-ABI sr_store_set_*).
class StoreSet {
 public:
  StoreSet(int dim, int dtype, const int* devices, int n_dev);
  int dim() const { return dim_; }
  int shards() const { return (int)shards_.size(); }
  int64_t rows() const;
  int64_t live() const;
  void add_host(const float* vecs, int64_t n, int64_t* out_rows);
  void remove(const int64_t* rows, int64_t n);
  void get(const int64_t* rows, int64_t n, float* out);
  void search_host(const float* q, int B, int k, float* out_dist, int64_t* out_rows,
                   const uint8_t* allow = nullptr, int64_t mask_key = 0);
  void set_scan_dtype(int dtype);

  std::mutex mu;

 private:
  // rows -> per-shard local rows and their positions in the argument
  void split(const int64_t* rows, int64_t n, std::vector<std::vector<int64_t>>& local,
             std::vector<std::vector<int64_t>>& pos) const;
  int dim_;
  std::vector<std::unique_ptr<Store>> shards_;
  std::vector<std::vector<int64_t>> tables_;  // per shard: local row -> global row
  std::vector<int32_t> shard_of_;             // global row -> shard
  std::vector<int64_t> local_of_;             // global row -> local row
};

// ------------------------------------------------------------------------------------------------
class Encoder {
 public:
  Encoder(const sr_encoder_config& cfg, int device);
  ~Encoder();

  void set_weight(const std::string& name, const float* data, int64_t numel);
  std::string missing() const;  // empty when every weight is set

  // forward_dev's "keep all tokens" request (mode 0 only): the sparse head's outputs, computed from
  // the final states of every token, so the last layer runs in full whatever the pooling.
  struct SparseOut {
    const int32_t* special_ids;   // host, n_special in [0, 16]
    int n_special;
    float* tok_weight;            // B x S device, may be null
    int32_t* terms;               // B x S device
    float* weights;               // B x S device
    int32_t* count;               // B device
  };
  // the multi-vector (ColBERT) head's outputs: the compacted unit token vectors and their count
  struct MultiVecOut {
    half_t* vecs;                 // B x S x dc device; rows [len, S) of a sequence are zero
    int32_t* len;                 // B device
  };
  // one request for the heads that read every token's final state: either or both
  struct TokenHeads {
    const SparseOut* sparse = nullptr;
    const MultiVecOut* multivec = nullptr;
  };
  // mode 0: pooled embeddings to `out` (dtype/ld_out); mode 1: classifier logits (fp32).
  void forward_dev(const int32_t* ids, const int32_t* mask, const int32_t* types, int B, int S,
                   int mode, int pool, void* out, int out_dtype, int ld_out, hipStream_t s,
                   const TokenHeads* heads = nullptr);
  // the multi-vector group of forward_host: the fp16 values as fp32, B x S x dc, and the counts
  struct MultiVecHost {
    float* vecs;
    int32_t* len;
  };
  // host buffers, blocking: upload, forward_dev, download.  `out` is the dense embedding (mode 0,
  // fp32 B x hidden) or the logits (mode 1); the optional groups (mode 0) are the sparse outputs
  // (a SparseOut of host pointers) and the multi-vector outputs
  void forward_host(const int32_t* ids, const int32_t* mask, const int32_t* types, int B, int S,
                    int mode, int pool, float* out, const SparseOut* sparse = nullptr,
                    const MultiVecHost* multivec = nullptr);
  int colbert_dim() const { return colbert_w_set_ ? colbert_dc_ : 0; }

  const sr_encoder_config& config() const { return cfg_; }
  // fp8 modes (LN-folded encoders), 0 = fp16.  Product modes: 1 = FFN2 (FFN1 stores e4m3(2 GELU),
  // FFN2 runs on the block-scaled fp8 MFMA with an e4m3 copy of its weight); 3 = FFN1 + FFN2 (FFN1
  // reads the e4m3 copy of the residual sums that the O-projection's *_STATS epilogue writes; QKV +
  // attention stay fp16, fused): the shipped fp8 mode, it ranks like the fp32 oracle on the
  // discriminative fidelity sets; 2 = mode 3 + the QKV GEMMs of layers >= 1 on the e4m3 residual
  // copy, an opt-in speed / fidelity trade (std / err 2.0).  Measured and rejected (the
  // diagnostic library keeps them for the record): 4 = mode 3 + QKV in fp8 on normalised e4m3 rows
  // (2.0), 5 = mode 3 + the O-projection of the fused layers on e4m3 ctx written by K5c (6.4).
  // fp8_plan() is the only code that knows the numbers.
  void set_fp8(int mode);
  int device() const { return device_; }
  std::mutex mu;

 private:
  struct Target {
    void* ptr;
    int64_t numel;
    bool f16;
    float* master = nullptr;  // fp32 copy kept for LayerNorm folding (QKV / FFN1 weights)
    int64_t split_k = 0;      // split weights: rows of split_k fp32 -> [fp16 hi | fp16 lo]
  };
  struct Layer {
    DevBuf wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b;
    // LayerNorm folding (fp16 residual stream): fp32 masters and the folded copies
    DevBuf wqkv32, w132, wqkv_f, cqkv, dqkv, w1_f, c1, d1, bo_f, b2_f, w2h;
    // fp8 modes: e4m3 copies of w2h (FFN) and of the folded w1_f / wqkv_f (all), their per-row
    // exponents and the folded column sums of the quantised weights
    DevBuf w2_8, w2e, w1_8, w1e, c1_8, wqkv8, wqkve, cqkv8;
    DevBuf wo_8, woe;  // fp8 mode 5: e4m3 rows of the O-projection weight + their E8M0 exponents
    // K/V-free CLS-only last layer: block-diagonal K / V weights, zero bias (H*D)
    DevBuf wk_bd, wv_bd, zb;
  };
  // which GEMMs of the folded layers an fp8 mode runs on the block-scaled fp8 MFMA
  struct Fp8Plan {
    bool ffn2 = false;      // FFN2 on e4m3(2 GELU) written by FFN1
    bool ffn1 = false;      // FFN1 on the e4m3 copy of u1 written by the O-projection
    bool qkv = false;       // QKV of layers >= 1 on an e4m3 copy of the previous block's output
    bool qkv_norm = false;  // ... of its NORMALISED rows (quantize_norm_fp8), not of u2 itself
    bool oproj = false;     // O-projection of the fused layers on e4m3 ctx written by K5c
  };
  static Fp8Plan fp8_plan(int mode);
  // one launch chunk of forward_dev: nb sequences, M = nb * S tokens, from sequence b0 on
  struct Chunk {
    int64_t b0;
    int nb, S, M;
    const int32_t *ids, *mask, *types;  // at the chunk's first token (types may be null)
    bool cls_only;                      // only the first token's final state is consumed
    hipStream_t s;
    // the folded stack: u (un-normalised residual sums) lives in h16 (in place), the compact
    // last-layer rows in y32_; sA / mA: statistics of u after the O-projection, sB / mB: after FFN2
    half_t *U, *Uc;
    float *sA, *sB, *mA, *mB;
    uint8_t *u8, *ctx8;                 // e4m3 copies: residual rows; the fused layers' ctx (mode 5)
    bool fuse_qa, o8, kvfree;           // K5c layers; their fp8 O-projection; K/V-free last layer
  };
  bool fold_enabled() const;
  void prepare_fold(hipStream_t s);
  void begin(hipStream_t s) { SR_HIP(hipStreamWaitEvent(s, done_, 0)); }
  void end(hipStream_t s) { SR_HIP(hipEventRecord(done_, s)); }
  void register_target(const std::string& name, DevBuf& buf, int64_t numel, bool f16,
                       int64_t offset_elems = 0, int64_t total_elems = -1, int64_t split_k = 0);
  void ensure_ws(int64_t tokens);
  // forward_dev's stages, in call order
  void check_forward(int B, int S, int mode, int pool, int out_dtype, int ld_out,
                     const TokenHeads* heads) const;
  float* reserve_forward(int B, int S, int mode, int64_t chunk_seqs, const TokenHeads* heads);
  void embed_stage(const Chunk& c);
  void folded_stack(const Chunk& c);
  void fold_qkv_attention(const Chunk& c, size_t l, bool last);
  void fold_oproj(const Chunk& c, size_t l, bool last);
  void fold_ffn(const Chunk& c, size_t l, bool last);
  void unfolded_stack(const Chunk& c);
  void output_stage(const Chunk& c, int mode, int pool, void* out, int out_dtype, int ld_out,
                    const TokenHeads* heads, float* tok_weight);

  sr_encoder_config cfg_;
  int device_;
  hipStream_t stream_ = nullptr;
  hipEvent_t done_ = nullptr;
  int64_t max_tokens_;
  DevBuf wemb_, pemb_, temb_, embg_, embb_, wc_, bc_, wout_, bout_;
  std::vector<Layer> layers_;
  std::map<std::string, Target> targets_;
  std::map<std::string, bool> is_set_;
  // workspace
  DevBuf ids_, mask_, types_, pos_, h16_, h32_, qkv_, ctx_, y32_, ffn_, clst_, hostio_;
  // sparse head (optional: "sparse_linear.weight" [hidden], "sparse_linear.bias" [1], fp32) and the
  // token weights of one call when the caller wants none
  DevBuf sparse_w_, sparse_b_, sparse_tw_;
  bool sparse_w_set_ = false, sparse_b_set_ = false;
  // multi-vector head (optional: "colbert_linear.weight" [dc, hidden] fp16 in the GEMM's W layout,
  // "colbert_linear.bias" [dc] fp32) and the GEMM output of one launch chunk
  DevBuf colbert_w_, colbert_b_, colbert_v_;
  bool colbert_w_set_ = false, colbert_b_set_ = false;
  int colbert_dc_ = 0;
  DevBuf statA_, statB_, mrA_, mrB_;  // per-row LayerNorm partials / (mu, rstd) (folded path)
  bool fold_ready_ = false;  // folded weights match the current weights
  int fp8_ = 0;      // the mode set_fp8 was given
  Fp8Plan plan_;     // = fp8_plan(fp8_): what prepare_fold and the folded stages read
  // split weights (fp32-residual encoders, i.e. the embedders): each layer matrix W is held as
  // [fp16(W) | fp16(W - fp16(W))] and the GEMMs run K = 2 K_x over the repeated activation, which
  // removes the fp16 weight rounding (~9e-4 of the 1.1e-3 embedding error of 24-layer bge-m3)
  bool split_ = false;
  DevBuf u8_;  // e4m3 copy of the residual sums (fp8 modes 2 / 3) or normalised rows (mode 4)
  DevBuf unit_mr_;  // (mu, rstd) = (0, 1): fp8 mode 4 QKV statistics (stat_ld 0)
  static constexpr size_t kChunkWsBytes = size_t(64) << 20;
  DevBuf chunk_ws_;  // split-K partial tiles of the unfolded (embedder) GEMMs at short M
  int64_t ws_tokens_ = 0;
};

// ------------------------------------------------------------------------------------------------
// Lexical index over the rows of a store (k_lex.hip): BM25 (a posting carries tf), or impact
// (SR_LEX_IMPACT: a posting carries the fp32 bits of a learned document weight in tf's place and a
// row's score is the fixed-point dot product with the query's weights).
class LexIndex {
 public:
  LexIndex(int device, float k1, float b, int mode = SR_LEX_BM25);
  ~LexIndex();

  int mode() const { return mode_; }
  // one scored term of one query: its multiplicity (BM25) and idf (BM25) or query weight (impact)
  struct QTerm {
    int32_t term, mult;
    float w;
  };
  // impact mode.  n documents: terms[off[i] .. off[i+1]) distinct term ids with weights in
  // (0, SR_IMPACT_MAX_WEIGHT]
  void add_weighted(const int64_t* off, const int32_t* terms, const float* weights, int64_t n,
                    int64_t* first_row);
  // query b: terms qterms[qoff[b] .. qoff[b+1]) with weights >= 0 (a repeated id keeps its maximum)
  void search_weighted_host(const int64_t* qoff, const int32_t* qterms, const float* qweights, int B,
                            int k, const uint8_t* allow, int64_t mask_key, float* out_score,
                            int64_t* out_rows, uint32_t* out_fixed);
  void score_rows_weighted_host(const int64_t* qoff, const int32_t* qterms, const float* qweights,
                                int B, const int64_t* rows, int K, float* out_score,
                                uint32_t* out_fixed);

  // n documents: terms[off[i] .. off[i+1]) distinct term ids with frequencies tf, length dl[i]
  void add(const int64_t* off, const int32_t* terms, const int32_t* tf, const int32_t* dl,
           int64_t n, int64_t* first_row);
  void remove(const int64_t* rows, int64_t n);
  void compact(int64_t* old_to_new);
  // query b: terms qterms[qoff[b] .. qoff[b+1]) (repeats count); outputs on the device (search_dev,
  // on stream s) or the host
  void search_dev(const int64_t* qoff, const int32_t* qterms, int B, int k, const uint8_t* allow,
                  int64_t mask_key, float* out_score, int64_t* out_rows, hipStream_t s,
                  const sr_lex_global* glob = nullptr, int64_t row_offset = 0,
                  uint32_t* out_fixed = nullptr);
  // device-resident queries: tok [B, Lq] int32 (row stride Lq), qlen [B] int32, both in HBM.
  // query_stats_dev writes [n_live, sum_dl, df of every (query, position)] (2 + B Lq int64, the
  // vector a row-sharded corpus sums over its shards); search_tok_dev scores with those summed
  // statistics (gstats, device) or this index's own (null).  No host synchronisation.
  void query_stats_dev(const int32_t* tok, const int32_t* qlen, int B, int Lq, int64_t* out,
                       hipStream_t s);
  void search_tok_dev(const int32_t* tok, const int32_t* qlen, int B, int Lq, int k,
                      const int64_t* gstats, float* out_score, int64_t* out_rows, hipStream_t s,
                      int64_t row_offset);
  void totals(int64_t* n_live, int64_t* sum_dl) const;
  void df(const int32_t* terms, int n, int64_t* out);
  void search_host(const int64_t* qoff, const int32_t* qterms, int B, int k, const uint8_t* allow,
                   int64_t mask_key, float* out_score, int64_t* out_rows,
                   const sr_lex_global* glob = nullptr, uint32_t* out_fixed = nullptr);
  // exact BM25 of given (query, row) pairs (k_lex.hip lex_score_rows): rows [B][K] on the device
  // carry row_offset; out_score fp32 / out_fixed u32 (may be null) [B][K] on the device.  -inf / 0
  // for a row outside [0, rows) or tombstoned, `miss` / 0 for a live row without a scored term.
  // Synchronises s once (the host-built term tables).
  void score_rows_dev(const int64_t* qoff, const int32_t* qterms, int B, const int64_t* rows, int K,
                      const sr_lex_global* glob, int64_t row_offset, float* out_score,
                      uint32_t* out_fixed, hipStream_t s, float miss = 0.f);
  void score_rows_host(const int64_t* qoff, const int32_t* qterms, int B, const int64_t* rows, int K,
                       const sr_lex_global* glob, float* out_score, uint32_t* out_fixed);
  void stats(int64_t* rows, int64_t* live, int64_t* postings, int64_t* vocab, double* avgdl);
  void save(const char* path);
  static LexIndex* load(const char* path, int device);
  int device() const { return device_; }
  hipStream_t stream() const { return stream_; }
  void begin(hipStream_t s) { SR_HIP(hipStreamWaitEvent(s, done_, 0)); }
  void end(hipStream_t s) { SR_HIP(hipEventRecord(done_, s)); }

  std::mutex mu;

 private:
  void rebuild(hipStream_t s);
  const uint8_t* eligibility(const uint8_t* allow, int64_t mask_key, hipStream_t s);
  // add / add_weighted after their checks: upload n rows of validated postings
  void append(const int64_t* off, const int32_t* terms, const uint64_t* val, const int32_t* dl,
              int64_t n);
  // search_dev / search_weighted_host after the query preparation (between begin and end, rebuilt)
  void search_terms(const std::vector<std::vector<QTerm>>& qt, int k, const uint8_t* elig, float adl,
                    float* out_score, int64_t* out_rows, hipStream_t s, int64_t row_offset,
                    uint32_t* out_fixed);
  // score_rows_dev / score_rows_weighted_host likewise (qt sorted by term id inside a query)
  void score_rows_terms(const std::vector<std::vector<QTerm>>& qt, const int64_t* rows, int K,
                        int64_t row_offset, float adl, float miss, float* out_score,
                        uint32_t* out_fixed, hipStream_t s);
  std::vector<std::vector<QTerm>> weighted_query_terms(const int64_t* qoff, const int32_t* qterms,
                                                       const float* qweights, int B) const;
  static float idf(int64_t df, int64_t n_live);
  static float avgdl(int64_t sum_dl, int64_t n_live);
  void forward(std::vector<int32_t>& fterm, std::vector<uint64_t>& fval);
  void load_rows(const std::vector<int32_t>& dl, const std::vector<uint8_t>& live,
                 const std::vector<int32_t>& ft, const std::vector<uint64_t>& fv);

  int device_;
  float k1_, b_;
  int mode_;
  hipStream_t stream_ = nullptr;
  hipEvent_t done_ = nullptr;
  int64_t rows_ = 0, live_n_ = 0, P_ = 0, vocab_ = 0, nnz_ = 0, sum_dl_ = 0, max_df_ = 0;
  bool dirty_ = true;
  // device: forward index, per-row data (foff_[rows + 1]: first forward posting of each row),
  // inverted index, workspaces
  DevBuf fterm_, fval_, dlen_, live_, foff_, off_, post_, ws_, out_, mask_, caps_;
  // host mirrors
  std::vector<int32_t> dl_host_, df_host_;
  std::vector<uint8_t> live_host_;
  std::vector<int64_t> off_host_;
  int64_t version_ = 0, mask_key_ = 0, mask_version_ = -1;
};

// ------------------------------------------------------------------------------------------------
// Multi-vector index over the rows of a store (multivec.hip, k_multivec.hip): one token pool
// [n_tokens][dim] in HBM (fp16, or e4m3 bytes of 256 x: dtype SR_DTYPE_FP8_E4M3), the first token of
// every row (int64) and live flags; scores are MaxSim.
class MultiVecIndex {
 public:
  MultiVecIndex(int dim, int device, int dtype = SR_DTYPE_F16);
  ~MultiVecIndex();

  int dim() const { return dim_; }
  int device() const { return device_; }
  // n rows: row i is the tokens vecs[off[i] .. off[i+1]) (fp32 host, rounded to fp16)
  void add_host(const int64_t* off, const float* vecs, int64_t n, int64_t* first_row);
  // n rows: row i is the first len[i] tokens of vecs[i] ([n][ld_tok][dim] fp16 device, len device);
  // reads the lengths back (synchronises s)
  void add_dev(const half_t* vecs, const int32_t* len, int64_t n, int ld_tok, int64_t* first_row,
               hipStream_t s);
  void remove(const int64_t* rows, int64_t n);
  void stats(int64_t* n_rows, int64_t* n_live, int64_t* n_tokens) const;
  // the pool's dtype and the bytes of the stored tokens (not the capacity)
  void info(int* dtype, int64_t* pool_bytes) const;
  // fp32 values of the stored tokens (fp8: the dequantised ones)
  void get(int64_t row, float* out, int64_t cap, int64_t* n_tok);
  void score_rows_dev(const half_t* q, const int32_t* q_len, int B, int ld_q, const int64_t* rows,
                      int K, float* out, hipStream_t s);
  void score_rows_host(const float* q, const int32_t* q_len, int B, int ld_q, const int64_t* rows,
                       int K, float* out);
  // the k eligible rows (live, not empty, allow[row] != 0 where allow is given) with the highest
  // MaxSim per query, (score desc, row asc), -inf / -1 past them; the scan runs in slabs of at most
  // slab_rows rows (0: sr_mv_plan.h's default).  Device buffers, asynchronous on s, nothing read back.
  void search_dev(const half_t* q, const int32_t* q_len, int B, int ld_q, int k, const uint8_t* allow,
                  int64_t slab_rows, int64_t row_offset, float* out_score, int64_t* out_rows, hipStream_t s);
  // the same on host buffers (allow: n_rows bytes or null).  Blocking.
  void search_host(const float* q, const int32_t* q_len, int B, int ld_q, int k, const uint8_t* allow,
                   int64_t slab_rows, float* out_score, int64_t* out_rows);
  // drops the tombstoned rows in place (kept rows keep their order; capacities stay): the kept
  // tokens move down the pool in chunks, through at most stage_bytes of staging (0: the default);
  // old_to_new (n_rows entries, may be null) as Store::compact writes it
  void compact(int64_t stage_bytes, int64_t* old_to_new);
  void save(const char* path);
  static MultiVecIndex* load(const char* path, int device);
  static constexpr int64_t kDefaultStageBytes = int64_t(64) << 20;
  // a gap of this many bytes is enough for a chunk to move pool -> pool in one launch
  static constexpr int64_t kDirectMinBytes = int64_t(16) << 20;

  std::mutex mu;

 private:
  void begin(hipStream_t s) { SR_HIP(hipStreamWaitEvent(s, done_, 0)); }
  void end(hipStream_t s) { SR_HIP(hipEventRecord(done_, s)); }
  // room for the rows and tokens of an append (doubling; the contents move on stream s)
  void ensure_capacity(int64_t rows, int64_t tokens, hipStream_t s);
  // after the tokens are in the pool: offsets, live flags and the counts of n new rows
  void commit(const std::vector<int64_t>& len, hipStream_t s);

  bool fp8() const { return dtype_ == SR_DTYPE_FP8_E4M3; }
  size_t row_bytes() const { return (size_t)dim_ * (fp8() ? 1 : sizeof(half_t)); }

  int dim_, device_, dtype_;
  hipStream_t stream_ = nullptr;
  hipEvent_t done_ = nullptr;
  int64_t n_rows_ = 0, n_live_ = 0, n_tokens_ = 0, cap_rows_ = 0, cap_tokens_ = 0;
  DevBuf pool_, off_, live_, hostio_;
  DevBuf scan_;  // search: one slab's score scratch and the running [B, k] list
  std::vector<int64_t> off_host_{0};   // n_rows_ + 1 entries
  std::vector<uint8_t> live_host_;
};

}  // namespace sr
