// C-ABI entry points (include/super_rag_mi355x.h): argument checks, exception -> error-code
// mapping, per-object locking, and the HIP-event profiler.
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "sr_kernels.h"
#include "sr_mv_plan.h"
#include "sr_runtime.h"

struct sr_store {
  sr::Store* impl;
};
struct sr_encoder {
  sr::Encoder* impl;
};
struct sr_lex {
  sr::LexIndex* impl;
};
struct sr_store_set {
  sr::StoreSet* impl;
};
struct sr_mv {
  sr::MultiVecIndex* impl;
};

namespace sr {

static thread_local std::string t_last_error;
void set_last_error(const std::string& msg) { t_last_error = msg; }

// ---- profiler --------------------------------------------------------------------------------
namespace {
struct ProfRecord {
  std::string name;
  hipEvent_t ev0, ev1;
  double flops, bytes;
};
struct ProfAgg {
  int64_t launches = 0;
  double ms = 0, flops = 0, bytes = 0;
};
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRecord> g_prof_pending;
std::vector<hipEvent_t> g_event_pool;
std::map<std::string, ProfAgg> g_prof_agg;

hipEvent_t take_event() {
  if (!g_event_pool.empty()) {
    hipEvent_t e = g_event_pool.back();
    g_event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  SR_HIP(hipEventCreate(&e));
  return e;
}

void drain_pending_locked() {
  for (auto& r : g_prof_pending) {
    (void)hipEventSynchronize(r.ev1);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.ev0, r.ev1) == hipSuccess) {
      ProfAgg& a = g_prof_agg[r.name];
      a.launches += 1;
      a.ms += ms;
      a.flops += r.flops;
      a.bytes += r.bytes;
    }
    g_event_pool.push_back(r.ev0);
    g_event_pool.push_back(r.ev1);
  }
  g_prof_pending.clear();
}
}  // namespace

ProfScope::ProfScope(const char* n, hipStream_t s, double f, double b)
    : name(n), flops(f), bytes(b), stream(s) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!g_prof_on) return;
  ev0 = take_event();
  ev1 = take_event();
  if (hipEventRecord(ev0, stream) != hipSuccess) {
    g_event_pool.push_back(ev0);
    g_event_pool.push_back(ev1);
    ev0 = ev1 = nullptr;
  }
}

ProfScope::~ProfScope() {
  if (!ev0) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (hipEventRecord(ev1, stream) == hipSuccess) {
    g_prof_pending.push_back(ProfRecord{name, ev0, ev1, flops, bytes});
    if (g_prof_pending.size() > 65536) drain_pending_locked();
  } else {
    g_event_pool.push_back(ev0);
    g_event_pool.push_back(ev1);
  }
}

}  // namespace sr

#define SR_API_BEGIN try {
#define SR_API_END                           \
  return SR_OK;                              \
  }                                          \
  catch (const sr::Error& e) {               \
    sr::set_last_error(e.what());            \
    return e.code;                           \
  }                                          \
  catch (const std::bad_alloc&) {            \
    sr::set_last_error("host out of memory"); \
    return SR_ERR_OOM;                       \
  }                                          \
  catch (const std::exception& e) {          \
    sr::set_last_error(e.what());            \
    return SR_ERR_INVALID;                   \
  }

// The scoring mode an entry point needs (SR_LEX_BM25 / SR_LEX_IMPACT): SR_ERR_STATE on the other.
static void lex_need_mode(const sr_lex* x, int mode, const char* who) {
  if (x->impl->mode() != mode)
    throw sr::Error(SR_ERR_STATE, std::string(who) + (mode == SR_LEX_IMPACT
                                                          ? ": needs an impact index (sr_lex_create_impact)"
                                                          : ": needs a BM25 index, this one scores impacts"));
}

#define SR_NONNULL(p)                                                   \
  do {                                                                  \
    if (!(p)) throw sr::Error(SR_ERR_INVALID, "null argument: " #p);    \
  } while (0)

extern "C" {

const char* sr_last_error(void) { return sr::t_last_error.c_str(); }
int sr_version(void) { return 100; }

int sr_device_count(int* out) {
  SR_API_BEGIN
  SR_NONNULL(out);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *out = n;
  SR_API_END
}

int sr_memcpy(void* dst, const void* src, int64_t bytes, int kind, int device) {
  SR_API_BEGIN
  SR_NONNULL(dst);
  SR_NONNULL(src);
  sr::DeviceGuard g(device);
  const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice
                          : kind == 1 ? hipMemcpyDeviceToHost
                                      : hipMemcpyDeviceToDevice;
  SR_HIP(hipMemcpy(dst, src, (size_t)bytes, k));
  SR_API_END
}

// ---- store -----------------------------------------------------------------------------------
int sr_store_create(int dim, int device, int64_t initial_capacity, sr_store** out) {
  SR_API_BEGIN
  SR_NONNULL(out);
  *out = nullptr;
  auto* s = new sr_store{new sr::Store(dim, device, initial_capacity)};
  *out = s;
  SR_API_END
}

int sr_store_add(sr_store* s, const float* vecs, int64_t n, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->add_host(vecs, n, out_rows);
  SR_API_END
}

int sr_store_add_dev(sr_store* s, const void* vecs, int dtype, int64_t n, int64_t* first_row,
                     void* stream) {
  SR_API_BEGIN
  SR_NONNULL(s);
  SR_NONNULL(vecs);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  const int64_t first = s->impl->add_dev(vecs, dtype, n, reinterpret_cast<hipStream_t>(stream));
  if (first_row) *first_row = first;
  SR_API_END
}

int sr_store_remove(sr_store* s, const int64_t* rows, int64_t n) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->remove(rows, n);
  SR_API_END
}

int sr_store_count(sr_store* s, int64_t* n_rows, int64_t* n_live) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  if (n_rows) *n_rows = s->impl->rows();
  if (n_live) *n_live = s->impl->live();
  SR_API_END
}

int sr_store_dim(sr_store* s, int* dim) {
  SR_API_BEGIN
  SR_NONNULL(s);
  SR_NONNULL(dim);
  *dim = s->impl->dim();
  SR_API_END
}

int sr_store_get(sr_store* s, const int64_t* rows, int64_t n, float* out) {
  SR_API_BEGIN
  SR_NONNULL(s);
  if (n > 0) {
    SR_NONNULL(rows);
    SR_NONNULL(out);
  }
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->get(rows, n, out);
  SR_API_END
}

int sr_store_search(sr_store* s, const float* q, int B, int k, float* out_dist, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->search_host(q, B, k, out_dist, out_rows);
  SR_API_END
}

int sr_store_search_masked(sr_store* s, const float* q, int B, int k, const uint8_t* allow,
                           int64_t mask_key, float* out_dist, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(s);
  SR_NONNULL(allow);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->search_host(q, B, k, out_dist, out_rows, allow, mask_key);
  SR_API_END
}

int sr_store_search_sim(sr_store* s, const float* q, int B, int k, const uint8_t* allow,
                        int64_t mask_key, float* out_sim, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->search_host(q, B, k, out_sim, out_rows, allow, allow ? mask_key : 0, true);
  SR_API_END
}

int sr_store_search_dev(sr_store* s, const void* q, int q_dtype, int B, int k, float* out_sim,
                        int64_t* out_rows, int64_t row_offset, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(s);
  if (B > 0) {
    SR_NONNULL(q);
    SR_NONNULL(out_sim);
    SR_NONNULL(out_rows);
  }
  SR_CHECK(q_dtype == SR_DTYPE_F32 || q_dtype == SR_DTYPE_F16, "search: q dtype must be f32/f16");
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->search_dev(q, q_dtype, B, k, out_sim, out_rows, row_offset,
                      reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

// ---- MMR diversification (k_mmr.hip) -----------------------------------------------------------
int sr_mmr_rerank(const float* q, const float* cand, const int32_t* n_cand, int B, int K, int dim,
                  float lambda, int mode, float min_score, int k_out, float* out_score,
                  int32_t* out_index, int device) {
  SR_API_BEGIN
  sr::mmr_check_args(B, K, k_out, lambda, mode);
  SR_CHECK(dim > 0 && dim <= 8192, "mmr: dim must be in [1, 8192]");
  if (B == 0) return SR_OK;
  SR_NONNULL(q);
  SR_NONNULL(cand);
  SR_NONNULL(out_score);
  SR_NONNULL(out_index);
  sr::DeviceGuard g(device);
  const int64_t ld = sr::round_up(dim, 64);
  const int64_t nc = (int64_t)B * K, no = (int64_t)B * k_out;
  float *q32, *c32, *ds;
  sr::half_t *q16, *c16;  // the normalised rows the kernel reads
  int32_t *dn, *di;
  sr::Carve c;
  c.part((size_t)B * dim, &q32);
  c.part((size_t)nc * dim, &c32);
  c.part((size_t)B * ld, &q16);
  c.part((size_t)nc * ld, &c16);
  c.part((size_t)B, &dn);
  c.part((size_t)no, &ds, &di);
  sr::DevBuf ws;
  ws.carve(c);
  sr::ScopedStream st;
  SR_HIP(hipMemcpyAsync(q32, q, (size_t)B * dim * 4, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(c32, cand, (size_t)nc * dim * 4, hipMemcpyHostToDevice, st));
  if (n_cand) SR_HIP(hipMemcpyAsync(dn, n_cand, (size_t)B * 4, hipMemcpyHostToDevice, st));
  sr::launch_normalize_rows(q32, SR_DTYPE_F32, B, dim, q16, (int)ld, st);
  sr::launch_normalize_rows(c32, SR_DTYPE_F32, nc, dim, c16, (int)ld, st);
  sr::launch_mmr_rerank(c16, ld, nc, nullptr, 0, n_cand ? dn : nullptr, nullptr, q16, B, K, lambda,
                        mode, min_score, k_out, ds, nullptr, di, nullptr, st);
  SR_HIP(hipMemcpyAsync(out_score, ds, (size_t)no * 4, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(out_index, di, (size_t)no * 4, hipMemcpyDeviceToHost, st));
  SR_HIP(hipStreamSynchronize(st));
  SR_API_END
}

int sr_store_mmr_dev(sr_store* s, const int64_t* cand_rows, const float* cand_sims, int B, int K,
                     int64_t row_offset, float lambda, int mode, float min_score, int k_out,
                     float* out_score, float* out_sim, int64_t* out_rows, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(s);
  sr::mmr_check_args(B, K, k_out, lambda, mode);
  if (B == 0) return SR_OK;
  SR_NONNULL(cand_rows);
  SR_NONNULL(cand_sims);
  SR_NONNULL(out_score);
  SR_NONNULL(out_sim);
  SR_NONNULL(out_rows);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->mmr_dev(cand_rows, cand_sims, B, K, row_offset, lambda, mode, min_score, k_out,
                   out_score, out_sim, out_rows, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_store_search_mmr(sr_store* s, const float* q, int B, int k, int k_cand, float lambda,
                        int mode, float min_score, const uint8_t* allow, int64_t mask_key,
                        float* out_score, float* out_dist, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(s);
  sr::mmr_check_args(B, k_cand, k, lambda, mode);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->search_mmr_host(q, B, k, k_cand, lambda, mode, min_score, allow, allow ? mask_key : 0,
                           out_score, out_dist, out_rows);
  SR_API_END
}

int sr_store_search_subset(sr_store* s, const float* q, int B, int k, const int32_t* q_list,
                           int n_lists, const int64_t* list_off, const int64_t* list_rows,
                           float* out_sim, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->search_subset_host(q, B, k, q_list, n_lists, list_off, list_rows, out_sim, out_rows);
  SR_API_END
}

// ---- grouped search (k_group.hip) ----------------------------------------------------------------
int sr_store_search_grouped(sr_store* s, const float* q, int B, int k, int group_size, int k_cand,
                            const int32_t* group, int64_t group_key, const uint8_t* allow,
                            int64_t mask_key, float* out_sim, int64_t* out_rows,
                            int32_t* out_group) {
  SR_API_BEGIN
  SR_NONNULL(s);
  sr::group_check_args(B, k_cand, k, group_size);
  if (B == 0) return SR_OK;
  SR_NONNULL(q);
  SR_NONNULL(group);
  SR_NONNULL(out_sim);
  SR_NONNULL(out_rows);
  SR_NONNULL(out_group);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->search_grouped_host(q, B, k, group_size, k_cand, group, group_key, allow,
                               allow ? mask_key : 0, out_sim, out_rows, out_group);
  SR_API_END
}

int sr_store_group_dev(sr_store* s, const int64_t* cand_rows, const float* cand_sims, int B, int K,
                       int64_t row_offset, int k, int group_size, const int32_t* group,
                       int64_t group_key, float* out_sim, int64_t* out_rows, int32_t* out_group,
                       int32_t* out_complete, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(s);
  sr::group_check_args(B, K, k, group_size);
  if (B == 0) return SR_OK;
  SR_NONNULL(cand_rows);
  SR_NONNULL(cand_sims);
  SR_NONNULL(group);
  SR_NONNULL(out_sim);
  SR_NONNULL(out_rows);
  SR_NONNULL(out_group);
  SR_NONNULL(out_complete);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->group_dev(cand_rows, cand_sims, B, K, row_offset, k, group_size, group, group_key,
                     out_sim, out_rows, out_group, out_complete, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_store_set_scan_dtype(sr_store* s, int dtype) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->set_scan_dtype(dtype);
  SR_API_END
}

int sr_store_save(sr_store* s, const char* path) {
  SR_API_BEGIN
  SR_NONNULL(s);
  SR_NONNULL(path);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->save(path);
  SR_API_END
}

int sr_store_load(const char* path, int device, sr_store** out) {
  SR_API_BEGIN
  SR_NONNULL(path);
  SR_NONNULL(out);
  *out = nullptr;
  sr::Store* st = sr::Store::load(path, device);
  *out = new sr_store{st};
  SR_API_END
}

int sr_store_compact(sr_store* s, int64_t* old_to_new) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->compact(old_to_new);
  SR_API_END
}

void sr_store_destroy(sr_store* s) {
  if (!s) return;
  delete s->impl;
  delete s;
}

// ---- multi-device collection (SURVEY 8(b) sr_store_create(dim, dtype, devices, n_dev)) ---------
int sr_store_set_create(int dim, int dtype, const int* devices, int n_dev, sr_store_set** out) {
  SR_API_BEGIN
  SR_NONNULL(out);
  SR_NONNULL(devices);
  *out = nullptr;
  *out = new sr_store_set{new sr::StoreSet(dim, dtype, devices, n_dev)};
  SR_API_END
}

int sr_store_set_add(sr_store_set* s, const float* vecs, int64_t n, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->add_host(vecs, n, out_rows);
  SR_API_END
}

int sr_store_set_remove(sr_store_set* s, const int64_t* rows, int64_t n) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->remove(rows, n);
  SR_API_END
}

int sr_store_set_count(sr_store_set* s, int64_t* n_rows, int64_t* n_live, int* n_shards) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  if (n_rows) *n_rows = s->impl->rows();
  if (n_live) *n_live = s->impl->live();
  if (n_shards) *n_shards = s->impl->shards();
  SR_API_END
}

int sr_store_set_get(sr_store_set* s, const int64_t* rows, int64_t n, float* out) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->get(rows, n, out);
  SR_API_END
}

int sr_store_set_search(sr_store_set* s, const float* q, int B, int k, const uint8_t* allow,
                        int64_t mask_key, float* out_dist, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->search_host(q, B, k, out_dist, out_rows, allow, allow ? mask_key : 0);
  SR_API_END
}

int sr_store_set_set_scan_dtype(sr_store_set* s, int dtype) {
  SR_API_BEGIN
  SR_NONNULL(s);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->set_scan_dtype(dtype);
  SR_API_END
}

void sr_store_set_destroy(sr_store_set* s) {
  if (!s) return;
  delete s->impl;
  delete s;
}

int sr_topk_merge_dev(const float* sims, const int64_t* rows, int P, int B, int k, int k_out,
                      float* out_sim, int64_t* out_rows, int device, void* stream) {
  SR_API_BEGIN
  SR_CHECK(P >= 1 && B >= 0 && k >= 1, "merge: bad shape");
  if (B > 0) {
    SR_NONNULL(sims);
    SR_NONNULL(rows);
    SR_NONNULL(out_sim);
    SR_NONNULL(out_rows);
  }
  sr::DeviceGuard g(device);
  sr::launch_topk_merge(sims, rows, P, B, k, k_out, out_sim, out_rows,
                        reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

// ---- encoder ---------------------------------------------------------------------------------
// ---- lexical index / hybrid ------------------------------------------------------------------
int sr_lex_create(int device, float k1, float b, sr_lex** out) {
  SR_API_BEGIN
  SR_NONNULL(out);
  *out = nullptr;
  *out = new sr_lex{new sr::LexIndex(device, k1, b)};
  SR_API_END
}

int sr_lex_create_impact(int device, sr_lex** out) {
  SR_API_BEGIN
  SR_NONNULL(out);
  *out = nullptr;
  *out = new sr_lex{new sr::LexIndex(device, 0.f, 0.f, SR_LEX_IMPACT)};
  SR_API_END
}

int sr_lex_scoring(sr_lex* x, int* out_mode) {
  SR_API_BEGIN
  SR_NONNULL(x);
  SR_NONNULL(out_mode);
  *out_mode = x->impl->mode();
  SR_API_END
}

int sr_lex_add_weighted(sr_lex* x, const int64_t* off, const int32_t* terms, const float* weights,
                        int64_t n, int64_t* first_row) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_IMPACT, "sr_lex_add_weighted");
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->add_weighted(off, terms, weights, n, first_row);
  SR_API_END
}

int sr_lex_search_weighted(sr_lex* x, const int64_t* qoff, const int32_t* qterms,
                           const float* qweights, int B, int k, const uint8_t* allow,
                           int64_t mask_key, float* out_score, int64_t* out_rows,
                           uint32_t* out_fixed) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_IMPACT, "sr_lex_search_weighted");
  if (B > 0) {
    SR_NONNULL(qoff);
    SR_NONNULL(out_score);
    SR_NONNULL(out_rows);
    if (qoff[B] > 0) {
      SR_NONNULL(qterms);
      SR_NONNULL(qweights);
    }
  }
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->search_weighted_host(qoff, qterms, qweights, B, k, allow, mask_key, out_score, out_rows,
                                out_fixed);
  SR_API_END
}

int sr_lex_score_rows_weighted(sr_lex* x, const int64_t* qoff, const int32_t* qterms,
                               const float* qweights, int B, const int64_t* rows, int K,
                               float* out_score, uint32_t* out_fixed) {
  SR_API_BEGIN
  SR_CHECK(B >= 0 && K >= 0, "lex.score_rows: negative shape");
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_IMPACT, "sr_lex_score_rows_weighted");
  if (B == 0 || K == 0) return SR_OK;
  SR_NONNULL(qoff);
  SR_NONNULL(rows);
  SR_NONNULL(out_score);
  if (qoff[B] > 0) {
    SR_NONNULL(qterms);
    SR_NONNULL(qweights);
  }
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->score_rows_weighted_host(qoff, qterms, qweights, B, rows, K, out_score, out_fixed);
  SR_API_END
}

int sr_lex_add(sr_lex* x, const int64_t* off, const int32_t* terms, const int32_t* tf,
               const int32_t* dl, int64_t n, int64_t* first_row) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_add");
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->add(off, terms, tf, dl, n, first_row);
  SR_API_END
}

int sr_lex_remove(sr_lex* x, const int64_t* rows, int64_t n) {
  SR_API_BEGIN
  SR_NONNULL(x);
  if (n > 0) SR_NONNULL(rows);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->remove(rows, n);
  SR_API_END
}

int sr_lex_stats(sr_lex* x, int64_t* n_rows, int64_t* n_live, int64_t* n_postings, int64_t* vocab,
                 double* avgdl) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->stats(n_rows, n_live, n_postings, vocab, avgdl);
  SR_API_END
}

int sr_lex_search(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B, int k,
                  const uint8_t* allow, int64_t mask_key, float* out_score, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_search");
  if (B > 0) {
    SR_NONNULL(qoff);
    SR_NONNULL(out_score);
    SR_NONNULL(out_rows);
    if (qoff[B] > 0) SR_NONNULL(qterms);
  }
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->search_host(qoff, qterms, B, k, allow, mask_key, out_score, out_rows);
  SR_API_END
}

int sr_lex_search_global(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B, int k,
                         const uint8_t* allow, int64_t mask_key, const sr_lex_global* global,
                         float* out_score, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_search_global");
  if (B > 0) {
    SR_NONNULL(qoff);
    SR_NONNULL(out_score);
    SR_NONNULL(out_rows);
    if (qoff[B] > 0) SR_NONNULL(qterms);
  }
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->search_host(qoff, qterms, B, k, allow, mask_key, out_score, out_rows, global);
  SR_API_END
}

int sr_lex_search_global_fixed(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B, int k,
                               const uint8_t* allow, int64_t mask_key, const sr_lex_global* global,
                               float* out_score, int64_t* out_rows, uint32_t* out_fixed) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_search_global_fixed");
  if (B > 0) {
    SR_NONNULL(qoff);
    SR_NONNULL(out_score);
    SR_NONNULL(out_rows);
    SR_NONNULL(out_fixed);
    if (qoff[B] > 0) SR_NONNULL(qterms);
  }
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->search_host(qoff, qterms, B, k, allow, mask_key, out_score, out_rows, global, out_fixed);
  SR_API_END
}

int sr_lex_totals(sr_lex* x, int64_t* n_live, int64_t* sum_dl) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_totals");
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->totals(n_live, sum_dl);
  SR_API_END
}

int sr_lex_df(sr_lex* x, const int32_t* terms, int n, int64_t* out_df) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_df");
  SR_CHECK(n >= 0, "lex.df: negative count");
  if (n > 0) {
    SR_NONNULL(terms);
    SR_NONNULL(out_df);
  }
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->df(terms, n, out_df);
  SR_API_END
}

int sr_lex_search_dev(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B, int k,
                      const sr_lex_global* global, float* out_score, int64_t* out_rows,
                      int64_t row_offset, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_search_dev");
  if (B > 0) {
    SR_NONNULL(qoff);
    SR_NONNULL(out_score);
    SR_NONNULL(out_rows);
    if (qoff[B] > 0) SR_NONNULL(qterms);
  }
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->search_dev(qoff, qterms, B, k, nullptr, 0, out_score, out_rows,
                      reinterpret_cast<hipStream_t>(stream), global, row_offset);
  SR_API_END
}

int sr_lex_query_stats_dev(sr_lex* x, const int32_t* tok, const int32_t* qlen, int B, int Lq,
                           int64_t* out_stats, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_query_stats_dev");
  SR_NONNULL(out_stats);
  SR_CHECK(B >= 0 && Lq >= 0, "lex.query_stats: negative shape");
  if ((int64_t)B * Lq > 0) {
    SR_NONNULL(tok);
    SR_NONNULL(qlen);
  }
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->query_stats_dev(tok, qlen, B, Lq, out_stats, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_lex_search_tok_dev(sr_lex* x, const int32_t* tok, const int32_t* qlen, int B, int Lq, int k,
                          const int64_t* gstats, float* out_score, int64_t* out_rows,
                          int64_t row_offset, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_search_tok_dev");
  if (B > 0) {
    SR_NONNULL(qlen);
    SR_NONNULL(out_score);
    SR_NONNULL(out_rows);
    if (Lq > 0) SR_NONNULL(tok);
  }
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->search_tok_dev(tok, qlen, B, Lq, k, gstats, out_score, out_rows,
                          reinterpret_cast<hipStream_t>(stream), row_offset);
  SR_API_END
}

int sr_lex_score_rows(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B,
                      const int64_t* rows, int K, const sr_lex_global* global, float* out_score,
                      uint32_t* out_fixed) {
  SR_API_BEGIN
  SR_CHECK(B >= 0 && K >= 0, "lex.score_rows: negative shape");
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_score_rows");
  if (B == 0 || K == 0) return SR_OK;
  SR_NONNULL(qoff);
  SR_NONNULL(rows);
  SR_NONNULL(out_score);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->score_rows_host(qoff, qterms, B, rows, K, global, out_score, out_fixed);
  SR_API_END
}

int sr_lex_score_rows_dev(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B,
                          const int64_t* rows, int K, const sr_lex_global* global,
                          int64_t row_offset, float* out_score, uint32_t* out_fixed, void* stream) {
  SR_API_BEGIN
  SR_CHECK(B >= 0 && K >= 0, "lex.score_rows: negative shape");
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_lex_score_rows_dev");
  if (B == 0 || K == 0) return SR_OK;
  SR_NONNULL(qoff);
  SR_NONNULL(rows);
  SR_NONNULL(out_score);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->score_rows_dev(qoff, qterms, B, rows, K, global, row_offset, out_score, out_fixed,
                          reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_lex_save(sr_lex* x, const char* path) {
  SR_API_BEGIN
  SR_NONNULL(x);
  SR_NONNULL(path);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->save(path);
  SR_API_END
}

int sr_lex_load(const char* path, int device, sr_lex** out) {
  SR_API_BEGIN
  SR_NONNULL(path);
  SR_NONNULL(out);
  *out = nullptr;
  sr::LexIndex* li = sr::LexIndex::load(path, device);
  *out = new sr_lex{li};
  SR_API_END
}

int sr_lex_compact(sr_lex* x, int64_t* old_to_new) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->compact(old_to_new);
  SR_API_END
}

void sr_lex_destroy(sr_lex* x) {
  if (!x) return;
  delete x->impl;
  delete x;
}

int sr_rrf_fuse(const int64_t* rows_a, int ka, const int64_t* rows_b, int kb, int B,
                int rank_const, double min_score, int k_out, double* out_score,
                int64_t* out_rows, int device) {
  SR_API_BEGIN
  SR_CHECK(B >= 0, "rrf: negative batch");
  if (B == 0) return SR_OK;
  SR_NONNULL(out_score);
  SR_NONNULL(out_rows);
  if (ka > 0) SR_NONNULL(rows_a);
  if (kb > 0) SR_NONNULL(rows_b);
  sr::DeviceGuard g(device);
  const size_t na = (size_t)B * ka, nb = (size_t)B * kb, no = (size_t)B * k_out;
  int64_t *da, *db, *dr;
  double* ds;
  sr::Carve c;
  c.part(na, &da);
  c.part(nb, &db);
  c.part(no, &ds, &dr);
  sr::DevBuf ws;
  ws.carve(c);
  sr::ScopedStream st;
  if (na) SR_HIP(hipMemcpyAsync(da, rows_a, na * 8, hipMemcpyHostToDevice, st));
  if (nb) SR_HIP(hipMemcpyAsync(db, rows_b, nb * 8, hipMemcpyHostToDevice, st));
  sr::launch_rrf_fuse(da, ka, db, kb, B, rank_const, min_score, k_out, ds, dr, st);
  SR_HIP(hipMemcpyAsync(out_score, ds, no * 8, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(out_rows, dr, no * 8, hipMemcpyDeviceToHost, st));
  SR_HIP(hipStreamSynchronize(st));
  SR_API_END
}

int sr_rrf_fuse_dev(const int64_t* rows_a, int ka, const int64_t* rows_b, int kb, int B,
                    int rank_const, double min_score, int k_out, double* out_score,
                    int64_t* out_rows, int device, void* stream) {
  SR_API_BEGIN
  SR_CHECK(B >= 0, "rrf: negative batch");
  if (B == 0) return SR_OK;
  SR_NONNULL(out_score);
  SR_NONNULL(out_rows);
  sr::DeviceGuard g(device);
  sr::launch_rrf_fuse(rows_a, ka, rows_b, kb, B, rank_const, min_score, k_out, out_score, out_rows,
                      reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_hybrid_search(sr_store* s, sr_lex* x, const float* q, const int64_t* qoff,
                     const int32_t* qterms, int B, int k, int k_each, int rank_const,
                     double min_score, const uint8_t* allow, int64_t mask_key,
                     double* out_score, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(s);
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_hybrid_search");
  SR_CHECK(B >= 0, "hybrid: negative batch");
  if (B == 0) return SR_OK;
  SR_NONNULL(q);
  SR_NONNULL(qoff);
  SR_NONNULL(out_score);
  SR_NONNULL(out_rows);
  SR_CHECK(k_each >= 1 && k_each <= SR_MAX_TOPK, "hybrid: k_each must be in [1, 1024]");
  SR_CHECK(k >= 1 && k <= 2 * k_each, "hybrid: k must be in [1, 2 * k_each]");
  std::scoped_lock lk(s->impl->mu, x->impl->mu);
  sr::Store& st = *s->impl;
  sr::LexIndex& lx = *x->impl;
  SR_CHECK(st.device() == lx.device(), "hybrid: store and lexical index on different devices");
  int64_t lrows = 0;
  lx.stats(&lrows, nullptr, nullptr, nullptr, nullptr);
  SR_CHECK(lrows == st.rows(), "hybrid: store and lexical index hold different row counts");
  sr::DeviceGuard g(st.device());
  hipStream_t sm = lx.stream();
  const size_t nq = (size_t)B * st.dim(), ne = (size_t)B * k_each, no = (size_t)B * k;
  float *dq, *dsim, *lsc;
  int64_t *drow, *lrow, *orow;
  double* os;
  sr::Carve c;
  c.part(nq, &dq);
  c.part(ne, &dsim, &drow, &lsc, &lrow);
  c.part(no, &os, &orow);
  sr::DevBuf ws;
  ws.carve(c);
  const uint8_t* elig = st.eligibility(allow, mask_key);
  lx.begin(sm);
  SR_HIP(hipMemcpyAsync(dq, q, nq * 4, hipMemcpyHostToDevice, sm));
  st.search_dev(dq, SR_DTYPE_F32, B, k_each, dsim, drow, 0, sm, elig);
  lx.search_dev(qoff, qterms, B, k_each, allow, mask_key, lsc, lrow, sm);
  sr::launch_rrf_fuse(drow, k_each, lrow, k_each, B, rank_const, min_score, k, os, orow, sm);
  SR_HIP(hipMemcpyAsync(out_score, os, no * 8, hipMemcpyDeviceToHost, sm));
  SR_HIP(hipMemcpyAsync(out_rows, orow, no * 8, hipMemcpyDeviceToHost, sm));
  lx.end(sm);
  SR_HIP(hipStreamSynchronize(sm));
  SR_API_END
}

// ---- score fusion (k_fuse.hip) ---------------------------------------------------------------------
static void fuse_check_buffers(const float* score_a, const int64_t* rows_a, int ka, const float* score_b,
                        const int64_t* rows_b, int kb, const float* out_score,
                        const int64_t* out_rows) {
  SR_CHECK(out_score && out_rows, "score_fuse: null output buffer");
  SR_CHECK(ka == 0 || (score_a && rows_a), "score_fuse: null list a");
  SR_CHECK(kb == 0 || (score_b && rows_b), "score_fuse: null list b");
}

int sr_score_fuse_sides(const float* score_a, const int64_t* rows_a, int ka, const float* score_b,
                        const int64_t* rows_b, int kb, const float* side_a, const float* side_b,
                        int B, int mode, float alpha, float floor_a, float floor_b, float min_score,
                        int k_out, float* out_score, int64_t* out_rows, float* out_a, float* out_b,
                        int device) {
  SR_API_BEGIN
  sr::fuse_check_args(B, ka, kb, mode, alpha, k_out);
  if (B == 0) return SR_OK;
  fuse_check_buffers(score_a, rows_a, ka, score_b, rows_b, kb, out_score, out_rows);
  for (int64_t i = 0; i < (int64_t)B * ka; ++i)
    SR_CHECK(rows_a[i] <= 0xfffffffeLL, "score_fuse: rows must be in [0, 2^32 - 2] (or < 0: absent)");
  for (int64_t i = 0; i < (int64_t)B * kb; ++i)
    SR_CHECK(rows_b[i] <= 0xfffffffeLL, "score_fuse: rows must be in [0, 2^32 - 2] (or < 0: absent)");
  sr::DeviceGuard g(device);
  const size_t na = (size_t)B * ka, nb = (size_t)B * kb, no = (size_t)B * k_out;
  int64_t *da_r, *db_r, *do_r;
  float *da_s, *db_s, *dside, *dsideb, *do_s, *do_a, *do_b;
  sr::Carve c;
  c.part(na, &da_r, &da_s, &dsideb);  // side b scores the rows of list a
  c.part(nb, &db_r, &db_s, &dside);   // and side a those of list b
  c.part(no, &do_r, &do_s, &do_a, &do_b);
  sr::DevBuf ws;
  ws.carve(c);
  sr::ScopedStream st;
  if (na) {
    SR_HIP(hipMemcpyAsync(da_r, rows_a, na * 8, hipMemcpyHostToDevice, st));
    SR_HIP(hipMemcpyAsync(da_s, score_a, na * 4, hipMemcpyHostToDevice, st));
    if (side_b) SR_HIP(hipMemcpyAsync(dsideb, side_b, na * 4, hipMemcpyHostToDevice, st));
  }
  if (nb) {
    SR_HIP(hipMemcpyAsync(db_r, rows_b, nb * 8, hipMemcpyHostToDevice, st));
    SR_HIP(hipMemcpyAsync(db_s, score_b, nb * 4, hipMemcpyHostToDevice, st));
    if (side_a) SR_HIP(hipMemcpyAsync(dside, side_a, nb * 4, hipMemcpyHostToDevice, st));
  }
  sr::launch_score_fuse(da_s, da_r, ka, db_s, db_r, kb, side_a ? dside : nullptr, B, mode, alpha,
                        floor_a, floor_b, min_score, k_out, do_s, do_r, out_a ? do_a : nullptr,
                        out_b ? do_b : nullptr, st, side_b ? dsideb : nullptr);
  SR_HIP(hipMemcpyAsync(out_score, do_s, no * 4, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(out_rows, do_r, no * 8, hipMemcpyDeviceToHost, st));
  if (out_a) SR_HIP(hipMemcpyAsync(out_a, do_a, no * 4, hipMemcpyDeviceToHost, st));
  if (out_b) SR_HIP(hipMemcpyAsync(out_b, do_b, no * 4, hipMemcpyDeviceToHost, st));
  SR_HIP(hipStreamSynchronize(st));
  SR_API_END
}

int sr_score_fuse(const float* score_a, const int64_t* rows_a, int ka, const float* score_b,
                  const int64_t* rows_b, int kb, const float* side_a, int B, int mode, float alpha,
                  float floor_a, float floor_b, float min_score, int k_out, float* out_score,
                  int64_t* out_rows, float* out_a, float* out_b, int device) {
  return sr_score_fuse_sides(score_a, rows_a, ka, score_b, rows_b, kb, side_a, nullptr, B, mode, alpha,
                             floor_a, floor_b, min_score, k_out, out_score, out_rows, out_a, out_b,
                             device);
}

int sr_score_fuse_sides_dev(const float* score_a, const int64_t* rows_a, int ka,
                            const float* score_b, const int64_t* rows_b, int kb,
                            const float* side_a, const float* side_b, int B, int mode, float alpha,
                            float floor_a, float floor_b, float min_score, int k_out,
                            float* out_score, int64_t* out_rows, float* out_a, float* out_b,
                            int device, void* stream) {
  SR_API_BEGIN
  sr::fuse_check_args(B, ka, kb, mode, alpha, k_out);
  if (B == 0) return SR_OK;
  fuse_check_buffers(score_a, rows_a, ka, score_b, rows_b, kb, out_score, out_rows);
  sr::DeviceGuard g(device);
  sr::launch_score_fuse(score_a, rows_a, ka, score_b, rows_b, kb, side_a, B, mode, alpha, floor_a,
                        floor_b, min_score, k_out, out_score, out_rows, out_a, out_b,
                        reinterpret_cast<hipStream_t>(stream), side_b);
  SR_API_END
}

int sr_score_fuse_dev(const float* score_a, const int64_t* rows_a, int ka, const float* score_b,
                      const int64_t* rows_b, int kb, const float* side_a, int B, int mode,
                      float alpha, float floor_a, float floor_b, float min_score, int k_out,
                      float* out_score, int64_t* out_rows, float* out_a, float* out_b, int device,
                      void* stream) {
  return sr_score_fuse_sides_dev(score_a, rows_a, ka, score_b, rows_b, kb, side_a, nullptr, B, mode,
                                 alpha, floor_a, floor_b, min_score, k_out, out_score, out_rows, out_a,
                                 out_b, device, stream);
}

int sr_store_score_rows(sr_store* s, const float* q, int B, const int64_t* rows, int K,
                        float* out_sim) {
  SR_API_BEGIN
  SR_NONNULL(s);
  SR_CHECK(B >= 0 && K >= 0, "store.score_rows: negative shape");
  if (B == 0 || K == 0) return SR_OK;
  SR_NONNULL(q);
  SR_NONNULL(rows);
  SR_NONNULL(out_sim);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->score_rows_host(q, B, rows, K, out_sim);
  SR_API_END
}

int sr_store_score_rows_dev(sr_store* s, const void* q, int q_dtype, int B, const int64_t* rows,
                            int K, int64_t row_offset, float* out_sim, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(s);
  SR_CHECK(B >= 0 && K >= 0, "store.score_rows: negative shape");
  SR_CHECK(q_dtype == SR_DTYPE_F32 || q_dtype == SR_DTYPE_F16,
           "store.score_rows: query dtype must be fp32 or fp16");
  if (B == 0 || K == 0) return SR_OK;
  SR_NONNULL(q);
  SR_NONNULL(rows);
  SR_NONNULL(out_sim);
  std::lock_guard<std::mutex> lk(s->impl->mu);
  s->impl->score_rows_dev(q, q_dtype, B, rows, K, row_offset, out_sim,
                          reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_hybrid_search_fused(sr_store* s, sr_lex* x, const float* q, const int64_t* qoff,
                           const int32_t* qterms, int B, int k, int k_each, int mode, float alpha,
                           float min_score, const uint8_t* allow, int64_t mask_key,
                           float* out_score, int64_t* out_rows, float* out_dense, float* out_lex) {
  SR_API_BEGIN
  SR_CHECK(B >= 0, "hybrid: negative batch");
  SR_CHECK(k_each >= 1 && k_each <= SR_MAX_TOPK, "hybrid: k_each must be in [1, 1024]");
  SR_CHECK(k >= 1 && k <= 2 * k_each, "hybrid: k must be in [1, 2 * k_each]");
  sr::fuse_check_args(B, k_each, k_each, mode, alpha, k, /*allow_full=*/true);
  SR_NONNULL(s);
  SR_NONNULL(x);
  lex_need_mode(x, SR_LEX_BM25, "sr_hybrid_search_fused");
  if (B == 0) return SR_OK;
  SR_NONNULL(q);
  SR_NONNULL(qoff);
  SR_NONNULL(out_score);
  SR_NONNULL(out_rows);
  std::scoped_lock lk(s->impl->mu, x->impl->mu);
  sr::Store& st = *s->impl;
  sr::LexIndex& lx = *x->impl;
  SR_CHECK(st.device() == lx.device(), "hybrid: store and lexical index on different devices");
  int64_t lrows = 0;
  lx.stats(&lrows, nullptr, nullptr, nullptr, nullptr);
  SR_CHECK(lrows == st.rows(), "hybrid: store and lexical index hold different row counts");
  sr::DeviceGuard g(st.device());
  hipStream_t sm = lx.stream();
  const size_t ne = (size_t)B * k_each, no = (size_t)B * k;
  float *dq, *dsim, *lsc, *side, *sideb, *os, *oa, *ob;
  int64_t *drow, *lrow, *orow;
  sr::Carve c;
  c.part((size_t)B * st.dim(), &dq);
  c.part(ne, &drow, &dsim, &sideb);  // the dense list, and its rows' exact BM25 ("floor_full")
  c.part(ne, &lrow, &lsc, &side);    // the BM25 list, and its rows' exact cosines (floor modes)
  c.part(no, &orow, &os, &oa, &ob);
  sr::DevBuf ws;
  ws.carve(c);
  const bool full = mode == SR_FUSE_FLOOR_FULL;
  const bool floor_mode = mode == SR_FUSE_FLOOR || full;
  const uint8_t* elig = st.eligibility(allow, mask_key);
  lx.begin(sm);
  SR_HIP(hipMemcpyAsync(dq, q, (size_t)B * st.dim() * 4, hipMemcpyHostToDevice, sm));
  st.search_dev(dq, SR_DTYPE_F32, B, k_each, dsim, drow, 0, sm, elig);
  lx.search_dev(qoff, qterms, B, k_each, allow, mask_key, lsc, lrow, sm);
  if (floor_mode) st.score_rows_dev(dq, SR_DTYPE_F32, B, lrow, k_each, 0, side, sm);
  // the exact BM25 of the dense rows; a row that matches nothing (score 0) stays unknown
  if (full) lx.score_rows_dev(qoff, qterms, B, drow, k_each, nullptr, 0, sideb, nullptr, sm, -INFINITY);
  sr::launch_score_fuse(dsim, drow, k_each, lsc, lrow, k_each, floor_mode ? side : nullptr, B,
                        full ? SR_FUSE_FLOOR : mode, alpha, -1.0f, 0.0f, min_score, k, os, orow,
                        out_dense ? oa : nullptr, out_lex ? ob : nullptr, sm, full ? sideb : nullptr);
  SR_HIP(hipMemcpyAsync(out_score, os, no * 4, hipMemcpyDeviceToHost, sm));
  SR_HIP(hipMemcpyAsync(out_rows, orow, no * 8, hipMemcpyDeviceToHost, sm));
  if (out_dense) SR_HIP(hipMemcpyAsync(out_dense, oa, no * 4, hipMemcpyDeviceToHost, sm));
  if (out_lex) SR_HIP(hipMemcpyAsync(out_lex, ob, no * 4, hipMemcpyDeviceToHost, sm));
  lx.end(sm);
  SR_HIP(hipStreamSynchronize(sm));
  SR_API_END
}

int sr_encoder_create(const sr_encoder_config* cfg, int device, sr_encoder** out) {
  SR_API_BEGIN
  SR_NONNULL(cfg);
  SR_NONNULL(out);
  *out = nullptr;
  auto* e = new sr_encoder{new sr::Encoder(*cfg, device)};
  *out = e;
  SR_API_END
}

int sr_encoder_set_weight(sr_encoder* e, const char* name, const float* data, int64_t numel) {
  SR_API_BEGIN
  SR_NONNULL(e);
  SR_NONNULL(name);
  std::lock_guard<std::mutex> lk(e->impl->mu);
  e->impl->set_weight(name, data, numel);
  SR_API_END
}

int sr_encoder_ready(sr_encoder* e) {
  SR_API_BEGIN
  SR_NONNULL(e);
  std::lock_guard<std::mutex> lk(e->impl->mu);
  const std::string m = e->impl->missing();
  if (!m.empty()) throw sr::Error(SR_ERR_STATE, "encoder: weight not set: " + m);
  SR_API_END
}

int sr_encoder_forward(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                       const int32_t* type_ids, int B, int S, int pool, float* out) {
  SR_API_BEGIN
  SR_NONNULL(e);
  std::lock_guard<std::mutex> lk(e->impl->mu);
  e->impl->forward_host(ids, mask, type_ids, B, S, 0, pool, out);
  SR_API_END
}

int sr_encoder_forward_dev(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                           const int32_t* type_ids, int B, int S, int pool, void* out,
                           int out_dtype, int ld_out, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(e);
  if (B > 0) {
    SR_NONNULL(ids);
    SR_NONNULL(mask);
    SR_NONNULL(out);
  }
  std::lock_guard<std::mutex> lk(e->impl->mu);
  e->impl->forward_dev(ids, mask, type_ids, B, S, 0, pool, out, out_dtype, ld_out,
                       reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_sparse_terms_dev(const int32_t* ids, const int32_t* mask, const float* tok_weight, int B, int S,
                        const int32_t* special_ids, int n_special, int32_t* out_terms,
                        float* out_weights, int32_t* out_count, int device, void* stream) {
  SR_API_BEGIN
  sr::sparse_terms_check_args(B, S, n_special);
  if (n_special > 0) SR_NONNULL(special_ids);
  if (B == 0) return SR_OK;
  SR_NONNULL(ids);
  SR_NONNULL(mask);
  SR_NONNULL(tok_weight);
  SR_NONNULL(out_terms);
  SR_NONNULL(out_weights);
  SR_NONNULL(out_count);
  sr::DeviceGuard g(device);
  sr::launch_sparse_terms(ids, mask, tok_weight, B, S, special_ids, n_special, out_terms, out_weights,
                          out_count, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_encoder_forward_sparse_dev(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                                  const int32_t* type_ids, int B, int S, int pool, void* out_dense,
                                  int out_dtype, int ld_out, const int32_t* special_ids, int n_special,
                                  float* out_tok_weight, int32_t* out_terms, float* out_weights,
                                  int32_t* out_count, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(e);
  if (B > 0) {
    SR_NONNULL(ids);
    SR_NONNULL(mask);
    SR_NONNULL(out_dense);
    SR_NONNULL(out_terms);
    SR_NONNULL(out_weights);
    SR_NONNULL(out_count);
  }
  if (n_special > 0) SR_NONNULL(special_ids);
  std::lock_guard<std::mutex> lk(e->impl->mu);
  const sr::Encoder::SparseOut so{special_ids, n_special, out_tok_weight, out_terms, out_weights, out_count};
  sr::Encoder::TokenHeads th;
  th.sparse = &so;
  e->impl->forward_dev(ids, mask, type_ids, B, S, 0, pool, out_dense, out_dtype, ld_out,
                       reinterpret_cast<hipStream_t>(stream), &th);
  SR_API_END
}

int sr_encoder_forward_sparse(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                              const int32_t* type_ids, int B, int S, int pool, float* out_dense,
                              const int32_t* special_ids, int n_special, float* out_tok_weight,
                              int32_t* out_terms, float* out_weights, int32_t* out_count) {
  SR_API_BEGIN
  SR_NONNULL(e);
  if (n_special > 0) SR_NONNULL(special_ids);
  std::lock_guard<std::mutex> lk(e->impl->mu);
  const sr::Encoder::SparseOut so{special_ids, n_special, out_tok_weight, out_terms, out_weights, out_count};
  e->impl->forward_host(ids, mask, type_ids, B, S, 0, pool, out_dense, &so);
  SR_API_END
}

int sr_encoder_colbert_dim(sr_encoder* e, int* out) {
  SR_API_BEGIN
  SR_NONNULL(e);
  SR_NONNULL(out);
  std::lock_guard<std::mutex> lk(e->impl->mu);
  *out = e->impl->colbert_dim();
  SR_API_END
}

int sr_encoder_forward_multivec_dev(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                                    const int32_t* type_ids, int B, int S, int pool, void* out_dense,
                                    int out_dtype, int ld_out, void* out_vecs, int32_t* out_len,
                                    const int32_t* special_ids, int n_special, float* out_tok_weight,
                                    int32_t* out_terms, float* out_weights, int32_t* out_count,
                                    void* stream) {
  SR_API_BEGIN
  SR_NONNULL(e);
  const bool any_sparse = out_tok_weight || out_terms || out_weights || out_count;
  const bool with_sparse = out_terms && out_weights && out_count;
  SR_CHECK(!any_sparse || with_sparse,
           "encoder: the sparse outputs are one group: terms, weights and count together or none");
  if (B > 0) {
    SR_NONNULL(ids);
    SR_NONNULL(mask);
    SR_NONNULL(out_dense);
    SR_NONNULL(out_vecs);
    SR_NONNULL(out_len);
  }
  if (with_sparse && n_special > 0) SR_NONNULL(special_ids);
  std::lock_guard<std::mutex> lk(e->impl->mu);
  const sr::Encoder::SparseOut so{special_ids, n_special, out_tok_weight, out_terms, out_weights, out_count};
  const sr::Encoder::MultiVecOut mo{reinterpret_cast<sr::half_t*>(out_vecs), out_len};
  sr::Encoder::TokenHeads th;
  th.sparse = with_sparse ? &so : nullptr;
  th.multivec = &mo;
  e->impl->forward_dev(ids, mask, type_ids, B, S, 0, pool, out_dense, out_dtype, ld_out,
                       reinterpret_cast<hipStream_t>(stream), &th);
  SR_API_END
}

int sr_encoder_forward_multivec(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                                const int32_t* type_ids, int B, int S, int pool, float* out_dense,
                                float* out_vecs, int32_t* out_len, const int32_t* special_ids,
                                int n_special, float* out_tok_weight, int32_t* out_terms,
                                float* out_weights, int32_t* out_count) {
  SR_API_BEGIN
  SR_NONNULL(e);
  if (out_terms && n_special > 0) SR_NONNULL(special_ids);
  const bool any_sparse = out_tok_weight || out_terms || out_weights || out_count;
  const bool with_sparse = out_terms && out_weights && out_count;
  SR_CHECK(!any_sparse || with_sparse,
           "encoder: the sparse outputs are one group: terms, weights and count together or none");
  std::lock_guard<std::mutex> lk(e->impl->mu);
  const sr::Encoder::SparseOut so{special_ids, n_special, out_tok_weight, out_terms, out_weights, out_count};
  const sr::Encoder::MultiVecHost mo{out_vecs, out_len};
  e->impl->forward_host(ids, mask, type_ids, B, S, 0, pool, out_dense, with_sparse ? &so : nullptr, &mo);
  SR_API_END
}

// ---- multi-vector index ----------------------------------------------------------------------
int sr_mv_create_dtype(int dim, int device, int dtype, sr_mv** out) {
  SR_API_BEGIN
  SR_NONNULL(out);
  *out = nullptr;
  SR_CHECK(dim >= 64 && dim <= 1024 && dim % 64 == 0, "mv: dim must be a multiple of 64, <= 1024");
  SR_CHECK(dtype == SR_DTYPE_F16 || dtype == SR_DTYPE_FP8_E4M3,
           "mv: dtype must be SR_DTYPE_F16 or SR_DTYPE_FP8_E4M3");
  auto* x = new sr_mv{new sr::MultiVecIndex(dim, device, dtype)};
  *out = x;
  SR_API_END
}

int sr_mv_create(int dim, int device, sr_mv** out) {
  return sr_mv_create_dtype(dim, device, SR_DTYPE_F16, out);
}

int sr_mv_info(sr_mv* x, int* dtype, int64_t* pool_bytes) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->info(dtype, pool_bytes);
  SR_API_END
}

int sr_mv_add(sr_mv* x, const int64_t* off, const float* vecs, int64_t n, int64_t* first_row) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->add_host(off, vecs, n, first_row);
  SR_API_END
}

int sr_mv_add_dev(sr_mv* x, const void* vecs, const int32_t* len, int64_t n, int ld_tok,
                  int64_t* first_row, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->add_dev(reinterpret_cast<const sr::half_t*>(vecs), len, n, ld_tok, first_row,
                   reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_mv_remove(sr_mv* x, const int64_t* rows, int64_t n) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->remove(rows, n);
  SR_API_END
}

int sr_mv_stats(sr_mv* x, int64_t* n_rows, int64_t* n_live, int64_t* n_tokens) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->stats(n_rows, n_live, n_tokens);
  SR_API_END
}

int sr_mv_get(sr_mv* x, int64_t row, float* out, int64_t cap, int64_t* n_tok) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->get(row, out, cap, n_tok);
  SR_API_END
}

int sr_mv_score_rows_dev(sr_mv* x, const void* q, const int32_t* q_len, int B, int ld_q,
                         const int64_t* rows, int K, float* out_score, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->score_rows_dev(reinterpret_cast<const sr::half_t*>(q), q_len, B, ld_q, rows, K, out_score,
                          reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_mv_score_rows(sr_mv* x, const float* q, const int32_t* q_len, int B, int ld_q,
                     const int64_t* rows, int K, float* out_score) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->score_rows_host(q, q_len, B, ld_q, rows, K, out_score);
  SR_API_END
}

int sr_mv_search(sr_mv* x, const float* q, const int32_t* q_len, int B, int ld_q, int k,
                 const uint8_t* allow, int64_t slab_rows, float* out_score, int64_t* out_rows) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->search_host(q, q_len, B, ld_q, k, allow, slab_rows, out_score, out_rows);
  SR_API_END
}

int sr_mv_search_dev(sr_mv* x, const void* q, const int32_t* q_len, int B, int ld_q, int k,
                     const uint8_t* allow, int64_t slab_rows, int64_t row_offset, float* out_score,
                     int64_t* out_rows, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->search_dev(reinterpret_cast<const sr::half_t*>(q), q_len, B, ld_q, k, allow, slab_rows, row_offset,
                      out_score, out_rows, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_mv_search_group(int dim, int* queries) {
  SR_API_BEGIN
  SR_NONNULL(queries);
  if (dim < 64 || dim > 1024 || dim % 64 != 0)
    throw sr::Error(SR_ERR_INVALID, "mv: dim must be a multiple of 64, <= 1024");
  *queries = sr::mv_group_queries(dim);
  SR_API_END
}

int sr_mv_dim(sr_mv* x, int* dim) {
  SR_API_BEGIN
  SR_NONNULL(x);
  SR_NONNULL(dim);
  *dim = x->impl->dim();
  SR_API_END
}

int sr_mv_compact(sr_mv* x, int64_t stage_bytes, int64_t* old_to_new) {
  SR_API_BEGIN
  SR_NONNULL(x);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->compact(stage_bytes, old_to_new);
  SR_API_END
}

int sr_mv_save(sr_mv* x, const char* path) {
  SR_API_BEGIN
  SR_NONNULL(x);
  SR_NONNULL(path);
  std::lock_guard<std::mutex> lk(x->impl->mu);
  x->impl->save(path);
  SR_API_END
}

int sr_mv_load(const char* path, int device, sr_mv** out) {
  SR_API_BEGIN
  SR_NONNULL(out);
  *out = nullptr;
  SR_NONNULL(path);
  sr::MultiVecIndex* mv = sr::MultiVecIndex::load(path, device);
  *out = new sr_mv{mv};
  SR_API_END
}

void sr_mv_destroy(sr_mv* x) {
  if (!x) return;
  delete x->impl;
  delete x;
}

int sr_cross_score(sr_encoder* e, const int32_t* ids, const int32_t* mask, const int32_t* type_ids,
                   int P, int S, float* out_logits) {
  SR_API_BEGIN
  SR_NONNULL(e);
  std::lock_guard<std::mutex> lk(e->impl->mu);
  e->impl->forward_host(ids, mask, type_ids, P, S, 1, SR_POOL_CLS, out_logits);
  SR_API_END
}

int sr_cross_score_dev(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                       const int32_t* type_ids, int P, int S, float* out_logits, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(e);
  if (P > 0) {
    SR_NONNULL(ids);
    SR_NONNULL(mask);
    SR_NONNULL(out_logits);
  }
  std::lock_guard<std::mutex> lk(e->impl->mu);
  e->impl->forward_dev(ids, mask, type_ids, P, S, 1, SR_POOL_CLS, out_logits, SR_DTYPE_F32,
                       e->impl->config().hidden, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_encoder_set_fp8(sr_encoder* e, int mode) {
  SR_API_BEGIN
  SR_NONNULL(e);
  std::lock_guard<std::mutex> lk(e->impl->mu);
  e->impl->set_fp8(mode);
  SR_API_END
}

void sr_encoder_destroy(sr_encoder* e) {
  if (!e) return;
  delete e->impl;
  delete e;
}

// ---- pipeline helpers ------------------------------------------------------------------------
int sr_build_pairs_dev(const int32_t* q_tok, const int32_t* q_len, int lq_max, const int32_t* p_tok,
                       const int32_t* p_len, int lp_max, const int64_t* cand_rows, int B, int K,
                       int S, int style, int bos_id, int eos_id, int pad_id, int32_t* out_ids,
                       int32_t* out_mask, int32_t* out_type, int device, void* stream) {
  SR_API_BEGIN
  SR_CHECK(B >= 0 && K >= 1 && lq_max >= 1 && lp_max >= 1, "build_pairs: bad shape");
  if (B > 0) {
    SR_NONNULL(q_tok);
    SR_NONNULL(q_len);
    SR_NONNULL(p_tok);
    SR_NONNULL(p_len);
    SR_NONNULL(cand_rows);
    SR_NONNULL(out_ids);
    SR_NONNULL(out_mask);
  }
  sr::DeviceGuard g(device);
  sr::launch_build_pairs(q_tok, q_len, lq_max, p_tok, p_len, lp_max, cand_rows, B, K, S, style,
                         bos_id, eos_id, pad_id, out_ids, out_mask, out_type,
                         reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_rerank_select_dev(const float* logits, int B, int K, int k_out, int32_t* out_index,
                         int device, void* stream) {
  SR_API_BEGIN
  if (B > 0) {
    SR_NONNULL(logits);
    SR_NONNULL(out_index);
  }
  sr::DeviceGuard g(device);
  sr::launch_rerank_select(logits, B, K, k_out, out_index, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

// ---- diagnostics (libsrmi_diag.so only: include/super_rag_mi355x_diag.h) --------------------
#if SR_WITH_DIAG
int sr_diag_gemm(int variant, int epi, const void* X, int64_t lda, const void* W, const float* bias,
                 const void* R, int64_t ldr, void* Y, int64_t ldy, int M, int N, int K, int device,
                 void* stream) {
  SR_API_BEGIN
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(Y);
  SR_CHECK(epi >= 0 && epi <= 4, "diag_gemm: epi must be 0..4");
  SR_CHECK((epi != 2 && epi != 4) || R, "diag_gemm: residual epilogue needs R");
  sr::DeviceGuard g(device);
  sr::LnFold lf;  // variant | 0x100: split weights, W = [hi | lo] with K = 2 x_k
  if (variant >= 0 && (variant & 0x100)) {
    SR_CHECK(K % 128 == 0, "diag_gemm: split weights need K % 128 == 0");
    lf.x_k = K / 2;
    variant &= 0xff;
  }
  sr::launch_gemm_variant(variant, epi, reinterpret_cast<const sr::half_t*>(X), lda,
                          reinterpret_cast<const sr::half_t*>(W), bias, R, ldr, Y, ldy, M, N, K,
                          reinterpret_cast<hipStream_t>(stream), &lf);
  SR_API_END
}

int sr_diag_gemm_chunked(int variant, int epi, const void* X, int64_t lda, const void* W,
                         const float* bias, const void* R, int64_t ldr, void* Y, int64_t ldy, int M,
                         int N, int K, void* ws, int64_t ws_bytes, int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(Y);
  SR_NONNULL(ws);
  SR_CHECK(epi >= 0 && epi <= 4, "diag_gemm_chunked: epi must be 0..4");
  SR_CHECK((epi != 2 && epi != 4) || R, "diag_gemm_chunked: residual epilogue needs R");
  SR_CHECK(ws_bytes > 0, "diag_gemm_chunked: the workspace must not be empty");
  sr::DeviceGuard g(device);
  sr::LnFold lf;  // the embedders' lin(): chunked sums, split-K when the workspace holds the tiles
  if (variant >= 0 && (variant & 0x100)) {
    SR_CHECK(K % 128 == 0, "diag_gemm_chunked: split weights need K % 128 == 0");
    lf.x_k = K / 2;
  }
  lf.chunk_ws = static_cast<float*>(ws);
  lf.chunk_ws_bytes = ws_bytes;
  sr::launch_gemm_variant(sr::GEMM_SMALL, epi, reinterpret_cast<const sr::half_t*>(X), lda,
                          reinterpret_cast<const sr::half_t*>(W), bias, R, ldr, Y, ldy, M, N, K,
                          reinterpret_cast<hipStream_t>(stream), &lf);
  SR_API_END
}

int sr_diag_gemm_stats(const void* X, int64_t lda, const void* W, const float* bias, const void* R,
                       int64_t ldr, void* Y, int64_t ldy, int M, int N, int K, float* stat_out,
                       int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(R);
  SR_NONNULL(Y);
  SR_NONNULL(stat_out);
  SR_CHECK(N % 256 == 0, "diag_gemm_stats: N % 256 == 0");
  sr::DeviceGuard g(device);
  sr::LnFold lf;
  lf.stat_out = stat_out;
  sr::launch_gemm(sr::EPI_RES16_STATS, reinterpret_cast<const sr::half_t*>(X), lda,
                  reinterpret_cast<const sr::half_t*>(W), bias, R, ldr, Y, ldy, M, N, K,
                  reinterpret_cast<hipStream_t>(stream), &lf);
  SR_API_END
}

int sr_diag_gemm_lnr_stats(const void* X, int64_t lda, const void* W, const float* bias, const void* R,
                           int64_t ldr, const float* mr, const float* gamma, void* Y, int64_t ldy, int M,
                           int N, int K, float* stat_out, int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(R);
  SR_NONNULL(mr);
  SR_NONNULL(gamma);
  SR_NONNULL(Y);
  SR_NONNULL(stat_out);
  SR_CHECK(N % 256 == 0, "diag_gemm_lnr_stats: N % 256 == 0");
  sr::DeviceGuard g(device);
  sr::LnFold lf;
  lf.mr = mr;
  lf.gamma = gamma;
  lf.stat_out = stat_out;
  sr::launch_gemm(sr::EPI_LNR16_STATS, reinterpret_cast<const sr::half_t*>(X), lda,
                  reinterpret_cast<const sr::half_t*>(W), bias, R, ldr, Y, ldy, M, N, K,
                  reinterpret_cast<hipStream_t>(stream), &lf);
  SR_API_END
}

int sr_diag_gemm_stats_y8(int lnr, const void* X, int64_t lda, const void* W, const float* bias,
                          const void* R, int64_t ldr, const float* mr, const float* gamma, void* Y,
                          int64_t ldy, uint8_t* y8, int M, int N, int K, float* stat_out, int device,
                          void* stream) {
  SR_API_BEGIN
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(R);
  SR_NONNULL(Y);
  SR_NONNULL(y8);
  SR_NONNULL(stat_out);
  SR_CHECK(N % 256 == 0, "diag_gemm_stats_y8: N % 256 == 0");
  SR_CHECK(!lnr || (mr && gamma), "diag_gemm_stats_y8: the LNR form needs mr and gamma");
  sr::DeviceGuard g(device);
  sr::LnFold lf;
  lf.mr = lnr ? mr : nullptr;
  lf.gamma = lnr ? gamma : nullptr;
  lf.stat_out = stat_out;
  lf.y8 = y8;
  sr::launch_gemm(lnr ? sr::EPI_LNR16_STATS_Y8 : sr::EPI_RES16_STATS_Y8, reinterpret_cast<const sr::half_t*>(X),
                  lda, reinterpret_cast<const sr::half_t*>(W), bias, R, ldr, Y, ldy, M, N, K,
                  reinterpret_cast<hipStream_t>(stream), &lf);
  SR_API_END
}

int sr_diag_gemm_fold(int f8, int epi, const void* X, int64_t lda, const void* W, const uint8_t* wexp,
                      const float* bias, const float* colsum, const void* R, int64_t ldr, const float* mr,
                      int64_t stat_ld, const float* gamma, void* Y, int64_t ldy, uint8_t* y8,
                      float* stat_out, int M, int N, int K, int device, void* stream) {
  SR_API_BEGIN
  const bool lnf = epi == sr::EPI_LNF_F16;
  const bool lnr = epi == sr::EPI_LNR16_STATS || epi == sr::EPI_LNR16_STATS_Y8;
  const bool with_y8 = epi == sr::EPI_RES16_STATS_Y8 || epi == sr::EPI_LNR16_STATS_Y8;
  const bool stats = lnr || epi == sr::EPI_RES16_STATS || epi == sr::EPI_RES16_STATS_Y8;
  SR_CHECK(lnf || stats, "diag_gemm_fold: epi must be LNF_F16 (5), RES16_STATS (7), LNR16_STATS (8) or "
                         "their e4m3-copy forms (12, 13)");
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(Y);
  SR_CHECK(M > 0 && N > 0 && N % 256 == 0, "diag_gemm_fold: M > 0, N a positive multiple of 256");
  SR_CHECK(!f8 || wexp, "diag_gemm_fold: fp8 needs wexp");
  SR_CHECK(f8 ? (K % 128 == 0 && K >= 256) : (K % 64 == 0 && K >= 64),
           "diag_gemm_fold: K % 128 == 0, K >= 256 (fp8) / K % 64 == 0 (fp16)");
  SR_CHECK(lda >= K && lda % (f8 ? 16 : 8) == 0, "diag_gemm_fold: lda >= K, 16-byte rows");
  SR_CHECK(ldy >= N && ldy % 8 == 0, "diag_gemm_fold: ldy >= N, ldy % 8 == 0");
  SR_CHECK(!stats || (R && ldr >= N && ldr % 8 == 0), "diag_gemm_fold: the residual epilogues need R, ldr >= N, ldr % 8 == 0");
  SR_CHECK(!(lnf || lnr) || (mr && stat_ld >= 0), "diag_gemm_fold: LN-folded epilogues need mr, stat_ld >= 0");
  SR_CHECK(!lnf || colsum, "diag_gemm_fold: LNF needs colsum");
  SR_CHECK(!lnr || gamma, "diag_gemm_fold: LNR needs gamma");
  SR_CHECK(!stats || stat_out, "diag_gemm_fold: the *_STATS epilogues need stat_out");
  SR_CHECK(!with_y8 || y8, "diag_gemm_fold: the e4m3-copy epilogues need y8");
  sr::DeviceGuard g(device);
  sr::LnFold lf;
  lf.mr = (lnf || lnr) ? mr : nullptr;
  lf.stat_ld = (lnf || lnr) ? stat_ld : 1;
  lf.colsum = lnf ? colsum : nullptr;
  lf.gamma = lnr ? gamma : nullptr;
  lf.stat_out = stats ? stat_out : nullptr;
  lf.y8 = with_y8 ? y8 : nullptr;
  lf.wexp = f8 ? wexp : nullptr;
  if (f8)
    sr::launch_gemm_f8w(epi, reinterpret_cast<const uint8_t*>(X), lda, reinterpret_cast<const uint8_t*>(W), bias,
                        stats ? R : nullptr, stats ? ldr : 0, Y, ldy, M, N, K,
                        reinterpret_cast<hipStream_t>(stream), &lf);
  else
    sr::launch_gemm(epi, reinterpret_cast<const sr::half_t*>(X), lda, reinterpret_cast<const sr::half_t*>(W),
                    bias, stats ? R : nullptr, stats ? ldr : 0, Y, ldy, M, N, K,
                    reinterpret_cast<hipStream_t>(stream), &lf);
  SR_API_END
}

int sr_diag_quantize_rows_fp8(const void* W, int N, int K, uint8_t* W8, uint8_t* wexp, int device,
                              void* stream) {
  SR_API_BEGIN
  SR_NONNULL(W);
  SR_NONNULL(W8);
  SR_NONNULL(wexp);
  SR_CHECK(N > 0 && K > 0, "diag_quantize_rows_fp8: N > 0, K > 0");
  sr::DeviceGuard g(device);
  sr::launch_quantize_rows_fp8(reinterpret_cast<const sr::half_t*>(W), N, K, W8, wexp,
                               reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_diag_colsum_fp8(const uint8_t* W8, const uint8_t* wexp, int N, int K, float* colsum, int device,
                       void* stream) {
  SR_API_BEGIN
  SR_NONNULL(W8);
  SR_NONNULL(wexp);
  SR_NONNULL(colsum);
  SR_CHECK(N > 0 && K > 0, "diag_colsum_fp8: N > 0, K > 0");
  sr::DeviceGuard g(device);
  sr::launch_colsum_fp8(W8, wexp, N, K, colsum, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_diag_fold_ln_weight(const float* w32, const float* gamma, const float* beta, const float* bias,
                           int N, int K, void* w16, float* colsum, float* bias_out, int device,
                           void* stream) {
  SR_API_BEGIN
  SR_NONNULL(w32);
  SR_NONNULL(gamma);
  SR_NONNULL(beta);
  SR_NONNULL(bias);
  SR_NONNULL(w16);
  SR_NONNULL(colsum);
  SR_NONNULL(bias_out);
  SR_CHECK(N > 0 && K > 0, "diag_fold_ln_weight: N > 0, K > 0");
  sr::DeviceGuard g(device);
  sr::launch_fold_ln_weight(w32, gamma, beta, bias, N, K, reinterpret_cast<sr::half_t*>(w16), colsum,
                            bias_out, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_diag_ln_stats_finalize(const float* stat, int nparts, float eps, int M, float* mr, int device,
                              void* stream) {
  SR_API_BEGIN
  SR_NONNULL(stat);
  SR_NONNULL(mr);
  SR_CHECK(M > 0, "diag_ln_stats_finalize: M > 0");
  SR_CHECK(nparts >= 1 && nparts <= 16, "diag_ln_stats_finalize: 1..16 partials per row");
  SR_CHECK(eps > 0.f, "diag_ln_stats_finalize: eps > 0");
  sr::DeviceGuard g(device);
  sr::launch_ln_stats_finalize(stat, nparts, eps, M, mr, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_diag_mfma_rate(int f8, int blocks, int iters, float* sink, uint64_t* stamps, int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(sink);
  SR_NONNULL(stamps);
  sr::DeviceGuard g(device);
  sr::launch_mfma_rate(f8, blocks, iters, sink, stamps, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_diag_gemm_lnr_stats_stamps(const void* X, int64_t lda, const void* W, const float* bias, const void* R,
                                  int64_t ldr, const float* mr, const float* gamma, void* Y, int64_t ldy, int M,
                                  int N, int K, float* stat_out, uint64_t* stamps, int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(R);
  SR_NONNULL(mr);
  SR_NONNULL(gamma);
  SR_NONNULL(Y);
  SR_NONNULL(stat_out);
  SR_NONNULL(stamps);
  sr::DeviceGuard g(device);
  sr::launch_lnr_stats_stamps(reinterpret_cast<const sr::half_t*>(X), lda, reinterpret_cast<const sr::half_t*>(W),
                              bias, R, ldr, mr, gamma, Y, ldy, M, N, K, stat_out, stamps,
                              reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_diag_ffn1(int diag, int f8, const void* X, int64_t lda, const void* W, const uint8_t* wexp,
                 const float* bias, const float* colsum, const float* mr, void* Y, int64_t ldy, int M,
                 int N, int K, int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(colsum);
  SR_NONNULL(mr);
  SR_NONNULL(Y);
  SR_CHECK(!f8 || wexp, "diag_ffn1: fp8 needs wexp");
  sr::DeviceGuard g(device);
  sr::launch_ffn1_diag(diag, f8 != 0, X, lda, W, wexp, bias, colsum, mr, Y, ldy, M, N, K,
                       reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_diag_ffn1_stamps(int diag, const void* X, int64_t lda, const void* W, const float* bias,
                        const float* colsum, const float* mr, void* Y, int64_t ldy, int M, int N,
                        int K, uint64_t* stamps, int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(colsum);
  SR_NONNULL(mr);
  SR_NONNULL(Y);
  SR_NONNULL(stamps);
  sr::DeviceGuard g(device);
  sr::launch_ffn1_diag(diag, false, X, lda, W, nullptr, bias, colsum, mr, Y, ldy, M, N, K,
                       reinterpret_cast<hipStream_t>(stream), stamps);
  SR_API_END
}

int sr_diag_copy(const void* src, void* dst, int64_t bytes, int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(src);
  SR_NONNULL(dst);
  SR_CHECK(bytes >= 0 && bytes % 16 == 0, "diag_copy: bytes must be a non-negative multiple of 16");
  sr::DeviceGuard g(device);
  sr::launch_copy16(src, dst, bytes, reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_diag_qkv_attention_stamps(const void* X, int64_t lda, const void* W, const float* bias,
                                 const float* colsum, const float* mr, const int32_t* mask, void* ctx, int B,
                                 int S, int d, int heads, uint64_t* stamps, int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(colsum);
  SR_NONNULL(mr);
  SR_NONNULL(mask);
  SR_NONNULL(ctx);
  SR_NONNULL(stamps);
  sr::DeviceGuard g(device);
  sr::LnFold lf;
  lf.mr = mr;
  lf.colsum = colsum;
  sr::launch_qkv_attention(sr::EPI_LNF_F16, reinterpret_cast<const sr::half_t*>(X), lda,
                           reinterpret_cast<const sr::half_t*>(W), bias, &lf, mask,
                           reinterpret_cast<sr::half_t*>(ctx), B, S, d, heads,
                           reinterpret_cast<hipStream_t>(stream), nullptr, stamps);
  SR_API_END
}

int sr_diag_qkv_attention(int epi, const void* X, int64_t lda, const void* W, const float* bias,
                          const float* colsum, const float* mr, const int32_t* mask, void* ctx, int B, int S,
                          int d, int heads, int device, void* stream) {
  SR_API_BEGIN
  SR_CHECK(epi == sr::EPI_BIAS_F16 || epi == sr::EPI_LNF_F16,
           "diag_qkv_attention: epi must be BIAS_F16 (0) or LNF_F16 (5)");
  SR_NONNULL(X);
  SR_NONNULL(W);
  SR_NONNULL(bias);
  SR_NONNULL(mask);
  SR_NONNULL(ctx);
  SR_CHECK(epi != sr::EPI_LNF_F16 || (colsum && mr), "diag_qkv_attention: LNF needs colsum and mr");
  sr::DeviceGuard g(device);
  sr::LnFold lf;
  const bool lnf = epi == sr::EPI_LNF_F16;
  lf.mr = lnf ? mr : nullptr;
  lf.colsum = lnf ? colsum : nullptr;
  sr::launch_qkv_attention(epi, reinterpret_cast<const sr::half_t*>(X), lda,
                           reinterpret_cast<const sr::half_t*>(W), bias, lnf ? &lf : nullptr, mask,
                           reinterpret_cast<sr::half_t*>(ctx), B, S, d, heads,
                           reinterpret_cast<hipStream_t>(stream), nullptr, nullptr);
  SR_API_END
}

int sr_diag_cls_attn_fold(const void* w, const void* U, const float* mr, const int32_t* mask, int B, int S,
                          int D, int H, void* z, int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(w);
  SR_NONNULL(U);
  SR_NONNULL(mr);
  SR_NONNULL(mask);
  SR_NONNULL(z);
  sr::DeviceGuard g(device);
  sr::launch_cls_attn_fold(reinterpret_cast<const sr::half_t*>(w), reinterpret_cast<const sr::half_t*>(U), mr,
                           mask, B, S, D, H, reinterpret_cast<sr::half_t*>(z),
                           reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_diag_kv_blockdiag(const void* wqkv_f, int D, int H, void* wk_bd, void* wv_bd, int device,
                         void* stream) {
  SR_API_BEGIN
  SR_NONNULL(wqkv_f);
  SR_NONNULL(wk_bd);
  SR_NONNULL(wv_bd);
  SR_CHECK(H >= 1 && D >= H && D % H == 0, "diag_kv_blockdiag: H >= 1 and D a multiple of H");
  sr::DeviceGuard g(device);
  sr::launch_kv_blockdiag(reinterpret_cast<const sr::half_t*>(wqkv_f), D, H,
                          reinterpret_cast<sr::half_t*>(wk_bd), reinterpret_cast<sr::half_t*>(wv_bd),
                          reinterpret_cast<hipStream_t>(stream));
  SR_API_END
}

int sr_diag_attention(int variant, const void* qkv, const int32_t* mask, void* ctx, int B, int S,
                      int Sq, int d, int heads, int device, void* stream) {
  SR_API_BEGIN
  SR_NONNULL(qkv);
  SR_NONNULL(mask);
  SR_NONNULL(ctx);
  SR_CHECK(variant >= -1 && variant <= 3, "diag_attention: variant must be -1 .. 3");
  SR_CHECK(variant < 1 || (heads > 0 && d == 64 * heads && S <= 512),
           "diag_attention: variants 1-3 need head dim 64 and S <= 512");
  sr::DeviceGuard g(device);
  sr::attention_force_variant(variant);
  try {
    sr::launch_attention(reinterpret_cast<const sr::half_t*>(qkv), mask,
                         reinterpret_cast<sr::half_t*>(ctx), B, S, Sq, d, heads,
                         reinterpret_cast<hipStream_t>(stream));
  } catch (...) {
    sr::attention_force_variant(-1);
    throw;
  }
  sr::attention_force_variant(-1);
  SR_API_END
}
#endif  // SR_WITH_DIAG

// ---- profiling -------------------------------------------------------------------------------
int sr_profile_enable(int on) {
  SR_API_BEGIN
  std::lock_guard<std::mutex> lk(sr::g_prof_mu);
  if (on) {
    sr::drain_pending_locked();
    sr::g_prof_agg.clear();
  }
  sr::g_prof_on = on != 0;
  SR_API_END
}

int sr_profile_read(sr_kernel_stat* out, int max, int* n) {
  SR_API_BEGIN
  SR_NONNULL(n);
  std::lock_guard<std::mutex> lk(sr::g_prof_mu);
  sr::drain_pending_locked();
  int i = 0;
  for (const auto& kv : sr::g_prof_agg) {
    if (i >= max || !out) break;
    sr_kernel_stat& st = out[i++];
    std::memset(&st, 0, sizeof(st));
    std::strncpy(st.name, kv.first.c_str(), sizeof(st.name) - 1);
    st.launches = kv.second.launches;
    st.total_ms = kv.second.ms;
    st.flops = kv.second.flops;
    st.bytes = kv.second.bytes;
  }
  *n = i;
  SR_API_END
}

}  // extern "C"
