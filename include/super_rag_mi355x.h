/*
 * super_rag_mi355x.h — C-ABI of the MI355X (gfx950) embed -> retrieve -> rerank hot path.
 *
 * This library replaces the arithmetic that promoteAI/super-rag sends out of process:
 *   - the SeekDB HNSW cosine search behind
 *       super_rag/vectorstore/seekdb_connector.py:98-115  (SeekDBVectorStoreConnector.search)
 *       super_rag/vectorstore/seekdb_connector.py:56-96   (create_collection / add / delete)
 *     -> sr_store_*  (in-HBM exact cosine top-k, fp16 rows, MFMA scan + fused threshold filter)
 *   - the remote embedding server reached by litellm.embedding() at
 *       super_rag/llm/embed/embedding_service.py:153-194  (EmbeddingService._embed_batch)
 *     -> sr_encoder_forward*  (BERT / XLM-R encoder, CLS or masked-mean pool, L2 normalise)
 *   - the remote cross-encoder reached by litellm.arerank() at
 *       super_rag/llm/rerank/rerank_service.py:87-153    (RerankService._rank_texts)
 *     -> sr_cross_score*  (XLM-R encoder + RoBERTa classification head -> one logit per pair)
 *
 * Conventions
 *   - Every int-returning entry point returns SR_OK (0) on success and a negative SR_ERR_* code on
 *     failure; the message is available from sr_last_error() (thread-local, valid until the next
 *     call on the same thread).
 *   - Host pointers are caller-owned and only read/written during the call.  Device pointers
 *     (the *_dev entry points) must live on the object's device; `stream` is a hipStream_t used
 *     as given (NULL = the HIP null stream, which is what PyTorch reports for its default
 *     stream) and the call is asynchronous on it unless stated.  Host-pointer entry points run
 *     on the object's own stream and are blocking.
 *   - Objects are internally locked: every entry point is safe to call from several host threads.
 *     The Python binding calls through ctypes.CDLL, which releases the GIL for the duration.
 *   - Scores follow SeekDB's cosine semantics: dist = 1 - cos(q, x)  (lower is better,
 *     seekdb_connector.py:143 passes the distance through as DocumentWithScore.score).
 *     Ties are broken by ascending row id.  Missing results (k > live rows) are reported as
 *     row = -1, dist = +inf.
 */
#ifndef SUPER_RAG_MI355X_H
#define SUPER_RAG_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define SR_OK 0
#define SR_ERR_INVALID (-1)   /* bad argument / shape                                   */
#define SR_ERR_HIP (-2)       /* HIP runtime or kernel launch failure                    */
#define SR_ERR_OOM (-3)       /* device allocation failed                                */
#define SR_ERR_IO (-4)        /* snapshot read/write failure                             */
#define SR_ERR_STATE (-5)     /* object not ready (e.g. encoder weights missing)         */

#define SR_DTYPE_F32 0
#define SR_DTYPE_F16 1
#define SR_DTYPE_FP8_E4M3 2   /* OCP e4m3fn (scan copy of the store, sr_store_set_scan_dtype)  */

#define SR_POOL_CLS 0         /* BGE models: hidden state of the first token             */
#define SR_POOL_MEAN 1        /* attention-mask weighted mean over tokens                */

#define SR_MAX_TOPK 1024

typedef struct sr_store sr_store;
typedef struct sr_encoder sr_encoder;

const char* sr_last_error(void);
int sr_version(void);
/* Number of visible HIP devices (0 on a host without a GPU; never fails on such a host). */
int sr_device_count(int* out);
/* Copy `bytes` between host and device memory of `device` (kind: 0 = H2D, 1 = D2H, 2 = D2D). */
int sr_memcpy(void* dst, const void* src, int64_t bytes, int kind, int device);

/* ------------------------------------------------------------------------------------------------
 * Vector store  (replaces SeekDBVectorStoreConnector, seekdb_connector.py:31-155)
 * Rows are L2-normalised on insertion and kept as fp16 in HBM, row-major, dim padded to 64.
 * ---------------------------------------------------------------------------------------------- */

/* create_collection(vector_size=dim) — seekdb_connector.py:56-66 (HNSW, distance="cosine"). */
int sr_store_create(int dim, int device, int64_t initial_capacity, sr_store** out);
/* add(nodes) — seekdb_connector.py:68-85: n host fp32 rows (n x dim); out_rows[i] = row id. */
int sr_store_add(sr_store* s, const float* vecs, int64_t n, int64_t* out_rows);
/* Same, rows already on the device (dtype SR_DTYPE_F32 or SR_DTYPE_F16, n x dim, row-major).
 * Row ids are first_row .. first_row + n - 1. */
int sr_store_add_dev(sr_store* s, const void* vecs, int dtype, int64_t n, int64_t* first_row,
                     void* stream);
/* delete(ids=...) — seekdb_connector.py:90-96: tombstones rows (ignored ids are an error). */
int sr_store_remove(sr_store* s, const int64_t* rows, int64_t n);
int sr_store_count(sr_store* s, int64_t* n_rows, int64_t* n_live);
int sr_store_dim(sr_store* s, int* dim);
/* Read back stored (normalised, fp16-rounded) rows as fp32, for with_vectors / parity checks. */
int sr_store_get(sr_store* s, const int64_t* rows, int64_t n, float* out);
/* search(QueryWithEmbedding) — seekdb_connector.py:98-115 (collection.query n_results=top_k).
 * q: B x dim host fp32 (normalised internally).  out_dist / out_rows: B x k host buffers, each
 * query's results sorted by (dist asc, row asc).  Blocking. */
int sr_store_search(sr_store* s, const float* q, int B, int k, float* out_dist, int64_t* out_rows);
/* Filtered search (the score_threshold / filter kwargs the reference passes and SeekDB's
 * connector ignores, context/context.py:37-47, :74-111): only rows with
 * allow[row] != 0 (host, n_rows bytes) compete, so a query still gets its k best ELIGIBLE rows.
 * The eligibility mask (allow & live) is kept on the device and reused while mask_key (non-zero)
 * and the store contents are unchanged; mask_key 0 uploads it every call. */
int sr_store_search_masked(sr_store* s, const float* q, int B, int k, const uint8_t* allow,
                           int64_t mask_key, float* out_dist, int64_t* out_rows);
/* sr_store_search / sr_store_search_masked (allow may be NULL) returning the similarities
 * (descending, -inf when missing) instead of 1 - sim: for callers that merge several stores' lists
 * (two neighbouring fp32 similarities can round to one fp32 distance). */
int sr_store_search_sim(sr_store* s, const float* q, int B, int k, const uint8_t* allow,
                        int64_t mask_key, float* out_sim, int64_t* out_rows);
/* Device variant: q is B x dim on the device (SR_DTYPE_F32 or SR_DTYPE_F16), out_sim/out_rows
 * device buffers of B x k (similarity = 1 - dist, rows int64; -1 / -inf when missing).
 * row_offset is added to every returned row (global row id of a shard).  Synchronises `stream`
 * once at the end to check the candidate-overflow flag (and reruns the exact slow path if set). */
int sr_store_search_dev(sr_store* s, const void* q, int q_dtype, int B, int k, float* out_sim,
                        int64_t* out_rows, int64_t row_offset, void* stream);
/* Each query searches only the rows of its own list (pre-filtered search: the chat_id / indexer
 * filters of context/context.py:74-111 resolved to row lists by the caller).  lists: CSR
 * (list_off[n_lists + 1], list_off[0] == 0; list_rows strictly ascending inside a list, every row in
 * [0, n_rows)); q_list[b] in [0, n_lists) names query b's list (lists may be shared and may be
 * empty).  Tombstoned rows in a list are skipped.  out_sim / out_rows: B x k host buffers,
 * (sim desc, row asc); -inf / -1 past the eligible rows.  Reads the fp16 rows in either scan mode.
 * k obeys sr_store_search's limits; B == 0 is a no-op.  Anything else is SR_ERR_INVALID before any
 * device work.  Blocking.  One launch scores every (query, row of its list) pair, whatever the
 * number of distinct lists (k_subset.hip), where sr_store_search_masked scans the whole store once
 * per mask.  Not provided: a device-pointer (*_dev) variant and an sr_store_set_* counterpart (a
 * caller with several stores splits the lists per store and merges, as the Python ShardedStore
 * does). */
int sr_store_search_subset(sr_store* s, const float* q, int B, int k, const int32_t* q_list,
                           int n_lists, const int64_t* list_off, const int64_t* list_rows,
                           float* out_sim, int64_t* out_rows);
/* Scan precision (BASELINE config 5 "fp8 MFMA GEMM path"): SR_DTYPE_F16 (default) or
 * SR_DTYPE_FP8_E4M3: an fp8 copy of the rows (per-row power-of-two scale) is scanned with the
 * block-scaled fp8 MFMA (half the HBM bytes of the fp16 scan), the top max(2k, k + 32) candidates
 * are re-scored exactly on the fp16 rows, and the exact top k is returned (same result as the fp16
 * scan whenever the fp8 stage keeps the true top k among its candidates; recall measured in
 * tests/test_gpu_store.py and bench).  Quantises every row when switched on. */
int sr_store_set_scan_dtype(sr_store* s, int dtype);
/* Snapshot (checkpoint/resume of the corpus; SeekDB persisted rows server-side). */
int sr_store_save(sr_store* s, const char* path);
int sr_store_load(const char* path, int device, sr_store** out);
/* Drop tombstoned rows; old_to_new (host, n_rows entries, may be NULL) receives the new row id
 * of every old row (-1 for removed rows). */
int sr_store_compact(sr_store* s, int64_t* old_to_new);
void sr_store_destroy(sr_store* s);

/* ------------------------------------------------------------------------------------------------
 * Multi-device collection: SURVEY §8(b)'s sr_store_create(dim, dtype, devices, n_dev) — the
 * reference configures one vector DB per deployment (super_rag/config.py:65-67, adaptor
 * vectorstore/connector.py:4-15); here a collection is row-sharded over the listed devices (the
 * same device may repeat).  Global row ids are the insertion order across shards (each add batch
 * goes to the shard with the fewest rows), so every result equals one sr_store's bit for bit:
 * shards are searched concurrently (K1 + K2 on each device) and merged by (dist asc, row asc).
 * dtype: SR_DTYPE_F16, or SR_DTYPE_FP8_E4M3 for the fp8 scan copy (sr_store_set_scan_dtype).
 * Snapshots, compaction and the device-buffer entry points stay per shard (sr_store_*; the Python
 * connector's ShardedStore composes them). */
typedef struct sr_store_set sr_store_set;
int sr_store_set_create(int dim, int dtype, const int* devices, int n_dev, sr_store_set** out);
int sr_store_set_add(sr_store_set* s, const float* vecs, int64_t n, int64_t* out_rows);
int sr_store_set_remove(sr_store_set* s, const int64_t* rows, int64_t n);
int sr_store_set_count(sr_store_set* s, int64_t* n_rows, int64_t* n_live, int* n_shards);
int sr_store_set_get(sr_store_set* s, const int64_t* rows, int64_t n, float* out);
/* sr_store_search semantics; allow (host, n_rows bytes) may be NULL, else as sr_store_search_masked. */
int sr_store_set_search(sr_store_set* s, const float* q, int B, int k, const uint8_t* allow,
                        int64_t mask_key, float* out_dist, int64_t* out_rows);
int sr_store_set_set_scan_dtype(sr_store_set* s, int dtype);
void sr_store_set_destroy(sr_store_set* s);

/* Merge P per-shard top-k lists (device buffers P x B x k of similarity and global row, as written
 * by sr_store_search_dev) into one B x k_out list per query, on `device`. */
int sr_topk_merge_dev(const float* sims, const int64_t* rows, int P, int B, int k, int k_out,
                      float* out_sim, int64_t* out_rows, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MMR diversification (maximal marginal relevance; graphiti maximal_marginal_relevance,
 * graphiti_core/search/search_utils.py:1884-1922).  All scores are similarities (higher is
 * better).  For one query with unit candidate rows c_i (zero rows stay zero), rel_i = cos(q, c_i)
 * and G_ij = c_i . c_j:
 *   SR_MMR_ONEPASS  the reference function: score_i = lambda rel_i + (lambda - 1) m_i with
 *                   m_i = max(0, max_{j != i} G_ij) (the reference's zero diagonal: a lone
 *                   candidate or one with only negative similarities gets 0); order (score desc,
 *                   candidate position asc); score < min_score dropped; first k_out kept.  Two exact
 *                   duplicates both get m = 1: both are demoted.
 *   SR_MMR_GREEDY   the classical iteration: S starts empty; every step picks the unselected i
 *                   maximising lambda rel_i + (lambda - 1) max(0, max_{j in S} G_ij) (ties: lower
 *                   position) and reports that value as its score; stops after k_out picks, when
 *                   the candidates run out or when the best value is below min_score.  The first
 *                   of two duplicates keeps its rank, the second is demoted.
 * lambda in [0, 1], K (candidates per query) in [1, SR_MMR_MAX_CAND], k_out in [1, K]; anything
 * else is SR_ERR_INVALID before any device call.  The Gram matrix is computed on the fp16 rows with
 * fp32 accumulation by one workgroup per query (128 candidates: the 64 KiB fp32 matrix fits its LDS).
 * ---------------------------------------------------------------------------------------------- */
#define SR_MMR_ONEPASS 0
#define SR_MMR_GREEDY 1
#define SR_MMR_MAX_CAND 128

/* Explicit vectors (graphiti's signature). q: B x dim, cand: B x K x dim host fp32,
 * n_cand[b] <= K valid ones (NULL = K). out_index: positions into the candidate list
 * (-1 past the end), out_score: -inf past the end. Blocking.  The query and the candidates are
 * normalised to fp16 rows exactly as a store normalises the rows it is given. */
int sr_mmr_rerank(const float* q, const float* cand, const int32_t* n_cand, int B, int K,
                  int dim, float lambda, int mode, float min_score, int k_out,
                  float* out_score, int32_t* out_index, int device);

/* Candidates as sr_store_search_dev wrote them (rows carry row_offset, -1 = missing;
 * cand_sims = rel). Device outputs B x k_out: MMR score, cosine of the kept row, row
 * (+row_offset; -inf / -inf / -1 past the end). Asynchronous on stream. */
int sr_store_mmr_dev(sr_store* s, const int64_t* cand_rows, const float* cand_sims, int B,
                     int K, int64_t row_offset, float lambda, int mode, float min_score,
                     int k_out, float* out_score, float* out_sim, int64_t* out_rows,
                     void* stream);

/* Scan top-k_cand (sr_store_search_sim semantics, allow may be NULL), then MMR, keep k.
 * out_dist = 1 - cos of the kept rows (SeekDB's score), in MMR order (+inf past the end; out_score
 * -inf, out_rows -1). Blocking.  Under the fp8 scan mode the candidates carry their exact fp16
 * re-scored similarities and MMR reads the fp16 rows, as in the fp16 mode. */
int sr_store_search_mmr(sr_store* s, const float* q, int B, int k, int k_cand,
                        float lambda, int mode, float min_score, const uint8_t* allow,
                        int64_t mask_key, float* out_score, float* out_dist,
                        int64_t* out_rows);

/* ------------------------------------------------------------------------------------------------
 * Grouped search (Qdrant search_groups, Milvus group_by_field): the k best DISTINCT groups of a
 * query with the best row or rows of each, exact (k_group.hip).  The indexer stores every doc_part of
 * a document_id as a row of its own, so the k nearest rows are often k chunks of one document.
 * group: host int32 [n_rows]; g >= 0 names a group, -1 makes the row a group of its own, any other
 * value is an error.  It is kept on the device and reused while group_key (non-zero) and the store
 * contents are unchanged; group_key 0 uploads (and validates) it every call.
 * Semantics: walk all eligible rows (live, and allowed when allow is given) in the store's order
 * (similarity desc, row asc); a row is kept when its group holds fewer than group_size kept rows and
 * its group is already kept or fewer than k groups are.  Groups come in order of first appearance
 * (the order of their best rows), the rows of a group in walk order.  out_sim / out_rows:
 * B x k x group_size, SIMILARITIES (not distances), -inf / -1 in unfilled slots; out_group: B x k, -1
 * for an unfilled group slot (its first row is -1, which tells it from an ungrouped row's slot).
 * Limits: k in [1, SR_MAX_TOPK], group_size in [1, SR_GROUP_MAX_SIZE], k * group_size <= k_cand <=
 * SR_MAX_TOPK (and sr_store_search's limit on k applies to k_cand); B == 0 is a no-op; anything
 * else, a null buffer or an id below -1 is SR_ERR_INVALID before any device work.
 * Not provided: an sr_store_set_* counterpart (the Python ShardedStore merges per-shard results by
 * the same walk) and grouped MMR / hybrid / subset search.
 * ---------------------------------------------------------------------------------------------- */
#define SR_GROUP_MAX_SIZE 8

/* Blocking, exact.  Scans the top k_cand rows (sr_store_search_sim semantics, allow may be NULL) and
 * collapses them on the device; a query whose k_cand rows do not settle the answer (a few large
 * groups fill the list) continues on its own with the settled groups masked out, at most k more
 * scans, so the result never depends on k_cand.  SR_ERR_STATE if that bound were ever exceeded.
 * Under the fp8 scan mode the candidates carry their exact fp16 re-scored similarities. */
int sr_store_search_grouped(sr_store* s, const float* q, int B, int k, int group_size, int k_cand,
                            const int32_t* group, int64_t group_key,
                            const uint8_t* allow, int64_t mask_key,
                            float* out_sim, int64_t* out_rows, int32_t* out_group);

/* Collapse a candidate list that sr_store_search_dev wrote (device buffers B x K: rows carrying
 * row_offset, -1 = missing; similarities), k * group_size <= K <= SR_MAX_TOPK.  Device outputs as
 * above (rows keep row_offset) plus out_complete [B] int32: 1 when query b's result is already
 * exact (the list was not full, or k groups were found and each holds group_size rows or is an
 * ungrouped row), 0 when only a continuation could tell.  No continuation here.  group is a HOST
 * array, as above.  Asynchronous on stream. */
int sr_store_group_dev(sr_store* s, const int64_t* cand_rows, const float* cand_sims, int B, int K,
                       int64_t row_offset, int k, int group_size,
                       const int32_t* group, int64_t group_key,
                       float* out_sim, int64_t* out_rows, int32_t* out_group,
                       int32_t* out_complete, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Lexical (BM25) index and hybrid dense + lexical retrieval  (BASELINE config 5)
 * The reference declares a `fulltext_search` node type (schema/view_models.py:276-283,
 * FulltextSearchParams{topk, keywords} at :1043-1047) and a merge slot for its output
 * (nodeflow/runners/merge.py:18-20) but ships no backend for them; these entry points are that
 * backend.  Rows are the same row ids as the companion sr_store (the connector adds both in step).
 * Scoring is Okapi BM25 with Lucene's idf ln(1 + (N - df + 0.5) / (df + 0.5)) over LIVE rows,
 * accumulated in 2^-16 fixed point (exact, order-independent); see DESIGN.md "Hybrid retrieval".
 * ---------------------------------------------------------------------------------------------- */
typedef struct sr_lex sr_lex;

int sr_lex_create(int device, float k1, float b, sr_lex** out);
/* Append n documents: document i has the DISTINCT term ids terms[off[i] .. off[i+1]) with
 * frequencies tf[...] (>= 1) and length dl[i] (tokens); off[0] == 0.  first_row receives the row
 * id of document 0 (rows are consecutive). */
int sr_lex_add(sr_lex* x, const int64_t* off, const int32_t* terms, const int32_t* tf,
               const int32_t* dl, int64_t n, int64_t* first_row);
int sr_lex_remove(sr_lex* x, const int64_t* rows, int64_t n);
int sr_lex_stats(sr_lex* x, int64_t* n_rows, int64_t* n_live, int64_t* n_postings,
                 int64_t* vocab, double* avgdl);
/* BM25 top-k: query b is the term ids qterms[qoff[b] .. qoff[b+1]) (a repeated term counts once
 * per occurrence; unknown ids are ignored).  out_score / out_rows: B x k host buffers sorted by
 * (score desc, row asc); -inf / -1 past the matching rows.  allow (optional, n_rows bytes) as in
 * sr_store_search_masked. */
int sr_lex_search(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B, int k,
                  const uint8_t* allow, int64_t mask_key, float* out_score, int64_t* out_rows);
/* Corpus-wide statistics of a row-sharded lexical corpus, so every shard scores with the same N,
 * avgdl and document frequencies (then per-shard results merge into exactly one index's):
 * n_live / sum_dl summed over the shards (sr_lex_totals), df[i] of terms[i] summed (sr_lex_df)
 * for every term of the queries. */
typedef struct sr_lex_global {
  int64_t n_live;
  int64_t sum_dl;
  const int32_t* terms;
  const int64_t* df;
  int n_terms;
} sr_lex_global;
int sr_lex_totals(sr_lex* x, int64_t* n_live, int64_t* sum_dl);
/* sr_lex_search scored with the corpus-wide statistics of a row-sharded collection (one shard of a
 * multi-device fulltext / hybrid collection; global NULL = sr_lex_search). */
int sr_lex_search_global(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B, int k,
                         const uint8_t* allow, int64_t mask_key, const sr_lex_global* global,
                         float* out_score, int64_t* out_rows);
/* The same with the exact 2^-16 fixed-point scores too (out_fixed, B x k uint32; score =
 * out_fixed / 65536, 0 past the matches): fp32 rounds scores above 256, so a row-sharded
 * collection merges its shards' lists on these to keep one index's (score, row) order. */
int sr_lex_search_global_fixed(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B, int k,
                               const uint8_t* allow, int64_t mask_key, const sr_lex_global* global,
                               float* out_score, int64_t* out_rows, uint32_t* out_fixed);
int sr_lex_df(sr_lex* x, const int32_t* terms, int n, int64_t* out_df);
/* Device outputs (B x k on the index's device, score fp32 / row int64 + row_offset; -inf / -1 past
 * the matches), asynchronous on `stream` after the host-side term preparation; global may be NULL
 * (this index's own statistics). */
int sr_lex_search_dev(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B, int k,
                      const sr_lex_global* global, float* out_score, int64_t* out_rows,
                      int64_t row_offset, void* stream);
/* Device-resident queries (the batched hybrid pipeline: query tokens already in HBM, no host copy
 * of the queries).  Asynchronous on `stream` when the batch fits one worst-case query group
 * (B x Lq x max df keys within the 2 GiB key budget, B <= 1024); a larger batch is grouped by the
 * queries' actual candidate caps, computed on the device and read back ONCE (one blocking
 * hipStreamSynchronize on `stream`, which also waits for work queued before it).  tok: B x Lq int32 device (row stride Lq), qlen: B int32 device.
 * sr_lex_query_stats_dev writes out_stats[0] = live rows, [1] = summed document length, [2 + q Lq +
 * i] = live df of query q's i-th token (0 past qlen[q]): 2 + B Lq int64 on the device, the vector a
 * row-sharded corpus sums over its shards (one all-reduce).  sr_lex_search_tok_dev = sr_lex_search_dev
 * for those queries, scored with the summed vector gstats (device, NULL = this index's own
 * statistics); same results bit for bit. */
int sr_lex_query_stats_dev(sr_lex* x, const int32_t* tok, const int32_t* qlen, int B, int Lq,
                           int64_t* out_stats, void* stream);
int sr_lex_search_tok_dev(sr_lex* x, const int32_t* tok, const int32_t* qlen, int B, int Lq, int k,
                          const int64_t* gstats, float* out_score, int64_t* out_rows,
                          int64_t row_offset, void* stream);
/* Exact BM25 of given (query, row) pairs, sr_store_score_rows' lexical twin (k_lex.hip
 * lex_score_rows): out_score[b, j] = the score sr_lex_search gives row rows[b, j] for query b, from
 * the row's own forward postings (the index keeps foff[rows + 1], the first posting of each row).
 * The scored terms, their multiplicities, idf and avgdl are the search's (distinct query terms with
 * 0 <= t < vocabulary and live df > 0; this index's statistics, or `global`: a query term missing
 * from its table is the search's error), the sum is the same order-independent 2^-16 fixed point:
 * out_fixed (optional, B x K uint32) equals sr_lex_search_global_fixed's value for the same pair
 * bit for bit and out_score = (float)out_fixed / 65536.  A row < 0, >= n_rows or tombstoned gives
 * -inf / 0 (checked before anything is indexed by it); a live row that shares no scored term gives
 * 0.0f / 0.  Host queries as for sr_lex_search; rows: B x K host int64; blocking.  B == 0 or K == 0 is
 * a no-op; argument errors are SR_ERR_INVALID before any device work.  Triggers the pending rebuild
 * of the inverted index (df comes from it). */
int sr_lex_score_rows(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B,
                      const int64_t* rows, int K, const sr_lex_global* global, float* out_score,
                      uint32_t* out_fixed);
/* Device rows (B x K int64 carrying row_offset) and device outputs (out_fixed may be NULL), on
 * `stream`, which is synchronised once for the host-built term tables, as sr_lex_search_dev does. */
int sr_lex_score_rows_dev(sr_lex* x, const int64_t* qoff, const int32_t* qterms, int B,
                          const int64_t* rows, int K, const sr_lex_global* global,
                          int64_t row_offset, float* out_score, uint32_t* out_fixed, void* stream);
int sr_lex_save(sr_lex* x, const char* path);
int sr_lex_load(const char* path, int device, sr_lex** out);
int sr_lex_compact(sr_lex* x, int64_t* old_to_new);
void sr_lex_destroy(sr_lex* x);

/* ------------------------------------------------------------------------------------------------
 * Learned-sparse retrieval: the impact scoring mode of sr_lex (k_lex.hip; DESIGN.md "Learned-sparse
 * retrieval").  An sr_lex created by sr_lex_create_impact holds, per posting, an fp32 document
 * weight where a BM25 index holds tf (bge-m3's sparse head, SPLADE, a "sparse vector" of Qdrant /
 * Milvus), and a query is term ids WITH weights.  Scoring, exact and order-independent: for every
 * posting of a scored term t in a live eligible row, p = fl32(qw_t * dw) (one fp32 multiply),
 * fixed = max(1, rint(p * 65536)) as uint32; a row's score is the integer sum out_fixed over those
 * postings (a row carrying t in two postings sums both) and out_score = (float)out_fixed / 65536.
 * It differs from the fp64 dot product by at most n_shared (2^-16 + p 2^-24) per row.
 * Limits, all SR_ERR_INVALID on the host before any device work: document weights finite and in
 * (0, SR_IMPACT_MAX_WEIGHT]; query weights finite and >= 0; a query whose distinct term ids (known
 * to the index or not) give sum_t (16 * qw_t * 65536 + 1) >= 2^32, in double, is rejected, so no
 * row's uint32 sum of distinct terms can overflow.  Query preparation: a zero-weight term is
 * dropped, a term id repeated in one query keeps its MAXIMUM weight (bge-m3's rule), ids < 0, >=
 * the vocabulary or with no live posting are ignored.
 * sr_lex_remove / _stats (avgdl reported as 0) / _compact / _save / _load / _destroy work on both
 * modes; an impact snapshot has the magic "SRMILEX2" and the layout of "SRMILEX1" with the weight's
 * bits in tf's place (the loader checks the weight range as it checks tf) and sr_lex_load restores
 * the mode.  Every BM25 entry point (sr_lex_add, sr_lex_search*, sr_lex_score_rows*, sr_lex_df,
 * sr_lex_totals, sr_lex_query_stats_dev, sr_hybrid_search*) returns SR_ERR_STATE on an impact index,
 * and every *_weighted entry point returns SR_ERR_STATE on a BM25 index.
 * Not provided: *_dev variants, corpus-global statistics (the score needs none, so per-shard lists
 * of a row-sharded corpus merge as they are), ShardedLex / sr_store_set_* counterparts, a connector
 * ctx switch, and a fused C entry point (lexical.sparse_hybrid_search composes the existing ones).
 * ---------------------------------------------------------------------------------------------- */
#define SR_LEX_BM25 0
#define SR_LEX_IMPACT 1
#define SR_IMPACT_MAX_WEIGHT 16.0f

int sr_lex_create_impact(int device, sr_lex** out);
/* out_mode = SR_LEX_BM25 or SR_LEX_IMPACT. */
int sr_lex_scoring(sr_lex* x, int* out_mode);
/* Append n documents: document i has the DISTINCT term ids terms[off[i] .. off[i+1]) with weights
 * weights[...]; off[0] == 0; first_row as in sr_lex_add. */
int sr_lex_add_weighted(sr_lex* x, const int64_t* off, const int32_t* terms, const float* weights,
                        int64_t n, int64_t* first_row);
/* Impact top-k: query b is the term ids qterms[qoff[b] .. qoff[b+1]) with weights qweights[...].
 * Outputs, order, allow and mask_key as in sr_lex_search; out_fixed (optional, B x k uint32) the exact
 * fixed-point scores, 0 past the matches.  Host buffers, blocking. */
int sr_lex_search_weighted(sr_lex* x, const int64_t* qoff, const int32_t* qterms,
                           const float* qweights, int B, int k, const uint8_t* allow,
                           int64_t mask_key, float* out_score, int64_t* out_rows,
                           uint32_t* out_fixed);
/* Exact impact score of given (query, row) pairs, as sr_lex_score_rows: -inf / 0 for a row < 0, >=
 * n_rows or tombstoned (checked before anything is indexed by it), 0.0f / 0 for a live row sharing
 * no scored term, else sr_lex_search_weighted's value for the same pair bit for bit. */
int sr_lex_score_rows_weighted(sr_lex* x, const int64_t* qoff, const int32_t* qterms,
                               const float* qweights, int B, const int64_t* rows, int K,
                               float* out_score, uint32_t* out_fixed);

/* ------------------------------------------------------------------------------------------------
 * Multi-vector (late interaction, ColBERT) index (multivec.hip, k_multivec.hip; DESIGN.md
 * "Multi-vector retrieval"): per row of a collection the list of its token vectors (bge-m3's
 * multi-vector output; Qdrant / Vespa / Milvus "multi-vector"), row-aligned with the store like
 * sr_lex: row i of the index is row i of the collection.  One fp16 token pool [n_tokens, dim] in HBM,
 * an int64 offsets array and live flags.  Score of a query (Lq >= 1 vectors q_i) against a row (Ld
 * >= 1 vectors d_j), MaxSim:
 *   score = (1 / Lq) sum_i max_j (q_i . d_j)
 * on the fp16 values as stored, fp32 accumulation (v_mfma_f32_16x16x32_f16), the sum over i in a
 * fixed order, one division.  |score - exact| <= (dim + Lq) 2^-23 max||q_i|| max||d_j||.  A pair's
 * bits depend on the pair alone: not on B, K, its position, the other candidates, or how the row was
 * added.  out_score[b, k] is -inf when rows[b, k] is < 0, past the index, removed or holds 0 tokens,
 * and when q_len[b] == 0; a row may repeat within a query.
 * Limits, SR_ERR_INVALID before any device work: dim a multiple of 64, <= 1024; K in [1, SR_MAX_TOPK];
 * ld_q >= 1; q_len[b] in [0, min(ld_q, SR_MV_MAX_QUERY_TOKENS)] (checked by the host variant; the
 * device variant cannot read it without a synchronisation and clamps it to that range); B == 0 is a
 * no-op.
 *   sr_mv_add       n rows, row i = the tokens vecs[off[i] .. off[i+1]) x dim (fp32 host, rounded to
 *                   nearest fp16; off[0] == 0); a row may hold 0 tokens; first_row (optional) receives
 *                   the first new row id.  Blocking.
 *   sr_mv_add_dev   n rows, row i = the first len[i] tokens of vecs[i] (fp16 [n, ld_tok, dim] and len
 *                   int32 [n], device: what sr_encoder_forward_multivec_dev writes).  Reads the lengths
 *                   back to size the pool: synchronises `stream`, and has finished when it returns.
 *   sr_mv_remove    tombstones rows (in range; twice is harmless); the tokens stay in the pool.
 *   sr_mv_get       row's tokens as fp32 (the stored values) into out (room for cap tokens; at
 *                   most cap are written); n_tok receives the row's count.
 *   sr_mv_score_rows_dev  q fp16 [B, ld_q, dim], q_len int32 [B], rows int64 [B, K], out_score fp32
 *                   [B, K], all device; the query rows at and past q_len[b] are never read.
 *                   Asynchronous on `stream`.
 *   sr_mv_score_rows      the same on host buffers, q fp32 rounded to nearest fp16.  Blocking.
 *   sr_mv_create_dtype    sr_mv_create with the pool's dtype: SR_DTYPE_F16 (what sr_mv_create means) or
 *                   SR_DTYPE_FP8_E4M3; anything else is SR_ERR_INVALID before any device work.
 *   sr_mv_info      the pool's dtype and pool_bytes = n_tokens * dim * element size (2 or 1): the
 *                   stored tokens, not the capacity.  Either output may be NULL.
 * fp8 pool (SR_DTYPE_FP8_E4M3, opt-in; meant for unit-norm tokens, which is what the head emits): a
 * token element x is stored as the one byte e4m3_rne(256 * fp16(x)): OCP e4m3fn, round to nearest
 * even, saturating at +-448 (the dense store's fp8 scan format).  No per-token scale, no fp16 copy; a
 * pool row is dim bytes.  An element with |x| > 1.75 saturates (to +-1.75), on both add paths.  The
 * dequantised value of a byte c is d^ = e4m3_value(c) / 256, exact in fp32; for a unit token
 * ||d^ - d|| <= 2^-4 ||d|| + sqrt(dim) 2^-18.  sr_mv_add rounds fp32 -> fp16 as on an fp16 pool and
 * then quantises with sr_mv_add_dev's kernel (the double rounding is the definition), so both adds of
 * the same values store the same bytes; sr_mv_get returns d^.  Score contract:
 *   maxsim8(q, row) = (1 / Lq) sum_i max_j (q_i . d^_j)
 * with the caller's fp16 query, unquantised, and fp32 accumulation: the fp16 definition applied to
 * the dequantised tokens, under the same bound |score - exact| <= (dim + Lq) 2^-23 max||q_i||
 * max||d^_j|| and the same bit-identity and -inf rules.  Quantisation changes what is stored, never how
 * it is scored.  Everything else (growth, remove, stats, both score entry points, the limits) is the
 * same on both dtypes.
 *   sr_mv_dim       the index's dim (what a loaded index was saved with).
 *   sr_mv_compact   drops the tombstoned rows, as sr_store_compact / sr_lex_compact do: kept rows keep
 *                   their order, old_to_new (n_rows int64, may be NULL) receives the new row of a kept
 *                   row and -1 for a dropped one, and equals the store's map for the same removals.
 *                   Afterwards n_rows == n_live and n_tokens counts the kept rows' tokens.  In place:
 *                   the pool is not duplicated and nothing is reallocated or shrunk; the kept bytes are
 *                   moved, never re-quantised, so every score of a kept row keeps its bits.  The extra
 *                   device memory is at most stage_bytes of staging (0: the default, 64 MiB) plus two
 *                   int64 per kept row; stage_bytes below one token's bytes (dim * 2, dim for fp8) or
 *                   negative is SR_ERR_INVALID and leaves the index untouched.  Blocking.
 *   sr_mv_save      writes the whole state (tombstoned rows included) to `path` through "<path>.tmp",
 *                   fsync and rename: a failed save leaves a previous snapshot intact.  Little endian:
 *                   "SRMIMVX1", int32 dim, int32 dtype, int64 n_rows, int64 n_tokens, (n_rows + 1)
 *                   int64 offsets, n_rows live bytes, n_tokens * dim * element size pool bytes as
 *                   held in HBM.
 *   sr_mv_load      the index a snapshot describes, on `device`; it scores bit for bit like the saved
 *                   one and takes every call above.  The file is checked in full before any device
 *                   work; SR_ERR_IO for: a wrong magic, dim not a multiple of 64 in [64, 1024], an
 *                   unknown dtype, n_rows or n_tokens outside [0, 2^40], a size other than the header
 *                   implies (truncated, or a trailing byte), off[0] != 0, decreasing offsets, a row of
 *                   2^31 tokens or more, off[n_rows] != n_tokens, a live byte above 1, an e4m3 NaN code
 *                   (0x7f, 0xff) in an fp8 pool.
 * Whole-corpus search (k_mvscan.hip; DESIGN.md "Whole-corpus MaxSim search"): the index as a first
 * stage of its own, exact, one pass over the pool per group of queries.
 *   sr_mv_search_dev  q fp16 [B, ld_q, dim], q_len int32 [B], allow n_rows bytes or NULL, out_score
 *                   fp32 [B, k], out_rows int64 [B, k], all device.  For query b the k eligible rows
 *                   with the highest MaxSim, ordered by (score desc, row asc), the store's tie rule.  A
 *                   row is eligible when it is live, holds at least one token and, where allow is
 *                   given, allow[row] != 0.  Slots past the eligible rows hold -inf / -1; a query with
 *                   q_len[b] == 0 gets -inf / -1 in every slot; so does every query on an empty index.
 *                   row_offset is added to every real row.  Asynchronous on `stream` after its
 *                   host-side planning; nothing is read back.
 *   sr_mv_search    the same on host buffers: q fp32 rounded to nearest fp16, allow n_rows host bytes
 *                   or NULL, uploaded per call (no key cache), no row_offset.  Blocking.
 *   sr_mv_search_group  the queries of one workgroup of the scan at `dim` (the Q below): 3 up to dim
 *                   384, 2 up to 512, 1 above.  Needs no device.
 * Score bits: out_score for (b, row) equals what sr_mv_score_rows / _dev returns for the same pair,
 * bit for bit, on both pool dtypes: a pair's bits depend on the pair alone here too, not on B, k, allow,
 * slab_rows or the other rows.  The query rows at and past q_len[b] are never read; the device variant
 * clamps q_len as sr_mv_score_rows_dev does, the host variant checks it.  Token values are finite by
 * contract; the place of a NaN score in the list is unspecified, but nothing is indexed by it.
 * Memory: the scan works in slabs of at most slab_rows consecutive rows; 0 means as many rows as keep
 * the per-slab score scratch B * rows * 4 bytes within 64 MiB, at least 1024.  The extra device memory
 * is that scratch plus a running list of B * k 64-bit keys, kept by the index between calls: never
 * O(B * n_rows), never O(number of slabs).  The result does not depend on slab_rows, in bits.
 * Limits, SR_ERR_INVALID before any device work: a NULL handle; k outside [1, SR_MAX_TOPK]; ld_q < 1;
 * B < 0; slab_rows < 0; row_offset < 0; a null buffer (allow excepted); q_len[b] outside [0, min(ld_q,
 * SR_MV_MAX_QUERY_TOKENS)] on the host variant.  B == 0 is a no-op.
 * Not provided: a multi-device variant, shrinking the pool, per-token scales or residual codecs,
 * quantised queries, a fused rerank entry point (multivec.m3_rerank composes the existing ones); for
 * the search: an allow key cache, grouped, MMR or subset variants, approximate pruning (centroids,
 * PLAID), a connector ctx switch.
 * ---------------------------------------------------------------------------------------------- */
#define SR_MV_MAX_QUERY_TOKENS 512
typedef struct sr_mv sr_mv;

int sr_mv_create(int dim, int device, sr_mv** out);
int sr_mv_create_dtype(int dim, int device, int dtype, sr_mv** out);
int sr_mv_info(sr_mv* x, int* dtype, int64_t* pool_bytes);
int sr_mv_add(sr_mv* x, const int64_t* off, const float* vecs, int64_t n, int64_t* first_row);
int sr_mv_add_dev(sr_mv* x, const void* vecs, const int32_t* len, int64_t n, int ld_tok,
                  int64_t* first_row, void* stream);
int sr_mv_remove(sr_mv* x, const int64_t* rows, int64_t n);
int sr_mv_stats(sr_mv* x, int64_t* n_rows, int64_t* n_live, int64_t* n_tokens);
int sr_mv_get(sr_mv* x, int64_t row, float* out, int64_t cap, int64_t* n_tok);
int sr_mv_score_rows_dev(sr_mv* x, const void* q, const int32_t* q_len, int B, int ld_q,
                         const int64_t* rows, int K, float* out_score, void* stream);
int sr_mv_score_rows(sr_mv* x, const float* q, const int32_t* q_len, int B, int ld_q,
                     const int64_t* rows, int K, float* out_score);
int sr_mv_search(sr_mv* x, const float* q, const int32_t* q_len, int B, int ld_q, int k,
                 const uint8_t* allow, int64_t slab_rows, float* out_score, int64_t* out_rows);
int sr_mv_search_dev(sr_mv* x, const void* q, const int32_t* q_len, int B, int ld_q, int k,
                     const uint8_t* allow, int64_t slab_rows, int64_t row_offset,
                     float* out_score, int64_t* out_rows, void* stream);
int sr_mv_search_group(int dim, int* queries);
int sr_mv_dim(sr_mv* x, int* dim);
int sr_mv_compact(sr_mv* x, int64_t stage_bytes, int64_t* old_to_new);
int sr_mv_save(sr_mv* x, const char* path);
int sr_mv_load(const char* path, int device, sr_mv** out);
void sr_mv_destroy(sr_mv* x);

/* Reciprocal-rank fusion of two ranked row lists per query (B x ka and B x kb, -1 padded), as
 * graphiti rrf (graphiti_core/search/search_utils.py:1762-1778): score = sum 1 / (rank +
 * rank_const) in fp64, order (score desc, first appearance), rows with score < min_score
 * dropped.  Host buffers; computed on `device`. */
int sr_rrf_fuse(const int64_t* rows_a, int ka, const int64_t* rows_b, int kb, int B,
                int rank_const, double min_score, int k_out, double* out_score,
                int64_t* out_rows, int device);
/* Same on device buffers, asynchronous on `stream` of `device`. */
int sr_rrf_fuse_dev(const int64_t* rows_a, int ka, const int64_t* rows_b, int kb, int B,
                    int rank_const, double min_score, int k_out, double* out_score,
                    int64_t* out_rows, int device, void* stream);
/* Hybrid retrieval on one device: dense top-k_each (sr_store_search semantics) and BM25
 * top-k_each of the same queries, fused on the device by rrf into B x k (out_score = rrf score).
 * q: B x dim host fp32; the lexical query as in sr_lex_search; allow optional (mask_key as in
 * sr_store_search_masked). */
int sr_hybrid_search(sr_store* s, sr_lex* x, const float* q, const int64_t* qoff,
                     const int32_t* qterms, int B, int k, int k_each, int rank_const,
                     double min_score, const uint8_t* allow, int64_t mask_key,
                     double* out_score, int64_t* out_rows);

/* ------------------------------------------------------------------------------------------------
 * Score-based fusion (Weaviate relativeScoreFusion, Milvus WeightedRanker, min-max linear
 * combination; Bruch et al. 2023): the alternative to rrf that keeps the scores (k_fuse.hip).
 * Per query two scored lists: a = (score_a [ka] fp32, rows_a [ka] int64) and b likewise with kb.
 * An entry with row < 0 is absent wherever it stands; a row appears at most once per list; no
 * order is assumed; the scores of present entries are finite.  side_a [kb] (optional): the a-metric
 * score of each b row, for example the exact cosine of a BM25 hit; -inf = unknown.
 * Semantics, fp32, every operation rounded once (no FMA contraction), correctly rounded division:
 *   hi    = max of the present scores of the list itself (-inf for an empty list); side_a never
 *           enters hi or lo
 *   lo    = SR_FUSE_MINMAX: min of the present scores of the list (+inf for an empty list);
 *           SR_FUSE_FLOOR: the caller's floor_a / floor_b
 *   score = a row's a-score is list a's value when the row is in list a, else side_a of its b entry
 *           (unknown without side_a or for -inf); its b-score is list b's value or unknown
 *   norm(s) = hi > lo ? max(0, (s - lo) / (hi - lo)) : 1 for a known score, 0 for an unknown one
 *   fused = (alpha * norm_a) + (one_minus_alpha * norm_b), one_minus_alpha = 1.0f - alpha
 * Output: the first k_out distinct rows by (fused desc, row asc), the store's tie rule (not rrf's
 * "first appearance"); rows with fused < min_score are dropped; unfilled slots hold -inf / -1.
 * out_a / out_b (optional, B x k_out): the a- and b-score of each kept row as used above (side_a
 * included), -inf where unknown.
 * Limits: ka, kb in [0, 2048]; k_out in [1, 2048]; alpha in [0, 1]; rows in [0, 2^32 - 2] (checked by
 * the host variant; the device variant reads whatever it is given without indexing anything by
 * it).  B == 0 is a no-op; anything else, a null buffer or an unknown mode is SR_ERR_INVALID before
 * any device call.
 * Not provided: an sr_store_set_* counterpart (the Python ShardedLex fuses the merged lists),
 * fusion with grouped / diversified / subset search, and any claim about retrieval quality.
 * ---------------------------------------------------------------------------------------------- */
#define SR_FUSE_MINMAX 0 /* "relative": lo = the list's own minimum */
#define SR_FUSE_FLOOR 1  /* "floor": lo = floor_a / floor_b, the metric's theoretical minimum */
#define SR_FUSE_FLOOR_FULL 2 /* "floor_full": SR_FUSE_FLOOR with BOTH sides completed; accepted by
                                sr_hybrid_search_fused only (sr_score_fuse* reject it: pass
                                SR_FUSE_FLOOR and side_b to sr_score_fuse_sides*) */

/* Host buffers, blocking; computed on `device`. */
int sr_score_fuse(const float* score_a, const int64_t* rows_a, int ka, const float* score_b,
                  const int64_t* rows_b, int kb, const float* side_a, int B, int mode, float alpha,
                  float floor_a, float floor_b, float min_score, int k_out, float* out_score,
                  int64_t* out_rows, float* out_a, float* out_b, int device);
/* Same on device buffers, asynchronous on `stream` of `device`. */
int sr_score_fuse_dev(const float* score_a, const int64_t* rows_a, int ka, const float* score_b,
                      const int64_t* rows_b, int kb, const float* side_a, int B, int mode,
                      float alpha, float floor_a, float floor_b, float min_score, int k_out,
                      float* out_score, int64_t* out_rows, float* out_a, float* out_b, int device,
                      void* stream);

/* sr_score_fuse with the mirror of side_a: side_b [ka] (optional) is the b-metric score of each a
 * row, for example the exact BM25 (sr_lex_score_rows) of a dense hit; -inf = unknown.  It is used
 * only for a row that list b does not hold (its b-score is then side_b of its a entry instead of
 * unknown), never enters hi_b / lo_b, and shows in out_b.  side_b == NULL is sr_score_fuse bit for
 * bit.  Same limits and errors. */
int sr_score_fuse_sides(const float* score_a, const int64_t* rows_a, int ka, const float* score_b,
                        const int64_t* rows_b, int kb, const float* side_a, const float* side_b,
                        int B, int mode, float alpha, float floor_a, float floor_b, float min_score,
                        int k_out, float* out_score, int64_t* out_rows, float* out_a, float* out_b,
                        int device);
int sr_score_fuse_sides_dev(const float* score_a, const int64_t* rows_a, int ka,
                            const float* score_b, const int64_t* rows_b, int kb,
                            const float* side_a, const float* side_b, int B, int mode, float alpha,
                            float floor_a, float floor_b, float min_score, int k_out,
                            float* out_score, int64_t* out_rows, float* out_a, float* out_b,
                            int device, void* stream);

/* Exact cosine of given (query, row) pairs on the fp16 rows (either scan dtype): out_sim[b, j] =
 * q_b . x_rows[b, j] with the query normalised as a search normalises it and fp32 accumulation;
 * -inf for a row < 0, a row >= n_rows or a tombstoned row (checked before anything is indexed).
 * q: B x dim host fp32; rows: B x K host int64; blocking.  B or K == 0 is a no-op. */
int sr_store_score_rows(sr_store* s, const float* q, int B, const int64_t* rows, int K,
                        float* out_sim);
/* Device buffers (q_dtype as in sr_store_search_dev; rows carry row_offset); asynchronous on
 * `stream`. */
int sr_store_score_rows_dev(sr_store* s, const void* q, int q_dtype, int B, const int64_t* rows,
                            int K, int64_t row_offset, float* out_sim, void* stream);

/* sr_hybrid_search with score fusion as its last step: list a = the dense top-k_each with its
 * cosines, list b = the BM25 top-k_each with its scores, fused by sr_score_fuse semantics into
 * B x k (k in [1, 2 k_each], k_each in [1, SR_MAX_TOPK]); out_score fp32 fused scores, out_dense /
 * out_lex (optional) the components.  SR_FUSE_MINMAX passes no side scores.  SR_FUSE_FLOOR uses
 * floor_a = -1 (cosine), floor_b = 0 (BM25) and completes the dense side: side_a = the exact
 * cosines (sr_store_score_rows semantics) of the BM25 list's rows.  In SR_FUSE_FLOOR the BM25 side
 * is NOT completed for dense-only rows: a row that shares no term with the query has BM25 exactly
 * 0, which is the floor, so only a row that matches but was truncated from the BM25 top-k_each is
 * under-scored, by less than that list's minimum.  SR_FUSE_FLOOR_FULL completes that side too: it is
 * SR_FUSE_FLOOR plus side_b = the exact BM25 (sr_lex_score_rows semantics, this index's statistics)
 * of the dense list's rows, with a score of exactly 0 passed as -inf (unknown).  A non-matching row
 * then scores as in SR_FUSE_FLOOR (unknown -> 0) and not by the fusion's "known score on an empty
 * list -> 1" rule, which would add 1 - alpha to every row when no row matches the query; only
 * matching rows truncated from the BM25 list change, and a row's fused score no longer depends on
 * where k_each cut the other list. */
int sr_hybrid_search_fused(sr_store* s, sr_lex* x, const float* q, const int64_t* qoff,
                           const int32_t* qterms, int B, int k, int k_each, int mode, float alpha,
                           float min_score, const uint8_t* allow, int64_t mask_key,
                           float* out_score, int64_t* out_rows, float* out_dense, float* out_lex);

/* ------------------------------------------------------------------------------------------------
 * Transformer encoder (BERT / XLM-R family: bge-small/base-en, bge-m3, bge-reranker-*)
 * Weights are set by Hugging Face tensor name without the model prefix, e.g.
 * "embeddings.word_embeddings.weight", "encoder.layer.3.attention.self.query.weight",
 * "classifier.dense.weight", "classifier.out_proj.bias".  Matrices are stored fp16 in HBM,
 * biases / LayerNorm parameters fp32.  Activations are fp16 GEMM operands with an fp32
 * residual stream; accumulation is fp32 everywhere.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sr_encoder_config {
  int vocab_size;
  int hidden;           /* d                                         */
  int layers;           /* L                                         */
  int heads;            /* d / heads must be 32 or 64               */
  int intermediate;     /* FFN width                                 */
  int max_position;
  int type_vocab;       /* token-type rows (1 for XLM-R, 2 for BERT) */
  float ln_eps;         /* 1e-12 BERT, 1e-5 XLM-R                    */
  int position_offset;  /* 0: BERT (pos = index); >0: XLM-R padding_idx (pos = cumsum(mask)+pad) */
  int classifier;       /* 0: none; 1: RoBERTa classification head (dense+tanh+out_proj)       */
  int num_labels;       /* classifier outputs (1 for bge-reranker)                             */
  int max_tokens;       /* workspace size in tokens per launch chunk (0 = default 262144)      */
  int residual_fp16;    /* 0: fp32 residual stream (embeddings, <= 1e-3 rel error);
                           1: fp16 residual stream (cross-encoders: ~2.5x less LayerNorm and
                              epilogue traffic, ranking-level fidelity)                         */
} sr_encoder_config;

int sr_encoder_create(const sr_encoder_config* cfg, int device, sr_encoder** out);
int sr_encoder_set_weight(sr_encoder* e, const char* name, const float* data, int64_t numel);
/* Returns SR_OK when every weight has been set, SR_ERR_STATE (message lists a missing one) else. */
int sr_encoder_ready(sr_encoder* e);
/* Sentence embeddings: ids/mask/type_ids are B x S int32 host arrays (type_ids may be NULL);
 * out: B x hidden fp32, L2-normalised (EmbeddingService.embed_documents result rows). Blocking. */
int sr_encoder_forward(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                       const int32_t* type_ids, int B, int S, int pool, float* out);
/* Device variant; out dtype SR_DTYPE_F32 (B x hidden) or SR_DTYPE_F16 (B x ld_out, row-major,
 * ld_out >= hidden, zero-padded to ld_out so it can be fed to sr_store_search_dev). */
int sr_encoder_forward_dev(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                           const int32_t* type_ids, int B, int S, int pool, void* out,
                           int out_dtype, int ld_out, void* stream);
/* The sparse head of a multi-function embedder (bge-m3's sparse_linear; k_encoder_misc.hip,
 * DESIGN.md "Learned-sparse retrieval").  sr_encoder_set_weight accepts "sparse_linear.weight"
 * (hidden values) and "sparse_linear.bias" (1 value), kept fp32.  They are optional:
 * sr_encoder_ready and every other call behave the same with or without them, and the calls
 * below return SR_ERR_STATE until both are set.
 *   token weight   tw[b, s] = max(0, sum_i h[b, s, i] w[i] + bias) where mask[b, s] != 0, else 0,
 *                  h the final state of the token (fp32 accumulation);
 *   term collapse  a position qualifies when mask != 0, tw > 0 and ids[b, s] is none of special_ids;
 *                  each distinct qualifying id is emitted once, with the MAXIMUM tw over its
 *                  qualifying positions, in ascending order of its first qualifying position
 *                  (bge-m3's _process_token_weights): out_terms[b, 0 .. out_count[b]) and
 *                  out_weights likewise; the slots past the count hold -1 / 0.  Exact.
 * sr_sparse_terms_dev is the collapse alone, on any token weights (no encoder needed): ids / mask /
 * tok_weight B x S device, special_ids host with n_special in [0, 16], outputs B x S / B x S / B
 * device; S in [1, 8192]; asynchronous on `stream` of `device`.  B == 0 is a no-op; a shape outside
 * these limits or a null buffer is SR_ERR_INVALID before any device call.
 * sr_encoder_forward_sparse_dev is ONE forward pass giving the dense embedding (out_dense /
 * out_dtype / ld_out as in sr_encoder_forward_dev) and the sparse outputs (device; out_tok_weight B x
 * S may be NULL).  The last layer runs for every token whatever the pooling, so with SR_POOL_MEAN the
 * dense output equals sr_encoder_forward_dev's bit for bit, and with SR_POOL_CLS it comes from a full
 * last layer where sr_encoder_forward_dev computes the CLS rows only (the same values within
 * rounding).  sr_encoder_forward_sparse takes and fills host buffers (out_dense B x hidden fp32) and
 * blocks.
 * Not provided: an fp16 / packed output of the terms, a sparse head on a cross-encoder
 * (classifier models), and sequences longer than 8192 tokens. */
int sr_sparse_terms_dev(const int32_t* ids, const int32_t* mask, const float* tok_weight, int B, int S,
                        const int32_t* special_ids, int n_special, int32_t* out_terms,
                        float* out_weights, int32_t* out_count, int device, void* stream);
int sr_encoder_forward_sparse_dev(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                                  const int32_t* type_ids, int B, int S, int pool, void* out_dense,
                                  int out_dtype, int ld_out, const int32_t* special_ids, int n_special,
                                  float* out_tok_weight, int32_t* out_terms, float* out_weights,
                                  int32_t* out_count, void* stream);
int sr_encoder_forward_sparse(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                              const int32_t* type_ids, int B, int S, int pool, float* out_dense,
                              const int32_t* special_ids, int n_special, float* out_tok_weight,
                              int32_t* out_terms, float* out_weights, int32_t* out_count);
/* The multi-vector (ColBERT) head of a multi-function embedder (bge-m3's colbert_linear;
 * k_encoder_misc.hip colbert_pack, DESIGN.md "Multi-vector retrieval").  sr_encoder_set_weight accepts
 * "colbert_linear.weight" (dc * hidden values, row-major [dc, hidden]; dc is inferred from the count
 * and must be a multiple of 128, <= 1024; kept fp16) and "colbert_linear.bias" (dc values, fp32).
 * Optional like the sparse head: sr_encoder_ready and every other call behave the same with or
 * without them, and the calls below return SR_ERR_STATE (naming the missing one) until both are set.
 * The weight defines dc (a weight of another dc unsets the bias); the bias is set after it
 * (SR_ERR_STATE before) and holds dc values; any other count is SR_ERR_INVALID.
 * sr_encoder_colbert_dim gives dc, 0 without the weight.
 *   v[b, s] = W h[b, s] + bias (fp16 operands, fp32 accumulation, rounded to fp16),
 *   u[b, s] = v / max(||v||, 1e-12) (fp32 norm, rounded to fp16);
 *   the multi-vector of sequence b is u[b, s] over the positions s >= 1 with mask[b, s] != 0, in
 *   position order: position 0 (CLS / <s>) is always dropped, the closing separator stays.
 * sr_encoder_forward_multivec_dev is ONE forward pass giving the dense embedding (out_dense /
 * out_dtype / ld_out as in sr_encoder_forward_dev; the last layer runs in full, so SR_POOL_MEAN equals
 * sr_encoder_forward_dev bit for bit and SR_POOL_CLS equals sr_encoder_forward_sparse_dev's), out_vecs
 * (fp16, B x S x dc device: rows [0, out_len[b]) of sequence b the compacted unit vectors, the rows
 * behind them zero) and out_len (B int32 device): the layout sr_mv_add_dev takes.  The sparse outputs of
 * sr_encoder_forward_sparse_dev are one optional group: out_terms, out_weights and out_count all NULL
 * (then special_ids and n_special are ignored and out_tok_weight must be NULL too), or all set
 * (out_tok_weight stays optional); a half-given group is SR_ERR_INVALID.  S in [1, 8192].
 * sr_encoder_forward_multivec takes and fills host buffers (out_dense B x hidden fp32, out_vecs B x S
 * x dc fp32 holding the fp16 values) and blocks. */
int sr_encoder_colbert_dim(sr_encoder* e, int* out);
int sr_encoder_forward_multivec_dev(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                                    const int32_t* type_ids, int B, int S, int pool, void* out_dense,
                                    int out_dtype, int ld_out, void* out_vecs, int32_t* out_len,
                                    const int32_t* special_ids, int n_special, float* out_tok_weight,
                                    int32_t* out_terms, float* out_weights, int32_t* out_count,
                                    void* stream);
int sr_encoder_forward_multivec(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                                const int32_t* type_ids, int B, int S, int pool, float* out_dense,
                                float* out_vecs, int32_t* out_len, const int32_t* special_ids,
                                int n_special, float* out_tok_weight, int32_t* out_terms,
                                float* out_weights, int32_t* out_count);
/* Cross-encoder relevance: P (query, passage) pairs already packed as token ids (P x S);
 * out_logits: P x num_labels fp32 raw logits (bge-reranker scores = logits, sigmoid optional). */
int sr_cross_score(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                   const int32_t* type_ids, int P, int S, float* out_logits);
int sr_cross_score_dev(sr_encoder* e, const int32_t* ids, const int32_t* mask,
                       const int32_t* type_ids, int P, int S, float* out_logits, void* stream);
/* fp8 precision modes (BASELINE config 5 "fp8 MFMA GEMM path"; LN-folded fp16-residual encoders,
 * e.g. the cross-encoders).  1: FFN1 stores OCP e4m3 activations and FFN2 runs the block-scaled
 * fp8 MFMA against an e4m3 copy of its weight (per-row power-of-two scales); 2: also FFN1 and the
 * QKV GEMMs of layers >= 1 on e4m3 copies of the residual sums (written by the residual
 * epilogues) and of the folded weights; 3: FFN1 and FFN2 as in mode 2, the QKV projection and
 * attention stay fp16 (fused).  0 (default): fp16.  Opt-in: logits move by the fp8 rounding
 * (tests/test_gpu_encoder.py; ranking fidelity per mode: tests/test_gpu_rerank_fidelity.py). */
int sr_encoder_set_fp8(sr_encoder* e, int mode);
void sr_encoder_destroy(sr_encoder* e);

/* ------------------------------------------------------------------------------------------------
 * Device pipeline helpers for the batched search path (embed -> top-K -> pairs -> rerank)
 * ---------------------------------------------------------------------------------------------- */
/* Pack cross-encoder inputs for every (query b, candidate j):
 *   style 0 (RoBERTa/XLM-R):  <s> q </s> </s> p </s>      style 1 (BERT): [CLS] q [SEP] p [SEP]
 * q_tok: B x lq_max content tokens (no specials), q_len: B;  p_tok: N x lp_max, p_len: N;
 * cand_rows: B x K (int64; rows < 0 give an all-padding pair).  The passage is truncated first,
 * then the query.  out_ids / out_mask / out_type: (B*K) x S int32 (out_type may be NULL). */
int sr_build_pairs_dev(const int32_t* q_tok, const int32_t* q_len, int lq_max,
                       const int32_t* p_tok, const int32_t* p_len, int lp_max,
                       const int64_t* cand_rows, int B, int K, int S, int style,
                       int bos_id, int eos_id, int pad_id,
                       int32_t* out_ids, int32_t* out_mask, int32_t* out_type,
                       int device, void* stream);
/* Per query: order the K candidates by (logit desc, candidate index asc) and keep k_out.
 * logits: B x K fp32; out_index: B x k_out int32 positions into the candidate list. */
int sr_rerank_select_dev(const float* logits, int B, int K, int k_out, int32_t* out_index,
                         int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Profiling: per-kernel HIP-event timing of every launch on the library's streams.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sr_kernel_stat {
  char name[64];        /* kernel family, e.g. "gemm_f16_gelu", "cosine_scan"              */
  int64_t launches;
  double total_ms;      /* sum of HIP-event durations                                        */
  double flops;         /* algorithmic FLOPs over all launches                               */
  double bytes;         /* algorithmic HBM bytes over all launches                           */
} sr_kernel_stat;

int sr_profile_enable(int on);              /* clears the table when turned on                  */
/* Fills up to max entries (synchronises the recorded events); *n receives the number written. */
int sr_profile_read(sr_kernel_stat* out, int max, int* n);

/* The kernel-level diagnostics (sr_diag_*: single-kernel parity entry points, timing-only
 * variants, the HBM copy yardstick) are not part of this library: they live in the separate
 * libsrmi_diag.so, declared in super_rag_mi355x_diag.h. */

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif

#endif /* SUPER_RAG_MI355X_H */
