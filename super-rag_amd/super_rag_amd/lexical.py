"""Lexical (BM25) retrieval and dense + lexical hybrid fusion: host side of sr_lex_* /
sr_rrf_fuse / sr_hybrid_search (include/super_rag_mi355x.h).

The reference declares the pieces but ships no backend: a ``fulltext_search`` node type and
``FulltextSearchParams{topk, keywords}`` (schema/view_models.py:276-283, :1043-1047), a
``fulltext_search_docs`` merge slot (nodeflow/runners/merge.py:18-20) and a
``enable_vector_and_fulltext`` collection flag.  Here:

  * ``analyze(text)``: lower-case, Unicode ``\\w+`` tokens (no stemming, no stop words);
  * ``Vocab``: term -> int32 id per collection (persisted with the collection snapshot);
  * ``NativeLexIndex``: the device BM25 index (k_lex.hip): Okapi BM25, k1 = 1.2, b = 0.75, Lucene's
    idf ln(1 + (N - df + 0.5) / (df + 0.5)) over live rows, scores in 2^-16 fixed point;
  * ``rrf_fuse`` / ``hybrid_search``: reciprocal-rank fusion as graphiti's ``rrf``
    (graphiti_core/search/search_utils.py:1762-1778), on the device;
  * ``score_fuse`` / ``hybrid_search(fusion="relative" | "floor")``: score-based fusion (weighted
    min-max or floor-normalised cosine + BM25, k_fuse.hip), opt-in next to rrf;
  * ``NativeLexIndex.score_rows`` / ``ShardedLex.score_rows``: the exact BM25 of given (query, row)
    pairs (lex_score_rows), and ``fusion="floor_full"``: floor fusion with the BM25 side completed
    by it for the dense list's rows, as the dense side already is.
  * ``NativeImpactIndex`` / ``sparse_hybrid_search``: learned-sparse retrieval, the same index in
    its impact scoring mode (documents and queries are term ids with fp32 weights, e.g. bge-m3's
    sparse vectors from ``Encoder.embed_sparse``; the score is their fixed-point dot product) and
    its fusion with the dense side by the rules above.
There is no CPU fallback: every entry point needs the HIP library and a GPU.
"""
from __future__ import annotations

import ctypes
import re
from collections import Counter
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N

_TOKEN = re.compile(r"\w+", re.UNICODE)
K1 = 1.2
B = 0.75


def analyze(text: Optional[str]) -> List[str]:
    """Text -> lexical tokens (lower-cased Unicode word characters)."""
    return _TOKEN.findall(text.lower()) if text else []


class Vocab:
    """Term string <-> dense int32 id."""

    def __init__(self, terms: Iterable[str] = ()):
        self.terms: List[str] = []
        self.ids: Dict[str, int] = {}
        for t in terms:
            self.ids.setdefault(t, len(self.terms))
            if len(self.ids) > len(self.terms):
                self.terms.append(t)

    def __len__(self) -> int:
        return len(self.terms)

    def doc_ids(self, tokens: Sequence[str]) -> List[int]:
        """Ids of a document's tokens, adding new terms."""
        out = []
        for t in tokens:
            i = self.ids.get(t)
            if i is None:
                i = self.ids[t] = len(self.terms)
                self.terms.append(t)
            out.append(i)
        return out

    def query_ids(self, tokens: Sequence[str]) -> List[int]:
        """Ids of a query's tokens; unknown terms are dropped (they match no row)."""
        return [self.ids[t] for t in tokens if t in self.ids]


def doc_arrays(docs: Sequence[Sequence[int]]):
    """Token-id lists -> (off int64[n+1], terms int32, tf int32, dl int32): each document's distinct
    terms in first-occurrence order with their counts; dl = token count."""
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    terms: List[int] = []
    tfs: List[int] = []
    dl = np.empty(len(docs), dtype=np.int32)
    for i, d in enumerate(docs):
        c = Counter(d)
        terms.extend(c.keys())
        tfs.extend(c.values())
        off[i + 1] = len(terms)
        dl[i] = len(d)
    return off, np.asarray(terms, dtype=np.int32), np.asarray(tfs, dtype=np.int32), dl


def query_arrays(queries: Sequence[Sequence[int]]):
    qoff = np.zeros(len(queries) + 1, dtype=np.int64)
    flat: List[int] = []
    for i, q in enumerate(queries):
        flat.extend(int(t) for t in q)
        qoff[i + 1] = len(flat)
    qterms = np.asarray(flat if flat else [0], dtype=np.int32)
    return qoff, qterms


class LexGlobalC(ctypes.Structure):
    """sr_lex_global: corpus-wide statistics of a row-sharded lexical corpus."""
    _fields_ = [("n_live", ctypes.c_int64), ("sum_dl", ctypes.c_int64), ("terms", ctypes.c_void_p),
                ("df", ctypes.c_void_p), ("n_terms", ctypes.c_int)]


def _global_c(global_stats):
    """(n_live, sum_dl, terms, df) -> (sr_lex_global, the arrays it points into), or (None, None)."""
    if global_stats is None:
        return None, None
    n_live, sum_dl, gt, gdf = global_stats
    gt = np.ascontiguousarray(gt, dtype=np.int32)
    gdf = np.ascontiguousarray(gdf, dtype=np.int64)
    return LexGlobalC(int(n_live), int(sum_dl), gt.ctypes.data, gdf.ctypes.data, int(gt.size)), (gt, gdf)


def _mask(allow, n_rows: int):
    a = np.ascontiguousarray(np.asarray(allow, dtype=np.uint8))
    if a.shape != (n_rows,):
        raise ValueError(f"allow mask must have {n_rows} entries, got {a.shape}")
    return a if n_rows else np.zeros(1, dtype=np.uint8)


class NativeLexIndex:
    """BM25 index over the rows of a store, resident in HBM of one device."""

    def __init__(self, device: int = 0, k1: float = K1, b: float = B, _handle=None):
        self._h = None
        if _handle is None:
            N.require_gpu()
            h = ctypes.c_void_p()
            N.call("sr_lex_create", int(device), float(k1), float(b), ctypes.byref(h))
            _handle = h
        self._h = _handle
        self.device = int(device)

    @classmethod
    def load(cls, path: str, device: int = 0) -> "NativeLexIndex":
        N.require_gpu()
        h = ctypes.c_void_p()
        N.call("sr_lex_load", path.encode(), int(device), ctypes.byref(h))
        if lex_scoring(h) != N.SR_LEX_BM25:
            N.load().sr_lex_destroy(h)
            raise ValueError(f"{path} is an impact (learned-sparse) snapshot: load it with "
                             "NativeImpactIndex.load")
        return cls(device, _handle=h)

    def close(self) -> None:
        if self._h:
            N.load().sr_lex_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, docs: Sequence[Sequence[int]]) -> int:
        """Append documents (token-id lists); returns the first row id."""
        if not len(docs):
            return self.stats()["rows"]
        return self.add_arrays(*doc_arrays(docs))

    def add_arrays(self, off, terms, tf, dl) -> int:
        """Bulk append of pre-tokenised documents in the C-ABI layout (doc_arrays output:
        off int64[n+1], distinct terms int32 with counts tf int32, lengths dl int32)."""
        off = np.ascontiguousarray(off, dtype=np.int64)
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        tf = np.ascontiguousarray(tf, dtype=np.int32)
        dl = np.ascontiguousarray(dl, dtype=np.int32)
        n = len(off) - 1
        if terms.size == 0:
            terms, tf = np.zeros(1, np.int32), np.ones(1, np.int32)
        first = ctypes.c_int64(0)
        N.call("sr_lex_add", self._h, N.ptr(off), N.ptr(terms), N.ptr(tf), N.ptr(dl), n,
               ctypes.byref(first))
        return int(first.value)

    def remove(self, rows) -> None:
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        N.call("sr_lex_remove", self._h, N.ptr(r), r.shape[0])

    def compact(self) -> np.ndarray:
        n = self.stats()["rows"]
        m = np.empty(max(n, 1), dtype=np.int64)
        N.call("sr_lex_compact", self._h, N.ptr(m))
        return m[:n]

    def save(self, path: str) -> None:
        N.call("sr_lex_save", self._h, path.encode())

    def stats(self) -> dict:
        v = [ctypes.c_int64(0) for _ in range(4)]
        a = ctypes.c_double(0.0)
        N.call("sr_lex_stats", self._h, *[ctypes.byref(x) for x in v], ctypes.byref(a))
        return {"rows": v[0].value, "live": v[1].value, "postings": v[2].value,
                "vocab": v[3].value, "avgdl": a.value}

    def search(self, queries: Sequence[Sequence[int]], k: int, allow=None, mask_key: int = 0,
               global_stats=None, fixed: bool = False):
        """BM25 top-k per query (token-id lists) -> (score [B,k] fp32 desc, rows [B,k] int64).
        global_stats: (n_live, sum_dl, terms, df) of a whole row-sharded corpus (ShardedLex).
        fixed: also return the exact 2^-16 fixed-point scores [B,k] uint32 (sr_lex_search_global_
        fixed; the fp32 scores round above 256), the key a sharded merge orders by."""
        Bq = len(queries)
        scores = np.empty((Bq, k), dtype=np.float32)
        rows = np.empty((Bq, k), dtype=np.int64)
        fx = np.zeros((Bq, k), dtype=np.uint32) if fixed else None
        if Bq == 0:
            return (scores, rows, fx) if fixed else (scores, rows)
        qoff, qterms = query_arrays(queries)
        a = None if allow is None else _mask(allow, self.stats()["rows"])
        g = None
        if global_stats is not None:
            n_live, sum_dl, gt, gdf = global_stats
            gt = np.ascontiguousarray(gt, dtype=np.int32)
            gdf = np.ascontiguousarray(gdf, dtype=np.int64)
            g = LexGlobalC(int(n_live), int(sum_dl), gt.ctypes.data, gdf.ctypes.data, int(gt.size))
        if fixed:
            N.call("sr_lex_search_global_fixed", self._h, N.ptr(qoff), N.ptr(qterms), Bq, int(k),
                   None if a is None else N.ptr(a), int(mask_key),
                   None if g is None else ctypes.byref(g), N.ptr(scores), N.ptr(rows), N.ptr(fx))
            return scores, rows, fx
        if g is None:
            N.call("sr_lex_search", self._h, N.ptr(qoff), N.ptr(qterms), Bq, int(k),
                   None if a is None else N.ptr(a), int(mask_key), N.ptr(scores), N.ptr(rows))
        else:
            N.call("sr_lex_search_global", self._h, N.ptr(qoff), N.ptr(qterms), Bq, int(k),
                   None if a is None else N.ptr(a), int(mask_key), ctypes.byref(g), N.ptr(scores),
                   N.ptr(rows))
        return scores, rows

    def score_rows(self, queries: Sequence[Sequence[int]], rows, global_stats=None,
                   fixed: bool = False):
        """Exact BM25 of given (query, row) pairs (sr_lex_score_rows): queries as for search, rows
        [B, K] int64 -> score [B, K] fp32, the score search gives that row for that query: -inf for a
        row < 0, past the index or tombstoned, 0 for a live row that shares no scored term.
        global_stats as for search; fixed: also the exact 2^-16 fixed-point scores [B, K] uint32."""
        Bq = len(queries)
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        if r.ndim != 2 or r.shape[0] != Bq:
            raise ValueError(f"rows must be [{Bq}, K], got {r.shape}")
        score = np.empty(r.shape, dtype=np.float32)
        fx = np.zeros(r.shape, dtype=np.uint32) if fixed else None
        if r.size:
            qoff, qterms = query_arrays(queries)
            g, _keep = _global_c(global_stats)
            N.call("sr_lex_score_rows", self._h, N.ptr(qoff), N.ptr(qterms), Bq, N.ptr(r), r.shape[1],
                   None if g is None else ctypes.byref(g), N.ptr(score), N.ptr(fx) if fixed else None)
        return (score, fx) if fixed else score

    def score_rows_dev(self, qoff, qterms, rows, global_stats=None, row_offset: int = 0,
                       fixed: bool = False, stream=None):
        """score_rows on device rows: qoff / qterms host arrays (query_arrays), rows [B, K] int64
        torch tensor on this device carrying ``row_offset`` -> score [B, K] fp32 device tensor (and
        the fixed-point scores as int32 bit patterns of the uint32 values with ``fixed``);
        sr_lex_score_rows_dev, ``stream`` synchronised once."""
        import torch
        qoff = np.ascontiguousarray(qoff, dtype=np.int64)
        qterms = np.ascontiguousarray(qterms, dtype=np.int32)
        Bq = len(qoff) - 1
        rows = rows.contiguous()
        if not (rows.is_cuda and rows.dtype == torch.int64 and rows.dim() == 2 and rows.shape[0] == Bq):
            raise ValueError(f"rows must be a CUDA int64 tensor [{Bq}, K]")
        score = torch.empty(rows.shape, dtype=torch.float32, device=rows.device)
        fx = torch.zeros(rows.shape, dtype=torch.int32, device=rows.device) if fixed else None
        if rows.numel():
            g, _keep = _global_c(global_stats)
            N.call("sr_lex_score_rows_dev", self._h, N.ptr(qoff), N.ptr(qterms), Bq, N.ptr(rows),
                   rows.shape[1], None if g is None else ctypes.byref(g), int(row_offset),
                   N.ptr(score), N.ptr(fx) if fixed else None, N.stream_handle(stream))
        return (score, fx) if fixed else score

    def totals(self):
        """(live rows, summed document length) of this index."""
        n, d = ctypes.c_int64(0), ctypes.c_int64(0)
        N.call("sr_lex_totals", self._h, ctypes.byref(n), ctypes.byref(d))
        return int(n.value), int(d.value)

    def df(self, terms) -> np.ndarray:
        """Live document frequency of each term id (0 for unknown terms)."""
        t = np.ascontiguousarray(np.asarray(terms, dtype=np.int32))
        out = np.zeros(t.shape[0], dtype=np.int64)
        if t.size:
            N.call("sr_lex_df", self._h, N.ptr(t), t.shape[0], N.ptr(out))
        return out

    def search_dev(self, qoff, qterms, k: int, global_stats=None, row_offset: int = 0,
                   out_score=None, out_rows=None, stream=None):
        """Device outputs: (score [B,k] fp32, rows [B,k] int64 + row_offset) torch tensors.
        qoff / qterms: host arrays (query_arrays); global_stats: (n_live, sum_dl, terms, df) of the
        whole row-sharded corpus, or None for this index's own statistics."""
        import torch
        qoff = np.ascontiguousarray(qoff, dtype=np.int64)
        qterms = np.ascontiguousarray(qterms, dtype=np.int32)
        Bq = len(qoff) - 1
        dev = torch.device("cuda", self.device)
        if out_score is None:
            out_score = torch.empty((Bq, k), dtype=torch.float32, device=dev)
        if out_rows is None:
            out_rows = torch.empty((Bq, k), dtype=torch.int64, device=dev)
        g = None
        if global_stats is not None:
            n_live, sum_dl, gt, gdf = global_stats
            gt = np.ascontiguousarray(gt, dtype=np.int32)
            gdf = np.ascontiguousarray(gdf, dtype=np.int64)
            g = LexGlobalC(int(n_live), int(sum_dl), gt.ctypes.data, gdf.ctypes.data, int(gt.size))
        N.call("sr_lex_search_dev", self._h, N.ptr(qoff), N.ptr(qterms), Bq, int(k),
               None if g is None else ctypes.byref(g), N.ptr(out_score), N.ptr(out_rows),
               int(row_offset), N.stream_handle(stream))
        return out_score, out_rows

    def query_stats_dev(self, tok, qlen, stream=None):
        """Device-resident queries (torch int32 tok [B, Lq], qlen [B] on this device) -> int64 device
        vector [live rows, summed length, df of every (query, position)]: the statistics a
        row-sharded corpus all-reduces before search_tok_dev (no host synchronisation)."""
        import torch
        tok, qlen = _dev_i32(tok), _dev_i32(qlen)
        B, Lq = tok.shape
        out = torch.empty(2 + B * Lq, dtype=torch.int64, device=tok.device)
        N.call("sr_lex_query_stats_dev", self._h, N.ptr(tok), N.ptr(qlen), B, Lq, N.ptr(out),
               N.stream_handle(stream))
        return out

    def search_tok_dev(self, tok, qlen, k: int, gstats=None, row_offset: int = 0, stream=None):
        """BM25 top-k of device-resident queries (query i = tok[i, :qlen[i]], term ids) -> device
        (score [B, k] fp32, rows [B, k] int64 + row_offset); gstats: the all-reduced
        query_stats_dev vector of a row-sharded corpus, or None for this index's own statistics.
        Identical results to search_dev on the same queries, without a host copy of the queries;
        asynchronous unless the batch exceeds one worst-case query group (B x Lq x max df keys
        over the 2 GiB budget, or B > 1024): then the device-computed per-query caps are read back
        once (one synchronisation of `stream`) to size the groups."""
        import torch
        tok, qlen = _dev_i32(tok), _dev_i32(qlen)
        B, Lq = tok.shape
        score = torch.empty((B, k), dtype=torch.float32, device=tok.device)
        rows = torch.empty((B, k), dtype=torch.int64, device=tok.device)
        if gstats is not None:
            gstats = gstats.contiguous()
            assert gstats.dtype == torch.int64 and gstats.numel() == 2 + B * Lq and gstats.is_cuda
        N.call("sr_lex_search_tok_dev", self._h, N.ptr(tok), N.ptr(qlen), B, Lq, int(k),
               None if gstats is None else N.ptr(gstats), N.ptr(score), N.ptr(rows),
               int(row_offset), N.stream_handle(stream))
        return score, rows

    def hybrid(self, store, queries, query_terms, k: int, k_each: Optional[int] = None,
               rank_const: int = 1, min_score: float = float("-inf"), allow=None, mask_key: int = 0,
               fusion: str = "rrf", alpha: float = 0.5):
        """hybrid_search over (store, this index)."""
        return hybrid_search(store, self, queries, query_terms, k, k_each, rank_const, min_score,
                             allow, mask_key, fusion=fusion, alpha=alpha)


class ShardedLex:
    """BM25 index of a row-sharded collection (store.ShardedStore, ctx "devices"): one lexical shard
    per store shard, on the same device and holding the same rows (the store's routing tables), so
    a fulltext / hybrid collection can span GPUs.  Every shard scores with the corpus-wide N,
    summed length and df of the query terms (sr_lex_search_global; the totals and df are summed on
    the host, as the connector's queries are host arrays), each shard's top-k is mapped to global
    rows and the lists merge on (exact 2^-16 fixed-point score desc, global row asc) -- one
    index's order, so results equal a single-device collection's for every score (the shards'
    fp32 scores round above 256; sr_lex_search_global_fixed returns the exact ones).  Global rows are
    the store's: ``add`` must follow the store's add of the same rows (the connector's order)."""

    MAGIC = "SRMILEXSHARDS1"

    def __init__(self, store, factory=None, _shards=None, _tables=None):
        self.store = store
        self.devices = list(store.devices)
        factory = factory or (lambda dev: NativeLexIndex(dev))
        self.shards = _shards if _shards is not None else [factory(d) for d in self.devices]
        self.tables = _tables if _tables is not None else [np.zeros(0, np.int64) for _ in self.devices]

    def _n(self) -> int:
        return sum(len(t) for t in self.tables)

    def add(self, docs) -> int:
        """Documents of global rows [first, first + n) (first = rows so far), each to the shard
        the store put its row on."""
        first = self._n()
        n = len(docs)
        g = np.arange(first, first + n, dtype=np.int64)
        if n and (g[-1] >= len(self.store.shard_of)):
            raise RuntimeError("lexical rows ahead of the store")
        for s, sh in enumerate(self.shards):
            sel = np.nonzero(self.store.shard_of[g] == s)[0] if n else np.zeros(0, np.int64)
            if not sel.size:
                continue
            loc = self.store.local_of[g[sel]]
            got = sh.add([docs[i] for i in sel.tolist()])
            if int(got) != int(loc[0]) or not np.array_equal(loc, np.arange(loc[0], loc[0] + len(loc))):
                raise RuntimeError("lexical shard rows out of step with the store shard")
            self.tables[s] = np.concatenate([self.tables[s], g[sel]])
        return first

    def _route(self, rows):
        r = np.asarray(rows, dtype=np.int64)
        owner = np.full(self._n(), -1, np.int64)
        local = np.full(self._n(), -1, np.int64)
        for s, t in enumerate(self.tables):
            owner[t] = s
            local[t] = np.arange(len(t))
        return r, owner, local

    def remove(self, rows) -> None:
        r, owner, local = self._route(rows)
        for s, sh in enumerate(self.shards):
            sel = r[owner[r] == s]
            if sel.size:
                sh.remove(local[sel])

    def compact(self) -> np.ndarray:
        n = self._n()
        alive = np.zeros(n, bool)
        for s, sh in enumerate(self.shards):
            m = np.asarray(sh.compact())
            keep = m >= 0
            alive[self.tables[s][keep]] = True
            self.tables[s] = self.tables[s][keep]
        remap = np.full(n, -1, np.int64)
        remap[alive] = np.arange(int(alive.sum()))
        self.tables = [remap[t] for t in self.tables]
        return remap

    def stats(self) -> dict:
        out = {"rows": 0, "live": 0}
        for sh in self.shards:
            st = sh.stats()
            out["rows"] += st["rows"]
            out["live"] += st["live"]
        return out

    def totals(self):
        n = d = 0
        for sh in self.shards:
            a, b = sh.totals()
            n, d = n + a, d + b
        return n, d

    def global_stats(self, queries):
        terms = np.unique(np.asarray([int(t) for q in queries for t in q], dtype=np.int64)).astype(np.int32)
        n_live, sum_dl = self.totals()
        df = np.zeros(terms.size, np.int64)
        for sh in self.shards:
            df += np.asarray(sh.df(terms), np.int64)
        return n_live, sum_dl, terms, df

    def search(self, queries, k: int, allow=None, mask_key: int = 0):
        Bq = len(queries)
        st = self.global_stats(queries)
        scores, rows = [], []
        for s, sh in enumerate(self.shards):
            a = None if allow is None else np.asarray(allow, dtype=np.uint8)[self.tables[s]]
            # a shard's device mask cache is keyed per shard (0 = never cached)
            mk = (int(mask_key) << 6) | s if (a is not None and mask_key) else 0
            # merged on the exact fixed-point scores (fp32 rounds them above 256, where a merge
            # on fp32 would order two distinct scores by row): one index's order for every score
            sc, r, fx = sh.search(queries, k, allow=a, mask_key=mk, global_stats=st, fixed=True)
            t = self.tables[s]
            g = np.where(r >= 0, t[np.clip(r, 0, None)] if len(t) else -1, -1)
            scores.append(np.where(g >= 0, np.asarray(fx, np.int64), -1))
            rows.append(g)
        S, R = np.concatenate(scores, 1), np.concatenate(rows, 1)
        out_s = np.full((Bq, k), -np.inf, np.float32)
        out_r = np.full((Bq, k), -1, np.int64)
        for b in range(Bq):
            big = np.where(R[b] >= 0, R[b], np.iinfo(np.int64).max)
            o = np.lexsort((big, -S[b]))[:k]
            ok = R[b][o] >= 0
            out_s[b, : ok.sum()] = S[b][o][ok].astype(np.float32) / np.float32(65536.0)
            out_r[b, : ok.sum()] = R[b][o][ok]
        return out_s, out_r

    def score_rows(self, queries, rows, fixed: bool = False):
        """NativeLexIndex.score_rows with global rows: every pair goes to the shard that owns its
        row and is scored with the corpus-wide statistics (global_stats(queries)), so the result
        equals one index's bit for bit; -inf for a row < 0 (a -1 padded list), outside the
        collection or tombstoned."""
        Bq = len(queries)
        r = np.asarray(rows, dtype=np.int64)
        if r.ndim != 2 or r.shape[0] != Bq:
            raise ValueError(f"rows must be [{Bq}, K], got {r.shape}")
        n = self._n()
        _, owner_of, local_of = self._route(np.zeros(0, np.int64))
        ok = (r >= 0) & (r < n)
        safe = np.where(ok, r, 0)
        owner = np.where(ok, owner_of[safe] if n else -1, -1)
        out = np.full(r.shape, -np.inf, dtype=np.float32)
        out_fx = np.zeros(r.shape, dtype=np.uint32)
        st = self.global_stats(queries) if r.size else None
        for s, sh in enumerate(self.shards):
            mine = owner == s
            if not mine.any():
                continue
            local = np.where(mine, local_of[safe] if n else -1, -1)
            got, fx = sh.score_rows(queries, local, global_stats=st, fixed=True)
            out[mine] = np.asarray(got, np.float32)[mine]
            out_fx[mine] = np.asarray(fx, np.uint32)[mine]
        return (out, out_fx) if fixed else out

    def hybrid(self, store, queries, query_terms, k: int, k_each: Optional[int] = None,
               rank_const: int = 1, min_score: float = float("-inf"), allow=None, mask_key: int = 0,
               fusion: str = "rrf", alpha: float = 0.5):
        """Dense top-k_each over the sharded store and BM25 top-k_each over these shards, fused by
        rrf (sr_hybrid_search's three steps on a sharded collection) or, with ``fusion`` "relative"
        / "floor", by score (sr_hybrid_search_fused's steps).  Score fusion works on the MERGED
        lists: the dense side merges on similarities (ShardedStore.search_sim), the normalisation
        sees the collection's lists, never a shard's, and "floor" completes the dense side through
        ShardedStore.score_rows ("floor_full" also the BM25 side, through score_rows of the merged
        dense list), so the result equals a single-device collection's bit for bit."""
        mode = fusion_mode(fusion)
        k_each = int(k_each or k)
        if mode is None:
            _, dense = store.search(queries, k_each, allow=allow, mask_key=mask_key)
            _, lex = self.search(query_terms, k_each, allow=allow, mask_key=mask_key)
            return _rrf_rows(dense, lex, k, rank_const, min_score, self.devices[0])
        check_alpha(alpha)
        sims, dense = store.search_sim(queries, k_each, allow=allow, mask_key=mask_key)
        lsc, lex = self.search(query_terms, k_each, allow=allow, mask_key=mask_key)
        full = mode == N.SR_FUSE_FLOOR_FULL
        side = store.score_rows(queries, lex) if (mode == N.SR_FUSE_FLOOR or full) else None
        side_b = unknown_where_zero(self.score_rows(query_terms, dense)) if full else None
        score, rows, _, _ = _fuse_rows(sims, dense, lsc, lex, side, N.SR_FUSE_FLOOR if full else mode,
                                       alpha, -1.0, 0.0, min_score, k, self.devices[0], side_b)
        return score, rows

    def save(self, path: str) -> None:
        import json
        import os
        for i, sh in enumerate(self.shards):
            sh.save(f"{path}.s{i}")
        np.savez(f"{path}.rows.tmp.npz", **{f"s{i}": t for i, t in enumerate(self.tables)})
        os.replace(f"{path}.rows.tmp.npz", f"{path}.rows.npz")
        with open(path + ".tmp", "w") as f:
            json.dump({"magic": self.MAGIC, "shards": len(self.shards)}, f)
        os.replace(path + ".tmp", path)

    @classmethod
    def is_manifest(cls, path: str) -> bool:
        with open(path, "rb") as f:
            return cls.MAGIC.encode() in f.read(64)

    @classmethod
    def load(cls, path: str, store, loader=None) -> "ShardedLex":
        import json
        with open(path) as f:
            man = json.load(f)
        if man.get("magic") != cls.MAGIC or int(man["shards"]) != len(store.devices):
            raise IOError(f"{path}: a {man.get('shards')}-shard lexical index cannot load on "
                          f"devices {store.devices}")
        loader = loader or (lambda p, dev: NativeLexIndex.load(p, dev))
        shards = [loader(f"{path}.s{i}", d) for i, d in enumerate(store.devices)]
        with np.load(f"{path}.rows.npz") as z:
            tables = [z[f"s{i}"].astype(np.int64) for i in range(len(store.devices))]
        return cls(store, _shards=shards, _tables=tables)


def _rrf_rows(rows_a, rows_b, k, rank_const, min_score, device):
    """rrf of two host row lists on the device (rrf_fuse), or through the test seam."""
    return _rrf_impl[0](rows_a, rows_b, k, rank_const, min_score, device)


def _fuse_rows(score_a, rows_a, score_b, rows_b, side_a, mode, alpha, floor_a, floor_b, min_score, k,
               device, side_b=None):
    """score_fuse of two host lists on the device, or through the test seam (which sees ``side_b``
    as a keyword, and only when there is one: a seam of before side_b keeps working)."""
    kw = {} if side_b is None else {"side_b": side_b}
    return _fuse_impl[0](score_a, rows_a, score_b, rows_b, side_a, mode, alpha, floor_a, floor_b,
                         min_score, k, device, **kw)


def unknown_where_zero(score) -> np.ndarray:
    """BM25 pair scores -> "floor_full"'s side_b: a score of exactly 0 (the row matches nothing)
    becomes -inf, unknown, so that row fuses as it does in "floor"."""
    s = np.asarray(score, dtype=np.float32)
    return np.where(s == 0, np.float32(-np.inf), s).astype(np.float32)


FUSIONS = ("rrf", "relative", "floor", "floor_full")


def fusion_mode(fusion: str):
    """Fusion name -> None for "rrf", else the SR_FUSE_* mode; ValueError for an unknown name."""
    if fusion == "rrf":
        return None
    if fusion == "relative":
        return N.SR_FUSE_MINMAX
    if fusion == "floor":
        return N.SR_FUSE_FLOOR
    if fusion == "floor_full":
        return N.SR_FUSE_FLOOR_FULL
    raise ValueError(f"unsupported fusion '{fusion}' (one of {', '.join(FUSIONS)})")


def check_alpha(alpha) -> float:
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise ValueError(f"alpha must be in [0, 1] (the weight of the dense side), got {alpha}")
    return a


def _dev_i32(t):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError("device-resident lexical queries must be CUDA tensors")
    return t.to(torch.int32).contiguous()


def rrf_fuse(rows_a, rows_b, k: int, rank_const: int = 1, min_score: float = 0.0,
             device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Device rrf of two ranked row lists per query ([B, ka], [B, kb], -1 padded)."""
    N.require_gpu()
    a = np.ascontiguousarray(np.asarray(rows_a, dtype=np.int64))
    b = np.ascontiguousarray(np.asarray(rows_b, dtype=np.int64))
    Bq = a.shape[0]
    assert b.shape[0] == Bq
    scores = np.empty((Bq, k), dtype=np.float64)
    rows = np.empty((Bq, k), dtype=np.int64)
    N.call("sr_rrf_fuse", N.ptr(a), a.shape[1], N.ptr(b), b.shape[1], Bq, int(rank_const),
           float(min_score), int(k), N.ptr(scores), N.ptr(rows), int(device))
    return scores, rows


def rrf_fuse_dev(rows_a, rows_b, k: int, rank_const: int = 1, min_score: float = float("-inf"),
                 stream=None):
    """rrf of two ranked row lists per query on the device (torch int64 [B, ka], [B, kb], -1
    padded) -> (score [B, k] fp64, rows [B, k] int64) device tensors."""
    import torch
    a, b = rows_a.contiguous(), rows_b.contiguous()
    Bq = a.shape[0]
    scores = torch.empty((Bq, k), dtype=torch.float64, device=a.device)
    rows = torch.empty((Bq, k), dtype=torch.int64, device=a.device)
    N.call("sr_rrf_fuse_dev", N.ptr(a), a.shape[1], N.ptr(b), b.shape[1], Bq, int(rank_const),
           float(min_score), int(k), N.ptr(scores), N.ptr(rows), a.device.index or 0,
           N.stream_handle(stream))
    return scores, rows


def _fuse_list_mode(mode, who: str) -> int:
    m = fusion_mode(mode) if isinstance(mode, str) else int(mode)
    if m is None or m == N.SR_FUSE_FLOOR_FULL:
        raise ValueError(f"{who}: mode must be 'relative' or 'floor' ('floor_full' is 'floor' with "
                         "side_a and side_b)")
    return m


def score_fuse(score_a, rows_a, score_b, rows_b, k: int, mode: str = "relative", alpha: float = 0.5,
               side_a=None, floor_a: float = -1.0, floor_b: float = 0.0,
               min_score: float = float("-inf"), device: int = 0, side_b=None):
    """Device score fusion of two scored row lists per query (sr_score_fuse; host arrays score
    [B, ka] fp32 / rows [B, ka] int64 and the same with kb; row < 0 = absent; ``side_a`` [B, kb]:
    the a-metric score of each b row, -inf = unknown; ``side_b`` [B, ka]: its mirror, the b-metric
    score of each a row, sr_score_fuse_sides).  ``mode``: "relative" (min-max of each
    list) or "floor" (lo = floor_a / floor_b).  Returns (fused [B,k] fp32 desc, rows [B,k] int64,
    a [B,k] fp32, b [B,k] fp32): -inf / -1 / -inf / -inf in unfilled slots."""
    m = _fuse_list_mode(mode, "score_fuse")
    N.require_gpu()
    ra = np.ascontiguousarray(np.asarray(rows_a, dtype=np.int64))
    rb = np.ascontiguousarray(np.asarray(rows_b, dtype=np.int64))
    Bq = ra.shape[0]
    sa = np.ascontiguousarray(np.asarray(score_a, dtype=np.float32).reshape(ra.shape))
    sb = np.ascontiguousarray(np.asarray(score_b, dtype=np.float32).reshape(rb.shape))
    assert ra.ndim == 2 and rb.ndim == 2 and rb.shape[0] == Bq
    sd = None
    if side_a is not None:
        sd = np.ascontiguousarray(np.asarray(side_a, dtype=np.float32).reshape(rb.shape))
    ka, kb = ra.shape[1], rb.shape[1]
    k = int(k)
    out = [np.empty((Bq, max(k, 0)), dtype=t) for t in (np.float32, np.int64, np.float32, np.float32)]
    lists = (N.ptr(sa) if ka and Bq else None, N.ptr(ra) if ka and Bq else None, ka,
             N.ptr(sb) if kb and Bq else None, N.ptr(rb) if kb and Bq else None, kb,
             N.ptr(sd) if (sd is not None and kb and Bq) else None)
    tail = (Bq, m, float(alpha), float(floor_a), float(floor_b), float(min_score), k, N.ptr(out[0]),
            N.ptr(out[1]), N.ptr(out[2]), N.ptr(out[3]), int(device))
    if side_b is None:
        N.call("sr_score_fuse", *lists, *tail)
    else:
        sdb = np.ascontiguousarray(np.asarray(side_b, dtype=np.float32).reshape(ra.shape))
        N.call("sr_score_fuse_sides", *lists, N.ptr(sdb) if ka and Bq else None, *tail)
    return tuple(out)


def score_fuse_dev(score_a, rows_a, score_b, rows_b, k: int, mode: str = "relative",
                   alpha: float = 0.5, side_a=None, floor_a: float = -1.0, floor_b: float = 0.0,
                   min_score: float = float("-inf"), stream=None, side_b=None):
    """score_fuse on device tensors (torch fp32 / int64 [B, ka], [B, kb]; sr_score_fuse_dev, or
    sr_score_fuse_sides_dev with ``side_b`` [B, ka]), asynchronous on ``stream`` -> device tensors
    (fused, rows, a, b) [B, k]."""
    import torch
    m = _fuse_list_mode(mode, "score_fuse_dev")
    ra, rb = rows_a.contiguous(), rows_b.contiguous()
    sa, sb = score_a.contiguous(), score_b.contiguous()
    assert ra.is_cuda and ra.dtype == torch.int64 and rb.dtype == torch.int64
    assert sa.dtype == torch.float32 and sb.dtype == torch.float32
    assert sa.shape == ra.shape and sb.shape == rb.shape and ra.dim() == 2 and rb.shape[0] == ra.shape[0]
    sd = None
    if side_a is not None:
        sd = side_a.contiguous()
        assert sd.dtype == torch.float32 and sd.shape == rb.shape
    Bq, k = ra.shape[0], int(k)
    dev = ra.device
    out = [torch.empty((Bq, max(k, 0)), dtype=t, device=dev)
           for t in (torch.float32, torch.int64, torch.float32, torch.float32)]
    lists = (N.ptr(sa), N.ptr(ra), ra.shape[1], N.ptr(sb), N.ptr(rb), rb.shape[1],
             None if sd is None else N.ptr(sd))
    tail = (Bq, m, float(alpha), float(floor_a), float(floor_b), float(min_score), k, N.ptr(out[0]),
            N.ptr(out[1]), N.ptr(out[2]), N.ptr(out[3]), dev.index or 0, N.stream_handle(stream))
    if side_b is None:
        N.call("sr_score_fuse_dev", *lists, *tail)
    else:
        sdb = side_b.contiguous()
        assert sdb.dtype == torch.float32 and sdb.shape == ra.shape
        N.call("sr_score_fuse_sides_dev", *lists, N.ptr(sdb), *tail)
    return tuple(out)


def hybrid_search(store, lex: NativeLexIndex, queries, query_terms: Sequence[Sequence[int]], k: int,
                  k_each: Optional[int] = None, rank_const: int = 1,
                  min_score: float = float("-inf"), allow=None, mask_key: int = 0,
                  fusion: str = "rrf", alpha: float = 0.5, components: bool = False):
    """Dense top-k_each (cosine, store) and BM25 top-k_each (lex) fused on the device.
    ``fusion`` "rrf" (default): reciprocal rank -> (rrf score [B,k] fp64 desc, rows [B,k] int64).
    "relative" / "floor" / "floor_full": score fusion (sr_hybrid_search_fused) with ``alpha`` the
    weight of the dense side ("floor" completes the dense side with the exact cosines of the BM25
    rows, "floor_full" also the BM25 side with the exact BM25 of the dense rows) -> (fused score [B,k] fp32 desc, rows [B,k] int64), and with ``components`` also the
    cosine and the BM25 score of each kept row (-inf where unknown)."""
    mode = fusion_mode(fusion)
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
    if q.ndim == 1:
        q = q[None]
    Bq = q.shape[0]
    assert len(query_terms) == Bq
    k_each = int(k_each or k)
    if mode is not None:
        check_alpha(alpha)
        out = [np.empty((Bq, k), dtype=t) for t in (np.float32, np.int64, np.float32, np.float32)]
        if Bq:
            qoff, qterms = query_arrays(query_terms)
            a = None if allow is None else _mask(allow, store.count()[0])
            N.call("sr_hybrid_search_fused", store._h, lex._h, N.ptr(q), N.ptr(qoff), N.ptr(qterms),
                   Bq, int(k), k_each, mode, float(alpha), float(min_score),
                   None if a is None else N.ptr(a), int(mask_key), N.ptr(out[0]), N.ptr(out[1]),
                   N.ptr(out[2]), N.ptr(out[3]))
        return tuple(out) if components else (out[0], out[1])
    scores = np.empty((Bq, k), dtype=np.float64)
    rows = np.empty((Bq, k), dtype=np.int64)
    if Bq == 0:
        return scores, rows
    qoff, qterms = query_arrays(query_terms)
    a = None if allow is None else _mask(allow, store.count()[0])
    N.call("sr_hybrid_search", store._h, lex._h, N.ptr(q), N.ptr(qoff), N.ptr(qterms), Bq, int(k),
           k_each, int(rank_const), float(min_score), None if a is None else N.ptr(a),
           int(mask_key), N.ptr(scores), N.ptr(rows))
    return scores, rows


def lex_scoring(handle) -> int:
    """SR_LEX_BM25 or SR_LEX_IMPACT of a native sr_lex handle (sr_lex_scoring)."""
    m = ctypes.c_int32(0)
    N.call("sr_lex_scoring", handle, ctypes.byref(m))
    return int(m.value)


def weighted_arrays(items):
    """[(terms, weights) | {term: weight}] -> (off int64[n+1], terms int32, weights fp32), the C-ABI
    layout of sr_lex_add_weighted documents and sr_lex_search_weighted queries."""
    off = np.zeros(len(items) + 1, dtype=np.int64)
    flat_t: list = []
    flat_w: list = []
    for i, it in enumerate(items):       # (one pass over Python lists: a query batch is packed per call)
        if isinstance(it, dict):
            t, w = list(it.keys()), list(it.values())
        else:
            t, w = it
            t = t.tolist() if hasattr(t, "tolist") else list(t)
            w = w.tolist() if hasattr(w, "tolist") else list(w)
        if len(t) != len(w):
            raise ValueError(f"item {i}: {len(t)} terms but {len(w)} weights")
        flat_t += t
        flat_w += w
        off[i + 1] = len(flat_t)
    if not flat_t:
        return off, np.zeros(1, np.int32), np.ones(1, np.float32)
    terms = np.asarray(flat_t, dtype=np.int64)
    if terms.min() < -2**31 or terms.max() >= 2**31:
        raise ValueError("term id outside int32")
    return off, terms.astype(np.int32), np.asarray(flat_w, dtype=np.float32)


class NativeImpactIndex:
    """Learned-sparse index over the rows of a store, resident in HBM of one device: sr_lex in its
    impact scoring mode (k_lex.hip).  A document and a query are term ids with fp32 weights (bge-m3's
    sparse head, SPLADE, any "sparse vector"); a row's score is the dot product over shared terms in
    2^-16 fixed point, every product rounded on its own (exact and order-independent; DESIGN.md
    "Learned-sparse retrieval").  Document weights lie in (0, 16], query weights are >= 0."""

    def __init__(self, device: int = 0, _handle=None):
        self._h = None
        if _handle is None:
            N.require_gpu()
            h = ctypes.c_void_p()
            N.call("sr_lex_create_impact", int(device), ctypes.byref(h))
            _handle = h
        self._h = _handle
        self.device = int(device)

    @classmethod
    def load(cls, path: str, device: int = 0) -> "NativeImpactIndex":
        N.require_gpu()
        h = ctypes.c_void_p()
        N.call("sr_lex_load", path.encode(), int(device), ctypes.byref(h))
        if lex_scoring(h) != N.SR_LEX_IMPACT:
            N.load().sr_lex_destroy(h)
            raise ValueError(f"{path} is a BM25 snapshot: load it with NativeLexIndex.load")
        return cls(device, _handle=h)

    close = NativeLexIndex.close
    __del__ = NativeLexIndex.__del__
    remove = NativeLexIndex.remove
    compact = NativeLexIndex.compact
    save = NativeLexIndex.save
    stats = NativeLexIndex.stats

    def add(self, docs) -> int:
        """Append documents, each (terms, weights) or {term: weight} with distinct terms; returns
        the first row id."""
        if not len(docs):
            return self.stats()["rows"]
        return self.add_arrays(*weighted_arrays(docs))

    def add_arrays(self, off, terms, weights) -> int:
        """Bulk append in the C-ABI layout (weighted_arrays output)."""
        off = np.ascontiguousarray(off, dtype=np.int64)
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        if terms.size == 0:
            terms, weights = np.zeros(1, np.int32), np.ones(1, np.float32)
        first = ctypes.c_int64(0)
        N.call("sr_lex_add_weighted", self._h, N.ptr(off), N.ptr(terms), N.ptr(weights), len(off) - 1,
               ctypes.byref(first))
        return int(first.value)

    def search(self, queries, k: int, allow=None, mask_key: int = 0, fixed: bool = False):
        """Impact top-k per query ((terms, weights) or {term: weight}; a repeated id keeps its
        maximum weight) -> (score [B,k] fp32 desc, rows [B,k] int64), -inf / -1 past the matches;
        fixed: also the exact 2^-16 fixed-point scores [B,k] uint32."""
        Bq = len(queries)
        scores = np.empty((Bq, k), dtype=np.float32)
        rows = np.empty((Bq, k), dtype=np.int64)
        fx = np.zeros((Bq, k), dtype=np.uint32) if fixed else None
        if Bq:
            qoff, qterms, qw = weighted_arrays(queries)
            a = None if allow is None else _mask(allow, self.stats()["rows"])
            N.call("sr_lex_search_weighted", self._h, N.ptr(qoff), N.ptr(qterms), N.ptr(qw), Bq, int(k),
                   None if a is None else N.ptr(a), int(mask_key), N.ptr(scores), N.ptr(rows),
                   N.ptr(fx) if fixed else None)
        return (scores, rows, fx) if fixed else (scores, rows)

    def score_rows(self, queries, rows, fixed: bool = False):
        """Exact impact score of given (query, row) pairs (sr_lex_score_rows_weighted): rows [B, K]
        int64 -> score [B, K] fp32, the score search gives that row: -inf for a row < 0, past the
        index or tombstoned, 0 for a live row that shares no scored term."""
        Bq = len(queries)
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        if r.ndim != 2 or r.shape[0] != Bq:
            raise ValueError(f"rows must be [{Bq}, K], got {r.shape}")
        score = np.empty(r.shape, dtype=np.float32)
        fx = np.zeros(r.shape, dtype=np.uint32) if fixed else None
        if r.size:
            qoff, qterms, qw = weighted_arrays(queries)
            N.call("sr_lex_score_rows_weighted", self._h, N.ptr(qoff), N.ptr(qterms), N.ptr(qw), Bq,
                   N.ptr(r), r.shape[1], N.ptr(score), N.ptr(fx) if fixed else None)
        return (score, fx) if fixed else score


def sparse_hybrid_search(store, index: NativeImpactIndex, q, q_sparse, k: int,
                         k_each: Optional[int] = None, fusion: str = "rrf", alpha: float = 0.5,
                         min_score: float = float("-inf"), allow=None, mask_key: int = 0,
                         rank_const: int = 1):
    """Dense + learned-sparse retrieval: dense top-k_each (store.search_sim) and impact top-k_each
    (index.search of ``q_sparse``), fused on the device by hybrid_search's rules with the impact
    score in BM25's place.  "rrf" -> (rrf score [B,k] fp64, rows); "relative": min-max of each
    list; "floor": floor_a = -1, floor_b = 0 and the dense side completed with the exact cosines
    of the sparse list's rows; "floor_full": also the sparse side completed with the exact impact
    scores of the dense list's rows, an exact 0 passed as unknown -> (fused [B,k] fp32, rows)."""
    mode = fusion_mode(fusion)
    qd = np.ascontiguousarray(np.asarray(q, dtype=np.float32))
    if qd.ndim == 1:
        qd = qd[None]
    if len(q_sparse) != qd.shape[0]:
        raise ValueError(f"{qd.shape[0]} dense queries but {len(q_sparse)} sparse ones")
    k_each = int(k_each or k)
    sims, dense = store.search_sim(qd, k_each, allow=allow, mask_key=mask_key)
    ssc, sparse = index.search(q_sparse, k_each, allow=allow, mask_key=mask_key)
    if mode is None:
        return rrf_fuse(dense, sparse, k, rank_const, min_score, index.device)
    check_alpha(alpha)
    full = mode == N.SR_FUSE_FLOOR_FULL
    side_a = store.score_rows(qd, sparse) if (mode == N.SR_FUSE_FLOOR or full) else None
    side_b = unknown_where_zero(index.score_rows(q_sparse, dense)) if full else None
    score, rows, _, _ = score_fuse(sims, dense, ssc, sparse, k, N.SR_FUSE_FLOOR if full else mode,
                                   alpha, side_a, -1.0, 0.0, min_score, index.device, side_b=side_b)
    return score, rows


_rrf_impl = [lambda a, b, k, rc, ms, dev: rrf_fuse(a, b, k, rc, ms, dev)]


def _fuse_native(sa, ra, sb, rb, side, mode, alpha, fa, fb, ms, k, dev, side_b=None):
    return score_fuse(sa, ra, sb, rb, k, mode, alpha, side, fa, fb, ms, dev, side_b=side_b)


_fuse_impl = [_fuse_native]


def set_rrf_backend(fn) -> None:
    """Test seam: replace the host-list rrf used by ShardedLex.hybrid (CPU doubles)."""
    _rrf_impl[0] = fn or (lambda a, b, k, rc, ms, dev: rrf_fuse(a, b, k, rc, ms, dev))


def set_fuse_backend(fn) -> None:
    """Test seam: replace the host-list score fusion used by ShardedLex.hybrid (CPU doubles);
    fn(score_a, rows_a, score_b, rows_b, side_a, mode, alpha, floor_a, floor_b, min_score, k,
    device[, side_b=...]) -> (fused, rows, a, b); side_b is passed only for "floor_full"."""
    _fuse_impl[0] = fn or _fuse_native
