"""The impact (learned-sparse) scoring of k_lex.hip and the token -> term collapse of the sparse
head, restated in numpy float32 (include/super_rag_mi355x.h, "Learned-sparse retrieval").

Scoring.  For every posting (term t, weight dw) of a live eligible row and a query weight qw_t:
p = fl32(qw_t * dw), one fp32 multiply; fixed = max(1, rint(p * 65536)) as an integer (rint: ties to
even); a row's score is the integer sum over its postings whose term the query scores, a term held
in two postings counting twice; score = fp32(fixed) / 65536.  Order (fixed desc, row asc).
Query preparation.  Weights must be finite and >= 0 and document weights finite and in (0, 16]
(ValueError); a zero-weight term is dropped; a repeated id keeps its MAXIMUM weight; ids the index
does not score (< 0, >= vocabulary, no live posting) are ignored; the query is rejected when the sum
over its distinct ids of 16 * qw * 65536 + 1, in double, reaches 2^32.
Collapse.  A position qualifies when mask != 0, tw > 0 and its id is no special id; every distinct
qualifying id once, with the maximum tw over its qualifying positions, in ascending order of its first
qualifying position (bge-m3's _process_token_weights as an insertion-ordered dict).
"""
from __future__ import annotations

import numpy as np

F = np.float32
SCALE = F(65536.0)
MAX_WEIGHT = 16.0


def query_bound(qd) -> float:
    """sum over the prepared query's terms of 16 * qw * 65536 + 1, in double."""
    return float(sum(MAX_WEIGHT * float(w) * 65536.0 + 1.0 for w in qd.values()))


def overflows(qd) -> bool:
    return query_bound(qd) >= 4294967296.0


def prepare_query(terms, weights, scored=None):
    """-> {term: fp32 weight} in first-occurrence order: zero weights dropped, a repeated id keeps
    its maximum; ValueError for a weight that is negative or not finite and for a query past the
    overflow bound (both judged before ``scored``); then ids for which ``scored(t)`` is false (the
    index does not know them, or every posting is dead) are dropped."""
    t = np.asarray(terms, np.int64).reshape(-1)
    w = np.asarray(weights, F).reshape(-1)
    if t.shape != w.shape:
        raise ValueError("terms and weights differ in length")
    if not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("query weights must be finite and >= 0")
    qd = {}
    for ti, wi in zip(t.tolist(), w):
        if wi == 0:
            continue
        if ti not in qd or wi > qd[ti]:
            qd[ti] = wi
    if overflows(qd):
        raise ValueError("query weights too large")
    if scored is not None:
        qd = {ti: wi for ti, wi in qd.items() if scored(ti)}
    return qd


def as_query(q):
    """(terms, weights) or {term: weight} -> (terms, weights)."""
    if isinstance(q, dict):
        return list(q.keys()), list(q.values())
    return q


def fixed_products(qw, dw) -> np.ndarray:
    """max(1, rint(fl32(qw * dw) * 65536)) elementwise, as uint64."""
    p = np.asarray(qw, F) * np.asarray(dw, F)               # one rounded fp32 multiply
    q = np.rint(p * SCALE)                                  # exact scaling, ties to even
    return np.maximum(q, F(1.0)).astype(np.uint64)


class ImpactCorpus:
    """Rows of (term, weight) postings in the C-ABI layout: off int64 [n + 1], terms int32, weights
    fp32; live bool [n]."""

    def __init__(self, off, terms, weights, live=None):
        self.off = np.asarray(off, np.int64)
        self.terms = np.asarray(terms, np.int64)[: self.off[-1]]
        self.weights = np.asarray(weights, F)[: self.off[-1]]
        self.n = len(self.off) - 1
        if self.weights.size and not (np.isfinite(self.weights).all() and (self.weights > 0).all()
                                      and (self.weights <= F(MAX_WEIGHT)).all()):
            raise ValueError("document weights must be finite and in (0, 16]")
        self.live = np.ones(self.n, bool) if live is None else np.asarray(live, bool).copy()
        self.row = np.repeat(np.arange(self.n), np.diff(self.off))
        order = np.argsort(self.terms, kind="stable")
        self._order, self._sorted = order, self.terms[order]

    def postings(self, t) -> np.ndarray:
        """Indices of the postings of term t (all rows, dead ones too), ascending."""
        lo, hi = np.searchsorted(self._sorted, [t, t + 1])
        return self._order[lo:hi]

    def remove(self, rows):
        self.live[np.asarray(rows, np.int64)] = False

    def keep(self, rows):
        """The corpus of the rows ``rows`` (ascending), renumbered from 0: compact, or a slice."""
        rows = np.asarray(rows, np.int64)
        sel = np.concatenate([np.arange(self.off[r], self.off[r + 1]) for r in rows]) if len(rows) \
            else np.zeros(0, np.int64)
        sel = sel.astype(np.int64)
        off = np.concatenate([[0], np.cumsum(self.off[rows + 1] - self.off[rows])]) if len(rows) \
            else np.zeros(1, np.int64)
        return ImpactCorpus(off, self.terms[sel], self.weights[sel], self.live[rows])

    def scored(self, t) -> bool:
        """Whether the index scores term id t: a live posting of it exists."""
        return bool(self.live[self.row[self.postings(t)]].any())

    def fixed_scores(self, query, allow=None) -> np.ndarray:
        """The integer score of every row (0: dead, not allowed or nothing shared), uint64 [n]."""
        qd = prepare_query(*as_query(query), scored=self.scored)
        acc = np.zeros(self.n, np.uint64)
        ok = self.live if allow is None else (self.live & (np.asarray(allow) != 0))
        for t, qw in qd.items():
            sel = self.postings(t)
            sel = sel[ok[self.row[sel]]]
            np.add.at(acc, self.row[sel], fixed_products(qw, self.weights[sel]))
        assert acc.max(initial=0) < 2 ** 32
        return acc


def topk(corpus: ImpactCorpus, queries, k, allow=None):
    """-> (score [B,k] fp32, rows [B,k] int64, fixed [B,k] uint32): (fixed desc, row asc); -inf / -1 /
    0 past the matching rows."""
    B = len(queries)
    scores = np.full((B, k), -np.inf, F)
    rows = np.full((B, k), -1, np.int64)
    fixed = np.zeros((B, k), np.uint32)
    for i, q in enumerate(queries):
        acc = corpus.fixed_scores(q, allow)
        hit = np.nonzero(acc)[0]
        order = hit[np.lexsort((hit, -acc[hit].astype(np.int64)))][:k]
        m = len(order)
        rows[i, :m] = order
        fixed[i, :m] = acc[order]
        scores[i, :m] = acc[order].astype(F) / SCALE
    return scores, rows, fixed


def score_rows(corpus: ImpactCorpus, queries, rows):
    """-> (score [B,K] fp32, fixed [B,K] uint32): -inf / 0 for a row < 0, >= n or dead; 0.0 / 0 for a
    live row sharing no scored term."""
    rows = np.asarray(rows, np.int64)
    score = np.full(rows.shape, -np.inf, F)
    fixed = np.zeros(rows.shape, np.uint32)
    for i, q in enumerate(queries):
        acc = corpus.fixed_scores(q)
        ok = (rows[i] >= 0) & (rows[i] < corpus.n)
        ok[ok] = corpus.live[rows[i][ok]]
        fixed[i, ok] = acc[rows[i][ok]]
        score[i, ok] = acc[rows[i][ok]].astype(F) / SCALE
    return score, fixed


def dot64(corpus: ImpactCorpus, query):
    """fp64 brute force: (dot [n], shared postings [n], sum of p over them [n]) of the live rows."""
    qd = prepare_query(*as_query(query), scored=corpus.scored)
    dot = np.zeros(corpus.n)
    shared = np.zeros(corpus.n, np.int64)
    for t, qw in qd.items():
        sel = corpus.postings(t)
        sel = sel[corpus.live[corpus.row[sel]]]
        np.add.at(dot, corpus.row[sel], float(qw) * corpus.weights[sel].astype(np.float64))
        np.add.at(shared, corpus.row[sel], 1)
    return dot, shared


def collapse(ids, mask, tw, special_ids=()):
    """-> (terms [B,S] int32, weights [B,S] fp32, count [B] int32); slots past count hold -1 / 0."""
    ids = np.asarray(ids, np.int64)
    mask = np.asarray(mask)
    tw = np.asarray(tw, F)
    B, S = ids.shape
    out_t = np.full((B, S), -1, np.int32)
    out_w = np.zeros((B, S), F)
    cnt = np.zeros(B, np.int32)
    special = np.asarray(list(special_ids), np.int64)
    for b in range(B):
        pos = np.nonzero((mask[b] != 0) & (tw[b] > 0) & ~np.isin(ids[b], special))[0]
        if not pos.size:
            continue
        uniq, first, inv = np.unique(ids[b, pos], return_index=True, return_inverse=True)
        best = np.zeros(uniq.size, F)
        np.maximum.at(best, inv.reshape(-1), tw[b, pos])
        order = np.argsort(first, kind="stable")        # pos ascends: first qualifying position
        cnt[b] = uniq.size
        out_t[b, : uniq.size] = uniq[order]
        out_w[b, : uniq.size] = best[order]
    return out_t, out_w, cnt
