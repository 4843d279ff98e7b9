"""Per-pair BM25 reference (tests helper): the exact fixed-point score of one (query, row) pair, in
np.float32 scalars so that every operation rounds once, as the kernel's do (k_lex.hip
lex_score_rows; include/super_rag_mi355x.h, sr_lex_score_rows).

It walks THE ROW'S OWN postings, (term, tf) pairs in the order they were added, and sums the weight of
every posting whose term is one of the query's scored terms; oracle.bm25.bm25_fixed_scores walks the
term lists of an inverted index instead, so the two agree only if both are right.  Only idf32 and
avgdl32, the two definitions with a libm call or a division by a count, are taken from the oracle.

  scored terms = distinct query terms t with 0 <= t < vocabulary and live df(t) > 0
  mult(t)      = occurrences of t in the query
  w(p)         = idf(t_p) * ((tf_p * (k1 + 1)) / (tf_p + k1 * ((1 - b) + b * (dl_r / avgdl))))   fp32
  fixed(b, r)  = sum over the postings p of row r with t_p scored of max(1, rint(w(p) * 2^16)) * mult(t_p)
  score        = fp32(fixed) / 2^16
A row < 0, >= rows or tombstoned has no score (-inf / 0); a live row without a scored term scores 0.
"""
from __future__ import annotations

import functools
from collections import Counter

import numpy as np

from oracle.bm25 import LexCorpus, avgdl32, idf32

F = np.float32
SCALE = F(65536.0)


@functools.lru_cache(maxsize=None)
def _weight(idf_bits: int, tf: int, dl: int, adl_bits: int, k1: float, b: float) -> int:
    """max(1, rint(w * 2^16)) of one posting; the fp32 inputs come as bit patterns (cache keys)."""
    idf = np.uint32(idf_bits).view(F)
    adl = np.uint32(adl_bits).view(F)
    k1, b = F(k1), F(b)
    omb, k1p1 = F(F(1.0) - b), F(k1 + F(1.0))
    t1 = F(F(dl) / adl)
    norm = F(k1 * F(omb + F(b * t1)))
    w = F(idf * F(F(F(tf) * k1p1) / F(F(tf) + norm)))
    q = np.rint(F(w * SCALE))
    return 1 if q < 1 else int(q)


def _bits(x) -> int:
    return int(np.asarray(x, F).reshape(1).view(np.uint32)[0])


def query_table(corpus: LexCorpus, query, stats=None):
    """{term: (idf fp32 bits, mult)} of the query's scored terms, and avgdl's fp32 bits.  stats =
    (n_live, sum_dl, df: term -> int) of a whole row-sharded corpus, or None for this corpus's own."""
    if stats is None:
        n_live = int(corpus.live.sum())
        adl = avgdl32(corpus.dl, corpus.live)
        df_of = lambda t: int(corpus.df[t])
    else:
        n_live, sum_dl, df_of = int(stats[0]), int(stats[1]), stats[2]
        adl = F(float(sum_dl) / n_live) if n_live > 0 else F(1.0)
    table = {}
    for t, mult in Counter(int(x) for x in query).items():
        if t < 0 or t >= corpus.vocab or corpus.df[t] == 0:
            continue
        table[t] = (_bits(idf32(n_live, df_of(t))), mult)
    return table, _bits(adl)


def pair_fixed(corpus: LexCorpus, table, adl_bits: int, row: int, k1=1.2, b=0.75):
    """Fixed-point score of one row for a query_table, or None for a row without a score."""
    if row < 0 or row >= corpus.n or not corpus.live[row]:
        return None
    dl = int(corpus.dl[row])
    acc = 0
    for p in range(int(corpus.off[row]), int(corpus.off[row + 1])):   # the row's own postings
        e = table.get(int(corpus.terms[p]))
        if e is not None:
            acc += _weight(e[0], int(corpus.tf[p]), dl, adl_bits, float(k1), float(b)) * e[1]
    return acc


def score_rows(corpus: LexCorpus, queries, rows, k1=1.2, b=0.75, stats=None):
    """-> (score [B, K] fp32, fixed [B, K] uint32) for rows [B, K]; -inf / 0 where a row has no score.
    stats: one (n_live, sum_dl, df) for every query, or a list with one per query."""
    rows = np.asarray(rows, np.int64)
    score = np.full(rows.shape, -np.inf, F)
    fixed = np.zeros(rows.shape, np.uint32)
    for i, q in enumerate(queries):
        table, adl_bits = query_table(corpus, q, stats[i] if isinstance(stats, list) else stats)
        for j, r in enumerate(rows[i].tolist()):
            acc = pair_fixed(corpus, table, adl_bits, r, k1, b)
            if acc is not None:
                assert acc < 2 ** 32, "fixed-point accumulator overflow"
                fixed[i, j] = acc
                score[i, j] = F(acc) / SCALE
    return score, fixed
