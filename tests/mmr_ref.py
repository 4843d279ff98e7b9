"""fp64 numpy restatement of the two MMR modes of include/super_rag_mi355x.h (tests helper).

SR_MMR_ONEPASS restates graphiti's ``maximal_marginal_relevance`` (super_rag/graphiti/
graphiti_core/search/search_utils.py:1884-1922): a similarity matrix with a zero diagonal, the
maximum over the WHOLE row (so never below 0), score = lambda rel + (lambda - 1) max, a stable
descending sort over insertion order, scores below min_score dropped.  SR_MMR_GREEDY is the
classical iteration.  tests/test_mmr_fixture.py pins the one-pass mode to the reference's own
outputs (tests/golden/mmr_fixtures.npz).

Every function takes the query ``q`` [dim] and the candidates ``C`` [n, dim] as fp64 arrays that
are already unit (or zero) rows; ``valid`` [n] bool marks missing candidates (default: all valid).
Dots are taken pair by pair with np.dot, so exact duplicate rows get bit-equal values.
"""
from __future__ import annotations

import numpy as np


def normalize(x):
    """Rows / |row| in fp64, zero rows unchanged (graphiti normalize_l2, row-wise)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.array(x, copy=True)
    for i in range(x.shape[0]) if x.ndim == 2 else ():
        n = np.linalg.norm(x[i], 2)
        if n != 0:
            out[i] = x[i] / n
    if x.ndim == 1:
        n = np.linalg.norm(x, 2)
        out = x / n if n != 0 else out
    return out


def relevance(q, C):
    return np.array([np.dot(q, c) for c in C], dtype=np.float64)


def gram(C):
    """G_ij = c_i . c_j for i != j, zero diagonal (the reference's similarity matrix)."""
    n = len(C)
    G = np.zeros((n, n))
    for i in range(n):
        for j in range(i):
            G[i, j] = G[j, i] = np.dot(C[i], C[j])
    return G


def onepass_scores(rel, G, lam, valid=None):
    """score_i = lam rel_i + (lam - 1) max(0, max_{j != i, j valid} G_ij); -inf for missing i."""
    n = len(rel)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    Gv = np.where(valid[None, :], G, 0.0)          # missing columns take no part (diagonal is 0)
    m = Gv.max(axis=1) if n else np.zeros(0)
    return np.where(valid, lam * rel + (lam - 1) * m, -np.inf)


def mmr_onepass(q, C, lam, min_score=-2.0, k=None, valid=None):
    """(positions, scores): order (score desc, position asc), score >= min_score, first k."""
    n = len(C)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    s = onepass_scores(relevance(q, C), gram(C), lam, valid)
    order = sorted((i for i in range(n) if valid[i]), key=lambda i: s[i], reverse=True)
    order = [i for i in order if s[i] >= min_score]
    if k is not None:
        order = order[:k]
    return order, [float(s[i]) for i in order]


def greedy_values(rel, G, lam, picked, valid=None):
    """Marginal value of every candidate given the picks so far (-inf: picked or missing)."""
    n = len(rel)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    cur = np.zeros(n)
    for p in picked:
        cur = np.maximum(cur, G[:, p])
    v = lam * rel + (lam - 1) * cur
    v = np.where(valid, v, -np.inf)
    v[list(picked)] = -np.inf
    return v


def mmr_greedy(q, C, lam, min_score=-2.0, k=None, valid=None, rel=None, G=None):
    """(positions, scores) of the greedy iteration; ties go to the lower position."""
    n = len(C)
    rel = relevance(q, C) if rel is None else rel
    G = gram(C) if G is None else G
    k = n if k is None else k
    picked, scores = [], []
    while len(picked) < k:
        v = greedy_values(rel, G, lam, picked, valid)
        p = int(np.argmax(v))                       # first maximum = lowest position
        if not np.isfinite(v[p]) or v[p] < min_score:
            break
        picked.append(p)
        scores.append(float(v[p]))
    return picked, scores
