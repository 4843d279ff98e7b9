"""CPU doubles for the score-fusion tests: the doubles of tests/doubles.py with the methods score
fusion needs (search_sim, score_rows, hybrid(fusion=..., alpha=...)), fused by tests/fuse_ref.py.
Similarities are per-row dot products summed exactly (math.fsum) and rounded to fp32, so a row scores
the same whichever shard holds it (a BLAS product may sum in another order for another shape or
alignment)."""
from __future__ import annotations

import math

import numpy as np

import fuse_ref as FR
from doubles import NumpyLex, NumpyStore


class FuseStore(NumpyStore):
    def _sims(self, q):
        q = np.asarray(q, np.float64)
        if q.ndim == 1:
            q = q[None]
        unit = lambda m: np.asarray([v / max(math.sqrt(math.fsum(v * v)), 1e-300) for v in m]).reshape(m.shape)
        qn, rn = unit(q), unit(np.asarray(self.rows, np.float64))
        return np.asarray([[np.float32(math.fsum(r * v)) for r in rn] for v in qn],
                          np.float32).reshape(len(qn), len(rn))

    def search_sim(self, q, k, allow=None, mask_key=0):
        live = self.live if allow is None else (self.live & np.asarray(allow, dtype=bool))
        S = self._sims(q)
        sim = np.full((len(S), k), -np.inf, np.float32)
        rows = np.full((len(S), k), -1, np.int64)
        for b, s in enumerate(S):
            order = [i for i in np.lexsort((np.arange(len(s)), -s.astype(np.float64))) if live[i]][:k]
            sim[b, : len(order)] = s[order]
            rows[b, : len(order)] = order
        return sim, rows

    def score_rows(self, q, rows):
        S = self._sims(q)
        rows = np.asarray(rows, np.int64)
        out = np.full(rows.shape, -np.inf, np.float32)
        for b in range(rows.shape[0]):
            for j, r in enumerate(rows[b].tolist()):
                if 0 <= r < len(self.rows) and self.live[r]:
                    out[b, j] = S[b, r]
        return out


def fuse_backend(sa, ra, sb, rb, side, mode, alpha, fa, fb, ms, k, dev):
    """lexical.set_fuse_backend double: tests/fuse_ref.py in place of the kernel."""
    return FR.score_fuse(sa, ra, sb, rb, side, mode, alpha, fa, fb, ms, k)


class FuseLex(NumpyLex):
    """NumpyLex whose hybrid takes ``fusion`` / ``alpha`` (NativeLexIndex.hybrid's signature)."""

    def hybrid(self, store, queries, query_terms, k, k_each=None, rank_const=1,
               min_score=float("-inf"), allow=None, mask_key=0, fusion="rrf", alpha=0.5):
        if fusion == "rrf":
            return NumpyLex.hybrid(self, store, queries, query_terms, k, k_each, rank_const,
                                   min_score, allow, mask_key)
        k_each = k_each or k
        sims, dense = store.search_sim(queries, k_each, allow=allow, mask_key=mask_key)
        lsc, lex = self.search(query_terms, k_each, allow=allow)
        side = store.score_rows(queries, lex) if fusion == "floor" else None
        out = FR.score_fuse(sims, dense, lsc, lex, side, FR.MODES[fusion], alpha, -1.0, 0.0,
                            min_score, k)
        return out[0], out[1]
