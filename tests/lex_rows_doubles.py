"""CPU doubles for the pair-scoring / two-sided fusion tests: tests/fuse_doubles.py's doubles with
NativeLexIndex.score_rows (scored by tests/lex_rows_ref.py) and hybrid(fusion="floor_full") (fused by
tests/fuse_sides_ref.py)."""
from __future__ import annotations

import numpy as np

import fuse_ref as FR
import fuse_sides_ref as FS
import lex_rows_ref as LR
from fuse_doubles import FuseLex


def sides_backend(sa, ra, sb, rb, side, mode, alpha, fa, fb, ms, k, dev, side_b=None):
    """lexical.set_fuse_backend double that knows the side_b keyword."""
    return FS.score_fuse(sa, ra, sb, rb, side, side_b, mode, alpha, fa, fb, ms, k)


class RowsLex(FuseLex):
    def score_rows(self, queries, rows, global_stats=None, fixed=False):
        st = None
        if global_stats is not None:
            n_live, sum_dl, gt, gdf = global_stats
            d = dict(zip(np.asarray(gt).tolist(), np.asarray(gdf).tolist()))
            st = (n_live, sum_dl, d.__getitem__)
        score, fx = LR.score_rows(self._corpus(), queries, rows, stats=st)
        return (score, fx) if fixed else score

    def hybrid(self, store, queries, query_terms, k, k_each=None, rank_const=1,
               min_score=float("-inf"), allow=None, mask_key=0, fusion="rrf", alpha=0.5):
        if fusion != "floor_full":
            return FuseLex.hybrid(self, store, queries, query_terms, k, k_each, rank_const, min_score,
                                  allow, mask_key, fusion, alpha)
        k_each = k_each or k
        sims, dense = store.search_sim(queries, k_each, allow=allow, mask_key=mask_key)
        lsc, lex = self.search(query_terms, k_each, allow=allow)
        side_a = store.score_rows(queries, lex)
        side_b = FS.unknown_where_zero(self.score_rows(query_terms, dense))
        out = FS.score_fuse(sims, dense, lsc, lex, side_a, side_b, FR.FLOOR, alpha, -1.0, 0.0,
                            min_score, k)
        return out[0], out[1]
