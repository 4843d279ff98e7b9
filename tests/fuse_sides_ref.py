"""tests/fuse_ref.py's function with ``side_b`` (include/super_rag_mi355x.h, sr_score_fuse_sides): the
reference of the two-sided fusion tests, in np.float32 scalars like fuse_ref.

``side_b[i]`` is the exact mirror of ``side_a``: the b-metric score of list a's row i (-inf:
unknown), used only for a row that list b does not hold; it never enters hi_b / lo_b.  Everything
else is fuse_ref's definition, whose ``norm`` and constants are imported, not restated.
"""
from __future__ import annotations

import numpy as np

from fuse_ref import FLOOR, MINMAX, NINF, F, norm  # noqa: F401  (MINMAX / FLOOR re-exported)


def fuse_one(score_a, rows_a, score_b, rows_b, side_a=None, side_b=None, mode=MINMAX, alpha=0.5,
             floor_a=-1.0, floor_b=0.0, min_score=-np.inf, k_out=10):
    """One query.  Returns (fused [k_out] f32, rows [k_out] i64, a [k_out] f32, b [k_out] f32)."""
    score_a, score_b = np.asarray(score_a, F).reshape(-1), np.asarray(score_b, F).reshape(-1)
    rows_a = np.asarray(rows_a, np.int64).reshape(-1)
    rows_b = np.asarray(rows_b, np.int64).reshape(-1)
    sda = None if side_a is None else np.asarray(side_a, F).reshape(-1)
    sdb = None if side_b is None else np.asarray(side_b, F).reshape(-1)
    alpha = F(alpha)
    one_minus_alpha = F(F(1.0) - alpha)
    min_score = F(min_score)

    def extremes(score, rows, floor):
        hi, lo = NINF, F(np.inf)
        for s, r in zip(score, rows):
            if r >= 0:
                hi, lo = max(hi, s), min(lo, s)
        return hi, (F(floor) if mode == FLOOR else lo)

    hi_a, lo_a = extremes(score_a, rows_a, floor_a)
    hi_b, lo_b = extremes(score_b, rows_b, floor_b)

    own_a, side_of_a = {}, {}       # row -> its a score; row -> side_b of its a entry
    for i, r in enumerate(rows_a.tolist()):
        if r >= 0:
            own_a[r] = score_a[i]
            side_of_a[r] = NINF if sdb is None else sdb[i]
    own_b, side_of_b = {}, {}
    for j, r in enumerate(rows_b.tolist()):
        if r >= 0:
            own_b[r] = score_b[j]
            side_of_b[r] = NINF if sda is None else sda[j]
    items = []
    for r in sorted(set(own_a) | set(own_b)):
        xa = own_a[r] if r in own_a else side_of_b[r]
        xb = own_b[r] if r in own_b else side_of_a[r]
        na = norm(xa, hi_a, lo_a) if xa > NINF else F(0.0)
        nb = norm(xb, hi_b, lo_b) if xb > NINF else F(0.0)
        fused = F(F(alpha * na) + F(one_minus_alpha * nb))
        if not fused < min_score:
            items.append((fused, r, xa, xb))
    items.sort(key=lambda t: (-float(t[0]), t[1]))
    out_s = np.full(k_out, -np.inf, F)
    out_r = np.full(k_out, -1, np.int64)
    out_a = np.full(k_out, -np.inf, F)
    out_b = np.full(k_out, -np.inf, F)
    for i, (f, r, xa, xb) in enumerate(items[:k_out]):
        out_s[i], out_r[i], out_a[i], out_b[i] = f, r, xa, xb
    return out_s, out_r, out_a, out_b


def score_fuse(score_a, rows_a, score_b, rows_b, side_a=None, side_b=None, mode=MINMAX, alpha=0.5,
               floor_a=-1.0, floor_b=0.0, min_score=-np.inf, k_out=10):
    """fuse_one for a batch: lists [B, ka] / [B, kb].  Returns ([B, k_out] f32, i64, f32, f32)."""
    rows_a = np.asarray(rows_a, np.int64)
    rows_b = np.asarray(rows_b, np.int64)
    B = rows_a.shape[0]
    score_a = np.asarray(score_a, F).reshape(B, -1)
    score_b = np.asarray(score_b, F).reshape(B, -1)
    out = [np.empty((B, k_out), t) for t in (F, np.int64, F, F)]
    for b in range(B):
        one = fuse_one(score_a[b], rows_a[b], score_b[b], rows_b[b],
                       None if side_a is None else np.asarray(side_a, F)[b],
                       None if side_b is None else np.asarray(side_b, F)[b], mode, alpha, floor_a,
                       floor_b, min_score, k_out)
        for o, v in zip(out, one):
            o[b] = v
    return tuple(out)


def unknown_where_zero(score):
    """"floor_full"'s side_b from BM25 pair scores: exactly 0 (no shared term) -> -inf (unknown)."""
    s = np.asarray(score, F)
    return np.where(s == 0, NINF, s).astype(F)
