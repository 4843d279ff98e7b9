"""Plain numpy restatement of score fusion (include/super_rag_mi355x.h, sr_score_fuse), in np.float32
scalars so that every operation rounds once, as the kernel's do: the reference of every score-fusion
test (tests helper, the role of tests/group_ref.py).

Per query two scored lists a and b.  An entry with row < 0 is absent wherever it stands; a row
appears at most once per list; no order is assumed.  ``side_a[j]``: the a-metric score of b's row j
(-inf: unknown), used only for a row that list a does not hold.
  hi      = max of the list's own present scores (-inf for an empty list)
  lo      = MINMAX: min of them (+inf for an empty list); FLOOR: floor_a / floor_b
  norm(s) = hi > lo ? max(0, (s - lo) / (hi - lo)) : 1 for a known score, 0 for an unknown one
  fused   = (alpha * norm_a) + (one_minus_alpha * norm_b), one_minus_alpha = float32(1) - alpha
Output: the first k_out distinct rows by (fused desc, row asc), rows with fused < min_score dropped,
-inf / -1 in unfilled slots; out_a / out_b: the a- and b-score used for each kept row (-inf: unknown).
"""
from __future__ import annotations

import numpy as np

MINMAX = 0
FLOOR = 1
MODES = {"relative": MINMAX, "floor": FLOOR}

F = np.float32
NINF = F(-np.inf)


def norm(s, hi, lo):
    """Normalised score of a KNOWN score s."""
    if hi > lo:
        return max(F(0.0), F(F(s - lo) / F(hi - lo)))
    return F(1.0)


def fuse_one(score_a, rows_a, score_b, rows_b, side_a=None, mode=MINMAX, alpha=0.5, floor_a=-1.0,
             floor_b=0.0, min_score=-np.inf, k_out=10):
    """One query.  Returns (fused [k_out] f32, rows [k_out] i64, a [k_out] f32, b [k_out] f32)."""
    score_a, score_b = np.asarray(score_a, F).reshape(-1), np.asarray(score_b, F).reshape(-1)
    rows_a = np.asarray(rows_a, np.int64).reshape(-1)
    rows_b = np.asarray(rows_b, np.int64).reshape(-1)
    side = None if side_a is None else np.asarray(side_a, F).reshape(-1)
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

    sa = {int(r): s for s, r in zip(score_a, rows_a) if r >= 0}
    sb, sd = {}, {}
    for j, r in enumerate(rows_b.tolist()):
        if r >= 0:
            sb[r] = score_b[j]
            sd[r] = NINF if side is None else side[j]
    items = []
    for r in sorted(set(sa) | set(sb)):
        xa = sa[r] if r in sa else sd[r]
        xb = sb.get(r, NINF)
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


def score_fuse(score_a, rows_a, score_b, rows_b, side_a=None, mode=MINMAX, alpha=0.5, floor_a=-1.0,
               floor_b=0.0, min_score=-np.inf, k_out=10):
    """fuse_one for a batch: lists [B, ka] / [B, kb].  Returns ([B, k_out] f32, i64, f32, f32)."""
    rows_a = np.asarray(rows_a, np.int64)
    rows_b = np.asarray(rows_b, np.int64)
    B = rows_a.shape[0]
    score_a = np.asarray(score_a, F).reshape(B, -1)
    score_b = np.asarray(score_b, F).reshape(B, -1)
    out = [np.empty((B, k_out), t) for t in (F, np.int64, F, F)]
    for b in range(B):
        one = fuse_one(score_a[b], rows_a[b], score_b[b], rows_b[b],
                       None if side_a is None else np.asarray(side_a, F)[b], mode, alpha, floor_a,
                       floor_b, min_score, k_out)
        for o, v in zip(out, one):
            o[b] = v
    return tuple(out)


def rrf_winner(rows_a, rows_b, rank_const=1):
    """The row reciprocal-rank fusion puts first (ranked lists, -1 padded): for the hand case in
    which rrf and score fusion disagree."""
    score, first = {}, {}
    for lst in (rows_a, rows_b):
        for i, r in enumerate(int(x) for x in lst if x >= 0):
            score[r] = score.get(r, 0.0) + 1.0 / (i + rank_const)
            first.setdefault(r, len(first))
    return min(score, key=lambda r: (-score[r], first[r]))
