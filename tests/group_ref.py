"""Plain numpy restatement of grouped search (include/super_rag_mi355x.h, sr_store_search_grouped):
the walk every grouped-search test compares against (tests helper, the role of tests/mmr_ref.py).

Walk all eligible rows in the store's order (similarity desc, row asc).  A row is kept when
  * its group already has fewer than ``group_size`` kept rows, and
  * its group is already a kept group, or fewer than ``k`` groups are kept.
Group id ``g >= 0`` names a group, ``-1`` makes the row a group of its own.  Groups come in order of
first appearance, the rows of a group in walk order; unfilled slots hold row -1 / similarity -inf,
an unfilled group slot reports group -1.
"""
from __future__ import annotations

import numpy as np


def ranking(sims, rows):
    """(sims, rows) of the valid entries (row >= 0) in the store's order: sim desc, row asc."""
    sims = np.asarray(sims).reshape(-1)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    ok = rows >= 0
    sims, rows = sims[ok], rows[ok]
    o = np.lexsort((rows, -sims.astype(np.float64)))
    return sims[o], rows[o]


def group_walk(sims, rows, group, k, group_size=1):
    """The walk over a COMPLETE ranking (``sims`` / ``rows`` already in walk order, every row >= 0).
    Returns (sim [k, group_size] float64, rows [k, group_size] int64, groups [k] int32)."""
    group = np.asarray(group)
    out_s = np.full((k, group_size), -np.inf, dtype=np.float64)
    out_r = np.full((k, group_size), -1, dtype=np.int64)
    out_g = np.full(k, -1, dtype=np.int32)
    slot = {}          # group key -> (ordinal, kept rows so far)
    for s, r in zip(np.asarray(sims).tolist(), np.asarray(rows).tolist()):
        g = int(group[r])
        if g < -1:
            raise ValueError(f"group id {g} of row {r}: ids are >= -1")
        key = ("row", r) if g == -1 else g
        hit = slot.get(key)
        if hit is None:
            if len(slot) >= k:
                continue
            hit = slot[key] = [len(slot), 0]
            out_g[hit[0]] = g
        if hit[1] >= group_size:
            continue
        out_s[hit[0], hit[1]] = s
        out_r[hit[0], hit[1]] = r
        hit[1] += 1
    return out_s, out_r, out_g


def grouped_search(sims, rows, group, k, group_size=1):
    """group_walk for a batch: ``sims`` / ``rows`` [B, n] complete rankings as search_sim returns them
    (-1 rows past the eligible ones, in any order).  Returns ([B, k, g], [B, k, g], [B, k])."""
    sims, rows = np.asarray(sims), np.asarray(rows)
    B = sims.shape[0]
    out_s = np.full((B, k, group_size), -np.inf, dtype=np.float64)
    out_r = np.full((B, k, group_size), -1, dtype=np.int64)
    out_g = np.full((B, k), -1, dtype=np.int32)
    for b in range(B):
        s, r = ranking(sims[b], rows[b])
        out_s[b], out_r[b], out_g[b] = group_walk(s, r, group, k, group_size)
    return out_s, out_r, out_g
