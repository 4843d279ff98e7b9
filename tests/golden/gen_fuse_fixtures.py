"""Write the score-fusion fixtures: tiny cases whose expected outputs were worked out BY HAND from the
statement in include/super_rag_mi355x.h (sr_score_fuse), not by any implementation.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_fuse_fixtures.py

Every score is a small dyadic rational, so each intermediate below is exact in fp32 and the expected
values are exact.  The arithmetic of each case stands in the comment above it.  Output:
tests/golden/fuse_fixtures.npz (arrays "<case>.<field>"; "names" lists the cases).
"""
from __future__ import annotations

import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuse_fixtures.npz")
NI = -np.inf
MINMAX, FLOOR = 0, 1
BIG = 2 ** 32 - 2


def case(name, a, b, k_out, want, mode=MINMAX, alpha=0.5, side=None, min_score=NI, floor_a=-1.0,
         floor_b=0.0, comp=None, rrf_winner=None):
    """a / b: [(row, score), ...]; want: [(fused, row), ...] padded below to k_out;
    comp: [(a-score, b-score), ...] of the kept rows."""
    d = {
        "rows_a": np.asarray([r for r, _ in a], np.int64), "score_a": np.asarray([s for _, s in a], np.float32),
        "rows_b": np.asarray([r for r, _ in b], np.int64), "score_b": np.asarray([s for _, s in b], np.float32),
        "mode": np.int32(mode), "alpha": np.float32(alpha), "min_score": np.float32(min_score),
        "floor_a": np.float32(floor_a), "floor_b": np.float32(floor_b), "k_out": np.int32(k_out),
        "has_side": np.int32(side is not None),
        "side_a": np.asarray(side if side is not None else [], np.float32),
        "want_score": np.asarray([f for f, _ in want] + [NI] * (k_out - len(want)), np.float32),
        "want_rows": np.asarray([r for _, r in want] + [-1] * (k_out - len(want)), np.int64),
        "has_comp": np.int32(comp is not None),
        "want_a": np.asarray(([x for x, _ in comp] + [NI] * (k_out - len(comp))) if comp else [], np.float32),
        "want_b": np.asarray(([x for _, x in comp] + [NI] * (k_out - len(comp))) if comp else [], np.float32),
        "rrf_winner": np.int64(-1 if rrf_winner is None else rrf_winner),
    }
    return name, d


def cases():
    out = []
    # The case the issue opens with.  a: hi 1, lo 0 -> 10: 1, 11: .75, 12: 0.  b: hi 8, lo 0 -> 13: 1,
    # 11: .875, 14: 0.  alpha .5: 10: .5; 11: .375 + .4375 = .8125; 12: 0; 13: .5; 14: 0.
    # rrf (rank_const 1): 10: 1, 13: 1, 11: 1/2 + 1/2 = 1 -> a three-way tie, first appearance: 10.
    # Score fusion puts 11 (second in both lists) first; 10 and 13 tie at .5 and order by row.
    ab = ([(10, 1.0), (11, 0.75), (12, 0.0)], [(13, 8.0), (11, 7.0), (14, 0.0)])
    out.append(case("rrf_disagrees_both_lists_tie_by_row", *ab, 5,
                    [(0.8125, 11), (0.5, 10), (0.5, 13), (0.0, 12), (0.0, 14)], rrf_winner=10,
                    comp=[(0.75, 7.0), (1.0, NI), (NI, 8.0), (0.0, NI), (NI, 0.0)]))
    # the same with min_score .5: the two zeros go
    out.append(case("min_score_cut", *ab, 5, [(0.8125, 11), (0.5, 10), (0.5, 13)], min_score=0.5))
    # the same, k_out 1
    out.append(case("k_out_one", *ab, 1, [(0.8125, 11)]))
    # hi == lo in list a (norm 1 for both) and a one-entry list b (norm 1).  alpha .25:
    # 5: .25 1 + .75 0 = .25;  6: .25 + .75 = 1.  k_out 3 > two distinct rows.
    out.append(case("hi_equals_lo_one_entry_list_k_out_beyond", [(5, 0.5), (6, 0.5)], [(6, 3.0)], 3,
                    [(1.0, 6), (0.25, 5)], alpha=0.25))
    # list b empty (kb = 0), alpha 1: a: hi 4, lo 2 -> 3: 0, 1: 1, 2: .5
    out.append(case("empty_list_b_alpha_one", [(3, 2.0), (1, 4.0), (2, 3.0)], [], 2,
                    [(1.0, 1), (0.5, 2)], alpha=1.0))
    # both lists empty
    out.append(case("both_empty", [], [], 2, []))
    # alpha 0: only b counts.  b: hi 4, lo 2 -> 2: 1, 3: 0.  1: 0 (b unknown).  Zeros order by row.
    out.append(case("alpha_zero", [(1, 1.0), (2, 0.0)], [(2, 4.0), (3, 2.0)], 3,
                    [(1.0, 2), (0.0, 1), (0.0, 3)], alpha=0.0))
    # absent entries in the middle of a and at the head of b; their scores (99, -5) enter nothing.
    # a: {7: 1, 9: .5}: hi 1, lo .5 -> 7: 1, 9: 0.  b: {9: 2}: one entry -> 1.
    # 7: .5;  9: 0 + .5 = .5 -> a tie, by row
    out.append(case("absent_entry_in_the_middle", [(7, 1.0), (-1, 99.0), (9, 0.5)], [(-1, -5.0), (9, 2.0)], 4,
                    [(0.5, 7), (0.5, 9)], comp=[(1.0, NI), (0.5, 2.0)]))
    # FLOOR with side scores.  a: hi 1, lo -1 -> norm = (s + 1) / 2: 1: 1, 2: .5.  b: hi 4, lo 0 ->
    # 2: 1, 3: .5, 4: .25.  side: row 2 is in list a, so its side .75 is ignored; row 3: .5 -> .75
    # (above list a's minimum 0); row 4: unknown -> 0.
    # 1: .5;  2: .25 + .5 = .75;  3: .375 + .25 = .625;  4: 0 + .125 = .125
    fl = ([(1, 1.0), (2, 0.0)], [(2, 4.0), (3, 2.0), (4, 1.0)])
    out.append(case("floor_with_side", *fl, 4, [(0.75, 2), (0.625, 3), (0.5, 1), (0.125, 4)], mode=FLOOR,
                    side=[0.75, 0.5, NI], comp=[(0.0, 4.0), (0.5, 2.0), (1.0, NI), (NI, 1.0)]))
    # the same without side scores: 3: 0 + .25;  4: .125
    out.append(case("floor_without_side", *fl, 4, [(0.75, 2), (0.5, 1), (0.25, 3), (0.125, 4)], mode=FLOOR,
                    comp=[(0.0, 4.0), (1.0, NI), (NI, 2.0), (NI, 1.0)]))
    # MINMAX with side scores below and above list a's minimum.  a: hi 1, lo .5 -> 1: 1, 2: 0.
    # b: hi == lo -> 3: 1, 4: 1.  side of 3: .25 -> max(0, -.25 / .5) = 0;  of 4: .75 -> .5.
    # 1: .5;  2: 0;  3: 0 + .5 = .5;  4: .25 + .5 = .75.  Side scores leave hi and lo alone.
    out.append(case("side_below_and_above_list_minimum", [(1, 1.0), (2, 0.5)], [(3, 2.0), (4, 2.0)], 4,
                    [(0.75, 4), (0.5, 1), (0.5, 3), (0.0, 2)], side=[0.25, 0.75],
                    comp=[(0.75, 2.0), (1.0, NI), (0.25, 2.0), (0.5, NI)]))
    # the largest row id.  a: hi 1, lo 0.  b: hi == lo -> 1.  BIG: .5 + .5 = 1;  0: 0 + .5 = .5
    out.append(case("row_two_to_the_32_minus_2", [(BIG, 1.0), (0, 0.0)], [(0, 1.0), (BIG, 1.0)], 2,
                    [(1.0, BIG), (0.5, 0)]))
    # FLOOR, list a empty: hi = -inf is not above the floor, so a KNOWN side score normalises to 1.
    # b: hi 2, lo 0 -> 1: 1, 2: .5.  1: .5 + .5 = 1;  2: 0 + .25 = .25
    out.append(case("floor_empty_list_a_known_side_is_one", [], [(1, 2.0), (2, 1.0)], 2,
                    [(1.0, 1), (0.25, 2)], mode=FLOOR, side=[0.3, NI]))
    return out


def main():
    cs = cases()
    arrays = {"names": np.asarray([n for n, _ in cs])}
    for n, d in cs:
        for f, v in d.items():
            arrays[f"{n}.{f}"] = v
    np.savez(OUT, **arrays)
    print(f"wrote {len(cs)} cases to {OUT}")


if __name__ == "__main__":
    main()
