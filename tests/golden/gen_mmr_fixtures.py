"""Capture MMR fixtures from the REAL reference function (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_mmr_fixtures.py

graphiti's ``maximal_marginal_relevance`` (super_rag/graphiti/graphiti_core/search/search_utils.py:
1884-1922) and ``normalize_l2`` (graphiti_core/helpers.py:100-103) are imported from /root/reference
with the module stubbing of gen_cosine_fixtures.py.  The candidates come from the corpora already
committed in cosine_fixtures.npz, by case name and row indices, so mmr_fixtures.npz holds only
indices, lambda, min_score and the reference's output order and fp64 scores (data only;
/root/reference never travels).  The reference normalises the candidates but not the query; the
library normalises both, so the reference is called with normalize_l2(q).

Cases: families random / clustered / ties_zeros (exact duplicates and zero rows) / sparse for dims
64 / 384 / 768 / 1024, K in {1, 2, 17, 100, 128} (dim 1024 holds 64 rows: K in {1, 2, 17, 64}),
lambda cycling through {0, 0.3, 0.5, 1}, min_score through {-2, 0.1}, the zero query of every
ties_zeros corpus, and one hand-made pair of antipodal candidates (the clamp at 0), whose vectors
are stored in the fixture itself.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_cosine_fixtures import _import  # noqa: E402
from gen_rrf_fixtures import REF  # noqa: E402

SRC = os.path.join(HERE, "cosine_fixtures.npz")
OUT = os.path.join(HERE, "mmr_fixtures.npz")
FAMILIES = ("random", "clustered", "ties_zeros", "sparse")
LAMBDAS = (0.0, 0.3, 0.5, 1.0)
MIN_SCORES = (-2.0, 0.1)


def values(codes, exp):
    return codes.astype(np.float64) / 16.0 * np.exp2(exp.astype(np.float64))[:, None]


def pick_rows(fam: str, n: int, K: int, rng) -> np.ndarray:
    if fam == "ties_zeros":
        # duplicates of rows 1 and 5, the zero rows, then random others
        special = [1, 3, 7, 12, 5, 20, 21, n - 1, 2, 9, n // 2]
        if K == 1:
            return np.array([2], np.int32)               # a lone zero row
        if K == 2:
            return np.array([3, 1], np.int32)            # two exact duplicates
        rest = [r for r in rng.permutation(n).tolist() if r not in special]
        rows = (special + rest)[:K]
        return np.array(rng.permutation(rows), np.int32)
    return rng.choice(n, K, replace=False).astype(np.int32)


def main():
    sys.path.insert(0, REF)
    mmr = _import("super_rag.graphiti.graphiti_core.search.search_utils", "maximal_marginal_relevance")
    norm = _import("super_rag.graphiti.graphiti_core.helpers", "normalize_l2")
    z = np.load(SRC)
    rng = np.random.default_rng(20261019)
    out, names = {}, []
    tick = 0

    def run(name, C, q, lam, ms):
        cands = {str(i): list(c) for i, c in enumerate(C)}
        ids, scores = mmr(list(norm(list(q))), cands, lam, ms)
        out[name + ".lam"], out[name + ".min_score"] = np.float64(lam), np.float64(ms)
        out[name + ".ids"] = np.array([int(i) for i in ids], np.int32)
        out[name + ".scores"] = np.array([float(s) for s in scores], np.float64)
        names.append(name)

    for dim in (64, 384, 768, 1024):
        for fam in FAMILIES:
            src = f"{fam}_{dim}"
            C = values(z[src + ".c"], z[src + ".ce"])
            Q = values(z[src + ".q"], z[src + ".qe"])
            n = C.shape[0]
            for K in ((1, 2, 17, 100, 128) if n >= 128 else (1, 2, 17, 64)):
                lam = LAMBDAS[tick % 4]
                ms = MIN_SCORES[(tick // 4) % 2]
                qi = tick % Q.shape[0]
                if fam == "ties_zeros" and K == 17:
                    qi = Q.shape[0] - 1                      # the zero query
                tick += 1
                rows = pick_rows(fam, n, K, rng)
                name = f"{src}_k{K}"
                out[name + ".src"], out[name + ".rows"], out[name + ".qi"] = np.array(src), rows, np.int32(qi)
                run(name, C[rows], Q[qi], lam, ms)
    # hand-made: two antipodal candidates; G_01 = -1, so both maxima clamp at 0
    c = np.zeros((2, 64))
    c[0, :4] = (3.0, -1.0, 2.0, 0.5)
    c[1] = -c[0]
    q = np.zeros(64)
    q[:4] = (1.0, 0.0, 1.0, 0.0)
    for lam in (0.0, 0.5):
        name = f"antipodal_l{int(lam * 10)}"
        out[name + ".src"], out[name + ".c"], out[name + ".q"] = np.array(""), c, q
        run(name, c, q, lam, -2.0)
    out["cases"] = np.array(names)
    out["source"] = np.array("super_rag/graphiti/graphiti_core/search/search_utils.py:1884-1922 "
                             "(maximal_marginal_relevance); graphiti_core/helpers.py:100-103 "
                             "(normalize_l2)")
    np.savez_compressed(OUT, **out)
    print(f"wrote {len(names)} MMR cases to {OUT}")


if __name__ == "__main__":
    main()
