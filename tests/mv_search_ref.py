"""Reference restatement of the multi-vector index's whole-corpus search (sr_mv_search), numpy fp64:

scores(q_list, docs, live, allow)   MaxSim of every query against every row, -inf for a row that is
                                    dead, not allowed or without tokens and for an empty query
topk(score, k, row_offset)          per query the k rows with a score above -inf ordered by (score desc,
                                    row asc) via np.lexsort((rows, -score)), -inf / -1 past them
search(...)                         the two together
The GPU tests use topk() on the DEVICE's own sr_mv_score_rows values too: the search must equal that
bit for bit."""
import numpy as np

import colbert_ref as CR


def eligible(docs, live=None, allow=None):
    ok = np.array([len(d) > 0 for d in docs], dtype=bool).reshape(-1)
    if live is not None:
        ok &= np.asarray(live).reshape(-1) != 0
    if allow is not None:
        ok &= np.asarray(allow).reshape(-1) != 0
    return ok


def scores(q_list, docs, live=None, allow=None):
    """-> fp64 [B, n_rows]."""
    ok = eligible(docs, live, allow)
    out = np.full((len(q_list), len(docs)), -np.inf, np.float64)
    for b, q in enumerate(q_list):
        if len(q) == 0:
            continue
        for r, d in enumerate(docs):
            if ok[r]:
                out[b, r] = CR.maxsim(q, d)
    return out


def topk(score, k, row_offset=0):
    """score [B, n_rows] (any float dtype, -inf = not eligible) -> (score [B, k] of the same dtype,
    rows [B, k] int64)."""
    score = np.asarray(score)
    B, n = score.shape
    out_s = np.full((B, k), -np.inf, score.dtype)
    out_r = np.full((B, k), -1, np.int64)
    rows = np.arange(n, dtype=np.int64)
    for b in range(B):
        keep = rows[~np.isneginf(score[b])]
        order = keep[np.lexsort((keep, -score[b, keep].astype(np.float64)))][:k]
        out_s[b, :order.size] = score[b, order]
        out_r[b, :order.size] = order + row_offset
    return out_s, out_r


def search(q_list, docs, k, live=None, allow=None, row_offset=0):
    return topk(scores(q_list, docs, live, allow), k, row_offset)


def search_loop(q_list, docs, k, live=None, allow=None, row_offset=0):
    """search() as plain loops (the restatement's own check)."""
    out_s, out_r = [], []
    for q in q_list:
        cand = []
        for r, d in enumerate(docs):
            if len(d) == 0 or len(q) == 0:
                continue
            if live is not None and not live[r]:
                continue
            if allow is not None and not allow[r]:
                continue
            cand.append((-CR.maxsim_loop(q, d), r))
        cand.sort()
        cand = cand[:k]
        out_s.append([-s for s, _ in cand] + [-np.inf] * (k - len(cand)))
        out_r.append([r + row_offset for _, r in cand] + [-1] * (k - len(cand)))
    return np.asarray(out_s, np.float64).reshape(len(q_list), k), np.asarray(out_r, np.int64).reshape(len(q_list), k)
