"""Device time of lex_score_rows, the exact BM25 of given (query, row) pairs (DESIGN.md "Exact BM25 row
scoring").

    python tools/lex_rows_time.py [rows] [postings_per_row] [B] [K] [dim]   (defaults 1000000 100 256 100 768)

Builds a lexical index of ``rows`` documents of about ``postings_per_row`` distinct terms each (60 % ..
140 % of it, over a vocabulary of 32,771 terms) and a store of as many clustered random rows, takes B
queries of 6 terms and, as the pairs, each query's dense top-K rows (the rows "floor_full" fusion
completes), then prints one JSON line with the milliseconds per batch from sr_profile_read's device
events of ``lex_score_rows`` over the B x K pairs.  Beside it, as yardsticks and not rivals: ``lex_score``
+ ``lex_select`` of the same query batch (a whole BM25 top-K search) and ``score_rows`` (the cosine
twin) over the same pairs.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-rag_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from super_rag_amd import _native as N  # noqa: E402
from super_rag_amd.lexical import NativeLexIndex, query_arrays  # noqa: E402
from super_rag_amd.store import NativeStore  # noqa: E402

VOCAB = 32771        # prime: base + j * step (mod VOCAB) are distinct terms for j < VOCAB


def profiled(f, reps):
    f()
    torch.cuda.synchronize()
    N.profile_enable(True)
    N.profile_read()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    stats = N.profile_read()
    N.profile_enable(False)
    return {n: v["total_ms"] / reps for n, v in stats.items()}


def main():
    a = [int(x) for x in sys.argv[1:]]
    rows, per_row, B, K, dim = (a + [1_000_000, 100, 256, 100, 768][len(a):])[:5]
    reps = 20
    rng = np.random.default_rng(0)
    lex = NativeLexIndex()
    postings = 0
    for c0 in range(0, rows, 100_000):
        n = min(rows, c0 + 100_000) - c0
        L = rng.integers(max(1, per_row * 6 // 10), per_row * 14 // 10 + 1, n)
        off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
        row = np.repeat(np.arange(n), L)
        j = np.arange(off[-1]) - off[row]
        base, step = rng.integers(0, VOCAB, n), rng.integers(1, VOCAB, n)
        terms = ((base[row] + j * step[row]) % VOCAB).astype(np.int32)
        tf = rng.integers(1, 4, off[-1]).astype(np.int32)
        dl = (np.add.reduceat(tf, off[:-1]) + rng.integers(0, 20, n)).astype(np.int32)
        lex.add_arrays(off, terms, tf, dl)
        postings += int(off[-1])

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    centers = torch.randn((1024, dim), generator=g, device=dev)
    st = NativeStore(dim, capacity=rows)
    for c0 in range(0, rows, 1 << 18):
        n = min(rows, c0 + (1 << 18)) - c0
        pick = torch.randint(0, 1024, (n,), generator=g, device=dev)
        st.add_dev((centers[pick] + 0.5 * torch.randn((n, dim), generator=g, device=dev)).contiguous())
    pick = torch.randint(0, 1024, (B,), generator=g, device=dev)
    q = (centers[pick] + 0.7 * torch.randn((B, dim), generator=g, device=dev)).contiguous()
    _, pairs = st.search_dev(q, K)
    pairs = pairs.contiguous()
    queries = [rng.integers(0, VOCAB, 6).tolist() for _ in range(B)]
    qoff, qterms = query_arrays(queries)
    torch.cuda.synchronize()

    t_rows = profiled(lambda: lex.score_rows_dev(qoff, qterms, pairs), reps)["lex_score_rows"]
    t_search = profiled(lambda: lex.search_dev(qoff, qterms, K), reps)
    t_cos = profiled(lambda: st.score_rows_dev(q, pairs), reps)["score_rows"]
    score, fixed = lex.score_rows_dev(qoff, qterms, pairs, fixed=True)
    torch.cuda.synchronize()
    per_pair = postings / rows * 12.0 + 37.0
    print(json.dumps({
        "rows": rows, "postings": postings, "postings_per_row": round(postings / rows, 1), "B": B, "K": K,
        "pairs": B * K, "terms_per_query": 6,
        "lex_score_rows_ms": round(t_rows, 4),
        "lex_score_rows_GBps": round(B * K * per_pair / (t_rows * 1e-3) / 1e9, 1),
        "lex_score_ms": round(t_search["lex_score"], 4), "lex_select_ms": round(t_search["lex_select"], 4),
        "score_rows_ms": round(t_cos, 4), "dim": dim,
        "matching_pairs": int((fixed != 0).sum().item())}))
    st.close()
    lex.close()


if __name__ == "__main__":
    main()
