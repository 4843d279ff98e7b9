"""Device time of score fusion next to rank fusion, and of score_rows (DESIGN.md "Score fusion").

    python tools/fuse_time.py [rows] [dim] [B]                      (defaults 1000000 768 256)

Fills a store with clustered random rows and, for k_each = 100 and 1024, builds per query
  * list a: the dense top-k_each of the store (search_dev), and
  * list b: k_each rows, half of them drawn from list a and half from the rest of the store, with
    descending random scores (a stand-in for a BM25 list: the fusion kernels read only rows and
    scores),
then prints one JSON line with the milliseconds per batch, from sr_profile_read's device events, of
``score_fuse`` in both modes (floor mode with the side scores score_rows produced) beside ``rrf_fuse``
on the same two row lists (k_out = k_each), and of ``score_rows`` over list b's rows (B x k_each
pairs).  rrf_fuse is the yardstick printed beside them, not a like-for-like rival: it compares every
pair of entries (O(n^2)) and reads no scores.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-rag_amd")]

import torch  # noqa: E402

from super_rag_amd import _native as N  # noqa: E402
from super_rag_amd.lexical import rrf_fuse_dev, score_fuse_dev  # noqa: E402
from super_rag_amd.store import NativeStore  # noqa: E402


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
    rows, dim, B = (a + [1_000_000, 768, 256][len(a):])[:3]
    reps = 20
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

    for k_each in (100, 1024):
        sims, ra = st.search_dev(q, k_each)
        half = k_each // 2
        # list b: half of list a's rows (a random half, per query) + rows of the store outside list a
        take = torch.argsort(torch.rand((B, k_each), generator=g, device=dev), dim=1)[:, :half]
        shared = torch.gather(ra, 1, take)
        fresh = torch.empty((B, k_each - half), dtype=torch.int64, device=dev)
        for b in range(B):       # distinct rows outside list a (rejection on a sorted sample)
            cand = torch.unique(torch.randint(0, rows, (4 * k_each,), generator=g, device=dev))
            cand = cand[~torch.isin(cand, ra[b])]
            fresh[b] = cand[torch.randperm(cand.numel(), generator=g, device=dev)[: k_each - half]]
        rb = torch.cat([shared, fresh], 1)
        rb = torch.gather(rb, 1, torch.argsort(torch.rand((B, k_each), generator=g, device=dev), dim=1)).contiguous()
        sb = torch.sort(20.0 * torch.rand((B, k_each), generator=g, device=dev), dim=1, descending=True)[0].contiguous()
        side = st.score_rows_dev(q, rb)
        torch.cuda.synchronize()

        t_rrf = profiled(lambda: rrf_fuse_dev(ra, rb, k_each), reps)["rrf_fuse"]
        t_rel = profiled(lambda: score_fuse_dev(sims, ra, sb, rb, k_each, "relative"), reps)["score_fuse"]
        t_flo = profiled(lambda: score_fuse_dev(sims, ra, sb, rb, k_each, "floor", side_a=side), reps)["score_fuse"]
        t_rows = profiled(lambda: st.score_rows_dev(q, rb), reps)["score_rows"]
        fused = score_fuse_dev(sims, ra, sb, rb, k_each, "floor", side_a=side)
        torch.cuda.synchronize()
        print(json.dumps({
            "rows": rows, "dim": dim, "B": B, "k_each": k_each, "k_out": k_each,
            "distinct_rows_per_query": 2 * k_each - half,
            "score_fuse_relative_ms": round(t_rel, 4), "score_fuse_floor_ms": round(t_flo, 4),
            "rrf_fuse_ms": round(t_rrf, 4), "score_rows_ms": round(t_rows, 4),
            "score_rows_pairs": B * k_each,
            "score_rows_GBps": round(B * k_each * st_ld(dim) * 2 / (t_rows * 1e-3) / 1e9, 1),
            "kept_rows": int((fused[1] >= 0).sum().item())}))
    st.close()


def st_ld(dim):
    return (dim + 63) // 64 * 64


if __name__ == "__main__":
    main()
