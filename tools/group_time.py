"""Time of grouped search next to the scan it follows and to its host alternative (DESIGN.md
"Grouped search").

    python tools/group_time.py [rows] [dim] [B] [k] [coherence %]      (defaults 1000000 768 256 10 0)

Fills a store with clustered random rows; every row belongs to a "document" of about 8 rows of its
cluster.  With coherence c > 0 a row's offset from its cluster centre is c x its document's own
direction + sqrt(1 - c^2) x noise, so the chunks of a document lie near each other (0: they are no
closer to each other than to the rest of the cluster, the worst case for group_size > 1).
For group_size 1 and 3 at the default fetch_k it prints one JSON line with
  * ``group_collapse`` and ``cosine_scan`` (+ ``cosine_scan_dense``) milliseconds per batch from
    sr_profile_read, and the continuation rounds the batch needed;
  * the wall time of the whole NativeStore.search_grouped call beside the only alternative without
    it: search_sim with k = fetch_k followed by the tests/group_ref.py walk on the host (which is
    not exact when the list runs short of k groups).
A last line gives the cost of one continuation round at B = 1: a group array of whole clusters
(about rows / 1024 rows per group) with fetch_k = 64 forces several rounds per query.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-rag_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import group_ref  # noqa: E402
from super_rag_amd import _native as N  # noqa: E402
from super_rag_amd.store import NativeStore, group_fetch_k  # noqa: E402


def wall_ms(f, reps):
    f()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    return (time.perf_counter() - t0) / reps * 1e3


def profiled(f, reps):
    f()
    N.profile_enable(True)
    N.profile_read()
    for _ in range(reps):
        f()
    stats = N.profile_read()
    N.profile_enable(False)
    return {n: dict(v, per_call_ms=v["total_ms"] / reps) for n, v in stats.items()}


def main():
    a = [int(x) for x in sys.argv[1:]]
    rows, dim, B, k, coh = (a + [1_000_000, 768, 256, 10, 0][len(a):])[:5]
    coh = coh / 100.0
    reps = 20
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    centers = torch.randn((1024, dim), generator=g, device=dev)
    st = NativeStore(dim, capacity=rows)
    cluster = np.empty(rows, np.int32)
    doc = np.empty(rows, np.int32)
    docs_per_cluster = max(1, rows // 1024 // 8)
    doc_dir = torch.randn((1024 * docs_per_cluster, dim), generator=g, device=dev) if coh > 0 else None
    for c0 in range(0, rows, 1 << 18):
        n = min(rows, c0 + (1 << 18)) - c0
        pick = torch.randint(0, 1024, (n,), generator=g, device=dev)
        d = pick * docs_per_cluster + torch.randint(0, docs_per_cluster, (n,), generator=g, device=dev)
        cluster[c0:c0 + n] = pick.cpu().numpy()
        doc[c0:c0 + n] = d.cpu().numpy()
        off = torch.randn((n, dim), generator=g, device=dev)
        if coh > 0:
            off = coh * doc_dir[d] + (1.0 - coh * coh) ** 0.5 * off
        st.add_dev((centers[pick] + 0.5 * off).contiguous())
    del doc_dir
    pick = torch.randint(0, 1024, (B,), generator=g, device=dev)
    q = (centers[pick] + 0.7 * torch.randn((B, dim), generator=g, device=dev)).cpu().numpy()

    for size in (1, 3):
        fetch_k = group_fetch_k(k, size)
        grouped = lambda: st.search_grouped(q, k, doc, group_size=size, group_key=1, sim=True)  # noqa: E731

        def host():
            sims, r = st.search_sim(q, fetch_k)
            return group_ref.grouped_search(sims, r, doc, k, size)

        stats = profiled(grouped, reps)
        scan_ms = sum(v["per_call_ms"] for n, v in stats.items() if n.startswith("cosine_scan"))
        got, want = grouped(), host()
        print(json.dumps({
            "rows": rows, "dim": dim, "B": B, "k": k, "coherence": coh, "group_size": size,
            "fetch_k": fetch_k,
            "group_collapse_ms": round(stats["group_collapse"]["per_call_ms"], 4),
            "cosine_scan_ms": round(scan_ms, 4),
            "collapse_over_scan": round(stats["group_collapse"]["per_call_ms"] / scan_ms, 5),
            "continuation_rounds_per_batch": stats.get("group_mask", {"launches": 0})["launches"] / reps,
            "search_grouped_wall_ms": round(wall_ms(grouped, reps), 3),
            "search_plus_host_walk_wall_ms": round(wall_ms(host, 3), 3),
            "search_sim_wall_ms": round(wall_ms(lambda: st.search_sim(q, fetch_k), reps), 3),
            "same_rows_as_host_walk": bool(np.array_equal(got[1], want[1]))}))

    # one continuation round at B = 1: whole clusters as groups, a short list
    q1 = q[:1]
    skew = lambda: st.search_grouped(q1, k, cluster, group_size=1, fetch_k=64, group_key=2, sim=True)  # noqa: E731
    flat = lambda: st.search_grouped(q1, k, doc, group_size=1, fetch_k=64, group_key=1, sim=True)  # noqa: E731
    stats = profiled(skew, reps)
    rounds = stats.get("group_mask", {"launches": 0})["launches"] / reps
    device_ms = sum(v["per_call_ms"] for v in stats.values())
    w_skew, w_flat = wall_ms(skew, reps), wall_ms(flat, reps)
    flat_rounds = profiled(flat, 2).get("group_mask", {"launches": 0})["launches"] / 2
    print(json.dumps({
        "rows": rows, "dim": dim, "B": 1, "k": k, "group_size": 1, "fetch_k": 64,
        "continuation_rounds": rounds, "wall_ms": round(w_skew, 3),
        "wall_ms_without_skew": round(w_flat, 3), "rounds_without_skew": flat_rounds,
        "wall_ms_per_round": round((w_skew - w_flat) / max(rounds - flat_rounds, 1), 3),
        "device_ms_per_scan": round(device_ms / (rounds + 1), 4),
        "group_mask_ms": round(stats["group_mask"]["total_ms"] / max(stats["group_mask"]["launches"], 1), 4)
        if "group_mask" in stats else None,
        "group_collapse_ms": round(stats["group_collapse"]["total_ms"] / stats["group_collapse"]["launches"], 4)}))
    st.close()


if __name__ == "__main__":
    main()
