"""Time of the MMR stage next to the scan it follows (DESIGN.md "MMR").

    python tools/mmr_time.py [rows] [dim] [B] [fetch_k] [k]      (defaults 1000000 768 256 100 10)

Fills a store with clustered random rows, runs one warm-up and then `reps` profiled searches of B
queries through NativeStore.search_mmr in both modes, and prints the per-search milliseconds of
``mmr_rerank`` and ``cosine_scan`` (+ ``cosine_scan_dense``) from sr_profile_read, their ratio and
the stage's algorithmic GB/s and GFLOP/s, as one JSON line per mode.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-rag_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from super_rag_amd import _native as N  # noqa: E402
from super_rag_amd.store import NativeStore  # noqa: E402


def main():
    a = [int(x) for x in sys.argv[1:]]
    rows, dim, B, fetch_k, k = (a + [1_000_000, 768, 256, 100, 10][len(a):])[:5]
    reps = 50
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
    q = (centers[pick] + 0.7 * torch.randn((B, dim), generator=g, device=dev)).cpu().numpy()
    for mode in ("onepass", "greedy"):
        st.search_mmr(q, k, fetch_k, mode=mode)                    # warm-up (workspaces, code load)
        N.profile_enable(True)
        N.profile_read()
        for _ in range(reps):
            score, dist, r = st.search_mmr(q, k, fetch_k, mode=mode)
        stats = N.profile_read()
        N.profile_enable(False)
        mmr = stats["mmr_rerank"]
        scan_ms = sum(v["total_ms"] for n, v in stats.items() if n.startswith("cosine_scan")) / reps
        mmr_ms = mmr["total_ms"] / mmr["launches"]
        print(json.dumps({
            "mode": mode, "rows": rows, "dim": dim, "B": B, "fetch_k": fetch_k, "k": k,
            "mmr_rerank_ms": round(mmr_ms, 4), "cosine_scan_ms": round(scan_ms, 4),
            "mmr_over_scan": round(mmr_ms / scan_ms, 4),
            "mmr_GBps": round(mmr["bytes"] / mmr["launches"] / mmr_ms / 1e6, 1),
            "mmr_GFLOPps": round(mmr["flops"] / mmr["launches"] / mmr_ms / 1e6, 1),
            "kept": int((r >= 0).sum()), "finite": bool(np.isfinite(score[r >= 0]).all())}))
    st.close()


if __name__ == "__main__":
    main()
