"""Time of the batched subset search next to the masked search it replaces (DESIGN.md "Subset
search").

    python tools/subset_time.py [rows] [dim] [B] [k]      (defaults 1000000 768 256 10)

Fills a store with clustered random rows.  For L in {256, 4096, 65536} every one of the B queries
gets its own random ascending list of L rows; after one warm-up, `reps` profiled
NativeStore.search_subset calls give the per-launch milliseconds of ``subset_scan`` and
``topk_select`` from sr_profile_read, the gather rate (rows x row bytes / subset_scan time) and the
wall time of the whole call (list upload included).  Next to them: the wall time of one B = 1
search_subset with one such list, and of one B = 1 masked search (a fresh mask every call: what one
distinct filter costs on the mask path) with its scan + select kernel time.  One JSON line per L.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-rag_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from super_rag_amd import _native as N  # noqa: E402
from super_rag_amd.store import NativeStore  # noqa: E402


def _wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    a = [int(x) for x in sys.argv[1:]]
    rows, dim, B, k = (a + [1_000_000, 768, 256, 10][len(a):])[:4]
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
    rng = np.random.default_rng(0)
    ld = (dim + 63) // 64 * 64
    for L in (256, 4096, 65536):
        L = min(L, rows)
        # ascending, distinct, spread over the whole store: one random row per stride of rows / L
        base = (np.arange(L, dtype=np.int64) * rows) // L
        lists = [base + rng.integers(0, max(rows // L, 1), L) for _ in range(B)]
        reps = 20 if L <= 4096 else 5
        st.search_subset(q, k, lists)                              # warm-up (workspaces, code load)
        N.profile_enable(True)
        N.profile_read()
        t0 = time.perf_counter()
        for _ in range(reps):
            d, r = st.search_subset(q, k, lists)
        call_ms = (time.perf_counter() - t0) / reps * 1e3
        stats = N.profile_read()
        N.profile_enable(False)
        scan, sel = stats["subset_scan"], stats["topk_select"]
        scan_ms = scan["total_ms"] / reps                          # (several passes count as one)
        sel_ms = sel["total_ms"] / reps
        mask = np.zeros(rows, np.uint8)
        mask[lists[0]] = 1
        masked_ms = _wall(lambda: st.search(q[:1], k, allow=mask, mask_key=0), 5)
        N.profile_enable(True)
        N.profile_read()
        st.search(q[:1], k, allow=mask, mask_key=0)
        ms = N.profile_read()
        N.profile_enable(False)
        masked_dev_ms = sum(v["total_ms"] for n, v in ms.items()
                            if n.startswith("cosine_scan") or n == "topk_select")
        subset1_ms = _wall(lambda: st.search_subset(q[:1], k, lists[:1]), 5)
        print(json.dumps({
            "L": L, "rows": rows, "dim": dim, "B": B, "k": k,
            "subset_scan_ms": round(scan_ms, 4), "topk_select_ms": round(sel_ms, 4),
            "scan_launches_per_call": scan["launches"] // reps,
            "gather_GBps": round(B * L * ld * 2.0 / scan_ms / 1e6, 1),
            "subset_call_ms": round(call_ms, 3),
            "masked_b1_ms": round(masked_ms, 3), "masked_b1_kernels_ms": round(masked_dev_ms, 4),
            "masked_x_B_ms": round(B * masked_ms, 1),
            "subset_b1_ms": round(subset1_ms, 3),
            "kept": int((r >= 0).sum()), "finite": bool(np.isfinite(d[r >= 0]).all())}), flush=True)
    st.close()


if __name__ == "__main__":
    main()
