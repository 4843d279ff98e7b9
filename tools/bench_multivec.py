"""Multi-vector (MaxSim) benchmark on one MI355X (DESIGN.md "Multi-vector retrieval"); diagnostic, not
the headline bench.py line.

    python tools/bench_multivec.py [--repeats 9] [--pool-tokens 1048576] [--skip-encoder]
                                   [--dtype fp16|fp8|both] [--out profiles/multivec_bench.json]

Part 1, sr_mv_score_rows_dev at the (B, K, dim, Lq, Ld) shapes of SHAPES: an index of pool-tokens / Ld
rows of Ld random unit tokens (so nothing is cache-resident by construction: 2 GiB at dim 1024), random
candidate rows, random unit queries.  Per shape: the time, the bytes of candidate tokens gathered (B K Ld
dim 2, once per 64-token query block) and that rate as a fraction of the library's copy yardstick
(sr_diag_copy, read + written bytes, measured in the same process); both rates come from the wall time
of whole calls, and the kernel's own rate from the profiler's events is reported next to them.
--dtype picks the index's storage (fp16, the default, or fp8: bytes per token dim instead of 2 dim); with
"both" the two indices are built over the same tokens and the same queries and candidate lists are timed on
each in the same process, per shape fp16 first (the yardstick of the comparison is that run, not an earlier
figure): the record then holds both call times with their min-max, the ratio fp16 / fp8 and the fp8 rate on
fp8 bytes against the copy yardstick, and goes to profiles/multivec_fp8_bench.json.
Part 2, the head's cost: embed_multivec_dev against embed_sparse_dev and embed_dev (mean pooling, so all
three run the full last layer) on bge-m3's shape with seeded weights (vocabulary cut to --vocab rows), at
B = 64, S = 512 and B = 2, S = 8192, with the two added kernels' own times from the profiler.
Every figure is the median of --repeats timed runs after a warm-up.  Prints one JSON line and writes it
to --out.
--compact runs part 3 alone and writes profiles/multivec_compact_bench.json: sr_mv_compact on an index of
--pool-tokens tokens at dim 1024 (rows of 256 tokens), fp16 and fp8, with every second row or a random 10 %
of the rows removed, at stage_bytes 16 / 64 / 256 MiB.  The call's wall time (it is blocking), median of
--repeats after a warm-up, each on a freshly rebuilt index; the bytes of the tokens that move, read and
written once, over that time, next to the copy yardstick counted the same way (a staged chunk moves its
bytes twice, so its ceiling is half the yardstick); and the chunks and tokens the schedule sends down each
path, from the planner's restatement in tests/mv_snapshot_ref.py.
--search runs part 4 alone and writes profiles/multivec_search_bench.json: sr_mv_search_dev (DESIGN.md
"Whole-corpus MaxSim search") on the index of part 1 (rows of 256 tokens) at dims 128 and 1024, fp16 and fp8,
Lq 32, k 100, B 1 / 32 / 256: (a) the call's wall time and the scan and selection kernels' own times from the
profiler's events, (b) the composition available without it, sr_mv_score_rows_dev over all rows in calls of
K = 1024 plus torch.topk, on the same index in the same process, (c) the copy yardstick.  The scan's bytes
are pool bytes x ceil(B / Q) per 64-token query block.
"""
import argparse
import json
import os
import sys
import time
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-rag_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from super_rag_amd import _native as N  # noqa: E402
from super_rag_amd.multivec import NativeMultiVectorIndex  # noqa: E402

# (B, K, dim, Lq, Ld)
SHAPES = [(256, 100, 1024, 32, 256), (32, 100, 1024, 32, 256), (1, 100, 1024, 32, 256),
          (256, 100, 128, 32, 256), (8, 100, 1024, 200, 2048)]


def median_ms(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def kernel_ms(fn, names, repeats):
    N.profile_enable(True)
    N.profile_read()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    prof = N.profile_read()
    N.profile_enable(False)
    return {k: (prof[k]["total_ms"] / repeats if k in prof else None) for k in names}


def copy_yardstick_gbs(nbytes, repeats):
    x = torch.empty(nbytes // 2, dtype=torch.float16, device="cuda").normal_()
    y = torch.empty_like(x)
    st = torch.cuda.current_stream().cuda_stream
    ms = median_ms(lambda: N.call_diag("sr_diag_copy", x.data_ptr(), y.data_ptr(), x.numel() * 2, 0, st),
                   repeats)[0]
    return 2.0 * x.numel() * 2 / (ms * 1e-3) / 1e9


def unit_rows(shape, gen):
    x = torch.randn(shape, dtype=torch.float32, device="cuda", generator=gen)
    return (x / x.norm(dim=-1, keepdim=True)).to(torch.float16)


KERNEL = {"fp16": "maxsim", "fp8": "maxsim_fp8"}
ELEMENT_BYTES = {"fp16": 2, "fp8": 1}


def time_shape(x, dtype, shape, q, qlen, rows, n, copy_gbs, repeats):
    """One shape on one index: the record of the single-dtype table."""
    B, K, dim, Lq, Ld = shape
    score = torch.empty((B, K), dtype=torch.float32, device="cuda")
    ms = median_ms(lambda: x.score_rows_dev(q, qlen, rows, out=score), repeats)
    name = KERNEL[dtype]
    k = kernel_ms(lambda: x.score_rows_dev(q, qlen, rows, out=score), (name,), repeats)[name]
    blocks = (Lq + 63) // 64
    nbytes = float(B) * K * Ld * dim * ELEMENT_BYTES[dtype] * blocks
    rate = lambda t_ms: nbytes / (t_ms * 1e-3) / 1e9
    return {"B": B, "K": K, "dim": dim, "Lq": Lq, "Ld": Ld, "pool_rows": n,
            "ms": round(ms[0], 4), "min_max_ms": [round(ms[1], 4), round(ms[2], 4)],
            "kernel_ms": None if k is None else round(k, 4),
            "candidate_bytes": nbytes, "query_blocks": blocks,
            # the call's wall time, as the copy yardstick is timed; the kernel's own rate apart
            "GBs": round(rate(ms[0]), 1), "fraction_of_copy": round(rate(ms[0]) / copy_gbs, 3),
            "kernel_GBs": None if k is None else round(rate(k), 1),
            "TFs": round(2.0 * B * K * Ld * Lq * dim / (ms[0] * 1e-3) / 1e12, 1),
            "finite": bool(torch.isfinite(score).all().item())}, score


def bench_maxsim(a, copy_gbs):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    dtypes = ["fp16", "fp8"] if a.dtype == "both" else [a.dtype]
    out, cache = [], {}
    for shape in SHAPES:
        B, K, dim, Lq, Ld = shape
        if (dim, Ld) not in cache:
            for xs, _ in cache.values():                      # one pool per dtype at a time
                for x in xs.values():
                    x.close()
            cache.clear()
            n = max(K, a.pool_tokens // Ld)
            xs = {d: NativeMultiVectorIndex(dim, dtype=d) for d in dtypes}
            step = max(1, (1 << 28) // (Ld * dim * 2))        # 256 MiB of fp16 tokens per add
            for i in range(0, n, step):
                m = min(step, n - i)
                toks = unit_rows((m, Ld, dim), gen)           # the same tokens into every index
                lens = torch.full((m,), Ld, dtype=torch.int32, device="cuda")
                for x in xs.values():
                    x.add_dev(toks, lens)
            cache[(dim, Ld)] = (xs, n)
        xs, n = cache[(dim, Ld)]
        q = unit_rows((B, Lq, dim), gen)
        qlen = torch.full((B,), Lq, dtype=torch.int32, device="cuda")
        rows = torch.randint(0, n, (B, K), dtype=torch.int64, device="cuda", generator=gen)
        rec, score = {}, {}
        for d in dtypes:
            rec[d], score[d] = time_shape(xs[d], d, shape, q, qlen, rows, n, copy_gbs, a.repeats)
            print("# maxsim", d, rec[d], flush=True)
        if a.dtype != "both":
            out.append(rec[a.dtype])
            continue
        r16, r8 = rec["fp16"], rec["fp8"]
        spread = max(r16["min_max_ms"][1] - r16["min_max_ms"][0], r8["min_max_ms"][1] - r8["min_max_ms"][0])
        out.append({"B": B, "K": K, "dim": dim, "Lq": Lq, "Ld": Ld, "pool_rows": n,
                    "fp16_ms": r16["ms"], "fp16_min_max_ms": r16["min_max_ms"], "fp16_kernel_ms": r16["kernel_ms"],
                    "fp8_ms": r8["ms"], "fp8_min_max_ms": r8["min_max_ms"], "fp8_kernel_ms": r8["kernel_ms"],
                    "fp16_over_fp8": round(r16["ms"] / r8["ms"], 3),
                    "kernel_fp16_over_fp8": (None if not (r16["kernel_ms"] and r8["kernel_ms"])
                                             else round(r16["kernel_ms"] / r8["kernel_ms"], 3)),
                    # fp8 slower than fp16 by more than the wider of the two recorded min-max spreads?
                    "spread_ms": round(spread, 4), "fp8_not_slower": bool(r8["ms"] <= r16["ms"] + spread),
                    "fp16_GBs": r16["GBs"], "fp16_fraction_of_copy": r16["fraction_of_copy"],
                    "fp8_candidate_bytes": r8["candidate_bytes"], "fp8_GBs": r8["GBs"],
                    "fp8_fraction_of_copy": r8["fraction_of_copy"], "fp8_kernel_GBs": r8["kernel_GBs"],
                    "fp8_TFs": r8["TFs"],
                    "max_abs_score_diff": float((score["fp16"] - score["fp8"]).abs().max().item()),
                    "finite": r16["finite"] and r8["finite"]})
        print("# maxsim both", out[-1], flush=True)
    for xs, _ in cache.values():
        for x in xs.values():
            x.close()
    return out


def bench_compact(a, copy_gbs):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mv_snapshot_ref as R
    dim, Ld = 1024, 256
    n = a.pool_tokens // Ld
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    step = min(n, (1 << 28) // (Ld * dim * 2))                # one 256 MiB block of tokens, added repeatedly
    toks = unit_rows((step, Ld, dim), gen)
    lens = torch.full((step,), Ld, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(0)
    patterns = {"every_second_row": np.arange(0, n, 2),
                "random_10_percent": np.sort(rng.choice(n, n // 10, replace=False))}
    out = []
    for dtype in ("fp16", "fp8"):
        rb = dim * ELEMENT_BYTES[dtype]
        for pname, dead in patterns.items():
            live = np.ones(n, bool)
            live[dead] = False
            src = R.sources([Ld] * n, live)
            moved = int((src != np.arange(src.size)).sum())
            for stage_mib in (16, 64, 256):
                plan = R.plan([Ld] * n, live, (stage_mib << 20) // rb, R.DIRECT_MIN_BYTES // rb)
                staged_tok = sum(t1 - t0 for t0, t1, s in plan if s)
                ts, kernel = [], None
                for it in range(a.repeats + 2):               # the first run is the warm-up, the last profiled
                    profiled = it == a.repeats + 1
                    x = NativeMultiVectorIndex(dim, dtype=dtype)
                    for i in range(0, n, step):
                        m = min(step, n - i)
                        x.add_dev(toks[:m], lens[:m])
                    x.remove(dead)
                    torch.cuda.synchronize()
                    if profiled:                              # the move kernel's own time, all launches of the call
                        N.profile_enable(True)
                        N.profile_read()
                    t = time.perf_counter()
                    x.compact(stage_mib << 20)
                    ts.append((time.perf_counter() - t) * 1e3)
                    if profiled:
                        prof = N.profile_read()
                        N.profile_enable(False)
                        kernel = prof["mv_move"]["total_ms"] if "mv_move" in prof else None
                    assert x.stats()["rows"] == int(live.sum())
                    x.close()
                ts = ts[1:-1]
                ms = float(np.median(ts))
                gbs = 2.0 * moved * rb / (ms * 1e-3) / 1e9
                out.append({"dtype": dtype, "pattern": pname, "stage_MiB": stage_mib, "rows": n, "dead_rows": int(dead.size),
                            "moved_bytes": moved * rb, "ms": round(ms, 3),
                            "min_max_ms": [round(float(np.min(ts)), 3), round(float(np.max(ts)), 3)],
                            "moved_GBs_read_plus_written": round(gbs, 1), "fraction_of_copy": round(gbs / copy_gbs, 3),
                            # the kernel alone: every launch of one call, gathers into the stage included (the
                            # stage -> pool copies are not kernels of the library and are not in it)
                            "move_kernel_ms": None if kernel is None else round(kernel, 3),
                            "move_kernel_GBs": None if not kernel else round(2.0 * moved * rb / (kernel * 1e-3) / 1e9, 1),
                            "chunks_direct": sum(1 for c in plan if not c[2]), "chunks_staged": sum(1 for c in plan if c[2]),
                            "staged_token_fraction": round(staged_tok / max(moved, 1), 3)})
                print("# compact", out[-1], flush=True)
    return out


# (dim, Lq, k) x B of the whole-corpus search table
SEARCH_SHAPES = [(128, 32, 100), (1024, 32, 100)]
SEARCH_B = [1, 32, 256]
SCAN_KERNEL = {"fp16": "maxsim_scan", "fp8": "maxsim_scan_fp8"}


def bench_search(a, copy_gbs):
    """sr_mv_search_dev against the composition the library offered before it (sr_mv_score_rows_dev over
    all rows in calls of K = 1024, then torch.topk), on the same index in the same process."""
    from super_rag_amd.multivec import search_group_queries
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    Ld, out = 256, []
    for dim, Lq, k in SEARCH_SHAPES:
        n = a.pool_tokens // Ld
        Q = search_group_queries(dim)
        xs = {d: NativeMultiVectorIndex(dim, dtype=d) for d in ("fp16", "fp8")}
        step = max(1, (1 << 28) // (Ld * dim * 2))
        for i in range(0, n, step):
            m = min(step, n - i)
            toks = unit_rows((m, Ld, dim), gen)
            lens = torch.full((m,), Ld, dtype=torch.int32, device="cuda")
            for x in xs.values():
                x.add_dev(toks, lens)
        for B in SEARCH_B:
            q = unit_rows((B, Lq, dim), gen)
            qlen = torch.full((B,), Lq, dtype=torch.int32, device="cuda")
            chunks = [torch.arange(r0, min(n, r0 + 1024), dtype=torch.int64, device="cuda").repeat(B, 1).contiguous()
                      for r0 in range(0, n, 1024)]
            for d, x in xs.items():
                res = (torch.empty((B, k), dtype=torch.float32, device="cuda"),
                       torch.empty((B, k), dtype=torch.int64, device="cuda"))

                def composed():
                    s = torch.cat([x.score_rows_dev(q, qlen, r) for r in chunks], dim=1)
                    return torch.topk(s, k, dim=1)

                ms = median_ms(lambda: x.search_dev(q, qlen, k, out=res), a.repeats)
                kn = kernel_ms(lambda: x.search_dev(q, qlen, k, out=res), (SCAN_KERNEL[d], "mv_topk"), a.repeats)
                cm = median_ms(composed, a.repeats)
                top = composed()
                same = bool((top.values == res[0]).all().item())
                blocks = (Lq + 63) // 64
                groups = (B + Q - 1) // Q
                nbytes = float(x.nbytes) * groups * blocks
                scan = kn[SCAN_KERNEL[d]]
                out.append({"dtype": d, "dim": dim, "B": B, "Lq": Lq, "k": k, "rows": n, "Ld": Ld, "Q": Q,
                            "search_ms": round(ms[0], 4), "search_min_max_ms": [round(ms[1], 4), round(ms[2], 4)],
                            "scan_kernel_ms": None if scan is None else round(scan, 4),
                            "topk_kernel_ms": None if kn["mv_topk"] is None else round(kn["mv_topk"], 4),
                            "composed_ms": round(cm[0], 4), "composed_min_max_ms": [round(cm[1], 4), round(cm[2], 4)],
                            "search_over_composed": round(ms[0] / cm[0], 3),
                            "scan_bytes": nbytes, "pool_bytes": x.nbytes, "query_groups": groups,
                            "scan_GBs": round(nbytes / (ms[0] * 1e-3) / 1e9, 1),
                            "scan_fraction_of_copy": round(nbytes / (ms[0] * 1e-3) / 1e9 / copy_gbs, 3),
                            "scan_kernel_GBs": None if not scan else round(nbytes / (scan * 1e-3) / 1e9, 1),
                            "scores_equal_composed": same})
                print("# search", out[-1], flush=True)
        for x in xs.values():
            x.close()
    return out


def bench_forward(a):
    from super_rag_amd.encoder import MODELS, Encoder, random_weights
    spec = replace(MODELS["bge-m3"], vocab_size=a.vocab)
    enc = Encoder(spec, weights=random_weights(spec, 0, "hf"), max_tokens=a.max_tokens)
    rng = np.random.default_rng(1)
    enc.set_sparse_head(rng.standard_normal(spec.hidden).astype(np.float32) / 32.0, [0.0])
    enc.set_colbert_head(rng.standard_normal((1024, spec.hidden)).astype(np.float32) / 32.0,
                         0.1 * rng.standard_normal(1024).astype(np.float32))
    out = {"model": "bge-m3 shape, seeded weights, dc 1024", "vocab": a.vocab, "max_tokens": a.max_tokens}
    for B, S in ((64, 512), (2, 8192)):
        ids = torch.as_tensor(rng.integers(5, a.vocab, (B, S)).astype(np.int32)).cuda()
        ids[:, 0] = spec.bos_id
        mask = torch.ones_like(ids)
        plain = median_ms(lambda: enc.embed_dev(ids, mask, pool="mean"), a.repeats)
        sparse = median_ms(lambda: enc.embed_sparse_dev(ids, mask, pool="mean"), a.repeats)
        multi = median_ms(lambda: enc.embed_multivec_dev(ids, mask, pool="mean"), a.repeats)
        all3 = median_ms(lambda: enc.embed_multivec_dev(ids, mask, pool="mean", with_sparse=True), a.repeats)
        k = kernel_ms(lambda: enc.embed_multivec_dev(ids, mask, pool="mean"), ("gemm_f16_bias", "colbert_pack"),
                      a.repeats)
        out[f"B{B}_S{S}"] = {"forward_mean_ms": round(plain[0], 3), "forward_sparse_mean_ms": round(sparse[0], 3),
                             "forward_multivec_mean_ms": round(multi[0], 3),
                             "forward_multivec_sparse_mean_ms": round(all3[0], 3),
                             "min_max_ms": {"mean": [round(plain[1], 3), round(plain[2], 3)],
                                            "sparse": [round(sparse[1], 3), round(sparse[2], 3)],
                                            "multivec": [round(multi[1], 3), round(multi[2], 3)]},
                             "colbert_pack_ms": k["colbert_pack"], "bias_gemms_ms_all_layers": k["gemm_f16_bias"]}
        print("# forward", B, S, out[f"B{B}_S{S}"], flush=True)
    enc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--pool-tokens", type=int, default=1 << 20)
    ap.add_argument("--vocab", type=int, default=32000, help="encoder vocabulary rows (bge-m3: 250002)")
    ap.add_argument("--max-tokens", type=int, default=32768)
    ap.add_argument("--skip-encoder", action="store_true")
    ap.add_argument("--dtype", choices=("fp16", "fp8", "both"), default="fp16",
                    help="token storage of the index; both: fp16 and fp8 over the same tokens, compared")
    ap.add_argument("--compact", action="store_true",
                    help="part 3 alone: sr_mv_compact, to profiles/multivec_compact_bench.json")
    ap.add_argument("--search", action="store_true",
                    help="part 4 alone: sr_mv_search_dev against score_rows_dev + topk, to "
                         "profiles/multivec_search_bench.json")
    ap.add_argument("--out", default=None,
                    help="default profiles/multivec_bench.json, profiles/multivec_fp8_bench.json with --dtype both")
    a = ap.parse_args()
    if a.out is None and a.compact:
        a.out = os.path.join(ROOT, "profiles", "multivec_compact_bench.json")
    if a.out is None and a.search:
        a.out = os.path.join(ROOT, "profiles", "multivec_search_bench.json")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "multivec_fp8_bench.json" if a.dtype == "both" else "multivec_bench.json")
    os.environ.setdefault("SUPER_RAG_AMD_SYNTHETIC", "1")
    N.require_gpu()
    copy_gbs = copy_yardstick_gbs(1 << 28, a.repeats)
    rec = {"metric": "sr_mv_score_rows_dev against the copy yardstick; multi-vector forward vs sparse / plain",
           "repeats": a.repeats, "statistic": "median of repeats after one warm-up call",
           "copy_yardstick_GBs": round(copy_gbs, 1), "pool_tokens": a.pool_tokens, "dtype": a.dtype}
    if a.compact:
        rec["metric"] = "sr_mv_compact call time and moved bytes per second against the copy yardstick"
        rec["statistic"] = "median of repeats after one warm-up, each on a freshly rebuilt index"
        rec["compact"] = bench_compact(a, copy_gbs)
    elif a.search:
        rec["metric"] = ("sr_mv_search_dev (whole-corpus MaxSim top-k) against sr_mv_score_rows_dev over all rows + "
                         "torch.topk, and its pool bytes per second against the copy yardstick")
        rec["dtype"] = "both"
        rec["search"] = bench_search(a, copy_gbs)
    else:
        rec["maxsim"] = bench_maxsim(a, copy_gbs)
        if not a.skip_encoder:
            rec["forward"] = bench_forward(a)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
