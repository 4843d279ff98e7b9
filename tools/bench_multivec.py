"""Multi-vector (MaxSim) benchmark on one MI355X (DESIGN.md "Multi-vector retrieval"); diagnostic, not
the headline bench.py line.

    python tools/bench_multivec.py [--repeats 9] [--pool-tokens 1048576] [--skip-encoder]
                                   [--out profiles/multivec_bench.json]

Part 1, sr_mv_score_rows_dev at the (B, K, dim, Lq, Ld) shapes of SHAPES: an index of pool-tokens / Ld
rows of Ld random unit tokens (so nothing is cache-resident by construction: 2 GiB at dim 1024), random
candidate rows, random unit queries.  Per shape: the time, the bytes of candidate tokens gathered (B K Ld
dim 2, once per 64-token query block) and that rate as a fraction of the library's copy yardstick
(sr_diag_copy, read + written bytes, measured in the same process); both rates come from the wall time
of whole calls, and the kernel's own rate from the profiler's events is reported next to them.
Part 2, the head's cost: embed_multivec_dev against embed_sparse_dev and embed_dev (mean pooling, so all
three run the full last layer) on bge-m3's shape with seeded weights (vocabulary cut to --vocab rows), at
B = 64, S = 512 and B = 2, S = 8192, with the two added kernels' own times from the profiler.
Every figure is the median of --repeats timed runs after a warm-up.  Prints one JSON line and writes it
to --out.
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


def bench_maxsim(a, copy_gbs):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    out, cache = [], {}
    for B, K, dim, Lq, Ld in SHAPES:
        if (dim, Ld) not in cache:
            cache.clear()                                     # one pool at a time
            n = max(K, a.pool_tokens // Ld)
            x = NativeMultiVectorIndex(dim)
            step = max(1, (1 << 28) // (Ld * dim * 2))        # 256 MiB of tokens per add
            for i in range(0, n, step):
                m = min(step, n - i)
                x.add_dev(unit_rows((m, Ld, dim), gen), torch.full((m,), Ld, dtype=torch.int32, device="cuda"))
            cache[(dim, Ld)] = (x, n)
        x, n = cache[(dim, Ld)]
        q = unit_rows((B, Lq, dim), gen)
        qlen = torch.full((B,), Lq, dtype=torch.int32, device="cuda")
        rows = torch.randint(0, n, (B, K), dtype=torch.int64, device="cuda", generator=gen)
        score = torch.empty((B, K), dtype=torch.float32, device="cuda")
        ms = median_ms(lambda: x.score_rows_dev(q, qlen, rows, out=score), a.repeats)
        k = kernel_ms(lambda: x.score_rows_dev(q, qlen, rows, out=score), ("maxsim",), a.repeats)
        blocks = (Lq + 63) // 64
        nbytes = float(B) * K * Ld * dim * 2 * blocks
        rate = lambda t_ms: nbytes / (t_ms * 1e-3) / 1e9
        out.append({"B": B, "K": K, "dim": dim, "Lq": Lq, "Ld": Ld, "pool_rows": n,
                    "ms": round(ms[0], 4), "min_max_ms": [round(ms[1], 4), round(ms[2], 4)],
                    "kernel_ms": None if k["maxsim"] is None else round(k["maxsim"], 4),
                    "candidate_bytes": nbytes, "query_blocks": blocks,
                    # the call's wall time, as the copy yardstick is timed; the kernel's own rate apart
                    "GBs": round(rate(ms[0]), 1), "fraction_of_copy": round(rate(ms[0]) / copy_gbs, 3),
                    "kernel_GBs": None if k["maxsim"] is None else round(rate(k["maxsim"]), 1),
                    "TFs": round(2.0 * B * K * Ld * Lq * dim / (ms[0] * 1e-3) / 1e12, 1),
                    "finite": bool(torch.isfinite(score).all().item())})
        print("# maxsim", out[-1], flush=True)
    for x, _ in cache.values():
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multivec_bench.json"))
    a = ap.parse_args()
    os.environ.setdefault("SUPER_RAG_AMD_SYNTHETIC", "1")
    N.require_gpu()
    copy_gbs = copy_yardstick_gbs(1 << 28, a.repeats)
    rec = {"metric": "sr_mv_score_rows_dev against the copy yardstick; multi-vector forward vs sparse / plain",
           "repeats": a.repeats, "statistic": "median of repeats after one warm-up call",
           "copy_yardstick_GBs": round(copy_gbs, 1), "pool_tokens": a.pool_tokens}
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
