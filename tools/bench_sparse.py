"""Learned-sparse retrieval benchmark on one MI355X (DESIGN.md "Learned-sparse retrieval");
diagnostic, not the headline bench.py line.

    python tools/bench_sparse.py [--docs 1000000] [--k 100] [--repeats 9] [--skip-encoder]

Part 1, impact search against BM25 on the SAME postings: a seeded Zipf corpus (tools/bench_lexical.py's
law) indexed twice, once with tf (NativeLexIndex) and once with the weight log2(1 + tf) in tf's place
(NativeImpactIndex); the same queries (the impact side with seeded weights); B = 32 and 256, k = 100.
Part 2, the sparse forward against the plain forward: bge-m3's shape (24 layers, d = 1024; the
vocabulary cut to --vocab rows, which no kernel's time depends on) with seeded weights, at S = 512,
B = 64 and S = 8192, B = 2: embed_sparse_dev against embed_dev with mean pooling (both run the full last
layer: the difference is the head and the collapse) and against CLS pooling (the cost of giving up the
CLS-only last layer), the two new kernels' own times from the profiler, and sparse_token_weights'
rate against the library's copy yardstick (sr_diag_copy, read + written bytes).
Every figure is the median of --repeats timed runs after a warm-up.  Prints one JSON line.
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
from super_rag_amd.lexical import NativeImpactIndex, NativeLexIndex  # noqa: E402


def gen_docs(n, vocab, mean_len, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(mean_len // 2, mean_len * 3 // 2 + 1, n).astype(np.int64)
    t = (rng.zipf(1.2, int(lens.sum())) - 1) % vocab
    doc = np.repeat(np.arange(n, dtype=np.int64), lens)
    key, cnt = np.unique(doc * vocab + t, return_counts=True)
    off = np.concatenate([[0], np.cumsum(np.bincount(key // vocab, minlength=n))]).astype(np.int64)
    return off, (key % vocab).astype(np.int32), cnt.astype(np.int32), lens.astype(np.int32)


def gen_queries(B, vocab, seed):
    rng = np.random.default_rng(seed)
    return [(((rng.zipf(1.2, rng.integers(4, 9)) - 1) % (vocab - 100)) + 100).tolist() for _ in range(B)]


def median_ms(fn, repeats, sync=None):
    fn()
    ts = []
    for _ in range(repeats):
        if sync:
            sync()
        t = time.perf_counter()
        fn()
        if sync:
            sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def kernel_ms(fn, names, repeats):
    """Per-call time of the named profiler scopes over ``repeats`` calls of fn."""
    N.profile_enable(True)
    N.profile_read()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    prof = N.profile_read()
    N.profile_enable(False)
    return {k: (prof[k]["total_ms"] / repeats if k in prof else None) for k in names}, prof


def bench_impact(a):
    off, terms, tf, dl = gen_docs(a.docs, a.lex_vocab, a.mean_len, 0)
    lex, imp = NativeLexIndex(), NativeImpactIndex()
    lex.add_arrays(off, terms, tf, dl)
    imp.add_arrays(off, terms, np.log2(1.0 + tf).astype(np.float32))
    df = np.bincount(terms, minlength=a.lex_vocab)
    out = {"docs": a.docs, "postings": int(len(terms)), "k": a.k}
    for B in (32, 256):
        qs = gen_queries(B, a.lex_vocab, 2)
        rng = np.random.default_rng(3)
        qw = [(np.unique(q), np.exp(rng.normal(0, 0.5, len(np.unique(q)))).astype(np.float32)) for q in qs]
        scored = int(sum(df[np.unique(q)].sum() for q in qs))
        bm = median_ms(lambda: lex.search(qs, a.k), a.repeats)
        im = median_ms(lambda: imp.search(qw, a.k), a.repeats)
        kb, _ = kernel_ms(lambda: lex.search(qs, a.k), ("lex_score", "lex_select"), a.repeats)
        ki, _ = kernel_ms(lambda: imp.search(qw, a.k), ("lex_score_impact", "lex_select"), a.repeats)
        out[f"B{B}"] = {"postings_scored": scored,
                        "bm25_ms": round(bm[0], 3), "bm25_min_max_ms": [round(bm[1], 3), round(bm[2], 3)],
                        "impact_ms": round(im[0], 3), "impact_min_max_ms": [round(im[1], 3), round(im[2], 3)],
                        "lex_score_ms": kb["lex_score"], "lex_score_impact_ms": ki["lex_score_impact"],
                        "lex_select_ms_bm25": kb["lex_select"], "lex_select_ms_impact": ki["lex_select"]}
    rows = np.random.default_rng(4).integers(0, a.docs, (256, 100))
    qs = gen_queries(256, a.lex_vocab, 2)
    qw = [(np.unique(q), np.ones(len(np.unique(q)), np.float32)) for q in qs]
    kr, _ = kernel_ms(lambda: imp.score_rows(qw, rows), ("lex_score_rows_impact",), a.repeats)
    out["score_rows_256x100_kernel_ms"] = kr["lex_score_rows_impact"]
    lex.close()
    imp.close()
    return out


def copy_yardstick_gbs(nbytes, repeats):
    x = torch.empty(nbytes // 2, dtype=torch.float16, device="cuda").normal_()
    y = torch.empty_like(x)
    st = torch.cuda.current_stream().cuda_stream
    ms = median_ms(lambda: N.call_diag("sr_diag_copy", x.data_ptr(), y.data_ptr(), x.numel() * 2, 0, st),
                   repeats, torch.cuda.synchronize)[0]
    return 2.0 * x.numel() * 2 / (ms * 1e-3) / 1e9


def bench_forward(a):
    from super_rag_amd.encoder import MODELS, Encoder, random_weights
    spec = replace(MODELS["bge-m3"], vocab_size=a.vocab)
    enc = Encoder(spec, weights=random_weights(spec, 0, "hf"), max_tokens=a.max_tokens)
    rng = np.random.default_rng(1)
    w = rng.standard_normal(spec.hidden).astype(np.float32) / 32.0
    out = {"model": "bge-m3 shape, seeded weights", "vocab": a.vocab, "max_tokens": a.max_tokens}
    sync = torch.cuda.synchronize
    for B, S in ((64, 512), (2, 8192)):
        ids = torch.as_tensor(rng.integers(5, a.vocab, (B, S)).astype(np.int32)).cuda()
        ids[:, 0] = spec.bos_id
        mask = torch.ones_like(ids)
        # centre the head on this batch, so about half of the tokens keep a weight: with a large
        # bias every token weight is its pre-activation + bias, whose median gives the bias to use
        enc.set_sparse_head(w, [1000.0])
        pre = enc.embed_sparse_dev(ids, mask, pool="mean", return_token_weights=True)[4] - 1000.0
        enc.set_sparse_head(w, [-float(pre.median().item())])
        plain_mean = median_ms(lambda: enc.embed_dev(ids, mask, pool="mean"), a.repeats, sync)
        plain_cls = median_ms(lambda: enc.embed_dev(ids, mask, pool="cls"), a.repeats, sync)
        sparse_mean = median_ms(lambda: enc.embed_sparse_dev(ids, mask, pool="mean"), a.repeats, sync)
        sparse_cls = median_ms(lambda: enc.embed_sparse_dev(ids, mask, pool="cls"), a.repeats, sync)
        k, prof = kernel_ms(lambda: enc.embed_sparse_dev(ids, mask, pool="mean"),
                            ("sparse_token_weights", "sparse_terms"), a.repeats)
        tw_bytes = prof["sparse_token_weights"]["bytes"] / a.repeats
        tw_gbs = tw_bytes / (k["sparse_token_weights"] * 1e-3) / 1e9
        res = enc.embed_sparse_dev(ids, mask, pool="mean", return_token_weights=True)
        count, kept = res[3], float((res[4] > 0).float().mean().item())
        out[f"B{B}_S{S}"] = {
            "forward_mean_ms": round(plain_mean[0], 3), "forward_sparse_mean_ms": round(sparse_mean[0], 3),
            "forward_cls_ms": round(plain_cls[0], 3), "forward_sparse_cls_ms": round(sparse_cls[0], 3),
            "min_max_ms": {"mean": [round(plain_mean[1], 3), round(plain_mean[2], 3)],
                           "sparse_mean": [round(sparse_mean[1], 3), round(sparse_mean[2], 3)],
                           "cls": [round(plain_cls[1], 3), round(plain_cls[2], 3)],
                           "sparse_cls": [round(sparse_cls[1], 3), round(sparse_cls[2], 3)]},
            "sparse_token_weights_ms": k["sparse_token_weights"], "sparse_terms_ms": k["sparse_terms"],
            "sparse_token_weights_GBs": round(tw_gbs, 1),
            "tokens_kept": round(kept, 3), "pre_activation_std": round(float(pre.std().item()), 4),
            "terms_per_sequence": float(count.float().mean().item())}
    out["copy_yardstick_GBs"] = round(copy_yardstick_gbs(1 << 28, a.repeats), 1)
    enc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--lex-vocab", type=int, default=1_000_000)
    ap.add_argument("--mean-len", type=int, default=48)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--vocab", type=int, default=32000, help="encoder vocabulary rows (bge-m3: 250002)")
    ap.add_argument("--max-tokens", type=int, default=32768)
    ap.add_argument("--skip-encoder", action="store_true")
    ap.add_argument("--skip-impact", action="store_true")
    a = ap.parse_args()
    os.environ.setdefault("SUPER_RAG_AMD_SYNTHETIC", "1")
    rec = {"metric": "impact search vs BM25 on the same postings; sparse forward vs plain forward",
           "repeats": a.repeats, "statistic": "median of repeats after one warm-up call"}
    if not a.skip_impact:
        rec["impact"] = bench_impact(a)
        print("# impact done", flush=True)
    if not a.skip_encoder:
        rec["forward"] = bench_forward(a)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
