"""Embedding error of the fp32-residual embedders against the fp32 oracle with and without the
split (hi + lo) weights (SR_WEIGHT_SPLIT), per model, weight style ("test", "hf", "outlier") and
sequence length (S = 32 full rows; S = 32, 128, 512 ragged), and the embed time at B = 256,
S = 32 for each model / style / mode.  The oracle runs on the GPU (torch fp32, TF32 off).

    python tools/embed_split_error.py [--models bge-base-en,bge-small-en,bge-m3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-rag_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import encoder_ref as R  # noqa: E402
from super_rag_amd.encoder import MODELS, Encoder, random_weights  # noqa: E402


def cfg(spec):
    return R.RefConfig(spec.vocab_size, spec.hidden, spec.layers, spec.heads, spec.intermediate,
                       spec.max_position, spec.type_vocab, spec.ln_eps, spec.position_offset,
                       spec.classifier, spec.num_labels)


def batch(spec, B, S, ragged, seed=1):
    rng = np.random.default_rng(seed)
    ids = rng.integers(1000, spec.vocab_size, (B, S)).astype(np.int32)
    lens = rng.integers(max(1, S // 3), S + 1, B) if ragged else np.full(B, S)
    lens[0] = S
    mask = (np.arange(S)[None] < lens[:, None]).astype(np.int32)
    ids[:, 0] = spec.bos_id
    return np.where(mask == 1, ids, spec.pad_id).astype(np.int32), mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="bge-base-en,bge-small-en,bge-m3")
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    dev = torch.device("cuda", 0)
    for name in a.models.split(","):
        spec = MODELS[name]
        for style in ("test", "hf", "outlier"):
            w = random_weights(spec, seed=7, style=style)
            wd = {k: torch.as_tensor(v, device=dev) for k, v in w.items()}
            shapes = [(8, 32, False), (8, 32, True), (8, 128, True), (4, 512, True)]
            cases = [(B, S, rg) + batch(spec, B, S, rg) for B, S, rg in shapes]
            refs = [R.embed(cfg(spec), wd, ids, mask) for _, _, _, ids, mask in cases]
            for split in ("1", "0"):
                os.environ["SR_WEIGHT_SPLIT"] = split
                enc = Encoder(spec, device=0, weights=w)
                for (B, S, rg, ids, mask), ref in zip(cases, refs):
                    got = enc.embed(ids, mask)
                    err = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
                    print(f"{name} weights={style} split={split} B={B} S={S}{' ragged' if rg else ''}: "
                          f"max rel err {err.max():.3e} mean {err.mean():.3e}", flush=True)
                di = torch.from_numpy(np.tile(cases[0][3], (32, 1))).to(dev)
                dm = torch.ones_like(di)
                for _ in range(3):
                    enc.embed_dev(di, dm)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    enc.embed_dev(di, dm)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / 10 * 1e3
                print(f"{name} weights={style} split={split}: B=256 S=32 embed {ms:.3f} ms", flush=True)
                enc.close()
            del wd, refs


if __name__ == "__main__":
    main()
