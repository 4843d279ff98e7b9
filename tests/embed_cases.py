"""Test helper: the inputs of the embedders' precision checks, shared by the CPU test of the
rounding model (tests/test_embed_precision_model.py) and the shipped-mode GPU tests
(tests/test_gpu_encoder.py), so the condition checked on the reference alone ("the rounding design
can pass these inputs with room") is a statement about exactly the inputs the device is held to.

A case is (model, weight style, B, S, ragged, pools).  Weights are random_weights(spec,
WEIGHT_SEED[model], style); token ids and lengths come from batch().  The large-batch cases
compare BIG_ROWS of a B = 96 batch (and the same sequences at BIG_ROWS_24 of its B = 24
companion): the reference runs on those three sequences only.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import encoder_ref as R

WEIGHT_SEED = {"bge-base-en": 7, "bge-small-en": 31}
REF_CAP = 7e-4         # fp16-operand restatement vs fp64 oracle, on the reference alone
FP32_CAP = 1e-5        # fp32 oracle vs fp64 oracle
DEVICE_BAR = 1e-3      # north_star: embeddings within 1e-3 relative


@dataclass(frozen=True)
class Case:
    name: str
    model: str
    B: int
    S: int
    ragged: bool
    styles: tuple
    pools: tuple
    seed: int


CASES = (
    Case("base_s512", "bge-base-en", 4, 512, True, ("test", "outlier"), ("cls", "mean"), 512),
    Case("base_s128", "bge-base-en", 8, 128, True, ("test", "outlier"), ("cls",), 128),
    Case("base_s32", "bge-base-en", 8, 32, False, ("outlier",), ("cls",), 32),
    Case("small_s128", "bge-small-en", 8, 128, True, ("hf", "test", "outlier"), ("cls", "mean"), 129),
)
# 96 x 512 = 49,152 tokens: every GEMM on the persistent pipelined kernel; its companion of
# 24 x 512 = 12,288 tokens holds the same three sequences at BIG_ROWS_24
BIG = Case("base_big", "bge-base-en", 96, 512, True, ("test",), ("cls",), 96)
BIG_ROWS = (0, 47, 95)
BIG_ROWS_24 = (0, 11, 23)


def spec_of(model: str):
    from super_rag_amd.encoder import MODELS
    return MODELS[model]


def ref_cfg(spec) -> R.RefConfig:
    return R.RefConfig(spec.vocab_size, spec.hidden, spec.layers, spec.heads, spec.intermediate,
                       spec.max_position, spec.type_vocab, spec.ln_eps, spec.position_offset,
                       spec.classifier, spec.num_labels)


def weights(model: str, style: str) -> dict:
    from super_rag_amd.encoder import random_weights
    return random_weights(spec_of(model), seed=WEIGHT_SEED[model], style=style)


def torch_weights(w: dict, dtype, device="cpu") -> dict:
    import torch
    return {k: torch.as_tensor(v).to(device=device, dtype=dtype) for k, v in w.items()}


def batch(case: Case):
    """(ids, mask) int32 [B, S]: random tokens after the leading bos, ragged lengths in
    [S / 3, S] with row 0 at full length, padding after each row's length."""
    spec = spec_of(case.model)
    rng = np.random.default_rng(case.seed)
    B, S = case.B, case.S
    ids = rng.integers(5, spec.vocab_size, (B, S)).astype(np.int32)
    lens = rng.integers(max(1, S // 3), S + 1, B) if case.ragged else np.full(B, S)
    lens[0] = S
    mask = (np.arange(S)[None] < lens[:, None]).astype(np.int32)
    ids[:, 0] = spec.bos_id
    ids = np.where(mask == 1, ids, spec.pad_id).astype(np.int32)
    return ids, mask


def big_batches():
    """(ids96, mask96), (ids24, mask24): the companion holds rows BIG_ROWS of the large batch at
    BIG_ROWS_24 and its rows 1.. elsewhere."""
    ids, mask = batch(BIG)
    ids24, mask24 = ids[:24].copy(), mask[:24].copy()
    for src, dst in zip(BIG_ROWS, BIG_ROWS_24):
        ids24[dst], mask24[dst] = ids[src], mask[src]
    return (ids, mask), (ids24, mask24)


def rel(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)
