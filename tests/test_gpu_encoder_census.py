"""Launch census of Encoder::forward_dev: which kernels one forward pass launches, how often, and the
flops / bytes the launchers book for them, per configuration, against a recorded table.

The profile hooks (sr_profile_enable / sr_profile_read) aggregate per kernel name the launch count
and the flops and bytes each launcher computes ON THE HOST from its launch shape, so the three
numbers fingerprint every launch's M, N and K.  A configuration is one freshly built encoder and its
first forward pass.  Only launchers that book a profile record appear: the GEMMs, attention, the
LayerNorm / statistics kernels, embedding, pooling and the token heads do; the position ids, the
classifier's final dot product and the weight preparation of prepare_fold do not.  The
configurations are the smallest at which each branch of the folded-layer loop, the unfolded loop and
the output stage is taken: 3 layers (first, middle, last) and B = 5 throughout.

The expected table, tests/golden/encoder_launch_census.json, was recorded by
tests/golden/gen_encoder_census.py on the commit BEFORE forward_dev was split into stages; this test
never regenerates it.  launches compare exactly, flops and bytes to a relative 1e-12 (the same host
arithmetic on the same shapes; the slack only covers the order of the fp64 sums).
"""
import json
import os

import numpy as np
import pytest

from test_gpu_encoder import _batch, _tiny

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_launch_census.json")
B = 5
SWITCHES = ("SR_LN_FOLD", "SR_FUSED_QKV_ATTN", "SR_KVFREE_CLS")

# shape a: the folded cross-encoder at which K5c (S = 128, head dim 64) and the K/V-free last layer
# exist; shape d: folded, d % 256 == 0, no K/V-free form at S = 16; shape f: unfolded, fp32 residual
_A = dict(arch="xlmr", d=768, L=3, H=12, F=1024, classifier=1, P=200, res16=True)
_D = dict(arch="xlmr", d=256, L=3, H=4, F=512, classifier=1, P=200, res16=True)
_E = dict(arch="xlmr", d=256, L=3, H=4, F=512, classifier=0, P=200, res16=True)
_F = dict(arch="bert", d=128, L=3, H=2, F=256, classifier=0, P=80, res16=False)

# name -> (shape, S, fp8 mode, call, environment switches, max_tokens)
CONFIGS = {}
for _m in (0, 1, 2, 3):   # a: fused QKV + attention layers and the K/V-free last layer
    CONFIGS[f"a_s128_fp8_{_m}"] = (_A, 128, _m, "cross", {}, 0)
CONFIGS["b_s128_unfused_qkv"] = (_A, 128, 0, "cross", {"SR_FUSED_QKV_ATTN": "0"}, 0)
CONFIGS["b_s128_kv_gemm_last"] = (_A, 128, 0, "cross", {"SR_KVFREE_CLS": "0"}, 0)
for _m in (0, 3):         # c: unfused layers
    CONFIGS[f"c_s64_fp8_{_m}"] = (_A, 64, _m, "cross", {}, 0)
CONFIGS["d_s16_cls_only_last"] = (_D, 16, 0, "cross", {}, 0)
CONFIGS["e_s16_folded_embed_mean"] = (_E, 16, 0, "embed_mean", {}, 0)
CONFIGS["e_s16_folded_embed_cls"] = (_E, 16, 0, "embed_cls", {}, 0)
CONFIGS["f_s17_unfolded_embed"] = (_F, 17, 0, "embed_cls", {}, 0)
CONFIGS["g_s17_token_heads"] = (_F, 17, 0, "multivec", {}, 0)
CONFIGS["g_s17_token_heads_two_chunks"] = (_F, 17, 0, "multivec", {}, 3 * 17)   # chunks of 3 + 2


def run_census(name, setenv, delenv):
    """Build the configuration's encoder, run its one forward pass under the profiler and return
    {kernel: {"launches", "flops", "bytes"}}.  setenv(k, v) / delenv(k) change the environment
    (monkeypatch's in the test) before the encoder is built."""
    from super_rag_amd import _native as N
    from super_rag_amd.encoder import Encoder, random_weights
    shape, S, fp8, call, env, max_tokens = CONFIGS[name]
    for k in SWITCHES:
        delenv(k)
    for k, v in env.items():
        setenv(k, v)
    spec = _tiny(**shape)
    enc = Encoder(spec, weights=random_weights(spec, seed=11, style="test"), max_tokens=max_tokens)
    try:
        if fp8:
            enc.set_fp8(fp8)
        if call == "multivec":
            rng = np.random.default_rng(12)
            enc.set_sparse_head(rng.standard_normal(spec.hidden), [0.1])
            enc.set_colbert_head(0.1 * rng.standard_normal((128, spec.hidden)), np.zeros(128))
        ids, mask = _batch(spec, B, S, seed=13)
        N.profile_enable(True)
        try:
            if call == "cross":
                enc.cross_score(ids, mask)
            elif call == "multivec":
                enc.embed_multivec(ids, mask, with_sparse=True)
            else:
                enc.embed(ids, mask, pool=call.split("_")[1])
        finally:
            N.profile_enable(False)
        stats = N.profile_read()
    finally:
        enc.close()
    return {k: {f: v[f] for f in ("launches", "flops", "bytes")} for k, v in sorted(stats.items())}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_lists_every_configuration(golden):
    assert sorted(golden) == sorted(CONFIGS)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_launch_census(name, golden, monkeypatch):
    got = run_census(name, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    want = golden[name]
    print(name, json.dumps(got))
    assert sorted(got) == sorted(want), "the set of launched kernels changed"
    for k, w in want.items():
        g = got[k]
        assert g["launches"] == w["launches"], (k, g, w)
        for f in ("flops", "bytes"):
            assert abs(g[f] - w[f]) <= 1e-12 * abs(w[f]), (k, f, g, w)
