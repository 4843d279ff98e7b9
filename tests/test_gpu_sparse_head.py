"""GPU: the sparse head (k_encoder_misc.hip sparse_token_weights / sparse_terms; sr_sparse_terms_dev,
sr_encoder_forward_sparse / _dev).

The collapse is exact: compared with tests/impact_ref.py's for equality, alone on synthetic token
weights and in the forward on THE DEVICE'S OWN token weights, so the forward's rounding never decides
which terms exist.  The token weights are held against relu(h_ref . w + bias) of the fp64 oracle
within 2e-3 ||h_ref[b, s]|| ||w|| (Cauchy-Schwarz on the project's 1e-3 relative bar for one token's
state, doubled because only CLS states had been measured on the device before).  Measured on the
MI355X: max |dtw| / gate 0.029 (style "test") and 0.038 ("outlier") over the cases below.
"""
import functools

import numpy as np
import pytest

import embed_cases as EC
import impact_ref as IR
from oracle import encoder_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
MODEL = "bge-small-en"


def _u32(a):
    return np.asarray(a, F).view(np.uint32)


# -- the collapse alone ---------------------------------------------------------------------------------
def _collapse_dev(ids, mask, tw, special):
    import torch
    from super_rag_amd import _native as NV
    B, S = ids.shape
    d = lambda a, t: torch.as_tensor(np.ascontiguousarray(a, dtype=t)).cuda()
    di, dm, dw = d(ids, np.int32), d(mask, np.int32), d(tw, F)
    terms = torch.full((B, S), 77, dtype=torch.int32, device="cuda")
    weights = torch.full((B, S), 7.0, dtype=torch.float32, device="cuda")
    count = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    sp = np.ascontiguousarray(np.asarray(list(special), np.int32))
    NV.call("sr_sparse_terms_dev", NV.ptr(di), NV.ptr(dm), NV.ptr(dw), B, S, NV.ptr(sp) if sp.size else None,
            int(sp.size), NV.ptr(terms), NV.ptr(weights), NV.ptr(count), 0, NV.stream_handle())
    torch.cuda.synchronize()
    return terms.cpu().numpy(), weights.cpu().numpy(), count.cpu().numpy()


def _token_case(B, S, vocab, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, vocab, (B, S)).astype(np.int32)
    tw = np.maximum(rng.normal(0.1, 1.0, (B, S)), 0).astype(F)      # about half the tokens at 0
    tw[:, 3::11] = F(0.75)                                            # equal weights
    lens = rng.integers(max(1, S // 3), S + 1, B)
    lens[0] = S
    mask = (np.arange(S)[None] < lens[:, None]).astype(np.int32)
    ids[0, 2], ids[0, S - 1] = 4, 4                                   # a duplicate whose maximum comes later
    tw[0, 2], tw[0, S - 1] = F(0.1), F(9.0)
    ids[0, S // 2], tw[0, S // 2] = 2, F(1.0)                         # a special id in the middle
    if B > 1:
        tw[B - 1] = 0                                                 # a sequence that keeps nothing
    return ids, mask, tw


@pytest.mark.parametrize("B,S,vocab", [(2, 8192, 50), (2, 8192, 250000), (3, 128, 50), (3, 33, 6),
                                       (3, 1025, 300), (2, 64, 10)])
def test_collapse_alone_equals_the_reference(B, S, vocab):
    ids, mask, tw = _token_case(B, S, vocab, seed=S + vocab)
    for special in ((0, 2, 5), (), tuple(range(16))):
        want = IR.collapse(ids, mask, tw, special)
        got = _collapse_dev(ids, mask, tw, special)
        np.testing.assert_array_equal(got[2], want[2], err_msg=f"count, special={special}")
        np.testing.assert_array_equal(got[0], want[0], err_msg=f"terms, special={special}")
        np.testing.assert_array_equal(_u32(got[1]), _u32(want[1]), err_msg=f"weights, special={special}")
    if S >= 33:
        t, w, c = IR.collapse(ids, mask, tw, (0, 2, 5))
        assert w[0][t[0].tolist().index(4)] == F(9.0) and 2 not in t[0, :c[0]]
        assert c[B - 1] == 0 and 0 < c[0] <= S
        if vocab == 50:
            assert c[0] <= 47                                         # heavy duplication
        if vocab == 250000:
            assert c[0] > S // 4                                      # almost none


# -- the forward ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _encoder(style, max_tokens):
    from super_rag_amd.encoder import Encoder
    return Encoder(EC.spec_of(MODEL), weights=EC.weights(MODEL, style), max_tokens=max_tokens)


@functools.lru_cache(maxsize=None)
def _oracle_weights(style, dtype):
    import torch
    return EC.torch_weights(EC.weights(MODEL, style), getattr(torch, dtype), "cuda")


def _batch(B, S, ragged, seed):
    """embed_cases.batch's inputs with, in every sequence, forced repeated token ids and a [SEP] in
    the middle of the valid tokens."""
    spec = EC.spec_of(MODEL)
    ids, mask = EC.batch(EC.Case("sparse", MODEL, B, S, ragged, (), (), seed))
    lens = mask.sum(1)
    for b in range(B):
        n = int(lens[b])
        ids[b, 1:n:5] = ids[b, 1]                                     # one id at every fifth position
        ids[b, 2:n:7] = ids[b, 2]
        ids[b, n // 2] = spec.eos_id
    return ids, mask


FORWARD = [("b3_s128", 3, 128, True, 0), ("b5_s128_chunks", 5, 128, True, 256), ("b3_s32", 3, 32, False, 0)]


@pytest.mark.parametrize("name,B,S,ragged,max_tokens", FORWARD, ids=[c[0] for c in FORWARD])
@pytest.mark.parametrize("style", ["test", "outlier"])
def test_forward_sparse(style, name, B, S, ragged, max_tokens):
    import torch
    spec = EC.spec_of(MODEL)
    enc = _encoder(style, max_tokens)
    ids, mask = _batch(B, S, ragged, seed=S + B)
    valid = mask != 0
    # the head: w ~ N(0, 1 / hidden); bias centres the fp32 oracle's pre-activations, so about half
    # of the valid tokens keep a weight
    w = (np.random.default_rng(17).standard_normal(spec.hidden) / np.sqrt(spec.hidden)).astype(F)
    with torch.no_grad():
        h32 = R.encode_hidden(EC.ref_cfg(spec), _oracle_weights(style, "float32"), ids, mask)
        h64 = R.encode_hidden(EC.ref_cfg(spec), _oracle_weights(style, "float64"), ids, mask)
    h64_t = h64
    h32, h64 = h32.cpu().numpy(), h64.cpu().numpy()
    pre32 = h32.astype(np.float64) @ w.astype(np.float64)
    bias = F(-np.median(pre32[valid]))
    tw_ref = np.maximum(h64 @ w.astype(np.float64) + float(bias), 0.0)
    kept = (tw_ref[valid] > 0).mean()
    assert 0.3 <= kept <= 0.7, kept
    enc.set_sparse_head(w, [bias])
    special = sorted({spec.bos_id, spec.eos_id, spec.pad_id, spec.unk_id})
    assert special == [0, 100, 101, 102]
    for pool in ("mean", "cls"):
        dense, sparse, tw = enc.embed_sparse(ids, mask, pool=pool, return_token_weights=True)
        # (a) the dense output
        if pool == "mean":
            np.testing.assert_array_equal(_u32(dense), _u32(enc.embed(ids, mask, pool="mean")))
        ref = R.pool_hidden(h64_t, mask, pool)
        err = EC.rel(dense.astype(np.float64), ref)
        assert err.max() <= EC.DEVICE_BAR, (pool, err)
        # (b) the collapse of the device's own token weights, exactly
        want_t, want_w, want_c = IR.collapse(ids, mask, tw, special)
        assert len(sparse) == B
        for b in range(B):
            n = int(want_c[b])
            np.testing.assert_array_equal(sparse[b][0], want_t[b, :n], err_msg=f"{pool} terms of {b}")
            np.testing.assert_array_equal(_u32(sparse[b][1]), _u32(want_w[b, :n]), err_msg=f"{pool} weights of {b}")
            assert sparse[b][0].dtype == np.int32 and sparse[b][1].dtype == F
            assert n < int(((tw[b] > 0) & valid[b]).sum())            # repeated ids did collapse
            assert not set(sparse[b][0].tolist()) & set(special)
        # (c) the token weights against the fp64 oracle
        assert (tw[~valid] == 0).all() and (tw >= 0).all()
        gate = 2e-3 * np.linalg.norm(h64, axis=-1) * np.linalg.norm(w.astype(np.float64))
        ratio = np.abs(tw.astype(np.float64) - tw_ref)[valid] / gate[valid]
        print(f"sparse head {name} {style} {pool}: kept {kept:.2f}, max |dtw| / gate {ratio.max():.3f}, "
              f"median gate {np.median(gate[valid]):.4f}, tw std {tw_ref[valid].std():.2f}, "
              f"dense rel err {err.max():.2e}")
        assert ratio.max() <= 1.0, ratio.max()
    # the device entry point: the same bits, with and without the token weights returned
    d = lambda a: torch.as_tensor(a).cuda()
    out = enc.embed_sparse_dev(d(ids), d(mask), fp16=False, pool="cls", return_token_weights=True)
    out2 = enc.embed_sparse_dev(d(ids), d(mask), fp16=False, pool="cls")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_u32(out[0].cpu().numpy()), _u32(dense))
    np.testing.assert_array_equal(_u32(out[4].cpu().numpy()), _u32(tw))
    np.testing.assert_array_equal(out[1].cpu().numpy(), want_t)
    np.testing.assert_array_equal(_u32(out[2].cpu().numpy()), _u32(want_w))
    np.testing.assert_array_equal(out[3].cpu().numpy(), want_c)
    for x, y in zip(out[:4], out2):
        assert torch.equal(x, y)


def test_the_head_is_optional_and_checked():
    from super_rag_amd import _native as NV
    from super_rag_amd.encoder import Encoder, ModelSpec, random_weights
    spec = ModelSpec("tiny-bert", "bert", 300, 128, 2, 2, 256, 64, 2, 1e-12, 0)
    assert spec.unk_id == 100 and EC.spec_of("bge-small-en").unk_id == 100
    from super_rag_amd.encoder import MODELS
    assert MODELS["bge-m3"].unk_id == 3
    enc = Encoder(spec, weights=random_weights(spec, 3, "test"))
    ids = np.random.default_rng(0).integers(5, 300, (2, 16)).astype(np.int32)
    mask = np.ones_like(ids)
    before = enc.embed(ids, mask)
    with pytest.raises(NV.NativeError) as e:
        enc.embed_sparse(ids, mask)
    assert e.value.code == NV.SR_ERR_STATE and "sparse_linear.weight" in e.value.message
    with pytest.raises(ValueError):
        enc.set_sparse_head(np.zeros(64, F), [0.0])
    w = np.full(128, 0.01, F)
    NV.call("sr_encoder_set_weight", enc._h, b"sparse_linear.weight", NV.ptr(w), w.size)
    with pytest.raises(NV.NativeError) as e:
        enc.embed_sparse(ids, mask)
    assert e.value.code == NV.SR_ERR_STATE and "sparse_linear.bias" in e.value.message
    with pytest.raises(NV.NativeError) as e:
        NV.call("sr_encoder_set_weight", enc._h, b"sparse_linear.bias", NV.ptr(w), 2)
    assert e.value.code == NV.SR_ERR_INVALID
    enc.set_sparse_head(w, [100.0])                                   # every token keeps a weight
    np.testing.assert_array_equal(_u32(enc.embed(ids, mask)), _u32(before))   # existing calls unchanged
    dense, sparse = enc.embed_sparse(ids, mask, special_ids=[])
    assert dense.shape == before.shape
    for b in range(2):
        want = list(dict.fromkeys(ids[b].tolist()))
        assert sparse[b][0].tolist() == want and (sparse[b][1] > 50).all()
    with pytest.raises(NV.NativeError) as e:
        enc.embed_sparse(ids, mask, special_ids=list(range(17)))
    assert e.value.code == NV.SR_ERR_INVALID
    enc.close()
