"""GPU: the multi-vector head in the encoder forward (k_encoder_misc.hip colbert_pack after the head's
GEMM; sr_encoder_forward_multivec / _dev) on bge-small-en, and the path from there through sr_mv to
m3_rerank.

The vectors are held against the fp64 oracle (encoder_ref.encode_hidden -> colbert_ref.head):
||u_dev - u_ref|| <= 4e-3 ||h_ref|| ||W||_2 / ||v_ref|| + 2^-9 (the project's 2e-3 ||h_ref|| bar for
one token's state taken through W, ||W||_2 the spectral norm, doubled by the normalisation since
||d(v / ||v||)|| <= 2 ||dv|| / ||v||, plus two fp16 roundings).  The end-to-end comparisons use THE
DEVICE'S OWN vectors and scores, so the forward's rounding never decides them.
Measured on the MI355X, max ||u_dev - u_ref|| / gate at dc = 384 / 128: style "test" 0.062 / 0.051 (B = 3,
S = 128), 0.063 / 0.051 (B = 5 chunked), 0.061 / 0.049 (S = 32); "outlier" 0.131 / 0.112, 0.175 / 0.146,
0.068 / 0.053.
"""
import functools

import numpy as np
import pytest

import colbert_ref as CR
import embed_cases as EC
from oracle import encoder_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
MODEL = "bge-small-en"


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _encoder(style, max_tokens):
    from super_rag_amd.encoder import Encoder
    return Encoder(EC.spec_of(MODEL), weights=EC.weights(MODEL, style), max_tokens=max_tokens)


@functools.lru_cache(maxsize=None)
def _oracle_weights(style):
    import torch
    return EC.torch_weights(EC.weights(MODEL, style), torch.float64, "cuda")


def _head(dc, hidden):
    rng = np.random.default_rng(100 + dc)
    W = (rng.standard_normal((dc, hidden)) / np.sqrt(hidden)).astype(F)
    b = (0.1 * rng.standard_normal(dc)).astype(F)
    return W, b


def _sparse_head(hidden):
    w = (np.random.default_rng(17).standard_normal(hidden) / np.sqrt(hidden)).astype(F)
    return w, [F(0.05)]


FORWARD = [("b3_s128", 3, 128, True, 0), ("b5_s128_chunks", 5, 128, True, 256), ("b3_s32", 3, 32, False, 0)]


@pytest.mark.parametrize("name,B,S,ragged,max_tokens", FORWARD, ids=[c[0] for c in FORWARD])
@pytest.mark.parametrize("style", ["test", "outlier"])
def test_forward_multivec(style, name, B, S, ragged, max_tokens):
    import torch
    spec = EC.spec_of(MODEL)
    enc = _encoder(style, max_tokens)
    ids, mask = EC.batch(EC.Case("colbert", MODEL, B, S, ragged, (), (), S + B))
    if name == "b3_s128":                                                 # a hole in the middle of the valid tokens
        n = int(mask[1].sum())
        assert n >= 8
        mask[1, n // 2] = 0
        mask[1, n // 2 + 1] = 0
    with torch.no_grad():
        h64_t = R.encode_hidden(EC.ref_cfg(spec), _oracle_weights(style), ids, mask)
    h64 = h64_t.cpu().numpy()
    enc.set_sparse_head(*_sparse_head(spec.hidden))
    want_len = ((mask != 0) & (np.arange(S)[None] >= 1)).sum(1).astype(np.int32)
    if name != "b3_s128":
        np.testing.assert_array_equal(want_len, mask.sum(1) - 1)
    d = lambda a: torch.as_tensor(a).cuda()
    for dc in (384, 128):
        W, b = _head(dc, spec.hidden)
        enc.set_colbert_head(W, b)
        assert enc.has_colbert_head and enc.colbert_dim == dc
        v_ref, u_ref = CR.head_all(h64, W, b)
        w2 = np.linalg.norm(W.astype(np.float64), 2)
        worst = 0.0
        for pool in ("mean", "cls"):
            dense, mv = enc.embed_multivec(ids, mask, pool=pool)
            # (a) the dense output
            if pool == "mean":
                np.testing.assert_array_equal(_u32(dense), _u32(enc.embed(ids, mask, pool="mean")))
            err = EC.rel(dense.astype(np.float64), R.pool_hidden(h64_t, mask, pool))
            assert err.max() <= EC.DEVICE_BAR, (pool, err)
            # (b) lengths and compaction
            assert [m.shape for m in mv] == [(int(n), dc) for n in want_len]
            # (c) the vectors against the fp64 oracle
            for i in range(B):
                pos = CR.kept_positions(mask[i])
                gate = (4e-3 * np.linalg.norm(h64[i, pos], axis=-1) * w2 / np.linalg.norm(v_ref[i, pos], axis=-1)
                        + 2.0 ** -9)
                diff = np.linalg.norm(mv[i].astype(np.float64) - u_ref[i, pos], axis=-1)
                worst = max(worst, float((diff / gate).max()))
                assert (diff <= gate).all(), (pool, i, float((diff / gate).max()))
                assert np.abs(np.linalg.norm(mv[i].astype(np.float64), axis=-1) - 1.0).max() <= 2.0 ** -9
            # (d) with the sparse outputs: the same bits as embed_sparse, and the same vectors
            dense_s, sparse_s = enc.embed_sparse(ids, mask, pool=pool)
            dense3, mv3, sparse3 = enc.embed_multivec(ids, mask, pool=pool, with_sparse=True)
            np.testing.assert_array_equal(_u32(dense3), _u32(dense_s))
            np.testing.assert_array_equal(_u32(dense3), _u32(dense))
            for i in range(B):
                np.testing.assert_array_equal(_u32(mv3[i]), _u32(mv[i]))
                np.testing.assert_array_equal(sparse3[i][0], sparse_s[i][0])
                np.testing.assert_array_equal(_u32(sparse3[i][1]), _u32(sparse_s[i][1]))
        print(f"colbert head {name} {style} dc {dc}: max ratio {worst:.3f}")
        # the device entry point: the same bits, zero rows past the length
        out, vecs, lens = enc.embed_multivec_dev(d(ids), d(mask), fp16=False, pool="cls")
        out6 = enc.embed_multivec_dev(d(ids), d(mask), fp16=False, pool="cls", with_sparse=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_u32(out.cpu().numpy()), _u32(dense))
        np.testing.assert_array_equal(lens.cpu().numpy(), want_len)
        hv = vecs.cpu().numpy()
        assert hv.dtype == np.float16 and hv.shape == (B, S, dc)
        for i in range(B):
            n = int(want_len[i])
            np.testing.assert_array_equal(hv[i, :n].astype(F), mv[i])
            assert (hv[i, n:].view(np.uint16) == 0).all()
        assert torch.equal(out6[1], vecs) and torch.equal(out6[2], lens) and torch.equal(out6[0], out)
        for i in range(B):
            c = int(out6[5][i])
            np.testing.assert_array_equal(out6[3][i, :c].cpu().numpy(), sparse_s[i][0])


def test_documents_to_index_to_rerank():
    import torch
    from super_rag_amd.lexical import NativeImpactIndex
    from super_rag_amd.multivec import NativeMultiVectorIndex, m3_rerank
    from super_rag_amd.store import NativeStore
    spec = EC.spec_of(MODEL)
    enc = _encoder("test", 0)
    dc = 128
    enc.set_colbert_head(*_head(dc, spec.hidden))
    enc.set_sparse_head(_sparse_head(spec.hidden)[0], [F(0.5)])
    ids, mask = EC.batch(EC.Case("colbert_docs", MODEL, 12, 32, True, (), (), 5))
    qids, qmask = EC.batch(EC.Case("colbert_q", MODEL, 3, 16, True, (), (), 6))
    qids[:, 1:9] = ids[[0, 4, 7], 1:9]                                     # shared tokens: sparse overlap
    d = lambda a: torch.as_tensor(a).cuda()
    out, vecs, lens, terms, weights, count = enc.embed_multivec_dev(d(ids), d(mask), fp16=False, with_sparse=True)
    mv = NativeMultiVectorIndex(dc)
    assert mv.add_dev(vecs, lens) == 0
    dense_d, mv_d, sparse_d = enc.embed_multivec(ids, mask, with_sparse=True)
    dense_q, mv_q, sparse_q = enc.embed_multivec(qids, qmask, with_sparse=True)
    np.testing.assert_array_equal(lens.cpu().numpy(), [m.shape[0] for m in mv_d])
    for i in range(12):
        np.testing.assert_array_equal(mv.get(i), mv_d[i])
    rows = np.stack([np.arange(12), np.arange(12)[::-1], np.r_[np.arange(0, 12, 2), -1, 12, 3, 3, 5, 1]]).astype(np.int64)
    got = mv.score_rows(mv_q, rows)
    ref = CR.maxsim_rows(mv_q, mv_d, rows)
    for b in range(3):
        for k in range(12):
            if np.isneginf(ref[b, k]):
                assert np.isneginf(got[b, k])
            else:
                assert abs(got[b, k] - ref[b, k]) <= CR.gate(dc, len(mv_q[b]), mv_q[b], mv_d[rows[b, k]])
    # m3_rerank against the reference combination of the device's own three score arrays
    store = NativeStore(spec.hidden)
    store.add(dense_d)
    impact = NativeImpactIndex()
    impact.add(sparse_d)
    store.remove([9])
    cos = store.score_rows(dense_q, rows)
    sp = impact.score_rows(sparse_q, rows)
    assert (sp[np.isfinite(sp)] > 0).any()
    for imp, qs, spv, w in ((None, None, None, (1, 1, 1)), (impact, sparse_q, sp, (1, 1, 1)),
                            (impact, sparse_q, sp, (0.4, 0.2, 0.4))):
        score, r = m3_rerank(store, mv, dense_q, mv_q, rows, 5, impact=imp, q_sparse=qs, weights=w)
        want_s, want_r = CR.rerank(cos, got, spv, rows, 5, w)
        np.testing.assert_array_equal(r, want_r)
        fin = np.isfinite(want_s)
        assert fin[:, 0].all() and np.isneginf(score[~fin]).all()
        assert (np.abs(score[fin].astype(np.float64) - want_s[fin]) <= np.spacing(np.abs(want_s[fin]))).all()
        assert not (r == 9).any() and (r >= 0).all()
    score, r = m3_rerank(store, mv, dense_q, mv_q, rows[:, :3], 5)
    assert (r[:, 3:] == -1).all() and np.isneginf(score[:, 3:]).all()
    # m3_search = the first stage, then m3_rerank: without an impact index (search_sim) and with one
    # (sparse_hybrid_search), bit for bit
    from super_rag_amd.lexical import sparse_hybrid_search
    from super_rag_amd.multivec import m3_search
    s1, r1 = m3_search(store, mv, dense_q, mv_q, 3, k_cand=8)
    _, cand = store.search_sim(dense_q, 8)
    s2, r2 = m3_rerank(store, mv, dense_q, mv_q, cand, 3)
    np.testing.assert_array_equal(r1, r2)
    np.testing.assert_array_equal(_u32(s1), _u32(s2))
    assert (r1 >= 0).all() and not (r1 == 9).any()
    s1, r1 = m3_search(store, mv, dense_q, mv_q, 3, k_cand=8, impact=impact, q_sparse=sparse_q, weights=(1, 2, 1))
    _, cand = sparse_hybrid_search(store, impact, dense_q, sparse_q, 8)
    s2, r2 = m3_rerank(store, mv, dense_q, mv_q, cand, 3, impact=impact, q_sparse=sparse_q, weights=(1, 2, 1))
    np.testing.assert_array_equal(r1, r2)
    np.testing.assert_array_equal(_u32(s1), _u32(s2))
    assert (r1 >= 0).all() and not (r1 == 9).any()
    # the default k_cand = 4 k is clamped to the 1024 candidates one query can rerank
    s1, r1 = m3_search(store, mv, dense_q, mv_q, 300)
    assert r1.shape == (3, 300) and (r1[:, :11] >= 0).all() and (r1[:, 11:] == -1).all()
    for bad in (1025, 2):
        with pytest.raises(ValueError, match="k_cand"):
            m3_search(store, mv, dense_q, mv_q, 3, k_cand=bad)
    for o in (mv, store, impact):
        o.close()


def test_the_head_is_optional_and_checked():
    from super_rag_amd import _native as NV
    from super_rag_amd.encoder import Encoder, ModelSpec, random_weights
    spec = ModelSpec("tiny-bert", "bert", 300, 128, 2, 2, 256, 64, 2, 1e-12, 0)
    enc = Encoder(spec, weights=random_weights(spec, 3, "test"))
    assert not enc.has_colbert_head and enc.colbert_dim == 0
    ids = np.random.default_rng(0).integers(5, 300, (2, 16)).astype(np.int32)
    mask = np.ones_like(ids)
    before = enc.embed(ids, mask)
    with pytest.raises(NV.NativeError) as e:
        enc.embed_multivec(ids, mask)
    assert e.value.code == NV.SR_ERR_STATE and "colbert_linear.weight" in e.value.message
    with pytest.raises(ValueError):
        enc.set_colbert_head(np.zeros((128, 64), F), np.zeros(128, F))
    with pytest.raises(ValueError):
        enc.set_colbert_head(np.zeros((96, 128), F), np.zeros(96, F))
    rng = np.random.default_rng(1)
    w = (rng.standard_normal((128, 128)) / 11.0).astype(F)
    for bad in (128 * 96, 128 * 128 + 1, 128 * 1152):                       # dc 96, no whole rows, dc 1152
        big = np.zeros(bad, F)
        with pytest.raises(NV.NativeError) as e:
            NV.call("sr_encoder_set_weight", enc._h, b"colbert_linear.weight", NV.ptr(big), big.size)
        assert e.value.code == NV.SR_ERR_INVALID
    NV.call("sr_encoder_set_weight", enc._h, b"colbert_linear.weight", NV.ptr(w), w.size)
    assert enc.colbert_dim == 128
    with pytest.raises(NV.NativeError) as e:
        enc.embed_multivec(ids, mask)
    assert e.value.code == NV.SR_ERR_STATE and "colbert_linear.bias" in e.value.message
    with pytest.raises(NV.NativeError) as e:
        NV.call("sr_encoder_set_weight", enc._h, b"colbert_linear.bias", NV.ptr(w), 256)
    assert e.value.code == NV.SR_ERR_INVALID
    NV.call("sr_encoder_ready", enc._h)                                    # never part of ready
    enc.set_colbert_head(w, np.zeros(128, F))
    np.testing.assert_array_equal(_u32(enc.embed(ids, mask)), _u32(before))    # existing calls unchanged
    dense, mv = enc.embed_multivec(ids, mask)
    assert dense.shape == before.shape and [m.shape for m in mv] == [(15, 128)] * 2
    # a half-given sparse group, and null outputs
    B, S = ids.shape
    dense = np.empty((B, 128), F)
    vecs = np.empty((B, S, 128), F)
    lens = np.zeros(B, np.int32)
    terms = np.zeros((B, S), np.int32)
    p = NV.ptr
    with pytest.raises(NV.NativeError) as e:
        NV.call("sr_encoder_forward_multivec", enc._h, p(ids), p(mask), None, B, S, 0, p(dense), p(vecs),
                p(lens), None, 0, None, p(terms), None, None)
    assert e.value.code == NV.SR_ERR_INVALID
    with pytest.raises(NV.NativeError) as e:
        NV.call("sr_encoder_forward_multivec", enc._h, p(ids), p(mask), None, B, S, 0, p(dense), None,
                p(lens), None, 0, None, None, None, None)
    assert e.value.code == NV.SR_ERR_INVALID
    with pytest.raises(NV.NativeError) as e:                               # the sparse head is still missing
        enc.embed_multivec(ids, mask, with_sparse=True)
    assert e.value.code == NV.SR_ERR_STATE and "sparse_linear.weight" in e.value.message
    enc.close()
