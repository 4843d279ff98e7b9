"""GPU: the multi-vector index's fp8 storage mode (SR_DTYPE_FP8_E4M3; multivec.hip, k_multivec.hip's
maxsim_kernel<true> and mv_pack_fp8_kernel).  A token element x is stored as e4m3_rne(256 fp16(x)); the
score is MaxSim of the caller's fp16 query against the dequantised tokens d^ = e4m3_value / 256, fp32
accumulation.  The reference is fp64 on those values (tests/mv_fp8_ref.py on tests/colbert_ref.py).

Gate, the fp16 kernel's and derived the same way: the operands are the fp16 values of 256 d^ (exact:
every e4m3 value is a normal fp16) and of q, so the products are exact in fp32, only the dim
accumulations and the Lq additions of the mean round, and the last factor 2^-8 is exact:
|score - ref| <= (dim + Lq) 2^-23 max||q_i|| max||d^_j||.
Against the fp16 index on the same tokens: |max_j a_j - max_j b_j| <= max_j |a_j - b_j| with a_j = q_i .
d^_j and b_j = q_i . d_j, carried through the mean, gives |maxsim8 - maxsim16| <= max||q_i|| max_j
||d^_j - d_j|| for the exact values; each device score adds its own gate.
Bit-identity is checked on the uint32 views.
"""
import functools

import numpy as np
import pytest

import colbert_ref as CR
import mv_fp8_ref as Q

pytestmark = pytest.mark.gpu

F = np.float32
DIMS = [64, 128, 384, 1024]
LQS = [1, 15, 16, 17, 64, 65, 200]
DOC_LENS = [0, 1, 15, 16, 17, 63, 65, 511, 2049]
N_RANK = 100


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _new(dim, dtype="fp8"):
    from super_rag_amd.multivec import NativeMultiVectorIndex
    return NativeMultiVectorIndex(dim, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _corpus(dim):
    """The mixed-length rows, then N_RANK ranking candidates built against a 32-token query; next to the
    tokens as added (fp16 values) their dequantised fp64 values, computed once."""
    rng = np.random.default_rng(2000 + dim)
    docs = [CR.unit_f16(rng, n, dim) for n in DOC_LENS]
    rq = CR.unit_f16(rng, 32, dim)
    alphas = np.linspace(0.0, 0.9, N_RANK)
    docs += [CR.mixed_doc(rng, rq, 32 + int(rng.integers(0, 24)), a) for a in rng.permutation(alphas)]
    deq = [Q.dequant(Q.quant(d)) for d in docs]
    return docs, deq, rq


@functools.lru_cache(maxsize=None)
def _index(dim, dtype="fp8"):
    docs, _, _ = _corpus(dim)
    x = _new(dim, dtype)
    assert x.add(docs) == 0
    return x


def _queries(rng, lq, dim):
    """Three queries of lengths lq, (lq + 1) // 2 and 1 in one padded array with ld_q = lq + 3 and NaN
    in every row at and past q_len."""
    lens = [lq, (lq + 1) // 2, 1]
    qs = [CR.unit_f16(rng, n, dim) for n in lens]
    pad = np.full((3, lq + 3, dim), np.nan, F)
    for b, q in enumerate(qs):
        pad[b, :q.shape[0]] = q
    return qs, pad, np.asarray(lens, np.int32)


def _check(got, qs, deq, rows, dim, live=None):
    """deq: the dequantised fp64 tokens of every row."""
    ref = CR.maxsim_rows(qs, deq, rows, live)
    worst = 0.0
    for b in range(rows.shape[0]):
        for k in range(rows.shape[1]):
            if np.isneginf(ref[b, k]):
                assert np.isneginf(got[b, k]), (b, k, got[b, k])
                continue
            g = CR.gate(dim, len(qs[b]), qs[b], deq[rows[b, k]])
            err = abs(float(got[b, k]) - ref[b, k])
            worst = max(worst, err / g)
            assert err <= g, (dim, len(qs[b]), b, k, rows[b, k], got[b, k], ref[b, k], err / g)
    return worst


# -- what is stored -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 128])
def test_stored_bytes_on_the_grid_by_every_way_of_adding(dim):
    import torch
    toks = Q.grid_tokens(dim)                                             # fp16 values: ties, subnormals, saturation
    want = Q.stored(toks)
    assert np.isfinite(want).all() and np.abs(want).max() == F(1.75)
    # fp32 input that is no fp16 value: the host path rounds to fp16 first (the pinned double rounding)
    pos = np.sort(Q.E4M3[:0x7F])
    mids = (pos[:-1] + pos[1:]) / 2.0
    odd = np.zeros(2 * dim, F)
    odd[:mids.size] = (mids / 256.0 * (1.0 + 2.0 ** -20)).astype(F)      # just above every tie
    odd = odd.reshape(2, dim)
    assert (Q.quant(odd) != Q.quant_direct(odd)).any()
    x = _new(dim)
    assert x.dtype == "fp8" and x.nbytes == 0
    assert x.add([toks, odd, toks[:0], toks[3:5]]) == 0
    np.testing.assert_array_equal(_u32(x.get(0)), _u32(want))
    np.testing.assert_array_equal(_u32(x.get(1)), _u32(Q.stored(odd)))
    assert x.get(2).shape == (0, dim)
    np.testing.assert_array_equal(_u32(x.get(3)), _u32(want[3:5]))
    n_tok = toks.shape[0] + 2 + 2
    assert x.stats() == {"rows": 4, "live": 4, "tokens": n_tok} and x.nbytes == n_tok * dim
    # add_dev of the same fp16 values, in bulk (ld_tok > len, the padding never read into the pool) and alone
    n = toks.shape[0]
    pad = np.full((3, n + 3, dim), 7.0, np.float16)
    pad[0, :n] = toks.astype(np.float16)
    pad[1, :2] = toks[3:5].astype(np.float16)
    pad[2, :n - 1] = toks[1:].astype(np.float16)
    lens = np.asarray([n, 2, n - 1], np.int32)
    dv, dl = torch.as_tensor(pad).cuda(), torch.as_tensor(lens).cuda()
    y, z = _new(dim), _new(dim)
    assert y.add_dev(dv, dl) == 0
    for i in range(3):
        assert z.add_dev(dv[i:i + 1].contiguous(), dl[i:i + 1].contiguous()) == i
    for other in (y, z):
        assert other.stats() == {"rows": 3, "live": 3, "tokens": 2 * n + 1}
        np.testing.assert_array_equal(_u32(other.get(0)), _u32(want))
        np.testing.assert_array_equal(_u32(other.get(1)), _u32(want[3:5]))
        np.testing.assert_array_equal(_u32(other.get(2)), _u32(want[1:]))
        other.close()
    # rows added one call each on the host path: the same bytes as in bulk
    w = _new(dim)
    for i, d in enumerate((toks, odd, toks[:0], toks[3:5])):
        assert w.add([d]) == i
    for i in range(4):
        np.testing.assert_array_equal(_u32(w.get(i)), _u32(x.get(i)))
    w.close()
    x.close()


def test_rows_survive_pool_growth():
    dim = 64
    rng = np.random.default_rng(5)
    x = _new(dim)
    first = CR.unit_f16(rng, 37, dim)
    q = CR.unit_f16(rng, 9, dim)
    x.add([first])
    s0 = x.score_rows([q], np.array([[0]], np.int64))
    total, adds = 37, 0
    while total <= 4096:                                                  # the pool starts at 1024 tokens and doubles
        x.add([CR.unit_f16(rng, 700, dim)])
        total += 700
        adds += 1
    assert adds >= 5 and x.stats()["tokens"] == total and x.nbytes == total * dim
    np.testing.assert_array_equal(_u32(x.get(0)), _u32(Q.stored(first)))
    np.testing.assert_array_equal(_u32(x.score_rows([q], np.array([[0]], np.int64))), _u32(s0))
    x.close()


# -- the score ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_maxsim8_against_fp64_over_query_and_document_lengths(dim):
    x = _index(dim)
    docs, deq, rq = _corpus(dim)
    rng = np.random.default_rng(dim)
    nd = len(DOC_LENS)
    worst = 0.0
    for lq in LQS:
        qs, pad, qlen = _queries(rng, lq, dim)
        # (3, 7): every mixed-length row, a missing one and a row past the index, over the queries
        rows = np.array([[8, 0, 1, 2, -1, 3, 4], [5, 6, 7, 8, 0, len(docs), 2], [7, 8, 4, 6, 5, 1, 3]], np.int64)
        got = x.score_rows(pad, rows, q_len=qlen)
        worst = max(worst, _check(got, qs, deq, rows, dim))
        one = x.score_rows(pad[:1], rows[:1, :1], q_len=qlen[:1])                       # (1, 1)
        np.testing.assert_array_equal(_u32(one), _u32(got[:1, :1]))
        worst = max(worst, _check(one, qs[:1], deq, rows[:1, :1], dim))
        cand = np.arange(nd, nd + N_RANK, dtype=np.int64)                               # (2, 100)
        r100 = np.stack([cand, np.r_[np.arange(nd), cand[:N_RANK - nd]]])
        got = x.score_rows(pad[:2], r100, q_len=qlen[:2])
        worst = max(worst, _check(got, qs[:2], deq, r100, dim))
    print(f"maxsim8 dim {dim}: max |err| / gate {worst:.3f}")


@pytest.mark.parametrize("dim", [64, 128])
def test_e4m3_subnormal_tokens_are_not_flushed(dim):
    x = _new(dim)
    sub = np.full((17, dim), 7 * 2.0 ** -17, F)                           # 256 x = 7 * 2^-9: an e4m3 subnormal
    one = np.zeros((3, dim), F)
    one[1, dim - 1] = 2.0 ** -9 / 256.0                                   # the smallest nonzero code, once
    x.add([sub, one, sub[:1]])
    np.testing.assert_array_equal(x.get(0), sub)                          # stored exactly
    np.testing.assert_array_equal(x.get(1), one)
    q = np.ones((3, dim), F)
    rows = np.array([[0, 1, 2]], np.int64)
    got = x.score_rows([q], rows)
    deq = [Q.dequant(Q.quant(d)) for d in (sub, one, sub[:1])]
    ref = CR.maxsim_rows([q], deq, rows)
    assert ref[0, 0] == dim * 7 * 2.0 ** -17 and ref[0, 1] == 2.0 ** -17 and ref[0, 2] == ref[0, 0]
    for k in range(3):
        g = CR.gate(dim, 3, q, deq[k])
        assert g < ref[0, k] / 8                                          # a flushed path (score 0) cannot pass
        assert abs(float(got[0, k]) - ref[0, k]) <= g, (k, got[0, k], ref[0, k], g)
    x.close()


@pytest.mark.parametrize("dim", [64, 1024])
def test_against_the_fp16_index_on_the_same_tokens(dim):
    x8, x16 = _index(dim), _index(dim, "fp16")
    docs, deq, rq = _corpus(dim)
    assert x16.dtype == "fp16" and x16.nbytes == 2 * x8.nbytes == 2 * dim * sum(d.shape[0] for d in docs)
    rng = np.random.default_rng(17 + dim)
    qs = [rq, CR.unit_f16(rng, 65, dim)]
    nd = len(DOC_LENS)
    rows = np.stack([np.arange(nd, nd + 20), np.r_[np.arange(1, nd), np.arange(nd, nd + 20 - (nd - 1))]]).astype(np.int64)
    s8, s16 = x8.score_rows(qs, rows), x16.score_rows(qs, rows)
    worst = 0.0
    for b in range(2):
        nq = np.linalg.norm(qs[b].astype(np.float64), axis=1).max()
        for k in range(rows.shape[1]):
            r = rows[b, k]
            dq = np.linalg.norm(deq[r] - docs[r].astype(np.float64), axis=1).max()     # from the reference
            bound = nq * dq + CR.gate(dim, len(qs[b]), qs[b], deq[r]) + CR.gate(dim, len(qs[b]), qs[b], docs[r])
            diff = abs(float(s8[b, k]) - float(s16[b, k]))
            worst = max(worst, diff / bound)
            assert diff <= bound, (dim, b, k, r, s8[b, k], s16[b, k], bound)
    assert (s8 != s16).any()                                              # two pools, not one
    print(f"fp8 vs fp16 dim {dim}: max |diff| / bound {worst:.3f}")


@pytest.mark.parametrize("dim", [64, 384])
def test_adversarial_cases(dim):
    rng = np.random.default_rng(11 + dim)
    x = _new(dim)
    docs, queries = [], []
    for ld in (1, 17, 65):                                                # every dot product negative
        q, d = CR.all_negative_case(rng, 5, ld, dim)
        queries.append(q), docs.append(d)
    for ld in (17, 65, 2049):                                             # the argmax in the last partial tile
        q, d = CR.tail_argmax_case(rng, 33, ld, dim)
        queries.append(q), docs.append(d)
    q, d = CR.first_last_case(rng, 4, 40, dim)                            # best matches first and last
    queries.append(q), docs.append(d)
    d2 = d.copy()                                                         # two documents, one token apart
    d2[20] = q[2]
    queries.append(q), docs.append(d2)
    deq = [Q.dequant(Q.quant(t)) for t in docs]
    # the generators' properties hold on the dequantised tokens too
    for i in range(3):
        assert (queries[i].astype(np.float64) @ deq[i].T).max() < 0
    for i, ld in ((3, 17), (4, 65), (5, 2049)):
        assert ((queries[i].astype(np.float64) @ deq[i].T).argmax(axis=1) >= ld - ld % 16).all()
    arg = (q.astype(np.float64) @ deq[6].T).argmax(axis=1)
    assert arg[0] == 0 and arg[1] == 39
    x.add(docs)
    rows = np.arange(len(docs), dtype=np.int64)[:, None]
    got = x.score_rows(queries, rows)
    _check(got, queries, deq, rows, dim)
    assert (got[:3] < 0).all() and np.isfinite(got).all()
    pair = np.array([[6, 7]], np.int64)
    both = x.score_rows([q], pair)
    _check(both, [q], deq, pair, dim)
    assert both[0, 1] > both[0, 0]
    x.close()


def test_sentinels_and_bookkeeping():
    dim = 128
    rng = np.random.default_rng(21)
    docs = [CR.unit_f16(rng, n, dim) for n in (5, 0, 33, 16, 70)]
    deq = [Q.dequant(Q.quant(d)) for d in docs]
    q = CR.unit_f16(rng, 9, dim)
    x = _new(dim)
    assert x.stats() == {"rows": 0, "live": 0, "tokens": 0}
    assert np.isneginf(x.score_rows([q], np.array([[0, -1]], np.int64))).all()        # an empty index
    assert x.add(docs) == 0 and x.add([]) == 5
    assert x.stats() == {"rows": 5, "live": 5, "tokens": 124} and x.nbytes == 124 * dim
    rows = np.array([[0, 1, 2, 3, 4, -1, 5, 2]], np.int64)
    s0 = x.score_rows([q], rows)
    _check(s0, [q], deq, rows, dim)                                       # -inf: empty, -1, past the index
    assert np.isneginf(s0[0, [1, 5, 6]]).all() and np.isfinite(s0[0, [0, 2, 3, 4, 7]]).all()
    assert _u32(s0)[0, 2] == _u32(s0)[0, 7]                               # a duplicate scores the same
    assert np.isneginf(x.score_rows([q[:0]], rows)).all()                 # q_len = 0
    x.remove([2, 2])
    assert x.stats() == {"rows": 5, "live": 4, "tokens": 124} and x.nbytes == 124 * dim
    s1 = x.score_rows([q], rows)
    _check(s1, [q], deq, rows, dim, live=np.array([1, 1, 0, 1, 1], bool))
    assert np.isneginf(s1[0, [2, 7]]).all()
    np.testing.assert_array_equal(_u32(s1[0, [0, 3, 4]]), _u32(s0[0, [0, 3, 4]]))
    np.testing.assert_array_equal(_u32(x.get(2)), _u32(Q.stored(docs[2])))            # the tokens stay in the pool
    x.close()


@pytest.mark.parametrize("dim", [64, 1024])
def test_bit_identity_within_fp8(dim):
    import torch
    x = _index(dim)
    docs, deq, rq = _corpus(dim)
    rng = np.random.default_rng(7 + dim)
    q2 = CR.unit_f16(rng, 17, dim)
    nd = len(DOC_LENS)
    cand = np.arange(nd, nd + N_RANK, dtype=np.int64)
    rows = np.stack([cand, cand[::-1]])
    got = x.score_rows([rq, rq], rows)                                    # (2, 100), the same query twice
    _check(got, [rq, rq], deq, rows, dim)
    np.testing.assert_array_equal(_u32(got[1]), _u32(got[0, ::-1]))       # another b, reversed order
    pick = [0, 1, 31, 32, 33, 63, 64, 99]                                 # one call against calls with K = 1
    single = np.concatenate([x.score_rows([rq], cand[i:i + 1][None]) for i in pick], axis=1)
    np.testing.assert_array_equal(_u32(single[0]), _u32(got[0, pick]))
    # among other queries and candidates: (3, 7) with this query at b = 2
    mixed = np.array([[3, 4, 5, 6, 7, 8, 0], [11, 8, 10, 12, 8, 13, 1], cand[[5, 0, 99, 50, 5, 7, 33]]], np.int64)
    gm = x.score_rows([q2, q2[:3], rq], mixed)
    np.testing.assert_array_equal(_u32(gm[2]), _u32(got[0, [5, 0, 99, 50, 5, 7, 33]]))
    assert _u32(gm)[2, 0] == _u32(gm)[2, 4] and _u32(gm)[1, 1] == _u32(gm)[1, 4]
    _check(gm, [q2, q2[:3], rq], deq, mixed, dim)
    # host against device entry point, NaN in the unread query rows
    qs, pad, qlen = _queries(rng, 65, dim)
    r3 = np.array([[8, 7, 20, 3, -1], [1, 2, 30, 40, 8], [0, 5, 6, 7, 108]], np.int64)
    host = x.score_rows(pad, r3, q_len=qlen)
    dq = torch.as_tensor(pad).cuda().to(torch.float16)
    dev = x.score_rows_dev(dq, torch.as_tensor(qlen).cuda(), torch.as_tensor(r3).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_u32(dev.cpu().numpy()), _u32(host))
    _check(host, qs, deq, r3, dim)


# -- reranking ------------------------------------------------------------------------------------------------
def test_m3_rerank_on_an_fp8_index():
    from super_rag_amd.lexical import NativeImpactIndex
    from super_rag_amd.multivec import m3_rerank
    from super_rag_amd.store import NativeStore
    dim, hidden = 128, 128
    rng = np.random.default_rng(31)
    mv_d = [CR.unit_f16(rng, int(n), dim) for n in rng.integers(3, 40, 12)]
    mv_q = [CR.unit_f16(rng, n, dim) for n in (5, 16, 9)]
    dense_d = CR.unit(rng.standard_normal((12, hidden))).astype(F)
    dense_q = CR.unit(rng.standard_normal((3, hidden))).astype(F)
    sparse_d = [{int(t): float(w) for t, w in zip(rng.permutation(30)[:6], rng.uniform(0.1, 2.0, 6))} for _ in range(12)]
    sparse_q = [{int(t): float(w) for t, w in zip(rng.permutation(30)[:8], rng.uniform(0.1, 2.0, 8))} for _ in range(3)]
    mv = _new(dim)
    assert mv.add(mv_d) == 0
    store = NativeStore(hidden)
    store.add(dense_d)
    impact = NativeImpactIndex()
    impact.add(sparse_d)
    store.remove([9])
    rows = np.stack([np.arange(12), np.arange(12)[::-1], np.r_[np.arange(0, 12, 2), -1, 12, 3, 3, 5, 1]]).astype(np.int64)
    cos = store.score_rows(dense_q, rows)
    ms = mv.score_rows(mv_q, rows)
    sp = impact.score_rows(sparse_q, rows)
    _check(ms, mv_q, [Q.dequant(Q.quant(d)) for d in mv_d], rows, dim)
    assert (sp[np.isfinite(sp)] > 0).any()
    for imp, qs, spv, w in ((None, None, None, (1, 1, 1)), (impact, sparse_q, sp, (1, 1, 1)),
                            (impact, sparse_q, sp, (0.4, 0.2, 0.4))):
        score, r = m3_rerank(store, mv, dense_q, mv_q, rows, 5, impact=imp, q_sparse=qs, weights=w)
        want_s, want_r = CR.rerank(cos, ms, spv, rows, 5, w)
        np.testing.assert_array_equal(r, want_r)
        fin = np.isfinite(want_s)
        assert fin[:, 0].all() and np.isneginf(score[~fin]).all()
        assert (np.abs(score[fin].astype(np.float64) - want_s[fin]) <= np.spacing(np.abs(want_s[fin]))).all()
        assert not (r == 9).any() and (r >= 0).all()
    for o in (mv, store, impact):
        o.close()


# -- limits ---------------------------------------------------------------------------------------------------
def test_create_dtype_limits_and_info():
    import ctypes
    from super_rag_amd import _native as NV

    def code(fn, *a):
        with pytest.raises(NV.NativeError) as e:
            NV.call(fn, *a)
        return e.value.code

    h = ctypes.c_void_p()
    inv = NV.SR_ERR_INVALID
    for bad in (NV.SR_DTYPE_F32, 3, -1):
        assert code("sr_mv_create_dtype", 64, 0, bad, ctypes.byref(h)) == inv
    for dim in (63, 1088, 0):
        assert code("sr_mv_create_dtype", dim, 0, NV.SR_DTYPE_FP8_E4M3, ctypes.byref(h)) == inv
    assert code("sr_mv_create_dtype", 64, 0, NV.SR_DTYPE_FP8_E4M3, None) == inv
    assert code("sr_mv_info", None, None, None) == inv
    dt, nb = ctypes.c_int(-1), ctypes.c_int64(-1)
    toks = CR.unit_f16(np.random.default_rng(0), 3, 64)
    off = np.array([0, 3], np.int64)
    for create, args, want_dt, per_tok in (("sr_mv_create", (64, 0), NV.SR_DTYPE_F16, 128),
                                           ("sr_mv_create_dtype", (64, 0, NV.SR_DTYPE_F16), NV.SR_DTYPE_F16, 128),
                                           ("sr_mv_create_dtype", (64, 0, NV.SR_DTYPE_FP8_E4M3), NV.SR_DTYPE_FP8_E4M3, 64)):
        NV.call(create, *args, ctypes.byref(h))
        NV.call("sr_mv_info", h, ctypes.byref(dt), ctypes.byref(nb))
        assert (dt.value, nb.value) == (want_dt, 0)
        NV.call("sr_mv_add", h, NV.ptr(off), NV.ptr(toks), 1, None)
        NV.call("sr_mv_info", h, ctypes.byref(dt), ctypes.byref(nb))
        assert (dt.value, nb.value) == (want_dt, 3 * per_tok)
        NV.call("sr_mv_info", h, None, None)                              # both outputs are optional
        NV.load().sr_mv_destroy(h)
