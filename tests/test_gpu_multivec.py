"""GPU: the multi-vector index and the MaxSim kernel alone (multivec.hip, k_multivec.hip; sr_mv_*),
on synthetic unit vectors rounded to fp16.  The reference is fp64 on those fp16 values
(tests/colbert_ref.py).

Gate, derived and not tuned: fp16 x fp16 products are exact in fp32, so only the accumulation rounds:
|score - ref| <= (dim + Lq) 2^-23 max||q_i|| max||d_j|| (2^-23 and not 2^-24: the rounding of the
accumulate inside the MFMA is not documented).  Bit-identity (the same pair in another batch, another
position, another call, another way of adding the row) is checked on the uint32 views.
Measured on the MI355X: max |err| / gate 0.006 (dim 64), 0.003 (128), 0.001 (384), below 0.001 (1024).
"""
import functools

import numpy as np
import pytest

import colbert_ref as CR

pytestmark = pytest.mark.gpu

F = np.float32
DIMS = [64, 128, 384, 1024]
LQS = [1, 15, 16, 17, 33, 64, 65, 200, 512]
DOC_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 511, 2049]
N_RANK = 100


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _corpus(dim):
    """The mixed-length rows 0..9, then N_RANK ranking candidates built against a 32-token query."""
    rng = np.random.default_rng(1000 + dim)
    docs = [CR.unit_f16(rng, n, dim) for n in DOC_LENS]
    rq = CR.unit_f16(rng, 32, dim)
    alphas = np.linspace(0.0, 0.9, N_RANK)
    docs += [CR.mixed_doc(rng, rq, 32 + int(rng.integers(0, 24)), a) for a in rng.permutation(alphas)]
    return docs, rq


@functools.lru_cache(maxsize=None)
def _index(dim):
    from super_rag_amd.multivec import NativeMultiVectorIndex
    docs, _ = _corpus(dim)
    x = NativeMultiVectorIndex(dim)
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


def _check(got, qs, docs, rows, dim, live=None):
    ref = CR.maxsim_rows(qs, docs, rows, live)
    worst = 0.0
    for b in range(rows.shape[0]):
        for k in range(rows.shape[1]):
            if np.isneginf(ref[b, k]):
                assert np.isneginf(got[b, k]), (b, k, got[b, k])
                continue
            g = CR.gate(dim, len(qs[b]), qs[b], docs[rows[b, k]])
            err = abs(float(got[b, k]) - ref[b, k])
            worst = max(worst, err / g)
            assert err <= g, (dim, len(qs[b]), b, k, rows[b, k], got[b, k], ref[b, k], err / g)
    return worst


@pytest.mark.parametrize("dim", DIMS)
def test_maxsim_against_fp64_over_query_and_document_lengths(dim):
    x = _index(dim)
    docs, _ = _corpus(dim)
    rng = np.random.default_rng(dim)
    worst = 0.0
    for lq in LQS:
        qs, pad, qlen = _queries(rng, lq, dim)
        # (3, 7): every mixed-length row, a missing one and a row past the index, over the queries
        rows = np.array([[9, 0, 1, 2, -1, 3, 4], [5, 6, 7, 8, 9, len(docs), 2], [8, 9, 4, 6, 5, 1, 7]], np.int64)
        got = x.score_rows(pad, rows, q_len=qlen)
        worst = max(worst, _check(got, qs, docs, rows, dim))
        # (1, 1)
        one = x.score_rows(pad[:1], rows[:1, :1], q_len=qlen[:1])
        np.testing.assert_array_equal(_u32(one), _u32(got[:1, :1]))
    print(f"maxsim dim {dim}: max |err| / gate {worst:.3f}")


@pytest.mark.parametrize("dim", DIMS)
def test_ranking_of_100_candidates_and_bit_identity(dim):
    x = _index(dim)
    docs, rq = _corpus(dim)
    rng = np.random.default_rng(7 + dim)
    q2 = CR.unit_f16(rng, 17, dim)
    cand = np.arange(len(DOC_LENS), len(DOC_LENS) + N_RANK, dtype=np.int64)
    rows = np.stack([cand, cand[::-1]])
    got = x.score_rows([rq, rq], rows)                                   # (2, 100), the same query twice
    worst = _check(got, [rq, rq], docs, rows, dim)
    ref = CR.maxsim_rows([rq], docs, cand[None])[0]
    assert ref.min() < 0.45 and ref.max() > 0.85, (ref.min(), ref.max())
    # the device's ranking is valid under the gate, no pair excluded
    g = CR.gate(dim, 32, rq, np.concatenate([docs[r] for r in cand], axis=0))     # max ||d_j|| of the candidates
    order = np.lexsort((cand, -got[0].astype(np.float64)))
    r = ref[order]
    assert (r[:-1] >= r[1:] - 2 * g).all()
    # the same pair at another b and in reversed candidate order
    np.testing.assert_array_equal(_u32(got[1]), _u32(got[0, ::-1]))
    # one call with K = 100 against 100 calls with K = 1
    single = np.concatenate([x.score_rows([rq], cand[i:i + 1][None]) for i in range(N_RANK)], axis=1)
    np.testing.assert_array_equal(_u32(single[0]), _u32(got[0]))
    # among other queries and candidates: (3, 7) with this query at b = 2
    mixed = np.array([[3, 4, 5, 6, 7, 8, 9], [11, 9, 10, 12, 9, 13, 1], cand[[5, 0, 99, 50, 5, 7, 33]]], np.int64)
    gm = x.score_rows([q2, q2[:3], rq], mixed)
    np.testing.assert_array_equal(_u32(gm[2]), _u32(got[0, [5, 0, 99, 50, 5, 7, 33]]))
    assert gm[2, 0] == gm[2, 4] and gm[1, 1] == gm[1, 4]                  # duplicates score equal
    worst = max(worst, _check(gm, [q2, q2[:3], rq], docs, mixed, dim))
    print(f"maxsim ranking dim {dim}: max |err| / gate {worst:.3f}, ref scores {ref.min():.2f} .. {ref.max():.2f}")


@pytest.mark.parametrize("dim", [64, 1024])
def test_host_and_device_entry_points_agree_in_bits(dim):
    import torch
    x = _index(dim)
    docs, rq = _corpus(dim)
    rng = np.random.default_rng(3)
    qs, pad, qlen = _queries(rng, 65, dim)
    rows = np.array([[9, 8, 20, 3, -1], [1, 2, 30, 40, 9], [0, 5, 6, 7, 109]], np.int64)
    host = x.score_rows(pad, rows, q_len=qlen)
    dq = torch.as_tensor(pad).cuda().to(torch.float16)                    # (NaN rows stay NaN)
    dev = x.score_rows_dev(dq, torch.as_tensor(qlen).cuda(), torch.as_tensor(rows).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_u32(dev.cpu().numpy()), _u32(host))
    _check(host, qs, docs, rows, dim)


@pytest.mark.parametrize("dim", [64, 384])
def test_adversarial_cases(dim):
    from super_rag_amd.multivec import NativeMultiVectorIndex
    rng = np.random.default_rng(11 + dim)
    x = NativeMultiVectorIndex(dim)
    docs, queries, rows = [], [], []
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
    x.add(docs)
    rows = np.arange(len(docs), dtype=np.int64)[:, None]
    got = x.score_rows(queries, rows)
    _check(got, queries, docs, rows, dim)
    assert (got[:3] < 0).all() and np.isfinite(got).all()
    both = x.score_rows([q], np.array([[6, 7]], np.int64))
    _check(both, [q], docs, np.array([[6, 7]], np.int64), dim)
    assert both[0, 1] > both[0, 0]
    x.close()


def test_sentinels_bookkeeping_growth_and_the_two_ways_to_add():
    import torch
    from super_rag_amd.multivec import NativeMultiVectorIndex
    dim = 128
    rng = np.random.default_rng(21)
    docs = [CR.unit_f16(rng, n, dim) for n in (5, 0, 33, 16, 70)]
    q = CR.unit_f16(rng, 9, dim)
    x = NativeMultiVectorIndex(dim)
    assert x.stats() == {"rows": 0, "live": 0, "tokens": 0}
    assert np.isneginf(x.score_rows([q], np.array([[0, -1]], np.int64))).all()     # an empty index
    assert x.add(docs) == 0 and x.add([]) == 5
    assert x.stats() == {"rows": 5, "live": 5, "tokens": 124}
    for i, d in enumerate(docs):
        np.testing.assert_array_equal(x.get(i), d)                        # the fp16 values exactly
    rows = np.array([[0, 1, 2, 3, 4, -1, 5, 2]], np.int64)
    s0 = x.score_rows([q], rows)
    assert np.isneginf(s0[0, [1, 5, 6]]).all() and np.isfinite(s0[0, [0, 2, 3, 4, 7]]).all()
    assert s0[0, 2] == s0[0, 7]
    assert np.isneginf(x.score_rows([q[:0]], rows)).all()                  # q_len = 0
    # further adds that make the pool and the row arrays grow: scores unchanged
    more = [CR.unit_f16(rng, 40, dim) for _ in range(300)]
    assert x.add(more) == 5
    assert x.stats() == {"rows": 305, "live": 305, "tokens": 124 + 300 * 40}
    np.testing.assert_array_equal(_u32(x.score_rows([q], rows)[0, [0, 2, 3, 4, 7]]), _u32(s0[0, [0, 2, 3, 4, 7]]))
    np.testing.assert_array_equal(x.get(4), docs[4])
    x.remove([2, 2, 304])
    assert x.stats() == {"rows": 305, "live": 303, "tokens": 124 + 300 * 40}
    s1 = x.score_rows([q], rows)
    assert np.isneginf(s1[0, [2, 7]]).all()
    np.testing.assert_array_equal(_u32(s1[0, [0, 3, 4]]), _u32(s0[0, [0, 3, 4]]))
    # add_dev on the fp16 values, in bulk and row by row, against add on fp32 host input
    ld_tok = 72
    pad = np.full((5, ld_tok, dim), 7.0, np.float16)
    for i, d in enumerate(docs):
        pad[i, :d.shape[0]] = d.astype(np.float16)
    lens = np.asarray([d.shape[0] for d in docs], np.int32)
    dv, dl = torch.as_tensor(pad).cuda(), torch.as_tensor(lens).cuda()
    y, z = NativeMultiVectorIndex(dim), NativeMultiVectorIndex(dim)
    assert y.add_dev(dv, dl) == 0
    for i in range(5):
        assert z.add_dev(dv[i:i + 1].contiguous(), dl[i:i + 1].contiguous()) == i
    r5 = np.array([[0, 1, 2, 3, 4]], np.int64)
    for other in (y, z):
        assert other.stats() == {"rows": 5, "live": 5, "tokens": 124}
        for i, d in enumerate(docs):
            np.testing.assert_array_equal(other.get(i), d)
        np.testing.assert_array_equal(_u32(other.score_rows([q], r5)), _u32(s0[:, :5]))
        other.close()
    x.close()


def test_limits_and_rejections():
    import ctypes
    from super_rag_amd import _native as NV
    from super_rag_amd.multivec import NativeMultiVectorIndex

    def code(fn, *a):
        with pytest.raises(NV.NativeError) as e:
            NV.call(fn, *a)
        return e.value.code

    h = ctypes.c_void_p()
    for dim in (63, 1088, 0):
        assert code("sr_mv_create", dim, 0, ctypes.byref(h)) == NV.SR_ERR_INVALID
    assert code("sr_mv_create", 64, 0, None) == NV.SR_ERR_INVALID
    x = NativeMultiVectorIndex(64)
    x.add([CR.unit_f16(np.random.default_rng(0), 3, 64)])
    q = np.zeros((1, 513, 64), F)
    out = np.zeros((1, 1025), F)
    rows = np.zeros((1, 1025), np.int64)
    p = NV.ptr
    ok_len, long_len = np.array([4], np.int32), np.array([513], np.int32)
    inv = NV.SR_ERR_INVALID
    assert code("sr_mv_score_rows", x._h, p(q), p(ok_len), 1, 8, p(rows), 1025, p(out)) == inv      # K
    assert code("sr_mv_score_rows", x._h, p(q), p(ok_len), 1, 8, p(rows), 0, p(out)) == inv
    assert code("sr_mv_score_rows", x._h, p(q), p(long_len), 1, 512, p(rows), 1, p(out)) == inv     # q_len 513
    assert code("sr_mv_score_rows", x._h, p(q), p(long_len), 1, 513, p(rows), 1, p(out)) == inv     # also with room
    assert code("sr_mv_score_rows", x._h, p(q), p(ok_len), 1, 0, p(rows), 1, p(out)) == inv
    assert code("sr_mv_score_rows", x._h, p(q), p(ok_len), 1, 3, p(rows), 1, p(out)) == inv         # ld_q < q_len
    assert code("sr_mv_score_rows", x._h, p(q), np.array([-1], np.int32).ctypes.data, 1, 8, p(rows), 1, p(out)) == inv
    assert code("sr_mv_score_rows", x._h, p(q), p(ok_len), -1, 8, p(rows), 1, p(out)) == inv
    for bad in ((None, p(ok_len), p(rows), p(out)), (p(q), None, p(rows), p(out)),
                (p(q), p(ok_len), None, p(out)), (p(q), p(ok_len), p(rows), None)):
        assert code("sr_mv_score_rows", x._h, bad[0], bad[1], 1, 8, bad[2], 1, bad[3]) == inv
        assert code("sr_mv_score_rows_dev", x._h, bad[0], bad[1], 1, 8, bad[2], 1, bad[3], None) == inv
    assert code("sr_mv_score_rows", None, p(q), p(ok_len), 1, 8, p(rows), 1, p(out)) == inv
    assert code("sr_mv_score_rows_dev", x._h, p(q), p(ok_len), 1, 8, p(rows), 1025, p(out), None) == inv
    assert code("sr_mv_score_rows_dev", x._h, p(q), p(ok_len), 1, 0, p(rows), 1, p(out), None) == inv
    NV.call("sr_mv_score_rows", x._h, None, None, 0, 8, None, 1, None)                              # B == 0
    off = np.array([0, 2], np.int64)
    assert code("sr_mv_add", x._h, None, p(q), 1, None) == inv
    assert code("sr_mv_add", x._h, p(off), None, 1, None) == inv
    assert code("sr_mv_add", x._h, p(np.array([1, 2], np.int64)), p(q), 1, None) == inv
    assert code("sr_mv_add", x._h, p(np.array([0, 2, 1], np.int64)), p(q), 2, None) == inv
    assert code("sr_mv_add_dev", x._h, None, None, 1, 8, None, None) == inv
    assert code("sr_mv_remove", x._h, p(np.array([1], np.int64)), 1) == inv                         # past the index
    assert code("sr_mv_remove", x._h, None, 1) == inv
    assert code("sr_mv_get", x._h, 1, p(out), 8, None) == inv
    assert code("sr_mv_get", x._h, 0, None, 8, None) == inv
    assert x.stats() == {"rows": 1, "live": 1, "tokens": 3}
    x.close()
