"""GPU: the multi-vector index's whole-corpus search (sr_mv_search / sr_mv_search_dev; k_mvscan.hip,
sr_mv_plan.h), fp16 and fp8 pools.

Primary oracle, the device itself: sr_mv_score_rows over every row (calls of K <= 1024), sorted on the
host by (score desc, row asc) and padded (mv_search_ref.topk).  The search must equal it exactly: the
rows, and the scores on their uint32 views.  Independent check: the fp64 reference of the returned
rows under colbert_ref.gate, the bound test_gpu_multivec.py derives ((dim + Lq) 2^-23 max||q|| max||d||);
no other tolerance is used here.
Measured on the MI355X: every comparison with the oracle exact; fp64 check max |err| / gate 0.007
(dim 64), 0.003 (128), 0.001 (384), 0.001 (1024), fp8 no higher."""
import functools

import numpy as np
import pytest

import colbert_ref as CR
import mv_search_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
DIMS = [64, 128, 384, 1024]
DTYPES = ["fp16", "fp8"]
DOC_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 511, 2049]
N_MIXED = 100
LQ_BATCH = [200, 1, 65, 17, 0]


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _new(dim, dtype="fp16"):
    from super_rag_amd.multivec import NativeMultiVectorIndex
    return NativeMultiVectorIndex(dim, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _corpus(dim):
    """150 rows: five rounds of the mixed lengths 0 .. 2049, then N_MIXED rows built against a 32-token
    query (MaxSim from the noise level up to about 0.9)."""
    rng = np.random.default_rng(2000 + dim)
    docs = [CR.unit_f16(rng, DOC_LENS[i % len(DOC_LENS)], dim) for i in range(50)]
    rq = CR.unit_f16(rng, 32, dim)
    alphas = np.linspace(0.0, 0.9, N_MIXED)
    docs += [CR.mixed_doc(rng, rq, 32 + int(rng.integers(0, 24)), a) for a in rng.permutation(alphas)]
    return docs, rq


@functools.lru_cache(maxsize=None)
def _index(dim, dtype):
    x = _new(dim, dtype)
    assert x.add(_corpus(dim)[0]) == 0
    return x


@functools.lru_cache(maxsize=None)
def _batch(dim, lens=tuple(LQ_BATCH)):
    """Queries of the given lengths in one padded array, NaN in every row at and past q_len."""
    rng = np.random.default_rng(77 + dim + len(lens))
    qs = [CR.unit_f16(rng, n, dim) for n in lens]
    pad = np.full((len(lens), max(lens) + 3, dim), np.nan, F)
    for b, q in enumerate(qs):
        pad[b, :q.shape[0]] = q
    return qs, pad, np.asarray(lens, np.int32)


def _all_scores(x, pad, qlen):
    """sr_mv_score_rows of every (query, row) pair -> fp32 [B, n_rows], in calls of K <= 1024."""
    n = x.stats()["rows"]
    B = pad.shape[0]
    out = np.full((B, n), -np.inf, F)
    for r0 in range(0, n, 1024):
        rows = np.tile(np.arange(r0, min(n, r0 + 1024), dtype=np.int64), (B, 1))
        out[:, r0:r0 + rows.shape[1]] = x.score_rows(pad, rows, q_len=qlen)
    return out


def _oracle(x, pad, qlen, k, allow=None, row_offset=0):
    s = _all_scores(x, pad, qlen)
    if allow is not None:
        s[:, np.asarray(allow).reshape(-1) == 0] = -np.inf
    return R.topk(s, k, row_offset)


@functools.lru_cache(maxsize=None)
def _cached_scores(dim, dtype, lens):
    _, pad, qlen = _batch(dim, lens)
    s = _all_scores(_index(dim, dtype), pad, qlen)
    s.setflags(write=False)
    return s


def _same(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(_u32(got[0]), _u32(want[0]))


# -- the oracle: the device's own pair scores -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_search_equals_the_sorted_pair_scores(dim, dtype):
    from super_rag_amd.multivec import search_group_queries
    x = _index(dim, dtype)
    n = x.stats()["rows"]
    Q = search_group_queries(dim)
    eligible = sum(1 for d in _corpus(dim)[0] if len(d))
    assert eligible < 200 and n == 150
    for lens in (tuple(LQ_BATCH), (33,), tuple([40, 7, 64, 3, 90][:Q + 1])):
        _, pad, qlen = _batch(dim, lens)
        s = _cached_scores(dim, dtype, lens)
        for k in (1, 10, 200):
            got = x.search(pad, k, q_len=qlen)
            _same(got, R.topk(s, k))
            for b, lq in enumerate(lens):
                m = min(k, eligible) if lq else 0
                assert (got[1][b, :m] >= 0).all() and (got[1][b, m:] == -1).all()
                assert np.isfinite(got[0][b, :m]).all() and np.isneginf(got[0][b, m:]).all()
    # the list-of-arrays convention gives the same bits
    qs, pad, qlen = _batch(dim)
    _same(x.search(qs, 10), x.search(pad, 10, q_len=qlen))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_result_does_not_depend_on_slab_rows(dim, dtype):
    x = _index(dim, dtype)
    _, pad, qlen = _batch(dim)
    want = R.topk(_cached_scores(dim, dtype, tuple(LQ_BATCH)), 20)
    for slab in (7, 64, 0, 149, 150, 151):
        _same(x.search(pad, 20, q_len=qlen, slab_rows=slab), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_row_slabs_on_a_40_row_index(dtype):
    dim = 128
    x = _new(dim, dtype)
    x.add(_corpus(dim)[0][:40])
    _, pad, qlen = _batch(dim)
    want = _oracle(x, pad, qlen, 50)
    for slab in (1, 0):
        _same(x.search(pad, 50, q_len=qlen, slab_rows=slab), want)
    x.close()


# -- ties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_identical_documents_come_out_adjacent_in_row_order(dtype):
    dim = 64
    rng = np.random.default_rng(5)
    q = CR.unit_f16(rng, 20, dim)
    docs = [CR.unit_f16(rng, int(n), dim) for n in rng.integers(10, 30, 300)]
    twin = CR.mixed_doc(rng, q, 40, 0.95)
    at = [3, 150, 290]                      # about 3000 tokens apart: other windows, and other slabs below
    for r in at:
        docs[r] = twin
    x = _new(dim, dtype)
    x.add(docs)
    pad, qlen = q[None].astype(F), np.asarray([20], np.int32)
    s = _all_scores(x, pad, qlen)
    assert _u32(s[0, at[0]]) == _u32(s[0, at[1]]) == _u32(s[0, at[2]]) and s[0].argmax() in at
    for slab in (0, 64, 100):
        for k, want in ((1, at[:1]), (2, at[:2]), (3, at), (5, None)):
            got = x.search(pad, k, q_len=qlen, slab_rows=slab)
            _same(got, R.topk(s, k))
            assert got[1][0, :min(k, 3)].tolist() == (want if want is not None else at)
    x.close()


# -- eligibility ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_removed_rows_allow_masks_and_empty_rows(dtype):
    import torch
    dim = 128
    docs = _corpus(dim)[0]
    n = len(docs)
    x = _new(dim, dtype)
    # an empty index
    _, pad, qlen = _batch(dim)
    s, r = x.search(pad, 4, q_len=qlen)
    assert np.isneginf(s).all() and (r == -1).all() and s.shape == (5, 4)
    x.add(docs)
    allow = (np.arange(n) % 4 != 1)
    dq = torch.as_tensor(pad).cuda().to(torch.float16)
    dlen = torch.as_tensor(qlen).cuda()

    def check(al):
        for k in (10, 200):
            want = _oracle(x, pad, qlen, k, al)
            got = x.search(pad, k, q_len=qlen, allow=al, slab_rows=64)
            _same(got, want)
            empty = [i for i, d in enumerate(docs) if len(d) == 0]
            assert not np.isin(got[1], empty).any()            # a row with 0 tokens is never reported
            # the device entry point: the same bits, row_offset on every real row, -1 kept
            dal = None if al is None else torch.as_tensor(np.asarray(al, np.uint8)).cuda()
            ds, dr = x.search_dev(dq, dlen, k, allow=dal, row_offset=1000, slab_rows=0)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_u32(ds.cpu().numpy()), _u32(want[0]))
            np.testing.assert_array_equal(dr.cpu().numpy(), np.where(want[1] >= 0, want[1] + 1000, -1))
        return got

    check(None)
    got = check(allow)
    assert not np.isin(got[1], np.nonzero(~allow)[0]).any()
    dead = np.arange(0, n, 3)
    x.remove(dead)                                             # a third of the rows
    got = check(None)
    assert not np.isin(got[1], dead).any()
    got = check(allow)                                         # both together
    assert not np.isin(got[1], dead).any() and not np.isin(got[1], np.nonzero(~allow)[0]).any()
    s, r = x.search(pad, 3, q_len=qlen, allow=np.zeros(n, bool))
    assert np.isneginf(s).all() and (r == -1).all()            # nothing allowed
    x.remove(np.arange(n))                                     # all rows removed
    s, r = x.search(pad, 3, q_len=qlen)
    assert np.isneginf(s).all() and (r == -1).all()
    ds, dr = x.search_dev(dq, dlen, 3, row_offset=5)
    torch.cuda.synchronize()
    assert torch.isneginf(ds).all() and (dr == -1).all()
    x.close()


def test_k_1024_over_1300_short_rows():
    dim = 64
    rng = np.random.default_rng(9)
    docs = [CR.unit_f16(rng, int(n), dim) for n in rng.integers(1, 21, 1300)]
    x = _new(dim)
    x.add(docs)
    qs = [CR.unit_f16(rng, n, dim) for n in (12, 70)]
    pad, qlen = _pad(qs, dim)
    want = _oracle(x, pad, qlen, 1024)
    assert (want[1] >= 0).all()
    for slab in (0, 500):
        _same(x.search(pad, 1024, q_len=qlen, slab_rows=slab), want)
    x.close()


def _pad(qs, dim):
    from super_rag_amd.multivec import pad_queries
    return pad_queries(qs, dim)


# -- the fp64 reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_returned_rows_against_fp64_under_the_maxsim_gate(dim, dtype):
    x = _index(dim, dtype)
    docs, rq = _corpus(dim)
    mixed = range(50, 50 + N_MIXED)
    stored = {i: x.get(i) for i in mixed} if dtype == "fp8" else dict(enumerate(docs))   # what the pool holds
    allow = np.arange(len(docs)) >= 50                                            # the mixed rows only
    s, r = x.search([rq], N_MIXED, allow=allow)
    assert sorted(r[0].tolist()) == list(range(50, 50 + N_MIXED))
    ref = np.array([CR.maxsim(rq, stored[i]) for i in r[0]])
    assert ref.max() > 0.8 and ref.min() < 0.5, (ref.min(), ref.max())
    g = CR.gate(dim, 32, rq, np.concatenate([stored[i] for i in mixed], axis=0))
    err = np.abs(s[0].astype(np.float64) - ref)
    print(f"mv search dim {dim} {dtype}: max |err| / gate {err.max() / g:.3f}")
    assert (err <= g).all()                                   # every returned score within one gate
    assert (ref[:-1] >= ref[1:] - 2 * g).all()                # the order is valid within twice the gate


# -- lifecycle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_search_after_growth_compaction_and_reload(dtype, tmp_path):
    from super_rag_amd.multivec import NativeMultiVectorIndex
    dim = 128
    docs = _corpus(dim)[0]
    _, pad, qlen = _batch(dim)
    x = _new(dim, dtype)
    x.add(docs[:20])
    _same(x.search(pad, 30, q_len=qlen), _oracle(x, pad, qlen, 30))
    x.add(docs[20:])                                           # the pool and the row arrays grow
    before = _oracle(x, pad, qlen, 30)
    _same(x.search(pad, 30, q_len=qlen, slab_rows=33), before)
    dead = np.arange(1, len(docs), 4)
    x.remove(dead)
    m = x.compact()
    want = _oracle(x, pad, qlen, 30)
    _same(x.search(pad, 30, q_len=qlen, slab_rows=33), want)
    # the kept rows keep their bits under their new ids
    old = _oracle_ids(before, m)
    assert set(want[1][0][want[1][0] >= 0]) >= set(old[0][old[0] >= 0][:5])
    p = str(tmp_path / "x.srmv")
    x.save(p)
    y = NativeMultiVectorIndex.load(p)
    _same(y.search(pad, 30, q_len=qlen), want)
    for o in (x, y):
        o.close()


def _oracle_ids(res, old_to_new):
    rows = res[1]
    return np.where(rows >= 0, np.asarray(old_to_new)[np.maximum(rows, 0)], -1)


# -- m3_search --------------------------------------------------------------------------------------------------
def test_m3_search_first_stage():
    from super_rag_amd.multivec import m3_rerank, m3_search
    from super_rag_amd.store import NativeStore
    dim, hidden, n = 128, 64, 60
    rng = np.random.default_rng(41)
    mv_d = [CR.unit_f16(rng, int(l), dim) for l in rng.integers(0, 40, n)]
    mv_q = [CR.unit_f16(rng, l, dim) for l in (5, 16, 9)]
    dense_d = CR.unit(rng.standard_normal((n, hidden))).astype(F)
    dense_q = CR.unit(rng.standard_normal((3, hidden))).astype(F)
    mv = _new(dim)
    mv.add(mv_d)
    store = NativeStore(hidden)
    store.add(dense_d)
    store.remove([7])
    mv.remove([7])
    allow = np.arange(n) % 5 != 2
    for al in (None, allow):
        _, cand = mv.search(mv_q, 12, allow=al)
        want = m3_rerank(store, mv, dense_q, mv_q, cand, 4)
        got = m3_search(store, mv, dense_q, mv_q, 4, k_cand=12, allow=al, first_stage="multivec")
        _same(got, want)
        assert not (got[1] == 7).any()
        if al is not None:
            assert not np.isin(got[1], np.nonzero(~allow)[0]).any()
    _same(m3_search(store, mv, dense_q, mv_q, 4, k_cand=12, first_stage="dense"),
          m3_search(store, mv, dense_q, mv_q, 4, k_cand=12))
    with pytest.raises(ValueError, match="nonsense"):
        m3_search(store, mv, dense_q, mv_q, 4, first_stage="nonsense")
    for o in (mv, store):
        o.close()


# -- limits -----------------------------------------------------------------------------------------------------
def test_limits_and_rejections():
    import torch
    from super_rag_amd import _native as NV
    dim = 64
    x = _new(dim)
    x.add(_corpus(dim)[0][:12])
    q = np.zeros((2, 4, dim), F)
    qlen = np.array([4, 2], np.int32)
    s, r = np.empty((2, 3), F), np.empty((2, 3), np.int64)
    P = NV.ptr

    def code(fn, *a):
        with pytest.raises(NV.NativeError) as e:
            NV.call(fn, *a)
        return e.value.code

    def host(B=2, ld_q=4, k=3, slab=0, q_=q, l_=qlen, s_=s, r_=r, h=x._h):
        return code("sr_mv_search", h, P(q_), P(l_), B, ld_q, k, None, slab, P(s_), P(r_))

    for kw in (dict(k=0), dict(k=NV.SR_MAX_TOPK + 1), dict(k=-1), dict(ld_q=0), dict(B=-1), dict(slab=-1),
               dict(q_=None), dict(l_=None), dict(s_=None), dict(r_=None), dict(h=None),
               dict(l_=np.array([5, 2], np.int32)), dict(l_=np.array([4, -1], np.int32)),
               dict(l_=np.array([513, 2], np.int32), ld_q=600)):
        assert host(**kw) == NV.SR_ERR_INVALID, kw
    NV.call("sr_mv_search", x._h, P(q), P(qlen), 0, 4, 3, None, 0, P(s), P(r))        # B == 0: a no-op
    NV.call("sr_mv_search", x._h, None, None, 0, 4, 3, None, 0, None, None)
    dq = torch.zeros((2, 4, dim), dtype=torch.float16, device="cuda")
    dl = torch.as_tensor(qlen).cuda()
    ds = torch.empty((2, 3), dtype=torch.float32, device="cuda")
    dr = torch.empty((2, 3), dtype=torch.int64, device="cuda")

    def dev(B=2, ld_q=4, k=3, slab=0, off=0, q_=dq, l_=dl, s_=ds, r_=dr, h=x._h):
        return code("sr_mv_search_dev", h, P(q_), P(l_), B, ld_q, k, None, slab, off, P(s_), P(r_), None)

    for kw in (dict(k=0), dict(k=NV.SR_MAX_TOPK + 1), dict(ld_q=0), dict(B=-1), dict(slab=-1), dict(off=-1),
               dict(q_=None), dict(l_=None), dict(s_=None), dict(r_=None), dict(h=None)):
        assert dev(**kw) == NV.SR_ERR_INVALID, kw
    NV.call("sr_mv_search_dev", x._h, None, None, 0, 4, 3, None, 0, 0, None, None, None)
    # the Python surface: tensor checks and the allow length, before the call
    with pytest.raises(ValueError):
        x.search_dev(dq.float(), dl, 3)
    with pytest.raises(ValueError):
        x.search_dev(dq, dl.cpu(), 3)
    with pytest.raises(ValueError, match="one entry per row"):
        x.search_dev(dq, dl, 3, allow=torch.ones(11, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="one entry per row"):
        x.search([q[0]], 3, allow=np.ones(13, np.uint8))
    with pytest.raises(ValueError):
        x.search_dev(dq, dl, 3, out=(ds, dr[:, :2]))
    # k = SR_MAX_TOPK itself and the device clamp of q_len are accepted
    out = x.search_dev(dq, torch.tensor([9, 600], dtype=torch.int32, device="cuda"), NV.SR_MAX_TOPK)
    torch.cuda.synchronize()
    assert out[0].shape == (2, NV.SR_MAX_TOPK)
    x.close()
