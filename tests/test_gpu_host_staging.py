"""GPU: a host entry point is upload + the _dev path + download, so its result equals the _dev entry
point's bit for bit when the latter is fed torch device tensors holding the same values.

The host entry points stage their arguments and results in one device buffer carved into typed parts
(csrc/sr_carve.h).  The shapes here make every part's element count odd (dim 20, B 3, k 5, fetch_k
21, lists of 1 / 7 / 33 rows, ka 5 / kb 7), the shapes at which a layout that packs an 8-byte part
directly behind 4-byte ones puts it on an address that is only 4-byte aligned.  No tolerance exists
in this file except where a comparison is delegated to an existing test's own check (subset search,
the store-less MMR): everything else is equality of bits.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, N, B, K, FETCH = 20, 300, 3, 5, 21
DEAD = np.arange(3, N, 10)                     # a tenth of the rows, removed
QUERIES = [[1], [2, 3], [4, 5, 4]]             # 1, 2 and 3 BM25 terms
VOCAB = 11
SCANS = ["fp16", "fp8"]


def _rows_and_queries():
    rng = np.random.default_rng(20)
    cent = rng.standard_normal((9, DIM))
    x = (cent[np.arange(N) % 9] + 0.4 * rng.standard_normal((N, DIM))).astype(np.float32)
    q = (cent[[0, 4, 8]] + 0.5 * rng.standard_normal((B, DIM))).astype(np.float32)
    return x, q


@functools.lru_cache(maxsize=None)
def _store(scan):
    """A store the tests only read: 300 rows of dim 20, 30 of them removed."""
    from super_rag_amd.store import NativeStore
    x, q = _rows_and_queries()
    s = NativeStore(DIM, device=0)
    s.add(x)
    s.remove(DEAD)
    s.set_scan_dtype(scan)
    return s, q


@functools.lru_cache(maxsize=None)
def _lex():
    """A BM25 index over the same 300 rows (1 to 4 distinct terms of 11 each), the same rows removed."""
    from super_rag_amd.lexical import NativeLexIndex
    rng = np.random.default_rng(21)
    docs = [rng.integers(0, VOCAB, rng.integers(1, 6)).tolist() for _ in range(N)]
    lex = NativeLexIndex(device=0)
    lex.add(docs)
    lex.remove(DEAD)
    return lex


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _same(got, want, what=""):
    """Equal dtype, shape and bytes (so -inf, signed zeros and NaN payloads count too)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, got, want)


def _sim_or_ninf(sim, rows):
    return np.where(rows >= 0, sim, -np.inf).astype(np.float32)


def _dist(sim, rows):
    return np.where(rows >= 0, np.float32(1.0) - sim, np.float32(np.inf)).astype(np.float32)


# -- the store ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("k", [K, 275])             # 275 > the 270 live rows: five missing per query
def test_search_sim_and_search_equal_search_dev(scan, k):
    s, q = _store(scan)
    sim_d, rows_d = _host(*s.search_dev(_dev(q), k))
    assert ((rows_d >= 0).sum(axis=1) == min(k, N - len(DEAD))).all()
    assert not np.isin(rows_d, DEAD).any()
    sim_h, rows_h = s.search_sim(q, k)
    _same(rows_h, rows_d, "search_sim rows")
    _same(sim_h, _sim_or_ninf(sim_d, rows_d), "search_sim sims")
    dist_h, rows_h = s.search(q, k)
    _same(rows_h, rows_d, "search rows")
    _same(dist_h, _dist(sim_d, rows_d), "search distances")


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("mode", ["onepass", "greedy"])
def test_search_mmr_equals_search_dev_then_mmr_dev(scan, mode):
    s, q = _store(scan)
    sim, cand = s.search_dev(_dev(q), FETCH)
    sc_d, sim_d, rows_d = _host(*s.mmr_dev(cand, sim, K, lam=0.4, mode=mode))
    sc_h, dist_h, rows_h = s.search_mmr(q, K, FETCH, lam=0.4, mode=mode)
    assert (rows_d >= 0).all()
    _same(rows_h, rows_d, "mmr rows")
    _same(sc_h, sc_d, "mmr scores")
    _same(dist_h, _dist(sim_d, rows_d), "mmr distances")


@pytest.mark.parametrize("scan", SCANS)
def test_score_rows_equals_score_rows_dev(scan):
    s, q = _store(scan)
    rows = np.array([[0, 299, 3, -1, 150, 300, 7],          # 3: removed; -1, 300, 10**6: no row
                     [13, 1, 2, 10 ** 6, 298, 297, 23],
                     [5, 5, 299, 0, 33, 43, 44]], np.int64)
    got = s.score_rows(q, rows)
    want, = _host(s.score_rows_dev(_dev(q), _dev(rows)))
    assert np.isneginf(got[rows == 3]).all() and np.isfinite(got[0, 0])
    _same(got, want, "score_rows")


@pytest.mark.parametrize("scan", SCANS)
def test_search_grouped_equals_search_dev_then_group_dev_when_round_0_completes(scan):
    s, q = _store(scan)
    group = (np.arange(N) // 2).astype(np.int32)             # pairs: the top 21 hold >= 11 groups
    sim, cand = s.search_dev(_dev(q), FETCH)
    sim_d, rows_d, grp_d, comp = _host(*s.group_dev(cand, sim, K, group, group_size=1))
    assert (comp == 1).all(), "round 0 was meant to complete for every query"
    sim_h, rows_h, grp_h = s.search_grouped(q, K, group, group_size=1, fetch_k=FETCH, sim=True)
    _same(rows_h, rows_d, "grouped rows")
    _same(grp_h, grp_d, "grouped groups")
    _same(sim_h, _sim_or_ninf(sim_d, rows_d), "grouped sims")


@pytest.mark.parametrize("scan", SCANS)
def test_search_grouped_continuation_equals_the_walk_over_the_full_list(scan):
    from super_rag_amd.store import group_walk
    s, q = _store(scan)
    group = (np.arange(N) % 7).astype(np.int32)              # 7 groups, 3 rows of each of 5 wanted
    sim, cand = s.search_dev(_dev(q), FETCH)
    comp, = _host(s.group_dev(cand, sim, K, group, group_size=3)[3])
    assert (comp == 0).any(), "this group array was meant to force a continuation"
    sim_h, rows_h, grp_h = s.search_grouped(q, K, group, group_size=3, fetch_k=FETCH, sim=True)
    full_sim, full_rows = s.search_sim(q, N)
    for b in range(B):
        w_sim, w_rows, w_grp = group_walk(full_sim[b], full_rows[b], group, K, 3)
        _same(rows_h[b], w_rows, f"walk rows {b}")
        _same(grp_h[b], w_grp, f"walk groups {b}")
        _same(sim_h[b], w_sim.astype(np.float32), f"walk sims {b}")   # fp32 -> fp64 -> fp32: exact


@pytest.mark.parametrize("scan", SCANS)
def test_search_subset_with_odd_length_lists(scan):
    import test_gpu_subset as SUB
    s, q = _store(scan)
    stored = s.get(np.arange(N)).astype(np.float64)
    live = np.ones(N, bool)
    live[DEAD] = False
    lists = [SUB._sublist(N, L, seed=L) for L in (1, 7, 33)]
    SUB._check(s, stored, q, K, lists, ql=[2, 0, 1], live=live)


# -- the lexical index ---------------------------------------------------------------------------------
def test_lex_search_and_score_rows_equal_their_dev_paths():
    from super_rag_amd.lexical import query_arrays
    lex = _lex()
    qoff, qterms = query_arrays(QUERIES)
    sc_d, rows_d = _host(*lex.search_dev(qoff, qterms, K))
    assert (rows_d >= 0).all() and not np.isin(rows_d, DEAD).any()
    sc_h, rows_h = lex.search(QUERIES, K)
    _same(rows_h, rows_d, "lex rows")
    _same(sc_h, sc_d, "lex scores")
    sc_f, rows_f, fx = lex.search(QUERIES, K, fixed=True)
    _same(rows_f, rows_d, "lex rows (fixed)")
    _same(sc_f, sc_d, "lex scores (fixed)")

    rows = np.array([[0, 299, 3, -1, 150, 300, 7],
                     [13, 1, 2, 10 ** 6, 298, 297, 23],
                     [5, 5, 299, 0, 33, 43, 44]], np.int64)
    rows[:, :K] = rows_d                                   # pairs that do score, then the edge rows
    sr_d, fx_d = _host(*lex.score_rows_dev(qoff, qterms, _dev(rows), fixed=True))
    sr_h, fx_h = lex.score_rows(QUERIES, rows, fixed=True)
    _same(sr_h, sr_d, "lex score_rows")
    _same(fx_h, fx_d.view(np.uint32), "lex score_rows fixed")
    _same(fx_h[:, :K], fx, "score_rows fixed against the search's own")
    _same(lex.score_rows(QUERIES, rows), sr_d, "lex score_rows without the fixed output")


# -- fusion of lists -------------------------------------------------------------------------------------
def _lists():
    rng = np.random.default_rng(22)
    ra = np.stack([rng.permutation(40)[:5] for _ in range(B)]).astype(np.int64)
    rb = np.stack([rng.permutation(40)[:7] for _ in range(B)]).astype(np.int64)
    rb[:, 1] = ra[:, 0]                                    # shared rows, and absent ones
    rb[:, 4] = ra[:, 3]
    ra[1, 4] = rb[2, 6] = -1
    sa = np.sort(rng.random((B, 5)).astype(np.float32), axis=1)[:, ::-1].copy()
    sb = np.sort(9 * rng.random((B, 7)).astype(np.float32), axis=1)[:, ::-1].copy()
    side_a = rng.random((B, 7)).astype(np.float32)
    side_b = (9 * rng.random((B, 5))).astype(np.float32)
    side_a[0, 2] = side_b[2, 1] = -np.inf                  # unknown
    return ra, sa, rb, sb, side_a, side_b


def test_rrf_fuse_equals_rrf_fuse_dev():
    from super_rag_amd.lexical import rrf_fuse, rrf_fuse_dev
    ra, _, rb, _, _, _ = _lists()
    for k, ms in ((9, float("-inf")), (12, 0.4)):
        sc_h, rows_h = rrf_fuse(ra, rb, k, rank_const=1, min_score=ms)
        sc_d, rows_d = _host(*rrf_fuse_dev(_dev(ra), _dev(rb), k, rank_const=1, min_score=ms))
        assert (rows_d[:, 0] >= 0).all()
        _same(rows_h, rows_d, "rrf rows")
        _same(sc_h, sc_d, "rrf scores")


@pytest.mark.parametrize("mode", ["relative", "floor"])
@pytest.mark.parametrize("sides", ["none", "a", "b", "both"])
def test_score_fuse_equals_score_fuse_dev(mode, sides):
    from super_rag_amd.lexical import score_fuse, score_fuse_dev
    ra, sa, rb, sb, side_a, side_b = _lists()
    da = side_a if sides in ("a", "both") else None
    db = side_b if sides in ("b", "both") else None
    got = score_fuse(sa, ra, sb, rb, 9, mode=mode, alpha=0.3, side_a=da, side_b=db)
    want = _host(*score_fuse_dev(_dev(sa), _dev(ra), _dev(sb), _dev(rb), 9, mode=mode, alpha=0.3,
                                 side_a=None if da is None else _dev(da),
                                 side_b=None if db is None else _dev(db)))
    assert (want[1][:, 0] >= 0).all()
    for g, w, what in zip(got, want, ("fused", "rows", "a", "b")):
        _same(g, w, f"score_fuse {what}")


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("fusion", ["rrf", "floor", "floor_full"])
def test_hybrid_search_equals_its_steps_composed_from_the_dev_calls(scan, fusion):
    import torch
    from super_rag_amd.lexical import hybrid_search, query_arrays, rrf_fuse_dev, score_fuse_dev
    s, q = _store(scan)
    lex = _lex()
    k, k_each = 7, K
    qoff, qterms = query_arrays(QUERIES)
    qd = _dev(q)
    sim, drow = s.search_dev(qd, k_each)
    lsc, lrow = lex.search_dev(qoff, qterms, k_each)
    if fusion == "rrf":
        want = _host(*rrf_fuse_dev(drow, lrow, k, rank_const=1, min_score=float("-inf")))
        got = hybrid_search(s, lex, q, QUERIES, k, k_each, rank_const=1, fusion="rrf")
    else:
        side_a = s.score_rows_dev(qd, lrow)
        side_b = None
        if fusion == "floor_full":                         # a row that matches nothing stays unknown
            bm = lex.score_rows_dev(qoff, qterms, drow)
            side_b = torch.where(bm == 0, torch.full_like(bm, float("-inf")), bm)
        want = _host(*score_fuse_dev(sim, drow, lsc, lrow, k, mode="floor", alpha=0.3, side_a=side_a,
                                     floor_a=-1.0, floor_b=0.0, side_b=side_b))
        got = hybrid_search(s, lex, q, QUERIES, k, k_each, fusion=fusion, alpha=0.3, components=True)
    assert (want[1][:, 0] >= 0).all()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"hybrid {fusion} output {i}")


# -- the store-less MMR ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["onepass", "greedy"])
def test_mmr_rerank_against_the_numpy_reference(mode):
    import mmr_ref as R
    import test_gpu_mmr as M
    from super_rag_amd.store import mmr_rerank
    Kc, k, lam, ms = 7, 5, 0.5, -2.0
    C, q = M._clustered(np.random.default_rng(23), B, Kc, DIM)
    n_cand = np.array([Kc, 0, Kc - 2], np.int32)
    Ch, qh = M.held(C.reshape(B * Kc, DIM)).reshape(B, Kc, DIM), M.held(q)
    for nc in (None, n_cand):
        sc, ix = mmr_rerank(q, C, nc, lam=lam, mode=mode, min_score=ms, k=k)
        assert sc.shape == (B, k) and ix.shape == (B, k)
        for b in range(B):
            valid = np.arange(Kc) < (Kc if nc is None else nc[b])
            rel, G = M.rel_gram(qh[b], Ch[b])
            assert (ix[b] < (Kc if nc is None else nc[b])).all()
            assert (ix[b][0] >= 0) == bool(valid.any())
            if mode == "onepass":
                M.check_onepass(sc[b], ix[b], R.onepass_scores(rel, G, lam, valid), ms, k)
            else:
                M.check_greedy(sc[b], ix[b], rel, G, lam, ms, k, valid)


# -- the encoder -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_types", [False, True])
def test_encoder_forward_equals_forward_dev(with_types):
    import test_gpu_encoder as E
    from super_rag_amd.encoder import Encoder, random_weights
    S = 5
    for classifier in (0, 1):
        spec = E._tiny("bert", classifier=classifier)
        enc = Encoder(spec, weights=random_weights(spec, seed=3, style="test"))
        ids, mask = E._batch(spec, B, S, seed=S)
        tt = (np.arange(S)[None] >= 2).astype(np.int32).repeat(B, 0) if with_types else None
        dev = [_dev(ids), _dev(mask), None if tt is None else _dev(tt)]
        if classifier:
            got = enc.cross_score(ids, mask, tt)
            want, = _host(enc.cross_score_dev(*dev))
        else:
            got = enc.embed(ids, mask, tt)
            want, = _host(enc.embed_dev(*dev, fp16=False))
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        _same(got, want, f"encoder classifier={classifier}")
        enc.close()
