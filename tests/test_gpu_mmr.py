"""GPU: MMR diversification (k_mmr.hip; sr_mmr_rerank / sr_store_search_mmr / sr_store_mmr_dev).

Tolerances.  Rows are compared as the store holds them (fp16, read back with get) and evaluated by
the fp64 restatement tests/mmr_ref.py.  tests/test_gpu_cosine_fixtures.py bounds one fp32-MFMA dot
of such rows by 2e-6; an MMR score is lambda e1 + (1 - lambda) e2 of two such errors, so at most
2e-6, plus a few fp32 roundings of values <= 1: BAND = 2.5e-6.  Against the reference's own fp64
scores (tests/golden/mmr_fixtures.npz) the per-pair fp16 rounding of the rows is added: |dot of
the fp16 rows - dot of the exact rows| for rel and for every G_ij under the maximum.  The fp16 rows
of that budget are the ones read back from the store.  The host emulation quantize_like_store,
which test_gpu_cosine_fixtures.py uses under its 1e-4 base tolerance, is not bit-exact (its fp32
norm is summed in another order; an ulp of it moves every element of one value across an fp16
boundary, and the fixtures' integer-coded rows repeat values): with its budget random_768_k100
misses by 2.0e-6 (|device - reference| 1.61e-5 against 2.5e-6 + 1.16e-5) while the device is within
2.5e-6 of the fp64 scores of the rows it holds (measured: <= 1.7e-7 over all fixtures); 3 of that
case's 100 stored rows differ from the emulation.  Both budgets are printed.

One-pass mode is checked for value, order and kept set; greedy mode for validity (every pick is
within the band of the best remaining marginal value given the device's own earlier picks), and
for equality with the restatement where the gaps exceed the band.
"""
import numpy as np
import pytest

import mmr_ref as R
from oracle.cosine_topk import quantize_like_store, same_topk_modulo_ties
from test_mmr_fixture import CASES, IDS

pytestmark = pytest.mark.gpu

BAND = 2.5e-6


def held(x):
    """x [n, dim] as a store holds it: normalised fp16 rows, read back as fp64."""
    from super_rag_amd.store import NativeStore
    x = np.asarray(x, np.float32)
    s = NativeStore(x.shape[1], device=0)
    s.add(x)
    out = s.get(np.arange(x.shape[0])).astype(np.float64)
    s.close()
    return out


def rel_gram(q, C):
    G = C @ C.T
    np.fill_diagonal(G, 0.0)
    return C @ q, G


def check_tail(score, index):
    n = int((index >= 0).sum())
    assert (index[:n] >= 0).all() and (index[n:] == -1).all()
    assert np.isneginf(score[n:]).all() and np.isfinite(score[:n]).all()
    assert len(set(index[:n].tolist())) == n
    return n


def check_onepass(score, index, s64, ms, k, tol=None, eps=BAND):
    """score / index: one query's device output; s64: fp64 scores per position (-inf: missing)."""
    n = check_tail(score, index)
    ids = index[:n].tolist()
    tol = np.full(len(s64), BAND) if tol is None else tol
    for t, i in enumerate(ids):
        assert np.isfinite(s64[i]), f"missing candidate {i} returned"
        assert abs(float(score[t]) - s64[i]) <= tol[i], (t, i, float(score[t]), s64[i])
        assert score[t] >= np.float32(ms)
    for t in range(n - 1):          # (device score desc, position asc)
        assert score[t] > score[t + 1] or (score[t] == score[t + 1] and ids[t] < ids[t + 1])
    ref = sorted((i for i in range(len(s64)) if np.isfinite(s64[i])), key=lambda i: s64[i], reverse=True)
    ref = [i for i in ref if s64[i] >= ms][:k]
    if len(ref) == n:
        assert same_topk_modulo_ties([ids], [score[:n].astype(np.float64)], [ref], [s64[ref]], eps)
    else:                           # rows within the band of the min_score cut may fall either side
        assert all(abs(s64[i] - ms) <= eps for i in set(ref) ^ set(ids)), (ref, ids)


def check_greedy(score, index, rel, G, lam, ms, k, valid=None):
    n = check_tail(score, index)
    picked = []
    for t in range(k):
        v = R.greedy_values(rel, G, lam, picked, valid)
        best = float(v.max()) if len(v) else -np.inf
        if t >= n:                  # the device stopped: nothing left at or above min_score
            assert not np.isfinite(best) or best < ms + BAND, (t, best)
            break
        p = int(index[t])
        assert np.isfinite(v[p]), f"candidate {p} is missing or was picked before"
        assert v[p] >= best - BAND, (t, p, v[p], best)
        assert abs(float(score[t]) - v[p]) <= BAND, (t, p, float(score[t]), v[p])
        assert score[t] >= np.float32(ms)
        picked.append(p)
    return picked


def min_gap(rel, G, lam, ms, k, valid=None):
    """Smallest distance between the best and the second-best marginal value over the greedy run
    of the restatement (and between the last best value and min_score)."""
    picked, gap = [], np.inf
    for _ in range(k):
        v = R.greedy_values(rel, G, lam, picked, valid)
        o = np.sort(v[np.isfinite(v)])[::-1]
        if len(o) == 0:
            break
        gap = min(gap, abs(o[0] - ms))
        if o[0] < ms:
            break
        if len(o) > 1:
            gap = min(gap, o[0] - o[1])
        picked.append(int(np.argmax(v)))
    return gap


# -- the reference's fixtures ------------------------------------------------------------------
def _rounding_budget(C, q, lam, cq, qq):
    """Per-candidate bound of |score on the fp16 rows cq / qq - score on the exact rows C / q|:
    the per-pair rounding of rel and of G (a maximum moves by at most the largest move under it)."""
    Cn, qn = R.normalize(C), R.normalize(q)
    r_rel = np.abs(cq @ qq - Cn @ qn)
    r_g = np.abs(cq @ cq.T - Cn @ Cn.T)
    np.fill_diagonal(r_g, 0.0)
    return lam * r_rel + (1.0 - lam) * (r_g.max(axis=1) if len(C) else 0.0)


def _reference_scores(C, q, lam, ids, scores):
    """fp64 reference score of every position: the fixture's where it lists the row (the rest fell
    below min_score there: the restatement, pinned to the fixture by tests/test_mmr_fixture.py)."""
    Cn, qn = R.normalize(C), R.normalize(q)
    s = R.onepass_scores(R.relevance(qn, Cn), R.gram(Cn), lam)
    s[np.asarray(ids, dtype=np.int64)] = scores
    return s


@pytest.mark.parametrize("name,C,q,lam,ms,ids,scores", CASES, ids=IDS)
def test_onepass_fixtures_through_mmr_rerank_and_search_mmr(name, C, q, lam, ms, ids, scores):
    from super_rag_amd.store import NativeStore, mmr_rerank
    K, dim = C.shape
    s_ref = _reference_scores(C, q, lam, ids, scores)
    st = NativeStore(dim, device=0)
    st.add(C.astype(np.float32))
    Ch = st.get(np.arange(K)).astype(np.float64)
    qh = held(q[None])[0]
    # the rounding budget of the rows the device holds.  quantize_like_store emulates them on the
    # host, but not to the bit: its fp32 norm is summed in another order, and in these fixtures
    # (small integer codes: many elements of a row share one value) an ulp of the norm moves all
    # elements of one value across an fp16 rounding boundary together.  Its budget is printed; the
    # one asserted is that of the rows read back from the store (see the module docstring).
    tol_ref = BAND + _rounding_budget(C, q, lam, Ch, qh)
    tol_host = BAND + _rounding_budget(C, q, lam, quantize_like_store(C).astype(np.float64),
                                       quantize_like_store(q[None])[0].astype(np.float64))
    print(name, "budget max: held rows %.3g, quantize_like_store %.3g, rows differing %d of %d" % (
        tol_ref.max() - BAND, tol_host.max() - BAND,
        int((Ch != quantize_like_store(C).astype(np.float64)).any(axis=1).sum()), K))
    eps_ref = BAND + 2 * float((tol_ref - BAND).max())
    rel, G = rel_gram(qh, Ch)
    s_held = R.onepass_scores(rel, G, lam)
    for k in sorted({K, min(K, 5)}):
        sc, ix = mmr_rerank(q[None], C[None], lam=lam, mode="onepass", min_score=ms, k=k)
        print(name, "rerank k", k, "max |dev - held|",
              max([abs(float(a) - s_held[i]) for a, i in zip(sc[0], ix[0]) if i >= 0], default=0.0))
        check_onepass(sc[0], ix[0], s_held, ms, k)
        check_onepass(sc[0], ix[0], s_ref, ms, k, tol=tol_ref, eps=eps_ref)
        # the store path: the fixture's candidates are the whole store, fetch_k = K
        sc2, dist, rows = st.search_mmr(q[None].astype(np.float32), k, K, lam=lam, mode="onepass",
                                        min_score=ms)
        ix2 = rows[0].astype(np.int64)
        print(name, "store  k", k, "max |dev - held|",
              max([abs(float(a) - s_held[i]) for a, i in zip(sc2[0], ix2) if i >= 0], default=0.0))
        # position in the candidate list = rank in the scan's order; the score of a row does not
        # depend on it, and ties are exact duplicates, so check by row id with ties by scan rank
        n = check_tail(sc2[0], ix2)
        for t in range(n):
            i = int(ix2[t])
            assert abs(float(sc2[0][t]) - s_held[i]) <= BAND
            assert abs(float(sc2[0][t]) - s_ref[i]) <= tol_ref[i]
            assert abs((1.0 - float(dist[0][t])) - rel[i]) <= BAND
        assert np.isposinf(dist[0][n:]).all()
        assert all(sc2[0][t] >= sc2[0][t + 1] for t in range(n - 1))
        ref = [i for i in sorted(range(K), key=lambda i: s_held[i], reverse=True) if s_held[i] >= ms][:k]
        if len(ref) == n:
            assert same_topk_modulo_ties([ix2[:n]], [sc2[0][:n].astype(np.float64)], [ref],
                                         [s_held[ref]], BAND)
        else:
            assert all(abs(s_held[i] - ms) <= BAND for i in set(ref) ^ set(ix2[:n].tolist()))
    st.close()


@pytest.mark.parametrize("name,C,q,lam,ms,ids,scores", CASES, ids=IDS)
def test_greedy_fixture_candidates_are_valid_selections(name, C, q, lam, ms, ids, scores):
    from super_rag_amd.store import mmr_rerank
    K = len(C)
    Ch, qh = held(C), held(q[None])[0]
    rel, G = rel_gram(qh, Ch)
    sc, ix = mmr_rerank(q[None], C[None], lam=lam, mode="greedy", min_score=ms, k=K)
    picked = check_greedy(sc[0], ix[0], rel, G, lam, ms, K)
    if name.startswith("random"):
        # the device must make the restatement's picks.  Gaps between the best and the next
        # marginal value, measured with the restatement on the fp16-rounded rows when this test was
        # written: >= 3.9e-5 on every random case but two.  random_64_k100 (lambda 1) has one gap
        # of 3.0e-6, above the band but below twice it; the lambda = 0 cases start from exact ties
        # at 0 (every value is -cur = 0 until no candidate with a non-positive similarity to the
        # picks is left), which the device and the restatement both resolve by position.
        print(name, "smallest greedy gap", min_gap(rel, G, lam, ms, K))
        want, _ = R.mmr_greedy(qh, Ch, lam, ms, K, rel=rel, G=G)
        assert picked == want


# -- shapes: every tile edge, padded dims, several blocks, ragged counts ---------------------------
def _clustered(rng, B, K, dim):
    cent = rng.standard_normal((max(K // 4, 1), dim))
    C = cent[rng.integers(0, len(cent), (B, K))] + 0.4 * rng.standard_normal((B, K, dim))
    if K >= 4:
        C[:, K - 1] = C[:, 1]                                      # an exact duplicate pair
        C[:, K // 2] = 0.0                                         # a zero row
    q = cent[rng.integers(0, len(cent), B)] + 0.5 * rng.standard_normal((B, dim))
    return C.astype(np.float32), q.astype(np.float32)


SHAPES = [(1, 64, 1), (2, 100, 3), (15, 384, 3), (16, 64, 33), (17, 100, 33), (100, 1024, 3),
          (128, 384, 1), (128, 1024, 33)]


@pytest.mark.parametrize("mode", ["onepass", "greedy"])
@pytest.mark.parametrize("K,dim,B", SHAPES, ids=[f"K{k}_d{d}_B{b}" for k, d, b in SHAPES])
def test_shapes_and_ragged_candidate_counts(K, dim, B, mode):
    from super_rag_amd.store import mmr_rerank
    rng = np.random.default_rng(K * 1000 + dim + B)
    C, q = _clustered(rng, B, K, dim)
    n_cand = rng.integers(0, K + 1, B).astype(np.int32)
    n_cand[0] = K
    if B > 2:
        n_cand[1], n_cand[2] = 0, max(K - 1, 0)
    lam, ms = 0.5, (-2.0 if K % 2 else 0.05)
    k = max(1, (3 * K) // 4)
    Ch = held(C.reshape(B * K, dim)).reshape(B, K, dim)
    qh = held(q)
    for nc in (None, n_cand):
        sc, ix = mmr_rerank(q, C, nc, lam=lam, mode=mode, min_score=ms, k=k)
        sc_again, ix_again = mmr_rerank(q, C, nc, lam=lam, mode=mode, min_score=ms, k=k)
        assert np.array_equal(ix, ix_again) and np.array_equal(sc.view(np.uint32), sc_again.view(np.uint32))
        for b in range(B):
            valid = np.arange(K) < (K if nc is None else nc[b])
            rel, G = rel_gram(qh[b], Ch[b])
            assert (ix[b] < (K if nc is None else nc[b])).all()
            if mode == "onepass":
                check_onepass(sc[b], ix[b], R.onepass_scores(rel, G, lam, valid), ms, k)
            else:
                check_greedy(sc[b], ix[b], rel, G, lam, ms, k, valid)


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_lambda_end_points(lam):
    from super_rag_amd.store import mmr_rerank
    rng = np.random.default_rng(11)
    C, q = _clustered(rng, 3, 40, 100)
    Ch, qh = held(C.reshape(120, 100)).reshape(3, 40, 100), held(q)
    for mode in ("onepass", "greedy"):
        sc, ix = mmr_rerank(q, C, lam=lam, mode=mode, k=40)
        for b in range(3):
            rel, G = rel_gram(qh[b], Ch[b])
            if mode == "onepass":
                check_onepass(sc[b], ix[b], R.onepass_scores(rel, G, lam), -2.0, 40)
            else:
                check_greedy(sc[b], ix[b], rel, G, lam, -2.0, 40)
            if lam == 1.0 and mode == "greedy":      # exact ties in relevance: lower position first
                assert ix[b].tolist().index(1) + 1 == ix[b].tolist().index(39)


# -- the store paths -------------------------------------------------------------------------------
def _store(n, dim, seed, dead=(), device=0):
    from super_rag_amd.store import NativeStore
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((12, dim))
    x = (cent[np.arange(n) % 12] + 0.35 * rng.standard_normal((n, dim))).astype(np.float32)
    x[n - 3:] = x[:3]                                              # exact duplicates
    s = NativeStore(dim, device=device)
    s.add(x)
    if len(dead):
        s.remove(np.asarray(dead, np.int64))
    q = (cent[rng.integers(0, 12, 33)] + 0.5 * rng.standard_normal((33, dim))).astype(np.float32)
    return s, x, q


def _check_store_result(s, q, score, dist, rows, fetch_k, k, lam, mode, ms, allow=None):
    """search_mmr against the restatement on the scan's own candidate list (search_sim)."""
    sim, cand = s.search_sim(q, fetch_k, allow=allow)
    n_rows = s.count()[0]
    Hs = s.get(np.arange(n_rows)).astype(np.float64)
    qh = held(q)
    for b in range(len(q)):
        valid = cand[b] >= 0
        Cb = Hs[np.clip(cand[b], 0, None)]
        rel, G = rel_gram(qh[b], Cb)
        assert np.all(np.abs(rel[valid] - sim[b][valid]) <= 2e-6)
        pos_of = {int(r): i for i, r in enumerate(cand[b]) if r >= 0}
        assert all(int(r) in pos_of for r in rows[b] if r >= 0), "a row outside the candidates"
        index = np.array([pos_of[int(r)] if r >= 0 else -1 for r in rows[b]], np.int64)
        if mode == "onepass":
            check_onepass(score[b], index, R.onepass_scores(rel, G, lam, valid), ms, k)
        else:
            check_greedy(score[b], index, rel, G, lam, ms, k, valid)
        kept = index >= 0
        assert np.all(np.abs((1.0 - dist[b][kept].astype(np.float64)) - rel[index[kept]]) <= BAND)
        assert np.isposinf(dist[b][~kept]).all()


@pytest.mark.parametrize("mode", ["onepass", "greedy"])
def test_search_mmr_with_mask_tombstones_and_missing_candidates(mode):
    n, dim = 300, 100
    dead = np.arange(5, n, 7)
    s, x, q = _store(n, dim, 3, dead)
    allow = (np.arange(n) % 3 != 1).astype(np.uint8)
    for fetch_k, k, al in ((128, 20, None), (100, 100, allow), (17, 16, allow)):
        score, dist, rows = s.search_mmr(q, k, fetch_k, lam=0.5, mode=mode, allow=al, mask_key=5)
        live = rows[rows >= 0]
        assert not np.isin(live, dead).any()                       # tombstoned rows never returned
        if al is not None:
            assert al[live].all()
        _check_store_result(s, q, score, dist, rows, fetch_k, k, 0.5, mode, -2.0, allow=al)
    s.close()
    # fewer live rows than fetch_k: the scan reports -1 for the missing candidates
    s, x, q = _store(40, 64, 4, dead=np.arange(0, 40, 4))
    score, dist, rows = s.search_mmr(q[:3], 35, 100, lam=0.3, mode=mode)
    assert ((rows >= 0).sum(axis=1) == 30).all() and (rows[:, 30:] == -1).all()
    assert np.isneginf(score[:, 30:]).all()
    _check_store_result(s, q[:3], score, dist, rows, 100, 35, 0.3, mode, -2.0)
    # and an empty store
    s.remove(np.setdiff1d(np.arange(40), np.arange(0, 40, 4)))
    score, dist, rows = s.search_mmr(q[:2], 4, 8, mode=mode)
    assert (rows == -1).all() and np.isneginf(score).all() and np.isposinf(dist).all()
    s.close()


@pytest.mark.parametrize("mode", ["onepass", "greedy"])
def test_mmr_dev_on_search_dev_outputs_equals_search_mmr(mode):
    import torch
    s, x, q = _store(500, 384, 6, dead=[7, 8, 9])
    score, dist, rows = s.search_mmr(q, 10, 64, lam=0.4, mode=mode, min_score=0.05)
    qd = torch.from_numpy(q).cuda()
    sim, cand = s.search_dev(qd, 64, row_offset=1000)
    assert int(cand.min()) >= 1000
    d_score, d_sim, d_rows = s.mmr_dev(cand, sim, 10, lam=0.4, mode=mode, min_score=0.05, row_offset=1000)
    torch.cuda.synchronize()
    d_rows = d_rows.cpu().numpy()
    assert np.array_equal(np.where(d_rows >= 0, d_rows - 1000, -1), rows)
    assert np.array_equal(d_score.cpu().numpy().view(np.uint32), score.view(np.uint32))
    keep = rows >= 0
    assert np.array_equal((np.float32(1.0) - d_sim.cpu().numpy())[keep], dist[keep])
    # determinism: a second run gives identical bits
    score2, dist2, rows2 = s.search_mmr(q, 10, 64, lam=0.4, mode=mode, min_score=0.05)
    assert np.array_equal(rows, rows2) and np.array_equal(score.view(np.uint32), score2.view(np.uint32))
    assert np.array_equal(dist.view(np.uint32), dist2.view(np.uint32))
    s.close()


def test_search_mmr_under_the_fp8_scan_reads_the_fp16_rows():
    s, x, q = _store(400, 768, 8)
    want = s.search_mmr(q, 10, 40, lam=0.5, mode="greedy")
    s.set_scan_dtype("fp8")
    got = s.search_mmr(q, 10, 40, lam=0.5, mode="greedy")
    _check_store_result(s, q, got[0], got[1], got[2], 40, 10, 0.5, "greedy", -2.0)
    s.set_scan_dtype("fp16")
    assert np.array_equal(s.search_mmr(q, 10, 40, lam=0.5, mode="greedy")[2], want[2])
    s.close()


@pytest.mark.parametrize("mode", ["onepass", "greedy"])
def test_sharded_store_returns_the_single_stores_result_within_the_band(mode):
    from super_rag_amd.store import NativeStore, ShardedStore
    rng = np.random.default_rng(9)
    dim, n = 384, 900
    cent = rng.standard_normal((10, dim))
    x = (cent[np.arange(n) % 10] + 0.35 * rng.standard_normal((n, dim))).astype(np.float32)
    q = (cent[rng.integers(0, 10, 5)] + 0.5 * rng.standard_normal((5, dim))).astype(np.float32)
    one, sh = NativeStore(dim), ShardedStore(dim, [0, 0])
    for a in range(0, n, 150):
        one.add(x[a:a + 150])
        sh.add(x[a:a + 150])
    dead = np.arange(3, n, 11)
    one.remove(dead)
    sh.remove(dead)
    allow = (np.arange(n) % 4 != 0).astype(np.uint8)
    for al in (None, allow):
        s1, d1, r1 = one.search_mmr(q, 12, 48, lam=0.5, mode=mode, allow=al, mask_key=3)
        s2, d2, r2 = sh.search_mmr(q, 12, 48, lam=0.5, mode=mode, allow=al, mask_key=3)
        _check_store_result(one, q, s2, d2, r2, 48, 12, 0.5, mode, -2.0, allow=al)
        for b in range(len(q)):
            both = {int(r): float(v) for r, v in zip(r1[b], s1[b]) if r >= 0}
            for r, v in zip(r2[b], s2[b]):
                if int(r) in both:
                    assert abs(both[int(r)] - float(v)) <= BAND
            assert not np.isin(r2[b][r2[b] >= 0], dead).any()
    one.close()
    sh.close()


def test_connector_diversify_returns_each_duplicate_group_once():
    from super_rag_amd import vectorstore as V
    from super_rag_amd.models import QueryWithEmbedding, TextNode
    V._collections.clear()
    rng = np.random.default_rng(12)
    dim = 384
    basis = np.linalg.qr(rng.standard_normal((dim, 6)))[0].T       # q direction + 5 orthonormal axes
    qv = basis[0]
    nodes = []
    for g in range(5):                                             # 5 passages, 4 copies of each
        v = (0.60 + 0.01 * g) * qv + 0.8 * basis[1 + g]
        nodes += [TextNode(text=f"group{g}", metadata={"copy": c}, embedding=v.tolist()) for c in range(4)]
    for i in range(180):
        nodes.append(TextNode(text=f"other{i}", metadata={}, embedding=rng.standard_normal(dim).tolist()))
    try:
        plain = V.MI355XVectorStoreConnector({"collection": "mmr_gpu", "coalesce": False})
        plain.store.add(nodes)
        query = QueryWithEmbedding(query="q", top_k=5, embedding=qv.tolist())
        got = [d.text for d in plain.search(query).results]
        assert got == ["group4"] * 4 + ["group3"]                  # the plain search returns the copies
        div = V.MI355XVectorStoreConnector({"collection": "mmr_gpu", "coalesce": False,
                                            "diversify": "mmr", "mmr_mode": "greedy"})
        res = div.search(query).results
        assert sorted(d.text for d in res) == [f"group{g}" for g in range(5)]
        assert res[0].text == "group4"
        # scores stay cosine distances
        for d in res:
            g = int(d.text[-1])
            assert d.score == pytest.approx(1.0 - (0.60 + 0.01 * g) / np.hypot(0.60 + 0.01 * g, 0.8), abs=1e-3)
        assert [d.text for d in plain.search(query, diversify="mmr", mmr_mode="greedy").results] == \
            [d.text for d in res]
    finally:
        V._collections.clear()
