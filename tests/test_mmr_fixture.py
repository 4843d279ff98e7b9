"""CPU: the MMR restatement pinned to the reference's own function, the greedy mode's properties,
the argument checks of the C ABI and the connector's plumbing.

tests/golden/mmr_fixtures.npz holds the outputs of graphiti's ``maximal_marginal_relevance``
(super_rag/graphiti/graphiti_core/search/search_utils.py:1884-1922), captured by
tests/golden/gen_mmr_fixtures.py on candidates drawn from the corpora of cosine_fixtures.npz.
tests/mmr_ref.py (SR_MMR_ONEPASS) must reproduce every case's id order exactly and its scores to
1e-12; the GPU suite (tests/test_gpu_mmr.py) then checks the device against it.
"""
import os

import numpy as np
import pytest

import mmr_ref as R
from doubles import NumpyStore

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def load_cases():
    """[(name, C [K, dim] fp64 raw candidates, q [dim] fp64 raw query, lambda, min_score,
    reference ids, reference scores)]"""
    z = np.load(os.path.join(GOLD, "mmr_fixtures.npz"))
    cz = np.load(os.path.join(GOLD, "cosine_fixtures.npz"))
    val = lambda c, e: c.astype(np.float64) / 16.0 * np.exp2(e.astype(np.float64))[:, None]
    corp = {}
    out = []
    for name in z["cases"].tolist():
        src = str(z[name + ".src"])
        if src:
            if src not in corp:
                corp[src] = (val(cz[src + ".c"], cz[src + ".ce"]), val(cz[src + ".q"], cz[src + ".qe"]))
            C, q = corp[src][0][z[name + ".rows"]], corp[src][1][int(z[name + ".qi"])]
        else:
            C, q = z[name + ".c"], z[name + ".q"]
        out.append((name, C, q, float(z[name + ".lam"]), float(z[name + ".min_score"]),
                    z[name + ".ids"].tolist(), z[name + ".scores"]))
    return out


CASES = load_cases()
IDS = [c[0] for c in CASES]


def test_fixture_covers_the_requested_cases():
    names = set(IDS)
    for fam in ("random", "clustered", "ties_zeros", "sparse"):
        for dim in (64, 384, 768, 1024):
            assert any(n.startswith(f"{fam}_{dim}_k") for n in names)
    assert {len(c[1]) for c in CASES} >= {1, 2, 17, 100, 128}
    assert {c[3] for c in CASES} == {0.0, 0.3, 0.5, 1.0}
    assert {c[4] for c in CASES} == {-2.0, 0.1}
    assert any(not c[2].any() for c in CASES)                      # the zero query
    assert any(len(c[5]) < len(c[1]) for c in CASES)               # min_score drops something
    assert "antipodal_l5" in names


@pytest.mark.parametrize("name,C,q,lam,ms,ids,scores", CASES, ids=IDS)
def test_restatement_reproduces_the_reference(name, C, q, lam, ms, ids, scores):
    got_ids, got_scores = R.mmr_onepass(R.normalize(q), R.normalize(C), lam, ms)
    assert got_ids == ids
    np.testing.assert_allclose(got_scores, scores, rtol=0, atol=1e-12)


def test_antipodal_candidates_clamp_at_zero():
    case = {c[0]: c for c in CASES}["antipodal_l5"]
    _, C, q, lam, ms, ids, scores = case
    Cn, qn = R.normalize(C), R.normalize(q)
    assert np.dot(Cn[0], Cn[1]) == pytest.approx(-1.0)
    # m = max(0, -1) = 0: the score is lambda rel alone
    np.testing.assert_allclose(scores, sorted(lam * R.relevance(qn, Cn), reverse=True), atol=1e-15)
    assert ids == [0, 1]


def _unit(rng, n, dim):
    return R.normalize(rng.standard_normal((n, dim)))


def test_greedy_lambda_one_is_relevance_order():
    rng = np.random.default_rng(1)
    C, q = _unit(rng, 40, 32), _unit(rng, 1, 32)[0]
    C[7] = C[3]                                                    # a tie: lower position first
    ids, scores = R.mmr_greedy(q, C, 1.0)
    rel = R.relevance(q, C)
    assert ids == sorted(range(40), key=lambda i: rel[i], reverse=True)
    np.testing.assert_allclose(scores, rel[ids], atol=0)
    assert ids.index(3) + 1 == ids.index(7)


def test_greedy_keeps_the_first_duplicate_and_demotes_the_second():
    rng = np.random.default_rng(2)
    C, q = _unit(rng, 30, 48), _unit(rng, 1, 48)[0]
    rel = R.relevance(q, C)
    top = int(np.argmax(rel))
    C = np.concatenate([C, C[top:top + 1]])                       # position 30 duplicates the best row
    rel = R.relevance(q, C)
    by_rel = sorted(range(31), key=lambda i: rel[i], reverse=True)
    assert by_rel[:2] == [top, 30]
    ids, scores = R.mmr_greedy(q, C, 0.5)
    assert ids[0] == top and scores[0] == pytest.approx(0.5 * rel[top])
    assert ids.index(30) > 1                                       # the copy lost its relevance rank
    # the one-pass mode demotes both copies (both have m = 1)
    one, _ = R.mmr_onepass(q, C, 0.5)
    assert one.index(top) > 0 and one.index(30) == one.index(top) + 1
    # greedy scores never increase: stopping at min_score equals filtering
    assert all(a >= b for a, b in zip(scores, scores[1:]))
    cut = scores[len(scores) // 2]
    assert R.mmr_greedy(q, C, 0.5, min_score=cut)[0] == [i for i, s in zip(ids, scores) if s >= cut]


def test_first_pick_is_the_same_in_both_modes_when_every_maximum_is_zero():
    # mutually non-positive similarities: orthogonal axes and their negatives
    C = np.concatenate([np.eye(6, 12), -np.eye(6, 12)])
    q = R.normalize(np.arange(1.0, 13.0))
    assert R.gram(C).max() <= 0
    one, s1 = R.mmr_onepass(q, C, 0.3)
    gre, s2 = R.mmr_greedy(q, C, 0.3)
    assert one[0] == gre[0] and s1[0] == s2[0]


@pytest.mark.parametrize("K,lam,k_out,word", [(129, 0.5, 10, "candidates"), (16, 1.5, 4, "lambda"),
                                              (16, 0.5, 17, "k_out")])
def test_argument_errors_are_invalid_before_any_device_call(K, lam, k_out, word):
    from super_rag_amd import _native
    from super_rag_amd.store import mmr_rerank
    q = np.ones((1, 8), np.float32)
    with pytest.raises(_native.NativeError) as e:
        mmr_rerank(q, np.ones((1, K, 8), np.float32), lam=lam, k=k_out)
    assert e.value.code == _native.SR_ERR_INVALID and word in e.value.message
    # the store entry points check the same limits before they touch the (here null) store's device
    lib = _native.load()
    rc = lib.sr_store_search_mmr(None, None, 1, k_out, K, lam, 0, -2.0, None, 0, None, None, None)
    assert rc == _native.SR_ERR_INVALID
    rc = lib.sr_store_mmr_dev(None, None, None, 1, K, 0, lam, 0, -2.0, k_out, None, None, None, None)
    assert rc == _native.SR_ERR_INVALID


# -- the connector on a CPU double that implements search_mmr -------------------------------------
class MmrStore(NumpyStore):
    calls: list = []

    def search_mmr(self, queries, k, fetch_k, lam=0.5, mode="onepass", min_score=-2.0, allow=None,
                   mask_key=0):
        MmrStore.calls.append(dict(B=len(queries), k=k, fetch_k=fetch_k, lam=lam, mode=mode,
                                   allow=None if allow is None else np.asarray(allow).copy()))
        dist, rows = NumpyStore.search(self, queries, fetch_k, allow=allow, mask_key=mask_key)
        B = len(queries)
        score = np.full((B, k), -np.inf, np.float32)
        od = np.full((B, k), np.inf, np.float32)
        orr = np.full((B, k), -1, np.int64)
        for b in range(B):
            r = rows[b][rows[b] >= 0]
            C, q = R.normalize(self.rows[r]), R.normalize(np.asarray(queries[b], np.float64))
            f = R.mmr_onepass if mode == "onepass" else R.mmr_greedy
            ids, sc = f(q, C, lam, min_score, k)
            score[b, :len(ids)], od[b, :len(ids)], orr[b, :len(ids)] = sc, dist[b][ids], r[ids]
        return score, od, orr

    def search(self, q, k, allow=None, mask_key=0):
        MmrStore.calls.append(dict(plain=True, B=len(q), k=k))
        return NumpyStore.search(self, q, k, allow=allow, mask_key=mask_key)


@pytest.fixture
def mmr_backend():
    from super_rag_amd import vectorstore as V
    V.set_store_backend(lambda dim, dev: MmrStore(dim, dev), MmrStore.load)
    V._collections.clear()
    MmrStore.calls = []
    yield V
    V._collections.clear()
    V.set_store_backend(V._native_store, V._native_load)


def _fill(V, name, ctx=None, n=60, dim=16, seed=0):
    from super_rag_amd.models import TextNode
    rng = np.random.default_rng(seed)
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    vecs[10:14] = vecs[5]                                          # planted duplicates of row 5
    conn = V.MI355XVectorStoreConnector({"collection": name, "coalesce": False, **(ctx or {})})
    conn.store.add([TextNode(text=f"t{i}", metadata={"g": i % 2}, embedding=v.tolist())
                    for i, v in enumerate(vecs)])
    return conn, vecs


def _query(vec, k):
    from super_rag_amd.models import QueryWithEmbedding
    return QueryWithEmbedding(query="q", top_k=k, embedding=[float(x) for x in vec])


def test_connector_context_keys_and_kwargs_reach_the_store(mmr_backend):
    V = mmr_backend
    conn, vecs = _fill(V, "mmr_a", {"diversify": "mmr", "mmr_lambda": 0.3, "mmr_mode": "greedy",
                                    "mmr_fetch_k": 24})
    res = conn.search(_query(vecs[5], 6)).results
    call = MmrStore.calls[-1]
    assert (call["k"], call["fetch_k"], call["lam"], call["mode"]) == (6, 24, 0.3, "greedy")
    assert len(res) == 6
    # scores are cosine distances of the kept rows, in MMR (not distance) order
    want = MmrStore.search_mmr(V._collections["mmr_a"].store, vecs[5][None], 6, 24, 0.3, "greedy")
    assert [d.score for d in res] == [float(x) for x in want[1][0]]
    assert [d.text for d in res] == [f"t{r}" for r in want[2][0]]
    assert res[0].score == pytest.approx(0.0, abs=1e-12) and all(0.0 <= d.score <= 2.0 for d in res)
    assert [d.score for d in res] != sorted(d.score for d in res)
    # the duplicate group of row 5 appears once under greedy
    assert sum(d.text in ("t5", "t10", "t11", "t12", "t13") for d in res) == 1
    # per-call kwargs override every key
    conn.search(_query(vecs[5], 6), mmr_lambda=0.9, mmr_mode="onepass", mmr_fetch_k=40)
    call = MmrStore.calls[-1]
    assert (call["k"], call["fetch_k"], call["lam"], call["mode"]) == (6, 40, 0.9, "onepass")
    # the default fetch_k is min(128, max(4 top_k, 20))
    plain = V.MI355XVectorStoreConnector({"collection": "mmr_a", "coalesce": False})
    for k, fk in ((3, 20), (10, 40), (40, 128)):
        plain.search(_query(vecs[1], k), diversify="mmr")
        assert MmrStore.calls[-1]["fetch_k"] == fk and MmrStore.calls[-1]["lam"] == 0.5
    # a kwarg can also switch it off for one call
    conn.search(_query(vecs[5], 6), diversify=None)
    assert MmrStore.calls[-1].get("plain")


def test_connector_diversify_off_calls_search_exactly_as_today(mmr_backend):
    V = mmr_backend
    conn, vecs = _fill(V, "mmr_b")
    MmrStore.calls = []
    res = conn.search(_query(vecs[5], 7)).results
    assert MmrStore.calls == [dict(plain=True, B=1, k=7)]
    d, r = NumpyStore.search(V._collections["mmr_b"].store, vecs[5][None], 7)
    assert [x.score for x in res] == [float(v) for v in d[0]]
    assert [x.text for x in res] == [f"t{i}" for i in r[0]]


def test_connector_grouping_separates_different_settings(mmr_backend):
    V = mmr_backend
    conn, vecs = _fill(V, "mmr_c", {"honor_filter": True})
    c = V._collections["mmr_c"]
    MmrStore.calls = []
    items = [(vecs[0], 4, None), (vecs[1], 5, None, (0.5, "onepass", 20)),
             (vecs[2], 3, None, (0.5, "onepass", 20)), (vecs[3], 4, None, (0.5, "greedy", 20)),
             (vecs[4], 4, None, (0.7, "onepass", 20)), (vecs[5], 4, None, (0.5, "onepass", 24)),
             (vecs[6], 4, {"g": 1}, (0.5, "onepass", 20)), (vecs[7], 2, None)]
    out = V.MI355XVectorStoreConnector._search_batch(c, items)
    assert [len(o) for o in out] == [4, 5, 3, 4, 4, 4, 4, 2]
    calls = MmrStore.calls
    assert len(calls) == 6                                         # only items 1 + 2 and 0 + 7 share a call
    assert sorted(c_["B"] for c_ in calls) == [1, 1, 1, 1, 2, 2]
    shared = [c_ for c_ in calls if c_["B"] == 2 and not c_.get("plain")][0]
    assert (shared["k"], shared["fetch_k"], shared["mode"]) == (5, 20, "onepass")
    masked = [c_ for c_ in calls if c_.get("allow") is not None]
    assert len(masked) == 1 and masked[0]["allow"].tolist() == [i % 2 for i in range(60)]
    assert all(t.metadata["g"] == 1 for t in out[6])
    # every item equals its own single-item batch
    for it, o in zip(items, out):
        solo = V.MI355XVectorStoreConnector._search_batch(c, [it])[0]
        assert [(d.text, d.score) for d in solo] == [(d.text, d.score) for d in o]


def test_connector_threshold_is_a_filter_not_a_prefix_cut(mmr_backend):
    V = mmr_backend
    conn, vecs = _fill(V, "mmr_d", {"diversify": "mmr", "mmr_mode": "greedy", "mmr_lambda": 0.3,
                                    "honor_score_threshold": True})
    full = conn.search(_query(vecs[5], 10)).results
    sims = [1.0 - d.score for d in full]
    assert sims != sorted(sims, reverse=True)                      # MMR order is not similarity order
    thr = sorted(sims)[len(sims) // 2]
    got = conn.search(_query(vecs[5], 10), score_threshold=thr).results
    assert [d.text for d in got] == [d.text for d, s in zip(full, sims) if s >= thr]
    assert 0 < len(got) < len(full)


def test_connector_limits(mmr_backend):
    V = mmr_backend
    with pytest.raises(ValueError, match="hybrid"):
        V.MI355XVectorStoreConnector({"collection": "x", "hybrid": True, "diversify": "mmr"})
    with pytest.raises(ValueError, match="diversify"):
        V.MI355XVectorStoreConnector({"collection": "x", "diversify": "dpp"})
    conn, vecs = _fill(V, "mmr_e", {"diversify": "mmr"}, n=20)
    with pytest.raises(ValueError, match="128"):
        conn.search(_query(vecs[0], 129))
    with pytest.raises(ValueError, match="128"):
        conn.search(_query(vecs[0], 5), mmr_fetch_k=200)
    # a fetch_k below top_k is raised to top_k
    conn.search(_query(vecs[0], 12), mmr_fetch_k=4)
    assert MmrStore.calls[-1]["fetch_k"] == 12


def test_connector_async_paths_carry_the_settings(mmr_backend):
    import asyncio
    V = mmr_backend
    conn, vecs = _fill(V, "mmr_f", {"diversify": "mmr", "coalesce": True})
    res = asyncio.run(conn.asearch(_query(vecs[5], 5), mmr_mode="greedy"))
    assert MmrStore.calls[-1]["mode"] == "greedy" and len(res.results) == 5
    sync = conn.search(_query(vecs[5], 5), mmr_mode="greedy").results
    assert [(d.text, d.score) for d in sync] == [(d.text, d.score) for d in res.results]
