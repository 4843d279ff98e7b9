"""CPU: the connector's opt-in field index and subset planner (ctx "filter_index" /
"subset_max_rows" with "honor_filter"): posting lists of metadata fields resolve a filter to its row
list on the host, and all such items of a batch reach the store in ONE search_subset call instead of
one masked search per distinct filter.  The store double adds an fp64 search_subset to NumpyStore
and counts calls; the kernel itself is tested in test_gpu_subset.py."""
import os
import re

import numpy as np
import pytest

from doubles import NumpyStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SubsetStore(NumpyStore):
    """NumpyStore + search_subset (each query against the rows of its own list), counting calls."""

    def __init__(self, dim, device=0):
        super().__init__(dim, device)
        self.calls = {"search": 0, "search_subset": 0}

    def search(self, q, k, allow=None, mask_key=0):
        self.calls["search"] += 1
        return super().search(q, k, allow=allow, mask_key=mask_key)

    def search_subset(self, queries, k, lists, q_list=None, sim=False):
        self.calls["search_subset"] += 1
        q = np.asarray(queries, np.float64)
        ql = np.arange(len(q)) if q_list is None else np.asarray(q_list)
        dist = np.full((len(q), k), np.inf)
        rows = np.full((len(q), k), -1, dtype=np.int64)
        for b in range(len(q)):
            rl = np.asarray(lists[ql[b]], dtype=np.int64)
            assert (np.diff(rl) > 0).all() and (rl.size == 0 or (rl[0] >= 0 and rl[-1] < len(self.rows)))
            allow = np.zeros(len(self.rows), bool)
            allow[rl] = True
            d, r = NumpyStore.search(self, q[b:b + 1], k, allow=allow)
            dist[b], rows[b] = d[0], r[0]
        return ((np.where(rows >= 0, 1.0 - dist, -np.inf), rows) if sim else (dist, rows))

    @classmethod
    def load(cls, path, device=0):
        with np.load(path) as z:
            s = cls(z["rows"].shape[1])
            s.rows, s.live = z["rows"], z["live"]
        return s


@pytest.fixture
def V():
    from super_rag_amd import vectorstore as V
    V._collections.clear()
    yield V
    V._collections.clear()
    V.set_store_backend(V._native_store, V._native_load)


def _conn(V, store_cls=SubsetStore, **kw):
    V.set_store_backend(lambda dim, dev: store_cls(dim, dev), store_cls.load)
    return V.MI355XVectorStoreConnector({"collection": "sub", "honor_filter": True, "coalesce": False,
                                         **kw})


def _nodes(metas, vecs):
    from super_rag_amd.models import TextNode
    return [TextNode(text=f"t{m.get('i', j)}", metadata=m, embedding=v.tolist())
            for j, (m, v) in enumerate(zip(metas, vecs))]


def _brute_index(c, fields):
    from super_rag_amd.filters import indexable
    want = {f: {} for f in fields}
    for r, md in enumerate(c.metadatas):
        for f in fields:
            if md and md.get(f) is not None and indexable(md.get(f)):
                want[f].setdefault(md[f], []).append(r)
    return want


def _index_as_lists(c):
    return {f: {v: list(p) for v, p in post.items() if len(p)} for f, post in c.findex.items()}


def _metas(n, rng):
    out = []
    for i in range(n):
        m = {"i": i, "chat_id": f"c{int(rng.integers(0, 12))}"}
        r = rng.random()
        if r < 0.4:
            m["indexer"] = "vector"
        elif r < 0.6:
            m["indexer"] = "graph"
        if rng.random() < 0.3:
            m["n"] = int(rng.integers(0, 4))
        if rng.random() < 0.05:
            m["chat_id"] = ["c1", "c2"]           # unhashable: never indexed, never == a scalar
        if rng.random() < 0.05:
            m["n"] = float("nan")
        out.append(m)
    return out


def test_field_index_follows_add_delete_compaction_and_restore(V, tmp_path):
    rng = np.random.default_rng(0)
    fields = ["chat_id", "n"]
    conn = _conn(V, filter_index=fields, snapshot_dir=str(tmp_path), compact_ratio=0.5)
    metas = _metas(300, rng)
    vecs = rng.standard_normal((300, 8))
    ids = conn.add(_nodes(metas[:100], vecs[:100]))
    c = V._get("sub")
    assert _index_as_lists(c) == _brute_index(c, fields)
    ids += conn.add(_nodes(metas[100:], vecs[100:]))
    assert _index_as_lists(c) == _brute_index(c, fields)
    # delete: the index is left alone (tombstoned rows are dropped on the device)
    before = _index_as_lists(c)
    conn.delete(ids=ids[:50])
    assert _index_as_lists(c) == before and c.store.count() == (300, 250)
    # auto-compaction (more than half the rows dead) renumbers the posting lists
    conn.delete(ids=ids[50:170])
    assert c.store.count() == (130, 130) and len(c.metadatas) == 130
    assert _index_as_lists(c) == _brute_index(c, fields)
    # restart from the snapshot: rebuilt from the restored metadata; the snapshot holds no index
    V._collections.clear()
    conn2 = _conn(V, filter_index=fields, snapshot_dir=str(tmp_path))
    c2 = V._get("sub")
    assert c2 is not c and len(c2.metadatas) == 130
    assert _index_as_lists(c2) == _brute_index(c2, fields)
    conn2.add(_nodes(metas[:7], vecs[:7]))
    assert _index_as_lists(c2) == _brute_index(c2, fields)
    # a connector without the key on the same collection changes nothing; one naming another
    # field back-fills it
    _conn(V, filter_index=["indexer"])
    assert _index_as_lists(c2) == _brute_index(c2, ["chat_id", "n", "indexer"])


def test_plan_resolvable_and_not():
    from super_rag_amd.filters import plan
    a = lambda *r: np.asarray(r, dtype=np.int64)
    index = {"chat_id": {"c1": a(0, 2, 4, 6, 8), "c2": a(1, 3), "c3": a(5, 7, 9, 10, 11, 12)},
             "n": {1: a(2, 3, 4), 2: a(9)}}
    rows, rest = plan({"chat_id": "c1"}, index)
    assert rows.tolist() == [0, 2, 4, 6, 8] and rest == []
    rows, rest = plan({"chat_id": {"$eq": "c2"}}, index)
    assert rows.tolist() == [1, 3] and rest == []
    rows, rest = plan({"chat_id": {"$in": ["c2", "c1", "zz", "c2"]}}, index)      # $in: sorted union
    assert rows.tolist() == [0, 1, 2, 3, 4, 6, 8] and rest == []
    assert plan({"chat_id": "nobody"}, index)[0].tolist() == []
    # conjunctions (and / $and / clause list / several keys) pick the shortest list; the others stay
    for f in ({"and": [{"chat_id": "c1"}, {"n": 1}]}, {"$and": [{"chat_id": "c1"}, {"n": 1}]},
              [{"chat_id": "c1"}, {"n": 1}], {"chat_id": "c1", "n": 1}):
        rows, rest = plan(f, index)
        assert rows.tolist() == [2, 3, 4] and rest == [{"chat_id": "c1"}]
    rows, rest = plan({"and": [{"chat_id": {"$in": ["c1", "c2"]}}, {"n": {"$in": [1, 2]}}]}, index)
    assert rows.tolist() == [2, 3, 4, 9] and rest == [{"chat_id": {"$in": ["c1", "c2"]}}]
    # 1 == 1.0 == True: one posting list, as matches compares
    assert plan({"n": 1.0}, index)[0].tolist() == [2, 3, 4]
    assert plan({"n": {"$in": [1, True, 1.0]}}, index)[0].tolist() == [2, 3, 4]
    # a clause with a further operator narrows the search but stays to be checked
    rows, rest = plan({"n": {"$in": [1, 2], "$ne": 2}}, index)
    assert rows.tolist() == [2, 3, 4, 9] and rest == [{"n": {"$in": [1, 2], "$ne": 2}}]
    # the reference's filter: the or clause is a remaining clause
    ref = {"and": [{"or": [{"indexer": {"$in": ["vector"]}}, {"indexer": {"$exists": False}}]},
                   {"chat_id": "c2"}]}
    rows, rest = plan(ref, index)
    assert rows.tolist() == [1, 3] and rest == [ref["and"][0]]
    # not resolvable: no equality / $in clause on an indexed field among the conjuncts
    for f in (None, {"other": "x"}, {"or": [{"chat_id": "c1"}, {"chat_id": "c2"}]},
              {"not": {"chat_id": "c1"}}, {"chat_id": {"$ne": "c1"}}, {"chat_id": {"$nin": ["c1"]}},
              {"chat_id": {"$exists": True}}, {"n": {"$gt": 0}}, {"chat_id": ["c1"]},
              {"chat_id": {"$in": [["c1"]]}}, {"n": float("nan")}, {"n": {"$in": [1, float("nan")]}},
              {"and": [{"n": {"$gte": 1}}, {"or": [{"chat_id": "c1"}]}]}, [], {}, "chat_id"):
        assert plan(f, index) is None, f


def _random_filter(rng):
    chat = lambda: f"c{int(rng.integers(0, 14))}"
    clause = [
        lambda: {"chat_id": chat()},
        lambda: {"chat_id": {"$eq": chat()}},
        lambda: {"chat_id": {"$in": [chat() for _ in range(int(rng.integers(0, 4)))]}},
        lambda: {"n": int(rng.integers(0, 5))},
        lambda: {"n": {"$in": [int(rng.integers(0, 5)), float(rng.integers(0, 5))]}},
        lambda: {"n": {"$gte": 1}},
        lambda: {"indexer": {"$exists": False}},
        lambda: {"or": [{"indexer": {"$in": ["vector"]}}, {"indexer": {"$exists": False}}]},
        lambda: {"not": {"indexer": "graph"}},
        lambda: {"chat_id": {"$in": [chat(), chat()], "$ne": chat()}},
    ]
    parts = [clause[int(rng.integers(0, len(clause)))]() for _ in range(int(rng.integers(1, 4)))]
    shape = int(rng.integers(0, 4))
    if len(parts) == 1 and shape == 0:
        return parts[0]
    return [{"and": parts}, {"$and": parts}, parts, {"and": [parts[0], {"$and": parts[1:]}]}][shape]


def test_planned_lists_equal_matches_over_random_filters(V):
    from super_rag_amd.filters import matches, plan
    rng = np.random.default_rng(1)
    conn = _conn(V, filter_index=["chat_id", "n"], subset_max_rows=10 ** 9)
    metas = _metas(500, rng)
    ids = conn.add(_nodes(metas, rng.standard_normal((500, 4))))
    conn.delete(ids=ids[::9])                       # deleted rows stay in the lists (device drops them)
    c = V._get("sub")
    md = [m for m in metas]
    resolved = 0
    for _ in range(300):
        f = _random_filter(rng)
        want = [r for r in range(500) if matches(f, md[r])]
        got = V.MI355XVectorStoreConnector._subset_rows(c, f)
        if plan(f, c.findex) is None:
            assert got is None
            continue
        resolved += 1
        live = [r for r in got.tolist() if c.ids[r] is not None]
        assert live == [r for r in want if c.ids[r] is not None], f
        assert (np.diff(got) > 0).all()
    assert 100 < resolved < 300


def _fill_chats(conn, n=600, chats=50, seed=2):
    rng = np.random.default_rng(seed)
    metas = [{"i": i, "chat_id": f"c{i % chats}", **({"indexer": "vector"} if i % 3 else {})}
             for i in range(n)]
    vecs = rng.standard_normal((n, 8))
    conn.add(_nodes(metas, vecs))
    return metas, vecs, rng


def _texts(res):
    return [[(d.text, round(d.score, 12)) for d in r] for r in res]


def test_one_subset_call_for_fifty_filters_and_matches_only_on_posting_rows(V, monkeypatch):
    from super_rag_amd import filters
    conn = _conn(V, filter_index=["chat_id"])
    metas, vecs, rng = _fill_chats(conn)
    c = V._get("sub")
    ref = lambda chat: {"and": [{"or": [{"indexer": {"$in": ["vector"]}}, {"indexer": {"$exists": False}}]},
                                {"chat_id": chat}]}
    items = [(rng.standard_normal(8), 5, ref(f"c{j}")) for j in range(50)]
    calls = {"n": 0, "depth": 0}
    real = filters.matches

    def counting(flt, md):                     # outermost calls only (matches recurses by name)
        calls["n"] += calls["depth"] == 0
        calls["depth"] += 1
        try:
            return real(flt, md)
        finally:
            calls["depth"] -= 1
    monkeypatch.setattr(filters, "matches", counting)
    got = V.MI355XVectorStoreConnector._search_batch(c, items)
    assert c.store.calls == {"search": 0, "search_subset": 1}
    posting_rows = sum(len(c.findex["chat_id"][f"c{j}"]) for j in range(50))
    assert posting_rows == 600 and 0 < calls["n"] <= posting_rows
    # a second batch with the same filters: resolved lists are cached, no metadata is read
    calls["n"] = 0
    V.MI355XVectorStoreConnector._search_batch(c, items[:10] + items[:10])
    assert calls["n"] == 0 and c.store.calls == {"search": 0, "search_subset": 2}
    # one chat only: its 12 rows, not the collection's 600
    c.subsets.clear()
    V.MI355XVectorStoreConnector._search_batch(c, items[3:4])
    assert calls["n"] == 12
    monkeypatch.setattr(filters, "matches", real)
    # same documents as the mask path of a connector without the index
    V._collections.clear()
    plain = _conn(V)
    _fill_chats(plain)
    c0 = V._get("sub")
    want = V.MI355XVectorStoreConnector._search_batch(c0, items)
    assert c0.findex is None and c0.store.calls == {"search": 50, "search_subset": 0}
    assert _texts(got) == _texts(want)
    for j, r in enumerate(got):
        assert 0 < len(r) <= 5 and all(d.metadata["chat_id"] == f"c{j}" for d in r)


def test_routing_fallbacks(V):
    conn = _conn(V, filter_index=["chat_id"], subset_max_rows=12)
    metas, vecs, rng = _fill_chats(conn, n=600, chats=50)
    conn.add(_nodes([{"i": 600, "chat_id": "c0"}], rng.standard_normal((1, 8))))   # c0: 13 rows
    c = V._get("sub")
    q = rng.standard_normal(8)
    SB = V.MI355XVectorStoreConnector._search_batch
    mmr = (0.5, "onepass", 20)
    c.store.search_mmr = lambda Q, k, fetch_k, **kw: (None,) + c.store.search(Q, k, allow=kw["allow"])
    items = [(q, 3, {"chat_id": "c1"}),                 # subset
             (q, 3, {"chat_id": "c0"}),                 # 13 rows > subset_max_rows: mask
             (q, 3, {"chat_id": {"$ne": "c1"}}),        # not resolvable: mask
             (q, 3, None),                              # no filter: plain search
             (q, 3, {"chat_id": "c1"}, mmr),            # diversified: mask path + search_mmr
             (q, 3, {"i": 7}),                          # field not indexed: mask
             (q, 3, {"chat_id": "c1"})]                 # shares the first item's list
    out = SB(c, items)
    assert c.store.calls == {"search": 5, "search_subset": 1}
    assert [d.text for d in out[0]] == [d.text for d in out[6]] == [d.text for d in out[4]]
    assert all(d.metadata["chat_id"] == "c0" for d in out[1]) and len(out[1]) == 3
    assert all(d.metadata["chat_id"] != "c1" for d in out[2])
    assert [d.metadata["i"] for d in out[5]] == [7]
    assert sorted(k for k, v in c.subsets.items() if v[1] is None) == ['{"chat_id": "c0"}']
    # the cache of resolved lists is bounded by rows
    old = V.SUBSET_CACHE_ROWS
    V.SUBSET_CACHE_ROWS = 30
    try:
        c.subset_max_rows = 100
        SB(c, [(q, 3, {"chat_id": f"c{j}"}) for j in range(1, 9)])
        assert sum(len(v[1]) for v in c.subsets.values() if v[1] is not None) <= 30
        assert next(reversed(c.subsets)) == '{"chat_id": "c8"}'
    finally:
        V.SUBSET_CACHE_ROWS = old
    # hybrid and fulltext searches never take the subset path
    from doubles import NumpyLex
    from super_rag_amd.models import QueryWithEmbedding
    V.set_lex_backend(lambda dev: NumpyLex(dev), NumpyLex.load)
    try:
        hy = V.MI355XVectorStoreConnector({"collection": "sub", "honor_filter": True, "hybrid": True,
                                           "filter_index": ["chat_id"]})
        n0 = dict(c.store.calls)
        res = hy.search(QueryWithEmbedding(query="t13", top_k=3, embedding=q.tolist()),
                        filter={"chat_id": "c13"}).results
        hy.fulltext_search("t13", 3, filter={"chat_id": "c13"})
        assert res and all(d.metadata["chat_id"] == "c13" for d in res)
        assert c.store.calls["search_subset"] == n0["search_subset"]
    finally:
        V.set_lex_backend(V._native_lex, V._native_lex_load)


def test_unset_key_or_store_without_search_subset_is_todays_path(V):
    from super_rag_amd.models import QueryWithEmbedding

    class Counting(NumpyStore):
        def __init__(self, dim, device=0):
            super().__init__(dim, device)
            self.n = 0

        def search(self, q, k, allow=None, mask_key=0):
            self.n += 1
            self.last_allow = None if allow is None else np.asarray(allow).copy()
            return super().search(q, k, allow=allow, mask_key=mask_key)

    results = {}
    for name, cls, kw in (("today", Counting, {}),
                          ("index_no_method", Counting, {"filter_index": ["chat_id"]}),
                          ("no_honor_filter", SubsetStore, {"filter_index": ["chat_id"], "honor_filter": False}),
                          ("subset", SubsetStore, {"filter_index": ["chat_id"]})):
        V._collections.clear()
        conn = _conn(V, store_cls=cls, **kw)
        metas, vecs, rng = _fill_chats(conn, n=200, chats=10)
        c = V._get("sub")
        q = QueryWithEmbedding(query="q", top_k=4, embedding=rng.standard_normal(8).tolist())
        res = [conn.search(q, filter={"chat_id": f"c{j}"}).results for j in (1, 2, 1)]
        results[name] = _texts(res)
        if cls is Counting:
            assert c.store.n == 3 and c.store.last_allow.sum() == 20 and len(c.masks) == 2
            assert not hasattr(c.store, "search_subset")
        elif name == "no_honor_filter":
            assert c.findex is None and c.store.calls == {"search": 3, "search_subset": 0}
        else:
            assert c.store.calls == {"search": 0, "search_subset": 3} and not c.masks
    assert results["today"] == results["index_no_method"] == results["subset"]
    assert results["no_honor_filter"] != results["today"]      # the filter is ignored there


def test_sharded_store_splits_lists_and_matches_single_store():
    from super_rag_amd.store import ShardedStore
    rng = np.random.default_rng(5)
    single = SubsetStore(6)
    sh = ShardedStore(6, [0, 0, 0], factory=lambda d, dev: SubsetStore(d, dev))
    for n in (40, 25, 60, 10):
        v = rng.standard_normal((n, 6))
        single.add(v)
        sh.add(v)
    dead = np.arange(3, 135, 7)
    single.remove(dead)
    sh.remove(dead)
    lists = [np.arange(135), np.arange(0, 135, 3), np.asarray([], np.int64), np.asarray([44]),
             np.sort(rng.choice(135, 50, replace=False))]
    q = rng.standard_normal((7, 6))
    ql = np.asarray([0, 1, 2, 3, 4, 4, 1])
    for k in (1, 8, 60):
        d0, r0 = single.search_subset(q, k, lists, q_list=ql)
        d1, r1 = sh.search_subset(q, k, lists, q_list=ql)
        assert np.array_equal(r0, r1)
        np.testing.assert_allclose(d1, d0, atol=1e-6)
        s1, r2 = sh.search_subset(q, k, lists, q_list=ql, sim=True)
        assert np.array_equal(r2, r0) and np.isneginf(s1[r0 < 0]).all()
    assert (r0[2] == -1).all() and r0[3].tolist() == [44] + [-1] * 59
    d, r = sh.search_subset(q[:5], 4, lists)                 # q_list defaults to arange(B)
    assert np.array_equal(r, single.search_subset(q[:5], 4, lists)[1])
    with pytest.raises(ValueError):
        sh.search_subset(q, 4, [np.asarray([135])] * 7)


def test_symbol_declared_exported_and_bound():
    import shutil
    import subprocess
    from super_rag_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "super_rag_mi355x.h")).read(),
                 flags=re.S)
    decl = re.search(r"int\s+sr_store_search_subset\s*\(([^)]*)\)", src)
    assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES["sr_store_search_subset"][1]) == 10
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for path in (_native.library_path(), _native.diag_library_path()):
        out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True,
                             check=True).stdout
        assert "sr_store_search_subset" in {l.split()[-1] for l in out.splitlines()}
    lib = _native.load()
    # arguments are checked before any device work: no store -> SR_ERR_INVALID without a GPU
    assert lib.sr_store_search_subset(None, None, 1, 1, None, 1, None, None, None, None) == _native.SR_ERR_INVALID
