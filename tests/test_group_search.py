"""CPU: grouped search (the k best distinct groups with the best rows of each): the walk of
tests/group_ref.py on hand-made rankings, the C entry point's declaration / export / argument check,
the connector's ``group_by`` bookkeeping and routing against a numpy store double, and
ShardedStore.search_grouped over two such doubles.  The kernels are tested in test_gpu_group.py."""
import os
import re

import numpy as np
import pytest

import group_ref as R
from doubles import NumpyStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


# -- the reference walk -------------------------------------------------------------------------
def _walk(group, k, gsz, sims=None):
    """Rows 0 .. n - 1 ranked in that order (descending similarities unless given)."""
    n = len(group)
    sims = np.linspace(0.9, 0.1, n) if sims is None else np.asarray(sims, float)
    return R.group_walk(sims, np.arange(n), np.asarray(group), k, gsz)


def test_walk_all_groups_distinct():
    s, r, g = _walk([5, 4, 3, 2, 1], 3, 1)
    assert r.tolist() == [[0], [1], [2]] and g.tolist() == [5, 4, 3]
    assert s[:, 0].tolist() == pytest.approx([0.9, 0.7, 0.5])


def test_walk_single_group():
    s, r, g = _walk([7] * 6, 3, 2)
    assert r.tolist() == [[0, 1], [-1, -1], [-1, -1]] and g.tolist() == [7, -1, -1]
    assert np.isneginf(s[1:]).all() and np.isfinite(s[0]).all()


def test_walk_mix_with_ungrouped_rows():
    # -1 rows are groups of their own: rows 1 and 3 take a slot each and never a second row
    s, r, g = _walk([2, -1, 2, -1, 9, 2, 9], 4, 2)
    assert r.tolist() == [[0, 2], [1, -1], [3, -1], [4, 6]]
    assert g.tolist() == [2, -1, -1, 9]
    # an unfilled group slot is told from an ungrouped row's by its first row
    s, r, g = _walk([2, -1], 3, 1)
    assert g.tolist() == [2, -1, -1] and r[:, 0].tolist() == [0, 1, -1]


def test_walk_group_size_and_group_cap():
    # group 1 appears first; k = 2 groups are 1 and 2: group 3 is never kept, however good its rows
    s, r, g = _walk([1, 2, 3, 3, 1, 2, 1, 1], 2, 3)
    assert g.tolist() == [1, 2] and r.tolist() == [[0, 4, 6], [1, 5, -1]]
    # rows past group_size are dropped although the group is kept
    assert 7 not in r


def test_walk_fewer_than_k_groups_and_ties():
    s, r, g = _walk([4, 4, 6], 5, 2)
    assert g.tolist() == [4, 6, -1, -1, -1] and r.tolist() == [[0, 1], [2, -1]] + [[-1, -1]] * 3
    # equal similarities: row asc decides (ranking sorts; group_walk takes the order it is given)
    sims, rows = R.ranking([0.5, 0.5, 0.5, 0.8], [3, 1, 2, 0])
    assert rows.tolist() == [0, 1, 2, 3]
    out = R.grouped_search(np.array([[0.5, 0.5, 0.5, 0.8, 0.0]]), np.array([[3, 1, 2, 0, -1]]),
                           np.array([9, 8, 9, 8]), 2, 1)
    assert out[1][0].tolist() == [[0], [1]] and out[2][0].tolist() == [9, 8]
    with pytest.raises(ValueError):
        _walk([0, -2], 1, 1)


# -- the C entry point ----------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    import shutil
    import subprocess
    from super_rag_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "super_rag_mi355x.h")).read(), flags=re.S)
    for name, arity in (("sr_store_search_grouped", 13), ("sr_store_group_dev", 15)):
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", src)
        assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]) == arity
    assert re.search(r"#define\s+SR_GROUP_MAX_SIZE\s+8\b", src) and _native.SR_GROUP_MAX_SIZE == 8
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for path in (_native.library_path(), _native.diag_library_path()):
        out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True,
                             check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines()}
        assert {"sr_store_search_grouped", "sr_store_group_dev"} <= exported
    lib = _native.load()
    # arguments are checked before any device work: no store -> SR_ERR_INVALID without a GPU
    assert lib.sr_store_search_grouped(None, None, 1, 1, 1, 1, None, 0, None, 0, None, None,
                                       None) == _native.SR_ERR_INVALID
    assert lib.sr_store_group_dev(None, None, None, 1, 1, 0, 1, 1, None, 0, None, None, None, None,
                                  None) == _native.SR_ERR_INVALID


# -- the connector ----------------------------------------------------------------------------------
class GroupStore(NumpyStore):
    """NumpyStore + search_grouped (the walk over the complete fp64 ranking), recording calls."""

    def __init__(self, dim, device=0):
        super().__init__(dim, device)
        self.calls = []

    def search(self, q, k, allow=None, mask_key=0):
        self.calls.append(("search", len(q), k))
        return super().search(q, k, allow=allow, mask_key=mask_key)

    def search_grouped(self, queries, k, group, group_size=1, fetch_k=None, allow=None, mask_key=0,
                       group_key=0, sim=False):
        n = len(self.rows)
        group = np.asarray(group)
        assert group.shape == (n,) and group.dtype == np.int32
        self.calls.append(("search_grouped", len(queries), k, group_size, fetch_k, allow is not None,
                           group_key, group.copy()))
        d, r = NumpyStore.search(self, queries, max(n, 1), allow=allow)
        s, rows, groups = R.grouped_search(np.where(r >= 0, 1.0 - d, -INF), r, group, k, group_size)
        return (s if sim else np.where(rows >= 0, 1.0 - s, INF)), rows, groups


@pytest.fixture
def V():
    from super_rag_amd import vectorstore as V
    V._collections.clear()
    yield V
    V._collections.clear()
    V.set_store_backend(V._native_store, V._native_load)


def _conn(V, store_cls=GroupStore, **kw):
    V.set_store_backend(lambda dim, dev: store_cls(dim, dev), store_cls.load)
    return V.MI355XVectorStoreConnector({"collection": "grp", "coalesce": False, **kw})


def _nodes(metas, vecs):
    from super_rag_amd.models import TextNode
    return [TextNode(text=f"t{m['i']}", metadata=m, embedding=v.tolist()) for m, v in zip(metas, vecs)]


def _metas(n, rng, first=0):
    out = []
    for i in range(first, first + n):
        m = {"i": i}
        u = rng.random()
        if u < 0.7:
            m["document_id"] = f"d{int(rng.integers(0, 9))}"
        elif u < 0.8:
            m["document_id"] = ["d1", "d2"]          # unhashable: a group of its own
        elif u < 0.85:
            m["document_id"] = float("nan")          # equals nothing: a group of its own
        m["part"] = int(rng.integers(0, 3))
        out.append(m)
    return out


def _brute_ids(c, field):
    """Group ids from the metadata alone: same value <=> same id, no value <=> -1 (a tombstoned row,
    whose metadata is gone, is skipped)."""
    from super_rag_amd.filters import indexable
    key, arr = c.group_array(field)
    assert arr.dtype == np.int32 and arr.shape == (len(c.metadatas),) and key > 0
    seen = {}
    for r, md in enumerate(c.metadatas):
        if md is None:
            continue
        v = md.get(field)
        if v is None or not indexable(v):
            assert arr[r] == -1, (r, v)
        else:
            assert arr[r] >= 0 and seen.setdefault(v, arr[r]) == arr[r], (r, v)
    assert len(set(seen.values())) == len(seen)
    return key, arr


def _query(vec, top_k):
    from super_rag_amd.models import QueryWithEmbedding
    return QueryWithEmbedding(query="q", top_k=top_k, embedding=np.asarray(vec).tolist())


def test_group_ids_follow_add_delete_compaction_and_restore(V, tmp_path):
    rng = np.random.default_rng(0)
    conn = _conn(V, group_by="document_id", snapshot_dir=str(tmp_path), compact_ratio=0.5)
    metas = _metas(300, rng)
    vecs = rng.standard_normal((300, 8))
    ids = conn.add(_nodes(metas[:100], vecs[:100]))
    c = V._get("grp")
    k0, a0 = _brute_ids(c, "document_id")
    assert c.group_array("document_id")[0] == k0            # unchanged array: the same serial key
    ids += conn.add(_nodes(metas[100:], vecs[100:]))
    k1, a1 = _brute_ids(c, "document_id")
    assert k1 != k0 and np.array_equal(a1[:100], a0) and (a1 == -1).any()
    # delete leaves the ids alone (tombstoned rows are dropped on the device)
    conn.delete(ids=ids[:50])
    k2, a2 = _brute_ids(c, "document_id")
    assert np.array_equal(a2, a1) and k2 == k1 and c.store.count() == (300, 250)
    # auto-compaction (more than half the rows dead) renumbers the rows: the survivors keep their ids
    conn.delete(ids=ids[50:170])
    assert c.store.count() == (130, 130)
    k3, a3 = _brute_ids(c, "document_id")
    assert np.array_equal(a3, a1[170:]) and k3 != k2
    # restart from the snapshot: rebuilt from the restored metadata; the snapshot holds no ids
    V._collections.clear()
    conn2 = _conn(V, group_by="document_id", snapshot_dir=str(tmp_path))
    c2 = V._get("grp")
    assert c2 is not c and len(c2.metadatas) == 130
    _, b0 = _brute_ids(c2, "document_id")
    assert np.array_equal(b0 == -1, a3 == -1)
    conn2.add(_nodes(_metas(7, rng, first=300), vecs[:7]))
    _brute_ids(c2, "document_id")
    # a per-call kwarg naming another field back-fills it
    conn2.search(_query(vecs[0], 2), group_by="part")
    _, p = _brute_ids(c2, "part")
    assert (p >= 0).all() and len(set(p.tolist())) == 3


def test_flattening_order_kwarg_overrides_and_threshold(V):
    rng = np.random.default_rng(1)
    conn = _conn(V, group_by="document_id", group_size=2, honor_score_threshold=True)
    metas = _metas(200, rng)
    vecs = rng.standard_normal((200, 8))
    conn.add(_nodes(metas, vecs))
    c = V._get("grp")
    _, garr = c.group_array("document_id")
    q = rng.standard_normal(8)
    d, r = NumpyStore.search(c.store, q[None], 200)
    s_ref, r_ref, g_ref = R.grouped_search(1.0 - d, r, garr, 4, 2)
    res = conn.search(_query(q, 4)).results
    # group by group, best group first, a group's rows by distance ascending; top_k counts groups
    assert [x.metadata["i"] for x in res] == [int(x) for x in r_ref[0].reshape(-1) if x >= 0]
    assert 4 <= len(res) <= 8
    assert [x.score for x in res] == pytest.approx([1.0 - s for s in s_ref[0].reshape(-1) if np.isfinite(s)])
    for j in range(4):
        part = [x.score for x in res if x.metadata["i"] in r_ref[0, j].tolist()]
        assert part == sorted(part)
    call = c.store.calls[-1]
    assert call[:6] == ("search_grouped", 1, 4, 2, 64, False) and call[6] == c.group_array("document_id")[0]
    # kwargs override the ctx keys
    res1 = conn.search(_query(q, 4), group_size=1, group_fetch_k=500).results
    assert c.store.calls[-1][:5] == ("search_grouped", 1, 4, 1, 500)
    assert [x.metadata["i"] for x in res1] == r_ref[0, :, 0].tolist()
    conn.search(_query(q, 30), group_size=8)
    assert c.store.calls[-1][4] == 960                       # default min(1024, max(4 k g, 64))
    conn.search(_query(q, 100), group_size=8)
    assert c.store.calls[-1][4] == 1024
    conn.search(_query(q, 3), group_fetch_k=2)
    assert c.store.calls[-1][4] == 6                         # never below top_k group_size
    by_part = conn.search(_query(q, 3), group_by="part", group_size=1).results
    assert sorted(x.metadata["part"] for x in by_part) == [0, 1, 2]
    # score_threshold filters rows (not a prefix cut): rows of a later group may pass
    thr = 1.0 - float(np.sort([x.score for x in res])[2])
    kept = conn.search(_query(q, 4), score_threshold=thr).results
    assert [x.metadata["i"] for x in kept] == [x.metadata["i"] for x in res if 1.0 - x.score >= thr]
    assert len(kept) == 3
    # group_by off for one call: today's plain search
    plain = conn.search(_query(q, 4), group_by=None).results
    assert [x.metadata["i"] for x in plain] == r[0, :4].tolist() and c.store.calls[-1][0] == "search"


def test_value_errors_and_store_without_search_grouped(V):
    rng = np.random.default_rng(2)
    with pytest.raises(ValueError, match="hybrid and group_by cannot be combined"):
        _conn(V, group_by="document_id", hybrid=True)
    with pytest.raises(ValueError, match="diversify and group_by cannot be combined"):
        _conn(V, group_by="document_id", diversify="mmr")
    conn = _conn(V, group_by="document_id")
    metas = _metas(40, rng)
    vecs = rng.standard_normal((40, 8))
    conn.add(_nodes(metas, vecs))
    with pytest.raises(ValueError, match="diversify and group_by"):
        conn.search(_query(vecs[0], 3), diversify="mmr")
    with pytest.raises(ValueError, match="hybrid and group_by"):
        _conn(V, hybrid=True).search(_query(vecs[0], 3), group_by="document_id")
    for bad in (0, 9):
        with pytest.raises(ValueError, match="group_size must be in"):
            conn.search(_query(vecs[0], 3), group_size=bad)
    with pytest.raises(ValueError, match="exceeds the cap"):
        conn.search(_query(vecs[0], 200), group_size=8)
    with pytest.raises(ValueError, match="group_fetch_k 2000 exceeds the cap"):
        conn.search(_query(vecs[0], 3), group_fetch_k=2000)
    # a store without search_grouped: a clear error, never a silent fallback
    V._collections.clear()
    plain = _conn(V, store_cls=NumpyStore, group_by="document_id")
    plain.add(_nodes(metas, vecs))
    with pytest.raises(RuntimeError, match="search_grouped"):
        plain.search(_query(vecs[0], 3))
    assert len(plain.search(_query(vecs[0], 3), group_by=None).results) == 3


def test_ungrouped_items_stay_todays_tuples_and_grouped_items_batch_per_grouping(V):
    rng = np.random.default_rng(3)
    conn = _conn(V, honor_filter=True)
    metas = _metas(120, rng)
    vecs = rng.standard_normal((120, 8))
    conn.add(_nodes(metas, vecs))
    c = V._get("grp")
    assert c.gindex is None                                   # nothing kept until a connector asks
    q = rng.standard_normal((6, 8))
    assert conn._group_params({}, 5) is None
    assert conn._item(q[0], 5, None, None)[1:] == (5, None)
    assert conn._item(q[0], 5, None, (0.5, "onepass", 20))[1:] == (5, None, (0.5, "onepass", 20))
    grp = conn._group_params({"group_by": "document_id", "group_size": 2}, 5)
    assert grp == ("document_id", 2, 64)
    assert conn._item(q[0], 5, None, None, grp)[1:] == (5, None, None, grp)
    flt = {"part": 1}
    items = [(q[0], 3, None), (q[1], 5, None, None, grp), (q[2], 4, None, None, grp), (q[3], 2, flt),
             (q[4], 5, flt, None, grp), (q[5], 5, None, None, ("part", 1, 64))]
    c.store.calls.clear()
    out = V.MI355XVectorStoreConnector._search_batch(c, items)
    calls = sorted(x[:6] for x in c.store.calls)
    # one grouped search per (filter, grouping); items 1 and 2 share one with k = max; the filtered
    # grouped item takes the mask path
    assert calls == [("search", 1, 2), ("search", 1, 3), ("search_grouped", 1, 5, 1, 64, False),
                     ("search_grouped", 1, 5, 2, 64, True), ("search_grouped", 2, 5, 2, 64, False)]
    _, garr = c.group_array("document_id")
    for i, k in ((1, 5), (2, 4)):
        d, r = NumpyStore.search(c.store, q[i:i + 1], 120)
        ref = R.grouped_search(1.0 - d, r, garr, k, 2)
        assert [x.metadata["i"] for x in out[i]] == [int(x) for x in ref[1][0].reshape(-1) if x >= 0]
    assert all(x.metadata["part"] == 1 for x in out[4]) and len(out[4]) >= 5
    assert len(out[0]) == 3 and len(out[3]) == 2 and len(out[5]) == 3
    # coalesced searches batch the same way
    co = _conn(V, coalesce=True, group_by="document_id", group_size=2)
    res = co.search(_query(q[1], 5)).results
    assert [x.metadata["i"] for x in res] == [x.metadata["i"] for x in out[1]]


# -- ShardedStore -----------------------------------------------------------------------------------
def test_sharded_grouped_search_equals_the_walk_over_the_union():
    from super_rag_amd.store import ShardedStore
    rng = np.random.default_rng(5)
    n, dim = 400, 8
    x = rng.standard_normal((n, dim))
    single = GroupStore(dim)
    sh = ShardedStore(dim, [0, 1], factory=lambda d, dev: GroupStore(d, dev))
    for a, b in ((0, 150), (150, 170), (170, 330), (330, n)):        # batches alternate shards
        single.add(x[a:b])
        sh.add(x[a:b])
    assert len(set(sh.shard_of.tolist())) == 2
    dead = np.arange(3, n, 13)
    single.remove(dead)
    sh.remove(dead)
    # groups whose rows straddle both shards; a fifth of the rows ungrouped
    group = np.where(rng.random(n) < 0.2, -1, rng.integers(0, 12, n)).astype(np.int32)
    allow = rng.random(n) < 0.7
    q = rng.standard_normal((5, dim))
    for k, gsz, al in ((3, 1, None), (4, 3, None), (12, 8, None), (5, 2, allow)):
        want = single.search_grouped(q, k, group, group_size=gsz, allow=al, sim=True)
        got = sh.search_grouped(q, k, group, group_size=gsz, allow=al, sim=True)
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
        ok = want[1] >= 0
        np.testing.assert_allclose(got[0][ok], want[0][ok], atol=1e-6)
        assert np.isneginf(got[0][~ok]).all() and got[0].dtype == np.float32
        d, r, g = sh.search_grouped(q, k, group, group_size=gsz, allow=al)
        assert np.array_equal(r, want[1]) and np.isposinf(d[~ok]).all()
        np.testing.assert_allclose(d[ok], 1.0 - want[0][ok], atol=1e-6)
    # the later rows of a kept group may sit in a shard where the group is not among the k best:
    # the case the second pass exists for shows up in this data
    first = [s_.search_grouped(q, 4, group[sh.tables[i]], group_size=3, sim=True)[1] for i, s_ in enumerate(sh.shards)]
    union = np.concatenate([np.where(r >= 0, sh.tables[i][np.clip(r, 0, None)], -1).reshape(5, -1)
                            for i, r in enumerate(first)], axis=1)
    want = single.search_grouped(q, 4, group, group_size=3, sim=True)[1]
    assert any(not np.isin(want[b][want[b] >= 0], union[b]).all() for b in range(5))
    with pytest.raises(ValueError):
        sh.search_grouped(q, 3, group[:-1])
