"""GPU: batched subset search (k_subset.hip; sr_store_search_subset / NativeStore.search_subset /
ShardedStore.search_subset / the connector's ctx "filter_index" route).

Every query searches only the rows of its own list.  Two references:
  * the CPU oracle on the rows read back from the store and identically quantised queries, exactly
    as test_gpu_store._check does, with live = indicator(list) & live; band EPS = 1e-4 (fp16 query
    rounding, test_gpu_store.py:20-22);
  * the masked search of the same store (store.search(q, k, allow=indicator(list))): device against
    device, band 1e-6 (test_gpu_store.py:196).
Largest differences observed on an MI355X over this file (distances): 4.2e-5 against the oracle, 0
against the masked search (every subset result was bit-identical to it).
"""
import functools

import numpy as np
import pytest

from oracle.cosine_topk import cosine_topk, quantize_like_store, same_topk_modulo_ties

pytestmark = pytest.mark.gpu

EPS = 1e-4          # against the oracle: fp16 query rounding (test_gpu_store.py:20-22)
DEV = 1e-6          # device against device (test_gpu_store.py:196)
CHUNK = 512         # list rows per work item of subset_scan
CAP = 16384         # select_capacity()
OBSERVED = {"oracle": 0.0, "device": 0.0}


def _clustered(n, dim, seed, centers=64):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, dim)).astype(np.float32)
    return c[np.arange(n) % centers] + 0.5 * rng.standard_normal((n, dim)).astype(np.float32)


def _queries(x, b, seed, noise=0.3):
    rng = np.random.default_rng(seed)
    base = x[rng.integers(0, x.shape[0], b)]
    u = rng.standard_normal(base.shape).astype(np.float32)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return base / np.linalg.norm(base, axis=1, keepdims=True) + noise * u


def _new_store(x):
    from super_rag_amd.store import NativeStore
    s = NativeStore(x.shape[1], device=0)
    s.add(x)
    return s


@functools.lru_cache(maxsize=None)
def _base(dim, n):
    """A store that the tests only read, its rows and the rows as stored (fp64), built once."""
    x = _clustered(n, dim, seed=dim + n)
    s = _new_store(x)
    return s, x, s.get(np.arange(n)).astype(np.float64)


def _sublist(n, length, seed):
    return np.sort(np.random.default_rng(seed).choice(n, length, replace=False)).astype(np.int64)


def _indicator(n, rows):
    m = np.zeros(n, bool)
    m[np.asarray(rows, dtype=np.int64)] = True
    return m


def _check(store, stored, q, k, lists, ql=None, live=None, device_lists=40):
    """search_subset against the oracle (every query) and the masked search (up to ``device_lists``
    distinct lists); returns (sim, rows)."""
    n = stored.shape[0]
    B = len(q)
    ql = np.arange(B) if ql is None else np.asarray(ql)
    live = np.ones(n, bool) if live is None else live
    s_gpu, r_gpu = store.search_subset(q, k, lists, q_list=ql, sim=True)
    d_gpu, r_d = store.search_subset(q, k, lists, q_list=ql)
    assert np.array_equal(r_d, r_gpu)
    np.testing.assert_array_equal(d_gpu, np.where(r_gpu >= 0, np.float32(1.0) - s_gpu, np.inf))
    assert s_gpu.dtype == np.float32 and r_gpu.dtype == np.int64 and s_gpu.shape == (B, k)
    qq = quantize_like_store(q).astype(np.float64)
    for b in range(B):
        elig = _indicator(n, lists[ql[b]]) & live
        d_ref, r_ref = cosine_topk(stored, qq[b:b + 1], k, live=elig, normalize=False)
        s_ref = np.where(r_ref >= 0, 1.0 - d_ref, -np.inf)
        sg = s_gpu[b:b + 1].astype(np.float64)
        assert same_topk_modulo_ties(r_gpu[b:b + 1], sg, r_ref, s_ref, EPS), b
        ok = r_ref[0] >= 0
        assert np.array_equal(r_gpu[b] >= 0, ok), b
        assert ok.sum() == min(k, int(elig.sum()))
        assert (r_gpu[b][~ok] == -1).all() and np.isneginf(s_gpu[b][~ok]).all()
        assert np.isposinf(d_gpu[b][~ok]).all()
        if ok.any():
            OBSERVED["oracle"] = max(OBSERVED["oracle"], float(np.abs(d_gpu[b][ok] - d_ref[0][ok]).max()))
        np.testing.assert_allclose(d_gpu[b][ok], d_ref[0][ok], atol=EPS)
        assert elig[r_gpu[b][ok]].all()
        key = list(zip((-s_gpu[b][ok]).tolist(), r_gpu[b][ok].tolist()))
        assert key == sorted(key), b                     # (sim desc, row asc), exactly
    for l in np.unique(ql)[:device_lists]:
        sel = np.nonzero(ql == l)[0]
        d_m, r_m = store.search(q[sel], k, allow=_indicator(n, lists[l]))
        s_m = np.where(r_m >= 0, 1.0 - d_m.astype(np.float64), -np.inf)
        sg = np.where(r_gpu[sel] >= 0, 1.0 - d_gpu[sel].astype(np.float64), -np.inf)
        assert same_topk_modulo_ties(r_gpu[sel], sg, r_m, s_m, DEV), l
        ok = r_m >= 0
        assert np.array_equal(r_gpu[sel] >= 0, ok)
        if ok.any():
            OBSERVED["device"] = max(OBSERVED["device"], float(np.abs(d_gpu[sel][ok] - d_m[ok]).max()))
        np.testing.assert_allclose(d_gpu[sel][ok], d_m[ok], atol=DEV)
    print(f"observed max |d - oracle| {OBSERVED['oracle']:.3e}  max |d - masked| {OBSERVED['device']:.3e}")
    return s_gpu, r_gpu


@pytest.mark.parametrize("dim,n", [(64, 3000), (100, 3000), (768, 3000), (2100, 700)])
def test_list_lengths_and_column_tile_edges(dim, n):
    # lengths 0 / 1 / 15 / 16 / 17 and one below / at / one above the 512-row chunk; 1, 16 and 17
    # queries sharing a list (one, one full and two column tiles) mixed with singletons; k = 20 is
    # above the short lengths (padding) and below the long ones.  dim 100 pads to 128; dim 2100
    # (ld 2112 > 2048) takes the kernel without the LDS-resident queries.
    s, x, stored = _base(dim, n)
    lengths = [0, 1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, min(n, 2 * CHUNK + 37), 40, 300]
    lists = [_sublist(n, L, seed=L + dim) for L in lengths]
    ql = list(range(9)) + [9] * 16 + [10] * 17 + [4, 0, 7]
    q = _queries(x, len(ql), seed=dim)
    _check(s, stored, q, 20, lists, ql)


def test_one_list_per_query_default_q_list_and_k_edges():
    s, x, stored = _base(64, 3000)
    lists = [_sublist(3000, L, seed=L) for L in (5, 700, 33)]
    q = _queries(x, 3, seed=1)
    s0, r0 = _check(s, stored, q, 1, lists)
    s1, r1 = s.search_subset(q, 1, lists, sim=True)               # q_list = arange(B)
    assert np.array_equal(r0, r1) and np.array_equal(s0, s1)
    _check(s, stored, q, 1024, lists)                              # k far above two of the lists
    assert s.search_subset(np.zeros((0, 64), np.float32), 5, [])[1].shape == (0, 5)   # B == 0
    with pytest.raises(ValueError):
        s.search_subset(q, 5, lists[:2])
    with pytest.raises(Exception):
        s.search_subset(q, 1025, lists)


def test_long_list_takes_two_select_passes():
    # 16,500 rows with k = 100: more than cap - k = 16,284, so the second pass scores the last 216
    # rows behind the first pass's 100 winners; a second, short list and an empty one share the block
    n, k = 20_000, 100
    assert 16_500 > CAP - k
    s, x, stored = _base(64, n)
    lists = [_sublist(n, 16_500, seed=7), _sublist(n, 90, seed=8), np.zeros(0, np.int64)]
    ql = [0, 1, 2, 0] + [1] * 3
    q = _queries(x, len(ql), seed=9)
    # the best row of query 3 is the LAST row of the long list: it only arrives in pass two
    q[3] = x[lists[0][-1]]
    _, r = _check(s, stored, q, k, lists, ql)
    assert r[3][0] == lists[0][-1]


def test_b300_crosses_the_query_block():
    s, x, stored = _base(64, 3000)
    rng = np.random.default_rng(11)
    lists = [_sublist(3000, int(L), seed=100 + i) for i, L in enumerate(rng.integers(0, 600, 60))]
    ql = rng.integers(0, 60, 300)
    q = _queries(x, 300, seed=12)
    _check(s, stored, q, 10, lists, ql, device_lists=12)


def test_tombstones_then_compaction():
    n, k = 20_000, 50
    x = _clustered(n, 64, seed=21)
    s = _new_store(x)
    stored = s.get(np.arange(n)).astype(np.float64)
    long_list = _sublist(n, 16_500, seed=22)
    lists = [_sublist(n, 400, seed=23), _sublist(n, 30, seed=24), long_list, _sublist(n, 600, seed=25)]
    dead = np.unique(np.concatenate([lists[0][::3], lists[1],          # list 1: every row dead
                                     long_list[:16_460],                # pass one of the long list: all dead
                                     np.arange(1, n, 41)]))
    s.remove(dead)
    live = ~_indicator(n, dead)
    ql = [0, 1, 2, 3, 0, 2]
    q = _queries(x, len(ql), seed=26)
    assert 16_460 > CAP - k
    _, r = _check(s, stored, q, k, lists, ql, live=live)
    assert (r[1] == -1).all() and not np.isin(r, dead).any()
    assert (r[2] >= 0).sum() == int(live[long_list].sum()) < k        # pass two starts from < k winners
    # compact, remap the lists, search again: the same rows under their new ids
    m = s.compact()
    assert s.count() == (int(live.sum()), int(live.sum()))
    lists2 = [m[l][m[l] >= 0] for l in lists]
    stored2 = s.get(np.arange(int(live.sum()))).astype(np.float64)
    _, r2 = _check(s, stored2, q, k, lists2, ql)
    assert np.array_equal(np.where(r >= 0, m[np.maximum(r, 0)], -1), r2)


def test_fp8_scan_mode_is_bit_identical():
    n = 6000
    x = _clustered(n, 768, seed=31)
    s = _new_store(x)
    s.remove(np.arange(0, n, 13))
    lists = [_sublist(n, L, seed=L) for L in (3, 511, 1500, 64)]
    ql = [0, 1, 2, 3, 2, 2]
    q = _queries(x, len(ql), seed=32)
    s16, r16 = s.search_subset(q, 40, lists, q_list=ql, sim=True)
    s.set_scan_dtype("fp8")
    s8, r8 = s.search_subset(q, 40, lists, q_list=ql, sim=True)
    s.add(x[:5])                                   # rows added in fp8 mode are searched the same way
    lists[0] = np.concatenate([lists[0], [n, n + 4]])
    s8b, r8b = s.search_subset(q, 40, lists, q_list=ql, sim=True)
    s.set_scan_dtype("fp16")
    s16b, r16b = s.search_subset(q, 40, lists, q_list=ql, sim=True)
    assert np.array_equal(r8, r16) and np.array_equal(s8.view(np.uint32), s16.view(np.uint32))
    assert np.array_equal(r8b, r16b) and np.array_equal(s8b.view(np.uint32), s16b.view(np.uint32))
    assert n in r8b[0] or n + 4 in r8b[0]


def _raw(store, q, k, ql, off, rows):
    """sr_store_search_subset on raw arrays; (return code, out_sim, out_rows) with sentinels."""
    from super_rag_amd import _native as N
    q = np.ascontiguousarray(q, np.float32)
    ql = np.ascontiguousarray(ql, np.int32)
    off = np.ascontiguousarray(off, np.int64)
    rows = np.ascontiguousarray(rows, np.int64)
    out_s = np.full((len(q), k), 7.5, np.float32)
    out_r = np.full((len(q), k), -77, np.int64)
    rc = N.load().sr_store_search_subset(store._h, N.ptr(q), len(q), k, N.ptr(ql), len(off) - 1,
                                         N.ptr(off), N.ptr(rows), N.ptr(out_s), N.ptr(out_r))
    return rc, out_s, out_r


def test_invalid_input_is_rejected_before_any_result():
    from super_rag_amd import _native as N
    s, x, _ = _base(64, 3000)
    q = _queries(x, 2, seed=41)
    good = dict(ql=[0, 1], off=[0, 3, 5], rows=[1, 5, 9, 0, 2999])
    rc, out_s, out_r = _raw(s, q, 4, **good)
    assert rc == N.SR_OK and sorted(out_r[0, :3].tolist()) == [1, 5, 9] and (out_r[:, 3] == -1).all()
    bad = {
        "unsorted list": dict(good, rows=[1, 9, 5, 0, 2999]),
        "duplicated row": dict(good, rows=[1, 5, 5, 0, 2999]),
        "row == n_rows": dict(good, rows=[1, 5, 9, 0, 3000]),
        "negative row": dict(good, rows=[-1, 5, 9, 0, 2999]),
        "q_list past the lists": dict(good, ql=[0, 2]),
        "negative q_list": dict(good, ql=[-1, 1]),
        "list_off[0] != 0": dict(good, off=[1, 3, 5]),
        "decreasing list_off": dict(good, off=[0, 4, 3]),
    }
    for name, args in bad.items():
        rc, out_s, out_r = _raw(s, q, 4, **args)
        assert rc == N.SR_ERR_INVALID, name
        assert (out_s == 7.5).all() and (out_r == -77).all(), name
    for k in (0, 1025):
        assert _raw(s, q, k, **good)[0] == N.SR_ERR_INVALID
    with pytest.raises(N.NativeError) as e:
        s.search_subset(q, 4, [[3, 2], [1]])
    assert e.value.code == N.SR_ERR_INVALID and "ascending" in e.value.message
    d, r = s.search(q, 4)                                   # the store is unharmed
    assert (r >= 0).all()


def test_sharded_store_equals_single_store():
    from super_rag_amd.store import ShardedStore
    n, dim, k = 6000, 64, 30
    x = _clustered(n, dim, seed=51)
    from super_rag_amd.store import NativeStore
    single = NativeStore(dim, device=0)
    sh = ShardedStore(dim, [0, 0])
    for a, b in ((0, 2500), (2500, 2600), (2600, 4800), (4800, 6000)):   # batches alternate shards
        single.add(x[a:b])
        sh.add(x[a:b])
    assert len(set(sh.shard_of.tolist())) == 2
    dead = np.arange(7, n, 17)
    single.remove(dead)
    sh.remove(dead)
    lists = [_sublist(n, L, seed=50 + L) for L in (0, 1, 17, 513, 3000)] + [np.arange(2400, 2700)]
    assert all(len(set(sh.shard_of[l].tolist())) == 2 for l in lists[2:])   # straddle both shards
    ql = [0, 1, 2, 3, 4, 5, 4, 3]
    q = _queries(x, len(ql), seed=52)
    stored = single.get(np.arange(n)).astype(np.float64)
    _check(single, stored, q, k, lists, ql, live=~_indicator(n, dead))
    for sim in (True, False):
        v0, r0 = single.search_subset(q, k, lists, q_list=ql, sim=sim)
        v1, r1 = sh.search_subset(q, k, lists, q_list=ql, sim=sim)
        s0 = v0.astype(np.float64) if sim else np.where(r0 >= 0, 1.0 - v0.astype(np.float64), -np.inf)
        s1 = v1.astype(np.float64) if sim else np.where(r1 >= 0, 1.0 - v1.astype(np.float64), -np.inf)
        assert same_topk_modulo_ties(r1, s1, r0, s0, DEV)
        ok = r0 >= 0
        assert np.array_equal(r1 >= 0, ok)
        np.testing.assert_allclose(v1[ok], v0[ok], atol=DEV)
        assert v1.dtype == np.float32
        assert (np.isneginf(v1[~ok]) if sim else np.isposinf(v1[~ok])).all()
    sh.close()


def test_connector_batch_of_forty_filters_is_one_subset_scan():
    from super_rag_amd import _native as N
    from super_rag_amd import vectorstore as V
    from super_rag_amd.context import ContextManager
    from super_rag_amd.models import TextNode
    n, dim, chats = 3000, 64, 40
    rng = np.random.default_rng(61)
    x = _clustered(n, dim, seed=62)
    metas = []
    for i in range(n):
        m = {"i": i, "chat_id": f"c{int(rng.integers(0, chats))}"}
        r = rng.random()
        if r < 0.5:
            m["indexer"] = "vector"
        elif r < 0.7:
            m["indexer"] = "graph"
        metas.append(m)
    nodes = [TextNode(text=f"t{i}", metadata=m, embedding=v.tolist()) for i, (m, v) in enumerate(zip(metas, x))]
    cm = ContextManager.__new__(ContextManager)
    flts = [cm._create_combined_filter(["vector"], f"c{j}") for j in range(chats)]
    assert "and" in flts[0] and "or" in flts[0]["and"][0]            # the reference's shape
    items = [(q, 10, f) for q, f in zip(_queries(x, chats, seed=63), flts)]
    V._collections.pop("subset_gpu_a", None)
    V._collections.pop("subset_gpu_b", None)
    try:
        a = V.MI355XVectorStoreConnector({"collection": "subset_gpu_a", "honor_filter": True,
                                          "filter_index": ["chat_id"]})
        b = V.MI355XVectorStoreConnector({"collection": "subset_gpu_b", "honor_filter": True})
        ids = a.add(nodes)
        b.add(nodes)
        a.delete(ids=ids[5:400:9])
        b.delete(ids=[u for u in (V._get("subset_gpu_b").ids[r] for r in range(5, 400, 9))])
        ca, cb = V._get("subset_gpu_a"), V._get("subset_gpu_b")
        N.profile_enable(True)
        got = V.MI355XVectorStoreConnector._search_batch(ca, items)
        stats = N.profile_read()
        N.profile_enable(False)
        assert stats["subset_scan"]["launches"] == 1, stats.keys()
        assert not [name for name in stats if name.startswith("cosine_scan")], stats.keys()
        want = V.MI355XVectorStoreConnector._search_batch(cb, items)
        assert len(cb.masks) == V.MASK_CACHE_SIZE and not ca.masks
        for j, (g, w) in enumerate(zip(got, want)):
            assert 0 < len(w) <= 10 and len(g) == len(w)
            assert all(d.metadata["chat_id"] == f"c{j}" and d.metadata.get("indexer", "vector") == "vector"
                       for d in g)
            sg = {d.text: d.score for d in g}
            sw = {d.text: d.score for d in w}
            kth = max(sw.values())
            for t in set(sg) ^ set(sw):                      # exchanged only inside a tie band
                assert abs(sg.get(t, sw.get(t)) - kth) <= DEV, (j, t)
            np.testing.assert_allclose([d.score for d in g], [d.score for d in w], atol=DEV)
            assert [d.score for d in g] == sorted(d.score for d in g)
    finally:
        N.profile_enable(False)
        for name in ("subset_gpu_a", "subset_gpu_b"):
            c = V._collections.pop(name, None)
            if c is not None:
                c.store.close()
