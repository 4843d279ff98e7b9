"""GPU: grouped search (k_group.hip; sr_store_search_grouped / sr_store_group_dev,
NativeStore.search_grouped / group_dev, ShardedStore.search_grouped, the connector's ``group_by``).

Primary reference: the walk of tests/group_ref.py over the COMPLETE device ranking, which stores of
at most 1000 rows give through search_sim(q, k = n_rows): rows and groups identical, similarities
within DEV = 1e-6 (device against device, test_gpu_store.py:196).  Secondary reference: the same walk
over the fp64 oracle's ranking (oracle.cosine_topk on quantize_like_store rows), exact rows, distances
within EPS = 1e-4 (fp16 query rounding, test_gpu_store.py:20-22), on seeds whose decisive
similarities are more than 2 EPS apart (asserted by _oracle_case, chosen with the oracle alone).
Largest differences observed on an MI355X over this file: 0 against the device ranking (every
similarity bit-identical), 4.9e-7 in distance against the oracle, 2.4e-7 between the fp8 and the
fp16 scan mode's similarities (same rows and groups).
"""
import functools

import numpy as np
import pytest

import group_ref as R
from oracle.cosine_topk import cosine_topk, quantize_like_store

pytestmark = pytest.mark.gpu

EPS = 1e-4          # against the oracle: fp16 query rounding (test_gpu_store.py:20-22)
DEV = 1e-6          # device against device (test_gpu_store.py:196)
N = 1000            # rows: the complete ranking fits one search_sim call (SR_MAX_TOPK = 1024)
OBSERVED = {"device": 0.0, "oracle": 0.0}


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
def _base(dim):
    """A clustered store that the tests only read, and its rows, built once per dimension."""
    x = _clustered(N, dim, seed=dim)
    return _new_store(x), x


def _groups(kind, n=N):
    i = np.arange(n)
    if kind == "cluster":      # a group = a cluster of ~16 near rows: the head of a ranking is one group
        g = i % 64
    elif kind == "own":        # every row its own group
        g = i.copy()
    elif kind == "one":        # all rows in one group
        g = np.zeros(n, np.int64)
    elif kind == "third":      # about a third of the rows ungrouped
        g = np.where(np.random.default_rng(3).random(n) < 1 / 3, -1, i % 64)
    elif kind == "few":        # fewer groups in the store than k
        g = i % 2
    else:
        raise KeyError(kind)
    return g.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _ranking(dim, B):
    """Queries and the complete device ranking of the base store, computed once and shared."""
    s, x = _base(dim)
    q = _queries(x, B, seed=100 + B)
    sims, rows = s.search_sim(q, N)
    for a in (q, sims, rows):
        a.setflags(write=False)
    return q, sims, rows


def _compare(got, ref, what=""):
    (gs_, gr, gg), (rs, rr, rg) = got, ref
    assert gs_.dtype == np.float32 and gr.dtype == np.int64 and gg.dtype == np.int32
    np.testing.assert_array_equal(gr, rr, err_msg=f"rows {what}")
    np.testing.assert_array_equal(gg, rg, err_msg=f"groups {what}")
    ok = rr >= 0
    assert np.isneginf(gs_[~ok]).all(), what
    if ok.any():
        OBSERVED["device"] = max(OBSERVED["device"], float(np.abs(gs_[ok] - rs[ok]).max()))
    np.testing.assert_allclose(gs_[ok], rs[ok], rtol=0, atol=DEV, err_msg=what)


def _check(store, q, full, group, k, gsz, fetch_k=None, allow=None, ref=None):
    """search_grouped against the walk over the complete device ranking ``full`` = (sims, rows)."""
    ref = R.grouped_search(full[0], full[1], group, k, gsz) if ref is None else ref
    got = store.search_grouped(q, k, group, group_size=gsz, fetch_k=fetch_k, allow=allow, sim=True)
    _compare(got, ref, f"k={k} g={gsz} fetch_k={fetch_k}")
    d, r, g = store.search_grouped(q, k, group, group_size=gsz, fetch_k=fetch_k, allow=allow)
    assert np.array_equal(r, got[1]) and np.array_equal(g, got[2])
    np.testing.assert_array_equal(d, np.where(r >= 0, np.float32(1.0) - got[0], np.inf))
    return got


def _scans(stats):
    return sum(v["launches"] for name, v in stats.items() if name.startswith("cosine_scan"))


@pytest.mark.parametrize("dim", [64, 100, 768])
def test_matrix_of_b_k_group_size_and_fetch_k(dim):
    # clustered groups: the head of every ranking is one group, so the minimum fetch_k = k group_size
    # needs continuation rounds and fetch_k = 1024 (the whole store) never does
    s, _ = _base(dim)
    group = _groups("cluster")
    for B in (1, 5, 33):
        q, sims, rows = _ranking(dim, B)
        for k in (1, 3, 10):
            for gsz in (1, 2, 8):
                ref = R.grouped_search(sims, rows, group, k, gsz)
                for fetch_k in (k * gsz, 1024):
                    _check(s, q, (sims, rows), group, k, gsz, fetch_k=fetch_k, ref=ref)
    print(f"observed max |sim - device ranking| {OBSERVED['device']:.3e}")


@pytest.mark.parametrize("kind", ["own", "one", "third", "few"])
def test_group_shapes(kind):
    s, _ = _base(64)
    group = _groups(kind)
    q, sims, rows = _ranking(64, 5)
    for k in (3, 10):
        for gsz in (1, 2, 8):
            ref = R.grouped_search(sims, rows, group, k, gsz)
            for fetch_k in (k * gsz, None, 1024):
                got = _check(s, q, (sims, rows), group, k, gsz, fetch_k=fetch_k, ref=ref)
    if kind == "own":
        assert (got[1][:, :, 0] == rows[:, :10]).all() and (got[1][:, :, 1:] == -1).all()
    if kind == "one":
        assert (got[2][:, 0] == 0).all() and (got[2][:, 1:] == -1).all()
        assert (got[1][:, 0, :] == rows[:, :8]).all() and (got[1][:, 1:, :] == -1).all()
    if kind == "few":
        assert (np.sort(got[2][:, :2], axis=1) == [0, 1]).all() and (got[2][:, 2:] == -1).all()
    if kind == "third":
        assert (got[2] == -1).any() and (got[1][:, :, 0] >= 0).all()   # ungrouped rows hold slots


@functools.lru_cache(maxsize=None)
def _big_group_store():
    """Two big groups around one point (group 7: 400 rows very near it, group 8: 300 rows a little
    farther), the other 300 rows far away in groups 10 .. 14."""
    dim = 64
    rng = np.random.default_rng(17)
    c = rng.standard_normal(dim).astype(np.float32)
    c /= np.linalg.norm(c)
    x = rng.standard_normal((N, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[:400] = c + 0.3 * x[:400]
    x[400:700] = c + 0.8 * x[400:700]
    group = np.concatenate([np.full(400, 7), np.full(300, 8), 10 + np.arange(300) % 5]).astype(np.int32)
    perm = rng.permutation(N)                      # the groups are interleaved in row order
    return _new_store(x[perm]), x[perm], group[perm], c


def test_big_groups_force_open_rounds():
    from super_rag_amd import _native as Nat
    s, x, group, c = _big_group_store()
    q = c[None]
    sims, rows = s.search_sim(q, N)
    assert (group[rows[0, :64]] == 7).all() and (group[rows[0, 400:464]] == 8).all()
    ref = R.grouped_search(sims, rows, group, 3, 2)
    assert sorted(ref[2][0].tolist())[:2] == [7, 8] and (ref[1] >= 0).all()
    Nat.profile_enable(True)
    try:
        got = s.search_grouped(q, 3, group, group_size=2, fetch_k=64, sim=True)
        stats = Nat.profile_read()
    finally:
        Nat.profile_enable(False)
    _compare(got, ref)
    # round 0 sees only group 7, round 1 (7 masked) only group 8, round 2 the rest: three scans,
    # and never more than 1 + (k + 1)
    assert 3 <= _scans(stats) <= 5, stats
    assert stats["group_collapse"]["launches"] == _scans(stats)
    assert stats["group_mask"]["launches"] == _scans(stats) - 1
    _check(s, q, (sims, rows), group, 3, 2, fetch_k=1024)


def test_closed_round_fetches_later_members():
    # unclustered rows, 500 groups of two rows each: with fetch_k = k group_size = 6 round 0 finds the
    # k = 3 groups by their best rows, the second members lie far past the list: one closed round
    from super_rag_amd import _native as Nat
    dim = 64
    rng = np.random.default_rng(29)
    x = rng.standard_normal((N, dim)).astype(np.float32)
    group = (np.arange(N) % 500).astype(np.int32)
    s = _new_store(x)
    q = rng.standard_normal((4, dim)).astype(np.float32)
    sims, rows = s.search_sim(q, N)
    top = group[rows[:, :6]]
    assert all(len(set(t[:3].tolist())) == 3 for t in top)            # k groups found in round 0 ...
    partner = np.array([[np.nonzero(rows[b] == (r + 500) % N)[0][0] for r in rows[b, :3]] for b in range(4)])
    assert (partner >= 6).all()                                        # ... their partners past fetch_k
    ref = R.grouped_search(sims, rows, group, 3, 2)
    assert (ref[1] >= 0).all()
    Nat.profile_enable(True)
    try:
        got = s.search_grouped(q[:1], 3, group, group_size=2, fetch_k=6, sim=True)
        stats = Nat.profile_read()
    finally:
        Nat.profile_enable(False)
    _compare(got, tuple(a[:1] for a in ref))
    assert _scans(stats) == 2 and stats["group_mask"]["launches"] == 1, stats
    _check(s, q, (sims, rows), group, 3, 2, fetch_k=6, ref=ref)
    s.close()


def test_duplicate_rows_in_different_groups_tie_by_row():
    s0, x = _base(64)
    x = x.copy()
    dup = [10, 500, 700, 701, 999]
    x[dup] = x[3]
    s = _new_store(x)
    group = _groups("cluster").copy()
    group[dup] = [900, 901, 902, 902, -1]
    q = np.stack([x[3], x[3] + 0.05 * x[4]])
    sims, rows = s.search_sim(q, N)
    assert rows[0, :6].tolist() == [3, 10, 500, 700, 701, 999]         # equal similarities: row asc
    for k, gsz in ((4, 1), (5, 2), (10, 8)):
        for fetch_k in (k * gsz, 1024):
            got = _check(s, q, (sims, rows), group, k, gsz, fetch_k=fetch_k)
    assert got[2][0, :5].tolist() == [3, 900, 901, 902, -1]
    assert got[1][0, 3, :3].tolist() == [700, 701, -1] and got[1][0, 4, :2].tolist() == [999, -1]
    s.close()


def test_tombstones_then_compaction_and_allow_mask():
    x = _clustered(N, 100, seed=41)
    s = _new_store(x)
    group = _groups("third")
    q = _queries(x, 5, seed=42)
    dead = np.unique(np.concatenate([np.arange(0, N, 64), np.arange(1, N, 7)]))   # cluster 0's head too
    s.remove(dead)
    sims, rows = s.search_sim(q, N)
    assert not np.isin(rows, dead).any() and (rows >= 0).sum(axis=1).tolist() == [N - len(dead)] * 5
    got = None
    for k, gsz, fetch_k in ((3, 2, 6), (10, 1, None), (10, 8, 80), (10, 8, 1024)):
        got = _check(s, q, (sims, rows), group, k, gsz, fetch_k=fetch_k)
        assert not np.isin(got[1], dead).any()
    # an allow mask on top of the tombstones (cached by mask_key, and the group array by group_key)
    allow = np.random.default_rng(43).random(N) < 0.4
    asims, arows = s.search_sim(q, N, allow=allow)
    for _ in range(2):
        ga = s.search_grouped(q, 10, group, group_size=2, fetch_k=20, allow=allow, mask_key=77,
                              group_key=78, sim=True)
        _compare(ga, R.grouped_search(asims, arows, group, 10, 2))
    assert allow[ga[1][ga[1] >= 0]].all()
    # compaction renumbers the rows: the same rows under their new ids with the remapped group array
    m = s.compact()
    keep = m >= 0
    group2 = group[keep]
    sims2, rows2 = s.search_sim(q, N)
    g2 = _check(s, q, (sims2, rows2), group2, 10, 8, fetch_k=1024)
    assert np.array_equal(np.where(got[1] >= 0, m[np.maximum(got[1], 0)], -1), g2[1])
    assert np.array_equal(got[2], g2[2])
    s.close()


def test_fp8_scan_mode_gives_the_fp16_result():
    x = _clustered(N, 768, seed=51)
    s = _new_store(x)
    group = _groups("cluster")
    q = _queries(x, 5, seed=52)
    sims, rows = s.search_sim(q, N)
    cases = ((3, 2, 6), (10, 1, None), (10, 8, 80))
    want = [_check(s, q, (sims, rows), group, k, gsz, fetch_k=f) for k, gsz, f in cases]
    s.set_scan_dtype("fp8")
    worst = 0.0
    for (k, gsz, f), w in zip(cases, want):
        got = s.search_grouped(q, k, group, group_size=gsz, fetch_k=f, sim=True)
        np.testing.assert_array_equal(got[1], w[1])
        np.testing.assert_array_equal(got[2], w[2])
        ok = w[1] >= 0
        worst = max(worst, float(np.abs(got[0][ok] - w[0][ok]).max()))
        print(f"fp8 against fp16 mode, k={k} g={gsz}: max |sim8 - sim16| {worst:.3e}")
        # the same rows and groups; the fp8 mode's candidates carry similarities re-scored on the
        # fp16 rows by another kernel than the fp16 scan (as in the two modes' search()), so those
        # agree within the device-against-device band, not bit for bit (2.4e-7 observed)
        np.testing.assert_allclose(got[0][ok], w[0][ok], rtol=0, atol=DEV)
        assert np.isneginf(got[0][~ok]).all()
    s.close()


def _raw(store, q, k, gsz, k_cand, group, null=()):
    """sr_store_search_grouped on raw arrays: (return code, outputs filled with sentinels)."""
    from super_rag_amd import _native as Nat
    q = np.ascontiguousarray(q, np.float32)
    group = np.ascontiguousarray(group, np.int32)
    shape = (len(q), max(k, 1), max(gsz, 1))
    out_s = np.full(shape, 7.5, np.float32)
    out_r = np.full(shape, -77, np.int64)
    out_g = np.full(shape[:2], -66, np.int32)
    args = dict(q=Nat.ptr(q), group=Nat.ptr(group), out_s=Nat.ptr(out_s), out_r=Nat.ptr(out_r),
                out_g=Nat.ptr(out_g))
    for name in null:
        args[name] = None
    rc = Nat.load().sr_store_search_grouped(store._h, args["q"], len(q), k, gsz, k_cand, args["group"], 0,
                                            None, 0, args["out_s"], args["out_r"], args["out_g"])
    return rc, out_s, out_r, out_g


def test_invalid_arguments_and_empty_batch():
    from super_rag_amd import _native as Nat
    s, x = _base(64)
    group = _groups("cluster")
    q = _queries(x, 2, seed=61)
    rc, out_s, out_r, out_g = _raw(s, q, 3, 2, 6, group)
    assert rc == Nat.SR_OK and (out_r[:, :, 0] >= 0).all() and (out_g >= 0).all()
    bad_group = group.copy()
    bad_group[N - 1] = -2
    bad = {
        "k = 0": (0, 2, 6, group, ()),
        "k above SR_MAX_TOPK": (1025, 1, 1024, group, ()),
        "group_size = 0": (3, 0, 6, group, ()),
        "group_size above SR_GROUP_MAX_SIZE": (3, 9, 64, group, ()),
        "k_cand below k group_size": (3, 2, 5, group, ()),
        "k_cand above SR_MAX_TOPK": (3, 2, 1025, group, ()),
        "k group_size above SR_MAX_TOPK": (200, 8, 1024, group, ()),
        "group id below -1": (3, 2, 6, bad_group, ()),
        "null queries": (3, 2, 6, group, ("q",)),
        "null group": (3, 2, 6, group, ("group",)),
        "null out_sim": (3, 2, 6, group, ("out_s",)),
        "null out_rows": (3, 2, 6, group, ("out_r",)),
        "null out_group": (3, 2, 6, group, ("out_g",)),
    }
    for name, (k, gsz, k_cand, g, null) in bad.items():
        rc, out_s, out_r, out_g = _raw(s, q, k, gsz, k_cand, g, null)
        assert rc == Nat.SR_ERR_INVALID, name
        assert (out_s == 7.5).all() and (out_r == -77).all() and (out_g == -66).all(), name
    with pytest.raises(ValueError):
        s.search_grouped(q, 3, group[:-1])
    # B == 0 is a no-op
    d, r, g = s.search_grouped(np.zeros((0, 64), np.float32), 3, group, group_size=2)
    assert d.shape == (0, 3, 2) and r.shape == (0, 3, 2) and g.shape == (0, 3)
    assert _raw(s, q[:0], 3, 2, 6, group)[0] == Nat.SR_OK
    d, r = s.search(q, 4)                                   # the store is unharmed
    assert (r >= 0).all()


def test_result_does_not_depend_on_fetch_k():
    s, x = _base(768)
    group = _groups("third")
    q, _, _ = _ranking(768, 5)
    for k, gsz in ((10, 1), (10, 3), (40, 8)):
        a = s.search_grouped(q, k, group, group_size=gsz, sim=True)                 # default fetch_k
        b = s.search_grouped(q, k, group, group_size=gsz, fetch_k=1024, sim=True)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)


def test_group_dev_collapses_a_search_dev_list():
    import torch
    s, x, group, c = _big_group_store()
    far = x[np.nonzero(group >= 10)[0][0]]
    q = torch.from_numpy(np.stack([far, c]).astype(np.float32)).cuda()
    K, k, gsz, off = 64, 3, 2, 5000
    sim, rows = s.search_dev(q, K, row_offset=off)
    o_sim, o_rows, o_group, o_done = s.group_dev(rows, sim, k, group, group_size=gsz, row_offset=off)
    torch.cuda.synchronize()
    sim, rows = sim.cpu().numpy(), rows.cpu().numpy()
    assert (rows >= off).all()
    ref = R.grouped_search(sim, rows - off, group, k, gsz)
    got = (o_sim.cpu().numpy(), np.where(o_rows.cpu().numpy() >= 0, o_rows.cpu().numpy() - off, -1),
           o_group.cpu().numpy())
    _compare(got, ref)
    # query 0 (far from the big groups): three groups with two rows each inside its 64 rows; query 1
    # (the big groups' centre): all 64 rows are group 7, the list is full: only a continuation could tell
    assert (ref[1][0] >= 0).all() and (group[rows[1] - off] == 7).all()
    assert o_done.cpu().numpy().tolist() == [1, 0]
    # a list that is not full is complete whatever it holds
    sim2, rows2 = s.search_dev(q, 1024)
    done2 = s.group_dev(rows2, sim2, 10, group, group_size=8)[3]
    torch.cuda.synchronize()
    assert (rows2[:, -1] == -1).all() and done2.cpu().numpy().tolist() == [1, 1]


def test_sharded_store_equals_single_store():
    from super_rag_amd.store import NativeStore, ShardedStore
    dim = 64
    x = _clustered(N, dim, seed=71)
    single = NativeStore(dim, device=0)
    sh = ShardedStore(dim, [0, 0])
    for a, b in ((0, 300), (300, 420), (420, 800), (800, N)):        # batches alternate shards
        single.add(x[a:b])
        sh.add(x[a:b])
    assert len(set(sh.shard_of.tolist())) == 2
    dead = np.arange(5, N, 11)
    single.remove(dead)
    sh.remove(dead)
    group = _groups("third")
    q = _queries(x, 5, seed=72)
    sims, rows = single.search_sim(q, N)
    for k, gsz, fetch_k in ((3, 2, 6), (10, 8, None)):
        want = _check(single, q, (sims, rows), group, k, gsz, fetch_k=fetch_k)
        _compare(sh.search_grouped(q, k, group, group_size=gsz, fetch_k=fetch_k, sim=True), want)
        d, r, g = sh.search_grouped(q, k, group, group_size=gsz, fetch_k=fetch_k)
        assert np.array_equal(r, want[1]) and np.array_equal(g, want[2]) and d.dtype == np.float32
        assert np.isposinf(d[r < 0]).all()
    sh.close()
    single.close()


def test_connector_round_trip_with_group_by():
    from super_rag_amd import vectorstore as V
    from super_rag_amd.models import QueryWithEmbedding, TextNode
    n, dim = 600, 64
    x = _clustered(n, dim, seed=81)
    metas = [{"i": i, "document_id": f"doc{i % 64}"} if i % 5 else {"i": i} for i in range(n)]
    nodes = [TextNode(text=f"t{i}", metadata=m, embedding=v.tolist()) for i, (m, v) in enumerate(zip(metas, x))]
    V._collections.pop("group_gpu", None)
    try:
        conn = V.MI355XVectorStoreConnector({"collection": "group_gpu", "group_by": "document_id",
                                             "group_size": 2, "coalesce": False})
        conn.add(nodes)
        c = V._get("group_gpu")
        q = _queries(x, 3, seed=82)
        group = np.array([i % 64 if i % 5 else -1 for i in range(n)], np.int32)
        sims, rows = c.store.search_sim(q, n)
        ref = R.grouped_search(sims, rows, group, 4, 2)
        for b in range(3):
            res = conn.search(QueryWithEmbedding(query="q", top_k=4, embedding=q[b].tolist())).results
            want = [int(r) for r in ref[1][b].reshape(-1) if r >= 0]
            assert [d.metadata["i"] for d in res] == want and 4 <= len(res) <= 8
            docs = [d.metadata.get("document_id") for d in res]
            assert len({d for d in docs if d is not None}) + docs.count(None) == 4
            np.testing.assert_allclose([d.score for d in res],
                                       [1.0 - s for s in ref[0][b].reshape(-1) if np.isfinite(s)], atol=DEV)
    finally:
        cc = V._collections.pop("group_gpu", None)
        if cc is not None:
            cc.store.close()


# -- secondary check: the fp64 oracle ---------------------------------------------------------------
def _oracle_case(dim, seed, B, k, gsz):
    """Rows, queries, groups and the oracle's grouped result for a seed, with the condition that makes
    the comparison tie-free ASSERTED (a wrong seed fails here, it never passes vacuously): for every
    query the best-row similarities of the first k + 1 groups are more than 2 EPS apart, and inside
    every kept group so are consecutive members down to the one after the group_size-th."""
    x = _clustered(N, dim, seed=seed)
    q = _queries(x, B, seed=seed + 1)
    group = _groups("third")
    stored = quantize_like_store(x).astype(np.float64)
    d, r = cosine_topk(stored, quantize_like_store(q).astype(np.float64), N, normalize=False)
    sims = 1.0 - d
    for b in range(B):
        first, members = [], {}
        for s_, row in zip(sims[b].tolist(), r[b].tolist()):
            key = ("row", row) if group[row] < 0 else int(group[row])
            if key not in members:
                if len(first) == k + 1:
                    continue
                first.append(key)
                members[key] = []
            if len(members[key]) <= gsz:
                members[key].append(s_)
        best = np.array([members[key][0] for key in first])
        assert len(first) == k + 1 and (-np.diff(best) > 2 * EPS).all(), (seed, b, "group order")
        for key in first[:k]:
            assert (-np.diff(np.array(members[key])) > 2 * EPS).all(), (seed, b, key)
    return x, q, group, R.grouped_search(sims, r, group, k, gsz)


@pytest.mark.parametrize("dim,seed,k,gsz", [(64, 200, 3, 2), (100, 301, 10, 1), (768, 400, 10, 3)])
def test_against_fp64_oracle(dim, seed, k, gsz):
    x, q, group, ref = _oracle_case(dim, seed, 5, k, gsz)
    s = _new_store(x)
    for fetch_k in (k * gsz, None):
        d, r, g = s.search_grouped(q, k, group, group_size=gsz, fetch_k=fetch_k)
        np.testing.assert_array_equal(r, ref[1])
        np.testing.assert_array_equal(g, ref[2])
        ok = r >= 0
        OBSERVED["oracle"] = max(OBSERVED["oracle"], float(np.abs(d[ok] - (1.0 - ref[0][ok])).max()))
        np.testing.assert_allclose(d[ok], 1.0 - ref[0][ok], rtol=0, atol=EPS)
    print(f"observed max |dist - oracle| {OBSERVED['oracle']:.3e}")
    s.close()
