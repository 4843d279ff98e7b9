"""GPU: exact BM25 of (query, row) pairs (k_lex.hip lex_score_rows; sr_lex_score_rows / _dev), the
two-sided score fusion (sr_score_fuse_sides / _dev) and hybrid_search(fusion="floor_full").

No tolerance anywhere: the pair scores are integer sums compared with tests/lex_rows_ref.py for
equality (and the fp32 score with fixed / 65536 bit for bit), the fusion with tests/fuse_sides_ref.py
bit for bit, the sharded collection with the single index bit for bit.
"""
import functools

import numpy as np
import pytest

import fuse_ref as FR
import fuse_sides_ref as FS
import lex_rows_ref as LR
from oracle.bm25 import LexCorpus

pytestmark = pytest.mark.gpu

N = 600
DEAD_TERM = 11           # every document of this term is removed in the "remove" step


def _u32(a):
    return np.asarray(a, np.float32).view(np.uint32)


# -- corpora ------------------------------------------------------------------------------------------------
def _rows_arrays(vocab, seed):
    """600 rows as (off, terms, tf, dl): every 50th row without a posting, rows of 1 distinct term, the
    long rows (vocabulary 400: 63, 64, 65 and 300 distinct terms, around the wave width and many
    strides of it; vocabulary 40: as many as the vocabulary holds), small rows of 2..12 terms, and
    three rows that carry one term in two postings.  tf in 1..3."""
    rng = np.random.default_rng(seed)
    long_rows = [63, 64, 65, 300] if vocab >= 300 else [vocab - 1, vocab]
    off, terms, tfs, dl = [0], [], [], []
    for r in range(N):
        if r % 50 == 0:
            cnt = 0
        elif r % 10 == 1:
            cnt = 1
        elif r % 10 == 3:
            cnt = long_rows[(r // 10) % len(long_rows)]
        else:
            cnt = int(rng.integers(2, 13))
        t = rng.choice(vocab, cnt, replace=False).tolist()
        if r in (17, 222, 405):
            t.append(t[0])                       # the same term in two postings of one row
        f = rng.integers(1, 4, len(t)).tolist()
        terms += t
        tfs += f
        off.append(len(terms))
        dl.append(int(sum(f)) + int(rng.integers(0, 3)))
    return (np.asarray(off, np.int64), np.asarray(terms, np.int32), np.asarray(tfs, np.int32),
            np.asarray(dl, np.int32))


def _slice(arrays, keep):
    """The document arrays of the rows ``keep`` (ascending row ids), renumbered 0.."""
    off, terms, tf, dl = arrays
    o, t, f = [0], [], []
    for r in keep:
        t.append(terms[off[r]:off[r + 1]])
        f.append(tf[off[r]:off[r + 1]])
        o.append(o[-1] + int(off[r + 1] - off[r]))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return np.asarray(o, np.int64), cat(t, np.int32), cat(f, np.int32), np.asarray(dl, np.int32)[list(keep)]


def _queries(vocab, seed):
    rng = np.random.default_rng(seed)
    many = rng.choice(vocab, 70, replace=False).tolist() if vocab >= 70 else list(range(70))
    return [[7], [3, 3, 9, 3, 9], [vocab + 5, -2, DEAD_TERM, 2 ** 26 + 1], [DEAD_TERM],
            rng.integers(0, vocab, 4).tolist(), many, []]


def _pairs(n, dead_row):
    """K = n + 3: -1, n (the first row past the end), a tombstoned row (once more), and every row."""
    return np.concatenate([[-1, n, dead_row], np.arange(n)]).astype(np.int64)


def _check(lex, corpus, queries, dead_row, what, stats=None, global_stats=None):
    n = corpus.n
    rows = np.tile(_pairs(n, dead_row), (len(queries), 1))
    want_s, want_f = LR.score_rows(corpus, queries, rows, stats=stats)
    got_s, got_f = lex.score_rows(queries, rows, global_stats=global_stats, fixed=True)
    assert got_s.dtype == np.float32 and got_f.dtype == np.uint32 and got_s.shape == rows.shape
    np.testing.assert_array_equal(got_f, want_f, err_msg=what)                    # integers, no tolerance
    valid = (rows >= 0) & (rows < n)
    valid[valid] = corpus.live[rows[valid]]
    assert np.isneginf(got_s[~valid]).all() and (got_f[~valid] == 0).all(), what
    np.testing.assert_array_equal(_u32(got_s[valid]),
                                  _u32(got_f[valid].astype(np.float32) / np.float32(65536.0)), err_msg=what)
    np.testing.assert_array_equal(_u32(got_s), _u32(want_s), err_msg=what)
    np.testing.assert_array_equal(_u32(lex.score_rows(queries, rows, global_stats=global_stats)), _u32(got_s))
    return want_f


@pytest.mark.parametrize("vocab", [40, 400])
def test_all_pairs_equal_the_reference_through_the_index_life(vocab, tmp_path):
    from super_rag_amd.lexical import NativeLexIndex
    arrays = _rows_arrays(vocab, seed=vocab)
    off, terms, tf, dl = arrays
    queries = _queries(vocab, seed=vocab + 1)
    lex = NativeLexIndex()
    # 1. one add
    first = list(range(400))
    lex.add_arrays(*_slice(arrays, first))
    f = _check(lex, LexCorpus(*_slice(arrays, first)), queries, 0, "first add")
    assert (f[:, 3:] > 0).sum() > 200
    # 2. a second add: the offsets are appended
    lex.add_arrays(*_slice(arrays, range(400, N)))
    corpus = LexCorpus(off, terms, tf, dl)
    f = _check(lex, corpus, queries, 0, "second add")
    assert (f[3, 3:] > 0).any()                                       # DEAD_TERM still scores
    many = f[5, 3:]
    if vocab == 400:   # the 70-term query takes two LDS batches, and the long rows several strides
        lens = np.diff(off)
        assert len(set(queries[5])) == 70 and {63, 64, 65, 300} <= set(lens.tolist())
        assert all((many[lens == L] > 0).any() for L in (63, 64, 65, 300))
    # 3. remove: tombstones, and every document of one term
    dead = np.union1d(np.arange(4, N, 7), np.unique(corpus.row[corpus.terms == DEAD_TERM]))
    lex.remove(dead)
    corpus.remove(dead)
    assert corpus.df[DEAD_TERM] == 0
    f = _check(lex, corpus, queries, int(dead[0]), "remove")
    assert (f[3] == 0).all() and (f[:, 3:] > 0).sum() > 200           # the removed term scores nothing
    # ... with the statistics of a larger fictitious corpus
    ids = np.unique(np.asarray([t for q in queries for t in q], np.int64)).astype(np.int32)
    gdf = np.asarray([int(corpus.df[t]) * 3 + 5 if 0 <= t < corpus.vocab else 0 for t in ids.tolist()], np.int64)
    n_live, sum_dl = int(corpus.live.sum()) * 4 + 17, int(corpus.dl[corpus.live].sum()) * 4 + 1000
    table = dict(zip(ids.tolist(), gdf.tolist()))
    _check(lex, corpus, queries, int(dead[0]), "global", stats=(n_live, sum_dl, table.__getitem__),
           global_stats=(n_live, sum_dl, ids, gdf))
    # 4. save + load: the offsets are derived from the snapshot's postings
    path = str(tmp_path / "lex.bin")
    lex.save(path)
    loaded = NativeLexIndex.load(path)
    _check(loaded, corpus, queries, int(dead[0]), "save + load")
    loaded.close()
    # 5. compact: rows renumbered, offsets rebuilt
    remap = lex.compact()
    keep = np.nonzero(corpus.live)[0]
    np.testing.assert_array_equal(remap[keep], np.arange(len(keep)))
    compacted = LexCorpus(*_slice(arrays, keep.tolist()))
    _check(lex, compacted, queries, len(keep) - 1, "compact")
    # ... and an add after it appends to the rebuilt offsets
    lex.add_arrays(*_slice(arrays, range(10, 60)))
    both = keep.tolist() + list(range(10, 60))
    _check(lex, LexCorpus(*_slice(arrays, both)), queries, 0, "add after compact")
    lex.close()


@functools.lru_cache(maxsize=None)
def _index():
    """The vocabulary-40 corpus with tombstones: (index, oracle corpus, queries); built once, only read."""
    from super_rag_amd.lexical import NativeLexIndex
    arrays = _rows_arrays(40, seed=40)
    corpus = LexCorpus(*arrays)
    lex = NativeLexIndex()
    lex.add_arrays(*arrays)
    dead = np.arange(4, N, 7)
    lex.remove(dead)
    corpus.remove(dead)
    return lex, corpus, _queries(40, seed=41), dead


def test_small_and_ragged_shapes():
    """B = 1, K = 1; B = 3, K = 257 (not a multiple of the pairs per workgroup); empty shapes."""
    lex, corpus, queries, dead = _index()
    rng = np.random.default_rng(5)
    for B, K in ((1, 1), (3, 257), (2, 3), (7, 4)):
        qs = [queries[i % len(queries)] for i in range(1, B + 1)]
        rows = rng.integers(-1, N + 1, (B, K)).astype(np.int64)
        want_s, want_f = LR.score_rows(corpus, qs, rows)
        got_s, got_f = lex.score_rows(qs, rows, fixed=True)
        np.testing.assert_array_equal(got_f, want_f)
        np.testing.assert_array_equal(_u32(got_s), _u32(want_s))
    r7 = int(corpus.row[(corpus.terms == 7) & corpus.live[corpus.row]][0])         # a live row holding term 7
    one, one_f = lex.score_rows([[7]], np.asarray([[r7]]), fixed=True)
    assert one.shape == (1, 1) and one_f[0, 0] > 0 and one_f[0, 0] == LR.score_rows(corpus, [[7]], [[r7]])[1][0, 0]
    assert lex.score_rows([], np.zeros((0, 5), np.int64)).shape == (0, 5)
    assert lex.score_rows([[7], [3]], np.zeros((2, 0), np.int64)).shape == (2, 0)
    with pytest.raises(ValueError):
        lex.score_rows([[7]], np.zeros((2, 3), np.int64))


@pytest.mark.parametrize("with_global", [False, True])
def test_agrees_with_the_search(with_global):
    """For every (query, row) the search returns, score_rows gives the same fixed-point score."""
    lex, corpus, queries, dead = _index()
    gs = None
    if with_global:      # statistics of a larger fictitious corpus
        ids = np.unique(np.asarray([t for q in queries for t in q], np.int64)).astype(np.int32)
        gdf = np.asarray([int(corpus.df[t]) * 3 + 5 if 0 <= t < corpus.vocab else 0 for t in ids.tolist()],
                         np.int64)
        gs = (int(corpus.live.sum()) * 4 + 17, int(corpus.dl[corpus.live].sum()) * 4 + 1000, ids, gdf)
    sc, rows, fx = lex.search(queries, N, global_stats=gs, fixed=True)
    assert (rows >= 0).sum() > 500
    got_s, got_f = lex.score_rows(queries, rows, global_stats=gs, fixed=True)
    hit = rows >= 0
    np.testing.assert_array_equal(got_f[hit], fx[hit])
    np.testing.assert_array_equal(_u32(got_s[hit]), _u32(sc[hit]))
    assert np.isneginf(got_s[~hit]).all() and (got_f[~hit] == 0).all()
    # and every live row the search did not return shares no scored term: exactly 0
    allrows = np.tile(np.arange(N, dtype=np.int64), (len(queries), 1))
    full = lex.score_rows(queries, allrows)
    for b in range(len(queries)):
        missing = np.setdiff1d(np.nonzero(corpus.live)[0], rows[b][hit[b]])
        assert (full[b, missing] == 0).all()
    # a query term missing from the global table is the search's error
    if with_global:
        from super_rag_amd import _native
        short = (gs[0], gs[1], gs[2][gs[2] != 7], gs[3][gs[2] != 7])
        for call in (lambda: lex.search([[7]], 5, global_stats=short),
                     lambda: lex.score_rows([[7]], allrows[:1], global_stats=short)):
            with pytest.raises(_native.NativeError, match="missing from the global df table"):
                call()


def test_device_rows_with_a_row_offset():
    import torch
    from super_rag_amd.lexical import query_arrays
    lex, corpus, queries, dead = _index()
    rows = np.tile(_pairs(N, int(dead[0])), (len(queries), 1))
    want_s, want_f = lex.score_rows(queries, rows, fixed=True)
    qoff, qterms = query_arrays(queries)
    for off in (0, 1000):
        rd = torch.from_numpy(np.where(rows >= 0, rows + off, rows)).cuda()
        s, f = lex.score_rows_dev(qoff, qterms, rd, row_offset=off, fixed=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(f.cpu().numpy().view(np.uint32), want_f)
        np.testing.assert_array_equal(_u32(s.cpu().numpy()), _u32(want_s))
        s2 = lex.score_rows_dev(qoff, qterms, rd, row_offset=off)
        np.testing.assert_array_equal(_u32(s2.cpu().numpy()), _u32(want_s))
    # a row below the offset is not this index's
    rd = torch.from_numpy(rows[:, 3:8].copy()).cuda()
    assert np.isneginf(lex.score_rows_dev(qoff, qterms, rd, row_offset=1000).cpu().numpy()).all()


# -- sr_score_fuse_sides ---------------------------------------------------------------------------------------
def _lists(B, ka, kb, seed):
    """Two lists per query sharing about half their rows, scores on small grids (exact ties), some
    entries absent, side scores on the other list's grid (below and above it) with some unknown."""
    rng = np.random.default_rng(seed)
    ra = np.full((B, ka), -1, np.int64)
    rb = np.full((B, kb), -1, np.int64)
    for b in range(B):
        pool = rng.permutation(4 * (ka + kb) + 4)[: ka + kb].astype(np.int64)
        ra[b] = pool[:ka]
        shared = min(ka, kb) // 2
        rb[b, :shared] = rng.permutation(ra[b])[:shared]
        rb[b, shared:] = pool[ka:ka + kb - shared]
        rb[b] = rng.permutation(rb[b])
    sa = (rng.integers(0, 16, (B, ka)) / 16.0).astype(np.float32)
    sb = (rng.integers(0, 16, (B, kb)) / 4.0).astype(np.float32)
    side_a = (rng.integers(-4, 20, (B, kb)) / 16.0).astype(np.float32)
    side_b = (rng.integers(-2, 20, (B, ka)) / 4.0).astype(np.float32)
    side_a[rng.random((B, kb)) < 0.15] = -np.inf
    side_b[rng.random((B, ka)) < 0.15] = -np.inf
    if ka >= 4:
        gone = rng.random((B, ka)) < 0.1
        ra[gone], sa[gone] = -1, 99.0
    if kb >= 4:
        gone = rng.random((B, kb)) < 0.1
        rb[gone], sb[gone] = -1, -99.0
    return sa, ra, sb, rb, side_a, side_b


def _same(got, ref, what):
    for g, r, name in zip(got, ref, ("fused", "rows", "a", "b")):
        g = np.asarray(g)
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name)
        if g.dtype == np.float32:       # bit equality, -inf included
            np.testing.assert_array_equal(g.view(np.uint32), r.view(np.uint32), err_msg=f"{name} {what}")
        else:
            np.testing.assert_array_equal(g, r, err_msg=f"{name} {what}")


@pytest.mark.parametrize("ka", [0, 1, 5, 100])
def test_score_fuse_sides_equals_the_reference_bit_for_bit(ka):
    import torch
    from super_rag_amd.lexical import score_fuse, score_fuse_dev
    B = 3
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    for ki, kb in enumerate((0, 1, 5, 100)):
        sa, ra, sb, rb, side_a, side_b = _lists(B, ka, kb, seed=100 * ka + kb)
        n = ka + kb
        for si, (wa, wb) in enumerate(((True, True), (True, False), (False, True), (False, False))):
            mode = ("floor", "relative")[(si + ki) % 2]
            alpha = (0.5, 0.3, 0.75, 0.0, 1.0)[(si + ki + ka) % 5]
            min_score = 0.25 if (si + ki) % 4 == 3 else -np.inf
            xa, xb = (side_a if wa else None), (side_b if wb else None)
            ref = FS.score_fuse(sa, ra, sb, rb, xa, xb, FR.MODES[mode], alpha, -1.0, 0.0, min_score, 2048)
            what = f"ka={ka} kb={kb} side_a={wa} side_b={wb} {mode} alpha={alpha}"
            kw = dict(mode=mode, alpha=alpha, min_score=min_score)
            host = score_fuse(sa, ra, sb, rb, 2048, side_a=xa, side_b=xb, **kw)
            _same(host, ref, "host " + what)
            if not wb:     # side_b=None is sr_score_fuse itself, and fuse_ref
                _same(host, FR.score_fuse(sa, ra, sb, rb, xa, FR.MODES[mode], alpha, -1.0, 0.0, min_score, 2048),
                      "one-sided " + what)
            for k_out in sorted({1, max(n, 1), 2048}):
                got = score_fuse_dev(t(sa), t(ra), t(sb), t(rb), k_out, side_a=t(xa), side_b=t(xb), **kw)
                torch.cuda.synchronize()
                _same([g.cpu().numpy() for g in got], [r[:, :k_out] for r in ref], f"dev k_out={k_out} " + what)
    # the hand-worked case of test_lex_score_rows.py, on the device
    s, r, xa, xb = score_fuse([[1.0, 0.0, -0.5]], [[1, 2, 5]], [[4.0, 2.0, 1.0]], [[2, 3, 4]], 6, "floor", 0.5,
                              side_a=[[0.75, 0.5, -np.inf]], side_b=[[3.0, 1.0, -np.inf]])
    assert r[0].tolist() == [1, 2, 3, 4, 5, -1] and s[0, :5].tolist() == [0.875, 0.75, 0.625, 0.125, 0.125]
    assert xb[0, :4].tolist() == [3.0, 4.0, 2.0, 1.0] and np.isneginf(xb[0, 4])


# -- hybrid_search(fusion="floor_full") --------------------------------------------------------------------------
SEED = 20261026      # chosen on the CPU oracle so that the condition asserted below holds with margin


def _collection_data(seed=SEED):
    """600 x 64 vectors, documents over a vocabulary of 40 with up to 12 distinct terms each, removed
    rows, 8 queries of 1..5 terms and an allow mask (numpy only)."""
    rng = np.random.default_rng(seed)
    n, vocab, dim, B = N, 40, 64, 8
    docs = [rng.choice(vocab, rng.integers(1, 13), replace=False).tolist() for _ in range(n)]
    docs = [d + [d[0]] * int(rng.integers(0, 3)) for d in docs]               # tf 1..3 for the first term
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    dead = rng.choice(n, 40, replace=False)
    qv = rng.standard_normal((B, dim)).astype(np.float32)
    qs = [rng.integers(0, vocab, rng.integers(1, 6)).tolist() for _ in range(B)]
    allow = rng.random(n) < 0.6
    return docs, vecs, dead, qv, qs, allow


@functools.lru_cache(maxsize=None)
def _collection():
    """Store + lexical index of _collection_data with its tombstones; built once, only read."""
    from super_rag_amd.lexical import NativeLexIndex
    from super_rag_amd.store import NativeStore
    docs, vecs, dead, qv, qs, allow = _collection_data()
    store, lex = NativeStore(vecs.shape[1]), NativeLexIndex()
    store.add(vecs)
    lex.add(docs)
    store.remove(dead)
    lex.remove(dead)
    return store, lex, vecs, docs, dead, qv, qs, allow


def _full_ref(store, lex, qv, qs, k, k_each, alpha, allow=None, mkey=0, min_score=-np.inf):
    """fuse_sides_ref of the lists the plain calls return; also the "floor" result of the same lists
    and, per query, the dense-only rows with a positive BM25 (the rows "floor_full" completes)."""
    sims, dr = store.search_sim(qv, k_each, allow=allow, mask_key=mkey)
    lsc, lr = lex.search(qs, k_each, allow=allow, mask_key=mkey)
    side_a = store.score_rows(qv, lr)
    bm = lex.score_rows(qs, dr)
    full = FS.score_fuse(sims, dr, lsc, lr, side_a, FS.unknown_where_zero(bm), FS.FLOOR, alpha, -1.0, 0.0,
                         min_score, k)
    floor = FS.score_fuse(sims, dr, lsc, lr, side_a, None, FS.FLOOR, alpha, -1.0, 0.0, min_score, k)
    completed = [(dr[b] >= 0) & ~np.isin(dr[b], lr[b]) & (bm[b] > 0) for b in range(len(qs))]
    return full, floor, completed


@pytest.mark.parametrize("masked", [False, True])
def test_hybrid_floor_full_is_the_two_sided_fusion_of_its_lists(masked):
    from super_rag_amd.lexical import hybrid_search
    store, lex, _, _, dead, qv, qs, allow = _collection()
    al, mkey = (allow, 9) if masked else (None, 0)
    for k, k_each, alpha in ((16, 8, 0.5), (5, 8, 0.3)):
        full, floor, completed = _full_ref(store, lex, qv, qs, k, k_each, alpha, al, mkey)
        # the condition, from the reference lists alone: every query has a dense-only row with a
        # positive BM25, and completing it changes at least one query's answer (looked at in the whole
        # fused list, k = 2 k_each: a short k may cut the rows that moved)
        assert all(c.any() for c in completed), [int(c.sum()) for c in completed]
        differs = [b for b in range(len(qs)) if not (np.array_equal(full[0][b], floor[0][b])
                                                     and np.array_equal(full[1][b], floor[1][b]))]
        assert differs or k < 2 * k_each
        got = hybrid_search(store, lex, qv, qs, k, k_each, allow=al, mask_key=mkey, fusion="floor_full",
                            alpha=alpha, components=True)
        _same(got, full, f"floor_full k={k} alpha={alpha} masked={masked}")
        was = hybrid_search(store, lex, qv, qs, k, k_each, allow=al, mask_key=mkey, fusion="floor",
                            alpha=alpha, components=True)
        _same(was, floor, f"floor k={k} alpha={alpha} masked={masked}")          # "floor" is unchanged
        r = got[1][got[1] >= 0]
        assert r.size and not np.isin(r, dead).any() and (al is None or al[r].all())
        s2, r2 = lex.hybrid(store, qv, qs, k, k_each, allow=al, mask_key=mkey, fusion="floor_full", alpha=alpha)
        np.testing.assert_array_equal(r2, got[1])
        np.testing.assert_array_equal(_u32(s2), _u32(got[0]))
    # a query whose terms match no row: no row is lifted by 1 - alpha
    none = [[45]] * len(qs)
    a = hybrid_search(store, lex, qv, none, 8, 8, fusion="floor_full", components=True)
    b = hybrid_search(store, lex, qv, none, 8, 8, fusion="floor", components=True)
    _same(a, b, "no match")
    assert np.isneginf(a[3]).all()


def test_two_shards_equal_one_device_bit_for_bit():
    from super_rag_amd.lexical import ShardedLex
    from super_rag_amd.store import ShardedStore
    store, lex, vecs, docs, dead, qv, qs, allow = _collection()
    sh = ShardedStore(vecs.shape[1], [0, 0])
    shl = ShardedLex(sh)
    for a, b in ((0, 150), (150, 230), (230, 480), (480, N)):     # batches alternate shards
        sh.add(vecs[a:b])
        shl.add(docs[a:b])
    sh.remove(dead)
    shl.remove(dead)
    assert len(set(sh.shard_of.tolist())) == 2
    rows = np.random.default_rng(1).integers(-1, N + 1, (len(qs), 90))
    rows[:, 0], rows[:, 1] = int(dead[0]), N
    want_s, want_f = lex.score_rows(qs, rows, fixed=True)
    got_s, got_f = shl.score_rows(qs, rows, fixed=True)
    np.testing.assert_array_equal(got_f, want_f)
    np.testing.assert_array_equal(_u32(got_s), _u32(want_s))
    assert (want_f > 0).sum() > 100 and np.isneginf(got_s[:, :2]).all()
    for k, k_each, alpha, al, mkey in ((16, 8, 0.5, None, 0), (10, 8, 0.25, allow, 7)):
        want = lex.hybrid(store, qv, qs, k, k_each, allow=al, mask_key=mkey, fusion="floor_full", alpha=alpha)
        got = shl.hybrid(sh, qv, qs, k, k_each, allow=al, mask_key=mkey, fusion="floor_full", alpha=alpha)
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(_u32(got[0]), _u32(want[0]))
    sh.close()
