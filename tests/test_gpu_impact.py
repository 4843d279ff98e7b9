"""GPU: the impact (learned-sparse) scoring mode of sr_lex (k_lex.hip lex_score<IMPACT> /
lex_score_rows<IMPACT>; sr_lex_*_weighted) and lexical.sparse_hybrid_search.

No tolerance anywhere: the scores are integer sums compared with tests/impact_ref.py for equality,
the fp32 scores with fixed / 65536 bit for bit, the fusions with tests/fuse_sides_ref.py and
oracle.bm25.rrf_rows bit for bit.
"""
import ctypes
import functools
import struct

import numpy as np
import pytest

import fuse_sides_ref as FS
import impact_ref as IR
from oracle.bm25 import LexCorpus, bm25_topk, rrf_rows

pytestmark = pytest.mark.gpu

N = 8200                 # two 8,192-row accumulation blocks
SHARED = 5               # rows 8,191 and 8,192 both carry it
DEAD_TERM = 11           # every document of this term is removed in the "remove" step
F = np.float32
# repeated values (score ties), the maximum, and weights whose product with a small query weight is
# below half a fixed-point unit (the clamp to 1)
WEIGHTS = np.asarray([16.0, 2.0 ** -12, 2.0 ** -20, 0.125, 0.25, 0.5, 0.5, 1.0, 1.0, 2.0, 0.3, 1.7], F)


def _u32(a):
    return np.asarray(a, F).view(np.uint32)


def _rows_arrays(vocab, seed):
    """8,200 rows as (off, terms, weights): every 50th row empty, rows of 1 term, long rows
    (vocabulary 400: 63 / 64 / 65 / 300 terms; vocabulary 40: 39 / 40), rows of 2..12 terms, three
    rows that carry one term in two postings."""
    rng = np.random.default_rng(seed)
    long_rows = [63, 64, 65, 300] if vocab >= 300 else [vocab - 1, vocab]
    off, terms, weights = [0], [], []
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
        if r in (8191, 8192):
            t[0] = SHARED if SHARED not in t else t[0]
        if r in (17, 4222, 8195):
            t.append(t[0])                       # the same term in two postings of one row
        w = np.where(rng.random(len(t)) < 0.7, rng.choice(WEIGHTS, len(t)),
                     np.exp(rng.normal(-0.5, 1.0, len(t))).clip(1e-6, 16.0)).astype(F)
        terms += t
        weights += w.tolist()
        off.append(len(terms))
    return np.asarray(off, np.int64), np.asarray(terms, np.int32), np.asarray(weights, F)


def _queries(vocab, seed):
    rng = np.random.default_rng(seed)
    many = rng.choice(vocab, 70, replace=False).tolist() if vocab >= 70 else list(range(70))
    return [
        ([7], [1.5]),                                                  # one term
        (many, np.exp(rng.normal(0, 1, 70)).astype(F)),                # more than a 64-slot batch
        ([3, 3, 9, 3, 9], [0.5, 2.0, 1.0, 1.25, 0.25]),                # repeated ids: the maximum counts
        ([4, 6, SHARED], [0.0, 1.0, 0.75]),                            # a zero weight is dropped
        ([vocab + 5, -2, 2 ** 26 + 1], [1.0, 1.0, 1.0]),               # nothing the index knows
        ([DEAD_TERM], [1.0]),
        ([7, 8, 12], [2.0 ** -6, 2.0 ** -5, 2.0 ** -6]),               # products under half a unit
        {2: 0.5, 13: 0.5, 21: 1.0},                                    # a dict; equal weights
        ([], []),
    ]


def _pairs(n, dead_row):
    return np.concatenate([[-1, n, dead_row], np.arange(n)]).astype(np.int64)


K_BIG = 1000


def _check(ix, corpus, queries, dead_row, what, allow=None, mask_key=0):
    """search at k = 1, 10, 1000 and score_rows of every row against the reference; returns the
    reference's (rows [B, 1000], fixed [B, 1000])."""
    want_s, want_r, want_f = IR.topk(corpus, queries, K_BIG, allow)
    for k in (K_BIG, 10, 1):
        got_s, got_r, got_f = ix.search(queries, k, allow=allow, mask_key=mask_key, fixed=True)
        assert got_s.dtype == F and got_r.dtype == np.int64 and got_f.dtype == np.uint32
        np.testing.assert_array_equal(got_f, want_f[:, :k], err_msg=f"{what} k={k}")
        np.testing.assert_array_equal(got_r, want_r[:, :k], err_msg=f"{what} k={k}")
        np.testing.assert_array_equal(_u32(got_s), _u32(want_s[:, :k]), err_msg=f"{what} k={k}")
        s2, r2 = ix.search(queries, k, allow=allow, mask_key=mask_key)       # out_fixed == NULL
        np.testing.assert_array_equal(r2, got_r)
        np.testing.assert_array_equal(_u32(s2), _u32(got_s))
    if allow is not None:
        return want_r, want_f
    n = corpus.n
    rows = np.tile(_pairs(n, dead_row), (len(queries), 1))
    ref_s, ref_f = IR.score_rows(corpus, queries, rows)
    got_s, got_f = ix.score_rows(queries, rows, fixed=True)
    np.testing.assert_array_equal(got_f, ref_f, err_msg=what)
    np.testing.assert_array_equal(_u32(got_s), _u32(ref_s), err_msg=what)
    np.testing.assert_array_equal(_u32(ix.score_rows(queries, rows)), _u32(got_s))
    valid = (rows >= 0) & (rows < n)
    valid[valid] = corpus.live[rows[valid]]
    assert np.isneginf(got_s[~valid]).all() and (got_f[~valid] == 0).all(), what
    # ... and against the search: every listed row has the pair score, bit for bit
    for b in range(len(queries)):
        m = want_r[b] >= 0
        np.testing.assert_array_equal(got_f[b, 3 + want_r[b, m]], want_f[b, m], err_msg=what)
    return want_r, want_f


@pytest.mark.parametrize("vocab", [40, 400])
def test_search_and_pairs_equal_the_reference_through_the_index_life(vocab, tmp_path):
    from super_rag_amd.lexical import NativeImpactIndex
    off, terms, weights = _rows_arrays(vocab, seed=vocab)
    queries = _queries(vocab, seed=vocab + 1)
    corpus = IR.ImpactCorpus(off, terms, weights)
    ix = NativeImpactIndex()
    split = 5000
    first = corpus.keep(np.arange(split))
    assert ix.add_arrays(first.off, first.terms, first.weights) == 0
    rest = corpus.keep(np.arange(split, N))
    assert ix.add_arrays(rest.off, rest.terms, rest.weights) == split
    st = ix.stats()
    assert (st["rows"], st["live"], st["postings"], st["avgdl"]) == (N, N, int(off[-1]), 0.0)
    want_r, want_f = _check(ix, corpus, queries, 0, "two adds")
    # what the corpus was built to exercise, shown on the reference
    nhit = (want_r >= 0).sum(1)
    assert nhit[4] == 0 and nhit[8] == 0 and nhit[5] > 0
    if vocab == 400:
        assert 0 < nhit[0] < K_BIG                                    # k above the number of matches
        lens = np.diff(off)
        assert len(set(queries[1][0])) == 70 and {63, 64, 65, 300} <= set(lens.tolist())
    f0 = corpus.fixed_scores(queries[3])
    assert f0[8191] > 0 and f0[8192] > 0                              # both sides of the block boundary
    assert any((np.diff(want_f[b][want_r[b] >= 0].astype(np.int64)) == 0).any() for b in (0, 3, 7)), "no ties"
    tiny = corpus.fixed_scores(queries[6])
    assert (tiny == 1).any() or ((tiny > 0) & (tiny < 4)).any()       # clamped products
    # allow masks, with the device mask cached under a key and reused
    rng = np.random.default_rng(3)
    allow = rng.random(N) < 0.5
    _check(ix, corpus, queries, 0, "allow", allow=allow, mask_key=0)
    _check(ix, corpus, queries, 0, "allow cached", allow=allow, mask_key=77)
    _check(ix, corpus, queries, 0, "allow reused", allow=allow, mask_key=77)
    # remove: tombstones on both sides of the block boundary, and every document of one term
    dead = np.union1d(np.union1d(np.arange(4, N, 7), [8192]), np.unique(corpus.row[corpus.terms == DEAD_TERM]))
    ix.remove(dead)
    corpus.remove(dead)
    want_r, _ = _check(ix, corpus, queries, int(dead[0]), "remove")
    assert (want_r[5] < 0).all() and not np.isin(want_r[want_r >= 0], dead).any()
    _check(ix, corpus, queries, 0, "remove + allow", allow=allow, mask_key=77)    # the key outlives nothing
    # save + load
    path = str(tmp_path / "impact.bin")
    ix.save(path)
    assert open(path, "rb").read(8) == b"SRMILEX2"
    loaded = NativeImpactIndex.load(path)
    assert loaded.stats() == ix.stats()
    _check(loaded, corpus, queries, int(dead[0]), "save + load")
    loaded.close()
    # compact
    remap = ix.compact()
    keep = np.nonzero(corpus.live)[0]
    np.testing.assert_array_equal(remap[keep], np.arange(len(keep)))
    assert (remap[dead] == -1).all()
    compacted = corpus.keep(keep)
    _check(ix, compacted, queries, len(keep) - 1, "compact")
    ix.close()


@functools.lru_cache(maxsize=None)
def _small():
    from super_rag_amd.lexical import NativeImpactIndex
    ix = NativeImpactIndex()
    ix.add([{1: 0.5, 2: 1.0}, ([2, 3], [2.0, 16.0]), {}])
    return ix


def _raises(code, fn, *a, **kw):
    from super_rag_amd import _native
    with pytest.raises(_native.NativeError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value
    return e.value


def test_every_limit_is_an_invalid_argument():
    from super_rag_amd import _native as NV
    ix = _small()
    before = ix.stats()
    above = float(np.nextafter(F(16), F(17)))
    for w in (0.0, -0.0, -1.0, float("nan"), float("inf"), above):
        _raises(NV.SR_ERR_INVALID, ix.add, [([1, 2], [1.0, w])])
    _raises(NV.SR_ERR_INVALID, ix.add, [([1, -1], [1.0, 1.0])])
    _raises(NV.SR_ERR_INVALID, ix.add, [([1, 2 ** 26], [1.0, 1.0])])
    assert ix.stats() == before                                       # a refused add leaves no row
    for w in (-1.0, float("nan"), float("inf"), -float("inf")):
        _raises(NV.SR_ERR_INVALID, ix.search, [([1, 2], [1.0, w])], 2)
        _raises(NV.SR_ERR_INVALID, ix.score_rows, [([1, 2], [1.0, w])], [[0]])
        _raises(NV.SR_ERR_INVALID, ix.search, [([1, 99], [1.0, w])], 2)          # judged even on an unknown id
    # the overflow bound, at its edge for one term and summed over many
    below = float(np.nextafter(F(4096), F(0)))
    s, r, f = ix.search([([3], [below])], 2, fixed=True)
    assert r[0].tolist() == [1, -1] and int(f[0, 0]) == int(IR.fixed_products(F(below), F(16.0)))
    assert int(f[0, 0]) == 2 ** 32 - 256
    _raises(NV.SR_ERR_INVALID, ix.search, [([3], [4096.0])], 2)
    _raises(NV.SR_ERR_INVALID, ix.score_rows, [([3], [4096.0])], [[0]])
    ix.search([(list(range(255)), [16.0] * 255)], 2)
    _raises(NV.SR_ERR_INVALID, ix.search, [(list(range(256)), [16.0] * 256)], 2)
    ix.search([([3] * 300, [16.0] * 300)], 2)                         # repeats do not add up
    for k in (0, 1025):
        _raises(NV.SR_ERR_INVALID, ix.search, [([1], [1.0])], k)
    # the hand-checkable scores of the three rows
    s, r, f = ix.search([([2, 3, 2], [1.0, 0.5, 3.0])], 3, fixed=True)
    assert r[0].tolist() == [1, 0, -1] and f[0].tolist() == [(6 + 8) * 65536, 3 * 65536, 0]
    assert s[0, :2].tolist() == [14.0, 3.0] and np.isneginf(s[0, 2])
    sc = ix.score_rows([([2, 3, 2], [1.0, 0.5, 3.0])], [[2, 1, 3, -1]])
    assert sc[0, 0] == 0.0 and sc[0, 1] == 14.0 and np.isneginf(sc[0, 2:]).all()


def _zero_args(name, *handles):
    """Arguments of entry point ``name``: the handles, then null pointers and zeros."""
    from super_rag_amd import _native as NV
    args = list(handles)
    for t in NV.SIGNATURES[name][1][len(handles):]:
        is_ptr = t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)
        args.append(None if is_ptr else 0)
    return args


def test_each_mode_rejects_the_other_modes_entry_points():
    from super_rag_amd import _native as NV
    from super_rag_amd.lexical import NativeLexIndex
    from super_rag_amd.store import NativeStore
    lib = NV.load()
    imp, bm = _small(), NativeLexIndex()
    bm.add([[1, 2, 2], [3]])
    store = NativeStore(64)
    bm25_only = ["sr_lex_add", "sr_lex_search", "sr_lex_search_global", "sr_lex_search_global_fixed",
                 "sr_lex_totals", "sr_lex_df", "sr_lex_search_dev", "sr_lex_query_stats_dev",
                 "sr_lex_search_tok_dev", "sr_lex_score_rows", "sr_lex_score_rows_dev"]
    for name in bm25_only:
        assert getattr(lib, name)(*_zero_args(name, imp._h)) == NV.SR_ERR_STATE, name
        assert b"BM25" in lib.sr_last_error()
    for name in ("sr_hybrid_search", "sr_hybrid_search_fused"):
        args = _zero_args(name, store._h, imp._h)
        args[6], args[7] = 1, 1                                       # k, k_each: shapes are judged first
        assert getattr(lib, name)(*args) == NV.SR_ERR_STATE, name
    for name in ("sr_lex_add_weighted", "sr_lex_search_weighted", "sr_lex_score_rows_weighted"):
        assert getattr(lib, name)(*_zero_args(name, bm._h)) == NV.SR_ERR_STATE, name
        assert b"impact" in lib.sr_last_error()
    assert bm.search([[1]], 1)[1][0, 0] == 0 and imp.search([{1: 1.0}], 1)[1][0, 0] == 0   # both still work
    mode = ctypes.c_int32(-1)
    assert lib.sr_lex_scoring(bm._h, ctypes.byref(mode)) == 0 and mode.value == NV.SR_LEX_BM25
    assert lib.sr_lex_scoring(imp._h, ctypes.byref(mode)) == 0 and mode.value == NV.SR_LEX_IMPACT
    assert lib.sr_lex_scoring(None, ctypes.byref(mode)) == NV.SR_ERR_INVALID
    store.close()
    bm.close()


def test_snapshots_keep_their_mode(tmp_path):
    """A "SRMILEX1" file written from the documented layout (what the library has always written)
    loads and searches as BM25; each Python class refuses the other mode's snapshot."""
    from super_rag_amd.lexical import NativeImpactIndex, NativeLexIndex
    rng = np.random.default_rng(5)
    n, vocab = 300, 30
    docs = [rng.integers(0, vocab, rng.integers(1, 12)).tolist() for _ in range(n)]
    from super_rag_amd.lexical import doc_arrays
    off, terms, tf, dl = doc_arrays(docs)
    live = np.ones(n, np.uint8)
    live[::9] = 0
    row = np.repeat(np.arange(n, dtype=np.uint64), np.diff(off))
    blob = (b"SRMILEX1" + struct.pack("<ffqq", 1.2, 0.75, n, int(off[-1])) + dl.tobytes() + live.tobytes()
            + terms.tobytes() + ((row << np.uint64(32)) | tf.astype(np.uint64)).tobytes())
    old = str(tmp_path / "old.bin")
    open(old, "wb").write(blob)
    lex = NativeLexIndex.load(old)
    corpus = LexCorpus(off, terms, tf, dl, live=live.astype(bool))
    qs = [[1, 2, 2], [7], [29, 3, 40]]
    want_s, want_r = bm25_topk(corpus, qs, 10)
    got_s, got_r = lex.search(qs, 10)
    np.testing.assert_array_equal(got_r, want_r)
    np.testing.assert_array_equal(_u32(got_s), _u32(want_s))
    again = str(tmp_path / "again.bin")
    lex.save(again)
    assert open(again, "rb").read() == blob                          # and is written back byte for byte
    lex.close()
    with pytest.raises(ValueError, match="BM25 snapshot"):
        NativeImpactIndex.load(old)
    imp = str(tmp_path / "imp.bin")
    _small().save(imp)
    with pytest.raises(ValueError, match="impact"):
        NativeLexIndex.load(imp)


@functools.lru_cache(maxsize=None)
def _collection():
    """A 64-dimension store and an impact index of the same 8,200 rows (vocabulary 400), with
    tombstones; built once, only read."""
    from super_rag_amd.lexical import NativeImpactIndex
    from super_rag_amd.store import NativeStore
    off, terms, weights = _rows_arrays(400, seed=400)
    corpus = IR.ImpactCorpus(off, terms, weights)
    rng = np.random.default_rng(8)
    vecs = rng.standard_normal((N, 64)).astype(F)
    store, ix = NativeStore(64), NativeImpactIndex()
    store.add(vecs)
    ix.add_arrays(off, terms, weights)
    dead = rng.choice(N, 300, replace=False)
    store.remove(dead)
    ix.remove(dead)
    corpus.remove(dead)
    B = 6
    # queries near stored rows that also match the sparse query, so the two lists overlap
    qv = (vecs[rng.choice(N, B, replace=False)] + 0.5 * rng.standard_normal((B, 64))).astype(F)
    qs = [(rng.choice(400, 6, replace=False).tolist(), np.exp(rng.normal(0, 0.7, 6)).astype(F)) for _ in range(B - 1)]
    qs.append(([401], [1.0]))                                         # a sparse query that matches nothing
    allow = rng.random(N) < 0.6
    return store, ix, corpus, dead, qv, qs, allow


@pytest.mark.parametrize("masked", [False, True])
def test_sparse_hybrid_search_equals_the_reference_fusion_of_the_reference_lists(masked):
    from super_rag_amd.lexical import sparse_hybrid_search
    store, ix, corpus, dead, qv, qs, allow = _collection()
    al, mkey = (allow, 5) if masked else (None, 0)
    for k, k_each, alpha in ((20, 16, 0.5), (7, 16, 0.3)):
        sims, dr = store.search_sim(qv, k_each, allow=al, mask_key=mkey)
        ssc, sr, _ = IR.topk(corpus, qs, k_each, al)                 # the reference's sparse list
        side_a = store.score_rows(qv, sr)
        side_b = FS.unknown_where_zero(IR.score_rows(corpus, qs, dr)[0])
        want = {
            "relative": FS.score_fuse(sims, dr, ssc, sr, None, None, FS.MINMAX, alpha, -1.0, 0.0, -np.inf, k),
            "floor": FS.score_fuse(sims, dr, ssc, sr, side_a, None, FS.FLOOR, alpha, -1.0, 0.0, -np.inf, k),
            "floor_full": FS.score_fuse(sims, dr, ssc, sr, side_a, side_b, FS.FLOOR, alpha, -1.0, 0.0, -np.inf, k),
        }
        for fusion, ref in want.items():
            got_s, got_r = sparse_hybrid_search(store, ix, qv, qs, k, k_each, fusion=fusion, alpha=alpha,
                                                allow=al, mask_key=mkey)
            np.testing.assert_array_equal(got_r, ref[1], err_msg=fusion)
            np.testing.assert_array_equal(_u32(got_s), _u32(ref[0]), err_msg=fusion)
            r = got_r[got_r >= 0]
            assert r.size and not np.isin(r, dead).any() and (al is None or al[r].all())
        # floor_full completes something floor does not (dense-only rows with a positive sparse score)
        assert np.isfinite(side_b).any()
        rs, rr = sparse_hybrid_search(store, ix, qv, qs, k, k_each, fusion="rrf", allow=al, mask_key=mkey)
        ws, wr = rrf_rows(dr, sr, k)
        np.testing.assert_array_equal(rr, wr)
        np.testing.assert_array_equal(rs.view(np.uint64), ws.view(np.uint64))
    assert (sr[-1] < 0).all()                                         # the query without a match
    with pytest.raises(ValueError):
        sparse_hybrid_search(store, ix, qv, qs, 5, fusion="borda")
    with pytest.raises(ValueError):
        sparse_hybrid_search(store, ix, qv, qs, 5, fusion="floor", alpha=1.5)
