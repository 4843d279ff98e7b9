"""CPU: exact BM25 row scoring and two-sided floor fusion: the per-pair reference (tests/lex_rows_ref.py)
against the oracle's term-list scorer, tests/fuse_sides_ref.py against tests/fuse_ref.py and a
hand-worked side_b case, the new C entry points' declaration / export / argument checks, the
"floor_full" fusion name in the Python layers, and ShardedLex.score_rows / hybrid(fusion="floor_full")
over two double shards.  The kernels are tested in test_gpu_lex_score_rows.py."""
import os
import re

import numpy as np
import pytest

import fuse_ref as FR
import fuse_sides_ref as FS
import lex_rows_ref as LR
from fuse_doubles import FuseStore, fuse_backend
from lex_rows_doubles import RowsLex, sides_backend
from oracle.bm25 import LexCorpus, bm25_fixed_scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "fuse_fixtures.npz")
NAMES = ["sr_lex_score_rows", "sr_lex_score_rows_dev", "sr_score_fuse_sides", "sr_score_fuse_sides_dev"]
NI = -np.inf


# -- the per-pair reference against the oracle's term-list scorer ----------------------------------------
def _corpus(seed=3, n=600, vocab=40):
    from super_rag_amd.lexical import doc_arrays
    rng = np.random.default_rng(seed)
    docs = [rng.integers(0, vocab, rng.integers(0, 13)).tolist() for _ in range(n)]
    return LexCorpus(*doc_arrays(docs)), rng


def _queries(rng, vocab=40):
    qs = [rng.integers(0, vocab, rng.integers(1, 6)).tolist() for _ in range(6)]
    return qs + [[7], [3, 3, 9, 3], [vocab + 5, -2, 11], []]


@pytest.mark.parametrize("removed", [False, True])
@pytest.mark.parametrize("global_stats", [False, True])
def test_pair_reference_equals_the_term_list_oracle(removed, global_stats):
    corpus, rng = _corpus()
    n = corpus.n
    if removed:
        corpus.remove(np.arange(4, n, 7))
        # and every document of one term: it is no longer scored
        corpus.remove(np.unique(corpus.row[corpus.terms == 11]))
        assert corpus.df[11] == 0
    qs = _queries(rng)
    stats = None
    if global_stats:     # a fictitious larger corpus this one is a shard of
        df = {t: int(corpus.df[t]) * 3 + 5 for t in range(corpus.vocab)}
        stats = (int(corpus.live.sum()) * 4 + 17, int(corpus.dl[corpus.live].sum()) * 4 + 1000, df.__getitem__)
    rows = np.tile(np.arange(-1, n + 1, dtype=np.int64), (len(qs), 1))      # every row, -1 and n
    score, fixed = LR.score_rows(corpus, qs, rows, stats=stats)
    assert score.dtype == np.float32 and fixed.dtype == np.uint32
    hits = 0
    for i, q in enumerate(qs):
        want = bm25_fixed_scores(corpus, q, stats=stats)
        np.testing.assert_array_equal(fixed[i, 1:-1], want)                  # integers: exact
        live = corpus.live
        assert np.isneginf(score[i, [0, -1]]).all() and (fixed[i, [0, -1]] == 0).all()
        assert np.isneginf(score[i, 1:-1][~live]).all() and (want[~live] == 0).all()
        np.testing.assert_array_equal(score[i, 1:-1][live],
                                      want[live].astype(np.float32) / np.float32(65536.0))
        hits += int((want > 0).sum())
    assert hits > 500          # the comparison is not of zeros


# -- fuse_sides_ref ---------------------------------------------------------------------------------------
def _cases():
    with np.load(FIX) as z:
        names = [str(n) for n in z["names"]]
        return {n: {k[len(n) + 1:]: z[k] for k in z.files if k.startswith(n + ".")} for n in names}


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_without_side_b_it_is_fuse_ref(name):
    c = CASES[name]
    side = c["side_a"] if int(c["has_side"]) else None
    args = (c["score_a"], c["rows_a"], c["score_b"], c["rows_b"], side)
    rest = (int(c["mode"]), c["alpha"], c["floor_a"], c["floor_b"], c["min_score"], int(c["k_out"]))
    want = FR.fuse_one(*args, *rest)
    got = FS.fuse_one(*args, None, *rest)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(got[1], c["want_rows"])
    np.testing.assert_array_equal(got[0], c["want_score"])
    batch = FS.score_fuse(*[None if a is None else a[None] for a in args], None, *rest)
    for g, w in zip(batch, want):
        np.testing.assert_array_equal(g[0], w)


def test_side_b_hand_worked():
    """The mirror of the fixture "floor_with_side".  FLOOR, floor_a = -1, floor_b = 0, alpha = .5.
    a: hi 1, lo -1 -> row 1: 1, row 2: .5, row 5: .25.   b: hi 4, lo 0 -> row 2: 1, row 3: .5, row 4: .25.
    side_a of b's rows (2, 3, 4) = (.75 ignored: row 2 is in a, .5 -> .75, unknown -> 0);
    side_b of a's rows (1, 2, 5) = (3 -> .75, 1 ignored: row 2 is in b, unknown -> 0).
    1: .5 + .375 = .875;  2: .25 + .5 = .75;  3: .375 + .25 = .625;  4: 0 + .125;  5: .125 + 0 (tie: row asc)."""
    a = ([1.0, 0.0, -0.5], [1, 2, 5])
    b = ([4.0, 2.0, 1.0], [2, 3, 4])
    side_a, side_b = [0.75, 0.5, NI], [3.0, 1.0, NI]
    s, r, xa, xb = FS.fuse_one(*a, *b, side_a, side_b, FS.FLOOR, 0.5, -1.0, 0.0, NI, 6)
    np.testing.assert_array_equal(r, [1, 2, 3, 4, 5, -1])
    np.testing.assert_array_equal(s, np.asarray([0.875, 0.75, 0.625, 0.125, 0.125, NI], np.float32))
    np.testing.assert_array_equal(xa, np.asarray([1.0, 0.0, 0.5, NI, -0.5, NI], np.float32))
    np.testing.assert_array_equal(xb, np.asarray([3.0, 4.0, 2.0, 1.0, NI, NI], np.float32))
    # without side_b row 1 has no b score: .5, behind rows 2 and 3
    s0, r0, _, xb0 = FS.fuse_one(*a, *b, side_a, None, FS.FLOOR, 0.5, -1.0, 0.0, NI, 6)
    np.testing.assert_array_equal(r0, [2, 3, 1, 4, 5, -1])
    np.testing.assert_array_equal(s0, np.asarray([0.75, 0.625, 0.5, 0.125, 0.125, NI], np.float32))
    assert np.isneginf(xb0[2])
    # a side score above list b's maximum leaves hi_b alone: row 1 normalises to 8 / 4 = 2, row 2 stays 1
    s1, r1, _, _ = FS.fuse_one(*a, *b, side_a, [8.0, 1.0, NI], FS.FLOOR, 0.5, -1.0, 0.0, NI, 2)
    np.testing.assert_array_equal(r1, [1, 2])
    np.testing.assert_array_equal(s1, np.asarray([1.5, 0.75], np.float32))
    # MINMAX: lo_b = 1, so side_b = .5 of row 1 is below it -> max(0, ...) = 0, as for side_a
    s2, r2, _, _ = FS.fuse_one(*a, *b, None, [0.5, NI, 2.5], FS.MINMAX, 0.5, k_out=5)
    got = dict(zip(r2.tolist(), s2.tolist()))
    assert got[1] == 0.5 and got[5] == 0.25                  # 5: a-norm 0, b-norm (2.5 - 1) / 3 = .5
    assert FS.unknown_where_zero([0.0, 1.5, NI]).tolist() == [NI, 1.5, NI]


# -- the C entry points -------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    import shutil
    import subprocess
    from super_rag_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "super_rag_mi355x.h")).read(), flags=re.S)
    for name, arity in zip(NAMES, (9, 11, 20, 21)):
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", src)
        assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]) == arity, name
    assert re.search(r"#define\s+SR_FUSE_FLOOR_FULL\s+2\b", src) and _native.SR_FUSE_FLOOR_FULL == 2
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for path in (_native.library_path(), _native.diag_library_path()):
        out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True,
                             check=True).stdout
        assert set(NAMES) <= {l.split()[-1] for l in out.splitlines()}


def _invalid(code, word):
    from super_rag_amd import _native
    assert code == _native.SR_ERR_INVALID
    msg = _native.load().sr_last_error().decode()
    assert word in msg, msg


def test_argument_validation_needs_no_device():
    """Every limit violation is SR_ERR_INVALID with a message before any device call: this host has
    no GPU, so a device call would fail with another code."""
    from super_rag_amd import _native
    lib = _native.load()
    f32, i64 = np.float32, np.int64
    sa, ra = np.zeros((1, 4), f32), np.arange(4, dtype=i64)[None]
    sb, rb = np.zeros((1, 3), f32), np.arange(3, dtype=i64)[None]
    side_b = np.zeros((1, 4), f32)
    os_, or_ = np.zeros((1, 8), f32), np.zeros((1, 8), i64)
    P = _native.ptr

    def host(sa_=sa, ra_=ra, ka=4, kb=3, B=1, mode=1, alpha=0.5, k_out=4, os__=os_):
        return lib.sr_score_fuse_sides(None if sa_ is None else P(sa_), None if ra_ is None else P(ra_), ka,
                                       P(sb), P(rb), kb, None, P(side_b), B, mode, alpha, -1.0, 0.0,
                                       float("-inf"), k_out, None if os__ is None else P(os__), P(or_),
                                       None, None, 0)

    def dev(sa_=sa, ka=4, kb=3, B=1, mode=1, alpha=0.5, k_out=4, **_):
        # host memory stands in for device buffers: validation must never touch it
        return lib.sr_score_fuse_sides_dev(None if sa_ is None else P(sa_), P(ra), ka, P(sb), P(rb), kb,
                                           None, P(side_b), B, mode, alpha, -1.0, 0.0, float("-inf"),
                                           k_out, P(os_), P(or_), None, None, 0, None)

    for call in (host, dev):
        _invalid(call(ka=2049), "list length")
        _invalid(call(kb=-1), "list length")
        _invalid(call(k_out=0), "k_out")
        _invalid(call(k_out=2049), "k_out")
        _invalid(call(alpha=1.5), "alpha")
        _invalid(call(alpha=float("nan")), "alpha")
        _invalid(call(mode=7), "mode")
        _invalid(call(mode=_native.SR_FUSE_FLOOR_FULL), "mode")      # only sr_hybrid_search_fused takes it
        _invalid(call(B=-1), "batch")
        _invalid(call(sa_=None), "null")
        assert call(B=0, sa_=None) == _native.SR_OK                  # a no-op, whatever the buffers
    _invalid(host(os__=None), "null")
    big = ra.copy()
    big[0, 2] = 2 ** 32 - 1
    _invalid(host(ra_=big), "2^32")
    # the one-sided entry points still reject the new mode
    _invalid(lib.sr_score_fuse(P(sa), P(ra), 4, P(sb), P(rb), 3, None, 1, 2, 0.5, -1.0, 0.0, float("-inf"),
                               4, P(os_), P(or_), None, None, 0), "mode")
    # sr_hybrid_search_fused accepts it: the next check (null store) answers, and 7 is still unknown
    q = np.zeros((1, 8), f32)

    def fused(mode):
        return lib.sr_hybrid_search_fused(None, None, P(q), None, None, 1, 4, 4, mode, 0.5,
                                          float("-inf"), None, 0, P(os_), P(or_), None, None)
    _invalid(fused(2), "null")
    _invalid(fused(7), "mode")

    qoff, qt = np.asarray([0, 1], i64), np.zeros(1, np.int32)
    out, fx = np.zeros((1, 3), f32), np.zeros((1, 3), np.uint32)
    _invalid(lib.sr_lex_score_rows(None, P(qoff), P(qt), 1, P(rb), 3, None, P(out), P(fx)), "null")
    _invalid(lib.sr_lex_score_rows(None, P(qoff), P(qt), -1, P(rb), 3, None, P(out), P(fx)), "negative")
    _invalid(lib.sr_lex_score_rows(None, P(qoff), P(qt), 1, P(rb), -3, None, P(out), None), "negative")
    _invalid(lib.sr_lex_score_rows_dev(None, P(qoff), P(qt), 1, P(rb), 3, None, 0, P(out), None, None), "null")
    _invalid(lib.sr_lex_score_rows_dev(None, P(qoff), P(qt), 1, P(rb), -1, None, 0, P(out), None, None),
             "negative")


# -- the Python layers ---------------------------------------------------------------------------------------
def test_fusion_name_and_wrappers():
    from super_rag_amd import lexical
    assert lexical.fusion_mode("floor_full") == 2
    assert lexical.FUSIONS == ("rrf", "relative", "floor", "floor_full")
    with pytest.raises(ValueError):
        lexical.fusion_mode("floor_all")
    # the list-level calls take "floor" and the side scores, not the collection-level name
    z = np.zeros((1, 2), np.float32)
    with pytest.raises(ValueError, match="side_b"):
        lexical.score_fuse(z, z.astype(np.int64), z, z.astype(np.int64), 2, mode="floor_full")
    with pytest.raises(ValueError):
        lexical.hybrid_search(None, None, np.zeros((1, 4)), [[1]], 3, fusion="floor_full", alpha=2.0)


def test_pipeline_rejects_floor_full():
    from super_rag_amd.pipeline import SearchPipeline
    for kw in ({}, {"force_exchange": True}):
        with pytest.raises(ValueError, match="not built"):
            SearchPipeline(None, None, None, None, None, fusion="floor_full", **kw)


@pytest.fixture
def V():
    from super_rag_amd import lexical, vectorstore as V
    V.set_store_backend(lambda dim, dev: FuseStore(dim, dev), FuseStore.load)
    V.set_lex_backend(lambda dev: RowsLex(dev), RowsLex.load)
    lexical.set_fuse_backend(sides_backend)
    V._collections.clear()
    yield V
    V._collections.clear()
    V.set_store_backend(V._native_store, V._native_load)
    V.set_lex_backend(V._native_lex, V._native_lex_load)
    lexical.set_fuse_backend(None)


def _unit(c, dim=4):
    v = np.zeros(dim)
    v[0], v[1] = c, np.sqrt(1.0 - c * c)
    return v


def test_connector_accepts_floor_full(V):
    """Query (e0, "zeta"), k_each = 2.  Row 0 is the best dense row and holds the keyword once among
    many tokens: it falls out of the BM25 top-2 (rows 2 and 3), so "floor" counts its BM25 as nothing
    and "floor_full" as what it is."""
    from super_rag_amd.models import QueryWithEmbedding, TextNode
    spec = [(1.0, "zeta beta beta beta beta beta beta beta beta beta"), (0.9, "alpha beta"),
            (-0.2, "zeta zeta zeta"), (-0.3, "zeta zeta gamma"), (0.1, "gamma delta"), (-0.8, "delta")]
    nodes = [TextNode(text=t, metadata={"i": i}, embedding=_unit(c).tolist()) for i, (c, t) in enumerate(spec)]
    conn = lambda **kw: V.MI355XVectorStoreConnector({"collection": "ff", "coalesce": False, "hybrid": True,
                                                      "hybrid_k_each": 2, **kw})
    flo = conn(hybrid_fusion="floor")
    flo.store.add(nodes)
    full = conn(hybrid_fusion="floor_full")
    assert full.hybrid_fusion == "floor_full"
    q = QueryWithEmbedding(query="zeta", top_k=4, embedding=_unit(1.0).tolist())
    got_flo, got_full = flo.search(q).results, full.search(q).results
    c = V._get("ff")
    qv, terms = _unit(1.0)[None], [c.vocab.query_ids(["zeta"])]
    sims, dense = c.store.search_sim(qv, 2)
    lsc, lex = c.lex.search(terms, 2)
    assert dense[0].tolist() == [0, 1] and sorted(lex[0].tolist()) == [2, 3]
    side_a = c.store.score_rows(qv, lex)
    bm = c.lex.score_rows(terms, dense)
    assert bm[0, 0] > 0 and bm[0, 1] == 0                 # row 0 matches, row 1 does not
    for got, side_b in ((got_flo, None), (got_full, FS.unknown_where_zero(bm))):
        s, r, _, _ = FS.score_fuse(sims, dense, lsc, lex, side_a, side_b, FS.FLOOR, 0.5, k_out=4)
        keep = r[0] >= 0
        assert [d.metadata["i"] for d in got] == r[0][keep].tolist()
        assert [d.score for d in got] == [float(x) for x in s[0][keep]]
    by_row = lambda got: {d.metadata["i"]: d.score for d in got}
    assert by_row(got_full)[0] > by_row(got_flo)[0]       # the truncated match is completed
    assert by_row(got_full)[1] == by_row(got_flo)[1]      # a non-matching row scores as before
    # the existing exclusions apply to it as well
    with pytest.raises(ValueError):
        conn(hybrid_fusion="floor_full", group_by="document_id")
    with pytest.raises(ValueError):
        conn(hybrid_fusion="floor_full", diversify="mmr")
    with pytest.raises(ValueError):
        conn(hybrid_fusion="floor_full", hybrid_alpha=1.5)


# -- ShardedLex -----------------------------------------------------------------------------------------------
def test_sharded_score_rows_and_floor_full_equal_one_shard():
    from super_rag_amd import lexical
    from super_rag_amd.lexical import ShardedLex
    from super_rag_amd.store import ShardedStore
    rng = np.random.default_rng(11)
    n, dim, vocab = 120, 8, 14
    x = rng.standard_normal((n, dim)).astype(np.float32)
    docs = [rng.integers(0, vocab, rng.integers(1, 9)).tolist() for _ in range(n)]
    single, slex = FuseStore(dim), RowsLex()
    sh = ShardedStore(dim, [0, 1], factory=lambda d, dev: FuseStore(d, dev))
    shl = ShardedLex(sh, factory=lambda dev: RowsLex(dev))
    for a, b in ((0, 40), (40, 55), (55, 100), (100, n)):          # batches alternate shards
        single.add(x[a:b])
        slex.add(docs[a:b])
        sh.add(x[a:b])
        shl.add(docs[a:b])
    assert len(set(sh.shard_of.tolist())) == 2
    dead = np.arange(2, n, 9)
    for o in (single, slex, sh, shl):
        o.remove(dead)
    allow = rng.random(n) < 0.7
    q = rng.standard_normal((4, dim)).astype(np.float32)
    terms = [rng.integers(0, vocab, 3).tolist() for _ in range(3)] + [[5, 5, vocab + 3, -1]]
    # routing: every pair to its owner, corpus-wide statistics, -inf for -1 / outside / tombstoned
    rows = rng.integers(-2, n + 3, (4, 23))
    rows[0, :4] = [-1, n, int(dead[0]), 2 ** 40]
    want_s, want_f = slex.score_rows(terms, rows, fixed=True)
    got_s, got_f = shl.score_rows(terms, rows, fixed=True)
    np.testing.assert_array_equal(got_f, want_f)
    np.testing.assert_array_equal(got_s.view(np.uint32), want_s.view(np.uint32))
    np.testing.assert_array_equal(shl.score_rows(terms, rows).view(np.uint32), want_s.view(np.uint32))
    assert np.isneginf(got_s[0, :4]).all() and (got_f[0, :4] == 0).all() and (want_f > 0).sum() > 20
    with pytest.raises(ValueError):
        shl.score_rows(terms, rows[:3])
    assert shl.score_rows(terms, np.zeros((4, 0), np.int64)).shape == (4, 0)
    lexical.set_fuse_backend(sides_backend)
    try:
        changed = 0
        for k, k_each, alpha, al in ((5, 10, 0.5, None), (20, 10, 0.3, None), (7, 12, 0.8, allow),
                                     (3, 40, 0.0, None), (3, 40, 1.0, allow)):
            want = slex.hybrid(single, q, terms, k, k_each, allow=al, fusion="floor_full", alpha=alpha)
            got = shl.hybrid(sh, q, terms, k, k_each, allow=al, fusion="floor_full", alpha=alpha)
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_array_equal(got[0].view(np.uint32), want[0].view(np.uint32))   # bit for bit
            assert got[0].dtype == np.float32 and (want[1][:, 0] >= 0).all()
            floor = shl.hybrid(sh, q, terms, k, k_each, allow=al, fusion="floor", alpha=alpha)
            changed += int(not np.array_equal(floor[0], got[0]))
        assert changed                                    # the completion changes something here
        # a seam of before side_b (no such keyword) still serves the one-sided fusions
        lexical.set_fuse_backend(fuse_backend)
        a = shl.hybrid(sh, q, terms, 5, 10, fusion="floor")
        b = slex.hybrid(single, q, terms, 5, 10, fusion="floor")
        np.testing.assert_array_equal(a[0], b[0])
    finally:
        lexical.set_fuse_backend(None)
