"""CPU: score-based hybrid fusion (weighted cosine + BM25 by normalised score): tests/fuse_ref.py
against the hand-worked fixtures, the five C entry points' declaration / export / argument checks,
the connector's ``hybrid_fusion`` / ``hybrid_alpha`` keys on doubles and ShardedLex.hybrid(fusion=...)
over two double shards.  The kernels are tested in test_gpu_score_fusion.py."""
import os
import re

import numpy as np
import pytest

import fuse_ref as FR
from fuse_doubles import FuseLex, FuseStore, fuse_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "fuse_fixtures.npz")
NAMES = ["sr_score_fuse", "sr_score_fuse_dev", "sr_store_score_rows", "sr_store_score_rows_dev",
         "sr_hybrid_search_fused"]


def _cases():
    with np.load(FIX) as z:
        names = [str(n) for n in z["names"]]
        return {n: {k[len(n) + 1:]: z[k] for k in z.files if k.startswith(n + ".")} for n in names}


CASES = _cases()


# -- the reference against the hand-worked cases ------------------------------------------------
def test_fixtures_cover_the_listed_cases():
    assert len(CASES) >= 12
    for need in ("rrf_disagrees", "hi_equals_lo", "one_entry_list", "empty_list_b", "both_empty",
                 "both_lists", "tie_by_row", "alpha_zero", "alpha_one", "min_score_cut",
                 "k_out_beyond", "side_below_and_above", "absent_entry_in_the_middle"):
        assert any(need in n for n in CASES), need


@pytest.mark.parametrize("name", sorted(CASES))
def test_fuse_ref_equals_the_hand_worked_fixture(name):
    c = CASES[name]
    side = c["side_a"] if int(c["has_side"]) else None
    s, r, a, b = FR.fuse_one(c["score_a"], c["rows_a"], c["score_b"], c["rows_b"], side,
                             int(c["mode"]), c["alpha"], c["floor_a"], c["floor_b"],
                             c["min_score"], int(c["k_out"]))
    assert s.dtype == np.float32 and r.dtype == np.int64
    np.testing.assert_array_equal(r, c["want_rows"])
    np.testing.assert_array_equal(s, c["want_score"])          # exact: dyadic scores
    if int(c["has_comp"]):
        np.testing.assert_array_equal(a, c["want_a"])
        np.testing.assert_array_equal(b, c["want_b"])
    # the batch form is the same function
    sb, rb, _, _ = FR.score_fuse(c["score_a"][None], c["rows_a"][None], c["score_b"][None],
                                 c["rows_b"][None], None if side is None else side[None],
                                 int(c["mode"]), c["alpha"], c["floor_a"], c["floor_b"],
                                 c["min_score"], int(c["k_out"]))
    np.testing.assert_array_equal(sb[0], s)
    np.testing.assert_array_equal(rb[0], r)
    if int(c["rrf_winner"]) >= 0:
        # rank fusion and score fusion disagree on the winner of this case
        assert FR.rrf_winner(c["rows_a"], c["rows_b"]) == int(c["rrf_winner"]) != int(r[0])


def test_fuse_ref_rounds_every_operation_to_fp32():
    # 0.1 and 0.7 are not fp32 numbers: the fused score is the fp32 chain, not the fp64 one
    s, r, _, _ = FR.fuse_one([0.9, 0.3, 0.1], [0, 1, 2], [5.0, 3.3, 0.7], [1, 2, 3], None, FR.MINMAX,
                             0.3, k_out=4)
    f = np.float32
    na = f(f(f(0.3) - f(0.1)) / f(f(0.9) - f(0.1)))
    nb = f(1.0)
    want = f(f(f(0.3) * na) + f(f(f(1.0) - f(0.3)) * nb))
    assert r[0] == 1 and s[0] == want and s.dtype == np.float32


# -- the C entry points -----------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    import shutil
    import subprocess
    from super_rag_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "super_rag_mi355x.h")).read(), flags=re.S)
    for name, arity in zip(NAMES, (19, 20, 6, 9, 17)):
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", src)
        assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]) == arity, name
    assert re.search(r"#define\s+SR_FUSE_MINMAX\s+0\b", src) and _native.SR_FUSE_MINMAX == 0
    assert re.search(r"#define\s+SR_FUSE_FLOOR\s+1\b", src) and _native.SR_FUSE_FLOOR == 1
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
    os_, or_ = np.zeros((1, 8), f32), np.zeros((1, 8), i64)
    P = _native.ptr

    def host(sa_=sa, ra_=ra, ka=4, sb_=sb, rb_=rb, kb=3, B=1, mode=0, alpha=0.5, k_out=4, os__=os_,
             or__=or_):
        return lib.sr_score_fuse(None if sa_ is None else P(sa_), None if ra_ is None else P(ra_), ka,
                                 None if sb_ is None else P(sb_), None if rb_ is None else P(rb_), kb,
                                 None, B, mode, alpha, -1.0, 0.0, float("-inf"), k_out,
                                 None if os__ is None else P(os__), None if or__ is None else P(or__),
                                 None, None, 0)

    def dev(ka=4, kb=3, B=1, mode=0, alpha=0.5, k_out=4, null=False):
        # host memory stands in for device buffers: validation must never touch it
        return lib.sr_score_fuse_dev(None if null else P(sa), P(ra), ka, P(sb), P(rb), kb, None, B,
                                     mode, alpha, -1.0, 0.0, float("-inf"), k_out, P(os_), P(or_),
                                     None, None, 0, None)

    for call in (host, dev):
        _invalid(call(ka=2049), "list length")
        _invalid(call(kb=2049), "list length")
        _invalid(call(ka=-1), "list length")
        _invalid(call(k_out=0), "k_out")
        _invalid(call(k_out=2049), "k_out")
        _invalid(call(alpha=1.5), "alpha")
        _invalid(call(alpha=-0.25), "alpha")
        _invalid(call(alpha=float("nan")), "alpha")
        _invalid(call(mode=7), "mode")
        _invalid(call(B=-1), "batch")
    _invalid(host(sa_=None), "null")
    _invalid(host(rb_=None), "null")
    _invalid(host(os__=None), "null")
    _invalid(host(or__=None), "null")
    _invalid(dev(null=True), "null")
    big = ra.copy()
    big[0, 2] = 2 ** 32
    _invalid(host(ra_=big), "2^32")
    big[0, 2] = 2 ** 32 - 1
    _invalid(host(ra_=big), "2^32")
    # B == 0 is a no-op, whatever the buffers
    assert host(B=0, sa_=None, ra_=None, os__=None, or__=None) == _native.SR_OK
    assert dev(B=0, null=True) == _native.SR_OK

    q = np.zeros((1, 8), f32)
    out = np.zeros((1, 3), f32)
    _invalid(lib.sr_store_score_rows(None, P(q), 1, P(rb), 3, P(out)), "null")
    _invalid(lib.sr_store_score_rows_dev(None, P(q), _native.SR_DTYPE_F32, 1, P(rb), 3, 0, P(out), None),
             "null")

    def fused(s=None, k=4, k_each=4, mode=0, alpha=0.5, B=1):
        return lib.sr_hybrid_search_fused(s, None, P(q), None, None, B, k, k_each, mode, alpha,
                                          float("-inf"), None, 0, P(os_), P(or_), None, None)
    _invalid(fused(), "null")
    _invalid(fused(k_each=1025), "k_each")
    _invalid(fused(k_each=0), "k_each")
    _invalid(fused(k=9), "2 * k_each")
    _invalid(fused(k=0), "k must")
    _invalid(fused(alpha=1.5), "alpha")
    _invalid(fused(mode=7), "mode")
    _invalid(fused(B=-1), "batch")


def test_python_wrappers_reject_bad_names_and_alpha():
    from super_rag_amd import lexical
    assert lexical.fusion_mode("rrf") is None
    assert (lexical.fusion_mode("relative"), lexical.fusion_mode("floor")) == (0, 1)
    with pytest.raises(ValueError):
        lexical.fusion_mode("borda")
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            lexical.check_alpha(bad)
    assert lexical.check_alpha(0) == 0.0 and lexical.check_alpha(1) == 1.0
    with pytest.raises(ValueError):
        lexical.hybrid_search(None, None, np.zeros((1, 4)), [[1]], 3, fusion="borda")
    with pytest.raises(ValueError):
        lexical.hybrid_search(None, None, np.zeros((1, 4)), [[1]], 3, fusion="relative", alpha=2.0)


# -- the connector -------------------------------------------------------------------------------------
@pytest.fixture
def V():
    from super_rag_amd import lexical, vectorstore as V
    V.set_store_backend(lambda dim, dev: FuseStore(dim, dev), FuseStore.load)
    V.set_lex_backend(lambda dev: FuseLex(dev), FuseLex.load)
    lexical.set_fuse_backend(fuse_backend)
    V._collections.clear()
    yield V
    V._collections.clear()
    V.set_store_backend(V._native_store, V._native_load)
    V.set_lex_backend(V._native_lex, V._native_lex_load)
    lexical.set_fuse_backend(None)


def _conn(V, name="fuse", **kw):
    return V.MI355XVectorStoreConnector({"collection": name, "coalesce": False, **kw})


def _unit(c, dim=4):
    """A unit vector with cosine c to e0."""
    v = np.zeros(dim)
    v[0], v[1] = c, np.sqrt(1.0 - c * c)
    return v


def _weak_keyword_nodes():
    """Query = (e0, "zeta").  Row 0: the best dense row, no keyword.  Row 1: second in BOTH lists, close
    to the top of each.  Row 2: the best keyword row (three of three tokens) and far from the query.
    Rows 3..: keyword and dense rows below them, so neither list ends at row 1."""
    from super_rag_amd.models import TextNode
    spec = [(1.0, "alpha beta"), (0.96, "zeta zeta zeta gamma"), (-0.5, "zeta zeta zeta"),
            (0.2, "zeta beta beta beta beta beta beta beta"), (0.5, "beta gamma"), (0.4, "gamma gamma"),
            (0.1, "zeta delta delta delta delta delta delta delta delta delta"), (-0.9, "delta")]
    return [TextNode(text=t, metadata={"i": i}, embedding=_unit(c).tolist()) for i, (c, t) in enumerate(spec)]


def _q(text, top_k, vec=None):
    from super_rag_amd.models import QueryWithEmbedding
    return QueryWithEmbedding(query=text, top_k=top_k, embedding=(_unit(1.0) if vec is None else vec).tolist())


def test_relative_fusion_reorders_where_rrf_picks_by_rank(V):
    nodes = _weak_keyword_nodes()
    rrf = _conn(V, hybrid=True, hybrid_k_each=4)
    rrf.store.add(nodes)
    rel = _conn(V, hybrid=True, hybrid_k_each=4, hybrid_fusion="relative")
    flo = _conn(V, hybrid=True, hybrid_k_each=4, hybrid_fusion="floor", hybrid_alpha=0.25)
    got_rrf = rrf.search(_q("zeta", 4)).results
    got_rel = rel.search(_q("zeta", 4)).results
    got_flo = flo.search(_q("zeta", 4)).results
    # rank fusion: rows 0, 1 and 2 all score 1.0 (first, second in both, first); first appearance wins
    assert [d.metadata["i"] for d in got_rrf][:3] == [0, 1, 2] and got_rrf[0].score == 1.0
    # score fusion: the row that is near the top of both lists wins
    assert got_rel[0].metadata["i"] == 1 and got_flo[0].metadata["i"] == 1
    # and the whole answer is fuse_ref of the two lists the plain paths return
    c = V._get("fuse")
    qv = _unit(1.0)[None]
    terms = [c.vocab.query_ids(["zeta"])]
    sims, dense = c.store.search_sim(qv, 4)
    lsc, lex = c.lex.search(terms, 4)
    for conn, got, mode, alpha, side in ((rel, got_rel, FR.MINMAX, 0.5, None),
                                         (flo, got_flo, FR.FLOOR, 0.25, c.store.score_rows(qv, lex))):
        s, r, _, _ = FR.score_fuse(sims, dense, lsc, lex, side, mode, alpha, k_out=4)
        keep = r[0] >= 0
        assert [d.metadata["i"] for d in got] == r[0][keep].tolist()
        assert [d.score for d in got] == [float(x) for x in s[0][keep]]
        assert all(a.score >= b.score for a, b in zip(got, got[1:]))      # fused score, descending
        assert conn.hybrid_fusion in ("relative", "floor")


def test_default_ctx_is_todays_rrf(V):
    from doubles import NumpyLex, NumpyStore
    nodes = _weak_keyword_nodes()
    new = _conn(V, hybrid=True, hybrid_k_each=5)
    new.store.add(nodes)
    assert new.hybrid_fusion == "rrf" and new.hybrid_alpha == 0.5
    explicit = _conn(V, hybrid=True, hybrid_k_each=5, hybrid_fusion="rrf", hybrid_alpha=0.9)
    # the doubles of before this feature know no fusion keyword: the default path passes none
    V.set_store_backend(lambda dim, dev: NumpyStore(dim, dev), NumpyStore.load)
    V.set_lex_backend(lambda dev: NumpyLex(dev), NumpyLex.load)
    old = _conn(V, name="old", hybrid=True, hybrid_k_each=5)
    old.store.add(nodes)
    for text, vec in (("zeta", _unit(1.0)), ("beta gamma", _unit(0.3)), ("delta zeta", _unit(-0.2))):
        want = [(d.metadata["i"], d.score) for d in old.search(_q(text, 6, vec)).results]
        assert want
        for conn in (new, explicit):
            assert [(d.metadata["i"], d.score) for d in conn.search(_q(text, 6, vec)).results] == want


def test_bad_keys_raise(V):
    with pytest.raises(ValueError):
        _conn(V, hybrid=True, hybrid_fusion="borda")
    with pytest.raises(ValueError):
        _conn(V, hybrid_fusion="Relative")              # validated even without hybrid
    for bad in (1.5, -0.01, float("nan")):
        with pytest.raises(ValueError):
            _conn(V, hybrid=True, hybrid_fusion="relative", hybrid_alpha=bad)
    # fusion does not lift the existing exclusions
    with pytest.raises(ValueError):
        _conn(V, hybrid=True, hybrid_fusion="relative", group_by="document_id")
    with pytest.raises(ValueError):
        _conn(V, hybrid=True, hybrid_fusion="floor", diversify="mmr")
    assert _conn(V, hybrid=True, hybrid_fusion="floor", hybrid_alpha=1).hybrid_alpha == 1.0


# -- ShardedLex ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", ["relative", "floor"])
def test_sharded_hybrid_fusion_equals_one_shard(fusion):
    from super_rag_amd import lexical
    from super_rag_amd.lexical import ShardedLex
    from super_rag_amd.store import ShardedStore
    rng = np.random.default_rng(11)
    n, dim, vocab = 120, 8, 14
    x = rng.standard_normal((n, dim)).astype(np.float32)       # (ShardedStore.add takes fp32 vectors)
    docs = [rng.integers(0, vocab, rng.integers(1, 9)).tolist() for _ in range(n)]
    single, slex = FuseStore(dim), FuseLex()
    sh = ShardedStore(dim, [0, 1], factory=lambda d, dev: FuseStore(d, dev))
    shl = ShardedLex(sh, factory=lambda dev: FuseLex(dev))
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
    terms = [rng.integers(0, vocab, 3).tolist() for _ in range(4)]
    lexical.set_fuse_backend(fuse_backend)
    try:
        # the sharded store's own lists are the single store's
        for al in (None, allow):
            a, b = single.search_sim(q, 10, allow=al), sh.search_sim(q, 10, allow=al)
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(a[0], b[0])
        rows = rng.integers(-2, n + 3, (4, 17))
        np.testing.assert_array_equal(sh.score_rows(q, rows), single.score_rows(q, rows))
        assert np.isneginf(sh.score_rows(q, np.asarray([[-1], [n], [int(dead[0])], [2 ** 40]]))).all()
        for k, k_each, alpha, al in ((5, 10, 0.5, None), (20, 10, 0.3, None), (7, 12, 0.8, allow),
                                     (3, 40, 0.0, None), (3, 40, 1.0, allow)):
            want = slex.hybrid(single, q, terms, k, k_each, allow=al, fusion=fusion, alpha=alpha)
            got = shl.hybrid(sh, q, terms, k, k_each, allow=al, fusion=fusion, alpha=alpha)
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_array_equal(got[0], want[0])            # bit for bit
            assert got[0].dtype == np.float32 and (want[1][:, 0] >= 0).all()
        with pytest.raises(ValueError):
            shl.hybrid(sh, q, terms, 5, 10, fusion="borda")
        with pytest.raises(ValueError):
            shl.hybrid(sh, q, terms, 5, 10, fusion="relative", alpha=1.01)
    finally:
        lexical.set_fuse_backend(None)
