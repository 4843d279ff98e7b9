"""GPU: the multi-vector index's life cycle: in-place compaction (sr_mv_compact; k_multivec.hip's
mv_move_kernel behind multivec.hip's chunk schedule), snapshots (sr_mv_save / sr_mv_load) and
multivec.compact_aligned.  The reference is tests/mv_snapshot_ref.py (format, compaction, the chunk
planner) with tests/mv_fp8_ref.py for the fp8 bytes.  Every comparison is of bits: uint32 views of
scores and token values, raw bytes of files.  No tolerance appears anywhere."""
import functools
import os

import numpy as np
import pytest

import colbert_ref as CR
import mv_fp8_ref as Q
import mv_snapshot_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
# rows of 0 / 1 / 15 / 16 / 17 / 65 / 511 tokens: a 1-token row first (a gap of one token in front of
# the 511-token row), zero-token rows, a 1-token row behind a prefix of 625 tokens, a 65-token row
LENS = [1, 511, 0, 15, 16, 17, 65, 0, 1, 65, 17, 1, 16, 0, 15]
NROWS = len(LENS)
PATTERNS = {
    "none": [],
    "all": list(range(NROWS)),
    "first": [0],
    "last": [NROWS - 1],
    "alternating": list(range(0, NROWS, 2)),
    "prefix_then_one_token": [8],
    "zero_token_rows": [2, 7, 13],
    "one_then_65_tokens": [0, 6],          # gap 1 (staged at a 3-token stage), then gap 66 (direct)
}
CONFIGS = [(64, "fp16"), (64, "fp8"), (1024, "fp16"), (1024, "fp8")]
LQS = (1, 17, 65)
CODE = {"fp16": R.DTYPE_F16, "fp8": R.DTYPE_FP8}


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _new(dim, dtype):
    from super_rag_amd.multivec import NativeMultiVectorIndex
    return NativeMultiVectorIndex(dim, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _data(dim):
    """The rows, four more to add later, and the fixed queries; computed once per dim."""
    rng = np.random.default_rng(7000 + dim)
    docs = [CR.unit_f16(rng, n, dim) for n in LENS]
    extra = [CR.unit_f16(rng, n, dim) for n in (3, 0, 20, 1)]
    qs = [CR.unit_f16(rng, n, dim) for n in LQS]
    return docs, extra, qs


def _pool_of(x, docs_added, dim, dtype):
    """The reference pool bytes: what get gives (fp16), or the reference quantiser on the rows as they
    were added (fp8; get's values are checked against it on the way)."""
    n = x.stats()["rows"]
    got = [x.get(r) for r in range(n)]
    if dtype == "fp8":
        for g, d in zip(got, docs_added):
            np.testing.assert_array_equal(_u32(g), _u32(Q.stored(d)))
        return R.pool_bytes(docs_added, dim, R.DTYPE_FP8), got
    return R.pool_bytes(got, dim, R.DTYPE_F16), got


def _all_scores(x, qs, n):
    rows = np.tile(np.arange(n + 2, dtype=np.int64), (len(qs), 1))      # two indexes past the end
    return x.score_rows(qs, rows)


def _add_dev(x, docs, dim):
    import torch
    ld = max(1, max(d.shape[0] for d in docs)) + 2
    pad = np.full((len(docs), ld, dim), 3.0, np.float16)
    for i, d in enumerate(docs):
        pad[i, :d.shape[0]] = d.astype(np.float16)
    lens = np.asarray([d.shape[0] for d in docs], np.int32)
    return x.add_dev(torch.as_tensor(pad).cuda(), torch.as_tensor(lens).cuda())


def _file(x, path):
    x.save(str(path))
    with open(path, "rb") as f:
        return f.read()


# -- compaction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("dim,dtype", CONFIGS)
def test_compaction_in_place(dim, dtype, pattern, tmp_path):
    from super_rag_amd.store import NativeStore
    docs, extra, qs = _data(dim)
    dead = PATTERNS[pattern]
    rb = R.row_bytes(dim, CODE[dtype])
    live = np.ones(NROWS, bool)
    live[dead] = False
    keep = np.nonzero(live)[0]
    m = keep.size
    want_map = R.old_to_new(live)
    # the store's map for the same removals, once per case
    store = NativeStore(64)
    store.add(CR.unit(np.random.default_rng(1).standard_normal((NROWS, 64))).astype(F))
    if dead:
        store.remove(dead)
    store_map = store.compact()
    store.close()
    np.testing.assert_array_equal(store_map, want_map)
    # what the schedule must exercise (the reference planner, in tokens)
    if pattern == "first":
        p3 = R.plan(LENS, live, 3)
        # (all staged but the tail: a last chunk no longer than the gap goes direct)
        assert sum(s for _, _, s in p3) >= 3 and all(s for _, _, s in p3[:-1])
        assert any(1 < t0 < 511 for t0, _, _ in p3)                       # the 511-token row is cut
    if pattern == "one_then_65_tokens":
        kinds = [s for _, _, s in R.plan(LENS, live, 3)]
        assert True in kinds and False in kinds and kinds == sorted(kinds, reverse=True)

    for stage in (0, rb, 3 * rb):
        x = _new(dim, dtype)
        assert x.add(docs) == 0
        pool0, got0 = _pool_of(x, docs, dim, dtype)
        before = _all_scores(x, qs, NROWS)
        if dead:
            x.remove(dead)
        # a stage below one token: the error, and nothing changes
        from super_rag_amd import _native as NV
        for bad in (rb - 1, 1, -1):
            with pytest.raises(NV.NativeError) as e:
                x.compact(bad)
            assert e.value.code == NV.SR_ERR_INVALID
        assert x.stats() == {"rows": NROWS, "live": m, "tokens": sum(LENS)}
        snap_dead = _file(x, tmp_path / "dead.srmv")
        assert snap_dead == R.write(dim, CODE[dtype], LENS, live, pool0)

        got_map = x.compact(stage)
        np.testing.assert_array_equal(got_map, want_map)
        lens1, live1, pool1, _ = R.compact(LENS, live, pool0, rb)
        assert x.stats() == {"rows": m, "live": m, "tokens": int(lens1.sum())}
        assert x.nbytes == int(lens1.sum()) * rb and x.dtype == dtype
        for new, old in enumerate(keep):
            g = x.get(new)
            assert g.shape == got0[old].shape
            np.testing.assert_array_equal(_u32(g), _u32(got0[old]))
        # offsets, live flags and the pool, byte for byte, through the snapshot
        snap1 = _file(x, tmp_path / "c.srmv")
        assert snap1 == R.write(dim, CODE[dtype], lens1, live1, pool1)
        # scores: index j now holds old row keep[j]; everything at and past m is out of range
        after = _all_scores(x, qs, NROWS)
        want = np.full(before.shape, -np.inf, F)
        want[:, :m] = before[:, keep]
        np.testing.assert_array_equal(_u32(after), _u32(want))
        # a second compaction is the identity
        np.testing.assert_array_equal(x.compact(stage), np.arange(m))
        assert _file(x, tmp_path / "c2.srmv") == snap1
        # it goes on living: both adds and a removal, against a fresh index holding the same rows
        fresh = _new(dim, dtype)
        fresh.add([docs[r] for r in keep])
        for y in (x, fresh):
            assert y.add(extra[:2]) == m
            assert _add_dev(y, extra[2:], dim) == m + 2
            y.remove([m + 2] + ([0] if m else []))
        assert x.stats() == fresh.stats() == {"rows": m + 4, "live": m + 3 - (1 if m else 0),
                                             "tokens": int(lens1.sum()) + 24}
        np.testing.assert_array_equal(_u32(_all_scores(x, qs, m + 4)), _u32(_all_scores(fresh, qs, m + 4)))
        assert _file(x, tmp_path / "a.srmv") == _file(fresh, tmp_path / "b.srmv")
        x.close()
        fresh.close()


def test_compaction_of_a_pool_past_2_31_bytes():
    """270 rows of 4096 fp16 tokens at dim 1024: 2.1 GiB, so the byte offsets of the moved tokens pass
    2^31.  Row 0 dies and an 8 MiB stage makes every chunk direct (gap 4096 >= 4096 stage tokens); then
    row 120 of the rest dies and the default stage makes every chunk staged (a gap of 4096 tokens, 8 MiB, is below the 16 MiB
    from which a chunk goes direct)."""
    import torch
    dim, ld, n = 1024, 4096, 270
    x = _new(dim, "fp16")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    lens = torch.full((54,), ld, dtype=torch.int32, device="cuda")
    for i in range(0, n, 54):
        t = torch.randn((54, ld, dim), dtype=torch.float32, device="cuda", generator=gen)
        x.add_dev((t / t.norm(dim=-1, keepdim=True)).to(torch.float16), lens)
        del t
    assert x.stats() == {"rows": n, "live": n, "tokens": n * ld} and x.nbytes > 1 << 31
    q = [CR.unit_f16(np.random.default_rng(3), 17, dim)]
    probe = [1, 99, 101, 150, n - 1]
    tok = {r: x.get(r) for r in probe}
    before = x.score_rows(q, np.asarray([probe], np.int64))
    live = np.ones(n, bool)
    for dead, stage, staged in ((0, ld * dim * 2, False), (120, 0, True)):
        plan = R.plan([ld] * live.size, live & (np.arange(live.size) != dead), (stage or R.DEFAULT_STAGE_BYTES) // (dim * 2),
                      R.DIRECT_MIN_BYTES // (dim * 2))
        assert plan and all(s == staged for _, _, s in plan) and plan[-1][1] * dim * 2 > 1 << 31
        x.remove([dead])
        o2n = x.compact(stage)
        live[dead] = False
        np.testing.assert_array_equal(o2n, R.old_to_new(live))
        live = live[live]
        probe = [int(o2n[r]) for r in probe]
        assert min(probe) >= 0 and x.stats() == {"rows": live.size, "live": live.size, "tokens": live.size * ld}
        np.testing.assert_array_equal(_u32(x.score_rows(q, np.asarray([probe], np.int64))), _u32(before))
    for r, old in zip(probe, tok):
        np.testing.assert_array_equal(_u32(x.get(r)), _u32(tok[old]))
    x.close()


# -- snapshots -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype", CONFIGS)
def test_snapshot_round_trip_and_life_after_load(dim, dtype, tmp_path):
    from super_rag_amd.multivec import NativeMultiVectorIndex
    docs, extra, qs = _data(dim)
    dead = PATTERNS["alternating"]
    live = np.ones(NROWS, bool)
    live[dead] = False
    x = _new(dim, dtype)
    x.add(docs)
    x.remove(dead)
    pool0, got0 = _pool_of(x, docs, dim, dtype)
    snap = _file(x, tmp_path / "x.srmv")
    assert snap == R.write(dim, CODE[dtype], LENS, live, pool0)          # tombstoned rows included
    assert not os.path.exists(str(tmp_path / "x.srmv") + ".tmp")
    y = NativeMultiVectorIndex.load(str(tmp_path / "x.srmv"))
    assert (y.dim, y.dtype, y.device) == (dim, dtype, 0)
    assert y.stats() == x.stats() and y.nbytes == x.nbytes
    for r in range(NROWS):
        np.testing.assert_array_equal(_u32(y.get(r)), _u32(got0[r]))
    np.testing.assert_array_equal(_u32(_all_scores(y, qs, NROWS)), _u32(_all_scores(x, qs, NROWS)))
    assert _file(y, tmp_path / "y.srmv") == snap                         # load -> save reproduces the file
    # load -> compact -> save equals compact -> save, and both take adds and removals alike afterwards
    rb = R.row_bytes(dim, CODE[dtype])
    np.testing.assert_array_equal(y.compact(3 * rb), x.compact())
    assert _file(y, tmp_path / "yc.srmv") == _file(x, tmp_path / "xc.srmv")
    m = int(live.sum())
    for z in (x, y):
        assert z.add(extra[:2]) == m
        assert _add_dev(z, extra[2:], dim) == m + 2
        z.remove([1, m + 3])
    np.testing.assert_array_equal(_u32(_all_scores(y, qs, m + 4)), _u32(_all_scores(x, qs, m + 4)))
    np.testing.assert_array_equal(y.compact(), x.compact(rb))
    assert _file(y, tmp_path / "yd.srmv") == _file(x, tmp_path / "xd.srmv")
    x.close()
    y.close()


@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_empty_index_round_trips(dtype, tmp_path):
    from super_rag_amd.multivec import NativeMultiVectorIndex
    x = _new(128, dtype)
    np.testing.assert_array_equal(x.compact(), np.zeros(0, np.int64))
    snap = _file(x, tmp_path / "e.srmv")
    assert snap == R.write(128, CODE[dtype], [], [], np.zeros(0, np.uint8))
    y = NativeMultiVectorIndex.load(str(tmp_path / "e.srmv"))
    assert (y.dim, y.dtype) == (128, dtype) and y.stats() == {"rows": 0, "live": 0, "tokens": 0}
    assert _file(y, tmp_path / "e2.srmv") == snap
    d = CR.unit_f16(np.random.default_rng(0), 5, 128)
    assert y.add([d]) == 0 and x.add([d]) == 0
    q = [CR.unit_f16(np.random.default_rng(1), 4, 128)]
    np.testing.assert_array_equal(_u32(y.score_rows(q, np.array([[0]]))), _u32(x.score_rows(q, np.array([[0]]))))
    # every row dead: compaction empties the index, which then still works
    y.remove([0])
    np.testing.assert_array_equal(y.compact(), np.array([-1]))
    assert y.stats() == {"rows": 0, "live": 0, "tokens": 0}
    assert _file(y, tmp_path / "e3.srmv") == snap
    assert y.add([d]) == 0
    np.testing.assert_array_equal(_u32(y.score_rows(q, np.array([[0]]))), _u32(x.score_rows(q, np.array([[0]]))))
    x.close()
    y.close()


@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_corrupt_snapshots_are_refused_and_the_process_keeps_working(dtype, tmp_path):
    from super_rag_amd import _native as NV
    from super_rag_amd.multivec import NativeMultiVectorIndex
    good, lens, live = R.example(CODE[dtype])
    p = tmp_path / "c.srmv"
    cases = R.corruptions(good)
    assert len(cases) > len(good)
    for name, bad in cases:
        p.write_bytes(bad)
        with pytest.raises(NV.NativeError) as e:
            NativeMultiVectorIndex.load(str(p))
        assert e.value.code == NV.SR_ERR_IO, name
    with pytest.raises(NV.NativeError) as e:
        NativeMultiVectorIndex.load(str(tmp_path / "missing.srmv"))
    assert e.value.code == NV.SR_ERR_IO
    p.write_bytes(good)
    y = NativeMultiVectorIndex.load(str(p))
    assert y.stats() == {"rows": 3, "live": 2, "tokens": 3} and y.dtype == dtype
    assert _file(y, tmp_path / "again.srmv") == good
    y.close()


def test_failed_save_leaves_the_previous_snapshot_intact(tmp_path):
    from super_rag_amd import _native as NV
    docs, _, _ = _data(64)
    x = _new(64, "fp16")
    x.add(docs[:4])
    p = tmp_path / "keep.srmv"
    snap = _file(x, p)
    x.add(docs[4:6])
    with pytest.raises(NV.NativeError) as e:
        x.save(str(tmp_path / "no_such_dir" / "x.srmv"))
    assert e.value.code == NV.SR_ERR_IO
    os.mkdir(str(p) + ".tmp")                       # the writer cannot open its temporary file
    with pytest.raises(NV.NativeError) as e:
        x.save(str(p))
    assert e.value.code == NV.SR_ERR_IO
    assert p.read_bytes() == snap
    os.rmdir(str(p) + ".tmp")
    assert _file(x, p) != snap and x.stats()["rows"] == 6
    x.close()


# -- the collection as one ---------------------------------------------------------------------------------------
def _aligned_inputs(seed=83):
    dim, hidden, n = 128, 128, 14
    rng = np.random.default_rng(seed)
    mv_q = [CR.unit_f16(rng, k, dim) for k in (6, 17)]
    alphas = rng.permutation(np.linspace(0.05, 0.9, n))
    mv_d = [CR.mixed_doc(rng, mv_q[i % 2], 20 + int(rng.integers(0, 12)), a) for i, a in enumerate(alphas)]
    dense_d = CR.unit(rng.standard_normal((n, hidden))).astype(F)
    dense_q = CR.unit(rng.standard_normal((2, hidden))).astype(F)
    sparse_d = [{int(t): float(w) for t, w in zip(rng.permutation(30)[:6], rng.uniform(0.1, 2.0, 6))} for _ in range(n)]
    sparse_q = [{int(t): float(w) for t, w in zip(rng.permutation(30)[:8], rng.uniform(0.1, 2.0, 8))} for _ in range(2)]
    return dim, hidden, n, mv_q, mv_d, dense_d, dense_q, sparse_d, sparse_q


def _reference_scores(mv_q, mv_d, dense_d, dense_q, sparse_d, sparse_q, rows, live):
    """fp64 cosine and MaxSim, the impact reference's score: the three terms of the combined score."""
    import impact_ref as IR
    from super_rag_amd.lexical import weighted_arrays
    cos = np.full(rows.shape, -np.inf)
    dn = dense_d.astype(np.float64)
    for b in range(rows.shape[0]):
        for k, r in enumerate(rows[b]):
            if 0 <= r < len(dn) and live[r]:
                cos[b, k] = float(dn[r] @ dense_q[b].astype(np.float64)) / (np.linalg.norm(dn[r]) * np.linalg.norm(dense_q[b]))
    ms = CR.maxsim_rows(mv_q, mv_d, rows, live)
    off, terms, weights = weighted_arrays(sparse_d)
    sp, _ = IR.score_rows(IR.ImpactCorpus(off, terms, weights, live), sparse_q, rows)
    return cos, ms, sp


def test_compact_aligned_keeps_the_collection_aligned():
    from super_rag_amd.lexical import NativeImpactIndex
    from super_rag_amd.multivec import compact_aligned, m3_rerank
    from super_rag_amd.store import NativeStore
    dim, hidden, n, mv_q, mv_d, dense_d, dense_q, sparse_d, sparse_q = _aligned_inputs()
    dead = [0, 3, 4, 9]
    live = np.ones(n, bool)
    live[dead] = False
    cand = np.stack([np.arange(n), np.arange(n)[::-1]]).astype(np.int64)
    # the inputs separate neighbouring ranks by more than 1e-3 on the reference
    cos, ms, sp = _reference_scores(mv_q, mv_d, dense_d, dense_q, sparse_d, sparse_q, cand, live)
    ref_s, ref_r = CR.rerank(cos, ms, sp, cand, 6)
    assert np.isfinite(ref_s).all() and (ref_s[:, :-1] - ref_s[:, 1:] > 1e-3).all(), ref_s
    full_s, _ = CR.rerank(cos, ms, sp, cand, int(live.sum()))
    assert (full_s[:, :6] == ref_s).all() and (full_s[:, 5] - full_s[:, 6] > 1e-3).all()

    store, mv, impact = NativeStore(hidden), _new(dim, "fp16"), NativeImpactIndex()
    store.add(dense_d)
    mv.add(mv_d)
    impact.add(sparse_d)
    # misaligned parts are refused before anything is touched
    mv.remove(dead[:1])
    with pytest.raises(ValueError):
        compact_aligned(store, mv, impact)
    assert store.count() == (n, n) and mv.stats()["rows"] == n and impact.stats()["rows"] == n
    store.remove(dead)
    mv.remove(dead[1:])
    impact.remove(dead)
    s0, r0 = m3_rerank(store, mv, dense_q, mv_q, cand, 6, impact=impact, q_sparse=sparse_q)
    np.testing.assert_array_equal(r0, ref_r)
    o2n = compact_aligned(store, mv, impact, stage_bytes=3 * dim * 2)
    np.testing.assert_array_equal(o2n, R.old_to_new(live))
    m = int(live.sum())
    assert store.count() == (m, m) and mv.stats()["rows"] == m and impact.stats()["rows"] == m
    mapped = o2n[cand]                                  # dropped candidates become -1
    s1, r1 = m3_rerank(store, mv, dense_q, mv_q, mapped, 6, impact=impact, q_sparse=sparse_q)
    np.testing.assert_array_equal(r1, o2n[r0])          # the same documents in the same order
    np.testing.assert_array_equal(_u32(s1), _u32(s0))
    for o in (store, mv, impact):
        o.close()
