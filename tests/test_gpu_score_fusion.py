"""GPU: score-based hybrid fusion (k_fuse.hip; sr_score_fuse / sr_score_fuse_dev, sr_store_score_rows /
_dev, sr_hybrid_search_fused, ShardedStore + ShardedLex, SearchPipeline(fusion=...)).

score_fuse is compared with tests/fuse_ref.py BIT FOR BIT (scores, rows and component outputs): both
sides perform the same correctly rounded fp32 operations in the same order, so no tolerance exists.
score_rows is compared with the similarity the scan reports for the same pair within DEV = 1e-6
(device against device, test_gpu_store.py:196) and with the fp64 oracle within EPS = 1e-4 (fp16 query
rounding, test_gpu_store.py:20-22).  sr_hybrid_search_fused, the sharded collection and the pipeline
are compared bit for bit with fuse_ref applied to the lists the device's own list calls return.
Largest deviations observed on an MI355X over this file (printed by the score_rows test): see
DESIGN.md, "Score fusion".
"""
import functools

import numpy as np
import pytest

import fuse_ref as FR
from oracle.cosine_topk import normalize_rows, quantize_like_store

pytestmark = pytest.mark.gpu

EPS = 1e-4
DEV = 1e-6
BIG = 2 ** 32 - 2
SHAPES = [(0, 0), (1, 0), (0, 1), (1, 1), (31, 33), (64, 64), (100, 100), (1000, 24), (1024, 1024),
          (2048, 2048), (2047, 3)]
BATCHES = [1, 3, 33]
OVERLAPS = [0.0, 0.5, 1.0]
ALPHAS = [0.5, 0.3, 0.75, 0.0, 1.0]


def _lists(B, ka, kb, overlap, seed):
    """Two lists per query: distinct rows in [0, 2^32 - 2] (0 and 2^32 - 2 among them), ``overlap`` of
    list b's rows taken from list a, scores on 16-value grids (exact ties are common), about a tenth
    of the entries absent (row -1 with a score that must enter nothing), side scores on list a's grid
    with about a tenth unknown (-inf)."""
    rng = np.random.default_rng(seed)
    ra = np.full((B, ka), -1, np.int64)
    rb = np.full((B, kb), -1, np.int64)
    for b in range(B):
        pool = rng.permutation(np.unique(rng.integers(1, BIG, 2 * (ka + kb) + 8, dtype=np.int64)))[: ka + kb]
        assert len(pool) == ka + kb
        if ka + kb >= 2:                       # the extreme ids are always present
            pool[0], pool[-1] = 0, BIG
        ra[b] = pool[:ka]
        shared = int(round(overlap * min(ka, kb)))
        rb[b, :shared] = rng.permutation(ra[b])[:shared]
        rb[b, shared:] = pool[ka:ka + kb - shared]
        rb[b] = rng.permutation(rb[b])
    sa = (rng.integers(0, 16, (B, ka)) / 16.0).astype(np.float32)
    sb = (rng.integers(0, 16, (B, kb)) / 4.0).astype(np.float32)
    side = (rng.integers(-4, 20, (B, kb)) / 16.0).astype(np.float32)       # below and above the grid
    side[rng.random((B, kb)) < 0.1] = -np.inf
    if ka >= 4:
        gone = rng.random((B, ka)) < 0.1
        ra[gone], sa[gone] = -1, 99.0
    if kb >= 4:
        gone = rng.random((B, kb)) < 0.1
        rb[gone], sb[gone] = -1, -99.0
    return sa, ra, sb, rb, side


def _same(got, ref, what):
    for g, r, name in zip(got, ref, ("fused", "rows", "a", "b")):
        g = np.asarray(g)
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name)
        if g.dtype == np.float32:       # bit equality, -inf included
            np.testing.assert_array_equal(g.view(np.uint32), r.view(np.uint32), err_msg=f"{name} {what}")
        else:
            np.testing.assert_array_equal(g, r, err_msg=f"{name} {what}")


@pytest.mark.parametrize("bi", range(len(BATCHES)))
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_score_fuse_equals_the_reference_bit_for_bit(si, bi):
    import torch
    from super_rag_amd.lexical import score_fuse, score_fuse_dev
    (ka, kb), B = SHAPES[si], BATCHES[bi]
    overlap = OVERLAPS[(si + bi) % 3]                 # every (B, overlap) pair occurs over the shapes
    sa, ra, sb, rb, side = _lists(B, ka, kb, overlap, seed=1000 * si + bi)
    n = ka + kb
    t = lambda a: torch.from_numpy(a).cuda()
    dev = [t(x) for x in (sa, ra, sb, rb, side)]
    combos = [("relative", False), ("floor", True), ("relative", True), ("floor", False)]
    if B == 33:                                       # two of the four per case, all four over the shapes
        combos = combos[:2] if si % 2 == 0 else combos[2:]
    for ci, (mode, with_side) in enumerate(combos):
        alpha = ALPHAS[(si + bi + ci) % len(ALPHAS)]
        min_score = 0.25 if (si + ci) % 4 == 3 else -np.inf
        sd = side if with_side else None
        ref = FR.score_fuse(sa, ra, sb, rb, sd, FR.MODES[mode], alpha, -1.0, 0.0, min_score, 2048)
        what = f"ka={ka} kb={kb} B={B} overlap={overlap} {mode} side={with_side} alpha={alpha}"
        kw = dict(mode=mode, alpha=alpha, min_score=min_score)
        _same(score_fuse(sa, ra, sb, rb, 2048, side_a=sd, **kw), ref, "host " + what)
        for k_out in (1, max(n, 1), 2048):
            k_out = min(k_out, 2048)
            got = score_fuse_dev(dev[0], dev[1], dev[2], dev[3], k_out,
                                 side_a=dev[4] if with_side else None, **kw)
            torch.cuda.synchronize()
            _same([g.cpu().numpy() for g in got], [r[:, :k_out] for r in ref], f"dev k_out={k_out} " + what)


def test_score_fuse_on_the_hand_worked_fixtures():
    import os
    from super_rag_amd.lexical import score_fuse
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuse_fixtures.npz")
    with np.load(path) as z:
        for n in [str(x) for x in z["names"]]:
            c = {k[len(n) + 1:]: z[k] for k in z.files if k.startswith(n + ".")}
            side = c["side_a"][None] if int(c["has_side"]) else None
            s, r, a, b = score_fuse(c["score_a"][None], c["rows_a"][None], c["score_b"][None],
                                    c["rows_b"][None], int(c["k_out"]), int(c["mode"]), float(c["alpha"]),
                                    side, float(c["floor_a"]), float(c["floor_b"]), float(c["min_score"]))
            np.testing.assert_array_equal(r[0], c["want_rows"], err_msg=n)
            np.testing.assert_array_equal(s[0], c["want_score"], err_msg=n)
            if int(c["has_comp"]):
                np.testing.assert_array_equal(a[0], c["want_a"], err_msg=n)
                np.testing.assert_array_equal(b[0], c["want_b"], err_msg=n)


# -- score_rows -------------------------------------------------------------------------------------------
N_ROWS = 300


@functools.lru_cache(maxsize=None)
def _store(dim):
    """A 300-row store with tombstones, its rows, the dead rows; built once per dimension."""
    from super_rag_amd.store import NativeStore
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    s = NativeStore(dim, device=0)
    s.add(x)
    dead = np.arange(7, N_ROWS, 11)
    s.remove(dead)
    return s, x, dead


@pytest.mark.parametrize("dim", [64, 72, 768, 1024])
def test_score_rows_equals_the_scan_and_the_oracle(dim):
    import torch
    s, x, dead = _store(dim)
    live = np.ones(N_ROWS, bool)
    live[dead] = False
    worst = {"scan": 0.0, "oracle": 0.0}
    for B in (1, 33):
        rng = np.random.default_rng(10 * dim + B)
        q = rng.standard_normal((B, dim)).astype(np.float32)
        sims, rows = s.search_sim(q, N_ROWS)                    # the complete ranking of the live rows
        scan = np.full((B, N_ROWS), np.nan, np.float32)
        for b in range(B):
            ok = rows[b] >= 0
            scan[b, rows[b][ok]] = sims[b][ok]
        assert (~np.isnan(scan) == live[None]).all()
        oracle = normalize_rows(q) @ quantize_like_store(x).astype(np.float64).T
        for K in (1, 5, 130):
            r = rng.integers(0, N_ROWS, (B, K)).astype(np.int64)
            bad = rng.random((B, K))
            r[bad < 0.1] = -1
            r[(bad >= 0.1) & (bad < 0.15)] = N_ROWS               # first row past the end
            r[(bad >= 0.15) & (bad < 0.2)] = 2 ** 40
            r[(bad >= 0.2) & (bad < 0.3)] = rng.choice(dead, int(((bad >= 0.2) & (bad < 0.3)).sum()))
            got = s.score_rows(q, r)
            assert got.dtype == np.float32 and got.shape == (B, K)
            valid = (r >= 0) & (r < N_ROWS)
            valid[valid] = live[r[valid]]
            assert np.isneginf(got[~valid]).all() and np.isfinite(got[valid]).all()
            bi, _ = np.nonzero(valid)
            if len(bi):
                d_scan = np.abs(got[valid] - scan[bi, r[valid]])
                d_or = np.abs(got[valid].astype(np.float64) - oracle[bi, r[valid]])
                worst["scan"] = max(worst["scan"], float(d_scan.max()))
                worst["oracle"] = max(worst["oracle"], float(d_or.max()))
            # device variant: fp32 and fp16 queries, rows carrying a row offset; an fp16 query is the
            # same numbers as its fp32 copy, so the host call on that copy is its exact reference
            q_h = q.astype(np.float16)
            for qd, off, want in ((torch.from_numpy(q).cuda(), 0, got),
                                  (torch.from_numpy(q_h).cuda(), 1000, s.score_rows(q_h.astype(np.float32), r))):
                rd = torch.from_numpy(np.where(r >= 0, r + off, r)).cuda()
                gd = s.score_rows_dev(qd.contiguous(), rd, row_offset=off).cpu().numpy()
                np.testing.assert_array_equal(gd.view(np.uint32), want.view(np.uint32))
            # both scan dtypes read the same fp16 rows: identical values
            s.set_scan_dtype("fp8")
            try:
                np.testing.assert_array_equal(s.score_rows(q, r).view(np.uint32), got.view(np.uint32))
            finally:
                s.set_scan_dtype("fp16")
    print(f"score_rows dim={dim}: max |score_rows - scan| = {worst['scan']:.3g}, "
          f"max |score_rows - fp64 oracle| = {worst['oracle']:.3g}")
    assert worst["scan"] <= DEV and worst["oracle"] <= EPS, worst


# -- sr_hybrid_search_fused --------------------------------------------------------------------------------
def _docs(rng, n, vocab, max_len=12):
    return [((rng.zipf(1.3, rng.integers(1, max_len + 1)) - 1) % vocab).tolist() for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _collection():
    """3000 x 64 store + lexical index with tombstones, queries; built once, only read."""
    from super_rag_amd.lexical import NativeLexIndex
    from super_rag_amd.store import NativeStore
    rng = np.random.default_rng(9)
    n, vocab, dim, B = 3000, 300, 64, 5
    docs = _docs(rng, n, vocab)
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    store, lex = NativeStore(dim), NativeLexIndex()
    store.add(vecs)
    lex.add(docs)
    dead = rng.choice(n, 200, replace=False)
    store.remove(dead)
    lex.remove(dead)
    qv = rng.standard_normal((B, dim)).astype(np.float32)
    qs = _docs(rng, B, vocab, max_len=4)
    allow = rng.random(n) < 0.5
    return store, lex, vecs, docs, dead, qv, qs, allow


def _fused_ref(store, lex, qv, qs, k, k_each, fusion, alpha, allow=None, mkey=0, min_score=-np.inf):
    sims, dr = store.search_sim(qv, k_each, allow=allow, mask_key=mkey)
    lsc, lr = lex.search(qs, k_each, allow=allow, mask_key=mkey)
    side = store.score_rows(qv, lr) if fusion == "floor" else None
    return FR.score_fuse(sims, dr, lsc, lr, side, FR.MODES[fusion], alpha, -1.0, 0.0, min_score, k), lr


@pytest.mark.parametrize("fusion", ["relative", "floor"])
def test_hybrid_search_fused_is_score_fuse_of_its_lists(fusion):
    from super_rag_amd.lexical import hybrid_search
    store, lex, _, _, dead, qv, qs, allow = _collection()
    for k, k_each, alpha, al, mkey, ms in ((10, 40, 0.5, None, 0, -np.inf), (80, 40, 0.3, allow, 5, -np.inf),
                                           (7, 100, 0.8, allow, 5, 0.3), (2, 1, 0.5, None, 0, -np.inf)):
        got = hybrid_search(store, lex, qv, qs, k, k_each, allow=al, mask_key=mkey, fusion=fusion,
                            alpha=alpha, min_score=ms, components=True)
        ref, lr = _fused_ref(store, lex, qv, qs, k, k_each, fusion, alpha, al, mkey, ms)
        _same(got, ref, f"{fusion} k={k} k_each={k_each} alpha={alpha}")
        r = got[1][got[1] >= 0]
        assert r.size and not np.isin(r, dead).any()
        if al is not None:
            assert al[r].all()
        s2, r2 = hybrid_search(store, lex, qv, qs, k, k_each, allow=al, mask_key=mkey, fusion=fusion,
                               alpha=alpha, min_score=ms)
        np.testing.assert_array_equal(r2, got[1])
        np.testing.assert_array_equal(s2, got[0])
    # a BM25 hit outside the dense list got its exact cosine in floor mode (and none in relative)
    got = hybrid_search(store, lex, qv, qs, 80, 40, fusion=fusion, components=True)
    only_lex = (got[1] >= 0) & ~np.isin(got[1], store.search_sim(qv, 40)[1])
    assert only_lex.any()
    assert (np.isfinite(got[2][only_lex]).all() if fusion == "floor" else np.isneginf(got[2][only_lex]).all())
    # the default stays rrf: fp64 scores
    assert hybrid_search(store, lex, qv, qs, 5, 10)[0].dtype == np.float64


@pytest.mark.parametrize("fusion", ["relative", "floor"])
def test_two_shards_equal_one_device_bit_for_bit(fusion):
    from super_rag_amd.lexical import ShardedLex
    from super_rag_amd.store import ShardedStore
    store, lex, vecs, docs, dead, qv, qs, allow = _collection()
    sh = ShardedStore(vecs.shape[1], [0, 0])
    shl = ShardedLex(sh)
    for a, b in ((0, 700), (700, 1100), (1100, 2300), (2300, 3000)):     # batches alternate shards
        sh.add(vecs[a:b])
        shl.add(docs[a:b])
    sh.remove(dead)
    shl.remove(dead)
    assert len(set(sh.shard_of.tolist())) == 2
    sa, ra = store.search_sim(qv, 50)
    sb, rb = sh.search_sim(qv, 50)
    np.testing.assert_array_equal(rb, ra)
    np.testing.assert_array_equal(sb.view(np.uint32), sa.view(np.uint32))
    rows = np.random.default_rng(1).integers(-1, 3001, (5, 40))
    np.testing.assert_array_equal(sh.score_rows(qv, rows).view(np.uint32),
                                  store.score_rows(qv, rows).view(np.uint32))
    for k, k_each, alpha, al, mkey in ((10, 40, 0.5, None, 0), (60, 40, 0.25, allow, 7)):
        want = lex.hybrid(store, qv, qs, k, k_each, allow=al, mask_key=mkey, fusion=fusion, alpha=alpha)
        got = shl.hybrid(sh, qv, qs, k, k_each, allow=al, mask_key=mkey, fusion=fusion, alpha=alpha)
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    sh.close()


# -- SearchPipeline ----------------------------------------------------------------------------------------
def test_pipeline_fusion_equals_score_fuse_of_its_candidate_lists(tmp_path):
    import torch
    import torch.distributed as dist
    from super_rag_amd.pipeline import SearchPipeline
    store, lex, vecs, docs, dead, qv, _, _ = _collection()
    rng = np.random.default_rng(2)
    B, Lq, K, ke = qv.shape[0], 4, 30, 20
    q16 = torch.from_numpy(qv).cuda().half().contiguous()
    q_tok = torch.from_numpy(rng.integers(0, 300, (B, Lq)).astype(np.int32)).cuda()
    q_len = torch.from_numpy(rng.integers(1, Lq + 1, B).astype(np.int32)).cuda()

    def want(fusion, alpha):
        sims, rows = store.search_dev(q16, ke)
        lsc, lrows = lex.search_tok_dev(q_tok, q_len, ke)
        side = store.score_rows_dev(q16, lrows).cpu().numpy() if fusion == "floor" else None
        torch.cuda.synchronize()
        ref = FR.score_fuse(sims.cpu().numpy(), rows.cpu().numpy(), lsc.cpu().numpy(), lrows.cpu().numpy(),
                            side, FR.MODES[fusion], alpha, -1.0, 0.0, -np.inf, K)
        return ref[0], ref[1]

    def run(**kw):
        pipe = SearchPipeline(None, None, store, None, None, k_candidates=K, k_final=5, lexical=lex,
                              k_each=ke, **kw)
        s, r = pipe.retrieve_hybrid(q16, q_tok, q_len)
        torch.cuda.synchronize()
        return s.cpu().numpy(), r.cpu().numpy()

    for fusion, alpha in (("relative", 0.5), ("relative", 0.2), ("floor", 0.6)):
        _same(run(fusion=fusion, alpha=alpha), want(fusion, alpha), f"pipeline {fusion}")
    rrf_s, rrf_r = run()
    assert not np.array_equal(rrf_r, want("relative", 0.5)[1])      # the default is still rrf
    with pytest.raises(ValueError):
        run(fusion="borda")
    with pytest.raises(ValueError):
        run(fusion="relative", alpha=1.5)
    # a world of one with the exchange forced on (gloo, staged through host memory)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        _same(run(fusion="relative", alpha=0.5, force_exchange=True), want("relative", 0.5),
              "pipeline relative, exchange")
        with pytest.raises(ValueError):
            run(fusion="floor", force_exchange=True)
    finally:
        dist.destroy_process_group()
