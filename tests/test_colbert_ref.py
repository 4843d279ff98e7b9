"""CPU: the multi-vector reference helpers (tests/colbert_ref.py) against plain loops and hand-made
cases, m3_rerank's combination and tie order, encoder.load_colbert_head, and the adversarial
generators the GPU tests rely on (checked to really have their property)."""
import os

import numpy as np
import pytest

import colbert_ref as CR

F = np.float32


def test_head_restatement_equals_the_loops():
    rng = np.random.default_rng(0)
    B, S, d, dc = 2, 6, 5, 4
    h = rng.standard_normal((B, S, d))
    W = rng.standard_normal((dc, d))
    b = rng.standard_normal(dc)
    mask = np.array([[1, 1, 1, 1, 0, 0], [1, 1, 0, 1, 1, 1]], np.int32)   # a prefix and a hole
    got, lens = CR.head(h, mask, W, b)
    want = CR.head_loop(h, mask, W, b)
    assert lens.tolist() == [3, 4] and lens.tolist() == (mask.sum(1) - 1).tolist()
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-14)
        np.testing.assert_allclose(np.linalg.norm(g, axis=1), 1.0, atol=1e-14)


def test_compaction_drops_cls_keeps_the_closing_token_and_follows_the_mask():
    rng = np.random.default_rng(1)
    S, d, dc = 7, 4, 3
    h = rng.standard_normal((1, S, d))
    W, b = rng.standard_normal((dc, d)), rng.standard_normal(dc)
    _, u = CR.head_all(h, W, b)
    # prefix mask of 5: positions 1..4 stay (4 = the closing token), 0 (CLS) never does
    got, lens = CR.head(h, np.array([[1, 1, 1, 1, 1, 0, 0]]), W, b)
    assert lens.tolist() == [4]
    np.testing.assert_array_equal(got[0], u[0, 1:5])
    # a hole at position 2: order kept, the hole skipped; CLS dropped even if it were masked in
    got, lens = CR.head(h, np.array([[1, 1, 0, 1, 1, 1, 0]]), W, b)
    assert lens.tolist() == [4]
    np.testing.assert_array_equal(got[0], u[0, [1, 3, 4, 5]])
    got, lens = CR.head(h, np.array([[0, 1, 1, 0, 0, 0, 0]]), W, b)
    np.testing.assert_array_equal(got[0], u[0, [1, 2]])
    got, lens = CR.head(h, np.array([[1, 0, 0, 0, 0, 0, 0]]), W, b)
    assert lens.tolist() == [0] and got[0].shape == (0, dc)
    # a zero state with a zero bias: the 1e-12 floor keeps the vector at 0
    v, u0 = CR.head_all(np.zeros((1, 2, d)), W, np.zeros(dc))
    assert (u0 == 0).all()


def test_maxsim_equals_the_triple_loop_and_its_inf_cases():
    rng = np.random.default_rng(2)
    for lq, ld, dim in [(1, 1, 3), (3, 5, 8), (7, 2, 16)]:
        q, d = rng.standard_normal((lq, dim)), rng.standard_normal((ld, dim))
        assert abs(CR.maxsim(q, d) - CR.maxsim_loop(q, d)) <= 1e-12
    q = rng.standard_normal((2, 4))
    assert CR.maxsim(q, np.zeros((0, 4))) == -np.inf and CR.maxsim(np.zeros((0, 4)), q) == -np.inf
    # all dot products negative: the maximum is the least negative one, never a padding 0
    qn, dn = np.array([[1.0, 0.0]]), np.array([[-1.0, 0.0], [-0.5, 0.1]])
    assert CR.maxsim(qn, dn) == -0.5
    docs = [q, np.zeros((0, 4)), q[:1]]
    rows = np.array([[0, -1, 3, 1, 2, 0]])
    live = np.array([True, True, False])
    got = CR.maxsim_rows([q], docs, rows, live)
    assert np.isneginf(got[0, [1, 2, 3, 4]]).all()              # -1, past the index, empty, removed
    assert got[0, 0] == got[0, 5] == CR.maxsim(q, q)            # a duplicate scores the same
    assert np.isneginf(CR.maxsim_rows([np.zeros((0, 4))], docs, rows)).all()    # an empty query


def test_combined_score_and_selection_on_hand_made_scores():
    cos = np.array([[0.5, 0.25, 0.75, 0.5, -np.inf]], F)
    ms = np.array([[0.25, 0.5, 0.5, 0.25, 0.5]], F)
    sp = np.array([[1.0, 0.0, 0.5, 1.0, 2.0]], F)
    rows = np.array([[9, 4, 7, 3, 5]], np.int64)
    s3 = CR.combine(cos, ms, sp)
    np.testing.assert_array_equal(s3[0, :4], np.array([1.75, 0.75, 1.75, 1.75], F) / F(3))
    s2 = CR.combine(cos, ms, None, (1, 5, 3))                   # the sparse weight is dropped with its term
    np.testing.assert_array_equal(s2[0, :4], (cos[0, :4] + F(3) * ms[0, :4]) / F(4))
    sc, r = CR.rerank(cos, ms, sp, rows, 5)
    # three candidates tie at 1.75 / 3: the lower row first; the removed one (-inf cosine) stays out
    assert r.tolist() == [[3, 7, 9, 4, -1]]
    assert sc[0, 0] == sc[0, 1] == sc[0, 2] > sc[0, 3] and np.isneginf(sc[0, 4])
    rows2 = rows.copy()
    rows2[0, 2] = -1
    sc, r = CR.rerank(cos, ms, sp, rows2, 2)
    assert r.tolist() == [[3, 9]]
    w = (2, 0, 1)
    np.testing.assert_array_equal(CR.combine(cos, ms, sp, w)[0, :4], (F(2) * cos[0, :4] + ms[0, :4]) / F(3))


def test_combine_dev_matches_the_reference_on_the_cpu():
    torch = pytest.importorskip("torch")
    from super_rag_amd.multivec import combine_dev
    rng = np.random.default_rng(5)
    B, K = 3, 17
    cos = rng.uniform(-1, 1, (B, K)).astype(F)
    ms = rng.uniform(-1, 1, (B, K)).astype(F)
    sp = rng.uniform(0, 4, (B, K)).astype(F)
    rows = np.stack([rng.permutation(40)[:K] for _ in range(B)]).astype(np.int64)
    cos[0, 3] = -np.inf
    rows[1, 5] = -1
    ms[2, 2], cos[2, 2], sp[2, 2] = ms[2, 1], cos[2, 1], sp[2, 1]             # an exact tie
    t = torch.as_tensor
    for sparse, w in ((sp, (1, 1, 1)), (None, (1, 1, 1)), (sp, (0.3, 0.2, 1.5))):
        for k in (1, 5, K, K + 3):
            want_s, want_r = CR.rerank(cos, ms, sparse, rows, k, w)
            got_s, got_r = combine_dev(t(cos), t(ms), None if sparse is None else t(sparse), t(rows), k, w)
            np.testing.assert_array_equal(got_r.numpy(), want_r)
            np.testing.assert_array_equal(got_s.numpy().view(np.uint32), want_s.view(np.uint32))


def test_m3_search_names_a_bad_k_cand_before_any_device_work():
    from super_rag_amd.multivec import m3_search
    q = np.zeros((1, 8), F)
    for k, k_cand in ((10, 1025), (10, 9), (300, 2000)):
        with pytest.raises(ValueError, match="k_cand"):
            m3_search(None, None, q, [q], k, k_cand=k_cand)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k must be"):
            m3_search(None, None, q, [q], k)


def test_load_colbert_head(tmp_path):
    torch = pytest.importorskip("torch")
    from super_rag_amd.encoder import ModelAssetsError, load_colbert_head
    hidden = 64
    assert load_colbert_head(None, hidden) is None and load_colbert_head(str(tmp_path), hidden) is None
    path = os.path.join(str(tmp_path), "colbert_linear.pt")
    w = torch.randn(128, hidden, dtype=torch.float16)
    b = torch.randn(128)
    torch.save({"weight": w, "bias": b}, path)
    gw, gb = load_colbert_head(str(tmp_path), hidden)
    assert gw.dtype == F and gw.shape == (128, hidden) and gb.shape == (128,)
    np.testing.assert_array_equal(gw, w.float().numpy())
    np.testing.assert_array_equal(gb, b.numpy())
    torch.save({"weight": w}, path)                                           # a missing key
    with pytest.raises(ModelAssetsError):
        load_colbert_head(str(tmp_path), hidden)
    torch.save({"weight": w, "bias": b}, path)                                # the wrong hidden size
    with pytest.raises(ModelAssetsError):
        load_colbert_head(str(tmp_path), hidden + 64)
    torch.save({"weight": w, "bias": b[:64]}, path)                           # a bias of another length
    with pytest.raises(ModelAssetsError):
        load_colbert_head(str(tmp_path), hidden)
    torch.save({"weight": w[:96], "bias": b[:96]}, path)                      # dc no multiple of 128
    with pytest.raises(ModelAssetsError):
        load_colbert_head(str(tmp_path), hidden)
    torch.save({"weight": torch.randn(1152, hidden), "bias": torch.randn(1152)}, path)   # dc > 1024
    with pytest.raises(ModelAssetsError):
        load_colbert_head(str(tmp_path), hidden)


@pytest.mark.parametrize("dim", [64, 1024])
def test_adversarial_generators_have_their_property(dim):
    rng = np.random.default_rng(dim)
    for ld in (1, 17, 65):
        q, d = CR.all_negative_case(rng, 5, ld, dim)
        assert (q.astype(np.float64) @ d.astype(np.float64).T).max() < 0
        assert CR.maxsim(q, d) < 0
    for ld in (17, 65, 2049):
        q, d = CR.tail_argmax_case(rng, 33, ld, dim)
        arg = (q.astype(np.float64) @ d.astype(np.float64).T).argmax(axis=1)
        assert (arg >= ld - ld % 16).all(), (ld, arg)
    q, d = CR.first_last_case(rng, 4, 40, dim)
    arg = (q.astype(np.float64) @ d.astype(np.float64).T).argmax(axis=1)
    assert arg[0] == 0 and arg[1] == 39
    # fp16 rounding keeps the vectors at unit length within 2^-10, and the values are fp16 values
    u = CR.unit_f16(rng, 8, dim)
    assert np.abs(np.linalg.norm(u.astype(np.float64), axis=1) - 1).max() < 2.0 ** -10
    np.testing.assert_array_equal(u, u.astype(np.float16).astype(F))
    # the ranking candidates spread over a wide band of scores
    qq = CR.unit_f16(rng, 32, dim)
    lo, hi = CR.maxsim(qq, CR.mixed_doc(rng, qq, 40, 0.0)), CR.maxsim(qq, CR.mixed_doc(rng, qq, 40, 0.9))
    assert lo < 0.5 < 0.8 < hi, (lo, hi)
