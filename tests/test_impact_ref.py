"""CPU: tests/impact_ref.py, the numpy float32 restatement of the impact scoring and of the sparse
head's token -> term collapse, against definitions that share no code with it: an fp64 brute-force
dot product within the bound the fixed point implies, hand-computed roundings, a Python dict loop."""
import numpy as np
import pytest

import impact_ref as IR

F = np.float32


def _corpus(n=300, vocab=60, seed=0):
    rng = np.random.default_rng(seed)
    off, terms, weights = [0], [], []
    for r in range(n):
        cnt = 0 if r % 50 == 0 else int(rng.integers(1, 13))
        t = rng.choice(vocab, cnt, replace=False).tolist()
        if r in (17, 222):
            t.append(t[0])                              # one term in two postings
        terms += t
        weights += np.exp(rng.normal(-1.0, 1.5, len(t))).clip(1e-7, 16.0).tolist()
        off.append(len(terms))
    return IR.ImpactCorpus(off, terms, weights)


def test_fixed_scores_stay_within_the_bound_of_the_fp64_dot_product():
    c = _corpus()
    c.remove(np.arange(3, 300, 11))
    rng = np.random.default_rng(1)
    for _ in range(8):
        qt = rng.choice(60, 9, replace=False)
        qw = np.exp(rng.normal(0.0, 1.0, 9)).astype(F)
        acc = c.fixed_scores((qt, qw))
        dot, shared = IR.dot64(c, (qt, qw))
        # per shared posting: half a unit of 2^-16 from rint, or up to one from the clamp to 1, plus
        # the fp32 product's half ulp (p 2^-24); summed: n_shared 2^-16 + dot 2^-24
        bound = shared * 2.0 ** -16 + dot * 2.0 ** -24
        err = np.abs(acc.astype(np.float64) / 65536.0 - dot)
        assert (err <= bound).all(), (err - bound).max()
        assert (acc[~c.live] == 0).all() and (acc[shared == 0] == 0).all()
        assert (acc[(shared > 0) & c.live] >= 1).all()
        assert (shared[[17, 222]] <= 10).all()


def test_a_term_in_two_postings_counts_twice():
    c = IR.ImpactCorpus([0, 2, 3], [5, 5, 5], [0.5, 0.25, 0.5])
    acc = c.fixed_scores(([5], [1.0]))
    assert acc.tolist() == [32768 + 16384, 32768]


def test_clamp_to_one_and_rint_ties():
    # p * 65536 < 0.5 rounds to 0 and is clamped to 1: a match never scores 0
    assert IR.fixed_products(F(2.0 ** -10), F(2.0 ** -10)).item() == 1
    assert IR.fixed_products(F(1e-7), F(1e-7)).item() == 1
    # ties go to even: 0.5 -> 0 -> clamp 1; 1.5 -> 2; 2.5 -> 2; 3.5 -> 4
    for units, want in ((0.5, 1), (1.5, 2), (2.5, 2), (3.5, 4)):
        assert IR.fixed_products(F(units), F(2.0 ** -16)).item() == want
    # the product is rounded to fp32 before it is scaled: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 -> 1 + 2^-11
    x = F(1.0 + 2.0 ** -12)
    assert IR.fixed_products(x, x).item() == int(np.rint(float(F(x * x)) * 65536.0)) == 65536 + 32
    # the largest admissible product
    assert IR.fixed_products(F(16.0), F(16.0)).item() == 256 * 65536


def test_equal_scores_are_ordered_by_row_and_slots_past_the_matches_are_padded():
    c = IR.ImpactCorpus([0, 1, 2, 3, 3, 4], [7, 7, 7, 7], [0.5, 1.0, 0.5, 0.5])
    s, r, f = IR.topk(c, [([7], [2.0])], 6)
    assert r[0].tolist() == [1, 0, 2, 4, -1, -1]
    assert f[0].tolist() == [131072, 65536, 65536, 65536, 0, 0]
    assert s[0, :4].tolist() == [2.0, 1.0, 1.0, 1.0] and np.isneginf(s[0, 4:]).all()
    s1, r1, _ = IR.topk(c, [([7], [2.0])], 2)
    assert r1[0].tolist() == [1, 0]
    c.remove([0])
    assert IR.topk(c, [([7], [2.0])], 2)[1][0].tolist() == [1, 2]
    allow = np.array([1, 0, 1, 1, 1], np.uint8)
    assert IR.topk(c, [([7], [2.0])], 3, allow=allow)[1][0].tolist() == [2, 4, -1]
    sc, fx = IR.score_rows(c, [([7], [2.0])], [[-1, 5, 0, 3, 1]])
    assert fx[0].tolist() == [0, 0, 0, 0, 131072]
    assert np.isneginf(sc[0, :3]).all() and sc[0, 3] == 0.0 and sc[0, 4] == 2.0


def test_query_preparation():
    qd = IR.prepare_query([4, 9, 4, 2, 9, 4], [0.5, 0.0, 2.0, 1.0, 0.25, 1.5])
    assert list(qd.items()) == [(4, F(2.0)), (2, F(1.0)), (9, F(0.25))]   # max, first occurrence, zero dropped
    qd = IR.prepare_query([4, -1, 2 ** 26, 77, 2], [1, 1, 1, 1, 1], scored=lambda t: t in (4, 2))
    assert list(qd) == [4, 2]
    for bad in (-0.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            IR.prepare_query([1], [bad])
    c = IR.ImpactCorpus([0, 1, 2], [3, 8], [1.0, 1.0])
    c.remove([1])
    assert c.scored(3) and not c.scored(8) and not c.scored(99)
    assert c.fixed_scores(([8, 99, -4], [1.0, 1.0, 1.0])).tolist() == [0, 0]
    for w in (0.0, -1.0, np.nan, 16.5, np.inf):
        with pytest.raises(ValueError):
            IR.ImpactCorpus([0, 1], [1], [w])


def test_overflow_predicate_at_its_boundary():
    # one term: 16 w 2^16 + 1 >= 2^32  <=>  w >= (2^32 - 1) / 2^20 = 4096 - 2^-20; fp32 spacing below
    # 4096 is 2^-12, so 4096 is rejected and its predecessor passes
    below = np.nextafter(F(4096.0), F(0.0))
    assert not IR.overflows({1: below}) and IR.overflows({1: F(4096.0)})
    assert IR.query_bound({1: below}) == 2.0 ** 32 - 256.0 + 1.0
    IR.prepare_query([1], [below])
    with pytest.raises(ValueError):
        IR.prepare_query([1], [4096.0])
    # the + 1 of every term counts: 256 terms of 16 (2^28 each) reach 2^32 + 256, 255 do not
    assert IR.overflows({t: F(16.0) for t in range(256)})
    assert not IR.overflows({t: F(16.0) for t in range(255)})
    # repeats keep one maximum, so they do not add up; a zero weight adds nothing
    IR.prepare_query([5] * 300 + [6], [16.0] * 300 + [0.0])
    # and the bound is what it claims: the largest row sum a passing query can reach stays in uint32
    qd = {t: F(16.0) for t in range(255)}
    worst = sum(int(IR.fixed_products(w, F(16.0))) for w in qd.values())
    assert worst <= IR.query_bound(qd) < 2 ** 32


def _collapse_loop(ids, mask, tw, special):
    out = []
    for b in range(len(ids)):
        d = {}
        for s in range(len(ids[b])):
            t, w = int(ids[b][s]), tw[b][s]
            if mask[b][s] == 0 or not w > 0 or t in special:
                continue
            if t not in d or w > d[t]:
                d[t] = w
        out.append(d)
    return out


@pytest.mark.parametrize("S,vocab", [(33, 6), (128, 50), (257, 250000)])
def test_collapse_equals_a_dict_loop(S, vocab):
    rng = np.random.default_rng(S)
    B = 4
    ids = rng.integers(0, vocab, (B, S))
    tw = np.maximum(rng.normal(0.2, 1.0, (B, S)), 0).astype(F)
    tw[:, ::7] = F(0.75)                                    # equal weights
    mask = np.ones((B, S), np.int32)
    mask[1, S // 2:] = 0
    tw[2] = 0                                               # a sequence that keeps nothing
    ids[0, 3], ids[0, S - 2] = 4, 4                         # a duplicate whose maximum comes later
    tw[0, 3], tw[0, S - 2] = F(0.1), F(9.0)
    special = (0, 2, 5)
    ids[3, S // 2] = 2                                      # a special id in the middle
    tw[3, S // 2] = F(1.0)
    terms, weights, cnt = IR.collapse(ids, mask, tw, special)
    want = _collapse_loop(ids.tolist(), mask, tw, special)
    assert cnt[2] == 0 and cnt[0] > 0
    for b in range(B):
        n = int(cnt[b])
        assert terms[b, :n].tolist() == list(want[b].keys())
        assert weights[b, :n].tolist() == [float(w) for w in want[b].values()]
        assert (terms[b, n:] == -1).all() and (weights[b, n:] == 0).all()
        assert not set(terms[b, :n].tolist()) & set(special)
    assert weights[0][terms[0].tolist().index(4)] == F(9.0)
    t0, w0, c0 = IR.collapse(ids, mask, tw, ())             # no special ids
    assert (c0 >= cnt).all() and (c0 > cnt).any()
