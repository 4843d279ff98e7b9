"""CPU checks of tests/attn_ref.py, the host reference of the attention GPU tests:

  * every selector / decoy case the GPU tests run satisfies the gap condition (>= 160 log2 units),
    recomputed here from the fp16 operands the kernel reads;
  * an fp32 / fp16 numpy emulation of the kernels' documented rounding points reproduces the exact
    cases bit for bit and stays inside the derived bound on the random cases;
  * each mutation of the emulation (a plausible kernel bug) fails at least one case the GPU tests
    run; the counts are printed (pytest -s) and quoted in DESIGN.md.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as A  # noqa: E402


def _split(case):
    B, S, H, dh = case["B"], case["S"], case["heads"], case["dh"]
    x = case["qkv"].astype(np.float64).reshape(B, S, 3, H, dh)
    return x[:, :, 0], x[:, :, 1], x[:, :, 2]


K5_CASES = [(S, 3, 64, A.K5_PATS, S * 7) for S in sorted({s for s, _ in A.K5_SHAPES})] + \
           [(S, 3, 32, A.K5_PATS, S * 11) for S in A.K5_DH32_S] + \
           [(600, 2, 64, A.K5_PATS, 600), (512, 4, 64, A.K5_PATS + (0,), 4096)]


@pytest.mark.parametrize("S,heads,dh,pats,seed", K5_CASES, ids=lambda v: str(v) if isinstance(v, int) else "p")
def test_k5_selector_cases_gap(S, heads, dh, pats, seed):
    case = A.selector_qkv(S, heads, dh, pats, seed)
    Q, K, V = _split(case)
    exp, gmin, decoys, win = A.selector_check(Q, K, V, case["masks"], A.LOG2E / math.sqrt(dh))
    assert gmin >= A.GAP_MIN and np.array_equal(A.f16(exp).reshape(case["expect"].shape), case["expect"])
    live = case["masks"].any(1)
    mixed = (live & ~case["masks"].all(1)).sum()             # sequences with live and masked keys
    assert decoys > 0 and (S < 100 or decoys >= 0.15 * mixed * heads * S)   # about a quarter of their queries
    if S > 128:   # winners in the first and in later 128-key blocks
        assert (win[live] < 128).any() and (win[live] >= 128).any()
    assert not case["expect"][~live].any()


@pytest.mark.parametrize("epi", [0, 5])
@pytest.mark.parametrize("heads,pats,pad", A.K5C_SELECTOR + [A.K5C_MANY], ids=lambda v: str(v) if isinstance(v, int) else "p")
def test_k5c_selector_cases_gap_and_exact_gemm(heads, pats, pad, epi):
    many = len(pats) > 3
    case = A.k5c_case(heads, pats, epi, (99 + epi) if many else heads * 10 + epi, pad)
    assert case["gap_min"] >= A.GAP_MIN
    # the GEMM is exact: the fp64 epilogue on the fp16 operands is a multiple of 2^-10 and rounds to the
    # Q | K | V the builder holds, for every live row
    (Q, K, V), _ = A.k5c_qkv_exact(case)
    for got, want in ((Q, case["Q"]), (K, case["K"]), (V, case["V"])):
        m = case["masks"]
        assert np.all(got[m] == np.rint(got[m] * 1024) / 1024) and np.array_equal(A.r16(got[m]), want[m])
    d = case["d"]
    assert (case["bias"] != 0).all()
    if epi == 5:
        assert (case["colsum"][2 * d:] != 0).all() and (case["mr"][case["masks"].reshape(-1), 0] != 0).all()
    if pad:
        assert (case["X"][:, d:] == np.float16(60000.0)).all()
    if not case["masks"].all():
        assert case["decoys"] > 0


ALL_FOLD = [(D, H, S, 3, S) for D, H in A.FOLD_GEOM for S in sorted(set(A.FOLD_S1 + A.FOLD_S2))] + \
           [(768, 12, S, 300, 1) for S in (128, 48)] + [(768, 12, S, 1, 2) for S in (128, 48)]


@pytest.mark.parametrize("D,H,S,B,seed", ALL_FOLD)
def test_fold_selector_cases_gap(D, H, S, B, seed):
    case = A.fold_selector_case(D, H, S, B, seed)
    assert case["gap_min"] >= A.GAP_MIN and case["lo_nonzero"] > 0
    assert case["masks"].any(1).all()            # every sequence keeps a live token
    # recomputed from the operands the kernel reads (junk rows included): fp64 winner and gap per head
    U = case["U"].astype(np.float64).reshape(B, S, D)
    for b in range(min(B, 5)):
        w, mr, live = case["w"][b].astype(np.float64), case["mr"][b].astype(np.float64), case["masks"][b]
        s = mr[None, :, 1] * (w @ U[b].T - mr[None, :, 0] * w.sum(1)[:, None]) * 0.125 * A.LOG2E
        s[:, ~live] = -np.inf
        win = s.argmax(1)
        if live.sum() > 1:
            top2 = np.sort(s, 1)[:, -2:]
            assert (top2[:, 1] - top2[:, 0]).min() >= A.GAP_MIN
        z = mr[win, 1][:, None] * (U[b][win] - mr[win, 0][:, None])
        hi, lo = A.hi_lo(z)
        assert np.array_equal(hi, case["hi"][b]) and np.array_equal(lo, case["lo"][b])


def test_emulation_reproduces_exact_cases():
    c = A.selector_qkv(130, 3, 64, A.K5_PATS, 130 * 7)
    assert np.array_equal(A.emu_attention(c["qkv"], c["masks"], 3, 64), c["expect"])
    c = A.selector_qkv(100, 3, 32, A.K5_PATS, 100 * 11)
    assert np.array_equal(A.emu_attention(c["qkv"], c["masks"], 3, 32), c["expect"])
    for epi in (0, 5):
        c = A.k5c_case(2, (0, 1), epi, 20 + epi, 8)
        assert np.array_equal(A.emu_k5c(c)[c["check"]], c["expect"][c["check"]])
    for S, sr in ((48, True), (128, False)):
        c = A.fold_selector_case(768, 12, S, 3, S)
        hi, lo = A.emu_fold(c, sr)
        assert np.array_equal(hi, c["hi"]) and np.array_equal(lo, c["lo"])


def _k5_random(S=100, heads=3, dh=32, B=6):
    d = heads * dh
    qkv = (np.random.default_rng(S * 13).standard_normal((B * S, 3 * d)) * 1.5).astype(np.float16)
    masks = A.pattern_masks((0, 1, 5, 4, 3, 0), S, S)
    x = qkv.astype(np.float64).reshape(B, S, 3, heads, dh)
    ref, bound = A.attention_bound(x[:, :, 0], x[:, :, 1], x[:, :, 2], masks, dh)
    return qkv, masks, ref, bound


def _k5c_random(epi, heads=2):
    case = A.k5c_random_case(heads, 3, epi, 7 * heads + epi, 8)
    (Q, K, V), (dQ, dK, dV) = A.k5c_qkv_exact(case)
    ref, bound = A.attention_bound(Q, K, V, case["masks"], 64, dQ, dK, dV)
    return case, ref, bound


def _outside(got, ref, bound, rows=None):
    bad = ~(np.abs(got.astype(np.float64).reshape(ref.shape) - ref) <= bound)
    return int(bad.sum() if rows is None else bad[rows].sum())


def test_emulation_inside_bound_on_random_cases():
    qkv, masks, ref, bound = _k5_random()
    assert _outside(A.emu_attention(qkv, masks, 3, 32), ref, bound) == 0
    for epi in (0, 5):
        case, ref, bound = _k5c_random(epi)
        assert _outside(A.emu_k5c(case), ref, bound, case["masks"]) == 0
    for S, sr in ((48, True), (128, False)):
        case = A.fold_random_case(768, 12, S, 3, S + 768)
        ref, bound = A.fold_case_ref(case, sr)
        hi, lo = A.emu_fold(case, sr)
        assert _outside(hi.astype(np.float64) + lo.astype(np.float64), ref, bound) == 0
        assert A.hi_is_nearest(hi, lo)


def test_uniform_bracket_rule():
    ref = np.array([[1.0, 1.0 / 3.0, 2049.0 / 3.0, -0.1]])
    lo, hi = A.uniform_bracket(ref, np.array([4]))
    assert np.array_equal(lo, hi) and np.array_equal(lo, A.f16(ref))
    lo, hi = A.uniform_bracket(ref, np.array([3]))
    assert np.all(np.abs(hi.astype(np.float64) - lo.astype(np.float64)) <= 2 * A.half_ulp16(ref))
    # a reference sitting on a rounding boundary gets both neighbours, nothing else does
    tie = np.array([[1.0 + 2.0 ** -11]])
    lo, hi = A.uniform_bracket(tie, np.array([3]))
    assert float(lo[0, 0]) == 1.0 and float(hi[0, 0]) == 1.0 + 2.0 ** -10


MUTATIONS = ["mask_shift", "kv_swap", "head_off", "scale", "last_kstep", "no_mu_colsum", "no_mu_alpha", "no_sig",
             "no_lo"]


@pytest.mark.parametrize("mut", MUTATIONS)
def test_mutation_fails_a_gpu_case(mut):
    """counts[name] = outputs that differ (exact cases) or leave the bound (random cases)."""
    counts = {}
    if mut in ("mask_shift", "kv_swap", "head_off", "scale"):
        c = A.selector_qkv(130, 3, 64, A.K5_PATS, 130 * 7)
        counts["K5 selector S=130"] = int((A.emu_attention(c["qkv"], c["masks"], 3, 64, mut=mut) != c["expect"]).sum())
        c = A.selector_qkv(130, 3, 64, A.K5_PATS, 130 * 7, uniform=True)
        lo, hi = A.uniform_bracket(np.broadcast_to(c["ref"], (6, 130, 3, 64)).reshape(6, 130, 192), c["nlive"])
        g = A.emu_attention(c["qkv"], c["masks"], 3, 64, mut=mut).astype(np.float64)
        counts["K5 uniform S=130"] = int(((g < lo) | (g > hi)).sum())
        qkv, masks, ref, bound = _k5_random()
        counts["K5 d_h=32 random S=100"] = _outside(A.emu_attention(qkv, masks, 3, 32, mut=mut), ref, bound)
    if mut in ("mask_shift", "kv_swap", "head_off", "scale", "last_kstep", "no_mu_colsum"):
        c = A.k5c_case(2, (0, 1), 5, 25, 8)
        counts["K5c selector H=2 LNF"] = int((A.emu_k5c(c, mut)[c["check"]] != c["expect"][c["check"]]).sum())
        case, ref, bound = _k5c_random(5)
        counts["K5c random H=2 LNF"] = _outside(A.emu_k5c(case, mut), ref, bound, case["masks"])
    if mut in ("no_mu_alpha", "no_sig", "no_lo"):
        for S, sr in ((48, True), (128, False)):
            c = A.fold_selector_case(768, 12, S, 3, S)
            hi, lo = A.emu_fold(c, sr, mut)
            counts[f"fold selector S={S} single_read={sr}"] = int((hi != c["hi"]).sum() + (lo != c["lo"]).sum())
            case = A.fold_random_case(768, 12, S, 3, S + 768)
            ref, bound = A.fold_case_ref(case, sr)
            hi, lo = A.emu_fold(case, sr, mut)
            counts[f"fold random S={S} single_read={sr}"] = _outside(hi.astype(np.float64) + lo.astype(np.float64), ref, bound)
    print(f"mutation {mut}: {counts}")
    assert counts and max(counts.values()) > 0, counts
