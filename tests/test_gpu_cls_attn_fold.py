"""GPU: the K/V-free CLS-only last layer one kernel at a time -- cls_attn_fold1_kernel (single read,
S <= 128), cls_attn_fold_kernel (two passes; S <= 128 by SR_CLS_FOLD_1READ=0) through
sr_diag_cls_attn_fold, and kv_blockdiag_kernel through sr_diag_kv_blockdiag.  Operands and
references: tests/attn_ref.py (its docstring derives the gap condition and the bound).

  selector / decoy cases   every head selects one live token by >= 160 log2 units (asserted on the
                           CPU), so z' = rstd_j (u_j - mu_j) exactly and the output must be the pair
                           hi = fp16(z'), lo = fp16(z' - hi), bit for bit.  mu_j alpha_h and sig_h are
                           far from inert here: dropping either changes thousands of outputs
                           (tests/test_attn_ref.py counts them).
  random offset rows       |mean| up to ~10 standard deviations, ragged / holed masks, junk in the
                           masked tokens' U rows and mr: hi + lo against fp64 within the derived bound,
                           and hi an fp16 nearest to hi + lo (== fp16(hi + lo) except where lo rounded up
                           to exactly half an ulp of hi: attn_ref.hi_is_nearest)
Single read: S 16 .. 128 gives 1 - 4 LDS rounds, waves without rows (has == false) and waves without a
round of their own; B = 300 makes the persistent walkers take two sequences (prefetched rows).  Every
sequence keeps a live token: an all-masked sequence is outside the kernel's contract (sr_kernels.h).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -1234.0
FORMS = [(S, True) for S in A.FOLD_S1] + [(S, False) for S in A.FOLD_S2]


def _launch(case, single_read, monkeypatch):
    """-> (hi, lo) [B, H, D] fp16; SR_CLS_FOLD_1READ is read per launch."""
    import torch
    from super_rag_amd import _native as NT
    B, S, D, H = case["B"], case["S"], case["D"], case["H"]
    assert single_read == (S <= 128 and single_read)
    if S <= 128:
        monkeypatch.setenv("SR_CLS_FOLD_1READ", "1" if single_read else "0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    w, U, mr, mask = t(case["w"]), t(case["U"]), t(case["mr"]), t(case["mask"])
    z = torch.full((B + 1, 2 * H * D), SENTINEL, device="cuda:0", dtype=torch.float16)
    NT.call_diag("sr_diag_cls_attn_fold", w.data_ptr(), U.data_ptr(), mr.data_ptr(), mask.data_ptr(), B, S, D, H,
                 z.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((z[B:] == SENTINEL).all()), "the row past B was written"
    zz = z[:B].cpu().numpy().reshape(B, 2, H, D)
    return zz[:, 0], zz[:, 1]


@pytest.mark.parametrize("D,H", A.FOLD_GEOM)
@pytest.mark.parametrize("S,single_read", FORMS)
def test_fold_selector_exact(D, H, S, single_read, monkeypatch):
    case = A.fold_selector_case(D, H, S, 3, S)
    assert case["gap_min"] >= A.GAP_MIN and case["lo_nonzero"] > 0
    hi, lo = _launch(case, single_read, monkeypatch)
    assert np.array_equal(hi, case["hi"]), f"{int((hi != case['hi']).sum())} hi elements differ"
    assert np.array_equal(lo, case["lo"]), f"{int((lo != case['lo']).sum())} lo elements differ"


@pytest.mark.parametrize("S,single_read", [(128, True), (48, True), (128, False)])
def test_fold_selector_exact_many_sequences(S, single_read, monkeypatch):
    # B = 300 > 256 workgroups: the single-read walkers take a second sequence (rows prefetched
    # during the first one's rounds); B = 1: a lone sequence
    case = A.fold_selector_case(768, 12, S, 300, 1)
    hi, lo = _launch(case, single_read, monkeypatch)
    assert np.array_equal(hi, case["hi"]) and np.array_equal(lo, case["lo"])
    one = A.fold_selector_case(768, 12, S, 1, 2)
    hi, lo = _launch(one, single_read, monkeypatch)
    assert np.array_equal(hi, one["hi"]) and np.array_equal(lo, one["lo"])


@pytest.mark.parametrize("D,H", A.FOLD_GEOM)
@pytest.mark.parametrize("S,single_read", FORMS)
def test_fold_random_bound(D, H, S, single_read, monkeypatch):
    case = A.fold_random_case(D, H, S, 3, S + D)
    ref, bound = A.fold_case_ref(case, single_read)
    hi, lo = _launch(case, single_read, monkeypatch)
    got = hi.astype(np.float64) + lo.astype(np.float64)
    ratio = np.abs(got - ref) / bound
    print(f"fold D {D} S {S} single_read {single_read}: max error / bound {ratio.max():.4f}, "
          f"max |err| {np.abs(got - ref).max():.3e}")
    assert np.isfinite(got).all() and ratio.max() <= 1.0
    assert A.hi_is_nearest(hi, lo), "hi must be an fp16 nearest to hi + lo"


def test_fold_random_bound_many_sequences(monkeypatch):
    case = A.fold_random_case(768, 12, 96, 300, 5)
    ref, bound = A.fold_case_ref(case, True)
    hi, lo = _launch(case, True, monkeypatch)
    got = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.isfinite(got).all() and (np.abs(got - ref) <= bound).all()


@pytest.mark.parametrize("D,H", A.FOLD_GEOM)
def test_kv_blockdiag_exact(D, H):
    import torch
    from super_rag_amd import _native as NT
    # every entry encodes its own (row, column): row r, column c -> the fp16 bit pattern of (37 r + c)
    # mod 30000 + 1024 (finite, non-zero patterns; a misplaced or transposed entry cannot match)
    r, c = np.ix_(np.arange(3 * D), np.arange(D))
    wqkv = (((37 * r + c) % 30000) + 1024).astype(np.uint16).view(np.float16)
    assert np.isfinite(wqkv).all() and (wqkv != 0).all()
    wk_ref, wv_ref = A.kv_blockdiag_ref(wqkv, D, H)
    t = torch.from_numpy(wqkv).to("cuda:0")
    wk = torch.full((H * D, D), SENTINEL, device="cuda:0", dtype=torch.float16)
    wv = torch.full((D, 2 * H * D), SENTINEL, device="cuda:0", dtype=torch.float16)
    NT.call_diag("sr_diag_kv_blockdiag", t.data_ptr(), D, H, wk.data_ptr(), wv.data_ptr(), 0,
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(wk.cpu().numpy().view(np.uint16), wk_ref.view(np.uint16))
    assert np.array_equal(wv.cpu().numpy().view(np.uint16), wv_ref.view(np.uint16))
