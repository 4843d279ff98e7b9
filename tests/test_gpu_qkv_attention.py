"""GPU: K5c (qkv_attn_kernel, the fused QKV projection + attention of the cross-encoder layers) one
kernel at a time through sr_diag_qkv_attention -- the product instantiations <false> (bias epilogue)
and <true> (LayerNorm fold), launched as encoder.cpp launches them.  Operands and references:
tests/attn_ref.py (its docstring derives the gap condition of the exact cases and the bound).

  selector / decoy cases   softmax is exactly one-hot (gap >= 160 log2 units, asserted on the CPU), Q,
                           K, V exact through the dyadic GEMM: ctx == V[winner] bit for bit
  uniform cases            K = 0: ctx = mean of the live V rows, fp16(ref) exactly for a power-of-two
                           n_live, else within the one-ulp straddle rule (attn_ref.uniform_bracket)
  random offset rows       fp64 reference within the derived per-element bound
  unfused pair             bit for bit against sr_diag_gemm_fold / sr_diag_gemm + sr_diag_attention 1
Shapes: heads 1 (d = 64: one K-step), 2 (both staging groups), 12 (head groups of 6), 16 (of 8); B 1 - 3
(odd B: the last panel holds one sequence) and B = 45 x 12 heads = 276 tiles (walkers take several);
lda = d and d + 8 (gap columns poisoned); guard rows past B S; ragged, holed and fully masked
sequences; junk in masked tokens' X rows and mr that must not reach a live query.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -1234.0
GUARD = 8


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _launch(case):
    """One sr_diag_qkv_attention launch -> ctx [B, S, d] fp16 (numpy); the guard rows must be untouched."""
    import torch
    from super_rag_amd import _native as NT
    B, S, d = case["B"], case["S"], case["d"]
    X, W, bias, mask = _dev(case["X"]), _dev(case["W"]), _dev(case["bias"]), _dev(case["mask"])
    lnf = case["epi"] == 5
    colsum, mr = (_dev(case["colsum"]), _dev(case["mr"])) if lnf else (None, None)
    ctx = torch.full((B * S + GUARD, d), SENTINEL, device="cuda:0", dtype=torch.float16)
    NT.call_diag("sr_diag_qkv_attention", case["epi"], X.data_ptr(), case["lda"], W.data_ptr(), bias.data_ptr(),
                 colsum.data_ptr() if lnf else None, mr.data_ptr() if lnf else None, mask.data_ptr(),
                 ctx.data_ptr(), B, S, d, case["heads"], 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((ctx[B * S:] == SENTINEL).all()), "rows past B S were written"
    return ctx[:B * S].cpu().numpy().reshape(B, S, d)


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("epi", [0, 5])
@pytest.mark.parametrize("heads,pats,pad", A.K5C_SELECTOR, ids=lambda v: _ids(v))
def test_k5c_selector_exact(heads, pats, pad, epi):
    case = A.k5c_case(heads, pats, epi, heads * 10 + epi, pad)
    assert case["gap_min"] >= A.GAP_MIN
    got, ck = _launch(case), case["check"]
    assert np.array_equal(got[ck], case["expect"][ck]), \
        f"{int((got[ck] != case['expect'][ck]).sum())} of {case['expect'][ck].size} elements differ"
    # other junk in the masked tokens' X rows and mr: not one bit of a live query may change
    other = A.k5c_case(heads, pats, epi, heads * 10 + epi, pad, junk_seed=1)
    assert not np.array_equal(other["X"], case["X"]) or case["masks"].all()
    assert np.array_equal(_launch(other)[ck], got[ck])


@pytest.mark.parametrize("epi", [0, 5])
def test_k5c_selector_many_tiles(epi):
    heads, pats, pad = A.K5C_MANY                       # 23 panels x 12 heads = 276 tiles over 256 walkers
    case = A.k5c_case(heads, pats, epi, 99 + epi, pad)
    got, ck = _launch(case), case["check"]
    assert np.array_equal(got[ck], case["expect"][ck])


@pytest.mark.parametrize("epi", [0, 5])
@pytest.mark.parametrize("heads,pats,pad", [A.K5C_SELECTOR[i] for i in (1, 3, 4, 6)], ids=lambda v: _ids(v))
def test_k5c_uniform(heads, pats, pad, epi):
    case = A.k5c_case(heads, pats, epi, heads * 10 + epi, pad, uniform=True)
    got, ck = _launch(case), case["check"]
    B, S, d = got.shape
    lo, hi = A.uniform_bracket(np.broadcast_to(case["ref"], (B, S, heads, 64)).reshape(B, S, d), case["nlive"])
    g = got.astype(np.float64)
    ok = (g >= lo.astype(np.float64)) & (g <= hi.astype(np.float64))
    assert ok[ck].all(), f"{int((~ok[ck]).sum())} elements outside the uniform bracket"
    pow2 = [b for b in range(B) if case["nlive"][b] & (case["nlive"][b] - 1) == 0]    # 0 (zero rows), 1, 128
    assert len(pow2) >= (4 in pats) + (3 in pats) + (2 in pats)
    assert all(np.array_equal(got[b][ck[b]], lo[b][ck[b]]) for b in pow2)


@pytest.mark.parametrize("epi", [0, 5])
@pytest.mark.parametrize("heads,pad", [(2, 8), (12, 0)])
def test_k5c_random_bound(heads, pad, epi):
    case = A.k5c_random_case(heads, 3, epi, 7 * heads + epi, pad)
    (Q, K, V), (dQ, dK, dV) = A.k5c_qkv_exact(case)
    ref, bound = A.attention_bound(Q, K, V, case["masks"], 64, dQ, dK, dV)
    got = _launch(case).astype(np.float64).reshape(ref.shape)
    ck = case["masks"]
    ratio = (np.abs(got - ref) / bound)[ck]
    print(f"K5c epi {epi} heads {heads}: max error / bound {ratio.max():.4f}, max |err| {np.abs(got - ref)[ck].max():.3e}")
    assert np.isfinite(got[ck]).all() and ratio.max() <= 1.0


@pytest.mark.parametrize("epi", [0, 5])
@pytest.mark.parametrize("heads", [1, 2, 12, 16])
def test_k5c_equals_unfused_pair(heads, epi):
    """k_attention.hip: 'Numerics equal the unfused pair bit for bit'.  The GEMM wants N % 256 == 0:
    W, bias and colsum are padded with zero rows and the first 3 d columns of its output copied out."""
    import torch
    from super_rag_amd import _native as NT
    case = A.k5c_random_case(heads, 3, epi, 31 * heads + epi, 8 if heads % 2 else 0)
    fused = _launch(case)
    B, S, d = case["B"], case["S"], case["d"]
    M, N = B * S, 3 * d
    Np = (N + 255) // 256 * 256
    pad = lambda a: np.concatenate([a, np.zeros((Np - N,) + a.shape[1:], a.dtype)])
    X, W, bias, mask = _dev(case["X"]), _dev(pad(case["W"])), _dev(pad(case["bias"])), _dev(case["mask"])
    Y = torch.zeros((M, Np), device="cuda:0", dtype=torch.float16)
    st = torch.cuda.current_stream().cuda_stream
    if epi == 5:
        colsum, mr = _dev(pad(case["colsum"])), _dev(case["mr"])
        NT.call_diag("sr_diag_gemm_fold", 0, 5, X.data_ptr(), case["lda"], W.data_ptr(), None, bias.data_ptr(),
                     colsum.data_ptr(), None, 0, mr.data_ptr(), 1, None, Y.data_ptr(), Np, None, None, M, Np, d,
                     0, st)
    else:
        NT.call_diag("sr_diag_gemm", -1, 0, X.data_ptr(), case["lda"], W.data_ptr(), bias.data_ptr(), None, 0,
                     Y.data_ptr(), Np, M, Np, d, 0, st)
    qkv = Y[:, :N].contiguous()
    ctx = torch.full((M, d), SENTINEL, device="cuda:0", dtype=torch.float16)
    NT.call_diag("sr_diag_attention", 1, qkv.data_ptr(), mask.data_ptr(), ctx.data_ptr(), B, S, S, d, heads, 0, st)
    torch.cuda.synchronize()
    pair = ctx.cpu().numpy().reshape(B, S, d)
    assert np.array_equal(fused.view(np.uint16), pair.view(np.uint16))
