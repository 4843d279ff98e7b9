"""GPU: the K5 attention family (attention_kernel<64 / 32>, attention64_kernel in its SPLIT / 4-wave /
8-wave / STREAM forms, attention512_kernel) through sr_diag_attention on operands with an exact
answer (tests/attn_ref.py; its docstring derives the gap condition and the bound):

  selector / decoy cases   one live key ahead of every other by >= 160 log2 units (asserted on the
                           CPU): softmax is one-hot in every evaluation order, ctx == V[winner] bit for
                           bit.  Winners fall in the first and in later key blocks (both rescale
                           directions), decoys put the best key under the mask, masks have holes.
  uniform cases            K = 0: ctx = the mean of the live V rows (fp16(ref) for a power-of-two
                           n_live, else the one-ulp straddle rule)
  fully masked sequence    every kernel computes l = 0 -> inv = 0 -> exact zero rows
  d_h = 32 random          fp64 reference within the derived per-element bound
test_gpu_attention.py keeps the Gaussian 4e-3 parity of the same kernels.
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
VARIANTS = [0, 1, 2, 3, -1]


def _launch(variant, qkv, mask, B, S, Sq, d, heads):
    import torch
    from super_rag_amd import _native as NT
    tq = torch.from_numpy(np.ascontiguousarray(qkv)).to("cuda:0")
    tm = torch.from_numpy(np.ascontiguousarray(mask)).to("cuda:0")
    ctx = torch.full((B * Sq + GUARD, d), SENTINEL, device="cuda:0", dtype=torch.float16)
    NT.call_diag("sr_diag_attention", variant, tq.data_ptr(), tm.data_ptr(), ctx.data_ptr(), B, S, Sq, d, heads,
                 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((ctx[B * Sq:] == SENTINEL).all()), "rows past B Sq were written"
    return ctx[:B * Sq].cpu().numpy().reshape(B, Sq, d)


def _check_selector(variant, case, Sq, reps=1):
    assert case["gap_min"] >= A.GAP_MIN and case["decoys"] > 0
    B, S, d, heads = case["B"], case["S"], case["d"], case["heads"]
    qkv, mask, exp = case["qkv"], case["mask"], case["expect"][:, :Sq]
    if reps > 1:  # the same sequences again: more (sequence, head) tiles than walkers
        qkv, mask, exp = np.tile(qkv, (reps, 1)), np.tile(mask, (reps, 1)), np.tile(exp, (reps, 1, 1))
    got = _launch(variant, qkv, mask, B * reps, S, Sq, d, heads)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} of {exp.size} elements differ"
    dead = ~np.tile(case["masks"], (reps, 1)).any(1)
    assert not dead.any() or not got[dead].any()        # fully masked: exact zeros


def _check_uniform(variant, case, Sq):
    B, S, d, heads, dh = case["B"], case["S"], case["d"], case["heads"], case["dh"]
    got = _launch(variant, case["qkv"], case["mask"], B, S, Sq, d, heads)
    lo, hi = A.uniform_bracket(np.broadcast_to(case["ref"], (B, Sq, heads, dh)).reshape(B, Sq, d), case["nlive"])
    g = got.astype(np.float64)
    ok = (g >= lo.astype(np.float64)) & (g <= hi.astype(np.float64))
    assert ok.all(), f"{int((~ok).sum())} elements outside the uniform bracket"
    n = case["nlive"]
    pow2 = (n & (n - 1)) == 0
    assert pow2.any() and np.array_equal(got[pow2], lo[pow2])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("S,Sq", A.K5_SHAPES)
def test_attention_selector_exact(variant, S, Sq):
    _check_selector(variant, A.selector_qkv(S, 3, 64, A.K5_PATS, S * 7), Sq)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("S,Sq", A.K5_SHAPES)
def test_attention_uniform(variant, S, Sq):
    _check_uniform(variant, A.selector_qkv(S, 3, 64, A.K5_PATS, S * 7, uniform=True), Sq)


@pytest.mark.parametrize("variant", [0, -1])
@pytest.mark.parametrize("S", A.K5_DH32_S)
def test_attention_dh32_exact(variant, S):
    _check_selector(variant, A.selector_qkv(S, 3, 32, A.K5_PATS, S * 11), S)
    _check_uniform(variant, A.selector_qkv(S, 3, 32, A.K5_PATS, S * 11, uniform=True), S)


def test_attention_auto_long_sequence():
    # S > 512: the automatic route takes the 64-key-tile kernel; ten key tiles, winners in every one
    _check_selector(-1, A.selector_qkv(600, 2, 64, A.K5_PATS, 600), 600)
    _check_uniform(-1, A.selector_qkv(600, 2, 64, A.K5_PATS, 600, uniform=True), 600)


def test_attention_k5d_many_tiles_exact():
    # K5d: 70 sequences x 4 heads = 280 tiles over 256 walkers (seven different sequences, ten times)
    case = A.selector_qkv(512, 4, 64, A.K5_PATS + (0,), 4096)
    _check_selector(-1, case, 512, reps=10)


@pytest.mark.parametrize("variant", [0, -1])
@pytest.mark.parametrize("S", A.K5_DH32_S)
def test_attention_dh32_random_bound(variant, S):
    B, heads, dh = 6, 3, 32
    d = heads * dh
    rng = np.random.default_rng(S * 13)
    qkv = (rng.standard_normal((B * S, 3 * d)) * 1.5).astype(np.float16)
    masks = A.pattern_masks((0, 1, 5, 4, 3, 0), S, S)
    x = qkv.astype(np.float64).reshape(B, S, 3, heads, dh)
    ref, bound = A.attention_bound(x[:, :, 0], x[:, :, 1], x[:, :, 2], masks, dh)
    got = _launch(variant, qkv, masks.astype(np.int32), B, S, S, d, heads).astype(np.float64).reshape(ref.shape)
    ratio = np.abs(got - ref) / bound
    print(f"d_h 32 variant {variant} S {S}: max error / bound {ratio.max():.4f}, max |err| {np.abs(got - ref).max():.3e}")
    assert np.isfinite(got).all() and ratio.max() <= 1.0
