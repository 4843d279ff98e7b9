"""GPU: the weight-side helpers of the LayerNorm fold and the fp8 plan, one kernel each (through
sr_diag_quantize_rows_fp8 / sr_diag_colsum_fp8 / sr_diag_fold_ln_weight / sr_diag_ln_stats_finalize)
against the exact / fp64 references of tests/fold_ref.py.

Bounds (u = 2^-24, the fp32 unit roundoff; none comes from a run of the kernels):
  * quantize_rows_fp8: bytes and exponents exact (the scaling is a power of two).
  * colsum_fp8 / fold_ln_weight sums of K terms: K u sum|terms| (any summation order); exact on
    dyadic rows.  fold_ln_weight's w16 = fp16(fp32(w) fp32(gamma)): numpy does the same two roundings.
  * ln_stats_finalize, mu: 4 u max_i |S_i / 128|.
  * ln_stats_finalize, rstd (relative), by one rounding per operation of the kernel's formula
        s = sum S_i;  mu = s / n;  d_i = S_i / 128 - mu;  M2 = sum M2_i + sum 128 d_i d_i;
        v = M2 / n + eps;  rstd = 1 / sqrt(v)                       (n = 128 nparts)
    With e = mu^ - mu: |e| <= nparts u A, A = max_i |S_i / 128| (nparts - 1 additions and one
    division, each relative u, on at most n A).  Because sum d_i = 0, the error of mu enters M2
    only in second order: sum 128 (d_i - e)^2 = sum 128 d_i^2 + n e^2.  Every term of M2 is
    non-negative, so its roundings (one subtraction -- twice in the square --, one product and at
    most 2 nparts additions per term) add relatively: <= (2 nparts + 4) u.  v adds the division and
    the addition of eps, 2 u more.  rstd = v^(-1/2) halves the relative error of v; sqrtf and the
    division are taken as faithful (1 ulp = 2 u each):
        |rstd^ - rstd| / rstd <= ((2 nparts + 6) u + (nparts u A)^2 / v) / 2 + 4 u.
    Constant rows (dyadic values): every operation before the square root is exact, so mu is exact
    and rstd = 1 / sqrt(fp32(eps)) within the 4 u of the two faithful roundings.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fold_ref as FR  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _quantize(W16):
    """fp16 numpy [N][K] -> (bytes, wexp, wexp guard) from the device."""
    import torch
    from super_rag_amd import _native as NT
    N, K = W16.shape
    W = torch.from_numpy(W16).to(_dev())
    W8 = torch.full((N, K), 0x7F, device=_dev(), dtype=torch.uint8)
    wexp = torch.full((N + 64,), 0xA5, device=_dev(), dtype=torch.uint8)
    NT.call_diag("sr_diag_quantize_rows_fp8", W.data_ptr(), N, K, W8.data_ptr(), wexp.data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    return W8.cpu().numpy(), wexp[:N].cpu().numpy(), wexp[N:].cpu().numpy()


@pytest.mark.parametrize("K", [256, 768, 3072])
@pytest.mark.parametrize("N", [1, 5, 256])
def test_quantize_rows_fp8_is_exact(N, K):
    rows = FR.quantize_case_rows(K)
    W16 = rows[(np.arange(N) * 7 + (0 if N > 1 else 3)) % len(rows)]   # N = 1: a 1.75 2^j row's successor
    b, wexp, guard = _quantize(W16)
    rb, rexp = FR.quantize_rows_ref(W16)
    assert np.array_equal(wexp, rexp), np.nonzero(wexp != rexp)[0][:8]
    assert np.array_equal(b, rb), int((b != rb).sum())
    assert np.all(guard == 0xA5), "wexp bytes past N were written"


def test_quantize_rows_fp8_every_edge_row():
    rows = FR.quantize_case_rows(256)
    b, wexp, guard = _quantize(rows)
    rb, rexp = FR.quantize_rows_ref(rows)
    assert np.array_equal(wexp, rexp) and np.array_equal(b, rb) and np.all(guard == 0xA5)


def _colsum(W8, wexp):
    import torch
    from super_rag_amd import _native as NT
    N, K = W8.shape
    w = torch.from_numpy(W8).to(_dev())
    e = torch.from_numpy(wexp).to(_dev())
    out = torch.full((N + 16,), 777.0, device=_dev())
    NT.call_diag("sr_diag_colsum_fp8", w.data_ptr(), e.data_ptr(), N, K, out.data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[N:] == 777.0), "colsum past N was written"
    return o[:N].astype(np.float64)


@pytest.mark.parametrize("N,K", [(1, 256), (5, 768), (256, 3072)])
def test_colsum_fp8(N, K):
    rng = np.random.default_rng(N + K)
    # random rows through the reference quantiser (every exponent the edge rows produce)
    W16 = (rng.standard_normal((N, K)) * 0.04).astype(np.float16)
    edge = FR.quantize_case_rows(K)
    W16[: min(N, len(edge))] = edge[: min(N, len(edge))]
    W8, wexp = FR.quantize_rows_ref(W16)
    Wd = FR.dequant_rows(W8, wexp)
    got, ref = _colsum(W8, wexp), Wd.sum(1)
    bound = K * U * np.abs(Wd).sum(1)
    err = np.abs(got - ref)
    print(f"colsum_fp8 N {N} K {K}: max err / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}")
    assert np.all(err <= bound)
    # dyadic rows: integers (|w| <= 8) under exponents 95 .. 135: exact in any order
    iw = rng.integers(-8, 9, (N, K)).astype(np.float64)
    wexp = FR.WEXP_CYCLE[np.arange(N) % 16].astype(np.uint8)
    W8 = FR.e4m3_bytes(iw)
    got = _colsum(W8, wexp)
    assert np.array_equal(got, FR.dequant_rows(W8, wexp).sum(1))


@pytest.mark.parametrize("K", [256, 768, 1024])
@pytest.mark.parametrize("N", [1, 3, 256])
def test_fold_ln_weight(N, K):
    import torch
    from super_rag_amd import _native as NT
    rng = np.random.default_rng(N * K)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    gamma = (1.0 + 0.3 * rng.standard_normal(K)).astype(np.float32)
    gamma[::7] *= -1.0
    gamma[3::11] = 0.0
    beta = (0.2 * rng.standard_normal(K)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    d = _dev()
    tw, tg, tb, tbias = (torch.from_numpy(a).to(d) for a in (w, gamma, beta, bias))
    w16 = torch.full((N + 2, K), 1234.0, device=d, dtype=torch.float16)
    colsum = torch.full((N + 16,), 777.0, device=d)
    bout = torch.full((N + 16,), 777.0, device=d)
    NT.call_diag("sr_diag_fold_ln_weight", tw.data_ptr(), tg.data_ptr(), tb.data_ptr(), tbias.data_ptr(), N, K,
                 w16.data_ptr(), colsum.data_ptr(), bout.data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    want16 = (w * gamma[None, :]).astype(np.float32).astype(np.float16)   # fp32 product, then fp16
    got16 = w16.cpu().numpy()
    assert np.array_equal(got16[:N].view(np.uint16), want16.view(np.uint16))
    assert np.all(got16[N:] == np.float16(1234.0)) and np.all(colsum[N:].cpu().numpy() == 777.0)
    assert np.all(bout[N:].cpu().numpy() == 777.0)
    h = want16.astype(np.float64)
    err_c = np.abs(colsum[:N].cpu().numpy().astype(np.float64) - h.sum(1))
    bound_c = K * U * np.abs(h).sum(1)
    terms = w.astype(np.float64) * beta.astype(np.float64)[None, :]
    err_b = np.abs(bout[:N].cpu().numpy().astype(np.float64) - (terms.sum(1) + bias))
    bound_b = K * U * (np.abs(terms).sum(1) + np.abs(bias))
    print(f"fold_ln_weight N {N} K {K}: colsum err / bound {np.max(err_c / bound_c):.3f}, "
          f"bias err / bound {np.max(err_b / bound_b):.3f}")
    assert np.all(err_c <= bound_c) and np.all(err_b <= bound_b)


def _finalize_rows(M, nparts, rng):
    """Synthetic rows [M][128 nparts] (fp64): centred, |mean| / std = 600, and constant dyadic rows."""
    n = 128 * nparts
    x = rng.standard_normal((M, n))
    kind = np.arange(M) % 4
    x[kind == 1] = x[kind == 1] * 0.5 + 300.0                      # |mean| / std = 600
    x[kind == 2] = x[kind == 2] * 0.01 - 6.0
    const = np.array([3.0, -0.5, 100.0, 0.0])[(np.arange(M) // 4) % 4]
    x[kind == 3] = const[kind == 3][:, None]
    return x, kind == 3


@pytest.mark.parametrize("eps", [1e-5, 1e-12])
@pytest.mark.parametrize("M", [1, 255, 257, 1000])
@pytest.mark.parametrize("nparts", [1, 2, 6, 8, 16])
def test_ln_stats_finalize(nparts, M, eps):
    import torch
    from super_rag_amd import _native as NT
    rng = np.random.default_rng(nparts * 1000 + M)
    x, const = _finalize_rows(M, nparts, rng)
    if M == 1:
        const[:] = False
    spans = x.reshape(M, nparts, 128)
    S = spans.sum(-1)
    M2 = ((spans - spans.mean(-1, keepdims=True)) ** 2).sum(-1)
    stat32 = np.stack([S, M2], -1).astype(np.float32)              # the partials the kernel reads
    d = _dev()
    st = torch.from_numpy(stat32).to(d)
    GUARD = 33
    mr = torch.full((M + GUARD, 2), 777.0, device=d)
    NT.call_diag("sr_diag_ln_stats_finalize", st.data_ptr(), nparts, float(eps), M, mr.data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    out = mr.cpu().numpy().astype(np.float64)
    assert np.all(out[M:] == 777.0), "rows past M were written"
    S64, M264 = stat32[..., 0].astype(np.float64), stat32[..., 1].astype(np.float64)
    n = 128.0 * nparts
    eps32 = float(np.float32(eps))
    mu = S64.sum(1) / n
    m2 = M264.sum(1) + (128.0 * (S64 / 128.0 - mu[:, None]) ** 2).sum(1)
    v = m2 / n + eps32
    rstd = 1.0 / np.sqrt(v)
    A = np.abs(S64 / 128.0).max(1)
    err_mu = np.abs(out[:M, 0] - mu)
    bound_mu = 4.0 * U * A
    rel = np.abs(out[:M, 1] - rstd) / rstd
    bound = ((2 * nparts + 6) * U + (nparts * U * A) ** 2 / v) / 2.0 + 4.0 * U
    gen = ~const
    rm = np.max(err_mu[gen] / np.maximum(bound_mu[gen], 1e-300))
    rr = np.max(rel[gen] / bound[gen])
    print(f"ln_stats_finalize nparts {nparts} M {M} eps {eps}: mu err / bound {rm:.3f}, rstd err / bound {rr:.3f}")
    assert np.all(err_mu[gen] <= bound_mu[gen])
    assert np.all(rel[gen] <= bound[gen])
    if const.any():
        assert np.array_equal(out[:M, 0][const], mu[const])       # exact
        assert np.all(m2[const] == 0.0)
        assert np.all(np.abs(out[:M, 1][const] * np.sqrt(eps32) - 1.0) <= 4.0 * U)
