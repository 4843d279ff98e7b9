"""GPU: the FFN1 epilogues' GELU tables, clamp and saturation per element (through sr_diag_ffn1,
diag 0: the product kernels gemm_f16_lnfold_gelu / gemm_f8_lnfold_gelu_out8) against 2 GELU in fp64.

Operands are built so that the pre-activation of output (m, n) is known exactly, pre = o_m + b_n:
  * rows carry o_r = (r - 256) / 32, r = m mod 512 (-8 .. 7.97 in steps of 1/32) as exact products:
    fp16 rows are one-hot (x = o / rstd against a weight of 1).  An e4m3 product has an 8-bit
    significand at most and cannot hold (r - 256) / 32 for every r, so fp8 rows carry two entries,
    o = 16 hi / 32 + lo / 32 (hi = -16 .. 15, lo = 0 .. 15, weights 1/2 and 1/32 under the row
    exponent): two exact products whose sum is exact;
  * columns c = n mod 512: c <= 128 the fine grid b = c 2^-12 (+ 1/8 per 256-column tile), so the
    outputs cover [-8, 8] at 2^-12 < h8 / 8; 13 out-of-range columns and 370 columns of non-dyadic
    fp32 values, whose weight rows are zero (pre = b for every row);
  * first launch mu = 0, rstd = 1; second launch rstd_m in {1/2, 1, 2, 4}, mu_m != 0 and a column
    sum c_n != 0, with one more entry x = mu_m against a weight c_n, so acc - mu c = o / rstd exactly
    and rstd (acc - mu c) + b is the same grid;
  * a node launch (16 zero rows, pre = b) puts every e4m3-table node and midpoint inside +-1 (which
    include the fp16 table's), rounded to fp32, through both forms.
Every output must lie in fold_ref.bracket(two_gelu(pre), gelu_slack(pre, form)): the table error
derived from the tables' construction, then the monotone output rounding.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fold_ref as FR  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 48
OUT_OF_RANGE = [5.65, -5.65, 5.66, -5.66, 6.0, -6.0, 50.0, -50.0, 223.9, 224.0, 225.0, 1000.0, -1000.0]
MU = np.array([0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0])


def _dev():
    import torch
    return torch.device("cuda", 0)


def _columns(N):
    """(b [N] fp32, grid [N] bool: the weight row carries the row offsets)."""
    n = np.arange(N)
    c = n % 512
    b = np.zeros(N, np.float64)
    grid = c <= 128
    b[grid] = c[grid] * 2.0 ** -12 + (n[grid] // 256) * 0.125
    oor = (c > 128) & (c < 129 + len(OUT_OF_RANGE))
    b[oor] = np.array(OUT_OF_RANGE)[c[oor] - 129]
    rest = c >= 129 + len(OUT_OF_RANGE)
    b[rest] = -8.0 + 16.0 * (c[rest] - 142) / 369.0 + (n[rest] // 512) * 0.01
    return b.astype(np.float32), grid


def _build(f8, M, N, K, second):
    """-> dict(X, W, wexp, bias, colsum, mr: device tensors; pre: fp64 [512][N] by r = m mod 512)."""
    import torch
    d = _dev()
    m = np.arange(M)
    r = m % 512
    j = r - 256
    if second:
        rstd = 2.0 ** (((m * 5 + m // 512) % 4) - 1)
        mu = MU[(m * 3 + m // 512) % 8]
    else:
        rstd, mu = np.ones(M), np.zeros(M)
    b32, grid = _columns(N)
    n = np.arange(N)
    cn = (((n * 3 + n // 256) % 7) - 3) / 2.0
    cn[cn == 0.0] = 2.0
    X = np.zeros((M, K))
    W = np.zeros((N, K))
    if f8:
        hi = np.floor_divide(j, 16)
        lo = j - 16 * hi
        s = 2.0 ** ((n % 5) - 3.0)                                # the row scale 2^(wexp - 127)
        X[m, r % 64] = hi / rstd
        X[m, 64 + r % 64] = lo / rstd
        X[m, 128 + r % 64] = mu
        W[:, 0:64] = np.where(grid, 0.5, 0.0)[:, None]
        W[:, 64:128] = np.where(grid, 2.0 ** -5, 0.0)[:, None]
        W[:, 128:192] = cn[:, None]
        W8v = W / s[:, None]
        X8, W8 = FR.e4m3_bytes(X), FR.e4m3_bytes(W8v)
        assert np.array_equal(FR.e4m3_values(X8), X) and np.array_equal(FR.e4m3_values(W8), W8v)
        wexp = (127 + (n % 5) - 3).astype(np.uint8)
        Xt, Wt = torch.from_numpy(X8).to(d), torch.from_numpy(W8).to(d)
        wexp_t = torch.from_numpy(wexp).to(d)
    else:
        X[m, r % 64] = (j / 32.0) / rstd
        X[m, 64 + r % 64] = mu
        W[:, 0:64] = np.where(grid, 1.0, 0.0)[:, None]
        W[:, 64:128] = cn[:, None]
        X16, W16 = X.astype(np.float16), W.astype(np.float16)
        assert np.array_equal(X16.astype(np.float64), X) and np.array_equal(W16.astype(np.float64), W)
        Xt, Wt, wexp_t = torch.from_numpy(X16).to(d), torch.from_numpy(W16).to(d), None
    # the construction, checked in fp64: acc - mu c = o / rstd on grid columns, 0 on the others
    rows = np.arange(min(M, 1024))
    acc = X[rows] @ W.T
    t = acc - mu[rows, None] * cn[None, :]
    o = (j[rows] / 32.0)[:, None] * grid[None, :]
    assert np.array_equal(t * rstd[rows, None], o)
    assert np.all(np.abs(X[rows]) @ np.abs(W).T < 2.0 ** 10)       # multiples of 2^-7 below 2^10: exact in fp32
    pre = (np.arange(512) - 256)[:, None] / 32.0 * grid[None, :] + b32.astype(np.float64)[None, :]
    assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre)
    return dict(X=Xt, W=Wt, wexp=wexp_t, bias=torch.from_numpy(b32).to(d),
                colsum=torch.from_numpy(cn.astype(np.float32)).to(d),
                mr=torch.from_numpy(np.stack([mu, rstd], 1).astype(np.float32)).to(d), pre=pre)


def _run(f8, M, N, K, X, W, wexp, bias, colsum, mr):
    """sr_diag_ffn1 (diag 0) -> the outputs as fp64 values [M][N] and the raw bytes (fp8); the guard
    band after row M is checked here."""
    import torch
    from super_rag_amd import _native as NT
    d = _dev()
    if f8:
        Yall = torch.full((M + GUARD, N), 0x5A, device=d, dtype=torch.uint8)
    else:
        Yall = torch.full((M + GUARD, N), 1234.0, device=d, dtype=torch.float16)
    NT.call_diag("sr_diag_ffn1", 0, 1 if f8 else 0, X.data_ptr(), K, W.data_ptr(),
                 wexp.data_ptr() if f8 else None, bias.data_ptr(), colsum.data_ptr(), mr.data_ptr(),
                 Yall.data_ptr(), N, M, N, K, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((Yall[M:] == (0x5A if f8 else 1234.0)).all()), "rows past M were written"
    if not f8:
        return Yall[:M].double(), None
    raw = Yall[:M]
    assert not bool(((raw & 0x7F) == 0x7F).any()), "an e4m3 NaN code was stored"
    vals = torch.from_numpy(np.nan_to_num(FR.e4m3_values(np.arange(256, dtype=np.uint8)))).to(d)
    return vals[raw.long()], raw


@functools.lru_cache(maxsize=4)
def _bounds(key, form):
    """(lo, hi) of every distinct pre-activation; key: the bytes of the fp64 array and its shape."""
    pre = np.frombuffer(key[0], np.float64).reshape(key[1])
    rnd = FR.rnd_e4m3 if form == "e4m3" else FR.rnd_fp16
    return FR.bracket(FR.two_gelu(pre), FR.gelu_slack(pre, form), rnd)


def _check(f8, got, raw, pre, tag):
    """got [M][N] against the brackets of pre [P][N], row m <-> pre row m mod P."""
    import torch
    d = _dev()
    form = "e4m3" if f8 else "fp16"
    lo, hi = _bounds((pre.tobytes(), pre.shape), form)
    M = got.shape[0]
    idx = torch.arange(M, device=d) % pre.shape[0]
    lo_t, hi_t = torch.from_numpy(lo).to(d)[idx], torch.from_numpy(hi).to(d)[idx]
    bad = (got < lo_t) | (got > hi_t)
    if bool(bad.any()):
        i = bad.nonzero()[0].tolist()
        p = pre[i[0] % pre.shape[0], i[1]]
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} outputs outside their bracket; first at {i}: "
                             f"pre {p!r} got {float(got[i[0], i[1]])!r} not in [{float(lo_t[i[0], i[1]])!r}, "
                             f"{float(hi_t[i[0], i[1]])!r}]")
    print(f"{tag}: {bad.numel()} outputs inside their brackets; bracket ends equal on "
          f"{100.0 * float(np.mean(lo == hi)):.2f} % of the distinct pre-activations")
    if f8:
        pre_t = torch.from_numpy(pre).to(d)[idx]
        assert bool((raw[pre_t >= 224.0] == 0x7E).all()), "pre >= 224 must saturate to 448 (0x7E)"
        assert bool(((raw[pre_t <= -FR.XMAX] & 0x7F) == 0).all()), "pre <= -XMAX must give +-0"
        assert int((pre_t >= 224.0).sum()) > 0 and int((pre_t <= -FR.XMAX).sum()) > 0


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("f8", [False, True])
def test_ffn1_exact_grid(f8, second):
    """M = N = 512, K = 256 (fp8) / 128 (fp16): the one-tile-per-workgroup kernel."""
    M, N, K = 512, 512, 256 if f8 else 128
    c = _build(f8, M, N, K, second)
    pre = c.pop("pre")
    # the grid the issue asks for: [-8, 8] at 2^-12 (< h8 / 8), every out-of-range column
    pts = np.unique(pre)
    grid = pts[(pts >= -8.0) & (pts <= 8.0)]
    assert np.diff(grid).max() <= 2.0 ** -12 < FR.H8 / 8 and grid[0] == -8.0 and grid[-1] == 8.0
    assert set(np.float32(OUT_OF_RANGE).astype(np.float64)) <= set(pts)
    got, raw = _run(f8, M, N, K, **c)
    _check(f8, got, raw, pre, f"f8 {int(f8)} second {int(second)} {M}x{N}x{K}")


@pytest.mark.parametrize("f8", [False, True])
def test_ffn1_table_nodes_and_midpoints(f8):
    """Every node and midpoint of the 4,097-node table inside +-1 (the 1,025-node table's are
    among them), as the nearest fp32 value, with zero rows: pre = b."""
    import torch
    d = _dev()
    jj = np.arange(2 * 4096 + 1)
    sp = -FR.XMAX + jj * (FR.H8 / 2.0)
    sp = sp[np.abs(sp) <= 1.0]
    assert sp.size >= 1447 and np.any(np.abs(sp) < 1e-12)
    N = -(-sp.size // 256) * 256
    M, K = 16, 256 if f8 else 128
    b32 = np.zeros(N, np.float32)
    b32[:sp.size] = sp.astype(np.float32)
    X = torch.zeros(M, K, device=d, dtype=torch.uint8 if f8 else torch.float16)
    W = torch.zeros(N, K, device=d, dtype=torch.uint8 if f8 else torch.float16)
    wexp = torch.full((N,), 127, device=d, dtype=torch.uint8)
    mr = torch.tensor([[0.0, 1.0]] * M, device=d)
    got, raw = _run(f8, M, N, K, X, W, wexp, torch.from_numpy(b32).to(d), torch.zeros(N, device=d), mr)
    form = "e4m3" if f8 else "fp16"
    pre = b32.astype(np.float64)[None, :]
    lo, hi = FR.bracket(FR.two_gelu(pre), FR.gelu_slack(pre, form), FR.rnd_e4m3 if f8 else FR.rnd_fp16)
    g = got.cpu().numpy()
    assert np.all((g >= lo) & (g <= hi)), int(np.sum((g < lo) | (g > hi)))


@pytest.mark.parametrize("f8", [False, True])
def test_ffn1_persistent_grid(f8):
    """516 tiles (>= 512) and K / 2 >= 256 for fp8: the persistent kernel, whose bias / column sums /
    row statistics are staged in LDS per tile (stage_cst); the second launch's operands."""
    M, N, K = 128 * 256 + 77, 1024, 512 if f8 else 256
    c = _build(f8, M, N, K, True)
    pre = c.pop("pre")
    got, raw = _run(f8, M, N, K, **c)
    _check(f8, got, raw, pre, f"f8 {int(f8)} persistent {M}x{N}x{K}")


@pytest.mark.parametrize("f8", [False, True])
def test_ffn1_random_operands_per_element(f8):
    """The random-operand case of test_gpu_ffn1_epilogue.py at its smallest shape, per element: the
    bracket of two_gelu(pre) with gelu_slack plus the accumulation bound rstd K 2^-23 sum_k |x_k w_k|
    (fp64, from the operands) carried through 2 GELU's slope (<= 1.13 in magnitude)."""
    import torch
    M, N, K = 77, 1024, 768
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(M + N + int(f8))
    u = torch.randn(M, K, device=dev, generator=g) * 0.7 + 0.05
    Wf = torch.randn(N, K, device=dev, generator=g) * 0.04
    bias = torch.randn(N, device=dev, generator=g) * 0.1
    mr = torch.stack([u.mean(1), torch.rsqrt(u.var(1, unbiased=False) + 1e-5)], 1).contiguous()
    if f8:
        X8 = FR.e4m3_bytes(u.double().cpu().numpy())
        W8, wexp = FR.quantize_rows_ref(Wf.half().cpu().numpy())
        Xd, Wd = FR.e4m3_values(X8), FR.dequant_rows(W8, wexp)
        X, W, we = (torch.from_numpy(a).to(dev) for a in (X8, W8, wexp))
    else:
        X, W, we = u.half().contiguous(), Wf.half().contiguous(), None
        Xd, Wd = X.double().cpu().numpy(), W.double().cpu().numpy()
    colsum32 = Wd.sum(1).astype(np.float32)
    got, raw = _run(f8, M, N, K, X, W, we, bias, torch.from_numpy(colsum32).to(dev), mr)
    mu, rstd = (mr.double().cpu().numpy()[:, i:i + 1] for i in (0, 1))
    pre = rstd * (Xd @ Wd.T - mu * colsum32.astype(np.float64)[None, :]) + bias.double().cpu().numpy()[None, :]
    accb = rstd * K * 2.0 ** -23 * (np.abs(Xd) @ np.abs(Wd).T)
    form = "e4m3" if f8 else "fp16"
    slack = FR.gelu_slack(pre, form) + 1.13 * accb
    lo, hi = FR.bracket(FR.two_gelu(pre), slack, FR.rnd_e4m3 if f8 else FR.rnd_fp16)
    gv = got.cpu().numpy()
    bad = (gv < lo) | (gv > hi)
    print(f"f8 {int(f8)} random {M}x{N}x{K}: bracket ends equal on {100 * np.mean(lo == hi):.2f} % of the outputs, "
          f"max |pre| {np.abs(pre).max():.2f}")
    assert not bad.any(), (int(bad.sum()), pre[bad][:4], gv[bad][:4], lo[bad][:4], hi[bad][:4])
