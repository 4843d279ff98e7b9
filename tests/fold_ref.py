"""fp64 / exact-integer references for the LayerNorm-fold kernels and the fp8 FFN GEMMs (numpy):

e4m3_values / e4m3_bytes   OCP e4m3fn, exact round-to-nearest-even with saturation at +-448
quantize_rows_ref          launch_quantize_rows_fp8: per-row power-of-two scale + e4m3 bytes
two_gelu                   x erfc(-x / sqrt 2) = 2 GELU(x), fp64
gelu_slack                 the error the FFN1 epilogues' erfc tables are allowed, from their construction
bracket                    (rnd(y - d), rnd(y + d)): rounding is monotone, a correct output lies between
dyadic_gemm_case           GEMM operands whose every intermediate is exact in fp32 in any order

Error model of the tables (k_gemm.hip gelu_t_tab_init / gelu_t8_tab_init).  2 GELU(x) = x T(x),
T(x) = erfc(-x / sqrt 2), T'(x) = sqrt(2 / pi) exp(-x^2 / 2), |T''(x)| = |x| T'(x).  The tables hold
T at nodes -XMAX + i h over [-XMAX, XMAX], XMAX = 4 sqrt 2:
  * e4m3 form: 4,097 nodes (h8 = 2 XMAX / 4096), the NEAREST node's value.  The node is at most
    h8 / 2 from x (h8 when the fp32 index arithmetic lands on the other side of a midpoint, which
    the interval below covers), so |dT| <= (h8 / 2) max T' over [x - h8, x + h8].
  * fp16 form: 1,025 nodes (h16 = 2 XMAX / 1024), linear interpolation: |dT| <= (h16^2 / 8)
    max |T''| over [x - h16, x + h16] (the classical bound; the interval covers an fp32 index that
    falls into the neighbouring cell).
  * outside [-XMAX, XMAX] both forms take the end node: |dT| = |T(x) - T(+-XMAX)|, plus what the
    end node itself is off by: XMAX is an fp32 constant in the kernel (T'(XMAX) XMAX 2^-24) and the
    entry is rounded to fp32 (2^-24 T(+-XMAX)).  Left of -XMAX, T(x) falls far below T(-XMAX) =
    1.5e-8, so the relative terms below do not cover these two (an fp32 emulation exceeds the bound
    without them by ~1e-14 just outside -XMAX, tests/test_fold_ref.py).
The output error is |x| |dT|; on top a relative 2^-20 of that term (fp32 rounding of the table
entries and of the interpolation) and 2^-21 |2 GELU(x)| (the handful of fp32 roundings of the
product).  Nothing here is fitted to a run of the kernels.
"""
import math

import numpy as np

XMAX = 4.0 * math.sqrt(2.0)
H16 = 2.0 * XMAX / 1024.0
H8 = 2.0 * XMAX / 4096.0
NAN_CODES = (0x7F, 0xFF)


def _e4m3_table():
    t = np.empty(256, np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        a = math.ldexp(m, -9) if e == 0 else math.ldexp(8 + m, e - 10)
        t[c] = -a if c & 0x80 else a
    t[list(NAN_CODES)] = np.nan
    return t


_E4M3 = _e4m3_table()
_POS = _E4M3[:0x7F].copy()                       # codes 0x00 .. 0x7E: 0 .. 448, ascending
_MID = (_POS[:-1] + _POS[1:]) / 2.0              # exact in fp64


def e4m3_values(codes):
    """fp64 value of every e4m3fn byte (NaN for 0x7F / 0xFF)."""
    return _E4M3[np.asarray(codes, np.uint8)]


def e4m3_bytes(x):
    """fp64 values -> e4m3fn bytes: round to nearest, ties to the even code, saturating at +-448
    (by searching the code table: no floating-point arithmetic on x besides comparisons)."""
    x = np.asarray(x, np.float64)
    assert not np.isnan(x).any()
    a = np.minimum(np.abs(x), 448.0)
    lo = np.searchsorted(_POS, a, side="right") - 1          # largest code with value <= a
    hi = np.minimum(lo + 1, 0x7E)
    mid = np.where(hi > lo, _MID[np.minimum(lo, 0x7D)], np.inf)
    up = (a > mid) | ((a == mid) & (lo % 2 == 1))
    code = np.where(up, hi, lo)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def fp16_rne(x):
    """fp64 -> fp16 (numpy converts with one rounding, to nearest even)."""
    return np.asarray(x, np.float64).astype(np.float16)


def quantize_rows_ref(W16):
    """W16 [N][K] fp16 -> (bytes [N][K] uint8, wexp [N] uint8): e the largest integer with
    amax 2^e <= 448 (0 for a zero row), clamped to +-127, wexp = 127 - e, bytes = e4m3(w 2^e).
    amax = f 2^x with f in [0.5, 1) (math.frexp, exact): amax 2^e <= 448 = 0.875 2^9 <=> e <= 9 - x
    when f <= 0.875, e <= 8 - x otherwise."""
    W = np.asarray(W16, np.float16)
    assert W.ndim == 2
    Wd = W.astype(np.float64)
    es = np.zeros(W.shape[0], np.int64)
    for n in range(W.shape[0]):
        amax = float(np.abs(Wd[n]).max())
        if amax > 0.0:
            f, x = math.frexp(amax)
            es[n] = (9 - x) if f <= 0.875 else (8 - x)
    es = np.clip(es, -127, 127)
    scaled = np.ldexp(Wd, es[:, None].astype(np.int32))      # exact: a power-of-two scale
    return e4m3_bytes(scaled), (127 - es).astype(np.uint8)


def quantize_case_rows(K):
    """Rows (fp16) whose maxima sit on the edges of the exponent choice: 1.75 2^j (amax 2^e = 448
    exactly), the next fp16 above (e drops by one), the fp16 subnormal minimum, 65504, zero; negative
    maxima; the maximum at k = 0, K - 1 and 63."""
    rng = np.random.default_rng(K)
    amax = []
    for j in (-14, -9, -3, 0, 1, 7, 14):
        a = np.float16(1.75 * 2.0 ** j)
        amax += [a, np.nextafter(a, np.float16(np.inf))]
    amax += [np.float16(2.0 ** -24), np.float16(65504.0), np.float16(0.0), np.float16(0.3), np.float16(448.0)]
    rows = []
    for i, a in enumerate(amax):
        for kmax in (0, K - 1, 63):
            sign = -1.0 if (i + kmax) % 2 else 1.0
            r = (rng.uniform(-1, 1, K) * float(a)).astype(np.float16)
            r[np.abs(r) > a] = a
            r[kmax] = np.float16(sign * float(a))
            rows.append(r)
    return np.stack(rows)


def dequant_rows(bytes_, wexp):
    """fp64 value of e4m3 weight rows with E8M0 row exponents: W8 2^(wexp - 127)."""
    return np.ldexp(e4m3_values(bytes_), (np.asarray(wexp, np.int32) - 127)[:, None])


def _erfc(x):
    from scipy.special import erfc
    return erfc(x)


def T(x):
    return _erfc(-np.asarray(x, np.float64) / math.sqrt(2.0))


def two_gelu(x):
    x = np.asarray(x, np.float64)
    return x * T(x)


def _tp(x):
    return math.sqrt(2.0 / math.pi) * np.exp(-0.5 * np.square(x))


def gelu_slack(x, form):
    """Allowed |got - two_gelu(x)| of the FFN1 epilogue before its output rounding; form 'e4m3'
    (nearest node) or 'fp16' (interpolated).  See the module docstring."""
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    if form == "e4m3":
        near = np.maximum(ax - H8, 0.0)                      # T' is largest nearest to 0
        dT = (H8 / 2.0) * _tp(near)
    elif form == "fp16":
        lo, hi = np.maximum(ax - H16, 0.0), ax + H16         # |T''| = t T'(t) peaks at t = 1
        t = np.where(hi < 1.0, hi, np.where(lo > 1.0, lo, 1.0))
        dT = (H16 * H16 / 8.0) * t * _tp(t)
    else:
        raise ValueError(form)
    end = T(np.copysign(XMAX, x))
    out = np.abs(T(x) - end) + float(_tp(XMAX)) * XMAX * 2.0 ** -24 + 2.0 ** -24 * end
    dT = np.where(ax > XMAX, out, dT)
    return ax * dT * (1.0 + 2.0 ** -20) + 2.0 ** -21 * np.abs(two_gelu(x))


def rnd_e4m3(v):
    return e4m3_values(e4m3_bytes(v))


def rnd_fp16(v):
    return fp16_rne(v).astype(np.float64)


def bracket(y, d, rnd):
    y, d = np.asarray(y, np.float64), np.asarray(d, np.float64)
    return rnd(y - d), rnd(y + d)


# ---- dyadic GEMM operands ------------------------------------------------------------------------
WEXP_CYCLE = np.array([127, 95, 126, 135, 120, 125, 131, 110, 124, 128, 103, 123, 133, 122, 121, 129],
                      np.int64)                              # position 0 carries the zero row
IX_MAX, IW_DENSE, IW_SPARSE, NNZ_SPARSE = 8, 8, 1, 2


def _assert_exact(abs_sum, q, what):
    """Every term a multiple of q (by construction) and the sum of magnitudes below 2^24 q: every
    partial sum of any evaluation order is an integer multiple of q below 2^24 q, exact in fp32."""
    assert np.all(abs_sum < 2.0 ** 24 * q), what


def dyadic_gemm_case(N, K, rows, seed, f8=True, device="cpu"):
    """Operands of Y = epi(X W^T ...) for which every fp32 evaluation order is exact (torch tensors
    on `device`; the matrices are drawn there, the reference of a large case runs there in fp64).

    Column n has a scale s_n = 2^(wexp_n - 127) (f8: the E8M0 row exponent over integer e4m3 bytes,
    WEXP_CYCLE = 95 .. 135; fp16: folded into the fp16 weight, wexp_n in 119 .. 127) and a quantum
    q_n = 2^-10 s_n:
      X[m][k] = ix 2^-6, |ix| <= 8;  W[n][k] = iw s_n, |iw| <= 8 (dense rows, s_n <= 1/2) or two
      entries of +-1 (s_n >= 1: keeps the outputs small, so the fp32 span statistics stay well
      conditioned and fp16 does not overflow); one zero row per 16, with wexp 127;
      products: multiples of 2^-6 s_n (the magnitude conditions are asserted below);
      bias = ib 2^-6 s_n, |ib| <= 16;  colsum = ic s_n, |ic| <= 16;  gamma = ig 2^-8 s_n, ig odd,
      |ig| <= 3;  mu_m = im 2^-6 (LNF) / an integer up to 800 (LNR);  rstd_m in {1/4, 1/2, 1, 2};
      R_lnr[m][n] = mu_m + d, |d| <= 8 (fp16 integers: |mean| / std up to ~170);
      R_res[m][n] = d 2^-6 s_n where fp16 holds that exactly (s_n >= 2^-18), else 0.
    rows: operand / statistics rows to generate (strided cases read every 7th of them)."""
    import torch
    rng = np.random.default_rng(seed)
    wexp = WEXP_CYCLE[np.arange(N) % len(WEXP_CYCLE)].copy()
    if not f8:
        wexp = 127 - ((127 - wexp) % 9)                      # 119 .. 127: fp16 holds iw 2^-8 .. iw
    zero_row = np.arange(N) % len(WEXP_CYCLE) == 0
    assert np.all(wexp[zero_row] == 127)
    s = np.ldexp(1.0, (wexp - 127).astype(np.int32))
    iw = rng.integers(-IW_DENSE, IW_DENSE + 1, (N, K))
    for n in np.nonzero(s >= 1.0)[0]:
        row = np.zeros(K, np.int64)
        row[rng.choice(K, NNZ_SPARSE, replace=False)] = rng.choice([-IW_SPARSE, IW_SPARSE], NNZ_SPARSE)
        iw[n] = row
    iw[zero_row] = 0
    ib, ic = rng.integers(-16, 17, N), rng.integers(-16, 17, N)
    ig = rng.choice([-3, -1, 1, 3], N)
    bias, colsum, gamma = ib * 2.0 ** -6 * s, ic * s, ig * 2.0 ** -8 * s
    rstd = rng.choice([0.25, 0.5, 1.0, 2.0], rows)
    mu_lnf = rng.integers(-16, 17, rows) * 2.0 ** -6
    mu_lnr = rng.choice([0.0, 3.0, -40.0, 500.0, -800.0], rows)
    q = s * 2.0 ** -10
    # the magnitude conditions, per output column, with every row-dependent factor at its maximum
    prod = IX_MAX * 2.0 ** -6 * np.abs(iw).sum(1) * s        # >= sum_k |x_k w_k| of any row
    res_ok = s * 2.0 ** -6 >= 2.0 ** -24
    lnf = 2.0 * (prod + 16 * 2.0 ** -6 * np.abs(colsum)) + np.abs(bias)
    lnr = prod + np.abs(bias) + 2.0 * (808.0 + 800.0) * np.abs(gamma)
    res = prod + np.abs(bias) + 8 * 2.0 ** -6 * s
    _assert_exact(np.maximum(np.maximum(lnf, lnr), res), q, "dyadic_gemm_case: sums must stay below 2^24 quanta")
    for a in (bias / q, colsum / q, gamma / q):
        assert np.all(a == np.rint(a))
    g = torch.Generator(device=device).manual_seed(seed)
    dev = torch.device(device)
    ixt = torch.randint(-IX_MAX, IX_MAX + 1, (rows, K), device=dev, generator=g, dtype=torch.int16)
    dt = torch.randint(-8, 9, (rows, N), device=dev, generator=g, dtype=torch.int16)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    out = dict(N=N, K=K, rows=rows, f8=f8, wexp=torch.from_numpy(wexp.astype(np.uint8)).to(dev),
               bias=t32(bias), colsum=t32(colsum), gamma=t32(gamma), q=t64(q),
               mr_lnf=t32(np.stack([mu_lnf, rstd], 1)), mr_lnr=t32(np.stack([mu_lnr, rstd], 1)))
    for k, v in (("bias", bias), ("colsum", colsum), ("gamma", gamma)):
        assert np.all(out[k].double().cpu().numpy() == v)    # fp32 holds them exactly
    R_lnr = (t64(mu_lnr)[:, None] + dt.double()).half()
    R_res = (dt.double() * t64(np.where(res_ok, 2.0 ** -6 * s, 0.0))[None, :]).half()
    assert bool((R_lnr.double() == t64(mu_lnr)[:, None] + dt.double()).all())
    out["R_lnr"], out["R_res"] = R_lnr, R_res
    if f8:
        lut = torch.from_numpy(e4m3_bytes(np.arange(-8, 9, dtype=np.float64))).to(dev)      # integers
        lutx = torch.from_numpy(e4m3_bytes(np.arange(-8, 9, dtype=np.float64) * 2.0 ** -6)).to(dev)
        assert np.all(e4m3_values(lutx.cpu().numpy()) == np.arange(-8, 9) * 2.0 ** -6)
        assert np.all(e4m3_values(lut.cpu().numpy()) == np.arange(-8, 9))
        out["X"] = lutx[(ixt + 8).long()].contiguous()
        out["W"] = lut[torch.from_numpy(iw + 8).to(dev)].contiguous()
    else:
        out["X"] = (ixt.double() * 2.0 ** -6).half().contiguous()
        out["W"] = t64(iw * s[:, None]).half().contiguous()
        assert bool((out["W"].double() == t64(iw * s[:, None])).all())
    out["Xd"] = lambda sl=slice(None): ixt[sl].double() * 2.0 ** -6      # dequantised, fp64
    out["Wd"] = t64(iw * s[:, None])
    return out


def fold_ref_t(epi, Xd, Wd, bias, colsum=None, R=None, mr=None, gamma=None):
    """fp64 value of the folded epilogues on dequantised operands (torch; epi 'lnf', 'res', 'lnr')."""
    acc = Xd.double() @ Wd.double().T
    b = bias.double()[None, :]
    if epi == "res":
        return acc + b + R.double()
    mu, rstd = mr.double()[:, 0:1], mr.double()[:, 1:2]
    if epi == "lnf":
        return rstd * (acc - mu * colsum.double()[None, :]) + b
    if epi == "lnr":
        return acc + b + ((R.double() - mu) * rstd) * gamma.double()[None, :]
    raise ValueError(epi)


def fp16_to_e4m3_lut():
    """e4m3_bytes of every finite fp16 bit pattern (index: the pattern as uint16; NaN patterns 0)."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    v = bits.view(np.float16).astype(np.float64)
    nan = np.isnan(v)
    return np.where(nan, 0, e4m3_bytes(np.where(nan, 0.0, v))).astype(np.uint8)
