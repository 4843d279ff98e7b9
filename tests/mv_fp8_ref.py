"""Reference restatement of the multi-vector index's fp8 storage mode (SR_DTYPE_FP8_E4M3), numpy:

quant(x32)        fp32 -> fp16 (round to nearest even) -> x 256 -> OCP e4m3fn (round to nearest even,
                  saturating at +-448) -> uint8: the byte the pool stores for a token element
dequant(codes)    fp64 value of the bytes, e4m3_value(c) / 256, by a 256-entry table built from the
                  format's definition (sign, 4 exponent bits with bias 7, 3 mantissa bits; exponent 0
                  is subnormal, steps of 2^-9; 0x7f and 0xff are NaN and never stored)
maxsim_rows8      colbert_ref.maxsim_rows on the dequantised tokens: the score contract
and the grid of values the storage tests run on.
"""
import numpy as np

import colbert_ref as CR

F = np.float32
NAN_CODES = (0x7F, 0xFF)
E4M3_MAX = 448.0


def _table():
    t = np.empty(256, np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        a = m * 2.0 ** -9 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -a if c & 0x80 else a
    t[list(NAN_CODES)] = np.nan
    return t


E4M3 = _table()                      # value of every code
FINITE_CODES = np.array([c for c in range(256) if c not in NAN_CODES], np.uint8)


def e4m3_rne(v):
    """fp64 values -> e4m3fn codes, round to nearest even on the code grid, saturating at +-448."""
    v = np.asarray(v, np.float64)
    sign = np.where(np.signbit(v), 0x80, 0).astype(np.int64)
    a = np.minimum(np.abs(v), E4M3_MAX)
    sub = a < 2.0 ** -6
    m_sub = np.rint(a * 512.0).astype(np.int64)                   # 0 .. 8 (8 is the smallest normal's code)
    _, ex = np.frexp(np.where(sub, 1.0, a))                       # a = f 2^ex, f in [0.5, 1)
    e = ex - 1
    m = np.rint((np.ldexp(np.where(sub, 1.0, a), -e) - 1.0) * 8.0).astype(np.int64)   # 0 .. 8 (8 carries)
    code = np.where(sub, m_sub, (e + 7) * 8 + m)
    return (sign | code).astype(np.uint8)


def quant(x32):
    h = np.asarray(x32, F).astype(np.float16)
    return e4m3_rne(h.astype(np.float64) * 256.0)


def quant_direct(x32):
    """Without the fp16 step: what a single rounding would store (the double-rounding test's foil)."""
    return e4m3_rne(np.asarray(x32, F).astype(np.float64) * 256.0)


def dequant(codes):
    return E4M3[np.asarray(codes, np.uint8)] / 256.0


def stored(x32):
    """The values sr_mv_get returns for tokens added as x32, fp32 (exact)."""
    return dequant(quant(x32)).astype(F)


def maxsim_rows8(q_list, docs, rows, live=None):
    """docs: the token arrays as they were added (fp32 / fp16 values)."""
    return CR.maxsim_rows(q_list, [dequant(quant(d)) for d in docs], rows, live)


def grid():
    """Token elements x (fp32; every one an fp16 value) whose 256 x covers: every finite code's value,
    every midpoint between adjacent codes (a tie: both parities of the lower code occur), points just
    to either side of the midpoints, the whole subnormal range |256 x| < 2^-6 on a 2^-12 lattice, +-0
    and +-1, and values past the saturation point 1.75."""
    pos = np.sort(E4M3[:0x7F])                                    # 0 .. 448, ascending
    mids = (pos[:-1] + pos[1:]) / 2.0
    near = np.concatenate([mids * (1 + 2.0 ** -9), mids * (1 - 2.0 ** -9)])
    subn = np.arange(0, 2 ** 6 + 1) * 2.0 ** -12
    past = np.array([449.0, 464.0, 480.0, 512.0, 1000.0, 65504.0 * 256.0])       # x up to the fp16 maximum
    v = np.concatenate([pos, mids, near, subn, [256.0], past]) / 256.0
    v = np.concatenate([v, -v, [0.0, -0.0, 1.0, -1.0]])
    x = v.astype(np.float16).astype(F)
    return x


def grid_tokens(dim):
    """grid() laid out as tokens [n, dim], the tail filled with zeros."""
    g = grid()
    n = -(-g.size // dim)
    out = np.zeros(n * dim, F)
    out[:g.size] = g
    return out.reshape(n, dim)
