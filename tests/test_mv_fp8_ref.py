"""CPU: the fp8 multi-vector reference (tests/mv_fp8_ref.py) against the format's definition and
torch.float8_e4m3fn, the norm bound of the quantisation error, the pinned double rounding of the host
add path, and what of the feature needs no GPU: the constructor's dtype check and the exported symbols.

Norm bound, derived: a normal e4m3 value has a 3-bit mantissa, so round to nearest moves 256 x by at
most half an ulp, 2^-4 relative; below 2^-6 the codes are 2^-9 apart, so the error is at most 2^-10,
that is 2^-18 in x.  Per element |d^ - d| <= max(2^-4 |d|, 2^-18), hence
||d^ - d|| <= 2^-4 ||d|| + sqrt(dim) 2^-18 for every token without a saturating element.
"""
import numpy as np
import pytest

import colbert_ref as CR
import mv_fp8_ref as Q

F = np.float32


def test_every_code_round_trips_and_the_table_is_the_format():
    torch = pytest.importorskip("torch")
    assert Q.NAN_CODES == (0x7F, 0xFF) and np.isnan(Q.E4M3[list(Q.NAN_CODES)]).all()
    codes = Q.FINITE_CODES
    assert codes.size == 254
    back = Q.quant(Q.dequant(codes).astype(F))
    keep = codes != 0x80                                             # -0 comes back as -0 too, by its sign bit
    np.testing.assert_array_equal(back[keep], codes[keep])
    assert back[codes == 0x80][0] == 0x80
    # landmarks of the definition
    assert Q.E4M3[0x01] == 2.0 ** -9 and Q.E4M3[0x08] == 2.0 ** -6 and Q.E4M3[0x38] == 1.0
    assert Q.E4M3[0x7E] == 448.0 and Q.E4M3[0xFE] == -448.0
    t = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    np.testing.assert_array_equal(t[codes], Q.E4M3[codes])
    assert np.isnan(t[list(Q.NAN_CODES)]).all()
    # dequantised values are exact in fp32
    np.testing.assert_array_equal(Q.dequant(codes).astype(F).astype(np.float64), Q.dequant(codes))


def test_quant_agrees_with_torch_on_ties_subnormals_and_saturates_past_448():
    torch = pytest.importorskip("torch")
    x = Q.grid()
    np.testing.assert_array_equal(x, x.astype(np.float16).astype(F))          # the grid holds fp16 values
    y = x.astype(np.float64) * 256.0
    pos = np.sort(Q.E4M3[:0x7F])
    mids = (pos[:-1] + pos[1:]) / 2.0
    assert np.isin(mids, y).all() and np.isin(-mids, y).all()                 # every tie is on the grid
    assert np.isin(np.arange(65) * 2.0 ** -12, y).all()                       # the subnormal range
    for v in (0.0, 1.0):
        assert (x == v).any() and ((x == -v) & np.signbit(x)).any()
    got = Q.quant(x)
    inside = np.abs(y) <= Q.E4M3_MAX
    want = torch.tensor(y[inside], dtype=torch.float32).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    np.testing.assert_array_equal(got[inside], want)
    # ties went to the even code, and both parities of the lower neighbour occurred
    tie = Q.quant((mids / 256.0).astype(F))
    assert (tie % 2 == 0).all()
    lower = Q.e4m3_rne(pos[:-1])
    np.testing.assert_array_equal(tie, np.where(lower % 2 == 0, lower, lower + 1))
    assert (lower % 2 == 0).any() and (lower % 2 == 1).any()
    # past 448 (|x| > 1.75): the largest finite code of the sign, never a NaN code
    assert (~inside).sum() >= 12
    np.testing.assert_array_equal(got[~inside], np.where(y[~inside] > 0, 0x7E, 0xFE))
    assert not np.isin(got, Q.NAN_CODES).any()
    np.testing.assert_array_equal(Q.stored(np.array([2.0, -3.0, 1.75], F)), np.array([1.75, -1.75, 1.75], F))


@pytest.mark.parametrize("dim", [64, 128, 1024])
def test_norm_bound_of_the_quantisation_error(dim):
    rng = np.random.default_rng(dim)
    toks = [CR.unit_f16(rng, 64, dim)]
    for ld in (1, 17, 65):
        toks += list(CR.all_negative_case(rng, 5, ld, dim))
    toks += list(CR.tail_argmax_case(rng, 33, 65, dim))
    toks += list(CR.first_last_case(rng, 4, 40, dim))
    sparse = np.zeros((3, dim), F)                                            # nearly all of the norm in one element
    sparse[0, 0], sparse[1, 5], sparse[2, dim - 1] = 1.0, -0.999, 0.9
    sparse[:, 1] = 2.0 ** -17
    toks.append(sparse)
    worst = 0.0
    for d in toks:
        d64 = np.asarray(d, np.float64)
        err = np.linalg.norm(Q.dequant(Q.quant(d)) - d64, axis=1)
        bound = 2.0 ** -4 * np.linalg.norm(d64, axis=1) + np.sqrt(dim) * 2.0 ** -18
        assert (err <= bound).all(), (dim, (err / bound).max())
        worst = max(worst, float((err / bound).max()))
    print(f"fp8 norm bound dim {dim}: max err / bound {worst:.3f}")


def test_double_rounding_is_pinned():
    """sr_mv_add on an fp8 index rounds fp32 -> fp16 -> e4m3: there are fp32 values whose direct e4m3
    rounding differs.  Search just above every tie: fp16 pulls the value onto the tie, which then goes
    to the even code, where the direct rounding goes up."""
    pos = np.sort(Q.E4M3[:0x7F])
    mids = (pos[:-1] + pos[1:]) / 2.0
    x = (mids / 256.0 * (1.0 + 2.0 ** -20)).astype(F)
    two, one = Q.quant(x), Q.quant_direct(x)
    found = np.nonzero(two != one)[0]
    assert found.size > 0
    i = int(found[0])
    assert x[i] > mids[i] / 256.0 and float(np.float16(x[i])) == mids[i] / 256.0
    assert one[i] == two[i] + 1 and two[i] % 2 == 0
    # the pinned case: 256 x just above 1.0625, the tie between the codes of 1 and 1.125
    xp = np.array([1.0625 / 256.0 * (1.0 + 2.0 ** -20)], F)
    assert Q.quant(xp)[0] == 0x38 and Q.quant_direct(xp)[0] == 0x39
    assert Q.stored(xp)[0] == F(1.0 / 256.0)


def test_maxsim_rows8_is_maxsim_rows_on_the_dequantised_tokens():
    rng = np.random.default_rng(3)
    docs = [CR.unit_f16(rng, n, 64) for n in (3, 0, 20)]
    q = [CR.unit_f16(rng, 5, 64)]
    rows = np.array([[0, 1, 2, -1, 3]], np.int64)
    got = Q.maxsim_rows8(q, docs, rows, live=np.array([True, True, True]))
    assert np.isneginf(got[0, [1, 3, 4]]).all()
    for k in (0, 2):
        assert got[0, k] == CR.maxsim(q[0], Q.stored(docs[k]).astype(np.float64))
        assert got[0, k] != CR.maxsim(q[0], docs[k])


def test_constructor_rejects_an_unknown_dtype_without_a_gpu():
    from super_rag_amd import multivec
    assert set(multivec.MV_DTYPES) == {"fp16", "fp8"}
    for bad in ("int8", "FP8", None, 2):
        with pytest.raises(ValueError, match="dtype"):
            multivec.NativeMultiVectorIndex(64, dtype=bad)


def test_new_symbols_are_declared_exported_and_bound():
    import shutil
    import subprocess
    from super_rag_amd import _native
    names = {"sr_mv_create_dtype", "sr_mv_info"}
    assert names <= set(_native.SIGNATURES)
    lib = _native.load()
    assert all(hasattr(lib, n) for n in names)
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for path in (_native.library_path(), _native.diag_library_path()):
        out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert names <= {l.split()[-1] for l in out.splitlines()}
    # a bad dtype is refused before any device work (no GPU needed to see it)
    import ctypes
    h = ctypes.c_void_p()
    for bad in (_native.SR_DTYPE_F32, 3, -1):
        assert lib.sr_mv_create_dtype(64, 0, bad, ctypes.byref(h)) == _native.SR_ERR_INVALID
        assert b"dtype" in lib.sr_last_error()
