"""CPU (ctypes, no GPU): sr_lex_load validates an impact snapshot ("SRMILEX2") before anything is
allocated on a device, and sr_sparse_terms_dev its arguments before any device call.

The files are written by hand from the documented layout (k_lex.hip, LexIndex::save): magic [8],
float k1, float b, int64 rows, int64 P, rows x int32 dl, rows x u8 live, P x int32 term,
P x u64 (row << 32 | fp32 bits of the weight)."""
import ctypes
import struct

import numpy as np
import pytest


def _lib():
    from super_rag_amd import _native
    return _native, _native.load()


def _snapshot(rows_of_postings, weights, magic=b"SRMILEX2", n_rows=3, size_rows=None, size_p=None):
    """rows_of_postings: the row of every posting; weights: its fp32 weight (or raw uint32 bits)."""
    P = len(rows_of_postings)
    bits = [w if isinstance(w, int) else struct.unpack("<I", struct.pack("<f", w))[0] for w in weights]
    fv = np.asarray([(r << 32) | b for r, b in zip(rows_of_postings, bits)], np.uint64)
    head = magic + struct.pack("<ffqq", 0.0, 0.0, n_rows if size_rows is None else size_rows,
                               P if size_p is None else size_p)
    dl = np.bincount(np.asarray(rows_of_postings, np.int64), minlength=n_rows).astype(np.int32)
    return (head + dl.tobytes() + np.ones(n_rows, np.uint8).tobytes()
            + np.arange(P, dtype=np.int32).tobytes() + fv.tobytes())


def _load(path):
    N, lib = _lib()
    h = ctypes.c_void_p()
    rc = lib.sr_lex_load(str(path).encode(), 0, ctypes.byref(h))
    if rc == N.SR_OK:
        mode = ctypes.c_int32(-1)
        assert lib.sr_lex_scoring(h, ctypes.byref(mode)) == N.SR_OK
        lib.sr_lex_destroy(h)
        return rc, mode.value
    assert not h.value
    return rc, None


GOOD = ([0, 0, 1, 2], [0.5, 16.0, 1e-6, 2.0])


def test_a_well_formed_impact_snapshot_passes_validation(tmp_path):
    """The control of the cases below: the same bytes, uncorrupted, get past the loader's checks (to
    the device allocation, which fails with SR_ERR_HIP where there is no GPU)."""
    N, _ = _lib()
    p = tmp_path / "good.bin"
    p.write_bytes(_snapshot(*GOOD))
    rc, mode = _load(p)
    assert rc in (N.SR_OK, N.SR_ERR_HIP), rc
    if rc == N.SR_OK:
        assert mode == N.SR_LEX_IMPACT


CORRUPT = {
    "truncated": lambda: _snapshot(*GOOD)[:-5],
    "truncated header": lambda: _snapshot(*GOOD)[:20],
    "trailing bytes": lambda: _snapshot(*GOOD) + b"\0" * 12,
    "rows field too large": lambda: _snapshot(*GOOD, size_rows=4),
    "postings field too small": lambda: _snapshot(*GOOD, size_p=3),
    "negative rows field": lambda: _snapshot(*GOOD, size_rows=-1),
    "weight 0": lambda: _snapshot([0, 0, 1, 2], [0.5, 0.0, 1.0, 2.0]),
    "weight -0": lambda: _snapshot([0, 0, 1, 2], [0.5, -0.0, 1.0, 2.0]),
    "negative weight": lambda: _snapshot([0, 0, 1, 2], [0.5, -1.0, 1.0, 2.0]),
    "NaN weight": lambda: _snapshot([0, 0, 1, 2], [0.5, float("nan"), 1.0, 2.0]),
    "infinite weight": lambda: _snapshot([0, 0, 1, 2], [0.5, float("inf"), 1.0, 2.0]),
    "weight above 16": lambda: _snapshot([0, 0, 1, 2], [0.5, float(np.nextafter(np.float32(16), np.float32(17))), 1.0, 2.0]),
    "postings out of row order": lambda: _snapshot([0, 2, 1, 2], [0.5, 1.0, 1.0, 2.0]),
    "posting of a row past the index": lambda: _snapshot([0, 0, 1, 3], [0.5, 1.0, 1.0, 2.0]),
    "unknown magic": lambda: _snapshot(*GOOD, magic=b"SRMILEX3"),
}


@pytest.mark.parametrize("what", sorted(CORRUPT))
def test_corrupt_impact_snapshot_is_an_io_error(what, tmp_path):
    N, lib = _lib()
    p = tmp_path / "bad.bin"
    p.write_bytes(CORRUPT[what]())
    rc, _ = _load(p)
    assert rc == N.SR_ERR_IO, (what, rc)
    assert b"lex.load" in lib.sr_last_error()


def test_the_two_magics_never_read_as_each_other(tmp_path):
    """The fp32 bits of a positive weight are a valid tf, so only the magic tells the two apart: tf
    values (1, 2, 3: denormal bit patterns) under "SRMILEX2" are valid tiny weights, and weight
    bits under "SRMILEX1" are valid tf, each restored in the mode its magic names."""
    N, _ = _lib()
    p = tmp_path / "x.bin"
    p.write_bytes(_snapshot([0, 1, 2], [1, 2, 3], magic=b"SRMILEX1"))
    rc, mode = _load(p)
    assert rc in (N.SR_OK, N.SR_ERR_HIP) and mode in (None, N.SR_LEX_BM25)
    # a BM25 snapshot whose tf has the sign bit is rejected as before; the same bits as a weight too
    for magic in (b"SRMILEX1", b"SRMILEX2"):
        p.write_bytes(_snapshot([0, 1, 2], [1, 0x80000001, 3], magic=magic))
        assert _load(p)[0] == N.SR_ERR_IO


def test_sparse_terms_rejects_bad_arguments_before_any_device_call():
    N, lib = _lib()
    buf = (ctypes.c_int32 * 64)()
    fbuf = (ctypes.c_float * 64)()
    p, fp = ctypes.addressof(buf), ctypes.addressof(fbuf)

    def call(ids=p, mask=p, tw=fp, B=2, S=8, special=p, n_special=2, terms=p, weights=fp, count=p):
        return lib.sr_sparse_terms_dev(ids, mask, tw, B, S, special, n_special, terms, weights, count, 0, None)

    for kw in (dict(n_special=17), dict(n_special=-1), dict(S=0), dict(S=8193), dict(B=-1),
               dict(ids=None), dict(mask=None), dict(tw=None), dict(terms=None), dict(weights=None),
               dict(count=None), dict(special=None)):
        assert call(**kw) == N.SR_ERR_INVALID, kw
        assert lib.sr_last_error()
    assert call(B=0) == N.SR_OK                                      # a no-op, no device needed
    assert call(B=0, ids=None, n_special=0, special=None) == N.SR_OK
