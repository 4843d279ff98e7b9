"""CPU: the reference of the multi-vector index's whole-corpus search (tests/mv_search_ref.py) against
plain loops and hand-made scores, the new entry points in header, bindings and both libraries, and the
rejections that need no device.  The GPU tests (test_gpu_mv_search.py) compare the device against
sr_mv_score_rows bit for bit and against this reference under the MaxSim gate."""
import ctypes
import os
import re

import numpy as np
import pytest

import colbert_ref as CR
import mv_search_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sr_mv_search": 10, "sr_mv_search_dev": 12, "sr_mv_search_group": 2}


# -- the reference -----------------------------------------------------------------------------------------
def _case(seed, dim=16):
    rng = np.random.default_rng(seed)
    lens = [3, 0, 5, 1, 7, 2, 0, 4, 6, 1, 3]
    docs = [CR.unit_f16(rng, n, dim) for n in lens]
    qs = [CR.unit_f16(rng, n, dim) for n in (4, 1, 0, 9)]
    return qs, docs


@pytest.mark.parametrize("k", [1, 3, 9, 20])
def test_reference_matches_a_plain_loop(k):
    qs, docs = _case(k)
    n = len(docs)
    live = np.ones(n, bool)
    live[[2, 9]] = False
    allow = np.arange(n) % 3 != 1
    for lv, al in ((None, None), (live, None), (None, allow), (live, allow)):
        s, r = R.search(qs, docs, k, lv, al, row_offset=100)
        ls, lr = R.search_loop(qs, docs, k, lv, al, row_offset=100)
        np.testing.assert_array_equal(r, lr)
        np.testing.assert_allclose(s, ls, rtol=0, atol=1e-12)
        ok = R.eligible(docs, lv, al)
        for b in range(len(qs)):
            real = r[b][r[b] >= 0] - 100
            assert ok[real].all() and len(set(real.tolist())) == real.size
            assert real.size == (min(k, int(ok.sum())) if len(qs[b]) else 0)
            assert np.isneginf(s[b, real.size:]).all() and (r[b, real.size:] == -1).all()
            assert (np.diff(s[b, :real.size]) <= 0).all()


def test_padding_ties_and_empty_query_on_hand_made_scores():
    ninf = -np.inf
    score = np.array([[0.5, ninf, 0.75, 0.5, 0.25, 0.5, ninf],
                      [ninf] * 7,                                  # an empty query: every row -inf
                      [0.0, -0.0, -1.0, ninf, 0.0, 2.0, -1.0]], np.float32)
    s, r = R.topk(score, 4)
    assert r.tolist() == [[2, 0, 3, 5], [-1] * 4, [5, 0, 1, 4]]    # ties to the lower row; -0.0 == 0.0
    assert s[0].tolist() == [0.75, 0.5, 0.5, 0.5] and np.isneginf(s[1]).all()
    # a k that cuts between the three equal rows keeps the lower ones
    assert R.topk(score, 3)[1][0].tolist() == [2, 0, 3]
    assert R.topk(score, 2)[1][0].tolist() == [2, 0]
    # more slots than eligible rows: -inf / -1 past them, and a -inf row is never reported
    s, r = R.topk(score, 9, row_offset=10)
    assert r[0].tolist() == [12, 10, 13, 15, 14, -1, -1, -1, -1]
    assert np.isneginf(s[0, 5:]).all() and s.dtype == np.float32
    assert r[2].tolist() == [15, 10, 11, 14, 12, 16, -1, -1, -1]
    assert (r[1] == -1).all()
    # no rows at all
    s, r = R.topk(np.zeros((2, 0), np.float32), 3)
    assert np.isneginf(s).all() and (r == -1).all()


# -- the library and the Python surface --------------------------------------------------------------------
def _header_arity():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "super_rag_mi355x.h")).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(sr_mv_search\w*)\s*\(([^)]*)\)\s*;", src):
        out[name] = len([a for a in args.split(",") if a.strip()])
    return out


def test_new_symbols_in_header_bindings_and_both_libraries():
    from super_rag_amd import _native
    assert _header_arity() == NEW
    for name, arity in NEW.items():
        res, args = _native.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == arity, name
        assert name not in _native.DIAG_SIGNATURES
        assert hasattr(_native.load(), name), name
        assert hasattr(_native.load_diag(), name), name


def test_null_handle_and_bad_dim_are_invalid_without_a_device():
    from super_rag_amd import _native
    lib = _native.load()
    f, i, r = np.zeros(64, np.float32), np.ones(1, np.int32), np.zeros(1, np.int64)
    assert lib.sr_mv_search(None, _native.ptr(f), _native.ptr(i), 1, 1, 1, None, 0, _native.ptr(f),
                            _native.ptr(r)) == _native.SR_ERR_INVALID
    assert lib.sr_mv_search_dev(None, None, None, 1, 1, 1, None, 0, 0, None, None, None) == _native.SR_ERR_INVALID
    q = ctypes.c_int(0)
    for dim in (0, 32, 100, 1088, -64):
        assert lib.sr_mv_search_group(dim, ctypes.byref(q)) == _native.SR_ERR_INVALID, dim
    assert lib.sr_mv_search_group(128, None) == _native.SR_ERR_INVALID


def test_group_queries_follow_the_lds_rule():
    from super_rag_amd.multivec import search_group_queries
    for dim in range(64, 1025, 64):
        block = 64 * ((dim + 127) // 128 * 128) * 2
        want = max(1, min(3, (160 * 1024 - 16 * 1024) // block))
        assert search_group_queries(dim) == want, dim
    assert search_group_queries(128) == 3 and search_group_queries(1024) == 1


class _Recorder:
    """Stands for a store / index: any use is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"touched {name} before rejecting the argument")


def test_m3_search_rejects_an_unknown_first_stage_before_any_work():
    from super_rag_amd.multivec import m3_search
    with pytest.raises(ValueError, match="nonsense"):
        m3_search(_Recorder(), _Recorder(), np.zeros((1, 8)), [np.zeros((1, 8))], 3, first_stage="nonsense")


def test_search_rejects_a_wrong_length_allow_before_the_call():
    from super_rag_amd import multivec

    class Fake(multivec.NativeMultiVectorIndex):
        def __init__(self):
            self._h, self.dim, self.device, self._dtype = None, 64, 0, "fp16"

        def stats(self):
            return {"rows": 5, "live": 5, "tokens": 9}

    x = Fake()
    q = [np.zeros((2, 64), np.float32)]
    for bad in (np.ones(4, np.uint8), np.ones(6, bool), np.ones((2, 5), np.uint8), []):
        with pytest.raises(ValueError, match="one entry per row"):
            x.search(q, 3, allow=bad)
    with pytest.raises(ValueError, match="padded queries"):
        x.search(np.zeros((2, 3, 32), np.float32), 3, q_len=[1, 1])
