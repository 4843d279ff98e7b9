"""CPU: the reference of the multi-vector index's snapshots and in-place compaction
(tests/mv_snapshot_ref.py) against plain loops and hand-made cases, the library's new exports, and
multivec.compact_aligned's refusal on doubles.  The GPU tests (test_gpu_multivec_lifecycle.py) compare
the device against this reference bit for bit."""
import struct

import numpy as np
import pytest

import mv_snapshot_ref as R
from doubles import NumpyLex, NumpyStore

DTYPES = [R.DTYPE_F16, R.DTYPE_FP8]


# -- format ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_writer_and_parser_round_trip(dtype):
    b, lens, live = R.example(dtype)
    p = R.parse(b)
    assert (p["dim"], p["dtype"]) == (64, dtype)
    assert p["off"].tolist() == [0, 2, 2, 3] and p["live"].tolist() == live
    assert p["pool"].size == 3 * R.row_bytes(64, dtype)
    assert R.write(p["dim"], p["dtype"], np.diff(p["off"]), p["live"], p["pool"]) == b
    assert len(b) == 32 + 8 * 4 + 3 + 3 * R.row_bytes(64, dtype)
    # the header, field by field
    assert b[:8] == b"SRMIMVX1" and struct.unpack("<iiqq", b[8:32]) == (64, dtype, 3, 3)


def test_empty_index_round_trips():
    b = R.write(128, R.DTYPE_F16, [], [], np.zeros(0, np.uint8))
    assert len(b) == 40
    p = R.parse(b)
    assert p["off"].tolist() == [0] and p["live"].size == 0 and p["pool"].size == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_parser_rejects_each_corruption(dtype):
    b, _, _ = R.example(dtype)
    cases = R.corruptions(b)
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names) and len(cases) > len(b) + 40
    for want in ("trailing byte", "bad magic", "off[0] != 0", "decreasing offset", "off[n] != n_tokens",
                 "a row of 2^31 tokens", "live byte 2", "truncated at 0", f"truncated at {len(b) - 1}"):
        assert want in names
    assert ("fp8 byte 0x7f" in names) == (dtype == R.DTYPE_FP8)
    for name, bad in cases:
        assert bad != b, name
        with pytest.raises(R.SnapshotError):
            R.parse(bad)


def test_fp16_pool_may_hold_any_byte():
    b, _, _ = R.example(R.DTYPE_F16)
    R.parse(b[:-1] + b"\x7f")


# -- compaction --------------------------------------------------------------------------------------------
CASES = [
    ([3, 0, 5, 1, 4], [1, 0, 1, 0, 1]),
    ([3, 0, 5, 1, 4], [1, 1, 1, 1, 1]),
    ([3, 0, 5, 1, 4], [0, 0, 0, 0, 0]),
    ([3, 0, 5, 1, 4], [0, 1, 1, 1, 1]),
    ([3, 0, 5, 1, 4], [1, 1, 1, 1, 0]),
    ([4, 7, 1, 30, 0, 2, 9], [1, 1, 0, 1, 0, 1, 1]),        # a live prefix, then a dead 1-token row
    ([2, 0, 3, 0, 0, 6], [1, 0, 1, 0, 1, 1]),               # only zero-token rows are dead
    ([1, 40, 6, 3, 20, 5], [0, 1, 1, 0, 1, 1]),             # a row far longer than a small stage
    ([5, 1, 9, 65, 30, 12], [1, 0, 1, 0, 1, 1]),            # gap 1 (staged), then gap 66 (direct)
]


def _pool(lens, rb, seed=0):
    return np.random.default_rng(seed).integers(0, 256, int(np.sum(lens)) * rb, dtype=np.uint8)


@pytest.mark.parametrize("lens,live", CASES)
def test_compaction_reference_matches_a_plain_loop(lens, live):
    rb = 64
    pool = _pool(lens, rb)
    got_lens, got_live, got_pool, got_map = R.compact(lens, live, pool, rb)
    want_lens, want_pool, want_map, at, new = [], [], [], 0, 0
    for n, l in zip(lens, live):
        if l:
            want_lens.append(n)
            want_pool.append(pool[at * rb:(at + n) * rb])
            want_map.append(new)
            new += 1
        else:
            want_map.append(-1)
        at += n
    assert got_lens.tolist() == want_lens and got_map.tolist() == want_map
    assert got_live.tolist() == [1] * len(want_lens)
    assert got_pool.tobytes() == b"".join(p.tobytes() for p in want_pool)
    assert R.old_to_new(live).tolist() == want_map


@pytest.mark.parametrize("stage", [1, 2, 3, 7, 64, 1 << 20])
@pytest.mark.parametrize("lens,live", CASES)
def test_planner_properties(lens, live, stage):
    src = R.sources(lens, live)
    T = src.size
    chunks = R.plan(lens, live, stage)
    moved = np.nonzero(src != np.arange(T))[0]
    first = int(moved[0]) if moved.size else T
    # the chunks tile [first moved token, T) exactly once, in order
    at = first
    for t0, t1, staged in chunks:
        assert t0 == at and t1 > t0
        at = t1
        if staged:
            assert t1 - t0 <= stage                       # fits the stage
        else:
            assert src[t0:t1].min() >= t1                 # reads nothing it writes
    assert at == T
    # the leading prefix is untouched: everything before the first dead row at least
    dead = [i for i, l in enumerate(live) if not l]
    lead = int(np.sum(lens[:dead[0]])) if dead else T
    assert first >= min(lead, T)
    if not dead:
        assert chunks == []
    # the schedule executed in order, hazards checked, gives the reference's pool
    rb = 16
    pool = _pool(lens, rb, 3)
    want = R.compact(lens, live, pool, rb)[2]
    assert R.run_plan(lens, live, pool, rb, stage).tobytes() == want.tobytes()


def test_planner_hand_made_schedules():
    # rows 5 | 1 dead | 9 | 65 dead | 30 | 12, stage 3: tokens 0 .. 4 stay; the 9-token row (gap 1) goes
    # through the stage in three chunks; from the 30-token row on the gap is 66 and one direct launch
    # takes the remaining 42 tokens
    lens, live = [5, 1, 9, 65, 30, 12], [1, 0, 1, 0, 1, 1]
    assert R.plan(lens, live, 3) == [(5, 8, True), (8, 11, True), (11, 14, True), (14, 56, False)]
    # stage 1: gap 1 >= 1, so every chunk is direct and as long as its gap
    assert R.plan(lens, live, 1)[:3] == [(5, 6, False), (6, 7, False), (7, 8, False)]
    assert all(not s for _, _, s in R.plan(lens, live, 1))
    # a row longer than the stage is split, and chunks are cut by tokens, not rows: the 40-token row
    # behind a 1-token gap, stage 16 (the gap grows to 4 at token 46, still below the stage)
    lens, live = [1, 40, 6, 3, 20, 5], [0, 1, 1, 0, 1, 1]
    assert R.plan(lens, live, 16) == [(0, 16, True), (16, 32, True), (32, 48, True), (48, 64, True),
                                      (64, 71, True)]
    # stage 4: staged while the gap is 1, direct in gap-sized chunks once it is 4
    assert R.plan(lens, live, 4)[-7:] == [(44, 48, True)] + [(t, min(t + 4, 71), False) for t in range(48, 71, 4)]
    # a large stage and a small gap: everything in one staged chunk
    assert R.plan(lens, live, 1 << 20) == [(0, 71, True)]
    # a stage above the direct threshold: a gap of 4 tokens is enough for a chunk to go direct, whatever
    # the stage; below it the chunk takes the whole stage
    assert R.plan(lens, live, 16, 4) == [(0, 16, True), (16, 32, True), (32, 48, True)] + [
        (t, min(t + 4, 71), False) for t in range(48, 71, 4)]
    assert R.plan(lens, live, 3, 4) == R.plan(lens, live, 3)
    pool = _pool(lens, 16, 9)
    assert R.run_plan(lens, live, pool, 16, 16, 4).tobytes() == R.compact(lens, live, pool, 16)[2].tobytes()
    # nothing dead, or only rows without tokens dead: nothing moves
    assert R.plan([3, 4], [1, 1], 8) == []
    assert R.plan([2, 0, 3, 0, 0, 6], [1, 0, 1, 0, 1, 1], 8) == []
    assert R.plan([3, 4], [0, 0], 8) == []


# -- the library and the Python surface --------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    from super_rag_amd import _native
    lib = _native.load()
    for name in ("sr_mv_compact", "sr_mv_save", "sr_mv_load", "sr_mv_dim"):
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    # argument errors are reported without a device
    assert lib.sr_mv_compact(None, 0, None) == _native.SR_ERR_INVALID
    assert lib.sr_mv_save(None, b"x") == _native.SR_ERR_INVALID
    assert lib.sr_mv_load(None, 0, None) == _native.SR_ERR_INVALID
    assert lib.sr_mv_dim(None, None) == _native.SR_ERR_INVALID


def test_loader_refuses_a_corrupt_file_before_any_device_work(tmp_path):
    import ctypes
    from super_rag_amd import _native
    lib = _native.load()
    b, _, _ = R.example(R.DTYPE_FP8)
    p = tmp_path / "x.srmv"
    for name, bad in R.corruptions(b, truncations=False) + [("truncated", b[:-1]), ("empty", b"")]:
        p.write_bytes(bad)
        h = ctypes.c_void_p()
        assert lib.sr_mv_load(str(p).encode(), 0, ctypes.byref(h)) == _native.SR_ERR_IO, name
        assert not h.value
    assert lib.sr_mv_load(str(tmp_path / "missing").encode(), 0, ctypes.byref(h)) == _native.SR_ERR_IO


class _MvDouble:
    """A token index double: counts only, and a record of the calls."""

    def __init__(self, rows, live):
        self.rows, self.live, self.calls = rows, live, []

    def stats(self):
        return {"rows": self.rows, "live": self.live, "tokens": 0}

    def compact(self, stage_bytes=0):
        self.calls.append(stage_bytes)
        m = np.full(self.rows, -1, np.int64)
        m[:self.live] = np.arange(self.live)
        return m


def test_compact_aligned_rejects_mismatched_counts_before_any_call():
    from super_rag_amd.multivec import compact_aligned
    store = NumpyStore(4)
    store.add(np.eye(4))
    store.remove([3])
    lex = NumpyLex()
    lex.add([[1], [2], [3], [4]])
    lex.remove([3])
    for mv in (_MvDouble(4, 4), _MvDouble(5, 3), _MvDouble(3, 3)):
        with pytest.raises(ValueError, match="row-aligned"):
            compact_aligned(store, mv, lex)
        assert mv.calls == [] and store.count() == (4, 3) and lex.stats() == {"rows": 4, "live": 3}
    lex2 = NumpyLex()
    lex2.add([[1], [2], [3], [4]])
    with pytest.raises(ValueError):
        compact_aligned(store, _MvDouble(4, 3), lex2)
    assert store.count() == (4, 3)


def test_compact_aligned_compacts_every_part_and_names_a_differing_map():
    from super_rag_amd.multivec import compact_aligned
    store = NumpyStore(4)
    store.add(np.eye(4))
    store.remove([3])
    lex = NumpyLex()
    lex.add([[1], [2], [3], [4]])
    lex.remove([3])
    mv = _MvDouble(4, 3)
    m = compact_aligned(store, mv, lex, stage_bytes=4096)
    assert m.tolist() == [0, 1, 2, -1] and mv.calls == [4096]
    assert store.count() == (3, 3) and lex.stats() == {"rows": 3, "live": 3}
    # the same counts but another row removed: the maps differ, and the part is named
    store = NumpyStore(4)
    store.add(np.eye(4))
    store.remove([0])
    with pytest.raises(RuntimeError, match="multivec"):
        compact_aligned(store, _MvDouble(4, 3))
