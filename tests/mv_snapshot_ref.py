"""Reference restatement of the multi-vector index's snapshots and in-place compaction, numpy
(multivec.hip MultiVecIndex::save / load / compact; DESIGN.md "Multi-vector retrieval").

write(...)        the snapshot's bytes: "SRMIMVX1", int32 dim, int32 dtype, int64 n_rows, int64
                  n_tokens, (n_rows + 1) int64 offsets, n_rows live bytes, n_tokens * row_bytes pool
                  bytes (little endian)
parse(bytes)      the fields back, raising SnapshotError on every rule the loader enforces
pool_bytes(...)   the pool bytes of rows given as fp32 token arrays: fp16 values, or the e4m3 bytes of
                  mv_fp8_ref.quant
compact(...)      (lens, live, pool) after dropping the dead rows, and old_to_new
plan(...)         the chunk schedule of the in-place compaction: (t0, t1, staged) over the kept
                  tokens that move
run_plan(...)     the schedule executed on a numpy pool in chunk order, reading only the pool as the
                  earlier chunks left it: what the device does, hazards included
"""
import struct

import numpy as np

MAGIC = b"SRMIMVX1"
DTYPE_F16, DTYPE_FP8 = 1, 2            # SR_DTYPE_F16, SR_DTYPE_FP8_E4M3
HEADER = 32
LIMIT = 1 << 40
DEFAULT_STAGE_BYTES = 64 << 20
DIRECT_MIN_BYTES = 16 << 20


class SnapshotError(ValueError):
    pass


def row_bytes(dim, dtype):
    return dim * (1 if dtype == DTYPE_FP8 else 2)


def write(dim, dtype, lens, live, pool):
    """lens [n] tokens per row, live [n] 0 / 1, pool: uint8 [n_tokens * row_bytes] -> bytes."""
    lens = np.asarray(lens, np.int64)
    off = np.zeros(lens.size + 1, np.int64)
    off[1:] = np.cumsum(lens)
    pool = np.ascontiguousarray(pool, np.uint8).reshape(-1)
    assert pool.size == int(off[-1]) * row_bytes(dim, dtype)
    return (MAGIC + struct.pack("<iiqq", dim, dtype, lens.size, int(off[-1])) + off.astype("<i8").tobytes()
            + np.asarray(live, np.uint8).tobytes() + pool.tobytes())


def parse(b):
    """-> dict(dim, dtype, off, live, pool); SnapshotError for anything the loader refuses."""
    b = bytes(b)
    if len(b) < HEADER or b[:8] != MAGIC:
        raise SnapshotError("magic")
    dim, dtype, n, T = struct.unpack("<iiqq", b[8:HEADER])
    if not (64 <= dim <= 1024 and dim % 64 == 0):
        raise SnapshotError("dim")
    if dtype not in (DTYPE_F16, DTYPE_FP8):
        raise SnapshotError("dtype")
    if not (0 <= n <= LIMIT and 0 <= T <= LIMIT):
        raise SnapshotError("counts")
    rb = row_bytes(dim, dtype)
    if len(b) != HEADER + 8 * (n + 1) + n + T * rb:
        raise SnapshotError("size")
    off = np.frombuffer(b, "<i8", n + 1, HEADER).astype(np.int64)
    live = np.frombuffer(b, np.uint8, n, HEADER + 8 * (n + 1))
    pool = np.frombuffer(b, np.uint8, T * rb, HEADER + 8 * (n + 1) + n)
    if off[0] != 0 or off[-1] != T:
        raise SnapshotError("offset ends")
    for i in range(n):
        if int(off[i + 1]) < int(off[i]) or int(off[i + 1]) - int(off[i]) >= 1 << 31:
            raise SnapshotError("offsets")
    if (live > 1).any():
        raise SnapshotError("live")
    if dtype == DTYPE_FP8 and ((pool & 0x7F) == 0x7F).any():
        raise SnapshotError("fp8 NaN code")
    return {"dim": dim, "dtype": dtype, "off": off, "live": live.copy(), "pool": pool.copy()}


def pool_bytes(docs, dim, dtype):
    """docs: fp32 arrays [n_tokens, dim] (the values the index holds for fp16; the values added for
    fp8) -> uint8 pool."""
    if not docs:
        return np.zeros(0, np.uint8)
    x = np.concatenate([np.asarray(d, np.float32).reshape(-1, dim) for d in docs], axis=0)
    if dtype == DTYPE_FP8:
        import mv_fp8_ref as Q
        return Q.quant(x).reshape(-1)
    return x.astype("<f2").view(np.uint8).reshape(-1)


def example(dtype, dim=64, seed=5):
    """A small valid snapshot: 3 rows of 2 / 0 / 1 tokens, the last one dead -> (bytes, lens, live)."""
    rng = np.random.default_rng(seed + dtype)
    lens, live = [2, 0, 1], [1, 1, 0]
    x = rng.standard_normal((3, dim))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return write(dim, dtype, lens, live, pool_bytes([x], dim, dtype)), lens, live


def _patched(b, at, fmt, value):
    out = bytearray(b)
    out[at:at + struct.calcsize(fmt)] = struct.pack(fmt, value)
    return bytes(out)


def corruptions(b, truncations=True):
    """[(name, bytes)]: single corruptions of the valid snapshot b (of example()'s shape: 3 rows),
    each of which the loader must refuse.  The header values include ones near 2^31, 2^40 and 2^62
    and negatives."""
    dim, dtype, n, T = struct.unpack("<iiqq", b[8:HEADER])
    out = []
    if truncations:
        out += [(f"truncated at {k}", b[:k]) for k in range(len(b))]
    out.append(("trailing byte", b + b"\0"))
    out.append(("bad magic", b[:3] + bytes([b[3] ^ 0x20]) + b[4:]))
    for d in (0, -64, 32, 96, 1088, 2048, 0x7FFFFFC0, -(1 << 31)):
        out.append((f"dim {d}", _patched(b, 8, "<i", d)))
    for t in (0, 3, -1, 0x7FFFFFFF, 256 + dtype):
        out.append((f"dtype {t}", _patched(b, 12, "<i", t)))
    big = (-1, n - 1, n + 1, (1 << 31) - 1, 1 << 31, 1 << 40, (1 << 40) + 1, 1 << 62, -(1 << 62), -(1 << 63))
    for v in big:
        out.append((f"n_rows {v}", _patched(b, 16, "<q", v)))
    for v in big[:1] + (T - 1, T + 1) + big[3:]:
        out.append((f"n_tokens {v}", _patched(b, 24, "<q", v)))
    o = HEADER
    out.append(("off[0] != 0", _patched(b, o, "<q", 1)))
    out.append(("off[0] negative", _patched(b, o, "<q", -1)))
    out.append(("decreasing offset", _patched(b, o + 8, "<q", T + 1)))   # off[1] > off[2]
    out.append(("negative offset", _patched(b, o + 16, "<q", -(1 << 62))))
    out.append(("off[n] != n_tokens", _patched(b, o + 8 * n, "<q", T + 1)))
    out.append(("a row of 2^31 tokens", _patched(_patched(b, o + 8 * n, "<q", (1 << 31) + 2), 24, "<q", (1 << 31) + 2)))
    out.append(("live byte 2", _patched(b, o + 8 * (n + 1), "<B", 2)))
    out.append(("live byte 255", _patched(b, o + 8 * (n + 1) + n - 1, "<B", 255)))
    if dtype == DTYPE_FP8:
        p = o + 8 * (n + 1) + n
        out.append(("fp8 byte 0x7f", _patched(b, p + 5, "<B", 0x7F)))
        out.append(("fp8 byte 0xff", _patched(b, len(b) - 1, "<B", 0xFF)))
    return out


def old_to_new(live):
    live = np.asarray(live).astype(bool)
    m = np.full(live.size, -1, np.int64)
    m[live] = np.arange(int(live.sum()))
    return m


def compact(lens, live, pool, rb):
    """-> (lens, live, pool, old_to_new) after dropping the dead rows, kept rows in order."""
    lens = np.asarray(lens, np.int64)
    live = np.asarray(live).astype(bool)
    pool = np.asarray(pool, np.uint8).reshape(-1, rb)
    tok_live = np.repeat(live, lens)
    return lens[live], np.ones(int(live.sum()), np.uint8), pool[tok_live].reshape(-1), old_to_new(live)


def sources(lens, live):
    """src[t]: the old pool position of the kept token that lands at t."""
    lens = np.asarray(lens, np.int64)
    return np.nonzero(np.repeat(np.asarray(live).astype(bool), lens))[0].astype(np.int64)


def plan(lens, live, stage_tokens, direct_tokens=None):
    """The chunks [(t0, t1, staged)] over the kept tokens from the first one that moves: with gap =
    src(t0) - t0, left = the tokens still to place and D = min(stage_tokens, direct_tokens), direct (t1
    = t0 + min(gap, left)) when gap >= min(D, left), else staged (t1 = t0 + min(stage_tokens, left)).
    direct_tokens: DIRECT_MIN_BYTES // row_bytes, the gap from which a chunk goes pool -> pool whatever
    the stage; None (no such cap) gives the same schedule whenever stage_tokens is not above it."""
    assert stage_tokens >= 1
    D = stage_tokens if direct_tokens is None else min(stage_tokens, max(1, direct_tokens))
    src = sources(lens, live)
    T = src.size
    moved = np.nonzero(src != np.arange(T))[0]
    out = []
    t = int(moved[0]) if moved.size else T
    while t < T:
        gap = int(src[t]) - t
        if gap >= min(D, T - t):
            out.append((t, t + min(gap, T - t), False))
        else:
            out.append((t, t + min(stage_tokens, T - t), True))
        t = out[-1][1]
    return out


def run_plan(lens, live, pool, rb, stage_tokens, direct_tokens=None):
    """Executes plan() on a copy of the pool the way the device does: a direct chunk reads and writes
    the pool itself, a staged chunk goes through a buffer of stage_tokens tokens.  Every write is
    checked against the reads still to come, so a schedule with a hazard fails here."""
    pool = np.array(pool, np.uint8).reshape(-1, rb)
    src = sources(lens, live)
    dirty = np.zeros(pool.shape[0], bool)             # positions some chunk has written
    for t0, t1, staged in plan(lens, live, stage_tokens, direct_tokens):
        s = src[t0:t1]
        assert not dirty[s].any(), "a chunk reads what an earlier chunk wrote"
        if staged:
            assert t1 - t0 <= stage_tokens
            stage = pool[s].copy()
            pool[t0:t1] = stage
        else:
            assert s.min() >= t1, "a direct chunk reads its own destination"
            pool[t0:t1] = pool[s]
        dirty[t0:t1] = True
    return pool[:src.size].reshape(-1)
