"""Multi-vector (late interaction, ColBERT) retrieval on the MI355X library: the sr_mv index and the
bge-m3 "dense + sparse + multi-vector" rerank of first-stage candidates.

A document and a query are lists of per-token unit vectors (Encoder.embed_multivec); the score of a
pair is MaxSim, ``(1 / Lq) * sum_i max_j q_i . d_j``, computed exactly on the stored values by the
MFMA kernel of k_multivec.hip.  NativeMultiVectorIndex is row-aligned with the store like the
lexical indexes: row i of the index is row i of the collection (DESIGN.md "Multi-vector
retrieval").  The tokens are stored as fp16 (the default) or, with ``dtype="fp8"``, as one OCP e4m3
byte of ``256 x`` each: half the memory and half the bytes the kernel gathers, scored with the same
definition on the dequantised values (the query stays fp16).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _native as N


def pad_queries(q_vecs: Sequence, dim: int):
    """[(Lq_b, dim)] -> (q [B, ld_q, dim] fp32 zero padded, q_len [B] int32), ld_q = max(1, max Lq)."""
    B = len(q_vecs)
    arrs = [np.asarray(v, dtype=np.float32).reshape(-1, dim) for v in q_vecs]
    ld = max([1] + [a.shape[0] for a in arrs])
    q = np.zeros((B, ld, dim), dtype=np.float32)
    qlen = np.zeros(B, dtype=np.int32)
    for b, a in enumerate(arrs):
        q[b, :a.shape[0]] = a
        qlen[b] = a.shape[0]
    return q, qlen


MV_DTYPES = {"fp16": N.SR_DTYPE_F16, "fp8": N.SR_DTYPE_FP8_E4M3}


class NativeMultiVectorIndex:
    """Per-row token vectors resident in HBM of one device (sr_mv_*): one token pool, row offsets
    and live flags.  ``dim`` is a multiple of 64, at most 1024.  ``dtype``: "fp16", or "fp8" for
    e4m3(256 x) bytes (unit-norm tokens; an element past 1.75 in magnitude saturates)."""

    def __init__(self, dim: int, device: int = 0, dtype: str = "fp16"):
        self._h = None
        if dtype not in MV_DTYPES:
            raise ValueError(f"dtype must be one of {sorted(MV_DTYPES)}, got {dtype!r}")
        N.require_gpu()
        h = ctypes.c_void_p()
        N.call("sr_mv_create_dtype", int(dim), int(device), MV_DTYPES[dtype], ctypes.byref(h))
        self._h = h
        self.dim = int(dim)
        self.device = int(device)
        self._dtype = dtype

    @classmethod
    def load(cls, path: str, device: int = 0) -> "NativeMultiVectorIndex":
        """The index a snapshot written by ``save`` describes (sr_mv_load); ``dim`` and the dtype
        come from the file.  A file that breaks any rule of the format raises NativeError with
        SR_ERR_IO before any device work."""
        N.require_gpu()
        h = ctypes.c_void_p()
        N.call("sr_mv_load", path.encode(), int(device), ctypes.byref(h))
        self = cls.__new__(cls)
        self._h = h
        dim, dt = ctypes.c_int(0), ctypes.c_int(0)
        N.call("sr_mv_dim", h, ctypes.byref(dim))
        N.call("sr_mv_info", h, ctypes.byref(dt), None)
        self.dim = int(dim.value)
        self.device = int(device)
        self._dtype = {v: k for k, v in MV_DTYPES.items()}[int(dt.value)]
        return self

    def save(self, path: str) -> None:
        """Write the whole state, tombstoned rows included (sr_mv_save): through ``path + ".tmp"``,
        fsync and rename, so a failed save leaves a previous snapshot intact."""
        N.call("sr_mv_save", self._h, path.encode())

    def compact(self, stage_bytes: int = 0) -> np.ndarray:
        """Drop the removed rows in place (sr_mv_compact) -> old_to_new [rows] int64, -1 for a
        dropped row: the map NativeStore.compact returns for the same removals.  ``stage_bytes``
        bounds the staging memory (0: the default 64 MiB; at least one token's bytes)."""
        n = self.stats()["rows"]
        m = np.empty(max(n, 1), dtype=np.int64)
        N.call("sr_mv_compact", self._h, int(stage_bytes), N.ptr(m))
        return m[:n]

    @property
    def dtype(self) -> str:
        """"fp16" or "fp8": how the tokens are stored."""
        return self._dtype

    @property
    def nbytes(self) -> int:
        """Bytes of the stored tokens (sr_mv_info: tokens * dim * element size, not the capacity)."""
        n = ctypes.c_int64(0)
        N.call("sr_mv_info", self._h, None, ctypes.byref(n))
        return int(n.value)

    def close(self) -> None:
        if getattr(self, "_h", None):
            N.load().sr_mv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, docs: Sequence) -> int:
        """Append rows, each an array [n_tokens, dim] (fp32, rounded to fp16, then quantised on an
        fp8 index; 0 tokens allowed); returns the first row id."""
        arrs = [np.asarray(d, dtype=np.float32).reshape(-1, self.dim) for d in docs]
        off = np.zeros(len(arrs) + 1, dtype=np.int64)
        if arrs:
            off[1:] = np.cumsum([a.shape[0] for a in arrs])
        flat = (np.ascontiguousarray(np.concatenate(arrs, axis=0)) if arrs and off[-1]
                else np.zeros((1, self.dim), np.float32))
        first = ctypes.c_int64(0)
        N.call("sr_mv_add", self._h, N.ptr(off), N.ptr(flat), len(arrs), ctypes.byref(first))
        return int(first.value)

    def add_dev(self, vecs, lens, stream=None) -> int:
        """Append rows from device tensors: vecs fp16 [n, ld_tok, dim], lens int32 [n] (row i is the
        first lens[i] tokens of vecs[i]: Encoder.embed_multivec_dev's outputs); returns the first
        row id.  Reads the lengths back (synchronises the stream)."""
        import torch
        if not (vecs.is_cuda and vecs.is_contiguous() and vecs.dtype == torch.float16 and vecs.dim() == 3
                and vecs.shape[2] == self.dim):
            raise ValueError(f"add_dev: contiguous fp16 device vectors [n, ld_tok, {self.dim}]")
        if not (lens.is_cuda and lens.is_contiguous() and lens.dtype == torch.int32
                and lens.shape == (vecs.shape[0],)):
            raise ValueError("add_dev: contiguous int32 device lengths [n]")
        first = ctypes.c_int64(0)
        N.call("sr_mv_add_dev", self._h, N.ptr(vecs), N.ptr(lens), int(vecs.shape[0]), int(vecs.shape[1]),
               ctypes.byref(first), N.stream_handle(stream))
        return int(first.value)

    def remove(self, rows) -> None:
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        N.call("sr_mv_remove", self._h, N.ptr(r), int(r.size))

    def stats(self) -> dict:
        n, live, tok = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        N.call("sr_mv_stats", self._h, ctypes.byref(n), ctypes.byref(live), ctypes.byref(tok))
        return {"rows": int(n.value), "live": int(live.value), "tokens": int(tok.value)}

    def get(self, row: int) -> np.ndarray:
        """The stored token vectors of a row (fp8: dequantised), as fp32 [n_tokens, dim]."""
        n = ctypes.c_int64(0)
        N.call("sr_mv_get", self._h, int(row), None, 0, ctypes.byref(n))
        out = np.empty((int(n.value), self.dim), dtype=np.float32)
        if out.size:
            N.call("sr_mv_get", self._h, int(row), N.ptr(out), int(n.value), ctypes.byref(n))
        return out

    def score_rows(self, q_vecs, rows, q_len=None) -> np.ndarray:
        """MaxSim of given (query, row) pairs (sr_mv_score_rows).  q_vecs: a list of [Lq_b, dim]
        arrays, or, with q_len [B], one padded array [B, ld_q, dim] whose rows at and past q_len[b]
        are never read; rows [B, K] int64 -> score [B, K] fp32, -inf for a row < 0, past the index,
        removed or without tokens, and for an empty query."""
        if q_len is None:
            q, qlen = pad_queries(q_vecs, self.dim)
        else:
            q = np.ascontiguousarray(np.asarray(q_vecs, dtype=np.float32))
            qlen = np.ascontiguousarray(np.asarray(q_len, dtype=np.int32).reshape(-1))
            if q.ndim != 3 or q.shape[2] != self.dim or q.shape[0] != qlen.size:
                raise ValueError(f"padded queries must be [{qlen.size}, ld_q, {self.dim}], got {q.shape}")
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        if r.ndim != 2 or r.shape[0] != q.shape[0]:
            raise ValueError(f"rows must be [{q.shape[0]}, K], got {r.shape}")
        out = np.empty(r.shape, dtype=np.float32)
        if r.size:
            N.call("sr_mv_score_rows", self._h, N.ptr(q), N.ptr(qlen), q.shape[0], q.shape[1], N.ptr(r),
                   r.shape[1], N.ptr(out))
        return out

    def score_rows_dev(self, q, q_len, rows, out=None, stream=None):
        """score_rows on device tensors (sr_mv_score_rows_dev), asynchronous on ``stream``: q fp16
        [B, ld_q, dim], q_len int32 [B], rows int64 [B, K] -> fp32 [B, K].

        NOTE: unlike score_rows, this call cannot inspect ``q_len`` (it lives on the device and a
        check would synchronise the stream), so it raises nothing for a bad length: q_len[b] is
        CLAMPED to [0, min(ld_q, 512)].  A caller that passes q_len[b] > ld_q or > 512 gets the
        MaxSim over the first min(ld_q, 512) query tokens only, a plausible but different score,
        and no error; q_len[b] <= 0 gives -inf.  Keep q_len within the padded rows."""
        import torch
        if not (q.is_cuda and q.is_contiguous() and q.dtype == torch.float16 and q.dim() == 3
                and q.shape[2] == self.dim):
            raise ValueError(f"score_rows_dev: contiguous fp16 device queries [B, ld_q, {self.dim}]")
        if not (q_len.is_contiguous() and q_len.dtype == torch.int32 and rows.is_contiguous()
                and rows.dtype == torch.int64 and rows.dim() == 2 and rows.shape[0] == q.shape[0]
                and q_len.shape == (q.shape[0],)):
            raise ValueError("score_rows_dev: q_len int32 [B] and rows int64 [B, K]")
        B, K = rows.shape
        if out is None:
            out = torch.empty((B, K), dtype=torch.float32, device=q.device)
        if B and K:
            N.call("sr_mv_score_rows_dev", self._h, N.ptr(q), N.ptr(q_len), B, int(q.shape[1]), N.ptr(rows),
                   K, N.ptr(out), N.stream_handle(stream))
        return out

    def _padded(self, q_vecs, q_len, what):
        """(q [B, ld_q, dim] fp32, q_len [B] int32) of score_rows' / search's two query conventions."""
        if q_len is None:
            return pad_queries(q_vecs, self.dim)
        q = np.ascontiguousarray(np.asarray(q_vecs, dtype=np.float32))
        qlen = np.ascontiguousarray(np.asarray(q_len, dtype=np.int32).reshape(-1))
        if q.ndim != 3 or q.shape[2] != self.dim or q.shape[0] != qlen.size:
            raise ValueError(f"{what}: padded queries must be [{qlen.size}, ld_q, {self.dim}], got {q.shape}")
        return q, qlen

    def _allow_bytes(self, allow):
        """allow -> uint8 [rows] (non-zero: the row may be returned), ValueError on another length."""
        a = np.ascontiguousarray(np.asarray(allow).reshape(-1) != 0).astype(np.uint8)
        n = self.stats()["rows"]
        if a.size != n:
            raise ValueError(f"allow must have one entry per row ({n}), got {a.size}")
        return a

    def search(self, q_vecs, k: int, q_len=None, allow=None, slab_rows: int = 0):
        """Exact MaxSim top-k over the whole index (sr_mv_search): for every query the k eligible rows
        (live, at least one token, allow[row] != 0 where ``allow`` [rows] is given) with the highest
        MaxSim -> (score [B, k] fp32, rows [B, k] int64), ordered (score desc, row asc), -inf / -1 past
        the eligible rows and for an empty query.  Every score is score_rows' value of the pair, bit
        for bit.  q_vecs / q_len as for score_rows.  ``slab_rows`` bounds the rows scanned per pass
        (0: the default, 64 MiB of score scratch); the result does not depend on it."""
        q, qlen = self._padded(q_vecs, q_len, "search")
        a = None if allow is None else self._allow_bytes(allow)
        B = q.shape[0]
        score = np.empty((B, max(int(k), 0)), dtype=np.float32)
        rows = np.empty((B, max(int(k), 0)), dtype=np.int64)
        N.call("sr_mv_search", self._h, N.ptr(q), N.ptr(qlen), B, q.shape[1], int(k),
               None if a is None or a.size == 0 else N.ptr(a), int(slab_rows), N.ptr(score), N.ptr(rows))
        return score, rows

    def search_dev(self, q, q_len, k: int, allow=None, row_offset: int = 0, slab_rows: int = 0, out=None,
                   stream=None):
        """search on device tensors (sr_mv_search_dev), asynchronous on ``stream``: q fp16 [B, ld_q,
        dim], q_len int32 [B], allow uint8 / bool [rows] or None -> (score fp32 [B, k], rows int64
        [B, k]); ``row_offset`` is added to every real row; ``out`` may give the two output tensors.

        NOTE: unlike search, this call cannot inspect ``q_len`` (it lives on the device and a check
        would synchronise the stream), so it raises nothing for a bad length: q_len[b] is CLAMPED to
        [0, min(ld_q, 512)].  A caller that passes q_len[b] > ld_q or > 512 gets the MaxSim over the
        first min(ld_q, 512) query tokens only, a plausible but different ranking, and no error;
        q_len[b] <= 0 gives -inf / -1.  Keep q_len within the padded rows."""
        import torch
        if not (q.is_cuda and q.is_contiguous() and q.dtype == torch.float16 and q.dim() == 3
                and q.shape[2] == self.dim):
            raise ValueError(f"search_dev: contiguous fp16 device queries [B, ld_q, {self.dim}]")
        if not (q_len.is_cuda and q_len.is_contiguous() and q_len.dtype == torch.int32
                and q_len.shape == (q.shape[0],)):
            raise ValueError("search_dev: q_len int32 [B] on the device")
        if allow is not None:
            if not (allow.is_cuda and allow.is_contiguous() and allow.dtype in (torch.uint8, torch.bool)
                    and allow.dim() == 1):
                raise ValueError("search_dev: allow must be a contiguous uint8 / bool device tensor [rows]")
            n = self.stats()["rows"]
            if allow.numel() != n:
                raise ValueError(f"allow must have one entry per row ({n}), got {allow.numel()}")
        B, k = int(q.shape[0]), int(k)
        if out is None:
            out = (torch.empty((B, max(k, 0)), dtype=torch.float32, device=q.device),
                   torch.empty((B, max(k, 0)), dtype=torch.int64, device=q.device))
        score, rows = out
        if not (score.is_cuda and score.is_contiguous() and score.dtype == torch.float32
                and rows.is_cuda and rows.is_contiguous() and rows.dtype == torch.int64
                and tuple(score.shape) == (B, k) and tuple(rows.shape) == (B, k)):
            raise ValueError(f"search_dev: out must be (fp32 [{B}, {k}], int64 [{B}, {k}]) on the device")
        N.call("sr_mv_search_dev", self._h, N.ptr(q), N.ptr(q_len), B, int(q.shape[1]), k,
               None if allow is None or allow.numel() == 0 else N.ptr(allow), int(slab_rows), int(row_offset),
               N.ptr(score), N.ptr(rows), N.stream_handle(stream))
        return score, rows


def search_group_queries(dim: int) -> int:
    """Queries one workgroup of the whole-corpus scan shares a document tile among at ``dim``
    (sr_mv_search_group; needs no device)."""
    q = ctypes.c_int(0)
    N.call("sr_mv_search_group", int(dim), ctypes.byref(q))
    return int(q.value)


def _rows_live(part):
    """(rows, live) of a store (count()) or of a row-aligned index (stats())."""
    if hasattr(part, "count"):
        n, live = part.count()
    else:
        st = part.stats()
        n, live = st["rows"], st["live"]
    return int(n), int(live)


def compact_aligned(store, mv, *others, stage_bytes: int = 0) -> np.ndarray:
    """Compact a store, its token index and any further row-aligned indexes (impact / BM25) as one
    step, so row i of each stays row i of the collection -> old_to_new [rows] int64 (the store's
    map).  Raises ValueError, before anything is touched, unless every part reports the same
    (rows, live); RuntimeError naming the part whose map differs from the store's (the parts had
    different rows removed: the collection is then no longer aligned)."""
    parts = [("store", store), ("multivec", mv)] + [(f"index {i + 1}", o) for i, o in enumerate(others)]
    counts = [(name, _rows_live(p)) for name, p in parts]
    if any(c != counts[0][1] for _, c in counts):
        raise ValueError("compact_aligned: the parts are not row-aligned, (rows, live) = "
                         + ", ".join(f"{name} {c}" for name, c in counts))
    ref = np.asarray(store.compact(), dtype=np.int64)
    for name, p in parts[1:]:
        m = np.asarray(p.compact(stage_bytes) if p is mv else p.compact(), dtype=np.int64)
        if m.shape != ref.shape or not np.array_equal(m, ref):
            raise RuntimeError(f"compact_aligned: the map of {name} differs from the store's")
    return ref


def combine_dev(cos, maxsim, sparse, rows, k: int, weights=(1.0, 1.0, 1.0)):
    """The weighted mean and the selection of m3_rerank on device tensors [B, K] (fp32 scores, int64
    rows; sparse None drops that term and its weight): fp32, every operation rounded once, in the
    order ((w_d * cos + w_s * sparse) + w_c * maxsim) / (w_d + w_s + w_c).  A candidate is valid when
    its row is >= 0 and every score is finite; the others stay out.  -> (score [B, k] desc, rows
    [B, k]), ties to the lower row, -inf / -1 past the valid candidates."""
    import torch
    wd, ws, wc = (float(w) for w in weights)
    f = torch.float32
    dev = cos.device
    t = lambda w: torch.tensor(w, dtype=f, device=dev)
    total = t(wd) * cos
    wsum = np.float32(wd)
    valid = (rows >= 0) & torch.isfinite(cos) & torch.isfinite(maxsim)
    if sparse is not None:
        total = total + t(ws) * sparse
        wsum = np.float32(wsum + np.float32(ws))
        valid = valid & torch.isfinite(sparse)
    total = total + t(wc) * maxsim
    wsum = np.float32(wsum + np.float32(wc))
    score = total / t(float(wsum))
    neg = torch.full_like(score, float("-inf"))
    score = torch.where(valid, score, neg)
    big = torch.iinfo(torch.int64).max
    key_rows = torch.where(valid, rows, torch.full_like(rows, big))
    # (score desc, row asc): a stable sort by score over the rows in ascending order
    o1 = torch.argsort(key_rows, dim=1, stable=True)
    s1 = torch.gather(score, 1, o1)
    o2 = torch.argsort(s1, dim=1, descending=True, stable=True)
    order = torch.gather(o1, 1, o2)
    B, K = score.shape
    kk = min(int(k), K)
    out_s = torch.full((B, int(k)), float("-inf"), dtype=f, device=dev)
    out_r = torch.full((B, int(k)), -1, dtype=torch.int64, device=dev)
    out_s[:, :kk] = torch.gather(score, 1, order[:, :kk])
    out_r[:, :kk] = torch.gather(torch.where(valid, rows, torch.full_like(rows, -1)), 1, order[:, :kk])
    return out_s, out_r


def m3_rerank(store, mv: NativeMultiVectorIndex, q_dense, q_vecs, cand_rows, k: int, impact=None,
              q_sparse=None, weights=(1, 1, 1)):
    """bge-m3's "colbert+sparse+dense" rerank of first-stage candidates: the weighted mean
    ``(w_d * cos + w_s * sparse + w_c * maxsim) / (w_d + w_s + w_c)`` of the exact cosine
    (store.score_rows), the exact impact score (impact.score_rows of ``q_sparse``; the term and its
    weight are dropped when ``impact`` is None) and MaxSim (mv.score_rows of ``q_vecs``) of every
    candidate.  cand_rows [B, K] int64 (a first-stage list: a row is expected once per query and is
    reported as often as it is listed), -1 or removed rows stay out.  The sum and the selection run on
    the device -> (score [B, k] fp32 desc, rows [B, k] int64), ties to the lower row, -inf / -1 past
    the valid candidates."""
    import torch
    qd = np.ascontiguousarray(np.asarray(q_dense, dtype=np.float32))
    if qd.ndim == 1:
        qd = qd[None]
    r = np.ascontiguousarray(np.asarray(cand_rows, dtype=np.int64))
    if r.ndim != 2 or r.shape[0] != qd.shape[0]:
        raise ValueError(f"cand_rows must be [{qd.shape[0]}, K], got {r.shape}")
    if len(q_vecs) != qd.shape[0]:
        raise ValueError(f"{qd.shape[0]} dense queries but {len(q_vecs)} multi-vector ones")
    if impact is not None and (q_sparse is None or len(q_sparse) != qd.shape[0]):
        raise ValueError("an impact index needs one sparse query per dense query")
    if len(weights) != 3 or not all(np.isfinite(w) and w >= 0 for w in weights):
        raise ValueError("weights must be three finite values >= 0")
    if float(weights[0]) + (float(weights[1]) if impact is not None else 0.0) + float(weights[2]) <= 0:
        raise ValueError("the weights in use must not all be 0")
    cos = store.score_rows(qd, r)
    ms = mv.score_rows(q_vecs, r)
    sp = impact.score_rows(q_sparse, r) if impact is not None else None
    dev = torch.device("cuda", mv.device)
    d = lambda a: torch.as_tensor(a).to(dev)
    score, rows = combine_dev(d(cos), d(ms), None if sp is None else d(sp), d(r), int(k), weights)
    return score.cpu().numpy(), rows.cpu().numpy()


def m3_search(store, mv: NativeMultiVectorIndex, q_dense, q_vecs, k: int, k_cand: Optional[int] = None,
              impact=None, q_sparse=None, weights=(1, 1, 1), fusion: str = "rrf", allow=None,
              mask_key: int = 0, first_stage: str = "dense"):
    """First stage + m3_rerank: the k_cand (default 4 k) candidates of lexical.sparse_hybrid_search
    (dense + learned sparse, ``fusion`` as there) or, without an impact index, of store.search_sim,
    reranked by the combined score.  k <= k_cand <= 1024 (sr_mv_score_rows' limit on the candidates
    of one query); the default is clamped to it.  ``first_stage="multivec"`` takes the candidates
    from the exact MaxSim scan ``mv.search(q_vecs, k_cand, allow=allow)`` instead (``mask_key`` is
    unused there), so a passage only late interaction finds can reach the rerank."""
    if first_stage not in ("dense", "multivec"):
        raise ValueError(f'first_stage must be "dense" or "multivec", got {first_stage!r}')
    k = int(k)
    if not 1 <= k <= N.SR_MAX_TOPK:
        raise ValueError(f"k must be in [1, {N.SR_MAX_TOPK}], got {k}")
    k_cand = min(4 * k, N.SR_MAX_TOPK) if k_cand is None else int(k_cand)
    if not k <= k_cand <= N.SR_MAX_TOPK:
        raise ValueError(f"k_cand must be in [k, {N.SR_MAX_TOPK}] (the candidates one query can "
                         f"rerank), got k_cand = {k_cand} with k = {k}")
    qd = np.ascontiguousarray(np.asarray(q_dense, dtype=np.float32))
    if qd.ndim == 1:
        qd = qd[None]
    if first_stage == "multivec":
        _, cand = mv.search(q_vecs, k_cand, allow=allow)
    elif impact is not None:
        from .lexical import sparse_hybrid_search
        _, cand = sparse_hybrid_search(store, impact, qd, q_sparse, k_cand, fusion=fusion, allow=allow,
                                       mask_key=mask_key)
    else:
        _, cand = store.search_sim(qd, k_cand, allow=allow, mask_key=mask_key)
    return m3_rerank(store, mv, qd, q_vecs, cand, k, impact=impact, q_sparse=q_sparse, weights=weights)
