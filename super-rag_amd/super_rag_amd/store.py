"""Python handle of the in-HBM cosine store (sr_store_* in include/super_rag_mi355x.h)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N


class NativeStore:
    """Exact cosine top-k over L2-normalised fp16 rows resident in HBM of one device.

    Row ids are int64 positions (append order); the vector-store connector maps them to the
    uuid strings the reference hands out (seekdb_connector.py:68-85).
    """

    def __init__(self, dim: int, device: int = 0, capacity: int = 1024, _handle=None):
        self._h = None
        if _handle is None:
            N.require_gpu()
            h = ctypes.c_void_p()
            N.call("sr_store_create", int(dim), int(device), int(capacity), ctypes.byref(h))
            _handle = h
        self._h = _handle
        self.device = int(device)
        d = ctypes.c_int32(0)
        N.call("sr_store_dim", self._h, ctypes.byref(d))
        self.dim = int(d.value)

    @classmethod
    def load(cls, path: str, device: int = 0) -> "NativeStore":
        N.require_gpu()
        h = ctypes.c_void_p()
        N.call("sr_store_load", path.encode(), int(device), ctypes.byref(h))
        return cls(0, device, _handle=h)

    def close(self) -> None:
        if self._h:
            N.load().sr_store_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- mutation ---------------------------------------------------------------------------------
    def add(self, vecs) -> np.ndarray:
        v = np.ascontiguousarray(np.asarray(vecs, dtype=np.float32))
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise ValueError(f"expected (n, {self.dim}) vectors, got {v.shape}")
        rows = np.empty(v.shape[0], dtype=np.int64)
        N.call("sr_store_add", self._h, N.ptr(v), v.shape[0], N.ptr(rows))
        return rows

    def add_dev(self, vecs, stream=None) -> int:
        """Append rows from a device tensor (fp32/fp16, [n, dim]); returns the first row id."""
        import torch
        assert vecs.is_cuda and vecs.is_contiguous() and vecs.shape[1] == self.dim
        dt = N.SR_DTYPE_F16 if vecs.dtype == torch.float16 else N.SR_DTYPE_F32
        if vecs.dtype not in (torch.float16, torch.float32):
            raise TypeError("add_dev: fp16 or fp32 rows")
        first = ctypes.c_int64(0)
        N.call("sr_store_add_dev", self._h, N.ptr(vecs), dt, vecs.shape[0], ctypes.byref(first),
               N.stream_handle(stream))
        return int(first.value)

    def remove(self, rows) -> None:
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        N.call("sr_store_remove", self._h, N.ptr(r), r.shape[0])

    def compact(self) -> np.ndarray:
        n, _ = self.count()
        m = np.empty(max(n, 1), dtype=np.int64)
        N.call("sr_store_compact", self._h, N.ptr(m))
        return m[:n]

    def set_scan_dtype(self, dtype: str) -> None:
        """"fp16" (default) or "fp8": scan an OCP e4m3 copy of the rows with the block-scaled fp8
        MFMA and re-score the candidates exactly on the fp16 rows (sr_store_set_scan_dtype)."""
        code = {"fp16": N.SR_DTYPE_F16, "fp8": N.SR_DTYPE_FP8_E4M3}[dtype]
        N.call("sr_store_set_scan_dtype", self._h, code)

    def save(self, path: str) -> None:
        N.call("sr_store_save", self._h, path.encode())

    # -- queries ----------------------------------------------------------------------------------
    def count(self):
        n, live = ctypes.c_int64(0), ctypes.c_int64(0)
        N.call("sr_store_count", self._h, ctypes.byref(n), ctypes.byref(live))
        return int(n.value), int(live.value)

    def get(self, rows) -> np.ndarray:
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        out = np.empty((r.shape[0], self.dim), dtype=np.float32)
        N.call("sr_store_get", self._h, N.ptr(r), r.shape[0], N.ptr(out))
        return out

    def search(self, queries, k: int, allow=None, mask_key: int = 0):
        """Host path: returns (dist [B,k] fp32, rows [B,k] int64); dist = 1 - cos, ascending.
        ``allow`` (bool/uint8 [n_rows]) restricts the candidates to the allowed rows (the mask is
        cached on the device while ``mask_key`` != 0 and the store is unchanged)."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        B = q.shape[0]
        dist = np.empty((B, k), dtype=np.float32)
        rows = np.empty((B, k), dtype=np.int64)
        if allow is None:
            N.call("sr_store_search", self._h, N.ptr(q), B, int(k), N.ptr(dist), N.ptr(rows))
        else:
            n, _ = self.count()
            a = np.ascontiguousarray(np.asarray(allow, dtype=np.uint8))
            if a.shape != (n,):
                raise ValueError(f"allow mask must have {n} entries, got {a.shape}")
            if n == 0:
                a = np.zeros(1, dtype=np.uint8)
            N.call("sr_store_search_masked", self._h, N.ptr(q), B, int(k), N.ptr(a), int(mask_key),
                   N.ptr(dist), N.ptr(rows))
        return dist, rows

    def search_sim(self, queries, k: int, allow=None, mask_key: int = 0):
        """search() returning (sim [B,k] fp32 descending, -inf when missing; rows [B,k]): the
        exact similarities, for merging several stores' lists (ShardedStore)."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        B = q.shape[0]
        sim = np.empty((B, k), dtype=np.float32)
        rows = np.empty((B, k), dtype=np.int64)
        a = None
        if allow is not None:
            n, _ = self.count()
            a = np.ascontiguousarray(np.asarray(allow, dtype=np.uint8))
            if a.shape != (n,):
                raise ValueError(f"allow mask must have {n} entries, got {a.shape}")
            if n == 0:
                a = np.zeros(1, dtype=np.uint8)
        N.call("sr_store_search_sim", self._h, N.ptr(q), B, int(k), N.ptr(a) if a is not None else None,
               int(mask_key) if a is not None else 0, N.ptr(sim), N.ptr(rows))
        return np.where(rows >= 0, sim, -np.inf).astype(np.float32), rows

    def search_subset(self, queries, k: int, lists, q_list=None, sim: bool = False):
        """Pre-filtered search: query b searches only the rows of ``lists[q_list[b]]``
        (sr_store_search_subset; one device launch whatever the number of distinct lists).
        ``lists``: a sequence of int64 row arrays, each strictly ascending; ``q_list`` [B] defaults to
        arange(B), which needs one list per query.  Returns (dist [B,k] fp32 = 1 - sim, +inf when
        missing; rows [B,k] int64, -1 when missing) exactly as search() reports them, or with
        ``sim=True`` (sim [B,k] descending, -inf when missing; rows).  Tombstoned rows are skipped;
        the fp16 rows are read in either scan mode."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        B = q.shape[0]
        off, flat = pack_lists(lists)
        if q_list is None:
            if len(lists) != B:
                raise ValueError(f"search_subset: {len(lists)} lists for {B} queries and no q_list")
            ql = np.arange(B, dtype=np.int32)
        else:
            ql = np.ascontiguousarray(np.asarray(q_list, dtype=np.int32))
            if ql.shape != (B,):
                raise ValueError(f"q_list must have {B} entries, got {ql.shape}")
        s = np.empty((B, k), dtype=np.float32)
        rows = np.empty((B, k), dtype=np.int64)
        N.call("sr_store_search_subset", self._h, N.ptr(q), B, int(k), N.ptr(ql), len(lists),
               N.ptr(off), N.ptr(flat), N.ptr(s), N.ptr(rows))
        if sim:
            return np.where(rows >= 0, s, -np.inf).astype(np.float32), rows
        return np.where(rows >= 0, np.float32(1.0) - s, np.float32(np.inf)).astype(np.float32), rows

    def search_dev(self, q, k: int, out_sim=None, out_rows=None, row_offset: int = 0, stream=None):
        """Device path: q [B, >=dim] fp16/fp32 device tensor (only the first `dim` columns are
        read when q is exactly [B, dim]; a padded fp16 [B, ld] query must be sliced by the caller).
        Returns (sim [B,k] fp32, rows [B,k] int64) device tensors."""
        import torch
        assert q.is_cuda and q.is_contiguous() and q.shape[1] == self.dim
        B = q.shape[0]
        dt = N.SR_DTYPE_F16 if q.dtype == torch.float16 else N.SR_DTYPE_F32
        if out_sim is None:
            out_sim = torch.empty((B, k), dtype=torch.float32, device=q.device)
        if out_rows is None:
            out_rows = torch.empty((B, k), dtype=torch.int64, device=q.device)
        N.call("sr_store_search_dev", self._h, N.ptr(q), dt, B, int(k), N.ptr(out_sim),
               N.ptr(out_rows), int(row_offset), N.stream_handle(stream))
        return out_sim, out_rows


    def search_mmr(self, queries, k: int, fetch_k: int, lam: float = 0.5, mode: str = "onepass",
                   min_score: float = -2.0, allow=None, mask_key: int = 0):
        """Top-``fetch_k`` scan, then MMR diversification on the device, keep ``k``
        (sr_store_search_mmr).  Returns (score [B,k] fp32 MMR score, -inf when missing; dist [B,k]
        fp32 = 1 - cos of the kept rows, +inf when missing; rows [B,k] int64, -1 when missing), each
        query's results in MMR order.  ``mode``: "onepass" (graphiti's function) or "greedy"."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        B = q.shape[0]
        score = np.empty((B, k), dtype=np.float32)
        dist = np.empty((B, k), dtype=np.float32)
        rows = np.empty((B, k), dtype=np.int64)
        a = None
        if allow is not None:
            n, _ = self.count()
            a = np.ascontiguousarray(np.asarray(allow, dtype=np.uint8))
            if a.shape != (n,):
                raise ValueError(f"allow mask must have {n} entries, got {a.shape}")
            if n == 0:
                a = np.zeros(1, dtype=np.uint8)
        N.call("sr_store_search_mmr", self._h, N.ptr(q), B, int(k), int(fetch_k), float(lam),
               mmr_mode(mode), float(min_score), N.ptr(a) if a is not None else None,
               int(mask_key) if a is not None else 0, N.ptr(score), N.ptr(dist), N.ptr(rows))
        return score, dist, rows

    def mmr_dev(self, cand_rows, cand_sims, k: int, lam: float = 0.5, mode: str = "onepass",
                min_score: float = -2.0, row_offset: int = 0, stream=None):
        """MMR over candidates as search_dev wrote them (device tensors [B, K]: rows carrying
        ``row_offset``, -1 = missing; similarities).  Returns device tensors (score [B,k] fp32,
        sim [B,k] fp32, rows [B,k] int64), -inf / -inf / -1 past the end (sr_store_mmr_dev)."""
        import torch
        assert cand_rows.is_cuda and cand_rows.is_contiguous() and cand_rows.dtype == torch.int64
        assert cand_sims.is_cuda and cand_sims.is_contiguous() and cand_sims.dtype == torch.float32
        assert cand_rows.shape == cand_sims.shape and cand_rows.dim() == 2
        B, K = cand_rows.shape
        out_score = torch.empty((B, k), dtype=torch.float32, device=cand_rows.device)
        out_sim = torch.empty((B, k), dtype=torch.float32, device=cand_rows.device)
        out_rows = torch.empty((B, k), dtype=torch.int64, device=cand_rows.device)
        N.call("sr_store_mmr_dev", self._h, N.ptr(cand_rows), N.ptr(cand_sims), B, K, int(row_offset),
               float(lam), mmr_mode(mode), float(min_score), int(k), N.ptr(out_score),
               N.ptr(out_sim), N.ptr(out_rows), N.stream_handle(stream))
        return out_score, out_sim, out_rows

    def score_rows(self, queries, rows) -> np.ndarray:
        """Exact cosine of given (query, row) pairs on the fp16 rows (sr_store_score_rows): queries
        [B, dim], rows [B, K] int64 -> sim [B, K] fp32, -inf for a row < 0, a row outside the store
        or a tombstoned row.  The same value in either scan mode."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        if r.ndim != 2 or r.shape[0] != q.shape[0]:
            raise ValueError(f"rows must be [{q.shape[0]}, K], got {r.shape}")
        out = np.empty(r.shape, dtype=np.float32)
        if r.size:
            N.call("sr_store_score_rows", self._h, N.ptr(q), q.shape[0], N.ptr(r), r.shape[1],
                   N.ptr(out))
        return out

    def score_rows_dev(self, q, rows, row_offset: int = 0, out=None, stream=None):
        """score_rows on device tensors: q [B, dim] fp16/fp32 as search_dev takes it, rows [B, K]
        int64 carrying ``row_offset`` -> sim [B, K] fp32 device tensor (sr_store_score_rows_dev)."""
        import torch
        assert q.is_cuda and q.is_contiguous() and q.shape[1] == self.dim
        assert rows.is_cuda and rows.is_contiguous() and rows.dtype == torch.int64
        assert rows.dim() == 2 and rows.shape[0] == q.shape[0]
        dt = N.SR_DTYPE_F16 if q.dtype == torch.float16 else N.SR_DTYPE_F32
        if out is None:
            out = torch.empty(tuple(rows.shape), dtype=torch.float32, device=q.device)
        if rows.numel():
            N.call("sr_store_score_rows_dev", self._h, N.ptr(q), dt, q.shape[0], N.ptr(rows),
                   rows.shape[1], int(row_offset), N.ptr(out), N.stream_handle(stream))
        return out

    def _group_arg(self, group):
        n, _ = self.count()
        g = np.ascontiguousarray(np.asarray(group, dtype=np.int32))
        if g.shape != (n,):
            raise ValueError(f"group array must have {n} entries, got {g.shape}")
        return g if n else np.zeros(1, dtype=np.int32)

    def search_grouped(self, queries, k: int, group, group_size: int = 1, fetch_k: int | None = None,
                       allow=None, mask_key: int = 0, group_key: int = 0, sim: bool = False):
        """Grouped search (sr_store_search_grouped): the ``k`` best distinct groups of every query
        with the ``group_size`` best rows of each, exact whatever ``fetch_k`` (the rows scanned per
        round; default min(1024, max(4 k group_size, 64))).  ``group`` int32 [n_rows]: >= 0 a group,
        -1 a group of its own; kept on the device while ``group_key`` != 0 and the store is
        unchanged.  Returns (dist [B,k,g] fp32 = 1 - sim, +inf when missing, or with ``sim=True`` the
        similarities, -inf when missing; rows [B,k,g] int64, -1 when missing; groups [B,k] int32,
        -1 for an unfilled group slot): groups best first, a group's rows best first."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        B, k, gs = q.shape[0], int(k), int(group_size)
        fetch = group_fetch_k(k, gs) if fetch_k is None else int(fetch_k)
        g = self._group_arg(group)
        a = None
        if allow is not None:
            n, _ = self.count()
            a = np.ascontiguousarray(np.asarray(allow, dtype=np.uint8))
            if a.shape != (n,):
                raise ValueError(f"allow mask must have {n} entries, got {a.shape}")
            if n == 0:
                a = np.zeros(1, dtype=np.uint8)
        shape = (B, max(k, 0), max(gs, 0))
        s = np.empty(shape, dtype=np.float32)
        rows = np.empty(shape, dtype=np.int64)
        groups = np.empty(shape[:2], dtype=np.int32)
        N.call("sr_store_search_grouped", self._h, N.ptr(q), B, k, gs, fetch, N.ptr(g), int(group_key),
               N.ptr(a) if a is not None else None, int(mask_key) if a is not None else 0,
               N.ptr(s), N.ptr(rows), N.ptr(groups))
        if sim:
            return np.where(rows >= 0, s, -np.inf).astype(np.float32), rows, groups
        return (np.where(rows >= 0, np.float32(1.0) - s, np.float32(np.inf)).astype(np.float32), rows,
                groups)

    def group_dev(self, cand_rows, cand_sims, k: int, group, group_size: int = 1, group_key: int = 0,
                  row_offset: int = 0, stream=None):
        """Collapse candidates as search_dev wrote them (device tensors [B, K]) into the ``k`` best
        groups with ``group_size`` rows each, no continuation (sr_store_group_dev).  Returns device
        tensors (sim [B,k,g] fp32, rows [B,k,g] int64, groups [B,k] int32, complete [B] int32: 1
        when the query's result is already exact)."""
        import torch
        assert cand_rows.is_cuda and cand_rows.is_contiguous() and cand_rows.dtype == torch.int64
        assert cand_sims.is_cuda and cand_sims.is_contiguous() and cand_sims.dtype == torch.float32
        assert cand_rows.shape == cand_sims.shape and cand_rows.dim() == 2
        B, K = cand_rows.shape
        k, gs = int(k), int(group_size)
        g = self._group_arg(group)
        dev = cand_rows.device
        out_sim = torch.empty((B, max(k, 0), max(gs, 0)), dtype=torch.float32, device=dev)
        out_rows = torch.empty((B, max(k, 0), max(gs, 0)), dtype=torch.int64, device=dev)
        out_group = torch.empty((B, max(k, 0)), dtype=torch.int32, device=dev)
        out_complete = torch.empty((B,), dtype=torch.int32, device=dev)
        N.call("sr_store_group_dev", self._h, N.ptr(cand_rows), N.ptr(cand_sims), B, K, int(row_offset),
               k, gs, N.ptr(g), int(group_key), N.ptr(out_sim), N.ptr(out_rows), N.ptr(out_group),
               N.ptr(out_complete), N.stream_handle(stream))
        return out_sim, out_rows, out_group, out_complete


def group_fetch_k(k: int, group_size: int) -> int:
    """Default rows scanned per round of a grouped search."""
    return min(N.SR_MAX_TOPK, max(4 * int(k) * int(group_size), 64))


def group_walk(sims, rows, group, k: int, group_size: int):
    """The grouped-search walk on the host (ShardedStore's merge): ``sims`` / ``rows`` 1-D candidates
    in any order (row < 0: missing), ``group`` indexed by row.  Rows are taken in (sim desc, row asc)
    order; a row is kept while its group holds fewer than ``group_size`` rows and is a kept group or
    fewer than ``k`` groups are.  Returns (sim [k,g] float64 -inf, rows [k,g] int64 -1, groups [k]
    int32 -1)."""
    sims = np.asarray(sims, dtype=np.float64).reshape(-1)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    ok = rows >= 0
    sims, rows = sims[ok], rows[ok]
    order = np.lexsort((rows, -sims))
    out_s = np.full((k, group_size), -np.inf, dtype=np.float64)
    out_r = np.full((k, group_size), -1, dtype=np.int64)
    out_g = np.full(k, -1, dtype=np.int32)
    seen = {}
    for i in order.tolist():
        r = int(rows[i])
        g = int(group[r])
        key = (r,) if g < 0 else g
        at = seen.get(key)
        if at is None:
            if len(seen) >= k:
                continue
            at = seen[key] = [len(seen), 0]
            out_g[at[0]] = g
        if at[1] < group_size:
            out_s[at[0], at[1]], out_r[at[0], at[1]] = sims[i], r
            at[1] += 1
    return out_s, out_r, out_g


def pack_lists(lists):
    """Row lists -> CSR (list_off [n + 1] int64, list_rows int64), the layout of
    sr_store_search_subset."""
    arrs = [np.asarray(l, dtype=np.int64).reshape(-1) for l in lists]
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    if arrs:
        np.cumsum([a.size for a in arrs], out=off[1:])
    flat = np.ascontiguousarray(np.concatenate(arrs)) if arrs and off[-1] else np.zeros(1, np.int64)
    return off, flat


def mmr_mode(mode) -> int:
    """"onepass" / "greedy" (or the SR_MMR_* code) -> SR_MMR_* code."""
    if isinstance(mode, str):
        try:
            return {"onepass": N.SR_MMR_ONEPASS, "greedy": N.SR_MMR_GREEDY}[mode]
        except KeyError:
            raise ValueError(f"mmr mode must be 'onepass' or 'greedy', got {mode!r}") from None
    return int(mode)


def mmr_rerank(q, cand, n_cand=None, lam: float = 0.5, mode: str = "onepass",
               min_score: float = -2.0, k: int | None = None, device: int = 0):
    """MMR over explicit vectors (graphiti's maximal_marginal_relevance signature, batched):
    q [B, dim], cand [B, K, dim] (host), ``n_cand`` [B] valid candidates per query (None: K).
    Returns (score [B,k] fp32, index [B,k] int32 positions into the candidate list), -inf / -1
    past the end; k defaults to K.  The query is normalised like the candidates
    (sr_mmr_rerank)."""
    qq = np.ascontiguousarray(np.asarray(q, dtype=np.float32))
    c = np.ascontiguousarray(np.asarray(cand, dtype=np.float32))
    if qq.ndim == 1:
        qq, c = qq[None], (c[None] if c.ndim == 2 else c)
    if c.ndim != 3 or c.shape[0] != qq.shape[0] or c.shape[2] != qq.shape[1]:
        raise ValueError(f"expected q (B, dim) and cand (B, K, dim), got {qq.shape} and {c.shape}")
    B, K, dim = c.shape
    k = K if k is None else int(k)
    nc = None
    if n_cand is not None:
        nc = np.ascontiguousarray(np.asarray(n_cand, dtype=np.int32))
        if nc.shape != (B,) or (nc < 0).any() or (nc > K).any():
            raise ValueError(f"n_cand must hold {B} counts in [0, {K}]")
    score = np.empty((B, max(k, 0)), dtype=np.float32)
    index = np.empty((B, max(k, 0)), dtype=np.int32)
    N.call("sr_mmr_rerank", N.ptr(qq), N.ptr(c), N.ptr(nc) if nc is not None else None, B, K, dim,
           float(lam), mmr_mode(mode), float(min_score), k, N.ptr(score), N.ptr(index), int(device))
    return score, index


def topk_merge_dev(sims, rows, k_out: int, device: int = 0, stream=None):
    """Merge [P, B, k] per-shard lists (device tensors) into [B, k_out] (sim desc, row asc)."""
    import torch
    P, B, k = sims.shape
    out_sim = torch.empty((B, k_out), dtype=torch.float32, device=sims.device)
    out_rows = torch.empty((B, k_out), dtype=torch.int64, device=sims.device)
    N.call("sr_topk_merge_dev", N.ptr(sims.contiguous()), N.ptr(rows.contiguous()), P, B, k,
           int(k_out), N.ptr(out_sim), N.ptr(out_rows), int(device), N.stream_handle(stream))
    return out_sim, out_rows


class NativeStoreSet:
    """One collection row-sharded over several devices behind ONE native handle
    (sr_store_set_*, SURVEY §8(b)'s sr_store_create(dim, dtype, devices, n_dev)): the library keeps
    one in-HBM store per listed device, hands out global row ids in insertion order, searches the
    shards concurrently and merges by (distance asc, row asc) — results equal one NativeStore's.
    Host-buffer interface (add / remove / get / count / search with an optional allow mask);
    snapshots, compaction and the device-buffer paths stay with ShardedStore / NativeStore."""

    def __init__(self, dim: int, devices, dtype: str = "fp16"):
        N.require_gpu()
        devs = np.ascontiguousarray(np.asarray(list(devices), dtype=np.int32))
        if devs.size == 0:
            raise ValueError("NativeStoreSet needs at least one device")
        code = {"fp16": N.SR_DTYPE_F16, "fp8": N.SR_DTYPE_FP8_E4M3}[dtype]
        self._h = None
        h = ctypes.c_void_p()
        N.call("sr_store_set_create", int(dim), code, N.ptr(devs), int(devs.size), ctypes.byref(h))
        self._h = h
        self.dim = int(dim)
        self.devices = [int(d) for d in devs]

    def close(self) -> None:
        if self._h:
            N.load().sr_store_set_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, vecs) -> np.ndarray:
        v = np.ascontiguousarray(np.asarray(vecs, dtype=np.float32))
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise ValueError(f"expected (n, {self.dim}) vectors, got {v.shape}")
        rows = np.empty(v.shape[0], dtype=np.int64)
        N.call("sr_store_set_add", self._h, N.ptr(v), int(v.shape[0]), N.ptr(rows))
        return rows

    def remove(self, rows) -> None:
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        N.call("sr_store_set_remove", self._h, N.ptr(r), int(r.size))

    def count(self):
        n, live, sh = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
        N.call("sr_store_set_count", self._h, ctypes.byref(n), ctypes.byref(live), ctypes.byref(sh))
        return int(n.value), int(live.value)

    def get(self, rows) -> np.ndarray:
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        out = np.empty((r.size, self.dim), dtype=np.float32)
        N.call("sr_store_set_get", self._h, N.ptr(r), int(r.size), N.ptr(out))
        return out

    def set_scan_dtype(self, dtype: str) -> None:
        N.call("sr_store_set_set_scan_dtype", self._h,
               {"fp16": N.SR_DTYPE_F16, "fp8": N.SR_DTYPE_FP8_E4M3}[dtype])

    def search(self, queries, k: int, allow=None, mask_key: int = 0):
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        B = q.shape[0]
        dist = np.empty((B, k), dtype=np.float32)
        rows = np.empty((B, k), dtype=np.int64)
        a = None
        if allow is not None:
            n, _ = self.count()
            a = np.ascontiguousarray(np.asarray(allow, dtype=np.uint8))
            if a.shape != (n,):
                raise ValueError(f"allow mask must have {n} entries, got {a.shape}")
        N.call("sr_store_set_search", self._h, N.ptr(q), B, int(k),
               N.ptr(a) if a is not None else None, int(mask_key) if a is not None else 0,
               N.ptr(dist), N.ptr(rows))
        return dist, rows


class ShardedStore:
    """One collection row-sharded over several stores / devices (VECTOR_DB_CONTEXT "devices").

    Same host interface as NativeStore.  Global row ids are the insertion order across all shards
    (exactly the ids one NativeStore would hand out), so results equal a single store's: each add
    batch goes to the shard with the fewest rows (ties: lowest index), a per-shard table maps its
    local rows to global rows.  search() without a filter runs K1 + K2 on every device (each on
    its current stream, so the devices scan concurrently), maps local rows to global rows on the
    device, moves the (B, k) lists to the first device and merges them there with K2 topk_merge
    (sr_topk_merge_dev: similarity desc, global row asc).  Filtered searches run each shard's
    masked search and merge the short lists on the host with the same order.

    ``factory(dim, device)`` builds one shard (NativeStore; test doubles on CPU).
    """

    MAGIC = "SRMISHARDS1"

    def __init__(self, dim: int, devices, factory=None, _shards=None, _tables=None):
        self.dim = int(dim)
        self.devices = [int(d) for d in devices]
        if not self.devices:
            raise ValueError("ShardedStore needs at least one device")
        factory = factory or (lambda d, dev: NativeStore(d, device=dev))
        self.shards = _shards if _shards is not None else [factory(self.dim, d) for d in self.devices]
        self.tables = _tables if _tables is not None else [np.zeros(0, np.int64) for _ in self.devices]
        self._rebuild_index()
        self._dev_tables = None      # per-shard global-row tables on the devices (lazy)

    def _rebuild_index(self) -> None:
        n = sum(len(t) for t in self.tables)
        self.shard_of = np.full(n, -1, np.int32)
        self.local_of = np.full(n, -1, np.int64)
        for s, t in enumerate(self.tables):
            self.shard_of[t] = s
            self.local_of[t] = np.arange(len(t))

    # -- mutation -----------------------------------------------------------------------------------
    def add(self, vecs) -> np.ndarray:
        v = np.ascontiguousarray(np.asarray(vecs, dtype=np.float32))
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise ValueError(f"expected (n, {self.dim}) vectors, got {v.shape}")
        s = int(np.argmin([len(t) for t in self.tables]))
        first = len(self.shard_of)
        local = self.shards[s].add(v)
        if len(local) and int(local[0]) != len(self.tables[s]):
            raise RuntimeError("shard row numbering out of step")
        rows = np.arange(first, first + v.shape[0], dtype=np.int64)
        self.tables[s] = np.concatenate([self.tables[s], rows])
        self.shard_of = np.concatenate([self.shard_of, np.full(len(rows), s, np.int32)])
        self.local_of = np.concatenate([self.local_of, np.asarray(local, np.int64)])
        self._dev_tables = None
        return rows

    def remove(self, rows) -> None:
        r = np.asarray(rows, dtype=np.int64)
        for s in range(len(self.shards)):
            sel = r[self.shard_of[r] == s]
            if sel.size:
                self.shards[s].remove(self.local_of[sel])

    def compact(self) -> np.ndarray:
        n = len(self.shard_of)
        alive = np.zeros(n, bool)
        for s, sh in enumerate(self.shards):
            m = np.asarray(sh.compact())
            keep = m >= 0
            alive[self.tables[s][keep]] = True
            self.tables[s] = self.tables[s][keep]           # new local order = old order
        remap = np.full(n, -1, np.int64)
        remap[alive] = np.arange(int(alive.sum()))
        self.tables = [remap[t] for t in self.tables]
        self._rebuild_index()
        self._dev_tables = None
        return remap

    def set_scan_dtype(self, dtype: str) -> None:
        for sh in self.shards:
            sh.set_scan_dtype(dtype)

    def close(self) -> None:
        for sh in self.shards:
            if hasattr(sh, "close"):
                sh.close()

    # -- queries ------------------------------------------------------------------------------------
    def count(self):
        n = live = 0
        for sh in self.shards:
            a, b = sh.count()
            n, live = n + a, live + b
        return n, live

    def get(self, rows) -> np.ndarray:
        r = np.asarray(rows, dtype=np.int64)
        out = np.empty((r.shape[0], self.dim), dtype=np.float32)
        for s in range(len(self.shards)):
            sel = np.nonzero(self.shard_of[r] == s)[0]
            if sel.size:
                out[sel] = self.shards[s].get(self.local_of[r[sel]])
        return out

    def search(self, queries, k: int, allow=None, mask_key: int = 0):
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        if allow is None and all(hasattr(sh, "search_dev") for sh in self.shards):
            return self._search_device(q, int(k))
        return self._search_host(q, int(k), allow, mask_key)

    def search_sim(self, queries, k: int, allow=None, mask_key: int = 0):
        """search() returning (sim [B,k] fp32 descending, -inf when missing; rows [B,k]): every
        shard's search_sim merged on the host by (similarity desc, global row asc), the single
        store's list bit for bit (search() reports 1 - sim, which cannot be turned back)."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        B, k = q.shape[0], int(k)
        keys, rows = [], []
        for s, sh in enumerate(self.shards):
            a = None if allow is None else np.asarray(allow, dtype=np.uint8)[self.tables[s]]
            sim, r = sh.search_sim(q, k, allow=a, mask_key=mask_key)
            g = np.where(r >= 0, self.tables[s][np.clip(r, 0, None)] if len(self.tables[s]) else -1, -1)
            keys.append(np.where(g >= 0, -np.asarray(sim, np.float64), np.inf))
            rows.append(g)
        out_d, out_r = self._merge_host(keys, rows, B, k)
        return np.where(out_r >= 0, (-out_d).astype(np.float32), -np.inf).astype(np.float32), out_r

    def score_rows(self, queries, rows) -> np.ndarray:
        """NativeStore.score_rows with global rows: every pair goes to the shard that owns its row
        (the routing tables); -inf for a row < 0, outside the collection or tombstoned."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        r = np.asarray(rows, dtype=np.int64)
        if r.ndim != 2 or r.shape[0] != q.shape[0]:
            raise ValueError(f"rows must be [{q.shape[0]}, K], got {r.shape}")
        n = len(self.shard_of)
        ok = (r >= 0) & (r < n)
        safe = np.where(ok, r, 0)
        owner = np.where(ok, self.shard_of[safe] if n else -1, -1)
        out = np.full(r.shape, -np.inf, dtype=np.float32)
        for s, sh in enumerate(self.shards):
            mine = owner == s
            if not mine.any():
                continue
            local = np.where(mine, self.local_of[safe] if n else -1, -1)
            got = np.asarray(sh.score_rows(q, local), dtype=np.float32)
            out[mine] = got[mine]
        return out

    def search_mmr(self, queries, k: int, fetch_k: int, lam: float = 0.5, mode: str = "onepass",
                   min_score: float = -2.0, allow=None, mask_key: int = 0):
        """NativeStore.search_mmr over the shards: the merged top-``fetch_k`` of search(), those
        rows read back with get() (stored rows re-normalise to themselves within fp16 rounding)
        and diversified by mmr_rerank on the first device.  Returns (score, dist, rows)."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        k, fetch_k = int(k), int(fetch_k)
        if not 1 <= k <= fetch_k <= N.SR_MMR_MAX_CAND:
            raise ValueError(f"search_mmr needs 1 <= k <= fetch_k <= {N.SR_MMR_MAX_CAND}, "
                             f"got k={k}, fetch_k={fetch_k}")
        dist, rows = self.search(q, fetch_k, allow=allow, mask_key=mask_key)
        B = q.shape[0]
        ok = rows >= 0
        n_cand = ok.sum(axis=1).astype(np.int32)          # the valid rows are a prefix
        cand = np.zeros((B, fetch_k, self.dim), dtype=np.float32)
        if ok.any():
            cand[ok] = self.get(rows[ok])
        score, index = mmr_rerank(q, cand, n_cand, lam=lam, mode=mode, min_score=min_score, k=k,
                                  device=self.devices[0])
        kept = index >= 0
        pos = np.clip(index, 0, None).astype(np.int64)
        out_rows = np.where(kept, np.take_along_axis(rows, pos, axis=1), -1)
        out_dist = np.where(kept, np.take_along_axis(np.asarray(dist, np.float32), pos, axis=1),
                            np.float32(np.inf)).astype(np.float32)
        return score, out_dist, out_rows

    def search_subset(self, queries, k: int, lists, q_list=None, sim: bool = False):
        """NativeStore.search_subset over the shards: every list is split by shard (local ids stay
        ascending: a shard's table is appended in global order), each shard searches its parts and
        the short lists merge on the host by (similarity desc, global row asc), so the result is
        the single store's."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        B, k = q.shape[0], int(k)
        arrs = [np.asarray(l, dtype=np.int64).reshape(-1) for l in lists]
        n = len(self.shard_of)
        for a in arrs:
            if a.size and (a.min() < 0 or a.max() >= n):
                raise ValueError(f"search_subset: list row outside [0, {n})")
        dists, rows = [], []
        for s, sh in enumerate(self.shards):
            parts = [self.local_of[a[self.shard_of[a] == s]] for a in arrs]
            sm, r = sh.search_subset(q, k, parts, q_list=q_list, sim=True)
            g = np.where(r >= 0, self.tables[s][np.clip(r, 0, None)] if len(self.tables[s]) else -1, -1)
            dists.append(np.where(g >= 0, -np.asarray(sm, np.float64), np.inf))
            rows.append(g)
        out_d, out_r = self._merge_host(dists, rows, B, k)
        ok = out_r >= 0
        s32 = (-out_d).astype(np.float32)
        if sim:
            return np.where(ok, s32, -np.inf).astype(np.float32), out_r
        return np.where(ok, np.float32(1.0) - s32, np.inf).astype(np.float32), out_r

    def search_grouped(self, queries, k: int, group, group_size: int = 1, fetch_k: int | None = None,
                       allow=None, mask_key: int = 0, group_key: int = 0, sim: bool = False):
        """NativeStore.search_grouped over the shards: every shard searches with its slice of the
        group array (global row order), and the per-shard results merge on the host by the same
        walk over their union with global rows.  The merged GROUPS are exact (a group among the
        collection's k best is among the k best of the shard that holds its best row), and so are
        the rows for ``group_size`` 1.  A larger group's later rows may sit in a shard where the group
        is not among the k best, so for ``group_size`` > 1 every query takes a second pass: each
        shard searches only the rows of the query's k groups (an allow mask), which returns every
        shard's best ``group_size`` rows of each of them, and the walk over that union is exact."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != store dim {self.dim}")
        B, k, gs = q.shape[0], int(k), int(group_size)
        n = len(self.shard_of)
        g = np.asarray(group, dtype=np.int32)
        if g.shape != (n,):
            raise ValueError(f"group array must have {n} entries, got {g.shape}")
        sims, rows = [], []
        for s, sh in enumerate(self.shards):
            a = None if allow is None else np.asarray(allow, dtype=np.uint8)[self.tables[s]]
            sm, r, _ = sh.search_grouped(q, k, g[self.tables[s]], group_size=gs, fetch_k=fetch_k,
                                         allow=a, mask_key=mask_key, group_key=group_key, sim=True)
            r = np.asarray(r).reshape(B, -1)
            glob = np.where(r >= 0, self.tables[s][np.clip(r, 0, None)] if len(self.tables[s]) else -1, -1)
            sims.append(np.asarray(sm).reshape(B, -1))
            rows.append(glob)
        S, R = np.concatenate(sims, 1), np.concatenate(rows, 1)
        out_s = np.full((B, k, gs), -np.inf, dtype=np.float32)
        out_r = np.full((B, k, gs), -1, dtype=np.int64)
        out_g = np.full((B, k), -1, dtype=np.int32)
        base = None if allow is None else np.asarray(allow, dtype=np.uint8) != 0
        for b in range(B):
            out_s[b], out_r[b], out_g[b] = group_walk(S[b], R[b], g, k, gs)
            best = out_r[b, :, 0]
            kb = int((best >= 0).sum())
            if gs == 1 or kb == 0:
                continue
            # second pass: only the rows of this query's groups (and its ungrouped kept rows)
            m = np.isin(g, out_g[b][(best >= 0) & (out_g[b] >= 0)])
            m[best[(best >= 0) & (out_g[b] < 0)]] = True
            if base is not None:
                m &= base
            s2, r2 = [], []
            for s, sh in enumerate(self.shards):
                sm, r, _ = sh.search_grouped(q[b:b + 1], kb, g[self.tables[s]], group_size=gs,
                                             fetch_k=fetch_k, allow=m[self.tables[s]], mask_key=0,
                                             group_key=group_key, sim=True)
                r = np.asarray(r).reshape(-1)
                r2.append(np.where(r >= 0, self.tables[s][np.clip(r, 0, None)] if len(self.tables[s]) else -1, -1))
                s2.append(np.asarray(sm).reshape(-1))
            out_s[b], out_r[b], out_g[b] = group_walk(np.concatenate(s2), np.concatenate(r2), g, k, gs)
        if sim:
            return out_s, out_r, out_g
        return (np.where(out_r >= 0, np.float32(1.0) - out_s, np.float32(np.inf)).astype(np.float32),
                out_r, out_g)

    @staticmethod
    def _merge_host(dists, rows, B, k):
        """Per-shard (merge key asc, global row) lists -> the k best per query, ties by row."""
        D, R = np.concatenate(dists, 1), np.concatenate(rows, 1)
        out_d = np.full((B, k), np.inf, D.dtype)
        out_r = np.full((B, k), -1, np.int64)
        for b in range(B):
            big = np.where(R[b] >= 0, R[b], np.iinfo(np.int64).max)
            o = np.lexsort((big, D[b]))[:k]
            out_d[b], out_r[b] = D[b][o], np.where(np.isfinite(D[b][o]), R[b][o], -1)
        return out_d, out_r

    def _search_host(self, q, k, allow, mask_key):
        B = q.shape[0]
        dists, rows = [], []
        # native shards hand back their exact similarities: the merge then orders by similarity as
        # one store does (1 - sim in fp32 can merge two neighbouring similarities into one distance)
        exact = all(hasattr(sh, "search_sim") for sh in self.shards)
        for s, sh in enumerate(self.shards):
            a = None if allow is None else np.asarray(allow, dtype=np.uint8)[self.tables[s]]
            if exact:
                sim, r = sh.search_sim(q, k, allow=a, mask_key=mask_key)
                d = -sim.astype(np.float64)    # merge key; converted back to 1 - sim below
            else:
                d, r = sh.search(q, k, allow=a, mask_key=mask_key) if a is not None else sh.search(q, k)
            d = np.asarray(d)          # the shards' own precision (fp32 from the device)
            g = np.where(r >= 0, self.tables[s][np.clip(r, 0, None)] if len(self.tables[s]) else -1, -1)
            dists.append(np.where(g >= 0, d, np.inf))
            rows.append(g)
        out_d, out_r = self._merge_host(dists, rows, B, k)
        if exact:  # -sim -> 1 - sim in fp32, as the single store reports it
            ok = out_r >= 0
            out_d = np.where(ok, (np.float32(1.0) - (-out_d).astype(np.float32)), np.inf).astype(np.float32)
        return out_d, out_r

    def _search_device(self, q, k):
        import torch
        dev0 = torch.device("cuda", self.devices[0])
        if self._dev_tables is None:
            self._dev_tables = [torch.as_tensor(t, device=torch.device("cuda", d))
                                for t, d in zip(self.tables, self.devices)]
        qh = torch.from_numpy(q)
        sims, rows = [], []
        for sh, d, tab in zip(self.shards, self.devices, self._dev_tables):
            dev = torch.device("cuda", d)
            with torch.cuda.device(dev):
                qd = qh.to(dev, non_blocking=False)
                sim, loc = sh.search_dev(qd, k, stream=torch.cuda.current_stream(dev))
                ok = loc >= 0
                glob = torch.where(ok, tab[loc.clamp_min(0)] if tab.numel() else loc, loc)
                sims.append(torch.where(ok, sim, torch.full_like(sim, float("-inf"))).to(dev0))
                rows.append(glob.to(dev0))
        with torch.cuda.device(dev0):
            s, r = topk_merge_dev(torch.stack(sims), torch.stack(rows), k, device=self.devices[0],
                                  stream=torch.cuda.current_stream(dev0))
            s, r = s.cpu().numpy(), r.cpu().numpy()
        dist = np.where(r >= 0, np.float32(1.0) - s, np.float32(np.inf)).astype(np.float32)
        return dist, np.where(r >= 0, r, -1)

    # -- persistence --------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """<path>: manifest; <path>.s<i>: shard i (store snapshot); <path>.rows.npz: tables."""
        import json
        import os
        for i, sh in enumerate(self.shards):
            sh.save(f"{path}.s{i}")
        np.savez(f"{path}.rows.tmp.npz", **{f"s{i}": t for i, t in enumerate(self.tables)})
        os.replace(f"{path}.rows.tmp.npz", f"{path}.rows.npz")
        with open(path + ".tmp", "w") as f:
            json.dump({"magic": self.MAGIC, "dim": self.dim, "shards": len(self.shards)}, f)
        os.replace(path + ".tmp", path)

    @classmethod
    def is_manifest(cls, path: str) -> bool:
        with open(path, "rb") as f:
            head = f.read(64)
        return cls.MAGIC.encode() in head

    @classmethod
    def load(cls, path: str, devices, loader=None) -> "ShardedStore":
        import json
        with open(path) as f:
            man = json.load(f)
        devices = list(devices)
        if man.get("magic") != cls.MAGIC or len(devices) != int(man["shards"]):
            raise IOError(f"{path}: a {man.get('shards')}-shard collection cannot load on "
                          f"devices {devices}")
        loader = loader or (lambda p, dev: NativeStore.load(p, device=dev))
        shards = [loader(f"{path}.s{i}", d) for i, d in enumerate(devices)]
        with np.load(f"{path}.rows.npz") as z:
            tables = [z[f"s{i}"].astype(np.int64) for i in range(len(devices))]
        return cls(int(man["dim"]), devices, _shards=shards, _tables=tables)
