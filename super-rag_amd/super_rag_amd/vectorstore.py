"""Drop-in vector-store connector: the SeekDB collection replaced by the in-HBM cosine store.

Mirrors SeekDBVectorStoreConnector (super_rag/vectorstore/seekdb_connector.py:31-155):
  * ``__init__(ctx, **kw)`` with ``ctx["collection"]``; ``.store`` is the connector itself
    (embedding_utils.py:95 calls ``connector.store.add``); ``.collection_name``;
  * ``create_collection(vector_size=...)``  (HNSW cosine -> exact cosine, :56-66)
  * ``add(nodes) -> uuid4 string ids``        (:68-85)
  * ``delete(ids=[...])`` / ValueError("ids is required") (:90-96), ``delete_collection()``
  * ``search(QueryWithEmbedding, **kw) -> QueryResult`` with ``score = cosine distance``
    ascending and no ids in the documents (:98-155); the extra kwargs the reference passes
    (limit, score_threshold, filter, search_params, ...) are accepted and ignored, as there.
Opt-in lexical retrieval (ctx ``fulltext``): every added node's text is also indexed for BM25 on
the device (lexical.py, k_lex.hip); ``fulltext_search(text, top_k, keywords)`` backs the
reference's ``fulltext_search`` node type, and ctx ``hybrid`` makes ``search`` fuse the dense and
the BM25 rankings by reciprocal rank on the device (score = rrf score, descending) or, with ctx
``hybrid_fusion`` "relative" / "floor" / "floor_full" and ``hybrid_alpha`` (the weight of the dense side), by their
normalised scores (k_fuse.hip; score = fused score, descending).  Both work on
collections sharded over several devices (ctx ``devices``: lexical.ShardedLex, corpus-wide BM25
statistics), with the same results as one device.
Opt-in diversification (ctx ``diversify="mmr"``, ``mmr_lambda``, ``mmr_mode``, ``mmr_fetch_k``, each
overridable per call by a kwarg of the same name): ``search`` scans the top ``mmr_fetch_k`` rows and
keeps ``top_k`` of them by maximal marginal relevance on the device (k_mmr.hip); results come in MMR
order and ``score`` stays the cosine distance.
Opt-in pre-filtering (ctx ``filter_index=[fields]`` with ``honor_filter``; ``subset_max_rows``): the
collection keeps ``value -> rows`` posting lists of the named metadata fields; a filter with an
equality / $in clause on such a field (filters.plan) is resolved to its row list on the host and
ALL such items of a batch, whatever their filters, go to the device in one search_subset call that
scores only those rows (k_subset.hip) instead of one masked full scan per distinct filter.  Same
results; every other filter, diversified and hybrid / fulltext searches keep the mask path.
Opt-in grouped search (ctx ``group_by=<metadata field>``, ``group_size``, ``group_fetch_k``, each
overridable per call by a kwarg of the same name): ``top_k`` counts GROUPS (distinct values of the
field, e.g. ``document_id``; a row without the field is a group of its own) and ``search`` returns
the ``top_k`` best groups with the ``group_size`` best rows of each, exact, collapsed on the device
(k_group.hip): group by group, best group first, a group's rows by distance ascending, at most
``top_k * group_size`` documents.  Not combinable with ``diversify`` or ``hybrid``.
Collections are process-wide (like a server): every connector object for the same collection
name sees the same rows.  Row ids <-> uuid strings, texts and metadata live on the host; vectors
live in HBM.  With ``ctx["snapshot_dir"]`` a collection is reloaded at construction and
re-snapshotted after every add/delete (checkpoint/resume; SeekDB persisted server-side).
"""
from __future__ import annotations

import asyncio

from array import array
import copy
import json
from collections import OrderedDict
import logging
import os
import threading
import uuid
from typing import Any, Callable, Dict, List, Optional

import numpy as np

from ._native import devices_gate
from .models import DocumentWithScore, QueryResult

logger = logging.getLogger(__name__)

VECTOR_DB_TYPE = "mi355x"
MASK_CACHE_SIZE = 8      # filter masks kept per collection (n_rows bytes each)
SUBSET_MAX_ROWS = 65536  # ctx "subset_max_rows": longest resolved list the subset path takes
SUBSET_CACHE_ROWS = 1 << 22   # resolved row lists kept per collection, by total rows (8 bytes each)


def _native_store(dim: int, device: int):
    from .store import NativeStore
    return NativeStore(dim, device=device)


def _native_load(path: str, device: int):
    from .store import NativeStore
    return NativeStore.load(path, device=device)


def _native_lex(device: int):
    from .lexical import NativeLexIndex
    return NativeLexIndex(device)


def _native_lex_load(path: str, device: int):
    from .lexical import NativeLexIndex
    return NativeLexIndex.load(path, device)


_store_factory: Callable = _native_store
_store_loader: Callable = _native_load
_lex_factory: Callable = _native_lex
_lex_loader: Callable = _native_lex_load


def set_store_backend(factory: Callable, loader: Callable | None = None) -> None:
    """Test seam: replace how per-collection stores are created / loaded."""
    global _store_factory, _store_loader
    _store_factory = factory
    _store_loader = loader or _native_load


def set_lex_backend(factory: Callable, loader: Callable | None = None) -> None:
    """Test seam: replace how per-collection lexical indexes are created / loaded."""
    global _lex_factory, _lex_loader
    _lex_factory = factory
    _lex_loader = loader or _native_lex_load


def _make_store(dim: int, device: int, devices: Optional[List[int]]):
    """One store on `device`, or a ShardedStore over ctx["devices"] (one shard per entry)."""
    if devices and len(devices) > 1:
        from .store import ShardedStore
        return ShardedStore(dim, devices, factory=lambda d, dev: _store_factory(d, dev))
    return _store_factory(dim, devices[0] if devices else device)


def _load_store(path: str, device: int, devices: Optional[List[int]]):
    from .store import ShardedStore
    if ShardedStore.is_manifest(path):
        return ShardedStore.load(path, devices or [device], loader=_store_loader)
    if devices and len(devices) > 1:
        raise IOError(f"{path}: a single-device collection cannot load on devices {devices}")
    return _store_loader(path, devices[0] if devices else device)



def _json_copy(v):
    """Deep copy of JSON-like metadata (dict / list / scalars), ~10x cheaper than copy.deepcopy:
    every returned document owns its metadata, as SeekDB's JSON-decoded results did."""
    if isinstance(v, dict):
        return {k: _json_copy(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_json_copy(x) for x in v]
    if isinstance(v, (str, int, float, bool)) or v is None:
        return v
    return copy.deepcopy(v)


# DocumentWithScore without re-validation for the connector's own, already typed values (text str,
# score float, metadata dict): 100 per request on the per-request path
_make_doc = getattr(DocumentWithScore, "model_construct", DocumentWithScore)

class _Collection:
    def __init__(self, name: str, dim: int, device: int, store=None,
                 devices: Optional[List[int]] = None):
        self.name = name
        self.dim = dim
        self.device = device
        self.devices = devices
        self.store = store if store is not None else _make_store(dim, device, devices)
        self.ids: List[Optional[str]] = []       # row -> uuid (None once deleted)
        self.row_of: Dict[str, int] = {}
        self.texts: List[Optional[str]] = []
        self.metadatas: List[Optional[dict]] = []
        self.lock = threading.RLock()
        self.coalescer = None   # created on first coalesced search (coalesce.py)
        self.text_coalescers: Dict[int, Any] = {}  # encoder id -> fused embed + search batches
        self.version = 0        # bumped on every add / delete / compaction
        # filter -> (version, mask_key, allow mask): a small LRU (each mask is n_rows bytes)
        self.masks: "OrderedDict[str, tuple]" = OrderedDict()
        self.lex = None         # BM25 index over the same rows (ctx "fulltext"), lexical.py
        self.vocab = None
        self.journal = None     # persist.Journal with ctx["snapshot_dir"]
        # ctx "filter_index": field -> {value: array('q') of ascending rows} (hashable scalar values
        # only; tombstoned rows stay listed, the device drops them), None until a connector asks
        self.findex: Optional[Dict[str, Dict[Any, array]]] = None
        self.subset_max_rows = SUBSET_MAX_ROWS
        # filter -> (version, resolved rows or None when the list is too long, the subset_max_rows
        # that decided it): LRU bounded by total rows
        self.subsets: "OrderedDict[str, tuple]" = OrderedDict()
        # ctx "group_by": field -> {"ids": value -> int32 group id (hashable scalar values only),
        # "rows": array('i') group id per row (-1: no such value, a group of its own; a tombstoned
        # row keeps its id), "key" / "arr": serial key and numpy copy of the array the device caches},
        # None until a connector asks
        self.gindex: Optional[Dict[str, dict]] = None

    def ensure_groups(self, field: str) -> None:
        """Keep group ids of a metadata field, back-filling the rows added before."""
        if self.gindex is None:
            self.gindex = {}
        if field not in self.gindex:
            self.gindex[field] = {"ids": {}, "rows": array("i"), "key": 0, "arr": None}
            self.group_rows(self.metadatas, [field])

    def group_rows(self, metadatas, fields=None) -> None:
        """Append the group ids of new rows (in row order) to every grouped field."""
        if self.gindex is None:
            return
        from .filters import indexable
        for f in (self.gindex if fields is None else fields):
            gi = self.gindex[f]
            ids, rows = gi["ids"], gi["rows"]
            for md in metadatas:
                v = md.get(f) if md else None
                if v is not None and indexable(v):
                    g = ids.get(v)
                    if g is None:
                        g = ids[v] = len(ids)
                    rows.append(g)
                else:
                    rows.append(-1)
            gi["arr"] = None

    def remap_groups(self, remap) -> None:
        """Renumber the per-row group ids through a compaction's old -> new row map (the kept rows
        keep their order)."""
        if self.gindex is None:
            return
        keep = np.asarray(remap, dtype=np.int64) >= 0
        for gi in self.gindex.values():
            old = np.array(gi["rows"], dtype=np.int32)
            gi["rows"] = array("i", old[keep[:len(old)]].tolist())
            gi["arr"] = None

    def group_array(self, field: str):
        """(serial key, int32 group id per row) of a grouped field: the key changes with the array,
        so the store reuses its device copy while both are unchanged."""
        gi = self.gindex[field]
        if gi["arr"] is None:
            gi["arr"] = np.array(gi["rows"], dtype=np.int32)
            global _mask_serial
            with _registry_lock:
                _mask_serial += 1
                gi["key"] = _mask_serial
        return gi["key"], gi["arr"]

    def ensure_index(self, fields) -> None:
        """Index the named metadata fields, back-filling the rows added before."""
        new = [f for f in fields if self.findex is None or f not in self.findex]
        if not new:
            return
        if self.findex is None:
            self.findex = {}
        for f in new:
            self.findex[f] = {}
        self.index_rows(0, self.metadatas, new)

    def index_rows(self, first: int, metadatas, fields=None) -> None:
        """Append rows first .. first + len(metadatas) - 1 to the posting lists."""
        if self.findex is None:
            return
        from .filters import indexable
        for f in (self.findex if fields is None else fields):
            posting = self.findex[f]
            for r, md in enumerate(metadatas, first):
                if md:
                    v = md.get(f)
                    if v is not None and indexable(v):
                        p = posting.get(v)
                        if p is None:
                            p = posting[v] = array("q")
                        p.append(r)

    def remap_index(self, remap) -> None:
        """Renumber the posting lists through a compaction's old -> new row map (-1: dropped)."""
        if self.findex is None:
            return
        remap = np.asarray(remap, dtype=np.int64)
        for f, posting in self.findex.items():
            out = {}
            for v, p in posting.items():
                new = remap[np.frombuffer(p, dtype=np.int64)] if len(p) else np.zeros(0, np.int64)
                new = new[new >= 0]
                if new.size:
                    out[v] = array("q", new.tolist())
            self.findex[f] = out
        self.subsets.clear()

    def ensure_lex(self) -> None:
        """Create the lexical index, back-filling the rows added before it existed.  A collection
        sharded over several devices gets a ShardedLex over the same shards."""
        if self.lex is not None:
            return
        from .lexical import ShardedLex, Vocab, analyze
        vocab = Vocab()
        if hasattr(self.store, "shard_of"):
            lex = ShardedLex(self.store, factory=lambda dev: _lex_factory(dev))
        else:
            lex = _lex_factory(self.device)
        if self.ids:
            lex.add([vocab.doc_ids(analyze(t)) if t is not None else [] for t in self.texts])
            dead = [r for r, u in enumerate(self.ids) if u is None]
            if dead:
                lex.remove(np.asarray(dead, dtype=np.int64))
        self.lex, self.vocab = lex, vocab

    # -- checkpoint / resume (persist.py) ----------------------------------------------------------
    def persist_add(self, first_row: int, vecs, ids, texts, metadatas) -> None:
        if self.journal is None:
            return
        if self.journal.gen is None:
            self.journal.checkpoint(self)          # first base of a new collection
        else:
            self.journal.append_add(first_row, vecs, ids, texts, metadatas)

    def persist_delete(self, rows, compacted: bool) -> None:
        if self.journal is None:
            return
        if compacted or self.journal.gen is None:
            self.journal.checkpoint(self)          # rows were renumbered: new base
        else:
            self.journal.append_delete(rows)

    def maybe_checkpoint(self, ratio: float) -> None:
        j = self.journal
        if j is not None and j.gen is not None and \
                j.journal_bytes() > ratio * j.base_bytes() + (64 << 20):
            j.checkpoint(self)

    def _replay(self, rec: dict) -> None:
        if rec["op"] == "add":
            vecs = self.journal.vectors(rec, self.dim)
            rows = self.store.add(vecs)
            if int(rows[0]) != int(rec["row"]) or len(rows) != len(rec["ids"]):
                raise IOError(f"{self.journal.log_path}: add replays at row {int(rows[0])}, "
                              f"journaled at {rec['row']}")
            if self.lex is not None:
                from .lexical import analyze
                self.lex.add([self.vocab.doc_ids(analyze(t)) for t in rec["texts"]])
            self.index_rows(len(self.ids), rec["metadatas"])
            self.group_rows(rec["metadatas"])
            for u, t, m in zip(rec["ids"], rec["texts"], rec["metadatas"]):
                self.row_of[u] = len(self.ids)
                self.ids.append(u)
                self.texts.append(t)
                self.metadatas.append(m)
        elif rec["op"] == "del":
            rows = np.asarray(rec["rows"], dtype=np.int64)
            self.store.remove(rows)
            if self.lex is not None:
                self.lex.remove(rows)
            for r in rows.tolist():
                self.row_of.pop(self.ids[r], None)
                self.ids[r] = self.texts[r] = self.metadatas[r] = None
        else:
            raise IOError(f"{self.journal.log_path}: unknown journal op {rec['op']!r}")

    @classmethod
    def restore(cls, name: str, directory: str, device: int,
                devices: Optional[List[int]] = None) -> Optional["_Collection"]:
        from .persist import Journal
        j = Journal(directory, name)
        meta = j.read_meta()
        if meta is None:
            return None
        gen = meta.get("gen")            # None: the round-1 layout (<name>.srmi, no journal)
        store = _load_store(j.store_path(gen), device, devices)
        n_rows, _ = store.count()
        if n_rows != meta.get("n_rows", len(meta["ids"])) or n_rows != len(meta["ids"]):
            raise IOError(f"snapshot of {name} is inconsistent: {n_rows} stored rows, metadata "
                          f"for {len(meta['ids'])} (generation {gen})")
        c = cls(name, int(meta["dim"]), device, store=store, devices=devices)
        c.ids = meta["ids"]
        c.texts = meta["texts"]
        c.metadatas = meta["metadatas"]
        c.row_of = {u: i for i, u in enumerate(c.ids) if u is not None}
        if "lex_vocab" in meta and os.path.exists(j.lex_path(gen)):
            from .lexical import ShardedLex, Vocab
            if ShardedLex.is_manifest(j.lex_path(gen)):
                if not hasattr(store, "shard_of"):
                    raise IOError(f"{j.lex_path(gen)}: a sharded lexical index for a single-device store")
                c.lex = ShardedLex.load(j.lex_path(gen), store, loader=lambda p, d: _lex_loader(p, d))
            else:
                c.lex = _lex_loader(j.lex_path(gen), device)
            c.vocab = Vocab(meta["lex_vocab"])
        j.gen = gen
        c.journal = j
        for rec in j.records(gen):
            c._replay(rec)
        if gen is None:
            j.checkpoint(c)              # migrate to the journaled layout
        return c


_registry_lock = threading.Lock()
_collections: Dict[str, _Collection] = {}
_mask_serial = 0   # device-mask cache keys (sr_store_search_masked)


def _get(name: str) -> Optional[_Collection]:
    with _registry_lock:
        return _collections.get(name)


class MI355XVectorStoreConnector:
    def __init__(self, ctx: Dict[str, Any], **kwargs: Any):
        self.ctx = ctx
        self.collection_name = ctx["collection"]
        self.vector_size = ctx.get("vector_size", 1024)
        self.distance = ctx.get("distance", "cosine")
        if self.distance != "cosine":
            raise ValueError(f"unsupported distance '{self.distance}' (only cosine)")
        self.device = int(ctx.get("device", os.environ.get("SUPER_RAG_AMD_DEVICE", 0)))
        # ctx "devices": shard the collection's rows over several GPUs (store.ShardedStore)
        devs = ctx.get("devices")
        self.devices = [int(d) for d in devs] if devs else None
        self.snapshot_dir = ctx.get("snapshot_dir")
        self.coalesce = bool(ctx.get("coalesce", True))
        self.max_batch = int(ctx.get("max_batch", 256))
        # opt-in: apply the score_threshold / filter kwargs the reference passes and SeekDB's
        # connector ignores (seekdb_connector.py:99-100).  Off by default = reference behaviour.
        self.honor_score_threshold = bool(ctx.get("honor_score_threshold", False))
        self.honor_filter = bool(ctx.get("honor_filter", False))
        self.compact_ratio = float(ctx.get("compact_ratio", 0.5))
        # opt-in lexical retrieval: BM25 index of the node texts; hybrid = rrf-fused search
        self.hybrid = bool(ctx.get("hybrid", False))
        self.fulltext = bool(ctx.get("fulltext", False)) or self.hybrid
        self.hybrid_k_each = ctx.get("hybrid_k_each")
        self.rrf_rank_const = int(ctx.get("rrf_rank_const", 1))
        # opt-in score fusion (k_fuse.hip): "relative" (min-max of each list), "floor" (cosine from
        # -1, BM25 from 0, dense side completed) or "floor_full" (floor with the BM25 side completed
        # too, lex_score_rows); hybrid_alpha = the weight of the dense side
        from .lexical import check_alpha, fusion_mode
        self.hybrid_fusion = str(ctx.get("hybrid_fusion", "rrf"))
        fusion_mode(self.hybrid_fusion)          # ValueError for an unknown name
        self.hybrid_alpha = check_alpha(ctx.get("hybrid_alpha", 0.5))
        self.scan_dtype = str(ctx.get("scan_dtype", "fp16"))   # "fp8": e4m3 scan + fp16 re-score
        # opt-in diversification: MMR over the top mmr_fetch_k rows on the device (k_mmr.hip);
        # each key can be overridden per call by a search kwarg of the same name
        self.diversify = ctx.get("diversify")
        if self.diversify not in (None, "mmr"):
            raise ValueError(f"unsupported diversify '{self.diversify}' (None or 'mmr')")
        self.mmr_lambda = float(ctx.get("mmr_lambda", 0.5))      # graphiti DEFAULT_MMR_LAMBDA
        self.mmr_mode = str(ctx.get("mmr_mode", "onepass"))
        self.mmr_fetch_k = ctx.get("mmr_fetch_k")                # None: min(128, max(4 top_k, 20))
        if self.hybrid and self.diversify:
            raise ValueError("hybrid and diversify cannot be combined (rrf scores are not cosines)")
        # opt-in pre-filtering: posting lists of these metadata fields; a filter they resolve
        # searches only its rows (one search_subset call per batch).  Needs honor_filter.
        fi = ctx.get("filter_index")
        if isinstance(fi, str):
            fi = [fi]
        self.filter_index = [str(f) for f in fi] if fi and self.honor_filter else None
        self.subset_max_rows = int(ctx.get("subset_max_rows", SUBSET_MAX_ROWS))
        # opt-in grouped search: top_k distinct values of a metadata field with the group_size best
        # rows of each (k_group.hip); each key can be overridden per call by a kwarg of its name
        self.group_by = ctx.get("group_by")
        self.group_size = int(ctx.get("group_size", 1))
        self.group_fetch_k = ctx.get("group_fetch_k")   # None: min(1024, max(4 top_k group_size, 64))
        if self.group_by is not None and self.hybrid:
            raise ValueError("hybrid and group_by cannot be combined (rrf scores are not cosines)")
        if self.group_by is not None and self.diversify:
            raise ValueError("diversify and group_by cannot be combined (MMR order is not a ranking "
                             "to walk)")
        self.checkpoint_ratio = float(ctx.get("checkpoint_ratio", 1.0))
        self.store = self
        if self.snapshot_dir and _get(self.collection_name) is None:
            c = _Collection.restore(self.collection_name, self.snapshot_dir, self.device,
                                    self.devices)
            if c is not None:
                with _registry_lock:
                    _collections.setdefault(self.collection_name, c)
        c = _get(self.collection_name)
        if c is not None:
            self._apply_scan_dtype(c)
            self._apply_filter_index(c)
            self._apply_group_by(c)

    def _apply_group_by(self, c: _Collection) -> None:
        if self.group_by is not None:
            with c.lock:
                c.ensure_groups(str(self.group_by))

    def _apply_filter_index(self, c: _Collection) -> None:
        if self.filter_index:
            with c.lock:
                c.ensure_index(self.filter_index)
                c.subset_max_rows = self.subset_max_rows

    def _apply_scan_dtype(self, c: _Collection) -> None:
        if getattr(c, "scan_dtype", "fp16") != self.scan_dtype and hasattr(c.store, "set_scan_dtype"):
            with c.lock:
                c.store.set_scan_dtype(self.scan_dtype)
                c.scan_dtype = self.scan_dtype

    # -- collection lifecycle ---------------------------------------------------------------------
    def _get_or_create(self, dim: int) -> _Collection:
        with _registry_lock:
            c = _collections.get(self.collection_name)
            if c is None:
                c = _Collection(self.collection_name, int(dim), self.device,
                                devices=self.devices)
                if self.snapshot_dir:
                    from .persist import Journal
                    c.journal = Journal(self.snapshot_dir, self.collection_name)
                _collections[self.collection_name] = c
        self._apply_scan_dtype(c)
        self._apply_filter_index(c)
        self._apply_group_by(c)
        return c

    def create_collection(self, **kwargs: Any):
        vector_size = int(kwargs.get("vector_size") or self.vector_size)
        c = self._get_or_create(vector_size)
        if c.dim != vector_size:
            raise ValueError(f"collection {self.collection_name} exists with dimension {c.dim}, "
                             f"not {vector_size}")

    def delete_collection(self):
        with _registry_lock:
            c = _collections.pop(self.collection_name, None)
        if c is not None and hasattr(c.store, "close"):
            c.store.close()
        if self.snapshot_dir:
            from .persist import Journal
            Journal(self.snapshot_dir, self.collection_name).remove_all()

    # -- mutation ---------------------------------------------------------------------------------
    def add(self, nodes) -> List[str]:
        if not nodes:
            return []
        vecs = np.asarray([n.embedding for n in nodes], dtype=np.float32)
        if vecs.ndim != 2:
            raise ValueError("every node needs an embedding of the same dimension")
        c = self._get_or_create(vecs.shape[1])
        if vecs.shape[1] != c.dim:
            raise ValueError(f"embedding dimension {vecs.shape[1]} != collection dimension {c.dim}")
        ids = [str(uuid.uuid4()) for _ in nodes]
        with c.lock:
            if self.fulltext:
                c.ensure_lex()
            rows = c.store.add(vecs)
            if c.lex is not None:
                from .lexical import analyze
                first = c.lex.add([c.vocab.doc_ids(analyze(n.text)) for n in nodes])
                assert first == int(rows[0]), "lexical index out of step with the store"
            first = len(c.ids)
            for u, r, n in zip(ids, rows, nodes):
                assert int(r) == len(c.ids)
                c.ids.append(u)
                c.row_of[u] = int(r)
                c.texts.append(n.text)
                c.metadatas.append(copy.deepcopy(n.metadata) if n.metadata is not None else None)
            c.index_rows(first, c.metadatas[first:])
            c.group_rows(c.metadatas[first:])
            c.version += 1
            c.persist_add(first, vecs, ids, c.texts[first:], c.metadatas[first:])
            c.maybe_checkpoint(self.checkpoint_ratio)
        logger.debug("Added %d documents to collection %s", len(ids), self.collection_name)
        return ids

    def delete(self, **delete_kwargs: Any):
        ids = delete_kwargs.get("ids")
        if not ids:
            raise ValueError("ids is required")
        c = _get(self.collection_name)
        if c is None:
            return
        with c.lock:
            rows = [c.row_of.pop(u) for u in ids if u in c.row_of]
            if rows:
                c.store.remove(np.asarray(rows, dtype=np.int64))
                if c.lex is not None:
                    c.lex.remove(np.asarray(rows, dtype=np.int64))
                for r in rows:
                    c.ids[r] = None
                    c.texts[r] = None
                    c.metadatas[r] = None
                n_rows, n_live = c.store.count()
                compacted = bool(n_rows and n_live < (1.0 - self.compact_ratio) * n_rows)
                if compacted:
                    self._compact(c)
                c.version += 1
                c.persist_delete(rows, compacted)
                c.maybe_checkpoint(self.checkpoint_ratio)

    def _compact(self, c: _Collection) -> None:
        remap = c.store.compact()
        if c.lex is not None:
            lremap = c.lex.compact()
            assert np.array_equal(np.asarray(lremap), np.asarray(remap)), "lexical remap differs"
        c.remap_index(remap)
        c.remap_groups(remap)
        keep = [i for i, r in enumerate(remap) if r >= 0]
        c.ids = [c.ids[i] for i in keep]
        c.texts = [c.texts[i] for i in keep]
        c.metadatas = [c.metadatas[i] for i in keep]
        c.row_of = {u: i for i, u in enumerate(c.ids)}

    # -- query ------------------------------------------------------------------------------------
    def _mmr_params(self, kwargs, top_k: int):
        """None (diversify off: the search item stays the (q, k, filter) it is today) or the
        (lambda, mode, fetch_k) of this call: ctx keys, each overridden by a kwarg of its name."""
        div = kwargs.get("diversify", self.diversify)
        if div is None:
            return None
        if div != "mmr":
            raise ValueError(f"unsupported diversify '{div}' (None or 'mmr')")
        if self.hybrid:
            raise ValueError("hybrid and diversify cannot be combined (rrf scores are not cosines)")
        from ._native import SR_MMR_MAX_CAND as cap
        lam = float(kwargs.get("mmr_lambda", self.mmr_lambda))
        mode = str(kwargs.get("mmr_mode", self.mmr_mode))
        if mode not in ("onepass", "greedy"):
            raise ValueError(f"mmr_mode must be 'onepass' or 'greedy', got {mode!r}")
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"mmr_lambda must be in [0, 1], got {lam}")
        fetch = kwargs.get("mmr_fetch_k", self.mmr_fetch_k)
        if int(top_k) > cap:
            raise ValueError(f"diversify='mmr': top_k {int(top_k)} exceeds the cap of {cap} candidates")
        if fetch is None:
            fetch = min(cap, max(4 * int(top_k), 20))
        elif int(fetch) > cap:
            raise ValueError(f"diversify='mmr': mmr_fetch_k {int(fetch)} exceeds the cap of {cap} "
                             f"candidates")
        return lam, mode, max(int(fetch), int(top_k))

    def _group_params(self, kwargs, top_k: int):
        """None (group_by off: the search item stays the tuple it is today) or the (field,
        group_size, fetch_k) of this call: ctx keys, each overridden by a kwarg of its name."""
        field = kwargs.get("group_by", self.group_by)
        if field is None:
            return None
        if self.hybrid:
            raise ValueError("hybrid and group_by cannot be combined (rrf scores are not cosines)")
        if kwargs.get("diversify", self.diversify) is not None:
            raise ValueError("diversify and group_by cannot be combined (MMR order is not a ranking "
                             "to walk)")
        from ._native import SR_GROUP_MAX_SIZE, SR_MAX_TOPK as cap
        size = int(kwargs.get("group_size", self.group_size))
        if not 1 <= size <= SR_GROUP_MAX_SIZE:
            raise ValueError(f"group_size must be in [1, {SR_GROUP_MAX_SIZE}], got {size}")
        need = int(top_k) * size
        if need > cap:
            raise ValueError(f"group_by: top_k {int(top_k)} x group_size {size} exceeds the cap of "
                             f"{cap} rows")
        fetch = kwargs.get("group_fetch_k", self.group_fetch_k)
        if fetch is None:
            fetch = min(cap, max(4 * need, 64))
        elif int(fetch) > cap:
            raise ValueError(f"group_by: group_fetch_k {int(fetch)} exceeds the cap of {cap} rows")
        return str(field), size, max(int(fetch), need)

    @staticmethod
    def _item(q, k: int, flt, mmr, grp=None):
        if grp is not None:
            return (q, k, flt, None, grp)
        return (q, k, flt) if mmr is None else (q, k, flt, mmr)

    def search(self, query, **kwargs):
        c = _get(self.collection_name)
        if c is None or query.top_k is None or query.top_k <= 0:
            return QueryResult(query=query.query, results=[])
        q = np.asarray(query.embedding, dtype=np.float32)
        flt = kwargs.get("filter") if self.honor_filter else None
        thr = kwargs.get("score_threshold") if self.honor_score_threshold else None
        grp = self._group_params(kwargs, query.top_k)
        mmr = self._mmr_params(kwargs, query.top_k)
        if self.hybrid:
            # rrf of the dense and the BM25 rankings on the device; score = rrf score (desc)
            return QueryResult(query=query.query,
                               results=self._hybrid(c, q, query.query or "", int(query.top_k), flt))
        if self.coalesce:
            # concurrent single-query searches share one device batch (coalesce.py)
            results = self._coalescer(c)(self._item(q, int(query.top_k), flt, mmr, grp))
        else:
            results = self._search_batch(c, [self._item(q, int(query.top_k), flt, mmr, grp)])[0]
        return QueryResult(query=query.query, results=self._threshold(results, thr))

    async def asearch(self, query, **kwargs):
        """search for a coroutine: a coalesced dense search awaits its device batch without
        holding a worker thread (coalesce.Coalescer.acall); hybrid / uncoalesced searches run
        search in a worker thread.  Same results."""
        c = _get(self.collection_name)
        if c is None or query.top_k is None or query.top_k <= 0 or self.hybrid or not self.coalesce:
            return await asyncio.to_thread(self.search, query, **kwargs)
        q = np.asarray(query.embedding, dtype=np.float32)
        flt = kwargs.get("filter") if self.honor_filter else None
        thr = kwargs.get("score_threshold") if self.honor_score_threshold else None
        grp = self._group_params(kwargs, query.top_k)
        mmr = self._mmr_params(kwargs, query.top_k)
        results = await self._coalescer(c).acall(self._item(q, int(query.top_k), flt, mmr, grp))
        return QueryResult(query=query.query, results=self._threshold(results, thr))

    def can_fuse_embed(self, embedding_model) -> bool:
        """Whether asearch_text applies: a coalescing dense connector and this package's
        coalescing EmbeddingService (its encoder and tokenizer in this process)."""
        # (SUPER_RAG_AMD_FUSE_EMBED_SEARCH=0: the two coalesced steps, for A/B measurements)
        if os.environ.get("SUPER_RAG_AMD_FUSE_EMBED_SEARCH", "1") == "0":
            return False
        return (self.coalesce and not self.hybrid and bool(getattr(embedding_model, "coalesce", False))
                and getattr(embedding_model, "encoder", None) is not None
                and getattr(embedding_model, "tokenizer", None) is not None
                and hasattr(type(embedding_model), "_embed_with"))

    async def asearch_text(self, text: str, embedding_model, top_k: int, **kwargs):
        """embed_query + search of one request as ONE coalesced step: concurrent requests' query
        texts are embedded in one device batch and searched in one device batch, back to back,
        by the same leader (instead of an embed batch and then a separate search batch, whose
        coalescers each saw about half the requests in flight).  Same embedding bits for as long
        as the coalesced batch stays on the short-M GEMM path (the 128 x 128 kernel sums K in the
        same chunks split or not, k_gemm.hip KCHUNK: below 10,753 tokens for bge-base, 336
        queries at S = 32); a larger batch moves GEMMs to the persistent kernel, which sums K in
        one chain, and the embeddings then differ by fp16-level rounding (4e-4 relative measured
        at S = 512), each within 1e-3 of the oracle (tests/test_gpu_encoder.py).  Same search, same errors (EmptyTextError before anything
        runs, BatchProcessingError for a failed device batch)."""
        from .errors import EmptyTextError
        if not text or not text.strip():
            raise EmptyTextError(1)
        c = _get(self.collection_name)
        if c is None or top_k is None or top_k <= 0:
            await embedding_model.aembed_query(text)
            return QueryResult(query=text, results=[])
        flt = kwargs.get("filter") if self.honor_filter else None
        thr = kwargs.get("score_threshold") if self.honor_score_threshold else None
        grp = self._group_params(kwargs, top_k)
        item = self._item(text.replace("\n", " "), int(top_k), flt, self._mmr_params(kwargs, top_k), grp)
        results = await self._text_coalescer(c, embedding_model).acall(item)
        return QueryResult(query=text, results=self._threshold(results, thr))

    def _text_coalescer(self, c, em):
        key = id(em.encoder)
        co = c.text_coalescers.get(key)
        if co is None:
            with c.lock:
                co = c.text_coalescers.get(key)
                if co is None:
                    from .coalesce import Coalescer
                    enc, tok, dev_b = em.encoder, em.tokenizer, em.device_batch
                    embed_with = type(em)._embed_with

                    def run(items, c=c):
                        vecs = embed_with(enc, tok, dev_b, [it[0] for it in items])
                        return self._search_batch(c, [(vecs[i],) + tuple(it[1:]) for i, it in enumerate(items)])
                    co = Coalescer(run, max_batch=min(self.max_batch, dev_b))
                    c.text_coalescers[key] = co
        return co

    def _coalescer(self, c):
        if c.coalescer is None:
            with c.lock:
                if c.coalescer is None:
                    from .coalesce import Coalescer
                    c.coalescer = Coalescer(lambda items, c=c: self._search_batch(c, items),
                                            max_batch=self.max_batch)
        return c.coalescer

    @staticmethod
    def _threshold(results, thr):
        if thr is None:
            return results
        # similarity = 1 - distance >= threshold (a filter, not a prefix cut: diversified results
        # come in MMR order, not by distance)
        return [d for d in results if 1.0 - d.score >= float(thr)]

    @staticmethod
    def _allow_mask(c: _Collection, flt):
        """(mask_key, allow[n_rows]) for a filter, cached per collection version."""
        from .filters import canonical, matches
        key = canonical(flt)
        hit = c.masks.get(key)
        if hit is not None and hit[0] == c.version:
            c.masks.move_to_end(key)
            return hit[1], hit[2]
        allow = np.fromiter((u is not None and matches(flt, md)
                             for u, md in zip(c.ids, c.metadatas)), dtype=np.uint8, count=len(c.ids))
        global _mask_serial
        with _registry_lock:
            _mask_serial += 1
            mkey = _mask_serial
        c.masks[key] = (c.version, mkey, allow)
        c.masks.move_to_end(key)
        for k in [k for k, v in c.masks.items() if v[0] != c.version]:
            del c.masks[k]                      # stale: the rows changed since
        while len(c.masks) > MASK_CACHE_SIZE:
            c.masks.popitem(last=False)
        return mkey, allow

    @staticmethod
    def _subset_rows(c: _Collection, flt):
        """The ascending rows a filter resolves to through the field index (filters.plan, its
        remaining clauses checked with ``matches`` on the posting list's rows only), or None when
        the filter is not resolvable or its list exceeds subset_max_rows.  Cached per filter and
        collection version; the cache is bounded by its total rows."""
        from .filters import canonical, matches, plan
        key = canonical(flt)
        hit = c.subsets.get(key)
        if hit is not None and hit[0] == c.version and hit[2] == c.subset_max_rows:
            c.subsets.move_to_end(key)
            return hit[1]
        got = plan(flt, c.findex)
        if got is None:
            return None
        rows, rest = got
        if rest:
            md = c.metadatas
            rows = rows[np.fromiter((matches(rest, md[r]) for r in rows.tolist()), dtype=bool,
                                    count=len(rows))]
        if len(rows) > c.subset_max_rows:
            rows = None
        for k in [k for k, v in c.subsets.items() if v[0] != c.version]:
            del c.subsets[k]                    # stale: the rows changed since
        c.subsets[key] = (c.version, rows, c.subset_max_rows)
        c.subsets.move_to_end(key)
        total = sum(len(v[1]) for v in c.subsets.values() if v[1] is not None)
        while total > SUBSET_CACHE_ROWS and len(c.subsets) > 1:
            _, old = c.subsets.popitem(last=False)
            total -= 0 if old[1] is None else len(old[1])
        return rows

    @staticmethod
    def _has_subset(store) -> bool:
        shards = getattr(store, "shards", None)
        if shards is not None:
            return all(hasattr(sh, "search_subset") for sh in shards)
        return hasattr(store, "search_subset")

    @staticmethod
    def _has_grouped(store) -> bool:
        shards = getattr(store, "shards", None)
        if shards is not None:
            return all(hasattr(sh, "search_grouped") for sh in shards)
        return hasattr(store, "search_grouped")

    @staticmethod
    def _search_batch(c: _Collection, items) -> List[List[DocumentWithScore]]:
        """[(query vector, top_k, filter[, (mmr lambda, mode, fetch_k)[, (group field, group_size,
        fetch_k)]])] -> per query [DocumentWithScore] (distance asc, MMR order for a diversified
        item, group by group for a grouped one; no ids).  With a field index, every undiversified,
        ungrouped item whose filter resolves to a row list goes to the store in ONE search_subset
        call (items with the same filter share a list); the other queries share one device search
        per filter and MMR / grouping setting."""
        out: List[List[DocumentWithScore]] = [[] for _ in items]
        groups: Dict[tuple, list] = {}
        with c.lock:
            sub_idx, sub_list, lists, list_of = [], [], [], {}
            use_subset = c.findex is not None and MI355XVectorStoreConnector._has_subset(c.store)
            for i, it in enumerate(items):
                flt = it[2]
                fkey = "" if flt is None else json.dumps(flt, sort_keys=True, default=str)
                mmr = it[3] if len(it) > 3 else None
                grp = it[4] if len(it) > 4 else None
                if use_subset and flt is not None and mmr is None and grp is None:
                    li = list_of.get(fkey)
                    if li is None:
                        rows = MI355XVectorStoreConnector._subset_rows(c, flt)
                        li = list_of[fkey] = -1 if rows is None else len(lists)
                        if rows is not None:
                            lists.append(rows)
                    if li >= 0:
                        sub_idx.append(i)
                        sub_list.append(li)
                        continue
                groups.setdefault((fkey, mmr) if grp is None else (fkey, mmr, grp), []).append(i)
            if sub_idx:
                Q = np.stack([np.asarray(items[i][0], dtype=np.float32).reshape(-1) for i in sub_idx])
                kmax = max(items[i][1] for i in sub_idx)
                with devices_gate(_store_devices(c.store), "search"):
                    dist, rows = c.store.search_subset(Q, kmax, lists,
                                                       q_list=np.asarray(sub_list, dtype=np.int32))
                for j, i in enumerate(sub_idx):
                    k = items[i][1]
                    out[i] = [_make_doc(text=c.texts[r], score=float(d),
                                        metadata=_json_copy(c.metadatas[r]))
                              for d, r in zip(dist[j, :k].tolist(), rows[j, :k].tolist()) if r >= 0]
            for gkey_, idx in groups.items():
                key, mmr = gkey_[0], gkey_[1]
                grp = gkey_[2] if len(gkey_) > 2 else None
                Q = np.stack([np.asarray(items[i][0], dtype=np.float32).reshape(-1) for i in idx])
                kmax = max(items[i][1] for i in idx)
                allow, mkey = None, 0
                if key != "":
                    mkey, allow = MI355XVectorStoreConnector._allow_mask(c, items[idx[0]][2])
                if grp is not None:
                    field, size, fetch_k = grp
                    if not MI355XVectorStoreConnector._has_grouped(c.store):
                        raise RuntimeError(f"group_by needs a store with search_grouped; "
                                           f"{type(c.store).__name__} has none")
                    c.ensure_groups(field)
                    gkey, garr = c.group_array(field)
                    with devices_gate(_store_devices(c.store), "search"):
                        dist, rows, _ = c.store.search_grouped(
                            Q, kmax, garr, group_size=size, fetch_k=max(fetch_k, kmax * size),
                            allow=allow, mask_key=mkey, group_key=gkey)
                    # [B, k, g] -> the first k groups, group by group (rows of a group: distance asc)
                    dist = np.asarray(dist).reshape(len(idx), -1)
                    rows = np.asarray(rows).reshape(len(idx), -1)
                    for j, i in enumerate(idx):
                        n_out = items[i][1] * size
                        out[i] = [_make_doc(text=c.texts[r], score=float(d),
                                            metadata=_json_copy(c.metadatas[r]))
                                  for d, r in zip(dist[j, :n_out].tolist(), rows[j, :n_out].tolist())
                                  if r >= 0]
                    continue
                if mmr is not None:
                    lam, mode, fetch_k = mmr
                    with devices_gate(_store_devices(c.store), "search"):
                        _, dist, rows = c.store.search_mmr(Q, kmax, fetch_k, lam=lam, mode=mode,
                                                           allow=allow, mask_key=mkey)
                elif key == "":
                    with devices_gate(_store_devices(c.store), "search"):
                        dist, rows = c.store.search(Q, kmax)
                else:
                    with devices_gate(_store_devices(c.store), "search"):
                        dist, rows = c.store.search(Q, kmax, allow=allow, mask_key=mkey)
                for j, i in enumerate(idx):
                    k = items[i][1]
                    out[i] = [_make_doc(text=c.texts[r], score=float(d),
                                        metadata=_json_copy(c.metadatas[r]))
                              for d, r in zip(dist[j, :k].tolist(), rows[j, :k].tolist()) if r >= 0]
        return out

    def _hybrid(self, c: _Collection, q, text: str, k: int, flt) -> List[DocumentWithScore]:
        from .lexical import analyze
        with c.lock:
            c.ensure_lex()
            terms = c.vocab.query_ids(analyze(text))
            k_each = int(self.hybrid_k_each or max(k, 4 * k))
            k_each = min(k_each, 1024)
            k = min(k, 2 * k_each)
            allow, mkey = None, 0
            if flt is not None:
                mkey, allow = self._allow_mask(c, flt)
            with devices_gate(_store_devices(c.store), "search"):
                # (the default passes no fusion keyword: the rrf call is the one it always was)
                fuse = {} if self.hybrid_fusion == "rrf" else {"fusion": self.hybrid_fusion,
                                                               "alpha": self.hybrid_alpha}
                scores, rows = c.lex.hybrid(c.store, q.reshape(1, -1), [terms], k, k_each,
                                            self.rrf_rank_const, allow=allow, mask_key=mkey, **fuse)
            return [_make_doc(text=c.texts[r], score=float(s), metadata=_json_copy(c.metadatas[r]))
                    for s, r in zip(scores[0].tolist(), rows[0].tolist()) if r >= 0]

    def fulltext_search(self, query_text: str, top_k: int, keywords: Optional[List[str]] = None,
                        **kwargs: Any) -> List[DocumentWithScore]:
        """BM25 top-k over the collection's texts (the reference's ``fulltext_search`` node,
        FulltextSearchParams{topk, keywords}); score = BM25 score, descending.  ``keywords``, when
        given, replace the query text's terms.  kwargs ``filter`` is honoured with
        ctx["honor_filter"], as in search()."""
        c = _get(self.collection_name)
        if c is None or top_k is None or top_k <= 0:
            return []
        from .lexical import analyze
        text = " ".join(keywords) if keywords else (query_text or "")
        flt = kwargs.get("filter") if self.honor_filter else None
        with c.lock:
            c.ensure_lex()
            terms = c.vocab.query_ids(analyze(text))
            if not terms:
                return []
            allow, mkey = None, 0
            if flt is not None:
                mkey, allow = self._allow_mask(c, flt)
            with devices_gate(_store_devices(c.store), "search"):
                scores, rows = c.lex.search([terms], min(int(top_k), 1024), allow=allow,
                                            mask_key=mkey)
            return [_make_doc(text=c.texts[r], score=float(s), metadata=_json_copy(c.metadatas[r]))
                    for s, r in zip(scores[0].tolist(), rows[0].tolist()) if r >= 0]

    def get_vectors(self, ids: List[str]) -> np.ndarray:
        """Stored (normalised, fp16-rounded) vectors for uuids (with_vectors=True support)."""
        c = _get(self.collection_name)
        if c is None:
            raise KeyError(self.collection_name)
        with c.lock:
            return c.store.get(np.asarray([c.row_of[u] for u in ids], dtype=np.int64))


def _store_devices(store) -> List[int]:
    """The devices a collection's store computes on: every shard's for a ShardedStore (its
    searches run on all of them), else the store's one device."""
    devs = getattr(store, "devices", None)
    return list(devs) if devs else [int(getattr(store, "device", 0))]


class VectorStoreConnectorAdaptor:
    """vectorstore/connector.py:4-15 with the ``"mi355x"`` arm."""

    def __init__(self, vector_store_type, ctx: Dict[str, Any], **kwargs: Any) -> None:
        self.ctx = ctx
        self.vector_store_type = vector_store_type
        if vector_store_type == VECTOR_DB_TYPE:
            self.connector = MI355XVectorStoreConnector(ctx, **kwargs)
        else:
            raise ValueError("unsupported vector store type:", vector_store_type)
