"""Metadata filter evaluation for the vector store's opt-in filtered search.

The reference builds SeekDB-style filter dicts in ContextManager._create_combined_filter
(context/context.py:74-111), e.g.
    {"and": [{"or": [{"indexer": {"$in": ["vector"]}}, {"indexer": {"$exists": False}}]},
             {"chat_id": "c1"}]}
and passes them to the connector, which ignores them (seekdb_connector.py:99-100).  With
``ctx["honor_filter"]`` the MI355X connector applies them: rows whose metadata does not match are
excluded from the device search (sr_store_search_masked), so a query still gets its k best
matching rows.  Supported: and / or / not (with or without "$"), field equality and the operators
$eq $ne $in $nin $exists $gt $gte $lt $lte $contains; a list of clauses is a conjunction.
"""
from __future__ import annotations

import json
from typing import Any, Mapping

_MISSING = object()


def canonical(flt: Any) -> str:
    """Stable cache key of a filter."""
    return json.dumps(flt, sort_keys=True, default=str)


def _field(cond: Any, val: Any) -> bool:
    present = val is not _MISSING
    if not isinstance(cond, Mapping):
        return present and val == cond
    for op, arg in cond.items():
        if op == "$eq":
            ok = present and val == arg
        elif op == "$ne":
            ok = not (present and val == arg)
        elif op == "$in":
            ok = present and val in arg
        elif op == "$nin":
            ok = not (present and val in arg)
        elif op == "$exists":
            ok = present == bool(arg)
        elif op in ("$gt", "$gte", "$lt", "$lte"):
            try:
                ok = present and {"$gt": val > arg, "$gte": val >= arg,
                                  "$lt": val < arg, "$lte": val <= arg}[op]
            except TypeError:
                ok = False
        elif op == "$contains":
            try:
                ok = present and arg in val
            except TypeError:
                ok = False
        else:
            raise ValueError(f"unsupported filter operator {op!r}")
        if not ok:
            return False
    return True


def indexable(v: Any) -> bool:
    """Values a field index keeps: hashable scalars, for which a dict lookup is the ``==`` of
    _field (1 == 1.0 == True share a key, as they compare equal).  NaN equals nothing, itself
    included, so it is left to ``matches``."""
    return isinstance(v, (str, int, float, bool)) and v == v


def _conjuncts(flt: Any):
    """The clauses ``matches`` ANDs together: a clause list, and / $and and the keys of one mapping,
    flattened; every returned clause is a one-key mapping.  None: not a filter ``matches`` accepts
    (left to it to report)."""
    if isinstance(flt, (list, tuple)):
        parts = [_conjuncts(c) for c in flt]
    elif isinstance(flt, Mapping):
        parts = []
        for key, cond in flt.items():
            if key in ("and", "$and"):
                if not isinstance(cond, (list, tuple)):
                    return None
                parts.extend(_conjuncts(c) for c in cond)
            else:
                parts.append([{key: cond}])
    else:
        return None
    if any(p is None for p in parts):
        return None
    return [c for p in parts for c in p]


def _clause_values(clause: Mapping, index: Mapping):
    """(values, exact) when the clause is ``field: scalar``, ``{"$eq": scalar}`` or
    ``{"$in": [scalars]}`` on an indexed field: the clause holds only for rows in the union of those
    values' posting lists, and for all of them when ``exact`` (no further operator in the clause)."""
    (key, cond), = clause.items()
    if key in ("or", "$or", "not", "$not") or key not in index:
        return None
    if not isinstance(cond, Mapping):
        return ([cond], True) if indexable(cond) else None
    if "$eq" in cond and indexable(cond["$eq"]):
        return [cond["$eq"]], len(cond) == 1
    arg = cond.get("$in")
    if isinstance(arg, (list, tuple)) and all(indexable(v) for v in arg):
        return list(arg), len(cond) == 1
    return None


def plan(flt: Any, index: Mapping):
    """Resolve a filter through a field index ``{field: {value: ascending rows}}``.

    Returns None when no conjunct of the filter is an equality / $in clause on an indexed field
    (the filter then takes the mask path), else ``(rows, rest)``: ``rows`` (ascending int64) is
    the shortest posting list, or union of an $in's lists, among those clauses, a superset of the
    matching rows; ``rest`` is the list of conjuncts still to be checked with ``matches`` on those
    rows only (empty: ``rows`` is the answer)."""
    import numpy as np
    clauses = _conjuncts(flt) if flt is not None else None
    if not clauses:
        return None
    best = None
    for i, cl in enumerate(clauses):
        got = _clause_values(cl, index)
        if got is None:
            continue
        values, exact = got
        posting = index[next(iter(cl))]
        parts, seen = [], set()
        for v in values:
            if v not in seen:           # (1 and 1.0 name one posting list)
                seen.add(v)
                p = posting.get(v)
                if p is not None and len(p):
                    parts.append(p)
        size = sum(len(p) for p in parts)
        if best is None or size < best[0]:
            best = (size, i, parts, exact)
    if best is None:
        return None
    _, i, parts, exact = best
    if not parts:
        rows = np.zeros(0, np.int64)
    elif len(parts) == 1:
        rows = np.array(parts[0], dtype=np.int64)
    else:
        rows = np.unique(np.concatenate([np.asarray(p, dtype=np.int64) for p in parts]))
    rest = [c for j, c in enumerate(clauses) if j != i or not exact]
    return rows, rest


def matches(flt: Any, metadata: Mapping | None) -> bool:
    """Does a row's metadata satisfy the filter?  ``None`` matches everything."""
    if flt is None:
        return True
    md = metadata or {}
    if isinstance(flt, (list, tuple)):
        return all(matches(c, md) for c in flt)
    if not isinstance(flt, Mapping):
        raise ValueError(f"unsupported filter {flt!r}")
    for key, cond in flt.items():
        if key in ("and", "$and"):
            ok = all(matches(c, md) for c in cond)
        elif key in ("or", "$or"):
            ok = any(matches(c, md) for c in cond)
        elif key in ("not", "$not"):
            ok = not matches(cond, md)
        else:
            ok = _field(cond, md.get(key, _MISSING))
        if not ok:
            return False
    return True
