"""Reference definition of a document at a past version (Engine.checkout / crdt_checkout_async) —
TEST INFRASTRUCTURE.

A document's version is its next order.  Walk the items of the current state in document order (the
canonical spans, expanded item by item).  An item with order x is old-visible at version v when

  x < v, and no delete-log entry (key, target, len) covers x with a delete order
  key + (x - target) < v  (a delete run that straddles v counts with its part below v).

The document at version v is the sequence of old-visible items in that order: its text is their
code points, its length their count, its position p the p-th of them.  An item with order >= v does
not exist at v.  (The same "old-visible" as tests/diff_ref.py.)
"""
import numpy as np


def ref_checkout(ex: dict, v: int) -> np.ndarray:
    """ex: the `canon`, `deletes` and `next_order` tables of OracleDoc.export() / Engine.export().
    Returns the orders of the old-visible items at version v, in document order (u32)."""
    v = int(v)
    n = int(ex["next_order"])
    if not 0 <= v <= n:
        raise ValueError(f"version {v} outside [0, {n}]")
    old_deleted = np.zeros(n + 1, dtype=bool)  # per item: a delete op with order < v covers it
    for key, target, ln in np.asarray(ex["deletes"], dtype=np.int64).reshape(-1, 3):
        below = min(int(ln), max(0, v - int(key)))  # the run's delete orders key + j < v
        old_deleted[int(target):int(target) + below] = True
    canon = np.asarray(ex["canon"], dtype=np.uint32).reshape(-1, 4)
    first = canon[:, 0].astype(np.int64)
    ln = np.abs(canon[:, 3].astype(np.int32)).astype(np.int64)
    # every item of every span, in document order
    x = np.repeat(first, ln) + (np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln))
    old_vis = (x < v) & ~old_deleted[np.minimum(x, n)]
    return x[old_vis].astype(np.uint32)


def ref_queries_at(order: np.ndarray, ex: dict, v: int):
    """loc -> pos on a view, item by item, from its order list: (pos, deleted) arrays indexed by
    order.  For the order of an insert item below v: the old-visible items before it in document
    order, and 0 (in the view) or 1 (deleted before v).  Any other order (>= v, or a delete op's):
    pos 0xFFFFFFFF, deleted 2."""
    n = int(ex["next_order"])
    canon = np.asarray(ex["canon"], dtype=np.uint32).reshape(-1, 4)
    first = canon[:, 0].astype(np.int64)
    ln = np.abs(canon[:, 3].astype(np.int32)).astype(np.int64)
    x = np.repeat(first, ln) + (np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln))
    in_view = np.zeros(n + 1, dtype=bool)
    in_view[np.asarray(order, dtype=np.int64)] = True
    vis = in_view[x]
    before = np.cumsum(vis) - vis
    pos = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    deleted = np.full(n, 2, dtype=np.uint8)
    known = x < int(v)
    pos[x[known]] = before[known]
    deleted[x[known]] = ~vis[known]
    return pos, deleted
