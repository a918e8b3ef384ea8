"""Reference definition of the patches between two versions of a document (Engine.diff_between /
crdt_diff_between_async) — TEST INFRASTRUCTURE.

A document's version is its next order.  For a version v, an item with order x is visible at v when

  x < v, and no delete-log entry (key, target, len) covers x with a delete order
  key + (x - target) < v  (a delete run that straddles v counts with its part below v):

the "old-visible" of tests/diff_ref.py and tests/checkout_ref.py.  ref_diff_between walks the items
of the current state in document order (the canonical spans, expanded item by item) and calls an
item old if it is visible at `a` and new if it is visible at `b`:

  K (old and new) closes the current patch; D (old only) adds 1 to its del_len; I (new only)
  appends the item to its inserted items; N (neither) is ignored and closes nothing.

A patch is a maximal run of D and I items with no K between them; pos = new items before the run.
Applied front to back, each at its pos in the text the previous ones left, the patches turn the
text at version a into the text at version b, whichever of the two is the later one.  With b = the
current version this is ref_diff(ex, a).  The form is unique: results compare exactly.
"""
import numpy as np


def _deleted_before(ex: dict, v: int) -> set:
    out = set()
    for key, target, ln in np.asarray(ex["deletes"], dtype=np.int64).reshape(-1, 3):
        for j in range(min(int(ln), max(0, v - int(key)))):
            out.add(int(target) + j)
    return out


def ref_diff_between(ex: dict, a: int, b: int):
    """ex: the `canon`, `deletes` and `next_order` tables of OracleDoc.export() / Engine.export().
    Returns (patches [n, 4] u32 = (pos, del_len, ins_len, ins_off), ins_order [n_ins] u32)."""
    a, b = int(a), int(b)
    for v in (a, b):
        if not 0 <= v <= int(ex["next_order"]):
            raise ValueError(f"version {v} outside [0, {int(ex['next_order'])}]")
    del_a, del_b = _deleted_before(ex, a), _deleted_before(ex, b)
    patches, ins = [], []
    cur = None      # the open patch: [pos, del_len, ins_len, ins_off]
    visible = 0     # new items walked so far
    for order, _ol, _orr, ln in np.asarray(ex["canon"], dtype=np.uint32).reshape(-1, 4):
        ln = abs(int(np.int32(ln)))
        for x in range(int(order), int(order) + ln):
            old = x < a and x not in del_a
            new = x < b and x not in del_b
            if old and new:                  # K
                cur = None
            elif old or new:                 # D or I
                if cur is None:
                    cur = [visible, 0, 0, len(ins)]
                    patches.append(cur)
                if old:
                    cur[1] += 1
                else:
                    cur[2] += 1
                    ins.append(x)
            visible += new
    return np.array(patches, dtype=np.uint32).reshape(-1, 4), np.array(ins, dtype=np.uint32)


def _visible_at(ex: dict, x: np.ndarray, v: int) -> np.ndarray:
    n = int(ex["next_order"])
    deleted = np.zeros(n + 1, dtype=bool)
    for key, target, ln in np.asarray(ex["deletes"], dtype=np.int64).reshape(-1, 3):
        deleted[int(target):int(target) + min(int(ln), max(0, v - int(key)))] = True
    return (x < v) & ~deleted[np.minimum(x, n)]


def ref_diff_between_arrays(ex: dict, a: int, b: int):
    """ref_diff_between on whole arrays, for documents of several hundred thousand items (the same
    walk: tests/test_diff_between_ref.py holds the two equal on every pair it samples)."""
    a, b = int(a), int(b)
    for v in (a, b):
        if not 0 <= v <= int(ex["next_order"]):
            raise ValueError(f"version {v} outside [0, {int(ex['next_order'])}]")
    canon = np.asarray(ex["canon"], dtype=np.uint32).reshape(-1, 4)
    first = canon[:, 0].astype(np.int64)
    ln = np.abs(canon[:, 3].astype(np.int32)).astype(np.int64)
    x = np.repeat(first, ln) + (np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln))
    old, new = _visible_at(ex, x, a), _visible_at(ex, x, b)
    new_before = np.cumsum(new) - new
    keep = old | new                      # N items are transparent: drop them
    old, new, x, new_before = old[keep], new[keep], x[keep], new_before[keep]
    content = old != new
    after_k = np.concatenate(([True], ~content[:-1]))  # the item before is a K, or there is none
    start = content & after_k
    pid = np.cumsum(start) - 1            # the patch of every content item
    n_pat = int(start.sum())
    d = old & content
    i = new & content
    del_len = np.bincount(pid[d], minlength=n_pat)
    ins_len = np.bincount(pid[i], minlength=n_pat)
    ins_off = np.cumsum(ins_len) - ins_len
    patches = np.stack([new_before[start], del_len, ins_len, ins_off], axis=1) if n_pat else np.zeros((0, 4))
    return patches.astype(np.uint32).reshape(-1, 4), x[i].astype(np.uint32)
