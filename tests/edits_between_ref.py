"""Reference definition of the edits in units between two versions of a document
(Engine.edits_between / crdt_edits_between_async) — TEST INFRASTRUCTURE.  No Python codec inside:
widths and units come from encode_ref.encode_char.

The edits are the two-version diff of tests/diff_between_ref.py restated in units, as
tests/edits_ref.py restates tests/diff_ref.py.  The item walk and the K / D / I / N classes are
ref_diff_between's: an item is old when it is visible at `a` and new when it is visible at `b`.  The
width w(x) of the item with order x is the number of units encode_char gives for content[x] under
enc (a value that is no scalar value is U+FFFD).  Edit p is patch p of ref_diff_between:

  pos, del_len, ins_len   the patch's
  unit        sum of w over the new items before the patch
  del_units   sum of w over its D items
  ins_units   sum of w over its I items
  ins_off     first unit of its inserted text in the pool = sum of ins_units of the earlier edits
  reserved    0

The pool is the concatenation, in patch order, of the encodings of every I item.  Applied front to
back to the encoded text at version a (edits_ref.apply_edits), the edits give the encoded text at
version b, whichever of the two is the later one.  With b = the current version this is
ref_edits(ex, a, content, enc).
"""
import numpy as np

from diff_between_ref import _deleted_before, _visible_at, ref_diff_between, ref_diff_between_arrays
from encode_ref import UTF8, encode_char


def ref_edits_between(ex: dict, a: int, b: int, content, enc: int):
    """ex: the `canon`, `deletes` and `next_order` tables of an export; content: one value per order.
    Returns (edits [n, 8] u32 = (pos, del_len, ins_len, unit, del_units, ins_units, ins_off, 0),
    pool: np.uint8 (UTF-8) or np.uint16 (UTF-16))."""
    a, b = int(a), int(b)
    patches, ins_order = ref_diff_between(ex, a, b)  # (raises for a version outside [0, next_order])
    if len(content) < int(ex["next_order"]):
        raise ValueError("content shorter than the document's orders")
    del_a, del_b = _deleted_before(ex, a), _deleted_before(ex, b)
    edits, pool = [], []
    cur = None       # the open edit
    visible = 0      # new items walked so far
    vis_units = 0    # ... and their units
    for order, _ol, _orr, ln in np.asarray(ex["canon"], dtype=np.uint32).reshape(-1, 4):
        ln = abs(int(np.int32(ln)))
        for x in range(int(order), int(order) + ln):
            old = x < a and x not in del_a
            new = x < b and x not in del_b
            units = encode_char(int(content[x]), enc)
            if old and new:                  # K
                cur = None
            elif old or new:                 # D or I
                if cur is None:
                    cur = [visible, 0, 0, vis_units, 0, 0, len(pool), 0]
                    edits.append(cur)
                if old:
                    cur[1] += 1
                    cur[4] += len(units)
                else:
                    cur[2] += 1
                    cur[5] += len(units)
                    pool += units
            if new:
                visible += 1
                vis_units += len(units)
    edits = np.array(edits, dtype=np.uint32).reshape(-1, 8)
    # the item columns are the two-version diff's: the walk above is ref_diff_between's
    assert edits.shape[0] == patches.shape[0] and np.array_equal(edits[:, :3], patches[:, :3])
    assert int(edits[:, 2].sum()) == ins_order.shape[0]
    return edits, np.array(pool, np.uint8 if enc == UTF8 else np.uint16)


def _widths(content, enc: int) -> np.ndarray:
    """encode_char's width of every content value, on the whole array"""
    c = np.asarray(content, dtype=np.uint32).astype(np.int64)
    c = np.where((c < 0xD800) | ((c >= 0xE000) & (c <= 0x10FFFF)), c, 0xFFFD)
    if enc == UTF8:
        return 1 + (c >= 0x80) + (c >= 0x800) + (c >= 0x10000)
    return 1 + (c >= 0x10000)


def ref_edits_between_arrays(ex: dict, a: int, b: int, content, enc: int):
    """ref_edits_between on whole arrays, for documents of several hundred thousand items (the same
    walk: tests/test_edits_between_ref.py holds the two equal on every pair it samples)."""
    a, b = int(a), int(b)
    patches, ins_order = ref_diff_between_arrays(ex, a, b)
    n = int(ex["next_order"])
    if len(content) < n:
        raise ValueError("content shorter than the document's orders")
    content = np.asarray(content, dtype=np.uint32)
    canon = np.asarray(ex["canon"], dtype=np.uint32).reshape(-1, 4)
    first = canon[:, 0].astype(np.int64)
    ln = np.abs(canon[:, 3].astype(np.int32)).astype(np.int64)
    x = np.repeat(first, ln) + (np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln))
    w = _widths(content, enc)[x]
    old, new = _visible_at(ex, x, a), _visible_at(ex, x, b)
    new_units_before = np.cumsum(w * new) - w * new
    keep = old | new
    old, new, w, new_units_before = old[keep], new[keep], w[keep], new_units_before[keep]
    change = old != new
    start = change & np.concatenate(([True], ~change[:-1]))
    pid = np.cumsum(start) - 1
    n_pat = int(start.sum())
    assert n_pat == patches.shape[0]
    d, i = old & change, new & change
    du = np.bincount(pid[d], weights=w[d], minlength=n_pat).astype(np.int64)
    iu = np.bincount(pid[i], weights=w[i], minlength=n_pat).astype(np.int64)
    edits = np.zeros((n_pat, 8), np.int64)
    edits[:, :3] = patches[:, :3]
    edits[:, 3] = new_units_before[start]
    edits[:, 4] = du
    edits[:, 5] = iu
    edits[:, 6] = np.cumsum(iu) - iu
    pool = []
    for c in content[ins_order]:
        pool += encode_char(int(c), enc)
    return edits.astype(np.uint32), np.array(pool, np.uint8 if enc == UTF8 else np.uint16)

