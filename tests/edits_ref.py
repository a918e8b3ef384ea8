"""Reference definition of the text edits in units (Engine.edits / crdt_edits_async) — TEST
INFRASTRUCTURE.  No Python codec inside: widths and units come from encode_ref.encode_char.

The edits are the diff of tests/diff_ref.py restated in units.  The item walk and the K / D / I / N
classes are ref_diff's, unchanged.  The width w(x) of the item with order x is the number of units
encode_char gives for content[x] under enc (a value that is no scalar value is U+FFFD).  Edit p is
patch p of ref_diff:

  pos, del_len, ins_len   the patch's
  unit        sum of w over the new-visible items before the patch
  del_units   sum of w over its D items
  ins_units   sum of w over its I items
  ins_off     first unit of its inserted text in the pool = sum of ins_units of the earlier edits
  reserved    0

The pool is the concatenation, in patch order, of the encodings of every I item.  Applied front to
back to the encoded text at version v, replacing del_units units at unit (an offset in the text the
earlier edits left) with the edit's ins_units units, the edits give the encoded current text.
"""
import numpy as np

from diff_ref import ref_diff
from encode_ref import BOUNDARY, NOT_SCALAR, UTF8, cycle_text, encode_char


def ref_edits(ex: dict, v: int, content, enc: int):
    """ex: the `canon`, `deletes` and `next_order` tables of an export; content: one value per order.
    Returns (edits [n, 8] u32 = (pos, del_len, ins_len, unit, del_units, ins_units, ins_off, 0),
    pool: np.uint8 (UTF-8) or np.uint16 (UTF-16))."""
    v = int(v)
    patches, ins_order = ref_diff(ex, v)  # (raises for a version outside [0, next_order])
    if len(content) < int(ex["next_order"]):
        raise ValueError("content shorter than the document's orders")
    old_deleted = set()
    for key, target, ln in np.asarray(ex["deletes"], dtype=np.int64).reshape(-1, 3):
        for j in range(int(ln)):
            if key + j < v:
                old_deleted.add(int(target + j))
    edits, pool = [], []
    cur = None       # the open edit
    visible = 0      # new-visible items walked so far
    vis_units = 0    # ... and their units
    for order, _ol, _orr, ln in np.asarray(ex["canon"], dtype=np.uint32).reshape(-1, 4):
        ln = int(np.int32(ln))
        new_vis = ln > 0
        for x in range(int(order), int(order) + abs(ln)):
            old_vis = x < v and x not in old_deleted
            units = encode_char(int(content[x]), enc)
            if old_vis and new_vis:          # K
                cur = None
            elif old_vis or new_vis:         # D or I
                if cur is None:
                    cur = [visible, 0, 0, vis_units, 0, 0, len(pool), 0]
                    edits.append(cur)
                if old_vis:
                    cur[1] += 1
                    cur[4] += len(units)
                else:
                    cur[2] += 1
                    cur[5] += len(units)
                    pool += units
            if new_vis:
                visible += 1
                vis_units += len(units)
    edits = np.array(edits, dtype=np.uint32).reshape(-1, 8)
    # the item columns are the diff's: the walk above is ref_diff's
    assert np.array_equal(edits[:, :3], patches[:, :3])
    assert int(edits[:, 2].sum()) == ins_order.shape[0]
    return edits, np.array(pool, np.uint8 if enc == UTF8 else np.uint16)


def apply_edits(old_units, edits, ins):
    """Apply edits front to back: at unit replace del_units units with ins[ins_off : ins_off + ins_units]."""
    ins = np.asarray(ins)
    out = [int(x) for x in old_units]
    for _pos, _dl, _il, unit, du, iu, off, _r in np.asarray(edits, dtype=np.int64).reshape(-1, 8):
        assert unit + du <= len(out), (unit, du, len(out))
        out[unit:unit + du] = [int(x) for x in ins[off:off + iu]]
    return np.array(out, dtype=ins.dtype)


def mixed_content(n: int, seed: int = 0) -> np.ndarray:
    """n content values: every width of both encodings and values that are no scalar values, in an
    order that does not repeat with the 32-order sample grid (cycle_text runs between random
    picks of encode_ref.BOUNDARY + NOT_SCALAR)"""
    rng = np.random.default_rng(1000 + seed)
    pool = np.array(BOUNDARY + NOT_SCALAR, np.uint32)
    out = cycle_text(n)
    pick = rng.random(n) < 0.4
    out[pick] = rng.choice(pool, int(pick.sum()))
    return out
