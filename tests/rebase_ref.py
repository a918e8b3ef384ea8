"""Reference definition of the rebase map (Engine.rebase_async / crdt_rebase_async and its queries) —
TEST INFRASTRUCTURE.

The map of an index is built from its patches (tests/diff_ref.py) or edits (tests/edits_ref.py), one
span (old_at, old_len, new_at, new_len) per patch, in patch order:

  new_at = pos       new_len = ins_len       old_len = del_len
  old_at = pos - (ins_len of the earlier patches) + (del_len of the earlier patches)

old_at is where the patch starts in the old text: every earlier patch moved what follows it by its
ins_len - del_len.  The units table is the same with (unit, del_units, ins_units) of the edits.

A query maps a cursor position x (the gap before item x) of the source side's text.  OLD_TO_NEW
reads a span as (a, la, b, lb) = (old_at, old_len, new_at, new_len), NEW_TO_OLD as (new_at, new_len,
old_at, old_len).  With k the last span whose a <= x:

  no such span          y = x                             hit 0
  x > a + la            y = x - (a + la) + (b + lb)       hit 0
  otherwise             y = b if side < 0 else b + lb     hit 1 iff a < x < a + la

  side = bias (LEFT -1, RIGHT +1) when la == 0; else -1 at x == a, +1 at x == a + la, bias inside.

x is not checked against a text's length; answers are taken modulo 2^32.
"""
import numpy as np

OLD_TO_NEW, NEW_TO_OLD = 0, 1
LEFT, RIGHT = 0, 1
M32 = 0xFFFFFFFF


def ref_rebase_table(patches_or_edits, units: bool = False) -> np.ndarray:
    """patches [n, 4] u32 (pos, del_len, ins_len, ins_off) or edits [n, 8] u32 (pos, del_len,
    ins_len, unit, del_units, ins_units, ins_off, 0); units=True takes the edits' unit columns.
    Returns the spans [n, 4] u32 = (old_at, old_len, new_at, new_len)."""
    rows = np.asarray(patches_or_edits, dtype=np.int64)
    rows = rows.reshape(-1, rows.shape[-1] if rows.ndim == 2 else 4)
    if units and rows.shape[1] != 8:
        raise ValueError("the unit table needs edits")
    cols = (3, 4, 5) if units else (0, 1, 2)
    out = []
    shift = 0  # ins - del of the patches walked so far: new position - old position after them
    for row in rows:
        at, dl, il = (int(row[c]) for c in cols)
        out.append([(at - shift) & M32, dl, at, il])
        shift += il - dl
    return np.array(out, dtype=np.uint32).reshape(-1, 4)


def ref_rebase(table, x: int, dir: int = OLD_TO_NEW, bias: int = RIGHT):
    """(y, hit) for one position, span by span"""
    x = int(x)
    last = None
    rows = table if isinstance(table, list) else np.asarray(table, dtype=np.int64).reshape(-1, 4).tolist()
    for oa, ol, na, nl in rows:
        a, la, b, lb = (oa, ol, na, nl) if dir == OLD_TO_NEW else (na, nl, oa, ol)
        if a <= x:
            last = (int(a), int(la), int(b), int(lb))
    if last is None:
        return x & M32, 0
    a, la, b, lb = last
    if x > a + la:
        return (x - (a + la) + (b + lb)) & M32, 0
    if la == 0:
        side = 1 if bias == RIGHT else -1
    elif x == a:
        side = -1
    elif x == a + la:
        side = 1
    else:
        side = 1 if bias == RIGHT else -1
    return (b if side < 0 else b + lb) & M32, int(a < x < a + la)


def ref_rebase_many(table, xs, dir: int = OLD_TO_NEW, bias: int = RIGHT):
    """ref_rebase for every x of xs: (y u32 array, hit u8 array)"""
    rows = np.asarray(table, dtype=np.int64).reshape(-1, 4).tolist()  # (converted once)
    got = [ref_rebase(rows, x, dir, bias) for x in xs]
    return (np.array([g[0] for g in got], dtype=np.uint32).reshape(-1),
            np.array([g[1] for g in got], dtype=np.uint8).reshape(-1))
