"""Reference definition of the per-document diff (Engine.diff / crdt_diff_async) — TEST INFRASTRUCTURE.

A document's version is its next order.  "The document at version v" is the effect of every insert
item and delete op with order < v.  ref_diff walks the items of the current state in document order
(the canonical spans, expanded item by item) and classifies each item with order x:

  old-visible  x < v and no delete-log entry (key, target, len) covers x with a delete order
               key + (x - target) < v (a delete run that straddles v counts with its part below v)
  new-visible  its canonical span has len > 0

  K (old and new visible) closes the current patch; D (old only) adds 1 to its del_len; I (new
  only) appends the item to its inserted items; N (neither) is ignored and closes nothing.

A patch is a maximal run of D and I items with no K between them; pos = new-visible items before
the run.  Applied front to back, each at its pos in the text the previous ones left, the patches
turn the text at version v into the current text.  The form is unique: results compare exactly.
"""
import numpy as np


def ref_diff(ex: dict, v: int):
    """ex: the `canon`, `deletes` and `next_order` tables of OracleDoc.export() / Engine.export().
    Returns (patches [n, 4] u32 = (pos, del_len, ins_len, ins_off), ins_order [n_ins] u32)."""
    v = int(v)
    if not 0 <= v <= int(ex["next_order"]):
        raise ValueError(f"version {v} outside [0, {int(ex['next_order'])}]")
    old_deleted = set()
    for key, target, ln in np.asarray(ex["deletes"], dtype=np.int64).reshape(-1, 3):
        for j in range(int(ln)):
            if key + j < v:
                old_deleted.add(int(target + j))
    patches, ins = [], []
    cur = None      # the open patch: [pos, del_len, ins_len, ins_off]
    visible = 0     # new-visible items walked so far
    for order, _ol, _orr, ln in np.asarray(ex["canon"], dtype=np.uint32).reshape(-1, 4):
        ln = int(np.int32(ln))
        new_vis = ln > 0
        for x in range(int(order), int(order) + abs(ln)):
            old_vis = x < v and x not in old_deleted
            if old_vis and new_vis:          # K
                cur = None
            elif old_vis or new_vis:         # D or I
                if cur is None:
                    cur = [visible, 0, 0, len(ins)]
                    patches.append(cur)
                if old_vis:
                    cur[1] += 1
                else:
                    cur[2] += 1
                    ins.append(x)
            visible += new_vis
    return np.array(patches, dtype=np.uint32).reshape(-1, 4), np.array(ins, dtype=np.uint32)


def apply_patches(text, patches, ins=None):
    """Apply patches front to back like crdt_local_ops: at pos remove del_len items, then insert
    ins[ins_off : ins_off + ins_len].  `patches` may be the (patches, ins_order) pair ref_diff
    returns; `ins` holds one value per inserted item (orders, or code points)."""
    if ins is None:
        patches, ins = patches
    out = [int(x) for x in text]
    ins = [int(x) for x in ins]
    for pos, dl, il, off in np.asarray(patches, dtype=np.int64).reshape(-1, 4):
        assert pos + dl <= len(out), (pos, dl, len(out))
        out[pos:pos + dl] = ins[off:off + il]
    return np.array(out, dtype=np.uint32)
