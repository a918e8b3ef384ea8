"""CPU checks of the definition of the rebase map (tests/rebase_ref.py) by brute force on the
oracle, and of the library's rebase entry points being exported.

For a history replayed by the oracle and every version v of it, the old text is ref_checkout(export,
v) and the new text ref_checkout(export, next_order): two lists of item orders.  The map built from
ref_diff(export, v) must send the position of every item that is in both lists to its position in
the other list (in both directions, with the right bias and hit 0), be monotonic, answer left <=
right, and have an old side that lies inside the old text.  The unit tables from ref_edits are
checked the same way against the unit offsets of ref_encode on both texts.
"""
import ctypes

import numpy as np
import pytest

import crdt_amd
from checkout_ref import ref_checkout
from diff_ref import ref_diff
from edits_ref import mixed_content, ref_edits
from encode_ref import UTF8, UTF16, ref_encode
from fuzz_gen import concurrent_wire, parse_wire
from rebase_ref import LEFT, NEW_TO_OLD, OLD_TO_NEW, RIGHT, ref_rebase, ref_rebase_many, ref_rebase_table
from test_diff_ref import LAYOUTS, double_delete_txns, replay

REBASE_SYMBOLS = ["crdt_rebase_async", "crdt_rebase_counts", "crdt_rebase_read", "crdt_rebase", "crdt_rebase_dev_async",
                  "crdt_last_rebase_ms"]


def check_table(table, old_at_of_kept, new_at_of_kept, old_len, new_len):
    """the properties of one table; old_at_of_kept[j] / new_at_of_kept[j]: where kept item j starts
    in the old / new text (chars: its index; units: its unit offset)"""
    t = table.astype(np.int64)
    # both sides ascend, neighbours at least one kept item apart, and end inside their text
    for at, ln, total in ((t[:, 0], t[:, 1], old_len), (t[:, 2], t[:, 3], new_len)):
        assert (at[1:] > at[:-1] + ln[:-1]).all()
        assert t.shape[0] == 0 or at[-1] + ln[-1] <= total
    # item identity and the round trip
    y, hit = ref_rebase_many(table, old_at_of_kept, OLD_TO_NEW, RIGHT)
    assert y.tolist() == list(new_at_of_kept) and not hit.any()
    x, hit = ref_rebase_many(table, new_at_of_kept, NEW_TO_OLD, RIGHT)
    assert x.tolist() == list(old_at_of_kept) and not hit.any()
    # monotonic, and left <= right, at every position (and two past the end)
    for dir, n in ((OLD_TO_NEW, old_len), (NEW_TO_OLD, new_len)):
        xs = range(n + 3)
        yl, hl = ref_rebase_many(table, xs, dir, LEFT)
        yr, hr = ref_rebase_many(table, xs, dir, RIGHT)
        assert (np.diff(yl.astype(np.int64)) >= 0).all() and (np.diff(yr.astype(np.int64)) >= 0).all()
        assert (yl <= yr).all()
        assert np.array_equal(hl, hr)  # (hit does not depend on the bias)
        # the ends of the texts map to each other
        other = new_len if dir == OLD_TO_NEW else old_len
        assert int(yr[n]) == other and int(yl[0]) == 0


def check_history(ex, content=None, encs=()):
    """every version of one exported history; returns the number of spans seen"""
    n = int(ex["next_order"])
    new = ref_checkout(ex, n)
    new_at = {int(o): k for k, o in enumerate(new)}
    starts_new = {enc: ref_encode(content[new], enc)[1] for enc in encs}
    spans = 0
    for v in range(n + 1):
        old = ref_checkout(ex, v)
        kept = [(k, new_at[int(o)]) for k, o in enumerate(old) if int(o) in new_at]
        patches, _ = ref_diff(ex, v)
        table = ref_rebase_table(patches)
        assert table.shape[0] == patches.shape[0]
        check_table(table, [a for a, _ in kept], [b for _, b in kept], len(old), len(new))
        spans += table.shape[0]
        for enc in encs:
            edits, _ = ref_edits(ex, v, content, enc)
            assert np.array_equal(ref_rebase_table(edits), table)  # the char table of the edits is the diff's
            ut = ref_rebase_table(edits, units=True)
            so = ref_encode(content[old], enc)[1]
            sn = starts_new[enc]
            check_table(ut, [int(so[a]) for a, _ in kept], [int(sn[b]) for _, b in kept], int(so[-1]), int(sn[-1]))
    return spans


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", range(4))
def test_reference_against_the_oracle_at_every_version(seed, layout):
    wire, n = concurrent_wire(seed)
    txns = parse_wire(wire)[1]
    assert len(txns) == n
    ex = replay(txns, layout).export()
    assert check_history(ex) > ex["next_order"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", range(4))
def test_reference_unit_tables_at_every_version(seed, layout):
    wire, _ = concurrent_wire(seed)
    ex = replay(parse_wire(wire)[1], layout).export()
    content = mixed_content(ex["next_order"], 7 + seed)
    assert check_history(ex, content, (UTF8, UTF16)) > 0


def test_reference_rule_case_by_case():
    # old text a b c d e f g h, new text a X Y d e Z f: bc -> XY, Z inserted before f, gh deleted
    patches = np.array([[1, 2, 2, 0], [5, 0, 1, 2], [7, 2, 0, 3]], np.uint32)
    table = ref_rebase_table(patches)
    assert table.tolist() == [[1, 2, 1, 2], [5, 0, 5, 1], [6, 2, 7, 0]]
    want = {  # x: (left, right, hit), old -> new
        0: (0, 0, 0), 1: (1, 1, 0), 2: (1, 3, 1), 3: (3, 3, 0), 4: (4, 4, 0),
        5: (5, 6, 0), 6: (7, 7, 0), 7: (7, 7, 1), 8: (7, 7, 0), 9: (8, 8, 0)}
    for x, (yl, yr, hit) in want.items():
        assert ref_rebase(table, x, OLD_TO_NEW, LEFT) == (yl, hit), x
        assert ref_rebase(table, x, OLD_TO_NEW, RIGHT) == (yr, hit), x
    back = {0: (0, 0, 0), 1: (1, 1, 0), 2: (1, 3, 1), 3: (3, 3, 0), 5: (5, 5, 0), 6: (5, 5, 0), 7: (6, 8, 0), 8: (9, 9, 0)}
    for x, (yl, yr, hit) in back.items():
        assert ref_rebase(table, x, NEW_TO_OLD, LEFT) == (yl, hit), x
        assert ref_rebase(table, x, NEW_TO_OLD, RIGHT) == (yr, hit), x
    # no span: the identity; arithmetic is modulo 2^32
    empty = ref_rebase_table(np.zeros((0, 4), np.uint32))
    assert empty.shape == (0, 4) and ref_rebase(empty, 77, OLD_TO_NEW, LEFT) == (77, 0)
    assert ref_rebase(table, 0xFFFFFFFF, NEW_TO_OLD, RIGHT) == (0, 0)
    with pytest.raises(ValueError):
        ref_rebase_table(patches, units=True)


def test_reference_double_deletes():
    # after B only the old text is 0 1 6 7 8 9 and C's delete takes items 6 and 7
    ex = replay(double_delete_txns()).export()
    table = ref_rebase_table(ref_diff(ex, 14)[0])
    assert table.tolist() == [[2, 2, 2, 0]]
    assert [ref_rebase(table, x, OLD_TO_NEW, RIGHT) for x in range(7)] == [(0, 0), (1, 0), (2, 0), (2, 1), (2, 0), (3, 0), (4, 0)]
    assert check_history(ex) > 0


def test_library_exports_the_rebase_entry_points():
    crdt_amd.build()
    lib = ctypes.CDLL(crdt_amd.LIB_PATH)
    for s in REBASE_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in crdt_amd.EXPORTED_SYMBOLS, s
