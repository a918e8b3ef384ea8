"""CPU checks of the diff definition (tests/diff_ref.py) against the oracle's texts, and of the
library's diff entry points being exported.

ref_diff(export of the full replay, v) applied to the oracle's text of a prefix replay that ends at
version v must give the oracle's text of the full replay.  Content is np.arange(next_order), so a
text is the list of its visible items' orders and ins_order is the inserted content.
"""
import ctypes
import gzip
import os

import numpy as np
import pytest

import crdt_amd
from diff_ref import apply_patches, ref_diff
from fuzz_gen import build_wire, concurrent_wire, parse_wire
from oracle_lib import OracleDoc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = [(32, 16), (4, 8)]
R = ("ROOT", 0xFFFFFFFF)

DIFF_SYMBOLS = ["crdt_doc_version", "crdt_diff_async", "crdt_diff_counts", "crdt_diff_read", "crdt_last_diff_ms"]


def double_delete_txns():
    """A inserts 10 items; B and C concurrently delete [2, 6) and [4, 8) (items 4 and 5 twice).
    Orders: A 0..9, B's delete 10..13, C's delete 14..17."""
    return [("A", 0, [R], [(0, "ROOT", R[1], "ROOT", R[1], 10)]),
            ("B", 0, [("A", 9)], [(1, "A", 2, None, 0, 4)]),
            ("C", 0, [("A", 9)], [(1, "A", 4, None, 0, 4)])]


def micro_txns(name: str):
    with gzip.open(os.path.join(ROOT, "data", "micro", name + ".rtx.gz"), "rb") as f:
        return parse_wire(f.read())[1]


def replay(txns, layout=(32, 16)):
    o = OracleDoc(*layout)
    if txns:
        assert o.apply_remote_wire(build_wire(txns)) == 0
    return o


def check_cuts(txns, cuts, layout=(32, 16)):
    """the reference's patches turn every prefix replay's text into the full replay's; returns the
    number of patches seen"""
    full = replay(txns, layout)
    ex = full.export()
    content = np.arange(ex["next_order"], dtype=np.uint32)
    new_text = full.text(content)[0]
    n_patches = 0
    for k in cuts:
        old = replay(txns[:k], layout)
        v = old.sizes()["next_order"]
        patches, ins = ref_diff(ex, v)
        assert int(patches[:, 2].sum()) == ins.shape[0]
        got = apply_patches(old.text(content)[0], patches, ins)
        assert np.array_equal(got, new_text), (k, v)
        n_patches += patches.shape[0]
    return n_patches


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", range(4))
def test_reference_against_oracle_texts(seed, layout):
    wire, n = concurrent_wire(seed)
    txns = parse_wire(wire)[1]
    assert len(txns) == n
    assert check_cuts(txns, [0, 1, n // 3, n // 2, n - 1, n], layout) > 0


def test_reference_double_deletes():
    txns = double_delete_txns()
    ex = replay(txns).export()
    assert ex["next_order"] == 18
    # after B only: old text 0 1 6 7 8 9 -> new text 0 1 8 9
    p, ins = ref_diff(ex, 14)
    assert p.tolist() == [[2, 2, 0, 0]] and ins.shape[0] == 0
    # after both: nothing changed
    p, ins = ref_diff(ex, 18)
    assert p.shape[0] == 0 and ins.shape[0] == 0
    # inside B's delete run (orders 10, 11 applied: items 2, 3 gone): 4 5 6 7 still to delete
    p, _ = ref_diff(ex, 12)
    assert p.tolist() == [[2, 4, 0, 0]]
    assert check_cuts(txns, [0, 1, 2, 3]) == 3
    # and with C before B (the same final state, other versions in between)
    swapped = [txns[0], txns[2], txns[1]]
    assert check_cuts(swapped, [0, 1, 2, 3]) == 3


def test_reference_micro_trace_cut_at_half():
    txns = micro_txns("del1")
    n = len(txns)
    # half the txns lie inside the base typing run; 50,000 + 10,000 also cuts the single deletes
    assert check_cuts(txns, [n // 2, 60000]) > 2


def test_library_exports_the_diff_entry_points():
    crdt_amd.build()
    lib = ctypes.CDLL(crdt_amd.LIB_PATH)
    for s in DIFF_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in crdt_amd.EXPORTED_SYMBOLS, s
