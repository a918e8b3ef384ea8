"""CPU checks of the checkout definition (tests/checkout_ref.py) against the oracle's texts, and of
the library's checkout entry points being exported.

ref_checkout(export of the full replay, v) must equal the oracle's text of a prefix replay that
ends at version v.  Content is np.arange(next_order), so a text is the list of its items' orders.
The inputs are those of tests/test_diff_ref.py.
"""
import ctypes

import numpy as np
import pytest

import crdt_amd
from checkout_ref import ref_checkout
from diff_ref import ref_diff
from fuzz_gen import concurrent_wire, parse_wire
from test_diff_ref import LAYOUTS, double_delete_txns, micro_txns, replay

CHECKOUT_SYMBOLS = ["crdt_checkout_async", "crdt_checkout_lens", "crdt_checkout_read", "crdt_checkout_digest",
                    "crdt_pos_to_loc_at", "crdt_loc_to_pos_at", "crdt_pos_to_loc_at_dev_async",
                    "crdt_loc_to_pos_at_dev_async", "crdt_last_checkout_ms"]


def check_version(ex, v, old):
    """the view at v is the prefix replay `old`'s text, and the diff from v accounts for the rest"""
    content = np.arange(ex["next_order"], dtype=np.uint32)
    assert old.sizes()["next_order"] == v
    got = ref_checkout(ex, v)
    assert np.array_equal(got, old.text(content)[0]), v
    patches, _ = ref_diff(ex, v)
    assert got.shape[0] + int(patches[:, 2].sum()) - int(patches[:, 1].sum()) == ex["len"], v


def check_cuts(txns, cuts, layout=(32, 16)):
    ex = replay(txns, layout).export()
    for k in cuts:
        old = replay(txns[:k], layout)
        check_version(ex, old.sizes()["next_order"], old)
    return ex


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", range(4))
def test_reference_against_oracle_texts(seed, layout):
    wire, n = concurrent_wire(seed)
    txns = parse_wire(wire)[1]
    ex = check_cuts(txns, [0, 1, n // 3, n // 2, n - 1, n], layout)
    assert ref_checkout(ex, 0).shape[0] == 0
    assert ref_checkout(ex, ex["next_order"]).shape[0] == ex["len"]


def truncated(txns, v):
    """the one-op txns of the double-delete history, cut so that the replay ends at version v (also
    inside a txn: the op applies with the part of its length below v)"""
    out, at = [], 0
    for agent, seq, parents, ops in txns:
        (kind, an, asq, bn, bsq, ln), = ops
        take = min(ln, v - at)
        if take <= 0:
            break
        out.append((agent, seq, parents, [(kind, an, asq, bn, bsq, take)]))
        at += take
    return out


@pytest.mark.parametrize("swap", [False, True])
def test_reference_double_deletes_at_every_version(swap):
    txns = double_delete_txns()
    if swap:
        txns = [txns[0], txns[2], txns[1]]
    ex = replay(txns).export()
    assert ex["next_order"] == 18
    for v in range(19):  # 12 lies inside the first delete txn, 14 between the two, 16 inside the second
        check_version(ex, v, replay(truncated(txns, v)))
    # after the first delete txn only; inside it
    assert ref_checkout(ex, 14).tolist() == ([0, 1, 2, 3, 8, 9] if swap else [0, 1, 6, 7, 8, 9])
    assert ref_checkout(ex, 12).tolist() == ([0, 1, 2, 3, 6, 7, 8, 9] if swap else [0, 1, 4, 5, 6, 7, 8, 9])
    assert ref_checkout(ex, 18).tolist() == [0, 1, 8, 9]


def test_reference_micro_trace_cut_at_half():
    txns = micro_txns("del1")
    # half the txns lie inside the base typing run; 50,000 + 10,000 also cuts the single deletes
    check_cuts(txns, [len(txns) // 2, 60000])


def test_library_exports_the_checkout_entry_points():
    crdt_amd.build()
    lib = ctypes.CDLL(crdt_amd.LIB_PATH)
    for s in CHECKOUT_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in crdt_amd.EXPORTED_SYMBOLS, s
