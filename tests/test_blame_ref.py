"""CPU checks of the authorship-run definition (tests/blame_ref.py) against the oracle's pos_to_loc,
and of the library's blame entry points being exported.

ref_blame's runs, expanded item by item, must be the oracle's answer for every position; no two
neighbouring runs may chain under the mode (maximality).
"""
import ctypes

import numpy as np
import pytest

import crdt_amd
from blame_ref import chains, expand, ref_blame
from fuzz_gen import build_wire, concurrent_wire, parse_wire
from oracle_lib import OracleDoc
from test_diff_ref import double_delete_txns

LAYOUTS = [(32, 16), (4, 8)]

BLAME_SYMBOLS = ["crdt_blame_async", "crdt_blame_counts", "crdt_blame_read", "crdt_last_blame_ms"]


def alternating_doc(o, n, names=("xa", "yb")):
    """two authors alternately append one character each: n items, one canonical span, n
    client_with_order runs"""
    ag = [o.agent(x) for x in names]
    for j in range(n):
        assert o.apply_local(ag[j % 2], [(j, 0, 1)]) == 0
    return ag


def tombstone_doc(o):
    """xa types 10 characters, yb inserts 2 in the middle, and they are then deleted"""
    xa, yb = o.agent("xa"), o.agent("yb")
    assert o.apply_local(xa, [(0, 0, 10)]) == 0
    assert o.apply_local(yb, [(5, 0, 2)]) == 0
    assert o.apply_local(xa, [(5, 2, 0)]) == 0
    return xa, yb


def check_against_oracle(o):
    """both modes of ref_blame against pos_to_loc of every position; returns the two run counts"""
    ex = o.export()
    n = len(o)
    oa, os_ = o.pos_to_loc(np.arange(n, dtype=np.uint32))
    counts = []
    for mode in ("agent", "id"):
        runs = ref_blame(ex, mode)
        assert int(runs[:, 1].sum()) == n
        assert (runs[:, 1] > 0).all()
        agents, seqs = expand(runs, mode)
        assert agents == [int(x) for x in oa], mode
        if mode == "id":
            assert seqs == [int(x) for x in os_]
        m = 0 if mode == "agent" else 1
        for a, b in zip(runs[:-1], runs[1:]):  # maximality: the last item of a run does not chain with the next run's first
            last = (int(a[2]), int(a[3]) + int(a[1]) - 1)
            assert not chains(last, (int(b[2]), int(b[3])), m), (mode, a, b)
        counts.append(runs.shape[0])
    return counts


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", range(6))
def test_reference_against_oracle_pos_to_loc(seed, layout):
    wire, _ = concurrent_wire(seed)
    o = OracleDoc(*layout)
    assert o.apply_remote_wire(wire) == 0
    n_agent, n_id = check_against_oracle(o)
    assert 18 <= n_agent <= 29 and 24 <= n_id <= 38, (n_agent, n_id)
    assert n_id > n_agent
    if seed in (0, 3, 4):  # a run crosses canonical spans
        visible = int((o.export()["canon"][:, 3].astype(np.int32) > 0).sum())
        assert n_id < visible, (n_id, visible)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_reference_alternating_authors(layout):
    o = OracleDoc(*layout)
    alternating_doc(o, 700)
    ex = o.export()
    assert len(ex["canon"]) == 1 and len(ex["cwo"]) == 700
    assert check_against_oracle(o) == [700, 700]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_reference_tombstones_between_chained_spans(layout):
    o = OracleDoc(*layout)
    xa, _ = tombstone_doc(o)
    ex = o.export()
    assert len(ex["canon"]) == 3
    for mode in ("agent", "id"):
        assert ref_blame(ex, mode).tolist() == [[0, 10, xa, 0]]
    assert check_against_oracle(o) == [1, 1]


def test_reference_double_deletes():
    o = OracleDoc()
    assert o.apply_remote_wire(build_wire(double_delete_txns())) == 0
    ex = o.export()
    a = o.agent("A")
    # items 2..7 are gone: 0 1 8 9 remain, all of agent A
    assert ref_blame(ex, "agent").tolist() == [[0, 4, a, 0]]
    assert ref_blame(ex, "id").tolist() == [[0, 2, a, 0], [2, 2, a, 8]]
    assert check_against_oracle(o) == [1, 2]


def test_reference_empty_and_fully_deleted():
    o = OracleDoc()
    assert ref_blame(o.export(), "agent").shape == (0, 4)
    a = o.agent("xa")
    assert o.apply_local(a, [(0, 0, 7)]) == 0 and o.apply_local(a, [(0, 7, 0)]) == 0
    assert ref_blame(o.export(), "id").shape == (0, 4)


def test_prefixes_parse():
    # the GPU test replays every prefix of this history: each must be a valid history of its own
    txns = parse_wire(concurrent_wire(3)[0])[1]
    for k in (1, len(txns) // 2, len(txns)):
        o = OracleDoc()
        assert o.apply_remote_wire(build_wire(txns[:k])) == 0
        check_against_oracle(o)


def test_library_exports_the_blame_entry_points():
    crdt_amd.build()
    lib = ctypes.CDLL(crdt_amd.LIB_PATH)
    for s in BLAME_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in crdt_amd.EXPORTED_SYMBOLS, s
