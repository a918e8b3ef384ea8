"""Delete runs in k_replay's leaf-split loop (replay_core.h fast_deletes; DESIGN §4 "Carried
cursor"): between the deletes of a run the cursor is carried -- delete_segment hands back the place
of the next target, and after delete_general the caller derives it from the cursor it holds --
instead of looked up by order, and an overflowing delete
whose split keeps the cursor's entry in the cached leaf is taken by the closed form after the split
("split first").  The replay must still take every step the reference takes.

Hand-built compact remote streams (one author, a typed base text, then the runs), the smallest
that reach each branch, replay on the CPU emulation at both leaf layouts and are compared state for
state with the oracle.  The emulator asserts at every carried cursor that a lookup of the target's
order finds the same place (replay_core.h carried_is_found), in every emulator test.

test_cases_reach_their_branches proves through the emulator's statistics build (tests/emu `make
stats`) that every case reaches the branch it is named for, at each layout.  The same stream does
not meet the same leaf at L = 4 and at L = 32, so a case may hold several streams: all of them
replay at both layouts, and at each layout the case's counters must all have been hit.

One case of the kind "a general delete whose last piece prepends, overflowing at a split" cannot
be built: for the leaf to overflow with a prepend, the entry must split in three (off > 0, a
visible remainder) and the remainder must be appendable to the visible entry after it in the same
leaf -- two visible neighbours of consecutive orders, the second naming the first's last item as
its origin_left, with one origin_right.  insert_internal appends such an item to its neighbour
when it arrives, and no split or delete separates one entry into two visible neighbours, so no
replay produces that leaf; the three traces and the micro workloads never take a prepend in
delete_general at all (counter 65 stays 0 at both layouts).  Case "prepend" therefore takes the
prepend that does occur -- a deleted piece onto the deleted run after it, in leaf_delete at a full
leaf -- and checks that the split-first path declined nothing and took nothing there.  So two
guards of fast_deletes are run by no test: split first's decline on a prepend (counter 73) and the
lookup inside the loop (counter 75); DESIGN §4 says so."""
import ctypes as C
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

import emu_lib
from crdt_amd.traces import TRACE_NAMES, load_remote_wire
from emu_lib import EmuDoc, diff_states
from oracle_lib import OracleDoc, trace_to_wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {32: (32, 16), 4: (4, 8)}
MICRO = ["bs10", "bs200", "fd200", "del1"]

# replay_core.h CRDT_STAT sites
SPLITS, FOLLOW_BACK, FOLLOW_FWD, NONFOLLOW, CALLS, OVER_BACK, OVER_FWD, OVER_OFF0 = 0, 4, 5, 6, 9, 48, 49, 52
CYCLE_CALLS = 57
CARRIED, LOOKUP_KEPT, SPLIT_FIRST, ONE_ITEM, P0, PRE_GENERAL, LONG_RUN, DECLINED_PRE, PRE_LEAF, LOOKUP_LOOP = 59, 60, 61, 62, 63, 65, 68, 73, 74, 75


def ins(pos):
    return [(pos, 0, 1)]


def back(pos, k):  # k backspaces, the first deleting the char at pos
    return [(pos - i, 1, 0) for i in range(k)]


def fwd(pos, k):  # k forward deletes at pos
    return [(pos, 1, 0)] * k


BASE = 600
# 14 single chars typed into the base text at 150, 161, 172, ...: base pieces of 150, 10, ..., 10 and
# 320 chars around them, 29 entries -- a 32-entry leaf with three free slots; runs in the first
# piece split it below L/2 (the entries after it move), runs in the last piece at or above L/2
PRELUDE = [op for j in range(14) for op in ins(150 + 11 * j)]
N = BASE + 14
LAST = 150 + 11 * 14  # the last base piece's first position


def _hit(*keys):
    return lambda z: sum(int(z[k]) for k in keys) > 0


def crosses_twice(z):
    """one stream's counters: the run crosses a full leaf twice (split_at calls, plus back_cycles
    calls, each of which makes at least one split of its own)"""
    return int(z[SPLITS]) + int(z[CYCLE_CALLS]) >= 2


MID = lambda z: int(z[OVER_BACK]) + int(z[OVER_FWD]) > int(z[OVER_OFF0])  # an overflowing delete at off > 0  # noqa: E731

# name -> (streams, base length, [predicates over the counters summed over the streams]); the
# first two streams of the four run cases are the long runs: each must cross a full leaf twice.
# A backspace run of 100 keeps the general delete at a non-follow overflow (whole cycles are left:
# counter 6), so each backspace case has a third, short run, which must split first (counter 61).
CASES = {
    "back_from_last_item": ([PRELUDE + back(149, 100), PRELUDE + back(N - 1, 100), PRELUDE + back(149, 8)], BASE,
                            [_hit(OVER_BACK), _hit(CARRIED), _hit(NONFOLLOW), _hit(SPLIT_FIRST), _hit(FOLLOW_BACK)]),
    "back_from_mid_entry": ([PRELUDE + back(120, 100), PRELUDE + back(N - 40, 100), PRELUDE + back(120, 8)], BASE,
                            [_hit(OVER_BACK), _hit(CARRIED), _hit(NONFOLLOW), _hit(SPLIT_FIRST), _hit(FOLLOW_BACK)]),
    # (the third stream: two chars typed at the start of a 3-entry text fill a 4-entry leaf with the
    # run's entry at index 0)
    "forward_from_off0": ([PRELUDE + fwd(0, 100), PRELUDE + fwd(LAST, 100), ins(150) + [(0, 0, 1), (1, 0, 1)] + fwd(0, 2)], BASE,
                          [_hit(OVER_FWD), _hit(OVER_OFF0), _hit(CARRIED), _hit(SPLIT_FIRST), _hit(FOLLOW_FWD)]),
    # (a fifteenth char leaves the 32-entry leaf one free slot: the run's first delete, at off > 0,
    # overflows it)
    "forward_from_mid_entry": ([PRELUDE + fwd(30, 100), PRELUDE + fwd(LAST + 30, 100),
                                PRELUDE + ins(LAST + 11) + fwd(30, 40), PRELUDE + ins(LAST + 11) + fwd(LAST + 42, 40)], BASE,
                               [_hit(OVER_FWD), MID, _hit(CARRIED), _hit(SPLIT_FIRST), _hit(FOLLOW_FWD)]),
    # the run reaches its entry's first item and goes on in the entry before it: three calls, each
    # entered through a lookup
    "back_into_entry_before": ([ins(100) + back(110, 30) + ins(5)], BASE,
                               [lambda z: int(z[CALLS]) >= 3 and int(z[LOOKUP_KEPT]) >= 3, lambda z: int(z[LOOKUP_LOOP]) == 0]),
    "forward_to_entry_end": ([ins(100) + fwd(90, 30) + ins(5)], BASE,
                             [lambda z: int(z[CALLS]) >= 3 and int(z[LOOKUP_KEPT]) >= 3, lambda z: int(z[LOOKUP_LOOP]) == 0]),
    "one_item_entry": ([ins(100) + ins(106) + back(105, 5), ins(100) + back(110, 11)], BASE, [_hit(ONE_ITEM)]),
    # a single forward delete leaves [A][d][C]; a backspace run from A's last item prepends its first
    # deleted item onto d (second stream: the deleted item a split left behind the run's entry)
    "next_entry_takes_first_deleted": ([fwd(300, 1) + ins(5) + back(300, 10), PRELUDE + back(120, 100)], BASE, [_hit(P0)]),
    "prepend": ([ins(100) + ins(200) + fwd(150, 1) + ins(5) + back(150, 1) + ins(7) + fwd(300, 2) + ins(9) + back(301, 3)], BASE,
                [_hit(PRE_LEAF), lambda z: int(z[DECLINED_PRE]) == 0 and int(z[PRE_GENERAL]) == 0]),
    "run_longer_than_a_window": ([[op for i in range(70) for op in ins(7 + 5 * i)] + back(590, 150)], BASE, [_hit(LONG_RUN), _hit(CARRIED)]),
    # one run that outgrows the planned leaves of the 4-entry layout: the replay stops inside the
    # run on capacity and resumes at a record in its middle
    "cut_by_leaf_capacity": ([back(900, 700)], 1000, [_hit(CARRIED)]),
}
GROWS = "cut_by_leaf_capacity"
LONG_RUNS = ["back_from_last_item", "back_from_mid_entry", "forward_from_off0", "forward_from_mid_entry"]


@functools.lru_cache(maxsize=None)
def wires():
    """name -> the case's streams as remote wires (built once, the same for both layouts)"""
    out = {}
    for name, (streams, base, _) in CASES.items():
        ws = []
        for ops in streams:
            v = [(0, 0, base)] + ops
            ws.append(trace_to_wire(np.ones(len(v), np.uint32), np.array(v, np.uint32)))
        out[name] = ws
    return out


@functools.lru_cache(maxsize=None)
def oracle_docs(leaf):
    """(name, stream index) -> the oracle after the stream, computed once per layout"""
    out = {}
    for name, ws in wires().items():
        for i, w in enumerate(ws):
            o = OracleDoc(*LAYOUTS[leaf])
            assert o.apply_remote_wire(w) == 0, (name, i)
            out[name, i] = o
    return out


@functools.lru_cache(maxsize=None)
def micro_wire(name):
    with gzip.open(os.path.join(ROOT, "data", "micro", name + ".rtx.gz"), "rb") as f:
        return f.read()


def _same_as_oracle(e, o, what):
    assert e.check() == "", what
    assert diff_states(e.export(), o.export()) == [], what


@pytest.mark.parametrize("leaf", [32, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_streams_match_oracle(name, leaf):
    for i, w in enumerate(wires()[name]):
        e = EmuDoc(leaf)
        assert e.run_wire(w) == 0, (name, i)
        _same_as_oracle(e, oracle_docs(leaf)[name, i], (name, i))
        if name == GROWS and leaf == 4:
            assert e.sizes()["grow_events"] > 0


@pytest.mark.parametrize("leaf", [32, 4])
@pytest.mark.parametrize("name", MICRO + list(TRACE_NAMES))
def test_micro_wires_and_traces_match_oracle(name, leaf):
    w = micro_wire(name) if name in MICRO else load_remote_wire(name)
    o = OracleDoc(*LAYOUTS[leaf])
    assert o.apply_remote_wire(w) == 0
    e = EmuDoc(leaf)
    assert e.run_wire(w) == 0
    _same_as_oracle(e, o, name)


# ------------------------------------------------------------------ the branches are reached
@pytest.fixture(scope="module")
def stats_lib(tmp_path_factory):
    # (`make stats` into a directory of this process: parallel test workers build side by side)
    td = str(tmp_path_factory.mktemp("emu_stats"))
    subprocess.run(["make", "-s", "-C", emu_lib.EMU_DIR, "stats", "BUILD=" + td], check=True)
    L = C.CDLL(os.path.join(td, "libemu_stats.so"))
    u32, vp, P = C.c_uint32, C.c_void_p, C.POINTER
    L.emu_new.restype = vp
    L.emu_new.argtypes = [u32]
    L.emu_free.argtypes = [vp]
    L.emu_run_wire.argtypes = [vp, C.c_char_p, C.c_size_t, u32]
    L.emu_sizes.argtypes = [vp, P(C.c_uint64)]
    L.emu_stats.argtypes = [P(C.c_uint64), C.c_int]
    return L


def _counters(L, wire, leaf):
    """the statistics build's counters of one replay of `wire` (and the replay's status)"""
    z = np.zeros(128, np.uint64)
    L.emu_stats(z.ctypes.data_as(C.POINTER(C.c_uint64)), 1)
    h = L.emu_new(leaf)
    st = L.emu_run_wire(h, wire, len(wire), 48)
    s = np.zeros(14, np.uint64)
    L.emu_sizes(h, s.ctypes.data_as(C.POINTER(C.c_uint64)))
    L.emu_free(h)
    L.emu_stats(z.ctypes.data_as(C.POINTER(C.c_uint64)), 1)
    return st, z, int(s[12])


@pytest.mark.parametrize("leaf", [32, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_reach_their_branches(stats_lib, name, leaf):
    total, grown = np.zeros(128, np.uint64), 0
    for i, w in enumerate(wires()[name]):
        st, z, grow_events = _counters(stats_lib, w, leaf)
        assert st == 0
        if name in LONG_RUNS and i < 2:
            assert crosses_twice(z), (name, leaf, i, int(z[SPLITS]), int(z[CYCLE_CALLS]))
        total += z
        grown += grow_events
    missed = [i for i, want in enumerate(CASES[name][2]) if not want(total)]
    assert not missed, (name, leaf, missed, {k: int(v) for k, v in enumerate(total) if v})
    if name == GROWS and leaf == 4:
        assert grown > 0


def test_no_lookup_inside_a_run_on_the_traces(stats_lib):
    # what part 1 claims: on the flagship trace every cursor inside a run is carried; the lookups
    # that remain are the runs' entry points
    st, z, _ = _counters(stats_lib, load_remote_wire("automerge-paper"), 32)
    assert st == 0
    assert int(z[CARRIED]) > 0 and int(z[LOOKUP_LOOP]) == 0 and int(z[PRE_GENERAL]) == 0
    assert int(z[SPLIT_FIRST]) > 0
