"""CPU-only: multi-op remote txns and general-form record groups (RTXN + RINS / RDEL + RPARENT,
replayed by replay_core.h apply_txn's interpreter and, for one-op runs, by fast_txn at stride 3).

 - fuzz_gen.multi_op_wire's committed histories hold the txn shapes no other generator makes
   (shape floors), its recorder input is sound, and the oracle ends at most 1 in 10 of them with an
   error status;
 - every history, every hand-built window stream of tests/general_streams.py and every txn that
   fails at its second or third op replays on the CPU emulation, at both leaf layouts with tight
   capacities, to the oracle's status and the oracle's state, exactly;
 - the emulator's statistics build (tests/emu `make stats`) proves which branches the window
   families reach: counters 76 / 77 (run(): fast_txn took a general-form remote txn / txns those
   calls consumed), 47 (apply_txn calls), 78 / 79 (rec_at read a record from the window / from
   memory).

tests/test_gpu_multi_op.py and tests/test_gpu_window_general.py replay the same inputs on the
engine.  The emulator replays a window stream as ONE wire behind its prep txns, so a stream's
records sit general_streams.records(prep) further on than in the engine's second batch; the pads
of family (a) cover every lane either way."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import emu_lib
import general_streams as gs
from emu_lib import EmuDoc, diff_states
from fuzz_gen import (MULTI_OP_SEEDS, draw_multi_op_txn, multi_op_family, multi_op_params, multi_op_wire, parse_wire,
                      txn_shape)
from oracle_lib import OracleDoc, trace_to_wire

LAYOUTS = {32: (32, 16), 4: (4, 8)}


def same_as_oracle(wire, leaf, what):
    """the emulator's replay of `wire` against the oracle's: status, invariants, state; returns the status"""
    o = OracleDoc(*LAYOUTS[leaf])
    so = o.apply_remote_wire(wire)
    e = EmuDoc(leaf)
    se = e.run_wire(wire, 48)
    assert se == so, (what, leaf, se, so)
    if so == 0:
        assert e.check() == "", (what, leaf)
        assert diff_states(o.export(), e.export()) == [], (what, leaf)
    return so


# ------------------------------------------------------------------ the generator
def test_shape_floors():
    """The committed histories (MULTI_OP_SEEDS, multi_op_params) hold, counted with the committed
    generator: 2,095 txns, of them 1,309 mixed (inserts and deletes), 1,209 with at least 2
    inserts, 761 inserts with an origin in their own txn's seq range, 466 deletes with a target in
    their own txn's seq range, 573 txns with at least 5 wire ops.  Each floor is half of that (and
    at least 100): a generator that slides back to one-op histories fails here."""
    tot = np.zeros(5, np.int64)
    for _seed, w in multi_op_family():
        for t in parse_wire(w)[1]:
            tot += np.array(txn_shape(t), np.int64)
    print(tot.tolist())
    for got, floor in zip(tot.tolist(), (654, 604, 380, 233, 286)):
        assert got >= max(floor, 100), tot.tolist()


def test_same_seed_same_bytes():
    assert multi_op_wire(5, **multi_op_params(5)) == multi_op_wire(5, **multi_op_params(5))
    assert multi_op_wire(5, **multi_op_params(5))[0] == dict(multi_op_family())[5]
    assert multi_op_wire(5)[0] != multi_op_wire(6)[0]
    assert len(parse_wire(multi_op_wire(3, leaf=4)[0])[1]) > 10  # (replicas at the debug layout)


def test_at_most_one_in_ten_histories_stops():
    # a history the oracle ends with an error status counts only in the status comparisons
    for leaf in (32, 4):
        bad = [s for s, w in multi_op_family() if OracleDoc(*LAYOUTS[leaf]).apply_remote_wire(w) != 0]
        print(leaf, bad)
        assert 10 * len(bad) <= len(MULTI_OP_SEEDS)


def test_histories_are_concurrent():
    # several heads: some txn of every history with more than one agent has several parents
    for seed, w in multi_op_family():
        txns = parse_wire(w)[1]
        if len(txns) > 20:
            assert any(len(t[2]) > 1 for t in txns), seed
            assert len({t[0] for t in txns}) == multi_op_params(seed)["n_agents"]


def multi_op_trace(seed, n_txns=300):
    """a single agent's local trace regrouped into txns of 1..4 ops, replaces included"""
    rng = random.Random(seed)
    counts, patches, n = [], [], 0
    for _ in range(n_txns):
        ops, n = draw_multi_op_txn(rng, n, end_ok=True)
        counts.append(len(ops))
        patches += ops
    return np.array(counts, np.uint32), np.array(patches, np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("leaf", [32, 4])
def test_recorder_is_sound(leaf):
    # the local trace applied to one oracle, its recorded wire applied to a fresh one: equal exports
    for seed in range(4):
        counts, patches = multi_op_trace(seed)
        assert (counts > 1).sum() > 100 and ((patches[:, 1] > 0) & (patches[:, 2] > 0)).sum() > 20
        a = OracleDoc(*LAYOUTS[leaf])
        assert a.apply_trace(a.agent("solo"), counts, patches) == 0
        w = trace_to_wire(counts, patches, "solo", leaf)
        assert len(parse_wire(w)[1]) == counts.shape[0]  # one remote txn per local txn
        r = OracleDoc(*LAYOUTS[leaf])
        assert r.apply_remote_wire(w) == 0
        assert diff_states(a.export(), r.export()) == []
        same_as_oracle(w, leaf, ("solo", seed))


# ------------------------------------------------------------------ emulator parity
@pytest.mark.parametrize("leaf", [32, 4])
def test_histories_match_oracle(leaf):
    sts = [same_as_oracle(w, leaf, seed) for seed, w in multi_op_family()]
    assert sum(s == 0 for s in sts) >= 36


@pytest.mark.parametrize("leaf", [32, 4])
@pytest.mark.parametrize("family", ["runs", "groups"])
def test_window_families_match_oracle(family, leaf):
    fam = gs.run_family() if family == "runs" else gs.group_family()
    assert len(fam) == (1344 if family == "runs" else 576)
    for name, (_p, _s, w) in fam.items():
        assert same_as_oracle(w, leaf, name) == 0, name


@pytest.mark.parametrize("leaf", [32, 4])
def test_no_stream_stops_for_capacity(leaf):
    # a stop for capacity resumes with the window loaded at the record it stopped at (before a txn
    # of n ops the replay wants 2n free leaves: a group would stop at its own header and resume
    # with it in lane 0).  The prep's warm-up txn grows the tables, so the stream part replays
    # without a stop: as many growth events with the stream as without it
    for fam in (gs.run_family(), gs.group_family()):
        grown = {}
        for name, (w0, _s, w) in fam.items():
            if w0 not in grown:
                e = EmuDoc(leaf)
                assert e.run_wire(w0, 48) == 0
                grown[w0] = e.sizes()["grow_events"]
                assert grown[w0] > 0  # (the warm-up does grow them)
            e = EmuDoc(leaf)
            assert e.run_wire(w, 48) == 0
            assert e.sizes()["grow_events"] == grown[w0], name


def test_window_streams_are_what_they_claim():
    # pads are compact records, a run's txns and a group are general-form: the record counts
    prep, s = gs.run_stream(5, 20, "back")
    assert gs.records(prep) == gs.PREP_RECORDS and gs.records(s) == 5 + 3 * 20 + 3
    prep, s = gs.group_stream(57, 62, 3, True)
    assert gs.records(prep) == gs.PREP_RECORDS + 6 + 3
    assert gs.records(s) == 57 + (1 + 62 + 3) + 3 * gs.TAIL_TYPED + 3 * gs.TAIL_DELETES
    assert {op[0] for op in s[57][3]} == {0, 1} and len(s[57][2]) == 3
    # the groups' records end short of, at and past every window threshold, and past 128
    ends = {pad + 1 + nops + np_ for pad in gs.GROUP_PADS for nops in gs.GROUP_NOPS for np_ in gs.GROUP_PARENTS}
    assert {60, 61, 62, 63, 64, 65, 66, 123, 124, 125, 126, 127, 128, 129} <= ends and max(ends) > 192


@pytest.mark.parametrize("leaf", [32, 4])
def test_error_statuses_match_oracle(leaf):
    seen = set()
    for name in gs.ERROR_CASES:
        st = same_as_oracle(gs.error_wire(name), leaf, name)
        assert st != 0, name
        seen.add(st)
    assert len(seen) >= 3  # (unknown id, unknown agent, bad input)
    assert same_as_oracle(gs.good_wire(), leaf, "good") == 0


# ------------------------------------------------------------------ the branches are reached
FAST_GEN, FAST_GEN_TXNS, APPLY_TXN, REC_WINDOW, REC_MEMORY = 76, 77, 47, 78, 79


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
    L.emu_stats.argtypes = [P(C.c_uint64), C.c_int]
    return L


def counters(L, wire, leaf):
    z = np.zeros(128, np.uint64)
    L.emu_stats(z.ctypes.data_as(C.POINTER(C.c_uint64)), 1)
    h = L.emu_new(leaf)
    st = L.emu_run_wire(h, wire, len(wire), 48)
    L.emu_free(h)
    L.emu_stats(z.ctypes.data_as(C.POINTER(C.c_uint64)), 1)
    assert st == 0
    return z.astype(np.int64)


@pytest.mark.parametrize("leaf", [32, 4])
def test_runs_are_taken_at_stride_3(stats_lib, leaf):
    """Family (a): the general-form txns of a run of n >= 2 are consumed by fast_txn, 3 records
    each (counter 77 counts them; the stream holds no other general-form one-op txn that the fast
    path can take: the prep's are other authors' or the document's first), all but at most one --
    so not op by op through apply_txn, which takes the prep's four txns and little else (counter
    47).  A typing run is one entry: fast_txn takes several txns per call (77 against 76); a's
    deletes of base items are no run of its own items and go one txn per call.  Every pad, so every
    phase of the run against the window."""
    fam = gs.run_family()
    for kind in gs.RUN_KINDS:
        for n in (2, 20, 21, 22, 43, 64):
            for pad in gs.RUN_PADS:
                z = counters(stats_lib, fam[f"{kind}_n{n}_pad{pad}"][2], leaf)
                what = (kind, n, pad, int(z[FAST_GEN]), int(z[FAST_GEN_TXNS]), int(z[APPLY_TXN]))
                assert n - 1 <= z[FAST_GEN_TXNS] <= n, what
                if n >= 20:
                    assert z[APPLY_TXN] < n, what  # (the whole stream: fewer calls than the run has txns)
                if kind == "typing" and n >= 20:
                    assert z[FAST_GEN_TXNS] >= 2 * z[FAST_GEN], what


@pytest.mark.parametrize("leaf", [32, 4])
def test_groups_read_window_and_memory(stats_lib, leaf):
    """Family (b): apply_txn's rec_at reads a group's op and parent records from the window's lanes
    (counter 78) and, past the window, from memory (counter 79): a group that begins near the
    window's end or holds more than 64 records does both within one txn."""
    fam = gs.group_family()
    prep = {}
    both = 0
    for name, (w0, _s, w) in fam.items():
        if w0 not in prep:
            prep[w0] = counters(stats_lib, w0, leaf)
        z = counters(stats_lib, w, leaf) - prep[w0]  # the stream part's reads alone (the replay is deterministic)
        nops = int(name.split("_ops")[1].split("_")[0])
        np_ = int(name.split("_p")[1].split("_")[0])
        # the stream's general-form txns: the group, and the tail's one-op txns (2 reads each)
        assert z[REC_WINDOW] + z[REC_MEMORY] == nops + np_ + 2 * (gs.TAIL_TYPED + gs.TAIL_DELETES) - 2 * z[FAST_GEN_TXNS], name
        assert z[REC_WINDOW] > 0, name
        if nops >= 120:  # more records than a window holds: both within the one txn
            assert z[REC_MEMORY] >= nops - 64, name
        both += int(z[REC_MEMORY] > 0)
    print(both)
    assert both >= len(fam) // 2
