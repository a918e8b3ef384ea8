"""CPU-only: LOCAL record streams (REC_LC, host_plan.h encode_local_txn) placed against the replay's
64-record window -- tests/local_streams.py's families on the oracle and on the CPU emulation of
replay_core.h, at both leaf layouts; tests/test_gpu_window_local.py replays the same scripts on the
engine, whose scans (wave_gpu.h typing_scan_r / delete_scan_r / front_scan) the emulation does not
compile.

 - the scripts are what they claim: the record counts behind the lane claims, and no script but the
   named ones (the *_past_* runs, the all-empty-op txn) ends with an error status on the oracle;
 - every script, base insert and stream as one batch (record k of a script is record k + 1 of the
   stream), replays on the emulation to the oracle's status and state, exactly, and the replay's
   record cursor ends at 1 + local_streams.records(ops): the host encodes what records() counts;
 - the emulator's statistics build (tests/emu `make stats`) proves the intended branches run.
   Counters (replay_core.h CRDT_STAT): 47 apply_txn calls; 9 / 12 fast_deletes calls / the runs'
   txns; 80 typing_run's scans past the window; 81 fast_deletes' scans past the window; 82 / 90
   front_scan results > 1 / their sum; 83 prepends that split a full leaf (split_at(0)) and scan
   for the front run that refills it; 84 leaf_delete_span successes; 85 local_delete_pieces calls;
   86 / 87 typing runs of >= 2 txns / their txns; 88 / 89 delete runs of >= 2 txns / their txns;
   91 / 92 leaf_delete_span pieces that joined the entry after them (the deleted rest of the first
   entry / the visible rest of the last).

Sensitivity (checked by hand on a scratch copy of tests/emu/wave_cpu.h, one term of a local scan's
predicate removed at a time, this file run against each):
   typing_scan_b, compact local: author -- second_author_in_typing (state and run counters);
     w3 - 1 < 0xFFFF -- big_chunk_in_typing, by test_near_misses_make_two_runs only (the chunk
     appends to the entry either way: the same state); pos -- most scripts of A to D;
   delete_scan_b, compact local: author -- second_author_in_forward / _back; w2 == 1 -- del2_in_*;
     pos -- forward_then_back, back_then_forward;
   front_scan: author -- second_author_in_front; pos -- run*_front, delete_in_front; length --
     other_length_in_front.
   Three terms cannot fail alone and their mutants pass: w2 == 0 (typing), w3 == 0 (delete) and
   w2 == 0 (front) -- the host never encodes an LC record that both deletes and inserts (a replace
   is two records), so a record that gets past the other terms always satisfies these."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_lib
import local_streams as ls
from emu_lib import EmuDoc, diff_states

u32, vp, P = C.c_uint32, C.c_void_p, C.POINTER


def _declare(L):
    L.emu_new.restype = vp
    L.emu_new.argtypes = [u32]
    L.emu_free.argtypes = [vp]
    L.emu_agent.argtypes = [vp, C.c_char_p]
    L.emu_run_local_agents.argtypes = [vp, u32, P(u32), P(u32), P(u32), u32]
    return L


def run_agents(L, h, ops, leaf_div=48):
    """base insert + ops as one stream on emulated document h (AUTHORS interned: ids 0 and 1)"""
    assert [L.emu_agent(h, nm.encode()) for nm in ls.AUTHORS] == [0, 1]
    a, c, p = ls.flat(ls.base_ops() + ops)
    return L.emu_run_local_agents(h, a.shape[0], a.ctypes.data_as(P(u32)), c.ctypes.data_as(P(u32)),
                                  p.ctypes.data_as(P(u32)), leaf_div)


# ------------------------------------------------------------------ the scripts
def test_family_sizes_and_records():
    assert {f: len(ls.family(f)) for f in ls.FAMILIES} == {
        "A": len(ls.A_LENS) * len(ls.KINDS), "B": len(ls.B_LENS) * len(ls.B_PADS) * len(ls.KINDS),
        "C": 11 * len(ls.C_LANES), "D": 17 * len(ls.D_PADS), "E": 4 * len(ls.E_LENS)}
    assert len(ls.scripts()) == sum(len(ls.family(f)) for f in ls.FAMILIES)
    # records(): one per non-empty part; an all-empty txn keeps LTXN + one LOP per op
    assert ls.records([(0, [(5, 0, 1)]), (0, [(5, 2, 3)]), (0, [(1, 0, 2), (9, 0, 0), (3, 1, 1)]), (0, [(5, 0, 0), (9, 0, 0)])]) == 1 + 2 + 3 + 3
    sc = ls.scripts()
    # families A, B, E: one record per txn; a run of family B begins in lane `pad`
    for name in ("stream129_typing_mixed", "run130_pad61_front_w2", "back_past_start_70"):
        assert ls.records(sc[name][0]) == len(sc[name][0])
    assert len(sc["run130_pad63_back"][0]) == 63 + 130 + 3
    ops = sc["run2_pad63_typing_mixed"][0]
    assert ops[63][1] == [(221, 0, 1)] and ops[64][1] == [(222, 0, 2)]  # chunks of unequal length, each at the previous end
    # family C: the span delete (the script's longest delete) is record 61 / 62 / 63
    for name, (ops, _st) in ls.family("C").items():
        k = max(range(len(ops)), key=lambda i: ops[i][1][0][1])
        assert ops[k][1][0][1] > 1 and ls.records(ops[:k]) == int(name.rsplit("lane", 1)[1]), name
    # family D: the near miss is record pad + D_HEAD -- record 34 of the first window, or 64: the first past it
    for name, (ops, _st) in ls.family("D").items():
        pad = int(name.rsplit("pad", 1)[1])
        if "between_runs" in name:
            assert len(ops[pad + 10][1]) > 1, name
            continue
        head, miss = ops[pad:pad + ls.D_HEAD], ops[pad + ls.D_HEAD]
        assert ls.records(ops[:pad + ls.D_HEAD]) == pad + ls.D_HEAD and pad + ls.D_HEAD in (34, 64)
        assert all(a == 0 and len(tx) == 1 for a, tx in head), name
        (p0, _d0, _i0), (p1, _d1, i1) = head[-2][1][0], head[-1][1][0]
        go_on = (0, 0, i1) if i1 and p0 == p1 else (p1 + i1, 0, i1) if i1 else (2 * p1 - p0, 1, 0)  # what would continue the run
        if name.startswith("second_author"):
            assert miss == (1, [go_on]), name  # the very record that continues the run, by the other author
        else:
            assert miss[0] == 0 and miss[1] != [go_on], name
    assert {n for n in sc if "big_chunk" in n} == {"big_chunk_in_typing_pad30", "big_chunk_in_typing_pad60"}


@pytest.mark.parametrize("leaf", [32, 4])
def test_only_the_named_scripts_fail(leaf):
    # the error scripts are exactly the *_past_* runs and the all-empty-op txn; every other script
    # ends with status 0 on the oracle, so no case drops out of the comparisons silently
    assert ls.error_scripts() == sorted(
        [f"{k}_past_{e}_{n}" for k, e in (("forward", "end"), ("back", "start")) for n in ls.E_LENS] +
        [f"empty_txn_between_runs_pad{p}" for p in ls.D_PADS])
    for name, (_o, st) in ls.oracles(leaf).items():
        assert st == ls.scripts()[name][1], (name, st)
    for name in ls.error_scripts():
        assert ls.oracles(leaf)[name][1] == (ls.ERR_EMPTY_TXN if name.startswith("empty") else ls.ERR_POS_OOB)
    # the runs that meet the text's ends delete its last / first char: one record more is out of bounds
    for k in ls.E_LENS:
        assert len(ls.oracles(leaf)[f"forward_to_end_{k}"][0]) == ls.BASE - k
        assert ls.scripts()[f"back_past_start_{k}"][0][-1][1] == [(0xFFFFFFFF, 1, 0)]


# ------------------------------------------------------------------ emulator parity
@pytest.mark.parametrize("leaf", [32, 4])
@pytest.mark.parametrize("fam", list(ls.FAMILIES))
def test_emulator_matches_oracle(fam, leaf):
    L = _declare(emu_lib.lib())
    bad = []
    for name, (ops, want) in ls.family(fam).items():
        o, so = ls.oracles(leaf)[name]
        e = EmuDoc(leaf)
        se = run_agents(L, e.h, ops)
        if se != so or so != want:
            bad.append((name, "status", se, so, want))
        elif so == 0:
            if e.check() != "":
                bad.append((name, e.check()))
            d = diff_states(ls.oracle_exports(leaf)[name], e.export())
            if d:
                bad.append((name, d[0]))
            if e.sizes()["rec_pos"] != 1 + ls.records(ops):
                bad.append((name, "rec_pos", e.sizes()["rec_pos"], 1 + ls.records(ops)))
    assert not bad, (len(bad), bad[:12])


# ------------------------------------------------------------------ the branches are reached
APPLY_TXN, DEL_CALLS, DEL_TXNS = 47, 9, 12
TYPING_PAST, DELETE_PAST, FRONT_RUNS, FRONT_SPLIT, SPAN_OK, PIECES = 80, 81, 82, 83, 84, 85
TYPING_RUNS, TYPING_RUN_TXNS, DELETE_RUNS, DELETE_RUN_TXNS, FRONT_RUN_TXNS, D_PRE, C_PRE = 86, 87, 88, 89, 90, 91, 92


@pytest.fixture(scope="module")
def stats_lib(tmp_path_factory):
    # (`make stats` into a directory of this process: parallel test workers build side by side)
    td = str(tmp_path_factory.mktemp("emu_stats"))
    subprocess.run(["make", "-s", "-C", emu_lib.EMU_DIR, "stats", "BUILD=" + td], check=True)
    L = _declare(C.CDLL(os.path.join(td, "libemu_stats.so")))
    L.emu_stats.argtypes = [P(C.c_uint64), C.c_int]
    return L


def counters(L, ops, leaf, want=0):
    """the stream part's counters: the whole replay's less the base insert's alone (the replay is
    deterministic; the base insert, the document's first txn, is one apply_txn call)"""
    out = []
    for s in ([], ops):
        z = np.zeros(128, np.uint64)
        L.emu_stats(z.ctypes.data_as(P(C.c_uint64)), 1)
        h = L.emu_new(leaf)
        st = run_agents(L, h, s)
        L.emu_free(h)
        L.emu_stats(z.ctypes.data_as(P(C.c_uint64)), 1)
        out.append(z.astype(np.int64))
    assert st == want
    return out[1] - out[0]


@pytest.mark.parametrize("leaf", [32, 4])
def test_runs_go_on_past_the_window(stats_lib, leaf):
    """Behind the base insert a run of 130 begins in lane 1: the typing scan and the delete scan
    each go on past the window at least once (typing_scan_at / delete_scan_at) and the run is taken
    as ONE run of 130 txns; a front run is cut by the window and the leaf's room, taken in runs all
    the same, through prepends that find the leaf full (split_at(0)) at either layout."""
    sc = ls.scripts()
    for kind in ls.KINDS:
        z = counters(stats_lib, sc[f"run130_pad0_{kind}"][0], leaf)
        what = (kind, leaf, z[80:93].tolist())
        if kind.startswith("typing"):
            assert z[TYPING_PAST] >= 1 and z[TYPING_RUNS] == 1 and z[TYPING_RUN_TXNS] == 130, what
        elif kind in ("forward", "back"):
            assert z[DELETE_PAST] >= 1 and z[DELETE_RUNS] == 1 and z[DELETE_RUN_TXNS] == 130, what
            assert z[DEL_CALLS] == 1 and z[DEL_TXNS] == 130, what
        else:
            assert z[FRONT_RUNS] >= 2 and z[FRONT_SPLIT] >= 1 and z[FRONT_RUN_TXNS] >= 130, what
    # the same at every pad: the run of 130 is found from whichever lane it begins in
    for pad in ls.B_PADS:
        for kind, past in (("typing_mixed", TYPING_PAST), ("back", DELETE_PAST)):
            z = counters(stats_lib, sc[f"run130_pad{pad}_{kind}"][0], leaf)
            assert z[past] >= 1, (kind, pad, leaf)


def test_families_a_and_b_never_take_the_interpreter(stats_lib):
    # at leaf 32 every record of families A and B is taken by a fast path: apply_txn (counter 47)
    # runs for the base insert alone
    for fam in ("A", "B"):
        for name, (ops, _st) in ls.family(fam).items():
            z = counters(stats_lib, ops, 32)
            assert z[APPLY_TXN] == 0, (name, int(z[APPLY_TXN]))


@pytest.mark.parametrize("leaf", [32, 4])
def test_near_misses_make_two_runs(stats_lib, leaf):
    """Family D: the record that misses one term of the predicate cuts its run in two -- two runs of
    at least 2 txns (not one: the miss was not taken into the run; not singles: the scan took the
    rest), holding all the run's txns but the few next to the miss that start anew.  With the miss
    as the first record past the window (pad 60) the run is cut by the scan past the window."""
    n = ls.D_HEAD + ls.D_TAIL
    for name, (ops, want) in ls.family("D").items():
        z = counters(stats_lib, ops, leaf, want)
        what = (name, leaf, z[80:93].tolist())
        pad = int(name.rsplit("pad", 1)[1])
        if "between_runs" in name:
            assert z[TYPING_RUNS] == 1 and 9 <= z[TYPING_RUN_TXNS] <= 10, what
            assert z[DELETE_RUN_TXNS] == (10 if want == 0 else 0), what  # (an error stops the document: no second run)
        elif "typing" in name:
            assert z[TYPING_RUNS] == 2 and n - 2 <= z[TYPING_RUN_TXNS] <= n + 1, what
            assert pad == 30 or z[TYPING_PAST] >= 1, what
        elif "front" in name:
            assert z[FRONT_RUNS] >= 2 and z[FRONT_RUN_TXNS] >= n - 1, what
        else:
            assert z[DELETE_RUNS] == 2 and n - 2 <= z[DELETE_RUN_TXNS] <= n, what
            assert pad == 30 or z[DELETE_PAST] >= 1, what


@pytest.mark.parametrize("leaf", [32, 4])
def test_delete_spans_reach_both_span_paths(stats_lib, leaf):
    """Family C at each layout: leaf_delete_span places spans inside the cached leaf (with the
    deleted rest of the first entry joining a deleted run after it: before_deleted_run),
    local_delete_pieces takes the ones that leave it.  No local history makes the visible rest of a
    span's last entry join the entry after it (counter 92): that needs two visible neighbours with
    consecutive orders, the second's origin_left the first's last item and the same origin_right,
    and such items are applied back to back and merge when the second goes in."""
    tot = np.zeros(128, np.int64)
    for name, (ops, _st) in ls.family("C").items():
        z = counters(stats_lib, ops, leaf)
        what = (name, leaf, z[80:93].tolist())
        assert z[SPAN_OK] + z[PIECES] >= 1, what  # every span is taken by one of the two
        if "beyond_the_leaf" in name or "whole_document" in name:
            assert z[PIECES] >= 1, what
        if "before_deleted_run" in name:
            assert z[SPAN_OK] >= 1 and z[D_PRE] == 1, what
        tot += z
    print(leaf, tot[80:93].tolist())
    assert tot[SPAN_OK] >= 3 * 4 and tot[PIECES] >= 3 * 2 and tot[C_PRE] == 0
