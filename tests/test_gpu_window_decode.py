"""Window decode of k_replay (wave_gpu.h decode_window; DESIGN §4 "Window decode"): the fast paths
find how many compact remote records continue a typing run or a one-item delete run from the record
window's lanes and go on past the window's end (the *_scan_at continuations).  With the decode on
(the default) a typing run's length comes from a mask decoded once where the window moves; switched
off (crdt_set_window_decode), from a scan at every insert; delete runs are scanned either way.  How
a run is found must never change what is replayed: every case here runs with the switch on and off,
at both leaf layouts, and compares the full export with the oracle's, exactly.

A hand-built stream is staged on a document that already holds a base text (a first batch), so the
second batch is compact records only and record k of the stream sits in lane k of the first window:
runs are placed to start, end and cross at the window's first and last lanes, and past it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from crdt_amd.traces import load_remote_wire  # noqa: E402
from fuzz_gen import build_wire, parse_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from test_gpu_fused_publish import LAYOUTS, MICRO, golden_digest, micro_wire, oracle_of  # noqa: E402
from test_gpu_parity import assert_same  # noqa: E402

BASE = 600  # chars of the base text (one insert: one entry, one general-form txn)


class Doc:
    """a local edit script: one-op txns on a text whose length is tracked"""

    def __init__(self, n=BASE):
        self.n = n
        self.ops = []

    def typing(self, pos, k):  # k chars typed from pos on: the first lands at pos, the others continue it
        self.ops += [(pos + i, 0, 1) for i in range(k)]
        self.n += k
        return self

    def forward(self, pos, k):  # k forward deletes at pos
        assert pos + k <= self.n
        self.ops += [(pos, 1, 0)] * k
        self.n -= k
        return self

    def back(self, pos, k):  # k backspaces, the first deleting the char at pos
        assert k - 1 <= pos < self.n
        self.ops += [(pos - i, 1, 0) for i in range(k)]
        self.n -= k
        return self

    def jumps(self, k):  # k single inserts, no two neighbours: records that continue nothing
        for i in range(k):
            self.ops.append((7 + (i % 2) * (self.n // 2) + 3 * (i // 2), 0, 1))
            self.n += 1
        return self

    def run(self, kind, k):
        if kind == "typing":
            return self.typing(self.n, k)  # at the end of the text: origin_right ROOT, appends to the last entry
        if kind == "typing_mid":
            return self.typing(self.n // 3, k)  # inside an entry: an insert, then the typing that appends to it
        if kind == "forward":
            return self.forward(self.n // 2 - k // 2, k)
        return self.back(self.n // 2 + k // 2, k)


KINDS = ["typing", "typing_mid", "forward", "back"]


def scripts():
    """name -> Doc, the hand-built streams"""
    out = {}
    # 1. streams of 1, 63, 64, 65 and 129 records, one run each
    for n in (1, 63, 64, 65, 129):
        for kind in KINDS:
            out[f"stream{n}_{kind}"] = Doc().run(kind, n)
    # 2. runs of 1, 2, 63, 64, 65 and 130 records behind 0..64 records that continue nothing (the run
    #    then starts at lane 0, 1, 30 or 61 of a window, or the window moves to it), and followed
    #    by records that end it: runs end at lanes 62, 63 and past the window
    for n in (1, 2, 63, 64, 65, 130):
        for pad in (0, 1, 30, 61, 62, 64):
            for kind in KINDS:
                out[f"run{n}_pad{pad}_{kind}"] = Doc().jumps(pad).run(kind, n).jumps(3)
    # 3. delete runs cut short by the room of their entry: a char typed into the base text splits
    #    it into three entries, and the runs cross the pieces mid-window
    out["cut_back"] = Doc().typing(100, 1).back(110, 30).jumps(2)
    out["cut_forward"] = Doc().typing(100, 1).forward(90, 30).jumps(2)
    out["cut_both"] = Doc().typing(100, 3).typing(300, 2).back(310, 25).forward(95, 20).back(99, 12)
    # 4. an insert run followed directly by a backspace run over it, and mixed neighbours
    out["type_then_back"] = Doc().typing(200, 10).back(209, 10).typing(50, 5).back(54, 8)
    d = Doc().typing(BASE, 70)
    out["type_back_at_end"] = d.back(d.n - 1, 75)
    out["mixed"] = Doc().typing(300, 20).forward(100, 20).typing(100, 20).back(400, 20).forward(0, 5).typing(0, 5)
    # 6. an insert at the start of the text (origin_left ROOT) and typing at its end (origin_right ROOT)
    out["root_left"] = Doc().typing(0, 12).jumps(2)
    out["root_right"] = Doc().jumps(2).typing(BASE + 2, 66)
    # longer inserts and deletes (len > 1) between one-item runs
    d = Doc()
    d.ops += [(10, 0, 5), (15, 0, 1), (16, 0, 3), (19, 0, 1), (40, 3, 0), (40, 1, 0), (40, 1, 0), (39, 1, 0), (38, 2, 0)]
    out["long_ops"] = d
    return out


def _ones(ops):
    return np.ones(len(ops), np.uint32), np.array(ops, np.uint32).reshape(-1, 3)


def _wire_of_local(doc, agent, counts, patches):
    """the remote wire of `agent`'s local txns applied to oracle `doc` (and applies them); these
    scripts are a few hundred txns: a small buffer"""
    import ctypes as C
    from oracle_lib import _p, lib
    buf = C.create_string_buffer(1 << 18)
    n = lib().orc_local_trace_to_wire(doc.h, agent, counts.shape[0], _p(counts), _p(patches), C.cast(buf, C.c_void_p), 1 << 18)
    assert n > 0
    return buf.raw[:n]


@functools.lru_cache(maxsize=None)
def wires():
    """name -> (base batch, stream batch): built once, the same for both leaf layouts"""
    out = {}
    for name, doc in scripts().items():
        o = OracleDoc()
        a = o.agent("jeremy")
        w0 = _wire_of_local(o, a, *_ones([(0, 0, BASE)]))
        out[name] = (w0, _wire_of_local(o, a, *_ones(doc.ops)))
    # 5. a second author and general-form txns in the middle of a window: alice types, bob (who has
    #    alice's text) edits, alice merges bob and goes on (her next txn has bob's as its parent);
    #    and a replace op (delete + insert: a two-op general-form txn) between two runs
    o1, o2 = OracleDoc(), OracleDoc()
    a = o1.agent("alice")
    w0 = _wire_of_local(o1, a, *_ones([(0, 0, BASE)]))
    wa1 = _wire_of_local(o1, a, *_ones(Doc().typing(BASE, 20).back(BASE + 19, 6).ops))
    assert o2.apply_remote_wire(w0) == 0 and o2.apply_remote_wire(wa1) == 0
    wb = _wire_of_local(o2, o2.agent("bob"), *_ones(Doc(len(o2)).typing(50, 6).back(55, 3).forward(10, 4).ops))
    assert o1.apply_remote_wire(wb) == 0
    wa2 = _wire_of_local(o1, a, *_ones(Doc(len(o1)).typing(300, 12).forward(200, 9).back(150, 9).ops))
    out["two_authors"] = (w0, build_wire(parse_wire(wa1)[1] + parse_wire(wb)[1] + parse_wire(wa2)[1]))
    o = OracleDoc()
    a = o.agent("jeremy")
    w0 = _wire_of_local(o, a, *_ones([(0, 0, BASE)]))
    ops = Doc().typing(BASE, 20).ops + [(100, 2, 3)] + Doc(BASE + 21).forward(300, 10).typing(20, 10).ops
    out["replace_between_runs"] = (w0, _wire_of_local(o, a, *_ones(ops)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_exports(leaf):
    """name -> the oracle's export after both batches, computed once per leaf layout"""
    out = {}
    for name, (w0, w1) in wires().items():
        o = OracleDoc(*LAYOUTS[leaf])
        assert o.apply_remote_wire(w0) == 0 and o.apply_remote_wire(w1) == 0, name
        out[name] = o.export()
    return out


def test_stream_shapes():
    # the hand-built batches are what they claim: one one-op txn (one compact record) per edit, each
    # by the base text's author with its previous txn as the only parent
    for name, n in (("stream1_typing", 1), ("stream129_back", 129), ("run130_pad61_typing", 61 + 130 + 3)):
        txns = parse_wire(wires()[name][1])[1]
        assert len(txns) == n
        assert all(len(ops) == 1 and ps == [(a, s - 1)] and s >= BASE for a, s, ps, ops in txns)
    assert {t[0] for t in parse_wire(wires()["two_authors"][1])[1]} == {"alice", "bob"}


ON_OFF = pytest.mark.parametrize("on", [True, False], ids=["decode", "scan"])


@ON_OFF
@pytest.mark.parametrize("leaf", [32, 4])
def test_hand_built_streams(leaf, on):
    ws = wires()
    names = sorted(ws)
    docs = list(range(len(names)))
    e = crdt_amd.Engine(len(names), leaf)
    e.window_decode(on)
    assert (e.apply_remote_wire(docs, [ws[n][0] for n in names]) == 0).all()
    st = e.apply_remote_wire(docs, [ws[n][1] for n in names])
    assert (st == 0).all(), [names[i] for i in np.flatnonzero(st)]
    want = oracle_exports(leaf)
    bad = []
    for d, n in enumerate(names):
        try:
            assert_same(e.export(d), want[n])
        except AssertionError as x:
            bad.append((n, " ".join(str(x).split())[:60]))
    e.close()
    assert not bad, (len(bad), bad)


@ON_OFF
@pytest.mark.parametrize("leaf", [32, 4])
def test_micro_wires_and_automerge_paper(leaf, on):
    # 7. the per-path micro workloads and the flagship trace on 4 documents, through crdt_run (growth
    # stops that resume mid-stream) and then the benchmark's steady step on the fitted engine
    ms = list(MICRO)
    n = len(ms) + 4
    e = crdt_amd.Engine(n, leaf)
    e.window_decode(on)
    ap = load_remote_wire("automerge-paper")
    e.apply_remote_wire(list(range(n)), [micro_wire(m) for m in ms] + [ap] * 4, stage_only=True)
    want = [oracle_of(m, leaf)[0] for m in ms] + [golden_digest("automerge-paper", leaf)] * 4
    assert (e.run() == 0).all()
    assert [int(x) for x in e.digests()] == want
    e.publish_async()
    e.fit()
    e.reset_async()
    e.run_async()
    e.publish_async()
    e.sync()
    assert (e.status() == 0).all()
    assert [int(x) for x in e.digests()] == want
    for d, m in enumerate(ms):
        assert np.array_equal(e.export(d)["canon"], oracle_of(m, leaf)[2]), m
    e.close()


def test_switch_takes_effect_per_launch():
    # one engine, the same stream replayed with the decode on, off and on again: the same digest
    e = crdt_amd.Engine(2, 32)
    e.apply_remote_wire([0, 1], [micro_wire("jump10"), micro_wire("typing")], stage_only=True)
    assert (e.run() == 0).all()
    want = e.digests()
    e.publish_async()
    e.fit()
    for on in (False, True):
        e.window_decode(on)
        e.reset_async()
        e.run_async()
        e.publish_async()
        e.sync()
        assert (e.status() == 0).all() and np.array_equal(e.digests(), want)
    e.close()
