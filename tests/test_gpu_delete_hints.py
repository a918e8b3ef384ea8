"""Delete-run hints in k_replay (replay_core.h fast_deletes; DESIGN §4 "Delete-run hints"): for a
compact remote delete the kernel takes the run's length and direction from the record's w3, written
by the encoder (tests/test_delete_hints.py checks the encoder), and no longer reads the following
records.  What depends on the document's state still cuts the run in the kernel: the entry's room,
the author's last item_orders run, the tables' room, the leaf's room.  Every case compares the full
export with the oracle's, exactly, at both leaf layouts: once staged in batches on a planned
(not fitted) engine, where tables grow and the replay resumes inside a run, and once as a single
batch replayed again on the fitted engine (the benchmark's steady step)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from crdt_amd.traces import load_remote_wire  # noqa: E402
from fuzz_gen import build_wire, parse_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from test_gpu_fused_publish import LAYOUTS, golden_digest, micro_wire, oracle_of  # noqa: E402
from test_gpu_parity import assert_same  # noqa: E402
from test_gpu_window_decode import BASE, Doc, _ones, _wire_of_local  # noqa: E402

AUTHOR = "jeremy"


def _deletes(seq, targets):
    """one-item-per-op delete txns by AUTHOR on his own items, written directly: [(target seq, len)],
    each txn with his previous one as its only parent (a target may be deleted already: a double delete)"""
    txns = []
    for t, ln in targets:
        txns.append((AUTHOR, seq, [(AUTHOR, seq - 1)], [(1, AUTHOR, t, None, 0, ln)]))
        seq += ln
    return build_wire(txns)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> the batches of one document, in staging order"""
    def base(n=BASE):
        o = OracleDoc()
        a = o.agent(AUTHOR)
        return o, a, _wire_of_local(o, a, *_ones([(0, 0, n)]))

    def of(doc, n=BASE):
        o, a, w0 = base(n)
        return [w0, _wire_of_local(o, a, *_ones(doc.ops))]
    out = {}
    # runs of 1 .. 130 records behind 0, 1, 61 and 64 records that continue nothing: the run starts
    # at the first, second or last-but-two lane of a record window or past it, and crosses its end
    for n in (1, 2, 63, 64, 65, 130):
        for pad in (0, 1, 61, 64):
            for kind in ("back", "forward"):
                out[f"run{n}_pad{pad}_{kind}"] = of(Doc().jumps(pad).run(kind, n).jumps(3))
    # a backspace run that turns into a forward run and back, as edits (the targets jump where it
    # turns) and as target steps -1 -1 +1 +1 -1 (the last three delete deleted items again)
    out["flip_edits"] = of(Doc().back(300, 3).forward(298, 2).back(297, 2).forward(100, 1).back(99, 4))
    out["flip_steps"] = [base()[2], _deletes(BASE, [(t, 1) for t in (300, 299, 298, 299, 300, 299)])]
    # a len-2 delete in the middle of len-1 deletes, where it would continue the run and where not
    out["len2_back"] = [base()[2], _deletes(BASE, [(300, 1), (299, 1), (298, 1), (296, 2), (295, 1), (294, 1), (293, 1)])]
    out["len2_forward"] = [base()[2], _deletes(BASE, [(300, 1), (301, 1), (302, 2), (304, 1), (305, 1)])]
    d = Doc()
    d.ops += [(40, 1, 0), (40, 1, 0), (40, 2, 0), (40, 1, 0), (39, 1, 0), (37, 2, 0), (36, 1, 0)]
    out["len2_edits"] = of(d)
    # runs cut by the room of their entry: a char typed into the base text splits it into three
    # entries, and the runs cross the pieces
    out["cut_back"] = of(Doc().typing(100, 1).back(110, 30).jumps(2))
    out["cut_forward"] = of(Doc().typing(100, 1).forward(90, 30).jumps(2))
    out["cut_both"] = of(Doc().typing(100, 3).typing(300, 2).back(310, 25).forward(95, 20).back(99, 12))
    # a run whose targets leave the author's last item_orders run: the base text typed in two
    # halves with bob's txn merged between them, then one backspace run across the seam (its seqs
    # and target seqs go on evenly; the orders behind them do not)
    o1, o2 = OracleDoc(), OracleDoc()
    a = o1.agent(AUTHOR)
    w0 = _wire_of_local(o1, a, *_ones([(0, 0, 300)]))
    assert o2.apply_remote_wire(w0) == 0
    wb = _wire_of_local(o2, o2.agent("bob"), *_ones([(10, 0, 5)]))
    assert o1.apply_remote_wire(wb) == 0
    seam = [(305, 0, 300)] + Doc(605).back(312, 20).forward(400, 3).ops
    out["seam"] = [w0, wb, _wire_of_local(o1, a, *_ones(seam))]
    # a run split over two staged batches: the first batch's hints stop at its end
    o, a, w0 = base()
    out["two_batches"] = [w0, _wire_of_local(o, a, *_ones(Doc().back(400, 20).ops)),
                          _wire_of_local(o, a, *_ones(Doc(BASE - 20).back(380, 20).jumps(2).ops))]
    o, a, w0 = base()
    out["two_batches_forward"] = [w0, _wire_of_local(o, a, *_ones(Doc().forward(200, 70).ops)),
                                  _wire_of_local(o, a, *_ones(Doc(BASE - 70).forward(200, 70).ops))]
    # a backspace run long enough to split a 32-entry leaf more than once (closed-form cycles)
    out["back200"] = of(Doc().back(450, 200).jumps(2))
    # ... and one that outgrows the planned leaves of the 4-entry layout: the replay stops inside
    # the run on capacity and resumes at a record in its middle
    out["back700"] = of(Doc(1000).back(900, 700), 1000)
    return out


@functools.lru_cache(maxsize=None)
def oracle_exports(leaf):
    out = {}
    for name, ws in cases().items():
        o = OracleDoc(*LAYOUTS[leaf])
        for w in ws:
            assert o.apply_remote_wire(w) == 0, name
        out[name] = o.export()
    return out


def _compare(e, names, want):
    bad = []
    for d, n in enumerate(names):
        try:
            assert_same(e.export(d), want[n])
        except AssertionError as x:
            bad.append((n, " ".join(str(x).split())[:60]))
    assert not bad, (len(bad), bad)


@pytest.mark.parametrize("leaf", [32, 4])
def test_runs_staged_in_batches(leaf):
    cs = cases()
    names = sorted(cs)
    e = crdt_amd.Engine(len(names), leaf)
    for b in range(max(len(ws) for ws in cs.values())):
        docs = [d for d, n in enumerate(names) if len(cs[n]) > b]
        st = e.apply_remote_wire(docs, [cs[names[d]][b] for d in docs])
        assert (st == 0).all(), (b, [names[docs[i]] for i in np.flatnonzero(st)])
    _compare(e, names, oracle_exports(leaf))
    e.close()


@pytest.mark.parametrize("leaf", [32, 4])
def test_runs_in_one_batch_then_fitted(leaf):
    cs = cases()
    names = sorted(cs)
    docs = list(range(len(names)))
    e = crdt_amd.Engine(len(names), leaf)
    one = [build_wire([t for w in cs[n] for t in parse_wire(w)[1]]) for n in names]
    e.apply_remote_wire(docs, one, stage_only=True)
    assert (e.run() == 0).all()
    want = oracle_exports(leaf)
    _compare(e, names, want)
    e.publish_async()
    e.fit()
    e.reset_async()
    e.run_async()
    e.publish_async()
    e.sync()
    assert (e.status() == 0).all()
    _compare(e, names, want)
    e.close()


@pytest.mark.parametrize("leaf", [32, 4])
def test_micro_wires_and_automerge_paper(leaf):
    # the delete micro workloads and the flagship trace on 4 documents against their golden digests,
    # through crdt_run (growth stops that resume mid-stream) and the steady step on the fitted engine
    ms = ["del1", "bs10", "bs200", "fd200"]
    n = len(ms) + 4
    e = crdt_amd.Engine(n, leaf)
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
