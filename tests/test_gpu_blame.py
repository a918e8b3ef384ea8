"""GPU checks of the authorship runs (crdt_blame_async: k_blame, k_result_scan<BlameRes>) through the C ABI.
Every result must equal tests/blame_ref.py's ref_blame of the engine's own export exactly, so agent
ids are the engine's.

k_blame walks 256 canonical spans of a document per loop pass (kernels.h DIFF_T), 64 per wave.
"""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from blame_ref import expand, ref_blame  # noqa: E402
from fuzz_gen import build_wire, concurrent_wire, parse_wire  # noqa: E402
from test_diff_ref import double_delete_txns  # noqa: E402

WAVE, PASS = 64, 256  # canonical spans per wave / per pass of k_blame's per-workgroup loop
NO_RESULT = 0xFFFFFFFF
MODES = ("agent", "id")
CARRY_SEED, CARRY_OPS = 6, 500  # the carries' fixture (carry_ops), chosen on the CPU oracle


def same_as_ref(e, d, mode, got, ex=None):
    want = ref_blame(ex if ex is not None else e.export(d), mode)
    assert got.shape == want.shape and np.array_equal(got, want), (d, mode, got[:8], want[:8])
    return want.shape[0]


def check_all(e, docs, exports=None):
    """one blame call per mode over docs, each result against the reference; returns {mode: results}"""
    exports = exports if exports is not None else {d: e.export(d) for d in docs}
    out = {}
    for mode in MODES:
        res = e.blame(docs, mode)
        assert len(res) == len(docs)
        for i, d in enumerate(docs):
            same_as_ref(e, d, mode, res[i], exports[d])
        out[mode] = res
    return out


def crossings(ex, runs, step):
    """span indexes k, multiples of `step`, where the run of the first visible item at or after
    span k began before it: a run that crosses the boundary"""
    canon = ex["canon"]
    ln = canon[:, 3].astype(np.int32)
    vis = np.where(ln > 0, ln, 0)
    vpos = np.concatenate([[0], np.cumsum(vis)])
    starts = set(int(x) for x in runs[:, 0])
    out = []
    for k in range(step, canon.shape[0], step):
        later = np.flatnonzero(vis[k:] > 0)
        if later.size and vpos[k] > 0 and int(vpos[k + later[0]]) not in starts:
            out.append(k)
    return out


@pytest.mark.parametrize("leaf", [32, 4])
def test_every_prefix_of_a_tiny_history(leaf):
    txns = parse_wire(concurrent_wire(3)[0])[1]
    n = len(txns)
    e = crdt_amd.Engine(n + 1, leaf)
    assert (e.apply_remote_wire(list(range(1, n + 1)), [build_wire(txns[:k]) for k in range(1, n + 1)]) == 0).all()
    docs = list(range(n + 1))
    res = check_all(e, docs)
    for mode in MODES:
        assert res[mode][0].shape == (0, 4)  # the empty document
        assert res[mode][1][:, :2].tolist() == [[0, int(e.lens([1])[0])]]  # the base txn alone: one author
    runs = res["id"][n]
    ln = int(e.lens([n])[0])
    assert int(runs[:, 1].sum()) == ln and runs.shape[0] > res["agent"][n].shape[0] > 3
    ga, gs = e.pos_to_loc(np.full(ln, n, np.uint32), np.arange(ln, dtype=np.uint32))
    agents, seqs = expand(runs, "id")
    assert agents == [int(x) for x in ga] and seqs == [int(x) for x in gs]


def carry_ops(seed=CARRY_SEED, n_ops=CARRY_OPS):
    """one-op txns that keep most of what they type: 3 in 4 insert 1..3 characters at a random
    position, the others delete 1..3.  Most inserts split a span, so spans outnumber the ops."""
    rng = random.Random(seed)
    n, ops = 0, []
    for _ in range(n_ops):
        if n < 4 or rng.random() < 0.75:
            k = rng.randint(1, 3)
            ops.append([(rng.randint(0, n), 0, k)])
            n += k
        else:
            pos = rng.randint(0, n - 1)
            k = rng.randint(1, min(3, n - pos))
            ops.append([(pos, k, 0)])
            n -= k
    return ops


def interleaved_ops(xa, yb, n=300, keep=7):
    """xa types n characters in one txn; yb puts a character between every two of them; all of
    those but every `keep`-th are deleted again.  2n - 1 canonical spans of one item; xa's items
    chain over the tombstones in ID mode too (consecutive seqs)."""
    tx = [(xa, [(0, 0, n)])]
    tx += [(yb, [(2 * j + 1, 0, 1)]) for j in range(n - 1)]
    tx += [(xa, [(2 * j + 1, 1, 0)]) for j in range(n - 2, -1, -1) if j % keep != 5]
    return tx


def test_carries_across_lanes_waves_and_passes():
    ops = carry_ops()
    e = crdt_amd.Engine(5, 32)
    ag = [int(e.agent_intern([0, 3, 4], [name] * 3)[0]) for name in ("xa", "yb", "zc")]
    one = int(e.agent_intern([2], ["xa"])[0])
    multi = [(ag[j % 3], op) for j, op in enumerate(ops)]
    single = [(ag[0], op) for op in ops]
    st = e.apply_local([(0, multi), (2, [(one, [(0, 0, 1)])]), (3, single),   # document 1 stays empty
                        (4, interleaved_ops(ag[0], ag[1]))])
    assert (st == 0).all()
    cn = e.canon_counts()
    assert cn[0] > 2 * PASS and cn[0] == cn[3] and cn[4] > 2 * PASS, cn  # at least 3 passes
    docs = [0, 1, 2, 3, 4]
    exports = {d: e.export(d) for d in docs}
    res = check_all(e, docs, exports)
    # the fixtures exercise both carries: a run crosses a wave's boundary that is no pass boundary,
    # and a pass boundary (document 0 by its authors' luck in AGENT mode; document 4 in both modes)
    for d, mode in ((0, "agent"), (4, "agent"), (4, "id")):
        cw = crossings(exports[d], res[mode][d], WAVE)
        assert [k for k in cw if k % PASS] and [k for k in cw if k % PASS == 0], (d, mode, cw)
    for mode in MODES:
        assert res[mode][1].shape == (0, 4)
        assert res[mode][2].tolist() == [[0, 1, one, 0]]
        assert 20 < res[mode][4].shape[0] < 100
    ln = int(e.lens([3])[0])
    visible = int((exports[3]["canon"][:, 3].astype(np.int32) > 0).sum())
    assert visible > 100 and ln > 0
    assert res["agent"][3].tolist() == [[0, ln, ag[0], int(res["id"][3][0, 3])]]  # one author: one run over every span
    assert res["agent"][0].shape[0] > 10 and res["id"][0].shape[0] > res["agent"][0].shape[0]


def alternating(agents, n, start=0):
    return [(agents[j % 2], [(start + j, 0, 1)]) for j in range(n)]


def test_one_span_over_many_client_runs():
    # two authors alternately append one character each: one canonical span over 700
    # client_with_order runs, 700 runs in both modes.  Alone, as the middle of three listed
    # documents, and with 300 ordinary spans typed before and after it by a third author (inserts
    # at position 0 make a span each), so the long span sits inside a pass next to ordinary lanes
    e = crdt_amd.Engine(4, 32)
    docs = [0, 1, 2, 3]
    xa, yb, zc = (e.agent_intern(docs, [name] * 4) for name in ("xa", "yb", "zc"))
    per = []
    for d in docs:
        a = [int(xa[d]), int(yb[d])]
        z = int(zc[d])
        if d == 0:
            per.append((d, alternating(a, 700)))
        elif d == 1:
            per.append((d, [(z, [(0, 0, 3)])]))
        elif d == 2:
            per.append((d, [(a[0], [(0, 0, 5)]), (z, [(2, 0, 1)])]))
        else:
            tx = [(z, [(0, 0, 1)]) for _ in range(300)]
            tx += alternating(a, 700, 300)
            tx += [(z, [(1000, 0, 1)])] + [(z, [(1000, 0, 1)]) for _ in range(299)]
            per.append((d, tx))
    assert (e.apply_local(per) == 0).all()
    cn = e.canon_counts()
    assert cn[0] == 1 and e.export_sizes(0)["cwo"] == 700
    assert cn[3] > 2 * PASS, cn
    ex3 = e.export(3)
    assert int(np.abs(ex3["canon"][:, 3].astype(np.int32)).max()) >= 700  # the long span survived whole
    for mode in MODES:
        alone = e.blame([0], mode)
        assert same_as_ref(e, 0, mode, alone[0]) == 700
        res = e.blame([1, 0, 2], mode)
        assert np.array_equal(res[1], alone[0])
        same_as_ref(e, 1, mode, res[0])
        same_as_ref(e, 2, mode, res[2])
        wide = e.blame([3], mode)[0]
        same_as_ref(e, 3, mode, wide, ex3)
        assert wide.shape[0] >= 702


@pytest.mark.parametrize("swap", [False, True])
def test_tombstones_and_double_deletes(swap):
    txns = double_delete_txns()
    if swap:
        txns = [txns[0], txns[2], txns[1]]
    e = crdt_amd.Engine(2, 32)
    xa, yb = int(e.agent_intern([0], ["xa"])[0]), int(e.agent_intern([0], ["yb"])[0])
    # xa types 10 characters, yb inserts 2 in the middle, and they are then deleted
    assert e.apply_local([(0, [(xa, [(0, 0, 10)]), (yb, [(5, 0, 2)]), (xa, [(5, 2, 0)])])])[0] == 0
    assert (e.apply_remote_wire([1], [build_wire(txns)]) == 0).all()
    assert e.canon_counts()[0] == 3
    res = check_all(e, [0, 1])
    for mode in MODES:
        assert res[mode][0].tolist() == [[0, 10, xa, 0]]
    a = int(res["agent"][1][0, 2])
    assert res["agent"][1].tolist() == [[0, 4, a, 0]]                # 0 1 8 9 remain
    assert res["id"][1].tolist() == [[0, 2, a, 0], [2, 2, a, 8]]


def test_listed_subset_replacement_and_copies():
    e = crdt_amd.Engine(6, 32)
    wires = [concurrent_wire(s)[0] for s in range(6)]
    assert (e.apply_remote_wire(list(range(6)), wires) == 0).all()
    dg = e.digests()
    docs = [5, 0, 3]
    first = e.blame(docs, "id")
    for i, d in enumerate(docs):
        assert same_as_ref(e, d, "id", first[i]) > 3
    assert e.blame_counts().shape[0] == 3
    # a blame changes no document
    assert np.array_equal(e.digests(), dg)
    # the result is a copy: replaying documents afterwards (listed or not) does not change it
    ag = e.agent_intern([0, 1], ["late"] * 2)
    assert (e.apply_local([(0, [(int(ag[0]), [(0, 0, 4)])]), (1, [(int(ag[1]), [(1, 2, 0)])])]) == 0).all()
    for i in range(3):
        assert np.array_equal(e.blame_read(i), first[i])
    # a second call replaces the first one's result
    second = e.blame([1, 0], "agent")
    assert e.blame_counts().shape[0] == 2
    same_as_ref(e, 1, "agent", second[0])
    same_as_ref(e, 0, "agent", second[1])
    assert second[1][0].tolist()[:2] == [0, 4]  # the late author's 4 characters at the front
    assert np.array_equal(e.blame_read(1), second[1])
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.blame_read(2)


def test_errors():
    wire, _ = concurrent_wire(1)
    e = crdt_amd.Engine(4, 32)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.blame_read(0)  # before any blame
    assert (e.apply_remote_wire([0, 2, 3], [wire] * 3) == 0).all()
    ag = int(e.agent_intern([1], ["p"])[0])
    bad = [[(0, 0, 5)], [(2, 1, 0)], [(3, 5, 0)], [(0, 0, 1)]]      # the third txn deletes past the end
    assert e.apply_local([(1, [(ag, o) for o in bad])])[0] == -1
    docs = [0, 1, 2, 3]
    res = e.blame(docs, "id", strict=False)
    counts = e.blame_counts()
    assert [int(x) == NO_RESULT for x in counts] == [False, True, False, False]
    assert res[1] is None
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.blame_read(1)
    for i in (0, 2, 3):  # the neighbours' results are intact
        same_as_ref(e, i, "id", res[i])
        same_as_ref(e, i, "id", e.blame_read(i))
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.blame(docs, "id")  # strict
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.blame_read(4)  # out of range
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.blame([0, 0], "agent")  # a document named twice
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.blame([0, 7], "agent")  # no such document
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.blame_async([0], 2)  # no such mode
    # the engine still answers
    same_as_ref(e, 3, "agent", e.blame([3], "agent")[0])


def test_allocation_failure_leaves_the_engine_usable():
    wire, _ = concurrent_wire(2)
    L = crdt_amd.lib()
    failed = 0
    for k in range(16):  # the first blame of an engine allocates every buffer it needs: fail each in turn
        before = crdt_amd.Engine.device_bytes()[0]
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        dg = e.digests()
        L.crdt_test_fail_alloc_after(k)
        try:
            e.blame([0, 1], "id")
            ok = True
        except crdt_amd.CrdtError as x:
            assert "rc=-102" in str(x), x
            ok = False
        finally:
            L.crdt_test_fail_alloc_after(-1)
        if not ok:
            failed += 1
            # no relayout was involved: the engine is not poisoned and the same blame then succeeds
            with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                e.blame_read(0)  # without a blame result
            assert np.array_equal(e.digests(), dg)
            res = e.blame([0, 1], "id")
            same_as_ref(e, 0, "id", res[0])
            same_as_ref(e, 1, "id", res[1])
        e.close()
        now = crdt_amd.Engine.device_bytes()[0]
        assert now <= before, (k, now, before)  # nothing of a closed engine stays allocated
        if ok:
            break
    assert 1 <= failed < 16, failed


def test_blame_ms_and_the_one_document_wrapper():
    doc = crdt_amd.ListCRDT()
    a, b = doc.get_or_create_agent_id("xa"), doc.get_or_create_agent_id("yb")
    assert doc.local_insert(a, 0, 6) == 0 and doc.local_insert(b, 3, 2) == 0 and doc.local_delete(a, 0, 1) == 0
    assert doc.blame("agent").tolist() == [[0, 2, a, 1], [2, 2, b, 0], [4, 3, a, 3]]
    assert doc.blame("id").tolist() == [[0, 2, a, 1], [2, 2, b, 0], [4, 3, a, 3]]
    assert doc.blame().tolist() == doc.blame("agent").tolist()
    assert doc.e.blame_ms() > 0
