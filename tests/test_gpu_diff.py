"""GPU checks of the per-document diff (crdt_diff_async: k_diff_mark, k_diff, k_result_scan<DiffRes>) through
the C ABI.  Every result must equal tests/diff_ref.py's ref_diff of the engine's own export exactly;
where content is set, the patches with their ins_text, applied to the oracle's text of the earlier
version, must give the engine's current text.

k_diff walks 256 canonical spans of a document per loop pass (kernels.h DIFF_T).
"""
import gzip
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from crdt_amd.traces import content_by_order, load_trace  # noqa: E402
from diff_ref import apply_patches, ref_diff  # noqa: E402
from fuzz_gen import build_wire, concurrent_wire, parse_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from test_diff_ref import double_delete_txns  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIFF_PASS = 256  # canonical spans per pass of k_diff's per-workgroup loop
NO_RESULT = 0xFFFFFFFF


def same_as_ref(e, d, since, got):
    want_p, want_i = ref_diff(e.export(d), since)
    pat, io, _ = got
    assert pat.shape == want_p.shape and np.array_equal(pat, want_p), (d, since, pat[:8], want_p[:8])
    assert np.array_equal(io, want_i), (d, since)
    return want_p.shape[0]


def caps(leaf):
    return (leaf, 16 if leaf == 32 else 8)


@pytest.mark.parametrize("leaf", [32, 4])
def test_every_version_of_a_tiny_history(leaf):
    # document d of next_order + 1 copies of one concurrent history is diffed from version d: since
    # = 0, = version, inside txns, not a multiple of 32, and delete runs that straddle since
    wire, _ = concurrent_wire(3)
    o = OracleDoc(*caps(leaf))
    assert o.apply_remote_wire(wire) == 0
    n = o.sizes()["next_order"]
    assert 100 < n < 400
    e = crdt_amd.Engine(n + 1, leaf)
    e.stage_remote_replicated(wire, 0xFFFFFFFF, [""] * (n + 1))  # (no name of the batch is renamed)
    assert (e.run() == 0).all()
    assert (e.versions() == n).all()
    docs = np.arange(n + 1)
    res = e.diff(docs, docs)
    total = sum(same_as_ref(e, d, d, res[d]) for d in range(n + 1))
    assert total > n  # (many versions need several patches)
    assert res[n][0].shape[0] == 0 and res[n][1].shape[0] == 0    # since = version: nothing changed
    assert res[0][0].shape[0] == 1 and res[0][0][0].tolist() == [0, 0, len(o), 0]  # since = 0: the whole text
    assert e.diff_ms() > 0


def two_halves(e, docs, first, second, apply):
    """apply `first[i]` then `second[i]` to docs[i]; returns the versions in between"""
    assert (apply(e, docs, first) == 0).all()
    v = e.versions(docs)
    assert (apply(e, docs, second) == 0).all()
    return v


def check_text(e, d, since, got, old_text):
    pat, io, it = got
    assert it is not None and it.shape == io.shape
    assert np.array_equal(apply_patches(old_text, pat, it), e.text(d)), (d, since)


@pytest.mark.parametrize("leaf", [32, 4])
def test_text_of_a_trace_applied_in_two_halves(leaf):
    t = load_trace("sveltecomponent")
    k = t.n_txns // 2
    h = int(t.counts[:k].sum())
    e = crdt_amd.Engine(2, leaf)
    ag = int(e.agent_intern([0, 1], ["jeremy"] * 2)[0])
    assert (e.apply_trace([0, 1], ag, t.counts[:k], t.patches[:h]) == 0).all()
    v = e.versions()
    assert v[0] == v[1] and 0 < v[0]
    assert (e.apply_trace([0, 1], ag, t.counts[k:], t.patches[h:]) == 0).all()
    assert v[0] < e.versions()[0]
    c = content_by_order(t)
    e.set_content([0, 1], [0, 0], [c])
    assert e.canon_counts()[0] > 64 and e.versions()[0] > 64 * 32  # (many spans, many bitmap words)
    since = [int(v[0]), 0]
    res = e.diff([0, 1], since)
    assert same_as_ref(e, 0, since[0], res[0]) > 1
    assert same_as_ref(e, 1, 0, res[1]) == 1
    o = OracleDoc(*caps(leaf))
    assert o.apply_trace(o.agent("jeremy"), t.counts[:k], t.patches[:h]) == 0
    check_text(e, 0, since[0], res[0], o.text(c)[0])
    check_text(e, 1, 0, res[1], np.zeros(0, np.uint32))


@pytest.mark.parametrize("name", ["bs200", "del1", "jump10"])
def test_patterns(name):
    # backspace runs, single deletes, and jumps that make many small patches: a 50,000-char base
    # then 20,000 ops of one shape, cut at half the txns (inside the base) and in the middle of the ops
    with gzip.open(os.path.join(ROOT, "data", "micro", name + ".rtx.gz"), "rb") as f:
        txns = parse_wire(f.read())[1]
    cuts = [len(txns) // 2, 60000]
    e = crdt_amd.Engine(2, 32)
    st = e.apply_remote_wire([0, 1], [build_wire(txns[:k]) for k in cuts])
    assert (st == 0).all()
    v = e.versions()
    st = e.apply_remote_wire([0, 1], [build_wire(txns[k:]) for k in cuts])
    assert (st == 0).all()
    n = int(e.versions()[0])
    c = np.random.default_rng(7).integers(0x20, 0xD7FF, n, dtype=np.uint32)
    e.set_content([0, 1], [0, 0], [c])
    res = e.diff([0, 1], v)
    for d, k in enumerate(cuts):
        assert same_as_ref(e, d, int(v[d]), res[d]) > 1
        o = OracleDoc()
        assert o.apply_remote_wire(build_wire(txns[:k])) == 0
        assert o.sizes()["next_order"] == int(v[d])
        check_text(e, d, int(v[d]), res[d], o.text(c)[0])


@pytest.mark.parametrize("swap", [False, True])
def test_double_deletes(swap):
    txns = double_delete_txns()
    if swap:
        txns = [txns[0], txns[2], txns[1]]
    since = [14, 18, 12, 10, 0]  # after the first delete txn only; after both; inside it; before; empty
    e = crdt_amd.Engine(len(since), 32)
    assert (e.apply_remote_wire(list(range(len(since))), [build_wire(txns)] * len(since)) == 0).all()
    res = e.diff(list(range(len(since))), since)
    for d, v in enumerate(since):
        same_as_ref(e, d, v, res[d])
    # after the first delete txn the text is 0 1 6 7 8 9 (swapped: 0 1 2 3 8 9); now it is 0 1 8 9
    assert res[0][0].tolist() == [[2, 2, 0, 0]]
    assert res[1][0].shape[0] == 0
    assert res[3][0].tolist() == [[2, 6, 0, 0]]


def test_wide_document_with_an_empty_and_a_one_item_document():
    # 700 single-char inserts at position 0 are 700 canonical spans (document order is the reverse
    # of the orders); deletes and inserts in the middle split them further: at least two full
    # passes of k_diff's loop (DIFF_PASS spans each) and a remainder
    first = [[(0, 0, 1)] for _ in range(700)]
    second = [[(3 * j, 1, 0)] for j in range(100)] + [[(5 * j + 1, 0, 2)] for j in range(60)]
    e = crdt_amd.Engine(5, 32)
    ag = e.agent_intern(list(range(5)), ["w"] * 5)
    wide = [0, 3, 4]
    assert (e.apply_local([(d, [(int(ag[d]), op) for op in first]) for d in wide]) == 0).all()
    v = int(e.versions([0])[0])
    assert v == 700
    assert (e.apply_local([(d, [(int(ag[d]), op) for op in second]) for d in wide] +
                          [(2, [(int(ag[2]), [(0, 0, 1)])])]) == 0).all()
    cn = e.canon_counts()
    assert cn[0] >= 2 * DIFF_PASS + 1 and cn[0] % DIFF_PASS != 0, cn
    n = int(e.versions([0])[0])
    c = np.random.default_rng(11).integers(0x20, 0xD7FF, n, dtype=np.uint32)
    e.set_content(wide + [1, 2], [0] * 5, [c])
    docs = [0, 1, 2, 3, 4]
    since = [v, 0, 0, 0, 333]
    res = e.diff(docs, since)
    for d, s in zip(docs, since):
        same_as_ref(e, d, s, res[d])
    assert res[1][0].shape[0] == 0                       # the empty document
    assert res[2][0].tolist() == [[0, 0, 1, 0]]          # the one-item document
    assert res[0][0].shape[0] > DIFF_PASS // 2           # patches spread over every pass
    for d, s in ((0, v), (4, 333)):
        o = OracleDoc()
        a = o.agent("w")
        for op in first[:s]:
            assert o.apply_local(a, op) == 0
        check_text(e, d, s, res[d], o.text(c)[0])


def test_bitmap_past_the_lds_threshold():
    # k_diff_mark builds bitmaps of up to 16,384 words (524,256 orders) in LDS and larger ones with
    # atomics in HBM: a 600,000-char document on either side of a small one, in one call.  The
    # delete after the cut joins the 50,000 items deleted before it into one deleted span of
    # 50,200 items whose middle is marked (counted by a whole wave, kernels.h DIFF_LONG)
    first = [[(0, 0, 600_000)], [(1000, 50_000, 0)]]
    second = [[(5, 0, 10)], [(910, 200, 0)], [(200_000, 3, 0)], [(100, 300, 0)]]
    e = crdt_amd.Engine(3, 32)
    ag = e.agent_intern([0, 1, 2], ["big"] * 3)
    small = [[(0, 0, 40)], [(3, 5, 0)]]
    assert (e.apply_local([(0, [(int(ag[0]), op) for op in first]), (1, [(int(ag[1]), op) for op in small]),
                           (2, [(int(ag[2]), op) for op in first])]) == 0).all()
    v = e.versions()
    assert v[0] == 650_000 and v[0] // 32 + 1 > 16384 > v[1] // 32 + 1
    assert (e.apply_local([(0, [(int(ag[0]), op) for op in second]), (1, [(int(ag[1]), [(10, 2, 1)])]),
                           (2, [(int(ag[2]), op) for op in second])]) == 0).all()
    since = [int(v[0]), int(v[1]), 0]
    res = e.diff([0, 1, 2], since)
    assert same_as_ref(e, 0, since[0], res[0]) == 4
    assert same_as_ref(e, 1, since[1], res[1]) == 1
    assert same_as_ref(e, 2, 0, res[2]) == 1
    assert res[0][0][2].tolist() == [610, 200, 0, 10]  # 100 D items on either side of the 50,000 deleted before


def test_errors_and_purity():
    wire, _ = concurrent_wire(1)
    e = crdt_amd.Engine(4, 32)
    assert (e.apply_remote_wire([0, 2, 3], [wire] * 3) == 0).all()
    ag = int(e.agent_intern([1], ["p"])[0])
    bad = [[(0, 0, 5)], [(2, 1, 0)], [(3, 5, 0)], [(0, 0, 1)]]      # the third txn deletes past the end
    assert e.apply_local([(1, [(ag, o) for o in bad])])[0] == -1
    ver = e.versions()
    dg = e.digests()
    qd = np.array([0, 0, 2, 3, 3], np.uint32)
    qp = np.array([0, 5, 1, 2, int(e.lens()[3]) - 1], np.uint32)
    loc = e.pos_to_loc(qd, qp)
    docs, since = [0, 1, 2, 3], [5, 0, int(ver[2]) + 1, 0]
    res = e.diff(docs, since, strict=False)
    npat, nins = e.diff_counts()
    assert [int(x) == NO_RESULT for x in npat] == [False, True, True, False]
    assert [int(x) == NO_RESULT for x in nins] == [False, True, True, False]
    assert res[1] is None and res[2] is None
    for i in (1, 2):  # the poisoned document; since above the version
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.diff_read(i)
    # the neighbours' results are intact (and without content there is no ins_text)
    same_as_ref(e, 0, 5, res[0])
    same_as_ref(e, 0, 5, e.diff_read(0))
    same_as_ref(e, 3, 0, e.diff_read(3))
    assert res[0][2] is None and res[3][2] is None
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.diff(docs, since)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.diff([0, 0], [0, 0])  # a document named twice
    # a diff changes no document
    assert np.array_equal(e.digests(), dg)
    loc2 = e.pos_to_loc(qd, qp)
    assert np.array_equal(loc[0], loc2[0]) and np.array_equal(loc[1], loc2[1])
    assert np.array_equal(e.versions(), ver)
    # a second call replaces the first one's result
    res = e.diff([3], [7])
    npat, _ = e.diff_counts()
    assert npat.shape[0] == 1
    same_as_ref(e, 3, 7, res[0])
    same_as_ref(e, 3, 7, e.diff_read(0))
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.diff_read(1)


def test_allocation_failure_leaves_the_engine_usable():
    wire, _ = concurrent_wire(2)
    L = crdt_amd.lib()
    failed = 0
    for k in range(16):  # the first diff of an engine allocates every buffer it needs: fail each in turn
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        dg = e.digests()
        L.crdt_test_fail_alloc_after(k)
        try:
            e.diff([0, 1], [9, 0])
            ok = True
        except crdt_amd.CrdtError as x:
            assert "rc=-102" in str(x), x
            ok = False
        finally:
            L.crdt_test_fail_alloc_after(-1)
        if ok:
            e.close()
            break
        failed += 1
        # no relayout was involved: the engine is not poisoned and the same diff then succeeds
        assert np.array_equal(e.digests(), dg)
        res = e.diff([0, 1], [9, 0])
        same_as_ref(e, 0, 9, res[0])
        same_as_ref(e, 1, 0, res[1])
        e.close()
    assert 1 <= failed < 16, failed
