"""GPU checks of the patches between two versions (crdt_diff_between_async: k_diff_mark twice, k_diff2,
k_result_scan<DiffRes>) through the C ABI.  Every result must equal tests/diff_between_ref.py's
ref_diff_between of the engine's own export exactly; where content is set, the patches with their
ins_text, applied to the oracle's text at `from`, must give the oracle's text at `to`.

docs has no duplicates, so every (from, to) pair of a call has a document of its own.  k_diff2 walks
256 canonical spans of a document per loop pass (kernels.h DIFF_T), a span of up to 256 orders in
one lane and a longer one with the whole wave (DIFF2_LONG), 32 orders (one bitmap word) at a time.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from checkout_ref import ref_checkout  # noqa: E402
from diff_between_ref import ref_diff_between, ref_diff_between_arrays  # noqa: E402
from diff_ref import apply_patches  # noqa: E402
from fuzz_gen import build_wire, concurrent_wire, parse_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from rebase_ref import ref_rebase_table  # noqa: E402

DIFF_PASS = 256  # canonical spans per pass of k_diff2's per-workgroup loop
NO_RESULT = 0xFFFFFFFF


def same(got, want, what):
    pat, io = got[0], got[1]
    assert pat.shape == want[0].shape and np.array_equal(pat, want[0]), (what, pat[:8], want[0][:8])
    assert np.array_equal(io, want[1]), what
    return pat.shape[0]


def same_as_ref(e, d, a, b, got, ref=ref_diff_between):
    return same(got, ref(e.export(d), a, b), (d, a, b))


def caps(leaf):
    return (leaf, 16 if leaf == 32 else 8)


@pytest.mark.parametrize("leaf", [32, 4])
def test_every_ordered_pair_of_a_tiny_history(leaf):
    # the first 12 txns of a concurrent history, one copy per ordered pair of its versions: from and
    # to at 0, at the version, inside txns, on either side of the 32-order word, and delete runs
    # that straddle either
    txns = parse_wire(concurrent_wire(3)[0])[1][:12]
    wire = build_wire(txns)
    o = OracleDoc(*caps(leaf))
    assert o.apply_remote_wire(wire) == 0
    n = o.sizes()["next_order"]
    assert 40 <= n <= 62
    assert len({t[0] for t in txns}) >= 2
    assert np.asarray(o.export()["deletes"]).reshape(-1, 3).shape[0] >= 1
    nv = n + 1
    e = crdt_amd.Engine(nv * nv, leaf)
    e.stage_remote_replicated(wire, 0xFFFFFFFF, [""] * (nv * nv))  # (no name of the batch is renamed)
    assert (e.run() == 0).all()
    assert (e.versions() == n).all()
    dg = e.digests()
    assert (dg == dg[0]).all()  # the copies are one document: one export serves every reference
    ex = e.export(0)
    docs = np.arange(nv * nv)
    a, b = docs // nv, docs % nv
    res = e.diff_between(docs, a, b)
    total = mixed = 0
    for d in docs:
        pat = res[d][0]
        total += same(res[d], ref_diff_between(ex, a[d], b[d]), (a[d], b[d]))
        mixed += int(a[d] > b[d] and ((pat[:, 1] > 0) & (pat[:, 2] > 0)).any())
    assert total > nv * nv  # (many pairs need several patches)
    assert mixed > 0        # going back takes out and puts in within one patch
    for v in range(nv):     # the diagonal: nothing changed
        assert res[v * nv + v][0].shape[0] == 0 and res[v * nv + v][1].shape[0] == 0
    assert e.diff_ms() > 0
    # the column to = version is the diff, array for array
    col = docs[b == n]
    now = e.diff(col, a[col])
    for d, r in zip(col, now):
        same(res[d], r, ("pin", a[d]))


def test_word_boundaries_inside_one_span():
    # one 200-item span; single-char deletes, a txn each, of the items with orders 31, 32, 63, 64,
    # 95 and 96 (the last and the first order of a bitmap word), then of 129, 128 and 130 (one
    # deleted span in the end, whose middle goes first), then a few inserts.  from and to at every
    # version from the first delete on, both directions
    six = [31, 32, 63, 64, 95, 96]
    hit = six + [129, 128, 130]
    ops = [[(0, 0, 200)]]
    for k, x in enumerate(six):
        ops.append([(x - k, 1, 0)])  # k items before it are gone
    ops += [[(123, 1, 0)], [(122, 1, 0)], [(122, 1, 0)]]
    ops += [[(31, 0, 3)], [(100, 0, 2)], [(0, 0, 1)]]
    vs = [200 + k for k in range(len(hit) + 1)] + [212, 214, 215]
    nv = len(vs)
    e = crdt_amd.Engine(nv * nv, 32)
    ag = e.agent_intern(list(range(nv * nv)), ["w"] * (nv * nv))
    assert (e.apply_local([(d, [(int(ag[d]), op) for op in ops]) for d in range(nv * nv)]) == 0).all()
    assert (e.versions() == vs[-1]).all()
    ex = e.export(0)
    dl = np.asarray(ex["deletes"]).reshape(-1, 3)
    assert sorted(int(t) + j for _, t, ln in dl for j in range(int(ln))) == sorted(hit)  # (neighbouring deletes share a run)
    assert [128, 0xFFFFFFFF - 2] in np.asarray(ex["canon"], np.uint32).reshape(-1, 4)[:, [0, 3]].tolist()  # (one span, len -3)
    docs = np.arange(nv * nv)
    a, b = np.array(vs)[docs // nv], np.array(vs)[docs % nv]
    res = e.diff_between(docs, a, b)
    total = 0
    for d in docs:
        total += same(res[d], ref_diff_between(ex, a[d], b[d]), (a[d], b[d]))
    assert total > 2 * nv * nv
    # from before the deletes to after them: one patch per pair of neighbouring items
    assert res[6][0].tolist() == [[31, 2, 0, 0], [61, 2, 0, 0], [91, 2, 0, 0]]
    assert res[6 * nv][0].tolist() == [[31, 0, 2, 0], [63, 0, 2, 2], [95, 0, 2, 4]]
    assert res[6 * nv][1].tolist() == six
    # from after the nine deletes back to after the seventh: 128 and 130 return around 129, which stays deleted
    assert res[9 * nv + 7][0].tolist() == [[122, 0, 2, 0]] and res[9 * nv + 7][1].tolist() == [128, 130]


def test_several_passes_and_a_long_span():
    # 700 single-char inserts at position 0 are 700 canonical spans (document order is the reverse
    # of the orders); deletes and inserts all over the text split them further: two full passes of
    # k_diff2's loop (DIFF_PASS spans each) and a remainder.  Next to it an empty and a one-item
    # document
    first = [[(0, 0, 1)] for _ in range(700)]
    second = [[(6 * j, 1, 0)] for j in range(100)] + [[(9 * j + 1, 0, 2)] for j in range(60)]
    ops = first + second
    mid = 700 + 100 + 2 * 30  # the version after 130 of the second half's 160 txns
    end = 700 + 100 + 2 * 60
    cut = {0: 0, 333: 333, 700: 700, mid: 830, end: 860}  # version -> txns applied
    vs = list(cut)
    nv = len(vs)
    nd = nv * nv + 2
    empty, one = nv * nv, nv * nv + 1
    e = crdt_amd.Engine(nd, 32)
    ag = e.agent_intern(list(range(nd)), ["w"] * nd)
    assert (e.apply_local([(d, [(int(ag[d]), op) for op in ops]) for d in range(nv * nv)] +
                          [(one, [(int(ag[one]), [(0, 0, 1)])])]) == 0).all()
    assert int(e.versions([0])[0]) == end
    cn = e.canon_counts()
    assert cn[0] >= 2 * DIFF_PASS + 1 and cn[0] % DIFF_PASS != 0, cn
    c = np.random.default_rng(11).integers(0x20, 0xD7FF, end, dtype=np.uint32)
    e.set_content(list(range(nd)), [0] * nd, [c])
    docs = np.arange(nd)
    a = np.array([vs[d // nv] for d in range(nv * nv)] + [0, 1])
    b = np.array([vs[d % nv] for d in range(nv * nv)] + [0, 0])
    res = e.diff_between(docs, a, b)
    ex = e.export(0)
    for d in range(nv * nv):
        same(res[d], ref_diff_between(ex, a[d], b[d]), (a[d], b[d]))
    assert res[empty][0].shape[0] == 0                    # the empty document
    assert res[one][0].tolist() == [[0, 1, 0, 0]]         # the one-item document, back to nothing
    # (700, end): the patches' positions fall into the spans of every pass
    pat = res[2 * nv + 4][0]
    canon = np.asarray(ex["canon"], np.uint32).reshape(-1, 4)
    assert canon.shape[0] == cn[0]
    vis_end = np.cumsum(np.maximum(canon[:, 3].astype(np.int32), 0))  # new items up to and with each span
    span_of = np.searchsorted(vis_end, pat[:, 0], side="right")
    assert set((np.minimum(span_of, cn[0] - 1) // DIFF_PASS).tolist()) == set(range(int(cn[0] - 1) // DIFF_PASS + 1))
    # the texts: oracle replays of the prefixes
    text = {}
    for v, k in cut.items():
        o = OracleDoc()
        w = o.agent("w")
        for op in ops[:k]:
            assert o.apply_local(w, op) == 0
        assert o.sizes()["next_order"] == v
        text[v] = o.text(c)[0]
    for d in range(nv * nv):
        p, io, it = res[d]
        assert it is not None and it.shape == io.shape
        assert np.array_equal(apply_patches(text[a[d]], p, it), text[b[d]]), (a[d], b[d])


def test_bitmaps_past_the_lds_threshold():
    # k_diff_mark builds bitmaps of up to 16,384 words (524,256 orders) in LDS and larger ones with
    # atomics in HBM: here both bitmaps of three 600,000-char documents, with a small document in
    # between, in one call.  The delete after the cut joins the 50,000 items deleted before it
    # into one deleted span of 50,200 items whose middle is deleted at v and whose ends are not;
    # the 600,000-item span and its parts go to the whole wave (kernels.h DIFF2_LONG)
    first = [[(0, 0, 600_000)], [(1000, 50_000, 0)]]
    second = [[(5, 0, 10)], [(910, 200, 0)], [(200_000, 3, 0)], [(100, 300, 0)]]
    small = [[(0, 0, 40)], [(3, 5, 0)]]
    big = [0, 2, 3]
    e = crdt_amd.Engine(4, 32)
    ag = e.agent_intern([0, 1, 2, 3], ["big"] * 4)
    assert (e.apply_local([(d, [(int(ag[d]), op) for op in first]) for d in big] +
                          [(1, [(int(ag[1]), op) for op in small])]) == 0).all()
    v = e.versions()
    assert v[0] == 650_000 and v[0] // 32 + 1 > 16384 > v[1] // 32 + 1
    assert (e.apply_local([(d, [(int(ag[d]), op) for op in second]) for d in big] +
                          [(1, [(int(ag[1]), [(10, 2, 1)])])]) == 0).all()
    end = e.versions()
    a = [int(v[0]), int(end[1]), int(end[2]), 0]
    b = [int(end[0]), int(v[1]), int(v[2]), int(v[3])]
    res = e.diff_between([0, 1, 2, 3], a, b)
    assert same_as_ref(e, 0, a[0], b[0], res[0], ref_diff_between_arrays) == 4
    assert same_as_ref(e, 1, a[1], b[1], res[1]) == 1
    assert same_as_ref(e, 2, a[2], b[2], res[2], ref_diff_between_arrays) == 4
    assert same_as_ref(e, 3, a[3], b[3], res[3], ref_diff_between_arrays) == 1
    assert res[0][0][2].tolist() == [610, 200, 0, 10]  # 100 D items on either side of the 50,000 deleted before
    assert res[2][0][2].tolist() == [900, 0, 200, 300]  # ... and back: they return around the 50,000 that stay deleted
    assert res[3][0].tolist() == [[0, 0, 550_000, 0]]


def test_rebase_on_it():
    wire, _ = concurrent_wire(2)
    o = OracleDoc()
    assert o.apply_remote_wire(wire) == 0
    n = o.sizes()["next_order"]
    pairs = [(n // 3, 2 * n // 3 + 1), (2 * n // 3 + 1, n // 3), (n // 2, n), (n, 7), (5, 5)]
    e = crdt_amd.Engine(len(pairs), 32)
    e.stage_remote_replicated(wire, 0xFFFFFFFF, [""] * len(pairs))
    assert (e.run() == 0).all()
    ex = e.export(0)
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    res = e.diff_between(list(range(len(pairs))), a, b)
    e.rebase_async("diff")
    counts = e.rebase_counts()
    kept_seen = 0
    for i, (x, y) in enumerate(pairs):
        want = ref_diff_between(ex, x, y)
        same(res[i], want, (x, y))
        table = ref_rebase_table(want[0])
        assert int(counts[i]) == table.shape[0]
        assert np.array_equal(e.rebase_read(i, "chars", counts), table), (x, y)
        # an item visible at both versions: its index at `from` maps to its index at `to`
        old, new = ref_checkout(ex, x), ref_checkout(ex, y)
        kept, at_old, at_new = np.intersect1d(old, new, return_indices=True)
        got, hit = e.rebase(np.full(len(kept), i, np.uint32), at_old.astype(np.uint32), "chars", "old_to_new", "right")
        assert np.array_equal(got, at_new.astype(np.uint32)) and not hit.any(), (x, y)
        back, hit = e.rebase(np.full(len(kept), i, np.uint32), got, "chars", "new_to_old", "right")
        assert np.array_equal(back, at_old.astype(np.uint32)) and not hit.any(), (x, y)
        kept_seen += len(kept)
    assert kept_seen > 20 and int(counts[0]) > 0 and int(counts[1]) == int(counts[0]) and int(counts[4]) == 0


def test_errors_and_purity():
    wire, _ = concurrent_wire(1)
    e = crdt_amd.Engine(5, 32)
    assert (e.apply_remote_wire([0, 2, 3, 4], [wire] * 4) == 0).all()
    ag = int(e.agent_intern([1], ["p"])[0])
    bad = [[(0, 0, 5)], [(2, 1, 0)], [(3, 5, 0)], [(0, 0, 1)]]      # the third txn deletes past the end
    assert e.apply_local([(1, [(ag, o) for o in bad])])[0] == -1
    ver = e.versions()
    dg = e.digests()
    qd = np.array([0, 0, 2, 3, 3], np.uint32)
    qp = np.array([0, 5, 1, 2, int(e.lens()[3]) - 1], np.uint32)
    loc = e.pos_to_loc(qd, qp)
    co = e.checkout([0, 3], [9, 4])
    before = e.diff([0, 3], [5, 0])
    n = int(ver[0])
    docs = [0, 1, 2, 3, 4]
    a = [5, 0, n + 1, n, 3]          # a poisoned document; from above the version
    b = [n - 2, 0, 0, 2, n + 1]      # to above the version
    res = e.diff_between(docs, a, b, strict=False)
    npat, nins = e.diff_counts()
    assert [int(x) == NO_RESULT for x in npat] == [False, True, True, False, True]
    assert [int(x) == NO_RESULT for x in nins] == [False, True, True, False, True]
    assert res[1] is None and res[2] is None and res[4] is None
    for i in (1, 2, 4):
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.diff_read(i)
    # the neighbours' results are intact (and without content there is no ins_text)
    same_as_ref(e, 0, 5, n - 2, res[0])
    same_as_ref(e, 0, 5, n - 2, e.diff_read(0))
    same_as_ref(e, 3, n, 2, e.diff_read(3))
    assert res[0][2] is None and res[3][2] is None
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.diff_between(docs, a, b)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.diff_between([0, 0], [0, 0], [1, 2])  # a document named twice
    # the call changes no document, and not the checkout made before it
    assert np.array_equal(e.digests(), dg)
    loc2 = e.pos_to_loc(qd, qp)
    assert np.array_equal(loc[0], loc2[0]) and np.array_equal(loc[1], loc2[1])
    assert np.array_equal(e.versions(), ver)
    lens = e.checkout_lens()
    for i in range(2):
        assert np.array_equal(e.checkout_read(i, lens)[0], co[i][0])
    # a second call replaces the first one's result
    res = e.diff_between([3], [7], [n - 1])
    npat, _ = e.diff_counts()
    assert npat.shape[0] == 1
    same_as_ref(e, 3, 7, n - 1, res[0])
    same_as_ref(e, 3, 7, n - 1, e.diff_read(0))
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.diff_read(1)
    # and a diff after it gives what it gave before
    after = e.diff([0, 3], [5, 0])
    for x, y in zip(before, after):
        same(x, y, "diff after diff_between")


def test_allocation_failure_leaves_the_engine_usable():
    wire, _ = concurrent_wire(2)
    L = crdt_amd.lib()
    o = OracleDoc()
    assert o.apply_remote_wire(wire) == 0
    n = o.sizes()["next_order"]
    a, b = [9, n], [n - 3, 4]
    failed = 0
    for k in range(20):  # the first call of an engine allocates every buffer it needs: fail each in turn
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        dg = e.digests()
        L.crdt_test_fail_alloc_after(k)
        try:
            e.diff_between([0, 1], a, b)
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
        # no relayout was involved: the engine is not poisoned and the same call then succeeds
        assert np.array_equal(e.digests(), dg)
        res = e.diff_between([0, 1], a, b)
        same_as_ref(e, 0, a[0], b[0], res[0])
        same_as_ref(e, 1, a[1], b[1], res[1])
        e.close()
    assert 3 <= failed < 20, failed
