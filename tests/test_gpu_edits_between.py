"""GPU checks of the edits in units between two versions (crdt_edits_between_async: k_diff_mark
twice, k_ed_planes, k_edits2, k_result_scan<EdRes>) through the C ABI.  Every result must equal
tests/edits_between_ref.py's ref_edits_between of the engine's own export exactly, in both encodings.

docs has no duplicates, so every (from, to) pair of a call has a document of its own.  k_edits2 walks
256 canonical spans of a document per loop pass (kernels.h DIFF_T), a span of up to 256 orders in one
lane and a longer one with the whole wave (DIFF2_LONG), 32 orders (one bitmap word) at a time;
k_ed_planes writes the width planes of 256 words (8,192 orders) per pass.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from checkout_ref import ref_checkout  # noqa: E402
from edits_between_ref import ref_edits_between, ref_edits_between_arrays  # noqa: E402
from edits_ref import apply_edits, mixed_content  # noqa: E402
from encode_ref import BOUNDARY, NOT_SCALAR, UTF8, UTF16, ref_encode  # noqa: E402
from fuzz_gen import build_wire, concurrent_wire, parse_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from rebase_ref import ref_rebase_table  # noqa: E402

ENCS = {"utf8": UTF8, "utf16": UTF16}
DIFF_PASS = 256   # canonical spans per pass of k_edits2's per-workgroup loop
DIFF2_LONG = 256  # a span with more orders below max(from, to) is walked by the whole wave
NO_RESULT = 0xFFFFFFFF


def same(got, want, what):
    ed, ins = got
    assert ed.shape == want[0].shape and np.array_equal(ed, want[0]), (what, ed[:8], want[0][:8])
    assert ins.dtype == want[1].dtype and np.array_equal(ins, want[1]), what
    return ed.shape[0]


def same_as_ref(e, d, a, b, got, content, enc, ref=ref_edits_between):
    return same(got, ref(e.export(d), a, b, content, enc), (d, a, b, enc))


def caps(leaf):
    return (leaf, 16 if leaf == 32 else 8)


@pytest.mark.parametrize("encname", list(ENCS))
@pytest.mark.parametrize("leaf", [32, 4])
def test_every_ordered_pair_of_a_tiny_history(leaf, encname):
    # the first 12 txns of a concurrent history, one copy per ordered pair of its versions: from and
    # to at 0, at the version, inside txns, on either side of the 32-order word, and delete runs
    # that straddle either
    enc = ENCS[encname]
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
    c = mixed_content(n, 3)
    e.set_content(docs, [0] * (nv * nv), [c])
    a, b = docs // nv, docs % nv
    res = e.edits_between(docs, a, b, encname)
    total = 0
    for d in docs:
        total += same(res[d], ref_edits_between(ex, a[d], b[d], c, enc), (a[d], b[d]))
    assert total > nv * nv  # (many pairs need several edits)
    for v in range(nv):     # the diagonal: nothing changed
        assert res[v * nv + v][0].shape[0] == 0 and res[v * nv + v][1].shape[0] == 0
    assert e.edits_ms() > 0
    # the item columns are the two-version diff's
    diff = e.diff_between(docs, a, b)
    for d in docs:
        assert np.array_equal(res[d][0][:, :3], diff[d][0][:, :3]), (a[d], b[d])
    # the column to = version is the edits result, array for array, pool included
    col = docs[b == n]
    now = e.edits(col, a[col], encname)
    for d, r in zip(col, now):
        same(res[d], r, ("pin", a[d]))


def test_word_boundaries_inside_one_span():
    # test_gpu_diff_between.py's construction: one 200-item span; single-char deletes, a txn each, of
    # the items with orders 31, 32, 63, 64, 95 and 96 (the last and the first order of a bitmap
    # word), then of 129, 128 and 130 (one deleted span in the end, whose middle goes first), then
    # a few inserts.  from and to at every version from the first delete on, both directions; the
    # content has every width of both encodings and values that are no scalar values
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
    c = mixed_content(vs[-1], 7)
    pool = BOUNDARY + NOT_SCALAR
    for k, x in enumerate(hit + [30, 33, 62, 65, 94, 97, 127, 131]):  # every width at and next to the deleted orders
        c[x] = pool[(2 * k + 1) % len(pool)]
    assert {len(ref_encode(c[x:x + 1], UTF8)[0]) for x in hit} == {1, 2, 3, 4}
    docs = np.arange(nv * nv)
    e.set_content(docs, [0] * (nv * nv), [c])
    a, b = np.array(vs)[docs // nv], np.array(vs)[docs % nv]
    for encname, enc in ENCS.items():
        res = e.edits_between(docs, a, b, encname)
        total = 0
        for d in docs:
            total += same(res[d], ref_edits_between(ex, a[d], b[d], c, enc), (a[d], b[d], enc))
        assert total > 2 * nv * nv
        w = [len(ref_encode(c[x:x + 1], enc)[0]) for x in range(vs[-1])]
        # from before the deletes to after them: one edit per pair of neighbouring items
        assert res[6][0][:, :3].tolist() == [[31, 2, 0], [61, 2, 0], [91, 2, 0]]
        assert res[6][0][:, 4].tolist() == [w[31] + w[32], w[63] + w[64], w[95] + w[96]]
        assert res[6 * nv][0][:, 5].tolist() == res[6][0][:, 4].tolist()
        # from after the nine deletes back to after the seventh: 128 and 130 return around 129, which stays deleted
        assert res[9 * nv + 7][0].tolist() == [[122, 0, 2, sum(w[:128]) - sum(w[x] for x in six), 0, w[128] + w[130], 0, 0]]
        assert np.array_equal(res[9 * nv + 7][1], ref_encode(c[[128, 130]], enc)[0])


@pytest.mark.parametrize("encname", list(ENCS))
def test_several_passes_and_a_long_span(encname):
    # 760 single-char inserts at position 0 are 760 canonical spans (document order is the reverse
    # of the orders), then one 9,000-char insert in the middle (more than 8,192 orders: two passes of
    # k_ed_planes), then deletes over the first 1,300 chars, inserts among the last 380 and one
    # 700-char delete inside the long insert: spans past DIFF2_LONG, visible and deleted, which the
    # whole wave walks, and edits in the spans of every pass.  Next to it an empty and a one-item
    # document
    enc = ENCS[encname]
    first = [[(0, 0, 1)] for _ in range(760)]
    long_ = [[(380, 0, 9000)]]
    second = [[(13 * j, 1, 0)] for j in range(100)] + [[(9300 + 7 * j, 0, 2)] for j in range(60)] + [[(500, 700, 0)]]
    ops = first + long_ + second
    end = 760 + 9000 + 100 + 120 + 700
    cut = {0: 0, 333: 333, 760: 760, 9760: 761, 9760 + 100 + 60: 761 + 130, end: len(ops)}  # version -> txns applied
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
    ex = e.export(0)
    canon = np.asarray(ex["canon"], np.uint32).reshape(-1, 4)
    slen = canon[:, 3].astype(np.int32)
    assert slen.max() > DIFF2_LONG and -slen.min() > DIFF2_LONG and end > 8192
    c = mixed_content(end, 11)
    e.set_content(list(range(nd)), [0] * nd, [c])
    docs = np.arange(nd)
    a = np.array([vs[d // nv] for d in range(nv * nv)] + [0, 1])
    b = np.array([vs[d % nv] for d in range(nv * nv)] + [0, 0])
    res = e.edits_between(docs, a, b, encname)
    for d in range(nv * nv):
        same(res[d], ref_edits_between_arrays(ex, a[d], b[d], c, enc), (a[d], b[d]))
    for d in (2 * nv + 5, 5 * nv + 1, 4 * nv + 3):  # ... and the item walk on a few
        same(res[d], ref_edits_between(ex, a[d], b[d], c, enc), (a[d], b[d]))
    assert res[empty][0].shape[0] == 0 and res[empty][1].shape[0] == 0    # the empty document
    w0 = len(ref_encode(c[:1], enc)[0])
    assert res[one][0].tolist() == [[0, 1, 0, 0, w0, 0, 0, 0]]            # the one-item document, back to nothing
    # (9760, end): the edits' positions fall into the spans of every pass
    pos = res[3 * nv + 5][0][:, 0]
    vis_end = np.cumsum(np.maximum(slen, 0))  # new items up to and with each span
    span_of = np.minimum(np.searchsorted(vis_end, pos, side="right"), cn[0] - 1)
    assert set((span_of // DIFF_PASS).tolist()) == set(range(int(cn[0] - 1) // DIFF_PASS + 1))
    # the texts: oracle replays of the prefixes
    text = {}
    for v, k in cut.items():
        o = OracleDoc()
        w = o.agent("w")
        for op in ops[:k]:
            assert o.apply_local(w, op) == 0
        assert o.sizes()["next_order"] == v
        text[v] = ref_encode(o.text(c)[0], enc)[0]
    for d in range(nv * nv):
        assert np.array_equal(apply_edits(text[a[d]], res[d][0], res[d][1]), text[b[d]]), (a[d], b[d])


def test_both_bitmaps_past_the_lds_threshold():
    # the 650,000-order document of test_gpu_edits.py (both bitmaps built with atomics in HBM, 80
    # passes of k_ed_planes) next to a 40-char one, in one call; to below the version, so the
    # second bitmap matters: the delete after the cut joins the 50,000 items deleted before it into
    # one deleted span of 50,200 items whose middle is deleted at v and whose ends are not
    first = [[(0, 0, 600_000)], [(1000, 50_000, 0)]]
    second = [[(5, 0, 10)], [(910, 200, 0)], [(200_000, 3, 0)], [(100, 300, 0)]]
    small = [[(0, 0, 40)], [(3, 5, 0)]]
    big = [0, 2]
    e = crdt_amd.Engine(3, 32)
    ag = e.agent_intern([0, 1, 2], ["big"] * 3)
    assert (e.apply_local([(d, [(int(ag[d]), op) for op in first]) for d in big] +
                          [(1, [(int(ag[1]), op) for op in small])]) == 0).all()
    v = e.versions()
    assert v[0] == 650_000 and v[0] // 32 + 1 > 16384 > v[1] // 32 + 1
    assert (e.apply_local([(d, [(int(ag[d]), op) for op in second]) for d in big] +
                          [(1, [(int(ag[1]), [(10, 2, 1)])])]) == 0).all()
    end = e.versions()
    c = mixed_content(int(end[0]), 17)
    e.set_content([0, 1, 2], [0, 0, 0], [c])
    a = [int(end[0]), int(end[1]), 600_000]
    b = [int(v[0]), int(v[1]), int(end[2]) - 300]
    res = e.edits_between([0, 1, 2], a, b, "utf8")
    assert same_as_ref(e, 0, a[0], b[0], res[0], c, UTF8, ref_edits_between_arrays) == 4
    assert same_as_ref(e, 1, a[1], b[1], res[1], c, UTF8) == 1
    assert same_as_ref(e, 2, a[2], b[2], res[2], c, UTF8, ref_edits_between_arrays) >= 3
    third = res[0][0][2].tolist()
    assert third[:3] == [900, 0, 200]  # they return around the 50,000 that stay deleted
    w = [len(ref_encode(c[x:x + 1], UTF8)[0]) for x in list(range(900, 1000)) + list(range(51_000, 51_100))]
    assert third[5] == sum(w) and third[5] > 200
    res16 = e.edits_between([2, 1, 0], a[::-1], b[::-1], "utf16")
    assert same_as_ref(e, 1, a[1], b[1], res16[1], c, UTF16) == 1
    assert same_as_ref(e, 0, a[0], b[0], res16[2], c, UTF16, ref_edits_between_arrays) == 4
    assert res16[2][0][2][5] < third[5]


@pytest.mark.parametrize("encname", list(ENCS))
def test_against_the_engines_other_answers(encname):
    enc = ENCS[encname]
    wire, _ = concurrent_wire(2)
    o = OracleDoc()
    assert o.apply_remote_wire(wire) == 0
    n = o.sizes()["next_order"]
    pairs = [(n // 3, 2 * n // 3 + 1), (2 * n // 3 + 1, n // 3), (n // 2, n), (n, 7), (5, 5), (0, n)]
    e = crdt_amd.Engine(len(pairs), 32)
    e.stage_remote_replicated(wire, 0xFFFFFFFF, [""] * len(pairs))
    assert (e.run() == 0).all()
    ex = e.export(0)
    c = mixed_content(n, 21)
    idx = list(range(len(pairs)))
    e.set_content(idx, [0] * len(pairs), [c])
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    res = e.edits_between(idx, a, b, encname)
    # unit is pos_to_units on an encode of a checkout at `to`, where to is the version
    e.encode(idx, encname)
    for i in (2, 5):
        ed = res[i][0]
        assert len(ed) > 0 and np.array_equal(ed[:, 3], e.pos_to_units(np.full(len(ed), i, np.uint32), ed[:, 0]))
        assert np.array_equal(e.checkout([i], [n])[0][1], e.text(i))
    # the rebase from the result maps kept items in both directions, in chars and in units
    e.rebase_async("edits")
    counts = e.rebase_counts()
    kept_seen = 0
    for i, (x, y) in enumerate(pairs):
        want = ref_edits_between(ex, x, y, c, enc)
        same(res[i], want, (x, y))
        assert int(counts[i]) == want[0].shape[0]
        assert np.array_equal(e.rebase_read(i, "chars", counts), ref_rebase_table(want[0]))
        assert np.array_equal(e.rebase_read(i, "units", counts), ref_rebase_table(want[0], units=True))
        old, new = ref_checkout(ex, x), ref_checkout(ex, y)
        kept, at_old, at_new = np.intersect1d(old, new, return_indices=True)
        q = np.full(len(kept), i, np.uint32)
        got, hit = e.rebase(q, at_old.astype(np.uint32), "chars", "old_to_new", "right")
        assert np.array_equal(got, at_new.astype(np.uint32)) and not hit.any(), (x, y)
        back, hit = e.rebase(q, got, "chars", "new_to_old", "right")
        assert np.array_equal(back, at_old.astype(np.uint32)) and not hit.any(), (x, y)
        u_old, u_new = ref_encode(c[old], enc)[1][at_old], ref_encode(c[new], enc)[1][at_new]
        got, hit = e.rebase(q, u_old, "units", "old_to_new", "right")
        assert np.array_equal(got, u_new) and not hit.any(), (x, y)
        back, hit = e.rebase(q, got, "units", "new_to_old", "right")
        assert np.array_equal(back, u_old) and not hit.any(), (x, y)
        kept_seen += len(kept)
    assert kept_seen > 20 and int(counts[0]) > 0 and int(counts[1]) == int(counts[0]) and int(counts[4]) == 0


def test_no_result_indexes_and_purity():
    wire, _ = concurrent_wire(1)
    e = crdt_amd.Engine(8, 32)
    assert (e.apply_remote_wire([0, 2, 3, 5, 6, 7], [wire] * 6) == 0).all()
    ag = int(e.agent_intern([1], ["p"])[0])
    bad = [[(0, 0, 5)], [(2, 1, 0)], [(3, 5, 0)], [(0, 0, 1)]]      # the third txn deletes past the end
    assert e.apply_local([(1, [(ag, o) for o in bad])])[0] == -1
    ver = e.versions()
    nv = int(ver[0])
    c = mixed_content(nv, 31)
    # 0, 5 healthy; 1 poisoned (with content); 2 asked from above its version; 6 asked to above its
    # version; 3 one entry short; 4 (empty) without content; 7 healthy, for the other results
    e.set_content([0, 1, 2, 3, 5, 6, 7], [0, 0, 0, 1, 0, 0, 0], [c, c[:-1]])
    dg = e.digests()

    def others():
        diff = e.diff([7, 0], [nv // 2, 3])
        co = e.checkout([0, 7], [9, nv // 3])
        bl = e.blame([7, 0], "id")
        enc = e.encode([5, 0, 7], "utf8")
        lines = e.lines("lf")
        found = e.find("A")
        e.rebase_async("diff")
        return diff, co, bl, enc, lines, found

    def read_others():
        return ([e.diff_read(i) for i in range(2)], [e.checkout_read(i) for i in range(2)],
                [e.blame_read(i) for i in range(2)], [e.encode_read(i) for i in range(3)],
                [e.lines_read(i) for i in range(3)], [e.find_read(i) for i in range(3)],
                [e.rebase_read(i, "chars") for i in range(2)])

    def eq(x, y):
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(eq(p, q) for p, q in zip(x, y))
        if x is None or isinstance(x, bytes):
            return x == y
        return np.array_equal(x, y)

    first = others()
    snap = read_others()
    before_now = e.edits([0, 5], [5, 0], "utf16")
    mem = e.mem_bytes()
    docs = list(range(7))
    a = [5, 0, nv + 1, 0, 0, 0, 3]
    b = [nv - 2, 0, 0, 2, 0, nv, nv + 1]
    none = [False, True, True, True, True, False, True]
    for encname, enc in ENCS.items():
        res = e.edits_between(docs, a, b, encname, strict=False)
        ned, nun = e.edits_counts()
        assert [int(x) == NO_RESULT for x in ned] == none
        assert [int(x) == NO_RESULT for x in nun] == none
        for i in docs:
            if none[i]:
                assert res[i] is None
                with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                    e.edits_read(i)
                assert e.L.crdt_edits_read(e.h, i, None, None) == -100
        # the neighbours' results are intact
        same_as_ref(e, 0, 5, nv - 2, res[0], c, enc)
        same_as_ref(e, 0, 5, nv - 2, e.edits_read(0), c, enc)
        same_as_ref(e, 5, 0, nv, e.edits_read(5), c, enc)
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.edits_between(docs, a, b, encname)  # strict
    assert e.mem_bytes() > mem  # the new buffers are counted
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.edits_between([0, 0], [0, 0], [1, 2])  # a document named twice
    for enc in (2, -1):
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.edits_between_async([0], [0], [1], enc)  # an unknown enc
    # (calls rejected for their arguments leave the last result)
    same_as_ref(e, 5, 0, nv, e.edits_read(5), c, UTF16)
    # the call changes no document and none of the other results
    assert np.array_equal(e.digests(), dg) and np.array_equal(e.versions(), ver)
    assert eq(snap, read_others())
    # ... and their calls leave the edits result readable and unchanged
    keep = [e.edits_read(i) for i in (0, 5)]
    assert eq(first, others())
    for i, k in zip((0, 5), keep):
        assert eq(list(k), list(e.edits_read(i)))
    # a second call replaces the first one's result
    res = e.edits_between([5], [7], [nv - 1], "utf8")
    assert e.edits_counts()[0].shape[0] == 1
    same_as_ref(e, 5, 7, nv - 1, res[0], c, UTF8)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.edits_read(1)
    assert e.edits_between([], [], []) == [] and len(e.edits_counts()[0]) == 0
    # a following edits call gives what it gave before
    after = e.edits([0, 5], [5, 0], "utf16")
    assert eq([list(x) for x in before_now], [list(x) for x in after])
    # a document whose widths sum to 0xFFFFFFFF or more is out of reach of a test (2^30 orders); the
    # flag is k_ed_planes' sum over all orders, checked by the counts of every other test here
    # crdt_docs_alloc frees the result
    e.edits_between([5], [7], [nv - 1], "utf8")
    assert e.L.crdt_docs_alloc(e.h, 2) == 0
    e.n_docs = 2
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.edits_counts()


def test_scan_slices_with_more_than_one_index_per_thread():
    # 1,100 tiny documents in one call: k_result_scan's 1,024 threads take two indexes each (the
    # last ones none), and both of its offsets (edits, inserted units) cross the slices
    n = 1100
    e = crdt_amd.Engine(n, 32)
    ag = e.agent_intern(list(range(n)), ["t"] * n)
    ops = []
    for d in range(n):
        tx = [[(0, 0, 2 + d % 5)], [(1, 1, 0)], [(d % 2, 0, 1 + d % 3)]]
        ops.append((d, [(int(ag[d]), op) for op in tx[:1 + d % 3]]))
    assert (e.apply_local(ops) == 0).all()
    ver = e.versions()
    c = mixed_content(16, 41)
    e.set_content(list(range(n)), [0] * n, [c])
    docs = np.arange(n)[::-1].copy()
    a = np.array([d % (int(ver[d]) + 1) for d in docs], np.uint32)
    b = np.array([(d // 3) % (int(ver[d]) + 1) for d in docs], np.uint32)
    res = e.edits_between(docs, a, b, "utf8")
    ned, nun = e.edits_counts()
    assert int(ned.sum()) > n // 2 and int(nun.sum()) > n // 2
    for i, d in enumerate(docs):
        same_as_ref(e, int(d), int(a[i]), int(b[i]), res[i], c, UTF8)


def test_allocation_failure_leaves_the_engine_usable():
    wire, _ = concurrent_wire(2)
    L = crdt_amd.lib()
    failed = 0
    for k in range(28):  # the first call of an engine allocates every buffer it needs: fail each in turn
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        n = int(e.versions([0])[0])
        c = mixed_content(n, 51)
        e.set_content([0, 1], [0, 0], [c])
        dg = e.digests()
        a, b = [9, n], [n - 3, 4]
        L.crdt_test_fail_alloc_after(k)
        try:
            e.edits_between([0, 1], a, b, "utf16")
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
        # no relayout was involved: the engine is not poisoned, has no edits result, and the same call then succeeds
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.edits_counts()
        assert np.array_equal(e.digests(), dg)
        res = e.edits_between([0, 1], a, b, "utf16")
        same_as_ref(e, 0, a[0], b[0], res[0], c, UTF16)
        same_as_ref(e, 1, a[1], b[1], res[1], c, UTF16)
        e.close()
    assert 11 <= failed < 28, failed  # (at least the job's two and the nine buffers of its own)
