"""GPU checks of the text edits in units (crdt_edits_async: k_diff_mark, k_ed_prefix, k_edits,
k_result_scan<EdRes>) through the C ABI.  Every result must equal tests/edits_ref.py's ref_edits of
the engine's own export exactly, in both encodings.

k_edits walks 256 canonical spans of a document per loop pass (kernels.h DIFF_T); k_ed_prefix
writes one record of the width index per 32 orders, 256 records (8,192 orders) per pass.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from crdt_amd.traces import load_trace  # noqa: E402
from edits_ref import apply_edits, mixed_content, ref_edits  # noqa: E402
from encode_ref import UTF8, UTF16, ref_encode  # noqa: E402
from fuzz_gen import concurrent_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402

ENCS = {"utf8": UTF8, "utf16": UTF16}
DIFF_PASS = 256  # canonical spans per pass of k_edits' per-workgroup loop
NO_RESULT = 0xFFFFFFFF


def same_as_ref(e, d, since, got, content, enc):
    want_e, want_u = ref_edits(e.export(d), since, content, enc)
    ed, ins = got
    assert ed.shape == want_e.shape and np.array_equal(ed, want_e), (d, since, ed[:8], want_e[:8])
    assert ins.dtype == want_u.dtype and np.array_equal(ins, want_u), (d, since)
    return want_e.shape[0]


def caps(leaf):
    return (leaf, 16 if leaf == 32 else 8)


def check_text(e, d, got, old_text, enc):
    """the edits turn the encoded old text into the encoding of the engine's current text"""
    ed, ins = got
    assert np.array_equal(apply_edits(ref_encode(old_text, enc)[0], ed, ins), ref_encode(e.text(d), enc)[0]), d


@pytest.mark.parametrize("encname", list(ENCS))
@pytest.mark.parametrize("leaf", [32, 4])
def test_every_version_of_a_tiny_history(leaf, encname):
    # document d of next_order + 1 copies of one concurrent history from version d: since = 0,
    # = version, inside txns, on and off the 32-order sample grid, delete runs that straddle since
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
    c = mixed_content(n, 3)
    e.set_content(docs, [0] * (n + 1), [c])
    res = e.edits(docs, docs, encname)
    total = sum(same_as_ref(e, d, d, res[d], c, ENCS[encname]) for d in range(n + 1))
    assert total > n  # (many versions need several edits)
    assert res[n][0].shape[0] == 0 and res[n][1].shape[0] == 0    # since = version: nothing changed
    whole = ref_encode(e.text(0), ENCS[encname])[0]
    assert res[0][0].tolist() == [[0, 0, len(o), 0, 0, len(whole), 0, 0]]  # since = 0: the whole text
    assert np.array_equal(res[0][1], whole)
    assert e.edits_ms() > 0


@pytest.mark.parametrize("encname", list(ENCS))
def test_wide_document_with_an_empty_and_a_one_item_document(encname):
    # the shape of test_gpu_diff.py's wide test: 700 single-char inserts at position 0 are 700
    # canonical spans, deletes and inserts in the middle split them further: at least two full
    # passes of k_edits' loop and a remainder, with edits in every pass
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
    c = mixed_content(n, 11)
    e.set_content(wide + [1, 2], [0] * 5, [c])
    docs = [0, 1, 2, 3, 4]
    since = [v, 0, 0, 0, 333]
    enc = ENCS[encname]
    res = e.edits(docs, since, encname)
    for d, s in zip(docs, since):
        same_as_ref(e, d, s, res[d], c, enc)
    assert res[1][0].shape[0] == 0 and res[1][1].shape[0] == 0          # the empty document
    w0 = len(ref_encode(c[:1], enc)[0])
    assert res[2][0].tolist() == [[0, 0, 1, 0, 0, w0, 0, 0]]            # the one-item document
    assert res[0][0].shape[0] > DIFF_PASS // 2                           # edits spread over every pass
    for d, s in ((0, v), (4, 333)):
        o = OracleDoc()
        a = o.agent("w")
        for op in first[:s]:
            assert o.apply_local(a, op) == 0
        check_text(e, d, res[d], o.text(c)[0], enc)


@pytest.mark.parametrize("leaf", [32, 4])
def test_trace_applied_in_two_halves(leaf):
    t = load_trace("sveltecomponent")
    k = t.n_txns // 2
    h = int(t.counts[:k].sum())
    e = crdt_amd.Engine(2, leaf)
    ag = int(e.agent_intern([0, 1], ["jeremy"] * 2)[0])
    assert (e.apply_trace([0, 1], ag, t.counts[:k], t.patches[:h]) == 0).all()
    v = e.versions()
    assert v[0] == v[1] and 0 < v[0]
    assert (e.apply_trace([0, 1], ag, t.counts[k:], t.patches[h:]) == 0).all()
    n = int(e.versions()[0])
    assert v[0] < n and e.canon_counts()[0] > DIFF_PASS and n > 8192  # (many spans, more than one prefix pass)
    c = mixed_content(n, 13)
    e.set_content([0, 1], [0, 0], [c])
    o = OracleDoc(*caps(leaf))
    assert o.apply_trace(o.agent("jeremy"), t.counts[:k], t.patches[:h]) == 0
    old = o.text(c)[0]
    # (one encoding per document keeps the reference walks short; both see both halves' spans)
    for encname, since in (("utf8", [int(v[0]), 0]), ("utf16", [0, int(v[1])])):
        res = e.edits([0, 1], since, encname)
        for d in (0, 1):
            if since[d] == 0:
                assert res[d][0].shape[0] == 1
                check_text(e, d, res[d], np.zeros(0, np.uint32), ENCS[encname])
            else:
                assert same_as_ref(e, d, since[d], res[d], c, ENCS[encname]) > 1
                check_text(e, d, res[d], old, ENCS[encname])


def test_long_deleted_span_and_the_bitmap_past_the_lds_threshold():
    # the 650,000-order document of test_gpu_diff.py's test_bitmap_past_the_lds_threshold (bitmap
    # built with atomics in HBM, 80 prefix passes) next to a 40-char one, in one call.  The delete
    # after the cut joins the 50,000 items deleted before it into one deleted span of 50,200 items
    # whose middle is marked: its del_units come from the two samples' differences
    first = [[(0, 0, 600_000)], [(1000, 50_000, 0)]]
    second = [[(5, 0, 10)], [(910, 200, 0)], [(200_000, 3, 0)], [(100, 300, 0)]]
    e = crdt_amd.Engine(2, 32)
    ag = e.agent_intern([0, 1], ["big"] * 2)
    small = [[(0, 0, 40)], [(3, 5, 0)]]
    assert (e.apply_local([(0, [(int(ag[0]), op) for op in first]), (1, [(int(ag[1]), op) for op in small])]) == 0).all()
    v = e.versions()
    assert v[0] == 650_000 and v[0] // 32 + 1 > 16384 > v[1] // 32 + 1
    assert (e.apply_local([(0, [(int(ag[0]), op) for op in second]), (1, [(int(ag[1]), [(10, 2, 1)])])]) == 0).all()
    c = mixed_content(int(e.versions()[0]), 17)
    e.set_content([0, 1], [0, 0], [c])
    since = [int(v[0]), int(v[1])]
    res = e.edits([0, 1], since, "utf8")
    assert same_as_ref(e, 0, since[0], res[0], c, UTF8) == 4
    assert same_as_ref(e, 1, since[1], res[1], c, UTF8) == 1
    third = res[0][0][2].tolist()
    assert third[:3] == [610, 200, 0]  # 100 D items on either side of the 50,000 deleted before
    # (10 chars went in at position 5 first: positions 910..1,109 are the items 900..999 and 51,000..51,099)
    w = [len(ref_encode(c[x:x + 1], UTF8)[0]) for x in list(range(900, 1000)) + list(range(51_000, 51_100))]
    assert third[4] == sum(w) and third[4] > 200
    res16 = e.edits([1, 0], since[::-1], "utf16")
    assert same_as_ref(e, 1, since[1], res16[0], c, UTF16) == 1
    assert np.array_equal(res16[1][0][:, :3], res[0][0][:, :3]) and res16[1][0][2][4] < third[4]


@pytest.mark.parametrize("encname", list(ENCS))
def test_against_the_engines_other_answers(encname):
    e = crdt_amd.Engine(4, 32)
    wires = [concurrent_wire(s)[0] for s in range(4)]
    assert (e.apply_remote_wire(list(range(4)), wires) == 0).all()
    ver = e.versions()
    streams = [mixed_content(int(v), 20 + i) for i, v in enumerate(ver)]
    e.set_content(list(range(4)), list(range(4)), streams)
    docs = [2, 0, 3, 1]
    since = [int(ver[d]) // (i + 2) for i, d in enumerate(docs)]
    res = e.edits(docs, since, encname)
    diff = e.diff(docs, since)
    enc = e.encode(docs, encname)
    n_edits = 0
    for i in range(4):
        ed, ins = res[i]
        assert np.array_equal(ed[:, :3], diff[i][0][:, :3])
        assert np.array_equal(ed[:, 3], e.pos_to_units(np.full(len(ed), i, np.uint32), ed[:, 0]))
        text = np.frombuffer(enc[i], np.uint8) if encname == "utf8" else enc[i]
        for _pos, _dl, _il, unit, _du, iu, off, _r in ed.tolist():
            assert np.array_equal(ins[off:off + iu], text[unit:unit + iu])
        n_edits += len(ed)
    assert n_edits > 8


def test_no_result_indexes_and_purity():
    wire, _ = concurrent_wire(1)
    e = crdt_amd.Engine(6, 32)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.edits_counts()  # before any edits call
    assert (e.apply_remote_wire([0, 2, 3, 5], [wire] * 4) == 0).all()
    ag = int(e.agent_intern([1], ["p"])[0])
    bad = [[(0, 0, 5)], [(2, 1, 0)], [(3, 5, 0)], [(0, 0, 1)]]      # the third txn deletes past the end
    assert e.apply_local([(1, [(ag, o) for o in bad])])[0] == -1
    ver = e.versions()
    nv = int(ver[0])
    c = mixed_content(nv, 31)
    # 0, 5 healthy; 1 poisoned (with content); 2 asked from above its version; 3 one entry short;
    # 4 (empty) without content
    e.set_content([0, 1, 2, 3, 5], [0, 0, 0, 1, 0], [c, c[:-1]])
    dg = e.digests()
    qd = np.array([0, 0, 2, 3, 3], np.uint32)
    qp = np.array([0, 5, 1, 2, int(e.lens()[3]) - 1], np.uint32)
    loc = e.pos_to_loc(qd, qp)
    docs = list(range(6))
    since = [5, 0, nv + 1, 0, 0, 0]
    none = [False, True, True, True, True, False]
    for encname, enc in ENCS.items():
        res = e.edits(docs, since, encname, strict=False)
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
        same_as_ref(e, 0, 5, res[0], c, enc)
        same_as_ref(e, 0, 5, e.edits_read(0), c, enc)
        same_as_ref(e, 5, 0, e.edits_read(5), c, enc)
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.edits(docs, since, encname)  # strict
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.edits([0, 0], [0, 0])  # a document named twice
    for enc in (2, -1):
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.edits_async([0], [0], enc)  # an unknown enc
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.edits_read(6)  # out of range
    # (calls rejected for their arguments leave the last result)
    same_as_ref(e, 5, 0, e.edits_read(5), c, UTF16)
    # an edits call changes no document
    assert np.array_equal(e.digests(), dg)
    loc2 = e.pos_to_loc(qd, qp)
    assert np.array_equal(loc[0], loc2[0]) and np.array_equal(loc[1], loc2[1])
    assert np.array_equal(e.versions(), ver)
    # a second call replaces the first one's result
    res = e.edits([5], [7], "utf8")
    assert e.edits_counts()[0].shape[0] == 1
    same_as_ref(e, 5, 7, res[0], c, UTF8)
    same_as_ref(e, 5, 7, e.edits_read(0), c, UTF8)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.edits_read(1)
    assert e.edits([], []) == [] and len(e.edits_counts()[0]) == 0
    # crdt_docs_alloc frees the result
    e.edits([5], [7], "utf8")
    assert e.L.crdt_docs_alloc(e.h, 2) == 0
    e.n_docs = 2
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.edits_counts()
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.edits_read(0)


def test_independent_of_the_six_other_results():
    rng = np.random.default_rng(71)
    e = crdt_amd.Engine(6, 32)
    docs6 = list(range(6))
    assert (e.apply_remote_wire(docs6, [concurrent_wire(s)[0] for s in range(6)]) == 0).all()
    streams = [rng.choice(np.array([0x61, 0x62, 0x41, 0x0A, 0xE9, 0x1F600, 0xD800], np.uint32), int(v)) for v in e.versions()]
    e.set_content(docs6, docs6, streams)
    v = e.versions([2, 4])
    docs = [5, 0, 3]  # a listed subset, not ascending

    def six():
        diff = e.diff([2, 4], v // 2)
        co = e.checkout([4, 2], v[::-1] // 3)
        bl = e.blame([2, 4], "id")
        enc = e.encode(docs, "utf8")
        lines = e.lines("lf")
        found = e.find("a")
        return diff, co, bl, enc, lines, found

    def read_six():
        return ([e.diff_read(i) for i in range(2)], [e.checkout_read(i) for i in range(2)],
                [e.blame_read(i) for i in range(2)], [e.encode_read(i) for i in range(3)],
                [e.lines_read(i) for i in range(3)], [e.find_read(i) for i in range(3)])

    def same(a, b):
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if a is None or isinstance(a, bytes):
            return a == b
        return np.array_equal(a, b)

    first = six()
    assert same(first, read_six())
    before = e.mem_bytes()
    since = [int(x) // 2 for x in e.versions([4, 1, 2])]
    res = e.edits([4, 1, 2], since, "utf16")
    assert e.mem_bytes() > before  # the buffers are counted
    assert sum(len(r[0]) for r in res) > 3
    # reading each of the six gives what it gave before
    assert same(first, read_six())
    # ... and running the six calls again leaves the edits result readable and unchanged
    assert same(first, six())
    for i, (d, s) in enumerate(zip([4, 1, 2], since)):
        got = e.edits_read(i)
        assert same(list(res[i]), list(got))
        same_as_ref(e, d, s, got, streams[d], UTF16)


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
    since = np.array([d % (int(ver[d]) + 1) for d in docs], np.uint32)
    res = e.edits(docs, since, "utf8")
    ned, nun = e.edits_counts()
    assert int(ned.sum()) > n // 2 and int(nun.sum()) > n
    for i, d in enumerate(docs):
        same_as_ref(e, int(d), int(since[i]), res[i], c, UTF8)


def test_allocation_failure_leaves_the_engine_usable():
    wire, _ = concurrent_wire(2)
    L = crdt_amd.lib()
    failed = 0
    for k in range(24):  # the first edits call of an engine allocates every buffer it needs: fail each in turn
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        c = mixed_content(int(e.versions([0])[0]), 51)
        e.set_content([0, 1], [0, 0], [c])
        dg = e.digests()
        L.crdt_test_fail_alloc_after(k)
        try:
            e.edits([0, 1], [9, 0], "utf16")
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
        res = e.edits([0, 1], [9, 0], "utf16")
        same_as_ref(e, 0, 9, res[0], c, UTF16)
        same_as_ref(e, 1, 0, res[1], c, UTF16)
        e.close()
    assert 9 <= failed < 24, failed  # (at least the job's two and the seven buffers of its own)
