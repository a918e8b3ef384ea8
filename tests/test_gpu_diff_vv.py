"""GPU checks of the patches between two causal versions given as version vectors
(crdt_version_vector: k_vv_of; crdt_diff_vv_async: k_vv_mark twice, k_diff2_sets,
k_result_scan<DiffRes>; crdt_diff_vv_closed) through the C ABI.  Every result must equal
tests/diff_vv_ref.py's ref_diff_vv of the engine's own export exactly, and every closed flag its
ref_vv_closed.

k_vv_mark builds an index's two bitmaps in LDS when they fit the launch's budget and with atomics in
device memory otherwise; crdt_test_set_vv_lds_words(0) sends every document the second way.  Every
call here runs both ways (diff_both) and the two results must be identical.

docs has no duplicates, so a call has one pair of vectors per document; the documents of `small`
are replayed once and every test's calls go over them again with other vectors.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from diff_ref import apply_patches  # noqa: E402
from diff_vv_cases import (DIFF2_LONG, DIFF_T, LONG_VECTORS, MANY_VECTORS, NEIGHBOUR_VECTORS, cut_vectors, long_span,  # noqa: E402
                           many_spans, neighbour_deletes, random_vectors, vector)
from diff_vv_ref import next_seqs, ref_diff_vv, ref_version_vector, ref_vv_closed  # noqa: E402
from fuzz_gen import build_wire, concurrent_wire, gossip_family  # noqa: E402
from general_streams import run_stream  # noqa: E402
from rebase_ref import ref_rebase_table  # noqa: E402
from test_diff_ref import double_delete_txns  # noqa: E402

NO_RESULT = 0xFFFFFFFF
DEFAULT_LDS_WORDS = 16384  # kernels.h DIFF_MARK_WORDS
VV_SYMBOLS = ["crdt_version_vector", "crdt_version_vector_dev_async", "crdt_diff_vv_async", "crdt_diff_vv_closed",
              "crdt_test_set_vv_lds_words"]


def same(got, want, what):
    pat, io = got[0], got[1]
    assert pat.shape == want[0].shape and np.array_equal(pat, want[0]), (what, pat[:8], want[0][:8])
    assert np.array_equal(io, want[1]), what
    return pat.shape[0]


def same_arrays(x, y, what):
    """two results of the engine, array for array, ins_text included"""
    same(x, y, what)
    assert (x[2] is None) == (y[2] is None), what
    if x[2] is not None:
        assert np.array_equal(x[2], y[2]), what


def diff_both(e, docs, fv, tv, strict=True):
    """diff_vv with the bitmaps in LDS and with them in device memory: (the result, both sides'
    closed flags), identical both ways"""
    L = crdt_amd.lib()
    out = []
    try:
        for words in (DEFAULT_LDS_WORDS, 0):
            L.crdt_test_set_vv_lds_words(words)
            res = e.diff_vv(docs, fv, tv, strict=strict)
            out.append((res, e.diff_vv_closed(), e.diff_counts()))
    finally:
        L.crdt_test_set_vv_lds_words(DEFAULT_LDS_WORDS)
    (r0, c0, n0), (r1, c1, n1) = out
    assert np.array_equal(n0[0], n1[0]) and np.array_equal(n0[1], n1[1])
    assert np.array_equal(c0[0], c1[0]) and np.array_equal(c0[1], c1[1])
    for i, (x, y) in enumerate(zip(r0, r1)):
        assert (x is None) == (y is None), i
        if x is not None:
            same_arrays(x, y, ("lds / hbm", i))
    return r0, c0


class Small:
    """the small concurrent documents, replayed once: fuzz histories (3 agents), gossip histories
    (4 agents, partial delivery), the double deletes, a general-form stream on its prep (a 256-op
    txn), and the three hand-built shapes of tests/diff_vv_cases.py"""

    def __init__(self):
        self.wires = [concurrent_wire(s)[0] for s in range(3)]
        self.wires += [w for _s, _k, w in gossip_family("A")[1:6:2]]
        self.wires.append(build_wire(double_delete_txns()))
        p, s = run_stream(5, 20, "back")
        self.wires.append(build_wire(p + s))
        self.neighbour, self.long, self.many = len(self.wires), len(self.wires) + 1, len(self.wires) + 2
        self.wires += [build_wire(neighbour_deletes()), build_wire(long_span()), build_wire(many_spans())]
        self.n = len(self.wires)
        self.docs = list(range(self.n))
        self.e = crdt_amd.Engine(self.n, 32)
        assert (self.e.apply_remote_wire(self.docs, self.wires) == 0).all()
        self.ex = [self.e.export(d) for d in self.docs]
        self.ver = [int(x["next_order"]) for x in self.ex]
        self.full = [next_seqs(x).astype(np.uint32) for x in self.ex]
        # content: every document reads one stream, long enough for the largest
        self.content = np.random.default_rng(5).integers(0x20, 0xD7FF, max(self.ver), dtype=np.uint32)
        self.e.set_content(self.docs, [0] * self.n, [self.content])

    def ids(self, d, names):
        return {n: int(self.e.agent_intern([d], [n])[0]) for n in names}

    def check(self, fv, tv, what):
        """one call over every document, both ways, against the reference: patches, inserted
        orders, inserted text and both closed flags; returns the patches seen"""
        res, (cf, ct) = diff_both(self.e, self.docs, fv, tv)
        total = 0
        for d in self.docs:
            total += same(res[d], ref_diff_vv(self.ex[d], fv[d], tv[d]), (what, d, fv[d], tv[d]))
            assert np.array_equal(res[d][2], self.content[res[d][1]]), (what, d)
            assert bool(cf[d]) == ref_vv_closed(self.ex[d], fv[d]), (what, d, fv[d])
            assert bool(ct[d]) == ref_vv_closed(self.ex[d], tv[d]), (what, d, tv[d])
        return total


@pytest.fixture(scope="module")
def small():
    s = Small()
    yield s
    s.e.close()


def test_library_exports_the_entry_points():
    L = crdt_amd.lib()
    for s in VV_SYMBOLS:
        assert hasattr(L, s), s
        assert s in crdt_amd.EXPORTED_SYMBOLS, s


def test_documents_are_small_and_concurrent(small):
    agents = [len(v) for v in small.full]
    assert all(2 <= a <= 5 for a in agents), agents
    assert all(v <= 1400 for v in small.ver) and sum(100 <= v <= 500 for v in small.ver) >= 6, small.ver
    assert any(np.asarray(x["dd"]).size for x in small.ex)   # double deletes among them


def test_random_vectors(small):
    rng = np.random.default_rng(17)
    draws = [random_vectors(x, rng, 6) for x in small.ex]
    total = 0
    for k in range(0, 6, 2):
        total += small.check([v[k] for v in draws], [v[k + 1] for v in draws], "random")
    assert total > 300


def test_vectors_that_cut_runs_and_words(small):
    # per document: the full vector, it cut just below the orders 31, 32 and 33, and at the first,
    # second, last and next seq of its longest client_with_order runs; each against a random vector,
    # in both directions
    rng = np.random.default_rng(23)
    cuts = [cut_vectors(x) for x in small.ex]
    rounds = max(len(c) for c in cuts)
    assert rounds >= 12
    total = 0
    for k in range(rounds):
        a = [c[k % len(c)] for c in cuts]
        b = [random_vectors(x, rng, 1)[0] for x in small.ex]
        total += small.check(a, b, ("cut", k)) if k % 2 else small.check(b, a, ("cut back", k))
    assert total > 1000


def test_equal_zero_full_and_swapped(small):
    rng = np.random.default_rng(29)
    r = [random_vectors(x, rng, 1)[0] for x in small.ex]
    zero_len = [np.zeros(0, np.uint32) for _ in small.docs]      # entries beyond the length count as 0
    zeros = [np.zeros_like(v) for v in small.full]
    assert small.check(r, r, "equal") == 0                        # from == to: no patches
    assert small.check(small.full, small.full, "full, full") == 0
    assert small.check(zero_len, zeros, "zero, zero") == 0
    # nothing -> now is one patch that inserts the text; now -> nothing one that deletes it
    res, _ = diff_both(small.e, small.docs, zero_len, small.full)
    back, _ = diff_both(small.e, small.docs, small.full, zeros)
    lens = small.e.lens()
    for d in small.docs:
        n = int(lens[d])
        assert res[d][0].tolist() == ([[0, 0, n, 0]] if n else []), d
        assert back[d][0].tolist() == ([[0, n, 0, 0]] if n else []), d
        assert np.array_equal(res[d][2], small.e.text(d))
    assert small.check(zero_len, small.full, "zero, full") > 0
    # swapped: as many patches, del_len and ins_len exchanged
    fwd, _ = diff_both(small.e, small.docs, r, small.full)
    rev, _ = diff_both(small.e, small.docs, small.full, r)
    for d in small.docs:
        assert fwd[d][0].shape == rev[d][0].shape, d
        assert np.array_equal(fwd[d][0][:, 1], rev[d][0][:, 2]) and np.array_equal(fwd[d][0][:, 2], rev[d][0][:, 1]), d
    assert small.check(r, small.full, "r, full") + small.check(small.full, r, "full, r") > 0


def test_prefix_vectors_give_the_two_version_diff(small):
    # versions 0, 1, the orders around 32, inside and at the end of txns, the version: the vectors
    # of k_vv_of, and on them the call is crdt_diff_between_async array for array (ins_off and
    # ins_text included); with the full `to` it is crdt_diff_async
    e = small.e
    picks = [[0, 1, 31, 32, 33, v // 3, v // 2 + 1, v - 1, v] for v in small.ver]
    total = 0
    for ka, kb in [(0, 8), (8, 0), (1, 5), (5, 1), (2, 3), (4, 6), (6, 2), (7, 3), (3, 7), (6, 6), (5, 8), (2, 8)]:
        a = [min(p[ka], v) for p, v in zip(picks, small.ver)]
        b = [min(p[kb], v) for p, v in zip(picks, small.ver)]
        fv, tv = e.version_vector(small.docs, a), e.version_vector(small.docs, b)
        for d in small.docs:
            assert np.array_equal(fv[d], ref_version_vector(small.ex[d], a[d], len(small.full[d]))), (d, a[d])
        res, (cf, ct) = diff_both(e, small.docs, fv, tv)
        assert cf.all() and ct.all()                   # a state the replica went through is closed
        want = e.diff_between(small.docs, a, b)
        for d in small.docs:
            same_arrays(res[d], want[d], ("between", d, a[d], b[d]))
            assert np.array_equal(res[d][0][:, 3], want[d][0][:, 3])
            total += res[d][0].shape[0]
        if kb == 8:
            now = e.diff(small.docs, a)
            for d in small.docs:
                same_arrays(res[d], now[d], ("diff", d, a[d]))
    assert total > 12 * small.n                        # (more than a patch per pair and document: 423)
    now = e.version_vector(small.docs)                 # version == NULL: now
    for d in small.docs:
        assert np.array_equal(now[d], small.full[d]), d


def test_delete_run_whose_member_part_is_no_prefix(small):
    # tests/diff_vv_cases.py neighbour_deletes: B's and C's delete ops are one run (10, 3, 2) of the
    # log; {A, C} holds its second order only, so item 4 is gone and item 3 is not
    d = small.neighbour
    assert np.asarray(small.ex[d]["deletes"]).reshape(-1, 3).tolist() == [[10, 3, 2]]
    ids = small.ids(d, "ABC")
    vvs = [vector(v, ids) for v in NEIGHBOUR_VECTORS]
    text = {}
    for i, a in enumerate(vvs):
        for j, b in enumerate(vvs):
            res, (cf, ct) = diff_both(small.e, [d], [a], [b])
            same(res[0], ref_diff_vv(small.ex[d], a, b), (NEIGHBOUR_VECTORS[i], NEIGHBOUR_VECTORS[j]))
            assert bool(cf[0]) == ref_vv_closed(small.ex[d], a) and bool(ct[0]) == ref_vv_closed(small.ex[d], b)
            if i == 0:
                text[j] = res[0][1]                    # from nothing: the inserted orders are the text
    assert text[3].tolist() == [0, 1, 2, 3, 5, 6, 7, 8, 9]        # {A: 10, C: 1}
    assert text[2].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9]        # {A: 10, B: 1}
    assert text[4].tolist() == [0, 1, 2, 5, 6, 7, 8, 9]


def test_long_span_and_many_spans(small):
    # one canonical span of 520 orders (d2_long: the whole wave walks it) cut by the vectors at
    # several places, and a document of more than DIFF_T canonical spans (the pass-to-pass carry),
    # every ordered pair of their vectors
    dl, dm = small.long, small.many
    canon = np.asarray(small.ex[dl]["canon"], np.uint32).reshape(-1, 4)
    assert int(np.abs(canon[:, 3].astype(np.int32)).max()) > DIFF2_LONG
    assert np.asarray(small.ex[dm]["canon"]).reshape(-1, 4).shape[0] > DIFF_T
    lv = [vector(v, small.ids(dl, "XYZW")) for v in LONG_VECTORS]
    mv = [vector(v, small.ids(dm, "PQD")) for v in MANY_VECTORS]
    n = max(len(lv), len(mv))
    total = in_second_pass = 0
    for i in range(n):
        for j in range(n):
            fv = [lv[i % len(lv)], mv[i % len(mv)]]
            tv = [lv[j % len(lv)], mv[j % len(mv)]]
            res, (cf, ct) = diff_both(small.e, [dl, dm], fv, tv)
            for k, d in enumerate((dl, dm)):
                total += same(res[k], ref_diff_vv(small.ex[d], fv[k], tv[k]), (d, fv[k], tv[k]))
                assert bool(cf[k]) == ref_vv_closed(small.ex[d], fv[k]) and bool(ct[k]) == ref_vv_closed(small.ex[d], tv[k])
                assert np.array_equal(res[k][2], small.content[res[k][1]])
            # items of orders below 300 - DIFF_T stand in the second pass of the many-span walk
            in_second_pass += int((res[1][1] < 300 - DIFF_T).any())
    assert total > 1000 and in_second_pass > 10
    # {X: 350}: X's first 300 and its orders 600 .. 649 around Y's 300, which are left out
    res, _ = diff_both(small.e, [dl], [np.zeros(0, np.uint32)], [lv[3]])
    assert res[0][1].tolist() == list(range(300)) + list(range(600, 650))


def test_lds_and_hbm_indexes_in_one_launch(small):
    # budgets between the documents' pair sizes: the launch has dynamic LDS for the pairs that fit
    # (xw > 0), the other documents' words are zeroed by the host and take the atomics in device
    # memory, and which way an index goes is decided block by block.  A pair is 2 x
    # pub_words(ord_cap) words with ord_cap above the document's orders, which are 12 to 1,340 here:
    # the powers of two from 2 to 8,192 words lie below every pair, between them and above all
    L = crdt_amd.lib()
    rng = np.random.default_rng(37)
    fv = [random_vectors(x, rng, 1)[0] for x in small.ex]
    tv = [random_vectors(x, rng, 1)[0] for x in small.ex]
    want, closed = diff_both(small.e, small.docs, fv, tv)
    assert min(small.ver) < 32 and max(small.ver) > 1024
    budgets = [2 << k for k in range(13)]
    try:
        for words in budgets:
            L.crdt_test_set_vv_lds_words(words)
            res = small.e.diff_vv(small.docs, fv, tv)
            cf, ct = small.e.diff_vv_closed()
            assert np.array_equal(cf, closed[0]) and np.array_equal(ct, closed[1]), words
            for d in small.docs:
                same_arrays(res[d], want[d], ("budget", words, d))
                same(res[d], ref_diff_vv(small.ex[d], fv[d], tv[d]), ("budget", words, d))
    finally:
        L.crdt_test_set_vv_lds_words(DEFAULT_LDS_WORDS)


def test_indexes_without_a_result():
    wire = concurrent_wire(1)[0]
    e = crdt_amd.Engine(6, 32)
    assert (e.apply_remote_wire([0, 2, 3, 4, 5], [wire] * 5) == 0).all()
    ag = int(e.agent_intern([1], ["p"])[0])
    bad = [[(0, 0, 5)], [(2, 1, 0)], [(3, 5, 0)], [(0, 0, 1)]]      # the third txn deletes past the end
    assert e.apply_local([(1, [(ag, o) for o in bad])])[0] == -1
    ex = e.export(0)
    full = next_seqs(ex).astype(np.uint32)
    dg = e.digests()
    over, longer = full.copy(), np.concatenate([full, [0]]).astype(np.uint32)
    over[1] += 1
    half = (full // 2).astype(np.uint32)
    docs = [0, 1, 2, 3, 4, 5]
    fv = [half, np.zeros(0, np.uint32), over, full, half, half]   # a poisoned document; an entry above the next seq
    tv = [full, np.zeros(0, np.uint32), full, half, longer, full]  # a vector longer than n_agents (its extra entry 0)
    res, (cf, ct) = diff_both(e, docs, fv, tv, strict=False)
    npat, nins = e.diff_counts()
    assert [int(x) == NO_RESULT for x in npat] == [False, True, True, False, True, False]
    assert [int(x) == NO_RESULT for x in nins] == [False, True, True, False, True, False]
    assert res[1] is None and res[2] is None and res[4] is None
    assert not cf[1] and not ct[1] and not cf[2] and not ct[4]
    for i in (1, 2, 4):
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.diff_read(i)
    # the neighbours are intact
    same(res[0], ref_diff_vv(ex, half, full), 0)
    same(res[3], ref_diff_vv(ex, full, half), 3)
    same(res[5], ref_diff_vv(ex, half, full), 5)
    same(e.diff_read(3), ref_diff_vv(ex, full, half), "read 3")
    assert res[0][2] is None                                       # (no content: no ins_text)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.diff_vv(docs, fv, tv)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.diff_vv([0, 0], [half, half], [full, full])              # a document named twice
    assert np.array_equal(e.digests(), dg)                         # the call changes no document
    # the flags belong to the vv call: another diff takes them away
    e.diff_between([0], [3], [9])
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.diff_vv_closed()
    e.diff_vv([0], [half], [full])
    assert e.diff_vv_closed()[0].shape == (1,)
    e.close()


def test_closed_flags(small):
    e = small.e
    # 1 for the vectors of order prefixes (test_prefix_vectors_give_the_two_version_diff: every one)
    # 0 for a vector that holds a txn without its parent: C's delete without B's, which C had seen
    d = small.neighbour
    ids = small.ids(d, "ABC")
    fv, tv = list(small.full), list(small.full)
    fv[d], tv[d] = vector({"A": 10, "C": 1}, ids), vector({"A": 10, "B": 1}, ids)
    _, (cf, ct) = diff_both(e, small.docs, fv, tv)
    assert not cf[d] and ct[d]
    assert cf[[x for x in small.docs if x != d]].all()
    # 0 for a vector that holds delete ops but not the seqs of the agents whose items they delete:
    # D's six deletes without P and Q; 1 for D's first three on all of P and Q
    d = small.many
    ids = small.ids(d, "PQD")
    ex = small.ex[d]
    fv[d], tv[d] = vector({"D": 6}, ids), vector({"P": 150, "Q": 150, "D": 3}, ids)
    _, (cf, ct) = diff_both(e, small.docs, fv, tv)
    assert not cf[d] and ct[d]
    assert ref_vv_closed(ex, tv[d]) and not ref_vv_closed(ex, fv[d])
    # the long span's: Z's delete ops 0 .. 6 are a prefix of its txn; X up to 350 without Y is open
    d = small.long
    ids = small.ids(d, "XYZW")
    fv[d], tv[d] = vector({"X": 400, "Y": 300, "Z": 7}, ids), vector({"X": 350}, ids)
    _, (cf, ct) = diff_both(e, small.docs, fv, tv)
    assert cf[d] and not ct[d]


def test_rebase_on_it(small):
    e = small.e
    rng = np.random.default_rng(31)
    fv = [random_vectors(x, rng, 1)[0] for x in small.ex]
    tv = [random_vectors(x, rng, 1)[0] for x in small.ex]
    res = e.diff_vv(small.docs, fv, tv)
    e.rebase_async("diff")
    counts = e.rebase_counts()
    spans = 0
    for d in small.docs:
        want = ref_diff_vv(small.ex[d], fv[d], tv[d])
        same(res[d], want, ("rebase", d))
        table = ref_rebase_table(want[0])
        assert int(counts[d]) == table.shape[0]
        assert np.array_equal(e.rebase_read(d, "chars", counts), table), d
        spans += table.shape[0]
    assert spans > 50


def test_version_vector(small):
    e = small.e
    for pick in (lambda v: 0, lambda v: 1, lambda v: v // 2, lambda v: v - 1, lambda v: v):
        vs = [pick(v) for v in small.ver]
        got = e.version_vector(small.docs, vs)
        for d in small.docs:
            assert np.array_equal(got[d], ref_version_vector(small.ex[d], vs[d], len(small.full[d]))), (d, vs[d])
    # inside a txn: the long span's X run cut at order 17, its Y run at 317
    d = small.long
    ids = small.ids(d, "XYZW")
    assert np.array_equal(e.version_vector([d], [17])[0], vector({"X": 17}, ids))
    assert np.array_equal(e.version_vector([d], [317])[0], vector({"X": 300, "Y": 17}, ids))
    assert np.array_equal(e.version_vector([d], [707])[0], vector({"X": 400, "Y": 300, "Z": 7}, ids))
    # a version above the document's; a slot smaller than the document's agents
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.version_vector([0, d], [0, small.ver[d] + 1])
    L = crdt_amd.lib()
    doc = np.array([d], np.uint32)
    off = np.array([0, 3], np.uint64)
    out = np.zeros(4, np.uint32)
    p32, p64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    assert L.crdt_version_vector(e.h, 1, doc.ctypes.data_as(p32), None, off.ctypes.data_as(p64), out.ctypes.data_as(p32)) == -100
    off[1] = 4
    assert L.crdt_version_vector(e.h, 1, doc.ctypes.data_as(p32), None, off.ctypes.data_as(p64), out.ctypes.data_as(p32)) == 0
    assert np.array_equal(out, small.full[d])


def test_allocation_failure_leaves_the_engine_usable():
    wire = concurrent_wire(2)[0]
    L = crdt_amd.lib()
    failed = 0
    for k in range(24):  # the first call of an engine allocates every buffer it needs: fail each in turn
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        ex = e.export(0)
        full = next_seqs(ex).astype(np.uint32)
        fv, tv = [full // 2, full], [full, full // 3]
        dg = e.digests()
        L.crdt_test_fail_alloc_after(k)
        try:
            e.diff_vv([0, 1], fv, tv)
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
        res = e.diff_vv([0, 1], fv, tv)
        same(res[0], ref_diff_vv(ex, fv[0], tv[0]), 0)
        same(res[1], ref_diff_vv(ex, fv[1], tv[1]), 1)
        e.close()
    assert 3 <= failed < 24, failed
