"""GPU checks of documents at a past version (crdt_checkout_async: k_diff_mark, k_co_rank, k_co_count,
k_result_scan<CoRes>, k_co_write; k_pos_to_loc_at / k_loc_to_pos_at) through the C ABI.  Every view must equal
tests/checkout_ref.py's ref_checkout of the engine's own export exactly; at versions that end a txn
the text, its digest and the two mappings must equal an oracle replay of the history's prefix.

k_co_count walks 256 canonical spans of a document per loop pass, k_co_write 64 per wave and chunk.
"""
import gzip
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from checkout_ref import ref_checkout, ref_queries_at  # noqa: E402
from diff_ref import apply_patches  # noqa: E402
from fuzz_gen import build_wire, concurrent_wire, parse_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from test_checkout_ref import truncated  # noqa: E402
from test_diff_ref import double_delete_txns  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS = 256  # canonical spans per pass of k_co_count's per-workgroup loop
NO_RESULT = 0xFFFFFFFF
INVALID = 0xFFFFFFFF


def caps(leaf):
    return (leaf, 16 if leaf == 32 else 8)


def same_as_ref(e, d, v, got, content=None):
    """view `got` = (order, text) of document d at v equals the reference; returns its length"""
    want = ref_checkout(e.export(d), v)
    order, text = got
    assert order.shape == want.shape and np.array_equal(order, want), (d, v, order[:8], want[:8])
    if content is not None:
        assert text is not None and np.array_equal(text, content[want]), (d, v)
    return want.shape[0]


def txn_len(t):
    return sum(op[5] for op in t[3])


def loc_names(agents, names):
    """agent ids -> names (None for the root / invalid agent 0xFFFF)"""
    return [None if int(a) == 0xFFFF else names[int(a)] for a in agents]


@pytest.mark.parametrize("leaf", [32, 4])
def test_every_version_of_a_tiny_history(leaf):
    # document d of next_order + 1 copies of one concurrent history is checked out at version d, in
    # one call: 0, the current version, inside txns, not a multiple of 32, delete runs cut by v
    wire, _ = concurrent_wire(3)
    names, txns = parse_wire(wire)
    names = [x for x in names if x != "ROOT"]
    o = OracleDoc(*caps(leaf))
    assert o.apply_remote_wire(wire) == 0
    n = o.sizes()["next_order"]
    assert 100 < n < 400
    e = crdt_amd.Engine(n + 1, leaf)
    e.stage_remote_replicated(wire, 0xFFFFFFFF, [""] * (n + 1))  # (no name of the batch is renamed)
    assert (e.run() == 0).all()
    assert (e.versions() == n).all()
    c = np.random.default_rng(3).integers(0x20, 0xD7FF, n, dtype=np.uint32)
    e.set_content(list(range(n + 1)), [0] * (n + 1), [c])
    # the engine's agent ids by name (a known name is a pure lookup); every copy interned alike
    ids = e.agent_intern([0] * len(names), names)
    eng_name = {int(a): nm for a, nm in zip(ids, names)}
    docs = np.arange(n + 1)
    res = e.checkout(docs, docs)
    lens = e.checkout_lens()
    dg = e.checkout_digests()
    for d in range(n + 1):
        assert same_as_ref(e, d, d, res[d], c) == int(lens[d])
    assert lens[0] == 0 and int(dg[0]) == OracleDoc(*caps(leaf)).text(c)[1]
    assert np.array_equal(res[n][1], e.text(n)) and dg[n] == e.text_digests()[n]
    assert e.checkout_ms() > 0
    # every (agent, seq) the full history assigned, and one seq past each agent's last
    cwo = e.export(0)["cwo"].astype(np.int64)
    run_len = cwo[:, 3]
    loc_a = np.repeat(cwo[:, 1], run_len)
    loc_s = np.repeat(cwo[:, 2], run_len) + (np.arange(n) - np.repeat(np.cumsum(run_len) - run_len, run_len))
    agents = np.unique(cwo[:, 1])
    past = [loc_s[loc_a == a].max() + 1 for a in agents]
    loc_a, loc_s = np.concatenate([loc_a, agents]), np.concatenate([loc_s, past])
    assert loc_a.shape[0] == n + agents.shape[0]
    v = 0
    for k in range(1, len(txns) + 1):  # every version that ends a txn: an oracle prefix replay
        v += txn_len(txns[k - 1])
        p = OracleDoc(*caps(leaf))
        assert p.apply_remote_wire(build_wire(txns[:k])) == 0 and p.sizes()["next_order"] == v
        text, digest = p.text(c)
        assert np.array_equal(res[v][1], text) and int(dg[v]) == digest, v
        ora_id = {nm: p.agent(nm) for nm in names}
        ora_name = {i: nm for nm, i in ora_id.items()}
        pos = np.arange(int(lens[v]) + 2, dtype=np.uint32)
        ga, gs = e.pos_to_loc_at(np.full(pos.shape, v), pos)
        oa, os_ = p.pos_to_loc(pos)
        assert np.array_equal(gs, os_), v
        assert loc_names(ga, eng_name) == loc_names(oa, ora_name), v
        assert int(ga[-1]) == 0xFFFF and int(gs[-1]) == INVALID and int(ga[-2]) == 0xFFFF
        gp, gd = e.loc_to_pos_at(np.full(loc_a.shape, v), loc_a, loc_s)
        op, od = p.loc_to_pos([ora_id[eng_name[int(a)]] for a in loc_a], loc_s)
        assert np.array_equal(gd, od), v
        assert np.array_equal(gp[od != 2], op[od != 2]), v
        if v < n:
            assert (gd == 2).sum() > agents.shape[0]  # ids not yet known at v


@pytest.mark.parametrize("swap", [False, True])
def test_double_deletes(swap):
    txns = double_delete_txns()
    if swap:
        txns = [txns[0], txns[2], txns[1]]
    e = crdt_amd.Engine(19, 32)
    assert (e.apply_remote_wire(list(range(19)), [build_wire(txns)] * 19) == 0).all()
    c = np.arange(100, 118, dtype=np.uint32)
    e.set_content(list(range(19)), [0] * 19, [c])
    res = e.checkout(list(range(19)), list(range(19)))
    dg = e.checkout_digests()
    for v in range(19):
        same_as_ref(e, v, v, res[v], c)
    for v in (0, 10, 14, 18):  # the versions that end a txn
        p = OracleDoc()
        if v:
            assert p.apply_remote_wire(build_wire(truncated(txns, v))) == 0
        assert p.sizes()["next_order"] == v
        text, digest = p.text(c)
        assert np.array_equal(res[v][1], text) and int(dg[v]) == digest
    assert res[14][0].tolist() == ([0, 1, 2, 3, 8, 9] if swap else [0, 1, 6, 7, 8, 9])
    assert res[12][0].tolist() == ([0, 1, 2, 3, 6, 7, 8, 9] if swap else [0, 1, 4, 5, 6, 7, 8, 9])
    # items 4 and 5 are deleted twice: gone from the first delete on, whichever txn came first
    p, dl = e.loc_to_pos_at([12, 14, 18, 9], [0] * 4, [4] * 4)
    assert dl.tolist() == ([1, 1, 1, 0] if swap else [0, 1, 1, 0]) and p.tolist() == ([4, 4, 2, 4] if swap else [2, 2, 2, 4])


def test_wide_document_with_an_empty_and_a_one_item_document():
    # 700 single-char inserts at position 0 are 700 canonical spans (document order is the reverse
    # of the orders); deletes and inserts in the middle split them further: two full passes of
    # k_co_count's loop and a remainder, eleven 64-span chunks of k_co_write and a partial one
    first = [[(0, 0, 1)] for _ in range(700)]
    second = [[(3 * j, 1, 0)] for j in range(100)] + [[(5 * j + 1, 0, 2)] for j in range(60)]
    e = crdt_amd.Engine(5, 32)
    ag = e.agent_intern(list(range(5)), ["w"] * 5)
    wide = [0, 3, 4]
    assert (e.apply_local([(d, [(int(ag[d]), op) for op in first]) for d in wide]) == 0).all()
    assert int(e.versions([0])[0]) == 700
    assert (e.apply_local([(d, [(int(ag[d]), op) for op in second]) for d in wide] +
                          [(2, [(int(ag[2]), [(0, 0, 1)])])]) == 0).all()
    cn = e.canon_counts()
    assert cn[0] >= 2 * PASS + 1 and cn[0] % PASS != 0 and cn[0] % 64 != 0, cn
    n = int(e.versions([0])[0])
    c = np.random.default_rng(11).integers(0x20, 0xD7FF, n, dtype=np.uint32)
    e.set_content(wide + [1, 2], [0] * 5, [c])
    docs = [0, 1, 2, 3, 4]
    for versions in ([700, 0, 1, 333, n], [n - 37, 0, 0, 65, 257], [750, 0, 1, 0, 1]):
        res = e.checkout(docs, versions)
        lens = e.checkout_lens()
        for d, v in zip(docs, versions):
            assert same_as_ref(e, d, v, res[d], c) == int(lens[d])
        assert lens[1] == 0                                      # the empty document
        assert res[2][0].tolist() == ([0] if versions[2] else [])  # the one-item document
    res = e.checkout(docs, [700, 0, 1, 333, n])
    assert res[0][0].shape[0] == 700 and np.array_equal(res[0][0], np.arange(700)[::-1])
    for d, s in ((0, 700), (3, 333)):
        o = OracleDoc()
        a = o.agent("w")
        for op in first[:s]:
            assert o.apply_local(a, op) == 0
        text, digest = o.text(c)
        assert np.array_equal(res[d][1], text) and int(e.checkout_digests()[d]) == digest
    assert np.array_equal(res[4][1], e.text(4)) and e.checkout_digests()[4] == e.text_digests()[4]


@pytest.mark.parametrize("name", ["bs200", "del1", "jump10"])
def test_patterns(name):
    # backspace runs, single deletes and jumps: a 50,000-char base then 20,000 one-item ops of one
    # shape, applied in two halves cut in the middle of the ops; "half + 3" lies three ops further,
    # inside a backspace run.  (These traces' deleted canonical spans stay short: the deleted span of
    # more than 256 orders that v cuts is test_bitmap_past_the_lds_threshold's.)
    with gzip.open(os.path.join(ROOT, "data", "micro", name + ".rtx.gz"), "rb") as f:
        txns = parse_wire(f.read())[1]
    k = 60000
    e = crdt_amd.Engine(4, 32)
    docs = [0, 1, 2, 3]
    assert (e.apply_remote_wire(docs, [build_wire(txns[:k])] * 4) == 0).all()
    half = int(e.versions()[0])
    assert (e.apply_remote_wire(docs, [build_wire(txns[k:])] * 4) == 0).all()
    n = int(e.versions()[0])
    c = np.random.default_rng(7).integers(0x20, 0xD7FF, n, dtype=np.uint32)
    e.set_content(docs, [0] * 4, [c])
    versions = [half, 0, n, half + 3]
    res = e.checkout(docs, versions)
    dg = e.checkout_digests()
    ex = e.export(0)
    for d, v in zip(docs, versions):
        want = ref_checkout(ex, v)  # (the four documents hold the same history)
        assert np.array_equal(res[d][0], want) and np.array_equal(res[d][1], c[want]), (d, v)
    o = OracleDoc()
    assert o.apply_remote_wire(build_wire(txns[:k])) == 0 and o.sizes()["next_order"] == half
    text, digest = o.text(c)
    assert np.array_equal(res[0][1], text) and int(dg[0]) == digest
    assert res[1][0].shape[0] == 0
    assert np.array_equal(res[2][1], e.text(2)) and dg[2] == e.text_digests()[2]
    # the diff from the same version turns the checked-out text into the current one
    patches = e.diff(docs, versions)
    for d in docs:
        pat, _, it = patches[d]
        assert np.array_equal(apply_patches(res[d][1], pat, it), e.text(d)), d


def test_bitmap_past_the_lds_threshold():
    # k_diff_mark builds bitmaps of up to 16,384 words in LDS and larger ones with atomics in HBM:
    # a 650,000-order document on either side of a small one, in one call.  Document 2 is checked
    # out inside the 50,000-item delete run: the deleted span of 50,200 items is cut by v
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
    versions = [int(v[0]), int(v[1]), 625_001]
    res = e.checkout([0, 1, 2], versions, strict=True)
    rng = np.random.default_rng(5)
    for d in (0, 1, 2):
        ex = e.export(d)
        n_ord = same_as_ref(e, d, versions[d], res[d])
        order = res[d][0]
        cwo = ex["cwo"].astype(np.int64)
        # 1,000 positions (and the two past the end) -> (agent, seq) through client_with_order
        pos = np.append(rng.integers(0, max(n_ord, 1), 1000), [n_ord, n_ord + 1]).astype(np.uint32)
        ga, gs = e.pos_to_loc_at(np.full(pos.shape, d), pos)
        ok = pos < n_ord
        x = order[pos[ok]].astype(np.int64)
        r = np.searchsorted(cwo[:, 0], x, side="right") - 1
        assert np.array_equal(ga[ok], cwo[r, 1]) and np.array_equal(gs[ok], cwo[r, 2] + (x - cwo[r, 0]))
        assert (ga[~ok] == 0xFFFF).all() and (gs[~ok] == INVALID).all()
        # 1,000 orders of any kind (items in the view, deleted before v, not yet known, delete ops)
        want_p, want_d = ref_queries_at(order, ex, versions[d])
        x = rng.integers(0, ex["next_order"], 1000)
        r = np.searchsorted(cwo[:, 0], x, side="right") - 1
        gp, gd = e.loc_to_pos_at(np.full(x.shape, d), cwo[r, 1], cwo[r, 2] + (x - cwo[r, 0]))
        assert np.array_equal(gd, want_d[x]) and np.array_equal(gp, want_p[x]), d
        if d != 1:
            assert set(gd.tolist()) == {0, 1, 2}
    assert res[2][0].shape[0] == 600_000 - 25_001


def test_errors_and_purity():
    wire, _ = concurrent_wire(1)
    e = crdt_amd.Engine(4, 32)
    assert (e.apply_remote_wire([0, 2, 3], [wire] * 3) == 0).all()
    ag = int(e.agent_intern([1], ["p"])[0])
    bad = [[(0, 0, 5)], [(2, 1, 0)], [(3, 5, 0)], [(0, 0, 1)]]      # the third txn deletes past the end
    assert e.apply_local([(1, [(ag, o) for o in bad])])[0] == -1
    ver = e.versions()
    n = int(ver[0])
    c = np.random.default_rng(2).integers(0x20, 0xD7FF, n, dtype=np.uint32)
    e.set_content([0, 2], [0, 0], [c])                              # document 3 has no content
    dg = e.digests()
    text0 = e.text(0)
    d0 = e.diff([0], [5])[0]
    docs, versions = [0, 1, 2, 3], [5, 0, int(ver[2]) + 1, n]
    res = e.checkout(docs, versions, strict=False)
    lens = e.checkout_lens()
    assert [int(x) == NO_RESULT for x in lens] == [False, True, True, False]
    assert res[1] is None and res[2] is None
    for i in (1, 2, 4):  # the poisoned document; a version above the document's; out of range
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.checkout_read(i)
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.pos_to_loc_at([0, i], [0, 0])
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.loc_to_pos_at([i, 0], [0, 0], [0, 0])
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.checkout(docs, versions)
    # the neighbours' results are intact; without content there is no text, but the orders read
    same_as_ref(e, 0, 5, res[0], c)
    same_as_ref(e, 3, n, res[3])
    assert res[3][1] is None and e.checkout_digests()[3] == 0
    buf = np.zeros(int(lens[3]), np.uint32)  # (the library's own answer for text without content)
    assert e.L.crdt_checkout_read(e.h, 3, None, crdt_amd._p(buf)) == -100
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.checkout([0, 0], [0, 0])  # a document named twice
    # at v = version the _at queries are the queries on the current state
    res = e.checkout(docs, versions, strict=False)
    pos = np.arange(int(lens[3]) + 2, dtype=np.uint32)
    a1, s1 = e.pos_to_loc_at(np.full(pos.shape, 3), pos)
    a2, s2 = e.pos_to_loc(np.full(pos.shape, 3), pos)
    assert np.array_equal(a1, a2) and np.array_equal(s1, s2)
    p1, dl1 = e.loc_to_pos_at(np.full(pos.shape, 3), a2, s2)
    p2, dl2 = e.loc_to_pos(np.full(pos.shape, 3), a2, s2)
    assert np.array_equal(p1, p2) and np.array_equal(dl1, dl2)
    for a in range(3):
        seq = np.arange(n + 1, dtype=np.uint32)
        p1, dl1 = e.loc_to_pos_at(np.full(seq.shape, 3), np.full(seq.shape, a), seq)
        p2, dl2 = e.loc_to_pos(np.full(seq.shape, 3), np.full(seq.shape, a), seq)
        assert np.array_equal(dl1, dl2) and np.array_equal(p1[dl2 != 2], p2[dl2 != 2])
    # a checkout changes no document, the text or an earlier diff result
    assert np.array_equal(e.digests(), dg) and np.array_equal(e.versions(), ver)
    assert np.array_equal(e.text(0), text0)
    again = e.diff_read(0)
    assert np.array_equal(again[0], d0[0]) and np.array_equal(again[1], d0[1]) and np.array_equal(again[2], d0[2])
    # after a further apply the arrays still read, the queries do not answer
    a3 = int(e.agent_intern([3], ["late"])[0])
    before = e.checkout_read(0)
    assert e.apply_local([(3, [(a3, [(0, 0, 2)])])])[0] == 0
    after = e.checkout_read(0)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    same_as_ref(e, 0, 5, after, c)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.pos_to_loc_at([0], [0])
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.loc_to_pos_at([0], [0], [0])
    e.sync()
    e.publish_async()  # (publishing alone does not bring them back: the views are of the old index)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.pos_to_loc_at([0], [0])
    # a second call replaces the first one's result
    res = e.checkout([3], [7])
    assert e.checkout_lens().shape[0] == 1
    same_as_ref(e, 3, 7, res[0])
    a1, s1 = e.pos_to_loc_at([0], [0])
    assert int(a1[0]) != 0xFFFF
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.checkout_read(1)


def test_allocation_failure_leaves_the_engine_usable():
    wire, _ = concurrent_wire(2)
    L = crdt_amd.lib()
    failed = 0
    for k in range(24):  # the first checkout of an engine allocates every buffer it needs: fail each in turn
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        dg = e.digests()
        L.crdt_test_fail_alloc_after(k)
        try:
            e.checkout([0, 1], [9, 0])
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
        # no relayout was involved: the engine is not poisoned, it has no checkout, and the same
        # checkout then succeeds
        assert np.array_equal(e.digests(), dg)
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.checkout_lens()
        res = e.checkout([0, 1], [9, 0])
        same_as_ref(e, 0, 9, res[0])
        same_as_ref(e, 1, 0, res[1])
        a, s = e.pos_to_loc_at([0], [0])
        assert int(a[0]) != 0xFFFF
        e.close()
    assert 1 <= failed < 24, failed


def test_one_document_forms_and_device_pointer_queries():
    import torch
    from crdt_amd.traces import utf32_to_str
    d = crdt_amd.ListCRDT()
    a = d.get_or_create_agent_id("seph")
    assert d.local_insert(a, 0, 5) == 0          # hello
    v1 = d.version()
    assert d.local_delete(a, 1, 3) == 0          # ho
    v2 = d.version()
    assert d.local_insert(a, 1, 2) == 0          # h + "ey" + o
    c = np.array([ord(x) for x in "hello"] + [0] * 3 + [ord(x) for x in "ey"], np.uint32)
    d.set_content(c)
    assert d.to_string() == "heyo"
    assert [d.to_string_at(v) for v in (0, 3, v1, v1 + 2, v2, d.version())] == ["", "hel", "hello", "hlo", "ho", "heyo"]
    assert utf32_to_str(d.text_at(v1 + 1)) == "hllo"
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        d.text_at(d.version() + 1)
    # device-pointer forms on the view at v1 + 2 ("hlo"); an idx out of range is answered as invalid
    e = d.e
    e.checkout_async([0], [v1 + 2])
    dev = "cuda"
    idx = torch.tensor([0, 0, 0, 0, 7], dtype=torch.int32, device=dev)
    pos = torch.tensor([0, 1, 2, 3, 0], dtype=torch.int32, device=dev)
    ag = torch.zeros(5, dtype=torch.int16, device=dev)
    sq = torch.zeros(5, dtype=torch.int32, device=dev)
    assert e.L.crdt_pos_to_loc_at_dev_async(e.h, 5, idx.data_ptr(), pos.data_ptr(), ag.data_ptr(), sq.data_ptr()) == 0
    out_p = torch.zeros(5, dtype=torch.int32, device=dev)
    out_d = torch.zeros(5, dtype=torch.uint8, device=dev)
    seq = torch.tensor([0, 1, 3, 8, 0], dtype=torch.int32, device=dev)  # h; e (deleted); l; "e" of "ey" (not yet known)
    agq = torch.full((5,), a, dtype=torch.int16, device=dev)
    assert e.L.crdt_loc_to_pos_at_dev_async(e.h, 5, idx.data_ptr(), agq.data_ptr(), seq.data_ptr(), out_p.data_ptr(),
                                            out_d.data_ptr()) == 0
    e.sync()
    assert sq.cpu().numpy().view(np.uint32).tolist() == [0, 3, 4, INVALID, INVALID]
    assert ag.cpu().numpy().view(np.uint16).tolist() == [a, a, a, 0xFFFF, 0xFFFF]
    assert out_d.cpu().tolist() == [0, 1, 0, 2, 2]
    assert out_p.cpu().numpy().view(np.uint32).tolist() == [0, 1, 1, INVALID, INVALID]
