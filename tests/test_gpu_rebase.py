"""GPU checks of the rebase map (crdt_rebase_async: k_rebase_build; crdt_rebase / crdt_rebase_dev_async:
k_rebase) through the C ABI.  Every table must equal tests/rebase_ref.py's ref_rebase_table of the
reference diff / edits of the engine's own export, and every answer ref_rebase on that table, exactly.

k_rebase_build takes 256 patches of an index per loop pass and carries the running ins - del sums
from pass to pass.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (before the first engine: torch finds no GPU once another HIP runtime is up)

import crdt_amd  # noqa: E402
from diff_ref import ref_diff  # noqa: E402
from edits_ref import mixed_content, ref_edits  # noqa: E402
from encode_ref import UTF8, UTF16, ref_encode  # noqa: E402
from fuzz_gen import concurrent_wire, parse_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from rebase_ref import LEFT, NEW_TO_OLD, OLD_TO_NEW, RIGHT, ref_rebase_many, ref_rebase_table  # noqa: E402
from test_diff_ref import replay  # noqa: E402

ENCS = {"utf8": UTF8, "utf16": UTF16}
DIRS = (("old_to_new", OLD_TO_NEW), ("new_to_old", NEW_TO_OLD))
BIASES = (("left", LEFT), ("right", RIGHT))
BUILD_PASS = 256  # patches per pass of k_rebase_build's per-workgroup loop
NO_RESULT = 0xFFFFFFFF
E_ARG = "rc=-100"


def caps(leaf):
    return (leaf, 16 if leaf == 32 else 8)


def check_tables(e, tables, kind="chars"):
    """the map's tables of `kind` equal `tables` (one per index; None: no result)"""
    counts = e.rebase_counts()
    assert len(counts) == len(tables)
    for i, w in enumerate(tables):
        if w is None:
            assert int(counts[i]) == NO_RESULT
            continue
        assert int(counts[i]) == w.shape[0], (i, counts[i], w.shape)
        got = e.rebase_read(i, kind, counts)
        assert got.dtype == np.uint32 and got.shape == w.shape and np.array_equal(got, w), (i, kind, got[:4], w[:4])
    return counts


def sweep(idxs, tables, lens, dir, step=1):
    """every x in [0, len + 2] (every step-th) of every listed index, with the reference's answers
    per bias: (idx, x, {bias: (y, hit)})"""
    qi = np.concatenate([np.full(len(range(0, n + 3, step)), i, np.uint32) for i, n in zip(idxs, lens)])
    qx = np.concatenate([np.arange(0, n + 3, step, dtype=np.uint32) for n in lens])
    want = {}
    for _, b in BIASES:
        got = [ref_rebase_many(t, range(0, n + 3, step), dir, b) for t, n in zip(tables, lens)]
        want[b] = (np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got]))
    return qi, qx, want


def check_queries(e, idxs, tables, old_lens, new_lens, kind="chars", step=1, seed=5):
    """both directions and both biases over every position, several indexes mixed in one call each"""
    for (dirname, d), lens in zip(DIRS, (old_lens, new_lens)):
        qi, qx, want = sweep(idxs, tables, lens, d, step)
        o = np.random.default_rng(seed).permutation(len(qi))
        for biasname, b in BIASES:
            y, hit = e.rebase(qi[o], qx[o], kind, dirname, biasname)
            assert np.array_equal(y, want[b][0][o]), (kind, dirname, biasname)
            assert np.array_equal(hit, want[b][1][o]), (kind, dirname, biasname)


def dev_rebase(e, qi, qx, kind, dir, bias, with_hit=True):
    """the device-pointer form on torch buffers, on the engine's stream: (y, hit or None)"""
    with torch.cuda.stream(torch.cuda.ExternalStream(e.stream(), device=torch.cuda.current_device())):
        ti = torch.from_numpy(np.ascontiguousarray(qi, np.uint32).view(np.int32)).to("cuda", non_blocking=False)
        tx = torch.from_numpy(np.ascontiguousarray(qx, np.uint32).view(np.int32)).to("cuda", non_blocking=False)
        y = torch.full((len(qi),), 7, dtype=torch.int32, device="cuda")
        h = torch.full((len(qi),), 7, dtype=torch.uint8, device="cuda")
        rc = e.L.crdt_rebase_dev_async(e.h, len(qi), ti.data_ptr(), tx.data_ptr(), kind, dir, bias, y.data_ptr(),
                                       h.data_ptr() if with_hit else None)
        assert rc == 0, rc
        e.sync()
        return y.cpu().numpy().view(np.uint32), h.cpu().numpy() if with_hit else None


@pytest.mark.parametrize("leaf", [32, 4])
def test_every_version_of_a_tiny_history(leaf):
    # document d of next_order + 1 copies of one concurrent history, mapped from version d: since = 0,
    # = version, inside txns, delete runs that straddle since
    wire, _ = concurrent_wire(3)
    o = OracleDoc(*caps(leaf))
    assert o.apply_remote_wire(wire) == 0
    n = o.sizes()["next_order"]
    assert 100 < n < 400
    e = crdt_amd.Engine(n + 1, leaf)
    e.stage_remote_replicated(wire, 0xFFFFFFFF, [""] * (n + 1))  # (no name of the batch is renamed)
    assert (e.run() == 0).all()
    assert (e.versions() == n).all()
    docs = np.arange(n + 1, dtype=np.uint32)
    dg = e.digests()
    assert (dg == dg[0]).all()  # the copies are one document: one export serves every reference
    ex = e.export(0)
    e.diff_async(docs, docs)
    e.rebase_async("diff")
    tables = [ref_rebase_table(ref_diff(ex, d)[0]) for d in range(n + 1)]
    counts = check_tables(e, tables)
    assert int(counts.sum()) > n  # (many versions need several spans)
    assert e.rebase_ms() > 0
    new_len = int(e.lens([0])[0])
    assert new_len == len(o)
    e.checkout_async(docs, docs)
    old_lens = e.checkout_lens().astype(np.int64).tolist()
    check_queries(e, docs.tolist(), tables, old_lens, [new_len] * (n + 1))
    # through other kernels: an old position on a kept item is where the item's id now stands
    qi = np.concatenate([np.full(m, d, np.uint32) for d, m in enumerate(old_lens)])
    qx = np.concatenate([np.arange(m, dtype=np.uint32) for m in old_lens])
    ag, sq = e.pos_to_loc_at(qi, qx)
    pos, deleted = e.loc_to_pos(qi, ag, sq)
    kept = deleted == 0
    assert kept.sum() > n and (deleted[~kept] == 1).all()
    y, hit = e.rebase(qi[kept], qx[kept], "chars", "old_to_new", "right")
    assert np.array_equal(y, pos[kept]) and not hit.any()
    back, hit = e.rebase(qi[kept], y, "chars", "new_to_old", "right")
    assert np.array_equal(back, qx[kept]) and not hit.any()
    # since = version: no span, the identity map
    assert counts[n] == 0 and e.rebase_read(n).shape == (0, 4)
    xs = np.arange(new_len + 3, dtype=np.uint32)
    for dirname, _ in DIRS:
        for biasname, _ in BIASES:
            y, hit = e.rebase(np.full(len(xs), n, np.uint32), xs, "chars", dirname, biasname)
            assert np.array_equal(y, xs) and not hit.any()
    # since = 0: the whole text is one insertion
    assert e.rebase_read(0).tolist() == [[0, 0, 0, new_len]]


@pytest.mark.parametrize("encname", list(ENCS))
def test_edits_source_both_tables(encname):
    enc = ENCS[encname]
    wires = [concurrent_wire(s)[0] for s in range(4)]
    e = crdt_amd.Engine(4, 32)
    assert (e.apply_remote_wire(list(range(4)), wires) == 0).all()
    ver = e.versions()
    streams = [mixed_content(int(v), 20 + i) for i, v in enumerate(ver)]
    e.set_content(list(range(4)), list(range(4)), streams)
    docs = [2, 0, 3, 1]
    # the version each document had after a prefix of its txns, and the oracle's text there
    olds, since = [], []
    for i, d in enumerate(docs):
        txns = parse_wire(wires[d])[1]
        old = replay(txns[:len(txns) // (i + 2) + 1])
        olds.append(old)
        since.append(old.sizes()["next_order"])
    assert all(0 < s < int(ver[d]) for s, d in zip(since, docs))
    e.edits_async(docs, since, encname)
    e.rebase_async("edits")
    eds = [ref_edits(e.export(d), s, streams[d], enc)[0] for d, s in zip(docs, since)]
    ct = [ref_rebase_table(x) for x in eds]
    ut = [ref_rebase_table(x, units=True) for x in eds]
    counts = check_tables(e, ct, "chars")
    check_tables(e, ut, "units")
    assert int(counts.sum()) > 8
    new_enc = e.encode(docs, encname)
    units_new, chars_new = e.encode_lens()
    n_kept = 0
    old_chars, old_units = [], []
    for i, d in enumerate(docs):
        ids = np.arange(int(ver[d]), dtype=np.uint32)
        old_orders = olds[i].text(ids)[0]      # content = the orders: a text is its items' orders
        new_orders = e.checkout([d], [int(ver[d])])[0][0]
        assert len(new_orders) == chars_new[i]
        start_old = ref_encode(streams[d][old_orders], enc)[1]
        old_chars.append(len(old_orders))
        old_units.append(int(start_old[-1]))
        at = {int(x): k for k, x in enumerate(new_orders)}
        kept = [(k, at[int(x)]) for k, x in enumerate(old_orders) if int(x) in at]
        n_kept += len(kept)
        idx = np.full(len(kept), i, np.uint32)
        # a kept char's old unit offset maps to its unit offset in the encode of the current text
        want = e.pos_to_units(idx, [b for _, b in kept])
        y, hit = e.rebase(idx, [int(start_old[a]) for a, _ in kept], "units", "old_to_new", "right")
        assert np.array_equal(y, want) and not hit.any()
        y, hit = e.rebase(idx, [a for a, _ in kept], "chars", "old_to_new", "right")
        assert y.tolist() == [b for _, b in kept] and not hit.any()
    assert n_kept > 40
    assert len(new_enc) == 4
    check_queries(e, list(range(4)), ut, old_units, units_new.astype(np.int64).tolist(), "units")
    check_queries(e, list(range(4)), ct, old_chars, chars_new.astype(np.int64).tolist(), "chars")
    # a map built from a diff has no unit table
    e.diff_async(docs, since)
    e.rebase_async("diff")
    check_tables(e, ct, "chars")
    one = np.zeros(1, np.uint32)
    with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
        e.rebase(one, one, "units")
    with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
        e.rebase_read(0, "units")
    assert e.L.crdt_rebase_dev_async(e.h, 0, None, None, 1, 0, 0, None, None) == -100


def test_more_than_two_build_passes():
    # 1,400 single-char inserts at position 0, then every other one of the first 1,200 deleted one
    # txn at a time: 600 patches that no two of which touch, plus inserts: at least two full passes
    # of k_rebase_build's loop and a remainder, next to an empty and a one-item document
    first = [[(0, 0, 1)] for _ in range(1400)]
    second = [[(j, 1, 0)] for j in range(600)] + [[(7 * j + 3, 0, 1 + j % 3)] for j in range(40)]
    e = crdt_amd.Engine(3, 32)
    ag = e.agent_intern([0, 1, 2], ["w"] * 3)
    assert (e.apply_local([(0, [(int(ag[0]), op) for op in first])]) == 0).all()
    v = int(e.versions([0])[0])
    assert v == 1400
    assert (e.apply_local([(0, [(int(ag[0]), op) for op in second]), (2, [(int(ag[2]), [(0, 0, 1)])])]) == 0).all()
    docs, since = [0, 1, 2], [v, 0, 0]
    n = int(e.versions([0])[0])
    c = mixed_content(n, 11)
    e.set_content(docs, [0] * 3, [c])
    exs = [e.export(d) for d in docs]
    new_lens = e.lens(docs).astype(np.int64).tolist()
    old_lens = [1400, 0, 0]
    e.diff_async(docs, since)
    e.rebase_async("diff")
    tables = [ref_rebase_table(ref_diff(x, s)[0]) for x, s in zip(exs, since)]
    counts = check_tables(e, tables)
    assert counts[0] >= 2 * BUILD_PASS + 1 and counts[0] % BUILD_PASS != 0, counts
    assert counts[1] == 0 and e.rebase_read(2).tolist() == [[0, 0, 0, 1]]
    check_queries(e, docs, tables, old_lens, new_lens)
    # the unit sums carry from pass to pass too
    e.edits_async(docs, since, "utf8")
    e.rebase_async("edits")
    eds = [ref_edits(x, s, c, UTF8)[0] for x, s in zip(exs, since)]
    check_tables(e, tables, "chars")
    ut = [ref_rebase_table(x, units=True) for x in eds]
    check_tables(e, ut, "units")
    old_units = [int(ut[0][-1, 0]) + int(ut[0][-1, 1]) + 5, 0, 0]
    new_units = [len(ref_encode(e.text(d), UTF8)[0]) for d in docs]
    check_queries(e, docs, ut, old_units, new_units, "units", step=3)


def test_per_index_errors_and_argument_errors():
    wire, _ = concurrent_wire(1)
    e = crdt_amd.Engine(3, 32)
    one = np.zeros(1, np.uint32)
    assert (e.apply_remote_wire([0, 1, 2], [wire] * 3) == 0).all()
    # before any diff, and before any map
    for src in ("diff", "edits"):
        with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
            e.rebase_async(src)
    for call in (e.rebase_counts, lambda: e.rebase_read(0), lambda: e.rebase(one, one)):
        with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
            call()
    assert e.rebase_ms() == 0
    assert e.L.crdt_rebase_dev_async(e.h, 1, None, None, 0, 0, 0, None, None) == -100
    nv = int(e.versions([0])[0])
    ex = e.export(0)
    since = [3, nv + 1, 0]
    e.diff_async([0, 1, 2], since)
    with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
        e.rebase_async("edits")  # the other source still has none
    for src in (2, -1):
        with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
            e.rebase_async(src)
    e.rebase_async("diff")
    tables = [ref_rebase_table(ref_diff(ex, 3)[0]), None, ref_rebase_table(ref_diff(ex, 0)[0])]
    counts = check_tables(e, tables)
    assert counts[1] == NO_RESULT
    with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
        e.rebase_read(1)
    assert e.L.crdt_rebase_read(e.h, 1, 0, None) == -100
    with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
        e.rebase_read(3)
    # a host query that names an index without a result, or one out of range, fails whole and writes nothing
    u32p, u8p = crdt_amd._p, lambda a: crdt_amd._p(a, crdt_amd.C.c_uint8)
    for bad in (1, 3, 0x7FFFFFFF):
        qi = np.array([0, bad, 2], np.uint32)
        qx = np.array([1, 1, 1], np.uint32)
        y, hit = np.full(3, 7, np.uint32), np.full(3, 7, np.uint8)
        assert e.L.crdt_rebase(e.h, 3, u32p(qi), u32p(qx), 0, 0, 1, u32p(y), u8p(hit)) == -100
        assert (y == 7).all() and (hit == 7).all()
    # the device form answers such a query 0xFFFFFFFF with hit 0; the others are not affected
    qi = np.array([0, 1, 3, 0x7FFFFFFF, 2, 0xFFFFFFFF], np.uint32)
    qx = np.array([5, 5, 5, 5, 5, 5], np.uint32)
    good = np.array([True, False, False, False, True, False])
    for _, d in DIRS:
        for _, b in BIASES:
            y, hit = dev_rebase(e, qi, qx, 0, d, b)
            wy, wh = e.rebase(qi[good], qx[good], 0, d, b)
            assert np.array_equal(y[good], wy) and np.array_equal(hit[good], wh)
            assert (y[~good] == NO_RESULT).all() and (hit[~good] == 0).all()
    # unknown kind / dir / bias, in both forms
    for kind, d, b in ((2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 2), (0, 0, -1)):
        with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
            e.rebase(one, one, kind, d, b)
        assert e.L.crdt_rebase_dev_async(e.h, 0, None, None, kind, d, b, None, None) == -100
    with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
        e.rebase_read(0, 2)
    # n = 0 is a no-op in both forms
    y, hit = e.rebase([], [])
    assert y.shape == (0,) and hit.shape == (0,)
    assert e.L.crdt_rebase(e.h, 0, None, None, 0, 0, 0, None, None) == 0
    assert e.L.crdt_rebase_dev_async(e.h, 0, None, None, 0, 1, 1, None, None) == 0
    # hit is optional
    y = np.full(2, 7, np.uint32)
    qi = np.array([0, 2], np.uint32)
    assert e.L.crdt_rebase(e.h, 2, u32p(qi), u32p(qi), 0, 0, 1, u32p(y), None) == 0
    assert np.array_equal(y, e.rebase(qi, qi)[0])
    # (calls rejected for their arguments left the map)
    check_tables(e, tables)
    # a diff of no document gives a map of no index
    e.diff_async([], [])
    e.rebase_async("diff")
    assert len(e.rebase_counts()) == 0
    with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
        e.rebase(one, one)


def test_lifetime_of_the_map_and_the_other_results():
    e = crdt_amd.Engine(4, 32)
    docs4 = list(range(4))
    assert (e.apply_remote_wire(docs4, [concurrent_wire(s)[0] for s in range(4)]) == 0).all()
    ver = e.versions()
    streams = [mixed_content(int(v) + 64, 60 + i) for i, v in enumerate(ver)]
    e.set_content(docs4, docs4, streams)
    docs = [3, 1, 0]
    since = [int(ver[d]) // 2 for d in docs]
    new_lens = e.lens(docs).astype(np.int64).tolist()

    def same(a, b):
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if a is None or isinstance(a, bytes):
            return a == b
        return np.array_equal(a, b)

    def sources():
        return [e.diff_read(i) for i in range(3)], [e.edits_read(i) for i in range(3)]

    e.diff_async(docs, since)
    e.edits_async(docs, since, "utf16")
    before = sources()
    mem = e.mem_bytes()
    e.rebase_async("diff")
    assert e.mem_bytes() > mem  # the buffers are counted
    assert same(before, sources())  # the sources read back unchanged
    e.rebase_async("edits")
    assert same(before, sources())
    ct = [ref_rebase_table(ref_diff(e.export(d), s)[0]) for d, s in zip(docs, since)]
    ut = [ref_rebase_table(ref_edits(e.export(d), s, streams[d], UTF16)[0], units=True) for d, s in zip(docs, since)]
    check_tables(e, ct, "chars")
    check_tables(e, ut, "units")
    old_lens = [int(t[-1, 0] + t[-1, 1]) + 4 for t in ct]
    old_units = [int(t[-1, 0] + t[-1, 1]) + 4 for t in ut]
    new_units = [int(t[-1, 2] + t[-1, 3]) + 4 for t in ut]
    # the map is a copy: other diffs, edits and encodes, more txns and a publish leave it as it was
    e.diff_async([0, 2], [1, 2])
    e.edits_async([1], [0], "utf8")
    ag = e.agent_intern(docs4, ["later"] * 4)
    assert (e.apply_local([(d, [(int(ag[d]), [(0, 0, 5)]), (int(ag[d]), [(2, 4, 0)])]) for d in docs4]) == 0).all()
    e.publish_async()
    e.encode(docs4, "utf8")
    e.diff_async(docs4, [0] * 4)
    check_tables(e, ct, "chars")
    check_tables(e, ut, "units")
    check_queries(e, [0, 1, 2], ct, old_lens, new_lens)
    check_queries(e, [0, 1, 2], ut, old_units, new_units, "units")
    # the next map replaces it
    e.rebase_async("diff")
    assert len(e.rebase_counts()) == 4
    with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
        e.rebase_read(0, "units")
    # crdt_docs_alloc drops the map
    assert e.L.crdt_docs_alloc(e.h, 2) == 0
    e.n_docs = 2
    one = np.zeros(1, np.uint32)
    for call in (e.rebase_counts, lambda: e.rebase_read(0), lambda: e.rebase(one, one), lambda: e.rebase_async("diff")):
        with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
            call()
    assert e.L.crdt_rebase_dev_async(e.h, 1, None, None, 0, 0, 0, None, None) == -100


def test_allocation_failure_leaves_the_engine_usable():
    wire, _ = concurrent_wire(2)
    L = crdt_amd.lib()
    failed = 0
    for k in range(8):  # the first rebase call of an engine allocates every buffer it needs: fail each in turn
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        c = mixed_content(int(e.versions([0])[0]), 51)
        e.set_content([0, 1], [0, 0], [c])
        dg = e.digests()
        src = e.edits([0, 1], [9, 0], "utf16")
        L.crdt_test_fail_alloc_after(k)
        try:
            e.rebase_async("edits")
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
        # the engine is not poisoned, has no map, keeps the source, and the same call then succeeds
        with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
            e.rebase_counts()
        with pytest.raises(crdt_amd.CrdtError, match=E_ARG):
            e.rebase(np.zeros(1, np.uint32), np.zeros(1, np.uint32))
        assert np.array_equal(e.digests(), dg)
        for i in range(2):
            got = e.edits_read(i)
            assert np.array_equal(got[0], src[i][0]) and np.array_equal(got[1], src[i][1])
        e.rebase_async("edits")
        check_tables(e, [ref_rebase_table(src[0][0]), ref_rebase_table(src[1][0])], "chars")
        ut = [ref_rebase_table(src[0][0], units=True), ref_rebase_table(src[1][0], units=True)]
        check_tables(e, ut, "units")
        xs = np.arange(40, dtype=np.uint32)
        y, hit = e.rebase(np.zeros(40, np.uint32), xs, "units", "old_to_new", "left")
        wy, wh = ref_rebase_many(ut[0], xs, OLD_TO_NEW, LEFT)
        assert np.array_equal(y, wy) and np.array_equal(hit, wh)
        e.close()
    assert failed == 4, failed  # (the per-index results, the job's totals and the two tables)


def test_device_pointer_form_equals_the_host_form():
    e = crdt_amd.Engine(3, 32)
    assert (e.apply_remote_wire([0, 1, 2], [concurrent_wire(s)[0] for s in (4, 5, 6)]) == 0).all()
    ver = e.versions()
    streams = [mixed_content(int(v), 80 + i) for i, v in enumerate(ver)]
    e.set_content([0, 1, 2], [0, 1, 2], streams)
    since = [int(v) // 3 for v in ver]
    e.edits_async([0, 1, 2], since, "utf8")
    e.rebase_async("edits")
    assert e.rebase_counts().sum() > 6
    rng = np.random.default_rng(9)
    nq = 3000  # (more than one block, not a multiple of 256)
    qi = rng.integers(0, 3, nq).astype(np.uint32)
    qx = rng.integers(0, 400, nq).astype(np.uint32)
    qx[:4] = [0, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000]
    for kind in (0, 1):
        for _, d in DIRS:
            for _, b in BIASES:
                wy, wh = e.rebase(qi, qx, kind, d, b)
                y, hit = dev_rebase(e, qi, qx, kind, d, b)
                assert np.array_equal(y, wy) and np.array_equal(hit, wh), (kind, d, b)
                y, hit = dev_rebase(e, qi, qx, kind, d, b, with_hit=False)
                assert np.array_equal(y, wy) and hit is None
    assert wh.any() and not wh.all()


def test_the_one_document_wrapper():
    doc = crdt_amd.ListCRDT()
    a = doc.get_or_create_agent_id("seph")
    assert doc.local_insert(a, 0, 8) == 0          # a b c d e f g h
    v = doc.version()
    assert doc.apply_local_txn(a, [(1, 2, 2)]) == 0  # bc -> XY
    assert doc.local_insert(a, 5, 1) == 0          # Z before f
    assert doc.local_delete(a, 7, 2) == 0          # g h
    y, hit = doc.rebase_since(v, np.arange(10))
    assert y.tolist() == [0, 1, 3, 3, 4, 6, 7, 7, 7, 8] and hit.tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 0, 0]
    y, hit = doc.rebase_since(v, np.arange(10), bias="left")
    assert y.tolist() == [0, 1, 1, 3, 4, 5, 7, 7, 7, 8]
    x, hit = doc.rebase_since(v, [0, 1, 2, 3, 5, 6, 7, 8], dir="new_to_old")
    assert x.tolist() == [0, 1, 3, 3, 5, 5, 8, 9] and hit.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
