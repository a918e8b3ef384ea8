"""GPU checks of the encoded text and its unit offsets (crdt_encode_async: k_enc_count, k_result_scan<EncRes>,
k_enc_write; k_pos_to_units, k_units_to_pos) through the C ABI.  Every result must equal
tests/encode_ref.py's ref_encode of the engine's own crdt_text exactly.

The encode kernels take 1,024 chars of a document per loop pass (csrc/encode.h ENC_PASS), 256 per
wave as four rows of 64, and keep one sample per 64 chars (ENC_S); documents are packed in the unit
pool, so most start and end inside a dword.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (before the first engine: torch finds no GPU once another HIP runtime is up)

import crdt_amd  # noqa: E402
from crdt_amd.traces import content_by_order, fnv1a64, load_trace  # noqa: E402
from encode_ref import (BOUNDARY, INVALID, NOT_SCALAR, UTF8, UTF16, cycle_text, ref_encode,  # noqa: E402
                        ref_units_to_pos_all)
from fuzz_gen import concurrent_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402

ENCS = (("utf8", UTF8), ("utf16", UTF16))
# the row (64), a wave's chars (256), the pass (1,024) and every allowed sample distance, each from both sides
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1025, 2049]
LENGTHS += [1024, 1345]  # (a whole pass; a second pass that ends one char into a wave's second row)


def pattern(kind: int, n: int, rng) -> np.ndarray:
    if kind == 0:
        return np.array([0x20 + j % 95 for j in range(n)], np.uint32)      # ASCII
    if kind == 1:
        return np.full(n, 0x1F600, np.uint32)                              # the largest expansion
    if kind == 2:
        return cycle_text(n)                                               # widths 1, 4, 2, 3
    return rng.choice(np.array(BOUNDARY + NOT_SCALAR, dtype=np.uint32), n)  # every boundary, the invalid values too


def as_array(units, enc):
    return np.frombuffer(units, np.uint8) if enc == UTF8 else units


def same_as_ref(e, d, enc, got, chars=None):
    """got (bytes / u16 array) against the reference of the engine's own text; returns the char starts"""
    want, start = ref_encode(e.text(d), enc)
    got = as_array(got, enc)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (d, enc, got[:12], want[:12])
    if chars is not None:
        assert int(chars) == len(start) - 1
    return start


def all_queries(starts):
    """every u in [0, units + 2] and every pos in [0, chars + 2] of every index, with the
    reference's answers: (idx_u, u, want_pos, want_mid), (idx_p, pos, want_units)"""
    iu, uu, wp, wm, ip, pp, wu = [], [], [], [], [], [], []
    for i, st in enumerate(starts):
        chars, units = len(st) - 1, int(st[-1])
        p, m = ref_units_to_pos_all(st)
        iu.append(np.full(units + 3, i, np.uint32))
        uu.append(np.arange(units + 3, dtype=np.uint32))
        wp.append(p)
        wm.append(m)
        ip.append(np.full(chars + 3, i, np.uint32))
        pp.append(np.arange(chars + 3, dtype=np.uint32))
        wu.append(np.concatenate([st, [INVALID, INVALID]]).astype(np.uint32))
    cat = np.concatenate
    return (cat(iu), cat(uu), cat(wp), cat(wm)), (cat(ip), cat(pp), cat(wu))


def check_queries(e, starts, device_form=True, seed=3):
    (iu, uu, wp, wm), (ip, pp, wu) = all_queries(starts)
    # several documents mixed in one batch
    rng = np.random.default_rng(seed)
    o1, o2 = rng.permutation(len(iu)), rng.permutation(len(ip))
    iu, uu, wp, wm = iu[o1], uu[o1], wp[o1], wm[o1]
    ip, pp, wu = ip[o2], pp[o2], wu[o2]
    gp, gm = e.units_to_pos(iu, uu)
    assert np.array_equal(gp, wp) and np.array_equal(gm, wm)
    assert np.array_equal(e.pos_to_units(ip, pp), wu)
    # the round trip on the engine's own answers
    ok = gp != INVALID
    back = e.pos_to_units(iu[ok], gp[ok])
    assert (back <= uu[ok]).all() and np.array_equal(back == uu[ok], gm[ok] == 0)
    if not device_form:
        return
    with torch.cuda.stream(torch.cuda.ExternalStream(e.stream(), device=torch.cuda.current_device())):
        t = [torch.from_numpy(x.astype(np.int32)).to("cuda", non_blocking=False) for x in (iu, uu, ip, pp)]
        d_pos = torch.full((len(iu),), 7, dtype=torch.int32, device="cuda")
        d_mid = torch.full((len(iu),), 7, dtype=torch.uint8, device="cuda")
        d_unit = torch.full((len(ip),), 7, dtype=torch.int32, device="cuda")
        assert e.L.crdt_units_to_pos_dev_async(e.h, len(iu), t[0].data_ptr(), t[1].data_ptr(), d_pos.data_ptr(), d_mid.data_ptr()) == 0
        assert e.L.crdt_pos_to_units_dev_async(e.h, len(ip), t[2].data_ptr(), t[3].data_ptr(), d_unit.data_ptr()) == 0
        e.sync()
        assert np.array_equal(d_pos.cpu().numpy().view(np.uint32), wp)
        assert np.array_equal(d_mid.cpu().numpy(), wm)
        assert np.array_equal(d_unit.cpu().numpy().view(np.uint32), wu)


@pytest.mark.parametrize("leaf", [32, 4])
def test_lengths_patterns_and_exhaustive_queries(leaf):
    rng = np.random.default_rng(21)
    # (2049, 0, 1025, ...: the empty document sits between two full ones, in every pattern)
    order = [2049, 0, 1025] + [n for n in LENGTHS if n not in (2049, 0, 1025)]
    shapes = [(kind, n) for kind in range(4) for n in order]
    nd = len(shapes)
    e = crdt_amd.Engine(nd, leaf)
    docs = list(range(nd))
    ag = e.agent_intern(docs, ["xa"] * nd)
    assert (e.apply_local([(d, [(int(ag[d]), [(0, 0, n)])]) for d, (_, n) in enumerate(shapes) if n]) == 0).all()
    texts = [pattern(kind, n, rng) for kind, n in shapes]
    e.set_content(docs, docs, texts)
    for name, enc in ENCS:
        res = e.encode(docs, name)
        units, chars = e.encode_lens()
        starts = []
        for d in docs:
            assert np.array_equal(e.text(d), texts[d])
            starts.append(same_as_ref(e, d, enc, res[d], chars[d]))
            assert int(units[d]) == int(starts[d][-1]) and int(chars[d]) == shapes[d][1]
        assert len(res[1]) == 0 and len(res[0]) > 0 and len(res[2]) > 0
        if enc == UTF8:  # the expansions of the four patterns, at 2049 chars
            assert [int(units[k * len(order)]) for k in range(3)] == [2049, 4 * 2049, 2049 // 4 * 10 + 1]
        check_queries(e, starts)
        assert e.encode_ms() > 0


def test_edited_text_concurrent_history_and_trace():
    rng = np.random.default_rng(22)
    wires = [concurrent_wire(s, n_agents=3, rounds=5)[0] for s in range(4)]
    t = load_trace("sveltecomponent")
    n = len(wires)
    e = crdt_amd.Engine(n + 1, 32)
    assert (e.apply_remote_wire(list(range(n)), wires) == 0).all()
    ag = int(e.agent_intern([n], ["jeremy"])[0])
    assert e.apply_trace([n], ag, t.counts, t.patches)[0] == 0
    streams = []
    for d in range(n):
        o = OracleDoc()
        o.apply_remote_wire(wires[d])
        c = rng.integers(0, 0x120000, o.sizes()["next_order"], dtype=np.uint32)
        c[::7] = rng.choice(np.array(BOUNDARY + NOT_SCALAR, dtype=np.uint32), len(c[::7]))
        streams.append(c)
        ot, _ = o.text(c)
        assert len(ot) > 8 and not np.array_equal(ot, c[:len(ot)])  # text order differs from content order
    streams.append(content_by_order(t))
    docs = list(range(n + 1))
    e.set_content(docs, docs, streams)
    for name, enc in ENCS:
        res = e.encode(docs, name)
        units, chars = e.encode_lens()
        starts = [same_as_ref(e, d, enc, res[d], chars[d]) for d in docs]
        if enc == UTF8:
            assert int(units[n]) == t.end_bytes and int(chars[n]) == t.end_len
            assert fnv1a64(res[n]) == t.end_fnv  # the reference's endContent
        else:
            assert int(units[n]) == t.end_len
        check_queries(e, starts[:n], device_form=False)
        # the trace's document: a sample of its offsets (it is ASCII: unit u is char u)
        q = rng.integers(0, t.end_len + 3, 4096).astype(np.uint32)
        idx = np.full(len(q), n, np.uint32)
        want = np.where(q <= t.end_len, q, INVALID).astype(np.uint32)
        gp, gm = e.units_to_pos(idx, q)
        assert np.array_equal(gp, want) and not gm.any()
        assert np.array_equal(e.pos_to_units(idx, q), want)


def test_result_lifetime_and_the_other_results():
    rng = np.random.default_rng(23)
    e = crdt_amd.Engine(6, 32)
    wires = [concurrent_wire(s)[0] for s in range(6)]
    assert (e.apply_remote_wire(list(range(6)), wires) == 0).all()
    docs6 = list(range(6))
    streams = [rng.choice(np.array(BOUNDARY, dtype=np.uint32), int(v) + 16) for v in e.versions()]  # (room for the late edits)
    e.set_content(docs6, docs6, streams)
    # diff, checkout and blame results made before the encode
    v = e.versions([2, 4])
    diff0 = e.diff([2, 4], v // 2)
    co0 = e.checkout([4, 2], v[::-1] // 3)
    bl0 = e.blame([2, 4], "id")
    dg = e.digests()
    docs = [5, 0, 3]  # a listed subset, not ascending
    first = e.encode(docs, "utf8")
    starts = [same_as_ref(e, d, UTF8, first[i]) for i, d in enumerate(docs)]
    assert len(e.encode_lens()[0]) == 3
    check_queries(e, starts, device_form=False)
    assert np.array_equal(e.digests(), dg)  # an encode changes no document
    for i in range(2):  # ... and none of the other results
        for a, b in zip(diff0[i], e.diff_read(i)):
            assert np.array_equal(a, b)
        for a, b in zip(co0[i], e.checkout_read(i)):
            assert np.array_equal(a, b)
        assert np.array_equal(bl0[i], e.blame_read(i))
    # more edits and a new materialise: the old result and its queries still give the old answers
    old_text0 = e.text(0)
    ag = e.agent_intern([0, 1], ["late"] * 2)
    assert (e.apply_local([(0, [(int(ag[0]), [(0, 0, 4)])]), (1, [(int(ag[1]), [(1, 2, 0)])])]) == 0).all()
    e.materialize_async()
    e.sync()
    new_text0 = e.text(0)
    assert len(new_text0) == len(old_text0) + 4
    for i in range(3):
        assert e.encode_read(i) == first[i]
    check_queries(e, starts, device_form=False, seed=4)
    # a second encode replaces the first, and gives the new text
    second = e.encode([1, 0], "utf16")
    units, chars = e.encode_lens()
    assert len(units) == 2 and int(chars[1]) == len(new_text0)
    starts2 = [same_as_ref(e, 1, UTF16, second[0]), same_as_ref(e, 0, UTF16, second[1])]
    assert np.array_equal(as_array(second[1], UTF16), ref_encode(new_text0, UTF16)[0])
    check_queries(e, starts2, device_form=False)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.encode_read(2)
    # the buffers are counted, and an empty list is a valid (empty) result
    before = e.mem_bytes()
    e.encode(docs6, "utf8")
    assert e.mem_bytes() > before
    assert e.encode([], "utf8") == []
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.pos_to_units([0], [0])


def test_no_result_and_argument_errors():
    wire, _ = concurrent_wire(1)
    e = crdt_amd.Engine(6, 32)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.encode_read(0)  # before any encode
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.pos_to_units([0], [0])
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.units_to_pos([0], [0])
    assert e.L.crdt_pos_to_units_dev_async(e.h, 1, None, None, None) == -100
    assert e.L.crdt_units_to_pos_dev_async(e.h, 1, None, None, None, None) == -100
    assert (e.apply_remote_wire([0, 2, 3, 5], [wire] * 4) == 0).all()
    ag = int(e.agent_intern([1], ["p"])[0])
    bad = [[(0, 0, 5)], [(2, 1, 0)], [(3, 5, 0)], [(0, 0, 1)]]      # the third txn deletes past the end
    assert e.apply_local([(1, [(ag, o) for o in bad])])[0] == -1
    nv = int(e.versions([0])[0])
    c = np.random.default_rng(24).choice(np.array(BOUNDARY + NOT_SCALAR, dtype=np.uint32), nv)
    # 0, 2, 5 healthy; 1 poisoned (with content); 3 one entry short; 4 (empty) without content
    e.set_content([0, 1, 2, 3, 5], [0, 0, 0, 1, 0], [c, c[:-1]])
    docs = list(range(6))
    none = [False, True, False, True, True, False]
    for name, enc in ENCS:
        res = e.encode(docs, name, strict=False)
        units, chars = e.encode_lens()
        assert [int(x) == INVALID for x in units] == none and [int(x) == INVALID for x in chars] == none
        starts = {}
        for i in docs:
            if none[i]:
                assert res[i] is None
                with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                    e.encode_read(i)
                for call in (e.pos_to_units, e.units_to_pos):
                    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                        call([0, i], [0, 0])  # a host query that names it
            else:  # the neighbours' results are intact
                starts[i] = same_as_ref(e, i, enc, res[i], chars[i])
                same_as_ref(e, i, enc, e.encode_read(i))
        keep = [i for i in docs if not none[i]]  # the healthy ones' queries, all in one batch
        (iu, uu, wp, wm), (ip, pp, wu) = all_queries([starts[i] for i in keep])
        remap = np.array(keep, np.uint32)
        gp, gm = e.units_to_pos(remap[iu], uu)
        assert np.array_equal(gp, wp) and np.array_equal(gm, wm)
        assert np.array_equal(e.pos_to_units(remap[ip], pp), wu)
        # the device form answers an idx out of range or without a result 0xFFFFFFFF, mid 0
        with torch.cuda.stream(torch.cuda.ExternalStream(e.stream(), device=torch.cuda.current_device())):
            idx = torch.tensor([0, 1, 3, 4, 6, 0x7FFFFFFF, 0], dtype=torch.int32, device="cuda")
            val = torch.tensor([1, 0, 0, 0, 0, 0, 1], dtype=torch.int32, device="cuda")
            o_p = torch.full((7,), 7, dtype=torch.int32, device="cuda")
            o_m = torch.full((7,), 7, dtype=torch.uint8, device="cuda")
            o_u = torch.full((7,), 7, dtype=torch.int32, device="cuda")
            assert e.L.crdt_units_to_pos_dev_async(e.h, 7, idx.data_ptr(), val.data_ptr(), o_p.data_ptr(), o_m.data_ptr()) == 0
            assert e.L.crdt_pos_to_units_dev_async(e.h, 7, idx.data_ptr(), val.data_ptr(), o_u.data_ptr()) == 0
            e.sync()
            got_p, got_m, got_u = o_p.cpu().numpy().view(np.uint32), o_m.cpu().numpy(), o_u.cpu().numpy().view(np.uint32)
        w_p, w_m = ref_units_to_pos_all(starts[0])
        assert got_p.tolist() == [int(w_p[1])] + [INVALID] * 5 + [int(w_p[1])]
        assert got_m.tolist() == [int(w_m[1])] + [0] * 5 + [int(w_m[1])]
        assert got_u.tolist() == [int(starts[0][1])] + [INVALID] * 5 + [int(starts[0][1])]
        # mid may be NULL
        i1 = np.zeros(3, np.uint32)
        u1 = np.arange(3, dtype=np.uint32)
        p1 = np.zeros(3, np.uint32)
        P = crdt_amd.C.POINTER
        assert e.L.crdt_units_to_pos(e.h, 3, i1.ctypes.data_as(P(crdt_amd.C.c_uint32)), u1.ctypes.data_as(P(crdt_amd.C.c_uint32)),
                                     p1.ctypes.data_as(P(crdt_amd.C.c_uint32)), None) == 0
        assert np.array_equal(p1, w_p[:3])
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.encode(docs, "utf8")  # strict
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.encode_read(6)  # out of range
    for call in (e.pos_to_units, e.units_to_pos):
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            call([0, 6], [0, 0])  # idx out of range
    out = np.full(4, 9, np.uint32)
    P32 = crdt_amd.C.POINTER(crdt_amd.C.c_uint32)
    i2, z2 = np.array([0, 1], np.uint32), np.zeros(2, np.uint32)
    assert e.L.crdt_pos_to_units(e.h, 2, i2.ctypes.data_as(P32), z2.ctypes.data_as(P32), out.ctypes.data_as(P32)) == -100
    assert (out == 9).all()  # ... and nothing was written
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.encode([0, 0], "utf8")  # a document named twice
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.encode([0, 7], "utf8")  # no such document
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.encode_async([0], 2)  # no such encoding
    # the engine still answers
    same_as_ref(e, 5, UTF8, e.encode([5], "utf8")[0])


def test_allocation_failure_leaves_the_engine_usable():
    wire, _ = concurrent_wire(2)
    L = crdt_amd.lib()
    failed = 0
    for k in range(16):  # the first encode of an engine allocates every buffer it needs: fail each in turn
        before = crdt_amd.Engine.device_bytes()[0]
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        c = cycle_text(int(e.versions([0])[0]))
        e.set_content([0, 1], [0, 0], [c])
        dg = e.digests()
        L.crdt_test_fail_alloc_after(k)
        try:
            e.encode([0, 1], "utf8")
            ok = True
        except crdt_amd.CrdtError as x:
            assert "rc=-102" in str(x), x
            ok = False
        finally:
            L.crdt_test_fail_alloc_after(-1)
        if not ok:
            failed += 1
            # no relayout was involved: the engine is not poisoned and the same encode then succeeds
            with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                e.encode_read(0)  # without an encode result
            with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                e.pos_to_units([0], [0])
            assert np.array_equal(e.digests(), dg)
            res = e.encode([0, 1], "utf8")
            starts = [same_as_ref(e, d, UTF8, res[d]) for d in (0, 1)]
            check_queries(e, starts, device_form=False)
        e.close()
        now = crdt_amd.Engine.device_bytes()[0]
        assert now <= before, (k, now, before)  # nothing of a closed engine stays allocated
        if ok:
            break
    assert 6 <= failed < 16, failed  # (the encode's own six buffers at least; before them the index's and the text's)


def test_the_one_document_wrapper():
    doc = crdt_amd.ListCRDT()
    a = doc.get_or_create_agent_id("seph")
    assert doc.local_insert(a, 0, 5) == 0 and doc.local_delete(a, 1, 1) == 0
    doc.set_content(np.array([0x68, 0x65, 0xE9, 0x20AC, 0x1F600, 0], np.uint32))  # (order 5 is the delete)
    s = "hé€\U0001F600"
    assert doc.to_string() == s
    assert doc.to_bytes() == s.encode("utf-8")
    assert doc.len_utf16() == len(s.encode("utf-16-le")) // 2 == 5
    assert doc.e.encode([0], "utf16")[0].tobytes() == s.encode("utf-16-le")
    assert doc.e.units_to_pos([0] * 6, list(range(6)))[0].tolist() == [0, 1, 2, 3, 3, 4]
    assert doc.e.encode_ms() > 0
