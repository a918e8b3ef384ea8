"""GPU checks of the line index (crdt_lines_async: k_ln_count, k_result_scan<LnRes>, k_ln_write;
k_pos_to_linecol, k_linecol_to_pos) through the C ABI.  Every result must equal tests/lines_ref.py
applied to the engine's own crdt_text exactly.

The line sweeps take a document's aligned dwords of the packed unit pool 1,024 per loop pass
(csrc/lines.h LN_PASS), 256 per wave as four rows of 64.  In units that is LN_ROW_U / LN_WAVE_U /
LN_PASS_U below, per encoding; documents are packed, so most start and end inside a dword and the
seams fall at every phase.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (before the first engine: torch finds no GPU once another HIP runtime is up)

import crdt_amd  # noqa: E402
from crdt_amd.traces import content_by_order, load_trace  # noqa: E402
from encode_ref import UTF8, UTF16, cycle_text, ref_encode  # noqa: E402
from fuzz_gen import concurrent_wire  # noqa: E402
from lines_ref import (COL_CHARS, COL_UNITS, EOL_ANY, EOL_LF, INVALID, ref_breaks, ref_lines,  # noqa: E402
                       ref_linecol_to_pos_all, ref_pos_to_linecol_all)
from oracle_lib import OracleDoc  # noqa: E402

ENCS = {"utf8": UTF8, "utf16": UTF16}
EOLS = (("lf", EOL_LF), ("any", EOL_ANY))
KINDS = (("units", COL_UNITS), ("chars", COL_CHARS))
# units per row of 64 dwords, per wave (4 rows) and per loop pass (4 waves), UTF-8 / UTF-16
LN_ROW_U = {UTF8: 256, UTF16: 128}
LN_WAVE_U = {UTF8: 1024, UTF16: 512}
LN_PASS_U = {UTF8: 4096, UTF16: 2048}
# the encode test's list (its row, wave and pass in chars) ...
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1025, 2049, 1024, 1345]
# ... and one below, at and one above each of the sizes above, and one above two passes, in units
for _enc in (UTF8, UTF16):
    for _u in (LN_ROW_U[_enc], LN_WAVE_U[_enc], LN_PASS_U[_enc]):
        LENGTHS += [n for n in (_u - 1, _u, _u + 1) if n not in LENGTHS]
    LENGTHS += [n for n in (2 * LN_PASS_U[_enc] + 1,) if n not in LENGTHS]
# LF, CR, a char of every width, other conventions' breaks (none here), the four UTF-16 traps of a
# byte-wise compare, and a value that encodes as U+FFFD
ALPHABET = [0x0A, 0x0D, 0x61, 0xE9, 0x20AC, 0x1F600, 0x0B, 0x0C, 0x85, 0x2028, 0x010A, 0x0A0A, 0x0A0D, 0x0D0A, 0xD800]
N_PATTERNS = 9


def pattern(kind: int, n: int, rng) -> np.ndarray:
    if kind == 0:
        return np.array([0x20 + j % 95 for j in range(n)], np.uint32)      # no break at all
    if kind == 1:
        return np.full(n, 0x0A, np.uint32)                                 # all LF
    if kind == 2:
        return np.full(n, 0x0D, np.uint32)                                 # all CR
    if kind < 7:  # "\r\n" repeated after 0..3 'a': the pair straddles every dword, row, wave and pass seam in turn
        lead = kind - 3
        body = np.tile(np.array([0x0D, 0x0A], np.uint32), n // 2 + 1)
        return np.concatenate([np.full(lead, 0x61, np.uint32), body])[:n]
    if kind == 7:  # the width cycle, with LF in place of its ASCII char
        t = cycle_text(n)
        t[t == 0x41] = 0x0A
        return t
    return rng.choice(np.array(ALPHABET, dtype=np.uint32), n)


def neighbours():
    """packed neighbours: a last CR directly before a first LF, the same around an empty document,
    and a document that ends in LF"""
    s = ["ab\r", "\nab", "ab\r", "", "\nab", "ab\n", "\n"]
    return [np.array([ord(c) for c in x], np.uint32) for x in s]


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(41)
    # (8193, 0, 4097, ...: the empty document sits between two full ones, in every pattern)
    order = [8193, 0, 4097] + [n for n in LENGTHS if n not in (8193, 0, 4097)]
    shapes = [(kind, n) for kind in range(N_PATTERNS) for n in order]
    return shapes, [pattern(kind, n, rng) for kind, n in shapes] + neighbours()


def reference(text, enc):
    """(start, {eol: line starts}) of one text"""
    _, start = ref_encode(text, enc)
    return start, {eol: ref_lines(text, start, eol) for _, eol in EOLS}


def all_queries(idxs, starts, lines):
    """every pos in [0, chars + 2], and every (line, col) with line in [0, n_lines + 1] and col in
    [0, extent + 2], of every listed index, per column kind, with the reference's answers:
    {kind: (idx, pos, want_line, want_col, idx, line, col, want_pos, want_mid)}"""
    out = {}
    for _, kind in KINDS:
        cols = [[] for _ in range(9)]
        for i, st, ln in zip(idxs, starts, lines):
            wl, wc = ref_pos_to_linecol_all(ln, st, kind)
            ql, qc, qp, qm = ref_linecol_to_pos_all(ln, st, kind)
            for k, x in enumerate((np.full(len(wl), i, np.uint32), np.arange(len(wl), dtype=np.uint32), wl, wc,
                                   np.full(len(ql), i, np.uint32), ql, qc, qp, qm)):
                cols[k].append(x)
        out[kind] = tuple(np.concatenate(c) for c in cols)
    return out


@functools.lru_cache(maxsize=None)
def corpus_reference(encname):
    """the corpus' starts, line starts and queries, shared by the two leaf sizes (the texts are the
    same: every test checks crdt_text against them first)"""
    _, texts = corpus()
    refs = [reference(t, ENCS[encname]) for t in texts]
    starts = [r[0] for r in refs]
    idxs = list(range(len(texts)))
    return starts, {eol: ([r[1][eol] for r in refs], all_queries(idxs, starts, [r[1][eol] for r in refs])) for _, eol in EOLS}


def check_index(e, idxs, lines):
    """n_lines, crdt_lines_read and every line start of the listed indexes"""
    counts = e.line_counts()
    for i, ln in zip(idxs, lines):
        assert int(counts[i]) == len(ln), (i, int(counts[i]), len(ln))
        got = e.lines_read(i, counts)
        assert got.dtype == np.uint32 and got.shape == ln.shape and np.array_equal(got, ln), (i, got[:6], ln[:6])
    return counts


def check_queries(e, queries, device_form=True, seed=5):
    rng = np.random.default_rng(seed)
    for kindname, kind in KINDS:
        ip, pp, wl, wc, il, ll, cc, wp, wm = queries[kind]
        # several documents mixed in one batch
        o1, o2 = rng.permutation(len(ip)), rng.permutation(len(il))
        ip, pp, wl, wc = ip[o1], pp[o1], wl[o1], wc[o1]
        il, ll, cc, wp, wm = il[o2], ll[o2], cc[o2], wp[o2], wm[o2]
        gl, gc = e.pos_to_linecol(ip, pp, kindname)
        assert np.array_equal(gl, wl) and np.array_equal(gc, wc), kindname
        gp, gm = e.linecol_to_pos(il, ll, cc, kindname)
        assert np.array_equal(gp, wp) and np.array_equal(gm, wm), kindname
        # the round trip on the engine's own answers
        ok = gl != INVALID
        bp, bm = e.linecol_to_pos(ip[ok], gl[ok], gc[ok], kindname)
        assert np.array_equal(bp, pp[ok]) and not bm.any()
        if not device_form:
            continue
        with torch.cuda.stream(torch.cuda.ExternalStream(e.stream(), device=torch.cuda.current_device())):
            t = [torch.from_numpy(x.astype(np.int32)).to("cuda", non_blocking=False) for x in (ip, pp, il, ll, cc)]
            d_line = torch.full((len(ip),), 7, dtype=torch.int32, device="cuda")
            d_col = torch.full((len(ip),), 7, dtype=torch.int32, device="cuda")
            d_pos = torch.full((len(il),), 7, dtype=torch.int32, device="cuda")
            d_mid = torch.full((len(il),), 7, dtype=torch.uint8, device="cuda")
            assert e.L.crdt_pos_to_linecol_dev_async(e.h, len(ip), t[0].data_ptr(), t[1].data_ptr(), kind, d_line.data_ptr(),
                                                     d_col.data_ptr()) == 0
            assert e.L.crdt_linecol_to_pos_dev_async(e.h, len(il), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), kind,
                                                     d_pos.data_ptr(), d_mid.data_ptr()) == 0
            e.sync()
            assert np.array_equal(d_line.cpu().numpy().view(np.uint32), wl)
            assert np.array_equal(d_col.cpu().numpy().view(np.uint32), wc)
            assert np.array_equal(d_pos.cpu().numpy().view(np.uint32), wp)
            assert np.array_equal(d_mid.cpu().numpy(), wm)


def check_all(e, docs, enc, eol, device_form=False, seed=5):
    """the line index of the last encode (of `docs`, in `enc`) against the reference of the engine's own text"""
    refs = [reference(e.text(d), enc) for d in docs]
    idxs = list(range(len(docs)))
    starts, lines = [r[0] for r in refs], [r[1][eol] for r in refs]
    check_index(e, idxs, lines)
    check_queries(e, all_queries(idxs, starts, lines), device_form, seed)
    return starts, lines


@pytest.mark.parametrize("encname", ["utf8", "utf16"])
@pytest.mark.parametrize("leaf", [32, 4])
def test_lengths_patterns_and_exhaustive_queries(leaf, encname):
    shapes, texts = corpus()
    nd = len(texts)
    e = crdt_amd.Engine(nd, leaf)
    docs = list(range(nd))
    ag = e.agent_intern(docs, ["xa"] * nd)
    assert (e.apply_local([(d, [(int(ag[d]), [(0, 0, len(t))])]) for d, t in enumerate(texts) if len(t)]) == 0).all()
    e.set_content(docs, docs, texts)
    starts, per_eol = corpus_reference(encname)
    e.encode_async(docs, encname)
    units, chars = e.encode_lens()
    for d in docs:
        assert np.array_equal(e.text(d), texts[d])
        assert int(units[d]) == int(starts[d][-1]) and int(chars[d]) == len(texts[d])
    for eolname, eol in EOLS:
        e.lines_async(eolname)
        lines, queries = per_eol[eol]
        counts = check_index(e, docs, lines)
        base = len(shapes)  # the packed neighbours
        assert [int(counts[base + k]) for k in range(7)] == ([1, 2, 1, 1, 2, 2, 2] if eol == EOL_LF else [2, 2, 2, 1, 2, 2, 2])
        assert lines[base + 1][1].tolist() == [1, 1] and lines[base + 4][1].tolist() == [1, 1]
        if eol == EOL_ANY:  # the CR is a break of its own document; the neighbour's line 0 starts at {0, 0}
            assert lines[base][1].tolist() == [3, 3] and lines[base + 2][1].tolist() == [3, 3]
        check_queries(e, queries)
        assert e.lines_ms() > 0


def test_edited_text_concurrent_history_and_trace():
    rng = np.random.default_rng(42)
    wires = [concurrent_wire(s, n_agents=3, rounds=5)[0] for s in range(3)]
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
        streams.append(rng.choice(np.array(ALPHABET, dtype=np.uint32), o.sizes()["next_order"]))
    streams.append(content_by_order(t))
    docs = list(range(n + 1))
    e.set_content(docs, docs, streams)
    text = e.text(n)
    for encname, enc in ENCS.items():
        res = e.encode(docs, encname)
        for eolname, eol in EOLS:
            e.lines_async(eolname)
            check_all(e, docs[:n], enc, eol)  # (indexes 0..n-1 are documents 0..n-1)
            # the trace's document: its count, its starts, and a sample of its queries
            want = len(ref_breaks(text, eol)) + 1
            counts = e.line_counts()
            assert int(counts[n]) == want and want > 1
            got = e.lines_read(n, counts)
            if enc == UTF8:  # the byte offsets after each break in the encoded bytes
                b = np.frombuffer(res[n], np.uint8)
                brk = b == 10
                if eol == EOL_ANY:
                    brk |= (b == 13) & np.concatenate([b[1:] != 10, [True]])
                assert np.array_equal(got[1:, 0], np.flatnonzero(brk) + 1)
            start, lines = reference(text, enc)
            assert np.array_equal(got, lines[eol])
            q = rng.integers(0, len(text) + 3, 4096).astype(np.uint32)
            idx = np.full(len(q), n, np.uint32)
            for kindname, kind in KINDS:
                wl, wc = ref_pos_to_linecol_all(lines[eol], start, kind)
                gl, gc = e.pos_to_linecol(idx, q, kindname)
                assert np.array_equal(gl, wl[q]) and np.array_equal(gc, wc[q])
                ok = gl != INVALID
                bp, bm = e.linecol_to_pos(idx[ok], gl[ok], gc[ok], kindname)
                assert np.array_equal(bp, q[ok]) and not bm.any()


def test_result_lifetime_and_the_other_results():
    rng = np.random.default_rng(43)
    e = crdt_amd.Engine(6, 32)
    wires = [concurrent_wire(s)[0] for s in range(6)]
    assert (e.apply_remote_wire(list(range(6)), wires) == 0).all()
    docs6 = list(range(6))
    streams = [rng.choice(np.array(ALPHABET[:6], dtype=np.uint32), int(v) + 16) for v in e.versions()]  # (room for the late edits)
    e.set_content(docs6, docs6, streams)
    # diff, checkout, blame and encode results made before the line index
    v = e.versions([2, 4])
    diff0 = e.diff([2, 4], v // 2)
    co0 = e.checkout([4, 2], v[::-1] // 3)
    bl0 = e.blame([2, 4], "id")
    dg = e.digests()
    docs = [5, 0, 3]  # a listed subset, not ascending
    enc0 = e.encode(docs, "utf8")
    lens0 = e.encode_lens()
    before = e.mem_bytes()
    e.lines_async("lf")
    assert e.mem_bytes() > before  # the buffers are counted
    starts, lines_lf = check_all(e, docs, UTF8, EOL_LF)
    assert len(e.line_counts()) == 3
    assert np.array_equal(e.digests(), dg)  # a line index changes no document
    for i in range(2):  # ... and none of the other results
        for a, b in zip(diff0[i], e.diff_read(i)):
            assert np.array_equal(a, b)
        for a, b in zip(co0[i], e.checkout_read(i)):
            assert np.array_equal(a, b)
        assert np.array_equal(bl0[i], e.blame_read(i))
    for i in range(3):
        assert e.encode_read(i) == enc0[i]
    assert all(np.array_equal(a, b) for a, b in zip(lens0, e.encode_lens()))
    # a second line index with the other eol replaces the first
    e.lines_async("any")
    _, lines_any = check_all(e, docs, UTF8, EOL_ANY)
    assert any(len(a) != len(b) for a, b in zip(lines_lf, lines_any))
    queries = all_queries([0, 1, 2], starts, lines_any)
    # more edits and a new materialise: the index and its queries still give the old answers
    old_text0 = e.text(0)
    ag = e.agent_intern([0, 1], ["late"] * 2)
    assert (e.apply_local([(0, [(int(ag[0]), [(0, 0, 4)])]), (1, [(int(ag[1]), [(1, 2, 0)])])]) == 0).all()
    e.materialize_async()
    e.sync()
    assert len(e.text(0)) == len(old_text0) + 4
    check_index(e, [0, 1, 2], lines_any)
    check_queries(e, queries, device_form=False, seed=6)
    # a new encode drops it
    e.encode_async([1, 0], "utf16")
    one = np.zeros(1, np.uint32)
    for call in (e.line_counts, lambda: e.lines_read(0, np.ones(2, np.uint32)), lambda: e.pos_to_linecol(one, one),
                 lambda: e.linecol_to_pos(one, one, one), lambda: e.linecol_to_pos(one, one, one, "chars")):
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            call()
    assert e.L.crdt_pos_to_linecol_dev_async(e.h, 1, None, None, 0, None, None) == -100
    assert e.L.crdt_linecol_to_pos_dev_async(e.h, 1, None, None, None, 0, None, None) == -100
    # ... and the next line index is of the new encode, and of the new text
    e.lines_async("any")
    check_all(e, [1, 0], UTF16, EOL_ANY)
    assert len(e.line_counts()) == 2
    # a later encode call drops it, successful or not: one rejected for its arguments leaves the
    # encode result, on which the next line index is built
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.encode_async([0, 0], "utf8")
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.line_counts()
    assert len(e.encode_lens()[0]) == 2
    e.lines_async("lf")
    check_all(e, [1, 0], UTF16, EOL_LF)
    # an encode of [] gives an empty line index
    assert e.encode([], "utf8") == []
    assert e.lines("lf") == [] and len(e.line_counts()) == 0
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.pos_to_linecol(one, one)


def test_no_result_and_argument_errors():
    wire, _ = concurrent_wire(1)
    e = crdt_amd.Engine(6, 32)
    one = np.zeros(1, np.uint32)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.lines_async("lf")  # before any encode
    for call in (e.line_counts, lambda: e.lines_read(0, np.ones(1, np.uint32)), lambda: e.pos_to_linecol(one, one),
                 lambda: e.linecol_to_pos(one, one, one)):
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            call()
    assert (e.apply_remote_wire([0, 2, 3, 5], [wire] * 4) == 0).all()
    ag = int(e.agent_intern([1], ["p"])[0])
    bad = [[(0, 0, 5)], [(2, 1, 0)], [(3, 5, 0)], [(0, 0, 1)]]      # the third txn deletes past the end
    assert e.apply_local([(1, [(ag, o) for o in bad])])[0] == -1
    nv = int(e.versions([0])[0])
    c = np.random.default_rng(44).choice(np.array(ALPHABET, dtype=np.uint32), nv)
    # 0, 2, 5 healthy; 1 poisoned (with content); 3 one entry short; 4 (empty) without content
    e.set_content([0, 1, 2, 3, 5], [0, 0, 0, 1, 0], [c, c[:-1]])
    docs = list(range(6))
    none = [False, True, False, True, True, False]
    keep = [i for i in docs if not none[i]]
    P32, P8 = crdt_amd.C.POINTER(crdt_amd.C.c_uint32), crdt_amd.C.POINTER(crdt_amd.C.c_uint8)

    def p32(a):
        return a.ctypes.data_as(P32)

    for encname, enc in ENCS.items():
        e.encode(docs, encname, strict=False)
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.lines_async(2)  # an unknown eol
        for eolname, eol in EOLS:
            res = e.lines(eolname, strict=False)
            counts = e.line_counts()
            assert [int(x) == INVALID for x in counts] == none
            for i in docs:
                if not none[i]:
                    continue
                assert res[i] is None
                with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                    e.lines_read(i)
                with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                    e.pos_to_linecol([0, i], [0, 0])  # a host query that names it
                with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                    e.linecol_to_pos([0, i], [0, 0], [0, 0], "chars")
            with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                e.lines(eolname)  # strict
            # the healthy ones' answers are intact, all in one batch
            refs = [reference(e.text(i), enc) for i in keep]
            starts, lines = [r[0] for r in refs], [r[1][eol] for r in refs]
            check_index(e, keep, lines)
            check_queries(e, all_queries(keep, starts, lines), device_form=False)
            # the device form answers an idx out of range or without a result 0xFFFFFFFF, mid 0
            wl, wc = ref_pos_to_linecol_all(lines[0], starts[0], COL_UNITS)
            with torch.cuda.stream(torch.cuda.ExternalStream(e.stream(), device=torch.cuda.current_device())):
                idx = torch.tensor([0, 1, 3, 4, 6, 0x7FFFFFFF, 0], dtype=torch.int32, device="cuda")
                val = torch.tensor([1, 0, 0, 0, 0, 0, 1], dtype=torch.int32, device="cuda")
                zero = torch.zeros(7, dtype=torch.int32, device="cuda")
                o_l = torch.full((7,), 7, dtype=torch.int32, device="cuda")
                o_c = torch.full((7,), 7, dtype=torch.int32, device="cuda")
                o_p = torch.full((7,), 7, dtype=torch.int32, device="cuda")
                o_m = torch.full((7,), 7, dtype=torch.uint8, device="cuda")
                assert e.L.crdt_pos_to_linecol_dev_async(e.h, 7, idx.data_ptr(), val.data_ptr(), 0, o_l.data_ptr(), o_c.data_ptr()) == 0
                assert e.L.crdt_linecol_to_pos_dev_async(e.h, 7, idx.data_ptr(), zero.data_ptr(), zero.data_ptr(), 1, o_p.data_ptr(),
                                                         o_m.data_ptr()) == 0
                e.sync()
                got = [x.cpu().numpy() for x in (o_l, o_c, o_p, o_m)]
            assert got[0].view(np.uint32).tolist() == [int(wl[1])] + [INVALID] * 5 + [int(wl[1])]
            assert got[1].view(np.uint32).tolist() == [int(wc[1])] + [INVALID] * 5 + [int(wc[1])]
            assert got[2].view(np.uint32).tolist() == [0] + [INVALID] * 5 + [0]
            assert got[3].tolist() == [0] * 7
        # mid may be NULL
        i1, z1, c1, p1 = np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.arange(3, dtype=np.uint32), np.full(3, 9, np.uint32)
        assert e.L.crdt_linecol_to_pos(e.h, 3, p32(i1), p32(z1), p32(c1), 0, p32(p1), None) == 0
        want = ref_linecol_to_pos_all(lines[0], starts[0], COL_UNITS)
        assert p1.tolist() == want[2][:3].tolist() and want[0][:3].tolist() == [0, 0, 0]  # (line 0, cols 0..2)
    # host forms: an idx without a result or out of range, or an unknown col_kind: -100 and nothing written
    out, out2, m = np.full(2, 9, np.uint32), np.full(2, 9, np.uint32), np.full(2, 9, np.uint8)
    z2 = np.zeros(2, np.uint32)
    for i2, kind in ((np.array([0, 1], np.uint32), 0), (np.array([0, 6], np.uint32), 1), (z2, 2), (z2, -1)):
        assert e.L.crdt_pos_to_linecol(e.h, 2, p32(i2), p32(z2), kind, p32(out), p32(out2)) == -100
        assert e.L.crdt_linecol_to_pos(e.h, 2, p32(i2), p32(z2), p32(z2), kind, p32(out), m.ctypes.data_as(P8)) == -100
        assert (out == 9).all() and (out2 == 9).all() and (m == 9).all()
    assert e.L.crdt_pos_to_linecol_dev_async(e.h, 0, None, None, 2, None, None) == -100  # an unknown col_kind
    assert e.L.crdt_linecol_to_pos_dev_async(e.h, 0, None, None, None, 2, None, None) == -100
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.lines_read(6)  # out of range
    # the engine still answers
    e.encode([5], "utf8")
    e.lines_async("any")
    check_all(e, [5], UTF8, EOL_ANY)


def test_allocation_failure_leaves_the_engine_usable():
    wire, _ = concurrent_wire(2)
    L = crdt_amd.lib()
    failed = 0
    for k in range(8):  # the first line index of an engine allocates every buffer it needs: fail each in turn
        before = crdt_amd.Engine.device_bytes()[0]
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        c = cycle_text(int(e.versions([0])[0]))
        c[c == 0x41] = 0x0A
        e.set_content([0, 1], [0, 0], [c])
        enc0 = e.encode([0, 1], "utf8")
        dg = e.digests()
        L.crdt_test_fail_alloc_after(k)
        try:
            e.lines_async("lf")
            ok = True
        except crdt_amd.CrdtError as x:
            assert "rc=-102" in str(x), x
            ok = False
        finally:
            L.crdt_test_fail_alloc_after(-1)
        if not ok:
            failed += 1
            # the engine is not poisoned, has no line index, and its encode result is intact
            with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                e.line_counts()
            with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                e.pos_to_linecol([0], [0])
            assert np.array_equal(e.digests(), dg)
            assert [e.encode_read(i) for i in (0, 1)] == enc0
            e.lines_async("lf")  # ... and the same call then succeeds
        check_all(e, [0, 1], UTF8, EOL_LF)
        e.close()
        now = crdt_amd.Engine.device_bytes()[0]
        assert now <= before, (k, now, before)  # nothing of a closed engine stays allocated
        if ok:
            break
    assert 3 <= failed < 8, failed  # (the per-index counts, the total and the table)


def test_the_one_document_wrapper():
    doc = crdt_amd.ListCRDT()
    a = doc.get_or_create_agent_id("seph")
    s = "hé\r\n€\U0001F600\nx\r"
    assert doc.local_insert(a, 0, len(s)) == 0
    doc.set_content(np.array([ord(c) for c in s], np.uint32))
    assert doc.to_string() == s
    assert doc.line_count() == 3 and doc.line_count("any") == 4
    assert doc.pos_to_linecol(5) == (1, 1) and doc.pos_to_linecol(6) == (1, 3)       # UTF-16 units
    assert doc.pos_to_linecol(6, "utf8") == (1, 7) and doc.pos_to_linecol(6, col="chars") == (1, 2)
    assert doc.pos_to_linecol(len(s), eol="any") == (3, 0) and doc.pos_to_linecol(len(s)) == (2, 2)
    assert doc.linecol_to_pos(1, 3) == 6 and doc.linecol_to_pos(1, 2) == 5             # (col 2: inside the surrogate pair)
    assert doc.linecol_to_pos(3, 0, eol="any") == len(s) and doc.linecol_to_pos(3, 0) == INVALID
    assert doc.e.lines_ms() > 0
