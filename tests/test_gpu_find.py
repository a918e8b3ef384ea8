"""GPU checks of find (crdt_find_async: k_find_count, k_result_scan<FdRes>, k_find_write; k_find_seek)
through the C ABI.  Every result must equal tests/find_ref.py applied to the engine's own crdt_text
exactly.

The find sweeps take a document's aligned dwords of the packed unit pool 1,024 per loop pass
(csrc/find.h, as csrc/lines.h), 256 per wave as four rows of 64, and verify a candidate against an
LDS window that reaches 64 dwords past the pass.  Documents are packed, so most start and end inside
a dword and the seams fall at every phase; the repeated-pattern texts put a match across every one.
"""
import collections
import functools
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (before the first engine: torch finds no GPU once another HIP runtime is up)

import crdt_amd  # noqa: E402
from crdt_amd.traces import content_by_order, load_trace, utf32_to_str  # noqa: E402
from encode_ref import UTF8, UTF16, cycle_text, ref_encode  # noqa: E402
from find_ref import INVALID, SEEK_NEXT, SEEK_PREV, ref_find, ref_find_pos, ref_seek, sanitise  # noqa: E402
from fuzz_gen import concurrent_wire  # noqa: E402
from lines_ref import EOL_LF, ref_lines  # noqa: E402

ENCS = {"utf8": UTF8, "utf16": UTF16}
DIRS = (("next", SEEK_NEXT), ("prev", SEEK_PREV))
# the line test's lengths: the encode test's list, one below, at and one above the row, the wave and
# the pass in units of either encoding, and one above two passes
LN_ROW_U = {UTF8: 256, UTF16: 128}
LN_WAVE_U = {UTF8: 1024, UTF16: 512}
LN_PASS_U = {UTF8: 4096, UTF16: 2048}
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1025, 2049, 1024, 1345]
for _enc in (UTF8, UTF16):
    for _u in (LN_ROW_U[_enc], LN_WAVE_U[_enc], LN_PASS_U[_enc]):
        LENGTHS += [n for n in (_u - 1, _u, _u + 1) if n not in LENGTHS]
    LENGTHS += [n for n in (2 * LN_PASS_U[_enc] + 1,) if n not in LENGTHS]
# a char of every width, the case pairs, the UTF-16 traps of a byte-wise compare or fold (U+0141,
# U+4100, U+0A0A), the Kelvin sign, and a value that encodes as U+FFFD next to U+FFFD itself
ALPHABET = [0x61, 0x41, 0x62, 0xE9, 0xC9, 0x20AC, 0x1F600, 0x212A, 0x0141, 0x4100, 0x0A0A, 0xD800, 0xFFFD]
_rng0 = np.random.default_rng(60)
# 64 ASCII chars with no period, and 64 four-byte chars (two UTF-16 units each) with none: the
# longest pattern is 256 bytes / 128 u16, the full window
S64 = _rng0.choice(np.array([ord(c) for c in "abcdefgh"], np.uint32), 64)
Q64 = (0x1F600 + _rng0.permutation(64)).astype(np.uint32)
# the texts whose repetition the corpus holds
REPEATED = [S64[:9], S64, Q64]
# (pattern, icase): every length of the issue's list in ASCII, 5 and 64 in four-byte chars, the
# fold, and the explicit cases
PATTERNS = [(S64[:m], False) for m in (1, 2, 3, 4, 5, 7, 8, 9, 31, 63, 64)] + [(Q64[:5], False), (Q64, False)]
PATTERNS += [(np.full(m, 0x61, np.uint32), False) for m in (1, 2, 9, 64)]                 # all 'a'
PATTERNS += [(np.array([0x41 if j % 2 else 0x61 for j in range(m)], np.uint32), True) for m in (1, 3, 64)]  # aAa... folded
PATTERNS += [(np.array([0x61, 0x62], np.uint32), False), (np.array([0x42, 0x61, 0x42], np.uint32), True),
             (np.array([0x41, 0x1F600, 0xE9, 0x20AC, 0x41], np.uint32), False),           # the width cycle
             (np.array([0xD800], np.uint32), False), (np.array([0xFFFD], np.uint32), False),
             (np.array([0x41], np.uint32), True), (np.array([0x6B], np.uint32), True), (np.array([0xC9], np.uint32), True),
             (np.array([0x20AC, 0x1F600], np.uint32), False)]
N_KINDS = 4 + 8 * len(REPEATED)
# hand-made documents after the corpus: the explicit cases
EXTRA = [[0xFFFD], [0xD800], [0x0141], [0x4100], [0x212A], [0x41], [0x61], [0x4B], [0xC9], [0xE9]]


def content(kind: int, n: int, rng) -> np.ndarray:
    if kind == 0:
        return np.full(n, 0x61, np.uint32)                                  # all 'a'
    if kind == 1:
        return rng.choice(np.array([0x61, 0x62], np.uint32), n)              # random over {a, b}
    if kind == 2:
        return cycle_text(n)                                                # the width cycle
    if kind == 3:
        return rng.choice(np.array(ALPHABET, dtype=np.uint32), n)
    # a text repeated after 0..3 'x' (a match straddles every dword, row, wave and pass seam in turn);
    # in the second half of these kinds the text's last char is replaced at every second repetition
    # (near misses that fail only at the far end of the window)
    k = kind - 4
    rep, lead, miss = REPEATED[k // 8], k % 4, (k % 8) >= 4
    body = np.tile(rep, n // len(rep) + 1)
    if miss:
        body[2 * len(rep) - 1::2 * len(rep)] = 0x7A
    return np.concatenate([np.full(lead, 0x78, np.uint32), body])[:n]


def neighbours(a, c):
    """packed neighbours: pattern a + c must not be assembled from one document's end and the
    next one's start, nor across an empty document"""
    a, c = np.asarray(a, np.uint32), np.asarray(c, np.uint32)
    return [a, c, a, np.zeros(0, np.uint32), np.concatenate([c, a]), np.concatenate([a, c])]


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(61)
    # (8193, 0, 4097, ...: the empty document sits between two full ones, in every kind)
    order = [8193, 0, 4097] + [n for n in LENGTHS if n not in (8193, 0, 4097)]
    shapes = [(kind, n) for kind in range(N_KINDS) for n in order]
    texts = [content(kind, n, rng) for kind, n in shapes] + [np.array(x, np.uint32) for x in EXTRA]
    return shapes, texts + neighbours([0x61, 0x62], [0x63])


@functools.lru_cache(maxsize=None)
def corpus_starts(encname):
    """per document of the corpus: the unit offset of every char"""
    return [ref_encode(t, ENCS[encname])[1] for t in corpus()[1]]


@functools.lru_cache(maxsize=None)
def corpus_positions(k):
    """the match positions of PATTERNS[k] in every document of the corpus (the same for both
    encodings and leaf sizes: every test checks crdt_text against the corpus first)"""
    pat, icase = PATTERNS[k]
    return [ref_find_pos(t, pat, icase) for t in corpus()[1]]


def corpus_matches(k, encname):
    return [np.stack([st[p], p], axis=1).astype(np.uint32).reshape(-1, 2)
            for st, p in zip(corpus_starts(encname), corpus_positions(k))]


def load(e, texts):
    """one local insert per document plus set_content, as the line test sets its texts up"""
    nd = len(texts)
    docs = list(range(nd))
    ag = e.agent_intern(docs, ["xa"] * nd)
    assert (e.apply_local([(d, [(int(ag[d]), [(0, 0, len(t))])]) for d, t in enumerate(texts) if len(t)]) == 0).all()
    e.set_content(docs, docs, texts)
    return docs


def check_matches(e, idxs, want):
    """n_matches and crdt_find_read of the listed indexes"""
    counts = e.find_counts()
    for i, w in zip(idxs, want):
        assert int(counts[i]) == len(w), (i, int(counts[i]), len(w))
        got = e.find_read(i, counts)
        assert got.dtype == np.uint32 and got.shape == w.shape and np.array_equal(got, w), (i, got[:4], w[:4])
    return counts


def seek_queries(idxs, chars, matches):
    """every pos in [0, chars + 2] of every listed index, with the reference's answers per direction"""
    qi = np.concatenate([np.full(c + 3, i, np.uint32) for i, c in zip(idxs, chars)])
    qp = np.concatenate([np.arange(c + 3, dtype=np.uint32) for c in chars])
    want = {d: np.concatenate([ref_seek(m, np.arange(c + 3), d) for c, m in zip(chars, matches)]) for _, d in DIRS}
    return qi, qp, want


def check_seeks(e, idxs, chars, matches, device_form=True, seed=7):
    qi, qp, want = seek_queries(idxs, chars, matches)
    o = np.random.default_rng(seed).permutation(len(qi))  # several documents mixed in one batch
    qi, qp = qi[o], qp[o]
    for dirname, d in DIRS:
        assert np.array_equal(e.find_seek(qi, qp, dirname), want[d][o]), dirname
    if not device_form:
        return
    with torch.cuda.stream(torch.cuda.ExternalStream(e.stream(), device=torch.cuda.current_device())):
        ti = torch.from_numpy(qi.astype(np.int32)).to("cuda", non_blocking=False)
        tp = torch.from_numpy(qp.astype(np.int32)).to("cuda", non_blocking=False)
        outs = []
        for _, d in DIRS:
            k = torch.full((len(qi),), 7, dtype=torch.int32, device="cuda")
            assert e.L.crdt_find_seek_dev_async(e.h, len(qi), ti.data_ptr(), tp.data_ptr(), d, k.data_ptr()) == 0
            outs.append(k)
        e.sync()
        for (_, d), k in zip(DIRS, outs):
            assert np.array_equal(k.cpu().numpy().view(np.uint32), want[d][o])


def check_all(e, docs, enc, pattern, icase=False, seeks=True, seed=7):
    """the find result of the last encode (of `docs`, in `enc`) against the reference of the engine's own text"""
    texts = [e.text(d) for d in docs]
    want = [ref_find(t, ref_encode(t, enc)[1], pattern, icase) for t in texts]
    idxs = list(range(len(docs)))
    check_matches(e, idxs, want)
    if seeks:
        check_seeks(e, idxs, [len(t) for t in texts], want, device_form=False, seed=seed)
    return want


def corpus_engine(leaf, encname):
    shapes, texts = corpus()
    e = crdt_amd.Engine(len(texts), leaf)
    docs = load(e, texts)
    starts = corpus_starts(encname)
    e.encode_async(docs, encname)
    units, chars = e.encode_lens()
    for d in docs:
        assert np.array_equal(e.text(d), texts[d])
        assert int(units[d]) == int(starts[d][-1]) and int(chars[d]) == len(texts[d])
    return e, shapes, texts


@pytest.mark.parametrize("encname", ["utf8", "utf16"])
@pytest.mark.parametrize("leaf", [32, 4])
def test_seams_lengths_contents_and_patterns(leaf, encname):
    e, shapes, texts = corpus_engine(leaf, encname)
    idxs = list(range(len(texts)))
    base = len(shapes)              # the explicit cases
    nb = base + len(EXTRA)          # the packed neighbours
    by_pattern = {}
    for k, (pat, icase) in enumerate(PATTERNS):
        e.find_async(pat, icase)
        counts = check_matches(e, idxs, corpus_matches(k, encname))
        assert e.find_ms() > 0
        by_pattern[(tuple(pat.tolist()), icase)] = [int(x) for x in counts]
        if (pat == 0x61).all() and not icase:  # 'a' * m in all 'a': every start but the last m - 1
            m = len(pat)
            for i, (kind, n) in enumerate(shapes):
                if kind == 0:
                    assert int(counts[i]) == max(0, n - m + 1), (m, n)
    # a value that is no scalar value is U+FFFD, in the pattern and in the text
    for p in (0xD800, 0xFFFD):
        assert by_pattern[((p,), False)][base:base + 2] == [1, 1]
    # 'A' folded matches 'A' and 'a', and no UTF-16 unit that merely holds 0x41 in one of its bytes
    assert by_pattern[((0x41,), True)][base:base + 10] == [0, 0, 0, 0, 0, 1, 1, 0, 0, 0]
    # 'k' folded matches 'K' and not the Kelvin sign; nothing outside ASCII folds
    assert by_pattern[((0x6B,), True)][base:base + 10] == [0, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    assert by_pattern[((0xC9,), True)][base:base + 10] == [0, 0, 0, 0, 0, 0, 0, 0, 1, 0]
    # the packed neighbours "ab", "c", "ab", "", "cab", "abc"
    for pat, want in (("abc", [0, 0, 0, 0, 0, 1]), ("b", [1, 0, 1, 0, 1, 1]), ("ca", [0, 0, 0, 0, 1, 0])):
        e.find_async(pat)
        counts = e.find_counts()
        assert [int(counts[nb + k]) for k in range(6)] == want, pat
        for k in range(6):
            assert np.array_equal(e.find_read(nb + k, counts), ref_find(texts[nb + k], corpus_starts(encname)[nb + k], pat))


@pytest.mark.parametrize("encname", ["utf8", "utf16"])
def test_packed_neighbours_at_the_full_pattern_length_and_the_end_of_the_pool(encname):
    enc = ENCS[encname]
    for pat in (S64, Q64):
        texts = neighbours(pat[:40], pat[40:])
        e = crdt_amd.Engine(len(texts), 32)
        docs = load(e, texts)
        e.encode_async(docs, encname)
        units, _ = e.encode_lens()
        # the last document of the call ends exactly at the end of the pool: its units fill whole dwords
        assert (int(units.sum()) * (1 if enc == UTF8 else 2)) % 4 == 0
        # (documents 0 | 1 and 2 | 4 put the whole pattern, and 1 | 2 its tail and head, side by side in the pool)
        for p, want in ((pat, [0, 0, 0, 0, 0, 1]), (pat[40:], [0, 1, 0, 0, 1, 1]), (pat[32:48], [0, 0, 0, 0, 0, 1]),
                        (np.concatenate([pat[56:], pat[:8]]), [0, 0, 0, 0, 1, 0])):
            e.find_async(p)
            assert [int(x) for x in e.find_counts()] == want
            check_all(e, docs, enc, p)


@pytest.mark.parametrize("encname", ["utf8", "utf16"])
def test_seek_every_position_both_directions(encname):
    e, shapes, texts = corpus_engine(32, encname)
    idxs = list(range(len(texts)))
    chars = [len(t) for t in texts]
    # many matches, few, overlapping ones, four-byte chars, and a pattern most documents do not hold
    for k in (0, 8, 13, 11, 19):
        pat, icase = PATTERNS[k]
        e.find_async(pat, icase)
        want = corpus_matches(k, encname)
        assert any(len(w) == 0 for w in want) and any(len(w) > 1 for w in want)
        check_seeks(e, idxs, chars, want, seed=k)
    # an index with 0 matches answers 0xFFFFFFFF everywhere (the last pattern: the empty document)
    q = np.arange(5, dtype=np.uint32)
    for dirname, _ in DIRS:
        assert (e.find_seek(np.full(5, 1, np.uint32), q, dirname) == INVALID).all()


def test_edited_text_concurrent_history_and_trace():
    rng = np.random.default_rng(62)
    wires = [concurrent_wire(s, n_agents=3, rounds=5)[0] for s in range(3)]
    t = load_trace("sveltecomponent")
    n = len(wires)
    e = crdt_amd.Engine(n + 1, 32)
    assert (e.apply_remote_wire(list(range(n)), wires) == 0).all()
    ag = int(e.agent_intern([n], ["jeremy"])[0])
    assert e.apply_trace([n], ag, t.counts, t.patches)[0] == 0
    nv = e.versions(list(range(n)))
    streams = [rng.choice(np.array([0x61, 0x62, 0x41], np.uint32), int(v)) for v in nv]
    streams.append(content_by_order(t))
    docs = list(range(n + 1))
    e.set_content(docs, docs, streams)
    text = e.text(n)
    s = utf32_to_str(text)
    word = collections.Counter(re.findall(r"[A-Za-z]{5,}", s)).most_common(1)[0][0]  # a word of the trace's text
    for encname, enc in ENCS.items():
        res = e.encode(docs, encname)
        for pat, icase in (("ab", False), ("a", True), ("aba", True), ("bAa", False)):
            e.find_async(pat, icase)
            check_all(e, docs[:n], enc, pat, icase)  # (indexes 0..n-1 are documents 0..n-1)
        # the trace's document: the units of every match of the word equal a lookahead search over
        # the encoded bytes
        e.find_async(word)
        counts = e.find_counts()
        assert int(counts[n]) > 1
        got = e.find_read(n, counts)
        if enc == UTF8:
            want = [m.start() for m in re.finditer(b"(?=" + re.escape(word.encode("utf-8")) + b")", res[n])]
        else:
            hay = res[n].astype("<u2").tobytes()
            at = [m.start() for m in re.finditer(b"(?=" + re.escape(word.encode("utf-16-le")) + b")", hay)]
            want = [o // 2 for o in at if o % 2 == 0]
        assert got[:, 0].tolist() == want
        assert np.array_equal(got, ref_find(text, ref_encode(text, enc)[1], word))
        q = rng.integers(0, len(text) + 3, 4096).astype(np.uint32)
        for dirname, d in DIRS:
            assert np.array_equal(e.find_seek(np.full(len(q), n, np.uint32), q, dirname), ref_seek(got, q, d))


def test_result_lifetime_and_the_other_results():
    rng = np.random.default_rng(63)
    e = crdt_amd.Engine(6, 32)
    wires = [concurrent_wire(s)[0] for s in range(6)]
    assert (e.apply_remote_wire(list(range(6)), wires) == 0).all()
    docs6 = list(range(6))
    streams = [rng.choice(np.array([0x61, 0x62, 0x41, 0x0A, 0xE9, 0x1F600], np.uint32), int(v) + 16) for v in e.versions()]  # (room for the late edits)
    e.set_content(docs6, docs6, streams)
    # diff, checkout, blame and encode results and a line index made before the find
    v = e.versions([2, 4])
    diff0 = e.diff([2, 4], v // 2)
    co0 = e.checkout([4, 2], v[::-1] // 3)
    bl0 = e.blame([2, 4], "id")
    dg = e.digests()
    docs = [5, 0, 3]  # a listed subset, not ascending
    enc0 = e.encode(docs, "utf8")
    lens0 = e.encode_lens()
    lines0 = e.lines("lf")
    before = e.mem_bytes()
    e.find_async("a")
    assert e.mem_bytes() > before  # the buffers are counted
    first = check_all(e, docs, UTF8, "a")
    assert len(e.find_counts()) == 3
    assert np.array_equal(e.digests(), dg)  # a find changes no document
    for i in range(2):  # ... and none of the other results
        for a, b in zip(diff0[i], e.diff_read(i)):
            assert np.array_equal(a, b)
        for a, b in zip(co0[i], e.checkout_read(i)):
            assert np.array_equal(a, b)
        assert np.array_equal(bl0[i], e.blame_read(i))
    for i in range(3):
        assert e.encode_read(i) == enc0[i]
        assert np.array_equal(e.lines_read(i), lines0[i])  # the line index too
        t = e.text(docs[i])
        assert np.array_equal(lines0[i], ref_lines(t, ref_encode(t, UTF8)[1], EOL_LF))
    assert all(np.array_equal(a, b) for a, b in zip(lens0, e.encode_lens()))
    # a later line index does not touch the find result
    e.lines_async("any")
    check_matches(e, [0, 1, 2], first)
    # a second find replaces the first
    e.find_async("AB", icase=True)
    second = check_all(e, docs, UTF8, "AB", True)
    assert any(len(a) != len(b) for a, b in zip(first, second))
    chars = [int(c) for c in lens0[1]]
    # more edits and a new materialise: the result and its seeks still give the old answers
    old_text0 = e.text(0)
    ag = e.agent_intern([0, 1], ["late"] * 2)
    assert (e.apply_local([(0, [(int(ag[0]), [(0, 0, 4)])]), (1, [(int(ag[1]), [(1, 2, 0)])])]) == 0).all()
    e.materialize_async()
    e.sync()
    assert len(e.text(0)) == len(old_text0) + 4
    check_matches(e, [0, 1, 2], second)
    check_seeks(e, [0, 1, 2], chars, second, device_form=False, seed=8)
    # a new encode drops it
    e.encode_async([1, 0], "utf16")
    one = np.zeros(1, np.uint32)
    for call in (e.find_counts, lambda: e.find_read(0, np.ones(2, np.uint32)), lambda: e.find_seek(one, one),
                 lambda: e.find_seek(one, one, "prev")):
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            call()
    assert e.L.crdt_find_seek_dev_async(e.h, 1, None, None, 0, None) == -100
    # ... and the next find is of the new encode, and of the new text
    e.find_async("ab")
    check_all(e, [1, 0], UTF16, "ab")
    assert len(e.find_counts()) == 2
    # a later encode call drops it, successful or not: one rejected for its arguments leaves the
    # encode result, on which the next find is built
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.encode_async([0, 0], "utf8")
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.find_counts()
    assert e.L.crdt_find_seek_dev_async(e.h, 1, None, None, 1, None) == -100
    assert len(e.encode_lens()[0]) == 2
    e.find_async("\U0001F600")
    check_all(e, [1, 0], UTF16, "\U0001F600")
    # an encode of [] gives an empty result
    assert e.encode([], "utf8") == []
    assert e.find("a") == [] and len(e.find_counts()) == 0
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.find_seek(one, one)


def test_no_result_and_argument_errors():
    wire, _ = concurrent_wire(1)
    e = crdt_amd.Engine(6, 32)
    one = np.zeros(1, np.uint32)
    P32 = crdt_amd.C.POINTER(crdt_amd.C.c_uint32)

    def p32(a):
        return a.ctypes.data_as(P32)

    ab = np.array([0x61, 0x62], np.uint32)
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.find_async("a")  # before any encode
    for call in (e.find_counts, lambda: e.find_read(0, np.ones(1, np.uint32)), lambda: e.find_seek(one, one)):
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            call()
    assert (e.apply_remote_wire([0, 2, 3, 5], [wire] * 4) == 0).all()
    ag = int(e.agent_intern([1], ["p"])[0])
    bad = [[(0, 0, 5)], [(2, 1, 0)], [(3, 5, 0)], [(0, 0, 1)]]      # the third txn deletes past the end
    assert e.apply_local([(1, [(ag, o) for o in bad])])[0] == -1
    nv = int(e.versions([0])[0])
    c = np.random.default_rng(64).choice(np.array([0x61, 0x62, 0x41, 0xE9], np.uint32), nv)
    # 0, 2, 5 healthy; 1 poisoned (with content); 3 one entry short; 4 (empty) without content
    e.set_content([0, 1, 2, 3, 5], [0, 0, 0, 1, 0], [c, c[:-1]])
    docs = list(range(6))
    none = [False, True, False, True, True, False]
    keep = [i for i in docs if not none[i]]
    for encname, enc in ENCS.items():
        e.encode(docs, encname, strict=False)
        e.find_async("ab")
        long65 = np.full(65, 0x61, np.uint32)
        assert e.L.crdt_find_async(e.h, p32(ab), 0, 0) == -100          # n_chars 0
        assert e.L.crdt_find_async(e.h, p32(long65), 65, 0) == -100     # ... and 65
        assert e.L.crdt_find_async(e.h, None, 2, 0) == -100             # a NULL pattern
        assert e.L.crdt_find_async(e.h, p32(ab), 2, 2) == -100          # an unknown flag bit
        assert e.L.crdt_find_async(e.h, p32(ab), 2, -1) == -100
        with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
            e.find_seek(one, one, 2)  # an unknown dir
        assert e.L.crdt_find_seek_dev_async(e.h, 0, None, None, 2, None) == -100
        assert e.L.crdt_find_seek_dev_async(e.h, 0, None, None, -1, None) == -100
        for pat, icase in (("a", False), ("A", True)):
            res = e.find(pat, icase, strict=False)
            counts = e.find_counts()
            assert [int(x) == INVALID for x in counts] == none
            for i in docs:
                if not none[i]:
                    continue
                assert res[i] is None
                with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                    e.find_read(i)
                with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                    e.find_seek([0, i], [0, 0])  # a host seek that names it
            with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                e.find(pat, icase)  # strict
            # the healthy ones' answers are intact, all in one batch
            texts = [e.text(i) for i in keep]
            want = [ref_find(t, ref_encode(t, enc)[1], pat, icase) for t in texts]
            check_matches(e, keep, want)
            check_seeks(e, keep, [len(t) for t in texts], want, device_form=False)
            assert np.array_equal(res[0], want[0]) and len(want[0]) > 1
            # the device form answers an idx out of range or without a result 0xFFFFFFFF
            with torch.cuda.stream(torch.cuda.ExternalStream(e.stream(), device=torch.cuda.current_device())):
                idx = torch.tensor([0, 1, 3, 4, 6, 0x7FFFFFFF, 0], dtype=torch.int32, device="cuda")
                val = torch.tensor([1, 0, 0, 0, 0, 0, 1], dtype=torch.int32, device="cuda")
                outs = []
                for _, d in DIRS:
                    k = torch.full((7,), 7, dtype=torch.int32, device="cuda")
                    assert e.L.crdt_find_seek_dev_async(e.h, 7, idx.data_ptr(), val.data_ptr(), d, k.data_ptr()) == 0
                    outs.append(k)
                e.sync()
                got = [k.cpu().numpy().view(np.uint32).tolist() for k in outs]
            for (_, d), g in zip(DIRS, got):
                w = int(ref_seek(want[0], [1], d)[0])
                assert g == [w] + [INVALID] * 5 + [w]
    # host form: an idx without a result or out of range, or an unknown dir: -100 and nothing written
    out = np.full(2, 9, np.uint32)
    z2 = np.zeros(2, np.uint32)
    for i2, d in ((np.array([0, 1], np.uint32), 0), (np.array([0, 6], np.uint32), 1), (z2, 2), (z2, -1)):
        assert e.L.crdt_find_seek(e.h, 2, p32(i2), p32(z2), d, p32(out)) == -100
        assert (out == 9).all()
    with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
        e.find_read(6)  # out of range
    # the engine still answers
    e.encode([5], "utf8")
    e.find_async("b")
    check_all(e, [5], UTF8, "b")


def test_allocation_failure_leaves_the_engine_usable():
    wire, _ = concurrent_wire(2)
    L = crdt_amd.lib()
    failed = 0
    for k in range(8):  # the first find of an engine allocates every buffer it needs: fail each in turn
        before = crdt_amd.Engine.device_bytes()[0]
        e = crdt_amd.Engine(2, 32)
        assert (e.apply_remote_wire([0, 1], [wire] * 2) == 0).all()
        c = cycle_text(int(e.versions([0])[0]))
        c[1::8] = 0x0A
        e.set_content([0, 1], [0, 0], [c])
        enc0 = e.encode([0, 1], "utf8")
        lines0 = e.lines("lf")
        dg = e.digests()
        L.crdt_test_fail_alloc_after(k)
        try:
            e.find_async("A")
            ok = True
        except crdt_amd.CrdtError as x:
            assert "rc=-102" in str(x), x
            ok = False
        finally:
            L.crdt_test_fail_alloc_after(-1)
        if not ok:
            failed += 1
            # the engine is not poisoned, has no find result, and its encode result and line index are intact
            with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                e.find_counts()
            with pytest.raises(crdt_amd.CrdtError, match="rc=-100"):
                e.find_seek([0], [0])
            assert np.array_equal(e.digests(), dg)
            assert [e.encode_read(i) for i in (0, 1)] == enc0
            assert all(np.array_equal(e.lines_read(i), lines0[i]) for i in (0, 1))
            e.find_async("A")  # ... and the same call then succeeds
        want = check_all(e, [0, 1], UTF8, "A")
        assert len(want[0]) > 1
        e.close()
        now = crdt_amd.Engine.device_bytes()[0]
        assert now <= before, (k, now, before)  # nothing of a closed engine stays allocated
        if ok:
            break
    assert failed == 4, failed  # (the per-index counts, the total, the pattern and the table)


def test_the_one_document_wrapper():
    doc = crdt_amd.ListCRDT()
    a = doc.get_or_create_agent_id("seph")
    s = "héllo €\U0001F600 HÉLLO hello\ud800"
    assert doc.local_insert(a, 0, len(s)) == 0
    doc.set_content(np.array([ord(c) for c in s], np.uint32))
    assert np.array_equal(sanitise(doc.e.text(0)), sanitise(s))

    def want(pat, enc, flags=0):
        at = [m.start() for m in re.finditer("(?=" + re.escape(pat) + ")", s, flags)]
        return [[len(s[:p].encode(enc)) // (1 if enc == "utf-8" else 2), p] for p in at]

    assert want("llo", "utf-8") == [[3, 2], [24, 17]] and want("llo", "utf-16-le") == [[2, 2], [18, 17]]
    assert doc.find("llo").tolist() == want("llo", "utf-16-le")                # UTF-16 units
    assert doc.find("llo", "utf8").tolist() == want("llo", "utf-8")            # bytes
    assert doc.find("llo", icase=True).tolist() == want("llo", "utf-16-le", re.ASCII | re.IGNORECASE)
    assert doc.find("llo", icase=True)[:, 1].tolist() == [2, 11, 17]
    assert doc.find("hé", icase=True)[:, 1].tolist() == [0]                    # (É does not fold)
    assert doc.find("\ufffd")[:, 1].tolist() == [len(s) - 1] and doc.find("\ud800")[:, 1].tolist() == [len(s) - 1]
    assert doc.find("xyz").shape == (0, 2)
    assert doc.e.find_seek([0, 0], [3, 3], "next").tolist() == [INVALID, INVALID]
    doc.e.find_async("l")
    assert doc.e.find_seek([0, 0], [4, 4], "next").tolist() == [2, 2] and doc.e.find_seek([0], [4], "prev").tolist() == [1]
    assert doc.e.find_ms() > 0
