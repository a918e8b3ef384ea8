"""CPU checks of the find definition (tests/find_ref.py) against Python itself (re lookahead search
over the str and over its encoded bytes), of the ASCII-only fold, of the seek against a linear
scan, and of the library's find entry points being exported.
"""
import ctypes
import re

import numpy as np
import pytest

import crdt_amd
from encode_ref import UTF8, UTF16, ref_encode
from find_ref import INVALID, SEEK_NEXT, SEEK_PREV, ref_find, ref_find_pos, ref_seek

# (the header declares six functions for this feature)
FIND_SYMBOLS = ["crdt_find_async", "crdt_find_counts", "crdt_find_read", "crdt_find_seek", "crdt_find_seek_dev_async",
                "crdt_last_find_ms"]

# scalar values only: a char of every width, the case pairs, and the chars a wider fold would touch
ALPHABET = [0x61, 0x41, 0x62, 0x4B, 0x6B, 0xE9, 0xC9, 0x20AC, 0x1F600, 0x212A, 0x0130, 0x0141, 0x4100]
HAND_MADE = [("", "a"), ("a", "a"), ("aaaa", "aa"), ("aaaa", "aaaaa"), ("abcabcab", "abc"), ("abcabcab", "cab"),
             ("xabababx", "abab"), ("é€\U0001F600é€", "é€"), ("\U0001F600\U0001F600\U0001F600", "\U0001F600\U0001F600"),
             ("a.b*c", ".b*"), ("KkK", "k"), ("ÉéE", "é")]


def cases():
    rng = np.random.default_rng(51)
    out = list(HAND_MADE)
    for n in (1, 2, 3, 7, 64, 65, 300):
        for sub in (ALPHABET[:2], ALPHABET[:3], ALPHABET):
            s = "".join(map(chr, rng.choice(sub, n).tolist()))
            for m in (1, 2, 3, 5):
                a = int(rng.integers(0, max(1, n - m + 1)))
                out.append((s, s[a:a + m] or "a"))                              # a pattern taken from the text
                out.append((s, "".join(map(chr, rng.choice(sub, m).tolist()))))  # ... and a random one
    return out


def lookahead(pat, s, flags=0):
    """every start of pat in s (str or bytes), overlapping occurrences included"""
    pre, post = (b"(?=", b")") if isinstance(pat, bytes) else ("(?=", ")")
    return [m.start() for m in re.finditer(pre + re.escape(pat) + post, s, flags)]


def u32(s):
    return np.array([ord(c) for c in s], np.uint32)


def test_matches_equal_pythons_lookahead_search():
    for s, pat in cases():
        got = ref_find_pos(u32(s), pat)
        assert got.dtype == np.uint32 and got.tolist() == lookahead(pat, s), (s, pat)
        assert ref_find_pos(u32(s), u32(pat)).tolist() == got.tolist()  # (a str or an array)


def test_units_equal_the_lookahead_search_over_the_encoded_bytes():
    for s, pat in cases():
        t = u32(s)
        _, start = ref_encode(t, UTF8)
        got = ref_find(t, start, pat)
        assert got.dtype == np.uint32 and got.shape == (len(got), 2)
        assert got[:, 0].tolist() == lookahead(pat.encode("utf-8"), s.encode("utf-8")), (s, pat)
        _, start = ref_encode(t, UTF16)
        got = ref_find(t, start, pat)
        # byte offsets of the UTF-16 search, odd ones (no unit boundary) discarded
        want = [o // 2 for o in lookahead(pat.encode("utf-16-le"), s.encode("utf-16-le")) if o % 2 == 0]
        assert got[:, 0].tolist() == want, (s, pat)
        assert got[:, 1].tolist() == lookahead(pat, s)


def test_the_fold_is_ascii_only():
    # re.ASCII | re.IGNORECASE folds A-Z / a-z and nothing else: not U+212A (KELVIN SIGN) to k, not É to é
    assert ref_find_pos(u32("KkK"), "k", True).tolist() == [0, 1]
    assert ref_find_pos(u32("KkK"), "K", True).tolist() == [2]
    assert ref_find_pos(u32("ÉéE"), "é", True).tolist() == [1]
    assert ref_find_pos(u32("ÉéE"), "É", True).tolist() == [0]
    assert ref_find_pos(u32("İiI"), "i", True).tolist() == [1, 2]
    for s, pat in cases():
        got = ref_find_pos(u32(s), pat, True)
        assert got.tolist() == lookahead(pat, s, re.ASCII | re.IGNORECASE), (s, pat)
        assert set(ref_find_pos(u32(s), pat).tolist()) <= set(got.tolist())


def test_values_that_are_no_scalar_values_are_u_fffd():
    t = np.array([0xD800, 0x61, 0xFFFD, 0x110000, 0xDFFF, 0xFFFFFFFF], np.uint32)
    for pat in ([0xD800], [0xFFFD], [0x110000], [0xDFFF]):
        assert ref_find_pos(t, np.array(pat, np.uint32)).tolist() == [0, 2, 3, 4, 5]
    assert ref_find_pos(t, "\ud800a").tolist() == [0]  # (a str goes through ord: a lone surrogate)
    with pytest.raises(ValueError):
        ref_find_pos(t, "")
    with pytest.raises(ValueError):
        ref_find_pos(t, "a" * 65)


def test_seek_equals_a_linear_scan():
    for s, pat in cases()[::3]:
        t = u32(s)
        _, start = ref_encode(t, UTF8)
        mt = ref_find(t, start, pat)
        q = np.arange(len(s) + 3, dtype=np.uint32)
        nxt, prv = ref_seek(mt, q, SEEK_NEXT), ref_seek(mt, q, SEEK_PREV)
        assert nxt.dtype == prv.dtype == np.uint32
        for p in q.tolist():
            ge = [k for k in range(len(mt)) if int(mt[k, 1]) >= p]
            le = [k for k in range(len(mt)) if int(mt[k, 1]) <= p]
            assert int(nxt[p]) == (ge[0] if ge else INVALID) and int(prv[p]) == (le[-1] if le else INVALID), (s, pat, p)
    with pytest.raises(ValueError):
        ref_seek(np.zeros((0, 2), np.uint32), [0], 2)


def test_library_exports_the_find_entry_points():
    crdt_amd.build()
    lib = ctypes.CDLL(crdt_amd.LIB_PATH)
    for s in FIND_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in crdt_amd.EXPORTED_SYMBOLS, s
