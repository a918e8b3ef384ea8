"""CPU checks of the encoded-text definition (tests/encode_ref.py) against Python's own codecs,
of its query properties, of the reference's trace fixtures, and of the library's encode entry
points being exported.
"""
import ctypes

import numpy as np
import pytest

import crdt_amd
from crdt_amd.traces import content_by_order, fnv1a64, load_trace
from encode_ref import (BOUNDARY, INVALID, NOT_SCALAR, UTF8, UTF16, cycle_text, ref_encode, ref_pos_to_units,
                        ref_units_to_pos, ref_units_to_pos_all)
from oracle_lib import OracleDoc

# (the header declares eight functions for this feature)
ENCODE_SYMBOLS = ["crdt_encode_async", "crdt_encode_lens", "crdt_encode_read", "crdt_pos_to_units", "crdt_units_to_pos",
                  "crdt_pos_to_units_dev_async", "crdt_units_to_pos_dev_async", "crdt_last_encode_ms"]


def scalar_texts():
    rng = np.random.default_rng(11)
    pool = np.array(BOUNDARY, np.uint32)
    out = [np.zeros(0, np.uint32), pool, pool[::-1].copy(), cycle_text(41)]
    out += [np.array([c], np.uint32) for c in BOUNDARY]
    out += [rng.choice(pool, n) for n in (2, 63, 64, 65, 300)]
    any_scalar = rng.integers(0, 0x110000, 2000, dtype=np.uint32)
    out.append(any_scalar[(any_scalar < 0xD800) | (any_scalar >= 0xE000)])
    return out


def test_reference_equals_the_python_codecs():
    for t in scalar_texts():
        s = "".join(map(chr, t.tolist()))
        u8, st8 = ref_encode(t, UTF8)
        u16, st16 = ref_encode(t, UTF16)
        assert u8.dtype == np.uint8 and u8.tobytes() == s.encode("utf-8")
        assert u16.dtype == np.uint16 and u16.astype("<u2").tobytes() == s.encode("utf-16-le")
        assert len(st8) == len(st16) == len(t) + 1 and st8[-1] == len(u8) and st16[-1] == len(u16)
        if len(t):
            assert np.array_equal(np.diff(st8.astype(np.int64)), [len(chr(c).encode("utf-8")) for c in t.tolist()])
            assert np.array_equal(np.diff(st16.astype(np.int64)), [len(chr(c).encode("utf-16-le")) // 2 for c in t.tolist()])


def test_values_that_are_no_scalar_values_encode_as_the_replacement_character():
    for enc in (UTF8, UTF16):
        want = ref_encode(np.array([0xFFFD], np.uint32), enc)[0]
        for c in NOT_SCALAR:
            assert np.array_equal(ref_encode(np.array([c], np.uint32), enc)[0], want), hex(c)
        mixed = np.array([0x41, 0xD800, 0x1F600, 0xFFFFFFFF, 0x7FF], np.uint32)
        clean = np.array([0x41, 0xFFFD, 0x1F600, 0xFFFD, 0x7FF], np.uint32)
        assert np.array_equal(ref_encode(mixed, enc)[0], ref_encode(clean, enc)[0])
    assert ref_encode(np.array([0xDFFF], np.uint32), UTF8)[0].tobytes() == b"\xef\xbf\xbd"
    assert ref_encode(np.array([0x110000], np.uint32), UTF16)[0].tolist() == [0xFFFD]


def test_query_properties():
    rng = np.random.default_rng(12)
    texts = scalar_texts() + [rng.choice(np.array(BOUNDARY + NOT_SCALAR, np.uint32), 150)]
    for t in texts:
        for enc in (UTF8, UTF16):
            units, start = ref_encode(t, enc)
            chars, n = len(t), len(units)
            pos_all, mid_all = ref_units_to_pos_all(start)
            for u in range(n + 3):
                pos, mid = ref_units_to_pos(start, u)
                assert (pos, mid) == (int(pos_all[u]), int(mid_all[u]))
                if u > n:
                    assert (pos, mid) == (INVALID, 0)
                    continue
                # the round trip: back at or below u, and at u exactly when u starts a char
                back = ref_pos_to_units(start, pos)
                assert back <= u and (back == u) == (mid == 0)
                if u == n:
                    assert (pos, mid) == (chars, 0)
                    continue
                # the mid rule, on the units themselves
                x = int(units[u])
                cont = (x & 0xC0) == 0x80 if enc == UTF8 else 0xDC00 <= x <= 0xDFFF
                assert mid == int(cont)
            for p in range(chars + 3):
                got = ref_pos_to_units(start, p)
                assert got == (int(start[p]) if p <= chars else INVALID)
                if p <= chars:
                    assert ref_units_to_pos(start, got) == (p, 0)
            assert ref_pos_to_units(start, chars) == n


@pytest.mark.parametrize("name", ["sveltecomponent", "rustcode", "automerge-paper"])
def test_trace_fixtures(name):
    # the reference's endContent, through the definition (all three are ASCII: end_bytes == end_len)
    t = load_trace(name)
    o = OracleDoc(32, 16)
    assert o.apply_trace(o.agent("a"), t.counts, t.patches) == 0
    txt, _ = o.text(content_by_order(t))
    units, start = ref_encode(txt, UTF8)
    assert len(units) == t.end_bytes and int(start[-1]) == t.end_bytes
    assert fnv1a64(units.tobytes()) == t.end_fnv


def test_library_exports_the_encode_entry_points():
    crdt_amd.build()
    lib = ctypes.CDLL(crdt_amd.LIB_PATH)
    for s in ENCODE_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in crdt_amd.EXPORTED_SYMBOLS, s
