"""CPU checks of the line-index definition (tests/lines_ref.py) against Python itself (str.split,
re.split, the codecs), of the bijection between positions and (line, column) pairs, of the
whole-document helpers the GPU tests use, and of the library's line entry points being exported.
"""
import ctypes
import re

import numpy as np

import crdt_amd
from encode_ref import UTF8, UTF16, ref_encode
from lines_ref import (COL_CHARS, COL_UNITS, EOL_ANY, EOL_LF, INVALID, ref_extent, ref_linecol_to_pos,
                       ref_linecol_to_pos_all, ref_lines, ref_pos_to_linecol, ref_pos_to_linecol_all)

# (the header declares eight functions for this feature)
LINES_SYMBOLS = ["crdt_lines_async", "crdt_line_counts", "crdt_lines_read", "crdt_pos_to_linecol", "crdt_linecol_to_pos",
                 "crdt_pos_to_linecol_dev_async", "crdt_linecol_to_pos_dev_async", "crdt_last_lines_ms"]

# LF, CR, a char of every width, the breaks of other conventions (none here), and the UTF-16 traps
# of a byte-wise compare (U+010A, U+0A0A, U+0A0D, U+0D0A)
ALPHABET = [0x0A, 0x0D, 0x61, 0xE9, 0x20AC, 0x1F600, 0x0B, 0x0C, 0x85, 0x2028, 0x2029, 0x010A, 0x0A0A, 0x0A0D, 0x0D0A]
HAND_MADE = ["", "\n", "\r", "\r\n", "\n\r", "\r\r\n", "\n\n", "a", "a\n", "a\r", "a\r\n", "\na", "\ra", "\r\na",
             "a\nb", "a\rb", "a\r\nb", "é\n€\r\U0001F600\r\n", "\r\n\r\n", "\r\r", "x y\u0085z\x0b\x0c",
             "\u0a0a\u010a\u0a0d\u0d0a", "ab\r", "ab\r\n\r"]


def texts():
    rng = np.random.default_rng(31)
    out = list(HAND_MADE)
    for n in (1, 2, 3, 7, 64, 65, 200):
        for _ in range(3):
            out.append("".join(map(chr, rng.choice(ALPHABET, n).tolist())))
        out.append("".join(map(chr, rng.choice([0x0A, 0x0D], n).tolist())))
    return out


def python_lines(s: str, eol: int) -> list:
    return s.split("\n") if eol == EOL_LF else re.split("\r\n|\r|\n", s)


def unit_len(s: str, enc: int) -> int:
    return len(s.encode("utf-8")) if enc == UTF8 else len(s.encode("utf-16-le")) // 2


def test_lines_equal_pythons_split():
    for s in texts():
        t = np.array([ord(c) for c in s], np.uint32)
        for enc in (UTF8, UTF16):
            _, start = ref_encode(t, enc)
            for eol in (EOL_LF, EOL_ANY):
                lines = ref_lines(t, start, eol)
                want = python_lines(s, eol)
                assert lines.dtype == np.uint32 and lines.shape == (len(want), 2), (s, eol)
                assert lines[0].tolist() == [0, 0]
                # every line is the text between its start and the next start, less its terminator
                ends = lines[1:, 1].tolist() + [len(s)]
                for k, w in enumerate(want):
                    a, b = int(lines[k, 1]), ends[k]
                    got = s[a:b]
                    if k + 1 < len(want):
                        term = got[len(w):]
                        assert term in (("\n",) if eol == EOL_LF else ("\n", "\r", "\r\n")), (s, eol, k)
                        got = got[:len(w)]
                    assert got == w, (s, eol, k)
                    assert int(lines[k, 0]) == unit_len(s[:a], enc)
                    assert ref_extent(lines, start, k, COL_CHARS) == b - a
                    assert ref_extent(lines, start, k, COL_UNITS) == unit_len(s[a:b], enc)


def test_columns_equal_the_encoded_length_of_the_line_prefix():
    for s in texts():
        t = np.array([ord(c) for c in s], np.uint32)
        for enc in (UTF8, UTF16):
            _, start = ref_encode(t, enc)
            for eol in (EOL_LF, EOL_ANY):
                lines = ref_lines(t, start, eol)
                for p in range(len(s) + 1):
                    line, col = ref_pos_to_linecol(lines, start, p, COL_CHARS)
                    a = int(lines[line, 1])
                    assert a <= p and col == p - a and (line + 1 == len(lines) or p < int(lines[line + 1, 1]))
                    line_u, col_u = ref_pos_to_linecol(lines, start, p, COL_UNITS)
                    assert line_u == line and col_u == unit_len(s[a:p], enc)
                for p in (len(s) + 1, len(s) + 2):
                    for kind in (COL_UNITS, COL_CHARS):
                        assert ref_pos_to_linecol(lines, start, p, kind) == (INVALID, INVALID)


def test_the_two_mappings_are_inverse_bijections():
    for s in texts():
        t = np.array([ord(c) for c in s], np.uint32)
        for enc in (UTF8, UTF16):
            _, start = ref_encode(t, enc)
            chars = len(t)
            for eol in (EOL_LF, EOL_ANY):
                lines = ref_lines(t, start, eol)
                n = len(lines)
                for kind in (COL_UNITS, COL_CHARS):
                    seen = {}
                    for line in range(n + 2):
                        ext = ref_extent(lines, start, line, kind) if line < n else 0
                        for col in range(ext + 3):
                            pos, mid = ref_linecol_to_pos(lines, start, line, col, kind)
                            valid = line < n and (col < ext or (line == n - 1 and col == ext))
                            if not valid:
                                assert (pos, mid) == (INVALID, 0)
                                continue
                            assert pos <= chars
                            back = ref_pos_to_linecol(lines, start, pos, kind)
                            # back at or before the column, and at it exactly when it starts a char
                            assert back[0] == line and back[1] <= col and (back[1] == col) == (mid == 0)
                            if kind == COL_CHARS:
                                assert mid == 0
                            if mid == 0:
                                assert pos not in seen
                                seen[pos] = (line, col)
                    # every position is the image of exactly one valid pair with mid == 0: its own
                    assert sorted(seen) == list(range(chars + 1))
                    for p in range(chars + 1):
                        assert seen[p] == ref_pos_to_linecol(lines, start, p, kind)
                    assert seen[chars][0] == n - 1  # the end-of-document cursor is on the last line


def test_whole_document_helpers_equal_the_one_query_functions():
    for s in texts():
        t = np.array([ord(c) for c in s], np.uint32)
        for enc in (UTF8, UTF16):
            _, start = ref_encode(t, enc)
            for eol in (EOL_LF, EOL_ANY):
                lines = ref_lines(t, start, eol)
                n = len(lines)
                for kind in (COL_UNITS, COL_CHARS):
                    gl, gc = ref_pos_to_linecol_all(lines, start, kind)
                    want = [ref_pos_to_linecol(lines, start, p, kind) for p in range(len(t) + 3)]
                    assert gl.dtype == gc.dtype == np.uint32
                    assert list(zip(gl.tolist(), gc.tolist())) == want
                    ql, qc, qp, qm = ref_linecol_to_pos_all(lines, start, kind)
                    pairs = [(line, col) for line in range(n + 2)
                             for col in range((ref_extent(lines, start, line, kind) if line < n else 0) + 3)]
                    assert list(zip(ql.tolist(), qc.tolist())) == pairs
                    want = [ref_linecol_to_pos(lines, start, line, col, kind) for line, col in pairs]
                    assert qp.dtype == np.uint32 and qm.dtype == np.uint8
                    assert list(zip(qp.tolist(), qm.tolist())) == want


def test_library_exports_the_line_entry_points():
    crdt_amd.build()
    lib = ctypes.CDLL(crdt_amd.LIB_PATH)
    for s in LINES_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in crdt_amd.EXPORTED_SYMBOLS, s
