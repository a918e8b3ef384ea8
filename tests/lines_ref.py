"""Reference for the line index (include/crdt_gpu.h "line index"), written from the definition item
by item: a per-char walk over the UTF-32 text and the `start` array of encode_ref.ref_encode (the
unit offset of every char, start[chars] = units).  No str.split / re inside: those are what
tests/test_lines_ref.py checks this file against.

The *_all helpers give the answers to every query of a document as arrays (what the GPU tests
compare whole batches with); test_lines_ref.py checks them against the one-query functions.
"""
import numpy as np

EOL_LF, EOL_ANY = 0, 1          # CRDT_EOL_LF, CRDT_EOL_ANY
COL_UNITS, COL_CHARS = 0, 1     # CRDT_COL_UNITS, CRDT_COL_CHARS
INVALID = 0xFFFFFFFF
LF, CR = 0x0A, 0x0D


def ref_breaks(text_u32, eol: int) -> list:
    """the chars a break follows"""
    out = []
    n = len(text_u32)
    for p in range(n):
        c = int(text_u32[p])
        if c == LF:
            # a break follows every U+000A (both modes)
            out.append(p)
        elif c == CR and eol == EOL_ANY:
            # ... and every U+000D that is not immediately followed by U+000A in the same document:
            # CR LF is one break, after the LF; a CR that is the document's last char is a break
            if p + 1 == n or int(text_u32[p + 1]) != LF:
                out.append(p)
        # no other char breaks a line in either mode (U+000B, U+000C, U+0085, U+2028, U+2029 ...)
    return out


def ref_lines(text_u32, start, eol: int) -> np.ndarray:
    """the line starts [n_lines, 2] = (unit, pos): line 0 starts at unit 0, char 0; line k >= 1 at the
    unit and char after the k-th break.  n_lines = breaks + 1: an empty document has one (empty)
    line, a text that ends in a break an empty last line."""
    if eol not in (EOL_LF, EOL_ANY):
        raise ValueError(eol)
    rows = [(0, 0)]
    for p in ref_breaks(text_u32, eol):
        rows.append((int(start[p + 1]), p + 1))
    return np.array(rows, np.uint32).reshape(-1, 2)


def ref_extent(lines, start, line: int, kind: int) -> int:
    """from the line's start to the next line's start, its terminator included; for the last line to
    {units, chars}"""
    chars, units = len(start) - 1, int(start[-1])
    k = 0 if kind == COL_UNITS else 1
    end = int(lines[line + 1][k]) if line + 1 < len(lines) else (units, chars)[k]
    return end - int(lines[line][k])


def ref_pos_to_linecol(lines, start, pos: int, kind: int):
    """(line, col): for pos <= chars the last line whose start char is <= pos; col = pos - start.pos
    (chars) or (units before char pos) - start.unit (units).  pos == chars is the end-of-document
    cursor on the last line; pos > chars gives (0xFFFFFFFF, 0xFFFFFFFF)."""
    if kind not in (COL_UNITS, COL_CHARS):
        raise ValueError(kind)
    chars = len(start) - 1
    if pos > chars:
        return INVALID, INVALID
    line = 0
    while line + 1 < len(lines) and int(lines[line + 1][1]) <= pos:
        line += 1
    if kind == COL_CHARS:
        return line, pos - int(lines[line][1])
    return line, int(start[pos]) - int(lines[line][0])


def ref_linecol_to_pos(lines, start, line: int, col: int, kind: int):
    """(pos, mid): valid iff line < n_lines and col < the line's extent in that column kind; for the
    last line col == extent is valid too and gives chars.  Otherwise (0xFFFFFFFF, 0).  With unit
    columns a column that falls inside a char gives that char with mid = 1."""
    if kind not in (COL_UNITS, COL_CHARS):
        raise ValueError(kind)
    chars = len(start) - 1
    if line >= len(lines):
        return INVALID, 0
    ext = ref_extent(lines, start, line, kind)
    last = line + 1 == len(lines)
    if not (col < ext or (last and col == ext)):
        return INVALID, 0
    if kind == COL_CHARS:
        return int(lines[line][1]) + col, 0
    u = int(lines[line][0]) + col
    if u == int(start[-1]):
        return chars, 0
    pos = int(lines[line][1])  # the char whose encoding covers unit u: it lies on this line
    while not int(start[pos]) <= u < int(start[pos + 1]):
        pos += 1
    return pos, int(u != int(start[pos]))


# ---- every query of one document at once -------------------------------------------------------

def ref_pos_to_linecol_all(lines, start, kind: int):
    """ref_pos_to_linecol for every pos in [0, chars + 2]: (line, col) arrays"""
    chars = len(start) - 1
    pos = np.arange(chars + 1, dtype=np.int64)
    line = np.searchsorted(lines[:, 1].astype(np.int64), pos, side="right") - 1
    if kind == COL_CHARS:
        col = pos - lines[line, 1]
    else:
        col = np.asarray(start, np.int64)[pos] - lines[line, 0]
    pad = np.full(2, INVALID, np.uint32)
    return np.concatenate([line.astype(np.uint32), pad]), np.concatenate([col.astype(np.uint32), pad])


def ref_linecol_to_pos_all(lines, start, kind: int):
    """ref_linecol_to_pos for every line in [0, n_lines + 1] and every col in [0, extent + 2] (extent
    0 past the last line): (line, col, pos, mid) arrays"""
    chars, units = len(start) - 1, int(start[-1])
    n = len(lines)
    k = 0 if kind == COL_UNITS else 1
    first = np.concatenate([lines[:, k].astype(np.int64), [(units, chars)[k]]])
    ext = np.concatenate([np.diff(first), [0, 0]])             # per line in [0, n + 1]
    cnt = ext + 3
    line = np.repeat(np.arange(n + 2, dtype=np.int64), cnt)
    col = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ok = (line < n) & ((col < ext[line]) | ((line == n - 1) & (col == ext[line])))
    at = np.where(ok, first[np.minimum(line, n - 1)] + col, 0)  # the unit / the char, in the document
    if kind == COL_CHARS:
        pos, mid = at, np.zeros(len(at), np.uint8)
    else:
        # the char that covers each unit, and whether the unit is not its first (encode_ref.ref_units_to_pos_all)
        upos = np.zeros(units + 1, np.int64)
        umid = np.zeros(units + 1, np.uint8)
        st = np.asarray(start, np.int64)
        upos[st[:-1]] = 1
        umid[:units] = 1 - upos[:units]
        upos = np.cumsum(upos) - 1
        upos[units] = chars
        pos, mid = upos[at], umid[at]
    pos = np.where(ok, pos, INVALID).astype(np.uint32)
    mid = np.where(ok, mid, 0).astype(np.uint8)
    return line.astype(np.uint32), col.astype(np.uint32), pos, mid
