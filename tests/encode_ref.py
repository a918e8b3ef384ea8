"""Reference for the encoded text and its unit offsets (include/crdt_gpu.h "encoded text and unit
offsets"), written from the definition item by item.  No Python codec inside: the codecs are what
tests/test_encode_ref.py checks this file against.
"""
import numpy as np

UTF8, UTF16 = 0, 1          # CRDT_ENC_UTF8, CRDT_ENC_UTF16
INVALID = 0xFFFFFFFF
REPLACEMENT = 0xFFFD
# every value at which the width or the validity of a content value changes
BOUNDARY = [0, 0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xE000, 0xFFFD, 0xFFFF, 0x10000, 0x10FFFF]
NOT_SCALAR = [0xD800, 0xDFFF, 0x110000, 0xFFFFFFFF]


def scalar(c: int) -> int:
    """c if it is a Unicode scalar value, else U+FFFD"""
    return c if c < 0xD800 or 0xE000 <= c <= 0x10FFFF else REPLACEMENT


def encode_char(c: int, enc: int) -> list:
    """the units of content value c"""
    c = scalar(c)
    if enc == UTF8:
        if c < 0x80:
            return [c]
        if c < 0x800:
            return [0xC0 | (c >> 6), 0x80 | (c & 0x3F)]
        if c < 0x10000:
            return [0xE0 | (c >> 12), 0x80 | ((c >> 6) & 0x3F), 0x80 | (c & 0x3F)]
        return [0xF0 | (c >> 18), 0x80 | ((c >> 12) & 0x3F), 0x80 | ((c >> 6) & 0x3F), 0x80 | (c & 0x3F)]
    if enc == UTF16:
        if c < 0x10000:
            return [c]
        return [0xD800 + ((c - 0x10000) >> 10), 0xDC00 + ((c - 0x10000) & 0x3FF)]
    raise ValueError(enc)


def ref_encode(text_u32, enc: int):
    """(units: np.uint8 (UTF-8) or np.uint16 (UTF-16) array, start: the unit offset of every char,
    with start[chars] = units)"""
    units, start = [], []
    for c in text_u32:
        start.append(len(units))
        units += encode_char(int(c), enc)
    start.append(len(units))
    return np.array(units, np.uint8 if enc == UTF8 else np.uint16), np.array(start, np.uint32)


def ref_pos_to_units(start, pos: int) -> int:
    """units before char pos (pos == chars: units), 0xFFFFFFFF above chars"""
    chars = len(start) - 1
    return int(start[pos]) if pos <= chars else INVALID


def ref_units_to_pos(start, u: int):
    """(pos, mid): the char whose encoding covers unit u and whether u is not its first unit;
    u == units: (chars, 0); above: (0xFFFFFFFF, 0)"""
    chars, units = len(start) - 1, int(start[-1])
    if u > units:
        return INVALID, 0
    if u == units:
        return chars, 0
    pos = 0
    while not int(start[pos]) <= u < int(start[pos + 1]):
        pos += 1
    return pos, int(u != int(start[pos]))


def ref_units_to_pos_all(start):
    """ref_units_to_pos for every u in [0, units + 2], as arrays (pos, mid)"""
    chars, units = len(start) - 1, int(start[-1])
    pos = np.full(units + 3, INVALID, np.uint32)
    mid = np.zeros(units + 3, np.uint8)
    for p in range(chars):
        a, b = int(start[p]), int(start[p + 1])
        pos[a:b] = p
        mid[a + 1:b] = 1
    pos[units] = chars
    return pos, mid


def cycle_text(n: int) -> np.ndarray:
    """n chars whose UTF-8 widths cycle 1, 4, 2, 3 (UTF-16: 1, 2, 1, 1)"""
    return np.array([(0x41, 0x1F600, 0xE9, 0x20AC)[j % 4] for j in range(n)], np.uint32)
