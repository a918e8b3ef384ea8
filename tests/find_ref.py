"""Reference for find (include/crdt_gpu.h "find"), written from the definition at the char level:
sanitise and fold the text and the pattern as uint32 arrays, compare the pattern's chars one by one
against the text shifted by their index, and look the unit offsets up in the `start` array of
encode_ref.ref_encode (the unit offset of every char, start[chars] = units).  Independent of the
encoding: no units are compared.  No re / str.find inside: those are what tests/test_find_ref.py
checks this file against.
"""
import numpy as np

FIND_EXACT, FIND_ASCII_ICASE = 0, 1   # CRDT_FIND_*
SEEK_NEXT, SEEK_PREV = 0, 1           # CRDT_SEEK_*
FIND_MAX_CHARS = 64                   # CRDT_FIND_MAX_CHARS
INVALID = 0xFFFFFFFF
REPLACEMENT = 0xFFFD


def code_points(x) -> np.ndarray:
    """a str (its code points by ord, lone surrogates included) or an array of values, as uint32"""
    if isinstance(x, str):
        x = [ord(c) for c in x]
    return np.asarray(x, dtype=np.uint32).reshape(-1)


def sanitise(a) -> np.ndarray:
    """each value as the encoder sanitises it: a surrogate or a value above 0x10FFFF is U+FFFD"""
    a = code_points(a).astype(np.int64)
    bad = ((a >= 0xD800) & (a <= 0xDFFF)) | (a > 0x10FFFF)
    return np.where(bad, REPLACEMENT, a)


def fold(a: np.ndarray, icase: bool) -> np.ndarray:
    """c + 0x20 for 0x41 <= c <= 0x5A with the case flag; nothing outside ASCII folds"""
    if not icase:
        return a
    return np.where((a >= 0x41) & (a <= 0x5A), a + 0x20, a)


def ref_find_pos(text_u32, pattern, icase: bool = False) -> np.ndarray:
    """every char position p with p + m <= chars and fold(T[p + j]) == fold(P[j]) for all j < m,
    ascending, overlapping matches included"""
    t = fold(sanitise(text_u32), icase)
    p = fold(sanitise(pattern), icase)
    m = len(p)
    if not 1 <= m <= FIND_MAX_CHARS:
        raise ValueError(m)
    n = len(t) - m + 1  # the positions with p + m <= chars
    if n <= 0:
        return np.zeros(0, np.uint32)  # an empty document, or one shorter than the pattern: 0 matches
    hit = np.ones(n, bool)
    for j in range(m):
        hit &= t[j:j + n] == p[j]
        if not hit.any():
            break
    return np.flatnonzero(hit).astype(np.uint32)


def ref_find(text_u32, start, pattern, icase: bool = False) -> np.ndarray:
    """the matches [n, 2] = (unit, pos): unit = the units before char pos in that encode"""
    pos = ref_find_pos(text_u32, pattern, icase)
    return np.stack([np.asarray(start, np.uint32)[pos], pos], axis=1).astype(np.uint32).reshape(-1, 2)


def ref_seek(matches, pos, direction: int) -> np.ndarray:
    """per pos[q]: the number of the first match with match.pos >= pos[q] (SEEK_NEXT) or of the last
    match with match.pos <= pos[q] (SEEK_PREV); 0xFFFFFFFF when there is none.  pos is not checked
    against the document's chars."""
    mp = np.asarray(matches, np.int64).reshape(-1, 2)[:, 1]
    q = np.asarray(pos, np.int64)
    if direction == SEEK_NEXT:
        k = np.searchsorted(mp, q, side="left")
        return np.where(k < len(mp), k, INVALID).astype(np.uint32)
    if direction == SEEK_PREV:
        k = np.searchsorted(mp, q, side="right") - 1
        return np.where(k >= 0, k, INVALID).astype(np.uint32)
    raise ValueError(direction)
