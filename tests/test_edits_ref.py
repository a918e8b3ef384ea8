"""CPU checks of the definition of the text edits in units (tests/edits_ref.py) against the oracle's
texts of prefix replays, the diff reference, the encode reference and Python's own codecs, and of
the library's edits entry points being exported.

ref_edits(export of the full replay, v, content, enc) applied to the encoding of the oracle's text
of a prefix replay that ends at version v must give the encoding of the oracle's text of the full
replay.
"""
import ctypes

import numpy as np
import pytest

import crdt_amd
from diff_ref import ref_diff
from edits_ref import apply_edits, mixed_content, ref_edits
from encode_ref import UTF8, UTF16, ref_encode, ref_pos_to_units, scalar
from fuzz_gen import concurrent_wire, parse_wire
from test_diff_ref import LAYOUTS, double_delete_txns, micro_txns, replay

EDITS_SYMBOLS = ["crdt_edits_async", "crdt_edits_counts", "crdt_edits_read", "crdt_last_edits_ms"]
ENCS = [UTF8, UTF16]


def codec_units(values, enc):
    """Python's codec on the values, one that is no scalar value replaced by U+FFFD first"""
    s = "".join(chr(scalar(int(c))) for c in values)
    if enc == UTF8:
        return np.frombuffer(s.encode("utf-8"), np.uint8)
    return np.frombuffer(s.encode("utf-16-le"), "<u2").astype(np.uint16)


def check_cuts(txns, cuts, layout=(32, 16), seed=0):
    """the four properties of the definition at every cut, in both encodings; returns the number
    of edits seen"""
    full = replay(txns, layout)
    ex = full.export()
    content = mixed_content(ex["next_order"], seed)
    new_text = full.text(content)[0]
    n_edits = 0
    for k in cuts:
        old = replay(txns[:k], layout)
        v = old.sizes()["next_order"]
        old_text = old.text(content)[0]
        patches, ins_order = ref_diff(ex, v)
        for enc in ENCS:
            edits, pool = ref_edits(ex, v, content, enc)
            new_units, start = ref_encode(new_text, enc)
            # applied to the encoded old text they give the encoded new text
            got = apply_edits(ref_encode(old_text, enc)[0], edits, pool)
            assert got.dtype == new_units.dtype and np.array_equal(got, new_units), (k, v, enc)
            # the item columns are the diff's
            assert edits.shape[0] == patches.shape[0] and np.array_equal(edits[:, :3], patches[:, :3]), (k, v, enc)
            assert not edits[:, 7].any()
            # unit is the unit offset of pos in the new text
            assert edits[:, 3].tolist() == [ref_pos_to_units(start, int(p)) for p in edits[:, 0]], (k, v, enc)
            # the pool is the codec's encoding of the inserted items, and ins_off walks it
            assert np.array_equal(pool, codec_units(content[ins_order], enc)), (k, v, enc)
            assert edits[:, 6].tolist() == (np.cumsum(edits[:, 5]) - edits[:, 5]).tolist()
            assert int(edits[:, 5].sum()) == pool.shape[0]
            n_edits += edits.shape[0]
    return n_edits


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", range(4))
def test_reference_against_oracle_texts(seed, layout):
    # the 48 concurrent cases of test_diff_ref.py: 4 histories x 6 cuts x 2 layouts
    wire, n = concurrent_wire(seed)
    txns = parse_wire(wire)[1]
    assert len(txns) == n
    assert check_cuts(txns, [0, 1, n // 3, n // 2, n - 1, n], layout, seed) > 0


def test_reference_double_deletes():
    txns = double_delete_txns()
    assert check_cuts(txns, [0, 1, 2, 3]) == 2 * 3  # (three patches, in each encoding)
    assert check_cuts([txns[0], txns[2], txns[1]], [0, 1, 2, 3], seed=1) == 2 * 3
    # deleted units are counted once, from the content of the deleted orders: after B only the old
    # text is 0 1 6 7 8 9 and C's delete takes items 6 and 7
    ex = replay(txns).export()
    content = mixed_content(18, 5)
    for enc in ENCS:
        edits, pool = ref_edits(ex, 14, content, enc)
        w = [len(ref_encode(content[x:x + 1], enc)[0]) for x in range(18)]
        assert edits.tolist() == [[2, 2, 0, w[0] + w[1], w[6] + w[7], 0, 0, 0]] and pool.shape[0] == 0


def test_reference_micro_trace_cut_at_half():
    txns = micro_txns("del1")
    assert check_cuts(txns, [len(txns) // 2, 60000], seed=2) > 2


def test_library_exports_the_edits_entry_points():
    crdt_amd.build()
    lib = ctypes.CDLL(crdt_amd.LIB_PATH)
    for s in EDITS_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in crdt_amd.EXPORTED_SYMBOLS, s
