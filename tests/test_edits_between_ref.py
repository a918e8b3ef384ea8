"""CPU checks of the definition of the edits in units between two versions
(tests/edits_between_ref.py) against the checkout, edits and encode definitions, the oracle's texts
and Python's own codecs, and of the library's entry point being exported.

On the histories of tests/test_diff_between_ref.py, with mixed_content and in both encodings, for
every ordered pair (a, b) of the sampled versions (0, the version, versions inside txns, both sides
of a 32-order word):
  1. the edits of (a, b) applied to the encoding of the text at a give the encoding of the text at b
     (at the txn boundaries these are the oracle's texts of prefix replays);
  2. unit is ref_pos_to_units of pos on the encoding at b;
  3. (a, current version) is ref_edits(ex, a), array for array, pool included;
  4. (a, a) is empty;
  5. (b, a) mirrors (a, b): as many edits, del_* and ins_* swapped;
and the pool is Python's codec on content[ins_order], and the array form equals the item walk.
"""
import ctypes

import numpy as np
import pytest

import crdt_amd
from checkout_ref import ref_checkout
from diff_between_ref import ref_diff_between
from edits_between_ref import ref_edits_between, ref_edits_between_arrays
from edits_ref import apply_edits, mixed_content, ref_edits
from encode_ref import UTF8, UTF16, ref_encode, ref_pos_to_units
from fuzz_gen import concurrent_wire, parse_wire
from test_diff_ref import LAYOUTS, double_delete_txns, micro_txns, replay
from test_edits_ref import codec_units

ENCS = [UTF8, UTF16]


def same(x, y):
    return x[0].shape == y[0].shape and np.array_equal(x[0], y[0]) and x[1].dtype == y[1].dtype and np.array_equal(x[1], y[1])


def check_pairs(ex, versions, content, between=ref_edits_between, arrays=True):
    """the five properties on every ordered pair of `versions`, in both encodings; returns the edits seen"""
    n = int(ex["next_order"])
    n_edits = 0
    for enc in ENCS:
        enc_at = {v: ref_encode(content[ref_checkout(ex, v)], enc) for v in versions}
        res = {(a, b): between(ex, a, b, content, enc) for a in versions for b in versions}
        for (a, b), (ed, pool) in res.items():
            units, start = enc_at[b]
            got = apply_edits(enc_at[a][0], ed, pool)
            assert got.dtype == units.dtype and np.array_equal(got, units), (a, b, enc)                   # 1
            assert ed[:, 3].tolist() == [ref_pos_to_units(start, int(p)) for p in ed[:, 0]], (a, b, enc)  # 2
            if b == n:
                assert same((ed, pool), ref_edits(ex, a, content, enc)), (a, enc)                         # 3
            if a == b:
                assert ed.shape[0] == 0 and pool.shape[0] == 0, (a, enc)                                  # 4
            back = res[(b, a)][0]
            assert back.shape == ed.shape, (a, b, enc)                                                    # 5
            assert np.array_equal(back[:, [1, 4]], ed[:, [2, 5]]) and np.array_equal(back[:, [2, 5]], ed[:, [1, 4]]), (a, b, enc)
            # the pool is the codec's encoding of the inserted items, and ins_off walks it
            ins_order = ref_diff_between(ex, a, b)[1]
            assert np.array_equal(pool, codec_units(content[ins_order], enc)), (a, b, enc)
            assert ed[:, 6].tolist() == (np.cumsum(ed[:, 5]) - ed[:, 5]).tolist() and not ed[:, 7].any()
            assert int(ed[:, 5].sum()) == pool.shape[0]
            if arrays:
                assert same(ref_edits_between_arrays(ex, a, b, content, enc), (ed, pool)), (a, b, enc)
            n_edits += ed.shape[0]
    return n_edits


def boundary_versions(txns, cuts, layout, ex, content):
    """the versions after txns[:k] for k in cuts; at each the checkout's text is the oracle's text of the prefix replay"""
    out = []
    for k in cuts:
        old = replay(txns[:k], layout)
        v = old.sizes()["next_order"]
        assert np.array_equal(content[ref_checkout(ex, v)], old.text(content)[0]), (k, v)
        out.append(int(v))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", range(4))
def test_every_ordered_pair_of_the_sampled_versions(seed, layout):
    wire, n = concurrent_wire(seed)
    txns = parse_wire(wire)[1]
    ex = replay(txns, layout).export()
    no = int(ex["next_order"])
    content = mixed_content(no, seed)
    vs = boundary_versions(txns, [0, 1, n // 3, n // 2, n - 1, n], layout, ex, content)
    # ... versions inside txns and both sides of a 32-order word
    vs = sorted(set(vs + [vs[2] + 1, vs[3] + 1, no - 1, 31, 32, 33]))
    assert vs[0] == 0 and vs[-1] == no and no > 33
    assert check_pairs(ex, vs, content) > len(vs)


@pytest.mark.parametrize("swap", [False, True])
def test_double_deletes(swap):
    txns = double_delete_txns()
    if swap:
        txns = [txns[0], txns[2], txns[1]]
    ex = replay(txns).export()
    assert ex["next_order"] == 18
    content = mixed_content(18, 5)
    boundary_versions(txns, [0, 1, 2, 3], (32, 16), ex, content)
    assert check_pairs(ex, list(range(19)), content) > 0
    if not swap:
        w = {enc: [len(ref_encode(content[x:x + 1], enc)[0]) for x in range(18)] for enc in ENCS}
        for enc in ENCS:
            # after B the text is 0 1 6 7 8 9; back to before B: items 2..5 return at position 2
            ed, pool = ref_edits_between(ex, 14, 10, content, enc)
            iu = sum(w[enc][2:6])
            assert ed.tolist() == [[2, 0, 4, w[enc][0] + w[enc][1], 0, iu, 0, 0]] and pool.shape[0] == iu
            # from inside B's run (2, 3 gone) to inside C's run (6 gone too): 4 5 6 leave at position 2
            ed, pool = ref_edits_between(ex, 12, 17, content, enc)
            assert ed.tolist() == [[2, 3, 0, w[enc][0] + w[enc][1], sum(w[enc][4:7]), 0, 0, 0]] and pool.shape[0] == 0


def test_micro_trace_between_its_cuts():
    txns = micro_txns("del1")
    ex = replay(txns).export()
    content = mixed_content(int(ex["next_order"]), 2)
    vs = boundary_versions(txns, [len(txns) // 2, 60000], (32, 16), ex, content) + [int(ex["next_order"])]
    assert check_pairs(ex, vs, content, ref_edits_between_arrays, arrays=False) > 4
    for enc in ENCS:
        assert same(ref_edits_between_arrays(ex, vs[1], vs[0], content, enc), ref_edits_between(ex, vs[1], vs[0], content, enc))


def test_library_exports_the_entry_point():
    crdt_amd.build()
    lib = ctypes.CDLL(crdt_amd.LIB_PATH)
    assert hasattr(lib, "crdt_edits_between_async")
    assert "crdt_edits_between_async" in crdt_amd.EXPORTED_SYMBOLS
    assert hasattr(crdt_amd.Engine, "edits_between_async") and hasattr(crdt_amd.Engine, "edits_between")
