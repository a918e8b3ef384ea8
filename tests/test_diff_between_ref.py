"""CPU checks of the two-version diff definition (tests/diff_between_ref.py) against the checkout
and diff definitions and the oracle's texts.

Content is np.arange(next_order), so a text is the list of its visible items' orders, ins_order is
the inserted content, and ref_checkout(ex, v) is the text at version v.  On the histories and cuts
of tests/test_diff_ref.py, for every ordered pair (a, b) of the sampled versions:
  the patches of (a, b) applied to the text at a give the text at b;
  (a, current version) is ref_diff(ex, a), array for array;
  (b, a) mirrors (a, b): as many patches, del_len and ins_len swapped;
  (a, a) is empty;
and at the txn boundaries the text at a is the oracle's text of the prefix replay.
"""
import numpy as np
import pytest

from checkout_ref import ref_checkout
from diff_between_ref import ref_diff_between, ref_diff_between_arrays
from diff_ref import apply_patches, ref_diff
from fuzz_gen import concurrent_wire, parse_wire
from test_diff_ref import LAYOUTS, double_delete_txns, micro_txns, replay


def same(x, y):
    return x[0].shape == y[0].shape and np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def check_pairs(ex, versions, between=ref_diff_between):
    """every ordered pair of `versions`; returns (patches seen, pairs a > b with deletes and inserts in one patch)"""
    n = int(ex["next_order"])
    texts = {v: ref_checkout(ex, v) for v in versions}
    res = {(a, b): between(ex, a, b) for a in versions for b in versions}
    n_pat = mixed = 0
    for (a, b), (pat, ins) in res.items():
        assert int(pat[:, 2].sum()) == ins.shape[0], (a, b)
        assert np.array_equal(apply_patches(texts[a], pat, ins), texts[b]), (a, b)
        back = res[(b, a)][0]
        assert back.shape == pat.shape, (a, b)
        assert np.array_equal(back[:, 1], pat[:, 2]) and np.array_equal(back[:, 2], pat[:, 1]), (a, b)
        if a == b:
            assert pat.shape[0] == 0 and ins.shape[0] == 0, a
        if b == n:
            assert same((pat, ins), ref_diff(ex, a)), a
        n_pat += pat.shape[0]
        mixed += int(a > b and ((pat[:, 1] > 0) & (pat[:, 2] > 0)).any())
    return n_pat, mixed


def boundary_versions(txns, cuts, layout, ex):
    """the versions after txns[:k] for k in cuts; at each the checkout is the oracle's text of the prefix replay"""
    content = np.arange(ex["next_order"], dtype=np.uint32)
    out = []
    for k in cuts:
        old = replay(txns[:k], layout)
        v = old.sizes()["next_order"]
        assert np.array_equal(ref_checkout(ex, v), old.text(content)[0]), (k, v)
        out.append(int(v))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", range(4))
def test_every_ordered_pair_of_the_sampled_versions(seed, layout):
    wire, n = concurrent_wire(seed)
    txns = parse_wire(wire)[1]
    ex = replay(txns, layout).export()
    vs = boundary_versions(txns, [0, 1, n // 3, n // 2, n - 1, n], layout, ex)
    # ... and versions inside txns: one past a boundary, one before the end
    vs = sorted(set(vs + [vs[2] + 1, vs[3] + 1, int(ex["next_order"]) - 1]))
    n_pat, mixed = check_pairs(ex, vs)
    assert n_pat > len(vs) and mixed > 0
    for a in vs:
        for b in vs:
            assert same(ref_diff_between_arrays(ex, a, b), ref_diff_between(ex, a, b)), (a, b)


@pytest.mark.parametrize("swap", [False, True])
def test_double_deletes(swap):
    txns = double_delete_txns()
    if swap:
        txns = [txns[0], txns[2], txns[1]]
    ex = replay(txns).export()
    assert ex["next_order"] == 18
    boundary_versions(txns, [0, 1, 2, 3], (32, 16), ex)
    assert check_pairs(ex, list(range(19)))[0] > 0
    for a in range(19):
        for b in range(19):
            assert same(ref_diff_between_arrays(ex, a, b), ref_diff_between(ex, a, b)), (a, b)
    if not swap:
        # B's delete [2, 6) is orders 10..13, C's [4, 8) is 14..17.  After B the text is 0 1 6 7 8 9;
        # back to before B: items 2..5 return at position 2
        p, ins = ref_diff_between(ex, 14, 10)
        assert p.tolist() == [[2, 0, 4, 0]] and ins.tolist() == [2, 3, 4, 5]
        # inside C's run (14, 15 applied: items 4, 5 deleted a second time, nothing visible changes)
        p, _ = ref_diff_between(ex, 14, 16)
        assert p.shape[0] == 0
        # from inside B's run (2, 3 gone) to inside C's run (6 gone too): 4 5 6 leave at position 2
        p, _ = ref_diff_between(ex, 12, 17)
        assert p.tolist() == [[2, 3, 0, 0]]


def test_micro_trace_between_its_cuts():
    txns = micro_txns("del1")
    ex = replay(txns).export()
    vs = boundary_versions(txns, [len(txns) // 2, 60000], (32, 16), ex) + [int(ex["next_order"])]
    n_pat, _ = check_pairs(ex, vs, ref_diff_between_arrays)
    assert n_pat > 4
    assert same(ref_diff_between_arrays(ex, vs[1], vs[0]), ref_diff_between(ex, vs[1], vs[0]))
