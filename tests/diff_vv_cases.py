"""Hand-built histories and version vectors for the causal-version diff -- TEST INFRASTRUCTURE shared
by tests/test_diff_vv_ref.py (the shapes, on the oracle) and tests/test_gpu_diff_vv.py (the engine).

Histories are parsed txn lists (fuzz_gen.parse_wire's form, general_streams' helpers); vectors are
{agent name: seqs seen}, turned into arrays by `vector` with the replica's own agent ids.
"""
import numpy as np

from diff_vv_ref import ids_by_order, next_seqs
from general_streams import Author, R, dele, ins

DIFF2_LONG = 256  # kernels.h: spans with more orders are walked by the whole wave
DIFF_T = 256      # kernels.h: canonical spans per pass of the walk's loop


def neighbour_deletes():
    """A inserts 10 items; B deletes item 3, then C, who has seen B, deletes item 4: two txns of two
    agents whose delete ops have consecutive orders (10, 11) and consecutive targets, so the delete
    log holds them as ONE run (10, 3, 2).  A vector with C and without B holds the second order of
    that run and not the first."""
    return [("A", 0, [R], [ins(R, R, 10)]),
            ("B", 0, [("A", 9)], [dele(("A", 3))]),
            ("C", 0, [("B", 0)], [dele(("A", 4))])]


NEIGHBOUR_VECTORS = [{}, {"A": 10}, {"A": 10, "B": 1}, {"A": 10, "C": 1}, {"A": 10, "B": 1, "C": 1}, {"A": 4, "C": 1},
                     {"A": 5, "B": 1, "C": 1}, {"C": 1}]


def long_span():
    """X types 300 chars, Y types 300 on from X's last, X 100 on from Y's last: 700 contiguous orders,
    each item's origin_left the order before it -- one canonical span of three runs of two agents.
    Z then deletes X's items 10 .. 29 and W deletes Y's items 250 .. 254 (orders 550 .. 554), which
    leaves the visible span [30, 550): 520 orders, past DIFF2_LONG.  Vectors cut it at any order."""
    out = []
    x, y = Author("X", 0, out), Author("Y", 0, out)
    x.txn([ins(R, R, 300)], parents=[R])
    y.txn([ins(x.last(), R, 300)], parents=[x.last()])
    x.txn([ins(y.last(), R, 100)], parents=[y.last()])
    z = Author("Z", 0, out).txn([dele(("X", 10), 20)], parents=[x.last()])
    Author("W", 0, out).txn([dele(("Y", 250), 5)], parents=[z.last()])
    return out


LONG_VECTORS = [{}, {"X": 150}, {"X": 300, "Y": 100}, {"X": 350}, {"X": 400, "Y": 300, "Z": 7},
                {"X": 400, "Y": 300, "Z": 20, "W": 5}, {"X": 20, "Z": 20}, {"X": 33, "Y": 300, "W": 2},
                {"X": 400, "Y": 31, "Z": 20}, {"X": 289, "Y": 257, "W": 5}]


def many_spans(n=300):
    """P and Q take turns inserting one char at the start of the text: n items in the reverse of
    their orders, so n canonical spans, past DIFF_T; D then deletes one-item runs all over it.  A
    vector with other counts for P and Q is no order prefix, and its patches fall into both passes
    of the walk."""
    out = []
    prev = None
    seq = {"P": 0, "Q": 0}
    for k in range(n):
        a = "PQ"[k % 2]
        out.append((a, seq[a], [prev or R], [ins(R, prev or R, 1)]))
        prev = (a, seq[a])
        seq[a] += 1
    d = Author("D", 0, out)
    for j, t in enumerate([("P", 3), ("Q", 40), ("P", 41), ("Q", 100), ("P", 149), ("Q", 0)]):
        d.txn([dele(t)], parents=[prev] if j == 0 else None)
    return out


MANY_VECTORS = [{}, {"P": 100, "Q": 30}, {"P": 150, "Q": 150, "D": 2}, {"P": 150, "Q": 150, "D": 6}, {"P": 20, "Q": 150},
                {"P": 150}, {"Q": 149, "D": 6}, {"P": 131, "Q": 129, "D": 4}]


def vector(named: dict, ids: dict) -> np.ndarray:
    """{agent name: seqs} as an array over a replica's agent ids (ids: {name: id})"""
    out = np.zeros(len(ids), np.uint32)
    for name, x in named.items():
        out[ids[name]] = x
    return out


def cut_vectors(ex: dict, max_runs: int = 4):
    """the full vector, and it cut just below the orders 31, 32 and 33 and at the first, second, last
    and next seq of the longest client_with_order runs of two or more orders: vectors that end
    inside a run, on either side of a bitmap word, and on a run's edges"""
    full = next_seqs(ex).astype(np.uint32)
    agent, seq = ids_by_order(ex)
    out = [full]
    for x in (31, 32, 33):
        if x < int(ex["next_order"]):
            v = full.copy()
            v[agent[x]] = seq[x]
            out.append(v)
    cwo = np.asarray(ex["cwo"], dtype=np.int64).reshape(-1, 4)
    runs = cwo[cwo[:, 3] >= 2]
    for _key, a, s, ln in runs[np.argsort(-runs[:, 3], kind="stable")][:max_runs]:
        for cut in (s, s + 1, s + ln - 1, s + ln):
            v = full.copy()
            v[a] = cut
            out.append(v)
    return out


def random_vectors(ex: dict, rng, n: int):
    nxt = next_seqs(ex)
    return [rng.integers(0, nxt + 1).astype(np.uint32) for _ in range(n)]
