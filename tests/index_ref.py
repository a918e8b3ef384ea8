"""A plain numpy reference of the published index -- TEST INFRASTRUCTURE.

From the oracle's export()["raw"] and ["leaf_sizes"] only: the canonical spans (canon_of), the
visible prefix (vpos_of), the span-start bitmap with its word prefix and the spans by first order
(index_of), and what k_publish_big's boundary resolution meets on a document (big_ranges).  Plus the
seeded document generators that tests/test_index_ref.py (CPU: their coverage conditions) and
tests/test_gpu_index_edges.py (GPU: the index and the queries on them) share.  Every generator
returns one agent's local ops [(pos, del, ins), ...] as a u32 array, one op per txn."""
import functools
import random

import numpy as np

from kernel_consts import PUB_BIG_MIN, PUB_BIG_WAVES

LAYOUTS = {32: (32, 16), 4: (4, 8)}


def _cols(a):
    a = np.asarray(a, np.uint32).reshape(-1, 4)
    return a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), a[:, 2].astype(np.int64), a[:, 3].view(np.int32).astype(np.int64)


def appends(raw) -> np.ndarray:
    """app[i]: raw entry i appends to entry i - 1 (YjsSpan::can_append, span.rs:47-53); app[0] False"""
    order, ol, orr, ln = _cols(raw)
    app = np.zeros(order.shape[0], bool)
    end = order[:-1] + np.abs(ln[:-1])
    app[1:] = (end == order[1:]) & (ol[1:] == end - 1) & (orr[:-1] == orr[1:]) & ((ln[:-1] > 0) == (ln[1:] > 0))
    return app


def canon_of(raw) -> np.ndarray:
    """canonical spans [n, 4] u32 (order, origin_left, origin_right, signed len) of raw entries in
    document order: maximal runs of entries that append to their predecessor"""
    raw = np.asarray(raw, np.uint32).reshape(-1, 4)
    if not raw.shape[0]:
        return np.zeros((0, 4), np.uint32)
    st = np.flatnonzero(~appends(raw))
    out = raw[st].copy()
    out[:, 3] = np.add.reduceat(raw[:, 3].view(np.int32).astype(np.int64), st).astype(np.int32).view(np.uint32)
    return out


def vpos_of(canon) -> np.ndarray:
    """visible items before each canonical span: exclusive cumulative sum of the positive lengths"""
    ln = _cols(canon)[3]
    vis = np.where(ln > 0, ln, 0)
    return (np.cumsum(vis) - vis).astype(np.uint32)


def index_of(canon, next_order: int):
    """(bits, pre, sorted): the span-start bitmap over words [0, next_order / 32], the set bits
    before each word, and the span indices by first order"""
    order = _cols(canon)[0]
    nw = next_order // 32 + 1
    bits = np.zeros(nw, np.uint32)
    np.bitwise_or.at(bits, order >> 5, (np.uint32(1) << (order & 31).astype(np.uint32)))
    pc = np.unpackbits(bits.view(np.uint8)).reshape(nw, 32).sum(1).astype(np.int64)
    pre = (np.cumsum(pc) - pc).astype(np.uint32)
    return bits, pre, np.argsort(order, kind="stable").astype(np.uint32)


def span_of_order(canon, index, o: np.ndarray) -> np.ndarray:
    """the canonical span holding each order of `o` through the index alone (rank of the order in
    the bitmap -> sorted -> span), -1 where there is none: what loc -> pos does on the device"""
    bits, pre, srt = index
    order, _, _, ln = _cols(canon)
    o = np.asarray(o, np.int64)
    wd = np.minimum(o >> 5, bits.shape[0] - 1)
    mask = (np.uint64(0xFFFFFFFF) >> (np.uint64(31) - (o & 31).astype(np.uint64))).astype(np.uint32)
    below = bits[wd] & mask
    r = pre[wd].astype(np.int64) + np.unpackbits(below.view(np.uint8)).reshape(-1, 32).sum(1).astype(np.int64)
    ok = (o >> 5 < bits.shape[0]) & (r > 0)
    k = srt[np.where(ok, r - 1, 0)].astype(np.int64)
    ok &= (o - order[k] >= 0) & (o - order[k] < np.abs(ln[k]))
    return np.where(ok, k, -1)


def loc_to_pos_ref(ex: dict, agent: int, seq: np.ndarray, canon=None, index=None):
    """(pos, deleted) of (agent, seq) from an export: seq -> order through client_with_order's runs
    of the agent, order -> span through index_of, then vpos; (0xFFFFFFFF, 2) where unknown"""
    canon = canon_of(ex["raw"]) if canon is None else canon
    index = index_of(canon, ex["next_order"]) if index is None else index
    seq = np.asarray(seq, np.int64)
    cw = np.asarray(ex["cwo"], np.int64).reshape(-1, 4)
    cw = cw[cw[:, 1] == agent]
    cw = cw[np.argsort(cw[:, 2], kind="stable")]  # (key, agent, seq, len) runs of the agent by seq
    o = np.full(seq.shape, -1, np.int64)
    if cw.shape[0]:
        r = np.maximum(np.searchsorted(cw[:, 2], seq, side="right") - 1, 0)
        inside = (seq >= cw[r, 2]) & (seq < cw[r, 2] + cw[r, 3])
        o = np.where(inside, cw[r, 0] + seq - cw[r, 2], -1)
    k = np.where(o >= 0, span_of_order(canon, index, np.maximum(o, 0)), -1)
    order, _, _, ln = _cols(canon)
    vp = vpos_of(canon).astype(np.int64)
    kk = np.maximum(k, 0)
    pos = np.where(k >= 0, vp[kk] + np.where(ln[kk] > 0, o - order[kk], 0), 0xFFFFFFFF).astype(np.uint32)
    dl = np.where(k >= 0, (ln[kk] < 0).astype(np.uint8), 2).astype(np.uint8)
    return pos, dl


def pos_to_loc_ref(ex: dict, pos: np.ndarray, canon=None):
    """(agent, seq) of each visible position from an export: the last span whose vpos <= pos, its
    order through client_with_order; (0xFFFF, 0xFFFFFFFF) past the end"""
    canon = canon_of(ex["raw"]) if canon is None else canon
    pos = np.asarray(pos, np.int64)
    order = _cols(canon)[0]
    vp = vpos_of(canon).astype(np.int64)
    ok = (pos < ex["len"]) & (canon.shape[0] > 0)
    ag = np.full(pos.shape, 0xFFFF, np.uint16)
    sq = np.full(pos.shape, 0xFFFFFFFF, np.uint32)
    if ok.any():
        k = np.searchsorted(vp, pos[ok], side="right") - 1
        o = order[k] + pos[ok] - vp[k]
        cw = np.asarray(ex["cwo"], np.int64).reshape(-1, 4)  # (sorted by key = first order)
        r = np.searchsorted(cw[:, 0], o, side="right") - 1
        assert ((o >= cw[r, 0]) & (o < cw[r, 0] + cw[r, 3])).all()
        ag[ok] = cw[r, 1]
        sq[ok] = cw[r, 2] + o - cw[r, 0]
    return ag, sq


def big_ranges(leaf_sizes, raw) -> dict:
    """What k_publish_big's PUB_BIG_WAVES leaf ranges [n_leaves * w / W, n_leaves * (w + 1) / W) hold:
    merge[w - 1]: the span open at the end of range w - 1 continues into range w (w = 1 .. W - 1);
    single[w]: the whole range is one span; skip_write[w]: range w merges into its predecessor (its
    first span is skipped) and its first leaf starts a further span, which the same compaction step
    writes; n_leaves"""
    W = PUB_BIG_WAVES
    ls = np.asarray(leaf_sizes, np.int64)
    n = ls.shape[0]
    assert n >= W and (ls > 0).all()
    ent = np.concatenate([[0], np.cumsum(ls)])
    app = appends(raw)
    assert ent[-1] == app.shape[0]
    lo = [n * w // W for w in range(W + 1)]
    merge = np.array([bool(app[ent[lo[w]]]) for w in range(1, W)])
    single = np.array([bool(app[ent[lo[w]] + 1:ent[lo[w + 1]]].all()) for w in range(W)])
    skip_write = np.array([w > 0 and bool(merge[w - 1]) and not app[ent[lo[w]] + 1:ent[lo[w] + 1]].all() for w in range(W)])
    return dict(merge=merge, single=single, skip_write=skip_write, n_leaves=n)


def coverage(br: dict) -> dict:
    """the boundary-resolution cases one document's big_ranges() reaches"""
    m, s = br["merge"], br["single"]
    return dict(
        merging=bool(m.any()), non_merging=bool((~m).any()),
        # boundary w merges into a single range w whose end merges again: `extra` is carried through it
        chain_through_single=bool((m[:-1] & s[1:-1] & m[1:]).any()),
        # a merged-into range that closes its first span itself: lead_len comes from inside the range
        lead_closes_inside=bool((m & ~s[1:]).any()),
        skip_then_write=bool(br["skip_write"].any()),
        odd_leaf_count=br["n_leaves"] % PUB_BIG_WAVES != 0)


# ---- generators -----------------------------------------------------------------------------------
def _ops(lst) -> np.ndarray:
    return np.array(lst, np.uint32).reshape(-1, 3)


BIG_DELETES = {4: (300, 700, 1500), 32: (700, 3000, 6000, 12000)}
# seeds whose documents reach, per layout, every case of coverage() (tests/test_index_ref.py asserts
# it): of 48 leaf-32 seeds most merge at all 15 boundaries, since the long stretches hold most leaves
BIG_SEEDS = {4: tuple(range(8)), 32: (23, 27, 37)}


def big_family(seed: int, L: int) -> np.ndarray:
    """One insert, then left to right: keep a visible run of 1..8 chars, forward-delete the next d
    chars one op each (d in 1..4 with probability 0.97, else a long stretch from BIG_DELETES[L]),
    until the document has about 1.05 * PUB_BIG_MIN * L raw entries: every deleted char is an entry
    and every deleted stretch one canonical span, so spans of all lengths cross the leaf ranges."""
    rng = random.Random(1000 * L + seed)
    target = int(1.05 * PUB_BIG_MIN * L)
    runs, entries = [], 0
    while entries < target:
        r = rng.randint(1, 8)
        d = rng.randint(1, 4) if rng.random() < 0.97 else rng.choice(BIG_DELETES[L])
        runs.append((r, d))
        entries += d + 1
    n = sum(r + d for r, d in runs) + 3
    ops, p = [(0, 0, n)], 0
    for r, d in runs:
        p += r
        ops += [(p, 1, 0)] * d
    return _ops(ops)


def whole_run_deleted(n: int) -> np.ndarray:
    """a typed run forward-deleted char by char: n deleted entries, one canonical span"""
    return _ops([(0, 0, n)] + [(0, 1, 0)] * n)


def head_tail(n_del: int, head: int = 64) -> np.ndarray:
    """a visible head and tail around a middle of n_del chars deleted one by one, then a few chars typed at the end"""
    return _ops([(0, 0, n_del + 2 * head)] + [(head, 1, 0)] * n_del + [(2 * head, 0, 7)])


FIXED_N = {4: 8200, 32: 66000}  # deleted chars of the two fixed shapes: just past PUB_BIG_MIN leaves


def prepends(n: int) -> np.ndarray:
    """n single-char inserts at position 0: n raw entries, n canonical spans, orders descending"""
    p = np.zeros((n, 3), np.uint32)
    p[:, 2] = 1
    return p


@functools.lru_cache(maxsize=None)
def group_prepends() -> int:
    """prepends that give a leaf-4 document more than 64 * GROUP leaves: more than 64 groups at its
    root, whatever their fill, so compact_range's search for a range's first group takes a second pass"""
    from kernel_consts import GROUP
    n = 17000
    while oracle_doc(("prepends", n), 4).sizes()["leaves"] <= 64 * GROUP:
        n += 1000
    return n


def prepends_deleted(n: int, s: int, k: int) -> np.ndarray:
    """prepends(n), then the chars at positions [s, s + k) deleted one by one: their spans' orders
    descend, so they do not coalesce -- spans s .. s + k all have vpos s"""
    return np.concatenate([prepends(n), _ops([(s, 1, 0)] * k)])


def scattered(n0: int, k: int, seed: int) -> np.ndarray:
    """one insert of n0 chars, then k single-char inserts at random positions: about 2k + 1 spans
    whose first orders are spread over the whole order range; next_order = n0 + k"""
    rng = random.Random(seed)
    return _ops([(0, 0, n0)] + [(rng.randint(0, n0 + i), 0, 1) for i in range(k)])


@functools.lru_cache(maxsize=None)
def oracle_doc(key, L: int):
    """the oracle's replay of a generated document, computed once per (key, layout): key =
    ("big", seed) | ("whole",) | ("head_tail",) | ("prepends", n) | ("prepends_deleted", n, s, k) |
    ("scattered", n0, k, seed) | ("random", seed) | ("ops", bytes of a u32 [n, 3] array)"""
    from oracle_lib import OracleDoc
    ops = ops_of(key, L)
    o = OracleDoc(*LAYOUTS[L])
    assert o.apply_trace(o.agent("seph"), np.ones(ops.shape[0], np.uint32), ops) == 0
    return o


@functools.lru_cache(maxsize=None)
def ops_of(key, L: int) -> np.ndarray:
    kind = key[0]
    if kind == "big":
        return big_family(key[1], L)
    if kind == "whole":
        return whole_run_deleted(FIXED_N[L])
    if kind == "head_tail":
        return head_tail(FIXED_N[L])
    if kind == "prepends":
        return prepends(key[1])
    if kind == "prepends_deleted":
        return prepends_deleted(*key[1:])
    if kind == "scattered":
        return scattered(*key[1:])
    if kind == "random":
        return random_big(key[1], L)
    if kind == "ops":
        return np.frombuffer(key[1], np.uint32).reshape(-1, 3)
    raise KeyError(key)


def random_big(seed: int, L: int) -> np.ndarray:
    """fuzz_gen.random_local_trace grown until the oracle has at least PUB_BIG_MIN leaves"""
    from fuzz_gen import random_local_trace
    from oracle_lib import OracleDoc
    n = 3 * PUB_BIG_MIN * L // 2
    while True:
        c, p = random_local_trace(seed, n)
        o = OracleDoc(*LAYOUTS[L])
        assert o.apply_trace(o.agent("seph"), c, p) == 0
        if o.sizes()["leaves"] >= PUB_BIG_MIN:
            return p
        n += n // 4


@functools.lru_cache(maxsize=None)
def config5_big(seed: int, L: int):
    """(wire, oracle) of a fuzz_gen.config5_wire history (several agents, deletes that arrive out of
    order) grown until the oracle has at least PUB_BIG_MIN leaves"""
    from fuzz_gen import config5_wire
    from oracle_lib import OracleDoc
    rounds = 16
    while True:
        w = config5_wire(seed, base_len=1 << 16, n_agents=8, rounds=rounds, ops=8, hot=256, del_frac=0.5)
        o = OracleDoc(*LAYOUTS[L])
        assert o.apply_remote_wire(w) == 0
        if o.sizes()["leaves"] >= PUB_BIG_MIN:
            return w, o
        rounds += rounds // 2
