"""The published index (canon, vpos, corder, sorted, the span-start bitmap and its word prefix) and
the three query-kernel families on it, at every size threshold that picks a code path
(tests/kernel_consts.py reads them from the sources), either side, exact against the oracle.

Every case asserts that it reached the path it names: through Engine.publish_plan() (which
publisher the host planned) or through the counts it just read (canon_counts, exported
client_with_order rows, versions, the oracle's leaf count)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from fuzz_gen import concurrent_wire, config5_wire  # noqa: E402
from kernel_consts import (GROUP, PUB_BIG_FEW_DOCS, PUB_BIG_MAX, PUB_BIG_MIN, PUBX_MAX_WORDS, QBLK_CWO, QBLK_MAX,  # noqa: E402
                           QBLK_Q, QBLK_W, QM_TILE)
from oracle_lib import OracleDoc  # noqa: E402
import index_ref as R  # noqa: E402

NOT_FOUND = (0xFFFF, 0xFFFFFFFF)
SAMPLE_ABOVE = 100_000  # orders above which a document's queries are sampled (still exact)
N_SAMPLES = 16384
MODES = ("lds", "per_thread", "merge")


def oracle_for(ops, L):
    return R.oracle_doc(("ops", np.ascontiguousarray(ops, np.uint32).tobytes()), L)


def engine_with(n_docs, L, local=None, wires=None):
    """an engine whose documents `local` {doc: ops of agent "seph", one op per txn} and `wires`
    {doc: remote wire} are replayed; every other document stays empty"""
    e = crdt_amd.Engine(n_docs, L)
    if local:
        docs = sorted(local)
        ag = e.agent_intern(docs, ["seph"] * len(docs))
        ops = [np.asarray(local[d], np.uint32).reshape(-1, 3) for d in docs]
        off = np.concatenate([[0], np.cumsum([o.shape[0] for o in ops])])
        tx = np.concatenate([np.stack([np.full(o.shape[0], a, np.uint32), np.ones(o.shape[0], np.uint32)], 1)
                             for a, o in zip(ag, ops)])
        st = e.apply_local_arrays(docs, off, tx, np.concatenate(ops))
        assert (st == 0).all(), st
    if wires:
        docs = sorted(wires)
        assert (e.apply_remote_wire(docs, [wires[d] for d in docs]) == 0).all()
    return e


def positions_of(ln, next_order, rng):
    if next_order <= SAMPLE_ABOVE:
        return np.arange(ln + 2, dtype=np.uint32)
    return np.concatenate([rng.integers(0, ln + 2, N_SAMPLES), [0, max(ln - 1, 0), ln, ln + 1]]).astype(np.uint32)


def edge_orders(next_order):
    """every order o with o & 31 in {0, 31} in the first and last 64 bitmap words, next_order - 1, next_order"""
    nw = next_order // 32 + 1
    w = np.unique(np.concatenate([np.arange(min(64, nw)), np.arange(max(nw - 64, 0), nw)]))
    o = np.concatenate([32 * w, 32 * w + 31, [max(next_order - 1, 0), next_order]])
    return np.unique(o[o <= next_order])


def locs_of(ex, n_agents, rng):
    """(agent, seq) queries: every seq 0 .. next_order of every agent, or for long documents the
    locations of edge_orders(), N_SAMPLES random ones and one past each agent's range"""
    no = ex["next_order"]
    if no <= SAMPLE_ABOVE:
        seq = np.tile(np.arange(no + 1, dtype=np.uint32), n_agents)
        return np.repeat(np.arange(n_agents, dtype=np.uint16), no + 1), seq
    cw = ex["cwo"].astype(np.int64)  # (key, agent, seq, len), by key
    o = edge_orders(no)
    r = np.maximum(np.searchsorted(cw[:, 0], o, side="right") - 1, 0)
    inside = (o >= cw[r, 0]) & (o < cw[r, 0] + cw[r, 3])
    ag = np.concatenate([cw[r, 1][inside], rng.integers(0, n_agents, N_SAMPLES), np.arange(n_agents)])
    sq = np.concatenate([(cw[r, 2] + o - cw[r, 0])[inside], rng.integers(0, no + 1, N_SAMPLES), np.full(n_agents, no)])
    return ag.astype(np.uint16), sq.astype(np.uint32)


def query_errors(e, d, o, ex=None, modes=MODES, seed=5):
    """pos -> loc and loc -> pos of document d against the oracle, exact: under "lds" and
    "per_thread" as asked, under "merge" the positions ascending.  Returns one line per (mode,
    direction) that differs, with its first differing query: a wrong index shows in every part it
    reaches, not only in the first one compared."""
    ex = o.export() if ex is None else ex
    rng = np.random.default_rng(seed)
    pos = positions_of(ex["len"], ex["next_order"], rng)
    oa, os_ = o.pos_to_loc(pos)
    ag, sq = locs_of(ex, o.sizes()["agents"], rng)
    op, od = o.loc_to_pos(ag, sq)
    srt = np.argsort(pos, kind="stable")
    errs = []
    try:
        for mode in modes:
            e.query_kernel(mode)
            p, wa, ws = (pos[srt], oa[srt], os_[srt]) if mode == "merge" else (pos, oa, os_)
            ga, gs = e.pos_to_loc(np.full(p.shape, d, np.uint32), p)
            bad = np.flatnonzero((ga != wa) | (gs != ws))
            if bad.size:
                i = bad[0]
                errs.append(f"{mode} pos_to_loc doc {d}: {bad.size} differ, first pos {p[i]}: ({ga[i]}, {gs[i]}) != ({wa[i]}, {ws[i]})")
            if mode == "merge":
                continue  # (loc -> pos under "merge" is the per-thread kernel)
            gp, gd = e.loc_to_pos(np.full(sq.shape, d, np.uint32), ag, sq)
            bad = np.flatnonzero((gd != od) | ((od != 2) & (gp != op)))
            if bad.size:
                i = bad[0]
                errs.append(f"{mode} loc_to_pos doc {d}: {bad.size} differ, first ({ag[i]}, {sq[i]}): ({gp[i]}, {gd[i]}) != ({op[i]}, {od[i]})")
    finally:
        e.query_kernel("lds")
    return errs


def check_index(e, d, o, modes=MODES):
    """the published index of document d and every query on it against the oracle, exact; every
    part is compared before the first difference fails the test"""
    ex = o.export()
    g = e.export(d)
    errs = []
    if g["canon"].shape != ex["canon"].shape:
        errs.append(f"canon doc {d}: {g['canon'].shape[0]} spans != {ex['canon'].shape[0]}")
    else:
        bad = np.flatnonzero((g["canon"] != ex["canon"]).any(1))
        if bad.size:
            errs.append(f"canon doc {d}: {bad.size} spans differ, first {bad[0]}: {g['canon'][bad[0]]} != {ex['canon'][bad[0]]}")
    if not np.array_equal(e.debug_vpos(d), R.vpos_of(ex["canon"])):
        errs.append(f"vpos doc {d}")
    if (int(e.lens([d])[0]), int(e.canon_counts()[d]), int(e.versions([d])[0])) != (len(o), ex["canon"].shape[0], ex["next_order"]):
        errs.append(f"len / canon_counts / version doc {d}")
    if int(e.digests()[d]) != o.digest():
        errs.append(f"digest doc {d}")
    errs += query_errors(e, d, o, ex, modes)
    assert not errs, errs


def check_empty(e, docs):
    """empty neighbours: length 0, and every query on them answers "not found" """
    docs = np.asarray(docs, np.uint32)
    assert (e.lens(docs) == 0).all()
    d = np.repeat(docs, 3)
    try:
        for mode in MODES:
            e.query_kernel(mode)
            ga, gs = e.pos_to_loc(d, np.tile(np.array([0, 1, 7], np.uint32), docs.shape[0]))
            assert (ga == NOT_FOUND[0]).all() and (gs == NOT_FOUND[1]).all(), mode
            gp, gd = e.loc_to_pos(d, np.zeros(d.shape, np.uint16), np.tile(np.array([0, 1, 7], np.uint32), docs.shape[0]))
            assert (gd == 2).all(), mode
    finally:
        e.query_kernel("lds")


def few_docs_engine(L, ops, n_docs=2):
    """document 0 of a small batch: past PUB_BIG_MIN leaves it publishes with k_publish_big"""
    return engine_with(n_docs, L, {0: ops})


MANY = PUB_BIG_FEW_DOCS + 1
MANY_AT = 517  # where the one real document of a MANY-document engine sits


# ---- A. each publisher, same document, both layouts ------------------------------------------------
@pytest.mark.parametrize("L", [32, 4])
def test_same_document_through_both_publishers(L):
    key = ("big", R.BIG_SEEDS[L][0])
    o = R.oracle_doc(key, L)
    assert PUB_BIG_MIN <= o.sizes()["leaves"] < PUB_BIG_MAX
    e = few_docs_engine(L, R.ops_of(key, L))
    plan, _ = e.publish_plan()
    assert list(plan) == [2, 0]  # k_publish_big; the empty neighbour stays with k_publish + k_pub_index
    check_index(e, 0, o)
    check_empty(e, [1])
    canon_big, vpos_big = e.export(0)["canon"], e.debug_vpos(0)
    e.close()
    e = engine_with(MANY, L, {MANY_AT: R.ops_of(key, L)})
    plan, _ = e.publish_plan()
    assert (plan == 0).all()  # more than PUB_BIG_FEW_DOCS documents: one wave, k_publish + k_pub_index
    check_index(e, MANY_AT, o)
    check_empty(e, [0, MANY_AT - 1, MANY_AT + 1, MANY - 1])
    assert np.array_equal(e.export(MANY_AT)["canon"], canon_big) and np.array_equal(e.debug_vpos(MANY_AT), vpos_big)


def test_index_built_in_the_publishing_wave():
    # plan 1: a bitmap past PUBX_MAX_WORDS words is built by publish_index<1> inside k_publish's wave,
    # beside a small document whose index k_pub_index builds in LDS; about 4,000 spans whose first
    # orders are spread over the whole bitmap
    ops = [R.scattered(600_000, 2000, 31), R.prepends(50)]
    orc = [oracle_for(p, 32) for p in ops]
    assert all(o.sizes()["leaves"] < PUB_BIG_MIN for o in orc)
    assert orc[0].sizes()["canon"] > 3500
    e = engine_with(2, 32, {0: ops[0], 1: ops[1]})
    plan, words = e.publish_plan()
    assert list(plan) == [1, 0] and words[0] > PUBX_MAX_WORDS >= words[1], (plan, words)
    o0 = np.sort(orc[0].export()["canon"][:, 0])
    assert (np.histogram(o0, bins=64, range=(0, 602_000))[0] > 0).all()  # (first orders over the whole bitmap)
    for d in (0, 1):
        check_index(e, d, orc[d])


@pytest.mark.parametrize("publisher", ["k_publish_big", "k_publish"])
def test_more_than_64_groups(publisher):
    # leaf-4 prepends past 64 * GROUP leaves: the root has more than 64 groups, so compact_range's
    # search for the group holding a range's first leaf takes a second 64-group pass (k_publish_big:
    # most ranges start past group 64; k_publish walks all groups from the first)
    n = R.group_prepends()
    o = R.oracle_doc(("prepends", n), 4)
    assert 64 * GROUP < o.sizes()["leaves"] < PUB_BIG_MAX
    big = publisher == "k_publish_big"
    d = 0 if big else MANY_AT
    e = engine_with(2 if big else MANY, 4, {d: R.prepends(n)})
    assert int(e.publish_plan()[0][d]) == (2 if big else 0)
    assert int(e.canon_counts()[d]) == n
    check_index(e, d, o)


# ---- B. k_publish_big boundary resolution -----------------------------------------------------------
@pytest.mark.parametrize("L,seed", [(L, s) for L in (4, 32) for s in R.BIG_SEEDS[L]])
def test_big_family(L, seed):
    # (which boundary cases the family reaches -- merging and not, `extra` carried through a single
    # range, lead_len from a span closed inside the range, a skipped first span with further spans in
    # the same step, a leaf count not divisible by 16 -- is asserted in tests/test_index_ref.py)
    o = R.oracle_doc(("big", seed), L)
    assert PUB_BIG_MIN <= o.sizes()["leaves"] < PUB_BIG_MAX
    e = few_docs_engine(L, R.ops_of(("big", seed), L), n_docs=1)
    assert list(e.publish_plan()[0]) == [2]
    check_index(e, 0, o)


@pytest.mark.parametrize("L", [32, 4])
def test_big_fixed_shapes(L):
    keys = [("whole",), ("head_tail",)]
    orc = [R.oracle_doc(k, L) for k in keys]
    assert all(o.sizes()["leaves"] >= PUB_BIG_MIN for o in orc)
    e = engine_with(2, L, {d: R.ops_of(k, L) for d, k in enumerate(keys)})
    assert list(e.publish_plan()[0]) == [2, 2]
    assert list(e.canon_counts()) == [1, 4]
    for d in (0, 1):
        check_index(e, d, orc[d])


def test_big_general_editing():
    # leaf 4, past PUB_BIG_MIN leaves: two generated-edit documents and one concurrent, deletion-heavy
    # history of several agents (deletes that arrive out of order, double deletes)
    orc = [R.oracle_doc(("random", s), 4) for s in (0, 1)]
    w, oc = R.config5_big(0, 4)
    orc.append(oc)
    assert all(PUB_BIG_MIN <= o.sizes()["leaves"] < PUB_BIG_MAX for o in orc)
    e = engine_with(3, 4, {s: R.ops_of(("random", s), 4) for s in (0, 1)}, {2: w})
    assert list(e.publish_plan()[0]) == [2, 2, 2]
    for d in range(3):
        check_index(e, d, orc[d])


# ---- C. query-kernel thresholds, either side ---------------------------------------------------------
def check_every_position(e, d, o, mode):
    pos = np.arange(len(o) + 2, dtype=np.uint32)
    e.query_kernel(mode)
    try:
        ga, gs = e.pos_to_loc(np.full(pos.shape, d, np.uint32), pos)
    finally:
        e.query_kernel("lds")
    oa, os_ = o.pos_to_loc(pos)
    bad = np.flatnonzero((ga != oa) | (gs != os_))
    assert not bad.size, (mode, d, int(pos[bad[0]]), (int(ga[bad[0]]), int(gs[bad[0]])), (int(oa[bad[0]]), int(os_[bad[0]])))


def test_qblk_max_spans_either_side():
    # single-char prepends: every item its own span.  QBLK_MAX - 1 and QBLK_MAX spans search vpos
    # staged in LDS, QBLK_MAX + 1 per thread in HBM; every position of each, each in batches of its own
    ns = [QBLK_MAX - 1, QBLK_MAX, QBLK_MAX + 1]
    e = engine_with(3, 32, {d: R.prepends(n) for d, n in enumerate(ns)})
    assert list(e.canon_counts()) == ns
    for d, n in enumerate(ns):
        o = R.oracle_doc(("prepends", n), 32)
        assert o.sizes()["canon"] == n
        for mode in ("lds", "per_thread"):
            check_every_position(e, d, o, mode)
    e.close()
    n = QBLK_MAX + 1
    e = engine_with(1, 4, {0: R.prepends(n)})
    assert list(e.canon_counts()) == [n]
    for mode in ("merge", "lds"):
        check_every_position(e, 0, R.oracle_doc(("prepends", n), 4), mode)


SWEEP_CN = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097)


@functools.lru_cache(maxsize=None)
def sweep_engine():
    return engine_with(len(SWEEP_CN), 32, {d: R.prepends(n) for d, n in enumerate(SWEEP_CN)})


@pytest.mark.parametrize("mode", MODES)
def test_search_over_every_span_count(mode):
    # the lockstep search's halving sequence (for (n = cn; n > 1; n -= n >> 1)) depends on cn alone:
    # powers of two and their neighbours, and under "merge" span counts around and past QM_TILE
    e = sweep_engine()
    assert list(e.canon_counts()) == list(SWEEP_CN)
    assert sum(cn > QM_TILE for cn in SWEEP_CN) >= 2 and QM_TILE - 1 in SWEEP_CN and QM_TILE in SWEEP_CN
    for d, cn in enumerate(SWEEP_CN):
        check_every_position(e, d, R.oracle_doc(("prepends", cn), 32), mode)


def test_equal_vpos_at_a_tile_edge():
    # a stretch of deleted spans (all with the vpos of the visible span after them) across, from and
    # up to a QM_TILE boundary of vpos; positions around it, each ten times, in sorted chunks
    n = QM_TILE + 100
    stretches = [(QM_TILE - 1, 3), (QM_TILE, 5), (QM_TILE - 3, 3)]
    e = engine_with(len(stretches), 32, {d: R.prepends_deleted(n, s, k) for d, (s, k) in enumerate(stretches)})
    assert list(e.canon_counts()) == [n] * len(stretches)  # (deleted in descending order: nothing coalesces)
    for d, (s, k) in enumerate(stretches):
        o = R.oracle_doc(("prepends_deleted", n, s, k), 32)
        vp = e.debug_vpos(d)
        assert (vp[s:s + k + 1] == s).all() and vp[s - 1] == s - 1 and vp[s + k + 1] == s + 1
        near = np.repeat(np.arange(s - 3, s + 4, dtype=np.uint32), 10)
        pos = np.sort(np.concatenate([np.arange(len(o) + 2, dtype=np.uint32), near]))
        assert pos.shape[0] < QBLK_Q  # (one sorted chunk)
        oa, os_ = o.pos_to_loc(pos)
        for mode in MODES:
            e.query_kernel(mode)
            ga, gs = e.pos_to_loc(np.full(pos.shape, d, np.uint32), pos)
            assert np.array_equal(ga, oa) and np.array_equal(gs, os_), (mode, d)
            # ... and in a batch of several sorted chunks, the stretch's positions opening a chunk
            rep = np.sort(np.concatenate([np.repeat(pos, 3), np.full(QBLK_Q, s, np.uint32)]))
            ga, gs = e.pos_to_loc(np.full(rep.shape, d, np.uint32), rep)
            wa, ws = o.pos_to_loc(rep)
            assert np.array_equal(ga, wa) and np.array_equal(gs, ws), (mode, d)
        e.query_kernel("lds")
        check_index(e, d, o)


def test_qblk_cwo_runs_either_side():
    # two agents alternately type one char at the end: one client_with_order run per txn (QBLK_CWO
    # runs are staged in LDS with vpos, QBLK_CWO + 1 stay in HBM) and a single canonical span
    ns = [QBLK_CWO, QBLK_CWO + 1]
    e = crdt_amd.Engine(2, 32)
    ag = e.agent_intern([0, 0, 1, 1], ["ann", "bob", "ann", "bob"]).reshape(2, 2)
    st = e.apply_local([(d, [(int(ag[d][i & 1]), [(i, 0, 1)]) for i in range(n)]) for d, n in enumerate(ns)])
    assert (st == 0).all()
    for d, n in enumerate(ns):
        o = OracleDoc(32, 16)
        oag = [o.agent("ann"), o.agent("bob")]
        for i in range(n):
            assert o.apply_local(oag[i & 1], [(i, 0, 1)]) == 0
        assert o.sizes()["cwo"] == n and o.sizes()["canon"] == 1
        assert e.export(d)["cwo"].shape[0] == n and int(e.canon_counts()[d]) == 1
        check_index(e, d, o)
        for mode in MODES:
            e.query_kernel(mode)
            ga, gs = e.pos_to_loc(np.full(n, d, np.uint32), np.arange(n, dtype=np.uint32))
            assert np.array_equal(ga, np.array(oag, np.uint16)[np.arange(n) & 1]), mode  # the agents alternate
            assert np.array_equal(gs, np.arange(n, dtype=np.uint32) >> 1), mode
        e.query_kernel("lds")


def test_qblk_w_bitmap_words_either_side():
    # next_order 32 * QBLK_W - 1: QBLK_W used bitmap words, staged in LDS; one more item: the
    # per-thread span_of_order in HBM.  The extra item is typed at the document's end, so every
    # common order keeps its position.
    k = 2000
    ops0 = R.scattered(32 * QBLK_W - 1 - k, k, 17)
    ops1 = np.concatenate([ops0, np.array([(32 * QBLK_W - 1, 0, 1)], np.uint32)])
    orc = [oracle_for(ops0, 32), oracle_for(ops1, 32)]
    e = engine_with(2, 32, {0: ops0, 1: ops1})
    assert list(e.versions()) == [32 * QBLK_W - 1, 32 * QBLK_W]
    assert [int(v) // 32 + 1 for v in e.versions()] == [QBLK_W, QBLK_W + 1]  # (used words: staged, not staged)
    for d in (0, 1):
        check_index(e, d, orc[d])
    ex = orc[0].export()
    ag, sq = locs_of(ex, 1, np.random.default_rng(23))
    for mode in ("lds", "per_thread"):
        e.query_kernel(mode)
        a = e.loc_to_pos(np.zeros(sq.shape, np.uint32), ag, sq)
        b = e.loc_to_pos(np.ones(sq.shape, np.uint32), ag, sq)
        common = sq < 32 * QBLK_W - 1
        assert common.sum() > N_SAMPLES and np.array_equal(a[1][common], b[1][common]), mode
        assert np.array_equal(a[0][common & (a[1] != 2)], b[0][common & (a[1] != 2)]), mode
    e.query_kernel("lds")


@functools.lru_cache(maxsize=None)
def agents_engine():
    wires = {0: config5_wire(5), 1: concurrent_wire(41, n_agents=6, rounds=8)[0]}
    # (one agent: scattered typing, then two stretches deleted char by char)
    p = np.concatenate([R.scattered(3000, 400, 9), np.array([(100, 1, 0)] * 300 + [(700, 1, 0)] * 300, np.uint32)])
    e = engine_with(3, 32, {2: p}, wires)
    orc = []
    for d in (0, 1):
        o = OracleDoc(32, 16)
        assert o.apply_remote_wire(wires[d]) == 0
        orc.append(o)
    orc.append(oracle_for(p, 32))
    return e, orc


@pytest.mark.parametrize("mode", ["lds", "per_thread"])
def test_loc_to_pos_several_agents_every_chunk_form(mode):
    # documents of several agents in one batch with a one-agent document: uniform chunks, a chunk
    # straddling two documents, interleaved documents, a document index and agents that do not exist,
    # seqs of delete ops and seqs past an agent's end
    e, orc = agents_engine()
    n_ag = [o.sizes()["agents"] for o in orc]
    assert n_ag[0] > 8 and n_ag[1] > 2 and n_ag[2] == 1
    top = []
    for o in orc:  # seqs each agent has
        cw = o.export()["cwo"].astype(np.int64)
        t = np.zeros(o.sizes()["agents"] + 2, np.int64)
        np.maximum.at(t, cw[:, 1], cw[:, 2] + cw[:, 3])
        top.append(t)
    rng = np.random.default_rng(3)
    h = QBLK_Q // 2
    docs = np.concatenate([np.full(2 * QBLK_Q + h, 0), np.full(QBLK_Q, 1), np.full(QBLK_Q + h, 2),
                           rng.integers(0, 4, 2 * QBLK_Q + 77)]).astype(np.uint32)  # (document 3 does not exist)
    ag = np.array([rng.integers(0, (n_ag[d] if d < 3 else 1) + 2) for d in docs], np.uint16)
    sq = np.array([rng.integers(0, (top[d][a] if d < 3 else 5) + 3) for d, a in zip(docs, ag)], np.uint32)
    e.query_kernel(mode)
    try:
        gp, gd = e.loc_to_pos(docs, ag, sq)
    finally:
        e.query_kernel("lds")
    assert (gd[docs == 3] == 2).all()
    for d in range(3):
        m = docs == d
        op, od = orc[d].loc_to_pos(ag[m], sq[m])
        assert np.array_equal(gd[m], od), (mode, d)
        assert np.array_equal(gp[m][od != 2], op[od != 2]), (mode, d)
        assert (od == 0).sum() > 50 and (od == 2).sum() > 50, (d, np.bincount(od))
    assert sum(int((orc[d].loc_to_pos(ag[docs == d], sq[docs == d])[1] == 1).sum()) for d in range(3)) > 50


# ---- D. batch forms, each pos -> loc mode and both loc -> pos kernels ------------------------------------
N_SPANS = 5000


@functools.lru_cache(maxsize=None)
def forms_engine():
    """documents: 0 empty, 1 one span, 2 N_SPANS spans, 3 poisoned (its stream ends with a delete past
    the end, as test_gpu_edge.test_error_mid_batch_poisons_only_its_document)"""
    e = crdt_amd.Engine(4, 32)
    ag = e.agent_intern([1, 2, 3], ["seph"] * 3)
    one, many = np.array([(0, 0, 100)], np.uint32), R.prepends(N_SPANS)
    bad = [(0, 0, 5), (2, 1, 0), (3, 5, 0)]
    st = e.apply_local([(1, [(int(ag[0]), one)]), (2, [(int(ag[1]), [tuple(p)]) for p in many]),
                        (3, [(int(ag[2]), [p]) for p in bad])])
    assert list(st) == [0, 0, -1]
    assert list(e.canon_counts()[1:3]) == [1, N_SPANS] and list(e.lens([0, 1, 2])) == [0, 100, N_SPANS]
    return e, {1: oracle_for(one, 32), 2: R.oracle_doc(("prepends", N_SPANS), 32)}


def expect_p2l(orc, docs, pos):
    wa = np.full(pos.shape, NOT_FOUND[0], np.uint16)
    ws = np.full(pos.shape, NOT_FOUND[1], np.uint32)
    for d, o in orc.items():
        m = docs == d
        wa[m], ws[m] = o.pos_to_loc(pos[m])
    return wa, ws


@pytest.mark.parametrize("mode", MODES)
def test_batch_forms(mode):
    e, orc = forms_engine()
    rng = np.random.default_rng(7)
    e.query_kernel(mode)
    try:
        def p2l(docs, pos):
            docs, pos = np.asarray(docs, np.uint32), np.asarray(pos, np.uint32)
            ga, gs = e.pos_to_loc(docs, pos)
            wa, ws = expect_p2l(orc, docs, pos)
            bad = np.flatnonzero((ga != wa) | (gs != ws))
            assert not bad.size, (mode, int(bad[0]), int(docs[bad[0]]), int(pos[bad[0]]), int(ga[bad[0]]), int(gs[bad[0]]))
            return ga

        def l2p(docs, seq):
            docs, seq = np.asarray(docs, np.uint32), np.asarray(seq, np.uint32)
            gp, gd = e.loc_to_pos(docs, np.zeros(seq.shape, np.uint16), seq)
            wp, wd = np.full(seq.shape, NOT_FOUND[1], np.uint32), np.full(seq.shape, 2, np.uint8)
            for d, o in orc.items():
                m = docs == d
                wp[m], wd[m] = o.loc_to_pos(np.zeros(int(m.sum()), np.uint16), seq[m])
            assert np.array_equal(gd, wd) and np.array_equal(gp[wd != 2], wp[wd != 2]), mode
            return gd

        for n in (1, QBLK_Q - 1, QBLK_Q, QBLK_Q + 1, 2 * QBLK_Q + 1):  # batch sizes around the chunk
            for srt in (False, True):
                pos = rng.integers(0, N_SPANS + 2, n).astype(np.uint32)
                p2l(np.full(n, 2), np.sort(pos) if srt else pos)
                l2p(np.full(n, 2), np.sort(pos) if srt else pos)
        q = np.arange(QBLK_Q, dtype=np.uint32)
        for d in (4, 7, 0xFFFFFFFF):  # a uniform chunk whose document does not exist
            assert (p2l(np.full(QBLK_Q, d), q) == NOT_FOUND[0]).all()
            assert (l2p(np.full(QBLK_Q, d), q) == 2).all()
        assert (p2l(np.zeros(QBLK_Q), q) == NOT_FOUND[0]).all()  # ... on the empty document
        assert (l2p(np.zeros(QBLK_Q), q) == 2).all()
        # ... on the poisoned document, between chunks of its neighbours, which are unaffected
        docs = np.concatenate([np.full(QBLK_Q, 2), np.full(QBLK_Q, 3), np.full(QBLK_Q, 1), np.full(5, 3), np.full(5, 2)])
        pos = np.concatenate([q, q % 7, q % 103, np.arange(5), np.arange(5)])
        ga = p2l(docs, pos)
        assert (ga[docs == 3] == NOT_FOUND[0]).all() and (ga[docs == 2] != NOT_FOUND[0]).all()
        gd = l2p(docs, pos)
        assert (gd[docs == 3] == 2).all() and (gd[docs == 2] == 0).all()
        # a sorted chunk in which every position is >= len; one that starts in the last tile of vpos
        assert (p2l(np.full(QBLK_Q, 2), N_SPANS + q) == NOT_FOUND[0]).all()
        assert (p2l(np.full(QBLK_Q, 1), 100 + q) == NOT_FOUND[0]).all()
        last = (N_SPANS - 1) // QM_TILE * QM_TILE
        assert 0 < last < N_SPANS
        ga = p2l(np.full(N_SPANS - last + 2, 2), np.arange(last, N_SPANS + 2))
        assert (ga[:-2] != NOT_FOUND[0]).all()
        ga = p2l(np.full(QBLK_Q, 2), np.sort(rng.integers(last + 1, N_SPANS, QBLK_Q)))
        assert (ga != NOT_FOUND[0]).all()
    finally:
        e.query_kernel("lds")
