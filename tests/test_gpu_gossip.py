"""GPU parity on partially delivered concurrent histories (fuzz_gen.gossip_log, each in its log
order and under two causal shuffles): the HIP engine against the oracle, bit-exact, per delivery
order.  These are the histories on which integrate's scan (replay_core.h apply_txn, M_INS) takes its
Less and Greater arms, rewinds into leaves that left the cache and passes dozens of leaves in one
scan; tests/test_gossip_ref.py asserts that on the oracle's counters, tests/test_emu_parity.py runs
the same histories through the CPU emulation.

Delivery orders do not converge in the reference (fuzz_gen.gossip_log): nothing here compares two
orders of one history with each other.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from blame_ref import ref_blame  # noqa: E402
from checkout_ref import ref_checkout, ref_queries_at  # noqa: E402
from diff_ref import ref_diff  # noqa: E402
from fuzz_gen import GOSSIP_ORDERS, gossip_family  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from test_gpu_parity import assert_same, check_queries  # noqa: E402


def caps(L):
    return (L, 16 if L == 32 else 8)


def fresh_oracles(fams, L):
    out = []
    for fam in fams:
        for _seed, _k, w in gossip_family(fam):
            o = OracleDoc(*caps(L))
            out.append((o, o.apply_remote_wire(w)))
    return out


@functools.lru_cache(maxsize=None)
def oracles(fams, L):
    """[(oracle, status)] per history of the families, computed once; the tests leave them unchanged"""
    return fresh_oracles(fams, L)


def wires_of(fams):
    return [w for fam in fams for _seed, _k, w in gossip_family(fam)]


def check_documents(e, fams, L, full, msg):
    """every document of e (one per history of fams, in wires_of's order) against its oracle:
    digest, the whole exported state of the first `full` documents, and every pos -> loc and
    loc -> pos answer for the first order of every seed"""
    dg = e.digests()
    for d, (o, so) in enumerate(oracles(fams, L)):
        assert so == 0
        assert int(dg[d]) == o.digest(), (msg, d)
        if d < full:
            assert_same(e.export(d), o.export())
        if d % GOSSIP_ORDERS == 0:
            check_queries(e, d, o)


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("L", [32, 4])
def test_partial_delivery_histories(L, share):
    # families A, B and D (4, 6 and 8 agents; D has the deep scans) in one engine and one launch;
    # with and without shared streams, because the host picks the kernel instance per stream shape
    fams = ("A", "B", "D")
    wires = wires_of(fams)
    e = crdt_amd.Engine(len(wires), L)
    e.share_streams(share)
    st = e.apply_remote_wire(list(range(len(wires))), wires)
    assert (st == 0).all(), st
    check_documents(e, fams, L, len(wires), (L, share))
    e.close()


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("L", [32, 4])
def test_seventy_agents(L, share):
    # family E: 70 agents, more than the name ranks kept in LDS (RANK_LDS = 64), frontiers of up to
    # 66 heads (25 live in lanes), agents that first appear at any point of the history
    fams = ("E",)
    wires = wires_of(fams)
    e = crdt_amd.Engine(len(wires), L)
    e.share_streams(share)
    st = e.apply_remote_wire(list(range(len(wires))), wires)
    assert (st == 0).all(), st
    assert max(len(o.export()["frontier"]) for o, _ in oracles(fams, L)) > 25
    check_documents(e, fams, L, 6, (L, share))
    e.close()


@pytest.mark.parametrize("L", [32, 4])
def test_histories_that_stop(L):
    # family X (deletes of 1..4 items): some histories stop with ERR_UNKNOWN_ID where a delete
    # run's targets are not contiguous at the receiver.  Same status as the oracle per document,
    # the finished ones equal in full, and a stopped one refuses a further txn with its status.
    fams = ("X",)
    wires = wires_of(fams)
    orc = oracles(fams, L)
    exp = [so for _, so in orc]
    assert 1 <= sum(s != 0 for s in exp) <= len(exp) // 2
    for share in (True, False):
        e = crdt_amd.Engine(len(wires), L)
        e.share_streams(share)
        st = e.apply_remote_wire(list(range(len(wires))), wires)
        assert [int(s) for s in st] == exp, (share, list(st), exp)
        dg = e.digests()
        for d, (o, so) in enumerate(orc):
            if so == 0:
                assert int(dg[d]) == o.digest(), (share, d)
                assert_same(e.export(d), o.export())
                if d % GOSSIP_ORDERS == 0:
                    check_queries(e, d, o)
        ids = e.agent_intern(list(range(len(wires))), ["late"] * len(wires))
        st2 = e.apply_local([(d, [(int(ids[d]), [(0, 0, 1)])]) for d in range(len(wires))])
        for d, (o, so) in enumerate(orc):
            assert int(st2[d]) == so, (share, d, st2[d], so)  # (a finished document takes the txn)
        e.close()


@pytest.mark.parametrize("L", [32, 4])
def test_local_txns_after_the_remote_replay(L):
    # a second launch on family B: a new agent applies an insert and a delete to every document.
    # begin() reloads a fragmented frontier and the local path runs on a document whose
    # client_with_order runs interleave six agents (test_wide_frontier_then_local's pattern).
    fams = ("B",)
    wires = wires_of(fams)
    txs = [[5, 0, 3], [0, 2, 0]]
    e = crdt_amd.Engine(len(wires), L)
    st = e.apply_remote_wire(list(range(len(wires))), wires)
    assert (st == 0).all(), st
    ids = e.agent_intern(list(range(len(wires))), ["local-editor"] * len(wires))
    st = e.apply_local([(d, [(int(ids[d]), [t]) for t in txs]) for d in range(len(wires))])
    assert (st == 0).all(), st
    dg = e.digests()
    for d, (o, so) in enumerate(fresh_oracles(fams, L)):
        assert so == 0
        a = o.agent("local-editor")
        assert a == int(ids[d])
        for t in txs:
            assert o.apply_local(a, [t]) == 0
        assert int(dg[d]) == o.digest(), (L, d)
        assert_same(e.export(d), o.export())
        if d % GOSSIP_ORDERS == 0:
            check_queries(e, d, o)
    e.close()


def test_results_over_fragmented_agent_runs():
    # blame, checkout (with its queries) and diff read client_with_order; family B's tables
    # interleave six agents' runs every few items.  Leaf 32, the first order of each seed; every
    # result against its Python reference fed the ORACLE's export.
    fams = ("B",)
    pick = [d for d in range(len(wires_of(fams))) if d % GOSSIP_ORDERS == 0]
    wires = [wires_of(fams)[d] for d in pick]
    exs = [oracles(fams, 32)[d][0].export() for d in pick]
    e = crdt_amd.Engine(len(wires), 32)
    assert (e.apply_remote_wire(list(range(len(wires))), wires) == 0).all()
    docs = list(range(len(wires)))
    for ex in exs:
        assert ex["cwo"].shape[0] > 100 and len(set(ex["cwo"][:, 1].tolist())) == 6
    for mode in ("agent", "id"):
        res = e.blame(docs, mode)
        for d, ex in enumerate(exs):
            want = ref_blame(ex, mode)
            assert res[d].shape == want.shape and np.array_equal(res[d], want), (d, mode)
    for which in range(4):  # versions 1, the middle, the last but one, the last (= the current one)
        vs = [(1, int(ex["next_order"]) // 2, int(ex["next_order"]) - 1, int(ex["next_order"]))[which] for ex in exs]
        co = e.checkout(docs, vs)
        for d, ex in enumerate(exs):
            order = ref_checkout(ex, vs[d])
            assert co[d][0].shape == order.shape and np.array_equal(co[d][0], order), (d, vs[d])
            cwo = ex["cwo"].astype(np.int64)
            # every position of the view (and two past its end) -> (agent, seq)
            pos = np.arange(order.shape[0] + 2, dtype=np.uint32)
            ga, gs = e.pos_to_loc_at(np.full(pos.shape, d), pos)
            x = order.astype(np.int64)
            r = np.searchsorted(cwo[:, 0], x, side="right") - 1
            assert np.array_equal(ga[:-2], cwo[r, 1]) and np.array_equal(gs[:-2], cwo[r, 2] + (x - cwo[r, 0])), (d, vs[d])
            assert (ga[-2:] == 0xFFFF).all() and (gs[-2:] == 0xFFFFFFFF).all()
            # every order of the document (in the view, deleted before v, not yet known, delete ops)
            want_p, want_d = ref_queries_at(order, ex, vs[d])
            x = np.arange(int(ex["next_order"]), dtype=np.int64)
            r = np.searchsorted(cwo[:, 0], x, side="right") - 1
            gp, gd = e.loc_to_pos_at(np.full(x.shape, d), cwo[r, 1], cwo[r, 2] + (x - cwo[r, 0]))
            assert np.array_equal(gd, want_d) and np.array_equal(gp, want_p), (d, vs[d])
        df = e.diff(docs, vs)
        for d, ex in enumerate(exs):
            want_p, want_i = ref_diff(ex, vs[d])
            assert df[d][0].shape == want_p.shape and np.array_equal(df[d][0], want_p), (d, vs[d])
            assert np.array_equal(df[d][1], want_i), (d, vs[d])
    e.close()
