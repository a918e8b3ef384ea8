"""Fused publish (k_replay waves publish their own documents on a fitted index): every
case runs through the C ABI with the fusion on and off, at both leaf layouts, and compares the
published index bit for bit between the two runs -- canon_n, canonical spans, vpos, lengths,
statuses, digests -- and the answers of pos -> loc and loc -> pos queries; where the oracle has the
history (the micro workloads, the traces' committed digests) both runs are compared with it too."""
import functools
import gzip
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from crdt_amd.traces import load_remote_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from test_gpu_edge import _wire_of_local  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {32: (32, 16), 4: (4, 8)}
MICRO = ["base", "bs10", "bs200", "del1", "fd200", "jump1", "jump10", "typing"]
from kernel_consts import PUB_BIG_MIN  # noqa: E402  (kernels.h: leaves from which a document of a small batch publishes with a workgroup)
N_QUERIES = 300


@functools.lru_cache(maxsize=None)
def micro_wire(name: str) -> bytes:
    with gzip.open(os.path.join(ROOT, "data", "micro", name + ".rtx.gz"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def oracle_of(name: str, leaf: int):
    """(digest, len, canonical spans) of the oracle's replay of a micro workload: computed once"""
    o = OracleDoc(*LAYOUTS[leaf])
    assert o.apply_remote_wire(micro_wire(name)) == 0
    return o.digest(), len(o), o.export()["canon"]


def golden_digest(trace: str, leaf: int) -> int:
    with open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")) as f:
        return int(json.load(f)[f"{trace}/L{leaf}"]["remote_digest"], 16)


def snapshot(e):
    """everything a publish leaves behind, per document, plus query answers on it"""
    n = e.n_docs
    cn = e.canon_counts()
    lens = e.lens()
    out = dict(canon_n=cn, lens=lens, status=e.status(), digests=e.digests(),
               canon=[e.export(d)["canon"] for d in range(n)], vpos=[e.debug_vpos(d) for d in range(n)])
    rng = np.random.default_rng(11)
    docs = np.repeat(np.arange(n, dtype=np.uint32), N_QUERIES)
    pos = (rng.random(n * N_QUERIES) * (np.repeat(lens, N_QUERIES) + 2)).astype(np.uint32)  # (some past the end)
    out["p2l"] = e.pos_to_loc(docs, pos)
    ag, seq = out["p2l"]
    seq2 = np.where(rng.random(seq.shape[0]) < 0.5, seq, rng.integers(0, 80000, seq.shape[0])).astype(np.uint32)
    out["l2p"] = e.loc_to_pos(docs, np.where(ag == 0xFFFF, 0, ag).astype(np.uint16), seq2)
    return out


def assert_same_snapshot(a, b):
    for k in ("canon_n", "lens", "status", "digests"):
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])
    for k in ("canon", "vpos"):
        for d, (x, y) in enumerate(zip(a[k], b[k])):
            assert x.shape == y.shape and np.array_equal(x, y), (k, d)
    for k in ("p2l", "l2p"):
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), k


def both_modes(leaf, scenario):
    """scenario(engine factory) -> (snapshot, per-document "published by its replay wave" flags);
    run with the fusion on and off; returns the on-run's results after comparing the two"""
    res = {}
    for on in (True, False):
        def make(n):
            e = crdt_amd.Engine(n, leaf)
            e.fused_publish(on)
            return e
        res[on] = scenario(make)
    assert_same_snapshot(res[True][0], res[False][0])
    assert res[False][1] is None or not res[False][1].any()
    return res[True]


def fit_reset_run_publish(e):
    """the benchmark's steady step, after an untimed run + publish + fit"""
    assert (e.run() == 0).all()
    e.publish_async()
    e.fit()
    e.reset_async()
    e.run_async()
    e.publish_async()
    e.sync()


@pytest.mark.parametrize("leaf", [32, 4])
def test_uneven_streams(leaf):
    # 9 documents = more than two workgroups of 4 waves: the eight micro workloads and one empty
    # document, so the waves of a workgroup end at different times and some publish while their
    # neighbours still replay.  Documents past PUB_BIG_MIN leaves (leaf 4: five of them) stay with
    # k_publish_big in the same launch.
    def scenario(make):
        e = make(9)
        e.apply_remote_wire(list(range(8)), [micro_wire(m) for m in MICRO], stage_only=True)
        fit_reset_run_publish(e)
        n0, flags = e.fused_publish_stats()
        assert (e.status() == 0).all()
        leaves = np.array([e.export_sizes(d)["leaves"] for d in range(9)])
        return snapshot(e), flags, leaves, n0

    snap, flags, leaves, launches = both_modes(leaf, scenario)
    small = leaves < PUB_BIG_MIN
    assert launches >= 1 and np.array_equal(flags[:8], small[:8]), (flags, leaves)
    assert small[[0, 7]].all() and small.sum() >= (8 if leaf == 32 else 3)
    for d, m in enumerate(MICRO):
        dg, ln, canon = oracle_of(m, leaf)
        assert int(snap["digests"][d]) == dg and int(snap["lens"][d]) == ln, m
        assert np.array_equal(snap["canon"][d], canon), m
    assert snap["lens"][8] == 0 and snap["canon_n"][8] <= 1


@pytest.mark.parametrize("leaf", [32, 4])
def test_capacity_stop_and_resume(leaf):
    # documents stop with NEED_CAPACITY in their first launch (every table starts at its floor) and
    # resume after growth; the index is not sized yet, so no launch of this run may fuse, and the
    # publish that follows is k_publish's
    def scenario(make):
        e = make(3)
        st = e.apply_remote_wire([0, 1, 2], [micro_wire("del1"), micro_wire("jump10"), micro_wire("bs200")])
        assert (st == 0).all()
        e.publish_async()
        e.sync()
        n0, flags = e.fused_publish_stats()
        assert n0 == 0 and not flags.any()
        return snapshot(e), flags

    snap, _ = both_modes(leaf, scenario)
    for d, m in enumerate(["del1", "jump10", "bs200"]):
        assert int(snap["digests"][d]) == oracle_of(m, leaf)[0]


@pytest.mark.parametrize("leaf", [32, 4])
def test_fit_reset_run_publish(leaf):
    # the benchmark's sequence at 8 documents of two micro traces: the fused path is taken (every
    # document below PUB_BIG_MIN leaves is published by its replay wave)
    names = ["typing", "bs10"] * 4

    def scenario(make):
        e = make(8)
        e.apply_remote_wire(list(range(8)), [micro_wire(m) for m in names], stage_only=True)
        fit_reset_run_publish(e)
        n0, flags = e.fused_publish_stats()
        leaves = np.array([e.export_sizes(d)["leaves"] for d in range(8)])
        snap = snapshot(e)
        # a second steady step on the same engine publishes the same index again
        e.reset_async()
        e.run_async()
        e.publish_async()
        e.sync()
        assert_same_snapshot(snap, snapshot(e))
        return snap, flags, leaves, n0, e.fused_publish_stats()[0]

    snap, flags, leaves, n0, n1 = both_modes(leaf, scenario)
    assert n0 == 1 and n1 == 2
    assert np.array_equal(flags, leaves < PUB_BIG_MIN) and flags[0::2].all(), (flags, leaves)
    if leaf == 32:
        assert flags.all()
    for d, m in enumerate(names):
        assert int(snap["digests"][d]) == oracle_of(m, leaf)[0]


@pytest.mark.parametrize("leaf", [32, 4])
def test_stale_stamps(leaf):
    # reset then publish with no run: the index is the empty documents', not the one the replay
    # waves published before the reset; then a second stream staged after a publish: the index is
    # the new state's
    def scenario(make):
        e = make(4)
        w = [micro_wire("jump10"), micro_wire("typing")] * 2
        e.apply_remote_wire([0, 1, 2, 3], w, stage_only=True)
        fit_reset_run_publish(e)
        launches, flags = e.fused_publish_stats()
        assert flags.all() == (launches > 0)  # (both documents are short: on, their waves published them)
        full = snapshot(e)
        e.reset_async()
        e.publish_async()
        e.sync()
        assert not e.fused_publish_stats()[1].any()
        empty = snapshot(e)
        assert (empty["lens"] == 0).all() and (empty["canon_n"] <= 1).all()
        # replay again (fused), publish, then stage a second stream on top and run it
        e.run_async()
        e.publish_async()
        e.sync()
        assert_same_snapshot(full, snapshot(e))
        o = OracleDoc(*LAYOUTS[leaf])
        assert o.apply_remote_wire(micro_wire("typing")) == 0
        ops = [(5, 3, 0), (0, 0, 4), (len(o) - 2, 0, 7)]
        w2 = _wire_of_local(o, o.agent("second"), np.ones(len(ops), np.uint32), np.array(ops, np.uint32))
        assert (e.apply_remote_wire([1, 3], [w2, w2]) == 0).all()
        e.publish_async()
        e.sync()
        assert not e.fused_publish_stats()[1].any()
        snap = snapshot(e)
        assert int(snap["digests"][1]) == int(snap["digests"][3]) == o.digest()
        assert int(snap["digests"][0]) == int(full["digests"][0])
        return snap, None

    both_modes(leaf, scenario)


@pytest.mark.parametrize("leaf", [32, 4])
def test_refusal(leaf):
    # a document whose canonical spans exceed canon_cap (or whose orders exceed ord_cap) is refused
    # the same way in both modes: canon_n 0 and digest 0.  Forced with a deliberately small noted
    # fit: generated-edit documents fitted to the capacities noted on one batch of a corpus only
    # (crdt_fit_note), then reseeded to another batch, whose documents need a little more or less
    # of every table; no growth happens in crdt_run_async, so some stop for capacity (and publish
    # what they reached), some finish inside the state tables but past the index and are refused.
    n, ops, seed = 48, 2000, 0xFACADE

    def scenario(make):
        e = make(n)
        e.stage_random(list(range(n)), "gen", ops, seed)
        assert (e.run() == 0).all()
        e.publish_async()
        e.sync()
        e.fit_note(False)
        e.fit_note(True)
        e.reseed_random_async(seed, 7 * n)
        e.reset_async()
        e.run_async()
        e.publish_async()
        e.sync()
        return snapshot(e), e.fused_publish_stats()[1]

    snap, flags = both_modes(leaf, scenario)
    assert flags.all()
    refused = (snap["status"] == 0) & (snap["canon_n"] == 0) & (snap["digests"] == 0)
    assert refused.any(), (snap["status"], snap["canon_n"])
    # (a refused document has a length and no spans: position queries on it find nothing)
    assert (snap["p2l"][0].reshape(n, N_QUERIES)[refused] == 0xFFFF).all()
    assert ((snap["canon_n"] > 0) & (snap["digests"] > 1)).any()


@pytest.mark.parametrize("leaf", [32, 4])
def test_big_and_small_mixed(leaf):
    # one document on the k_publish_big list (>= PUB_BIG_MIN leaves in a batch of <= 1,024 documents:
    # automerge-paper at leaf 32, sveltecomponent at leaf 4) beside a small one in the same launch:
    # the big one is published by k_publish_big, the small one by its replay wave
    trace = "automerge-paper" if leaf == 32 else "sveltecomponent"

    def scenario(make):
        e = make(2)
        e.apply_remote_wire([0, 1], [load_remote_wire(trace), micro_wire("jump10")], stage_only=True)
        fit_reset_run_publish(e)
        n0, flags = e.fused_publish_stats()
        leaves = [e.export_sizes(d)["leaves"] for d in range(2)]
        return snapshot(e), flags, leaves, n0

    snap, flags, leaves, n0 = both_modes(leaf, scenario)
    assert leaves[0] >= PUB_BIG_MIN > leaves[1], leaves
    assert n0 == 1 and list(flags) == [False, True]
    assert int(snap["digests"][0]) == golden_digest(trace, leaf)
    assert int(snap["digests"][1]) == oracle_of("jump10", leaf)[0]
