"""GPU parity on concurrent histories of multi-op remote txns (fuzz_gen.multi_op_wire: txns that
insert and delete, insert twice, name items their own earlier ops created and delete parts of their
own inserts): the shapes only apply_txn's interpreter replays (replay_core.h), through the general
record form RTXN + RINS / RDEL per op + RPARENT per parent.  The HIP engine against the oracle,
bit-exact: status, full export, digest, every pos -> loc and loc -> pos answer.  All histories are
documents of one engine per layout, so a layout costs one launch.  tests/test_multi_op_ref.py
asserts the histories' shapes on the CPU and replays them through the CPU emulation.

A history the oracle ends with an error status counts in the status comparison only."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from checkout_ref import ref_checkout  # noqa: E402
from diff_ref import ref_diff  # noqa: E402
from fuzz_gen import build_wire, draw_multi_op_txn, multi_op_family, parse_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from test_gpu_fused_publish import LAYOUTS  # noqa: E402
from test_gpu_parity import assert_same, check_queries  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def wires():
    return [w for _seed, w in multi_op_family()]


@functools.lru_cache(maxsize=None)
def oracles(leaf):
    """[(oracle, status)] per history, computed once per layout; the tests leave them unchanged"""
    out = []
    for w in wires():
        o = OracleDoc(*LAYOUTS[leaf])
        out.append((o, o.apply_remote_wire(w)))
    return out


def check_documents(e, st, leaf, msg):
    orc = oracles(leaf)
    assert [int(s) for s in st] == [so for _, so in orc], (msg, list(st))
    assert sum(so == 0 for _, so in orc) >= len(orc) - len(orc) // 10
    dg = e.digests()
    for d, (o, so) in enumerate(orc):
        if so == 0:
            assert_same(e.export(d), o.export())
            assert int(dg[d]) == o.digest(), (msg, d)
            check_queries(e, d, o)


def replay_and_compare(leaf):
    """growth, then steady: one replay from the tables' floors (they grow, the replay resumes
    mid-stream), then the same streams once more on the fitted engine, in one launch"""
    ws = wires()
    e = crdt_amd.Engine(len(ws), leaf)
    st = e.apply_remote_wire(list(range(len(ws))), ws)
    check_documents(e, st, leaf, (leaf, "growth"))
    e.publish_async()
    e.fit()
    e.reset_async()
    e.run_async()
    e.publish_async()
    e.sync()
    check_documents(e, e.status(), leaf, (leaf, "steady"))
    e.close()


@pytest.mark.parametrize("leaf", [32, 4])
def test_growth_then_steady(leaf):
    replay_and_compare(leaf)


def test_general_shape_instance():
    # the host launches a stream of remote records only in k_replay's remote-only instance, and a
    # document's staged stream is wholly remote or wholly local; CRDT_NO_SHAPES=1 (read once per
    # process) keeps every stream on the general instance, which the two-level root's documents
    # use: the same comparison in a child process with it set
    env = dict(os.environ, CRDT_NO_SHAPES="1")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_multi_op as t; "
            "t.replay_and_compare(32); t.replay_and_compare(4); print('general shape ok')"
            % (HERE, os.path.join(os.path.dirname(HERE), "text-crdt-rust_amd")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=HERE)
    assert r.returncode == 0 and "general shape ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def local_batch(seed, n_txns=40):
    """(counts, patches) of a local multi-op batch: txns of 1..4 LocalOps, replaces included"""
    rng = random.Random(seed)
    counts, patches, n = [], [], 0
    for _ in range(n_txns):
        ops, n = draw_multi_op_txn(rng, n, end_ok=True)
        counts.append(len(ops))
        patches += ops
    return np.array(counts, np.uint32), np.array(patches, np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("leaf", [32, 4])
def test_remote_batch_then_local_multi_op_batch(leaf):
    # documents that mix a remote multi_op_wire batch with a local multi-op txn batch (counts above
    # 1: LTXN + LOP records, a replace's delete and insert in one op) by a late agent: the local
    # launch begins on a frontier of several heads and on tables several agents interleave in
    ws = wires()
    good = [d for d, (_, so) in enumerate(oracles(leaf)) if so == 0]
    e = crdt_amd.Engine(len(good), leaf)
    docs = list(range(len(good)))
    assert (e.apply_remote_wire(docs, [ws[d] for d in good]) == 0).all()
    ids = e.agent_intern(docs, ["late"] * len(docs))
    per_doc, want = [], []
    for i, d in enumerate(good):
        o = OracleDoc(*LAYOUTS[leaf])
        assert o.apply_remote_wire(ws[d]) == 0
        a = o.agent("late")
        assert a == int(ids[i])
        rng = random.Random(900 + d)
        txns, n = [], len(o)
        for _ in range(12):
            ops, n = draw_multi_op_txn(rng, n)
            txns.append((a, ops))
            assert o.apply_local(a, ops) == 0
        assert sum(len(t[1]) > 1 for t in txns) >= 3
        per_doc.append((i, txns))
        want.append(o)
    st = e.apply_local(per_doc)
    assert (st == 0).all(), st
    dg = e.digests()
    for i, o in enumerate(want):
        assert_same(e.export(i), o.export())
        assert int(dg[i]) == o.digest(), (leaf, i)
        check_queries(e, i, o)
    e.close()


@pytest.mark.parametrize("leaf", [32, 4])
def test_local_multi_op_batch_then_remote_batch(leaf):
    # the other order: every document first applies a local multi-op batch by agent "solo" (its own
    # trace), then a remote batch by other agents that builds on it -- the recorded wire of
    # multi-op txns two further replicas made on top of solo's text
    from oracle_lib import _p, lib
    import ctypes as C
    n_docs = 12
    e = crdt_amd.Engine(n_docs, leaf)
    docs = list(range(n_docs))
    ids = e.agent_intern(docs, ["solo"] * n_docs)
    per_doc, remote, want = [], [], []
    buf = C.create_string_buffer(1 << 16)
    for d in docs:
        counts, patches = local_batch(40 + d)
        o = OracleDoc(*LAYOUTS[leaf])
        a = o.agent("solo")
        assert a == int(ids[d]) and o.apply_trace(a, counts, patches) == 0
        off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        per_doc.append((d, [(a, patches[off[k]:off[k + 1]]) for k in range(counts.shape[0])]))
        # two replicas of that text edit concurrently; their recorded txns, u's then v's, are the batch
        rng = random.Random(70 + d)
        txns = []
        for name in ("u", "v"):
            r = OracleDoc(*LAYOUTS[leaf])
            assert r.apply_trace(r.agent("solo"), counts, patches) == 0
            ra = r.agent(name)
            for _ in range(8):
                ops, _n = draw_multi_op_txn(rng, len(r))
                c = np.array([len(ops)], np.uint32)
                p = np.array(ops, np.uint32).reshape(-1, 3)
                n = lib().orc_local_trace_to_wire(r.h, ra, 1, _p(c), _p(p), C.cast(buf, C.c_void_p), 1 << 16)
                assert n > 0
                txns += parse_wire(buf.raw[:n])[1]
        w = build_wire(txns)
        remote.append(w)
        want.append((o, o.apply_remote_wire(w)))
    assert (e.apply_local(per_doc) == 0).all()
    st = e.apply_remote_wire(docs, remote)
    assert [int(s) for s in st] == [so for _, so in want], list(st)
    assert sum(so == 0 for _, so in want) >= n_docs - 1
    dg = e.digests()
    for d, (o, so) in enumerate(want):
        if so == 0:
            assert_same(e.export(d), o.export())
            assert int(dg[d]) == o.digest(), (leaf, d)
            check_queries(e, d, o)
    e.close()


VERSION_HISTORIES = 4


@pytest.mark.parametrize("leaf", [32, 4])
def test_every_version_inside_multi_op_txns(leaf):
    # a version may lie inside a txn: checkout at, and diff from, every version 0 .. next_order of
    # four histories -- document k of next_order + 1 copies of a history at version k, all
    # histories' copies in one engine and one call each -- against the references fed the ORACLE's export
    orc = oracles(leaf)
    pick = [d for d, (o, so) in enumerate(orc) if so == 0 and 150 <= o.sizes()["next_order"] <= 450][:VERSION_HISTORIES]
    assert len(pick) == VERSION_HISTORIES
    ws = wires()
    exs = [orc[d][0].export() for d in pick]
    vers = [int(ex["next_order"]) for ex in exs]
    doc_wire, doc_hist, doc_v = [], [], []
    for h, d in enumerate(pick):
        doc_wire += [ws[d]] * (vers[h] + 1)
        doc_hist += [h] * (vers[h] + 1)
        doc_v += list(range(vers[h] + 1))
    n = len(doc_wire)
    e = crdt_amd.Engine(n, leaf)
    docs = np.arange(n)
    assert (e.apply_remote_wire(docs, doc_wire) == 0).all()
    assert np.array_equal(e.versions(), [vers[h] for h in doc_hist])
    co = e.checkout(docs, doc_v)
    df = e.diff(docs, doc_v)
    for i in range(n):
        ex, v = exs[doc_hist[i]], doc_v[i]
        order = ref_checkout(ex, v)
        assert co[i][0].shape == order.shape and np.array_equal(co[i][0], order), (doc_hist[i], v)
        want_p, want_i = ref_diff(ex, v)
        assert df[i][0].shape == want_p.shape and np.array_equal(df[i][0], want_p), (doc_hist[i], v)
        assert np.array_equal(df[i][1], want_i), (doc_hist[i], v)
    e.close()
