"""The carried cursor and the split-first path of k_replay's delete runs (replay_core.h
fast_deletes; DESIGN §4 "Carried cursor") on the GPU: the hand-built streams of
tests/test_delete_carry.py (which proves on the CPU emulation that each reaches its branch), four
documents each, and the delete micro workloads and the flagship trace on two documents each, at
both leaf layouts.  The full export -- raw spans, tables, digests -- is compared with the oracle's,
exactly, after crdt_run and again after the steady step on the fitted engine."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from crdt_amd.traces import load_remote_wire  # noqa: E402
from test_delete_carry import MICRO, oracle_docs, wires  # noqa: E402
from test_gpu_fused_publish import golden_digest, micro_wire, oracle_of  # noqa: E402
from test_gpu_parity import assert_same  # noqa: E402

COPIES = 4


def _compare(e, keys, want):
    bad = []
    for d, k in enumerate(keys):
        try:
            assert_same(e.export(d), want[k])
        except AssertionError as x:
            bad.append((k, " ".join(str(x).split())[:60]))
    assert not bad, (len(bad), bad)


@pytest.mark.parametrize("leaf", [32, 4])
def test_hand_built_streams(leaf):
    ws = wires()
    keys = [(n, i) for n in sorted(ws) for i in range(len(ws[n])) for _ in range(COPIES)]
    docs = list(range(len(keys)))
    e = crdt_amd.Engine(len(keys), leaf)
    st = e.apply_remote_wire(docs, [ws[n][i] for n, i in keys])
    assert (st == 0).all(), [keys[i] for i in np.flatnonzero(st)]
    want = {k: o.export() for k, o in oracle_docs(leaf).items()}
    _compare(e, keys, want)
    # the benchmark's steady step: the same streams replayed in one launch on the fitted engine
    e.publish_async()
    e.fit()
    e.reset_async()
    e.run_async()
    e.publish_async()
    e.sync()
    assert (e.status() == 0).all()
    _compare(e, keys, want)
    e.close()


@pytest.mark.parametrize("leaf", [32, 4])
def test_micro_wires_and_automerge_paper(leaf):
    ms = [m for m in MICRO for _ in range(2)]
    n = len(ms) + 2
    e = crdt_amd.Engine(n, leaf)
    ap = load_remote_wire("automerge-paper")
    e.apply_remote_wire(list(range(n)), [micro_wire(m) for m in ms] + [ap] * 2, stage_only=True)
    want = [oracle_of(m, leaf)[0] for m in ms] + [golden_digest("automerge-paper", leaf)] * 2
    assert (e.run() == 0).all()
    assert [int(x) for x in e.digests()] == want
    e.publish_async()
    e.fit()
    e.reset_async()
    e.run_async()
    e.publish_async()
    e.sync()
    assert (e.status() == 0).all()
    assert [int(x) for x in e.digests()] == want
    for d, m in enumerate(ms):
        assert np.array_equal(e.export(d)["canon"], oracle_of(m, leaf)[2]), m
    e.close()
