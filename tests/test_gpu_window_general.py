"""General-form record groups against k_replay's record window (replay_core.h rec / rec_at /
rec_window over wave_gpu.h rec_slide, rec_load2, rec_get, ld_rec): the hand-built streams of
tests/general_streams.py -- (a) runs of general-form one-op txns, which fast_txn takes at stride 3,
at every phase of the 64-record window, and (b) txns of up to 140 ops and 1 or 3 parents whose
1 + ops + parents records end short of, at and past every threshold at which rec() slides or
reloads the window, with general-form txns behind them that read the window after the jump -- and
multi-op txns that fail at their second or third op.  Every stream replays at both leaf layouts,
with the window decode (crdt_set_window_decode) on and off, in one engine per layout and switch, and
its full export is compared with the oracle's, exactly.  tests/test_multi_op_ref.py replays the
same streams on the CPU emulation and proves through its statistics build which branches they reach.

A stream's prep txns are staged as a first batch and the stream as a second, so record k of the
stream sits in lane k of the first window.  Verified by reading the code: staging a batch resets
the document's record cursor (kernels.h k_reset_recpos) and sets its record count to the batch's;
a Replayer starts with no window (T_RB_BASE = 0x80000000), so the first rec(0) loads the window at
record 0 (rec_window -> rec_load2); the host encodes a pad as one compact record and every other
txn of a stream as 1 + ops + parents records (host_plan.h encode_remote; general_streams.records
counts the same way and test_stream_batches_hold_the_records_they_claim compares the two through
the wire).  A replay that stops for capacity would resume with a window loaded at the record it
stopped at -- and before a txn of n ops the replay reserves 2n free leaves (replay_core.h fits), so
without more a group of 33 ops or more stops AT its header and resumes with the header in lane 0,
whatever the pad.  The prep batch therefore holds a warm-up txn that grows the leaf table
(general_streams._prep), and the stream batch replays in one launch without growth handling
(crdt_run_async): status 0 there says no document stopped."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
import general_streams as gs  # noqa: E402
from fuzz_gen import parse_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from test_gpu_fused_publish import LAYOUTS  # noqa: E402
from test_gpu_parity import assert_same, check_queries  # noqa: E402

ON_OFF = pytest.mark.parametrize("on", [True, False], ids=["decode", "scan"])
FAMILIES = {"runs": gs.run_family, "groups": gs.group_family}


@functools.lru_cache(maxsize=None)
def oracle_exports(family, leaf):
    """name -> the oracle's export after both batches, computed once per family and layout"""
    out = {}
    for name, (w0, w1, _w) in FAMILIES[family]().items():
        o = OracleDoc(*LAYOUTS[leaf])
        assert o.apply_remote_wire(w0) == 0 and o.apply_remote_wire(w1) == 0, name
        out[name] = o.export()
    return out


def test_stream_batches_hold_the_records_they_claim():
    # the second batch of a stream is pads (one op, own items, own previous txn as the parent: the
    # compact form), then txns that each name a base item or hold several ops (the general form)
    for fam, name, pad in (("runs", "typing_n22_pad63", 63), ("runs", "back_n64_pad0", 0), ("groups", "mixed_p3_ops125_pad61", 61)):
        txns = parse_wire(FAMILIES[fam]()[name][1])[1]
        assert gs.records(txns[:pad]) == pad and all(t[0] == "a" for t in txns)
        for a, s, ps, ops in txns[pad:-3] if fam == "runs" else txns[pad:]:
            assert len(ops) > 1 or any(nm == "base" for nm in (ops[0][1], ops[0][3]))


@ON_OFF
@pytest.mark.parametrize("leaf", [32, 4])
@pytest.mark.parametrize("family", ["runs", "groups"])
def test_window_families(family, leaf, on):
    fam = FAMILIES[family]()
    names = sorted(fam)
    docs = list(range(len(names)))
    e = crdt_amd.Engine(len(names), leaf)
    e.window_decode(on)
    assert (e.apply_remote_wire(docs, [fam[n][0] for n in names]) == 0).all()
    # the stream batch in ONE launch without growth handling (crdt_run_async): status 0 for every
    # document also says that none stopped for capacity, so each read its window from record 0 on
    e.apply_remote_wire(docs, [fam[n][1] for n in names], stage_only=True)
    e.run_async()
    e.sync()
    st = e.status()
    assert (st == 0).all(), [(names[i], int(st[i])) for i in np.flatnonzero(st)][:8]
    want = oracle_exports(family, leaf)
    bad = []
    for d, n in enumerate(names):
        try:
            assert_same(e.export(d), want[n])
        except AssertionError as x:
            bad.append((n, " ".join(str(x).split())[:60]))
    e.close()
    assert not bad, (len(bad), bad[:8])


@ON_OFF
@pytest.mark.parametrize("leaf", [32, 4])
def test_error_in_the_middle_of_a_multi_op_txn(leaf, on):
    # a three-op txn whose second or third op fails, between two good documents: the oracle's
    # status, the good documents untouched, and the failed one takes no further txn -- neither the
    # one behind the failing txn in its batch nor a later local one
    good = gs.good_wire()
    og = OracleDoc(*LAYOUTS[leaf])
    assert og.apply_remote_wire(good) == 0
    for name in gs.ERROR_CASES:
        w = gs.error_wire(name)
        o = OracleDoc(*LAYOUTS[leaf])
        want = o.apply_remote_wire(w)
        assert want != 0, name
        e = crdt_amd.Engine(3, leaf)
        e.window_decode(on)
        st = e.apply_remote_wire([0, 1, 2], [good, w, good])
        assert [int(s) for s in st] == [0, want, 0], (name, list(st), want)
        for d in (0, 2):
            assert_same(e.export(d), og.export())
            assert int(e.digests()[d]) == og.digest()
            check_queries(e, d, og)
        ids = e.agent_intern([0, 1, 2], ["late"] * 3)
        st2 = e.apply_local([(d, [(int(ids[d]), [(0, 0, 1)])]) for d in range(3)])
        assert [int(s) for s in st2] == [0, want, 0], (name, list(st2))
        e.close()
