"""Hostile remote input on the engine: the hand-built compact-record streams of
tests/hostile_streams.py through k_replay's lane-parallel forms (wave_gpu.h decode_window's mask,
typing_scan_m / typing_scan_at, the hinted fast_deletes with its carried cursor), malformed wire
batches through the staging entry points, and the parent limit.  tests/test_hostile_streams_ref.py
asserts the families' conditions and replays them on the CPU emulation, which scans where the
kernel reads a mask; tests/test_wire_malformed.py shows, on the CPU and under sanitizers, that the
malformed wires used here are refused cleanly by the parser.

Every error case sits next to a valid one (hostile_streams.interleaved), all documents of one
engine: a document that stops with the oracle's status is the expected result, and its neighbours in
the block must equal the oracle in full.  Nothing here can fault the device: a stopped document is
a status, and a malformed wire never reaches it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
import hostile_streams as hs  # noqa: E402
from fuzz_gen import build_wire  # noqa: E402
from oracle_lib import OracleDoc  # noqa: E402
from test_gpu_fused_publish import LAYOUTS  # noqa: E402
from test_gpu_parity import KEYS, assert_same, check_queries  # noqa: E402

ON_OFF = pytest.mark.parametrize("on", [True, False], ids=["decode", "scan"])
M32 = 0xFFFFFFFF
R = ("ROOT", M32)


def check_documents(e, st, cases, leaf, msg):
    """every document's status is the oracle's; a document with status 0 equals the oracle's in
    full (export, digest, every position query)"""
    res = hs.oracle_results(leaf)
    want = [res[c.name][0] for c in cases]
    got = [int(s) for s in st]
    wrong = [(c.name, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, (msg, len(wrong), wrong[:10])
    dg = e.digests()
    bad = []
    for d, c in enumerate(cases):
        if want[d] != 0:
            continue
        o = res[c.name][1]
        try:
            assert_same(e.export(d), o.export())
            assert int(dg[d]) == o.digest(), "digest"
            check_queries(e, d, o)
        except AssertionError as x:
            bad.append((d, c.name, " ".join(str(x).split())[:80]))
    assert not bad, (msg, len(bad), bad[:8])
    return want


@ON_OFF
@pytest.mark.parametrize("leaf", [32, 4])
def test_stream_batch_in_one_launch(leaf, on):
    # the base batch first; the stream batch then replays in ONE launch without growth handling
    # (crdt_run_async), so every document reads its window from record 0 on: txn k of a stream is
    # lane k of the first window.  (A stop for capacity would show as a status the oracle never has.)
    cases = hs.interleaved()
    docs = list(range(len(cases)))
    assert 600 <= len(cases) <= 800 and sum(c.want != 0 for c in cases) == len(cases) // 2
    e = crdt_amd.Engine(len(cases), leaf)
    e.window_decode(on)
    assert (e.apply_remote_wire(docs, [c.wires[0] for c in cases]) == 0).all()
    e.apply_remote_wire(docs, [c.wires[1] for c in cases], stage_only=True)
    e.run_async()
    e.sync()
    want = check_documents(e, e.status(), cases, leaf, (leaf, on, "one launch"))
    # a stopped document takes no further txn: a later local one is refused with the same status,
    # and the good documents take it
    ids = e.agent_intern(docs, ["late"] * len(docs))
    st2 = e.apply_local([(d, [(int(ids[d]), [(0, 0, 1)])]) for d in docs])
    assert [int(s) for s in st2] == want
    e.close()


@ON_OFF
@pytest.mark.parametrize("leaf", [32, 4])
def test_one_wire_with_growth_stops(leaf, on):
    # base and stream as one wire through crdt_apply_remote_wire: the tables grow from their floors
    # and the replay resumes mid-stream, windows loaded at whatever record it stopped at
    cases = hs.interleaved()
    docs = list(range(len(cases)))
    e = crdt_amd.Engine(len(cases), leaf)
    e.window_decode(on)
    st = e.apply_remote_wire(docs, [c.wires[2] for c in cases])
    check_documents(e, st, cases, leaf, (leaf, on, "one wire"))
    e.close()


# ---------------------------------------------------------------- CRDT_E_WIRE on the engine
def _expect_rc(rc, what):
    return pytest.raises(crdt_amd.CrdtError, match=f"{what} failed rc={rc} ")


@pytest.mark.parametrize("leaf", [32, 4])
def test_rejected_wire_changes_nothing(leaf):
    n = 3
    docs = list(range(n))
    ws = [hs.doc_wires(d) for d in docs]
    e = crdt_amd.Engine(n, leaf)
    assert (e.apply_remote_wire(docs, [w[0] for w in ws]) == 0).all()
    before = e.digests().copy()
    for name, bad in hs.malformed_wires().items():
        for at in (1, 2):  # the malformed wire second or third: documents before it would have been encoded
            batch = [w[1] for w in ws]
            batch[at] = bad
            with _expect_rc(-103, "apply_remote_wire"):
                e.apply_remote_wire(docs, batch)
            with _expect_rc(-103, "stage_remote"):
                e.apply_remote_wire(docs, batch, stage_only=True)
            assert np.array_equal(e.digests(), before), (name, at)
            assert (e.status() == 0).all()
    # a later valid call: exports, agent ids included, as if the rejected calls had not happened
    assert (e.apply_remote_wire(docs, [w[2] for w in ws]) == 0).all()
    for d in docs:
        o = OracleDoc(*LAYOUTS[leaf])
        assert o.apply_remote_wire(ws[d][0]) == 0 and o.apply_remote_wire(ws[d][2]) == 0
        assert_same(e.export(d), o.export())
        assert int(e.digests()[d]) == o.digest()
        check_queries(e, d, o)
    e.close()


def test_rejected_replicated_wire_changes_nothing():
    def whole(base):
        return build_wire([(base, 0, [R], [(0, "ROOT", M32, "ROOT", M32, 10)]),
                           ("amy", 0, [(base, 9)], [(0, base, 5, base, 6, 3)]),
                           ("zed", 0, [("amy", 2)], [(0, "amy", 1, "amy", 2, 2), (1, base, 0, None, 0, 2)])])
    names = [f"base{d}" for d in range(4)]  # (name 0 of the batch, "base", renamed per document)
    e = crdt_amd.Engine(4, 32)
    before = e.digests().copy()
    for name, bad in hs.malformed_wires().items():
        with _expect_rc(-103, "stage_replicated"):
            e.stage_remote_replicated(bad, 0, names)
        assert np.array_equal(e.digests(), before), name
    e.stage_remote_replicated(whole("base"), 0, names)
    assert (e.run() == 0).all()
    for d in range(4):
        o = OracleDoc()
        assert o.apply_remote_wire(whole(names[d])) == 0
        assert_same(e.export(d), o.export())
        assert int(e.digests()[d]) == o.digest()
    e.close()


def test_misaligned_wire_pointer_is_refused():
    # WireView keeps u32 pointers into the caller's buffer: a wire that does not start on a 4-byte
    # boundary is CRDT_E_ARG (-100) at both remote staging entry points, and nothing changes
    L = crdt_amd.lib()
    first, _rejected, later = hs.doc_wires(0)
    e = crdt_amd.Engine(1, 32)
    assert e.apply_remote_wire([0], [first])[0] == 0
    before = e.digests().copy()
    buf = C.create_string_buffer(len(later) + 8)
    base = (C.addressof(buf) + 3) & ~3
    docs = np.zeros(1, np.uint32)
    ln = np.array([len(later)], np.uint64)
    st = np.zeros(1, np.int32)
    for off in (1, 2, 3):
        C.memmove(base + off, later, len(later))
        arr = (C.c_char_p * 1)(C.c_char_p(base + off))
        u32p, u64p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
        assert L.crdt_stage_remote_wire(e.h, 1, docs.ctypes.data_as(u32p), arr, ln.ctypes.data_as(u64p)) == -100
        assert L.crdt_apply_remote_wire(e.h, 1, docs.ctypes.data_as(u32p), arr, ln.ctypes.data_as(u64p),
                                        st.ctypes.data_as(i32p)) == -100
        assert L.crdt_stage_remote_replicated(e.h, C.c_char_p(base + off), len(later), 0, None) == -100
        assert np.array_equal(e.digests(), before)
    # the same bytes on the boundary are taken
    C.memmove(base, later, len(later))
    arr = (C.c_char_p * 1)(C.c_char_p(base))
    assert L.crdt_apply_remote_wire(e.h, 1, docs.ctypes.data_as(C.POINTER(C.c_uint32)), arr,
                                    ln.ctypes.data_as(C.POINTER(C.c_uint64)), st.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    o = OracleDoc()
    assert o.apply_remote_wire(first) == 0 and o.apply_remote_wire(later) == 0
    assert st[0] == 0 and int(e.digests()[0]) == o.digest()
    assert_same(e.export(0), o.export())
    e.close()


# ---------------------------------------------------------------- the parent limit
@pytest.mark.parametrize("leaf", [32, 4])
def test_parent_limit(leaf):
    # 65,535 parents fit the record header and replay as the oracle does; a txn of 65,536 stops its
    # document with CRDT_ERR_BAD_INPUT at the header: the state is the oracle's of the wire without
    # that txn (and what follows it), and the neighbour is intact
    w_ok, _ = hs.parent_limit_wires(65535)
    w_over, head = hs.parent_limit_wires(65536)
    e = crdt_amd.Engine(3, leaf)
    st = e.apply_remote_wire([0, 1, 2], [w_ok, w_over, w_ok])
    assert [int(s) for s in st] == [0, -9, 0]
    o = OracleDoc(*LAYOUTS[leaf])
    assert o.apply_remote_wire(w_ok) == 0
    for d in (0, 2):
        assert_same(e.export(d), o.export())
        assert int(e.digests()[d]) == o.digest()
        check_queries(e, d, o)
    o = OracleDoc(*LAYOUTS[leaf])
    assert o.apply_remote_wire(head) == 0
    # (every table of the replay; the canonical spans are the published index, and k_publish
    # leaves a stopped document out)
    assert_same(e.export(1), o.export(), [k for k in KEYS if k != "canon"])
    assert e.export(1)["canon"].shape[0] == 0
    e.close()
