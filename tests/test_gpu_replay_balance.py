"""Progress balance of k_replay's waves (kernels.h balance_board_tick): wave priority
changes when instructions issue, never what they compute.  Every case replays the same streams
with the balance on and off, at both leaf layouts, and compares status, digest and the full export
byte for byte; after every launch the board's copy-out must hold no slot with work left (every way
out of the replay clears the wave's slot), and the stamped writes must be there exactly when the
launch ran with the board.  Both policies are covered: "on" is the board on every launch, "auto"
(the default) the rotation on launches whose waves are all resident at once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from crdt_amd.traces import load_remote_wire  # noqa: E402
from fuzz_gen import build_wire, parse_wire  # noqa: E402
from test_gpu_fused_publish import micro_wire, oracle_of, golden_digest  # noqa: E402

LEFT = 0xFFFFFF  # a slot is launch stamp << 24 | records left
ST_CAPACITY, ST_BAD_INPUT = -6, -9


def resident_waves() -> int:
    """k_replay waves the device holds at once: 8 per SIMD, 4 SIMDs per compute unit"""
    import ctypes as C
    crdt_amd.lib()  # (the engine library brings the HIP runtime in)
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    cus = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(cus), 63, 0) == 0  # hipDeviceAttributeMultiprocessorCount
    assert 1 <= cus.value <= 1024, cus.value
    return 8 * 4 * cus.value


def check_board(e, policy):
    """after a launch (the copy-out waits for the stream): the launch ran with `policy` (0 none,
    1 the board, 2 the rotation); no slot of any launch keeps work left; this launch's stamp is on the board
    exactly when it ran with the board"""
    board, stamp, pol = e.balance_board()
    assert pol == policy and 1 <= stamp <= 255, (pol, stamp)
    dirty = np.argwhere((board & LEFT) != 0)
    assert dirty.shape[0] == 0, (dirty[:8], board[tuple(dirty[0])] if dirty.shape[0] else None)
    assert ((board >> 24) == stamp).any() == (policy == 1)
    return stamp


def state_of(e, docs=None):
    docs = range(e.n_docs) if docs is None else docs
    return dict(status=e.status(), digests=e.digests(), lens=e.lens(), export={d: e.export(d) for d in docs})


def assert_same_state(a, b):
    for k in ("status", "digests", "lens"):
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])
    assert a["export"].keys() == b["export"].keys()
    for d in a["export"]:
        x, y = a["export"][d], b["export"][d]
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), (d, k)


def grow_then_steady(e, policy, docs=None):
    """crdt_run from the tables' floors (launches that stop for capacity and resume), then the
    benchmark's steady step on the fitted engine (one launch, fused publish); the board is checked
    after both"""
    st = e.run()
    check_board(e, policy)
    e.publish_async()
    e.fit()
    e.reset_async()
    e.run_async()
    e.publish_async()
    e.sync()
    check_board(e, policy)
    assert np.array_equal(e.status(), st)
    return state_of(e, docs)


def on_and_off(leaf, n, stage, on="on", policy_on=1, docs=None):
    """stage(engine) on two engines, balance `on` and off; the two states are equal"""
    res = {}
    for mode, policy in ((on, policy_on), ("off", 0)):
        e = crdt_amd.Engine(n, leaf)
        e.replay_balance(mode)
        stage(e)
        res[mode] = grow_then_steady(e, policy, docs)
        e.close()
    assert_same_state(res[on], res["off"])
    return res[on]


MODES = [("on", 1), ("auto", 2)]  # (mode, the policy its launches run with while every wave is resident)


@pytest.mark.parametrize("mode,policy", MODES)
@pytest.mark.parametrize("leaf", [32, 4])
def test_one_document(leaf, mode, policy):
    # a lone wave ranks only itself: the highest level all the way
    s = on_and_off(leaf, 1, lambda e: e.apply_remote_wire([0], [micro_wire("typing")], stage_only=True), mode, policy)
    assert s["status"][0] == 0 and int(s["digests"][0]) == oracle_of("typing", leaf)[0]


UNEQUAL = ["typing", "bs10", "jump1", "del1", "sveltecomponent", "jump1", "typing", "sveltecomponent", "bs10"]


def unequal_wire(name):
    return load_remote_wire(name) if name == "sveltecomponent" else micro_wire(name)


@pytest.mark.parametrize("mode,policy", MODES)
@pytest.mark.parametrize("leaf", [32, 4])
def test_unequal_documents(leaf, mode, policy):
    # 9 documents of unequal length: more than 8, so at least two share a SIMD and rank differently
    # tick after tick.  9 waves fit resident: automatic mode (the default) balances them too
    def stage(e):
        e.apply_remote_wire(list(range(9)), [unequal_wire(m) for m in UNEQUAL], stage_only=True)

    s = on_and_off(leaf, 9, stage, mode, policy)
    assert (s["status"] == 0).all()
    for d, m in enumerate(UNEQUAL):
        want = golden_digest(m, leaf) if m == "sveltecomponent" else oracle_of(m, leaf)[0]
        assert int(s["digests"][d]) == want, m


@pytest.mark.parametrize("mode,policy", MODES)
@pytest.mark.parametrize("leaf", [32, 4])
def test_generated_ops(leaf, mode, policy):
    # the generated-op instance: the tick sits at the draws' refill, once per 64 ops
    s = on_and_off(leaf, 5, lambda e: e.stage_random(list(range(5)), "gen", 2000, 0xBA1A), mode, policy)
    assert (s["status"] == 0).all() and len(set(s["digests"].tolist())) == 5


@pytest.mark.parametrize("leaf", [32, 4])
def test_more_waves_than_resident(leaf):
    # one document more than the device holds at once: the launch runs in rounds and later waves
    # take over the slots of finished ones.  Automatic mode leaves such a launch alone (no stamped
    # write on the board); forced on, the state is still the same.  Status, digest and length are
    # compared for every document, the full export for every 512th and the last.
    n = resident_waves() + 1
    wire = micro_wire("typing")

    def stage(e):
        e.share_streams(True)
        e.stage_remote_replicated(wire, 0, ["u%05d" % i for i in range(n)])

    res = {}
    for mode, policy in (("on", 1), ("auto", 0)):
        e = crdt_amd.Engine(n, leaf)
        e.replay_balance(mode)
        stage(e)
        res[mode] = grow_then_steady(e, policy, list(range(0, n, 512)) + [n - 1])
        e.close()
    assert_same_state(res["on"], res["auto"])
    assert (res["on"]["status"] == 0).all() and (res["on"]["lens"] == oracle_of("typing", leaf)[1]).all()
    assert (res["on"]["digests"] == np.uint64(oracle_of("typing", leaf)[0])).all()


def test_automatic_mode_at_the_resident_capacity():
    # exactly as many documents as fit resident: still on (the rotation: nothing on the board)
    n = resident_waves()
    e = crdt_amd.Engine(n, 32)
    e.share_streams(True)
    e.stage_remote_replicated(micro_wire("typing"), 0, ["u%05d" % i for i in range(n)])
    e.run_async()
    e.sync()
    check_board(e, 2)
    e.close()


@pytest.mark.parametrize("leaf", [32, 4])
def test_bad_input_stop_clears_the_slot(leaf):
    # document 1's stream holds a zero-length remote op half-way: its wave stops there with
    # BAD_INPUT, after several ticks, and must leave its slot empty like the waves that finish
    names, txns = parse_wire(micro_wire("typing"))
    k = len(txns) // 2
    a, s, ps, ops = txns[k]
    txns[k] = (a, s, ps, [(op[0], op[1], op[2], op[3], op[4], 0) for op in ops])
    bad = build_wire(txns)

    def stage(e):
        e.apply_remote_wire([0, 1, 2], [micro_wire("typing"), bad, micro_wire("bs10")], stage_only=True)

    s = on_and_off(leaf, 3, stage)
    assert list(s["status"]) == [0, ST_BAD_INPUT, 0]
    assert int(s["digests"][0]) == oracle_of("typing", leaf)[0] and int(s["digests"][2]) == oracle_of("bs10", leaf)[0]


@pytest.mark.parametrize("leaf", [32, 4])
def test_capacity_stop_clears_the_slot(leaf):
    # a launch from the tables' floors with no growth around it (crdt_run_async): the documents stop
    # with NEED_CAPACITY mid-stream and their slots are empty; crdt_run then grows, resumes and ends
    # in the same state as with the balance off
    ms = ["del1", "jump10", "bs200"]
    res = {}
    for mode, policy in (("on", 1), ("off", 0)):
        e = crdt_amd.Engine(3, leaf)
        e.replay_balance(mode)
        e.apply_remote_wire([0, 1, 2], [micro_wire(m) for m in ms], stage_only=True)
        e.run_async()
        e.sync()
        check_board(e, policy)
        stopped = e.status()
        assert (stopped == ST_CAPACITY).any(), stopped
        assert (e.run() == 0).all()
        check_board(e, policy)
        res[mode] = state_of(e)
        res[mode]["stopped"] = stopped
        e.close()
    assert np.array_equal(res["on"].pop("stopped"), res["off"].pop("stopped"))
    assert_same_state(res["on"], res["off"])
    for d, m in enumerate(ms):
        assert int(res["on"]["digests"][d]) == oracle_of(m, leaf)[0]
