"""The hostile compact-record streams of tests/hostile_streams.py on the CPU: the conditions the
families are built under (asserted, with counts), and every stream through the CPU emulation of the
replay (tests/emu: replay_core.h with a scanning backend) against the oracle, at both leaf layouts.
tests/test_gpu_hostile_streams.py replays the same streams on the engine, where the scans are
wave_gpu.h's lane-parallel forms."""
import pytest

import hostile_streams as hs
from emu_lib import EmuDoc, diff_states
from hostile_streams import records

LAYOUTS = (32, 4)


def test_families_are_complete():
    # 15 error families and 10 long-run ones, at 7 lanes, in 2 variants; 13 valid families at 7 pads
    assert len(hs.ERRORS) == 15 and len(hs.LONG_ERRORS) == 2 * len(hs.RUN_BAD_AT) == 10
    err, ok = hs.error_cases(), hs.valid_cases()
    assert len(err) == (15 + 10) * len(hs.LANES) * 2 == 350
    assert len(ok) == 13 * len(hs.LANES) == 91
    assert len({c.name for c in err + ok}) == 441
    assert hs.LANES == (0, 1, 30, 61, 62, 63, 64)


def test_stream_shapes():
    # a stream batch is compact records only (so txn k is record k, lane k of the first window),
    # but for the families that need one general-form txn; every stream stays within 200 txns
    for c in hs.error_cases() + hs.valid_cases():
        assert len(c.stream) <= 200, c.name
        if c.family not in hs.GENERAL_FORM:
            assert records(c.stream) == len(c.stream), c.name
        else:
            assert records(c.stream) > len(c.stream), c.name
    # the bad record sits where the case says: on the lane, or behind the family's own first records
    for c in hs.error_cases():
        if c.family in hs.LONG_ERRORS:
            assert c.bad == c.lane + int(c.family.rsplit("bad", 1)[-1].rsplit("gap", 1)[-1]), c.name
        else:
            assert c.bad >= c.lane and (c.bad == c.lane or c.lane < 8), c.name
            if c.family not in hs.GENERAL_FORM:
                assert records(c.stream[:c.bad]) == c.bad
        assert (c.bad == len(c.stream) - 1) == c.name.endswith("_last"), c.name
    on_lane = {c.lane for c in hs.error_cases() if c.bad == c.lane}
    assert on_lane == {30, 61, 62, 63, 64}  # (lanes 0 and 1 hold the bad record of the long runs' pads only)
    long_lanes = {c.bad for c in hs.error_cases() if c.family in hs.LONG_ERRORS}
    assert {1, 2, 62, 63, 64, 65, 100, 126, 127, 128, 164} <= long_lanes


@pytest.mark.parametrize("L", LAYOUTS)
def test_oracle_statuses_do_not_depend_on_the_lane(L):
    # conditions on the families, not measurements: every error case has the family's status at
    # every lane and in both variants (so never 0), every valid case has status 0; none is skipped
    res = hs.oracle_results(L)
    wrong = [(c.name, res[c.name][0], c.want) for c in hs.error_cases() + hs.valid_cases() if res[c.name][0] != c.want]
    assert not wrong, (len(wrong), wrong[:10])
    assert sum(res[c.name][0] != 0 for c in hs.error_cases()) == 350
    assert sum(res[c.name][0] == 0 for c in hs.valid_cases()) == 91
    assert {c.want for c in hs.error_cases()} == {-2, -4, -5, -9}


@pytest.mark.parametrize("L", LAYOUTS)
def test_emulated_replay_matches_oracle(L):
    res = hs.oracle_results(L)
    bad = []
    for c in hs.error_cases() + hs.valid_cases():
        want, o = res[c.name]
        whole = c.wires[2]  # (an EmuDoc replays one stream from an empty document: base and stream as one wire)
        e = EmuDoc(L)
        st = e.run_wire(whole)
        if st != want:
            bad.append((c.name, "one wire", st, want))
        elif want == 0 and (e.check() != "" or diff_states(e.export(), o.export())):
            bad.append((c.name, "one wire", e.check(), diff_states(e.export(), o.export())[:1]))
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("L", LAYOUTS)
def test_parent_limit(L):
    # a txn holds at most 65,535 parents (the record header's 16-bit field; include/crdt_gpu.h):
    # with 65,535 the replay equals the oracle; with 65,536 the document stops at that txn with
    # CRDT_ERR_BAD_INPUT (-9), holding what the wire's txns before it made (the oracle, which has
    # no such limit, applies the txn)
    from oracle_lib import OracleDoc
    lay = {32: (32, 16), 4: (4, 8)}[L]
    w, _head = hs.parent_limit_wires(65535)
    o, e = OracleDoc(*lay), EmuDoc(L)
    assert o.apply_remote_wire(w) == 0 and e.run_wire(w) == 0
    assert e.check() == "" and diff_states(e.export(), o.export()) == []
    w, head = hs.parent_limit_wires(65536)
    o, o2, e = OracleDoc(*lay), OracleDoc(*lay), EmuDoc(L)
    assert o.apply_remote_wire(w) == 0 and o2.apply_remote_wire(head) == 0
    assert e.run_wire(w) == -9
    assert e.check() == "" and diff_states(e.export(), o2.export()) == []
