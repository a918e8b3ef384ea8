"""The rotation policy's level maps on the device (kernels.h balance_board_tick, balance_levels.h;
DESIGN §4): a priority changes when instructions issue, never what they compute, so what a map
can break is the kernel-argument word it travels in, its arithmetic at the tick, or the kernel's
register budget -- all of which show on any launch with more than one wave per SIMD.  For every map,
at both leaf layouts, 64 documents built from the eight micro wires and one automerge-paper document
replay in one launch with the rotation forced on; status, digests, lengths and the full exports are
compared byte for byte with the balance off (replayed once per layout), the launch reports the
rotation policy, and the board holds no slot with work left."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
from crdt_amd.traces import load_remote_wire  # noqa: E402
from test_gpu_fused_publish import micro_wire, oracle_of, golden_digest  # noqa: E402
from test_gpu_replay_balance import assert_same_state, check_board, grow_then_steady  # noqa: E402

MICRO = ["base", "bs10", "bs200", "del1", "fd200", "jump1", "jump10", "typing"]
NAMES = [MICRO[d % 8] for d in range(64)] + ["automerge-paper"]
MAPS = list(range(crdt_amd.BALANCE_MAPS))
_off = {}


def replay(leaf, mode, policy, bmap=None):
    e = crdt_amd.Engine(len(NAMES), leaf)
    e.replay_balance(mode)
    if bmap is not None:
        e.set_balance_map(bmap)
    wires = {m: micro_wire(m) for m in MICRO}
    wires["automerge-paper"] = load_remote_wire("automerge-paper")
    e.apply_remote_wire(list(range(len(NAMES))), [wires[m] for m in NAMES], stage_only=True)
    s = grow_then_steady(e, policy)  # (the board is checked after the growing replay and after the steady step)
    e.close()
    return s


def balance_off(leaf):
    if leaf not in _off:
        s = _off[leaf] = replay(leaf, "off", 0)
        assert (s["status"] == 0).all()
        for d, m in enumerate(NAMES):
            want = golden_digest(m, leaf) if m == "automerge-paper" else oracle_of(m, leaf)[0]
            assert int(s["digests"][d]) == want, m
    return _off[leaf]


@pytest.mark.parametrize("bmap", MAPS)
@pytest.mark.parametrize("leaf", [32, 4])
def test_map_leaves_the_state_alone(leaf, bmap):
    assert_same_state(replay(leaf, "rotate", 2, bmap), balance_off(leaf))


def test_map_numbers_are_checked():
    e = crdt_amd.Engine(1, 32)
    for bad in (-1, crdt_amd.BALANCE_MAPS):
        with pytest.raises(crdt_amd.CrdtError):
            e.set_balance_map(bad)
    e.set_balance_map(crdt_amd.BALANCE_MAPS - 1)
    e.replay_balance("auto")  # (one resident wave: automatic mode rotates it, with the map just set)
    e.apply_remote_wire([0], [micro_wire("typing")], stage_only=True)
    assert (e.run() == 0).all()
    check_board(e, 2)
    assert int(e.digests()[0]) == oracle_of("typing", 32)[0]
    e.close()
