"""Reference definition of the authorship runs (Engine.blame / crdt_blame_async) — TEST INFRASTRUCTURE.

Walk the visible items of the current state in document order: the items of the canonical spans
with len > 0, expanded item by item.  Item number p of that walk is position p.  Its order x has,
through the client_with_order table, an id (agent, seq): what pos_to_loc answers for p.

A run is a maximal stretch of consecutive positions whose neighbours chain:

  mode "agent" (0)  the same agent
  mode "id"    (1)  the same agent, and the right item's seq is the left item's plus 1

A run is (pos, len, agent, seq) with agent and seq of its first item.  Deleted items are not part
of the walk, so two visible stretches with tombstones between them chain if their ids allow it.
The form is unique: results compare exactly.
"""
import numpy as np

MODES = {"agent": 0, "id": 1, 0: 0, 1: 1}


def item_ids(ex: dict):
    """(agent, seq) of every visible item in document order, from the `canon`, `cwo` and `next_order`
    tables of OracleDoc.export() / Engine.export()"""
    n = int(ex["next_order"])
    agent = np.full(n, -1, np.int64)
    seq = np.full(n, -1, np.int64)
    for key, ag, sq, ln in np.asarray(ex["cwo"], dtype=np.int64).reshape(-1, 4):
        for j in range(int(ln)):
            agent[key + j] = ag
            seq[key + j] = sq + j
    out = []
    for order, _ol, _orr, ln in np.asarray(ex["canon"], dtype=np.uint32).reshape(-1, 4):
        ln = int(np.int32(ln))
        for x in range(int(order), int(order) + max(ln, 0)):
            assert agent[x] >= 0, f"order {x} has no client_with_order run"
            out.append((int(agent[x]), int(seq[x])))
    return out


def chains(left, right, mode: int) -> bool:
    return left[0] == right[0] and (mode == 0 or right[1] == left[1] + 1)


def ref_blame(ex: dict, mode) -> np.ndarray:
    """runs [n, 4] u32 = (pos, len, agent, seq), item by item"""
    mode = MODES[mode]
    runs = []
    prev = None
    for p, cur in enumerate(item_ids(ex)):
        if prev is not None and chains(prev, cur, mode):
            runs[-1][1] += 1
        else:
            runs.append([p, 1, cur[0], cur[1]])
        prev = cur
    return np.array(runs, dtype=np.uint32).reshape(-1, 4)


def expand(runs: np.ndarray, mode):
    """(agent, seq) per position from runs; seq is None per item in agent mode"""
    mode = MODES[mode]
    agents, seqs = [], []
    for pos, ln, ag, sq in np.asarray(runs, dtype=np.int64).reshape(-1, 4):
        assert pos == len(agents), (pos, len(agents))
        agents += [int(ag)] * int(ln)
        seqs += [int(sq) + j for j in range(int(ln))] if mode == 1 else [None] * int(ln)
    return agents, seqs
