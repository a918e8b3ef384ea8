"""Reference definition of causal versions given as version vectors (Engine.version_vector /
Engine.diff_vv / Engine.diff_vv_closed, include/crdt_gpu.h "Causal versions") -- TEST INFRASTRUCTURE.

A version vector vv of a document names, per agent id, how many of its seqs have been seen (entries
beyond its length count as 0).  The version is the set S of orders x whose id (agent, seq) in
client_with_order has seq < vv[agent]: insert items and delete ops alike.  An item with order x is
visible at S when

  x is in S, and no delete-log entry (key, target, len) covers x with its delete order
  key + (x - target) in S.

ref_diff_vv is tests/diff_between_ref.py's walk, item by item, with "visible at a / b" replaced by
"visible at S_from / S_to".  An order prefix "every order below v" is such a set (an agent's seqs
are applied in seq order): ref_version_vector gives its vector, and on those vectors ref_diff_vv
is ref_diff_between.

Sets of orders are boolean arrays over the orders 0 .. next_order - 1.
"""
import numpy as np

ROOT_ORDER = 0xFFFFFFFF


def ids_by_order(ex: dict):
    """(agent, seq) of every order, from client_with_order (key, agent, seq, len); kept with the
    export under "_ids_by_order" (an export is not changed after it is made)"""
    if "_ids_by_order" not in ex:
        ex["_ids_by_order"] = _ids_by_order(ex)
    return ex["_ids_by_order"]


def _ids_by_order(ex: dict):
    cwo = np.asarray(ex["cwo"], dtype=np.int64).reshape(-1, 4)
    n = int(ex["next_order"])
    agent, seq = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for key, a, s, ln in cwo:
        agent[key:key + ln] = a
        seq[key:key + ln] = s + np.arange(ln)
    assert int(cwo[:, 3].sum()) == n  # (every order has an id)
    return agent, seq


def next_seqs(ex: dict) -> np.ndarray:
    """per agent id that has an order: its next seq (the largest entry a vector may hold)"""
    agent, seq = ids_by_order(ex)
    out = np.zeros(int(agent.max()) + 1 if agent.size else 0, dtype=np.int64)
    np.maximum.at(out, agent, seq + 1)
    return out


def ref_version_vector(ex: dict, v: int, n_agents=None) -> np.ndarray:
    """the vector of the order prefix v: per agent, its seqs among the orders below v"""
    v = int(v)
    if not 0 <= v <= int(ex["next_order"]):
        raise ValueError(f"version {v} outside [0, {int(ex['next_order'])}]")
    agent, seq = ids_by_order(ex)
    out = np.zeros(len(next_seqs(ex)) if n_agents is None else int(n_agents), dtype=np.int64)
    np.maximum.at(out, agent[:v], seq[:v] + 1)
    return out.astype(np.uint32)


def members(ex: dict, vv) -> np.ndarray:
    """S: the orders whose (agent, seq) has seq < vv[agent]; raises for a vector out of bounds"""
    nxt = next_seqs(ex)
    have = np.zeros(max(len(nxt), len(vv)), dtype=np.int64)
    have[:len(vv)] = np.asarray(vv, dtype=np.int64)
    top = np.zeros_like(have)
    top[:len(nxt)] = nxt
    if (have > top).any():
        raise ValueError(f"vector {have.tolist()} above the agents' next seqs {top.tolist()}")
    agent, seq = ids_by_order(ex)
    return seq < have[agent]


def deleted_by(ex: dict, S: np.ndarray) -> np.ndarray:
    """the items covered by a delete-log entry with its delete order in S"""
    out = np.zeros(S.shape[0], dtype=bool)
    for key, target, ln in np.asarray(ex["deletes"], dtype=np.int64).reshape(-1, 3):
        out[target:target + ln] |= S[key:key + ln]
    return out


def items(ex: dict) -> np.ndarray:
    """the orders of every item of the current state, in document order"""
    canon = np.asarray(ex["canon"], dtype=np.uint32).reshape(-1, 4)
    first = canon[:, 0].astype(np.int64)
    ln = np.abs(canon[:, 3].astype(np.int32)).astype(np.int64)
    return np.repeat(first, ln) + (np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln))


def visible(ex: dict, vv) -> np.ndarray:
    S = members(ex, vv)
    return S & ~deleted_by(ex, S)


def text_at(ex: dict, vv) -> np.ndarray:
    """the visible items of S in document order, as orders"""
    x = items(ex)
    return x[visible(ex, vv)[x]].astype(np.uint32)


def ref_diff_vv(ex: dict, vv_from, vv_to):
    """ex: the `canon`, `deletes`, `cwo` and `next_order` tables of OracleDoc.export() / Engine.export().
    Returns (patches [n, 4] u32 = (pos, del_len, ins_len, ins_off), ins_order [n_ins] u32)."""
    vis_a, vis_b = visible(ex, vv_from), visible(ex, vv_to)
    patches, ins = [], []
    cur = None      # the open patch: [pos, del_len, ins_len, ins_off]
    seen = 0        # new items walked so far
    for x in items(ex).tolist():
        old, new = bool(vis_a[x]), bool(vis_b[x])
        if old and new:                  # K
            cur = None
        elif old or new:                 # D or I
            if cur is None:
                cur = [seen, 0, 0, len(ins)]
                patches.append(cur)
            if old:
                cur[1] += 1
            else:
                cur[2] += 1
                ins.append(x)
        seen += new
    return np.array(patches, dtype=np.uint32).reshape(-1, 4), np.array(ins, dtype=np.uint32)


def ref_vv_closed(ex: dict, vv) -> bool:
    """S is causally closed: every txn (a row of `txns`: order, len, shadow, poff, pn) with at least
    one order in S has all its parents but ROOT in S, and S holds a prefix of every txn it touches"""
    S = members(ex, vv)
    par = np.asarray(ex["parents"], dtype=np.int64)
    for order, ln, _shadow, poff, pn in np.asarray(ex["txns"], dtype=np.int64).reshape(-1, 5):
        inside = S[order:order + ln]
        k = int(inside.sum())
        if k == 0:
            continue
        if not inside[:k].all():         # (a member after a non-member)
            return False
        for p in par[poff:poff + pn]:
            if int(p) != ROOT_ORDER and not S[int(p)]:
                return False
    return True
