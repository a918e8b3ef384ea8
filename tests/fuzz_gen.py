"""Seeded workload generators shared by CPU (emulator) and GPU parity tests — TEST INFRASTRUCTURE.

random_local_trace: the reference's make_random_change (doc.rs:544-569): insert weight 0.55 if
len < 100 else 0.45; insert 1 char at U[0, len]; delete U[1, min(10, len-pos)] at U[0, len-1].
concurrent_wire: several agents editing their own replicas (oracle) and exchanging remote txns;
returns one causally ordered wire batch that replays the whole history.
gossip_log / causal_shuffle / gossip_family: partially delivered concurrent histories (every agent
pulls from one peer at a time) and seeded causal reorderings of them.
multi_op_wire / multi_op_family: concurrent_wire's scheme with local txns of 1..4 ops (replaces,
typing on, deletes inside the txn's own insert): multi-op remote txns in a concurrent history.
"""
import bisect
import functools
import os
import random
import struct

import numpy as np


def random_local_trace(seed: int, n_ops: int, ins_max: int = 1):
    rng = random.Random(seed)
    n = 0
    patches = []
    for _ in range(n_ops):
        w = 0.55 if n < 100 else 0.45
        if n == 0 or rng.random() < w:
            pos = rng.randint(0, n)
            k = rng.randint(1, ins_max)
            patches.append((pos, 0, k))
            n += k
        else:
            pos = rng.randint(0, n - 1)
            span = rng.randint(1, min(10, n - pos))
            patches.append((pos, span, 0))
            n -= span
    p = np.array(patches, dtype=np.uint32).reshape(-1, 3)
    return np.ones(p.shape[0], np.uint32), p


def parse_wire(w: bytes):
    """wire -> (names, txns[(agent, seq, parents[(name,seq)], ops[(kind,a,as,b,bs,len)])])."""
    off = 0

    def rd():
        nonlocal off
        v = struct.unpack_from("<I", w, off)[0]
        off += 4
        return v
    assert rd() == 0x31585452
    names = []
    for _ in range(rd()):
        bl = rd()
        names.append(w[off:off + bl].decode())
        off += (bl + 3) & ~3
    txns = []
    for _ in range(rd()):
        a, s, np_, no = rd(), rd(), rd(), rd()
        ps = [(names[rd()], rd()) for _ in range(np_)]
        ops = []
        for _ in range(no):
            k, an, asq, bn, bsq, ln = rd(), rd(), rd(), rd(), rd(), rd()
            ops.append((k, names[an], asq, names[bn] if k == 0 else None, bsq, ln))
        txns.append((names[a], s, ps, ops))
    return names, txns


def build_wire(txns):
    names = []

    def ni(n):
        if n not in names:
            names.append(n)
        return names.index(n)
    body = []
    for agent, seq, parents, ops in txns:
        body += [ni(agent), seq, len(parents), len(ops)]
        for pn, ps in parents:
            body += [ni(pn), ps]
        for k, an, asq, bn, bsq, ln in ops:
            body += [k, ni(an), asq, ni(bn) if k == 0 else 0, bsq if k == 0 else 0, ln]
    out = struct.pack("<II", 0x31585452, len(names))
    for n in names:
        b = n.encode()
        out += struct.pack("<I", len(b)) + b + b"\0" * ((4 - len(b) % 4) % 4)
    return out + struct.pack("<I", len(txns)) + np.array(body, dtype=np.uint32).tobytes()


def concurrent_wire(seed: int, n_agents: int = 3, rounds: int = 6, ops_per_round: int = 4, base_len: int = 20):
    """Agents edit replicas concurrently each round, then everyone merges everything.

    Uses the oracle's local->remote recorder per replica.  Returns (wire, n_txns).
    """
    from oracle_lib import OracleDoc, lib, _p
    import ctypes as C
    rng = random.Random(seed)
    L = lib()
    names = [f"agent{chr(97 + i)}{rng.randint(0, 9)}" for i in range(n_agents)]
    history = []  # causally ordered txn list (parsed)

    def record(doc, agent_id, ops):
        c = np.array([len(ops)], np.uint32)
        p = np.array(ops, np.uint32).reshape(-1, 3)
        n = L.orc_local_trace_to_wire(doc.h, agent_id, 1, _p(c), _p(p), None, 0)
        # the sizing call applied the txn; fetch the bytes by re-running on a twin is not possible,
        # so record via a scratch buffer call instead (apply once):
        raise RuntimeError("use record2")

    def record2(doc, agent_id, ops):
        c = np.array([len(ops)], np.uint32)
        p = np.array(ops, np.uint32).reshape(-1, 3)
        buf = C.create_string_buffer(1 << 20)
        n = L.orc_local_trace_to_wire(doc.h, agent_id, 1, _p(c), _p(p), C.cast(buf, C.c_void_p), 1 << 20)
        if n < 0:
            return None
        return parse_wire(buf.raw[:n])[1]

    reps = []
    seen = []
    for i in range(n_agents):
        d = OracleDoc()
        reps.append(d)
        seen.append(0)
    # base document by agent 0, delivered to everyone
    a0 = reps[0].agent(names[0])
    tx = record2(reps[0], a0, [(0, 0, base_len)])
    history += tx
    seen[0] = len(history)
    for r in range(rounds):
        # deliver everything not yet seen
        for i in range(n_agents):
            new = history[seen[i]:]
            if new and i != 0 or (new and seen[i] < len(history)):
                if reps[i].apply_remote_wire(build_wire(new)) != 0:
                    return build_wire(history), len(history)
            seen[i] = len(history)
        snapshot = len(history)
        round_txns = []
        for i in range(n_agents):
            ai = reps[i].agent(names[i])
            for _ in range(ops_per_round):
                n = len(reps[i])
                if n == 0 or rng.random() < 0.6:
                    op = (rng.randint(0, n), 0, rng.randint(1, 3))
                else:
                    pos = rng.randint(0, n - 1)
                    op = (pos, rng.randint(1, min(4, n - pos)), 0)
                t = record2(reps[i], ai, [op])
                if t is None:
                    break
                round_txns.append((i, t))
        # deliver in a shuffled but per-agent-ordered interleaving
        order = list(range(len(round_txns)))
        per = {}
        for k, (i, t) in enumerate(round_txns):
            per.setdefault(i, []).append(t)
        seq = []
        while any(per.values()):
            i = rng.choice([k for k, v in per.items() if v])
            seq += per[i].pop(0)
        history += seq
        for i in range(n_agents):
            # each agent already has its own txns; mark them seen via full re-delivery of others
            others = [t for t in history[snapshot:] if t[0] != names[i]]
            if others and reps[i].apply_remote_wire(build_wire(others)) != 0:
                return build_wire(history), len(history)
            seen[i] = len(history)
    return build_wire(history), len(history)


MULTI_OP_KINDS = ("replace", "delete", "insert", "typing_on", "delete_inside")
MULTI_OP_WEIGHTS = (0.2, 0.15, 0.25, 0.25, 0.15)


def draw_multi_op_txn(rng, n: int, end_ok: bool = False):
    """One local txn of 1..4 LocalOps (pos, del, ins) on a text of `n` items, each op drawn against
    the length the ops before it leave.  Kinds (MULTI_OP_KINDS, drawn with MULTI_OP_WEIGHTS):
    a replace (delete 1..3 and insert 1..3 at one position), a plain delete of 1..4, a plain insert
    of 1..3, typing on (an insert directly after the txn's previous insert: its origin_left is an
    item of its own txn) and a delete inside the txn's previous insert (its target is an item of
    its own txn).  A kind that cannot be drawn (no previous insert, too short a text) falls back
    to a plain insert.  Unless `end_ok`, nothing is inserted after the text's last item and no
    delete leaves fewer than 2 items (gossip_log's ERR_NONTERMINATING restriction).
    Returns (ops, the text's length after them)."""
    ops = []
    last = None  # (pos, len) of the txn's previous insert, in the text as it is now
    hi = 0 if end_ok else 1  # inserts land in [0, n - hi]
    for _ in range(rng.randint(1, 4)):
        kind = rng.choices(MULTI_OP_KINDS, MULTI_OP_WEIGHTS)[0]
        op = None
        if kind == "replace" and n - hi >= 2 and n >= 3:
            d = rng.randint(1, min(3, n - hi - 1, n - 2))
            p = rng.randint(0, n - hi - d)
            i = rng.randint(1, 3)
            op, new_last = (p, d, i), (p, i)
        elif kind == "delete" and n >= 3:
            p = rng.randint(0, n - 2)
            d = rng.randint(1, min(4, n - p, n - 2))
            op = (p, d, 0)
            if last is None or p >= last[0] + last[1]:
                new_last = last
            elif p + d <= last[0]:
                new_last = (last[0] - d, last[1])
            else:
                new_last = None
        elif kind == "typing_on" and last is not None and last[0] + last[1] <= n - hi:
            i = rng.randint(1, 3)
            op, new_last = (last[0] + last[1], 0, i), (last[0], last[1] + i)
        elif kind == "delete_inside" and last is not None and n >= 3:
            p = rng.randint(last[0], last[0] + last[1] - 1)
            d = rng.randint(1, min(2, last[0] + last[1] - p, n - 2))
            op, new_last = (p, d, 0), ((last[0], last[1] - d) if last[1] > d else None)
        if op is None:  # a plain insert, also the fall-back
            p = rng.randint(0, max(n - hi, 0))
            i = rng.randint(1, 3)
            op, new_last = (p, 0, i), (p, i)
        ops.append(op)
        n += op[2] - op[1]
        last = new_last
    return ops, n


def multi_op_wire(seed: int, n_agents: int = 3, rounds: int = 6, txns_per_round: int = 3, base_len: int = 20,
                  leaf: int = 32):
    """concurrent_wire's scheme with multi-op txns: every agent edits an oracle replica of its own
    (layout `leaf`), each local txn is draw_multi_op_txn's 1..4 LocalOps recorded through the
    oracle's local->remote recorder as ONE remote txn (a replace, a delete the recorder splits at a
    client_with_order run boundary and every further LocalOp add wire ops), delivery within a round
    is shuffled but keeps each agent's order, and at the end of a round everyone merges.  The
    history is truncated where a merge fails.  So the remote txns insert and delete, insert twice,
    name items their own earlier ops created and delete parts of their own inserts -- the shapes
    only apply_txn's interpreter replays -- in a history whose frontier has several heads.
    Returns (wire, n_txns) like concurrent_wire."""
    from oracle_lib import OracleDoc, lib, _p
    import ctypes as C
    rng = random.Random(seed)
    L = lib()
    names = [f"m{chr(97 + i)}{rng.randrange(1 << 12):03x}" for i in range(n_agents)]
    buf = C.create_string_buffer(1 << 16)

    def record(doc, agent_id, ops):
        c = np.array([len(ops)], np.uint32)
        p = np.array(ops, np.uint32).reshape(-1, 3)
        n = L.orc_local_trace_to_wire(doc.h, agent_id, 1, _p(c), _p(p), C.cast(buf, C.c_void_p), 1 << 16)
        return None if n < 0 else parse_wire(buf.raw[:n])[1]

    reps = [OracleDoc(leaf, 16 if leaf == 32 else 8) for _ in range(n_agents)]
    ids = [reps[i].agent(names[i]) for i in range(n_agents)]
    history = record(reps[0], ids[0], [(0, 0, base_len)])
    for i in range(1, n_agents):
        if reps[i].apply_remote_wire(build_wire(history)) != 0:
            return build_wire(history), len(history)
    for _ in range(rounds):
        snapshot = len(history)
        per = {}
        for i in range(n_agents):
            for _ in range(txns_per_round):
                ops, _n = draw_multi_op_txn(rng, len(reps[i]))
                t = record(reps[i], ids[i], ops)
                if t is None:
                    break
                per.setdefault(i, []).append(t)
        while any(per.values()):  # a shuffled interleaving that keeps each agent's order
            i = rng.choice([k for k, v in per.items() if v])
            history += per[i].pop(0)
        for i in range(n_agents):
            others = [t for t in history[snapshot:] if t[0] != names[i]]
            if others and reps[i].apply_remote_wire(build_wire(others)) != 0:
                return build_wire(history), len(history)
    return build_wire(history), len(history)


# the committed histories of tests/test_multi_op_ref.py, tests/test_gpu_multi_op.py: per seed
# (n_agents, rounds)
MULTI_OP_SEEDS = range(40)


def multi_op_params(seed: int) -> dict:
    return dict(n_agents=2 + seed % 4, rounds=4 + seed % 3)


@functools.lru_cache(maxsize=None)
def multi_op_family():
    """[(seed, wire)] of the committed multi-op histories; generated once per process"""
    return [(s, multi_op_wire(s, **multi_op_params(s))[0]) for s in MULTI_OP_SEEDS]


def txn_shape(t):
    """shape flags of one parsed remote txn: (mixed, two_inserts, own_origin inserts, own_target
    deletes, five_ops) -- an own origin / target is an id of the txn's author inside the txn's own
    seq range"""
    a, s, _ps, ops = t
    end = s + sum(op[5] for op in ops)
    n_ins = sum(op[0] == 0 for op in ops)
    own_o = sum(1 for k, an, asq, bn, bsq, _ln in ops
                if k == 0 and ((an == a and s <= asq < end) or (bn == a and s <= bsq < end)))
    own_t = sum(1 for k, an, asq, _bn, _bsq, ln in ops if k != 0 and an == a and asq < end and asq + ln > s)
    return (0 < n_ins < len(ops), n_ins >= 2, own_o, own_t, len(ops) >= 5)


def config5_wire(seed: int, base_len: int = 4096, n_agents: int = 16, rounds: int = 8, ops: int = 4,
                 hot: int = 32, del_frac: float = 0.6):
    """BASELINE config 5 shape: concurrent, deletion-heavy.

    Agent "base" inserts `base_len` chars (one txn, contiguous orders).  Then `rounds` rounds: each
    of `n_agents` agents makes `ops` single-op txns against the round-start snapshot -- 60 %
    deletes of 1..64 base items (contiguous targets, Q4; overlapping deletes make double deletes),
    40 % inserts of 1..8 chars at one of `hot` shared hotspots (origin_left = base item h,
    origin_right = base item h+1, so concurrent inserts tie in integrate's Equal branch).  A txn's
    parents are the round-start frontier (first txn of the agent in the round) or the agent's
    previous txn.  Delivery within a round is a seeded interleaving that keeps each agent's order.
    Returns the wire batch (one causally ordered history)."""
    rng = random.Random(seed)
    names = [f"a{i:02d}_{rng.randrange(1 << 20):05x}" for i in range(n_agents)]
    R = ("ROOT", 0xFFFFFFFF)
    txns = [("base", 0, [R], [(0, "ROOT", R[1], "ROOT", R[1], base_len)])]
    hotspots = sorted(rng.sample(range(base_len - 1), min(hot, base_len - 1)))
    frontier = [("base", base_len - 1)]
    seq = {a: 0 for a in names}
    for _ in range(rounds):
        per_agent = {}
        for a in names:
            lst, parents = [], list(frontier)
            for _ in range(ops):
                if rng.random() < del_frac:
                    ln = rng.randint(1, min(64, base_len))
                    s = rng.randrange(0, base_len - ln + 1)
                    op = (1, "base", s, None, 0, ln)
                else:
                    h = rng.choice(hotspots)
                    ln = rng.randint(1, 8)
                    op = (0, "base", h, "base", h + 1, ln)
                lst.append((a, seq[a], parents, [op]))
                seq[a] += ln
                parents = [(a, seq[a] - 1)]
            per_agent[a] = lst
        while any(per_agent.values()):
            a = rng.choice([k for k, v in per_agent.items() if v])
            txns.append(per_agent[a].pop(0))
        frontier = [(a, seq[a] - 1) for a in names]
    return build_wire(txns)


def gossip_log(seed: int, n_agents: int = 4, steps: int = 200, base_len: int = 16, p_edit: float = 0.7,
               p_ins: float = 0.65, ins_max: int = 3, hot=None, leaf: int = 32, del_max: int = 1):
    """A concurrent history with partial delivery: A may have seen B's txns but not C's.

    Every agent edits an oracle replica of its own (layout `leaf`) and a set records which txns it
    knows.  Agent 0 inserts `base_len` chars and everyone receives that txn.  Then `steps` times a
    random agent either (probability `p_edit`) makes one local single-op txn, recorded through the
    oracle's local->remote recorder like concurrent_wire's record2, or pulls from one random peer:
    every txn the peer knows and it does not, in log order, as one remote batch.  An edit is an
    insert of 1..`ins_max` chars with probability `p_ins`, at a position in [0, len-1] (with
    probability 0.7 one of the absolute positions `hot`, clamped to len-1), else a delete of
    1..`del_max` chars at a position in [0, len-2].  So an insert's origins are often another
    agent's items that a third agent has not seen, agents first appear at a receiver in the middle
    of a history, and integrate's scan meets entries left and right of the new item's origin_left.

    Two restrictions, both limits of the reference that the oracle restates:
      - no insert at the document's end: concurrent scans would run off the document
        (ERR_NONTERMINATING, as in test_error_statuses_match);
      - `del_max` = 1 by default: a remote delete of several items assumes their orders are
        contiguous at the receiver, and under partial delivery they are not (ERR_UNKNOWN_ID).  With
        `del_max` > 1 some histories stop with an error status; if a pull fails during generation
        the history is truncated there, as concurrent_wire does.

    Returns the parsed txn log in creation order, which is one causal order.  Delivery orders do
    NOT converge in the restated reference: the final id sequence of one history differs between
    causal orders (entry merging depends on arrival order).  The engine's contract
    is bit-exactness against the oracle for EACH order; do not add a convergence check here."""
    from oracle_lib import OracleDoc, lib, _p
    import ctypes as C
    rng = random.Random(seed)
    L = lib()
    names = [f"g{rng.randrange(1 << 16):04x}{i}" for i in range(n_agents)]
    reps = [OracleDoc(leaf, 16 if leaf == 32 else 8) for _ in range(n_agents)]
    ids = [None] * n_agents
    known = [set() for _ in range(n_agents)]
    log = []
    buf = C.create_string_buffer(1 << 16)

    def record(i, op):
        if ids[i] is None:
            ids[i] = reps[i].agent(names[i])
        c = np.array([1], np.uint32)
        p = np.array([op], np.uint32).reshape(-1, 3)
        n = L.orc_local_trace_to_wire(reps[i].h, ids[i], 1, _p(c), _p(p), C.cast(buf, C.c_void_p), 1 << 16)
        assert n > 0, (n, seed, op)
        for t in parse_wire(buf.raw[:n])[1]:
            known[i].add(len(log))
            log.append(t)

    record(0, (0, 0, base_len))
    for i in range(1, n_agents):
        assert reps[i].apply_remote_wire(build_wire(log)) == 0
        known[i] |= known[0]
    for _ in range(steps):
        i = rng.randrange(n_agents)
        if rng.random() < p_edit:
            n = len(reps[i])
            if n < 2 or rng.random() < p_ins:
                if hot and rng.random() < 0.7:
                    pos = min(rng.choice(hot), n - 1)
                else:
                    pos = rng.randint(0, n - 1)
                record(i, (pos, 0, rng.randint(1, ins_max)))
            else:
                pos = rng.randint(0, n - 2)
                record(i, (pos, rng.randint(1, min(del_max, n - 1 - pos)), 0))
        else:
            j = rng.choice([k for k in range(n_agents) if k != i])
            new = sorted(known[j] - known[i])
            if new:
                if reps[i].apply_remote_wire(build_wire([log[k] for k in new])) != 0:
                    return log
                known[i] |= known[j]
    return log


def causal_deps(log):
    """Per txn of a parsed log, the set of log indexes it depends on: the txns holding its parents,
    its agent's previous txn (the one whose seq range ends where this one starts), and the txns
    holding every id its ops name -- both origins of an insert, every item of a delete's target."""
    starts, owners = {}, {}
    for k, (a, s, _ps, _ops) in enumerate(log):
        starts.setdefault(a, []).append(s)  # (an agent's txns appear in seq order in any causal log)
        owners.setdefault(a, []).append(k)

    def owner(a, s):
        return owners[a][bisect.bisect_right(starts[a], s) - 1]
    deps = []
    for k, (a, s, ps, ops) in enumerate(log):
        d = set()
        for pn, pq in ps:
            if pn != "ROOT":
                d.add(owner(pn, pq))
        if s > 0:
            d.add(owner(a, s - 1))
        for kind, an, asq, bn, bsq, ln in ops:
            if kind == 0:
                for nm, sq in ((an, asq), (bn, bsq)):
                    if nm != "ROOT":
                        d.add(owner(nm, sq))
            else:
                d.update(owner(an, asq + j) for j in range(ln))
        d.discard(k)
        deps.append(d)
    return deps


def causal_shuffle(log, seed: int):
    """A seeded random topological order of a parsed log under causal_deps: a permutation of the
    log that every replica could have received.  (The replayed state depends on the order; see
    gossip_log.)"""
    rng = random.Random(seed)
    deps = causal_deps(log)
    waiting = [len(d) for d in deps]
    children = [[] for _ in log]
    for k, d in enumerate(deps):
        for x in d:
            children[x].append(k)
    ready = [k for k, w in enumerate(waiting) if w == 0]
    out = []
    while ready:
        i = rng.randrange(len(ready))
        ready[i], ready[-1] = ready[-1], ready[i]
        k = ready.pop()
        out.append(log[k])
        for c in children[k]:
            waiting[c] -= 1
            if waiting[c] == 0:
                ready.append(c)
    assert len(out) == len(log)
    return out


# the gossip families of tests/test_gossip_ref.py, tests/test_emu_parity.py and tests/test_gpu_gossip.py
# (all: p_ins 0.65, ins_max 3).  A: small; B: three hotspots; D: two hotspots, 8 agents, edit-heavy:
# the deep scans; E: 70 agents, past the 64 name ranks kept in LDS and the 25 frontier heads kept
# in lanes; X: B with deletes of 1..4 items: the family whose histories can stop with an error.
GOSSIP_FAMILIES = {
    "A": dict(n_agents=4, steps=300, base_len=16),
    "B": dict(n_agents=6, steps=600, hot=[3, 7, 11], p_edit=0.8),
    "D": dict(n_agents=8, steps=1500, hot=[2, 9], p_edit=0.85, base_len=12),
    "E": dict(n_agents=70, steps=2500, hot=[4], p_edit=0.8),
    "X": dict(n_agents=6, steps=600, hot=[3, 7, 11], p_edit=0.8, del_max=4),
}
GOSSIP_SEEDS = {"A": range(4), "B": range(4), "D": range(4), "E": range(4), "X": range(4)}
GOSSIP_ORDERS = 3  # the log order and two causal shuffles


@functools.lru_cache(maxsize=None)
def gossip_family(name: str):
    """Every history of a family as wire batches: [(seed, order, wire)], order 0 = the log order,
    1 and 2 = causal shuffles; generated once per process."""
    out = []
    for seed in GOSSIP_SEEDS[name]:
        log = gossip_log(seed, **GOSSIP_FAMILIES[name])
        out.append((seed, 0, build_wire(log)))
        for k in range(1, GOSSIP_ORDERS):
            out.append((seed, k, build_wire(causal_shuffle(log, 1000 * k + seed))))
    return out


def config1_probes(counts, patches, agent: int, seed=None):
    """BASELINE config 1's per-op check: after every txn, pos_to_loc(the txn's first op position)
    and loc_to_pos(the txn's first item = (agent, seq of its first order)).  With `seed`, every
    other probe instead asks a random position (up to 2 past the end) and a random earlier seq."""
    c = np.asarray(counts, dtype=np.int64)
    p = np.asarray(patches, dtype=np.int64).reshape(-1, 3)
    first_op = np.concatenate([[0], np.cumsum(c)[:-1]])
    op_len = p[:, 1] + p[:, 2]
    txn_len = np.add.reduceat(op_len, first_op) if len(c) else np.zeros(0, np.int64)
    seq0 = np.concatenate([[0], np.cumsum(txn_len)[:-1]])
    pr = np.stack([p[first_op, 0], np.full(len(c), agent), seq0], 1)
    if seed is not None:
        rng = np.random.default_rng(seed)
        k = np.arange(len(c)) % 2 == 1
        pr[k, 0] = rng.integers(0, np.maximum(p[first_op[k], 0] + 3, 1))
        pr[k, 2] = rng.integers(0, seq0[k] + txn_len[k])
    return pr.astype(np.uint32)


_GEN = None


def _gen_lib():
    """tests/gen/build/libgen.so (C++ config-5 history generator; built on first use)."""
    global _GEN
    if _GEN is None:
        import ctypes as C
        import fcntl
        import subprocess
        d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gen")
        os.makedirs(os.path.join(d, "build"), exist_ok=True)
        with open(os.path.join(d, "build", ".lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.run(["make", "-s", "-C", d], check=True)
        L = C.CDLL(os.path.join(d, "build", "libgen.so"))
        L.c5_gen_batch.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_double, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.c5_free.argtypes = [C.c_void_p]
        _GEN = L
    return _GEN


def config5_wires(seeds, base_len: int = 1 << 20, n_agents: int = 16, rounds: int = 64, ops: int = 64,
                  hot: int = 32, del_frac: float = 0.6, threads: int = 8):
    """BASELINE config 5 histories from the C++ generator (tests/gen/config5_gen.cpp): the shape of
    config5_wire above, one history per seed (its own ops and its own delivery interleaving),
    generated on `threads` threads.  Returns a list of wire batches (bytes)."""
    import ctypes as C
    L = _gen_lib()
    sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
    n = int(sd.shape[0])
    ptr = (C.c_void_p * n)()
    ln = np.zeros(n, np.uint64)
    rc = L.c5_gen_batch(n, sd.ctypes.data_as(C.POINTER(C.c_uint64)), base_len, n_agents, rounds, ops, hot, del_frac,
                        threads, ptr, ln.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise ValueError("c5_gen_batch: bad parameters")
    out = []
    for i in range(n):
        out.append(C.string_at(ptr[i], int(ln[i])))
        L.c5_free(ptr[i])
    return out
