"""Hostile compact-record streams: hand-built remote batches that no editing session produces --
TEST INFRASTRUCTURE shared by tests/test_hostile_streams_ref.py (oracle, CPU emulation) and
tests/test_gpu_hostile_streams.py (the engine).

k_replay's fast paths accept whole runs of compact remote (RC) records lane-parallel: the typing
mask of the record window (wave_gpu.h decode_window), the typing scans (typing_scan_m /
typing_scan_at) and the hinted delete runs with their carried cursor (replay_core.h fast_deletes).
The other tests feed them streams derived from valid local scripts.  Here a record is wrong in the
middle of a run -- a seq gap, an unknown target, a delete of a delete op's seq, a run that walks
into seqs that name no item -- or valid in a shape a local script never has (the author deleting
an item twice, a run across entries and tombstones, an origin_right that changes mid-run).

Every case is (base txns, stream txns).  The base batch builds the document: author "w" inserts
WARM chars and deletes them in one txn of WARM one-item ops (the leaf table grows there, as in
general_streams._prep, so that the stream batch replays in one launch without a capacity stop),
then author "a" inserts BASE chars behind them, with w's last txn as its parent: one frontier head,
so a's compact records are candidates for the fast paths.  The stream batch is txns of the compact
shape (one op on the author's own items or ROOT, the author's previous txn the only parent), so
staged as a second batch record k of the stream is lane k of the first window.  It begins with
`pad` records that continue nothing -- a's one-char inserts between base items 7 + 3i and
8 + 3i -- which move the interesting record to a chosen lane.  Pads are inserts, not deletes, so
that every seq below the stream's running seq names an item unless the family itself made a delete
op: no status depends on the pad.  Families use base items from 200 on (pads end at 197) and take
every seq they name from the stream's running seq.

An op is (kind, a_name, a_seq, b_name, b_seq, len) as in fuzz_gen.parse_wire."""
import functools
import struct

from fuzz_gen import build_wire

BASE = 600
WARM = 248  # (the base batch is then 3 + (1 + WARM + 1) + 3 = 256 records: four whole windows)
M32 = 0xFFFFFFFF
R = ("ROOT", M32)
LANES = (0, 1, 30, 61, 62, 63, 64)  # where the interesting record lands; 64: the second window
RUN = 130                           # records of the long runs
RUN_BAD_AT = (1, 62, 63, 64, 100)   # index of the one bad record in a long run


def base_txns(with_b=False):
    """-> (txns, a's next seq).  with_b: author "b" has one char of its own (between base items
    500 and 501), and a one more (at the end) with b's txn as its parent: one head again"""
    out = [("w", 0, [R], [(0, "ROOT", M32, "ROOT", M32, WARM)]),
           ("w", WARM, [("w", WARM - 1)], [(1, "w", k, None, 0, 1) for k in range(WARM)]),
           ("a", 0, [("w", 2 * WARM - 1)], [(0, "w", WARM - 1, "ROOT", M32, BASE)])]
    if not with_b:
        return out, BASE
    out.append(("b", 0, [("a", BASE - 1)], [(0, "a", 500, "a", 501, 1)]))
    out.append(("a", BASE, [("b", 0)], [(0, "a", BASE - 1, "ROOT", M32, 1)]))
    return out, BASE + 1


class Stream:
    """txns of the compact shape, word by word: seq, parent and every id can be given wrong"""

    def __init__(self, seq_a=BASE):
        self.txns = []
        self.seq = {"a": seq_a, "b": 1}

    def rec(self, op, ag="a", seq=None, parent=None):
        s = self.seq[ag] if seq is None else seq
        self.txns.append((ag, s, [parent if parent is not None else (ag, (s - 1) & M32)], [op]))
        self.seq[ag] = (s + op[5]) & M32
        return s

    def ins(self, ol, orr, n=1, ag="a", **kw):
        """an insert between ag's items ol and orr (None: ROOT); returns its seq"""
        def oid(x):
            return R if x is None else (ag, x)
        return self.rec((0,) + oid(ol) + oid(orr) + (n,), ag, **kw)

    def dele(self, t, n=1, ag="a", **kw):
        return self.rec((1, ag, t, None, 0, n), ag, **kw)

    def pads(self, n):
        for i in range(n):
            self.ins(7 + 3 * i, 8 + 3 * i)
        return self

    def typing(self, k, after, right, n=1, ag="a"):
        """k records: the first after item `after`, each further one after the author's previous
        item; origin_right `right` throughout"""
        for i in range(k):
            self.ins(after if i == 0 else self.seq[ag] - 1, right, n, ag)
        return self

    def back(self, t, k, ag="a"):
        for i in range(k):
            self.dele(t - i, ag=ag)
        return self

    def fwd(self, t, k, ag="a"):
        for i in range(k):
            self.dele(t + i, ag=ag)
        return self


def records(txns):
    """records the host encodes for the txns (host_plan.h encode_remote): 1 for the compact form --
    one op of 1 .. 0x7FF items on the author's own items (a seq other than 0xFFFFFFFF) or ROOT, the
    author's previous txn the only parent -- else 1 + ops + parents"""
    n = 0
    for a, s, ps, ops in txns:
        compact = len(ops) == 1 and ps == [(a, s - 1)] and s >= 1 and 1 <= ops[0][5] <= 0x7FF
        if compact:
            k, an, asq, bn, bsq, _ln = ops[0]
            ids = ((an, asq), (bn, bsq)) if k == 0 else ((an, asq),)
            compact = all(i == R or (i[0] == a and i[1] != M32) for i in ids)
        n += 1 if compact else 1 + len(ops) + len(ps)
    return n


def _typing_tail(h):  # two records that continue the typing at base item 300
    h.ins(h.seq["a"] - 1, 301)
    h.ins(h.seq["a"] - 1, 301)


# ---------------------------------------------------------------- error families
# name -> (the oracle's status, build(h)): build appends the family's records, the bad one last,
# and may return a function that appends what follows the bad record in the second variant (the
# rest of a long run); the default is _typing_tail.
def _seq_gap(h):  # a typing run whose fourth record skips a seq; every other term continues the run
    h.typing(3, 300, 301)
    s = h.seq["a"]
    h.ins(s, 301, seq=s + 1)


def _seq_repeat(h):  # ... whose fourth record has the third's seq, after the third's item
    h.typing(3, 300, 301)
    s = h.seq["a"]
    h.ins(s - 1, 301, seq=s - 1)


def _duplicate_txn(h):  # the third record once more, word for word
    h.typing(3, 300, 301)
    h.txns.append(h.txns[-1])


def _ol_own_seq(h):
    h.typing(2, 300, 301)
    h.ins(h.seq["a"], 301)


def _ol_future_seq(h):
    h.typing(2, 300, 301)
    h.ins(h.seq["a"] + 5, 301)


def _ol_delete_op(h):  # origin_left = own seq - 1 as in a typing run, but that seq is a delete op's
    h.typing(2, 300, 301)
    d = h.dele(250)
    h.ins(d, 301)


def _ol_equals_or(h):
    h.typing(2, 300, 301)
    h.ins(350, 350)


def _or_before_ol(h):
    h.typing(2, 300, 301)
    h.ins(350, 340)


def _del_own_seq(h):
    h.back(400, 2)
    h.dele(h.seq["a"])


def _del_future_seq(h):
    h.back(400, 2)
    h.dele(h.seq["a"] + 7)


def _del_delete_op(h):  # the target continues the backspace run's seqs... into the run's own delete ops
    d = h.dele(400)
    h.dele(399)
    h.dele(d)


def _back_below_zero(h):  # targets 2, 1, 0, then -1 (that last record has the general form)
    h.back(2, 3)
    h.dele(M32)


def _fwd_past_typed(h):  # a forward run over the last typed items and on: the next seq is the run's first delete op
    t = h.seq["a"]
    h.typing(5, 300, 301)
    h.fwd(t + 3, 3)


def _zero_len_ins(h):
    h.typing(2, 300, 301)
    h.ins(h.seq["a"] - 1, 301, n=0)


def _zero_len_del(h):
    h.back(400, 2)
    h.dele(398, n=0)


def _back_run_bad_at(i):
    def build(h):  # RUN backspaces from base item 450 down; record i names a seq far ahead
        h.back(450, i)
        h.dele(h.seq["a"] + 1000)
        return lambda h: h.back(450 - i - 1, RUN - i - 1)
    return build


def _typing_run_bad_at(i):
    def build(h):  # RUN typed chars behind base item 300; record i skips a seq
        h.typing(i, 300, 301)
        s = h.seq["a"]
        h.ins(s, 301, seq=s + 1)
        return lambda h: h.typing(RUN - i - 1, h.seq["a"] - 1, 301)
    return build


ERRORS = {
    "seq_gap": (-2, _seq_gap), "seq_repeat": (-2, _seq_repeat), "duplicate_txn": (-2, _duplicate_txn),
    "ol_own_seq": (-4, _ol_own_seq), "ol_future_seq": (-4, _ol_future_seq), "ol_delete_op": (-4, _ol_delete_op),
    "ol_equals_or": (-5, _ol_equals_or), "or_before_ol": (-5, _or_before_ol),
    "del_own_seq": (-4, _del_own_seq), "del_future_seq": (-4, _del_future_seq), "del_delete_op": (-4, _del_delete_op),
    "back_below_zero": (-4, _back_below_zero), "fwd_past_typed": (-4, _fwd_past_typed),
    "zero_len_ins": (-9, _zero_len_ins), "zero_len_del": (-9, _zero_len_del),
}
LONG_ERRORS = {}
for _i in RUN_BAD_AT:
    LONG_ERRORS[f"back{RUN}_bad{_i}"] = (-4, _back_run_bad_at(_i))
    LONG_ERRORS[f"typing{RUN}_gap{_i}"] = (-2, _typing_run_bad_at(_i))
GENERAL_FORM = {"back_below_zero", "zero_len_ins", "zero_len_del", "len_7ff_800", "parent_not_previous"}  # hold a record of the general form


# ---------------------------------------------------------------- valid, non-local families
def _double_forward(h):  # a forward run, then one that overlaps it: the author deletes items twice
    h.fwd(300, 10).fwd(305, 10)


def _across_deleted(h):  # runs across an item that is already deleted
    h.dele(320)
    h.back(325, 10)
    h.dele(340)
    h.fwd(335, 10)


def _across_entries(h):  # runs across an entry boundary made by an insert
    h.ins(350, 351)
    h.back(355, 10)
    h.ins(250, 251)
    h.fwd(245, 10)


def _typed_and_older(h):  # runs from older items (base or pads) on into typed ones, and back down
    t = h.seq["a"]
    h.typing(5, 300, 301)
    h.fwd(t - 2, 4)
    h.back(t + 4, 8)


def _same_target_4(h):
    for _ in range(4):
        h.dele(300)


def _len_2_3(h):
    h.ins(400, 401, 2)
    for n in (3, 2, 3, 1, 2):
        h.ins(h.seq["a"] - 1, 401, n)
    h.dele(h.seq["a"] - 4, 2)
    h.dele(h.seq["a"] - 9, 3)


def _len_7ff_800(h):  # 0x7FF is the longest compact op; 0x800 has the general form
    t = h.ins(400, 401, 0x7FF)
    h.ins(h.seq["a"] - 1, 401)
    u = h.ins(h.seq["a"] - 1, 401, 0x800)
    h.ins(h.seq["a"] - 1, 401)
    h.dele(t, 0x7FF)
    h.dele(u, 0x800)
    h.ins(h.seq["a"] - 0x800 - 0x7FF - 1, 401)


def _or_changes(h):  # a typing run whose origin_right changes in its middle
    h.typing(3, 400, 401)
    h.ins(h.seq["a"] - 1, 402)
    h.ins(h.seq["a"] - 1, 402)
    h.ins(h.seq["a"] - 1, 405)


def _ol_previous_but_one(h):
    h.typing(3, 400, 401)
    h.ins(h.seq["a"] - 2, 401)
    h.ins(h.seq["a"] - 2, 401)
    h.ins(h.seq["a"] - 1, 401)


def _parent_not_previous(h):  # one parent, but not seq - 1 (general form; two heads from there on)
    h.typing(3, 400, 401)
    s = h.seq["a"]
    h.ins(s - 1, 401, parent=("a", s - 3))
    h.typing(3, h.seq["a"] - 1, 401)
    h.back(450, 3)


def _root_root(h):
    for _ in range(3):
        h.ins(None, None)
    h.ins(h.seq["a"] - 1, None)
    h.ins(h.seq["a"] - 1, None)


def _end_70(h):  # typing at the end of the text (origin_right ROOT) for 70 records
    h.typing(70, BASE - 1, None)


def _author_b(h):  # b types and deletes its own items between a's runs
    h.typing(3, 300, 301)
    h.typing(3, 0, None, ag="b")
    h.back(450, 3)
    h.back(3, 2, ag="b")
    h.typing(3, h.seq["a"] - 4, 301)
    h.typing(2, 1, None, ag="b")
    h.fwd(200, 3)
    h.fwd(1, 1, ag="b")


VALID = {
    "double_forward": _double_forward, "across_deleted": _across_deleted, "across_entries": _across_entries,
    "typed_and_older": _typed_and_older, "same_target_4": _same_target_4, "len_2_3": _len_2_3,
    "len_7ff_800": _len_7ff_800, "or_changes": _or_changes, "ol_previous_but_one": _ol_previous_but_one,
    "parent_not_previous": _parent_not_previous, "root_root": _root_root, "end_70": _end_70, "author_b": _author_b,
}


# ---------------------------------------------------------------- the cases
class Case:
    def __init__(self, name, family, lane, base, stream, want, bad):
        self.name, self.family, self.lane, self.base, self.stream = name, family, lane, base, stream
        self.want = want  # the status the family expects of the oracle (0: a valid family)
        self.bad = bad    # index of the bad txn in `stream` (None: a valid family)

    @functools.cached_property
    def wires(self):
        """(base batch, stream batch, both as one wire)"""
        return build_wire(self.base), build_wire(self.stream), build_wire(self.base + self.stream)


def _error_case(fam, want, build, lane, late):
    # the family's own records before the bad one count as part of the pad: the bad record is txn
    # max(lane, its index in the family) of the stream; a long run starts at the pad instead
    base, seq_a = base_txns()
    if fam in LONG_ERRORS:
        pad = lane
    else:
        dry = Stream(seq_a)
        build(dry)
        pad = max(lane - (len(dry.txns) - 1), 0)
    h = Stream(seq_a).pads(pad)
    tail = build(h) or _typing_tail
    bad = len(h.txns) - 1
    if late:  # ... and a few records later one that fails with another status: the first must win
        tail(h)
        if want == -5:
            h.dele(h.seq["a"] + 7)   # (a seq far ahead: -4)
        else:
            h.ins(350, 350)          # (origin_left == origin_right: -5)
    return Case(f"{fam}_lane{lane}_{'late' if late else 'last'}", fam, lane, base, h.txns, want, bad)


@functools.lru_cache(maxsize=None)
def error_cases():
    """every error family at every lane, in two variants: `last` -- the bad record ends the stream
    (a replay that swallowed it ends with status 0) -- and `late`"""
    out = []
    for table in (ERRORS, LONG_ERRORS):
        for fam, (want, build) in table.items():
            for lane in LANES:
                for late in (False, True):
                    out.append(_error_case(fam, want, build, lane, late))
    return out


@functools.lru_cache(maxsize=None)
def valid_cases():
    out = []
    for fam, build in VALID.items():
        for lane in LANES:
            base, seq_a = base_txns(with_b=fam == "author_b")
            h = Stream(seq_a).pads(lane)
            build(h)
            out.append(Case(f"{fam}_pad{lane}", fam, lane, base, h.txns, 0, None))
    return out


def interleaved():
    """error and valid cases alternating (the valid ones cycled), so that the four waves of a block
    mix failing documents with good ones"""
    err, ok = error_cases(), valid_cases()
    out = []
    for i, c in enumerate(err):
        out += [c, ok[i % len(ok)]]
    return out


@functools.lru_cache(maxsize=None)
def oracle_results(leaf):
    """case name -> (status after both batches, OracleDoc), once per layout; left unchanged"""
    from oracle_lib import OracleDoc
    layouts = {32: (32, 16), 4: (4, 8)}
    out = {}
    for c in error_cases() + valid_cases():
        o = OracleDoc(*layouts[leaf])
        w0, w1, _ = c.wires
        assert o.apply_remote_wire(w0) == 0, c.name
        out[c.name] = (o.apply_remote_wire(w1), o)
    return out


# ---------------------------------------------------------------- the parent limit
def parent_limit_wires(k):
    """(wire with a txn of k parents -- all the same id -- in its middle, the wire without that
    txn and what follows it)"""
    head = [("a", 0, [R], [(0, "ROOT", M32, "ROOT", M32, 50)]), ("a", 50, [("a", 49)], [(0, "a", 49, "ROOT", M32, 1)])]
    many = ("a", 51, [("a", 50)] * k, [(0, "a", 50, "ROOT", M32, 1)])
    tail = [("a", 52, [("a", 51)], [(1, "a", 10, None, 0, 1)])]
    return build_wire(head + [many] + tail), build_wire(head)


# ---------------------------------------------------------------- CRDT_E_WIRE on the engine
def doc_wires(d):
    """first: "base" writes 10 chars.  rejected: a batch by a new author "zed".  later: a batch in
    which "amy" is new before "zed" is -- had the rejected call interned zed, amy and zed would
    swap agent ids (get_or_create order, doc.rs:66-80)"""
    first = build_wire([("base", 0, [R], [(0, "ROOT", M32, "ROOT", M32, 10 + d)])])
    rejected = build_wire([("zed", 0, [("base", 9 + d)], [(0, "base", 3, "base", 4, 2)])])
    later = build_wire([("amy", 0, [("base", 9 + d)], [(0, "base", 5, "base", 6, 3)]),
                        ("zed", 0, [("amy", 2)], [(0, "amy", 1, "amy", 2, 2), (1, "base", 0, None, 0, 2)])])
    return first, rejected, later


def malformed_wires():
    """wires that tests/test_wire_malformed.py shows to be refused cleanly: a batch that ends
    early, a txn count the buffer cannot hold, a wrong magic, a name index outside the table"""
    w = doc_wires(0)[1]
    words = list(struct.unpack(f"<{len(w) // 4}I", w))
    n_txns_at = 2 + (1 + 1) + (1 + 1)  # magic, n_names, "zed" and "base" with their length words
    assert words[n_txns_at] == 1

    def patched(i, v):
        x = list(words)
        x[i] = v
        return struct.pack(f"<{len(x)}I", *x)
    return {"cut": w[:-4], "n_txns_huge": patched(n_txns_at, 0x0FFFFFFF), "n_names_huge": patched(1, 0xFFFFFFFF),
            "magic": patched(0, 0x31585453), "name_index": patched(n_txns_at + 1, 2)}
