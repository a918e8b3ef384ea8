"""Hand-built general-form record streams (RTXN + RINS / RDEL per op + RPARENT per parent) placed
against k_replay's 64-record window, and multi-op txns that fail at their second or third op --
TEST INFRASTRUCTURE shared by tests/test_multi_op_ref.py (oracle, CPU emulation, branch reach) and
tests/test_gpu_window_general.py / tests/test_gpu_multi_op.py (the engine).

Every stream is a pair (prep, stream) of parsed txn lists.  `prep` builds the document: author
"base" inserts BASE chars, author "w" grows the tables (_prep), author "a" inserts 200 chars of its
own after base item 50 (one general-form txn: it names base's items), and what a family needs
before its first placed record.
`stream` is what is placed: `pad` compact records first -- a's one-item deletes of its own items at
seqs 0, 2, 4, ...: one record each, none continues a run -- so the record after them sits `pad`
records into the stream.  Staged as a second batch (test_gpu_window_general.py) record k of
`stream` is lane k of the first window; replayed as one wire after `prep` (the CPU emulation) it
sits PREP_RECORDS further on.

An op is (kind, a_name, a_seq, b_name, b_seq, len) as in fuzz_gen.parse_wire: kind 0 an insert
with origin_left a and origin_right b, kind 1 a delete of `len` items from a on."""
import functools

from fuzz_gen import build_wire

BASE = 600
OWN = 200  # a's first insert: seqs 0 .. OWN - 1 are items of its own
R = ("ROOT", 0xFFFFFFFF)


def ins(ol, orr, n=1):
    return (0, ol[0], ol[1], orr[0], orr[1], n)


def dele(target, n=1):
    return (1, target[0], target[1], None, 0, n)


def b(k):  # base item k
    return ("base", k)


class Author:
    """txns of one author, each with the author's previous txn as its first parent"""

    def __init__(self, name, seq=0, out=None):
        self.name, self.seq, self.out = name, seq, [] if out is None else out

    def txn(self, ops, parents=None, more_parents=()):
        ps = parents if parents is not None else [(self.name, self.seq - 1)] + list(more_parents)
        self.out.append((self.name, self.seq, ps, list(ops)))
        self.seq += sum(op[5] for op in ops)
        return self

    def last(self):  # the last id this author made
        return (self.name, self.seq - 1)

    def pads(self, n, first=0):
        for j in range(first, first + n):
            self.txn([dele((self.name, 2 * j))])
        return self


WARM = 256  # ops of the warm-up txn
PREP_RECORDS = 3 + 3 + (1 + WARM + 1) + 3  # base's txn, w's insert, w's deletes, a's insert


def _prep():
    """base's text, the warm-up, a's own text.  The warm-up: before a txn of n ops the replay
    reserves 2n free leaves (replay_core.h fits) and otherwise stops for capacity AT the txn's
    header -- it would resume with a window loaded at that record, the header in lane 0, whatever
    the pad.  So author "w" first inserts WARM chars at the start of the text and deletes them in
    one txn of WARM one-item ops: the leaf table grows there, in prep, to more than a stream needs
    (doubling keeps > 2 * WARM - 64 leaves free), and no stream stops: test_multi_op_ref.py
    test_no_stream_stops_for_capacity."""
    out = [("base", 0, [R], [ins(R, R, BASE)])]
    w = Author("w", 0, out)
    w.txn([ins(R, b(0), WARM)], parents=[b(BASE - 1)])
    w.txn([dele(("w", k)) for k in range(WARM)])
    a = Author("a", 0, out)
    a.txn([ins(b(50), b(51), OWN)], parents=[w.last()])
    return out, a


def records(txns):
    """records the host encodes for a parsed txn list: 1 for a compact txn (one op on the author's
    own items, the author's previous txn the only parent), else 1 + ops + parents"""
    n = 0
    for a, s, ps, ops in txns:
        own = all(nm in (a, "ROOT") for op in ops for nm in ((op[1], op[3]) if op[0] == 0 else (op[1],)))
        compact = len(ops) == 1 and ps == [(a, s - 1)] and s >= 1 and own
        n += 1 if compact else 1 + len(ops) + len(ps)
    return n


# ---------------------------------------------------------------- (a) stride-3 runs at every phase
RUN_PADS = range(64)
RUN_LENS = (1, 2, 20, 21, 22, 43, 64)
RUN_KINDS = ("typing", "forward", "back")


def run_stream(pad, n, kind):
    """a run of n general-form one-op txns (3 records each: every op names a base item) behind
    `pad` compact records, three compact deletes after it.  typing: inside base text, the first
    char between base items 300 and 301, each further one after a's previous item with
    origin_right base 301; forward: deletes of base items 400, 401, ...; back: of 500, 499, ..."""
    prep, a = _prep()
    s = Author("a", a.seq)
    s.pads(pad)
    for i in range(n):
        if kind == "typing":
            s.txn([ins(b(300) if i == 0 else s.last(), b(301))])
        elif kind == "forward":
            s.txn([dele(b(400 + i))])
        else:
            s.txn([dele(b(500 - i))])
    s.pads(3, pad)
    return prep, s.out


# ---------------------------------------------------------------- (b) many-op groups at the thresholds
GROUP_PADS = (0, 1, 57, 58, 59, 60, 61, 62, 63)
GROUP_NOPS = (2, 3, 58, 59, 60, 61, 62, 63, 64, 120, 121, 122, 123, 124, 125, 140)
GROUP_PARENTS = (1, 3)
TAIL_TYPED, TAIL_DELETES = 70, 10


def group_stream(pad, nops, parents, mixed):
    """one txn of `nops` ops and `parents` parents behind `pad` compact records: 1 + nops +
    parents records that end short of, at and past where rec() moves the window (61 / 62 / 64 / 65
    / 124 / 125 records on) and past 128.  prep: with 3 parents, agents x and y each insert one
    char concurrently (parent: the base's last item), so the group's parents are a's previous txn
    and both heads; then a inserts one char between base items 300 and 301.  Plain ops are
    one-char inserts between base items 21 + 4k and 22 + 4k; a mixed group cycles through such an
    insert, an insert whose origin_left is the txn's own previous item (origin_right base 599) and
    a one-item delete of base item 21 + 4k.  Behind the group a types TAIL_TYPED chars (the first
    between base 500 and 501, the others after its previous item with origin_right base 599) and
    deletes base items 580, 579, ...: general-form txns that read the window after the jump."""
    prep, a = _prep()
    heads = []
    if parents == 3:
        for nm, at in (("x", 10), ("y", 12)):
            Author(nm, 0, prep).txn([ins(b(at), b(at + 1))], parents=[b(BASE - 1)])
            heads.append((nm, 0))
    a.txn([ins(b(300), b(301))])
    s = Author("a", a.seq)
    s.pads(pad)
    ops, seq = [], s.seq
    for k in range(nops):
        which = k % 3 if mixed else 0
        if which == 0:
            ops.append(ins(b(21 + 4 * k), b(22 + 4 * k)))
        elif which == 1:
            ops.append(ins(("a", seq - 1), b(BASE - 1)))
        else:
            ops.append(dele(b(21 + 4 * k)))
        seq += 1
    s.txn(ops, more_parents=heads)
    for i in range(TAIL_TYPED):
        s.txn([ins(b(500), b(501)) if i == 0 else ins(s.last(), b(BASE - 1))])
    for i in range(TAIL_DELETES):
        s.txn([dele(b(580 - i))])
    return prep, s.out


@functools.lru_cache(maxsize=None)
def run_family():
    """name -> (prep wire, stream wire, one wire of both): 1,344 streams"""
    out = {}
    for kind in RUN_KINDS:
        for n in RUN_LENS:
            for pad in RUN_PADS:
                p, s = run_stream(pad, n, kind)
                out[f"{kind}_n{n}_pad{pad}"] = (build_wire(p), build_wire(s), build_wire(p + s))
    return out


@functools.lru_cache(maxsize=None)
def group_family():
    """name -> (prep wire, stream wire, one wire of both): 576 streams"""
    out = {}
    for mixed in (False, True):
        for np_ in GROUP_PARENTS:
            for nops in GROUP_NOPS:
                for pad in GROUP_PADS:
                    p, s = group_stream(pad, nops, np_, mixed)
                    out[f"{'mixed' if mixed else 'plain'}_p{np_}_ops{nops}_pad{pad}"] = (build_wire(p), build_wire(s), build_wire(p + s))
    return out


# ---------------------------------------------------------------- txns that fail at their 2nd / 3rd op
def _error_txns(bad_ops):
    out = [("base", 0, [R], [ins(R, R, 30)])]
    a = Author("a", 0, out)
    a.txn([ins(b(10), b(11), 2), dele(b(20))], parents=[b(29)])  # a good two-op txn: seqs 0 .. 2
    a.txn(bad_ops(a.seq))
    a.txn([ins(b(5), b(6))])  # never applied: the document stopped
    return out


ERROR_CASES = {
    # an origin that names a delete order of its own txn: the id is known, no item carries it
    "origin_is_own_delete": lambda s: [dele(b(3)), ins(("a", s), b(8)), ins(b(1), b(2))],
    # a delete target one past its own txn's last seq
    "target_past_own_txn": lambda s: [ins(b(3), b(4)), ins(("a", s), b(4)), dele(("a", s + 3))],
    # a name of the wire's name table that no txn has interned
    "name_never_interned": lambda s: [ins(b(3), b(4)), ins(("ghost", 0), b(4)), ins(b(1), b(2))],
    # an op of length 0
    "zero_length_op": lambda s: [ins(b(3), b(4)), dele(b(7), 0), ins(b(1), b(2))],
}


def error_wire(name):
    return build_wire(_error_txns(ERROR_CASES[name]))


def good_wire():
    """the same history with a well-formed three-op txn in the failing one's place"""
    return build_wire(_error_txns(lambda s: [ins(b(3), b(4)), ins(("a", s), b(4)), dele(("a", s))]))
