"""Hand-built LOCAL record streams placed against k_replay's 64-record window -- TEST INFRASTRUCTURE
shared by tests/test_window_local_ref.py (oracle, CPU emulation, branch reach) and
tests/test_gpu_window_local.py (the engine).  Pure Python: no crdt_amd import.

Local records (REC_LC, one per LocalOp part, host_plan.h encode_local_txn) take code of their own
in the replay: the `compact && !remote` branches of the typing and delete scans, the front-run scan
and leaf_insert_front, leaf_delete_span / local_delete_pieces, the SHAPE_LOCAL instance of k_replay.
A script here is a list of local txns on a text whose first txn is one insert of BASE chars:

    ops = [(author, [(pos, del, ins), ...]), ...]        author 0 or 1 (AUTHORS)

scripts() maps name -> (ops, expected status).  Staged as a second batch behind the base insert,
record k of a script sits in lane k of the first window; staged with the base insert, in lane
k + 1.  records(ops) counts records as the host encodes them, so a test can say which lane a run
starts in.  The only scripts that end with an error status are those of error_scripts() (the *_past_* runs
and the all-empty-op txn); tests/test_window_local_ref.py asserts the oracle agrees."""
import functools

BASE = 600  # chars of the base text (one insert: one entry)
AUTHORS = ("jeremy", "second")
ERR_POS_OOB, ERR_EMPTY_TXN = -1, -7


def base_ops():
    return [(0, [(0, 0, BASE)])]


def records(ops):
    """records host_plan.h encode_local_txn makes of the txns: a one-op txn that deletes or inserts
    is one REC_LC; a replace op and a multi-op txn are one REC_LC per non-empty part (a replace's
    delete, then its insert); a txn whose ops are all empty keeps the general form, LTXN + one LOP
    per op (a one-op empty txn is one REC_LC)"""
    n = 0
    for _a, tx in ops:
        span = sum(d + i for _p, d, i in tx)
        if span != 0 and (len(tx) > 1 or (tx[0][1] != 0 and tx[0][2] != 0)):
            n += sum((d != 0) + (i != 0) for _p, d, i in tx)
        elif len(tx) == 1:
            n += 1
        else:
            n += 1 + len(tx)
    return n


class Doc:
    """a local edit script: one-op txns by author 0 on a text whose length is tracked, unless a
    call says otherwise"""

    def __init__(self, n=BASE):
        self.n = n
        self.ops = []

    def op(self, pos, dl, ins, author=0):  # one one-op txn; its effect on the length is the caller's claim
        self.ops.append((author, [(pos, dl, ins)]))
        self.n += ins - dl
        return self

    def txn(self, tx, author=0):  # one txn of several ops
        self.ops.append((author, list(tx)))
        self.n += sum(i - d for _p, d, i in tx)
        return self

    def typing(self, pos, k, w=1):
        """k chunks typed from pos on, each at the previous pos plus the previous length; w: the
        chunk width, or a tuple of widths to cycle through"""
        ws = (w,) if isinstance(w, int) else tuple(w)
        for i in range(k):
            self.op(pos, 0, ws[i % len(ws)])
            pos += ws[i % len(ws)]
        return self

    def front(self, k, w=1):  # k inserts of w chars at position 0
        for _ in range(k):
            self.op(0, 0, w)
        return self

    def forward(self, pos, k):  # k forward deletes at pos
        assert pos + k <= self.n
        for _ in range(k):
            self.op(pos, 1, 0)
        return self

    def back(self, pos, k):  # k backspaces, the first deleting the char at pos
        assert k - 1 <= pos < self.n
        for i in range(k):
            self.op(pos - i, 1, 0)
        return self

    def jumps(self, k):  # k single inserts, no two neighbours: records that continue nothing
        for i in range(k):
            self.op(7 + (i % 2) * (self.n // 2) + 3 * (i // 2), 0, 1)
        return self

    def far(self, k):
        """k single inserts near the end of the text, each one position before the last: records
        that continue nothing and leave the first 400 chars' entries alone (family C's pads)"""
        for i in range(k):
            self.op(self.n - 10 - 2 * i, 0, 1)
        return self

    def to_lane(self, lane):  # far pads until the next record is record `lane` of the script
        assert records(self.ops) <= lane
        return self.far(lane - records(self.ops))

    def run(self, kind, k):
        if kind == "typing":
            return self.typing(self.n, k)  # at the end of the text: appends to the last entry
        if kind == "typing_mid":
            return self.typing(self.n // 3, k)  # inside an entry: an insert, then the typing that appends to it
        if kind == "typing_w3":
            return self.typing(self.n, k, 3)
        if kind == "typing_mixed":
            return self.typing(self.n // 3, k, (1, 2, 5))  # the run's total is a sum of unequal lengths
        if kind == "forward":
            return self.forward(self.n // 2 - k // 2, k)
        if kind == "back":
            return self.back(self.n // 2 + k // 2, k)
        if kind == "front":
            return self.front(k, 1)
        assert kind == "front_w2", kind
        return self.front(k, 2)


KINDS = ("typing", "typing_mid", "typing_w3", "typing_mixed", "forward", "back", "front", "front_w2")
A_LENS = (1, 63, 64, 65, 129)
B_LENS = (1, 2, 63, 64, 65, 130)
B_PADS = (0, 1, 30, 61, 62, 63, 64)
C_LANES = (61, 62, 63)
D_PADS = (30, 60)
D_HEAD, D_TAIL = 4, 20  # a near miss sits behind D_HEAD records of its run: record 34, or 64 -- the first past the window
E_LENS = (3, 70)
P = 200  # where family D's runs begin (inside the base entry, clear of the pads' places)


def family_a():
    return {f"stream{n}_{kind}": Doc().run(kind, n) for n in A_LENS for kind in KINDS}


def family_b():
    return {f"run{n}_pad{pad}_{kind}": Doc().jumps(pad).run(kind, n).jumps(3)
            for n in B_LENS for pad in B_PADS for kind in KINDS}


def _entries(d):
    """family C's ground: single chars typed at 20, 40 and 60 cut the base entry, so the text
    begins  B[0:20] x1 B[20:39] x2 B[39:58] x3 B[58:...]  -- 7 entries, x1 at position 20, x2 at 40,
    x3 at 60"""
    return d.op(20, 0, 1).op(40, 0, 1).op(60, 0, 1)


def family_c():
    """delete spans (one delete of l > 1 items that leaves its first entry), each as record 61, 62
    and 63 of its script"""
    out = {}
    for lane in C_LANES:
        def put(name, d):
            out[f"span_{name}_lane{lane}"] = d.jumps(3)

        # mid-entry to mid-entry over four entries: B[10:20] x1 B[20:39] x2 and four items of B[39:58]
        put("several_entries", _entries(Doc()).to_lane(lane).op(10, 35, 0))
        # ... ending exactly at an entry's end (x1's)
        put("to_entry_end", _entries(Doc()).to_lane(lane).op(10, 11, 0))
        # from offset 0 of an entry (x1) into the middle of the next, and from the text's first item
        put("from_offset0", _entries(Doc()).to_lane(lane).op(20, 10, 0))
        put("from_text_start", _entries(Doc()).to_lane(lane).op(0, 25, 0))
        # from offset 0 to an entry's end: whole entries only (x1 B[20:39] x2)
        put("whole_entries", _entries(Doc()).to_lane(lane).op(20, 21, 0))
        # directly before a deleted run that its deleted rest appends onto: B[30:35] is deleted
        # first, then [25, 35) of what is left -- B[25:30], whose deleted form continues into
        # B[30:35], and on over that deleted entry (skipped) into B[35:40]
        put("before_deleted_run", Doc().op(30, 5, 0).to_lane(lane).op(25, 10, 0))
        # directly before a visible entry: the delete ends inside B[20:39], whose visible rest
        # B[30:39] lies before the visible x2 and cannot join it (another run): it is inserted.  (No local history puts a visible rest before an entry it CAN prepend
        # onto: two visible entries with consecutive orders and the same origin_right are typed
        # back to back and merge when the second is inserted; test_window_local_ref.py counts it.)
        put("before_visible_entry", _entries(Doc()).to_lane(lane).op(15, 16, 0))
        # over deleted entries that it skips: x1 and B[25:30] are deleted one by one, then one
        # delete from B[15] over both deleted places
        put("skips_deleted", _entries(Doc()).op(20, 1, 0).op(25, 5, 0).to_lane(lane).op(15, 30, 0))
        # beyond the cached leaf's end: far more entries than a leaf holds lie in the span (at leaf
        # 32 the 40 chars typed apart make 80 entries)
        d = Doc()
        for i in range(40):
            d.op(10 + 5 * i + i, 0, 1)
        put("beyond_the_leaf", d.to_lane(lane).op(5, 230, 0))
        # the whole document
        d = _entries(Doc()).to_lane(lane)
        put("whole_document", d.op(0, d.n, 0).typing(0, 40))
        # a typing run over the freshly deleted place afterwards
        put("typing_after", _entries(Doc()).to_lane(lane).op(10, 35, 0).typing(10, 12).back(21, 5))
    return out


def family_d():
    """near misses: one record that violates exactly one term of a scan's predicate in the middle
    of an otherwise perfect run, as record pad + D_HEAD"""
    out = {}
    for pad in D_PADS:
        def put(name, d):
            out[f"{name}_pad{pad}"] = d.jumps(3)

        def start():
            return Doc().jumps(pad)

        # --- typing (typing_scan_r: author, Z == 0, Q - 1 < 0xFFFF, Y == p1 + p3)
        put("second_author_in_typing", start().typing(P, D_HEAD).op(P + D_HEAD, 0, 1, author=1).typing(P + D_HEAD + 1, D_TAIL))
        put("replace_continues_typing", start().typing(P, D_HEAD).op(P + D_HEAD, 2, 3).typing(P + D_HEAD + 3, D_TAIL))
        put("big_chunk_in_typing", start().typing(P, D_HEAD).op(P + D_HEAD, 0, 65536).typing(P + D_HEAD + 65536, D_TAIL))
        put("pos_plus_1_in_typing", start().typing(P, D_HEAD).typing(P + D_HEAD + 1, 1 + D_TAIL))
        # --- forward deletes and backspaces (delete_scan_r: author, Z == 1, Q == 0, Y == p1 + delta)
        S = P + 40  # where the backspace runs begin: they stay inside [P, S]
        put("del2_in_forward", start().forward(P, D_HEAD).op(P, 2, 0).forward(P, D_TAIL))
        put("insert_in_forward", start().forward(P, D_HEAD).op(P, 0, 1).forward(P, D_TAIL))
        put("second_author_in_forward", start().forward(P, D_HEAD).op(P, 1, 0, author=1).forward(P, D_TAIL))
        put("del2_in_back", start().back(S, D_HEAD).op(S - D_HEAD, 2, 0).back(S - D_HEAD - 1, D_TAIL))
        put("insert_in_back", start().back(S, D_HEAD).op(S - D_HEAD, 0, 1).back(S - D_HEAD, D_TAIL))
        put("second_author_in_back", start().back(S, D_HEAD).op(S - D_HEAD, 1, 0, author=1).back(S - D_HEAD - 1, D_TAIL))
        put("forward_then_back", start().forward(P, D_HEAD).back(P - 1, D_TAIL))  # delta changes sign mid-run
        put("back_then_forward", start().back(S, D_HEAD).forward(S - D_HEAD + 1, D_TAIL))
        # --- prepends (front_scan: author, pos 0, del 0, the same length)
        put("other_length_in_front", start().front(D_HEAD).front(1, 2).front(D_TAIL))
        put("second_author_in_front", start().front(D_HEAD).op(0, 0, 1, author=1).front(D_TAIL))
        put("delete_in_front", start().front(D_HEAD).op(0, 1, 0).front(D_TAIL))
        # --- a multi-op txn (one compact record per part) and a txn of empty ops (general LTXN
        # form, ERR_EMPTY_TXN: the document stops there) between two runs
        put("multi_op_between_runs", start().typing(P, 10).txn([(5, 0, 2), (50, 1, 0), (80, 2, 3)]).forward(P, 10))
        put("empty_txn_between_runs", start().typing(P, 10).txn([(5, 0, 0), (9, 0, 0)]).forward(P, 10))
    return out


def family_e():
    """delete runs that meet the text's ends, and one record more"""
    out = {}
    for k in E_LENS:
        out[f"forward_to_end_{k}"] = Doc().forward(BASE - k, k)
        d = Doc().forward(BASE - k, k)
        out[f"forward_past_end_{k}"] = d.op(BASE - k, 1, 0)  # pos == the text's length
        out[f"back_to_start_{k}"] = Doc().back(k - 1, k)
        d = Doc().back(k - 1, k)
        # pos 0xFFFFFFFF = 0 - 1 satisfies the scan's Y == p1 + delta: only the room of the entry
        # (no item before the first) keeps it out of the run
        out[f"back_past_start_{k}"] = d.op(0xFFFFFFFF, 1, 0)
    return out


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e}


def expected_status(name):
    if "_past_" in name:
        return ERR_POS_OOB
    if name.startswith("empty_txn_"):
        return ERR_EMPTY_TXN
    return 0


@functools.lru_cache(maxsize=None)
def family(f):
    """name -> (ops, expected status) of one family, built once"""
    return {name: (d.ops, expected_status(name)) for name, d in FAMILIES[f]().items()}


@functools.lru_cache(maxsize=None)
def scripts():
    """name -> (ops, expected status), every family"""
    out = {}
    for f in FAMILIES:
        for name, v in family(f).items():
            assert name not in out, name
            out[name] = v
    return out


def family_of(name):
    return next(f for f in FAMILIES if name in family(f))


def error_scripts():
    return sorted(n for n, (_ops, st) in scripts().items() if st != 0)


# ---------------------------------------------------------------- the oracle's replay, once per layout
LAYOUTS = {32: (32, 16), 4: (4, 8)}


def flat(ops):
    """(agents [T], counts [T], patches [sum counts, 3]) of a txn list, as uint32 arrays"""
    import numpy as np
    agents = np.array([a for a, _tx in ops], np.uint32)
    counts = np.array([len(tx) for _a, tx in ops], np.uint32)
    patches = np.array([op for _a, tx in ops for op in tx], np.uint32).reshape(-1, 3)
    return agents, counts, patches


def oracle_doc(leaf, ops):
    """a fresh oracle document with AUTHORS interned (ids 0 and 1) after `ops`, one apply_local per
    txn up to the first that fails; returns (document, status)"""
    from oracle_lib import OracleDoc
    o = OracleDoc(*LAYOUTS[leaf])
    ids = [o.agent(nm) for nm in AUTHORS]
    assert ids == [0, 1]
    for a, tx in ops:
        st = o.apply_local(a, tx)
        if st != 0:
            return o, st
    return o, 0


@functools.lru_cache(maxsize=None)
def oracles(leaf):
    """name -> (oracle document after the base insert and the script, status); computed once per
    layout, the tests leave the documents unchanged"""
    return {name: oracle_doc(leaf, base_ops() + ops) for name, (ops, _st) in scripts().items()}


@functools.lru_cache(maxsize=None)
def oracle_exports(leaf):
    return {name: o.export() for name, (o, st) in oracles(leaf).items() if st == 0}
