"""Delete-run hints of the remote encoder (host_plan.h hint_delete_runs; DESIGN §4 "Delete-run
hints"): every compact remote (RC) delete record carries in w3 the length m of the maximal run of
one-item deletes that starts at it and the run's direction, w3 = backspace << 31 | m, and the
replay's fast delete path trusts it instead of scanning.  A hint that over-counts would make the
replay skip records, so the encoder is checked here on its own, on the CPU:

* tests/hints/encode_dump.cpp (a stand-alone program around WireView::parse + encode_remote, built
  with -fsanitize=address,undefined) prints the records of a wire batch;
* every RC delete's (back, m) is recomputed from the printed w0..w2 by the definition, as a plain
  forward loop per record, and compared exactly;
* every other word of every record is compared with an encoder restated here from the record
  format (crdt_types.h): the hints change nothing else.

The same streams then go through the CPU emulation of the replay (which reads the hints as the
kernel does) and are compared with the oracle."""
import functools
import os
import subprocess

import numpy as np
import pytest

from crdt_amd.traces import TRACE_NAMES, load_remote_wire
from fuzz_gen import build_wire, parse_wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "text-crdt-rust_amd", "csrc")
M32 = 0xFFFFFFFF
ROOT_AGENT, UNKNOWN_AGENT = 0xFFFF, 0xFFFE
REC_RTXN, REC_RINS, REC_RDEL, REC_RPARENT, REC_RC = 3, 4, 5, 6, 8
RC_DEL = (REC_RC << 1) | 1  # w0 >> 27 of a compact remote delete
BACK = 1 << 31


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """records(wire, second=None) -> [(batch, w0, w1, w2, w3)] as encode_dump prints them"""
    td = tmp_path_factory.mktemp("hints")
    exe = str(td / "encode_dump")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "hints", "encode_dump.cpp")], check=True)
    n = [0]

    def records(wire, second=None):
        args = [exe]
        for w in (wire, second):
            if w is None:
                continue
            p = str(td / f"w{n[0]}.rtx")
            n[0] += 1
            with open(p, "wb") as f:
                f.write(w)
            args += (["--append"] if len(args) > 1 else []) + [p]
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])  # (a sanitizer report goes to stderr)
        return [tuple(int(x, 16) for x in ln.split()) for ln in r.stdout.splitlines()]
    return records


# ------------------------------------------------------------------ the format, restated
def ref_encode(txns, table):
    """the records of a wire batch by the record format (crdt_types.h), every hint left 0: what the
    encoder emitted before the hints.  `table`: the document's agent names (ids in creation order)"""
    recs = []

    def res(name):
        return ROOT_AGENT if name == "ROOT" else table.index(name) if name in table else UNKNOWN_AGENT
    for agent, seq, parents, ops in txns:
        if agent != "ROOT" and agent not in table:
            table.append(agent)
        author = res(agent)
        tl = sum(o[5] for o in ops)
        zero = any(o[5] == 0 or o[5] > 0x0FFFFFFF for o in ops)
        has_del = any(o[0] for o in ops)
        if (len(ops) == 1 and len(parents) == 1 and author < 0xFFFE and seq >= 1 and res(parents[0][0]) == author
                and parents[0][1] == seq - 1):
            k, an, asq, bn, bsq, ln = ops[0]
            ok = 1 <= ln <= 0x7FF
            e2 = e3 = 0
            if ok and k == 0:
                for nm, sq, which in ((an, asq, 2), (bn, bsq, 3)):
                    a = res(nm)
                    enc = M32 if a == ROOT_AGENT else sq
                    ok = ok and (a == ROOT_AGENT or (a == author and sq != M32))
                    if which == 2:
                        e2 = enc
                    else:
                        e3 = enc
            elif ok:
                ok = res(an) == author and asq != M32
                e2 = asq
            if ok:
                recs.append(((REC_RC << 28) | ((1 if k else 0) << 27) | (ln << 16) | author, seq, e2, e3))
                continue
        if len(ops) > 0x03FFFFFF or len(parents) > 0xFFFF:  # a count past its header field: malformed
            zero = True
        recs.append(((REC_RTXN << 28) | (int(zero) << 27) | (int(has_del) << 26) | (len(ops) & 0x03FFFFFF),
                     (author & 0xFFFF) | ((len(parents) & 0xFFFF) << 16), seq, min(tl, M32)))
        for k, an, asq, bn, bsq, ln in ops:
            if k == 0:
                recs.append(((REC_RINS << 28) | (ln & 0x0FFFFFFF), (res(an) & 0xFFFF) | ((res(bn) & 0xFFFF) << 16), asq, bsq))
            else:
                recs.append(((REC_RDEL << 28) | (ln & 0x0FFFFFFF), res(an) & 0xFFFF, asq, 0))
        for pn, ps in parents:
            recs.append((REC_RPARENT << 28, res(pn) & 0xFFFF, ps, 0))
    return recs


def hint_of(recs, j, end):
    """(back, m) of the RC delete record j by the definition: the records j .. j+m-1 (before `end`,
    the end of j's batch) are RC deletes of one item by one author, w1 rises by 1 from record to
    record, w2 moves by one constant step of +1 or -1; m is maximal"""
    w0, w1, w2 = recs[j][:3]
    m, d = 1, None
    if (w0 >> 16) & 0x7FF == 1:
        while j + m < end:
            p, r = recs[j + m - 1], recs[j + m]
            step = (r[2] - p[2]) & M32
            if r[0] != w0 or r[1] != (p[1] + 1) & M32 or step not in (1, M32) or (d is not None and step != d):
                break
            d = step
            m += 1
    return d == M32, m


def check_dump(got, batches):
    """got: encode_dump's lines; batches: the wires' parsed txns, in staging order.  Every word of
    every record is compared; returns the RC delete records' hints in stream order"""
    table, want, ends = [], [], []
    for txns in batches:
        want += ref_encode(txns, table)
        ends.append(len(want))
    assert len(got) == len(want)
    assert [g[0] for g in got] == [0 if i < ends[0] else 1 for i in range(len(got))]
    recs = [g[1:] for g in got]
    hints = []
    for j, (r, w) in enumerate(zip(recs, want)):
        assert r[:3] == w[:3], (j, [hex(x) for x in r], [hex(x) for x in w])
        if r[0] >> 27 == RC_DEL:
            back, m = hint_of(recs, j, ends[0] if j < ends[0] else ends[-1])
            assert r[3] == (BACK if back else 0) | m, (j, hex(r[3]), back, m)
            hints.append(r[3])
        else:
            assert r[3] == w[3], (j, hex(r[3]), hex(w[3]))
    return hints


# ------------------------------------------------------------------ hand-built batches
class Stream:
    """txns of a wire, built directly (the encoder looks at the records' shape alone, not at whether
    the history could be applied): every txn has its author's previous txn as the only parent"""

    def __init__(self):
        self.txns, self.seq = [], {}

    def txn(self, agent, ops, parents=None):
        s = self.seq.get(agent, 0)
        ps = parents if parents is not None else ([(agent, s - 1)] if s else [("ROOT", M32)])
        self.txns.append((agent, s, ps, ops))
        self.seq[agent] = s + sum(o[5] for o in ops)
        return self

    def base(self, agent="a", n=600):
        return self.txn(agent, [(0, "ROOT", M32, "ROOT", M32, n)])

    def dele(self, target, ln=1, agent="a", of=None):
        return self.txn(agent, [(1, of or agent, target, None, 0, ln)])

    def ins(self, left, agent="a"):
        return self.txn(agent, [(0, agent, left, agent, left + 1, 1)])

    def steps(self, start, steps, agent="a"):  # one-item deletes: the first at `start`, then moving by `steps`
        t = start
        self.dele(t, agent=agent)
        for d in steps:
            t += d
            self.dele(t, agent=agent)
        return self


def wire_of(s):
    w = build_wire(s.txns)
    assert parse_wire(w)[1] == [(a, q, list(p), list(o)) for a, q, p, o in s.txns]
    return w


@pytest.mark.parametrize("n", [1, 2, 3, 130])
@pytest.mark.parametrize("d", [-1, 1], ids=["back", "forward"])
def test_single_runs(dump, n, d):
    s = Stream().base().steps(300, [d] * (n - 1)).ins(10)
    hints = check_dump(dump(wire_of(s)), [s.txns])
    b = BACK if d < 0 else 0
    assert hints == [(b | m) if m > 1 else 1 for m in range(n, 0, -1)]


def test_direction_flip(dump):
    # steps -1, -1, +1, +1, -1: targets 300 299 298 299 300 299; a record that ends one run starts the next
    s = Stream().base().steps(300, [-1, -1, 1, 1, -1])
    hints = check_dump(dump(wire_of(s)), [s.txns])
    assert hints == [BACK | 3, BACK | 2, 3, 2, BACK | 2, 1]


def test_len2_in_the_middle(dump):
    s = Stream().base().steps(300, [-1, -1]).dele(296, ln=2).steps(295, [-1, -1])
    hints = check_dump(dump(wire_of(s)), [s.txns])
    assert hints == [BACK | 3, BACK | 2, 1, 1, BACK | 3, BACK | 2, 1]
    # ... and a len-2 delete whose target would continue the run
    s = Stream().base().steps(300, [1]).dele(302, ln=2).steps(304, [1])
    assert check_dump(dump(wire_of(s)), [s.txns]) == [2, 1, 1, 2, 1]


def test_seq_gap(dump):
    # an insert between two deletes: the targets go on, the seqs do not
    s = Stream().base().steps(300, [-1]).ins(20).steps(298, [-1, -1])
    hints = check_dump(dump(wire_of(s)), [s.txns])
    assert hints == [BACK | 2, 1, BACK | 3, BACK | 2, 1]
    # the same target step with a seq that does not rise by one (a txn of another shape between: two ops)
    s = Stream().base().steps(300, [1]).txn("a", [(1, "a", 5, None, 0, 1), (1, "a", 9, None, 0, 1)]).steps(302, [1])
    assert check_dump(dump(wire_of(s)), [s.txns]) == [2, 1, 2, 1]


def test_two_authors_alternating(dump):
    s = Stream().base("a").base("b")
    for i in range(6):
        s.dele(300 - i, agent="a").dele(200 + i, agent="b")
    hints = check_dump(dump(wire_of(s)), [s.txns])
    assert hints == [1] * 12
    # an author deleting the other's items is no compact record: general form, no hint, and it ends a run
    s = Stream().base("a").base("b").steps(300, [-1, -1], "a").dele(100, agent="a", of="b").steps(297, [-1], "a")
    got = dump(wire_of(s))
    assert check_dump(got, [s.txns]) == [BACK | 3, BACK | 2, 1, BACK | 2, 1]
    assert [g[4] for g in got if g[1] >> 28 == REC_RDEL] == [0]


def test_run_split_over_two_batches(dump):
    # the run goes on in the second batch: the first batch's hints stop at its end, the second
    # batch's pass does not touch them, and its own records count from where they stand
    s1 = Stream().base().steps(300, [-1] * 4)
    s2 = Stream()
    s2.seq = dict(s1.seq)
    s2.steps(295, [-1] * 2).ins(3)
    got = dump(wire_of(s1), wire_of(s2))
    assert check_dump(got, [s1.txns, s2.txns]) == [BACK | 5, BACK | 4, BACK | 3, BACK | 2, 1, BACK | 3, BACK | 2, 1]
    # staged as one batch it is one run
    s = Stream().base().steps(300, [-1] * 7).ins(3)
    assert check_dump(dump(wire_of(s)), [s.txns])[:3] == [BACK | 8, BACK | 7, BACK | 6]


@pytest.mark.parametrize("name", TRACE_NAMES)
def test_committed_traces(dump, name):
    w = load_remote_wire(name)
    hints = check_dump(dump(w), [parse_wire(w)[1]])
    # (the traces do hold runs in both directions: the comparison above is not vacuous)
    assert any(h & BACK and h & ~BACK > 1 for h in hints) and any(not h & BACK and h > 1 for h in hints)


# ------------------------------------------------------------------ the replay reads them
def _valid_streams():
    """name -> local edit script of a history the oracle can apply: a base text and the run shapes above"""
    def back(pos, k):
        return [(pos - i, 1, 0) for i in range(k)]

    def fwd(pos, k):
        return [(pos, 1, 0)] * k
    out = {
        "back130": back(400, 130),
        "fwd130": fwd(100, 130),
        "back200": back(450, 200),  # (splits a 32-entry leaf more than once: the closed-form cycles)
        "flip": back(300, 3) + fwd(298, 2) + back(297, 2),
        "len2": back(300, 3) + [(296, 2, 0)] + back(295, 3) + fwd(10, 2) + [(10, 2, 0)] + fwd(10, 3),
        "gap": back(300, 2) + [(20, 0, 1)] + back(300, 3) + fwd(40, 2) + [(5, 0, 1)] + fwd(41, 3),
        "cut": [(100, 0, 1)] + back(110, 30) + [(300, 0, 2)] + fwd(290, 30),
    }
    out = {k: [(0, 0, 600)] + v for k, v in out.items()}
    # one run that outgrows the planned leaves of the 4-entry layout: the replay stops inside the
    # run on capacity and resumes at a record in its middle, whose own hint counts the rest
    out[GROWS] = [(0, 0, 1000)] + back(900, 700)
    return out


GROWS = "back700"


@functools.lru_cache(maxsize=None)
def _valid_wires():
    from oracle_lib import trace_to_wire
    return {k: trace_to_wire(np.ones(len(v), np.uint32), np.array(v, np.uint32)) for k, v in _valid_streams().items()}


@pytest.mark.parametrize("L", [32, 4])
def test_emulated_replay_matches_oracle(L):
    from emu_lib import EmuDoc, diff_states
    from oracle_lib import OracleDoc
    layouts = {32: (32, 16), 4: (4, 8)}
    for name, w in _valid_wires().items():
        o = OracleDoc(*layouts[L])
        assert o.apply_remote_wire(w) == 0, name
        e = EmuDoc(L)
        assert e.run_wire(w) == 0, name
        assert e.check() == "", name
        assert diff_states(e.export(), o.export()) == [], name
        if name == GROWS and L == 4:
            assert e.sizes()["grow_events"] > 0
