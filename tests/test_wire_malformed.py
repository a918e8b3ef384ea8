"""Malformed remote wire batches against the host parser (host_plan.h WireView::parse): a wire is a
peer's input, so every truncation and every single-word corruption of two small batches goes
through tests/hints/encode_dump.cpp -- a stand-alone program around WireView::parse + encode_remote,
built with -fsanitize=address,undefined as tests/test_delete_hints.py builds it -- and must be
either parsed (exit 0) or refused (exit 3): no other exit, nothing on stderr.

What is expected comes from `parse_strict` below, the wire format restated from the comment in
include/crdt_gpu.h ("Remote wire batch"), not from the parser under test or the oracle's:

  'RTX1' | n_names | n_names x {byte_len, bytes, pad to 4} | n_txns | n_txns x {agent_name, seq,
  n_parents, n_ops, n_parents x {name, seq}, n_ops x {kind, a_name, a_seq, b_name, b_seq, len}}

Every field lies inside the buffer, the pad of a name included; every name index that is read is
below n_names (a Del's b is not read); kind is 0 or 1.  Three choices the comment records and this
test pins: names are bytes (no UTF-8 check), pad bytes are not looked at, bytes after the last txn
are ignored.  For a wire that is accepted, the printed records are compared word by word with
test_delete_hints.check_dump (the record format restated there).

The counts of a wire size the parser's tables, so a corrupted n_names / n_txns must be refused by
the length check before anything is sized by it: those cases run once more against a build without
sanitizers under an address-space limit (RLIMIT_AS, below) that the tables would not fit in."""
import concurrent.futures
import os
import resource
import struct
import subprocess

import pytest

from fuzz_gen import build_wire
from test_delete_hints import CSRC, ROOT, check_dump

MAGIC = 0x31585452
M32 = 0xFFFFFFFF
R = ("ROOT", M32)
VALUES = (0, 1, 2, 3, 7, 0xFFFE, 0xFFFF, 0x10000, 0x0FFFFFFF, 0x10000000, 0x7FFFFFFF, 0xFFFFFFFD, 0xFFFFFFFF)

# The address-space limit of the unsanitized runs.  The program itself maps its image, libstdc++ and
# libc, a stack and the wires it reads (0.6 MiB at most) -- a few tens of MiB, and the valid wires
# that run under the same limit show that it suffices; n_names = 0x0FFFFFFF (the smallest corrupted count
# of VALUES that matters) would size the name table at 0x0FFFFFFF * sizeof(std::string) = 8 GiB and
# the txn table at 0x0FFFFFFF * 40 bytes = 10 GiB: 32 to 40 times the limit.
RLIMIT_AS_BYTES = 256 << 20


# ------------------------------------------------------------------ the format, restated
class _Bad(Exception):
    pass


def parse_strict(w):
    """(names, txns) of a well-formed wire -- txns as fuzz_gen.parse_wire gives them, names decoded
    byte for byte (latin-1) -- or None"""
    n, off = len(w), 0

    def rd():
        nonlocal off
        if off + 4 > n:
            raise _Bad
        off += 4
        return struct.unpack_from("<I", w, off - 4)[0]

    def name(i):
        if i >= len(names):
            raise _Bad
        return names[i]
    try:
        if rd() != MAGIC:
            return None
        nn = rd()
        if 4 * nn > n - off:  # (each name takes at least its length word: no loop of 2^32 rounds)
            return None
        names = []
        for _ in range(nn):
            bl = rd()
            end = off + ((bl + 3) & ~3)
            if end > n:
                return None
            names.append(w[off:off + bl].decode("latin-1"))
            off = end
        nt = rd()
        if 16 * nt > n - off:
            return None
        txns = []
        for _ in range(nt):
            a, s, np_, no = rd(), rd(), rd(), rd()
            agent = name(a)
            if 8 * np_ + 24 * no > n - off:
                return None
            ps = [(name(rd()), rd()) for _ in range(np_)]
            ops = []
            for _ in range(no):
                k, an, asq, bn, bsq, ln = rd(), rd(), rd(), rd(), rd(), rd()
                if k > 1:
                    return None
                ops.append((k, name(an), asq, name(bn) if k == 0 else None, bsq, ln))
            txns.append((agent, s, ps, ops))
        return names, txns
    except _Bad:
        return None


def well_formed(w):
    return parse_strict(w) is not None


# ------------------------------------------------------------------ the two base wires
def base_wires():
    """full: two authors whose names (5 and 2 bytes) are no multiple of 4, a multi-op txn, a
    multi-parent txn, a compact record; empty: no names, no txns"""
    full = build_wire([
        ("alice", 0, [R], [(0, "ROOT", M32, "ROOT", M32, 3)]),
        ("bo", 0, [("alice", 2)], [(0, "alice", 0, "alice", 1, 1), (1, "alice", 2, None, 0, 1)]),
        ("alice", 3, [("alice", 2), ("bo", 1)], [(0, "bo", 0, "alice", 1, 1)]),
        ("alice", 4, [("alice", 3)], [(1, "alice", 3, None, 0, 1)]),
    ])
    return {"full": full, "empty": struct.pack("<III", MAGIC, 0, 0)}


def count_words(w):
    """word indices of n_names and n_txns"""
    names, _ = parse_strict(w)
    off = 8
    for nm in names:
        off += 4 + ((len(nm) + 3) & ~3)
    return 1, off // 4


def set_word(w, i, v):
    return w[:4 * i] + struct.pack("<I", v) + w[4 * i + 4:]


def mutations(w):
    """[(label, bytes)]: every truncation, every word replaced by every value of VALUES"""
    out = [(f"trunc{n}", w[:n]) for n in range(len(w))]
    for i in range(len(w) // 4):
        for v in VALUES:
            if struct.unpack_from("<I", w, 4 * i)[0] != v:
                out.append((f"word{i}={v:#x}", set_word(w, i, v)))
    return out


def with_parents(k):
    """a second txn with k parents (every one the first txn's last item)"""
    return build_wire([("alice", 0, [R], [(0, "ROOT", M32, "ROOT", M32, 3)]),
                       ("alice", 3, [("alice", 2)] * k, [(0, "alice", 2, "ROOT", M32, 1)])])


def special_cases():
    full = base_wires()["full"]
    out = [("wrong_magic", set_word(full, 0, MAGIC ^ 0x01000000)), ("no_magic", b"RTX2" + full[4:])]
    # the last name's length set so that its bytes run exactly to the end of the buffer, and one
    # byte past it; and a buffer cut so that the (unpadded) name is its last bytes, and one short
    names, _ = parse_strict(full)
    off = 8 + sum(4 + ((len(nm) + 3) & ~3) for nm in names[:-1])  # the last name's length word
    room = len(full) - (off + 4)
    out += [("name_to_end", set_word(full, off // 4, room)), ("name_past_end", set_word(full, off // 4, room + 1))]
    one = struct.pack("<III", MAGIC, 1, 5) + b"alice"
    out += [("name_is_the_tail", one), ("name_tail_short", one[:-1]), ("name_padded_no_txns", one + b"\0" * 3)]
    out += [("name_padded_0_txns", one + b"\0" * 3 + struct.pack("<I", 0))]
    # bytes behind the last txn are ignored (pinned: accepted today)
    out += [("trailing_word", full + struct.pack("<I", 7)), ("trailing_byte", full + b"\x01"),
            ("empty_trailing", base_wires()["empty"] + b"\xff" * 9)]
    out += [("parents_65535", with_parents(65535)), ("parents_65536", with_parents(65536))]
    return out


def test_reference_on_known_wires():
    # the restated format agrees with the writer (fuzz_gen.build_wire) on what a valid wire holds,
    # and refuses the cases whose verdict is clear from the format alone
    from fuzz_gen import parse_wire
    for w in base_wires().values():
        got = parse_strict(w)
        assert got is not None and (got[0], got[1]) == parse_wire(w)
    want = {"wrong_magic": False, "no_magic": False, "name_to_end": False, "name_past_end": False,
            "name_is_the_tail": False, "name_tail_short": False, "name_padded_no_txns": False,
            "name_padded_0_txns": True, "trailing_word": True, "trailing_byte": True, "empty_trailing": True,
            "parents_65535": True, "parents_65536": True}
    assert {k: well_formed(w) for k, w in special_cases()} == want
    full = base_wires()["full"]
    assert not any(well_formed(full[:n]) for n in range(len(full)))  # (its last txn ends the buffer)
    i_names, i_txns = count_words(full)
    for v in VALUES:
        if v == 3 or 4 * v > len(full):  # (a small wrong count reads txn words as names: either verdict)
            assert well_formed(set_word(full, i_names, v)) == (v == 3)
        assert well_formed(set_word(full, i_txns, v)) == (v <= 4)  # (fewer txns: the rest is trailing bytes)


# ------------------------------------------------------------------ the program
def _compile(td, name, flags):
    exe = str(td / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", *flags, "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "hints", "encode_dump.cpp")],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    td = tmp_path_factory.mktemp("wire")
    return td, _compile(td, "encode_dump_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), \
        _compile(td, "encode_dump_plain", [])


def _limit_address_space():
    resource.setrlimit(resource.RLIMIT_AS, (RLIMIT_AS_BYTES, RLIMIT_AS_BYTES))


def run_cases(td, exe, cases, tag, limited=False):
    """every (label, wire) through `exe -q`: [(label, wire, returncode, stdout, stderr)]"""
    paths = []
    for k, (_label, w) in enumerate(cases):
        paths.append(str(td / f"{tag}{k}.rtx"))
        with open(paths[-1], "wb") as f:
            f.write(w)

    def one(p):
        return subprocess.run([exe, "-q", p], capture_output=True, text=True,
                              preexec_fn=_limit_address_space if limited else None)
    if limited:  # (preexec_fn and threads do not mix: these few run one by one)
        rs = [one(p) for p in paths]
    else:
        with concurrent.futures.ThreadPoolExecutor(8) as ex:
            rs = list(ex.map(one, paths))
    for p in paths:
        os.unlink(p)
    return [(label, w, r.returncode, r.stdout, r.stderr) for (label, w), r in zip(cases, rs)]


def check_results(results):
    """exit 0 when and only when the restated format accepts the wire, else exit 3; nothing on
    stderr; an accepted wire's records are the record format's.  Returns (accepted, refused)"""
    other = [(label, rc) for label, _w, rc, _o, _e in results if rc not in (0, 3)]
    assert not other, (len(other), other[:8])
    noisy = [(label, err[-400:]) for label, _w, _rc, _o, err in results if err]
    assert not noisy, (len(noisy), noisy[:2])
    wrong = [(label, rc) for label, w, rc, _o, _e in results if (rc == 0) != well_formed(w)]
    assert not wrong, (len(wrong), wrong[:8])
    n_ok = 0
    for label, w, rc, out, _e in results:
        if rc == 0:
            got = [tuple(int(x, 16) for x in ln.split()) for ln in out.splitlines()]
            try:
                check_dump(got, [parse_strict(w)[1]])
            except AssertionError as x:
                raise AssertionError(f"{label}: {x}") from None
            n_ok += 1
    return n_ok, len(results) - n_ok


@pytest.mark.parametrize("base", ["full", "empty"])
def test_every_truncation_and_every_word(programs, base):
    td, san, _plain = programs
    w = base_wires()[base]
    cases = mutations(w) + [("unchanged", w)]
    assert len(cases) > (1000 if base == "full" else 40)
    ok, bad = check_results(run_cases(td, san, cases, base))
    print(f"{base}: {len(cases)} wires, {ok} accepted, {bad} refused, 0 other exits, no sanitizer output")
    # both verdicts occur: a corrupted seq or length is still a wire, a corrupted count or index is not
    assert ok >= (len(w) // 4 if base == "full" else 1) and bad >= len(w)


def test_special_cases(programs):
    td, san, _plain = programs
    cases = special_cases()
    results = run_cases(td, san, cases, "special")
    check_results(results)
    rc = {label: r for label, _w, r, _o, _e in results}
    assert rc["trailing_word"] == rc["trailing_byte"] == rc["empty_trailing"] == 0  # pinned: ignored
    assert rc["name_to_end"] == rc["name_past_end"] == rc["name_is_the_tail"] == rc["name_tail_short"] == 3
    # 65,535 parents fit the header's 16-bit field; 65,536 do not, and the header says so (bit 27:
    # the replay stops there with CRDT_ERR_BAD_INPUT) instead of a count of 0 with 65,536 stray
    # parent records behind it
    heads = {}
    for label, _w, _r, out, _e in results:
        if label.startswith("parents_"):
            recs = [tuple(int(x, 16) for x in ln.split()) for ln in out.splitlines()]
            assert len(recs) == 3 + 2 + int(label[8:])
            heads[label] = recs[3]
    assert heads["parents_65535"][1] >> 27 == (3 << 1) and heads["parents_65535"][2] >> 16 == 0xFFFF
    assert heads["parents_65536"][1] >> 27 == (3 << 1) | 1


@pytest.mark.parametrize("base", ["full", "empty"])
def test_huge_counts_are_refused_by_the_length_check(programs, base):
    # without sanitizers, under RLIMIT_AS: a parser that sized a table by the count first would
    # die of std::bad_alloc here (an exit that is neither 0 nor 3) or be killed
    td, _san, plain = programs
    w = base_wires()[base]
    cases = [(f"word{i}={v:#x}", set_word(w, i, v)) for i in count_words(w) for v in VALUES]
    cases.append(("unchanged", w))
    results = run_cases(td, plain, cases, base + "_as", limited=True)
    ok, bad = check_results(results)
    assert ok >= 1 and bad >= 2 * sum(v >= 0x10000 for v in VALUES)


def test_wires_of_the_engine_tests_are_refused_cleanly(programs):
    # tests/test_gpu_hostile_streams.py hands these to the engine's staging entry points, in a
    # process that holds the GPU: here they are shown to end in a clean refusal, under sanitizers and
    # under the address-space limit, and the valid wires beside them to be taken
    import hostile_streams as hs
    td, san, plain = programs
    cases = list(hs.malformed_wires().items()) + [(f"valid{k}", w) for k, w in enumerate(hs.doc_wires(1))]
    for exe, limited in ((san, False), (plain, True)):
        results = run_cases(td, exe, cases, "engine", limited)
        assert check_results(results) == (3, len(hs.malformed_wires()))
        assert all(rc == 3 for label, _w, rc, _o, _e in results if not label.startswith("valid"))
