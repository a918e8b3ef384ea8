"""k_replay's LOCAL-record fast paths at every phase of the 64-record window: the hand-built scripts
of tests/local_streams.py on the engine against the oracle, bit-exact -- status, full export,
digest, and every pos -> loc / loc -> pos answer on one script per kind.

Local records (REC_LC) take code the remote window tests never run: the `compact && !remote`
branches of wave_gpu.h typing_scan_r and delete_scan_r, front_scan and leaf_insert_front,
leaf_delete_span / local_delete_pieces, the SHAPE_LOCAL instance of k_replay.  The CPU emulation
(tests/test_window_local_ref.py: the same scripts, branch reach by counters) compiles
tests/emu/wave_cpu.h, not wave_gpu.h, so a scan term lost on the GPU shows only here.

One engine per layout, one document per script.
 - two batches: the base insert, then the script -- staging resets the record cursor, so record k
   of a script sits in lane k of the first window; also on the two-level root (CRDT_FORCE_HBM_ROOT:
   the SHAPE_ALL instance that takes local records);
 - one launch: base insert and script staged as one batch (lane k + 1), run() with growth stops,
   then the same streams once more from reset in one launch, with the capacities that just held it;
 - probed: a PROBE record after every txn (LC, PROBE, LC, ...): every scan must stop at the PROBE.
Documents that end with an error status (the *_past_* runs, the all-empty-op txn) sit between good
ones: the oracle's status, the neighbours untouched, and no further txn taken."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crdt_amd  # noqa: E402
import local_streams as ls  # noqa: E402
from test_gpu_hroot import hroot  # noqa: E402,F401  (the CRDT_FORCE_HBM_ROOT fixture)
from test_gpu_parity import assert_same, check_queries  # noqa: E402

# one script per kind gets every query checked (a run that crosses the window's end), and one each
# of the span, near-miss and text-end families
QUERIED = [f"run65_pad30_{k}" for k in ls.KINDS] + ["span_skips_deleted_lane63", "span_whole_document_lane62",
                                                    "second_author_in_typing_pad60", "delete_in_front_pad30", "back_to_start_70"]


def names():
    return sorted(ls.scripts())


@functools.lru_cache(maxsize=None)
def arrays(what):
    """(docs, txn_off, txns [T, 2], ops [N, 3]) of every document's base insert / script / both"""
    tx, ops, off = [], [], [0]
    for name in names():
        s = {"base": ls.base_ops(), "stream": ls.scripts()[name][0], "both": ls.base_ops() + ls.scripts()[name][0]}[what]
        a, c, p = ls.flat(s)
        tx.append(np.stack([a, c], 1))
        ops.append(p)
        off.append(off[-1] + a.shape[0])
    return np.arange(len(names()), dtype=np.uint32), np.array(off, np.uint64), np.concatenate(tx), np.concatenate(ops)


def engine(leaf):
    n = len(names())
    e = crdt_amd.Engine(n, leaf)
    ids = e.agent_intern(np.repeat(np.arange(n), 2), list(ls.AUTHORS) * n)
    assert ids.reshape(n, 2).tolist() == [[0, 1]] * n
    return e


def compare(e, st, leaf, msg):
    """every document against the oracle: status; for status 0 the export and the digest"""
    ns = names()
    orc = ls.oracles(leaf)
    want_st = [orc[n][1] for n in ns]
    assert want_st == [ls.scripts()[n][1] for n in ns]
    got = [int(s) for s in st]
    assert got == want_st, (msg, [(n, g, w) for n, g, w in zip(ns, got, want_st) if g != w][:10])
    want = ls.oracle_exports(leaf)
    dg = e.digests()
    bad = []
    for d, n in enumerate(ns):
        if want_st[d] != 0:
            continue
        try:
            assert_same(e.export(d), want[n])
            assert int(dg[d]) == orc[n][0].digest(), "digest"
        except AssertionError as x:
            bad.append((n, " ".join(str(x).split())[:70]))
    assert not bad, (msg, len(bad), bad[:12])


def two_batches(leaf):
    ns = names()
    e = engine(leaf)
    assert (e.apply_local_arrays(*arrays("base")) == 0).all()
    st = e.apply_local_arrays(*arrays("stream"))
    compare(e, st, leaf, (leaf, "two batches"))
    for n in QUERIED:
        check_queries(e, ns.index(n), ls.oracles(leaf)[n][0])
    # the stopped documents take no further txn, and leave every other document as it is
    err = [ns.index(n) for n in ls.error_scripts()]
    assert len(err) == 6
    before = e.digests().copy()
    st2 = e.apply_local([(d, [(0, [(0, 0, 1)])]) for d in err])
    assert [int(s) for s in st2] == [ls.scripts()[ns[d]][1] for d in err], list(st2)
    good = np.array([ls.scripts()[n][1] == 0 for n in ns])
    assert np.array_equal(e.digests()[good], before[good])
    for d in err:
        for nb in (d - 1, d + 1):
            if 0 <= nb < len(ns) and good[nb]:
                assert_same(e.export(nb), ls.oracle_exports(leaf)[ns[nb]])
    e.close()


@pytest.mark.parametrize("leaf", [32, 4])
def test_two_batches(leaf):
    two_batches(leaf)


@pytest.mark.parametrize("leaf", [32, 4])
def test_two_batches_on_the_two_level_root(hroot, leaf):
    two_batches(leaf)


@pytest.mark.parametrize("leaf", [32, 4])
def test_one_launch(leaf):
    e = engine(leaf)
    e.apply_local_arrays(*arrays("both"), stage_only=True)
    compare(e, e.run(), leaf, (leaf, "one batch, growth"))
    # once more from reset, in one launch: the capacities held this very history a moment ago, so
    # no document may stop for capacity (ST_NEED_CAPACITY, -11, would show in the status)
    e.reset_async()
    e.run_async()
    e.sync()
    compare(e, e.status(), leaf, (leaf, "one batch, steady"))
    e.close()


def probes_of(ops, rng):
    """one probe per txn: the txn's position and its first item (author 0's seqs go on behind the
    base insert's); every other probe asks a random position (up to 2 past the end) and a random
    earlier seq instead"""
    out, seq = [], ls.BASE
    for k, (_a, tx) in enumerate(ops):
        pos, ask = tx[0][0], seq
        if k % 2:
            pos, ask = int(rng.integers(0, ls.BASE + 3)), int(rng.integers(0, seq + 1))
        out.append((pos, 0, ask))
        seq += sum(d + i for _p, d, i in tx)
    return np.array(out, np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("leaf", [32, 4])
def test_probed(leaf):
    # families A and E with a PROBE record behind every record: no run may be taken past a PROBE,
    # and every answer is the oracle's after the same txn
    from oracle_lib import OracleDoc
    pick = sorted(list(ls.family("A")) + list(ls.family("E")))
    n = len(pick)
    e = crdt_amd.Engine(n, leaf)
    assert (e.agent_intern(list(range(n)), [ls.AUTHORS[0]] * n) == 0).all()
    docs = np.arange(n, dtype=np.uint32)
    base = ls.flat(ls.base_ops())
    assert (e.apply_local_arrays(docs, np.arange(n + 1), np.tile(np.stack(base[:2], 1), (n, 1)), np.tile(base[2], (n, 1))) == 0).all()
    rng = np.random.default_rng(7)
    tx, ops, prs, off, want_st, want_ans = [], [], [], [0], [], []
    for name in pick:
        s = ls.scripts()[name][0]
        a, c, p = ls.flat(s)
        assert (a == 0).all()
        q = probes_of(s, rng)
        o = OracleDoc(*ls.LAYOUTS[leaf])
        assert o.agent(ls.AUTHORS[0]) == 0 and o.apply_local(0, ls.base_ops()[0][1]) == 0
        so, ans = o.probe_trace(0, c, p, q)
        assert so == ls.scripts()[name][1], name
        tx.append(np.stack([a, c], 1)), ops.append(p), prs.append(q), off.append(off[-1] + a.shape[0])
        want_st.append(so)
        want_ans.append(ans)
    st, ans = e.apply_local_probed(docs, off, np.concatenate(tx), np.concatenate(ops), np.concatenate(prs))
    assert [int(s) for s in st] == want_st, list(st)
    assert sum(s != 0 for s in want_st) == 4
    for d, name in enumerate(pick):
        got, want = ans[off[d]:off[d + 1]], want_ans[d]
        if want_st[d] != 0:  # the last txn failed: the answers behind every txn before it
            got, want = got[:-1], want[:-1]
        bad = np.argwhere((got != want).any(1))
        assert bad.size == 0, (name, int(bad[0][0]), got[bad[0][0]], want[bad[0][0]])
    dg = e.digests()
    for d, name in enumerate(pick):
        if want_st[d] == 0:
            assert int(dg[d]) == ls.oracles(leaf)[name][0].digest(), name
    e.close()
