"""CPU checks of the causal-version definition (tests/diff_vv_ref.py) on oracle exports, and of the
library's entry points for it being declared, bound and exported.

Content is np.arange(next_order), so a text is the list of its visible items' orders and ins_order
is the inserted content.

  Prefix equivalence: every order prefix is a version vector, and on those vectors ref_diff_vv is
  ref_diff_between, array for array.
  Patch application: the patches of (vv_from, vv_to), applied to the visible items of S_from in
  document order, give the visible items of S_to -- for prefixes and for random vectors, which are
  neither prefixes nor causally closed.
  Replica independence: two replicas that applied one gossip history in two delivery orders number
  its orders differently, and a vector, translated by agent name, names the same state on both.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import crdt_amd
from diff_between_ref import ref_diff_between
from diff_ref import apply_patches
from diff_vv_cases import (DIFF2_LONG, DIFF_T, LONG_VECTORS, MANY_VECTORS, NEIGHBOUR_VECTORS, cut_vectors, long_span,
                           many_spans, neighbour_deletes, vector)
from diff_vv_ref import (ids_by_order, items, members, next_seqs, ref_diff_vv, ref_version_vector, ref_vv_closed, text_at)
from fuzz_gen import GOSSIP_ORDERS, concurrent_wire, gossip_family, parse_wire
from oracle_lib import OracleDoc
from test_diff_ref import LAYOUTS, double_delete_txns, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VV_SYMBOLS = ["crdt_version_vector", "crdt_version_vector_dev_async", "crdt_diff_vv_async", "crdt_diff_vv_closed",
              "crdt_test_set_vv_lds_words"]


def same(x, y):
    return x[0].shape == y[0].shape and np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def sampled_versions(ex):
    """0, the version, every txn record's first order and one past it, and the orders around 32"""
    n = int(ex["next_order"])
    tx = np.asarray(ex["txns"], dtype=np.int64).reshape(-1, 5)
    vs = {0, n, n - 1} | {int(t) for t in tx[:, 0]} | {int(t) + 1 for t in tx[:, 0]} | {31, 32, 33}
    return sorted(v for v in vs if 0 <= v <= n)


def check_prefix_pairs(ex, versions):
    vvs = {v: ref_version_vector(ex, v) for v in versions}
    n_pat = 0
    for a in versions:
        assert ref_vv_closed(ex, vvs[a]), a      # a state the replica went through is closed
        ta = text_at(ex, vvs[a])
        for b in versions:
            got = ref_diff_vv(ex, vvs[a], vvs[b])
            assert same(got, ref_diff_between(ex, a, b)), (a, b)
            assert np.array_equal(apply_patches(ta, got[0], got[1]), text_at(ex, vvs[b])), (a, b)
            n_pat += got[0].shape[0]
    return n_pat


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", range(4))
def test_prefix_vectors_give_the_two_version_diff_on_fuzz_documents(seed, layout):
    txns = parse_wire(concurrent_wire(seed)[0])[1]
    ex = replay(txns, layout).export()
    vs = sampled_versions(ex)[::3] + [int(ex["next_order"])]
    assert check_prefix_pairs(ex, sorted(set(vs))) > len(vs)


@pytest.mark.parametrize("swap", [False, True])
def test_prefix_vectors_on_double_deletes(swap):
    txns = double_delete_txns()
    if swap:
        txns = [txns[0], txns[2], txns[1]]
    ex = replay(txns).export()
    assert check_prefix_pairs(ex, list(range(19))) > 0
    # B's delete [2, 6) alone, C's alone, both: items 4 and 5 are deleted by either
    a, b, c = (replay(txns).agent(x) for x in "ABC")
    vv = np.zeros(3, np.uint32)
    vv[a] = 10
    assert text_at(ex, vv).tolist() == list(range(10))
    only_b, only_c = vv.copy(), vv.copy()
    only_b[b] = 4
    only_c[c] = 4
    assert text_at(ex, only_b).tolist() == [0, 1, 6, 7, 8, 9]
    assert text_at(ex, only_c).tolist() == [0, 1, 2, 3, 8, 9]
    p, ins = ref_diff_vv(ex, only_b, only_c)
    assert p.tolist() == [[2, 2, 2, 0]] and ins.tolist() == [2, 3]   # (4 and 5, in neither text, close nothing)
    assert ref_vv_closed(ex, only_b) and ref_vv_closed(ex, only_c)
    # B's delete without the items it deletes: not closed, and nothing to see
    orphan = np.zeros(3, np.uint32)
    orphan[b] = 4
    assert not ref_vv_closed(ex, orphan) and text_at(ex, orphan).shape[0] == 0


def test_prefix_vectors_on_gossip_histories():
    n_pat = 0
    for _seed, _k, w in gossip_family("A"):
        o = OracleDoc()
        assert o.apply_remote_wire(w) == 0
        ex = o.export()
        n_pat += check_prefix_pairs(ex, sampled_versions(ex)[::12] + [int(ex["next_order"])])
    assert n_pat > 1000


@pytest.mark.parametrize("seed", range(4))
def test_patches_of_random_vectors_apply(seed):
    # vectors drawn per agent in [0, next seq]: S is no order prefix and mostly not causally closed
    # (a delete op without its target, an insert without its origin); the walk does not care
    txns = parse_wire(concurrent_wire(seed)[0])[1]
    ex = replay(txns).export()
    nxt = next_seqs(ex)
    rng = np.random.default_rng(seed)
    vvs = [rng.integers(0, nxt + 1).astype(np.uint32) for _ in range(12)] + [nxt.astype(np.uint32), np.zeros(0, np.uint32)]
    texts = [text_at(ex, v) for v in vvs]
    open_seen = n_pat = 0
    for i, a in enumerate(vvs):
        open_seen += not ref_vv_closed(ex, a)
        for j, b in enumerate(vvs):
            pat, ins = ref_diff_vv(ex, a, b)
            assert int(pat[:, 2].sum()) == ins.shape[0]
            assert np.array_equal(apply_patches(texts[i], pat, ins), texts[j]), (a, b)
            back = ref_diff_vv(ex, b, a)[0]
            assert np.array_equal(back[:, 1], pat[:, 2]) and np.array_equal(back[:, 2], pat[:, 1])
            if i == j:
                assert pat.shape[0] == 0
            n_pat += pat.shape[0]
    assert open_seen >= 6 and n_pat > 100
    assert texts[-1].shape[0] == 0                              # the zero vector (here of length 0)
    assert np.array_equal(texts[-2], text_at(ex, ref_version_vector(ex, ex["next_order"])))
    with pytest.raises(ValueError):
        text_at(ex, (nxt + (np.arange(len(nxt)) == 1)).astype(np.uint32))   # an entry above the next seq
    with pytest.raises(ValueError):
        text_at(ex, np.concatenate([nxt, [1]]).astype(np.uint32))           # an agent the document has not


def replicas(fam):
    """per history of a gossip family: its GOSSIP_ORDERS replays as (export, {agent id: name})"""
    hist = gossip_family(fam)
    for s in range(0, len(hist), GOSSIP_ORDERS):
        reps = []
        for _seed, _k, w in hist[s:s + GOSSIP_ORDERS]:
            o = OracleDoc()
            assert o.apply_remote_wire(w) == 0
            reps.append((o.export(), {o.agent(n): n for n in parse_wire(w)[0] if n != "ROOT"}))
        yield reps


def named_ids(ex, names, orders):
    """(agent name, seq) of the listed orders: what two replicas can compare"""
    agent, seq = ids_by_order(ex)
    return [(names[int(agent[x])], int(seq[x])) for x in orders]


def translate(vv, names_from, names_to):
    ids_to = {n: a for a, n in names_to.items()}
    out = np.zeros(len(names_to), np.uint32)
    for a, x in enumerate(vv):
        out[ids_to[names_from[a]]] = x
    return out


def test_a_vector_names_the_same_state_on_replicas_with_other_delivery_orders():
    """The reason for version vectors.  For every history of gossip family A and each of its two
    causal shuffles against the log order (8 pairs of replicas): the vector of EVERY order prefix of
    either replica -- every state either went through, each causally closed -- is translated to the
    other replica by agent name; so are 80 unions per pair of a prefix of one replica with a prefix
    of the other (closed, and in general a prefix of neither), and whatever ref_vv_closed accepts of
    200 random vectors per pair.  On every pair each must be closed on the other replica too and
    the visible ids must be the same set.

    The text as a sequence can only agree where the two replicas' documents do: the full vector is
    one of the vectors, and its text is the replica's final text.  Delivery orders do not converge
    in the restated reference (entry merging depends on arrival order; fuzz_gen's
    gossip_log says the same), so the pairs split by the oracle's own final id sequences, before
    any vector is looked at:
      6 of the 8 pairs end with the same id sequence: there the text at every vector, and the text
        of the diff from the zero vector, must be equal id for id;
      on the other 2 (seeds 1 and 2, first shuffle) the final texts differ, and with them the text
        at 295 of 804 and 137 of 842 vectors; only the set form is asserted there.
    (328 of the 640 unions are a prefix of neither replica; of the 1,600 random vectors 1 is closed.)"""
    strict = loose = vectors = unions = no_prefix = drawn = 0
    rng = np.random.default_rng(41)
    differ = []  # per pair that did not converge: (vectors, vectors whose texts differ as sequences)
    for reps in replicas("A"):
        (ex0, nm0) = reps[0]
        final0 = named_ids(ex0, nm0, items(ex0))
        for ex1, nm1 in reps[1:]:
            converged = named_ids(ex1, nm1, items(ex1)) == final0
            strict += converged
            loose += not converged
            if not converged:
                differ.append([0, 0])
            sides = ((ex0, nm0, ex1, nm1), (ex1, nm1, ex0, nm0))
            for exa, nma, exb, nmb in sides:
                n_a, n_b = int(exa["next_order"]), int(exb["next_order"])
                todo = [ref_version_vector(exa, v, len(nma)) for v in range(n_a + 1)]
                prefixes = {tuple(x.tolist()) for x in todo}
                for _ in range(40):  # a prefix of this replica joined with a prefix of the other
                    u = np.maximum(ref_version_vector(exa, rng.integers(0, n_a + 1), len(nma)),
                                   translate(ref_version_vector(exb, rng.integers(0, n_b + 1), len(nmb)), nmb, nma))
                    todo.append(u)
                    unions += 1
                    no_prefix += tuple(u.tolist()) not in prefixes
                nxt = np.zeros(len(nma), np.int64)
                nxt[:len(next_seqs(exa))] = next_seqs(exa)
                for _ in range(100):  # random vectors, those that are closed
                    u = rng.integers(0, nxt + 1).astype(np.uint32)
                    if ref_vv_closed(exa, u):
                        todo.append(u)
                        drawn += 1
                for v, vva in enumerate(todo):
                    vvb = translate(vva, nma, nmb)
                    assert ref_vv_closed(exa, vva) and ref_vv_closed(exb, vvb), v
                    ta, tb = named_ids(exa, nma, text_at(exa, vva)), named_ids(exb, nmb, text_at(exb, vvb))
                    assert sorted(ta) == sorted(tb), v
                    vectors += 1
                    if not converged:
                        differ[-1][0] += 1
                        differ[-1][1] += ta != tb
                    if converged:
                        assert ta == tb, v
                        if v % 8 == 0 or v > n_a:  # the diff from nothing inserts that text
                            pat, ins = ref_diff_vv(exb, np.zeros(0, np.uint32), vvb)
                            assert named_ids(exb, nmb, ins) == ta and pat.shape[0] == (1 if ta else 0), v
    print("pairs that converge", strict, "that do not", loose, "(vectors, differing texts)", differ,
          "unions", unions, "of them no prefix", no_prefix, "closed random vectors", drawn)
    assert strict == 6 and loose == 2 and vectors > 4000, (strict, loose, vectors)
    assert unions == 640 and no_prefix > unions // 4, (unions, no_prefix)


def test_closed_flags_of_the_reference():
    txns = parse_wire(concurrent_wire(2)[0])[1]
    ex = replay(txns).export()
    n = int(ex["next_order"])
    tx = np.asarray(ex["txns"], dtype=np.int64).reshape(-1, 5)
    par = np.asarray(ex["parents"], dtype=np.int64)
    agent, seq = ids_by_order(ex)
    full = ref_version_vector(ex, n)
    assert ref_vv_closed(ex, full) and ref_vv_closed(ex, np.zeros(0, np.uint32))
    # a txn whose parent is another agent's: keep it, drop the parent
    cut = 0
    for order, _ln, _sh, poff, pn in tx:
        for p in par[poff:poff + pn]:
            if p != 0xFFFFFFFF and agent[p] != agent[order]:
                vv = full.copy()
                vv[agent[p]] = seq[p]          # the parent's agent stops just before the parent
                if vv[agent[order]] > seq[order]:
                    assert not ref_vv_closed(ex, vv), (order, p)
                    cut += 1
    assert cut > 3


def oracle_of(txns):
    o = replay(txns)
    return o.export(), {n: o.agent(n) for n in {t[0] for t in txns}}


def check_named_vectors(ex, ids, named):
    vvs = [vector(v, ids) for v in named]
    texts = [text_at(ex, v) for v in vvs]
    n_pat = 0
    for i, a in enumerate(vvs):
        for j, b in enumerate(vvs):
            pat, ins = ref_diff_vv(ex, a, b)
            assert np.array_equal(apply_patches(texts[i], pat, ins), texts[j]), (named[i], named[j])
            n_pat += pat.shape[0]
    return vvs, texts, n_pat


def test_the_hand_built_cases_have_the_shapes_they_are_for():
    # two agents' delete txns in one delete-log run, and a vector that holds only its second order
    ex, ids = oracle_of(neighbour_deletes())
    assert np.asarray(ex["deletes"]).reshape(-1, 3).tolist() == [[10, 3, 2]]
    vvs, texts, _ = check_named_vectors(ex, ids, NEIGHBOUR_VECTORS)
    only_c = vector({"A": 10, "C": 1}, ids)
    assert members(ex, only_c)[[10, 11]].tolist() == [False, True]
    assert text_at(ex, only_c).tolist() == [0, 1, 2, 3, 5, 6, 7, 8, 9]
    assert not ref_vv_closed(ex, only_c)                        # C's txn without its parent, B's
    assert ref_vv_closed(ex, vector({"A": 10, "B": 1}, ids))
    assert not ref_vv_closed(ex, vector({"C": 1}, ids))         # a delete op without the items it needs
    assert not ref_vv_closed(ex, vector({"A": 4, "C": 1}, ids))
    assert ref_diff_vv(ex, vector({"A": 10, "B": 1}, ids), only_c)[0].tolist() == [[3, 1, 1, 0]]
    # one canonical span of more than DIFF2_LONG orders, cut by the vectors at several places
    ex, ids = oracle_of(long_span())
    canon = np.asarray(ex["canon"], np.uint32).reshape(-1, 4)
    assert canon[:, [0, 3]].tolist() == [[0, 10], [10, 0x100000000 - 20], [30, 520], [550, 0x100000000 - 5], [555, 145]]
    assert 520 > DIFF2_LONG and np.asarray(ex["cwo"]).reshape(-1, 4).shape[0] == 5
    _, texts, n_pat = check_named_vectors(ex, ids, LONG_VECTORS)
    assert n_pat > 150
    assert texts[3].tolist() == list(range(300)) + list(range(600, 650))   # (Y's 300 orders left out)
    assert texts[6].tolist() == list(range(10))
    # more than DIFF_T canonical spans
    ex, ids = oracle_of(many_spans())
    assert np.asarray(ex["canon"]).reshape(-1, 4).shape[0] > DIFF_T
    _, texts, n_pat = check_named_vectors(ex, ids, MANY_VECTORS)
    assert n_pat > 300
    # the cuts: inside runs, around order 32, on runs' edges -- no two alike
    ex = replay(parse_wire(concurrent_wire(1)[0])[1]).export()
    cuts = cut_vectors(ex)
    assert len(cuts) >= 12 and len({tuple(v.tolist()) for v in cuts}) >= 10


def test_library_declares_binds_and_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "crdt_gpu.h")).read()
    declared = set(re.findall(r"\b(crdt_[a-z_0-9]+)\s*\(", header))
    crdt_amd.build()
    lib = ctypes.CDLL(crdt_amd.LIB_PATH)
    for s in VV_SYMBOLS:
        assert s in declared, s
        assert s in crdt_amd.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    for m in ("version_vector", "diff_vv", "diff_vv_async", "diff_vv_closed"):
        assert callable(getattr(crdt_amd.Engine, m)), m
    assert crdt_amd.lib().crdt_diff_vv_async.argtypes is not None
