"""The numpy reference of the published index (tests/index_ref.py) against the oracle, and the
coverage conditions of the generated documents that tests/test_gpu_index_edges.py publishes: which
boundary-resolution cases of k_publish_big they reach is proven here, without a GPU."""
import functools

import numpy as np
import pytest

from crdt_amd.traces import load_trace
from fuzz_gen import concurrent_wire, config5_wire, random_local_trace
from kernel_consts import GROUP, PUB_BIG_MAX, PUB_BIG_MIN, PUB_BIG_WAVES, kernel_consts
from oracle_lib import OracleDoc
import index_ref as R

TRACES = ["sveltecomponent", "rustcode", "automerge-paper"]


@functools.lru_cache(maxsize=None)
def oracle_of(name: str, L: int):
    o = OracleDoc(*R.LAYOUTS[L])
    if name in TRACES:
        t = load_trace(name)
        assert o.apply_trace(o.agent("jeremy"), t.counts, t.patches) == 0
    elif name.startswith("random"):
        c, p = random_local_trace(int(name[6:]), 6000)
        assert o.apply_trace(o.agent("seph"), c, p) == 0
    elif name.startswith("config5_"):
        assert o.apply_remote_wire(config5_wire(int(name[8:]))) == 0
    else:
        assert o.apply_remote_wire(concurrent_wire(int(name[10:]), n_agents=5, rounds=8)[0]) == 0
    return o, o.export()


DOCS = TRACES + ["random3", "random4", "config5_1", "config5_2", "concurrent7"]


def test_kernel_consts_reads_the_sources():
    k = kernel_consts()
    assert set(k) >= {"PUB_BIG_MIN", "PUB_BIG_FEW_DOCS", "PUB_BIG_MAX", "PUBX_MAX_WORDS", "QBLK_MAX", "QBLK_CWO", "QBLK_W",
                      "QBLK_Q", "QM_TILE", "GROUP"}
    assert all(isinstance(v, int) and v > 0 for v in k.values())
    assert PUB_BIG_MIN < PUB_BIG_MAX and k["QM_TILE"] < k["QBLK_Q"] < k["QBLK_MAX"]


@pytest.mark.parametrize("L", [32, 4])
@pytest.mark.parametrize("name", DOCS)
def test_canon_and_vpos_match_the_oracle(name, L):
    o, ex = oracle_of(name, L)
    canon = R.canon_of(ex["raw"])
    assert canon.shape == ex["canon"].shape and np.array_equal(canon, ex["canon"])  # every column
    assert int(ex["leaf_sizes"].sum()) == ex["raw"].shape[0]
    # vpos_of: every position (and two past the end) through the reference's spans = the oracle's tree walk
    pos = np.arange(ex["len"] + 2, dtype=np.uint32)
    ag, sq = R.pos_to_loc_ref(ex, pos, canon)
    oa, os_ = o.pos_to_loc(pos)
    assert np.array_equal(ag, oa) and np.array_equal(sq, os_)


@pytest.mark.parametrize("L", [32, 4])
@pytest.mark.parametrize("name", DOCS)
def test_index_matches_the_oracle_loc_to_pos(name, L):
    o, ex = oracle_of(name, L)
    canon = R.canon_of(ex["raw"])
    bits, pre, srt = index = R.index_of(canon, ex["next_order"])
    assert bits.shape[0] == ex["next_order"] // 32 + 1 == pre.shape[0]
    assert int(np.unpackbits(bits.view(np.uint8)).sum()) == canon.shape[0] == srt.shape[0]
    assert (np.diff(canon[srt, 0].astype(np.int64)) > 0).all()
    seq = np.arange(ex["next_order"] + 2, dtype=np.uint32)
    seen = 0
    for a in range(o.sizes()["agents"] + 1):  # (one agent past the last: nothing found)
        pos, dl = R.loc_to_pos_ref(ex, a, seq, canon, index)
        op, od = o.loc_to_pos(np.full(seq.shape, a, np.uint16), seq)
        assert np.array_equal(dl, od), (a, int(np.flatnonzero(dl != od)[0]))
        assert np.array_equal(pos[od != 2], op[od != 2]), a
        seen += int((od != 2).sum())
    assert seen == int(np.abs(canon[:, 3].view(np.int32).astype(np.int64)).sum())  # every item, once


def big_doc(key, L):
    o = R.oracle_doc(key, L)
    ex = o.export()
    return o, ex, R.big_ranges(ex["leaf_sizes"], ex["raw"])


@pytest.mark.parametrize("L", [32, 4])
def test_big_family_reaches_every_boundary_case(L):
    cov = {}
    for seed in R.BIG_SEEDS[L]:
        o, ex, br = big_doc(("big", seed), L)
        assert PUB_BIG_MIN <= br["n_leaves"] < PUB_BIG_MAX, (seed, br["n_leaves"])
        assert np.array_equal(R.canon_of(ex["raw"]), ex["canon"])
        assert br["merge"].shape == (PUB_BIG_WAVES - 1,) and br["single"].shape == (PUB_BIG_WAVES,)
        for k, v in R.coverage(br).items():
            cov[k] = cov.get(k, 0) + int(v)
    assert set(cov) == {"merging", "non_merging", "chain_through_single", "lead_closes_inside", "skip_then_write",
                        "odd_leaf_count"}
    assert all(v >= 1 for v in cov.values()), cov


@pytest.mark.parametrize("L", [32, 4])
def test_fixed_shapes(L):
    o, ex, br = big_doc(("whole",), L)
    assert br["n_leaves"] >= PUB_BIG_MIN and ex["canon"].shape[0] == 1
    assert br["merge"].all() and br["single"].all()
    o, ex, br = big_doc(("head_tail",), L)
    assert br["n_leaves"] >= PUB_BIG_MIN and ex["canon"].shape[0] == 4
    assert br["merge"].all() and br["single"][1:-1].all() and not br["single"][0] and not br["single"][-1]
    assert np.array_equal(R.canon_of(ex["raw"]), ex["canon"])


def test_general_editing_documents_are_long():
    for key in (("random", 0), ("random", 1)):
        o, ex, br = big_doc(key, 4)
        assert PUB_BIG_MIN <= br["n_leaves"] < PUB_BIG_MAX
        assert np.array_equal(R.canon_of(ex["raw"]), ex["canon"])
    w, o = R.config5_big(0, 4)
    ex = o.export()
    assert PUB_BIG_MIN <= o.sizes()["leaves"] < PUB_BIG_MAX and o.sizes()["agents"] > 2 and o.sizes()["dd"] > 0
    assert np.array_equal(R.canon_of(ex["raw"]), ex["canon"])


def test_group_document_has_more_than_64_groups_of_leaves():
    n = R.group_prepends()
    o = R.oracle_doc(("prepends", n), 4)
    assert 64 * GROUP < o.sizes()["leaves"] < PUB_BIG_MAX and o.sizes()["canon"] == n
