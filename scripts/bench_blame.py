"""Blame timing beside its yardsticks: AP remote documents (bench.py's config 2 state), the authorship
runs in ID mode (the whole pos -> loc table, run-length encoded) and in AGENT mode (one author per
document: 1 run each, the floor of the two sweeps), next to a publish and a text materialisation of
the same engine, which sweep the same canonical spans, and next to the only route to the same
answer without crdt_blame_async: crdt_pos_to_loc_dev_async over every position of every document
(in chunks of --chunk documents; the caller would still run-length encode the answers).  One
multi-author line: config-5 histories (tests/gen) at scripts/bench_config5.py's size, --c5-docs
documents over --c5-distinct histories.  Times: HIP events on the engine stream, median of --reps
(the first blame of a shape also allocates its result array inside the timed window)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-crdt-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crdt_amd  # noqa: E402
from crdt_amd.traces import content_by_order, load_remote_wire, load_trace  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--chunk", type=int, default=512, help="documents per pos -> loc query batch")
ap.add_argument("--c5-docs", type=int, default=1024)
ap.add_argument("--c5-distinct", type=int, default=8)
ap.add_argument("--no-c5", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()

import torch  # noqa: E402

hip = C.CDLL("libamdhip64.so")
ev = [C.c_void_p() for _ in range(2)]
for x in ev:
    hip.hipEventCreate(C.byref(x))


def events_ms(e, fn):
    s_ = C.c_void_p(e.stream())
    hip.hipEventRecord(ev[0], s_)
    fn()
    hip.hipEventRecord(ev[1], s_)
    hip.hipEventSynchronize(ev[1])
    x = C.c_float()
    hip.hipEventElapsedTime(C.byref(x), ev[0], ev[1])
    return x.value


def med(name, fn):
    ms = [fn() for _ in range(a.reps)]
    print(name, [round(x, 3) for x in ms], file=sys.stderr, flush=True)
    return float(np.median(ms))


def blame_ms(e, docs, mode):
    e.blame_async(docs, mode)
    return e.blame_ms()


def materialize_ms(e):
    e.materialize_async()
    e.text_digests()  # (waits for it and reads the events: crdt_last_materialize_ms is set by the calls that wait)
    return e.materialize_ms()


def expanded(runs):
    """(agent, seq) of every position from ID-mode runs"""
    ln = runs[:, 1].astype(np.int64)
    first = np.repeat(np.cumsum(ln) - ln, ln)
    j = np.arange(int(ln.sum()), dtype=np.int64) - first
    return np.repeat(runs[:, 2], ln).astype(np.uint16), (np.repeat(runs[:, 3], ln).astype(np.int64) + j).astype(np.uint32)


n = a.docs
t = load_trace("automerge-paper")
e = crdt_amd.Engine(n, 32)
e.device_intern(True)
e.stage_remote_replicated(load_remote_wire("automerge-paper"), 0, ["%08x-c" % ((d * 2654435761) % (1 << 32)) for d in range(n)])
assert (e.run() == 0).all()
e.publish_async()
e.sync()
docs = np.arange(n, dtype=np.uint32)
e.set_content(docs, [0] * n, [content_by_order(t)])
ln = int(e.lens([0])[0])
assert (e.lens() == ln).all()

out = {"metric": "device ms per call (AP remote documents)", "docs": n, "text_chars_per_doc": ln,
       "canonical_spans_per_doc": int(e.canon_counts()[0]), "cwo_runs_per_doc": e.export_sizes(0)["cwo"],
       "build_id": crdt_amd.build_id()}
out["publish_ms"] = med("publish", lambda: events_ms(e, e.publish_async))
out["materialize_ms"] = med("materialize", lambda: materialize_ms(e))
for mode in ("id", "agent"):
    out[f"blame_{mode}_ms"] = med("blame " + mode, lambda: blame_ms(e, docs, mode))
    counts = e.blame_counts()
    assert (counts == counts[0]).all()
    first, last = e.blame_read(0), e.blame_read(n - 1)
    assert np.array_equal(first[:, [0, 1, 3]], last[:, [0, 1, 3]]) and int(first[:, 1].sum()) == ln
    out[f"blame_{mode}_runs_per_doc"] = int(counts[0])
    if mode == "id":
        id_runs = first
assert out["blame_agent_runs_per_doc"] == 1

# the query route: every position of every document through crdt_pos_to_loc_dev_async
dev = torch.device("cuda", 0)
ch = min(a.chunk, n)
assert n % ch == 0
d_doc = torch.arange(ch, dtype=torch.int32, device=dev).repeat_interleave(ln)
d_pos = torch.arange(ln, dtype=torch.int32, device=dev).repeat(ch)
o_ag = torch.zeros(ch * ln, dtype=torch.int16, device=dev)
o_sq = torch.zeros(ch * ln, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
L = e.L


def query_route_ms():
    total = 0.0
    for c0 in range(0, n, ch):
        total += events_ms(e, lambda: L.crdt_pos_to_loc_dev_async(e.h, ch * ln, d_doc.data_ptr(), d_pos.data_ptr(),
                                                                   o_ag.data_ptr(), o_sq.data_ptr()))
        d_doc.add_(ch if c0 + ch < n else ch - n)  # the next chunk's documents (untimed); back to the first at the end
        torch.cuda.synchronize()
    return total


for kern in ("lds", "merge"):
    e.query_kernel(kern)
    out[f"pos_to_loc_all_positions_{kern}_ms"] = med("pos_to_loc " + kern, query_route_ms)
    # parity: the last chunk's answers for its last document are the ID-mode runs, expanded
    ga = o_ag[-ln:].cpu().numpy().view(np.uint16)
    gs = o_sq[-ln:].cpu().numpy().view(np.uint32)
    wa, ws = expanded(id_runs)
    assert np.array_equal(gs, ws) and (ga == ga[0]).all()
e.query_kernel("lds")
out["queries_total"] = n * ln
best = min(out["pos_to_loc_all_positions_lds_ms"], out["pos_to_loc_all_positions_merge_ms"])
out["query_route_vs_blame_id"] = best / out["blame_id_ms"]
out["blame_id_vs_materialize"] = out["blame_id_ms"] / out["materialize_ms"]
out["blame_agent_vs_materialize"] = out["blame_agent_ms"] / out["materialize_ms"]
del d_doc, d_pos, o_ag, o_sq
e.close()

if not a.no_c5:
    # multi-author: config-5 histories (16 agents, deletion-heavy), as scripts/bench_config5.py builds them
    from fuzz_gen import config5_wires  # noqa: E402
    nd = a.c5_docs
    wires = config5_wires([0xC5000000 + s for s in range(a.c5_distinct)], base_len=1 << 20, n_agents=16, rounds=64, ops=64,
                          threads=min(16, os.cpu_count() or 1))
    e5 = crdt_amd.Engine(nd, 32)
    e5.share_streams(True)
    e5.apply_remote_wire(list(range(nd)), [wires[d % a.c5_distinct] for d in range(nd)], stage_only=True)
    assert (e5.run() == 0).all()
    e5.publish_async()
    e5.sync()
    d5 = np.arange(nd, dtype=np.uint32)
    c5 = {"docs": nd, "distinct_histories": a.c5_distinct, "text_chars_doc0": int(e5.lens([0])[0]),
          "canonical_spans_doc0": int(e5.canon_counts()[0]), "cwo_runs_doc0": e5.export_sizes(0)["cwo"]}
    c5["publish_ms"] = med("c5 publish", lambda: events_ms(e5, e5.publish_async))
    for mode in ("id", "agent"):
        c5[f"blame_{mode}_ms"] = med("c5 blame " + mode, lambda: blame_ms(e5, d5, mode))
        counts = e5.blame_counts()
        assert np.array_equal(e5.blame_read(0), e5.blame_read(a.c5_distinct)) or nd <= a.c5_distinct
        c5[f"blame_{mode}_runs_doc0"] = int(counts[0])
    runs = e5.blame([0], "id")[0]
    p = np.arange(c5["text_chars_doc0"], dtype=np.uint32)
    ga, gs = e5.pos_to_loc(np.zeros_like(p), p)
    wa, ws = expanded(runs)
    assert np.array_equal(ga, wa) and np.array_equal(gs, ws)
    out["config5"] = c5

print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
