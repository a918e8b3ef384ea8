"""Rebase timing beside the route a caller had without it: AP remote documents (bench.py's config 2
state), mapped from the version at half the transactions to now (the shape of
profiles/diff_bench_8192.json).
 (a) crdt_rebase_async from the diff result (crdt_last_rebase_ms: one build kernel);
 (b) crdt_rebase_dev_async for --queries-per-doc uniformly drawn old positions per document, in one
     shuffled batch;
 (c) the same positions without the map: crdt_checkout_async at `since` (crdt_last_checkout_ms),
     then crdt_pos_to_loc_at_dev_async and crdt_loc_to_pos_dev_async.
The run asserts that (b)'s answers with CRDT_BIAS_RIGHT equal (c)'s for every position on an item
that is still visible.  Device times: HIP events on the engine stream, median of --reps (the first
call of a shape also allocates its buffers inside the timed window)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-crdt-rust_amd"))
import crdt_amd  # noqa: E402
from crdt_amd.traces import load_remote_wire, load_trace  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--queries-per-doc", type=int, default=4096, help="8,192 x 4,096 = 33.5 M positions")
ap.add_argument("--out", default="")
a = ap.parse_args()

import torch  # noqa: E402

hip = C.CDLL("libamdhip64.so")
ev = [C.c_void_p() for _ in range(2)]
for x in ev:
    hip.hipEventCreate(C.byref(x))
runs = {}


def events_ms(e, fn):
    s_ = C.c_void_p(e.stream())
    hip.hipEventRecord(ev[0], s_)
    rc = fn()
    hip.hipEventRecord(ev[1], s_)
    hip.hipEventSynchronize(ev[1])
    assert rc == 0, rc
    x = C.c_float()
    hip.hipEventElapsedTime(C.byref(x), ev[0], ev[1])
    return x.value


def med(name, fn):
    ms = [fn() for _ in range(a.reps)]
    runs[name] = [round(x, 3) for x in ms]
    print(name, runs[name], file=sys.stderr, flush=True)
    return float(np.median(ms))


def diff_ms(e, docs, since):
    e.diff_async(docs, since)
    return e.diff_ms()


def rebase_ms(e):
    e.rebase_async("diff")
    return e.rebase_ms()


def checkout_ms(e, docs, since):
    e.checkout_async(docs, since)
    return e.checkout_ms()


n = a.docs
t = load_trace("automerge-paper")
e = crdt_amd.Engine(n, 32)
e.device_intern(True)
e.stage_remote_replicated(load_remote_wire("automerge-paper"), 0, ["%08x-c" % ((d * 2654435761) % (1 << 32)) for d in range(n)])
assert (e.run() == 0).all()
e.publish_async()
e.sync()
docs = np.arange(n, dtype=np.uint32)
version = int(e.versions([0])[0])
assert version == t.n_orders
# the remote form has one txn per local txn and the same orders: the version after half the txns
h = int(t.counts[: t.n_txns // 2].sum())
v_half = int(t.patches[:h, 1].sum() + t.patches[:h, 2].sum())
since = np.full(n, v_half, np.uint32)

out = {"metric": "device ms per call (AP remote documents)", "docs": n, "version": version, "since_half": v_half,
       "build_id": crdt_amd.build_id(), "text_chars_per_doc": int(e.lens([0])[0])}
out["diff_half_ms"] = med("diff_half", lambda: diff_ms(e, docs, since))
out["rebase_build_ms"] = med("rebase_build", lambda: rebase_ms(e))                      # (a)
counts = e.rebase_counts()
assert (counts == counts[0]).all()
out["spans_per_doc"] = int(counts[0])
out["checkout_half_ms"] = med("checkout_half", lambda: checkout_ms(e, docs, since))     # (c), the view
old_len = int(e.checkout_lens()[0])
out["old_chars_per_doc"] = old_len

dev = torch.device("cuda", 0)
nq = n * a.queries_per_doc
g = torch.Generator(device=dev)
g.manual_seed(5)
d_idx = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(a.queries_per_doc)
d_idx = d_idx[torch.randperm(nq, device=dev, generator=g)].contiguous()  # (docs = 0 .. n-1: an index is its document)
d_x = torch.randint(0, old_len, (nq,), dtype=torch.int32, device=dev, generator=g)
o_y = torch.zeros(nq, dtype=torch.int32, device=dev)
o_hit = torch.zeros(nq, dtype=torch.uint8, device=dev)
o_ag = torch.zeros(nq, dtype=torch.int16, device=dev)
o_sq = torch.zeros(nq, dtype=torch.int32, device=dev)
o_pos = torch.zeros(nq, dtype=torch.int32, device=dev)
o_del = torch.zeros(nq, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
L = e.L
out["positions"] = nq
out["rebase_query_ms"] = med("rebase_query", lambda: events_ms(e, lambda: L.crdt_rebase_dev_async(               # (b)
    e.h, nq, d_idx.data_ptr(), d_x.data_ptr(), 0, 0, 1, o_y.data_ptr(), o_hit.data_ptr())))
out["pos_to_loc_at_ms"] = med("pos_to_loc_at", lambda: events_ms(e, lambda: L.crdt_pos_to_loc_at_dev_async(     # (c), the queries
    e.h, nq, d_idx.data_ptr(), d_x.data_ptr(), o_ag.data_ptr(), o_sq.data_ptr())))
out["loc_to_pos_ms"] = med("loc_to_pos", lambda: events_ms(e, lambda: L.crdt_loc_to_pos_dev_async(
    e.h, nq, d_idx.data_ptr(), o_ag.data_ptr(), o_sq.data_ptr(), o_pos.data_ptr(), o_del.data_ptr())))
kept = o_del == 0
assert bool(((o_del == 0) | (o_del == 1)).all())
assert torch.equal(o_y[kept], o_pos[kept]) and not bool(o_hit[kept].any())
out["positions_on_kept_items"] = int(kept.sum())
out["rebase_query_mq_per_s"] = nq / out["rebase_query_ms"] / 1e3
out["route_without_map_ms"] = out["checkout_half_ms"] + out["pos_to_loc_at_ms"] + out["loc_to_pos_ms"]
out["route_with_map_ms"] = out["rebase_build_ms"] + out["rebase_query_ms"]
out["without_vs_with_map"] = out["route_without_map_ms"] / out["route_with_map_ms"]
out["per_query_part_without_vs_with_map"] = (out["pos_to_loc_at_ms"] + out["loc_to_pos_ms"]) / out["rebase_query_ms"]
out["per_call_ms_runs"] = runs
e.close()

print(json.dumps({k: v for k, v in out.items() if k != "per_call_ms_runs"}))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
