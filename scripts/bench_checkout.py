"""Checkout timing beside its yardsticks: AP remote documents (bench.py's config 2 state), every
document checked out at the version after half the transactions and at the current version
(crdt_last_checkout_ms: mark the deletes, rank, count, scan, write), next to a text materialisation
and the half-history diff of the same engine, which sweep the same canonical spans.  Times: HIP
events on the engine stream, median of --reps (the first checkout of a shape also allocates its
result arrays inside the timed window)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-crdt-rust_amd"))
import crdt_amd  # noqa: E402
from crdt_amd.traces import content_by_order, load_remote_wire, load_trace  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None, help="result file (default profiles/checkout_bench_<docs>.json)")
a = ap.parse_args()

n = a.docs
t = load_trace("automerge-paper")
e = crdt_amd.Engine(n, 32)
e.device_intern(True)
e.stage_remote_replicated(load_remote_wire("automerge-paper"), 0, ["%08x-c" % ((d * 2654435761) % (1 << 32)) for d in range(n)])
assert (e.run() == 0).all()
e.publish_async()
e.sync()
docs = np.arange(n, dtype=np.uint32)
content = content_by_order(t)
e.set_content(docs, [0] * n, [content])
version = int(e.versions([0])[0])
assert version == t.n_orders
# the remote form has one txn per local txn and the same orders: the version after half the txns
h = int(t.counts[: t.n_txns // 2].sum())
v_half = int(t.patches[:h, 1].sum() + t.patches[:h, 2].sum())
runs = {}


def materialize_ms():
    e.materialize_async()
    e.text_digests()  # (waits for it and reads the events: crdt_last_materialize_ms is set by the calls that wait)
    return e.materialize_ms()


def diff_ms(since):
    e.diff_async(docs, np.full(n, since, np.uint32))
    return e.diff_ms()


def checkout_ms(v):
    e.checkout_async(docs, np.full(n, v, np.uint32))
    return e.checkout_ms()


def med(key, fn, *args):
    ms = [fn(*args) for _ in range(a.reps)]
    runs[key] = [round(x, 3) for x in ms]
    print(key, runs[key], file=sys.stderr)
    return float(np.median(ms))


out = {"metric": "device ms per call (AP remote documents)", "docs": n, "version": version, "version_half": v_half,
       "canonical_spans_per_doc": int(e.canon_counts()[0]), "build_id": crdt_amd.build_id()}
out["materialize_ms"] = med("materialize", materialize_ms)
out["diff_half_ms"] = med("diff_half", diff_ms, v_half)
for name, v in (("half", v_half), ("now", version)):
    out[f"checkout_{name}_ms"] = med("checkout_" + name, checkout_ms, v)
    lens = e.checkout_lens()
    dg = e.checkout_digests()
    assert (lens == lens[0]).all() and (dg == dg[0]).all() and dg[0] != 0
    first, last = e.checkout_read(0), e.checkout_read(n - 1)
    assert all(np.array_equal(x, y) for x, y in zip(first, last))
    assert np.array_equal(first[1], content[first[0]])
    out[f"checkout_{name}_chars_per_doc"] = int(lens[0])
assert np.array_equal(first[1], e.text(0)) and dg[0] == e.text_digests()[0]  # at the current version: the text
out["text_chars_per_doc"] = int(e.lens([0])[0])
# bytes the write pass moves at the current version per document: the spans (16 B) and their opos
# (4 B) read, per char the content read (4 B) and order + text written (8 B)
wr = out["canonical_spans_per_doc"] * 20 + out["text_chars_per_doc"] * 12
out["checkout_now_write_bytes_per_doc"] = wr
out["checkout_now_vs_materialize"] = out["checkout_now_ms"] / out["materialize_ms"]
out["checkout_half_vs_materialize"] = out["checkout_half_ms"] / out["materialize_ms"]
out["checkout_half_vs_diff_half"] = out["checkout_half_ms"] / out["diff_half_ms"]
out["per_call_ms_runs"] = runs
out["command"] = "python scripts/bench_checkout.py"
path = a.out or os.path.join(ROOT, "profiles", f"checkout_bench_{n}.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({k: v for k, v in out.items() if k != "per_call_ms_runs"}))
