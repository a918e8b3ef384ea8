"""Diff timing beside its yardsticks: AP remote documents (bench.py's config 2 state), the patches
from the version at half the transactions to now and from version 0 (crdt_last_diff_ms: mark the
deletes, count, scan, write), next to a publish and a text materialisation of the same engine,
which sweep the same canonical spans.  Times: HIP events on the engine stream, median of --reps
(the first diff of a shape also allocates its result arrays inside the timed window)."""
import argparse
import ctypes as C
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
e.set_content(docs, [0] * n, [content_by_order(t)])
version = int(e.versions([0])[0])
assert version == t.n_orders
# the remote form has one txn per local txn and the same orders: the version after half the txns
h = int(t.counts[: t.n_txns // 2].sum())
v_half = int(t.patches[:h, 1].sum() + t.patches[:h, 2].sum())

hip = C.CDLL("libamdhip64.so")
ev = [C.c_void_p() for _ in range(2)]
for x in ev:
    hip.hipEventCreate(C.byref(x))
s_ = C.c_void_p(e.stream())


def publish_ms():
    hip.hipEventRecord(ev[0], s_)
    e.publish_async()
    hip.hipEventRecord(ev[1], s_)
    hip.hipEventSynchronize(ev[1])
    x = C.c_float()
    hip.hipEventElapsedTime(C.byref(x), ev[0], ev[1])
    return x.value


def materialize_ms():
    e.materialize_async()
    e.text_digests()  # (waits for it and reads the events: crdt_last_materialize_ms is set by the calls that wait)
    return e.materialize_ms()


def diff_ms(since):
    e.diff_async(docs, np.full(n, since, np.uint32))
    return e.diff_ms()


def med(fn, *args):
    ms = [fn(*args) for _ in range(a.reps)]
    print(fn.__name__, *args, [round(x, 3) for x in ms], file=sys.stderr)
    return float(np.median(ms))


out = {"metric": "device ms per call (AP remote documents)", "docs": n, "version": version, "since_half": v_half,
       "canonical_spans_per_doc": int(e.canon_counts()[0]), "build_id": crdt_amd.build_id()}
out["publish_ms"] = med(publish_ms)
out["materialize_ms"] = med(materialize_ms)
for name, since in (("half", v_half), ("zero", 0)):
    out[f"diff_{name}_ms"] = med(diff_ms, since)
    npat, nins = e.diff_counts()
    assert (npat == npat[0]).all() and (nins == nins[0]).all()
    first, last = e.diff_read(0), e.diff_read(n - 1)
    assert all(np.array_equal(x, y) for x, y in zip(first, last))
    out[f"diff_{name}_patches_per_doc"] = int(npat[0])
    out[f"diff_{name}_ins_per_doc"] = int(nins[0])
out["text_chars_per_doc"] = int(e.lens([0])[0])
out["diff_half_vs_materialize"] = out["diff_half_ms"] / out["materialize_ms"]
print(json.dumps(out))
