"""Edits timing beside its yardsticks: AP remote documents (bench.py's config 2 state), the text
edits in units from the version at half the transactions to now and from version 0, in both
encodings (crdt_last_edits_ms: mark the deletes, width prefix, count, scan, write), next to the
diff at the same version on the same build (crdt_last_diff_ms) and to the only other route to part
of the answer: that diff followed by an encode of the same documents (crdt_last_encode_ms, which
gives unit offsets and inserted units through queries and a read of the whole text, but no deleted
units).  Times: HIP events on the engine stream, median of --reps (the first call of a shape also
allocates its result arrays inside the timed window)."""
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


def edits_ms(since, enc):
    e.edits_async(docs, np.full(n, since, np.uint32), enc)
    return e.edits_ms()


def diff_ms(since):
    e.diff_async(docs, np.full(n, since, np.uint32))
    return e.diff_ms()


def encode_ms(enc):
    e.encode_async(docs, enc)
    return e.encode_ms()


def med(fn, *args):
    ms = [fn(*args) for _ in range(a.reps)]
    print(fn.__name__, *args, [round(x, 3) for x in ms], file=sys.stderr)
    return float(np.median(ms))


out = {"metric": "device ms per call (AP remote documents)", "docs": n, "version": version, "since_half": v_half,
       "canonical_spans_per_doc": int(e.canon_counts()[0]), "text_chars_per_doc": int(e.lens([0])[0]),
       "build_id": crdt_amd.build_id()}
for enc in ("utf8", "utf16"):
    out[f"encode_{enc}_ms"] = med(encode_ms, enc)
for name, since in (("half", v_half), ("zero", 0)):
    out[f"diff_{name}_ms"] = med(diff_ms, since)
    npat, _ = e.diff_counts()
    for enc in ("utf8", "utf16"):
        ms = med(edits_ms, since, enc)
        ned, nun = e.edits_counts()
        assert (ned == npat).all() and (nun == nun[0]).all()
        first, last = e.edits_read(0), e.edits_read(n - 1)
        assert all(np.array_equal(x, y) for x, y in zip(first, last))
        k = f"edits_{name}_{enc}"
        out[k + "_ms"] = ms
        out[k + "_edits_per_doc"] = int(ned[0])
        out[k + "_ins_units_per_doc"] = int(nun[0])
        out[k + "_del_units_per_doc"] = int(first[0][:, 4].sum())
        out[k + "_vs_diff"] = ms / out[f"diff_{name}_ms"]
        out[k + "_vs_diff_plus_encode"] = ms / (out[f"diff_{name}_ms"] + out[f"encode_{enc}_ms"])
print(json.dumps(out))
