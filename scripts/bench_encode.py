"""Encode timing beside its yardsticks: AP remote documents with content (bench.py's config 2 state),
their text as UTF-8 and as UTF-16 (crdt_encode_async: count sweep, scan, the one host read of the
total, write sweep), next to a text materialisation and a publish of the same engine in the same
run.  k_materialize moves 20 B per canonical span plus 8 B per char; the encoder reads 4 B and writes
about 1 B per ASCII char, plus 4 B per 64 chars of index.  Then --queries-per-doc random units -> pos
and pos -> units queries per document in one batch, beside crdt_pos_to_loc_dev_async on the same
batch shape.  Last, the only route to the bytes without crdt_encode_async: crdt_text to the host and a
host transcode, over --host-docs documents, given per document.  Device times: HIP events on the
engine stream, median of --reps (the first encode of a shape also allocates its buffers inside the
timed window); the host route is wall clock."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-crdt-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crdt_amd  # noqa: E402
from crdt_amd.traces import content_by_order, fnv1a64, load_remote_wire, load_trace, utf32_to_str  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--queries-per-doc", type=int, default=4096, help="8,192 x 4,096 = 33.5 M queries")
ap.add_argument("--host-docs", type=int, default=32, help="documents of the crdt_text + host transcode route")
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


def encode_ms(e, docs, enc):
    e.encode_async(docs, enc)
    return e.encode_ms()


def materialize_ms(e):
    e.materialize_async()
    e.text_digests()  # (waits for it and reads the events: crdt_last_materialize_ms is set by the calls that wait)
    return e.materialize_ms()


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
       "canonical_spans_per_doc": int(e.canon_counts()[0]), "sample_chars": 64, "build_id": crdt_amd.build_id()}
out["publish_ms"] = med("publish", lambda: events_ms(e, e.publish_async))
out["materialize_ms"] = med("materialize", lambda: materialize_ms(e))
out["encode_utf16_ms"] = med("encode utf16", lambda: encode_ms(e, docs, "utf16"))
units, chars = e.encode_lens()
assert (units == ln).all() and (chars == ln).all()  # (the trace is ASCII)
out["encode_utf8_ms"] = med("encode utf8", lambda: encode_ms(e, docs, "utf8"))
units, chars = e.encode_lens()
assert (units == t.end_bytes).all() and (chars == ln).all()
for d in (0, n - 1):
    assert fnv1a64(e.encode_read(d, (units, chars))) == t.end_fnv  # the reference's endContent
out["units_per_doc_utf8"] = int(units[0])
out["encode_utf8_vs_materialize"] = out["encode_utf8_ms"] / out["materialize_ms"]
out["encode_utf16_vs_materialize"] = out["encode_utf16_ms"] / out["materialize_ms"]
out["encode_utf8_gb_per_s"] = n * ln * (4 * 2 + 1 + 1 / 16) / out["encode_utf8_ms"] / 1e6  # (two sweeps read the text)

# random queries on the UTF-8 result, beside pos -> loc on the same batch shape
dev = torch.device("cuda", 0)
nq = n * a.queries_per_doc
g = torch.Generator(device=dev)
g.manual_seed(5)
d_idx = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(a.queries_per_doc)
d_idx = d_idx[torch.randperm(nq, device=dev, generator=g)].contiguous()
d_val = torch.randint(0, ln, (nq,), dtype=torch.int32, device=dev, generator=g)
o_a = torch.zeros(nq, dtype=torch.int32, device=dev)
o_m = torch.zeros(nq, dtype=torch.uint8, device=dev)
o_ag = torch.zeros(nq, dtype=torch.int16, device=dev)
torch.cuda.synchronize()
L = e.L
out["queries"] = nq
out["units_to_pos_ms"] = med("units_to_pos", lambda: events_ms(e, lambda: L.crdt_units_to_pos_dev_async(
    e.h, nq, d_idx.data_ptr(), d_val.data_ptr(), o_a.data_ptr(), o_m.data_ptr())))
assert torch.equal(o_a, d_val) and not bool(o_m.any())  # (ASCII: unit u is char u)
o_a.zero_()
out["pos_to_units_ms"] = med("pos_to_units", lambda: events_ms(e, lambda: L.crdt_pos_to_units_dev_async(
    e.h, nq, d_idx.data_ptr(), d_val.data_ptr(), o_a.data_ptr())))
assert torch.equal(o_a, d_val)
out["pos_to_loc_ms"] = med("pos_to_loc", lambda: events_ms(e, lambda: L.crdt_pos_to_loc_dev_async(
    e.h, nq, d_idx.data_ptr(), d_val.data_ptr(), o_ag.data_ptr(), o_a.data_ptr())))
out["units_to_pos_mq_per_s"] = nq / out["units_to_pos_ms"] / 1e3
out["pos_to_units_mq_per_s"] = nq / out["pos_to_units_ms"] / 1e3
del d_idx, d_val, o_a, o_m, o_ag

# the route without crdt_encode_async: the UTF-32 text to the host, transcoded there
k = min(a.host_docs, n)
t0 = time.perf_counter()
for d in range(k):
    b = utf32_to_str(e.text(d)).encode()
host_s = time.perf_counter() - t0
assert fnv1a64(b) == t.end_fnv
out["host_route_docs"] = k
out["host_route_ms_per_doc"] = host_s * 1e3 / k
out["encode_utf8_ms_per_doc"] = out["encode_utf8_ms"] / n
out["host_route_vs_encode_utf8_per_doc"] = out["host_route_ms_per_doc"] / out["encode_utf8_ms_per_doc"]
e.close()

print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
