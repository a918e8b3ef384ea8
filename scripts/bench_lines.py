"""Line-index timing beside its yardsticks: AP remote documents with content (bench.py's config 2
state; the content is LaTeX and has real line breaks).  After an encode in each encoding,
crdt_lines_async in both EOL modes (count sweep, scan, the one host read of the total, write
sweep), next to the encode itself and a text materialisation of the same engine in the same run.
The two line sweeps read the packed unit pool twice (1 to 2 B per ASCII char each); the encoder
reads 8 B per char of UTF-32.  Then --queries-per-doc random pos -> (line, col) queries per
document in one shuffled batch and the (line, col) -> pos queries of their answers, in both column
kinds, beside crdt_pos_to_units_dev_async / crdt_units_to_pos_dev_async on the same batch.  Last,
the only route to a line table without crdt_lines_async: crdt_encode_read to the host and a scan
for the line breaks there, over --host-docs documents, given per document.  Device times: HIP
events on the engine stream, median of --reps (the first line index of a shape also allocates its
buffers inside the timed window); the host route is wall clock."""
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
from crdt_amd.traces import content_by_order, load_remote_wire, load_trace  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--queries-per-doc", type=int, default=4096, help="8,192 x 4,096 = 33.5 M queries")
ap.add_argument("--host-docs", type=int, default=32, help="documents of the crdt_encode_read + host scan route")
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


def lines_ms(e, eol):
    e.lines_async(eol)
    return e.lines_ms()


def materialize_ms(e):
    e.materialize_async()
    e.text_digests()  # (waits for it and reads the events: crdt_last_materialize_ms is set by the calls that wait)
    return e.materialize_ms()


def host_lines(b, eol):
    """line starts in bytes of UTF-8 bytes b, on the host"""
    brk = b == 10
    if eol == "any":
        brk |= (b == 13) & np.concatenate([b[1:] != 10, [True]])
    return np.concatenate([[0], np.flatnonzero(brk) + 1])


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

out = {"metric": "device ms per call (AP remote documents)", "docs": n, "text_chars_per_doc": ln, "build_id": crdt_amd.build_id()}
out["materialize_ms"] = med("materialize", lambda: materialize_ms(e))
for enc in ("utf16", "utf8"):  # (the UTF-8 result stays for the queries)
    out[f"encode_{enc}_ms"] = med("encode " + enc, lambda: encode_ms(e, docs, enc))
    units, chars = e.encode_lens()
    assert (units == ln).all() and (chars == ln).all()  # (the trace is ASCII)
    for eol in ("lf", "any"):
        out[f"lines_{enc}_{eol}_ms"] = med(f"lines {enc} {eol}", lambda: lines_ms(e, eol))
        out[f"lines_{enc}_{eol}_vs_encode"] = out[f"lines_{enc}_{eol}_ms"] / out[f"encode_{enc}_ms"]
        counts = e.line_counts()
        assert (counts == counts[0]).all()
        out[f"lines_per_doc_{eol}"] = int(counts[0])
usz = 1
out["lines_utf8_lf_gb_per_s"] = n * ln * usz * 2 / out["lines_utf8_lf_ms"] / 1e6  # (two sweeps read the units)
# the last index (UTF-8, any) against the host scan of the encoded bytes, first and last document
for d in (0, n - 1):
    want = host_lines(np.frombuffer(e.encode_read(d, (units, chars)), np.uint8).copy(), "any")
    got = e.lines_read(d, counts)
    assert np.array_equal(got[:, 0], want) and np.array_equal(got[:, 1], want)  # (ASCII: unit u is char u)
starts = want

# random queries on the UTF-8 / any result, beside the encode's queries on the same batch
dev = torch.device("cuda", 0)
nq = n * a.queries_per_doc
g = torch.Generator(device=dev)
g.manual_seed(5)
d_idx = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(a.queries_per_doc)
d_idx = d_idx[torch.randperm(nq, device=dev, generator=g)].contiguous()
d_val = torch.randint(0, ln, (nq,), dtype=torch.int32, device=dev, generator=g)
o_l = torch.zeros(nq, dtype=torch.int32, device=dev)
o_c = torch.zeros(nq, dtype=torch.int32, device=dev)
o_p = torch.zeros(nq, dtype=torch.int32, device=dev)
o_m = torch.zeros(nq, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
L = e.L
out["queries"] = nq
d_starts = torch.from_numpy(starts.astype(np.int64)).to(dev)
want_l = torch.searchsorted(d_starts, d_val.to(torch.int64), right=True) - 1
want_c = d_val.to(torch.int64) - d_starts[want_l]
for kindname, kind in (("units", 0), ("chars", 1)):
    out[f"pos_to_linecol_{kindname}_ms"] = med("pos_to_linecol " + kindname, lambda: events_ms(e, lambda: L.crdt_pos_to_linecol_dev_async(
        e.h, nq, d_idx.data_ptr(), d_val.data_ptr(), kind, o_l.data_ptr(), o_c.data_ptr())))
    assert torch.equal(o_l.to(torch.int64), want_l) and torch.equal(o_c.to(torch.int64), want_c)
    o_p.zero_()
    out[f"linecol_to_pos_{kindname}_ms"] = med("linecol_to_pos " + kindname, lambda: events_ms(e, lambda: L.crdt_linecol_to_pos_dev_async(
        e.h, nq, d_idx.data_ptr(), o_l.data_ptr(), o_c.data_ptr(), kind, o_p.data_ptr(), o_m.data_ptr())))
    assert torch.equal(o_p, d_val) and not bool(o_m.any())
    out[f"pos_to_linecol_{kindname}_mq_per_s"] = nq / out[f"pos_to_linecol_{kindname}_ms"] / 1e3
    out[f"linecol_to_pos_{kindname}_mq_per_s"] = nq / out[f"linecol_to_pos_{kindname}_ms"] / 1e3
del want_l, want_c
o_p.zero_()
out["pos_to_units_ms"] = med("pos_to_units", lambda: events_ms(e, lambda: L.crdt_pos_to_units_dev_async(
    e.h, nq, d_idx.data_ptr(), d_val.data_ptr(), o_p.data_ptr())))
assert torch.equal(o_p, d_val)
out["units_to_pos_ms"] = med("units_to_pos", lambda: events_ms(e, lambda: L.crdt_units_to_pos_dev_async(
    e.h, nq, d_idx.data_ptr(), d_val.data_ptr(), o_p.data_ptr(), o_m.data_ptr())))
del d_idx, d_val, o_l, o_c, o_p, o_m

# the route without crdt_lines_async: the encoded bytes to the host, scanned there
k = min(a.host_docs, n)
t0 = time.perf_counter()
for d in range(k):
    b = np.frombuffer(e.encode_read(d, (units, chars)), np.uint8)
    hl = np.flatnonzero(b == 10)
host_s = time.perf_counter() - t0
assert len(hl) + 1 == out["lines_per_doc_lf"]
out["host_route_docs"] = k
out["host_route_ms_per_doc"] = host_s * 1e3 / k
out["lines_utf8_lf_ms_per_doc"] = out["lines_utf8_lf_ms"] / n
out["host_route_vs_lines_utf8_lf_per_doc"] = out["host_route_ms_per_doc"] / out["lines_utf8_lf_ms_per_doc"]
e.close()

print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
