"""Causal-version diff timing beside its yardstick: AP remote documents (bench.py's config 2 state).
crdt_diff_vv_async from the vector of half the history to the vector of now, next to
crdt_diff_between_async on the same documents and the same two versions as order prefixes (half,
end) in the same run; the two must give the same result, array for array.  Times: HIP events on
the engine stream (crdt_last_diff_ms: mark twice, count, scan, write), median of --reps (the first
call of a shape also allocates its result arrays inside the timed window).  --lds-words 0 times the
path that builds the bitmaps with atomics in device memory.

Per-kernel times come from a kernel trace of a run of its own, merged into the result file:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/bench_diff_vv.py --reps 2 --out /dev/null
  python scripts/bench_diff_vv.py --kernels DIR/.../kt_kernel_trace.csv --out profiles/diff_vv_bench_8192.json
(the second command runs nothing on the device)."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-crdt-rust_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--lds-words", type=int, default=None, help="crdt_test_set_vv_lds_words before the vv calls")
ap.add_argument("--out", default=None, help="result file (default profiles/diff_vv_bench_<docs>.json)")
ap.add_argument("--kernels", default=None, help="a kernel trace (csv) of a run of this script: merge its per-kernel times into --out")
a = ap.parse_args()
path = a.out or os.path.join(ROOT, "profiles", f"diff_vv_bench_{a.docs}.json")


def kernel_times(trace):
    """the ms of the kernels of the last crdt_diff_vv_async and the last crdt_diff_between_async of the trace"""
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    out, marks, cur = {}, [], None
    for r in rows:
        nm = r["Kernel_Name"]
        ms = round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6, 4)
        if "k_vv_mark" in nm or "k_diff_mark" in nm:
            marks.append(ms)
        elif "k_diff2_sets<false>" in nm or "k_diff2_sets<0>" in nm:
            cur = ("vv", {"mark_from_ms": marks[-2], "mark_to_ms": marks[-1], "count_ms": ms})
        elif "k_diff2<false>" in nm or "k_diff2<0>" in nm:
            cur = ("between", {"mark_from_ms": marks[-2], "mark_to_ms": marks[-1], "count_ms": ms})
        elif "k_result_scan" in nm and "DiffRes" in nm and cur is not None:
            cur[1]["scan_ms"] = ms
        elif ("k_diff2_sets<true>" in nm or "k_diff2_sets<1>" in nm or "k_diff2<true>" in nm or "k_diff2<1>" in nm) and cur is not None:
            cur[1]["write_ms"] = ms
            out[cur[0]] = cur[1]
            cur = None
    return out


if a.kernels:
    with open(path) as f:
        out = json.load(f)
    out["kernel_ms"] = kernel_times(a.kernels)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["kernel_ms"]))
    sys.exit(0)

import crdt_amd  # noqa: E402
from crdt_amd.traces import content_by_order, load_remote_wire, load_trace  # noqa: E402

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
h = int(t.counts[: t.n_txns // 2].sum())
v_half = int(t.patches[:h, 1].sum() + t.patches[:h, 2].sum())  # the version after half the txns
vv_half, vv_end = e.version_vector([0, 0], [v_half, version])  # (the copies are one document)
runs = {}


def between_ms():
    e.diff_between_async(docs, np.full(n, v_half, np.uint32), np.full(n, version, np.uint32))
    return e.diff_ms()


def vv_ms():
    e.diff_vv_async(docs, [vv_half] * n, [vv_end] * n)
    return e.diff_ms()


def med(key, fn):
    ms = [fn() for _ in range(a.reps)]
    runs[key] = [round(x, 3) for x in ms]
    print(key, runs[key], file=sys.stderr)
    return float(np.median(ms))


out = {"metric": "device ms per call (AP remote documents)", "docs": n, "version": version, "version_half": v_half,
       "vector_half": vv_half.tolist(), "vector_end": vv_end.tolist(), "canonical_spans_per_doc": int(e.canon_counts()[0]),
       "build_id": crdt_amd.build_id(), "lds_words": a.lds_words}
out["between_half_end_ms"] = med("between_half_end", between_ms)
pin = [e.diff_read(0), e.diff_read(n - 1)]
if a.lds_words is not None:
    crdt_amd.lib().crdt_test_set_vv_lds_words(a.lds_words)
out["vv_half_end_ms"] = med("vv_half_end", vv_ms)
npat, nins = e.diff_counts()
assert (npat == npat[0]).all() and (nins == nins[0]).all()
for got, want in zip([e.diff_read(0), e.diff_read(n - 1)], pin):  # the same question: the same answer, array for array
    assert all(np.array_equal(p, q) for p, q in zip(got, want))
cf, ct = e.diff_vv_closed()
assert cf.all() and ct.all()
out["patches_per_doc"] = int(npat[0])
out["ins_per_doc"] = int(nins[0])
out["vv_vs_between"] = out["vv_half_end_ms"] / out["between_half_end_ms"]
out["per_call_ms_runs"] = runs
out["command"] = "python scripts/bench_diff_vv.py" + ("" if a.lds_words is None else f" --lds-words {a.lds_words}")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({k: v for k, v in out.items() if k != "per_call_ms_runs"}))
