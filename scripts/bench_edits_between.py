"""Two-version edits timing beside its yardsticks: AP remote documents (bench.py's config 2 state)
with one shared content stream.  The edits between (half, end), (0, half), (half, 0) and (quarter,
three quarters), where a name is the version after that share of the transactions, in both
encodings; in the same process and for the same versions crdt_edits_async(half) -- the existing
kernels answering the same question as (half, end) -- and crdt_diff_between_async for each pair.
Times: HIP events on the engine stream (crdt_last_edits_ms: mark the deletes twice, index the
widths, count, scan, write), median of --reps (the first call of a shape also allocates its result
arrays inside the timed window).

Per-kernel times come from a kernel trace of a run of its own, merged into the result file:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/bench_edits_between.py --reps 2 --out /dev/null
  python scripts/bench_edits_between.py --kernels DIR/.../kt_kernel_trace.csv --out profiles/edits_between_bench_8192.json
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
ap.add_argument("--out", default=None, help="result file (default profiles/edits_between_bench_<docs>.json)")
ap.add_argument("--kernels", default=None, help="a kernel trace (csv) of a run of this script: merge its per-kernel times into --out")
a = ap.parse_args()
path = a.out or os.path.join(ROOT, "profiles", f"edits_between_bench_{a.docs}.json")
PAIRS = ("half_end", "zero_half", "half_zero", "quarter_threequarters")
ENCS = ("utf8", "utf16")


def kernel_times(trace):
    """per two-version edits call of the trace, in launch order: the ms of its kernels (two
    k_diff_mark, k_ed_planes, k_edits2<., false>, k_result_scan<EdRes>, k_edits2<., true>).  Returns
    {enc: {pair: {...}}} with the last repetition of each."""
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    calls, marks, cur = [], [], None
    for r in rows:
        nm = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "k_diff_mark" in nm:
            marks.append(ms)
        elif "k_ed_planes" in nm:
            cur = {"mark_from_ms": marks[-2], "mark_to_ms": marks[-1], "planes_ms": ms}
        elif "k_edits2" in nm and cur is not None and "count_ms" not in cur:
            cur["count_ms"] = ms
        elif "k_result_scan" in nm and "EdRes" in nm and cur is not None:
            cur["scan_ms"] = ms
        elif "k_edits2" in nm and cur is not None:
            cur["write_ms"] = ms
            calls.append(cur)
            cur = None
    assert calls and len(calls) % (len(PAIRS) * len(ENCS)) == 0, len(calls)
    reps = len(calls) // (len(PAIRS) * len(ENCS))
    out = {}
    for i, enc in enumerate(ENCS):
        out[enc] = {}
        for j, name in enumerate(PAIRS):
            out[enc][name] = {k: round(v, 4) for k, v in calls[(i * len(PAIRS) + j) * reps + reps - 1].items()}
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


def version_after(share):
    """the remote form has one txn per local txn and the same orders: the version after that share of the txns"""
    h = int(t.counts[: int(t.n_txns * share)].sum())
    return int(t.patches[:h, 1].sum() + t.patches[:h, 2].sum())


v_q, v_half, v_3q = version_after(0.25), version_after(0.5), version_after(0.75)
VERS = dict(zip(PAIRS, ((v_half, version), (0, v_half), (v_half, 0), (v_q, v_3q))))
runs = {}


def edits_ms(since, enc):
    e.edits_async(docs, np.full(n, since, np.uint32), enc)
    return e.edits_ms()


def edits_between_ms(x, y, enc):
    e.edits_between_async(docs, np.full(n, x, np.uint32), np.full(n, y, np.uint32), enc)
    return e.edits_ms()


def diff_between_ms(x, y):
    e.diff_between_async(docs, np.full(n, x, np.uint32), np.full(n, y, np.uint32))
    return e.diff_ms()


def med(key, fn, *args):
    ms = [fn(*args) for _ in range(a.reps)]
    runs[key] = [round(x, 3) for x in ms]
    print(key, runs[key], file=sys.stderr)
    return float(np.median(ms))


out = {"metric": "device ms per call (AP remote documents, one shared content stream)", "docs": n, "version": version,
       "version_quarter": v_q, "version_half": v_half, "version_three_quarters": v_3q,
       "canonical_spans_per_doc": int(e.canon_counts()[0]), "build_id": crdt_amd.build_id()}
for name, (x, y) in VERS.items():
    out[f"diff_between_{name}_ms"] = med("diff_between_" + name, diff_between_ms, x, y)
for enc in ENCS:
    out[f"edits_half_{enc}_ms"] = med(f"edits_half_{enc}", edits_ms, v_half, enc)
    pin = e.edits_read(0)
    for name, (x, y) in VERS.items():
        key = f"edits_between_{name}_{enc}"
        out[key + "_ms"] = med(key, edits_between_ms, x, y, enc)
        ned, nun = e.edits_counts()
        assert (ned == ned[0]).all() and (nun == nun[0]).all()
        first, last = e.edits_read(0), e.edits_read(n - 1)
        assert all(np.array_equal(p, q) for p, q in zip(first, last))
        if name == "half_end":  # the same question as the edits: the same answer, array for array
            assert all(np.array_equal(p, q) for p, q in zip(first, pin))
            out[key + "_vs_edits_half"] = out[key + "_ms"] / out[f"edits_half_{enc}_ms"]
        out[key + "_vs_diff_between"] = out[key + "_ms"] / out[f"diff_between_{name}_ms"]
        out[key + "_edits_per_doc"] = int(ned[0])
        out[key + "_ins_units_per_doc"] = int(nun[0])
out["per_call_ms_runs"] = runs
out["command"] = "python scripts/bench_edits_between.py"
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({k: v for k, v in out.items() if k != "per_call_ms_runs"}))
