"""Two-version diff timing beside its yardsticks: AP remote documents (bench.py's config 2 state).
The patches between (half, end) next to crdt_diff_async(half) -- the existing kernel answering the
same question -- then (0, half), (half, 0) and (quarter, three quarters), where a name is the
version after that share of the transactions; next to a text materialisation and the two checkouts
a caller would diff on the host instead.  Times: HIP events on the engine stream
(crdt_last_diff_ms: mark the deletes once or twice, count, scan, write), median of --reps (the first
call of a shape also allocates its result arrays inside the timed window).

Per-kernel times come from a kernel trace of a run of its own, merged into the result file:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/bench_diff_between.py --reps 2 --out /dev/null
  python scripts/bench_diff_between.py --kernels DIR/.../kt_kernel_trace.csv --out profiles/diff_between_bench_8192.json
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
ap.add_argument("--out", default=None, help="result file (default profiles/diff_between_bench_<docs>.json)")
ap.add_argument("--kernels", default=None, help="a kernel trace (csv) of a run of this script: merge its per-kernel times into --out")
a = ap.parse_args()
path = a.out or os.path.join(ROOT, "profiles", f"diff_between_bench_{a.docs}.json")
PAIRS = ("half_end", "zero_half", "half_zero", "quarter_threequarters")


def kernel_times(trace):
    """per call of the trace, in launch order: the ms of its kernels.  A diff is k_diff_mark,
    k_diff<false>, k_result_scan<DiffRes>, k_diff<true>; a two-version diff has two marks and
    k_diff2.  Returns {"diff_half": {...}, pair: {...}} with the last repetition of each."""
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    calls, marks, cur = [], [], None
    for r in rows:
        nm = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "k_diff_mark" in nm:
            marks.append(ms)
        elif "k_diff2<false>" in nm or "k_diff2<0>" in nm:
            cur = {"kind": "between", "mark_from_ms": marks[-2], "mark_to_ms": marks[-1], "count_ms": ms}
        elif "k_diff<false>" in nm or "k_diff<0>" in nm:
            cur = {"kind": "diff", "mark_ms": marks[-1], "count_ms": ms}
        elif "k_result_scan" in nm and "DiffRes" in nm and cur is not None:
            cur["scan_ms"] = ms
        elif ("k_diff2<true>" in nm or "k_diff2<1>" in nm or "k_diff<true>" in nm or "k_diff<1>" in nm) and cur is not None:
            cur["write_ms"] = ms
            calls.append(cur)
            cur = None
    diffs = [c for c in calls if c["kind"] == "diff"]
    betw = [c for c in calls if c["kind"] == "between"]
    assert len(betw) % len(PAIRS) == 0 and betw, (len(diffs), len(betw))
    reps = len(betw) // len(PAIRS)
    out = {"diff_half": {k: round(v, 4) for k, v in diffs[reps - 1].items() if k != "kind"}}
    for j, name in enumerate(PAIRS):
        out[name] = {k: round(v, 4) for k, v in betw[j * reps + reps - 1].items() if k != "kind"}
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
runs = {}


def materialize_ms():
    e.materialize_async()
    e.text_digests()  # (waits for it and reads the events: crdt_last_materialize_ms is set by the calls that wait)
    return e.materialize_ms()


def diff_ms(since):
    e.diff_async(docs, np.full(n, since, np.uint32))
    return e.diff_ms()


def between_ms(x, y):
    e.diff_between_async(docs, np.full(n, x, np.uint32), np.full(n, y, np.uint32))
    return e.diff_ms()


def checkout_ms(v):
    e.checkout_async(docs, np.full(n, v, np.uint32))
    return e.checkout_ms()


def med(key, fn, *args):
    ms = [fn(*args) for _ in range(a.reps)]
    runs[key] = [round(x, 3) for x in ms]
    print(key, runs[key], file=sys.stderr)
    return float(np.median(ms))


out = {"metric": "device ms per call (AP remote documents)", "docs": n, "version": version, "version_quarter": v_q,
       "version_half": v_half, "version_three_quarters": v_3q, "canonical_spans_per_doc": int(e.canon_counts()[0]),
       "build_id": crdt_amd.build_id()}
out["diff_half_ms"] = med("diff_half", diff_ms, v_half)
pin = e.diff_read(0)
for name, (x, y) in zip(PAIRS, ((v_half, version), (0, v_half), (v_half, 0), (v_q, v_3q))):
    out[f"between_{name}_ms"] = med("between_" + name, between_ms, x, y)
    npat, nins = e.diff_counts()
    assert (npat == npat[0]).all() and (nins == nins[0]).all()
    first, last = e.diff_read(0), e.diff_read(n - 1)
    assert all(np.array_equal(p, q) for p, q in zip(first, last))
    if name == "half_end":  # the same question as the diff: the same answer, array for array
        assert all(np.array_equal(p, q) for p, q in zip(first, pin))
    out[f"between_{name}_patches_per_doc"] = int(npat[0])
    out[f"between_{name}_ins_per_doc"] = int(nins[0])
out["materialize_ms"] = med("materialize", materialize_ms)
for name, v in (("quarter", v_q), ("half", v_half), ("three_quarters", v_3q), ("end", version)):
    out[f"checkout_{name}_ms"] = med("checkout_" + name, checkout_ms, v)
out["text_chars_per_doc"] = int(e.lens([0])[0])
out["between_half_end_vs_diff_half"] = out["between_half_end_ms"] / out["diff_half_ms"]
out["between_half_end_vs_materialize"] = out["between_half_end_ms"] / out["materialize_ms"]
out["between_half_end_vs_two_checkouts"] = out["between_half_end_ms"] / (out["checkout_half_ms"] + out["checkout_end_ms"])
out["between_quarter_threequarters_vs_two_checkouts"] = (out["between_quarter_threequarters_ms"] /
                                                         (out["checkout_quarter_ms"] + out["checkout_three_quarters_ms"]))
out["per_call_ms_runs"] = runs
out["command"] = "python scripts/bench_diff_between.py"
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({k: v for k, v in out.items() if k != "per_call_ms_runs"}))
