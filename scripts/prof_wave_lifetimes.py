"""Diagnostic: when each k_replay wave starts and ends, and where it ran (build with -DCRDT_PROF
-DCRDT_PROF_MODE=4 into build/libcrdt_gpu_prof4.so, run with CRDT_GPU_LIB pointing at it).  Every
wave records the 100 MHz real-time counter at its start and after finish(), HW_ID and XCC_ID
(kernels.h replay_doc).  One clean launch of n automerge-paper documents (fit, reset, run, as
bench.py's step) without the fused publish gives the lifetimes the fused publish has to fill; the
same launch with it on gives what each wave's publish then took; a k_publish launch of 1,025
documents (about one wave per SIMD: an unloaded machine) gives one wave's publish time alone.
The replay ends are also grouped by HW_ID.WAVE_ID, with which wave of each (w, w + 4) pair of a
SIMD ends first: the rotation's level map decides who ties with whom (CRDT_BALANCE_MAP picks it)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-crdt-rust_amd"))
import numpy as np  # noqa: E402
import crdt_amd  # noqa: E402
from crdt_amd.traces import load_remote_wire  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
P0 = 19  # DocState.prof0
TICK_US = 0.01  # 100 MHz
wire = load_remote_wire("automerge-paper")


def engine(docs, fused):
    e = crdt_amd.Engine(docs, 32)
    e.fused_publish(fused)
    e.stage_remote_replicated(wire, 0, ["u%05d" % i for i in range(docs)])
    assert (e.run() == 0).all()
    e.publish_async()
    e.fit()
    return e


def launch(e):
    e.reset_async()
    e.run_async()
    e.sync()
    s = np.array([e.debug_state(d) for d in range(e.n_docs)])[:, P0:P0 + 4]
    t0, t1, hw, x = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    base = t0.min()
    start = (t0 - base).astype(np.uint32).astype(np.float64) * TICK_US  # (u32 differences: the counter may wrap)
    end = (t1 - base).astype(np.uint32).astype(np.float64) * TICK_US
    tail = (x >> 4).astype(np.float64) * TICK_US
    return start, end, tail, hw, x & 15


def dist(v):
    q = np.percentile(v, [0, 10, 20, 30, 40, 50, 60, 70, 80, 90, 100])
    return " ".join(f"{x:9.1f}" for x in q)


def by_wave_id(start, end, hw, simd_key):
    """replay ends grouped by HW_ID.WAVE_ID & 7 (the progress balance's levels are a function of the
    wave id: kernels.h balance_board_tick), which member of each (w, w + 4) pair of a SIMD ends
    first, and whether the wave id follows the start order (the arbiter's age)"""
    wid = hw & 15
    print(f"HW_ID.WAVE_ID values seen: {dict(zip(*[a.tolist() for a in np.unique(wid, return_counts=True)]))}")
    print("replay end by WAVE_ID & 7 (us): id  waves  mean start      min       10%       50%       90%       max      mean")
    for k in range(8):
        m = (wid & 7) == k
        if not m.any():
            continue
        q = np.percentile(end[m], [0, 10, 50, 90, 100])
        print(f"    {k:2d}  {int(m.sum()):5d}  {start[m].mean():10.2f} " + " ".join(f"{x:9.1f}" for x in q) + f" {end[m].mean():9.1f}")
    order = np.lexsort((wid, simd_key))
    key, w7, en, st = simd_key[order], (wid & 7)[order], end[order], start[order]
    first = {k: [0, 0, 0.0] for k in range(4)}  # pair -> [w first, w + 4 first, sum of (end[w + 4] - end[w])]
    older = [0, 0]  # pairs of neighbouring wave ids on a SIMD: the lower id started first / later
    for lo in np.flatnonzero(np.r_[True, key[1:] != key[:-1]]):
        hi = lo + int((key[lo:] == key[lo]).sum()) if lo + 1 < key.shape[0] else lo + 1
        ids = w7[lo:hi]
        if ids.shape[0] != 8 or (np.sort(ids) != np.arange(8)).any():
            continue  # (a SIMD that did not hold ids 0..7 once each)
        e8, s8 = np.empty(8), np.empty(8)
        e8[ids], s8[ids] = en[lo:hi], st[lo:hi]
        for k in range(4):
            first[k][0 if e8[k] < e8[k + 4] else 1] += 1
            first[k][2] += e8[k + 4] - e8[k]
        for k in range(7):
            older[0 if s8[k] <= s8[k + 1] else 1] += 1
    print("pairs (w, w + 4) on SIMDs that hold wave ids 0..7 once each: pair  w ends first  w + 4 ends first  mean end[w + 4] - end[w] (us)")
    for k in range(4):
        a, b, d = first[k]
        print(f"    ({k}, {k + 4})  {a:6d}  {b:6d}  {d / max(a + b, 1):10.1f}")
    print(f"start order on those SIMDs: the lower of two neighbouring wave ids started first (or with it) in {older[0]} of {older[0] + older[1]} cases")


print(f"environment: CRDT_BALANCE_MAP={os.environ.get('CRDT_BALANCE_MAP')} CRDT_REPLAY_BALANCE={os.environ.get('CRDT_REPLAY_BALANCE')} CRDT_GPU_LIB={os.path.basename(os.environ.get('CRDT_GPU_LIB', ''))}")
e = engine(n, False)
launch(e)  # (warm)
start, end, _, hw, xcc = launch(e)
kend = end.max()
print(f"k_replay<32, SHAPE_REMOTE>, {n} automerge-paper documents, one clean launch, fused publish off; times in us from the first wave's start")
print("                   min       10%       20%       30%       40%       50%       60%       70%       80%       90%       max")
print(f"wave start   {dist(start)}")
print(f"wave end     {dist(end)}")
print(f"residency    {dist(end - start)}")
print(f"idle at end  {dist(kend - end)}   (last end - this wave's end)")
print(f"last end {kend:.1f} us; mean residency {np.mean(end - start):.1f} us = {np.mean(end - start) / kend:.1%} of the launch; "
      f"mean idle at end {np.mean(kend - end):.1f} us")
cu, simd, se, sh = (hw >> 8) & 15, (hw >> 4) & 3, (hw >> 13) & 7, (hw >> 12) & 1
slot = ((xcc.astype(np.int64) * 8 + se) * 2 + sh) * 16 + cu
per_simd = np.bincount(slot * 4 + simd)
per_simd = per_simd[per_simd > 0]
print(f"(XCC, SE, SH, CU, SIMD) slots used {per_simd.shape[0]}; waves per SIMD min {per_simd.min()} median {int(np.median(per_simd))} max {per_simd.max()}; "
      f"histogram {dict(zip(*[a.tolist() for a in np.unique(per_simd, return_counts=True)]))}")
by_wave_id(start, end, hw, slot * 4 + simd)
print("end-time spread by XCC (us): xcc  waves  first end   median end   last end")
for k in np.unique(xcc):
    m = xcc == k
    print(f"    {int(k):2d}  {int(m.sum()):5d}  {end[m].min():9.1f}  {np.median(end[m]):9.1f}  {end[m].max():9.1f}")
cus = np.unique(slot)
last = np.array([end[slot == c].max() for c in cus])
first = np.array([end[slot == c].min() for c in cus])
print(f"end-time spread by CU ({cus.shape[0]} CUs): last end of a CU  {dist(last)}")
print(f"                                   first end of a CU {dist(first)}")
print(f"                                   last - first      {dist(last - first)}")
e.close()

# one wave's publish time on an unloaded machine: k_publish (+ k_pub_index) of 1,025 documents
e1 = engine(1025, False)
pub = []
for _ in range(3):
    e1.reset_async()
    e1.run_async()
    e1.sync()
    e1.canon_counts()  # (publishes, and times the publish launches with events)
    pub.append(e1.timings()[1])
t_pub = min(pub) * 1000.0
print(f"publish of 1,025 documents (k_publish + k_pub_index, about one wave per SIMD): {t_pub:.1f} us")
e1.close()

# the same launch with the fused publish: what each wave's publish took, and the new ends
e = engine(n, True)
launch(e)
start2, end2, tail2, hw2, xcc2 = launch(e)
assert e.fused_publish_stats()[1].all()
print("fused publish on: the replay ends (before the wave's publish)")
by_wave_id(start2, end2, hw2, (((xcc2.astype(np.int64) * 8 + ((hw2 >> 13) & 7)) * 2 + ((hw2 >> 12) & 1)) * 16 + ((hw2 >> 8) & 15)) * 4 + ((hw2 >> 4) & 3))
print(f"fused publish on: wave's publish after finish() (us)  {dist(tail2)}   mean {tail2.mean():.1f}")
print(f"fused publish on: wave end incl. publish          {dist(end2 + tail2)}")
print(f"fused publish on: last end {np.max(end2 + tail2):.1f} us (off: {kend:.1f} us)")
for name, t in (("1,025-document publish", t_pub), ("mean fused publish", float(tail2.mean()))):
    ov = np.minimum(t, kend - end)
    print(f"expected overlap, one wave's publish = {name} ({t:.1f} us): mean over waves of min(publish, last end - wave end) = {ov.mean():.1f} us "
          f"({(ov >= t).mean():.1%} of the waves hide it whole)")
