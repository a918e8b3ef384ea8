"""Find timing beside its yardsticks: AP remote documents with content (bench.py's config 2
state; the content is LaTeX, ASCII).  After an encode in each encoding, crdt_find_async (count
sweep, scan, the one host read of the total, write sweep) for a 1-char pattern, a common short word
of the text, the same word with the ASCII case fold, and a 64-char pattern with no match, next to
crdt_lines_async (EOL_LF) and the encode itself on the same engine in the same run.  Find and the
line index sweep the same bytes twice; find adds the LDS window and the verification of every
candidate, and a table entry per match.  Then --queries-per-doc seeks per document in one shuffled
batch, in both directions.  Last, the only route to the matches without crdt_find_async:
crdt_encode_read to the host and a regular-expression lookahead search there, over --host-docs
documents, given per document.  Device times: HIP events on the engine stream, median of --reps
(the first find of a shape also allocates its buffers inside the timed window); the host route is
wall clock."""
import argparse
import collections
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-crdt-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crdt_amd  # noqa: E402
from crdt_amd.traces import content_by_order, load_remote_wire, load_trace, utf32_to_str  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--queries-per-doc", type=int, default=4096, help="8,192 x 4,096 = 33.5 M seeks")
ap.add_argument("--host-docs", type=int, default=32, help="documents of the crdt_encode_read + host search route")
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


def find_ms(e, pat, icase):
    e.find_async(pat, icase)
    return e.find_ms()


def host_find(hay: bytes, pat: bytes, flags=0):
    return [m.start() for m in re.finditer(b"(?=" + re.escape(pat) + b")", hay, flags)]


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
text = utf32_to_str(e.text(0))
word = collections.Counter(re.findall(r"[a-z]{3,5}", text)).most_common(1)[0][0]  # a common short word of the text
nomatch = ("find has no such text " * 4)[:64]
assert len(nomatch) == 64 and nomatch not in text
# (name, pattern, icase)
cases = [("char", "e", False), ("word", word, False), ("word_icase", word, True), ("nomatch64", nomatch, False)]

out = {"metric": "device ms per call (AP remote documents)", "docs": n, "text_chars_per_doc": ln, "build_id": crdt_amd.build_id(),
       "word": word}
for enc in ("utf16", "utf8"):  # (the UTF-8 result stays for the seeks)
    out[f"encode_{enc}_ms"] = med("encode " + enc, lambda: encode_ms(e, docs, enc))
    units, chars = e.encode_lens()
    assert (units == ln).all() and (chars == ln).all()  # (the trace is ASCII)
    out[f"lines_{enc}_lf_ms"] = med(f"lines {enc} lf", lambda: lines_ms(e, "lf"))
    for name, pat, icase in cases:
        out[f"find_{enc}_{name}_ms"] = med(f"find {enc} {name}", lambda: find_ms(e, pat, icase))
        out[f"find_{enc}_{name}_vs_lines"] = out[f"find_{enc}_{name}_ms"] / out[f"lines_{enc}_lf_ms"]
        counts = e.find_counts()
        assert (counts == counts[0]).all()
        out[f"matches_per_doc_{name}"] = int(counts[0])
        flags = re.IGNORECASE if icase else 0
        want = host_find(text.encode("ascii"), pat.encode("ascii"), flags)
        for d in (0, n - 1):  # against the host search, first and last document
            got = e.find_read(d, counts)
            assert np.array_equal(got[:, 0], want) and np.array_equal(got[:, 1], want)  # (ASCII: unit u is char u)
out["find_utf8_char_gb_per_s"] = n * ln * 2 / out["find_utf8_char_ms"] / 1e6  # (two sweeps read the units)

# seeks on the UTF-8 result of the word, both directions
e.find_async(word)
counts = e.find_counts()
mpos = e.find_read(0, counts)[:, 1].astype(np.int64)
dev = torch.device("cuda", 0)
nq = n * a.queries_per_doc
g = torch.Generator(device=dev)
g.manual_seed(5)
d_idx = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(a.queries_per_doc)
d_idx = d_idx[torch.randperm(nq, device=dev, generator=g)].contiguous()
d_val = torch.randint(0, ln, (nq,), dtype=torch.int32, device=dev, generator=g)
o_k = torch.zeros(nq, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
L = e.L
out["seeks"] = nq
d_mpos = torch.from_numpy(mpos).to(dev)
for dirname, d in (("next", 0), ("prev", 1)):
    out[f"find_seek_{dirname}_ms"] = med("find_seek " + dirname, lambda: events_ms(e, lambda: L.crdt_find_seek_dev_async(
        e.h, nq, d_idx.data_ptr(), d_val.data_ptr(), d, o_k.data_ptr())))
    k = torch.searchsorted(d_mpos, d_val.to(torch.int64), right=bool(d)) - d
    k = torch.where((k < 0) | (k >= len(mpos)), torch.full_like(k, 0xFFFFFFFF), k)
    assert torch.equal(o_k.to(torch.int64) & 0xFFFFFFFF, k)
    out[f"find_seek_{dirname}_mq_per_s"] = nq / out[f"find_seek_{dirname}_ms"] / 1e3
del d_idx, d_val, o_k

# the route without crdt_find_async: the encoded bytes to the host, searched there
k = min(a.host_docs, n)
t0 = time.perf_counter()
for d in range(k):
    hm = host_find(e.encode_read(d, (units, chars)), word.encode("ascii"))
host_s = time.perf_counter() - t0
assert len(hm) == out["matches_per_doc_word"]
out["host_route_docs"] = k
out["host_route_ms_per_doc"] = host_s * 1e3 / k
out["find_utf8_word_ms_per_doc"] = out["find_utf8_word_ms"] / n
out["host_route_vs_find_utf8_word_per_doc"] = out["host_route_ms_per_doc"] / out["find_utf8_word_ms_per_doc"]
e.close()

print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
