"""crdt_amd — Python binding of the MI355X list-CRDT engine (include/crdt_gpu.h).

The product is the C ABI library text-crdt-rust_amd/build/libcrdt_gpu.so (HIP kernels for gfx950 +
C++ host).  This module is a thin ctypes layer used by tests and bench.py; it mirrors the
reference's `ListCRDT` surface (src/list/doc.rs) for one document (`ListCRDT`) and exposes the
batched many-document form (`Engine`).  There is no CPU fallback: without the built library or a
gfx950 device every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Iterable, Sequence

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(PKG_DIR)
REPO = os.path.dirname(PKG_ROOT)
LIB_PATH = os.path.join(PKG_ROOT, "build", "libcrdt_gpu.so")
CSRC = os.path.join(PKG_ROOT, "csrc")
INCLUDE = os.path.join(REPO, "include")

OK = 0
STATUS_NAMES = {0: "OK", -1: "POS_OOB", -2: "SEQ", -3: "UNKNOWN_AGENT", -4: "UNKNOWN_ID", -5: "NONTERMINATING",
                -6: "CAPACITY", -7: "EMPTY_TXN", -8: "FRONTIER", -9: "BAD_INPUT", -10: "INTERNAL"}
ROOT_AGENT = 0xFFFF
ROOT_ORDER = 0xFFFFFFFF


BALANCE_MAPS = 3  # level maps of the replay's rotation policy (csrc/balance_levels.h BALANCE_MAPS)


class CrdtError(RuntimeError):
    pass


def _build_cmd(out: str, defines: Sequence[str]) -> list:
    # Codegen options for the replay's wave-uniform control flow (measured on k_replay, 8,192 AP
    # documents, scripts/gpu_ab.sh):
    #  -phi-elim-split-all-critical-edges: the fast paths have many early exits into one shared
    #   "not applicable" block; without edge splitting the register copies that block's phis need
    #   are placed before every conditional branch and run whether it is taken or not (118 -> 110 ms);
    #  -structurizecfg-skip-uniform-regions: uniform branches stay plain s_cbranch_scc jumps instead
    #   of being structurized into exec-mask flow blocks with 64-bit boolean phis (109 -> 99 ms).
    return ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
            "-fno-strict-aliasing", "-mllvm", "-phi-elim-split-all-critical-edges=1",
            "-mllvm", "-structurizecfg-skip-uniform-regions=1", "-I" + INCLUDE, "-I" + CSRC, "-o", out + ".tmp"] + [
            "-D" + d for d in defines] + [os.path.join(CSRC, "engine.hip"), os.path.join(CSRC, "trace_ingest.cpp"), "-lz"]


def source_hash(defines: Sequence[str] = ()) -> str:
    """sha256 (16 hex digits) over every source the library is built from (csrc/*, the public
    headers) and the build line: what build() keys a rebuild on, embedded in the library
    (crdt_build_id) and printed by __graft_entry__.smoke()."""
    import hashlib
    h = hashlib.sha256()
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)) + [os.path.join(INCLUDE, x) for x in ("crdt_gpu.h", "crdt_trace.h")]
    for p in srcs:
        h.update(os.path.relpath(p, REPO).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    h.update(" ".join(_build_cmd("OUT", defines)[1:]).replace(REPO, "").encode())
    return h.hexdigest()[:16]


def build(force: bool = False, verbose: bool = False, out: str = LIB_PATH, defines: Sequence[str] = ()) -> str:
    """Compile libcrdt_gpu.so for gfx950 with hipcc (in-tree).  The rebuild is keyed on
    source_hash() (sources + build line), stored beside the library (`out` + ".srchash") and
    embedded in it (crdt_build_id), not on file times.  `defines` only for diagnostic builds
    written to another `out` (e.g. CRDT_PROF)."""
    hsh = source_hash(defines)
    stamp = out + ".srchash"
    if not force and os.path.exists(out) and os.path.exists(stamp):
        with open(stamp) as f:
            if f.read().strip() == hsh:
                return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = _build_cmd(out, list(defines) + [f'CRDT_SRC_HASH="{hsh}"'])
    r = subprocess.run(cmd, capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise CrdtError("hipcc failed:\n" + (r.stderr or "")[-4000:])
    if not defines:  # (diagnostic builds, e.g. CRDT_PROF, may spill: they are never the product)
        check_codegen(out + ".tmp")
    os.replace(out + ".tmp", out)
    with open(stamp, "w") as f:
        f.write(hsh + "\n")
    return out


def build_id(path: str = None) -> str:
    """crdt_build_id() of the library `path` (default: the one lib() loads)."""
    L = lib() if path is None else C.CDLL(path)
    L.crdt_build_id.restype = C.c_char_p
    return L.crdt_build_id().decode()


# The replay's speed rests on its register budget: 8 waves per SIMD need <= 64 VGPRs (the 512-
# VGPR file / 8), and a scratch spill of a value the replay loop updates would put memory round
# trips into every context access.  A toolchain change that breaks either would silently halve
# throughput (97 VGPRs = 4 waves/SIMD = 216 ms vs 185 ms), so build() refuses such
# a library.  k_replay may keep ONE 16-byte spill slot with at most 4 stores in the whole kernel:
# at 64 VGPRs the allocator spills a register quad holding the constant half {32, 0} of the
# double-delete block record that dd_insert's block split writes (stored at kernel entry and in
# the three inlined copies of that split, once per 32 double-delete entries; reloaded on the same
# rare paths).  Same-box A/B: no cost.  A spill of a value the replay loop updates
# would show up as more scratch stores.
SCRATCH_STORES_MAX = {"k_replay": 4, "k_replay_dec": 0}
CODEGEN_LIMITS = {
    "k_replay": {"vgpr_count": 64, "vgpr_spill_count": 16, "private_segment_fixed_size": 32},
    # the remote-only instance with the window decode (kernels.h k_replay_dec): the same budget, no spill
    "k_replay_dec": {"vgpr_count": 64, "vgpr_spill_count": 0, "private_segment_fixed_size": 0},
    # the two-level-root instance (documents past the LDS root) runs at 4 waves per SIMD
    "k_replay_hr": {"vgpr_count": 128, "vgpr_spill_count": 0, "private_segment_fixed_size": 0},
    "k_publish": {"vgpr_count": 64, "vgpr_spill_count": 0, "private_segment_fixed_size": 0},
}
LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def kernel_resources(lib_path: str) -> dict:
    """Per-kernel resource metadata of the gfx950 code object inside `lib_path` (the AMDGPU
    metadata note: .vgpr_count, .sgpr_count, spills, .private_segment_fixed_size, LDS)."""
    import re
    import tempfile
    import shutil
    with tempfile.TemporaryDirectory() as td:
        # the HIP fat binary sits in the library's .hip_fatbin section; llvm-objdump --offloading
        # extracts its bundles next to the (copied) input
        cp = os.path.join(td, "lib.so")
        shutil.copyfile(lib_path, cp)
        r = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "--offloading", cp], capture_output=True, text=True)
        cos = [f for f in os.listdir(td) if "amdgcn-amd-amdhsa--gfx950" in f]
        if r.returncode != 0 or not cos:
            raise CrdtError("no gfx950 code object in " + lib_path + ": " + (r.stderr or "")[-500:])
        notes = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(td, cos[0])],
                               capture_output=True, text=True, check=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if line.lstrip().startswith("- "):
            cur = {}
        if k == "name":
            out[v] = cur
        elif re.fullmatch(r"-?\d+", v):
            cur[k] = int(v)
    return out


def scratch_stores(lib_path: str) -> dict:
    """Scratch store instructions per kernel of the gfx950 code object inside `lib_path`."""
    import re
    import tempfile
    import shutil
    with tempfile.TemporaryDirectory() as td:
        cp = os.path.join(td, "lib.so")
        shutil.copyfile(lib_path, cp)
        subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "--offloading", cp], capture_output=True, text=True)
        cos = [f for f in os.listdir(td) if "amdgcn-amd-amdhsa--gfx950" in f]
        if not cos:
            raise CrdtError("no gfx950 code object in " + lib_path)
        dis = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", "--no-show-raw-insn", os.path.join(td, cos[0])],
                             capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = 0
        elif cur and ("scratch_store" in line or "buffer_store" in line and "off, s[0:3]" in line):
            out[cur] += 1
    return out


def check_codegen(lib_path: str) -> dict:
    """Raise CrdtError if a guarded kernel exceeds CODEGEN_LIMITS (or SCRATCH_STORES_MAX); returns
    the guarded kernels' resources."""
    res = kernel_resources(lib_path)
    ss = scratch_stores(lib_path)
    for name, n in ss.items():
        for k, mx in SCRATCH_STORES_MAX.items():
            if f"{len(k)}{k}I" in name and n > mx:
                raise CrdtError(f"codegen guard: {name} has {n} scratch stores > {mx} (a spill inside the replay loop; "
                                f"see DESIGN.md §4)")
    seen = {}
    for name, r in res.items():
        for k, lim in CODEGEN_LIMITS.items():
            if f"{len(k)}{k}I" not in name:  # mangled template name, e.g. _ZN4crdt8k_replayILi32EE...
                continue
            seen[name] = r
            for field, mx in lim.items():
                if r.get(field, 0) > mx:
                    raise CrdtError(f"codegen guard: {name} {field} = {r.get(field)} > {mx} "
                                    f"(the replay's 8-waves/SIMD register budget; see DESIGN.md §4)")
    for k in CODEGEN_LIMITS:
        if not any(f"{len(k)}{k}I" in n for n in seen):
            raise CrdtError(f"codegen guard: kernel {k} not found in {lib_path}")
    return seen


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("CRDT_GPU_LIB", LIB_PATH)  # diagnostic builds only (e.g. -DCRDT_PROF)
    if not os.path.exists(path):
        raise CrdtError(f"{path} not built (run __graft_entry__.build())")
    L = C.CDLL(path)
    if path != LIB_PATH:  # a diagnostic library from an older tree may lack later entry points
        class _Missing:
            def __init__(self, name):
                self.name = name

            def __call__(self, *a):
                raise CrdtError(f"{self.name}: not in {path}")
        for name in EXPORTED_SYMBOLS:
            if not hasattr(L, name):
                setattr(L, name, _Missing(name))
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
    P = C.POINTER

    class Cfg(C.Structure):
        _fields_ = [("leaf_cap", C.c_uint32), ("device", C.c_int32)]
    L.Cfg = Cfg
    L.crdt_engine_create.argtypes = [P(Cfg), P(vp)]
    L.crdt_engine_destroy.argtypes = [vp]
    L.crdt_docs_alloc.argtypes = [vp, u64]
    L.crdt_num_docs.argtypes = [vp]
    L.crdt_num_docs.restype = u64
    L.crdt_agent_intern.argtypes = [vp, u64, P(u32), P(C.c_char_p), P(C.c_uint16)]
    L.crdt_agent_intern_dev.argtypes = [vp, u64, P(u32), P(u64), C.c_char_p, P(C.c_uint16), P(u32)]
    L.crdt_apply_local.argtypes = [vp, u64, P(u32), P(u64), vp, vp, P(i32)]
    L.crdt_stage_local.argtypes = [vp, u64, P(u32), P(u64), vp, vp]
    L.crdt_apply_remote_wire.argtypes = [vp, u64, P(u32), P(C.c_char_p), P(u64), P(i32)]
    L.crdt_stage_remote_wire.argtypes = [vp, u64, P(u32), P(C.c_char_p), P(u64)]
    L.crdt_stage_remote_replicated.argtypes = [vp, C.c_char_p, u64, u32, P(C.c_char_p)]
    L.crdt_stage_random.argtypes = [vp, u64, P(u32), C.c_char_p, u32, u64]
    L.crdt_stage_local_shared.argtypes = [vp, u64, P(u32), P(u32), u32, P(u64), vp, vp]
    L.crdt_debug_state.argtypes = [vp, u32, P(u32)]
    L.crdt_fit.argtypes = [vp]
    # (round-5 entry points; a diagnostic library from before them (CRDT_GPU_LIB) loads without them)
    for f, at in (("crdt_fit_note", [vp, C.c_int]), ("crdt_test_fail_alloc_after", [C.c_longlong]),
                  ("crdt_reseed_random_async", [vp, u64, u64]), ("crdt_digest_dev_async", [vp, vp])):
        if hasattr(L, f):
            getattr(L, f).argtypes = at
    L.crdt_set_share_streams.argtypes = [vp, C.c_int]
    for f in ("crdt_set_device_intern", "crdt_set_query_kernel", "crdt_set_fused_publish"):
        if hasattr(L, f):  # (older libraries, for A/B runs, lack them)
            getattr(L, f).argtypes = [vp, C.c_int]
    if hasattr(L, "crdt_fused_publish_stats"):
        L.crdt_fused_publish_stats.argtypes = [vp, P(u64), P(C.c_uint8)]
        L.crdt_debug_vpos.argtypes = [vp, u32, P(u32)]
    if hasattr(L, "crdt_debug_publish_plan"):
        L.crdt_debug_publish_plan.argtypes = [vp, P(C.c_uint8), P(u32)]
    if hasattr(L, "crdt_set_replay_balance"):
        L.crdt_set_replay_balance.argtypes = [vp, C.c_int]
        L.crdt_debug_balance_board.argtypes = [vp, P(u32), P(u32), P(C.c_int)]
    if hasattr(L, "crdt_set_window_decode"):
        L.crdt_set_window_decode.argtypes = [vp, C.c_int]
    if hasattr(L, "crdt_set_balance_map"):
        L.crdt_set_balance_map.argtypes = [vp, C.c_int]
    L.crdt_apply_local_probed.argtypes = [vp, u64, P(u32), P(u64), vp, vp, vp, vp, P(i32)]
    L.crdt_mem_bytes.argtypes = [vp]
    L.crdt_mem_bytes.restype = u64
    if hasattr(L, "crdt_device_bytes"):  # (older libraries, for A/B runs, lack it)
        L.crdt_device_bytes.argtypes = [P(u64), P(u64), C.c_int]
    L.crdt_reset_async.argtypes = [vp]
    L.crdt_run.argtypes = [vp, P(i32)]
    L.crdt_run_async.argtypes = [vp]
    L.crdt_publish_async.argtypes = [vp]
    L.crdt_sync.argtypes = [vp]
    L.crdt_pos_to_loc.argtypes = [vp, u64, P(u32), P(u32), P(C.c_uint16), P(u32)]
    L.crdt_loc_to_pos.argtypes = [vp, u64, P(u32), P(C.c_uint16), P(u32), P(u32), P(C.c_uint8)]
    L.crdt_pos_to_loc_dev_async.argtypes = [vp, u64, vp, vp, vp, vp]
    L.crdt_loc_to_pos_dev_async.argtypes = [vp, u64, vp, vp, vp, vp, vp]
    L.crdt_doc_len.argtypes = [vp, u64, P(u32), P(u32)]
    L.crdt_doc_status.argtypes = [vp, P(i32)]
    L.crdt_digest.argtypes = [vp, P(u64)]
    if hasattr(L, "crdt_canon_counts"):  # (older libraries, for A/B runs, lack it)
        L.crdt_canon_counts.argtypes = [vp, P(u32)]
    L.crdt_export_sizes.argtypes = [vp, u32, P(u64)]
    L.crdt_export.argtypes = [vp, u32] + [P(u32)] * 9
    L.crdt_last_timings.argtypes = [vp, P(C.c_double), P(C.c_double)]
    L.crdt_stream.argtypes = [vp]
    L.crdt_stream.restype = vp
    L.crdt_set_content.argtypes = [vp, u64, P(u32), P(u32), u32, P(u64), P(u32)]
    L.crdt_materialize_async.argtypes = [vp]
    L.crdt_set_content_copies.argtypes = [vp, u64, P(u32), P(u32), u64]
    L.crdt_text.argtypes = [vp, u32, P(u32), u64, P(u64)]
    L.crdt_text_digest.argtypes = [vp, P(u64)]
    L.crdt_last_materialize_ms.argtypes = [vp, P(C.c_double)]
    L.crdt_doc_version.argtypes = [vp, u64, P(u32), P(u32)]
    L.crdt_diff_async.argtypes = [vp, u64, P(u32), P(u32)]
    L.crdt_diff_between_async.argtypes = [vp, u64, P(u32), P(u32), P(u32)]
    L.crdt_version_vector.argtypes = [vp, u64, P(u32), P(u32), P(u64), P(u32)]
    L.crdt_version_vector_dev_async.argtypes = [vp, u64, vp, vp, vp, vp]
    L.crdt_diff_vv_async.argtypes = [vp, u64, P(u32), P(u64), P(u32), P(u32)]
    L.crdt_diff_vv_closed.argtypes = [vp, P(C.c_uint8), P(C.c_uint8)]
    L.crdt_test_set_vv_lds_words.argtypes = [u32]
    L.crdt_diff_counts.argtypes = [vp, P(u32), P(u32)]
    L.crdt_diff_read.argtypes = [vp, u64, vp, P(u32), P(u32)]
    L.crdt_last_diff_ms.argtypes = [vp, P(C.c_double)]
    L.crdt_checkout_async.argtypes = [vp, u64, P(u32), P(u32)]
    L.crdt_checkout_lens.argtypes = [vp, P(u32)]
    L.crdt_checkout_read.argtypes = [vp, u64, P(u32), P(u32)]
    L.crdt_checkout_digest.argtypes = [vp, P(u64)]
    L.crdt_pos_to_loc_at.argtypes = [vp, u64, P(u32), P(u32), P(C.c_uint16), P(u32)]
    L.crdt_loc_to_pos_at.argtypes = [vp, u64, P(u32), P(C.c_uint16), P(u32), P(u32), P(C.c_uint8)]
    L.crdt_pos_to_loc_at_dev_async.argtypes = [vp, u64, vp, vp, vp, vp]
    L.crdt_loc_to_pos_at_dev_async.argtypes = [vp, u64, vp, vp, vp, vp, vp]
    L.crdt_last_checkout_ms.argtypes = [vp, P(C.c_double)]
    L.crdt_blame_async.argtypes = [vp, u64, P(u32), C.c_int]
    L.crdt_blame_counts.argtypes = [vp, P(u32)]
    L.crdt_blame_read.argtypes = [vp, u64, vp]
    L.crdt_last_blame_ms.argtypes = [vp, P(C.c_double)]
    L.crdt_encode_async.argtypes = [vp, u64, P(u32), C.c_int]
    L.crdt_encode_lens.argtypes = [vp, P(u32), P(u32)]
    L.crdt_encode_read.argtypes = [vp, u64, vp, u64]
    L.crdt_pos_to_units.argtypes = [vp, u64, P(u32), P(u32), P(u32)]
    L.crdt_units_to_pos.argtypes = [vp, u64, P(u32), P(u32), P(u32), P(C.c_uint8)]
    L.crdt_pos_to_units_dev_async.argtypes = [vp, u64, vp, vp, vp]
    L.crdt_units_to_pos_dev_async.argtypes = [vp, u64, vp, vp, vp, vp]
    L.crdt_last_encode_ms.argtypes = [vp, P(C.c_double)]
    L.crdt_lines_async.argtypes = [vp, C.c_int]
    L.crdt_line_counts.argtypes = [vp, P(u32)]
    L.crdt_lines_read.argtypes = [vp, u64, vp]
    L.crdt_pos_to_linecol.argtypes = [vp, u64, P(u32), P(u32), C.c_int, P(u32), P(u32)]
    L.crdt_linecol_to_pos.argtypes = [vp, u64, P(u32), P(u32), P(u32), C.c_int, P(u32), P(C.c_uint8)]
    L.crdt_pos_to_linecol_dev_async.argtypes = [vp, u64, vp, vp, C.c_int, vp, vp]
    L.crdt_linecol_to_pos_dev_async.argtypes = [vp, u64, vp, vp, vp, C.c_int, vp, vp]
    L.crdt_last_lines_ms.argtypes = [vp, P(C.c_double)]
    L.crdt_find_async.argtypes = [vp, P(u32), u32, C.c_int]
    L.crdt_find_counts.argtypes = [vp, P(u32)]
    L.crdt_find_read.argtypes = [vp, u64, vp]
    L.crdt_find_seek.argtypes = [vp, u64, P(u32), P(u32), C.c_int, P(u32)]
    L.crdt_find_seek_dev_async.argtypes = [vp, u64, vp, vp, C.c_int, vp]
    L.crdt_last_find_ms.argtypes = [vp, P(C.c_double)]
    L.crdt_edits_async.argtypes = [vp, u64, P(u32), P(u32), C.c_int]
    L.crdt_edits_between_async.argtypes = [vp, u64, P(u32), P(u32), P(u32), C.c_int]
    L.crdt_edits_counts.argtypes = [vp, P(u32), P(u32)]
    L.crdt_edits_read.argtypes = [vp, u64, vp, vp]
    L.crdt_last_edits_ms.argtypes = [vp, P(C.c_double)]
    L.crdt_rebase_async.argtypes = [vp, C.c_int]
    L.crdt_rebase_counts.argtypes = [vp, P(u32)]
    L.crdt_rebase_read.argtypes = [vp, u64, C.c_int, vp]
    L.crdt_rebase.argtypes = [vp, u64, P(u32), P(u32), C.c_int, C.c_int, C.c_int, P(u32), P(C.c_uint8)]
    L.crdt_rebase_dev_async.argtypes = [vp, u64, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.crdt_last_rebase_ms.argtypes = [vp, P(C.c_double)]
    L.crdt_last_error.restype = C.c_char_p
    L.crdt_trace_load.argtypes = [C.c_char_p, P(vp)]
    L.crdt_trace_parse.argtypes = [C.c_char_p, u64, P(vp)]
    L.crdt_trace_sizes.argtypes = [vp, P(u64)]
    L.crdt_trace_copy.argtypes = [vp, vp, vp, C.c_char_p, C.c_char_p, C.c_char_p]
    L.crdt_trace_free.argtypes = [vp]
    L.crdt_trace_free.restype = None
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "crdt_engine_create", "crdt_engine_destroy", "crdt_docs_alloc", "crdt_num_docs", "crdt_agent_intern", "crdt_agent_intern_dev",
    "crdt_apply_local", "crdt_apply_remote_wire", "crdt_stage_local", "crdt_stage_remote_wire",
    "crdt_stage_remote_replicated", "crdt_reset_async", "crdt_run", "crdt_run_async", "crdt_publish_async",
    "crdt_sync", "crdt_pos_to_loc", "crdt_loc_to_pos", "crdt_pos_to_loc_dev_async", "crdt_loc_to_pos_dev_async",
    "crdt_doc_len", "crdt_doc_status", "crdt_digest", "crdt_export_sizes", "crdt_export", "crdt_last_timings",
    "crdt_stream", "crdt_last_error", "crdt_build_id", "crdt_stage_random", "crdt_debug_state",
    "crdt_stage_local_shared", "crdt_set_content", "crdt_materialize_async", "crdt_text", "crdt_text_digest",
    "crdt_last_materialize_ms", "crdt_set_content_copies", "crdt_canon_counts", "crdt_fit", "crdt_mem_bytes", "crdt_apply_local_probed", "crdt_set_share_streams", "crdt_set_device_intern", "crdt_set_query_kernel", "crdt_device_bytes",
    "crdt_fit_note", "crdt_reseed_random_async", "crdt_digest_dev_async", "crdt_test_fail_alloc_after",
    "crdt_doc_version", "crdt_diff_async", "crdt_diff_between_async", "crdt_diff_counts", "crdt_diff_read", "crdt_last_diff_ms",
    "crdt_version_vector", "crdt_version_vector_dev_async", "crdt_diff_vv_async", "crdt_diff_vv_closed", "crdt_test_set_vv_lds_words",
    "crdt_checkout_async", "crdt_checkout_lens", "crdt_checkout_read", "crdt_checkout_digest", "crdt_pos_to_loc_at",
    "crdt_loc_to_pos_at", "crdt_pos_to_loc_at_dev_async", "crdt_loc_to_pos_at_dev_async", "crdt_last_checkout_ms",
    "crdt_blame_async", "crdt_blame_counts", "crdt_blame_read", "crdt_last_blame_ms",
    "crdt_encode_async", "crdt_encode_lens", "crdt_encode_read", "crdt_pos_to_units", "crdt_units_to_pos",
    "crdt_pos_to_units_dev_async", "crdt_units_to_pos_dev_async", "crdt_last_encode_ms",
    "crdt_lines_async", "crdt_line_counts", "crdt_lines_read", "crdt_pos_to_linecol", "crdt_linecol_to_pos",
    "crdt_pos_to_linecol_dev_async", "crdt_linecol_to_pos_dev_async", "crdt_last_lines_ms",
    "crdt_find_async", "crdt_find_counts", "crdt_find_read", "crdt_find_seek", "crdt_find_seek_dev_async", "crdt_last_find_ms",
    "crdt_edits_async", "crdt_edits_between_async", "crdt_edits_counts", "crdt_edits_read", "crdt_last_edits_ms",
    "crdt_rebase_async", "crdt_rebase_counts", "crdt_rebase_read", "crdt_rebase", "crdt_rebase_dev_async", "crdt_last_rebase_ms",
    "crdt_set_fused_publish", "crdt_fused_publish_stats", "crdt_debug_vpos", "crdt_debug_publish_plan",
    "crdt_set_replay_balance", "crdt_debug_balance_board", "crdt_set_window_decode", "crdt_set_balance_map",
    # include/crdt_trace.h (host-only trace ingestion)
    "crdt_trace_load", "crdt_trace_parse", "crdt_trace_sizes", "crdt_trace_copy", "crdt_trace_free",
]


def _p(a, t=C.c_uint32):
    return a.ctypes.data_as(C.POINTER(t))


def _check(rc: int, what: str):
    if rc != 0:
        err = lib().crdt_last_error()
        raise CrdtError(f"{what} failed rc={rc} {err.decode() if err else ''}")


class Engine:
    """Many documents on one MI355X.  Mirrors ListCRDT per document (index `doc`)."""

    def __init__(self, n_docs: int, leaf_cap: int = 32, device: int = 0):
        L = lib()
        self.L = L
        self.h = C.c_void_p()
        cfg = L.Cfg(leaf_cap, device)
        _check(L.crdt_engine_create(C.byref(cfg), C.byref(self.h)), "crdt_engine_create")
        _check(L.crdt_docs_alloc(self.h, n_docs), "crdt_docs_alloc")
        self.n_docs = n_docs
        self.leaf_cap = leaf_cap

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.crdt_engine_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- ListCRDT::get_or_create_agent_id (doc.rs:66-80)
    def agent_intern(self, docs: Sequence[int], names: Sequence[str]) -> np.ndarray:
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        out = np.zeros(len(names), np.uint16)
        _check(self.L.crdt_agent_intern(self.h, len(names), _p(d), arr, _p(out, C.c_uint16)), "agent_intern")
        return out

    def agent_intern_dev(self, docs: Sequence[int], names: Sequence) -> tuple:
        """get_or_create_agent_id on the device (k_intern): (ids u16, ranks u32) per name; names
        are str or bytes (any bytes).  Same ids as agent_intern on the same call."""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        bs = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        off = np.zeros(len(bs) + 1, np.uint64)
        off[1:] = np.cumsum([len(b) for b in bs]) if bs else []
        blob = b"".join(bs)
        out = np.zeros(len(bs), np.uint16)
        rank = np.zeros(len(bs), np.uint32)
        _check(self.L.crdt_agent_intern_dev(self.h, len(bs), _p(d), _p(off, C.c_uint64), blob, _p(out, C.c_uint16),
                                            _p(rank)), "agent_intern_dev")
        return out, rank

    @staticmethod
    def _local_arrays(per_doc):
        """per_doc: list of (doc, [(agent, ops[(pos,del,ins)...]), ...])."""
        docs, txn_off, txns, ops = [], [0], [], []
        for doc, tx in per_doc:
            docs.append(doc)
            for agent, o in tx:
                o = np.asarray(o, dtype=np.uint32).reshape(-1, 3)
                txns.append((agent, o.shape[0]))
                ops.append(o)
            txn_off.append(len(txns))
        return (np.array(docs, np.uint32), np.array(txn_off, np.uint64),
                np.array(txns, np.uint32).reshape(-1, 2),
                np.concatenate(ops).astype(np.uint32) if ops else np.zeros((0, 3), np.uint32))

    def apply_local(self, per_doc, stage_only: bool = False) -> np.ndarray:
        return self.apply_local_arrays(*self._local_arrays(per_doc), stage_only=stage_only)

    def apply_local_probed(self, d, off, tx, ops, probes):
        """apply_local_arrays with one probe (pos, agent, seq) after every txn; returns (status,
        answers [T, 4] = (agent, seq) of pos, (pos, deleted) of (agent, seq))"""
        d = np.ascontiguousarray(d, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        tx = np.ascontiguousarray(tx, dtype=np.uint32).reshape(-1, 2)
        ops = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 3)
        pr = np.ascontiguousarray(probes, dtype=np.uint32).reshape(-1, 3)
        ans = np.zeros((tx.shape[0], 4), np.uint32)
        st = np.zeros(d.shape[0], np.int32)
        _check(self.L.crdt_apply_local_probed(self.h, d.shape[0], _p(d), _p(off, C.c_uint64), tx.ctypes.data,
                                              ops.ctypes.data, pr.ctypes.data, ans.ctypes.data, _p(st, C.c_int32)),
               "apply_local_probed")
        return st, ans

    def apply_local_arrays(self, d, off, tx, ops, stage_only: bool = False) -> np.ndarray:
        """crdt_apply_local on CSR arrays: docs [n], txn_off [n+1] (u64), txns [T,2] (agent, n_ops),
        ops [sum n_ops, 3] (pos, del, ins).  stage_only: crdt_stage_local (run() replays it)."""
        d = np.ascontiguousarray(d, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        tx = np.ascontiguousarray(tx, dtype=np.uint32).reshape(-1, 2)
        ops = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 3)
        if stage_only:
            _check(self.L.crdt_stage_local(self.h, d.shape[0], _p(d), _p(off, C.c_uint64), tx.ctypes.data, ops.ctypes.data),
                   "stage_local")
            return np.zeros(d.shape[0], np.int32)
        st = np.zeros(d.shape[0], np.int32)
        _check(self.L.crdt_apply_local(self.h, d.shape[0], _p(d), _p(off, C.c_uint64), tx.ctypes.data,
                                       ops.ctypes.data, _p(st, C.c_int32)), "apply_local")
        return st

    def apply_trace(self, docs: Sequence[int], agent: int | Sequence[int], counts: np.ndarray, patches: np.ndarray,
                    stage_only: bool = False) -> np.ndarray:
        """Apply the same trace (txn patch counts + patches) to every doc in `docs`."""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        n = d.shape[0]
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        agents = np.broadcast_to(np.asarray(agent, dtype=np.uint32), (n,))
        tx = np.zeros((n * counts.shape[0], 2), np.uint32)
        for i in range(n):
            tx[i * counts.shape[0]:(i + 1) * counts.shape[0], 0] = agents[i]
            tx[i * counts.shape[0]:(i + 1) * counts.shape[0], 1] = counts
        off = (np.arange(n + 1, dtype=np.uint64) * counts.shape[0]).astype(np.uint64)
        ops = np.ascontiguousarray(np.tile(np.asarray(patches, np.uint32).reshape(-1, 3), (n, 1)))
        if stage_only:
            _check(self.L.crdt_stage_local(self.h, n, _p(d), _p(off, C.c_uint64), tx.ctypes.data, ops.ctypes.data),
                   "stage_local")
            return np.zeros(n, np.int32)
        st = np.zeros(n, np.int32)
        _check(self.L.crdt_apply_local(self.h, n, _p(d), _p(off, C.c_uint64), tx.ctypes.data, ops.ctypes.data,
                                       _p(st, C.c_int32)), "apply_local")
        return st

    def apply_remote_wire(self, docs: Sequence[int], wires: Sequence[bytes], stage_only: bool = False) -> np.ndarray:
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        arr = (C.c_char_p * len(wires))(*wires)
        ln = np.array([len(w) for w in wires], np.uint64)
        if stage_only:
            _check(self.L.crdt_stage_remote_wire(self.h, d.shape[0], _p(d), arr, _p(ln, C.c_uint64)), "stage_remote")
            return np.zeros(d.shape[0], np.int32)
        st = np.zeros(d.shape[0], np.int32)
        _check(self.L.crdt_apply_remote_wire(self.h, d.shape[0], _p(d), arr, _p(ln, C.c_uint64), _p(st, C.c_int32)),
               "apply_remote_wire")
        return st

    def stage_remote_replicated(self, wire: bytes, rename_idx: int, names: Sequence[str]):
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        _check(self.L.crdt_stage_remote_replicated(self.h, wire, len(wire), rename_idx, arr), "stage_replicated")

    # --- shared local streams (config 3 corpora): doc i replays traces[stream_of_doc[i]] as `agent`
    def stage_local_shared(self, docs: Sequence[int], stream_of_doc: Sequence[int], agent: int, traces) -> None:
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        so = np.ascontiguousarray(stream_of_doc, dtype=np.uint32)
        txn_off = np.concatenate([[0], np.cumsum([t.counts.shape[0] for t in traces])]).astype(np.uint64)
        tx = np.zeros((int(txn_off[-1]), 2), np.uint32)
        tx[:, 0] = agent
        tx[:, 1] = np.concatenate([t.counts for t in traces])
        ops = np.ascontiguousarray(np.concatenate([np.asarray(t.patches, np.uint32).reshape(-1, 3) for t in traces]))
        _check(self.L.crdt_stage_local_shared(self.h, d.shape[0], _p(d), _p(so), len(traces), _p(txn_off, C.c_uint64),
                                              tx.ctypes.data, ops.ctypes.data), "stage_local_shared")

    # --- config 4: make_random_change (doc.rs:544-569) generated on the device
    def stage_random(self, docs: Sequence[int], agent: str, n_ops: int, seed: int):
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        _check(self.L.crdt_stage_random(self.h, d.shape[0], _p(d), agent.encode(), n_ops, seed), "stage_random")

    def apply_random(self, docs: Sequence[int], agent: str, n_ops: int, seed: int) -> np.ndarray:
        self.stage_random(docs, agent, n_ops, seed)
        st = self.run()
        return st[np.asarray(docs, dtype=np.int64)]

    def debug_state(self, doc: int) -> np.ndarray:
        out = np.zeros(23, np.uint32)
        _check(self.L.crdt_debug_state(self.h, doc, _p(out)), "debug_state")
        return out

    def fit(self):
        """shrink capacities to the staged streams' use (after run + publish)"""
        _check(self.L.crdt_fit(self.h), "fit")

    def fit_note(self, apply: bool = False):
        """apply=False: note the capacities fit() would set into each document's running maximum;
        apply=True: capacities = the noted maxima (config 4 corpus batches on one engine)"""
        _check(self.L.crdt_fit_note(self.h, int(apply)), "fit_note")

    def reseed_random_async(self, seed: int, id_base: int):
        """generated-edit documents (stage_random) become documents id_base + d of the corpus"""
        _check(self.L.crdt_reseed_random_async(self.h, C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), C.c_uint64(id_base)),
               "reseed_random_async")

    def digests_dev_async(self, dev_ptr: int):
        """copy the per-document digests to a device buffer (n_docs u64) on the engine stream"""
        _check(self.L.crdt_digest_dev_async(self.h, C.c_void_p(dev_ptr)), "digest_dev_async")

    def share_streams(self, on: bool = True):
        """documents staged from the same host stream read one device copy"""
        _check(self.L.crdt_set_share_streams(self.h, int(on)), "share_streams")

    QUERY_KERNELS = {"lds": 0, "per_thread": 1, "merge": 2}

    def query_kernel(self, mode: str):
        """kernels behind the device query entry points: "lds" (default), "per_thread", "merge"
        (sorted batches; same answers for any batch)"""
        _check(self.L.crdt_set_query_kernel(self.h, self.QUERY_KERNELS[mode]), "query_kernel")

    def device_intern(self, on: bool = True):
        """stage_remote_replicated interns every document's authors with k_intern (same ids)"""
        _check(self.L.crdt_set_device_intern(self.h, int(on)), "device_intern")

    def fused_publish(self, on: bool = True):
        """replay waves publish their own documents on a fitted index (default on; same index)"""
        _check(self.L.crdt_set_fused_publish(self.h, int(on)), "fused_publish")

    def fused_publish_stats(self):
        """(k_replay launches with the fused publish on, per document: the current index was written
        by its replay wave)"""
        n = C.c_uint64()
        per = np.zeros(self.n_docs, np.uint8)
        _check(self.L.crdt_fused_publish_stats(self.h, C.byref(n), _p(per, C.c_uint8)), "fused_publish_stats")
        return n.value, per.astype(bool)

    BALANCE_MODES = {"off": 0, "on": 1, "auto": 2, "rotate": 3}

    def replay_balance(self, mode="auto"):
        """replay waves set their own issue priority as they go ("auto", the default: the rotation
        policy on launches whose waves are all resident at once; "off": never; "on" / "rotate": the
        progress board / the rotation on every launch); same state either way"""
        _check(self.L.crdt_set_replay_balance(self.h, int(self.BALANCE_MODES.get(mode, mode))), "replay_balance")

    def set_balance_map(self, bmap: int):
        """the rotation policy's level map (0 .. BALANCE_MAPS - 1, csrc/balance_levels.h: which waves
        of a SIMD tie at a priority level in a time slice); same state whatever the map"""
        _check(self.L.crdt_set_balance_map(self.h, int(bmap)), "set_balance_map")

    def window_decode(self, on=True):
        """remote-only streams replay in the kernel instance that decodes typing runs once per
        record window (default on) or in the one that scans the window at every insert; same state"""
        _check(self.L.crdt_set_window_decode(self.h, int(on)), "window_decode")

    def balance_board(self):
        """(board [16384, 16] u32: per SIMD row and wave slot, launch stamp << 24 | records left;
        the last replay launch's stamp; the policy it ran with: 0 none, 1 the board, 2 rotation)"""
        board = np.zeros((16384, 16), np.uint32)
        stamp, policy = C.c_uint32(), C.c_int()
        _check(self.L.crdt_debug_balance_board(self.h, _p(board), C.byref(stamp), C.byref(policy)), "debug_balance_board")
        return board, stamp.value, policy.value

    def debug_vpos(self, doc: int) -> np.ndarray:
        """visible items before each canonical span of the document's published index"""
        out = np.zeros(max(int(self.canon_counts()[doc]), 1), np.uint32)
        _check(self.L.crdt_debug_vpos(self.h, doc, _p(out)), "debug_vpos")
        return out[: int(self.canon_counts()[doc])]

    def publish_plan(self):
        """(plan, words) per document, as the host planned them at the last index sizing: plan 0 =
        k_publish + k_pub_index, 1 = k_publish building the index in its own wave, 2 =
        k_publish_big; words = the document's span-start bitmap words (pub_words(ord_cap))"""
        plan = np.zeros(self.n_docs, np.uint8)
        words = np.zeros(self.n_docs, np.uint32)
        _check(self.L.crdt_debug_publish_plan(self.h, _p(plan, C.c_uint8), _p(words)), "debug_publish_plan")
        return plan, words

    def mem_bytes(self) -> int:
        """device bytes held by the per-document pools + staged records"""
        return int(self.L.crdt_mem_bytes(self.h))

    @staticmethod
    def device_bytes(reset_peak: bool = False):
        """(current, peak) device bytes held by this process's engines (crdt_device_bytes)"""
        cur, peak = C.c_uint64(), C.c_uint64()
        lib().crdt_device_bytes(C.byref(cur), C.byref(peak), int(reset_peak))
        return cur.value, peak.value

    def reset_async(self):
        _check(self.L.crdt_reset_async(self.h), "reset")

    def run(self) -> np.ndarray:
        st = np.zeros(self.n_docs, np.int32)
        _check(self.L.crdt_run(self.h, _p(st, C.c_int32)), "run")
        return st

    def run_async(self):
        _check(self.L.crdt_run_async(self.h), "run_async")

    def publish_async(self):
        _check(self.L.crdt_publish_async(self.h), "publish")

    def sync(self):
        _check(self.L.crdt_sync(self.h), "sync")

    def status(self) -> np.ndarray:
        st = np.zeros(self.n_docs, np.int32)
        _check(self.L.crdt_doc_status(self.h, _p(st, C.c_int32)), "status")
        return st

    def lens(self, docs=None) -> np.ndarray:
        d = np.arange(self.n_docs, dtype=np.uint32) if docs is None else np.ascontiguousarray(docs, dtype=np.uint32)
        out = np.zeros(d.shape[0], np.uint32)
        _check(self.L.crdt_doc_len(self.h, d.shape[0], _p(d), _p(out)), "doc_len")
        return out

    def digests(self) -> np.ndarray:
        out = np.zeros(self.n_docs, np.uint64)
        _check(self.L.crdt_digest(self.h, _p(out, C.c_uint64)), "digest")
        return out

    def canon_counts(self) -> np.ndarray:
        """canonical spans of every document's published index"""
        out = np.zeros(self.n_docs, np.uint32)
        _check(self.L.crdt_canon_counts(self.h, _p(out)), "canon_counts")
        return out

    def pos_to_loc(self, docs, pos):
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        p = np.ascontiguousarray(pos, dtype=np.uint32)
        a = np.zeros(p.shape[0], np.uint16)
        s = np.zeros(p.shape[0], np.uint32)
        _check(self.L.crdt_pos_to_loc(self.h, p.shape[0], _p(d), _p(p), _p(a, C.c_uint16), _p(s)), "pos_to_loc")
        return a, s

    def loc_to_pos(self, docs, agent, seq):
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        a = np.ascontiguousarray(agent, dtype=np.uint16)
        s = np.ascontiguousarray(seq, dtype=np.uint32)
        p = np.zeros(s.shape[0], np.uint32)
        dl = np.zeros(s.shape[0], np.uint8)
        _check(self.L.crdt_loc_to_pos(self.h, s.shape[0], _p(d), _p(a, C.c_uint16), _p(s), _p(p), _p(dl, C.c_uint8)),
               "loc_to_pos")
        return p, dl

    def export_sizes(self, doc: int) -> dict:
        s = np.zeros(12, np.uint64)
        _check(self.L.crdt_export_sizes(self.h, doc, _p(s, C.c_uint64)), "export_sizes")
        keys = ["raw", "leaves", "canon", "cwo", "deletes", "dd", "txns", "parents", "frontier", "agents",
                "next_order", "len"]
        return {k: int(v) for k, v in zip(keys, s)}

    def export(self, doc: int) -> dict:
        s = np.zeros(12, np.uint64)
        _check(self.L.crdt_export_sizes(self.h, doc, _p(s, C.c_uint64)), "export_sizes")
        n = [int(x) for x in s]
        raw = np.zeros((n[0], 4), np.uint32)
        ls = np.zeros(n[1], np.uint32)
        canon = np.zeros((n[2], 4), np.uint32)
        cwo = np.zeros((n[3], 4), np.uint32)
        dl = np.zeros((n[4], 3), np.uint32)
        dd = np.zeros((n[5], 3), np.uint32)
        tx = np.zeros((n[6], 5), np.uint32)
        pa = np.zeros(n[7], np.uint32)
        fr = np.zeros(n[8], np.uint32)
        _check(self.L.crdt_export(self.h, doc, _p(raw), _p(ls), _p(canon), _p(cwo), _p(dl), _p(dd), _p(tx), _p(pa),
                                  _p(fr)), "export")
        return dict(raw=raw, leaf_sizes=ls, canon=canon, cwo=cwo, deletes=dl, dd=dd, txns=tx, parents=pa,
                    frontier=fr, len=n[11], next_order=n[10])

    # --- text materialisation (ListCRDT::to_string with the rope on, doc.rs:498-505)
    def set_content(self, docs: Sequence[int], stream_of_doc: Sequence[int], streams: Sequence[np.ndarray]):
        """docs[i] reads the order-indexed UTF-32 table streams[stream_of_doc[i]]."""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        so = np.ascontiguousarray(stream_of_doc, dtype=np.uint32)
        off = np.concatenate([[0], np.cumsum([len(x) for x in streams])]).astype(np.uint64)
        data = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint32) for x in streams])
                                    if streams else np.zeros(0, np.uint32))
        _check(self.L.crdt_set_content(self.h, d.shape[0], _p(d), _p(so), len(streams), _p(off, C.c_uint64),
                                       _p(data)), "set_content")

    def set_content_copies(self, docs: Sequence[int], content: np.ndarray):
        """every docs[i] gets its own device copy of one order-indexed UTF-32 table"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        c = np.ascontiguousarray(content, dtype=np.uint32)
        _check(self.L.crdt_set_content_copies(self.h, d.shape[0], _p(d), _p(c), c.shape[0]), "set_content_copies")

    def materialize_async(self):
        _check(self.L.crdt_materialize_async(self.h), "materialize")

    def text(self, doc: int) -> np.ndarray:
        n = C.c_uint64()
        _check(self.L.crdt_text(self.h, doc, None, 0, C.byref(n)), "text")
        out = np.zeros(n.value, np.uint32)
        _check(self.L.crdt_text(self.h, doc, _p(out), n.value, C.byref(n)), "text")
        return out

    def text_digests(self) -> np.ndarray:
        out = np.zeros(self.n_docs, np.uint64)
        _check(self.L.crdt_text_digest(self.h, _p(out, C.c_uint64)), "text_digest")
        return out

    def materialize_ms(self) -> float:
        x = C.c_double()
        self.L.crdt_last_materialize_ms(self.h, C.byref(x))
        return x.value

    # --- what a replay changed: text patches from a past version to now (crdt_gpu.h "what a replay changed")
    def versions(self, docs=None) -> np.ndarray:
        """next order of every listed document (get_next_order): the version diff() counts from"""
        d = np.arange(self.n_docs, dtype=np.uint32) if docs is None else np.ascontiguousarray(docs, dtype=np.uint32)
        out = np.zeros(d.shape[0], np.uint32)
        _check(self.L.crdt_doc_version(self.h, d.shape[0], _p(d), _p(out)), "doc_version")
        return out

    def diff_async(self, docs, since):
        """compute the patches from version since[i] to now for docs[i] (no duplicates) on the device"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        s = np.ascontiguousarray(since, dtype=np.uint32)
        if d.shape != s.shape or d.ndim != 1:
            raise ValueError("diff: docs and since are 1-d and of equal length")
        _check(self.L.crdt_diff_async(self.h, d.shape[0], _p(d), _p(s)), "diff_async")
        self._diff_n = d.shape[0]

    def diff_counts(self):
        """(n_patches, n_ins) per index of the last diff_async; 0xFFFFFFFF marks an index without a
        result (since above the document's version, or a poisoned document)"""
        n = getattr(self, "_diff_n", 0)
        npat, nins = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        _check(self.L.crdt_diff_counts(self.h, _p(npat), _p(nins)), "diff_counts")
        return npat, nins

    def diff_read(self, i: int, counts=None, text: bool = True):
        """result i of the last diff_async: (patches [n, 4] u32 = (pos, del_len, ins_len, ins_off),
        ins_order, ins_text or None); raises CrdtError (rc=-100) for an index without a result"""
        npat, nins = counts if counts is not None else self.diff_counts()
        bad = not 0 <= i < len(npat) or int(npat[i]) == 0xFFFFFFFF  # (the library answers CRDT_E_ARG)
        pat = np.zeros((0 if bad else int(npat[i]), 4), np.uint32)
        io = np.zeros(0 if bad else int(nins[i]), np.uint32)
        _check(self.L.crdt_diff_read(self.h, i, pat.ctypes.data, _p(io), None), "diff_read")
        it = None
        if text:
            it = np.zeros_like(io)
            if self.L.crdt_diff_read(self.h, i, None, None, _p(it)) != 0:
                it = None  # (no content, or too short a stream, for this document)
        return pat, io, it

    def diff(self, docs, since, strict: bool = True):
        """[(patches (n, 4) u32, ins_order, ins_text or None)] per docs[i]: the patches that turn the
        text of docs[i] at version since[i] into its current text.  An index without a result
        (since above the version, a poisoned document) raises CrdtError, or is None with
        strict=False; the other indexes are not affected."""
        self.diff_async(docs, since)
        counts = self.diff_counts()
        bad = np.flatnonzero(counts[0] == 0xFFFFFFFF)
        if strict and bad.size:
            raise CrdtError(f"diff failed rc=-100 for indexes {bad.tolist()}: since above the version, or a poisoned document")
        return [None if int(counts[0][i]) == 0xFFFFFFFF else self.diff_read(i, counts) for i in range(len(counts[0]))]

    def diff_between_async(self, docs, from_, to):
        """compute the patches from version from_[i] to version to[i] for docs[i] (no duplicates) on
        the device; the result replaces the last diff result and is read like one (diff_counts,
        diff_read, diff_ms, rebase_async("diff"))"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        a = np.ascontiguousarray(from_, dtype=np.uint32)
        b = np.ascontiguousarray(to, dtype=np.uint32)
        if d.shape != a.shape or d.shape != b.shape or d.ndim != 1:
            raise ValueError("diff_between: docs, from_ and to are 1-d and of equal length")
        _check(self.L.crdt_diff_between_async(self.h, d.shape[0], _p(d), _p(a), _p(b)), "diff_between_async")
        self._diff_n = d.shape[0]

    def diff_between(self, docs, from_, to, strict: bool = True):
        """what diff() returns, for the patches that turn the text of docs[i] at version from_[i]
        into its text at version to[i] (either may be the later one).  An index without a result
        (a version above the document's, a poisoned document) raises CrdtError, or is None with
        strict=False; the other indexes are not affected."""
        self.diff_between_async(docs, from_, to)
        counts = self.diff_counts()
        bad = np.flatnonzero(counts[0] == 0xFFFFFFFF)
        if strict and bad.size:
            raise CrdtError(f"diff_between failed rc=-100 for indexes {bad.tolist()}: a version above the document's, or a poisoned document")
        return [None if int(counts[0][i]) == 0xFFFFFFFF else self.diff_read(i, counts) for i in range(len(counts[0]))]

    # --- causal versions: version vectors (crdt_gpu.h "Causal versions")
    EXPORT_SIZES_AGENTS = 9  # crdt_export_sizes: the index of a document's agent count

    def _n_agents(self, docs) -> np.ndarray:
        """agent count of every listed document: the length of its version vectors (one
        crdt_export_sizes call per distinct document; pass n_agents to version_vector to skip it)"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        s = np.zeros(12, np.uint64)
        seen = {}
        for x in d.tolist():
            if x not in seen:
                _check(self.L.crdt_export_sizes(self.h, x, _p(s, C.c_uint64)), "export_sizes")
                seen[x] = int(s[self.EXPORT_SIZES_AGENTS])
        return np.array([seen[x] for x in d.tolist()], np.uint32)

    def version_vector(self, docs, versions=None, n_agents=None):
        """[vv (n_agents,) u32] per docs[q]: the version vector of the order prefix versions[q] of
        docs[q] (None: now), vv[a] = the seqs of agent id a among the orders below it.  n_agents:
        the documents' agent counts if the caller holds them (one number, or one per query; a
        count below a document's raises CrdtError); else they are asked for, document by document"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        v = None if versions is None else np.ascontiguousarray(versions, dtype=np.uint32)
        if d.ndim != 1 or (v is not None and v.shape != d.shape):
            raise ValueError("version_vector: docs and versions are 1-d and of equal length")
        na = self._n_agents(d) if n_agents is None else np.broadcast_to(np.asarray(n_agents, np.uint32), d.shape)
        off = np.zeros(d.shape[0] + 1, np.uint64)
        off[1:] = np.cumsum(na, dtype=np.uint64)
        out = np.zeros(int(off[-1]), np.uint32)
        _check(self.L.crdt_version_vector(self.h, d.shape[0], _p(d), None if v is None else _p(v), _p(off, C.c_uint64), _p(out)),
               "version_vector")
        return [out[int(off[q]):int(off[q + 1])].copy() for q in range(d.shape[0])]

    def diff_vv_async(self, docs, from_vv, to_vv):
        """compute the patches from the causal version from_vv[i] to the causal version to_vv[i] of
        docs[i] (no duplicates; two version vectors per index, sequences of per-agent seq counts,
        the shorter of a pair padded with 0) on the device; the result replaces the last diff
        result and is read like one (diff_counts, diff_read, diff_ms, rebase_async("diff"))"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        if d.ndim != 1 or len(from_vv) != d.shape[0] or len(to_vv) != d.shape[0]:
            raise ValueError("diff_vv: docs is 1-d, with a from and a to vector per document")
        fa = [np.asarray(x, dtype=np.uint32).ravel() for x in from_vv]
        ta = [np.asarray(x, dtype=np.uint32).ravel() for x in to_vv]
        ln = np.array([max(len(x), len(y)) for x, y in zip(fa, ta)], dtype=np.uint64)
        off = np.zeros(d.shape[0] + 1, np.uint64)
        off[1:] = np.cumsum(ln, dtype=np.uint64)
        f, t = np.zeros(int(off[-1]) + 1, np.uint32), np.zeros(int(off[-1]) + 1, np.uint32)
        for i, (x, y) in enumerate(zip(fa, ta)):
            f[int(off[i]):int(off[i]) + len(x)] = x
            t[int(off[i]):int(off[i]) + len(y)] = y
        _check(self.L.crdt_diff_vv_async(self.h, d.shape[0], _p(d), _p(off, C.c_uint64), _p(f), _p(t)), "diff_vv_async")
        self._diff_n = d.shape[0]

    def diff_vv(self, docs, from_vv, to_vv, strict: bool = True):
        """what diff_between() returns, for the patches that turn the text of docs[i] at the causal
        version from_vv[i] into its text at to_vv[i].  An index without a result (a vector longer
        than the document's agents, an entry above the agent's next seq, a poisoned document)
        raises CrdtError, or is None with strict=False; the other indexes are not affected."""
        self.diff_vv_async(docs, from_vv, to_vv)
        counts = self.diff_counts()
        bad = np.flatnonzero(counts[0] == 0xFFFFFFFF)
        if strict and bad.size:
            raise CrdtError(f"diff_vv failed rc=-100 for indexes {bad.tolist()}: a vector out of bounds, or a poisoned document")
        return [None if int(counts[0][i]) == 0xFFFFFFFF else self.diff_read(i, counts) for i in range(len(counts[0]))]

    def diff_vv_closed(self):
        """(closed_from, closed_to) bool arrays per index of the last diff_vv: the side's set of
        orders is causally closed (every txn it touches with its parents, and from its first order)"""
        n = getattr(self, "_diff_n", 0)
        a, b = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        _check(self.L.crdt_diff_vv_closed(self.h, _p(a, C.c_uint8), _p(b, C.c_uint8)), "diff_vv_closed")
        return a.astype(bool), b.astype(bool)

    def diff_ms(self) -> float:
        """device time of the last diff (HIP events)"""
        x = C.c_double()
        _check(self.L.crdt_last_diff_ms(self.h, C.byref(x)), "last_diff_ms")
        return x.value

    # --- text edits in units (crdt_gpu.h "text edits in units")
    def edits_async(self, docs, since, enc="utf8"):
        """compute the edits from version since[i] to now for docs[i] (no duplicates) on the device,
        in units of enc ("utf8" / "utf16", or CRDT_ENC_UTF8 = 0 / CRDT_ENC_UTF16 = 1); replaces the
        last edits result"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        s = np.ascontiguousarray(since, dtype=np.uint32)
        if d.shape != s.shape or d.ndim != 1:
            raise ValueError("edits: docs and since are 1-d and of equal length")
        enc = int(self.ENCODINGS.get(enc, enc))
        _check(self.L.crdt_edits_async(self.h, d.shape[0], _p(d), _p(s), enc), "edits_async")
        self._ed_n, self._ed_enc = d.shape[0], enc

    def edits_counts(self):
        """(n_edits, n_ins_units) per index of the last edits_async; 0xFFFFFFFF marks an index
        without a result (since above the version, a poisoned document, one without content)"""
        n = getattr(self, "_ed_n", 0)
        ned, nun = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        _check(self.L.crdt_edits_counts(self.h, _p(ned), _p(nun)), "edits_counts")
        return ned, nun

    def edits_read(self, i: int, counts=None):
        """result i of the last edits_async: (edits [n, 8] u32 = (pos, del_len, ins_len, unit,
        del_units, ins_units, ins_off, 0), ins: np.uint8 (UTF-8) or np.uint16 (UTF-16) array);
        raises CrdtError (rc=-100) for an index without a result"""
        ned, nun = counts if counts is not None else self.edits_counts()
        bad = not 0 <= i < len(ned) or int(ned[i]) == 0xFFFFFFFF  # (the library answers CRDT_E_ARG)
        ed = np.zeros((0 if bad else int(ned[i]), 8), np.uint32)
        ins = np.zeros(0 if bad else int(nun[i]), np.uint16 if getattr(self, "_ed_enc", 0) == 1 else np.uint8)
        _check(self.L.crdt_edits_read(self.h, i, ed.ctypes.data, ins.ctypes.data), "edits_read")
        return ed, ins

    def edits(self, docs, since, enc="utf8", strict: bool = True):
        """[(edits (n, 8) u32, ins np.uint8 | np.uint16)] per docs[i]: the edits that turn the encoded
        text of docs[i] at version since[i] into its encoded current text.  An index without a result
        raises CrdtError, or is None with strict=False; the other indexes are not affected."""
        self.edits_async(docs, since, enc)
        counts = self.edits_counts()
        bad = np.flatnonzero(counts[0] == 0xFFFFFFFF)
        if strict and bad.size:
            raise CrdtError(f"edits failed rc=-100 for indexes {bad.tolist()}: since above the version, a poisoned "
                            f"document, or one without content")
        return [None if int(counts[0][i]) == 0xFFFFFFFF else self.edits_read(i, counts) for i in range(len(counts[0]))]

    def edits_between_async(self, docs, from_, to, enc="utf8"):
        """compute the edits from version from_[i] to version to[i] for docs[i] (no duplicates) on the
        device, in units of enc; the result replaces the last edits result and is read like one
        (edits_counts, edits_read, edits_ms, rebase_async("edits"))"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        a = np.ascontiguousarray(from_, dtype=np.uint32)
        b = np.ascontiguousarray(to, dtype=np.uint32)
        if d.shape != a.shape or d.shape != b.shape or d.ndim != 1:
            raise ValueError("edits_between: docs, from_ and to are 1-d and of equal length")
        enc = int(self.ENCODINGS.get(enc, enc))
        _check(self.L.crdt_edits_between_async(self.h, d.shape[0], _p(d), _p(a), _p(b), enc), "edits_between_async")
        self._ed_n, self._ed_enc = d.shape[0], enc

    def edits_between(self, docs, from_, to, enc="utf8", strict: bool = True):
        """what edits() returns, for the edits that turn the encoded text of docs[i] at version
        from_[i] into its encoded text at version to[i] (either may be the later one).  An index
        without a result raises CrdtError, or is None with strict=False; the other indexes are not
        affected."""
        self.edits_between_async(docs, from_, to, enc)
        counts = self.edits_counts()
        bad = np.flatnonzero(counts[0] == 0xFFFFFFFF)
        if strict and bad.size:
            raise CrdtError(f"edits_between failed rc=-100 for indexes {bad.tolist()}: a version above the document's, a "
                            f"poisoned document, or one without content")
        return [None if int(counts[0][i]) == 0xFFFFFFFF else self.edits_read(i, counts) for i in range(len(counts[0]))]

    def edits_ms(self) -> float:
        """device time of the last edits call (HIP events)"""
        x = C.c_double()
        _check(self.L.crdt_last_edits_ms(self.h, C.byref(x)), "last_edits_ms")
        return x.value

    # --- documents at a past version (crdt_gpu.h "documents at a past version")
    def checkout_async(self, docs, versions):
        """build the views of docs[i] (no duplicates) at versions[i] on the device; replaces the last checkout"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        v = np.ascontiguousarray(versions, dtype=np.uint32)
        if d.shape != v.shape or d.ndim != 1:
            raise ValueError("checkout: docs and versions are 1-d and of equal length")
        _check(self.L.crdt_checkout_async(self.h, d.shape[0], _p(d), _p(v)), "checkout_async")
        self._co_n = d.shape[0]

    def checkout_lens(self) -> np.ndarray:
        """length of every index of the last checkout_async; 0xFFFFFFFF marks an index without a result
        (version above the document's version, or a poisoned document)"""
        out = np.zeros(getattr(self, "_co_n", 0), np.uint32)
        _check(self.L.crdt_checkout_lens(self.h, _p(out)), "checkout_lens")
        return out

    def checkout_read(self, i: int, lens=None, text: bool = True):
        """view i of the last checkout_async: (order of every item in document order, their code points
        or None); raises CrdtError (rc=-100) for an index without a result"""
        lens = lens if lens is not None else self.checkout_lens()
        bad = not 0 <= i < len(lens) or int(lens[i]) == 0xFFFFFFFF  # (the library answers CRDT_E_ARG)
        order = np.zeros(0 if bad else int(lens[i]), np.uint32)
        _check(self.L.crdt_checkout_read(self.h, i, _p(order), None), "checkout_read")
        tx = None
        if text:
            tx = np.zeros_like(order)
            if self.L.crdt_checkout_read(self.h, i, None, _p(tx)) != 0:
                tx = None  # (no content, or too short a stream, for this document)
        return order, tx

    def checkout(self, docs, versions, strict: bool = True):
        """[(order, text or None)] per docs[i]: the document at version versions[i].  An index without
        a result raises CrdtError, or is None with strict=False; the other indexes are not affected."""
        self.checkout_async(docs, versions)
        lens = self.checkout_lens()
        bad = np.flatnonzero(lens == 0xFFFFFFFF)
        if strict and bad.size:
            raise CrdtError(f"checkout failed rc=-100 for indexes {bad.tolist()}: version above the document's, or a poisoned document")
        return [None if int(lens[i]) == 0xFFFFFFFF else self.checkout_read(i, lens) for i in range(len(lens))]

    def checkout_digests(self) -> np.ndarray:
        """text digest of every index of the last checkout (0: no content, or no result)"""
        out = np.zeros(getattr(self, "_co_n", 0), np.uint64)
        _check(self.L.crdt_checkout_digest(self.h, _p(out, C.c_uint64)), "checkout_digest")
        return out

    def pos_to_loc_at(self, idx, pos):
        """pos_to_loc on the views of the last checkout: idx[q] names an index of it"""
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        p = np.ascontiguousarray(pos, dtype=np.uint32)
        a = np.zeros(p.shape[0], np.uint16)
        s = np.zeros(p.shape[0], np.uint32)
        _check(self.L.crdt_pos_to_loc_at(self.h, p.shape[0], _p(i), _p(p), _p(a, C.c_uint16), _p(s)), "pos_to_loc_at")
        return a, s

    def loc_to_pos_at(self, idx, agent, seq):
        """loc_to_pos on the views of the last checkout (deleted: 0/1, 2 = not known at that version)"""
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        a = np.ascontiguousarray(agent, dtype=np.uint16)
        s = np.ascontiguousarray(seq, dtype=np.uint32)
        p = np.zeros(s.shape[0], np.uint32)
        dl = np.zeros(s.shape[0], np.uint8)
        _check(self.L.crdt_loc_to_pos_at(self.h, s.shape[0], _p(i), _p(a, C.c_uint16), _p(s), _p(p), _p(dl, C.c_uint8)),
               "loc_to_pos_at")
        return p, dl

    def checkout_ms(self) -> float:
        """device time of the last checkout (HIP events)"""
        x = C.c_double()
        _check(self.L.crdt_last_checkout_ms(self.h, C.byref(x)), "last_checkout_ms")
        return x.value

    # --- who wrote what: authorship runs of the current text (crdt_gpu.h "who wrote what")
    BLAME_MODES = {"agent": 0, "id": 1}

    def blame_async(self, docs, mode):
        """compute the authorship runs of docs[i] (no duplicates) on the device; mode is "agent" / "id"
        (or CRDT_BLAME_AGENT = 0 / CRDT_BLAME_ID = 1); replaces the last blame"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        if d.ndim != 1:
            raise ValueError("blame: docs is 1-d")
        _check(self.L.crdt_blame_async(self.h, d.shape[0], _p(d), int(self.BLAME_MODES.get(mode, mode))), "blame_async")
        self._blame_n = d.shape[0]

    def blame_counts(self) -> np.ndarray:
        """runs per index of the last blame_async; 0xFFFFFFFF marks an index without a result (a
        poisoned document)"""
        out = np.zeros(getattr(self, "_blame_n", 0), np.uint32)
        _check(self.L.crdt_blame_counts(self.h, _p(out)), "blame_counts")
        return out

    def blame_read(self, i: int, counts=None) -> np.ndarray:
        """result i of the last blame_async: runs [n, 4] u32 = (pos, len, agent, seq); raises CrdtError
        (rc=-100) for an index without a result"""
        counts = counts if counts is not None else self.blame_counts()
        bad = not 0 <= i < len(counts) or int(counts[i]) == 0xFFFFFFFF  # (the library answers CRDT_E_ARG)
        runs = np.zeros((0 if bad else int(counts[i]), 4), np.uint32)
        _check(self.L.crdt_blame_read(self.h, i, runs.ctypes.data), "blame_read")
        return runs

    def blame(self, docs, mode="agent", strict: bool = True):
        """[runs (n, 4) u32 = (pos, len, agent, seq)] per docs[i]: maximal stretches of the current text
        by one agent (mode="agent"), or with consecutive ids (mode="id": item pos + j of a run is
        (agent, seq + j)).  An index without a result (a poisoned document) raises CrdtError, or is
        None with strict=False; the other indexes are not affected."""
        self.blame_async(docs, mode)
        counts = self.blame_counts()
        bad = np.flatnonzero(counts == 0xFFFFFFFF)
        if strict and bad.size:
            raise CrdtError(f"blame failed rc=-100 for indexes {bad.tolist()}: a poisoned document")
        return [None if int(counts[i]) == 0xFFFFFFFF else self.blame_read(i, counts) for i in range(len(counts))]

    def blame_ms(self) -> float:
        """device time of the last blame (HIP events)"""
        x = C.c_double()
        _check(self.L.crdt_last_blame_ms(self.h, C.byref(x)), "last_blame_ms")
        return x.value

    # --- encoded text and unit offsets (crdt_gpu.h "encoded text and unit offsets")
    ENCODINGS = {"utf8": 0, "utf16": 1}

    def encode_async(self, docs, enc):
        """encode the text of docs[i] (no duplicates) on the device; enc is "utf8" / "utf16" (or
        CRDT_ENC_UTF8 = 0 / CRDT_ENC_UTF16 = 1); replaces the last encode"""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        if d.ndim != 1:
            raise ValueError("encode: docs is 1-d")
        enc = int(self.ENCODINGS.get(enc, enc))
        _check(self.L.crdt_encode_async(self.h, d.shape[0], _p(d), enc), "encode_async")
        self._enc_n, self._enc = d.shape[0], enc

    def encode_lens(self):
        """(units, chars) per index of the last encode_async; 0xFFFFFFFF marks an index without a
        result (a poisoned document, one without content or with too short a stream)"""
        n = getattr(self, "_enc_n", 0)
        units, chars = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        _check(self.L.crdt_encode_lens(self.h, _p(units), _p(chars)), "encode_lens")
        return units, chars

    def encode_read(self, i: int, lens=None):
        """result i of the last encode_async: bytes (UTF-8) or an np.uint16 array (UTF-16); raises
        CrdtError (rc=-100) for an index without a result"""
        units = (lens if lens is not None else self.encode_lens())[0]
        bad = not 0 <= i < len(units) or int(units[i]) == 0xFFFFFFFF  # (the library answers CRDT_E_ARG)
        n = 0 if bad else int(units[i])
        out = np.zeros(n, np.uint16 if getattr(self, "_enc", 0) == 1 else np.uint8)
        _check(self.L.crdt_encode_read(self.h, i, out.ctypes.data, n), "encode_read")
        return out if out.dtype == np.uint16 else out.tobytes()

    def encode(self, docs, enc="utf8", strict: bool = True):
        """[bytes (enc="utf8") or np.uint16 array (enc="utf16")] per docs[i]: the document's text,
        encoded.  An index without a result raises CrdtError, or is None with strict=False; the other
        indexes are not affected."""
        self.encode_async(docs, enc)
        lens = self.encode_lens()
        bad = np.flatnonzero(lens[0] == 0xFFFFFFFF)
        if strict and bad.size:
            raise CrdtError(f"encode failed rc=-100 for indexes {bad.tolist()}: a poisoned document, or one without content")
        return [None if int(lens[0][i]) == 0xFFFFFFFF else self.encode_read(i, lens) for i in range(len(lens[0]))]

    def pos_to_units(self, idx, pos) -> np.ndarray:
        """units before char pos[q] of index idx[q] of the last encode (0xFFFFFFFF: pos above its chars)"""
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        p = np.ascontiguousarray(pos, dtype=np.uint32)
        if i.shape != p.shape or i.ndim != 1:
            raise ValueError("pos_to_units: idx and pos are 1-d and of equal length")
        u = np.zeros(p.shape[0], np.uint32)
        _check(self.L.crdt_pos_to_units(self.h, p.shape[0], _p(i), _p(p), _p(u)), "pos_to_units")
        return u

    def units_to_pos(self, idx, unit):
        """(pos, mid): the char of index idx[q] of the last encode that covers unit unit[q], and whether
        the unit is not that char's first (0xFFFFFFFF, 0: unit above its units)"""
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        u = np.ascontiguousarray(unit, dtype=np.uint32)
        if i.shape != u.shape or i.ndim != 1:
            raise ValueError("units_to_pos: idx and unit are 1-d and of equal length")
        p = np.zeros(u.shape[0], np.uint32)
        m = np.zeros(u.shape[0], np.uint8)
        _check(self.L.crdt_units_to_pos(self.h, u.shape[0], _p(i), _p(u), _p(p), _p(m, C.c_uint8)), "units_to_pos")
        return p, m

    def encode_ms(self) -> float:
        """device time of the last encode (HIP events)"""
        x = C.c_double()
        _check(self.L.crdt_last_encode_ms(self.h, C.byref(x)), "last_encode_ms")
        return x.value

    # --- line index of the last encode (crdt_gpu.h "line index")
    EOLS = {"lf": 0, "any": 1}
    COL_KINDS = {"units": 0, "chars": 1}

    def lines_async(self, eol):
        """index the lines of every index of the last encode on the device; eol is "lf" / "any" (or
        CRDT_EOL_LF = 0 / CRDT_EOL_ANY = 1); replaces the last line index"""
        _check(self.L.crdt_lines_async(self.h, int(self.EOLS.get(eol, eol))), "lines_async")

    def line_counts(self) -> np.ndarray:
        """lines per index of the last encode; 0xFFFFFFFF marks an index without a result"""
        out = np.zeros(getattr(self, "_enc_n", 0), np.uint32)
        _check(self.L.crdt_line_counts(self.h, _p(out)), "line_counts")
        return out

    def lines_read(self, i: int, counts=None) -> np.ndarray:
        """the line starts of index i: [n_lines, 2] u32 = (unit, pos); raises CrdtError (rc=-100) for
        an index without a result"""
        counts = counts if counts is not None else self.line_counts()
        bad = not 0 <= i < len(counts) or int(counts[i]) == 0xFFFFFFFF  # (the library answers CRDT_E_ARG)
        out = np.zeros((1 if bad else int(counts[i]), 2), np.uint32)
        _check(self.L.crdt_lines_read(self.h, i, out.ctypes.data), "lines_read")
        return out

    def lines(self, eol="lf", strict: bool = True):
        """[line starts (n_lines, 2) u32 = (unit, pos)] per index of the last encode.  An index
        without a result raises CrdtError, or is None with strict=False."""
        self.lines_async(eol)
        counts = self.line_counts()
        bad = np.flatnonzero(counts == 0xFFFFFFFF)
        if strict and bad.size:
            raise CrdtError(f"lines failed rc=-100 for indexes {bad.tolist()}: the encode has no result for them")
        return [None if int(counts[i]) == 0xFFFFFFFF else self.lines_read(i, counts) for i in range(len(counts))]

    def pos_to_linecol(self, idx, pos, col="units"):
        """(line, col) of char pos[q] of index idx[q]; col counts "units" of the encode or "chars"
        (0xFFFFFFFF for both: pos above its chars)"""
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        p = np.ascontiguousarray(pos, dtype=np.uint32)
        if i.shape != p.shape or i.ndim != 1:
            raise ValueError("pos_to_linecol: idx and pos are 1-d and of equal length")
        ln, c = np.zeros(p.shape[0], np.uint32), np.zeros(p.shape[0], np.uint32)
        _check(self.L.crdt_pos_to_linecol(self.h, p.shape[0], _p(i), _p(p), int(self.COL_KINDS.get(col, col)), _p(ln), _p(c)),
               "pos_to_linecol")
        return ln, c

    def linecol_to_pos(self, idx, line, col, kind="units"):
        """(pos, mid): the char at column col[q] ("units" of the encode, or "chars") of line line[q] of
        index idx[q], and whether a unit column falls inside it (0xFFFFFFFF, 0: no such line or column)"""
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        ln = np.ascontiguousarray(line, dtype=np.uint32)
        c = np.ascontiguousarray(col, dtype=np.uint32)
        if not i.shape == ln.shape == c.shape or i.ndim != 1:
            raise ValueError("linecol_to_pos: idx, line and col are 1-d and of equal length")
        p = np.zeros(c.shape[0], np.uint32)
        m = np.zeros(c.shape[0], np.uint8)
        _check(self.L.crdt_linecol_to_pos(self.h, c.shape[0], _p(i), _p(ln), _p(c), int(self.COL_KINDS.get(kind, kind)), _p(p),
                                          _p(m, C.c_uint8)), "linecol_to_pos")
        return p, m

    def lines_ms(self) -> float:
        """device time of the last line index (HIP events)"""
        x = C.c_double()
        _check(self.L.crdt_last_lines_ms(self.h, C.byref(x)), "last_lines_ms")
        return x.value

    # --- find in the last encode (crdt_gpu.h "find")
    SEEK_DIRS = {"next": 0, "prev": 1}

    def find_async(self, pattern, icase: bool = False):
        """search every index of the last encode on the device for `pattern`: a str (its code points
        by ord, so lone surrogates are possible) or a uint32 array of 1..64 code points; icase folds
        ASCII A-Z only; replaces the last find result"""
        if isinstance(pattern, str):
            pattern = [ord(c) for c in pattern]
        p = np.ascontiguousarray(pattern, dtype=np.uint32)
        if p.ndim != 1:
            raise ValueError("find: pattern is a str or 1-d")
        _check(self.L.crdt_find_async(self.h, _p(p), p.shape[0], 1 if icase else 0), "find_async")

    def find_counts(self) -> np.ndarray:
        """matches per index of the last encode; 0xFFFFFFFF marks an index without a result"""
        out = np.zeros(getattr(self, "_enc_n", 0), np.uint32)
        _check(self.L.crdt_find_counts(self.h, _p(out)), "find_counts")
        return out

    def find_read(self, i: int, counts=None) -> np.ndarray:
        """the matches of index i: [n_matches, 2] u32 = (unit, pos), ascending; raises CrdtError
        (rc=-100) for an index without a result"""
        counts = counts if counts is not None else self.find_counts()
        bad = not 0 <= i < len(counts) or int(counts[i]) == 0xFFFFFFFF  # (the library answers CRDT_E_ARG)
        out = np.zeros((0 if bad else int(counts[i]), 2), np.uint32)
        _check(self.L.crdt_find_read(self.h, i, out.ctypes.data if out.size else None), "find_read")
        return out

    def find(self, pattern, icase: bool = False, strict: bool = True):
        """[matches (n_matches, 2) u32 = (unit, pos)] per index of the last encode.  An index without
        a result raises CrdtError, or is None with strict=False."""
        self.find_async(pattern, icase)
        counts = self.find_counts()
        bad = np.flatnonzero(counts == 0xFFFFFFFF)
        if strict and bad.size:
            raise CrdtError(f"find failed rc=-100 for indexes {bad.tolist()}: the encode has no result for them")
        return [None if int(counts[i]) == 0xFFFFFFFF else self.find_read(i, counts) for i in range(len(counts))]

    def find_seek(self, idx, pos, dir="next") -> np.ndarray:
        """the number, within index idx[q], of the first match at or after char pos[q] (dir "next") or
        of the last match at or before it ("prev"); 0xFFFFFFFF: none"""
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        p = np.ascontiguousarray(pos, dtype=np.uint32)
        if i.shape != p.shape or i.ndim != 1:
            raise ValueError("find_seek: idx and pos are 1-d and of equal length")
        k = np.zeros(p.shape[0], np.uint32)
        _check(self.L.crdt_find_seek(self.h, p.shape[0], _p(i), _p(p), int(self.SEEK_DIRS.get(dir, dir)), _p(k)), "find_seek")
        return k

    def find_ms(self) -> float:
        """device time of the last find (HIP events)"""
        x = C.c_double()
        _check(self.L.crdt_last_find_ms(self.h, C.byref(x)), "last_find_ms")
        return x.value

    # --- rebase: positions between a past version and the current text (crdt_gpu.h "rebase")
    REBASE_SRCS = {"diff": 0, "edits": 1}
    REBASE_KINDS = {"chars": 0, "units": 1}
    REBASE_DIRS = {"old_to_new": 0, "new_to_old": 1}
    BIASES = {"left": 0, "right": 1}

    def rebase_async(self, src="diff"):
        """build the rebase map on the device from the last diff ("diff") or the last edits result
        ("edits", which also gives the unit table); replaces the last map"""
        src = int(self.REBASE_SRCS.get(src, src))
        _check(self.L.crdt_rebase_async(self.h, src), "rebase_async")
        self._rb_n = getattr(self, "_ed_n" if src == 1 else "_diff_n", 0)

    def rebase_counts(self) -> np.ndarray:
        """spans per index of the map's source call; 0xFFFFFFFF marks an index without a result"""
        out = np.zeros(getattr(self, "_rb_n", 0), np.uint32)
        _check(self.L.crdt_rebase_counts(self.h, _p(out)), "rebase_counts")
        return out

    def rebase_read(self, i: int, kind="chars", counts=None) -> np.ndarray:
        """the spans of index i: [n_spans, 4] u32 = (old_at, old_len, new_at, new_len), in "chars" or
        in "units"; raises CrdtError (rc=-100) for an index without a result"""
        counts = counts if counts is not None else self.rebase_counts()
        bad = not 0 <= i < len(counts) or int(counts[i]) == 0xFFFFFFFF  # (the library answers CRDT_E_ARG)
        out = np.zeros((0 if bad else int(counts[i]), 4), np.uint32)
        _check(self.L.crdt_rebase_read(self.h, i, int(self.REBASE_KINDS.get(kind, kind)), out.ctypes.data if out.size else None),
               "rebase_read")
        return out

    def rebase(self, idx, x, kind="chars", dir="old_to_new", bias="right"):
        """(y, hit): position x[q] of index idx[q]'s old text mapped into its current text
        ("old_to_new") or back ("new_to_old"), in "chars" or "units"; bias "left" / "right" decides
        at an insertion and inside a replaced stretch, where hit is 1"""
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        p = np.ascontiguousarray(x, dtype=np.uint32)
        if i.shape != p.shape or i.ndim != 1:
            raise ValueError("rebase: idx and x are 1-d and of equal length")
        y, hit = np.zeros(p.shape[0], np.uint32), np.zeros(p.shape[0], np.uint8)
        _check(self.L.crdt_rebase(self.h, p.shape[0], _p(i), _p(p), int(self.REBASE_KINDS.get(kind, kind)),
                                  int(self.REBASE_DIRS.get(dir, dir)), int(self.BIASES.get(bias, bias)), _p(y),
                                  _p(hit, C.c_uint8)), "rebase")
        return y, hit

    def rebase_ms(self) -> float:
        """device time of the last rebase_async (HIP events)"""
        x = C.c_double()
        _check(self.L.crdt_last_rebase_ms(self.h, C.byref(x)), "last_rebase_ms")
        return x.value

    def timings(self):
        a, b = C.c_double(), C.c_double()
        self.L.crdt_last_timings(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def stream(self) -> int:
        return self.L.crdt_stream(self.h) or 0


class ListCRDT:
    """One document with the reference's method names (src/list/doc.rs), on its own engine."""

    def __init__(self, leaf_cap: int = 32, device: int = 0):
        self.e = Engine(1, leaf_cap, device)

    def get_or_create_agent_id(self, name: str) -> int:         # doc.rs:66
        return int(self.e.agent_intern([0], [name])[0])

    def apply_local_txn(self, agent: int, ops) -> int:          # doc.rs:376
        return int(self.e.apply_local([(0, [(agent, ops)])])[0])

    def local_insert(self, agent: int, pos: int, ins_len: int) -> int:   # doc.rs:472
        return self.apply_local_txn(agent, [(pos, 0, ins_len)])

    def local_delete(self, agent: int, pos: int, del_span: int) -> int:  # doc.rs:478
        return self.apply_local_txn(agent, [(pos, del_span, 0)])

    def apply_remote_wire(self, wire: bytes) -> int:            # doc.rs:242 (batch of RemoteTxn)
        return int(self.e.apply_remote_wire([0], [wire])[0])

    def set_content(self, content: np.ndarray):
        self.e.set_content([0], [0], [content])

    def to_string(self) -> str:                                 # doc.rs:498-505 (rope on)
        from .traces import utf32_to_str
        return utf32_to_str(self.e.text(0))

    def __len__(self) -> int:                                   # doc.rs:484
        return int(self.e.lens([0])[0])

    def version(self) -> int:                                   # get_next_order
        return int(self.e.versions([0])[0])

    def diff_since(self, v: int):
        """(patches [n, 4] u32 = (pos, del_len, ins_len, ins_off), ins_order, ins_text or None): what
        turns the text at version `v` (an earlier version()) into the current text"""
        return self.e.diff([0], [v])[0]

    def rebase_since(self, v: int, positions, dir: str = "old_to_new", bias: str = "right"):
        """(y, hit): char positions of the text at version `v` (an earlier version()) moved to where
        they stand in the current text, or back with dir "new_to_old" (Engine.rebase)"""
        self.e.diff([0], [v])
        self.e.rebase_async("diff")
        p = np.ascontiguousarray(positions, dtype=np.uint32)
        return self.e.rebase(np.zeros(p.shape[0], np.uint32), p, "chars", dir, bias)

    def diff_between(self, a: int, b: int):
        """diff_since's triple for what turns the text at version `a` into the text at version `b`
        (any two versions up to version(), in either order)"""
        return self.e.diff_between([0], [a], [b])[0]

    def edits_between(self, a: int, b: int, enc="utf8"):
        """(edits [n, 8] u32, ins np.uint8 | np.uint16): what turns the encoded text at version `a`
        into the encoded text at version `b` (Engine.edits_between; needs set_content)"""
        return self.e.edits_between([0], [a], [b], enc)[0]

    def rebase_between(self, a: int, b: int, positions, dir: str = "old_to_new", bias: str = "right"):
        """(y, hit): char positions of the text at version `a` moved to where they stand in the text
        at version `b`, or back with dir "new_to_old" (Engine.rebase)"""
        self.e.diff_between([0], [a], [b])
        self.e.rebase_async("diff")
        p = np.ascontiguousarray(positions, dtype=np.uint32)
        return self.e.rebase(np.zeros(p.shape[0], np.uint32), p, "chars", dir, bias)

    def text_at(self, v: int) -> np.ndarray:
        """the text (UTF-32 code points) at version `v` (an earlier version(); needs set_content)"""
        tx = self.e.checkout([0], [v])[0][1]
        if tx is None:
            raise CrdtError("text_at failed rc=-100: the document has no content (or too short a stream)")
        return tx

    def to_string_at(self, v: int) -> str:
        from .traces import utf32_to_str
        return utf32_to_str(self.text_at(v))

    def blame(self, mode: str = "agent") -> np.ndarray:
        """authorship runs [n, 4] u32 = (pos, len, agent, seq) of the current text (Engine.blame)"""
        return self.e.blame([0], mode)[0]

    def to_bytes(self) -> bytes:
        """the text as UTF-8 (what the reference's to_string holds, doc.rs:498-505), encoded on the device"""
        return self.e.encode([0], "utf8")[0]

    def len_utf16(self) -> int:
        """length of the text in UTF-16 code units"""
        self.e.encode_async([0], "utf16")
        n = int(self.e.encode_lens()[0][0])
        if n == 0xFFFFFFFF:
            raise CrdtError("len_utf16 failed rc=-100: a poisoned document, or one without content")
        return n

    def line_count(self, eol: str = "lf") -> int:
        """lines of the text (breaks + 1); eol "lf", or "any" for LF, CR LF and lone CR"""
        self.e.encode([0], "utf8")
        return int(self.e.lines(eol)[0].shape[0])

    def pos_to_linecol(self, pos: int, enc: str = "utf16", eol: str = "lf", col: str = "units"):
        """(line, col) of char `pos`; col in units of `enc` (an LSP Position with "utf16"), or in "chars" """
        self.e.encode([0], enc)
        self.e.lines_async(eol)
        ln, c = self.e.pos_to_linecol([0], [pos], col)
        return int(ln[0]), int(c[0])

    def linecol_to_pos(self, line: int, col: int, enc: str = "utf16", eol: str = "lf", kind: str = "units") -> int:
        """the char position of (line, col); 0xFFFFFFFF if there is no such line or column"""
        self.e.encode([0], enc)
        self.e.lines_async(eol)
        return int(self.e.linecol_to_pos([0], [line], [col], kind)[0][0])

    def find(self, pattern, enc: str = "utf16", icase: bool = False) -> np.ndarray:
        """every occurrence of `pattern` (a str or uint32 code points) in the text, overlapping ones
        included: [n, 2] u32 = (unit offset in `enc`, char position), ascending"""
        self.e.encode([0], enc)
        return self.e.find(pattern, icase)[0]

    def status(self) -> int:
        return int(self.e.status()[0])
