"""The kernels' size thresholds, read from the sources -- TEST INFRASTRUCTURE.

`#define NAME <int>u?` and `constexpr u32 NAME = <int>` in csrc/kernels.h and csrc/crdt_types.h, so
that the tests that sit on a threshold move with the code."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "text-crdt-rust_amd", "csrc")
NAMES = ("PUB_BIG_MIN", "PUB_BIG_FEW_DOCS", "PUB_BIG_MAX", "PUB_BIG_WAVES", "PUBX_MAX_WORDS", "QBLK_MAX", "QBLK_CWO",
         "QBLK_W", "QBLK_Q", "QM_TILE", "GROUP")


def kernel_consts() -> dict:
    src = "".join(open(os.path.join(CSRC, f)).read() for f in ("kernels.h", "crdt_types.h"))
    out = {}
    for name in NAMES:
        m = re.search(r"^\s*(?:#define\s+%s\s+|constexpr\s+u32\s+%s\s*=\s*)(\d+)u?\b" % (name, name), src, re.M)
        if not m:
            raise KeyError(f"{name}: no integer #define / constexpr u32 in csrc/kernels.h or csrc/crdt_types.h")
        out[name] = int(m.group(1))
    return out


globals().update(kernel_consts())
