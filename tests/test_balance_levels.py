"""The rotation policy's level maps (csrc/balance_levels.h, DESIGN §4 "Progress balance") as a pure
function: a stand-alone host program around the header prints level(map, slice, wave id) for every
map, and the table is checked for what the balance relies on: a short period, every wave id at
every level for a quarter of it, map 0 the old formula bit for bit, and, for the other maps, no two
of a SIMD's eight wave ids tied at one level for more than half of the period (under map 0 ids w
and w + 4 are tied all the time, which is what the other maps are there to undo)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "text-crdt-rust_amd", "csrc")
SLICES = 256  # tabulated slices per map (several periods)
IDS = 16      # HW_ID.WAVE_ID is a four-bit field

PROGRAM = r"""
#include <cstdio>
#include "balance_levels.h"
static_assert(crdt::balance_level(0, 5, 6) == ((5u + 6u) & 3u), "usable in constant expressions");
int main() {
  std::printf("%u %u\n", crdt::BALANCE_MAPS, crdt::BALANCE_MAP_PERIOD);
  for (unsigned m = 0; m < crdt::BALANCE_MAPS + 1; m++)  // (one past the last: the fall-back)
    for (unsigned s = 0; s < SLICES; s++) {
      for (unsigned w = 0; w < IDS; w++) std::printf("%u ", crdt::balance_level(m, s, w));
      std::printf("\n");
    }
  // the slice is the real-time counter shifted down: any 32-bit value
  for (unsigned m = 0; m < crdt::BALANCE_MAPS; m++)
    for (unsigned s = 0xFFFFFF00u; s != 0x100u; s++)
      for (unsigned w = 0; w < IDS; w++)
        if (crdt::balance_level(m, s, w) > 3u) return 1;
  return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("balance_levels")
    src, exe = d / "levels.cpp", d / "levels"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-DSLICES={SLICES}", f"-DIDS={IDS}", "-I" + CSRC,
                    "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    maps, period = (int(x) for x in out[0].split())
    t = np.array([[int(x) for x in line.split()] for line in out[1:]], np.int64).reshape(maps + 1, SLICES, IDS)
    for m in range(maps):
        print(f"map {m}: rows = slices 0..{period - 1}, columns = wave ids 0..{IDS - 1}")
        for s in range(period):
            print("   ", " ".join(str(v) for v in t[m, s]))
    return maps, period, t


def period_of(tm):
    for p in range(1, SLICES // 2 + 1):
        if np.array_equal(tm[p:], tm[:-p]):
            return p
    return None


def test_maps_exist(table):
    maps, period, t = table
    assert maps >= 2 and period <= 64
    assert t.min() >= 0 and t.max() <= 3
    assert np.array_equal(t[maps], t[0])  # a map number past the last is map 0


def test_period_is_at_most_64_slices(table):
    maps, period, t = table
    for m in range(maps):
        p = period_of(t[m])
        assert p is not None and p <= 64 and period % p == 0, (m, p)


def test_every_wave_id_holds_every_level_a_quarter_of_the_period(table):
    maps, _, t = table
    for m in range(maps):
        p = period_of(t[m])
        assert p % 4 == 0, (m, p)
        for w in range(IDS):
            counts = np.bincount(t[m, :p, w], minlength=4)
            assert (counts == p // 4).all(), (m, w, counts)


def test_map_0_is_the_old_formula(table):
    _, _, t = table
    s, w = np.meshgrid(np.arange(SLICES), np.arange(IDS), indexing="ij")
    assert np.array_equal(t[0], (s + w) & 3)


def test_no_two_wave_ids_of_a_simd_stay_tied(table):
    maps, _, t = table
    # the defect: under map 0, w and w + 4 share a level in every slice
    assert all((t[0, :, w] == t[0, :, w + 4]).all() for w in range(4))
    for m in range(1, maps):
        p = period_of(t[m])
        for a in range(8):
            for b in range(a + 1, 8):
                shared = int((t[m, :p, a] == t[m, :p, b]).sum())
                assert 2 * shared <= p, (m, a, b, shared, p)
