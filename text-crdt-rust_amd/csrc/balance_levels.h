// The rotation policy's level map (kernels.h balance_board_tick, BAL_ROTATE): which of the four
// s_setprio levels a wave holds in a time slice, as a pure function of (map, slice, HW_ID.WAVE_ID),
// so the same text runs in the kernel (on SGPRs) and in a host program that tabulates it
// (tests/test_balance_levels.py).
//
// A SIMD holds up to eight replay waves (wave ids 0..7 where all are resident) and has four levels,
// so waves tie; the issue arbiter breaks a tie by age, and on this workload the older wave of a
// tie is always the one with the lower wave id (profiles/wave_lifetimes_by_id_parent.txt, DESIGN
// §5).  A map is up to four partitions of the eight ids into four groups ("types", each held for
// four slices, in turn); within a type the levels rotate over the groups, level = (group + slice)
// & 3, so every id holds every level for exactly a quarter of the time under any map.  What a map
// chooses is who ties with whom.  A wave's mean place in its SIMD's order (level first, then age)
// is (8 - s) / 2 + p for a group of s waves of which p are older, and the waves end in that order:
//   0  groups {w, w + 4}: level = (slice + id) & 3, as before the maps.  The same wave of each pair
//      wins every tie for the whole launch: ids 0..3 have mean place 3.0, ids 4..7 4.0.  With four
//      waves per SIMD (ids 0..3) the levels are distinct.
//   1  changing partners: pairs {0,1}{2,3}{4,5}{6,7}, then {7,0}{1,2}{3,4}{5,6}.  Ids 1..6 win one
//      tie and lose the other (3.5); id 0 wins both (3.0), id 7 loses both (4.0).
//   2  uneven groups: {0,1}{2,3}{4,5,6}{7}, then {0}{1,2,4}{3,5}{6,7}: mean places 3.25 .. 3.75, the
//      narrowest range two partitions reach with no two ids together in both (no map can make
//      them equal: id 0 is the older wave of every tie it is in, id 7 the younger).
// Map 2 is the default (0.8 ms off the 59 ms step of 8,192 automerge-paper documents).
// The kernel reads the map's table (balance_table, made on the host) from its arguments: choosing
// the map by its number at the tick, some 4,000 times per document, cost 0.3 ms per step.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BAL_LEVEL_FN __host__ __device__ constexpr
#else
#define BAL_LEVEL_FN constexpr
#endif

namespace crdt {

constexpr uint32_t BALANCE_MAPS = 3;         // maps 0 .. BALANCE_MAPS - 1
constexpr uint32_t BALANCE_MAP_PERIOD = 16;  // every map repeats after this many slices (or a divisor of it)

// one type: the group (0..3) of ids 0..7, two bits each
BAL_LEVEL_FN uint64_t balance_groups(uint32_t g0, uint32_t g1, uint32_t g2, uint32_t g3, uint32_t g4, uint32_t g5,
                                     uint32_t g6, uint32_t g7) {
  return (uint64_t)(g0 | g1 << 2 | g2 << 4 | g3 << 6 | g4 << 8 | g5 << 10 | g6 << 12 | g7 << 14);
}
// a map's table: type t (slices 4t .. 4t + 3 of the period) in bits 16t .. 16t + 15
BAL_LEVEL_FN uint64_t balance_types(uint64_t a, uint64_t b) { return a | b << 16 | a << 32 | b << 48; }
BAL_LEVEL_FN uint64_t balance_table(uint32_t map) {
  return map == 1u   ? balance_types(balance_groups(0, 0, 1, 1, 2, 2, 3, 3), balance_groups(0, 1, 1, 2, 2, 3, 3, 0))
         : map == 2u ? balance_types(balance_groups(0, 0, 1, 1, 2, 2, 2, 3), balance_groups(0, 1, 1, 2, 1, 2, 3, 3))
                     : balance_types(balance_groups(0, 1, 2, 3, 0, 1, 2, 3), balance_groups(0, 1, 2, 3, 0, 1, 2, 3));
}
// (only bits 0-2 of wave_id count; map 0's groups are id & 3, so there the id may as well be whole)
BAL_LEVEL_FN uint32_t balance_level_in(uint64_t table, uint32_t slice, uint32_t wave_id) {
  return ((uint32_t)(table >> ((slice & 12u) * 4u + (wave_id & 7u) * 2u)) + slice) & 3u;
}
BAL_LEVEL_FN uint32_t balance_level(uint32_t map, uint32_t slice, uint32_t wave_id) {
  return balance_level_in(balance_table(map), slice, wave_id);
}

}  // namespace crdt
