// Position mapping between a past version and the current text (crdt_rebase_async and its queries,
// include/crdt_gpu.h).  A diff or edits result is a sorted patch list per index; what a caller that
// holds cursors, selections or diagnostics in the old text needs on top of it is where every patch
// starts in the old text -- a prefix sum of ins - del over the earlier patches -- and a batched
// search over the result.  k_rebase_build copies a source result into span tables
//   {old_at, old_len, new_at, new_len}
// in chars and, from an edits source, in that call's units; k_rebase answers
// (idx, x, kind, dir, bias) queries on them.  The map is a copy: the kernels of the queries read
// nothing but the span tables and their per-index results.
//
// Spans are ascending on both sides and neighbours are at least one kept item apart (a patch is a
// maximal run of deleted and inserted items), so "the last span that starts at or before x" is
// one binary search on either side and the rule below is a function of that span alone.
#pragma once
#include "edits.h"

namespace crdt {

constexpr u32 RB_FROM_DIFF = 0u, RB_FROM_EDITS = 1u;  // CRDT_REBASE_FROM_*
constexpr u32 RB_CHARS = 0u, RB_UNITS = 1u;            // CRDT_REBASE_CHARS / _UNITS
constexpr u32 RB_OLD_TO_NEW = 0u, RB_NEW_TO_OLD = 1u;  // CRDT_REBASE_OLD_TO_NEW / _NEW_TO_OLD
constexpr u32 RB_LEFT = 0u, RB_RIGHT = 1u;             // CRDT_BIAS_*
#define RB_T 256u  // threads per index: k_rebase_build takes RB_T patches per loop pass
#define RB_WAVES 4u

struct alignas(16) RbSpan { u32 old_at, old_len, new_at, new_len; };  // crdt_rebase_span (include/crdt_gpu.h)
struct RbRes {
  u32 n_spans;  // INVALID: the source has no result for this index
  u32 pad_;
  u64 off;      // first span of this index in both tables: the source's poff / eoff
};
struct RbIO {
  RbRes* res;   // [i]
  RbSpan* ch;   // [res[i].off + p]: span p in chars
  RbSpan* un;   // ... in units (an edits source only)
  u64 cap;      // entries of each table: the source's total, which every store stays below
};

// what k_rebase_build reads of a source: the index's count, offset and "no result", and patch p's
// char columns and (an edits source) unit columns
struct RbDiffSrc {
  const DiffRes* res;
  const Patch* pat;
  static constexpr bool UNITS = false;
  __device__ __forceinline__ bool head(u32 i, u32& m, u64& off) const {
    DiffRes r = res[i];
    m = r.n_pat;
    off = r.poff;
    return (r.flags & DIFF_BAD) == 0u;
  }
  __device__ __forceinline__ void load(u64 at, uint4& c, uint4& u) const {
    c = *(const uint4*)(pat + at);  // pos, del_len, ins_len, ins_off
    u = make_uint4(0u, 0u, 0u, 0u);
  }
};
struct RbEditSrc {
  const EdRes* res;
  const Edit* ed;
  static constexpr bool UNITS = true;
  __device__ __forceinline__ bool head(u32 i, u32& m, u64& off) const {
    EdRes r = res[i];
    m = r.n_ed;
    off = r.eoff;
    return (r.flags & ED_BAD) == 0u;
  }
  __device__ __forceinline__ void load(u64 at, uint4& c, uint4& u) const {
    const uint4* p = (const uint4*)(ed + at);
    c = p[0];                      // pos, del_len, ins_len, unit
    uint4 t = p[1];                // del_units, ins_units, ins_off, reserved
    u = make_uint4(c.w, t.x, t.y, 0u);  // unit, del_units, ins_units
  }
};

// One block of RB_WAVES waves per index of the source, RB_T patches per loop pass.  Patch p's span
// is {pos - S, del, pos, ins} with S = the sum of ins - del over the patches before it (mod 2^32:
// the result lies in the old text): one wave scan of the deltas per table, the waves' totals meet
// in LDS, and the running sums carry from pass to pass in registers (every thread folds the same
// LDS totals, as k_diff does).  The spans go to the source's own per-index offset, so the tables
// need no offsets scan; every store stays below the source's totals (cap).
template <class Src>
__global__ __launch_bounds__(RB_T) void k_rebase_build(Src S, RbIO R, u32 n) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  u32 m;
  u64 off;
  bool ok = S.head(i, m, off);
  if (tid == 0) R.res[i] = RbRes{ok ? m : INVALID, 0u, ok ? off : 0ull};
  if (!ok) return;
  __shared__ u32 s_t[2][RB_WAVES];
  u32 r_c = 0, r_u = 0;  // carried: ins - del of the passes before this one, in chars and in units
  for (u32 p0 = 0; p0 < m; p0 += RB_T) {
    u32 p = p0 + tid;
    bool in = p < m && off + p < R.cap;
    uint4 c = make_uint4(0u, 0u, 0u, 0u), u = c;
    if (in) S.load(off + p, c, u);
    u32 dc = c.z - c.y, du = u.z - u.y;
    u32 Ic = wave_incl_scan(dc), Iu = Src::UNITS ? wave_incl_scan(du) : 0u;
    if (l == 63u) {
      s_t[0][wv] = Ic;
      s_t[1][wv] = Iu;
    }
    __syncthreads();
    u32 b_c = r_c, b_u = r_u;
    for (u32 w = 0; w < RB_WAVES; w++) {
      u32 tc = s_t[0][w], tu = s_t[1][w];
      b_c += w < wv ? tc : 0u;
      b_u += w < wv ? tu : 0u;
      r_c += tc;
      r_u += tu;
    }
    if (in) {
      *(uint4*)(R.ch + off + p) = make_uint4(c.x - (b_c + Ic - dc), c.y, c.x, c.z);
      if (Src::UNITS) *(uint4*)(R.un + off + p) = make_uint4(u.x - (b_u + Iu - du), u.y, u.x, u.z);
    }
    __syncthreads();  // (the next pass rewrites the LDS totals)
  }
}

// The mapping rule (ProseMirror's StepMap.map), on the span (a, la, b, lb) read from the query's
// source side: the last span with a <= x.
//   none                 y = x
//   x > a + la           y = x - (a + la) + (b + lb)
//   otherwise            y = b (side < 0) or b + lb; side = bias when la == 0, else -1 at x == a,
//                        +1 at x == a + la, bias strictly inside; hit = a < x < a + la
// One thread per query (grid stride): a binary search over the index's spans by their start on the
// source side.  DIR picks the columns at compile time and bias is a scalar argument, so a wave
// takes no per-lane branch on either.  x is not checked against a text's length; the arithmetic is
// mod 2^32 (x >= a in every branch, so x - a does not wrap).  An idx out of range, or an index
// without a result, is answered INVALID with hit = 0.
template <u32 DIR>
__global__ __launch_bounds__(256) void k_rebase(const RbRes* res, const RbSpan* tab, u32 n_idx, u64 nq, const u32* idx,
                                               const u32* xs, u32 bias, u32* y, u8* hit) {
  for (u64 q = (u64)blockIdx.x * 256u + threadIdx.x; q < nq; q += (u64)gridDim.x * 256u) {
    u32 i = idx[q], x = xs[q];
    u32 ans = INVALID, h = 0u;
    if (i < n_idx) {
      RbRes rs = res[i];
      if (rs.n_spans != INVALID) {
        const RbSpan* t = tab + rs.off;
        u32 lo = 0u, hi = rs.n_spans;  // the first span that starts past x is in [lo, hi]
        while (lo < hi) {
          u32 md = lo + ((hi - lo) >> 1);
          u32 a = DIR == RB_OLD_TO_NEW ? t[md].old_at : t[md].new_at;
          if (a <= x) lo = md + 1u; else hi = md;
        }
        ans = x;
        if (lo) {
          uint4 s = *(const uint4*)(t + (lo - 1u));
          u32 a = DIR == RB_OLD_TO_NEW ? s.x : s.z, la = DIR == RB_OLD_TO_NEW ? s.y : s.w;
          u32 b = DIR == RB_OLD_TO_NEW ? s.z : s.x, lb = DIR == RB_OLD_TO_NEW ? s.w : s.y;
          u32 dx = x - a;
          if (dx > la) {
            ans = dx - la + b + lb;
          } else {
            bool right = (la == 0u || (dx != 0u && dx != la)) ? bias == RB_RIGHT : dx != 0u;
            ans = right ? b + lb : b;
            h = dx != 0u && dx != la ? 1u : 0u;
          }
        }
      }
    }
    y[q] = ans;
    if (hit) hit[q] = (u8)h;
  }
}

}  // namespace crdt
