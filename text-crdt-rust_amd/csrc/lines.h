// Line index of the encoded text (crdt_lines_async and its queries, include/crdt_gpu.h): for every
// index of the last encode a table of line starts {unit offset, char position}, and the two
// mappings char position <-> (line, column).  Reads nothing but the encode result (the packed unit
// pool, its per-index results and its samples); the queries read nothing but that and the table.
//
// A break follows every LF unit (EOL_LF), or every LF and every CR whose next unit in the same
// document is not LF (EOL_ANY).  Both are one-unit chars in either encoding, so a break is found by
// per-unit compares on the pool's dwords: a UTF-8 continuation byte is never 0x0A / 0x0D, and a
// UTF-16 unit is compared whole (U+0A0A, U+010A, U+0D0A are no breaks).
//
// The sweeps take a document's aligned pool dwords (4 bytes or 2 u16 each) LN_PASS = 1,024 per loop
// pass: a wave takes 256 consecutive dwords as LN_ROWS = 4 rows of 64, lane l dword l of the row.
// In units a row is 256 / 128, a wave's share 1,024 / 512 and a pass 4,096 / 2,048 (UTF-8 / UTF-16).
// The pool is packed: the first and the last dword of a document are shared with its neighbours,
// and every flag is masked to the document's own units.
#pragma once
#include "encode.h"

namespace crdt {

constexpr u32 EOL_LF = 0u, EOL_ANY = 1u;        // CRDT_EOL_*
constexpr u32 COL_UNITS = 0u, COL_CHARS = 1u;   // CRDT_COL_*
#define LN_T 256u      // threads per index
#define LN_WAVES 4u
#define LN_ROWS 4u     // rows of 64 dwords a wave takes per loop pass
#define LN_PASS 1024u  // dwords per loop pass (LN_WAVES * LN_ROWS * 64)

struct LineStart {
  u32 unit, pos;  // the line's first unit and first char, in the document
};
struct LnRes {
  u32 n_lines;  // INVALID: no result for this index
  u32 pad_;
  u64 off;      // first entry of this index in the table (k_result_scan); it has n_lines + 1 entries
};
struct LnIO {
  LnRes* res;      // [i]
  LineStart* tab;  // [res[i].off + k]: line k's start, and at k = n_lines the sentinel {units, chars}
};

// One bit per unit of dword x, at bit 8 j / 16 j for unit j (as enc_starts): the unit equals c.
// Exact per field: (y & LOW) + LOW carries into the field's top bit iff its low bits are not 0,
// and never out of the field.
template <u32 ENC>
__device__ __forceinline__ u32 ln_eq(u32 x, u32 c) {
  constexpr u32 LOW = ENC == ENC_UTF8 ? 0x7F7F7F7Fu : 0x7FFF7FFFu;
  constexpr u32 REP = ENC == ENC_UTF8 ? 0x01010101u : 0x00010001u;
  constexpr u32 SH = ENC == ENC_UTF8 ? 8u : 16u;
  u32 y = x ^ (c * REP);
  return ~(((y & LOW) + LOW) | y | LOW) >> (SH - 1u);
}

// A document's place in the pool: its dwords are words[0 .. nw), its first unit is unit `head` of
// words[0], and `endu` = head + units (the document's end, in units from words[0]).
struct LnDoc {
  const u32* words;
  u32 nw, head;
  u64 endu;
};
template <u32 ENC>
__device__ __forceinline__ LnDoc ln_doc(const EncIO& E, const EncRes& rs) {
  constexpr u32 UPD = ENC == ENC_UTF8 ? 4u : 2u;  // units per dword
  LnDoc D;
  D.words = (const u32*)E.units + rs.off / UPD;
  D.head = (u32)(rs.off % UPD);
  D.endu = (u64)D.head + rs.units;
  D.nw = rs.units ? (u32)((D.endu + UPD - 1u) / UPD) : 0u;
  return D;
}

// The flags of a wave's LN_ROWS rows of a pass -- lane l of row j holds dword kw + 64 j + l of the
// document (at or past nw: none) -- one bit per unit as ln_eq, masked to the document's units:
// brk = a break follows the unit, st = the unit starts a char.  The LF lookahead of a dword's last
// unit is the first unit of the next dword: the next lane's, which every lane picks out of one
// ballot of the row; the row's last lane takes the next row's lane 0 (bit 0 of that row's ballot),
// and the last row's the dword after the wave's share, which every lane loads (one address) with
// the rows.  A unit past the document's end reads as "not LF", whatever the neighbour document
// starts with.  Called by whole waves.
template <u32 ENC, u32 EOL>
__device__ __forceinline__ void ln_flags(const LnDoc& D, u32 kw, u32 l, u32 (&brk)[LN_ROWS], u32 (&st)[LN_ROWS]) {
  constexpr u32 UPD = ENC == ENC_UTF8 ? 4u : 2u;
  constexpr u32 SH = ENC == ENC_UTF8 ? 8u : 16u;
  constexpr u32 REP = ENC == ENC_UTF8 ? 0x01010101u : 0x00010001u;
  u32 x[LN_ROWS], m[LN_ROWS];
#pragma unroll
  for (u32 j = 0; j < LN_ROWS; j++) {
    u32 k = kw + j * 64u + l;
    bool in = k < D.nw;
    x[j] = in ? D.words[k] : 0u;
    u32 a = k == 0u ? D.head : 0u;
    u32 b = (u32)min((u64)UPD, D.endu - (u64)k * UPD) - 1u;  // (in: endu - k UPD >= 1)
    m[j] = in ? enc_range<ENC>(a, b) & REP : 0u;
  }
  u32 xn = 0u;
  if (EOL == EOL_ANY) {
    u32 kn = kw + LN_ROWS * 64u;
    xn = kn < D.nw ? D.words[kn] : 0u;  // (unit 0 of a dword 0 < kn < nw is the document's)
  }
#pragma unroll
  for (u32 j = 0; j < LN_ROWS; j++) {
    st[j] = enc_starts<ENC>(x[j]) & m[j];
    brk[j] = ln_eq<ENC>(x[j], 0x0Au) & m[j];
  }
  if (EOL == EOL_ANY) {
    u64 nxt = uni(ln_eq<ENC>(xn, 0x0Au) & 1u);  // the first unit after the row is an LF of this document
#pragma unroll
    for (u32 j = LN_ROWS; j-- > 0u;) {
      u32 lf = brk[j];
      u64 first = ballot((lf & 1u) != 0u);                        // bit l: lane l's first unit is one
      u32 nf = (u32)(((first >> 1) | (nxt << 63)) >> l) & 1u;     // ... and lane l + 1's (the next row's lane 0)
      u32 nlf = (lf >> SH) | (nf << (32u - SH));                  // bit of unit j: unit j + 1 is one
      brk[j] = lf | (ln_eq<ENC>(x[j], 0x0Du) & m[j] & ~nlf);
      nxt = first & 1ull;
    }
  }
}

// First sweep.  One block of LN_WAVES waves per index of the encode: counts the breaks of its
// units; n_lines = breaks + 1.  An index without an encode result has none here.
template <u32 ENC, u32 EOL>
__global__ __launch_bounds__(LN_T) void k_ln_count(EncIO E, LnIO Lo, u32 n) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  EncRes rs = E.res[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  if (rs.units == INVALID) {
    if (tid == 0) Lo.res[i] = LnRes{INVALID, 0u, 0ull};
    return;
  }
  LnDoc D = ln_doc<ENC>(E, rs);
  u32 wq = wv * (LN_ROWS * 64u);  // this wave's first dword in a pass
  u32 cnt = 0u;
  for (u32 k0 = 0; k0 < D.nw; k0 += LN_PASS) {
    u32 brk[LN_ROWS], st[LN_ROWS];
    ln_flags<ENC, EOL>(D, k0 + wq, l, brk, st);
#pragma unroll
    for (u32 j = 0; j < LN_ROWS; j++) cnt += (u32)__popc(brk[j]);
  }
  __shared__ u32 s_c[LN_WAVES];
  u32 t = wave_sum(cnt);
  if (l == 0u) s_c[wv] = t;
  __syncthreads();
  if (tid == 0) Lo.res[i] = LnRes{s_c[0] + s_c[1] + s_c[2] + s_c[3] + 1u, 0u, 0ull};
}

// k_result_scan's view of an LnRes: its table entries (n_lines + 1: the sentinel; an index without
// a result counts as 0)
__device__ __forceinline__ void scan_counts(const LnRes& r, u64* c) { c[0] = r.n_lines == INVALID ? 0ull : (u64)r.n_lines + 1ull; }
__device__ __forceinline__ void scan_store(LnRes& r, const u64* off) { r.off = off[0]; }

// Second sweep, after k_result_scan: the same passes and rows.  Two running counts are carried from
// pass to pass in registers (every thread folds the same LDS values, as k_enc_count carries its
// units): the breaks so far (the line number) and the char starts so far (the char position).
// A dword has at most 4 of each and a pass at most 4,096, so both ride one wave scan per row as a
// packed pair (breaks in the low, starts in the high 16 bits); the waves' totals meet in LDS, in
// two rows that alternate from pass to pass (one barrier per pass, as in k_enc_count).  The break
// at unit u, the r-th of the document, writes entry r = {u + 1, char starts in [0, u]}; thread 0
// writes entry 0 = {0, 0} and the sentinel {units, chars}.  (r < n_lines by construction: the count
// sweep read the same units on the same stream.)
template <u32 ENC, u32 EOL>
__global__ __launch_bounds__(LN_T) void k_ln_write(EncIO E, LnIO Lo, u32 n) {
  constexpr u32 UPD = ENC == ENC_UTF8 ? 4u : 2u;
  constexpr u32 SH = ENC == ENC_UTF8 ? 8u : 16u;
  u32 i = blockIdx.x;
  if (i >= n) return;
  LnRes lr = Lo.res[i];
  if (lr.n_lines == INVALID) return;
  EncRes rs = E.res[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  LineStart* tab = Lo.tab + lr.off;
  if (tid == 0) {
    tab[0] = LineStart{0u, 0u};
    tab[lr.n_lines] = LineStart{rs.units, rs.chars};
  }
  LnDoc D = ln_doc<ENC>(E, rs);
  __shared__ u32 s_w[2][LN_WAVES];
  u32 wq = wv * (LN_ROWS * 64u);
  u32 run_b = 0u, run_s = 0u;  // carried: breaks and char starts of the passes before this one
  for (u32 k0 = 0, row = 0; k0 < D.nw; k0 += LN_PASS, row ^= 1u) {
    u32 brk[LN_ROWS], st[LN_ROWS], v[LN_ROWS], inc[LN_ROWS], tot[LN_ROWS];
    ln_flags<ENC, EOL>(D, k0 + wq, l, brk, st);
#pragma unroll
    for (u32 j = 0; j < LN_ROWS; j++) v[j] = (u32)__popc(brk[j]) | ((u32)__popc(st[j]) << 16);
#pragma unroll
    for (u32 j = 0; j < LN_ROWS; j++) {
      inc[j] = wave_incl_scan(v[j]);
      tot[j] = rdlane(inc[j], 63);
    }
    if (l == 0u) s_w[row][wv] = tot[0] + tot[1] + tot[2] + tot[3];
    __syncthreads();
    u32 base = 0u, all = 0u;  // packed: the waves before this one, and the whole pass
    for (u32 x = 0; x < LN_WAVES; x++) {
      u32 w = s_w[row][x];
      base += x < wv ? w : 0u;
      all += w;
    }
#pragma unroll
    for (u32 j = 0; j < LN_ROWS; j++) {
      u32 ex = base + inc[j] - v[j];  // this dword's exclusive pair, in the pass
      base += tot[j];
      u32 r = run_b + (ex & 0xFFFFu), cs = run_s + (ex >> 16);
      u32 k = k0 + wq + j * 64u + l;
      u32 b = brk[j];
      while (b) {
        u32 jj = (u32)__builtin_ctz(b) / SH;  // the break's unit in the dword
        r++;
        u32 u = k * UPD + jj - D.head;        // ... and in the document
        if (r < lr.n_lines) tab[r] = LineStart{u + 1u, cs + (u32)__popc(st[j] & enc_range<ENC>(0u, jj))};
        b &= b - 1u;
      }
    }
    run_b += all & 0xFFFFu;
    run_s += all >> 16;
  }
}

// The two walks of k_pos_to_units / k_units_to_pos (encode.h), as device functions.
// units before char p of index i, for p <= rs.chars
template <u32 ENC>
__device__ __forceinline__ u32 ln_pos_to_units(const EncIO& E, const EncRes& rs, u32 i, u32 p) {
  constexpr u32 UPD = ENC == ENC_UTF8 ? 4u : 2u;
  constexpr u32 SH = ENC == ENC_UTF8 ? 8u : 16u;
  const u32* words = (const u32*)E.units;
  if (p == rs.chars) return rs.units;
  u32 r = p & (ENC_S - 1u);
  u32 s = E.samples[E.sp_base[i] + (p >> ENC_S_LOG)];
  if (!r) return s;
  u32 ans = rs.units;  // (never left standing: char p < chars starts inside the document)
  u64 g0 = rs.off + s;
  u64 w0 = g0 / UPD, w1 = (rs.off + rs.units - 1u) / UPD;
  u32 cnt = 0u;  // char starts seen, the sample's own included: the answer is start number r
  for (u64 w = w0; w <= w1; w++) {
    u32 st = enc_starts<ENC>(words[w]);
    if (w == w0) st &= enc_range<ENC>((u32)(g0 % UPD), UPD - 1u);
    u32 k = (u32)__popc(st);
    if (cnt + k > r) {
      for (u32 x = cnt; x < r; x++) st &= st - 1u;  // drop the starts before number r
      u64 g = w * UPD + ((u32)__builtin_ctz(st) / SH);
      ans = (u32)(g - rs.off);
      break;
    }
    cnt += k;
  }
  return ans;
}
// the char of index i whose encoding covers unit u, for u <= rs.units; mid = u is not its first unit
template <u32 ENC>
__device__ __forceinline__ u32 ln_units_to_pos(const EncIO& E, const EncRes& rs, u32 i, u32 u, u32& mid) {
  constexpr u32 UPD = ENC == ENC_UTF8 ? 4u : 2u;
  constexpr u32 SH = ENC == ENC_UTF8 ? 8u : 16u;
  const u32* words = (const u32*)E.units;
  mid = 0u;
  if (u == rs.units) return rs.chars;
  const u32* smp = E.samples + E.sp_base[i];
  u32 lo = 0u, hi = (rs.chars >> ENC_S_LOG) + 1u;  // smp[lo] <= u < smp[hi] (hi may be the end)
  while (hi - lo > 1u) {
    u32 md = (lo + hi) >> 1;
    if (smp[md] <= u) lo = md; else hi = md;
  }
  u64 g0 = rs.off + smp[lo], g1 = rs.off + u;
  u64 w0 = g0 / UPD, w1 = g1 / UPD;
  u32 cnt = 0u, st = 0u;
  for (u64 w = w0; w <= w1; w++) {
    st = enc_starts<ENC>(words[w]);
    u32 a = w == w0 ? (u32)(g0 % UPD) : 0u, b = w == w1 ? (u32)(g1 % UPD) : UPD - 1u;
    cnt += (u32)__popc(st & enc_range<ENC>(a, b));
  }
  mid = ((st >> ((u32)(g1 % UPD) * SH)) & 1u) ^ 1u;
  return (lo << ENC_S_LOG) + cnt - 1u;
}

// pos -> (line, col).  One thread per query (grid stride).  A binary search over the index's line
// starts finds the last line that starts at or before pos; the column is the distance from that
// start in chars (COL_CHARS: the table alone) or in units (COL_UNITS: the sample walk).  idx out of
// range or without a result, or pos above the document's chars: INVALID for both.
template <u32 ENC>
__global__ __launch_bounds__(256) void k_pos_to_linecol(EncIO E, LnIO Lo, u32 n_idx, u64 nq, const u32* idx, const u32* pos,
                                                        u32 kind, u32* line, u32* col) {
  for (u64 q = (u64)blockIdx.x * 256u + threadIdx.x; q < nq; q += (u64)gridDim.x * 256u) {
    u32 i = idx[q], p = pos[q];
    u32 ln = INVALID, c = INVALID;
    if (i < n_idx) {
      EncRes rs = E.res[i];
      LnRes lr = Lo.res[i];
      if (rs.units != INVALID && lr.n_lines != INVALID && p <= rs.chars) {
        const LineStart* tab = Lo.tab + lr.off;
        u32 lo = 0u, hi = lr.n_lines;  // tab[lo].pos <= p, and p < tab[hi].pos or hi = n_lines
        while (hi - lo > 1u) {
          u32 md = (lo + hi) >> 1;
          if (tab[md].pos <= p) lo = md; else hi = md;
        }
        LineStart s = tab[lo];
        ln = lo;
        c = kind == COL_CHARS ? p - s.pos : ln_pos_to_units<ENC>(E, rs, i, p) - s.unit;
      }
    }
    line[q] = ln;
    col[q] = c;
  }
}

// (line, col) -> pos.  One thread per query (grid stride).  The line's extent is the distance to
// the next entry (the sentinel after the last line); a column inside it -- or at its end, on the
// last line -- is valid.  COL_UNITS: the char that covers unit start + col, with mid = 1 if the
// column falls inside it.  Anything else: INVALID, mid 0.
template <u32 ENC>
__global__ __launch_bounds__(256) void k_linecol_to_pos(EncIO E, LnIO Lo, u32 n_idx, u64 nq, const u32* idx, const u32* line,
                                                        const u32* col, u32 kind, u32* pos, u8* mid) {
  for (u64 q = (u64)blockIdx.x * 256u + threadIdx.x; q < nq; q += (u64)gridDim.x * 256u) {
    u32 i = idx[q], ln = line[q], c = col[q];
    u32 ans = INVALID, m = 0u;
    if (i < n_idx) {
      EncRes rs = E.res[i];
      LnRes lr = Lo.res[i];
      if (rs.units != INVALID && lr.n_lines != INVALID && ln < lr.n_lines) {
        const LineStart* tab = Lo.tab + lr.off;
        LineStart s = tab[ln], e = tab[ln + 1u];
        bool last = ln + 1u == lr.n_lines;
        u32 ext = kind == COL_CHARS ? e.pos - s.pos : e.unit - s.unit;
        if (c < ext || (last && c == ext)) {
          if (kind == COL_CHARS) ans = s.pos + c;
          else ans = ln_units_to_pos<ENC>(E, rs, i, s.unit + c, m);
        }
      }
    }
    pos[q] = ans;
    if (mid) mid[q] = (u8)m;
  }
}

}  // namespace crdt
