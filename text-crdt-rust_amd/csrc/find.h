// Literal text search on the encoded text (crdt_find_async and its queries, include/crdt_gpu.h):
// for every index of the last encode the table of all matches {unit offset, char position} of one
// pattern, overlapping ones included, in ascending order, and the seek "first match at or after /
// last match at or before a char position".  Reads nothing but the encode result (the packed unit
// pool and its per-index results); the seek reads nothing but the match table.
//
// Why comparing units finds exactly the char-level matches.  The host sanitises the pattern's code
// points as the encoder sanitises content (no scalar value -> U+FFFD), folds them when asked, and
// encodes them with the encoder's rule into the encode's units; the kernels compare units.
//  - Encoding is injective on scalar values, and the units of a char never are a prefix of another
//    char's, so equal unit strings that both start at a char boundary are equal char strings.
//  - A UTF-8 pattern starts with a non-continuation byte and a UTF-16 pattern never starts with a
//    low surrogate, so a unit-level occurrence starts where a char starts; it then runs over whole
//    chars of the text for as long as the pattern's chars last, and ends where a char ends.
//  - So a unit-level occurrence that lies inside the document -- u >= 0 and u + m_units <= units in
//    the document's own units -- is exactly a char-level match, and every char-level match is one.
//    The masks below rest on this: a candidate is a unit, inside the document, that equals the
//    pattern's first unit, and no char-start test is made on it.
//  - CRDT_FIND_ASCII_ICASE: fold(c) = c + 0x20 for 0x41 <= c <= 0x5A.  A unit folds iff it lies in
//    0x41..0x5A.  In UTF-8 such a byte is always a whole ASCII char (lead and continuation bytes
//    are >= 0x80); in UTF-16 the unit is folded whole, so 0x0041 folds and 0x0141 / 0x4100 do not,
//    and a surrogate never lies in the range.  Folded text against the folded pattern is the
//    definition; folding changes no bit that enc_starts reads.
//
// The sweeps are the line index's (lines.h): a document's aligned pool dwords FD_PASS = 1,024 per
// loop pass, a wave 256 of them as 4 coalesced rows of 64.  A match that starts in a lane's dword
// runs up to m_units - 1 units further (at most 255 B / 127 u16): into later lanes, rows, waves
// and the next pass.  So a pass's dwords go to LDS (folded when asked) with a halo of FD_HALO = 64
// dwords after them, and a candidate is verified against that window a dword at a time, the
// window's dwords funnel-shifted to the candidate's unit phase.  (A pattern has at most 64 dwords;
// the last window dword a candidate at dword w reads is w + 64.)  The pool is packed, so the dwords
// after a document's last are the next document's: they are never loaded -- the window holds 0
// there -- and a match is bounded by the length test above, not by what the window contains: the
// document's last dword is shared with its neighbour.  No dword at or past nw is read, so none past
// the pool's end is.
//
// The pattern's dwords are staged in LDS from a small device buffer (a runtime-indexed array in a
// by-value kernel argument would land in scratch).
#pragma once
#include "lines.h"

namespace crdt {

constexpr u32 FIND_ICASE = 1u;   // CRDT_FIND_ASCII_ICASE
constexpr u32 SEEK_NEXT = 0u, SEEK_PREV = 1u;  // CRDT_SEEK_*
#define FD_MAX_CHARS 64u  // CRDT_FIND_MAX_CHARS
#define FD_PAT_W 64u      // dwords of the longest pattern (64 chars of 4 B / of 2 u16)
#define FD_HALO 64u       // dwords staged after a pass
#define FD_WIN (LN_PASS + FD_HALO)

struct Match {
  u32 unit, pos;  // the match's first unit and first char, in the document
};
struct FdRes {
  u32 n_matches;  // INVALID: no result for this index
  u32 pad_;
  u64 off;        // first entry of this index in the table (k_result_scan)
};
struct FdIO {
  FdRes* res;   // [i]
  Match* tab;   // [res[i].off + k]: match k
};
struct FdPat {
  const u32* units;  // the pattern's units, packed as the pool packs them, zero-padded to a dword
  u32 m_units;       // 1 .. 256 (UTF-8) / 128 (UTF-16)
  u32 fold;          // FIND_ICASE: fold the text's units (the pattern's are folded already)
};

// units in 0x41..0x5A plus 0x20, per field.  t = the unit without its top bit; t + A sets the top
// bit iff t >= 0x41 and t + B iff t >= 0x5B (no carry leaves the field); a unit whose own top bit
// is set is none.
template <u32 ENC>
__device__ __forceinline__ u32 fd_fold(u32 x) {
  constexpr u32 LOW = ENC == ENC_UTF8 ? 0x7F7F7F7Fu : 0x7FFF7FFFu;
  constexpr u32 A = ENC == ENC_UTF8 ? 0x3F3F3F3Fu : 0x7FBF7FBFu;
  constexpr u32 B = ENC == ENC_UTF8 ? 0x25252525u : 0x7FA57FA5u;
  constexpr u32 SH = ENC == ENC_UTF8 ? 2u : 10u;  // top bit of the field -> 0x20
  u32 t = x & LOW;
  u32 up = (t + A) & ~(t + B) & ~x & ~LOW;
  return x | (up >> SH);
}

// Stage the window of the pass that starts at dword k0 of the document: win[w] = dword k0 + w,
// folded when asked, 0 at or past nw.  Called by all FD threads of the block.
template <u32 ENC>
__device__ __forceinline__ void fd_stage(const LnDoc& D, u32 k0, u32 fold, u32* win) {
  u32 tid = threadIdx.x;
  u32 x[LN_ROWS + 1u];
#pragma unroll
  for (u32 j = 0; j < LN_ROWS; j++) {
    u32 k = k0 + j * LN_T + tid;
    x[j] = k < D.nw ? D.words[k] : 0u;
  }
  u32 kh = k0 + LN_PASS + tid;
  x[LN_ROWS] = tid < FD_HALO && kh < D.nw ? D.words[kh] : 0u;
  if (fold) {
#pragma unroll
    for (u32 j = 0; j <= LN_ROWS; j++) x[j] = fd_fold<ENC>(x[j]);
  }
#pragma unroll
  for (u32 j = 0; j < LN_ROWS; j++) win[j * LN_T + tid] = x[j];
  if (tid < FD_HALO) win[LN_PASS + tid] = x[LN_ROWS];
}

// The matches that start in window dword w (document dword k = k0 + w), one bit per unit as ln_eq.
// lastu = the last unit, counted from words[0], at which a match may start (endu - m_units): the
// length test; the first dword's units before the document's head are masked as in ln_flags.
// pat = the pattern's dwords in LDS, nd of them, tmask = the units of the last one.
template <u32 ENC>
__device__ __forceinline__ u32 fd_matches(const LnDoc& D, const u32* win, const u32* pat, u32 w, u32 k, u64 lastu, u32 first,
                                          u32 nd, u32 tmask) {
  constexpr u32 UPD = ENC == ENC_UTF8 ? 4u : 2u;
  constexpr u32 REP = ENC == ENC_UTF8 ? 0x01010101u : 0x00010001u;
  u64 ku = (u64)k * UPD;
  if (k >= D.nw || ku > lastu) return 0u;
  u32 a = k == 0u ? D.head : 0u;
  u32 b = (u32)min((u64)UPD - 1u, lastu - ku);
  u32 x = win[w];
  u32 cand = ln_eq<ENC>(x, first) & enc_range<ENC>(a, b) & REP;
  u32 hit = 0u;
  while (cand) {
    u32 bit = (u32)__builtin_ctz(cand);  // SH * (the candidate's unit in the dword)
    u32 lo = x;
    bool ok = true;
    for (u32 t = 0; t < nd && ok; t++) {
      u32 hi = win[w + t + 1u];
      u32 v = (u32)((((u64)hi << 32) | lo) >> bit);
      u32 d = v ^ pat[t];
      if (t + 1u == nd) d &= tmask;
      ok = d == 0u;
      lo = hi;
    }
    hit |= ok ? 1u << bit : 0u;
    cand &= cand - 1u;
  }
  return hit;
}

// what both sweeps derive from the pattern: its dwords, the mask of the last one, its first unit
template <u32 ENC>
__device__ __forceinline__ void fd_pat_shape(u32 m_units, u32& nd, u32& tmask) {
  constexpr u32 UPD = ENC == ENC_UTF8 ? 4u : 2u;
  constexpr u32 SH = ENC == ENC_UTF8 ? 8u : 16u;
  nd = (m_units + UPD - 1u) / UPD;
  u32 rem = m_units - (nd - 1u) * UPD;  // 1 .. UPD units in the last dword
  tmask = rem == UPD ? 0xFFFFFFFFu : (1u << (rem * SH)) - 1u;
}

// First sweep.  One block of LN_WAVES waves per index of the encode: counts the matches that start
// in its units.  An index without an encode result has none here; a document shorter than the
// pattern has 0.  The windows alternate between two LDS buffers, so a pass has one barrier (a
// buffer is rewritten two passes later, past the barrier every wave reaches only after reading it).
template <u32 ENC>
__global__ __launch_bounds__(LN_T) void k_find_count(EncIO E, FdIO F, FdPat Pt, u32 n) {
  constexpr u32 UMASK = ENC == ENC_UTF8 ? 0xFFu : 0xFFFFu;
  u32 i = blockIdx.x;
  if (i >= n) return;
  EncRes rs = E.res[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  if (rs.units == INVALID || rs.units < Pt.m_units) {
    if (tid == 0) F.res[i] = FdRes{rs.units == INVALID ? INVALID : 0u, 0u, 0ull};
    return;
  }
  LnDoc D = ln_doc<ENC>(E, rs);
  __shared__ u32 s_win[2][FD_WIN];
  __shared__ u32 s_pat[FD_PAT_W];
  __shared__ u32 s_c[LN_WAVES];
  u32 nd, tmask;
  fd_pat_shape<ENC>(Pt.m_units, nd, tmask);
  if (tid < FD_PAT_W) s_pat[tid] = tid < nd ? Pt.units[tid] : 0u;
  u64 lastu = D.endu - Pt.m_units;
  u32 wq = wv * (LN_ROWS * 64u);  // this wave's first dword in a pass
  u32 cnt = 0u;
  for (u32 k0 = 0, row = 0; k0 < D.nw; k0 += LN_PASS, row ^= 1u) {
    const u32* win = s_win[row];
    fd_stage<ENC>(D, k0, Pt.fold, s_win[row]);
    __syncthreads();
    u32 first = s_pat[0] & UMASK;
#pragma unroll
    for (u32 j = 0; j < LN_ROWS; j++) {
      u32 w = wq + j * 64u + l;
      cnt += (u32)__popc(fd_matches<ENC>(D, win, s_pat, w, k0 + w, lastu, first, nd, tmask));
    }
  }
  u32 t = wave_sum(cnt);
  if (l == 0u) s_c[wv] = t;
  __syncthreads();
  if (tid == 0) F.res[i] = FdRes{s_c[0] + s_c[1] + s_c[2] + s_c[3], 0u, 0ull};
}

// k_result_scan's view of an FdRes: its matches (an index without a result counts as 0)
__device__ __forceinline__ void scan_counts(const FdRes& r, u64* c) { c[0] = r.n_matches == INVALID ? 0ull : (u64)r.n_matches; }
__device__ __forceinline__ void scan_store(FdRes& r, const u64* off) { r.off = off[0]; }

// Second sweep, after k_result_scan: the same passes, rows and windows.  Two running counts are
// carried from pass to pass in registers, as k_ln_write carries its: the matches so far (the rank
// in the table) and the char starts so far (the char position).  A dword has at most 4 of each and
// a pass at most 4,096, so both ride one wave scan per row as a packed pair (matches in the low,
// starts in the high 16 bits); the waves' totals meet in LDS.  The next pass's window is staged
// before this pass's barrier, into the other buffer, and the waves' totals alternate between two
// rows, so a pass has one barrier: it orders the next window's stores before their reads and this
// pass's totals before theirs, and a buffer (or row) is rewritten only past the barrier that every
// wave reaches after its last read of it.  The match at unit u with rank r writes entry r =
// {u, char starts in [0, u)}.  (r < n_matches by construction: the count sweep read the same units
// on the same stream.)
template <u32 ENC>
__global__ __launch_bounds__(LN_T) void k_find_write(EncIO E, FdIO F, FdPat Pt, u32 n) {
  constexpr u32 UPD = ENC == ENC_UTF8 ? 4u : 2u;
  constexpr u32 SH = ENC == ENC_UTF8 ? 8u : 16u;
  constexpr u32 REP = ENC == ENC_UTF8 ? 0x01010101u : 0x00010001u;
  constexpr u32 UMASK = ENC == ENC_UTF8 ? 0xFFu : 0xFFFFu;
  u32 i = blockIdx.x;
  if (i >= n) return;
  FdRes fr = F.res[i];
  if (fr.n_matches == INVALID || fr.n_matches == 0u) return;
  EncRes rs = E.res[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  Match* tab = F.tab + fr.off;
  LnDoc D = ln_doc<ENC>(E, rs);
  __shared__ u32 s_win[2][FD_WIN];
  __shared__ u32 s_pat[FD_PAT_W];
  __shared__ u32 s_w[2][LN_WAVES];
  u32 nd, tmask;
  fd_pat_shape<ENC>(Pt.m_units, nd, tmask);
  if (tid < FD_PAT_W) s_pat[tid] = tid < nd ? Pt.units[tid] : 0u;
  u64 lastu = D.endu - Pt.m_units;  // (n_matches > 0: units >= m_units)
  u32 wq = wv * (LN_ROWS * 64u);
  u32 run_m = 0u, run_s = 0u;  // carried: matches and char starts of the passes before this one
  fd_stage<ENC>(D, 0u, Pt.fold, s_win[0]);
  __syncthreads();
  u32 first = s_pat[0] & UMASK;
  for (u32 k0 = 0, row = 0; k0 < D.nw; k0 += LN_PASS, row ^= 1u) {
    const u32* win = s_win[row];
    if (D.nw - k0 > LN_PASS) fd_stage<ENC>(D, k0 + LN_PASS, Pt.fold, s_win[row ^ 1u]);
    u32 mt[LN_ROWS], st[LN_ROWS], v[LN_ROWS], inc[LN_ROWS], tot[LN_ROWS];
#pragma unroll
    for (u32 j = 0; j < LN_ROWS; j++) {
      u32 w = wq + j * 64u + l, k = k0 + w;
      mt[j] = fd_matches<ENC>(D, win, s_pat, w, k, lastu, first, nd, tmask);
      bool in = k < D.nw;
      u32 a = k == 0u ? D.head : 0u;
      u32 b = (u32)min((u64)UPD, D.endu - (u64)k * UPD) - 1u;  // (in: endu - k UPD >= 1)
      st[j] = in ? enc_starts<ENC>(win[w]) & enc_range<ENC>(a, b) & REP : 0u;
      v[j] = (u32)__popc(mt[j]) | ((u32)__popc(st[j]) << 16);
    }
#pragma unroll
    for (u32 j = 0; j < LN_ROWS; j++) {
      inc[j] = wave_incl_scan(v[j]);
      tot[j] = rdlane(inc[j], 63);
    }
    if (l == 0u) s_w[row][wv] = tot[0] + tot[1] + tot[2] + tot[3];
    __syncthreads();
    u32 base = 0u, all = 0u;  // packed: the waves before this one, and the whole pass
    for (u32 x = 0; x < LN_WAVES; x++) {
      u32 ww = s_w[row][x];
      base += x < wv ? ww : 0u;
      all += ww;
    }
#pragma unroll
    for (u32 j = 0; j < LN_ROWS; j++) {
      u32 ex = base + inc[j] - v[j];  // this dword's exclusive pair, in the pass
      base += tot[j];
      u32 r = run_m + (ex & 0xFFFFu), cs = run_s + (ex >> 16);
      u32 k = k0 + wq + j * 64u + l;
      u32 b = mt[j];
      while (b) {
        u32 jj = (u32)__builtin_ctz(b) / SH;  // the match's first unit in the dword
        u32 u = k * UPD + jj - D.head;        // ... and in the document
        // (unit jj starts a char: the count of starts in [0, jj] includes it)
        if (r < fr.n_matches) tab[r] = Match{u, cs + (u32)__popc(st[j] & enc_range<ENC>(0u, jj)) - 1u};
        r++;
        b &= b - 1u;
      }
    }
    run_m += all & 0xFFFFu;
    run_s += all >> 16;
  }
}

// Find next / previous from a char position.  One thread per query (grid stride): a binary search
// over the index's matches by pos.  SEEK_NEXT: the first match with match.pos >= pos; SEEK_PREV:
// the last match with match.pos <= pos; INVALID when there is none, for an idx out of range and
// for an index without a result.  pos is not checked against the document's chars.
__global__ __launch_bounds__(256) void k_find_seek(FdIO F, u32 n_idx, u64 nq, const u32* idx, const u32* pos, u32 dir, u32* out) {
  for (u64 q = (u64)blockIdx.x * 256u + threadIdx.x; q < nq; q += (u64)gridDim.x * 256u) {
    u32 i = idx[q], p = pos[q];
    u32 ans = INVALID;
    if (i < n_idx) {
      FdRes fr = F.res[i];
      if (fr.n_matches != INVALID) {
        const Match* tab = F.tab + fr.off;
        u32 lo = 0u, hi = fr.n_matches;  // the first match at or past the bound is in [lo, hi]
        while (lo < hi) {
          u32 md = lo + ((hi - lo) >> 1);
          u32 mp = tab[md].pos;
          bool below = dir == SEEK_NEXT ? mp < p : mp <= p;
          if (below) lo = md + 1u; else hi = md;
        }
        if (dir == SEEK_NEXT) ans = lo < fr.n_matches ? lo : INVALID;
        else ans = lo ? lo - 1u : INVALID;
      }
    }
    out[q] = ans;
  }
}

}  // namespace crdt
