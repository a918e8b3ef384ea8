// Encoded text and unit offsets (crdt_encode_async and its queries, include/crdt_gpu.h): every
// listed document's materialised UTF-32 text (TextIO: text + ord_base, tlen) re-encoded as UTF-8
// bytes or UTF-16 code units, plus a sampled prefix index that maps char positions to unit offsets
// and back.  Reads nothing but what k_materialize left; the queries read nothing but the result.
//
// A content value that is no Unicode scalar value (a surrogate, or above 0x10FFFF) encodes as
// U+FFFD.  Unit offsets count bytes (UTF-8) or u16 units (UTF-16); the unit pool is byte-addressed
// and packed: document i's units start at byte res[i].off * (bytes per unit), with no padding
// between documents, so a UTF-8 document starts at any byte and a UTF-16 one at any even byte.
//
// Sample k of a document = units before char k * ENC_S, for every k * ENC_S <= chars.  ENC_S = 64:
// one row of a wave (below), so a sample is a row's exclusive base in the count sweep (no extra
// work), the write sweep's waves start from their own sample without meeting each other, and a
// query walks at most 64 chars (16 dwords of ASCII, 64 in the worst case) after its lookup.  The
// index costs 4 B per 64 chars: 1/16 of the ASCII bytes it indexes.
#pragma once
#include "kernels.h"

namespace crdt {

constexpr u32 ENC_UTF8 = 0u, ENC_UTF16 = 1u;  // CRDT_ENC_*
#define ENC_T 256u     // threads per document
#define ENC_WAVES 4u
#define ENC_ROWS 4u    // rows of 64 chars a wave takes per loop pass
#define ENC_PASS 1024u // chars per loop pass (ENC_WAVES * ENC_ROWS * 64)
#define ENC_S 64u      // chars per sample (see above)
#define ENC_S_LOG 6u

struct EncRes {
  u32 units, chars;  // both INVALID: no result for this index
  u64 off;           // first unit of this index in the unit pool, in units (k_result_scan)
};
struct EncIO {
  const u32* docs;     // [i] the listed documents
  const u64* sp_base;  // [i] first sample of index i
  EncRes* res;         // [i]
  u32* samples;        // [sp_base[i] + k]
  u8* units;           // the unit pool (bytes; 4-byte aligned, its size a multiple of 4)
};

__device__ __forceinline__ u32 enc_scalar(u32 c) { return (c - 0xD800u < 0x800u || c > 0x10FFFFu) ? 0xFFFDu : c; }

// units of content value c, i.e. of enc_scalar(c), without the detour: a surrogate already lies
// in the 3-byte / 1-unit range of U+FFFD, and a value above 0x10FFFF loses the last step again
template <u32 ENC>
__device__ __forceinline__ u32 enc_width_raw(u32 c) {
  if (ENC == ENC_UTF8) return 1u + (u32)(c >= 0x80u) + (u32)(c >= 0x800u) + (u32)(c >= 0x10000u) - (u32)(c > 0x10FFFFu);
  return 1u + (u32)(c >= 0x10000u) - (u32)(c > 0x10FFFFu);
}

// the units of scalar value c, packed little endian (first unit in the low bits)
template <u32 ENC>
__device__ __forceinline__ u32 enc_pack(u32 c) {
  if (ENC == ENC_UTF8) {
    if (c < 0x80u) return c;
    if (c < 0x800u) return (0xC0u | (c >> 6)) | ((0x80u | (c & 0x3Fu)) << 8);
    if (c < 0x10000u) return (0xE0u | (c >> 12)) | ((0x80u | ((c >> 6) & 0x3Fu)) << 8) | ((0x80u | (c & 0x3Fu)) << 16);
    return (0xF0u | (c >> 18)) | ((0x80u | ((c >> 12) & 0x3Fu)) << 8) | ((0x80u | ((c >> 6) & 0x3Fu)) << 16) |
           ((0x80u | (c & 0x3Fu)) << 24);
  }
  if (c < 0x10000u) return c;
  u32 v = c - 0x10000u;
  return (0xD800u + (v >> 10)) | ((0xDC00u + (v & 0x3FFu)) << 16);
}

// First sweep.  One block of ENC_WAVES waves per listed document, ENC_PASS = 1,024 chars per pass:
// a wave takes 256 consecutive chars as ENC_ROWS = 4 rows of 64, lane l the chars l, 64 + l, ... of
// them, so every load is a coalesced row of UTF-32 and a row is exactly one sample.  Per-char
// widths, one wave scan per row, the waves' totals meet in LDS; the running unit count is carried
// from pass to pass in registers (every thread folds the same LDS values, as k_blame carries its
// tail).  Lanes 0..3 of a wave write its four samples.  A pass's loads are issued one pass ahead,
// and the waves' totals alternate between two LDS rows, so a pass has one barrier (a row is
// rewritten two passes later, past the barrier that every wave reaches only after reading it).
// (At 256 chars per pass -- one row per wave, one barrier and one LDS exchange per 256 chars -- the
// two sweeps were bound by instruction issue, not by memory: DESIGN.md.)  A document without text
// (tlen INVALID: poisoned, no content, too short a stream) or whose units do not fit below
// 0xFFFFFFFF has no result.
template <u32 ENC>
__global__ __launch_bounds__(ENC_T) void k_enc_count(Pools P, TextIO T, EncIO E, u32 n) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  u32 d = E.docs[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  u32 tl = T.tlen[d];
  if (tl == INVALID) {
    if (tid == 0) E.res[i] = EncRes{INVALID, INVALID, 0ull};
    return;
  }
  const DocSeg& sg = P.seg[d];
  u32 chars = min(tl, sg.ord_cap);
  const u32* src = T.text + sg.ord_base;
  u32* smp = E.samples + E.sp_base[i];
  __shared__ u32 s_w[2][ENC_WAVES];
  u64 run = 0;  // carried: units of the passes before this one
  u32 wq = wv * (ENC_ROWS * 64u);  // this wave's first char in a pass
  u32 cur[ENC_ROWS];
#pragma unroll
  for (u32 j = 0; j < ENC_ROWS; j++) {
    u32 c = wq + j * 64u + l;
    cur[j] = c < chars ? src[c] : 0u;
  }
  for (u32 c0 = 0, row = 0; c0 < chars; c0 += ENC_PASS, row ^= 1u) {
    u32 left = chars - c0;  // > 0; an index at or past chars is never formed into an address
    u32 nxt[ENC_ROWS], w[ENC_ROWS], tot[ENC_ROWS];
    if (left >= 2u * ENC_PASS) {  // this pass and the next one are whole: no guards
#pragma unroll
      for (u32 j = 0; j < ENC_ROWS; j++) {
        nxt[j] = src[c0 + ENC_PASS + wq + j * 64u + l];
        w[j] = enc_width_raw<ENC>(cur[j]);
      }
    } else {
#pragma unroll
      for (u32 j = 0; j < ENC_ROWS; j++) {
        u32 r = wq + j * 64u + l;  // this lane's char of row j, in the pass
        nxt[j] = left > ENC_PASS && left - ENC_PASS > r ? src[c0 + ENC_PASS + r] : 0u;  // the next pass's
        w[j] = r < left ? enc_width_raw<ENC>(cur[j]) : 0u;
      }
    }
#pragma unroll
    for (u32 j = 0; j < ENC_ROWS; j++) tot[j] = rdlane(wave_incl_scan(w[j]), 63);
    if (l == 0u) s_w[row][wv] = tot[0] + tot[1] + tot[2] + tot[3];
    __syncthreads();
    u64 base = run;
    for (u32 x = 0; x < wv; x++) base += s_w[row][x];
    // lane j writes the sample of row j: the units before its first char
    u32 before = (l > 0u ? tot[0] : 0u) + (l > 1u ? tot[1] : 0u) + (l > 2u ? tot[2] : 0u);
    if (l < ENC_ROWS && wq + l * 64u < left) smp[((c0 + wq) >> ENC_S_LOG) + l] = (u32)base + before;
    for (u32 x = 0; x < ENC_WAVES; x++) run += s_w[row][x];
#pragma unroll
    for (u32 j = 0; j < ENC_ROWS; j++) cur[j] = nxt[j];
  }
  if (tid == 0) {
    if (run >= (u64)INVALID) {
      E.res[i] = EncRes{INVALID, INVALID, 0ull};
    } else {
      if ((chars & (ENC_S - 1u)) == 0u) smp[chars >> ENC_S_LOG] = (u32)run;  // the sample at the text's end
      E.res[i] = EncRes{(u32)run, chars, 0ull};
    }
  }
}

// k_result_scan's view of an EncRes: its units (an index without a result counts as 0)
__device__ __forceinline__ void scan_counts(const EncRes& r, u64* c) { c[0] = r.units == INVALID ? 0u : r.units; }
__device__ __forceinline__ void scan_store(EncRes& r, const u64* off) { r.off = off[0]; }

// Second sweep, after k_result_scan: the same passes and rows.  A wave's first unit is its sample; the
// row scans and the row totals before a row give every char its unit offset.  The pass's units (at
// most 4,096 B) are assembled in LDS at the byte phase (0..3) their first byte has in the pool, and
// go out as whole aligned dwords, coalesced.  A dword only partly inside the pass -- the first and
// the last one, at most: the document's unaligned head and tail, or the seam between two passes --
// is stored byte by byte by its one thread, so no byte outside the document is ever written (the
// neighbour documents' blocks write theirs at the same time).  The next pass's chars and samples
// are loaded one pass ahead, and the passes alternate between two LDS buffers, so a pass has one
// barrier.
template <u32 ENC>
__global__ __launch_bounds__(ENC_T) void k_enc_write(Pools P, TextIO T, EncIO E, u32 n) {
  constexpr u32 USZ = ENC == ENC_UTF8 ? 1u : 2u;          // bytes per unit
  constexpr u32 PASS_B = ENC_PASS * 4u;                   // most bytes of a pass (either encoding)
  u32 i = blockIdx.x;
  if (i >= n) return;
  EncRes rs = E.res[i];
  if (rs.units == INVALID) return;
  u32 d = E.docs[i];
  u32 tid = threadIdx.x, l = lane_id();
  const DocSeg& sg = P.seg[d];
  u32 chars = rs.chars;
  const u32* src = T.text + sg.ord_base;
  const u32* smp = E.samples + E.sp_base[i];
  __shared__ u32 s_bufs[2][PASS_B / 4u + 1u];  // + the phase
  u32 wq = (tid >> 6) * (ENC_ROWS * 64u);      // this wave's first char in a pass
  // the samples at the start and the end of a pass and at this wave's first char (rs.units past the text)
  u32 p0 = 0u;
  u32 p1 = ENC_PASS < chars ? smp[ENC_PASS >> ENC_S_LOG] : rs.units;
  u32 wb = wq < chars ? smp[wq >> ENC_S_LOG] : rs.units;
  u32 cur[ENC_ROWS];
#pragma unroll
  for (u32 j = 0; j < ENC_ROWS; j++) {
    u32 c = wq + j * 64u + l;
    cur[j] = c < chars ? src[c] : 0u;
  }
  for (u32 c0 = 0, row = 0; c0 < chars; c0 += ENC_PASS, row ^= 1u) {
    u32* s_buf = s_bufs[row];
    u8* sb = (u8*)s_buf;
    u32 left = chars - c0;  // > 0; an index at or past chars is never formed into an address
    bool more = left > ENC_PASS;
    u32 p2 = more && left - ENC_PASS > ENC_PASS ? smp[(c0 + 2u * ENC_PASS) >> ENC_S_LOG] : rs.units;
    u32 wbn = more && left - ENC_PASS > wq ? smp[(c0 + ENC_PASS + wq) >> ENC_S_LOG] : rs.units;
    u64 gb = (rs.off + p0) * USZ;  // the pass's first byte in the pool
    u32 nb = (p1 - p0) * USZ;
    u32 ph = (u32)gb & 3u;
    // (the guards hold by construction: the count sweep read the same text on the same stream)
    bool pass_ok = p1 <= rs.units && p0 <= p1 && nb <= PASS_B;
    u32 nxt[ENC_ROWS], ws[ENC_ROWS];
    if (left >= 2u * ENC_PASS) {  // this pass and the next one are whole: no guards
#pragma unroll
      for (u32 j = 0; j < ENC_ROWS; j++) {
        nxt[j] = src[c0 + ENC_PASS + wq + j * 64u + l];
        ws[j] = enc_width_raw<ENC>(cur[j]);
      }
    } else {
#pragma unroll
      for (u32 j = 0; j < ENC_ROWS; j++) {
        u32 r = wq + j * 64u + l;  // this lane's char of row j, in the pass
        nxt[j] = more && left - ENC_PASS > r ? src[c0 + ENC_PASS + r] : 0u;
        ws[j] = r < left ? enc_width_raw<ENC>(cur[j]) : 0u;
      }
    }
    u32 rb = wb;  // first unit of the row
#pragma unroll
    for (u32 j = 0; j < ENC_ROWS; j++) {
      u32 cp = enc_scalar(cur[j]);
      u32 w = ws[j];
      u32 Ci = wave_incl_scan(w);
      u32 uo = rb + Ci - w;  // this char's first unit, in the document
      rb += rdlane(Ci, 63);
      if (w > 0u && pass_ok && uo >= p0 && uo + w <= p1) {
        u32 at = ph + (uo - p0) * USZ;
        u32 v = enc_pack<ENC>(cp);
        if (ENC == ENC_UTF8) {
          for (u32 b = 0; b < w; b++) sb[at + b] = (u8)(v >> (8u * b));
        } else {
          u16* s16 = (u16*)(sb + at);  // (at is even: gb and every unit offset are)
          s16[0] = (u16)v;
          if (w == 2u) s16[1] = (u16)(v >> 16);
        }
      }
    }
    __syncthreads();
    if (pass_ok) {
      u32 lo = ph, hi = ph + nb;  // the pass's bytes in s_buf
      u8* g = E.units + (gb - ph);
      for (u32 t = tid; t * 4u < hi; t += ENC_T) {
        u32 b0 = t * 4u;
        if (b0 >= lo && b0 + 4u <= hi) {
          *(u32*)(g + b0) = s_buf[t];
        } else {
          for (u32 b = max(b0, lo); b < min(b0 + 4u, hi); b++) g[b] = sb[b];
        }
      }
    }
#pragma unroll
    for (u32 j = 0; j < ENC_ROWS; j++) cur[j] = nxt[j];
    p0 = p1;
    p1 = p2;
    wb = wbn;
  }
}

// One bit per unit of the aligned pool dword x, at bit 8 j (UTF-8) / 16 j (UTF-16) for unit j: the
// unit starts a char (no continuation byte 10xxxxxx / no low surrogate 0xDC00..0xDFFF).
template <u32 ENC>
__device__ __forceinline__ u32 enc_starts(u32 x) {
  if (ENC == ENC_UTF8) return ~((x >> 7) & ~(x >> 6)) & 0x01010101u;
  return (u32)((x & 0xFC00u) != 0xDC00u) | ((u32)((x & 0xFC000000u) != 0xDC000000u) << 16);
}
// the bits of units a..b (inclusive) of a dword
template <u32 ENC>
__device__ __forceinline__ u32 enc_range(u32 a, u32 b) {
  constexpr u32 SH = ENC == ENC_UTF8 ? 8u : 16u;
  return (0xFFFFFFFFu << (a * SH)) & (0xFFFFFFFFu >> (31u - b * SH));
}

// units -> pos.  One thread per query (grid stride).  A binary search over the document's samples
// (monotone in units) finds the last sample at or below u; the walk then counts, a dword at a time,
// the char starts among the units from that sample up to and including u.  idx out of range or
// without a result, or u above the document's units: INVALID, mid 0.
template <u32 ENC>
__global__ __launch_bounds__(256) void k_units_to_pos(EncIO E, u32 n_idx, u64 nq, const u32* idx, const u32* unit, u32* pos,
                                                      u8* mid) {
  constexpr u32 UPD = ENC == ENC_UTF8 ? 4u : 2u;  // units per dword
  constexpr u32 SH = ENC == ENC_UTF8 ? 8u : 16u;
  const u32* words = (const u32*)E.units;
  for (u64 q = (u64)blockIdx.x * 256u + threadIdx.x; q < nq; q += (u64)gridDim.x * 256u) {
    u32 i = idx[q], u = unit[q];
    u32 ans = INVALID, m = 0u;
    if (i < n_idx) {
      EncRes rs = E.res[i];
      if (rs.units != INVALID && u <= rs.units) {
        if (u == rs.units) {
          ans = rs.chars;
        } else {
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
          m = ((st >> ((u32)(g1 % UPD) * SH)) & 1u) ^ 1u;
          ans = (lo << ENC_S_LOG) + cnt - 1u;
        }
      }
    }
    pos[q] = ans;
    if (mid) mid[q] = (u8)m;
  }
}

// pos -> units.  One thread per query (grid stride).  Sample pos / ENC_S, then a walk over the
// encoded units, a dword at a time, to the (pos % ENC_S)-th char start after the sample's.  idx out
// of range or without a result, or pos above the document's chars: INVALID.
template <u32 ENC>
__global__ __launch_bounds__(256) void k_pos_to_units(EncIO E, u32 n_idx, u64 nq, const u32* idx, const u32* pos, u32* unit) {
  constexpr u32 UPD = ENC == ENC_UTF8 ? 4u : 2u;
  constexpr u32 SH = ENC == ENC_UTF8 ? 8u : 16u;
  const u32* words = (const u32*)E.units;
  for (u64 q = (u64)blockIdx.x * 256u + threadIdx.x; q < nq; q += (u64)gridDim.x * 256u) {
    u32 i = idx[q], p = pos[q];
    u32 ans = INVALID;
    if (i < n_idx) {
      EncRes rs = E.res[i];
      if (rs.units != INVALID && p <= rs.chars) {
        u32 r = p & (ENC_S - 1u);
        if (p == rs.chars) {
          ans = rs.units;
        } else {
          u32 s = E.samples[E.sp_base[i] + (p >> ENC_S_LOG)];
          ans = s;
          if (r) {
            ans = rs.units;  // (never left standing: char p < chars starts inside the document)
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
          }
        }
      }
    }
    unit[q] = ans;
  }
}

}  // namespace crdt
