// Edits in units between two versions (crdt_edits_between_async, include/crdt_gpu.h): the walk of
// crdt_diff_between_async -- an item is old when it is visible at `from` and new when it is visible
// at `to`, K / D / I / N and the patches as above k_diff2 (kernels.h) -- with the widths and the
// fields of crdt_edits_async (edits.h).  The result is the edits result: EdRes, Edit and the pool
// are k_edits', and everything that reads an edits result reads this one.
//
// As in k_diff2 a span's items change class at any order, so k_edits' closed form per span does
// not hold and the classes come from the two bitmaps one 32-order word at a time.  The widths come
// the same way: k_ed_planes leaves, per bitmap word, the widths of its 32 orders as bit planes (bit
// 0 and bit 1 of w - 1, as EdWord holds them; UTF-16 has bit 0 only: 8 or 4 bytes per 32 orders),
// and the units of any class mask M inside a word are popc(M) + popc(M & b0) + 2 popc(M & b1)
// (e2_units): no content read and no item loop but for the inserted items that are encoded.  No
// running sums: every word of a span is walked for its classes anyway, and its units are three
// popcounts more.
#pragma once
#include "edits.h"

namespace crdt {

template <u32 ENC>
constexpr u32 ED2_PL = ENC == ENC_UTF8 ? 2u : 1u;  // plane words per bitmap word
template <u32 ENC>
using EdUnit = typename std::conditional<ENC == ENC_UTF8, u8, u16>::type;

struct Ed2IO {
  EdIO e;           // since = from, bm = the "deleted before from" bitmaps (words is not used); the result as k_edits'
  const u32* to;    // [i]
  const u32* bm_b;  // "deleted before to", at the same bm_base
  u32* planes;      // [(bm_base[i] + w) * ED2_PL + (0, 1)]: b0 (and b1) of word w, for every w <= next_order >> 5
};

// Width planes.  One block of 4 waves per listed document, 256 bitmap words (8,192 orders) per
// pass, rows and ballots as k_ed_prefix: a wave takes 64 consecutive words as 32 rows of 64 orders,
// lane l the order l of a row (coalesced), eight rows' loads in flight, and lane w keeps the halves
// of the two ballots that are word w's planes.  No scan and no barrier inside the loop: a word's
// planes depend on its own orders only.  The widths' sum over all orders, which decides with the
// rest of k_ed_prefix's conditions whether the index has a result (res[i].flags), is one reduction
// at the end.
template <u32 ENC>
__global__ __launch_bounds__(DIFF_T) void k_ed_planes(Pools P, Ed2IO E2, u32 n) {
  const EdIO& E = E2.e;
  u32 i = blockIdx.x;
  if (i >= n) return;
  u32 d = E.docs[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  i32 stt = P.st[d].status;
  u32 no = P.st[d].next_order, from = E.since[i], to = E2.to[i];
  u64 cb = E.cbase[d], cl = E.clen[d];
  if ((stt != ST_OK && stt != ST_NEED_CAPACITY) || from > no || to > no || cb == NO_CONTENT || cl < (u64)no) {
    if (tid == 0) E.res[i] = EdRes{0u, 0u, ED_BAD, no, 0ull, 0ull};
    return;
  }
  u32 nw = pub_words(P.seg[d].ord_cap);  // ord_cap > every order: next_order >> 5 < nw
  u32* pl = E2.planes + E.bm_base[i] * ED2_PL<ENC>;
  const u32* src = E.content + cb;
  u32 last = min(no >> 5, nw - 1u);  // the last word that gets its planes
  u64 tot = 0;                       // this lane's words: the sum of their widths
  for (u32 w0 = 0; w0 <= last; w0 += DIFF_T) {
    u32 wb = w0 + wv * 64u;  // this wave's first word
    u32 wi = wb + l;
    u32 a_b0 = 0, a_b1 = 0;
    u64 wo = (u64)wb * 32u;  // the wave's first order; its rows with an order below next_order:
    u32 rows = wo < (u64)no ? (u32)min((u64)32u, ((u64)no - wo + 63u) >> 6) : 0u;
    for (u32 j0 = 0; j0 < rows; j0 += 8u) {
      u32 cv[8];
#pragma unroll
      for (u32 q = 0; q < 8u; q++) {
        u64 o = wo + (u64)(j0 + q) * 64u + l;
        cv[q] = o < (u64)no ? src[o] : 0u;  // (a 0 has width 1: no bit in either plane)
      }
#pragma unroll
      for (u32 q = 0; q < 8u; q++) {
        u32 j = j0 + q;
        u32 w1 = enc_width_raw<ENC>(cv[q]) - 1u;  // 0..3
        u64 b0 = ballot((w1 & 1u) != 0u), b1 = ballot((w1 & 2u) != 0u);
        if (l == 2u * j) { a_b0 = (u32)b0; a_b1 = (u32)b1; }
        if (l == 2u * j + 1u) { a_b0 = (u32)(b0 >> 32); a_b1 = (u32)(b1 >> 32); }
      }
    }
    u64 wfirst = (u64)wi * 32u;
    u32 nin = wfirst < (u64)no ? (u32)min((u64)32u, (u64)no - wfirst) : 0u;  // the word's orders below next_order
    tot += nin + (u32)__popc(a_b0) + 2u * (u32)__popc(a_b1);
    if (wi <= last) {
      if (ENC == ENC_UTF8) *(uint2*)(pl + (u64)wi * 2u) = make_uint2(a_b0, a_b1);
      else pl[wi] = a_b0;
    }
  }
  __shared__ u64 s_t[DIFF_WAVES];
  tot = wave_sum64(tot);
  if (l == 0u) s_t[wv] = tot;
  __syncthreads();
  if (tid == 0) {
    u64 all = 0;
    for (u32 w = 0; w < DIFF_WAVES; w++) all += s_t[w];
    E.res[i] = EdRes{0u, 0u, all >= (u64)INVALID ? ED_BAD : 0u, no, 0ull, 0ull};
  }
}

// A wave-uniform value moved into a vector register.  k_edits2's write sweep is short of scalar
// registers (its uniform pointers and bounds, the ballots and the exec masks of its nested loops
// want more than the 102 there are, and the allocator then spills some into vector lanes); what
// only ever meets per-lane values -- the versions, the edits' pointer and the results' bounds -- is
// kept in vector registers instead.
__device__ __forceinline__ u32 in_vgpr(u32 x) {
  u32 r;
  asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(x));
  return r;
}
template <class T>
__device__ __forceinline__ T* in_vgpr(T* p) {
  u64 x = (u64)p;
  return (T*)(((u64)in_vgpr((u32)(x >> 32)) << 32) | in_vgpr((u32)x));
}
// one word of a span [a, b): k_diff2's classes and the word's width planes
struct E2Word {
  D2Word x;
  u32 b0, b1;
};
template <u32 ENC>
__device__ __forceinline__ E2Word e2_word(const u32* bma, const u32* bmb, const u32* pl, u32 w, u32 a, u32 b, u32 from, u32 to) {
  E2Word r;
  r.x = d2_word(bma, bmb, w, a, b, from, to);
  if (ENC == ENC_UTF8) {
    uint2 p = *(const uint2*)(pl + (u64)w * 2u);
    r.b0 = p.x;
    r.b1 = p.y;
  } else {
    r.b0 = pl[w];
    r.b1 = 0u;
  }
  return r;
}
// the units of the items of mask M in a word with planes b0, b1
template <u32 ENC>
__device__ __forceinline__ u32 e2_units(u32 M, u32 b0, u32 b1) {
  u32 s = (u32)__popc(M) + (u32)__popc(M & b0);
  if (ENC == ENC_UTF8) s += 2u * (u32)__popc(M & b1);
  return s;
}
// D, I and new items and their units: of a word, a stretch, or everything before a point
struct E2Cnt {
  u32 d, i, n, du, iu, nu;
};
__device__ __forceinline__ E2Cnt operator+(const E2Cnt& a, const E2Cnt& b) {
  return E2Cnt{a.d + b.d, a.i + b.i, a.n + b.n, a.du + b.du, a.iu + b.iu, a.nu + b.nu};
}
__device__ __forceinline__ E2Cnt operator-(const E2Cnt& a, const E2Cnt& b) {
  return E2Cnt{a.d - b.d, a.i - b.i, a.n - b.n, a.du - b.du, a.iu - b.iu, a.nu - b.nu};
}
__device__ __forceinline__ E2Cnt e2_scan(const E2Cnt& a) {
  return E2Cnt{wave_incl_scan(a.d), wave_incl_scan(a.i), wave_incl_scan(a.n), wave_incl_scan(a.du), wave_incl_scan(a.iu), wave_incl_scan(a.nu)};
}
__device__ __forceinline__ E2Cnt e2_rdlane(const E2Cnt& a, u32 s) {
  return E2Cnt{rdlane(a.d, s), rdlane(a.i, s), rdlane(a.n, s), rdlane(a.du, s), rdlane(a.iu, s), rdlane(a.nu, s)};
}
// (lane s's counts in every lane, kept in vector registers: the write sweep is short of scalar ones)
__device__ __forceinline__ E2Cnt e2_shfl(const E2Cnt& a, u32 s) {
  return E2Cnt{shfl(a.d, s), shfl(a.i, s), shfl(a.n, s), shfl(a.du, s), shfl(a.iu, s), shfl(a.nu, s)};
}
// ... of the items of word x below mask lowm
template <u32 ENC>
__device__ __forceinline__ E2Cnt e2_count(const E2Word& x, u32 lowm) {
  u32 D = x.x.o & ~x.x.n & lowm, I = x.x.n & ~x.x.o & lowm, N = x.x.n & lowm;
  return E2Cnt{(u32)__popc(D), (u32)__popc(I), (u32)__popc(N), e2_units<ENC>(D, x.b0, x.b1), e2_units<ENC>(I, x.b0, x.b1),
               e2_units<ENC>(N, x.b0, x.b1)};
}
// the summary of a stretch of items: k_diff2's D2Sum with units next to items
struct E2Sum {
  u32 has, fc, lc, si;
  E2Cnt c;
};
// the edits that start in one word: pos, unit and ins_off and, for now, the D / I items and units
// before the start in the four length fields (as k_edits); c0 = the counts before the word
template <u32 ENC>
__device__ __forceinline__ void e2_emit(u32 S, const E2Word& x, u32 p, const E2Cnt& c0, Edit* ed, u32 my_ed) {
  while (S) {
    u32 lowm = (1u << (u32)__builtin_ctz(S)) - 1u;
    S &= S - 1u;
    if (p < my_ed) {
      E2Cnt c = c0 + e2_count<ENC>(x, lowm);
      ed[p] = Edit{c.n, c.d, c.i, c.nu, c.du, c.iu, c.iu, 0u};
    }
    p++;
  }
}
// one inserted item goes out: w units of pk at dst, below the first sweep's count
template <u32 ENC>
__device__ __forceinline__ void e2_put(EdUnit<ENC>* up, u32 my_un, u32 dst, u32 pk, u32 w) {
  for (u32 q = 0; q < w; q++)
    if (dst + q < my_un) up[dst + q] = (EdUnit<ENC>)(pk >> (q * (u32)(8u * sizeof(EdUnit<ENC>))));
}

// A long span [ua, ub) walked by the whole wave, 64 words per step in lane order (d2_long with
// units).  WRITE = false: its summary.  WRITE = true: `open` / p / at are the true state and counts
// before the span (the same in every lane, in vector registers); its edits are written by the lanes that hold their words, and its inserted items
// are encoded with contiguous stores: lane l takes item t + l of the step's, finds its word by the
// 6-step search over the scan and its bit by the 5-step search over the word; the units before it
// are those before the step, before its word (the scan) and below its bit (the word's planes).
template <u32 ENC, bool WRITE>
__device__ __forceinline__ E2Sum e2_long(const u32* bma, const u32* bmb, const u32* pl, u32 ua, u32 ub, u32 from, u32 to, u32 l,
                                         u32 open, u32 p, E2Cnt at, Edit* ed, u32 my_ed, EdUnit<ENC>* up, u32 my_un,
                                         const u32* src) {
  E2Sum t{0u, 0u, 0u, 0u, E2Cnt{0u, 0u, 0u, 0u, 0u, 0u}};
  u32 wl = (ub - 1u) >> 5;
  u64 lower = (1ull << l) - 1ull;
  for (u32 w0 = ua >> 5; w0 <= wl; w0 += 64u) {
    u32 w = w0 + l;
    E2Word x{D2Word{0u, 0u, 0u, 0u, 0u}, 0u, 0u};
    if (w <= wl) x = e2_word<ENC>(bma, bmb, pl, w, ua, ub, from, to);
    bool h = x.x.X != 0u;
    bool lastc = h && d2_last_c(x.x);
    u64 mO = ballot(lastc), mC = ballot(h && !lastc);
    u64 lo = mO & lower, lc = mC & lower;
    bool ob = (lo | lc) ? lo > lc : open != 0u;  // a patch is open before this lane's word
    u32 S = d2_starts(x.x, ob);
    u32 ns = (u32)__popc(S);
    E2Cnt own = e2_count<ENC>(x, 0xFFFFFFFFu);
    if (!WRITE) {
      if (!t.has && (mO | mC)) {
        t.has = 1u;
        t.fc = rdlane(h && d2_first_c(x.x) ? 1u : 0u, (u32)__builtin_ctzll(mO | mC));
      }
      t.si += ns;  // (this lane's words: summed over the lanes after the last step)
      t.c = t.c + own;
    } else {
      u32 Pi = wave_incl_scan(ns);
      E2Cnt inc = e2_scan(own);
      e2_emit<ENC>(S, x, p + Pi - ns, at + inc - own, ed, my_ed);
      u32 im = x.x.n & ~x.x.o;
      u32 st = inc.i - own.i;     // the word's first inserted item within the step
      u32 ust = inc.iu - own.iu;  // the inserted units of the step before the word
      u32 Tn = rdlane(inc.i, 63);
      for (u32 t0 = 0; t0 < Tn; t0 += 64u) {
        u32 j = t0 + l;
        u32 s = 0;
#pragma unroll
        for (u32 step = 32u; step >= 1u; step >>= 1) s += shfl(inc.i, s + step - 1u) <= j ? step : 0u;
        u32 sm = shfl(im, s), sst = shfl(st, s), sus = shfl(ust, s), sb0 = shfl(x.b0, s), sb1 = shfl(x.b1, s);
        bool act = j < Tn;
        u32 bit = act ? nth_bit(sm, j - sst) : 0u;
        u32 o = ((w0 + s) << 5) + bit;
        u32 dst = at.iu + sus + e2_units<ENC>(sm & ((1u << bit) - 1u), sb0, sb1);
        u32 cv = act ? src[o] : 0u;
        u32 wd = act ? enc_width_raw<ENC>(cv) : 0u;
        e2_put<ENC>(up, my_un, dst, enc_pack<ENC>(enc_scalar(cv)), wd);
      }
      p += shfl(Pi, 63u);
      at = at + e2_shfl(inc, 63u);
    }
    if (mO | mC) open = mO > mC ? 1u : 0u;
  }
  if (!WRITE) {
    t.si = wave_sum(t.si);
    t.c = e2_rdlane(e2_scan(t.c), 63);
  }
  t.lc = (t.has && open) ? 1u : 0u;
  return t;
}

// One block per listed document, DIFF_T canonical spans per loop pass, in document order: k_diff2's
// sweep with units carried next to items, count sweep / k_result_scan<EdRes> / write sweep as
// k_edits.  Within a pass each thread summarises its span word by word (E2Sum; spans past
// DIFF2_LONG by the whole wave), the ballots and wave scans give the state and the counts before
// every span, and the waves' totals meet in LDS; the open state and the counts of edits, of D, I
// and new items and of their units carry from pass to pass in registers.  The write sweep walks the
// words of every span in which an edit starts once more, with the true state before it, and the
// lane writes those starts: pos, unit and ins_off and, for now, the D / I items and units before
// the start in the four length fields; a last sweep over the document's edits turns neighbouring
// starts into lengths (as k_edits).  The wave encodes its short spans' inserted items together, lane
// l on item t + l: the units before an item are the inserted units before the wave, those of the
// wave's long spans before the item's span, those of the short spans' items of earlier rounds and a
// scan of the round's widths; a long span's items go out in e2_long.  Every store stays below the
// counts of the first sweep.
template <u32 ENC, bool WRITE>
__global__ __launch_bounds__(DIFF_T) void k_edits2(Pools P, PubOut O, Ed2IO E2, u32 n) {
  typedef EdUnit<ENC> Unit;
  const EdIO& E = E2.e;
  u32 i = blockIdx.x;
  if (i >= n) return;
  EdRes rs = E.res[i];
  if (rs.flags & ED_BAD) return;  // (k_ed_planes)
  u32 d = E.docs[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  u32 from = E.since[i], to = E2.to[i];
  const DocSeg& sg = P.seg[d];
  const Span* cn = O.canon + sg.canon_base;
  u32 ns = min(O.canon_n[d], sg.canon_cap);
  // items at or above both versions are N; every order is below ord_cap (the bitmaps' words)
  u32 top = min(max(from, to), sg.ord_cap);
  u64 base = E.bm_base[i];
  const u32* bma = E.bm + base;
  const u32* bmb = E2.bm_b + base;
  const u32* pl = E2.planes + base * ED2_PL<ENC>;
  const u32* src = E.content + E.cbase[d];
  u32 my_ed = 0, my_un = 0;  // (WRITE) this index's counts from the first sweep: every store stays below them
  Edit* ed = nullptr;
  Unit* up = nullptr;
  if (WRITE) {
    from = in_vgpr(from); to = in_vgpr(to); top = in_vgpr(top);
    my_ed = in_vgpr(rs.n_ed); my_un = in_vgpr(rs.n_units);
    ed = in_vgpr(E.edits + rs.eoff);
    up = (Unit*)E.units + rs.uoff;  // (the item loops' pointers stay scalar: their loads and stores take a scalar base)
  }
  __shared__ u32 s_op[DIFF_WAVES], s_st[DIFF_WAVES], s_d[DIFF_WAVES], s_i[DIFF_WAVES], s_n[DIFF_WAVES], s_du[DIFF_WAVES],
      s_iu[DIFF_WAVES], s_nu[DIFF_WAVES];
  // carried: a patch is open; edits so far; D, I and new items and their units so far
  u32 c_open = 0, c_pat = 0;
  E2Cnt c_c{0u, 0u, 0u, 0u, 0u, 0u};
  for (u32 k0 = 0; k0 < ns; k0 += DIFF_T) {
    u32 k = k0 + tid;
    Span sp = k < ns ? cn[k] : Span{0, 0, 0, 0};
    u32 a = min(sp.order, top), b = (u32)min((u64)sp.order + slen(sp), (u64)top);
    u32 cnt = b > a ? b - a : 0u;
    E2Sum m{0u, 0u, 0u, 0u, E2Cnt{0u, 0u, 0u, 0u, 0u, 0u}};
    bool shrt = cnt != 0u && cnt <= DIFF2_LONG;
    u32 fo = 0, hi = 0;  // (WRITE) the span's first and last inserted order
    if (shrt) {
      bool open = true;
      for (u32 w = a >> 5; w <= ((b - 1u) >> 5); w++) {
        E2Word x = e2_word<ENC>(bma, bmb, pl, w, a, b, from, to);
        if (x.x.X) {
          if (!m.has) {
            m.has = 1u;
            m.fc = d2_first_c(x.x) ? 1u : 0u;
          }
          m.si += (u32)__popc(d2_starts(x.x, open));
          open = d2_last_c(x.x);
        }
        u32 im = x.x.n & ~x.x.o;
        if (WRITE && im) {
          if (!m.c.i) fo = (w << 5) + (u32)__builtin_ctz(im);
          hi = (w << 5) + 31u - (u32)__clz(im);
        }
        m.c = m.c + e2_count<ENC>(x, 0xFFFFFFFFu);
      }
      m.lc = (m.has && open) ? 1u : 0u;
    }
    u64 big = ballot(cnt > DIFF2_LONG);
    for (u64 bg = big; bg;) {
      u32 s = (u32)__builtin_ctzll(bg);
      bg &= bg - 1ull;
      E2Sum t = e2_long<ENC, false>(bma, bmb, pl, rdlane(a, s), rdlane(b, s), from, to, l, 1u, 0u, E2Cnt{0u, 0u, 0u, 0u, 0u, 0u},
                                    nullptr, 0u, nullptr, 0u, nullptr);
      if (l == s) m = t;
    }
    // state after each span: its last X item is a C (a patch is open) or a K (none is)
    u64 mO = ballot(m.has && m.lc), mC = ballot(m.has && !m.lc);
    E2Cnt inc = e2_scan(m.c);
    if (l == 63u) {
      s_d[wv] = inc.d;
      s_i[wv] = inc.i;
      s_n[wv] = inc.n;
      s_du[wv] = inc.du;
      s_iu[wv] = inc.iu;
      s_nu[wv] = inc.nu;
      s_op[wv] = (mO | mC) ? (mO > mC ? 1u : 2u) : 0u;  // (the higher lane decides) 0: no X item in this wave
    }
    __syncthreads();
    u32 open_in = c_open;
    E2Cnt in = c_c;  // the counts before this wave
    for (u32 w = 0; w < wv; w++) {
      u32 op = s_op[w];
      if (op) open_in = op == 1u;
      in = in + E2Cnt{s_d[w], s_i[w], s_n[w], s_du[w], s_iu[w], s_nu[w]};
    }
    u64 lower = (1ull << l) - 1ull;
    u64 lo = mO & lower, lc = mC & lower;
    bool open_before = (lo | lc) ? lo > lc : open_in != 0u;
    u32 nst = m.si + ((m.fc && !open_before) ? 1u : 0u);  // the edits that start in this span
    u32 Pi = wave_incl_scan(nst);
    if (l == 63u) s_st[wv] = Pi;
    __syncthreads();
    if (WRITE) {
      u32 p = c_pat + Pi - nst;
      for (u32 w = 0; w < wv; w++) p += s_st[w];
      E2Cnt ex = in + inc - m.c;  // the counts before this span
      if (shrt && nst != 0u) {    // the edits that start in this span: its words once more, with the true state
        bool open = open_before;
        u32 pp = p;
        E2Cnt c0 = ex;
        for (u32 w = a >> 5; w <= ((b - 1u) >> 5); w++) {
          E2Word x = e2_word<ENC>(bma, bmb, pl, w, a, b, from, to);
          u32 S = d2_starts(x.x, open);
          e2_emit<ENC>(S, x, pp, c0, ed, my_ed);
          pp += (u32)__popc(S);
          c0 = c0 + e2_count<ENC>(x, 0xFFFFFFFFu);
          if (x.x.X) open = d2_last_c(x.x);
        }
      }
      // the short spans' inserted items: lane l takes item t + l of the wave's, its span by the
      // 6-step search over the scan and its order as in k_diff2 (closed form for a span whose
      // inserted items are one run of orders, a walk of the words otherwise)
      u32 is = shrt ? m.c.i : 0u;
      u32 Is = wave_incl_scan(is);
      u32 st = Is - is;
      u32 Tn = rdlane(Is, 63);
      u32 lu = shrt ? 0u : m.c.iu;  // (a long span's inserted units lie between the short spans')
      u32 LUex = wave_incl_scan(lu) - lu;
      u64 mRun = ballot(is != 0u && hi - fo + 1u == is);
      u32 urun = in.iu;
      for (u32 t0 = 0; t0 < Tn; t0 += 64u) {
        u32 j = t0 + l;
        u32 s = 0;
#pragma unroll
        for (u32 step = 32u; step >= 1u; step >>= 1) s += shfl(Is, s + step - 1u) <= j ? step : 0u;
        u32 r = j - shfl(st, s);
        u32 o = shfl(fo, s) + r;
        u32 slu = shfl(LUex, s);
        bool act = j < Tn;
        bool walk = act && ((mRun >> s) & 1ull) == 0ull;
        if (ballot(walk)) {
          u32 sa = shfl(a, s), sb = shfl(b, s);
          if (walk) {
            for (u32 w = sa >> 5; w <= ((sb - 1u) >> 5); w++) {
              D2Word x = d2_word(bma, bmb, w, sa, sb, from, to);
              u32 im = x.n & ~x.o;
              u32 c = (u32)__popc(im);
              if (r < c) {
                o = (w << 5) + nth_bit(im, r);
                break;
              }
              r -= c;
            }
          }
        }
        u32 cv = act ? src[o] : 0u;
        u32 wd = act ? enc_width_raw<ENC>(cv) : 0u;
        u32 winc = wave_incl_scan(wd);
        e2_put<ENC>(up, my_un, urun + slu + winc - wd, enc_pack<ENC>(enc_scalar(cv)), wd);
        urun += rdlane(winc, 63);
      }
      for (u64 bg = big; bg;) {
        u32 s = (u32)__builtin_ctzll(bg);
        bg &= bg - 1ull;
        e2_long<ENC, true>(bma, bmb, pl, rdlane(a, s), rdlane(b, s), from, to, l, shfl(open_before ? 1u : 0u, s),
                           shfl(p, s), e2_shfl(ex, s), ed, my_ed, up, my_un, src);
      }
    }
    for (u32 w = 0; w < DIFF_WAVES; w++) {
      u32 op = s_op[w];
      if (op) c_open = op == 1u;
      c_c = c_c + E2Cnt{s_d[w], s_i[w], s_n[w], s_du[w], s_iu[w], s_nu[w]};
      c_pat += s_st[w];
    }
    __syncthreads();  // (the next pass rewrites the LDS totals)
  }
  if (!WRITE) {
    if (tid == 0) E.res[i] = EdRes{c_pat, c_c.iu, 0u, rs.version, 0ull, 0ull};
    return;
  }
  // the lengths of edit p: the D / I items and units from its start to the next edit's start, as k_edits
  u32 np = min(c_pat, my_ed);
  __syncthreads();
  for (u32 p0 = 0; p0 < np; p0 += DIFF_T) {
    u32 p = p0 + tid;
    u32 d0 = 0, d1 = 0, i0 = 0, i1 = 0, du0 = 0, du1 = 0, iu0 = 0, iu1 = 0;
    if (p < np) {
      Edit x = ed[p];
      d0 = x.del_len; i0 = x.ins_len; du0 = x.del_units; iu0 = x.ins_units;
      d1 = c_c.d; i1 = c_c.i; du1 = c_c.du; iu1 = c_c.iu;
      if (p + 1u < np) {
        Edit y = ed[p + 1u];
        d1 = y.del_len; i1 = y.ins_len; du1 = y.del_units; iu1 = y.ins_units;
      }
    }
    __syncthreads();
    if (p < np) {
      ed[p].del_len = d1 - d0;
      ed[p].ins_len = i1 - i0;
      ed[p].del_units = du1 - du0;
      ed[p].ins_units = iu1 - iu0;
    }
  }
}

}  // namespace crdt
