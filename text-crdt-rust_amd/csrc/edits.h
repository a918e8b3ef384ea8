// Text edits in units (crdt_edits_async, include/crdt_gpu.h): the diff of crdt_diff_async -- the
// same item walk and K / D / I / N classes (kernels.h, above k_diff) -- restated in the units of
// crdt_encode_async: every patch also carries the unit offset of its pos, the units of its deleted
// and of its inserted items, and the inserted items go out encoded (UTF-8 bytes or UTF-16 units),
// packed per index in patch order.  A caller that keeps a UTF-8 or UTF-16 buffer applies the edits
// front to back: replace del_units units at unit with the edit's ins_units units.
//
// The width w(x) of the item with order x is enc_width_raw(content[x]) (encode.h: a value that is
// no scalar is U+FFFD).  Deleted items are not in the current text, so their widths come from the
// order-indexed content, and a span's units must not cost a walk of its items: k_ed_prefix leaves,
// once per 32 orders (one bitmap word of k_diff_mark), one 24-byte record (EdWord): three running
// sums over the orders below the word -- w over all orders, w over the orders whose "deleted before
// since" bit is set, and the set bits themselves -- the word's own widths as two bit planes (w - 1
// is 0..3: bit 0 and bit 1 of it for each of the 32 orders; UTF-16 has bit 0 only), and the bitmap
// word again.  With it the units below any order o, all of them or those with a clear bitmap bit,
// are a sum plus three popcounts under the mask of o's word (ed_below, ed_below_clear): one record
// read, so every per-span quantity is a difference of two such lookups and the sweeps read no
// content but that of the inserted items they encode.  Content at the orders of delete ops means
// nothing, but any value has a width, and a span's range never contains such an order.  The index
// is 0.75 B per order next to the bitmap's 0.125 B.
//
// The sweeps are k_diff's: count, k_result_scan<EdRes> (edits, inserted units), write.
#pragma once
#include <type_traits>

#include "encode.h"

namespace crdt {

struct Edit { u32 pos, del_len, ins_len, unit, del_units, ins_units, ins_off, reserved; };  // crdt_edit (include/crdt_gpu.h)
constexpr u32 ED_BAD = 1u;  // no result for this index (k_ed_prefix decides: see there)
struct EdRes {
  u32 n_ed, n_units, flags, version;  // n_units: the inserted units of all its edits
  u64 eoff, uoff;  // first edit / first inserted unit of this index in the result arrays (k_result_scan)
};
struct alignas(8) EdWord {  // the width index of the orders [32 w, 32 w + 32)
  u32 sa;      // sum of w(x) over the orders x < 32 w
  u32 b0, b1;  // bit (x & 31): bit 0 / bit 1 of w(x) - 1 (b1 is 0 for UTF-16)
  u32 bm;      // k_diff_mark's word
  u32 sd;      // sum of w(x) over the orders x < 32 w whose bitmap bit is set
  u32 sc;      // the set bitmap bits below word w
};
struct EdIO {
  const u32* docs;     // [i] the listed documents
  const u32* since;    // [i]
  const u64* bm_base;  // [i] first word of the index's bitmap in bm, and its first record in words
  const u32* bm;       // k_diff_mark's bitmap: bit x set = a delete op with order < since covers item x
  EdWord* words;       // [bm_base[i] + w], for every w <= next_order >> 5
  EdRes* res;          // [i]
  Edit* edits;         // [res[i].eoff + p]
  u8* units;           // the inserted-unit pool: index i's units start at unit res[i].uoff
  const u32* content;  // TextIO's content streams
  const u64* cbase;
  const u64* clen;
};

// the two-counter instance of k_result_scan: edits and inserted units (0 for an index without a result)
template <>
constexpr u32 SCAN_K<EdRes> = 2;
__device__ __forceinline__ void scan_counts(const EdRes& r, u64* c) {
  bool bad = (r.flags & ED_BAD) != 0u;
  c[0] = bad ? 0ull : (u64)r.n_ed;
  c[1] = bad ? 0ull : (u64)r.n_units;
}
__device__ __forceinline__ void scan_store(EdRes& r, const u64* off) { r.eoff = off[0]; r.uoff = off[1]; }

// Width prefix.  One block of 4 waves per listed document, 256 bitmap words (8,192 orders) per
// pass; a wave takes 64 consecutive words as 32 rows of 64 orders (two words), lane l the order l
// of a row, so every content load is a coalesced row.  A width is 1..4, so two ballots of the bits
// of (width - 1) hold a row's widths, and lane w of the wave keeps the halves that are word w's two
// bit planes; after the 32 rows the sums of a lane's word -- all of it, and under the bitmap word
// -- are popcounts of its planes.  Eight rows' loads are issued before the first is used.  (A first
// version took the sums per row in scalar registers, twelve popcounts a row, with one load in
// flight: 2.9 ms for 8,192 AP documents, DESIGN.md.)  One wave scan per sum, the waves' totals meet
// in LDS, the running sums carry from pass to pass in registers (every thread folds the same LDS
// values, as k_diff does).  The record of word w is written for every w <= next_order >> 5, which
// is every word a lookup can name.
//
// Also decides whether the index has a result (res[i].flags, read by both sweeps): not when since
// is above the version, the document is poisoned, it has no content or a stream shorter than its
// orders, or its widths sum to 0xFFFFFFFF or more (so every unit count below fits 32 bits).
template <u32 ENC>
__global__ __launch_bounds__(DIFF_T) void k_ed_prefix(Pools P, EdIO E, u32 n) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  u32 d = E.docs[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  i32 stt = P.st[d].status;
  u32 no = P.st[d].next_order, v = E.since[i];
  u64 cb = E.cbase[d], cl = E.clen[d];
  if ((stt != ST_OK && stt != ST_NEED_CAPACITY) || v > no || cb == NO_CONTENT || cl < (u64)no) {
    if (tid == 0) E.res[i] = EdRes{0u, 0u, ED_BAD, no, 0ull, 0ull};
    return;
  }
  u32 nw = pub_words(P.seg[d].ord_cap);  // ord_cap > every order: next_order >> 5 < nw
  u64 base = E.bm_base[i];
  const u32* bm = E.bm + base;
  const u32* src = E.content + cb;
  u32 last = min(no >> 5, nw - 1u);  // the last word that gets a record
  __shared__ u32 s_t[3][DIFF_WAVES];
  u64 r_all = 0, r_del = 0;  // carried: the sums over the passes before this one
  u32 r_cnt = 0;
  for (u32 w0 = 0; w0 <= last; w0 += DIFF_T) {
    u32 wb = w0 + wv * 64u;  // this wave's first word
    u32 wi = wb + l;
    u32 mybm = wi < nw ? bm[wi] : 0u;
    u32 a_b0 = 0, a_b1 = 0;  // this lane's word: the two bit planes of its orders' widths
    u64 wo = (u64)wb * 32u;  // the wave's first order; its rows with an order below next_order:
    u32 rows = wo < (u64)no ? (u32)min((u64)32u, ((u64)no - wo + 63u) >> 6) : 0u;
    for (u32 j0 = 0; j0 < rows; j0 += 8u) {  // (rows past the last one hold nothing: their lanes keep their zeros)
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
    // the word's sums: over its orders below next_order, and over those under the bitmap word
    u64 wfirst = (u64)wi * 32u;
    u32 nin = wfirst < (u64)no ? (u32)min((u64)32u, (u64)no - wfirst) : 0u;
    u32 mv = nin == 32u ? 0xFFFFFFFFu : (1u << nin) - 1u;
    u32 dm = mybm & mv;
    u32 a_all = (u32)__popc(mv) + (u32)__popc(a_b0) + 2u * (u32)__popc(a_b1);
    u32 a_del = (u32)__popc(dm) + (u32)__popc(a_b0 & dm) + 2u * (u32)__popc(a_b1 & dm);
    u32 a_cnt = (u32)__popc(mybm);
    u32 Ia = wave_incl_scan(a_all), Id = wave_incl_scan(a_del), Ic = wave_incl_scan(a_cnt);
    if (l == 63u) {
      s_t[0][wv] = Ia;
      s_t[1][wv] = Id;
      s_t[2][wv] = Ic;
    }
    __syncthreads();
    u64 b_all = r_all, b_del = r_del;
    u32 b_cnt = r_cnt;
    for (u32 w = 0; w < wv; w++) {
      b_all += s_t[0][w];
      b_del += s_t[1][w];
      b_cnt += s_t[2][w];
    }
    if (wi <= last)
      E.words[base + wi] = EdWord{(u32)b_all + Ia - a_all, a_b0, a_b1, mybm, (u32)b_del + Id - a_del, b_cnt + Ic - a_cnt};
    for (u32 w = 0; w < DIFF_WAVES; w++) {
      r_all += s_t[0][w];
      r_del += s_t[1][w];
      r_cnt += s_t[2][w];
    }
    __syncthreads();  // (the next pass rewrites the LDS totals)
  }
  if (tid == 0) E.res[i] = EdRes{0u, 0u, r_all >= (u64)INVALID ? ED_BAD : 0u, no, 0ull, 0ull};
}

// Units of the orders below o, from the document's records W (o <= next_order, so word o >> 5 has
// one; at a word's first order the mask is empty).  Mod 2^32: the sums of a document with a result
// fit, and only differences are used.
template <u32 ENC>
__device__ __forceinline__ u32 ed_below(const EdWord* W, u32 o) {
  const EdWord& r = W[o >> 5];
  u32 m = (1u << (o & 31u)) - 1u;
  u32 s = r.sa + (u32)__popc(m) + (u32)__popc(r.b0 & m);
  if (ENC == ENC_UTF8) s += 2u * (u32)__popc(r.b1 & m);
  return s;
}
// ... of those whose bitmap bit is clear, and (marked) the set bitmap bits below o
template <u32 ENC>
__device__ __forceinline__ u32 ed_below_clear(const EdWord* W, u32 o, u32& marked) {
  EdWord r = W[o >> 5];
  u32 m = (1u << (o & 31u)) - 1u;
  marked = r.sc + (u32)__popc(r.bm & m);
  m &= ~r.bm;
  u32 s = r.sa - r.sd + (u32)__popc(m) + (u32)__popc(r.b0 & m);
  if (ENC == ENC_UTF8) s += 2u * (u32)__popc(r.b1 & m);
  return s;
}

// One block per listed document, DIFF_T canonical spans per loop pass, in document order: k_diff's
// sweep with units carried next to items.  WRITE = false counts the document's edits and inserted
// units (res[i]); WRITE = true, after k_result_scan, writes them.  Within a pass each thread
// classifies its span (k, d, i) and takes its kept, deleted and inserted units from the index
// (no item loop: ed_below, ed_below_clear); wave scans give the D / I items and units, the new-visible
// units and the patch starts before it, and the waves' totals meet in LDS; the open-patch state and
// the running sums carry from pass to pass in registers.  The start span of edit p writes its pos,
// its unit (new-visible units before it) and its ins_off and, for now, the D / I items and units
// before it into the four length fields; a last sweep over the document's edits turns neighbouring
// starts into lengths.  The inserted items are expanded per wave with lane l on item t + l, as
// k_diff does; their pool is the concatenation of their encodings in document order, so an item's
// first unit is the inserted units before its wave plus a wave scan of the widths.  Every store
// stays below the counts of the first sweep.
template <u32 ENC, bool WRITE>
__global__ __launch_bounds__(DIFF_T) void k_edits(Pools P, PubOut O, EdIO E, u32 n) {
  typedef typename std::conditional<ENC == ENC_UTF8, u8, u16>::type Unit;
  u32 i = blockIdx.x;
  if (i >= n) return;
  EdRes rs = E.res[i];
  if (rs.flags & ED_BAD) return;  // (k_ed_prefix)
  u32 d = E.docs[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  u32 v = E.since[i];
  const DocSeg& sg = P.seg[d];
  u64 cbase = sg.canon_base;
  const Span* cn = O.canon + cbase;
  const u32* vp = O.vpos + cbase;
  u32 ns = min(O.canon_n[d], sg.canon_cap);
  const EdWord* W = E.words + E.bm_base[i];
  const u32* src = E.content + E.cbase[d];
  u32 my_ed = 0, my_un = 0;  // (WRITE) this index's counts from the first pass: every store stays below them
  Edit* ed = nullptr;
  Unit* up = nullptr;
  if (WRITE) {
    my_ed = rs.n_ed; my_un = rs.n_units;
    ed = E.edits + rs.eoff;
    up = (Unit*)E.units + rs.uoff;
  }
  __shared__ u32 s_op[DIFF_WAVES], s_st[DIFF_WAVES], s_d[DIFF_WAVES], s_i[DIFF_WAVES], s_du[DIFF_WAVES], s_iu[DIFF_WAVES],
      s_vu[DIFF_WAVES];
  // carried: a patch is open; edits, D / I items, D / I units and new-visible units so far
  u32 c_open = 0, c_pat = 0, c_del = 0, c_ins = 0, c_du = 0, c_iu = 0, c_vu = 0;
  for (u32 k0 = 0; k0 < ns; k0 += DIFF_T) {
    u32 k = k0 + tid;
    Span sp = k < ns ? cn[k] : Span{0, 0, 0, 0};
    u32 ln = slen(sp);
    u32 below = sp.order < v ? min(ln, v - sp.order) : 0u;  // the span's orders below `since`
    u32 kk = 0, dd = 0, ii = 0, ku = 0, du = 0, iu = 0;
    if (sp.len > 0) {
      kk = below; ii = ln - below;
      u32 u0 = ed_below<ENC>(W, sp.order), u1 = kk ? ed_below<ENC>(W, sp.order + kk) : u0;
      ku = u1 - u0;
      iu = ii ? ed_below<ENC>(W, sp.order + ln) - u1 : 0u;
    } else if (below != 0u) {
      // deleted span: its orders [a, b) below `since` that no earlier delete covers are D items
      u32 ma, mb;
      u32 ua = ed_below_clear<ENC>(W, sp.order, ma), ub = ed_below_clear<ENC>(W, sp.order + below, mb);
      dd = below - (mb - ma);
      du = ub - ua;
    }
    u32 vu = ku + iu;
    bool c = (dd + ii) != 0u, bk = kk != 0u;
    // patch state after each span: content opens (or keeps open) a patch, a K-only span closes it
    u64 mO = ballot(c), mC = ballot(bk && !c);
    u32 Di = wave_incl_scan(dd), Ii = wave_incl_scan(ii);
    u32 DUi = wave_incl_scan(du), IUi = wave_incl_scan(iu), VUi = wave_incl_scan(vu);
    if (l == 63u) {
      s_d[wv] = Di;
      s_i[wv] = Ii;
      s_du[wv] = DUi;
      s_iu[wv] = IUi;
      s_vu[wv] = VUi;
      s_op[wv] = (mO | mC) ? (mO > mC ? 1u : 2u) : 0u;  // (the higher lane decides) 0: no K, D or I item in this wave
    }
    __syncthreads();
    u32 open_in = c_open, d_in = c_del, i_in = c_ins, du_in = c_du, iu_in = c_iu, vu_in = c_vu;
    for (u32 w = 0; w < wv; w++) {
      u32 op = s_op[w];
      if (op) open_in = op == 1u;
      d_in += s_d[w];
      i_in += s_i[w];
      du_in += s_du[w];
      iu_in += s_iu[w];
      vu_in += s_vu[w];
    }
    u64 lower = (1ull << l) - 1ull;
    u64 lo = mO & lower, lc = mC & lower;
    bool open_before = (lo | lc) ? lo > lc : open_in != 0u;
    bool start = c && (bk || !open_before);
    u64 mS = ballot(start);
    if (l == 0u) s_st[wv] = (u32)__popcll(mS);
    __syncthreads();
    if (WRITE) {
      u32 p = c_pat + (u32)__popcll(mS & lower);
      for (u32 w = 0; w < wv; w++) p += s_st[w];
      u32 IUex = iu_in + IUi - iu;  // I units before this span
      if (start && p < my_ed)
        ed[p] = Edit{vp[k] + kk, d_in + Di - dd, i_in + Ii - ii, vu_in + VUi - vu + ku, du_in + DUi - du, IUex, IUex, 0u};
      // the wave's inserted items: lane l takes item t + l of the wave's Tn (its span by a 6-step
      // search over the scan, as in k_diff); the units before it are the inserted units before the
      // wave (iu_in), those of the wave's items before this round (urun) and a scan of the round's widths
      u32 fo = sp.order + kk;  // the span's first inserted order
      u32 st = Ii - ii;        // its first item within the wave
      u32 Tn = rdlane(Ii, 63);
      u32 urun = iu_in;
      for (u32 t = 0; t < Tn; t += 64u) {
        u32 j = t + l;
        u32 s = 0;
#pragma unroll
        for (u32 step = 32u; step >= 1u; step >>= 1) s += shfl(Ii, s + step - 1u) <= j ? step : 0u;
        u32 sfo = shfl(fo, s), sst = shfl(st, s);
        bool act = j < Tn;
        u32 cv = act ? src[sfo + (j - sst)] : 0u;
        u32 w = act ? enc_width_raw<ENC>(cv) : 0u;
        u32 inc = wave_incl_scan(w);
        u32 dst = urun + inc - w;
        urun += rdlane(inc, 63);
        u32 pk = enc_pack<ENC>(enc_scalar(cv));
        for (u32 q = 0; q < w; q++)
          if (dst + q < my_un) up[dst + q] = (Unit)(pk >> (q * (u32)(8u * sizeof(Unit))));
      }
    }
    for (u32 w = 0; w < DIFF_WAVES; w++) {
      u32 op = s_op[w];
      if (op) c_open = op == 1u;
      c_del += s_d[w];
      c_ins += s_i[w];
      c_du += s_du[w];
      c_iu += s_iu[w];
      c_vu += s_vu[w];
      c_pat += s_st[w];
    }
    __syncthreads();  // (the next pass rewrites the LDS totals)
  }
  if (!WRITE) {
    if (tid == 0) E.res[i] = EdRes{c_pat, c_iu, 0u, rs.version, 0ull, 0ull};
    return;
  }
  // the lengths of edit p: the D / I items and units from its start to the next edit's start (the
  // document's totals after the last one).  Each sweep reads its edits and their successors, then
  // writes; the next sweep's edits are untouched until then.
  u32 np = min(c_pat, my_ed);
  __syncthreads();
  for (u32 p0 = 0; p0 < np; p0 += DIFF_T) {
    u32 p = p0 + tid;
    u32 d0 = 0, d1 = 0, i0 = 0, i1 = 0, du0 = 0, du1 = 0, iu0 = 0, iu1 = 0;
    if (p < np) {
      Edit x = ed[p];
      d0 = x.del_len; i0 = x.ins_len; du0 = x.del_units; iu0 = x.ins_units;
      d1 = c_del; i1 = c_ins; du1 = c_du; iu1 = c_iu;
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
