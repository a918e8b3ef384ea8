// Patches between two causal versions given as version vectors (crdt_version_vector,
// crdt_diff_vv_async, include/crdt_gpu.h).  A version vector names, per agent of the document, how
// many of its seqs have been seen; the version is the set S of orders whose id (agent, seq) has
// seq < vv[agent].  An order-prefix version "everything below v" is such a set -- an agent's seqs
// are applied in seq order, so the orders below v hold a seq prefix of every agent (k_vv_of gives
// its vector) -- but a vector also names states that no prefix of this replica's orders is: what
// another replica acknowledged, or now without one author's last txn.
//
// k_vv_mark turns a vector into two order-indexed bitmaps, from client_with_order and the delete
// log; k_diff2_sets is k_diff2's walk (kernels.h d2_walk) with "the orders below from / to"
// replaced by the member bitmaps.
#pragma once
#include "kernels.h"

namespace crdt {

// crdt_version_vector: the vector of the order prefix ver[q] (ver == nullptr: now) of doc[q], one
// block per query, threads take agents: the agent's item_orders runs are in seq order and so in
// order order, so the seqs below the version are a binary search for the first run that starts at
// or above it.  A query without an answer (a document out of range or poisoned, a version above
// the document's, fewer than n_agents entries at vv_off[q]) fills its entries with INVALID.
#define VV_OF_T 64u
__global__ __launch_bounds__(VV_OF_T) void k_vv_of(Pools P, u32 n_docs, u32 nq, const u32* doc, const u32* ver,
                                                   const u64* vv_off, u32* vv_out) {
  u32 q = blockIdx.x;
  if (q >= nq) return;
  u32 d = doc[q];
  u64 off = vv_off[q], room = vv_off[q + 1u] - off;
  bool ok = d < n_docs;
  u32 na = 0, v = 0;
  if (ok) {
    i32 stt = P.st[d].status;
    u32 no = P.st[d].next_order;
    na = min(P.st[d].n_agents, P.seg[d].agent_cap);
    v = ver ? ver[q] : no;
    ok = (stt == ST_OK || stt == ST_NEED_CAPACITY) && v <= no && (u64)na <= room;
  }
  if (!ok) {
    for (u64 a = threadIdx.x; a < room; a += VV_OF_T) vv_out[off + a] = INVALID;
    return;
  }
  const DocSeg& sg = P.seg[d];
  for (u32 a = threadIdx.x; a < na; a += VV_OF_T) {
    AgentRec A = P.agents[sg.agent_base + a];
    const ARun* ar = P.arun + sg.arun_base + A.run_base;
    u32 lo = 0, hi = A.run_cnt;  // the runs that start below v
    while (lo < hi) {
      u32 mid = (lo + hi) >> 1;
      if (ar[mid].order < v) lo = mid + 1u;
      else hi = mid;
    }
    u32 s = 0;
    if (lo) {
      ARun r = ar[lo - 1u];
      s = r.key + min(r.len, v - r.order);
    }
    vv_out[off + a] = s;
  }
}

struct VvIO {
  const u32* docs;     // [i] the listed documents
  const u64* vv_off;   // [i], [i + 1]: the index's vector in vv
  const u32* vv;       // this side's vectors
  const u64* bm_base;  // [i] first word of the index's bitmap pair in bm
  u32* bm;             // member bitmap (bit x = x in S), then, pub_words(ord_cap) words on, the
                       // "deleted by S" bitmap (a delete op with its order in S covers item x)
  u32* flag;           // [i] VV_BAD | VV_CLOSED (kernels.h)
};

// bit x of an order-indexed bitmap
__device__ __forceinline__ bool vv_bit(const u32* bm, u32 x) { return ((bm[x >> 5] >> (x & 31u)) & 1u) != 0u; }

// The three phases on the index's bitmap pair at `mem` (LDS or HBM, zeroed), nw words each.
//   1  threads take client_with_order runs: run (key, agent, seq, len) puts the orders
//      [key, key + clamp(vv[agent] - seq, 0, len)) into the member bitmap, one atomic OR per word.
//   2  threads take delete-log runs (key, target, len): the member bits of [key, key + len) are
//      read a destination word at a time, shifted onto [target, target + len) and OR-ed into the
//      deleted bitmap.  The member part of a run is any subset of it, not a prefix: the log merges
//      delete ops of different txns, and of different agents, whose keys and targets continue.
//   3  closedness: S holds a prefix of every txn it touches -- a member order whose predecessor
//      is no member must be the first order of a txn record (a record is a chain of txns, each
//      the only parent of the next); threads take bitmap words and search the txn of every such
//      rise -- and a txn record whose first order is a member has every parent but ROOT in S
//      (threads take records).  A thread that finds S open sets *s_open (LDS, 0 on entry).
template <bool LDS>
__device__ __forceinline__ void vv_mark_phases(const Pools& P, const DocSeg& sg, const DocState& st, const u32* vv, u32 nv,
                                               u32* mem, u32 nw, u32* s_open) {
  u32 ord_cap = sg.ord_cap;  // > every order: word (ord_cap - 1) >> 5 is inside the bitmaps
  u32* del = mem + nw;
  const CwoRun* cw = P.cwo + sg.cwo_base;
  u32 ncwo = min(st.n_cwo, sg.cwo_cap);
  for (u32 r = threadIdx.x; r < ncwo; r += DIFF_T) {
    CwoRun q = cw[r];
    u32 v = q.agent < nv ? vv[q.agent] : 0u;
    if (v <= q.seq || q.key >= ord_cap) continue;
    u32 m = min(q.len, v - q.seq);
    u32 a = q.key, b = (u32)min((u64)q.key + m, (u64)ord_cap);
    if (a >= b) continue;
    for (u32 w = a >> 5; w <= ((b - 1u) >> 5); w++) atomicOr(&mem[w], range_mask(w, a, b));
  }
  if (!LDS) __threadfence();
  __syncthreads();
  const DelRun* dels = P.dels + sg.del_base;
  u32 nd = min(st.n_del, sg.del_cap);
  for (u32 r = threadIdx.x; r < nd; r += DIFF_T) {
    DelRun q = dels[r];
    if (q.key >= ord_cap || q.order >= ord_cap) continue;
    u32 len = min(q.len, min(ord_cap - q.key, ord_cap - q.order));
    if (!len) continue;
    u32 ta = q.order, tb = q.order + len;
    for (u32 w = ta >> 5; w <= ((tb - 1u) >> 5); w++) {
      u32 lo = max(ta, w << 5), hi = min(tb, (w + 1u) << 5);  // the targets [lo, hi) of word w
      u32 s = q.key + (lo - ta), c = hi - lo;                 // their delete orders [s, s + c), c <= 32
      u32 sw = s >> 5, sh = s & 31u;
      u32 bits = mem[sw] >> sh;
      if (sh + c > 32u) bits |= mem[sw + 1u] << (32u - sh);  // (sh > 0; order s + c - 1 is in word sw + 1)
      if (c < 32u) bits &= (1u << c) - 1u;
      bits <<= lo & 31u;
      if (bits) atomicOr(&del[w], bits);
    }
  }
  const TxnRec* tx = P.txns + sg.txn_base;
  const u32* par = P.parents + sg.par_base;
  u32 ntx = min(st.n_txn, sg.txn_cap);
  bool open = false;
  for (u32 w = threadIdx.x; w < nw; w += DIFF_T) {
    u32 m = mem[w];
    u32 rise = m & ~((m << 1) | (w ? mem[w - 1u] >> 31 : 0u));
    while (rise) {
      u32 x = (w << 5) + (u32)__builtin_ctz(rise);
      rise &= rise - 1u;
      u32 lo = 0, hi = ntx;  // the records that start at or below x
      while (lo < hi) {
        u32 mid = (lo + hi) >> 1;
        if (tx[mid].order <= x) lo = mid + 1u;
        else hi = mid;
      }
      if (!lo || tx[lo - 1u].order != x) open = true;
    }
  }
  for (u32 t = threadIdx.x; t < ntx; t += DIFF_T) {
    TxnRec x = tx[t];
    if (x.order >= ord_cap || !vv_bit(mem, x.order)) continue;
    u32 pn = x.poff <= sg.par_cap ? min(x.pn, sg.par_cap - x.poff) : 0u;
    for (u32 j = 0; j < pn; j++) {
      u32 p = par[x.poff + j];
      if (p != ROOT_ORDER && (p >= ord_cap || !vv_bit(mem, p))) open = true;
    }
  }
  if (open) atomicOr(s_open, 1u);
}

// One block per index, as k_diff_mark, once per side.  A bitmap pair of at most xw words in all
// (the launch's dynamic LDS: the host passes the largest listed pair that fits its budget,
// DIFF_MARK_WORDS or the test hook's cap) is built in LDS and stored whole; a larger one takes
// the atomics in HBM, on words the host zeroed.  An index whose vector is longer than the
// document's agents, or has an entry above the agent's next seq, or whose document is poisoned,
// is marked VV_BAD.
__global__ __launch_bounds__(DIFF_T) void k_vv_mark(Pools P, VvIO V, u32 n, u32 xw) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  u32 d = V.docs[i];
  const DocState& st = P.st[d];
  const DocSeg& sg = P.seg[d];
  __shared__ u32 s_flags[2];  // (static: the whole dynamic budget is bitmap)
  u32* s_bad = &s_flags[0];
  u32* s_open = &s_flags[1];
  u32* s_bm = s_dyn;
  if (threadIdx.x < 2u) s_flags[threadIdx.x] = 0u;
  __syncthreads();
  i32 stt = st.status;
  u64 off = V.vv_off[i], cnt = V.vv_off[i + 1u] - off;
  u32 na = min(st.n_agents, sg.agent_cap);
  bool bad = (stt != ST_OK && stt != ST_NEED_CAPACITY) || cnt > (u64)na;
  const u32* vv = V.vv + off;
  if (!bad) {
    for (u32 a = threadIdx.x; a < (u32)cnt; a += DIFF_T) {
      AgentRec A = P.agents[sg.agent_base + a];
      u32 next = 0;  // the agent's next seq (doc.rs:20-24)
      if (A.run_cnt) {
        ARun r = P.arun[sg.arun_base + A.run_base + A.run_cnt - 1u];
        next = r.key + r.len;
      }
      if (vv[a] > next) atomicOr(s_bad, 1u);
    }
  }
  __syncthreads();
  if (bad || *s_bad) {
    if (threadIdx.x == 0) V.flag[i] = VV_BAD;
    return;
  }
  u32 nw = pub_words(sg.ord_cap);
  u32* bm = V.bm + V.bm_base[i];
  if (2u * nw <= xw) {
    for (u32 w = threadIdx.x; w < 2u * nw; w += DIFF_T) s_bm[w] = 0u;
    __syncthreads();
    vv_mark_phases<true>(P, sg, st, vv, (u32)cnt, s_bm, nw, s_open);
    __syncthreads();
    for (u32 w = threadIdx.x; w < 2u * nw; w += DIFF_T) bm[w] = s_bm[w];
  } else {
    vv_mark_phases<false>(P, sg, st, vv, (u32)cnt, bm, nw, s_open);
    __syncthreads();
  }
  if (threadIdx.x == 0) V.flag[i] = *s_open ? 0u : VV_CLOSED;
}

// k_diff2 with a set of orders on either side (k_vv_mark's bitmap pairs and flags)
struct DiffVvIO {
  Diff2IO e;       // d.bm / bm_b: the two sides' bitmap pairs at d.bm_base; d.since and to are not read
  const u32* fa;   // [i] k_vv_mark's flags of the from side
  const u32* fb;   // ... of the to side
};
template <bool WRITE>
__global__ __launch_bounds__(DIFF_T) void k_diff2_sets(Pools P, PubOut O, DiffVvIO E, u32 n) {
  d2_walk<WRITE, true>(P, O, E.e, n, E.fa, E.fb);
}

}  // namespace crdt
