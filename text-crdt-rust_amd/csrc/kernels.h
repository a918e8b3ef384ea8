// Device kernels of the engine.
//   k_init      ListCRDT::new() per document (wave per document)
//   k_replay    apply the staged record stream (wave per document, replay_core.h)
//   k_relayout_pool  move every document's part of one pool into its re-sized pool (block per document)
//   k_publish   flat index build: canonical spans (can_append compaction of the leaf entries in
//               document order), visible-prefix vpos, order->span scatter, digest
//   k_pub_index the order->span index of k_publish's documents, built in LDS (block per document)
//   k_pos_to_loc / k_loc_to_pos   batched lookups on the published index (thread per query)
//   k_materialize  document text from the published index + content streams (block per document)
//   k_diff_mark / k_diff / k_result_scan  per-document text patches from a past version to now, from
//               the published index + the delete log (block per listed document)
//   k_diff2     (after k_diff_mark twice) the patches between two versions, from the same inputs
//   k_co_rank / k_co_count / k_result_scan / k_co_write  the document at a past version (checkout): its
//               items' orders and text, from the same inputs (block per listed document)
//   k_pos_to_loc_at / k_loc_to_pos_at   the two lookups on a checked-out view (thread per query)
//   k_blame / k_result_scan  authorship runs of the current text, from the published index +
//               client_with_order (block per listed document)
#pragma once
#include "replay_core.h"
#include "wave_gpu.h"
#include "balance_levels.h"

namespace crdt {

struct PubOut {
  Span* canon;    // [canon_base + k]
  u32* vpos;      // [canon_base + k]  visible items before canonical span k
  u32* sorted;    // [canon_base + r]  the canonical spans by first order (rank -> span)
  u32* corder;    // [canon_base + k]  first order of canonical span k (k_pub_index's input: 4 B
                  //                   per span instead of re-reading the 16 B spans)
  u32* pub;       // [pub_base + w]    bit (o & 31) of word o >> 5: a canonical span starts at order o;
                  // [pub_base + pub_words + w]  set bits in words [0, w)
  u32* canon_n;   // [doc]
  u32* len;       // [doc]
  u64* digest;    // [doc]
  u32* stamp;     // [doc]  id of the replay launch whose wave published the document (fused publish:
                  //        publish_doc from replay_doc), 0 = none, STAMP_BIG = a k_publish_big document
};
constexpr u32 STAMP_BIG = 0xFFFFFFFFu;  // (no launch id: the host's counter skips it)

// Order -> canonical span through the published index: r = span starts at or below `order`;
// the span is sorted[r - 1] if it contains the order (delete orders lie in no span).  Returns
// the span index or INVALID.
#ifdef PUB_PLAIN_LOADS
__device__ __forceinline__ u32 ld_l2(const u32* p) { return *p; }
#else
__device__ __forceinline__ u32 ld_l2(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif
__device__ __forceinline__ u32 span_of_order(const PubOut& O, const DocSeg& seg, u32 cn, u32 order) {
  u32 nw = pub_words(seg.ord_cap);
  const u32* bits = O.pub + seg.pub_base;
  u32 wd = order >> 5;
  if (wd >= nw) return INVALID;
  u32 r = bits[nw + wd] + (u32)__popc(bits[wd] & (0xFFFFFFFFu >> (31u - (order & 31u))));
  if (r == 0u || r > cn) return INVALID;
  u32 k = O.sorted[seg.canon_base + r - 1u];
  if (k >= cn) return INVALID;
  Span sp = O.canon[seg.canon_base + k];
  return order - sp.order < slen(sp) ? k : INVALID;
}

#define WAVES_PER_BLOCK 4

// Dynamic LDS of the wave-per-document kernels: each wave's slice (crdt_types.h wave_lds_words):
// the scan's prefetch row, the directory root (flat: 4 x rcap u32; two-level: 3 x rcap + 2) and
// the document's agent ranks (RANK_LDS u32; launch shape: engine.hip launch_shape).
extern __shared__ u32 s_dyn[];
template <int L, bool HR = false>
__device__ __forceinline__ WaveGPU<L, HR> wave_with_root(u32 rcap) {
  WaveGPU<L, HR> w;
  // the LDS address space survives into the member: root accesses are ds_* (lgkmcnt only);
  // a generic pointer would make them flat ops, whose waits also drain every pending store
  w.rcap = rcap;
  u32 root = HR ? 3u * rcap + 2u : 4u * rcap;
  w.pf = (typename WaveGPU<L, HR>::lds_u32*)(s_dyn + uni(threadIdx.x >> 6) * wave_lds_words(rcap, HR));
  w.rt = w.pf + PF_LDS;
  w.rk = w.rt + root;
  return w;
}
// Document of the calling wave: wave k of the launch takes list[k] (or k without a list).
__device__ __forceinline__ u32 wave_doc(u32 wpb, const u32* list, u32 n, u32& d) {
  u32 k = uni(blockIdx.x * wpb + (threadIdx.x >> 6));
  if (k >= n) return 0;
  d = list ? uni(list[k]) : k;
  return 1;
}

template <int L>
__global__ __launch_bounds__(256) void k_init(Pools P, u32 n, u32 wpb, u32 rcap) {
  u32 d;
  if (!wave_doc(wpb, nullptr, n, d)) return;
  Replayer<WaveGPU<L>, L> r(P, d, wave_with_root<L>(rcap));
  r.init_empty();
  AgentRec* ag = r.agents();
  for (u32 a = lane_id(); a < r.g(S_N_AGENTS); a += 64) ag[a].run_cnt = 0;
  r.finish();
}

// n: waves of this launch (documents in `list`, or the first n documents)
// Register budget: 8 waves per SIMD (<= 64 VGPRs, <= 80 SGPRs).  Each document is one dependent
// chain, so resident waves are what hides its latencies: 8 waves/SIMD replays 8,192 automerge-paper
// documents in 185 ms where the compiler's own choice (84 VGPRs: 5 waves/SIMD) takes 199 ms and
// 97 VGPRs (4 waves/SIMD) took 216 ms (scripts/gpu_ab.sh).  What the budget costs is a few spills
// in cold paths.
// k_replay's arguments, one struct: the kernel-argument segment then has this layout, and the
// fused publish (publish_tail) reads its part from the segment when it runs.  O, xw, pub_id are
// never read as kernel arguments, so the replay loop carries none of them in registers.
// pub_id != 0: every wave publishes its document after finish() and stamps it with pub_id, the
// host's id of this launch (k_publish skips the documents so stamped); 0: no fused publish.
// bal_*: the progress balance (balance_board_tick below), read from the segment at every tick.
struct ReplayArgs {
  Pools P;
  u32 n, wpb, rcap;
  const u32* list;
  PubOut O;
  u32 xw, pub_id;
  u32* bal_board;  // [BAL_ROWS][BAL_SLOTS]
  u32 bal_stamp;   // this launch's stamp, 1..255
  u32 bal_mode;    // BAL_*
  u64 bal_table;   // BAL_ROTATE's level map (balance_levels.h balance_table)
};
template <int L>
__device__ __forceinline__ void publish_tail(const DocState* stp);
__device__ __forceinline__ void balance_done();

template <int L, bool HR, u32 SH = SHAPE_ALL, bool FUSE = false, bool DEC = false>
__device__ __forceinline__ void replay_doc(Pools P, u32 n, u32 wpb, u32 rcap, const u32* list) {
  u32 d;
  if (!wave_doc(wpb, list, n, d)) return;
#ifdef CRDT_PROF
  const u32 life_t0 = (u32)__builtin_amdgcn_s_memrealtime();  // (prof_mode 4: wave lifetimes)
#endif
  static_assert(!DEC || (!HR && SH == SHAPE_REMOTE), "the window decode is built into the remote-only instance");
  Replayer<WaveGPU<L, HR>, L, DEC> r(P, d, wave_with_root<L, HR>(rcap));
  WaveGPU<L, HR>& w = r.w;
  if (r.status() == ST_NEED_CAPACITY) r.p(S_STATUS, (u32)ST_OK);  // resume after growth
  if (r.status() != ST_OK || r.g(S_REC_POS) >= r.rec_n()) {
    w.st((u32*)&P.st[d].status, (u32)r.status());
    if constexpr (!HR) balance_done();
    return;
  }
  r.begin();
  r.template run<SH>();
  r.finish();
#ifdef CRDT_PROF
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // (finish()'s stores have left the wave)
  const u32 life_t1 = (u32)__builtin_amdgcn_s_memrealtime();
#endif
  // (whatever ended run(): the stream's end or any stop status)
  if constexpr (!HR) balance_done();
  if constexpr (FUSE) publish_tail<L>(r.stp());  // (the document from its state pointer: d need not live through the loop)
#ifdef CRDT_PROF
  if (r.prof_mode == 4u) {
    // over the path counters: start and end (after finish()) on the 100 MHz real-time counter,
    // HW_ID, and XCC_ID (bits 0-3) with the ticks the fused publish then took above it (<< 4)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    const u32 tail = (u32)__builtin_amdgcn_s_memrealtime() - life_t1;
    w.st(&P.st[d].prof0, life_t0);
    w.st(&P.st[d].prof1, life_t1);
    w.st(&P.st[d].prof2, (u32)__builtin_amdgcn_s_getreg(4 | (31 << 11)));
    w.st(&P.st[d].prof3, ((u32)__builtin_amdgcn_s_getreg(20 | (31 << 11)) & 15u) | (tail << 4));
  }
#endif
}
#ifndef CRDT_REPLAY_WAVES
#define CRDT_REPLAY_WAVES 8  // waves per SIMD the replay's register budget is held to (diagnostic builds vary it)
#endif
// SH: the stream shape of every document of the launch (crdt_types.h SHAPE_*; the host launches
// each shape's documents in their own instance: SHAPE_ALL is the general one)
#ifndef CRDT_REPLAY_WAVES_GEN
#define CRDT_REPLAY_WAVES_GEN CRDT_REPLAY_WAVES  // (the generated-op instance's budget; diagnostic builds vary it)
#endif
template <int L, u32 SH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SH == SHAPE_GEN ? CRDT_REPLAY_WAVES_GEN : CRDT_REPLAY_WAVES))) void k_replay(ReplayArgs A) {
  replay_doc<L, false, SH, true>(A.P, A.n, A.wpb, A.rcap, A.list);
}
// k_replay<L, SHAPE_REMOTE> reading typing runs from the decoded record window (wave_gpu.h
// decode_window).  Remote-only streams have both kernels and the host picks one per launch
// (crdt_set_window_decode): the switch costs the replay loop nothing, where a mode word read in the
// kernel cost registers.  Same register budget (crdt_amd CODEGEN_LIMITS).
template <int L>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CRDT_REPLAY_WAVES))) void k_replay_dec(ReplayArgs A) {
  replay_doc<L, false, SHAPE_REMOTE, true, true>(A.P, A.n, A.wpb, A.rcap, A.list);
}
// Documents past the LDS root replay with the two-level root (wave_gpu.h HR).  They are few and
// long, so this instance is held to 4 waves per SIMD (<= 128 VGPRs: no scratch for its extra
// root state) instead of the batch kernel's 8.
template <int L>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_replay_hr(Pools P, u32 n, u32 wpb, u32 rcap, const u32* list) {
  replay_doc<L, true>(P, n, wpb, rcap, list);
}

// crdt_reseed_random_async: every document whose staged stream is one GEN record (crdt_stage_random)
// gets the generator seed of document id_base + d, (u32)mix64(seed ^ (id_base + d)) -- the seed
// crdt_stage_random gives document d for id_base 0 -- so one engine replays the batches of a
// larger corpus (BASELINE config 4: 1 M documents) without restaging.  Other documents are untouched.
__global__ void k_reseed_gen(Pools P, u32 n, u64 seed, u64 id_base) {
  u32 d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n) return;
  DocSeg sg = P.seg[d];
  if (sg.rec_n != 1u) return;
  Rec* r = const_cast<Rec*>(P.recs + sg.rec_base);  // (the staged record pool: read-only to the replay)
  if (rec_kind(*r) != REC_GEN) return;
  r->w3 = (u32)mix64(seed ^ (id_base + d));
}

// Reset the per-call record cursor of every document (new stream staged).
__global__ void k_reset_recpos(DocState* st, u32 n, u32 n_agents_dummy) {
  u32 d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d < n) st[d].rec_pos = 0;
}

// Host-side agent counts into every document's state (before k_init / a replay).
__global__ void k_set_n_agents(DocState* st, const u32* na, u32 n) {
  u32 d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d < n) st[d].n_agents = na[d];
}

template <class T>
__device__ __forceinline__ void bcopy(T* dst, const T* src, u64 n) {
  for (u64 k = threadIdx.x; k < n; k += blockDim.x) dst[k] = src[k];
}

// Move one pool of document state into re-sized pools (growth / re-staging / fit; engine.hip layout: the pools move one at a time, each freed
// before the next is allocated, so a relayout needs the old pools + the largest new one, not both
// sets).  Block per document.  src / dst differ only in the pool being moved (and, for
// RL_ARUN, in the agent tables: src.agents the old one, dst.agents the new one with its run
// bases); RL_AGENTS moves the agents' run counts and last-run copies into the new table.
enum : u32 { RL_LEAVES, RL_SOL, RL_DIR_LEAF, RL_DIR_VIS, RL_LEAF_OF, RL_AGENT_OF, RL_CWO, RL_DELS, RL_DD, RL_DDB,
             RL_TXNS, RL_PARENTS, RL_FRONTIER, RL_GROUPS, RL_ARUN, RL_AGENTS, RL_N };
template <int L>
__global__ __launch_bounds__(256) void k_relayout_pool(Pools src, Pools dst, const DocSeg* old_seg, const u32* new_n_agents, u32 n,
                                                       u32 which) {
  u32 d = blockIdx.x;
  if (d >= n) return;
  DocState s = dst.st[d];
  DocSeg o = old_seg[d];
  DocSeg w = dst.seg[d];
  switch (which) {
    case RL_LEAVES: bcopy(dst.leaves + w.leaf_base * L, src.leaves + o.leaf_base * L, (u64)s.n_leaves * L); break;
    case RL_SOL: bcopy(dst.slot_of_leaf + 2 * w.leaf_base, src.slot_of_leaf + 2 * o.leaf_base, 2ull * s.n_leaves); break;
    case RL_DIR_LEAF: bcopy(dst.dir_leaf + w.blk_base * GROUP, src.dir_leaf + o.blk_base * GROUP, (u64)s.n_blocks * GROUP); break;
    case RL_DIR_VIS: bcopy(dst.dir_vis + w.blk_base * GROUP, src.dir_vis + o.blk_base * GROUP, (u64)s.n_blocks * GROUP); break;
    case RL_LEAF_OF:
      if (w.flags & o.flags & DOC_TRACK_MAP) bcopy(dst.leaf_of + w.map_base, src.leaf_of + o.map_base, s.next_order);
      break;
    case RL_AGENT_OF:
      if (w.flags & o.flags & DOC_TRACK_AGENT) bcopy(dst.agent_of + w.map_base, src.agent_of + o.map_base, s.next_order);
      break;
    case RL_CWO: bcopy(dst.cwo + w.cwo_base, src.cwo + o.cwo_base, s.n_cwo); break;
    case RL_DELS: bcopy(dst.dels + w.del_base, src.dels + o.del_base, s.n_del); break;
    case RL_DD: bcopy(dst.dd + w.dd_base * DD_BLK, src.dd + o.dd_base * DD_BLK, (u64)s.n_ddb * DD_BLK); break;
    case RL_DDB: bcopy(dst.ddb + w.dd_base, src.ddb + o.dd_base, s.n_ddb); break;
    case RL_TXNS: bcopy(dst.txns + w.txn_base, src.txns + o.txn_base, s.n_txn); break;
    case RL_PARENTS: bcopy(dst.parents + w.par_base, src.parents + o.par_base, s.n_par); break;
    case RL_FRONTIER: bcopy(dst.frontier + w.fr_base, src.frontier + o.fr_base, s.n_fr); break;
    case RL_GROUPS: bcopy(dst.groups + w.grp_base, src.groups + o.grp_base, s.ng); break;
    case RL_ARUN:
      for (u32 a = 0; a < s.n_agents; a++) {
        AgentRec ao = src.agents[o.agent_base + a];
        AgentRec an = dst.agents[w.agent_base + a];
        bcopy(dst.arun + w.arun_base + an.run_base, src.arun + o.arun_base + ao.run_base, ao.run_cnt);
      }
      break;
    case RL_AGENTS:
      for (u32 a = threadIdx.x; a < s.n_agents; a += blockDim.x) {
        AgentRec ao = src.agents[o.agent_base + a];  // (run base / cap: the new layout's)
        AgentRec* q = dst.agents + w.agent_base + a;
        q->run_cnt = ao.run_cnt;
        q->tkey = ao.tkey;
        q->torder = ao.torder;
        q->tlen = ao.tlen;
      }
      __syncthreads();
      if (threadIdx.x == 0) dst.st[d].n_agents = new_n_agents[d];
      break;
  }
}

// Order -> leaf map of documents that start keeping it (their first remote stream after local
// ones): INVALID everywhere, then every entry's orders -> its leaf, in directory order.  Block per
// listed document; the barrier orders the two sweeps' stores.
template <int L>
__global__ __launch_bounds__(256) void k_build_map(Pools P, const u32* docs, u32 n) {
  if (blockIdx.x >= n) return;
  u32 d = docs[blockIdx.x];
  DocState s = P.st[d];
  DocSeg sg = P.seg[d];
  u32* lof = P.leaf_of + sg.map_base;
  for (u64 o = threadIdx.x; o < s.next_order; o += blockDim.x) lof[o] = INVALID;
  __syncthreads();
  const GroupRec* gr = P.groups + sg.grp_base;
  const Span* lv = P.leaves + sg.leaf_base * L;
  for (u32 g = 0; g < s.ng; g++) {
    GroupRec G = gr[g];
    for (u32 i = 0; i < G.cnt; i++) {
      u32 leaf = P.dir_leaf[(sg.blk_base + G.blk) * GROUP + i];
      for (u32 e = 0; e < (u32)L; e++) {
        Span sp = lv[(u64)leaf * L + e];
        for (u32 t = threadIdx.x; t < slen(sp); t += blockDim.x) lof[sp.order + t] = leaf;
      }
    }
  }
}

// Order -> agent map of documents that start keeping it (a second agent appears in a tracked
// document that already holds state): every client_with_order run's orders -> its agent.
__global__ __launch_bounds__(256) void k_build_agent_map(Pools P, const u32* docs, u32 n) {
  if (blockIdx.x >= n) return;
  u32 d = docs[blockIdx.x];
  DocState s = P.st[d];
  DocSeg sg = P.seg[d];
  u16* oag = P.agent_of + sg.map_base;
  const CwoRun* cw = P.cwo + sg.cwo_base;
  for (u32 k = 0; k < s.n_cwo; k++) {
    CwoRun r = cw[k];  // (the last run's length is current: the replay's tails were flushed)
    for (u32 t = threadIdx.x; t < r.len; t += blockDim.x) oag[r.key + t] = (u16)r.agent;
  }
}

// ---------------------------------------------------------------------------------------------
// digest helpers (identical to oracle/crdt_oracle.hpp)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 elem_hash(u32 section, u64 idx, u64 a, u64 b) {
  u64 k = mix64(((u64)section << 56) ^ idx);
  return mix64(mix64(k ^ a) ^ b);
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
  for (u32 off = 32; off >= 1; off >>= 1) {
    u32 lo = (u32)v, hi = (u32)(v >> 32);
    u32 src = lane_id() ^ off;
    u32 olo = shfl(lo, src), ohi = shfl(hi, src);
    v += ((u64)ohi << 32) | olo;
  }
  return v;
}

// ---------------------------------------------------------------------------------------------
// k_publish: the flat index of every document (canonical spans in document order, visible prefix,
// order -> span index, digest).  One wave per document (k_publish), or for long documents one
// workgroup of PUB_BIG_WAVES waves (k_publish_big): the leaf sequence is cut into one range per
// wave, each wave compacts its range, the spans that cross range boundaries are resolved once,
// and the index sweeps are split over the waves.
// ---------------------------------------------------------------------------------------------
#ifndef PUB_DEPTH
#define PUB_DEPTH 1  // compaction steps whose leaf loads are in flight at once (compact_range)
#endif
#ifndef PUB_TAIL_DEPTH
#define PUB_TAIL_DEPTH 3  // the same for a replay wave's own publish (publish_tail): the waves of a SIMD end one
                          // after the other, so a publishing wave has the memory system nearly to itself
#endif
#define PUB_BIG_WAVES 16
#define PUB_BIG_MIN 2048u        // leaves from which a document may publish with a workgroup ...
#define PUB_BIG_FEW_DOCS 1024u   // ... when the batch has at most this many documents
#define PUB_BIG_MAX 16384u       // leaves from which it always does

// A published document whose digest k_digest has not computed yet (publish writes it; k_digest
// replaces it)
constexpr u64 DIGEST_PENDING = 1ull;
// Digest term of canonical span k (section 1; oracle/crdt_oracle.hpp digest()).
__device__ __forceinline__ u64 span_hash(u32 k, const Span& sp) {
  return elem_hash(1, k, ((u64)sp.order << 32) | sp.ol, ((u64)sp.orr << 32) | (u32)sp.len);
}

// What one wave's leaf range contributes (k_publish_big boundary resolution).
struct RangeSum {
  u32 spans;      // canonical spans starting in the range (its first entry counts as a start)
  u32 vis;        // visible items
  u32 single;     // the whole range is one span
  i32 lead_len;   // signed length of the range's first span inside the range
  Span first, last;  // first and last raw entries
};

// Canonical compaction of leaves [a, b) (directory order) by one wave, lane i = entry i of a leaf:
// an entry starts a new span unless YjsSpan::can_append(previous entry, entry) (span.rs:47-53;
// merging is transitive, so the previous raw entry stands for the open span); span lengths are
// segmented sums of a prefix scan; the span still open at a leaf's end carries over (uniform
// registers).  WRITE: spans go to canon/vpos from index `out` with visible offsets from `vis`;
// skip_first: the range's first span continues the previous range's (not written); extra: the
// signed length the range's last span continues by in later ranges.  !WRITE: fill `sum`.
// Every written span's first order also goes to corder.
// DEPTH: compaction steps whose leaf loads are in flight at once (PUB_DEPTH for the publish kernels,
// whose 8 waves per SIMD walk together; PUB_TAIL_DEPTH for a replay wave's own publish).
template <int L, bool WRITE, int DEPTH = PUB_DEPTH>
__device__ __forceinline__ void compact_range(const Pools& P, const DocSeg& seg, u32 ng, u32 a, u32 b, Span* canon,
                                              u32* vpos, u32* corder, u32 ccap, u32& out, u32& vis, u32 skip_first,
                                              i32 extra, RangeSum& sum) {
  const u32 l = lane_id();
  const Span* leaves = P.leaves + seg.leaf_base * L;
  const GroupRec* groups = P.groups + seg.grp_base;  // the root level, read in order from HBM
  const u32 vis0 = vis;
  u32 have = 0, skip = skip_first, nsp = 0, first_done = 0;
  Span open{0, 0, 0, 0};
  u32 open_vpos = 0;
  // the group holding leaf a: prefix of the groups' slot counts
  u32 g = 0, base = 0;
  if (a) {
    for (u32 r = 0; r < ng; r += 64) {
      u32 c = r + l < ng ? groups[r + l].cnt : 0u;
      u32 incl = wave_incl_scan(c);
      u32 k = (u32)__popcll(ballot(r + l < ng && incl + base <= a));
      if (k < 64u && r + k < ng) { g = r + k; base += k ? rdlane(incl, k - 1u) : 0u; break; }
      base += rdlane(incl, 63);
    }
  }
  for (u32 idx = a; g < ng && idx < b; g++) {
    u32 blk = uni(groups[g].blk), cnt = uni(groups[g].cnt);
    u32 i0 = idx - base;        // first slot of this group in the range
    base += cnt;
    if (i0 >= cnt) continue;
    u32 iend = b - (base - cnt) < cnt ? b - (base - cnt) : cnt;  // slot bound in this group
    u32 mydl = P.dir_leaf[(seg.blk_base + blk) * GROUP + l];  // 64-slot row: always in bounds
    // 64/L leaves per step: lane l holds entry l%L of leaf i + l/L; the valid entries (packed at
    // the front of each leaf) are then compacted to lanes [0, nn) with one ds_permute, so the
    // scan below sees one contiguous run of entries in document order.  Software pipeline: the
    // next step's loads are in flight while this step is scanned and its spans stored (vmcnt
    // counts stores too, so an unpipelined load would wait behind them).
    constexpr u32 PER = 64u / (u32)L;
    u32 sub = l / (u32)L;
    // (lane-parallel conditions below are bitwise, not short-circuit: && on per-lane values
    // compiles to exec-masked branches; the load is unconditional from a valid leaf, then masked)
    // (the masking happens when the step uses the entries, so a prefetched load is not waited for)
    auto ld = [&](u32 i) -> uint4 {
      u32 li = i + sub;
      u32 leaf = shfl(mydl, li < iend ? li : 0u);
      return *(const uint4*)(leaves + (u64)leaf * L + (l & (u32)(L - 1)));
    };
    // DEPTH steps of loads in flight (Little's law: one wave's 1 KiB per step is too little to
    // cover HBM latency at 8 waves per SIMD)
    uint4 vn = ld(i0);
    uint4 vn2{0, 0, 0, 0}, vn3{0, 0, 0, 0};
    if constexpr (DEPTH >= 2) {
      if (i0 + PER < iend) vn2 = ld(i0 + PER);
    }
    if constexpr (DEPTH >= 3) {
      if (i0 + 2u * PER < iend) vn3 = ld(i0 + 2u * PER);
    }
    for (u32 i = i0; i < iend; i += PER) {
      uint4 v = vn;
      {  // lanes of leaves past the group's range: empty
        bool in = i + sub < iend;
        v = uint4{in ? v.x : 0u, in ? v.y : 0u, in ? v.z : 0u, in ? v.w : 0u};
      }
      if constexpr (DEPTH >= 3) {
        vn = vn2;
        vn2 = vn3;
        if (i + 3u * PER < iend) vn3 = ld(i + 3u * PER);
      } else if constexpr (DEPTH >= 2) {
        vn = vn2;
        if (i + 2u * PER < iend) vn2 = ld(i + 2u * PER);
      } else {
        if (i + PER < iend) vn = ld(i + PER);
      }
      u64 VM = ballot(v.w != 0u);
      u32 nn = (u32)__popcll(VM);
      if (PER > 1) {
        u64 below = (1ull << l) - 1ull;
        u32 c1 = (u32)__popcll(VM & below);  // (valid entries below this lane; the empty ones are l - c1)
        u32 dst = v.w != 0u ? c1 : nn + l - c1;
        int ad = (int)(dst << 2);
        v.x = (u32)__builtin_amdgcn_ds_permute(ad, (int)v.x);
        v.y = (u32)__builtin_amdgcn_ds_permute(ad, (int)v.y);
        v.z = (u32)__builtin_amdgcn_ds_permute(ad, (int)v.z);
        v.w = (u32)__builtin_amdgcn_ds_permute(ad, (int)v.w);
      }
      if (nn == 0u) continue;
      bool valid = l < nn;
      Span e{v.x, v.y, v.z, (i32)v.w};
      u32 px = shfl(v.x, l - 1u), py = shfl(v.y, l - 1u), pz = shfl(v.z, l - 1u), pw = shfl(v.w, l - 1u);
      Span prev = l == 0u ? sum.last : Span{px, py, pz, (i32)pw};
      bool app = valid & ((l != 0u) | (have != 0u)) & can_append_b(prev, e);
      bool start = valid & !app;
      u64 M = ballot(start);
      u32 len_u = valid ? v.w : 0u;
      u32 Pl = wave_incl_scan(len_u);  // signed lengths, two's complement sums
      u32 cl = valid && (i32)v.w > 0 ? v.w : 0u;
      u32 V = wave_incl_scan(cl);
      u32 leaf_vis = rdlane(V, 63);
      u64 above = M & ~((2ull << l) - 1ull);
      u32 nxt = above ? (u32)__builtin_ctzll(above) : nn;
      u32 p_end = shfl(Pl, nxt - 1u);
      i32 glen = (i32)(p_end - (Pl - len_u));  // span starting at this lane: lanes [l, nxt)
      u32 fs = M ? (u32)__builtin_ctzll(M) : nn;
      if (have && fs) open.len += (i32)rdlane(Pl, fs - 1u);
      if (!first_done) {
        if (!have) sum.first = Span{rdlane(v.x, 0), rdlane(v.y, 0), rdlane(v.z, 0), (i32)rdlane(v.w, 0)};
      }
      if (M) {
        if (have) {  // the open span closes
          if (!first_done) { sum.lead_len = open.len; first_done = 1; }
          if (WRITE) {
            if (skip) skip = 0;
            else {
              if (l == 0u && out < ccap) {
                canon[out] = open; vpos[out] = open_vpos; corder[out] = open.order;
              }
              out++;
            }
          }
        }
        u32 ls = 63u - (u32)__builtin_clzll(M);
        u32 rank = (u32)__popcll(M & ((1ull << l) - 1ull));
        u32 firsts = (u32)__popcll(M) - 1u;  // spans that also close in this step
        if (!first_done && firsts) { sum.lead_len = (i32)rdlane((u32)glen, fs); first_done = 1; }
        if (WRITE) {
          u32 sk = skip && firsts ? 1u : 0u;  // the skipped first span is the step's first start
          if (start && l != ls && rank >= sk && out + rank - sk < ccap) {
            Span sp{v.x, v.y, v.z, glen};
            canon[out + rank - sk] = sp;
            vpos[out + rank - sk] = vis + V - cl;
            corder[out + rank - sk] = v.x;
          }
          out += firsts - sk;
          if (sk) skip = 0;
        }
        nsp += (u32)__popcll(M);
        open = Span{rdlane(v.x, ls), rdlane(v.y, ls), rdlane(v.z, ls), (i32)rdlane((u32)glen, ls)};
        open_vpos = vis + rdlane(V - cl, ls);
        have = 1;
      }
      sum.last = Span{rdlane(v.x, nn - 1u), rdlane(v.y, nn - 1u), rdlane(v.z, nn - 1u), (i32)rdlane(v.w, nn - 1u)};
      vis += leaf_vis;
    }
    idx = base;
  }
  if (have) {
    if (!first_done) { sum.lead_len = open.len; sum.single = 1; }
    else sum.single = 0;
    if (WRITE && !skip) {
      open.len += extra;
      if (l == 0 && out < ccap) {
        canon[out] = open; vpos[out] = open_vpos; corder[out] = open.order;
      }
      out++;
    }
  }
  sum.spans = nsp;
  sum.vis = vis - vis0;
}

// Order -> canonical span index (replaces a 4 B/order table): a bitmap over the
// orders with a bit at every canonical span's first order, the exclusive count of set bits before
// every word, and the spans listed by first order.  Three sweeps: set the bits (atomic OR: spans
// are in document order, not order order), prefix-count the words, scatter every span to its
// rank.  Per document 2 bits per order + 4 B per span are written instead of 4 B per item order.
// Reads go through L2 (ld_l2): other lanes wrote them.  Wave `wv` of `nwv` takes every nwv-th
// chunk; the word prefix is one contiguous word range per wave plus a cross-wave carry (lds_c:
// nwv u32 of LDS, k_publish_big only).
template <int NWV>
__device__ __forceinline__ void publish_index(const PubOut& O, const DocSeg& seg, const DocState& s, const Span* canon,
                                              u32 out, u32 wv, u32* lds_c) {
  const u32 l = lane_id();
#ifdef PUB_NO_INDEX
  const u32 nw = pub_words(seg.ord_cap), used = 0u;
#else
  const u32 nw = pub_words(seg.ord_cap), used = s.next_order / 32u + 1u;
#endif
  u32* bits = O.pub + seg.pub_base;
  u32* pre = bits + nw;
  u32* sorted = O.sorted + seg.canon_base;
  for (u32 i = wv * 64u + l; i < used; i += 64u * NWV) bits[i] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (NWV > 1) __syncthreads();
  for (u32 k0 = wv * 64u; k0 < out; k0 += 64u * NWV) {
    u32 k = k0 + l;
    Span sp = k < out ? canon[k] : Span{0, 0, 0, 0};
#ifndef PUB_NO_INDEX
    // nearby spans share bitmap words: OR each distinct word's bits across the wave first, then
    // one atomic per word (same-address atomics serialise at L2)
    u32 wd = sp.order >> 5, bit = 1u << (sp.order & 31u);
    for (u64 todo = ballot(k < out); todo;) {
      u32 wl = rdlane(wd, (u32)__builtin_ctzll(todo));
      u64 m = ballot(k < out && wd == wl);
      u32 word = wave_or((m >> l) & 1u ? bit : 0u);
      if (l == (u32)__builtin_ctzll(m)) atomicOr(bits + wl, word);
      todo &= ~m;
    }
#endif
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  // word prefix: this wave's contiguous word range [wa, wb), 4 steps per iteration (their loads
  // in flight together)
  const u32 per_wave = ((used + NWV - 1u) / NWV + 63u) & ~63u;
  const u32 wa = wv * per_wave < used ? wv * per_wave : used, wb = wa + per_wave < used ? wa + per_wave : used;
  u32 carry = 0;
  if (NWV > 1) {
    __syncthreads();  // every wave's atomics are done
    u32 t = 0;
    for (u32 i = wa + l; i < wb; i += 64) t += (u32)__popc(ld_l2(bits + i));
    t = wave_sum(t);
    if (l == 0) lds_c[wv] = t;
    __syncthreads();
    u32 c = l < wv ? lds_c[l] : 0u;
    carry = wave_sum(c);
  }
  for (u32 i0 = wa; i0 < wb; i0 += 256) {
    u32 x[4];
#pragma unroll
    for (u32 u = 0; u < 4; u++) {
      u32 i = i0 + 64 * u + l;
      x[u] = i < wb ? (u32)__popc(ld_l2(bits + i)) : 0u;
    }
#pragma unroll
    for (u32 u = 0; u < 4; u++) {
      u32 i = i0 + 64 * u + l;
      u32 incl = wave_incl_scan(x[u]);
      if (i < wb) pre[i] = carry + incl - x[u];
      carry += rdlane(incl, 63);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (NWV > 1) __syncthreads();
#ifndef PUB_NO_INDEX
  for (u32 k0 = wv * 256u; k0 < out; k0 += 256u * NWV) {
    u32 o[4], r[4];
#pragma unroll
    for (u32 u = 0; u < 4; u++) {
      u32 k = k0 + 64 * u + l;
      o[u] = k < out ? canon[k].order : 0u;
    }
#pragma unroll
    for (u32 u = 0; u < 4; u++) {
      u32 wd = o[u] >> 5;
      r[u] = ld_l2(pre + wd) + (u32)__popc(ld_l2(bits + wd) & ((1u << (o[u] & 31u)) - 1u));
    }
#pragma unroll
    for (u32 u = 0; u < 4; u++) {
      u32 k = k0 + 64 * u + l;
      if (k < out) sorted[r[u]] = k;
    }
  }
#endif
}

// The digest's other sections (client_with_order, deletes, double deletes, txns + parents,
// frontier) by one wave, and the counts.  Identical to oracle/crdt_oracle.hpp digest().
template <int L>
__device__ __forceinline__ u64 digest_tables(const Pools& P, const DocSeg& seg, const DocState& s, WaveGPU<L>& w) {
  const u32 l = lane_id();
  u64 h = 0;
  const CwoRun* cwo = P.cwo + seg.cwo_base;
  for (u32 k = l; k < s.n_cwo; k += 64) {
    CwoRun r = cwo[k];
    h += elem_hash(2, k, ((u64)r.key << 32) | r.agent, ((u64)r.seq << 32) | r.len);
  }
  const DelRun* dels = P.dels + seg.del_base;
  for (u32 k = l; k < s.n_del; k += 64) {
    DelRun r = dels[k];
    h += elem_hash(3, k, ((u64)r.key << 32) | r.order, r.len);
  }
  const DDRun* dd = P.dd + seg.dd_base * DD_BLK;  // blocks in directory order = the flat RLE
  const DDBlk* ddb = P.ddb + seg.dd_base;
  for (u32 lb = 0, k0 = 0; lb < s.n_ddb; lb++) {
    DDBlk B = w.ldT(ddb + lb);
    if (l < B.cnt) {
      DDRun r = dd[(u64)B.phys * DD_BLK + l];
      h += elem_hash(4, k0 + l, ((u64)r.key << 32) | r.len, r.excess);
    }
    k0 += B.cnt;
  }
  const TxnRec* tx = P.txns + seg.txn_base;
  const u32* par = P.parents + seg.par_base;
  for (u32 k = l; k < s.n_txn; k += 64) {
    TxnRec t = tx[k];
    h += elem_hash(5, k, ((u64)t.order << 32) | t.len, ((u64)t.shadow << 32) | t.pn);
    for (u32 j = 0; j < t.pn; j++) h += elem_hash(6, t.poff + j, par[t.poff + j], k);
  }
  const u32* fr = P.frontier + seg.fr_base;
  for (u32 k = l; k < s.n_fr; k += 64) h += elem_hash(7, k, fr[k], 0);
  return h;
}
__device__ __forceinline__ u64 digest_counts(const DocState& s, u32 out) {
  u64 counts = elem_hash(8, 0, ((u64)s.len << 32) | out, ((u64)s.n_cwo << 32) | s.n_del);
  return counts ^ elem_hash(9, 0, ((u64)s.n_dd << 32) | s.n_txn, ((u64)s.n_fr << 32) | s.n_par);
}

// One wave publishes document d (k_publish; publish_tail: the wave that replayed it).
// xw: documents whose bitmap has at most xw words get their order -> span index from k_pub_index
// (launched next); the others build it here.
template <int L, int DEPTH = PUB_DEPTH>
__device__ __forceinline__ void publish_doc(const Pools& P, const PubOut& O, u32 d, u32 xw, u32 stamp) {
  WaveGPU<L> w;
  DocState s = w.ldT(P.st + d);
  DocSeg seg = w.ld_seg(P.seg + d);
  u32 l = lane_id();
  if ((s.status != ST_OK && s.status != ST_NEED_CAPACITY) || s.next_order >= seg.ord_cap) {
    if (l == 0) { O.canon_n[d] = 0; O.len[d] = s.len; O.digest[d] = 0; O.stamp[d] = stamp; }
    return;
  }
  Span* canon = O.canon + seg.canon_base;
  u32* vpos = O.vpos + seg.canon_base;
  u32 out = 0, vis = 0;
  RangeSum sum{};
  compact_range<L, true, DEPTH>(P, seg, s.ng, 0u, s.n_leaves, canon, vpos, O.corder + seg.canon_base, seg.canon_cap,
                                out, vis, 0u, 0, sum);
  if (out > seg.canon_cap) {  // canonical spans beyond the planned capacity: report, never write past it
    if (l == 0) { O.canon_n[d] = 0; O.len[d] = s.len; O.digest[d] = 0; O.stamp[d] = stamp; }
    return;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (pub_words(seg.ord_cap) > xw) publish_index<1>(O, seg, s, canon, out, 0u, nullptr);
  if (l == 0) {
    O.canon_n[d] = out;
    O.len[d] = s.len;
    O.digest[d] = DIGEST_PENDING;  // (k_digest computes it on request)
    O.stamp[d] = stamp;
  }
}
// The replay wave's publish of its own document, after finish() (fused publish; replay_doc).  What
// finish() stored -- the state by lanes, the tables' tails, the root groups -- is read back here by
// other lanes of the same wave: the fence orders those stores before the loads, as the kernel
// boundary does for k_publish.  Documents of the k_publish_big list (STAMP_BIG) stay with it.
// The replay's registers are dead here; so that the tail adds nothing to what the replay loop
// keeps live (k_replay's 8-waves-per-SIMD budget), it takes its arguments from the kernel-argument
// segment now (ReplayArgs) -- through a pointer the compiler cannot trace back to the segment, or it
// would merge these loads with the kernel's own at entry and carry the values through the loop.
typedef const __attribute__((address_space(4))) u32* karg_u32;
template <class T>
__device__ __forceinline__ T ld_karg(karg_u32 kp, size_t off) {
  static_assert(sizeof(T) % 4 == 0, "dwords");
  T t;
  u32* o = (u32*)&t;
#pragma unroll
  for (u32 k = 0; k < sizeof(T) / 4; k++) o[k] = kp[off / 4 + k];
  return t;
}
template <int L>
__device__ __forceinline__ void publish_tail(const DocState* stp) {
  karg_u32 kp = (karg_u32)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("; publish_tail: kernel-argument segment pointer" : "+s"(kp));
  const u32 pub_id = ld_karg<u32>(kp, offsetof(ReplayArgs, pub_id));
  if (!pub_id) return;
  const Pools P = ld_karg<Pools>(kp, offsetof(ReplayArgs, P));
  const PubOut O = ld_karg<PubOut>(kp, offsetof(ReplayArgs, O));
  const u32 d = uni((u32)(stp - P.st));
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  if (uni(O.stamp[d]) == STAMP_BIG) return;
  publish_doc<L, PUB_TAIL_DEPTH>(P, O, d, ld_karg<u32>(kp, offsetof(ReplayArgs, xw)), pub_id);
}

// ---------------------------------------------------------------------------------------------
// Progress balance of k_replay's waves.  The eight waves of a SIMD start together, but its issue
// arbiter picks by priority, then by age: at equal priority the oldest wave wins every contested
// slot, equal documents end one after the other, and the last ones replay alone at the speed of one
// dependent chain.  So every wave sets its own priority (s_setprio, 0..3) where its
// record window moves (Replayer::rec_window, about once per 64 records; the generated-op loop's
// refill), from the work it has left:
//   BAL_BOARD   longest remaining first.  The waves of a SIMD come from different workgroups, so
//               they meet in a global board: one row per SIMD (XCC_ID and HW_ID's SE / SH / CU /
//               SIMD fields), one slot per HW_ID.WAVE_ID, slot = launch stamp << 24 | records left.
//               A tick stores the wave's slot, reads the row past the CU's L1, ranks itself among
//               the slots with this launch's stamp and something left, and takes the level of its
//               rank: the wave that fell behind is promoted at the next tick.  Slots of other
//               launches do not match the stamp (no clearing between launches); a wave that ends
//               writes "nothing left" (balance_done).  No wave waits for another's value: a stale
//               or missing slot only makes a rank slightly wrong.
//   BAL_ROTATE  the levels rotate over the wave ids in time slices of the real-time counter: no
//               memory traffic, removes the age order of equal documents, blind to unequal ones.
//               Which wave ids tie at a level in a slice is the level map's choice
//               (balance_levels.h, ReplayArgs::bal_table).
// Everything is read from the kernel-argument segment at the tick (as publish_tail does) and dies
// in it: the replay loop carries nothing for it in registers.
// ---------------------------------------------------------------------------------------------
constexpr u32 BAL_ROWS = 1u << 14, BAL_SLOTS = 16u, BAL_LEFT_MAX = 0xFFFFFFu;
enum : u32 { BAL_OFF = 0, BAL_BOARD = 1, BAL_ROTATE = 2 };
#ifndef BAL_ROTATE_SHIFT
#define BAL_ROTATE_SHIFT 13  // time slice of BAL_ROTATE: 2^13 ticks of the 100 MHz counter = 82 us, a few window moves
#endif
typedef __attribute__((address_space(1))) u32 bal_u32;  // (global_load / global_store, never flat)

__device__ __forceinline__ karg_u32 balance_kargs() {
  karg_u32 kp = (karg_u32)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("; balance: kernel-argument segment pointer" : "+s"(kp));
  return kp;
}
// This wave's slot: every index field is masked to its width, so the slot lies inside the board
// whatever the registers hold.
__device__ __forceinline__ bal_u32* balance_row(karg_u32 kp, u32 hw) {
  const u32 xcc = (u32)__builtin_amdgcn_s_getreg(20 | (31 << 11)) & 15u;      // XCC_ID
  const u32 row = (xcc << 10) | (((hw >> 8) & 0xFFu) << 2) | ((hw >> 4) & 3u);  // SE, SH, CU | SIMD
  static_assert((15u << 10 | 0xFFu << 2 | 3u) == BAL_ROWS - 1u, "row key bits");
  return (bal_u32*)ld_karg<u32*>(kp, offsetof(ReplayArgs, bal_board)) + row * BAL_SLOTS;
}
// s_setprio takes an immediate and ignores EXEC: a four-way branch on a wave-uniform level
__device__ __forceinline__ void balance_setprio(u32 level) {
  level = uni(level);
  asm("" : "+s"(level));  // (an SGPR value: s_cmp + s_cbranch around each s_setprio)
  if (level == 0u) __builtin_amdgcn_s_setprio(0);
  else if (level == 1u) __builtin_amdgcn_s_setprio(1);
  else if (level == 2u) __builtin_amdgcn_s_setprio(2);
  else __builtin_amdgcn_s_setprio(3);
}
__device__ __forceinline__ void balance_board_tick(u32 remaining) {
  karg_u32 kp = balance_kargs();
  const u32 mode = ld_karg<u32>(kp, offsetof(ReplayArgs, bal_mode));
  if (mode == BAL_OFF) return;
  const u32 hw = (u32)__builtin_amdgcn_s_getreg(4 | (31 << 11));  // HW_ID: WAVE_ID in bits 0-3
  if (mode == BAL_ROTATE) {
    // (the level map's table: kernel-argument words, read here and dead after the level; SGPR arithmetic)
    const u64 table = ld_karg<u64>(kp, offsetof(ReplayArgs, bal_table));
    balance_setprio(balance_level_in(table, (u32)(__builtin_amdgcn_s_memrealtime() >> BAL_ROTATE_SHIFT), hw));
    return;
  }
  bal_u32* row = balance_row(kp, hw);
  const u32 slot = hw & (BAL_SLOTS - 1u);
  const u32 stamp = ld_karg<u32>(kp, offsetof(ReplayArgs, bal_stamp)) << 24;
  const u32 mine = stamp | (remaining < BAL_LEFT_MAX ? remaining : BAL_LEFT_MAX);
  const u32 l = lane_here();
  if (l == 0u) __hip_atomic_store(row + slot, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // lane k < 16 reads slot k (the others re-read one of them and are masked); the wave's own slot
  // counts from its register, not from the load (another lane's store may not be visible yet)
  const u32 v = __hip_atomic_load(row + (l & (BAL_SLOTS - 1u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool live = (l < BAL_SLOTS) & (l != slot) & ((v ^ stamp) - 1u < BAL_LEFT_MAX);  // this launch's, something left
  const bool ahead = live & ((v > mine) | ((v == mine) & (l < slot)));                 // (ties: the lower slot first)
  const u32 n = (u32)__popcll(ballot(live)) + 1u, rank = (u32)__popcll(ballot(ahead));
  // rank 0 (most left) -> level 3; up to 4 waves one level each, up to 8 two, up to 16 four per level
  const u32 r = rank >> (n > 8u ? 2u : n > 4u ? 1u : 0u);
  balance_setprio(3u - (r < 3u ? r : 3u));
}
// A wave leaves the replay (the stream's end, any stop status, nothing to do): nothing left, and
// priority 0 again, so the waves' publish tails run as peers.
__device__ __forceinline__ void balance_done() {
  karg_u32 kp = balance_kargs();
  const u32 mode = ld_karg<u32>(kp, offsetof(ReplayArgs, bal_mode));
  if (mode == BAL_OFF) return;
  if (mode == BAL_BOARD) {
    const u32 hw = (u32)__builtin_amdgcn_s_getreg(4 | (31 << 11));
    bal_u32* row = balance_row(kp, hw);
    const u32 stamp = ld_karg<u32>(kp, offsetof(ReplayArgs, bal_stamp)) << 24;
    if (lane_here() == 0u) __hip_atomic_store(row + (hw & (BAL_SLOTS - 1u)), stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __builtin_amdgcn_s_setprio(0);
}

// pub_id: the host's id of the last replay launch; a document its replay wave published
// (stamp == pub_id) is current, the wave returns at once.
// (8 waves per SIMD need <= 80 SGPRs: unconstrained, the compiler took 102, i.e. 6 waves per SIMD and
// 8,192 documents in 1.33 rounds)
template <int L>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_publish(Pools P, PubOut O, u32 n, const u32* list, u32 xw, u32 pub_id) {
  u32 d;
  if (!wave_doc(WAVES_PER_BLOCK, list, n, d)) return;
  if (uni(O.stamp[d]) == pub_id) return;
  publish_doc<L>(P, O, d, xw, 0u);
}

// Long documents: one workgroup of PUB_BIG_WAVES waves per listed document.
template <int L>
__global__ __launch_bounds__(64 * PUB_BIG_WAVES) void k_publish_big(Pools P, PubOut O, const u32* list) {
  constexpr u32 NWV = PUB_BIG_WAVES;
  __shared__ RangeSum s_sum[NWV];
  __shared__ u32 s_base[NWV], s_vbase[NWV], s_skip[NWV], s_c[NWV], s_total;
  __shared__ i32 s_extra[NWV];
  const u32 d = list[blockIdx.x];
  const u32 l = lane_id(), wv = uni(threadIdx.x >> 6);
  WaveGPU<L> w;
  DocState s = w.ldT(P.st + d);
  DocSeg seg = w.ld_seg(P.seg + d);
  if ((s.status != ST_OK && s.status != ST_NEED_CAPACITY) || s.next_order >= seg.ord_cap) {
    if (threadIdx.x == 0) { O.canon_n[d] = 0; O.len[d] = s.len; O.digest[d] = 0; }
    return;
  }
  Span* canon = O.canon + seg.canon_base;
  u32* vpos = O.vpos + seg.canon_base;
  // this wave's leaves (every range holds leaves: the host sends only documents with many)
  const u32 a = (u32)((u64)s.n_leaves * wv / NWV), b = (u32)((u64)s.n_leaves * (wv + 1u) / NWV);
  u32 out = 0, vis = 0;
  RangeSum sum{};
  u32* corder = O.corder + seg.canon_base;
  compact_range<L, false>(P, seg, s.ng, a, b, canon, vpos, corder, seg.canon_cap, out, vis, 0u, 0, sum);
  if (l == 0) s_sum[wv] = sum;
  __syncthreads();
  if (wv == 0) {  // boundary resolution, lane = range
    RangeSum me = s_sum[l < NWV ? l : 0u];
    Span prv = s_sum[l > 0u && l <= NWV ? l - 1u : 0u].last;
    u32 merge = l > 0u && l < NWV && can_append(prv, me.first);
    u32 cnt = l < NWV ? me.spans - merge : 0u;
    u32 ci = wave_incl_scan(cnt), vi = wave_incl_scan(l < NWV ? me.vis : 0u);
    if (l < NWV) { s_base[l] = ci - cnt; s_vbase[l] = vi - me.vis; s_skip[l] = merge; }
    if (l == 0) s_total = rdlane(ci, NWV - 1u);
    // extra_r = merge_{r+1} ? lead_{r+1} + (single_{r+1} ? extra_{r+1} : 0) : 0, from the last range back
    i32 extra = 0;
    for (i32 r = (i32)NWV - 1; r >= 0; r--) {
      u32 mr = rdlane(merge, (u32)r + 1u < NWV ? (u32)r + 1u : 0u) & ((u32)r + 1u < NWV);
      i32 nx = (i32)rdlane((u32)me.lead_len, (u32)r + 1u < NWV ? (u32)r + 1u : 0u);
      u32 sg = rdlane(me.single, (u32)r + 1u < NWV ? (u32)r + 1u : 0u);
      extra = mr ? nx + (sg ? extra : 0) : 0;
      if (l == 0) s_extra[r] = extra;
    }
  }
  __syncthreads();
  out = s_base[wv];
  vis = s_vbase[wv];
  RangeSum sum2{};
  compact_range<L, true>(P, seg, s.ng, a, b, canon, vpos, corder, seg.canon_cap, out, vis, s_skip[wv], s_extra[wv],
                         sum2);
  const u32 total = s_total;
  if (total > seg.canon_cap) {
    if (threadIdx.x == 0) { O.canon_n[d] = 0; O.len[d] = s.len; O.digest[d] = 0; }
    return;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  publish_index<NWV>(O, seg, s, canon, total, wv, s_c);
  if (threadIdx.x == 0) {
    O.canon_n[d] = total;
    O.len[d] = s.len;
    O.digest[d] = DIGEST_PENDING;  // (k_digest computes it on request)
  }
}

// k_digest: the 64-bit state digest of every published document (oracle/crdt_oracle.hpp digest():
// canonical spans, then the RLE tables and the counts), one wave per document, run on request
// (crdt_digest, crdt_digest_dev_async) after a publish -- the digest is the parity checker's
// summary of a state, not part of the flat index the queries read, so publish does not compute
// it.  Documents publish refused (not OK, or past their planned index capacity) keep digest 0.
template <int L>
__global__ __launch_bounds__(256) void k_digest(Pools P, PubOut O, u32 n) {
  u32 d;
  if (!wave_doc(WAVES_PER_BLOCK, nullptr, n, d)) return;
  if (O.digest[d] != DIGEST_PENDING) return;
  WaveGPU<L> w;
  DocState s = w.ldT(P.st + d);
  DocSeg seg = w.ld_seg(P.seg + d);
  const u32 l = lane_id();
  const u32 out = O.canon_n[d];
  const Span* canon = O.canon + seg.canon_base;
  u64 h = 0;
  for (u32 k = l; k < out; k += 64) h += span_hash(k, canon[k]);
  h += digest_tables<L>(P, seg, s, w);
  h = wave_sum64(h);
  if (l == 0) O.digest[d] = mix64(h ^ digest_counts(s, out));
}

// ---------------------------------------------------------------------------------------------
// k_pub_index: the order -> span index (publish_index's three sweeps) of the documents k_publish
// left it to, one PUBX_THREADS block per document, with the bitmap in LDS: the bits are set with
// LDS atomics (ds_or) instead of one global atomic per distinct word, and the word prefix and the
// scatter's ranks read LDS instead of L2.  Global traffic per document: the span first orders
// (corder, 4 B per span) twice, the bitmap and its word prefix written once, the rank -> span
// table scattered once.  LDS: xw bitmap words + an exclusive prefix per 8-word group.
// ---------------------------------------------------------------------------------------------
#define PUBX_THREADS 256
#define PUBX_MAX_WORDS 16384u  // bitmaps up to 524,288 orders (72 KiB of LDS: two blocks per CU)
CRDT_HD u32 pubx_lds_bytes(u32 xw) { return (xw + xw / 8u + 1u) * 4u; }

__global__ __launch_bounds__(PUBX_THREADS) void k_pub_index(Pools P, PubOut O, const u32* list, u32 xw) {
  extern __shared__ u32 xl[];
  __shared__ u32 s_w[PUBX_THREADS / 64];
  u32* lb = xl;       // [xw] bitmap
  u32* lg = xl + xw;  // [xw / 8 + 1] set bits in the 8-word groups before each group
  const u32 d = list ? list[blockIdx.x] : blockIdx.x;
  const u32 t = threadIdx.x;
  const DocState* sp = P.st + d;
  const DocSeg seg = P.seg[d];
  const i32 status = sp->status;
  const u32 next_order = sp->next_order;
  if ((status != ST_OK && status != ST_NEED_CAPACITY) || next_order >= seg.ord_cap) return;
  const u32 nw = pub_words(seg.ord_cap);
  if (nw > xw) return;  // k_publish built this one
  const u32 out = O.canon_n[d];  // 0 when k_publish refused the document
  const u32 used = next_order / 32u + 1u;  // <= nw
  const u32* co = O.corder + seg.canon_base;
  u32* bits = O.pub + seg.pub_base;
  u32* pre = bits + nw;
  u32* sorted = O.sorted + seg.canon_base;
  for (u32 i = t; i < used; i += PUBX_THREADS) lb[i] = 0u;
  __syncthreads();
  // (corder sweeps 8 loads per thread at a time: one dependent HBM wait per 8 spans, not per span)
  for (u32 k0 = t; k0 < out; k0 += 8u * PUBX_THREADS) {
    u32 ov[8];
#pragma unroll
    for (u32 u = 0; u < 8u; u++) {
      u32 k = k0 + u * PUBX_THREADS;
      ov[u] = k < out ? co[k] : INVALID;
    }
#pragma unroll
    for (u32 u = 0; u < 8u; u++)
      if (ov[u] != INVALID) atomicOr(lb + (ov[u] >> 5), 1u << (ov[u] & 31u));
  }
  __syncthreads();
  // group prefix: thread t owns groups [g0, g1)
  const u32 ngr = (used + 7u) / 8u, per = (ngr + PUBX_THREADS - 1u) / PUBX_THREADS;
  const u32 g0 = t * per < ngr ? t * per : ngr, g1 = g0 + per < ngr ? g0 + per : ngr;
  u32 c = 0;
  for (u32 i = g0 * 8u; i < g1 * 8u && i < used; i++) c += (u32)__popc(lb[i]);
  const u32 incl = wave_incl_scan(c);
  if ((t & 63u) == 63u) s_w[t >> 6] = incl;
  __syncthreads();
  u32 run = incl - c;
  for (u32 wv = 0; wv < (t >> 6); wv++) run += s_w[wv];
  for (u32 g = g0; g < g1; g++) {
    lg[g] = run;
    for (u32 i = g * 8u; i < g * 8u + 8u && i < used; i++) run += (u32)__popc(lb[i]);
  }
  __syncthreads();
  // the bitmap and its word prefix, written once (coalesced)
  for (u32 i = t; i < used; i += PUBX_THREADS) {
    u32 r = lg[i >> 3];
    for (u32 j = i & ~7u; j < i; j++) r += (u32)__popc(lb[j]);
    bits[i] = lb[i];
    pre[i] = r;
  }
  // rank -> span
  for (u32 k0 = t; k0 < out; k0 += 8u * PUBX_THREADS) {
    u32 ov[8];
#pragma unroll
    for (u32 u = 0; u < 8u; u++) {
      u32 k = k0 + u * PUBX_THREADS;
      ov[u] = k < out ? co[k] : INVALID;
    }
#pragma unroll
    for (u32 u = 0; u < 8u; u++) {
      u32 o = ov[u];
      if (o == INVALID) continue;
      u32 wd = o >> 5;
      u32 r = lg[wd >> 3];
      for (u32 j = wd & ~7u; j < wd; j++) r += (u32)__popc(lb[j]);
      r += (u32)__popc(lb[wd] & ((1u << (o & 31u)) - 1u));
      sorted[r] = k0 + u * PUBX_THREADS;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Text materialisation.  The reference keeps a rope in step with the tree when
// USE_INNER_ROPE is on: insert the content at cursor.count_pos() (doc.rs:230-233), remove the
// deleted visible range (doc.rs:430-432; the remote delete arm is todo!() at doc.rs:329-333).
// The rope therefore always equals "content of the visible items in document order", which is
// what this kernel writes from the published index: for canonical span k with len > 0,
// text[vpos[k] + i] = content[order_k + i].  Content is an order-indexed UTF-32 table (entries at
// delete orders are never read).
// ---------------------------------------------------------------------------------------------
#define NO_CONTENT 0xFFFFFFFFFFFFFFFFull

struct TextIO {
  const u32* content;  // order-indexed code points: document d reads content[cbase[d] + order]
  const u64* cbase;    // [doc] (NO_CONTENT: no content staged)
  const u64* clen;     // [doc] entries available from cbase
  u32* text;           // [ord_base + pos]
  u32* tlen;           // [doc] visible chars written, INVALID if not materialised
  u64* tdigest;        // [doc] text digest (0 if not materialised)
};

// text digest, identical in oracle/crdt_oracle.hpp (text_digest): a 32-bit murmur3 finaliser per
// (position, code point), summed in 64 bits, mixed once at the end (full-rate-friendly: two 32-bit
// multiplies per char instead of a 64-bit splitmix)
__device__ __forceinline__ u32 text_hash(u32 pos, u32 cp) {
  u32 h = (pos * 0x9E3779B1u) ^ cp;
  h ^= h >> 16; h *= 0x85EBCA6Bu;
  h ^= h >> 13; h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

// One block (MAT_WAVES waves) per document; wave w takes chunks w, w+MAT_WAVES, ... of 64
// canonical spans (each chunk's output starts at vpos[k0], so chunks are independent).  Within a
// chunk a prefix scan of the visible lengths gives each output position j; lane l owns positions
// t+l and finds its span through LDS start flags (below), so stores are fully coalesced
// (contiguous positions) and loads are contiguous within a span.  U positions per lane are in
// flight per step.
#define MAT_WAVES 4
template <int L>
__global__ __launch_bounds__(64 * MAT_WAVES) void k_materialize(Pools P, PubOut O, TextIO T, u32 n) {
  u32 d = blockIdx.x;
  if (d >= n) return;
  u32 l = lane_id();
  u32 wv = uni(threadIdx.x >> 6);
  __shared__ u64 s_h[MAT_WAVES];
  i32 stt = P.st[d].status;
  u32 next_order = P.st[d].next_order;
  u64 cb = T.cbase[d], cl = T.clen[d];
  if ((stt != ST_OK && stt != ST_NEED_CAPACITY) || cb == NO_CONTENT || cl < (u64)next_order) {
    if (threadIdx.x == 0) { T.tlen[d] = INVALID; T.tdigest[d] = 0; }
    return;
  }
  DocSeg seg = P.seg[d];
  const Span* cn = O.canon + seg.canon_base;
  const u32* vp = O.vpos + seg.canon_base;
  u32 ns = O.canon_n[d];
  const u32* src = T.content + cb;
  u32* dst = T.text + seg.ord_base;
  constexpr u32 U = 4;
  // span of output position j: spans with visible items flag their first position in a 64-slot
  // LDS row per window (tag = step number, no clearing) together with base = order - start;
  // position j takes the highest flag at or below it, else the last span starting at or before
  // the window (a uniform readlane).  Two LDS writes, one ballot and one LDS read per window
  // instead of a 6-step bpermute search.
  __shared__ u32 s_tag[MAT_WAVES][U][64], s_base[MAT_WAVES][U][64];
#pragma unroll
  for (u32 u = 0; u < U; u++) s_tag[wv][u][l] = ~0u;
  u32 tag = 0;
  u64 h = 0;
  for (u32 k0 = wv * 64; k0 < ns; k0 += 64 * MAT_WAVES) {
    u32 k = k0 + l;
    Span sp = k < ns ? cn[k] : Span{0, 0, 0, 0};
    u32 ln = sp.len > 0 ? (u32)sp.len : 0u;
    u32 base = uni(vp[k0]);
    u32 Pi = wave_incl_scan(ln);
    u32 Tn = rdlane(Pi, 63);
    u32 st = Pi - ln;            // first output position of span k within the chunk
    u32 ob = sp.order - st;      // content index of position j in span k = ob + j
    for (u32 t = 0; t < Tn; t += 64 * U) {
      ++tag;
#pragma unroll
      for (u32 u = 0; u < U; u++) {
        u32 tu = t + u * 64;
        if (ln > 0 && st >= tu && st - tu < 64u) {
          s_tag[wv][u][st - tu] = tag;
          s_base[wv][u][st - tu] = ob;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      u32 cp[U], jj[U];
#pragma unroll
      for (u32 u = 0; u < U; u++) {
        u32 tu = t + u * 64;
        u32 j = tu + l;
        u64 hm = ballot(s_tag[wv][u][l] == tag) & ((2ull << l) - 1ull);
        u64 B0 = ballot(ln > 0 && st <= tu);
        u32 lt = B0 ? 63u - (u32)__builtin_clzll(B0) : 0u;
        u32 b = hm ? s_base[wv][u][63u - (u32)__builtin_clzll(hm)] : rdlane(ob, lt);
        jj[u] = j;
        cp[u] = j < Tn ? src[b + j] : 0u;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
      for (u32 u = 0; u < U; u++) {
        if (jj[u] < Tn) {
          dst[base + jj[u]] = cp[u];
          h += text_hash(base + jj[u], cp[u]);
        }
      }
    }
  }
  h = wave_sum64(h);
  if (l == 0) s_h[wv] = h;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 hs = 0;
    for (u32 w = 0; w < MAT_WAVES; w++) hs += s_h[w];
    u32 len = O.len[d];
    T.tlen[d] = len;
    T.tdigest[d] = mix64(hs ^ ((u64)len << 32 | 0x54ull));
  }
}

// ---------------------------------------------------------------------------------------------
// Per-document diff (crdt_diff_async): the patches that turn a document's text at version `since`
// (every insert item and delete op with order < since applied) into its current text, from the
// published index and the delete log.  No reference counterpart: the reference's rope arm for
// remote deletes is todo!() (doc.rs:329-333), so a caller of apply_remote_txn cannot learn what
// changed.  Walk the items in document order; an item with order x is
//   old-visible: x < since and no delete-log run covers it with a delete order < since;
//   new-visible: its canonical span has len > 0.
// K (both) closes the current patch, D (old only) adds to its del_len, I (new only) appends to
// its inserted items, N (neither) is ignored.  A patch is a maximal run of D and I items; its pos
// is the number of new-visible items before it.
//
// Per canonical span this is closed form.  A visible span is never in the delete log, so it is
// K^k I^i with k = its orders below `since`; a deleted span is D^d with d = its orders below
// `since` whose bit in the "deleted before since" bitmap (k_diff_mark) is clear, the rest N.
// A patch starts at a span with d + i > 0 that has k > 0 or whose last predecessor with any K, D
// or I item ended on a K; patch p's del_len / ins_len are the D / I items between its start and
// the next patch's start.
// ---------------------------------------------------------------------------------------------
struct Patch { u32 pos, del_len, ins_len, ins_off; };  // crdt_patch (include/crdt_gpu.h)
constexpr u32 DIFF_BAD = 1u;    // since > version, or a poisoned document: no result for this index
constexpr u32 DIFF_TEXT = 2u;   // ins_text was written (the document has content for all its orders)
struct DiffRes {
  u32 n_pat, n_ins, flags, version;
  u64 poff, ioff;  // first patch / first inserted item of this index in the result arrays (k_result_scan)
};
struct DiffIO {
  const u32* docs;     // [i] the listed documents
  const u32* since;    // [i]
  const u64* bm_base;  // [i] first word of the index's bitmap in bm
  u32* bm;             // bit (x & 31) of word x >> 5: a delete op with order < since covers item x
                       // (pub_words(ord_cap) words per index, zeroed per call)
  DiffRes* res;        // [i]
  Patch* patches;      // [res[i].poff + p]
  u32* ins_order;      // [res[i].ioff + j]
  u32* ins_text;       // [res[i].ioff + j]
  const u32* content;  // TextIO's content streams
  const u64* cbase;
  const u64* clen;
};
#define DIFF_T 256u       // threads per document: k_diff walks DIFF_T canonical spans per loop pass
#define DIFF_WAVES 4u
#define DIFF_LONG 256u    // deleted spans with more orders below `since` are counted by the whole wave

// bits [a, b) that fall into word w (a < b; the range's words are a >> 5 .. (b - 1) >> 5)
__device__ __forceinline__ u32 range_mask(u32 w, u32 a, u32 b) {
  u32 lo = w == (a >> 5) ? (a & 31u) : 0u;
  u32 hi = w == ((b - 1u) >> 5) ? ((b - 1u) & 31u) : 31u;
  return (0xFFFFFFFFu << lo) & (0xFFFFFFFFu >> (31u - hi));
}

// The delete log's runs with key < since, clipped at since (a run that straddles it counts with
// its part below), scattered into the index's order-indexed bitmap: lanes take runs, one atomic
// OR of the combined mask per word.  A bitmap of at most xw words (the launch's dynamic LDS; the
// host passes the largest listed bitmap up to DIFF_MARK_WORDS) is built in LDS and stored whole;
// a larger one takes the atomics in HBM, on words the host zeroed.  (8,192 AP documents, half
// the log: 7.5 ms with every atomic in HBM.)
#define DIFF_MARK_WORDS 16384u  // 64 KiB of LDS: bitmaps up to 524,256 orders
__global__ __launch_bounds__(DIFF_T) void k_diff_mark(Pools P, DiffIO D, u32 n, u32 xw) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  u32 d = D.docs[i];
  i32 stt = P.st[d].status;
  u32 no = P.st[d].next_order, v = D.since[i];
  if ((stt != ST_OK && stt != ST_NEED_CAPACITY) || v > no) return;
  const DocSeg& sg = P.seg[d];
  u32 ord_cap = sg.ord_cap;  // > every order: word (ord_cap - 1) >> 5 is inside the bitmap
  u32 nw = pub_words(ord_cap);
  const DelRun* dels = P.dels + sg.del_base;
  u32* bm = D.bm + D.bm_base[i];
  // the runs with key < since: the log is in key order
  u32 lo = 0, hi = min(P.st[d].n_del, sg.del_cap);
  while (lo < hi) {
    u32 mid = (lo + hi) >> 1;
    if (dels[mid].key < v) lo = mid + 1u;
    else hi = mid;
  }
  u32 nd = lo;
  bool in_lds = nw <= xw;
  if (in_lds) {
    for (u32 w = threadIdx.x; w < nw; w += DIFF_T) s_dyn[w] = 0u;
    __syncthreads();
  }
  for (u32 r = threadIdx.x; r < nd; r += DIFF_T) {
    DelRun q = dels[r];
    if (q.key >= v || q.order >= ord_cap) continue;
    u32 m = min(q.len, v - q.key);
    u32 a = q.order, b = (u32)min((u64)q.order + m, (u64)ord_cap);
    if (a >= b) continue;
    if (in_lds) {
      for (u32 w = a >> 5; w <= ((b - 1u) >> 5); w++) atomicOr(&s_dyn[w], range_mask(w, a, b));
    } else {
      for (u32 w = a >> 5; w <= ((b - 1u) >> 5); w++) atomicOr(&bm[w], range_mask(w, a, b));
    }
  }
  if (in_lds) {
    __syncthreads();
    for (u32 w = threadIdx.x; w < nw; w += DIFF_T) bm[w] = s_dyn[w];
  }
}

// Exclusive scan of the indexes' result counts into their result offsets, shared by every result
// pass (one block; thread t takes a contiguous slice of the indexes; thread 0 scans the slices'
// sums serially); totals[j] = the sum of counter j over all indexes.  A result type Res with
// SCAN_K<Res> counters gives its counts with scan_counts(res, c) -- 0 for an index without a
// result, whether its count field is 0 (CoRes, BlameRes) or INVALID -- and takes its offsets
// with scan_store(res, off); both stand next to the type.
#define DIFF_SCAN_T 1024u
template <class Res>
constexpr u32 SCAN_K = 1;
template <class Res>
__global__ __launch_bounds__(DIFF_SCAN_T) void k_result_scan(Res* res, u32 n, u64* totals) {
  constexpr u32 K = SCAN_K<Res>;
  __shared__ u64 s_a[K][DIFF_SCAN_T];
  u32 t = threadIdx.x;
  u32 per = (n + DIFF_SCAN_T - 1u) / DIFF_SCAN_T;
  u64 lo = min((u64)t * per, (u64)n), hi = min(lo + per, (u64)n);
  u64 a[K] = {}, c[K];
  for (u64 k = lo; k < hi; k++) {
    scan_counts(res[k], c);
    for (u32 j = 0; j < K; j++) a[j] += c[j];
  }
  for (u32 j = 0; j < K; j++) s_a[j][t] = a[j];
  __syncthreads();
  if (t == 0) {
    for (u32 j = 0; j < K; j++) {
      u64 s = 0;
      for (u32 x = 0; x < DIFF_SCAN_T; x++) {
        u64 p = s_a[j][x];
        s_a[j][x] = s;
        s += p;
      }
      totals[j] = s;
    }
  }
  __syncthreads();
  for (u32 j = 0; j < K; j++) a[j] = s_a[j][t];
  for (u64 k = lo; k < hi; k++) {
    scan_counts(res[k], c);
    scan_store(res[k], a);
    for (u32 j = 0; j < K; j++) a[j] += c[j];
  }
}
// the diff's two counters: patches and inserted items
template <>
constexpr u32 SCAN_K<DiffRes> = 2;
__device__ __forceinline__ void scan_counts(const DiffRes& r, u64* c) { c[0] = r.n_pat; c[1] = r.n_ins; }
__device__ __forceinline__ void scan_store(DiffRes& r, const u64* off) { r.poff = off[0]; r.ioff = off[1]; }

// One block per listed document, DIFF_T canonical spans per loop pass, in document order.
// WRITE = false counts the document's patches and inserted items (res[i]); WRITE = true, after
// k_result_scan, writes them.  Within a pass each thread classifies its span (k, d, i above), wave
// scans give the D / I items and patch starts before it, and the waves' totals meet in LDS; the
// "is a patch open" state, the patch count and the D / I counts carry from pass to pass in
// registers (every thread folds the same LDS totals).  The start span of patch p writes its pos,
// its ins_off and, for now, the D items before it into ins_len; a last sweep over the document's
// patches turns neighbouring starts into del_len and ins_len.
template <bool WRITE>
__global__ __launch_bounds__(DIFF_T) void k_diff(Pools P, PubOut O, DiffIO D, u32 n) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  u32 d = D.docs[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  i32 stt = P.st[d].status;
  u32 no = P.st[d].next_order, v = D.since[i];
  u64 cb = D.cbase[d], cl = D.clen[d];
  bool text = cb != NO_CONTENT && cl >= (u64)no;
  if ((stt != ST_OK && stt != ST_NEED_CAPACITY) || v > no) {
    if (!WRITE && tid == 0) D.res[i] = DiffRes{0u, 0u, DIFF_BAD, no, 0ull, 0ull};
    return;
  }
  const DocSeg& sg = P.seg[d];
  u64 cbase = sg.canon_base;
  const Span* cn = O.canon + cbase;
  const u32* vp = O.vpos + cbase;
  u32 ns = min(O.canon_n[d], sg.canon_cap);
  const u32* bm = D.bm + D.bm_base[i];
  u32 my_pat = 0, my_ins = 0;  // (WRITE) this index's counts from the first pass: every store stays below them
  Patch* pat = nullptr;
  u32* io = nullptr;
  u32* it = nullptr;
  if (WRITE) {
    DiffRes rs = D.res[i];
    my_pat = rs.n_pat; my_ins = rs.n_ins;
    pat = D.patches + rs.poff;
    io = D.ins_order + rs.ioff;
    it = D.ins_text + rs.ioff;
  }
  const u32* src = D.content + (text ? cb : 0ull);
  __shared__ u32 s_op[DIFF_WAVES], s_d[DIFF_WAVES], s_i[DIFF_WAVES], s_st[DIFF_WAVES];
  u32 c_open = 0, c_pat = 0, c_del = 0, c_ins = 0;  // carried: a patch is open; patches, D and I items so far
  for (u32 k0 = 0; k0 < ns; k0 += DIFF_T) {
    u32 k = k0 + tid;
    Span sp = k < ns ? cn[k] : Span{0, 0, 0, 0};
    u32 ln = slen(sp);
    u32 below = sp.order < v ? min(ln, v - sp.order) : 0u;  // the span's orders below `since`
    u32 kk = 0, dd = 0, ii = 0;
    if (sp.len > 0) { kk = below; ii = ln - below; }
    // deleted span: its orders [a, b) below `since` that no earlier delete covers are D items
    u32 a = sp.order, b = sp.order + (sp.len < 0 ? below : 0u);
    u32 cnt = b - a;
    if (cnt != 0u && cnt <= DIFF_LONG) {
      u32 set = 0;
      for (u32 w = a >> 5; w <= ((b - 1u) >> 5); w++) set += (u32)__popc(bm[w] & range_mask(w, a, b));
      dd = cnt - set;
    }
    u64 big = ballot(cnt > DIFF_LONG);
    while (big) {  // long ones: the wave's lanes take words
      u32 s = (u32)__builtin_ctzll(big);
      big &= big - 1ull;
      u32 ua = rdlane(a, s), ub = rdlane(b, s);
      u32 set = 0;
      for (u32 w = (ua >> 5) + l; w <= ((ub - 1u) >> 5); w += 64u) set += (u32)__popc(bm[w] & range_mask(w, ua, ub));
      set = wave_sum(set);
      if (l == s) dd = (ub - ua) - set;
    }
    bool c = (dd + ii) != 0u, bk = kk != 0u;
    // patch state after each span: content opens (or keeps open) a patch, a K-only span closes it
    u64 mO = ballot(c), mC = ballot(bk && !c);
    u32 Di = wave_incl_scan(dd), Ii = wave_incl_scan(ii);
    if (l == 63u) {
      s_d[wv] = Di;
      s_i[wv] = Ii;
      s_op[wv] = (mO | mC) ? (mO > mC ? 1u : 2u) : 0u;  // (the higher lane decides) 0: no K, D or I item in this wave
    }
    __syncthreads();
    u32 open_in = c_open, d_in = c_del, i_in = c_ins;
    for (u32 w = 0; w < wv; w++) {
      u32 op = s_op[w];
      if (op) open_in = op == 1u;
      d_in += s_d[w];
      i_in += s_i[w];
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
      u32 Dex = d_in + Di - dd, Iex = i_in + Ii - ii;  // D / I items before this span
      if (start && p < my_pat) pat[p] = Patch{vp[k] + kk, 0u, Dex, Iex};
      // the wave's inserted items: lane l takes item t + l of the wave's Tn, so stores are
      // contiguous; its span is the first lane whose inclusive count passes it (a 6-step search
      // over the scan through ds_bpermute; lanes without inserted items repeat their
      // predecessor's count and are never found)
      u32 fo = sp.order + kk;  // the span's first inserted order
      u32 st = Ii - ii;        // its first item within the wave
      u32 Tn = rdlane(Ii, 63);
      u32 wbase = Iex - st;    // I items before this wave (the same in every lane)
      for (u32 t = 0; t < Tn; t += 64u) {
        u32 j = t + l;
        u32 s = 0;
#pragma unroll
        for (u32 step = 32u; step >= 1u; step >>= 1) s += shfl(Ii, s + step - 1u) <= j ? step : 0u;
        u32 sfo = shfl(fo, s), sst = shfl(st, s);
        u32 x = wbase + j, o = sfo + (j - sst);
        if (j < Tn && x < my_ins) {
          io[x] = o;
          if (text) it[x] = src[o];
        }
      }
    }
    for (u32 w = 0; w < DIFF_WAVES; w++) {
      u32 op = s_op[w];
      if (op) c_open = op == 1u;
      c_del += s_d[w];
      c_ins += s_i[w];
      c_pat += s_st[w];
    }
    __syncthreads();  // (the next pass rewrites the LDS totals)
  }
  if (!WRITE) {
    if (tid == 0) D.res[i] = DiffRes{c_pat, c_ins, text ? DIFF_TEXT : 0u, no, 0ull, 0ull};
    return;
  }
  // del_len / ins_len of patch p: the D / I items from its start to the next patch's start (the
  // document's totals after the last one).  Each sweep reads its patches and their successors,
  // then writes; the next sweep's patches are untouched until then.
  u32 np = min(c_pat, my_pat);
  __syncthreads();
  for (u32 p0 = 0; p0 < np; p0 += DIFF_T) {
    u32 p = p0 + tid;
    u32 d0 = 0, d1 = 0, i0 = 0, i1 = 0;
    if (p < np) {
      Patch x = pat[p];
      d0 = x.ins_len; i0 = x.ins_off;
      d1 = c_del; i1 = c_ins;
      if (p + 1u < np) {
        Patch y = pat[p + 1u];
        d1 = y.ins_len; i1 = y.ins_off;
      }
    }
    __syncthreads();
    if (p < np) {
      pat[p].del_len = d1 - d0;
      pat[p].ins_len = i1 - i0;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Patches between two versions (crdt_diff_between_async): the diff's walk with both sides taken
// from a version.  An item with order x is old when it is visible at `from` and new when it is
// visible at `to` ("old-visible" above, once per version: x below the version and its bit clear in
// that version's "deleted before" bitmap, k_diff_mark run twice).  K / D / I / N and the patches
// are the diff's; pos counts the new items before the patch, which is not the published vpos.
//
// No closed form per span: a span's items change class at any order, so one span can hold several
// patches.  Only order and |len| of a span matter; its classes come from the bitmaps one 32-order
// word at a time:
//   old = below(from) & ~bm_a,  new = below(to) & ~bm_b,  K = old & new,  C = old ^ new (D or I),
//   X = old | new (not N).
// A C item starts a patch when the last X item before it is a K or there is none.  Within a word
// that is one add: (K << 1) + ~X carries every K up through the N items above it onto the next X
// item (d2_starts); across words, spans, lanes, waves and passes the state "the last X item was a
// C" is carried, with the counts of patches and of D, I and new items.
// ---------------------------------------------------------------------------------------------
struct Diff2IO {
  DiffIO d;         // since = from, bm = the "deleted before from" bitmaps; the result as the diff's
  const u32* to;    // [i]
  const u32* bm_b;  // "deleted before to", at the same bm_base
};
#define DIFF2_LONG 256u  // spans with more orders below max(from, to) are walked by the whole wave

// the orders below v among the 32 of word w
__device__ __forceinline__ u32 below_mask(u32 w, u32 v) {
  u32 base = w << 5;
  return v <= base ? 0u : (v - base >= 32u ? 0xFFFFFFFFu : (1u << (v - base)) - 1u);
}
// one word of a span [a, b): its old, new, K, C and X items
struct D2Word {
  u32 o, n, K, C, X;
};
// (SETS, csrc/diff_vv.h: either side is a set of orders given as a member bitmap, ma / mb, in
// place of "the orders below from / to")
template <bool SETS = false>
__device__ __forceinline__ D2Word d2_word(const u32* bma, const u32* bmb, u32 w, u32 a, u32 b, u32 from, u32 to,
                                          const u32* ma = nullptr, const u32* mb = nullptr) {
  u32 m = range_mask(w, a, b);
  u32 o, n;
  if (SETS) {
    o = m & ma[w] & ~bma[w];
    n = m & mb[w] & ~bmb[w];
  } else {
    o = m & below_mask(w, from) & ~bma[w];
    n = m & below_mask(w, to) & ~bmb[w];
  }
  return D2Word{o, n, o & n, o ^ n, o | n};
}
// the patch starts of a word: C items whose last X predecessor in the word is a K, and the word's
// first X item if it is a C and no patch is open before the word
__device__ __forceinline__ u32 d2_starts(const D2Word& x, bool open) {
  u32 s = x.C & x.X & ((x.K << 1) + ~x.X);
  if (!open) s |= x.X & (0u - x.X) & x.C;
  return s;
}
__device__ __forceinline__ bool d2_first_c(const D2Word& x) { return (x.X & (0u - x.X) & x.C) != 0u; }           // (X != 0)
__device__ __forceinline__ bool d2_last_c(const D2Word& x) { return ((x.C >> (31u - (u32)__clz(x.X))) & 1u) != 0u; }  // (X != 0)
// The summary of a stretch of items: any X item; its first / last X item is a C; the patch starts
// after its first X item (counted as if a patch were open before the stretch: the first item's
// start depends on what precedes and is added by whoever knows that); its D, I and new items.
struct D2Sum {
  u32 has, fc, lc, si, dd, ii, nn;
};
// the r-th (from 0) set bit of m (r < popc(m))
__device__ __forceinline__ u32 nth_bit(u32 m, u32 r) {
  u32 bit = 0;
#pragma unroll
  for (u32 sh = 16u; sh >= 1u; sh >>= 1) {
    u32 c = (u32)__popc((m >> bit) & ((1u << sh) - 1u));
    if (c <= r) {
      r -= c;
      bit += sh;
    }
  }
  return bit;
}
// the patches that start in one word: pos and, for now, the D / I items before the start in
// ins_len / ins_off (as k_diff); n0 / d0 / i0 = new, D and I items before the word
__device__ __forceinline__ void d2_emit(u32 S, const D2Word& x, u32 p, u32 n0, u32 d0, u32 i0, Patch* pat, u32 my_pat) {
  while (S) {
    u32 lowm = (1u << (u32)__builtin_ctz(S)) - 1u;
    S &= S - 1u;
    if (p < my_pat)
      pat[p] = Patch{n0 + (u32)__popc(x.n & lowm), 0u, d0 + (u32)__popc(x.o & ~x.n & lowm), i0 + (u32)__popc(x.n & ~x.o & lowm)};
    p++;
  }
}

// A long span [ua, ub) walked by the whole wave, 64 words per step in lane order.  WRITE = false:
// its summary.  WRITE = true: `open` / p / n0 / d0 / i0 are the true state and counts before the
// span; its patches are written by the lanes that hold their words, and its inserted items with
// contiguous stores: lane l takes item t + l of the step's, finds its word by the 6-step search
// over the scan (as k_diff) and its bit by a 5-step search over the word.
template <bool WRITE, bool SETS = false>
__device__ __forceinline__ D2Sum d2_long(const u32* bma, const u32* bmb, u32 ua, u32 ub, u32 from, u32 to, u32 l, bool open,
                                         u32 p, u32 n0, u32 d0, u32 i0, Patch* pat, u32 my_pat, u32* io, u32* it, u32 my_ins,
                                         bool text, const u32* src, const u32* ma = nullptr, const u32* mb = nullptr) {
  D2Sum t{0u, 0u, 0u, 0u, 0u, 0u, 0u};
  u32 wl = (ub - 1u) >> 5;
  u64 lower = (1ull << l) - 1ull;
  for (u32 w0 = ua >> 5; w0 <= wl; w0 += 64u) {
    u32 w = w0 + l;
    D2Word x{0u, 0u, 0u, 0u, 0u};
    if (w <= wl) x = d2_word<SETS>(bma, bmb, w, ua, ub, from, to, ma, mb);
    bool h = x.X != 0u;
    bool lastc = h && d2_last_c(x);
    u64 mO = ballot(lastc), mC = ballot(h && !lastc);
    u64 lo = mO & lower, lc = mC & lower;
    bool ob = (lo | lc) ? lo > lc : open;  // a patch is open before this lane's word
    u32 S = d2_starts(x, ob);
    u32 ns = (u32)__popc(S), nd = (u32)__popc(x.o & ~x.n), ni = (u32)__popc(x.n & ~x.o), nn = (u32)__popc(x.n);
    if (!WRITE) {
      if (!t.has && (mO | mC)) {
        t.has = 1u;
        t.fc = rdlane(h && d2_first_c(x) ? 1u : 0u, (u32)__builtin_ctzll(mO | mC));
      }
      t.si += wave_sum(ns);
      t.dd += wave_sum(nd);
      t.ii += wave_sum(ni);
      t.nn += wave_sum(nn);
    } else {
      u32 Pi = wave_incl_scan(ns), Di = wave_incl_scan(nd), Ii = wave_incl_scan(ni), Ni = wave_incl_scan(nn);
      d2_emit(S, x, p + Pi - ns, n0 + Ni - nn, d0 + Di - nd, i0 + Ii - ni, pat, my_pat);
      u32 im = x.n & ~x.o;
      u32 st = Ii - ni;  // the word's first inserted item within the step
      u32 Tn = rdlane(Ii, 63);
      for (u32 t0 = 0; t0 < Tn; t0 += 64u) {
        u32 j = t0 + l;
        u32 s = 0;
#pragma unroll
        for (u32 step = 32u; step >= 1u; step >>= 1) s += shfl(Ii, s + step - 1u) <= j ? step : 0u;
        u32 sm = shfl(im, s), sst = shfl(st, s);
        u32 o = ((w0 + s) << 5) + nth_bit(sm, j - sst);
        u32 xi = i0 + j;
        if (j < Tn && xi < my_ins) {
          io[xi] = o;
          if (text) it[xi] = src[o];
        }
      }
      p += rdlane(Pi, 63);
      n0 += rdlane(Ni, 63);
      d0 += rdlane(Di, 63);
      i0 += Tn;
    }
    if (mO | mC) open = mO > mC;
  }
  t.lc = (t.has && open) ? 1u : 0u;
  return t;
}

// One block per listed document, DIFF_T canonical spans per loop pass, in document order, count
// sweep / k_result_scan<DiffRes> / write sweep as k_diff.  Within a pass each thread summarises
// its span word by word (D2Sum; spans past DIFF2_LONG by the whole wave), the ballots and wave
// scans of k_diff give the state and the counts before every span, and the waves' totals meet in
// LDS; the open state and the counts of patches, D, I and new items carry from pass to pass in
// registers.  The write sweep then walks the words of every span in which a patch starts once
// more, with the true state before it, and the lane writes those patches; the wave writes its
// short spans' inserted items together and a long span's in d2_long, with contiguous stores; the
// last sweep over the document's patches turns neighbouring starts into del_len and ins_len.
// (The walk itself is d2_walk, which k_diff2 instantiates for two versions and k_diff2_sets,
// csrc/diff_vv.h, for two sets of orders: SETS reads each side's member bitmap at the index's
// bm_base and its "deleted by the set" bitmap in the pub_words(ord_cap) words after it, and takes
// the sides' k_vv_mark flags fa / fb in place of the two version checks.)
constexpr u32 VV_BAD = 1u;     // k_vv_mark: a vector out of bounds, or a poisoned document
constexpr u32 VV_CLOSED = 2u;  // k_vv_mark: the set is causally closed
template <bool WRITE, bool SETS>
__device__ __forceinline__ void d2_walk(const Pools& P, const PubOut& O, const Diff2IO& E, u32 n, const u32* fa, const u32* fb) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  const DiffIO& D = E.d;
  u32 d = D.docs[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  i32 stt = P.st[d].status;
  u32 no = P.st[d].next_order, from = SETS ? no : D.since[i], to = SETS ? no : E.to[i];
  u64 cb = D.cbase[d], cl = D.clen[d];
  bool text = cb != NO_CONTENT && cl >= (u64)no;
  bool bad = (stt != ST_OK && stt != ST_NEED_CAPACITY) || from > no || to > no;
  if (SETS) bad = bad || ((fa[i] | fb[i]) & VV_BAD) != 0u;
  if (bad) {
    if (!WRITE && tid == 0) D.res[i] = DiffRes{0u, 0u, DIFF_BAD, no, 0ull, 0ull};
    return;
  }
  const DocSeg& sg = P.seg[d];
  const Span* cn = O.canon + sg.canon_base;
  u32 ns = min(O.canon_n[d], sg.canon_cap);
  // items at or above both versions are N; every order is below ord_cap (the bitmaps' words)
  u32 top = min(max(from, to), sg.ord_cap);
  const u32* bma = D.bm + D.bm_base[i];
  const u32* bmb = E.bm_b + D.bm_base[i];
  const u32* ma = nullptr;
  const u32* mb = nullptr;
  if (SETS) {
    u32 nw = pub_words(sg.ord_cap);
    ma = bma; mb = bmb;
    bma += nw; bmb += nw;
  }
  u32 my_pat = 0, my_ins = 0;  // (WRITE) this index's counts from the first sweep: every store stays below them
  Patch* pat = nullptr;
  u32* io = nullptr;
  u32* it = nullptr;
  if (WRITE) {
    DiffRes rs = D.res[i];
    my_pat = rs.n_pat; my_ins = rs.n_ins;
    pat = D.patches + rs.poff;
    io = D.ins_order + rs.ioff;
    it = D.ins_text + rs.ioff;
  }
  const u32* src = D.content + (text ? cb : 0ull);
  __shared__ u32 s_op[DIFF_WAVES], s_d[DIFF_WAVES], s_i[DIFF_WAVES], s_n[DIFF_WAVES], s_st[DIFF_WAVES];
  u32 c_open = 0, c_pat = 0, c_del = 0, c_ins = 0, c_new = 0;  // carried: a patch is open; patches, D, I and new items so far
  for (u32 k0 = 0; k0 < ns; k0 += DIFF_T) {
    u32 k = k0 + tid;
    Span sp = k < ns ? cn[k] : Span{0, 0, 0, 0};
    u32 a = min(sp.order, top), b = (u32)min((u64)sp.order + slen(sp), (u64)top);
    u32 cnt = b > a ? b - a : 0u;
    D2Sum m{0u, 0u, 0u, 0u, 0u, 0u, 0u};
    bool shrt = cnt != 0u && cnt <= DIFF2_LONG;
    u32 fo = 0, hi = 0;  // (WRITE) the span's first and last inserted order
    if (shrt) {
      bool open = true;
      for (u32 w = a >> 5; w <= ((b - 1u) >> 5); w++) {
        D2Word x = d2_word<SETS>(bma, bmb, w, a, b, from, to, ma, mb);
        if (x.X) {
          if (!m.has) {
            m.has = 1u;
            m.fc = d2_first_c(x) ? 1u : 0u;
          }
          m.si += (u32)__popc(d2_starts(x, open));
          open = d2_last_c(x);
        }
        u32 im = x.n & ~x.o;
        if (WRITE && im) {
          if (!m.ii) fo = (w << 5) + (u32)__builtin_ctz(im);
          hi = (w << 5) + 31u - (u32)__clz(im);
        }
        m.dd += (u32)__popc(x.o & ~x.n);
        m.ii += (u32)__popc(im);
        m.nn += (u32)__popc(x.n);
      }
      m.lc = (m.has && open) ? 1u : 0u;
    }
    u64 big = ballot(cnt > DIFF2_LONG);
    for (u64 bg = big; bg;) {
      u32 s = (u32)__builtin_ctzll(bg);
      bg &= bg - 1ull;
      D2Sum t = d2_long<false, SETS>(bma, bmb, rdlane(a, s), rdlane(b, s), from, to, l, true, 0u, 0u, 0u, 0u, nullptr, 0u,
                                     nullptr, nullptr, 0u, false, nullptr, ma, mb);
      if (l == s) m = t;
    }
    // state after each span: its last X item is a C (a patch is open) or a K (none is)
    u64 mO = ballot(m.has && m.lc), mC = ballot(m.has && !m.lc);
    u32 Di = wave_incl_scan(m.dd), Ii = wave_incl_scan(m.ii), Ni = wave_incl_scan(m.nn);
    if (l == 63u) {
      s_d[wv] = Di;
      s_i[wv] = Ii;
      s_n[wv] = Ni;
      s_op[wv] = (mO | mC) ? (mO > mC ? 1u : 2u) : 0u;  // (the higher lane decides) 0: no X item in this wave
    }
    __syncthreads();
    u32 open_in = c_open, d_in = c_del, i_in = c_ins, n_in = c_new;
    for (u32 w = 0; w < wv; w++) {
      u32 op = s_op[w];
      if (op) open_in = op == 1u;
      d_in += s_d[w];
      i_in += s_i[w];
      n_in += s_n[w];
    }
    u64 lower = (1ull << l) - 1ull;
    u64 lo = mO & lower, lc = mC & lower;
    bool open_before = (lo | lc) ? lo > lc : open_in != 0u;
    u32 nst = m.si + ((m.fc && !open_before) ? 1u : 0u);  // the patches that start in this span
    u32 Pi = wave_incl_scan(nst);
    if (l == 63u) s_st[wv] = Pi;
    __syncthreads();
    if (WRITE) {
      u32 p = c_pat + Pi - nst;
      for (u32 w = 0; w < wv; w++) p += s_st[w];
      u32 Dex = d_in + Di - m.dd, Iex = i_in + Ii - m.ii, Nex = n_in + Ni - m.nn;  // D / I / new items before this span
      if (shrt && nst != 0u) {  // the patches that start in this span: its words once more, with the true state
        bool open = open_before;
        u32 pp = p, n0 = Nex, d0 = Dex, i0 = Iex;
        for (u32 w = a >> 5; w <= ((b - 1u) >> 5); w++) {
          D2Word x = d2_word<SETS>(bma, bmb, w, a, b, from, to, ma, mb);
          u32 S = d2_starts(x, open);
          d2_emit(S, x, pp, n0, d0, i0, pat, my_pat);
          pp += (u32)__popc(S);
          n0 += (u32)__popc(x.n);
          d0 += (u32)__popc(x.o & ~x.n);
          i0 += (u32)__popc(x.n & ~x.o);
          if (x.X) open = d2_last_c(x);
        }
      }
      // the short spans' inserted items: lane l takes item t + l of the wave's, so stores are
      // contiguous; its span by the 6-step search over the scan (as k_diff).  A span whose
      // inserted items are one run of orders (nearly all) gives the order in closed form; of
      // another the lane walks the words to its item
      u32 is = shrt ? m.ii : 0u;
      u32 Is = wave_incl_scan(is);
      u32 st = Is - is;
      u32 Tn = rdlane(Is, 63);
      u64 mRun = ballot(is != 0u && hi - fo + 1u == is);
      for (u32 t0 = 0; t0 < Tn; t0 += 64u) {
        u32 j = t0 + l;
        u32 s = 0;
#pragma unroll
        for (u32 step = 32u; step >= 1u; step >>= 1) s += shfl(Is, s + step - 1u) <= j ? step : 0u;
        u32 r = j - shfl(st, s);
        u32 o = shfl(fo, s) + r;
        u32 xi = shfl(Iex, s) + r;
        bool walk = j < Tn && ((mRun >> s) & 1ull) == 0ull;
        if (ballot(walk)) {
          u32 sa = shfl(a, s), sb = shfl(b, s);
          if (walk) {
            for (u32 w = sa >> 5; w <= ((sb - 1u) >> 5); w++) {
              D2Word x = d2_word<SETS>(bma, bmb, w, sa, sb, from, to, ma, mb);
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
        if (j < Tn && xi < my_ins) {
          io[xi] = o;
          if (text) it[xi] = src[o];
        }
      }
      for (u64 bg = big; bg;) {
        u32 s = (u32)__builtin_ctzll(bg);
        bg &= bg - 1ull;
        d2_long<true, SETS>(bma, bmb, rdlane(a, s), rdlane(b, s), from, to, l, rdlane(open_before ? 1u : 0u, s) != 0u,
                            rdlane(p, s), rdlane(Nex, s), rdlane(Dex, s), rdlane(Iex, s), pat, my_pat, io, it, my_ins, text, src,
                            ma, mb);
      }
    }
    for (u32 w = 0; w < DIFF_WAVES; w++) {
      u32 op = s_op[w];
      if (op) c_open = op == 1u;
      c_del += s_d[w];
      c_ins += s_i[w];
      c_new += s_n[w];
      c_pat += s_st[w];
    }
    __syncthreads();  // (the next pass rewrites the LDS totals)
  }
  if (!WRITE) {
    if (tid == 0) D.res[i] = DiffRes{c_pat, c_ins, text ? DIFF_TEXT : 0u, no, 0ull, 0ull};
    return;
  }
  // del_len / ins_len of patch p: the D / I items from its start to the next patch's start, as k_diff
  u32 np = min(c_pat, my_pat);
  __syncthreads();
  for (u32 p0 = 0; p0 < np; p0 += DIFF_T) {
    u32 p = p0 + tid;
    u32 d0 = 0, d1 = 0, i0 = 0, i1 = 0;
    if (p < np) {
      Patch x = pat[p];
      d0 = x.ins_len; i0 = x.ins_off;
      d1 = c_del; i1 = c_ins;
      if (p + 1u < np) {
        Patch y = pat[p + 1u];
        d1 = y.ins_len; i1 = y.ins_off;
      }
    }
    __syncthreads();
    if (p < np) {
      pat[p].del_len = d1 - d0;
      pat[p].ins_len = i1 - i0;
    }
  }
}
template <bool WRITE>
__global__ __launch_bounds__(DIFF_T) void k_diff2(Pools P, PubOut O, Diff2IO E, u32 n) {
  d2_walk<WRITE, false>(P, O, E, n, nullptr, nullptr);
}

template <class T>
__device__ __forceinline__ i32 find_run(const T* b, u32 n, u32 x) {  // simple_rle.rs:18-25 search
  u32 lo = 0, hi = n;
  while (lo < hi) {
    u32 mid = (lo + hi) >> 1;
    u32 k = ((const u32*)&b[mid])[0];
    u32 ln = WaveGPU<32>::rlen(b[mid]);
    if (x < k) hi = mid;
    else if (x >= k + ln) lo = mid + 1;
    else return (i32)mid;
  }
  return -1;
}

template <int L>
__global__ void k_pos_to_loc(Pools P, PubOut O, u32 n_docs, u64 nq, const u32* doc, const u32* pos, u16* agent, u32* seq) {
  for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (u64)gridDim.x * blockDim.x) {
    u32 d = doc[q], p = pos[q];
    u16 a = 0xFFFF;
    u32 sq = INVALID;
    if (d < n_docs) {
      i32 stt = P.st[d].status;
      if ((stt == ST_OK || stt == ST_NEED_CAPACITY) && p < O.len[d]) {
        DocSeg seg = P.seg[d];
        const u32* vp = O.vpos + seg.canon_base;
        const Span* cn = O.canon + seg.canon_base;
        u32 lo = 0, hi = O.canon_n[d];
        while (lo < hi) {
          u32 mid = (lo + hi) >> 1;
          if (vp[mid] <= p) lo = mid + 1; else hi = mid;
        }
        if (lo) {  // (no span: a document publish refused has len > 0 and canon_n 0 -- no answer, no vp[-1])
          u32 k = lo - 1;
          u32 order = cn[k].order + (p - vp[k]);
          const CwoRun* cw = P.cwo + seg.cwo_base;
          i32 r = find_run(cw, P.st[d].n_cwo, order);
          if (r >= 0) { a = (u16)cw[r].agent; sq = cw[r].seq + (order - cw[r].key); }
        }
      }
    }
    agent[q] = a;
    seq[q] = sq;
  }
}

// pos -> loc for a query batch whose queries come in runs per document (the usual shape: a
// document's cursors, or a batch sorted by document): block b answers queries
// [b * QBLK_Q, (b + 1) * QBLK_Q).  When they all name one document whose visible prefix vpos fits
// QBLK_MAX entries, the block stages vpos in LDS with coalesced loads (each entry read from HBM
// once per block instead of ~log2(spans) dependent gathers per query) and every query's binary
// search runs in LDS; any other chunk answers thread by thread from HBM, as k_pos_to_loc.
#define QBLK_Q 4096u
#define QBLK_T 1024u    // threads per block (16 waves: one block per CU holds the LDS)
#define QBLK_MAX 36864u  // 144 KiB of LDS
#define QBLK_CWO 512u    // client_with_order runs staged with it (8 KiB)
#define QBLK_LDS (QBLK_MAX * 4u + QBLK_CWO * 16u)
template <int L>
__global__ __launch_bounds__(QBLK_T) void k_pos_to_loc_blk(Pools P, PubOut O, u32 n_docs, u64 nq, const u32* doc, const u32* pos,
                                                        u16* agent, u32* seq) {
  extern __shared__ u32 s_vp[];
  __shared__ u32 s_mixed;
  const u32 t = threadIdx.x;
  const u64 q0 = (u64)blockIdx.x * QBLK_Q;
  const u64 q1 = q0 + QBLK_Q < nq ? q0 + QBLK_Q : nq;
  const u32 d0 = doc[q0];
  if (t == 0) s_mixed = 0;
  __syncthreads();
  u32 mixed = 0;
#pragma unroll
  for (u32 j = 0; j < QBLK_Q / QBLK_T; j++) {  // (unrolled: the loads are in flight together)
    u64 q = q0 + (u64)j * QBLK_T + t;
    mixed |= (q < q1 && doc[q] != d0) ? 1u : 0u;
  }
  if (mixed) s_mixed = 1;  // (any writer stores the same value)
  __syncthreads();
  bool staged = false;
  u32 cn = 0, dlen = 0, ncwo = 0;
  DocSeg seg{};
  if (!s_mixed && d0 < n_docs) {
    i32 stt = P.st[d0].status;
    cn = O.canon_n[d0];
    if ((stt == ST_OK || stt == ST_NEED_CAPACITY) && cn <= QBLK_MAX) {
      seg = P.seg[d0];
      dlen = cn ? O.len[d0] : 0u;  // (a document publish refused: no span, no answer)
      ncwo = P.st[d0].n_cwo;
      const u32* vp = O.vpos + seg.canon_base;
      for (u32 i0 = 0; i0 < cn; i0 += QBLK_T * 16u) {  // 16 loads per thread in flight per step
        u32 v[16];
#pragma unroll
        for (u32 u = 0; u < 16u; u++) {
          u32 i = i0 + u * QBLK_T + t;
          v[u] = i < cn ? vp[i] : 0u;
        }
#pragma unroll
        for (u32 u = 0; u < 16u; u++) {
          u32 i = i0 + u * QBLK_T + t;
          if (i < cn) s_vp[i] = v[u];
        }
      }
      staged = true;
    }
  }
  __syncthreads();
  if (!staged) {  // mixed chunk, long document or a failed one: per-thread search in HBM
    for (u64 q = q0 + t; q < q1; q += QBLK_T) {
      u32 d = doc[q], p = pos[q];
      u16 a = 0xFFFF;
      u32 sq = INVALID;
      if (d < n_docs) {
        i32 stt = P.st[d].status;
        if ((stt == ST_OK || stt == ST_NEED_CAPACITY) && p < O.len[d]) {
          DocSeg sg = P.seg[d];
          const u32* vp = O.vpos + sg.canon_base;
          u32 lo = 0, hi = O.canon_n[d];
          while (lo < hi) {
            u32 mid = (lo + hi) >> 1;
            if (vp[mid] <= p) lo = mid + 1; else hi = mid;
          }
          if (lo) {  // (as k_pos_to_loc: a document publish refused has no span to answer from)
            u32 k = lo - 1;
            u32 order = O.canon[sg.canon_base + k].order + (p - vp[k]);
            const CwoRun* cw = P.cwo + sg.cwo_base;
            i32 r = find_run(cw, P.st[d].n_cwo, order);
            if (r >= 0) { a = (u16)cw[r].agent; sq = cw[r].seq + (order - cw[r].key); }
          }
        }
      }
      agent[q] = a;
      seq[q] = sq;
    }
    return;
  }
  // 16 queries per thread in three sweeps, so that each sweep's independent loads are in flight
  // together: binary searches in LDS, then the spans' first orders (corder, 4 B per span), then
  // client_with_order runs (staged in LDS too when the table is short)
  const u32* co = O.corder + seg.canon_base;
  const CwoRun* cw = P.cwo + seg.cwo_base;
  CwoRun* s_cw = (CwoRun*)(s_vp + QBLK_MAX);
  const bool cw_lds = ncwo <= QBLK_CWO;
  if (cw_lds) {
    for (u32 i = t; i < ncwo; i += QBLK_T) s_cw[i] = cw[i];
  }
  __syncthreads();
  constexpr u32 QPT = QBLK_Q / QBLK_T;
  u32 kk[QPT], pp[QPT];
#pragma unroll
  for (u32 j = 0; j < QPT; j++) {
    u64 q = q0 + (u64)j * QBLK_T + t;
    pp[j] = q < q1 ? pos[q] : INVALID;
    kk[j] = 0u;
  }
  // the 16 searches in lockstep (the halving sequence depends only on cn), so each step's 16 LDS
  // reads are in flight together: kk = the last span whose vpos <= p
  for (u32 n = cn; n > 1u;) {
    u32 half = n >> 1;
#pragma unroll
    for (u32 j = 0; j < QPT; j++) kk[j] = s_vp[kk[j] + half] <= pp[j] ? kk[j] + half : kk[j];
    n -= half;
  }
#pragma unroll
  for (u32 j = 0; j < QPT; j++) {
    u32 p = pp[j];
    if (p < dlen) pp[j] = p - s_vp[kk[j]];  // (vpos[0] = 0 <= p: kk is a span)
    else kk[j] = INVALID;
  }
#pragma unroll
  for (u32 j = 0; j < QPT; j++) pp[j] = kk[j] != INVALID ? co[kk[j]] + pp[j] : INVALID;  // orders
#pragma unroll
  for (u32 j = 0; j < QPT; j++) {
    u64 q = q0 + (u64)j * QBLK_T + t;
    if (q >= q1) break;
    u16 a = 0xFFFF;
    u32 sq = INVALID;
    if (kk[j] != INVALID) {
      u32 order = pp[j];
      i32 r = cw_lds ? find_run(s_cw, ncwo, order) : find_run(cw, ncwo, order);
      if (r >= 0) {
        CwoRun c = cw_lds ? s_cw[r] : cw[r];
        a = (u16)c.agent;
        sq = c.seq + (order - c.key);
      }
    }
    agent[q] = a;
    seq[q] = sq;
  }
}

// loc -> pos in the same 4,096-query chunks: a one-document chunk stages the used words of its
// span-start bitmap and their prefix counts in LDS (coalesced), so order -> span rank is two LDS
// reads; the agent's item_orders run, the rank -> span entry and the span itself are gathered in
// sweeps with every thread's queries in flight together.  Other chunks: as k_loc_to_pos.
#define QBLK_W 16384u  // bitmap words staged (+ as many prefix words: 128 KiB)
template <int L>
__global__ __launch_bounds__(QBLK_T) void k_loc_to_pos_blk(Pools P, PubOut O, u32 n_docs, u64 nq, const u32* doc, const u16* agent,
                                                         const u32* seq, u32* pos, u8* deleted) {
  extern __shared__ u32 s_bw[];  // [0, used) bitmap words, [QBLK_W, QBLK_W + used) prefixes
  __shared__ u32 s_mixed;
  const u32 t = threadIdx.x;
  const u64 q0 = (u64)blockIdx.x * QBLK_Q;
  const u64 q1 = q0 + QBLK_Q < nq ? q0 + QBLK_Q : nq;
  const u32 d0 = doc[q0];
  if (t == 0) s_mixed = 0;
  __syncthreads();
  u32 mixed = 0;
#pragma unroll
  for (u32 j = 0; j < QBLK_Q / QBLK_T; j++) {
    u64 q = q0 + (u64)j * QBLK_T + t;
    mixed |= (q < q1 && doc[q] != d0) ? 1u : 0u;
  }
  if (mixed) s_mixed = 1;
  __syncthreads();
  bool staged = false;
  DocState st{};
  DocSeg seg{};
  u32 used = 0, cn = 0;
  if (!s_mixed && d0 < n_docs) {
    st = P.st[d0];
    used = st.next_order / 32u + 1u;
    if ((st.status == ST_OK || st.status == ST_NEED_CAPACITY) && used <= QBLK_W) {
      seg = P.seg[d0];
      cn = O.canon_n[d0];
      u32 nw = pub_words(seg.ord_cap);
      const u32* bits = O.pub + seg.pub_base;
      for (u32 i = t; i < used; i += QBLK_T) {
        u32 b = i < nw ? bits[i] : 0u, c = i < nw ? bits[nw + i] : 0u;
        s_bw[i] = b;
        s_bw[QBLK_W + i] = c;
      }
      staged = true;
    }
  }
  __syncthreads();
  if (!staged) {
    for (u64 q = q0 + t; q < q1; q += QBLK_T) {
      u32 d = doc[q];
      u32 ps = INVALID;
      u8 dl = 2;
      if (d < n_docs) {
        DocState s = P.st[d];
        if ((s.status == ST_OK || s.status == ST_NEED_CAPACITY) && agent[q] < s.n_agents) {
          DocSeg sg = P.seg[d];
          AgentRec A = P.agents[sg.agent_base + agent[q]];
          const ARun* ar = P.arun + sg.arun_base + A.run_base;
          i32 r = find_run(ar, A.run_cnt, seq[q]);
          if (r >= 0) {
            u32 order = ar[r].order + (seq[q] - ar[r].key);
            u32 k = span_of_order(O, sg, O.canon_n[d], order);
            if (k != INVALID) {
              Span sp = O.canon[sg.canon_base + k];
              ps = O.vpos[sg.canon_base + k] + (sp.len > 0 ? order - sp.order : 0u);
              dl = sp.len < 0 ? 1 : 0;
            }
          }
        }
      }
      pos[q] = ps;
      deleted[q] = dl;
    }
    return;
  }
  constexpr u32 QPT = QBLK_Q / QBLK_T;
  u32 od[QPT], kk[QPT];
  // sweep 1: (agent, seq) -> order (the agent's item_orders runs)
#pragma unroll
  for (u32 j = 0; j < QPT; j++) {
    u64 q = q0 + (u64)j * QBLK_T + t;
    od[j] = INVALID;
    if (q < q1) {
      u32 a = agent[q], sq = seq[q];
      if (a < st.n_agents) {
        AgentRec A = P.agents[seg.agent_base + a];
        const ARun* ar = P.arun + seg.arun_base + A.run_base;
        i32 r = find_run(ar, A.run_cnt, sq);
        if (r >= 0) od[j] = ar[r].order + (sq - ar[r].key);
      }
    }
  }
  // sweep 2: order -> span rank in LDS, rank -> span index (gathered together)
#pragma unroll
  for (u32 j = 0; j < QPT; j++) {
    u32 o = od[j], wd = o >> 5;
    u32 r = wd < used ? s_bw[QBLK_W + wd] + (u32)__popc(s_bw[wd] & (0xFFFFFFFFu >> (31u - (o & 31u)))) : 0u;
    kk[j] = (o != INVALID && r != 0u && r <= cn) ? O.sorted[seg.canon_base + r - 1u] : INVALID;
  }
  // sweep 3: the span and its visible prefix
#pragma unroll
  for (u32 j = 0; j < QPT; j++) {
    u64 q = q0 + (u64)j * QBLK_T + t;
    if (q >= q1) break;
    u32 ps = INVALID;
    u8 dl = 2;
    u32 k = kk[j];
    if (k < cn) {
      Span sp = O.canon[seg.canon_base + k];
      u32 o = od[j];
      if (o - sp.order < slen(sp)) {
        ps = O.vpos[seg.canon_base + k] + (sp.len > 0 ? o - sp.order : 0u);
        dl = sp.len < 0 ? 1 : 0;
      }
    }
    pos[q] = ps;
    deleted[q] = dl;
  }
}

template <int L>
__global__ void k_loc_to_pos(Pools P, PubOut O, u32 n_docs, u64 nq, const u32* doc, const u16* agent, const u32* seq, u32* pos, u8* deleted) {
  for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (u64)gridDim.x * blockDim.x) {
    u32 d = doc[q];
    u32 ps = INVALID;
    u8 dl = 2;
    if (d < n_docs) {
      DocState s = P.st[d];
      if ((s.status == ST_OK || s.status == ST_NEED_CAPACITY) && agent[q] < s.n_agents) {
        DocSeg seg = P.seg[d];
        AgentRec A = P.agents[seg.agent_base + agent[q]];
        const ARun* ar = P.arun + seg.arun_base + A.run_base;
        i32 r = find_run(ar, A.run_cnt, seq[q]);
        if (r >= 0) {
          u32 order = ar[r].order + (seq[q] - ar[r].key);
          u32 k = span_of_order(O, seg, O.canon_n[d], order);
          if (k != INVALID) {
            Span sp = O.canon[seg.canon_base + k];
            ps = O.vpos[seg.canon_base + k] + (sp.len > 0 ? order - sp.order : 0u);
            dl = sp.len < 0 ? 1 : 0;
          }
        }
      }
    }
    pos[q] = ps;
    deleted[q] = dl;
  }
}

// ---------------------------------------------------------------------------------------------
// Checkout (crdt_checkout_async): the document at a past version v -- the old-visible items of
// the diff's definition above, in document order -- as arrays (order and code point of every
// item) plus a per-span prefix `opos` that answers the two README mappings on that view.  From
// the published index and the delete log only; no reference counterpart (the reference keeps no
// history of its rope).
//
// k_diff_mark (as it is, on the checkout's own buffers) gives the "deleted before v" bitmap;
// k_co_rank adds a rank directory, rk[w] = set bits in words [0, w), so the set bits of any
// order range below v are two lookups.  The old-visible items of canonical span [a, a + n) are
// then its orders below v minus the set bits among them: closed form for a visible span (never
// in the delete log: no bit set) and for a deleted span of any length alike.
// ---------------------------------------------------------------------------------------------
constexpr u32 CO_BAD = 1u;    // version > the document's version, or a poisoned document: no result
constexpr u32 CO_TEXT = 2u;   // text and digest were written (the document has content for all its orders)
struct CoRes {
  u32 len, flags, version, at;  // old-visible items; CO_*; the document's version; v
  u64 off;                      // first item of this index in ord / text (k_result_scan)
  u64 digest;                   // text digest (text_hash per item, as k_materialize; 0 without content)
};
struct CoIO {
  const u32* docs;     // [i] the listed documents
  const u32* version;  // [i] v
  const u64* bm_base;  // [i] first word of the index's bitmap in bm / rk
  const u32* bm;       // k_diff_mark's bitmap: bit x set = a delete op with order < v covers item x
  u32* rk;             // [bm_base[i] + w] set bits in words [0, w) of the index's bitmap, w <= v >> 5
  const u64* sp_base;  // [i] first entry of the index in opos (canon_cap entries each)
  u32* opos;           // [sp_base[i] + k] old-visible items before canonical span k (vpos of the view)
  CoRes* res;          // [i]
  u32* ord;            // [res[i].off + p] order of item p of the view
  u32* text;           // [res[i].off + p] its code point
  const u32* content;  // TextIO's content streams
  const u64* cbase;
  const u64* clen;
};
#define CO_WAVES 4u

// set bits below order x (x <= v: word x >> 5 has a directory entry)
__device__ __forceinline__ u32 co_set_below(const u32* bm, const u32* rk, u32 x) {
  u32 w = x >> 5;
  return rk[w] + (u32)__popc(bm[w] & ((1u << (x & 31u)) - 1u));
}
// old-visible items of a canonical span at version v
__device__ __forceinline__ u32 co_span_count(const Span& sp, u32 v, const u32* bm, const u32* rk) {
  u32 below = sp.order < v ? min(slen(sp), v - sp.order) : 0u;
  if (sp.len > 0 || below == 0u) return below;
  return below - (co_set_below(bm, rk, sp.order + below) - co_set_below(bm, rk, sp.order));
}
// index of the n-th (from 0) set bit of m; m has more than n set bits
__device__ __forceinline__ u32 select32(u32 m, u32 n) {
  u32 pos = 0;
#pragma unroll
  for (u32 s = 16u; s >= 1u; s >>= 1) {
    u32 c = (u32)__popc((m >> pos) & ((1u << s) - 1u));
    if (n >= c) { n -= c; pos += s; }
  }
  return pos;
}
// the listed document has a view at v: it is alive, v is no later than its version, and its
// orders fit the published bitmap (publish sizes ord_cap above next_order)
__device__ __forceinline__ bool co_ok(const Pools& P, u32 d, u32 v, u32& no) {
  i32 stt = P.st[d].status;
  no = P.st[d].next_order;
  return (stt == ST_OK || stt == ST_NEED_CAPACITY) && v <= no && no < P.seg[d].ord_cap;
}

// The rank directory of words [0, v >> 5] of every listed bitmap, one block per index: a
// streaming block scan, 8 consecutive words per thread and pass (the waves' totals meet in LDS,
// the carry stays in registers).  The bitmap is read once, straight after k_diff_mark wrote it.
__global__ __launch_bounds__(DIFF_T) void k_co_rank(Pools P, CoIO C, u32 n) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  u32 d = C.docs[i], v = C.version[i], no;
  if (!co_ok(P, d, v, no)) return;
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  const u32 nwv = (v >> 5) + 1u;  // <= pub_words(ord_cap), the bitmap's size
  const u32* bm = C.bm + C.bm_base[i];
  u32* rk = C.rk + C.bm_base[i];
  __shared__ u32 s_w[DIFF_WAVES];
  u32 carry = 0;
  for (u32 w0 = 0; w0 < nwv; w0 += DIFF_T * 8u) {
    u32 wb = w0 + tid * 8u;
    u32 x[8], c = 0;
#pragma unroll
    for (u32 u = 0; u < 8u; u++) {
      x[u] = wb + u < nwv ? bm[wb + u] : 0u;
      c += (u32)__popc(x[u]);
    }
    u32 incl = wave_incl_scan(c);
    if (l == 63u) s_w[wv] = incl;
    __syncthreads();
    u32 run = carry + incl - c;
    for (u32 w = 0; w < wv; w++) run += s_w[w];
#pragma unroll
    for (u32 u = 0; u < 8u; u++) {
      if (wb + u < nwv) rk[wb + u] = run;
      run += (u32)__popc(x[u]);
    }
    for (u32 w = 0; w < DIFF_WAVES; w++) carry += s_w[w];
    __syncthreads();  // (the next pass rewrites the LDS totals)
  }
}

// opos and the view's length, one block per index, DIFF_T canonical spans per pass like k_diff.
__global__ __launch_bounds__(DIFF_T) void k_co_count(Pools P, PubOut O, CoIO C, u32 n) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  u32 d = C.docs[i], v = C.version[i], no;
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  if (!co_ok(P, d, v, no)) {
    if (tid == 0) C.res[i] = CoRes{0u, CO_BAD, no, v, 0ull, 0ull};
    return;
  }
  u64 cb = C.cbase[d], cl = C.clen[d];
  bool text = cb != NO_CONTENT && cl >= (u64)no;
  const DocSeg& sg = P.seg[d];
  const Span* cn = O.canon + sg.canon_base;
  u32 ns = min(O.canon_n[d], sg.canon_cap);
  const u32* bm = C.bm + C.bm_base[i];
  const u32* rk = C.rk + C.bm_base[i];
  u32* opos = C.opos + C.sp_base[i];
  __shared__ u32 s_c[DIFF_WAVES];
  u32 carry = 0;
  for (u32 k0 = 0; k0 < ns; k0 += DIFF_T) {
    u32 k = k0 + tid;
    u32 c = k < ns ? co_span_count(cn[k], v, bm, rk) : 0u;
    u32 incl = wave_incl_scan(c);
    if (l == 63u) s_c[wv] = incl;
    __syncthreads();
    u32 ex = carry + incl - c;
    for (u32 w = 0; w < wv; w++) ex += s_c[w];
    if (k < ns) opos[k] = ex;
    for (u32 w = 0; w < DIFF_WAVES; w++) carry += s_c[w];
    __syncthreads();
  }
  if (tid == 0) C.res[i] = CoRes{carry, text ? CO_TEXT : 0u, no, v, 0ull, 0ull};
}

// k_result_scan's view of a CoRes: the view's length (0 for an index without a result)
__device__ __forceinline__ void scan_counts(const CoRes& r, u64* c) { c[0] = r.len; }
__device__ __forceinline__ void scan_store(CoRes& r, const u64* off) { r.off = off[0]; }

// The views' items.  One block of CO_WAVES waves per index; wave w takes chunks w, w + CO_WAVES,
// ... of 64 canonical spans (a chunk's items start at opos[k0], so chunks are independent, and
// opos[k + 1] - opos[k0] is the chunk's inclusive scan: no recount).  Lane l takes item t + l of
// the chunk: its span by a 6-step search over the scan, as k_diff's inserted items; inside a
// span with no marked item below v -- every visible span, and a span deleted only after v -- the
// order is the span's first plus the item's offset; inside a deleted span that v cuts (some
// items marked), the j-th clear bit through the rank directory (binary search over the span's
// words) and a select within the word.  Stores of ord / text are contiguous either way.
__global__ __launch_bounds__(64 * CO_WAVES) void k_co_write(Pools P, PubOut O, CoIO C, u32 n) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  const CoRes rs = C.res[i];
  if (rs.flags & CO_BAD) return;
  u32 d = C.docs[i], v = rs.at, len = rs.len;
  u32 l = lane_id(), wv = uni(threadIdx.x >> 6);
  bool text = (rs.flags & CO_TEXT) != 0u;
  const DocSeg& sg = P.seg[d];
  const Span* cn = O.canon + sg.canon_base;
  u32 ns = min(O.canon_n[d], sg.canon_cap);
  const u32* bm = C.bm + C.bm_base[i];
  const u32* rk = C.rk + C.bm_base[i];
  const u32* opos = C.opos + C.sp_base[i];
  const u32* src = C.content + (text ? C.cbase[d] : 0ull);
  u32* ord = C.ord + rs.off;
  u32* txt = C.text + rs.off;
  __shared__ u64 s_h[CO_WAVES];
  u64 h = 0;
  for (u32 k0 = wv * 64u; k0 < ns; k0 += 64u * CO_WAVES) {
    u32 k = k0 + l;
    Span sp = k < ns ? cn[k] : Span{0, 0, 0, 0};
    u32 st = k < ns ? opos[k] : len;            // items before span k
    u32 nx = k + 1u < ns ? opos[k + 1u] : len;  // ... and before the next one
    u32 base = rdlane(st, 0);
    u32 cnt = nx - st, Pi = nx - base, Tn = rdlane(Pi, 63);
    st -= base;
    u32 below = sp.order < v ? min(slen(sp), v - sp.order) : 0u;
    bool cut = cnt != below && cnt != 0u;  // a deleted span with marked and unmarked items below v
    u32 c0 = cut ? sp.order - co_set_below(bm, rk, sp.order) : 0u;  // clear bits before the span
    u32 wl = sp.order >> 5, wh = cut ? (sp.order + below - 1u) >> 5 : 0u;
    for (u32 t = 0; t < Tn; t += 64u) {
      u32 j = t + l;
      u32 s = 0;
#pragma unroll
      for (u32 step = 32u; step >= 1u; step >>= 1) s += shfl(Pi, s + step - 1u) <= j ? step : 0u;
      u32 r = j - shfl(st, s);
      u32 o = shfl(sp.order, s) + r;
      u32 scut = shfl((u32)cut, s), sc0 = shfl(c0, s), lo = shfl(wl, s), hi = shfl(wh, s);
      if (j < Tn && scut) {
        u32 target = sc0 + r;  // clear bits before the wanted item
        while (lo < hi) {      // the last word with at most `target` clear bits before it
          u32 mid = (lo + hi + 1u) >> 1;
          if (32u * mid - rk[mid] <= target) lo = mid;
          else hi = mid - 1u;
        }
        o = min(32u * lo + select32(~bm[lo], target - (32u * lo - rk[lo])), v - 1u);  // (v > 0 here; in range by construction)
      }
      u32 x = base + j;
      if (j < Tn && x < len) {
        ord[x] = o;
        if (text) {
          u32 cp = src[o];
          txt[x] = cp;
          h += text_hash(x, cp);
        }
      }
    }
  }
  h = wave_sum64(h);
  if (l == 0) s_h[wv] = h;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 hs = 0;
    for (u32 w = 0; w < CO_WAVES; w++) hs += s_h[w];
    C.res[i].digest = text ? mix64(hs ^ ((u64)len << 32 | 0x54ull)) : 0ull;
  }
}

// pos -> loc on the view (thread per query): the item's order from the view's order array, then
// client_with_order as k_pos_to_loc.
__global__ void k_pos_to_loc_at(Pools P, CoIO C, u32 n_idx, u64 nq, const u32* idx, const u32* pos, u16* agent, u32* seq) {
  for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (u64)gridDim.x * blockDim.x) {
    u32 i = idx[q], p = pos[q];
    u16 a = 0xFFFF;
    u32 sq = INVALID;
    if (i < n_idx) {
      CoRes rs = C.res[i];
      if (!(rs.flags & CO_BAD) && p < rs.len) {
        u32 d = C.docs[i];
        u32 order = C.ord[rs.off + p];
        DocSeg seg = P.seg[d];
        const CwoRun* cw = P.cwo + seg.cwo_base;
        i32 r = find_run(cw, P.st[d].n_cwo, order);
        if (r >= 0) { a = (u16)cw[r].agent; sq = cw[r].seq + (order - cw[r].key); }
      }
    }
    agent[q] = a;
    seq[q] = sq;
  }
}

// loc -> pos on the view (thread per query): (agent, seq) -> order as k_loc_to_pos; an order at
// or above v does not exist at v (2, like an unknown id); else the span through the published
// order -> span index, opos and the old-visible items of the span before the order.
__global__ void k_loc_to_pos_at(Pools P, PubOut O, CoIO C, u32 n_idx, u64 nq, const u32* idx, const u16* agent, const u32* seq,
                                u32* pos, u8* deleted) {
  for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (u64)gridDim.x * blockDim.x) {
    u32 i = idx[q];
    u32 ps = INVALID;
    u8 dl = 2;
    if (i < n_idx) {
      CoRes rs = C.res[i];
      u32 d = C.docs[i];
      if (!(rs.flags & CO_BAD) && agent[q] < P.st[d].n_agents) {
        DocSeg seg = P.seg[d];
        AgentRec A = P.agents[seg.agent_base + agent[q]];
        const ARun* ar = P.arun + seg.arun_base + A.run_base;
        i32 r = find_run(ar, A.run_cnt, seq[q]);
        if (r >= 0) {
          u32 order = ar[r].order + (seq[q] - ar[r].key);
          u32 k = order < rs.at ? span_of_order(O, seg, min(O.canon_n[d], seg.canon_cap), order) : INVALID;
          if (k != INVALID) {
            Span sp = O.canon[seg.canon_base + k];
            ps = C.opos[C.sp_base[i] + k] + (order - sp.order);
            dl = 0;
            if (sp.len < 0) {
              const u32* bm = C.bm + C.bm_base[i];
              const u32* rk = C.rk + C.bm_base[i];
              ps -= co_set_below(bm, rk, order) - co_set_below(bm, rk, sp.order);
              dl = (u8)((bm[order >> 5] >> (order & 31u)) & 1u);
            }
          }
        }
      }
    }
    pos[q] = ps;
    deleted[q] = dl;
  }
}

// ---------------------------------------------------------------------------------------------
// Authorship runs (crdt_blame_async): who wrote each part of a document's current text, from the
// published index and client_with_order.  No reference counterpart (print_stats is the nearest).
// Walk the visible items in document order (the canonical spans with len > 0, item by item); item
// p has an order and through client_with_order an id (agent, seq), what k_pos_to_loc answers for
// p.  A run is a maximal stretch of positions whose neighbours chain: same agent (BLAME_AGENT),
// or same agent and seq + 1 (BLAME_ID).  A run is {pos, len, agent, seq} of its first item.
//
// Per visible canonical span [o, o + len) the orders are dense, so the client_with_order runs
// that overlap it are consecutive table entries from find_run(o): every boundary between two of
// them inside the span starts a run unless the two chain (compared, the table need not be
// maximally coalesced), and the span's first item starts one unless it chains with the tail --
// (agent, next seq) -- of the last visible span before it, tombstones in between or not.
// ---------------------------------------------------------------------------------------------
struct BlameRun { u32 pos, len, agent, seq; };  // crdt_blame_run (include/crdt_gpu.h)
constexpr u32 BLAME_AGENT = 0u, BLAME_ID = 1u;  // CRDT_BLAME_*
constexpr u32 BLAME_BAD = 1u;                   // a poisoned document: no result for this index
struct BlameRes {
  u32 n_runs, flags;
  u64 off;  // first run of this index in the result array (k_result_scan)
};
struct BlameIO {
  const u32* docs;  // [i] the listed documents
  BlameRes* res;    // [i]
  BlameRun* runs;   // [res[i].off + p]
};

// The client_with_order runs under one visible canonical span of ln items whose first order lies
// in run r0: the id of its first item (ha, hs), the tail after its last one (ta, ts) and the
// number of run starts inside it.  STORE writes those starts to out[p], out[p + 1], ... (below
// lim only).  A serial walk: one table entry per step, however many the span covers.
template <bool STORE>
__device__ __forceinline__ u32 blame_walk(const CwoRun* cw, u32 ncwo, u32 r0, u32 order, u32 ln, u32 mode, u32& ha, u32& hs,
                                          u32& ta, u32& ts, BlameRun* out, u32 p, u32 lim, u32 pos) {
  CwoRun q = cw[r0];
  u32 off = order - q.key;
  ha = q.agent;
  hs = q.seq + off;
  u32 done = min(q.len - off, ln);
  ta = ha;
  ts = hs + done;
  u32 starts = 0;
  for (u32 r = r0 + 1u; done < ln && r < ncwo; r++) {
    q = cw[r];
    bool chain = (q.agent == ta) & ((mode == BLAME_AGENT) | (q.seq == ts));
    if (!chain) {
      if (STORE && p + starts < lim) out[p + starts] = BlameRun{pos + done, 0u, q.agent, q.seq};
      starts++;
    }
    u32 take = min(q.len, ln - done);
    ta = q.agent;
    ts = q.seq + take;
    done += take;
  }
  return starts;
}

// One block per listed document, DIFF_T canonical spans per loop pass, in document order, like
// k_diff.  WRITE = false counts the document's runs (res[i]); WRITE = true, after k_result_scan,
// writes them.  Each thread walks its span (blame_walk).  The tail of the last visible span
// before it comes from the same wave (the highest visible lane below this one: a ballot and a
// shuffle), from an earlier wave of the pass (LDS) or from an earlier pass (carried in registers:
// every thread folds the same LDS values, as k_diff's c_open).  A wave scan of the spans' start
// counts gives each span the index of its first run.  The start of run p writes {pos, 0, agent,
// seq}; a last sweep over the document's runs turns neighbouring pos values into len.
template <bool WRITE>
__global__ __launch_bounds__(DIFF_T) void k_blame(Pools P, PubOut O, BlameIO B, u32 n, u32 mode) {
  u32 i = blockIdx.x;
  if (i >= n) return;
  u32 d = B.docs[i];
  u32 tid = threadIdx.x, l = lane_id(), wv = uni(tid >> 6);
  i32 stt = P.st[d].status;
  if (stt != ST_OK && stt != ST_NEED_CAPACITY) {
    if (!WRITE && tid == 0) B.res[i] = BlameRes{0u, BLAME_BAD, 0ull};
    return;
  }
  const DocSeg& sg = P.seg[d];
  const Span* cn = O.canon + sg.canon_base;
  const u32* vp = O.vpos + sg.canon_base;
  u32 ns = min(O.canon_n[d], sg.canon_cap);
  const CwoRun* cw = P.cwo + sg.cwo_base;
  u32 ncwo = min(P.st[d].n_cwo, sg.cwo_cap);
  u32 my_runs = 0;  // (WRITE) this index's count from the first sweep: every store stays below it
  BlameRun* runs = nullptr;
  if (WRITE) {
    BlameRes rs = B.res[i];
    my_runs = rs.n_runs;
    runs = B.runs + rs.off;
  }
  __shared__ u32 s_has[DIFF_WAVES], s_ta[DIFF_WAVES], s_ts[DIFF_WAVES], s_c[DIFF_WAVES];
  u32 c_has = 0, c_ta = 0, c_ts = 0, c_runs = 0;  // carried: a visible item was seen, its tail; runs so far
  for (u32 k0 = 0; k0 < ns; k0 += DIFF_T) {
    u32 k = k0 + tid;
    Span sp = k < ns ? cn[k] : Span{0, 0, 0, 0};
    bool vis = sp.len > 0;
    u32 ln = vis ? (u32)sp.len : 0u;
    u32 pos = vis ? vp[k] : 0u;
    i32 r0 = vis ? find_run(cw, ncwo, sp.order) : -1;
    // (an order outside the table -- never in a healthy document -- is one piece with the id
    // k_pos_to_loc answers for it)
    u32 ha = 0xFFFFu, hs = INVALID, ta = 0xFFFFu, ts = INVALID, inner = 0;
    if (r0 >= 0) inner = blame_walk<false>(cw, ncwo, (u32)r0, sp.order, ln, mode, ha, hs, ta, ts, nullptr, 0u, 0u, pos);
    u64 mV = ballot(vis);
    u32 top = mV ? 63u - (u32)__builtin_clzll(mV) : 0u;
    if (l == top) {  // the wave's last visible span (lane 0 of a wave without one)
      s_has[wv] = mV != 0ull;
      s_ta[wv] = ta;
      s_ts[wv] = ts;
    }
    __syncthreads();
    u32 p_has = c_has, p_ta = c_ta, p_ts = c_ts;
    for (u32 w = 0; w < wv; w++)
      if (s_has[w]) { p_has = 1u; p_ta = s_ta[w]; p_ts = s_ts[w]; }
    u64 below = mV & ((1ull << l) - 1ull);
    u32 src = below ? 63u - (u32)__builtin_clzll(below) : l;
    u32 qa = shfl(ta, src), qs = shfl(ts, src);
    if (below) { p_has = 1u; p_ta = qa; p_ts = qs; }
    bool chained = (p_has != 0u) & (p_ta == ha) & ((mode == BLAME_AGENT) | (p_ts == hs));
    bool hstart = vis && !chained;  // (the document's first visible item always starts a run)
    u32 cnt = (u32)hstart + inner;
    u32 Ci = wave_incl_scan(cnt);
    if (l == 63u) s_c[wv] = Ci;
    __syncthreads();
    if (WRITE) {
      u32 p = c_runs + Ci - cnt;
      for (u32 w = 0; w < wv; w++) p += s_c[w];
      if (hstart && p < my_runs) runs[p] = BlameRun{pos, 0u, ha, hs};
      if (inner) blame_walk<true>(cw, ncwo, (u32)r0, sp.order, ln, mode, ha, hs, ta, ts, runs, p + (u32)hstart, my_runs, pos);
    }
    for (u32 w = 0; w < DIFF_WAVES; w++) {
      if (s_has[w]) { c_has = 1u; c_ta = s_ta[w]; c_ts = s_ts[w]; }
      c_runs += s_c[w];
    }
    __syncthreads();  // (the next pass rewrites the LDS values)
  }
  if (!WRITE) {
    if (tid == 0) B.res[i] = BlameRes{c_runs, 0u, 0ull};
    return;
  }
  // len of run p: from its pos to the next run's (the document's length after the last one)
  u32 nr = min(c_runs, my_runs);
  u32 dlen = ns ? vp[ns - 1u] + clen(cn[ns - 1u]) : 0u;
  __syncthreads();
  for (u32 p = tid; p < nr; p += DIFF_T) {
    u32 nx = p + 1u < nr ? runs[p + 1u].pos : dlen;
    runs[p].len = nx - runs[p].pos;
  }
}

// k_result_scan's view of a BlameRes: its runs (0 for an index without a result)
__device__ __forceinline__ void scan_counts(const BlameRes& r, u64* c) { c[0] = r.n_runs; }
__device__ __forceinline__ void scan_store(BlameRes& r, const u64* off) { r.off = off[0]; }

// pos -> loc for sorted query batches by merge path (BASELINE north_star's sorted batches): a
// chunk of QBLK_Q queries that name one document, positions ascending, is merged against the
// document's visible prefix vpos[0..cn) (ascending, vpos[0] = 0) tile by tile.  vpos streams
// through LDS in QM_TILE-entry tiles (coalesced, the next tile's loads in flight while the current
// one is searched); the queries of a tile are the contiguous run of the sorted chunk below the
// next tile's first entry, and each searches only its tile (Cursor at content pos, root.rs:54-88).
// vpos is read once per chunk and the LDS footprint is small (24 KiB), so several chunks run per
// CU -- unlike k_pos_to_loc_blk, which stages the whole prefix (up to 144 KiB) first.  Pass 1
// writes each query's order into seq[], pass 2 maps orders to (agent, seq) through
// client_with_order.  A mixed or unsorted chunk is answered per thread.
#define QM_T 256u
#define QM_TILE 2048u
template <int L>
__global__ __launch_bounds__(QM_T) void k_pos_to_loc_merge(Pools P, PubOut O, u32 n_docs, u64 nq, const u32* doc, const u32* pos,
                                                          u16* agent, u32* seq) {
  __shared__ u32 s_q[QBLK_Q];
  __shared__ u32 s_a[QM_TILE];
  __shared__ u32 s_bad;
  const u32 t = threadIdx.x;
  const u64 q0 = (u64)blockIdx.x * QBLK_Q;
  const u64 q1 = q0 + QBLK_Q < nq ? q0 + QBLK_Q : nq;
  const u32 nb = (u32)(q1 - q0);
  const u32 d0 = doc[q0];
  if (t == 0) s_bad = 0;
  for (u32 j = t; j < nb; j += QM_T) s_q[j] = pos[q0 + j];
  __syncthreads();
  u32 bad = 0;
  for (u32 j = t; j < nb; j += QM_T) {  // one document, positions ascending
    bad |= doc[q0 + j] != d0 ? 1u : 0u;
    if (j) bad |= s_q[j - 1] > s_q[j] ? 1u : 0u;
  }
  if (bad) s_bad = 1;  // (any writer stores the same value)
  __syncthreads();
  i32 stt = d0 < n_docs ? P.st[d0].status : ST_BAD_INPUT;
  if (s_bad || d0 >= n_docs || !(stt == ST_OK || stt == ST_NEED_CAPACITY)) {
    for (u64 q = q0 + t; q < q1; q += QM_T) {
      u32 d = doc[q], p = pos[q];
      u16 a = 0xFFFF;
      u32 sq = INVALID;
      if (d < n_docs) {
        i32 s2 = P.st[d].status;
        if ((s2 == ST_OK || s2 == ST_NEED_CAPACITY) && p < O.len[d]) {
          DocSeg sg = P.seg[d];
          const u32* vp = O.vpos + sg.canon_base;
          u32 lo = 0, hi = O.canon_n[d];
          while (lo < hi) {
            u32 mid = (lo + hi) >> 1;
            if (vp[mid] <= p) lo = mid + 1; else hi = mid;
          }
          if (lo) {  // (as k_pos_to_loc: a document publish refused has no span to answer from)
            u32 k = lo - 1;
            u32 order = O.corder[sg.canon_base + k] + (p - vp[k]);
            const CwoRun* cw = P.cwo + sg.cwo_base;
            i32 r = find_run(cw, P.st[d].n_cwo, order);
            if (r >= 0) { a = (u16)cw[r].agent; sq = cw[r].seq + (order - cw[r].key); }
          }
        }
      }
      agent[q] = a;
      seq[q] = sq;
    }
    return;
  }
  const DocSeg sg = P.seg[d0];
  const u32 cn = O.canon_n[d0], dlen = O.len[d0];
  const u32* A = O.vpos + sg.canon_base;
  const u32* co = O.corder + sg.canon_base;
  constexpr u32 PT = QM_TILE / QM_T;  // tile entries per thread
  u32 nx[PT];
#pragma unroll
  for (u32 u = 0; u < PT; u++) nx[u] = u * QM_T + t < cn ? A[u * QM_T + t] : 0u;
  u32 qa = 0;  // queries [0, qa) answered
  for (u32 ts = 0; ts < cn && qa < nb; ts += QM_TILE) {
    const u32 tn = cn - ts < QM_TILE ? cn - ts : QM_TILE;
#pragma unroll
    for (u32 u = 0; u < PT; u++) s_a[u * QM_T + t] = nx[u];
    const u32 te = ts + QM_TILE;
    const u32 bound = te < cn ? A[te] : INVALID;  // the next tile's first entry (queries below it are here)
#pragma unroll
    for (u32 u = 0; u < PT; u++) nx[u] = te + u * QM_T + t < cn ? A[te + u * QM_T + t] : 0u;  // next tile, in flight
    __syncthreads();
    // this tile's queries: [qa, qb), qb = the first query >= bound (every thread alike)
    u32 lo = qa, hi = nb;
    while (lo < hi) {
      u32 mid = (lo + hi) >> 1;
      if (s_q[mid] < bound) lo = mid + 1; else hi = mid;
    }
    const u32 qb = bound == INVALID ? nb : lo;
    for (u32 j = qa + t; j < qb; j += QM_T) {
      u32 p = s_q[j];
      u32 l2 = 0, h2 = tn;  // the last tile entry <= p (s_a[0] <= p: earlier queries are answered)
      while (l2 < h2) {
        u32 mid = (l2 + h2) >> 1;
        if (s_a[mid] <= p) l2 = mid + 1; else h2 = mid;
      }
      u32 k = l2 - 1u;
      seq[q0 + j] = p < dlen ? co[ts + k] + (p - s_a[k]) : INVALID;
    }
    qa = qb;
    __syncthreads();
  }
  // pass 2: order -> (agent, seq), client_with_order.get (simple_rle.rs:98-103)
  const CwoRun* cw = P.cwo + sg.cwo_base;
  const u32 ncwo = P.st[d0].n_cwo;
  for (u64 q = q0 + t; q < q1; q += QM_T) {
    u32 order = (u32)(q - q0) < qa ? seq[q] : INVALID;  // (an empty document answers nothing)
    u16 a = 0xFFFF;
    u32 sq = INVALID;
    if (order != INVALID) {
      i32 r = find_run(cw, ncwo, order);
      if (r >= 0) { a = (u16)cw[r].agent; sq = cw[r].seq + (order - cw[r].key); }
    }
    agent[q] = a;
    seq[q] = sq;
  }
}

// ---------------------------------------------------------------------------------------------
// Agent-name interning on the device (ListCRDT::get_or_create_agent_id, doc.rs:66-89; SURVEY
// §8f row 3).  One wave per group (a document's name references in call order): ids in order of
// first appearance ("ROOT" -> ROOT_AGENT, never stored), and every distinct name's rank in
// byte-lexicographic order (Rust `str` Ord, the integrate tie-break's order, doc.rs:207).
// Group g owns refs [roff[g], roff[g+1]); ref r names bytes [noff[r], noff[r+1]).  A wave hashes
// 64 refs at once (FNV-1a), looks them up in an LDS open-addressing table, and admits the new
// names of the chunk one distinct name per step in lane order (the first appearance leads).
// ---------------------------------------------------------------------------------------------
constexpr u32 INTERN_MAX = 1024, INTERN_HT = 2 * INTERN_MAX;
struct InternIO {
  const u64* roff;
  const u32* noff;
  const unsigned char* bytes;
  u16* id;      // per ref
  u32* rank;    // per ref (INVALID for ROOT)
  u32* n_out;   // per group: distinct names
  i32* status;  // per group: 0, or -1 when a group has more than INTERN_MAX distinct names
};
__device__ __forceinline__ bool intern_eq(const unsigned char* b, u32 a0, u32 a1, u32 c0, u32 c1) {
  if (a1 - a0 != c1 - c0) return false;
  for (u32 i = 0; i < a1 - a0; i++)
    if (b[a0 + i] != b[c0 + i]) return false;
  return true;
}
__device__ __forceinline__ bool intern_less(const unsigned char* b, u32 a0, u32 a1, u32 c0, u32 c1) {
  u32 la = a1 - a0, lc = c1 - c0, m = la < lc ? la : lc;
  for (u32 i = 0; i < m; i++) {
    unsigned char x = b[a0 + i], y = b[c0 + i];
    if (x != y) return x < y;
  }
  return la < lc;
}
// One group's names -> ids by first appearance (one wave: the admission is sequential in ref
// order, which is what makes the ids the reference's).  ht / hh: open-addressing table of
// ht_slots (a power of two) slots, 0 = empty else id + 1, with the slot name's FNV-1a hash; rep:
// a ref naming each id.  Returns the distinct names (k); st = -1 past max_names.
__device__ __forceinline__ u32 intern_admit(const InternIO& io, u32 g, u32* ht, u32* hh, u32* rep, u32 ht_slots,
                                            u32 max_names, i32& st) {
  u32 l = threadIdx.x & 63u;
  const unsigned char* B = io.bytes;
  u64 r0 = io.roff[g], r1 = io.roff[g + 1];
  u32 k = 0;
  st = 0;
  for (u64 c = r0; c < r1 && st == 0; c += 64) {
    u64 r = c + l;
    bool v = r < r1;
    u32 a = v ? io.noff[r] : 0u, b = v ? io.noff[r + 1] : 0u;
    u32 h = 2166136261u;
    for (u32 i = a; i < b; i++) h = (h ^ B[i]) * 16777619u;
    bool root = v && b - a == 4u && B[a] == 'R' && B[a + 1] == 'O' && B[a + 2] == 'O' && B[a + 3] == 'T';
    u32 id = INVALID;
    if (v && !root) {  // lookup
      for (u32 s = h & (ht_slots - 1u);; s = (s + 1u) & (ht_slots - 1u)) {
        u32 e = ht[s];
        if (e == 0u) break;
        if (hh[s] == h && intern_eq(B, a, b, io.noff[rep[e - 1u]], io.noff[rep[e - 1u] + 1u])) { id = e - 1u; break; }
      }
    }
    u64 need = __builtin_amdgcn_ballot_w64(v && !root && id == INVALID);
    while (need) {  // admit the chunk's new names, first appearance first
      u32 ld = (u32)__builtin_ctzll(need);
      u32 lh = __builtin_amdgcn_readlane(h, ld), la = __builtin_amdgcn_readlane(a, ld), lb = __builtin_amdgcn_readlane(b, ld);
      if (k >= max_names) { st = -1; break; }
      bool mine = (need >> l) & 1ull;
      bool same = mine && h == lh && intern_eq(B, a, b, la, lb);
      if (same) id = k;
      if (l == ld) {
        u32 s = h & (ht_slots - 1u);
        while (ht[s] != 0u) s = (s + 1u) & (ht_slots - 1u);
        ht[s] = k + 1u;
        hh[s] = h;
        rep[k] = (u32)r;
      }
      __threadfence_block();
      __builtin_amdgcn_wave_barrier();
      k++;
      need &= ~__builtin_amdgcn_ballot_w64(same);
    }
    if (v) io.id[r] = (u16)(root ? ROOT_AGENT : id);
  }
  return k;
}
__global__ __launch_bounds__(64) void k_intern(InternIO io, u32 n_groups) {
  __shared__ u32 ht[INTERN_HT];      // 0 = empty, else id + 1
  __shared__ u32 hh[INTERN_HT];      // hash of the slot's name
  __shared__ u32 rep[INTERN_MAX];    // a ref naming each id (its first appearance)
  __shared__ u32 rk[INTERN_MAX];     // rank of each id
  u32 g = blockIdx.x, l = threadIdx.x;
  if (g >= n_groups) return;
  for (u32 i = l; i < INTERN_HT; i += 64) ht[i] = 0u;
  __builtin_amdgcn_wave_barrier();
  const unsigned char* B = io.bytes;
  u64 r0 = io.roff[g], r1 = io.roff[g + 1];
  i32 st;
  u32 k = intern_admit(io, g, ht, hh, rep, INTERN_HT, INTERN_MAX, st);
  __builtin_amdgcn_wave_barrier();
  // ranks: names smaller than each distinct name (lane per name)
  for (u32 i = l; i < k; i += 64) {
    u32 ra = rep[i], a = io.noff[ra], b = io.noff[ra + 1], cnt = 0;
    for (u32 j = 0; j < k; j++) {
      u32 rj = rep[j];
      cnt += intern_less(B, io.noff[rj], io.noff[rj + 1], a, b) ? 1u : 0u;
    }
    rk[i] = cnt;
  }
  __builtin_amdgcn_wave_barrier();
  for (u64 r = r0 + l; r < r1; r += 64) {
    u32 id = io.id[r];
    io.rank[r] = (id == ROOT_AGENT || id >= k) ? INVALID : rk[id];
  }
  if (l == 0) {
    io.n_out[g] = k;
    io.status[g] = st;
  }
}

// Groups past INTERN_MAX distinct names (a document with more agents than the LDS table holds;
// the reference allows 65,535, AgentId = u16): the same admission with the table in HBM scratch,
// and ranks from a block-wide bitonic sort of the names (byte-lexicographic) instead of k^2
// counting.  Block (256 threads) per listed group; scratch per block: INTERN_BIG_HT slots x 2 +
// INTERN_BIG_MAX x 3 u32.
constexpr u32 INTERN_BIG_MAX = 65534, INTERN_BIG_HT = 1u << 17, INTERN_BIG_SORT = 1u << 16;
constexpr u64 INTERN_BIG_SCRATCH = 2ull * INTERN_BIG_HT + 3ull * INTERN_BIG_SORT;  // u32 per group
__global__ __launch_bounds__(256) void k_intern_big(InternIO io, const u32* groups, u32 n, u32* scratch) {
  if (blockIdx.x >= n) return;
  u32 g = groups[blockIdx.x], t = threadIdx.x;
  u32* ht = scratch + (u64)blockIdx.x * INTERN_BIG_SCRATCH;
  u32* hh = ht + INTERN_BIG_HT;
  u32* rep = hh + INTERN_BIG_HT;
  u32* rk = rep + INTERN_BIG_SORT;
  u32* srt = rk + INTERN_BIG_SORT;
  for (u32 i = t; i < INTERN_BIG_HT; i += 256) ht[i] = 0u;
  __syncthreads();
  __shared__ u32 sk;
  __shared__ i32 sst;
  if (t < 64) {
    i32 st;
    u32 k = intern_admit(io, g, ht, hh, rep, INTERN_BIG_HT, INTERN_BIG_MAX, st);
    if (t == 0) { sk = k; sst = st; }
  }
  __syncthreads();
  u32 k = sk;
  const unsigned char* B = io.bytes;
  u32 P = 1;
  while (P < k) P <<= 1;
  for (u32 i = t; i < P; i += 256) srt[i] = i < k ? i : INVALID;
  __syncthreads();
  auto less = [&](u32 x, u32 y) -> bool {  // INVALID (padding) sorts last
    if (y == INVALID) return x != INVALID;
    if (x == INVALID) return false;
    u32 rx = rep[x], ry = rep[y];
    return intern_less(B, io.noff[rx], io.noff[rx + 1], io.noff[ry], io.noff[ry + 1]);
  };
  for (u32 size = 2; size <= P; size <<= 1) {
    for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
      for (u32 i = t; i < P / 2; i += 256) {
        u32 lo = 2 * i - (i & (stride - 1)), hi = lo + stride;  // pair (lo, hi) of this step
        bool up = (lo & size) == 0;
        u32 x = srt[lo], y = srt[hi];
        if (less(y, x) == up) { srt[lo] = y; srt[hi] = x; }
      }
      __syncthreads();
    }
  }
  for (u32 i = t; i < k; i += 256) rk[srt[i]] = i;
  __syncthreads();
  u64 r0 = io.roff[g], r1 = io.roff[g + 1];
  for (u64 r = r0 + t; r < r1; r += 256) {
    u32 id = io.id[r];
    io.rank[r] = (id == ROOT_AGENT || id >= k) ? INVALID : rk[id];
  }
  if (t == 0) {
    io.n_out[g] = k;
    io.status[g] = sst;
  }
}

}  // namespace crdt
