/*
 * crdt_gpu.h — C ABI of the MI355X list-CRDT engine (drop-in boundary for the hot path of
 * josephg/text-crdt-rust: position <-> CRDT-location remapping and batch merge of list-CRDT
 * edits, across many documents at once).
 *
 * The reference exposes this path only as a Rust crate API (src/lib.rs:3-14); there is no FFI.
 * Each entry point below names the reference function it replaces; a Rust binding would wrap
 * these in `ListCRDT`-shaped methods (see INTEGRATION.md for the cgo-free Rust `extern "C"`
 * block and a ctypes stub).
 *
 * Conventions
 *   - Caller-owned host buffers; the engine owns device memory.  Calls are synchronous at return
 *     unless named *_async (then crdt_sync()).  One engine per host thread per device.
 *   - Positions and lengths count Unicode scalar values (chars().count(), doc.rs:383).
 *   - Agent 0xFFFF = ROOT (doc.rs:68).  Order 0xFFFFFFFF = ROOT_ORDER (list/mod.rs:30).
 *   - A failing op poisons only its document (doc_status < 0); later ops of that document are
 *     skipped.  This mirrors "the reference panics": the document is dead, the rest live on.
 *   - Return value of every function: 0 = ok, < 0 = API error (CRDT_E_*).
 *   - A stage / apply call names each document at most once (its docs[] has no duplicates);
 *     a call that names a document twice returns CRDT_E_ARG and changes nothing.  Likewise a
 *     remote call with a malformed wire batch: every wire of the call is parsed before any
 *     author is interned, so a call that returns CRDT_E_WIRE changes nothing either (agent ids
 *     handed out later are those of a history in which the call never happened).  Every stage
 *     call replaces the staged streams of all documents (documents not named get none).
 *   - No exception crosses this boundary: host memory that runs out while a stage / apply call
 *     parses and encodes its input is CRDT_E_NOMEM.
 */
#ifndef CRDT_GPU_H
#define CRDT_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-document status codes (identical in the oracle and the kernels) ---------------- */
#define CRDT_OK 0
#define CRDT_ERR_POS_OOB -1          /* local op outside the document (root.rs:71,79; mutations.rs:573) */
#define CRDT_ERR_SEQ -2              /* remote txn seq != next seq of its agent (doc.rs:247) */
#define CRDT_ERR_UNKNOWN_AGENT -3    /* agent name/id not known to the document (doc.rs:92,237) */
#define CRDT_ERR_UNKNOWN_ID -4       /* (agent, seq) does not name an inserted item (doc.rs:27, root.rs:288) */
#define CRDT_ERR_NONTERMINATING -5   /* the reference's integrate / remote-delete loop never exits here */
#define CRDT_ERR_CAPACITY -6         /* a per-document structural limit was exceeded */
#define CRDT_ERR_EMPTY_TXN -7        /* zero-length txn (reference underflows first_order+0-1, doc.rs:351) */
#define CRDT_ERR_FRONTIER -8         /* advance_branch_by assertion (doc.rs:43) */
#define CRDT_ERR_BAD_INPUT -9        /* malformed record / zero-length remote op */
#define CRDT_ERR_INTERNAL -10

/* ---- API errors ---------------------------------------------------------------------------- */
#define CRDT_E_ARG -100
#define CRDT_E_DEVICE -101   /* no usable MI355X / HIP error */
#define CRDT_E_NOMEM -102
#define CRDT_E_WIRE -103     /* malformed remote wire batch */

typedef struct crdt_engine crdt_engine;

typedef struct {
  uint32_t leaf_cap;   /* 32 = reference release layout (range_tree/mod.rs:38), 4 = debug layout */
  int32_t device;      /* HIP device ordinal */
} crdt_cfg;

/* LocalOp (src/common.rs:45-50) with the inserted string replaced by its char count. */
typedef struct {
  uint32_t pos;
  uint32_t del_len;
  uint32_t ins_len;
} crdt_local_op;

/* One apply_local_txn(agent, &ops[..n_ops]) call (doc.rs:376). */
typedef struct {
  uint32_t agent;
  uint32_t n_ops;
} crdt_local_txn;

/* ListCRDT::new() x n — (re)creates n_docs empty documents (doc.rs:51-64). */
int crdt_engine_create(const crdt_cfg* cfg, crdt_engine** out);
void crdt_engine_destroy(crdt_engine* e);
int crdt_docs_alloc(crdt_engine* e, uint64_t n_docs);
uint64_t crdt_num_docs(const crdt_engine* e);

/* ListCRDT::get_or_create_agent_id (doc.rs:66-80), n independent (doc, name) requests. */
int crdt_agent_intern(crdt_engine* e, uint64_t n, const uint32_t* doc, const char* const* names,
                      uint16_t* agent_out);
/* The same interning done by a device kernel (one wave per document): name i is
 * the bytes [name_off[i], name_off[i+1]) of `bytes` (any bytes, not NUL-terminated).  Ids are
 * identical to crdt_agent_intern on the same call.  rank_out (optional): each name's rank among
 * the document's names in byte-lexicographic order (Rust str Ord; the order the integrate
 * tie-break compares, doc.rs:207), INVALID for "ROOT".  Up to 65,534 names per document (AgentId is
 * u16, doc.rs:66-80; CRDT_E_ARG beyond): documents with at most 1,024 names intern in an LDS table,
 * larger ones again with the table in HBM and ranks from a sort. */
int crdt_agent_intern_dev(crdt_engine* e, uint64_t n, const uint32_t* doc, const uint64_t* name_off,
                          const char* bytes, uint16_t* agent_out, uint32_t* rank_out);

/* ListCRDT::apply_local_txn (doc.rs:376-469) for many documents.  Document docs[i] applies txns
 * txns[txn_off[i] .. txn_off[i+1]) in order; ops are concatenated in txn order. */
int crdt_apply_local(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint64_t* txn_off,
                     const crdt_local_txn* txns, const crdt_local_op* ops, int32_t* doc_status);

/* ListCRDT::apply_remote_txn (doc.rs:242-348) for many documents: wire[i] (wire_len[i] bytes) is
 * a remote wire batch applied to docs[i].
 *
 * Remote wire batch (serialises RemoteTxn, src/list/external_txn.rs:5-30; little endian u32s):
 *   'RTX1' (0x31585452) | n_names | n_names x {byte_len, utf-8 bytes, zero pad to 4}
 *   | n_txns | n_txns x { agent_name, seq, n_parents, n_ops,
 *                         n_parents x {name, seq},
 *                         n_ops x {kind (0 Ins, 1 Del), a_name, a_seq, b_name, b_seq, len} }
 *   Ins: a = origin_left, b = origin_right, len = chars inserted.  Del: a = target, len.
 *   The name "ROOT" denotes the root id (doc.rs:68).
 *
 * A wire is a peer's input and is checked as such.  CRDT_E_WIRE: wrong magic, a count or a name
 * length that the remaining bytes cannot hold (counts are checked before anything is sized by
 * them), a name index outside the name table, a kind other than 0 or 1, a batch that ends early.
 * Names are compared as bytes, pad bytes and a Del's b are not looked at, and bytes after the last
 * txn are ignored.  CRDT_E_ARG: a wire pointer that is NULL or not 4-byte aligned (the batch is
 * read in place as u32s; the pointer is not dereferenced).
 * Limits: a txn holds at most 65,535 parents and 2^26 - 1 ops, an op at most 2^28 - 1 items.  A
 * txn beyond them is well-formed wire but cannot be replayed: its document stops at that txn with
 * CRDT_ERR_BAD_INPUT, unchanged by it, like one with a zero-length op. */
int crdt_apply_remote_wire(crdt_engine* e, uint64_t n_docs, const uint32_t* docs,
                           const uint8_t* const* wire, const uint64_t* wire_len, int32_t* doc_status);

/* Staged form (inputs resident in HBM, then replay without host transfers): */
int crdt_stage_local(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint64_t* txn_off,
                     const crdt_local_txn* txns, const crdt_local_op* ops);
int crdt_stage_remote_wire(crdt_engine* e, uint64_t n_docs, const uint32_t* docs,
                           const uint8_t* const* wire, const uint64_t* wire_len);
/* Shared local streams: stream k = txns[stream_txn_off[k] .. stream_txn_off[k+1]) (ops concatenated
 * in txn order); document docs[i] replays stream stream_of_doc[i].  Each stream is encoded and
 * uploaded once (device copies per document), e.g. a corpus of documents drawn from few traces. */
int crdt_stage_local_shared(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint32_t* stream_of_doc,
                            uint32_t n_streams, const uint64_t* stream_txn_off, const crdt_local_txn* txns,
                            const crdt_local_op* ops);
/* One wire batch replicated to docs [0, n_docs) of a fresh engine; name index `rename_idx` of the
 * batch's name table is replaced per document by names[d] (randomised client ids). */
int crdt_stage_remote_replicated(crdt_engine* e, const uint8_t* wire, uint64_t wire_len,
                                 uint32_t rename_idx, const char* const* names);
/* On-device edit generator (BASELINE config 4): each document docs[i] gets n_ops local txns by
 * `agent`, one LocalOp each, drawn on the GPU inside the replay wave with the semantics of the
 * reference's make_random_change (doc.rs:544-569; insert 1 char w.p. 0.55 below 100 chars else
 * 0.45, delete 1..10 chars).  Per-document seed = low 32 bits of splitmix64(seed ^ doc).  Only
 * one GEN record per document is staged, so 10^6 documents need no host-side op stream. */
int crdt_stage_random(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const char* agent, uint32_t n_ops,
                      uint64_t seed);
/* Reset every document to ListCRDT::new() state, keeping interned agents and staged records. */
int crdt_reset_async(crdt_engine* e);
/* Replay the staged records of every document (+ capacity growth/resume as needed). */
int crdt_run(crdt_engine* e, int32_t* doc_status /* n_docs, may be NULL */);
int crdt_run_async(crdt_engine* e);   /* single launch; no growth handling */
/* Rebuild the flat per-document index: canonical span array (stream compaction of the leaf
 * entries with YjsSpan::can_append), visible-prefix scan, order->span scatter.  (The digests are
 * not part of it: crdt_digest / crdt_digest_dev_async compute them on request.) */
int crdt_publish_async(crdt_engine* e);
int crdt_sync(crdt_engine* e);

/* ---- queries (the reference's README operations, README.md:22-25) ------------------------- */
/* Doc location -> CRDT location (§3.3: cursor_at_content_pos + client_with_order.get).
 * Invalid positions give agent 0xFFFF, seq 0xFFFFFFFF. */
int crdt_pos_to_loc(crdt_engine* e, uint64_t n, const uint32_t* doc, const uint32_t* pos,
                    uint16_t* agent, uint32_t* seq);
/* CRDT location -> doc location (§3.4: seq_to_order + Cursor::count_pos).  deleted: 0/1, 2 = unknown id. */
int crdt_loc_to_pos(crdt_engine* e, uint64_t n, const uint32_t* doc, const uint16_t* agent,
                    const uint32_t* seq, uint32_t* pos, uint8_t* deleted);
/* Device-pointer forms for batched query benchmarking (inputs/outputs already in HBM). */
int crdt_pos_to_loc_dev_async(crdt_engine* e, uint64_t n, const uint32_t* doc, const uint32_t* pos,
                              uint16_t* agent, uint32_t* seq);
int crdt_loc_to_pos_dev_async(crdt_engine* e, uint64_t n, const uint32_t* doc, const uint16_t* agent,
                              const uint32_t* seq, uint32_t* pos, uint8_t* deleted);

/* ---- text materialisation (the reference's USE_INNER_ROPE rope) ----------
 * The reference's rope (doc.rs:14-17, 59, 98 of list/mod.rs) receives the inserted string at
 * cursor.count_pos() on every integrate (doc.rs:230-233) and loses the deleted visible range on
 * every local delete (doc.rs:430-432); its remote-delete arm is todo!() (doc.rs:329-333), and
 * ListCRDT::to_string returns it (doc.rs:498-505).  Here the rope is computed from the published
 * index instead: the visible items in document order, each replaced by its code point.
 *
 * Content is an order-indexed UTF-32 table per document: content[order] is the code point of the
 * item with that order (orders are assigned as in assign_order_to_client, doc.rs:155-165: within a
 * txn, op by op, a LocalOp's deleted orders first, then its inserted chars).  Entries at delete
 * orders are never read.  Streams are shared: document docs[i] reads stream stream_of_doc[i] =
 * content[stream_off[k] .. stream_off[k+1]).  A call replaces all content set before. */
int crdt_set_content(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint32_t* stream_of_doc,
                     uint32_t n_streams, const uint64_t* stream_off, const uint32_t* content);
/* Write every document's text on the device (publishes first if needed; stream-ordered). */
// As crdt_set_content, with one stream that every listed document gets its own device copy of
// (docs[i] reads copy i); replaces all previously set content.
int crdt_set_content_copies(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint32_t* content,
                            uint64_t len);
int crdt_materialize_async(crdt_engine* e);
/* ListCRDT::to_string (doc.rs:498-505) as UTF-32: *n_out = visible chars; out may be NULL (size
 * query), else cap >= *n_out.  CRDT_E_ARG if the document has no content or its stream is shorter
 * than the document's orders, or if it is poisoned. */
int crdt_text(crdt_engine* e, uint32_t doc, uint32_t* out, uint64_t cap, uint64_t* n_out);
/* Per-document 64-bit digest of the text (same as the oracle's text_digest; 0 = not materialised). */
int crdt_text_digest(crdt_engine* e, uint64_t* per_doc /* n_docs */);
int crdt_last_materialize_ms(crdt_engine* e, double* ms);

/* ---- what a replay changed: per-document text patches between versions ---------------------
 * No reference counterpart: with the rope's remote-delete arm todo!() (doc.rs:329-333) a caller of
 * apply_remote_txn cannot learn what changed short of re-reading the text.
 *
 * A document's version is its next order (get_next_order); orders are dense and assigned in
 * application order, so "the document at version v" is the effect of every insert item and delete
 * op with order < v, for any 0 <= v <= version (also inside a txn).  Walk the items of the current
 * state in document order.  An item with order x is old-visible if x < v and no delete-log entry
 * (key, target, len) covers it with a delete order key + (x - target) < v, and new-visible if its
 * canonical span has len > 0.  Old and new visible: closes the current patch.  Old only: adds 1 to
 * its del_len.  New only: appended to its inserted items.  Neither: ignored.  A patch is a maximal
 * run of old-only and new-only items; pos = new-visible items before it.  Applied front to back
 * like crdt_local_ops, each at its pos in the text the previous ones left, the patches turn the
 * text at version v into the current text. */
/* next order of each listed document (get_next_order); batched form of export_sizes[10] */
int crdt_doc_version(crdt_engine* e, uint64_t n, const uint32_t* doc, uint32_t* version);
typedef struct { uint32_t pos, del_len, ins_len, ins_off; } crdt_patch;   /* ins_off: first inserted item
                                                                             in this document's ins arrays */
/* Compute, on the device and stream-ordered, the patches from version since[i] to now for docs[i]
 * (publishes first if needed, like crdt_materialize_async).  docs has no duplicates.  Replaces the
 * previous diff result.  Does not change any document.  (The call waits once inside, for the two
 * result totals that size the result arrays.)  CRDT_E_NOMEM if an allocation fails: the engine
 * stays usable, without a diff result. */
int crdt_diff_async(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint32_t* since);
/* The patches between two versions of docs[i]: from[i] and to[i], any 0 <= from, to <= version
 * (also inside a txn).  For a version v an item with order x is visible at v if x < v and no
 * delete-log entry (key, target, len) covers it with a delete order key + (x - target) < v: the
 * old-visible above, unchanged (a delete run that straddles v counts with its part below v).  The
 * walk is the diff's, over the items of the current state in document order, with an item old if
 * it is visible at from[i] and new if it is visible at to[i].  Old and new: closes the current
 * patch.  Old only: adds 1 to its del_len.  New only: appended to its inserted items.  Neither:
 * ignored, closes nothing.  A patch is a maximal run of old-only and new-only items; pos = new
 * items before it.  Applied front to back, the patches turn the text at from[i] into the text at
 * to[i].  from > to is allowed (the patches that take the newer text back to the older one);
 * from == to gives no patches; to == version gives exactly the result of crdt_diff_async(from),
 * array for array, ins_off included.
 * The result is the diff result: this call replaces it under the rules of crdt_diff_async
 * (stream-ordered, one wait inside, publishes first if needed, no duplicates in docs, CRDT_E_NOMEM
 * leaves the engine usable without a diff result), and crdt_diff_counts, crdt_diff_read,
 * crdt_last_diff_ms and crdt_rebase_async(CRDT_REBASE_FROM_DIFF) serve it without knowing which
 * call made it.  An index whose from[i] or to[i] is above the document's version, or whose
 * document is poisoned, has no result; the other indexes are not affected.  Does not change any
 * document. */
int crdt_diff_between_async(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint32_t* from,
                            const uint32_t* to);
/* Causal versions.  Orders are assigned in application order, so a version "everything with order
 * < v" means something on this replica only; what peers exchange is a version vector.  A version
 * vector of document d is vv[a] for the document's agent ids a = 0 .. n_agents - 1 (crdt_agent_intern;
 * mapping names to ids across replicas is the caller's).  The version it names is the set S of
 * orders x whose id (agent, seq) has seq < vv[agent]: delete ops as well as insert items, a delete
 * op's orders being in client_with_order too.  An item with order x is visible at S if x is in S
 * and no delete-log entry (key, target, len) covers x with its delete order key + (x - target) in
 * S.  S is taken as a set: nothing requires it to be causally closed ("now minus one txn" is a
 * legitimate version), and whether it is closed is reported (crdt_diff_vv_closed).  Entries beyond
 * a vector's length count as 0.  Every order-prefix version is such a set: an agent's seqs are
 * applied in seq order, so the orders below v hold a seq prefix of every agent.
 *
 * The vector of the order prefix version[q] of doc[q] (version == NULL: now), n_agents(doc[q])
 * entries written at vv_out[vv_off[q]]; vv_off has n + 1 ascending entries, and slot q is
 * vv_off[q] .. vv_off[q + 1].  CRDT_E_ARG if a slot is smaller than the document's agent count, a
 * version is above the document's, or a document is poisoned.  Computed on the device (syncs). */
int crdt_version_vector(crdt_engine* e, uint64_t n, const uint32_t* doc, const uint32_t* version,
                        const uint64_t* vv_off, uint32_t* vv_out);
/* The same on device arrays, stream-ordered and without checks on the host: a query that has no
 * answer (see above) fills its slot with 0xFFFFFFFF. */
int crdt_version_vector_dev_async(crdt_engine* e, uint64_t n, const uint32_t* doc, const uint32_t* version,
                                  const uint64_t* vv_off, uint32_t* vv_out);
/* The patches between two causal versions of docs[i]: the vectors from_vv[vv_off[i] .. vv_off[i+1])
 * and to_vv[vv_off[i] .. vv_off[i+1]), the same layout on both sides (vv_off has n_docs + 1
 * ascending entries).  The walk, the classes, the patches, pos, ins_off and the inserted-item
 * arrays are exactly those of crdt_diff_between_async, with "visible at from[i] / to[i]" replaced
 * by "visible at S_from / S_to" as defined above; on the vectors of two order prefixes
 * (crdt_version_vector) the result is that of crdt_diff_between_async on the prefixes, array for
 * array.
 * The result is the diff result: this call replaces it under the rules of crdt_diff_async
 * (stream-ordered, one wait inside, publishes first if needed, no duplicates in docs, CRDT_E_NOMEM
 * leaves the engine usable without a diff result), and crdt_diff_counts, crdt_diff_read,
 * crdt_last_diff_ms and crdt_rebase_async(CRDT_REBASE_FROM_DIFF) serve it without knowing which
 * call made it.  An index with a vector longer than the document's agent count or an entry above
 * that agent's next seq, or whose document is poisoned, has no result; the other indexes are not
 * affected.  Does not change any document. */
int crdt_diff_vv_async(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint64_t* vv_off,
                       const uint32_t* from_vv, const uint32_t* to_vv);
/* One byte per index of the last crdt_diff_vv_async and side (either may be NULL; syncs): 1 if the
 * side's S is causally closed -- every txn with at least one order in S has all its parents but
 * ROOT in S, and S holds a prefix of every txn it touches -- else 0 (also for an index without a
 * result).  CRDT_E_ARG if the last diff result was not made by crdt_diff_vv_async. */
int crdt_diff_vv_closed(crdt_engine* e, uint8_t* closed_from, uint8_t* closed_to);
/* Sizes of the last diff, per docs[i] of that call (syncs).  An index whose since[i] is above the
 * document's version, or whose document is poisoned, has no result: both sizes are 0xFFFFFFFF and
 * crdt_diff_read of it returns CRDT_E_ARG; the other indexes are not affected. */
int crdt_diff_counts(crdt_engine* e, uint32_t* n_patches, uint32_t* n_ins);
/* Result i of the last diff: patches[n_patches[i]], ins_order[n_ins[i]] (order of every inserted item),
 * ins_text[n_ins[i]] (its code point through crdt_set_content, as set when the diff was computed;
 * may be NULL; CRDT_E_ARG if asked for and the document has no content or too short a stream). */
int crdt_diff_read(crdt_engine* e, uint64_t i, crdt_patch* patches, uint32_t* ins_order, uint32_t* ins_text);
int crdt_last_diff_ms(crdt_engine* e, double* ms);   /* HIP events, like crdt_last_materialize_ms */

/* ---- text edits in units: the diff for a caller that keeps UTF-8 or UTF-16 text ------------------
 * The diff above, restated in the units of "encoded text and unit offsets" below (enc is
 * CRDT_ENC_UTF8: bytes, or CRDT_ENC_UTF16: uint16_t in host byte order), so that a Rust String, a
 * JS string or an editor buffer can apply it without encoding the whole text.
 *
 * Take the item walk and the old-visible / new-visible classes of the diff for (docs[i], since[i])
 * unchanged.  The width w(x) of the item with order x is the number of units crdt_encode_async
 * writes for its content value (crdt_set_content) under enc, with the same rule: a value that is no
 * Unicode scalar value counts, and is written, as U+FFFD.  Edit p is patch p of the diff:
 *   pos, del_len, ins_len  the patch's;
 *   unit       sum of w over the new-visible items before it: what crdt_pos_to_units answers for
 *              pos on an encode of the current text;
 *   del_units  sum of w over its old-only (deleted) items, which are in no current text;
 *   ins_units  sum of w over its new-only (inserted) items;
 *   ins_off    first unit of its inserted text in the index's inserted-unit pool = the ins_units
 *              of the index's earlier edits;
 *   reserved   0.
 * The inserted-unit pool of an index is the concatenation, in patch order, of the encodings of
 * every inserted item.  Applied front to back to the encoded text at since[i], each replacing
 * del_units units at unit (an offset in the text the earlier edits left) with its ins_units units,
 * the edits give the encoded current text.
 *
 * An index has no result (both counts 0xFFFFFFFF, crdt_edits_read returns CRDT_E_ARG, the other
 * indexes are not affected) when since[i] is above the document's version, the document is
 * poisoned, it has no content or a content stream shorter than its orders, or the sum of w over
 * all its orders is 0xFFFFFFFF or more. */
typedef struct { uint32_t pos, del_len, ins_len, unit, del_units, ins_units, ins_off, reserved; } crdt_edit;
/* Compute the edits on the device, stream-ordered (publishes first if needed).  docs has no
 * duplicates and enc is one of the two (CRDT_E_ARG).  Replaces the previous edits result; changes
 * no document and none of the diff result, the checkout, the blame result, the encode result, the
 * line index or the find result, and none of their calls touches the edits result;
 * crdt_docs_alloc frees it.  The result is a copy: it stays readable whatever is replayed or
 * published afterwards.  (The call waits once inside, for the two result totals.)  CRDT_E_NOMEM if
 * an allocation fails: the engine stays usable, without an edits result, and the same call then
 * succeeds. */
int crdt_edits_async(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint32_t* since, int enc);
/* The edits between two versions of docs[i]: from[i] and to[i], any 0 <= from, to <= version (also
 * inside a txn).  The item walk and the classes are exactly those of crdt_diff_between_async(from,
 * to): an item is old if it is visible at from[i] and new if it is visible at to[i].  The widths
 * w(x) and the fields are exactly those of crdt_edits_async.  Edit p is patch p of the two-version
 * diff: pos, del_len and ins_len are the patch's; unit is the sum of w over the new items before it
 * (what crdt_pos_to_units would answer for pos on an encode of the text at to[i]); del_units and
 * ins_units are the sums of w over its old-only and its new-only items; ins_off is the sum of the
 * earlier ins_units; reserved is 0.  The pool is the encodings of the new-only items in patch order.
 * Applied front to back to the encoded text at from[i], the edits give the encoded text at to[i].
 * from > to is allowed; from == to gives no edits; to == version gives exactly the result of
 * crdt_edits_async(from, enc), array for array, pool included.
 * An index has no result, as above, when from[i] or to[i] is above the document's version, the
 * document is poisoned, it has no content or a content stream shorter than its orders, or the sum
 * of w over all its orders is 0xFFFFFFFF or more; the other indexes are not affected.
 * The result is the edits result: this call replaces it under the rules of crdt_edits_async
 * (stream-ordered, one wait inside, publishes first if needed, no duplicates in docs, enc checked,
 * CRDT_E_NOMEM leaves the engine usable without an edits result and the same call then succeeds;
 * it changes no document and none of the other seven results), and crdt_edits_counts,
 * crdt_edits_read, crdt_last_edits_ms and crdt_rebase_async(CRDT_REBASE_FROM_EDITS) serve it
 * without knowing which call made it: for the rebase, old is the text at from[i] and new is the
 * text at to[i], in chars and in units. */
int crdt_edits_between_async(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint32_t* from,
                             const uint32_t* to, int enc);
/* Sizes of the last edits result, per docs[i] of that call (syncs); either may be NULL. */
int crdt_edits_counts(crdt_engine* e, uint32_t* n_edits, uint32_t* n_ins_units);
/* Result i: edits[n_edits[i]] and ins_units[n_ins_units[i]] (uint8_t or uint16_t by the call's enc);
 * either may be NULL. */
int crdt_edits_read(crdt_engine* e, uint64_t i, crdt_edit* edits, void* ins_units);
int crdt_last_edits_ms(crdt_engine* e, double* ms);   /* HIP events, like crdt_last_diff_ms */

/* ---- documents at a past version: text and position queries --------------------------------
 * No reference counterpart (the reference keeps no history of its rope).  "The document at version
 * v" is the sequence of old-visible items of the definition above, in document order, for any
 * 0 <= v <= version (also inside a txn); its text is their code points, its length their count,
 * its position p the p-th of them.  An item with order >= v does not exist at v.  For the same
 * application order this is the state of a replay that stopped at v.
 *
 * Build the views of docs[i] at version[i] on the device, stream-ordered (publishes first if
 * needed).  docs has no duplicates.  Replaces the previous checkout; changes no document and not
 * the diff result.  (The call waits once inside, for the total that sizes the result arrays.)
 * CRDT_E_NOMEM if an allocation fails: the engine stays usable, without a checkout. */
int crdt_checkout_async(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint32_t* version);
/* Length of every index of the last checkout (syncs).  An index whose version[i] is above the
 * document's version, or whose document is poisoned, has no result: its length is 0xFFFFFFFF, and
 * crdt_checkout_read of it and a host-form query that names it return CRDT_E_ARG; the other
 * indexes are not affected. */
int crdt_checkout_lens(crdt_engine* e, uint32_t* len);
/* View i: order[len[i]] (the order of every item, in document order) and text[len[i]] (its code
 * point through crdt_set_content, as set when the checkout was computed; may be NULL; CRDT_E_ARG
 * if asked for and the document has no content or too short a stream).  The arrays are copies:
 * they stay readable until the next checkout or crdt_docs_alloc, whatever happens to the documents. */
int crdt_checkout_read(crdt_engine* e, uint64_t i, uint32_t* order, uint32_t* text);
/* Text digest of every index (the function of crdt_text_digest; 0 without content or result). */
int crdt_checkout_digest(crdt_engine* e, uint64_t* per_index);
/* The README's two mappings on the views: idx[q] names an index of the last checkout; answers as
 * crdt_pos_to_loc / crdt_loc_to_pos (invalid position: agent 0xFFFF, seq 0xFFFFFFFF; deleted 0/1,
 * 2 = unknown id, which an id whose order is >= v is).  An idx out of range, or one without a
 * result, gives CRDT_E_ARG for the whole call and writes nothing.  The queries also read the
 * published index: CRDT_E_ARG once any document was replayed, staged and run, reset or published
 * again since the checkout. */
int crdt_pos_to_loc_at(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* pos, uint16_t* agent,
                       uint32_t* seq);
int crdt_loc_to_pos_at(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint16_t* agent, const uint32_t* seq,
                       uint32_t* pos, uint8_t* deleted);
/* Device-pointer forms (inputs/outputs already in HBM; async on the engine stream).  idx cannot be
 * checked on the host: a query whose idx is out of range or has no result is answered as an
 * invalid position / an unknown id. */
int crdt_pos_to_loc_at_dev_async(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* pos,
                                 uint16_t* agent, uint32_t* seq);
int crdt_loc_to_pos_at_dev_async(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint16_t* agent,
                                 const uint32_t* seq, uint32_t* pos, uint8_t* deleted);
int crdt_last_checkout_ms(crdt_engine* e, double* ms);   /* HIP events, like crdt_last_diff_ms */

/* ---- who wrote what: per-document authorship runs -------------------------------------------
 * No reference counterpart (print_stats is the nearest thing).  Walk the visible items of a
 * document's current state in document order (the items of the canonical spans with len > 0);
 * item number p of that walk is position p, and its id (agent, seq) is what crdt_pos_to_loc
 * answers for p.  A run is a maximal stretch of consecutive positions whose neighbours chain:
 * with CRDT_BLAME_AGENT when they have the same agent, with CRDT_BLAME_ID when they have the same
 * agent and the right one's seq is the left one's plus 1.  agent and seq of a run are those of
 * its first item: in ID mode item pos + j has id (agent, seq + j), so the runs are the whole
 * pos -> loc table, run-length encoded.  Runs come in position order and their lens sum to the
 * document's length; an empty or fully deleted document has none.  Deleted items are not part of
 * the walk: two visible stretches with tombstones between them chain if their ids allow it. */
enum { CRDT_BLAME_AGENT = 0, CRDT_BLAME_ID = 1 };
typedef struct { uint32_t pos, len, agent, seq; } crdt_blame_run;
/* Compute, on the device and stream-ordered, the runs of docs[i] (publishes first if needed, like
 * crdt_materialize_async).  docs has no duplicates; an unknown mode is CRDT_E_ARG.  Replaces the
 * previous blame result; changes no document and neither the diff result nor the checkout.  (The
 * call waits once inside, for the total that sizes the result array.)  CRDT_E_NOMEM if an
 * allocation fails: the engine stays usable, without a blame result. */
int crdt_blame_async(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, int mode);
/* Runs per docs[i] of the last blame (syncs).  An index whose document is poisoned has no result:
 * its count is 0xFFFFFFFF and crdt_blame_read of it returns CRDT_E_ARG; the other indexes are not
 * affected. */
int crdt_blame_counts(crdt_engine* e, uint32_t* n_runs);
/* Result i of the last blame: runs[n_runs[i]].  CRDT_E_ARG for i out of range or before any
 * blame.  The array is a copy: it stays readable until the next blame or crdt_docs_alloc,
 * whatever happens to the documents. */
int crdt_blame_read(crdt_engine* e, uint64_t i, crdt_blame_run* runs);
int crdt_last_blame_ms(crdt_engine* e, double* ms);   /* HIP events, like crdt_last_diff_ms */

/* ---- encoded text and unit offsets: UTF-8 / UTF-16 output, unit offset <-> position ----------
 * ListCRDT::to_string (doc.rs:498-505) returns a Rust String, which is UTF-8; an editor or LSP
 * client addresses text by UTF-16 code-unit offsets; every position of this header counts chars.
 * These calls hand over the text of crdt_text in either form and convert offsets both ways, on the
 * device.
 *
 * A content value c is a scalar value iff c < 0xD800 or 0xE000 <= c <= 0x10FFFF; any other value
 * (a surrogate, or above 0x10FFFF) is encoded as U+FFFD.  CRDT_ENC_UTF8: the unit is a byte, the
 * width 1 / 2 / 3 / 4 for c below 0x80 / 0x800 / 0x10000 / otherwise, standard bit layout.
 * CRDT_ENC_UTF16: the unit is a uint16_t in host byte order, the width 1 below 0x10000, otherwise 2:
 * 0xD800 + ((c - 0x10000) >> 10), then 0xDC00 + ((c - 0x10000) & 0x3FF).  A document's encoded text
 * is the concatenation of the encodings of its visible items in document order, the items of
 * crdt_text; chars is their count, units the encoded length in units. */
enum { CRDT_ENC_UTF8 = 0, CRDT_ENC_UTF16 = 1 };
/* Encode, on the device and stream-ordered, the text of docs[i] (materialises first if needed, and
 * therefore publishes).  docs has no duplicates; an unknown enc is CRDT_E_ARG.  Replaces the
 * previous encode result; changes no document and none of the diff result, the checkout and the
 * blame result.  (The call waits once inside, for the total that sizes the unit array.)
 * CRDT_E_NOMEM if an allocation fails: the engine stays usable, without an encode result. */
int crdt_encode_async(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, int enc);
/* Units and chars per docs[i] of the last encode (syncs; either pointer may be NULL).  An index
 * whose document is poisoned, has no content or too short a content stream has no result: both are
 * 0xFFFFFFFF, crdt_encode_read of it and a host-form query that names it return CRDT_E_ARG; the
 * other indexes are not affected.  A document whose units would not fit below 0xFFFFFFFF has no
 * result either. */
int crdt_encode_lens(crdt_engine* e, uint32_t* units, uint32_t* chars);
/* Result i of the last encode: units[i] units (bytes, or uint16_t) into out; cap_units >= units[i].
 * CRDT_E_ARG for i out of range or before any encode. */
int crdt_encode_read(crdt_engine* e, uint64_t i, void* out, uint64_t cap_units);
/* The two mappings on the last encode's results: idx[q] names an index of it.
 *   pos -> units: for pos <= chars the units before char pos (pos == chars gives units), else
 *     0xFFFFFFFF.
 *   units -> pos: for u < units the char whose encoding covers unit u, with mid = 1 if u is not
 *     that char's first unit (a continuation byte / a low surrogate), else 0; u == units gives
 *     chars, mid 0; u > units gives 0xFFFFFFFF, mid 0.  mid may be NULL.
 * The pos -> units answer of a units -> pos answer is <= u, with equality exactly when mid == 0.
 * An idx out of range, or one without a result, gives CRDT_E_ARG for the whole call and writes
 * nothing; so does a query before any encode.  The queries read nothing but the encode result
 * (the unit array and its index): result and queries stay valid until the next encode or
 * crdt_docs_alloc, whatever is replayed, published or materialised in between. */
int crdt_pos_to_units(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* pos, uint32_t* unit);
int crdt_units_to_pos(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* unit, uint32_t* pos,
                      uint8_t* mid);
/* Device-pointer forms (inputs/outputs already in HBM; async on the engine stream).  idx cannot be
 * checked on the host: a query whose idx is out of range or has no result is answered 0xFFFFFFFF,
 * with mid = 0. */
int crdt_pos_to_units_dev_async(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* pos,
                                uint32_t* unit);
int crdt_units_to_pos_dev_async(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* unit,
                                uint32_t* pos, uint8_t* mid);
int crdt_last_encode_ms(crdt_engine* e, double* ms);   /* HIP events, like crdt_last_diff_ms */

/* ---- line index: line counts, line starts, (line, column) <-> position -------------------------
 * An LSP Position is (line, character in UTF-16 units); a compiler diagnostic is line:column in
 * bytes.  These calls index the lines of the last encode result on the device: index i of the line
 * index is index i of that encode.
 *
 *  - The text is the encoded text of crdt_encode_async: its units and its chars.
 *  - CRDT_EOL_LF: a break follows every U+000A.
 *  - CRDT_EOL_ANY: a break follows every U+000A, and every U+000D that is not immediately followed
 *    by U+000A in the same document.  CR LF is one break, after the LF; a CR that is the document's
 *    last char is a break.
 *  - No other char breaks a line in either mode (not U+000B, U+000C, U+0085, U+2028, U+2029).
 *  - Line 0 starts at unit 0, char 0; line k >= 1 starts at the unit and char after the k-th break.
 *  - n_lines = breaks + 1: an empty document has one (empty) line, and a text that ends in a break
 *    has an empty last line.
 *  - A line's extent runs from its start to the next line's start, its terminator included; the
 *    last line's runs to {units, chars}.
 *  - pos -> (line, col): for pos <= chars the line is the last one whose start char is <= pos;
 *    col = pos - start.pos (CRDT_COL_CHARS), or (units before char pos) - start.unit
 *    (CRDT_COL_UNITS: bytes after CRDT_ENC_UTF8, UTF-16 code units after CRDT_ENC_UTF16).
 *    pos == chars is the end-of-document cursor on the last line; pos > chars gives line and col
 *    0xFFFFFFFF.
 *  - (line, col) -> pos: valid iff line < n_lines and col < the line's extent in that column kind;
 *    on the last line col == extent is valid too and gives chars.  Otherwise pos is 0xFFFFFFFF and
 *    mid 0.  With CRDT_COL_UNITS a column that falls inside a char gives that char with mid = 1, as
 *    the units -> pos mapping of the encode does.  The two mappings are inverse bijections between
 *    [0, chars] and the valid (line, col) pairs with mid == 0.  (A caller that wants the LSP clamp
 *    reads the extents from the line starts.) */
enum { CRDT_EOL_LF = 0, CRDT_EOL_ANY = 1 };
enum { CRDT_COL_UNITS = 0, CRDT_COL_CHARS = 1 };
typedef struct { uint32_t unit, pos; } crdt_line_start;
/* Index, on the device and stream-ordered, the lines of every index of the last encode (the call
 * waits once inside, for the total that sizes the table).  CRDT_E_ARG before any encode result and
 * for an unknown eol.  Replaces the previous line index: a second call on the same encode is how a
 * caller switches eol.  Changes no document, and neither the encode result nor the diff result, the
 * checkout and the blame result.  The line index belongs to the encode result it was built from:
 * a later encode call, successful or not, drops it, and so does crdt_docs_alloc; the reads and
 * queries below then return CRDT_E_ARG until the next line index is built.  Until then it stays
 * valid whatever is replayed, published or materialised: the kernels read nothing but the encode
 * result and the line table.
 * CRDT_E_NOMEM if an allocation fails: the engine stays usable, without a line index and with the
 * encode result intact. */
int crdt_lines_async(crdt_engine* e, int eol);
/* Lines per index of that encode (syncs).  An index the encode has no result for has none here:
 * its count is 0xFFFFFFFF, reading its starts returns CRDT_E_ARG, and a host-form query that names
 * it returns CRDT_E_ARG for the whole call and writes nothing (as does an idx out of range). */
int crdt_line_counts(crdt_engine* e, uint32_t* n_lines);
/* The starts of the n_lines[i] lines of index i; the first is {0, 0}. */
int crdt_lines_read(crdt_engine* e, uint64_t i, crdt_line_start* starts);
/* The two mappings (above); idx[q] names an index of the encode.  An unknown col_kind is
 * CRDT_E_ARG; mid may be NULL. */
int crdt_pos_to_linecol(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* pos, int col_kind,
                        uint32_t* line, uint32_t* col);
int crdt_linecol_to_pos(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* line, const uint32_t* col,
                        int col_kind, uint32_t* pos, uint8_t* mid);
/* Device-pointer forms (inputs/outputs already in HBM; async on the engine stream).  idx cannot be
 * checked on the host: a query whose idx is out of range or has no result is answered 0xFFFFFFFF
 * (line and col, or pos with mid = 0). */
int crdt_pos_to_linecol_dev_async(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* pos, int col_kind,
                                  uint32_t* line, uint32_t* col);
int crdt_linecol_to_pos_dev_async(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* line,
                                  const uint32_t* col, int col_kind, uint32_t* pos, uint8_t* mid);
int crdt_last_lines_ms(crdt_engine* e, double* ms);   /* HIP events, like crdt_last_diff_ms */

/* ---- find: every occurrence of a literal pattern in the encoded text -----------------------------
 * Searches every index of the last encode result on the device with one pattern: index i of the
 * find result is index i of that encode.
 *
 *  - The text of index i is the text of the last encode: chars items T[0..chars).  Each content
 *    value is sanitised as the encoder sanitises it (a surrogate or a value above 0x10FFFF is
 *    U+FFFD).
 *  - The pattern is given as UTF-32 code points P[0..m), like content, 1 <= m <=
 *    CRDT_FIND_MAX_CHARS, and is sanitised the same way: a pattern value that is no scalar value
 *    matches U+FFFD, and content that was no scalar value is matched by a pattern char U+FFFD.
 *  - fold(c) = c + 0x20 for 0x41 <= c <= 0x5A with CRDT_FIND_ASCII_ICASE, else c.  Nothing outside
 *    ASCII folds (not U+212A, not U+0130, not U+00C9).
 *  - A match at char position p exists iff p + m <= chars and fold(T[p + j]) == fold(P[j]) for all
 *    j < m.  All matches are reported, overlapping ones included ("aa" in "aaaa": 0, 1, 2).  A
 *    match lies wholly inside one document.  An empty document, or one shorter than the pattern,
 *    has 0 matches: that is a result.
 *  - Each match is {unit, pos}: pos = p, unit = the units before char p in that encode (what
 *    crdt_pos_to_units answers for p).  Matches come in ascending order.
 *  - (line, column) of a match: crdt_pos_to_linecol of its pos.  Non-overlapping "replace all"
 *    semantics: filter the sorted list greedily on the host. */
enum { CRDT_FIND_EXACT = 0, CRDT_FIND_ASCII_ICASE = 1 };
#define CRDT_FIND_MAX_CHARS 64
typedef struct { uint32_t unit, pos; } crdt_match;
/* Search, on the device and stream-ordered, every index of the last encode (the call waits once
 * inside, for the total that sizes the match table).  CRDT_E_ARG before any encode result, for
 * n_chars == 0 or above CRDT_FIND_MAX_CHARS, for a NULL pattern and for an unknown flag bit.
 * Replaces the previous find result.  Changes no document, and neither the encode result nor the
 * line index, the diff result, the checkout and the blame result; crdt_lines_async does not touch
 * the find result either.  The find result belongs to the encode result it was built from: a later
 * encode call, successful or not, drops it, and so does crdt_docs_alloc; the reads and seeks below
 * then return CRDT_E_ARG until the next find.  Until then it stays valid whatever is replayed,
 * published or materialised: the seeks read nothing but the match table.
 * CRDT_E_NOMEM if an allocation fails: the engine stays usable, without a find result and with the
 * encode result and the line index intact. */
int crdt_find_async(crdt_engine* e, const uint32_t* pattern, uint32_t n_chars, int flags);
/* Matches per index of that encode (syncs).  An index the encode has no result for has none here:
 * its count is 0xFFFFFFFF, reading its matches returns CRDT_E_ARG, and a host-form seek that names
 * it returns CRDT_E_ARG for the whole call and writes nothing (as does an idx out of range). */
int crdt_find_counts(crdt_engine* e, uint32_t* n_matches);
/* The n_matches[i] matches of index i (matches may be NULL when there are none). */
int crdt_find_read(crdt_engine* e, uint64_t i, crdt_match* matches);
/* Find next / previous from the cursor: k[q] is the number, within index idx[q], of the first match
 * with match.pos >= pos[q] (CRDT_SEEK_NEXT) or of the last match with match.pos <= pos[q]
 * (CRDT_SEEK_PREV); 0xFFFFFFFF when there is none.  pos is not checked against the document's
 * chars: the answer is a function of the match table alone, and wrapping round is the caller's
 * business.  An unknown dir is CRDT_E_ARG. */
enum { CRDT_SEEK_NEXT = 0, CRDT_SEEK_PREV = 1 };
int crdt_find_seek(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* pos, int dir, uint32_t* k);
/* Device-pointer form (inputs/outputs already in HBM; async on the engine stream).  idx cannot be
 * checked on the host: a query whose idx is out of range or has no result is answered 0xFFFFFFFF. */
int crdt_find_seek_dev_async(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* pos, int dir,
                             uint32_t* k);
int crdt_last_find_ms(crdt_engine* e, double* ms);   /* HIP events, like crdt_last_diff_ms */

/* ---- rebase: map positions between a past version and the current text ---------------------------
 * A caller of the diff or the edits holds things that point into the old text (cursors, selections,
 * diagnostics, breakpoints, find matches) and has to move them to where they now stand, or to ask
 * the reverse ("which old offset does this new one come from").  A rebase map is built from the
 * last diff result (CRDT_REBASE_FROM_DIFF) or the last edits result (CRDT_REBASE_FROM_EDITS):
 * index i of the map is index i of that call.
 *
 *  - Take index i's patches P_0 .. P_{m-1} (pos, del_len, ins_len).  The char table has one span
 *    per patch:
 *      new_at[p] = pos[p], new_len[p] = ins_len[p], old_len[p] = del_len[p],
 *      old_at[p] = pos[p] - (sum of ins_len[q], q < p) + (sum of del_len[q], q < p):
 *    where the patch starts in the text at since[i].  (For a result of crdt_diff_between_async
 *    the old side is the text at from[i] and the new side, "the current text" below, the text at
 *    to[i].)
 *  - The units table is the same with unit, del_units, ins_units of the edits.  It exists only for
 *    an edits source, in that call's encoding.
 *  - Spans are ascending on both sides, and neighbouring spans are at least one kept item apart.
 *  - A query is (idx, x, kind, dir, bias).  kind picks the table.  CRDT_REBASE_OLD_TO_NEW reads
 *    each span as (a, la, b, lb) = (old_at, old_len, new_at, new_len); CRDT_REBASE_NEW_TO_OLD swaps
 *    the two sides.  x is a cursor position: the gap before item x of the source side's text.
 *  - Let k be the last span with a[k] <= x.
 *      no such span:   y = x, hit = 0;
 *      x > a + la:     y = x - (a + la) + (b + lb), hit = 0;
 *      otherwise:      y = b if side < 0, else b + lb; hit = 1 iff a < x < a + la.
 *    side = bias (CRDT_BIAS_LEFT: -1, CRDT_BIAS_RIGHT: +1) when la == 0, a pure insertion on the
 *    other side; otherwise -1 at x == a, +1 at x == a + la, and bias strictly inside.  hit == 1
 *    means x was strictly inside a stretch that does not exist on the other side.  (The mapping
 *    rule of ProseMirror's StepMap.map.)
 *  - x is not checked against the length of either text, as crdt_find_seek does not check pos: the
 *    answer is a function of the table alone, in arithmetic modulo 2^32.
 *  - With OLD_TO_NEW, BIAS_RIGHT and x the index of an item visible in both texts: hit == 0 and y
 *    is that item's index in the current text; NEW_TO_OLD with BIAS_RIGHT maps y back to x.  For
 *    fixed dir and bias y is non-decreasing in x, and the left answer is <= the right answer. */
enum { CRDT_REBASE_FROM_DIFF = 0, CRDT_REBASE_FROM_EDITS = 1 };
enum { CRDT_REBASE_CHARS = 0, CRDT_REBASE_UNITS = 1 };
enum { CRDT_REBASE_OLD_TO_NEW = 0, CRDT_REBASE_NEW_TO_OLD = 1 };
enum { CRDT_BIAS_LEFT = 0, CRDT_BIAS_RIGHT = 1 };
typedef struct { uint32_t old_at, old_len, new_at, new_len; } crdt_rebase_span;
/* Build the map on the device, stream-ordered, from the named source.  CRDT_E_ARG for an unknown
 * src and when the source has no valid result.  Replaces the previous map.  The map is a copy: it
 * stays valid whatever is diffed, replayed, published or encoded afterwards, until the next call
 * or crdt_docs_alloc.  Changes no document and none of the other results, and none of their calls
 * touches the map.  No host wait inside: the tables are sized by the source's totals, which the
 * host holds since that call.  CRDT_E_NOMEM if an allocation fails: the engine stays usable,
 * without a map and with the source intact, and the same call then succeeds. */
int crdt_rebase_async(crdt_engine* e, int src);
/* Spans per index of the source call (syncs).  An index the source has no result for has none
 * here: its count is 0xFFFFFFFF, reading it returns CRDT_E_ARG, and a host-form query that names it
 * returns CRDT_E_ARG for the whole call and writes nothing (as does an idx out of range). */
int crdt_rebase_counts(crdt_engine* e, uint32_t* n_spans);
/* The n_spans[i] spans of index i in chars or in units (spans may be NULL when there are none).
 * CRDT_E_ARG for an unknown kind, and for CRDT_REBASE_UNITS on a map built from a diff. */
int crdt_rebase_read(crdt_engine* e, uint64_t i, int kind, crdt_rebase_span* spans);
/* The mapping (above); idx[q] names an index of the map; hit may be NULL.  CRDT_E_ARG for an unknown
 * kind, dir or bias, for CRDT_REBASE_UNITS on a map built from a diff, and before any map.  n == 0
 * is a no-op. */
int crdt_rebase(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* x, int kind, int dir, int bias,
                uint32_t* y, uint8_t* hit);
/* Device-pointer form (inputs/outputs already in HBM; async on the engine stream).  idx cannot be
 * checked on the host: a query whose idx is out of range or has no result is answered 0xFFFFFFFF,
 * with hit = 0. */
int crdt_rebase_dev_async(crdt_engine* e, uint64_t n, const uint32_t* idx, const uint32_t* x, int kind, int dir,
                          int bias, uint32_t* y, uint8_t* hit);
int crdt_last_rebase_ms(crdt_engine* e, double* ms);   /* HIP events, like crdt_last_diff_ms */

/* ListCRDT::len (doc.rs:484-486) */
int crdt_doc_len(crdt_engine* e, uint64_t n, const uint32_t* doc, uint32_t* len);
int crdt_doc_status(crdt_engine* e, int32_t* status /* n_docs */);
/* 64-bit digest of each document's canonical state (DESIGN.md "Digest"; same as the oracle). */
int crdt_digest(crdt_engine* e, uint64_t* per_doc /* n_docs */);
/* Canonical spans of each document's published index (YjsSpan::can_append runs; sizes[2] of
 * crdt_export_sizes for every document at once: the roofline's per-document span counts). */
int crdt_canon_counts(crdt_engine* e, uint32_t* per_doc /* n_docs */);

/* Export one document (parity / debugging).  sizes[12] = {raw entries, leaves, canonical spans,
 * cwo runs, delete runs, double-delete runs, txns, parents, frontier, agents, next_order, len}.
 * Any output pointer may be NULL.  raw/canon: 4 u32 per span (order, origin_left, origin_right,
 * len as i32); cwo: (order, agent, seq, len); deletes/dd: 3 u32; txns: (order, len, shadow,
 * parents_off, n_parents). */
int crdt_export_sizes(crdt_engine* e, uint32_t doc, uint64_t* sizes);
int crdt_export(crdt_engine* e, uint32_t doc, uint32_t* raw4, uint32_t* leaf_sizes, uint32_t* canon4,
                uint32_t* cwo4, uint32_t* del3, uint32_t* dd3, uint32_t* txn5, uint32_t* parents,
                uint32_t* frontier);

// Shrink every document's per-table capacities to what its staged stream used (call after a
// crdt_run + publish of it; a later reset + crdt_run_async replays it in exactly that room).
// Capacities grow again on the next stage.  (Host-side planning; no reference counterpart.)
int crdt_fit(crdt_engine* e);
// crdt_fit over several corpora replayed one after another on the same documents (BASELINE config
// 4's batches): apply = 0 notes the capacities crdt_fit would set into each document's running
// maximum (no relayout); apply = 1 sets every document's capacities to its noted maximum (one
// relayout) and forgets the maxima.  (Host-side planning; no reference counterpart.)
int crdt_fit_note(crdt_engine* e, int apply);
// Config 4 corpus batches: every document whose staged stream is one generated-edit record
// (crdt_stage_random) gets the seed crdt_stage_random would give document id_base + d
// ((u32)splitmix64(seed ^ (id_base + d)); the generator follows make_random_change,
// /root/reference/src/list/doc.rs:544-569).  Device-side, async on the engine stream; the next
// reset + crdt_run_async replays the new documents.
int crdt_reseed_random_async(crdt_engine* e, uint64_t seed, uint64_t id_base);
// crdt_digest into a device buffer (n_docs u64), async on the engine stream: publishes first if
// needed, then computes the digests of the published state (on request, as crdt_digest does).
int crdt_digest_dev_async(crdt_engine* e, uint64_t* dev_out);
// on != 0: documents staged in one call from the same host stream (crdt_stage_local_shared,
// crdt_stage_remote_replicated) read one device copy of it instead of a copy each (records
// are read-only input).  Off by default.
int crdt_set_share_streams(crdt_engine* e, int on);
// on != 0: crdt_stage_remote_replicated interns every document's authors on the device
// (crdt_agent_intern_dev, one wave per document) instead of on the host.  Same ids either way
// (get_or_create_agent_id, doc.rs:66-80).  Off by default.
int crdt_set_device_intern(crdt_engine* e, int on);
/* Kernel family behind crdt_pos_to_loc_dev_async / crdt_loc_to_pos_dev_async (same answers):
 *   CRDT_QUERY_LDS (default): 4,096-query chunks of one document stage its index in LDS and
 *     search in lockstep;
 *   CRDT_QUERY_PER_THREAD: one thread per query, binary searches in HBM;
 *   CRDT_QUERY_MERGE: for batches sorted per document (pos ascending; loc->pos by (agent, seq)):
 *     pos->loc merges each chunk against the document's visible prefix (merge path), loc->pos
 *     searches per thread; unsorted or mixed chunks are answered per thread. */
enum { CRDT_QUERY_LDS = 0, CRDT_QUERY_PER_THREAD = 1, CRDT_QUERY_MERGE = 2 };
int crdt_set_query_kernel(crdt_engine* e, int mode);
// on != 0 (the default; CRDT_NO_FUSED_PUBLISH=1 in the environment makes it off): a replay launched
// onto an index that crdt_fit sized for the staged streams (fit, reset, run, publish: the steady
// loop) has each replay wave publish its own document as it finishes; crdt_publish_async then only
// publishes the documents no wave did.  Same published index, bit for bit, either way.
int crdt_set_fused_publish(crdt_engine* e, int on);
// Test hook: replay launches (crdt_run, crdt_run_async) so far that ran with the fused publish on (launches, may be NULL), and
// per document (per_doc: n_docs bytes, may be NULL; waits for the stream) whether its current index
// was written by its replay wave.
int crdt_fused_publish_stats(crdt_engine* e, uint64_t* launches, uint8_t* per_doc);
/* Progress balance of the replay's waves.  The waves of one SIMD start together, but its issue
 * arbiter favours the oldest, so equal documents end one after the other and the last replay alone.
 * With the balance on, every replay wave sets its own issue priority about once per 64 records,
 * by one of two policies.  Scheduling only: the same state, bit for bit.
 *   rotation: the four priority levels rotate over the SIMD's wave slots in 82 us time slices, so
 *     no wave stays the arbiter's favourite (equal documents then end together; no memory traffic);
 *   board: from the records the wave has left against the other waves resident on its SIMD (most
 *     left = highest priority), through a 1 MiB board the engine owns: also evens out unequal
 *     documents, but gains less on equal ones.
 *   CRDT_BALANCE_AUTO (default): the rotation for a replay launch whose waves are all resident at
 *     once (documents <= 32 x the device's compute units, fewer where the LDS roots limit
 *     residency), nothing for launches that run in several rounds;
 *   CRDT_BALANCE_OFF: never; CRDT_BALANCE_ON / CRDT_BALANCE_ROTATE: the board / the rotation on
 *     every launch (CRDT_REPLAY_BALANCE=0 / 1 / 3 in the environment sets the engine's initial mode).
 * Documents past the LDS root (the two-level root's kernel) are never balanced. */
enum { CRDT_BALANCE_OFF = 0, CRDT_BALANCE_ON = 1, CRDT_BALANCE_AUTO = 2, CRDT_BALANCE_ROTATE = 3 };
int crdt_set_replay_balance(crdt_engine* e, int mode);
/* The rotation's level map: which wave slots of a SIMD hold which of the four levels in a time
 * slice (eight slots share four levels, and the arbiter breaks a tie by age, so what a map chooses
 * is who ties with whom).  0: level = (slice + slot) & 3, slots w and w + 4 tied for the whole
 * launch; 1: pairs of neighbouring slots, a slot tied with its upper and its lower neighbour in
 * turn; 2: groups of one, two and three slots, chosen so that the slots' mean places in the
 * arbiter's order lie closest together (the default: equal documents end closest together and
 * the launch is shortest).  Every map gives every slot each level a quarter of the time.
 * Scheduling only: the same state, bit for bit.  CRDT_BALANCE_MAP=0..2 in the environment sets the
 * engine's initial map; applies from the next replay launch on.  The policy that
 * crdt_debug_balance_board reports is 2 (rotation) whatever the map. */
#define CRDT_BALANCE_MAPS 3
#define CRDT_BALANCE_MAP_DEFAULT 2
int crdt_set_balance_map(crdt_engine* e, int map);
/* Window decode of the replay: a replay wave reads its stream through a 64-record window, and with
 * the decode on it derives, once where the window moves, which compact remote records continue the
 * typing run of the record before them (a lane mask), instead of scanning the window again at
 * every insert.  Two builds of the same kernel, picked per launch: the same state, bit for bit.
 * On by default (CRDT_WINDOW_DECODE=0 / 1 in the environment sets the engine's initial mode);
 * applies to remote-only streams, from the next replay launch on. */
int crdt_set_window_decode(crdt_engine* e, int on);
/* Test hook: the board after the stream has drained (board: CRDT_BALANCE_BOARD_WORDS words, 16 slots
 * per SIMD row, slot = launch stamp << 24 | records left; may be NULL), the stamp of the last replay
 * launch (1..255) and the policy it ran with (0 none, 1 the board, 2 rotation).  After a launch no
 * slot carries a non-zero "records left". */
#define CRDT_BALANCE_BOARD_WORDS (16384u * 16u)
int crdt_debug_balance_board(crdt_engine* e, uint32_t* board, uint32_t* stamp, int* policy);
/* The published index's visible-prefix array of one document (crdt_canon_counts entries: visible
 * items before each canonical span; debugging and tests).  Publishes first if needed. */
int crdt_debug_vpos(crdt_engine* e, uint32_t doc, uint32_t* vpos);
/* What the host planned for each document at the last index sizing: plan[d] = 0 k_publish + k_pub_index,
   1 k_publish building the index in its own wave (bitmap words > the launch's k_pub_index size),
   2 k_publish_big; words[d] = pub_words(ord_cap).  Either pointer may be null (n_docs entries
   otherwise; debugging and tests).  Publishes first if needed; host state only. */
int crdt_debug_publish_plan(crdt_engine* e, uint8_t* plan, uint32_t* words);
// Device bytes the engine holds (per-document pools, staged records, content, text).
uint64_t crdt_mem_bytes(const crdt_engine* e);
// Device bytes the engines of this process hold through their own allocations now, and the most
// they held at once since the last reset (a relayout -- growth, crdt_fit -- moves the pools one
// at a time: its peak is the old pools + the largest new one).  Diagnostic; never fails.
int crdt_device_bytes(uint64_t* current, uint64_t* peak, int reset_peak);
// Test hook: after k more device allocations by any engine of this process, the next one fails as
// out of memory (k < 0: never).  A relayout that fails part-way poisons its engine: every later
// call but crdt_engine_destroy / crdt_docs_alloc returns CRDT_E_NOMEM.
int crdt_test_fail_alloc_after(long long k);
// Test hook: the LDS budget, in 32-bit words, that crdt_diff_vv_async launches its mark kernel with
// (the default and the maximum: 16,384).  A document whose two bitmaps do not fit the budget takes
// the path that builds them in device memory, so a small budget sends small documents there.
int crdt_test_set_vv_lds_words(uint32_t words);
// Config 1's per-op check: after txn t (of every listed document), ask pos_to_loc(probes[t].pos)
// and loc_to_pos(probes[t].agent, probes[t].seq) on the state reached so far (the README's two
// mappings, cursor.rs:147-190 count_pos; answers as crdt_pos_to_loc / crdt_loc_to_pos).
// Otherwise as crdt_apply_local.  The probed documents keep the order -> leaf map.
typedef struct { uint32_t pos, agent, seq; } crdt_probe;
typedef struct { uint32_t agent, seq, pos, deleted; } crdt_probe_answer;
int crdt_apply_local_probed(crdt_engine* e, uint64_t n_docs, const uint32_t* docs, const uint64_t* txn_off,
                            const crdt_local_txn* txns, const crdt_local_op* ops, const crdt_probe* probes,
                            crdt_probe_answer* answers, int32_t* doc_status);
/* Raw per-document replay state (23 u32: status, resume point, table sizes, ...; debugging). */
int crdt_debug_state(crdt_engine* e, uint32_t doc, uint32_t* out23);
/* Device time of the last replay / publish launches in ms (HIP events on the engine stream). */
int crdt_last_timings(crdt_engine* e, double* replay_ms, double* publish_ms);
/* Engine stream (hipStream_t) for callers that time or order their own work. */
void* crdt_stream(crdt_engine* e);
/* Text of the last HIP error seen by this thread (empty if none). */
const char* crdt_last_error(void);
/* The source hash this library was built from (crdt_amd.build(): sha256 over the sources and the
 * build line, also stored beside the library), so a run can prove which sources it executed. */
const char* crdt_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* CRDT_GPU_H */
