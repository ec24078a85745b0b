/*
 * crdtgpu.h -- C ABI of the MI355X batched AWSet merge engine.
 *
 * The reference (rsms/go-crdt-playground, package crdt) has no FFI: its merge
 * path is a Go method set called in-process.  Each entry point below replaces
 * one of those methods, applied to a whole batch of independent documents at
 * once; a cgo package with the reference's types calls them.
 *
 *   crdt_awset_join_async / crdt_awset_join_batch
 *       replace (*AWSet).Merge / merge                 awset.go:103-161
 *   crdt_awset_fold_async / crdt_awset_fold_batch, mode CRDT_FOLD_AWSET
 *       replace an ordered sequence of (*AWSet).Merge  awset.go:103-161
 *   crdt_awset_fold_async / crdt_awset_fold_batch, mode CRDT_FOLD_DELTA
 *       replace (*AWSetDelta).Merge with MakeDeltaMergeData, deltaMerge and
 *       the (no-op) gcDeleted                          awset-delta_test.go:51-166
 *   crdt_awset_delta_extract_async / crdt_awset_delta_extract_batch
 *       replace (*AWSetDelta).MakeDeltaMergeData and the path select of
 *       (*AWSetDelta).Merge, run on the sending side against the clock the
 *       peer is known to have reached          awset-delta_test.go:51-65,79-105
 *   crdt_vv_max_async
 *       replaces (*VersionVector).Merge                crdt-misc.go:43-55
 *   crdt_causal_context_async
 *       the elementwise max over many version vectors (no reference
 *       counterpart: the per-GPU summary reduced across GPUs by RCCL)
 *   crdt_awset_apply_async / crdt_awset_apply_batch
 *       replace the state producers (*AWSet).Add / Del  awset.go:89-101
 *       and (*AWSetDelta).Del                          awset-delta_test.go:14-33
 *       applied as ordered op lists to a batch of documents
 *   crdt_awset_has_async / crdt_awset_has_batch
 *       replace (*AWSet).Has                           awset.go:87
 *       for per-document lists of query keys, with the entry's dot;
 *       crdt_tomb_has_async is the same lookup over AWSetDelta.Deleted
 *   crdt_awset_compare_async / crdt_awset_compare_batch
 *       replace the tests' assertEntries(A, ..) / assertEntries(B, ..): per
 *       document, do the two replicas hold the same elements, dots and clock;
 *       with the ascending list of the documents that still differ
 *   crdt_awset_digest_async / crdt_awset_digest_host / crdt_digest_diff_async
 *       the same question across GPUs or hosts: a 16-byte hash of each
 *       document's live state, and the comparison of two such arrays (no
 *       reference counterpart: its replicas meet in one process)
 *   crdt_awset_digest_idx_async
 *       the digests of the documents a worklist names, written into a
 *       resident digest array at their own positions (no reference counterpart)
 *   crdt_digest_tree_async / crdt_digest_tree_host / crdt_digest_tree_children_async /
 *   crdt_digest_tree_diff_async
 *       a hash tree over a digest array and the two sides of a level-by-level
 *       descent: which documents differ, from a few kilobytes instead of the
 *       whole array (no reference counterpart)
 *   crdt_awset_select_async
 *       those documents (or all of them: compaction) gathered into a packed
 *       batch for the next round (no reference counterpart)
 *   crdt_awset_scatter_async
 *       the merged sub-batch written back into the batch it was selected
 *       from: select's inverse (no reference counterpart)
 *   crdt_awset_diff_async / crdt_awset_diff_batch
 *       replace merge's decision log (update / add / remove per key,
 *       awset.go:109-158) in structured form: per document, the entries a
 *       merge removed and the entries it added or moved to another dot
 *   crdt_awset_join_log_async / crdt_awset_exchange_log_async
 *       the join and the exchange with that log written beside the merged
 *       state, from the one read the merge needs   awset.go:103-161
 *   crdt_awset_fold_log_async
 *       the fold, in either mode, with the log of its net effect: what the
 *       receiver of a delta message and an N-way merge report to an index
 *   crdt_awset_apply_log_async
 *       the local ops with the same log: what Add / Del / (*AWSetDelta).Del
 *       removed, added or moved to a new dot       awset.go:89-101
 *   crdt_awset_sources_async
 *       P resident replicas of every document gathered into the packed source
 *       batch the folds and the delta extraction read (no reference
 *       counterpart: the reference folds replicas it holds as Go values)
 *   crdt_awset_delta_join_async / crdt_awset_delta_exchange_async
 *       replace (*AWSetDelta).Merge, and the pair A.Merge(B); B.Merge(A) of
 *       the reference's own test, on resident replicas as they stand
 *                                      awset-delta_test.go:51-166, 173-174
 *   crdt_replica_select_async / crdt_replica_scatter_async
 *       select and scatter over a whole replica: the documents move with
 *       their Deleted tombstones and actors, which is what a sparse delta
 *       round and a sparse apply need (no reference counterpart)
 *   crdt_replica_scatter_inplace_async
 *       replaces crdt_replica_scatter_async in those rounds: a merged document
 *       is written into the slots its document already owns when it fits, and
 *       named in a spill list otherwise (no reference counterpart)
 *   crdt_replica_repack_async / crdt_headroom_capacity
 *       the same select or scatter writing a layout with spare slots per
 *       document, so that the in-place scatter finds room (no reference
 *       counterpart)
 *   crdt_global_context_allreduce / crdt_context_allreduce_async
 *       that summary combined across GPUs: RCCL all-reduce(max, u64)
 *       (the reference's counterpart is the CPU max over
 *       every merged VersionVector, crdt-misc.go:43-55)
 *
 * HasDot (crdt-misc.go:28-34) and Counter (:36-41) run inside the kernels.
 *
 * Encoding (SoA, all little-endian):
 *   entry  = key id u64 + dot actor u32 + dot counter u64   (20 B)
 *   VV     = R x u64 per state, R identical for every state of a call
 *   doc d of a batch owns the slots [offsets[d], offsets[d+1]); its live
 *   entries are the first counts[d] of them (counts == NULL: all slots live),
 *   keys strictly ascending.  Strings are interned to key ids by the caller.
 *
 * HasDot / Counter with actor == R index one past the reference's slice and
 * panic in Go; here the call returns CRDT_E_ACTOR_RANGE instead (outputs then
 * undefined).  actor > R is "never seen" (false / 0), as in the reference.
 *
 * Output: doc d of a join is written at out offset dst.offsets[d] +
 * src.offsets[d] (capacity = both inputs' capacities), its live count to
 * out->counts[d], its slot bounds to out->offsets[d] (n_docs+1 values) and its
 * VV to out->vv.  Entries come out sorted by key.  No scan over documents is
 * needed, so one launch finishes the batch, and the output is directly a valid
 * input batch for the next merge.  A document's slots past its live count
 * (counts[d] .. its capacity) are unspecified and may be written (the joins'
 * whole-sector stores pad them with zeros); slots of other documents never are.
 *
 * Threading: one crdt_ctx per host thread; *_async calls are ordered on the
 * given HIP stream; crdt_ctx_sync returns device-side errors.  Device buffers
 * passed to *_async are caller-owned (device-resident, e.g. torch tensors).
 * The *_batch calls take host buffers and are synchronous.
 *
 * Streams and graphs: the calls of one context share its workspace (worklist,
 * counters, fold scratch, status word).  A call issued on a different stream
 * than the previous call of the same context first waits (hipStreamWaitEvent)
 * for that call's launches, so calls of one context never overlap on the
 * device, whatever streams they use; crdt_ctx_sync also waits for them.  A
 * call made while its stream is capturing a HIP graph records no such wait
 * (the capture is ordered by its caller) and never allocates: if the
 * workspace would have to grow it returns CRDT_E_WORKSPACE (reserve first,
 * or run the call once eagerly).  Buffers the workspace outgrows are kept
 * until crdt_ctx_destroy, so graphs captured earlier stay valid.
 */
#ifndef CRDTGPU_H
#define CRDTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRDTGPU_ABI_VERSION 1

/* status codes */
#define CRDT_OK 0
#define CRDT_E_INVALID (-1)     /* null pointer, R==0 or R>CRDT_MAX_R, bad sizes       */
#define CRDT_E_ACTOR_RANGE (-2) /* HasDot/Counter at actor == R: reference panics     */
#define CRDT_E_UNSORTED (-3)    /* keys of a doc not strictly ascending (validation)  */
#define CRDT_E_CAPACITY (-4)    /* a doc's live count exceeds its slots               */
#define CRDT_E_HIP (-5)         /* HIP runtime error                                   */
#define CRDT_E_NOMEM (-6)       /* device allocation failed                            */
#define CRDT_E_WORKSPACE (-7)   /* fold block path needs crdt_ctx_reserve(max_fold_slots) */
#define CRDT_E_RCCL (-8)        /* RCCL not loadable, or a collective failed          */
#define CRDT_E_DUP_KEY (-9)     /* a key appears twice in one document (ingest sort)  */

#define CRDT_MAX_R 64 /* version-vector length limit (one wave lane per actor) */

/* fold modes */
#define CRDT_FOLD_AWSET 0 /* each step = (*AWSet).Merge: tombstones ignored       */
#define CRDT_FOLD_DELTA 1 /* each step = (*AWSetDelta).Merge                       */

typedef struct crdt_ctx crdt_ctx;

/* A batch of AWSet states (read-only view). */
typedef struct {
    uint32_t n_docs;
    uint32_t R;
    const uint32_t* offsets;  /* [n_docs+1] slot bounds                          */
    const uint32_t* counts;   /* [n_docs] live entries, or NULL = all slots live */
    const uint64_t* keys;     /* [offsets[n_docs]]                              */
    const uint32_t* actors;   /* [offsets[n_docs]]                              */
    const uint64_t* counters; /* [offsets[n_docs]]                              */
    const uint64_t* vv;       /* [n_docs*R]                                     */
} crdt_awset_batch;

/* Output of a join or fold (written). */
typedef struct {
    uint32_t* offsets;  /* [n_docs+1]                          */
    uint32_t* counts;   /* [n_docs]                            */
    uint64_t* keys;     /* capacity = Σ input slots            */
    uint32_t* actors;
    uint64_t* counters;
    uint64_t* vv;       /* [n_docs*R]                          */
} crdt_awset_out;

/*
 * Ordered source states folded into each dst doc (AWSet or AWSetDelta
 * states).  Doc d receives sources [doc_srcs[d], doc_srcs[d+1]) in that order.
 * Source s: replica actor src_actor[s] (AWSetDelta.Actor, read by the path
 * select of awset-delta_test.go:53), VV vv[s*R..], entries
 * [entry_off[s], entry_off[s+1]) and tombstones (AWSetDelta.Deleted)
 * [tomb_off[s], tomb_off[s+1]), each sorted by key.  tomb_off may be NULL.
 * Fold output capacity of doc d: dst slots + Σ its sources' entry slots, at
 * offset dst.offsets[d] + entry_off[doc_srcs[d]].
 */
typedef struct {
    uint32_t n_docs;
    uint32_t R;
    const uint32_t* doc_srcs;   /* [n_docs+1]  */
    const uint32_t* src_actor;  /* [n_srcs]    */
    const uint64_t* vv;         /* [n_srcs*R]  */
    const uint32_t* entry_off;  /* [n_srcs+1]  */
    const uint64_t* keys;
    const uint32_t* actors;
    const uint64_t* counters;
    const uint32_t* tomb_off;   /* [n_srcs+1] or NULL */
    const uint64_t* tkeys;
    const uint32_t* tactors;
    const uint64_t* tcounters;
} crdt_src_batch;

/* ---- context ---------------------------------------------------------- */
int crdt_ctx_create(int device, crdt_ctx** out);
void crdt_ctx_destroy(crdt_ctx* ctx);
/* Pre-size workspaces so that *_async calls never allocate (graph capture). */
int crdt_ctx_reserve(crdt_ctx* ctx, uint32_t max_docs, uint64_t max_fold_slots);
/* Promise that every doc of later joins holds <= max_entries live entries per
 * side (0xFFFFFFFF = no promise, the default).  At <= 64 the large-document
 * path is not launched; a doc that breaks the promise makes crdt_ctx_sync
 * return CRDT_E_INVALID. */
int crdt_ctx_set_max_doc_entries(crdt_ctx* ctx, uint32_t max_entries);
/* Tuning knobs (performance only, never results):
 *   "join_docs_per_wave"  1|2|4|8|16  documents one wavefront pipelines (default 8)
 *   "join_nt_stores"      0|1         non-temporal output stores (default 1)
 *   "probe_blocks_per_cu" 1..64       crdt_bw_probe grid (default 16)
 *   "probe_slab"          0|1         crdt_bw_probe: one contiguous slab per workgroup
 *                                     instead of a grid-stride sweep (default 0)
 *   "join_stage_stores"   0|1         survivors staged in LDS, whole-line stores (default 1)
 *   "join_slab_blocks_per_cu" 0..64   wave kernel block order: slabs of G = this x CUs
 *                                     blocks (crdt_device.hpp SlabMap; 0 = in order)
 *   "fold_lean_first"     0|1         folds: slot-walk pass first, the rest deferred (default 1)
 *   "digest_tree_fuse"    0|1         digest tree: the levels of 4,096 children and fewer in
 *                                     one workgroup's launch (default 1)
 *   "join_tile_capacity"  1..2^28     large documents: merge-path tiles of 1,024 merged
 *                                     positions per pass (default 2^22, 56 B each,
 *                                     allocated on first use); a call with more tiles runs
 *                                     in passes of this many, a pass may end inside a
 *                                     document
 *   "join_tile_max_passes" 1..65536   passes launched at most (default 256): a call with
 *                                     more tiles than this x capacity takes the
 *                                     per-document block kernel instead
 *   "join_tile_dispensers" 1|8        tile dispenser words (default 8, one per XCD)
 *   (also "join_tile_shape", "join_tile_nt_stores", "join_tile_split_blocks_per_cu",
 *   "join_tiles": see api.cpp)
 * and one layout option of the host-buffer (*_batch) joins, exchanges and folds:
 *   "pack_batch_outputs"  0|1         1: out holds only the live entries, doc d
 *                                     at offsets[d] = counts[0] + .. + counts[d-1]
 *                                     (less to download; the offsets are computed on the
 *                                     device, and outputs in crdt_host_alloc memory are
 *                                     written there by the device, no copy call); 0
 *                                     (default): at its capacity offset, as the *_async
 *                                     calls write.
 *   "span_staging"        0|1         inputs lying in one crdt_host_alloc block go up as
 *                                     one copy of the span they cover (default 1)
 * The *_batch calls check the slot layout on the host and the key order on the
 * device after the upload; a batch out of order reaches no merge kernel (the
 * merge's first kernel reads the check's verdict on the device) and the call
 * returns CRDT_E_UNSORTED with the outputs unspecified; crdt_validate_batch
 * checks everything on the host. */
int crdt_ctx_set_option(crdt_ctx* ctx, const char* name, int64_t value);
/* Wait for `stream`, return (and clear) the first device-side error. */
int crdt_ctx_sync(crdt_ctx* ctx, void* stream);
const char* crdt_strerror(int code);
int crdt_abi_version(void);

/* ---- device-resident, asynchronous on a HIP stream (NULL = default) ----
 * Join and exchange: a live count above a document's slots is clamped to them
 * and crdt_ctx_sync returns CRDT_E_CAPACITY; the document is then the join of
 * the clamped prefixes, every other document is what it would be without the
 * bad count, and no slot of another document is read as live or written. */
int crdt_awset_join_async(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_awset_batch* src,
                          const crdt_awset_out* out, void* stream);
/* Anti-entropy exchange: out_ab[d] = a[d] <- b[d] AND out_ba[d] = b[d] <- a[d]
 * (two (*AWSet).Merge calls per doc, awset.go:103-161) from ONE read of both
 * states.  Both directions keep the same keys at the same slots; only a
 * common key's dot differs (the src dot wins, awset.go:142).  So the two
 * outputs may share one key column: out_ba->keys == out_ab->keys is allowed
 * and writes the keys once; every other output array must be distinct and
 * must not overlap another (CRDT_E_INVALID when two arrays start at the same
 * address or the per-document arrays overlap; a partial overlap of the entry
 * arrays, whose capacity is in device memory, is undefined behaviour).
 * (crdt_awset_exchange_batch: the same for host outputs -- the shared column
 * is also downloaded once.) */
int crdt_awset_exchange_async(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b,
                              const crdt_awset_out* out_ab, const crdt_awset_out* out_ba, void* stream);
int crdt_awset_fold_async(crdt_ctx* ctx, int mode, const crdt_awset_batch* dst, const crdt_src_batch* srcs,
                          const crdt_awset_out* out, void* stream);
/* ---- delta extraction: the sending side of anti-entropy -------------------
 * Given AWSetDelta source states and, per doc, the clock peer_vv[d*R..] the
 * peer's replica of that doc is known to have reached (shared by the doc's
 * sources), write the message to ship: a packed crdt_src_batch with the same
 * n_docs, R and doc_srcs, src_actor and vv copied, and per source s of doc d,
 * P = peer_vv[d*R..]:
 *   tombstones = {(k,x) in Deleted : not (k in Entries and (e.actor != x.actor
 *                or e.counter > x.counter))}   awset-delta_test.go:93-102; no
 *                clock filter, the same for every kind
 *   CRDT_DELTA_FULL   P.Counter(src_actor[s]) == 0 (first contact, :53): every
 *                     entry; stays FULL when the state is empty
 *   CRDT_DELTA_DELTA  otherwise: entries {(k,e) : !P.HasDot(e)}         :84-92
 *   CRDT_DELTA_NONE   a DELTA with no entry and no tombstone to send (:60); the
 *                     source keeps its (empty) slot in the message
 * Entries and tombstones come out in key order; entry_off / tomb_off are the
 * exclusive prefix sums over all sources (no slack), so entry_off[n_srcs] and
 * tomb_off[n_srcs] are the totals shipped.  The message is a valid `srcs` of
 * crdt_awset_fold_* in CRDT_FOLD_DELTA mode, and for any peer_vv <= the
 * receiver's clock (elementwise; clocks only grow) folding it gives what
 * folding the full states gives: the receiver prunes again, and a FULL source
 * carries its tombstones in case the receiver has met that actor since.
 * Counter(src_actor) at src_actor == R, and on the DELTA path HasDot of an
 * entry dot with actor == R: CRDT_E_ACTOR_RANGE at sync (entry dots of a FULL
 * source and tombstone dots are not tested).  Output capacity: the input's
 * entry and tombstone slots.  srcs->tomb_off == NULL: no tombstones; out may
 * then pass NULL tombstone arrays, and a tomb_off it does pass is zeroed.
 * Workspace: two words per doc, sized by crdt_ctx_reserve(max_docs, ..). */
#define CRDT_DELTA_NONE 0
#define CRDT_DELTA_DELTA 1
#define CRDT_DELTA_FULL 2
typedef struct {            /* written; same layout as crdt_src_batch plus kind */
    uint32_t* doc_srcs;     /* [n_docs+1]  */
    uint32_t* src_actor;    /* [n_srcs]    */
    uint64_t* vv;           /* [n_srcs*R]  */
    uint32_t* entry_off;    /* [n_srcs+1]  */
    uint64_t* keys;
    uint32_t* actors;
    uint64_t* counters;
    uint32_t* tomb_off;     /* [n_srcs+1]  */
    uint64_t* tkeys;
    uint32_t* tactors;
    uint64_t* tcounters;
    uint8_t* kind;          /* [n_srcs] CRDT_DELTA_*, may be NULL */
} crdt_delta_out;
int crdt_awset_delta_extract_async(crdt_ctx* ctx, const crdt_src_batch* srcs, const uint64_t* peer_vv,
                                   const crdt_delta_out* out, void* stream);

/* dst[i] = max(dst[i], src[i]) for i < n (u64). */
int crdt_vv_max_async(crdt_ctx* ctx, uint64_t* dst, const uint64_t* src, size_t n, void* stream);
/* out[r] = max over d < n_docs of vv[d*R + r]  (the per-GPU causal-context summary). */
int crdt_causal_context_async(crdt_ctx* ctx, const uint64_t* vv, uint32_t n_docs, uint32_t R, uint64_t* out,
                              void* stream);

/* ---- synthetic workloads (bench / GPU tests; not part of a merge) ----------
 * "pair" (BASELINE config 2): n_docs documents x 2 replicas (A actor 0, B
 * actor 1), R = 2, 64 live entries each in 64 slots per doc; reachable states
 * (formulas: go-crdt-playground_amd/csrc/gen.hip).  a/b need n_docs*64 slots. */
int crdt_gen_pair_async(crdt_ctx* ctx, uint64_t seed, uint32_t n_docs, const crdt_awset_out* a,
                        const crdt_awset_out* b, void* stream);
/* "delta" (BASELINE config 3): n_docs dst docs x 64 entries (64 slots each),
 * R actors, n_srcs_per_doc ordered AWSetDelta sources per doc of 8 entries and
 * 2 tombstones.  Writes through srcs' pointers (all must be allocated:
 * n_docs*M sources, 8 and 2 slots each).  Formulas: csrc/gen.hip. */
int crdt_gen_delta_async(crdt_ctx* ctx, uint64_t seed, uint32_t n_docs, uint32_t R, uint32_t n_srcs_per_doc,
                         const crdt_awset_out* dst, const crdt_src_batch* srcs, void* stream);
/* "replicas" (BASELINE config 5): per doc `replicas` AWSet states of `entries`
 * entries (a power of two <= 32), R = replicas; dst = replica 0 (entries slots
 * per doc), srcs = replicas 1.. in order (entries slots each, 0 tombstones;
 * tomb_off must be allocated).  Fold with CRDT_FOLD_AWSET. */
/* "zipf" (BASELINE config 4): n_docs (< 2^24) docs, sizes from
 * crdt_gen_zipf_sizes (host, no GPU), A/B replicas with 50% concurrent
 * add/remove conflicts, R = 2.  offsets: device array [n_docs+1], the prefix
 * sum of the sizes (each side gets `size` slots per doc).  Formulas: gen.hip. */
int crdt_gen_zipf_sizes(uint64_t seed, uint32_t n_docs, uint32_t* sizes);
int crdt_gen_zipf_async(crdt_ctx* ctx, uint64_t seed, uint32_t n_docs, const uint32_t* offsets,
                        const crdt_awset_out* a, const crdt_awset_out* b, void* stream);
int crdt_gen_replicas_async(crdt_ctx* ctx, uint64_t seed, uint32_t n_docs, uint32_t replicas, uint32_t entries,
                            const crdt_awset_out* dst, const crdt_src_batch* srcs, void* stream);

/* ---- box bandwidth probes (not a merge; bench.py's roofline context) ------
 * Times `reps` launches of a streaming kernel over caller-owned device memory
 * on the context's stream (after one untimed launch) and returns the HBM rate
 * in GB/s (1e9 B/s): READ reads `bytes` of a (16 B per lane, four loads in
 * flight), WRITE writes `bytes` to b (16 B non-temporal stores; _PLAIN: plain
 * stores), COPY reads a and writes b (counts 2 x bytes).  READ needs b as a
 * 4-byte sink.  Grid: crdt_ctx_set_option("probe_blocks_per_cu", 1..64,
 * default 16) workgroups of 256 per CU.  Use buffers well above the 256 MiB
 * Infinity Cache.  Synchronous. */
#define CRDT_PROBE_READ 0
#define CRDT_PROBE_WRITE 1
#define CRDT_PROBE_COPY 2
#define CRDT_PROBE_WRITE_PLAIN 3
#define CRDT_PROBE_COPY_PLAIN 4
#define CRDT_PROBE_MIX 5       /* 3 reads : 4 writes of 16 B (the exchange's mix), nt stores; GB/s = all 7 */
#define CRDT_PROBE_MIX_PLAIN 6 /* the same, plain stores */
int crdt_bw_probe(crdt_ctx* ctx, int kind, const void* a, void* b, size_t bytes, int reps, double* gbs);
/* The shader clock (MHz) while every CU runs dependent integer chains:
 * shader-cycle counter over the fixed-rate wall clock on one wave.  Kernels
 * bound by instruction issue scale with it; streaming ones do not. */
int crdt_clock_probe(crdt_ctx* ctx, double* mhz);

/* ---- batched local operations: the state producers -----
 * Each document receives an ordered op list, applied to its replica state
 * (AWSet entries + VV, and for AWSetDelta its Deleted tombstones) as the
 * reference's calls would be, in order:
 *   CRDT_OP_ADD            (*AWSet).Add(k)            awset.go:89-94
 *                          vv[actor]++; entries[k] = {actor, vv[actor]}
 *   CRDT_OP_DEL            (*AWSet).Del(k)            awset.go:96-101
 *                          delete(entries, k); no clock bump
 *   CRDT_OP_DELTA_DEL      starts one (*AWSetDelta).Del(k...) call,
 *                          awset-delta_test.go:14-33: vv[actor]++ once
 *   CRDT_OP_DELTA_DEL_KEY  one key of that call (must follow the
 *                          DELTA_DEL or another DELTA_DEL_KEY): if k is in
 *                          entries, Deleted[k] = {actor, vv[actor]} and the
 *                          entry is deleted; otherwise nothing
 * Add(k1, k2) / Del(k1, k2) are one op per key in order.  `keys` of
 * CRDT_OP_DELTA_DEL ops are ignored.  The doc's replica actor is doc_actor[d];
 * an op that bumps the clock with actor >= R is Go's index-out-of-range panic:
 * CRDT_E_ACTOR_RANGE.  At most CRDT_MAX_OPS_PER_DOC ops per doc per call
 * (longer lists: successive calls); malformed lists: CRDT_E_INVALID.
 * Outputs: doc d's entries at out offset state.offsets[d] + op_off[d]
 * (capacity = state slots + ops), its tombstones at tombs.offsets[d] +
 * op_off[d] (tombs NULL: no Deleted yet, offsets 0); tomb_out may be NULL when
 * no DELTA_DEL_KEY op occurs.  Offsets/counts are written for every doc. */
#define CRDT_OP_ADD 0
#define CRDT_OP_DEL 1
#define CRDT_OP_DELTA_DEL 2
#define CRDT_OP_DELTA_DEL_KEY 3
#define CRDT_MAX_OPS_PER_DOC 256

typedef struct {
    uint32_t n_docs;
    const uint32_t* op_off;    /* [n_docs+1]  */
    const uint8_t* kind;       /* [n_ops]     */
    const uint64_t* keys;      /* [n_ops]     */
    const uint32_t* doc_actor; /* [n_docs]  AWSet.Actor of each doc's replica */
} crdt_op_batch;

/* AWSetDelta.Deleted of each doc of a batch (sorted by key). */
typedef struct {
    const uint32_t* offsets;  /* [n_docs+1] */
    const uint32_t* counts;   /* [n_docs] or NULL */
    const uint64_t* keys;
    const uint32_t* actors;
    const uint64_t* counters;
} crdt_tomb_batch;

typedef struct {
    uint32_t* offsets;  /* [n_docs+1] */
    uint32_t* counts;   /* [n_docs]   */
    uint64_t* keys;
    uint32_t* actors;
    uint64_t* counters;
} crdt_tomb_out;

int crdt_awset_apply_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_tomb_batch* tombs,
                           const crdt_op_batch* ops, const crdt_awset_out* out, const crdt_tomb_out* tomb_out,
                           void* stream);
int crdt_awset_apply_batch(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_tomb_batch* tombs,
                           const crdt_op_batch* ops, const crdt_awset_out* out, const crdt_tomb_out* tomb_out);

/* ---- membership reads: (*AWSet).Has on device-resident states -------------
 * Doc d asks the keys q->keys[q_off[d] .. q_off[d+1]).  Per query i of doc d:
 * found[i] = 1 iff the key equals one of the first counts[d] keys of the doc's
 * slots (all slots when counts == NULL), awset.go:87; actors[i] / counters[i] =
 * that entry's dot.  Slots past the live count are never matched, whatever
 * they hold (the joins pad them with zeros).  For an absent key found, actors
 * and counters are all 0, so every output word is written.  The VV is not read
 * (R is validated as elsewhere), so a join, exchange, fold or apply output
 * (crdt_awset_out with its offsets and counts) is a valid `state` as it
 * stands.  crdt_tomb_has_async: the same lookup over AWSetDelta.Deleted, "was
 * k deleted, and by which dot".
 * _async: one kernel launch, no workspace, no allocation, no host sync
 * (capturable on an unreserved context), ordered after the context's previous
 * call; n_queries == 0 launches nothing.  A live count above the doc's slots
 * is clamped to them and crdt_ctx_sync returns CRDT_E_CAPACITY.
 * CRDT_E_INVALID: NULL state, q, out, q_off or found, keys NULL with
 * n_queries > 0, q->n_docs != the state's, exactly one of actors / counters
 * NULL.
 * _batch (host arrays; for tests and small callers -- a host caller that holds
 * host maps looks its keys up there and has no use for it): checks q_off
 * (q_off[0] == 0, monotone, q_off[n_docs] == n_queries: CRDT_E_INVALID) and the
 * slot layout and counts (CRDT_E_CAPACITY) on the host, the key order on the
 * device after the upload (CRDT_E_UNSORTED, no lookup runs), and downloads the
 * outputs. */
typedef struct {            /* per-document query lists (read-only) */
    uint32_t n_docs;        /* must equal the state's n_docs */
    uint32_t n_queries;     /* == q_off[n_docs]; host-known, as n_slots is for the ingest sort */
    const uint32_t* q_off;  /* [n_docs+1] doc d asks keys[q_off[d] .. q_off[d+1]) */
    const uint64_t* keys;   /* [n_queries] any order within a doc, duplicates allowed */
} crdt_query_batch;
typedef struct {            /* written, one per query, in query order */
    uint8_t*  found;        /* [n_queries] 1 = key is a live entry of its doc, else 0 */
    uint32_t* actors;       /* [n_queries] the entry's dot, 0 when absent; may be NULL */
    uint64_t* counters;     /* [n_queries] likewise; may be NULL (both or neither) */
} crdt_query_out;
int crdt_awset_has_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_query_batch* q,
                         const crdt_query_out* out, void* stream);
int crdt_awset_has_batch(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_query_batch* q,
                         const crdt_query_out* out);
int crdt_tomb_has_async(crdt_ctx* ctx, const crdt_tomb_batch* tombs, uint32_t n_docs,
                        const crdt_query_batch* q, const crdt_query_out* out, void* stream);

/* ---- convergence check: have two replicas converged, and where not --------
 * The reference's tests end on assertEntries(A, ..) / assertEntries(B, ..), a
 * comparison of the two replicas' sorted values; crdt_awset_compare_* asks it
 * of every document of two batches at once.  Comparing clocks is not enough:
 * (*AWSet).Del does not bump the version vector (awset.go:97), so two replicas
 * with equal clocks can hold different entries -- the entries are compared.
 *   - Only the live prefix of each document is read: its first counts[d] slots
 *     (all slots when counts == NULL).  Slack is never read, whatever it holds.
 *   - Keys are strictly ascending, so the element sets are equal iff the live
 *     counts are equal and the keys are equal position by position.
 *   - CRDT_CMP_KEYS is set iff the element sets are not equal.
 *   - CRDT_CMP_DOTS is set iff KEYS is clear and some position's (actor,
 *     counter) differs; it is 0 whenever KEYS is set (not evaluated then; a
 *     document whose live counts differ has none of its entries read).
 *   - CRDT_CMP_A_AHEAD / CRDT_CMP_B_AHEAD come from the R clock words alone.
 *     flags[d] == 0: live state and VV bit-identical.
 *   - a and b must agree in n_docs and R; their slot layouts are independent.
 *   - worklist: the ids of the documents with flags & mask != 0, ascending, the
 *     same on every run (count / scan / emit, no atomic append); words at or past
 *     *n_work are not written.  summary counts are exact.  mask == 0: an empty
 *     worklist.
 *   - A live count above a document's slots is clamped to them and
 *     crdt_ctx_sync returns CRDT_E_CAPACITY, as in crdt_awset_has_async.
 *   - CRDT_E_INVALID: NULL a, b, out or flags; n_docs or R mismatch; R out of
 *     range; exactly one of worklist / n_work NULL; mask bits above 15.
 *   - n_docs == 0: nothing that reads documents is launched; summary and n_work
 *     are still written (zeros).
 * _async: no host sync, and no allocation on a reserved context: its workspace
 * is one word per document, sized by crdt_ctx_reserve(max_docs, ..)
 * (CRDT_E_WORKSPACE when it would have to grow during a graph capture).
 * Capturable; ordered after the context's previous call like every entry point.
 * After an exchange both outputs hold the same keys, so comparing them leaves
 * KEYS clear everywhere and only DOTS (a common key under two dots) can remain.
 * _batch (host arrays; for tests and small callers -- a host caller that holds
 * host maps compares them there): checks the slot layouts and counts on the
 * host (CRDT_E_INVALID / CRDT_E_CAPACITY), the key order on the device after the
 * upload (CRDT_E_UNSORTED, no compare runs), and downloads flags, summary,
 * n_work and the first *n_work worklist words. */
#define CRDT_CMP_KEYS    1u /* the element sets differ (what assertEntries tests)            */
#define CRDT_CMP_DOTS    2u /* same elements, at least one under a different dot             */
#define CRDT_CMP_A_AHEAD 4u /* a.vv[r] > b.vv[r] for some r < R                              */
#define CRDT_CMP_B_AHEAD 8u /* b.vv[r] > a.vv[r] for some r < R                              */
typedef struct {          /* written */
    uint8_t*  flags;      /* [n_docs] OR of CRDT_CMP_* for doc d; 0 = live state and VV bit-identical */
    uint32_t* summary;    /* [5] docs with KEYS, DOTS, A_AHEAD, B_AHEAD set, and docs with
                             flags & mask != 0; may be NULL */
    uint32_t* worklist;   /* [n_docs] ascending ids of docs with flags & mask != 0; may be NULL */
    uint32_t* n_work;     /* [1] entries of worklist; NULL iff worklist is NULL */
} crdt_compare_out;
int crdt_awset_compare_async(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b, uint32_t mask,
                             const crdt_compare_out* out, void* stream);
int crdt_awset_compare_batch(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b, uint32_t mask,
                             const crdt_compare_out* out);

/* ---- state digests: which documents differ from a peer's copy elsewhere -----
 * crdt_awset_compare_* needs both replicas on one device.  Between GPUs or
 * hosts a peer ships 16 B per document instead of its states: a digest of the
 * live state, diffed against the local one; the resulting worklist feeds
 * select, sources, the delta extraction and the folds.  Clocks cannot stand in
 * for it: (*AWSet).Del does not bump the version vector (awset.go:97).
 * The definition is part of the ABI and does not change.  All arithmetic is mod
 * 2^64; fmix is the splitmix64 finaliser:
 *   fmix(x): x ^= x>>30; x *= 0xBF58476D1CE4E5B9; x ^= x>>27;
 *            x *= 0x94D049BB133111EB; x ^= x>>31
 *   K_E = 0x9E3779B97F4A7C15  K_T = 0xC2B2AE3D27D4EB4F  K_A = 0xD6E8FEB86659FD93
 *   K_V = 0x165667B19E3779F9  K_N = 0x85EBCA77C2B2AE63
 *   hk(k)     = fmix(k + K_E)
 *   hd(k,a,c) = fmix(hk(k) ^ (c + K_A*(a+1)))           live entry k -> dot (a,c)
 *   ht(k,a,c) = fmix(fmix(k + K_T) ^ (c + K_A*(a+1)))   live tombstone (AWSetDelta.Deleted)
 *   hv(r,v)   = v == 0 ? 0 : fmix(v + K_V*(r+1))        clock word r
 * Document d with n live entries, m live tombstones and clock vv[0..R):
 *   digest[2d]   = fmix(sum hk + K_N*n)                      the element set (what
 *                                                            assertEntries tests)
 *   digest[2d+1] = fmix(sum hd + sum ht + sum hv + K_N*(n+m))  elements, dots,
 *                                                            Deleted and clock
 *   - Live prefix only: the first counts[d] slots of a document (all slots when
 *     counts == NULL), entries and tombstones alike.  Slack is never read.  A
 *     live count above the slots is clamped to them and crdt_ctx_sync returns
 *     CRDT_E_CAPACITY, as in crdt_awset_has_async.
 *   - The sums commute: the digest does not depend on the order of a document's
 *     entries, nor on how the device cuts the work up, so it is bit-identical
 *     on every run, and a host peer may hash a Go map in iteration order
 *     without sorting.
 *   - A zero clock word contributes nothing, so the digest does not depend on
 *     the R padding: [5,0] at R = 2 and [5,0,0,0] at R = 4 digest alike (the
 *     reference's VersionVectors are ragged; peers need not agree on R).
 *   - tombs == NULL, and a tomb batch whose documents are all empty, digest
 *     alike: an AWSet and an AWSetDelta with an empty Deleted agree.
 *   - Tombstones collected on one side only (crdt_tombstone_gc_async) change
 *     word 1 and never word 0: compare word 0 if you GC independently.
 *   - Digests are comparable only between peers that share the key interning,
 *     like everything else here.
 *   - An empty document with a zero clock digests to (0, 0).
 * crdt_awset_digest_async: digest is [2*n_docs] u64 on the device.  A join,
 * exchange, fold, apply or scatter output is a valid `state` as it stands.  The
 * digest words are the accumulators: no workspace, no allocation, no host sync,
 * kernel nodes only, capturable on an unreserved context; ordered after the
 * context's previous call like every entry point.  n_docs == 0 launches nothing.
 * CRDT_E_INVALID: NULL state or digest, R out of range, tombs without offsets,
 * digest starting where an input array starts.
 * crdt_awset_digest_host: the same definition over host arrays, no GPU and no
 * context, for the peer that holds host maps; a document's entries may lie in
 * ANY order.  The slot layout and the counts are checked (CRDT_E_INVALID: NULL
 * arrays, R out of range, offsets not monotone; CRDT_E_CAPACITY: a live count
 * above its slots; nothing is clamped here).
 * crdt_digest_diff_async: mine and theirs are [2*n_docs] u64 on the device; out
 * is written as by crdt_awset_compare_async with
 *   flags[d]   CRDT_DIG_ELEMENTS when word 0 differs, else CRDT_DIG_STATE when
 *              word 1 differs, else 0 (STATE is 0 whenever ELEMENTS is set)
 *   summary    [0] documents with ELEMENTS, [1] with STATE, [2] and [3] zero,
 *              [4] documents with flags & mask
 *   worklist   ascending, the same on every run, untouched at or past *n_work
 * so the worklist and n_work feed crdt_awset_select_async with no host round
 * trip.  Validation, n_docs == 0 (summary and n_work still written) and the
 * workspace (one word per document, crdt_ctx_reserve(max_docs, ..);
 * CRDT_E_WORKSPACE under capture) are those of crdt_awset_compare_async; mine
 * and theirs may be NULL only when n_docs == 0. */
#define CRDT_DIG_ELEMENTS 1u /* word 0 differs                       (== CRDT_CMP_KEYS) */
#define CRDT_DIG_STATE    2u /* word 0 equal, word 1 differs         (== CRDT_CMP_DOTS) */
int crdt_awset_digest_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_tomb_batch* tombs /* or NULL */,
                            uint64_t* digest, void* stream);
int crdt_awset_digest_host(const crdt_awset_batch* state, const crdt_tomb_batch* tombs /* or NULL */,
                           uint64_t* digest);
int crdt_digest_diff_async(crdt_ctx* ctx, const uint64_t* mine, const uint64_t* theirs, uint32_t n_docs, uint32_t mask,
                           const crdt_compare_out* out, void* stream);

/* ---- worklist digests: re-digest only the documents a round changed ---------
 * A caller who keeps a digest array beside a resident replica brings it up to
 * date after a sparse round without reading the replica whole: the call hashes
 * only the documents idx[0 .. min(*n_idx, n_max)) names and writes their two
 * words into `digest` ([2*n_digest_docs] u64 on the device) at their own
 * positions.  Every other word of `digest` keeps the bits it had: none is read
 * or written.
 *   CRDT_DIGEST_GATHER  `state` (and tombs) is the resident replica; document
 *       idx[j] of it goes to digest[2*idx[j]], digest[2*idx[j]+1].
 *       n_digest_docs must equal state->n_docs.  The form used after
 *       crdt_replica_scatter_inplace_async, crdt_replica_scatter_async or a
 *       sparse apply.
 *   CRDT_DIGEST_PLACE   `state` is a packed or merge-output sub-batch of at least
 *       n_max documents whose document j is the replica's document idx[j]; it
 *       goes to digest[2*idx[j]], digest[2*idx[j]+1]: the merged selection is
 *       digested straight into the replica's array, before or without the
 *       scatter.  state->n_docs >= n_max is required.
 * The two words written are bit for bit what crdt_awset_digest_async and
 * crdt_awset_digest_host give for that document (the definition above: live
 * prefix only, clamped counts, tombstones, the clock without its R padding,
 * (0, 0) for an empty document with a zero clock), the same on every run.
 * idx (device) may be in any order.  In GATHER it may repeat: every writer of a
 * word writes the same bits.  In PLACE a repeated target is the caller's error
 * and is NOT checked: which of the sub-batch documents' digests stays is
 * unspecified.  n_idx (device, one word) == NULL means n_max; *n_idx is read on
 * the device, so the worklist and n_work of crdt_awset_compare_async or
 * crdt_digest_diff_async, and spill_doc and n_spill of the in-place scatter, feed
 * this call with no host round trip.  Reported by crdt_ctx_sync:
 *   CRDT_E_CAPACITY  *n_idx > n_max (clamped to n_max), or a live count above its
 *                    slots (clamped to them, as in crdt_awset_digest_async)
 *   CRDT_E_INVALID   idx[j] >= n_digest_docs (in GATHER also >= state->n_docs):
 *                    nothing is written for that j, every other j is exact
 * Returned by the call, CRDT_E_INVALID: NULL state, idx or digest, R out of
 * range, tombs without offsets, mode above 1, n_digest_docs != state->n_docs in
 * GATHER, state->n_docs < n_max in PLACE, digest or idx starting where an input
 * array starts (digest also where idx or n_idx starts).
 * No workspace, no allocation, no host sync, kernel nodes only, capturable on an
 * unreserved context; ordered after the context's previous call like every entry
 * point.  n_max == 0 launches nothing.  One wavefront digests a listed document
 * of up to 2,048 live entries plus tombstones, one workgroup a larger one. */
#define CRDT_DIGEST_GATHER 0u /* document idx[j] of `state`          -> digest[2*idx[j]], digest[2*idx[j]+1] */
#define CRDT_DIGEST_PLACE  1u /* document j of `state` (a sub-batch) -> digest[2*idx[j]], digest[2*idx[j]+1] */
int crdt_awset_digest_idx_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_tomb_batch* tombs /* or NULL */,
                                const uint32_t* idx, const uint32_t* n_idx /* or NULL */, uint32_t n_max,
                                uint32_t n_digest_docs, uint32_t mode, uint64_t* digest, void* stream);

/* ---- digest trees: find differing documents without shipping every digest ----
 * crdt_digest_diff_async needs the peer's whole digest array, 16 B a document,
 * also when nothing differs.  A hash tree of fixed fan-out over the array lets
 * two peers find the differing documents level by level: the receiver names the
 * nodes that differ, the sender packs their children (256 B a node), the
 * receiver diffs them against its own and names the next level.  At level 0 the
 * list is the document worklist, with the flags of crdt_digest_diff_async; it
 * feeds crdt_awset_select_async, crdt_replica_select_async and
 * crdt_awset_digest_idx_async as it stands.
 * The definition is part of the ABI and does not change (fmix, K_N: above):
 *   CRDT_DIGEST_TREE_FANOUT = 16      K_P = 0x2545F4914F6CDD1D
 *   Level 0 is the caller's digest array, n_0 = n_docs nodes of two words; it is
 *   not copied into the tree.  Level l >= 1 has n_l = ceil(n_(l-1) / 16) nodes.
 *   L is the smallest l >= 1 with n_l == 1: one document still has a root above
 *   it, n_docs == 0 has no levels, L <= 8.
 *   tree is [2 * sum_(l=1..L) n_l] u64: the levels concatenated from level 1
 *   upwards, level l starting at node offset sum_(1<=k<l) n_k.
 *   Node i of level l has the c children 16i .. min(16i + 15, n_(l-1) - 1) of
 *   level l-1.  For each word w of 0 and 1 separately:
 *     node[w] = fmix( sum_(j<c) fmix(child_j[w] + K_P*(j+1)) + K_N*c )   mod 2^64
 *   - The slot salt K_P*(j+1) makes two swapped children show.
 *   - The sum keeps the value independent of how the work is cut up: the tree is
 *     bit-identical on every run, on the device and on the host.
 *   - The words stay separate: word 0 of a node covers exactly the element sets
 *     below it, word 1 everything else (dots, tombstones, clocks), so the
 *     ELEMENTS / STATE distinction carries up the tree.
 * There is no incremental update, deliberately: rebuilding reads the digest
 * array once (16 MB + 1 MB at 2^20 documents), while re-deriving the ancestors of
 * a k-document worklist reads 256 B * L per document before de-duplication and
 * touches nearly every level-1 node from about 5 % random documents on.  Keep
 * the array current with crdt_awset_digest_idx_async, then rebuild the tree whole.
 *
 * crdt_digest_tree_layout (host): level_nodes[l] = n_l for l = 0 .. L and
 * level_off[l] = the node offset of level l >= 1 in `tree`, zeros above L;
 * returns L.  The tree holds level_off[L] + 1 nodes.  Either array may be NULL.
 * crdt_digest_tree_host: the definition over host arrays, no GPU and no context,
 * for the peer that holds host maps.  CRDT_E_INVALID: NULL digest or tree with
 * n_docs > 0.
 * crdt_digest_tree_async: digest [2*n_docs] and tree on the device; every level
 * is built, one launch per level and one for all levels of 4,096 children and
 * fewer.  No workspace, no allocation, no host sync, kernel nodes only,
 * capturable on an unreserved context; ordered after the context's previous
 * call like every entry point.  n_docs == 0 launches nothing.  Arrays that are
 * only 8 B aligned are read and written word by word.  CRDT_E_INVALID: NULL
 * digest or tree with n_docs > 0, tree starting where digest starts.
 *
 * crdt_digest_tree_children_async, the sender's side.  `level` is the node array
 * of level l-1 with n_level nodes (the digest array, or tree + 2*level_off[l-1]);
 * `parents` a device list of node indices of level l, in any order, NULL: the
 * identity j -> j; n_parents one device word, NULL: n_max.  For
 * j < min(*n_parents, n_max) and c < 16 both words of child 16*parents[j] + c are
 * written to out[2*(16j + c)], out[2*(16j + c) + 1]; a child at or past n_level
 * is written as zeros; no word of out past 32 * min(*n_parents, n_max) is
 * touched.  The identity form is the level itself padded to a multiple of 16,
 * which is how a descent may start at any level.  Reported by crdt_ctx_sync:
 *   CRDT_E_CAPACITY  *n_parents > n_max (clamped to n_max)
 *   CRDT_E_INVALID   parents[j] >= ceil(n_level / 16): that parent's 16 slots are
 *                    zeros, every other is exact
 * Returned by the call, CRDT_E_INVALID: NULL out, NULL level with n_level > 0,
 * out starting where level, parents or n_parents starts, n_max above
 * ceil(n_level / 16) in the identity form.  No workspace; capturable on an
 * unreserved context.  n_max == 0 launches nothing.
 *
 * crdt_digest_tree_diff_async, the receiver's side.  mine_level / n_level: the
 * receiver's own level l-1; theirs: the packed array the peer's children call
 * wrote for the same parents / n_parents / n_max.  For every listed parent and
 * every child below n_level, e is "word 0 differs" and s "word 1 differs".
 *   leaf != 0  the children are documents: flag = CRDT_DIG_ELEMENTS if e, else
 *              CRDT_DIG_STATE if s; a child is listed iff flag & mask, exactly
 *              crdt_digest_diff_async's rule.
 *   leaf == 0  the children are nodes: flag = e | (s << 1), not exclusive; a
 *              child is listed iff flag & mask.  This is a superset: a node whose
 *              word 0 differs may still hide a document that differs in word 1
 *              only, so word 1 keeps its own bit.
 *   idx_out    the listed child indices, ascending (out_max words of room), and
 *   flags_out  (u8, parallel to it, or NULL) their flags
 *   n_out      one word: their exact total
 *   summary    (5 words, or NULL) [0] children with e (leaf: ELEMENTS), [1] with
 *              s (leaf: STATE), [2] and [3] zero, [4] children listed
 * Positions come from a count, a scan of the partial sums and an emit: no atomic
 * decides a position, the result is the same on every run.  idx_out / n_out are
 * the parents / n_parents of the next level's two calls with no host round trip.
 * `parents` must be strictly ascending, which a previous level's idx_out is.
 * Reported by crdt_ctx_sync:
 *   CRDT_E_CAPACITY  the total is above out_max: *n_out and summary are exact,
 *                    nothing is written at or past out_max; or *n_parents > n_max
 *                    (clamped)
 *   CRDT_E_INVALID   parents not strictly ascending, or a parent that is no node
 *                    (it lists nothing); every write stays in bounds
 * Returned by the call, CRDT_E_INVALID: NULL idx_out or n_out, NULL theirs with
 * n_max > 0, NULL mine_level with n_level > 0, mask outside 1..3, two of the
 * written arrays starting at one address or one of them where an input starts,
 * n_max above ceil(n_level / 16) in the identity form.  The partial sums (three
 * words per 64 listed parents) follow the workspace rules of
 * crdt_awset_scatter_async: crdt_ctx_reserve(max_docs, ..) covers every level of
 * max_docs documents, and a call that would have to grow the buffer while its
 * stream is capturing returns CRDT_E_WORKSPACE.  n_max == 0 still writes *n_out
 * and the summary. */
#define CRDT_DIGEST_TREE_FANOUT 16u
int crdt_digest_tree_layout(uint32_t n_docs, uint32_t level_nodes[9] /* or NULL */, uint32_t level_off[9] /* or NULL */);
int crdt_digest_tree_host(const uint64_t* digest, uint32_t n_docs, uint64_t* tree);
int crdt_digest_tree_async(crdt_ctx* ctx, const uint64_t* digest, uint32_t n_docs, uint64_t* tree, void* stream);
int crdt_digest_tree_children_async(crdt_ctx* ctx, const uint64_t* level, uint32_t n_level,
                                    const uint32_t* parents /* or NULL */, const uint32_t* n_parents /* or NULL */,
                                    uint32_t n_max, uint64_t* out, void* stream);
int crdt_digest_tree_diff_async(crdt_ctx* ctx, const uint64_t* mine_level, uint32_t n_level, const uint64_t* theirs,
                                const uint32_t* parents /* or NULL */, const uint32_t* n_parents /* or NULL */,
                                uint32_t n_max, uint32_t leaf, uint32_t mask, uint32_t* idx_out,
                                uint8_t* flags_out /* or NULL */, uint32_t* n_out, uint32_t out_max,
                                uint32_t* summary /* or NULL */, void* stream);

/* ---- select: a subset of documents (or all: compaction) as a packed batch --
 * out gets n_out documents packed with no slack: out->offsets[j] is the
 * exclusive prefix of the live counts and offsets[n_out] the total.  For
 * j < *n_idx, document j is the live entries, count and VV of `state` document
 * idx[j]; for j >= *n_idx it is empty (count 0, VV zeros).  The result is
 * directly a valid input batch.  idx (device) may be in any order and may
 * repeat; idx == NULL is the identity j -> j; n_idx (device, one word) == NULL
 * means n_out.  idx == NULL, n_idx == NULL and n_out == state->n_docs is the
 * device-side compaction of a merge output (whose documents sit at capacity
 * offsets).  *n_idx is read on the device, so the worklist and n_work of
 * crdt_awset_compare_async feed this call with no host round trip; only
 * choosing a smaller n_out needs the 4-byte read-back of n_work.
 * out must hold n_out + 1 offsets, n_out counts, n_out * R clock words and
 * out_slots entries.  Reported by crdt_ctx_sync:
 *   *n_idx > n_out       clamped to n_out, CRDT_E_CAPACITY
 *   total > out_slots    CRDT_E_CAPACITY; nothing is written at or past out_slots
 *   idx[j] >= n_docs     CRDT_E_INVALID; that document comes out empty
 *   a live count above the document's slots: clamped, CRDT_E_CAPACITY
 * out must not alias state: an out array starting where the state's array of
 * the same kind starts makes the call return CRDT_E_INVALID, as in the exchange.
 * No workspace, no allocation, no host sync: capturable on any context. */
int crdt_awset_select_async(crdt_ctx* ctx, const crdt_awset_batch* state, const uint32_t* idx,
                            const uint32_t* n_idx /* device, [1] */, uint32_t n_out, uint32_t out_slots,
                            const crdt_awset_out* out, void* stream);

/* ---- scatter: a merged sub-batch put back into the batch it was selected from
 * The inverse of select.  out gets state->n_docs documents packed with no
 * slack: out->offsets[d] is the exclusive prefix of the live counts and
 * offsets[n_docs] the total.  If idx[j] == d for some j < *n_idx, document d is
 * the live entries, count and VV of `sub` document j; otherwise it is the live
 * entries, count and VV of `state` document d.  A replacement may be longer,
 * shorter or empty, so every later offset moves.  The result is directly a
 * valid input batch.
 * state and sub must agree in R; their slot layouts are independent, either may
 * have counts, slack and documents at capacity offsets (a join, exchange, fold
 * or apply output is valid as it stands: the crdt_awset_out of an exchange over
 * a selected sub-batch is the intended `sub`), and only live prefixes are read.
 * idx (device, sub->n_docs words, required) may be in any order; n_idx (device,
 * one word) == NULL means sub->n_docs.  *n_idx is read on the device, so the
 * worklist and n_work of crdt_awset_compare_async feed select, the merge and
 * this call with no host round trip.  *n_idx == 0 is the identity select of
 * state.  state->n_docs == 0: offsets[0] = 0 is written and nothing that reads
 * documents is launched.
 * out must hold n_docs + 1 offsets, n_docs counts, n_docs * R clock words and
 * out_slots entries; entry slots at or past the total are not written.
 * Reported by crdt_ctx_sync:
 *   *n_idx > sub->n_docs  clamped to sub->n_docs, CRDT_E_CAPACITY
 *   idx[j] >= n_docs      CRDT_E_INVALID; that sub document is ignored
 *   two j name one document: CRDT_E_INVALID; the lowest j supplies it, so the
 *                         output is the same on every run
 *   total > out_slots     CRDT_E_CAPACITY; nothing is written at or past out_slots
 *   a live count above its document's slots, on either source: clamped,
 *                         CRDT_E_CAPACITY
 * Returned by the call (CRDT_E_INVALID): state, sub, out or idx NULL; R
 * different between state and sub, or out of range; an out array starting where
 * the array of the same kind of state or sub starts.
 * Workspace: one inverse-map word per state document (0xFFFFFFFF = not
 * replaced) and the partial sums of the offset scan (one word per 1,024
 * documents), in the context's buffers that crdt_ctx_reserve(max_docs, ..)
 * sizes: no allocation on a reserved context, CRDT_E_WORKSPACE when they would
 * have to grow during a graph capture.  No host sync, kernel nodes only,
 * capturable; ordered after the context's previous call like every entry point. */
int crdt_awset_scatter_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_awset_batch* sub,
                             const uint32_t* idx, const uint32_t* n_idx /* device, [1], or NULL */,
                             uint32_t out_slots, const crdt_awset_out* out, void* stream);

/* ---- merge diff: what a merge changed, per document -------------------------
 * Every merge call answers "what is the merged state"; this one answers "what
 * did the merge change".  The reference prints it per key as merge's decision
 * log -- update, add, skip, remove, keep (awset.go:109-158); this is its
 * structured form, for whoever keeps something beside the set (an index, a view,
 * a subscriber list) and for a host boundary that applies a merge output to Go
 * maps: only the lists need to cross PCIe, not the merged state.
 * before and after are two batches with the same n_docs and R.  Their slot
 * layouts are independent; either may have counts, slack, or documents at
 * capacity offsets: a join, exchange, fold, apply, select or scatter output is
 * valid as it stands.  Only live prefixes are read (the first counts[d] slots of
 * a document, all slots when counts == NULL); slack is never read, whatever it
 * holds.  The entries need no clock: only the CLOCK flag reads the vv.
 * Per document d:
 *   - removed: the live entries of before[d] whose key is not a live key of
 *     after[d], in key order, with the dot they had in before (the log's
 *     phase-2 `remove`, awset.go:145-158).
 *   - upserted: the live entries of after[d] whose key is not live in before[d]
 *     (kind CRDT_DIFF_ADDED: the log's `add`) or is live there under a different
 *     (actor, counter) (kind CRDT_DIFF_UPDATED: the log's `update`), in key
 *     order, with the dot they have in after.
 *     Deleting `removed` from before[d] and then assigning `upserted` gives
 *     exactly after[d]'s live entries.
 *   - flags[d] is the OR of CRDT_DIFF_REMOVED | CRDT_DIFF_ADDED |
 *     CRDT_DIFF_UPDATED for the kinds present, plus CRDT_DIFF_CLOCK when any of
 *     the R clock words differs.  flags[d] == 0 iff live state and VV are
 *     bit-identical: the same statement as crdt_awset_compare_*'s flags[d] == 0.
 *   - Both lists are packed with no slack: rem_off / ups_off are [n_docs + 1]
 *     exclusive prefixes and the last word is the total.  The offsets and the
 *     totals are exact even when a total exceeds the caller's rem_slots /
 *     ups_slots: crdt_ctx_sync then returns CRDT_E_CAPACITY, nothing is written
 *     at or past the slots given (the other list is complete), and the caller
 *     can read the totals, resize and call again.  rem_slots == 0 and ups_slots
 *     == 0 with NULL lists is the sizing call.
 *   - summary (optional): [0] removed records, [1] upsert records, [2] upsert
 *     records that are UPDATED, [3] documents with an entry change, [4]
 *     documents with flags != 0.
 *   - The output is the same bits on every run: no atomic decides a position.
 *   - A live count above a document's slots is clamped to them and crdt_ctx_sync
 *     returns CRDT_E_CAPACITY, as in crdt_awset_compare_async.
 * Returned by the call (CRDT_E_INVALID): before, after or out NULL; flags,
 * rem_off or ups_off NULL; rem_keys NULL with rem_slots > 0, ups_keys NULL with
 * ups_slots > 0; exactly one of a list's actors / counters NULL; an n_docs or R
 * mismatch, R out of range; an out array starting where an input array of the
 * same kind starts (offsets and counts against rem_off / ups_off; keys, actors,
 * counters against the lists' columns), or the two lists sharing a column.
 * n_docs == 0: rem_off[0], ups_off[0] and summary are written (zeros) and
 * nothing else; nothing that reads documents is launched.
 * Callers compose, this call does not: there is no idx argument.  To diff only
 * the documents a compare or digest worklist names, crdt_awset_select_async both
 * sides with that worklist first and diff the two selections.
 * _async: no host sync, kernel nodes only, capturable; ordered after the
 * context's previous call like every entry point.  Workspace: one flag word per
 * document, in the buffer crdt_ctx_reserve(max_docs, ..) sizes (no allocation
 * on a reserved context, CRDT_E_WORKSPACE when it would have to grow during a
 * graph capture), and a fixed 24 KB of partial sums the context owns from its
 * creation.
 * _batch (host arrays; for tests and small callers): checks the slot layouts
 * and counts on the host (CRDT_E_INVALID / CRDT_E_CAPACITY), the key order on the
 * device after the upload (CRDT_E_UNSORTED: no diff runs, out untouched), and
 * downloads only flags, summary, the offsets and the first min(total, slots)
 * words of each list, never a state.  A total above its slots returns
 * CRDT_E_CAPACITY after that download, so the totals can be read. */
#define CRDT_DIFF_REMOVED 1u /* a live key of before[d] is not live in after[d]       */
#define CRDT_DIFF_ADDED   2u /* a live key of after[d] is not live in before[d]       */
#define CRDT_DIFF_UPDATED 4u /* a key live in both, under different (actor, counter)  */
#define CRDT_DIFF_CLOCK   8u /* before.vv[r] != after.vv[r] for some r < R            */
typedef struct {            /* written */
    uint8_t*  flags;        /* [n_docs] OR of CRDT_DIFF_* for doc d */
    uint32_t* summary;      /* [5], may be NULL */
    uint32_t* rem_off;      /* [n_docs+1] */
    uint64_t* rem_keys;  uint32_t* rem_actors;  uint64_t* rem_counters;   /* dots: both or neither NULL */
    uint32_t* ups_off;      /* [n_docs+1] */
    uint64_t* ups_keys;  uint32_t* ups_actors;  uint64_t* ups_counters;
    uint8_t*  ups_kind;     /* [ups total] CRDT_DIFF_ADDED | CRDT_DIFF_UPDATED, may be NULL */
} crdt_diff_out;
int crdt_awset_diff_async(crdt_ctx* ctx, const crdt_awset_batch* before, const crdt_awset_batch* after,
                          uint32_t rem_slots, uint32_t ups_slots, const crdt_diff_out* out, void* stream);
int crdt_awset_diff_batch(crdt_ctx* ctx, const crdt_awset_batch* before, const crdt_awset_batch* after,
                          uint32_t rem_slots, uint32_t ups_slots, const crdt_diff_out* out);

/* ---- logged join and exchange: the merge with its decision log ----------------
 * crdt_awset_diff_* answers "what did the merge change" after the fact, from a
 * second read of both batches and a search per key.  The joins' kernels have
 * made every one of those decisions when they write the merged state (merge's
 * log, awset.go:109-158): a dst-only key the src clock covers is a `remove`, a
 * src-only key that survives an `add`, a common key whose dot changes an
 * `update`.  These two calls write that log beside the merged state, from the
 * one read the merge needs anyway.
 * The merged state: out (out_ab, out_ba) holds what crdt_awset_join_async
 * (crdt_awset_exchange_async) writes for the same inputs -- live entries,
 * counts, offsets and clocks bit for bit, document d at dst.offsets[d] +
 * src.offsets[d], slack unspecified.
 * The log of direction dst <- src is crdt_awset_diff_*'s answer for before =
 * dst, after = out, in a different layout.  Per document d:
 *   - removed: the live entries of dst[d] whose key is not live in out[d], in
 *     key order, with the dot they had in dst.
 *   - upserted: the live entries of out[d] whose key was not live in dst[d]
 *     (ups_kind CRDT_DIFF_ADDED) or was live there under a different (actor,
 *     counter) (CRDT_DIFF_UPDATED), in key order, with their new dot.
 *   - flags[d] and summary as crdt_awset_diff_async(dst, out) writes them,
 *     CRDT_DIFF_CLOCK included.
 * Layout: like every merge output, it needs no scan over documents.  A removed
 * entry was a dst entry, so document d's removed list starts at dst.offsets[d]
 * and holds rem_counts[d] entries, and rem_offsets repeats dst's slot bounds
 * (n_docs + 1 values); an upserted entry was a src entry, so its list starts at
 * src.offsets[d], holds ups_counts[d] entries, and ups_offsets repeats src's
 * bounds.  Each list read as (offsets, counts, keys, actors, counters) is a
 * valid crdt_tomb_batch as it stands.  Slots of a document at or past its count
 * are unspecified; slots of other documents are never written.  The bits are the
 * same on every run: no atomic decides a position (summary is a sum of integers).
 * Exchange: both directions from one read, as crdt_awset_exchange_async defines
 * them.  log_ab.removed is in a's layout and log_ab.upserted in b's; log_ba.removed
 * is in b's layout and log_ba.upserted in a's.  The shared key column stays the
 * plain exchange's: out_ba->keys == out_ab->keys is refused here.
 * Only live prefixes are read (counts, or all slots when counts == NULL); the two
 * batches' slot layouts are independent.
 * Reported by crdt_ctx_sync:
 *   CRDT_E_ACTOR_RANGE  any HasDot the merge evaluates at actor == R, as in the joins
 *   CRDT_E_CAPACITY     a live count above its slots (clamped)
 * Returned by the call (CRDT_E_INVALID): a NULL argument or a NULL required field
 * (summary and ups_kind may be NULL); an n_docs or R mismatch; R out of range; two
 * written arrays starting at one address (the shared key column included) or
 * overlapping per-document arrays; a written array starting where an input array
 * of the same kind starts.
 * n_docs == 0 launches nothing that reads documents; summary, when given, is
 * zeroed.  Ordered after the context's previous call; no host sync, kernel nodes
 * only, capturable.  Workspace: the join's worklist, one word per
 * document, sized by crdt_ctx_reserve(max_docs, ..); CRDT_E_WORKSPACE when it
 * would have to grow during a graph capture; and a fixed 64 KB of summary partial
 * sums in a buffer the context owns from its creation.  There is no _batch form. */
typedef struct {            /* written */
    uint8_t*  flags;        /* [n_docs] OR of CRDT_DIFF_REMOVED|ADDED|UPDATED|CLOCK */
    uint32_t* summary;      /* [5] as crdt_diff_out.summary, may be NULL */
    uint32_t* rem_offsets;  /* [n_docs+1] = dst.offsets */
    uint32_t* rem_counts;   /* [n_docs] */
    uint64_t* rem_keys;  uint32_t* rem_actors;  uint64_t* rem_counters;   /* capacity: dst's slots */
    uint32_t* ups_offsets;  /* [n_docs+1] = src.offsets */
    uint32_t* ups_counts;   /* [n_docs] */
    uint64_t* ups_keys;  uint32_t* ups_actors;  uint64_t* ups_counters;   /* capacity: src's slots */
    uint8_t*  ups_kind;     /* [src slots] CRDT_DIFF_ADDED | CRDT_DIFF_UPDATED, may be NULL */
} crdt_merge_log;
int crdt_awset_join_log_async(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_awset_batch* src,
                              const crdt_awset_out* out, const crdt_merge_log* log, void* stream);
int crdt_awset_exchange_log_async(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b,
                                  const crdt_awset_out* out_ab, const crdt_awset_out* out_ba,
                                  const crdt_merge_log* log_ab, const crdt_merge_log* log_ba, void* stream);

/* ---- sources: resident replicas assembled into a fold / extraction input ----
 * Replicas live on the device as state batches (crdt_awset_batch, plus
 * crdt_tomb_batch for AWSetDelta.Deleted, plus the replica's actor): the shape
 * apply, the joins, the folds and scatter write, with offsets, counts and slack.
 * The folds and the delta extraction read a crdt_src_batch.  This call gathers
 * n_reps replicas of the same n_docs documents into one packed source batch.
 * Shape: out describes a source batch with the replicas' common n_docs and R;
 * doc_srcs[d] = d * n_reps for d <= n_docs; source s = d * n_reps + p is replica
 * p's document d, so the replica order is the fold order.
 * Per source: src_actor[s] = reps[p].doc_actor[d], or reps[p].actor when
 * doc_actor is NULL; vv[s*R..] is the document's clock; the entries are the
 * document's live prefix (its first counts[d] slots, all slots when counts ==
 * NULL; slack is never read); the tombstones are the live prefix of `tombs`,
 * copied verbatim (the re-add filter belongs to the extraction).
 * Packing: entry_off and tomb_off are exclusive prefixes over all sources, no
 * slack; entry_off[n_srcs] and tomb_off[n_srcs] are the totals.  Everything
 * comes out in the order it had, so it stays key-ascending: the result is a
 * valid `srcs` of crdt_awset_fold_* in both modes and of
 * crdt_awset_delta_extract_*, as it stands.  A join, exchange, fold, apply or
 * scatter output is a valid replica state as it stands.
 * Tombstones: a replica with tombs == NULL contributes empty tombstone ranges.
 * If every replica has tombs == NULL, out may pass NULL tombstone arrays, and a
 * tomb_off it does pass is zeroed (the extraction's convention).  out->kind is
 * never written.
 * out must hold n_docs + 1 doc_srcs, n_srcs src_actor, n_srcs * R clock words,
 * n_srcs + 1 entry_off (and tomb_off), entry_slots entries and tomb_slots
 * tombstones.  Reported by crdt_ctx_sync:
 *   a live count above its slots, entries or tombstones: clamped, CRDT_E_CAPACITY
 *   a total above entry_slots or tomb_slots: CRDT_E_CAPACITY; nothing is written
 *                         at or past those slots (running totals in 64 bits)
 * Returned by the call (CRDT_E_INVALID): n_reps == 0 or > CRDT_MAX_REPLICAS;
 * reps, a state or out NULL, or a required out array NULL (the tombstone arrays
 * are required when some replica has tombs); replicas that disagree in n_docs
 * or R; R out of range; n_docs * n_reps >= 2^32; an out array starting where
 * the array of the same kind of any replica starts.
 * n_docs == 0: doc_srcs[0], entry_off[0] and tomb_off[0] are written as 0 and
 * nothing that reads documents is launched.
 * Workspace: the partial sums of the offset scan, two words per 1,024 sources,
 * in the context's buffers that crdt_ctx_reserve(max_docs, ..) sizes (each holds
 * max_docs words: enough for 1,024 * max_docs sources): no allocation on a
 * context reserved for n_srcs / 1,024 documents or more, CRDT_E_WORKSPACE when
 * they would have to grow during a graph capture.  The replica descriptors
 * travel in the kernel arguments: no host allocation, no copy call.  No host
 * sync, kernel nodes only, capturable; ordered after the context's previous
 * call like every entry point.  There is no _batch form: a caller who holds
 * host data builds the source batch on the host. */
#define CRDT_MAX_REPLICAS 16
typedef struct {                     /* one resident replica of every document (read-only) */
    const crdt_awset_batch* state;   /* required */
    const crdt_tomb_batch*  tombs;   /* AWSetDelta.Deleted, or NULL: none */
    const uint32_t* doc_actor;       /* device [n_docs]: AWSet.Actor per document (as crdt_op_batch), or NULL */
    uint32_t actor;                  /* used for every document when doc_actor == NULL */
} crdt_replica;
int crdt_awset_sources_async(crdt_ctx* ctx, const crdt_replica* reps, uint32_t n_reps, uint32_t entry_slots,
                             uint32_t tomb_slots, const crdt_delta_out* out, void* stream);

/* ---- replica select and scatter: Deleted and actors follow their documents ----
 * crdt_awset_select_async / crdt_awset_scatter_async over a whole crdt_replica:
 * the documents move with their AWSetDelta.Deleted tombstones and their actors,
 * so a sparse delta round (digest, digest_diff, select both replicas, delta
 * exchange, scatter both) and a sparse apply (select, apply, scatter) run with
 * nothing downloaded, and select-all packs a replica whose tombstones carry the
 * slack apply leaves.
 * Document mapping: select's and scatter's.  Select: out gets n_out documents;
 * for j < *n_idx document j is `rep` document idx[j] (idx == NULL: j), beyond it
 * is empty.  Scatter: out gets rep->state->n_docs documents; document d is `sub`
 * document j when idx[j] == d for some j < *n_idx (the lowest such j), and `rep`
 * document d otherwise.  rep and sub must agree in R; their document counts and
 * slot layouts are independent.
 * State part: out->state is bit for bit what crdt_awset_select_async /
 * crdt_awset_scatter_async write for the same state, idx, n_idx, n_out and
 * out_slots = entry_slots: live entries, counts and VV, packed with no slack,
 * offsets the exclusive prefix of the live counts, offsets[n_out] the total.
 * idx == NULL, n_idx == NULL and n_out == n_docs is the compaction of the replica.
 * Tombstones: the same document mapping over rep->tombs (or sub->tombs).  The
 * live prefix (counts[d] slots, all slots when counts == NULL) is copied verbatim
 * in its order, packed with no slack; out->tombs->offsets[n_out] is the total and
 * counts are written.  A replica with tombs == NULL contributes empty ranges.  If
 * no input replica has tombs, out->tombs may be NULL, and an out->tombs->offsets
 * (and counts) that is passed is zeroed (the convention of sources).  Compaction
 * of an apply output's tombstones (which sit at tombs.offsets[d] + op_off[d]) is
 * this call with idx == NULL.
 * Actors: when out->doc_actor != NULL, doc_actor[j] is the chosen source
 * document's actor: doc_actor[d] of that replica, or its uniform `actor` when its
 * doc_actor == NULL; empty documents beyond *n_idx get 0.
 * out->state must hold n_out + 1 offsets, n_out counts, n_out * R clock words and
 * entry_slots entries; out->tombs n_out + 1 offsets, n_out counts and tomb_slots
 * tombstones; out->doc_actor n_out words.  Reported by crdt_ctx_sync:
 *   select:  *n_idx > n_out  clamped to n_out, CRDT_E_CAPACITY
 *            idx[j] >= n_docs  CRDT_E_INVALID; that document comes out empty
 *   scatter: *n_idx > sub n_docs  clamped, CRDT_E_CAPACITY
 *            idx[j] >= n_docs  CRDT_E_INVALID; that sub document is ignored
 *            two j name one document: CRDT_E_INVALID; the lowest j supplies it
 *   a live count above its slots, entries or tombstones, on either source:
 *                         clamped, CRDT_E_CAPACITY
 *   an entry total above entry_slots, or a tombstone total above tomb_slots
 *                         (independently): CRDT_E_CAPACITY; nothing is written at
 *                         or past the exceeded array's slots; offsets and totals
 *                         stay exact (running totals in 64 bits)
 * Returned by the call (CRDT_E_INVALID): rep, a state, out or out->state NULL, or
 * one of its arrays; for scatter sub or idx NULL, or R different between rep and
 * sub; R out of range; a tomb batch without offsets; out->tombs (or one of its
 * arrays) NULL although an input replica has tombs; an output array starting
 * where an input array of the same kind starts.
 * Empty calls: with n_docs == 0 or n_out == 0, offsets[0] = 0 is written for
 * entries and tombstones and nothing that reads documents is launched.
 * Workspace: the partial sums of the offset scan, two words per 1,024 output
 * documents, and for scatter one inverse-map word per document (0xFFFFFFFF = not
 * replaced), in the context's buffers that crdt_ctx_reserve(max_docs, ..) sizes:
 * no allocation on a reserved context, CRDT_E_WORKSPACE when they would have to
 * grow during a graph capture.  The replica descriptors travel in the kernel
 * arguments.  No host sync, kernel nodes only, capturable; ordered after the
 * context's previous call like every entry point.  There is no _batch form. */
typedef struct {                    /* one resident replica, written */
    const crdt_awset_out* state;    /* required */
    const crdt_tomb_out*  tombs;    /* required iff some input replica of the call has tombs; else may be NULL */
    uint32_t* doc_actor;            /* [n_out documents], or NULL: actors not written */
} crdt_replica_out;
int crdt_replica_select_async(crdt_ctx* ctx, const crdt_replica* rep, const uint32_t* idx,
                              const uint32_t* n_idx /* device, [1], or NULL */, uint32_t n_out,
                              uint32_t entry_slots, uint32_t tomb_slots, const crdt_replica_out* out, void* stream);
int crdt_replica_scatter_async(crdt_ctx* ctx, const crdt_replica* rep, const crdt_replica* sub,
                               const uint32_t* idx, const uint32_t* n_idx /* device, [1], or NULL */,
                               uint32_t entry_slots, uint32_t tomb_slots, const crdt_replica_out* out, void* stream);

/* ---- in-place replica scatter: merged documents written back where they fit ----
 * Replaces crdt_replica_scatter_async (and, for state-only batches,
 * crdt_awset_scatter_async) in the sparse rounds.  Those calls write a new, packed
 * copy of the whole replica, so putting 5 % of the documents back costs a pass
 * over 100 %.  This call writes each merged document into the slots its document
 * already owns when it fits, touches nothing else, and names the documents that
 * do not fit, so that only those take the packed scatter.  Every merge output
 * sits at capacity offsets and so carries the slack this needs.
 * Document mapping: crdt_replica_scatter_async's.  Every j < *n_idx with
 * d = idx[j] takes part (n_idx == NULL: sub->state->n_docs).  Reported by
 * crdt_ctx_sync:
 *   *n_idx > sub n_docs   clamped, CRDT_E_CAPACITY
 *   idx[j] >= n_docs      CRDT_E_INVALID; that sub document is ignored
 *   two j name one document: CRDT_E_INVALID; the lowest j supplies it, the others
 *                         are ignored and never listed as spilled
 *   a sub live count above its slots, entries or tombstones: clamped,
 *                         CRDT_E_CAPACITY
 * Verdict per winning j, all or nothing.  ne, nt: sub document j's clamped live
 * entry and tombstone counts (nt = 0 when sub->tombs == NULL); ce = offsets[d+1] -
 * offsets[d], ct the same over tomb_offsets (0 when tomb_offsets == NULL).
 *   Placed, iff ne <= ce and nt <= ct: the live entries are copied verbatim to
 *     offsets[d] + i and counts[d] = ne; the R clock words are copied; the live
 *     tombstones are copied to tomb_offsets[d] + i and tomb_counts[d] = nt (0 when
 *     the replica keeps tombstones and sub has none); doc_actor[d], when given,
 *     becomes sub's actor for j (its doc_actor[j], or its uniform actor).
 *   Spilled, otherwise: nothing of document d is written (no entries, tombstones,
 *     count, clock or actor); j is appended to spill_j and d to spill_doc.  A
 *     spill is not an error.
 * Never written: offsets and tomb_offsets; every word of every document not
 * placed; in a placed document, every slot at or past its new count.  The
 * replica after the call is bit-identical to the replica before it except for
 * the live prefixes, counts, clocks and actors of the placed documents.
 * Spill lists: spill_j ascending, spill_doc[i] = idx[spill_j[i]], *n_spill exact;
 * no atomic decides a position, so the bits are the same on every run.  They
 * feed the existing calls with no host round trip:
 * crdt_replica_select_async(sub, spill_j, n_spill, ..) followed by
 * crdt_replica_scatter_async(rep, that, spill_doc, n_spill, ..) is the fallback
 * for what did not fit (with *n_spill == 0 that scatter is the identity); a
 * caller reads back the 4 bytes of n_spill to skip it.
 * Returned by the call (CRDT_E_INVALID): a NULL argument or a NULL required
 * array (counts included); R different between rep and sub, or out of range;
 * sub->tombs != NULL while rep->tomb_offsets == NULL; a tombstone batch without
 * offsets; a written array of rep starting where an array of the same kind of
 * sub starts; idx or a spill array NULL.
 * Empty calls: with n_docs == 0 or no sub documents, *n_spill = 0 is written and
 * nothing that reads documents is launched.
 * State-only batches: a crdt_replica with tombs == NULL onto a target with
 * tomb_offsets == NULL and doc_actor == NULL.
 * Workspace: the inverse map (one word per replica document), one verdict word
 * per sub document and the spill scan's partial sums (one word per 1,024 sub
 * documents), in context buffers that crdt_ctx_reserve(max_docs, ..) sizes for
 * max_docs >= both document counts: no allocation on a reserved context,
 * CRDT_E_WORKSPACE when one would have to grow during a graph capture.  No host
 * sync, kernel nodes only, capturable; ordered after the context's previous call
 * like every entry point; errors reported by crdt_ctx_sync. */
typedef struct {                 /* a resident replica updated in place */
    uint32_t n_docs; uint32_t R;
    const uint32_t* offsets;     /* [n_docs+1] slot bounds: read, never written        */
    uint32_t* counts;            /* [n_docs]   required (a document's length changes)  */
    uint64_t* keys; uint32_t* actors; uint64_t* counters;
    uint64_t* vv;                /* [n_docs*R] */
    const uint32_t* tomb_offsets;/* [n_docs+1], or NULL: the replica keeps no Deleted  */
    uint32_t* tomb_counts;       /* required when tomb_offsets != NULL                 */
    uint64_t* tkeys; uint32_t* tactors; uint64_t* tcounters;
    uint32_t* doc_actor;         /* [n_docs] or NULL: actors not written               */
} crdt_replica_inplace;

typedef struct {                 /* written; each list holds sub->state->n_docs words  */
    uint32_t* spill_j;           /* sub documents that did not fit, ascending          */
    uint32_t* spill_doc;         /* idx[spill_j[i]]: the replica document each names   */
    uint32_t* n_spill;           /* device, [1]                                        */
} crdt_spill_out;

int crdt_replica_scatter_inplace_async(crdt_ctx* ctx, const crdt_replica_inplace* rep,
                                       const crdt_replica* sub, const uint32_t* idx,
                                       const uint32_t* n_idx /* device, [1], or NULL */,
                                       const crdt_spill_out* spill, void* stream);

/* ---- replica repack with headroom: the layout policy of the in-place scatter ----
 * crdt_replica_select_async and crdt_replica_scatter_async write "packed with no
 * slack", and they are the fallback for a spill of
 * crdt_replica_scatter_inplace_async: a replica that has spilled comes back with
 * no spare slot and spills again.  This call is the same select (sub == NULL) or
 * scatter (sub != NULL) writing a layout that leaves every document spare slots,
 * by a policy the caller states.
 * Capacity of a document with n live slots (part of the ABI, like the digest):
 *     cap(n) = round_up(n + max(min_spare, (n * num) >> shift), align)
 * computed in 64 bits; a value above 2^32 - 1 saturates to 2^32 - 1.
 * crdt_headroom_capacity is that expression on the host (pure, no context); the
 * kernels evaluate the same inline.  A NULL policy is {0, 0, 0, 1}: packed.
 * entry_room sizes the entries, tomb_room the tombstones, independently.
 * Document mapping: with sub == NULL crdt_replica_select_async's (idx, n_idx,
 * n_out, empty documents beyond *n_idx); with sub != NULL
 * crdt_replica_scatter_async's (the inverse map, the lowest j wins), and n_out
 * must equal rep->state->n_docs.  An empty document gets cap(0) slots too: it can
 * take an Add.
 * Layout written: offsets is the exclusive prefix of the capacities and
 * offsets[n_out] their total; counts[d] is the live count (always written); the
 * live prefix, clock, tombstone live prefix and actor are what select and scatter
 * copy.  out->tombs, when passed, gets the tombstone layout by tomb_room even when
 * no input replica has tombs (cap(0) slots each).  Every slot at or past a
 * document's live count is never written.  With offsets[0] = 0 every document
 * starts at a multiple of align.  The output is a crdt_replica as it stands, and a
 * crdt_replica_inplace target (offsets, counts, columns, clock, tombstone arrays,
 * doc_actor) with no copy.  With both policies NULL every word the select and
 * scatter calls write is written bit-identically.
 * Reported by crdt_ctx_sync: the clamps and index errors of select and scatter,
 * unchanged; CRDT_E_CAPACITY when the capacity total of the entries exceeds
 * entry_slots or that of the tombstones tomb_slots (independently): nothing is
 * written at or past the exceeded array's slots, offsets and totals stay the
 * exact prefix modulo 2^32 (running totals in 64 bits), so a caller can size its
 * buffers from a first call; CRDT_E_CAPACITY when one document's cap(n) saturates.
 * Returned by the call (CRDT_E_INVALID): align not a power of two in 1..64;
 * shift > 31; sub != NULL and n_out != rep->state->n_docs; everything the select
 * and scatter forms return it for.
 * Empty calls, workspace (partial sums per 1,024 documents; the inverse map for the
 * scatter mapping; crdt_ctx_reserve sizing; CRDT_E_WORKSPACE under capture) and
 * ordering are select's and scatter's: kernel nodes only, capturable.  There is no
 * _batch form. */
typedef struct {                 /* capacity of a document with n live slots          */
    uint32_t min_spare;          /* at least this many spare slots                     */
    uint32_t num;                /* and at least (n * num) >> shift, in 64 bits        */
    uint32_t shift;              /* <= 31                                              */
    uint32_t align;              /* capacity rounded up to a multiple: 1, 2, 4, .., 64 */
} crdt_headroom;
uint32_t crdt_headroom_capacity(const crdt_headroom* h /* NULL: packed */, uint32_t n);
int crdt_replica_repack_async(crdt_ctx* ctx, const crdt_replica* rep, const crdt_replica* sub /* or NULL */,
                              const uint32_t* idx, const uint32_t* n_idx /* device, [1], or NULL */, uint32_t n_out,
                              const crdt_headroom* entry_room, const crdt_headroom* tomb_room,
                              uint32_t entry_slots, uint32_t tomb_slots, const crdt_replica_out* out, void* stream);

/* ---- delta merge of a resident replica pair ---------------------------------
 * (*AWSetDelta).Merge (awset-delta_test.go:51-65) applied to replicas in their
 * resident shape, with no source batch in between: out[d] = dst[d] <- src[d],
 * and for the exchange out_ab[d] = a[d] <- b[d] AND out_ba[d] = b[d] <- a[d]
 * (the test's A.Merge(B); B.Merge(A), :173-174) from ONE read of both replicas;
 * both directions read the states as they were before the call.  A crdt_replica
 * is used as it stands (state, tombs or NULL, doc_actor or actor); the join's
 * dst is a plain state, since the destination's tombstones and actor are not read.
 * Per direction dst <- src of document d, with s = src's actor for d and D, S
 * the two clocks before the call, kind[d] (when kind != NULL) is
 *   CRDT_DELTA_FULL   D.Counter(s) == 0 (:53): merge(S, src.Entries), exactly
 *                     what crdt_awset_join_async writes; tombstones ignored
 *   CRDT_DELTA_NONE   otherwise, when no src entry has a dot D has not seen
 *                     (changed, :84-92) and no src tombstone passes the re-add
 *                     filter (:93-102, which reads src's own entries, not D):
 *                     dst's live entries and dst's clock UNCHANGED (:60: the
 *                     clock is not merged)
 *   CRDT_DELTA_DELTA  otherwise: deltaMerge (:107-166).  Phase 2 runs over the
 *                     entries after phase 1, so an entry phase 1 just added can
 *                     be removed by a tombstone of its key; a tombstone whose key
 *                     neither replica holds still makes the document DELTA; the
 *                     clock becomes max(D, S).
 * Layout: the join's.  Document d of either output is at a.offsets[d] +
 * b.offsets[d] with both inputs' capacity, entries in key order; offsets, counts
 * and vv are written for every document; slack is unspecified.  Only live
 * prefixes are read (counts, or all slots when counts == NULL), of entries and
 * tombstones alike; the two replicas' slot layouts are independent; any join,
 * exchange, fold, apply, select or scatter output is a valid state as it stands.
 * Reported by crdt_ctx_sync:
 *   CRDT_E_ACTOR_RANGE  Counter(s) at s == R, and any HasDot the chosen path
 *                       evaluates at actor == R (as in the folds); s > R is
 *                       "never seen": the document is FULL
 *   CRDT_E_CAPACITY     a live count above its slots (clamped)
 * Returned by the call (CRDT_E_INVALID): a NULL argument other than kind; an
 * n_docs or R mismatch; R out of range; a tomb batch without offsets; two output
 * arrays starting at one address (the key sets of the two directions differ:
 * there is no shared key column) or overlapping per-document arrays; an output
 * array starting where an input array of the same kind starts.
 * n_docs == 0 launches nothing.  Ordered after the context's previous call; no
 * host sync, kernel nodes only, capturable.  Workspace: the join's worklist, one
 * word per document, sized by crdt_ctx_reserve(max_docs, ..); CRDT_E_WORKSPACE
 * when it would have to grow during a graph capture.  There is no _batch form: a
 * caller who holds host data builds a source batch and folds. */
int crdt_awset_delta_join_async(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_replica* src,
                                const crdt_awset_out* out, uint8_t* kind /* [n_docs] or NULL */, void* stream);
int crdt_awset_delta_exchange_async(crdt_ctx* ctx, const crdt_replica* a, const crdt_replica* b,
                                    const crdt_awset_out* out_ab, const crdt_awset_out* out_ba,
                                    uint8_t* kind_ab, uint8_t* kind_ba /* each [n_docs] or NULL */, void* stream);

/* ---- logged delta merge: the delta merge with its decision log ----------------
 * The two calls above with the log of crdt_awset_join_log_async beside them: who
 * keeps an index, a view or a feed beside the sets learns what a delta merge
 * changed without crdt_awset_diff_async's second read of both batches and its
 * search per key.  The delta merge's kernels have made every one of those
 * decisions when they write the merged state.
 * The merged state: out (out_ab, out_ba) and kind (kind_ab, kind_ba) hold what
 * crdt_awset_delta_join_async (crdt_awset_delta_exchange_async) writes for the
 * same inputs -- live entries, counts, offsets, clocks and kinds bit for bit,
 * document d at a.offsets[d] + b.offsets[d], slack unspecified.
 * The log of direction dst <- src is crdt_awset_diff_async(dst, out)'s answer in
 * the logged join's layout (crdt_merge_log, above): removed records at
 * dst.offsets[d], rem_offsets repeating dst's slot bounds; upserted records at
 * src.offsets[d], ups_offsets repeating src's; each list in key order and a valid
 * crdt_tomb_batch as it stands; flags[d] and the five words of summary as there.
 * By the kind of the direction (awset-delta_test.go:51-166):
 *   CRDT_DELTA_FULL   exactly the log crdt_awset_join_log_async writes.
 *   CRDT_DELTA_NONE   both lists empty and flags[d] == 0: CRDT_DIFF_CLOCK stays
 *                     clear even when src's clock is ahead, because the clock is
 *                     not merged (:60).  The document adds nothing to summary.
 *   CRDT_DELTA_DELTA  - a dst-only key is removed only by an effective tombstone
 *                       of src whose dot D has not seen (:149-164); never because
 *                       S covers its dot.
 *                     - a src-only key is ADDED when D has not seen its dot and no
 *                       such tombstone removes it again in phase 2; when one does,
 *                       there is no record at all.
 *                     - a common key is UPDATED when D has not seen s's dot and the
 *                       key survives.
 *                     - a common key that phase 1 moves to s's dot and phase 2 then
 *                       removes (src holds (x, c) and a tombstone (x, c' >= c) of
 *                       it, D[x] < c) is recorded as removed WITH THE DOT IT HAD IN
 *                       DST, and has no upsert record.
 *                     - a tombstone of a key neither side holds leaves no record;
 *                       the document is still DELTA, and CRDT_DIFF_CLOCK is set iff
 *                       out.vv[d] != dst.vv[d].
 * Exchange: both directions from one read.  log_ab.removed is in a's layout and
 * log_ab.upserted in b's; log_ba.removed is in b's layout and log_ba.upserted in
 * a's.  Slots of a list at or past its count are unspecified; slots of other
 * documents are never written.  The bits are the same on every run.
 * Reported by crdt_ctx_sync: as the delta merge above (CRDT_E_ACTOR_RANGE on
 * Counter(s) at s == R and on any HasDot the chosen path evaluates at actor == R;
 * CRDT_E_CAPACITY on a live count above its slots, clamped).
 * Returned by the call (CRDT_E_INVALID): the delta merge's and the logged join's
 * argument errors together -- a NULL argument or required field (summary,
 * ups_kind and the kind pointers may be NULL); an n_docs or R mismatch; R out of
 * range; a tomb batch without offsets; two written arrays (outputs, log arrays,
 * kinds) starting at one address or overlapping per-document arrays; a written
 * array starting where an input array of the same kind (state, tombstones,
 * doc_actor) starts.
 * n_docs == 0 launches nothing that reads documents; summary, when given, is
 * zeroed.  Ordered after the context's previous call; no host sync, kernel nodes
 * only, capturable.  Workspace: the join's worklist, one word per document, sized
 * by crdt_ctx_reserve(max_docs, ..); CRDT_E_WORKSPACE when it would have to grow
 * during a graph capture; and the logged join's fixed 64 KB of summary partial
 * sums.  There is no _batch form. */
int crdt_awset_delta_join_log_async(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_replica* src,
                                    const crdt_awset_out* out, uint8_t* kind /* [n_docs] or NULL */,
                                    const crdt_merge_log* log, void* stream);
int crdt_awset_delta_exchange_log_async(crdt_ctx* ctx, const crdt_replica* a, const crdt_replica* b,
                                        const crdt_awset_out* out_ab, const crdt_awset_out* out_ba,
                                        uint8_t* kind_ab, uint8_t* kind_ba /* each [n_docs] or NULL */,
                                        const crdt_merge_log* log_ab, const crdt_merge_log* log_ba, void* stream);

/* ---- logged fold: the ordered fold with the log of its net effect --------------
 * The pair-form logged calls above need both replicas resident on one device.
 * The receiver of a delta message (crdt_awset_delta_extract_* packs one as a
 * crdt_src_batch) and an N-way convergence merge their sources with the fold;
 * this call is crdt_awset_fold_async with the log beside the merged state.
 * The merged state: out holds what crdt_awset_fold_async(mode, dst, srcs, out)
 * writes for the same inputs -- live entries, counts, offsets and clocks bit for
 * bit, document d at dst.offsets[d] + entry_off[doc_srcs[d]], slack unspecified.
 * The log is the net effect of the whole ordered fold: exactly
 * crdt_awset_diff_async(before = dst, after = out)'s answer, per document d.
 *   - removed: the live entries of dst[d] whose key is not live in out[d], in
 *     key order, with the dot they had in dst.
 *   - upserted: the live entries of out[d] whose key was not live in dst[d]
 *     (CRDT_DIFF_ADDED) or was live there under a different (actor, counter)
 *     (CRDT_DIFF_UPDATED), in key order, with their final dot.
 *   - flags[d] and summary as the diff writes them; CRDT_DIFF_CLOCK iff dst.vv
 *     and out.vv differ in some r < R.
 * Intermediate steps do not show: a key that one step removes and a later step
 * adds again under the same dot leaves no record (under another dot: one
 * UPDATED); a key added and later removed leaves none; a key updated and later
 * removed leaves one removed record, with dst's dot.
 * Layout: no scan over documents.  The removed list of d starts at
 * dst.offsets[d]; rem_offsets repeats dst.offsets (n_docs + 1 values) and its
 * capacity is dst's slots.  The upserted list of d starts at
 * entry_off[doc_srcs[d]]: ups_offsets[d] = entry_off[doc_srcs[d]] for d <= n_docs,
 * and its capacity is the sources' entry slots of the document.  That is enough:
 * an upserted key ends under a dot dst did not hold for it, a step gives a key
 * no other dot than the one its source's entry of that key carries, so every
 * upserted key is the key of some source entry of d, and distinct keys need
 * distinct entries.  ups_kind is indexed like ups_keys.  Each list read as
 * (offsets, counts, keys, actors, counters) is a valid crdt_tomb_batch.  Slots
 * of a document at or past its count are unspecified; slots of other documents
 * are never written.  No atomic decides a position: the bits are the same on
 * every run.
 * srcs->tomb_off == NULL: no tombstones.  CRDT_FOLD_AWSET ignores tombstones.
 * Reported by crdt_ctx_sync, exactly as the fold reports them:
 *   CRDT_E_ACTOR_RANGE  where Go evaluates HasDot / Counter at actor == R
 *   CRDT_E_CAPACITY     a live count above its slots (clamped)
 *   CRDT_E_WORKSPACE    a document too large for one wavefront (more than 64
 *                       entries in dst, in a source, in a source's tombstones or
 *                       after some step) needs more fold slots than
 *                       crdt_ctx_reserve was given, or a workspace would have to
 *                       grow during a graph capture
 * Returned by the call (CRDT_E_INVALID): a NULL argument or a NULL required field
 * (summary and ups_kind may be NULL); an n_docs or R mismatch; R out of range; a
 * bad mode; two written arrays starting at one address or overlapping
 * per-document arrays; a written array starting where an input array of the same
 * kind starts.
 * n_docs == 0 launches nothing that reads documents; summary, when given, is
 * zeroed.  Ordered after the context's previous call; no host sync, kernel nodes
 * only, capturable.  Workspace: the fold's (worklist and fold slots, sized by
 * crdt_ctx_reserve) and the logged join's fixed 64 KB of summary partial sums.
 * There is no _batch form. */
int crdt_awset_fold_log_async(crdt_ctx* ctx, int mode, const crdt_awset_batch* dst, const crdt_src_batch* srcs,
                              const crdt_awset_out* out, const crdt_merge_log* log, void* stream);

/* ---- logged local ops: Add / Del / AWSetDelta.Del with the log of their effect --
 * The logged calls above report what a merge changed.  The other half of what
 * changes a resident set is its own replica's ops; this call is
 * crdt_awset_apply_async with the log beside the new state, so that an index or a
 * view kept beside a replica follows local ops and merges alike.  The host cannot
 * derive the log from the op list: whether a Del hits a live key, which dot the
 * removed entry had and whether an Add lands on a live key depend on the state.
 * The state part: out and tomb_out hold what crdt_awset_apply_async writes for
 * the same arguments -- offsets, counts, live entries, clocks and tombstones bit
 * for bit, with its refusal rules and its tomb_out == NULL rule.
 * The log is crdt_awset_diff_async(before = state, after = out)'s answer, per
 * document d, in the inputs' own slot layouts (crdt_merge_log, above):
 *   - removed: the live entries of state[d] whose key is not live in out[d], in
 *     key order, with the dot they had in state.  They lie at state.offsets[d],
 *     rem_counts[d] of them; rem_offsets repeats state.offsets (n_docs + 1
 *     values); the capacity is the state's slots.
 *   - upserted: the live entries of out[d] whose key was not live in state[d]
 *     (CRDT_DIFF_ADDED) or was live there under a different (actor, counter)
 *     (CRDT_DIFF_UPDATED), in key order, with their new dot.  They lie at
 *     ops.op_off[d], ups_counts[d] of them; ups_offsets repeats op_off; the
 *     capacity is the document's ops, which is enough: a document upserts at most
 *     one entry per ADD op.  ups_kind is [n_ops] and indexed like ups_keys.
 *   - flags[d] and summary as the diff writes them.  CRDT_DIFF_CLOCK is set iff
 *     the document has an op that bumps the clock (ADD, DELTA_DEL): a DELTA_DEL
 *     call none of whose keys is live is CLOCK and nothing else.
 * Each list read as (offsets, counts, keys, actors, counters) is a valid
 * crdt_tomb_batch.  Slots of a document at or past its count are unspecified;
 * slots of other documents are never written.  No atomic decides a position: the
 * bits are the same on every run.
 * What "the diff's answer" means for an op list:
 *   1. an ADD of a key live in the state is one UPDATED record, not a removal and
 *      an add, also when a DEL of that key comes earlier in the list;
 *   2. an ADD that mints the very dot the state's entry already has (the state
 *      holds (actor, vv[actor] + k) and the k-th bump adds that key) is no
 *      record: the dots are compared, and UPDATED is not set;
 *   3. a key added and then deleted within the call that was not in the state
 *      leaves no record; nor does a DEL or an ineffective DELTA_DEL_KEY of an
 *      absent key.  A key of the state added and then deleted is one removed
 *      record, with the state's dot;
 *   4. tombstone changes are not part of this log: it is the diff of the entries.
 *      tomb_out is the record of Deleted.
 * A refused document (more than CRDT_MAX_OPS_PER_DOC ops, an unknown kind, a
 * DELTA_DEL_KEY outside a call or without a tomb_out, a bump with actor >= R)
 * comes out with count 0 and undefined slots, as in crdt_awset_apply_async; its
 * log is empty -- rem_counts[d] = ups_counts[d] = 0, flags[d] = 0 -- and it adds
 * nothing to summary.  Every other document's log is exact.
 * Reported by crdt_ctx_sync, exactly as crdt_awset_apply_async reports them:
 *   CRDT_E_ACTOR_RANGE  a bump with actor >= R
 *   CRDT_E_INVALID      a malformed op list
 *   CRDT_E_CAPACITY     a live count above its slots (clamped; the log is that
 *                       of the clamped prefix)
 * Returned by the call (CRDT_E_INVALID): everything crdt_awset_apply_async
 * refuses; a NULL log or a NULL required field (summary and ups_kind may be
 * NULL); two written arrays starting at one address; a written array starting
 * where an input array of the same kind starts.
 * n_docs == 0 launches nothing that reads documents; summary, when given, is
 * zeroed.  Ordered after the context's previous call; no host sync, kernel nodes
 * only, capturable.  Workspace: the logged join's fixed 64 KB of summary partial
 * sums, which the context owns from its creation: nothing grows during a capture.
 * There is no _batch form. */
int crdt_awset_apply_log_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_tomb_batch* tombs,
                               const crdt_op_batch* ops, const crdt_awset_out* out, const crdt_tomb_out* tomb_out,
                               const crdt_merge_log* log, void* stream);

/* ---- ingest sort ---------------------------------------------------------
 * The merge kernels need each document's keys strictly ascending; a producer
 * that packs Go maps (random iteration order) can hand them over unsorted and
 * sort on the device: out gets each document's live entries ordered by key, at
 * the same slot offsets as `in` (out must not alias in; capacity = in's
 * slots), counts = live counts, VVs copied.  A key twice in one document:
 * CRDT_E_DUP_KEY.  n_slots = in->offsets[n_docs] (host-known for async). */
int crdt_awset_sort_async(crdt_ctx* ctx, const crdt_awset_batch* in, uint32_t n_slots, const crdt_awset_out* out,
                          void* stream);
int crdt_awset_sort_batch(crdt_ctx* ctx, const crdt_awset_batch* in, const crdt_awset_out* out);

/* ---- opt-in tombstone GC -------------------------------
 * The reference never collects tombstones: (*AWSetDelta).gcDeleted is an
 * empty stub (awset-delta_test.go:67-77) whose comment states the intent,
 * "remove entries in s.Deleted for srcVersionVector".  Nothing calls this
 * implicitly.  Doc d keeps tombstone (k, x) unless stable[d*R..].HasDot(x)
 * (crdt-misc.go:28-34; actor >= R is "not covered", kept).  Pass per doc the
 * clock every replica has reached (the elementwise min of the replicas' VVs,
 * crdt_vv_min_async) so that no replica can still need the delete, or the
 * source VV of the last merge for the stub's literal reading.  Output at the
 * input's slot offsets, compacted, in key order. */
int crdt_tombstone_gc_async(crdt_ctx* ctx, const crdt_tomb_batch* tombs, uint32_t n_docs, uint32_t R,
                            const uint64_t* stable_vv, const crdt_tomb_out* out, void* stream);
/* dst[i] = min(dst[i], src[i]) for i < n (u64): causal stability across replicas. */
int crdt_vv_min_async(crdt_ctx* ctx, uint64_t* dst, const uint64_t* src, size_t n, void* stream);

/* ---- fixture dumps and debug text, host buffers -------
 * crdt_awset_format: Go's (AWSet).String() of doc `doc` (awset.go:163-171:
 * VersionVector.String crdt-misc.go:57-68, then "
  %s  %q" per entry in
 * sorted key order, Dot.String crdt-misc.go:17-19).  names[id] is the string
 * of key id (ids order-preserving); names == NULL prints "#<id>".  The VV
 * prints all R words.  Writes at most cap bytes including the NUL; *len = the
 * full length.
 * crdt_batch_dump: a self-checking binary image of a batch (live entries
 * only, compact offsets); buf == NULL: *len = the size needed.
 * crdt_batch_info / crdt_batch_undump: check an image and read its sizes, then
 * fill caller arrays (offsets n_docs+1, counts, n_entries entries, n_docs*R vv). */
int crdt_awset_format(const crdt_awset_batch* b, uint32_t doc, const char* const* names, char* buf, size_t cap,
                      size_t* len);
int crdt_batch_dump(const crdt_awset_batch* b, void* buf, size_t cap, size_t* len);
int crdt_batch_info(const void* buf, size_t len, uint32_t* n_docs, uint32_t* R, uint64_t* n_entries);
int crdt_batch_undump(const void* buf, size_t len, const crdt_awset_out* out);

/* ---- multi-GPU: the global causal context over RCCL (xGMI) --------------
 * Documents shard over GPUs with no exchange; the one collective is the
 * causal-context summary, R u64 per GPU, combined with
 * ncclAllReduce(ncclUint64, ncclMax).  RCCL is bound at run time (an RCCL
 * already mapped by the process is reused); without it these return
 * CRDT_E_RCCL.
 *
 * One process, several GPUs: per_gpu[i] is a context on its own device and
 * vv_R[i] a device pointer on that device holding its summary (e.g. the
 * output of crdt_causal_context_async); every vv_R[i] is replaced by the
 * elementwise max over all of them, and out_vv_R (host, may be NULL)
 * receives a copy.  Synchronous.  The communicators are built on the first
 * call and kept while the same contexts are passed in the same order.
 *
 * One process per GPU: rank 0 makes an id (crdt_comm_unique_id), every rank
 * receives it out of band and calls crdt_comm_init; then
 * crdt_context_allreduce_async reduces vv_R in place on `stream`. */
#define CRDT_COMM_ID_BYTES 128
int crdt_global_context_allreduce(crdt_ctx* const* per_gpu, int n_gpus, uint64_t* const* vv_R, uint32_t R,
                                  uint64_t* out_vv_R);
int crdt_comm_unique_id(uint8_t* id /* [CRDT_COMM_ID_BYTES] */);
int crdt_comm_init(crdt_ctx* ctx, int n_ranks, int rank, const uint8_t* id);
int crdt_context_allreduce_async(crdt_ctx* ctx, uint64_t* vv_R, uint32_t R, void* stream);

/* ---- host buffers, synchronous: copies in, runs, copies out -------------
 * Host arrays from crdt_host_alloc (page-locked) cross PCIe by DMA at full
 * link rate; pageable arrays work too, staged by the HIP runtime.  A caller
 * packing many batches keeps its page-locked arrays and reuses them. */
int crdt_host_alloc(size_t bytes, void** out);
void crdt_host_free(void* p);
int crdt_awset_join_batch(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_awset_batch* src,
                          const crdt_awset_out* out);
int crdt_awset_exchange_batch(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b,
                              const crdt_awset_out* out_ab, const crdt_awset_out* out_ba);
int crdt_awset_fold_batch(crdt_ctx* ctx, int mode, const crdt_awset_batch* dst, const crdt_src_batch* srcs,
                          const crdt_awset_out* out);
/* Host arrays in and out: the slot layout is checked on the host, the key order
 * of source entries and tombstones on the device (CRDT_E_UNSORTED), and only
 * the packed live prefix of each output array is downloaded. */
int crdt_awset_delta_extract_batch(crdt_ctx* ctx, const crdt_src_batch* srcs, const uint64_t* peer_vv,
                                   const crdt_delta_out* out);

/* ---- host-side validation of a packed batch (no GPU) -------------------- */
int crdt_validate_batch(const crdt_awset_batch* b);
int crdt_validate_src_batch(const crdt_src_batch* s);
/* tombstones of n_docs documents: monotone offsets, counts <= slots, keys
 * strictly ascending per document (crdt_awset_apply_batch runs it first). */
int crdt_validate_tomb_batch(const crdt_tomb_batch* t, uint32_t n_docs);

#ifdef __cplusplus
}
#endif
#endif /* CRDTGPU_H */
