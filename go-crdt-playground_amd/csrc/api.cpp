// C ABI of the engine (include/crdtgpu.h): context, validation, launches and
// the synchronous host-buffer path used by the cgo drop-in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/crdtgpu.h"
#include "api_args.hpp"
#include "crdt_device.hpp"
#include "headroom.hpp"
#include "replica.hpp"

namespace crdt {
hipError_t launch_join(const BatchView& dst, const BatchView& src, const OutView& out, const OutView* out2,
                       const Work& wk, uint32_t docs_per_wave, bool nt_stores, bool stage_stores, uint32_t slab_blocks,
                       uint32_t block_grid, bool no_large,
                       const TileWork* tw, uint32_t n_cu, hipStream_t stream);
hipError_t launch_fold(int mode, const BatchView& dst, const SrcView& sb, const OutView& out, const Scratch& scr,
                       const Work& wk, uint32_t block_grid, bool lean_first, hipStream_t stream);
uint32_t tile_positions(uint32_t shape);
hipError_t sort_storage(uint32_t n_docs, uint32_t n_slots, size_t* bytes);
struct OrderRanges {  // pack.hip: one list of key ranges whose order is checked
    const uint32_t* off;
    const uint32_t* cnt;
    uint32_t n;
    const uint64_t* keys;
};
hipError_t launch_check_order(const void* sets, uint32_t n_sets, uint32_t* status, uint32_t n_cu, hipStream_t stream);
hipError_t launch_pack(uint32_t nout, const OutView* in, uint32_t* const* poff, uint32_t* const* host_off,
                       const OutView* out, uint32_t n, uint32_t R, const uint32_t* gate, uint32_t* host_status,
                       uint32_t n_cu, hipStream_t stream);
hipError_t launch_sort(const BatchView& in, uint32_t n_slots, const OutView& out, void* temp, size_t temp_bytes,
                       uint32_t* ends, uint32_t* idx, uint32_t* status, uint32_t n_cu, hipStream_t stream);
hipError_t launch_apply(const BatchView& st, const TombView& tb, const ApplyOps& ops, const OutView& out,
                        const TombOut& tout, bool has_tout, const Work& wk, uint32_t n_cu, hipStream_t stream);
hipError_t launch_extract(const SrcView& sv, const uint64_t* peer, const DeltaOutView& out, uint32_t* gcnt_e,
                          uint32_t* gcnt_t, const Work& wk, uint32_t n_cu, hipStream_t stream);
hipError_t launch_has(const HasView& sv, const HasQueries& qv, const HasOut& out, uint32_t* status,
                      const uint32_t* gate, uint32_t n_cu, hipStream_t stream);
hipError_t launch_compare(const BatchView& a, const BatchView& b, uint32_t mask, const CompareOutView& out,
                          uint32_t* fw, uint32_t* status, const uint32_t* gate, uint32_t n_cu, hipStream_t stream);
hipError_t launch_select(const BatchView& st, const uint32_t* idx, const uint32_t* n_idx, uint32_t n_out,
                         uint32_t out_slots, const OutView& out, uint32_t* status, uint32_t n_cu,
                         hipStream_t stream);
hipError_t launch_scatter(const BatchView& st, const BatchView& sub, const uint32_t* idx, const uint32_t* n_idx,
                          uint32_t out_slots, const OutView& out, uint32_t* inv, uint32_t* parts, uint32_t* status,
                          uint32_t n_cu, hipStream_t stream);
size_t diff_parts_bytes();
hipError_t launch_diff(const BatchView& before, const BatchView& after, uint32_t rem_slots, uint32_t ups_slots,
                       const DiffOutView& out, uint32_t* fw, uint32_t* parts, uint32_t* status, const uint32_t* gate,
                       uint32_t n_cu, hipStream_t stream);
hipError_t launch_sources(const SourcesArgs& s, uint32_t* parts_e, uint32_t* parts_t, uint32_t* status, uint32_t n_cu,
                          hipStream_t stream);
hipError_t launch_replica(const ReplicaArgs& a, uint32_t* inv, uint32_t* parts_e, uint32_t* parts_t, uint32_t* status,
                          uint32_t n_cu, hipStream_t stream);
hipError_t launch_delta_pair(const PairSide& A, const PairSide& B, const OutView& out_ab, const OutView* out_ba,
                             uint8_t* kind_ab, uint8_t* kind_ba, const Work& wk, uint32_t block_grid,
                             hipStream_t stream);
size_t join_log_parts_bytes();
hipError_t launch_join_log(const BatchView& A, const BatchView& B, const OutView& out_ab, const OutView* out_ba,
                           const MergeLogView& log_ab, const MergeLogView* log_ba, const Work& wk, uint32_t* parts,
                           uint32_t block_grid, hipStream_t stream);
hipError_t launch_delta_pair_log(const PairSide& A, const PairSide& B, const OutView& out_ab, const OutView* out_ba,
                                 uint8_t* kind_ab, uint8_t* kind_ba, const MergeLogView& log_ab,
                                 const MergeLogView* log_ba, const Work& wk, uint32_t* parts, uint32_t block_grid,
                                 hipStream_t stream);
hipError_t launch_fold_log(int mode, const BatchView& dst, const SrcView& sb, const OutView& out, const Scratch& scr,
                           const MergeLogView& lg, const Work& wk, uint32_t* parts, uint32_t block_grid,
                           hipStream_t stream);
hipError_t launch_apply_log(const BatchView& st, const TombView& tb, const ApplyOps& ops, const OutView& out,
                            const TombOut& tout, bool has_tout, const MergeLogView& lg, const Work& wk,
                            uint32_t* parts, uint32_t n_cu, hipStream_t stream);
hipError_t launch_digest(const HasView& st, const HasView& tb, const uint64_t* vv, uint32_t R, uint64_t* digest,
                         uint32_t* status, uint32_t n_cu, hipStream_t stream);
hipError_t launch_digest_idx(const HasView& st, const HasView& tb, const uint64_t* vv, uint32_t R, const uint32_t* idx,
                             const uint32_t* n_idx, uint32_t n_max, uint32_t n_digest, uint32_t mode, uint64_t* digest,
                             uint32_t* status, uint32_t n_cu, hipStream_t stream);
hipError_t launch_digest_diff(const uint64_t* mine, const uint64_t* theirs, uint32_t n, uint32_t mask,
                              const CompareOutView& out, uint32_t* fw, const uint32_t* gate, uint32_t n_cu,
                              hipStream_t stream);
hipError_t launch_digest_tree(const uint64_t* digest, uint32_t n_docs, uint64_t* tree, bool fuse, hipStream_t stream);
hipError_t launch_digest_tree_children(const uint64_t* level, uint32_t n_level, const uint32_t* parents,
                                       const uint32_t* n_parents, uint32_t n_max, uint64_t* out, uint32_t* status,
                                       hipStream_t stream);
size_t digest_tree_diff_parts(uint32_t n_max);
hipError_t launch_digest_tree_diff(const uint64_t* mine_level, uint32_t n_level, const uint64_t* theirs,
                                   const uint32_t* parents, const uint32_t* n_parents, uint32_t n_max, uint32_t leaf,
                                   uint32_t mask, uint32_t* idx_out, uint8_t* flags_out, uint32_t* n_out,
                                   uint32_t out_max, uint32_t* summary, uint32_t* parts, uint32_t* status,
                                   hipStream_t stream);
hipError_t launch_vv_max(uint64_t* dst, const uint64_t* src, size_t n, hipStream_t stream);
hipError_t launch_vv_min(uint64_t* dst, const uint64_t* src, size_t n, hipStream_t stream);
hipError_t launch_tomb_gc(const TombView& tb, uint32_t n_docs, uint32_t R, const uint64_t* stable, const TombOut& out,
                          uint32_t n_cu, hipStream_t stream);
hipError_t launch_reset_work(uint32_t* ws, hipStream_t stream);
hipError_t launch_context(const uint64_t* vv, uint32_t n_docs, uint32_t R, uint64_t* part, uint32_t n_part,
                          uint64_t* out, hipStream_t stream);
hipError_t launch_gen_pair(uint64_t seed, uint32_t n_docs, const OutView& A, const OutView& B, hipStream_t stream);
struct SrcOutView {
    uint32_t* doc_srcs;
    uint32_t* src_actor;
    uint64_t* vv;
    uint32_t* entry_off;
    uint64_t* keys;
    uint32_t* actors;
    uint64_t* counters;
    uint32_t* tomb_off;
    uint64_t* tkeys;
    uint32_t* tactors;
    uint64_t* tcounters;
};
hipError_t launch_gen_delta(uint64_t seed, uint32_t n_docs, uint32_t R, uint32_t M, const OutView& D,
                            const SrcOutView& S, hipStream_t stream);
hipError_t launch_gen_replicas(uint64_t seed, uint32_t n_docs, uint32_t P, uint32_t E, const OutView& D,
                               const SrcOutView& S, hipStream_t stream);
hipError_t launch_gen_zipf(uint64_t seed, uint32_t n_docs, const uint32_t* offsets, const OutView& A,
                           const OutView& B, hipStream_t stream);
uint32_t host_zipf_doc_size(uint64_t seed, uint32_t d);
hipError_t launch_clock_probe(uint64_t* out, uint32_t n_cu, hipStream_t stream);
hipError_t launch_probe(int kind, const void* a, void* b, size_t n16, uint32_t n_cu, uint32_t blocks_per_cu, bool slab,
                        hipStream_t stream);
}  // namespace crdt

using namespace crdt;

namespace {

constexpr uint32_t kCtxParts = 1024;

// Device buffer that only grows.  A buffer it outgrows is retired, not freed:
// a HIP graph captured earlier may still name it, so retired buffers live
// until crdt_ctx_destroy.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    std::vector<void*>* retired = nullptr;
    int reserve(size_t want) {
        if (want <= bytes) return CRDT_OK;
        if (p) {
            if (retired)
                retired->push_back(p);
            else
                (void)hipFree(p);
        }
        p = nullptr;
        bytes = 0;
        if (hipMalloc(&p, want) != hipSuccess) return CRDT_E_NOMEM;
        bytes = want;
        return CRDT_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T* as(size_t byte_off = 0) const {
        return reinterpret_cast<T*>(static_cast<char*>(p) + byte_off);
    }
};

// The page-locked blocks crdt_host_alloc made (base -> size): a *_batch call
// whose input arrays all lie in one of them is staged by ONE copy of the span
// they cover (Stager), because each runtime H2D copy call costs the host 1-7
// ms before its DMA is even submitted, whatever its size
// (profiles/r05i_boundary_timeline.txt), while the span moves at PCIe rate.
// Each block also keeps its device-side address: a host-path call whose outputs
// lie in such blocks has its packed results written there by the gather kernel
// (pack.hip) instead of copied back by runtime copy calls.
struct HostBlock {
    size_t size;
    uintptr_t dev;  // hipHostGetDevicePointer of the base (0: none)
};
std::mutex g_host_mu;
std::map<uintptr_t, HostBlock> g_host_blocks;

bool host_block(const void* p, uintptr_t& base, size_t& size, uintptr_t* dev = nullptr) {
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host_blocks.upper_bound(a);
    if (it == g_host_blocks.begin()) return false;
    --it;
    if (a >= it->first + it->second.size) return false;
    base = it->first;
    size = it->second.size;
    if (dev) *dev = it->second.dev;
    return true;
}

// The device address of host range [p, p + bytes) when all of it lies in one
// crdt_host_alloc block (0 otherwise).
uintptr_t host_dev_addr(const void* p, size_t bytes) {
    uintptr_t base = 0, dev = 0;
    size_t size = 0;
    if (!p || !host_block(p, base, size, &dev) || !dev) return 0;
    const uintptr_t a = (uintptr_t)p;
    if (a + bytes > base + size) return 0;
    return dev + (a - base);
}


}  // namespace

struct crdt_ctx {
    int device = 0;
    int n_cu = 256;
    // [0,64): per-call counters {wl_count, wl_head, -, ..., chunk_ctr[8] at 32}
    // zeroed by every call; [64,68): status word, cleared by crdt_ctx_sync.
    DevBuf ws;
    DevBuf worklist;
    DevBuf defer;  // folds: documents the lean pass leaves to the general kernel
    DevBuf spill_parts;  // in-place replica scatter: the spill scan's partial sums, one word per 1,024 documents
    DevBuf parts;
    DevBuf scratch;  // fold block path ping-pong: keys | actors | counters
    // large-document join tiles (tile.hip): descriptors + look-back words for
    // tile_cap tiles, per-slot and per-run tile counts for the worklist
    DevBuf tile_desc, tile_geo, tile_flags, tile_slot, tile_run;
    DevBuf sort_tmp, sort_idx, sort_ends;  // ingest sort (sort.hip)
    // crdt_ctx_set_option("join_tile_capacity"): 2^22 tiles (235 MB of tile workspace, on
    // first use); config 4 needs 1.035 M tiles of 1,024 positions, 2.07 M of 512
    uint32_t tile_cap = 1u << 22;
    bool join_tiles = true;                   // crdt_ctx_set_option("join_tiles")
    uint32_t tile_shape = 9;                  // crdt_ctx_set_option("join_tile_shape")
    bool tile_nt_stores = true;               // crdt_ctx_set_option("join_tile_nt_stores")
    uint32_t tile_split_bpc = 4;              // crdt_ctx_set_option("join_tile_split_blocks_per_cu")
    uint32_t tile_shards = 8;                 // crdt_ctx_set_option("join_tile_dispensers")
    uint32_t tile_max_passes = 256;           // crdt_ctx_set_option("join_tile_max_passes")
    // the tiles of the join this host-path call is about to launch, counted from
    // its host arrays (0: unknown, an _async call: bounded instead, join_common)
    uint64_t call_tiles = 0;
    size_t scratch_slots = 0;
    uint32_t max_doc_entries = 0xFFFFFFFFu;  // caller's promise (crdt_ctx_set_max_doc_entries)
    uint32_t join_docs_per_wave = 8;          // crdt_ctx_set_option("join_docs_per_wave")
    bool join_nt_stores = true;               // crdt_ctx_set_option("join_nt_stores")
    bool join_stage_stores = true;            // crdt_ctx_set_option("join_stage_stores")
    uint32_t join_slab_per_cu = 0;            // crdt_ctx_set_option("join_slab_blocks_per_cu"): 0 = blocks in order
    bool fold_lean_first = true;              // crdt_ctx_set_option("fold_lean_first")
    bool digest_tree_fuse = true;             // crdt_ctx_set_option("digest_tree_fuse")
    uint32_t probe_blocks_per_cu = 16;        // crdt_ctx_set_option("probe_blocks_per_cu")
    bool probe_slab = false;                  // crdt_ctx_set_option("probe_slab")
    bool pack_outputs = false;                // crdt_ctx_set_option("pack_batch_outputs")
    bool span_staging = true;                 // crdt_ctx_set_option("span_staging")
    // staging for the *_batch host path: per-array buffers, and the device image
    // of the part of one crdt_host_alloc block a call's inputs cover (Stager)
    DevBuf stage[48];
    DevBuf span_img;
    // set by a *_batch call around its merge launch: the merge's first kernel is
    // gated on the status word its order checks wrote (Work::gate)
    bool call_gate = false;
    // set by a *_batch call whose host arrays show no document above 64 live
    // entries on a side: the join launches no large-document path at all
    bool call_small = false;
    // page-locked word the packed-output gather copies the status word into, so
    // a host-path call reads its verdict without another runtime call
    uint32_t* host_status = nullptr;
    hipStream_t stream = nullptr;
    // Ordering of the shared workspace across streams: the last call's stream
    // and an event recorded after its launches.  A call on another stream
    // waits for that event first (see enter()).
    hipEvent_t last_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool has_last = false;
    std::vector<void*> retired;  // outgrown workspace buffers, freed at destroy
    void* comm = nullptr;        // RCCL communicator (comm.cpp)
    void* comm_group = nullptr;  // single-process group it belongs to (comm.cpp)
};

void crdt_internal_comm_release(crdt_ctx* ctx);
int crdt_internal_device(crdt_ctx* ctx) { return ctx->device; }
hipStream_t crdt_internal_stream(crdt_ctx* ctx) { return ctx->stream; }
void** crdt_internal_comm(crdt_ctx* ctx) { return &ctx->comm; }
void** crdt_internal_comm_group(crdt_ctx* ctx) { return &ctx->comm_group; }
// Order stream s after the context's last call (when that ran on another stream).
int crdt_internal_order(crdt_ctx* ctx, hipStream_t s) {
    if (ctx->has_last && ctx->last_stream != s && hipStreamWaitEvent(s, ctx->last_ev, 0) != hipSuccess)
        return CRDT_E_HIP;
    return CRDT_OK;
}

namespace {

int hip_err(hipError_t e) { return e == hipSuccess ? CRDT_OK : CRDT_E_HIP; }

int set_device(crdt_ctx* ctx) { return hip_err(hipSetDevice(ctx->device)); }

uint32_t block_grid(const crdt_ctx* ctx) { return (uint32_t)ctx->n_cu * 2u; }

Work make_work(crdt_ctx* ctx) {
    Work w;
    w.wl_count = ctx->ws.as<uint32_t>(0);
    w.wl_head = ctx->ws.as<uint32_t>(4);
    w.status = ctx->ws.as<uint32_t>(64);
    w.chunk_ctr = ctx->ws.as<uint32_t>(32);
    w.worklist = ctx->worklist.as<uint32_t>();
    w.defer_count = ctx->ws.as<uint32_t>(8);
    w.defer = ctx->defer.as<uint32_t>();
    w.gate = ctx->call_gate ? w.status : nullptr;
    return w;
}

// Start of a call that uses the context's shared workspace (worklist,
// counters, scratch, status word, context partials) on stream s.  Work of an
// earlier call on a different stream is ordered before it with a stream wait
// on that call's event.  While s is capturing a graph no wait is recorded
// (the caller orders the capture; the capture itself must not allocate, see
// grow()).
int enter(crdt_ctx* ctx, hipStream_t s, bool& capturing) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) return CRDT_E_HIP;
    capturing = st != hipStreamCaptureStatusNone;
    if (!capturing && ctx->has_last && ctx->last_stream != s)
        if (hipStreamWaitEvent(s, ctx->last_ev, 0) != hipSuccess) return CRDT_E_HIP;
    return CRDT_OK;
}

// End of such a call: its launches are what the next call on another stream waits for.
int leave(crdt_ctx* ctx, hipStream_t s, bool capturing, int rc) {
    if (rc != CRDT_OK || capturing) return rc;
    if (hipEventRecord(ctx->last_ev, s) != hipSuccess) return CRDT_E_HIP;
    ctx->last_stream = s;
    ctx->has_last = true;
    return CRDT_OK;
}

// Grow a workspace buffer; refused while capturing (an allocation would break
// the capture, and the graph would keep the old address).
int grow(DevBuf& b, size_t want, bool capturing) {
    if (want <= b.bytes) return CRDT_OK;
    if (capturing) return CRDT_E_WORKSPACE;
    return b.reserve(want);
}

int reserve_worklist(crdt_ctx* ctx, uint32_t n_docs) {
    // (two words at least: the replica scatter's two partial sums of a one-document replica)
    int rc = ctx->worklist.reserve(std::max<size_t>((size_t)n_docs, 2) * sizeof(uint32_t));
    if (rc == CRDT_OK) rc = ctx->defer.reserve(std::max<size_t>((size_t)n_docs, 2) * sizeof(uint32_t));
    if (rc == CRDT_OK) rc = ctx->spill_parts.reserve(((size_t)n_docs / 1024 + 1) * sizeof(uint32_t));
    return rc;
}

int reserve_scratch(crdt_ctx* ctx, uint64_t slots) {
    if (slots <= ctx->scratch_slots) return CRDT_OK;
    int rc = ctx->scratch.reserve(slots * 20 + 64);
    if (rc == CRDT_OK) ctx->scratch_slots = slots;
    return rc;
}

BatchView view(const crdt_awset_batch* b) {
    return BatchView{b->n_docs, b->R, b->offsets, b->counts, b->keys, b->actors, b->counters, b->vv};
}

OutView view(const crdt_awset_out* o) {
    return OutView{o->offsets, o->counts, o->keys, o->actors, o->counters, o->vv};
}

SrcView view(const crdt_src_batch* s) {
    return SrcView{s->n_docs,    s->R,       s->doc_srcs, s->src_actor, s->vv,    s->entry_off, s->keys,
                   s->actors,    s->counters, s->tomb_off, s->tkeys,     s->tactors, s->tcounters};
}

TombView view(const crdt_tomb_batch* t) {  // NULL: no tombstones
    return t ? TombView{t->offsets, t->counts, t->keys, t->actors, t->counters} : TombView{};
}

TombOut view(const crdt_tomb_out* t) {  // NULL: not written
    return t ? TombOut{t->offsets, t->counts, t->keys, t->actors, t->counters} : TombOut{};
}

MergeLogView view(const crdt_merge_log* l) {
    return MergeLogView{l->flags,      l->summary,      l->rem_offsets, l->rem_counts, l->rem_keys,
                        l->rem_actors, l->rem_counters, l->ups_offsets, l->ups_counts, l->ups_keys,
                        l->ups_actors, l->ups_counters, l->ups_kind};
}

DeltaOutView view(const crdt_delta_out* o, bool kind) {  // kind: the call writes out->kind
    return DeltaOutView{o->doc_srcs, o->src_actor, o->vv,    o->entry_off, o->keys,      o->actors,
                        o->counters, o->tomb_off,  o->tkeys, o->tactors,   o->tcounters, kind ? o->kind : nullptr};
}

HasView has_view(const crdt_awset_batch* b) {
    return HasView{b->n_docs, b->offsets, b->counts, b->keys, b->actors, b->counters};
}

HasView has_view(const crdt_tomb_batch* t, uint32_t n_docs) {  // NULL: no tombstones
    return t ? HasView{n_docs, t->offsets, t->counts, t->keys, t->actors, t->counters}
             : HasView{n_docs, nullptr, nullptr, nullptr, nullptr, nullptr};
}

SrcCols cols(const crdt_awset_batch* b) { return SrcCols{b->offsets, b->counts, b->keys, b->actors, b->counters}; }

SrcCols cols(const crdt_tomb_batch* t) {  // NULL: no tombstones
    return t ? SrcCols{t->offsets, t->counts, t->keys, t->actors, t->counters} : SrcCols{};
}

PairSide pair_side(const crdt_awset_batch* st, const crdt_tomb_batch* t, const uint32_t* doc_actor, uint32_t actor) {
    PairSide ps{};
    ps.st = view(st);
    ps.tb = view(t);
    ps.doc_actor = doc_actor;
    ps.actor = actor;
    return ps;
}

RepSide rep_side(const crdt_replica* r) {
    RepSide s{};
    s.n_docs = r->state->n_docs;
    s.actor = r->actor;
    s.e = cols(r->state);
    s.t = cols(r->tombs);
    s.vv = r->state->vv;
    s.doc_actor = r->doc_actor;
    return s;
}

// One call that uses the context's shared workspace on a stream: the constructor
// selects the device and enters (enter()), need() grows a workspace buffer, end()
// leaves (leave()).  Every step is skipped once rc is an error; a return that
// passes end() by records no event.
struct Call {
    crdt_ctx* ctx;
    hipStream_t s;
    bool cap = false;  // s is capturing a graph
    int rc;
    Call(crdt_ctx* c, void* stream) : ctx(c), s((hipStream_t)stream), rc(set_device(c)) {
        if (rc == CRDT_OK) rc = enter(ctx, s, cap);
    }
    void need_bytes(DevBuf& b, size_t bytes) {
        if (rc == CRDT_OK) rc = grow(b, bytes, cap);
    }
    void need(DevBuf& b, size_t words) { need_bytes(b, std::max<size_t>(words, 1) * sizeof(uint32_t)); }
    int end(int launch_rc) { return leave(ctx, s, cap, launch_rc); }
    int end(hipError_t e) { return end(hip_err(e)); }
};

}  // namespace

extern "C" {

int crdt_abi_version(void) { return CRDTGPU_ABI_VERSION; }

const char* crdt_strerror(int code) {
    switch (code) {
        case CRDT_OK: return "ok";
        case CRDT_E_INVALID: return "invalid argument";
        case CRDT_E_ACTOR_RANGE: return "dot actor == len(VersionVector): the reference panics (index out of range)";
        case CRDT_E_UNSORTED: return "keys of a document are not strictly ascending";
        case CRDT_E_CAPACITY: return "live count exceeds the document's slots";
        case CRDT_E_HIP: return "HIP runtime error";
        case CRDT_E_NOMEM: return "device allocation failed";
        case CRDT_E_WORKSPACE: return "fold scratch too small: call crdt_ctx_reserve with the output slot count";
        case CRDT_E_RCCL: return "RCCL unavailable or a collective failed";
        case CRDT_E_DUP_KEY: return "a key appears twice in one document";
        default: return "unknown error";
    }
}

int crdt_ctx_create(int device, crdt_ctx** out) {
    if (!out) return CRDT_E_INVALID;
    *out = nullptr;
    crdt_ctx* ctx = new (std::nothrow) crdt_ctx();
    if (!ctx) return CRDT_E_NOMEM;
    ctx->device = device;
    for (DevBuf* b : {&ctx->ws, &ctx->worklist, &ctx->defer, &ctx->spill_parts, &ctx->parts, &ctx->scratch, &ctx->tile_desc, &ctx->tile_geo, &ctx->tile_flags,
                      &ctx->tile_slot, &ctx->tile_run, &ctx->sort_tmp, &ctx->sort_idx, &ctx->sort_ends})
        b->retired = &ctx->retired;
    for (auto& b : ctx->stage) b.retired = &ctx->retired;
    ctx->span_img.retired = &ctx->retired;
    int rc = set_device(ctx);
    hipDeviceProp_t prop;
    if (rc == CRDT_OK && hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->n_cu = prop.multiProcessorCount;
    if (rc == CRDT_OK) rc = ctx->ws.reserve(128);
    if (rc == CRDT_OK) rc = hip_err(hipMemset(ctx->ws.p, 0, 128));
    if (rc == CRDT_OK) rc = reserve_worklist(ctx, 1024);
    if (rc == CRDT_OK) rc = ctx->parts.reserve((size_t)kCtxParts * CRDT_MAX_R * sizeof(uint64_t));
    if (rc == CRDT_OK) rc = hip_err(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    if (rc == CRDT_OK) rc = hip_err(hipEventCreateWithFlags(&ctx->last_ev, hipEventDisableTiming));
    if (rc == CRDT_OK && hipHostMalloc(reinterpret_cast<void**>(&ctx->host_status), 64, hipHostMallocDefault) != hipSuccess)
        ctx->host_status = nullptr;  // (then the host path reads the status word back instead)
    if (rc != CRDT_OK) {
        crdt_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return CRDT_OK;
}

void crdt_ctx_destroy(crdt_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // drain every queued call (an all-reduce on the communicator included)
    // before the communicator and the workspaces go away
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->last_ev) (void)hipEventSynchronize(ctx->last_ev);
    crdt_internal_comm_release(ctx);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->last_ev) (void)hipEventDestroy(ctx->last_ev);
    for (void* p : ctx->retired) (void)hipFree(p);
    ctx->retired.clear();
    if (ctx->host_status) (void)hipHostFree(ctx->host_status);
    ctx->ws.release();
    ctx->worklist.release();
    ctx->defer.release();
    ctx->spill_parts.release();
    ctx->parts.release();
    ctx->scratch.release();
    for (DevBuf* b : {&ctx->tile_desc, &ctx->tile_geo, &ctx->tile_flags, &ctx->tile_slot, &ctx->tile_run,
                      &ctx->sort_tmp, &ctx->sort_idx, &ctx->sort_ends})
        b->release();
    for (auto& b : ctx->stage) b.release();
    ctx->span_img.release();
    delete ctx;
}

int crdt_ctx_reserve(crdt_ctx* ctx, uint32_t max_docs, uint64_t max_fold_slots) {
    if (!ctx) return CRDT_E_INVALID;
    int rc = set_device(ctx);
    if (rc == CRDT_OK) rc = reserve_worklist(ctx, max_docs);
    if (rc == CRDT_OK) rc = reserve_scratch(ctx, max_fold_slots);
    return rc;
}

int crdt_ctx_set_max_doc_entries(crdt_ctx* ctx, uint32_t max_entries) {
    if (!ctx) return CRDT_E_INVALID;
    ctx->max_doc_entries = max_entries;
    return CRDT_OK;
}

int crdt_ctx_set_option(crdt_ctx* ctx, const char* name, int64_t value) {
    if (!ctx || !name) return CRDT_E_INVALID;
    if (!strcmp(name, "join_docs_per_wave")) {
        if (value != 1 && value != 2 && value != 4 && value != 8 && value != 16) return CRDT_E_INVALID;
        ctx->join_docs_per_wave = (uint32_t)value;
        return CRDT_OK;
    }
    if (!strcmp(name, "join_tile_capacity")) {  // tiles per pass of the tile path (workspace: 56 B a tile)
        if (value < 1 || value > (1ll << 28)) return CRDT_E_INVALID;
        ctx->tile_cap = (uint32_t)value;
        return CRDT_OK;
    }
    if (!strcmp(name, "join_tile_max_passes")) {  // more tiles than passes x capacity -> block kernel
        if (value < 1 || value > 65536) return CRDT_E_INVALID;
        ctx->tile_max_passes = (uint32_t)value;
        return CRDT_OK;
    }
    if (!strcmp(name, "join_tile_shape")) {  // threads x positions: look-back per tile 0: 512x4, 1: 256x4, 2: 256x8,
                                             // 3: 1024x2; deferred by a tile 4: 256x4, 5: 512x2, 6: 256x8, 7: 128x8,
                                             // and aligned store windows 8: 256x4, 9: 512x2 (default), 10: 256x2
        if (value < 0 || value > 10) return CRDT_E_INVALID;
        ctx->tile_shape = (uint32_t)value;
        return CRDT_OK;
    }
    if (!strcmp(name, "join_tile_dispensers")) {  // tile dispenser words: 1, or 8 (one per XCD, tile.hip)
        if (value != 1 && value != 8) return CRDT_E_INVALID;
        ctx->tile_shards = (uint32_t)value;
        return CRDT_OK;
    }
    if (!strcmp(name, "join_tile_split_blocks_per_cu")) {  // grid of the tile plan's merge-path search
        if (value < 1 || value > 64) return CRDT_E_INVALID;
        ctx->tile_split_bpc = (uint32_t)value;
        return CRDT_OK;
    }
    if (!strcmp(name, "join_tile_nt_stores")) {
        ctx->tile_nt_stores = value != 0;
        return CRDT_OK;
    }
    if (!strcmp(name, "join_tiles")) {  // 0: large documents one workgroup each (join_block_kernel)
        ctx->join_tiles = value != 0;
        return CRDT_OK;
    }
    if (!strcmp(name, "pack_batch_outputs")) {  // *_batch joins / exchanges / folds: live entries only, packed
        ctx->pack_outputs = value != 0;
        return CRDT_OK;
    }
    if (!strcmp(name, "span_staging")) {  // *_batch inputs in one crdt_host_alloc block: one copy of their span
        ctx->span_staging = value != 0;
        return CRDT_OK;
    }
    if (!strcmp(name, "probe_slab")) {  // bandwidth probes: one contiguous slab per workgroup
        ctx->probe_slab = value != 0;
        return CRDT_OK;
    }
    if (!strcmp(name, "probe_blocks_per_cu")) {
        if (value < 1 || value > 64) return CRDT_E_INVALID;
        ctx->probe_blocks_per_cu = (uint32_t)value;
        return CRDT_OK;
    }
    if (!strcmp(name, "fold_lean_first")) {  // both fold modes: lean slot-walk pass first, the rest deferred (fold.hip, launch_fold)
        ctx->fold_lean_first = value != 0;
        return CRDT_OK;
    }
    if (!strcmp(name, "digest_tree_fuse")) {  // 0: one launch per level up to the root (digest_tree.hip)
        ctx->digest_tree_fuse = value != 0;
        return CRDT_OK;
    }
    if (!strcmp(name, "join_nt_stores")) {
        ctx->join_nt_stores = value != 0;
        return CRDT_OK;
    }
    if (!strcmp(name, "join_stage_stores")) {
        ctx->join_stage_stores = value != 0;
        return CRDT_OK;
    }
    if (!strcmp(name, "join_slab_blocks_per_cu")) {  // slab order of the wave kernel's blocks (SlabMap G per CU)
        if (value < 0 || value > 64) return CRDT_E_INVALID;
        ctx->join_slab_per_cu = (uint32_t)value;
        return CRDT_OK;
    }
    return CRDT_E_INVALID;
}

int crdt_ctx_sync(crdt_ctx* ctx, void* stream) {
    if (!ctx) return CRDT_E_INVALID;
    int rc = set_device(ctx);
    if (rc != CRDT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipStreamSynchronize(s) != hipSuccess) return CRDT_E_HIP;
    // the status word is shared: also wait for the last call if it ran elsewhere
    if (ctx->has_last && ctx->last_stream != s && hipEventSynchronize(ctx->last_ev) != hipSuccess) return CRDT_E_HIP;
    uint32_t status = 0;
    if (hipMemcpy(&status, ctx->ws.as<uint32_t>(64), sizeof(status), hipMemcpyDeviceToHost) != hipSuccess)
        return CRDT_E_HIP;
    if (status) {
        if (hipMemset(ctx->ws.as<uint32_t>(64), 0, sizeof(uint32_t)) != hipSuccess) return CRDT_E_HIP;
        if (status & kErrUnsorted) return CRDT_E_UNSORTED;
        if (status & kErrActorRange) return CRDT_E_ACTOR_RANGE;
        if (status & kErrWorkspace) return CRDT_E_WORKSPACE;
        if (status & kErrHint) return CRDT_E_INVALID;
        if (status & kErrIndex) return CRDT_E_INVALID;
        if (status & kErrCapacity) return CRDT_E_CAPACITY;
        if (status & kErrDupKey) return CRDT_E_DUP_KEY;
    }
    return CRDT_OK;
}

static int join_common(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_awset_batch* src,
                       const crdt_awset_out* out, const crdt_awset_out* out2, void* stream) {
    if (!ctx || check_join(dst, src, out, out2) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->worklist, dst->n_docs);
    if (c.rc != CRDT_OK) return c.rc;
    const bool no_large = ctx->max_doc_entries <= 64 || ctx->call_small;
    TileWork tw{};
    const bool tiles = !no_large && ctx->join_tiles;
    if (tiles) {
        const size_t n = std::max<size_t>(dst->n_docs, 1);
        c.need_bytes(ctx->tile_desc, ((size_t)ctx->tile_cap + 1) * 16);  // (+1: the next pass's first split)
        c.need_bytes(ctx->tile_geo, ((size_t)ctx->tile_cap + 8) * 32);   // (+8: geo_slot)
        c.need_bytes(ctx->tile_flags, (size_t)ctx->tile_cap * 8);
        c.need_bytes(ctx->tile_slot, n * 4);
        c.need_bytes(ctx->tile_run, ((n + 1023) / 1024) * 4);
        if (c.rc != CRDT_OK) return c.rc;
        uint32_t* w = ctx->ws.as<uint32_t>(0);
        // Passes of tile_cap tiles: as many as the call's tiles can need.  A host-path
        // call counted them (ctx->call_tiles); otherwise a document of nd + ns merged
        // positions has ceil((nd + ns) / T) tiles, and a batch's slots are < 2^32 per
        // side, so a call has at most 2^33 / T + n_docs -- or, under the caller's
        // max_doc_entries promise, n_docs * ceil(2 max / T).  Passes past the call's
        // tiles return at once.  The block kernel is launched behind them (gated on
        // the plan's fallback word) unless the passes hold every tile a call can have
        // without trusting the promise: beyond them (tile_max_passes, or a broken
        // promise) it takes the worklist.
        const uint64_t T = tile_positions(ctx->tile_shape);
        const uint64_t hard = ctx->call_tiles ? ctx->call_tiles : (1ull << 33) / T + dst->n_docs;
        uint64_t bound = hard;
        if (!ctx->call_tiles && ctx->max_doc_entries != 0xFFFFFFFFu)
            bound = std::min<uint64_t>(bound, (uint64_t)dst->n_docs * ((2ull * ctx->max_doc_entries + T - 1) / T));
        auto passes_for = [&](uint64_t t) { return std::max<uint64_t>(1, (t + ctx->tile_cap - 1) / ctx->tile_cap); };
        const uint32_t passes = (uint32_t)std::min<uint64_t>(passes_for(bound), ctx->tile_max_passes);
        tw = TileWork{ctx->tile_desc.as<uint4>(), ctx->tile_geo.as<uint4>(), ctx->tile_flags.as<uint64_t>(), ctx->tile_slot.as<uint32_t>(),
                      ctx->tile_run.as<uint32_t>(), w + 3, w + 8, w + 5, w + 6, ctx->tile_cap,
                      tile_positions(ctx->tile_shape), ctx->tile_shape, ctx->tile_nt_stores ? 1u : 0u,
                      ctx->tile_split_bpc, ctx->tile_shards, 0u, passes, passes_for(hard) <= passes ? 1u : 0u};
    }
    // the per-call counters are read only by the large-document paths
    if (!no_large && launch_reset_work(ctx->ws.as<uint32_t>(0), c.s) != hipSuccess) return CRDT_E_HIP;
    OutView o2v;
    if (out2) o2v = view(out2);
    return c.end(launch_join(view(dst), view(src), view(out), out2 ? &o2v : nullptr, make_work(ctx),
                             ctx->join_docs_per_wave, ctx->join_nt_stores, ctx->join_stage_stores,
                             ctx->join_slab_per_cu * (uint32_t)ctx->n_cu, block_grid(ctx), no_large,
                             tiles ? &tw : nullptr, (uint32_t)ctx->n_cu, c.s));
}

int crdt_awset_join_async(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_awset_batch* src,
                          const crdt_awset_out* out, void* stream) {
    return join_common(ctx, dst, src, out, nullptr, stream);
}

int crdt_awset_exchange_async(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b,
                              const crdt_awset_out* out_ab, const crdt_awset_out* out_ba, void* stream) {
    if (check_exchange(a, b, out_ab, out_ba) != CRDT_OK) return CRDT_E_INVALID;
    return join_common(ctx, a, b, out_ab, out_ba, stream);
}

// The fold's scratch copy of the output slots: at least one slot, never allocated
// during a capture.
static int fold_scratch(crdt_ctx* ctx, bool cap, Scratch* scr) {
    if (ctx->scratch_slots == 0) {
        if (cap) return CRDT_E_WORKSPACE;
        if (reserve_scratch(ctx, 1) != CRDT_OK) return CRDT_E_NOMEM;
    }
    const size_t slots = ctx->scratch_slots;
    *scr = Scratch{ctx->scratch.as<uint64_t>(0), ctx->scratch.as<uint32_t>(slots * 16),
                   ctx->scratch.as<uint64_t>(slots * 8), slots};
    return CRDT_OK;
}

int crdt_awset_fold_async(crdt_ctx* ctx, int mode, const crdt_awset_batch* dst, const crdt_src_batch* srcs,
                          const crdt_awset_out* out, void* stream) {
    if (!ctx || check_fold(mode, dst, srcs, out) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->worklist, dst->n_docs);
    c.need(ctx->defer, dst->n_docs);
    if (c.rc != CRDT_OK) return c.rc;
    Scratch scr;
    if (int rc = fold_scratch(ctx, c.cap, &scr)) return rc;
    if (launch_reset_work(ctx->ws.as<uint32_t>(0), c.s) != hipSuccess) return CRDT_E_HIP;
    return c.end(launch_fold(mode, view(dst), view(srcs), view(out), scr, make_work(ctx), block_grid(ctx),
                             ctx->fold_lean_first, c.s));
}

// The group counts of the extraction (extract.hip) live in the worklist and
// defer buffers: one word per group of 64 / R documents each, at most n_docs,
// which is what crdt_ctx_reserve(max_docs, ..) sizes them for.
int crdt_awset_delta_extract_async(crdt_ctx* ctx, const crdt_src_batch* srcs, const uint64_t* peer_vv,
                                   const crdt_delta_out* out, void* stream) {
    if (!ctx || check_extract(srcs, peer_vv, out) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->worklist, srcs->n_docs);
    c.need(ctx->defer, srcs->n_docs);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_extract(view(srcs), peer_vv, view(out, true), ctx->worklist.as<uint32_t>(),
                                ctx->defer.as<uint32_t>(), make_work(ctx), (uint32_t)ctx->n_cu, c.s));
}

// Membership reads (query.hip): one launch over the five-array view, ordered
// after the context's previous call like every call that shares its status word.
static int has_common(crdt_ctx* ctx, const HasView& sv, const crdt_query_batch* q, const crdt_query_out* out,
                      void* stream) {
    if (q->n_queries == 0) return CRDT_OK;
    if (sv.n_docs == 0) return CRDT_E_INVALID;  // (queries of no document)
    Call c(ctx, stream);
    if (c.rc != CRDT_OK) return c.rc;
    const Work wk = make_work(ctx);
    return c.end(launch_has(sv, HasQueries{q->n_queries, q->q_off, q->keys},
                            HasOut{out->found, out->actors, out->counters}, wk.status, wk.gate, (uint32_t)ctx->n_cu,
                            c.s));
}

int crdt_awset_has_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_query_batch* q,
                         const crdt_query_out* out, void* stream) {
    if (!ctx || check_has(state, q, out) != CRDT_OK) return CRDT_E_INVALID;
    return has_common(ctx, has_view(state), q, out, stream);
}

int crdt_tomb_has_async(crdt_ctx* ctx, const crdt_tomb_batch* tombs, uint32_t n_docs, const crdt_query_batch* q,
                        const crdt_query_out* out, void* stream) {
    if (!ctx || check_tomb_has(tombs, n_docs, q, out) != CRDT_OK) return CRDT_E_INVALID;
    return has_common(ctx, has_view(tombs, n_docs), q, out, stream);
}

// Convergence check (compare.hip).  The per-document flag words the entry and
// clock passes OR into live in the defer buffer: one word per document, which is
// what crdt_ctx_reserve(max_docs, ..) sizes it for.
int crdt_awset_compare_async(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b, uint32_t mask,
                             const crdt_compare_out* out, void* stream) {
    if (!ctx || check_compare(a, b, mask, out) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->defer, a->n_docs);
    if (c.rc != CRDT_OK) return c.rc;
    const Work wk = make_work(ctx);
    return c.end(launch_compare(view(a), view(b), mask,
                                CompareOutView{out->flags, out->summary, out->worklist, out->n_work},
                                ctx->defer.as<uint32_t>(), wk.status, wk.gate, (uint32_t)ctx->n_cu, c.s));
}

// State digests (digest.hip): the digest words are the accumulators, no workspace.
int crdt_awset_digest_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_tomb_batch* tombs,
                            uint64_t* digest, void* stream) {
    if (!ctx || check_digest(state, tombs, digest) != CRDT_OK) return CRDT_E_INVALID;
    if (state->n_docs == 0) return CRDT_OK;
    Call c(ctx, stream);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_digest(has_view(state), has_view(tombs, state->n_docs), state->vv, state->R, digest,
                               make_work(ctx).status, (uint32_t)ctx->n_cu, c.s));
}

// Worklist digests (digest_idx.hip): each listed document has one owner, no workspace.
int crdt_awset_digest_idx_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_tomb_batch* tombs,
                                const uint32_t* idx, const uint32_t* n_idx, uint32_t n_max, uint32_t n_digest_docs,
                                uint32_t mode, uint64_t* digest, void* stream) {
    if (!ctx || check_digest_idx(state, tombs, idx, n_idx, n_max, n_digest_docs, mode, digest) != CRDT_OK)
        return CRDT_E_INVALID;
    if (n_max == 0) return CRDT_OK;
    Call c(ctx, stream);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_digest_idx(has_view(state), has_view(tombs, state->n_docs), state->vv, state->R, idx, n_idx,
                                   n_max, n_digest_docs, mode, digest, make_work(ctx).status, (uint32_t)ctx->n_cu,
                                   c.s));
}

// Digest comparison (digest.hip, then compare.hip's worklist step): the flag
// words live in the defer buffer, one per document, as in the compare.
int crdt_digest_diff_async(crdt_ctx* ctx, const uint64_t* mine, const uint64_t* theirs, uint32_t n_docs, uint32_t mask,
                           const crdt_compare_out* out, void* stream) {
    if (!ctx || check_digest_diff(mine, theirs, n_docs, mask, out) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->defer, n_docs);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_digest_diff(mine, theirs, n_docs, mask,
                                    CompareOutView{out->flags, out->summary, out->worklist, out->n_work},
                                    ctx->defer.as<uint32_t>(), make_work(ctx).gate, (uint32_t)ctx->n_cu, c.s));
}

// Digest tree (digest_tree.hip).  The build and the children gather use no
// workspace.  The diff's partial sums, three words per 64 listed parents, live in
// the defer buffer: at most n_docs words for the parents of a level of n_docs
// children, which is what crdt_ctx_reserve(max_docs, ..) sizes it for.
int crdt_digest_tree_async(crdt_ctx* ctx, const uint64_t* digest, uint32_t n_docs, uint64_t* tree, void* stream) {
    if (!ctx || check_digest_tree(digest, n_docs, tree) != CRDT_OK) return CRDT_E_INVALID;
    if (n_docs == 0) return CRDT_OK;
    Call c(ctx, stream);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_digest_tree(digest, n_docs, tree, ctx->digest_tree_fuse, c.s));
}

int crdt_digest_tree_children_async(crdt_ctx* ctx, const uint64_t* level, uint32_t n_level, const uint32_t* parents,
                                    const uint32_t* n_parents, uint32_t n_max, uint64_t* out, void* stream) {
    if (!ctx || check_digest_tree_children(level, n_level, parents, n_parents, n_max, out) != CRDT_OK)
        return CRDT_E_INVALID;
    if (n_max == 0) return CRDT_OK;
    Call c(ctx, stream);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_digest_tree_children(level, n_level, parents, n_parents, n_max, out, make_work(ctx).status,
                                             c.s));
}

int crdt_digest_tree_diff_async(crdt_ctx* ctx, const uint64_t* mine_level, uint32_t n_level, const uint64_t* theirs,
                                const uint32_t* parents, const uint32_t* n_parents, uint32_t n_max, uint32_t leaf,
                                uint32_t mask, uint32_t* idx_out, uint8_t* flags_out, uint32_t* n_out,
                                uint32_t out_max, uint32_t* summary, void* stream) {
    if (!ctx || check_digest_tree_diff(mine_level, n_level, theirs, parents, n_parents, n_max, mask, idx_out,
                                       flags_out, n_out, summary) != CRDT_OK)
        return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->defer, digest_tree_diff_parts(n_max));
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_digest_tree_diff(mine_level, n_level, theirs, parents, n_parents, n_max, leaf, mask, idx_out,
                                         flags_out, n_out, out_max, summary, ctx->defer.as<uint32_t>(),
                                         make_work(ctx).status, c.s));
}

// Sub-batch selection / compaction (compare.hip): no workspace.
int crdt_awset_select_async(crdt_ctx* ctx, const crdt_awset_batch* state, const uint32_t* idx, const uint32_t* n_idx,
                            uint32_t n_out, uint32_t out_slots, const crdt_awset_out* out, void* stream) {
    if (!ctx || check_select(state, out) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_select(view(state), idx, n_idx, n_out, out_slots, view(out), make_work(ctx).status,
                               (uint32_t)ctx->n_cu, c.s));
}

// Scatter (scatter.hip): the inverse map (one word per state document) lives in
// the worklist buffer and the scan's partial sums (one word per chunk of
// documents, at most n_docs) in the defer buffer, which is what
// crdt_ctx_reserve(max_docs, ..) sizes them for.
int crdt_awset_scatter_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_awset_batch* sub,
                             const uint32_t* idx, const uint32_t* n_idx, uint32_t out_slots, const crdt_awset_out* out,
                             void* stream) {
    if (!ctx || check_scatter(state, sub, idx, out) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->worklist, state->n_docs);
    c.need(ctx->defer, state->n_docs);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_scatter(view(state), view(sub), idx, n_idx, out_slots, view(out), ctx->worklist.as<uint32_t>(),
                                ctx->defer.as<uint32_t>(), make_work(ctx).status, (uint32_t)ctx->n_cu, c.s));
}

// Merge diff (diff.hip): the per-document flag words the count pass ORs into live
// in the defer buffer, one word per document, which is what
// crdt_ctx_reserve(max_docs, ..) sizes it for; the partial sums of the two lists
// (a fixed 3 x 2,048 words, whatever the batches hold) in the context-partials
// buffer, allocated once at crdt_ctx_create.
int crdt_awset_diff_async(crdt_ctx* ctx, const crdt_awset_batch* before, const crdt_awset_batch* after,
                          uint32_t rem_slots, uint32_t ups_slots, const crdt_diff_out* out, void* stream) {
    if (!ctx || check_diff(before, after, rem_slots, ups_slots, out) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->defer, before->n_docs);
    if (c.rc == CRDT_OK && ctx->parts.bytes < diff_parts_bytes()) c.rc = CRDT_E_WORKSPACE;  // (sized at create: never)
    if (c.rc != CRDT_OK) return c.rc;
    const Work wk = make_work(ctx);
    const DiffOutView ov{out->flags,      out->summary,  out->rem_off,    out->rem_keys,     out->rem_actors, out->rem_counters,
                         out->ups_off,    out->ups_keys, out->ups_actors, out->ups_counters, out->ups_kind};
    return c.end(launch_diff(view(before), view(after), rem_slots, ups_slots, ov, ctx->defer.as<uint32_t>(),
                             ctx->parts.as<uint32_t>(), wk.status, wk.gate, (uint32_t)ctx->n_cu, c.s));
}

// Sources (sources.hip): the scan's partial sums, one word per 1,024 sources for
// the entries (worklist buffer) and one for the tombstones (defer buffer).  The
// replica descriptors are flattened into the kernel arguments here.
int crdt_awset_sources_async(crdt_ctx* ctx, const crdt_replica* reps, uint32_t n_reps, uint32_t entry_slots,
                             uint32_t tomb_slots, const crdt_delta_out* out, void* stream) {
    if (!ctx || check_sources(reps, n_reps, out) != CRDT_OK) return CRDT_E_INVALID;
    SourcesArgs a{};
    for (uint32_t p = 0; p < n_reps; ++p) {
        SrcRep& r = a.rep[p];
        r.e = cols(reps[p].state);
        r.t = cols(reps[p].tombs);
        r.vv = reps[p].state->vv;
        r.doc_actor = reps[p].doc_actor;
        r.actor = reps[p].actor;
    }
    a.n_reps = n_reps;
    a.n_docs = reps[0].state->n_docs;
    a.R = reps[0].state->R;
    a.n_srcs = a.n_docs * n_reps;  // (< 2^32: checked)
    a.entry_slots = entry_slots;
    a.tomb_slots = tomb_slots;
    a.out = view(out, false);
    Call c(ctx, stream);
    const size_t n_parts = ((size_t)a.n_srcs + 1023) / 1024;
    c.need(ctx->worklist, n_parts);
    c.need(ctx->defer, n_parts);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_sources(a, ctx->worklist.as<uint32_t>(), ctx->defer.as<uint32_t>(), make_work(ctx).status,
                                (uint32_t)ctx->n_cu, c.s));
}

// Replica select / scatter (replica.hip).  sub == NULL: the select.  The scan's
// partial sums are one word per 1,024 output documents for the entries and one
// for the tombstones.  Select keeps them in the worklist and the defer buffer;
// scatter keeps its inverse map (one word per document) in the worklist buffer
// and both partial arrays in the defer buffer (2 * ceil(n / 1,024) <= max(n, 2)
// words), which is what crdt_ctx_reserve(max_docs, ..) sizes them for.
// room != NULL: the repack (replica_repack.hip) with the entry policy room[0] and
// the tombstone policy room[1]; same arguments and workspace.  The callers have
// checked the arguments.
static int replica_common(crdt_ctx* ctx, const crdt_replica* rep, const crdt_replica* sub, const uint32_t* idx,
                          const uint32_t* n_idx, uint32_t n_out, uint32_t entry_slots, uint32_t tomb_slots,
                          const crdt_replica_out* out, bool scatter, void* stream,
                          const crdt_headroom* room = nullptr) {
    ReplicaArgs a{};
    a.rep = rep_side(rep);
    if (scatter) a.sub = rep_side(sub);
    a.idx = idx;
    a.n_idx = n_idx;
    // an empty call writes offsets[0] = 0 alone and launches nothing that reads documents
    const uint32_t n = rep->state->n_docs == 0 ? 0u : (scatter ? rep->state->n_docs : n_out);
    a.n_out = n;
    a.R = rep->state->R;
    a.entry_slots = entry_slots;
    a.tomb_slots = tomb_slots;
    a.out = view(out->state);
    a.tout = view(out->tombs);
    // no input has tombstones: offsets (and counts) zeroed, no column written
    if (!rep->tombs && !(scatter && sub->tombs)) a.tout.keys = nullptr;
    a.out_actor = out->doc_actor;
    Call c(ctx, stream);
    const size_t n_parts = ((size_t)n + 1023) / 1024;
    uint32_t *inv = nullptr, *parts_e = nullptr, *parts_t = nullptr;
    if (scatter) {
        c.need(ctx->worklist, n);
        c.need(ctx->defer, std::max<size_t>(2 * n_parts, 2));
        if (c.rc != CRDT_OK) return c.rc;
        inv = ctx->worklist.as<uint32_t>();
        parts_e = ctx->defer.as<uint32_t>();
        parts_t = parts_e + n_parts;
        a.inv = inv;
    } else {
        c.need(ctx->worklist, n_parts);
        c.need(ctx->defer, n_parts);
        if (c.rc != CRDT_OK) return c.rc;
        parts_e = ctx->worklist.as<uint32_t>();
        parts_t = ctx->defer.as<uint32_t>();
    }
    if (room)
        return c.end(launch_replica_repack(RepackArgs{a, room[0], room[1]}, inv, parts_e, parts_t,
                                           make_work(ctx).status, (uint32_t)ctx->n_cu, c.s));
    return c.end(launch_replica(a, inv, parts_e, parts_t, make_work(ctx).status, (uint32_t)ctx->n_cu, c.s));
}

int crdt_replica_select_async(crdt_ctx* ctx, const crdt_replica* rep, const uint32_t* idx, const uint32_t* n_idx,
                              uint32_t n_out, uint32_t entry_slots, uint32_t tomb_slots, const crdt_replica_out* out,
                              void* stream) {
    if (!ctx || check_replica(rep, nullptr, idx, out, false) != CRDT_OK) return CRDT_E_INVALID;
    return replica_common(ctx, rep, nullptr, idx, n_idx, n_out, entry_slots, tomb_slots, out, false, stream);
}

int crdt_replica_scatter_async(crdt_ctx* ctx, const crdt_replica* rep, const crdt_replica* sub, const uint32_t* idx,
                               const uint32_t* n_idx, uint32_t entry_slots, uint32_t tomb_slots,
                               const crdt_replica_out* out, void* stream) {
    if (!ctx || check_replica(rep, sub, idx, out, true) != CRDT_OK) return CRDT_E_INVALID;
    return replica_common(ctx, rep, sub, idx, n_idx, 0u, entry_slots, tomb_slots, out, true, stream);
}

// The headroom policy's capacity: headroom_cap64 (headroom.hpp) saturated, the one
// definition the repack kernels share.  A NULL policy is packed.
uint32_t crdt_headroom_capacity(const crdt_headroom* h, uint32_t n) {
    bool sat = false;
    return headroom_cap(h ? *h : kHeadroomPacked, n, &sat);
}

// Replica repack (replica_repack.hip): select's arguments when sub == NULL,
// scatter's otherwise, and everything replica_common checks and sizes for them.
int crdt_replica_repack_async(crdt_ctx* ctx, const crdt_replica* rep, const crdt_replica* sub, const uint32_t* idx,
                              const uint32_t* n_idx, uint32_t n_out, const crdt_headroom* entry_room,
                              const crdt_headroom* tomb_room, uint32_t entry_slots, uint32_t tomb_slots,
                              const crdt_replica_out* out, void* stream) {
    const crdt_headroom room[2] = {entry_room ? *entry_room : kHeadroomPacked, tomb_room ? *tomb_room : kHeadroomPacked};
    if (!headroom_ok(room[0]) || !headroom_ok(room[1])) return CRDT_E_INVALID;
    if (!ctx || check_replica_repack(rep, sub, idx, n_out, out) != CRDT_OK) return CRDT_E_INVALID;
    return replica_common(ctx, rep, sub, idx, n_idx, n_out, entry_slots, tomb_slots, out, sub != nullptr, stream, room);
}

// In-place replica scatter (replica_inplace.hip).  Workspace: the inverse map,
// one word per replica document, in the worklist buffer; the verdicts, one word
// per sub document, in the defer buffer; the spill scan's partial sums, one word
// per 1,024 sub documents, in a buffer of their own (the other two are full at
// max_docs documents): all three sized by crdt_ctx_reserve(max_docs, ..).
int crdt_replica_scatter_inplace_async(crdt_ctx* ctx, const crdt_replica_inplace* rep, const crdt_replica* sub,
                                       const uint32_t* idx, const uint32_t* n_idx, const crdt_spill_out* spill,
                                       void* stream) {
    if (!ctx || check_inplace(rep, sub, idx, spill) != CRDT_OK) return CRDT_E_INVALID;
    InplaceArgs a{};
    a.sub = rep_side(sub);
    a.n_docs = rep->n_docs;
    a.R = rep->R;
    a.e = InplaceCols{rep->offsets, rep->counts, rep->keys, rep->actors, rep->counters};
    if (rep->tomb_offsets)
        a.t = InplaceCols{rep->tomb_offsets, rep->tomb_counts, rep->tkeys, rep->tactors, rep->tcounters};
    a.vv = rep->vv;
    a.doc_actor = rep->doc_actor;
    a.idx = idx;
    a.n_idx = n_idx;
    a.spill_j = spill->spill_j;
    a.spill_doc = spill->spill_doc;
    a.n_spill = spill->n_spill;
    Call c(ctx, stream);
    const size_t n_sub = sub->state->n_docs;
    c.need(ctx->worklist, rep->n_docs);
    c.need(ctx->defer, n_sub);
    c.need_bytes(ctx->spill_parts, (n_sub / 1024 + 1) * sizeof(uint32_t));
    if (c.rc != CRDT_OK) return c.rc;
    a.verdict = ctx->defer.as<uint32_t>();
    return c.end(launch_replica_inplace(a, ctx->worklist.as<uint32_t>(), ctx->spill_parts.as<uint32_t>(),
                                        make_work(ctx).status, (uint32_t)ctx->n_cu, c.s));
}

// Delta merge of a resident pair (delta_pair.hip).  Workspace: the join's
// worklist, one word per document, which crdt_ctx_reserve(max_docs, ..) sizes.
// a_tombs / a_doc_actor / a_actor: replica a beyond its state (the exchange);
// out_ba == NULL: the join, which reads none of them.  The callers have checked
// the arguments.
static int delta_pair_common(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_tomb_batch* a_tombs,
                             const uint32_t* a_doc_actor, uint32_t a_actor, const crdt_replica* b,
                             const crdt_awset_out* out_ab, const crdt_awset_out* out_ba, uint8_t* kind_ab,
                             uint8_t* kind_ba, void* stream) {
    if (!ctx) return CRDT_E_INVALID;
    if (a->n_docs == 0) return CRDT_OK;
    Call c(ctx, stream);
    c.need(ctx->worklist, a->n_docs);
    if (c.rc != CRDT_OK) return c.rc;
    if (launch_reset_work(ctx->ws.as<uint32_t>(0), c.s) != hipSuccess) return CRDT_E_HIP;
    OutView o2v;
    if (out_ba) o2v = view(out_ba);
    return c.end(launch_delta_pair(pair_side(a, a_tombs, a_doc_actor, a_actor),
                                   pair_side(b->state, b->tombs, b->doc_actor, b->actor), view(out_ab),
                                   out_ba ? &o2v : nullptr, kind_ab, kind_ba, make_work(ctx), block_grid(ctx), c.s));
}

int crdt_awset_delta_join_async(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_replica* src,
                                const crdt_awset_out* out, uint8_t* kind, void* stream) {
    if (check_delta_pair(dst, nullptr, nullptr, src, out, nullptr, kind, nullptr) != CRDT_OK) return CRDT_E_INVALID;
    return delta_pair_common(ctx, dst, nullptr, nullptr, 0u, src, out, nullptr, kind, nullptr, stream);
}

int crdt_awset_delta_exchange_async(crdt_ctx* ctx, const crdt_replica* a, const crdt_replica* b,
                                    const crdt_awset_out* out_ab, const crdt_awset_out* out_ba, uint8_t* kind_ab,
                                    uint8_t* kind_ba, void* stream) {
    if (check_delta_exchange(a, b, out_ab, out_ba, kind_ab, kind_ba) != CRDT_OK) return CRDT_E_INVALID;
    return delta_pair_common(ctx, a->state, a->tombs, a->doc_actor, a->actor, b, out_ab, out_ba, kind_ab, kind_ba,
                             stream);
}

// Logged join and exchange (join_log.hip).  Workspace: the join's worklist, one
// word per document, which crdt_ctx_reserve(max_docs, ..) sizes, and the summary's
// partial sums in the context-partials buffer, allocated once at crdt_ctx_create.
// out_ba / log_ba == NULL: the join.
static int join_log_common(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b,
                           const crdt_awset_out* out_ab, const crdt_awset_out* out_ba, const crdt_merge_log* log_ab,
                           const crdt_merge_log* log_ba, bool exchange, void* stream) {
    if (!ctx || check_join_log(a, b, out_ab, out_ba, log_ab, log_ba, exchange) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->worklist, a->n_docs);
    if (c.rc == CRDT_OK && ctx->parts.bytes < join_log_parts_bytes()) c.rc = CRDT_E_WORKSPACE;  // (sized at create: never)
    if (c.rc != CRDT_OK) return c.rc;
    if (a->n_docs != 0 && launch_reset_work(ctx->ws.as<uint32_t>(0), c.s) != hipSuccess) return CRDT_E_HIP;
    OutView o2v;
    MergeLogView l2v;
    if (out_ba) {
        o2v = view(out_ba);
        l2v = view(log_ba);
    }
    return c.end(launch_join_log(view(a), view(b), view(out_ab), out_ba ? &o2v : nullptr, view(log_ab),
                                 out_ba ? &l2v : nullptr, make_work(ctx), ctx->parts.as<uint32_t>(), block_grid(ctx),
                                 c.s));
}

int crdt_awset_join_log_async(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_awset_batch* src,
                              const crdt_awset_out* out, const crdt_merge_log* log, void* stream) {
    return join_log_common(ctx, dst, src, out, nullptr, log, nullptr, false, stream);
}

int crdt_awset_exchange_log_async(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b,
                                  const crdt_awset_out* out_ab, const crdt_awset_out* out_ba,
                                  const crdt_merge_log* log_ab, const crdt_merge_log* log_ba, void* stream) {
    return join_log_common(ctx, a, b, out_ab, out_ba, log_ab, log_ba, true, stream);
}

// Logged delta merge of a resident pair (delta_pair_log.hip).  Workspace: the
// join's worklist and the summary's partial sums, as the logged join.  The
// argument errors are the delta exchange's and the logged join's together.
// a_tombs / a_doc_actor / a_actor: replica a beyond its state (the exchange);
// out_ba / log_ba == NULL: the join, which reads none of them.  The callers have
// checked the arguments.
static int delta_pair_log_common(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_tomb_batch* a_tombs,
                                 const uint32_t* a_doc_actor, uint32_t a_actor, const crdt_replica* b,
                                 const crdt_awset_out* out_ab, const crdt_awset_out* out_ba, uint8_t* kind_ab,
                                 uint8_t* kind_ba, const crdt_merge_log* log_ab, const crdt_merge_log* log_ba,
                                 void* stream) {
    if (!ctx) return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->worklist, a->n_docs);
    if (c.rc == CRDT_OK && ctx->parts.bytes < join_log_parts_bytes()) c.rc = CRDT_E_WORKSPACE;  // (sized at create: never)
    if (c.rc != CRDT_OK) return c.rc;
    if (a->n_docs != 0 && launch_reset_work(ctx->ws.as<uint32_t>(0), c.s) != hipSuccess) return CRDT_E_HIP;
    OutView o2v;
    MergeLogView l2v;
    if (out_ba) {
        o2v = view(out_ba);
        l2v = view(log_ba);
    }
    return c.end(launch_delta_pair_log(pair_side(a, a_tombs, a_doc_actor, a_actor),
                                       pair_side(b->state, b->tombs, b->doc_actor, b->actor), view(out_ab),
                                       out_ba ? &o2v : nullptr, kind_ab, kind_ba, view(log_ab),
                                       out_ba ? &l2v : nullptr, make_work(ctx), ctx->parts.as<uint32_t>(),
                                       block_grid(ctx), c.s));
}

int crdt_awset_delta_join_log_async(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_replica* src,
                                    const crdt_awset_out* out, uint8_t* kind, const crdt_merge_log* log,
                                    void* stream) {
    if (check_delta_pair_log(dst, nullptr, nullptr, src, out, nullptr, kind, nullptr, log, nullptr) != CRDT_OK)
        return CRDT_E_INVALID;
    return delta_pair_log_common(ctx, dst, nullptr, nullptr, 0u, src, out, nullptr, kind, nullptr, log, nullptr,
                                 stream);
}

int crdt_awset_delta_exchange_log_async(crdt_ctx* ctx, const crdt_replica* a, const crdt_replica* b,
                                        const crdt_awset_out* out_ab, const crdt_awset_out* out_ba, uint8_t* kind_ab,
                                        uint8_t* kind_ba, const crdt_merge_log* log_ab, const crdt_merge_log* log_ba,
                                        void* stream) {
    if (check_delta_exchange_log(a, b, out_ab, out_ba, kind_ab, kind_ba, log_ab, log_ba) != CRDT_OK)
        return CRDT_E_INVALID;
    return delta_pair_log_common(ctx, a->state, a->tombs, a->doc_actor, a->actor, b, out_ab, out_ba, kind_ab,
                                 kind_ba, log_ab, log_ba, stream);
}

// Logged fold (fold_log.hip).  Workspace: the fold's worklist and scratch copy of
// the output slots, and the logged join's summary partial sums.  The argument
// errors are the fold's and the logged join's together.
int crdt_awset_fold_log_async(crdt_ctx* ctx, int mode, const crdt_awset_batch* dst, const crdt_src_batch* srcs,
                              const crdt_awset_out* out, const crdt_merge_log* log, void* stream) {
    if (!ctx || check_fold_log(mode, dst, srcs, out, log) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    c.need(ctx->worklist, dst->n_docs);
    if (c.rc == CRDT_OK && ctx->parts.bytes < join_log_parts_bytes()) c.rc = CRDT_E_WORKSPACE;  // (sized at create: never)
    if (c.rc != CRDT_OK) return c.rc;
    Scratch scr;
    if (int rc = fold_scratch(ctx, c.cap, &scr)) return rc;
    if (dst->n_docs != 0 && launch_reset_work(ctx->ws.as<uint32_t>(0), c.s) != hipSuccess) return CRDT_E_HIP;
    return c.end(launch_fold_log(mode, view(dst), view(srcs), view(out), scr, view(log), make_work(ctx),
                                 ctx->parts.as<uint32_t>(), block_grid(ctx), c.s));
}

int crdt_awset_apply_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_tomb_batch* tombs,
                           const crdt_op_batch* ops, const crdt_awset_out* out, const crdt_tomb_out* tomb_out,
                           void* stream) {
    if (!ctx || check_apply(state, tombs, ops, out, tomb_out) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    if (c.rc != CRDT_OK) return c.rc;
    const ApplyOps av{ops->n_docs, ops->op_off, ops->kind, ops->keys, ops->doc_actor};
    return c.end(launch_apply(view(state), view(tombs), av, view(out), view(tomb_out), tomb_out != nullptr,
                              make_work(ctx), (uint32_t)ctx->n_cu, c.s));
}

// Logged local ops (apply_log.hip).  Workspace: the logged join's summary partial
// sums.  The argument errors are apply's and the logged join's together.
int crdt_awset_apply_log_async(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_tomb_batch* tombs,
                               const crdt_op_batch* ops, const crdt_awset_out* out, const crdt_tomb_out* tomb_out,
                               const crdt_merge_log* log, void* stream) {
    if (!ctx || check_apply_log(state, tombs, ops, out, tomb_out, log) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    if (c.rc == CRDT_OK && ctx->parts.bytes < join_log_parts_bytes()) c.rc = CRDT_E_WORKSPACE;  // (sized at create: never)
    if (c.rc != CRDT_OK) return c.rc;
    const ApplyOps av{ops->n_docs, ops->op_off, ops->kind, ops->keys, ops->doc_actor};
    return c.end(launch_apply_log(view(state), view(tombs), av, view(out), view(tomb_out), tomb_out != nullptr,
                                  view(log), make_work(ctx), ctx->parts.as<uint32_t>(), (uint32_t)ctx->n_cu, c.s));
}

int crdt_awset_sort_async(crdt_ctx* ctx, const crdt_awset_batch* in, uint32_t n_slots, const crdt_awset_out* out,
                          void* stream) {
    if (!ctx || check_sort(in, n_slots, out) != CRDT_OK) return CRDT_E_INVALID;
    Call c(ctx, stream);
    if (c.rc != CRDT_OK) return c.rc;
    size_t tb = 0;
    if (sort_storage(in->n_docs, n_slots, &tb) != hipSuccess) return CRDT_E_HIP;
    c.need_bytes(ctx->sort_tmp, std::max<size_t>(tb, 16));
    c.need(ctx->sort_idx, n_slots);
    c.need(ctx->sort_ends, in->n_docs);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_sort(view(in), n_slots, view(out), ctx->sort_tmp.p, ctx->sort_tmp.bytes,
                             ctx->sort_ends.as<uint32_t>(), ctx->sort_idx.as<uint32_t>(), ctx->ws.as<uint32_t>(64),
                             (uint32_t)ctx->n_cu, c.s));
}

int crdt_vv_min_async(crdt_ctx* ctx, uint64_t* dst, const uint64_t* src, size_t n, void* stream) {
    if (!ctx || (n && (!dst || !src))) return CRDT_E_INVALID;
    int rc = set_device(ctx);
    if (rc != CRDT_OK) return rc;
    return hip_err(launch_vv_min(dst, src, n, (hipStream_t)stream));
}

int crdt_tombstone_gc_async(crdt_ctx* ctx, const crdt_tomb_batch* tombs, uint32_t n_docs, uint32_t R,
                            const uint64_t* stable_vv, const crdt_tomb_out* out, void* stream) {
    if (!ctx || !tombs || !tombs->offsets || !out || !out->offsets || !out->counts || R == 0 || R > CRDT_MAX_R ||
        (n_docs && !stable_vv))
        return CRDT_E_INVALID;
    int rc = set_device(ctx);
    if (rc != CRDT_OK) return rc;
    return hip_err(launch_tomb_gc(view(tombs), n_docs, R, stable_vv, view(out), (uint32_t)ctx->n_cu,
                                  (hipStream_t)stream));
}

int crdt_vv_max_async(crdt_ctx* ctx, uint64_t* dst, const uint64_t* src, size_t n, void* stream) {
    if (!ctx || (n && (!dst || !src))) return CRDT_E_INVALID;
    int rc = set_device(ctx);
    if (rc != CRDT_OK) return rc;
    return hip_err(launch_vv_max(dst, src, n, (hipStream_t)stream));
}

int crdt_causal_context_async(crdt_ctx* ctx, const uint64_t* vv, uint32_t n_docs, uint32_t R, uint64_t* out,
                              void* stream) {
    if (!ctx || !out || R == 0 || R > CRDT_MAX_R || (n_docs && !vv)) return CRDT_E_INVALID;
    const uint32_t n_part = std::min<uint32_t>(kCtxParts, std::max<uint32_t>(1u, (n_docs + 255) / 256));
    Call c(ctx, stream);
    if (c.rc != CRDT_OK) return c.rc;
    return c.end(launch_context(vv, n_docs, R, ctx->parts.as<uint64_t>(), n_part, out, c.s));
}

int crdt_gen_pair_async(crdt_ctx* ctx, uint64_t seed, uint32_t n_docs, const crdt_awset_out* a,
                        const crdt_awset_out* b, void* stream) {
    if (!ctx || !out_ptrs_ok(a) || !out_ptrs_ok(b)) return CRDT_E_INVALID;
    if ((uint64_t)n_docs * 64ull >= (1ull << 32)) return CRDT_E_INVALID;
    int rc = set_device(ctx);
    if (rc != CRDT_OK) return rc;
    return hip_err(launch_gen_pair(seed, n_docs, view(a), view(b), (hipStream_t)stream));
}

int crdt_gen_delta_async(crdt_ctx* ctx, uint64_t seed, uint32_t n_docs, uint32_t R, uint32_t n_srcs_per_doc,
                         const crdt_awset_out* dst, const crdt_src_batch* srcs, void* stream) {
    if (!ctx || !out_ptrs_ok(dst) || !src_ptrs_ok(srcs) || !srcs->tomb_off || R == 0 || R > CRDT_MAX_R ||
        n_srcs_per_doc == 0)
        return CRDT_E_INVALID;
    if ((uint64_t)n_docs * n_srcs_per_doc * 8ull >= (1ull << 32) || (uint64_t)n_docs * 64ull >= (1ull << 32))
        return CRDT_E_INVALID;
    int rc = set_device(ctx);
    if (rc != CRDT_OK) return rc;
    auto w = [](const void* p) { return const_cast<void*>(p); };
    SrcOutView S{(uint32_t*)w(srcs->doc_srcs), (uint32_t*)w(srcs->src_actor), (uint64_t*)w(srcs->vv),
                 (uint32_t*)w(srcs->entry_off), (uint64_t*)w(srcs->keys), (uint32_t*)w(srcs->actors),
                 (uint64_t*)w(srcs->counters), (uint32_t*)w(srcs->tomb_off), (uint64_t*)w(srcs->tkeys),
                 (uint32_t*)w(srcs->tactors), (uint64_t*)w(srcs->tcounters)};
    return hip_err(launch_gen_delta(seed, n_docs, R, n_srcs_per_doc, view(dst), S, (hipStream_t)stream));
}

int crdt_gen_replicas_async(crdt_ctx* ctx, uint64_t seed, uint32_t n_docs, uint32_t replicas, uint32_t entries,
                            const crdt_awset_out* dst, const crdt_src_batch* srcs, void* stream) {
    if (!ctx || !out_ptrs_ok(dst) || !src_ptrs_ok(srcs) || !srcs->tomb_off) return CRDT_E_INVALID;
    if (replicas < 2 || replicas > CRDT_MAX_R || entries < 1 || entries > 32 || (entries & (entries - 1)))
        return CRDT_E_INVALID;
    if ((uint64_t)n_docs * replicas * entries >= (1ull << 32)) return CRDT_E_INVALID;
    int rc = set_device(ctx);
    if (rc != CRDT_OK) return rc;
    auto w = [](const void* p) { return const_cast<void*>(p); };
    SrcOutView S{(uint32_t*)w(srcs->doc_srcs), (uint32_t*)w(srcs->src_actor), (uint64_t*)w(srcs->vv),
                 (uint32_t*)w(srcs->entry_off), (uint64_t*)w(srcs->keys), (uint32_t*)w(srcs->actors),
                 (uint64_t*)w(srcs->counters), (uint32_t*)w(srcs->tomb_off), (uint64_t*)w(srcs->tkeys),
                 (uint32_t*)w(srcs->tactors), (uint64_t*)w(srcs->tcounters)};
    return hip_err(launch_gen_replicas(seed, n_docs, replicas, entries, view(dst), S, (hipStream_t)stream));
}

int crdt_gen_zipf_sizes(uint64_t seed, uint32_t n_docs, uint32_t* sizes) {
    if (n_docs && !sizes) return CRDT_E_INVALID;
    for (uint32_t d = 0; d < n_docs; ++d) sizes[d] = host_zipf_doc_size(seed, d);
    return CRDT_OK;
}

int crdt_gen_zipf_async(crdt_ctx* ctx, uint64_t seed, uint32_t n_docs, const uint32_t* offsets,
                        const crdt_awset_out* a, const crdt_awset_out* b, void* stream) {
    if (!ctx || !offsets || !out_ptrs_ok(a) || !out_ptrs_ok(b) || n_docs >= (1u << 24)) return CRDT_E_INVALID;
    int rc = set_device(ctx);
    if (rc != CRDT_OK) return rc;
    return hip_err(launch_gen_zipf(seed, n_docs, offsets, view(a), view(b), (hipStream_t)stream));
}

int crdt_bw_probe(crdt_ctx* ctx, int kind, const void* a, void* b, size_t bytes, int reps, double* gbs) {
    if (!ctx || !gbs || kind < CRDT_PROBE_READ || kind > CRDT_PROBE_MIX_PLAIN || reps < 1 || bytes < 16 || !b ||
        (kind != CRDT_PROBE_WRITE && kind != CRDT_PROBE_WRITE_PLAIN && !a))
        return CRDT_E_INVALID;
    Call c(ctx, ctx->stream);
    if (c.rc != CRDT_OK) return c.rc;
    if (c.cap) return CRDT_E_INVALID;
    const hipStream_t s = c.s;
    const size_t n16 = bytes / 16;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = hip_err(hipEventCreate(&e0));
    if (rc == CRDT_OK) rc = hip_err(hipEventCreate(&e1));
    // one untimed launch (first touch, clocks up), then reps timed back to back
    if (rc == CRDT_OK) rc = hip_err(launch_probe(kind, a, b, n16, (uint32_t)ctx->n_cu, ctx->probe_blocks_per_cu, ctx->probe_slab, s));
    if (rc == CRDT_OK) rc = hip_err(hipEventRecord(e0, s));
    for (int r = 0; r < reps && rc == CRDT_OK; ++r)
        rc = hip_err(launch_probe(kind, a, b, n16, (uint32_t)ctx->n_cu, ctx->probe_blocks_per_cu, ctx->probe_slab, s));
    if (rc == CRDT_OK) rc = hip_err(hipEventRecord(e1, s));
    if (rc == CRDT_OK) rc = hip_err(hipEventSynchronize(e1));
    float ms = 0.f;
    if (rc == CRDT_OK) rc = hip_err(hipEventElapsedTime(&ms, e0, e1));
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc == CRDT_OK) {
        const bool mix = kind == CRDT_PROBE_MIX || kind == CRDT_PROBE_MIX_PLAIN;
        const double moved = mix ? (double)(n16 / 4) * 16.0 * 7.0
                                 : (double)n16 * 16.0 * ((kind == CRDT_PROBE_COPY || kind == CRDT_PROBE_COPY_PLAIN) ? 2.0 : 1.0);
        *gbs = ms > 0.f ? moved * reps / (ms * 1e-3) / 1e9 : 0.0;
    }
    return c.end(rc);
}

int crdt_host_alloc(size_t bytes, void** out) {
    if (!out) return CRDT_E_INVALID;
    *out = nullptr;
    if (bytes == 0) bytes = 1;
    // CRDT_HOST_MALLOC_FLAGS (diagnostics): hipHostMalloc flags instead of the default
    static const unsigned flags = [] {
        const char* e = std::getenv("CRDT_HOST_MALLOC_FLAGS");
        return e ? (unsigned)std::strtoul(e, nullptr, 0) : (unsigned)hipHostMallocDefault;
    }();
    if (hipHostMalloc(out, bytes, flags) != hipSuccess) return CRDT_E_NOMEM;
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, *out, 0) != hipSuccess) dev = nullptr;
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_blocks[(uintptr_t)*out] = HostBlock{bytes, (uintptr_t)dev};
    return CRDT_OK;
}

void crdt_host_free(void* p) {
    if (p) {
        {
            std::lock_guard<std::mutex> lk(g_host_mu);
            g_host_blocks.erase((uintptr_t)p);
        }
        (void)hipHostFree(p);
    }
}

int crdt_clock_probe(crdt_ctx* ctx, double* mhz) {
    if (!ctx || !mhz) return CRDT_E_INVALID;
    Call c(ctx, ctx->stream);
    if (c.rc != CRDT_OK) return c.rc;
    if (c.cap) return CRDT_E_INVALID;
    const hipStream_t s = c.s;
    int wall_khz = 0;
    if (hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || wall_khz <= 0)
        return CRDT_E_HIP;
    uint64_t* dev = ctx->parts.as<uint64_t>();  // 3 words of the context-summary partials, free between calls
    uint64_t host[2] = {0, 0};
    int rc = hip_err(launch_clock_probe(dev, (uint32_t)ctx->n_cu, s));  // warm-up: clocks ramp up
    if (rc == CRDT_OK) rc = hip_err(launch_clock_probe(dev, (uint32_t)ctx->n_cu, s));
    if (rc == CRDT_OK) rc = hip_err(hipMemcpyAsync(host, dev, sizeof(host), hipMemcpyDeviceToHost, s));
    if (rc == CRDT_OK) rc = hip_err(hipStreamSynchronize(s));
    if (rc == CRDT_OK) *mhz = host[1] ? (double)host[0] / ((double)host[1] / ((double)wall_khz * 1e3)) / 1e6 : 0.0;
    return c.end(rc);
}

/* ---------------- validation (host) ---------------- */

}  // extern "C"

// Pointers, slot bounds, live counts and (keys = true) the key order.  The
// *_batch calls check only the layout here (O(documents)) and the key order
// on the device after the upload (pack.hip, check_order_kernel), whose verdict
// the merge's first kernel reads before doing anything (Work::gate).
static int validate_batch(const crdt_awset_batch* b, bool keys) {
    if (!b || !b->offsets || b->R == 0 || b->R > CRDT_MAX_R) return CRDT_E_INVALID;
    if (b->n_docs && (!b->vv || ((b->offsets[b->n_docs] > b->offsets[0]) && (!b->keys || !b->actors || !b->counters))))
        return CRDT_E_INVALID;
    for (uint32_t d = 0; d < b->n_docs; d++) {
        const uint32_t o = b->offsets[d], e = b->offsets[d + 1];
        if (e < o) return CRDT_E_INVALID;
        const uint32_t n = b->counts ? b->counts[d] : e - o;
        if (n > e - o) return CRDT_E_CAPACITY;
        if (keys)
            for (uint32_t i = o + 1; i < o + n; i++)
                if (b->keys[i] <= b->keys[i - 1]) return CRDT_E_UNSORTED;
    }
    return CRDT_OK;
}

static int validate_src_batch(const crdt_src_batch* s, bool keys) {
    if (!src_ptrs_ok(s)) return CRDT_E_INVALID;
    const uint32_t ns = s->doc_srcs[s->n_docs];
    for (uint32_t d = 0; d < s->n_docs; d++)
        if (s->doc_srcs[d + 1] < s->doc_srcs[d]) return CRDT_E_INVALID;
    if (ns && !s->vv) return CRDT_E_INVALID;
    for (uint32_t k = 0; k < ns; k++) {
        const uint32_t o = s->entry_off[k], e = s->entry_off[k + 1];
        if (e < o) return CRDT_E_INVALID;
        if (keys)
            for (uint32_t i = o + 1; i < e; i++)
                if (s->keys[i] <= s->keys[i - 1]) return CRDT_E_UNSORTED;
        if (s->tomb_off) {
            const uint32_t to = s->tomb_off[k], te = s->tomb_off[k + 1];
            if (te < to) return CRDT_E_INVALID;
            if (keys)
                for (uint32_t i = to + 1; i < te; i++)
                    if (s->tkeys[i] <= s->tkeys[i - 1]) return CRDT_E_UNSORTED;
        }
    }
    return CRDT_OK;
}

extern "C" {

int crdt_validate_batch(const crdt_awset_batch* b) { return validate_batch(b, true); }

int crdt_validate_src_batch(const crdt_src_batch* s) { return validate_src_batch(s, true); }

int crdt_validate_tomb_batch(const crdt_tomb_batch* t, uint32_t n_docs) {
    if (!t || !t->offsets) return CRDT_E_INVALID;
    if (n_docs && t->offsets[n_docs] > t->offsets[0] && (!t->keys || !t->actors || !t->counters))
        return CRDT_E_INVALID;
    for (uint32_t d = 0; d < n_docs; d++) {
        const uint32_t o = t->offsets[d], e = t->offsets[d + 1];
        if (e < o) return CRDT_E_INVALID;
        const uint32_t n = t->counts ? t->counts[d] : e - o;
        if (n > e - o) return CRDT_E_CAPACITY;
        for (uint32_t i = o + 1; i < o + n; i++)
            if (t->keys[i] <= t->keys[i - 1]) return CRDT_E_UNSORTED;
    }
    return CRDT_OK;
}

/* ---------------- synchronous host-buffer path ---------------- */

}  // extern "C"

namespace {

// Diagnostics (CRDT_TRACE_STAGE): host time between the phases of a batch call.
struct PhaseClock {
    const char* what;
    bool on = std::getenv("CRDT_TRACE_STAGE") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    explicit PhaseClock(const char* w) : what(w) {}
    void mark(const char* phase) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "%s: %s %.3f ms\n", what, phase, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

constexpr int kStageSlots = 48;  // ctx->stage: per-array device buffers of one call

// The device copies of a host-path call's arrays.  Input arrays that lie in one
// crdt_host_alloc block are staged by ONE copy of the span they cover: each
// runtime H2D copy call costs the host 1-7 ms before its DMA is even
// submitted, whatever its size (profiles/r05i_boundary_timeline.txt), while
// the span moves at PCIe rate.  Other arrays, and output rooms, get a buffer of
// their own.  A call runs its input staging twice: first planning (plan():
// nothing is allocated, only the span the call's arrays cover is measured),
// then for real, so the device image is the size of that span, not of the
// whole block.
struct Stager {
    crdt_ctx* ctx;
    bool planning = false;
    int next = 0;
    int rc = CRDT_OK;
    uintptr_t blk = 0;  // the host block of the call's inputs (the first one met)
    size_t blk_size = 0;
    size_t lo = SIZE_MAX, hi = 0;  // the span of it the call covers
    size_t img_lo = 0;             // block offset of the device image's first byte
    char* dimg = nullptr;
    bool flushed = false;
    template <typename T>
    T* put(const T* host, size_t n) {  // allocate + copy in (n elements)
        if (rc != CRDT_OK) return nullptr;
        static const bool trace = std::getenv("CRDT_TRACE_STAGE") != nullptr;  // diagnostics: host time per step
        static const bool span = std::getenv("CRDT_NO_SPAN_STAGING") == nullptr;
        const uintptr_t a = (uintptr_t)host;
        const size_t bytes = n * sizeof(T);
        if (planning) {
            if (span && ctx->span_staging && host && n) {
                uintptr_t b0 = 0;
                size_t sz = 0;
                if (!blk && host_block(host, b0, sz)) {
                    blk = b0;
                    blk_size = sz;
                }
                if (blk && a >= blk && a + bytes <= blk + blk_size) {
                    lo = std::min(lo, (size_t)(a - blk));
                    hi = std::max(hi, (size_t)(a - blk) + bytes);
                }
            }
            return nullptr;
        }
        if (dimg && host && n && a >= blk + img_lo && a + bytes <= blk + hi) {
            const size_t off = a - blk - img_lo;
            // staged after the span went: its own copy, into the same image
            if (flushed && hipMemcpyAsync(dimg + off, host, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
                rc = CRDT_E_HIP;
            return reinterpret_cast<T*>(dimg + off);
        }
        if (next >= kStageSlots) {
            rc = CRDT_E_INVALID;
            return nullptr;
        }
        const auto t0 = std::chrono::steady_clock::now();
        DevBuf& b = ctx->stage[next++];
        rc = b.reserve(std::max<size_t>(n, 1) * sizeof(T));
        if (rc != CRDT_OK) return nullptr;
        const auto t1 = std::chrono::steady_clock::now();
        if (host && n && hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            rc = CRDT_E_HIP;
        if (trace) {
            const auto t2 = std::chrono::steady_clock::now();
            fprintf(stderr, "stage[%d] %zu B: reserve %.3f ms, copy call %.3f ms\n", next - 1, bytes,
                    std::chrono::duration<double, std::milli>(t1 - t0).count(),
                    std::chrono::duration<double, std::milli>(t2 - t1).count());
        }
        return b.as<T>();
    }
    template <typename T>
    T* room(size_t n) {
        return put<T>(nullptr, n);
    }
    // Run the call's input staging `f` planning, size the span's image, then run it for real.
    template <typename F>
    void plan(F&& f) {
        planning = true;
        f();
        planning = false;
        if (rc == CRDT_OK && blk && hi > lo) {
            img_lo = lo & ~(size_t)255;  // (the image keeps the block's 256-byte alignment)
            if (hi - img_lo <= ((size_t)4 << 30)) {  // (a larger span: array by array)
                rc = ctx->span_img.reserve(hi - img_lo);
                if (rc == CRDT_OK) dimg = ctx->span_img.as<char>();
            }
        }
        f();
    }
    // Copy the span of the host block that this call's arrays cover (one call).
    void flush() {
        if (rc == CRDT_OK && !flushed && dimg &&
            hipMemcpyAsync(dimg, reinterpret_cast<const char*>(blk) + img_lo, hi - img_lo, hipMemcpyHostToDevice,
                           ctx->stream) != hipSuccess)
            rc = CRDT_E_HIP;
        flushed = true;
    }
};

template <typename T>
int get(T* host, const T* dev, size_t n, hipStream_t s) {
    if (!n) return CRDT_OK;
    return hip_err(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
}

crdt_awset_batch stage_batch(Stager& st, const crdt_awset_batch* h) {
    crdt_awset_batch d = *h;
    const size_t slots = h->offsets[h->n_docs];
    d.offsets = st.put(h->offsets, (size_t)h->n_docs + 1);
    d.counts = h->counts ? st.put(h->counts, h->n_docs) : nullptr;
    d.keys = st.put(h->keys, slots);
    d.actors = st.put(h->actors, slots);
    d.counters = st.put(h->counters, slots);
    d.vv = st.put(h->vv, (size_t)h->n_docs * h->R);
    return d;
}

crdt_awset_out stage_out(Stager& st, uint32_t n_docs, uint32_t R, size_t slots) {
    crdt_awset_out o;
    o.offsets = st.room<uint32_t>((size_t)n_docs + 1);
    o.counts = st.room<uint32_t>(n_docs);
    o.keys = st.room<uint64_t>(slots);
    o.actors = st.room<uint32_t>(slots);
    o.counters = st.room<uint64_t>(slots);
    o.vv = st.room<uint64_t>((size_t)n_docs * R);
    return o;
}

// keys = false: the key column is shared with an output fetched before (exchange)
int fetch_out(const crdt_awset_out* h, const crdt_awset_out& d, uint32_t n_docs, uint32_t R, size_t slots,
              hipStream_t s, bool keys = true) {
    int rc = get(h->offsets, d.offsets, (size_t)n_docs + 1, s);
    if (rc == CRDT_OK) rc = get(h->counts, d.counts, n_docs, s);
    if (rc == CRDT_OK && keys) rc = get(h->keys, d.keys, slots, s);
    if (rc == CRDT_OK) rc = get(h->actors, d.actors, slots, s);
    if (rc == CRDT_OK) rc = get(h->counters, d.counters, slots, s);
    if (rc == CRDT_OK) rc = get(h->vv, d.vv, (size_t)n_docs * R, s);
    return rc;
}

// The key order of a staged batch (ranges off[r] .. + counts or off[r + 1]),
// checked on the device; a violation sets kErrUnsorted in the status word, which
// closes the merge's gate (Work::gate) and reads back as CRDT_E_UNSORTED.
int check_order(crdt_ctx* ctx, std::initializer_list<OrderRanges> sets) {
    return hip_err(launch_check_order(sets.begin(), (uint32_t)sets.size(), ctx->ws.as<uint32_t>(64),
                                      (uint32_t)ctx->n_cu, ctx->stream));
}

// The merge launch of a host-path call, gated on the device by its order checks.
template <typename F>
int gated(crdt_ctx* ctx, F&& launch) {
    ctx->call_gate = true;
    const int rc = launch();
    ctx->call_gate = false;
    ctx->call_tiles = 0;
    ctx->call_small = false;
    return rc;
}

// Tiles the join of host batches a <- b launches (tile.hip: ceil((nd + ns) / T)
// per document with more than 64 live entries on a side), so the tile path
// launches exactly the passes it needs (join_common).
uint64_t host_tiles(const crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b) {
    const uint64_t T = tile_positions(ctx->tile_shape);
    uint64_t t = 0;
    for (uint32_t d = 0; d < a->n_docs; ++d) {
        const uint64_t nd = a->counts ? a->counts[d] : a->offsets[d + 1] - a->offsets[d];
        const uint64_t ns = b->counts ? b->counts[d] : b->offsets[d + 1] - b->offsets[d];
        if (nd > 64 || ns > 64) t += (nd + ns + T - 1) / T;
    }
    return t;
}

// Before a host-path join's launch: the exact tile count, or no large-document
// path at all when no document has one (six launches fewer; 0 tiles <=> no
// document above 64 live entries on a side, whatever the tile options).
void plan_tiles(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b) {
    const uint64_t t = host_tiles(ctx, a, b);
    ctx->call_small = t == 0;
    ctx->call_tiles = std::max<uint64_t>(t, 1);
}

// The end of a host-path call: its one sync, then its status (read from the
// page-locked copy the gather kernel made when `copied`, else read back).
int finish(crdt_ctx* ctx, bool copied) {
    if (!copied || !ctx->host_status) return crdt_ctx_sync(ctx, ctx->stream);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return CRDT_E_HIP;
    const uint32_t st = __atomic_load_n(ctx->host_status, __ATOMIC_ACQUIRE);
    return st ? crdt_ctx_sync(ctx, ctx->stream) : CRDT_OK;  // (an error: the usual read-back and reset)
}

// Download merge outputs.  Default: at their capacity offsets, as the kernels
// wrote them.  pack_batch_outputs: only the live entries, gathered on the
// device at offsets computed on the device (pack_scan_kernel) -- an output
// whose host arrays all lie in crdt_host_alloc blocks is written there by the
// gather kernel itself (no copy call, no read-back: the call's one sync is its
// last); any other is gathered on the device, and the totals of all such
// outputs come back in ONE read-back before their copies.  keys[i] = false: an
// exchange's second output sharing the first's key column.
int fetch_outputs(crdt_ctx* ctx, Stager& st, int nout, const crdt_awset_out* const* h, const crdt_awset_out* d,
                  const bool* keys, uint32_t n, uint32_t R, size_t slots, bool* status_copied) {
    *status_copied = false;
    if (!ctx->pack_outputs) {
        int rc = CRDT_OK;
        for (int i = 0; i < nout && rc == CRDT_OK; ++i) rc = fetch_out(h[i], d[i], n, R, slots, ctx->stream, keys[i]);
        return rc;
    }
    static const bool no_zc = std::getenv("CRDT_NO_ZERO_COPY") != nullptr;  // diagnostics: copies only
    uint32_t* poff[2] = {nullptr, nullptr};
    uint32_t* hoff[2] = {nullptr, nullptr};
    OutView pk[2];
    bool zc[2] = {false, false};
    for (int i = 0; i < nout; ++i) {
        poff[i] = st.room<uint32_t>((size_t)n + 1);
        const uintptr_t ho = host_dev_addr(h[i]->offsets, ((size_t)n + 1) * 4),
                        hc = host_dev_addr(h[i]->counts, (size_t)n * 4),
                        hk = keys[i] ? host_dev_addr(h[i]->keys, slots * 8) : 1,
                        ha = host_dev_addr(h[i]->actors, slots * 4), hcc = host_dev_addr(h[i]->counters, slots * 8),
                        hv = host_dev_addr(h[i]->vv, (size_t)n * R * 8);
        zc[i] = !no_zc && ho && hc && hk && ha && hcc && hv;
        if (zc[i]) {
            hoff[i] = reinterpret_cast<uint32_t*>(ho);
            pk[i] = OutView{nullptr, reinterpret_cast<uint32_t*>(hc),
                            keys[i] ? reinterpret_cast<uint64_t*>(hk) : nullptr, reinterpret_cast<uint32_t*>(ha),
                            reinterpret_cast<uint64_t*>(hcc), reinterpret_cast<uint64_t*>(hv)};
        } else {
            pk[i] = OutView{nullptr, nullptr, keys[i] ? st.room<uint64_t>(slots) : nullptr, st.room<uint32_t>(slots),
                            st.room<uint64_t>(slots), nullptr};
        }
    }
    if (st.rc != CRDT_OK) return st.rc;
    const OutView in[2] = {view(&d[0]), nout > 1 ? view(&d[1]) : OutView{}};
    int rc = hip_err(launch_pack((uint32_t)nout, in, poff, hoff, pk, n, R, ctx->ws.as<uint32_t>(64), ctx->host_status,
                                 (uint32_t)ctx->n_cu, ctx->stream));
    *status_copied = rc == CRDT_OK && ctx->host_status != nullptr;
    if (rc != CRDT_OK || (zc[0] && (nout < 2 || zc[1]))) return rc;
    uint32_t tot[2] = {0, 0};
    for (int i = 0; i < nout && rc == CRDT_OK; ++i)
        if (!zc[i]) rc = get(&tot[i], poff[i] + n, 1, ctx->stream);
    if (rc == CRDT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = CRDT_E_HIP;
    for (int i = 0; i < nout && rc == CRDT_OK; ++i) {
        if (zc[i]) continue;
        if (tot[i] > slots) return CRDT_E_CAPACITY;  // (the scan clamps to capacity: never)
        rc = get(h[i]->offsets, poff[i], (size_t)n + 1, ctx->stream);
        if (rc == CRDT_OK) rc = get(h[i]->counts, d[i].counts, n, ctx->stream);
        if (rc == CRDT_OK && keys[i]) rc = get(h[i]->keys, pk[i].keys, tot[i], ctx->stream);
        if (rc == CRDT_OK) rc = get(h[i]->actors, pk[i].actors, tot[i], ctx->stream);
        if (rc == CRDT_OK) rc = get(h[i]->counters, pk[i].counters, tot[i], ctx->stream);
        if (rc == CRDT_OK) rc = get(h[i]->vv, d[i].vv, (size_t)n * R, ctx->stream);
    }
    return rc;
}

}  // namespace

extern "C" {

int crdt_awset_sort_batch(crdt_ctx* ctx, const crdt_awset_batch* in, const crdt_awset_out* out) {
    if (!ctx || !in || !in->offsets || !out_ptrs_ok(out) || in->R == 0 || in->R > CRDT_MAX_R) return CRDT_E_INVALID;
    const uint32_t n = in->n_docs;
    const size_t slots = in->offsets[n];
    int rc = set_device(ctx);
    if (rc != CRDT_OK) return rc;
    Stager st{ctx};
    crdt_awset_batch di{};
    st.plan([&] { di = stage_batch(st, in); });
    crdt_awset_out dout = stage_out(st, n, in->R, slots);
    st.flush();  // the inputs' span, if they lie in one crdt_host_alloc block
    if (st.rc != CRDT_OK) return st.rc;
    rc = crdt_awset_sort_async(ctx, &di, (uint32_t)slots, &dout, ctx->stream);
    if (rc == CRDT_OK) rc = fetch_out(out, dout, n, in->R, slots, ctx->stream);
    const int sync = crdt_ctx_sync(ctx, ctx->stream);
    return rc != CRDT_OK ? rc : sync;
}

int crdt_awset_apply_batch(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_tomb_batch* tombs,
                           const crdt_op_batch* ops, const crdt_awset_out* out, const crdt_tomb_out* tomb_out) {
    if (!ctx || !ops || !ops->op_off || !ops->doc_actor || !out_ptrs_ok(out)) return CRDT_E_INVALID;
    int rc = crdt_validate_batch(state);
    if (rc != CRDT_OK) return rc;
    if (ops->n_docs != state->n_docs) return CRDT_E_INVALID;
    const uint32_t n = state->n_docs;
    if (tombs && (rc = crdt_validate_tomb_batch(tombs, n)) != CRDT_OK) return rc;
    const size_t nops = ops->op_off[n];
    if (nops && (!ops->kind || !ops->keys)) return CRDT_E_INVALID;
    const uint64_t slots = (uint64_t)state->offsets[n] + nops;
    const uint64_t tin = tombs ? tombs->offsets[n] : 0;
    if (slots >= (1ull << 32) || tin + nops >= (1ull << 32)) return CRDT_E_INVALID;
    if ((rc = set_device(ctx)) != CRDT_OK) return rc;
    Stager st{ctx};
    crdt_awset_batch ds{};
    crdt_op_batch dops = *ops;
    crdt_tomb_batch dt{};
    st.plan([&] {
        ds = stage_batch(st, state);
        dops.op_off = st.put(ops->op_off, (size_t)n + 1);
        dops.kind = st.put(ops->kind, nops);
        dops.keys = st.put(ops->keys, nops);
        dops.doc_actor = st.put(ops->doc_actor, n);
        if (tombs) {
            dt.offsets = st.put(tombs->offsets, (size_t)n + 1);
            dt.counts = tombs->counts ? st.put(tombs->counts, n) : nullptr;
            dt.keys = st.put(tombs->keys, tin);
            dt.actors = st.put(tombs->actors, tin);
            dt.counters = st.put(tombs->counters, tin);
        }
    });
    crdt_awset_out dout = stage_out(st, n, state->R, slots);
    crdt_tomb_out dto{};
    if (tomb_out) {
        dto.offsets = st.room<uint32_t>((size_t)n + 1);
        dto.counts = st.room<uint32_t>(n);
        dto.keys = st.room<uint64_t>(tin + nops);
        dto.actors = st.room<uint32_t>(tin + nops);
        dto.counters = st.room<uint64_t>(tin + nops);
    }
    st.flush();  // the inputs' span, if they lie in one crdt_host_alloc block
    if (st.rc != CRDT_OK) return st.rc;
    rc = crdt_awset_apply_async(ctx, &ds, tombs ? &dt : nullptr, &dops, &dout, tomb_out ? &dto : nullptr,
                                ctx->stream);
    if (rc == CRDT_OK) rc = fetch_out(out, dout, n, state->R, slots, ctx->stream);
    if (rc == CRDT_OK && tomb_out) {
        rc = get(tomb_out->offsets, dto.offsets, (size_t)n + 1, ctx->stream);
        if (rc == CRDT_OK) rc = get(tomb_out->counts, dto.counts, n, ctx->stream);
        if (rc == CRDT_OK) rc = get(tomb_out->keys, dto.keys, tin + nops, ctx->stream);
        if (rc == CRDT_OK) rc = get(tomb_out->actors, dto.actors, tin + nops, ctx->stream);
        if (rc == CRDT_OK) rc = get(tomb_out->counters, dto.counters, tin + nops, ctx->stream);
    }
    const int sync = crdt_ctx_sync(ctx, ctx->stream);
    return rc != CRDT_OK ? rc : sync;
}

// The merge calls below make one host sync each (their last): the inputs go up
// (one copy of their span when they lie in one crdt_host_alloc block), the key
// order is checked on the device, the merge's first kernel reads that verdict
// (a batch out of order reaches no merge, Work::gate), and the outputs come
// back (fetch_outputs: with pack_batch_outputs into page-locked outputs, by
// the gather kernel itself).
int crdt_awset_join_batch(crdt_ctx* ctx, const crdt_awset_batch* dst, const crdt_awset_batch* src,
                          const crdt_awset_out* out) {
    if (!ctx || !out_ptrs_ok(out)) return CRDT_E_INVALID;
    int rc = validate_batch(dst, false);
    if (rc == CRDT_OK) rc = validate_batch(src, false);
    if (rc != CRDT_OK) return rc;
    if (dst->n_docs != src->n_docs || dst->R != src->R) return CRDT_E_INVALID;
    if ((uint64_t)dst->offsets[dst->n_docs] + src->offsets[src->n_docs] >= (1ull << 32)) return CRDT_E_INVALID;
    if ((rc = set_device(ctx)) != CRDT_OK) return rc;
    Stager st{ctx};
    crdt_awset_batch dd{}, ds{};
    st.plan([&] {
        dd = stage_batch(st, dst);
        ds = stage_batch(st, src);
    });
    const size_t slots = (size_t)dst->offsets[dst->n_docs] + src->offsets[src->n_docs];
    crdt_awset_out dout = stage_out(st, dst->n_docs, dst->R, slots);
    st.flush();  // the inputs' span, if they lie in one crdt_host_alloc block
    if (st.rc != CRDT_OK) return st.rc;
    rc = check_order(ctx, {{dd.offsets, dd.counts, dd.n_docs, dd.keys}, {ds.offsets, ds.counts, ds.n_docs, ds.keys}});
    plan_tiles(ctx, dst, src);
    if (rc == CRDT_OK) rc = gated(ctx, [&] { return crdt_awset_join_async(ctx, &dd, &ds, &dout, ctx->stream); });
    const crdt_awset_out* hs[1] = {out};
    const bool keys[1] = {true};
    bool copied = false;
    if (rc == CRDT_OK) rc = fetch_outputs(ctx, st, 1, hs, &dout, keys, dst->n_docs, dst->R, slots, &copied);
    ctx->call_tiles = 0;
    ctx->call_small = false;
    const int sync = finish(ctx, copied);
    return rc != CRDT_OK ? rc : sync;
}

int crdt_awset_exchange_batch(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b,
                              const crdt_awset_out* out_ab, const crdt_awset_out* out_ba) {
    if (!ctx || !out_ptrs_ok(out_ab) || !out_ptrs_ok(out_ba)) return CRDT_E_INVALID;
    int rc = validate_batch(a, false);
    if (rc == CRDT_OK) rc = validate_batch(b, false);
    if (rc != CRDT_OK) return rc;
    if (a->n_docs != b->n_docs || a->R != b->R) return CRDT_E_INVALID;
    if ((uint64_t)a->offsets[a->n_docs] + b->offsets[b->n_docs] >= (1ull << 32)) return CRDT_E_INVALID;
    if ((rc = set_device(ctx)) != CRDT_OK) return rc;
    PhaseClock pc("exchange_batch");
    Stager st{ctx};
    crdt_awset_batch da{}, db{};
    st.plan([&] {
        da = stage_batch(st, a);
        db = stage_batch(st, b);
    });
    const size_t slots = (size_t)a->offsets[a->n_docs] + b->offsets[b->n_docs];
    crdt_awset_out o[2] = {stage_out(st, a->n_docs, a->R, slots), stage_out(st, a->n_docs, a->R, slots)};
    st.flush();  // the inputs' span, if they lie in one crdt_host_alloc block
    if (st.rc != CRDT_OK) return st.rc;
    // host outputs sharing one key column: one device column, written and fetched once
    const bool share = out_ab->keys == out_ba->keys;
    if (share) o[1].keys = o[0].keys;
    pc.mark("stage issued");
    rc = check_order(ctx, {{da.offsets, da.counts, da.n_docs, da.keys}, {db.offsets, db.counts, db.n_docs, db.keys}});
    plan_tiles(ctx, a, b);
    if (rc == CRDT_OK) rc = gated(ctx, [&] { return crdt_awset_exchange_async(ctx, &da, &db, &o[0], &o[1], ctx->stream); });
    pc.mark("order checks + kernels issued");
    const crdt_awset_out* hs[2] = {out_ab, out_ba};
    const bool keys[2] = {true, !share};
    bool copied = false;
    if (rc == CRDT_OK) rc = fetch_outputs(ctx, st, 2, hs, o, keys, a->n_docs, a->R, slots, &copied);
    ctx->call_tiles = 0;
    ctx->call_small = false;
    pc.mark("fetches issued");
    const int sync = finish(ctx, copied);
    pc.mark("synced");
    return rc != CRDT_OK ? rc : sync;
}

int crdt_awset_fold_batch(crdt_ctx* ctx, int mode, const crdt_awset_batch* dst, const crdt_src_batch* srcs,
                          const crdt_awset_out* out) {
    if (!ctx || !out_ptrs_ok(out)) return CRDT_E_INVALID;
    int rc = validate_batch(dst, false);
    if (rc == CRDT_OK) rc = validate_src_batch(srcs, false);
    if (rc != CRDT_OK) return rc;
    if (dst->n_docs != srcs->n_docs || dst->R != srcs->R) return CRDT_E_INVALID;
    const uint32_t ns = srcs->doc_srcs[srcs->n_docs];
    const uint64_t total = (uint64_t)dst->offsets[dst->n_docs] + srcs->entry_off[ns];
    if (total >= (1ull << 32)) return CRDT_E_INVALID;
    if ((rc = set_device(ctx)) != CRDT_OK) return rc;
    if ((rc = reserve_scratch(ctx, total)) != CRDT_OK) return rc;
    Stager st{ctx};
    crdt_awset_batch dd{};
    crdt_src_batch ds = *srcs;
    const size_t ne = srcs->entry_off[ns];
    const size_t nt = srcs->tomb_off ? srcs->tomb_off[ns] : 0;
    st.plan([&] {
        dd = stage_batch(st, dst);
        ds.doc_srcs = st.put(srcs->doc_srcs, (size_t)srcs->n_docs + 1);
        ds.src_actor = st.put(srcs->src_actor, ns);
        ds.vv = st.put(srcs->vv, (size_t)ns * srcs->R);
        ds.entry_off = st.put(srcs->entry_off, (size_t)ns + 1);
        ds.keys = st.put(srcs->keys, ne);
        ds.actors = st.put(srcs->actors, ne);
        ds.counters = st.put(srcs->counters, ne);
        if (srcs->tomb_off) {
            ds.tomb_off = st.put(srcs->tomb_off, (size_t)ns + 1);
            ds.tkeys = st.put(srcs->tkeys, nt);
            ds.tactors = st.put(srcs->tactors, nt);
            ds.tcounters = st.put(srcs->tcounters, nt);
        }
    });
    crdt_awset_out dout = stage_out(st, dst->n_docs, dst->R, total);
    st.flush();  // the inputs' span, if they lie in one crdt_host_alloc block
    if (st.rc != CRDT_OK) return st.rc;
    rc = srcs->tomb_off ? check_order(ctx, {{dd.offsets, dd.counts, dd.n_docs, dd.keys}, {ds.entry_off, nullptr, ns, ds.keys},
                                            {ds.tomb_off, nullptr, ns, ds.tkeys}})
                        : check_order(ctx, {{dd.offsets, dd.counts, dd.n_docs, dd.keys}, {ds.entry_off, nullptr, ns, ds.keys}});
    if (rc == CRDT_OK) rc = gated(ctx, [&] { return crdt_awset_fold_async(ctx, mode, &dd, &ds, &dout, ctx->stream); });
    const crdt_awset_out* hs[1] = {out};
    const bool keys[1] = {true};
    bool copied = false;
    if (rc == CRDT_OK) rc = fetch_outputs(ctx, st, 1, hs, &dout, keys, dst->n_docs, dst->R, total, &copied);
    const int sync = finish(ctx, copied);
    return rc != CRDT_OK ? rc : sync;
}

// Two syncs: the packed totals come back first (8 bytes), then exactly the
// live prefix of each entry and tombstone array.
int crdt_awset_delta_extract_batch(crdt_ctx* ctx, const crdt_src_batch* srcs, const uint64_t* peer_vv,
                                   const crdt_delta_out* out) {
    if (!ctx || !out) return CRDT_E_INVALID;
    int rc = validate_src_batch(srcs, false);
    if (rc != CRDT_OK) return rc;
    if (srcs->n_docs && !peer_vv) return CRDT_E_INVALID;
    if (!out->doc_srcs || !out->src_actor || !out->vv || !out->entry_off || !out->keys || !out->actors ||
        !out->counters)
        return CRDT_E_INVALID;
    if (srcs->tomb_off && (!out->tomb_off || !out->tkeys || !out->tactors || !out->tcounters)) return CRDT_E_INVALID;
    const uint32_t n = srcs->n_docs, R = srcs->R;
    const uint32_t ns = srcs->doc_srcs[n];
    const size_t ne = srcs->entry_off[ns];
    const size_t nt = srcs->tomb_off ? srcs->tomb_off[ns] : 0;
    if (srcs->doc_srcs[0] != 0 || (ne && (!srcs->keys || !srcs->actors || !srcs->counters))) return CRDT_E_INVALID;
    if ((rc = set_device(ctx)) != CRDT_OK) return rc;
    Stager st{ctx};
    crdt_src_batch ds = *srcs;
    const uint64_t* dpeer = nullptr;
    st.plan([&] {
        ds.doc_srcs = st.put(srcs->doc_srcs, (size_t)n + 1);
        ds.src_actor = st.put(srcs->src_actor, ns);
        ds.vv = st.put(srcs->vv, (size_t)ns * R);
        ds.entry_off = st.put(srcs->entry_off, (size_t)ns + 1);
        ds.keys = st.put(srcs->keys, ne);
        ds.actors = st.put(srcs->actors, ne);
        ds.counters = st.put(srcs->counters, ne);
        if (srcs->tomb_off) {
            ds.tomb_off = st.put(srcs->tomb_off, (size_t)ns + 1);
            ds.tkeys = st.put(srcs->tkeys, nt);
            ds.tactors = st.put(srcs->tactors, nt);
            ds.tcounters = st.put(srcs->tcounters, nt);
        }
        dpeer = st.put(peer_vv, (size_t)n * R);
    });
    crdt_delta_out dout{};
    dout.doc_srcs = st.room<uint32_t>((size_t)n + 1);
    dout.src_actor = st.room<uint32_t>(ns);
    dout.vv = st.room<uint64_t>((size_t)ns * R);
    dout.entry_off = st.room<uint32_t>((size_t)ns + 1);
    dout.keys = st.room<uint64_t>(ne);
    dout.actors = st.room<uint32_t>(ne);
    dout.counters = st.room<uint64_t>(ne);
    dout.tomb_off = st.room<uint32_t>((size_t)ns + 1);
    dout.tkeys = st.room<uint64_t>(nt);
    dout.tactors = st.room<uint32_t>(nt);
    dout.tcounters = st.room<uint64_t>(nt);
    dout.kind = st.room<uint8_t>(ns);
    st.flush();  // the inputs' span, if they lie in one crdt_host_alloc block
    if (st.rc != CRDT_OK) return st.rc;
    rc = srcs->tomb_off ? check_order(ctx, {{ds.entry_off, nullptr, ns, ds.keys}, {ds.tomb_off, nullptr, ns, ds.tkeys}})
                        : check_order(ctx, {{ds.entry_off, nullptr, ns, ds.keys}});
    if (rc == CRDT_OK)
        rc = gated(ctx, [&] { return crdt_awset_delta_extract_async(ctx, &ds, dpeer, &dout, ctx->stream); });
    uint32_t tot_e = 0, tot_t = 0;
    if (rc == CRDT_OK) rc = get(&tot_e, dout.entry_off + ns, 1, ctx->stream);
    if (rc == CRDT_OK) rc = get(&tot_t, dout.tomb_off + ns, 1, ctx->stream);
    int sync = crdt_ctx_sync(ctx, ctx->stream);  // (an order violation ends the call here)
    if (rc != CRDT_OK || sync != CRDT_OK) return rc != CRDT_OK ? rc : sync;
    if (tot_e > ne || tot_t > nt) return CRDT_E_CAPACITY;  // (the kept are a subset of the input: never)
    rc = get(out->doc_srcs, dout.doc_srcs, (size_t)n + 1, ctx->stream);
    if (rc == CRDT_OK) rc = get(out->src_actor, dout.src_actor, ns, ctx->stream);
    if (rc == CRDT_OK) rc = get(out->vv, dout.vv, (size_t)ns * R, ctx->stream);
    if (rc == CRDT_OK) rc = get(out->entry_off, dout.entry_off, (size_t)ns + 1, ctx->stream);
    if (rc == CRDT_OK) rc = get(out->keys, dout.keys, tot_e, ctx->stream);
    if (rc == CRDT_OK) rc = get(out->actors, dout.actors, tot_e, ctx->stream);
    if (rc == CRDT_OK) rc = get(out->counters, dout.counters, tot_e, ctx->stream);
    if (rc == CRDT_OK && out->tomb_off) rc = get(out->tomb_off, dout.tomb_off, (size_t)ns + 1, ctx->stream);
    if (rc == CRDT_OK && srcs->tomb_off) {
        rc = get(out->tkeys, dout.tkeys, tot_t, ctx->stream);
        if (rc == CRDT_OK) rc = get(out->tactors, dout.tactors, tot_t, ctx->stream);
        if (rc == CRDT_OK) rc = get(out->tcounters, dout.tcounters, tot_t, ctx->stream);
    }
    if (rc == CRDT_OK && out->kind) rc = get(out->kind, dout.kind, ns, ctx->stream);
    sync = crdt_ctx_sync(ctx, ctx->stream);
    return rc != CRDT_OK ? rc : sync;
}

// For tests and small callers (include/crdtgpu.h): the query lists and the slot
// layout are checked here, the key order on the device; a state out of order
// reaches no lookup (Work::gate).
int crdt_awset_has_batch(crdt_ctx* ctx, const crdt_awset_batch* state, const crdt_query_batch* q,
                         const crdt_query_out* out) {
    if (!ctx || !state || !q || !out || !state->offsets || state->R == 0 || state->R > CRDT_MAX_R)
        return CRDT_E_INVALID;
    if (!q->q_off || !out->found || (q->n_queries && !q->keys) || q->n_docs != state->n_docs ||
        (out->actors == nullptr) != (out->counters == nullptr))
        return CRDT_E_INVALID;
    const uint32_t n = state->n_docs, nq = q->n_queries;
    if (q->q_off[0] != 0 || q->q_off[n] != nq) return CRDT_E_INVALID;
    for (uint32_t d = 0; d < n; ++d)
        if (q->q_off[d + 1] < q->q_off[d]) return CRDT_E_INVALID;
    const bool dots = out->actors != nullptr;
    for (uint32_t d = 0; d < n; ++d) {
        const uint32_t o = state->offsets[d], e = state->offsets[d + 1];
        if (e < o) return CRDT_E_INVALID;
        if ((state->counts ? state->counts[d] : e - o) > e - o) return CRDT_E_CAPACITY;
    }
    const size_t slots = state->offsets[n];
    if (n && slots > state->offsets[0] && (!state->keys || (dots && (!state->actors || !state->counters))))
        return CRDT_E_INVALID;
    if (nq == 0) return CRDT_OK;
    int rc = set_device(ctx);
    if (rc != CRDT_OK) return rc;
    Stager st{ctx};
    crdt_awset_batch ds = *state;
    crdt_query_batch dq = *q;
    st.plan([&] {
        ds.offsets = st.put(state->offsets, (size_t)n + 1);
        ds.counts = state->counts ? st.put(state->counts, n) : nullptr;
        ds.keys = st.put(state->keys, slots);
        ds.actors = dots ? st.put(state->actors, slots) : nullptr;
        ds.counters = dots ? st.put(state->counters, slots) : nullptr;
        dq.q_off = st.put(q->q_off, (size_t)n + 1);
        dq.keys = st.put(q->keys, nq);
    });
    ds.vv = nullptr;  // (not read)
    crdt_query_out dout{};
    dout.found = st.room<uint8_t>(nq);
    dout.actors = dots ? st.room<uint32_t>(nq) : nullptr;
    dout.counters = dots ? st.room<uint64_t>(nq) : nullptr;
    st.flush();  // the inputs' span, if they lie in one crdt_host_alloc block
    if (st.rc != CRDT_OK) return st.rc;
    rc = check_order(ctx, {{ds.offsets, ds.counts, n, ds.keys}});
    if (rc == CRDT_OK) rc = gated(ctx, [&] { return crdt_awset_has_async(ctx, &ds, &dq, &dout, ctx->stream); });
    int sync = crdt_ctx_sync(ctx, ctx->stream);  // (an order violation ends the call here)
    if (rc != CRDT_OK || sync != CRDT_OK) return rc != CRDT_OK ? rc : sync;
    rc = get(out->found, dout.found, nq, ctx->stream);
    if (rc == CRDT_OK && dots) rc = get(out->actors, dout.actors, nq, ctx->stream);
    if (rc == CRDT_OK && dots) rc = get(out->counters, dout.counters, nq, ctx->stream);
    sync = crdt_ctx_sync(ctx, ctx->stream);
    return rc != CRDT_OK ? rc : sync;
}

// For tests and small callers (include/crdtgpu.h): the slot layouts are checked
// here, the key order on the device; batches out of order reach no compare
// (Work::gate).
int crdt_awset_compare_batch(crdt_ctx* ctx, const crdt_awset_batch* a, const crdt_awset_batch* b, uint32_t mask,
                             const crdt_compare_out* out) {
    if (!ctx || !out || !out->flags) return CRDT_E_INVALID;
    int rc = validate_batch(a, false);
    if (rc == CRDT_OK) rc = validate_batch(b, false);
    if (rc != CRDT_OK) return rc;
    if (a->n_docs != b->n_docs || a->R != b->R || mask > 15u) return CRDT_E_INVALID;
    if ((out->worklist == nullptr) != (out->n_work == nullptr)) return CRDT_E_INVALID;
    const uint32_t n = a->n_docs;
    if ((rc = set_device(ctx)) != CRDT_OK) return rc;
    Stager st{ctx};
    crdt_awset_batch da = *a, db = *b;
    st.plan([&] {
        da = stage_batch(st, a);
        db = stage_batch(st, b);
    });
    crdt_compare_out dout{};
    dout.flags = st.room<uint8_t>(n);
    dout.summary = out->summary ? st.room<uint32_t>(5) : nullptr;
    dout.worklist = out->worklist ? st.room<uint32_t>(n) : nullptr;
    dout.n_work = out->worklist ? st.room<uint32_t>(1) : nullptr;
    st.flush();  // the inputs' span, if they lie in one crdt_host_alloc block
    if (st.rc != CRDT_OK) return st.rc;
    rc = check_order(ctx, {{da.offsets, da.counts, n, da.keys}, {db.offsets, db.counts, n, db.keys}});
    if (rc == CRDT_OK) rc = gated(ctx, [&] { return crdt_awset_compare_async(ctx, &da, &db, mask, &dout, ctx->stream); });
    uint32_t nw = 0;
    if (rc == CRDT_OK && out->worklist) rc = get(&nw, dout.n_work, 1, ctx->stream);
    int sync = crdt_ctx_sync(ctx, ctx->stream);  // (an order violation ends the call here)
    if (rc != CRDT_OK || sync != CRDT_OK) return rc != CRDT_OK ? rc : sync;
    if (nw > n) return CRDT_E_CAPACITY;  // (the list is a subset of the documents: never)
    rc = get(out->flags, dout.flags, n, ctx->stream);
    if (rc == CRDT_OK && out->summary) rc = get(out->summary, dout.summary, 5, ctx->stream);
    if (rc == CRDT_OK && out->worklist) rc = get(out->worklist, dout.worklist, nw, ctx->stream);
    if (rc == CRDT_OK && out->worklist) *out->n_work = nw;
    sync = crdt_ctx_sync(ctx, ctx->stream);
    return rc != CRDT_OK ? rc : sync;
}

// For tests and small callers (include/crdtgpu.h): the slot layouts are checked
// here, the key order on the device; batches out of order reach no diff
// (Work::gate).  Only flags, summary, the offsets and the live part of each list
// come back: never a state.
int crdt_awset_diff_batch(crdt_ctx* ctx, const crdt_awset_batch* before, const crdt_awset_batch* after,
                          uint32_t rem_slots, uint32_t ups_slots, const crdt_diff_out* out) {
    if (!ctx || !out) return CRDT_E_INVALID;
    int rc = validate_batch(before, false);
    if (rc == CRDT_OK) rc = validate_batch(after, false);
    if (rc != CRDT_OK) return rc;
    if (before->n_docs != after->n_docs || before->R != after->R) return CRDT_E_INVALID;
    if (!diff_out_ok(out, before, after, rem_slots, ups_slots)) return CRDT_E_INVALID;
    const uint32_t n = before->n_docs;
    if ((rc = set_device(ctx)) != CRDT_OK) return rc;
    Stager st{ctx};
    crdt_awset_batch db = *before, da = *after;
    st.plan([&] {
        db = stage_batch(st, before);
        da = stage_batch(st, after);
    });
    crdt_diff_out dout{};
    dout.flags = st.room<uint8_t>(n);
    dout.summary = out->summary ? st.room<uint32_t>(5) : nullptr;
    dout.rem_off = st.room<uint32_t>((size_t)n + 1);
    dout.ups_off = st.room<uint32_t>((size_t)n + 1);
    dout.rem_keys = st.room<uint64_t>(rem_slots);
    dout.ups_keys = st.room<uint64_t>(ups_slots);
    if (out->rem_actors) {
        dout.rem_actors = st.room<uint32_t>(rem_slots);
        dout.rem_counters = st.room<uint64_t>(rem_slots);
    }
    if (out->ups_actors) {
        dout.ups_actors = st.room<uint32_t>(ups_slots);
        dout.ups_counters = st.room<uint64_t>(ups_slots);
    }
    dout.ups_kind = out->ups_kind ? st.room<uint8_t>(ups_slots) : nullptr;
    st.flush();  // the inputs' span, if they lie in one crdt_host_alloc block
    if (st.rc != CRDT_OK) return st.rc;
    rc = check_order(ctx, {{db.offsets, db.counts, n, db.keys}, {da.offsets, da.counts, n, da.keys}});
    if (rc == CRDT_OK)
        rc = gated(ctx, [&] { return crdt_awset_diff_async(ctx, &db, &da, rem_slots, ups_slots, &dout, ctx->stream); });
    uint32_t tot[2] = {0, 0};
    if (rc == CRDT_OK) rc = get(&tot[0], dout.rem_off + n, 1, ctx->stream);
    if (rc == CRDT_OK) rc = get(&tot[1], dout.ups_off + n, 1, ctx->stream);
    int sync = crdt_ctx_sync(ctx, ctx->stream);  // (an order violation ends the call here)
    if (rc != CRDT_OK) return rc;
    if (sync != CRDT_OK && sync != CRDT_E_CAPACITY) return sync;
    const int verdict = sync;  // CRDT_E_CAPACITY: a list did not fit; the offsets and totals still come back
    const size_t nr = std::min(tot[0], rem_slots), nu = std::min(tot[1], ups_slots);
    rc = get(out->flags, dout.flags, n, ctx->stream);
    if (rc == CRDT_OK && out->summary) rc = get(out->summary, dout.summary, 5, ctx->stream);
    if (rc == CRDT_OK) rc = get(out->rem_off, dout.rem_off, (size_t)n + 1, ctx->stream);
    if (rc == CRDT_OK) rc = get(out->ups_off, dout.ups_off, (size_t)n + 1, ctx->stream);
    if (rc == CRDT_OK && out->rem_keys) rc = get(out->rem_keys, dout.rem_keys, nr, ctx->stream);
    if (rc == CRDT_OK && out->rem_actors) rc = get(out->rem_actors, dout.rem_actors, nr, ctx->stream);
    if (rc == CRDT_OK && out->rem_counters) rc = get(out->rem_counters, dout.rem_counters, nr, ctx->stream);
    if (rc == CRDT_OK && out->ups_keys) rc = get(out->ups_keys, dout.ups_keys, nu, ctx->stream);
    if (rc == CRDT_OK && out->ups_actors) rc = get(out->ups_actors, dout.ups_actors, nu, ctx->stream);
    if (rc == CRDT_OK && out->ups_counters) rc = get(out->ups_counters, dout.ups_counters, nu, ctx->stream);
    if (rc == CRDT_OK && out->ups_kind) rc = get(out->ups_kind, dout.ups_kind, nu, ctx->stream);
    sync = crdt_ctx_sync(ctx, ctx->stream);
    return rc != CRDT_OK ? rc : (sync != CRDT_OK ? sync : verdict);
}

}  // extern "C"
