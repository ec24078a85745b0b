// What replica.hip shares with replica_inplace.hip, and the in-place scatter's
// kernel arguments (crdt_replica_scatter_inplace_async; include/crdtgpu.h).
#pragma once
#include "crdt_device.hpp"

namespace crdt {

// The scatter's inverse map (replica_fill_kernel, replica_map_kernel; replica.hip):
// inv[d] = the lowest j < *n_idx with idx[j] == d, or 0xFFFFFFFF.  Reports *n_idx
// above n_sub (clamped, kErrCapacity), an idx[j] that is no document and a
// document named twice (kErrIndex).  n_docs > 0.
hipError_t launch_replica_map(const uint32_t* idx, const uint32_t* n_idx, uint32_t n_sub, uint32_t n_docs,
                              uint32_t* inv, uint32_t* status, uint32_t n_cu, hipStream_t stream);

// The entries, or the tombstones, of the replica written in place: off is read,
// never written.
struct InplaceCols {
    const uint32_t* off;  // NULL (tombstones): the replica keeps none
    uint32_t* cnt;
    uint64_t* keys;
    uint32_t* actors;
    uint64_t* counters;
};

struct InplaceArgs {
    RepSide sub;
    uint32_t n_docs, R;
    InplaceCols e, t;
    uint64_t* vv;
    uint32_t* doc_actor;    // NULL: not written
    const uint32_t* idx;    // [sub.n_docs]
    const uint32_t* n_idx;  // NULL: sub.n_docs
    const uint32_t* inv;    // [n_docs] the inverse map
    uint32_t* verdict;      // [sub.n_docs] kInpIgnored / kInpPlaced / kInpSpilled
    uint32_t* spill_j;
    uint32_t* spill_doc;
    uint32_t* n_spill;
};

// inv, verdict: n_docs and sub.n_docs workspace words; parts: one per 1,024 sub documents.
hipError_t launch_replica_inplace(const InplaceArgs& a, uint32_t* inv, uint32_t* parts, uint32_t* status,
                                  uint32_t n_cu, hipStream_t stream);

// Replica repack (crdt_replica_repack_async; replica_repack.hip): select's or
// scatter's arguments and the two headroom policies (NULL already replaced by
// the packed policy).
struct RepackArgs {
    ReplicaArgs s;
    crdt_headroom er, tr;
};

// launch_replica's workspace and conventions (replica.hip): a.s.inv != NULL is the
// scatter mapping, a.s.n_out == 0 writes offsets[0] = 0 alone.
hipError_t launch_replica_repack(const RepackArgs& a, uint32_t* inv, uint32_t* parts_e, uint32_t* parts_t,
                                 uint32_t* status, uint32_t n_cu, hipStream_t stream);

}  // namespace crdt
