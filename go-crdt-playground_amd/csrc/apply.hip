// Batched local operations on the device: the state producers of the merge
// path, applied to many documents at once.
//
//   CRDT_OP_ADD            (*AWSet).Add(k)          awset.go:89-94
//                          vv[actor]++; entries[k] = {actor, vv[actor]}
//   CRDT_OP_DEL            (*AWSet).Del(k)          awset.go:96-101
//                          delete(entries, k); the clock is not bumped
//   CRDT_OP_DELTA_DEL      (*AWSetDelta).Del(k...)  awset-delta_test.go:14-33:
//                          one call: vv[actor]++ once, dot2 = {actor, vv[actor]}
//   CRDT_OP_DELTA_DEL_KEY  a key of that call: if k is in entries,
//                          Deleted[k] = dot2 and the entry is removed
//
// The kernel body, with the per-key view it works from, is apply_wave.hpp; the
// logged call (apply_log.hip) runs the same body with its log switched on.
//
// What a caller can rely on (tests/test_gpu_apply_edges.py):
//   * offsets and counts (of out and of tomb_out) are written for every
//     document.  A document whose op list is refused (more than 256 ops, an
//     unknown kind, a DELTA_DEL_KEY outside a call or without a tomb_out, a
//     clock bump with actor >= R) has count 0 in both; its slots and its clock
//     are undefined; every other document of the batch is exact;
//   * a live count above the document's slots, state or tombstones, is clamped
//     to them and crdt_ctx_sync returns CRDT_E_CAPACITY, as in
//     crdt_awset_has_async;
//   * tomb_out == NULL: no tombstone is read or written, whatever `tombs`
//     holds; Deleted is left as the caller holds it.
// tomb_gc_kernel below has no status word: it takes counts[d] as given.
#include "apply_wave.hpp"

namespace crdt {

// Opt-in tombstone GC (crdt_tombstone_gc_async): one wavefront per doc keeps
// the tombstones the doc's stable clock has not covered, compacted in order
// with one ballot per 64 (gcDeleted, awset-delta_test.go:67-77, is empty in the
// reference; see include/crdtgpu.h for the rule).
__global__ __launch_bounds__(256) void tomb_gc_kernel(TombView tb, uint32_t n_docs, uint32_t R, const uint64_t* stable,
                                                      TombOut out) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t d = uniform(blockIdx.x * 4 + (threadIdx.x >> 6)); d < n_docs; d += gridDim.x * 4) {
        const uint32_t o = tb.offsets[d], n = live_count(tb.offsets, tb.counts, d);
        const uint64_t* vv = stable + (size_t)d * R;
        uint32_t kept = 0;
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t i = base + lane;
            const bool v = i < n;
            uint64_t k = 0, c = 0;
            uint32_t a = 0;
            if (v) {
                k = tb.keys[o + i];
                a = tb.actors[o + i];
                c = tb.counters[o + i];
            }
            const bool covered = v && a < R && vv[a] >= c;  // HasDot, crdt-misc.go:28-34
            const bool keep = v && !covered;
            const uint64_t m = ballot(keep);
            if (keep) {
                const uint32_t pos = kept + below(m);
                out.keys[o + pos] = k;
                out.actors[o + pos] = a;
                out.counters[o + pos] = c;
            }
            kept += popc(m);
        }
        if (lane == 0) {
            out.counts[d] = kept;
            out.offsets[d] = o;
            if (d == n_docs - 1) out.offsets[n_docs] = tb.offsets[n_docs];
        }
    }
}

hipError_t launch_tomb_gc(const TombView& tb, uint32_t n_docs, uint32_t R, const uint64_t* stable, const TombOut& out,
                          uint32_t n_cu, hipStream_t stream) {
    if (n_docs == 0) return hipSuccess;
    const uint32_t grid = min((n_docs + 3) / 4, n_cu * 16u);
    hipLaunchKernelGGL(tomb_gc_kernel, dim3(grid), dim3(256), 0, stream, tb, n_docs, R, stable, out);
    return hipGetLastError();
}

hipError_t launch_apply(const BatchView& st, const TombView& tb, const ApplyOps& ops, const OutView& out,
                        const TombOut& tout, bool has_tout, const Work& wk, uint32_t n_cu, hipStream_t stream) {
    if (st.n_docs == 0) return hipSuccess;
    const uint32_t need = (st.n_docs + kApplyWaves - 1) / kApplyWaves;
    const uint32_t grid = min(need, n_cu * 16u);
    hipLaunchKernelGGL((apply_kernel<kApplyWaves, false>), dim3(grid), dim3(kApplyWaves * 64), 0, stream, st, tb, ops,
                       out, tout, (uint32_t)has_tout, wk, ApplyLogArgs<false>{});
    return hipGetLastError();
}

}  // namespace crdt
