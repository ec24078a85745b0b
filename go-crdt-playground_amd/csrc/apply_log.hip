// Logged local ops (crdt_awset_apply_log_async): apply_kernel (apply_wave.hpp)
// with its log switched on.  Beside the state crdt_awset_apply_async writes, every
// document gets the diff of its entries: the state entries an op removed, at
// state.offsets[d] with the dot they had, and the entries an ADD left new or under
// another dot, at op_off[d] in key order; counts, offsets and flags for every
// document, a refused one's empty.  No position depends on another document, so
// the call is this one kernel between the summary's zero and reduce kernels
// (join_log.hip), which it skips when no summary is asked for.
//
// The logged form's shared struct is the plain one's plus one prefix table:
// 23,080 bytes per wavefront, 46,160 per workgroup of two, so three workgroups
// (six wavefronts) share a CU's 160 KB of LDS, as with the plain kernel's 44,096.
#include "apply_wave.hpp"

namespace crdt {

// parts: join_log_parts_bytes() of workspace, used when the log has a summary.
hipError_t launch_apply_log(const BatchView& st, const TombView& tb, const ApplyOps& ops, const OutView& out,
                            const TombOut& tout, bool has_tout, const MergeLogView& lg, const Work& wk,
                            uint32_t* parts, uint32_t n_cu, hipStream_t stream) {
    if (st.n_docs == 0)  // nothing that reads documents
        return lg.summary ? launch_log_zero(lg.summary, nullptr, 5u, stream) : hipSuccess;
    uint32_t* const pp = lg.summary ? parts : nullptr;
    if (pp) {
        const hipError_t e =
            launch_log_zero(pp, nullptr, (uint32_t)(join_log_parts_bytes() / sizeof(uint32_t)), stream);
        if (e != hipSuccess) return e;
    }
    const uint32_t need = (st.n_docs + kApplyWaves - 1) / kApplyWaves;
    const uint32_t grid = min(need, n_cu * 16u);
    hipLaunchKernelGGL((apply_kernel<kApplyWaves, true>), dim3(grid), dim3(kApplyWaves * 64), 0, stream, st, tb, ops,
                       out, tout, (uint32_t)has_tout, wk, ApplyLogArgs<true>{lg, pp});
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !pp) return e;
    return launch_log_summary(pp, lg.summary, nullptr, 1u, stream);
}

}  // namespace crdt
