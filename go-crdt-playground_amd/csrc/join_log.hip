// Logged join and exchange: out[d] = dst[d] <- src[d] as join.hip writes it
// (awset.go:103-161), and beside it the merge's decision log (awset.go:109-158)
// in structured form: the dst entries the merge removed and the src entries it
// added or moved a common key to.  The kernels that write the merged state have
// made each of those decisions already, so the log costs no second read of the
// batches and no search: it is crdt_awset_diff_async(dst, out)'s answer, laid
// out by the inputs' own slot bounds (a removed entry was a dst entry, so
// document d's removed list starts at dst.offsets[d]; an upserted entry was a
// src entry, so its list starts at src.offsets[d]) and therefore written with
// no scan over documents.
//
// The per-key rule is decide() of merge_block.hpp with full = true.  From its
// answer for one union key (dst dot d, src dot s):
//   dst-only and dropped        removed, with d        (the log's `remove`)
//   src-only and kept           upserted ADDED, with s (`add`)
//   common and the dot changes  upserted UPDATED, with s (`update`)
//
// Two paths, one launch each, dispatched as delta_pair.hip does:
//  * join_log_wave_kernel: one wavefront per document when both sides hold
//    <= 64 live entries, kLogDocs documents in turn per wave.  Both entry lists
//    and both clocks are staged in LDS once; lane i owns entry i of each side
//    and finds its key on the other side by LDS binary search.  Every position
//    is a ballot and a popcount: the survivor's slot as in join_wave_kernel,
//    the removed rank over the dst lanes, the upsert rank over the src lanes.
//    The exchange decides both directions from the one staging.
//    Staging, lookup, survivor placement, clock and slot bounds are the pair
//    merges' shared wave pieces (merge_wave.hpp); the ranks and sums are here.
//  * join_log_block_kernel: workgroups pop the worklist (for_each_work); per
//    direction the one merge-path window walk (merge_walk, merge_block.hpp)
//    with LogSink as its sink: three running offsets (survivors, removed,
//    upserted) from three block scans per window.  merge_walk's comment says
//    why a common key that straddles a window boundary is classified once.
//
// No atomic decides a position.  The summary is summed with integer atomics
// over kLogParts spread rows of partial sums (the context's partials buffer,
// zeroed by a kernel first) and reduced by join_log_summary_kernel.
//
// The sums, the flag byte and the walk's sink (LogSink) are shared with the
// logged delta merge (merge_log.hpp; delta_pair_log.hip), which also launches
// the zero and summary kernels below.
#include "crdt_device.hpp"
#include "merge_block.hpp"
#include "merge_log.hpp"
#include "merge_wave.hpp"

namespace crdt {

constexpr int kLogWaves = 4;       // wavefronts per workgroup of the wave path
constexpr int kLogDocs = 8;        // documents one wavefront takes in turn
constexpr int kLogWaveMax = 64;    // live entries per side the wave path takes
constexpr int kLogBlockNT = 256;   // block path: threads per workgroup
constexpr int kLogBlockIPT = 4;    // block path: merged positions per thread and window

size_t join_log_parts_bytes() { return (size_t)2 * kLogParts * kLogPartRow * sizeof(uint32_t); }

// One direction of a wave-path document: dst = side x of sm (nd entries, its
// slots at doff), src = side 1 - x (ns entries, slots at soff).
__device__ __forceinline__ void log_wave_dir(const WaveSmem& sm, uint32_t x, uint32_t nd, uint32_t ns, uint32_t R,
                                             uint32_t d, uint32_t doff, uint32_t soff, const OutView& out,
                                             const MergeLogView& lg, uint32_t lane, LogSums& sums, uint32_t& err) {
    const WaveDir p = wave_lookup(sm, x, nd, ns, lane);
    const Entries none{nullptr, nullptr, nullptr, 0};
    bool dkeep = false, skeep = false, supd = false;
    uint32_t oda = p.Da, osa = p.Sa;
    uint64_t odc = p.Dc, osc = p.Sc;
    if (p.dv) dkeep = decide(true, p.Da, p.Dc, p.dmatch, p.ja, p.jc, true, p.dvv, p.svv, R, none, p.Dk, oda, odc, err);
    if (p.sv) {
        if (p.smatch) {  // the common key as its src lane sees it: the dot the merge gives it against dst's
            decide(true, p.ia, p.ic, true, p.Sa, p.Sc, true, p.dvv, p.svv, R, none, p.Sk, osa, osc, err);
            supd = osa != p.ia || osc != p.ic;
        } else {
            skeep = decide(false, 0u, 0ull, true, p.Sa, p.Sc, true, p.dvv, p.svv, R, none, p.Sk, osa, osc, err);
        }
    }
    const bool removed = p.dv && !dkeep;
    const bool ups = skeep || supd;
    const uint32_t n_out = wave_place(p, dkeep, oda, odc, skeep, osa, osc, out, doff + soff);

    // a log record's slot: its kind's lanes below it
    const uint64_t rm = ballot(removed), um = ballot(ups), updm = ballot(supd);
    const uint32_t n_rem = popc(rm), n_ups = popc(um), n_upd = popc(updm);  // <= nd, <= ns: within the lists' slots
    if (removed) {
        const uint32_t q = doff + below(rm);
        lg.rem_keys[q] = p.Dk;
        lg.rem_actors[q] = p.Da;
        lg.rem_counters[q] = p.Dc;
    }
    if (ups) {
        const uint32_t q = soff + below(um);
        lg.ups_keys[q] = p.Sk;
        lg.ups_actors[q] = osa;
        lg.ups_counters[q] = osc;
        if (lg.ups_kind) lg.ups_kind[q] = (uint8_t)(supd ? CRDT_DIFF_UPDATED : CRDT_DIFF_ADDED);
    }
    const bool ahead = lane < R && p.svv[lane] > p.dvv[lane];  // the merged clock is max(D, S): it differs from D
    const uint32_t flags = log_flags(n_rem, n_ups, n_upd, ballot(ahead) != 0ull);
    if (lane == 0) {
        out.counts[d] = n_out;
        lg.flags[d] = (uint8_t)flags;
        lg.rem_counts[d] = n_rem;
        lg.ups_counts[d] = n_ups;
    }
    wave_clock(p, false, out, d, R, lane);
    sums_add(sums, n_rem, n_ups, n_upd, flags);
}

// EXCH: also o_ba = b <- a and its log.  parts == nullptr: no summary asked for.
template <int WAVES, int K, bool EXCH>
__global__ __launch_bounds__(WAVES * 64) void join_log_wave_kernel(BatchView A, BatchView B, OutView o_ab, OutView o_ba,
                                                                   MergeLogView l_ab, MergeLogView l_ba, Work wk,
                                                                   uint32_t* parts) {
    __shared__ WaveSmem smem[WAVES];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t R = A.R, n_docs = A.n_docs;
    WaveSmem& sm = smem[w];
    uint32_t err = 0;
    LogSums s_ab{}, s_ba{};

    // (whole waves leave or stay: the kernel has no workgroup barrier)
#pragma unroll 1
    for (uint32_t k = 0; k < (uint32_t)K; ++k) {
        const uint32_t d = uniform(blockIdx.x * (WAVES * K) + k * WAVES + w);
        if (d >= n_docs) break;
        uint32_t ao, bo;
        const uint32_t na = live_span(A.offsets, A.counts, d, ao, err);
        const uint32_t nb = live_span(B.offsets, B.counts, d, bo, err);
        if (lane == 0) {
            pair_bounds(o_ab.offsets, l_ab.rem_offsets, l_ab.ups_offsets, A.offsets, B.offsets, d, n_docs, ao, bo);
            if (EXCH)
                pair_bounds(o_ba.offsets, l_ba.rem_offsets, l_ba.ups_offsets, B.offsets, A.offsets, d, n_docs, bo, ao);
        }
        if (na > kLogWaveMax || nb > kLogWaveMax) {
            if (lane == 0) push_work(wk, d, n_docs);
            continue;
        }
        wave_sync();  // every lane's probes of the previous document are done
        wave_stage_pair(sm, A, B, d, ao, na, bo, nb, lane);
        wave_sync();
        log_wave_dir(sm, 0u, na, nb, R, d, ao, bo, o_ab, l_ab, lane, s_ab, err);
        if (EXCH) log_wave_dir(sm, 1u, nb, na, R, d, bo, ao, o_ba, l_ba, lane, s_ba, err);
    }
    if (parts && lane == 0) {
        const uint32_t row = blockIdx.x * WAVES + w;
        sums_flush(parts, 0u, row, s_ab);
        if (EXCH) sums_flush(parts, 1u, row, s_ba);
    }
    flag_error(wk.status, err);
}

// One direction of a block-path document, by the whole workgroup: the window
// walk with the log written beside the survivors.
template <int NT, int IPT>
__device__ __forceinline__ void log_block_dir(const BatchView& Dd, const BatchView& Sd, uint32_t d, uint32_t R, MergeSmem<NT, IPT>& sm,
                              const OutView& out, const MergeLogView& lg, uint32_t* parts, uint32_t dir,
                              uint32_t& err) {
    const uint32_t tid = threadIdx.x;
    uint32_t doff, soff;
    const uint32_t n_d = live_span(Dd.offsets, Dd.counts, d, doff, err);
    const uint32_t n_s = live_span(Sd.offsets, Sd.counts, d, soff, err);
    const Entries D{Dd.keys + doff, Dd.actors + doff, Dd.counters + doff, n_d};
    const Entries S{Sd.keys + soff, Sd.actors + soff, Sd.counters + soff, n_s};
    const Entries none{nullptr, nullptr, nullptr, 0};
    if (tid < R) {
        sm.dvv[tid] = Dd.vv[(size_t)d * R + tid];
        sm.svv[tid] = Sd.vv[(size_t)d * R + tid];
    }
    __syncthreads();
    const uint32_t obase = doff + soff;
    LogSink sink{{out.keys + obase, out.actors + obase, out.counters + obase},
                 {lg.rem_keys + doff, lg.rem_actors + doff, lg.rem_counters + doff},
                 {lg.ups_keys + soff, lg.ups_actors + soff, lg.ups_counters + soff},
                 lg.ups_kind ? lg.ups_kind + soff : nullptr, 0u, 0u, 0u, 0u};
    merge_walk<NT, IPT>(D, S, none, true, R, sm, sink, err);
    const uint32_t o = sink.o, o_rem = sink.o_rem, o_ups = sink.o_ups;
    uint32_t n_upd;
    block_exclusive_scan<NT>(sink.my_upd, sm.wave_tot, &n_upd);
    const bool clock = __syncthreads_or(tid < R && sm.svv[tid] > sm.dvv[tid]) != 0;
    const uint32_t flags = log_flags(o_rem, o_ups, n_upd, clock);
    if (tid == 0) {
        out.counts[d] = o;
        lg.flags[d] = (uint8_t)flags;
        lg.rem_counts[d] = o_rem;
        lg.ups_counts[d] = o_ups;
        if (parts) {
            LogSums s{};
            sums_add(s, o_rem, o_ups, n_upd, flags);
            sums_flush(parts, dir, blockIdx.x, s);
        }
    }
    if (tid < R) {
        const uint64_t x = sm.dvv[tid], y = sm.svv[tid];
        out.vv[(size_t)d * R + tid] = x > y ? x : y;
    }
    __syncthreads();  // sm.dvv / sm.svv are the next direction's
}

template <int NT, int IPT, bool EXCH>
__global__ __launch_bounds__(NT) void join_log_block_kernel(BatchView A, BatchView B, OutView o_ab, OutView o_ba,
                                                            MergeLogView l_ab, MergeLogView l_ba, Work wk,
                                                            uint32_t* parts) {
    __shared__ MergeSmem<NT, IPT> sm;
    const uint32_t R = A.R, n_docs = A.n_docs;
    uint32_t err = 0;
    for_each_work(wk, 0u, n_docs, &sm.word[0], [&](uint32_t d) {
        log_block_dir<NT, IPT>(A, B, d, R, sm, o_ab, l_ab, parts, 0u, err);
        if (EXCH) log_block_dir<NT, IPT>(B, A, d, R, sm, o_ba, l_ba, parts, 1u, err);
    });
    flag_error(wk.status, err);
}

// Zeroes n words (the partial rows, or a summary of a call without documents): a
// kernel rather than hipMemsetAsync, so a captured call is a graph of kernel nodes only.
__global__ __launch_bounds__(256) void join_log_zero_kernel(uint32_t* p, uint32_t* q, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        if (p) p[i] = 0u;
        if (q) q[i] = 0u;
    }
}

// summary of direction blockIdx.x = the column sums of its partial rows.
__global__ __launch_bounds__(256) void join_log_summary_kernel(const uint32_t* parts, uint32_t* s_ab, uint32_t* s_ba) {
    __shared__ uint32_t acc[4][kLogPartRow];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t* const out = blockIdx.x ? s_ba : s_ab;
    if (!out) return;  // (the whole workgroup)
    const uint32_t* const p = parts + (size_t)blockIdx.x * kLogParts * kLogPartRow;
    uint32_t v[5] = {0u, 0u, 0u, 0u, 0u};
    for (uint32_t row = tid; row < kLogParts; row += 256)
#pragma unroll
        for (int i = 0; i < 5; ++i) v[i] += p[row * kLogPartRow + i];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[i] += (uint32_t)__shfl_xor((int)v[i], o);
        if (lane == 0) acc[w][i] = v[i];
    }
    __syncthreads();
    if (tid < 5) out[tid] = acc[0][tid] + acc[1][tid] + acc[2][tid] + acc[3][tid];
}

hipError_t launch_log_zero(uint32_t* p, uint32_t* q, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(join_log_zero_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, q, n);
    return hipGetLastError();
}

hipError_t launch_log_summary(const uint32_t* parts, uint32_t* s_ab, uint32_t* s_ba, uint32_t dirs, hipStream_t stream) {
    hipLaunchKernelGGL(join_log_summary_kernel, dim3(dirs), dim3(256), 0, stream, parts, s_ab, s_ba);
    return hipGetLastError();
}

// log_ba == nullptr: the join (one direction).  parts: join_log_parts_bytes() of
// workspace, used when either log has a summary.
hipError_t launch_join_log(const BatchView& A, const BatchView& B, const OutView& out_ab, const OutView* out_ba,
                           const MergeLogView& log_ab, const MergeLogView* log_ba, const Work& wk, uint32_t* parts,
                           uint32_t block_grid, hipStream_t stream) {
    const uint32_t n = A.n_docs;
    const bool exch = out_ba != nullptr && log_ba != nullptr;
    uint32_t* const s_ab = log_ab.summary;
    uint32_t* const s_ba = exch ? log_ba->summary : nullptr;
    if (n == 0) {  // nothing that reads documents
        if (!s_ab && !s_ba) return hipSuccess;
        hipLaunchKernelGGL(join_log_zero_kernel, dim3(1), dim3(256), 0, stream, s_ab, s_ba, 5u);
        return hipGetLastError();
    }
    uint32_t* const pp = (s_ab || s_ba) ? parts : nullptr;
    if (pp) {
        const uint32_t words = (uint32_t)(join_log_parts_bytes() / sizeof(uint32_t));
        hipLaunchKernelGGL(join_log_zero_kernel, dim3((words + 255) / 256), dim3(256), 0, stream, pp,
                           (uint32_t*)nullptr, words);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const OutView& o2 = exch ? *out_ba : out_ab;
    const MergeLogView& l2 = exch ? *log_ba : log_ab;
    const uint32_t per_block = kLogWaves * kLogDocs;
    const dim3 grid((n + per_block - 1) / per_block), block(kLogWaves * 64);
    if (exch)
        hipLaunchKernelGGL((join_log_wave_kernel<kLogWaves, kLogDocs, true>), grid, block, 0, stream, A, B, out_ab, o2,
                           log_ab, l2, wk, pp);
    else
        hipLaunchKernelGGL((join_log_wave_kernel<kLogWaves, kLogDocs, false>), grid, block, 0, stream, A, B, out_ab, o2,
                           log_ab, l2, wk, pp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (exch)
        hipLaunchKernelGGL((join_log_block_kernel<kLogBlockNT, kLogBlockIPT, true>), dim3(block_grid), dim3(kLogBlockNT),
                           0, stream, A, B, out_ab, o2, log_ab, l2, wk, pp);
    else
        hipLaunchKernelGGL((join_log_block_kernel<kLogBlockNT, kLogBlockIPT, false>), dim3(block_grid),
                           dim3(kLogBlockNT), 0, stream, A, B, out_ab, o2, log_ab, l2, wk, pp);
    e = hipGetLastError();
    if (e != hipSuccess || !pp) return e;
    hipLaunchKernelGGL(join_log_summary_kernel, dim3(exch ? 2 : 1), dim3(256), 0, stream, pp, s_ab, s_ba);
    return hipGetLastError();
}

}  // namespace crdt
