// The decision log of a merge (join_log.hip, delta_pair_log.hip, fold_log.hip): what
// the logged kernels share beyond the merge itself.  The per-direction summary sums
// (LogSums: added up per wave or workgroup, flushed with integer atomics into
// kLogParts spread rows of the context's partials buffer, reduced by
// join_log_summary_kernel), the flag byte of a document, and the window walk's
// logging sink (LogSink; merge_block.hpp, merge_walk) with its sibling for the
// comparison of two states (DiffSink, diff_walk).  The zero and summary
// kernels live in join_log.hip and are launched through the two functions
// declared at the end.
#pragma once

#include "crdt_device.hpp"
#include "merge_block.hpp"

namespace crdt {

constexpr uint32_t kLogParts = 1024;  // rows of summary partial sums per direction
constexpr uint32_t kLogPartRow = 8;   // words per row (5 used)

// crdt_diff_out.summary of one direction, summed over the documents a wave or a
// workgroup has merged.
struct LogSums {
    uint32_t v[5];
};

__device__ __forceinline__ void sums_add(LogSums& s, uint32_t n_rem, uint32_t n_ups, uint32_t n_upd, uint32_t flags) {
    s.v[0] += n_rem;
    s.v[1] += n_ups;
    s.v[2] += n_upd;
    s.v[3] += (flags & 7u) ? 1u : 0u;
    s.v[4] += flags ? 1u : 0u;
}

// One thread adds the sums to row `row` of direction `dir` (integer adds: the
// total does not depend on their order).
__device__ __forceinline__ void sums_flush(uint32_t* parts, uint32_t dir, uint32_t row, const LogSums& s) {
    uint32_t* p = parts + ((size_t)dir * kLogParts + row % kLogParts) * kLogPartRow;
#pragma unroll
    for (int i = 0; i < 5; ++i)
        if (s.v[i]) atomicAdd(p + i, s.v[i]);
}

__device__ __forceinline__ uint32_t log_flags(uint32_t n_rem, uint32_t n_ups, uint32_t n_upd, bool clock) {
    return (n_rem ? CRDT_DIFF_REMOVED : 0u) | (n_ups > n_upd ? CRDT_DIFF_ADDED : 0u) | (n_upd ? CRDT_DIFF_UPDATED : 0u) |
           (clock ? CRDT_DIFF_CLOCK : 0u);
}

// The logging sink of the window walk (merge_block.hpp, merge_walk): the
// survivors as KeepSink places them, and beside them the removed and the upserted
// records, each list contiguous in key order: three running offsets from three
// block scans per window.
struct LogSink {
    static constexpr bool kLog = true;
    EntriesOut out, rem, ups;
    uint8_t* ups_kind;                // NULL: none
    uint32_t o, o_rem, o_ups;         // written so far: survivors (<= n_d + n_s), removed (<= n_d), upserted (<= n_s)
    uint32_t my_upd;                  // UPDATED records this thread has written

    template <int NT, int IPT>
    __device__ __forceinline__ void place(const uint8_t (&cls)[IPT], const uint64_t (&ok)[IPT],
                                          const uint32_t (&oa)[IPT], const uint64_t (&oc)[IPT], uint32_t* wave_tot) {
        uint32_t cnt = 0, cnt_rem = 0, cnt_ups = 0;
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
            cnt += (cls[q] & kPosKeep) ? 1u : 0u;
            cnt_rem += (cls[q] & kPosRem) ? 1u : 0u;
            cnt_ups += (cls[q] & (kPosAdd | kPosUpd)) ? 1u : 0u;
            my_upd += (cls[q] & kPosUpd) ? 1u : 0u;
        }
        uint32_t total, total_rem, total_ups;
        uint32_t pos = o + block_exclusive_scan<NT>(cnt, wave_tot, &total);
        uint32_t pos_rem = o_rem + block_exclusive_scan<NT>(cnt_rem, wave_tot, &total_rem);
        uint32_t pos_ups = o_ups + block_exclusive_scan<NT>(cnt_ups, wave_tot, &total_ups);
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
            if (cls[q] & kPosKeep) put_entry(out, pos++, ok[q], oa[q], oc[q]);
            if (cls[q] & kPosRem) put_entry(rem, pos_rem++, ok[q], oa[q], oc[q]);
            if (cls[q] & (kPosAdd | kPosUpd)) {
                put_entry(ups, pos_ups, ok[q], oa[q], oc[q]);
                if (ups_kind) ups_kind[pos_ups] = (uint8_t)((cls[q] & kPosUpd) ? CRDT_DIFF_UPDATED : CRDT_DIFF_ADDED);
                ++pos_ups;
            }
        }
        o += total;
        o_rem += total_rem;
        o_ups += total_ups;
    }
};

// LogSink's sibling for a walk that compares two states (the logged fold's block
// path, fold_log.hip): the state after is in place already, so only the two lists
// are written, with two running offsets.
struct DiffSink {
    static constexpr bool kLog = true;
    EntriesOut rem, ups;
    uint8_t* ups_kind;      // NULL: none
    uint32_t o_rem, o_ups;  // written so far: removed (<= the entries before), upserted (<= the entries after)
    uint32_t my_upd;        // UPDATED records this thread has written

    template <int NT, int IPT>
    __device__ __forceinline__ void place(const uint8_t (&cls)[IPT], const uint64_t (&ok)[IPT],
                                          const uint32_t (&oa)[IPT], const uint64_t (&oc)[IPT], uint32_t* wave_tot) {
        uint32_t cnt_rem = 0, cnt_ups = 0;
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
            cnt_rem += (cls[q] & kPosRem) ? 1u : 0u;
            cnt_ups += (cls[q] & (kPosAdd | kPosUpd)) ? 1u : 0u;
            my_upd += (cls[q] & kPosUpd) ? 1u : 0u;
        }
        uint32_t total_rem, total_ups;
        uint32_t pos_rem = o_rem + block_exclusive_scan<NT>(cnt_rem, wave_tot, &total_rem);
        uint32_t pos_ups = o_ups + block_exclusive_scan<NT>(cnt_ups, wave_tot, &total_ups);
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
            if (cls[q] & kPosRem) put_entry(rem, pos_rem++, ok[q], oa[q], oc[q]);
            if (cls[q] & (kPosAdd | kPosUpd)) {
                put_entry(ups, pos_ups, ok[q], oa[q], oc[q]);
                if (ups_kind) ups_kind[pos_ups] = (uint8_t)((cls[q] & kPosUpd) ? CRDT_DIFF_UPDATED : CRDT_DIFF_ADDED);
                ++pos_ups;
            }
        }
        o_rem += total_rem;
        o_ups += total_ups;
    }
};

// The window walk as a comparison (merge_block.hpp, merge_walk<.., DIFF>): the
// entries of `before` whose key `after` lacks are handed to the sink as removed
// with their own dot, the entries of `after` whose key `before` lacks as added
// and those it holds under another dot as updated, each with after's dot.
template <int NT, int IPT, class Sink>
__device__ __forceinline__ void diff_walk(const Entries& before, const Entries& after, MergeSmem<NT, IPT>& sm,
                                          Sink& sink) {
    uint32_t unused = 0;
    merge_walk<NT, IPT, Sink, true>(before, after, Entries{nullptr, nullptr, nullptr, 0u}, true, 0u, sm, sink, unused);
}

// Bytes of the partials buffer both directions' rows take.
size_t join_log_parts_bytes();

// join_log.hip's two small kernels.  Zero: n words of p and of q (either may be
// NULL), a kernel rather than hipMemsetAsync so that a captured call is a graph of
// kernel nodes only.  Summary: s_ab (and s_ba when dirs == 2) = the column sums of
// that direction's partial rows; a NULL summary is skipped.
hipError_t launch_log_zero(uint32_t* p, uint32_t* q, uint32_t n, hipStream_t stream);
hipError_t launch_log_summary(const uint32_t* parts, uint32_t* s_ab, uint32_t* s_ba, uint32_t dirs, hipStream_t stream);

}  // namespace crdt
