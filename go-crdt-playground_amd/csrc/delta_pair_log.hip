// Logged delta merge of a resident replica pair: out_ab[d] = a[d] <- b[d] and
// (exchange) out_ba[d] = b[d] <- a[d] as delta_pair.hip writes them, each one
// (*AWSetDelta).Merge (awset-delta_test.go:51-166), and beside each the merge's
// decision log in the logged join's layout (join_log.hip): the dst entries the
// merge removed at dst.offsets[d], the src entries it added or moved a common key
// to at src.offsets[d].  It is crdt_awset_diff_async(dst, out)'s answer, taken
// from the decisions the merge makes anyway: no second read, no search.
//
// The kind of a direction comes first, as in delta_pair.hip; the per-key rule is
// decide() of merge_block.hpp with the real `full` and src's tombstones.  From
// its answer for one union key (dst dot d, src dot s):
//   FULL   the logged join's log
//   NONE   nothing: empty lists, flags 0, the clock untouched (:60)
//   DELTA  dst-only and dropped         removed, with d  (only a tombstone drops it)
//          src-only and kept            upserted ADDED, with s
//          common, kept, dot changes    upserted UPDATED, with s
//          common and dropped           removed, with d: phase 1 may have moved the
//                                       key to s before a tombstone of phase 2
//                                       dropped it (:149-164); the log says what
//                                       left dst, so it carries d and no upsert
//          src-only, added then dropped no record at all
//
// Two paths, one launch each, dispatched as delta_pair.hip does:
//  * delta_pair_log_wave_kernel: one wavefront per document when both sides hold
//    <= 64 live entries and <= 64 live tombstones (PairWaveSmem staging, the kind
//    by pair_wave_kind, survivors by wave_place: merge_wave.hpp).  The removed
//    rank is a ballot over the dst lanes, the upsert rank one over the src lanes,
//    as in join_log_wave_kernel.
//  * delta_pair_log_block_kernel: workgroups pop the worklist (for_each_work);
//    per direction delta_changes takes the kind, then the window walk
//    (merge_walk) runs with LogSink in full or delta mode, or dst is copied and
//    the lists stay empty for NONE.
//
// The summary is summed as the logged join's (merge_log.hpp).
#include "crdt_device.hpp"
#include "merge_block.hpp"
#include "merge_log.hpp"
#include "merge_wave.hpp"

namespace crdt {

constexpr int kPairLogWaves = 4;      // wavefronts (= documents) per workgroup of the wave path
constexpr int kPairLogWaveMax = 64;   // live entries, and live tombstones, per side the wave path takes
constexpr int kPairLogBlockNT = 256;  // block path: threads per workgroup
constexpr int kPairLogBlockIPT = 4;   // block path: merged positions per thread and window

// One direction of a wave-path document: dst = side x of sm (nd entries, its
// slots at doff), src = side 1 - x (ns entries, nts tombstones, slots at soff).
__device__ __forceinline__ void pair_log_wave_dir(const PairWaveSmem& sm, uint32_t x, uint32_t nd, uint32_t ns,
                                                  uint32_t nts, uint32_t s_actor, uint32_t R, uint32_t d,
                                                  uint32_t doff, uint32_t soff, const OutView& out, uint8_t* kind_out,
                                                  const MergeLogView& lg, uint32_t lane, LogSums& sums,
                                                  uint32_t& err) {
    const uint32_t y = 1u - x;
    const WaveDir p = wave_lookup(sm, x, nd, ns, lane);
    const Entries tomb{sm.tk[y], sm.ta[y], sm.tc[y], nts};

    bool full;
    const uint32_t kind = pair_wave_kind(sm, p, y, ns, nts, s_actor, R, lane, full, err);
    const bool none = kind == CRDT_DELTA_NONE;

    bool dkeep = false, skeep = false, supd = false;
    uint32_t oda = p.Da, osa = p.Sa;
    uint64_t odc = p.Dc, osc = p.Sc;
    if (none) {
        dkeep = p.dv;
    } else {
        if (p.dv)
            dkeep = decide(true, p.Da, p.Dc, p.dmatch, p.ja, p.jc, full, p.dvv, p.svv, R, tomb, p.Dk, oda, odc, err);
        if (p.sv) {
            if (p.smatch) {  // the common key as its src lane sees it: UPDATED only when the key is kept
                const bool kept =
                    decide(true, p.ia, p.ic, true, p.Sa, p.Sc, full, p.dvv, p.svv, R, tomb, p.Sk, osa, osc, err);
                supd = kept && (osa != p.ia || osc != p.ic);
            } else {
                skeep = decide(false, 0u, 0ull, true, p.Sa, p.Sc, full, p.dvv, p.svv, R, tomb, p.Sk, osa, osc, err);
            }
        }
    }
    const bool removed = p.dv && !dkeep;
    const bool ups = skeep || supd;
    const uint32_t n_out = wave_place(p, dkeep, oda, odc, skeep, osa, osc, out, doff + soff);

    // a log record's slot: its kind's lanes below it
    const uint64_t rm = ballot(removed), um = ballot(ups), updm = ballot(supd);
    const uint32_t n_rem = popc(rm), n_ups = popc(um), n_upd = popc(updm);  // <= nd, <= ns: within the lists' slots
    if (removed) {  // with the dot it had in dst, whatever phase 1 made of a common key
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
    // the merged clock is max(D, S) unless the kind is NONE, which leaves D (:60)
    const bool ahead = !none && lane < R && p.svv[lane] > p.dvv[lane];
    const uint32_t flags = log_flags(n_rem, n_ups, n_upd, ballot(ahead) != 0ull);
    if (lane == 0) {
        out.counts[d] = n_out;
        if (kind_out) kind_out[d] = (uint8_t)kind;
        lg.flags[d] = (uint8_t)flags;
        lg.rem_counts[d] = n_rem;
        lg.ups_counts[d] = n_ups;
    }
    wave_clock(p, none, out, d, R, lane);
    sums_add(sums, n_rem, n_ups, n_upd, flags);
}

// EXCH: also out_ba = b <- a and its log.  Without it a's tombstones are never
// read (A.tb is empty).  parts == nullptr: no summary asked for.
template <int WAVES, bool EXCH>
__global__ __launch_bounds__(WAVES * 64) void delta_pair_log_wave_kernel(PairSide A, PairSide B, OutView o_ab,
                                                                         OutView o_ba, uint8_t* kind_ab,
                                                                         uint8_t* kind_ba, MergeLogView l_ab,
                                                                         MergeLogView l_ba, Work wk, uint32_t* parts) {
    __shared__ PairWaveSmem smem[WAVES];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t R = A.st.R, n_docs = A.st.n_docs;
    const uint32_t d = uniform(blockIdx.x * WAVES + w);
    if (d >= n_docs) return;  // (a whole wave; the kernel has no workgroup barrier)
    PairWaveSmem& sm = smem[w];
    uint32_t err = 0;

    uint32_t ao, bo, ato = 0, bto = 0;
    const uint32_t na = live_span(A.st.offsets, A.st.counts, d, ao, err);
    const uint32_t nb = live_span(B.st.offsets, B.st.counts, d, bo, err);
    const uint32_t nta = (EXCH && A.tb.offsets) ? live_span(A.tb.offsets, A.tb.counts, d, ato, err) : 0u;
    const uint32_t ntb = B.tb.offsets ? live_span(B.tb.offsets, B.tb.counts, d, bto, err) : 0u;

    if (lane == 0) {
        pair_bounds(o_ab.offsets, l_ab.rem_offsets, l_ab.ups_offsets, A.st.offsets, B.st.offsets, d, n_docs, ao, bo);
        if (EXCH)
            pair_bounds(o_ba.offsets, l_ba.rem_offsets, l_ba.ups_offsets, B.st.offsets, A.st.offsets, d, n_docs, bo, ao);
    }
    if (na > kPairLogWaveMax || nb > kPairLogWaveMax || nta > kPairLogWaveMax || ntb > kPairLogWaveMax) {
        if (lane == 0) push_work(wk, d, n_docs);
        flag_error(wk.status, err);
        return;
    }

    wave_stage_pair(sm, A.st, B.st, d, ao, na, bo, nb, lane);
    wave_stage(sm.tk[0], sm.ta[0], sm.tc[0], A.tb.keys, A.tb.actors, A.tb.counters, ato, nta, lane);
    wave_stage(sm.tk[1], sm.ta[1], sm.tc[1], B.tb.keys, B.tb.actors, B.tb.counters, bto, ntb, lane);
    wave_sync();

    LogSums s_ab{}, s_ba{};
    const uint32_t b_actor = B.doc_actor ? B.doc_actor[d] : B.actor;
    pair_log_wave_dir(sm, 0u, na, nb, ntb, b_actor, R, d, ao, bo, o_ab, kind_ab, l_ab, lane, s_ab, err);
    if (EXCH) {
        const uint32_t a_actor = A.doc_actor ? A.doc_actor[d] : A.actor;
        pair_log_wave_dir(sm, 1u, nb, na, nta, a_actor, R, d, bo, ao, o_ba, kind_ba, l_ba, lane, s_ba, err);
    }
    if (parts && lane == 0) {
        sums_flush(parts, 0u, d, s_ab);
        if (EXCH) sums_flush(parts, 1u, d, s_ba);
    }
    flag_error(wk.status, err);
}

// One direction of a block-path document, by the whole workgroup: the kind, then
// the window walk with the log written beside the survivors.
template <int NT, int IPT>
__device__ __forceinline__ void pair_log_block_dir(const PairSide& Dd, const PairSide& Sd, uint32_t d, uint32_t R,
                                                   MergeSmem<NT, IPT>& sm, const OutView& out, uint8_t* kind_out,
                                                   const MergeLogView& lg, uint32_t* parts, uint32_t dir,
                                                   uint32_t& err) {
    const uint32_t tid = threadIdx.x;
    uint32_t doff, soff, toff = 0;
    const uint32_t nd = live_span(Dd.st.offsets, Dd.st.counts, d, doff, err);
    const uint32_t ns = live_span(Sd.st.offsets, Sd.st.counts, d, soff, err);
    const uint32_t nt = Sd.tb.offsets ? live_span(Sd.tb.offsets, Sd.tb.counts, d, toff, err) : 0u;
    const Entries D{Dd.st.keys + doff, Dd.st.actors + doff, Dd.st.counters + doff, nd};
    const Entries S{Sd.st.keys + soff, Sd.st.actors + soff, Sd.st.counters + soff, ns};
    const Entries T{nt ? Sd.tb.keys + toff : nullptr, nt ? Sd.tb.actors + toff : nullptr,
                    nt ? Sd.tb.counters + toff : nullptr, nt};
    if (tid < R) {
        sm.dvv[tid] = Dd.st.vv[(size_t)d * R + tid];
        sm.svv[tid] = Sd.st.vv[(size_t)d * R + tid];
    }
    __syncthreads();
    const uint32_t s_actor = Sd.doc_actor ? Sd.doc_actor[d] : Sd.actor;
    const bool full = vv_counter(sm.dvv, R, s_actor, err) == 0ull;  // (every thread reads the same words)
    uint32_t kind = CRDT_DELTA_FULL;
    if (!full) kind = delta_changes<NT>(S, T, sm.dvv, R, err) ? CRDT_DELTA_DELTA : CRDT_DELTA_NONE;
    const bool none = kind == CRDT_DELTA_NONE;
    const uint32_t obase = doff + soff;
    const EntriesOut O{out.keys + obase, out.actors + obase, out.counters + obase};
    uint32_t o, o_rem = 0, o_ups = 0, n_upd = 0;
    bool clock = false;
    if (none) {  // dst as it stands, empty lists
        for (uint32_t t = tid; t < nd; t += NT) {
            O.k[t] = D.k[t];
            O.a[t] = D.a[t];
            O.c[t] = D.c[t];
        }
        o = nd;
    } else {
        LogSink sink{O,
                     {lg.rem_keys + doff, lg.rem_actors + doff, lg.rem_counters + doff},
                     {lg.ups_keys + soff, lg.ups_actors + soff, lg.ups_counters + soff},
                     lg.ups_kind ? lg.ups_kind + soff : nullptr, 0u, 0u, 0u, 0u};
        merge_walk<NT, IPT>(D, S, T, full, R, sm, sink, err);
        o = sink.o;
        o_rem = sink.o_rem;
        o_ups = sink.o_ups;
        block_exclusive_scan<NT>(sink.my_upd, sm.wave_tot, &n_upd);
        clock = __syncthreads_or(tid < R && sm.svv[tid] > sm.dvv[tid]) != 0;
    }
    const uint32_t flags = log_flags(o_rem, o_ups, n_upd, clock);
    if (tid == 0) {
        out.counts[d] = o;
        if (kind_out) kind_out[d] = (uint8_t)kind;
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
        const uint64_t a = sm.dvv[tid], b = sm.svv[tid];
        out.vv[(size_t)d * R + tid] = (none || a > b) ? a : b;
    }
    __syncthreads();  // sm.dvv / sm.svv are the next direction's
}

template <int NT, int IPT, bool EXCH>
__global__ __launch_bounds__(NT) void delta_pair_log_block_kernel(PairSide A, PairSide B, OutView o_ab, OutView o_ba,
                                                                  uint8_t* kind_ab, uint8_t* kind_ba,
                                                                  MergeLogView l_ab, MergeLogView l_ba, Work wk,
                                                                  uint32_t* parts) {
    __shared__ MergeSmem<NT, IPT> sm;
    const uint32_t R = A.st.R, n_docs = A.st.n_docs;
    uint32_t err = 0;
    for_each_work(wk, 0u, n_docs, &sm.word[0], [&](uint32_t d) {
        pair_log_block_dir<NT, IPT>(A, B, d, R, sm, o_ab, kind_ab, l_ab, parts, 0u, err);
        if (EXCH) pair_log_block_dir<NT, IPT>(B, A, d, R, sm, o_ba, kind_ba, l_ba, parts, 1u, err);
    });
    flag_error(wk.status, err);
}

// out_ba / log_ba == nullptr: the join (one direction, a's tombstones unused).
// parts: join_log_parts_bytes() of workspace, used when either log has a summary.
hipError_t launch_delta_pair_log(const PairSide& A, const PairSide& B, const OutView& out_ab, const OutView* out_ba,
                                 uint8_t* kind_ab, uint8_t* kind_ba, const MergeLogView& log_ab,
                                 const MergeLogView* log_ba, const Work& wk, uint32_t* parts, uint32_t block_grid,
                                 hipStream_t stream) {
    const uint32_t n = A.st.n_docs;
    const bool exch = out_ba != nullptr && log_ba != nullptr;
    uint32_t* const s_ab = log_ab.summary;
    uint32_t* const s_ba = exch ? log_ba->summary : nullptr;
    if (n == 0) {  // nothing that reads documents
        if (!s_ab && !s_ba) return hipSuccess;
        return launch_log_zero(s_ab, s_ba, 5u, stream);
    }
    uint32_t* const pp = (s_ab || s_ba) ? parts : nullptr;
    if (pp) {
        const hipError_t e =
            launch_log_zero(pp, nullptr, (uint32_t)(join_log_parts_bytes() / sizeof(uint32_t)), stream);
        if (e != hipSuccess) return e;
    }
    const OutView& o2 = exch ? *out_ba : out_ab;
    const MergeLogView& l2 = exch ? *log_ba : log_ab;
    const dim3 grid((n + kPairLogWaves - 1) / kPairLogWaves), block(kPairLogWaves * 64);
    if (exch)
        hipLaunchKernelGGL((delta_pair_log_wave_kernel<kPairLogWaves, true>), grid, block, 0, stream, A, B, out_ab, o2,
                           kind_ab, kind_ba, log_ab, l2, wk, pp);
    else
        hipLaunchKernelGGL((delta_pair_log_wave_kernel<kPairLogWaves, false>), grid, block, 0, stream, A, B, out_ab, o2,
                           kind_ab, kind_ba, log_ab, l2, wk, pp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (exch)
        hipLaunchKernelGGL((delta_pair_log_block_kernel<kPairLogBlockNT, kPairLogBlockIPT, true>), dim3(block_grid),
                           dim3(kPairLogBlockNT), 0, stream, A, B, out_ab, o2, kind_ab, kind_ba, log_ab, l2, wk, pp);
    else
        hipLaunchKernelGGL((delta_pair_log_block_kernel<kPairLogBlockNT, kPairLogBlockIPT, false>), dim3(block_grid),
                           dim3(kPairLogBlockNT), 0, stream, A, B, out_ab, o2, kind_ab, kind_ba, log_ab, l2, wk, pp);
    e = hipGetLastError();
    if (e != hipSuccess || !pp) return e;
    return launch_log_summary(pp, s_ab, s_ba, exch ? 2u : 1u, stream);
}

}  // namespace crdt
