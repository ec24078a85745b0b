// Logged fold: out[d] = (((dst[d] <- src[d][0]) <- src[d][1]) ... ) as fold.hip
// writes it (mode CRDT_FOLD_AWSET: each step (*AWSet).Merge, awset.go:103-161;
// CRDT_FOLD_DELTA: (*AWSetDelta).Merge, awset-delta_test.go:51-166), and beside it
// the log of the whole ordered fold in the logged join's records (join_log.hip):
// the dst entries that are gone at the end, the entries that are new or sit under
// another dot at the end.  It is crdt_awset_diff_async(dst, out)'s answer: the net
// effect, so a key a step removes and a later step brings back under its old dot
// leaves no record, and a key added and removed again none either.
//
// Layout.  The removed list of document d starts at dst.offsets[d] (a removed
// entry was a dst entry).  The upserted list starts at entry_off[doc_srcs[d]] and
// has the document's source entry slots for capacity: an upserted key's final dot
// differs from the one dst held for it (or dst held none), and a step only ever
// gives a key the dot of that step's source entry for it, so every upserted key
// is the key of some source entry of d, and distinct keys need distinct entries.
//
// This is the plain form beside the tuned fold kernels, which are not touched:
// the steps are taken one at a time, with the rule (decide, merge_block.hpp) and
// the step's kind (pair_wave_kind / delta_changes) called, not restated.
//  * fold_log_wave_kernel: one wavefront per document while dst's live entries,
//    every source's entries and tombstones and the state after every step hold
//    <= 64.  dst is staged twice in the wave's LDS: a copy that stays as it is and
//    the running state, which each step rewrites in place (the lanes hold their
//    entries in registers by then; survivors placed by ballot, wave_place).
//    Nothing of the document reaches global memory before its last step, so a
//    document that outgrows the wave at some step is handed to the worklist as it
//    was.  At the end the survivors go to out and the kept copy is compared with
//    them: ranks by ballot and popcount.
//  * fold_log_block_kernel: the worklist's documents, by fold_block_kernel's own
//    step loop (fold_block_doc), and then one more window walk of dst[d] against
//    out[d] (diff_walk, merge_log.hpp) that writes the two lists.  That is a
//    second read of a large document; the lean passes' log is left for later.
// The summary is summed as the logged join's (merge_log.hpp), one direction.
#include "crdt_device.hpp"
#include "merge_block.hpp"
#include "merge_log.hpp"
#include "merge_wave.hpp"

namespace crdt {

constexpr int kFoldLogWaves = 4;     // wavefronts per workgroup of the wave path
constexpr int kFoldLogDocs = 4;      // consecutive documents a wavefront takes in turn
constexpr int kFoldLogWaveMax = 64;  // entries of any list, and of the running state, the wave path takes
constexpr int kFoldLogBlockNT = 256;  // block path: threads per workgroup
constexpr int kFoldLogBlockIPT = 4;   // block path: merged positions per thread and window

// Slot bounds of document d's three outputs, from the inputs' own (dst's slots
// start at doff, the sources' entry slots at eoff).  Every document, whichever
// path folds it; the last one closes the columns.
__device__ __forceinline__ void fold_log_bounds(const OutView& out, const MergeLogView& lg, const BatchView& dst,
                                                const SrcView& sb, uint32_t d, uint32_t doff, uint32_t eoff) {
    out.offsets[d] = doff + eoff;
    lg.rem_offsets[d] = doff;
    lg.ups_offsets[d] = eoff;
    if (d == dst.n_docs - 1) {
        const uint32_t de = dst.offsets[dst.n_docs], ee = sb.entry_off[sb.doc_srcs[dst.n_docs]];
        out.offsets[dst.n_docs] = de + ee;
        lg.rem_offsets[dst.n_docs] = de;
        lg.ups_offsets[dst.n_docs] = ee;
    }
}

// One document by one wavefront.  sm side 0: the running state and its clock;
// side 1: the step's source, its clock and its tombstones; side 0's tombstone
// columns (a fold's dst has none) hold the copy of dst that stays as it is.
// Returns false when the document is left to the block path (nothing written but
// its slot bounds).
__device__ __forceinline__ bool fold_log_wave_doc(PairWaveSmem& sm, bool delta, const BatchView& dst, const SrcView& sb,
                                                  const OutView& out, const MergeLogView& lg, uint32_t d, uint32_t lane,
                                                  LogSums& sums, uint32_t& err) {
    const uint32_t R = dst.R;
    const bool tombs = delta && sb.tomb_off != nullptr;
    uint32_t doff;
    const uint32_t nb = uniform(live_span(dst.offsets, dst.counts, d, doff, err));
    doff = uniform(doff);
    const uint32_t dslots = uniform(dst.offsets[d + 1]) - doff;
    const uint32_t s0 = uniform(sb.doc_srcs[d]), s1 = uniform(sb.doc_srcs[d + 1]);
    const uint32_t eoff = uniform(sb.entry_off[s0]);
    const uint32_t ecap = uniform(sb.entry_off[s1]) - eoff;  // the sources' entry slots: the upserted list's
    if (lane == 0) fold_log_bounds(out, lg, dst, sb, d, doff, eoff);
    if (nb > kFoldLogWaveMax) return false;

    uint64_t* const bk = sm.tk[0];  // dst as it was
    uint64_t* const bc = sm.tc[0];
    uint32_t* const ba = sm.ta[0];
    wave_sync();  // the previous document's reads are done
    if (lane < nb) {
        const uint64_t k = dst.keys[doff + lane], c = dst.counters[doff + lane];
        const uint32_t a = dst.actors[doff + lane];
        bk[lane] = sm.ek[0][lane] = k;
        bc[lane] = sm.ec[0][lane] = c;
        ba[lane] = sm.ea[0][lane] = a;
    }
    const uint64_t v0 = lane < R ? dst.vv[(size_t)d * R + lane] : 0ull;  // dst's clock, for CRDT_DIFF_CLOCK
    if (lane < R) sm.vv[0][lane] = v0;

    const OutView run{nullptr, nullptr, sm.ek[0], sm.ea[0], sm.ec[0], nullptr};  // wave_place's target: the running state
    uint32_t nc = nb;  // live entries of the running state
    for (uint32_t k = s0; k < s1; ++k) {
        const uint32_t eo = uniform(sb.entry_off[k]);
        const uint32_t ns = uniform(sb.entry_off[k + 1]) - eo;
        uint32_t to = 0, nt = 0;
        if (tombs) {
            to = uniform(sb.tomb_off[k]);
            nt = uniform(sb.tomb_off[k + 1]) - to;
        }
        if (ns > kFoldLogWaveMax || nt > kFoldLogWaveMax) return false;
        const uint32_t s_actor = uniform(sb.src_actor[k]);
        if (delta && s_actor == R) {  // Counter(src.Actor) panics (awset-delta_test.go:53): the fold of d ends here
            err |= kErrActorRange;
            break;
        }
        wave_sync();  // the previous step's reads of side 1 are done
        wave_stage(sm.ek[1], sm.ea[1], sm.ec[1], sb.keys, sb.actors, sb.counters, eo, ns, lane);
        wave_stage(sm.tk[1], sm.ta[1], sm.tc[1], sb.tkeys, sb.tactors, sb.tcounters, to, nt, lane);
        if (lane < R) sm.vv[1][lane] = sb.vv[(size_t)k * R + lane];
        wave_sync();

        const WaveDir p = wave_lookup(sm, 0u, nc, ns, lane);
        bool full = true;
        if (delta && pair_wave_kind(sm, p, 1u, ns, nt, s_actor, R, lane, full, err) == CRDT_DELTA_NONE)
            continue;  // nothing changed, nothing deleted: not even the clocks are merged (:60)
        const Entries tomb{sm.tk[1], sm.ta[1], sm.tc[1], full ? 0u : nt};
        bool dkeep = false, skeep = false;
        uint32_t oda = p.Da, osa = p.Sa;
        uint64_t odc = p.Dc, osc = p.Sc;
        if (p.dv) dkeep = decide(true, p.Da, p.Dc, p.dmatch, p.ja, p.jc, full, p.dvv, p.svv, R, tomb, p.Dk, oda, odc, err);
        if (p.sv && !p.smatch)  // (a common key is decided where its dst lane sees it)
            skeep = decide(false, 0u, 0ull, true, p.Sa, p.Sc, full, p.dvv, p.svv, R, tomb, p.Sk, osa, osc, err);
        const uint32_t n_new = popc(ballot(dkeep)) + popc(ballot(skeep));
        if (n_new > kFoldLogWaveMax) return false;  // outgrows the wave: the block path folds d from the start
        const uint64_t vmax = lane < R ? max(p.dvv[lane], p.svv[lane]) : 0ull;
        wave_sync();  // every lane holds its entries and decisions in registers: the state is rewritten in place
        wave_place(p, dkeep, oda, odc, skeep, osa, osc, run, 0u);
        if (lane < R) sm.vv[0][lane] = vmax;
        nc = n_new;
    }
    wave_sync();

    // the survivors and the clock; nc <= the document's output slots (each survivor is a dst or a source entry)
    const uint32_t obase = doff + eoff;
    const bool fv = lane < nc && lane < dslots + ecap;
    const uint64_t Fk = sm.ek[0][lane], Fc = sm.ec[0][lane];
    const uint32_t Fa = sm.ea[0][lane];
    if (fv) {
        out.keys[obase + lane] = Fk;
        out.actors[obase + lane] = Fa;
        out.counters[obase + lane] = Fc;
    }
    const uint64_t v1 = lane < R ? sm.vv[0][lane] : 0ull;
    if (lane < R) out.vv[(size_t)d * R + lane] = v1;

    // dst as it was against the survivors: each side's lanes look their key up on the other
    const bool bv = lane < nb;
    const uint64_t Bk = bk[lane], Bc = bc[lane];
    const uint32_t Ba = ba[lane];
    const uint32_t j = lower_bound_pow<6>(sm.ek[0], nc, Bk);
    const bool removed = bv && !(j < nc && sm.ek[0][j & 63] == Bk);
    const uint32_t i = lower_bound_pow<6>(bk, nb, Fk);
    const bool fmatch = fv && i < nb && bk[i & 63] == Fk;
    const bool upd = fmatch && (ba[i & 63] != Fa || bc[i & 63] != Fc);
    const bool ups = fv && (!fmatch || upd);
    // a log record's slot: its kind's lanes below it
    const uint64_t rm = ballot(removed), um = ballot(ups), updm = ballot(upd);
    const uint32_t n_rem = popc(rm), n_ups = popc(um), n_upd = popc(updm);  // <= nb; <= ecap (header comment)
    if (removed) {
        const uint32_t q = doff + below(rm);
        lg.rem_keys[q] = Bk;
        lg.rem_actors[q] = Ba;
        lg.rem_counters[q] = Bc;
    }
    const uint32_t ur = below(um);
    if (ups && ur < ecap) {
        const uint32_t q = eoff + ur;
        lg.ups_keys[q] = Fk;
        lg.ups_actors[q] = Fa;
        lg.ups_counters[q] = Fc;
        if (lg.ups_kind) lg.ups_kind[q] = (uint8_t)(upd ? CRDT_DIFF_UPDATED : CRDT_DIFF_ADDED);
    }
    const uint32_t flags = log_flags(n_rem, n_ups, n_upd, ballot(v0 != v1) != 0ull);
    if (lane == 0) {
        out.counts[d] = nc;
        lg.flags[d] = (uint8_t)flags;
        lg.rem_counts[d] = n_rem;
        lg.ups_counts[d] = n_ups;
    }
    sums_add(sums, n_rem, n_ups, n_upd, flags);
    return true;
}

// parts == nullptr: no summary asked for.
template <int WAVES, int DOCS>
__global__ __launch_bounds__(WAVES * 64) void fold_log_wave_kernel(int mode, BatchView dst, SrcView sb, OutView out,
                                                                   MergeLogView lg, Work wk, uint32_t* parts) {
    __shared__ PairWaveSmem smem[WAVES];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t n_docs = dst.n_docs;
    const uint32_t wave = uniform(blockIdx.x * WAVES + w);
    const uint32_t first = wave * DOCS;
    if (first >= n_docs) return;  // (a whole wave; the kernel has no workgroup barrier)
    const uint32_t end = min(first + (uint32_t)DOCS, n_docs);
    uint32_t err = 0;
    LogSums sums{};
    for (uint32_t d = first; d < end; ++d)
        if (!fold_log_wave_doc(smem[w], mode == CRDT_FOLD_DELTA, dst, sb, out, lg, d, lane, sums, err) && lane == 0)
            push_work(wk, d, n_docs);
    if (parts && lane == 0) sums_flush(parts, 0u, wave, sums);
    flag_error(wk.status, err);
}

template <int NT, int IPT>
__global__ __launch_bounds__(NT) void fold_log_block_kernel(int mode, BatchView dst, SrcView sb, OutView out,
                                                            Scratch scr, MergeLogView lg, Work wk, uint32_t* parts) {
    __shared__ MergeSmem<NT, IPT> sm;
    const uint32_t tid = threadIdx.x;
    const uint32_t R = dst.R;
    uint32_t err = 0;
    for_each_work(wk, 0u, dst.n_docs, &sm.word[0], [&](uint32_t d) {
        const uint32_t n_out = fold_block_doc<NT, IPT>(mode, dst, sb, out, scr, wk, d, sm, err);  // (sm.dvv: the merged clock)
        uint32_t o_rem = 0, o_ups = 0, n_upd = 0;
        bool clock = false;
        if (n_out != kFoldNoDoc) {
            uint32_t doff, reported = 0;  // (fold_block_doc has reported a count above the slots)
            const uint32_t nb = live_span(dst.offsets, dst.counts, d, doff, reported);
            const uint32_t eoff = sb.entry_off[sb.doc_srcs[d]];
            const uint32_t obase = doff + eoff;
            const Entries before{dst.keys + doff, dst.actors + doff, dst.counters + doff, nb};
            const Entries after{out.keys + obase, out.actors + obase, out.counters + obase, n_out};
            DiffSink sink{{lg.rem_keys + doff, lg.rem_actors + doff, lg.rem_counters + doff},
                          {lg.ups_keys + eoff, lg.ups_actors + eoff, lg.ups_counters + eoff},
                          lg.ups_kind ? lg.ups_kind + eoff : nullptr, 0u, 0u, 0u};
            diff_walk<NT, IPT>(before, after, sm, sink);
            o_rem = sink.o_rem;
            o_ups = sink.o_ups;
            block_exclusive_scan<NT>(sink.my_upd, sm.wave_tot, &n_upd);
            clock = __syncthreads_or(tid < R && dst.vv[(size_t)d * R + tid] != sm.dvv[tid]) != 0;
        }
        const uint32_t flags = log_flags(o_rem, o_ups, n_upd, clock);
        if (tid == 0) {  // (a document the scratch is too small for: empty lists)
            lg.flags[d] = (uint8_t)flags;
            lg.rem_counts[d] = o_rem;
            lg.ups_counts[d] = o_ups;
            if (parts) {
                LogSums s{};
                sums_add(s, o_rem, o_ups, n_upd, flags);
                sums_flush(parts, 0u, blockIdx.x, s);
            }
        }
        __syncthreads();  // sm.dvv is the next document's
    });
    if (__syncthreads_or(err != 0) && tid == 0) atomicOr(wk.status, kErrActorRange);
}

// parts: join_log_parts_bytes() of workspace, used when the log has a summary.
hipError_t launch_fold_log(int mode, const BatchView& dst, const SrcView& sb, const OutView& out, const Scratch& scr,
                           const MergeLogView& lg, const Work& wk, uint32_t* parts, uint32_t block_grid,
                           hipStream_t stream) {
    const uint32_t n = dst.n_docs;
    if (n == 0)  // nothing that reads documents
        return lg.summary ? launch_log_zero(lg.summary, nullptr, 5u, stream) : hipSuccess;
    uint32_t* const pp = lg.summary ? parts : nullptr;
    if (pp) {
        const hipError_t e =
            launch_log_zero(pp, nullptr, (uint32_t)(join_log_parts_bytes() / sizeof(uint32_t)), stream);
        if (e != hipSuccess) return e;
    }
    constexpr uint32_t per_block = kFoldLogWaves * kFoldLogDocs;
    hipLaunchKernelGGL((fold_log_wave_kernel<kFoldLogWaves, kFoldLogDocs>), dim3((n + per_block - 1) / per_block),
                       dim3(kFoldLogWaves * 64), 0, stream, mode, dst, sb, out, lg, wk, pp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((fold_log_block_kernel<kFoldLogBlockNT, kFoldLogBlockIPT>), dim3(block_grid),
                       dim3(kFoldLogBlockNT), 0, stream, mode, dst, sb, out, scr, lg, wk, pp);
    e = hipGetLastError();
    if (e != hipSuccess || !pp) return e;
    return launch_log_summary(pp, lg.summary, nullptr, 1u, stream);
}

}  // namespace crdt
