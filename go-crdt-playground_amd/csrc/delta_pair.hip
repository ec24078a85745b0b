// Delta-state merge of a resident replica pair: out_ab[d] = a[d] <- b[d] and
// (exchange) out_ba[d] = b[d] <- a[d], each one (*AWSetDelta).Merge
// (awset-delta_test.go:51-65), from one read of both replicas.  The replicas
// stay in the shape apply, scatter, the joins and the folds write (state,
// Deleted, actor): no packed source batch is built.
//
// A direction dst <- src of one document, s = src's actor, D / S the clocks as
// they were before the call:
//   FULL   D.Counter(s) == 0 (:53): merge(S, src.Entries), tombstones ignored
//   DELTA  otherwise, when some src entry has a dot D has not seen (changed,
//          :84-92) or some src tombstone passes the re-add filter (:93-102):
//          deltaMerge (:107-166), clock max(D, S)
//   NONE   otherwise (:60): dst's live entries and dst's clock, unchanged
// The per-key rule of FULL and DELTA is decide() of merge_block.hpp.
//
// Two paths, one launch each:
//  * delta_pair_wave_kernel: one wavefront per document when both sides hold
//    <= 64 live entries and <= 64 live tombstones.  Both entry lists, both
//    tombstone lists and both clocks are staged in LDS once and both directions
//    are decided from that staging.  Lane i owns entry i of each side; a lookup
//    on the other side is an LDS binary search.  The kind of a direction is
//    taken first (Counter, then a ballot over changed and over the effective
//    tombstones); then every lane decides its two keys and the survivors are
//    compacted by ballot and popcount, as in join_wave_kernel, so the output is
//    sorted by key and written once.  Larger documents go to the worklist.
//    Staging, lookup, survivor placement, clock and slot bounds are shared with
//    the logged join (merge_wave.hpp); the kind and the tombstones are here.
//  * delta_pair_block_kernel: workgroups pop the worklist (for_each_work,
//    merge_block.hpp); per direction one pass over src's entries and
//    tombstones takes the kind (delta_changes), then block_merge runs in full
//    or delta mode, or dst is copied for NONE.
#include "crdt_device.hpp"
#include "merge_block.hpp"
#include "merge_wave.hpp"

namespace crdt {

constexpr int kPairWaves = 4;      // wavefronts (= documents) per workgroup of the wave path
constexpr int kPairWaveMax = 64;   // live entries, and live tombstones, per side the wave path takes
constexpr int kPairBlockNT = 256;  // block path: threads per workgroup
constexpr int kPairBlockIPT = 4;   // block path: merged positions per thread and window
// (PairWaveSmem and the kind of a direction: merge_wave.hpp, shared with delta_pair_log.hip)

// One direction of a wave-path document: dst = side x of sm, src = side 1 - x.
__device__ __forceinline__ void pair_wave_dir(const PairWaveSmem& sm, uint32_t x, uint32_t nd, uint32_t ns,
                                              uint32_t nts, uint32_t s_actor, uint32_t R, uint32_t d,
                                              uint32_t obase, const OutView& out, uint8_t* kind_out, uint32_t lane,
                                              uint32_t& err) {
    const uint32_t y = 1u - x;
    const WaveDir p = wave_lookup(sm, x, nd, ns, lane);
    const Entries tomb{sm.tk[y], sm.ta[y], sm.tc[y], nts};

    // the kind, before any entry is decided (:53, :60)
    bool full;
    const uint32_t kind = pair_wave_kind(sm, p, y, ns, nts, s_actor, R, lane, full, err);

    bool dkeep = false, skeep = false;
    uint32_t oda = p.Da, osa = p.Sa;
    uint64_t odc = p.Dc, osc = p.Sc;
    if (kind == CRDT_DELTA_NONE) {
        dkeep = p.dv;
    } else {
        if (p.dv)
            dkeep = decide(true, p.Da, p.Dc, p.dmatch, p.ja, p.jc, full, p.dvv, p.svv, R, tomb, p.Dk, oda, odc, err);
        if (p.sv && !p.smatch)
            skeep = decide(false, 0u, 0ull, true, p.Sa, p.Sc, full, p.dvv, p.svv, R, tomb, p.Sk, osa, osc, err);
    }
    const uint32_t n_out = wave_place(p, dkeep, oda, odc, skeep, osa, osc, out, obase);
    if (lane == 0) {
        out.counts[d] = n_out;
        if (kind_out) kind_out[d] = (uint8_t)kind;
    }
    wave_clock(p, kind == CRDT_DELTA_NONE, out, d, R, lane);  // (:165; NONE: untouched)
}

// EXCH: also out_ba = b <- a.  Without it a's tombstones are never read (A.tb is empty).
template <int WAVES, bool EXCH>
__global__ __launch_bounds__(WAVES * 64) void delta_pair_wave_kernel(PairSide A, PairSide B, OutView o_ab,
                                                                     OutView o_ba, uint8_t* kind_ab, uint8_t* kind_ba,
                                                                     Work wk) {
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
    const uint32_t obase = ao + bo;

    if (lane == 0) {
        pair_bounds(o_ab.offsets, nullptr, nullptr, A.st.offsets, B.st.offsets, d, n_docs, ao, bo);
        if (EXCH) pair_bounds(o_ba.offsets, nullptr, nullptr, B.st.offsets, A.st.offsets, d, n_docs, bo, ao);
    }
    if (na > kPairWaveMax || nb > kPairWaveMax || nta > kPairWaveMax || ntb > kPairWaveMax) {
        if (lane == 0) push_work(wk, d, n_docs);
        flag_error(wk.status, err);
        return;
    }

    wave_stage_pair(sm, A.st, B.st, d, ao, na, bo, nb, lane);
    wave_stage(sm.tk[0], sm.ta[0], sm.tc[0], A.tb.keys, A.tb.actors, A.tb.counters, ato, nta, lane);
    wave_stage(sm.tk[1], sm.ta[1], sm.tc[1], B.tb.keys, B.tb.actors, B.tb.counters, bto, ntb, lane);
    wave_sync();

    const uint32_t b_actor = B.doc_actor ? B.doc_actor[d] : B.actor;
    pair_wave_dir(sm, 0u, na, nb, ntb, b_actor, R, d, obase, o_ab, kind_ab, lane, err);
    if (EXCH) {
        const uint32_t a_actor = A.doc_actor ? A.doc_actor[d] : A.actor;
        pair_wave_dir(sm, 1u, nb, na, nta, a_actor, R, d, obase, o_ba, kind_ba, lane, err);
    }
    flag_error(wk.status, err);
}

// One direction of a block-path document, by the whole workgroup.
template <int NT, int IPT>
__device__ __forceinline__ void pair_block_dir(const PairSide& Dd, const PairSide& Sd, uint32_t d, uint32_t R,
                               MergeSmem<NT, IPT>& sm, const OutView& out, uint8_t* kind_out, uint32_t& err) {
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
    const uint32_t obase = doff + soff;
    const EntriesOut O{out.keys + obase, out.actors + obase, out.counters + obase};
    uint32_t n;
    if (kind == CRDT_DELTA_NONE) {
        for (uint32_t t = tid; t < nd; t += NT) {
            O.k[t] = D.k[t];
            O.a[t] = D.a[t];
            O.c[t] = D.c[t];
        }
        n = nd;
    } else {
        n = block_merge<NT, IPT>(D, S, T, full, R, sm, O, err);
    }
    if (tid == 0) {
        out.counts[d] = n;
        if (kind_out) kind_out[d] = (uint8_t)kind;
    }
    if (tid < R) {
        const uint64_t a = sm.dvv[tid], b = sm.svv[tid];
        out.vv[(size_t)d * R + tid] = (kind == CRDT_DELTA_NONE || a > b) ? a : b;
    }
    __syncthreads();  // sm.dvv / sm.svv are the next direction's
}

template <int NT, int IPT, bool EXCH>
__global__ __launch_bounds__(NT) void delta_pair_block_kernel(PairSide A, PairSide B, OutView o_ab, OutView o_ba,
                                                              uint8_t* kind_ab, uint8_t* kind_ba, Work wk) {
    __shared__ MergeSmem<NT, IPT> sm;
    const uint32_t R = A.st.R, n_docs = A.st.n_docs;
    uint32_t err = 0;
    for_each_work(wk, 0u, n_docs, &sm.word[0], [&](uint32_t d) {
        pair_block_dir<NT, IPT>(A, B, d, R, sm, o_ab, kind_ab, err);
        if (EXCH) pair_block_dir<NT, IPT>(B, A, d, R, sm, o_ba, kind_ba, err);
    });
    flag_error(wk.status, err);
}

// out_ba == nullptr: the join (one direction, a's tombstones unused).
hipError_t launch_delta_pair(const PairSide& A, const PairSide& B, const OutView& out_ab, const OutView* out_ba,
                             uint8_t* kind_ab, uint8_t* kind_ba, const Work& wk, uint32_t block_grid,
                             hipStream_t stream) {
    const uint32_t n = A.st.n_docs;
    if (n == 0) return hipSuccess;
    const dim3 grid((n + kPairWaves - 1) / kPairWaves), block(kPairWaves * 64);
    if (out_ba)
        hipLaunchKernelGGL((delta_pair_wave_kernel<kPairWaves, true>), grid, block, 0, stream, A, B, out_ab, *out_ba,
                           kind_ab, kind_ba, wk);
    else
        hipLaunchKernelGGL((delta_pair_wave_kernel<kPairWaves, false>), grid, block, 0, stream, A, B, out_ab, out_ab,
                           kind_ab, kind_ba, wk);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (out_ba)
        hipLaunchKernelGGL((delta_pair_block_kernel<kPairBlockNT, kPairBlockIPT, true>), dim3(block_grid),
                           dim3(kPairBlockNT), 0, stream, A, B, out_ab, *out_ba, kind_ab, kind_ba, wk);
    else
        hipLaunchKernelGGL((delta_pair_block_kernel<kPairBlockNT, kPairBlockIPT, false>), dim3(block_grid),
                           dim3(kPairBlockNT), 0, stream, A, B, out_ab, out_ab, kind_ab, kind_ba, wk);
    return hipGetLastError();
}

}  // namespace crdt
