// Replica select and scatter: a resident replica's documents moved with their
// Deleted tombstones and actors (crdt_replica_select_async,
// crdt_replica_scatter_async; include/crdtgpu.h).  Output document j copies ONE
// source document: the live entries, count and clock, the live tombstones and
// the actor.  Select takes `rep` document idx[j] (j < *n_idx; empty beyond),
// scatter takes `sub` document inv[j] when some idx names j and `rep` document j
// otherwise.  Entries and tombstones are each packed with no slack, so the
// state part is what select_gather_kernel (compare.hip) and
// scatter_gather_kernel (scatter.hip) write, bit for bit.  Up to eight launches,
// ordered by their kernel boundaries alone:
//
//   replica_fill_kernel      scatter only: inv[d] = kRepNone for every document.
//   replica_map_kernel       scatter only, one thread per j < *n_idx:
//       atomicMin(inv[idx[j]], j).  The lowest j naming a document supplies it; a
//       value returned that is not the sentinel is a duplicate, an idx[j] that is
//       no document is skipped: both kErrIndex.  The map is built once and serves
//       the offsets and every gather.
//   replica_count_kernel     the offsets' scan, step 1: the output documents are
//       cut into chunks of kRepScanChunk; workgroup c sums the live entry counts
//       and the live tombstone counts (each clamped to its slots, kErrCapacity)
//       of the chosen sources over chunk c into parts_e[c] and parts_t[c], 64-bit
//       sums stored saturated at 2^32 - 1.  Select's *n_idx clamp and its
//       out-of-range idx[j] are reported here.
//   replica_partials_kernel  step 2, one workgroup: both partial arrays become
//       their exclusive prefixes, kRepPartStep partials per step; the running
//       totals are kept in 64 bits for the checks against entry_slots and
//       tomb_slots, and both offsets[n_out] are written.
//   replica_emit_kernel      step 3: workgroup c rescans its chunk on top of its
//       two partials and writes the counts and offsets of entries and
//       tombstones, and the actors.
//       No workgroup of any step waits for a word another workgroup of the same
//       launch writes: no look-back, no polling.
//   replica_gather_kernel<0> the shape of sources_gather_kernel (sources.hip): the
//       OUTPUT positions are cut into chunks of kRepGatherChunk, grid-stride; the
//       documents of a chunk are found through the offsets just written and
//       staged in LDS (at most kRepRun of them: beyond, lanes search the offsets
//       in global memory) with their side, source slot offset and live count.  A
//       lane takes kRepJ pairs of neighbouring positions; a pair that lies in one
//       document at an even source index is read with 16 B loads (keys,
//       counters; 8 B actors), any other element by element; all loads of a lane
//       are issued before its first store, and the stores of a pair are 16 B.
//       Then the clocks, one lane per actor.
//   replica_gather_kernel<1> the same over the tombstones (launched when some
//       input replica has tombstones).
//
// Workspace: inv, one word per document (scatter), and parts_e / parts_t, one
// word each per chunk of kRepScanChunk documents.
#include "crdt_device.hpp"
#include "merge_block.hpp"
#include "replica.hpp"

namespace crdt {

constexpr int kRepNT = 256;
constexpr int kRepV = 4;                                 // documents per lane and scan chunk
constexpr uint32_t kRepScanChunk = kRepNT * kRepV;       // 1,024 documents per scan workgroup
constexpr int kRepPartNT = 1024;
constexpr uint32_t kRepPartStep = kRepPartNT;            // partials one step of the partials scan holds
constexpr int kRepJ = 4;                                 // pairs of positions per lane and gather chunk
constexpr uint32_t kRepGatherChunk = kRepNT * kRepJ * 2; // 2,048 output positions per gather step
constexpr uint32_t kRepRun = 1024;                       // documents staged in LDS at most
constexpr uint32_t kRepNone = 0xFFFFFFFFu;               // inv: the replica's own document

// Number of elements of the non-decreasing a[0..n) that are <= x.
__device__ __forceinline__ uint32_t rep_count_le(const uint32_t* a, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] <= x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Documents a select takes (the rest of the n_out come out empty).
__device__ __forceinline__ uint32_t rep_n_idx(const ReplicaArgs& s, uint32_t& err) {
    if (s.inv) return 0u;  // (scatter: read by replica_map_kernel alone)
    uint32_t n = s.n_idx ? *s.n_idx : s.n_out;
    if (n > s.n_out) {
        err |= kErrCapacity;
        n = s.n_out;
    }
    return n;
}

// The source of output document j: false = empty; side 1 = sub; d its document there.
__device__ __forceinline__ bool rep_pick(const ReplicaArgs& s, uint32_t j, uint32_t n_idx, uint32_t& side, uint32_t& d,
                                         uint32_t& err) {
    side = 0;
    d = j;
    if (s.inv) {
        const uint32_t x = s.inv[j];  // (holds only x < *n_idx <= sub.n_docs, or the sentinel)
        if (x < s.sub.n_docs) {
            side = 1;
            d = x;
        }
        return true;
    }
    if (j >= n_idx) return false;
    if (s.idx) d = s.idx[j];
    if (d >= s.rep.n_docs) {
        err |= kErrIndex;
        return false;
    }
    return true;
}

__global__ __launch_bounds__(kRepNT) void replica_fill_kernel(uint32_t* inv, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * kRepNT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kRepNT)
        inv[i] = kRepNone;
}

__global__ __launch_bounds__(kRepNT) void replica_map_kernel(const uint32_t* idx, const uint32_t* n_idx_p,
                                                             uint32_t n_sub, uint32_t n_docs, uint32_t* inv,
                                                             uint32_t* status) {
    uint32_t err = 0;
    uint32_t n_idx = n_idx_p ? *n_idx_p : n_sub;
    if (n_idx > n_sub) {
        err |= kErrCapacity;
        n_idx = n_sub;
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kRepNT + threadIdx.x; i < n_idx; i += (uint64_t)gridDim.x * kRepNT) {
        const uint32_t j = (uint32_t)i;
        const uint32_t d = idx[j];
        if (d >= n_docs)
            err |= kErrIndex;  // no document of the replica: this sub document is ignored
        else if (atomicMin(&inv[d], j) != kRepNone)
            err |= kErrIndex;  // named twice: the lowest j stays
    }
    flag_error(status, err);
}

__global__ __launch_bounds__(kRepNT) void replica_count_kernel(ReplicaArgs s, uint32_t* parts_e, uint32_t* parts_t,
                                                               uint32_t* status) {
    __shared__ unsigned long long s_sum[2];
    const uint32_t t = threadIdx.x, n = s.n_out;
    const uint32_t base = blockIdx.x * kRepScanChunk;  // (< n: the grid is the number of chunks)
    const uint32_t m = min(kRepScanChunk, n - base);
    if (t < 2) s_sum[t] = 0;
    __syncthreads();
    uint32_t err = 0;
    const uint32_t n_idx = rep_n_idx(s, err);
    unsigned long long me = 0, mt = 0;
#pragma unroll
    for (int k = 0; k < kRepV; ++k) {
        const uint32_t i = (uint32_t)k * kRepNT + t;
        if (i < m) {
            uint32_t side, d, o;
            if (rep_pick(s, base + i, n_idx, side, d, err)) {
                const RepSide& r = side ? s.sub : s.rep;
                me += (r.e.off ? live_span(r.e.off, r.e.cnt, d, o, err) : 0u);
                mt += (r.t.off ? live_span(r.t.off, r.t.cnt, d, o, err) : 0u);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        me += __shfl_xor(me, o);
        mt += __shfl_xor(mt, o);
    }
    if ((t & 63) == 0) {
        if (me) atomicAdd(&s_sum[0], me);
        if (mt) atomicAdd(&s_sum[1], mt);
    }
    __syncthreads();
    if (t == 0) {
        const unsigned long long se = s_sum[0], st = s_sum[1];
        if (se > (unsigned long long)s.entry_slots || st > (unsigned long long)s.tomb_slots) err |= kErrCapacity;
        parts_e[blockIdx.x] = se > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)se;
        parts_t[blockIdx.x] = st > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)st;
    }
    flag_error(status, err);
}

// One workgroup: parts[0..n_parts) -> exclusive prefixes (u32, as the offsets
// are); returns the u32 total, *over = the 64-bit total exceeds `slots`.
__device__ __forceinline__ uint32_t rep_partials(uint32_t* parts, uint32_t n_parts, uint32_t slots, uint32_t* wave_tot,
                                                 unsigned long long* s_total, bool* over) {
    const uint32_t t = threadIdx.x;
    if (t == 0) *s_total = 0;
    unsigned long long mine = 0;  // (the u32 prefix may wrap on an output that cannot fit: detected here)
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_parts; base += kRepPartStep) {
        const bool in = t < n_parts - base;
        const uint32_t v = in ? parts[base + t] : 0u;
        mine += v;
        uint32_t tot = 0;
        const uint32_t p = carry + block_exclusive_scan<kRepPartNT>(v, wave_tot, &tot);
        if (in) parts[base + t] = p;
        carry += tot;
    }
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((t & 63) == 0 && mine) atomicAdd(s_total, mine);
    __syncthreads();
    *over = *s_total > (unsigned long long)slots;
    __syncthreads();  // (s_total is reused by the next array)
    return carry;
}

// tomb_total may be NULL (no tombstone offsets passed).
__global__ __launch_bounds__(kRepPartNT) void replica_partials_kernel(uint32_t* parts_e, uint32_t* parts_t,
                                                                      uint32_t n_parts, uint32_t entry_slots,
                                                                      uint32_t tomb_slots, uint32_t* entry_total,
                                                                      uint32_t* tomb_total, uint32_t* status) {
    __shared__ uint32_t wave_tot[kRepPartNT / 64];
    __shared__ unsigned long long s_total;
    bool over_e = false, over_t = false;
    const uint32_t te = rep_partials(parts_e, n_parts, entry_slots, wave_tot, &s_total, &over_e);
    const uint32_t tt = rep_partials(parts_t, n_parts, tomb_slots, wave_tot, &s_total, &over_t);
    uint32_t err = 0;
    if (threadIdx.x == 0) {
        *entry_total = te;
        if (tomb_total) *tomb_total = tt;
        if (over_e || over_t) err |= kErrCapacity;
    }
    flag_error(status, err);
}

__global__ __launch_bounds__(kRepNT) void replica_emit_kernel(ReplicaArgs s, const uint32_t* parts_e,
                                                              const uint32_t* parts_t) {
    __shared__ uint32_t wave_tot[kRepNT / 64];
    __shared__ uint32_t run_e[kRepScanChunk];
    __shared__ uint32_t run_t[kRepScanChunk];
    const uint32_t t = threadIdx.x, n = s.n_out;
    const uint32_t base = blockIdx.x * kRepScanChunk;
    const uint32_t m = min(kRepScanChunk, n - base);
    uint32_t err = 0;  // (reported by replica_count_kernel)
    const uint32_t n_idx = rep_n_idx(s, err);
#pragma unroll
    for (int k = 0; k < kRepV; ++k) {
        const uint32_t i = (uint32_t)k * kRepNT + t;
        uint32_t ce = 0, ct = 0;
        if (i < m) {
            uint32_t side, d, o, actor = 0;
            if (rep_pick(s, base + i, n_idx, side, d, err)) {
                const RepSide& r = side ? s.sub : s.rep;
                ce = r.e.off ? live_span(r.e.off, r.e.cnt, d, o, err) : 0u;
                ct = r.t.off ? live_span(r.t.off, r.t.cnt, d, o, err) : 0u;
                actor = r.doc_actor ? r.doc_actor[d] : r.actor;
            }
            s.out.counts[base + i] = ce;
            if (s.tout.counts) s.tout.counts[base + i] = ct;
            if (s.out_actor) s.out_actor[base + i] = actor;
        }
        run_e[i] = ce;
        run_t[i] = ct;
    }
    __syncthreads();
    uint32_t ve[kRepV], vt[kRepV], sum_e = 0, sum_t = 0;
#pragma unroll
    for (int k = 0; k < kRepV; ++k) {
        ve[k] = run_e[t * kRepV + k];
        vt[k] = run_t[t * kRepV + k];
        sum_e += ve[k];
        sum_t += vt[k];
    }
    uint32_t tot = 0;
    uint32_t pe = parts_e[blockIdx.x] + block_exclusive_scan<kRepNT>(sum_e, wave_tot, &tot);
    uint32_t pt = parts_t[blockIdx.x] + block_exclusive_scan<kRepNT>(sum_t, wave_tot, &tot);
#pragma unroll
    for (int k = 0; k < kRepV; ++k) {
        run_e[t * kRepV + k] = pe;
        run_t[t * kRepV + k] = pt;
        pe += ve[k];
        pt += vt[k];
    }
    __syncthreads();
    for (uint32_t i = t; i < m; i += kRepNT) {
        s.out.offsets[base + i] = run_e[i];
        if (s.tout.offsets) s.tout.offsets[base + i] = run_t[i];
    }
}

// KIND 0: the entries through out.offsets, then the clocks; KIND 1: the tombstones through tout.offsets.
template <int KIND>
__global__ __launch_bounds__(kRepNT) void replica_gather_kernel(ReplicaArgs s, uint32_t vec) {
    __shared__ uint32_t s_oo[kRepRun];  // output offset of the staged documents
    __shared__ uint32_t s_so[kRepRun];  // slot offset of the source document each copies
    __shared__ uint32_t s_n[kRepRun];   // live count
    __shared__ uint32_t s_sd[kRepRun];  // 1: the source is the sub-replica
    const uint32_t t = threadIdx.x, n_out = s.n_out;
    const SrcCols c_rep = KIND ? s.rep.t : s.rep.e;
    const SrcCols c_sub = KIND ? s.sub.t : s.sub.e;
    const uint32_t* ooff = KIND ? s.tout.offsets : s.out.offsets;
    const uint32_t* ocnt = KIND ? s.tout.counts : s.out.counts;
    uint64_t* okeys = KIND ? s.tout.keys : s.out.keys;
    uint32_t* oactors = KIND ? s.tout.actors : s.out.actors;
    uint64_t* ocounters = KIND ? s.tout.counters : s.out.counters;
    uint32_t err = 0;  // (reported by replica_count_kernel)
    const uint32_t n_idx = rep_n_idx(s, err);
    // nothing is written at or past the slots, whatever the scan found
    const uint32_t total = min(ooff[n_out], KIND ? s.tomb_slots : s.entry_slots);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)total + kRepGatherChunk - 1) / kRepGatherChunk);

    // output document j: its output offset, the side, slot offset and (clamped) live count of its source
    auto doc = [&](uint32_t j, uint32_t& oo, uint32_t& so, uint32_t& n, uint32_t& sd) {
        oo = ooff[j];
        n = ocnt[j];  // (clamped to the source's slots by replica_emit_kernel)
        so = 0;
        sd = 0;
        uint32_t d;
        if (n && rep_pick(s, j, n_idx, sd, d, err)) {
            const uint32_t* off = sd ? c_sub.off : c_rep.off;
            so = off[d];  // (n != 0: this side has the columns)
        } else {
            n = 0;
        }
    };

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t base = chunk * kRepGatherChunk;
        const uint32_t m = min(kRepGatherChunk, total - base);
        // Documents of the chunk's first and last position.  The search runs over
        // ooff[1 .. n_out), so whatever the offsets hold the answer is a document.
        const uint32_t j_lo = rep_count_le(ooff + 1, n_out - 1, base);
        const uint32_t j_hi = j_lo + rep_count_le(ooff + 1 + j_lo, n_out - 1 - j_lo, base + (m - 1));
        const uint32_t span = j_hi - j_lo + 1;
        const bool staged = span <= kRepRun;
        if (staged) {
            for (uint32_t x = t; x < span; x += kRepNT) {
                uint32_t oo, so, n, sd;
                doc(j_lo + x, oo, so, n, sd);
                s_oo[x] = oo;
                s_so[x] = so;
                s_n[x] = n;
                s_sd[x] = sd;
            }
            __syncthreads();
        }
        // position p of the output: (copied, index in its source's columns, the side,
        // entries left in its document)
        auto locate = [&](uint32_t p, uint32_t& at, uint32_t& sd, uint32_t& left) {
            uint32_t oo, so, n;
            if (staged) {
                const uint32_t x = rep_count_le(s_oo + 1, span - 1, p);
                oo = s_oo[x];
                so = s_so[x];
                n = s_n[x];
                sd = s_sd[x];
            } else {
                doc(j_lo + rep_count_le(ooff + 1 + j_lo, span - 1, p), oo, so, n, sd);
            }
            const uint32_t i = p - oo;  // (below the document: wraps, never < n)
            at = so + i;
            left = i < n ? n - i : 0u;
            return i < n;
        };

        uint32_t c0[kRepJ], c1[kRepJ], e0[kRepJ], e1[kRepJ];
        bool m0[kRepJ], m1[kRepJ], v[kRepJ];
#pragma unroll
        for (int j = 0; j < kRepJ; ++j) {
            const uint32_t rel = 2u * ((uint32_t)j * kRepNT + t);
            c0[j] = c1[j] = e0[j] = e1[j] = 0;
            m0[j] = m1[j] = false;
            if (rel < m) {
                uint32_t left = 0;
                m0[j] = locate(base + rel, c0[j], e0[j], left);
                if (rel + 1 < m) {
                    if (left > 1) {  // the neighbour is the same document's next entry
                        c1[j] = c0[j] + 1;
                        e1[j] = e0[j];
                        m1[j] = true;
                    } else {
                        uint32_t l1;
                        m1[j] = locate(base + rel + 1, c1[j], e1[j], l1);
                    }
                }
            }
            v[j] = (vec & 1u) && m0[j] && m1[j] && e1[j] == e0[j] && c1[j] == c0[j] + 1 && (c0[j] & 1u) == 0u;
        }
        uint64_t k0[kRepJ], k1[kRepJ], n0[kRepJ], n1[kRepJ];
        uint32_t a0[kRepJ], a1[kRepJ];
#pragma unroll
        for (int j = 0; j < kRepJ; ++j) {
            k0[j] = k1[j] = n0[j] = n1[j] = 0;
            a0[j] = a1[j] = 0;
            const SrcCols& b0 = e0[j] ? c_sub : c_rep;
            const SrcCols& b1 = e1[j] ? c_sub : c_rep;
            if (v[j]) {
                const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(b0.keys + c0[j]);
                const ulonglong2 y = *reinterpret_cast<const ulonglong2*>(b0.counters + c0[j]);
                const uint2 z = *reinterpret_cast<const uint2*>(b0.actors + c0[j]);
                k0[j] = x.x;
                k1[j] = x.y;
                n0[j] = y.x;
                n1[j] = y.y;
                a0[j] = z.x;
                a1[j] = z.y;
            } else {
                if (m0[j]) {
                    k0[j] = b0.keys[c0[j]];
                    n0[j] = b0.counters[c0[j]];
                    a0[j] = b0.actors[c0[j]];
                }
                if (m1[j]) {
                    k1[j] = b1.keys[c1[j]];
                    n1[j] = b1.counters[c1[j]];
                    a1[j] = b1.actors[c1[j]];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kRepJ; ++j) {
            const size_t p0 = (size_t)base + 2u * ((uint32_t)j * kRepNT + t);
            if (m0[j] && m1[j] && (vec & 2u)) {  // (p0 is even: the output side of a pair is always aligned)
                *reinterpret_cast<ulonglong2*>(okeys + p0) = make_ulonglong2(k0[j], k1[j]);
                *reinterpret_cast<ulonglong2*>(ocounters + p0) = make_ulonglong2(n0[j], n1[j]);
                *reinterpret_cast<uint2*>(oactors + p0) = make_uint2(a0[j], a1[j]);
            } else {
                if (m0[j]) {
                    okeys[p0] = k0[j];
                    ocounters[p0] = n0[j];
                    oactors[p0] = a0[j];
                }
                if (m1[j]) {
                    okeys[p0 + 1] = k1[j];
                    ocounters[p0 + 1] = n1[j];
                    oactors[p0 + 1] = a1[j];
                }
            }
        }
        __syncthreads();  // (the staged arrays are reused by the next chunk)
    }

    if (KIND == 0) {
        // clocks: n_out x R words, one lane per actor, from the side that supplies the
        // document; an empty document's are zeros
        const uint32_t R = s.R;
        const uint64_t nw = (uint64_t)n_out * R;
        for (uint64_t w = (uint64_t)blockIdx.x * kRepNT + t; w < nw; w += (uint64_t)gridDim.x * kRepNT) {
            const uint32_t j = (uint32_t)(w / R);
            const uint32_t r = (uint32_t)(w - (uint64_t)j * R);
            uint32_t side, d;
            uint64_t x = 0;
            if (rep_pick(s, j, n_idx, side, d, err)) x = (side ? s.sub.vv : s.rep.vv)[(size_t)d * R + r];
            s.out.vv[w] = x;
        }
    }
}

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static bool cols_aligned(const SrcCols& c) {
    return aligned(c.keys, 16) && aligned(c.counters, 16) && aligned(c.actors, 8);
}

// The inverse map of a scatter, for launch_replica below and for the in-place
// scatter (replica_inplace.hip): fill, then map.  n > 0.
hipError_t launch_replica_map(const uint32_t* idx, const uint32_t* n_idx, uint32_t n_sub, uint32_t n, uint32_t* inv,
                              uint32_t* status, uint32_t n_cu, hipStream_t stream) {
    const uint32_t fgrid = min((n + (uint32_t)kRepNT - 1u) / (uint32_t)kRepNT, n_cu * 8u);
    hipLaunchKernelGGL(replica_fill_kernel, dim3(fgrid), dim3(kRepNT), 0, stream, inv, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t mgrid = max(1u, min((uint32_t)(((uint64_t)n_sub + kRepNT - 1) / kRepNT), n_cu * 8u));
    hipLaunchKernelGGL(replica_map_kernel, dim3(mgrid), dim3(kRepNT), 0, stream, idx, n_idx, n_sub, n, inv, status);
    return hipGetLastError();
}

// a.inv != NULL: scatter (a.inv is also the n_out workspace words the map is built
// in); parts_e, parts_t: one workspace word each per kRepScanChunk documents.
// a.n_out == 0: only offsets[0] (= 0) of the entries and the tombstones are written.
hipError_t launch_replica(const ReplicaArgs& a, uint32_t* inv, uint32_t* parts_e, uint32_t* parts_t, uint32_t* status,
                          uint32_t n_cu, hipStream_t stream) {
    const uint32_t n = a.n_out;
    const uint32_t n_parts = (uint32_t)(((uint64_t)n + kRepScanChunk - 1) / kRepScanChunk);
    hipError_t e = hipSuccess;
    if (n) {
        if (inv && (e = launch_replica_map(a.idx, a.n_idx, a.sub.n_docs, n, inv, status, n_cu, stream)) != hipSuccess)
            return e;
        hipLaunchKernelGGL(replica_count_kernel, dim3(n_parts), dim3(kRepNT), 0, stream, a, parts_e, parts_t, status);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(replica_partials_kernel, dim3(1), dim3(kRepPartNT), 0, stream, parts_e, parts_t, n_parts,
                       a.entry_slots, a.tomb_slots, a.out.offsets + n, a.tout.offsets ? a.tout.offsets + n : nullptr,
                       status);
    if ((e = hipGetLastError()) != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(replica_emit_kernel, dim3(n_parts), dim3(kRepNT), 0, stream, a, parts_e, parts_t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // bit 0: both sources' columns allow 16 B loads; bit 1: the output's allow 16 B stores
    const bool two = a.inv != nullptr;
    const bool vin_e = cols_aligned(a.rep.e) && (!two || cols_aligned(a.sub.e));
    const bool vout_e = aligned(a.out.keys, 16) && aligned(a.out.counters, 16) && aligned(a.out.actors, 8);
    hipLaunchKernelGGL(replica_gather_kernel<0>, dim3(n_cu * 8u), dim3(kRepNT), 0, stream, a,
                       (vin_e ? 1u : 0u) | (vout_e ? 2u : 0u));
    const bool any_t = a.rep.t.off || (two && a.sub.t.off);
    if ((e = hipGetLastError()) != hipSuccess || !any_t) return e;
    const bool vin_t = (!a.rep.t.off || cols_aligned(a.rep.t)) && (!two || !a.sub.t.off || cols_aligned(a.sub.t));
    const bool vout_t = aligned(a.tout.keys, 16) && aligned(a.tout.counters, 16) && aligned(a.tout.actors, 8);
    hipLaunchKernelGGL(replica_gather_kernel<1>, dim3(n_cu * 8u), dim3(kRepNT), 0, stream, a,
                       (vin_t ? 1u : 0u) | (vout_t ? 2u : 0u));
    return hipGetLastError();
}

}  // namespace crdt
