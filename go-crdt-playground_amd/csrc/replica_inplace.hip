// In-place replica scatter (crdt_replica_scatter_inplace_async; include/crdtgpu.h):
// each sub document j that wins its replica document d = idx[j] (the mapping of
// crdt_replica_scatter_async, through the same inverse map) is written into the
// slots d already owns when its live entries AND its live tombstones fit them,
// and is named in the spill lists otherwise.  Nothing is packed and no offset
// moves, so the call touches the bytes of the placed documents alone; the
// packed scatter (replica.hip) rewrites the whole replica.  Up to seven
// launches, ordered by their kernel boundaries alone:
//
//   replica_fill_kernel, replica_map_kernel   replica.hip's, as they stand
//       (launch_replica_map): inv[d] = the lowest j naming d.
//   inplace_verdict_kernel   the spill scan, step 1: the sub documents are cut
//       into chunks of kInpScanChunk; workgroup c writes verdict[j] (ignored:
//       j >= *n_idx, idx[j] no document, or a lower j names the same document;
//       placed; spilled), for a placed document the counts, tombstone counts and
//       actor of d, and the chunk's number of spilled documents into parts[c].
//   inplace_partials_kernel  step 2, one workgroup: parts become their exclusive
//       prefixes, kInpPartStep per step, and *n_spill is written.
//   inplace_emit_kernel      step 3: workgroup c rescans its chunk on top of
//       parts[c] and writes spill_j / spill_doc, ascending in j.
//       No workgroup of any step waits for a word another workgroup of the same
//       launch writes: no look-back, no polling, no atomic decides a position.
//   inplace_gather_kernel<0> replica_gather_kernel's shape turned round: the
//       position space is SUB's own slot space [0, sub.offsets[n_sub]), cut into
//       chunks of kInpGatherChunk, grid-stride, so no scan over positions is
//       needed and position p IS the source index.  The documents of a chunk are
//       found through sub.offsets and staged in LDS (at most kInpRun of them:
//       beyond, lanes search the offsets in global memory) with their slot
//       offset, live count (0 unless placed) and destination base
//       offsets[idx[j]].  A lane takes kInpJ pairs of neighbouring positions (the
//       first of a pair is even).  A pair that lies in one placed document is
//       read with 16 B loads (keys, counters; 8 B actors) when sub's columns are
//       aligned, and stored with 16 B stores when its destination index is even
//       and the replica's columns are aligned; any other element goes one by
//       one.  All loads of a lane are issued before its first store.  A position
//       in slack, in an ignored or in a spilled document loads and stores
//       nothing.  Then the clocks of the placed documents, one lane per word.
//   inplace_gather_kernel<1> the same over the tombstones (launched when both
//       sides have them).
//
// Workspace: inv, one word per replica document; verdict, one per sub document;
// parts, one per chunk of kInpScanChunk sub documents.
#include "crdt_device.hpp"
#include "merge_block.hpp"
#include "replica.hpp"

namespace crdt {

constexpr int kInpNT = 256;
constexpr int kInpV = 4;                                 // documents per lane and scan chunk
constexpr uint32_t kInpScanChunk = kInpNT * kInpV;       // 1,024 sub documents per scan workgroup
constexpr int kInpPartNT = 1024;
constexpr uint32_t kInpPartStep = kInpPartNT;            // partials one step of the partials scan holds
constexpr int kInpJ = 4;                                 // pairs of positions per lane and gather chunk
constexpr uint32_t kInpGatherChunk = kInpNT * kInpJ * 2; // 2,048 sub positions per gather step
constexpr uint32_t kInpRun = 1024;                       // documents staged in LDS at most
constexpr uint32_t kInpIgnored = 0, kInpPlaced = 1, kInpSpilled = 2;

// Number of elements of the non-decreasing a[0..n) that are <= x.
__device__ __forceinline__ uint32_t inp_count_le(const uint32_t* a, uint32_t n, uint32_t x) {
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

__device__ __forceinline__ uint32_t inp_slots(const uint32_t* off, uint32_t d) {
    const uint32_t b = off[d], e = off[d + 1];
    return e > b ? e - b : 0u;
}

__global__ __launch_bounds__(kInpNT) void inplace_verdict_kernel(InplaceArgs s, uint32_t* parts, uint32_t* status) {
    __shared__ uint32_t s_sum;
    const uint32_t t = threadIdx.x, n_sub = s.sub.n_docs;
    const uint32_t base = blockIdx.x * kInpScanChunk;  // (< n_sub: the grid is the number of chunks)
    const uint32_t m = min(kInpScanChunk, n_sub - base);
    if (t == 0) s_sum = 0;
    __syncthreads();
    uint32_t err = 0;
    const uint32_t n_idx = min(s.n_idx ? *s.n_idx : n_sub, n_sub);  // (the clamp is reported by replica_map_kernel)
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kInpV; ++k) {
        const uint32_t i = (uint32_t)k * kInpNT + t;
        if (i >= m) continue;
        const uint32_t j = base + i;
        uint32_t v = kInpIgnored;
        const uint32_t d = j < n_idx ? s.idx[j] : 0xFFFFFFFFu;
        if (d < s.n_docs && s.inv[d] == j) {
            uint32_t o;
            const uint32_t ne = live_span(s.sub.e.off, s.sub.e.cnt, j, o, err);
            const uint32_t nt = s.sub.t.off ? live_span(s.sub.t.off, s.sub.t.cnt, j, o, err) : 0u;
            const uint32_t ce = inp_slots(s.e.off, d);
            const uint32_t ct = s.t.off ? inp_slots(s.t.off, d) : 0u;
            if (ne <= ce && nt <= ct) {
                v = kInpPlaced;
                s.e.cnt[d] = ne;
                if (s.t.off) s.t.cnt[d] = nt;
                if (s.doc_actor) s.doc_actor[d] = s.sub.doc_actor ? s.sub.doc_actor[j] : s.sub.actor;
            } else {
                v = kInpSpilled;
                ++mine;
            }
        }
        s.verdict[j] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((t & 63) == 0 && mine) atomicAdd(&s_sum, mine);  // (a sum: the order of the adds changes no bit)
    __syncthreads();
    if (t == 0) parts[blockIdx.x] = s_sum;
    flag_error(status, err);
}

__global__ __launch_bounds__(kInpPartNT) void inplace_partials_kernel(uint32_t* parts, uint32_t n_parts,
                                                                      uint32_t* n_spill) {
    __shared__ uint32_t wave_tot[kInpPartNT / 64];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;  // (at most the number of sub documents: no wrap)
    for (uint32_t base = 0; base < n_parts; base += kInpPartStep) {
        const bool in = t < n_parts - base;
        const uint32_t v = in ? parts[base + t] : 0u;
        uint32_t tot = 0;
        const uint32_t p = carry + block_exclusive_scan<kInpPartNT>(v, wave_tot, &tot);
        if (in) parts[base + t] = p;
        carry += tot;
    }
    if (t == 0) *n_spill = carry;
}

__global__ __launch_bounds__(kInpNT) void inplace_emit_kernel(InplaceArgs s, const uint32_t* parts) {
    __shared__ uint32_t wave_tot[kInpNT / 64];
    const uint32_t t = threadIdx.x, n_sub = s.sub.n_docs;
    const uint32_t base = blockIdx.x * kInpScanChunk;
    const uint32_t m = min(kInpScanChunk, n_sub - base);
    bool sp[kInpV];
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kInpV; ++k) {  // a lane takes kInpV neighbouring documents, so the lists ascend
        const uint32_t i = t * kInpV + (uint32_t)k;
        sp[k] = i < m && s.verdict[base + i] == kInpSpilled;
        sum += sp[k] ? 1u : 0u;
    }
    uint32_t tot = 0;
    uint32_t pos = parts[blockIdx.x] + block_exclusive_scan<kInpNT>(sum, wave_tot, &tot);
#pragma unroll
    for (int k = 0; k < kInpV; ++k) {
        if (!sp[k]) continue;
        const uint32_t j = base + t * kInpV + (uint32_t)k;
        s.spill_j[pos] = j;  // (pos < the number of spilled documents <= n_sub)
        s.spill_doc[pos] = s.idx[j];
        ++pos;
    }
}

// KIND 0: the entries, then the clocks; KIND 1: the tombstones.
// vec bit 0: sub's columns allow 16 B loads; bit 1: the replica's allow 16 B stores.
template <int KIND>
__global__ __launch_bounds__(kInpNT) void inplace_gather_kernel(InplaceArgs s, uint32_t vec) {
    __shared__ uint32_t s_so[kInpRun];  // slot offset of the staged sub documents
    __shared__ uint32_t s_n[kInpRun];   // live count; 0 unless placed
    __shared__ uint32_t s_do[kInpRun];  // destination base: the replica document's slot offset
    const uint32_t t = threadIdx.x, n_sub = s.sub.n_docs;
    const SrcCols c_sub = KIND ? s.sub.t : s.sub.e;
    const InplaceCols c_rep = KIND ? s.t : s.e;
    const uint32_t* soff = c_sub.off;
    const uint32_t total = soff[n_sub];
    const uint32_t n_chunks = (uint32_t)(((uint64_t)total + kInpGatherChunk - 1) / kInpGatherChunk);

    // sub document j: its slot offset, its live count when placed (0 otherwise), its destination base
    auto doc = [&](uint32_t j, uint32_t& so, uint32_t& n, uint32_t& dst) {
        so = soff[j];
        n = 0;
        dst = 0;
        if (s.verdict[j] == kInpPlaced) {
            n = live_clamped(soff, c_sub.cnt, j);  // (fits d's slots: the verdict)
            dst = c_rep.off[s.idx[j]];
        }
    };

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t base = chunk * kInpGatherChunk;
        const uint32_t m = min(kInpGatherChunk, total - base);
        // Documents of the chunk's first and last position.  The search runs over
        // soff[1 .. n_sub), so whatever the offsets hold the answer is a document.
        const uint32_t j_lo = inp_count_le(soff + 1, n_sub - 1, base);
        const uint32_t j_hi = j_lo + inp_count_le(soff + 1 + j_lo, n_sub - 1 - j_lo, base + (m - 1));
        const uint32_t span = j_hi - j_lo + 1;
        const bool staged = span <= kInpRun;
        if (staged) {
            for (uint32_t x = t; x < span; x += kInpNT) {
                uint32_t so, n, dst;
                doc(j_lo + x, so, n, dst);
                s_so[x] = so;
                s_n[x] = n;
                s_do[x] = dst;
            }
            __syncthreads();
        }
        // sub position p: (moved, its destination index, entries left in its document)
        auto locate = [&](uint32_t p, uint32_t& at, uint32_t& left) {
            uint32_t so, n, dst;
            if (staged) {
                const uint32_t x = inp_count_le(s_so + 1, span - 1, p);
                so = s_so[x];
                n = s_n[x];
                dst = s_do[x];
            } else {
                doc(j_lo + inp_count_le(soff + 1 + j_lo, span - 1, p), so, n, dst);
            }
            const uint32_t i = p - so;  // (below the first document: wraps, never < n)
            at = dst + i;
            left = i < n ? n - i : 0u;
            return i < n;
        };

        uint32_t d0[kInpJ], d1[kInpJ];
        bool m0[kInpJ], m1[kInpJ], pr[kInpJ];
#pragma unroll
        for (int j = 0; j < kInpJ; ++j) {
            const uint32_t rel = 2u * ((uint32_t)j * kInpNT + t);
            d0[j] = d1[j] = 0;
            m0[j] = m1[j] = pr[j] = false;
            if (rel < m) {
                uint32_t left = 0;
                m0[j] = locate(base + rel, d0[j], left);
                if (rel + 1 < m) {
                    if (left > 1) {  // the neighbour is the same document's next entry
                        d1[j] = d0[j] + 1;
                        m1[j] = pr[j] = true;
                    } else {
                        uint32_t l1;
                        m1[j] = locate(base + rel + 1, d1[j], l1);
                    }
                }
            }
        }
        uint64_t k0[kInpJ], k1[kInpJ], n0[kInpJ], n1[kInpJ];
        uint32_t a0[kInpJ], a1[kInpJ];
#pragma unroll
        for (int j = 0; j < kInpJ; ++j) {
            const size_t p0 = (size_t)base + 2u * ((uint32_t)j * kInpNT + t);  // (even: the source side of a pair is aligned)
            k0[j] = k1[j] = n0[j] = n1[j] = 0;
            a0[j] = a1[j] = 0;
            if (pr[j] && (vec & 1u)) {
                const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(c_sub.keys + p0);
                const ulonglong2 y = *reinterpret_cast<const ulonglong2*>(c_sub.counters + p0);
                const uint2 z = *reinterpret_cast<const uint2*>(c_sub.actors + p0);
                k0[j] = x.x;
                k1[j] = x.y;
                n0[j] = y.x;
                n1[j] = y.y;
                a0[j] = z.x;
                a1[j] = z.y;
            } else {
                if (m0[j]) {
                    k0[j] = c_sub.keys[p0];
                    n0[j] = c_sub.counters[p0];
                    a0[j] = c_sub.actors[p0];
                }
                if (m1[j]) {
                    k1[j] = c_sub.keys[p0 + 1];
                    n1[j] = c_sub.counters[p0 + 1];
                    a1[j] = c_sub.actors[p0 + 1];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kInpJ; ++j) {
            if (pr[j] && (vec & 2u) && (d0[j] & 1u) == 0u) {
                *reinterpret_cast<ulonglong2*>(c_rep.keys + d0[j]) = make_ulonglong2(k0[j], k1[j]);
                *reinterpret_cast<ulonglong2*>(c_rep.counters + d0[j]) = make_ulonglong2(n0[j], n1[j]);
                *reinterpret_cast<uint2*>(c_rep.actors + d0[j]) = make_uint2(a0[j], a1[j]);
            } else {
                if (m0[j]) {
                    c_rep.keys[d0[j]] = k0[j];
                    c_rep.counters[d0[j]] = n0[j];
                    c_rep.actors[d0[j]] = a0[j];
                }
                if (m1[j]) {
                    c_rep.keys[d1[j]] = k1[j];
                    c_rep.counters[d1[j]] = n1[j];
                    c_rep.actors[d1[j]] = a1[j];
                }
            }
        }
        __syncthreads();  // (the staged arrays are reused by the next chunk)
    }

    if (KIND == 0) {
        // clocks of the placed documents: n_sub x R words, one lane per word
        const uint32_t R = s.R;
        const uint64_t nw = (uint64_t)n_sub * R;
        for (uint64_t w = (uint64_t)blockIdx.x * kInpNT + t; w < nw; w += (uint64_t)gridDim.x * kInpNT) {
            const uint32_t j = (uint32_t)(w / R);
            const uint32_t r = (uint32_t)(w - (uint64_t)j * R);
            if (s.verdict[j] == kInpPlaced) s.vv[(size_t)s.idx[j] * R + r] = s.sub.vv[w];
        }
    }
}

static bool inp_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// a.n_docs == 0 or a.sub.n_docs == 0: *n_spill = 0 alone is written.
hipError_t launch_replica_inplace(const InplaceArgs& a0, uint32_t* inv, uint32_t* parts, uint32_t* status,
                                  uint32_t n_cu, hipStream_t stream) {
    InplaceArgs a = a0;
    a.inv = inv;
    const uint32_t n_sub = a.n_docs ? a.sub.n_docs : 0u;
    const uint32_t n_parts = (uint32_t)(((uint64_t)n_sub + kInpScanChunk - 1) / kInpScanChunk);
    hipError_t e = hipSuccess;
    if (n_sub) {
        if ((e = launch_replica_map(a.idx, a.n_idx, n_sub, a.n_docs, inv, status, n_cu, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(inplace_verdict_kernel, dim3(n_parts), dim3(kInpNT), 0, stream, a, parts, status);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(inplace_partials_kernel, dim3(1), dim3(kInpPartNT), 0, stream, parts, n_parts, a.n_spill);
    if ((e = hipGetLastError()) != hipSuccess || n_sub == 0) return e;
    hipLaunchKernelGGL(inplace_emit_kernel, dim3(n_parts), dim3(kInpNT), 0, stream, a, parts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const bool vin_e = inp_aligned(a.sub.e.keys, 16) && inp_aligned(a.sub.e.counters, 16) && inp_aligned(a.sub.e.actors, 8);
    const bool vout_e = inp_aligned(a.e.keys, 16) && inp_aligned(a.e.counters, 16) && inp_aligned(a.e.actors, 8);
    hipLaunchKernelGGL(inplace_gather_kernel<0>, dim3(n_cu * 8u), dim3(kInpNT), 0, stream, a,
                       (vin_e ? 1u : 0u) | (vout_e ? 2u : 0u));
    if ((e = hipGetLastError()) != hipSuccess || !a.sub.t.off || !a.t.off) return e;
    const bool vin_t = inp_aligned(a.sub.t.keys, 16) && inp_aligned(a.sub.t.counters, 16) && inp_aligned(a.sub.t.actors, 8);
    const bool vout_t = inp_aligned(a.t.keys, 16) && inp_aligned(a.t.counters, 16) && inp_aligned(a.t.actors, 8);
    hipLaunchKernelGGL(inplace_gather_kernel<1>, dim3(n_cu * 8u), dim3(kInpNT), 0, stream, a,
                       (vin_t ? 1u : 0u) | (vout_t ? 2u : 0u));
    return hipGetLastError();
}

}  // namespace crdt
