// Scatter: a merged sub-batch put back into the resident batch it was selected
// from (crdt_awset_scatter_async; include/crdtgpu.h).  Output document d is the
// live entries, count and clock of sub document j when idx[j] == d for some
// j < *n_idx, and of state document d otherwise, packed with no slack: the
// inverse of crdt_awset_select_async, and with *n_idx == 0 its identity form.
// A replacement may be longer, shorter or empty, so every later offset moves.
// Six launches, ordered by their kernel boundaries alone:
//
//   scatter_fill_kernel      inv[d] = kSctNone ("not replaced") for every state document.
//   scatter_map_kernel       one thread per j < *n_idx: atomicMin(inv[idx[j]], j).
//       The lowest j naming a document supplies it, so the result is the same on
//       every run; a value returned that is not the sentinel is a duplicate, an
//       idx[j] that is no document is skipped: both kErrIndex.
//   scatter_count_kernel     the offsets' scan, step 1: the state's documents are
//       cut into chunks of kSctScanChunk; workgroup c sums the live count (clamped
//       to the slots, kErrCapacity) of the chosen source over chunk c into
//       parts[c], saturating at 2^32 - 1 (such a chunk alone exceeds any out_slots
//       and is reported here).
//   scatter_partials_kernel  step 2, one workgroup: parts[c] becomes its exclusive
//       prefix, kSctPartStep partials per step; the running total is kept in 64
//       bits for the check against out_slots, and offsets[n_docs] is written.
//   scatter_emit_kernel      step 3: workgroup c rescans its chunk
//       (block_exclusive_scan) on top of parts[c] and writes out.counts and
//       out.offsets.
//       No workgroup of any step waits for a word another workgroup of the same
//       launch writes: no look-back, no polling.
//   scatter_gather_kernel    the shape of select_gather_kernel (compare.hip): the
//       OUTPUT positions are cut into chunks of kSctGatherChunk, grid-stride; the
//       documents of a chunk are found through out.offsets and staged in LDS (at
//       most kSctRun of them: beyond, lanes search out.offsets in global memory)
//       with the side and slot offset of their source, taken from inv.  A lane
//       takes kSctJ pairs of neighbouring positions; a pair that lies in one
//       document at an even source index is read with 16 B loads (keys,
//       counters; 8 B actors), any other element by element; all loads of a lane
//       are issued before its first store, and the stores of a pair are 16 B (the
//       output side of a pair is always aligned).  Then the clocks, one lane per
//       actor, from whichever side supplies the document.
//
// Workspace: inv, one word per state document, and parts, one word per chunk.
#include "crdt_device.hpp"
#include "merge_block.hpp"

namespace crdt {

constexpr int kSctNT = 256;
constexpr int kSctV = 4;                                 // documents per lane and scan chunk
constexpr uint32_t kSctScanChunk = kSctNT * kSctV;       // 1,024 documents per scan workgroup
constexpr int kSctPartNT = 1024;
constexpr uint32_t kSctPartStep = kSctPartNT;            // partials one step of the partials scan holds
constexpr int kSctJ = 4;                                 // pairs of positions per lane and gather chunk
constexpr uint32_t kSctGatherChunk = kSctNT * kSctJ * 2; // 2,048 output positions per gather step
constexpr uint32_t kSctRun = 1024;                       // documents staged in LDS at most
constexpr uint32_t kSctNone = 0xFFFFFFFFu;               // inv: the state's own document

struct ScatterArgs {
    BatchView st, sub;
    const uint32_t* idx;    // [sub.n_docs]
    const uint32_t* n_idx;  // NULL: sub.n_docs
    uint32_t out_slots;
    OutView out;
};

// Number of elements of the non-decreasing a[0..n) that are <= x.
__device__ __forceinline__ uint32_t sct_count_le(const uint32_t* a, uint32_t n, uint32_t x) {
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

// The source of output document d: sub document j = inv[d], or the state's own
// (j == kSctNone); its slot offset and clamped live count.
__device__ __forceinline__ void sct_doc(const ScatterArgs& s, const uint32_t* inv, uint32_t d, uint32_t& j,
                                        uint32_t& o, uint32_t& n, uint32_t& err) {
    j = inv[d];
    if (j < s.sub.n_docs) {  // (inv holds only j < *n_idx <= sub.n_docs, or the sentinel)
        n = live_span(s.sub.offsets, s.sub.counts, j, o, err);
    } else {
        j = kSctNone;
        n = live_span(s.st.offsets, s.st.counts, d, o, err);
    }
}

__global__ __launch_bounds__(kSctNT) void scatter_fill_kernel(uint32_t* inv, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * kSctNT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSctNT)
        inv[i] = kSctNone;
}

__global__ __launch_bounds__(kSctNT) void scatter_map_kernel(ScatterArgs s, uint32_t* inv, uint32_t* status) {
    uint32_t err = 0;
    uint32_t n_idx = s.n_idx ? *s.n_idx : s.sub.n_docs;
    if (n_idx > s.sub.n_docs) {
        err |= kErrCapacity;
        n_idx = s.sub.n_docs;
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kSctNT + threadIdx.x; i < n_idx; i += (uint64_t)gridDim.x * kSctNT) {
        const uint32_t j = (uint32_t)i;
        const uint32_t d = s.idx[j];
        if (d >= s.st.n_docs)
            err |= kErrIndex;  // no document of the state: this sub document is ignored
        else if (atomicMin(&inv[d], j) != kSctNone)
            err |= kErrIndex;  // named twice: the lowest j stays
    }
    flag_error(status, err);
}

__global__ __launch_bounds__(kSctNT) void scatter_count_kernel(ScatterArgs s, const uint32_t* inv, uint32_t* parts,
                                                               uint32_t* status) {
    __shared__ unsigned long long s_sum;
    const uint32_t t = threadIdx.x, n = s.st.n_docs;
    const uint32_t base = blockIdx.x * kSctScanChunk;  // (< n: the grid is the number of chunks)
    const uint32_t m = min(kSctScanChunk, n - base);
    if (t == 0) s_sum = 0;
    __syncthreads();
    uint32_t err = 0;
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < kSctV; ++k) {
        const uint32_t i = (uint32_t)k * kSctNT + t;
        if (i < m) {
            uint32_t j, o, c;
            sct_doc(s, inv, base + i, j, o, c, err);
            mine += c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((t & 63) == 0 && mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (t == 0) {
        const unsigned long long sum = s_sum;
        if (sum > (unsigned long long)s.out_slots) err |= kErrCapacity;
        parts[blockIdx.x] = sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum;
    }
    flag_error(status, err);
}

// One workgroup: parts[0..n_parts) -> exclusive prefixes (u32, as the offsets
// are), the total into *total_out, checked in 64 bits against out_slots.
__global__ __launch_bounds__(kSctPartNT) void scatter_partials_kernel(uint32_t* parts, uint32_t n_parts,
                                                                      uint32_t out_slots, uint32_t* total_out,
                                                                      uint32_t* status) {
    __shared__ uint32_t wave_tot[kSctPartNT / 64];
    __shared__ unsigned long long s_total;
    const uint32_t t = threadIdx.x;
    if (t == 0) s_total = 0;
    unsigned long long mine = 0;  // (the u32 prefix may wrap on an output that cannot fit: detected here)
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_parts; base += kSctPartStep) {
        const bool in = t < n_parts - base;
        const uint32_t v = in ? parts[base + t] : 0u;
        mine += v;
        uint32_t tot = 0;
        const uint32_t p = carry + block_exclusive_scan<kSctPartNT>(v, wave_tot, &tot);
        if (in) parts[base + t] = p;
        carry += tot;
    }
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((t & 63) == 0 && mine) atomicAdd(&s_total, mine);
    __syncthreads();
    uint32_t err = 0;
    if (t == 0) {
        *total_out = carry;
        if (s_total > (unsigned long long)out_slots) err |= kErrCapacity;
    }
    flag_error(status, err);
}

__global__ __launch_bounds__(kSctNT) void scatter_emit_kernel(ScatterArgs s, const uint32_t* inv,
                                                              const uint32_t* parts) {
    __shared__ uint32_t wave_tot[kSctNT / 64];
    __shared__ uint32_t run[kSctScanChunk];
    const uint32_t t = threadIdx.x, n = s.st.n_docs;
    const uint32_t base = blockIdx.x * kSctScanChunk;
    const uint32_t m = min(kSctScanChunk, n - base);
    uint32_t err = 0;  // (reported by scatter_count_kernel)
#pragma unroll
    for (int k = 0; k < kSctV; ++k) {
        const uint32_t i = (uint32_t)k * kSctNT + t;
        uint32_t c = 0;
        if (i < m) {
            uint32_t j, o;
            sct_doc(s, inv, base + i, j, o, c, err);
            s.out.counts[base + i] = c;
        }
        run[i] = c;
    }
    __syncthreads();
    uint32_t v[kSctV], sum = 0;
#pragma unroll
    for (int k = 0; k < kSctV; ++k) {
        v[k] = run[t * kSctV + k];
        sum += v[k];
    }
    uint32_t tot = 0;
    uint32_t p = parts[blockIdx.x] + block_exclusive_scan<kSctNT>(sum, wave_tot, &tot);
#pragma unroll
    for (int k = 0; k < kSctV; ++k) {
        run[t * kSctV + k] = p;
        p += v[k];
    }
    __syncthreads();
    for (uint32_t i = t; i < m; i += kSctNT) s.out.offsets[base + i] = run[i];
}

__global__ __launch_bounds__(kSctNT) void scatter_gather_kernel(ScatterArgs s, const uint32_t* inv, uint32_t vec) {
    __shared__ uint32_t s_oo[kSctRun];  // output offset of the staged documents
    __shared__ uint32_t s_so[kSctRun];  // offset of the source document each copies
    __shared__ uint32_t s_n[kSctRun];   // live count
    __shared__ uint32_t s_sd[kSctRun];  // 1: the source is the sub-batch
    const uint32_t t = threadIdx.x, n_docs = s.st.n_docs;
    const uint32_t* ooff = s.out.offsets;
    // nothing is written at or past out_slots, whatever the scan found
    const uint32_t total = min(ooff[n_docs], s.out_slots);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)total + kSctGatherChunk - 1) / kSctGatherChunk);

    auto doc = [&](uint32_t d, uint32_t& oo, uint32_t& so, uint32_t& n, uint32_t& sd) {
        oo = ooff[d];
        n = s.out.counts[d];  // (clamped to the source's slots by scatter_emit_kernel)
        const uint32_t j = inv[d];
        sd = j < s.sub.n_docs ? 1u : 0u;
        so = sd ? s.sub.offsets[j] : s.st.offsets[d];
    };

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t base = chunk * kSctGatherChunk;
        const uint32_t m = min(kSctGatherChunk, total - base);
        // Documents of the chunk's first and last position.  The search runs over
        // offsets[1 .. n_docs), so whatever the offsets hold the answer is a document.
        const uint32_t d_lo = sct_count_le(ooff + 1, n_docs - 1, base);
        const uint32_t d_hi = d_lo + sct_count_le(ooff + 1 + d_lo, n_docs - 1 - d_lo, base + (m - 1));
        const uint32_t span = d_hi - d_lo + 1;
        const bool staged = span <= kSctRun;
        if (staged) {
            for (uint32_t x = t; x < span; x += kSctNT) {
                uint32_t oo, so, n, sd;
                doc(d_lo + x, oo, so, n, sd);
                s_oo[x] = oo;
                s_so[x] = so;
                s_n[x] = n;
                s_sd[x] = sd;
            }
            __syncthreads();
        }
        // position p of the output: (copied, index in its source, the source's side,
        // entries left in its document)
        auto locate = [&](uint32_t p, uint32_t& src, uint32_t& sd, uint32_t& left) {
            uint32_t oo, so, n;
            if (staged) {
                const uint32_t x = sct_count_le(s_oo + 1, span - 1, p);
                oo = s_oo[x];
                so = s_so[x];
                n = s_n[x];
                sd = s_sd[x];
            } else {
                doc(d_lo + sct_count_le(ooff + 1 + d_lo, span - 1, p), oo, so, n, sd);
            }
            const uint32_t i = p - oo;  // (below the document: wraps, never < n)
            src = so + i;
            left = i < n ? n - i : 0u;
            return i < n;
        };

        uint32_t c0[kSctJ], c1[kSctJ], e0[kSctJ], e1[kSctJ];
        bool m0[kSctJ], m1[kSctJ], v[kSctJ];
#pragma unroll
        for (int j = 0; j < kSctJ; ++j) {
            const uint32_t rel = 2u * ((uint32_t)j * kSctNT + t);
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
        uint64_t k0[kSctJ], k1[kSctJ], n0[kSctJ], n1[kSctJ];
        uint32_t a0[kSctJ], a1[kSctJ];
#pragma unroll
        for (int j = 0; j < kSctJ; ++j) {
            k0[j] = k1[j] = n0[j] = n1[j] = 0;
            a0[j] = a1[j] = 0;
            const BatchView& b0 = e0[j] ? s.sub : s.st;
            const BatchView& b1 = e1[j] ? s.sub : s.st;
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
        for (int j = 0; j < kSctJ; ++j) {
            const size_t p0 = (size_t)base + 2u * ((uint32_t)j * kSctNT + t);
            if (m0[j] && m1[j]) {  // (p0 is even: the output side of a pair is always aligned)
                if (vec & 2u) {
                    *reinterpret_cast<ulonglong2*>(s.out.keys + p0) = make_ulonglong2(k0[j], k1[j]);
                    *reinterpret_cast<ulonglong2*>(s.out.counters + p0) = make_ulonglong2(n0[j], n1[j]);
                    *reinterpret_cast<uint2*>(s.out.actors + p0) = make_uint2(a0[j], a1[j]);
                } else {
                    s.out.keys[p0] = k0[j];
                    s.out.counters[p0] = n0[j];
                    s.out.actors[p0] = a0[j];
                    s.out.keys[p0 + 1] = k1[j];
                    s.out.counters[p0 + 1] = n1[j];
                    s.out.actors[p0 + 1] = a1[j];
                }
            } else {
                if (m0[j]) {
                    s.out.keys[p0] = k0[j];
                    s.out.counters[p0] = n0[j];
                    s.out.actors[p0] = a0[j];
                }
                if (m1[j]) {
                    s.out.keys[p0 + 1] = k1[j];
                    s.out.counters[p0 + 1] = n1[j];
                    s.out.actors[p0 + 1] = a1[j];
                }
            }
        }
        __syncthreads();  // (the staged arrays are reused by the next chunk)
    }

    // clocks: n_docs x R words, one lane per actor, from the side that supplies the document
    const uint32_t R = s.st.R;
    const uint64_t nw = (uint64_t)n_docs * R;
    for (uint64_t w = (uint64_t)blockIdx.x * kSctNT + t; w < nw; w += (uint64_t)gridDim.x * kSctNT) {
        const uint32_t d = (uint32_t)(w / R);
        const uint32_t r = (uint32_t)(w - (uint64_t)d * R);
        const uint32_t j = inv[d];
        s.out.vv[w] = j < s.sub.n_docs ? s.sub.vv[(size_t)j * R + r] : s.st.vv[w];
    }
}

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// inv: n_docs workspace words, parts: one per kSctScanChunk documents.
// n_docs == 0: only offsets[0] = 0 is written.
hipError_t launch_scatter(const BatchView& st, const BatchView& sub, const uint32_t* idx, const uint32_t* n_idx,
                          uint32_t out_slots, const OutView& out, uint32_t* inv, uint32_t* parts, uint32_t* status,
                          uint32_t n_cu, hipStream_t stream) {
    const ScatterArgs s{st, sub, idx, n_idx, out_slots, out};
    const uint32_t n = st.n_docs;
    const uint32_t n_parts = (uint32_t)(((uint64_t)n + kSctScanChunk - 1) / kSctScanChunk);
    hipError_t e = hipSuccess;
    if (n) {
        const uint32_t fgrid = min((n + (uint32_t)kSctNT - 1u) / (uint32_t)kSctNT, n_cu * 8u);
        hipLaunchKernelGGL(scatter_fill_kernel, dim3(fgrid), dim3(kSctNT), 0, stream, inv, n);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        const uint32_t mgrid =
            max(1u, min((uint32_t)(((uint64_t)sub.n_docs + kSctNT - 1) / kSctNT), n_cu * 8u));
        hipLaunchKernelGGL(scatter_map_kernel, dim3(mgrid), dim3(kSctNT), 0, stream, s, inv, status);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(scatter_count_kernel, dim3(n_parts), dim3(kSctNT), 0, stream, s, inv, parts, status);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(scatter_partials_kernel, dim3(1), dim3(kSctPartNT), 0, stream, parts, n_parts, out_slots,
                       out.offsets + n, status);
    if ((e = hipGetLastError()) != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(scatter_emit_kernel, dim3(n_parts), dim3(kSctNT), 0, stream, s, inv, parts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // bit 0: both sources' columns allow 16 B loads; bit 1: the output's allow 16 B stores
    const bool vin = aligned(st.keys, 16) && aligned(st.counters, 16) && aligned(st.actors, 8) &&
                     aligned(sub.keys, 16) && aligned(sub.counters, 16) && aligned(sub.actors, 8);
    const bool vout = aligned(out.keys, 16) && aligned(out.counters, 16) && aligned(out.actors, 8);
    const uint32_t vec = (vin ? 1u : 0u) | (vout ? 2u : 0u);
    hipLaunchKernelGGL(scatter_gather_kernel, dim3(n_cu * 8u), dim3(kSctNT), 0, stream, s, inv, vec);
    return hipGetLastError();
}

}  // namespace crdt
