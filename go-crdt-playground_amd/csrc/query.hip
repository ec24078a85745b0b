// Batched membership reads (crdt_awset_has_async, crdt_tomb_has_async): the
// reference's one read primitive, (*AWSet).Has(k) (awset.go:87), over
// device-resident states -- and the same lookup over AWSetDelta.Deleted.
//
//   found[i]  = 1 iff query key i is one of the first counts[d] keys of its
//               document's slots (slots past the live count are never read)
//   actors[i], counters[i] = that entry's dot, 0 when absent (optional)
//
// The unit of work is the query, not the document: workgroups of kHasNT
// threads take chunks of kHasChunk = kHasNT x kHasQ consecutive queries,
// grid-stride; thread t of a chunk at `base` takes queries base + j*kHasNT + t,
// so the key loads and the output stores of one j are coalesced.
//
//   query's document   the largest d with q_off[d] <= i.  The workgroup finds
//       the documents of its chunk's first and last query with a uniform
//       search in global q_off; when that span is at most kHasRun documents
//       their q_off, slot offset and live count are staged in LDS and each
//       lane searches there, otherwise (long runs of documents that ask
//       nothing) each lane searches global q_off within the span.
//   key search   a lower bound over the document's live keys in global memory.
//       The kHasQ searches of a lane advance step by step together, so a lane
//       keeps kHasQ independent loads in flight instead of one dependent chain.
//   dot   a hit loads the entry's actor and counter.
//
// One kernel, no workspace: a document with many queries is served by as many
// lanes as it has queries, a large document by log2(n) probes per query.
#include "crdt_device.hpp"

namespace crdt {

constexpr int kHasNT = 256;
constexpr int kHasQ = 4;
constexpr uint32_t kHasChunk = kHasNT * kHasQ;  // 1,024 queries per workgroup step
constexpr uint32_t kHasRun = 256;               // documents staged in LDS at most (one per thread)

// Number of elements of the non-decreasing a[0..n) that are <= x.
__device__ __forceinline__ uint32_t has_count_le(const uint32_t* a, uint32_t n, uint32_t x) {
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

// Slot offset and live count of document d; a count above the slots is clamped
// to them (and flagged), so no probe ever leaves the document's region.
__device__ __forceinline__ void has_doc(const HasView& sv, uint32_t d, uint32_t& o, uint32_t& n, uint32_t& err) {
    const uint32_t b = sv.offsets[d], e = sv.offsets[d + 1];
    const uint32_t slots = e > b ? e - b : 0u;
    const uint32_t live = sv.counts ? sv.counts[d] : slots;
    if (live > slots) err |= kErrCapacity;
    o = b;
    n = min(live, slots);
}

__global__ __launch_bounds__(kHasNT) void has_kernel(HasView sv, HasQueries qv, HasOut out, uint32_t n_chunks,
                                                      uint32_t* status, const uint32_t* gate) {
    __shared__ uint32_t s_qoff[kHasRun];  // q_off of the staged documents
    __shared__ uint32_t s_off[kHasRun];   // slot offset
    __shared__ uint32_t s_cnt[kHasRun];   // live count (clamped)
    if (gate && (*gate & kErrUnsorted) != 0u) return;  // the host path's order check failed (Work::gate)
    const uint32_t t = threadIdx.x;
    const uint32_t nq = qv.n_queries, n_docs = sv.n_docs;
    uint32_t err = 0;

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t base = chunk * kHasChunk;  // (n_chunks = ceil(nq / kHasChunk): base < nq)
        const uint32_t m = min(kHasChunk, nq - base);
        // Documents of the chunk's first and last query.  The search runs over
        // q_off[1 .. n_docs), so whatever q_off holds the answer is a document.
        const uint32_t d_lo = has_count_le(qv.q_off + 1, n_docs - 1, base);
        const uint32_t d_hi = d_lo + has_count_le(qv.q_off + 1 + d_lo, n_docs - 1 - d_lo, base + (m - 1));
        const uint32_t span = d_hi - d_lo + 1;
        const bool staged = span <= kHasRun;
        if (staged) {
            if (t < span) {
                uint32_t o, n;
                has_doc(sv, d_lo + t, o, n, err);
                s_qoff[t] = qv.q_off[d_lo + t];
                s_off[t] = o;
                s_cnt[t] = n;
            }
            __syncthreads();
        }

        uint64_t k[kHasQ];
        uint32_t o[kHasQ], n[kHasQ], lo[kHasQ], hi[kHasQ];
#pragma unroll
        for (int j = 0; j < kHasQ; ++j) {
            const uint32_t rel = (uint32_t)j * kHasNT + t;
            k[j] = 0;
            o[j] = 0;
            n[j] = 0;
            if (rel < m) {
                const uint32_t i = base + rel;
                k[j] = qv.keys[i];
                if (staged) {
                    const uint32_t x = has_count_le(s_qoff + 1, span - 1, i);
                    o[j] = s_off[x];
                    n[j] = s_cnt[x];
                } else {
                    const uint32_t d = d_lo + has_count_le(qv.q_off + 1 + d_lo, span - 1, i);
                    has_doc(sv, d, o[j], n[j], err);
                }
            }
            lo[j] = 0;
            hi[j] = n[j];
        }

        // kHasQ lower bounds in step: every round issues the probes of all
        // unfinished searches before any is compared.
        for (;;) {
            bool any = false;
#pragma unroll
            for (int j = 0; j < kHasQ; ++j) any |= lo[j] < hi[j];
            if (!any) break;
            uint64_t v[kHasQ];
            uint32_t mid[kHasQ];
#pragma unroll
            for (int j = 0; j < kHasQ; ++j) {
                mid[j] = (lo[j] + hi[j]) >> 1;
                v[j] = lo[j] < hi[j] ? sv.keys[(size_t)o[j] + mid[j]] : 0ull;
            }
#pragma unroll
            for (int j = 0; j < kHasQ; ++j) {
                if (lo[j] < hi[j]) {
                    if (v[j] < k[j])
                        lo[j] = mid[j] + 1;
                    else
                        hi[j] = mid[j];
                }
            }
        }

        // lo = live keys below the query key: a hit iff the key there equals it
        uint64_t hk[kHasQ];
#pragma unroll
        for (int j = 0; j < kHasQ; ++j) hk[j] = lo[j] < n[j] ? sv.keys[(size_t)o[j] + lo[j]] : 0ull;
        bool hit[kHasQ];
#pragma unroll
        for (int j = 0; j < kHasQ; ++j) hit[j] = lo[j] < n[j] && hk[j] == k[j];
        if (out.actors) {
            uint32_t a[kHasQ];
            uint64_t c[kHasQ];
#pragma unroll
            for (int j = 0; j < kHasQ; ++j) {
                a[j] = hit[j] ? sv.actors[(size_t)o[j] + lo[j]] : 0u;
                c[j] = hit[j] ? sv.counters[(size_t)o[j] + lo[j]] : 0ull;
            }
#pragma unroll
            for (int j = 0; j < kHasQ; ++j) {
                const uint32_t rel = (uint32_t)j * kHasNT + t;
                if (rel < m) {
                    out.actors[(size_t)base + rel] = a[j];
                    out.counters[(size_t)base + rel] = c[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kHasQ; ++j) {
            const uint32_t rel = (uint32_t)j * kHasNT + t;
            if (rel < m) out.found[(size_t)base + rel] = hit[j] ? (uint8_t)1 : (uint8_t)0;
        }
        __syncthreads();  // (the staged arrays are reused by the next chunk)
    }
    flag_error(status, err);
}

// n_docs >= 1 and n_queries >= 1 (the caller launches nothing otherwise).
hipError_t launch_has(const HasView& sv, const HasQueries& qv, const HasOut& out, uint32_t* status,
                      const uint32_t* gate, uint32_t n_cu, hipStream_t stream) {
    const uint32_t n_chunks = (uint32_t)(((uint64_t)qv.n_queries + kHasChunk - 1) / kHasChunk);
    const uint32_t grid = min(n_chunks, n_cu * 8u);
    hipLaunchKernelGGL(has_kernel, dim3(grid), dim3(kHasNT), 0, stream, sv, qv, out, n_chunks, status, gate);
    return hipGetLastError();
}

}  // namespace crdt
