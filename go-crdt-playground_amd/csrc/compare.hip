// Convergence check and sub-batch selection on device-resident batches
// (crdt_awset_compare_async, crdt_awset_select_async; include/crdtgpu.h).
//
// compare: per document, CRDT_CMP_* bits of a[d] against b[d].  The reference's
// tests end on assertEntries(A, ..) / assertEntries(B, ..), a comparison of the
// replicas' sorted values; keys are strictly ascending here, so the element
// sets are equal iff the live counts are equal and the keys are equal position
// by position -- no merge walk.  Three launches:
//
//   compare_docs_kernel      one thread per document: the two live counts
//       (clamped to the slots, kErrCapacity) -> fw[d] = KEYS when they differ,
//       else 0.  This store is what zeroes the call's flag words.
//   compare_kernel           the unit of work is the slot, not the document: a's
//       slot space [0, a.offsets[n_docs]) is cut into chunks of kCmpChunk
//       positions, grid-stride; a lane takes kCmpJ pairs of neighbouring
//       positions.  The chunk finds the documents of its first and last position
//       with a uniform search in a.offsets, stages those documents' a offset, b
//       offset and common live count (0 when the counts differ: nothing of such
//       a document is read) in LDS when they are at most kCmpRun, and each lane
//       finds its position's document there; wider spans (many empty or
//       one-entry documents) search a.offsets in global memory.  A pair that
//       lies in one document at an even b index is read with 16 B loads (keys,
//       counters; 8 B actors), any other element by element; all key loads of a
//       lane are issued before the first compare, then the dot loads of the
//       positions whose keys matched.  Difference bits are ORed over the lanes
//       of a wave that hold the same document (they are neighbours) and the
//       first of them issues one atomicOr into fw[d].  Then the same kernel
//       walks the n_docs x R clock words of both sides, one lane per actor.
//   compare_worklist_kernel  one workgroup, the shape of pack_scan_kernel:
//       flags[d] = fw[d] with DOTS cleared under KEYS, the five summary counts,
//       and the ascending list of documents with flags & mask: count, scan,
//       emit -- the same list on every run.
//
// select: out document j = the live entries, count and clock of state document
// idx[j], packed with no slack.  select_scan_kernel (one workgroup) writes the
// counts and their exclusive prefix into out.offsets; select_gather_kernel is
// partitioned over OUTPUT positions in chunks of kSelChunk, found through
// out.offsets the way compare_kernel finds its documents, so a 10^6-entry
// document is copied by many workgroups and 10^6 one-entry documents by few;
// then the clocks, one lane per actor.  No workspace.
#include "crdt_device.hpp"
#include "merge_block.hpp"

namespace crdt {

constexpr int kCmpNT = 256;
constexpr int kCmpJ = 4;                               // pairs of positions per lane and chunk
constexpr uint32_t kCmpChunk = kCmpNT * kCmpJ * 2;     // 2,048 slot positions per workgroup step
constexpr uint32_t kCmpRun = 1024;                     // documents staged in LDS at most
constexpr uint32_t kCmpVvChunk = kCmpNT * kCmpJ;       // 1,024 clock words per workgroup step
constexpr uint32_t kSelChunk = kCmpChunk;              // output positions per gather step
constexpr uint32_t kSelRun = kCmpRun;
constexpr int kScanNT = 1024;                          // the single-workgroup scans
constexpr int kScanV = 8;
constexpr uint32_t kScanChunk = kScanNT * kScanV;      // 8,192 documents per scan step
constexpr uint32_t kNoDoc = 0xFFFFFFFFu;

// Number of elements of the non-decreasing a[0..n) that are <= x.
__device__ __forceinline__ uint32_t cmp_count_le(const uint32_t* a, uint32_t n, uint32_t x) {
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

// Document d of both sides: offsets, and the live count they share (0 when they differ).
__device__ __forceinline__ void cmp_doc(const BatchView& a, const BatchView& b, uint32_t d, uint32_t& ao, uint32_t& bo,
                                        uint32_t& n) {
    uint32_t na, nb, err = 0;
    na = live_span(a.offsets, a.counts, d, ao, err);
    nb = live_span(b.offsets, b.counts, d, bo, err);
    n = na == nb ? na : 0u;
}

// Every lane of the wave holds (d, bits); lanes with the same d are neighbours.
// The first lane of each run ORs the run's bits into fw[d] (d == kNoDoc: none).
__device__ __forceinline__ void seg_or(uint32_t* fw, uint32_t d, uint32_t bits) {
    const uint32_t lane = lane_id();
    const uint32_t prev = __shfl_up(d, 1);
    const bool head = lane == 0 || prev != d;
    const uint64_t heads = ballot(head);
    const uint64_t above = heads & ~low_mask(lane + 1);
    const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : 64u;
    const uint64_t seg = low_mask(end) & ~low_mask(lane);
    uint32_t r = 0;
#pragma unroll
    for (uint32_t bit = 1; bit <= 8; bit <<= 1)
        if (ballot((bits & bit) != 0) & seg) r |= bit;
    if (head && r && d != kNoDoc) atomicOr(&fw[d], r);
}

__global__ __launch_bounds__(256) void compare_docs_kernel(BatchView a, BatchView b, uint32_t* fw, uint32_t* status,
                                                           const uint32_t* gate) {
    if (gate && (*gate & kErrUnsorted) != 0u) return;  // the host path's order check failed (Work::gate)
    uint32_t err = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.n_docs; i += (uint64_t)gridDim.x * 256) {
        const uint32_t d = (uint32_t)i;
        uint32_t ao, bo, na, nb;
        na = live_span(a.offsets, a.counts, d, ao, err);
        nb = live_span(b.offsets, b.counts, d, bo, err);
        fw[d] = na != nb ? CRDT_CMP_KEYS : 0u;
    }
    flag_error(status, err);
}

// One position of a's slot space: its document, whether it is a live entry of a
// document whose counts agree, and the entry's index in b.
struct CmpPos {
    uint32_t d, q, i, n;
    bool live;
};

__global__ __launch_bounds__(kCmpNT) void compare_kernel(BatchView a, BatchView b, uint32_t* fw, uint32_t vec,
                                                         const uint32_t* gate) {
    __shared__ uint32_t s_ao[kCmpRun];  // a offset of the staged documents
    __shared__ uint32_t s_bo[kCmpRun];  // b offset
    __shared__ uint32_t s_n[kCmpRun];   // common live count, 0 when the counts differ
    if (gate && (*gate & kErrUnsorted) != 0u) return;
    const uint32_t t = threadIdx.x;
    const uint32_t n_docs = a.n_docs;
    const uint32_t total = a.offsets[n_docs];
    const uint32_t n_chunks = (uint32_t)(((uint64_t)total + kCmpChunk - 1) / kCmpChunk);

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t base = chunk * kCmpChunk;  // (base < total)
        const uint32_t m = min(kCmpChunk, total - base);
        // Documents of the chunk's first and last position.  The search runs over
        // offsets[1 .. n_docs), so whatever the offsets hold the answer is a document.
        const uint32_t d_lo = cmp_count_le(a.offsets + 1, n_docs - 1, base);
        const uint32_t d_hi = d_lo + cmp_count_le(a.offsets + 1 + d_lo, n_docs - 1 - d_lo, base + (m - 1));
        const uint32_t span = d_hi - d_lo + 1;
        const bool staged = span <= kCmpRun;
        if (staged) {
            for (uint32_t x = t; x < span; x += kCmpNT) {
                uint32_t ao, bo, n;
                cmp_doc(a, b, d_lo + x, ao, bo, n);
                s_ao[x] = ao;
                s_bo[x] = bo;
                s_n[x] = n;
            }
            __syncthreads();
        }
        auto locate = [&](uint32_t p) {
            CmpPos r;
            uint32_t ao, bo;
            if (staged) {
                const uint32_t x = cmp_count_le(s_ao + 1, span - 1, p);
                ao = s_ao[x];
                bo = s_bo[x];
                r.n = s_n[x];
                r.d = d_lo + x;
            } else {
                r.d = d_lo + cmp_count_le(a.offsets + 1 + d_lo, span - 1, p);
                cmp_doc(a, b, r.d, ao, bo, r.n);
            }
            r.i = p - ao;  // (below the document: wraps, never < n)
            r.live = r.i < r.n;
            r.q = bo + r.i;
            return r;
        };

        uint32_t q0[kCmpJ], q1[kCmpJ], d0[kCmpJ], d1[kCmpJ];
        bool m0[kCmpJ], m1[kCmpJ], v[kCmpJ];
#pragma unroll
        for (int j = 0; j < kCmpJ; ++j) {
            const uint32_t rel = 2u * ((uint32_t)j * kCmpNT + t);
            q0[j] = q1[j] = 0;
            d0[j] = d1[j] = kNoDoc;
            m0[j] = m1[j] = false;
            if (rel < m) {
                const CmpPos e0 = locate(base + rel);
                d0[j] = e0.d;
                q0[j] = e0.q;
                m0[j] = e0.live;
                if (e0.live && e0.i + 1 < e0.n) {  // the neighbour is the same document's next entry
                    d1[j] = e0.d;
                    q1[j] = e0.q + 1;
                    m1[j] = true;
                } else if (rel + 1 < m) {
                    const CmpPos e1 = locate(base + rel + 1);
                    d1[j] = e1.d;
                    q1[j] = e1.q;
                    m1[j] = e1.live;
                }
            }
            v[j] = vec && m0[j] && m1[j] && d1[j] == d0[j] && (q0[j] & 1u) == 0u;
        }

        // keys: every load of the lane before the first compare
        uint64_t ak0[kCmpJ], ak1[kCmpJ], bk0[kCmpJ], bk1[kCmpJ];
#pragma unroll
        for (int j = 0; j < kCmpJ; ++j) {
            const size_t p0 = (size_t)base + 2u * ((uint32_t)j * kCmpNT + t);
            ak0[j] = ak1[j] = bk0[j] = bk1[j] = 0;
            if (v[j]) {
                const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(a.keys + p0);
                const ulonglong2 y = *reinterpret_cast<const ulonglong2*>(b.keys + q0[j]);
                ak0[j] = x.x;
                ak1[j] = x.y;
                bk0[j] = y.x;
                bk1[j] = y.y;
            } else {
                if (m0[j]) {
                    ak0[j] = a.keys[p0];
                    bk0[j] = b.keys[q0[j]];
                }
                if (m1[j]) {
                    ak1[j] = a.keys[p0 + 1];
                    bk1[j] = b.keys[q1[j]];
                }
            }
        }
        bool kd0[kCmpJ], kd1[kCmpJ];
#pragma unroll
        for (int j = 0; j < kCmpJ; ++j) {
            kd0[j] = m0[j] && ak0[j] != bk0[j];
            kd1[j] = m1[j] && ak1[j] != bk1[j];
        }

        // dots of the positions whose keys matched
        uint32_t aa0[kCmpJ], aa1[kCmpJ], ba0[kCmpJ], ba1[kCmpJ];
        uint64_t ac0[kCmpJ], ac1[kCmpJ], bc0[kCmpJ], bc1[kCmpJ];
#pragma unroll
        for (int j = 0; j < kCmpJ; ++j) {
            const size_t p0 = (size_t)base + 2u * ((uint32_t)j * kCmpNT + t);
            const bool n0 = m0[j] && !kd0[j], n1 = m1[j] && !kd1[j];
            aa0[j] = aa1[j] = ba0[j] = ba1[j] = 0;
            ac0[j] = ac1[j] = bc0[j] = bc1[j] = 0;
            if (v[j] && n0 && n1) {
                const uint2 xa = *reinterpret_cast<const uint2*>(a.actors + p0);
                const uint2 ya = *reinterpret_cast<const uint2*>(b.actors + q0[j]);
                const ulonglong2 xc = *reinterpret_cast<const ulonglong2*>(a.counters + p0);
                const ulonglong2 yc = *reinterpret_cast<const ulonglong2*>(b.counters + q0[j]);
                aa0[j] = xa.x;
                aa1[j] = xa.y;
                ba0[j] = ya.x;
                ba1[j] = ya.y;
                ac0[j] = xc.x;
                ac1[j] = xc.y;
                bc0[j] = yc.x;
                bc1[j] = yc.y;
            } else {
                if (n0) {
                    aa0[j] = a.actors[p0];
                    ba0[j] = b.actors[q0[j]];
                    ac0[j] = a.counters[p0];
                    bc0[j] = b.counters[q0[j]];
                }
                if (n1) {
                    aa1[j] = a.actors[p0 + 1];
                    ba1[j] = b.actors[q1[j]];
                    ac1[j] = a.counters[p0 + 1];
                    bc1[j] = b.counters[q1[j]];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kCmpJ; ++j) {
            // (a position not read holds zeros on both sides: no difference)
            const uint32_t f0 = kd0[j] ? CRDT_CMP_KEYS : ((aa0[j] != ba0[j] || ac0[j] != bc0[j]) ? CRDT_CMP_DOTS : 0u);
            const uint32_t f1 = kd1[j] ? CRDT_CMP_KEYS : ((aa1[j] != ba1[j] || ac1[j] != bc1[j]) ? CRDT_CMP_DOTS : 0u);
            const bool same = d1[j] == d0[j];
            seg_or(fw, d0[j], f0 | (same ? f1 : 0u));
            if (!same && f1) atomicOr(&fw[d1[j]], f1);  // (f1 != 0: d1 is a document)
        }
        __syncthreads();  // (the staged arrays are reused by the next chunk)
    }

    // clocks: the n_docs x R words of both sides, one lane per actor
    const uint32_t R = a.R;
    const uint64_t nw = (uint64_t)n_docs * R;
    const uint64_t n_vc = (nw + kCmpVvChunk - 1) / kCmpVvChunk;
    for (uint64_t c = blockIdx.x; c < n_vc; c += gridDim.x) {
        uint64_t av[kCmpJ], bv[kCmpJ];
#pragma unroll
        for (int j = 0; j < kCmpJ; ++j) {
            const uint64_t w = c * kCmpVvChunk + (uint32_t)j * kCmpNT + t;
            av[j] = w < nw ? a.vv[w] : 0ull;
            bv[j] = w < nw ? b.vv[w] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < kCmpJ; ++j) {
            const uint64_t w = c * kCmpVvChunk + (uint32_t)j * kCmpNT + t;
            const uint32_t d = w < nw ? (uint32_t)(w / R) : kNoDoc;
            seg_or(fw, d, (av[j] > bv[j] ? CRDT_CMP_A_AHEAD : 0u) | (bv[j] > av[j] ? CRDT_CMP_B_AHEAD : 0u));
        }
    }
}

// One workgroup, in chunks of kScanChunk documents (pack.hip, pack_scan_kernel):
// the final flags, the summary and the ascending worklist.
__global__ __launch_bounds__(kScanNT) void compare_worklist_kernel(const uint32_t* fw, uint32_t n, uint32_t mask,
                                                                   CompareOutView out, const uint32_t* gate) {
    __shared__ uint32_t wave_tot[kScanNT / 64];
    __shared__ uint32_t run[kScanChunk];
    __shared__ uint32_t s_sum[5];
    if (gate && (*gate & kErrUnsorted) != 0u) return;
    const uint32_t t = threadIdx.x;
    if (t < 5) s_sum[t] = 0;
    uint32_t cnt[5] = {0, 0, 0, 0, 0};
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += kScanChunk) {
        const uint32_t m = min(kScanChunk, n - base);
        for (uint32_t i = t; i < kScanChunk; i += kScanNT) {
            uint32_t f = 0;
            if (i < m) {
                f = fw[base + i] & 15u;
                if (f & CRDT_CMP_KEYS) f &= ~CRDT_CMP_DOTS;  // DOTS is defined under equal element sets only
                out.flags[base + i] = (uint8_t)f;
#pragma unroll
                for (int k = 0; k < 4; ++k) cnt[k] += (f >> k) & 1u;
                cnt[4] += (f & mask) != 0u ? 1u : 0u;
            }
            run[i] = (f & mask) != 0u ? 1u : 0u;
        }
        __syncthreads();
        uint32_t v[kScanV], sum = 0;
#pragma unroll
        for (int j = 0; j < kScanV; ++j) {
            v[j] = run[t * kScanV + j];
            sum += v[j];
        }
        uint32_t tot = 0;
        uint32_t p = carry + block_exclusive_scan<kScanNT>(sum, wave_tot, &tot);
        if (out.worklist) {
#pragma unroll
            for (int j = 0; j < kScanV; ++j)
                if (v[j]) out.worklist[p++] = base + t * kScanV + j;
        }
        carry += tot;
        __syncthreads();  // (run and wave_tot are reused by the next chunk)
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        uint32_t x = cnt[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o);
        if ((t & 63) == 0 && x) atomicAdd(&s_sum[k], x);
    }
    __syncthreads();
    if (out.summary && t < 5) out.summary[t] = s_sum[t];
    if (out.n_work && t == 0) *out.n_work = carry;
}

// ---- select -----------------------------------------------------------------

struct SelectArgs {
    BatchView st;
    const uint32_t* idx;    // NULL: the identity
    const uint32_t* n_idx;  // NULL: n_out
    uint32_t n_out, out_slots;
    OutView out;
};

// Documents selected (the rest of the n_out come out empty).
__device__ __forceinline__ uint32_t sel_n_idx(const SelectArgs& s, uint32_t& err) {
    uint32_t n = s.n_idx ? *s.n_idx : s.n_out;
    if (n > s.n_out) {
        err |= kErrCapacity;
        n = s.n_out;
    }
    return n;
}

// The state document output document j copies, kNoDoc for an empty one.
__device__ __forceinline__ uint32_t sel_src(const SelectArgs& s, uint32_t j, uint32_t n_idx, uint32_t& err) {
    if (j >= n_idx) return kNoDoc;
    const uint32_t d = s.idx ? s.idx[j] : j;
    if (d >= s.st.n_docs) {
        err |= kErrIndex;
        return kNoDoc;
    }
    return d;
}

__global__ __launch_bounds__(kScanNT) void select_scan_kernel(SelectArgs s, uint32_t* status) {
    __shared__ uint32_t wave_tot[kScanNT / 64];
    __shared__ uint32_t run[kScanChunk];
    __shared__ unsigned long long s_total;
    const uint32_t t = threadIdx.x, n = s.n_out;
    uint32_t err = 0;
    const uint32_t n_idx = sel_n_idx(s, err);
    if (t == 0) s_total = 0;
    unsigned long long mine = 0;  // (the u32 prefix may wrap on an output that cannot fit: detected here)
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += kScanChunk) {
        const uint32_t m = min(kScanChunk, n - base);
        for (uint32_t i = t; i < kScanChunk; i += kScanNT) {
            uint32_t c = 0;
            if (i < m) {
                const uint32_t d = sel_src(s, base + i, n_idx, err);
                if (d != kNoDoc) {
                    uint32_t o;
                    c = live_span(s.st.offsets, s.st.counts, d, o, err);
                }
                s.out.counts[base + i] = c;
                mine += c;
            }
            run[i] = c;
        }
        __syncthreads();
        uint32_t v[kScanV], sum = 0;
#pragma unroll
        for (int j = 0; j < kScanV; ++j) {
            v[j] = run[t * kScanV + j];
            sum += v[j];
        }
        uint32_t tot = 0;
        uint32_t p = carry + block_exclusive_scan<kScanNT>(sum, wave_tot, &tot);
#pragma unroll
        for (int j = 0; j < kScanV; ++j) {
            run[t * kScanV + j] = p;
            p += v[j];
        }
        __syncthreads();
        for (uint32_t i = t; i < m; i += kScanNT) s.out.offsets[base + i] = run[i];
        carry += tot;
        __syncthreads();  // (run and wave_tot are reused by the next chunk)
    }
    __syncthreads();
    if (mine) atomicAdd(&s_total, mine);
    __syncthreads();
    if (t == 0) {
        s.out.offsets[n] = carry;
        if (s_total > (unsigned long long)s.out_slots) err |= kErrCapacity;
    }
    flag_error(status, err);
}

__global__ __launch_bounds__(kCmpNT) void select_gather_kernel(SelectArgs s, uint32_t vec) {
    __shared__ uint32_t s_oo[kSelRun];  // output offset of the staged documents
    __shared__ uint32_t s_so[kSelRun];  // offset of the state document each copies
    __shared__ uint32_t s_n[kSelRun];   // live count
    const uint32_t t = threadIdx.x, n_out = s.n_out;
    const uint32_t* ooff = s.out.offsets;
    uint32_t err = 0;  // (reported by select_scan_kernel)
    const uint32_t n_idx = sel_n_idx(s, err);
    // nothing is written at or past out_slots, whatever the scan found
    const uint32_t total = min(ooff[n_out], s.out_slots);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)total + kSelChunk - 1) / kSelChunk);

    auto doc = [&](uint32_t j, uint32_t& oo, uint32_t& so, uint32_t& n) {
        oo = ooff[j];
        n = s.out.counts[j];
        const uint32_t d = n ? sel_src(s, j, n_idx, err) : kNoDoc;
        so = d != kNoDoc ? s.st.offsets[d] : 0u;
        if (d == kNoDoc) n = 0;
    };

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t base = chunk * kSelChunk;
        const uint32_t m = min(kSelChunk, total - base);
        const uint32_t j_lo = cmp_count_le(ooff + 1, n_out - 1, base);
        const uint32_t j_hi = j_lo + cmp_count_le(ooff + 1 + j_lo, n_out - 1 - j_lo, base + (m - 1));
        const uint32_t span = j_hi - j_lo + 1;
        const bool staged = span <= kSelRun;
        if (staged) {
            for (uint32_t x = t; x < span; x += kCmpNT) {
                uint32_t oo, so, n;
                doc(j_lo + x, oo, so, n);
                s_oo[x] = oo;
                s_so[x] = so;
                s_n[x] = n;
            }
            __syncthreads();
        }
        // position p of the output: (copied, index in the state, entries left in its document)
        auto locate = [&](uint32_t p, uint32_t& src, uint32_t& left) {
            uint32_t oo, so, n;
            if (staged) {
                const uint32_t x = cmp_count_le(s_oo + 1, span - 1, p);
                oo = s_oo[x];
                so = s_so[x];
                n = s_n[x];
            } else {
                doc(j_lo + cmp_count_le(ooff + 1 + j_lo, span - 1, p), oo, so, n);
            }
            const uint32_t i = p - oo;
            src = so + i;
            left = i < n ? n - i : 0u;
            return i < n;
        };

        uint32_t c0[kCmpJ], c1[kCmpJ];
        bool m0[kCmpJ], m1[kCmpJ], v[kCmpJ];
#pragma unroll
        for (int j = 0; j < kCmpJ; ++j) {
            const uint32_t rel = 2u * ((uint32_t)j * kCmpNT + t);
            c0[j] = c1[j] = 0;
            m0[j] = m1[j] = false;
            if (rel < m) {
                uint32_t left = 0;
                m0[j] = locate(base + rel, c0[j], left);
                if (rel + 1 < m) {
                    if (left > 1) {
                        c1[j] = c0[j] + 1;
                        m1[j] = true;
                    } else {
                        uint32_t l1;
                        m1[j] = locate(base + rel + 1, c1[j], l1);
                    }
                }
            }
            v[j] = vec && m0[j] && m1[j] && c1[j] == c0[j] + 1 && (c0[j] & 1u) == 0u;
        }
        uint64_t k0[kCmpJ], k1[kCmpJ], n0[kCmpJ], n1[kCmpJ];
        uint32_t a0[kCmpJ], a1[kCmpJ];
#pragma unroll
        for (int j = 0; j < kCmpJ; ++j) {
            k0[j] = k1[j] = n0[j] = n1[j] = 0;
            a0[j] = a1[j] = 0;
            if (v[j]) {
                const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(s.st.keys + c0[j]);
                const ulonglong2 y = *reinterpret_cast<const ulonglong2*>(s.st.counters + c0[j]);
                const uint2 z = *reinterpret_cast<const uint2*>(s.st.actors + c0[j]);
                k0[j] = x.x;
                k1[j] = x.y;
                n0[j] = y.x;
                n1[j] = y.y;
                a0[j] = z.x;
                a1[j] = z.y;
            } else {
                if (m0[j]) {
                    k0[j] = s.st.keys[c0[j]];
                    n0[j] = s.st.counters[c0[j]];
                    a0[j] = s.st.actors[c0[j]];
                }
                if (m1[j]) {
                    k1[j] = s.st.keys[c1[j]];
                    n1[j] = s.st.counters[c1[j]];
                    a1[j] = s.st.actors[c1[j]];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kCmpJ; ++j) {
            const size_t p0 = (size_t)base + 2u * ((uint32_t)j * kCmpNT + t);
            if (v[j]) {  // (p0 is even: the output side of a pair is always aligned)
                *reinterpret_cast<ulonglong2*>(s.out.keys + p0) = make_ulonglong2(k0[j], k1[j]);
                *reinterpret_cast<ulonglong2*>(s.out.counters + p0) = make_ulonglong2(n0[j], n1[j]);
                *reinterpret_cast<uint2*>(s.out.actors + p0) = make_uint2(a0[j], a1[j]);
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

    // clocks: n_out x R words, one lane per actor; an empty document's are zeros
    const uint32_t R = s.st.R;
    const uint64_t nw = (uint64_t)n_out * R;
    for (uint64_t w = (uint64_t)blockIdx.x * kCmpNT + t; w < nw; w += (uint64_t)gridDim.x * kCmpNT) {
        const uint32_t j = (uint32_t)(w / R);
        const uint32_t r = (uint32_t)(w - (uint64_t)j * R);
        const uint32_t d = sel_src(s, j, n_idx, err);
        s.out.vv[w] = d != kNoDoc ? s.st.vv[(size_t)d * R + r] : 0ull;
    }
}

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The worklist step alone, over n flag words another launch wrote (also digest.hip's diff).
hipError_t launch_worklist(const uint32_t* fw, uint32_t n, uint32_t mask, const CompareOutView& out,
                           const uint32_t* gate, hipStream_t stream) {
    hipLaunchKernelGGL(compare_worklist_kernel, dim3(1), dim3(kScanNT), 0, stream, fw, n, mask, out, gate);
    return hipGetLastError();
}

// fw: n_docs workspace words.  n_docs == 0: only the summary and n_work are written.
hipError_t launch_compare(const BatchView& a, const BatchView& b, uint32_t mask, const CompareOutView& out,
                          uint32_t* fw, uint32_t* status, const uint32_t* gate, uint32_t n_cu, hipStream_t stream) {
    const uint32_t n = a.n_docs;
    if (n) {
        const uint32_t dgrid = min((n + 255u) / 256u, n_cu * 8u);
        hipLaunchKernelGGL(compare_docs_kernel, dim3(dgrid), dim3(256), 0, stream, a, b, fw, status, gate);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const uint32_t vec = aligned(a.keys, 16) && aligned(b.keys, 16) && aligned(a.counters, 16) &&
                             aligned(b.counters, 16) && aligned(a.actors, 8) && aligned(b.actors, 8);
        hipLaunchKernelGGL(compare_kernel, dim3(n_cu * 8u), dim3(kCmpNT), 0, stream, a, b, fw, vec, gate);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_worklist(fw, n, mask, out, gate, stream);
}

hipError_t launch_select(const BatchView& st, const uint32_t* idx, const uint32_t* n_idx, uint32_t n_out,
                         uint32_t out_slots, const OutView& out, uint32_t* status, uint32_t n_cu,
                         hipStream_t stream) {
    const SelectArgs s{st, idx, n_idx, n_out, out_slots, out};
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(kScanNT), 0, stream, s, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_out == 0) return e;
    const uint32_t vec = aligned(st.keys, 16) && aligned(st.counters, 16) && aligned(st.actors, 8) &&
                         aligned(out.keys, 16) && aligned(out.counters, 16) && aligned(out.actors, 8);
    hipLaunchKernelGGL(select_gather_kernel, dim3(n_cu * 8u), dim3(kCmpNT), 0, stream, s, vec);
    return hipGetLastError();
}

}  // namespace crdt
