// Per-document state digests of a device-resident batch and their comparison
// (crdt_awset_digest_async, crdt_digest_diff_async; include/crdtgpu.h).
//
// digest[2d] and digest[2d+1] are fmix of sums (mod 2^64) of per-entry,
// per-tombstone and per-clock-word hashes (digest_hash.hpp).  Sums of integers
// commute, so the result does not depend on how the work is cut up nor on the
// order the partial sums arrive in: bit-identical on every run.  The digest
// words themselves are the accumulators, no workspace.  Launches:
//
//   digest_init_kernel     G lanes per document (G: the power of two >= R), one
//       per clock word, summed by a butterfly; the first of them adds
//       K_N * counts (the live counts clamped to the slots, kErrCapacity) and
//       STORES both words: this is what initialises the accumulators.
//   digest_entries_kernel  the unit of work is the slot, not the document
//       (compare_kernel's partition): the slot space [0, offsets[n_docs]) is cut
//       into chunks of kDigChunk positions, grid-stride; a lane takes kDigJ pairs
//       of neighbouring positions.  The chunk finds the documents of its first
//       and last position with a uniform search in offsets and stages their
//       offset and live count in LDS when they are at most kDigRun (wider spans
//       -- many empty or one-entry documents -- search offsets in global memory).
//       Only live positions are read, a pair with 16 B loads (keys, counters;
//       8 B actors) when both are live; all loads of a lane are issued before
//       the first hash.  Per-lane sums are added over the neighbouring lanes of
//       the wave that hold the same document, then over the workgroup's waves
//       in LDS accumulators beside the staged documents.  A document whose live
//       entries all lie in the chunk has one owner, which adds with a plain
//       load and store; only documents that straddle a chunk boundary (and the
//       unstaged spans) use global atomicAdd on u64.
//       Run once over the entries (word 0: hk, word 1: hd) and, when the call
//       has tombstones, once over them (TOMB: word 1 only, ht).
//   digest_final_kernel    fmix of every word.
//
// diff: digest_diff_kernel writes one flag word per document (ELEMENTS when
// word 0 differs, else STATE when word 1 does) and compare.hip's worklist
// kernel turns them into flags, summary and the ascending worklist.
#include "crdt_device.hpp"
#include "digest_hash.hpp"

namespace crdt {

hipError_t launch_worklist(const uint32_t* fw, uint32_t n, uint32_t mask, const CompareOutView& out,
                           const uint32_t* gate, hipStream_t stream);

constexpr int kDigNT = 256;
constexpr int kDigJ = 2;                             // pairs of positions per lane and chunk (4: 86 VGPRs, 5 waves)
constexpr uint32_t kDigChunk = kDigNT * kDigJ * 2;   // 1,024 slot positions per workgroup step
constexpr uint32_t kDigRun = 512;                    // documents staged in LDS at most
constexpr uint32_t kDigNoDoc = 0xFFFFFFFFu;

typedef unsigned long long ull;

// Number of elements of the non-decreasing a[0..n) that are <= x.
__device__ __forceinline__ uint32_t dig_count_le(const uint32_t* a, uint32_t n, uint32_t x) {
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

// G = 1 << g_log lanes per document (G >= R, G <= 64): lane r of a group holds
// clock word r.  tb.offsets == NULL: no tombstones.
__global__ __launch_bounds__(256) void digest_init_kernel(HasView st, HasView tb, const uint64_t* vv, uint32_t R,
                                                          uint32_t g_log, uint64_t* digest, uint32_t* status) {
    const uint32_t G = 1u << g_log;
    const uint64_t n_lanes = (uint64_t)st.n_docs << g_log;
    uint32_t err = 0;
    // (the bound is uniform over the workgroup: every lane of a wave takes part in the shuffles)
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n_lanes; base += (uint64_t)gridDim.x * 256) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t r = (uint32_t)i & (G - 1u);
        const bool doc = i < n_lanes;
        const uint32_t d = doc ? (uint32_t)(i >> g_log) : 0u;
        uint64_t h = doc && r < R ? dig_clock(r, vv[(size_t)d * R + r]) : 0ull;
        for (uint32_t o = G >> 1; o > 0; o >>= 1) h += (uint64_t)__shfl_xor((ull)h, (int)o);
        if (doc && r == 0) {
            uint32_t o, n, m = 0;
            n = live_span(st.offsets, st.counts, d, o, err);
            if (tb.offsets) m = live_span(tb.offsets, tb.counts, d, o, err);
            digest[2 * (size_t)d] = kDigN * n;
            digest[2 * (size_t)d + 1] = h + kDigN * ((uint64_t)n + m);
        }
    }
    flag_error(status, err);
}

// Every lane of the wave holds (d, w0, w1); lanes with the same d are
// neighbours.  On return the first lane of each run holds the run's sums;
// returns whether this lane is one.
template <bool TOMB>
__device__ __forceinline__ bool dig_seg_sum(uint32_t d, uint64_t& w0, uint64_t& w1) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t dn = __shfl_down(d, o);
        const uint64_t x1 = (uint64_t)__shfl_down((ull)w1, o);
        const bool same = lane + o < 64 && dn == d;  // (then every lane between holds d too)
        w1 += same ? x1 : 0ull;
        if (!TOMB) {
            const uint64_t x0 = (uint64_t)__shfl_down((ull)w0, o);
            w0 += same ? x0 : 0ull;
        }
    }
    const uint32_t prev = __shfl_up(d, 1);
    return lane == 0 || prev != d;
}

// One position of the slot space: its document, and whether it is a live entry.
struct DigPos {
    uint32_t d, i, n;
    bool live;
};

template <bool TOMB>
__global__ __launch_bounds__(kDigNT) void digest_entries_kernel(HasView v, uint64_t* digest, uint32_t vec) {
    __shared__ uint32_t s_o[kDigRun];  // offset of the staged documents
    __shared__ uint32_t s_n[kDigRun];  // live count
    __shared__ ull s_w0[TOMB ? 1 : kDigRun];  // the chunk's sums of the staged documents
    __shared__ ull s_w1[kDigRun];
    const uint32_t t = threadIdx.x;
    const uint32_t n_docs = v.n_docs;
    const uint32_t total = v.offsets[n_docs];
    const uint32_t n_chunks = (uint32_t)(((uint64_t)total + kDigChunk - 1) / kDigChunk);

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t base = chunk * kDigChunk;  // (base < total)
        const uint32_t m = min(kDigChunk, total - base);
        // Documents of the chunk's first and last position.  The search runs over
        // offsets[1 .. n_docs), so whatever the offsets hold the answer is a document.
        const uint32_t d_lo = dig_count_le(v.offsets + 1, n_docs - 1, base);
        const uint32_t d_hi = d_lo + dig_count_le(v.offsets + 1 + d_lo, n_docs - 1 - d_lo, base + (m - 1));
        const uint32_t span = d_hi - d_lo + 1;
        const bool staged = span <= kDigRun;
        if (staged) {
            for (uint32_t x = t; x < span; x += kDigNT) {
                uint32_t o, n, err = 0;  // (reported by digest_init_kernel)
                n = live_span(v.offsets, v.counts, d_lo + x, o, err);
                s_o[x] = o;
                s_n[x] = n;
                if (!TOMB) s_w0[x] = 0;
                s_w1[x] = 0;
            }
            __syncthreads();
        }
        auto locate = [&](uint32_t p) {
            DigPos r;
            uint32_t o;
            if (staged) {
                const uint32_t x = dig_count_le(s_o + 1, span - 1, p);
                o = s_o[x];
                r.n = s_n[x];
                r.d = d_lo + x;
            } else {
                uint32_t err = 0;
                r.d = d_lo + dig_count_le(v.offsets + 1 + d_lo, span - 1, p);
                r.n = live_span(v.offsets, v.counts, r.d, o, err);
            }
            r.i = p - o;  // (below the document: wraps, never < n)
            r.live = r.i < r.n;
            return r;
        };
        // (d is a document of [d_lo, d_hi]: staged, d - d_lo < span <= kDigRun)
        auto add = [&](uint32_t d, uint64_t w0, uint64_t w1) {
            if (staged) {
                if (!TOMB) atomicAdd(&s_w0[d - d_lo], (ull)w0);
                atomicAdd(&s_w1[d - d_lo], (ull)w1);
            } else {
                if (!TOMB) atomicAdd(reinterpret_cast<ull*>(digest) + 2 * (size_t)d, (ull)w0);
                atomicAdd(reinterpret_cast<ull*>(digest) + 2 * (size_t)d + 1, (ull)w1);
            }
        };

        uint32_t d0[kDigJ], d1[kDigJ];
        bool m0[kDigJ], m1[kDigJ];
#pragma unroll
        for (int j = 0; j < kDigJ; ++j) {
            const uint32_t rel = 2u * ((uint32_t)j * kDigNT + t);
            d0[j] = d1[j] = kDigNoDoc;
            m0[j] = m1[j] = false;
            if (rel < m) {
                const DigPos e0 = locate(base + rel);
                d0[j] = e0.d;
                m0[j] = e0.live;
                if (e0.live && e0.i + 1 < e0.n) {  // the neighbour is the same document's next entry
                    d1[j] = e0.d;
                    m1[j] = true;
                } else if (rel + 1 < m) {
                    const DigPos e1 = locate(base + rel + 1);
                    d1[j] = e1.d;
                    m1[j] = e1.live;
                }
            }
        }

        // every load of the lane before the first hash; a position that is not live is not read
        uint64_t k0[kDigJ], k1[kDigJ], c0[kDigJ], c1[kDigJ];
        uint32_t a0[kDigJ], a1[kDigJ];
#pragma unroll
        for (int j = 0; j < kDigJ; ++j) {
            const size_t p0 = (size_t)base + 2u * ((uint32_t)j * kDigNT + t);  // (even)
            k0[j] = k1[j] = c0[j] = c1[j] = 0;
            a0[j] = a1[j] = 0;
            if (vec && m0[j] && m1[j]) {
                const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(v.keys + p0);
                const ulonglong2 y = *reinterpret_cast<const ulonglong2*>(v.counters + p0);
                const uint2 z = *reinterpret_cast<const uint2*>(v.actors + p0);
                k0[j] = x.x;
                k1[j] = x.y;
                c0[j] = y.x;
                c1[j] = y.y;
                a0[j] = z.x;
                a1[j] = z.y;
            } else {
                if (m0[j]) {
                    k0[j] = v.keys[p0];
                    c0[j] = v.counters[p0];
                    a0[j] = v.actors[p0];
                }
                if (m1[j]) {
                    k1[j] = v.keys[p0 + 1];
                    c1[j] = v.counters[p0 + 1];
                    a1[j] = v.actors[p0 + 1];
                }
            }
        }

        // the terms of pair j: (word 0, word 1) of each position, zero where it is not live
        auto terms = [&](int j, uint64_t& u0, uint64_t& u1, uint64_t& x0, uint64_t& x1) {
            const uint64_t h0 = TOMB ? dig_fmix(k0[j] + kDigT) : dig_key(k0[j]);
            const uint64_t h1 = TOMB ? dig_fmix(k1[j] + kDigT) : dig_key(k1[j]);
            u0 = m0[j] ? h0 : 0ull;
            u1 = m0[j] ? dig_dot(h0, a0[j], c0[j]) : 0ull;
            x0 = m1[j] ? h1 : 0ull;
            x1 = m1[j] ? dig_dot(h1, a1[j], c1[j]) : 0ull;
        };

        // One document under the whole wave (a large document): sum in the lane, then one butterfly.
        const uint32_t dw = uniform(d0[0]);
        bool one = dw != kDigNoDoc;
#pragma unroll
        for (int j = 0; j < kDigJ; ++j) one = one && d0[j] == dw && d1[j] == dw;
        if (ballot(!one) == 0ull) {
            uint64_t w0 = 0, w1 = 0;
#pragma unroll
            for (int j = 0; j < kDigJ; ++j) {
                uint64_t u0, u1, x0, x1;
                terms(j, u0, u1, x0, x1);
                w0 += u0 + x0;
                w1 += u1 + x1;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                if (!TOMB) w0 += (uint64_t)__shfl_xor((ull)w0, o);
                w1 += (uint64_t)__shfl_xor((ull)w1, o);
            }
            if (lane_id() == 0) add(dw, w0, w1);
        } else {
#pragma unroll
            for (int j = 0; j < kDigJ; ++j) {
                uint64_t u0, u1, x0, x1;
                terms(j, u0, u1, x0, x1);
                const bool same = d1[j] == d0[j];
                uint64_t w0 = u0 + (same ? x0 : 0ull), w1 = u1 + (same ? x1 : 0ull);
                const bool head = dig_seg_sum<TOMB>(d0[j], w0, w1);
                if (head && d0[j] != kDigNoDoc) add(d0[j], w0, w1);
                if (!same && m1[j]) add(d1[j], x0, x1);  // (live: d1 is a document)
            }
        }

        if (staged) {
            __syncthreads();
            for (uint32_t x = t; x < span; x += kDigNT) {
                const uint64_t lo = s_o[x], hi = lo + s_n[x], end = (uint64_t)base + m;
                if (hi <= lo || lo >= end || hi <= base) continue;  // no live position of it in this chunk
                ull* w = reinterpret_cast<ull*>(digest) + 2 * (size_t)(d_lo + x);
                if (lo >= base && hi <= end) {  // all of it: this workgroup step is its only writer
                    if (!TOMB) w[0] += s_w0[x];
                    w[1] += s_w1[x];
                } else {
                    if (!TOMB) atomicAdd(w, s_w0[x]);
                    atomicAdd(w + 1, s_w1[x]);
                }
            }
        }
        __syncthreads();  // (the staged arrays are reused by the next chunk)
    }
}

__global__ __launch_bounds__(256) void digest_final_kernel(uint64_t* digest, uint64_t n_words) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * 256)
        digest[i] = dig_fmix(digest[i]);
}

__global__ __launch_bounds__(256) void digest_diff_kernel(const uint64_t* mine, const uint64_t* theirs, uint32_t n,
                                                          uint32_t* fw) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const bool e = mine[2 * i] != theirs[2 * i], s = mine[2 * i + 1] != theirs[2 * i + 1];
        fw[i] = e ? CRDT_DIG_ELEMENTS : (s ? CRDT_DIG_STATE : 0u);
    }
}

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static uint32_t view_vec(const HasView& v) { return aligned(v.keys, 16) && aligned(v.counters, 16) && aligned(v.actors, 8); }

// tb.offsets == NULL: no tombstones.  n_docs == 0: nothing is launched.
hipError_t launch_digest(const HasView& st, const HasView& tb, const uint64_t* vv, uint32_t R, uint64_t* digest,
                         uint32_t* status, uint32_t n_cu, hipStream_t stream) {
    const uint32_t n = st.n_docs;
    if (n == 0) return hipSuccess;
    uint32_t g_log = 0;
    while ((1u << g_log) < R) ++g_log;
    const uint64_t init_blocks = (((uint64_t)n << g_log) + 255u) / 256u;
    hipLaunchKernelGGL(digest_init_kernel, dim3((uint32_t)std::min<uint64_t>(init_blocks, n_cu * 8u)), dim3(256), 0,
                       stream, st, tb, vv, R, g_log, digest, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(digest_entries_kernel<false>, dim3(n_cu * 8u), dim3(kDigNT), 0, stream, st, digest,
                       view_vec(st));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (tb.offsets) {
        hipLaunchKernelGGL(digest_entries_kernel<true>, dim3(n_cu * 8u), dim3(kDigNT), 0, stream, tb, digest,
                           view_vec(tb));
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint64_t fin_blocks = (2ull * n + 255u) / 256u;
    hipLaunchKernelGGL(digest_final_kernel, dim3((uint32_t)std::min<uint64_t>(fin_blocks, n_cu * 8u)), dim3(256), 0,
                       stream, digest, 2ull * n);
    return hipGetLastError();
}

// fw: n_docs workspace words.  n_docs == 0: only the summary and n_work are written.
hipError_t launch_digest_diff(const uint64_t* mine, const uint64_t* theirs, uint32_t n, uint32_t mask,
                              const CompareOutView& out, uint32_t* fw, const uint32_t* gate, uint32_t n_cu,
                              hipStream_t stream) {
    if (n) {
        hipLaunchKernelGGL(digest_diff_kernel, dim3(std::min((n + 255u) / 256u, n_cu * 8u)), dim3(256), 0, stream,
                           mine, theirs, n, fw);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_worklist(fw, n, mask, out, gate, stream);
}

}  // namespace crdt
