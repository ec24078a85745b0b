// Per-document state digests of the documents a worklist names
// (crdt_awset_digest_idx_async; include/crdtgpu.h, "worklist digests").
//
// The unit of work is the listed document, not the slot space (digest.hip): each
// listed document has one owner, which sums its terms (digest_hash.hpp) in
// registers, finalises them and stores its two words at digest[2 * idx[j]].  No
// accumulator in global memory, no atomic, no init or final pass, no workspace;
// no digest word outside the listed documents is read or written.  Sums of
// integers commute, so the words are bit for bit those of digest.hip and of
// crdt_awset_digest_host, on every run.  Launches:
//
//   digest_idx_wave_kernel   one wavefront per listed document, grid-stride over
//       the list.  The wave walks the live prefix of the entries, then of the
//       tombstones, in steps of 128 positions: a lane takes the pair at an even
//       position with 16 B loads (keys, counters; 8 B actors) when both are live
//       and the arrays are aligned, the scalar form for the odd first and last
//       position of a document that starts or ends at an odd slot; the step's
//       loads are issued before its hashes.  Lane r < R adds clock word r.  One
//       butterfly per word, + K_N * n / K_N * (n + m), fmix, one 16 B store.
//       Documents of more than kDigIdxWave live entries plus tombstones are left
//       to the block kernel.  Reports every error of the call: *n_idx above
//       n_max and counts above their slots (kErrCapacity, both clamped), idx[j]
//       that is no document (kErrIndex, nothing written for it).
//   digest_idx_block_kernel  the same list again, `per` entries per workgroup step
//       (n_max spread over the grid, 1 ... 256: a short list gives every large
//       document a workgroup of its own, a long one costs one offsets read per
//       entry and thread): each thread reads one listed document's spans, the
//       ones above kDigIdxWave are staged in LDS and then walked by the whole
//       workgroup one after the other, kDigIdxJ pairs per thread and step,
//       reduced over the waves in LDS.  A document of 2^20 entries is one
//       workgroup's serial walk.
#include "crdt_device.hpp"
#include "digest_hash.hpp"

namespace crdt {

constexpr uint32_t kDigIdxWave = 2048;  // live entries + tombstones one wavefront takes at most
constexpr int kDigIdxNT = 256;          // threads of the block kernel, list entries per workgroup step at most
constexpr int kDigIdxJ = 4;             // pairs of positions per thread and step of the block kernel

typedef unsigned long long ull;

struct DigIdxArgs {
    HasView st, tb;  // tb.offsets == NULL: no tombstones
    const uint64_t* vv;
    uint32_t R;
    const uint32_t* idx;
    const uint32_t* n_idx;  // NULL: n_max
    uint32_t n_max, n_digest;
    uint32_t place;  // CRDT_DIGEST_PLACE: listed document j is state document j
    uint32_t vec_st, vec_tb, vec_out;
    uint64_t* digest;
};

// Documents listed, clamped to n_max.
__device__ __forceinline__ uint32_t dig_idx_n(const DigIdxArgs& a, uint32_t& err) {
    uint32_t n = a.n_idx ? *a.n_idx : a.n_max;
    if (n > a.n_max) {
        err |= kErrCapacity;
        n = a.n_max;
    }
    return n;
}

// Listed document j: the document d whose digest words it writes and the state
// document sd it reads; false when idx[j] is no document.
__device__ __forceinline__ bool dig_idx_doc(const DigIdxArgs& a, uint32_t j, uint32_t& d, uint32_t& sd, uint32_t& err) {
    d = a.idx[j];
    if (d >= a.n_digest || (!a.place && d >= a.st.n_docs)) {
        err |= kErrIndex;
        return false;
    }
    sd = a.place ? j : d;  // (place: j < n_max <= st.n_docs, checked by the call)
    return true;
}

// The terms of the live positions [o, o + n) of v, added to w0 (entries only)
// and w1: thread t of nt takes J pairs per step, the pair at even position
// (o & ~1) + 2 * (j * nt + t) + step * 2 * J * nt.  Only live positions are read.
template <bool TOMB, int J>
__device__ __forceinline__ void dig_idx_walk(const HasView& v, uint32_t vec, uint32_t o, uint32_t n, uint32_t t,
                                             uint32_t nt, uint64_t& w0, uint64_t& w1) {
    const uint64_t lo = o, hi = (uint64_t)o + n;
    for (uint64_t base = lo & ~1ull; base < hi; base += 2ull * J * nt) {
        uint64_t k0[J], k1[J], c0[J], c1[J];
        uint32_t a0[J], a1[J];
        bool m0[J], m1[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const uint64_t p = base + 2ull * ((uint32_t)j * nt + t);  // (even)
            m0[j] = p >= lo && p < hi;
            m1[j] = p + 1 < hi;  // (p + 1 >= lo always)
            k0[j] = k1[j] = c0[j] = c1[j] = 0;
            a0[j] = a1[j] = 0;
            if (vec && m0[j] && m1[j]) {
                const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(v.keys + p);
                const ulonglong2 y = *reinterpret_cast<const ulonglong2*>(v.counters + p);
                const uint2 z = *reinterpret_cast<const uint2*>(v.actors + p);
                k0[j] = x.x;
                k1[j] = x.y;
                c0[j] = y.x;
                c1[j] = y.y;
                a0[j] = z.x;
                a1[j] = z.y;
            } else {
                if (m0[j]) {
                    k0[j] = v.keys[p];
                    c0[j] = v.counters[p];
                    a0[j] = v.actors[p];
                }
                if (m1[j]) {
                    k1[j] = v.keys[p + 1];
                    c1[j] = v.counters[p + 1];
                    a1[j] = v.actors[p + 1];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const uint64_t h0 = TOMB ? dig_fmix(k0[j] + kDigT) : dig_key(k0[j]);
            const uint64_t h1 = TOMB ? dig_fmix(k1[j] + kDigT) : dig_key(k1[j]);
            if (!TOMB) w0 += (m0[j] ? h0 : 0ull) + (m1[j] ? h1 : 0ull);
            w1 += (m0[j] ? dig_dot(h0, a0[j], c0[j]) : 0ull) + (m1[j] ? dig_dot(h1, a1[j], c1[j]) : 0ull);
        }
    }
}

__device__ __forceinline__ uint64_t dig_idx_wave_sum(uint64_t w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w += (uint64_t)__shfl_xor((ull)w, o);
    return w;
}

// sum0 / sum1: the sums of the terms of document d (n live entries, m live tombstones).
__device__ __forceinline__ void dig_idx_store(const DigIdxArgs& a, uint32_t d, uint32_t n, uint32_t m, uint64_t sum0,
                                              uint64_t sum1) {
    const uint64_t w0 = dig_fmix(sum0 + kDigN * n);
    const uint64_t w1 = dig_fmix(sum1 + kDigN * ((uint64_t)n + m));
    uint64_t* w = a.digest + 2 * (size_t)d;
    if (a.vec_out) {
        *reinterpret_cast<ulonglong2*>(w) = make_ulonglong2(w0, w1);
    } else {
        w[0] = w0;
        w[1] = w1;
    }
}

__global__ __launch_bounds__(256) void digest_idx_wave_kernel(DigIdxArgs a, uint32_t* status) {
    const uint32_t lane = lane_id();
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    uint32_t err = 0;
    const uint32_t n_list = dig_idx_n(a, err);
    // (j is the same in every lane of the wave: all of them take part in the butterflies)
    for (uint64_t j = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); j < n_list; j += n_waves) {
        uint32_t d, sd;
        if (!dig_idx_doc(a, (uint32_t)j, d, sd, err)) continue;
        uint32_t o, ot = 0, m = 0;
        const uint32_t n = live_span(a.st.offsets, a.st.counts, sd, o, err);
        if (a.tb.offsets) m = live_span(a.tb.offsets, a.tb.counts, sd, ot, err);
        if ((uint64_t)n + m > kDigIdxWave) continue;  // the block kernel's
        uint64_t w0 = 0, w1 = 0;
        dig_idx_walk<false, 1>(a.st, a.vec_st, o, n, lane, 64, w0, w1);
        if (m) dig_idx_walk<true, 1>(a.tb, a.vec_tb, ot, m, lane, 64, w0, w1);
        if (lane < a.R) w1 += dig_clock(lane, a.vv[(size_t)sd * a.R + lane]);
        w0 = dig_idx_wave_sum(w0);
        w1 = dig_idx_wave_sum(w1);
        if (lane == 0) dig_idx_store(a, d, n, m, w0, w1);
    }
    flag_error(status, err);
}

// per: list entries per workgroup step, 1 ... kDigIdxNT.
__global__ __launch_bounds__(kDigIdxNT) void digest_idx_block_kernel(DigIdxArgs a, uint32_t per) {
    __shared__ uint32_t s_big[kDigIdxNT];  // the step's list entries above the wave bound
    __shared__ uint32_t s_nbig;
    __shared__ ull s_w0[kDigIdxNT / 64], s_w1[kDigIdxNT / 64];
    const uint32_t t = threadIdx.x;
    uint32_t err = 0;  // (reported by digest_idx_wave_kernel)
    const uint32_t n_list = dig_idx_n(a, err);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)n_list + per - 1) / per);
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        if (t == 0) s_nbig = 0;
        __syncthreads();
        const uint64_t j = (uint64_t)chunk * per + t;
        uint32_t d, sd;
        if (t < per && j < n_list && dig_idx_doc(a, (uint32_t)j, d, sd, err)) {
            uint32_t o, m = 0;
            const uint32_t n = live_span(a.st.offsets, a.st.counts, sd, o, err);
            if (a.tb.offsets) m = live_span(a.tb.offsets, a.tb.counts, sd, o, err);
            if ((uint64_t)n + m > kDigIdxWave) s_big[atomicAdd(&s_nbig, 1u)] = (uint32_t)j;  // (any order)
        }
        __syncthreads();
        const uint32_t n_big = s_nbig;
        for (uint32_t x = 0; x < n_big; ++x) {
            (void)dig_idx_doc(a, s_big[x], d, sd, err);  // (a document: staged above)
            uint32_t o, ot = 0, m = 0;
            const uint32_t n = live_span(a.st.offsets, a.st.counts, sd, o, err);
            if (a.tb.offsets) m = live_span(a.tb.offsets, a.tb.counts, sd, ot, err);
            uint64_t w0 = 0, w1 = 0;
            dig_idx_walk<false, kDigIdxJ>(a.st, a.vec_st, o, n, t, kDigIdxNT, w0, w1);
            if (m) dig_idx_walk<true, kDigIdxJ>(a.tb, a.vec_tb, ot, m, t, kDigIdxNT, w0, w1);
            if (t < a.R) w1 += dig_clock(t, a.vv[(size_t)sd * a.R + t]);
            w0 = dig_idx_wave_sum(w0);
            w1 = dig_idx_wave_sum(w1);
            if ((t & 63u) == 0) {
                s_w0[t >> 6] = w0;
                s_w1[t >> 6] = w1;
            }
            __syncthreads();
            if (t == 0) {
                uint64_t sum0 = 0, sum1 = 0;
#pragma unroll
                for (int w = 0; w < kDigIdxNT / 64; ++w) {
                    sum0 += s_w0[w];
                    sum1 += s_w1[w];
                }
                dig_idx_store(a, d, n, m, sum0, sum1);
            }
            __syncthreads();  // (the partial sums are reused by the next document)
        }
        // (s_big and s_nbig are reused by the next step: the barrier above, or none taken and
        // the one below)
        __syncthreads();
    }
}

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static uint32_t view_vec(const HasView& v) { return aligned(v.keys, 16) && aligned(v.counters, 16) && aligned(v.actors, 8); }

// tb.offsets == NULL: no tombstones.  n_max == 0: nothing is launched.
hipError_t launch_digest_idx(const HasView& st, const HasView& tb, const uint64_t* vv, uint32_t R, const uint32_t* idx,
                             const uint32_t* n_idx, uint32_t n_max, uint32_t n_digest, uint32_t mode, uint64_t* digest,
                             uint32_t* status, uint32_t n_cu, hipStream_t stream) {
    if (n_max == 0) return hipSuccess;
    const DigIdxArgs a{st,    tb,       vv,   R,           idx,      n_idx,
                       n_max, n_digest, mode, view_vec(st), tb.offsets ? view_vec(tb) : 0u, aligned(digest, 16),
                       digest};
    const uint32_t wave_blocks = (uint32_t)(((uint64_t)n_max + 3u) / 4u);
    hipLaunchKernelGGL(digest_idx_wave_kernel, dim3(std::min(wave_blocks, n_cu * 8u)), dim3(256), 0, stream, a,
                       status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t grid = n_cu * 8u;
    const uint32_t per = std::min<uint32_t>((uint32_t)(((uint64_t)n_max + grid - 1) / grid), kDigIdxNT);  // (>= 1)
    const uint32_t chunks = (uint32_t)(((uint64_t)n_max + per - 1) / per);
    hipLaunchKernelGGL(digest_idx_block_kernel, dim3(std::min(chunks, grid)), dim3(kDigIdxNT), 0, stream, a, per);
    return hipGetLastError();
}

}  // namespace crdt
