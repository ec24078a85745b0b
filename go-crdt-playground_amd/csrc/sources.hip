// Sources: P resident replicas of every document gathered into one packed,
// source-major batch (crdt_awset_sources_async; include/crdtgpu.h) -- the shape
// the folds and the delta extraction read.  Source s = d * P + p is replica p's
// document d: its actor, its clock, the live prefix of its entries and of its
// tombstones, packed with no slack in the order they had.  The unit of the
// offset scan is the source, not the document.  Five launches (six with
// tombstones), ordered by their kernel boundaries alone:
//
//   sources_count_kernel     the offsets' scan, step 1: the sources are cut into
//       chunks of kSrcScanChunk; workgroup c sums the live entry counts and the
//       live tombstone counts (each clamped to its slots, kErrCapacity) of chunk
//       c into parts_e[c] and parts_t[c], 64-bit sums stored saturated at
//       2^32 - 1.
//   sources_partials_kernel  step 2, one workgroup: both partial arrays become
//       their exclusive prefixes, kSrcPartStep partials per step; the running
//       totals are kept in 64 bits for the checks against entry_slots and
//       tomb_slots, and entry_off[n_srcs] / tomb_off[n_srcs] are written.
//   sources_emit_kernel      step 3: workgroup c rescans its chunk on top of its
//       two partials and writes entry_off, tomb_off and src_actor; doc_srcs
//       (d * P, no scan) is written grid-stride by the same launch.
//       No workgroup of any step waits for a word another workgroup of the same
//       launch writes: no look-back, no polling.
//   sources_gather_kernel<0> the shape of scatter_gather_kernel (scatter.hip): the
//       OUTPUT positions are cut into chunks of kSrcGatherChunk, grid-stride; the
//       sources of a chunk are found through the entry_off just written and
//       staged in LDS (at most kSrcRun of them: beyond, lanes search entry_off in
//       global memory) with their replica, source slot offset and live count.  A
//       lane takes kSrcJ pairs of neighbouring positions; a pair that lies in one
//       document at an even source index is read with 16 B loads (keys,
//       counters; 8 B actors), any other element by element; all loads of a lane
//       are issued before its first store, and the stores of a pair are 16 B.
//       Then the clocks, one lane per word.
//   sources_gather_kernel<1> the same over the tombstones, through tomb_off
//       (launched when some replica has tombstones).
//
// The replica descriptors travel by value in the kernel arguments (SourcesArgs,
// 1.7 KB), so a call needs no table in device memory and no copy node in a
// captured graph.  A kernel never indexes that argument array with a lane's
// replica number (that would spill it to scratch): the first thread copies the
// columns it needs into an LDS table, one constant index at a time, and a lane
// picks its replica's column pointers with one LDS read each.
//
// Workspace: parts_e and parts_t, one word each per chunk of kSrcScanChunk sources.
#include "crdt_device.hpp"
#include "merge_block.hpp"

namespace crdt {

constexpr int kSrcNT = 256;
constexpr int kSrcV = 4;                                 // sources per lane and scan chunk
constexpr uint32_t kSrcScanChunk = kSrcNT * kSrcV;       // 1,024 sources per scan workgroup
constexpr int kSrcPartNT = 1024;
constexpr uint32_t kSrcPartStep = kSrcPartNT;            // partials one step of the partials scan holds
constexpr int kSrcJ = 4;                                 // pairs of positions per lane and gather chunk
constexpr uint32_t kSrcGatherChunk = kSrcNT * kSrcJ * 2; // 2,048 output positions per gather step
constexpr uint32_t kSrcRun = 1024;                       // sources staged in LDS at most

// What the scan reads of a replica.
struct SrcScanRow {
    const uint32_t* e_off;
    const uint32_t* e_cnt;
    const uint32_t* t_off;
    const uint32_t* t_cnt;
    const uint32_t* doc_actor;
    uint32_t actor;
};

// Number of elements of the non-decreasing a[0..n) that are <= x.
__device__ __forceinline__ uint32_t src_count_le(const uint32_t* a, uint32_t n, uint32_t x) {
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

// The scan's LDS table, filled by the first thread with constant indices into the arguments.
__device__ __forceinline__ void src_scan_table(const SourcesArgs& s, SrcScanRow* tab) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int p = 0; p < kSrcMaxReps; ++p)
            tab[p] = SrcScanRow{s.rep[p].e.off, s.rep[p].e.cnt, s.rep[p].t.off,
                                s.rep[p].t.cnt, s.rep[p].doc_actor, s.rep[p].actor};
    }
    __syncthreads();
}

__global__ __launch_bounds__(kSrcNT) void sources_count_kernel(SourcesArgs s, uint32_t* parts_e, uint32_t* parts_t,
                                                               uint32_t* status) {
    __shared__ SrcScanRow tab[kSrcMaxReps];
    __shared__ unsigned long long s_sum[2];
    const uint32_t t = threadIdx.x, n = s.n_srcs;
    const uint32_t base = blockIdx.x * kSrcScanChunk;  // (< n: the grid is the number of chunks)
    const uint32_t m = min(kSrcScanChunk, n - base);
    if (t < 2) s_sum[t] = 0;
    src_scan_table(s, tab);
    uint32_t err = 0;
    unsigned long long me = 0, mt = 0;
#pragma unroll
    for (int k = 0; k < kSrcV; ++k) {
        const uint32_t i = (uint32_t)k * kSrcNT + t;
        if (i < m) {
            const uint32_t src = base + i, d = src / s.n_reps, p = src - d * s.n_reps;
            uint32_t o;
            me += (tab[p].e_off ? live_span(tab[p].e_off, tab[p].e_cnt, d, o, err) : 0u);
            mt += (tab[p].t_off ? live_span(tab[p].t_off, tab[p].t_cnt, d, o, err) : 0u);
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
__device__ __forceinline__ uint32_t src_partials(uint32_t* parts, uint32_t n_parts, uint32_t slots, uint32_t* wave_tot,
                                                 unsigned long long* s_total, bool* over) {
    const uint32_t t = threadIdx.x;
    if (t == 0) *s_total = 0;
    unsigned long long mine = 0;  // (the u32 prefix may wrap on an output that cannot fit: detected here)
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_parts; base += kSrcPartStep) {
        const bool in = t < n_parts - base;
        const uint32_t v = in ? parts[base + t] : 0u;
        mine += v;
        uint32_t tot = 0;
        const uint32_t p = carry + block_exclusive_scan<kSrcPartNT>(v, wave_tot, &tot);
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

// tomb_total / doc_srcs0 may be NULL (no tomb_off passed / some document exists).
__global__ __launch_bounds__(kSrcPartNT) void sources_partials_kernel(uint32_t* parts_e, uint32_t* parts_t,
                                                                      uint32_t n_parts, uint32_t entry_slots,
                                                                      uint32_t tomb_slots, uint32_t* entry_total,
                                                                      uint32_t* tomb_total, uint32_t* doc_srcs0,
                                                                      uint32_t* status) {
    __shared__ uint32_t wave_tot[kSrcPartNT / 64];
    __shared__ unsigned long long s_total;
    bool over_e = false, over_t = false;
    const uint32_t te = src_partials(parts_e, n_parts, entry_slots, wave_tot, &s_total, &over_e);
    const uint32_t tt = src_partials(parts_t, n_parts, tomb_slots, wave_tot, &s_total, &over_t);
    uint32_t err = 0;
    if (threadIdx.x == 0) {
        *entry_total = te;
        if (tomb_total) *tomb_total = tt;
        if (doc_srcs0) *doc_srcs0 = 0u;
        if (over_e || over_t) err |= kErrCapacity;
    }
    flag_error(status, err);
}

__global__ __launch_bounds__(kSrcNT) void sources_emit_kernel(SourcesArgs s, const uint32_t* parts_e,
                                                              const uint32_t* parts_t) {
    __shared__ SrcScanRow tab[kSrcMaxReps];
    __shared__ uint32_t wave_tot[kSrcNT / 64];
    __shared__ uint32_t run_e[kSrcScanChunk];
    __shared__ uint32_t run_t[kSrcScanChunk];
    const uint32_t t = threadIdx.x, n = s.n_srcs;
    const uint32_t base = blockIdx.x * kSrcScanChunk;
    const uint32_t m = min(kSrcScanChunk, n - base);
    src_scan_table(s, tab);
    uint32_t err = 0;  // (reported by sources_count_kernel)
#pragma unroll
    for (int k = 0; k < kSrcV; ++k) {
        const uint32_t i = (uint32_t)k * kSrcNT + t;
        uint32_t ce = 0, ct = 0;
        if (i < m) {
            const uint32_t src = base + i, d = src / s.n_reps, p = src - d * s.n_reps;
            uint32_t o;
            ce = tab[p].e_off ? live_span(tab[p].e_off, tab[p].e_cnt, d, o, err) : 0u;
            ct = tab[p].t_off ? live_span(tab[p].t_off, tab[p].t_cnt, d, o, err) : 0u;
            const uint32_t* da = tab[p].doc_actor;
            s.out.src_actor[src] = da ? da[d] : tab[p].actor;
        }
        run_e[i] = ce;
        run_t[i] = ct;
    }
    __syncthreads();
    uint32_t ve[kSrcV], vt[kSrcV], sum_e = 0, sum_t = 0;
#pragma unroll
    for (int k = 0; k < kSrcV; ++k) {
        ve[k] = run_e[t * kSrcV + k];
        vt[k] = run_t[t * kSrcV + k];
        sum_e += ve[k];
        sum_t += vt[k];
    }
    uint32_t tot = 0;
    uint32_t pe = parts_e[blockIdx.x] + block_exclusive_scan<kSrcNT>(sum_e, wave_tot, &tot);
    uint32_t pt = parts_t[blockIdx.x] + block_exclusive_scan<kSrcNT>(sum_t, wave_tot, &tot);
#pragma unroll
    for (int k = 0; k < kSrcV; ++k) {
        run_e[t * kSrcV + k] = pe;
        run_t[t * kSrcV + k] = pt;
        pe += ve[k];
        pt += vt[k];
    }
    __syncthreads();
    for (uint32_t i = t; i < m; i += kSrcNT) {
        s.out.entry_off[base + i] = run_e[i];
        if (s.out.tomb_off) s.out.tomb_off[base + i] = run_t[i];
    }
    // doc_srcs[d] = d * P for d <= n_docs: no scan (n_docs * P < 2^32)
    for (uint64_t d = (uint64_t)blockIdx.x * kSrcNT + t; d <= s.n_docs; d += (uint64_t)gridDim.x * kSrcNT)
        s.out.doc_srcs[d] = (uint32_t)d * s.n_reps;
}

// KIND 0: the entries through entry_off, then the clocks; KIND 1: the tombstones through tomb_off.
template <int KIND>
__global__ __launch_bounds__(kSrcNT) void sources_gather_kernel(SourcesArgs s, uint32_t vec) {
    __shared__ SrcCols tab[kSrcMaxReps];
    __shared__ const uint64_t* tab_vv[kSrcMaxReps];
    __shared__ uint32_t s_oo[kSrcRun];  // output offset of the staged sources
    __shared__ uint32_t s_so[kSrcRun];  // slot offset of the document each copies
    __shared__ uint32_t s_n[kSrcRun];   // live count
    __shared__ uint32_t s_rp[kSrcRun];  // replica
    const uint32_t t = threadIdx.x, n_srcs = s.n_srcs, P = s.n_reps;
    if (t == 0) {
#pragma unroll
        for (int p = 0; p < kSrcMaxReps; ++p) {
            tab[p] = KIND ? s.rep[p].t : s.rep[p].e;
            tab_vv[p] = s.rep[p].vv;
        }
    }
    __syncthreads();
    const uint32_t* ooff = KIND ? s.out.tomb_off : s.out.entry_off;
    uint64_t* okeys = KIND ? s.out.tkeys : s.out.keys;
    uint32_t* oactors = KIND ? s.out.tactors : s.out.actors;
    uint64_t* ocounters = KIND ? s.out.tcounters : s.out.counters;
    // nothing is written at or past the slots, whatever the scan found
    const uint32_t total = min(ooff[n_srcs], KIND ? s.tomb_slots : s.entry_slots);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)total + kSrcGatherChunk - 1) / kSrcGatherChunk);

    // source x: its output offset, the slot offset and clamped live count of its document, its replica
    auto src = [&](uint32_t x, uint32_t& oo, uint32_t& so, uint32_t& n, uint32_t& rp) {
        oo = ooff[x];
        const uint32_t d = x / P;
        rp = x - d * P;
        uint32_t err = 0;  // (reported by sources_count_kernel)
        so = 0;
        n = tab[rp].off ? live_span(tab[rp].off, tab[rp].cnt, d, so, err) : 0u;  // NULL: no such column set
    };

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t base = chunk * kSrcGatherChunk;
        const uint32_t m = min(kSrcGatherChunk, total - base);
        // Sources of the chunk's first and last position.  The search runs over
        // ooff[1 .. n_srcs), so whatever the offsets hold the answer is a source.
        const uint32_t x_lo = src_count_le(ooff + 1, n_srcs - 1, base);
        const uint32_t x_hi = x_lo + src_count_le(ooff + 1 + x_lo, n_srcs - 1 - x_lo, base + (m - 1));
        const uint32_t span = x_hi - x_lo + 1;
        const bool staged = span <= kSrcRun;
        if (staged) {
            for (uint32_t x = t; x < span; x += kSrcNT) {
                uint32_t oo, so, n, rp;
                src(x_lo + x, oo, so, n, rp);
                s_oo[x] = oo;
                s_so[x] = so;
                s_n[x] = n;
                s_rp[x] = rp;
            }
            __syncthreads();
        }
        // position p of the output: (copied, index in its replica's columns, the replica,
        // entries left in its document)
        auto locate = [&](uint32_t p, uint32_t& at, uint32_t& rp, uint32_t& left) {
            uint32_t oo, so, n;
            if (staged) {
                const uint32_t x = src_count_le(s_oo + 1, span - 1, p);
                oo = s_oo[x];
                so = s_so[x];
                n = s_n[x];
                rp = s_rp[x];
            } else {
                src(x_lo + src_count_le(ooff + 1 + x_lo, span - 1, p), oo, so, n, rp);
            }
            const uint32_t i = p - oo;  // (below the source: wraps, never < n)
            at = so + i;
            left = i < n ? n - i : 0u;
            return i < n;
        };

        uint32_t c0[kSrcJ], c1[kSrcJ], e0[kSrcJ], e1[kSrcJ];
        bool m0[kSrcJ], m1[kSrcJ], v[kSrcJ];
#pragma unroll
        for (int j = 0; j < kSrcJ; ++j) {
            const uint32_t rel = 2u * ((uint32_t)j * kSrcNT + t);
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
        uint64_t k0[kSrcJ], k1[kSrcJ], n0[kSrcJ], n1[kSrcJ];
        uint32_t a0[kSrcJ], a1[kSrcJ];
#pragma unroll
        for (int j = 0; j < kSrcJ; ++j) {
            k0[j] = k1[j] = n0[j] = n1[j] = 0;
            a0[j] = a1[j] = 0;
            if (v[j]) {
                const SrcCols& b = tab[e0[j]];
                const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(b.keys + c0[j]);
                const ulonglong2 y = *reinterpret_cast<const ulonglong2*>(b.counters + c0[j]);
                const uint2 z = *reinterpret_cast<const uint2*>(b.actors + c0[j]);
                k0[j] = x.x;
                k1[j] = x.y;
                n0[j] = y.x;
                n1[j] = y.y;
                a0[j] = z.x;
                a1[j] = z.y;
            } else {
                if (m0[j]) {
                    const SrcCols& b = tab[e0[j]];
                    k0[j] = b.keys[c0[j]];
                    n0[j] = b.counters[c0[j]];
                    a0[j] = b.actors[c0[j]];
                }
                if (m1[j]) {
                    const SrcCols& b = tab[e1[j]];
                    k1[j] = b.keys[c1[j]];
                    n1[j] = b.counters[c1[j]];
                    a1[j] = b.actors[c1[j]];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kSrcJ; ++j) {
            const size_t p0 = (size_t)base + 2u * ((uint32_t)j * kSrcNT + t);
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
        // clocks: n_srcs x R words, one lane per word, from the source's replica
        const uint32_t R = s.R;
        const uint64_t nw = (uint64_t)n_srcs * R;
        for (uint64_t w = (uint64_t)blockIdx.x * kSrcNT + t; w < nw; w += (uint64_t)gridDim.x * kSrcNT) {
            const uint32_t x = (uint32_t)(w / R);
            const uint32_t r = (uint32_t)(w - (uint64_t)x * R);
            const uint32_t d = x / P, rp = x - d * P;
            s.out.vv[w] = tab_vv[rp][(size_t)d * R + r];
        }
    }
}

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static bool cols_aligned(const SrcCols& c) {
    return aligned(c.keys, 16) && aligned(c.counters, 16) && aligned(c.actors, 8);
}

// parts_e, parts_t: one workspace word each per kSrcScanChunk sources.
// n_docs == 0: only doc_srcs[0], entry_off[0] and tomb_off[0] (= 0) are written.
hipError_t launch_sources(const SourcesArgs& s, uint32_t* parts_e, uint32_t* parts_t, uint32_t* status, uint32_t n_cu,
                          hipStream_t stream) {
    const uint32_t n = s.n_srcs;
    const uint32_t n_parts = (uint32_t)(((uint64_t)n + kSrcScanChunk - 1) / kSrcScanChunk);
    hipError_t e = hipSuccess;
    if (n) {
        hipLaunchKernelGGL(sources_count_kernel, dim3(n_parts), dim3(kSrcNT), 0, stream, s, parts_e, parts_t, status);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(sources_partials_kernel, dim3(1), dim3(kSrcPartNT), 0, stream, parts_e, parts_t, n_parts,
                       s.entry_slots, s.tomb_slots, s.out.entry_off + n, s.out.tomb_off ? s.out.tomb_off + n : nullptr,
                       n ? nullptr : s.out.doc_srcs, status);
    if ((e = hipGetLastError()) != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(sources_emit_kernel, dim3(n_parts), dim3(kSrcNT), 0, stream, s, parts_e, parts_t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // bit 0: every replica's columns allow 16 B loads; bit 1: the output's allow 16 B stores
    bool vin_e = true, vin_t = true, any_t = false;
    for (uint32_t p = 0; p < s.n_reps; ++p) {
        vin_e = vin_e && cols_aligned(s.rep[p].e);
        if (s.rep[p].t.off) {
            any_t = true;
            vin_t = vin_t && cols_aligned(s.rep[p].t);
        }
    }
    const bool vout_e = aligned(s.out.keys, 16) && aligned(s.out.counters, 16) && aligned(s.out.actors, 8);
    hipLaunchKernelGGL(sources_gather_kernel<0>, dim3(n_cu * 8u), dim3(kSrcNT), 0, stream, s,
                       (vin_e ? 1u : 0u) | (vout_e ? 2u : 0u));
    if ((e = hipGetLastError()) != hipSuccess || !any_t) return e;
    const bool vout_t = aligned(s.out.tkeys, 16) && aligned(s.out.tcounters, 16) && aligned(s.out.tactors, 8);
    hipLaunchKernelGGL(sources_gather_kernel<1>, dim3(n_cu * 8u), dim3(kSrcNT), 0, stream, s,
                       (vin_t ? 1u : 0u) | (vout_t ? 2u : 0u));
    return hipGetLastError();
}

}  // namespace crdt
