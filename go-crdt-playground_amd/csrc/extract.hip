// Batched delta extraction (crdt_awset_delta_extract_async): the sending half of
// delta-state replication.  Per source state s of doc d, against the clock P
// the peer's replica of d is known to have reached:
//
//   tombstones out = {(k,x) in Deleted : not (k in Entries and
//                     (e.actor != x.actor or e.counter > x.counter))}
//                                          MakeDeltaMergeData, awset-delta_test.go:93-102
//   FULL   P.Counter(src_actor[s]) == 0    first contact, :53: every entry
//   DELTA  otherwise: entries {(k,e) : !P.HasDot(e)}                  :84-92
//   NONE   a DELTA with nothing to send                               :60
//
// The message is a packed crdt_src_batch: its entry_off / tomb_off are the
// exclusive prefix sums of the kept counts over all sources, computed on the
// device in three launches (count -> scan -> emit, no host read-back):
//
//   extract_kernel<false>   counts what each group of documents keeps
//   extract_scan_kernel     one workgroup: exclusive scan of the group counts
//                           (the form of pack.hip's pack_scan_kernel)
//   extract_kernel<true>    the same walk again, now writing at the group's base
//
// The unit of work is a group of G = 64 / R consecutive documents per
// wavefront: lane j*R + r holds P[r] of the group's j-th document, so a dot's
// coverage is one cross-lane read, and the sources of the whole group -- one
// contiguous span of the entry arrays and one of the tombstone arrays -- are
// streamed in 64-lane chunks whatever the size of a single source (config 3:
// 4 documents x 10 sources x (8 + 2) = 400 elements per wavefront).  Each lane
// finds its source by a search over the group's entry_off values staged in
// LDS, kExSrcs sources at a time; a tombstone lane binary-searches its own
// source's sorted entry keys.  Survivors are compacted with ballot / below /
// popc, so entries and tombstones come out in key order.
#include "crdt_device.hpp"
#include "merge_block.hpp"

namespace crdt {

constexpr int kExWaves = 4;
constexpr uint32_t kExSrcs = 128;  // sources a wavefront stages at a time
constexpr int kExScanNT = 1024;
constexpr int kExScanV = 8;  // scan chunk = kExScanNT x kExScanV = 8,192 groups

constexpr uint32_t kExFull = 0x80000000u;

struct ExtractWaveSmem {
    uint32_t dsrc[kWave + 1];    // doc_srcs of the group's documents
    uint32_t eo[kExSrcs + 1];    // entry_off of the staged sources
    uint32_t to[kExSrcs + 1];    // tomb_off
    uint32_t oeo[kExSrcs + 1];   // entries the group kept before each staged source
    uint32_t oto[kExSrcs + 1];   // tombstones
    uint32_t flag[kExSrcs];      // lane of its document's P[0] | kExFull
};

// Number of elements of the non-decreasing a[0..n) that are <= x.
__device__ __forceinline__ uint32_t count_le(const uint32_t* a, uint32_t n, uint32_t x) {
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

// v of lane `src` (every lane of the wave takes part).
__device__ __forceinline__ uint64_t lane_read(uint64_t v, uint32_t src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}

// The staged sources' output offsets: a lane holding the first element of its
// source knows how many elements the group kept before it (`pos`); the empty
// sources just before that source start at the same place.
__device__ __forceinline__ void mark_first(uint32_t* oo, const uint32_t* io, uint32_t sl, uint32_t i, uint32_t pos) {
    uint32_t j = sl;
    for (;;) {
        oo[j] = pos;
        if (j == 0 || io[j - 1] != i) break;
        --j;
    }
}

template <bool EMIT>
__global__ __launch_bounds__(kExWaves * 64) void extract_kernel(SrcView sv, const uint64_t* peer, DeltaOutView out,
                                                               uint32_t G, uint32_t n_groups, uint32_t* gcnt_e,
                                                               uint32_t* gcnt_t, Work wk) {
    __shared__ ExtractWaveSmem smem[kExWaves];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    ExtractWaveSmem& sm = smem[w];
    const uint32_t R = sv.R, n_docs = sv.n_docs;
    const bool tombs = sv.tomb_off != nullptr;
    if (!gate_open(wk)) return;
    uint32_t err = 0;

    for (uint32_t g = uniform(blockIdx.x * kExWaves + w); g < n_groups; g += gridDim.x * kExWaves) {
        const uint32_t d0 = g * G, nd = min(G, n_docs - d0);
        const uint64_t P = lane < nd * R ? peer[(size_t)d0 * R + lane] : 0ull;
        if (lane < nd) sm.dsrc[lane] = sv.doc_srcs[d0 + lane];
        if (lane == 0) sm.dsrc[nd] = sv.doc_srcs[d0 + nd];
        wave_sync();
        if (EMIT && lane < nd) out.doc_srcs[d0 + lane] = sm.dsrc[lane];
        const uint32_t s_lo = uniform(sm.dsrc[0]), s_hi = uniform(sm.dsrc[nd]);
        const uint32_t gb_e = EMIT ? gcnt_e[g] : 0u, gb_t = EMIT ? gcnt_t[g] : 0u;
        uint32_t run_e = 0, run_t = 0;  // kept so far in this group

        for (uint32_t sb = s_lo; sb < s_hi; sb += kExSrcs) {
            const uint32_t nb = min(kExSrcs, s_hi - sb);
            // ---- stage the sources' bounds, document and path (FULL / DELTA)
            for (uint32_t i = lane; i <= nb; i += 64) {
                sm.eo[i] = sv.entry_off[sb + i];
                sm.to[i] = tombs ? sv.tomb_off[sb + i] : 0u;
            }
            for (uint32_t i0 = 0; i0 < nb; i0 += 64) {
                const uint32_t i = i0 + lane;
                const bool v = i < nb;
                const uint32_t s = sb + (v ? i : 0u);
                const uint32_t a = sv.src_actor[s];
                const uint32_t j = count_le(sm.dsrc + 1, nd, s);  // its document: dsrc[j] <= s < dsrc[j + 1]
                const uint32_t pl = min(j, nd - 1) * R;
                // Counter(src_actor) (crdt-misc.go:36-41): actor > R is 0, actor == R the panic
                const uint64_t p = lane_read(P, pl + (a < R ? a : 0u));
                const bool full = a >= R || p == 0ull;
                if (v) {
                    if (a == R) err |= kErrActorRange;
                    sm.flag[i] = pl | (full ? kExFull : 0u);
                    if (EMIT) out.src_actor[s] = a;
                }
            }
            wave_sync();
            // ---- entries
            const uint32_t e_lo = uniform(sm.eo[0]), e_hi = uniform(sm.eo[nb]);
            for (uint32_t base = e_lo; base < e_hi; base += 64) {
                const uint32_t i = base + lane;
                const bool v = i < e_hi;
                uint32_t a = 0, sl = 0;
                uint64_t c = 0, k = 0;
                if (v) {
                    a = sv.actors[i];
                    c = sv.counters[i];
                    if (EMIT) k = sv.keys[i];
                    sl = count_le(sm.eo, nb + 1, i) - 1;  // eo[sl] <= i < eo[sl + 1]
                }
                const uint32_t f = sm.flag[sl];
                const bool full = (f & kExFull) != 0u;
                const uint64_t p = lane_read(P, (f & ~kExFull) + (a < R ? a : 0u));
                const bool covered = a < R && p >= c;  // HasDot, crdt-misc.go:28-34
                if (v && !full && a == R) err |= kErrActorRange;  // (the FULL path tests no entry dot)
                const bool keep = v && (full || !covered);
                const uint64_t m = ballot(keep);
                if (EMIT) {
                    const uint32_t pos = run_e + below(m);
                    if (v && i == sm.eo[sl]) mark_first(sm.oeo, sm.eo, sl, i, pos);
                    if (keep) {
                        out.keys[gb_e + pos] = k;
                        out.actors[gb_e + pos] = a;
                        out.counters[gb_e + pos] = c;
                    }
                }
                run_e += popc(m);
            }
            // ---- tombstones: kept unless the key was added again (no clock filter)
            const uint32_t t_lo = uniform(sm.to[0]), t_hi = uniform(sm.to[nb]);
            for (uint32_t base = t_lo; base < t_hi; base += 64) {
                const uint32_t i = base + lane;
                const bool v = i < t_hi;
                uint32_t a = 0, sl = 0;
                uint64_t c = 0, k = 0;
                bool keep = false;
                if (v) {
                    k = sv.tkeys[i];
                    a = sv.tactors[i];
                    c = sv.tcounters[i];
                    sl = count_le(sm.to, nb + 1, i) - 1;
                    const uint32_t eb = sm.eo[sl], en = sm.eo[sl + 1] - eb;
                    const uint32_t q = lower_bound(sv.keys + eb, en, k);
                    bool again = false;
                    if (q < en && sv.keys[eb + q] == k) again = sv.actors[eb + q] != a || sv.counters[eb + q] > c;
                    keep = !again;
                }
                const uint64_t m = ballot(keep);
                if (EMIT) {
                    const uint32_t pos = run_t + below(m);
                    if (v && i == sm.to[sl]) mark_first(sm.oto, sm.to, sl, i, pos);
                    if (keep) {
                        out.tkeys[gb_t + pos] = k;
                        out.tactors[gb_t + pos] = a;
                        out.tcounters[gb_t + pos] = c;
                    }
                }
                run_t += popc(m);
            }
            if (EMIT) {
                // the empty sources at the end of the staged run, and its end
                for (uint32_t i = lane; i <= nb; i += 64) {
                    if (sm.eo[i] == e_hi) sm.oeo[i] = run_e;
                    if (sm.to[i] == t_hi) sm.oto[i] = run_t;
                }
                wave_sync();
                // ---- per source: packed offsets, kind, clock
                for (uint32_t i = lane; i < nb; i += 64) {
                    const uint32_t s = sb + i;
                    const uint32_t oe = sm.oeo[i], ot = sm.oto[i];
                    out.entry_off[s] = gb_e + oe;
                    if (out.tomb_off) out.tomb_off[s] = gb_t + ot;
                    if (out.kind) {
                        const bool any = sm.oeo[i + 1] != oe || sm.oto[i + 1] != ot;
                        out.kind[s] = (sm.flag[i] & kExFull) ? (uint8_t)CRDT_DELTA_FULL
                                                             : (any ? (uint8_t)CRDT_DELTA_DELTA : (uint8_t)CRDT_DELTA_NONE);
                    }
                }
                const size_t v0 = (size_t)sb * R;
                const uint32_t vn = nb * R;
                for (uint32_t x = lane; x < vn; x += 64) out.vv[v0 + x] = sv.vv[v0 + x];
            }
            wave_sync();  // (the staged arrays are reused by the next run of sources)
        }
        if (!EMIT && lane == 0) {
            gcnt_e[g] = run_e;
            gcnt_t[g] = run_t;
        }
        wave_sync();  // (dsrc is reused by the next group)
    }
    if (!EMIT) flag_error(wk.status, err);
}

// One workgroup: both count arrays (n groups each) become their exclusive
// prefixes in place, in chunks of kExScanNT x kExScanV groups as
// pack_scan_kernel does; the totals are the message's last offsets.  After a
// failed order check (host path) nothing was counted: every offset is 0.
__global__ __launch_bounds__(kExScanNT) void extract_scan_kernel(uint32_t* gcnt_e, uint32_t* gcnt_t, uint32_t n,
                                                                 const uint32_t* doc_srcs, uint32_t n_docs,
                                                                 DeltaOutView out, const uint32_t* gate) {
    constexpr uint32_t C = kExScanNT * kExScanV;
    __shared__ uint32_t wave_tot[kExScanNT / 64];
    __shared__ uint32_t run[C];
    const uint32_t t = threadIdx.x;
    const bool open = !gate || (*gate & kErrUnsorted) == 0u;
    const uint32_t n_srcs = doc_srcs[n_docs];
    for (uint32_t k = 0; k < 2; ++k) {
        uint32_t* cnt = k ? gcnt_t : gcnt_e;
        uint32_t carry = 0;
        for (uint32_t base = 0; base < n; base += C) {
            const uint32_t m = min(C, n - base);
            for (uint32_t i = t; i < C; i += kExScanNT) run[i] = (open && i < m) ? cnt[base + i] : 0u;
            __syncthreads();
            uint32_t v[kExScanV], sum = 0;
#pragma unroll
            for (int j = 0; j < kExScanV; ++j) {
                v[j] = run[t * kExScanV + j];
                sum += v[j];
            }
            uint32_t tot = 0;
            uint32_t p = carry + block_exclusive_scan<kExScanNT>(sum, wave_tot, &tot);
            // (the scan's barriers order every read of run above before these writes)
#pragma unroll
            for (int j = 0; j < kExScanV; ++j) {
                run[t * kExScanV + j] = p;
                p += v[j];
            }
            __syncthreads();
            for (uint32_t i = t; i < m; i += kExScanNT) cnt[base + i] = run[i];
            carry += tot;
            __syncthreads();  // (run and wave_tot are reused by the next chunk)
        }
        if (t == 0) {
            if (k == 0) {
                out.doc_srcs[n_docs] = n_srcs;
                out.entry_off[n_srcs] = carry;
            } else if (out.tomb_off) {
                out.tomb_off[n_srcs] = carry;
            }
        }
    }
}

// gcnt_e / gcnt_t: workspace, one word per group of 64 / R documents each (<= n_docs).
hipError_t launch_extract(const SrcView& sv, const uint64_t* peer, const DeltaOutView& out, uint32_t* gcnt_e,
                          uint32_t* gcnt_t, const Work& wk, uint32_t n_cu, hipStream_t stream) {
    const uint32_t G = 64u / sv.R;
    const uint32_t n_groups = (sv.n_docs + G - 1) / G;
    const uint32_t grid = min((n_groups + kExWaves - 1) / kExWaves, n_cu * 8u);
    if (n_groups) {
        hipLaunchKernelGGL((extract_kernel<false>), dim3(grid), dim3(kExWaves * 64), 0, stream, sv, peer, out, G,
                           n_groups, gcnt_e, gcnt_t, wk);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(extract_scan_kernel, dim3(1), dim3(kExScanNT), 0, stream, gcnt_e, gcnt_t, n_groups, sv.doc_srcs,
                       sv.n_docs, out, wk.gate);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_groups == 0) return e;
    hipLaunchKernelGGL((extract_kernel<true>), dim3(grid), dim3(kExWaves * 64), 0, stream, sv, peer, out, G, n_groups,
                       gcnt_e, gcnt_t, wk);
    return hipGetLastError();
}

}  // namespace crdt
