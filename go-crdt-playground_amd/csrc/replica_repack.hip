// Replica repack with headroom (crdt_replica_repack_async; include/crdtgpu.h):
// replica select (sub == NULL) or replica scatter (replica.hip) writing a layout
// with spare slots.  Output document j copies ONE source document exactly as
// those calls do -- live entries, count, clock, live tombstones, actor -- but it
// owns cap(n) slots (headroom_cap, headroom.hpp: the one definition, shared with
// the host function crdt_headroom_capacity), n its live count; the entry policy
// and the tombstone policy are independent.  offsets are the exclusive prefix of
// the capacities, counts the live counts, and no slot at or past a document's
// live count is ever written.  With both policies packed every word written is
// the word launch_replica writes.
//
// replica.hip is left as it is (its kernels keep their resource figures), so the
// three-step scan and the gather are restated here over capacities, with this
// file's own constants (tests/replica_repack_cases.py mirrors them):
//
//   replica_fill_kernel, replica_map_kernel   scatter mapping only: the inverse
//       map, through launch_replica_map (replica.hpp).
//   repack_count_kernel      scan step 1: workgroup c sums the entry capacities and
//       the tombstone capacities of the kRpkScanChunk output documents of chunk c
//       into parts_e[c] and parts_t[c] (64-bit sums, stored modulo 2^32; a chunk
//       sum above the slots is kErrCapacity here).  Reports select's *n_idx clamp
//       and bad idx[j], live counts above their slots, and a capacity that
//       saturates (kErrCapacity).  Empty documents get cap(0).
//   repack_partials_kernel   step 2, one workgroup: both partial arrays become
//       their exclusive prefixes, kRpkPartStep per step; the running totals are
//       kept in 64 bits for the checks against entry_slots and tomb_slots; both
//       offsets[n_out] are written.
//   repack_emit_kernel       step 3: workgroup c rescans its chunk's capacities on
//       top of its partials and writes offsets, the LIVE counts and the actors.
//       No atomic and no look-back decides a position.
//   repack_gather_kernel<0>  The gather keeps the `sources` shape over OUTPUT
//       positions (the form chosen of the two the layout allows): the positions
//       [0, min(offsets[n_out], slots)) are cut into chunks of kRpkGatherChunk,
//       grid-stride; the documents of a chunk are found through the offsets just
//       written and staged in LDS (at most kRpkRun; beyond, lanes search the
//       offsets in global memory).  A position at or past its document's live
//       count lies in slack: its lane loads nothing and stores nothing.  A chunk
//       that lies wholly inside one document is resolved without staging, and
//       when it starts at or past that document's live count it is skipped
//       before any per-lane search.  A lane takes kRpkJ pairs of neighbouring
//       positions; a pair inside one live prefix at an even source index is read
//       with 16 B loads, any other element by element; all loads of a lane are
//       issued before its first store; the stores of a full pair are 16 B.  With
//       align >= 2 every document starts on an even position, so a pair never
//       straddles two documents and the 16 B store is the common path; at
//       align == 1 documents start at odd positions and their first and last
//       entries go element by element.  Then the clocks, one lane per actor.
//       The price of this form is that lanes are spent on slack (half of them at
//       doubling headroom); a second position space over live slots would not
//       spend them but needs a second scan and a second search per position.
//   repack_gather_kernel<1>  the same over the tombstones (launched when some
//       input replica has tombstones).
//
// Workspace: launch_replica's -- inv (scatter mapping), parts_e, parts_t.
#include "crdt_device.hpp"
#include "headroom.hpp"
#include "merge_block.hpp"
#include "replica.hpp"

namespace crdt {

constexpr int kRpkNT = 256;
constexpr int kRpkV = 4;                                 // documents per lane and scan chunk
constexpr uint32_t kRpkScanChunk = kRpkNT * kRpkV;       // 1,024 documents per scan workgroup
constexpr int kRpkPartNT = 1024;
constexpr uint32_t kRpkPartStep = kRpkPartNT;            // partials one step of the partials scan holds
constexpr int kRpkJ = 4;                                 // pairs of positions per lane and gather chunk
constexpr uint32_t kRpkGatherChunk = kRpkNT * kRpkJ * 2; // 2,048 output positions per gather step
constexpr uint32_t kRpkRun = 1024;                       // documents staged in LDS at most

// Number of elements of a[0..n) that are <= x (a non-decreasing; any a gives an index <= n).
__device__ __forceinline__ uint32_t rpk_count_le(const uint32_t* a, uint32_t n, uint32_t x) {
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

// Documents a select mapping takes (the rest of the n_out come out empty).
__device__ __forceinline__ uint32_t rpk_n_idx(const ReplicaArgs& s, uint32_t& err) {
    if (s.inv) return 0u;  // (scatter mapping: read by replica_map_kernel alone)
    uint32_t n = s.n_idx ? *s.n_idx : s.n_out;
    if (n > s.n_out) {
        err |= kErrCapacity;
        n = s.n_out;
    }
    return n;
}

// The source of output document j: false = empty; side 1 = sub; d its document there.
__device__ __forceinline__ bool rpk_pick(const ReplicaArgs& s, uint32_t j, uint32_t n_idx, uint32_t& side, uint32_t& d,
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

// Output document j: its live entry and tombstone counts (clamped to the source's
// slots) and its actor; the capacities follow from the counts alone.
__device__ __forceinline__ void rpk_live(const ReplicaArgs& s, uint32_t j, uint32_t n_idx, uint32_t& ne, uint32_t& nt,
                                         uint32_t& actor, uint32_t& err) {
    ne = nt = actor = 0;
    uint32_t side, d, o;
    if (rpk_pick(s, j, n_idx, side, d, err)) {
        const RepSide& r = side ? s.sub : s.rep;
        ne = r.e.off ? live_span(r.e.off, r.e.cnt, d, o, err) : 0u;
        nt = r.t.off ? live_span(r.t.off, r.t.cnt, d, o, err) : 0u;
        actor = r.doc_actor ? r.doc_actor[d] : r.actor;
    }
}

__global__ __launch_bounds__(kRpkNT) void repack_count_kernel(RepackArgs a, uint32_t* parts_e, uint32_t* parts_t,
                                                              uint32_t* status) {
    __shared__ unsigned long long s_sum[2];
    const ReplicaArgs& s = a.s;
    const uint32_t t = threadIdx.x, n = s.n_out;
    const uint32_t base = blockIdx.x * kRpkScanChunk;  // (< n: the grid is the number of chunks)
    const uint32_t m = min(kRpkScanChunk, n - base);
    const bool has_t = s.tout.offsets != nullptr;  // no tombstone output: no tombstone slots asked for
    if (t < 2) s_sum[t] = 0;
    __syncthreads();
    uint32_t err = 0;
    const uint32_t n_idx = rpk_n_idx(s, err);
    unsigned long long me = 0, mt = 0;
    bool sat = false;
#pragma unroll
    for (int k = 0; k < kRpkV; ++k) {
        const uint32_t i = (uint32_t)k * kRpkNT + t;
        if (i < m) {
            uint32_t ne, nt, actor;
            rpk_live(s, base + i, n_idx, ne, nt, actor, err);
            me += headroom_cap(a.er, ne, &sat);
            if (has_t) mt += headroom_cap(a.tr, nt, &sat);
        }
    }
    if (sat) err |= kErrCapacity;
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
        // (a sum that does not fit a word exceeds every slot count: reported here, and the
        // word stored keeps the offsets the prefix of the capacities modulo 2^32)
        if (se > (unsigned long long)s.entry_slots || st > (unsigned long long)s.tomb_slots) err |= kErrCapacity;
        parts_e[blockIdx.x] = (uint32_t)se;
        parts_t[blockIdx.x] = (uint32_t)st;
    }
    flag_error(status, err);
}

// One workgroup: parts[0..n_parts) -> exclusive prefixes (u32, as the offsets
// are); returns the u32 total, *over = the 64-bit total exceeds `slots`.
__device__ __forceinline__ uint32_t rpk_partials(uint32_t* parts, uint32_t n_parts, uint32_t slots, uint32_t* wave_tot,
                                                 unsigned long long* s_total, bool* over) {
    const uint32_t t = threadIdx.x;
    if (t == 0) *s_total = 0;
    unsigned long long mine = 0;  // (the u32 prefix may wrap on an output that cannot fit: detected here)
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_parts; base += kRpkPartStep) {
        const bool in = t < n_parts - base;
        const uint32_t v = in ? parts[base + t] : 0u;
        mine += v;
        uint32_t tot = 0;
        const uint32_t p = carry + block_exclusive_scan<kRpkPartNT>(v, wave_tot, &tot);
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
__global__ __launch_bounds__(kRpkPartNT) void repack_partials_kernel(uint32_t* parts_e, uint32_t* parts_t,
                                                                     uint32_t n_parts, uint32_t entry_slots,
                                                                     uint32_t tomb_slots, uint32_t* entry_total,
                                                                     uint32_t* tomb_total, uint32_t* status) {
    __shared__ uint32_t wave_tot[kRpkPartNT / 64];
    __shared__ unsigned long long s_total;
    bool over_e = false, over_t = false;
    const uint32_t te = rpk_partials(parts_e, n_parts, entry_slots, wave_tot, &s_total, &over_e);
    const uint32_t tt = rpk_partials(parts_t, n_parts, tomb_slots, wave_tot, &s_total, &over_t);
    uint32_t err = 0;
    if (threadIdx.x == 0) {
        *entry_total = te;
        if (tomb_total) *tomb_total = tt;
        if (over_e || over_t) err |= kErrCapacity;
    }
    flag_error(status, err);
}

__global__ __launch_bounds__(kRpkNT) void repack_emit_kernel(RepackArgs a, const uint32_t* parts_e,
                                                             const uint32_t* parts_t) {
    __shared__ uint32_t wave_tot[kRpkNT / 64];
    __shared__ uint32_t run_e[kRpkScanChunk];
    __shared__ uint32_t run_t[kRpkScanChunk];
    const ReplicaArgs& s = a.s;
    const uint32_t t = threadIdx.x, n = s.n_out;
    const uint32_t base = blockIdx.x * kRpkScanChunk;
    const uint32_t m = min(kRpkScanChunk, n - base);
    const bool has_t = s.tout.offsets != nullptr;
    uint32_t err = 0;  // (reported by repack_count_kernel)
    bool sat = false;
    const uint32_t n_idx = rpk_n_idx(s, err);
#pragma unroll
    for (int k = 0; k < kRpkV; ++k) {
        const uint32_t i = (uint32_t)k * kRpkNT + t;
        uint32_t ce = 0, ct = 0;
        if (i < m) {
            uint32_t ne, nt, actor;
            rpk_live(s, base + i, n_idx, ne, nt, actor, err);
            ce = headroom_cap(a.er, ne, &sat);
            if (has_t) ct = headroom_cap(a.tr, nt, &sat);
            s.out.counts[base + i] = ne;
            if (s.tout.counts) s.tout.counts[base + i] = nt;
            if (s.out_actor) s.out_actor[base + i] = actor;
        }
        run_e[i] = ce;
        run_t[i] = ct;
    }
    __syncthreads();
    uint32_t ve[kRpkV], vt[kRpkV], sum_e = 0, sum_t = 0;
#pragma unroll
    for (int k = 0; k < kRpkV; ++k) {
        ve[k] = run_e[t * kRpkV + k];
        vt[k] = run_t[t * kRpkV + k];
        sum_e += ve[k];
        sum_t += vt[k];
    }
    uint32_t tot = 0;
    uint32_t pe = parts_e[blockIdx.x] + block_exclusive_scan<kRpkNT>(sum_e, wave_tot, &tot);
    uint32_t pt = parts_t[blockIdx.x] + block_exclusive_scan<kRpkNT>(sum_t, wave_tot, &tot);
#pragma unroll
    for (int k = 0; k < kRpkV; ++k) {
        run_e[t * kRpkV + k] = pe;
        run_t[t * kRpkV + k] = pt;
        pe += ve[k];
        pt += vt[k];
    }
    __syncthreads();
    for (uint32_t i = t; i < m; i += kRpkNT) {
        s.out.offsets[base + i] = run_e[i];
        if (has_t) s.tout.offsets[base + i] = run_t[i];
    }
}

// KIND 0: the entries through out.offsets, then the clocks; KIND 1: the tombstones through tout.offsets.
template <int KIND>
__global__ __launch_bounds__(kRpkNT) void repack_gather_kernel(RepackArgs a, uint32_t vec) {
    __shared__ uint32_t s_oo[kRpkRun];  // output offset of the staged documents
    __shared__ uint32_t s_so[kRpkRun];  // slot offset of the source document each copies
    __shared__ uint32_t s_n[kRpkRun];   // live count
    __shared__ uint32_t s_sd[kRpkRun];  // 1: the source is the sub-replica
    const ReplicaArgs& s = a.s;
    const uint32_t t = threadIdx.x, n_out = s.n_out;
    const SrcCols c_rep = KIND ? s.rep.t : s.rep.e;
    const SrcCols c_sub = KIND ? s.sub.t : s.sub.e;
    const uint32_t* ooff = KIND ? s.tout.offsets : s.out.offsets;
    const uint32_t* ocnt = KIND ? s.tout.counts : s.out.counts;
    uint64_t* okeys = KIND ? s.tout.keys : s.out.keys;
    uint32_t* oactors = KIND ? s.tout.actors : s.out.actors;
    uint64_t* ocounters = KIND ? s.tout.counters : s.out.counters;
    uint32_t err = 0;  // (reported by repack_count_kernel)
    const uint32_t n_idx = rpk_n_idx(s, err);
    // nothing is written at or past the slots, whatever the scan found
    const uint32_t total = min(ooff[n_out], KIND ? s.tomb_slots : s.entry_slots);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)total + kRpkGatherChunk - 1) / kRpkGatherChunk);

    // output document j: its output offset, the side, slot offset and (clamped) live count of its source
    auto doc = [&](uint32_t j, uint32_t& oo, uint32_t& so, uint32_t& n, uint32_t& sd) {
        oo = ooff[j];
        n = ocnt[j];  // (the live count, clamped to the source's slots by repack_emit_kernel)
        so = 0;
        sd = 0;
        uint32_t d;
        if (n && rpk_pick(s, j, n_idx, sd, d, err)) {
            const uint32_t* off = sd ? c_sub.off : c_rep.off;
            so = off[d];  // (n != 0: this side has the columns)
        } else {
            n = 0;
        }
    };

    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t base = chunk * kRpkGatherChunk;
        const uint32_t m = min(kRpkGatherChunk, total - base);
        // Documents of the chunk's first and last position.  The search runs over
        // ooff[1 .. n_out), so whatever the offsets hold the answer is a document.
        const uint32_t j_lo = rpk_count_le(ooff + 1, n_out - 1, base);
        const uint32_t j_hi = j_lo + rpk_count_le(ooff + 1 + j_lo, n_out - 1 - j_lo, base + (m - 1));
        const uint32_t span = j_hi - j_lo + 1;
        const bool one = span == 1;  // the whole chunk lies in one document (uniform over the workgroup)
        const bool staged = !one && span <= kRpkRun;
        uint32_t one_oo = 0, one_so = 0, one_n = 0, one_sd = 0;
        if (one) {
            doc(j_lo, one_oo, one_so, one_n, one_sd);
            if (base - one_oo >= one_n) continue;  // wholly in slack (or below the document): nothing to write
        }
        if (staged) {
            for (uint32_t x = t; x < span; x += kRpkNT) {
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
            if (one) {
                oo = one_oo;
                so = one_so;
                n = one_n;
                sd = one_sd;
            } else if (staged) {
                const uint32_t x = rpk_count_le(s_oo + 1, span - 1, p);
                oo = s_oo[x];
                so = s_so[x];
                n = s_n[x];
                sd = s_sd[x];
            } else {
                doc(j_lo + rpk_count_le(ooff + 1 + j_lo, span - 1, p), oo, so, n, sd);
            }
            const uint32_t i = p - oo;  // (below the document: wraps, never < n)
            at = so + i;
            left = i < n ? n - i : 0u;
            return i < n;
        };

        uint32_t c0[kRpkJ], c1[kRpkJ], e0[kRpkJ], e1[kRpkJ];
        bool m0[kRpkJ], m1[kRpkJ], v[kRpkJ];
#pragma unroll
        for (int j = 0; j < kRpkJ; ++j) {
            const uint32_t rel = 2u * ((uint32_t)j * kRpkNT + t);
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
        uint64_t k0[kRpkJ], k1[kRpkJ], n0[kRpkJ], n1[kRpkJ];
        uint32_t a0[kRpkJ], a1[kRpkJ];
#pragma unroll
        for (int j = 0; j < kRpkJ; ++j) {
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
        for (int j = 0; j < kRpkJ; ++j) {
            const size_t p0 = (size_t)base + 2u * ((uint32_t)j * kRpkNT + t);
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
        for (uint64_t w = (uint64_t)blockIdx.x * kRpkNT + t; w < nw; w += (uint64_t)gridDim.x * kRpkNT) {
            const uint32_t j = (uint32_t)(w / R);
            const uint32_t r = (uint32_t)(w - (uint64_t)j * R);
            uint32_t side, d;
            uint64_t x = 0;
            if (rpk_pick(s, j, n_idx, side, d, err)) x = (side ? s.sub.vv : s.rep.vv)[(size_t)d * R + r];
            s.out.vv[w] = x;
        }
    }
}

static bool rpk_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static bool rpk_cols_aligned(const SrcCols& c) {
    return rpk_aligned(c.keys, 16) && rpk_aligned(c.counters, 16) && rpk_aligned(c.actors, 8);
}

hipError_t launch_replica_repack(const RepackArgs& ra, uint32_t* inv, uint32_t* parts_e, uint32_t* parts_t,
                                 uint32_t* status, uint32_t n_cu, hipStream_t stream) {
    const ReplicaArgs& a = ra.s;
    const uint32_t n = a.n_out;
    const uint32_t n_parts = (uint32_t)(((uint64_t)n + kRpkScanChunk - 1) / kRpkScanChunk);
    hipError_t e = hipSuccess;
    if (n) {
        if (inv && (e = launch_replica_map(a.idx, a.n_idx, a.sub.n_docs, n, inv, status, n_cu, stream)) != hipSuccess)
            return e;
        hipLaunchKernelGGL(repack_count_kernel, dim3(n_parts), dim3(kRpkNT), 0, stream, ra, parts_e, parts_t, status);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(repack_partials_kernel, dim3(1), dim3(kRpkPartNT), 0, stream, parts_e, parts_t, n_parts,
                       a.entry_slots, a.tomb_slots, a.out.offsets + n, a.tout.offsets ? a.tout.offsets + n : nullptr,
                       status);
    if ((e = hipGetLastError()) != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(repack_emit_kernel, dim3(n_parts), dim3(kRpkNT), 0, stream, ra, parts_e, parts_t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // bit 0: both sources' columns allow 16 B loads; bit 1: the output's allow 16 B stores
    const bool two = a.inv != nullptr;
    const bool vin_e = rpk_cols_aligned(a.rep.e) && (!two || rpk_cols_aligned(a.sub.e));
    const bool vout_e = rpk_aligned(a.out.keys, 16) && rpk_aligned(a.out.counters, 16) && rpk_aligned(a.out.actors, 8);
    hipLaunchKernelGGL(repack_gather_kernel<0>, dim3(n_cu * 8u), dim3(kRpkNT), 0, stream, ra,
                       (vin_e ? 1u : 0u) | (vout_e ? 2u : 0u));
    const bool any_t = a.rep.t.off || (two && a.sub.t.off);
    if ((e = hipGetLastError()) != hipSuccess || !any_t) return e;
    const bool vin_t = (!a.rep.t.off || rpk_cols_aligned(a.rep.t)) && (!two || !a.sub.t.off || rpk_cols_aligned(a.sub.t));
    const bool vout_t = rpk_aligned(a.tout.keys, 16) && rpk_aligned(a.tout.counters, 16) && rpk_aligned(a.tout.actors, 8);
    hipLaunchKernelGGL(repack_gather_kernel<1>, dim3(n_cu * 8u), dim3(kRpkNT), 0, stream, ra,
                       (vin_t ? 1u : 0u) | (vout_t ? 2u : 0u));
    return hipGetLastError();
}

}  // namespace crdt
