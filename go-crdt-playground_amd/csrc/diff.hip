// Merge diff on device-resident batches (crdt_awset_diff_async; include/crdtgpu.h):
// per document, the live entries of `before` whose key `after` no longer holds
// (removed: the reference's phase-2 `remove`, awset.go:145-158) and the live
// entries of `after` whose key `before` does not hold (added) or holds under
// another dot (updated) (awset.go:122-142), each list packed in key order with
// exclusive per-document offsets, plus CRDT_DIFF_* flags per document.
//
// Each list depends on one side's positions only: a position of `before` is
// removed iff its key is missing from after[d]; a position of `after` is
// upserted iff its key is missing from before[d] or found there under another
// dot.  So both lists come from one kernel form run over each side's slot space,
// and no merged order is needed.  Four launches, ordered by their kernel
// boundaries alone:
//
//   diff_init_kernel      one thread per document: fw[d] = 0 (the flag words the
//       count pass ORs into) and the live counts of both sides against their
//       slots (kErrCapacity; clamped everywhere below).
//   diff_count_kernel     the unit of work is the slot, not the document.  A
//       side's slot space [0, offsets[n_docs]) is cut into chunks of kDiffChunk
//       positions; the chunks are dealt in consecutive groups to at most
//       kDiffMaxParts workgroups per side (one group each: one chunk per
//       workgroup up to kDiffMaxParts chunks, more beyond), so the partial sums
//       fit a buffer of fixed size whatever the batch holds.  A chunk finds the
//       documents of its first and last position with a uniform search in the
//       offsets and stages them (own offset, own live count, the other side's
//       offset and live count) in LDS when they are at most kDiffRun; wider spans
//       (runs of empty documents) search the offsets in global memory.  A lane
//       takes kDiffJ positions, kDiffNT apart: its own keys are loaded first, then
//       the first probe of each -- the other side's key at the lane's own index
//       within the document -- then a galloping search from there (tile.hip,
//       merge_path_gallop's idea: two replicas of one document hold mostly the
//       same keys at mostly the same indices, so a converged document is answered
//       by the first probe), then the dots of the matched keys only.  The kept
//       count of the workgroup's chunks goes to parts[], the CRDT_DIFF_* bits are
//       ORed over the neighbouring lanes that hold one document (one atomicOr per
//       run) into fw[d].  Then the same kernel walks the n_docs x R clock words,
//       one lane per actor.
//   diff_partials_kernel  one workgroup: each side's partial sums become their
//       exclusive prefixes, kDiffPartStep per step; the running totals are kept in
//       64 bits for the check against rem_slots / ups_slots (kErrCapacity);
//       rem_off[n_docs], ups_off[n_docs] and summary[0..2] are written, and
//       summary[3..4] zeroed for the last pass.
//   diff_emit_kernel      the count pass again, chunk by chunk: the predicate is
//       recomputed, the survivors of a chunk are ranked by a block scan on top of
//       the workgroup's partial, and stored at their rank (contiguous, in key
//       order; nothing at or past the slots given).  The chunk that owns a
//       document's first slot position writes the document's offset: empty
//       documents and documents that are all slack share the rank before them;
//       documents that begin at the end of the slot space get the total.  Then
//       flags[d] = fw[d] and the summary's two document counts.
//
// No workgroup of any launch waits for a word another workgroup of the same
// launch writes: no look-back, no polling.  The lists are the same bits on every
// run: no atomic decides a position.
//
// Workspace: fw, one word per document; parts, 3 * kDiffMaxParts words.
#include "crdt_device.hpp"
#include "merge_block.hpp"

namespace crdt {

constexpr int kDiffNT = 256;
constexpr int kDiffJ = 4;                   // positions per lane and chunk
constexpr uint32_t kDiffChunk = 1024;       // slot positions per chunk
constexpr uint32_t kDiffRun = 1024;         // documents staged in LDS at most
constexpr uint32_t kDiffMaxParts = 2048;    // workgroups (and partial sums) per side at most
constexpr int kDiffPartNT = 1024;
constexpr uint32_t kDiffPartStep = 1024;    // partials one step of the partials scan holds
constexpr uint32_t kDiffVvChunk = 1024;     // clock words per workgroup step
constexpr uint32_t kDiffNoDoc = 0xFFFFFFFFu;
static_assert(kDiffChunk == (uint32_t)kDiffNT * kDiffJ, "a lane takes kDiffJ positions of a chunk");
static_assert(kDiffVvChunk == (uint32_t)kDiffNT * kDiffJ, "a lane takes kDiffJ clock words of a step");
static_assert(kDiffPartStep == (uint32_t)kDiffPartNT, "one partial per thread and step");

struct DiffArgs {
    BatchView before, after;
    uint32_t rem_slots, ups_slots;
    DiffOutView out;
};

// Number of elements of the non-decreasing a[0..n) that are <= x.
__device__ __forceinline__ uint32_t diff_count_le(const uint32_t* a, uint32_t n, uint32_t x) {
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

// Number of elements of the non-decreasing a[0..n) that are < x.
__device__ __forceinline__ uint32_t diff_count_lt(const uint32_t* a, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// How a side's slot space is cut up: chunks of kDiffChunk positions, dealt in
// groups of `group` consecutive chunks to n_parts <= kDiffMaxParts workgroups.
struct DiffGeo {
    uint32_t total, n_chunks, group, n_parts;
};

__device__ __forceinline__ DiffGeo diff_geo(const BatchView& v) {
    DiffGeo g;
    g.total = v.offsets[v.n_docs];
    g.n_chunks = (uint32_t)(((uint64_t)g.total + kDiffChunk - 1) / kDiffChunk);
    g.group = max(1u, (g.n_chunks + kDiffMaxParts - 1) / kDiffMaxParts);
    g.n_parts = (g.n_chunks + g.group - 1) / g.group;
    return g;
}

// Every lane of the wave holds (d, bits); lanes with the same d are neighbours.
// The first lane of each run ORs the run's bits into fw[d] (d == kDiffNoDoc: none).
__device__ __forceinline__ void diff_seg_or(uint32_t* fw, uint32_t d, uint32_t bits) {
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
    if (head && r && d != kDiffNoDoc) atomicOr(&fw[d], r);
}

// The index of key k in the strictly ascending y[0..n), n > 0: a galloping search
// from index g < n, whose key yk = y[g] the caller has loaded.  A hit at g costs
// nothing more; otherwise the step doubles away from g until it brackets k, and a
// bisection finishes: about twice a bisection's probes at worst.
__device__ __forceinline__ bool diff_find(const uint64_t* y, uint32_t n, uint32_t g, uint64_t yk, uint64_t k,
                                          uint32_t& r) {
    r = g;
    if (yk == k) return true;
    uint32_t lo, hi, step = 1;
    if (yk < k) {  // every y[< lo] < k
        lo = g + 1;
        hi = n;
        while (step != 0 && step <= hi - lo) {
            const uint32_t pr = lo + step - 1;
            if (y[pr] < k) {
                lo = pr + 1;
                step <<= 1;
            } else {
                hi = pr;
                break;
            }
        }
    } else {  // y[hi] >= k
        lo = 0;
        hi = g;
        while (step != 0 && step <= hi - lo) {
            const uint32_t pr = hi - step;
            if (y[pr] >= k) {
                hi = pr;
                step <<= 1;
            } else {
                lo = pr + 1;
                break;
            }
        }
    }
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (y[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    r = lo;
    return lo < n && y[lo] == k;
}

struct DiffSmem {
    uint32_t xo[kDiffRun];  // own-side offset of the staged documents
    uint32_t xn[kDiffRun];  // own-side live count
    uint32_t yo[kDiffRun];  // the other side's offset
    uint32_t yn[kDiffRun];  // the other side's live count
    uint32_t rank[kDiffChunk];
    uint32_t wave_tot[kDiffNT / 64];
    uint32_t upd;
};

// One chunk [base, base + m) of one side's slot space (AFTER: `after` against
// `before`, the upserts; else `before` against `after`, the removals).  Returns
// the number of kept positions.  !EMIT: also ORs the chunk's CRDT_DIFF_* bits
// into fw and adds its UPDATED records to upd.  EMIT: stores the kept entries at
// rank0 + their rank within the chunk, and the offsets of the documents whose
// first slot position lies in the chunk.  Called by every thread of the workgroup.
template <bool AFTER, bool EMIT>
__device__ __forceinline__ uint32_t diff_chunk(const DiffArgs& a, uint32_t base, uint32_t m, DiffSmem& sm, uint32_t* fw,
                                               uint32_t rank0, uint32_t& upd) {
    const BatchView& x = AFTER ? a.after : a.before;
    const BatchView& y = AFTER ? a.before : a.after;
    const uint32_t t = threadIdx.x, n_docs = x.n_docs;
    uint32_t err = 0;  // (reported by diff_init_kernel)
    // Documents of the chunk's first and last position.  The search runs over
    // offsets[1 .. n_docs), so whatever the offsets hold the answer is a document.
    const uint32_t d_lo = diff_count_le(x.offsets + 1, n_docs - 1, base);
    const uint32_t d_hi = d_lo + diff_count_le(x.offsets + 1 + d_lo, n_docs - 1 - d_lo, base + (m - 1));
    const uint32_t span = d_hi - d_lo + 1;
    const bool staged = span <= kDiffRun;
    if (staged) {
        for (uint32_t i = t; i < span; i += kDiffNT) {
            uint32_t xo, xn, yo, yn;
            xn = live_span(x.offsets, x.counts, d_lo + i, xo, err);
            yn = live_span(y.offsets, y.counts, d_lo + i, yo, err);
            sm.xo[i] = xo;
            sm.xn[i] = xn;
            sm.yo[i] = yo;
            sm.yn[i] = yn;
        }
        __syncthreads();
    }

    uint32_t dd[kDiffJ], yb[kDiffJ], ny[kDiffJ], gi[kDiffJ];
    bool live[kDiffJ];
    uint64_t k[kDiffJ], yk[kDiffJ];
    // own keys: every load of the lane before the first probe
#pragma unroll
    for (int j = 0; j < kDiffJ; ++j) {
        const uint32_t rel = (uint32_t)j * kDiffNT + t;
        dd[j] = kDiffNoDoc;
        yb[j] = ny[j] = gi[j] = 0;
        live[j] = false;
        k[j] = 0;
        if (rel < m) {
            const uint32_t p = base + rel;
            uint32_t xo, xn;
            if (staged) {
                const uint32_t i = diff_count_le(sm.xo + 1, span - 1, p);
                dd[j] = d_lo + i;
                xo = sm.xo[i];
                xn = sm.xn[i];
                yb[j] = sm.yo[i];
                ny[j] = sm.yn[i];
            } else {
                dd[j] = d_lo + diff_count_le(x.offsets + 1 + d_lo, span - 1, p);
                xn = live_span(x.offsets, x.counts, dd[j], xo, err);
                ny[j] = live_span(y.offsets, y.counts, dd[j], yb[j], err);
            }
            const uint32_t i = p - xo;  // (below the document: wraps, never < xn)
            live[j] = i < xn;
            gi[j] = ny[j] ? min(i, ny[j] - 1u) : 0u;
            if (live[j]) k[j] = x.keys[p];
        }
    }
    // first probes: the other side's key at the lane's own index
#pragma unroll
    for (int j = 0; j < kDiffJ; ++j) yk[j] = (live[j] && ny[j]) ? y.keys[(size_t)yb[j] + gi[j]] : 0ull;
    bool fnd[kDiffJ];
    uint32_t ri[kDiffJ];
#pragma unroll
    for (int j = 0; j < kDiffJ; ++j) {
        ri[j] = 0;
        fnd[j] = live[j] && ny[j] && diff_find(y.keys + yb[j], ny[j], gi[j], yk[j], k[j], ri[j]);
    }
    // dots: of the matched keys (the upserts' test), and of what is emitted
    const bool dots = EMIT && (AFTER ? a.out.ups_actors != nullptr : a.out.rem_actors != nullptr);
    bool keep[kDiffJ];
    uint32_t xa[kDiffJ];
    uint64_t xc[kDiffJ];
#pragma unroll
    for (int j = 0; j < kDiffJ; ++j) {
        const size_t p = (size_t)base + (uint32_t)j * kDiffNT + t;
        keep[j] = live[j] && !fnd[j];
        xa[j] = 0;
        xc[j] = 0;
        const bool need = AFTER ? (fnd[j] || (dots && live[j])) : (dots && keep[j]);
        if (need) {
            xa[j] = x.actors[p];
            xc[j] = x.counters[p];
        }
    }
    if (AFTER) {
        uint32_t ya[kDiffJ];
        uint64_t yc[kDiffJ];
#pragma unroll
        for (int j = 0; j < kDiffJ; ++j) {
            ya[j] = 0;
            yc[j] = 0;
            if (fnd[j]) {
                ya[j] = y.actors[(size_t)yb[j] + ri[j]];
                yc[j] = y.counters[(size_t)yb[j] + ri[j]];
            }
        }
#pragma unroll
        for (int j = 0; j < kDiffJ; ++j)
            if (fnd[j] && (xa[j] != ya[j] || xc[j] != yc[j])) keep[j] = true;
    }

    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < kDiffJ; ++j) cnt += keep[j] ? 1u : 0u;
    uint32_t tot = 0;
    if (!EMIT) {
#pragma unroll
        for (int j = 0; j < kDiffJ; ++j) {
            const uint32_t bits =
                !keep[j] ? 0u : (!AFTER ? CRDT_DIFF_REMOVED : (fnd[j] ? CRDT_DIFF_UPDATED : CRDT_DIFF_ADDED));
            diff_seg_or(fw, dd[j], bits);  // (the lanes of one j hold consecutive positions)
            if (AFTER && keep[j] && fnd[j]) ++upd;
        }
        (void)block_exclusive_scan<kDiffNT>(cnt, sm.wave_tot, &tot);
    } else {
        // rank in position order: position rel = j * kDiffNT + t, scanned kDiffJ per thread
#pragma unroll
        for (int j = 0; j < kDiffJ; ++j) sm.rank[(uint32_t)j * kDiffNT + t] = keep[j] ? 1u : 0u;
        __syncthreads();
        uint32_t v[kDiffJ], sum = 0;
#pragma unroll
        for (int j = 0; j < kDiffJ; ++j) {
            v[j] = sm.rank[t * kDiffJ + j];
            sum += v[j];
        }
        uint32_t p = block_exclusive_scan<kDiffNT>(sum, sm.wave_tot, &tot);
#pragma unroll
        for (int j = 0; j < kDiffJ; ++j) {
            sm.rank[t * kDiffJ + j] = p;  // (read above by this thread alone)
            p += v[j];
        }
        __syncthreads();
        const uint32_t slots = AFTER ? a.ups_slots : a.rem_slots;
        uint64_t* okeys = AFTER ? a.out.ups_keys : a.out.rem_keys;
        uint32_t* oact = AFTER ? a.out.ups_actors : a.out.rem_actors;
        uint64_t* octr = AFTER ? a.out.ups_counters : a.out.rem_counters;
#pragma unroll
        for (int j = 0; j < kDiffJ; ++j) {
            if (!keep[j]) continue;
            const uint32_t r = rank0 + sm.rank[(uint32_t)j * kDiffNT + t];
            if (r >= slots) continue;  // nothing is written at or past the slots given
            okeys[r] = k[j];
            if (dots) {
                oact[r] = xa[j];
                octr[r] = xc[j];
            }
            if (AFTER && a.out.ups_kind) a.out.ups_kind[r] = (uint8_t)(fnd[j] ? CRDT_DIFF_UPDATED : CRDT_DIFF_ADDED);
        }
        // the offsets of the documents whose first slot position lies in this chunk
        uint32_t* ooff = AFTER ? a.out.ups_off : a.out.rem_off;
        const uint32_t f_lo = diff_count_lt(x.offsets, n_docs, base);
        const uint32_t f_hi = f_lo + diff_count_lt(x.offsets + f_lo, n_docs - f_lo, base + m);
        for (uint32_t d = f_lo + t; d < f_hi; d += kDiffNT) {
            const uint32_t o = x.offsets[d] - base;
            if (o < m) ooff[d] = rank0 + sm.rank[o];
        }
    }
    __syncthreads();  // (the staged arrays and the ranks are reused by the next chunk)
    return tot;
}

__global__ __launch_bounds__(256) void diff_init_kernel(BatchView before, BatchView after, uint32_t* fw,
                                                        uint32_t* status, const uint32_t* gate) {
    if (gate && (*gate & kErrUnsorted) != 0u) return;  // the host path's order check failed (Work::gate)
    uint32_t err = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < before.n_docs; i += (uint64_t)gridDim.x * 256) {
        const uint32_t d = (uint32_t)i;
        uint32_t o;
        live_span(before.offsets, before.counts, d, o, err);
        live_span(after.offsets, after.counts, d, o, err);
        fw[d] = 0u;
    }
    flag_error(status, err);
}

// parts: [0, kDiffMaxParts) removed per workgroup of the `before` side,
// [kDiffMaxParts, 2 kDiffMaxParts) upserts per workgroup of the `after` side,
// [2 kDiffMaxParts, 3 kDiffMaxParts) the UPDATED among those.
__global__ __launch_bounds__(kDiffNT) void diff_count_kernel(DiffArgs a, uint32_t* fw, uint32_t* parts,
                                                             const uint32_t* gate) {
    __shared__ DiffSmem sm;
    if (gate && (*gate & kErrUnsorted) != 0u) return;
    const uint32_t t = threadIdx.x;
    const bool aft = blockIdx.x >= kDiffMaxParts;
    const uint32_t w = aft ? blockIdx.x - kDiffMaxParts : blockIdx.x;
    const DiffGeo g = diff_geo(aft ? a.after : a.before);
    if (w < g.n_parts) {  // (uniform over the workgroup)
        if (t == 0) sm.upd = 0;
        __syncthreads();
        uint32_t kept = 0, upd = 0;
        const uint32_t c_end = min(g.n_chunks, (w + 1u) * g.group);
        for (uint32_t c = w * g.group; c < c_end; ++c) {
            const uint32_t base = c * kDiffChunk;  // (base < total)
            const uint32_t m = min(kDiffChunk, g.total - base);
            kept += aft ? diff_chunk<true, false>(a, base, m, sm, fw, 0u, upd)
                        : diff_chunk<false, false>(a, base, m, sm, fw, 0u, upd);
        }
        if (aft) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) upd += (uint32_t)__shfl_xor((int)upd, o);
            if ((t & 63) == 0 && upd) atomicAdd(&sm.upd, upd);
            __syncthreads();
        }
        if (t == 0) {
            parts[blockIdx.x] = kept;
            if (aft) parts[2u * kDiffMaxParts + w] = sm.upd;
        }
    }

    // clocks: the n_docs x R words of both sides, one lane per actor
    const uint32_t R = a.before.R;
    const uint64_t nw = (uint64_t)a.before.n_docs * R;
    const uint64_t n_vc = (nw + kDiffVvChunk - 1) / kDiffVvChunk;
    for (uint64_t c = blockIdx.x; c < n_vc; c += gridDim.x) {
        uint64_t bv[kDiffJ], av[kDiffJ];
#pragma unroll
        for (int j = 0; j < kDiffJ; ++j) {
            const uint64_t i = c * kDiffVvChunk + (uint32_t)j * kDiffNT + t;
            bv[j] = i < nw ? a.before.vv[i] : 0ull;
            av[j] = i < nw ? a.after.vv[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < kDiffJ; ++j) {
            const uint64_t i = c * kDiffVvChunk + (uint32_t)j * kDiffNT + t;
            const uint32_t d = i < nw ? (uint32_t)(i / R) : kDiffNoDoc;
            diff_seg_or(fw, d, bv[j] != av[j] ? CRDT_DIFF_CLOCK : 0u);
        }
    }
}

// One workgroup: each side's parts -> exclusive prefixes (u32, as the offsets
// are), the totals checked in 64 bits against the slots given.
__global__ __launch_bounds__(kDiffPartNT) void diff_partials_kernel(DiffArgs a, uint32_t* parts, uint32_t* status,
                                                                    const uint32_t* gate) {
    __shared__ uint32_t wave_tot[kDiffPartNT / 64];
    __shared__ unsigned long long wave_sum[kDiffPartNT / 64];
    if (gate && (*gate & kErrUnsorted) != 0u) return;
    const uint32_t t = threadIdx.x, n_docs = a.before.n_docs;
    uint32_t err = 0;
    uint32_t totals[3] = {0, 0, 0};
    for (int side = 0; side < 3 && n_docs; ++side) {  // removed, upserts, the UPDATED among them (a sum only)
        const DiffGeo g = diff_geo(side == 0 ? a.before : a.after);
        uint32_t* ps = parts + (uint32_t)side * kDiffMaxParts;
        unsigned long long mine = 0;  // (a u32 prefix cannot wrap: a side keeps at most its 2^32 - 1 positions)
        uint32_t carry = 0;
        for (uint32_t base = 0; base < g.n_parts; base += kDiffPartStep) {
            const bool in = t < g.n_parts - base;
            const uint32_t v = in ? ps[base + t] : 0u;
            mine += v;
            uint32_t tot = 0;
            const uint32_t p = carry + block_exclusive_scan<kDiffPartNT>(v, wave_tot, &tot);
            if (in && side < 2) ps[base + t] = p;
            carry += tot;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
        if ((t & 63) == 0) wave_sum[t >> 6] = mine;
        __syncthreads();
        unsigned long long total = 0;
#pragma unroll
        for (int i = 0; i < kDiffPartNT / 64; ++i) total += wave_sum[i];
        __syncthreads();  // (wave_sum is reused by the next side)
        if (side < 2 && total > (unsigned long long)(side == 0 ? a.rem_slots : a.ups_slots)) err |= kErrCapacity;
        totals[side] = carry;
    }
    if (t == 0) {
        a.out.rem_off[n_docs] = totals[0];
        a.out.ups_off[n_docs] = totals[1];
        if (a.out.summary) {
            a.out.summary[0] = totals[0];
            a.out.summary[1] = totals[1];
            a.out.summary[2] = totals[2];
            a.out.summary[3] = 0u;
            a.out.summary[4] = 0u;
        }
    }
    flag_error(status, t == 0 ? err : 0u);
}

__global__ __launch_bounds__(kDiffNT) void diff_emit_kernel(DiffArgs a, const uint32_t* fw, const uint32_t* parts,
                                                            const uint32_t* gate) {
    __shared__ DiffSmem sm;
    if (gate && (*gate & kErrUnsorted) != 0u) return;
    const uint32_t t = threadIdx.x, n_docs = a.before.n_docs;
    const bool aft = blockIdx.x >= kDiffMaxParts;
    const uint32_t w = aft ? blockIdx.x - kDiffMaxParts : blockIdx.x;
    const DiffGeo g = diff_geo(aft ? a.after : a.before);
    if (w < g.n_parts) {  // (uniform over the workgroup)
        uint32_t rank = parts[blockIdx.x], upd = 0;
        const uint32_t c_end = min(g.n_chunks, (w + 1u) * g.group);
        for (uint32_t c = w * g.group; c < c_end; ++c) {
            const uint32_t base = c * kDiffChunk;
            const uint32_t m = min(kDiffChunk, g.total - base);
            rank += aft ? diff_chunk<true, true>(a, base, m, sm, nullptr, rank, upd)
                        : diff_chunk<false, true>(a, base, m, sm, nullptr, rank, upd);
        }
    }

    // per document: the final flags, the summary's document counts, and the
    // offsets of the documents no chunk owns (they begin at the end of the slot space)
    const uint32_t total_b = a.before.offsets[n_docs], total_a = a.after.offsets[n_docs];
    const uint32_t n_rem = a.out.rem_off[n_docs], n_ups = a.out.ups_off[n_docs];  // (diff_partials_kernel)
    uint32_t n_entry = 0, n_any = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kDiffNT + t; i < n_docs; i += (uint64_t)gridDim.x * kDiffNT) {
        const uint32_t d = (uint32_t)i;
        const uint32_t f = fw[d] & 15u;
        a.out.flags[d] = (uint8_t)f;
        n_entry += (f & (CRDT_DIFF_REMOVED | CRDT_DIFF_ADDED | CRDT_DIFF_UPDATED)) != 0u ? 1u : 0u;
        n_any += f != 0u ? 1u : 0u;
        if (a.before.offsets[d] >= total_b) a.out.rem_off[d] = n_rem;
        if (a.after.offsets[d] >= total_a) a.out.ups_off[d] = n_ups;
    }
    if (a.out.summary) {  // (integer sums: the same on every run)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n_entry += (uint32_t)__shfl_xor((int)n_entry, o);
            n_any += (uint32_t)__shfl_xor((int)n_any, o);
        }
        if ((t & 63) == 0) {
            if (n_entry) atomicAdd(&a.out.summary[3], n_entry);
            if (n_any) atomicAdd(&a.out.summary[4], n_any);
        }
    }
}

size_t diff_parts_bytes() { return (size_t)3 * kDiffMaxParts * sizeof(uint32_t); }

// fw: n_docs workspace words; parts: diff_parts_bytes().  n_docs == 0: only
// rem_off[0], ups_off[0] and the summary are written.
hipError_t launch_diff(const BatchView& before, const BatchView& after, uint32_t rem_slots, uint32_t ups_slots,
                       const DiffOutView& out, uint32_t* fw, uint32_t* parts, uint32_t* status, const uint32_t* gate,
                       uint32_t n_cu, hipStream_t stream) {
    const DiffArgs a{before, after, rem_slots, ups_slots, out};
    const uint32_t n = before.n_docs;
    hipError_t e = hipSuccess;
    if (n) {
        const uint32_t igrid = min((n + 255u) / 256u, n_cu * 8u);
        hipLaunchKernelGGL(diff_init_kernel, dim3(igrid), dim3(256), 0, stream, before, after, fw, status, gate);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(diff_count_kernel, dim3(2u * kDiffMaxParts), dim3(kDiffNT), 0, stream, a, fw, parts, gate);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(diff_partials_kernel, dim3(1), dim3(kDiffPartNT), 0, stream, a, parts, status, gate);
    if ((e = hipGetLastError()) != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(diff_emit_kernel, dim3(2u * kDiffMaxParts), dim3(kDiffNT), 0, stream, a, fw, parts, gate);
    return hipGetLastError();
}

}  // namespace crdt
