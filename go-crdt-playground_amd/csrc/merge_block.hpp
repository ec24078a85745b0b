// Block-level merge of one large document: dst <- src (+ tombstones).
//
// One workgroup of NT threads walks the two sorted entry lists with a
// merge-path window of T = NT*IPT merged positions per iteration.  Each thread
// finds its own diagonal split inside the LDS windows, decides IPT union keys
// with the per-key rule (DESIGN.md "Per-key rule"), and the workgroup scans the
// kept counts to place the survivors contiguously in key order.
//
// The walk exists once (merge_walk).  What it writes is its sink's business:
// block_merge places the survivors (KeepSink: join.hip, fold.hip, delta_pair.hip);
// the logged merges add the removed and upserted records beside them (LogSink,
// merge_log.hpp: join_log.hip, delta_pair_log.hip).  The file also holds what the block kernels share around
// the walk: the worklist loop (for_each_work), the test whether a delta source
// changes anything (delta_changes) and the ordered fold of one worklist document
// (fold_block_doc: fold.hip, fold_log.hip).
//
// The rule (union key k, dst dot d if present, src dot s if present):
//   changed  = has_s && (full || !dstVV.HasDot(s))   awset-delta_test.go:84-92
//   has_d && has_s : present, dot = changed ? s : d   awset.go:123-129,142
//   has_d only     : present = full ? !srcVV.HasDot(d) : true      awset.go:146-158
//   has_s only     : present = changed && !dstVV.HasDot(s)         awset.go:133-140
//   delta mode, present, k in src.Deleted as x and x "effective"
//   (not re-added, awset-delta_test.go:93-102): present = dstVV.HasDot(x)
//                                                     awset-delta_test.go:149-164
#pragma once

#include "crdt_device.hpp"

namespace crdt {

template <int NT, int IPT>
struct MergeSmem {
    static constexpr int T = NT * IPT;
    uint64_t dk[T];
    uint64_t dc[T];
    uint64_t sk[T];
    uint64_t sc[T];
    uint32_t da[T];
    uint32_t sa[T];
    uint64_t dvv[CRDT_MAX_R];
    uint64_t svv[CRDT_MAX_R];
    uint32_t wave_tot[NT / 64];
    uint32_t word[4];
};

struct Entries {
    const uint64_t* k;
    const uint32_t* a;
    const uint64_t* c;
    uint32_t n;
};

struct EntriesOut {
    uint64_t* k;
    uint32_t* a;
    uint64_t* c;
};

// # of dst elements among the first k merged (dst first on equal keys).
__device__ __forceinline__ uint32_t merge_path(const uint64_t* dk, uint32_t nd, const uint64_t* sk, uint32_t ns,
                                               uint32_t k) {
    uint32_t lo = k > ns ? k - ns : 0;
    uint32_t hi = k < nd ? k : nd;
    while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        if (dk[mid] <= sk[k - 1 - mid])
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Tombstone probe for delta mode: returns true and (xa, xc) when key is in t.
__device__ __forceinline__ bool tomb_find(const Entries& t, uint64_t key, uint32_t& xa, uint64_t& xc) {
    if (t.n == 0) return false;
    uint32_t h = lower_bound(t.k, t.n, key);
    if (h < t.n && t.k[h] == key) {
        xa = t.a[h];
        xc = t.c[h];
        return true;
    }
    return false;
}

// Per-key rule shared by every path.  Returns whether the key survives and its dot.
__device__ __forceinline__ bool decide(bool has_d, uint32_t d_a, uint64_t d_c, bool has_s, uint32_t s_a, uint64_t s_c,
                                       bool full, const uint64_t* dvv, const uint64_t* svv, uint32_t R,
                                       const Entries& tomb, uint64_t key, uint32_t& o_a, uint64_t& o_c,
                                       uint32_t& err) {
    const bool changed = has_s && (full || !has_dot(dvv, R, s_a, s_c, err));
    bool present;
    if (has_d) {
        present = has_s ? true : (full ? !has_dot(svv, R, d_a, d_c, err) : true);
        const bool take_s = has_s && changed;
        o_a = take_s ? s_a : d_a;
        o_c = take_s ? s_c : d_c;
    } else {
        present = changed && !has_dot(dvv, R, s_a, s_c, err);
        o_a = s_a;
        o_c = s_c;
    }
    if (!full && present) {
        uint32_t xa;
        uint64_t xc;
        if (tomb_find(tomb, key, xa, xc)) {
            const bool readded = has_s && (s_a != xa || s_c > xc);
            if (!readded) present = has_dot(dvv, R, xa, xc, err);
        }
    }
    return present;
}

// Block-wide exclusive scan of v (per thread); returns exclusive prefix, total in *tot.
template <int NT>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wave_tot, uint32_t* tot) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t y = __shfl_up(x, o);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) wave_tot[w] = x;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        uint32_t t = wave_tot[i];
        base += (i < (int)w) ? t : 0u;
        all += t;
    }
    __syncthreads();
    *tot = all;
    return base + x - v;
}

// What decide() made of one merged position of the window walk.  A keep / drop
// sink reads kPosKeep alone; the logged join's sink (join_log.hip) reads all four.
constexpr uint8_t kPosKeep = 1;  // survives, with the merged dot
constexpr uint8_t kPosRem = 2;   // a dst entry the merge dropped
constexpr uint8_t kPosAdd = 4;   // a src-only key the merge kept
constexpr uint8_t kPosUpd = 8;   // a common key whose dot the merge changed

__device__ __forceinline__ void put_entry(const EntriesOut& e, uint32_t p, uint64_t k, uint32_t a, uint64_t c) {
    e.k[p] = k;
    e.a[p] = a;
    e.c[p] = c;
}

// The keep / drop sink: the survivors, contiguous in key order.
struct KeepSink {
    static constexpr bool kLog = false;
    EntriesOut out;
    uint32_t o;  // survivors written so far

    // One window: thread-local classes and records of IPT positions -> one block scan, the stores.
    template <int NT, int IPT>
    __device__ __forceinline__ void place(const uint8_t (&cls)[IPT], const uint64_t (&ok)[IPT],
                                          const uint32_t (&oa)[IPT], const uint64_t (&oc)[IPT], uint32_t* wave_tot) {
        uint32_t cnt = 0;
#pragma unroll
        for (int q = 0; q < IPT; ++q) cnt += (cls[q] & kPosKeep) ? 1u : 0u;
        uint32_t total;
        uint32_t pos = o + block_exclusive_scan<NT>(cnt, wave_tot, &total);
#pragma unroll
        for (int q = 0; q < IPT; ++q)
            if (cls[q] & kPosKeep) put_entry(out, pos++, ok[q], oa[q], oc[q]);
        o += total;
    }
};

// The merge-path window walk of one document, dst <- src (+ tombstones), by the
// whole workgroup.  sm.dvv / sm.svv must hold the two version vectors.  Each
// window's positions are classified (kPos*) and handed to sink.place with the key
// and the dot their record carries: the merged dot of a survivor, and of a dropped
// dst entry its own (a logging sink is handed dst's dot even where delta mode moved
// the common key to src's dot before a tombstone dropped it).
//
// A common key is classified where its dst entry is taken, which always sees the
// src entry (the src window reaches a whole window ahead), so a pair that
// straddles a window boundary is kept, UPDATED or dropped exactly once; the src
// entry is skipped in the next window by prev_dk.
//
// DIFF: the same walk as a comparison of two states, D the one before and S the
// one after (diff_walk, merge_log.hpp): no rule and no clock is asked.  A common
// key is kept with S's dot (UPDATED when it differs from D's), a D-only key is
// dropped and an S-only key kept.
//
// (Not __forceinline__, like block_merge: inlined early, the walk costs the keep /
// drop kernels 20 to 30 VGPRs; the callers that pop the worklist are forced
// instead, so that no kernel ends up with a call.)
template <int NT, int IPT, class Sink, bool DIFF = false>
__device__ void merge_walk(const Entries& D, const Entries& S, const Entries& tomb, bool full,
                                           uint32_t R, MergeSmem<NT, IPT>& sm, Sink& sink, uint32_t& err) {
    constexpr uint32_t T = NT * IPT;
    const uint32_t tid = threadIdx.x;
    uint32_t i = 0, j = 0;
    while (i < D.n || j < S.n) {
        const uint32_t nd = min(T, D.n - i), ns = min(T, S.n - j);
        const uint32_t K = min(T, nd + ns);
        for (uint32_t t = tid; t < nd; t += NT) {
            sm.dk[t] = D.k[i + t];
            sm.da[t] = D.a[i + t];
            sm.dc[t] = D.c[i + t];
        }
        for (uint32_t t = tid; t < ns; t += NT) {
            sm.sk[t] = S.k[j + t];
            sm.sa[t] = S.a[j + t];
            sm.sc[t] = S.c[j + t];
        }
        const bool has_prev = i > 0;
        const uint64_t prev_dk = has_prev ? D.k[i - 1] : 0ull;
        __syncthreads();

        const uint32_t k0 = min(tid * IPT, K), k1 = min(k0 + IPT, K);
        uint32_t a = merge_path(sm.dk, nd, sm.sk, ns, k0);
        uint32_t b = k0 - a;

        uint64_t ok[IPT];
        uint32_t oa[IPT];
        uint64_t oc[IPT];
        uint8_t cls[IPT];
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
            cls[q] = 0;
            ok[q] = 0;
            oa[q] = 0;
            oc[q] = 0;
            if (k0 + q < k1) {
                const bool take_d = (a < nd) && (b >= ns || sm.dk[a] <= sm.sk[b]);
                if (take_d) {
                    const uint64_t key = sm.dk[a];
                    // (b < ns whenever src has an entry left: the src window reaches T entries ahead)
                    const bool match = (b < ns) && sm.sk[b] == key;
                    const uint32_t d_a = sm.da[a], s_a = match ? sm.sa[b] : 0u;
                    const uint64_t d_c = sm.dc[a], s_c = match ? sm.sc[b] : 0ull;
                    bool kp;
                    if constexpr (DIFF) {
                        kp = match;
                        oa[q] = s_a;
                        oc[q] = s_c;
                    } else {
                        kp = decide(true, d_a, d_c, match, s_a, s_c, full, sm.dvv, sm.svv, R, tomb, key, oa[q], oc[q],
                                    err);
                    }
                    ok[q] = key;
                    cls[q] = kp ? kPosKeep : kPosRem;
                    if (Sink::kLog) {
                        // UPDATED only on a kept key; a dropped entry's record carries dst's own dot.
                        // (Delta mode can move a common key to src's dot and then drop it by a
                        // tombstone; in full mode a common key is never dropped.)
                        if (kp && match && (oa[q] != d_a || oc[q] != d_c)) cls[q] |= kPosUpd;
                        if (!kp) {
                            oa[q] = d_a;
                            oc[q] = d_c;
                        }
                    }
                    ++a;
                } else {
                    const uint64_t key = sm.sk[b];
                    const bool match = (a > 0) ? (sm.dk[a - 1] == key) : (has_prev && prev_dk == key);
                    if (!match) {
                        bool kp;
                        if constexpr (DIFF) {
                            kp = true;
                            oa[q] = sm.sa[b];
                            oc[q] = sm.sc[b];
                        } else {
                            kp = decide(false, 0u, 0ull, true, sm.sa[b], sm.sc[b], full, sm.dvv, sm.svv, R, tomb, key,
                                        oa[q], oc[q], err);
                        }
                        ok[q] = key;
                        cls[q] = kp ? (kPosKeep | kPosAdd) : 0;
                    }
                    ++b;
                }
            }
        }
        sink.template place<NT, IPT>(cls, ok, oa, oc, sm.wave_tot);
        const uint32_t aK = merge_path(sm.dk, nd, sm.sk, ns, K);
        i += aK;
        j += K - aK;
        __syncthreads();
    }
}

// Merge one document, keep / drop.  Returns the number of entries written to out.
template <int NT, int IPT>
__device__ uint32_t block_merge(const Entries& D, const Entries& S, const Entries& tomb, bool full, uint32_t R,
                                MergeSmem<NT, IPT>& sm, const EntriesOut& out, uint32_t& err) {
    KeepSink sink{out, 0u};
    merge_walk<NT, IPT>(D, S, tomb, full, R, sm, sink, err);
    return sink.o;
}

// Does a delta source (entries S, tombstones T) change a dst whose clock is dvv:
// some entry has a dot dst has not seen (changed, awset-delta_test.go:84-92) or
// some tombstone passes the re-add filter (:93-102).  The whole workgroup calls it.
template <int NT>
__device__ __forceinline__ bool delta_changes(const Entries& S, const Entries& T, const uint64_t* dvv, uint32_t R,
                                              uint32_t& err) {
    const uint32_t tid = threadIdx.x;
    bool any = false;
    for (uint32_t e = tid; e < S.n; e += NT) any |= !has_dot(dvv, R, S.a[e], S.c[e], err);
    for (uint32_t t = tid; t < T.n; t += NT) {
        uint32_t ea;
        uint64_t ec;
        const bool readded = tomb_find(S, T.k[t], ea, ec) && (ea != T.a[t] || ec > T.c[t]);
        any |= !readded;
    }
    return __syncthreads_or(any) != 0;
}

// The ordered fold of one worklist document by the whole workgroup (fold.hip,
// fold_log.hip): every source of d merged into it in turn, one window walk per
// step, ping-ponging between the output slots and the context's scratch copy
// of them, so that out holds the result once the last step is done.  Returns
// the live entries written to out (and leaves the merged clock in sm.dvv), or
// kFoldNoDoc when the scratch is too small for the document (kErrWorkspace:
// nothing of d is written).  An actor-range error is left in err; the other
// reports go to wk.status directly.
constexpr uint32_t kFoldNoDoc = 0xFFFFFFFFu;

template <int NT, int IPT>
__device__ __forceinline__ uint32_t fold_block_doc(int mode, const BatchView& dst, const SrcView& sb,
                                                   const OutView& out, const Scratch& scr, const Work& wk,
                                                   uint32_t d, MergeSmem<NT, IPT>& sm, uint32_t& err) {
    const uint32_t tid = threadIdx.x;
    const uint32_t R = dst.R;
    const uint32_t s0 = sb.doc_srcs[d], s1 = sb.doc_srcs[d + 1];
    const uint32_t doff = dst.offsets[d];
    const uint32_t dslots = dst.offsets[d + 1] - doff;
    const uint32_t obase = doff + sb.entry_off[s0];
    const uint64_t cap = (uint64_t)dslots + (sb.entry_off[s1] - sb.entry_off[s0]);
    if ((uint64_t)obase + cap > scr.slots) {  // crdt_ctx_reserve was not told enough slots
        if (tid == 0) atomicOr(wk.status, kErrWorkspace);
        __syncthreads();
        return kFoldNoDoc;
    }
    const EntriesOut O{out.keys + obase, out.actors + obase, out.counters + obase};
    const EntriesOut X{scr.keys + obase, scr.actors + obase, scr.counters + obase};
    const uint32_t live = live_count(dst.offsets, dst.counts, d);
    if (live > dslots && tid == 0) atomicOr(wk.status, kErrCapacity);
    Entries cur{dst.keys + doff, dst.actors + doff, dst.counters + doff, live < dslots ? live : dslots};
    int where = 0;  // 0 = input, 1 = out, 2 = scratch
    if (tid < R) sm.dvv[tid] = dst.vv[(size_t)d * R + tid];
    __syncthreads();
    bool stop = false;
    for (uint32_t k = s0; k < s1 && !stop; ++k) {
        const uint32_t e0 = sb.entry_off[k];
        const Entries S{sb.keys + e0, sb.actors + e0, sb.counters + e0, sb.entry_off[k + 1] - e0};
        Entries Tm{nullptr, nullptr, nullptr, 0};
        if (sb.tomb_off && mode == CRDT_FOLD_DELTA) {
            const uint32_t t0 = sb.tomb_off[k];
            Tm = Entries{sb.tkeys + t0, sb.tactors + t0, sb.tcounters + t0, sb.tomb_off[k + 1] - t0};
        }
        if (tid < R) sm.svv[tid] = sb.vv[(size_t)k * R + tid];
        __syncthreads();
        uint32_t perr = 0;
        const bool full = (mode != CRDT_FOLD_DELTA) || vv_counter(sm.dvv, R, sb.src_actor[k], perr) == 0;
        if (perr) {
            err |= perr;
            stop = true;
            break;
        }
        if (!full && !delta_changes<NT>(S, Tm, sm.dvv, R, err)) continue;
        const EntriesOut& tgt = (where == 1) ? X : O;
        const uint32_t n = block_merge<NT, IPT>(cur, S, full ? Entries{nullptr, nullptr, nullptr, 0} : Tm, full, R, sm,
                                                tgt, err);
        if (tid < R) sm.dvv[tid] = max(sm.dvv[tid], sm.svv[tid]);
        where = (where == 1) ? 2 : 1;
        cur = Entries{tgt.k, tgt.a, tgt.c, n};
        __syncthreads();
    }
    if (where != 1) {  // result still in the input or the scratch copy
        for (uint32_t i = tid; i < cur.n; i += NT) {
            O.k[i] = cur.k[i];
            O.a[i] = cur.a[i];
            O.c[i] = cur.c[i];
        }
    }
    if (tid == 0) out.counts[d] = cur.n;
    if (tid < R) out.vv[(size_t)d * R + tid] = sm.dvv[tid];
    __syncthreads();
    return cur.n;
}

// The block path's worklist: workgroups pop documents from head word `head` of
// wk.wl_head (the exchange of join.hip runs the list twice, once per direction)
// until the list the previous launch filled is empty, and call body(d) for each.
// `word` is one LDS word.  An entry that is not a document of this call is never
// dereferenced (kErrWorkspace).
template <class Body>
__device__ __forceinline__ void for_each_work(const Work& wk, uint32_t head, uint32_t n_docs, uint32_t* word,
                                              Body&& body) {
    if (work_total(wk, n_docs) == 0) return;  // empty worklist: no dispensing atomics
    for (;;) {
        if (threadIdx.x == 0) *word = atomicAdd(wk.wl_head + head, 1u);
        __syncthreads();
        const uint32_t slot = *word;
        const uint32_t total = work_total(wk, n_docs);
        __syncthreads();
        if (slot >= total) break;
        const uint32_t d = wk.worklist[slot];
        if (d >= n_docs) {
            if (threadIdx.x == 0) atomicOr(wk.status, kErrWorkspace);
            continue;
        }
        body(d);
    }
}

}  // namespace crdt
