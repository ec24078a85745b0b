// Logged join and exchange: out[d] = dst[d] <- src[d] as join.hip writes it
// (awset.go:103-161), and beside it the merge's decision log (awset.go:109-158)
// in structured form: the dst entries the merge removed and the src entries it
// added or moved a common key to.  The kernels that write the merged state have
// made each of those decisions already, so the log costs no second read of the
// batches and no search: it is crdt_awset_diff_async(dst, out)'s answer, laid
// out by the inputs' own slot bounds (a removed entry was a dst entry, so
// document d's removed list starts at dst.offsets[d]; an upserted entry was a
// src entry, so its list starts at src.offsets[d]) and therefore written with
// no scan over documents.
//
// The per-key rule is decide() of merge_block.hpp with full = true.  From its
// answer for one union key (dst dot d, src dot s):
//   dst-only and dropped        removed, with d        (the log's `remove`)
//   src-only and kept           upserted ADDED, with s (`add`)
//   common and the dot changes  upserted UPDATED, with s (`update`)
//
// Two paths, one launch each, dispatched as delta_pair.hip does:
//  * join_log_wave_kernel: one wavefront per document when both sides hold
//    <= 64 live entries, kLogDocs documents in turn per wave.  Both entry lists
//    and both clocks are staged in LDS once; lane i owns entry i of each side
//    and finds its key on the other side by LDS binary search.  Every position
//    is a ballot and a popcount: the survivor's slot as in join_wave_kernel,
//    the removed rank over the dst lanes, the upsert rank over the src lanes.
//    The exchange decides both directions from the one staging.
//  * join_log_block_kernel: workgroups pop the worklist; per direction the
//    merge-path window walk of block_merge (merge_block.hpp), carrying three
//    running offsets (survivors, removed, upserted) from three block scans per
//    window.  A common key is classified where its dst entry is taken, which
//    always sees the src entry (the src window reaches a whole window ahead),
//    so a pair that straddles a window boundary is UPDATED (or unchanged)
//    exactly once; the src entry is skipped in the next window by prev_dk.
//
// No atomic decides a position.  The summary is summed with integer atomics
// over kLogParts spread rows of partial sums (the context's partials buffer,
// zeroed by a kernel first) and reduced by join_log_summary_kernel.
#include "crdt_device.hpp"
#include "merge_block.hpp"

namespace crdt {

constexpr int kLogWaves = 4;       // wavefronts per workgroup of the wave path
constexpr int kLogDocs = 8;        // documents one wavefront takes in turn
constexpr int kLogWaveMax = 64;    // live entries per side the wave path takes
constexpr int kLogBlockNT = 256;   // block path: threads per workgroup
constexpr int kLogBlockIPT = 4;    // block path: merged positions per thread and window
constexpr uint32_t kLogParts = 1024;  // rows of summary partial sums per direction
constexpr uint32_t kLogPartRow = 8;   // words per row (5 used)

size_t join_log_parts_bytes() { return (size_t)2 * kLogParts * kLogPartRow * sizeof(uint32_t); }

// Live prefix of document d: its first slot in o0, its length returned, clamped
// to the document's slots (kErrCapacity).
__device__ __forceinline__ uint32_t log_live(const uint32_t* offsets, const uint32_t* counts, uint32_t d, uint32_t& o0,
                                             uint32_t& err) {
    o0 = offsets[d];
    const uint32_t slots = offsets[d + 1] - o0;
    uint32_t n = counts ? counts[d] : slots;
    if (n > slots) {
        n = slots;
        err |= kErrCapacity;
    }
    return n;
}

// crdt_diff_out.summary of one direction, summed over the documents a wave or a
// workgroup has merged.
struct LogSums {
    uint32_t v[5];
};

__device__ __forceinline__ void sums_add(LogSums& s, uint32_t n_rem, uint32_t n_ups, uint32_t n_upd, uint32_t flags) {
    s.v[0] += n_rem;
    s.v[1] += n_ups;
    s.v[2] += n_upd;
    s.v[3] += (flags & 7u) ? 1u : 0u;
    s.v[4] += flags ? 1u : 0u;
}

// One thread adds the sums to row `row` of direction `dir` (integer adds: the
// total does not depend on their order).
__device__ __forceinline__ void sums_flush(uint32_t* parts, uint32_t dir, uint32_t row, const LogSums& s) {
    uint32_t* p = parts + ((size_t)dir * kLogParts + row % kLogParts) * kLogPartRow;
#pragma unroll
    for (int i = 0; i < 5; ++i)
        if (s.v[i]) atomicAdd(p + i, s.v[i]);
}

__device__ __forceinline__ uint32_t log_flags(uint32_t n_rem, uint32_t n_ups, uint32_t n_upd, bool clock) {
    return (n_rem ? CRDT_DIFF_REMOVED : 0u) | (n_ups > n_upd ? CRDT_DIFF_ADDED : 0u) | (n_upd ? CRDT_DIFF_UPDATED : 0u) |
           (clock ? CRDT_DIFF_CLOCK : 0u);
}

// Per wave: index 0 = replica a, 1 = replica b.
struct LogWaveSmem {
    uint64_t ek[2][64], ec[2][64];
    uint64_t vv[2][64];
    uint32_t ea[2][64];
};

// One direction of a wave-path document: dst = side x of sm (nd entries, its
// slots at doff), src = side 1 - x (ns entries, slots at soff).
__device__ __forceinline__ void log_wave_dir(const LogWaveSmem& sm, uint32_t x, uint32_t nd, uint32_t ns, uint32_t R,
                                             uint32_t d, uint32_t doff, uint32_t soff, const OutView& out,
                                             const MergeLogView& lg, uint32_t lane, LogSums& sums, uint32_t& err) {
    const uint32_t y = 1u - x;
    const uint64_t* const dk = sm.ek[x];
    const uint64_t* const sk = sm.ek[y];
    const uint64_t* const dvv = sm.vv[x];
    const uint64_t* const svv = sm.vv[y];
    const Entries none{nullptr, nullptr, nullptr, 0};
    const bool dv = lane < nd, sv = lane < ns;
    const uint64_t Dk = dk[lane], Dc = sm.ec[x][lane], Sk = sk[lane], Sc = sm.ec[y][lane];
    const uint32_t Da = sm.ea[x][lane], Sa = sm.ea[y][lane];

    // # src keys < Dk, # dst keys < Sk
    const uint32_t j = lower_bound_pow<6>(sk, ns, Dk);
    const uint32_t i = lower_bound_pow<6>(dk, nd, Sk);
    const bool dmatch = dv && j < ns && sk[j & 63] == Dk;
    const bool smatch = sv && i < nd && dk[i & 63] == Sk;
    bool dkeep = false, skeep = false, supd = false;
    uint32_t oda = Da, osa = Sa;
    uint64_t odc = Dc, osc = Sc;
    if (dv)
        dkeep = decide(true, Da, Dc, dmatch, dmatch ? sm.ea[y][j & 63] : 0u, dmatch ? sm.ec[y][j & 63] : 0ull, true, dvv,
                       svv, R, none, Dk, oda, odc, err);
    if (sv) {
        if (smatch) {  // the common key as its src lane sees it: the dot the merge gives it against dst's
            const uint32_t ma = sm.ea[x][i & 63];
            const uint64_t mc = sm.ec[x][i & 63];
            decide(true, ma, mc, true, Sa, Sc, true, dvv, svv, R, none, Sk, osa, osc, err);
            supd = osa != ma || osc != mc;
        } else {
            skeep = decide(false, 0u, 0ull, true, Sa, Sc, true, dvv, svv, R, none, Sk, osa, osc, err);
        }
    }
    const bool removed = dv && !dkeep;
    const bool ups = skeep || supd;

    // a survivor's slot: kept lanes of its own side below it + kept entries of
    // the other side with a smaller key; a log record's: its kind's lanes below it
    const uint64_t dm = ballot(dkeep), smk = ballot(skeep);
    const uint64_t rm = ballot(removed), um = ballot(ups), updm = ballot(supd);
    const uint32_t obase = doff + soff;
    const uint32_t dpos = below(dm) + popc(smk & low_mask(j));
    const uint32_t spos = below(smk) + popc(dm & low_mask(i));
    const uint32_t n_out = popc(dm) + popc(smk);  // <= nd + ns <= the document's output slots
    const uint32_t n_rem = popc(rm), n_ups = popc(um), n_upd = popc(updm);  // <= nd, <= ns: within the lists' slots
    if (dkeep) {
        out.keys[obase + dpos] = Dk;
        out.actors[obase + dpos] = oda;
        out.counters[obase + dpos] = odc;
    }
    if (skeep) {
        out.keys[obase + spos] = Sk;
        out.actors[obase + spos] = osa;
        out.counters[obase + spos] = osc;
    }
    if (removed) {
        const uint32_t p = doff + below(rm);
        lg.rem_keys[p] = Dk;
        lg.rem_actors[p] = Da;
        lg.rem_counters[p] = Dc;
    }
    if (ups) {
        const uint32_t p = soff + below(um);
        lg.ups_keys[p] = Sk;
        lg.ups_actors[p] = osa;
        lg.ups_counters[p] = osc;
        if (lg.ups_kind) lg.ups_kind[p] = (uint8_t)(supd ? CRDT_DIFF_UPDATED : CRDT_DIFF_ADDED);
    }
    const bool ahead = lane < R && svv[lane] > dvv[lane];  // the merged clock is max(D, S): it differs from D
    const uint32_t flags = log_flags(n_rem, n_ups, n_upd, ballot(ahead) != 0ull);
    if (lane == 0) {
        out.counts[d] = n_out;
        lg.flags[d] = (uint8_t)flags;
        lg.rem_counts[d] = n_rem;
        lg.ups_counts[d] = n_ups;
    }
    if (lane < R) {
        const uint64_t a = dvv[lane], b = svv[lane];
        out.vv[(size_t)d * R + lane] = a > b ? a : b;  // awset.go:160 -> crdt-misc.go:43-55
    }
    sums_add(sums, n_rem, n_ups, n_upd, flags);
}

// Slot bounds of one direction's outputs for document d: the merged state's and
// the two lists' (the inputs' own bounds), every document, whichever path merges it.
__device__ __forceinline__ void log_bounds(const OutView& out, const MergeLogView& lg, const BatchView& D,
                                           const BatchView& S, uint32_t d, uint32_t doff, uint32_t soff) {
    out.offsets[d] = doff + soff;
    lg.rem_offsets[d] = doff;
    lg.ups_offsets[d] = soff;
    if (d == D.n_docs - 1) {
        const uint32_t de = D.offsets[D.n_docs], se = S.offsets[D.n_docs];
        out.offsets[D.n_docs] = de + se;
        lg.rem_offsets[D.n_docs] = de;
        lg.ups_offsets[D.n_docs] = se;
    }
}

// EXCH: also o_ba = b <- a and its log.  parts == nullptr: no summary asked for.
template <int WAVES, int K, bool EXCH>
__global__ __launch_bounds__(WAVES * 64) void join_log_wave_kernel(BatchView A, BatchView B, OutView o_ab, OutView o_ba,
                                                                   MergeLogView l_ab, MergeLogView l_ba, Work wk,
                                                                   uint32_t* parts) {
    __shared__ LogWaveSmem smem[WAVES];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t R = A.R, n_docs = A.n_docs;
    LogWaveSmem& sm = smem[w];
    uint32_t err = 0;
    LogSums s_ab{}, s_ba{};

    // (whole waves leave or stay: the kernel has no workgroup barrier)
#pragma unroll 1
    for (uint32_t k = 0; k < (uint32_t)K; ++k) {
        const uint32_t d = uniform(blockIdx.x * (WAVES * K) + k * WAVES + w);
        if (d >= n_docs) break;
        uint32_t ao, bo;
        const uint32_t na = log_live(A.offsets, A.counts, d, ao, err);
        const uint32_t nb = log_live(B.offsets, B.counts, d, bo, err);
        if (lane == 0) {
            log_bounds(o_ab, l_ab, A, B, d, ao, bo);
            if (EXCH) log_bounds(o_ba, l_ba, B, A, d, bo, ao);
        }
        if (na > kLogWaveMax || nb > kLogWaveMax) {
            if (lane == 0) push_work(wk, d, n_docs);
            continue;
        }
        wave_sync();  // every lane's probes of the previous document are done
        // both documents, once; loads guarded per lane: slack is never read
        if (lane < na) {
            sm.ek[0][lane] = A.keys[ao + lane];
            sm.ea[0][lane] = A.actors[ao + lane];
            sm.ec[0][lane] = A.counters[ao + lane];
        }
        if (lane < nb) {
            sm.ek[1][lane] = B.keys[bo + lane];
            sm.ea[1][lane] = B.actors[bo + lane];
            sm.ec[1][lane] = B.counters[bo + lane];
        }
        if (lane < R) {
            sm.vv[0][lane] = A.vv[(size_t)d * R + lane];
            sm.vv[1][lane] = B.vv[(size_t)d * R + lane];
        }
        wave_sync();
        log_wave_dir(sm, 0u, na, nb, R, d, ao, bo, o_ab, l_ab, lane, s_ab, err);
        if (EXCH) log_wave_dir(sm, 1u, nb, na, R, d, bo, ao, o_ba, l_ba, lane, s_ba, err);
    }
    if (parts && lane == 0) {
        const uint32_t row = blockIdx.x * WAVES + w;
        sums_flush(parts, 0u, row, s_ab);
        if (EXCH) sums_flush(parts, 1u, row, s_ba);
    }
    flag_error(wk.status, err);
}

// One direction of a block-path document, by the whole workgroup: block_merge's
// window walk with the log written beside the survivors.
template <int NT, int IPT>
__device__ void log_block_dir(const BatchView& Dd, const BatchView& Sd, uint32_t d, uint32_t R, MergeSmem<NT, IPT>& sm,
                              const OutView& out, const MergeLogView& lg, uint32_t* parts, uint32_t dir,
                              uint32_t& err) {
    constexpr uint32_t T = NT * IPT;
    constexpr uint8_t KEEP = 1, REM = 2, ADD = 4, UPD = 8;
    const uint32_t tid = threadIdx.x;
    uint32_t doff, soff;
    const uint32_t n_d = log_live(Dd.offsets, Dd.counts, d, doff, err);
    const uint32_t n_s = log_live(Sd.offsets, Sd.counts, d, soff, err);
    const Entries D{Dd.keys + doff, Dd.actors + doff, Dd.counters + doff, n_d};
    const Entries S{Sd.keys + soff, Sd.actors + soff, Sd.counters + soff, n_s};
    const Entries none{nullptr, nullptr, nullptr, 0};
    if (tid < R) {
        sm.dvv[tid] = Dd.vv[(size_t)d * R + tid];
        sm.svv[tid] = Sd.vv[(size_t)d * R + tid];
    }
    __syncthreads();
    const uint32_t obase = doff + soff;
    const EntriesOut O{out.keys + obase, out.actors + obase, out.counters + obase};
    const EntriesOut RM{lg.rem_keys + doff, lg.rem_actors + doff, lg.rem_counters + doff};
    const EntriesOut UP{lg.ups_keys + soff, lg.ups_actors + soff, lg.ups_counters + soff};
    uint8_t* const UK = lg.ups_kind ? lg.ups_kind + soff : nullptr;

    uint32_t i = 0, j = 0;
    uint32_t o = 0, o_rem = 0, o_ups = 0;  // running offsets: survivors (<= n_d + n_s), removed (<= n_d), upserted (<= n_s)
    uint32_t my_upd = 0;
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

        // per merged position: the key, the dot its record carries (the merged dot of a
        // survivor or an upsert; of a removed entry its own, which decide returns too)
        uint64_t ok[IPT];
        uint32_t oa[IPT];
        uint64_t oc[IPT];
        uint8_t cls[IPT];
        uint32_t cnt = 0, cnt_rem = 0, cnt_ups = 0;
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
                    const bool kp = decide(true, d_a, d_c, match, s_a, s_c, true, sm.dvv, sm.svv, R, none, key, oa[q],
                                           oc[q], err);
                    ok[q] = key;
                    cls[q] = kp ? KEEP : REM;
                    if (match && (oa[q] != d_a || oc[q] != d_c)) cls[q] |= UPD;
                    ++a;
                } else {
                    const uint64_t key = sm.sk[b];
                    const bool match = (a > 0) ? (sm.dk[a - 1] == key) : (has_prev && prev_dk == key);
                    if (!match) {
                        const bool kp = decide(false, 0u, 0ull, true, sm.sa[b], sm.sc[b], true, sm.dvv, sm.svv, R, none,
                                               key, oa[q], oc[q], err);
                        ok[q] = key;
                        cls[q] = kp ? (KEEP | ADD) : 0;
                    }
                    ++b;
                }
                cnt += (cls[q] & KEEP) ? 1u : 0u;
                cnt_rem += (cls[q] & REM) ? 1u : 0u;
                cnt_ups += (cls[q] & (ADD | UPD)) ? 1u : 0u;
                my_upd += (cls[q] & UPD) ? 1u : 0u;
            }
        }
        uint32_t total, total_rem, total_ups;
        uint32_t pos = o + block_exclusive_scan<NT>(cnt, sm.wave_tot, &total);
        uint32_t pos_rem = o_rem + block_exclusive_scan<NT>(cnt_rem, sm.wave_tot, &total_rem);
        uint32_t pos_ups = o_ups + block_exclusive_scan<NT>(cnt_ups, sm.wave_tot, &total_ups);
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
            if (cls[q] & KEEP) {
                O.k[pos] = ok[q];
                O.a[pos] = oa[q];
                O.c[pos] = oc[q];
                ++pos;
            }
            if (cls[q] & REM) {
                RM.k[pos_rem] = ok[q];
                RM.a[pos_rem] = oa[q];
                RM.c[pos_rem] = oc[q];
                ++pos_rem;
            }
            if (cls[q] & (ADD | UPD)) {
                UP.k[pos_ups] = ok[q];
                UP.a[pos_ups] = oa[q];
                UP.c[pos_ups] = oc[q];
                if (UK) UK[pos_ups] = (uint8_t)((cls[q] & UPD) ? CRDT_DIFF_UPDATED : CRDT_DIFF_ADDED);
                ++pos_ups;
            }
        }
        const uint32_t aK = merge_path(sm.dk, nd, sm.sk, ns, K);
        i += aK;
        j += K - aK;
        o += total;
        o_rem += total_rem;
        o_ups += total_ups;
        __syncthreads();
    }
    uint32_t n_upd;
    block_exclusive_scan<NT>(my_upd, sm.wave_tot, &n_upd);
    const bool clock = __syncthreads_or(tid < R && sm.svv[tid] > sm.dvv[tid]) != 0;
    const uint32_t flags = log_flags(o_rem, o_ups, n_upd, clock);
    if (tid == 0) {
        out.counts[d] = o;
        lg.flags[d] = (uint8_t)flags;
        lg.rem_counts[d] = o_rem;
        lg.ups_counts[d] = o_ups;
        if (parts) {
            LogSums s{};
            sums_add(s, o_rem, o_ups, n_upd, flags);
            sums_flush(parts, dir, blockIdx.x, s);
        }
    }
    if (tid < R) {
        const uint64_t x = sm.dvv[tid], y = sm.svv[tid];
        out.vv[(size_t)d * R + tid] = x > y ? x : y;
    }
    __syncthreads();  // sm.dvv / sm.svv are the next direction's
}

template <int NT, int IPT, bool EXCH>
__global__ __launch_bounds__(NT) void join_log_block_kernel(BatchView A, BatchView B, OutView o_ab, OutView o_ba,
                                                            MergeLogView l_ab, MergeLogView l_ba, Work wk,
                                                            uint32_t* parts) {
    __shared__ MergeSmem<NT, IPT> sm;
    const uint32_t tid = threadIdx.x;
    const uint32_t R = A.R, n_docs = A.n_docs;
    uint32_t err = 0;
    if (work_total(wk, n_docs) == 0) return;  // empty worklist (set by the previous launch)
    for (;;) {
        if (tid == 0) sm.word[0] = atomicAdd(wk.wl_head, 1u);
        __syncthreads();
        const uint32_t slot = sm.word[0];
        const uint32_t total = work_total(wk, n_docs);
        __syncthreads();
        if (slot >= total) break;
        const uint32_t d = wk.worklist[slot];
        if (d >= n_docs) {  // not a document of this call: never dereferenced
            if (tid == 0) atomicOr(wk.status, kErrWorkspace);
            continue;
        }
        log_block_dir<NT, IPT>(A, B, d, R, sm, o_ab, l_ab, parts, 0u, err);
        if (EXCH) log_block_dir<NT, IPT>(B, A, d, R, sm, o_ba, l_ba, parts, 1u, err);
    }
    flag_error(wk.status, err);
}

// Zeroes n words (the partial rows, or a summary of a call without documents): a
// kernel rather than hipMemsetAsync, so a captured call is a graph of kernel nodes only.
__global__ __launch_bounds__(256) void join_log_zero_kernel(uint32_t* p, uint32_t* q, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        if (p) p[i] = 0u;
        if (q) q[i] = 0u;
    }
}

// summary of direction blockIdx.x = the column sums of its partial rows.
__global__ __launch_bounds__(256) void join_log_summary_kernel(const uint32_t* parts, uint32_t* s_ab, uint32_t* s_ba) {
    __shared__ uint32_t acc[4][kLogPartRow];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t* const out = blockIdx.x ? s_ba : s_ab;
    if (!out) return;  // (the whole workgroup)
    const uint32_t* const p = parts + (size_t)blockIdx.x * kLogParts * kLogPartRow;
    uint32_t v[5] = {0u, 0u, 0u, 0u, 0u};
    for (uint32_t row = tid; row < kLogParts; row += 256)
#pragma unroll
        for (int i = 0; i < 5; ++i) v[i] += p[row * kLogPartRow + i];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[i] += (uint32_t)__shfl_xor((int)v[i], o);
        if (lane == 0) acc[w][i] = v[i];
    }
    __syncthreads();
    if (tid < 5) out[tid] = acc[0][tid] + acc[1][tid] + acc[2][tid] + acc[3][tid];
}

// log_ba == nullptr: the join (one direction).  parts: join_log_parts_bytes() of
// workspace, used when either log has a summary.
hipError_t launch_join_log(const BatchView& A, const BatchView& B, const OutView& out_ab, const OutView* out_ba,
                           const MergeLogView& log_ab, const MergeLogView* log_ba, const Work& wk, uint32_t* parts,
                           uint32_t block_grid, hipStream_t stream) {
    const uint32_t n = A.n_docs;
    const bool exch = out_ba != nullptr && log_ba != nullptr;
    uint32_t* const s_ab = log_ab.summary;
    uint32_t* const s_ba = exch ? log_ba->summary : nullptr;
    if (n == 0) {  // nothing that reads documents
        if (!s_ab && !s_ba) return hipSuccess;
        hipLaunchKernelGGL(join_log_zero_kernel, dim3(1), dim3(256), 0, stream, s_ab, s_ba, 5u);
        return hipGetLastError();
    }
    uint32_t* const pp = (s_ab || s_ba) ? parts : nullptr;
    if (pp) {
        const uint32_t words = (uint32_t)(join_log_parts_bytes() / sizeof(uint32_t));
        hipLaunchKernelGGL(join_log_zero_kernel, dim3((words + 255) / 256), dim3(256), 0, stream, pp,
                           (uint32_t*)nullptr, words);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const OutView& o2 = exch ? *out_ba : out_ab;
    const MergeLogView& l2 = exch ? *log_ba : log_ab;
    const uint32_t per_block = kLogWaves * kLogDocs;
    const dim3 grid((n + per_block - 1) / per_block), block(kLogWaves * 64);
    if (exch)
        hipLaunchKernelGGL((join_log_wave_kernel<kLogWaves, kLogDocs, true>), grid, block, 0, stream, A, B, out_ab, o2,
                           log_ab, l2, wk, pp);
    else
        hipLaunchKernelGGL((join_log_wave_kernel<kLogWaves, kLogDocs, false>), grid, block, 0, stream, A, B, out_ab, o2,
                           log_ab, l2, wk, pp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (exch)
        hipLaunchKernelGGL((join_log_block_kernel<kLogBlockNT, kLogBlockIPT, true>), dim3(block_grid), dim3(kLogBlockNT),
                           0, stream, A, B, out_ab, o2, log_ab, l2, wk, pp);
    else
        hipLaunchKernelGGL((join_log_block_kernel<kLogBlockNT, kLogBlockIPT, false>), dim3(block_grid),
                           dim3(kLogBlockNT), 0, stream, A, B, out_ab, o2, log_ab, l2, wk, pp);
    e = hipGetLastError();
    if (e != hipSuccess || !pp) return e;
    hipLaunchKernelGGL(join_log_summary_kernel, dim3(exch ? 2 : 1), dim3(256), 0, stream, pp, s_ab, s_ba);
    return hipGetLastError();
}

}  // namespace crdt
