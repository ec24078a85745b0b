// Wave path of a pair merge (delta_pair.hip, join_log.hip): one wavefront per
// document when each list of both replicas holds <= 64 live entries.  Both
// sides' entries and clocks are staged in per-wave LDS once and every direction
// dst <- src is decided from that staging.  Lane i owns entry i of each side and
// finds its key on the other side by LDS binary search; the survivors are
// compacted by ballot and popcount, as in join_wave_kernel (join.hip), so the
// output is sorted by key and written once.  What a kernel adds of its own (the
// kind and the tombstones there, the log's ranks and sums here) stays with it.
#pragma once

#include "crdt_device.hpp"

namespace crdt {

// Per wave: index 0 = replica a, 1 = replica b.
struct WaveSmem {
    uint64_t ek[2][64], ec[2][64];  // entries
    uint64_t vv[2][64];
    uint32_t ea[2][64];
};

// Lane i stages element off + i of a list of n <= 64; loads guarded per lane:
// slack is never read.
__device__ __forceinline__ void wave_stage(uint64_t* k, uint32_t* a, uint64_t* c, const uint64_t* gk, const uint32_t* ga,
                                           const uint64_t* gc, uint32_t off, uint32_t n, uint32_t lane) {
    if (lane < n) {
        k[lane] = gk[off + lane];
        a[lane] = ga[off + lane];
        c[lane] = gc[off + lane];
    }
}

// Both replicas' document d, once: na entries of A at ao, nb of B at bo, the clocks.
__device__ __forceinline__ void wave_stage_pair(WaveSmem& sm, const BatchView& A, const BatchView& B, uint32_t d,
                                                uint32_t ao, uint32_t na, uint32_t bo, uint32_t nb, uint32_t lane) {
    const uint32_t R = A.R;
    wave_stage(sm.ek[0], sm.ea[0], sm.ec[0], A.keys, A.actors, A.counters, ao, na, lane);
    wave_stage(sm.ek[1], sm.ea[1], sm.ec[1], B.keys, B.actors, B.counters, bo, nb, lane);
    if (lane < R) {
        sm.vv[0][lane] = A.vv[(size_t)d * R + lane];
        sm.vv[1][lane] = B.vv[(size_t)d * R + lane];
    }
}

// One direction of a staged document as a lane sees it: dst = side x (nd entries),
// src = side 1 - x (ns entries).  The lane's own dst entry D* and src entry S*,
// and where each key falls on the other side.
struct WaveDir {
    const uint64_t *dk, *sk;    // the key columns
    const uint64_t *dvv, *svv;  // the clocks
    bool dv, sv;                // the lane holds a dst / a src entry
    uint64_t Dk, Dc, Sk, Sc;
    uint32_t Da, Sa;
    uint32_t j, i;         // # src keys < Dk, # dst keys < Sk
    bool dmatch, smatch;   // Dk is also in src (at j), Sk is also in dst (at i)
    uint32_t ja, ia;       // the matched entry's dot (0 without a match)
    uint64_t jc, ic;
};

__device__ __forceinline__ WaveDir wave_lookup(const WaveSmem& sm, uint32_t x, uint32_t nd, uint32_t ns, uint32_t lane) {
    const uint32_t y = 1u - x;
    WaveDir p;
    p.dk = sm.ek[x];
    p.sk = sm.ek[y];
    p.dvv = sm.vv[x];
    p.svv = sm.vv[y];
    p.dv = lane < nd;
    p.sv = lane < ns;
    p.Dk = p.dk[lane];
    p.Dc = sm.ec[x][lane];
    p.Da = sm.ea[x][lane];
    p.Sk = p.sk[lane];
    p.Sc = sm.ec[y][lane];
    p.Sa = sm.ea[y][lane];
    p.j = lower_bound_pow<6>(p.sk, ns, p.Dk);
    p.i = lower_bound_pow<6>(p.dk, nd, p.Sk);
    p.dmatch = p.dv && p.j < ns && p.sk[p.j & 63] == p.Dk;
    p.smatch = p.sv && p.i < nd && p.dk[p.i & 63] == p.Sk;
    p.ja = p.dmatch ? sm.ea[y][p.j & 63] : 0u;
    p.jc = p.dmatch ? sm.ec[y][p.j & 63] : 0ull;
    p.ia = p.smatch ? sm.ea[x][p.i & 63] : 0u;
    p.ic = p.smatch ? sm.ec[x][p.i & 63] : 0ull;
    return p;
}

// Stores the survivors (dkeep: the lane's dst entry with dot (oda, odc); skeep:
// its src entry with (osa, osc)) from slot obase on and returns their number.  A
// survivor's slot: kept lanes of its own side below it + kept entries of the
// other side with a smaller key.
__device__ __forceinline__ uint32_t wave_place(const WaveDir& p, bool dkeep, uint32_t oda, uint64_t odc, bool skeep,
                                               uint32_t osa, uint64_t osc, const OutView& out, uint32_t obase) {
    const uint64_t dm = ballot(dkeep), smk = ballot(skeep);
    const uint32_t dpos = obase + below(dm) + popc(smk & low_mask(p.j));
    const uint32_t spos = obase + below(smk) + popc(dm & low_mask(p.i));
    if (dkeep) {
        out.keys[dpos] = p.Dk;
        out.actors[dpos] = oda;
        out.counters[dpos] = odc;
    }
    if (skeep) {
        out.keys[spos] = p.Sk;
        out.actors[spos] = osa;
        out.counters[spos] = osc;
    }
    return popc(dm) + popc(smk);  // <= nd + ns <= the document's output slots
}

// The merged clock of document d: max(D, S) (awset.go:160 -> crdt-misc.go:43-55),
// or D untouched (keep_dst: a delta merge that changes nothing).
__device__ __forceinline__ void wave_clock(const WaveDir& p, bool keep_dst, const OutView& out, uint32_t d, uint32_t R,
                                           uint32_t lane) {
    if (lane < R) {
        const uint64_t a = p.dvv[lane], b = p.svv[lane];
        out.vv[(size_t)d * R + lane] = (keep_dst || a > b) ? a : b;
    }
}

// ---- the delta merges (delta_pair.hip, delta_pair_log.hip): tombstones and the kind.
// Per wave: the entries and clocks and both sides' tombstones (<= 64 a side).
struct alignas(8) PairWaveSmem : WaveSmem {
    alignas(8) uint64_t tk[2][64];
    alignas(8) uint64_t tc[2][64];
    uint32_t ta[2][64];
};

// The kind of the direction p of a staged document, before any entry is decided
// (awset-delta_test.go:53, :60): src = side y with ns entries, nts tombstones and
// actor s_actor.  full: D has never met src's actor.
__device__ __forceinline__ uint32_t pair_wave_kind(const PairWaveSmem& sm, const WaveDir& p, uint32_t y, uint32_t ns,
                                                   uint32_t nts, uint32_t s_actor, uint32_t R, uint32_t lane,
                                                   bool& full, uint32_t& err) {
    full = uniform((uint32_t)(vv_counter(p.dvv, R, s_actor, err) == 0ull)) != 0u;
    uint32_t kind = CRDT_DELTA_FULL;
    if (!full) {
        const bool changed = p.sv && !has_dot(p.dvv, R, p.Sa, p.Sc, err);
        bool effective = false;  // a tombstone the re-add filter lets through (:93-102)
        if (lane < nts) {
            const uint64_t Tk = sm.tk[y][lane];
            const uint32_t m = lower_bound_pow<6>(p.sk, ns, Tk);
            const bool readded = m < ns && p.sk[m & 63] == Tk &&
                                 (sm.ea[y][m & 63] != sm.ta[y][lane] || sm.ec[y][m & 63] > sm.tc[y][lane]);
            effective = !readded;
        }
        kind = (ballot(changed) | ballot(effective)) ? CRDT_DELTA_DELTA : CRDT_DELTA_NONE;
    }
    return kind;
}

// Slot bounds of one direction's outputs for document d, from the inputs' own
// (dst's slots start at doff, src's at soff): the merged state's, and the logged
// join's two lists (a removed entry was a dst entry, an upserted one a src entry;
// NULL: no log).  Every document, whichever path merges it; the last one closes
// the columns.
__device__ __forceinline__ void pair_bounds(uint32_t* out_off, uint32_t* rem_off, uint32_t* ups_off,
                                            const uint32_t* d_off, const uint32_t* s_off, uint32_t d, uint32_t n_docs,
                                            uint32_t doff, uint32_t soff) {
    out_off[d] = doff + soff;
    if (rem_off) rem_off[d] = doff;
    if (ups_off) ups_off[d] = soff;
    if (d == n_docs - 1) {
        const uint32_t de = d_off[n_docs], se = s_off[n_docs];
        out_off[n_docs] = de + se;
        if (rem_off) rem_off[n_docs] = de;
        if (ups_off) ups_off[n_docs] = se;
    }
}

}  // namespace crdt
