// Argument checks of the C ABI (include/crdtgpu.h): everything an *_async entry
// point refuses with CRDT_E_INVALID before it touches the device, except its NULL
// context.  Host code only -- descriptors are read, arrays never -- so a plain C++
// compiler builds it and tests/cpp/test_api_args.cpp drives every rule under
// ASan/UBSan.  api.cpp calls one check_* per entry-point family.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/crdtgpu.h"

namespace crdt {

// ---- required pointers ------------------------------------------------------

inline bool batch_ptrs_ok(const crdt_awset_batch* b) {
    return b && b->offsets && (b->n_docs == 0 || b->vv) && b->R > 0 && b->R <= CRDT_MAX_R;
}

inline bool out_ptrs_ok(const crdt_awset_out* o) {
    return o && o->offsets && o->counts && o->keys && o->actors && o->counters && o->vv;
}

inline bool src_ptrs_ok(const crdt_src_batch* s) {
    return s && s->doc_srcs && s->src_actor && s->entry_off && s->R > 0 && s->R <= CRDT_MAX_R &&
           (!s->tomb_off || (s->tkeys && s->tactors && s->tcounters));
}

// (summary and ups_kind are optional)
inline bool merge_log_ok(const crdt_merge_log* l) {
    return l && l->flags && l->rem_offsets && l->rem_counts && l->rem_keys && l->rem_actors && l->rem_counters &&
           l->ups_offsets && l->ups_counts && l->ups_keys && l->ups_actors && l->ups_counters;
}

inline bool tomb_out_ok(const crdt_tomb_out* t) {
    return t && t->offsets && t->counts && t->keys && t->actors && t->counters;
}

// columns: the apply reads them whatever the batch holds; every other caller needs the offsets alone
inline bool tomb_batch_ok(const crdt_tomb_batch* t, bool columns) {
    return t && t->offsets && (!columns || (t->keys && t->actors && t->counters));
}

// tombs: the tombstone columns too (the input has tombstones)
inline bool delta_out_ok(const crdt_delta_out* o, bool tombs) {
    return o && o->doc_srcs && o->src_actor && o->vv && o->entry_off && o->keys && o->actors && o->counters &&
           (!tombs || (o->tomb_off && o->tkeys && o->tactors && o->tcounters));
}

inline bool compare_out_ok(const crdt_compare_out* o, uint32_t mask) {
    return o && o->flags && mask <= 15u && (o->worklist == nullptr) == (o->n_work == nullptr);
}

// ---- array lists and the three aliasing rules ------------------------------------

// The arrays a call writes, or the inputs they are compared with.  A NULL pointer
// is never listed, so it never matches.  No heap; the largest user, the logged
// delta exchange, writes 2 x 6 + 2 x 13 + 2 = 40 arrays.
struct Arrays {
    struct Arr {
        uintptr_t p;
        size_t bytes;  // 0: size unknown on the host (entry arrays, empty per-document arrays)
        int width;     // bytes per element, 1 / 4 / 8: the array's kind
    };
    Arr a[40];
    int n = 0;
    void add(const void* p, int width, size_t bytes = 0) {
        if (p) a[n++] = Arr{(uintptr_t)p, bytes, width};
    }
    // written
    void add_out(const crdt_awset_out* o, size_t nd, size_t R) {  // (this order: check_exchange names keys, [3])
        add(o->offsets, 4, (nd + 1) * 4);
        add(o->counts, 4, nd * 4);
        add(o->vv, 8, nd * R * 8);
        add(o->keys, 8);
        add(o->actors, 4);
        add(o->counters, 8);
    }
    void add_log(const crdt_merge_log* l, size_t nd) {
        add(l->flags, 1, nd);
        add(l->summary, 4, 5 * 4);
        add(l->rem_offsets, 4, (nd + 1) * 4);
        add(l->rem_counts, 4, nd * 4);
        add(l->ups_offsets, 4, (nd + 1) * 4);
        add(l->ups_counts, 4, nd * 4);
        add(l->rem_keys, 8);
        add(l->rem_actors, 4);
        add(l->rem_counters, 8);
        add(l->ups_keys, 8);
        add(l->ups_actors, 4);
        add(l->ups_counters, 8);
        add(l->ups_kind, 1);
    }
    void add_tomb_out(const crdt_tomb_out* t) {  // unsized: its users compare starts alone
        add(t->offsets, 4);
        add(t->counts, 4);
        add(t->keys, 8);
        add(t->actors, 4);
        add(t->counters, 8);
    }
    void add_kind(const uint8_t* kind, size_t nd) { add(kind, 1, nd); }
    // inputs
    void add_batch(const crdt_awset_batch* b) {
        add(b->offsets, 4);
        add(b->counts, 4);
        add(b->actors, 4);
        add(b->keys, 8);
        add(b->counters, 8);
        add(b->vv, 8);
    }
    void add_tombs(const crdt_tomb_batch* t) {  // NULL: none
        if (!t) return;
        add(t->offsets, 4);
        add(t->counts, 4);
        add(t->actors, 4);
        add(t->keys, 8);
        add(t->counters, 8);
    }
    void add_replica(const crdt_replica* r) {
        add_batch(r->state);
        add_tombs(r->tombs);
        add(r->doc_actor, 4);
    }
};

// No two written arrays start at one address; (skip_i, skip_j): the one pair that may.
inline bool starts_distinct(const Arrays& w, int skip_i = -1, int skip_j = -1) {
    for (int i = 0; i < w.n; ++i)
        for (int j = i + 1; j < w.n; ++j)
            if (w.a[i].p == w.a[j].p && !(i == skip_i && j == skip_j)) return false;
    return true;
}

// No two written arrays whose sizes the host knows overlap.  The entry arrays'
// capacity lives in device memory: a partial overlap of them is undefined
// (include/crdtgpu.h).
inline bool sized_disjoint(const Arrays& w) {
    for (int i = 0; i < w.n; ++i)
        for (int j = i + 1; j < w.n; ++j) {
            const Arrays::Arr &x = w.a[i], &y = w.a[j];
            if (x.bytes && y.bytes && x.p < y.p + y.bytes && y.p < x.p + x.bytes) return false;
        }
    return true;
}

// No written array starts where a listed input of the same kind (width) starts;
// any_width: where any listed input starts.
inline bool off_inputs(const Arrays& w, const Arrays& in, bool any_width = false) {
    for (int i = 0; i < w.n; ++i)
        for (int j = 0; j < in.n; ++j)
            if (w.a[i].p == in.a[j].p && (any_width || w.a[i].width == in.a[j].width)) return false;
    return true;
}

// ---- one check per entry-point family ----------------------------------------
// Each returns CRDT_OK or CRDT_E_INVALID.  The families differ in which rules they
// apply; every difference is an argument or a comment at the call below, and none
// is to be "fixed" here: that would be a behaviour change.

inline int check_join(const crdt_awset_batch* dst, const crdt_awset_batch* src, const crdt_awset_out* out,
                      const crdt_awset_out* out2 /* or NULL */) {
    if (!batch_ptrs_ok(dst) || !batch_ptrs_ok(src) || !out_ptrs_ok(out) || (out2 && !out_ptrs_ok(out2)))
        return CRDT_E_INVALID;
    if (dst->n_docs != src->n_docs || dst->R != src->R) return CRDT_E_INVALID;
    return CRDT_OK;  // (no input rule: an output may start on an input)
}

inline int check_exchange(const crdt_awset_batch* a, const crdt_awset_batch* b, const crdt_awset_out* out_ab,
                          const crdt_awset_out* out_ba) {
    if (!out_ba || check_join(a, b, out_ab, out_ba) != CRDT_OK) return CRDT_E_INVALID;
    Arrays w;
    w.add_out(out_ab, a->n_docs, a->R);
    w.add_out(out_ba, a->n_docs, a->R);
    // out_ba->keys == out_ab->keys is one shared key column: both directions hold
    // the same keys at the same slots (the plain exchange alone allows it)
    if (!starts_distinct(w, 3, 9) || !sized_disjoint(w)) return CRDT_E_INVALID;
    return CRDT_OK;  // (no input rule, as the join)
}

inline int check_fold(int mode, const crdt_awset_batch* dst, const crdt_src_batch* srcs, const crdt_awset_out* out) {
    if (!batch_ptrs_ok(dst) || !src_ptrs_ok(srcs) || !out_ptrs_ok(out)) return CRDT_E_INVALID;
    if (mode != CRDT_FOLD_AWSET && mode != CRDT_FOLD_DELTA) return CRDT_E_INVALID;
    if (dst->n_docs != srcs->n_docs || dst->R != srcs->R) return CRDT_E_INVALID;
    return CRDT_OK;
}

inline int check_fold_log(int mode, const crdt_awset_batch* dst, const crdt_src_batch* srcs,
                          const crdt_awset_out* out, const crdt_merge_log* log) {
    if (check_fold(mode, dst, srcs, out) != CRDT_OK || !merge_log_ok(log)) return CRDT_E_INVALID;
    Arrays w, in;
    w.add_out(out, dst->n_docs, dst->R);
    w.add_log(log, dst->n_docs);
    in.add_batch(dst);
    for (const uint32_t* p : {srcs->doc_srcs, srcs->src_actor, srcs->entry_off, srcs->actors, srcs->tomb_off,
                              srcs->tactors})
        in.add(p, 4);
    for (const uint64_t* p : {srcs->vv, srcs->keys, srcs->counters, srcs->tkeys, srcs->tcounters}) in.add(p, 8);
    // (no 1-byte input is listed: flags and ups_kind are compared with written arrays only)
    if (!starts_distinct(w) || !sized_disjoint(w) || !off_inputs(w, in)) return CRDT_E_INVALID;
    return CRDT_OK;
}

inline int check_join_log(const crdt_awset_batch* a, const crdt_awset_batch* b, const crdt_awset_out* out_ab,
                          const crdt_awset_out* out_ba, const crdt_merge_log* log_ab, const crdt_merge_log* log_ba,
                          bool exchange) {
    if (exchange && (!out_ba || !log_ba)) return CRDT_E_INVALID;
    if (check_join(a, b, out_ab, out_ba) != CRDT_OK) return CRDT_E_INVALID;
    if (!merge_log_ok(log_ab) || (out_ba && !merge_log_ok(log_ba))) return CRDT_E_INVALID;
    Arrays w, in;
    w.add_out(out_ab, a->n_docs, a->R);
    w.add_log(log_ab, a->n_docs);
    if (out_ba) {
        w.add_out(out_ba, a->n_docs, a->R);
        w.add_log(log_ba, a->n_docs);
    }
    in.add_batch(a);
    in.add_batch(b);
    // no excepted pair: the logged exchange refuses the shared key column
    if (!starts_distinct(w) || !sized_disjoint(w) || !off_inputs(w, in)) return CRDT_E_INVALID;
    return CRDT_OK;
}

// The required pointers of a delta pair: replica a is (a, a_tombs, a_doc_actor), the
// join passes its dst state alone.
inline bool delta_pair_ptrs_ok(const crdt_awset_batch* a, const crdt_tomb_batch* a_tombs, const crdt_replica* b,
                               const crdt_awset_out* out_ab, const crdt_awset_out* out_ba) {
    if (!b || check_join(a, b->state, out_ab, out_ba) != CRDT_OK) return false;
    return !(a_tombs && !tomb_batch_ok(a_tombs, false)) && !(b->tombs && !tomb_batch_ok(b->tombs, false));
}

inline void add_pair_inputs(Arrays& in, const crdt_awset_batch* a, const crdt_tomb_batch* a_tombs,
                            const uint32_t* a_doc_actor, const crdt_replica* b) {
    in.add_batch(a);
    in.add_tombs(a_tombs);
    in.add(a_doc_actor, 4);
    in.add_replica(b);
}

inline int check_delta_pair(const crdt_awset_batch* a, const crdt_tomb_batch* a_tombs, const uint32_t* a_doc_actor,
                            const crdt_replica* b, const crdt_awset_out* out_ab, const crdt_awset_out* out_ba,
                            const uint8_t* kind_ab, const uint8_t* kind_ba) {
    if (!delta_pair_ptrs_ok(a, a_tombs, b, out_ab, out_ba)) return CRDT_E_INVALID;
    Arrays w, in;
    w.add_out(out_ab, a->n_docs, a->R);
    if (out_ba) w.add_out(out_ba, a->n_docs, a->R);
    add_pair_inputs(in, a, a_tombs, a_doc_actor, b);
    // no excepted pair: the two directions keep different keys
    if (!starts_distinct(w) || !sized_disjoint(w) || !off_inputs(w, in)) return CRDT_E_INVALID;
    // the kinds are not in the written set here: compared with each other alone
    // (the logged pair lists them)
    if (kind_ab && kind_ab == kind_ba) return CRDT_E_INVALID;
    return CRDT_OK;
}

inline int check_delta_exchange(const crdt_replica* a, const crdt_replica* b, const crdt_awset_out* out_ab,
                                const crdt_awset_out* out_ba, const uint8_t* kind_ab, const uint8_t* kind_ba) {
    if (!a || !out_ba) return CRDT_E_INVALID;
    return check_delta_pair(a->state, a->tombs, a->doc_actor, b, out_ab, out_ba, kind_ab, kind_ba);
}

inline int check_delta_pair_log(const crdt_awset_batch* a, const crdt_tomb_batch* a_tombs,
                                const uint32_t* a_doc_actor, const crdt_replica* b, const crdt_awset_out* out_ab,
                                const crdt_awset_out* out_ba, const uint8_t* kind_ab, const uint8_t* kind_ba,
                                const crdt_merge_log* log_ab, const crdt_merge_log* log_ba) {
    if (!delta_pair_ptrs_ok(a, a_tombs, b, out_ab, out_ba)) return CRDT_E_INVALID;
    if (!merge_log_ok(log_ab) || (out_ba && !merge_log_ok(log_ba))) return CRDT_E_INVALID;
    Arrays w, in;
    w.add_out(out_ab, a->n_docs, a->R);
    w.add_log(log_ab, a->n_docs);
    w.add_kind(kind_ab, a->n_docs);  // the kinds are written arrays of n_docs bytes here
    if (out_ba) {
        w.add_out(out_ba, a->n_docs, a->R);
        w.add_log(log_ba, a->n_docs);
        w.add_kind(kind_ba, a->n_docs);
    }
    add_pair_inputs(in, a, a_tombs, a_doc_actor, b);
    if (!starts_distinct(w) || !sized_disjoint(w) || !off_inputs(w, in)) return CRDT_E_INVALID;
    return CRDT_OK;
}

inline int check_delta_exchange_log(const crdt_replica* a, const crdt_replica* b, const crdt_awset_out* out_ab,
                                    const crdt_awset_out* out_ba, const uint8_t* kind_ab, const uint8_t* kind_ba,
                                    const crdt_merge_log* log_ab, const crdt_merge_log* log_ba) {
    if (!a || !out_ba || !log_ba) return CRDT_E_INVALID;
    return check_delta_pair_log(a->state, a->tombs, a->doc_actor, b, out_ab, out_ba, kind_ab, kind_ba, log_ab,
                                log_ba);
}

inline int check_apply(const crdt_awset_batch* state, const crdt_tomb_batch* tombs, const crdt_op_batch* ops,
                       const crdt_awset_out* out, const crdt_tomb_out* tomb_out) {
    if (!batch_ptrs_ok(state) || !ops || !ops->op_off || !ops->doc_actor || !out_ptrs_ok(out)) return CRDT_E_INVALID;
    if (ops->n_docs != state->n_docs) return CRDT_E_INVALID;
    if ((tombs && !tomb_batch_ok(tombs, true)) || (tomb_out && !tomb_out_ok(tomb_out))) return CRDT_E_INVALID;
    return CRDT_OK;  // (no aliasing rule at all)
}

inline int check_apply_log(const crdt_awset_batch* state, const crdt_tomb_batch* tombs, const crdt_op_batch* ops,
                           const crdt_awset_out* out, const crdt_tomb_out* tomb_out, const crdt_merge_log* log) {
    if (check_apply(state, tombs, ops, out, tomb_out) != CRDT_OK || !merge_log_ok(log)) return CRDT_E_INVALID;
    Arrays w, in;
    w.add_out(out, state->n_docs, state->R);
    w.add_log(log, state->n_docs);
    if (tomb_out) w.add_tomb_out(tomb_out);
    in.add_batch(state);
    in.add_tombs(tombs);
    in.add(ops->op_off, 4);
    in.add(ops->doc_actor, 4);
    in.add(ops->keys, 8);
    in.add(ops->kind, 1);  // the one 1-byte input of any call: flags and ups_kind are compared with it
    // starts only: unlike the other logged calls, no sized-overlap rule
    if (!starts_distinct(w) || !off_inputs(w, in)) return CRDT_E_INVALID;
    return CRDT_OK;
}

// Select, scatter and sources compare field by field (out->offsets with the
// input's offsets only), not kind by kind.
inline bool out_on_batch(const crdt_awset_out* out, const crdt_awset_batch* b) {
    return out->offsets == b->offsets || out->counts == b->counts || out->keys == b->keys ||
           out->actors == b->actors || out->counters == b->counters || out->vv == b->vv;
}

inline int check_select(const crdt_awset_batch* state, const crdt_awset_out* out) {
    if (!batch_ptrs_ok(state) || !out_ptrs_ok(out) || out_on_batch(out, state)) return CRDT_E_INVALID;
    return CRDT_OK;
}

inline int check_scatter(const crdt_awset_batch* state, const crdt_awset_batch* sub, const uint32_t* idx,
                         const crdt_awset_out* out) {
    if (!batch_ptrs_ok(state) || !batch_ptrs_ok(sub) || !idx || !out_ptrs_ok(out)) return CRDT_E_INVALID;
    if (state->R != sub->R || out_on_batch(out, state) || out_on_batch(out, sub)) return CRDT_E_INVALID;
    return CRDT_OK;
}

inline int check_sources(const crdt_replica* reps, uint32_t n_reps, const crdt_delta_out* out) {
    if (!reps || n_reps == 0 || n_reps > CRDT_MAX_REPLICAS || !delta_out_ok(out, false)) return CRDT_E_INVALID;
    for (uint32_t p = 0; p < n_reps; ++p) {
        const crdt_awset_batch* b = reps[p].state;
        if (!batch_ptrs_ok(b)) return CRDT_E_INVALID;
        if (b->n_docs != reps[0].state->n_docs || b->R != reps[0].state->R) return CRDT_E_INVALID;
        if (out->entry_off == b->offsets || out->keys == b->keys || out->actors == b->actors ||
            out->counters == b->counters || out->vv == b->vv || out->src_actor == reps[p].doc_actor)
            return CRDT_E_INVALID;
        if (const crdt_tomb_batch* t = reps[p].tombs) {
            if (!tomb_batch_ok(t, false) || !delta_out_ok(out, true)) return CRDT_E_INVALID;
            if (out->tomb_off == t->offsets || out->tkeys == t->keys || out->tactors == t->actors ||
                out->tcounters == t->counters)
                return CRDT_E_INVALID;
        }
    }
    if ((uint64_t)reps[0].state->n_docs * n_reps >= (1ull << 32)) return CRDT_E_INVALID;
    return CRDT_OK;
}

// Replica select (sub == NULL) and scatter; the repack takes the same arguments.
// No rule among the written arrays themselves, only against the inputs.
inline int check_replica(const crdt_replica* rep, const crdt_replica* sub, const uint32_t* idx,
                         const crdt_replica_out* out, bool scatter) {
    if (!rep || !batch_ptrs_ok(rep->state) || !out || !out_ptrs_ok(out->state)) return CRDT_E_INVALID;
    if (scatter && (!sub || !batch_ptrs_ok(sub->state) || !idx || sub->state->R != rep->state->R))
        return CRDT_E_INVALID;
    Arrays w, in;
    w.add_out(out->state, 0, 0);
    if (out->tombs) w.add_tomb_out(out->tombs);
    w.add(out->doc_actor, 4);
    bool any_t = false;
    for (const crdt_replica* r : {rep, scatter ? sub : nullptr}) {
        if (!r) continue;
        if (r->tombs) {
            if (!tomb_batch_ok(r->tombs, false)) return CRDT_E_INVALID;
            any_t = true;
        }
        in.add_replica(r);
    }
    if (!off_inputs(w, in)) return CRDT_E_INVALID;
    if (any_t && !tomb_out_ok(out->tombs)) return CRDT_E_INVALID;
    return CRDT_OK;
}

// (the policies themselves are checked by api.cpp: headroom.hpp's headroom_ok)
inline int check_replica_repack(const crdt_replica* rep, const crdt_replica* sub, const uint32_t* idx, uint32_t n_out,
                                const crdt_replica_out* out) {
    if (sub && (!rep || !rep->state || n_out != rep->state->n_docs)) return CRDT_E_INVALID;
    return check_replica(rep, sub, idx, out, sub != nullptr);
}

inline int check_inplace(const crdt_replica_inplace* rep, const crdt_replica* sub, const uint32_t* idx,
                         const crdt_spill_out* spill) {
    if (!rep || !sub || !batch_ptrs_ok(sub->state) || !idx || !spill) return CRDT_E_INVALID;
    if (!spill->spill_j || !spill->spill_doc || !spill->n_spill) return CRDT_E_INVALID;
    if (!rep->offsets || !rep->counts || !rep->keys || !rep->actors || !rep->counters || !rep->vv)
        return CRDT_E_INVALID;
    if (rep->R != sub->state->R || rep->R == 0 || rep->R > CRDT_MAX_R) return CRDT_E_INVALID;
    if (sub->tombs && (!sub->tombs->offsets || !rep->tomb_offsets || !rep->tkeys || !rep->tactors || !rep->tcounters))
        return CRDT_E_INVALID;
    if (rep->tomb_offsets && !rep->tomb_counts) return CRDT_E_INVALID;
    // what the call writes of rep (its offsets are read only), against sub's arrays
    Arrays w, in;
    for (const uint32_t* p : {(const uint32_t*)rep->counts, (const uint32_t*)rep->actors,
                              (const uint32_t*)rep->tomb_counts, (const uint32_t*)rep->tactors,
                              (const uint32_t*)rep->doc_actor, (const uint32_t*)spill->spill_j,
                              (const uint32_t*)spill->spill_doc, (const uint32_t*)spill->n_spill})
        w.add(p, 4);
    for (const uint64_t* p : {(const uint64_t*)rep->keys, (const uint64_t*)rep->counters, (const uint64_t*)rep->vv,
                              (const uint64_t*)rep->tkeys, (const uint64_t*)rep->tcounters})
        w.add(p, 8);
    in.add_replica(sub);
    if (!off_inputs(w, in)) return CRDT_E_INVALID;
    return CRDT_OK;
}

inline int check_digest(const crdt_awset_batch* state, const crdt_tomb_batch* tombs, const uint64_t* digest) {
    if (!batch_ptrs_ok(state) || !digest || (tombs && !tomb_batch_ok(tombs, false))) return CRDT_E_INVALID;
    Arrays w, in;
    w.add(digest, 8);
    in.add_batch(state);
    in.add_tombs(tombs);
    // any_width: the digest word is refused on every input array, whatever its kind
    if (!off_inputs(w, in, true)) return CRDT_E_INVALID;
    return CRDT_OK;
}

// The worklist digest: check_digest's rules, the mode and its document counts, and
// the list against the same inputs.
inline int check_digest_idx(const crdt_awset_batch* state, const crdt_tomb_batch* tombs, const uint32_t* idx,
                            const uint32_t* n_idx, uint32_t n_max, uint32_t n_digest_docs, uint32_t mode,
                            const uint64_t* digest) {
    if (!batch_ptrs_ok(state) || !idx || !digest || (tombs && !tomb_batch_ok(tombs, false))) return CRDT_E_INVALID;
    if (mode > CRDT_DIGEST_PLACE) return CRDT_E_INVALID;
    if (mode == CRDT_DIGEST_GATHER ? n_digest_docs != state->n_docs : state->n_docs < n_max) return CRDT_E_INVALID;
    Arrays w, in, list;
    in.add_batch(state);
    in.add_tombs(tombs);
    list.add(idx, 4);
    // any_width, as check_digest: the list is refused on every array of the replica, whatever its kind
    if (!off_inputs(list, in, true)) return CRDT_E_INVALID;
    // the one written array, against the replica, the list and its length
    in.add(idx, 4);
    in.add(n_idx, 4);
    w.add(digest, 8);
    if (!off_inputs(w, in, true)) return CRDT_E_INVALID;
    return CRDT_OK;
}

// ---- digest trees ----------------------------------------------------------------

// The build: both arrays unless there are no documents, the tree off the digest array.
inline int check_digest_tree(const uint64_t* digest, uint32_t n_docs, const uint64_t* tree) {
    if (n_docs == 0) return CRDT_OK;
    if (!digest || !tree || tree == digest) return CRDT_E_INVALID;
    return CRDT_OK;
}

// The list of a children / diff call against its level: the identity form
// (parents == NULL) names parents 0 .. n_max - 1, all of which must be nodes.
inline bool digest_tree_list_ok(const uint64_t* level, uint32_t n_level, const uint32_t* parents, uint32_t n_max) {
    if (n_level && !level) return false;
    const uint64_t n_nodes = ((uint64_t)n_level + CRDT_DIGEST_TREE_FANOUT - 1) / CRDT_DIGEST_TREE_FANOUT;
    return parents || n_max <= n_nodes;
}

inline int check_digest_tree_children(const uint64_t* level, uint32_t n_level, const uint32_t* parents,
                                      const uint32_t* n_parents, uint32_t n_max, const uint64_t* out) {
    if (!out || !digest_tree_list_ok(level, n_level, parents, n_max)) return CRDT_E_INVALID;
    Arrays w, in;
    w.add(out, 8);
    in.add(level, 8);
    in.add(parents, 4);
    in.add(n_parents, 4);
    if (!off_inputs(w, in, true)) return CRDT_E_INVALID;
    return CRDT_OK;
}

// (flags_out and summary are optional)
inline int check_digest_tree_diff(const uint64_t* mine_level, uint32_t n_level, const uint64_t* theirs,
                                  const uint32_t* parents, const uint32_t* n_parents, uint32_t n_max, uint32_t mask,
                                  const uint32_t* idx_out, const uint8_t* flags_out, const uint32_t* n_out,
                                  const uint32_t* summary) {
    if (!idx_out || !n_out || (n_max && !theirs) || !digest_tree_list_ok(mine_level, n_level, parents, n_max))
        return CRDT_E_INVALID;
    if (mask == 0 || mask > 3u) return CRDT_E_INVALID;
    Arrays w, in;
    w.add(idx_out, 4);
    w.add(flags_out, 1);
    w.add(n_out, 4, 4);
    w.add(summary, 4, 5 * 4);
    in.add(mine_level, 8);
    in.add(theirs, 8);
    in.add(parents, 4);
    in.add(n_parents, 4);
    if (!starts_distinct(w) || !sized_disjoint(w) || !off_inputs(w, in, true)) return CRDT_E_INVALID;
    return CRDT_OK;
}

inline int check_compare(const crdt_awset_batch* a, const crdt_awset_batch* b, uint32_t mask,
                         const crdt_compare_out* out) {
    if (!batch_ptrs_ok(a) || !batch_ptrs_ok(b) || !compare_out_ok(out, mask)) return CRDT_E_INVALID;
    if (a->n_docs != b->n_docs || a->R != b->R) return CRDT_E_INVALID;
    return CRDT_OK;
}

inline int check_digest_diff(const uint64_t* mine, const uint64_t* theirs, uint32_t n_docs, uint32_t mask,
                             const crdt_compare_out* out) {
    if (!compare_out_ok(out, mask) || (n_docs && (!mine || !theirs))) return CRDT_E_INVALID;
    return CRDT_OK;
}

// crdt_diff_out against the two inputs (include/crdtgpu.h): required pointers,
// the dots of a list both or neither, and no out array starting where an input
// array of the same kind (or the other list's column) starts.
inline bool diff_out_ok(const crdt_diff_out* o, const crdt_awset_batch* before, const crdt_awset_batch* after,
                        uint32_t rem_slots, uint32_t ups_slots) {
    if (!o || !o->flags || !o->rem_off || !o->ups_off) return false;
    if ((rem_slots && !o->rem_keys) || (ups_slots && !o->ups_keys)) return false;
    if ((o->rem_actors == nullptr) != (o->rem_counters == nullptr)) return false;
    if ((o->ups_actors == nullptr) != (o->ups_counters == nullptr)) return false;
    if (o->rem_off == o->ups_off) return false;
    if (o->rem_keys && (o->rem_keys == o->ups_keys || o->rem_keys == o->rem_counters || o->rem_keys == o->ups_counters))
        return false;
    if (o->ups_keys && (o->ups_keys == o->rem_counters || o->ups_keys == o->ups_counters)) return false;
    if (o->rem_actors && o->rem_actors == o->ups_actors) return false;
    if (o->rem_counters && o->rem_counters == o->ups_counters) return false;
    Arrays w, in;
    for (const uint32_t* p : {(const uint32_t*)o->rem_off, (const uint32_t*)o->ups_off, (const uint32_t*)o->summary,
                              (const uint32_t*)o->rem_actors, (const uint32_t*)o->ups_actors})
        w.add(p, 4);
    for (const uint64_t* p : {(const uint64_t*)o->rem_keys, (const uint64_t*)o->ups_keys,
                              (const uint64_t*)o->rem_counters, (const uint64_t*)o->ups_counters})
        w.add(p, 8);
    in.add_batch(before);
    in.add_batch(after);
    return off_inputs(w, in);
}

inline int check_diff(const crdt_awset_batch* before, const crdt_awset_batch* after, uint32_t rem_slots,
                      uint32_t ups_slots, const crdt_diff_out* out) {
    if (!batch_ptrs_ok(before) || !batch_ptrs_ok(after)) return CRDT_E_INVALID;
    if (before->n_docs != after->n_docs || before->R != after->R) return CRDT_E_INVALID;
    return diff_out_ok(out, before, after, rem_slots, ups_slots) ? CRDT_OK : CRDT_E_INVALID;
}

inline int check_extract(const crdt_src_batch* srcs, const uint64_t* peer_vv, const crdt_delta_out* out) {
    if (!src_ptrs_ok(srcs) || (srcs->n_docs && !peer_vv)) return CRDT_E_INVALID;
    return delta_out_ok(out, srcs->tomb_off != nullptr) ? CRDT_OK : CRDT_E_INVALID;
}

// The membership reads, up to their early return at n_queries == 0 (api.cpp: after
// it, queries of no document are refused).
inline int check_queries(const crdt_query_batch* q, const crdt_query_out* out, uint32_t n_docs) {
    if (!q || !out || !q->q_off || !out->found || (q->n_queries && !q->keys) || q->n_docs != n_docs ||
        (out->actors == nullptr) != (out->counters == nullptr))
        return CRDT_E_INVALID;
    return CRDT_OK;
}

inline int check_has(const crdt_awset_batch* state, const crdt_query_batch* q, const crdt_query_out* out) {
    if (!state || !state->offsets || state->R == 0 || state->R > CRDT_MAX_R) return CRDT_E_INVALID;
    return check_queries(q, out, state->n_docs);  // (the clock is not read: vv may be NULL)
}

inline int check_tomb_has(const crdt_tomb_batch* tombs, uint32_t n_docs, const crdt_query_batch* q,
                          const crdt_query_out* out) {
    if (!tomb_batch_ok(tombs, false)) return CRDT_E_INVALID;
    return check_queries(q, out, n_docs);
}

inline int check_sort(const crdt_awset_batch* in, uint32_t n_slots, const crdt_awset_out* out) {
    if (!batch_ptrs_ok(in) || !out_ptrs_ok(out) || out->keys == in->keys) return CRDT_E_INVALID;
    if (n_slots && (!in->keys || !in->actors || !in->counters)) return CRDT_E_INVALID;
    return CRDT_OK;
}

}  // namespace crdt
