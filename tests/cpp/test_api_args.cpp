// Host test of the C ABI's argument checks (go-crdt-playground_amd/csrc/api_args.hpp),
// built with ASan + UBSan by host/Makefile (build/test_api_args) and run by
// tests/test_api_args.py.  No device, no libcrdtgpu.so.
//
// The checks read descriptors, never arrays, so every array address is taken from
// one static buffer and nothing is ever stored there.  Shapes: n_docs = 1, R = 1
// (offsets 8 bytes, counts 4, vv 8, flags 1, summary 20) and n_docs = 0.
//
// One table row per check_* family.  Each row is driven through the same cases:
//   baseline      all arrays distinct, back to back (p_j == p_i + bytes_i accepted)
//   NULLs         every required pointer NULL: refused; every optional one: accepted
//   pairs         every two written arrays starting at one address
//   overlap       two sized arrays one element inside each other / exactly adjacent
//   inputs        every written array on every input array
//   n_docs = 0    baseline, pairs, and an empty array inside a sized one
// What each family answers was read off the entry points as they stood before the
// checks moved into api_args.hpp (and off tests/test_gpu_*.py, which run the same
// rejects on a device); the families differ, and the rows say where.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <string>
#include <vector>

#include "../../go-crdt-playground_amd/csrc/api_args.hpp"

using namespace crdt;

namespace {

alignas(8) unsigned char g_buf[1 << 14];

enum Size { OFF, CNT, VV, FLG, SUM, ENT };  // ENT: an entry array, size unknown on the host

size_t bytes_of(Size k, size_t n) {
    switch (k) {
        case OFF: return (n + 1) * 4;
        case CNT: return n * 4;
        case VV: return n * 8;  // R = 1
        case FLG: return n;
        case SUM: return 20;
        default: return 0;
    }
}

// Every descriptor a check can take, filled by fresh().
struct World {
    crdt_awset_batch A, B;
    crdt_tomb_batch TA, TB;
    const uint32_t *daA, *daB, *idx;
    crdt_replica RA, RB, reps[2];
    crdt_awset_out O1, O2;
    crdt_merge_log L1, L2;
    uint8_t *k1, *k2;
    crdt_tomb_out TO;
    crdt_op_batch OPS;
    crdt_src_batch S;
    crdt_delta_out DO;
    uint32_t* daO;
    crdt_replica_out RO;
    crdt_replica_inplace IP;
    crdt_spill_out SP;
    crdt_compare_out CO;
    crdt_diff_out DF;
    crdt_query_batch Q;
    crdt_query_out QO;
    uint64_t* digest;
    const uint64_t *peer, *mine, *theirs;
} W;

struct Field {  // one array pointer of W
    const char* name;
    void* at;  // address of the pointer field
    Size size;
    int width;
};
#define F(x, size, width) Field{#x, (void*)&W.x, size, width}

void* get(const Field& f) {
    void* p;
    memcpy(&p, f.at, sizeof p);
    return p;
}
void set(const Field& f, const void* p) { memcpy(f.at, &p, sizeof p); }

std::vector<Field> batch(crdt_awset_batch& b) {
    return {Field{"offsets", &b.offsets, OFF, 4}, Field{"counts", &b.counts, CNT, 4}, Field{"keys", &b.keys, ENT, 8},
            Field{"actors", &b.actors, ENT, 4},   Field{"counters", &b.counters, ENT, 8}, Field{"vv", &b.vv, VV, 8}};
}
std::vector<Field> tombs(crdt_tomb_batch& t) {
    return {Field{"t.offsets", &t.offsets, OFF, 4}, Field{"t.counts", &t.counts, CNT, 4},
            Field{"t.keys", &t.keys, ENT, 8},       Field{"t.actors", &t.actors, ENT, 4},
            Field{"t.counters", &t.counters, ENT, 8}};
}
std::vector<Field> out(crdt_awset_out& o) {
    return {Field{"offsets", &o.offsets, OFF, 4}, Field{"counts", &o.counts, CNT, 4}, Field{"vv", &o.vv, VV, 8},
            Field{"keys", &o.keys, ENT, 8},       Field{"actors", &o.actors, ENT, 4}, Field{"counters", &o.counters, ENT, 8}};
}
std::vector<Field> tomb_out(crdt_tomb_out& t) {
    return {Field{"to.offsets", &t.offsets, ENT, 4}, Field{"to.counts", &t.counts, ENT, 4},
            Field{"to.keys", &t.keys, ENT, 8},       Field{"to.actors", &t.actors, ENT, 4},
            Field{"to.counters", &t.counters, ENT, 8}};
}
std::vector<Field> log_req(crdt_merge_log& l) {
    return {Field{"flags", &l.flags, FLG, 1},
            Field{"rem_offsets", &l.rem_offsets, OFF, 4},
            Field{"rem_counts", &l.rem_counts, CNT, 4},
            Field{"ups_offsets", &l.ups_offsets, OFF, 4},
            Field{"ups_counts", &l.ups_counts, CNT, 4},
            Field{"rem_keys", &l.rem_keys, ENT, 8},
            Field{"rem_actors", &l.rem_actors, ENT, 4},
            Field{"rem_counters", &l.rem_counters, ENT, 8},
            Field{"ups_keys", &l.ups_keys, ENT, 8},
            Field{"ups_actors", &l.ups_actors, ENT, 4},
            Field{"ups_counters", &l.ups_counters, ENT, 8}};
}
std::vector<Field> log_opt(crdt_merge_log& l) {
    return {Field{"summary", &l.summary, SUM, 4}, Field{"ups_kind", &l.ups_kind, ENT, 1}};
}
std::vector<Field> srcs_fields() {
    return {F(S.doc_srcs, ENT, 4), F(S.src_actor, ENT, 4), F(S.vv, ENT, 8),     F(S.entry_off, ENT, 4),
            F(S.keys, ENT, 8),     F(S.actors, ENT, 4),    F(S.counters, ENT, 8), F(S.tomb_off, ENT, 4),
            F(S.tkeys, ENT, 8),    F(S.tactors, ENT, 4),   F(S.tcounters, ENT, 8)};
}
std::vector<Field> delta_out_fields() {
    return {F(DO.doc_srcs, ENT, 4), F(DO.src_actor, ENT, 4), F(DO.vv, ENT, 8),       F(DO.entry_off, ENT, 4),
            F(DO.keys, ENT, 8),     F(DO.actors, ENT, 4),    F(DO.counters, ENT, 8), F(DO.tomb_off, ENT, 4),
            F(DO.tkeys, ENT, 8),    F(DO.tactors, ENT, 4),   F(DO.tcounters, ENT, 8)};
}

std::vector<Field> operator+(std::vector<Field> a, const std::vector<Field>& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}

// Every array of W, in layout order: related per-document arrays are neighbours.
std::vector<Field> all_fields() {
    std::vector<Field> v = batch(W.A) + batch(W.B) + tombs(W.TA) + tombs(W.TB);
    v = v + std::vector<Field>{F(daA, CNT, 4), F(daB, CNT, 4), F(idx, CNT, 4)};
    v = v + out(W.O1) + log_req(W.L1) + log_opt(W.L1) + std::vector<Field>{F(k1, FLG, 1)};
    v = v + out(W.O2) + log_req(W.L2) + log_opt(W.L2) + std::vector<Field>{F(k2, FLG, 1)};
    v = v + tomb_out(W.TO) + srcs_fields() + delta_out_fields();
    v = v + std::vector<Field>{F(DO.kind, ENT, 1),       F(OPS.op_off, OFF, 4),    F(OPS.kind, ENT, 1),
                               F(OPS.keys, ENT, 8),      F(OPS.doc_actor, CNT, 4), F(daO, CNT, 4),
                               F(IP.offsets, OFF, 4),    F(IP.counts, CNT, 4),     F(IP.keys, ENT, 8),
                               F(IP.actors, ENT, 4),     F(IP.counters, ENT, 8),   F(IP.vv, VV, 8),
                               F(IP.tomb_offsets, OFF, 4), F(IP.tomb_counts, CNT, 4), F(IP.tkeys, ENT, 8),
                               F(IP.tactors, ENT, 4),    F(IP.tcounters, ENT, 8),  F(IP.doc_actor, CNT, 4),
                               F(SP.spill_j, ENT, 4),    F(SP.spill_doc, ENT, 4),  F(SP.n_spill, ENT, 4),
                               F(CO.flags, FLG, 1),      F(CO.summary, SUM, 4),    F(CO.worklist, CNT, 4),
                               F(CO.n_work, ENT, 4),     F(DF.flags, FLG, 1),      F(DF.summary, SUM, 4),
                               F(DF.rem_off, OFF, 4),    F(DF.rem_keys, ENT, 8),   F(DF.rem_actors, ENT, 4),
                               F(DF.rem_counters, ENT, 8), F(DF.ups_off, OFF, 4),  F(DF.ups_keys, ENT, 8),
                               F(DF.ups_actors, ENT, 4), F(DF.ups_counters, ENT, 8), F(DF.ups_kind, ENT, 1),
                               F(Q.q_off, OFF, 4),       F(Q.keys, ENT, 8),        F(QO.found, ENT, 1),
                               F(QO.actors, ENT, 4),     F(QO.counters, ENT, 8),   F(digest, ENT, 8),
                               F(peer, VV, 8),           F(mine, ENT, 8),          F(theirs, ENT, 8)};
    return v;
}

size_t g_n = 1;          // n_docs of the current world
unsigned char* g_spare;  // free space behind the last array

// The accepted baseline: every array distinct, back to back (an array whose size is
// zero or unknown still gets 8 bytes, so that its start is its own).
void fresh(size_t n) {
    g_n = n;
    memset(&W, 0, sizeof W);
    unsigned char* p = g_buf;
    for (const Field& f : all_fields()) {
        set(f, p);
        const size_t b = bytes_of(f.size, n);
        p += b ? b : 8;
    }
    g_spare = p + 64;
    W.A.n_docs = W.B.n_docs = W.OPS.n_docs = W.S.n_docs = W.IP.n_docs = W.Q.n_docs = (uint32_t)n;
    W.A.R = W.B.R = W.S.R = W.IP.R = 1;
    W.Q.n_queries = 1;
    W.RA = crdt_replica{&W.A, &W.TA, W.daA, 0};
    W.RB = crdt_replica{&W.B, &W.TB, W.daB, 1};
    W.RO = crdt_replica_out{&W.O1, &W.TO, W.daO};
}

void sync_replicas() {  // the descriptors that copy array pointers of W
    W.RA.doc_actor = W.daA;
    W.RB.doc_actor = W.daB;
    W.RO.doc_actor = W.daO;
    W.reps[0] = W.RA;
    W.reps[1] = W.RB;
}

struct Extra {
    const char* what;
    std::function<void()> change;
    bool ok;
};

struct Family {
    const char* name;
    std::function<int()> run;
    std::vector<Field> written_req, written_opt, inputs_req, inputs_opt;
    // two written arrays (by name, in list order) may start at one address
    std::function<bool(const std::string&, const std::string&)> pair_ok;
    bool overlap_rule;  // sized written arrays must not overlap
    // a written array may start on an input array
    std::function<bool(const Field&, const Field&)> input_ok;
    std::vector<Extra> extras;
};

int g_cases = 0, g_failed = 0;

void expect(const Family& f, bool ok, const std::string& what) {
    sync_replicas();
    const int rc = f.run();
    ++g_cases;
    if (rc != CRDT_OK && rc != CRDT_E_INVALID) {
        printf("FAIL %s: %s: code %d\n", f.name, what.c_str(), rc);
        ++g_failed;
    } else if ((rc == CRDT_OK) != ok) {
        printf("FAIL %s [n_docs=%zu]: %s: %s, want %s\n", f.name, g_n, what.c_str(), rc == CRDT_OK ? "accepted" : "refused",
               ok ? "accepted" : "refused");
        ++g_failed;
    }
}

const auto never = [](const std::string&, const std::string&) { return false; };
const auto always = [](const std::string&, const std::string&) { return true; };
const auto any_input = [](const Field&, const Field&) { return true; };
const auto other_width = [](const Field& w, const Field& in) { return w.width != in.width; };
std::string base(const std::string& s) { return s.substr(s.find_last_of('.') == std::string::npos ? 0 : s.find_last_of('.') + 1); }

void drive(const Family& f) {
    for (size_t n : {(size_t)1, (size_t)0}) {
        fresh(n);
        expect(f, true, "baseline");
        const std::vector<Field> wr = f.written_req + f.written_opt;
        const std::vector<Field> in = f.inputs_req + f.inputs_opt;
        if (n == 1) {
            for (const auto* list : {&f.written_req, &f.inputs_req})
                for (const Field& x : *list) {
                    fresh(n);
                    set(x, nullptr);
                    expect(f, false, std::string("NULL ") + x.name);
                }
            for (const auto* list : {&f.written_opt, &f.inputs_opt})
                for (const Field& x : *list) {
                    fresh(n);
                    set(x, nullptr);
                    expect(f, true, std::string("NULL ") + x.name);
                }
        }
        for (size_t i = 0; i < wr.size(); ++i)
            for (size_t j = i + 1; j < wr.size(); ++j) {
                fresh(n);
                set(wr[j], get(wr[i]));
                expect(f, f.pair_ok(wr[i].name, wr[j].name), std::string(wr[j].name) + " = " + wr[i].name);
            }
        for (size_t i = 0; i < wr.size(); ++i)
            for (size_t j = 0; j < wr.size(); ++j) {
                const size_t bi = bytes_of(wr[i].size, 1), bj = bytes_of(wr[j].size, 1);
                if (i == j || !bi || !bj) continue;
                if (n == 1) {
                    const size_t inside = bi >= 8 ? 4 : bi - 1;  // one word inside offsets / vv / summary
                    fresh(n);
                    set(wr[i], g_spare);
                    set(wr[j], g_spare + bi);
                    expect(f, true, std::string(wr[j].name) + " right behind " + wr[i].name);
                    if (!inside) continue;
                    set(wr[j], g_spare + inside);
                    expect(f, !f.overlap_rule, std::string(wr[j].name) + " inside " + wr[i].name);
                } else if (bytes_of(wr[i].size, 0) && !bytes_of(wr[j].size, 0)) {
                    fresh(n);  // an empty array takes part in the start rule only
                    set(wr[j], (unsigned char*)get(wr[i]) + 2);
                    expect(f, true, std::string("empty ") + wr[j].name + " inside " + wr[i].name);
                }
            }
        for (const Field& w : wr)
            for (const Field& x : in) {
                fresh(n);
                set(w, get(x));
                expect(f, f.input_ok(w, x), std::string(w.name) + " on input " + x.name);
            }
        if (n == 1)
            for (const Extra& e : f.extras) {
                fresh(n);
                e.change();
                expect(f, e.ok, e.what);
            }
    }
}

std::deque<std::string> g_names;  // (a deque: the names the fields point to never move)
std::vector<Field> named(const char* pre, std::vector<Field> v) {
    for (Field& f : v) {
        g_names.push_back(std::string(pre) + "." + f.name);
        f.name = g_names.back().c_str();
    }
    return v;
}
std::vector<Field> pick(const std::vector<Field>& v, std::initializer_list<int> idx) {
    std::vector<Field> r;
    for (int i : idx) r.push_back(v[i]);
    return r;
}

std::vector<Family> table() {
    const auto A = named("a", batch(W.A)), B = named("b", batch(W.B));
    const auto A_req = pick(A, {0, 5}), A_opt = pick(A, {1, 2, 3, 4});  // offsets, vv (n_docs > 0) required
    const auto B_req = pick(B, {0, 5}), B_opt = pick(B, {1, 2, 3, 4});
    const auto TA = named("a", tombs(W.TA)), TB = named("b", tombs(W.TB));
    const auto TA_req = pick(TA, {0}), TA_opt = pick(TA, {1, 2, 3, 4});
    const auto TB_req = pick(TB, {0}), TB_opt = pick(TB, {1, 2, 3, 4});
    const auto O1 = named("ab", out(W.O1)), O2 = named("ba", out(W.O2));
    const auto L1 = named("lab", log_req(W.L1)), L2 = named("lba", log_req(W.L2));
    const auto L1o = named("lab", log_opt(W.L1)), L2o = named("lba", log_opt(W.L2));
    const auto TO = tomb_out(W.TO);
    const std::vector<Field> K1{F(k1, FLG, 1)}, K2{F(k2, FLG, 1)}, DA{F(daA, CNT, 4)}, DB{F(daB, CNT, 4)};
    const std::vector<Field> K1u{F(k1, ENT, 1)}, K2u{F(k2, ENT, 1)};  // the unlogged pair does not size the kinds
    const auto S = srcs_fields();
    const auto S_req = pick(S, {0, 1, 3, 8, 9, 10}), S_opt = pick(S, {2, 4, 5, 6, 7});  // tomb_off set: its columns too
    const auto DO = delta_out_fields();
    const auto same_field = [](const Field& w, const Field& in) { return base(w.name) != base(in.name); };
    std::vector<Family> t;

    // Plain join: required pointers and matching shapes, no aliasing rule of any kind.
    t.push_back({"join", [] { return check_join(&W.A, &W.B, &W.O1, nullptr); }, O1, {}, A_req + B_req, A_opt + B_opt,
                 always, false, any_input,
                 {{"n_docs differ", [] { W.B.n_docs = 2; }, false},
                  {"R differ", [] { W.B.R = 2; }, false},
                  {"R = 0", [] { W.A.R = W.B.R = 0; }, false},
                  {"R = 65", [] { W.A.R = W.B.R = 65; }, false},
                  {"R = 64", [] { W.A.R = W.B.R = 64; }, true},
                  {"dst NULL", [] { W.A.offsets = nullptr; }, false}}});
    // Plain exchange: starts and sized overlaps among the twelve outputs, the shared
    // key column excepted (the logged and the delta exchanges refuse it); like the
    // join, an output on an input is accepted.
    t.push_back({"exchange", [] { return check_exchange(&W.A, &W.B, &W.O1, &W.O2); }, O1 + O2, {}, A_req + B_req,
                 A_opt + B_opt,
                 [](const std::string& x, const std::string& y) { return x == "ab.keys" && y == "ba.keys"; }, true,
                 any_input,
                 {{"out_ba keys = out_ab counters", [] { W.O2.keys = (uint64_t*)W.O1.counters; }, false}}});
    t.push_back({"fold_log", [] { return check_fold_log(CRDT_FOLD_DELTA, &W.A, &W.S, &W.O1, &W.L1); }, O1 + L1, L1o,
                 A_req + S_req, A_opt + S_opt, never, true, other_width,
                 {{"R differ", [] { W.S.R = 2; }, false},
                  {"n_docs differ", [] { W.S.n_docs = 2; }, false},
                  {"no tombstones", [] { W.S.tomb_off = nullptr; W.S.tkeys = nullptr; W.S.tactors = nullptr; W.S.tcounters = nullptr; }, true}}});
    t.push_back({"fold_log bad mode", [] { return check_fold_log(2, &W.A, &W.S, &W.O1, &W.L1) == CRDT_E_INVALID ? CRDT_OK : CRDT_E_ACTOR_RANGE; },
                 {}, {}, {}, {}, always, false, any_input, {}});
    // Logged join / exchange: every start distinct (the shared key column too),
    // sized overlaps, and the same-kind input rule.
    t.push_back({"join_log", [] { return check_join_log(&W.A, &W.B, &W.O1, nullptr, &W.L1, nullptr, false); }, O1 + L1,
                 L1o, A_req + B_req, A_opt + B_opt, never, true, other_width, {}});
    t.push_back({"exchange_log", [] { return check_join_log(&W.A, &W.B, &W.O1, &W.O2, &W.L1, &W.L2, true); },
                 O1 + L1 + O2 + L2, L1o + L2o, A_req + B_req, A_opt + B_opt, never, true, other_width, {}});
    t.push_back({"exchange_log without out_ba",
                 [] { return check_join_log(&W.A, &W.B, &W.O1, nullptr, &W.L1, &W.L2, true) == CRDT_E_INVALID ? CRDT_OK : CRDT_E_ACTOR_RANGE; },
                 {}, {}, {}, {}, always, false, any_input, {}});
    t.push_back({"exchange_log without log_ba",
                 [] { return check_join_log(&W.A, &W.B, &W.O1, &W.O2, &W.L1, nullptr, true) == CRDT_E_INVALID ? CRDT_OK : CRDT_E_ACTOR_RANGE; },
                 {}, {}, {}, {}, always, false, any_input, {}});
    // Delta pair, unlogged: the kinds are compared with each other only (kind_ab ==
    // kind_ba refused, a kind on an output array accepted); the logged pair lists them
    // as written arrays of n_docs bytes.
    const auto kinds_apart = [](const std::string& x, const std::string& y) {
        return (x == "k1" || x == "k2" || y == "k1" || y == "k2") && !(x == "k1" && y == "k2");
    };
    t.push_back({"delta_join", [] { return check_delta_pair(&W.A, nullptr, nullptr, &W.RB, &W.O1, nullptr, W.k1, nullptr); },
                 O1, K1u, A_req + B_req + TB_req, A_opt + B_opt + TB_opt + DB, kinds_apart, true,
                 [](const Field& w, const Field& in) { return w.width == 1 || w.width != in.width; },
                 {{"src NULL state", [] { W.RB.state = nullptr; }, false},
                  {"src no tombs", [] { W.RB.tombs = nullptr; }, true},
                  {"n_docs differ", [] { W.B.n_docs = 2; }, false}}});
    t.push_back({"delta_exchange", [] { return check_delta_exchange(&W.RA, &W.RB, &W.O1, &W.O2, W.k1, W.k2); }, O1 + O2,
                 K1u + K2u, A_req + B_req + TA_req + TB_req, A_opt + B_opt + TA_opt + TB_opt + DA + DB, kinds_apart, true,
                 [](const Field& w, const Field& in) { return w.width == 1 || w.width != in.width; },
                 {{"a no tombs", [] { W.RA.tombs = nullptr; }, true},
                  {"a NULL state", [] { W.RA.state = nullptr; }, false}}});
    t.push_back({"delta_exchange NULL a / out_ba",
                 [] {
                     return check_delta_exchange(nullptr, &W.RB, &W.O1, &W.O2, W.k1, W.k2) == CRDT_E_INVALID &&
                                    check_delta_exchange(&W.RA, nullptr, &W.O1, &W.O2, W.k1, W.k2) == CRDT_E_INVALID &&
                                    check_delta_exchange(&W.RA, &W.RB, &W.O1, nullptr, W.k1, W.k2) == CRDT_E_INVALID
                                ? CRDT_OK
                                : CRDT_E_ACTOR_RANGE;
                 },
                 {}, {}, {}, {}, always, false, any_input, {}});
    t.push_back({"delta_join_log",
                 [] { return check_delta_pair_log(&W.A, nullptr, nullptr, &W.RB, &W.O1, nullptr, W.k1, nullptr, &W.L1, nullptr); },
                 O1 + L1, L1o + K1, A_req + B_req + TB_req, A_opt + B_opt + TB_opt + DB, never, true, other_width,
                 // (the join reads nothing of a beyond its state: a's tombstones are no input)
                 {{"rem_counts on a's tomb actors", [] { W.L1.rem_counts = (uint32_t*)W.TA.actors; }, true}}});
    t.push_back({"delta_exchange_log",
                 [] { return check_delta_exchange_log(&W.RA, &W.RB, &W.O1, &W.O2, W.k1, W.k2, &W.L1, &W.L2); },
                 O1 + L1 + O2 + L2, L1o + K1 + L2o + K2, A_req + B_req + TA_req + TB_req,
                 A_opt + B_opt + TA_opt + TB_opt + DA + DB, never, true, other_width, {}});
    t.push_back({"delta_exchange_log NULL a / out_ba / log_ba",
                 [] {
                     return check_delta_exchange_log(nullptr, &W.RB, &W.O1, &W.O2, W.k1, W.k2, &W.L1, &W.L2) == CRDT_E_INVALID &&
                                    check_delta_exchange_log(&W.RA, &W.RB, &W.O1, nullptr, W.k1, W.k2, &W.L1, &W.L2) == CRDT_E_INVALID &&
                                    check_delta_exchange_log(&W.RA, &W.RB, &W.O1, &W.O2, W.k1, W.k2, &W.L1, nullptr) == CRDT_E_INVALID
                                ? CRDT_OK
                                : CRDT_E_ACTOR_RANGE;
                 },
                 {}, {}, {}, {}, always, false, any_input, {}});
    // Apply: no aliasing rule.  Logged apply: starts only -- a sized overlap is
    // accepted here and refused by the logged join, fold and delta pair -- and the
    // only call whose 1-byte arrays (flags, ups_kind) meet a 1-byte input (ops->kind).
    const std::vector<Field> OPS_req{F(OPS.op_off, OFF, 4), F(OPS.doc_actor, CNT, 4)},
        OPS_opt{F(OPS.kind, ENT, 1), F(OPS.keys, ENT, 8)};
    const auto TA_cols = pick(TA, {0, 2, 3, 4}), TA_cnt = pick(TA, {1});  // apply reads the columns: required
    t.push_back({"apply", [] { return check_apply(&W.A, &W.TA, &W.OPS, &W.O1, &W.TO); }, O1 + TO, {},
                 A_req + TA_cols + OPS_req, A_opt + TA_cnt + OPS_opt, always, false, any_input,
                 {{"ops n_docs differ", [] { W.OPS.n_docs = 2; }, false}}});
    t.push_back({"apply no tombs", [] { return check_apply(&W.A, nullptr, &W.OPS, &W.O1, nullptr); }, O1, {},
                 A_req + OPS_req, A_opt + OPS_opt, always, false, any_input, {}});
    t.push_back({"apply_log", [] { return check_apply_log(&W.A, &W.TA, &W.OPS, &W.O1, &W.TO, &W.L1); }, O1 + L1 + TO, L1o,
                 A_req + TA_cols + OPS_req, A_opt + TA_cnt + OPS_opt, never, false, other_width, {}});
    t.push_back({"apply_log no tombs", [] { return check_apply_log(&W.A, nullptr, &W.OPS, &W.O1, nullptr, &W.L1); },
                 O1 + L1, L1o, A_req + OPS_req, A_opt + OPS_opt, never, false, other_width,
                 {{"tomb_out arrays are not written", [] { W.TO.keys = W.O1.keys; }, true}}});
    // Select, scatter, sort, sources: field by field (out->offsets against the input's
    // offsets only), no rule among the outputs.
    t.push_back({"select", [] { return check_select(&W.A, &W.O1); }, O1, {}, A_req, A_opt, always, false, same_field, {}});
    t.push_back({"scatter", [] { return check_scatter(&W.A, &W.B, W.idx, &W.O1); }, O1, {}, A_req + B_req, A_opt + B_opt,
                 always, false, same_field,
                 {{"idx NULL", [] { W.idx = nullptr; }, false}, {"R differ", [] { W.B.R = 2; }, false},
                  {"n_docs differ", [] { W.B.n_docs = 7; }, true}}});
    t.push_back({"sort", [] { return check_sort(&W.A, 1, &W.O1); }, O1, {}, pick(A, {0, 2, 3, 4, 5}), pick(A, {1}), always, false,
                 [](const Field& w, const Field& in) { return !(std::string(w.name) == "ab.keys" && std::string(in.name) == "a.keys"); },
                 {}});
    t.push_back({"sort no slots", [] { return check_sort(&W.A, 0, &W.O1); }, O1, {}, A_req, A_opt, always, false,
                 [](const Field& w, const Field& in) { return !(std::string(w.name) == "ab.keys" && std::string(in.name) == "a.keys"); },
                 {}});
    const auto src_on = [](const Field& w, const Field& in) {
        static const char* const pairs[][2] = {{"entry_off", "offsets"}, {"keys", "keys"}, {"actors", "actors"},
                                               {"counters", "counters"}, {"vv", "vv"}, {"src_actor", "daA"},
                                               {"src_actor", "daB"}, {"tomb_off", "t.offsets"}, {"tkeys", "t.keys"},
                                               {"tactors", "t.actors"}, {"tcounters", "t.counters"}};
        const std::string wn = base(w.name);
        std::string in_n = in.name;
        if (in_n.rfind("a.", 0) == 0 || in_n.rfind("b.", 0) == 0) in_n = in_n.substr(2);
        for (const auto& p : pairs)
            if (wn == p[0] && in_n == p[1]) return false;
        return true;
    };
    t.push_back({"sources", [] { return check_sources(W.reps, 2, &W.DO); }, DO, {F(DO.kind, ENT, 1)},
                 A_req + B_req + TA_req + TB_req, A_opt + B_opt + TA_opt + TB_opt + DA + DB, always, false, src_on,
                 {{"no tombs: no tomb columns", [] { W.RA.tombs = W.RB.tombs = nullptr; W.DO.tomb_off = nullptr; W.DO.tkeys = nullptr; }, true},
                  {"replicas differ in R", [] { W.B.R = 2; }, false},
                  {"replicas differ in n_docs", [] { W.B.n_docs = 2; }, false},
                  {"a state NULL", [] { W.RA.state = nullptr; }, false}}});
    t.push_back({"sources n_reps",
                 [] {
                     return check_sources(W.reps, 0, &W.DO) == CRDT_E_INVALID && check_sources(nullptr, 2, &W.DO) == CRDT_E_INVALID &&
                                    check_sources(W.reps, CRDT_MAX_REPLICAS + 1, &W.DO) == CRDT_E_INVALID &&
                                    check_sources(W.reps, 2, nullptr) == CRDT_E_INVALID
                                ? CRDT_OK
                                : CRDT_E_ACTOR_RANGE;
                 },
                 {}, {}, {}, {}, always, false, any_input, {}});
    // Replica select / scatter / repack and the in-place scatter: the same-kind input
    // rule, and no rule among the written arrays.
    const std::vector<Field> DAO{F(daO, CNT, 4)};
    t.push_back({"replica_select", [] { return check_replica(&W.RA, nullptr, W.idx, &W.RO, false); }, O1 + TO, DAO,
                 A_req + TA_req, A_opt + TA_opt + DA, always, false, other_width,
                 {{"idx NULL", [] { W.idx = nullptr; }, true},
                  {"tombs in, none out", [] { W.RO.tombs = nullptr; }, false},
                  {"no tombs in, none out", [] { W.RA.tombs = nullptr; W.RO.tombs = nullptr; }, true},
                  {"no tombs in, partial out", [] { W.RA.tombs = nullptr; W.TO.keys = nullptr; }, true}}});
    t.push_back({"replica_scatter", [] { return check_replica(&W.RA, &W.RB, W.idx, &W.RO, true); }, O1 + TO, DAO,
                 A_req + B_req + TA_req + TB_req, A_opt + B_opt + TA_opt + TB_opt + DA + DB, always, false, other_width,
                 {{"idx NULL", [] { W.idx = nullptr; }, false},
                  {"R differ", [] { W.B.R = 2; }, false},
                  {"sub tombs only, none out", [] { W.RA.tombs = nullptr; W.RO.tombs = nullptr; }, false}}});
    t.push_back({"replica_repack", [] { return check_replica_repack(&W.RA, &W.RB, W.idx, (uint32_t)g_n, &W.RO); },
                 O1 + TO, DAO, A_req + B_req + TA_req + TB_req, A_opt + B_opt + TA_opt + TB_opt + DA + DB, always, false,
                 other_width, {}});
    t.push_back({"replica_repack n_out",
                 [] {
                     return check_replica_repack(&W.RA, &W.RB, W.idx, (uint32_t)g_n + 1, &W.RO) == CRDT_E_INVALID &&
                                    check_replica_repack(&W.RA, nullptr, W.idx, (uint32_t)g_n + 1, &W.RO) == CRDT_OK &&
                                    check_replica_repack(nullptr, &W.RB, W.idx, 0, &W.RO) == CRDT_E_INVALID
                                ? CRDT_OK
                                : CRDT_E_ACTOR_RANGE;
                 },
                 {}, {}, {}, {}, always, false, any_input, {}});
    const std::vector<Field> IPw{F(IP.counts, ENT, 4),  F(IP.keys, ENT, 8),    F(IP.actors, ENT, 4), F(IP.counters, ENT, 8),
                                 F(IP.vv, ENT, 8),      F(IP.tomb_counts, ENT, 4), F(IP.tkeys, ENT, 8), F(IP.tactors, ENT, 4),
                                 F(IP.tcounters, ENT, 8), F(SP.spill_j, ENT, 4), F(SP.spill_doc, ENT, 4), F(SP.n_spill, ENT, 4)};
    t.push_back({"inplace", [] { return check_inplace(&W.IP, &W.RB, W.idx, &W.SP); }, IPw, {F(IP.doc_actor, ENT, 4)},
                 B_req + TB_req, B_opt + TB_opt + DB, always, false, other_width,
                 {{"offsets NULL", [] { W.IP.offsets = nullptr; }, false},
                  {"tomb_offsets NULL, sub has tombs", [] { W.IP.tomb_offsets = nullptr; }, false},
                  {"the offsets are read, not written: may start on an input", [] { W.IP.offsets = W.B.offsets; W.IP.tomb_offsets = W.TB.offsets; }, true},
                  {"no tombs anywhere", [] { W.RB.tombs = nullptr; W.IP.tomb_offsets = nullptr; W.IP.tomb_counts = nullptr; W.IP.tkeys = nullptr; }, true},
                  {"idx NULL", [] { W.idx = nullptr; }, false},
                  {"R differ", [] { W.IP.R = 2; }, false},
                  {"R = 65", [] { W.IP.R = W.B.R = 65; }, false}}});
    // Digest: the digest word is refused on every input array, whatever its width.
    t.push_back({"digest", [] { return check_digest(&W.A, &W.TA, W.digest); }, {F(digest, ENT, 8)}, {}, A_req + TA_req,
                 A_opt + TA_opt, always, false, [](const Field&, const Field&) { return false; }, {}});
    t.push_back({"digest no tombs", [] { return check_digest(&W.A, nullptr, W.digest); }, {F(digest, ENT, 8)}, {}, A_req,
                 A_opt, always, false, [](const Field&, const Field&) { return false; },
                 {{"a tomb array is no input then", [] { W.digest = (uint64_t*)W.TA.keys; }, true}}});
    const std::vector<Field> COr{F(CO.flags, FLG, 1)}, COo{F(CO.summary, SUM, 4)};
    const std::vector<Extra> co_extras{{"worklist without n_work", [] { W.CO.n_work = nullptr; }, false},
                                       {"n_work without worklist", [] { W.CO.worklist = nullptr; }, false},
                                       {"neither", [] { W.CO.worklist = W.CO.n_work = nullptr; }, true}};
    for (uint32_t mask : {0u, 15u})
        t.push_back({"compare", [mask] { return check_compare(&W.A, &W.B, mask, &W.CO); }, COr, COo, A_req + B_req,
                     A_opt + B_opt, always, false, any_input, co_extras});
    t.push_back({"compare mask 16", [] { return check_compare(&W.A, &W.B, 16, &W.CO) == CRDT_E_INVALID ? CRDT_OK : CRDT_E_ACTOR_RANGE; },
                 {}, {}, {}, {}, always, false, any_input, {}});
    t.push_back({"digest_diff", [] { return check_digest_diff(W.mine, W.theirs, (uint32_t)g_n, 15, &W.CO); }, COr, COo, {},
                 {}, always, false, any_input, co_extras});
    t.push_back({"digest_diff NULL digests",
                 [] {
                     const bool ok0 = check_digest_diff(nullptr, nullptr, 0, 0, &W.CO) == CRDT_OK;
                     const bool bad = check_digest_diff(nullptr, W.theirs, 1, 0, &W.CO) == CRDT_E_INVALID &&
                                      check_digest_diff(W.mine, nullptr, 1, 0, &W.CO) == CRDT_E_INVALID &&
                                      check_digest_diff(W.mine, W.theirs, 1, 16, &W.CO) == CRDT_E_INVALID;
                     return ok0 && bad ? CRDT_OK : CRDT_E_ACTOR_RANGE;
                 },
                 {}, {}, {}, {}, always, false, any_input, {}});
    // Diff: the pairs the header names, not every pair; the dots of a list both or neither.
    const std::vector<Field> DFr{F(DF.flags, ENT, 1),      F(DF.rem_off, ENT, 4),      F(DF.rem_keys, ENT, 8),
                                 F(DF.rem_actors, ENT, 4), F(DF.rem_counters, ENT, 8), F(DF.ups_off, ENT, 4),
                                 F(DF.ups_keys, ENT, 8),   F(DF.ups_actors, ENT, 4),   F(DF.ups_counters, ENT, 8)};
    const std::vector<Field> DFo{F(DF.summary, ENT, 4), F(DF.ups_kind, ENT, 1)};
    const auto diff_pair = [](const std::string& x, const std::string& y) {
        static const char* const bad[][2] = {{"DF.rem_off", "DF.ups_off"},           {"DF.rem_keys", "DF.ups_keys"},
                                             {"DF.rem_keys", "DF.rem_counters"},     {"DF.rem_keys", "DF.ups_counters"},
                                             {"DF.rem_counters", "DF.ups_keys"},     {"DF.ups_keys", "DF.ups_counters"},
                                             {"DF.rem_actors", "DF.ups_actors"},     {"DF.rem_counters", "DF.ups_counters"}};
        for (const auto& p : bad)
            if (x == p[0] && y == p[1]) return false;
        return true;
    };
    t.push_back({"diff", [] { return check_diff(&W.A, &W.B, 1, 1, &W.DF); }, DFr, DFo, A_req + B_req, A_opt + B_opt, diff_pair,
                 false, other_width,
                 {{"no dots", [] { W.DF.rem_actors = nullptr; W.DF.rem_counters = nullptr; W.DF.ups_actors = nullptr; W.DF.ups_counters = nullptr; }, true},
                  {"n_docs differ", [] { W.B.n_docs = 2; }, false},
                  {"R differ", [] { W.B.R = 2; }, false}}});
    t.push_back({"diff sizing call", [] { W.DF.rem_keys = nullptr; W.DF.ups_keys = nullptr; return check_diff(&W.A, &W.B, 0, 0, &W.DF); },
                 {}, {}, {}, {}, always, false, any_input, {}});
    // Extract, has, tomb has: required pointers only.
    t.push_back({"extract", [] { return check_extract(&W.S, W.peer, &W.DO); }, DO, {F(DO.kind, ENT, 1)}, S_req + std::vector<Field>{F(peer, VV, 8)},
                 S_opt, always, false, any_input,
                 {{"no tombstones in: none out", [] { W.S.tomb_off = nullptr; W.DO.tomb_off = nullptr; W.DO.tkeys = nullptr; W.DO.tactors = nullptr; W.DO.tcounters = nullptr; }, true},
                  {"R = 0", [] { W.S.R = 0; }, false}}});
    t.push_back({"extract empty without peer clock", [] { W.S.n_docs = 0; return check_extract(&W.S, nullptr, &W.DO); }, {}, {}, {},
                 {}, always, false, any_input, {}});
    const std::vector<Field> QOr{F(QO.found, ENT, 1), F(QO.actors, ENT, 4), F(QO.counters, ENT, 8)};  // dots: both or neither
    const std::vector<Field> Qr{F(Q.q_off, OFF, 4), F(Q.keys, ENT, 8)};
    const std::vector<Extra> q_extras{{"no dots", [] { W.QO.actors = nullptr; W.QO.counters = nullptr; }, true},
                                      {"q n_docs differ", [] { W.Q.n_docs = 5; }, false},
                                      {"no queries, no keys", [] { W.Q.n_queries = 0; W.Q.keys = nullptr; }, true}};
    t.push_back({"has", [] { return check_has(&W.A, &W.Q, &W.QO); }, QOr, {}, pick(A, {0}) + Qr, pick(A, {1, 2, 3, 4, 5}), always,
                 false, any_input, q_extras});
    t.push_back({"tomb_has", [] { return check_tomb_has(&W.TA, (uint32_t)g_n, &W.Q, &W.QO); }, QOr, {}, TA_req + Qr, TA_opt, always,
                 false, any_input, q_extras});
    t.push_back({"has NULL descriptors",
                 [] {
                     return check_has(nullptr, &W.Q, &W.QO) == CRDT_E_INVALID && check_has(&W.A, nullptr, &W.QO) == CRDT_E_INVALID &&
                                    check_has(&W.A, &W.Q, nullptr) == CRDT_E_INVALID &&
                                    check_tomb_has(nullptr, (uint32_t)g_n, &W.Q, &W.QO) == CRDT_E_INVALID
                                ? CRDT_OK
                                : CRDT_E_ACTOR_RANGE;
                 },
                 {}, {}, {}, {}, always, false, any_input, {}});
    return t;
}

}  // namespace

int main() {
    const std::vector<Family> t = table();
    for (const Family& f : t) drive(f);
    if (g_failed) {
        printf("FAILED: %d of %d cases\n", g_failed, g_cases);
        return 1;
    }
    printf("ok: %d cases in %zu families\n", g_cases, t.size());
    return 0;
}
