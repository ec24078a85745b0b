// Host test of the worklist digest's argument check (check_digest_idx,
// go-crdt-playground_amd/csrc/api_args.hpp), built with ASan + UBSan by
// host/Makefile (build/test_api_args_digest_idx) and run by
// tests/test_digest_idx_args.py.  No device, no libcrdtgpu.so.
//
// The check reads descriptors, never arrays, so every array address is taken from
// one static buffer and nothing is ever stored there.  Cases, in both modes and
// with and without tombstones:
//   baseline   all arrays distinct: accepted; n_idx NULL and counts NULL: accepted
//   NULLs      state, idx, digest, state->offsets, state->vv (n_docs > 0), tombs
//              without offsets: refused
//   R          0 and CRDT_MAX_R + 1 refused, 1 and CRDT_MAX_R accepted
//   mode       2 and 0xFFFFFFFF refused
//   counts     GATHER: n_digest_docs != state->n_docs refused either way;
//              PLACE: state->n_docs < n_max refused, == and > accepted, and any
//              n_digest_docs accepted
//   aliasing   digest on every input array, on idx and on n_idx; idx on every
//              input array: refused, whatever the width; one element further: accepted
//   n_max = 0  the rules hold all the same (the call launches nothing afterwards)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../go-crdt-playground_amd/csrc/api_args.hpp"

using namespace crdt;

namespace {

alignas(16) unsigned char g_buf[1 << 12];
int g_cases = 0, g_failed = 0;

struct World {
    crdt_awset_batch st;
    crdt_tomb_batch tb;
    const uint32_t *idx, *n_idx;
    uint32_t n_max, n_digest, mode;
    uint64_t* digest;
    bool with_tombs;
};

// Every array 64 bytes from the next.
World fresh(uint32_t mode, bool with_tombs) {
    World w{};
    unsigned char* p = g_buf;
    auto next = [&]() {
        p += 64;
        return (void*)p;
    };
    w.st.n_docs = 3;
    w.st.R = 2;
    w.st.offsets = (const uint32_t*)next();
    w.st.counts = (const uint32_t*)next();
    w.st.keys = (const uint64_t*)next();
    w.st.actors = (const uint32_t*)next();
    w.st.counters = (const uint64_t*)next();
    w.st.vv = (const uint64_t*)next();
    w.tb.offsets = (const uint32_t*)next();
    w.tb.counts = (const uint32_t*)next();
    w.tb.keys = (const uint64_t*)next();
    w.tb.actors = (const uint32_t*)next();
    w.tb.counters = (const uint64_t*)next();
    w.idx = (const uint32_t*)next();
    w.n_idx = (const uint32_t*)next();
    w.digest = (uint64_t*)next();
    w.mode = mode;
    w.with_tombs = with_tombs;
    w.n_max = 2;
    w.n_digest = mode == CRDT_DIGEST_GATHER ? 3 : 10;
    return w;
}

int run(const World& w) {
    return check_digest_idx(&w.st, w.with_tombs ? &w.tb : nullptr, w.idx, w.n_idx, w.n_max, w.n_digest, w.mode,
                            w.digest);
}

void expect(const World& w, int want, const char* what) {
    ++g_cases;
    const int got = run(w);
    if (got != want) {
        ++g_failed;
        printf("FAIL mode %u tombs %d: %s: got %d, want %d\n", w.mode, (int)w.with_tombs, what, got, want);
    }
}

struct Input {
    const char* name;
    const void* p;
};

std::vector<Input> inputs(const World& w) {
    std::vector<Input> v = {{"offsets", w.st.offsets}, {"counts", w.st.counts},     {"keys", w.st.keys},
                            {"actors", w.st.actors},   {"counters", w.st.counters}, {"vv", w.st.vv}};
    if (w.with_tombs) {
        v.push_back({"t.offsets", w.tb.offsets});
        v.push_back({"t.counts", w.tb.counts});
        v.push_back({"t.keys", w.tb.keys});
        v.push_back({"t.actors", w.tb.actors});
        v.push_back({"t.counters", w.tb.counters});
    }
    return v;
}

void family(uint32_t mode, bool with_tombs) {
    const World base = fresh(mode, with_tombs);
    const int ok = CRDT_OK, bad = CRDT_E_INVALID;
    for (uint32_t n_max : {2u, 0u}) {
        World b = base;
        b.n_max = n_max;
        expect(b, ok, "baseline");
        World w = b;
        w.n_idx = nullptr;
        expect(w, ok, "n_idx NULL");
        w = b;
        w.st.counts = nullptr;
        w.tb.counts = nullptr;
        expect(w, ok, "counts NULL");
        w = b;
        w.st.keys = nullptr;  // (the entry arrays are not required pointers: an empty batch has none)
        expect(w, ok, "keys NULL");

        // required pointers
        ++g_cases;
        if (check_digest_idx(nullptr, nullptr, b.idx, b.n_idx, b.n_max, b.n_digest, b.mode, b.digest) != bad) {
            ++g_failed;
            printf("FAIL: NULL state accepted\n");
        }
        w = b;
        w.idx = nullptr;
        expect(w, bad, "idx NULL");
        w = b;
        w.digest = nullptr;
        expect(w, bad, "digest NULL");
        w = b;
        w.st.offsets = nullptr;
        expect(w, bad, "offsets NULL");
        w = b;
        w.st.vv = nullptr;
        expect(w, bad, "vv NULL");
        if (with_tombs) {
            w = b;
            w.tb.offsets = nullptr;
            expect(w, bad, "tombs without offsets");
            w = b;
            w.tb.keys = nullptr;  // (the columns are not required: only the offsets)
            expect(w, ok, "tombs without keys");
        }

        // R
        for (uint32_t R : {0u, (uint32_t)CRDT_MAX_R + 1u, 0xFFFFFFFFu}) {
            w = b;
            w.st.R = R;
            expect(w, bad, "R out of range");
        }
        for (uint32_t R : {1u, (uint32_t)CRDT_MAX_R}) {
            w = b;
            w.st.R = R;
            expect(w, ok, "R in range");
        }

        // mode
        for (uint32_t m : {2u, 3u, 0xFFFFFFFFu}) {
            w = b;
            w.mode = m;
            expect(w, bad, "mode above 1");
        }

        // the document counts
        if (mode == CRDT_DIGEST_GATHER) {
            for (uint32_t nd : {0u, 2u, 4u, 0xFFFFFFFFu}) {
                w = b;
                w.n_digest = nd;
                expect(w, bad, "GATHER: n_digest_docs != n_docs");
            }
            w = b;
            w.n_max = 1000;  // a list longer than the replica may repeat: no rule
            expect(w, ok, "GATHER: n_max above n_docs");
        } else {
            for (uint32_t nd : {0u, 2u, 3u, 4u, 0xFFFFFFFFu}) {
                w = b;
                w.n_digest = nd;
                expect(w, ok, "PLACE: any n_digest_docs");
            }
            w = b;
            w.n_max = 3;
            expect(w, ok, "PLACE: n_docs == n_max");
            w.n_max = 4;
            expect(w, bad, "PLACE: n_docs < n_max");
            w.n_max = 0xFFFFFFFFu;
            expect(w, bad, "PLACE: n_docs < n_max (max)");
        }

        // aliasing: starts only, whatever the width
        for (const Input& in : inputs(b)) {
            w = b;
            w.digest = (uint64_t*)in.p;
            expect(w, bad, in.name);
            w.digest = (uint64_t*)((const unsigned char*)in.p + 8);
            expect(w, ok, in.name);
            w = b;
            w.idx = (const uint32_t*)in.p;
            expect(w, bad, in.name);
            w.idx = (const uint32_t*)((const unsigned char*)in.p + 4);
            expect(w, ok, in.name);
        }
        w = b;
        w.digest = (uint64_t*)b.idx;
        expect(w, bad, "digest on idx");
        w = b;
        w.digest = (uint64_t*)b.n_idx;
        expect(w, bad, "digest on n_idx");
        w = b;
        w.n_idx = b.idx;  // (a length word at the list's start is the caller's business)
        expect(w, ok, "n_idx on idx");
        if (!with_tombs) {  // arrays of a tomb batch that is not passed are not inputs
            w = b;
            w.digest = (uint64_t*)b.tb.keys;
            expect(w, ok, "digest on an unused tomb array");
        }
    }
}

}  // namespace

int main() {
    int families = 0;
    for (uint32_t mode : {CRDT_DIGEST_GATHER, CRDT_DIGEST_PLACE})
        for (bool with_tombs : {false, true}) {
            family(mode, with_tombs);
            ++families;
        }
    if (g_failed) {
        printf("%d of %d cases failed\n", g_failed, g_cases);
        return 1;
    }
    printf("ok: %d cases in %d families\n", g_cases, families);
    return 0;
}
