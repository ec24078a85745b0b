// Host test of the digest tree's argument checks (check_digest_tree,
// check_digest_tree_children, check_digest_tree_diff;
// go-crdt-playground_amd/csrc/api_args.hpp), built with ASan + UBSan by
// host/Makefile (build/test_api_args_digest_tree) and run by
// tests/test_digest_tree_args.py.  No device, no libcrdtgpu.so.
//
// The checks read arguments, never arrays, so every array address is taken from
// one static buffer and nothing is ever stored there.  Families:
//   build     both arrays, either NULL, the tree on the digest array; n_docs == 0
//             accepts anything
//   children  baseline with a list and in the identity form; out / level NULL;
//             level NULL at n_level == 0; out on level, parents, n_parents and one
//             element further; the identity form's n_max against ceil(n_level / 16)
//             at n_level = 0, 1, 16, 17, 4,097 and 2^32 - 1, and a list with any n_max
//   diff      baseline; every required pointer NULL, every optional one NULL;
//             mask 0 .. 8; each written array on each input and on each other
//             written array; n_out inside the summary's five words; the identity rule
//   layout    crdt_digest_tree_layout's arithmetic (digest_hash.hpp, host code) at the
//             edges of every level count
#include <cstdint>
#include <cstdio>

#include "../../go-crdt-playground_amd/csrc/api_args.hpp"
#include "../../go-crdt-playground_amd/csrc/digest_hash.hpp"

using namespace crdt;

namespace {

alignas(16) unsigned char g_buf[1 << 12];
int g_cases = 0, g_failed = 0;

void* at(int slot) { return g_buf + 64 * (slot + 1); }

void expect(int got, int want, const char* family, const char* what, long long x = 0) {
    ++g_cases;
    if (got != want) {
        ++g_failed;
        printf("FAIL %s: %s (%lld): got %d, want %d\n", family, what, x, got, want);
    }
}

const int OK = CRDT_OK, BAD = CRDT_E_INVALID;

void family_build() {
    const uint64_t* digest = (const uint64_t*)at(0);
    uint64_t* tree = (uint64_t*)at(1);
    for (uint32_t n : {1u, 16u, 17u, 0xFFFFFFFFu}) {
        expect(check_digest_tree(digest, n, tree), OK, "build", "baseline", n);
        expect(check_digest_tree(nullptr, n, tree), BAD, "build", "digest NULL", n);
        expect(check_digest_tree(digest, n, nullptr), BAD, "build", "tree NULL", n);
        expect(check_digest_tree(digest, n, digest), BAD, "build", "tree on digest", n);
        expect(check_digest_tree(digest, n, digest + 1), OK, "build", "tree one word past digest", n);
    }
    expect(check_digest_tree(nullptr, 0, nullptr), OK, "build", "no documents, no arrays");
    expect(check_digest_tree(digest, 0, digest), OK, "build", "no documents, one array");
}

struct Identity {
    uint32_t n_level, n_nodes;
};
const Identity kIdentity[] = {{0, 0}, {1, 1}, {16, 1}, {17, 2}, {4097, 257}, {0xFFFFFFFFu, 1u << 28}};

void family_children() {
    const uint64_t* level = (const uint64_t*)at(0);
    const uint32_t* parents = (const uint32_t*)at(1);
    const uint32_t* n_parents = (const uint32_t*)at(2);
    uint64_t* out = (uint64_t*)at(3);
    const char* f = "children";
    expect(check_digest_tree_children(level, 40, parents, n_parents, 3, out), OK, f, "baseline");
    expect(check_digest_tree_children(level, 40, parents, nullptr, 3, out), OK, f, "n_parents NULL");
    expect(check_digest_tree_children(level, 40, nullptr, nullptr, 3, out), OK, f, "identity");
    expect(check_digest_tree_children(level, 40, nullptr, n_parents, 3, out), OK, f, "identity with a count");
    expect(check_digest_tree_children(level, 40, parents, n_parents, 3, nullptr), BAD, f, "out NULL");
    expect(check_digest_tree_children(nullptr, 40, parents, n_parents, 3, out), BAD, f, "level NULL");
    expect(check_digest_tree_children(nullptr, 0, parents, n_parents, 3, out), OK, f, "level NULL, empty level");
    expect(check_digest_tree_children(level, 40, parents, n_parents, 0, out), OK, f, "n_max 0");
    expect(check_digest_tree_children(level, 40, parents, n_parents, 0, nullptr), BAD, f, "n_max 0, out NULL");
    const void* ins[] = {level, parents, n_parents};
    for (const void* in : ins) {
        expect(check_digest_tree_children(level, 40, parents, n_parents, 3, (const uint64_t*)in), BAD, f,
               "out on an input");
        expect(check_digest_tree_children(level, 40, parents, n_parents, 3, (const uint64_t*)in + 1), OK, f,
               "out one word past an input");
    }
    for (const Identity& c : kIdentity) {
        expect(check_digest_tree_children(level, c.n_level, nullptr, nullptr, c.n_nodes, out), OK, f,
               "identity, every node", c.n_level);
        if (c.n_nodes)
            expect(check_digest_tree_children(level, c.n_level, nullptr, nullptr, c.n_nodes - 1, out), OK, f,
                   "identity, a prefix", c.n_level);
        expect(check_digest_tree_children(level, c.n_level, nullptr, nullptr, c.n_nodes + 1, out), BAD, f,
               "identity, one node too many", c.n_level);
        expect(check_digest_tree_children(level, c.n_level, parents, nullptr, c.n_nodes + 1, out), OK, f,
               "a list of any capacity", c.n_level);
    }
}

struct Diff {
    const uint64_t *mine, *theirs;
    const uint32_t *parents, *n_parents;
    uint32_t n_level, n_max, mask;
    uint32_t* idx_out;
    uint8_t* flags_out;
    uint32_t *n_out, *summary;
};

Diff fresh() {
    return Diff{(const uint64_t*)at(0), (const uint64_t*)at(1), (const uint32_t*)at(2), (const uint32_t*)at(3),
                40,                     3,                      3,                      (uint32_t*)at(4),
                (uint8_t*)at(5),        (uint32_t*)at(6),       (uint32_t*)at(7)};
}

int run(const Diff& d) {
    return check_digest_tree_diff(d.mine, d.n_level, d.theirs, d.parents, d.n_parents, d.n_max, d.mask, d.idx_out,
                                  d.flags_out, d.n_out, d.summary);
}

void family_diff() {
    const char* f = "diff";
    expect(run(fresh()), OK, f, "baseline");
    Diff d = fresh();
    d.mine = nullptr;
    expect(run(d), BAD, f, "mine_level NULL");
    d.n_level = 0;
    expect(run(d), OK, f, "mine_level NULL, empty level");
    d = fresh();
    d.theirs = nullptr;
    expect(run(d), BAD, f, "theirs NULL");
    d.n_max = 0;
    expect(run(d), OK, f, "theirs NULL, n_max 0");
    d = fresh();
    d.idx_out = nullptr;
    expect(run(d), BAD, f, "idx_out NULL");
    d = fresh();
    d.n_out = nullptr;
    expect(run(d), BAD, f, "n_out NULL");
    d = fresh();
    d.flags_out = nullptr;
    expect(run(d), OK, f, "flags_out NULL");
    d = fresh();
    d.summary = nullptr;
    expect(run(d), OK, f, "summary NULL");
    d = fresh();
    d.n_parents = nullptr;
    expect(run(d), OK, f, "n_parents NULL");
    d = fresh();
    d.parents = nullptr;
    expect(run(d), OK, f, "identity");
    for (uint32_t mask = 0; mask <= 8; ++mask) {
        d = fresh();
        d.mask = mask;
        expect(run(d), mask >= 1 && mask <= 3 ? OK : BAD, f, "mask", mask);
    }
    d = fresh();
    d.mask = 0xFFFFFFFFu;
    expect(run(d), BAD, f, "mask all ones");
    // each written array on each input, whatever the width, and one byte further
    for (int w = 0; w < 4; ++w)
        for (int in = 0; in < 4; ++in)
            for (int step = 0; step < 2; ++step) {
                d = fresh();
                unsigned char* p = (unsigned char*)at(in) + (step ? 8 : 0);
                if (w == 0) d.idx_out = (uint32_t*)p;
                if (w == 1) d.flags_out = (uint8_t*)p;
                if (w == 2) d.n_out = (uint32_t*)p;
                if (w == 3) d.summary = (uint32_t*)p;
                expect(run(d), step ? OK : BAD, f, "a written array on an input", 10 * w + in);
            }
    // two written arrays at one address
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b) {
            d = fresh();
            void* p = at(4 + a);
            if (b == 1) d.flags_out = (uint8_t*)p;
            if (b == 2) d.n_out = (uint32_t*)p;
            if (b == 3) d.summary = (uint32_t*)p;
            expect(run(d), BAD, f, "two written arrays at one address", 10 * a + b);
        }
    // n_out inside the summary's five words, and just past them
    for (int k = 0; k <= 5; ++k) {
        d = fresh();
        d.n_out = d.summary + k;
        expect(run(d), k < 5 ? BAD : OK, f, "n_out at a summary word", k);
    }
    d = fresh();
    d.summary = d.n_out - 4;
    expect(run(d), BAD, f, "the summary's last word on n_out");
    d.summary = d.n_out - 5;
    expect(run(d), OK, f, "the summary ends where n_out starts");
    for (const Identity& c : kIdentity) {
        d = fresh();
        d.parents = nullptr;
        d.n_level = c.n_level;
        d.n_max = c.n_nodes;
        expect(run(d), OK, f, "identity, every node", c.n_level);
        d.n_max = c.n_nodes + 1;
        expect(run(d), BAD, f, "identity, one node too many", c.n_level);
        d.parents = fresh().parents;
        expect(run(d), OK, f, "a list of any capacity", c.n_level);
    }
}

void family_layout() {
    const char* f = "layout";
    struct {
        uint32_t n;
        int L;
        uint32_t n1, total;
    } rows[] = {{0, 0, 0, 0},         {1, 1, 1, 1},          {2, 1, 1, 1},           {16, 1, 1, 1},
                {17, 2, 2, 3},        {256, 2, 16, 17},      {257, 3, 17, 20},       {4096, 3, 256, 273},
                {4097, 4, 257, 277},  {65537, 5, 4097, 4374}, {1048577, 6, 65537, 69911},
                {0xFFFFFFFFu, 8, 1u << 28, 286331153u}};
    for (auto& r : rows) {
        uint32_t nodes[9], off[9];
        const int L = dig_tree_layout(r.n, nodes, off);
        expect(L, r.L, f, "L", r.n);
        expect((int)(nodes[0] == r.n && nodes[1] == r.n1), 1, f, "level counts", r.n);
        expect((int)(L == 0 ? 0u : off[L] + 1u) == (int)r.total, 1, f, "total nodes", r.n);
        bool ok = L == 0 || nodes[L] == 1;
        for (int l = 1; l <= L; ++l)
            ok = ok && nodes[l] == (uint32_t)(((uint64_t)nodes[l - 1] + 15) / 16) &&
                 off[l] == (l == 1 ? 0u : off[l - 1] + nodes[l - 1]) && (l == L || nodes[l] > 1);
        for (int l = L + 1; l < 9; ++l) ok = ok && nodes[l] == 0 && off[l] == 0;
        expect((int)ok, 1, f, "every level", r.n);
    }
}

}  // namespace

int main() {
    family_build();
    family_children();
    family_diff();
    family_layout();
    if (g_failed) {
        printf("%d of %d cases failed\n", g_failed, g_cases);
        return 1;
    }
    printf("ok: %d cases in 4 families\n", g_cases);
    return 0;
}
