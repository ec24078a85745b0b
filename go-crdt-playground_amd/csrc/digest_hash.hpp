// The per-document state digest (include/crdtgpu.h, "state digests"): the hash
// terms, shared by the kernels (digest.hip) and the host statement of the
// definition (serial.cpp, crdt_awset_digest_host).  Part of the ABI: the
// constants and the mixing must not change once digests have been exchanged.
// All arithmetic is mod 2^64.
#pragma once

#include <stdint.h>

// serial.cpp is also built by a plain host compiler (the fuzz target): no HIP there.
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define CRDT_DIG_FN __host__ __device__ inline
#else
#define CRDT_DIG_FN inline
#endif

namespace crdt {

constexpr uint64_t kDigE = 0x9E3779B97F4A7C15ull;  // live entry keys
constexpr uint64_t kDigT = 0xC2B2AE3D27D4EB4Full;  // tombstone keys
constexpr uint64_t kDigA = 0xD6E8FEB86659FD93ull;  // dot actors
constexpr uint64_t kDigV = 0x165667B19E3779F9ull;  // clock words
constexpr uint64_t kDigN = 0x85EBCA77C2B2AE63ull;  // counts

// The splitmix64 finaliser.
CRDT_DIG_FN uint64_t dig_fmix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// hk: a live entry's key, the term of word 0.
CRDT_DIG_FN uint64_t dig_key(uint64_t k) { return dig_fmix(k + kDigE); }

// hd / ht: a key's hash (dig_key(k) of a live entry, dig_fmix(k + kDigT) of a
// tombstone) under the dot (a, c), the term of word 1.
CRDT_DIG_FN uint64_t dig_dot(uint64_t hkey, uint32_t a, uint64_t c) {
    return dig_fmix(hkey ^ (c + kDigA * ((uint64_t)a + 1)));
}

// hv: clock word r; a zero word contributes nothing, so the R padding does not show.
CRDT_DIG_FN uint64_t dig_clock(uint32_t r, uint64_t v) {
    return v == 0 ? 0 : dig_fmix(v + kDigV * ((uint64_t)r + 1));
}

// ---- the digest tree (include/crdtgpu.h, "digest trees") ------------------------
// A hash tree of fan-out 16 over a digest array; level 0 is the array itself.
// Word 0 and word 1 are hashed separately all the way up.

constexpr uint32_t kDigTreeFanout = 16;            // CRDT_DIGEST_TREE_FANOUT
constexpr uint32_t kDigTreeMaxLevels = 8;          // L <= 8 for n_docs < 2^32
constexpr uint64_t kDigP = 0x2545F4914F6CDD1Dull;  // child slots

// One word of child slot j (0 ... 15) of a node: the term of that node's word.
CRDT_DIG_FN uint64_t dig_tree_term(uint64_t w, uint32_t j) { return dig_fmix(w + kDigP * ((uint64_t)j + 1)); }

// One word of a node with c children whose terms sum to `sum`.
CRDT_DIG_FN uint64_t dig_tree_node(uint64_t sum, uint32_t c) { return dig_fmix(sum + kDigN * c); }

// nodes[l] / off[l] for l = 0 ... 8: the nodes of level l (nodes[0] = n_docs) and
// the node offset of level l >= 1 in the tree array; zero above L, which is returned.
inline int dig_tree_layout(uint32_t n_docs, uint32_t nodes[9], uint32_t off[9]) {
    for (int l = 0; l < 9; ++l) nodes[l] = off[l] = 0;
    nodes[0] = n_docs;
    if (n_docs == 0) return 0;
    int l = 0;
    uint32_t o = 0;
    do {
        ++l;
        nodes[l] = (uint32_t)(((uint64_t)nodes[l - 1] + kDigTreeFanout - 1) / kDigTreeFanout);
        off[l] = o;
        o += nodes[l];
    } while (nodes[l] != 1);
    return l;
}

}  // namespace crdt
