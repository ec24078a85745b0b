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

}  // namespace crdt
