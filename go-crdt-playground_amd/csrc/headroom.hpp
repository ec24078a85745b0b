// The headroom policy's capacity (crdt_headroom, crdt_headroom_capacity;
// include/crdtgpu.h): the ONE definition, read by the host function (api.cpp) and
// by the repack kernels (replica_repack.hip).
#pragma once
#include <stdint.h>

#include "../../include/crdtgpu.h"

namespace crdt {

constexpr crdt_headroom kHeadroomPacked = {0u, 0u, 0u, 1u};  // a NULL policy

// cap(n) = round_up(n + max(min_spare, (n * num) >> shift), align), unsaturated:
// n * num <= (2^32 - 1)^2, so the sum with n and align - 1 stays below 2^64.
// align is a power of two (1..64) and shift <= 31: checked where a policy enters.
__host__ __device__ inline uint64_t headroom_cap64(const crdt_headroom& h, uint32_t n) {
    const uint64_t prop = ((uint64_t)n * h.num) >> h.shift;
    const uint64_t spare = prop > h.min_spare ? prop : (uint64_t)h.min_spare;
    const uint64_t a = h.align;
    return ((uint64_t)n + spare + (a - 1)) & ~(a - 1);
}

// Saturated at 2^32 - 1; *sat is set (never cleared) when it did.
__host__ __device__ inline uint32_t headroom_cap(const crdt_headroom& h, uint32_t n, bool* sat) {
    const uint64_t c = headroom_cap64(h, n);
    if (c > 0xFFFFFFFFull) {
        *sat = true;
        return 0xFFFFFFFFu;
    }
    return (uint32_t)c;
}

inline bool headroom_ok(const crdt_headroom& h) {
    return h.align >= 1u && h.align <= 64u && (h.align & (h.align - 1u)) == 0u && h.shift <= 31u;
}

}  // namespace crdt
