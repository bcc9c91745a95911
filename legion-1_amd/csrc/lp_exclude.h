// lp_exclude.h -- target-edge exclusion (INTEGRATION.md "Target-edge exclusion"): the pair table's key, capacity and slot function, stated
// once for the kernels (lp_exclude.hip), the pool (memory_pool.cpp) and the C ABI (legion_lp_pair_slot, which a CPU test pins).
#pragma once
#include "internal.h"

namespace legion {

// An empty slot of the table.  No key equals it: a key's high word is an id >= 0.
constexpr uint64_t kLpEmpty = ~0ull;
// The unordered pair {u, v} of two ids >= 0 as one word: the smaller id in the high half
__host__ __device__ inline uint64_t lp_pair_key(int32_t u, int32_t v)
{
    const uint32_t lo = (uint32_t)(u < v ? u : v), hi = (uint32_t)(u < v ? v : u);
    return ((uint64_t)lo << 32) | (uint64_t)hi;
}
// The first slot a pair (lo <= hi) is looked for in a table of `cap` slots (a power of two); probing is linear from there
__host__ __device__ inline uint32_t lp_pair_slot(uint32_t lo, uint32_t hi, uint32_t cap) { return mix32(lo ^ mix32(hi)) & (cap - 1u); }
// Slots of the table of k triples: the smallest power of two >= max(4 k, 64), so that k keys fill at most a quarter of it
constexpr int32_t kLpMaxTriples = 1 << 28;
inline int32_t lp_pair_cap(int32_t k)
{
    int64_t cap = 64;
    while (cap < 4ll * k) cap <<= 1;
    return (int32_t)cap;
}

} // namespace legion
