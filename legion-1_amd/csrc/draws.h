// draws.h -- device-side helpers the .hip units share: the draw rules of the sampler modes, which every probe (probes.hip) calls exactly
// as its production kernel does, and the small lane / division helpers.  Device code: included by .hip units only.  (mix32, mulmod31 and
// the seeded_* keys are in internal.h: the host forms them too.)
#pragma once
#include "internal.h"

namespace legion {

// thrust::uniform_int_distribution<int>(0, deg-1) fed with x = minstd value (Kernels.cu:402-405;
// thrust/random/detail/uniform_int_distribution.inl:73-89, uniform_real_distribution.inl:71-79)
__device__ inline int32_t sample_index(uint32_t x, int32_t deg)
{
    double result = (double)(uint32_t)(x - 1u);
    result /= 2147483646.0;                  // 1.0 + double(max - min), max-min = 2147483645
    return (int32_t)(result * (double)deg + 0.0);
}

__device__ inline uint32_t fdiv(uint32_t n, const FastDiv& d)
{
    return d.d == 1 ? n : (uint32_t)(((uint64_t)n * d.m) >> d.s);
}

// Distinct-draw sampler mode (INTEGRATION.md "Sampling without replacement"): a row of degree d > f takes f distinct neighbour positions
// by Floyd's algorithm over hashed randoms, a pure function of (hop, row of the hop's input list); d <= f takes every neighbour once.
// All arithmetic is uint32 with wrap-around except the one 64-bit product.
// (mix32 lives in internal.h: the seeded mode's keys are formed on the host too.)  w: the batch's draw word, 0 with the seeded mode off.
__device__ inline uint32_t distinct_key(uint32_t row, uint32_t hop, uint32_t w) { return mix32((row + 0x9E3779B9u * hop) ^ w); }
__device__ inline uint32_t distinct_u(uint32_t key, uint32_t t) { return mix32(key ^ (0x85EBCA6Bu * (t + 1u))); }
// In place: p[0, f) holds distinct_u(key, t) on entry and the row's f positions on return; d > f.  Sequential per row (pick t looks at the
// picks before it): at most f (f - 1) / 2 compares.  p is LDS in k_sample, global memory in the probe.
__device__ inline void distinct_resolve(int32_t* p, int32_t d, int32_t f)
{
    for (int32_t t = 0; t < f; t++) {
        const uint32_t J = (uint32_t)(d - f + t);
        const int32_t r = (int32_t)__umulhi((uint32_t)p[t], J + 1u);   // (u * (J + 1)) >> 32 < J + 1 <= d
        bool hit = false;
        for (int32_t q = 0; q < t; q++) hit |= (p[q] == r);
        p[t] = hit ? (int32_t)J : r;
    }
}

// Weighted sampler mode (INTEGRATION.md "Weighted sampling"): slot j of row i of hop h under draw word w draws column (uc * d) >> 32 of its
// row and keeps the column's own neighbour when ub < the column's threshold, else takes the column's alias; uc, ub = distinct_u(K, 2j),
// distinct_u(K, 2j + 1) under the mode's own row key K.
__device__ inline uint32_t weighted_key(uint32_t row, uint32_t hop, uint32_t w) { return mix32(distinct_key(row, hop, w) ^ 0xC2B2AE35u); }
__device__ inline uint32_t weighted_column(uint32_t key, uint32_t j, int32_t d) { return __umulhi(distinct_u(key, 2u * j), (uint32_t)d); }   // < d, d > 0
__device__ inline uint32_t weighted_ub(uint32_t key, uint32_t j) { return distinct_u(key, 2u * j + 1u); }

__device__ inline int lane_id() { return threadIdx.x & 63; }
__device__ inline int wave_id() { return threadIdx.x >> 6; }

// Drawn link-prediction thirds (INTEGRATION.md "Drawn link-prediction thirds"): the positive and the negative of slot i of a batch, pure
// functions of the batch's draw word, the slot and its source.  u is the distinct mode's hash of (key, slot) with the source folded in, so
// that two GPUs of one job, which share the draw word, do not draw the same negatives.
__device__ inline uint32_t lp_u(uint32_t key, uint32_t i, int32_t src) { return mix32(distinct_u(key, i) ^ (uint32_t)src); }
__device__ inline int32_t lp_rho(uint32_t w, uint32_t i, int32_t src, int32_t d) { return (int32_t)__umulhi(lp_u(mix32(w ^ kLpPosTag), i, src), (uint32_t)d); }   // < d, d > 0
__device__ inline int32_t lp_neg(uint32_t w, uint32_t i, int32_t src, int32_t V) { return (int32_t)__umulhi(lp_u(mix32(w ^ kLpNegTag), i, src), (uint32_t)V); }   // < V

// A store through an index computed on the device is dropped unless the index lies inside the buffer (k_write, sampler.hip, has the reason).
#define LEGION_STORE_OK(i, cap) ((uint32_t)(i) < (uint32_t)(cap))

} // namespace legion
