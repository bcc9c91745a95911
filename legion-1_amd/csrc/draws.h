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

// Weighted sampling without replacement (INTEGRATION.md "Weighted sampling without replacement"): column c of row i of hop h under draw
// word w gets the exponential key -log(x_c) / w_c, x_c = (u_c + 0.5) 2^-32, u_c = distinct_u(K, c) under the mode's own row key K; the row's
// picks are the f eligible (w > 0) columns of smallest (key, column), handed out in ascending column order (Efraimidis-Spirakis).  fp64
// throughout, and no contraction: the log, the negation and the divide round one by one, as the NumPy statement's do.
__device__ inline uint32_t weighted_distinct_key(uint32_t row, uint32_t hop, uint32_t w) { return mix32(distinct_key(row, hop, w) ^ 0x27D4EB2Fu); }
__device__ inline uint32_t weighted_distinct_u(uint32_t key, uint32_t c) { return distinct_u(key, c); }
__device__ inline double weighted_distinct_x(uint32_t u) { return ((double)u + 0.5) * 0x1p-32; }   // exact, in (0, 1)
__device__ inline double weighted_distinct_keyval(uint32_t u, float w)   // w > 0, finite: the key is finite and > 0
{
#pragma clang fp contract(off)
    const double l = log(weighted_distinct_x(u));
    return -l / (double)w;
}
// A column that cannot enter a best list whose last key is tk, told without the log: -log(x) >= 1 - x, so key_c >= (1 - x) / w up to the
// few ulp of the log and the divide; 1 - x is exact in fp64 and the 2^-40 margin is a thousand times those ulp.  Where it matters -- a
// full list on a long row, tk w << 1 -- the bound is tight: the columns it lets through are about the ones that do enter.  tk = +inf
// (the list is not full yet) excludes nothing.
__device__ inline bool weighted_distinct_excluded(uint32_t u, float w, double tk)
{
#pragma clang fp contract(off)
    return 1.0 - weighted_distinct_x(u) > (tk * (double)w) * (1.0 + 0x1p-40);
}
// The node keys of the two shared-key rules ("Shared-key sampling" below states the first): the batch's salt and the hash of a neighbour id under it.
__device__ inline uint32_t shared_salt(uint32_t w) { return mix32(w ^ 0x165667B1u); }
__device__ inline uint32_t shared_key(int32_t nbr, uint32_t salt) { return mix32((uint32_t)nbr ^ salt); }
// Weighted shared-key sampling (INTEGRATION.md "Weighted shared-key sampling", GPUMemoryPool_SetSharedDraws on top of the weighted kind with
// GPUMemoryPool_SetWeightedDistinct): weighted sampling without replacement whose uniform belongs to the NEIGHBOUR NODE, not to the column.
// Ksw = mix32(shared_salt(w) ^ 0x27D4EB2F) is the batch's salt (no hop, no row), u_c = mix32(nbr[c] ^ Ksw), and the key is
// weighted_distinct_keyval(u_c, w_c) as it is: rows that see the same neighbours at the same weights prefer the same ones, and each row still
// takes its columns in proportion to their weights.  A negative entry is keyed by its bit pattern like any id.
__device__ inline uint32_t weighted_shared_salt(uint32_t w) { return mix32(shared_salt(w) ^ 0x27D4EB2Fu); }
__device__ inline uint32_t weighted_shared_u(int32_t nbr, uint32_t salt) { return shared_key(nbr, salt); }
// One WAVE resolves one row (every lane of the wave calls this with the same arguments): p[0, min(m, f)) := the row's picks in ascending
// column order, m = the row's eligible columns; returns min(m, f).  wp: the row's d > 0 weights; p is LDS in k_sample.  The lanes stride
// over the row in chunks of 64 (coalesced weight reads, no single-lane loop).  Pass 1 counts the eligible columns and compacts the first f
// of them by ballot prefix -- with m <= f that is the result, and no key is formed.  Pass 2 (m > f) keeps the best list sorted in registers,
// entry l in lane l: a column whose (key, column) lies in front of entry f - 1 is inserted where the ballot of the entries in front of
// it ends and the tail moves up one lane; at the end the first f entries are ranked by column.  A chunk forms the key (the fp64 log) only
// of the columns weighted_distinct_excluded lets through against the list's last key at the chunk's start (the key only falls from there).
// NODE (weighted shared-key sampling, below): the uniform of column c is the hash of the column's NEIGHBOUR ID, rowp[c], under the batch's
// salt `key` instead of the hash of c under the row's key: pass 2 loads rowp[c] beside wp[c] (two independent coalesced loads).  Nothing
// else differs, since everything else reads (u, w) alone; equal ids of equal weight have bit-equal keys, and the column settles them as
// the (key, column) compares already do.  NODE = false does not read rowp.
template <bool NODE>
__device__ inline int32_t weighted_distinct_resolve(int32_t* p, const float* __restrict__ wp, const int32_t* __restrict__ rowp, int32_t d, int32_t f, uint32_t key)
{
    const int lane = lane_id();
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint32_t ud = (uint32_t)d;
    uint32_t m = 0;
    for (uint32_t c0 = 0; c0 < ud; c0 += 64u) {   // uint32: d < 2^31, so c0 + 64 does not wrap
        const uint32_t c = c0 + (uint32_t)lane;
        const bool elig = c < ud && wp[c] > 0.0f;
        const unsigned long long b = __ballot(elig);
        const uint32_t at = m + (uint32_t)__popcll(b & lt);
        if (elig && at < (uint32_t)f) p[at] = (int32_t)c;
        m += (uint32_t)__popcll(b);
    }
    if (m <= (uint32_t)f) return (int32_t)m;
    const double inf = __builtin_huge_val();
    double bk = inf;              // entry `lane` of the best list: (key, column), sorted ascending; +inf = empty
    int32_t bc = 0x7FFFFFFF;
    for (uint32_t c0 = 0; c0 < ud; c0 += 64u) {
        const uint32_t c = c0 + (uint32_t)lane;
        const float w = c < ud ? wp[c] : 0.0f;
        uint32_t u;
        if constexpr (NODE) u = weighted_shared_u(c < ud ? rowp[c] : 0, key);
        else u = weighted_distinct_u(key, c);
        const double tk0 = __shfl(bk, f - 1);   // by the whole wave, in front of the lanes' own tests
        bool todo = w > 0.0f && !weighted_distinct_excluded(u, w, tk0);
        const double k = todo ? weighted_distinct_keyval(u, w) : inf;
        for (;;) {   // at most 64 rounds: every round retires one lane of the chunk
            const double tk = __shfl(bk, f - 1);
            const int32_t tc = __shfl(bc, f - 1);
            const unsigned long long beat = __ballot(todo && (k < tk || (k == tk && (int32_t)c < tc)));
            if (!beat) break;
            const int src = __ffsll((long long)beat) - 1;
            const double nk = __shfl(k, src);
            const int32_t nc = __shfl((int32_t)c, src);
            const int at = __popcll(__ballot(bk < nk || (bk == nk && bc < nc)));   // the entries in front are a prefix of the lanes: at < f
            const double uk = __shfl_up(bk, 1);
            const int32_t uc = __shfl_up(bc, 1);
            if (lane == at) { bk = nk; bc = nc; }
            else if (lane > at) { bk = uk; bc = uc; }
            if (lane == src) todo = false;
        }
    }
    int32_t rank = 0;
    for (int32_t t = 0; t < f; t++) rank += __shfl(bc, t) < bc;
    if (lane < f) p[rank] = bc;
    return f;
}

// Shared-key sampling (INTEGRATION.md "Shared-key sampling", GPUMemoryPool_SetSharedDraws on top of the distinct kind): the random number
// belongs to the NEIGHBOUR NODE, not to the row.  Ks = mix32(w ^ 0x165667B1) is the batch's node-key salt (no hop, no row), key_c =
// mix32(nbr[c] ^ Ks); a row of degree d > f takes its f columns of smallest (key, column), handed out in ascending column order; d <= f takes
// every column and forms no key.  mix32 is a bijection, so only equal ids tie, and the column settles those: (key << 32 | column) is one
// uint64 compare.  A negative entry is keyed by its bit pattern like any id.
__device__ inline unsigned long long wave_read64(unsigned long long v, int l)   // lane l's v, l wave-uniform: two v_readlane, no LDS crossbar
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
// One WAVE resolves one row of d > f (every lane of the wave calls this with the same arguments): p[0, f) := the row's picks in ascending
// column order.  rowp: the row's d ids; p is LDS in k_sample.  The lanes stride over the row in chunks of 64 (coalesced 256-byte reads, no
// single-lane loop).
//  d <= 64, one chunk, a key per lane: the f-th smallest key T is found by bisection over its 32 bits -- one compare and one ballot per
//    bit, the rest scalar --, the picks are the lanes of key < T and, of the lanes of key == T (multi-edges), the lowest columns that fill
//    the f; they are compacted by ballot prefix, which is column order.
//  d > 64: the best list sits sorted in registers, entry l in lane l, as (key << 32 | column).  The first chunk is ranked by counting (64
//    uniform lane reads) and each entry moved to the lane of its rank.  The later chunks are fetched four at a time (four independent loads
//    in flight: a hub's chunks are a chain of round trips otherwise); of a chunk only the entries in front of the list's entry f - 1 at the
//    chunk's start are candidates (the list's last entry only falls from there); each is inserted where the ballot of the entries in
//    front of it ends and the tail moves up one lane.  At the end the first f entries are ranked by column.  A lane past the row's end
//    holds 0xFFFFFFFF'80000000 | lane: behind every column (columns are < 2^31) and distinct, so the first chunk's ranks are a permutation.
__device__ inline void shared_resolve(int32_t* p, const int32_t* __restrict__ rowp, int32_t d, int32_t f, uint32_t salt)
{
    const int lane = lane_id();
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint32_t ud = (uint32_t)d;
    if (d <= 64) {
        const bool valid = lane < d;
        const uint32_t key = valid ? shared_key(rowp[lane], salt) : 0u;
        uint32_t T = 0;   // the smallest T with f or more keys <= T: bit by bit from the top, a bit stays 0 if the keys below it suffice
        for (int bit = 31; bit >= 0; bit--) {
            const uint32_t trial = T | ((1u << bit) - 1u);
            if (__popcll(__ballot(valid && key <= trial)) < f) T |= 1u << bit;
        }
        const bool less = valid && key < T, eq = valid && key == T;
        const int need = f - __popcll(__ballot(less));   // >= 1 of the lanes at T
        const bool in = less || (eq && __popcll(__ballot(eq) & lt) < need);
        const unsigned long long m = __ballot(in);
        if (in) p[__popcll(m & lt)] = lane;
        return;
    }
    auto entry = [&](int32_t id, uint32_t c) {
        return c < ud ? ((unsigned long long)shared_key(id, salt) << 32) | c : 0xFFFFFFFF80000000ull | (unsigned long long)lane;
    };
    unsigned long long b = entry(rowp[lane], (uint32_t)lane);   // d > 64: the first chunk is whole
    int32_t rank = 0;
    for (int t = 0; t < 64; t++) rank += wave_read64(b, t) < b;
    {   // entry of rank l to lane l: a push through the LDS crossbar, the ranks are a permutation of 0..63
        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_permute(rank << 2, (int)(uint32_t)b), hi = (uint32_t)__builtin_amdgcn_ds_permute(rank << 2, (int)(uint32_t)(b >> 32));
        b = ((unsigned long long)hi << 32) | lo;
    }
    for (uint32_t c0 = 64u; c0 < ud; c0 += 256u) {   // uint32: d < 2^31, so c0 + 319 does not wrap
        int32_t id[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const uint32_t c = c0 + 64u * u + (uint32_t)lane;
            id[u] = c < ud ? rowp[c] : 0;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const unsigned long long k = entry(id[u], c0 + 64u * u + (uint32_t)lane);
            bool todo = k < wave_read64(b, f - 1);   // by the whole wave, in front of any insertion
            for (;;) {   // at most 64 rounds: every round retires one lane of the chunk
                const unsigned long long beat = __ballot(todo && k < wave_read64(b, f - 1));
                if (!beat) break;
                const int src = __ffsll((long long)beat) - 1;
                const unsigned long long nk = wave_read64(k, src);
                const int at = __popcll(__ballot(b < nk));   // the entries in front are a prefix of the lanes: at < f
                const unsigned long long up = __shfl_up(b, 1);
                if (lane == at) b = nk;
                else if (lane > at) b = up;
                if (lane == src) todo = false;
            }
        }
    }
    const int32_t bc = lane < f ? (int32_t)(uint32_t)b : 0x7FFFFFFF;
    rank = 0;
    for (int32_t t = 0; t < f; t++) rank += __builtin_amdgcn_readlane(bc, t) < bc;
    if (lane < f) p[rank] = bc;
}

// Drawn link-prediction thirds (INTEGRATION.md "Drawn link-prediction thirds"): the positive and the negative of slot i of a batch, pure
// functions of the batch's draw word, the slot and its source.  u is the distinct mode's hash of (key, slot) with the source folded in, so
// that two GPUs of one job, which share the draw word, do not draw the same negatives.
__device__ inline uint32_t lp_u(uint32_t key, uint32_t i, int32_t src) { return mix32(distinct_u(key, i) ^ (uint32_t)src); }
__device__ inline int32_t lp_rho(uint32_t w, uint32_t i, int32_t src, int32_t d) { return (int32_t)__umulhi(lp_u(mix32(w ^ kLpPosTag), i, src), (uint32_t)d); }   // < d, d > 0
__device__ inline int32_t lp_neg(uint32_t w, uint32_t i, int32_t src, int32_t V) { return (int32_t)__umulhi(lp_u(mix32(w ^ kLpNegTag), i, src), (uint32_t)V); }   // < V

// A store through an index computed on the device is dropped unless the index lies inside the buffer (k_write, sampler.hip, has the reason).
#define LEGION_STORE_OK(i, cap) ((uint32_t)(i) < (uint32_t)(cap))

} // namespace legion
