// lp_exclude.hip -- target-edge exclusion for link prediction (no counterpart in the reference; INTEGRATION.md "Target-edge exclusion"):
// k_lp_pairs builds the hash table of a batch's target pairs behind k_seed, k_lp_edge_keep marks every COO edge of the batch behind the
// last hop.  Both read the batch's own pipe only -- never cand, the slot states, the tile prefixes, hop_state or pos_map.
#include "internal.h"
#include "draws.h"
#include "launch.h"
#include "lp_exclude.h"

#include "audit_hooks.h"

namespace legion {

// ------------------------------------------------------------------------------------------------
// The pair table: uint64[cap], open addressing, linear probing, at most a quarter full
// ------------------------------------------------------------------------------------------------
// One workgroup: empty the table and zero the counts, a barrier, then one key per valid triple i < k -- {ids[i], ids[k + i]} with both
// ids >= 0 -- by 64-bit compare-and-swap; a key that is there already is left alone.  The table is emptied for every batch, whatever it
// held (the scratch rule: nothing is epoch-tagged).  A batch whose level-0 size on the device is not 3 k leaves the table empty.
__global__ __launch_bounds__(kBlock) void k_lp_pairs(LpPairsArgs a)
{
    const uint32_t cap = (uint32_t)a.cap;
    for (uint32_t q = threadIdx.x; q < cap; q += kBlock) a.pairs[q] = kLpEmpty;
    if (threadIdx.x < kLpExcludedWords) a.excluded[threadIdx.x] = 0;
    __threadfence_block();
    __syncthreads();
    if (legion_level_size(a.nc, 0) != 3 * a.k) return;
    unsigned long long* tab = (unsigned long long*)a.pairs;
    for (int32_t i = threadIdx.x; i < a.k; i += kBlock) {
        const int32_t u = a.ids[i], v = a.ids[a.k + i];
        if (u < 0 || v < 0) continue;
        const uint64_t key = lp_pair_key(u, v);
        uint32_t slot = lp_pair_slot((uint32_t)(key >> 32), (uint32_t)key, cap);
        for (uint32_t step = 0; step < cap; step++) {   // k <= cap / 4 keys: an empty slot is always found; the bound is a belt
            const unsigned long long was = atomicCAS(tab + slot, (unsigned long long)kLpEmpty, (unsigned long long)key);
            if (was == kLpEmpty || was == key) break;
            slot = (slot + 1u) & (cap - 1u);
        }
    }
}

void launch_lp_pairs(hipStream_t s, const LpPairsArgs& a)
{
    if (a.k <= 0 || a.cap < 4 * (int64_t)a.k || (a.cap & (a.cap - 1))) { LEGION_ARG_ERROR("k_lp_pairs: the table's capacity must be a power of two of at least 4 k slots"); return; }
    LEGION_AUDIT_LAUNCH(s, "k_lp_pairs", LEGION_AW(a.pairs), LEGION_AW(a.excluded), LEGION_AL(a.ids), LEGION_AL(a.nc));
    k_lp_pairs<<<1, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
}

// ------------------------------------------------------------------------------------------------
// The marking pass: edge_keep[e] = 0 where {ids[dst_off[e]], ids[src_off[e]]} is a target pair, else 1
// ------------------------------------------------------------------------------------------------
// ids[0, B) are the seed slots verbatim and every node found later has a position >= B, so an edge can join two seeds only if both of its
// offsets are < B: decided from the two streamed words.  Only then are the two ids loaded and the table walked -- to the key, to an empty
// slot, or cap steps.
__device__ inline bool lp_is_target(const LpKeepArgs& a, uint32_t B, int32_t s, int32_t d)
{
    if ((uint32_t)s >= B || (uint32_t)d >= B) return false;
    const int32_t u = a.ids[d], v = a.ids[s];
    if (u < 0 || v < 0) return false;
    const uint32_t cap = (uint32_t)a.cap;
    const uint64_t key = lp_pair_key(u, v);
    uint32_t slot = lp_pair_slot((uint32_t)(key >> 32), (uint32_t)key, cap);
    for (uint32_t step = 0; step < cap; step++) {
        const uint64_t t = a.pairs[slot];
        if (t == key) return true;
        if (t == kLpEmpty) return false;
        slot = (slot + 1u) & (cap - 1u);
    }
    return false;
}

// A persistent grid over groups of four consecutive edges, one group per lane and trip: one 16-byte load of src_off and of dst_off and one
// 4-byte store of the four keep bytes (VEC: the three buffers are aligned for that; else, and in the last partial group, element by
// element).  Exactly the bytes edge_keep[0, E) are stored, E = legion_batch_edges clamped to the capacity.  The zeros are counted per hop in
// registers, reduced per wave by shuffles and per workgroup through LDS; one integer atomicAdd per hop with a zero and workgroup, and one for
// the total -- integer adds in any order give the same words.  !active: ones everywhere, and workgroup 0 zeroes the counts nobody adds to.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_lp_edge_keep(LpKeepArgs a)
{
    constexpr int W = kBlock / 64, HH = LEGION_MAX_HOPS;
    __shared__ int32_t s_cnt[W][HH];
    const int32_t E = max(min(legion_batch_edges(a.ec, a.hops), a.ids_cap), 0);
    const int32_t n0 = legion_level_size(a.nc, 0);
    const uint32_t B = a.active && n0 == 3 * a.k ? (uint32_t)min(n0, a.ids_cap) : 0u;
    int32_t end[HH], cnt[HH];
#pragma unroll
    for (int h = 0; h < HH; h++) {
        end[h] = h < a.hops ? max(min(legion_edges_through(a.ec, h + 1), E), 0) : E;
        cnt[h] = 0;
    }
    if (!a.active && blockIdx.x == 0 && threadIdx.x < kLpExcludedWords) a.excluded[threadIdx.x] = 0;
    const int32_t groups = (int32_t)(((int64_t)E + 3) >> 2);
    for (int32_t g = blockIdx.x * kBlock + threadIdx.x; g < groups; g += gridDim.x * kBlock) {
        const int32_t e0 = g << 2;
        const bool full = e0 + 4 <= E;
        int32_t s[4] = {-1, -1, -1, -1}, d[4] = {-1, -1, -1, -1};
        if (VEC && full) {
            const int4 sv = *(const int4*)(a.src_off + e0), dv = *(const int4*)(a.dst_off + e0);
            s[0] = sv.x; s[1] = sv.y; s[2] = sv.z; s[3] = sv.w;
            d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (e0 + j < E) { s[j] = a.src_off[e0 + j]; d[j] = a.dst_off[e0 + j]; }
        }
        uint32_t word = 0x01010101u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (lp_is_target(a, B, s[j], d[j])) {
                word &= ~(1u << (8 * j));
                const int32_t e = e0 + j;
                int32_t lo = 0;
#pragma unroll
                for (int h = 0; h < HH; h++) { cnt[h] += e >= lo && e < end[h]; lo = end[h]; }
            }
        }
        if (VEC && full) *(uint32_t*)(a.keep + e0) = word;
        else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (e0 + j < E) a.keep[e0 + j] = (uint8_t)(word >> (8 * j));
        }
    }
    if (!B) return;   // uniform over the grid: nothing was looked up, nothing is counted
#pragma unroll
    for (int h = 0; h < HH; h++) {
        int32_t c = cnt[h];
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
        if (lane_id() == 0) s_cnt[wave_id()][h] = c;
    }
    __syncthreads();
    if (threadIdx.x <= HH) {   // thread h < HH: hop h + 1; thread HH: the total
        int32_t c = 0;
        for (int h = 0; h < HH; h++)
            if ((int)threadIdx.x == h || (int)threadIdx.x == HH)
                for (int w = 0; w < W; w++) c += s_cnt[w][h];
        if (c) atomicAdd(a.excluded + ((int)threadIdx.x == HH ? 0 : (int)threadIdx.x + 1), c);
    }
}

// The grid rule of k_lp_edge_keep (tests/test_gpu_lp_exclude.py restates it to size its several-trips case): one workgroup per
// kBlock * 4 edges of the pool's static bound, at most kLpKeepBlocksPerCu per compute unit.  Four workgroups of 256 threads keep half of a
// CU's wave slots busy, which a pass of 16-byte loads and 4-byte stores does not need more of; the grid is resident at once and every lane
// loops over the rest.
constexpr int kLpKeepBlocksPerCu = 4;
void launch_lp_edge_keep(hipStream_t s, const LpKeepArgs& a, int32_t edges_bound)
{
    if (edges_bound <= 0 || a.ids_cap <= 0) return;
    if (a.hops < 1 || a.hops > LEGION_MAX_HOPS || a.k <= 0 || (a.active && (a.cap < 4 * (int64_t)a.k || (a.cap & (a.cap - 1))))) { LEGION_ARG_ERROR("k_lp_edge_keep: bad hop count, triple count or table capacity"); return; }
    LEGION_AUDIT_LAUNCH(s, "k_lp_edge_keep", LEGION_AW(a.keep), LEGION_AW(a.excluded), LEGION_AL(a.pairs), LEGION_AL(a.ids), LEGION_AL(a.src_off), LEGION_AL(a.dst_off), LEGION_AL(a.nc), LEGION_AL(a.ec));
    const int grid = grid_for(std::min(edges_bound, a.ids_cap), kBlock * 4, kLpKeepBlocksPerCu);
    const bool vec = ((uintptr_t)a.src_off | (uintptr_t)a.dst_off) % 16 == 0 && (uintptr_t)a.keep % 4 == 0;
    if (vec) k_lp_edge_keep<true><<<grid, kBlock, 0, s>>>(a);
    else k_lp_edge_keep<false><<<grid, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
}

} // namespace legion
