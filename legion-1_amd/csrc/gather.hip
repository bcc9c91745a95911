// gather.hip -- the feature side of a batch: the stand-alone cache lookups, the row gathers, the aggregated (and normalised) last hop and
// the owner-computes exchange passes, with their launch wrappers.  Stage names (S5, S6) as in sampler.hip.
#include "internal.h"
#include "draws.h"
#include "launch.h"

#include "audit_hooks.h"

namespace legion {

// ------------------------------------------------------------------------------------------------
// S6: stand-alone lookups (API parity with FindFeat / FindTopo; the hot path fuses them)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_find_feat(const int32_t* __restrict__ sampled_ids,
                                                      int32_t* __restrict__ cache_offset,
                                                      const int32_t* __restrict__ nc, int32_t off_idx,
                                                      int32_t size_idx, const int32_t* __restrict__ feat_map)
{
    const int32_t off = nc[off_idx], n = nc[size_idx];
    for (int32_t r = threadIdx.x + blockDim.x * blockIdx.x; r < n; r += gridDim.x * blockDim.x) {
        int32_t id = sampled_ids[off + r];
        cache_offset[r] = (id < 0 || !feat_map) ? -1 : feat_map[id];
    }
}

__global__ __launch_bounds__(kBlock) void k_find_topo(const int32_t* __restrict__ input_ids,
                                                      int8_t* __restrict__ part_index,
                                                      int32_t* __restrict__ part_offset, int32_t n,
                                                      const int8_t* __restrict__ owner,
                                                      const int32_t* __restrict__ row)
{
    for (int32_t i = threadIdx.x + blockDim.x * blockIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int32_t id = input_ids[i];
        bool ok = id >= 0 && owner;
        part_index[i] = ok ? owner[id] : (int8_t)-1;
        part_offset[i] = ok ? row[id] : -1;
    }
}

// ------------------------------------------------------------------------------------------------
// S5: feature gather from the unified cache / the backing table
// ------------------------------------------------------------------------------------------------
struct GatherKArgs {
    GatherArgs g;
    FastDiv div_c;   // / chunks-per-row
    FastDiv div_cap; // / cache_capacity
};

typedef float v4f __attribute__((ext_vector_type(4)));

// Source selection of one feature row (GPUCache.cu:387-400, Kernels.cu:672-691): cache slot gidx (FindFeat's answer, < 0 = miss) ->
// (clique GPU, chunk, row) of the shard tables, else row id % V of the backing table, else no source.  Pitches in floats.
// The one copy k_row_ptrs, k_gather_lookup and k_gather_sum share.
__device__ inline const float* row_source(const GatherArgs& g, const FastDiv& div_cap, int32_t id, int32_t gidx, int64_t tpitch, int64_t spitch)
{
    if (gidx >= 0) {
        const uint32_t didx = fdiv((uint32_t)gidx, div_cap);
        const uint32_t fidx = (uint32_t)gidx - didx * (uint32_t)g.cache_capacity;
        const float* chunk = g.shard_tab[didx * (uint32_t)g.nchunks + (fidx >> g.chunk_shift)];
        return chunk + (int64_t)(fidx & ((1u << g.chunk_shift) - 1u)) * spitch;
    }
    if (id >= 0 && g.table) return g.table + (int64_t)(id % g.total_num_nodes) * tpitch;
    return nullptr;
}

// FindFeat + source selection for the rows of one gather launch (GPUCache.cu:387-400, Kernels.cu:672-691): one thread
// per ROW resolves id -> cache slot -> (clique GPU, chunk, row) -> address, or the backing-table row on a miss.  The
// gather then starts every row with one coalesced 8-byte load; done inside the gather, the map probe and the
// chunk-table load sit on the critical path of every 16-byte chunk (profiles/r01_gather_sweep.md).
__global__ __launch_bounds__(kBlock) void k_row_ptrs(GatherKArgs a)
{
    constexpr int U = 4; // rows per thread and step: U independent map probes in flight
    const GatherArgs& g = a.g;
    const int32_t off = g.off_idx < 0 ? 0 : g.nc[g.off_idx];
    const int32_t rows = g.nc[g.size_idx];
    const int32_t stride = gridDim.x * blockDim.x;
    for (int32_t r0 = threadIdx.x + blockDim.x * blockIdx.x; r0 < rows; r0 += stride * U) {
        int32_t id[U], gidx[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int32_t r = r0 + u * stride;
            id[u] = r < rows ? g.sampled_ids[off + r] : -1;
        }
#pragma unroll
        for (int u = 0; u < U; u++) gidx[u] = (id[u] >= 0 && g.feat_map) ? g.feat_map[id[u]] : -1;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int32_t r = r0 + u * stride;
            if (r >= rows) continue;
            g.row_ptr[r] = row_source(g, a.div_cap, id[u], gidx[u], g.table_pitch > 0 ? g.table_pitch : g.F, g.shard_pitch > 0 ? g.shard_pitch : g.F);
        }
        if (g.hit_stats) { // feature_cache_hit (GPUCache.cu:130-147): one atomic per wave and step
            int32_t h = 0;
#pragma unroll
            for (int u = 0; u < U; u++) h += (r0 + u * stride < rows && gidx[u] >= 0) ? 1 : 0;
            for (int o = 32; o > 0; o >>= 1) h += __shfl_down(h, o);
            if (lane_id() == 0 && h) atomicAdd(g.hit_stats, h);
        }
    }
    if (g.hit_stats && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(g.hit_stats + 1, rows);
}

// Row layout of the flat work space: q -> (row, 16-byte chunk) = (q / C, q % C) -- a wave covers 64 consecutive chunks whatever
// the row length.  (A row-aligned layout -- 2^k lanes per row, the lanes >= C idle -- lost 5 % at F = 100:
// profiles/r03_other_shapes.md; kept as profiles/r06_removed_experiments.patch.)
template <typename VT, int UNROLL, int NT>
__global__ __launch_bounds__(kBlock) void k_gather(GatherKArgs a)
{
    constexpr int VEC = sizeof(VT) / 4;
    const GatherArgs& g = a.g;
    const int32_t off = g.off_idx < 0 ? 0 : g.nc[g.off_idx];
    const int32_t rows = g.nc[g.size_idx];
    const int32_t C = g.F / VEC;
    const int64_t total = (int64_t)rows * C;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t pitch = g.table_pitch > 0 ? g.table_pitch : g.F;   // floats between two rows of the backing table
    if (g.rows_seen && blockIdx.x == 0 && threadIdx.x == 0) *g.rows_seen = rows; // launch-size feedback for later batches
    for (int64_t q0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q0 < total; q0 += stride * UNROLL) {
        const VT* src[UNROLL];
        VT val[UNROLL];
        int64_t dsti[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int64_t q = q0 + u * stride;
            src[u] = nullptr;
            dsti[u] = 0;
            if (q < total) {
                const uint32_t r = fdiv((uint32_t)q, a.div_c); // rows*C < 2^31 is checked by the launcher
                const uint32_t ch = (uint32_t)q - r * (uint32_t)C;
                if (g.dst_rows > 0 && off + (int32_t)r >= g.dst_rows) continue; // never write past the buffer
                dsti[u] = ((int64_t)(off + (int32_t)r) * g.F) / VEC + ch;
                if (g.row_ptr) { // resolved by k_row_ptrs
                    const float* p = g.row_ptr[r];
                    if (p) src[u] = reinterpret_cast<const VT*>(p) + ch;
                    continue;
                }
                const int32_t id = g.sampled_ids[off + (int32_t)r]; // no cache: the backing table row (Kernels.cu:689)
                if (id >= 0) src[u] = reinterpret_cast<const VT*>(g.table + (int64_t)(id % g.total_num_nodes) * pitch) + ch;
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; u++)
            if (src[u]) val[u] = (NT >= 2) ? __builtin_nontemporal_load(src[u]) : *src[u];
#pragma unroll
        for (int u = 0; u < UNROLL; u++)
            if (src[u]) {
                if (NT >= 1) __builtin_nontemporal_store(val[u], reinterpret_cast<VT*>(g.dst) + dsti[u]);
                else reinterpret_cast<VT*>(g.dst)[dsti[u]] = val[u];
            }
    }
}

// ------------------------------------------------------------------------------------------------
// S5, edge features (no counterpart in the reference): edge_feat[e, :] = X[edge_ids[e], :]
// ------------------------------------------------------------------------------------------------
// The counterpart of k_gather for the graph's per-edge table (GPUGraphStorage_SetEdgeFeatures): float32 [E, dim], dense, in CSR order, row
// edge_ids[e] of it for every COO edge e of one hop (hop == 0: of the batch).  It reads the batch's PIPE only -- edge_ids as k_edge_ids left
// them, and ec -- and the table; never cand, cols, the tile prefixes, hop_state or the position table, which belong to the next batch's
// sampler while this runs on the gather stream.  The edge range comes from ec on the device, clamped to the buffers' capacity; the grid is
// persistent, sized from the hop's static bound.
// Another regime than k_gather: rows of 4-256 bytes (C = 1..16 chunks), 64-bit ids into a table of up to 1.6 G rows -- the source row is
// table + id * dim in 64-bit arithmetic throughout, only the flat work space (edge, chunk) is 32-bit-divided -- and the chain is id -> row,
// two dependent trips: U independent id loads go out, then U row loads, then U stores.  An id outside [0, E) cannot occur in a correct batch;
// if one does it forms no address and the row is stored as zeros (the pool's poison rule).  Every edge of the range is stored and nothing
// else.  Non-temporal loads and stores as in k_gather: a row is read for this edge and written once for a reader in another process.
struct EdgeGatherKArgs {
    EdgeGatherArgs g;
    FastDiv div_c;   // / chunks-per-row
};

template <typename VT, int U>
__global__ __launch_bounds__(kBlock) void k_gather_edges(EdgeGatherKArgs a)
{
    constexpr int VEC = sizeof(VT) / 4;
    const EdgeGatherArgs& g = a.g;
    const int32_t lo = g.hop > 0 ? legion_hop_edges_begin(g.ec, g.hop) : 0;
    const int32_t hi = g.hop > 0 ? legion_hop_edges_end(g.ec, g.hop) : legion_batch_edges(g.ec, g.hops);
    const int32_t e0 = max(lo, 0), e1 = min(hi, g.ids_cap);   // never past edge_ids / out, whatever the counters hold
    const int32_t C = g.dim / VEC;
    const int64_t total = e1 > e0 ? (int64_t)(e1 - e0) * C : 0;   // < 2^31: ids_cap * C is checked by the launcher
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q0 < total; q0 += stride * U) {
        int64_t id[U], dsti[U];
        uint32_t ch[U];
        VT val[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t q = q0 + u * stride;
            id[u] = -1; dsti[u] = -1; ch[u] = 0;
            if (q < total) {
                const uint32_t r = fdiv((uint32_t)q, a.div_c);
                ch[u] = (uint32_t)q - r * (uint32_t)C;
                const int64_t e = (int64_t)e0 + r;
                dsti[u] = e * C + ch[u];
                id[u] = g.edge_ids[e];
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            val[u] = VT(0.0f);
            if (id[u] >= 0 && id[u] < g.E) {
                const VT* src = reinterpret_cast<const VT*>(g.table + id[u] * (int64_t)g.dim) + ch[u];
                val[u] = __builtin_nontemporal_load(src);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (dsti[u] >= 0) __builtin_nontemporal_store(val[u], reinterpret_cast<VT*>(g.out) + dsti[u]);
    }
}

// (cached gather, same box, papers100M shape, 25 % of the rows cached: lookup pass k_row_ptrs + k_gather 416-423 us; k_gather_lookup<U> with U = 1: 455,
// U = 2: 412-414, U = 4: 418 (profiles/r04_cached_gather.md) -- the probes themselves (1.94 M random 4-byte reads of a 444 MB map) bound it: U = 2 is built)
// FindFeat inside the gather, ONE probe per row and wave: the first lane a wave gives to a row resolves
// id -> cache slot -> (clique GPU, chunk, row) -> source address (GPUCache.cu:387-400, Kernels.cu:672-691) and hands the address to
// the row's other lanes by __shfl -- F = 128: two probes per wave instead of 64 (round 1 probed in every chunk lane: 426 us), no
// row_ptr round trip through memory, no second launch.  The probe chain (id, map, chunk table) sits in front of the row loads of
// the wave, so U work items per lane are resolved together: U chains overlap instead of following each other.
template <typename VT, int U>
__global__ __launch_bounds__(kBlock) void k_gather_lookup(GatherKArgs a)
{
    constexpr int VEC = sizeof(VT) / 4;
    const GatherArgs& g = a.g;
    const int32_t off = g.off_idx < 0 ? 0 : g.nc[g.off_idx];
    const int32_t rows = g.nc[g.size_idx];
    const int32_t C = g.F / VEC;
    const int64_t total = (int64_t)rows * C;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tpitch = g.table_pitch > 0 ? g.table_pitch : g.F, spitch = g.shard_pitch > 0 ? g.shard_pitch : g.F;
    const int lane = lane_id();
    if (g.rows_seen && blockIdx.x == 0 && threadIdx.x == 0) *g.rows_seen = rows;
    for (int64_t q0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q0 - lane < total; q0 += stride * U) {   // whole waves stay in the loop: shuffles below
        uint32_t r[U], ch[U];
        int32_t id[U], gidx[U];
        bool lead[U], live[U];
        int src_lane[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t q = q0 + u * stride;
            live[u] = q < total;
            r[u] = fdiv((uint32_t)(live[u] ? q : 0), a.div_c);           // rows * C < 2^31 is checked by the launcher
            ch[u] = (uint32_t)(live[u] ? q : 0) - r[u] * (uint32_t)C;
            // first lane of this wave that works on row r: the row's chunk 0 if it sits in this wave, else lane 0
            const int64_t first = (int64_t)r[u] * C - (q - lane);
            src_lane[u] = first > 0 ? (int)first : 0;
            lead[u] = live[u] && lane == src_lane[u];
            id[u] = lead[u] ? g.sampled_ids[off + (int32_t)r[u]] : -1;
        }
#pragma unroll
        for (int u = 0; u < U; u++) gidx[u] = (lead[u] && id[u] >= 0) ? g.feat_map[id[u]] : -1;
        const VT* src[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const float* p = lead[u] ? row_source(g, a.div_cap, id[u], gidx[u], tpitch, spitch) : nullptr;
            const unsigned long long bits = (unsigned long long)(uintptr_t)p;
            const uint32_t lo = __shfl((uint32_t)bits, src_lane[u]), hi = __shfl((uint32_t)(bits >> 32), src_lane[u]);
            const float* rp = (const float*)(uintptr_t)(((unsigned long long)hi << 32) | lo);
            src[u] = (live[u] && rp && !(g.dst_rows > 0 && off + (int32_t)r[u] >= g.dst_rows)) ? reinterpret_cast<const VT*>(rp) + ch[u] : nullptr;
        }
        VT val[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            if (src[u]) val[u] = __builtin_nontemporal_load(src[u]);
#pragma unroll
        for (int u = 0; u < U; u++)
            if (src[u]) __builtin_nontemporal_store(val[u], reinterpret_cast<VT*>(g.dst) + ((int64_t)(off + (int32_t)r[u]) * g.F) / VEC + ch[u]);
    }
    // (feature_cache_hit, GPUCache.cu:130-147, is counted by the lookup PASS: the launcher sends every batch whose hit rate is
    // sampled through k_row_ptrs, which sees each row exactly once -- here a row that straddles two waves is probed by both)
}

// ------------------------------------------------------------------------------------------------
// S5, aggregated last hop (no counterpart in the reference): neighbour sums per input slot of the last hop
// ------------------------------------------------------------------------------------------------
// The rows found in the last hop are read by a GraphSAGE trainer for one thing: being summed into their hop-(H-1) neighbours.  This
// kernel hands over those sums instead of the rows.  Run i = input slot i of the last hop (a seed at H = 1, else edge i of hop H - 1);
// its draws are what k_sample parked in cand[i * f .. i * f + f), < 0 = no draw.
//   S[i, :] = ((0.0f + x[c(i, j0)]) + x[c(i, j1)]) + ...   over the j with a draw, ascending j, fp32, no reassociation
// written dense behind the n_in rows of the levels < H: dst row n_in + i.  A run without draws stores +0.0 (the buffer is reused).
// Work space like k_gather: flat (run, 16-byte chunk), one chunk per lane; per lane U slot ids of its run, their sources and their
// row loads go out together, then the adds in slot order.  Every run has at most f terms: even work, no atomics, and the order of
// the adds is fixed by construction, so the sums are bitwise reproducible.
// A hub row is read once per draw here (13-18 % of the papers100M last-hop draws repeat inside a 1-2 Ki-slot tile,
// profiles/r06_dedup_census.md), unlike k_gather's read-once rows: NT picks non-temporal row loads (profiles/agg_last_hop.md).
#ifndef LEGION_AGG_NT_LOADS
#define LEGION_AGG_NT_LOADS 0
#endif
struct GatherSumArgs {
    GatherArgs g;            // table / shards / map / pitches / F / dst / dst_rows / nc of the pipe (sampled_ids, row_ptr: unused)
    FastDiv div_c;           // / chunks-per-row
    FastDiv div_cap;         // / cache_capacity
    const int32_t* cand;     // the last hop's draws (the pipe's own buffer)
    const int32_t* ec;
    int32_t hops, f;
    int32_t cand_cap;        // elements of cand
    const float* wdraw;      // WT: the weight of every draw, by slot (k_draw_weights; the pipe's own buffer, cand_cap elements)
};

// WT (normalised sums, "S5, normalised last hop" below): every row is scaled by its draw's weight before it is added, the product and the
// add rounded separately -- S_w[i, :] = ((0.0f + fl(w0 * x0)) + fl(w1 * x1)) + ... -- which is what a trainer computes when it scales the
// rows first (GraphConv norm='both') and what NumPy states; a fused multiply-add would round once.
template <typename VT, int U, bool NT, bool WT>
__global__ __launch_bounds__(kBlock) void k_gather_sum(GatherSumArgs a)
{
    constexpr int VEC = sizeof(VT) / 4;
    const GatherArgs& g = a.g;
    const int32_t n_in = legion_first_block_dst(g.nc, a.hops);
    const int32_t runs = legion_hop_inputs(g.nc, a.ec, a.hops);
    const int32_t C = g.F / VEC;
    const int64_t total = (int64_t)runs * C;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tpitch = g.table_pitch > 0 ? g.table_pitch : g.F, spitch = g.shard_pitch > 0 ? g.shard_pitch : g.F;
    if (g.rows_seen && blockIdx.x == 0 && threadIdx.x == 0) *g.rows_seen = runs; // launch-size feedback for later batches
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
        const uint32_t i = fdiv((uint32_t)q, a.div_c); // runs * C < 2^31 is checked by the launcher
        const uint32_t ch = (uint32_t)q - i * (uint32_t)C;
        if (g.dst_rows > 0 && (int64_t)n_in + i >= g.dst_rows) continue; // never write past the buffer
        const int64_t slot0 = (int64_t)i * a.f;
        VT acc = VT(0.0f);
        for (int32_t j0 = 0; j0 < a.f; j0 += U) {
            int32_t id[U], gidx[U];
            const VT* src[U];
            VT val[U];
            float wt[WT ? U : 1];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t idx = slot0 + j0 + u;
                id[u] = (j0 + u < a.f && idx < a.cand_cap) ? a.cand[idx] : -1;
                if constexpr (WT) wt[u] = (j0 + u < a.f && idx < a.cand_cap) ? a.wdraw[idx] : 0.0f;   // streamed beside the draw; read only where the slot has one
            }
#pragma unroll
            for (int u = 0; u < U; u++) gidx[u] = (id[u] >= 0 && g.feat_map) ? g.feat_map[id[u]] : -1;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const float* p = row_source(g, a.div_cap, id[u], gidx[u], tpitch, spitch);
                src[u] = p ? reinterpret_cast<const VT*>(p) + ch : nullptr;
            }
#pragma unroll
            for (int u = 0; u < U; u++)
                if (src[u]) val[u] = NT ? __builtin_nontemporal_load(src[u]) : *src[u];
            if constexpr (WT) {
#pragma clang fp contract(off)
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (src[u]) acc = acc + val[u] * wt[u];
            } else {
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (src[u]) acc = acc + val[u];
            }
        }
        __builtin_nontemporal_store(acc, reinterpret_cast<VT*>(g.dst) + ((int64_t)(n_in + (int32_t)i) * g.F) / VEC + ch);
    }
}

// ------------------------------------------------------------------------------------------------
// S5, normalised last hop (no counterpart in the reference): the sums a GraphConv(norm='both') first layer needs
// ------------------------------------------------------------------------------------------------
// GraphConv(norm='both') scales every source row of block 1 by outdeg^-1/2, the out-degree counted INSIDE the block:
//   d[p] = #{ e < E : src_off[e] == p },  w[p] = 1.0f / sqrtf((float)max(d[p], 1))    (both correctly rounded)
// The block is the server's own output, so the server can weight the last hop's rows before it sums them (k_gather_sum<WT>).  Three
// small passes in front of the sums, all over data of the batch's PIPE (its draws, its COO, its counters: the pool's shared sampler
// scratch belongs to the next batch by then):
//   k_agg_norm_prep     zeroes d[0, n) and counts the draws (slots with cand != -1) of each chunk of slots;
//   k_block_out_deg     counts d over src_off[0, E) with integer atomics (order-independent: reproducible), one atomic per run of
//                       equal neighbouring lanes -- hub positions repeat in adjacent lanes;
//   k_draw_weights      k_write appended the last hop's edges in slot order, one per slot with a draw, so the edge of such a slot is
//                       (edges of the hops < H) + (draws in front of it): every workgroup adds up the chunk counts in front of its
//                       chunk (<= kMaxChunks words, no scan launch, no device-scope hand-off: k_write's scheme), ranks its slots by
//                       ballot, and leaves wdraw[slot] = w[src_off[edge]].
// A chunk is a contiguous range of slots, the same for the first and the third pass (both derive it from the slot count on the device
// and their common grid).
__device__ inline int64_t agg_norm_chunk_len(int64_t total, int32_t chunks)
{
    const int64_t per = (total + chunks - 1) / chunks;
    return (per + kBlock - 1) / kBlock * kBlock;
}
__device__ inline int64_t agg_norm_slots(const AggNormArgs& a)
{
    return min((int64_t)legion_hop_inputs(a.nc, a.ec, a.hops) * a.f, (int64_t)a.cand_cap);
}

__global__ __launch_bounds__(kBlock) void k_agg_norm_prep(AggNormArgs a)
{
    constexpr int W = kBlock / 64;
    __shared__ int32_t s_w[W];
    const int32_t n = min(legion_batch_nodes(a.nc, a.hops), a.ids_cap);
    for (int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x); p < n; p += (int32_t)(gridDim.x * kBlock)) a.out_deg[p] = 0;
    const int64_t total = agg_norm_slots(a);
    const int64_t len = agg_norm_chunk_len(total, (int32_t)gridDim.x);
    const int64_t lo = min((int64_t)blockIdx.x * len, total), hi = min(lo + len, total);
    int32_t mine = 0;
    for (int64_t idx = lo + threadIdx.x; idx < hi; idx += kBlock) mine += a.cand[idx] != -1;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if (lane_id() == 0) s_w[wave_id()] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t t = 0;
#pragma unroll
        for (int w = 0; w < W; w++) t += s_w[w];
        a.chunk_cnt[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kBlock) void k_block_out_deg(AggNormArgs a)
{
    const int32_t E = min(legion_batch_edges(a.ec, a.hops), a.ids_cap);
    const int lane = lane_id();
    const int32_t stride = (int32_t)(gridDim.x * kBlock);
    for (int32_t base = (int32_t)(blockIdx.x * kBlock); base < E; base += stride) {   // whole waves: the lanes settle their repeats together
        const int32_t e = base + (int32_t)threadIdx.x;
        const bool valid = e < E;
        const int32_t p = valid ? a.src_off[e] : -1;
        const int32_t before = __shfl_up(p, 1);
        const bool head = valid && (lane == 0 || before != p);
        // a run of equal positions ends in front of the next head or the first lane beyond E: its head adds the run's length
        const unsigned long long ends = __ballot(head) | ~__ballot(valid);
        const unsigned long long above = lane == 63 ? 0ull : ends & ~((2ull << lane) - 1ull);
        const int32_t run = (above ? __ffsll((long long)above) - 1 : 64) - lane;
        if (head && LEGION_STORE_OK(p, a.ids_cap)) atomicAdd(a.out_deg + p, run);     // no return value: fire and forget
    }
}

__global__ __launch_bounds__(kBlock) void k_draw_weights(AggNormArgs a)
{
    constexpr int W = kBlock / 64, PER = kMaxChunks / kBlock;
    __shared__ int32_t s_w[W];
    __shared__ int32_t s_c[W];
    const int lane = lane_id(), wave = wave_id();
    const unsigned long long lt = (1ull << lane) - 1ull;
    // draws in front of this workgroup's chunk
    int32_t mine = 0;
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int32_t c = (int32_t)threadIdx.x + kBlock * u;
        if (c < (int32_t)blockIdx.x) mine += a.chunk_cnt[c];
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if (lane == 0) s_w[wave] = mine;
    __syncthreads();
    int32_t rank0 = 0;
#pragma unroll
    for (int w = 0; w < W; w++) rank0 += s_w[w];
    const int32_t e_in = legion_hop_edges_begin(a.ec, a.hops);   // edges of the hops < H
    const int32_t E = min(legion_batch_edges(a.ec, a.hops), a.ids_cap);
    const int64_t total = agg_norm_slots(a);
    const int64_t len = agg_norm_chunk_len(total, (int32_t)gridDim.x);
    const int64_t lo = min((int64_t)blockIdx.x * len, total), hi = min(lo + len, total);
    for (int64_t s0 = lo; s0 < hi; s0 += kBlock) {
        const int64_t idx = s0 + threadIdx.x;
        const bool draw = idx < hi && a.cand[idx] != -1;
        const unsigned long long b = __ballot(draw);
        if (lane == 0) s_c[wave] = __popcll(b);
        __syncthreads();
        int32_t r = rank0 + __popcll(b & lt), all = 0;
#pragma unroll
        for (int w = 0; w < W; w++) {
            if (w < wave) r += s_c[w];
            all += s_c[w];
        }
        if (draw) {
            const int32_t e = e_in + r;
            const int32_t p = e < E ? a.src_off[e] : -1;
            const int32_t d = LEGION_STORE_OK(p, a.ids_cap) ? a.out_deg[p] : 1;
            a.wdraw[idx] = 1.0f / sqrtf((float)max(d, 1));
        }
        rank0 += all;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// S5, edge-weighted last hop (no counterpart in the reference): the sums a GraphConv / GCNConv with edge_weight needs
// ------------------------------------------------------------------------------------------------
// S_e[i, :] = ((0.0f + fl(edge_w[e(i, j0)] * x[c(i, j0)])) + fl(edge_w[e(i, j1)] * x[c(i, j1)])) + ...  -- k_gather_sum<WT> as it is, over
// wdraw[slot] = edge_w[edge of the slot's draw], edge_w being what k_edge_ids left in the pipe's buffer behind the last hop.  The slot -> edge
// rank is k_draw_weights': the edge of a slot with a draw is (edges of the hops < H) + (draws in front of it).  One kernel, launched twice on
// one grid: COUNT leaves the draws of every chunk of slots in chunk_cnt (k_agg_norm_prep's count without its zeroing of out_deg, a buffer
// this mode does not hold); the second pass adds up the chunk counts in front of its chunk in LDS, ranks its slots by ballot and stores the
// weights.  A rank beyond the batch's (clamped) edges gets 0.0f.  Reads the batch's own pipe only; plain vector stores, no atomics.
__device__ inline int64_t agg_norm_slots(const AggEdgeWeightArgs& a)
{
    return min((int64_t)legion_hop_inputs(a.nc, a.ec, a.hops) * a.f, (int64_t)a.cand_cap);
}

template <bool COUNT>
__global__ __launch_bounds__(kBlock) void k_draw_edge_weights(AggEdgeWeightArgs a)
{
    constexpr int W = kBlock / 64, PER = kMaxChunks / kBlock;
    __shared__ int32_t s_w[W];
    __shared__ int32_t s_c[W];
    const int lane = lane_id(), wave = wave_id();
    const int64_t total = agg_norm_slots(a);
    const int64_t len = agg_norm_chunk_len(total, (int32_t)gridDim.x);
    const int64_t lo = min((int64_t)blockIdx.x * len, total), hi = min(lo + len, total);
    int32_t mine = 0;
    if constexpr (COUNT) {
        for (int64_t idx = lo + threadIdx.x; idx < hi; idx += kBlock) mine += a.cand[idx] != -1;
    } else {   // draws in front of this workgroup's chunk
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int32_t c = (int32_t)threadIdx.x + kBlock * u;
            if (c < (int32_t)blockIdx.x) mine += a.chunk_cnt[c];
        }
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if (lane == 0) s_w[wave] = mine;
    __syncthreads();
    int32_t rank0 = 0;
#pragma unroll
    for (int w = 0; w < W; w++) rank0 += s_w[w];
    if constexpr (COUNT) {
        if (threadIdx.x == 0) a.chunk_cnt[blockIdx.x] = rank0;
    } else {
        const unsigned long long lt = (1ull << lane) - 1ull;
        const int32_t e_in = legion_hop_edges_begin(a.ec, a.hops);   // edges of the hops < H
        const int32_t E = min(legion_batch_edges(a.ec, a.hops), a.ids_cap);
        for (int64_t s0 = lo; s0 < hi; s0 += kBlock) {
            const int64_t idx = s0 + threadIdx.x;
            const bool draw = idx < hi && a.cand[idx] != -1;
            const unsigned long long b = __ballot(draw);
            if (lane == 0) s_c[wave] = __popcll(b);
            __syncthreads();
            int32_t r = rank0 + __popcll(b & lt), all = 0;
#pragma unroll
            for (int w = 0; w < W; w++) {
                if (w < wave) r += s_c[w];
                all += s_c[w];
            }
            if (draw) {
                const int32_t e = e_in + r;
                a.wdraw[idx] = e >= 0 && e < E ? a.edge_w[e] : 0.0f;
            }
            rank0 += all;
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// S5, owner-computes exchange variant (SURVEY 5 option b; one process per GPU): rows whose cache slot lives on another
// clique member are not read in-kernel over xGMI; the requester lists them per owner, the owners gather them from their
// own HBM and the rows come back in one all-to-all (RCCL / hipMemcpyPeer).  Everything else is gathered as usual.
// ------------------------------------------------------------------------------------------------
struct ExchArgs {
    GatherArgs g;
    FastDiv div_cap;
    int32_t me;               // this GPU's index inside its clique
    int32_t Kg;
    int32_t* slot;            // scratch [rows]: FindFeat result of the count pass
    int32_t* counts;          // [Kg]: rows requested from each clique member (me: 0)
    int32_t* cursor;          // [Kg]: fill cursors (zeroed by the count pass)
    int32_t* req_row;         // out, grouped by owner: row inside the owner's shard
    int32_t* req_dst;         // out, same order: destination row of the batch
};
// pass 1: FindFeat (GPUCache.cu:387-400) per row + rows per owner.  One LDS histogram per workgroup, Kg atomics per workgroup.
__global__ __launch_bounds__(kBlock) void k_exch_count(ExchArgs a)
{
    __shared__ int32_t s_cnt[kMaxParts];
    const GatherArgs& g = a.g;
    const int32_t rows = g.nc[g.size_idx];
    if (threadIdx.x < kMaxParts) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int32_t r = threadIdx.x + blockDim.x * blockIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const int32_t id = g.sampled_ids[r];
        const int32_t gidx = (id >= 0 && g.feat_map) ? g.feat_map[id] : -1;
        a.slot[r] = gidx;
        if (gidx >= 0) {
            const int32_t owner = (int32_t)fdiv((uint32_t)gidx, a.div_cap);
            if (owner != a.me) atomicAdd(&s_cnt[owner], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < a.Kg && s_cnt[threadIdx.x]) atomicAdd(a.counts + threadIdx.x, s_cnt[threadIdx.x]);
}
// pass 2: the request lists (contiguous per owner, owner-major) and the source address of every row that is served
// locally (own shard / backing table); rows owned by a peer get no address: the local gather skips them.
__global__ __launch_bounds__(kBlock) void k_exch_fill(ExchArgs a)
{
    __shared__ int32_t s_cnt[kMaxParts], s_base[kMaxParts];
    const GatherArgs& g = a.g;
    const int32_t rows = g.nc[g.size_idx];
    const int32_t per_wg = (rows + gridDim.x - 1) / gridDim.x;
    const int32_t r0 = blockIdx.x * per_wg, r1 = min(r0 + per_wg, rows);
    if (threadIdx.x < kMaxParts) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int32_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
        const int32_t gidx = a.slot[r];
        if (gidx >= 0) {
            const int32_t owner = (int32_t)fdiv((uint32_t)gidx, a.div_cap);
            if (owner != a.me) atomicAdd(&s_cnt[owner], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < a.Kg) {
        int32_t off = 0;                                   // lists are owner-major: offset of owner j = sum of counts before it
        for (int j = 0; j < (int)threadIdx.x; j++) off += a.counts[j];
        s_base[threadIdx.x] = off + (s_cnt[threadIdx.x] ? atomicAdd(a.cursor + threadIdx.x, s_cnt[threadIdx.x]) : 0);
        s_cnt[threadIdx.x] = 0;
    }
    __syncthreads();
    for (int32_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
        const int32_t gidx = a.slot[r];
        const int32_t id = g.sampled_ids[r];
        const float* src = nullptr;
        if (gidx >= 0) {
            const uint32_t owner = fdiv((uint32_t)gidx, a.div_cap);
            const uint32_t fidx = (uint32_t)gidx - owner * (uint32_t)g.cache_capacity;
            if ((int32_t)owner == a.me) {
                const float* chunk = g.shard_tab[owner * (uint32_t)g.nchunks + (fidx >> g.chunk_shift)];
                src = chunk + (int64_t)(fidx & ((1u << g.chunk_shift) - 1u)) * (g.shard_pitch > 0 ? g.shard_pitch : g.F);
            } else {
                const int32_t k = s_base[owner] + atomicAdd(&s_cnt[owner], 1);
                a.req_row[k] = (int32_t)fidx;
                a.req_dst[k] = r;
            }
        } else if (id >= 0 && g.table) {
            src = g.table + (int64_t)(id % g.total_num_nodes) * (g.table_pitch > 0 ? g.table_pitch : g.F);
        }
        g.row_ptr[r] = src;
    }
}
// owner side: rows list[0..n) of this GPU's shard -> out[n x F]; requester side: rows[k] -> dst[req_dst[k]]
template <typename VT, bool SCATTER>
__global__ __launch_bounds__(kBlock) void k_exch_rows(const float* const* __restrict__ shard_chunks, int32_t chunk_shift,
                                                      const int32_t* __restrict__ list, int32_t n, int32_t F, int32_t shard_pitch,
                                                      const float* __restrict__ in, float* __restrict__ out, FastDiv div_c,
                                                      int32_t out_rows)
{
    constexpr int VEC = sizeof(VT) / 4;
    const int32_t C = F / VEC;
    const int64_t total = (int64_t)n * C, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
        const uint32_t k = fdiv((uint32_t)q, div_c), ch = (uint32_t)q - k * (uint32_t)C;
        const int32_t row = list[k];
        if (SCATTER) {
            if (out_rows > 0 && row >= out_rows) continue; // never write past the buffer
            const VT v = __builtin_nontemporal_load(reinterpret_cast<const VT*>(in + (int64_t)k * F) + ch);
            __builtin_nontemporal_store(v, reinterpret_cast<VT*>(out + (int64_t)row * F) + ch);
        } else {
            const float* src = shard_chunks[row >> chunk_shift] + (int64_t)(row & ((1 << chunk_shift) - 1)) * shard_pitch;
            const VT v = __builtin_nontemporal_load(reinterpret_cast<const VT*>(src) + ch);
            __builtin_nontemporal_store(v, reinterpret_cast<VT*>(out + (int64_t)k * F) + ch);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: launch wrappers
// ------------------------------------------------------------------------------------------------
void launch_find_feat(hipStream_t s, const int32_t* sampled_ids, int32_t* cache_offset, const int32_t* nc,
                      int32_t op_id, const int32_t* feat_map, int32_t bound)
{
    const int l = (op_id - 1) / 2;
    LEGION_AUDIT_LAUNCH(s, "k_find_feat", LEGION_AW(cache_offset), LEGION_AL(sampled_ids), LEGION_AL(nc), LEGION_AL(feat_map));
    k_find_feat<<<grid_for(bound, kBlock), kBlock, 0, s>>>(sampled_ids, cache_offset, nc, legion_idx_level_offset(l), legion_idx_level_size(l), feat_map);
    HIP_CHECK_LAST();
}

void launch_find_topo(hipStream_t s, const int32_t* input_ids, int8_t* part_index, int32_t* part_offset,
                      int32_t batch_size, const int8_t* topo_owner, const int32_t* topo_row)
{
    if (batch_size <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_find_topo", LEGION_AW(part_index), LEGION_AW(part_offset), LEGION_AL(input_ids), LEGION_AL(topo_owner), LEGION_AL(topo_row));
    k_find_topo<<<grid_for(batch_size, kBlock), kBlock, 0, s>>>(input_ids, part_index, part_offset, batch_size, topo_owner, topo_row);
    HIP_CHECK_LAST();
}

void launch_gather(hipStream_t s, const GatherArgs& g, int32_t rows_bound)
{
    if (g.F <= 0 || rows_bound <= 0) return;
    GatherKArgs a;
    a.g = g;
    a.div_cap = FastDiv((uint32_t)(g.cache_capacity > 0 ? g.cache_capacity : 1));
    // the backing table may be the host's or a peer's; the shard chunk TABLE and the id -> slot map are this GPU's (the chunks it names: audited where it is published)
    LEGION_AUDIT_LAUNCH(s, "k_gather", LEGION_AW(g.dst), LEGION_AW(g.row_ptr), LEGION_AW(g.rows_seen), LEGION_AW(g.hit_stats), LEGION_AL(g.sampled_ids), LEGION_AL(g.nc), LEGION_AL(g.feat_map), LEGION_AL(g.shard_tab), LEGION_AR(g.table));
    const bool vec4 = rows_are_vec4(g.F, g.table, g.dst);
    const int C = vec4 ? g.F / 4 : g.F;
    const int lanes = C;
    if ((int64_t)rows_bound * lanes >= (1ll << 31)) { LEGION_ARG_ERROR("get_feature_kernel: rows*F exceeds 2^31 work items"); return; }
    a.div_c = FastDiv((uint32_t)C);
    // Tuned on MI355X (profiles/r01_gather_sweep.md): non-temporal loads and stores (rows are read once and
    // written once: keep them out of L2/MALL).
    // One 16-byte chunk per lane and iteration.  Best measured with 2-3 iterations per lane: fewer workgroups
    // run long serial loops, more leave most of the grid empty (profiles/r01_gather_sweep.md).  Sized from est_rows
    // (launch.h); without a report of an earlier launch: the bound, at most 512 workgroups per CU.
    int grid;
    // cached configurations: FindFeat + source selection run inside the gather (k_gather_lookup: one probe per row and wave, two work
    // items per lane).  A batch whose hit rate is sampled (every 500th) and a backing table in host memory take the lookup pass
    // (k_row_ptrs in front of k_gather): it counts every row exactly once / keeps the PCIe rows at full width.
    bool fused = false;
    if (g.row_ptr && !g.row_ptr_ready) {
        fused = !g.hit_stats && !g.table_on_host;
        if (!fused) {
            k_row_ptrs<<<grid_for(est_rows(g.rows_hint, rows_bound), kBlock * 4, 64), kBlock, 0, s>>>(a);
            HIP_CHECK_LAST();
        }
    }
    if (g.rows_hint > 0) {
        // (re-swept in round 2, profiles/r02_gather_grid_sweep.md: 1-4 iterations per lane all land within the run-to-run spread)
        grid = grid_for(est_rows(g.rows_hint, rows_bound) * lanes, kBlock * (g.table_on_host ? 1 : 3), 8192); // rows over PCIe: latency-bound, maximise lanes in flight
    } else {
        grid = grid_for((int64_t)rows_bound * lanes, kBlock, 512);
    }
    if (fused) { if (vec4) k_gather_lookup<v4f, 2><<<grid, kBlock, 0, s>>>(a); else k_gather_lookup<float, 2><<<grid, kBlock, 0, s>>>(a); }
    else if (vec4) k_gather<v4f, 1, 2><<<grid, kBlock, 0, s>>>(a);
    else k_gather<float, 1, 2><<<grid, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
}

// The grid rule of k_gather_edges (tests/test_gpu_edge_features.py restates it to size its several-trips case): one workgroup per
// kBlock * kEdgeGatherU (edge, chunk) items of the hop's static bound, at most kEdgeGatherBlocksPerCu per compute unit -- 8 workgroups of 256
// threads are what a CU holds, so the grid is resident at once and every lane loops over the rest.
constexpr int kEdgeGatherU = 2, kEdgeGatherBlocksPerCu = 8;
void launch_gather_edges(hipStream_t s, const EdgeGatherArgs& g, int32_t edges_bound)
{
    if (g.dim <= 0 || edges_bound <= 0) return;
    EdgeGatherKArgs a;
    a.g = g;
    // ids, counters and the output are the pipe's own, on this GPU; the table is the graph's copy on this physical device
    LEGION_AUDIT_LAUNCH(s, "k_gather_edges", LEGION_AW(g.out), LEGION_AL(g.edge_ids), LEGION_AL(g.ec), LEGION_AR(g.table));
    const bool vec4 = rows_are_vec4(g.dim, g.table, g.out);
    const int C = vec4 ? g.dim / 4 : g.dim;
    if ((int64_t)g.ids_cap * C >= (1ll << 31)) { LEGION_ARG_ERROR("k_gather_edges: edges * chunks per row reaches 2^31 work items"); return; }
    a.div_c = FastDiv((uint32_t)C);
    const int grid = grid_for((int64_t)std::min(edges_bound, g.ids_cap) * C, kBlock * kEdgeGatherU, kEdgeGatherBlocksPerCu);
    if (vec4) k_gather_edges<v4f, kEdgeGatherU><<<grid, kBlock, 0, s>>>(a);
    else k_gather_edges<float, kEdgeGatherU><<<grid, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
}

void launch_gather_sum(hipStream_t s, const GatherArgs& g, const int32_t* cand, int32_t cand_cap, const int32_t* ec, int32_t hops,
                       int32_t f, int32_t runs_bound, const float* wdraw)
{
    if (g.F <= 0 || runs_bound <= 0 || f <= 0) return;
    GatherSumArgs a;
    a.g = g;
    a.g.row_ptr = nullptr;
    a.div_cap = FastDiv((uint32_t)(g.cache_capacity > 0 ? g.cache_capacity : 1));
    a.cand = cand; a.cand_cap = cand_cap; a.ec = ec; a.hops = hops; a.f = f; a.wdraw = wdraw;
    // the draws (and their weights) are scratch of this GPU and the sums are written into its feature buffer; the backing table may be the host's or a peer's
    LEGION_AUDIT_LAUNCH(s, "k_gather_sum", LEGION_AW(g.dst), LEGION_AW(g.rows_seen), LEGION_AL(cand), LEGION_AL(wdraw), LEGION_AL(g.nc), LEGION_AL(ec), LEGION_AL(g.feat_map), LEGION_AL(g.shard_tab), LEGION_AR(g.table));
    const bool vec4 = rows_are_vec4(g.F, g.table, g.dst);
    const int C = vec4 ? g.F / 4 : g.F;
    if ((int64_t)runs_bound * C >= (1ll << 31)) { LEGION_ARG_ERROR("get_feature_kernel_agg: rows*F exceeds 2^31 work items"); return; }
    a.div_c = FastDiv((uint32_t)C);
    // one (run, chunk) item per lane, for the runs est_rows expects of the hop's input list
    const int grid = grid_for(est_rows(g.rows_hint, runs_bound) * C, kBlock, 8192);
    constexpr bool NT = LEGION_AGG_NT_LOADS != 0;
    auto* k = wdraw ? (vec4 ? k_gather_sum<v4f, 8, NT, true> : k_gather_sum<float, 8, NT, true>)
                    : (vec4 ? k_gather_sum<v4f, 8, NT, false> : k_gather_sum<float, 8, NT, false>);
    k<<<grid, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
}

void launch_agg_norm_weights(hipStream_t s, const AggNormArgs& a, int32_t slots_bound, int32_t edges_bound)
{
    if (slots_bound <= 0 || a.f <= 0) return;
    // every buffer is the pipe's own, on this GPU; grids from the static bounds of the hop and of the batch, loop bounds from the counters
    const int chunks = std::min<int64_t>(kMaxChunks, grid_for(slots_bound, kBlock));   // one grid for both chunked passes
    LEGION_AUDIT_LAUNCH(s, "k_agg_norm_prep", LEGION_AW(a.out_deg), LEGION_AW(a.chunk_cnt), LEGION_AL(a.cand), LEGION_AL(a.nc), LEGION_AL(a.ec));
    k_agg_norm_prep<<<chunks, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
    LEGION_AUDIT_LAUNCH(s, "k_block_out_deg", LEGION_AW(a.out_deg), LEGION_AL(a.src_off), LEGION_AL(a.ec));
    k_block_out_deg<<<grid_for(edges_bound, kBlock), kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
    LEGION_AUDIT_LAUNCH(s, "k_draw_weights", LEGION_AW(a.wdraw), LEGION_AL(a.out_deg), LEGION_AL(a.chunk_cnt), LEGION_AL(a.cand), LEGION_AL(a.src_off), LEGION_AL(a.nc), LEGION_AL(a.ec));
    k_draw_weights<<<chunks, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
}

void launch_agg_edge_weights(hipStream_t s, const AggEdgeWeightArgs& a, int32_t slots_bound)
{
    if (slots_bound <= 0 || a.f <= 0) return;
    // every buffer is the pipe's own, on this GPU; the grid from the static bound of the hop, loop bounds from the counters
    const int chunks = std::min<int64_t>(kMaxChunks, grid_for(slots_bound, kBlock));   // one grid for both passes, launch_agg_norm_weights' rule
    LEGION_AUDIT_LAUNCH(s, "k_draw_edge_weights<count>", LEGION_AW(a.chunk_cnt), LEGION_AL(a.cand), LEGION_AL(a.nc), LEGION_AL(a.ec));
    k_draw_edge_weights<true><<<chunks, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
    LEGION_AUDIT_LAUNCH(s, "k_draw_edge_weights", LEGION_AW(a.wdraw), LEGION_AL(a.chunk_cnt), LEGION_AL(a.cand), LEGION_AL(a.edge_w), LEGION_AL(a.nc), LEGION_AL(a.ec));
    k_draw_edge_weights<false><<<chunks, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
}

void launch_exchange_plan(hipStream_t s, const GatherArgs& g, int32_t me, int32_t Kg, int32_t* slot, int32_t* counts,
                          int32_t* req_row, int32_t* req_dst, int32_t rows_bound)
{
    if (rows_bound <= 0) return;
    ExchArgs a;
    a.g = g;
    a.div_cap = FastDiv((uint32_t)(g.cache_capacity > 0 ? g.cache_capacity : 1));
    a.me = me; a.Kg = Kg; a.slot = slot; a.counts = counts; a.cursor = counts + kMaxParts;
    a.req_row = req_row; a.req_dst = req_dst;
    LEGION_AUDIT_LAUNCH(s, "k_exch_count/k_exch_fill", LEGION_AW(slot), LEGION_AW(counts), LEGION_AW(req_row), LEGION_AW(req_dst), LEGION_AW(g.row_ptr), LEGION_AL(g.sampled_ids), LEGION_AL(g.nc), LEGION_AL(g.feat_map), LEGION_AL(g.shard_tab), LEGION_AR(g.table));
    HIP_CHECK(hipMemsetAsync(counts, 0, 2 * kMaxParts * sizeof(int32_t), s));
    const int grid = grid_for(est_rows(g.rows_hint, rows_bound), kBlock * 4, 64);
    k_exch_count<<<grid, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
    k_exch_fill<<<grid, kBlock, 0, s>>>(a);
    HIP_CHECK_LAST();
}
void launch_exchange_rows(hipStream_t s, bool scatter, const float* const* shard_chunks, int32_t chunk_shift, const int32_t* list,
                          int32_t n, int32_t F, int32_t shard_pitch, const float* in, float* out, int32_t out_rows)
{
    if (n <= 0 || F <= 0) return;
    if (shard_pitch <= 0) shard_pitch = F;
    const bool vec4 = rows_are_vec4(F, in, out);
    const int C = vec4 ? F / 4 : F;
    if ((int64_t)n * C >= (1ll << 31)) { LEGION_ARG_ERROR("legion_exchange: rows*F exceeds 2^31 work items"); return; }
    const FastDiv dc((uint32_t)C);
    LEGION_AUDIT_LAUNCH(s, "k_exch_rows", LEGION_AW(out), LEGION_AL(shard_chunks), LEGION_AL(list), LEGION_AL(in));
    const int grid = grid_for((int64_t)n * C, kBlock * 2, 8192);
    auto* k = scatter ? (vec4 ? k_exch_rows<v4f, true> : k_exch_rows<float, true>) : (vec4 ? k_exch_rows<v4f, false> : k_exch_rows<float, false>);
    k<<<grid, kBlock, 0, s>>>(shard_chunks, chunk_shift, list, n, F, shard_pitch, in, out, dc, out_rows);
    HIP_CHECK_LAST();
}

} // namespace legion
