// memory_pool.cpp -- host mirror of GPUMemoryPool (GPUMemoryPool.cuh:7-208): the per-batch scratch of one logical GPU, the serving modes
// it is in and the per-pipe output buffers the caller registered.
#include "internal.h"

#include <algorithm>
#include <cstring>

#include "device_mem.h"
#include "lp_exclude.h"

using namespace legion;

GPUMemoryPool::GPUMemoryPool(int32_t depth) : pipeline_depth(depth > 0 ? depth : 1), pipes(pipeline_depth) {}

// Every device scratch buffer the pool owns, in allocation order, with its size, its name, what an element of it is and how long what it holds
// means anything (include/legion_amd.h: LEGION_SCRATCH_*; DESIGN.md "What the pool's scratch may hold between launches"): pool_scratch() for
// what exists once, pool_pipe_buffers() behind it for what exists once per pipe (Pipe::own[]).  GPUMemoryPool_AllocateScratch and
// alloc_mode_buffers allocate the two tables, release_scratch frees and forgets them, GPUMemoryPool_ScratchInfo reports them and
// batch_generator_kernel audits their owner -- a buffer named here is in all of them, and a launcher asks for a pipe's buffer by its row
// (pipe_holds, launchers.cpp).  Sized from V, num_ids, max_slots and max_tiles as they are now.
//   hop:   written and read inside one GPU_Random_Sampling (k_sample, k_mark, k_write of one hop); dead once that call has returned.
//          cand is read back by callers behind the batch (GPUMemoryPool_GetCandidateBuffer), never by a later launch.
//   batch: carried from one op of a batch to a later one -- aux2[(h + 1) & 1] (the next hop's slot states, prepared by k_seed / k_write
//          while aux2[h & 1] is dead as soon as hop h has returned), agg_src_ids (the next hop's input list), row_ptr (exchange plan ->
//          local gather), cache_search_buffer / tmp_part_* (FindFeat / FindTopo answers the caller carries between two calls) and the per-pipe
//          buffers of the aggregated modes (last hop -> get_feature_kernel_agg); dead once the batch's last op has returned.
//   table: pos_map; an entry whose epoch field is greater than the running batch's means nothing.
// The buffers of the edge-id mode (GPUMemoryPool_SetEdgeIds) join the list once the pool has been in that mode, behind the others of their
// kind, and stay until the scratch is released: a pool that never saw the mode lists what it always listed.  cols (hop): k_sample's columns,
// read by k_edge_ids of the same GPU_Random_Sampling.  edge_ids / edge_w (batch, per pipe): outputs no launch reads, the caller's behind the batch.
// "Has been in the mode", once: the mode is on, or cols is there -- the one allocation every switch on makes on a pool that owns scratch and
// only release_scratch takes back.  (A pool without a device allocates nothing, so it lists the buffers exactly while the mode is on.)
static bool lists_edge_ids(const GPUMemoryPool* p) { return p->modes.edge_ids || p->cols; }
// The buffer of the edge-feature mode (GPUMemoryPool_SetEdgeFeatures) by the same rule: edge_feat (batch, per pipe), float32 [num_ids, dim], an
// output no launch reads, joins the list behind edge_w once the pool has been in the mode -- the mode is on, or the pipes hold the buffer
// (edge_feat_alloc_dim: the width they were allocated for, which only release_scratch forgets) -- at the width it is held at.
static int32_t listed_edge_feat_dim(const GPUMemoryPool* p) { return p->modes.edge_feat_dim > 0 ? p->modes.edge_feat_dim : p->edge_feat_alloc_dim; }
// The buffers of target-edge exclusion (GPUMemoryPool_SetLpExclude) by the same rule again: lp_pairs (batch, per pipe), uint64[cap], written by
// k_lp_pairs behind k_seed and read by k_lp_edge_keep behind the last hop; edge_keep (uint8[num_ids]) and lp_excluded (int32[8]), outputs no
// launch reads.  They join the list behind edge_feat once the pool has been in the mode -- the mode is on, or the pipes hold the table
// (lp_alloc_cap: the capacity it was allocated for, which only release_scratch forgets) -- at the capacity it is held at.
static int32_t listed_lp_cap(const GPUMemoryPool* p) { return p->modes.lp_exclude > 0 ? lp_pair_cap(p->modes.lp_exclude) : p->lp_alloc_cap; }
std::vector<ScratchBuffer> legion::pool_scratch(GPUMemoryPool* p)
{
    const size_t ids = (size_t)p->num_ids, slots = (size_t)p->max_slots, tiles = (size_t)p->max_tiles + 1;
    constexpr int32_t I = sizeof(int32_t), hop = LEGION_SCRATCH_HOP, batch = LEGION_SCRATCH_BATCH;
    std::vector<ScratchBuffer> all = {{(void**)&p->pos_map, (size_t)p->V * sizeof(pos_t), "pos_map", LEGION_SCRATCH_TABLE_ENTRY, sizeof(pos_t), LEGION_SCRATCH_TABLE},
            {(void**)&p->cand, slots * sizeof(int32_t), "cand", LEGION_SCRATCH_ID, I, hop},
            {(void**)&p->aux2[0], slots * sizeof(int32_t), "aux2[0]", LEGION_SCRATCH_SLOT_STATE, I, batch},
            {(void**)&p->aux2[1], slots * sizeof(int32_t), "aux2[1]", LEGION_SCRATCH_SLOT_STATE, I, batch},
            {(void**)&p->tile_edge, tiles * sizeof(int32_t), "tile_edge", LEGION_SCRATCH_COUNT, I, hop},
            {(void**)&p->tile_node, tiles * sizeof(int32_t), "tile_node", LEGION_SCRATCH_COUNT, I, hop},
            {(void**)&p->tile_pre, tiles * sizeof(int2), "tile_pre", LEGION_SCRATCH_COUNT_PAIR, sizeof(int2), hop},
            {(void**)&p->chunk_tot, (size_t)kMaxChunks * sizeof(int2), "chunk_tot", LEGION_SCRATCH_COUNT_PAIR, sizeof(int2), hop},
            {(void**)&p->hop_state, sizeof(HopState), "hop_state", LEGION_SCRATCH_COUNT, I, hop},
            {(void**)&p->cache_search_buffer, ids * sizeof(int32_t), "cache_search_buffer", LEGION_SCRATCH_ID, I, batch},
            {(void**)&p->row_ptr, ids * sizeof(float*), "row_ptr", LEGION_SCRATCH_DEVICE_POINTER, sizeof(float*), batch},
            {(void**)&p->agg_src_ids, ids * sizeof(int32_t), "agg_src_ids", LEGION_SCRATCH_ID, I, batch},
            {(void**)&p->tmp_part_ind, ids, "tmp_part_ind", LEGION_SCRATCH_ID, 1, batch},
            {(void**)&p->tmp_part_off, ids * sizeof(int32_t), "tmp_part_off", LEGION_SCRATCH_ID, I, batch}};
    if (lists_edge_ids(p)) all.push_back({(void**)&p->cols, slots * sizeof(int32_t), "cols", LEGION_SCRATCH_COUNT, I, hop});
    return all;
}
// The buffers the pool owns once per pipe, named once in the same way: which Pipe::own[], bytes per pipe, whether the modes want it now, whether
// it is listed, and its description.  The draw buffers of the aggregated last hop (cand_pipe) and, for the normalised sums, agg_out_deg /
// agg_wdraw / agg_chunk_cnt; the edge-weighted sums want the last two of them.  A new per-pipe buffer is one row here (and its PipeBuf name).
std::array<PipeBuffer, GPUMemoryPool::kPipeBufs> legion::pool_pipe_buffers(const GPUMemoryPool* p)
{
    using Pool = GPUMemoryPool;
    const bool agg = p->modes.agg_last_hop, norm = agg && p->modes.agg_norm, eid = p->modes.edge_ids, eid_listed = lists_edge_ids(p);
    const bool wdraw = norm || (agg && p->modes.agg_edge_weight);   // the edge-weighted sums rank their draws the same way, without the degrees
    const size_t ids = (size_t)p->num_ids, slots = (size_t)p->max_slots;
    const bool lpx = p->modes.lp_exclude > 0, lpx_listed = listed_lp_cap(p) > 0;
    constexpr int32_t I = sizeof(int32_t), batch = LEGION_SCRATCH_BATCH;
    return {{{Pool::kCandPipe, slots * sizeof(int32_t), agg, true, "cand_pipe", LEGION_SCRATCH_ID, I, batch},
             {Pool::kAggOutDeg, ids * sizeof(int32_t), norm, true, "agg_out_deg", LEGION_SCRATCH_COUNT, I, batch},
             {Pool::kAggWdraw, slots * sizeof(float), wdraw, true, "agg_wdraw", LEGION_SCRATCH_FLOAT, sizeof(float), batch},
             {Pool::kAggChunkCnt, (size_t)kMaxChunks * sizeof(int32_t), wdraw, true, "agg_chunk_cnt", LEGION_SCRATCH_COUNT, I, batch},
             // an edge id is one 8-byte word no kernel reads back: any bytes are safe in it, a pair of counts is what the poison's kinds offer
             {Pool::kEdgeIds, ids * sizeof(int64_t), eid, eid_listed, "edge_ids", LEGION_SCRATCH_COUNT_PAIR, sizeof(int64_t), batch},
             {Pool::kEdgeW, ids * sizeof(float), eid, eid_listed, "edge_w", LEGION_SCRATCH_FLOAT, sizeof(float), batch},
             {Pool::kEdgeFeat, ids * (size_t)listed_edge_feat_dim(p) * sizeof(float), p->modes.edge_feat_dim > 0, listed_edge_feat_dim(p) > 0, "edge_feat", LEGION_SCRATCH_FLOAT, sizeof(float), batch},
             // a table slot is one 8-byte word k_lp_pairs overwrites before anything reads it, a keep byte and a count are outputs: any bytes are safe in all three
             {Pool::kLpPairs, (size_t)listed_lp_cap(p) * sizeof(uint64_t), lpx, lpx_listed, "lp_pairs", LEGION_SCRATCH_COUNT_PAIR, sizeof(uint64_t), batch},
             {Pool::kEdgeKeep, ids, lpx, lpx_listed, "edge_keep", LEGION_SCRATCH_ID, 1, batch},
             {Pool::kLpExcluded, (size_t)kLpExcludedWords * sizeof(int32_t), lpx, lpx_listed, "lp_excluded", LEGION_SCRATCH_COUNT, I, batch}}};
}
// on the current device: what the pool's modes want and is missing is allocated, what is there stays
static void alloc_mode_buffers(GPUMemoryPool* p)
{
    if (!p->owns_scratch) return;
    if (p->modes.edge_feat_dim > 0 && p->edge_feat_alloc_dim != p->modes.edge_feat_dim) {   // another row width: the pipes' buffers are reallocated below
        if (p->edge_feat_alloc_dim) HIP_CHECK(hipDeviceSynchronize());                      // a gather into the old ones may still be in flight
        for (GPUMemoryPool::Pipe& pipe : p->pipes) { free_and_null(pipe.own[GPUMemoryPool::kEdgeFeat]); pipe.edge_feat_filled = false; }
        p->edge_feat_alloc_dim = p->modes.edge_feat_dim;
        p->edge_feat_gen++;
    }
    if (p->modes.lp_exclude > 0 && p->lp_alloc_cap != lp_pair_cap(p->modes.lp_exclude)) {   // another table capacity: the pipes' tables are reallocated below
        if (p->lp_alloc_cap) HIP_CHECK(hipDeviceSynchronize());                             // a marking pass over the old ones may still be in flight
        for (GPUMemoryPool::Pipe& pipe : p->pipes) { free_and_null(pipe.own[GPUMemoryPool::kLpPairs]); pipe.lp_marked = false; }
        p->lp_alloc_cap = lp_pair_cap(p->modes.lp_exclude);
        p->lp_gen++;
    }
    for (const PipeBuffer& b : pool_pipe_buffers(p))
        for (GPUMemoryPool::Pipe& pipe : p->pipes)
            if (b.wanted && !pipe.own[b.which]) HIP_CHECK(hipMalloc(&pipe.own[b.which], b.bytes));
    if (p->modes.edge_ids && !p->cols) HIP_CHECK(hipMalloc(&p->cols, (size_t)p->max_slots * sizeof(int32_t)));
}

// ---- the releases: each kind of scratch has one, and GPUMemoryPool_Finalize calls them all ----
static void release_scratch(GPUMemoryPool* p)
{
    for (const ScratchBuffer& b : pool_scratch(p)) free_and_null(*b.slot);
    for (const PipeBuffer& b : pool_pipe_buffers(p))   // every row, listed or not: with cols null again the pool lists the edge-id rows only while the mode is on
        for (GPUMemoryPool::Pipe& pipe : p->pipes) { free_and_null(pipe.own[b.which]); pipe.edge_w_filled = pipe.edge_feat_filled = pipe.lp_marked = false; }
    p->edge_feat_alloc_dim = 0;
    p->edge_feat_gen++;
    p->lp_alloc_cap = 0;
    p->lp_gen++;
}
static void release_ctl(GPUMemoryPool* p) { free_and_null(p->ctl); }
static void release_rows_seen(GPUMemoryPool* p)
{
    if (p->rows_seen) (void)hipHostFree(p->rows_seen);
    p->rows_seen = p->rows_seen_dev = nullptr;
}
// the shuffled copy of the training list (GPUMemoryPool_BeginRound allocates it on first use)
static void release_shuffle(GPUMemoryPool* p)
{
    free_and_null(p->shuf_ids);
    free_and_null(p->shuf_labels);
    p->shuf_cap = p->shuf_n = 0; p->shuf_src = nullptr; p->shuf_valid = false;
}

bool legion::pool_apply_modes(GPUMemoryPool* p, const ServeModes& wanted, const char* who)
{
    const std::string name(who);
    if (!p) { LEGION_ARG_ERROR((name + ": null pool").c_str()); return false; }
    if (p->capturing) { LEGION_ARG_ERROR((name + ": the pool is being captured").c_str()); return false; }
    if (wanted.agg_norm != 0 && wanted.agg_norm != 1) { LEGION_ARG_ERROR("GPUMemoryPool_SetAggNorm: unknown norm (0 = none, 1 = out-degree rsqrt)"); return false; }
    if (wanted.agg_norm && !wanted.agg_last_hop && wanted.agg_norm != p->modes.agg_norm) { LEGION_ARG_ERROR("GPUMemoryPool_SetAggNorm: the pool does not aggregate the last hop (GPUMemoryPool_SetAggLastHop first): only neighbour sums are normalised"); return false; }
    if (wanted.sampling != kSamplingReplace && wanted.sampling != kSamplingDistinct && wanted.sampling != kSamplingWeighted) { LEGION_ARG_ERROR("GPUMemoryPool_SetSampling: unknown sampling kind (0 = replace, 1 = distinct, 2 = weighted)"); return false; }
    if (wanted.lp_draw < 0) { LEGION_ARG_ERROR("GPUMemoryPool_SetLpDraw: negative triples per batch (0 = off, k > 0 = batches of 3 k)"); return false; }
    // the alias rule draws a column and may keep the column's ALIAS neighbour, whose id the table holds and whose column it does not (open)
    if (wanted.edge_ids && !sample_variant_exists(RowSource::Whole, draw_rule_of(wanted), true)) { LEGION_ARG_ERROR((name + ": edge ids (GPUMemoryPool_SetEdgeIds) cannot be handed over under weighted sampling with replacement (GPUMemoryPool_SetSampling(pool, 2) without GPUMemoryPool_SetWeightedDistinct): the alias table holds the alias neighbour's id, not its column").c_str()); return false; }
    // the edge-weighted sums are a flag on top of the aggregated mode (remembered while it is off, as the norm is) that reads the edge-id mode's edge_w
    if (wanted.agg_edge_weight && !wanted.agg_last_hop && !p->modes.agg_edge_weight) { LEGION_ARG_ERROR((name + ": edge-weighted sums (GPUMemoryPool_SetAggEdgeWeight) on a pool that does not aggregate the last hop (GPUMemoryPool_SetAggLastHop first): only neighbour sums are scaled").c_str()); return false; }
    if (wanted.agg_edge_weight && !wanted.edge_ids) { LEGION_ARG_ERROR((name + ": edge-weighted sums (GPUMemoryPool_SetAggEdgeWeight) need edge ids (GPUMemoryPool_SetEdgeIds first, and not off while the flag is on): the weight of a draw is the edge_w that mode hands over").c_str()); return false; }
    if (wanted.agg_edge_weight && wanted.agg_norm) { LEGION_ARG_ERROR((name + ": edge-weighted sums (GPUMemoryPool_SetAggEdgeWeight) together with a norm (GPUMemoryPool_SetAggNorm): GraphConv(norm='both', edge_weight=) rounds twice per product and has no kernel in this build").c_str()); return false; }
    // edge features are gathered by the ids the edge-id mode leaves: refused in the name of whichever setter comes second
    if (wanted.edge_feat_dim < 0) { LEGION_ARG_ERROR((name + ": negative edge-feature width (0 = off, dim > 0 = float32 [edges, dim] per batch)").c_str()); return false; }
    if (wanted.edge_feat_dim > 0 && !wanted.edge_ids) { LEGION_ARG_ERROR((name + ": edge features (GPUMemoryPool_SetEdgeFeatures) need edge ids (GPUMemoryPool_SetEdgeIds first, and not off while the mode is on): a row is gathered by the id that mode hands over").c_str()); return false; }
    if (wanted.edge_feat_dim > 0) {
        int64_t bytes = 0;
        if (__builtin_mul_overflow((int64_t)p->num_ids * (int64_t)sizeof(float), (int64_t)wanted.edge_feat_dim, &bytes)) { LEGION_ARG_ERROR((name + ": edge features (GPUMemoryPool_SetEdgeFeatures): the size of the per-pipe buffer, NumIds * dim * 4 bytes, overflows").c_str()); return false; }
        if ((int64_t)p->num_ids * edge_gather_chunks(wanted.edge_feat_dim) >= (1ll << 31)) { LEGION_ARG_ERROR((name + ": edge features (GPUMemoryPool_SetEdgeFeatures): NumIds * chunks per row reaches 2^31 work items (a row is gathered in 16-byte chunks where dim % 4 == 0, else float by float)").c_str()); return false; }
    }
    // target-edge exclusion reads the batch's own src and pos thirds: refused in the name of whichever setter comes second
    if (wanted.lp_exclude < 0) { LEGION_ARG_ERROR((name + ": negative triples per batch for target-edge exclusion (GPUMemoryPool_SetLpExclude: 0 = off, k > 0 = batches of 3 k)").c_str()); return false; }
    if (wanted.lp_exclude > kLpMaxTriples) { LEGION_ARG_ERROR((name + ": target-edge exclusion (GPUMemoryPool_SetLpExclude): more than 2^28 triples per batch exceed the pair table's 32-bit slots").c_str()); return false; }
    if (wanted.lp_exclude > 0 && wanted.lp_draw > 0 && wanted.lp_exclude != wanted.lp_draw) { LEGION_ARG_ERROR((name + ": target-edge exclusion (GPUMemoryPool_SetLpExclude) and drawn link-prediction thirds (GPUMemoryPool_SetLpDraw) with different triples per batch: both describe the same batch of 3 k seeds").c_str()); return false; }
    // the neighbour sums would contain the excluded draws (open: a zero weight per excluded draw)
    if (wanted.lp_exclude > 0 && wanted.agg_last_hop) { LEGION_ARG_ERROR((name + ": target-edge exclusion (GPUMemoryPool_SetLpExclude) together with the aggregated last hop (GPUMemoryPool_SetAggLastHop): the neighbour sums would contain the excluded draws").c_str()); return false; }
    if (wanted.lp_draw > 0 && !p->lp_graph) { LEGION_ARG_ERROR("GPUMemoryPool_SetLpDraw: null graph: the positives are neighbours read from it"); return false; }
    if (wanted.seed != p->modes.seed) p->shuf_valid = false;   // the copy holds another seed's permutation (off and on again under one seed keeps it)
    if (wanted.lp_draw != p->modes.lp_draw) p->shuf_valid = false;   // ... or was shuffled by seeds, not by triples of this k
    if (wanted.seeded != p->modes.seeded || wanted.seed != p->modes.seed) p->ctl_synced = false;   // ctl holds the other state's draw word: a batch graph must reset the cursor
    p->modes = wanted;
    alloc_mode_buffers(p);
    return true;
}

extern "C" {

GPUMemoryPool* NewGPUMemoryPool(int32_t pipeline_depth) { return new GPUMemoryPool(pipeline_depth); }

// Server.cu:184-196 (num_ids_) and :216-231 (scratch), sized for H hops
void GPUMemoryPool_AllocateScratch(GPUMemoryPool* p, int32_t total_num_nodes, int32_t batch_size,
                                   const int32_t* fanout, int32_t hops)
{
    if (!p || hops < 1 || hops > LEGION_MAX_HOPS || batch_size < 1 || total_num_nodes < 1) { LEGION_ARG_ERROR("GPUMemoryPool_AllocateScratch: bad arguments"); return; }
    if (p->owns_scratch) GPUMemoryPool_Finalize(p); // re-sizing an initialised pool: release the old scratch first
    p->V = total_num_nodes; p->batch_size = batch_size; p->hops = hops;
    int64_t ids = batch_size, cur = batch_size, max_slots = 0;
    p->level_bound[0] = batch_size;
    for (int h = 0; h < hops; h++) {
        p->fanout[h] = fanout[h];
        cur *= fanout[h];
        if (cur > max_slots) max_slots = cur;
        ids += cur;
        if (ids >= (1ll << 31)) { LEGION_ARG_ERROR("GPUMemoryPool_AllocateScratch: batch*fanouts exceeds int32"); return; }
        if (cur >= (1ll << 30)) { LEGION_ARG_ERROR("GPUMemoryPool_AllocateScratch: a hop of 2^30 or more slots exceeds the slot-state encoding"); return; }
        p->level_bound[h + 1] = (int32_t)cur;
    }
    p->num_ids = (int32_t)ids;
    p->max_slots = (int32_t)max_slots;
    p->max_tiles = (int32_t)sampler_max_tiles(max_slots);   // the narrow hops run smaller tiles (internal.h)
    p->owns_scratch = true;
    for (const ScratchBuffer& b : pool_scratch(p)) HIP_CHECK(hipMalloc(b.slot, b.bytes));
    HIP_CHECK(hipMemset(p->pos_map, 0xFF, (size_t)total_num_nodes * sizeof(pos_t)));
    p->batch_serial = 0;
    HIP_CHECK(hipMalloc(&p->ctl, sizeof(BatchCtl)));
    { const BatchCtl c{0, kEpochTop}; HIP_CHECK(hipMemcpy(p->ctl, &c, sizeof(c), hipMemcpyHostToDevice)); }
    p->ctl_synced = false;
    HIP_CHECK(hipHostMalloc((void**)&p->rows_seen, kRowsSeenWords * sizeof(int32_t), hipHostMallocMapped));
    memset(p->rows_seen, 0, kRowsSeenWords * sizeof(int32_t));
    HIP_CHECK(hipHostGetDevicePointer((void**)&p->rows_seen_dev, p->rows_seen, 0));
    alloc_mode_buffers(p);
    HIP_CHECK(hipDeviceSynchronize());
}
int32_t GPUMemoryPool_NumIds(const GPUMemoryPool* p) { return p->num_ids; }

// The mode setters: the pool's modes with one field changed, through pool_apply_modes (internal.h: what is refused, what is
// allocated).  Call them under the device the pool's scratch lives on.  Aggregated last hop: INTEGRATION.md "Aggregated last hop";
// norm: 0 = plain sums, 1 = out-degree rsqrt ("Normalised sums"); distinct draws: "Sampling without replacement", nothing is allocated;
// seed: "Seeded sampling", seed 0 is a seed like any other, nothing is allocated here (GPUMemoryPool_BeginRound fills the shuffled copy);
// drawn link-prediction thirds: "Drawn link-prediction thirds", k triples per batch (0 = off) and the graph the positives are read from,
// which the pool keeps (and forgets when the mode is switched off); nothing is allocated.
static ServeModes modes_of(const GPUMemoryPool* p) { return p ? p->modes : ServeModes(); }
void GPUMemoryPool_SetAggLastHop(GPUMemoryPool* p, int on) { ServeModes m = modes_of(p); m.agg_last_hop = on != 0; pool_apply_modes(p, m, "GPUMemoryPool_SetAggLastHop"); }
void GPUMemoryPool_SetAggNorm(GPUMemoryPool* p, int norm) { ServeModes m = modes_of(p); m.agg_norm = norm; pool_apply_modes(p, m, "GPUMemoryPool_SetAggNorm"); }
void GPUMemoryPool_SetSampleDistinct(GPUMemoryPool* p, int on) { ServeModes m = modes_of(p); m.sampling = on != 0; pool_apply_modes(p, m, "GPUMemoryPool_SetSampleDistinct"); }
// the sampling kind as the enumeration it is: 0 = replace, 1 = distinct (what SetSampleDistinct(1) sets), 2 = weighted ("Weighted sampling":
// nothing is allocated here, the alias table belongs to the graph: GPUGraphStorage_SetEdgeWeights)
void GPUMemoryPool_SetSampling(GPUMemoryPool* p, int kind) { ServeModes m = modes_of(p); m.sampling = kind; pool_apply_modes(p, m, "GPUMemoryPool_SetSampling"); }
int GPUMemoryPool_GetSampling(const GPUMemoryPool* p) { return p ? p->modes.sampling : 0; }
// weighted sampling without replacement ("Weighted sampling without replacement"): a flag on top of the weighted kind, remembered across
// kinds and acting only while the kind is 2; nothing is allocated here, the weights belong to the graph (GPUGraphStorage_RetainEdgeWeights)
void GPUMemoryPool_SetWeightedDistinct(GPUMemoryPool* p, int on) { ServeModes m = modes_of(p); m.weighted_distinct = on != 0; pool_apply_modes(p, m, "GPUMemoryPool_SetWeightedDistinct"); }
int GPUMemoryPool_GetWeightedDistinct(const GPUMemoryPool* p) { return p && p->modes.weighted_distinct ? 1 : 0; }
// shared-key sampling ("Shared-key sampling"): a flag on top of the distinct kind, remembered across kinds and acting only while the kind
// is 1; nothing is allocated.  An unseeded pool draws under word 0: deterministic, the same node keys in every batch
void GPUMemoryPool_SetSharedDraws(GPUMemoryPool* p, int on) { ServeModes m = modes_of(p); m.shared_draws = on != 0; pool_apply_modes(p, m, "GPUMemoryPool_SetSharedDraws"); }
int GPUMemoryPool_GetSharedDraws(const GPUMemoryPool* p) { return p && p->modes.shared_draws ? 1 : 0; }
// edge ids ("Edge ids"): every batch additionally leaves each COO edge's position in the whole CSR, and its weight where the graph retains them,
// in per-pipe buffers of the pool.  Allocates cols (max_slots words) and edge_ids / edge_w (num_ids elements per pipe) on the first switch on
void GPUMemoryPool_SetEdgeIds(GPUMemoryPool* p, int on) { ServeModes m = modes_of(p); m.edge_ids = on != 0; pool_apply_modes(p, m, "GPUMemoryPool_SetEdgeIds"); }
int GPUMemoryPool_GetEdgeIds(const GPUMemoryPool* p) { return p && p->modes.edge_ids ? 1 : 0; }
// edge-weighted sums ("Edge-weighted sums"): a flag on top of the aggregated last hop, only with edge ids on and without a norm; remembered while
// the aggregated mode is off.  Allocates agg_wdraw / agg_chunk_cnt per pipe where they are missing (no agg_out_deg: the degrees are the norm's)
void GPUMemoryPool_SetAggEdgeWeight(GPUMemoryPool* p, int on) { ServeModes m = modes_of(p); m.agg_edge_weight = on != 0; pool_apply_modes(p, m, "GPUMemoryPool_SetAggEdgeWeight"); }
int GPUMemoryPool_GetAggEdgeWeight(const GPUMemoryPool* p) { return p && p->modes.agg_edge_weight ? 1 : 0; }
// the current pipe's buffers as the last batch under the mode left them: int64 / float32 [legion_batch_edges(ec, H)], in the order and at the
// offsets of the COO.  Null before the mode was set; the weights are null unless that batch ran over a graph that retains them
int64_t* GPUMemoryPool_GetEdgeIdBuffer(const GPUMemoryPool* p)
{
    if (!p) { LEGION_ARG_ERROR("GPUMemoryPool_GetEdgeIdBuffer: null pool"); return nullptr; }
    return p->pipe().buf<int64_t>(GPUMemoryPool::kEdgeIds);
}
float* GPUMemoryPool_GetEdgeWeightBuffer(const GPUMemoryPool* p)
{
    if (!p) { LEGION_ARG_ERROR("GPUMemoryPool_GetEdgeWeightBuffer: null pool"); return nullptr; }
    return p->pipe().edge_w_filled ? p->pipe().buf<float>(GPUMemoryPool::kEdgeW) : nullptr;
}
// edge features ("Edge features"): dim > 0 = behind get_edge_feature_kernel(_all) the pipe holds edge_feat[e, :] = X[edge_ids[e], :], X the graph's
// table (GPUGraphStorage_SetEdgeFeatures); 0 = off.  Only with edge ids.  Allocates edge_feat (num_ids * dim floats per pipe); another dim reallocates it
void GPUMemoryPool_SetEdgeFeatures(GPUMemoryPool* p, int32_t dim) { ServeModes m = modes_of(p); m.edge_feat_dim = dim; pool_apply_modes(p, m, "GPUMemoryPool_SetEdgeFeatures"); }
int32_t GPUMemoryPool_GetEdgeFeatures(const GPUMemoryPool* p) { return p ? p->modes.edge_feat_dim : 0; }
// the current pipe's buffer, float32 [legion_batch_edges(ec, H), dim] in the order of the COO; null unless the pipe's last batch was gathered
float* GPUMemoryPool_GetEdgeFeatureBuffer(const GPUMemoryPool* p)
{
    if (!p) { LEGION_ARG_ERROR("GPUMemoryPool_GetEdgeFeatureBuffer: null pool"); return nullptr; }
    return p->pipe().edge_feat_filled ? p->pipe().buf<float>(GPUMemoryPool::kEdgeFeat) : nullptr;
}
void GPUMemoryPool_SetSampleSeed(GPUMemoryPool* p, int on, uint32_t seed)
{
    ServeModes m = modes_of(p);
    m.seeded = on != 0; m.seed = seed;
    if (pool_apply_modes(p, m, "GPUMemoryPool_SetSampleSeed")) p->ctl_synced = false;   // this call always has the next graph replay reset its cursor
}
void GPUMemoryPool_SetLpDraw(GPUMemoryPool* p, int32_t triples_per_batch, GPUGraphStorage* graph)
{
    ServeModes m = modes_of(p);
    m.lp_draw = triples_per_batch;
    GPUGraphStorage* const before = p ? p->lp_graph : nullptr;
    if (p && !p->capturing) p->lp_graph = triples_per_batch > 0 ? graph : nullptr;
    if (!pool_apply_modes(p, m, "GPUMemoryPool_SetLpDraw") && p && !p->capturing) p->lp_graph = before;
}
int32_t GPUMemoryPool_GetLpDraw(const GPUMemoryPool* p) { return p ? p->modes.lp_draw : 0; }
// target-edge exclusion ("Target-edge exclusion"): k > 0 = a training batch of 3 k seeds leaves edge_keep[e] = 0 for every COO edge that joins a
// target pair {ids[i], ids[k + i]}, 1 for every other, and the zeros per hop in lp_excluded; 0 = off.  Allocates lp_pairs (uint64[cap]), edge_keep
// (num_ids bytes) and lp_excluded (int32[8]) per pipe on the first switch on; a k of another table capacity reallocates lp_pairs
void GPUMemoryPool_SetLpExclude(GPUMemoryPool* p, int32_t triples_per_batch) { ServeModes m = modes_of(p); m.lp_exclude = triples_per_batch; pool_apply_modes(p, m, "GPUMemoryPool_SetLpExclude"); }
int32_t GPUMemoryPool_GetLpExclude(const GPUMemoryPool* p) { return p ? p->modes.lp_exclude : 0; }
// the current pipe's buffers, uint8 [legion_batch_edges(ec, H)] in the order of the COO and int32[8]; null unless the pipe's last batch ran the marking launch
uint8_t* GPUMemoryPool_GetEdgeKeepBuffer(const GPUMemoryPool* p)
{
    if (!p) { LEGION_ARG_ERROR("GPUMemoryPool_GetEdgeKeepBuffer: null pool"); return nullptr; }
    return p->pipe().lp_marked ? p->pipe().buf<uint8_t>(GPUMemoryPool::kEdgeKeep) : nullptr;
}
int32_t* GPUMemoryPool_GetLpExcludedBuffer(const GPUMemoryPool* p)
{
    if (!p) { LEGION_ARG_ERROR("GPUMemoryPool_GetLpExcludedBuffer: null pool"); return nullptr; }
    return p->pipe().lp_marked ? p->pipe().buf<int32_t>(GPUMemoryPool::kLpExcluded) : nullptr;
}
// the first slot the pair (lo <= hi) is looked for in a table of cap slots (a power of two): the kernels' function (lp_exclude.h), for a test to pin
uint32_t legion_lp_pair_slot(uint32_t lo, uint32_t hi, uint32_t cap) { return lp_pair_slot(lo, hi, cap); }
int GPUMemoryPool_GetAggLastHop(const GPUMemoryPool* p) { return p && p->modes.agg_last_hop ? 1 : 0; }
int GPUMemoryPool_GetAggNorm(const GPUMemoryPool* p) { return p ? p->modes.agg_norm : 0; }
int GPUMemoryPool_GetSampleDistinct(const GPUMemoryPool* p) { return p && p->modes.sampling == kSamplingDistinct ? 1 : 0; }
int GPUMemoryPool_GetSampleSeed(const GPUMemoryPool* p, uint32_t* seed)
{
    if (seed) *seed = p ? p->modes.seed : 0;
    return p && p->modes.seeded ? 1 : 0;
}
// the current pipe's block out-degrees as the last normalised batch left them (int32[legion_batch_nodes(nc, H)]); null before the mode was set
int32_t* GPUMemoryPool_GetAggOutDeg(const GPUMemoryPool* p)
{
    return p ? p->pipe().buf<int32_t>(GPUMemoryPool::kAggOutDeg) : nullptr;
}
int32_t GPUMemoryPool_GetRound(const GPUMemoryPool* p) { return p ? (int32_t)p->round : 0; }

// A new round (the trainer's epoch) begins: the draw words and the shuffle of the batches that follow are those of `round`.  Under a seed the
// pool's shuffled copy of (noder, dev_id)'s training list is (re)filled on `stream` -- the stream the batch generator runs on, so that the
// first k_seed of the round is ordered behind it.  noder == null: the training list stays in file order (lists served verbatim, e.g.
// link-prediction thirds); the draws are seeded all the same.  With the mode off the round is recorded and nothing is launched.
int GPUMemoryPool_BeginRound(void* stream, GPUMemoryPool* p, GPUNodeStorage* noder, int32_t dev_id, int32_t round)
{
    if (!p) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: null pool"); return -1; }
    if (p->capturing) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: the pool is being captured (a round begins between batches, not inside a recording)"); return -1; }
    if (round < 0) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: negative round"); return -1; }
    if (p->round != (uint32_t)round) p->shuf_valid = false;   // whatever the mode: the copy holds another round's permutation
    p->round = (uint32_t)round;
    p->ctl_synced = false;   // the next replay resets the cursor: k_set_cursor carries the round's draw key
    if (!p->modes.seeded) return 0;
    p->shuf_file_order = noder == nullptr;
    p->shuf_valid = false;
    if (!noder) return 0;
    if (!p->owns_scratch) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: GPUMemoryPool_AllocateScratch was not called"); return -1; }
    const GPUNodeStorage::SeedSet& set = noder->seed_set(LEGION_TRAINMODE, dev_id);
    if (set.num > 0 && (!set.ids || !set.labels)) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: the training list of this device is not built"); return -1; }
    const int32_t k = p->modes.lp_draw;   // drawn link-prediction thirds: whole triples move
    if (k > 0 && set.num % (3 * k) != 0) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: drawn link-prediction thirds (GPUMemoryPool_SetLpDraw): the training list's length is not a multiple of the batch of 3 k ([src | pos | neg] thirds, padded)"); return -1; }
    if (set.num > p->shuf_cap || !p->shuf_ids) {   // first use, or a longer list: batches that read the old copy may still be in flight
        HIP_CHECK(hipDeviceSynchronize());
        release_shuffle(p);
        p->shuf_cap = std::max(set.num, 1);
        HIP_CHECK(hipMalloc(&p->shuf_ids, (size_t)p->shuf_cap * sizeof(int32_t)));
        HIP_CHECK(hipMalloc(&p->shuf_labels, (size_t)p->shuf_cap * sizeof(int32_t)));
        if (!p->shuf_ids || !p->shuf_labels) return -1;
    }
    if (k > 0) launch_shuffle_triples((hipStream_t)stream, set.ids, set.labels, set.num, k, seeded_shuffle_key(p->modes.seed, p->round), p->shuf_ids, p->shuf_labels);
    else launch_shuffle_seeds((hipStream_t)stream, set.ids, set.labels, set.num, seeded_shuffle_key(p->modes.seed, p->round), p->shuf_ids, p->shuf_labels);
    p->shuf_n = set.num;
    p->shuf_src = set.ids;
    p->shuf_valid = true;
    return error_pending() ? -1 : 0;
}

#define POOL_PIPE_SETTER(name, field, type) \
    void GPUMemoryPool_Set##name(GPUMemoryPool* p, type* ptr, int32_t pipe) { \
        if (pipe < 0 || pipe >= p->pipeline_depth) { LEGION_ARG_ERROR("GPUMemoryPool_Set" #name ": bad pipe"); return; } \
        p->pipes[pipe].field = ptr; } \
    type* GPUMemoryPool_Get##name(const GPUMemoryPool* p) { return p->pipe().field; }
POOL_PIPE_SETTER(SampledIds, sampled_ids, int32_t)
POOL_PIPE_SETTER(FloatFeatures, float_features, float)
POOL_PIPE_SETTER(Labels, labels, int32_t)
POOL_PIPE_SETTER(AggSrcOf, agg_src_off, int32_t)
POOL_PIPE_SETTER(AggDstOf, agg_dst_off, int32_t)
POOL_PIPE_SETTER(NodeCounter, node_counter, int32_t)
POOL_PIPE_SETTER(EdgeCounter, edge_counter, int32_t)
#undef POOL_PIPE_SETTER
void GPUMemoryPool_SetFeatureRows(GPUMemoryPool* p, int32_t rows) { p->feature_rows = rows; }
void GPUMemoryPool_SetCurrentPipe(GPUMemoryPool* p, int32_t pipe) { p->current_pipe = pipe % p->pipeline_depth; }
void GPUMemoryPool_SetCurrentMode(GPUMemoryPool* p, int32_t mode) { p->mode = mode; }
void GPUMemoryPool_SetIter(GPUMemoryPool* p, int32_t iter) { p->iter = iter; }
int32_t GPUMemoryPool_GetCurrentMode(const GPUMemoryPool* p) { return p->mode; }
int32_t GPUMemoryPool_GetIter(const GPUMemoryPool* p) { return p->iter; }
int32_t* GPUMemoryPool_GetAggSrcId(const GPUMemoryPool* p) { return p->agg_src_ids; }
int32_t* GPUMemoryPool_GetCacheSearchBuffer(const GPUMemoryPool* p) { return p->cache_search_buffer; }
char* GPUMemoryPool_GetTmpPartIdx(const GPUMemoryPool* p) { return (char*)p->tmp_part_ind; }
int32_t* GPUMemoryPool_GetTmpPartOff(const GPUMemoryPool* p) { return p->tmp_part_off; }
uint64_t* GPUMemoryPool_GetPositionMap(const GPUMemoryPool* p) { return (uint64_t*)p->pos_map; }
int32_t* GPUMemoryPool_GetCandidateBuffer(const GPUMemoryPool* p) { return p->cand; }
// The list of pool_scratch() and the listed rows of pool_pipe_buffers(), then ctl, one entry per call: 0 and *out filled, 1 past the end of the list, -1
// (sticky error) for a null argument or a pipe the pool does not have.  Reads host state only: no device call, nothing changes.
int GPUMemoryPool_ScratchInfo(const GPUMemoryPool* pool, int32_t index, int32_t pipe, LegionScratchInfo* out)
{
    if (!pool || !out) { LEGION_ARG_ERROR("GPUMemoryPool_ScratchInfo: null argument"); return -1; }
    if (index < 0 || pipe < 0 || pipe >= pool->pipeline_depth) { LEGION_ARG_ERROR("GPUMemoryPool_ScratchInfo: bad index or pipe"); return -1; }
    GPUMemoryPool* p = const_cast<GPUMemoryPool*>(pool);   // pool_scratch takes the pool it allocates into; nothing is written through it here
    std::vector<LegionScratchInfo> all;
    for (const ScratchBuffer& b : pool_scratch(p)) all.push_back({b.name, *b.slot, (int64_t)b.bytes, b.kind, b.elem_bytes, b.lifetime, 0});
    for (const PipeBuffer& b : pool_pipe_buffers(p))
        if (b.listed) all.push_back({b.name, p->pipes[pipe].own[b.which], (int64_t)b.bytes, b.kind, b.elem_bytes, b.lifetime, 1});
    all.push_back({"ctl", p->ctl, (int64_t)sizeof(BatchCtl), LEGION_SCRATCH_COUNT, (int32_t)sizeof(int32_t), LEGION_SCRATCH_STATE, 0});
    if (index >= (int32_t)all.size()) return 1;
    *out = all[index];
    return 0;
}
uint32_t GPUMemoryPool_GetBatchSerial(const GPUMemoryPool* p) { return p->batch_serial; }
void GPUMemoryPool_SetBatchSerial(GPUMemoryPool* p, uint32_t serial) { p->batch_serial = serial; p->ctl_synced = false; }

void GPUMemoryPool_Finalize(GPUMemoryPool* p)
{
    if (!p || !p->owns_scratch) return;
    GPUMemoryPool_ReleasePeerExchange(p);
    release_scratch(p);
    release_ctl(p);
    release_rows_seen(p);
    release_shuffle(p);
    p->owns_scratch = false;
}
void GPUMemoryPool_Delete(GPUMemoryPool* p)
{
    if (!p) return;
    GPUMemoryPool_Finalize(p);
    delete p;
}

} // extern "C"
