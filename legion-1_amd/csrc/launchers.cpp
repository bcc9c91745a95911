// launchers.cpp -- the extern "C" operator launchers of the reference (src/Kernels.cuh:47-93,
// Kernels.cu:162-232,567-659,706-805) on top of the kernels' launch wrappers (sampler.hip, gather.hip), plus the Operator plugin classes
// (src/Operator.h:4-27, Operator.cu:10-124).
#include "internal.h"

#include <algorithm>
#include <cstring>
#include <iostream>

#include "lp_exclude.h"

#include "audit_hooks.h"

using namespace legion;

static inline int pool_dev(const GPUMemoryPool* p)
{
    if (p->device_id >= 0) return p->device_id;
    if (current_logical_device() >= 0) return current_logical_device();   // the logical GPU this thread selected (SetGPUDevice)
    int d = 0;
    (void)hipGetDevice(&d); // reference: dev_id = cudaGetDevice() (Kernels.cu:577-578)
    return d;
}

using Pool = GPUMemoryPool;
using Pipe = Pool::Pipe;

// the pool's current pipe, once the pool owns scratch and the caller registered the pipe's output buffers; null (sticky error) otherwise
static Pipe* pool_ready(GPUMemoryPool* p, const char* who)
{
    if (!p || !p->owns_scratch) { LEGION_ARG_ERROR((std::string(who) + ": GPUMemoryPool_AllocateScratch was not called").c_str()); return nullptr; }
    Pipe& pipe = p->pipe();
    if (!pipe.sampled_ids || !pipe.labels || !pipe.agg_src_off || !pipe.agg_dst_off || !pipe.node_counter || !pipe.edge_counter) {
        LEGION_ARG_ERROR((std::string(who) + ": output buffers of the current pipe are not set").c_str());
        return nullptr;
    }
    return &pipe;
}
// the pipe holds every one of `rows` (pool_pipe_buffers' rows, by Pipe::own[]) -- and `also`, what the caller needs beside them; false with `refusal` as the sticky error
static bool pipe_holds(const Pipe& pipe, std::initializer_list<Pool::PipeBuf> rows, const char* refusal, bool also = true)
{
    for (Pool::PipeBuf b : rows) also = also && pipe.own[b];
    if (!also) LEGION_ARG_ERROR(refusal);
    return also;
}

// Where logical GPU `dev` reads adjacency rows from: the whole CSR -- its HBM replica when there is one, else the (pinned host) table --
// and, with `fragments` (every launch but those of pre-sampling: a pre-sampling hop, a seed launch while the cache is still pre-sampling),
// the clique's fragments through the topology map, once the cache holds one and every fragment that map can name is readable from here.  The one statement of the rule: the sampler's hops and the positives of
// the drawn link-prediction thirds read a row from the same place.
static void csr_tables_of(CsrTables& csr, const GPUGraphStorage* graph, const GPUCache* cache, int dev, bool fragments)
{
    const int P = graph->partition_count;
    csr.partition_count = P;
    csr.indptr = graph->replica_indptr[dev] ? graph->replica_indptr[dev] : graph->csr_node_index_cpu;
    csr.indices = graph->replica_indices[dev] ? graph->replica_indices[dev] : graph->csr_dst_node_ids_cpu;
    csr.frag_indptr = nullptr; csr.frag_indices = nullptr;
    csr.ip_nch = csr.ix_nch = 1; csr.row_shift = graph->row_shift; csr.edge_shift = graph->edge_shift;
    csr.topo_owner = nullptr;
    csr.topo_row = nullptr;
    if (!fragments || !cache || dev >= cache->device_count || !cache->ctl[dev]->topo_owner || cache->ctl[dev]->edge_capacity <= 0) return;
    // every fragment the topology map of this GPU can name must be readable from here
    bool all = graph->d_frag_tab[dev] != nullptr;
    const int Kg = cache->Kg, K0 = (dev / Kg) * Kg;
    for (int g = K0; g < K0 + Kg && all; g++) all = graph->view[dev][g] && graph->frag[g].complete;
    if (all) {
        csr.frag_indptr = (const int64_t* const*)graph->d_frag_tab[dev];
        csr.frag_indices = (const int32_t* const*)(graph->d_frag_tab[dev] + (size_t)P * graph->ip_nch);
        csr.ip_nch = graph->ip_nch; csr.ix_nch = graph->ix_nch;
        csr.topo_owner = cache->ctl[dev]->topo_owner; csr.topo_row = cache->ctl[dev]->topo_row;
    }
}

// What logical GPU `dev` draws a hop by under `modes`: the rule, and the alias table and -- without replacement, which the graph keeps them
// for only when asked to -- the weights beside the whole CSR (both rules without replacement: by column key and by node key).  False (sticky error): the graph lacks the rule's table on this GPU.
static bool draw_tables_of(DrawTables& t, const GPUGraphStorage* graph, const ServeModes& modes, int dev)
{
    t.rule = draw_rule_of(modes);
    const bool weighted = draw_rule_facts(t.rule).whole_csr, wdistinct = draw_rule_facts(t.rule).reads_weights;
    t.alias = weighted && dev < (int)graph->alias.size() ? graph->alias[dev] : nullptr;
    t.weights = wdistinct && dev < (int)graph->weights.size() ? graph->weights[dev] : nullptr;
    if (weighted && !t.alias) { LEGION_ARG_ERROR("GPU_Random_Sampling: weighted sampling (GPUMemoryPool_SetSampling) over a graph without edge weights on this GPU: call GPUGraphStorage_SetEdgeWeights first"); return false; }
    if (wdistinct && !t.weights) { LEGION_ARG_ERROR("GPU_Random_Sampling: weighted sampling without replacement (GPUMemoryPool_SetWeightedDistinct) over a graph without retained edge weights on this GPU: call GPUGraphStorage_RetainEdgeWeights before GPUGraphStorage_SetEdgeWeights"); return false; }
    return true;
}

extern "C" {

// batch_generator_kernel, Kernels.cu:162-232
void batch_generator_kernel(void* strm_hdl, GPUNodeStorage* noder, GPUCache* cache, GPUMemoryPool* memorypool,
                            int32_t batch_size, int32_t counter, int32_t part_id, int32_t dev_id, int32_t mode)
{
    (void)part_id;   // cache: only the drawn link-prediction thirds look at it (the topology map of the positives' rows)
    const Pipe* pipe = noder ? pool_ready(memorypool, "batch_generator_kernel") : nullptr;
    if (!pipe) return;
    hipStream_t s = (hipStream_t)strm_hdl;
    if (mode < 0 || mode >= kModes) log_out() << "invalid mode: " << mode << "\n";
    const GPUNodeStorage::SeedSet& set = noder->seed_set(mode, dev_id);   // empty for an invalid mode
    int32_t* all_ids = set.ids;
    int32_t* all_labels = set.labels;
    const int32_t total_cap = set.num;
    if (all_ids == nullptr) { log_out() << "invalid src id ptr\n"; return; }
    if (all_labels == nullptr) { log_out() << "invalid label ptr\n"; return; }

    GPUMemoryPool* p = memorypool;
    // Seeded sampling: a training batch reads the round's shuffled copy of the list (same length, same indexing) unless the round was
    // begun in file order; the draw word of the batch comes from the pool's (seed, round) and the counter.
    const uint32_t seeded = p->modes.seeded ? 1u : 0u, draw_key = p->modes.seeded ? seeded_draw_key(p->modes.seed, p->round) : 0u;
    p->seed_reads_shuffle = false;
    if (p->modes.seeded && mode == LEGION_TRAINMODE && !p->shuf_file_order) {
        if (!p->shuf_valid || p->shuf_src != set.ids || p->shuf_n != total_cap) {
            LEGION_ARG_ERROR("batch_generator_kernel: seeded sampling (GPUMemoryPool_SetSampleSeed) serves training batches from the round's shuffled list: call GPUMemoryPool_BeginRound for this device's training list first");
            return;
        }
        all_ids = p->shuf_ids;
        all_labels = p->shuf_labels;
        p->seed_reads_shuffle = true;
    }
    // Drawn link-prediction thirds: a training batch is 3 k slots, the last two thirds drawn inside k_seed from the batch's draw word
    LpDrawArgs lp_args;
    const LpDrawArgs* lp = nullptr;
    if (p->modes.lp_draw > 0 && mode == LEGION_TRAINMODE) {
        const int32_t k = p->modes.lp_draw;
        const GPUGraphStorage* graph = p->lp_graph;
        if (!p->modes.seeded) { LEGION_ARG_ERROR("batch_generator_kernel: drawn link-prediction thirds (GPUMemoryPool_SetLpDraw) draw from the batch's draw word: seed the pool first (GPUMemoryPool_SetSampleSeed)"); return; }
        if (batch_size != 3 * k) { LEGION_ARG_ERROR("batch_generator_kernel: drawn link-prediction thirds (GPUMemoryPool_SetLpDraw): the batch size must be three times the pool's triples per batch"); return; }
        if (total_cap % (3 * k) != 0) { LEGION_ARG_ERROR("batch_generator_kernel: drawn link-prediction thirds (GPUMemoryPool_SetLpDraw): the training list's length is not a multiple of the batch of 3 k ([src | pos | neg] thirds, padded)"); return; }
        if (!graph || dev_id < 0 || dev_id >= graph->partition_count) { LEGION_ARG_ERROR("batch_generator_kernel: drawn link-prediction thirds (GPUMemoryPool_SetLpDraw): device outside the partition table of the pool's graph"); return; }
        lp_args.k = k;
        lp_args.V = std::min(p->V, graph->node_num);
        csr_tables_of(lp_args.csr, graph, cache, dev_id, cache && !cache->is_presc);   // pre-sampling batches: the whole CSR, like their hops
        lp = &lp_args;
    }
    // Target-edge exclusion: a training batch is 3 k seeds whose first two thirds are the target pairs; k_lp_pairs behind k_seed builds their table
    const int32_t lpx = mode == LEGION_TRAINMODE ? p->modes.lp_exclude : 0;
    if (lpx > 0) {
        if (batch_size != 3 * lpx) { LEGION_ARG_ERROR("batch_generator_kernel: target-edge exclusion (GPUMemoryPool_SetLpExclude): the batch size must be three times the pool's triples per batch"); return; }
        if (total_cap % (3 * lpx) != 0) { LEGION_ARG_ERROR("batch_generator_kernel: target-edge exclusion (GPUMemoryPool_SetLpExclude): the training list's length is not a multiple of the batch of 3 k ([src | pos | neg] thirds, padded)"); return; }
        if (!pipe_holds(*pipe, {Pool::kLpPairs, Pool::kEdgeKeep, Pool::kLpExcluded}, "batch_generator_kernel: target-edge exclusion (GPUMemoryPool_SetLpExclude) without the pool's per-pipe buffers (the mode was set before GPUMemoryPool_AllocateScratch failed?)", p->lp_alloc_cap == lp_pair_cap(lpx) && 3 * lpx <= p->batch_size)) return;
    }
    if (p->device_id != dev_id && audit::on()) {   // the pool starts serving this GPU: its scratch and its output buffers must live there
        for (const ScratchBuffer& b : pool_scratch(p)) if (*b.slot) LEGION_AUDIT_OWNER(*b.slot, dev_id, "batch_generator_kernel: scratch of the memory pool");
        for (const PipeBuffer& b : pool_pipe_buffers(p))
            for (const Pipe& each : p->pipes) if (each.own[b.which]) LEGION_AUDIT_OWNER(each.own[b.which], dev_id, "batch_generator_kernel: scratch of the memory pool");
        for (const Pipe& each : p->pipes) {
            LEGION_AUDIT_OWNER(each.sampled_ids, dev_id, "batch_generator_kernel: output buffers of the memory pool");
            LEGION_AUDIT_OWNER(each.node_counter, dev_id, "batch_generator_kernel: output buffers of the memory pool");
        }
        LEGION_AUDIT_OWNER(all_ids, dev_id, "batch_generator_kernel: seed list");
    }
    p->device_id = dev_id;
    p->progress = {};
    p->pipe().edge_feat_filled = false;   // a new batch on this pipe: its edge rows are not gathered yet
    p->pipe().lp_marked = false;          // ... and its edges are not marked yet
    SeedArgs a;
    a.batch_ids = pipe->sampled_ids; a.labels = pipe->labels; a.batch_size = batch_size;
    a.all_ids = all_ids; a.all_labels = all_labels; a.total_cap = total_cap;
    a.pos_map = p->pos_map; a.ctl = p->ctl; a.nc = pipe->node_counter; a.ec = pipe->edge_counter;
    a.aux_next = p->aux2[1]; a.f_next = p->fanout[0]; a.aux_cap = p->max_slots;
    a.seeded = seeded; a.draw_key = draw_key; a.lp = lp;
    if (p->capturing) {
        // Recording a batch graph: cursor, epoch and the clamped size (Kernels.cu:224) are read / computed on the
        // device, `counter` is ignored, bounds are those of a full batch.
        a.size = batch_size; a.counter = 0; a.epoch = 0;
    } else {
        // A new batch = a new epoch of the position table: entries of older batches become stale without
        // touching them (replaces cudaMemsetAsync(accessed_map) + ClearPosMap, Kernels.cu:216,750-756).
        if (++p->batch_serial >= kSerialLimit) { // epoch space exhausted: wipe once and start over
            HIP_CHECK(hipMemsetAsync(p->pos_map, 0xFF, (size_t)p->V * sizeof(pos_t), s));
            p->batch_serial = 1;
        }
        p->ctl_synced = false; // k_seed publishes (counter, epoch) of THIS batch: a batch graph must reset the cursor
        a.size = ((batch_size * (counter + 1)) >= total_cap) ? (total_cap - batch_size * counter) : batch_size;   // Kernels.cu:224
        a.counter = counter; a.epoch = kEpochTop - p->batch_serial;
    }
    if (a.size > p->batch_size) { LEGION_ARG_ERROR("batch_generator_kernel: batch larger than the pool was sized for"); return; }
    launch_seed(s, a, p->capturing);
    if (lpx > 0) {   // reads ids[0, 2 k) and the level-0 size as k_seed left them on this stream: a recorded batch has no per-batch arguments
        LpPairsArgs t;
        t.ids = pipe->sampled_ids; t.nc = pipe->node_counter; t.pairs = pipe->buf<uint64_t>(Pool::kLpPairs); t.excluded = pipe->buf<int32_t>(Pool::kLpExcluded);
        t.k = lpx; t.cap = p->lp_alloc_cap;
        launch_lp_pairs(s, t);
        p->progress.lp_pairs_built = true;
    }
    p->aux_ready_hop = 1; p->aux_ready_count = p->fanout[0]; // k_seed prepared the slot states of hop 1
    p->bound_n = a.size > 0 ? a.size : 0;
    p->bound_nodes = p->bound_n;
}

// GPU_Random_Sampling, Kernels.cu:567-659
void GPU_Random_Sampling(void* strm_hdl, GPUGraphStorage* graph, GPUCache* cache, GPUMemoryPool* memorypool,
                         int32_t count, int32_t op_id, int is_presc)
{
    if (graph == nullptr) { log_out() << "invalid storage ptr\n"; return; }
    Pipe* pipe = pool_ready(memorypool, "GPU_Random_Sampling");
    if (!pipe) return;
    GPUMemoryPool* p = memorypool;
    const int hop = op_id / 2;
    if (op_id < 2 || (op_id & 1) || hop > p->hops) { LEGION_ARG_ERROR("GPU_Random_Sampling: op_id must be 2,4,..,2*hops"); return; }
    const int dev = pool_dev(p);
    const int P = graph->partition_count;
    if (dev < 0 || dev >= P) { LEGION_ARG_ERROR("GPU_Random_Sampling: device outside the partition table"); return; }
    const int64_t slots = (int64_t)p->bound_n * count;
    if (slots > p->max_slots) { LEGION_ARG_ERROR("GPU_Random_Sampling: fan-out exceeds what the pool was sized for"); return; }
    if (slots <= 0) return;

    DrawTables draw;
    if (!draw_tables_of(draw, graph, p->modes, dev)) return;
    CsrTables csr;
    csr_tables_of(csr, graph, cache, dev, !is_presc && sample_variant_exists(RowSource::Fragments, draw.rule, false));   // pre-sampling: the whole CSR only (kernel_pre_sampler_optimized, Kernels.cu:636-649)
    SamplerBuffers b;
    b.sampled_ids = pipe->sampled_ids; b.agg_src_ids = p->agg_src_ids; b.agg_src_off = pipe->agg_src_off;
    b.agg_dst_off = pipe->agg_dst_off; b.nc = pipe->node_counter; b.ec = pipe->edge_counter;
    b.pos_map = p->pos_map; b.ctl = p->ctl; b.cand = p->cand;
    if (p->modes.agg_last_hop && hop == p->hops) {   // k_gather_sum reads the last hop's draws while the next batch samples: the pipe's own buffer
        if (!pipe_holds(*pipe, {Pool::kCandPipe}, "GPU_Random_Sampling: aggregated last hop without the per-pipe draw buffers (GPUMemoryPool_SetAggLastHop before AllocateScratch failed?)")) return;
        b.cand = pipe->buf<int32_t>(Pool::kCandPipe);
    }
    b.aux = p->aux2[hop & 1]; b.aux_next = p->aux2[(hop + 1) & 1]; b.tile_edge = p->tile_edge; b.tile_node = p->tile_node; b.tile_pre = p->tile_pre; b.chunk_tot = p->chunk_tot;
    b.hop_state = p->hop_state; b.edge_access_time = nullptr;
    if (is_presc) {
        // kernel_pre_sampler_optimized: host CSR only + topology hotness (Kernels.cu:636-649)
        if (!cache || dev >= cache->device_count || !cache->ctl[dev]->edge_access_time) { LEGION_ARG_ERROR("GPU_Random_Sampling: pre-sampling needs an initialised cache controller"); return; }
        b.edge_access_time = cache->ctl[dev]->edge_access_time;
    }
    b.aux_cap = p->max_slots;
    b.ids_cap = p->num_ids;
    b.V = p->V;
    b.aux_prepared = p->aux_ready_hop == hop && p->aux_ready_count == count;
    b.next_count = hop < p->hops ? p->fanout[hop] : 0;
    // Edge ids (GPUMemoryPool_SetEdgeIds): the hop parks its columns and one more launch behind k_write, on this stream, leaves every edge's
    // position in the WHOLE CSR in the pipe's buffer -- and its weight, where this GPU holds the graph's retained weights.  A pre-sampling
    // batch hands nothing over: it runs the hop as it always did, whatever the mode says.
    EdgeIdOut eo_args;
    const EdgeIdOut* eo = nullptr;
    if (p->modes.edge_ids && !is_presc) {
        if (!pipe_holds(*pipe, {Pool::kEdgeIds, Pool::kEdgeW}, "GPU_Random_Sampling: edge ids (GPUMemoryPool_SetEdgeIds) without the pool's buffers (the mode was set before GPUMemoryPool_AllocateScratch failed?)", p->cols != nullptr)) return;
        CsrTables whole;
        csr_tables_of(whole, graph, cache, dev, false);
        eo_args.cols = p->cols; eo_args.edge_ids = pipe->buf<int64_t>(Pool::kEdgeIds); eo_args.edge_w = pipe->buf<float>(Pool::kEdgeW);
        eo_args.indptr = whole.indptr; eo_args.E = graph->edge_num;
        eo_args.weights = graph->retain_weights && dev < (int)graph->weights.size() ? graph->weights[dev] : nullptr;
        pipe->edge_w_filled = eo_args.weights != nullptr;
        eo = &eo_args;
    }
    launch_sample_hop((hipStream_t)strm_hdl, csr, b, count, op_id, p->hops, (int32_t)slots, is_presc != 0, draw, eo);
    p->aux_ready_hop = hop + 1; p->aux_ready_count = b.next_count; // k_write prepared the next hop's slot states
    p->progress.sampled_hop = hop; p->progress.sampled_presc = is_presc != 0;
    if (eo && p->progress.edge_id_hop == hop - 1) p->progress.edge_id_hop = hop;
    // Target-edge exclusion (GPUMemoryPool_SetLpExclude): behind the last hop, on this stream and in front of the level's event, one launch marks
    // every edge of the batch from the pipe's own buffers.  A batch without a pair table (not a training batch) keeps every edge; a
    // pre-sampling batch hands nothing over.
    if (p->modes.lp_exclude > 0 && hop == p->hops && !is_presc) {
        if (!pipe_holds(*pipe, {Pool::kLpPairs, Pool::kEdgeKeep, Pool::kLpExcluded}, "GPU_Random_Sampling: target-edge exclusion (GPUMemoryPool_SetLpExclude) without the pool's per-pipe buffers (the mode was set before GPUMemoryPool_AllocateScratch failed?)", p->lp_alloc_cap == lp_pair_cap(p->modes.lp_exclude))) return;
        LpKeepArgs m;
        m.ids = pipe->sampled_ids; m.src_off = pipe->agg_src_off; m.dst_off = pipe->agg_dst_off; m.nc = pipe->node_counter; m.ec = pipe->edge_counter;
        m.pairs = pipe->buf<uint64_t>(Pool::kLpPairs); m.keep = pipe->buf<uint8_t>(Pool::kEdgeKeep); m.excluded = pipe->buf<int32_t>(Pool::kLpExcluded);
        m.k = p->modes.lp_exclude; m.cap = p->lp_alloc_cap; m.hops = p->hops; m.ids_cap = p->num_ids; m.active = p->progress.lp_pairs_built;
        launch_lp_edge_keep((hipStream_t)strm_hdl, m, p->num_ids);
        if (!p->capturing) pipe->lp_marked = true;   // a recording marks nothing yet: its replay sets the flag (LegionBatchGraph_Launch)
        p->progress.lp_marked = true;
    }
    p->bound_n = (int32_t)slots;          // next hop expands every sampled edge endpoint
    p->bound_nodes += (int32_t)slots;
}

// Launch-size feedback (launch.h: est_rows): the row count an earlier launch of this kind left in word `slot` of the pool's rows_seen
// becomes this launch's hint, and this launch leaves its own count in the same word.
static void rows_seen_feedback(GatherArgs& g, const GPUMemoryPool* p, int slot)
{
    if (!p->rows_seen || !p->rows_seen_dev) return;
    g.rows_hint = *(volatile int32_t*)(p->rows_seen + slot);
    g.rows_seen = p->rows_seen_dev + slot;
}

// Arguments of a gather over the rows (nc[off_idx], nc[size_idx]) of the current pipe; false (sticky error) if it cannot run.
static bool gather_args(GatherArgs& g, GPUCache* cache, GPUNodeStorage* noder, GPUMemoryPool* p, const Pipe& pipe, int32_t dev_id, int off_idx, int size_idx,
                        bool count_hits = true)
{
    const int32_t F = noder->float_attr_len;
    if (F < 0) log_out() << "error feature len\n"; // Kernels.cu:719-721
    if (!pipe.float_features) { LEGION_ARG_ERROR("get_feature_kernel: feature buffer of the current pipe is not set"); return false; }
    const bool replica = dev_id >= 0 && dev_id < noder->partition_count && noder->replica_attrs[dev_id];
    g.table = replica ? noder->replica_attrs[dev_id] : noder->float_attrs;
    g.table_pitch = replica ? noder->replica_pitch : noder->float_attr_pitch;
    g.shard_pitch = cache ? cache->shard_pitch : 0;
    g.table_on_host = g.table == noder->float_attrs && noder->features_location != LEGION_LOC_DEVICE;
    g.shard_tab = nullptr; g.chunk_shift = 30; g.nchunks = 1;
    g.feat_map = nullptr;
    g.row_ptr = nullptr; g.row_ptr_ready = false;
    g.cache_capacity = 1;
    g.F = F;
    g.total_num_nodes = noder->total_num_nodes;
    g.sampled_ids = pipe.sampled_ids;
    g.nc = pipe.node_counter;
    g.dst = pipe.float_features;
    g.off_idx = off_idx;
    g.size_idx = size_idx;
    g.dst_rows = p->feature_rows;
    g.rows_seen = nullptr; g.rows_hint = 0;
    g.hit_stats = nullptr;
    rows_seen_feedback(g, p, off_idx < 0 ? kRowsSeenAll : legion_idx_level(off_idx));   // level of a per-level gather, or "all rows of the batch"
    if (cache && dev_id >= 0 && dev_id < cache->device_count && cache->ctl[dev_id]->feat_map && cache->ctl[dev_id]->node_capacity > 0 &&
        cache->d_shard_tab[dev_id]) {
        const int Ki = dev_id / cache->Kg;
        g.feat_map = cache->ctl[dev_id]->feat_map;
        g.cache_capacity = cache->ctl[dev_id]->node_capacity;
        g.shard_tab = cache->d_shard_tab[dev_id]; // d_float_feature_cache_ptr_, GPUCache.cu:788-816
        g.chunk_shift = cache->chunk_shift[Ki];
        g.nchunks = cache->nchunks[Ki];
        g.row_ptr = p->row_ptr; // FindFeat + source selection as their own pass over the rows (k_row_ptrs)
        // the last gather of a batch: level `hops` of the per-level gathers, or the one gather over all rows
        // (a recorded batch graph would bake the decision in: graphs never sample)
        if (!p->capturing && count_hits) g.hit_stats = GPUCache_HitSampling(cache, dev_id, off_idx < 0 || off_idx == legion_idx_level_offset(p->hops), off_idx < 0 || off_idx == legion_idx_level_offset(0));
    }
    if (!g.table && !g.feat_map) { LEGION_ARG_ERROR("get_feature_kernel: no feature table"); return false; }
    return true;
}

// false: refused, nothing launched
static bool gather_common(void* strm_hdl, GPUCache* cache, GPUNodeStorage* noder, GPUMemoryPool* p, const Pipe& pipe, int32_t dev_id,
                          int off_idx, int size_idx, int32_t rows_bound)
{
    GatherArgs g;
    // an aggregated batch never reaches the last level's gather, which closes a hit-rate sample: its level gathers do not open one
    if (!gather_args(g, cache, noder, p, pipe, dev_id, off_idx, size_idx, !p->modes.agg_last_hop)) return false;
    launch_gather((hipStream_t)strm_hdl, g, rows_bound);
    // last counting launch of a sampled batch: the host may read the pinned {hits, rows} words once this event completes
    if (g.hit_stats && (off_idx < 0 || off_idx == legion_idx_level_offset(p->hops))) GPUCache_HitSamplingDone(cache, dev_id, strm_hdl);
    return true;
}

static bool peer_gather_is_exchange()
{
    const char* e = getenv("LEGION_PEER_GATHER");
    return e && strcmp(e, "exchange") == 0;
}

// $LEGION_PEER_GATHER=exchange and a filled clique cache (Kg > 1, every member in this process): the peers' rows travel as bulk
// copies (peer_exchange.cpp) instead of in-kernel xGMI loads
static bool use_peer_exchange(const GPUCache* cache, const GPUMemoryPool* p, int32_t dev_id)
{
    if (!peer_gather_is_exchange() || !cache || p->capturing) return false;
    if (cache->Kg <= 1 || dev_id < 0 || dev_id >= cache->device_count || !cache->ctl[dev_id]->feat_map || cache->ctl[dev_id]->node_capacity <= 0) return false;
    const int K0 = (dev_id / cache->Kg) * cache->Kg;
    for (int j = 0; j < cache->Kg; j++) if (is_remote_device(K0 + j)) return false;
    return true;
}

// get_feature_kernel, Kernels.cu:706-748.  op_id 2l+1 gathers level l.
void get_feature_kernel(void* strm_hdl, GPUCache* cache, GPUNodeStorage* noder, GPUMemoryPool* memorypool,
                        int32_t dev_id, int32_t op_id, int in_memory)
{
    const Pipe* pipe = noder ? pool_ready(memorypool, "get_feature_kernel") : nullptr;
    if (!pipe) return;
    const int l = (op_id - 1) / 2;
    if (op_id < 1 || !(op_id & 1) || l > memorypool->hops) { LEGION_ARG_ERROR("get_feature_kernel: op_id must be 1,3,..,2*hops+1"); return; }
    if (!in_memory) return; // the reference only launches the in-memory path (Kernels.cu:737-746)
    if (use_peer_exchange(cache, memorypool, dev_id)) {   // one exchange per batch: the last level's op gathers every level
        if (l == memorypool->hops) legion_peer_exchange_gather(strm_hdl, cache, noder, memorypool, dev_id);
        return;
    }
    if (gather_common(strm_hdl, cache, noder, memorypool, *pipe, dev_id, legion_idx_level_offset(l), legion_idx_level_size(l), memorypool->level_bound[l]))
        memorypool->progress.levels_gathered |= 1u << l;
}

// Aggregated last hop (no counterpart in the reference): behind the last hop's GPU_Random_Sampling of a pool in that mode
// (GPUMemoryPool_SetAggLastHop).  Feature rows [0, n_in) -- the levels < H -- are gathered here unless get_feature_kernel already
// gathered each of them, and the neighbour sums of the last hop's N input slots are written behind them, rows [n_in, n_in + N).
// every reason get_feature_kernel_agg cannot run on the pool's current batch: true with the sticky error
static bool agg_refusal(const GPUMemoryPool* p, const Pipe& pipe)
{
    if (!p->modes.agg_last_hop) { LEGION_ARG_ERROR("get_feature_kernel_agg: the pool does not aggregate the last hop (GPUMemoryPool_SetAggLastHop)"); return true; }
    // the exchange moves rows between clique members, not sums
    if (peer_gather_is_exchange()) { LEGION_ARG_ERROR("get_feature_kernel_agg: LEGION_PEER_GATHER=exchange cannot serve the aggregated last hop (GPUMemoryPool_SetAggLastHop): the exchange moves rows, not sums"); return true; }
    if (p->progress.sampled_hop != p->hops) { LEGION_ARG_ERROR("get_feature_kernel_agg: called before the last hop's GPU_Random_Sampling"); return true; }
    if (p->progress.sampled_presc) { LEGION_ARG_ERROR("get_feature_kernel_agg: a pre-sampling batch gathers nothing"); return true; }
    if (!pipe_holds(pipe, {Pool::kCandPipe}, "get_feature_kernel_agg: the per-pipe draw buffers are missing")) return true;
    if (p->modes.agg_norm && !pipe_holds(pipe, {Pool::kAggOutDeg, Pool::kAggWdraw, Pool::kAggChunkCnt}, "get_feature_kernel_agg: the per-pipe buffers of the normalised sums are missing (GPUMemoryPool_SetAggNorm before AllocateScratch failed?)")) return true;
    if (p->modes.agg_norm && !pipe.agg_src_off) { LEGION_ARG_ERROR("get_feature_kernel_agg: the COO buffers of the current pipe are not set"); return true; }
    // Edge-weighted sums (GPUMemoryPool_SetAggEdgeWeight): every draw's weight is the edge_w k_edge_ids left behind the last hop, in the pipe's buffer
    const bool ew = p->modes.agg_edge_weight;
    if (ew && !pipe_holds(pipe, {Pool::kAggWdraw, Pool::kAggChunkCnt}, "get_feature_kernel_agg: the per-pipe buffers of the edge-weighted sums are missing (GPUMemoryPool_SetAggEdgeWeight before AllocateScratch failed?)")) return true;
    if (ew && (!p->modes.edge_ids || !pipe.own[Pool::kEdgeW] || !pipe.edge_w_filled)) { LEGION_ARG_ERROR("get_feature_kernel_agg: edge-weighted sums (GPUMemoryPool_SetAggEdgeWeight) over a batch without edge weights: the graph does not retain its weights (GPUGraphStorage_RetainEdgeWeights before GPUGraphStorage_SetEdgeWeights)"); return true; }
    return false;
}
// The weight of every draw of the last hop by slot (agg_wdraw), in front of the weighted sums, from the pipe's own draws: by the block's
// out-degrees over the pipe's COO (the norm), or the edge_w k_edge_ids left (the edge-weighted sums) -- whichever the modes ask for
static void launch_draw_weights(hipStream_t s, const GPUMemoryPool* p, const Pipe& pipe)
{
    const int H = p->hops;
    const int32_t slots = (int32_t)std::min<int64_t>((int64_t)p->level_bound[H - 1] * p->fanout[H - 1], p->max_slots);
    auto common = [&](auto w) {   // what the two passes' arguments share
        w.nc = pipe.node_counter; w.ec = pipe.edge_counter; w.hops = H; w.f = p->fanout[H - 1];
        w.cand = pipe.buf<int32_t>(Pool::kCandPipe); w.cand_cap = p->max_slots; w.ids_cap = p->num_ids;
        w.chunk_cnt = pipe.buf<int32_t>(Pool::kAggChunkCnt); w.wdraw = pipe.buf<float>(Pool::kAggWdraw);
        return w;
    };
    if (p->modes.agg_norm) {
        AggNormArgs w = common(AggNormArgs{});
        w.src_off = pipe.agg_src_off; w.out_deg = pipe.buf<int32_t>(Pool::kAggOutDeg);
        launch_agg_norm_weights(s, w, slots, p->num_ids);
    }
    if (p->modes.agg_edge_weight) {
        AggEdgeWeightArgs w = common(AggEdgeWeightArgs{});
        w.edge_w = pipe.buf<float>(Pool::kEdgeW);
        launch_agg_edge_weights(s, w, slots);
    }
}

void get_feature_kernel_agg(void* strm_hdl, GPUCache* cache, GPUNodeStorage* noder, GPUMemoryPool* memorypool,
                            int32_t dev_id, int in_memory)
{
    const Pipe* pipe = noder ? pool_ready(memorypool, "get_feature_kernel_agg") : nullptr;
    GPUMemoryPool* p = memorypool;
    if (!pipe || agg_refusal(p, *pipe) || !in_memory) return;
    const int H = p->hops;
    GatherArgs g;
    if (!gather_args(g, cache, noder, p, *pipe, dev_id, -1, legion_idx_level_offset(H), false)) return;   // rows [0, n_in): the levels < H; the hit counter belongs to the default mode's batches
    if ((p->progress.levels_gathered & ((1u << H) - 1u)) != (1u << H) - 1u) {
        rows_seen_feedback(g, p, kRowsSeenAggIn);
        launch_gather((hipStream_t)strm_hdl, g, p->num_ids - p->level_bound[H]);
    }
    rows_seen_feedback(g, p, kRowsSeenAggRuns);
    launch_draw_weights((hipStream_t)strm_hdl, p, *pipe);
    launch_gather_sum((hipStream_t)strm_hdl, g, pipe->buf<int32_t>(Pool::kCandPipe), p->max_slots, pipe->edge_counter, H, p->fanout[H - 1], p->level_bound[H - 1],
                      p->modes.agg_norm || p->modes.agg_edge_weight ? pipe->buf<float>(Pool::kAggWdraw) : nullptr);
}

void get_feature_kernel_all(void* strm_hdl, GPUCache* cache, GPUNodeStorage* noder, GPUMemoryPool* memorypool,
                            int32_t dev_id, int in_memory)
{
    const Pipe* pipe = noder ? pool_ready(memorypool, "get_feature_kernel_all") : nullptr;
    if (!pipe || !in_memory) return;
    if (use_peer_exchange(cache, memorypool, dev_id)) { legion_peer_exchange_gather(strm_hdl, cache, noder, memorypool, dev_id); return; }
    gather_common(strm_hdl, cache, noder, memorypool, *pipe, dev_id, -1, LEGION_NC_TOTAL, memorypool->num_ids); // every row of the batch
}

// ---- edge features (no counterpart in the reference; INTEGRATION.md "Edge features") ----
// edge_feat[e, :] = X[edge_ids[e], :] for the COO edges of hop `hop` of the current pipe's batch (hop 0: of every hop), X the graph's table on
// this GPU.  Everything read is the batch's pipe's or the graph's, so the call may follow the hop on the gather stream.  Refused by name: a pool
// that is not in the mode, a graph without a table on this GPU or with another row width, a batch that left no edge ids for the hop.
static void edge_feature_gather(void* strm_hdl, GPUGraphStorage* graph, GPUMemoryPool* p, int32_t dev_id, int hop, const char* who)
{
    const std::string name(who);
    Pipe* pipe = graph ? pool_ready(p, who) : nullptr;
    if (!pipe) { if (!graph) LEGION_ARG_ERROR((name + ": null graph").c_str()); return; }
    const int32_t dim = p->modes.edge_feat_dim;
    if (dim <= 0) { LEGION_ARG_ERROR((name + ": the pool does not gather edge features (GPUMemoryPool_SetEdgeFeatures)").c_str()); return; }
    const float* table = dev_id >= 0 && dev_id < (int32_t)graph->edge_feat.size() ? graph->edge_feat[dev_id] : nullptr;
    if (!table) { LEGION_ARG_ERROR((name + ": the graph holds no edge-feature table on this GPU (GPUGraphStorage_SetEdgeFeatures)").c_str()); return; }
    if (graph->edge_feat_dim != dim) { LEGION_ARG_ERROR((name + ": the graph's edge-feature table has rows of " + std::to_string(graph->edge_feat_dim) + " floats, the pool gathers rows of " + std::to_string(dim) + " (GPUMemoryPool_SetEdgeFeatures)").c_str()); return; }
    const int last = hop > 0 ? hop : p->hops;   // the last hop whose ids are read
    if (p->progress.sampled_presc || p->progress.edge_id_hop < last) { LEGION_ARG_ERROR((name + ": the current pipe's batch left no edge ids for this hop: a pre-sampling batch, a batch sampled with edge ids off, or a hop whose GPU_Random_Sampling has not been called").c_str()); return; }
    if (!pipe_holds(*pipe, {Pool::kEdgeIds, Pool::kEdgeFeat}, (name + ": edge features without the pool's per-pipe buffers (the mode was set before GPUMemoryPool_AllocateScratch failed?)").c_str(), p->edge_feat_alloc_dim == dim)) return;
    EdgeGatherArgs a;
    a.table = table; a.E = graph->edge_num; a.dim = dim;
    a.edge_ids = pipe->buf<int64_t>(Pool::kEdgeIds); a.ec = pipe->edge_counter; a.hop = hop; a.hops = p->hops;
    a.out = pipe->buf<float>(Pool::kEdgeFeat); a.ids_cap = p->num_ids;
    // the static bound of the range: the hop's slots, or every hop's (num_ids less the seeds)
    const int32_t bound = hop > 0 ? p->level_bound[hop] : p->num_ids - p->level_bound[0];
    launch_gather_edges((hipStream_t)strm_hdl, a, bound);
    if (!p->capturing) pipe->edge_feat_filled = true;   // a recording gathers nothing yet: its replay sets the flag (LegionBatchGraph_Launch)
    p->progress.edge_feat_gathered = true;
}
// op_id: the hop's sampling op (2, 4, .., 2 * hops), behind that hop's GPU_Random_Sampling
void get_edge_feature_kernel(void* strm_hdl, GPUGraphStorage* graph, GPUMemoryPool* memorypool, int32_t dev_id, int32_t op_id)
{
    if (memorypool && memorypool->owns_scratch && (op_id < 2 || (op_id & 1) || op_id / 2 > memorypool->hops)) { LEGION_ARG_ERROR("get_edge_feature_kernel: op_id must be 2,4,..,2*hops"); return; }
    edge_feature_gather(strm_hdl, graph, memorypool, dev_id, op_id / 2, "get_edge_feature_kernel");
}
// every edge of the batch in one launch, behind the last hop's GPU_Random_Sampling: the bytes of the per-hop calls
void get_edge_feature_kernel_all(void* strm_hdl, GPUGraphStorage* graph, GPUMemoryPool* memorypool, int32_t dev_id)
{
    edge_feature_gather(strm_hdl, graph, memorypool, dev_id, 0, "get_edge_feature_kernel_all");
}

// ---- owner-computes exchange variant of the gather (SURVEY 5 option b), one process per GPU ---------------------------------
// Step 1 on the requester.  Rows [0, nc[0]) of the batch: those cached on ANOTHER clique member are listed (req_row: row in the
// owner's shard, req_dst: row of the batch; contiguous per owner, owner-major; counts[j] rows for clique member j); every other row
// (own shard, backing table) gets its source address.  counts: device int32[2 * LEGION_MAX_DEVICE].  Nothing is gathered yet: the
// caller reads the counts back while legion_exchange_local (step 1b, any stream behind this one) gathers the local rows.
int legion_exchange_plan(void* strm_hdl, GPUCache* cache, GPUNodeStorage* noder, GPUMemoryPool* memorypool, int32_t dev_id,
                         int32_t* req_row, int32_t* req_dst, int32_t* counts)
{
    const Pipe* pipe = noder && cache && req_row && req_dst && counts ? pool_ready(memorypool, "legion_exchange_plan") : nullptr;
    if (!pipe) return -1;
    GPUMemoryPool* p = memorypool;
    GatherArgs g;
    if (!gather_args(g, cache, noder, p, *pipe, dev_id, -1, LEGION_NC_TOTAL, false)) return -1;      // the hit counter belongs to the lookup pass of k_row_ptrs
    if (!g.feat_map || !g.row_ptr || !p->cache_search_buffer) { LEGION_ARG_ERROR("legion_exchange_plan: needs a filled unified cache"); return -1; }
    launch_exchange_plan((hipStream_t)strm_hdl, g, dev_id % cache->Kg, cache->Kg, p->cache_search_buffer, counts, req_row, req_dst, p->num_ids);
    return error_pending() ? -1 : 0;
}
// Step 1b on the requester: gather the rows legion_exchange_plan resolved locally (own shard / backing table); the peers' rows
// have no source and are skipped -- legion_exchange_scatter fills them in.
int legion_exchange_local(void* strm_hdl, GPUCache* cache, GPUNodeStorage* noder, GPUMemoryPool* memorypool, int32_t dev_id)
{
    const Pipe* pipe = noder && cache ? pool_ready(memorypool, "legion_exchange_local") : nullptr;
    if (!pipe) return -1;
    GPUMemoryPool* p = memorypool;
    GatherArgs g;
    if (!gather_args(g, cache, noder, p, *pipe, dev_id, -1, LEGION_NC_TOTAL, false)) return -1;
    if (!g.row_ptr) { LEGION_ARG_ERROR("legion_exchange_local: needs a filled unified cache"); return -1; }
    g.row_ptr_ready = true;   // k_exch_fill resolved the local rows (and left the peers' rows without a source)
    launch_gather((hipStream_t)strm_hdl, g, p->num_ids);
    return error_pending() ? -1 : 0;
}
// Step 2 on the owner: rows list[0..n) of THIS GPU's shard -> out[n x F] (a contiguous send buffer).
void legion_exchange_serve(void* strm_hdl, GPUCache* cache, int32_t dev_id, const int32_t* list, int32_t n, float* out)
{
    if (!cache || dev_id < 0 || dev_id >= cache->device_count || !cache->d_shard_tab[dev_id] || (n > 0 && (!list || !out))) { LEGION_ARG_ERROR("legion_exchange_serve: bad arguments"); return; }
    const int Ki = dev_id / cache->Kg, j = dev_id % cache->Kg;
    launch_exchange_rows((hipStream_t)strm_hdl, false, cache->d_shard_tab[dev_id] + (size_t)j * cache->nchunks[Ki], cache->chunk_shift[Ki], list, n,
                         cache->float_attr_len, cache->shard_pitch, nullptr, out, 0);
}
// Step 3 on the requester: rows[k] (as the owners returned them, in request order) -> feature row req_dst[k] of the current pipe.
void legion_exchange_scatter(void* strm_hdl, GPUMemoryPool* memorypool, const float* rows, const int32_t* req_dst, int32_t n, int32_t F)
{
    const Pipe* pipe = pool_ready(memorypool, "legion_exchange_scatter");
    if (!pipe) return;
    float* dst = pipe->float_features;
    if (!dst || (n > 0 && (!rows || !req_dst))) { LEGION_ARG_ERROR("legion_exchange_scatter: bad arguments"); return; }
    launch_exchange_rows((hipStream_t)strm_hdl, true, nullptr, 0, req_dst, n, F, F, rows, dst, memorypool->feature_rows);
}

// make_update_plan, Kernels.cu:758-783
void make_update_plan(void* strm_hdl, GPUGraphStorage* graph, GPUCache* cache, GPUMemoryPool* memorypool,
                      int32_t dev_id, int32_t mode)
{
    (void)graph;
    const Pipe* pipe = pool_ready(memorypool, "make_update_plan");
    if (!pipe) return;
    hipStream_t s = (hipStream_t)strm_hdl;
    if (mode == LEGION_TRAINMODE && cache) // CacheProfiling: HotnessMeasure during pre-sampling
        GPUCache_CacheProfiling(cache, pipe->sampled_ids, pipe->node_counter, strm_hdl, dev_id);
    // ClearPosMap (Kernels.cu:780) needs no launch: the next batch starts a new table epoch.
    (void)s;
}

// update_cache, Kernels.cu:785-805: the reference body is commented out -- a no-op.
void update_cache(void* strm_hdl, GPUCache* cache, GPUNodeStorage* noder, GPUMemoryPool* memorypool, int32_t dev_id,
                  int32_t mode)
{
    (void)strm_hdl; (void)cache; (void)noder; (void)memorypool; (void)dev_id; (void)mode;
}

} // extern "C"

// =================================== Operator plugin API ============================================
struct Operator {
    virtual ~Operator() = default;
    virtual void run(OpParams* params) = 0;
};

namespace {

inline void record(OpParams* p)
{
    if (p->event) HIP_CHECK(hipEventRecord((hipEvent_t)p->event, (hipStream_t)p->stream));
}

class Batch_Generator : public Operator { // Operator.cu:10-31
public:
    explicit Batch_Generator(int op_id) : op_id_(op_id) {}
    void run(OpParams* params) override
    {
        GPUNodeStorage* noder = (GPUNodeStorage*)params->noder;
        GPUCache* cache = (GPUCache*)params->cache;
        GPUMemoryPool* memorypool = (GPUMemoryPool*)params->memorypool;
        int32_t mode = GPUMemoryPool_GetCurrentMode(memorypool);
        int32_t iter = GPUMemoryPool_GetIter(memorypool);
        IPCEnv* env = (IPCEnv*)params->env;
        int32_t device_id = params->device_id;
        int32_t batch_size = IPCEnv_GetCurrentBatchsize(env, device_id, mode);
        batch_generator_kernel(params->stream, noder, cache, memorypool, batch_size, iter, device_id, device_id, mode);
        record(params);
    }
private:
    [[maybe_unused]] int op_id_;
};

class Random_Sampler : public Operator { // Operator.cu:37-55
public:
    explicit Random_Sampler(int op_id) : op_id_(op_id) {}
    void run(OpParams* params) override
    {
        GPU_Random_Sampling(params->stream, (GPUGraphStorage*)params->graph, (GPUCache*)params->cache,
                            (GPUMemoryPool*)params->memorypool, params->neighbor_count, op_id_, params->is_presc);
        record(params);
    }
private:
    [[maybe_unused]] int op_id_;
};

class Feature_Extractor : public Operator { // Operator.cu:61-76 (records no event)
public:
    explicit Feature_Extractor(int op_id) : op_id_(op_id) {}
    void run(OpParams* params) override
    {
        get_feature_kernel(params->stream, (GPUCache*)params->cache, (GPUNodeStorage*)params->noder,
                           (GPUMemoryPool*)params->memorypool, params->device_id, op_id_, params->in_memory);
    }
private:
    [[maybe_unused]] int op_id_;
};

class Cache_Planner : public Operator { // Operator.cu:82-97
public:
    explicit Cache_Planner(int op_id) : op_id_(op_id) {}
    void run(OpParams* params) override
    {
        GPUMemoryPool* memorypool = (GPUMemoryPool*)params->memorypool;
        int mode = GPUMemoryPool_GetCurrentMode(memorypool);
        make_update_plan(params->stream, (GPUGraphStorage*)params->graph, (GPUCache*)params->cache, memorypool,
                         params->device_id, mode);
        record(params);
    }
private:
    [[maybe_unused]] int op_id_;
};

class Cache_Updater : public Operator { // Operator.cu:103-119
public:
    explicit Cache_Updater(int op_id) : op_id_(op_id) {}
    void run(OpParams* params) override
    {
        GPUMemoryPool* memorypool = (GPUMemoryPool*)params->memorypool;
        int mode = GPUMemoryPool_GetCurrentMode(memorypool);
        update_cache(params->stream, (GPUCache*)params->cache, (GPUNodeStorage*)params->noder, memorypool,
                     params->device_id, mode);
        record(params);
    }
private:
    [[maybe_unused]] int op_id_;
};

} // namespace

extern "C" {
Operator* NewBatchGenerator(int op_id) { return new Batch_Generator(op_id); }
Operator* NewRandomSampler(int op_id) { return new Random_Sampler(op_id); }
Operator* NewFeatureExtractor(int op_id) { return new Feature_Extractor(op_id); }
Operator* NewCachePlanner(int op_id) { return new Cache_Planner(op_id); }
Operator* NewCacheUpdater(int op_id) { return new Cache_Updater(op_id); }
void Operator_run(Operator* op, OpParams* params) { if (op && params) op->run(params); }
void Operator_Delete(Operator* op) { delete op; }
}
