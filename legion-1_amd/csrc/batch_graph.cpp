// batch_graph.cpp -- one mini-batch (S1..S5: seed, H x sampler, gathers, planner) recorded once as a
// hipGraph and replayed with a single launch per batch.
//
// The reference drives every batch from the host: ~(2H+4) operator launches, each with per-batch
// arguments (Server.cu:301-328).  Here the two values that change from batch to batch -- the batch
// cursor inside the seed list and the position-table epoch -- live in device memory (BatchCtl):
// k_seed<SELF> reads them, k_advance (the last node of the graph) steps them, so the recorded graph
// has no per-batch arguments at all.  The host keeps a mirror (batch_serial / ctl_counter) and only
// launches k_set_cursor when the next batch is not the successor of the previous graph launch
// (first batch, epoch / mode change, or after a host-driven batch on the same pool).  Under seeded sampling
// the batch's draw word lives there too: k_set_cursor and k_advance form it from the round's key and the cursor,
// so a new round (GPUMemoryPool_BeginRound) needs no new recording.
#include "internal.h"

#include "audit_hooks.h"

using namespace legion;

struct LegionBatchGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    GPUMemoryPool* pool = nullptr;
    // what the recording left in the pool's per-batch host state (launchers called behind a replay decide from it, like behind the plain calls)
    GPUMemoryPool::Progress progress;
    // The serving modes the batch was recorded in (the pool refuses to change them during a recording).  A replay is refused only when the
    // pool's seeded state is another by now: the captured k_seed holds list pointers -- the seed set's, or the pool's shuffled copy (shuf_ids,
    // when the recording read it) --, so the graph only replays in that state; the seed, the round and the counter are not part of it
    // (k_set_cursor carries them into ctl).  Likewise for lp_draw: the captured k_seed is the instantiation, the k and the row tables of that state;
    // and for weighted_distinct: the captured k_sample is that state's instantiation, over the alias table or over the retained weights;
    // and for shared_draws: the captured k_sample is that state's instantiation; and for edge_ids: the captured hops park their columns and
    // launch k_edge_ids, or do neither; and for agg_edge_weight: a captured get_feature_kernel_agg ranks the draws' edge weights and sums
    // with them, or sums plainly.
    // and for edge_feat_dim: a captured get_edge_feature_kernel holds that row width and the pipe's edge_feat buffer of that width, which
    // another width reallocates (writes_edge_feat: the recording gathered edge rows, under the pool's allocation count edge_feat_gen; pipe: the one it ran on).
    // and for lp_exclude: a captured batch holds k_lp_pairs and k_lp_edge_keep with that k and the pipe's pair table of that capacity, which a k
    // of another capacity reallocates (uses_lp: the recording built or read the table, under the pool's allocation count lp_gen), or neither launch.
    ServeModes modes;
    const int32_t* shuf_ids = nullptr;
    int32_t pipe = 0;
    bool writes_edge_feat = false;
    uint32_t edge_feat_gen = 0;
    bool uses_lp = false;
    uint32_t lp_gen = 0;
};
// The replay rule, one row per mode field a recording is bound to (the comment above says why), compared in this order: the field's state, and
// the refusal when the recording had it on / had it off.  A field without a row (sampling, agg_last_hop, agg_norm, seed) is not compared.
struct ReplayRule { int32_t (*state)(const ServeModes&); const char *recorded_on, *recorded_off; };
constexpr ReplayRule kReplayRules[] = {
    {[](const ServeModes& m) -> int32_t { return m.seeded; }, "LegionBatchGraph_Launch: the graph was recorded under a seed (GPUMemoryPool_SetSampleSeed) and the pool is unseeded now: its k_seed holds the shuffled list's pointers -- record it again", "LegionBatchGraph_Launch: the graph was recorded unseeded and the pool is seeded now (GPUMemoryPool_SetSampleSeed): its k_seed holds the file-order list's pointers -- record it again"},
    {[](const ServeModes& m) -> int32_t { return m.lp_draw; }, "LegionBatchGraph_Launch: the graph was recorded with drawn link-prediction thirds (GPUMemoryPool_SetLpDraw) and the pool is in another lp_draw state now: its k_seed draws the thirds for that k -- record it again", "LegionBatchGraph_Launch: the graph was recorded without drawn link-prediction thirds and the pool draws them now (GPUMemoryPool_SetLpDraw): its k_seed reads all three thirds from the list -- record it again"},
    {[](const ServeModes& m) -> int32_t { return m.weighted_distinct; }, "LegionBatchGraph_Launch: the graph was recorded with weighted sampling without replacement (GPUMemoryPool_SetWeightedDistinct) and the pool has the flag off now: its k_sample is that mode's instantiation -- record it again", "LegionBatchGraph_Launch: the graph was recorded without weighted sampling without replacement and the pool has the flag on now (GPUMemoryPool_SetWeightedDistinct): its k_sample is another instantiation -- record it again"},
    {[](const ServeModes& m) -> int32_t { return m.shared_draws; }, "LegionBatchGraph_Launch: the graph was recorded with shared-key sampling (GPUMemoryPool_SetSharedDraws) and the pool has the flag off now: its k_sample is that mode's instantiation -- record it again", "LegionBatchGraph_Launch: the graph was recorded without shared-key sampling and the pool has the flag on now (GPUMemoryPool_SetSharedDraws): its k_sample is another instantiation -- record it again"},
    {[](const ServeModes& m) -> int32_t { return m.edge_ids; }, "LegionBatchGraph_Launch: the graph was recorded with edge ids (GPUMemoryPool_SetEdgeIds) and the pool has the mode off now: its hops park their columns and launch k_edge_ids -- record it again", "LegionBatchGraph_Launch: the graph was recorded without edge ids and the pool has the mode on now (GPUMemoryPool_SetEdgeIds): its hops leave no edge ids behind -- record it again"},
    {[](const ServeModes& m) -> int32_t { return m.agg_edge_weight; }, "LegionBatchGraph_Launch: the graph was recorded with edge-weighted sums (GPUMemoryPool_SetAggEdgeWeight) and the pool has the flag off now: its last hop is summed by k_draw_edge_weights and the weighted k_gather_sum -- record it again", "LegionBatchGraph_Launch: the graph was recorded without edge-weighted sums and the pool has the flag on now (GPUMemoryPool_SetAggEdgeWeight): its last hop is summed unweighted -- record it again"},
    {[](const ServeModes& m) -> int32_t { return m.edge_feat_dim; }, "LegionBatchGraph_Launch: the graph was recorded gathering edge features (GPUMemoryPool_SetEdgeFeatures) and the pool is at another row width, or has the mode off, now: its k_gather_edges holds that width and that buffer -- record it again", "LegionBatchGraph_Launch: the graph was recorded without edge features and the pool gathers them now (GPUMemoryPool_SetEdgeFeatures): it leaves no edge rows behind -- record it again"},
    {[](const ServeModes& m) -> int32_t { return m.lp_exclude; }, "LegionBatchGraph_Launch: the graph was recorded with target-edge exclusion (GPUMemoryPool_SetLpExclude) and the pool is in another lp_exclude state now: its k_lp_pairs and k_lp_edge_keep hold that k and that pair table -- record it again", "LegionBatchGraph_Launch: the graph was recorded without target-edge exclusion and the pool marks target edges now (GPUMemoryPool_SetLpExclude): it leaves no edge_keep behind -- record it again"}};

extern "C" {

int GPUMemoryPool_BeginBatchCapture(GPUMemoryPool* p, void* stream)
{
    if (!p || !p->owns_scratch || !p->ctl) { LEGION_ARG_ERROR("BeginBatchCapture: GPUMemoryPool_AllocateScratch was not called"); return -1; }
    if (p->capturing) { LEGION_ARG_ERROR("BeginBatchCapture: a capture is already running on this pool"); return -1; }
    if (!stream) { LEGION_ARG_ERROR("BeginBatchCapture: the legacy null stream cannot be captured"); return -1; }
    warm_static_tables(); // no allocation / copy may happen between Begin and End
    HIP_CHECK(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
    if (error_pending()) return -1;
    p->capturing = true;
    return 0;
}

LegionBatchGraph* GPUMemoryPool_EndBatchCapture(GPUMemoryPool* p, void* stream)
{
    if (!p || !p->capturing) { LEGION_ARG_ERROR("EndBatchCapture: no capture is running on this pool"); return nullptr; }
    launch_advance((hipStream_t)stream, p->ctl);
    p->capturing = false;
    LegionBatchGraph* g = new LegionBatchGraph();
    g->pool = p;
    g->progress = p->progress;
    g->modes = p->modes; g->shuf_ids = p->seed_reads_shuffle ? p->shuf_ids : nullptr;
    g->pipe = p->current_pipe; g->writes_edge_feat = p->progress.edge_feat_gathered; g->edge_feat_gen = p->edge_feat_gen;
    g->uses_lp = p->progress.lp_pairs_built || p->progress.lp_marked; g->lp_gen = p->lp_gen;
    HIP_CHECK(hipStreamEndCapture((hipStream_t)stream, &g->graph));
    if (g->graph) HIP_CHECK(hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0));
    if (!g->exec || error_pending()) {
        if (g->graph) (void)hipGraphDestroy(g->graph);
        delete g;
        return nullptr;
    }
    return g;
}

// Run the recorded batch for seed-list position `counter` (what batch_generator_kernel's `counter` is).
int LegionBatchGraph_Launch(LegionBatchGraph* g, void* stream, int32_t counter)
{
    if (!g || !g->exec || !g->pool || !g->pool->ctl) { LEGION_ARG_ERROR("LegionBatchGraph_Launch: null graph"); return -1; }
    GPUMemoryPool* p = g->pool;
    if (p->capturing) { LEGION_ARG_ERROR("LegionBatchGraph_Launch: pool is being captured"); return -1; }
    for (const ReplayRule& r : kReplayRules)
        if (r.state(g->modes) != r.state(p->modes)) { LEGION_ARG_ERROR(r.state(g->modes) ? r.recorded_on : r.recorded_off); return -1; }
    if (g->shuf_ids && (g->shuf_ids != p->shuf_ids || !p->shuf_valid)) {
        LEGION_ARG_ERROR("LegionBatchGraph_Launch: the graph reads the pool's shuffled training list, which GPUMemoryPool_BeginRound has not filled for this seed and round (or has reallocated: record the graph again)");
        return -1;
    }
    if (g->writes_edge_feat && g->edge_feat_gen != p->edge_feat_gen) {
        LEGION_ARG_ERROR("LegionBatchGraph_Launch: the graph writes an edge-feature buffer the pool has reallocated since (GPUMemoryPool_SetEdgeFeatures with another row width in between): record it again");
        return -1;
    }
    if (g->uses_lp && g->lp_gen != p->lp_gen) {
        LEGION_ARG_ERROR("LegionBatchGraph_Launch: the graph uses a pair table of target-edge exclusion the pool has reallocated since (GPUMemoryPool_SetLpExclude with a k of another table capacity in between): record it again");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    if (++p->batch_serial >= kSerialLimit) { // epoch space exhausted: wipe once and start over (as batch_generator_kernel)
        HIP_CHECK(hipMemsetAsync(p->pos_map, 0xFF, (size_t)p->V * sizeof(pos_t), s));
        p->batch_serial = 1;
        p->ctl_synced = false;
    }
    if (!p->ctl_synced || p->ctl_counter != counter) launch_set_cursor(s, p->ctl, counter, kEpochTop - p->batch_serial, p->modes.seeded ? 1u : 0u, p->modes.seeded ? seeded_draw_key(p->modes.seed, p->round) : 0u);
    HIP_CHECK(hipGraphLaunch(g->exec, s));
    // the batch now in flight is the recorded one: what the launchers behind it (get_feature_kernel_agg) decide from
    p->progress = g->progress;
    p->pipes[g->pipe].edge_feat_filled = g->progress.edge_feat_gathered;
    p->pipes[g->pipe].lp_marked = g->progress.lp_marked;
    p->ctl_synced = true;     // k_advance left (counter + 1, next epoch) in ctl
    p->ctl_counter = counter + 1;
    return error_pending() ? -1 : 0;
}

void LegionBatchGraph_Delete(LegionBatchGraph* g)
{
    if (!g) return;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
}

} // extern "C"
