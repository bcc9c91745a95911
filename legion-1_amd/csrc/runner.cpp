// runner.cpp -- per-GPU pipeline driver:
//   GPURunner   src/Server.cu:163-369   (a batch by stage, 2 streams + events, RunPreSc / RunOnce)
#include "internal.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

#include "audit_hooks.h"

using namespace legion;

struct Runner {
    int32_t num_ids = 0, float_attr_len = 0;
    GPUMemoryPool* memorypool = nullptr;
    int current_pipe = 0, pipeline_depth = LEGION_PIPELINE_DEPTH, local_dev_id = 0, mode = 0, hops = 0;
    // what the stages of a batch take, as Runner_Initialize was given it
    GPUCache* cache = nullptr; GPUGraphStorage* graph = nullptr; GPUNodeStorage* noder = nullptr; IPCEnv* env = nullptr;
    int32_t fanout[LEGION_MAX_HOPS] = {}, in_memory = 0;
    // streams[0]: the sampler side (seed launch, hops, planner), streams[1]: the gathers.  level_ev[l]: behind the seed launch (l = 0) or hop l
    hipStream_t streams[2] = {nullptr, nullptr};
    hipEvent_t level_ev[LEGION_MAX_HOPS + 1] = {}, plan_ev = nullptr;
    // $LEGION_BATCH_GRAPH=1: the sampler side of a batch (seed launch, hops, planner) is replayed as ONE recorded hipGraph per (pipe, mode)
    // on stream 0 and the rows are gathered by one plain launch on stream 1 behind it -- for launch-bound hosts / small batches
    // (-8 % / -5 % per batch at 0.3 x products, a tie at the BASELINE shapes: profiles/r04_graph_trace.md).  The whole batch as one graph
    // (one stream: loses the gather / sampler overlap; fork / join: 38-42 us of idle per batch on this runtime) lost to it at every shape and
    // is no longer a runner mode (profiles/r06_removed_experiments.patch); GPUMemoryPool_Begin/EndBatchCapture still record any op list.
    bool use_graph = false;
    // RunOnce is software-pipelined: the host enqueues batch i and only then waits for batch i-1 and posts its pipe, so the sampler of
    // batch i (stream 0) overlaps the gathers of batch i-1 (stream 1) on the GPU.  (The reference's synchronous loop, Server.cu:301-328,
    // waits for batch i before it looks at batch i+1.)
    // $LEGION_RUNNER_GATHER = auto (default) | level | all.  level: one get_feature_kernel per level on stream 1 behind each hop (the reference's
    // op list, Server.cu:198-207).  all: ONE gather over all rows behind the last hop (get_feature_kernel_all).  Same bytes in the same buffer.
    // Which is faster depends on the shape (profiles/r05_runner_gather.md, served batches, same box): when the gather outweighs the sampler the
    // single launch wins (papers100M {25,10,5} -2.8 %, products {25,10} -4 %), when the sampler outweighs it the per-level gathers hide behind the
    // long hops (products {25,10,5}: `all` +5.7 %).  auto decides once, after the pre-sampling epoch, from the last pre-sampled batch's counters.
    bool gather_all = false;
    bool gather_auto = true;
    // What the environment asked for (serve_modes_from_env; ServeModes in internal.h).  Aggregated last hop: get_feature_kernel_agg on stream 1
    // behind the last hop instead of the last level's gather; the feature buffers then hold n_in + N rows per batch, not n.
    ServeModes modes;
    // Seeded sampling.  round: the one the pool was last told (GPUMemoryPool_BeginRound), -1 = none yet.  lists_verbatim: the training
    // lists are served as they are (meta flag 2, link-prediction thirds): never shuffled, draws still seeded -- unless modes.lp_draw has
    // their triples shuffled and the pos / neg thirds drawn per batch.
    int32_t round = -1;
    bool lists_verbatim = false;
    int32_t presc_max_rows = 0;     // largest n_in + N of the pre-sampling epoch (read back per batch: that epoch is not pipelined anyway)
    bool pending = false;
    int pending_pipe = 0;
    int64_t short_batches = 0;      // batches with more nodes than the feature buffers hold rows (see hand_over)
    hipEvent_t done_ev[LEGION_PIPELINE_DEPTH] = {};
    LegionBatchGraph* graphs[LEGION_PIPELINE_DEPTH][3] = {};
};

// Seeded sampling: tell the pool the round, on the stream the batch generator runs on (the shuffled copy is refilled in front of the round's
// first k_seed and behind the last one of the round before).
static void begin_round(Runner* r, GPUNodeStorage* noder, int32_t round)
{
    if (!r->modes.seeded || r->round == round) return;
    const bool file_order = r->lists_verbatim && !r->modes.lp_draw;
    if (r->modes.lp_draw && r->round < 0)
        log_out() << r->local_dev_id << " Drawn link-prediction thirds: " << r->modes.lp_draw << " triples per batch (LEGION_LP_DRAW=1): the triples reshuffled per epoch, pos and neg drawn per batch\n";
    else if (file_order && r->round < 0)
        log_out() << r->local_dev_id << " Seeded sampling: the training lists are served verbatim (meta flag 2): not shuffled, the draws are seeded\n";
    GPUMemoryPool_BeginRound(r->streams[0], r->memorypool, file_order ? nullptr : noder, r->local_dev_id, round);
    r->round = round;
}

// Post a finished batch to its trainer.  The feature buffers hold a bounded number of rows (Runner_InitializeFeaturesBuffer: 1.2 x the
// largest batch of the pre-sampling epoch, Server.cu:275); the gather never writes past them, so a batch that reached more nodes arrives
// with its last rows missing and ipc_service.get_next refuses it (the reference's trainer reads past the allocation instead,
// ipc_cuda_kernel.cu:200).  That is a trainer-side failure with no server-side trace -- so the server leaves one: the first such batch
// is logged, all are counted (Runner_Finalize prints the total).
static void hand_over(Runner* r, IPCEnv* env, int pipe)
{
    const int32_t rows = r->memorypool ? r->memorypool->feature_rows : 0;
    int32_t nodes = IPCEnv_MirroredNodeCounter(env, r->local_dev_id, pipe, legion_idx_nodes_through(r->hops));
    if (r->modes.agg_last_hop && nodes >= 0) {     // the mirror is there: n_in + N rows (features, then one row of sums per input slot of the last hop)
        int32_t nc[LEGION_COUNTER_WORDS], ec[LEGION_COUNTER_WORDS];
        for (int i = 0; i < LEGION_COUNTER_WORDS; i++) { nc[i] = IPCEnv_MirroredNodeCounter(env, r->local_dev_id, pipe, i); ec[i] = IPCEnv_MirroredNodeCounter(env, r->local_dev_id, pipe, LEGION_COUNTER_WORDS + i); }
        nodes = legion_agg_rows(nc, ec, r->hops);
    }
    if (rows > 0 && nodes > rows) {
        if (r->short_batches++ == 0)
            log_out() << r->local_dev_id << " Feature buffer too small: a batch has " << nodes << (r->modes.agg_last_hop ? " rows (features + neighbour sums)" : " nodes") << ", the buffer holds " << rows
                      << " rows -- the rows beyond it are not gathered and the trainer will refuse the batch (evaluation batches larger than "
                         "the training batches of the pre-sampling epoch?)\n" << std::flush;
    }
    IPCEnv_IPCPost(env, r->local_dev_id, pipe);
}

static void advance_pipe(Runner* r)
{
    r->current_pipe = (r->current_pipe + 1) % r->pipeline_depth;
    GPUMemoryPool_SetCurrentPipe(r->memorypool, r->current_pipe);
}

// Wait for the trainer to free the current pipe.  Pipelined loop (batch i-1 in flight): hand batch i-1 over the moment it is complete --
// a trainer that is the bottleneck must not wait for our next enqueue.
// Poll first (IPCEnv_HandoffSpinUs, 200 us): the trainer usually frees the pipe within tens of microseconds of the post at the
// end of the previous RunOnce, and a sleep_for(10 us) really sleeps 60+ us (timer slack) -- on the critical chain of every batch
// (gather i-1 done -> post -> trainer -> pipe free -> sampler i+1 may start).  After the polling budget: sleep between looks, as before.
static void wait_for_pipe(Runner* r, IPCEnv* env)
{
    if (!r->pending) {
        IPCEnv_IPCWait(env, r->local_dev_id, r->current_pipe);
        return;
    }
    const auto t_wait = std::chrono::steady_clock::now();
    const auto spin = std::chrono::microseconds(IPCEnv_HandoffSpinUs());
    while (IPCEnv_IPCTryWait(env, r->local_dev_id, r->current_pipe, 0) != 0) {
        if (hipEventQuery(r->done_ev[r->pending_pipe]) == hipSuccess) {
            hand_over(r, env, r->pending_pipe);
            r->pending = false;
            IPCEnv_IPCWait(env, r->local_dev_id, r->current_pipe);
            break;
        }
        if (std::chrono::steady_clock::now() - t_wait < spin) { for (int i = 0; i < 64; i++) __builtin_ia32_pause(); }
        else std::this_thread::sleep_for(std::chrono::microseconds(10));
    }
}

// LEGION_ERR_RETURN (embedding / tests) and a failed batch: never leave a trainer blocked on sem_w.  The batch in flight
// is handed over as usual; the failed pipe is posted with nc[LEGION_NC_TOTAL] = -1 (every counter word 0xFFFFFFFF), which no valid
// batch produces -- a consumer must treat it as "server failed" (the reference's behaviour, exit(EXIT_FAILURE), is what
// the default LEGION_ERR_EXIT mode does instead).
static void post_poisoned(Runner* r, IPCEnv* env)
{
    if (r->pending) {
        (void)hipEventSynchronize(r->done_ev[r->pending_pipe]);
        hand_over(r, env, r->pending_pipe);
        r->pending = false;
    }
    (void)hipDeviceSynchronize();
    int32_t* nc = IPCEnv_GetNodeCounter(env, r->local_dev_id, r->current_pipe);
    if (nc) (void)hipMemset(nc, 0xFF, LEGION_COUNTER_WORDS * sizeof(int32_t));
    int32_t* ec = IPCEnv_GetEdgeCounter(env, r->local_dev_id, r->current_pipe);   // no stale edge counts of the pipe's previous batch
    if (ec) (void)hipMemset(ec, 0, LEGION_COUNTER_WORDS * sizeof(int32_t));
    IPCEnv_SetMirror(env, r->local_dev_id, r->current_pipe, -1, 0);
    (void)hipGetLastError();
    IPCEnv_IPCPost(env, r->local_dev_id, r->current_pipe);
    advance_pipe(r);
}

// What goes to the gather stream behind level l (l == hops: behind the last hop).  `want` is what the caller serves: None (pre-sampling, a
// recording), Level (each level's rows behind its hop) or All (every row with one launch behind the last hop: the levels below it are not
// gathered and their events not waited for).  The aggregated hand-off takes the last level's place and gathers what was not gathered per level.
enum class Gather { None, Level, All, Agg };
static Gather gather_behind(const Runner* r, int l, Gather want)
{
    if (want == Gather::None) return Gather::None;
    if (l < r->hops) return want == Gather::All ? Gather::None : Gather::Level;
    return r->modes.agg_last_hop ? Gather::Agg : want;
}

// ... and its launch, behind a wait for `behind` (recorded on the sampler stream)
static void enqueue_gather(Runner* r, int l, Gather want, hipEvent_t behind)
{
    const Gather what = gather_behind(r, l, want);
    if (what == Gather::None) return;
    HIP_CHECK(hipStreamWaitEvent(r->streams[1], behind, 0));
    if (what == Gather::Agg) get_feature_kernel_agg(r->streams[1], r->cache, r->noder, r->memorypool, r->local_dev_id, r->in_memory);
    else if (what == Gather::All) get_feature_kernel_all(r->streams[1], r->cache, r->noder, r->memorypool, r->local_dev_id, r->in_memory);
    else get_feature_kernel(r->streams[1], r->cache, r->noder, r->memorypool, r->local_dev_id, 2 * l + 1, r->in_memory);   // the launcher's op_id of level l
}

// A batch: the seed launch (level 0), hop 1 .. hop H, the planner on `sampler`; behind each level its event (when `record`) and, on the
// gather stream, what gather_behind says.  The host issues them interleaved, so a level's gather reaches its stream before the next hop
// reaches the sampler's.  A runner that was never initialised enqueues nothing.  A pool in the edge-id mode (LEGION_EDGE_IDS=1, or
// GPUMemoryPool_SetEdgeIds on Runner_GetMemoryPool) has every hop's GPU_Random_Sampling enqueue k_edge_ids behind its k_write, in front of the
// level's event: in-process runners and recordings leave the pipe's edge ids like the plain calls do.
static void enqueue_stages(Runner* r, hipStream_t sampler, bool presc, bool record, Gather want)
{
    GPUMemoryPool* pool = r->memorypool;
    if (!pool) return;
    const int32_t dev = r->local_dev_id, mode = GPUMemoryPool_GetCurrentMode(pool);
    for (int l = 0; l <= r->hops; l++) {
        if (l == 0) batch_generator_kernel(sampler, r->noder, r->cache, pool, IPCEnv_GetCurrentBatchsize(r->env, dev, mode), GPUMemoryPool_GetIter(pool), dev, dev, mode);
        else GPU_Random_Sampling(sampler, r->graph, r->cache, pool, r->fanout[l - 1], 2 * l, presc);   // the launcher's op_id of hop l
        if (record) HIP_CHECK(hipEventRecord(r->level_ev[l], sampler));
        enqueue_gather(r, l, want, r->level_ev[l]);
    }
    make_update_plan(sampler, r->graph, r->cache, pool, dev, mode);
    if (record) HIP_CHECK(hipEventRecord(r->plan_ev, sampler));
}

// $LEGION_BATCH_GRAPH=1 (see Runner::use_graph): the recorded sampler side of (pipe, mode) on stream 0 -- recorded on first use --, then
// all rows gathered on stream 1 behind it, whatever gather_all says.  False when the recording failed.
static bool run_graph(Runner* r, IPCEnv* env, int32_t batch_id)
{
    LegionBatchGraph*& g = r->graphs[r->current_pipe][r->mode];
    if (!g) { // record this (pipe, mode) once
        if (GPUMemoryPool_BeginBatchCapture(r->memorypool, r->streams[0]) == 0) {
            // the sampler side only, on ONE stream; the rows are gathered by one plain launch on stream 1 behind the graph, so the
            // gather of batch i overlaps the recorded sampler of batch i + 1 (the other pipe)
            enqueue_stages(r, r->streams[0], false, false, Gather::None);
            g = GPUMemoryPool_EndBatchCapture(r->memorypool, r->streams[0]);
        }
        if (!g) return false;
    }
    LegionBatchGraph_Launch(g, r->streams[0], IPCEnv_GetLocalBatchId(env, batch_id));
    HIP_CHECK(hipEventRecord(r->plan_ev, r->streams[0]));
    enqueue_gather(r, r->hops, Gather::All, r->plan_ev);
    return true;
}

// $LEGION_RUNNER_GATHER=auto: one-off estimate from the last batch of the pre-sampling epoch (its counters are still in pipe 0): sampler ~ 45 ps
// per slot (the memory system's random-access rate: 54 ps at papers100M, 43 ps at products {25,10,5}), gather ~ rows x (8F + 8) bytes at 6 TB/s
// (5.2 TB/s for rows that are not whole 128-byte lines).  A wrong guess costs a few per cent, never correctness.
static void choose_gather(Runner* r, GPUCache* cache, IPCEnv* env, const int32_t* fanout)
{
    int32_t nc[LEGION_COUNTER_WORDS] = {0}, ec[LEGION_COUNTER_WORDS] = {0};
    const int32_t* dnc = IPCEnv_GetNodeCounter(env, r->local_dev_id, 0);
    const int32_t* dec = IPCEnv_GetEdgeCounter(env, r->local_dev_id, 0);
    if (!(dnc && dec && hipMemcpy(nc, dnc, sizeof(nc), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(ec, dec, sizeof(ec), hipMemcpyDeviceToHost) == hipSuccess)) {
        (void)hipGetLastError();
        return;
    }
    double slots = 0.0;
    for (int h = 1; h <= r->hops; h++) slots += (double)legion_hop_inputs(nc, ec, h) * (double)fanout[h - 1];
    const double rows = (double)GPUCache_MaxIdNum(cache, r->local_dev_id);
    double gather_us = 0.0, sampler_us = 0.0;
    (void)legion_runner_gather_estimate(r->float_attr_len, rows, slots, &gather_us, &sampler_us);
    r->gather_all = gather_us > sampler_us;
    log_out() << r->local_dev_id << " Runner gather: " << (r->gather_all ? "one launch over all rows behind the last hop" : "per level behind each hop")
              << " (estimated gather " << (int)gather_us << " us, sampler " << (int)sampler_us << " us per batch)\n";
}

void legion::runner_set_lists_verbatim(Runner* r, bool verbatim) { r->lists_verbatim = verbatim; }

extern "C" {

// The estimate behind $LEGION_RUNNER_GATHER=auto (see Runner::gather_all): microseconds per batch of the gather (rows x (8F + 8) bytes at
// 6 TB/s, 5.2 TB/s for rows that are not whole 128-byte lines) and of the sampler (45 ps per slot: the memory system's random-access rate).
// Returns 1 when one gather over all rows behind the last hop is expected to win, 0 for the reference's per-level list.
int legion_runner_gather_estimate(int32_t F, double rows, double slots, double* gather_us, double* sampler_us)
{
    const double g = rows * (8.0 * F + 8.0) / (((F * 4) % 128 == 0) ? 6.0e6 : 5.2e6), smp = slots * 45e-6;
    if (gather_us) *gather_us = g;
    if (sampler_us) *sampler_us = smp;
    return g > smp ? 1 : 0;
}

Runner* NewGPURunner(void) { return new Runner(); }

// GPURunner::Initialize, Server.cu:169-271
void Runner_Initialize(Runner* r, RunnerParams* params)
{
    if (!r || !params || !params->fanout || params->hops < 1 || params->hops > LEGION_MAX_HOPS) { LEGION_ARG_ERROR("Runner_Initialize: bad arguments"); return; }
    std::string why;
    if (!serve_modes_from_env(r->modes, why)) { LEGION_ARG_ERROR(("Runner_Initialize: " + why).c_str()); return; }
    r->local_dev_id = params->device_id;
    IPCEnv* env = (IPCEnv*)params->env;
    if (!serve_modes_resolve_lp_draw(r->modes, r->lists_verbatim, r->modes.lp_draw && env ? IPCEnv_GetRawBatchsize(env) : 0, why)) { LEGION_ARG_ERROR(("Runner_Initialize: " + why).c_str()); return; }
    DeviceGuard guard(r->local_dev_id);
    GPUCache* cache = (GPUCache*)params->cache;
    GPUNodeStorage* noder = (GPUNodeStorage*)params->noder;
    HIP_CHECK(hipStreamCreateWithFlags(&r->streams[0], hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&r->streams[1], hipStreamNonBlocking));
    // the pool serves train, validation and test batches: size it for the largest of the three (the per-GPU
    // validation / test batch, CUDA_IPC_Service.cu:101-118, can exceed a small raw batch size)
    int batch_size = IPCEnv_GetRawBatchsize(env);
    batch_size = std::max(batch_size, IPCEnv_GetCurrentBatchsize(env, r->local_dev_id, LEGION_VALIDMODE));
    batch_size = std::max(batch_size, IPCEnv_GetCurrentBatchsize(env, r->local_dev_id, LEGION_TESTMODE));
    const int hop_num = params->hops;
    r->hops = hop_num;
    r->cache = cache; r->graph = (GPUGraphStorage*)params->graph; r->noder = noder; r->env = env; r->in_memory = params->in_memory;
    std::copy(params->fanout, params->fanout + hop_num, r->fanout);
    r->pipeline_depth = LEGION_PIPELINE_DEPTH;
    { const char* e = getenv("LEGION_BATCH_GRAPH"); r->use_graph = e && atoi(e) != 0; }
    { const char* e = getenv("LEGION_RUNNER_GATHER"); r->gather_all = e && strcmp(e, "all") == 0; r->gather_auto = !e || strcmp(e, "auto") == 0; }
    for (auto& ev : r->done_ev) HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    for (int l = 0; l <= hop_num; l++) HIP_CHECK(hipEventCreateWithFlags(&r->level_ev[l], hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&r->plan_ev, hipEventDisableTiming));
    const int total_num_nodes = GPUNodeStorage_TotalNodeNum(noder);
    GPUCache_InitializeCacheController(cache, r->local_dev_id, total_num_nodes);
    r->memorypool = NewGPUMemoryPool(r->pipeline_depth);
    GPUMemoryPool_AllocateScratch(r->memorypool, total_num_nodes, batch_size, params->fanout, hop_num);
    // before the pre-sampling epoch (the hotness profile sees what will be served): the pool's modes, their buffers on this runner's GPU; what a trainer reads
    const ServeModes& m = r->modes;
    r->memorypool->lp_graph = m.lp_draw ? (GPUGraphStorage*)params->graph : nullptr;   // the positives' rows (GPUMemoryPool_SetLpDraw keeps it the same way)
    pool_apply_modes(r->memorypool, m, "Runner_Initialize");
    ipc_env_publish_modes(env, m);
    if (m.agg_last_hop) log_out() << r->local_dev_id << " Hand-off: the last hop as neighbour sums (LEGION_AGG_LAST_HOP=1)\n";
    if (m.agg_norm) log_out() << r->local_dev_id << " Hand-off: the sums normalised by out-degree^-1/2 inside block 1 (LEGION_AGG_NORM=both)\n";
    if (m.agg_edge_weight) log_out() << r->local_dev_id << " Hand-off: the sums scaled by each edge's weight (LEGION_AGG_EDGE_WEIGHT=1)\n";
    if (m.edge_ids) {
        // the pool's per-pipe edge buffers go to the trainers as they are: the pool stays their owner, the env exports their handles.  A pipe
        // is posted behind done_ev, which stream 1 records behind plan_ev / the last level's event -- both behind the last hop's k_edge_ids
        for (int i = 0; i < r->pipeline_depth; i++) {
            const GPUMemoryPool::Pipe& pipe = r->memorypool->pipes[i];
            IPCEnv_RegisterEdgeBuffers(env, r->local_dev_id, i, pipe.buf<int64_t>(GPUMemoryPool::kEdgeIds), pipe.buf<float>(GPUMemoryPool::kEdgeW), GPUMemoryPool_NumIds(r->memorypool));
        }
        log_out() << r->local_dev_id << " Hand-off: every sampled edge's position in the whole CSR, " << GPUMemoryPool_NumIds(r->memorypool) << " per pipe (LEGION_EDGE_IDS=1)\n";
        if (serve_modes_edge_w_filled(m)) log_out() << r->local_dev_id << " Hand-off: every sampled edge's weight beside its id (" << (m.edge_weights ? "LEGION_EDGE_WEIGHTS=1" : "LEGION_WEIGHTED_DISTINCT=1") << ")\n";
    }
    log_out() << r->local_dev_id << " Sampling: " << draw_rule_facts(draw_rule_of(m)).sentence << "\n";
    if (m.seeded) log_out() << r->local_dev_id << " Sampling seed: " << m.seed << " (LEGION_SAMPLING_SEED): fresh draws per batch, the training list reshuffled per epoch\n";
    LEGION_AUDIT_OWNER(r->memorypool->pos_map, r->local_dev_id, "Runner_Initialize: scratch of the memory pool");
    LEGION_AUDIT_STREAM(r->streams[0], r->local_dev_id, "Runner_Initialize: sampler stream");
    LEGION_AUDIT_STREAM(r->streams[1], r->local_dev_id, "Runner_Initialize: gather stream");
    r->memorypool->device_id = r->local_dev_id;
    r->num_ids = GPUMemoryPool_NumIds(r->memorypool);
    r->float_attr_len = GPUNodeStorage_GetFloatAttrLen(noder);
    IPCEnv_InitializeSamplesBuffer(env, batch_size, r->num_ids, r->float_attr_len, r->local_dev_id, r->pipeline_depth);
    IPCEnv_SetHops(env, hop_num);
    r->current_pipe = 0;
    for (int i = 0; i < r->pipeline_depth; i++) {
        GPUMemoryPool_SetSampledIds(r->memorypool, IPCEnv_GetIds(env, r->local_dev_id, i), i);
        GPUMemoryPool_SetLabels(r->memorypool, IPCEnv_GetLabels(env, r->local_dev_id, i), i);
        GPUMemoryPool_SetAggSrcOf(r->memorypool, IPCEnv_GetAggSrc(env, r->local_dev_id, i), i);
        GPUMemoryPool_SetAggDstOf(r->memorypool, IPCEnv_GetAggDst(env, r->local_dev_id, i), i);
        GPUMemoryPool_SetNodeCounter(r->memorypool, IPCEnv_GetNodeCounter(env, r->local_dev_id, i), i);
        GPUMemoryPool_SetEdgeCounter(r->memorypool, IPCEnv_GetEdgeCounter(env, r->local_dev_id, i), i);
    }
}

// InitializeFeaturesBuffer, Server.cu:273-282: 1.2 x the largest batch seen while pre-sampling.
// Clamped to the static bound; the gather never writes beyond the buffer (rows are clamped).
void Runner_InitializeFeaturesBuffer(Runner* r, RunnerParams* params)
{
    GPUCache* cache = (GPUCache*)params->cache;
    IPCEnv* env = (IPCEnv*)params->env;
    DeviceGuard guard(r->local_dev_id);
    HIP_CHECK(hipStreamSynchronize(r->streams[0]));
    // aggregated hand-off: the buffer holds n_in + N rows per batch (largest of the pre-sampling epoch), same 1.2 x and seed-ratio rules
    int64_t num_ids = (int64_t)((r->modes.agg_last_hop ? r->presc_max_rows : GPUCache_MaxIdNum(cache, r->local_dev_id)) * 1.2);
    // The pre-sampling epoch only sees TRAINING batches.  A validation / test batch (up to 512 seeds per GPU, CUDA_IPC_Service.cu:101-118)
    // that is larger than the training batch reaches more nodes: scale the estimate by the seed ratio (unique nodes grow at most linearly
    // with the seeds).  The reference sizes by the training batches alone (Server.cu:275) -- with its 8000-seed training batches the case
    // does not arise; with a small --train_batch_size its trainer would read past the buffer.
    {
        const int raw = std::max(1, IPCEnv_GetRawBatchsize(env));
        const int eval = std::max(IPCEnv_GetCurrentBatchsize(env, r->local_dev_id, LEGION_VALIDMODE), IPCEnv_GetCurrentBatchsize(env, r->local_dev_id, LEGION_TESTMODE));
        if (eval > raw) num_ids = (int64_t)((double)num_ids * (double)eval / (double)raw);
    }
    if (num_ids > r->num_ids) num_ids = r->num_ids;
    if (num_ids < 1) num_ids = r->num_ids;
    if (r->gather_auto) choose_gather(r, cache, env, params->fanout);
    IPCEnv_InitializeFeaturesBuffer(env, 0, (int32_t)num_ids, r->float_attr_len, r->local_dev_id, r->pipeline_depth);
    for (int i = 0; i < r->pipeline_depth; i++)
        GPUMemoryPool_SetFloatFeatures(r->memorypool, IPCEnv_GetFloatFeatures(env, r->local_dev_id, i), i);
    GPUMemoryPool_SetFeatureRows(r->memorypool, (int32_t)num_ids);
}

// RunPreSc, Server.cu:284-299: the sampler side alone (seed launch, pre-sampling hops, planner), train mode
void Runner_RunPreSc(Runner* r, RunnerParams* params)
{
    DeviceGuard guard(r->local_dev_id);
    GPUMemoryPool_SetCurrentMode(r->memorypool, 0);
    GPUMemoryPool_SetIter(r->memorypool, params->global_batch_id);
    begin_round(r, (GPUNodeStorage*)params->noder, 0);   // the pre-sampling epoch is the first served epoch's draws
    enqueue_stages(r, r->streams[0], true, true, Gather::None);
    // the reference polls the (never recorded) updater event here, i.e. does not wait: batches of
    // the pre-sampling epoch are simply queued in order on stream 0.
    if (r->modes.agg_last_hop) {   // ... except that sizing the buffer for max(n_in + N) needs both counter arrays of every batch
        int32_t nc[LEGION_COUNTER_WORDS] = {0}, ec[LEGION_COUNTER_WORDS] = {0};
        HIP_CHECK(hipStreamSynchronize(r->streams[0]));
        HIP_CHECK(hipMemcpy(nc, r->memorypool->pipe().node_counter, sizeof(nc), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(ec, r->memorypool->pipe().edge_counter, sizeof(ec), hipMemcpyDeviceToHost));
        r->presc_max_rows = std::max(r->presc_max_rows, legion_agg_rows(nc, ec, r->hops));
    }
}

// RunOnce, Server.cu:301-328
void Runner_RunOnce(Runner* r, RunnerParams* params)
{
    DeviceGuard guard(r->local_dev_id);
    IPCEnv* env = (IPCEnv*)params->env;
    const int32_t batch_id = params->global_batch_id;
    r->mode = IPCEnv_GetCurrentMode(env, batch_id);
    GPUMemoryPool_SetCurrentMode(r->memorypool, r->mode);
    GPUMemoryPool_SetIter(r->memorypool, IPCEnv_GetLocalBatchId(env, batch_id));
    begin_round(r, (GPUNodeStorage*)params->noder, IPCEnv_GetRound(env, batch_id));
    wait_for_pipe(r, env);
    if (r->use_graph && r->mode >= 0 && r->mode < 3) {
        if (!run_graph(r, env, batch_id)) {
            LEGION_ARG_ERROR("Runner_RunOnce: recording the batch graph failed");
            if (error_is_fatal()) exit(EXIT_FAILURE);   // never leave the trainer waiting for a batch that will not come
            post_poisoned(r, env);
            return;
        }
    } else {
        enqueue_stages(r, r->streams[0], false, true, r->gather_all ? Gather::All : Gather::Level);
        HIP_CHECK(hipStreamWaitEvent(r->streams[1], r->plan_ev, 0));
    }
    // stream 1 is ordered behind every launch of the batch through the events, so the mirror and done_ev are its end; the reference spins on
    // cudaEventQuery of the updater's event here (Server.cu:318-324) -- this loop hands the batch over one RunOnce later (see `pending`)
    IPCEnv_MirrorCounters(env, r->local_dev_id, r->current_pipe, r->streams[1]);
    HIP_CHECK(hipEventRecord(r->done_ev[r->current_pipe], r->streams[1]));
    if (error_pending()) {
        // an operator refused its arguments (sticky error): the buffers of this pipe hold stale data.  Never hand
        // them to a trainer -- the reference's error behaviour is exit(EXIT_FAILURE) (Kernels.cuh:14-22).
        log_out() << "Runner_RunOnce: batch " << batch_id << " on GPU " << r->local_dev_id << " failed; server stops\n" << std::flush;
        if (error_is_fatal()) exit(EXIT_FAILURE);
        post_poisoned(r, env);
        return;
    }
    if (r->pending) { // batch i is queued: now hand batch i-1 to its trainer
        HIP_CHECK(hipEventSynchronize(r->done_ev[r->pending_pipe]));
        hand_over(r, env, r->pending_pipe);
    }
    r->pending = true;
    r->pending_pipe = r->current_pipe;
    advance_pipe(r);
}

// Finalize, Server.cu:330-335
void Runner_Finalize(Runner* r, RunnerParams* params)
{
    IPCEnv* env = (IPCEnv*)params->env;
    DeviceGuard guard(r->local_dev_id);
    if (r->pending) { // the last batch of the pipelined loop
        HIP_CHECK(hipEventSynchronize(r->done_ev[r->pending_pipe]));
        hand_over(r, env, r->pending_pipe);
        r->pending = false;
    }
    if (r->short_batches > 0)
        log_out() << r->local_dev_id << " Feature buffer too small for " << r->short_batches << " batches (see the first message)\n" << std::flush;
    IPCEnv_IPCWait(env, r->local_dev_id, (r->current_pipe + 1) % r->pipeline_depth);
    GPUMemoryPool_Finalize(r->memorypool);
}

GPUMemoryPool* Runner_GetMemoryPool(Runner* r) { return r ? r->memorypool : nullptr; }
int64_t Runner_ShortBatches(const Runner* r) { return r ? r->short_batches : 0; }

void Runner_Delete(Runner* r)
{
    if (!r) return;
    for (auto& pipe : r->graphs) for (auto& g : pipe) { LegionBatchGraph_Delete(g); g = nullptr; }
    for (auto e : r->level_ev) if (e) (void)hipEventDestroy(e);
    if (r->plan_ev) (void)hipEventDestroy(r->plan_ev);
    for (auto e : r->done_ev) if (e) (void)hipEventDestroy(e);
    if (r->streams[0]) (void)hipStreamDestroy(r->streams[0]);
    if (r->streams[1]) (void)hipStreamDestroy(r->streams[1]);
    GPUMemoryPool_Delete(r->memorypool);
    delete r;
}

} // extern "C"
