// runner.cpp -- per-GPU pipeline driver and the sampling server:
//   GPURunner   src/Server.cu:163-369   (op list, 2 streams + events, RunPreSc / RunOnce)
//   GPUServer   src/Server.cu:43-161    (boot, pre-sampling epoch, cache build, run loop)
//   GPUGraphStore (loader)  src/GPUGraphStore.cu:30-143,190-443  (meta_config + raw files + seed split)
// The Intel-PCM monitor of the reference (Server.h:54-135) is not rebuilt: CostModel gets its
// transaction input from the collected hotness instead (cache.cpp).
#include "internal.h"

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstring>
#include <fcntl.h>
#include <fstream>
#include <iostream>
#include <optional>
#include <sstream>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>

#include "audit_hooks.h"

using namespace legion;

// =========================================== Runner ======================================================
struct Runner {
    int32_t num_ids = 0, float_attr_len = 0;
    GPUMemoryPool* memorypool = nullptr;
    int current_pipe = 0, pipeline_depth = LEGION_PIPELINE_DEPTH, local_dev_id = 0, mode = 0, op_num = 0, hops = 0;
    hipStream_t streams[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> events;
    std::vector<Operator*> op_factory;
    std::vector<OpParams*> op_params;
    int32_t feature_rows = 0;
    // $LEGION_BATCH_GRAPH=1: the sampler side of a batch (BatchGen, samplers, planner) is replayed as ONE recorded hipGraph per (pipe, mode)
    // on stream 0 and the rows are gathered by one plain launch on stream 1 behind it -- for launch-bound hosts / small batches
    // (-8 % / -5 % per batch at 0.3 x products, a tie at the BASELINE shapes: profiles/r04_graph_trace.md).  The whole batch as one graph
    // (one stream: loses the gather / sampler overlap; fork / join: 38-42 us of idle per batch on this runtime) lost to it at every shape and
    // is no longer a runner mode (profiles/r06_removed_experiments.patch); GPUMemoryPool_Begin/EndBatchCapture still record any op list.
    bool use_graph = false;
    // RunOnce is software-pipelined: the host enqueues batch i and only then waits for batch i-1 and posts its pipe, so the sampler of
    // batch i (stream 0) overlaps the gathers of batch i-1 (stream 1) on the GPU.  (The reference's synchronous loop, Server.cu:301-328,
    // waits for batch i before it looks at batch i+1.)
    // $LEGION_RUNNER_GATHER = auto (default) | level | all.  level: one FeatureExtractor op per level on stream 1 behind each hop (the reference's
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

// Post a finished batch to its trainer.  The feature buffers hold a bounded number of rows (Runner_InitializeFeaturesBuffer: 1.2 x the
// largest batch of the pre-sampling epoch, Server.cu:275); the gather never writes past them, so a batch that reached more nodes arrives
// with its last rows missing and ipc_service.get_next refuses it (the reference's trainer reads past the allocation instead,
// ipc_cuda_kernel.cu:200).  That is a trainer-side failure with no server-side trace -- so the server leaves one: the first such batch
// is logged, all are counted (Runner_Finalize prints the total).

// $LEGION_SAMPLING_SEED: a decimal or 0x hex integer in [0, 2^32)
static bool parse_seed(const char* n, uint32_t& seed)
{
    const bool hex = n[0] == '0' && (n[1] == 'x' || n[1] == 'X');
    const char* digits = hex ? n + 2 : n;
    bool ok = digits[0] != 0 && strlen(digits) <= 16;
    for (const char* c = digits; ok && *c; c++) ok = hex ? isxdigit((unsigned char)*c) != 0 : isdigit((unsigned char)*c) != 0;
    unsigned long long v = 0;
    if (ok) { v = strtoull(digits, nullptr, hex ? 16 : 10); ok = v <= 0xFFFFFFFFull; }
    seed = ok ? (uint32_t)v : 0;
    return ok;
}

// LEGION_AGG_LAST_HOP: atoi, so anything non-numeric is off.  LEGION_AGG_NORM: unset / empty = plain sums, "both" only on a server that aggregates
// the last hop.  LEGION_SAMPLING: unset / empty / "replace" = with replacement, "distinct" or "weighted".  LEGION_SAMPLING_SEED: unset / empty = off.
// LEGION_LP_DRAW: unset / empty / "0" = off, "1" only under a seed (k is resolved against the meta line: serve_modes_resolve_lp_draw).
bool legion::serve_modes_from_env(ServeModes& m, std::string& why)
{
    m = ServeModes();
    const char* agg = getenv("LEGION_AGG_LAST_HOP");
    m.agg_last_hop = agg && atoi(agg) != 0;
    const char* norm = getenv("LEGION_AGG_NORM");
    if (norm && norm[0]) {
        if (strcmp(norm, "both") != 0) { why = std::string("LEGION_AGG_NORM=") + norm + " is not a known norm: `both` (GraphConv norm='both', out-degree rsqrt inside block 1) or unset"; return false; }
        if (!m.agg_last_hop) { why = "LEGION_AGG_NORM=both needs LEGION_AGG_LAST_HOP=1: only the last hop's neighbour sums are normalised"; return false; }
        m.agg_norm = 1;
    }
    const char* sampling = getenv("LEGION_SAMPLING");
    if (sampling && sampling[0] && strcmp(sampling, "replace") != 0) {
        if (strcmp(sampling, "weighted") == 0) m.sampling = kSamplingWeighted;
        else if (strcmp(sampling, "distinct") == 0) m.sampling = kSamplingDistinct;
        else { why = std::string("LEGION_SAMPLING=") + sampling + " is not a known sampling mode: `replace` (the default: draws with replacement) or `distinct` (min(degree, fan-out) distinct neighbours per row), or `weighted` (draws with replacement in proportion to the edge weights)"; return false; }
    }
    const char* seed = getenv("LEGION_SAMPLING_SEED");
    if (seed && seed[0]) {
        if (!parse_seed(seed, m.seed)) { why = std::string("LEGION_SAMPLING_SEED=") + seed + " is not a sampling seed: a decimal or 0x hex integer in [0, 2^32), or unset (the same batches every epoch)"; return false; }
        m.seeded = true;
    }
    const char* lp = getenv("LEGION_LP_DRAW");
    if (lp && lp[0] && strcmp(lp, "0") != 0) {
        if (strcmp(lp, "1") != 0) { why = std::string("LEGION_LP_DRAW=") + lp + " is not a known setting: `1` (the pos and neg thirds of link-prediction batches are drawn per batch), `0` or unset"; return false; }
        if (!m.seeded) { why = "LEGION_LP_DRAW=1 needs LEGION_SAMPLING_SEED: the thirds are drawn from the batch's draw word"; return false; }
        m.lp_draw = 1;
    }
    return true;
}

bool legion::serve_modes_resolve_lp_draw(ServeModes& m, bool lp_lists, int32_t raw_batch_size, std::string& why)
{
    if (!m.lp_draw) return true;
    if (!lp_lists) { why = "LEGION_LP_DRAW=1 needs link-prediction training lists (meta flag 2: [src | pos | neg] thirds per batch)"; return false; }
    if (raw_batch_size < 3 || raw_batch_size % 3 != 0) { why = "LEGION_LP_DRAW=1 needs a batch size divisible by 3 ([src | pos | neg] thirds), the meta line has " + std::to_string(raw_batch_size); return false; }
    m.lp_draw = raw_batch_size / 3;
    return true;
}

// the launcher refuses such a hop per batch (launch_sample_hop): a server that booted would fail every batch, the pre-sampling epoch first
bool legion::serve_modes_fit_fanout(const ServeModes& m, const int32_t* fanout, int32_t hops, std::string& why)
{
    for (int32_t h = 0; m.sampling == 1 && h < hops; h++)
        if (fanout[h] > kDistinctMaxFanout) {
            why = "LEGION_SAMPLING=distinct takes fan-outs of at most " + std::to_string(kDistinctMaxFanout) + ", hop " + std::to_string(h + 1) + " has " +
                  std::to_string(fanout[h]) + ": k_sample stages the picks of a tile's rows in static LDS";
            return false;
        }
    return true;
}

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

static void run_ops(Runner* r)
{
    const int last_feat = 2 * r->hops + 1;           // the FeatureExtractor behind the last hop
    for (int i = 0; i < r->op_num; i++) {
        if (r->gather_all && (i & 1) && i < last_feat) continue;
        if (i % 2 == 1) HIP_CHECK(hipStreamWaitEvent(r->streams[1], r->events[i - 1], 0));
        r->op_params[i]->is_presc = 0;
        if (r->modes.agg_last_hop && i == last_feat) {     // the levels < H that were not gathered per level, and the sums
            OpParams* fp = r->op_params[i];
            get_feature_kernel_agg(r->streams[1], (GPUCache*)fp->cache, (GPUNodeStorage*)fp->noder, r->memorypool, fp->device_id, fp->in_memory);
        } else if (r->gather_all && i == last_feat) {
            OpParams* fp = r->op_params[i];
            get_feature_kernel_all(r->streams[1], (GPUCache*)fp->cache, (GPUNodeStorage*)fp->noder, r->memorypool, fp->device_id, fp->in_memory);
        } else {
            Operator_run(r->op_factory[i], r->op_params[i]);
        }
    }
}

// $LEGION_BATCH_GRAPH=1 (see Runner::use_graph): the recorded sampler side of (pipe, mode) on stream 0 -- recorded on first use --, then
// all rows gathered on stream 1 behind it.  False when the recording failed.
static bool run_graph(Runner* r, IPCEnv* env, int32_t batch_id)
{
    LegionBatchGraph*& g = r->graphs[r->current_pipe][r->mode];
    if (!g) { // record this (pipe, mode) once
        if (GPUMemoryPool_BeginBatchCapture(r->memorypool, r->streams[0]) == 0) {
            // the sampler side only (BatchGen, samplers, planner: the even ops), on ONE stream; the rows are gathered by one plain
            // launch on stream 1 behind the graph, so the gather of batch i overlaps the recorded sampler of batch i + 1 (the other pipe)
            for (int i = 0; i < r->op_num; i += 2) {
                OpParams op = *r->op_params[i];
                op.stream = r->streams[0];
                op.event = nullptr;
                op.is_presc = 0;
                Operator_run(r->op_factory[i], &op);
            }
            g = GPUMemoryPool_EndBatchCapture(r->memorypool, r->streams[0]);
        }
        if (!g) return false;
    }
    LegionBatchGraph_Launch(g, r->streams[0], IPCEnv_GetLocalBatchId(env, batch_id));
    HIP_CHECK(hipEventRecord(r->events[0], r->streams[0]));
    HIP_CHECK(hipStreamWaitEvent(r->streams[1], r->events[0], 0));
    OpParams* fp = r->op_params[1];
    if (r->modes.agg_last_hop) get_feature_kernel_agg(r->streams[1], (GPUCache*)fp->cache, (GPUNodeStorage*)fp->noder, r->memorypool, fp->device_id, fp->in_memory);
    else get_feature_kernel_all(r->streams[1], (GPUCache*)fp->cache, (GPUNodeStorage*)fp->noder, r->memorypool, fp->device_id, fp->in_memory);
    Operator_run(r->op_factory[r->op_num - 1], r->op_params[r->op_num - 1]);   // Updater, stream 1
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
    // op list: [BatchGen, Feat, (Samp, Feat) x hops, Planner, Updater]  (Server.cu:198-207)
    r->op_num = (hop_num + 1) * 2 + 2;
    r->op_factory.resize(r->op_num);
    r->op_factory[0] = NewBatchGenerator(0);
    r->op_factory[1] = NewFeatureExtractor(1);
    for (int i = 0; i < hop_num; i++) {
        r->op_factory[2 * i + 2] = NewRandomSampler(2 * i + 2);
        r->op_factory[2 * i + 3] = NewFeatureExtractor(2 * i + 3);
    }
    r->op_factory[r->op_num - 2] = NewCachePlanner(r->op_num - 2);
    r->op_factory[r->op_num - 1] = NewCacheUpdater(r->op_num - 1);

    r->pipeline_depth = LEGION_PIPELINE_DEPTH;
    { const char* e = getenv("LEGION_BATCH_GRAPH"); r->use_graph = e && atoi(e) != 0; }
    { const char* e = getenv("LEGION_RUNNER_GATHER"); r->gather_all = e && strcmp(e, "all") == 0; r->gather_auto = !e || strcmp(e, "auto") == 0; }
    for (auto& ev : r->done_ev) HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
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
    log_out() << r->local_dev_id << " Sampling: " << (m.sampling == kSamplingWeighted ? "weighted by edge weight, with replacement, from the graph's alias table (LEGION_SAMPLING=weighted)" : m.sampling ? "distinct neighbours, min(degree, fan-out) per row (LEGION_SAMPLING=distinct)" : "with replacement (LEGION_SAMPLING=replace)") << "\n";
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
    r->events.resize(r->op_num);
    r->op_params.resize(r->op_num);
    for (int i = 0; i < r->op_num; i++) {
        OpParams* op = new OpParams();
        op->device_id = r->local_dev_id;
        op->stream = r->streams[i % 2];
        HIP_CHECK(hipEventCreateWithFlags(&r->events[i], hipEventDisableTiming));
        op->event = r->events[i];
        op->memorypool = r->memorypool;
        op->cache = cache;
        op->graph = params->graph;
        op->noder = noder;
        op->env = env;
        op->neighbor_count = 0;
        op->is_presc = 0;
        op->in_memory = params->in_memory;
        r->op_params[i] = op;
    }
    for (int i = 0; i < hop_num; i++) r->op_params[2 * i + 2]->neighbor_count = params->fanout[i];
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
    r->feature_rows = (int32_t)num_ids;
    IPCEnv_InitializeFeaturesBuffer(env, 0, (int32_t)num_ids, r->float_attr_len, r->local_dev_id, r->pipeline_depth);
    for (int i = 0; i < r->pipeline_depth; i++)
        GPUMemoryPool_SetFloatFeatures(r->memorypool, IPCEnv_GetFloatFeatures(env, r->local_dev_id, i), i);
    GPUMemoryPool_SetFeatureRows(r->memorypool, (int32_t)num_ids);
}

// RunPreSc, Server.cu:284-299: only the even ops (BatchGen, samplers, planner), train mode
void Runner_RunPreSc(Runner* r, RunnerParams* params)
{
    DeviceGuard guard(r->local_dev_id);
    GPUMemoryPool_SetCurrentMode(r->memorypool, 0);
    GPUMemoryPool_SetIter(r->memorypool, params->global_batch_id);
    begin_round(r, (GPUNodeStorage*)params->noder, 0);   // the pre-sampling epoch is the first served epoch's draws
    for (int i = 0; i < r->op_num; i += 2) {
        r->op_params[i]->is_presc = 1;
        Operator_run(r->op_factory[i], r->op_params[i]);
    }
    // the reference polls the (never recorded) updater event here, i.e. does not wait: batches of
    // the pre-sampling epoch are simply queued in order on stream 0.
    if (r->modes.agg_last_hop) {   // ... except that sizing the buffer for max(n_in + N) needs both counter arrays of every batch
        int32_t nc[LEGION_COUNTER_WORDS] = {0}, ec[LEGION_COUNTER_WORDS] = {0};
        HIP_CHECK(hipStreamSynchronize(r->streams[0]));
        HIP_CHECK(hipMemcpy(nc, r->memorypool->node_counter[r->memorypool->current_pipe], sizeof(nc), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(ec, r->memorypool->edge_counter[r->memorypool->current_pipe], sizeof(ec), hipMemcpyDeviceToHost));
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
        run_ops(r);
    }
    // the last op of the batch (updater / gather, stream 1) is ordered behind every other op through the op events; the reference spins on
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
    for (auto op : r->op_factory) Operator_Delete(op);
    for (auto p : r->op_params) delete p;
    for (auto e : r->events) (void)hipEventDestroy(e);
    for (auto e : r->done_ev) if (e) (void)hipEventDestroy(e);
    if (r->streams[0]) (void)hipStreamDestroy(r->streams[0]);
    if (r->streams[1]) (void)hipStreamDestroy(r->streams[1]);
    GPUMemoryPool_Delete(r->memorypool);
    delete r;
}

} // extern "C"

// =========================================== Server ======================================================
namespace {

// raw little-endian file -> memory (the mmap_*_read family, GPUGraphStore.cu:30-143)
bool read_file(const std::string& path, void* dst, int64_t max_bytes, int64_t* got = nullptr, bool quiet = false)
{
    int fd = open(path.c_str(), O_RDONLY);
    if (fd == -1) {
        if (!quiet) log_out() << "cannout open file: " << path << "\n";
        return false;
    }
    struct stat st;
    fstat(fd, &st);
    int64_t len = std::min<int64_t>(st.st_size, max_bytes);
    const void* buf = mmap(nullptr, (size_t)(len > 0 ? len : 1), PROT_READ, MAP_PRIVATE, fd, 0);
    if (buf == MAP_FAILED) { close(fd); return false; }
    memcpy(dst, buf, (size_t)len);
    munmap((void*)buf, (size_t)(len > 0 ? len : 1));
    close(fd);
    if (got) *got = len;
    return true;
}

struct Meta { // ReadMetaFIle, GPUGraphStore.cu:190-223
    std::string dataset_path;
    int32_t raw_batch_size = 0, node_num = 0, float_attr_len = 0, epoch = 0, partition = 0;
    int32_t set_num[kModes] = {0, 0, 0};   // seed-set sizes by mode: training, validation, testing
    int64_t edge_num = 0, cache_memory = 0;
};

// Dataset source `synth:<workload>[:<scale>[:<skew>]]` (extension): the tables of the named synthetic shape are generated on the device by
// the legion_synth_* calls bench.py uses -- 64 GB of files per start is not an option for the papers100M shape.  V, E, F of the meta line
// must be the generator's (E = 0: not checked); the seed-set sizes of the meta line take the first n ids of the generator's train / valid /
// test ranges.
struct SynthSource {
    std::string name;
    double scale = 1.0;
    int32_t skew = 205;
};

} // namespace

struct Server {
    int shard_count = 0, train_step = 0, max_step = 0;
    bool replicated = false;   // CSR + features replicated into every GPU's HBM: the cache has nothing to add
    std::string meta_path = "./meta_config";
    std::vector<int32_t> fanout{25, 10}; // Server.cu:68-69
    Meta meta;
    SynthSource synth_src;     // meta.dataset_path, when it names a synth: source
    GPUGraphStorage* graph = nullptr;
    GPUNodeStorage* noder = nullptr;
    GPUCache* cache = nullptr;
    IPCEnv* env = nullptr;
    std::vector<Runner*> runners;
    std::vector<RunnerParams*> params;
    int64_t* indptr = nullptr;
    int32_t* indices = nullptr;
    float* feats = nullptr;
    bool synth = false;        // the tables were generated in HBM (dataset source `synth:`), not read into pinned host memory
    int32_t synth_pitch = 0;   // floats between two feature rows of the generated tables
};

namespace {

// The seed lists the dataset source gives the split, by mode; from files also every node's label and, when the file exists,
// partition_<G>_bn
struct SeedLists {
    std::vector<int32_t> ids[kModes];
    std::vector<int32_t> labels, partition;
    bool have_part = false;
};

// One mode's seeds after the split: ids and labels per partition, and the per-partition views LegionBuildInfo takes of them
struct SeedSplit {
    std::vector<std::vector<int32_t>> ids, labels;
    std::vector<int32_t> num;
    std::vector<const int32_t*> id_ptr, label_ptr;
};

// The meta line, logged as the reference does.  Returns the refusal text (empty: accepted).  Host code only.
std::string read_meta(const std::string& path, Meta& m)
{
    std::ifstream f(path);
    if (!f.is_open()) { log_out() << "unable to open meta config file\n"; return "Server_Initialize: meta_config missing"; }
    std::string line;
    getline(f, line);
    std::istringstream iss(line);
    iss >> m.dataset_path >> m.raw_batch_size >> m.node_num >> m.edge_num >> m.float_attr_len >> m.set_num[LEGION_TRAINMODE] >>
        m.set_num[LEGION_VALIDMODE] >> m.set_num[LEGION_TESTMODE] >> m.cache_memory >> m.epoch >> m.partition;
    log_out() << "Dataset path:       " << m.dataset_path << "\nRaw Batchsize:      " << m.raw_batch_size
              << "\nGraph nodes num:    " << m.node_num << "\nGraph edges num:    " << m.edge_num
              << "\nFeature dim:        " << m.float_attr_len << "\nTraining set num:   " << m.set_num[LEGION_TRAINMODE]
              << "\nValidation set num: " << m.set_num[LEGION_VALIDMODE] << "\nTesting set num:    " << m.set_num[LEGION_TESTMODE]
              << "\nCache memory:       " << m.cache_memory << "\nTrain epoch:        " << m.epoch
              << "\nPartition?:         " << m.partition << "\n";
    // The reference reads the eleven fields unchecked (GPUGraphStore.cu:190-223): a short or mistyped line leaves zeros behind and the
    // first division by the batch size or the first zero-byte table ends the server without a message.  Refuse it here, by name.
    const int32_t min_set = *std::min_element(m.set_num, m.set_num + kModes), max_set = *std::max_element(m.set_num, m.set_num + kModes);
    const char* bad = nullptr;
    if (iss.fail()) bad = "fewer than eleven fields (path batch V E F n_train n_valid n_test cache_bytes epochs partition_flag)";
    else if (m.raw_batch_size < 1) bad = "batch size < 1";
    else if (m.node_num < 1) bad = "node count < 1";
    else if (m.edge_num < 0) bad = "negative edge count";
    else if (m.float_attr_len < 1) bad = "feature dim < 1";
    else if (min_set < 0) bad = "negative seed-set size";
    else if (max_set > m.node_num) bad = "a seed set larger than the node count";
    else if (m.cache_memory < 0) bad = "negative cache budget";
    else if (m.epoch < 0) bad = "negative epoch count";
    else if (m.partition < 0 || m.partition > 2) bad = "partition flag outside 0..2";
    return bad ? std::string("Server_Initialize: meta_config refused: ") + bad : std::string();
}

// `synth:<workload>[:<scale>[:<skew>]]` -> src; false for a dataset path that names files
bool parse_synth(const std::string& path, SynthSource& src)
{
    if (path.rfind("synth:", 0) != 0) return false;
    const std::string rest = path.substr(6);
    const size_t c1 = rest.find(':');
    src.name = rest.substr(0, c1);
    if (c1 != std::string::npos) {
        const std::string tail = rest.substr(c1 + 1);
        const size_t c2 = tail.find(':');
        src.scale = atof(tail.substr(0, c2).c_str());
        if (c2 != std::string::npos) src.skew = atoi(tail.substr(c2 + 1).c_str());
    }
    return true;
}

// One copy of the synthetic tables on the CURRENT device: degrees -> in-place scan -> indptr, neighbours, features.
bool synth_tables_here(const LegionSynthSpec& sp, int32_t skew, int32_t pitch, int64_t** indptr, int32_t** indices, float** feats, int64_t* E)
{
    const int32_t V = sp.V;
    HIP_CHECK(hipMalloc(indptr, ((size_t)V + 1) * sizeof(int64_t)));
    if (!*indptr) return false;
    HIP_CHECK(hipMemset(*indptr, 0, sizeof(int64_t)));
    legion_synth_degrees(nullptr, *indptr + 1, 0, V, sp.ladder);
    inclusive_scan_i64(nullptr, *indptr + 1, *indptr + 1, V);
    HIP_CHECK(hipMemcpy(E, *indptr + V, sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMalloc(indices, (size_t)std::max<int64_t>(*E, 1) * sizeof(int32_t)));
    if (!*indices) return false;
    legion_synth_neighbors_skew(nullptr, *indices, 0, *E, V, sp.M, sp.C, skew);
    HIP_CHECK(hipMalloc(feats, (size_t)V * pitch * sizeof(float)));
    if (!*feats) return false;
    if (pitch > sp.F) HIP_CHECK(hipMemset(*feats, 0, (size_t)V * pitch * sizeof(float)));
    legion_synth_features_pitched(nullptr, *feats, 0, V, sp.F, pitch);
    HIP_CHECK(hipDeviceSynchronize());
    return !error_pending();
}

// synth: source: check the meta line against the generator, generate the tables on logical GPU 0, list the seeds.
bool load_synth(Server* s, LegionSynthSpec& spec, SeedLists& lists)
{
    Meta& m = s->meta;
    const SynthSource& src = s->synth_src;
    if (legion_synth_spec(src.name.c_str(), src.scale, &spec) != 0) { LEGION_ARG_ERROR("Server_Initialize: the synth: dataset path names no known workload / scale"); return false; }
    if (spec.V != m.node_num || spec.F != m.float_attr_len || src.skew < 0 || src.skew > 256) {
        LEGION_ARG_ERROR("Server_Initialize: node count / feature dim of the meta line differ from the synth: generator's");
        return false;
    }
    const int32_t have[kModes] = {spec.n_train, spec.n_valid, spec.n_test};
    for (int mode = 0; mode < kModes; mode++)
        if (m.set_num[mode] > have[mode] || m.set_num[mode] < 0) {
            LEGION_ARG_ERROR("Server_Initialize: a seed set of the meta line is larger than the synth: generator's");
            return false;
        }
    log_out() << "Start generate graph (" << src.name << ", scale " << src.scale << ", skew " << src.skew << "/256)\n";
    s->synth = true;
    s->synth_pitch = legion_row_pitch(spec.F);
    {
        DeviceGuard guard(0);
        int64_t E = 0;
        if (!synth_tables_here(spec, src.skew, s->synth_pitch, &s->indptr, &s->indices, &s->feats, &E)) {
            LEGION_ARG_ERROR("Server_Initialize: generating the synth: tables failed");
            return false;
        }
        if (m.edge_num != 0 && m.edge_num != E) {
            LEGION_ARG_ERROR("Server_Initialize: edge count of the meta line differs from the synth: generator's");
            return false;
        }
        m.edge_num = E;
        log_out() << "Graph generated in HBM: " << E << " edges\n";
    }
    const int64_t first[kModes] = {0, spec.n_train, (int64_t)spec.n_train + spec.n_valid};   // the generator's train / valid / test ranges
    for (int mode = 0; mode < kModes; mode++) {
        lists.ids[mode].resize(m.set_num[mode]);
        for (int32_t i = 0; i < m.set_num[mode]; i++) lists.ids[mode][i] = legion_synth_seed_id_host(first[mode] + i, m.node_num, spec.M2, spec.C2);
    }
    return true;
}

// Load_Graph / Load_Feature (GPUGraphStore.cu:254-325): the tables into pinned, device-mapped host memory, then the seed lists, the labels
// and the optional partition_<G>_bn
bool load_files(Server* s, SeedLists& lists)
{
    static const char* const kSetFile[kModes] = {"trainingset", "validationset", "testingset"};
    const Meta& m = s->meta;
    const int32_t V = m.node_num, F = m.float_attr_len;
    log_out() << "Start load graph\n";
    s->indptr = (int64_t*)host_alloc_space64(((int64_t)V + 1) * 8);
    s->indices = (int32_t*)host_alloc_space64(m.edge_num * 4);
    bool ok = read_file(m.dataset_path + "edge_src", s->indptr, ((int64_t)V + 1) * 8);
    ok = read_file(m.dataset_path + "edge_dst", s->indices, m.edge_num * 4) && ok;
    log_out() << "start load node\n";
    s->feats = (float*)host_alloc_space64((int64_t)V * F * 4);
    ok = read_file(m.dataset_path + "features", s->feats, (int64_t)V * F * 4) && ok;
    lists.labels.resize(V); lists.partition.resize(V);
    for (int mode = 0; mode < kModes; mode++) {
        lists.ids[mode].resize(m.set_num[mode]);
        ok = read_file(m.dataset_path + kSetFile[mode], lists.ids[mode].data(), (int64_t)m.set_num[mode] * 4) && ok;
    }
    ok = read_file(m.dataset_path + "labels", lists.labels.data(), (int64_t)V * 4) && ok;
    // the reference only prints "cannout open file" and carries on with garbage (GPUGraphStore.cu:33-35); fail instead
    if (!ok) { LEGION_ARG_ERROR("Server_Initialize: dataset file(s) missing"); return false; }
    lists.have_part = read_file(m.dataset_path + "partition_" + std::to_string(s->shard_count) + "_bn", lists.partition.data(), (int64_t)V * 4, nullptr, true);
    return true;
}

// synth: source + flag 2: the per-GPU link-prediction lists are GENERATED (legion_synth_lp_seeds, the rule of synth.lp_trainingset): one
// triple per training id in list order, dealt by src % G with its GLOBAL number, every batch laid out as [src | pos | neg] thirds.
bool generate_lp_lists(const Server* s, const std::vector<int32_t>& training_ids, std::vector<std::vector<int32_t>>& out)
{
    const Meta& m = s->meta;
    const int G = s->shard_count;
    DeviceGuard guard(0);
    for (int g = 0; g < G; g++) {
        std::vector<int32_t> srcs;
        std::vector<int64_t> tno;
        for (int64_t t = 0; t < (int64_t)training_ids.size(); t++)
            if (training_ids[t] % G == g) { srcs.push_back(training_ids[t]); tno.push_back(t); }
        const int64_t n = (int64_t)srcs.size(), k = m.raw_batch_size / 3;
        const int64_t n_out = (n + k - 1) / k * m.raw_batch_size;
        out[g].assign((size_t)n_out, 0);
        if (n == 0) continue;
        int32_t *d_src = nullptr, *d_out = nullptr;
        int64_t* d_tno = nullptr;
        HIP_CHECK(hipMalloc(&d_src, (size_t)n * 4)); HIP_CHECK(hipMalloc(&d_tno, (size_t)n * 8)); HIP_CHECK(hipMalloc(&d_out, (size_t)n_out * 4));
        if (!d_src || !d_tno || !d_out) return false;
        HIP_CHECK(hipMemcpy(d_src, srcs.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_tno, tno.data(), (size_t)n * 8, hipMemcpyHostToDevice));
        legion_synth_lp_seeds(nullptr, d_out, d_src, d_tno, n, m.raw_batch_size, s->indptr, s->indices, m.node_num, 1);
        HIP_CHECK(hipMemcpy(out[g].data(), d_out, (size_t)n_out * 4, hipMemcpyDeviceToHost));
        (void)hipFree(d_src); (void)hipFree(d_tno); (void)hipFree(d_out);
    }
    if (error_pending()) return false;
    log_out() << "Link-prediction seed lists generated: " << out[0].size() << " seeds on GPU 0\n";
    return true;
}

// Pre-partitioned training lists (extension, not in the reference): meta flag 2 = GPU g serves the file
// trainingset_<G>_<g> verbatim.  Needed for link prediction on G > 1 GPUs: lp_sage.py:87-90 expects every
// batch as [src | pos | neg] thirds, which neither split rule below preserves (synth.lp_trainingset writes them).
bool read_lp_lists(const Meta& m, int G, std::vector<std::vector<int32_t>>& out)
{
    bool ok = true;
    for (int g = 0; g < G && ok; g++) {
        const std::string path = m.dataset_path + "trainingset_" + std::to_string(G) + "_" + std::to_string(g);
        struct stat st;
        if (stat(path.c_str(), &st) != 0) { log_out() << "cannout open file: " << path << "\n"; ok = false; break; }
        out[g].resize((size_t)st.st_size / 4);
        ok = read_file(path, out[g].data(), (int64_t)out[g].size() * 4);
        for (int32_t tid : out[g]) if (tid < 0 || tid >= m.node_num) ok = false;
    }
    if (!ok) LEGION_ARG_ERROR("Server_Initialize: pre-partitioned training lists (meta flag 2) missing or out of range");
    return ok;
}

// flags 0 / 1: training id t to partition t % G, or (flag 1) to partition_<G>_bn[t] when that file exists
bool split_training(const Meta& m, const SeedLists& lists, int G, std::vector<std::vector<int32_t>>& out)
{
    for (int32_t tid : lists.ids[LEGION_TRAINMODE]) {
        if (tid < 0 || tid >= m.node_num) { LEGION_ARG_ERROR("Server_Initialize: training id outside [0, V)"); return false; }
        int32_t part = (lists.have_part && m.partition == 1) ? lists.partition[tid] : tid % G;
        if (part >= 0 && part < G) out[part].push_back(tid); // the reference indexes unchecked (GPUGraphStore.cu:338-341)
    }
    return true;
}

// seed split, GPUGraphStore.cu:332-414: the training ids by the rule of the meta line's partition flag, the validation and test ids by
// id % G; then every id's label
bool split_seeds(const Server* s, const SeedLists& lists, const LegionSynthSpec& spec, SeedSplit* split)
{
    const Meta& m = s->meta;
    const int G = s->shard_count;
    for (int mode = 0; mode < kModes; mode++) split[mode].ids.assign(G, {});
    std::vector<std::vector<int32_t>>& train = split[LEGION_TRAINMODE].ids;
    const bool ok = m.partition != 2 ? split_training(m, lists, G, train)
                  : s->synth ? generate_lp_lists(s, lists.ids[LEGION_TRAINMODE], train)
                  : read_lp_lists(m, G, train);
    if (!ok) return false;
    for (int mode = LEGION_VALIDMODE; mode <= LEGION_TESTMODE; mode++)
        for (int32_t tid : lists.ids[mode]) { int32_t part = tid % G; if (part < G) split[mode].ids[part].push_back(tid); }
    for (int mode = 0; mode < kModes; mode++) {
        split[mode].labels.assign(G, {});
        for (int p = 0; p < G; p++)
            for (int32_t id : split[mode].ids[p])
                split[mode].labels[p].push_back(s->synth ? legion_synth_label_host(id, spec.classes) : lists.labels[id]);
    }
    return true;
}

// LegionBuildInfo of the boot (the split seeds, the tables where the dataset source left them) and what is built from it: the IPC
// environment's schedule and the two storages
void build_storages(Server* s, SeedSplit* split)
{
    const Meta& m = s->meta;
    const int G = s->shard_count;
    LegionBuildInfo info;
    memset(&info, 0, sizeof(info));
    info.partition_count = G;
    for (int mode = 0; mode < kModes; mode++) {
        SeedSplit& set = split[mode];
        for (int p = 0; p < G; p++) {
            set.num.push_back((int32_t)set.ids[p].size());
            set.id_ptr.push_back(set.ids[p].data());
            set.label_ptr.push_back(set.labels[p].data());
        }
        info.*kBuildInfoSeeds[mode].num = set.num.data();
        info.*kBuildInfoSeeds[mode].ids = set.id_ptr.data();
        info.*kBuildInfoSeeds[mode].labels = set.label_ptr.data();
    }
    info.total_num_nodes = m.node_num; info.float_attr_len = m.float_attr_len;
    const int32_t table_loc = s->synth ? LEGION_LOC_DEVICE : LEGION_LOC_HOST_PINNED;
    info.host_float_attrs = s->feats; info.features_location = table_loc;
    info.float_attr_pitch = s->synth ? s->synth_pitch : 0;
    info.csr_node_index = s->indptr; info.csr_dst_node_ids = s->indices; info.csr_location = table_loc;
    info.total_edge_num = m.edge_num; info.cache_edge_num = 0;
    info.epoch = m.epoch; info.raw_batch_size = m.raw_batch_size;

    s->env = NewIPCEnv(G);
    IPCEnv_Coordinate(s->env, &info);
    s->noder = NewGPUMemoryNodeStorage();
    GPUNodeStorage_Build(s->noder, &info);
    s->graph = NewGPUMemoryGraphStorage();
    GPUGraphStorage_Build(s->graph, &info);
}

// MI355X-first: 288 GB of HBM usually hold the whole dataset, so replicate the tables into every GPU's HBM
// instead of reading them over PCIe (the reference's UVA zero-copy).  $LEGION_TABLES = device | host | auto
// (default auto: replicate when CSR + features + 20 % fit into the free HBM of every GPU).
bool place_tables(Server* s, const LegionSynthSpec& spec)
{
    const Meta& m = s->meta;
    const int G = s->shard_count;
    const int32_t V = m.node_num, F = m.float_attr_len;
    const char* mode = getenv("LEGION_TABLES");
    const std::string tables = s->synth ? "synth" : (mode ? mode : "auto");
    const int64_t need = (((int64_t)V + 1) * 8 + m.edge_num * 4 + (int64_t)V * F * 4);
    bool replicate = tables == "device";
    if (tables == "auto") {
        replicate = true;
        for (int i = 0; i < G; i++) {
            DeviceGuard guard(i);
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            if ((double)need * 1.2 > (double)free_b) replicate = false;
        }
    }
    if (s->synth) {
        // generated in HBM on logical GPU 0; every other physical device of the job gets a copy of its own, generated in place
        // (the storages free them as replicas)
        std::vector<int> have{physical_device(0)};
        for (int i = 1; i < G; i++) {
            const int phys = physical_device(i);
            int src = -1;
            for (int j = 1; j < i; j++) if (physical_device(j) == phys && s->graph->replica_indptr[j]) src = j;
            if (phys == have[0]) {                                 // shares GPU 0's tables
                LEGION_AUDIT_SHARE(s->indptr, i); LEGION_AUDIT_SHARE(s->indices, i); LEGION_AUDIT_SHARE(s->feats, i);
                continue;
            }
            if (src >= 0) {
                s->graph->replica_indptr[i] = s->graph->replica_indptr[src]; s->graph->replica_indices[i] = s->graph->replica_indices[src];
                s->noder->replica_attrs[i] = s->noder->replica_attrs[src];
                LEGION_AUDIT_SHARE(s->graph->replica_indptr[i], i); LEGION_AUDIT_SHARE(s->graph->replica_indices[i], i); LEGION_AUDIT_SHARE(s->noder->replica_attrs[i], i);
                continue;
            }
            DeviceGuard guard(i);
            int64_t E2 = 0;
            if (!synth_tables_here(spec, s->synth_src.skew, s->synth_pitch, &s->graph->replica_indptr[i], &s->graph->replica_indices[i],
                                   &s->noder->replica_attrs[i], &E2) || E2 != m.edge_num) {
                LEGION_ARG_ERROR("Server_Initialize: generating the synth: tables on a further GPU failed");
                return false;
            }
        }
        s->noder->replica_pitch = s->synth_pitch;
        // $LEGION_SYNTH_CACHE=1: build the hotness cache anyway (budget = the meta line's cache_memory), as if the generated tables were the
        // reference's host tables -- the cost model, FillUp and the cached gather / partitioned sampler through the server binary on a
        // synth: source (bench.py's `cached_gather.served`, tests).  Default: everything is already HBM resident, a cache has nothing to add.
        { const char* e = getenv("LEGION_SYNTH_CACHE"); s->replicated = !(e && e[0] == '1'); }
        log_out() << "Tables generated in HBM: " << need / 1e9 << " GB per GPU" << (s->replicated ? "" : " (cache built on top: LEGION_SYNTH_CACHE=1)") << "\n";
    } else if (replicate) {
        GPUGraphStorage_ReplicateToDevices(s->graph);
        GPUNodeStorage_ReplicateToDevices(s->noder);
        s->replicated = true;
        log_out() << "Tables replicated into HBM: " << need / 1e9 << " GB per GPU\n";
    } else {
        log_out() << "Tables stay in pinned host memory (" << need / 1e9 << " GB)\n";
    }
    return true;
}

// LEGION_SAMPLING=weighted: the graph's edge weights -- `edge_weights` (float32[E], one per entry of edge_dst) beside the dataset's files,
// generated on the device for a synth: source -- become the graph's alias table on every GPU of the job (GPUGraphStorage_SetEdgeWeights).
bool load_edge_weights(Server* s)
{
    const Meta& m = s->meta;
    const int64_t E = m.edge_num;
    if (s->synth) {
        DeviceGuard guard(0);
        float* d_w = nullptr;
        HIP_CHECK(hipMalloc(&d_w, (size_t)std::max<int64_t>(E, 1) * sizeof(float)));
        if (!d_w) return false;
        legion_synth_edge_weights(nullptr, d_w, 0, E);
        HIP_CHECK(hipDeviceSynchronize());
        const int rc = GPUGraphStorage_SetEdgeWeights(s->graph, d_w, LEGION_LOC_DEVICE);
        (void)hipFree(d_w);
        if (rc != 0) return false;
    } else {
        std::vector<float> w((size_t)std::max<int64_t>(E, 1));
        int64_t got = 0;
        const std::string path = m.dataset_path + "edge_weights";
        if (!read_file(path, w.data(), E * 4, &got) || got != E * 4) {
            LEGION_ARG_ERROR(("Server_Initialize: LEGION_SAMPLING=weighted needs " + path + ": float32[" + std::to_string(E) + "], one weight per entry of edge_dst (missing or short)").c_str());
            return false;
        }
        if (GPUGraphStorage_SetEdgeWeights(s->graph, w.data(), LEGION_LOC_HOST_PAGEABLE) != 0) return false;
    }
    log_out() << "Edge weights: alias table built in HBM, " << E * 8 / 1e9 << " GB per GPU\n";
    return true;
}

// the cache, then one runner per GPU (GPUServer::Initialize, Server.cu:70-81)
void start_runners(Server* s)
{
    const int G = s->shard_count;
    s->cache = NewGPUCache();
    const int32_t train_step = IPCEnv_GetTrainStep(s->env);
    GPUCache_Initialize(s->cache, s->meta.cache_memory, 0, s->meta.float_attr_len, train_step, G);
    log_out() << "Storage Initialized\n";
    s->train_step = train_step;
    s->max_step = IPCEnv_GetMaxStep(s->env);
    s->runners.resize(G);
    s->params.resize(G);
    for (int i = 0; i < G; i++) {
        RunnerParams* p = new RunnerParams();
        p->device_id = i;
        p->fanout = s->fanout.data();
        p->hops = (int32_t)s->fanout.size();
        p->cache = s->cache; p->graph = s->graph; p->noder = s->noder; p->env = s->env;
        p->global_batch_id = 0;
        p->in_memory = 1;
        s->params[i] = p;
        s->runners[i] = NewGPURunner();
        s->runners[i]->lists_verbatim = s->meta.partition == 2;
        Runner_Initialize(s->runners[i], p);
    }
}

} // namespace

extern "C" {

Server* NewGPUServer(void) { return new Server(); }
void Server_SetFanout(Server* s, const int32_t* fanout, int32_t hops)
{
    if (!s || !fanout || hops < 1 || hops > LEGION_MAX_HOPS) { LEGION_ARG_ERROR("Server_SetFanout: bad arguments"); return; }
    s->fanout.assign(fanout, fanout + hops);
}
void Server_SetMetaConfigPath(Server* s, const char* path) { if (s && path) s->meta_path = path; }

// GPUServer::Initialize (Server.cu:45-81) + GPUGraphStore::Initialze (GPUGraphStore.cu:429-470)
void Server_Initialize(Server* s, int global_shard_count)
{
    if (!s || global_shard_count < 1 || global_shard_count > kMaxParts) { LEGION_ARG_ERROR("Server_Initialize: shard count must be 1..8"); return; }
    s->shard_count = global_shard_count;
    log_out() << "HIP Device Count: " << global_shard_count << "\n";
    const std::string refused = read_meta(s->meta_path, s->meta);
    if (!refused.empty()) { LEGION_ARG_ERROR(refused.c_str()); return; }
    ServeModes modes;   // checked before any device is touched; every runner parses them for itself
    std::string why;
    if (!serve_modes_from_env(modes, why) || !serve_modes_fit_fanout(modes, s->fanout.data(), (int32_t)s->fanout.size(), why) ||
        !serve_modes_resolve_lp_draw(modes, s->meta.partition == 2, s->meta.raw_batch_size, why)) { LEGION_ARG_ERROR(("Server_Initialize: " + why).c_str()); return; }
    const Meta& m = s->meta;
    // from the first device call on the main thread works on GPU 0 unless a scope below says otherwise (the reference's main thread never
    // leaves device 0); not before the meta line and the synth: source are validated -- a refused configuration touches no device
    std::optional<DeviceGuard> boot;
    LegionSynthSpec spec{};
    SeedLists lists;
    if (parse_synth(m.dataset_path, s->synth_src)) {
        if (!load_synth(s, spec, lists)) return;
        boot.emplace(0);
        if (m.partition == 2 && m.raw_batch_size % 3 != 0) {
            LEGION_ARG_ERROR("Server_Initialize: synth: link-prediction lists (meta flag 2) need a batch size divisible by 3 ([src | pos | neg] thirds, lp_sage.py:87-90)");
            return;
        }
    } else {
        boot.emplace(0);
        if (!load_files(s, lists)) return;
    }
    log_out() << "Finish Reading All Files\n";
    SeedSplit split[kModes];
    if (!split_seeds(s, lists, spec, split)) return;
    log_out() << "Finish Partition\n";
    build_storages(s, split);
    if (!place_tables(s, spec)) return;
    if (modes.sampling == kSamplingWeighted && !load_edge_weights(s)) return;
    start_runners(s);
}

// PreSc, Server.cu:83-114
void Server_PreSc(Server* s, int cache_agg_mode)
{
    DeviceGuard boot(0);
    auto t1 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (int i = 0; i < s->shard_count; i++)
        pool.emplace_back([s, i]() { // PreSCLoop, Server.cu:28-34
            for (int b = 0; b < s->train_step; b++) {
                s->params[i]->global_batch_id = b;
                Runner_RunPreSc(s->runners[i], s->params[i]);
            }
            Runner_InitializeFeaturesBuffer(s->runners[i], s->params[i]);
        });
    for (auto& th : pool) th.join();
    double t = std::chrono::duration_cast<std::chrono::duration<double>>(std::chrono::steady_clock::now() - t1).count();
    GPUCache_CandidateSelection(s->cache, cache_agg_mode, s->noder, s->graph);
    // everything already sits in each GPU's HBM: caching would only add an id -> slot indirection (option c)
    if (s->replicated) GPUCache_SetCapacity(s->cache, 0, 0);
    GPUCache_CostModel(s->cache, cache_agg_mode, s->noder, s->graph, nullptr, s->train_step);
    GPUCache_FillUp(s->cache, cache_agg_mode, s->noder, s->graph);
    log_out() << "First epoch cost: " << t << " s\n";
    log_out() << "System is ready for serving\n" << std::flush;
}

// Run, Server.cu:116-135
void Server_Run(Server* s)
{
    std::vector<std::thread> pool;
    for (int i = 0; i < s->shard_count; i++)
        pool.emplace_back([s, i]() { // RunnerLoop, Server.cu:36-41
            for (int b = 0; b < s->max_step; b++) {
                s->params[i]->global_batch_id = b;
                Runner_RunOnce(s->runners[i], s->params[i]);
            }
        });
    for (auto& th : pool) th.join();
}

// Finalize, Server.cu:137-146
void Server_Finalize(Server* s)
{
    DeviceGuard boot(0);
    for (int i = 0; i < s->shard_count; i++) {
        int64_t st[3];
        legion_peer_exchange_stats(Runner_GetMemoryPool(s->runners[i]), st);     // $LEGION_PEER_GATHER=exchange: what the bulk-copy gather did
        if (st[0] > 0) log_out() << i << " peer exchange gather: " << st[0] << " batches, " << st[1] << " rows over hipMemcpyPeerAsync, " << st[2] << " host syncs\n";
        Runner_Finalize(s->runners[i], s->params[i]);
    }
    GPUGraphStorage_Finalize(s->graph);
    GPUNodeStorage_Finalize(s->noder);
    IPCEnv_Finalize(s->env);
    log_out() << std::flush;
    (void)legion_audit_report();     // $LEGION_DEVICE_AUDIT=1: what the logical-device audit saw (server_main exits non-zero on a violation)
    log_out() << "Server Stopped\n";
}

void Server_Delete(Server* s)
{
    if (!s) return;
    DeviceGuard boot(0);
    for (auto r : s->runners) Runner_Delete(r);
    for (auto p : s->params) delete p;
    if (s->cache) GPUCache_Delete(s->cache);
    if (s->graph) GPUGraphStorage_Delete(s->graph);
    if (s->noder) GPUNodeStorage_Delete(s->noder);
    if (s->synth) {
        DeviceGuard guard(0);
        (void)hipFree(s->indptr); (void)hipFree(s->indices); (void)hipFree(s->feats);
    } else {
        if (s->indptr) host_free_space(s->indptr);
        if (s->indices) host_free_space(s->indices);
        if (s->feats) host_free_space(s->feats);
    }
    delete s;
}

} // extern "C"
