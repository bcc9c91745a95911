// ipc_env.cpp -- the server half of the hand-off (ipc_shm.h): CUDAIPCEnv, src/CUDA_IPC_Service.cu:39-360.
#include "ipc_shm.h"

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <ctime>
#include <mutex>
#include <sys/mman.h>
#include <unistd.h>

#include "audit_hooks.h"

using namespace legion;

struct IPCEnv {
    volatile shmStruct* shm = nullptr;
    int shm_fd = -1;
    volatile shmExt* ext = nullptr;    // the extension object ("<name>_ext"); never null once NewIPCEnv succeeded
    int ext_fd = -1;
    volatile shmExt2* ext2 = nullptr;  // "<name>_ext2": null until something it carries is on (ext2_of creates it)
    int ext2_fd = -1;
    int32_t device_count = 0;
    void* buf[LEGION_MAX_DEVICE][LEGION_PIPELINE_DEPTH][LEGION_MEMORY_USAGE] = {};   // the slab's indices; null: not registered
    sem_t* semr[LEGION_MAX_DEVICE][LEGION_PIPELINE_DEPTH] = {};
    sem_t* semw[LEGION_MAX_DEVICE][LEGION_PIPELINE_DEPTH] = {};
    int32_t pipes[LEGION_MAX_DEVICE] = {};   // pipes InitializeSamplesBuffer registered for a device; 0 = the device is not initialised
    int32_t raw_batch_size = 0;
    std::vector<int32_t> train_batch_size, valid_batch_size, test_batch_size;
    int32_t train_step = 0, valid_step = 0, test_step = 0, epoch = 0, pipeline_depth = LEGION_PIPELINE_DEPTH;
    std::vector<VmmRegion*> vmm;   // feature buffers above the HIP-IPC size limit (chunked, mapped, served over a unix socket)
    bool shm_pinned = false;       // the slab is registered with the runtime: asynchronous copies can target the counter mirror
    bool mirror_fresh[LEGION_MAX_DEVICE][LEGION_PIPELINE_DEPTH] = {};   // IPCEnv_MirrorCounters ran for the batch about to be posted
    int32_t* mirror_stage[LEGION_MAX_DEVICE][LEGION_PIPELINE_DEPTH] = {};  // slab not page-locked: queued copies land in pinned staging words
};

// The _ext2 object of an env: created (and tied to the slab as it stands) by the first caller that has something to put there, i.e. `create`.
// The runners of one server initialise on their own threads, hence the lock.
static void tie_ext2(IPCEnv* e)
{
    if (!e->ext2 || !e->ext) return;
    for (int i = 0; i < 3; i++) e->ext2->steps_copy[i] = e->ext->steps_copy[i];
    for (int d = 0; d < LEGION_MAX_DEVICE; d++) e->ext2->handle_sum[d] = e->ext->handle_sum[d];
}
static volatile shmExt2* ext2_of(IPCEnv* e, bool create)
{
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (!e || !e->shm || e->ext2 || !create) return e ? e->ext2 : nullptr;
    e->ext2 = (volatile shmExt2*)shm_map(sizeof(shmExt2), &e->ext2_fd, ext2_name());
    if (!e->ext2) { LEGION_ARG_ERROR("IPCEnv: shm_open/mmap of the second extension object (_ext2) failed"); return nullptr; }
    memset((void*)e->ext2, 0, sizeof(shmExt2));
    e->ext2->bytes = (uint32_t)sizeof(shmExt2);
    tie_ext2(e);
    e->ext2->magic = kExt2Magic;
    return e->ext2;
}
static const volatile shmExt2* ext2_of(const IPCEnv* e) { return e ? e->ext2 : nullptr; }

void legion::ipc_env_publish_modes(IPCEnv* e, const ServeModes& m)
{
    if (!e || !e->ext) return;
    volatile shmExt::Modes& w = e->ext->modes;
    w.agg_last_hop = m.agg_last_hop; w.agg_norm = m.agg_norm; w.sampling = m.sampling; w.sampling_seed = m.seeded ? m.seed : 0u; w.sampling_seeded = m.seeded;
    IPCEnv_SetLpDraw(e, m.lp_draw); IPCEnv_SetWeightedDistinct(e, m.weighted_distinct); IPCEnv_SetSharedDraws(e, m.shared_draws);
    IPCEnv_SetEdgeIds(e, m.edge_ids); IPCEnv_SetEdgeWeights(e, serve_modes_edge_w_filled(m)); IPCEnv_SetAggEdgeWeight(e, m.agg_edge_weight);
}

static const volatile shmExt* ext_of(const IPCEnv* e) { return e ? e->ext : nullptr; }
// both counter arrays of one (device, pipe), nc | ec, between the mirror, the pinned staging words and a local array
static void copy_counters(volatile int32_t* dst, const volatile int32_t* src)
{
    for (int i = 0; i < 2 * kWords; i++) dst[i] = src[i];
}

extern "C" {

static void pin_slab(IPCEnv* e);

// CUDAIPCEnv::CUDAIPCEnv, CUDA_IPC_Service.cu:41-65
IPCEnv* NewIPCEnv(int32_t device_count)
{
    if (device_count < 1 || device_count > LEGION_MAX_DEVICE) { LEGION_ARG_ERROR("NewIPCEnv: device_count must be 1..8"); return nullptr; }
    IPCEnv* e = new IPCEnv();
    log_out() << "start initialize ipc env\n";
    e->shm = (volatile shmStruct*)shm_map(sizeof(shmStruct), &e->shm_fd);
    if (!e->shm) {
        fprintf(log_file(), "Failed to create shared memory slab\n"); // reference: exit(EXIT_FAILURE) (CUDA_IPC_Service.cu:46-48)
        delete e;
        LEGION_ARG_ERROR("NewIPCEnv: shm_open/mmap failed");
        return nullptr;
    }
    e->ext = (volatile shmExt*)shm_map(sizeof(shmExt), &e->ext_fd, ext_name());
    if (!e->ext) {
        munmap((void*)e->shm, sizeof(shmStruct)); close(e->shm_fd);
        delete e;
        LEGION_ARG_ERROR("NewIPCEnv: shm_open/mmap of the extension object failed");
        return nullptr;
    }
    log_out() << "Shared Memory Opened\n";
    memset((void*)e->shm, 0, sizeof(shmStruct));     // ADVICE.md, open: a second server of the namespace wipes a live server's table here
    memset((void*)e->ext, 0, sizeof(shmExt));
    shm_unlink(ext2_name().c_str());                 // a fresh server must not inherit a dead server's words; its own appears with the first word that is on
    e->device_count = device_count;
    pin_slab(e);
    return e;
}

// Page-lock the slab so that a copy engine can write the counter mirror (hipMemcpyAsync into pageable memory is staged and
// synchronous).  Called with a device current; failure only costs the asynchronous path.
static void pin_slab(IPCEnv* e)
{
    if (e->shm_pinned || !e->ext) return;
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), bytes = (sizeof(shmExt) + page - 1) / page * page;
    const char* no_pin = getenv("LEGION_IPC_NO_PIN");      // test hook: behave as if the runtime refused (the staging path below)
    if (no_device()) { e->ext->mirror_magic = kMirrorMagic; return; }
    if (!(no_pin && no_pin[0] == '1') && hipHostRegister((void*)e->ext, bytes, hipHostRegisterPortable) == hipSuccess) e->shm_pinned = true;
    else (void)hipGetLastError();
    e->ext->mirror_magic = kMirrorMagic;    // the mirror is maintained either way (synchronously in IPCPost if need be)
}

// An evaluation split (validation or test): as many steps as the largest partition needs in batches of 512, every partition's set
// spread evenly over them (CUDA_IPC_Service.cu:101-118).  Returns the step count.
static int32_t eval_split(const int32_t* set_num, int32_t P, std::vector<int32_t>& batch_size)
{
    const int32_t raw_batch_size = 512;
    int32_t max_size = 0;
    for (int32_t i = 0; i < P; i++) max_size = std::max(max_size, set_num[i]);
    const int32_t step = (max_size - 1) / raw_batch_size + 1;
    batch_size.resize(P);
    for (int32_t i = 0; i < P; i++) batch_size[i] = (set_num[i] - 1) / step + 1;
    return step;
}

// Coordinate, CUDA_IPC_Service.cu:66-134
void IPCEnv_Coordinate(IPCEnv* e, const LegionBuildInfo* info)
{
    if (!e || !info) { LEGION_ARG_ERROR("IPCEnv_Coordinate: null argument"); return; }
    if (info->partition_count < 1 || info->partition_count > e->device_count || info->raw_batch_size < 1 || info->epoch < 0 ||
        !info->training_set_num || !info->validation_set_num || !info->testing_set_num) {
        // the reference divides by raw_batch_size unchecked (CUDA_IPC_Service.cu:89)
        LEGION_ARG_ERROR("IPCEnv_Coordinate: partition_count must be 1..device_count, raw_batch_size >= 1, epoch >= 0, the three size arrays non-null");
        return;
    }
    const int32_t P = info->partition_count;
    e->epoch = info->epoch;
    e->raw_batch_size = info->raw_batch_size;
    int32_t min_train_size = 1000000000;
    for (int32_t i = 0; i < P; i++) min_train_size = std::min(min_train_size, info->training_set_num[i]);
    e->train_step = (min_train_size - 1) / e->raw_batch_size;
    e->train_batch_size.assign(P, e->raw_batch_size);
    e->valid_step = eval_split(info->validation_set_num, P, e->valid_batch_size);
    e->test_step = eval_split(info->testing_set_num, P, e->test_batch_size);
    log_out() << "Train Steps: " << e->train_step << "\n";
    log_out() << "Valid Steps: " << e->valid_step << "\n";
    log_out() << "Test Steps: " << e->test_step << "\n";
    e->shm->steps[0] = e->train_step;
    e->shm->steps[1] = e->valid_step;
    e->shm->steps[2] = e->test_step;
    if (e->ext) for (int i = 0; i < 3; i++) e->ext->steps_copy[i] = e->shm->steps[i];
    tie_ext2(e);
}

int32_t IPCEnv_GetMaxStep(IPCEnv* e) { return ((e->train_step + e->valid_step) * e->epoch) + e->test_step; }

static void* ipc_alloc(volatile shmStruct* shm, int dev, int pipe, int which, size_t bytes)
{
    void* p = nullptr;
    if (no_device()) return nullptr;      // handle slot stays zero
    // a trainer would stall forever inside ipc_service.initialize() on a buffer it cannot import
    if (!ipc_size_ok((int64_t)bytes, which == LEGION_BUF_FEATURES ? "InitializeFeaturesBuffer (rows x F x 4 bytes of one pipe)" : "InitializeSamplesBuffer")) {
        if (!error_is_fatal()) return nullptr;
        fflush(stderr);
        exit(EXIT_FAILURE);
    }
    HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
    LEGION_AUDIT_OWNER(p, dev, "hand-off buffer");
    if (p) HIP_CHECK(hipIpcGetMemHandle((hipIpcMemHandle_t*)&shm->memHandle[dev][pipe][which], p));
    return p;
}

// InitializeSamplesBuffer, CUDA_IPC_Service.cu:140-201
void IPCEnv_InitializeSamplesBuffer(IPCEnv* e, int32_t batch_size, int32_t num_ids, int32_t feature_dim,
                                    int32_t device_id, int32_t pipeline_depth)
{
    (void)feature_dim;
    if (!e || device_id < 0 || device_id >= e->device_count || pipeline_depth < 1 || pipeline_depth > LEGION_PIPELINE_DEPTH) { LEGION_ARG_ERROR("InitializeSamplesBuffer: bad arguments"); return; }
    LEGION_DEVICE_GUARD(device_id);
    const struct { int slot; size_t count; } sized[] = {      // every slot but the features', int32 elements each
        {LEGION_BUF_IDS, (size_t)num_ids}, {LEGION_BUF_LABELS, (size_t)batch_size}, {LEGION_BUF_AGG_SRC, (size_t)num_ids},
        {LEGION_BUF_AGG_DST, (size_t)num_ids}, {LEGION_BUF_NODE_COUNTER, (size_t)kWords}, {LEGION_BUF_EDGE_COUNTER, (size_t)kWords}};
    for (int32_t i = 0; i < pipeline_depth; i++) {
        void** buf = e->buf[device_id][i];
        e->pipes[device_id] = i + 1;
        for (const auto& b : sized) buf[b.slot] = ipc_alloc(e->shm, device_id, i, b.slot, b.count * sizeof(int32_t));
        if (i == 0 && e->ext) { e->ext->handle_sum[device_id] = handle_checksum(&e->shm->memHandle[device_id][0][LEGION_BUF_IDS]); tie_ext2(e); }
        for (int slot : {LEGION_BUF_NODE_COUNTER, LEGION_BUF_EDGE_COUNTER})
            if (buf[slot]) HIP_CHECK(hipMemset(buf[slot], 0, kCounterBytes));
        // memory lock
        if (!sem_pair_open(device_id, i, true, e->semr[device_id][i], e->semw[device_id][i],
                           "InitializeSamplesBuffer: sem_open(sem_r) failed", "InitializeSamplesBuffer: sem_open(sem_w) failed")) return;
    }
    e->pipeline_depth = pipeline_depth;
}

// InitializeFeaturesBuffer, CUDA_IPC_Service.cu:203-212
void IPCEnv_InitializeFeaturesBuffer(IPCEnv* e, int32_t batch_size, int32_t num_ids, int32_t feature_dim,
                                     int32_t device_id, int32_t pipeline_depth)
{
    (void)batch_size;
    if (!e || device_id < 0 || device_id >= e->device_count) { LEGION_ARG_ERROR("InitializeFeaturesBuffer: bad arguments"); return; }
    if (no_device()) return;
    DeviceGuard guard(device_id);
    const size_t bytes = (size_t)num_ids * feature_dim * sizeof(float);
    const bool vmm = (int64_t)bytes > ipc_max_bytes();
    for (int32_t i = 0; i < pipeline_depth; i++) {
        void* p = nullptr;
        if (vmm) {   // too large for one IPC handle under the PyTorch runtime: chunks + one contiguous mapping on both sides
            VmmRegion* r = vmm_create(device_id, i, bytes);
            if (!r) {
                if (!error_is_fatal()) return;
                fflush(stderr);
                exit(EXIT_FAILURE);
            }
            e->vmm.push_back(r);
            memcpy((void*)&e->shm->memHandle[device_id][i][LEGION_BUF_FEATURES], &vmm_desc(r), sizeof(VmmDesc));
            p = vmm_va(r);
        } else {
            p = ipc_alloc(e->shm, device_id, i, LEGION_BUF_FEATURES, bytes);
        }
        if (!p) return;   // refused or out of memory: the error is sticky, nothing is registered
        e->buf[device_id][i][LEGION_BUF_FEATURES] = p;
    }
    e->ext->feature_rows[device_id] = num_ids;
}
// the serving modes published to the trainers, one mode per call (a runner publishes all of them at once: ipc_env_publish_modes)
void IPCEnv_SetAggLastHop(IPCEnv* e, int32_t on) { if (e && e->ext) e->ext->modes.agg_last_hop = on ? 1 : 0; }
int32_t IPCEnv_GetAggLastHop(const IPCEnv* e) { return ext_agg_last_hop(ext_of(e)); }
void IPCEnv_SetAggNorm(IPCEnv* e, int32_t norm) { if (e && e->ext) e->ext->modes.agg_norm = norm; }
int32_t IPCEnv_GetAggNorm(const IPCEnv* e) { return ext_agg_norm(ext_of(e)); }
void IPCEnv_SetSampling(IPCEnv* e, int32_t mode) { if (e && e->ext) e->ext->modes.sampling = mode == kSamplingWeighted ? kSamplingWeighted : mode ? kSamplingDistinct : kSamplingReplace; }
int32_t IPCEnv_GetSampling(const IPCEnv* e) { return ext_sampling(ext_of(e)); }
void IPCEnv_SetSamplingSeed(IPCEnv* e, int32_t on, uint32_t seed) { if (e && e->ext) { e->ext->modes.sampling_seed = on ? seed : 0u; e->ext->modes.sampling_seeded = on ? 1 : 0; } }
int32_t IPCEnv_GetSamplingSeed(const IPCEnv* e, uint32_t* seed) { return ext_sampling_seed(ext_of(e), seed); }
// ... and the words of the _ext2 object: the first setter of a word that is ON creates the object, a 0 on an env without it creates nothing
#define ENV_EXT2_WORD(Name, word, value) \
    void IPCEnv_Set##Name(IPCEnv* e, int32_t v) { if (volatile shmExt2* x = ext2_of(e, (value) != 0)) x->modes.word = (value); } \
    int32_t IPCEnv_Get##Name(const IPCEnv* e) { return ext2_##word(ext2_of(e)); }
ENV_EXT2_WORD(LpDraw, lp_draw, v > 0 ? v : 0)
ENV_EXT2_WORD(WeightedDistinct, weighted_distinct, v ? 1 : 0)
ENV_EXT2_WORD(SharedDraws, shared_draws, v ? 1 : 0)
ENV_EXT2_WORD(EdgeIds, edge_ids, v ? 1 : 0)
ENV_EXT2_WORD(EdgeWeights, edge_weights, v ? 1 : 0)
ENV_EXT2_WORD(AggEdgeWeight, agg_edge_weight, v ? 1 : 0)
#undef ENV_EXT2_WORD
// The edge buffers of a (device, pipe) -- the POOL's, which stays their owner: the env exports their handles into _ext2 and records how many
// elements each holds.  A buffer above the HIP-IPC size limit is refused by name, as ipc_alloc refuses one (the chunked path is the feature buffer's).
void IPCEnv_RegisterEdgeBuffers(IPCEnv* e, int32_t device_id, int32_t pipe, int64_t* ids, float* w, int32_t elems)
{
    if (!e || device_id < 0 || device_id >= e->device_count || pipe < 0 || pipe >= LEGION_PIPELINE_DEPTH || elems < 1) { LEGION_ARG_ERROR("IPCEnv_RegisterEdgeBuffers: bad arguments"); return; }
    if (!no_device()) {
        if (!ids) { LEGION_ARG_ERROR("IPCEnv_RegisterEdgeBuffers: null edge_ids buffer (GPUMemoryPool_SetEdgeIds first)"); return; }
        if (!ipc_size_ok((int64_t)elems * (int64_t)sizeof(int64_t), "IPCEnv_RegisterEdgeBuffers (edge_ids: 8 bytes per edge slot of one pipe)")) {
            if (!error_is_fatal()) return;
            fflush(stderr);
            exit(EXIT_FAILURE);
        }
    }
    volatile shmExt2* x = ext2_of(e, true);
    if (!x) return;
    if (!no_device()) {     // device-free: the handle slots stay zero
        LEGION_DEVICE_GUARD(device_id);
        HIP_CHECK(hipIpcGetMemHandle((hipIpcMemHandle_t*)&x->edge_handle[device_id][pipe][0], ids));
        if (w) HIP_CHECK(hipIpcGetMemHandle((hipIpcMemHandle_t*)&x->edge_handle[device_id][pipe][1], w));
    }
    x->edge_elems[device_id] = elems;
}
int32_t IPCEnv_GetEdgeElems(const IPCEnv* e, int32_t device_id) { return ext2_edge_elems(ext2_of(e), device_id); }
// the row capacity published to the trainers of a device (a server that re-sizes its feature buffers; tests)
void IPCEnv_SetFeatureRows(IPCEnv* e, int32_t device_id, int32_t rows)
{
    if (e && e->ext && device_id >= 0 && device_id < e->device_count) e->ext->feature_rows[device_id] = rows;
}
// nc[word] (word < kWords) or ec[word - kWords] of the batch about to be posted on (dev, pipe), from the host mirror IPCEnv_MirrorCounters queued (the caller has waited for
// that copy); -1 when the mirror of this batch was not queued
int32_t IPCEnv_MirroredNodeCounter(IPCEnv* e, int32_t dev_id, int32_t current_pipe, int32_t word)
{
    if (!e || !e->ext || dev_id < 0 || dev_id >= e->device_count || word < 0 || word >= 2 * kWords) return -1;
    const int q = current_pipe % e->pipeline_depth;
    if (!e->mirror_fresh[dev_id][q]) return -1;
    if (!e->shm_pinned) return e->mirror_stage[dev_id][q] ? e->mirror_stage[dev_id][q][word] : -1;
    return e->ext->counters[dev_id][q][word];
}

int32_t IPCEnv_GetRawBatchsize(IPCEnv* e) { return e->raw_batch_size; }

// GetLocalBatchId, CUDA_IPC_Service.cu:219-233
int32_t IPCEnv_GetLocalBatchId(IPCEnv* e, int32_t global_batch_id)
{
    int32_t local_batch_id = -1;
    if (global_batch_id < ((e->train_step + e->valid_step) * e->epoch)) {
        int32_t epoch_batch_id = global_batch_id % (e->train_step + e->valid_step);
        local_batch_id = (epoch_batch_id < e->train_step) ? epoch_batch_id : epoch_batch_id - e->train_step;
    } else {
        local_batch_id = (global_batch_id - ((e->train_step + e->valid_step) * e->epoch)) % e->test_step;
    }
    return local_batch_id;
}

// GetCurrentBatchsize, CUDA_IPC_Service.cu:235-243
int32_t IPCEnv_GetCurrentBatchsize(IPCEnv* e, int32_t dev_id, int32_t current_mode)
{
    if (current_mode == LEGION_TRAINMODE) return e->train_batch_size[dev_id];
    if (current_mode == LEGION_VALIDMODE) return e->valid_batch_size[dev_id];
    return e->test_batch_size[dev_id];
}

// GetCurrentMode, CUDA_IPC_Service.cu:246-259
int32_t IPCEnv_GetCurrentMode(IPCEnv* e, int32_t global_batch_id)
{
    if (global_batch_id < ((e->train_step + e->valid_step) * e->epoch)) {
        int32_t epoch_batch_id = global_batch_id % (e->train_step + e->valid_step);
        return (epoch_batch_id < e->train_step) ? LEGION_TRAINMODE : LEGION_VALIDMODE;
    }
    return LEGION_TESTMODE;
}

// a slot that was never registered (a device without InitializeSamplesBuffer, the feature slot before InitializeFeaturesBuffer) reads as null
#define ENV_GETTER(name, slot, type) \
    type* IPCEnv_Get##name(IPCEnv* e, int32_t dev_id, int32_t current_pipe) { \
        if (!e || dev_id < 0 || dev_id >= e->device_count) return nullptr; \
        return (type*)(e->buf[dev_id][current_pipe % e->pipeline_depth][slot]); }
ENV_GETTER(Ids, LEGION_BUF_IDS, int32_t)
ENV_GETTER(FloatFeatures, LEGION_BUF_FEATURES, float)
ENV_GETTER(Labels, LEGION_BUF_LABELS, int32_t)
ENV_GETTER(AggSrc, LEGION_BUF_AGG_SRC, int32_t)
ENV_GETTER(AggDst, LEGION_BUF_AGG_DST, int32_t)
ENV_GETTER(NodeCounter, LEGION_BUF_NODE_COUNTER, int32_t)
ENV_GETTER(EdgeCounter, LEGION_BUF_EDGE_COUNTER, int32_t)
#undef ENV_GETTER

// Queue the copy of the pipe's counters into the host mirror on `stream`, behind the kernels that wrote them.  The caller posts the
// pipe only after it has waited for that stream's work (the runner waits for an event recorded behind this call).
void IPCEnv_MirrorCounters(IPCEnv* e, int32_t dev_id, int32_t current_pipe, void* stream)
{
    if (!e || !e->ext || dev_id < 0 || dev_id >= e->device_count || !e->pipes[dev_id] || no_device()) return;
    const int q = current_pipe % e->pipeline_depth;
    int32_t* m = (int32_t*)&e->ext->counters[dev_id][q][0];
    if (!e->shm_pinned) {           // the runtime refused to page-lock the slab: queue the copies into pinned staging words, IPCPost moves them
        if (!e->mirror_stage[dev_id][q] && hipHostMalloc((void**)&e->mirror_stage[dev_id][q], 2 * kCounterBytes, hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            e->mirror_stage[dev_id][q] = nullptr;
            return;                 // IPCPost copies synchronously instead
        }
        m = e->mirror_stage[dev_id][q];
    }
    HIP_CHECK(hipMemcpyAsync(m, e->buf[dev_id][q][LEGION_BUF_NODE_COUNTER], kCounterBytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_CHECK(hipMemcpyAsync(m + kWords, e->buf[dev_id][q][LEGION_BUF_EDGE_COUNTER], kCounterBytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    e->mirror_fresh[dev_id][q] = true;
}
int IPCEnv_SlabPinned(IPCEnv* e) { return e && e->shm_pinned ? 1 : 0; }
// The mirror of a pipe whose counters the HOST decides (a poisoned pipe: nc[*] = -1, ec[*] = 0)
void IPCEnv_SetMirror(IPCEnv* e, int32_t dev_id, int32_t current_pipe, int32_t nc_fill, int32_t ec_fill)
{
    if (!e || !e->ext || dev_id < 0 || dev_id >= e->device_count) return;
    const int q = current_pipe % e->pipeline_depth;
    for (int i = 0; i < kWords; i++) { e->ext->counters[dev_id][q][i] = nc_fill; e->ext->counters[dev_id][q][kWords + i] = ec_fill; }
    if (e->mirror_stage[dev_id][q]) for (int i = 0; i < 2 * kWords; i++) e->mirror_stage[dev_id][q][i] = i < kWords ? nc_fill : ec_fill;
    e->mirror_fresh[dev_id][q] = true;
}
void IPCEnv_IPCPost(IPCEnv* e, int32_t dev_id, int32_t current_pipe)
{
    const int q = current_pipe % e->pipeline_depth;
    if (e->ext && e->mirror_fresh[dev_id][q] && !e->shm_pinned && e->mirror_stage[dev_id][q])     // staged by a queued copy the caller has waited for
        copy_counters(e->ext->counters[dev_id][q], e->mirror_stage[dev_id][q]);
    if (e->ext && e->ext->mirror_magic == kMirrorMagic && !e->mirror_fresh[dev_id][q] && e->pipes[dev_id] && !no_device()) {
        // a producer that did not queue the mirror copy (a reference-style RunOnce on this library): copy now -- the batch is
        // complete when a pipe is posted, so a blocking copy is correct, merely slower than the queued one
        DeviceGuard guard(dev_id);
        int32_t h[2 * kWords];
        if (hipMemcpy(h, e->buf[dev_id][q][LEGION_BUF_NODE_COUNTER], kCounterBytes, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(h + kWords, e->buf[dev_id][q][LEGION_BUF_EDGE_COUNTER], kCounterBytes, hipMemcpyDeviceToHost) == hipSuccess)
            copy_counters(e->ext->counters[dev_id][q], h);
        else { (void)hipGetLastError(); e->ext->mirror_magic = 0; }   // clients fall back to the device buffers
    }
    e->mirror_fresh[dev_id][q] = false;
    if (e->semw[dev_id][q]) sem_post(e->semw[dev_id][q]);
}
void IPCEnv_IPCWait(IPCEnv* e, int32_t dev_id, int32_t current_pipe)
{
    sem_t* sem = e->semr[dev_id][current_pipe % e->pipeline_depth];
    if (!sem) return;      // sem_open failed (sticky error): never block on a semaphore that does not exist
    sem_wait_spin(sem);
}
int IPCEnv_HandoffSpinUs(void) { return handoff_spin_us(); }
int IPCEnv_IPCTryWait(IPCEnv* e, int32_t dev_id, int32_t current_pipe, int32_t timeout_ms)
{
    if (timeout_ms <= 0) {     // a pure poll: no clock, no syscall beyond the futex word
        sem_t* sem0 = e->semr[dev_id][current_pipe % e->pipeline_depth];
        return (sem0 && sem_trywait(sem0) == 0) ? 0 : -1;
    }
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    ts.tv_sec += timeout_ms / 1000;
    ts.tv_nsec += (long)(timeout_ms % 1000) * 1000000L;
    if (ts.tv_nsec >= 1000000000L) { ts.tv_sec++; ts.tv_nsec -= 1000000000L; }
    int r;
    sem_t* sem = e->semr[dev_id][current_pipe % e->pipeline_depth];
    if (!sem) return -1;
    while ((r = sem_timedwait(sem, &ts)) != 0 && errno == EINTR) {}
    return r == 0 ? 0 : -1;
}

// Finalize, CUDA_IPC_Service.cu:299-325
void IPCEnv_Finalize(IPCEnv* e)
{
    if (!e) return;
    for (int32_t i = 0; i < e->device_count; i++) {
        if (!e->pipes[i]) continue;
        LEGION_DEVICE_GUARD(i);
        for (int32_t j = 0; j < e->pipes[i]; j++) {
            if (!no_device())        // device-free: nothing was allocated, only the semaphores exist
                for (void*& p : e->buf[i][j]) {
                    // a chunked feature buffer goes with its region below
                    if (std::none_of(e->vmm.begin(), e->vmm.end(), [&](const VmmRegion* r) { return vmm_va(r) == p; })) (void)hipFree(p);
                    p = nullptr;
                }
            if (!sem_pair_close(e->semr[i][j], e->semw[i][j])) log_out() << "close sem " << i << " " << j << " failed\n";
            sem_pair_unlink(i, j);
        }
        e->pipes[i] = 0;
    }
    for (VmmRegion* r : e->vmm) vmm_release(r);
    e->vmm.clear();
    if (e->shm) {
        if (e->shm_pinned && e->ext) { (void)hipHostUnregister((void*)e->ext); e->shm_pinned = false; }
        for (auto& dev : e->mirror_stage) for (auto& p : dev) if (p) { (void)hipHostFree(p); p = nullptr; }
        munmap((void*)e->shm, sizeof(shmStruct));
        close(e->shm_fd);
        shm_unlink(shm_name().c_str());
        e->shm = nullptr;
        if (e->ext) { munmap((void*)e->ext, sizeof(shmExt)); close(e->ext_fd); shm_unlink(ext_name().c_str()); e->ext = nullptr; }
        if (e->ext2) { munmap((void*)e->ext2, sizeof(shmExt2)); close(e->ext2_fd); e->ext2 = nullptr; }
        shm_unlink(ext2_name().c_str());
    }
}

int32_t IPCEnv_GetTrainStep(IPCEnv* e) { return e->train_step; }
// the round (epoch) a global batch belongs to: global_batch_id / (train + validation steps), so test batches get a round >= epochs
int32_t IPCEnv_GetRound(IPCEnv* e, int32_t global_batch_id)
{
    const int32_t per = e ? e->train_step + e->valid_step : 0;
    return per > 0 && global_batch_id >= 0 ? global_batch_id / per : 0;
}
void IPCEnv_SetHops(IPCEnv* e, int32_t hops) { if (e && e->ext) e->ext->hops = hops; }

} // extern "C"
