// ipc_client.cpp -- the trainer half of the hand-off (ipc_shm.h): GPUIPCEnv, pytorch_extension/ipc_cuda_kernel.cu:36-176.
#include "ipc_shm.h"

#include <cstring>
#include <sys/mman.h>
#include <unistd.h>

#include "audit_hooks.h"

using namespace legion;

struct LegionIPCClient {
    volatile shmStruct* shm = nullptr;
    int shm_fd = -1;
    volatile shmExt* ext = nullptr;    // null: the server has no extension object (a reference server): hops = 2, counters by device copy
    int ext_fd = -1;
    volatile shmExt2* ext2 = nullptr;  // null: the server has no "_ext2" object (none of its words is on, or an older server), or a stale one: every word reads 0
    int ext2_fd = -1;
    void* edge[LEGION_PIPELINE_DEPTH][2] = {};   // the served edge buffers: [0] = edge_ids int64, [1] = edge_w float32; null = not served
    int device = 0;
    void* buf[LEGION_PIPELINE_DEPTH][LEGION_MEMORY_USAGE] = {};   // the last index: LEGION_BUF_*
    sem_t* semr[LEGION_PIPELINE_DEPTH] = {};
    sem_t* semw[LEGION_PIPELINE_DEPTH] = {};
    int32_t steps[3] = {0, 0, 0};
    int32_t hops = 2;
    int current_pipe = 0;
    VmmMapping mapped[LEGION_PIPELINE_DEPTH];   // feature buffers that arrived as chunk descriptors (see VmmDesc): what to unmap / release on close
};

static const volatile shmExt* ext_of(const LegionIPCClient* c) { return c ? c->ext : nullptr; }
static const volatile shmExt2* ext2_of(const LegionIPCClient* c) { return c ? c->ext2 : nullptr; }
// why a client is refused: close what was opened, post nothing, and let `msg` be the error the caller reads
static LegionIPCClient* refuse(LegionIPCClient* c, const char* msg)
{
    legion_ipc_client_close(c);
    legion_clear_error();
    LEGION_ARG_ERROR(msg);
    return nullptr;
}

extern "C" {

// GPUIPCEnv::Initialize, ipc_cuda_kernel.cu:38-96.  device_id < 0: use the current device
// (the reference reads cudaGetDevice(), set by torch.cuda.set_device(rank) in the trainer).
LegionIPCClient* legion_ipc_client_open(int32_t device_id)
{
    LegionIPCClient* c = new LegionIPCClient();
    int cur = 0;
    if (!no_device()) HIP_CHECK(hipGetDevice(&cur));
    c->device = device_id >= 0 ? device_id : cur;
    // $LEGION_IPC_DEVICE: logical GPU (row of the shm handle table) when it differs from the physical device,
    // e.g. several logical GPUs of a clique exercised on one physical device
    if (device_id < 0 && getenv("LEGION_IPC_DEVICE")) c->device = atoi(getenv("LEGION_IPC_DEVICE"));
    c->shm = (volatile shmStruct*)shm_map(sizeof(shmStruct), &c->shm_fd);
    if (!c->shm) { fprintf(log_file(), "Failed to create shared memory slab\n"); delete c; LEGION_ARG_ERROR("legion_ipc_client_open: shm"); return nullptr; }
    c->ext = (volatile shmExt*)shm_map(sizeof(shmExt), &c->ext_fd, ext_name(), false);     // never created by a client
    for (int i = 0; i < 3; i++) c->steps[i] = c->shm->steps[i];
    if (c->device >= LEGION_MAX_DEVICE) { LEGION_ARG_ERROR("legion_ipc_client_open: device id >= 8"); delete c; return nullptr; }
    // an extension object that does not belong to the slab we attached to (left behind by a killed server, the slab re-created by a server
    // without the extension): ignore it -- 2 hops, counters by device copy, no row bound: the reference's behaviour
    if (c->ext && (c->ext->steps_copy[0] != c->steps[0] || c->ext->steps_copy[1] != c->steps[1] || c->ext->steps_copy[2] != c->steps[2] ||
                   c->ext->handle_sum[c->device] != handle_checksum(&c->shm->memHandle[c->device][0][LEGION_BUF_IDS]))) {
        munmap((void*)c->ext, sizeof(shmExt));
        close(c->ext_fd);
        c->ext = nullptr; c->ext_fd = -1;
    }
    c->hops = (c->ext && c->ext->hops > 0) ? c->ext->hops : 2;
    // the second extension object, likewise never created here and likewise ignored unless it belongs to this slab
    c->ext2 = (volatile shmExt2*)shm_map(sizeof(shmExt2), &c->ext2_fd, ext2_name(), false);
    if (c->ext2 && !ext2_tied(c->ext2, c->shm, c->device)) {
        munmap((void*)c->ext2, sizeof(shmExt2));
        close(c->ext2_fd);
        c->ext2 = nullptr; c->ext2_fd = -1;
    }
    // feature buffers that arrive as chunk descriptors first: they need the server's socket, the one step that depends on a second party
    for (int i = 0; i < LEGION_PIPELINE_DEPTH; i++) {
        hipIpcMemHandle_t h;
        memcpy(&h, (const void*)&c->shm->memHandle[c->device][i][LEGION_BUF_FEATURES], sizeof(h));
        if (memcmp(&h, kVmmMagic, sizeof(kVmmMagic)) != 0) continue;
        VmmDesc d;
        memcpy(&d, &h, sizeof(d));
        c->buf[i][LEGION_BUF_FEATURES] = vmm_attach(c->device, i, d, c->mapped[i]);
        if (!c->buf[i][LEGION_BUF_FEATURES]) {   // no trainer may run on a null feature buffer: close what was opened, post nothing
            legion_ipc_client_close(c);
            return nullptr;
        }
    }
    for (int i = 0; i < LEGION_PIPELINE_DEPTH; i++) {
        for (int w = 0; w < LEGION_MEMORY_USAGE; w++) {
            if (c->buf[i][w]) continue;      // attached above
            hipIpcMemHandle_t h;
            memcpy(&h, (const void*)&c->shm->memHandle[c->device][i][w], sizeof(h));
            static const hipIpcMemHandle_t zero{};
            if (memcmp(&h, &zero, sizeof(h)) == 0) {
                if (no_device()) continue;                       // the device-free test mode registers no buffers at all
                // The server has not registered this buffer yet: the sample buffers appear in Runner_Initialize, the FEATURE buffers only
                // after the pre-sampling epoch (Server.cu:33,273-282).  A trainer that attaches now would run on a null buffer and fault
                // on the GPU in its first kernel; the reference fails in cudaIpcOpenMemHandle here.  Refuse, by name.
                char msg[256];
                snprintf(msg, sizeof(msg), "legion_ipc_client_open: the server has not registered buffer %d of pipe %d of GPU %d yet "
                         "(start the trainer after \"System is ready for serving\")", w, i, c->device);
                return refuse(c, msg);
            }
            HIP_CHECK(hipIpcOpenMemHandle(&c->buf[i][w], h, hipIpcMemLazyEnablePeerAccess));
        }
    }
    // the served edge buffers of this device (LEGION_EDGE_IDS=1): a server that says so has registered them before it is ready for serving
    if (ext2_edge_ids(c->ext2) && !no_device()) {
        char msg[256];
        snprintf(msg, sizeof(msg), "legion_ipc_client_open: the server serves edge ids (LEGION_EDGE_IDS=1) but registered no edge buffers for GPU %d "
                 "(IPCEnv_RegisterEdgeBuffers; start the trainer after \"System is ready for serving\")", c->device);
        if (ext2_edge_elems(c->ext2, c->device) <= 0) return refuse(c, msg);
        for (int i = 0; i < LEGION_PIPELINE_DEPTH; i++)
            for (int w = 0; w < 2; w++) {
                hipIpcMemHandle_t h;
                if (!ext2_edge_handle(c->ext2, c->device, i, w, &h)) {
                    if (w == 0) return refuse(c, msg);
                    continue;      // no weights buffer: edge ids alone
                }
                HIP_CHECK(hipIpcOpenMemHandle(&c->edge[i][w], h, hipIpcMemLazyEnablePeerAccess));
            }
    }
    log_out() << "HIP: " << c->device << " IPC shared memory opened\n";
    for (int i = 0; i < LEGION_PIPELINE_DEPTH; i++) {
        if (!sem_pair_open(c->device, i, false, c->semr[i], c->semw[i], "legion_ipc_client_open: sem_open", "legion_ipc_client_open: sem_open")) { legion_ipc_client_close(c); return nullptr; }
        sem_post(c->semr[i]); // both pipes start free (ipc_cuda_kernel.cu:91)
    }
    c->current_pipe = 0;
    return c;
}

void legion_ipc_client_wait(LegionIPCClient* c)
{
    sem_wait_spin(c->semw[c->current_pipe]);
}
// Post(): the pipe's buffers go back to the server, which overwrites them with batch i + 2.  The reference's trainer never
// synchronises its device around synchronize() (legion_graphsage.py:93-116): what bounded its run-ahead was the BLOCKING counter copy of
// the next get_next (ipc_cuda_kernel.cu:195-196, legacy default stream: waits for everything the trainer has queued).  Here get_next reads
// the host mirror and synchronises nothing, so the wait moves to where it is needed: everything this process has queued on its device --
// kernels still reading the batch's ids / rows / COO -- completes BEFORE the semaphore is posted.  One device synchronisation per batch,
// as in the reference, and the pipe is really free when the server sees it.
void legion_ipc_client_post(LegionIPCClient* c)
{
    if (!no_device()) HIP_CHECK(hipDeviceSynchronize());
    legion_ipc_client_post_nosync(c);
}
// ... for a consumer that has already waited for its own work (an event / stream synchronisation of its own, or no device work at all)
void legion_ipc_client_post_nosync(LegionIPCClient* c)
{
    sem_post(c->semr[c->current_pipe]);
    c->current_pipe = (c->current_pipe + 1) % LEGION_PIPELINE_DEPTH;
}
void* legion_ipc_client_buffer(LegionIPCClient* c, int32_t which)
{
    if (!c || which < 0 || which >= LEGION_MEMORY_USAGE) return nullptr;
    return c->buf[c->current_pipe][which];
}
void legion_ipc_client_steps(LegionIPCClient* c, int32_t steps[3])
{
    for (int i = 0; i < 3; i++) steps[i] = c->steps[i];
}
int32_t legion_ipc_client_hops(LegionIPCClient* c) { return c->hops; }
int32_t legion_ipc_client_agg_last_hop(LegionIPCClient* c) { return ext_agg_last_hop(ext_of(c)); }
int32_t legion_ipc_client_agg_norm(LegionIPCClient* c) { return ext_agg_norm(ext_of(c)); }
int32_t legion_ipc_client_sampling(LegionIPCClient* c) { return ext_sampling(ext_of(c)); }
int32_t legion_ipc_client_sampling_seed(LegionIPCClient* c, uint32_t* seed) { return ext_sampling_seed(ext_of(c), seed); }
int32_t legion_ipc_client_lp_draw(LegionIPCClient* c) { return ext2_lp_draw(ext2_of(c)); }
int32_t legion_ipc_client_weighted_distinct(LegionIPCClient* c) { return ext2_weighted_distinct(ext2_of(c)); }
int32_t legion_ipc_client_shared_draws(LegionIPCClient* c) { return ext2_shared_draws(ext2_of(c)); }
int32_t legion_ipc_client_edge_ids(LegionIPCClient* c) { return ext2_edge_ids(ext2_of(c)); }
int32_t legion_ipc_client_edge_weights(LegionIPCClient* c) { return ext2_edge_weights(ext2_of(c)); }
int32_t legion_ipc_client_agg_edge_weight(LegionIPCClient* c) { return ext2_agg_edge_weight(ext2_of(c)); }
void* legion_ipc_client_edge_buffer(LegionIPCClient* c, int32_t which)
{
    if (!c || which < 0 || which > 1 || !ext2_edge_ids(c->ext2) || (which == 1 && !ext2_edge_weights(c->ext2))) return nullptr;
    return c->edge[c->current_pipe][which];
}
int32_t legion_ipc_client_edge_elems(LegionIPCClient* c) { return c ? ext2_edge_elems(c->ext2, c->device) : 0; }
int32_t legion_ipc_client_feature_rows(LegionIPCClient* c) { return (c && c->ext) ? c->ext->feature_rows[c->device] : 0; }
void legion_ipc_client_read_counters(LegionIPCClient* c, int32_t h_node_counter[LEGION_COUNTER_WORDS], int32_t h_edge_counter[LEGION_COUNTER_WORDS])
{
    if (c->ext && c->ext->mirror_magic == kMirrorMagic) {
        // the server's host mirror of this pipe: no device copy, no implicit synchronisation with the trainer's own GPU work
        const volatile int32_t* m = &c->ext->counters[c->device][c->current_pipe][0];
        for (int i = 0; i < kWords; i++) { h_node_counter[i] = m[i]; h_edge_counter[i] = m[kWords + i]; }
        return;
    }
    HIP_CHECK(hipMemcpy(h_node_counter, c->buf[c->current_pipe][LEGION_BUF_NODE_COUNTER], kCounterBytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(h_edge_counter, c->buf[c->current_pipe][LEGION_BUF_EDGE_COUNTER], kCounterBytes, hipMemcpyDeviceToHost));
}
void legion_ipc_client_close(LegionIPCClient* c)
{
    if (!c) return;
    for (int i = 0; i < LEGION_PIPELINE_DEPTH; i++) {
        for (int w = 0; w < LEGION_MEMORY_USAGE; w++) {
            if (!c->buf[i][w]) continue;
            if (c->mapped[i].va == c->buf[i][w]) vmm_unmap(c->mapped[i]);
            else (void)hipIpcCloseMemHandle(c->buf[i][w]);
        }
        for (void*& p : c->edge[i]) { if (p) (void)hipIpcCloseMemHandle(p); p = nullptr; }
        if (!sem_pair_close(c->semr[i], c->semw[i])) log_out() << "close sem " << i << " failed\n";
    }
    if (c->shm) { munmap((void*)c->shm, sizeof(shmStruct)); close(c->shm_fd); }
    if (c->ext) { munmap((void*)c->ext, sizeof(shmExt)); close(c->ext_fd); }
    if (c->ext2) { munmap((void*)c->ext2, sizeof(shmExt2)); close(c->ext2_fd); }
    delete c;
}

} // extern "C"
