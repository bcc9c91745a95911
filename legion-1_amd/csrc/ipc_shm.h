// ipc_shm.h -- what the two halves of the server <-> trainer hand-off must agree on, and nothing else: the shared-memory
// objects (the slab, "_ext" and, only when a server has something to put there, "_ext2"), their names, the semaphore pair of a (device, pipe) and the chunk descriptor of a buffer above the HIP-IPC size limit.
//   server half : ipc_env.cpp     CUDAIPCEnv            src/CUDA_IPC_Service.cu:39-360
//   trainer half: ipc_client.cpp  GPUIPCEnv             pytorch_extension/ipc_cuda_kernel.cu:36-176
//   shm helpers : ipc_shm.cpp     helper_multiprocess   src/helper_multiprocess.cpp:5-100
//   chunked hand-off buffer, both sides: ipc_vmm.cpp
// Contract kept byte for byte: POSIX shm "simpleIPCshm" holding
//   struct { int32 steps[3]; ipcMemHandle[8 dev][2 pipe][7 buf]; }   (12 + 8*2*7*64 = 7180 B;
// hipIpcMemHandle_t is 64 bytes like cudaIpcMemHandle_t), named semaphores sem_r_D_P / sem_w_D_P
// with initial value 0, producer: wait(sem_r) -> fill -> post(sem_w); consumer: wait(sem_w) ->
// use -> post(sem_r).  Extensions (hop count, counter mirror, feature-buffer rows) live in a SECOND shm
// object "<name>_ext" (shmExt below): the shared slab itself is exactly the reference's 7180 bytes.
#pragma once
#include "internal.h"

#include <cstddef>
#include <optional>
#include <semaphore.h>

namespace legion {

constexpr int kWords = LEGION_COUNTER_WORDS;                   // one counter array (nc or ec); the mirror holds nc | ec
constexpr size_t kCounterBytes = kWords * sizeof(int32_t);

static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle must be 64 bytes (CUDA_IPC_Service.cu:34-37)");

struct shmStruct {           // the reference's slab, byte for byte (CUDA_IPC_Service.cu:34-37, ipc_cuda_kernel.cu:31-34): 7180 bytes, nothing appended
    int32_t steps[3];
    hipIpcMemHandle_t memHandle[LEGION_MAX_DEVICE][LEGION_PIPELINE_DEPTH][LEGION_MEMORY_USAGE];   // the last index: LEGION_BUF_*
};
static_assert(sizeof(shmStruct) == 12 + 8 * 2 * 7 * 64, "the reference's shm layout is 7180 bytes");
// Everything this implementation adds lives in a SECOND shm object, "<name>_ext".  Rounds 1-4 appended it behind the reference struct in the
// same object; but the reference's trainer opens the slab with sharedMemoryCreate (ipc_cuda_kernel.cu:45 -> helper_multiprocess.cpp:35), which
// ftruncate()s it to ITS 7180 bytes -- cutting the appended words off under a running server (a SIGBUS on their next touch beyond the page).
// With a separate object the shared one is exactly the reference's, whoever creates or truncates it (tests/test_ref_shm_compat.py drives the
// reference's own helper against it).  A peer without the extension object simply does not find it: hops = 2, counters by device copy.
struct shmExt {
    uint32_t mirror_magic;    // kMirrorMagic: the server maintains the counter mirror below
    int32_t hops;             // number of hops the server samples (0: not told -> 2, the reference's layout)
    // rows the feature buffers of a device hold (InitializeFeaturesBuffer; 0 = not told).  The reference sizes them at 1.2 x the largest batch
    // of the pre-sampling epoch (Server.cu:275) and its trainer views [nc9, F] of them unchecked (ipc_cuda_kernel.cu:200): a batch with more
    // nodes reads past the allocation.  A client that knows the capacity refuses such a batch instead.
    int32_t feature_rows[LEGION_MAX_DEVICE];
    // host mirror of the two counter arrays of every (device, pipe), filled by the server before it posts the pipe.  The reference's
    // trainer reads them with a blocking cudaMemcpy from the IPC device buffers (ipc_cuda_kernel.cu:195-196): on the legacy default stream that
    // copy waits for everything the trainer has queued.  A client that finds the magic set reads the mirror instead; the two counter buffers stay valid.
    int32_t counters[LEGION_MAX_DEVICE][LEGION_PIPELINE_DEPTH][2 * kWords];   // nc | ec
    // What ties this object to the LIVE slab: the object is only unlinked by IPCEnv_Finalize, so after a killed server a server WITHOUT the
    // extension (the reference's) would leave a stale one in place and a client would read stale hops / counters for good.  The server stores
    // a copy of the slab's step counts and a checksum of the first handle it registers per device; a client ignores an extension that does not
    // match the slab it attached to (it then behaves as against a reference server).
    int32_t steps_copy[3];
    uint32_t handle_sum[LEGION_MAX_DEVICE];   // FNV-1a of memHandle[dev][0][LEGION_BUF_IDS]; 0 = nothing registered for that device yet
    // The serving modes (ServeModes, internal.h), appended behind everything older peers know, one word per mode as the modes came: the
    // fields above do not move and the object stays inside its one page, so a client of an older server reads 0 ("off") in every word it
    // knows and an older client never looks at the later ones.  Written by IPCEnv_Set* / ipc_env_publish_modes, read through ext_* below.
    struct Modes {
        int32_t agg_last_hop;     // 1 = the last hop is handed over as neighbour sums: feature rows [0, n_in) are features, rows [n_in, n_in + N) the sums
        int32_t agg_norm;         // how such a server normalises the sums: 0 = plain sums, 1 = every row scaled by its out-degree^-1/2 inside block 1
        int32_t sampling;         // how the server's sampler draws: 0 = with replacement (the reference's stream), 1 = distinct neighbours, 2 = by edge weight
        int32_t sampling_seeded;  // 0 = the reference's draws, the same batches every epoch; 1 = fresh draws per batch, the training list reshuffled per epoch ...
        uint32_t sampling_seed;   // ... under this seed.  Seed 0 is a seed: the flag says whether there is one
    } modes;
};
// Peers of other builds map this object, and the reference's trainer maps the slab: every field stays where the first build that had it
// put it (the mode words: 32-bit words 533 .. 537)
static_assert(offsetof(shmStruct, steps) == 0 && offsetof(shmStruct, memHandle) == 12, "the slab's fields moved");
static_assert(offsetof(shmExt, mirror_magic) == 0 && offsetof(shmExt, hops) == 4 && offsetof(shmExt, feature_rows) == 8 && offsetof(shmExt, counters) == 40 &&
              offsetof(shmExt, steps_copy) == 2088 && offsetof(shmExt, handle_sum) == 2100, "a field of the _ext object moved");
static_assert(offsetof(shmExt, modes.agg_last_hop) == 2132 && offsetof(shmExt, modes.agg_norm) == 2136 && offsetof(shmExt, modes.sampling) == 2140 &&
              offsetof(shmExt, modes.sampling_seeded) == 2144 && offsetof(shmExt, modes.sampling_seed) == 2148 && sizeof(shmExt) == 2152,
              "the mode words of the _ext object moved");
constexpr uint32_t kMirrorMagic = 0x4C474E43u;   // "LGNC"
uint32_t handle_checksum(const volatile void* h);

// The one reader of each mode word, for the server's IPCEnv_Get* and the trainer's legion_ipc_client_*.  No extension object: every mode off.
inline int32_t ext_agg_last_hop(const volatile shmExt* x) { return x ? x->modes.agg_last_hop : 0; }
inline int32_t ext_agg_norm(const volatile shmExt* x) { return x ? x->modes.agg_norm : 0; }
inline int32_t ext_sampling(const volatile shmExt* x) { return x ? x->modes.sampling : 0; }
inline int32_t ext_sampling_seed(const volatile shmExt* x, uint32_t* seed)
{
    const bool on = x && x->modes.sampling_seeded;
    if (seed) *seed = on ? x->modes.sampling_seed : 0u;
    return on ? 1 : 0;
}

// What came after the _ext object was full and pinned: a THIRD object, "<name>_ext2".  The server creates it only when
// something it carries is on -- one of the six mode words below, or registered edge buffers --, so a server with none of them leaves exactly
// the slab, _ext and the semaphores.  A client never creates it; absent, every word reads 0, which is how a client of an older server behaves.
// It only ever grows at the end: `bytes` is the WRITER's sizeof(shmExt2), and a reader trusts only the words below it.
struct shmExt2 {
    uint32_t magic;           // kExt2Magic
    uint32_t bytes;           // sizeof(shmExt2) of the build that wrote it
    int32_t steps_copy[3];    // the tie to the live slab, as in shmExt: a client ignores an object whose copies do not match the slab it
    uint32_t handle_sum[LEGION_MAX_DEVICE];   // attached to (a killed server's object under a later server that has none)
    struct Modes {
        int32_t lp_draw;            // k > 0 = a training batch is 3 k seeds whose pos and neg thirds the server draws per batch; 0 = off
        int32_t weighted_distinct;  // 1 = the weighted draws are without replacement (`sampling` in _ext stays 2)
        int32_t shared_draws;       // 1 = the distinct draws go by a key of the neighbour node
        int32_t edge_ids;           // 1 = every sampled edge's position in the whole CSR is served in edge_handle[..][0]
        int32_t edge_weights;       // 1 = edge_w is filled (the graph retains its weights), served in edge_handle[..][1]
        int32_t agg_edge_weight;    // 1 = the last hop's sums scale every row by its draw's edge weight
    } modes;
    int32_t edge_elems[LEGION_MAX_DEVICE];    // elements each edge buffer of a device holds (GPUMemoryPool_NumIds); 0 = none registered
    hipIpcMemHandle_t edge_handle[LEGION_MAX_DEVICE][LEGION_PIPELINE_DEPTH][2];   // [..][0] = edge_ids int64, [..][1] = edge_w float32
};
static_assert(offsetof(shmExt2, magic) == 0 && offsetof(shmExt2, bytes) == 4 && offsetof(shmExt2, steps_copy) == 8 && offsetof(shmExt2, handle_sum) == 20 &&
              offsetof(shmExt2, modes.lp_draw) == 52 && offsetof(shmExt2, modes.weighted_distinct) == 56 && offsetof(shmExt2, modes.shared_draws) == 60 &&
              offsetof(shmExt2, modes.edge_ids) == 64 && offsetof(shmExt2, modes.edge_weights) == 68 && offsetof(shmExt2, modes.agg_edge_weight) == 72 &&
              offsetof(shmExt2, edge_elems) == 76 && offsetof(shmExt2, edge_handle) == 108 && sizeof(shmExt2) == 108 + 8 * 2 * 2 * 64,
              "a field of the _ext2 object moved");
constexpr uint32_t kExt2Magic = 0x4C474E32u;   // "LGN2"
// whether the object belongs to the slab a peer attached to (and was written by a build that knows the tie)
bool ext2_tied(const volatile shmExt2* x, const volatile shmStruct* shm, int dev);
// The one reader of each word, beside ext_*: no object, or a writer that ended before the word, reads 0
#define LEGION_EXT2_WORD(name) \
    inline int32_t ext2_##name(const volatile shmExt2* x) { return x && x->bytes >= offsetof(shmExt2, modes.name) + sizeof(int32_t) ? x->modes.name : 0; }
LEGION_EXT2_WORD(lp_draw) LEGION_EXT2_WORD(weighted_distinct) LEGION_EXT2_WORD(shared_draws)
LEGION_EXT2_WORD(edge_ids) LEGION_EXT2_WORD(edge_weights) LEGION_EXT2_WORD(agg_edge_weight)
#undef LEGION_EXT2_WORD
inline int32_t ext2_edge_elems(const volatile shmExt2* x, int dev)
{
    return x && dev >= 0 && dev < LEGION_MAX_DEVICE && x->bytes >= offsetof(shmExt2, edge_elems) + sizeof(x->edge_elems) ? x->edge_elems[dev] : 0;
}
// the handle of (dev, pipe, which) into *h; false when the writer ended before the table or the slot is all zero ("no buffer")
bool ext2_edge_handle(const volatile shmExt2* x, int dev, int pipe, int which, hipIpcMemHandle_t* h);

// $LEGION_IPC_NO_DEVICE=1 (test hook: build containers without a GPU, the host-sanitizer run of tests/test_ipc_env_cpu.py): the slab,
// the named semaphores, the counter mirror and the poisoned-pipe protocol with no device call at all -- no hand-off buffer is
// allocated, the handle slots stay zero (a client takes an all-zero handle as "no buffer"), nothing is page-locked.
bool no_device();
#define LEGION_DEVICE_GUARD(dev) std::optional<::legion::DeviceGuard> guard_; if (!::legion::no_device()) guard_.emplace(dev)

// The names of a namespace (a prefix; default: the process's, $LEGION_IPC_NAMESPACE or legion_ipc_set_namespace), read at every call:
// tests switch the namespace inside one process.  "/<ns>simpleIPCshm", "/<ns>simpleIPCshm_ext", "/<ns>simpleIPCshm_ext2", "/<ns>sem_<r|w>_<dev>_<pipe>".
const std::string& ipc_ns();
std::string shm_name(const std::string& ns = ipc_ns());
std::string ext_name(const std::string& ns = ipc_ns());
std::string ext2_name(const std::string& ns = ipc_ns());
std::string sem_name(const char* rw, int dev, int pipe, const std::string& ns = ipc_ns());
// sharedMemoryCreate (helper_multiprocess.cpp:5-47): shm_open(O_RDWR|O_CREAT) + ftruncate + mmap
void* shm_map(size_t sz, int* fd_out, const std::string& name = shm_name(), bool create = true);

// The semaphore pair (sem_r, sem_w) of a (device, pipe), initial value 0.  `fresh` (the server): stale semaphores of a crashed run are
// removed first (the reference only unlinks in Finalize, CUDA_IPC_Service.cu:319-320, so a crash poisons the next start).  False with the
// errno line and the caller's refusal when one cannot be opened; that one and whatever follows it stay null.
bool sem_pair_open(int dev, int pipe, bool fresh, sem_t*& r, sem_t*& w, const char* refuse_r, const char* refuse_w);
bool sem_pair_close(sem_t*& r, sem_t*& w);   // tolerates null and SEM_FAILED; false when closing sem_w failed
void sem_pair_unlink(int dev, int pipe, const std::string& ns = ipc_ns());
int handoff_spin_us();
void sem_wait_spin(sem_t* sem);              // sem_wait with a polling prologue; EINTR-safe

// ---- hand-off buffers above the HIP-IPC size limit (ipc_vmm.cpp) -----------------------------------------------------
struct VmmDesc {               // lives in shmStruct::memHandle[dev][pipe][LEGION_BUF_FEATURES]
    char magic[8];             // "LGNVMM01"
    uint64_t total, chunk;     // bytes mapped, bytes per chunk (the last one may be shorter)
    uint32_t nchunks, pad;
};
static_assert(sizeof(VmmDesc) <= sizeof(hipIpcMemHandle_t), "descriptor must fit the handle slot");
constexpr char kVmmMagic[8] = {'L', 'G', 'N', 'V', 'M', 'M', '0', '1'};
struct VmmMapping {            // chunks mapped back to back into one reserved range: what it takes to give them back
    void* va = nullptr;
    size_t total = 0, chunk = 0;
    std::vector<hipMemGenericAllocationHandle_t> handles;
};
struct VmmRegion;              // server side: one mapped, exported buffer + the thread that serves its descriptors
VmmRegion* vmm_create(int logical_dev, int pipe, size_t bytes);   // nullptr (sticky error) when the platform cannot do it
const VmmDesc& vmm_desc(const VmmRegion* r);
void* vmm_va(const VmmRegion* r);
void vmm_release(VmmRegion* r);                                   // on the region's own device
// trainer side: fetch the descriptors of (dev, pipe), import, map back to back; nullptr with the refusal when that fails, nothing kept
void* vmm_attach(int dev, int pipe, const VmmDesc& want, VmmMapping& m);
void vmm_unmap(VmmMapping& m);                                    // unmap every chunk, release the handles, free the range: m is empty again

} // namespace legion
