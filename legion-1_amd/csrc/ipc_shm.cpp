// ipc_shm.cpp -- the shared-memory objects, names and semaphores of the hand-off (ipc_shm.h), for both halves.
#include "ipc_shm.h"

#include <cerrno>
#include <cstring>
#include <ctime>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace legion {

uint32_t handle_checksum(const volatile void* h)
{
    uint32_t x = 2166136261u;
    const volatile unsigned char* b = (const volatile unsigned char*)h;
    for (size_t i = 0; i < sizeof(hipIpcMemHandle_t); i++) { x ^= b[i]; x *= 16777619u; }
    return x ? x : 1u;
}

bool ext2_tied(const volatile shmExt2* x, const volatile shmStruct* shm, int dev)
{
    if (!x || !shm || dev < 0 || dev >= LEGION_MAX_DEVICE || x->magic != kExt2Magic || x->bytes < offsetof(shmExt2, modes)) return false;
    for (int i = 0; i < 3; i++) if (x->steps_copy[i] != shm->steps[i]) return false;
    return x->handle_sum[dev] == handle_checksum(&shm->memHandle[dev][0][LEGION_BUF_IDS]);
}
bool ext2_edge_handle(const volatile shmExt2* x, int dev, int pipe, int which, hipIpcMemHandle_t* h)
{
    if (!x || x->bytes < sizeof(shmExt2) || dev < 0 || dev >= LEGION_MAX_DEVICE || pipe < 0 || pipe >= LEGION_PIPELINE_DEPTH || which < 0 || which > 1) return false;
    static const hipIpcMemHandle_t zero{};
    memcpy(h, (const void*)&x->edge_handle[dev][pipe][which], sizeof(*h));
    return memcmp(h, &zero, sizeof(*h)) != 0;
}

bool no_device()
{
    static const bool v = [] { const char* e = getenv("LEGION_IPC_NO_DEVICE"); return e && e[0] == '1'; }();
    return v;
}

static std::string g_namespace;
static bool g_ns_init = false;
const std::string& ipc_ns()
{
    if (!g_ns_init) {
        const char* e = getenv("LEGION_IPC_NAMESPACE");
        if (e) g_namespace = e;
        g_ns_init = true;
    }
    return g_namespace;
}
std::string shm_name(const std::string& ns) { return "/" + ns + "simpleIPCshm"; }
std::string ext_name(const std::string& ns) { return shm_name(ns) + "_ext"; }
std::string ext2_name(const std::string& ns) { return shm_name(ns) + "_ext2"; }
std::string sem_name(const char* rw, int dev, int pipe, const std::string& ns)
{
    return "/" + ns + "sem_" + rw + "_" + std::to_string(dev) + "_" + std::to_string(pipe);
}

void* shm_map(size_t sz, int* fd_out, const std::string& name, bool create)
{
    int fd = shm_open(name.c_str(), create ? (O_RDWR | O_CREAT) : O_RDWR, 0777);
    if (fd < 0) return nullptr;
    struct stat st;
    if (fstat(fd, &st) == 0 && (size_t)st.st_size < sz && ftruncate(fd, (off_t)sz) != 0) { close(fd); return nullptr; }
    void* addr = mmap(nullptr, sz, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    if (addr == MAP_FAILED) { close(fd); return nullptr; }
    *fd_out = fd;
    return addr;
}

static sem_t* sem_open_or_refuse(const char* rw, int dev, int pipe, const char* refusal)
{
    sem_t* s = sem_open(sem_name(rw, dev, pipe).c_str(), O_CREAT | O_RDWR, 0666, 0);
    if (s != SEM_FAILED) return s;
    fprintf(log_file(), "errno = %d\n", errno);
    LEGION_ARG_ERROR(refusal);
    return nullptr;
}
bool sem_pair_open(int dev, int pipe, bool fresh, sem_t*& r, sem_t*& w, const char* refuse_r, const char* refuse_w)
{
    if (fresh) sem_pair_unlink(dev, pipe);
    r = sem_open_or_refuse("r", dev, pipe, refuse_r);
    w = r ? sem_open_or_refuse("w", dev, pipe, refuse_w) : nullptr;
    return r && w;
}
bool sem_pair_close(sem_t*& r, sem_t*& w)
{
    const bool ok = !(w && w != SEM_FAILED && sem_close(w) == -1);
    if (r && r != SEM_FAILED) sem_close(r);
    r = w = nullptr;
    return ok;
}
void sem_pair_unlink(int dev, int pipe, const std::string& ns)
{
    for (const char* rw : {"r", "w"}) sem_unlink(sem_name(rw, dev, pipe, ns).c_str());
}

// Waiting for the other side of the hand-off: poll the semaphore for a bounded time before blocking on it.  A blocked waiter is woken
// through the kernel (futex) -- 10-60 us on an idle core -- and that latency sits on the depth-2 handshake of every batch: the server may only
// refill a pipe after the trainer has handed it back.  A waiter polls for 200 us first (profiles/r05_handoff_spin.log: 0 / 50 / 200 / 1000 us
// measured, 200 kept).  A trainer that is the bottleneck costs the server at most that much polling per batch, then it sleeps as before.
int handoff_spin_us() { return 200; }
static inline int64_t mono_ns()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (int64_t)ts.tv_sec * 1000000000ll + ts.tv_nsec;
}
void sem_wait_spin(sem_t* sem)
{
    const int spin = handoff_spin_us();
    if (spin > 0) {
        const int64_t until = mono_ns() + (int64_t)spin * 1000;
        do {
            if (sem_trywait(sem) == 0) return;
            for (int i = 0; i < 32; i++) __builtin_ia32_pause();
        } while (mono_ns() < until);
    }
    while (sem_wait(sem) != 0 && errno == EINTR) {}
}

} // namespace legion

using namespace legion;

extern "C" {

void legion_ipc_set_namespace(const char* ns)
{
    g_namespace = ns ? ns : "";
    g_ns_init = true;
}
// Remove what a server of namespace `ns` that was KILLED left in /dev/shm (IPCEnv_Finalize never ran): the slab, its extension objects and
// the 2 x depth named semaphores of each of `devices` GPUs.  Safe to call when nothing is there.
void legion_ipc_unlink_namespace(const char* ns, int32_t devices)
{
    const std::string p = ns ? ns : "";
    shm_unlink(shm_name(p).c_str());
    shm_unlink(ext_name(p).c_str());
    shm_unlink(ext2_name(p).c_str());
    for (int d = 0; d < devices && d < LEGION_MAX_DEVICE; d++)
        for (int q = 0; q < LEGION_PIPELINE_DEPTH; q++) sem_pair_unlink(d, q, p);
}

} // extern "C"
