// ipc_vmm.cpp -- hand-off buffers above the HIP-IPC size limit, the server's side and the trainer's.
// hipIpcOpenMemHandle of the runtime bundled with the torch wheel (ROCm 7.0) never returns for an allocation of 2^31 bytes or
// more (profiles/r02_ipc_limit.md), and a trainer needs its feature rows as ONE contiguous tensor.  Such a buffer is therefore
// built from <= 1 GiB physical chunks (HIP virtual memory management), exported as POSIX file descriptors and handed to the
// trainer over an abstract unix socket (SCM_RIGHTS); the trainer maps the chunks back to back into one reserved virtual range
// (profiles/vmm_ipc_probe.*: 5 GiB mapped in 21 ms under ROCm 7.2, 3 GiB in 0.3 ms inside a PyTorch process).  The 64-byte
// handle slot of the shm table carries a descriptor (VmmDesc, ipc_shm.h) instead of an IPC handle.
#include "ipc_shm.h"

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <poll.h>
#include <sys/socket.h>
#include <sys/un.h>
#include <thread>
#include <unistd.h>

#include "audit_hooks.h"

namespace legion {

static socklen_t vmm_sock_addr(sockaddr_un* a, int dev, int pipe)
{
    memset(a, 0, sizeof(*a));
    a->sun_family = AF_UNIX;
    const std::string name = ipc_ns() + "legion_vmm_" + std::to_string(dev) + "_" + std::to_string(pipe);
    const size_t n = std::min(name.size(), sizeof(a->sun_path) - 2);
    memcpy(a->sun_path + 1, name.data(), n);       // abstract namespace: sun_path[0] == 0, nothing to unlink
    return (socklen_t)(offsetof(sockaddr_un, sun_path) + 1 + n);
}
static bool send_fd(int sock, int fd)
{
    char byte = 'f';
    iovec io{&byte, 1};
    alignas(cmsghdr) char ctrl[CMSG_SPACE(sizeof(int))] = {0};
    msghdr msg{};
    msg.msg_iov = &io; msg.msg_iovlen = 1; msg.msg_control = ctrl; msg.msg_controllen = sizeof(ctrl);
    cmsghdr* c = CMSG_FIRSTHDR(&msg);
    c->cmsg_level = SOL_SOCKET; c->cmsg_type = SCM_RIGHTS; c->cmsg_len = CMSG_LEN(sizeof(int));
    memcpy(CMSG_DATA(c), &fd, sizeof(int));
    return sendmsg(sock, &msg, MSG_NOSIGNAL) == 1;
}
static int recv_fd(int sock)
{
    char byte;
    iovec io{&byte, 1};
    alignas(cmsghdr) char ctrl[CMSG_SPACE(sizeof(int))] = {0};
    msghdr msg{};
    msg.msg_iov = &io; msg.msg_iovlen = 1; msg.msg_control = ctrl; msg.msg_controllen = sizeof(ctrl);
    if (recvmsg(sock, &msg, 0) != 1) return -1;
    cmsghdr* c = CMSG_FIRSTHDR(&msg);
    int fd = -1;
    if (c && c->cmsg_level == SOL_SOCKET && c->cmsg_type == SCM_RIGHTS) memcpy(&fd, CMSG_DATA(c), sizeof(int));
    return fd;
}

// Chunk by chunk, as they were mapped.  The unmap of a chunk that was imported or created but not mapped (a build that failed half-way)
// fails harmlessly.
void vmm_unmap(VmmMapping& m)
{
    if (m.va) {
        size_t off = 0;
        for (size_t k = 0; k < m.handles.size(); k++) {
            const size_t sz = std::min(m.chunk, m.total - off);
            (void)hipMemUnmap((char*)m.va + off, sz);
            off += sz;
        }
        for (auto h : m.handles) (void)hipMemRelease(h);
        (void)hipMemAddressFree(m.va, m.total);
        (void)hipGetLastError();
    }
    m = VmmMapping();
}

struct VmmRegion {
    VmmMapping map;
    VmmDesc desc{};
    std::vector<int> fds;
    int listen_fd = -1, device = 0;
    std::thread server;
    std::atomic<bool> stop{false};
};
const VmmDesc& vmm_desc(const VmmRegion* r) { return r->desc; }
void* vmm_va(const VmmRegion* r) { return r->map.va; }

static void vmm_serve(VmmRegion* r)
{
    while (!r->stop.load()) {
        pollfd p{r->listen_fd, POLLIN, 0};
        if (poll(&p, 1, 200) <= 0) continue;
        const int s = accept4(r->listen_fd, nullptr, nullptr, SOCK_CLOEXEC);
        if (s < 0) continue;
        // the descriptors are read/write dmabuf handles of the feature buffer: only hand them to a process of this user,
        // and never let a stalled client hold the serving thread (IPCEnv_Finalize joins it)
        timeval tv{2, 0};
        (void)setsockopt(s, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv));
        (void)setsockopt(s, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof(tv));
        ucred cred{};
        socklen_t cl = sizeof(cred);
        bool ok = getsockopt(s, SOL_SOCKET, SO_PEERCRED, &cred, &cl) == 0 && cred.uid == geteuid();
        ok = ok && send(s, &r->desc, sizeof(r->desc), MSG_NOSIGNAL) == (ssize_t)sizeof(r->desc);
        for (size_t i = 0; ok && i < r->fds.size(); i++) ok = send_fd(s, r->fds[i]);
        // the trainer acknowledges after it has mapped everything; wait for it in slices so that a shutdown is never blocked
        for (int waited = 0; ok && waited < 30 && !r->stop.load(); waited++) {
            char ack;
            const ssize_t n = recv(s, &ack, 1, 0);
            if (n >= 0 || (errno != EAGAIN && errno != EWOULDBLOCK && errno != EINTR)) break;
        }
        close(s);
    }
}
void vmm_release(VmmRegion* r)
{
    DeviceGuard guard(r->device);
    r->stop.store(true);
    if (r->server.joinable()) r->server.join();
    if (r->listen_fd >= 0) close(r->listen_fd);
    for (int fd : r->fds) close(fd);
    if (r->map.va && audit::on()) audit::region_gone(r->map.va);
    vmm_unmap(r->map);
    delete r;
}
VmmRegion* vmm_create(int logical_dev, int pipe, size_t bytes)
{
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = physical_device(logical_dev);
    prop.requestedHandleType = hipMemHandleTypePosixFileDescriptor;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || !gran) {
        (void)hipGetLastError();
        LEGION_ARG_ERROR("hand-off buffer above the HIP-IPC limit: this runtime has no virtual memory management");
        return nullptr;
    }
    // the chunk size of the cache shards too (open: nothing bounds the number of chunks, one exported descriptor each)
    const size_t chunk = std::max(gran, (size_t)shard_chunk_bytes() / gran * gran);
    VmmRegion* r = new VmmRegion();
    r->device = logical_dev;
    const size_t total = (bytes + gran - 1) / gran * gran;
    memcpy(r->desc.magic, kVmmMagic, 8);
    r->desc.total = total; r->desc.chunk = chunk; r->desc.nchunks = (uint32_t)((total + chunk - 1) / chunk);
    bool ok = hipMemAddressReserve(&r->map.va, total, 0, nullptr, 0) == hipSuccess;
    if (ok) { r->map.total = total; r->map.chunk = chunk; }
    for (uint32_t c = 0; ok && c < r->desc.nchunks; c++) {
        const size_t sz = std::min(chunk, total - (size_t)c * chunk);
        hipMemGenericAllocationHandle_t h;
        ok = hipMemCreate(&h, sz, &prop, 0) == hipSuccess;
        if (!ok) break;
        r->map.handles.push_back(h);
        ok = hipMemMap((char*)r->map.va + (size_t)c * chunk, sz, 0, h, 0) == hipSuccess;
        int fd = -1;
        ok = ok && hipMemExportToShareableHandle(&fd, h, hipMemHandleTypePosixFileDescriptor, 0) == hipSuccess;
        if (ok) r->fds.push_back(fd);
    }
    hipMemAccessDesc acc{};
    acc.location = prop.location; acc.flags = hipMemAccessFlagsProtReadWrite;
    ok = ok && hipMemSetAccess(r->map.va, total, &acc, 1) == hipSuccess;
    if (ok) {
        sockaddr_un addr;
        const socklen_t len = vmm_sock_addr(&addr, logical_dev, pipe);
        r->listen_fd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
        ok = r->listen_fd >= 0 && bind(r->listen_fd, (sockaddr*)&addr, len) == 0 && listen(r->listen_fd, 8) == 0;
    }
    if (!ok) {
        (void)hipGetLastError();
        LEGION_ARG_ERROR("hand-off buffer above the HIP-IPC limit: building the chunked (virtual memory) buffer failed");
        vmm_release(r);
        return nullptr;
    }
    if (audit::on()) audit::region(r->map.va, total, logical_dev, __FILE__, __LINE__);
    r->server = std::thread(vmm_serve, r);
    return r;
}

// osHandle: the ROCm 7.0 runtime (the one bundled with the torch wheel, hipRuntimeGetVersion 70051831) dereferences it as
// int*, ROCm 7.2 (70226015) takes the descriptor by value (like CUDA).  The convention is picked ONCE from the version of the
// runtime this process really loaded -- no trial call: a genuine failure of the first form (stale fd, out of memory) must come
// back as an error, not be retried in the form that makes the other runtime dereference a small integer.
static hipError_t vmm_import_fd(hipMemGenericAllocationHandle_t* h, int fd)
{
    static int by_pointer = -1;
    if (by_pointer < 0) {
        int v = 0;
        if (hipRuntimeGetVersion(&v) != hipSuccess) { (void)hipGetLastError(); v = 0; }
        by_pointer = v < 70100000;
    }
    static thread_local int fd_cell;
    fd_cell = fd;
    return hipMemImportFromShareableHandle(h, by_pointer ? (void*)&fd_cell : (void*)(uintptr_t)fd, hipMemHandleTypePosixFileDescriptor);
}

void* vmm_attach(int dev, int pipe, const VmmDesc& want, VmmMapping& m)
{
    sockaddr_un addr;
    const socklen_t len = vmm_sock_addr(&addr, dev, pipe);
    const int s = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    bool ok = s >= 0;
    const char* te = getenv("LEGION_VMM_ATTACH_TIMEOUT_MS");
    const int tries = std::max(1, (te && atoi(te) > 0 ? atoi(te) : 10000) / 100);
    for (int i = 0; ok && connect(s, (sockaddr*)&addr, len) != 0; i++) {
        if (i >= tries - 1) { ok = false; break; }
        usleep(100000);
    }
    if (ok) { timeval tv{10, 0}; (void)setsockopt(s, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv)); }
    VmmDesc d{};
    ok = ok && recv(s, &d, sizeof(d), MSG_WAITALL) == (ssize_t)sizeof(d) && memcmp(&d, &want, sizeof(d)) == 0;
    int cur = 0;
    (void)hipGetDevice(&cur);
    ok = ok && hipMemAddressReserve(&m.va, d.total, 0, nullptr, 0) == hipSuccess;
    if (ok) { m.total = d.total; m.chunk = d.chunk; }
    for (uint32_t k = 0; ok && k < d.nchunks; k++) {
        const int fd = recv_fd(s);
        hipMemGenericAllocationHandle_t h;
        ok = fd >= 0 && vmm_import_fd(&h, fd) == hipSuccess;
        if (fd >= 0) close(fd);
        if (!ok) break;
        m.handles.push_back(h);
        const size_t sz = std::min<size_t>(d.chunk, d.total - (size_t)k * d.chunk);
        ok = hipMemMap((char*)m.va + (size_t)k * d.chunk, sz, 0, h, 0) == hipSuccess;
    }
    hipMemAccessDesc acc{};
    acc.location.type = hipMemLocationTypeDevice; acc.location.id = cur; acc.flags = hipMemAccessFlagsProtReadWrite;
    ok = ok && hipMemSetAccess(m.va, d.total, &acc, 1) == hipSuccess;
    if (s >= 0) { if (ok) (void)!send(s, "d", 1, MSG_NOSIGNAL); close(s); }
    if (!ok) {
        (void)hipGetLastError();
        vmm_unmap(m);           // give back whatever was reserved / imported / mapped so far: the caller refuses the whole client
        legion_clear_error();   // this is why the client is refused: let it be the error the caller reads
        LEGION_ARG_ERROR("legion_ipc_client_open: attaching the chunked feature buffer failed");
        return nullptr;
    }
    return m.va;
}

} // namespace legion
