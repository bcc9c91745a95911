// chunks.cpp -- ChunkList (internal.h): the one storage format of the cache shards (cache.cpp) and the CSR fragments (graph_storage.cpp);
// and what graph_storage.cpp, node_storage.cpp and server.cpp share: peer access, adopted tables, the per-physical-device copies
#include "internal.h"

#include <cstring>
#include <set>

#include "audit_hooks.h"

namespace legion {

int chunk_shift(int64_t unit_bytes, int min_shift)
{
    const int64_t bytes = shard_chunk_bytes();
    int s = min_shift;
    while (s < 30 && (2ll << s) * unit_bytes <= bytes) s++;
    return s;
}

template <typename T>
void ChunkList<T>::release()
{
    for (T* p : chunks)
        if (p) (void)(imported ? hipIpcCloseMemHandle(p) : hipFree(p));
    chunks.clear();
    imported = false;
}
template <typename T>
int ChunkList<T>::export_chunk(int dev, int q, void* handle64, const char* who) const
{
    T* p = at(q);
    if (!p || !handle64 || imported) { LEGION_ARG_ERROR((std::string(who) + ": no such local chunk").c_str()); return -1; }
    DeviceGuard guard(dev);
    if (!ipc_export_ok(p, who)) return -1;
    HIP_CHECK(hipIpcGetMemHandle((hipIpcMemHandle_t*)handle64, p));
    return error_pending() ? -1 : 0;
}
template <typename T>
int ChunkList<T>::import_chunk(int q, const void* handle64, int64_t floor_bytes, int open_dev, const char* who)
{
    if (!ipc_size_ok(floor_bytes, who)) return -1;
    hipIpcMemHandle_t h;
    memcpy(&h, handle64, sizeof(h));
    void* p = nullptr;
    DeviceGuard guard(open_dev);
    HIP_CHECK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
    if (!p) return -1;
    if ((int)chunks.size() <= q) chunks.resize(q + 1, nullptr);
    chunks[q] = (T*)p;
    imported = true;
    return 0;
}
template struct ChunkList<float>;
template struct ChunkList<int64_t>;
template struct ChunkList<int32_t>;

template <typename T>
void upload_table(int viewer, const std::vector<T*>& h, T**& tab, bool realloc, const char* what)
{
    DeviceGuard guard(viewer);
    LEGION_AUDIT_TABLE(viewer, h.data(), h.size(), what);
    if (tab && (realloc || h.empty())) { HIP_CHECK(hipDeviceSynchronize()); (void)hipFree(tab); tab = nullptr; }
    if (h.empty()) return;
    if (!tab) HIP_CHECK(hipMalloc(&tab, h.size() * sizeof(T*)));
    HIP_CHECK(hipMemcpy(tab, h.data(), h.size() * sizeof(T*), hipMemcpyHostToDevice));
}
template void upload_table<float>(int, const std::vector<float*>&, float**&, bool, const char*);
template void upload_table<void>(int, const std::vector<void*>&, void**&, bool, const char*);

void enable_p2p(int32_t partition_count)
{
    std::set<int> phys;
    for (int i = 0; i < partition_count; i++) phys.insert(physical_device(i));
    // the audit's view: on a node every logical GPU is a device of its own and this loop enables every pair
    if (audit::on()) for (int a = 0; a < partition_count; a++) for (int b = 0; b < partition_count; b++) if (a != b) audit::record_peer(a, b);
    if (phys.size() < 2) return;
    int cur = 0;
    HIP_CHECK(hipGetDevice(&cur));
    for (int a : phys) {
        HIP_CHECK(hipSetDevice(a));
        for (int b : phys) {
            if (a == b) continue;
            int ok = 0;
            HIP_CHECK(hipDeviceCanAccessPeer(&ok, a, b));
            if (ok) {
                hipError_t e = hipDeviceEnablePeerAccess(b, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_CHECK(e);
                (void)hipGetLastError();
            }
        }
    }
    HIP_CHECK(hipSetDevice(cur));
}

template <typename T>
T* adopt_table(const T* src, int64_t count, int32_t location, bool* owns)
{
    *owns = false;
    if (location == LEGION_LOC_HOST_PAGEABLE) {
        T* p = (T*)host_alloc_space64(count * (int64_t)sizeof(T));
        if (p) memcpy(p, src, (size_t)count * sizeof(T));
        *owns = true;
        return p;
    }
    return const_cast<T*>(src);
}
template int64_t* adopt_table<int64_t>(const int64_t*, int64_t, int32_t, bool*);
template int32_t* adopt_table<int32_t>(const int32_t*, int64_t, int32_t, bool*);
template float* adopt_table<float>(const float*, int64_t, int32_t, bool*);

std::vector<int> device_leaders(int P)
{
    std::vector<int> leader(P, -1);
    for (int p = 0; p < P; p++) {
        if (is_remote_device(p)) continue;
        leader[p] = p;
        for (int q = 0; q < p; q++)
            if (leader[q] == q && physical_device(q) == physical_device(p)) { leader[p] = q; break; }
    }
    return leader;
}

template <typename T>
void replicate_table(const T* src, int64_t rows, int64_t width, int64_t src_pitch, int64_t dst_pitch, std::vector<T*>& replica)
{
    const std::vector<int> leader = device_leaders((int)replica.size());
    for (int p = 0; p < (int)replica.size(); p++) {
        if (leader[p] < 0 || replica[p]) continue;
        if (leader[p] != p) replica[p] = replica[leader[p]];
        else {
            DeviceGuard guard(p);
            T* copy = nullptr;
            const size_t bytes = (size_t)rows * dst_pitch * sizeof(T);
            HIP_CHECK(hipMalloc(&copy, bytes));
            if (copy && src_pitch == dst_pitch) HIP_CHECK(hipMemcpy(copy, src, bytes, hipMemcpyDefault));
            else if (copy) {
                HIP_CHECK(hipMemset(copy, 0, bytes));
                HIP_CHECK(hipMemcpy2D(copy, (size_t)dst_pitch * sizeof(T), src, (size_t)src_pitch * sizeof(T), (size_t)width * sizeof(T), (size_t)rows, hipMemcpyDefault));
            }
            replica[p] = copy;
        }
        LEGION_AUDIT_SHARE(replica[p], p);     // logical GPUs of one physical device share its replica
    }
}
template void replicate_table<int64_t>(const int64_t*, int64_t, int64_t, int64_t, int64_t, std::vector<int64_t*>&);
template void replicate_table<int32_t>(const int32_t*, int64_t, int64_t, int64_t, int64_t, std::vector<int32_t*>&);
template void replicate_table<float>(const float*, int64_t, int64_t, int64_t, int64_t, std::vector<float*>&);

} // namespace legion
