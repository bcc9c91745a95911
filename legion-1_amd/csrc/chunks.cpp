// chunks.cpp -- ChunkList (internal.h): the one storage format of the cache shards (cache.cpp) and the CSR fragments (storage.cpp)
#include "internal.h"

#include <cstring>

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

} // namespace legion
