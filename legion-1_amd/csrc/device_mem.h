// device_mem.h -- the frees of device memory that the storages, the pool and the cache share.  Include it LAST: it pulls in audit_hooks.h, so
// that every free below goes through the logical-device audit like the allocation it ends.
#pragma once
#include "internal.h"

#include "audit_hooks.h"

namespace legion {

// free (when there is something) and forget
template <typename T>
inline void free_and_null(T*& p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}

// A device temporary that frees itself on every way out of its scope.  Allocate into .p (HIP_CHECK(hipMalloc(&t.p, ..)) at the call site, so
// that a failure names that line); release() hands the allocation to the caller, reset() frees it early.
template <typename T>
struct DeviceTemp {
    T* p = nullptr;
    DeviceTemp() = default;
    DeviceTemp(const DeviceTemp&) = delete;
    DeviceTemp& operator=(const DeviceTemp&) = delete;
    ~DeviceTemp() { reset(); }
    void reset() { free_and_null(p); }
    T* release() { T* q = p; p = nullptr; return q; }
};

// The one free of an array filled under the per-physical-device rule (device_leaders, internal.h): the logical GPUs of a physical device
// hold the SAME pointer, so a copy is freed once, by pointer identity, and every holder forgets it.
template <typename T>
inline void free_replicas(std::vector<T*>& replica)
{
    for (size_t i = 0; i < replica.size(); i++) {
        if (!replica[i]) continue;
        T* p = replica[i];
        for (size_t j = i; j < replica.size(); j++) if (replica[j] == p) replica[j] = nullptr;
        (void)hipFree(p);
    }
}

} // namespace legion
