// sort_scan.hip -- the hipcub sort and scans of a cache build (once per build, never per batch).  The only unit that includes hipcub:
// its instantiations take most of the library's compile time and stay out of the units one edits.
#include "internal.h"
#include <hipcub/hipcub.hpp>

#include "audit_hooks.h"

namespace legion {

// thrust::sort_by_key(keys, ids, greater) (GPUCache.cu:631,651).  The reference's sort is not
// stable, so the order among equal keys is unspecified there; we use a stable descending radix
// sort seeded with ascending ids => ties in ascending id order (the oracle's documented rule).
void sort_by_hotness_desc(hipStream_t s, unsigned long long* keys, int32_t* ids, int32_t n)
{
    if (n <= 0) return;
    unsigned long long* keys_out = nullptr;
    int32_t* ids_out = nullptr;
    HIP_CHECK(hipMalloc(&keys_out, (size_t)n * sizeof(unsigned long long)));
    HIP_CHECK(hipMalloc(&ids_out, (size_t)n * sizeof(int32_t)));
    size_t tmp_bytes = 0;
    LEGION_AUDIT_LAUNCH(s, "hipcub::DeviceRadixSort", LEGION_AW(keys), LEGION_AW(ids));
    HIP_CHECK(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp_bytes, keys, keys_out, ids, ids_out, n, 0, 64, s));
    void* tmp = nullptr;
    HIP_CHECK(hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16));
    HIP_CHECK(hipcub::DeviceRadixSort::SortPairsDescending(tmp, tmp_bytes, keys, keys_out, ids, ids_out, n, 0, 64, s));
    HIP_CHECK(hipMemcpyAsync(keys, keys_out, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(ids, ids_out, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipFree(tmp));
    HIP_CHECK(hipFree(keys_out));
    HIP_CHECK(hipFree(ids_out));
}

template <typename T>
static void inclusive_scan_t(hipStream_t s, const T* in, T* out, int32_t n)
{
    if (n <= 0) return;
    size_t tmp_bytes = 0;
    LEGION_AUDIT_LAUNCH(s, "hipcub::DeviceScan", LEGION_AW(out), LEGION_AR(in));
    HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_bytes, in, out, n, s));
    void* tmp = nullptr;
    HIP_CHECK(hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16));
    HIP_CHECK(hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, in, out, n, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipFree(tmp));
}
void inclusive_scan_u64(hipStream_t s, const uint64_t* in, uint64_t* out, int32_t n) { inclusive_scan_t(s, in, out, n); }
void inclusive_scan_i64(hipStream_t s, const int64_t* in, int64_t* out, int32_t n) { inclusive_scan_t(s, in, out, n); }

} // namespace legion
