// node_storage.cpp -- host mirror of GPUMemoryNodeStorage (GPU_Memory_Node_Storage.cu:3-207): the feature table, its HBM replicas and the
// seed sets of every mode.
#include "internal.h"

#include "device_mem.h"

using namespace legion;

extern "C" {

GPUNodeStorage* NewGPUMemoryNodeStorage(void) { return new GPUNodeStorage(); }

static int32_t* upload_i32(const int32_t* src, int32_t n)
{
    int32_t* d = nullptr;
    HIP_CHECK(hipMalloc(&d, (size_t)(n > 0 ? n : 1) * sizeof(int32_t)));
    if (n > 0 && src) HIP_CHECK(hipMemcpy(d, src, (size_t)n * sizeof(int32_t), hipMemcpyDefault));
    return d;
}

void GPUNodeStorage_Build(GPUNodeStorage* n, const LegionBuildInfo* info)
{
    if (!n || !info) { LEGION_ARG_ERROR("GPUNodeStorage_Build: null argument"); return; }
    const int P = info->partition_count;
    if (P < 1 || P > kMaxParts) { LEGION_ARG_ERROR("GPUNodeStorage_Build: partition_count must be 1..8"); return; }
    n->partition_count = P;
    n->total_num_nodes = info->total_num_nodes;
    n->float_attr_len = info->float_attr_len;
    // float_attr_pitch is an extension field behind the reference's BuildInfo: 0 = dense.  Anything else must describe a
    // layout the gather can read: at least F floats, and -- when F allows 16-byte chunks -- rows that stay 16-byte aligned
    // (the float4 path is chosen from F and the base pointers).  A caller built against the shorter struct must zero it.
    if (info->float_attr_pitch != 0 && (info->float_attr_pitch < info->float_attr_len ||
                                        (info->float_attr_len % 4 == 0 && info->float_attr_pitch % 4 != 0))) {
        LEGION_ARG_ERROR("GPUNodeStorage_Build: float_attr_pitch must be 0 (dense) or >= float_attr_len, and a multiple of 4 floats when float_attr_len is");
        return;
    }
    n->float_attr_pitch = info->float_attr_pitch > info->float_attr_len ? info->float_attr_pitch : info->float_attr_len;
    n->replica_pitch = 0;
    n->features_location = info->features_location;
    bool owns = false;
    n->float_attrs = info->host_float_attrs
        ? adopt_table<float>(info->host_float_attrs, (int64_t)info->total_num_nodes * n->float_attr_pitch, info->features_location, &owns)
        : nullptr;
    n->owns_features = owns;
    n->replica_attrs.assign(P, nullptr);
    for (auto& sets : n->seeds) sets.assign(P, GPUNodeStorage::SeedSet());
    for (int p = 0; p < P; p++) { // GPU_Memory_Node_Storage.cu:41-96
        if (is_remote_device(p)) continue; // that partition's seed sets live in its own process
        DeviceGuard guard(p);
        for (int mode = 0; mode < kModes; mode++) {
            const BuildInfoSeedFields& f = kBuildInfoSeeds[mode];
            if (!(info->*f.num)) continue;
            GPUNodeStorage::SeedSet& set = n->seeds[mode][p];
            set.num = (info->*f.num)[p];
            set.ids = upload_i32((info->*f.ids)[p], set.num);
            set.labels = upload_i32((info->*f.labels)[p], set.num);
        }
        LEGION_AUDIT_OWNER(n->seeds[LEGION_TRAINMODE][p].ids, p, "GPUNodeStorage_Build: seed list");
    }
}

// the replica gets a line-aligned row pitch (legion_row_pitch); a table that has it already is copied as it lies
int64_t GPUNodeStorage_ReplicateToDevices(GPUNodeStorage* n)
{
    if (!n || !n->float_attrs || n->features_location == LEGION_LOC_DEVICE) return 0;
    const int32_t F = n->float_attr_len, pitch = legion_row_pitch(F);
    const int64_t V = n->total_num_nodes;
    n->replica_pitch = pitch;
    replicate_table<float>(n->float_attrs, V, F, n->float_attr_pitch, pitch, n->replica_attrs);
    return V * pitch * 4;
}

void GPUNodeStorage_Finalize(GPUNodeStorage* n)
{
    if (!n) return;
    free_replicas(n->replica_attrs);
    for (auto& sets : n->seeds)
        for (auto& set : sets) { free_and_null(set.ids); free_and_null(set.labels); }
    if (n->owns_features) { host_free_space(n->float_attrs); n->owns_features = false; }
}
int32_t* GPUNodeStorage_GetTrainingSetIds(const GPUNodeStorage* n, int32_t p) { return n->seed_set(LEGION_TRAINMODE, p).ids; }
int32_t* GPUNodeStorage_GetValidationSetIds(const GPUNodeStorage* n, int32_t p) { return n->seed_set(LEGION_VALIDMODE, p).ids; }
int32_t* GPUNodeStorage_GetTestingSetIds(const GPUNodeStorage* n, int32_t p) { return n->seed_set(LEGION_TESTMODE, p).ids; }
int32_t* GPUNodeStorage_GetTrainingLabels(const GPUNodeStorage* n, int32_t p) { return n->seed_set(LEGION_TRAINMODE, p).labels; }
int32_t* GPUNodeStorage_GetValidationLabels(const GPUNodeStorage* n, int32_t p) { return n->seed_set(LEGION_VALIDMODE, p).labels; }
int32_t* GPUNodeStorage_GetTestingLabels(const GPUNodeStorage* n, int32_t p) { return n->seed_set(LEGION_TESTMODE, p).labels; }
int32_t GPUNodeStorage_TrainingSetSize(const GPUNodeStorage* n, int32_t p) { return n->seed_set(LEGION_TRAINMODE, p).num; }
int32_t GPUNodeStorage_ValidationSetSize(const GPUNodeStorage* n, int32_t p) { return n->seed_set(LEGION_VALIDMODE, p).num; }
int32_t GPUNodeStorage_TestingSetSize(const GPUNodeStorage* n, int32_t p) { return n->seed_set(LEGION_TESTMODE, p).num; }
int32_t GPUNodeStorage_TotalNodeNum(const GPUNodeStorage* n) { return n->total_num_nodes; }
float* GPUNodeStorage_GetAllFloatAttr(const GPUNodeStorage* n) { return n->float_attrs; }
int32_t GPUNodeStorage_GetFloatAttrLen(const GPUNodeStorage* n) { return n->float_attr_len; }
void GPUNodeStorage_Delete(GPUNodeStorage* n)
{
    if (!n) return;
    GPUNodeStorage_Finalize(n);
    delete n;
}

} // extern "C"
