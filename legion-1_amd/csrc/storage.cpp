// storage.cpp -- host mirrors of GPUMemoryGraphStorage (GPU_Memory_Graph_Storage.cu:37-210),
// GPUMemoryNodeStorage (GPU_Memory_Node_Storage.cu:3-207) and GPUMemoryPool (GPUMemoryPool.cuh:7-208).
#include "internal.h"

#include <algorithm>
#include <cstring>
#include <set>

#include "audit_hooks.h"

using namespace legion;

// all-pairs peer access between the physical devices behind the logical GPUs
// (GPUGraphStore::EnableP2PAccess, GPUGraphStore.cu:145-168)
static void enable_p2p(int32_t partition_count)
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
static T* adopt_table(const T* src, int64_t count, int32_t location, bool* owns)
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

// one HBM replica per distinct physical device among the local logical GPUs
template <typename T>
static void replicate_table(const T* src, int64_t count, int32_t P, std::vector<T*>& replica)
{
    std::vector<std::pair<int, T*>> per_phys;
    for (int p = 0; p < P; p++) {
        if (is_remote_device(p) || replica[p]) continue;
        const int phys = physical_device(p);
        T* have = nullptr;
        for (auto& e : per_phys) if (e.first == phys) have = e.second;
        if (!have) {
            DeviceGuard guard(p);
            HIP_CHECK(hipMalloc(&have, (size_t)count * sizeof(T)));
            if (have) HIP_CHECK(hipMemcpy(have, src, (size_t)count * sizeof(T), hipMemcpyDefault));
            per_phys.emplace_back(phys, have);
        }
        LEGION_AUDIT_SHARE(have, p);     // logical GPUs of one physical device share its replica
        replica[p] = have;
    }
}
template <typename T>
static void free_replicas(std::vector<T*>& replica)
{
    for (size_t i = 0; i < replica.size(); i++) {
        if (!replica[i]) continue;
        T* p = replica[i];
        for (size_t j = i; j < replica.size(); j++) if (replica[j] == p) replica[j] = nullptr;
        (void)hipFree(p);
    }
}

extern "C" {

// ================================= graph storage ====================================================
GPUGraphStorage* NewGPUMemoryGraphStorage(void) { return new GPUGraphStorage(); }

void GPUGraphStorage_Build(GPUGraphStorage* g, const LegionBuildInfo* info)
{
    if (!g || !info) { LEGION_ARG_ERROR("GPUGraphStorage_Build: null argument"); return; }
    if (info->partition_count < 1 || info->partition_count > kMaxParts) { LEGION_ARG_ERROR("GPUGraphStorage_Build: partition_count must be 1..8"); return; }
    const int P = info->partition_count;
    g->partition_count = P;
    g->node_num = info->total_num_nodes;
    g->edge_num = info->total_edge_num;
    g->cache_edge_num = info->cache_edge_num;
    g->csr_location = info->csr_location;
    enable_p2p(P);
    bool o1 = false, o2 = false;
    g->csr_node_index_cpu = adopt_table<int64_t>(info->csr_node_index, (int64_t)info->total_num_nodes + 1, info->csr_location, &o1);
    g->csr_dst_node_ids_cpu = adopt_table<int32_t>(info->csr_dst_node_ids, info->total_edge_num, info->csr_location, &o2);
    g->owns_csr = o1 || o2;
    if (o1) g->csr_location = LEGION_LOC_HOST_PINNED;
    g->frag.assign(P, GPUGraphStorage::Fragment());
    g->replica_indptr.assign(P, nullptr);
    g->replica_indices.assign(P, nullptr);
    g->view.assign(P, std::vector<bool>(P, false));
    g->d_frag_tab.assign(P, nullptr);
    g->alias.assign(P, nullptr);
    g->weights.assign(P, nullptr);
    // chunk geometry of the fragments: powers of two that fit shard_chunk_bytes()
    g->row_shift = chunk_shift(sizeof(int64_t), 4);
    g->edge_shift = chunk_shift(sizeof(int32_t), 4);
}

static void free_fragment(GPUGraphStorage::Fragment& f)
{
    f.ip.release();
    f.ix.release();
    f = GPUGraphStorage::Fragment();
}

// (re)write the device-side chunk-pointer tables of every local viewer
static void publish_fragment_tables(GPUGraphStorage* g)
{
    const int P = g->partition_count;
    int ip_nch = 1, ix_nch = 1;
    for (const auto& f : g->frag) { ip_nch = std::max(ip_nch, (int)f.ip.chunks.size()); ix_nch = std::max(ix_nch, (int)f.ix.chunks.size()); }
    const bool regrow = ip_nch != g->ip_nch || ix_nch != g->ix_nch;
    g->ip_nch = ip_nch; g->ix_nch = ix_nch;
    for (int dev = 0; dev < P; dev++) {
        if (is_remote_device(dev)) continue;
        bool any = false;
        std::vector<void*> h((size_t)P * (ip_nch + ix_nch) + 1, nullptr); // +1: a zero-degree row at offset == edges names chunk ix_nch
        for (int p = 0; p < P; p++) {
            if (!g->view[dev][p]) continue;
            for (size_t q = 0; q < g->frag[p].ip.chunks.size(); q++) { h[(size_t)p * ip_nch + q] = g->frag[p].ip.chunks[q]; any = true; }
            for (size_t q = 0; q < g->frag[p].ix.chunks.size(); q++) h[(size_t)P * ip_nch + (size_t)p * ix_nch + q] = g->frag[p].ix.chunks[q];
        }
        if (!any) h.clear();   // the viewer sees no fragment: its table is freed
        upload_table(dev, h, g->d_frag_tab[dev], regrow, "fragment chunk table");
    }
}

// GraphCache (GPU_Memory_Graph_Storage.cu:98-133): fragment of clique GPU i holds rows QT[r*Kg+i]
void GPUGraphStorage_GraphCache(GPUGraphStorage* g, int32_t* QT, int32_t Ki, int32_t Kg, int32_t capacity)
{
    if (!g || !QT || Kg < 1 || (Ki + 1) * Kg > g->partition_count) { LEGION_ARG_ERROR("GraphCache: bad clique"); return; }
    for (int i = 0; i < Kg; i++) {
        const int dev = Ki * Kg + i;
        if (is_remote_device(dev)) continue; // built by its own process, imported here over IPC
        DeviceGuard guard(dev);
        HIP_CHECK(hipDeviceSynchronize());
        free_fragment(g->frag[dev]);
        if (capacity <= 0) continue;
        GPUGraphStorage::Fragment& f = g->frag[dev];
        int64_t* neighbor_count = nullptr;
        int64_t* d_index = nullptr; // contiguous build copy of the fragment's indptr
        HIP_CHECK(hipMalloc(&neighbor_count, (size_t)capacity * sizeof(int64_t)));
        HIP_CHECK(hipMalloc(&d_index, ((size_t)capacity + 1) * sizeof(int64_t)));
        HIP_CHECK(hipMemset(d_index, 0, sizeof(int64_t)));
        launch_neighbor_count(nullptr, QT, Kg, i, capacity, g->node_num, g->csr_node_index_cpu, neighbor_count);
        inclusive_scan_i64(nullptr, neighbor_count, d_index + 1, capacity);
        int64_t total = 0;
        HIP_CHECK(hipMemcpy(&total, d_index + capacity, sizeof(int64_t), hipMemcpyDeviceToHost));
        HIP_CHECK(hipFree(neighbor_count));
        f.rows = capacity;
        f.edges = total;
        // indices chunks: chunk q ends where the last row that starts before its upper boundary ends
        const int nx = chunk_count(total, g->edge_shift);
        std::vector<int64_t> ends(nx, total);
        if (nx > 1) {
            int64_t* d_ends = nullptr;
            HIP_CHECK(hipMalloc(&d_ends, (size_t)nx * sizeof(int64_t)));
            launch_chunk_ends(nullptr, d_index, capacity, g->edge_shift, nx, d_ends);
            HIP_CHECK(hipMemcpy(ends.data(), d_ends, (size_t)(nx - 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
            HIP_CHECK(hipFree(d_ends));
        }
        f.ix.chunks.assign(nx, nullptr);
        for (int q = 0; q < nx; q++) {
            const int64_t elems = ends[q] - ((int64_t)q << g->edge_shift); // <= 0: no row starts in this chunk
            HIP_CHECK(hipMalloc(&f.ix.chunks[q], (size_t)(elems > 0 ? elems : 1) * sizeof(int32_t)));
        }
        int32_t** d_chunks = nullptr;
        HIP_CHECK(hipMalloc(&d_chunks, ((size_t)nx + 1) * sizeof(int32_t*))); // +1: see publish_fragment_tables
        HIP_CHECK(hipMemcpy(d_chunks, f.ix.chunks.data(), (size_t)nx * sizeof(int32_t*), hipMemcpyHostToDevice));
        launch_topo_fill_up(nullptr, QT, Kg, i, capacity, g->node_num, g->csr_node_index_cpu, g->csr_dst_node_ids_cpu, d_index, d_chunks, g->edge_shift);
        // indptr chunks (one entry of overlap); a single chunk adopts the build copy
        const int np = chunk_count(capacity, g->row_shift);
        if (np == 1) {
            f.ip.chunks.assign(1, d_index);
            d_index = nullptr;
        } else {
            f.ip.chunks.assign(np, nullptr);
            const int64_t rpc = 1ll << g->row_shift;
            for (int q = 0; q < np; q++) {
                const int64_t r0 = q * rpc, n = std::min<int64_t>(rpc, capacity - r0) + 1;
                HIP_CHECK(hipMalloc(&f.ip.chunks[q], (size_t)n * sizeof(int64_t)));
                HIP_CHECK(hipMemcpy(f.ip.chunks[q], d_index + r0, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice));
            }
        }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipFree(d_chunks));
        if (d_index) HIP_CHECK(hipFree(d_index));
        for (auto* q : f.ip.chunks) LEGION_AUDIT_OWNER(q, dev, "GraphCache: indptr chunk of a fragment");
        for (auto* q : f.ix.chunks) LEGION_AUDIT_OWNER(q, dev, "GraphCache: indices chunk of a fragment");
        f.complete = true;
    }
    // every clique member sees every clique fragment (pointer tables copied D2D in the reference, :128-131)
    for (int i = 0; i < Kg; i++)
        for (int j = 0; j < Kg; j++) g->view[Ki * Kg + i][Ki * Kg + j] = true;
    publish_fragment_tables(g);
}

int64_t GPUGraphStorage_ReplicateToDevices(GPUGraphStorage* g)
{
    if (!g || !g->csr_node_index_cpu || g->csr_location == LEGION_LOC_DEVICE) return 0; // already HBM resident
    replicate_table<int64_t>(g->csr_node_index_cpu, (int64_t)g->node_num + 1, g->partition_count, g->replica_indptr);
    replicate_table<int32_t>(g->csr_dst_node_ids_cpu, g->edge_num, g->partition_count, g->replica_indices);
    return ((int64_t)g->node_num + 1) * 8 + g->edge_num * 4;
}

// ---- weighted sampler mode: the graph's edge weights as an alias table (INTEGRATION.md "Weighted sampling") ----
// The table of the whole CSR on the current device (logical GPU dev), from the weights wherever they lie; null with a sticky error.
// *bad := the number of refused weights (then nothing is built).  The fp64 scratch is freed before returning, and so is the weights' device
// copy -- unless `kept` is given and the table was built: then *kept := the copy (weighted sampling without replacement reads it).
static AliasEntry* build_alias_here(const GPUGraphStorage* g, int dev, const float* w, unsigned long long* bad, float** kept)
{
    const int64_t E = g->edge_num;
    float* d_w = nullptr;
    unsigned long long* d_bad = nullptr;
    double* d_p = nullptr;
    AliasEntry* table = nullptr;
    HIP_CHECK(hipMalloc(&d_w, (size_t)E * sizeof(float)));
    HIP_CHECK(hipMalloc(&d_bad, sizeof(unsigned long long)));
    if (d_w && d_bad) {
        HIP_CHECK(hipMemcpy(d_w, w, (size_t)E * sizeof(float), hipMemcpyDefault));
        HIP_CHECK(hipMemset(d_bad, 0, sizeof(unsigned long long)));
        launch_check_weights(nullptr, d_w, E, d_bad);
        *bad = ~0ull;
        HIP_CHECK(hipMemcpy(bad, d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (*bad == 0 && !error_pending()) {
            HIP_CHECK(hipMalloc(&d_p, (size_t)E * sizeof(double)));
            HIP_CHECK(hipMalloc(&table, (size_t)E * sizeof(AliasEntry)));
            if (d_p && table) {
                HIP_CHECK(hipMemset(table, 0, (size_t)E * sizeof(AliasEntry)));   // entries past a truncated degree are never drawn; keep them defined
                launch_build_alias(nullptr, g->replica_indptr[dev] ? g->replica_indptr[dev] : g->csr_node_index_cpu,
                                   g->replica_indices[dev] ? g->replica_indices[dev] : g->csr_dst_node_ids_cpu, d_w, g->node_num, E, d_p, table);
                HIP_CHECK(hipDeviceSynchronize());
            }
            if (error_pending() && table) { (void)hipFree(table); table = nullptr; }
        }
    }
    if (d_p) (void)hipFree(d_p);
    if (d_bad) (void)hipFree(d_bad);
    if (kept && table) { *kept = d_w; d_w = nullptr; }
    if (d_w) (void)hipFree(d_w);
    return table;
}

int GPUGraphStorage_SetEdgeWeights(GPUGraphStorage* g, const float* w, int32_t location)
{
    if (!g || g->alias.empty()) { LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeWeights: null graph, or GPUGraphStorage_Build was not called"); return -1; }
    if (w && location != LEGION_LOC_HOST_PINNED && location != LEGION_LOC_DEVICE && location != LEGION_LOC_HOST_PAGEABLE) { LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeWeights: location must be a LEGION_LOC_* value"); return -1; }
    const int P = g->partition_count;
    std::vector<AliasEntry*> fresh(P, nullptr);
    std::vector<float*> fresh_w(P, nullptr);
    if (w && g->edge_num > 0) {
        std::vector<std::pair<int, AliasEntry*>> per_phys;
        std::vector<float*> per_phys_w;
        for (int p = 0; p < P; p++) {
            if (is_remote_device(p)) continue;
            const int phys = physical_device(p);
            AliasEntry* have = nullptr;
            float* have_w = nullptr;
            for (size_t q = 0; q < per_phys.size(); q++) if (per_phys[q].first == phys) { have = per_phys[q].second; have_w = per_phys_w[q]; }
            if (!have) {
                DeviceGuard guard(p);
                unsigned long long bad = 0;
                have = build_alias_here(g, p, w, &bad, g->retain_weights ? &have_w : nullptr);
                if (!have) {   // refused or failed: the earlier table stays
                    if (bad && !error_pending())
                        LEGION_ARG_ERROR(("GPUGraphStorage_SetEdgeWeights: " + std::to_string(bad) + " of " + std::to_string(g->edge_num) +
                                          " edge weights are negative, NaN or infinite: weights must be finite and >= 0 (the earlier table, if any, stays)").c_str());
                    else if (!error_pending()) LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeWeights: building the alias table failed");
                    free_replicas(fresh);
                    free_replicas(fresh_w);
                    return -1;
                }
                per_phys.emplace_back(phys, have);
                per_phys_w.push_back(have_w);
            }
            LEGION_AUDIT_SHARE(have, p);
            fresh[p] = have;
            if (have_w) { LEGION_AUDIT_SHARE(have_w, p); fresh_w[p] = have_w; }
        }
    }
    // batches that read the earlier table may still be in flight
    for (int p = 0; p < P; p++)
        if (g->alias[p] && !is_remote_device(p)) { DeviceGuard guard(p); HIP_CHECK(hipDeviceSynchronize()); }
    free_replicas(g->alias);
    free_replicas(g->weights);
    g->alias = fresh;
    g->weights = fresh_w;
    return error_pending() ? -1 : 0;
}
// Before GPUGraphStorage_SetEdgeWeights: that call keeps (on != 0) the weights' float32[E] device copy on every physical device, next to
// the alias table, for weighted sampling without replacement.  It changes nothing that is already built; dropping the table drops the copy.
int GPUGraphStorage_RetainEdgeWeights(GPUGraphStorage* g, int on)
{
    if (!g || g->alias.empty()) { LEGION_ARG_ERROR("GPUGraphStorage_RetainEdgeWeights: null graph, or GPUGraphStorage_Build was not called"); return -1; }
    g->retain_weights = on != 0;
    return 0;
}
int GPUGraphStorage_HasRetainedEdgeWeights(const GPUGraphStorage* g)
{
    if (!g) return 0;
    for (const float* t : g->weights) if (t) return 1;
    return 0;
}
int GPUGraphStorage_HasEdgeWeights(const GPUGraphStorage* g)
{
    if (!g) return 0;
    for (const AliasEntry* t : g->alias) if (t) return 1;
    return 0;
}
int GPUGraphStorage_CopyAliasRows(const GPUGraphStorage* g, int32_t dev_id, int64_t e0, int64_t n, uint32_t* thr, int32_t* alias_id)
{
    if (!g || dev_id < 0 || dev_id >= (int32_t)g->alias.size() || !g->alias[dev_id]) { LEGION_ARG_ERROR("GPUGraphStorage_CopyAliasRows: this logical GPU holds no alias table (GPUGraphStorage_SetEdgeWeights)"); return -1; }
    if (e0 < 0 || n < 0 || e0 > g->edge_num - n) { LEGION_ARG_ERROR("GPUGraphStorage_CopyAliasRows: entries outside [0, edge count)"); return -1; }
    if (n == 0) return 0;
    if (!thr || !alias_id) { LEGION_ARG_ERROR("GPUGraphStorage_CopyAliasRows: null output"); return -1; }
    std::vector<AliasEntry> h((size_t)n);
    {
        DeviceGuard guard(dev_id);
        HIP_CHECK(hipMemcpy(h.data(), g->alias[dev_id] + e0, (size_t)n * sizeof(AliasEntry), hipMemcpyDeviceToHost));
    }
    if (error_pending()) return -1;
    for (int64_t i = 0; i < n; i++) { thr[i] = h[(size_t)i].thr; alias_id[i] = h[(size_t)i].alias_id; }
    return 0;
}

void GPUGraphStorage_Finalize(GPUGraphStorage* g)
{
    if (!g) return;
    free_replicas(g->alias);
    free_replicas(g->weights);
    free_replicas(g->replica_indptr);
    free_replicas(g->replica_indices);
    for (size_t i = 0; i < g->frag.size(); i++) {
        if (!is_remote_device((int)i) || g->frag[i].ip.imported) { DeviceGuard guard((int)i); free_fragment(g->frag[i]); }
        if (g->d_frag_tab[i]) { DeviceGuard guard((int)i); (void)hipFree(g->d_frag_tab[i]); g->d_frag_tab[i] = nullptr; }
    }
    if (g->owns_csr) {
        host_free_space(g->csr_node_index_cpu);
        host_free_space(g->csr_dst_node_ids_cpu);
        g->owns_csr = false;
    }
}
int32_t GPUGraphStorage_GetPartitionCount(const GPUGraphStorage* g) { return g->partition_count; }
int64_t* GPUGraphStorage_GetCSRNodeIndexCPU(const GPUGraphStorage* g) { return g->csr_node_index_cpu; }
int32_t* GPUGraphStorage_GetCSRNodeMatrixCPU(const GPUGraphStorage* g) { return g->csr_dst_node_ids_cpu; }
static bool frag_args_ok(const GPUGraphStorage* g, int32_t dev_id, int32_t part_id)
{
    return g && dev_id >= 0 && dev_id < g->partition_count && part_id >= 0 && part_id < g->partition_count;
}
int64_t* GPUGraphStorage_GetFragmentIndex(const GPUGraphStorage* g, int32_t dev_id, int32_t part_id)
{   // first chunk (the whole indptr when the fragment has one chunk)
    return frag_args_ok(g, dev_id, part_id) && g->view[dev_id][part_id] ? g->frag[part_id].ip.at(0) : nullptr;
}
int32_t* GPUGraphStorage_GetFragmentMatrix(const GPUGraphStorage* g, int32_t dev_id, int32_t part_id)
{
    return frag_args_ok(g, dev_id, part_id) && g->view[dev_id][part_id] ? g->frag[part_id].ix.at(0) : nullptr;
}
int32_t GPUGraphStorage_FragmentRows(const GPUGraphStorage* g, int32_t dev_id) { return frag_args_ok(g, dev_id, 0) ? g->frag[dev_id].rows : 0; }
int64_t GPUGraphStorage_FragmentEdges(const GPUGraphStorage* g, int32_t dev_id) { return frag_args_ok(g, dev_id, 0) ? g->frag[dev_id].edges : 0; }
int32_t GPUGraphStorage_FragmentChunkCount(const GPUGraphStorage* g, int32_t dev_id, int32_t which)
{
    if (!frag_args_ok(g, dev_id, 0)) return 0;
    return which == 0 ? (int32_t)g->frag[dev_id].ip.chunks.size() : (int32_t)g->frag[dev_id].ix.chunks.size();
}
int64_t GPUGraphStorage_FragmentChunkSpan(const GPUGraphStorage* g, int32_t which)
{
    return g ? (1ll << (which == 0 ? g->row_shift : g->edge_shift)) : 0;
}
void* GPUGraphStorage_GetFragmentChunk(const GPUGraphStorage* g, int32_t dev_id, int32_t which, int32_t chunk)
{
    if (!frag_args_ok(g, dev_id, 0)) return nullptr;
    return which == 0 ? (void*)g->frag[dev_id].ip.at(chunk) : (void*)g->frag[dev_id].ix.at(chunk);
}
int GPUGraphStorage_ExportFragmentChunk(GPUGraphStorage* g, int32_t dev_id, int32_t which, int32_t chunk, void* handle64)
{
    if (!frag_args_ok(g, dev_id, 0)) { LEGION_ARG_ERROR("ExportFragmentChunk: no such local chunk"); return -1; }
    const auto& f = g->frag[dev_id];
    return which == 0 ? f.ip.export_chunk(dev_id, chunk, handle64, "ExportFragmentChunk") : f.ix.export_chunk(dev_id, chunk, handle64, "ExportFragmentChunk");
}
int GPUGraphStorage_ImportFragmentChunk(GPUGraphStorage* g, int32_t owner_dev, int32_t viewer_dev, int32_t which, int32_t chunk,
                                        const void* handle64, int32_t rows, int64_t edges)
{
    if (!frag_args_ok(g, owner_dev, viewer_dev) || !handle64 || !is_remote_device(owner_dev) || rows <= 0 || edges < 0) { LEGION_ARG_ERROR("ImportFragmentChunk: owner must be a remote member"); return -1; }
    GPUGraphStorage::Fragment& f = g->frag[owner_dev];
    if (!f.ip.imported) {
        f.rows = rows; f.edges = edges; f.ip.imported = f.ix.imported = true;
        f.ip.chunks.assign(chunk_count(rows, g->row_shift), nullptr);
        f.ix.chunks.assign(chunk_count(edges, g->edge_shift), nullptr);
    }
    if (f.rows != rows || f.edges != edges) { LEGION_ARG_ERROR("ImportFragmentChunk: rows/edges differ from the first chunk's"); return -1; }
    const int n = which == 0 ? (int)f.ip.chunks.size() : (int)f.ix.chunks.size();
    if (chunk < 0 || chunk >= n) { LEGION_ARG_ERROR("ImportFragmentChunk: chunk out of range"); return -1; }
    // the viewer opens the chunk, once; floor: a lower bound of what the exporter allocated for it
    auto open = [&](auto& list, int64_t floor) { return list.chunks[chunk] ? 0 : list.import_chunk(chunk, handle64, floor, viewer_dev, "ImportFragmentChunk"); };
    if ((which == 0 ? open(f.ip, (std::min<int64_t>(rows, 1ll << g->row_shift) + 1) * (int64_t)sizeof(int64_t))
                    : open(f.ix, std::min<int64_t>(edges, 1ll << g->edge_shift) * (int64_t)sizeof(int32_t))) != 0) return -1;
    g->view[viewer_dev][owner_dev] = true;
    f.complete = f.ip.complete(chunk_count(rows, g->row_shift)) && f.ix.complete(chunk_count(edges, g->edge_shift));
    if (f.complete) publish_fragment_tables(g);
    return 0;
}
int GPUGraphStorage_ExportFragment(GPUGraphStorage* g, int32_t dev_id, void* handle_indptr64, void* handle_indices64, int32_t* rows_out)
{   // single-chunk fragments only; chunked fragments use the *Chunk calls
    if (GPUGraphStorage_FragmentChunkCount(g, dev_id, 0) != 1 || GPUGraphStorage_FragmentChunkCount(g, dev_id, 1) != 1) { LEGION_ARG_ERROR("ExportFragment: fragment has several chunks, use ExportFragmentChunk"); return -1; }
    if (rows_out) *rows_out = g->frag[dev_id].rows;
    if (GPUGraphStorage_ExportFragmentChunk(g, dev_id, 0, 0, handle_indptr64) != 0) return -1;
    return GPUGraphStorage_ExportFragmentChunk(g, dev_id, 1, 0, handle_indices64);
}
int GPUGraphStorage_ImportFragment(GPUGraphStorage* g, int32_t owner_dev, int32_t viewer_dev, const void* handle_indptr64,
                                   const void* handle_indices64, int32_t rows)
{   // single-chunk form: the edge count is not known here, any value inside the first chunk selects one chunk
    if (GPUGraphStorage_ImportFragmentChunk(g, owner_dev, viewer_dev, 0, 0, handle_indptr64, rows, 1) != 0) return -1;
    return GPUGraphStorage_ImportFragmentChunk(g, owner_dev, viewer_dev, 1, 0, handle_indices64, rows, 1);
}
void GPUGraphStorage_Delete(GPUGraphStorage* g)
{
    if (!g) return;
    GPUGraphStorage_Finalize(g);
    delete g;
}

// ================================= node storage =====================================================
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

int64_t GPUNodeStorage_ReplicateToDevices(GPUNodeStorage* n)
{
    if (!n || !n->float_attrs || n->features_location == LEGION_LOC_DEVICE) return 0;
    const int32_t F = n->float_attr_len, pitch = legion_row_pitch(F);
    const int64_t V = n->total_num_nodes;
    n->replica_pitch = pitch;
    if (pitch == n->float_attr_pitch) {
        replicate_table<float>(n->float_attrs, V * pitch, n->partition_count, n->replica_attrs);
        return V * pitch * 4;
    }
    // the replica gets a line-aligned row pitch (legion_row_pitch): one pitched copy per distinct physical device
    std::vector<std::pair<int, float*>> per_phys;
    for (int p = 0; p < n->partition_count; p++) {
        if (is_remote_device(p) || n->replica_attrs[p]) continue;
        const int phys = physical_device(p);
        float* have = nullptr;
        for (auto& e : per_phys) if (e.first == phys) have = e.second;
        if (!have) {
            DeviceGuard guard(p);
            HIP_CHECK(hipMalloc(&have, (size_t)V * pitch * sizeof(float)));
            if (have) {
                HIP_CHECK(hipMemset(have, 0, (size_t)V * pitch * sizeof(float)));
                HIP_CHECK(hipMemcpy2D(have, (size_t)pitch * sizeof(float), n->float_attrs, (size_t)n->float_attr_pitch * sizeof(float),
                                      (size_t)F * sizeof(float), (size_t)V, hipMemcpyDefault));
            }
            per_phys.emplace_back(phys, have);
        }
        LEGION_AUDIT_SHARE(have, p);
        n->replica_attrs[p] = have;
    }
    return V * pitch * 4;
}

void GPUNodeStorage_Finalize(GPUNodeStorage* n)
{
    if (!n) return;
    free_replicas(n->replica_attrs);
    for (auto& sets : n->seeds)
        for (auto& set : sets) {
            if (set.ids) (void)hipFree(set.ids);
            if (set.labels) (void)hipFree(set.labels);
            set.ids = set.labels = nullptr;
        }
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

// ================================= memory pool ======================================================
GPUMemoryPool::GPUMemoryPool(int32_t depth)
{
    pipeline_depth = depth > 0 ? depth : 1;
    float_features.assign(pipeline_depth, nullptr);
    labels.assign(pipeline_depth, nullptr);
    node_counter.assign(pipeline_depth, nullptr);
    edge_counter.assign(pipeline_depth, nullptr);
    sampled_ids.assign(pipeline_depth, nullptr);
    agg_src_off.assign(pipeline_depth, nullptr);
    agg_dst_off.assign(pipeline_depth, nullptr);
}

// The per-pipe buffers of the aggregated modes, on the current device: the draw buffers of the aggregated last hop (cand_pipe) and, for
// the normalised sums, agg_out_deg / agg_wdraw / agg_chunk_cnt.  What is there stays.
static void alloc_mode_buffers(GPUMemoryPool* p)
{
    if (!p->modes.agg_last_hop || !p->owns_scratch) return;
    p->cand_pipe.resize(p->pipeline_depth, nullptr);
    for (auto& c : p->cand_pipe)
        if (!c) HIP_CHECK(hipMalloc(&c, (size_t)p->max_slots * sizeof(int32_t)));
    if (!p->modes.agg_norm) return;
    p->agg_out_deg.resize(p->pipeline_depth, nullptr);
    p->agg_wdraw.resize(p->pipeline_depth, nullptr);
    p->agg_chunk_cnt.resize(p->pipeline_depth, nullptr);
    for (auto& d : p->agg_out_deg)
        if (!d) HIP_CHECK(hipMalloc(&d, (size_t)p->num_ids * sizeof(int32_t)));
    for (auto& w : p->agg_wdraw)
        if (!w) HIP_CHECK(hipMalloc(&w, (size_t)p->max_slots * sizeof(float)));
    for (auto& c : p->agg_chunk_cnt)
        if (!c) HIP_CHECK(hipMalloc(&c, (size_t)legion::kMaxChunks * sizeof(int32_t)));
}

bool legion::pool_apply_modes(GPUMemoryPool* p, const ServeModes& wanted, const char* who)
{
    const std::string name(who);
    if (!p) { LEGION_ARG_ERROR((name + ": null pool").c_str()); return false; }
    if (p->capturing) { LEGION_ARG_ERROR((name + ": the pool is being captured").c_str()); return false; }
    if (wanted.agg_norm != 0 && wanted.agg_norm != 1) { LEGION_ARG_ERROR("GPUMemoryPool_SetAggNorm: unknown norm (0 = none, 1 = out-degree rsqrt)"); return false; }
    if (wanted.agg_norm && !wanted.agg_last_hop && wanted.agg_norm != p->modes.agg_norm) { LEGION_ARG_ERROR("GPUMemoryPool_SetAggNorm: the pool does not aggregate the last hop (GPUMemoryPool_SetAggLastHop first): only neighbour sums are normalised"); return false; }
    if (wanted.sampling != kSamplingReplace && wanted.sampling != kSamplingDistinct && wanted.sampling != kSamplingWeighted) { LEGION_ARG_ERROR("GPUMemoryPool_SetSampling: unknown sampling kind (0 = replace, 1 = distinct, 2 = weighted)"); return false; }
    if (wanted.lp_draw < 0) { LEGION_ARG_ERROR("GPUMemoryPool_SetLpDraw: negative triples per batch (0 = off, k > 0 = batches of 3 k)"); return false; }
    if (wanted.lp_draw > 0 && !p->lp_graph) { LEGION_ARG_ERROR("GPUMemoryPool_SetLpDraw: null graph: the positives are neighbours read from it"); return false; }
    if (wanted.seed != p->modes.seed) p->shuf_valid = false;   // the copy holds another seed's permutation (off and on again under one seed keeps it)
    if (wanted.lp_draw != p->modes.lp_draw) p->shuf_valid = false;   // ... or was shuffled by seeds, not by triples of this k
    if (wanted.seeded != p->modes.seeded || wanted.seed != p->modes.seed) p->ctl_synced = false;   // ctl holds the other state's draw word: a batch graph must reset the cursor
    p->modes = wanted;
    alloc_mode_buffers(p);
    return true;
}

extern "C" {

GPUMemoryPool* NewGPUMemoryPool(int32_t pipeline_depth) { return new GPUMemoryPool(pipeline_depth); }

// Server.cu:184-196 (num_ids_) and :216-231 (scratch), sized for H hops
void GPUMemoryPool_AllocateScratch(GPUMemoryPool* p, int32_t total_num_nodes, int32_t batch_size,
                                   const int32_t* fanout, int32_t hops)
{
    if (!p || hops < 1 || hops > LEGION_MAX_HOPS || batch_size < 1 || total_num_nodes < 1) { LEGION_ARG_ERROR("GPUMemoryPool_AllocateScratch: bad arguments"); return; }
    if (p->owns_scratch) GPUMemoryPool_Finalize(p); // re-sizing an initialised pool: release the old scratch first
    p->V = total_num_nodes; p->batch_size = batch_size; p->hops = hops;
    int64_t ids = batch_size, cur = batch_size, max_slots = 0;
    p->level_bound[0] = batch_size;
    for (int h = 0; h < hops; h++) {
        p->fanout[h] = fanout[h];
        cur *= fanout[h];
        if (cur > max_slots) max_slots = cur;
        ids += cur;
        if (ids >= (1ll << 31)) { LEGION_ARG_ERROR("GPUMemoryPool_AllocateScratch: batch*fanouts exceeds int32"); return; }
        if (cur >= (1ll << 30)) { LEGION_ARG_ERROR("GPUMemoryPool_AllocateScratch: a hop of 2^30 or more slots exceeds the slot-state encoding"); return; }
        p->level_bound[h + 1] = (int32_t)cur;
    }
    p->num_ids = (int32_t)ids;
    p->max_slots = (int32_t)max_slots;
    p->max_tiles = (int32_t)sampler_max_tiles(max_slots);   // the narrow hops run smaller tiles (internal.h)
    p->owns_scratch = true;
    HIP_CHECK(hipMalloc(&p->pos_map, (size_t)total_num_nodes * sizeof(pos_t)));
    HIP_CHECK(hipMemset(p->pos_map, 0xFF, (size_t)total_num_nodes * sizeof(pos_t)));
    p->batch_serial = 0;
    HIP_CHECK(hipMalloc(&p->ctl, sizeof(BatchCtl)));
    { const BatchCtl c{0, kEpochTop}; HIP_CHECK(hipMemcpy(p->ctl, &c, sizeof(c), hipMemcpyHostToDevice)); }
    p->ctl_synced = false;
    HIP_CHECK(hipHostMalloc((void**)&p->rows_seen, kRowsSeenWords * sizeof(int32_t), hipHostMallocMapped));
    memset(p->rows_seen, 0, kRowsSeenWords * sizeof(int32_t));
    HIP_CHECK(hipHostGetDevicePointer((void**)&p->rows_seen_dev, p->rows_seen, 0));
    HIP_CHECK(hipMalloc(&p->cand, (size_t)p->max_slots * sizeof(int32_t)));
    for (auto& a : p->aux2) HIP_CHECK(hipMalloc(&a, (size_t)p->max_slots * sizeof(int32_t)));
    HIP_CHECK(hipMalloc(&p->tile_edge, (size_t)(p->max_tiles + 1) * sizeof(int32_t)));
    HIP_CHECK(hipMalloc(&p->tile_node, (size_t)(p->max_tiles + 1) * sizeof(int32_t)));
    HIP_CHECK(hipMalloc(&p->tile_pre, (size_t)(p->max_tiles + 1) * sizeof(int2)));
    HIP_CHECK(hipMalloc(&p->chunk_tot, (size_t)kMaxChunks * sizeof(int2)));
    HIP_CHECK(hipMalloc(&p->hop_state, sizeof(HopState)));
    HIP_CHECK(hipMalloc(&p->cache_search_buffer, (size_t)p->num_ids * sizeof(int32_t)));
    HIP_CHECK(hipMalloc((void**)&p->row_ptr, (size_t)p->num_ids * sizeof(float*)));
    HIP_CHECK(hipMalloc(&p->agg_src_ids, (size_t)p->num_ids * sizeof(int32_t)));
    HIP_CHECK(hipMalloc(&p->tmp_part_ind, (size_t)p->num_ids));
    HIP_CHECK(hipMalloc(&p->tmp_part_off, (size_t)p->num_ids * sizeof(int32_t)));
    alloc_mode_buffers(p);
    HIP_CHECK(hipDeviceSynchronize());
}
int32_t GPUMemoryPool_NumIds(const GPUMemoryPool* p) { return p->num_ids; }

// The mode setters: the pool's modes with one field changed, through pool_apply_modes (internal.h: what is refused, what is
// allocated).  Call them under the device the pool's scratch lives on.  Aggregated last hop: INTEGRATION.md "Aggregated last hop";
// norm: 0 = plain sums, 1 = out-degree rsqrt ("Normalised sums"); distinct draws: "Sampling without replacement", nothing is allocated;
// seed: "Seeded sampling", seed 0 is a seed like any other, nothing is allocated here (GPUMemoryPool_BeginRound fills the shuffled copy);
// drawn link-prediction thirds: "Drawn link-prediction thirds", k triples per batch (0 = off) and the graph the positives are read from,
// which the pool keeps (and forgets when the mode is switched off); nothing is allocated.
static ServeModes modes_of(const GPUMemoryPool* p) { return p ? p->modes : ServeModes(); }
void GPUMemoryPool_SetAggLastHop(GPUMemoryPool* p, int on) { ServeModes m = modes_of(p); m.agg_last_hop = on != 0; pool_apply_modes(p, m, "GPUMemoryPool_SetAggLastHop"); }
void GPUMemoryPool_SetAggNorm(GPUMemoryPool* p, int norm) { ServeModes m = modes_of(p); m.agg_norm = norm; pool_apply_modes(p, m, "GPUMemoryPool_SetAggNorm"); }
void GPUMemoryPool_SetSampleDistinct(GPUMemoryPool* p, int on) { ServeModes m = modes_of(p); m.sampling = on != 0; pool_apply_modes(p, m, "GPUMemoryPool_SetSampleDistinct"); }
// the sampling kind as the enumeration it is: 0 = replace, 1 = distinct (what SetSampleDistinct(1) sets), 2 = weighted ("Weighted sampling":
// nothing is allocated here, the alias table belongs to the graph: GPUGraphStorage_SetEdgeWeights)
void GPUMemoryPool_SetSampling(GPUMemoryPool* p, int kind) { ServeModes m = modes_of(p); m.sampling = kind; pool_apply_modes(p, m, "GPUMemoryPool_SetSampling"); }
int GPUMemoryPool_GetSampling(const GPUMemoryPool* p) { return p ? p->modes.sampling : 0; }
// weighted sampling without replacement ("Weighted sampling without replacement"): a flag on top of the weighted kind, remembered across
// kinds and acting only while the kind is 2; nothing is allocated here, the weights belong to the graph (GPUGraphStorage_RetainEdgeWeights)
void GPUMemoryPool_SetWeightedDistinct(GPUMemoryPool* p, int on) { ServeModes m = modes_of(p); m.weighted_distinct = on != 0; pool_apply_modes(p, m, "GPUMemoryPool_SetWeightedDistinct"); }
int GPUMemoryPool_GetWeightedDistinct(const GPUMemoryPool* p) { return p && p->modes.weighted_distinct ? 1 : 0; }
// shared-key sampling ("Shared-key sampling"): a flag on top of the distinct kind, remembered across kinds and acting only while the kind
// is 1; nothing is allocated.  An unseeded pool draws under word 0: deterministic, the same node keys in every batch
void GPUMemoryPool_SetSharedDraws(GPUMemoryPool* p, int on) { ServeModes m = modes_of(p); m.shared_draws = on != 0; pool_apply_modes(p, m, "GPUMemoryPool_SetSharedDraws"); }
int GPUMemoryPool_GetSharedDraws(const GPUMemoryPool* p) { return p && p->modes.shared_draws ? 1 : 0; }
void GPUMemoryPool_SetSampleSeed(GPUMemoryPool* p, int on, uint32_t seed)
{
    ServeModes m = modes_of(p);
    m.seeded = on != 0; m.seed = seed;
    if (pool_apply_modes(p, m, "GPUMemoryPool_SetSampleSeed")) p->ctl_synced = false;   // this call always has the next graph replay reset its cursor
}
void GPUMemoryPool_SetLpDraw(GPUMemoryPool* p, int32_t triples_per_batch, GPUGraphStorage* graph)
{
    ServeModes m = modes_of(p);
    m.lp_draw = triples_per_batch;
    GPUGraphStorage* const before = p ? p->lp_graph : nullptr;
    if (p && !p->capturing) p->lp_graph = triples_per_batch > 0 ? graph : nullptr;
    if (!pool_apply_modes(p, m, "GPUMemoryPool_SetLpDraw") && p && !p->capturing) p->lp_graph = before;
}
int32_t GPUMemoryPool_GetLpDraw(const GPUMemoryPool* p) { return p ? p->modes.lp_draw : 0; }
int GPUMemoryPool_GetAggLastHop(const GPUMemoryPool* p) { return p && p->modes.agg_last_hop ? 1 : 0; }
int GPUMemoryPool_GetAggNorm(const GPUMemoryPool* p) { return p ? p->modes.agg_norm : 0; }
int GPUMemoryPool_GetSampleDistinct(const GPUMemoryPool* p) { return p && p->modes.sampling == kSamplingDistinct ? 1 : 0; }
int GPUMemoryPool_GetSampleSeed(const GPUMemoryPool* p, uint32_t* seed)
{
    if (seed) *seed = p ? p->modes.seed : 0;
    return p && p->modes.seeded ? 1 : 0;
}
// the current pipe's block out-degrees as the last normalised batch left them (int32[legion_batch_nodes(nc, H)]); null before the mode was set
int32_t* GPUMemoryPool_GetAggOutDeg(const GPUMemoryPool* p)
{
    if (!p || p->current_pipe < 0 || p->current_pipe >= (int)p->agg_out_deg.size()) return nullptr;
    return p->agg_out_deg[p->current_pipe];
}
int32_t GPUMemoryPool_GetRound(const GPUMemoryPool* p) { return p ? (int32_t)p->round : 0; }

// A new round (the trainer's epoch) begins: the draw words and the shuffle of the batches that follow are those of `round`.  Under a seed the
// pool's shuffled copy of (noder, dev_id)'s training list is (re)filled on `stream` -- the stream the batch generator runs on, so that the
// first k_seed of the round is ordered behind it.  noder == null: the training list stays in file order (lists served verbatim, e.g.
// link-prediction thirds); the draws are seeded all the same.  With the mode off the round is recorded and nothing is launched.
int GPUMemoryPool_BeginRound(void* stream, GPUMemoryPool* p, GPUNodeStorage* noder, int32_t dev_id, int32_t round)
{
    if (!p) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: null pool"); return -1; }
    if (p->capturing) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: the pool is being captured (a round begins between batches, not inside a recording)"); return -1; }
    if (round < 0) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: negative round"); return -1; }
    if (p->round != (uint32_t)round) p->shuf_valid = false;   // whatever the mode: the copy holds another round's permutation
    p->round = (uint32_t)round;
    p->ctl_synced = false;   // the next replay resets the cursor: k_set_cursor carries the round's draw key
    if (!p->modes.seeded) return 0;
    p->shuf_file_order = noder == nullptr;
    p->shuf_valid = false;
    if (!noder) return 0;
    if (!p->owns_scratch) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: GPUMemoryPool_AllocateScratch was not called"); return -1; }
    const GPUNodeStorage::SeedSet& set = noder->seed_set(LEGION_TRAINMODE, dev_id);
    if (set.num > 0 && (!set.ids || !set.labels)) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: the training list of this device is not built"); return -1; }
    const int32_t k = p->modes.lp_draw;   // drawn link-prediction thirds: whole triples move
    if (k > 0 && set.num % (3 * k) != 0) { LEGION_ARG_ERROR("GPUMemoryPool_BeginRound: drawn link-prediction thirds (GPUMemoryPool_SetLpDraw): the training list's length is not a multiple of the batch of 3 k ([src | pos | neg] thirds, padded)"); return -1; }
    if (set.num > p->shuf_cap || !p->shuf_ids) {   // first use, or a longer list: batches that read the old copy may still be in flight
        HIP_CHECK(hipDeviceSynchronize());
        if (p->shuf_ids) (void)hipFree(p->shuf_ids);
        if (p->shuf_labels) (void)hipFree(p->shuf_labels);
        p->shuf_ids = p->shuf_labels = nullptr;
        p->shuf_cap = std::max(set.num, 1);
        HIP_CHECK(hipMalloc(&p->shuf_ids, (size_t)p->shuf_cap * sizeof(int32_t)));
        HIP_CHECK(hipMalloc(&p->shuf_labels, (size_t)p->shuf_cap * sizeof(int32_t)));
        if (!p->shuf_ids || !p->shuf_labels) return -1;
    }
    if (k > 0) launch_shuffle_triples((hipStream_t)stream, set.ids, set.labels, set.num, k, seeded_shuffle_key(p->modes.seed, p->round), p->shuf_ids, p->shuf_labels);
    else launch_shuffle_seeds((hipStream_t)stream, set.ids, set.labels, set.num, seeded_shuffle_key(p->modes.seed, p->round), p->shuf_ids, p->shuf_labels);
    p->shuf_n = set.num;
    p->shuf_src = set.ids;
    p->shuf_valid = true;
    return error_pending() ? -1 : 0;
}

#define POOL_PIPE_SETTER(name, field, type) \
    void GPUMemoryPool_Set##name(GPUMemoryPool* p, type* ptr, int32_t pipe) { \
        if (pipe < 0 || pipe >= p->pipeline_depth) { LEGION_ARG_ERROR("GPUMemoryPool_Set" #name ": bad pipe"); return; } \
        p->field[pipe] = ptr; } \
    type* GPUMemoryPool_Get##name(const GPUMemoryPool* p) { return p->field[p->current_pipe]; }
POOL_PIPE_SETTER(SampledIds, sampled_ids, int32_t)
POOL_PIPE_SETTER(FloatFeatures, float_features, float)
POOL_PIPE_SETTER(Labels, labels, int32_t)
POOL_PIPE_SETTER(AggSrcOf, agg_src_off, int32_t)
POOL_PIPE_SETTER(AggDstOf, agg_dst_off, int32_t)
POOL_PIPE_SETTER(NodeCounter, node_counter, int32_t)
POOL_PIPE_SETTER(EdgeCounter, edge_counter, int32_t)
#undef POOL_PIPE_SETTER
void GPUMemoryPool_SetFeatureRows(GPUMemoryPool* p, int32_t rows) { p->feature_rows = rows; }
void GPUMemoryPool_SetCurrentPipe(GPUMemoryPool* p, int32_t pipe) { p->current_pipe = pipe % p->pipeline_depth; }
void GPUMemoryPool_SetCurrentMode(GPUMemoryPool* p, int32_t mode) { p->mode = mode; }
void GPUMemoryPool_SetIter(GPUMemoryPool* p, int32_t iter) { p->iter = iter; }
int32_t GPUMemoryPool_GetCurrentMode(const GPUMemoryPool* p) { return p->mode; }
int32_t GPUMemoryPool_GetIter(const GPUMemoryPool* p) { return p->iter; }
int32_t* GPUMemoryPool_GetAggSrcId(const GPUMemoryPool* p) { return p->agg_src_ids; }
int32_t* GPUMemoryPool_GetCacheSearchBuffer(const GPUMemoryPool* p) { return p->cache_search_buffer; }
char* GPUMemoryPool_GetTmpPartIdx(const GPUMemoryPool* p) { return (char*)p->tmp_part_ind; }
int32_t* GPUMemoryPool_GetTmpPartOff(const GPUMemoryPool* p) { return p->tmp_part_off; }
uint64_t* GPUMemoryPool_GetPositionMap(const GPUMemoryPool* p) { return (uint64_t*)p->pos_map; }
int32_t* GPUMemoryPool_GetCandidateBuffer(const GPUMemoryPool* p) { return p->cand; }
uint32_t GPUMemoryPool_GetBatchSerial(const GPUMemoryPool* p) { return p->batch_serial; }
void GPUMemoryPool_SetBatchSerial(GPUMemoryPool* p, uint32_t serial) { p->batch_serial = serial; p->ctl_synced = false; }

void GPUMemoryPool_Finalize(GPUMemoryPool* p)
{
    if (!p || !p->owns_scratch) return;
    GPUMemoryPool_ReleasePeerExchange(p);
    (void)hipFree(p->pos_map); (void)hipFree(p->cand); for (auto& a : p->aux2) { (void)hipFree(a); a = nullptr; } (void)hipFree(p->tile_edge); (void)hipFree(p->tile_node); (void)hipFree(p->tile_pre); (void)hipFree(p->chunk_tot); p->tile_pre = p->chunk_tot = nullptr;
    (void)hipFree(p->hop_state); (void)hipFree(p->cache_search_buffer); (void)hipFree((void*)p->row_ptr); p->row_ptr = nullptr; (void)hipFree(p->agg_src_ids);
    (void)hipFree(p->tmp_part_ind); (void)hipFree(p->tmp_part_off); (void)hipFree(p->ctl); p->ctl = nullptr; if (p->rows_seen) { (void)hipHostFree(p->rows_seen); p->rows_seen = nullptr; p->rows_seen_dev = nullptr; }
    for (auto& c : p->cand_pipe) { (void)hipFree(c); c = nullptr; }
    for (auto& c : p->agg_out_deg) { (void)hipFree(c); c = nullptr; }
    for (auto& c : p->agg_wdraw) { (void)hipFree(c); c = nullptr; }
    for (auto& c : p->agg_chunk_cnt) { (void)hipFree(c); c = nullptr; }
    if (p->shuf_ids) (void)hipFree(p->shuf_ids);
    if (p->shuf_labels) (void)hipFree(p->shuf_labels);
    p->shuf_ids = p->shuf_labels = nullptr; p->shuf_cap = p->shuf_n = 0; p->shuf_src = nullptr; p->shuf_valid = false;
    p->pos_map = nullptr; p->cand = nullptr; p->tile_edge = p->tile_node = nullptr; p->hop_state = nullptr;
    p->cache_search_buffer = p->agg_src_ids = p->tmp_part_off = nullptr; p->tmp_part_ind = nullptr;
    p->owns_scratch = false;
}
void GPUMemoryPool_Delete(GPUMemoryPool* p)
{
    if (!p) return;
    GPUMemoryPool_Finalize(p);
    delete p;
}

} // extern "C"
