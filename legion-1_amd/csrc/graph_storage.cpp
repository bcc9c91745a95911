// graph_storage.cpp -- host mirror of GPUMemoryGraphStorage (GPU_Memory_Graph_Storage.cu:37-210): the whole CSR and its HBM replicas,
// the clique's CSR fragments (chunk lists, chunks.cpp) and the alias table of the weighted sampler modes.
#include "internal.h"

#include <algorithm>

#include "device_mem.h"

using namespace legion;

extern "C" {

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
    g->edge_feat.assign(P, nullptr);
    g->edge_feat_dim = 0;
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
        // the build's temporaries free themselves at the end of the iteration, newest first (d_chunks, then what is left of d_index)
        DeviceTemp<int64_t> neighbor_count, d_index; // d_index: contiguous build copy of the fragment's indptr
        HIP_CHECK(hipMalloc(&neighbor_count.p, (size_t)capacity * sizeof(int64_t)));
        HIP_CHECK(hipMalloc(&d_index.p, ((size_t)capacity + 1) * sizeof(int64_t)));
        HIP_CHECK(hipMemset(d_index.p, 0, sizeof(int64_t)));
        launch_neighbor_count(nullptr, QT, Kg, i, capacity, g->node_num, g->csr_node_index_cpu, neighbor_count.p);
        inclusive_scan_i64(nullptr, neighbor_count.p, d_index.p + 1, capacity);
        int64_t total = 0;
        HIP_CHECK(hipMemcpy(&total, d_index.p + capacity, sizeof(int64_t), hipMemcpyDeviceToHost));
        neighbor_count.reset();
        f.rows = capacity;
        f.edges = total;
        // indices chunks: chunk q ends where the last row that starts before its upper boundary ends
        const int nx = chunk_count(total, g->edge_shift);
        std::vector<int64_t> ends(nx, total);
        if (nx > 1) {
            DeviceTemp<int64_t> d_ends;
            HIP_CHECK(hipMalloc(&d_ends.p, (size_t)nx * sizeof(int64_t)));
            launch_chunk_ends(nullptr, d_index.p, capacity, g->edge_shift, nx, d_ends.p);
            HIP_CHECK(hipMemcpy(ends.data(), d_ends.p, (size_t)(nx - 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
        }
        f.ix.chunks.assign(nx, nullptr);
        for (int q = 0; q < nx; q++) {
            const int64_t elems = ends[q] - ((int64_t)q << g->edge_shift); // <= 0: no row starts in this chunk
            HIP_CHECK(hipMalloc(&f.ix.chunks[q], (size_t)(elems > 0 ? elems : 1) * sizeof(int32_t)));
        }
        DeviceTemp<int32_t*> d_chunks;
        HIP_CHECK(hipMalloc(&d_chunks.p, ((size_t)nx + 1) * sizeof(int32_t*))); // +1: see publish_fragment_tables
        HIP_CHECK(hipMemcpy(d_chunks.p, f.ix.chunks.data(), (size_t)nx * sizeof(int32_t*), hipMemcpyHostToDevice));
        launch_topo_fill_up(nullptr, QT, Kg, i, capacity, g->node_num, g->csr_node_index_cpu, g->csr_dst_node_ids_cpu, d_index.p, d_chunks.p, g->edge_shift);
        // indptr chunks (one entry of overlap); a single chunk adopts the build copy
        const int np = chunk_count(capacity, g->row_shift);
        if (np == 1) f.ip.chunks.assign(1, d_index.release());
        else {
            f.ip.chunks.assign(np, nullptr);
            const int64_t rpc = 1ll << g->row_shift;
            for (int q = 0; q < np; q++) {
                const int64_t r0 = q * rpc, n = std::min<int64_t>(rpc, capacity - r0) + 1;
                HIP_CHECK(hipMalloc(&f.ip.chunks[q], (size_t)n * sizeof(int64_t)));
                HIP_CHECK(hipMemcpy(f.ip.chunks[q], d_index.p + r0, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice));
            }
        }
        HIP_CHECK(hipDeviceSynchronize());
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
    const int64_t np = (int64_t)g->node_num + 1;
    replicate_table<int64_t>(g->csr_node_index_cpu, 1, np, np, np, g->replica_indptr);
    replicate_table<int32_t>(g->csr_dst_node_ids_cpu, 1, g->edge_num, g->edge_num, g->edge_num, g->replica_indices);
    return np * 8 + g->edge_num * 4;
}

// ---- weighted sampler mode: the graph's edge weights as an alias table (INTEGRATION.md "Weighted sampling") ----
// The table of the whole CSR on the current device (logical GPU dev), from the weights wherever they lie; null with a sticky error.
// *bad := the number of refused weights (then nothing is built).  The fp64 scratch is freed before returning, and so is the weights' device
// copy -- unless `kept` is given and the table was built: then *kept := the copy (weighted sampling without replacement reads it).
static AliasEntry* build_alias_here(const GPUGraphStorage* g, int dev, const float* w, unsigned long long* bad, float** kept)
{
    const int64_t E = g->edge_num;
    // whatever is not released to the caller is freed on every way out, newest first
    DeviceTemp<float> d_w;
    DeviceTemp<unsigned long long> d_bad;
    DeviceTemp<double> d_p;
    DeviceTemp<AliasEntry> table;
    HIP_CHECK(hipMalloc(&d_w.p, (size_t)E * sizeof(float)));
    HIP_CHECK(hipMalloc(&d_bad.p, sizeof(unsigned long long)));
    if (!d_w.p || !d_bad.p) return nullptr;
    HIP_CHECK(hipMemcpy(d_w.p, w, (size_t)E * sizeof(float), hipMemcpyDefault));
    HIP_CHECK(hipMemset(d_bad.p, 0, sizeof(unsigned long long)));
    launch_check_weights(nullptr, d_w.p, E, d_bad.p);
    *bad = ~0ull;
    HIP_CHECK(hipMemcpy(bad, d_bad.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (*bad != 0 || error_pending()) return nullptr;
    HIP_CHECK(hipMalloc(&d_p.p, (size_t)E * sizeof(double)));
    HIP_CHECK(hipMalloc(&table.p, (size_t)E * sizeof(AliasEntry)));
    if (d_p.p && table.p) {
        HIP_CHECK(hipMemset(table.p, 0, (size_t)E * sizeof(AliasEntry)));   // entries past a truncated degree are never drawn; keep them defined
        launch_build_alias(nullptr, g->replica_indptr[dev] ? g->replica_indptr[dev] : g->csr_node_index_cpu,
                           g->replica_indices[dev] ? g->replica_indices[dev] : g->csr_dst_node_ids_cpu, d_w.p, g->node_num, E, d_p.p, table.p);
        HIP_CHECK(hipDeviceSynchronize());
    }
    if (error_pending() || !table.p) return nullptr;
    if (kept) *kept = d_w.release();
    return table.release();
}

int GPUGraphStorage_SetEdgeWeights(GPUGraphStorage* g, const float* w, int32_t location)
{
    if (!g || g->alias.empty()) { LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeWeights: null graph, or GPUGraphStorage_Build was not called"); return -1; }
    if (w && location != LEGION_LOC_HOST_PINNED && location != LEGION_LOC_DEVICE && location != LEGION_LOC_HOST_PAGEABLE) { LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeWeights: location must be a LEGION_LOC_* value"); return -1; }
    const int P = g->partition_count;
    std::vector<AliasEntry*> fresh(P, nullptr);
    std::vector<float*> fresh_w(P, nullptr);
    if (w && g->edge_num > 0) {
        const std::vector<int> leader = device_leaders(P);   // table and retained weights in step: one copy of each per physical device
        for (int p = 0; p < P; p++) {
            if (leader[p] < 0) continue;
            if (leader[p] != p) { fresh[p] = fresh[leader[p]]; fresh_w[p] = fresh_w[leader[p]]; }
            else {
                DeviceGuard guard(p);
                unsigned long long bad = 0;
                fresh[p] = build_alias_here(g, p, w, &bad, g->retain_weights ? &fresh_w[p] : nullptr);
                if (!fresh[p]) {   // refused or failed: the earlier table stays
                    if (bad && !error_pending())
                        LEGION_ARG_ERROR(("GPUGraphStorage_SetEdgeWeights: " + std::to_string(bad) + " of " + std::to_string(g->edge_num) +
                                          " edge weights are negative, NaN or infinite: weights must be finite and >= 0 (the earlier table, if any, stays)").c_str());
                    else if (!error_pending()) LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeWeights: building the alias table failed");
                    free_replicas(fresh);
                    free_replicas(fresh_w);
                    return -1;
                }
            }
            LEGION_AUDIT_SHARE(fresh[p], p);
            if (fresh_w[p]) LEGION_AUDIT_SHARE(fresh_w[p], p);
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

// ---- edge features: a float32 [E, dim] table in CSR order (INTEGRATION.md "Edge features") ----
// Row e lies beside indices[e].  One device copy per physical device by the rule of the retained weights (device_leaders / free_replicas);
// x == NULL drops the table; a failed replacement keeps the earlier one, as SetEdgeWeights does.
int GPUGraphStorage_SetEdgeFeatures(GPUGraphStorage* g, const float* x, int32_t dim, int32_t location)
{
    if (!g || g->edge_feat.empty()) { LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeFeatures: null graph, or GPUGraphStorage_Build was not called"); return -1; }
    if (x && location != LEGION_LOC_HOST_PINNED && location != LEGION_LOC_DEVICE && location != LEGION_LOC_HOST_PAGEABLE) { LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeFeatures: location must be a LEGION_LOC_* value"); return -1; }
    if (x && dim < 1) { LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeFeatures: dim must be at least 1 (float32 [E, dim], dense)"); return -1; }
    int64_t bytes = 0;
    if (x && (__builtin_mul_overflow(g->edge_num, (int64_t)dim, &bytes) || __builtin_mul_overflow(bytes, (int64_t)sizeof(float), &bytes))) { LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeFeatures: the table's size, E * dim * 4 bytes, overflows"); return -1; }
    const int P = g->partition_count;
    std::vector<float*> fresh(P, nullptr);
    if (x && g->edge_num > 0) {
        const std::vector<int> leader = device_leaders(P);
        for (int p = 0; p < P; p++) {
            if (leader[p] < 0) continue;
            if (leader[p] != p) fresh[p] = fresh[leader[p]];
            else {
                DeviceGuard guard(p);
                HIP_CHECK(hipMalloc(&fresh[p], (size_t)bytes));
                if (fresh[p]) HIP_CHECK(hipMemcpy(fresh[p], x, (size_t)bytes, hipMemcpyDefault));
                if (!fresh[p] || error_pending()) {   // the earlier table stays
                    if (!error_pending()) LEGION_ARG_ERROR("GPUGraphStorage_SetEdgeFeatures: allocating the table failed");
                    free_replicas(fresh);
                    return -1;
                }
            }
            LEGION_AUDIT_SHARE(fresh[p], p);
        }
    }
    // gathers that read the earlier table may still be in flight
    for (int p = 0; p < P; p++)
        if (g->edge_feat[p] && !is_remote_device(p)) { DeviceGuard guard(p); HIP_CHECK(hipDeviceSynchronize()); }
    free_replicas(g->edge_feat);
    g->edge_feat = fresh;
    g->edge_feat_dim = x && g->edge_num > 0 ? dim : 0;
    return error_pending() ? -1 : 0;
}
int32_t GPUGraphStorage_GetEdgeFeatureDim(const GPUGraphStorage* g) { return g ? g->edge_feat_dim : 0; }
int GPUGraphStorage_CopyEdgeFeatureRows(const GPUGraphStorage* g, int32_t dev_id, int64_t e0, int64_t n, float* out)
{
    if (!g || dev_id < 0 || dev_id >= (int32_t)g->edge_feat.size() || !g->edge_feat[dev_id]) { LEGION_ARG_ERROR("GPUGraphStorage_CopyEdgeFeatureRows: this logical GPU holds no edge-feature table (GPUGraphStorage_SetEdgeFeatures)"); return -1; }
    if (e0 < 0 || n < 0 || e0 > g->edge_num - n) { LEGION_ARG_ERROR("GPUGraphStorage_CopyEdgeFeatureRows: rows outside [0, edge count)"); return -1; }
    if (n == 0) return 0;
    if (!out) { LEGION_ARG_ERROR("GPUGraphStorage_CopyEdgeFeatureRows: null output"); return -1; }
    DeviceGuard guard(dev_id);
    HIP_CHECK(hipMemcpy(out, g->edge_feat[dev_id] + e0 * g->edge_feat_dim, (size_t)n * g->edge_feat_dim * sizeof(float), hipMemcpyDeviceToHost));
    return error_pending() ? -1 : 0;
}

void GPUGraphStorage_Finalize(GPUGraphStorage* g)
{
    if (!g) return;
    free_replicas(g->alias);
    free_replicas(g->weights);
    free_replicas(g->edge_feat);
    g->edge_feat_dim = 0;
    free_replicas(g->replica_indptr);
    free_replicas(g->replica_indices);
    for (size_t i = 0; i < g->frag.size(); i++) {
        if (!is_remote_device((int)i) || g->frag[i].ip.imported) { DeviceGuard guard((int)i); free_fragment(g->frag[i]); }
        if (g->d_frag_tab[i]) { DeviceGuard guard((int)i); free_and_null(g->d_frag_tab[i]); }
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

} // extern "C"
