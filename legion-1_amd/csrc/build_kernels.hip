// build_kernels.hip -- everything that runs once per graph or per cache build and never in a served batch: hotness (the pre-sampling epoch's
// batches), the alias table of the weighted sampler mode, the cache maps and the fragments, with their launch wrappers.  (The sort and the
// scans: sort_scan.hip.)
#include "internal.h"
#include "draws.h"
#include "launch.h"

#include "audit_hooks.h"

namespace legion {

// S7: HotnessMeasure (GPUCache.cu:227-235)
__global__ __launch_bounds__(kBlock) void k_hotness(const int32_t* __restrict__ ids, const int32_t* __restrict__ nc,
                                                    int32_t hops, unsigned long long* __restrict__ access,
                                                    int32_t* __restrict__ max_ids)
{
    const int32_t n = hops > 0 ? legion_batch_nodes(nc, hops) : nc[LEGION_NC_TOTAL];
    // max_ids_ (GPUCache.cu:294-296) kept on the device: no blocking D2H per batch
    if (max_ids && blockIdx.x == 0 && threadIdx.x == 0) atomicMax(max_ids, n);
    for (int32_t i = threadIdx.x + blockDim.x * blockIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int32_t cid = ids[i];
        if (cid >= 0) atomicAdd(access + cid, 1ull);
    }
}

// ------------------------------------------------------------------------------------------------
// alias table of the weighted sampler mode (one-off per graph; GPUGraphStorage_SetEdgeWeights)
// ------------------------------------------------------------------------------------------------
// Weights that are negative, NaN or infinite.  The sum of the per-wave counts does not depend on the order they are added in.
__global__ void k_check_weights(const float* __restrict__ w, int64_t E, unsigned long long* bad)
{
    unsigned long long c = 0;
    for (int64_t i = threadIdx.x + (int64_t)blockDim.x * blockIdx.x; i < E; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = w[i];
        if (!(x >= 0.0f) || x > 3.402823466e+38f) c++;   // NaN fails the first test, +inf the second
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if (lane_id() == 0 && c) atomicAdd(bad, c);
}

__device__ inline uint32_t alias_thr(double p)   // floor(p * 2^32), saturated: p >= 1 - 2^-32 always keeps
{
    const double t = p * 4294967296.0;
    return t >= 4294967295.0 ? 0xFFFFFFFFu : (t > 0.0 ? (uint32_t)t : 0u);
}
// Vose's algorithm over one row, sequential, without work lists: p[k] = w[k] d / W on entry (fp64), out[k] = {always keep, own id} on
// entry.  `s` walks the columns once for the small ones (p < 1), `l` once for the large ones; the running large column's residual is
// held in a register, a large column that falls below 1 becomes a small one with its residual in p -- taken up at once when the small
// walk has passed it, found by that walk otherwise.  The last large column is never demoted: it stays the alias of every small column
// left (its residual is below 1 by rounding only), so a small column, and with it every zero weight, always gives its whole remainder to
// a column of positive weight.
__device__ inline void alias_vose(double* p, const int32_t* ids, AliasEntry* out, int32_t d)
{
    int32_t s = 0, l = 0;
    while (l < d && !(p[l] >= 1.0)) l++;
    if (l >= d) return;                       // no column above the mean (all equal up to rounding): every column keeps itself
    double pl = p[l];
    auto next_small = [&]() -> int32_t {
        while (s < d && (s == l || p[s] >= 1.0)) s++;
        return s < d ? s++ : -1;
    };
    int32_t cur = next_small();
    while (cur >= 0) {
        const double pc = p[cur];
        AliasEntry e;
        e.thr = alias_thr(pc); e.alias_id = ids[l];
        out[cur] = e;
        pl = (pl + pc) - 1.0;
        if (pl < 1.0) {
            int32_t l2 = l + 1;
            while (l2 < d && !(p[l2] >= 1.0)) l2++;
            if (l2 < d) {
                const int32_t demoted = l;
                p[demoted] = pl;
                l = l2; pl = p[l];
                cur = demoted < s ? demoted : next_small();
                continue;
            }
        }
        cur = next_small();
    }
}

// One lane per row of at most kAliasHubDegree neighbours: row sum in column order (fp64), p and the keep-itself entries, then alias_vose.
__global__ __launch_bounds__(kBlock) void k_build_alias(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, const float* __restrict__ w,
                                                        int32_t V, int64_t E, double* p, AliasEntry* table)
{
    const int32_t v = threadIdx.x + blockDim.x * blockIdx.x;
    if (v >= V) return;
    const int64_t start = indptr[v];
    const int32_t d = (int32_t)(indptr[v + 1] - start);   // int32 like the sampler's degree
    if (d <= 0 || d > kAliasHubDegree || start < 0 || start + d > E) return;
    double W = 0.0;
    for (int32_t k = 0; k < d; k++) W += (double)w[start + k];
    AliasEntry e;
    if (!(W > 0.0)) {
        e.thr = 0u; e.alias_id = -1;
        for (int32_t k = 0; k < d; k++) table[start + k] = e;
        return;
    }
    e.thr = 0xFFFFFFFFu;
    for (int32_t k = 0; k < d; k++) {
        p[start + k] = (double)w[start + k] * (double)d / W;
        e.alias_id = indices[start + k];
        table[start + k] = e;
    }
    alias_vose(p + start, indices + start, table + start, d);
}

// One wave per row of more than kAliasHubDegree neighbours (a workgroup is one wave): the lanes sum, scale and initialise the row together
// -- per-lane partial sums in column order, then a fixed butterfly, so the sum does not depend on timing --, lane 0 runs alias_vose.
__global__ __launch_bounds__(64) void k_build_alias_hub(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, const float* __restrict__ w,
                                                        int32_t V, int64_t E, double* p, AliasEntry* table)
{
    const int lane = threadIdx.x;
    for (int64_t base = (int64_t)blockIdx.x * 64; base < V; base += (int64_t)gridDim.x * 64) {
        const int64_t v = base + lane;
        int64_t my_start = 0;
        int32_t my_d = 0;
        if (v < V) { my_start = indptr[v]; my_d = (int32_t)(indptr[v + 1] - my_start); }
        unsigned long long hubs = __ballot(my_d > kAliasHubDegree && my_start >= 0 && my_start + my_d <= E);
        while (hubs) {
            const int src = __ffsll((long long)hubs) - 1;
            hubs &= hubs - 1;
            const int64_t start = __shfl(my_start, src);
            const int32_t d = __shfl(my_d, src);
            double W = 0.0;
            for (int32_t k = lane; k < d; k += 64) W += (double)w[start + k];
            for (int o = 32; o > 0; o >>= 1) W += __shfl_xor(W, o);   // a + b == b + a bit for bit: every lane holds the same sum
            AliasEntry e;
            if (!(W > 0.0)) {
                e.thr = 0u; e.alias_id = -1;
                for (int32_t k = lane; k < d; k += 64) table[start + k] = e;
                continue;
            }
            e.thr = 0xFFFFFFFFu;
            for (int32_t k = lane; k < d; k += 64) {
                p[start + k] = (double)w[start + k] * (double)d / W;
                e.alias_id = indices[start + k];
                table[start + k] = e;
            }
            __threadfence_block();
            __syncthreads();                  // lane 0 reads what the other lanes wrote
            if (lane == 0) alias_vose(p + start, indices + start, table + start, d);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// cache construction kernels (one-off; S8 / S9)
// ------------------------------------------------------------------------------------------------
__global__ void k_aggregate_access(unsigned long long* agg, const unsigned long long* add, int32_t n)
{   // GPUCache.cu:44-48
    for (int32_t i = threadIdx.x + blockDim.x * blockIdx.x; i < n; i += gridDim.x * blockDim.x) agg[i] += add[i];
}
__global__ void k_iota(int32_t* out, int32_t n)
{   // init_cache_order, GPUCache.cu:50-54
    for (int32_t i = threadIdx.x + blockDim.x * blockIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = i;
}
__global__ void k_fill_i32(int32_t* p, int32_t v, int64_t n)
{
    for (int64_t i = threadIdx.x + (int64_t)blockDim.x * blockIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void k_fill_i8(int8_t* p, int8_t v, int64_t n)
{
    for (int64_t i = threadIdx.x + (int64_t)blockDim.x * blockIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}
// InitPair (GPUCache.cu:103-108) scattered into the direct-mapped table: rank t -> slot
__global__ void k_build_feat_map(int32_t* feat_map, const int32_t* QF, int32_t capacity, int32_t Kg, int32_t V)
{
    const int64_t n = min((int64_t)capacity * Kg, (int64_t)V);
    for (int64_t t = threadIdx.x + (int64_t)blockDim.x * blockIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        feat_map[QF[t]] = (int32_t)((t % Kg) * capacity + t / Kg);
}
// InitIndexPair / InitOffsetPair (GPUCache.cu:88-100)
__global__ void k_build_topo_map(int8_t* owner, int32_t* row, const int32_t* QT, int32_t capacity, int32_t Kg,
                                 int32_t Ki, int32_t V)
{
    const int64_t n = min((int64_t)capacity * Kg, (int64_t)V);
    for (int64_t t = threadIdx.x + (int64_t)blockDim.x * blockIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        owner[QT[t]] = (int8_t)(t % Kg + Ki * Kg);
        row[QT[t]] = (int32_t)(t / Kg);
    }
}
// FeatFillUp (GPUCache.cu:200-205): cache row r of clique GPU Ki = features of QF[r*Kg + Ki]
__global__ void k_feat_fill_up(int32_t row0, int32_t rows, int32_t F, int32_t chunk_pitch, int32_t table_pitch, float* cache,
                               const float* table, const int32_t* QF, int32_t Kg, int32_t Ki, int32_t V)
{
    const int64_t n = (int64_t)rows * F;
    for (int64_t i = threadIdx.x + (int64_t)blockDim.x * blockIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lr = i / F, c = i % F, t = (row0 + lr) * Kg + Ki;
        if (t >= V) continue;
        cache[lr * chunk_pitch + c] = table[(int64_t)QF[t] * table_pitch + c];
    }
}
// dense / pitched row copy (HBM replica of a table with a line-aligned row pitch)
__global__ void k_copy_rows_pitched(float* dst, int32_t dst_pitch, const float* src, int32_t src_pitch, int32_t F, int64_t rows)
{
    const int64_t n = rows * F;
    for (int64_t i = threadIdx.x + (int64_t)blockDim.x * blockIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / F, c = i % F;
        dst[r * dst_pitch + c] = src[r * src_pitch + c];
    }
}
// GetNeighborCount (GPU_Memory_Graph_Storage.cu:14-20)
__global__ void k_neighbor_count(const int32_t* QT, int32_t Kg, int32_t Ki, int32_t capacity, int32_t V,
                                 const int64_t* indptr, int64_t* count_out)
{
    for (int32_t r = threadIdx.x + blockDim.x * blockIdx.x; r < capacity; r += gridDim.x * blockDim.x) {
        const int64_t t = (int64_t)r * Kg + Ki;
        int64_t c = 0;
        if (t < V) { int32_t id = QT[t]; c = indptr[id + 1] - indptr[id]; }
        count_out[r] = c;
    }
}
// TopoFillUp (GPU_Memory_Graph_Storage.cu:22-34); one wave per row, lanes stride the neighbours
__global__ void k_topo_fill_up(const int32_t* QT, int32_t Kg, int32_t Ki, int32_t capacity, int32_t V,
                               const int64_t* indptr, const int32_t* indices, const int64_t* frag_indptr,
                               int32_t* const* frag_chunks, int32_t edge_shift)
{
    const int32_t wave = (threadIdx.x + blockDim.x * blockIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int32_t r = wave; r < capacity; r += nwaves) {
        const int64_t t = (int64_t)r * Kg + Ki;
        if (t >= V) continue;
        const int32_t id = QT[t];
        const int64_t s = indptr[id], c = indptr[id + 1] - s, o = frag_indptr[r];
        int32_t* __restrict__ out = frag_chunks[o >> edge_shift] + (o & ((1ll << edge_shift) - 1)); // a row never leaves its chunk
        for (int64_t i = lane_id(); i < c; i += 64) out[i] = indices[s + i];
    }
}
// end offset of the last row starting before each chunk boundary: lower bound of the boundary in frag_indptr
__global__ void k_chunk_ends(const int64_t* frag_indptr, int32_t capacity, int32_t edge_shift, int32_t nch, int64_t* ends)
{
    const int32_t q = threadIdx.x + blockDim.x * blockIdx.x;
    if (q >= nch - 1) return;
    const int64_t boundary = (int64_t)(q + 1) << edge_shift;
    int32_t lo = 0, hi = capacity; // frag_indptr[capacity] = total >= boundary
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (frag_indptr[mid] < boundary) lo = mid + 1; else hi = mid;
    }
    ends[q] = frag_indptr[lo];
}
// GetEdgeMem (GPUCache.cu:35-41)
__global__ void k_edge_mem(const int32_t* order, uint64_t* edge_mem, int32_t V, const int64_t* indptr)
{
    for (int32_t i = threadIdx.x + blockDim.x * blockIdx.x; i < V; i += gridDim.x * blockDim.x) {
        int32_t id = order[i];
        edge_mem[i] = (uint64_t)(sizeof(int64_t) + sizeof(int32_t) * (indptr[id + 1] - indptr[id]));
    }
}
// PCM-free input of the cost model: 64-byte read transactions of the pre-sampling epoch's adjacency
// accesses, estimated from the edge hotness.  AT[t] = sampled edges of the rank-t row QT[t] (Kernels.cu:525: +1 per sampled
// edge).  Every sampled edge reads the row's 8-byte offset and one neighbour id (Kernels.cu:392-409); in 64-byte units a
// row of deg <= 14 ids has both in one line, a longer row needs a second one: weight = ceil((8 + 4 * min(deg, 16)) / 64),
// the "min(deg, .)" of the survey's formula taken at the 16 ids one transaction holds.  Integer only, deterministic.
__host__ __device__ inline uint64_t topo_transactions_of(uint64_t sampled_edges, int64_t deg)
{
    const int64_t ids = deg < 16 ? (deg < 0 ? 0 : deg) : 16;
    return sampled_edges * (uint64_t)((8 + 4 * ids + 63) / 64);
}
__global__ void k_topo_transactions(const int32_t* order, const uint64_t* hot, uint64_t* out, int32_t V, const int64_t* indptr)
{
    for (int32_t i = threadIdx.x + blockDim.x * blockIdx.x; i < V; i += gridDim.x * blockDim.x) {
        const int32_t id = order[i];
        out[i] = topo_transactions_of(hot[i], indptr[id + 1] - indptr[id]);
    }
}

// ------------------------------------------------------------------------------------------------
// host side: launch wrappers
// ------------------------------------------------------------------------------------------------
void launch_hotness(hipStream_t s, const int32_t* ids, const int32_t* nc, int32_t hops, unsigned long long* access,
                    int32_t* max_ids, int32_t bound)
{
    LEGION_AUDIT_LAUNCH(s, "k_hotness", LEGION_AW(access), LEGION_AW(max_ids), LEGION_AL(ids), LEGION_AL(nc));
    k_hotness<<<grid_for(bound, kBlock), kBlock, 0, s>>>(ids, nc, hops, access, max_ids);
    HIP_CHECK_LAST();
}
void launch_check_weights(hipStream_t s, const float* w, int64_t E, unsigned long long* bad)
{
    if (E <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_check_weights", LEGION_AW(bad), LEGION_AL(w));
    k_check_weights<<<grid_for(E, kBlock * 4), kBlock, 0, s>>>(w, E, bad);
    HIP_CHECK_LAST();
}
void launch_build_alias(hipStream_t s, const int64_t* indptr, const int32_t* indices, const float* w, int32_t V, int64_t E, double* p, AliasEntry* table)
{
    if (V <= 0 || E <= 0) return;
    // the CSR may be a peer's / the host's table; the weights' copy, the scratch and the table are this GPU's
    LEGION_AUDIT_LAUNCH(s, "k_build_alias", LEGION_AW(p), LEGION_AW(table), LEGION_AL(w), LEGION_AR(indptr), LEGION_AR(indices));
    k_build_alias<<<(V + kBlock - 1) / kBlock, kBlock, 0, s>>>(indptr, indices, w, V, E, p, table);
    HIP_CHECK_LAST();
    LEGION_AUDIT_LAUNCH(s, "k_build_alias_hub", LEGION_AW(p), LEGION_AW(table), LEGION_AL(w), LEGION_AR(indptr), LEGION_AR(indices));
    k_build_alias_hub<<<std::min((V + 63) / 64, sampler_cu_count() * 16), 64, 0, s>>>(indptr, indices, w, V, E, p, table);
    HIP_CHECK_LAST();
}

void launch_aggregate_access(hipStream_t s, unsigned long long* agg, const unsigned long long* add, int32_t n)
{
    LEGION_AUDIT_LAUNCH(s, "k_aggregate_access", LEGION_AW(agg), LEGION_AR(add));
    k_aggregate_access<<<grid_for(n, 256), 256, 0, s>>>(agg, add, n);
    HIP_CHECK_LAST();
}
void launch_iota(hipStream_t s, int32_t* out, int32_t n)
{
    LEGION_AUDIT_LAUNCH(s, "k_iota", LEGION_AW(out));
    k_iota<<<grid_for(n, 256), 256, 0, s>>>(out, n);
    HIP_CHECK_LAST();
}
void launch_fill_i32(hipStream_t s, int32_t* p, int32_t v, int64_t n)
{
    if (n <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_fill_i32", LEGION_AW(p));
    k_fill_i32<<<grid_for(n, 256), 256, 0, s>>>(p, v, n);
    HIP_CHECK_LAST();
}
void launch_fill_i8(hipStream_t s, int8_t* p, int8_t v, int64_t n)
{
    if (n <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_fill_i8", LEGION_AW(p));
    k_fill_i8<<<grid_for(n, 256), 256, 0, s>>>(p, v, n);
    HIP_CHECK_LAST();
}
void launch_build_feat_map(hipStream_t s, int32_t* feat_map, const int32_t* QF, int32_t capacity, int32_t Kg, int32_t V)
{
    launch_fill_i32(s, feat_map, -1, V);
    if (capacity <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_build_feat_map", LEGION_AW(feat_map), LEGION_AR(QF));
    k_build_feat_map<<<grid_for((int64_t)capacity * Kg, 256), 256, 0, s>>>(feat_map, QF, capacity, Kg, V);
    HIP_CHECK_LAST();
}
void launch_build_topo_map(hipStream_t s, int8_t* owner, int32_t* row, const int32_t* QT, int32_t capacity, int32_t Kg,
                           int32_t Ki, int32_t V)
{
    launch_fill_i8(s, owner, (int8_t)-1, V);
    launch_fill_i32(s, row, -1, V);
    if (capacity <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_build_topo_map", LEGION_AW(owner), LEGION_AW(row), LEGION_AR(QT));
    k_build_topo_map<<<grid_for((int64_t)capacity * Kg, 256), 256, 0, s>>>(owner, row, QT, capacity, Kg, Ki, V);
    HIP_CHECK_LAST();
}
void launch_feat_fill_up(hipStream_t s, int32_t row0, int32_t rows, int32_t F, int32_t chunk_pitch, int32_t table_pitch, float* chunk,
                         const float* table, const int32_t* QF, int32_t Kg, int32_t Ki, int32_t V)
{
    if (rows <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_feat_fill_up", LEGION_AW(chunk), LEGION_AR(table), LEGION_AR(QF));
    k_feat_fill_up<<<grid_for((int64_t)rows * F, 256), 256, 0, s>>>(row0, rows, F, chunk_pitch > 0 ? chunk_pitch : F, table_pitch > 0 ? table_pitch : F,
                                                                  chunk, table, QF, Kg, Ki, V);
    HIP_CHECK_LAST();
}
void launch_copy_rows_pitched(hipStream_t s, float* dst, int32_t dst_pitch, const float* src, int32_t src_pitch, int32_t F, int64_t rows)
{
    if (rows <= 0 || F <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_copy_rows_pitched", LEGION_AW(dst), LEGION_AR(src));
    k_copy_rows_pitched<<<grid_for(rows * F, 256), 256, 0, s>>>(dst, dst_pitch, src, src_pitch, F, rows);
    HIP_CHECK_LAST();
}
void launch_neighbor_count(hipStream_t s, const int32_t* QT, int32_t Kg, int32_t Ki, int32_t capacity, int32_t V,
                           const int64_t* indptr, int64_t* count_out)
{
    if (capacity <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_neighbor_count", LEGION_AW(count_out), LEGION_AR(QT), LEGION_AR(indptr));
    k_neighbor_count<<<grid_for(capacity, 256), 256, 0, s>>>(QT, Kg, Ki, capacity, V, indptr, count_out);
    HIP_CHECK_LAST();
}
void launch_topo_fill_up(hipStream_t s, const int32_t* QT, int32_t Kg, int32_t Ki, int32_t capacity, int32_t V,
                         const int64_t* indptr, const int32_t* indices, const int64_t* frag_indptr,
                         int32_t* const* frag_chunks, int32_t edge_shift)
{
    if (capacity <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_topo_fill_up", LEGION_AL(frag_indptr), LEGION_AL(frag_chunks), LEGION_AR(QT), LEGION_AR(indptr), LEGION_AR(indices));
    k_topo_fill_up<<<grid_for((int64_t)capacity * 64, 256), 256, 0, s>>>(QT, Kg, Ki, capacity, V, indptr, indices, frag_indptr, frag_chunks, edge_shift);
    HIP_CHECK_LAST();
}
void launch_chunk_ends(hipStream_t s, const int64_t* frag_indptr, int32_t capacity, int32_t edge_shift, int32_t nch, int64_t* ends)
{
    if (nch <= 1) return;
    LEGION_AUDIT_LAUNCH(s, "k_chunk_ends", LEGION_AW(ends), LEGION_AL(frag_indptr));
    k_chunk_ends<<<(nch + 63) / 64, 64, 0, s>>>(frag_indptr, capacity, edge_shift, nch, ends);
    HIP_CHECK_LAST();
}
void launch_edge_mem(hipStream_t s, const int32_t* order, uint64_t* edge_mem, int32_t V, const int64_t* indptr)
{
    LEGION_AUDIT_LAUNCH(s, "k_edge_mem", LEGION_AW(edge_mem), LEGION_AR(order), LEGION_AR(indptr));
    k_edge_mem<<<grid_for(V, 256), 256, 0, s>>>(order, edge_mem, V, indptr);
    HIP_CHECK_LAST();
}
void launch_topo_transactions(hipStream_t s, const int32_t* order, const uint64_t* hot, uint64_t* out, int32_t V, const int64_t* indptr)
{
    LEGION_AUDIT_LAUNCH(s, "k_topo_transactions", LEGION_AW(out), LEGION_AR(order), LEGION_AR(hot), LEGION_AR(indptr));
    k_topo_transactions<<<grid_for(V, 256), 256, 0, s>>>(order, hot, out, V, indptr);
    HIP_CHECK_LAST();
}

} // namespace legion
