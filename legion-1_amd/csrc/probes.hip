// probes.hip -- test probes: each evaluates one rule of the hot path for arbitrary inputs, through the very device functions its
// production kernel calls (draws.h, internal.h).  Nothing here runs in a batch.
#include "internal.h"
#include "draws.h"

#include "audit_hooks.h"

namespace legion {

__global__ void k_rng_probe(const int32_t* idx, const int32_t* deg, int32_t* k, int32_t n)
{
    int32_t i = threadIdx.x + blockDim.x * blockIdx.x;
    if (i < n) k[i] = sample_index(powmod31(kA, (uint64_t)idx[i] + 1ull), deg[i]);
}

// seeded stream: x = s_b * 48271^(idx + 1), as k_sample forms it (base times the slot's power)
__global__ void k_seeded_rng_probe(uint32_t w, const int32_t* idx, const int32_t* deg, int32_t* k, int32_t n)
{
    int32_t i = threadIdx.x + blockDim.x * blockIdx.x;
    if (i < n) k[i] = sample_index(mulmod31(seeded_stream_seed(w), powmod31(kA, (uint64_t)idx[i] + 1ull)), deg[i]);
}
__global__ void k_perm_probe(uint32_t ks, int32_t n, int32_t* out)
{
    const int32_t g = threadIdx.x + blockDim.x * blockIdx.x;
    if (g < n) out[g] = (int32_t)seeded_perm((uint32_t)g, (uint32_t)n, ks);
}

// drawn link-prediction thirds: position of the positive in a row of degree deg[i] (-1: deg <= 0, the source itself) and the negative of
// slot i with source src[i], by the device functions k_seed<.., LP> runs
__global__ void k_lp_draw_probe(uint32_t w, const int32_t* src, const int32_t* deg, int32_t V, int32_t* rho, int32_t* neg, int32_t n)
{
    const int32_t i = threadIdx.x + blockDim.x * blockIdx.x;
    if (i >= n) return;
    rho[i] = deg[i] > 0 ? lp_rho(w, (uint32_t)i, src[i], deg[i]) : -1;
    neg[i] = lp_neg(w, (uint32_t)i, src[i], V);
}

// The distinct mode's positions of n rows, by the device functions k_sample<.., DrawRule::Distinct> runs: pos[m * f + j] = neighbour position of slot j
// of row row[m] of hop hop[m] at degree deg[m], -1 = no draw.  One thread per row; the row's f words of pos are its work space.  w: the
// batch's draw word (legion_seeded_distinct_probe), 0 = the seeded mode off.
__global__ void k_distinct_probe(uint32_t w, const int32_t* row, const int32_t* hop, const int32_t* deg, int32_t f, int32_t* pos, int32_t n)
{
    const int32_t m = threadIdx.x + blockDim.x * blockIdx.x;
    if (m >= n) return;
    int32_t* out = pos + (int64_t)m * f;
    const int32_t d = deg[m];
    if (d <= f) {
        for (int32_t j = 0; j < f; j++) out[j] = j < d ? j : -1;
        return;
    }
    const uint32_t key = distinct_key((uint32_t)row[m], (uint32_t)hop[m], w);
    for (int32_t t = 0; t < f; t++) out[t] = (int32_t)distinct_u(key, (uint32_t)t);
    distinct_resolve(out, d, f);
}

// The weighted mode's draw of n slots, by the device functions k_sample<.., DrawRule::Weighted> runs: the column k[m] < deg[m] and the word ub[m] that
// is held against the column's threshold; deg[m] <= 0: k = -1, ub = 0.
__global__ void k_weighted_probe(const int32_t* row, const int32_t* hop, const int32_t* slot, const int32_t* deg, const uint32_t* word,
                                 int32_t* k, uint32_t* ub, int32_t n)
{
    const int32_t m = threadIdx.x + blockDim.x * blockIdx.x;
    if (m >= n) return;
    const int32_t d = deg[m];
    if (d <= 0) { k[m] = -1; ub[m] = 0u; return; }
    const uint32_t key = weighted_key((uint32_t)row[m], (uint32_t)hop[m], word[m]);
    k[m] = (int32_t)weighted_column(key, (uint32_t)slot[m], d);
    ub[m] = weighted_ub(key, (uint32_t)slot[m]);
}

// Weighted sampling without replacement: the hash and the fp64 key of n columns, by the device functions k_sample<.., DrawRule::WeightedDistinct> runs
__global__ void k_weighted_distinct_probe(const int32_t* row, const int32_t* hop, const int32_t* col, const uint32_t* word, const float* w,
                                          uint32_t* u, double* key, int32_t n)
{
    const int32_t m = threadIdx.x + blockDim.x * blockIdx.x;
    if (m >= n) return;
    const uint32_t uc = weighted_distinct_u(weighted_distinct_key((uint32_t)row[m], (uint32_t)hop[m], word[m]), (uint32_t)col[m]);
    u[m] = uc;
    key[m] = weighted_distinct_keyval(uc, w[m]);
}

// Shared-key sampling: the node key of n neighbour ids, by the device functions k_sample<.., DrawRule::Shared> forms it with
__global__ void k_shared_draw_probe(const int32_t* ids, const uint32_t* word, uint32_t* key, int32_t n)
{
    const int32_t m = threadIdx.x + blockDim.x * blockIdx.x;
    if (m < n) key[m] = shared_key(ids[m], shared_salt(word[m]));
}

// Weighted shared-key sampling: the node hash and the fp64 key of n (neighbour id, weight) pairs, by the device functions k_sample<.., DrawRule::WeightedShared> runs
__global__ void k_weighted_shared_probe(const int32_t* ids, const uint32_t* word, const float* w, uint32_t* u, double* key, int32_t n)
{
    const int32_t m = threadIdx.x + blockDim.x * blockIdx.x;
    if (m >= n) return;
    const uint32_t uc = weighted_shared_u(ids[m], weighted_shared_salt(word[m]));
    u[m] = uc;
    key[m] = weighted_distinct_keyval(uc, w[m]);
}

void launch_weighted_shared_probe(hipStream_t s, const int32_t* ids, const uint32_t* word, const float* w, uint32_t* u, double* key, int32_t n)
{
    if (n <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_weighted_shared_probe", LEGION_AW(u), LEGION_AW(key), LEGION_AL(ids), LEGION_AL(word), LEGION_AL(w));
    k_weighted_shared_probe<<<(n + 255) / 256, 256, 0, s>>>(ids, word, w, u, key, n);
    HIP_CHECK_LAST();
}
void launch_shared_draw_probe(hipStream_t s, const int32_t* ids, const uint32_t* word, uint32_t* key, int32_t n)
{
    if (n <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_shared_draw_probe", LEGION_AW(key), LEGION_AL(ids), LEGION_AL(word));
    k_shared_draw_probe<<<(n + 255) / 256, 256, 0, s>>>(ids, word, key, n);
    HIP_CHECK_LAST();
}
void launch_weighted_distinct_probe(hipStream_t s, const int32_t* row, const int32_t* hop, const int32_t* col, const uint32_t* word, const float* w,
                                    uint32_t* u, double* key, int32_t n)
{
    if (n <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_weighted_distinct_probe", LEGION_AW(u), LEGION_AW(key), LEGION_AL(row), LEGION_AL(hop), LEGION_AL(col), LEGION_AL(word), LEGION_AL(w));
    k_weighted_distinct_probe<<<(n + 255) / 256, 256, 0, s>>>(row, hop, col, word, w, u, key, n);
    HIP_CHECK_LAST();
}
void launch_seeded_distinct_probe(hipStream_t s, uint32_t w, const int32_t* row, const int32_t* hop, const int32_t* deg, int32_t f, int32_t* pos, int32_t n)
{
    if (n <= 0) return;
    if (f < 1 || f > kDistinctMaxFanout) { LEGION_ARG_ERROR("legion_distinct_probe: distinct sampling takes a fan-out of 1 to 64"); return; }
    LEGION_AUDIT_LAUNCH(s, "k_distinct_probe", LEGION_AW(pos), LEGION_AL(row), LEGION_AL(hop), LEGION_AL(deg));
    k_distinct_probe<<<(n + 255) / 256, 256, 0, s>>>(w, row, hop, deg, f, pos, n);
    HIP_CHECK_LAST();
}
void launch_distinct_probe(hipStream_t s, const int32_t* row, const int32_t* hop, const int32_t* deg, int32_t f, int32_t* pos, int32_t n)
{
    launch_seeded_distinct_probe(s, 0u, row, hop, deg, f, pos, n);
}
void launch_weighted_probe(hipStream_t s, const int32_t* row, const int32_t* hop, const int32_t* slot, const int32_t* deg, const uint32_t* word,
                           int32_t* k, uint32_t* ub, int32_t n)
{
    if (n <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_weighted_probe", LEGION_AW(k), LEGION_AW(ub), LEGION_AL(row), LEGION_AL(hop), LEGION_AL(slot), LEGION_AL(deg), LEGION_AL(word));
    k_weighted_probe<<<(n + 255) / 256, 256, 0, s>>>(row, hop, slot, deg, word, k, ub, n);
    HIP_CHECK_LAST();
}
void launch_seeded_rng_probe(hipStream_t s, uint32_t w, const int32_t* idx, const int32_t* deg, int32_t* k, int32_t n)
{
    if (n <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_seeded_rng_probe", LEGION_AW(k), LEGION_AL(idx), LEGION_AL(deg));
    k_seeded_rng_probe<<<(n + 255) / 256, 256, 0, s>>>(w, idx, deg, k, n);
    HIP_CHECK_LAST();
}
void launch_lp_draw_probe(hipStream_t s, uint32_t w, const int32_t* src, const int32_t* deg, int32_t V, int32_t* rho, int32_t* neg, int32_t n)
{
    if (n <= 0) return;
    if (V < 1) { LEGION_ARG_ERROR("legion_lp_draw_probe: V must be at least 1"); return; }
    LEGION_AUDIT_LAUNCH(s, "k_lp_draw_probe", LEGION_AW(rho), LEGION_AW(neg), LEGION_AL(src), LEGION_AL(deg));
    k_lp_draw_probe<<<(n + 255) / 256, 256, 0, s>>>(w, src, deg, V, rho, neg, n);
    HIP_CHECK_LAST();
}
void launch_perm_probe(hipStream_t s, uint32_t ks, int32_t n, int32_t* out)
{
    if (n <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_perm_probe", LEGION_AW(out));
    k_perm_probe<<<(n + 255) / 256, 256, 0, s>>>(ks, n, out);
    HIP_CHECK_LAST();
}
void launch_rng_probe(hipStream_t s, const int32_t* idx, const int32_t* deg, int32_t* k, int32_t n)
{
    if (n <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_rng_probe", LEGION_AW(k), LEGION_AL(idx), LEGION_AL(deg));
    k_rng_probe<<<(n + 255) / 256, 256, 0, s>>>(idx, deg, k, n);
    HIP_CHECK_LAST();
}

} // namespace legion
