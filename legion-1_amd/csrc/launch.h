// launch.h -- host-side helpers of the launch wrappers (.hip units): grid sizing and the two rules every gather-like launch shares.
#pragma once
#include "internal.h"

#include <algorithm>

namespace legion {

// Workgroups of a launch over work_items items, per_block per workgroup: at most blocks_per_cu per compute unit of the current device
// (sampler_cu_count: internal.h; one cached value per process, defined in sampler.hip).
static inline int grid_for(int64_t work_items, int per_block, int blocks_per_cu = 8)
{
    int64_t need = (work_items + per_block - 1) / per_block;
    int64_t cap = (int64_t)sampler_cu_count() * blocks_per_cu;
    if (need < 1) need = 1;
    return (int)(need < cap ? need : cap);
}

// Rows a launch is sized for.  The static bound is typically filled 15-60 %, so the grid comes from the row count an earlier launch of
// the same kind reported (GatherArgs::rows_seen -> rows_hint, no host round trip) + 25 % + 1024; without a report: the bound.  The kernels'
// grid-stride loops cover a batch that outgrows the estimate.  (Re-swept in round 2, profiles/r02_gather_grid_sweep.md: a 3-25 % margin
// lands within the run-to-run spread of 323-342 us at the papers100M shape.)
static inline int64_t est_rows(int32_t rows_hint, int64_t bound)
{
    return rows_hint > 0 ? std::min<int64_t>(bound, (int64_t)rows_hint + rows_hint / 4 + 1024) : bound;
}

// The 16-byte element path (v4f) of the row kernels: rows of F floats are 16-byte aligned when F % 4 == 0 and both ends are.  Cache chunks
// are hipMalloc'ed (256-byte aligned) and hold whole rows, so the two pointers a launch is given decide.
static inline bool rows_are_vec4(int32_t F, const void* p, const void* q)
{
    return (F % 4 == 0) && (((uintptr_t)p | (uintptr_t)q) % 16 == 0);
}

} // namespace legion
