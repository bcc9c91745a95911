// internal.h -- shared declarations of liblegion_amd (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/legion_amd.h"
#include "audit.h"

namespace legion {

// ---- error handling (reference: cudaCheckError(), Kernels.cuh:14-22) -------------------------
void report_error(const char* file, int line, const char* msg, bool hip_failure);
bool error_pending();
bool error_is_fatal();                                     // LEGION_ERR_EXIT mode (the reference's behaviour)
int64_t ipc_max_bytes();                                   // $LEGION_IPC_MAX_BYTES, see runtime.cpp
bool ipc_size_ok(int64_t bytes, const char* who);          // sticky error + false above the limit
bool ipc_export_ok(const void* ptr, const char* who);      // same, for the allocation `ptr` belongs to
int64_t shard_chunk_bytes();                               // $LEGION_SHARD_CHUNK_BYTES (default 1 GiB), read on every call
inline void check(hipError_t e, const char* file, int line)
{
    if (e != hipSuccess) report_error(file, line, hipGetErrorString(e), true);
}
#define HIP_CHECK(expr) ::legion::check((expr), __FILE__, __LINE__)
#define HIP_CHECK_LAST() ::legion::check(hipGetLastError(), __FILE__, __LINE__)
#define LEGION_ARG_ERROR(msg) ::legion::report_error(__FILE__, __LINE__, (msg), false)

// Where the library's progress prints go: stdout like the reference's (std::cout / printf all over Server.cu, GPUCache.cu,
// CUDA_IPC_Service.cu), or stderr under $LEGION_LOG=stderr (read once) -- for a host that owns stdout (bench.py's one JSON line).
std::ostream& log_out();
FILE* log_file();

int physical_device(int logical);
bool is_remote_device(int logical); // logical GPU driven by another process (one process per GPU)
// RAII: switch to a logical GPU (its physical device + the thread's logical current device), restore both on scope exit
struct DeviceGuard {
    int prev = -1, prev_logical = -1;
    explicit DeviceGuard(int logical);
    ~DeviceGuard();
};

// ---- cache shards and CSR fragments (chunks.cpp): lists of chunk allocations of <= shard_chunk_bytes(), each one HIP-IPC export
int chunk_shift(int64_t unit_bytes, int min_shift);        // largest s <= 30 (>= min_shift) with (1 << s) * unit_bytes <= chunk bytes
inline int chunk_count(int64_t n, int shift) { return n > 0 ? (int)(((n - 1) >> shift) + 1) : 1; }   // chunks of 2^shift for n elements
template <typename T>
struct ChunkList {
    std::vector<T*> chunks;
    bool imported = false;                                 // opened from another process' IPC handles (closed, not freed)
    T* at(int q) const { return q >= 0 && q < (int)chunks.size() ? chunks[q] : nullptr; }
    bool complete(size_t n) const { for (T* p : chunks) if (!p) return false; return chunks.size() == n; }
    void release();                                        // free / close every chunk: an empty local list again
    int export_chunk(int dev, int q, void* handle64, const char* who) const;   // 0, or -1 with a sticky error naming `who`
    // open the handle under logical GPU open_dev as chunk q, once the exporter's allocation (>= floor_bytes) passed the IPC limit
    int import_chunk(int q, const void* handle64, int64_t floor_bytes, int open_dev, const char* who);
};
// on `viewer`: audit h, then copy it into `tab` (allocated when null; freed first, after a device sync, when `realloc`; empty h: freed)
template <typename T> void upload_table(int viewer, const std::vector<T*>& h, T**& tab, bool realloc, const char* what);

// ---- what the three storages share (chunks.cpp; the frees that go with it: device_mem.h); hidden: the library exports what it exported ----
// all-pairs peer access between the physical devices behind the logical GPUs (GPUGraphStore::EnableP2PAccess, GPUGraphStore.cu:145-168)
__attribute__((visibility("hidden"))) void enable_p2p(int32_t partition_count);
// a table the caller handed over: pageable host memory is copied into pinned memory of our own (*owns := true), anything else is used in place
template <typename T> T* adopt_table(const T* src, int64_t count, int32_t location, bool* owns);
// "One copy per physical device, shared by its logical GPUs", stated once: leader[p] of the logical GPUs 0..P-1 is the first LOCAL q <= p
// with physical_device(q) == physical_device(p), -1 for a p another process drives.  The leader (leader[p] == p) builds the copy under
// its DeviceGuard, the others take array[leader[p]] and record LEGION_AUDIT_SHARE; free_replicas (device_mem.h) is the one free of such
// an array and goes by pointer identity -- the two belong together.  Host code only, no device is touched.
__attribute__((visibility("hidden"))) std::vector<int> device_leaders(int P);
// replica[p] := an HBM copy of `rows` rows of `width` elements of src (src_pitch elements apart) at dst_pitch, for every local logical GPU
// that holds none, by the rule above.  Equal pitches: one plain copy of rows * dst_pitch elements (a whole CSR array is one such row);
// otherwise the copy is zeroed and filled row by row.
template <typename T>
void replicate_table(const T* src, int64_t rows, int64_t width, int64_t src_pitch, int64_t dst_pitch, std::vector<T*>& replica);

// ---- constants --------------------------------------------------------------------------------
// Position-table entry: (epoch << kPosShift) | value.  epoch = kEpochTop - batch serial: entries of older batches compare GREATER than
// anything of the running batch (stale without being touched); value = kProvisional | slot idx while claimed in the running hop, else
// the node's final index in sampled_ids.  u64 entries, 32-bit epoch (never wraps in practice).  (A u32 entry -- 7-bit epoch, flag, 24-bit
// value, wiped every 126 batches -- was bit-identical and lost at two of three shapes: profiles/r05_sampler.md, r06_removed_experiments.patch.)
typedef unsigned long long pos_t;
constexpr int kPosShift = 32;
constexpr uint32_t kProvisional = 0x80000000u, kPosValueMask = 0x7FFFFFFFu;
constexpr uint32_t kEpochTop = 0xFFFFFFFFu, kSerialLimit = 0xFFFFFFF0u;
__host__ __device__ inline pos_t pos_entry(uint32_t epoch, uint32_t value) { return ((pos_t)epoch << kPosShift) | (pos_t)value; }
#ifndef LEGION_KTILE
#define LEGION_KTILE 1024
#endif
constexpr int kTile = LEGION_KTILE;            // sampler slots per workgroup tile (hops that fill the chip)
constexpr int kBlock = 256;                    // threads per workgroup
static_assert(kTile >= kBlock && kTile <= 2048 && (kTile & (kTile - 1)) == 0, "LEGION_KTILE: a power of two in [256, 2048] (k_sample stages 16 bytes of row descriptor per slot in static LDS)");
// A hop whose static slot bound (seeds x fan-outs so far) is at most kNarrowSlots does not fill the chip with kTile-slot tiles (hop 1 of the
// headline: 196 tiles on 256 CUs, each thread walking kTile / kBlock slots one after the other): its three passes run the kTileNarrow
// instantiation, one slot per thread.  The tile is a template parameter of k_sample / k_mark / k_write and the same in all three passes of a
// hop (launch_sample_hop picks it once); the RNG stream and every rank are indexed by slot, so results do not depend on it.  The per-tile
// scratch (tile_edge / tile_node / tile_pre) is sized for the larger of the two tile counts (sampler_max_tiles).
#ifndef LEGION_NARROW_SLOTS
#define LEGION_NARROW_SLOTS (256 * 1024)
#endif
constexpr int kTileNarrow = kBlock;
constexpr int64_t kNarrowSlots = LEGION_NARROW_SLOTS;
static_assert(kTileNarrow <= kTile, "one pow_tab of kTile entries serves both tile sizes");
constexpr int64_t sampler_tile_of(int64_t slots_bound) { return slots_bound <= kNarrowSlots ? kTileNarrow : kTile; }
// tiles of the largest hop a pool sized for `max_slots` slots can run, whichever tile size each of its hops selects
constexpr int64_t sampler_max_tiles(int64_t max_slots)
{
    const int64_t wide = (max_slots + kTile - 1) / kTile, narrow_slots = max_slots < kNarrowSlots ? max_slots : kNarrowSlots;
    const int64_t narrow = (narrow_slots + kTileNarrow - 1) / kTileNarrow;
    return wide > narrow ? wide : narrow;
}
// The rules without replacement: the largest fan-out k_sample runs under a rule that stages picks (its LDS holds the picks of a tile's rows, TILE + 2 of these)
constexpr int kDistinctMaxFanout = 64;
// The sampling kinds of ServeModes::sampling, the `sampling` word a trainer reads and GPUMemoryPool_SetSampling
constexpr int32_t kSamplingReplace = 0, kSamplingDistinct = 1, kSamplingWeighted = 2;
// Weighted sampler mode: one entry per CSR entry, beside indices[e] (INTEGRATION.md "Weighted sampling").  Column k of a row is drawn with
// probability 1 / degree; the draw keeps the column's own neighbour with probability thr / 2^32 and takes alias_id, the ID of another
// neighbour of the row, otherwise.  Every entry of a row whose weights are all zero is {0, -1}: no edge.
struct AliasEntry { uint32_t thr; int32_t alias_id; };
static_assert(sizeof(AliasEntry) == 8, "one 8-byte probe per weighted draw");
// rows of more neighbours than this are built by a whole wave (k_build_alias_hub), the others by one lane each (k_build_alias)
constexpr int32_t kAliasHubDegree = 256;
// k_mark runs one CONTIGUOUS chunk of tiles per workgroup and leaves the chunk totals in GPUMemoryPool::chunk_tot; k_write scans them in
// LDS, kMaxChunks / kBlock per thread.  One constant for the allocation (memory_pool.cpp), the grid clamp (launch_sample_hop) and the LDS
// array (k_write): changing one of them alone would let k_mark write past the allocation.
constexpr int kMaxChunks = 2048;
static_assert(kMaxChunks % kBlock == 0 && kMaxChunks >= 256 * 8, "kMaxChunks: a multiple of the workgroup size, >= 256 CUs x 8 workgroups");
constexpr int ilog2_c(int v) { return v <= 1 ? 0 : 1 + ilog2_c(v >> 1); }
constexpr int kMaxParts = LEGION_MAX_DEVICE;

// The serving modes as ONE value: what the environment asks for, what a Runner serves, what a pool is in (GPUMemoryPool::modes), what a
// batch graph was recorded in and what the "<name>_ext" object tells a trainer.  DESIGN.md "Where a serving mode lives" lists every place.
struct ServeModes {
    bool agg_last_hop = false;   // $LEGION_AGG_LAST_HOP=1: the last hop is handed over as neighbour sums (INTEGRATION.md "Aggregated last hop")
    int32_t agg_norm = 0;        // $LEGION_AGG_NORM=both, only with agg_last_hop: 1 = the sums weighted by out-degree^-1/2 inside block 1 ("Normalised sums")
    int32_t sampling = 0;        // $LEGION_SAMPLING: 0 = replace (the reference's stream), 1 = distinct: min(degree, fan-out) distinct neighbours per row,
                                 // 2 = weighted: with replacement, in proportion to the graph's edge weights (GPUGraphStorage_SetEdgeWeights)
    bool seeded = false;         // $LEGION_SAMPLING_SEED: every batch draws from its own word W(seed, round, counter), the training list is reshuffled
    uint32_t seed = 0;           // ... every round ("Seeded sampling").  Seed 0 is a seed like any other: `seeded` says whether there is one
    int32_t lp_draw = 0;         // $LEGION_LP_DRAW=1, only under a seed: k > 0 = a training batch is 3 k seeds whose pos and neg thirds are drawn per batch
                                 // ("Drawn link-prediction thirds"); from the environment it is 1 until serve_modes_resolve_lp_draw puts k there
    bool weighted_distinct = false;   // $LEGION_WEIGHTED_DISTINCT=1, only with sampling = weighted: the weighted draws are WITHOUT replacement, min(eligible
                                 // columns, fan-out) distinct columns per row by exponential keys over the graph's retained edge weights ("Weighted sampling
                                 // without replacement").  A flag on top of the kind: remembered across kinds, acts only while sampling == 2
    bool shared_draws = false;   // $LEGION_SHARED_DRAWS=1, only with sampling = distinct (and, from the environment, only under a seed): the random number belongs
                                 // to the NEIGHBOUR NODE, not to the row -- every row keeps its min(degree, fan-out) columns of smallest node key, so rows that see
                                 // the same neighbours pick the same ones ("Shared-key sampling").  A flag on top of the kind, like weighted_distinct: remembered
                                 // across kinds, acts while sampling == 1 and, with weighted_distinct on, while sampling == 2: there the exponential key's uniform
                                 // belongs to the neighbour node ("Weighted shared-key sampling")
    bool edge_ids = false;       // $LEGION_EDGE_IDS=1 / GPUMemoryPool_SetEdgeIds: every sampled edge's position in the whole CSR, and its weight where the graph
                                 // retains them, beside the pipe's COO ("Edge ids").  Refused together with the alias rule (sampling == 2 without
                                 // weighted_distinct); pre-sampling batches hand nothing over
    bool edge_weights = false;   // $LEGION_EDGE_WEIGHTS=1, only with edge_ids: the SERVER loads the graph's weights and retains them whatever the sampling
                                 // kind, so edge_w is filled.  Nothing of the pool's: it fills edge_w wherever the graph retains weights (serve_modes_edge_w_filled)
    bool agg_edge_weight = false;   // $LEGION_AGG_EDGE_WEIGHT=1 / GPUMemoryPool_SetAggEdgeWeight, only with agg_last_hop and edge_ids and
                                 // without agg_norm: the sums scale every row by its draw's edge weight, edge_w of the edge-id mode ("Edge-weighted sums").  A flag
                                 // on top of the aggregated mode: remembered while that mode is off, as the norm is
    int32_t edge_feat_dim = 0;   // GPUMemoryPool_SetEdgeFeatures, only with edge_ids: 0 = off, dim > 0 = get_edge_feature_kernel gathers edge_feat[e, :] = X[edge_ids[e], :]
                                 // from the graph's float32 [E, dim] table (GPUGraphStorage_SetEdgeFeatures) into a per-pipe buffer ("Edge features").  No variable,
                                 // no mode word: the pool's and the Engine's only (open: the served hand-off)
    int32_t lp_exclude = 0;      // GPUMemoryPool_SetLpExclude: 0 = off, k > 0 = a training batch of 3 k seeds has its target pairs {ids[i], ids[k + i]} looked up among
                                 // the batch's COO edges: edge_keep[e] = 0 where edge e joins a target pair, either direction ("Target-edge exclusion").  The edges are
                                 // marked, not removed.  Refused together with agg_last_hop and, at another k, with lp_draw.  No variable, no mode word: the pool's and
                                 // the Engine's only (open: the served hand-off)
    bool operator==(const ServeModes& o) const { return lp_exclude == o.lp_exclude && edge_feat_dim == o.edge_feat_dim && edge_weights == o.edge_weights && agg_last_hop == o.agg_last_hop && agg_norm == o.agg_norm && sampling == o.sampling && seeded == o.seeded && seed == o.seed && lp_draw == o.lp_draw && weighted_distinct == o.weighted_distinct && shared_draws == o.shared_draws && edge_ids == o.edge_ids && agg_edge_weight == o.agg_edge_weight; }
};
// The draw rule of a sampler hop: what `sampling` and the flags `weighted_distinct` and `shared_draws` say together.  draw_rule_of is the one
// place that reads the three; the launchers, the fan-out checks and the k_sample dispatch go by the rule and its facts below.
enum class DrawRule { Stream, Distinct, Weighted, WeightedDistinct, Shared, WeightedShared };
inline DrawRule draw_rule_of(const ServeModes& m)
{
    // shared_draws acts under the weighted kind only on top of weighted_distinct ("Weighted shared-key sampling"): without it the flag is remembered, not read
    if (m.sampling == kSamplingWeighted) return !m.weighted_distinct ? DrawRule::Weighted : m.shared_draws ? DrawRule::WeightedShared : DrawRule::WeightedDistinct;
    if (m.sampling == kSamplingDistinct) return m.shared_draws ? DrawRule::Shared : DrawRule::Distinct;
    return DrawRule::Stream;
}
// What is true of a rule, once, one row per rule in the enumeration's order (the assertion behind it holds the two together).  The kernel's branches,
// the launchers' refusals, the fan-out checks and the log line read this table and nothing else; a new rule is a new row.
//   whole_csr:     the rule's table (alias table, retained weights) lies beside the whole CSR's indices: never the fragments, exactly as pre-sampling
//   reads_weights: the rule reads the graph's retained edge weights, not the alias table
//   max_fanout:    the largest fan-out the rule runs, 0 = no bound; a rule has one because k_sample stages a row's picks in static LDS (s_pick): stages_picks()
//   picks_column:  what the rule picks is a column of the row (the alias rule may take the column's ALIAS neighbour, whose column nobody knows)
//   fanout_refusal / env_head, env_tail / sentence: the rule's name to a person, as launch_sample_hop refuses a fan-out above the bound, as
//                  serve_modes_fit_fanout puts its refusal together, and as Runner_Initialize logs what it serves (null where there is no bound)
struct DrawRuleFacts {
    DrawRule rule; bool whole_csr, reads_weights; int32_t max_fanout; bool picks_column; const char *fanout_refusal, *env_head, *env_tail, *sentence;
    constexpr bool stages_picks() const { return max_fanout != 0; }
};
constexpr DrawRuleFacts kDrawRuleFacts[] = {
    {DrawRule::Stream, false, false, 0, true, nullptr, nullptr, nullptr, "with replacement (LEGION_SAMPLING=replace)"},
    {DrawRule::Distinct, false, false, kDistinctMaxFanout, true, "GPU_Random_Sampling: distinct sampling (GPUMemoryPool_SetSampleDistinct) takes a fan-out of at most 64: k_sample stages the picks of a tile's rows in static LDS", "LEGION_SAMPLING=distinct", ": k_sample stages the picks of a tile's rows in static LDS", "distinct neighbours, min(degree, fan-out) per row (LEGION_SAMPLING=distinct)"},
    {DrawRule::Weighted, true, false, 0, false, nullptr, nullptr, nullptr, "weighted by edge weight, with replacement, from the graph's alias table (LEGION_SAMPLING=weighted)"},
    {DrawRule::WeightedDistinct, true, true, kDistinctMaxFanout, true, "GPU_Random_Sampling: weighted sampling without replacement (GPUMemoryPool_SetWeightedDistinct) takes a fan-out of at most 64: k_sample keeps a row's best picks one per lane and stages them in static LDS", "LEGION_WEIGHTED_DISTINCT=1", ": k_sample keeps a row's best picks one per lane and stages them in static LDS", "weighted by edge weight, without replacement: min(columns of weight > 0, fan-out) distinct columns per row, from the graph's retained weights (LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1)"},
    {DrawRule::Shared, false, false, kDistinctMaxFanout, true, "GPU_Random_Sampling: shared-key sampling (GPUMemoryPool_SetSharedDraws) takes a fan-out of at most 64: k_sample keeps a row's best picks one per lane and stages them in static LDS", "LEGION_SHARED_DRAWS=1", ": k_sample keeps a row's best picks one per lane and stages them in static LDS", "distinct neighbours, min(degree, fan-out) per row, by a key of the neighbour node: rows that see the same neighbours pick the same ones (LEGION_SAMPLING=distinct LEGION_SHARED_DRAWS=1)"},
    {DrawRule::WeightedShared, true, true, kDistinctMaxFanout, true, "GPU_Random_Sampling: weighted shared-key sampling (GPUMemoryPool_SetWeightedDistinct + GPUMemoryPool_SetSharedDraws) takes a fan-out of at most 64: k_sample keeps a row's best picks one per lane and stages them in static LDS", "LEGION_WEIGHTED_DISTINCT=1 LEGION_SHARED_DRAWS=1", ": k_sample keeps a row's best picks one per lane and stages them in static LDS", "weighted by edge weight, without replacement, by a key of the neighbour node: min(columns of weight > 0, fan-out) distinct columns per row, rows that see the same neighbours prefer the same ones (LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1 LEGION_SHARED_DRAWS=1)"}};
constexpr int kDrawRules = sizeof(kDrawRuleFacts) / sizeof(kDrawRuleFacts[0]);
constexpr const DrawRuleFacts& draw_rule_facts(DrawRule r) { return kDrawRuleFacts[(int)r]; }
static_assert([] { for (int i = 0; i < kDrawRules; i++) if ((int)kDrawRuleFacts[i].rule != i) return false; return true; }(), "kDrawRuleFacts: row i states rule i");
// Where k_sample reads a row: the whole CSR, the whole CSR while counting topology hotness (a pre-sampling hop), or the owner's fragment
// where the topology map names one.  launch_sample_hop derives it from (is_presc, the tables it was given).
enum class RowSource { Whole, Presc, Fragments }; constexpr int kRowSources = 3;
// Which k_sample<TILE, SRC, RULE, COLS> there are, for the kernel's assertion, the dispatch table built from it (sampler.hip) and every host
// check: no columns (GPUMemoryPool_SetEdgeIds) from a pre-sampling hop, which hands nothing over; none under a rule whose pick is not a
// column; no fragments under a rule whose table lies beside the whole CSR.
constexpr bool sample_variant_exists(RowSource s, DrawRule r, bool cols) { return !(cols && (s == RowSource::Presc || !draw_rule_facts(r).picks_column)) && !(s == RowSource::Fragments && draw_rule_facts(r).whole_csr); }
// whether a server of these modes retains the graph's edge weights (load_edge_weights(s, retain), server.cpp), and whether it serves edge_w filled
inline bool serve_modes_retain_weights(const ServeModes& m) { return m.edge_weights || (m.sampling == kSamplingWeighted && m.weighted_distinct); }
inline bool serve_modes_edge_w_filled(const ServeModes& m) { return m.edge_ids && serve_modes_retain_weights(m); }
// The only readers of the ten variables.  False with the refusal in `why` (the caller puts its name in front); tested in this order:
// unknown norm, norm without the aggregated mode, unknown sampling mode, malformed seed, unknown LEGION_LP_DRAW, LEGION_LP_DRAW without a
// seed, unknown LEGION_WEIGHTED_DISTINCT, LEGION_WEIGHTED_DISTINCT without LEGION_SAMPLING=weighted, unknown LEGION_SHARED_DRAWS,
// LEGION_SHARED_DRAWS without LEGION_SAMPLING=distinct (or =weighted with LEGION_WEIGHTED_DISTINCT=1), LEGION_SHARED_DRAWS without a seed; then unknown
// LEGION_EDGE_IDS, LEGION_EDGE_IDS under the alias rule, unknown LEGION_EDGE_WEIGHTS, LEGION_EDGE_WEIGHTS without LEGION_EDGE_IDS, unknown LEGION_AGG_EDGE_WEIGHT, and
// LEGION_AGG_EDGE_WEIGHT with every condition it misses named in one refusal.  Host code only, no device is touched.
bool serve_modes_from_env(ServeModes& m, std::string& why);
// LEGION_LP_DRAW against what is served, once the meta line is known: false with the refusal in `why` unless the training lists are
// link-prediction thirds (meta flag 2) of a batch size divisible by 3; m.lp_draw := raw_batch_size / 3.  Nothing to do with the mode off.
bool serve_modes_resolve_lp_draw(ServeModes& m, bool lp_lists, int32_t raw_batch_size, std::string& why);
// the fan-out bound of the modes' draw rule (DrawRuleFacts::max_fanout) against a fan-out list: false with the refusal in `why`
bool serve_modes_fit_fanout(const ServeModes& m, const int32_t* fanout, int32_t hops, std::string& why);
void runner_set_lists_verbatim(Runner* r, bool verbatim);   // before Runner_Initialize: meta flag 2 (Runner::lists_verbatim, runner.cpp)
// what a trainer reads: the five mode words of the "<name>_ext" object and the six of "<name>_ext2" (shmExt, shmExt2, ipc_shm.h) := m (ipc_env.cpp; the
// IPCEnv_Set* calls write one mode each).  The second object appears only when one of its words is on.
void ipc_env_publish_modes(IPCEnv* e, const ServeModes& m);

// The seed sets are indexed by mode everywhere (LEGION_TRAINMODE, LEGION_VALIDMODE, LEGION_TESTMODE); LegionBuildInfo names their fields
// one by one, this table gives them the same index.
constexpr int kModes = 3;
static_assert(LEGION_TRAINMODE == 0 && LEGION_VALIDMODE == 1 && LEGION_TESTMODE == 2, "seed sets are indexed by mode");
struct BuildInfoSeedFields {
    const int32_t* LegionBuildInfo::*num;
    const int32_t* const* LegionBuildInfo::*ids;
    const int32_t* const* LegionBuildInfo::*labels;
};
constexpr BuildInfoSeedFields kBuildInfoSeeds[kModes] = {
    {&LegionBuildInfo::training_set_num, &LegionBuildInfo::training_set_ids, &LegionBuildInfo::training_labels},
    {&LegionBuildInfo::validation_set_num, &LegionBuildInfo::validation_set_ids, &LegionBuildInfo::validation_labels},
    {&LegionBuildInfo::testing_set_num, &LegionBuildInfo::testing_set_ids, &LegionBuildInfo::testing_labels}};

// minstd_rand arithmetic (thrust::minstd_rand: x <- 48271 x mod 2^31-1), shared by the sampler and the generators
constexpr uint32_t kP31 = 2147483647u; // minstd modulus 2^31 - 1
constexpr uint32_t kA = 48271u;        // minstd multiplier

__host__ __device__ inline uint32_t mulmod31(uint32_t a, uint32_t b)
{
    uint64_t p = (uint64_t)a * (uint64_t)b;
    uint32_t r = (uint32_t)(p & kP31) + (uint32_t)(p >> 31); // < 2^32
    r = (r & kP31) + (r >> 31);
    return r >= kP31 ? r - kP31 : r;
}

__host__ __device__ inline uint32_t powmod31(uint32_t base, uint64_t e)
{
    uint32_t r = 1;
    while (e) {
        if (e & 1) r = mulmod31(r, base);
        base = mulmod31(base, base);
        e >>= 1;
    }
    return r;
}

// Seeded sampling (INTEGRATION.md "Seeded sampling"): the keys of a round and the draw word of a batch.  mix32 is the distinct mode's hash.
__host__ __device__ inline uint32_t mix32(uint32_t z)
{
    z ^= z >> 16; z *= 0x7feb352du; z ^= z >> 15; z *= 0x846ca68bu; z ^= z >> 16;
    return z;
}
constexpr uint32_t kShuffleTag = 0x53485546u, kDrawTag = 0x44524157u, kGolden = 0x9E3779B9u;
constexpr uint32_t kLpPosTag = 0x4C50504Fu, kLpNegTag = 0x4C504E45u;   // drawn link-prediction thirds: Kp = mix32(W ^ "LPPO"), Kn = mix32(W ^ "LPNE")
__host__ __device__ inline uint32_t seeded_shuffle_key(uint32_t seed, uint32_t round) { return mix32(mix32(seed ^ kShuffleTag) ^ round); }
__host__ __device__ inline uint32_t seeded_draw_key(uint32_t seed, uint32_t round) { return mix32(mix32(seed ^ kDrawTag) ^ round); }
__host__ __device__ inline uint32_t seeded_draw_word(uint32_t seeded, uint32_t draw_key, int32_t counter) { return seeded ? mix32(draw_key ^ (uint32_t)counter) : 0u; }
// the minstd seed of a batch: thrust::minstd_rand(s_b); 1 (the default-constructed engine, today's stream) for W = 0
__host__ __device__ inline uint32_t seeded_stream_seed(uint32_t w) { return 1u + w % 2147483646u; }
// The round's permutation of [0, n): a four-round Feistel network on b = bit_length(n - 1) rounded up to even bits, cycle-walked into
// [0, n) (the domain has fewer than 4 n points).  Only k_shuffle_seeds and the probe run it: once per epoch, never per batch.
__host__ __device__ inline uint32_t seeded_perm(uint32_t g, uint32_t n, uint32_t ks)
{
    if (n <= 1) return g;
    uint32_t b = 0;
    while (b < 32 && ((n - 1) >> b)) b++;
    const uint32_t h = (b + 1) >> 1, m = (1u << h) - 1u;
    uint32_t rk[4];
    for (uint32_t q = 0; q < 4; q++) rk[q] = mix32(ks + q * kGolden);
    uint32_t x = g;
    do {
        uint32_t L = x >> h, R = x & m;
        for (uint32_t q = 0; q < 4; q++) { const uint32_t t = L ^ (mix32(R ^ rk[q]) & m); L = R; R = t; }
        x = (L << h) | R;
    } while (x >= n);
    return x;
}

// unsigned division by a runtime constant (host precomputed): q = (n * m) >> 32 >> s, n < 2^31
struct FastDiv {
    uint32_t d = 1, m = 0, s = 0;
    FastDiv() = default;
    __host__ __device__ explicit FastDiv(uint32_t div)
    {
        d = div ? div : 1;
        if (d == 1) { m = 0; s = 0; return; }
        uint32_t l = 0;
        while ((1ull << l) < d) l++;
        m = (uint32_t)(((1ull << (31 + l)) / d) + 1ull);
        s = 31 + l;
    }
};

// ---- kernel launch API (sampler.hip, gather.hip, build_kernels.hip, sort_scan.hip, probes.hip) -------------------------------------------------------------
struct CsrTables {                 // GPU_Memory_Graph_Storage.cu:45-133: the whole CSR + the clique's fragments
    const int64_t* indptr;         // whole CSR (the reference's slot [P]): HBM replica or pinned host table
    const int32_t* indices;
    // fragments are lists of chunk allocations (see GPUGraphStorage): device-side pointer tables, part-major
    const int64_t* const* frag_indptr;  // [P * ip_nch]; chunk q of part p holds indptr entries [q<<row_shift, ((q+1)<<row_shift)]
    const int32_t* const* frag_indices; // [P * ix_nch]; chunk q holds the rows whose first edge lies in [q<<edge_shift, (q+1)<<edge_shift)
    int32_t ip_nch, ix_nch, row_shift, edge_shift;
    int32_t partition_count;
    const int8_t* topo_owner;      // int8[V]  owner logical GPU or -1 (edge_index_map), may be null
    const int32_t* topo_row;       // int32[V] row in the owner's fragment (edge_offset_map)
};

struct BatchCtl {                  // device-resident batch cursor (see k_seed); 20 bytes, one line
    int32_t counter;               // batch index inside the seed list
    uint32_t epoch;                // position-table epoch of the running batch
    // Seeded sampling (GPUMemoryPool_SetSampleSeed, INTEGRATION.md "Seeded sampling"): `draw` is the batch's draw word W -- what k_sample
    // reads, beside `epoch` --, 0 with the mode off, which is today's stream (s_b = 1) and today's distinct key.  Whoever sets `counter`
    // (k_seed host-driven, k_set_cursor, k_advance) sets it too, from the seeded flag and the round's key.
    uint32_t draw;
    uint32_t seeded;               // 0: mode off
    uint32_t draw_key;             // mix32(mix32(S ^ kDrawTag) ^ round)
};

struct HopState {                  // written by the scan kernel, read by the write/resolve kernels
    int32_t edge_base, node_base, n_edges, n_nodes, in_off, n_in, slots, pad;
};

struct SamplerBuffers {
    int32_t* sampled_ids;   // IPC buffer LEGION_BUF_IDS
    int32_t* agg_src_ids;   // per-edge neighbour id == next hop's input list
    int32_t* agg_src_off;   // IPC buffer LEGION_BUF_AGG_SRC
    int32_t* agg_dst_off;   // IPC buffer LEGION_BUF_AGG_DST
    int32_t* nc;            // IPC buffer LEGION_BUF_NODE_COUNTER
    int32_t* ec;            // IPC buffer LEGION_BUF_EDGE_COUNTER
    pos_t* pos_map;         // pos_t[V]: (epoch << kPosShift) | value
    const BatchCtl* ctl;    // ctl->epoch = 0xFFFFFFFF - batch serial: newer batches compare smaller
    int32_t* cand;          // i32[max slots of a hop]
    int32_t* aux;           // i32[max slots of a hop], slot state: -1 claim pending / won (k_mark: winner rank), >= 0 known position, <= -2 lost to slot -2-x
    int32_t* aux_next;      // the other buffer: k_write prepares it (-1) for the next hop
    int32_t next_count;     // fan-out of the next hop (0: none)
    int32_t aux_cap;        // elements per aux buffer
    int32_t ids_cap;        // elements of sampled_ids / agg_src_ids / agg_src_off / agg_dst_off (num_ids)
    int32_t V;              // entries of pos_map
    bool aux_prepared;      // aux already holds -1 for nc[LEGION_NC_NEXT_INPUTS] * count slots
    int32_t* tile_edge;     // i32[max tiles]
    int32_t* tile_node;     // i32[max tiles]
    int2* tile_pre;         // int2[max tiles]: (edges, new nodes) in front of a tile inside its k_mark chunk
    int2* chunk_tot;        // int2[kMaxChunks]: totals of the k_mark chunks
    HopState* hop_state;
    unsigned long long* edge_access_time; // pre-sampling only (may be null)
};

// Drawn link-prediction thirds: what k_seed<.., LP> needs beyond the default mode's arguments, fixed for a recording
struct LpDrawArgs {
    int32_t k = 0;                 // triples per batch: the batch is 3 k slots
    int32_t V = 0;                 // negatives are uniform on [0, V); V <= entries of the position table
    CsrTables csr = {};            // where the positive's row is read: as the sampler would read it on this GPU
};
// k_seed's operands; lp: null = the default mode (the instantiation that ran before the mode existed).  A self-driven launch (a captured batch
// graph) reads counter and epoch from ctl, computes the clamped size on the device and is sized for a full batch.
struct SeedArgs {
    int32_t *batch_ids, *labels;
    int32_t batch_size, size, counter, total_cap;
    const int32_t *all_ids, *all_labels;
    pos_t* pos_map;
    BatchCtl* ctl;
    int32_t *nc, *ec, *aux_next;
    int32_t f_next, aux_cap;
    uint32_t epoch, seeded, draw_key;
    const LpDrawArgs* lp;
};
void launch_seed(hipStream_t s, const SeedArgs& a, bool self_driven);
void launch_set_cursor(hipStream_t s, BatchCtl* ctl, int32_t counter, uint32_t epoch, uint32_t seeded = 0, uint32_t draw_key = 0);
// out_ids[g] = ids[perm(g)], out_labels[g] = labels[perm(g)] for g < n under shuffle key ks (seeded_perm)
void launch_shuffle_seeds(hipStream_t s, const int32_t* ids, const int32_t* labels, int32_t n, uint32_t ks, int32_t* out_ids, int32_t* out_labels);
// the same for a [src | pos | neg] list of batches of 3 k (n a multiple of 3 k): whole triples move, under perm on [0, n / 3)
void launch_shuffle_triples(hipStream_t s, const int32_t* ids, const int32_t* labels, int32_t n, int32_t k, uint32_t ks, int32_t* out_ids, int32_t* out_labels);
void launch_advance(hipStream_t s, BatchCtl* ctl);
int sampler_cu_count();       // compute units every grid is sized by (current device; asked once per process)
void warm_static_tables();   // per-device constant tables: must exist before a stream capture starts
// What a hop draws by: the rule and its tables beside the whole CSR -- the alias table (both weighted rules; Weighted reads it) and the graph's
// retained edge weights (WeightedDistinct and WeightedShared read them); null under the other rules.  Resolved from (graph, modes, device) in launchers.cpp.
struct DrawTables { DrawRule rule; const AliasEntry* alias; const float* weights; };
// Edge ids (GPUMemoryPool_SetEdgeIds): what a hop needs beyond the sampler's buffers to hand over every edge's position in the whole CSR.
// k_sample parks the slot's column in cols, k_edge_ids behind k_write stores edge_ids[e] = indptr[src] + column and, with weights, edge_w[e].
struct EdgeIdOut {
    int32_t* cols;            // i32[max slots of a hop], the pool's (dead once the hop has returned)
    int64_t* edge_ids;        // i64[ids_cap], the pipe's
    float* edge_w;            // f32[ids_cap], the pipe's; filled when `weights` is there
    const int64_t* indptr;    // the WHOLE CSR's, whatever the hop draws from (a fragment row is the whole row's copy)
    const float* weights;     // the graph's retained weights on this GPU, or null
    int64_t E;                // entries of the whole CSR
};
// eo: null = the hop as it always was; else the k_sample instantiation that parks the columns, and one more launch, k_edge_ids
void launch_sample_hop(hipStream_t s, const CsrTables& csr, const SamplerBuffers& b, int32_t count, int32_t op_id,
                       int32_t hops, int32_t slots_bound, bool is_presc, const DrawTables& draw, const EdgeIdOut* eo = nullptr);
// Weighted sampler mode, the graph's side (build_kernels.hip "alias table").  bad := the number of weights that are negative, NaN or infinite
// (a device word the caller zeroed); the table of every row of the CSR from w, with p = double[E] of scratch.  Deterministic: the same
// weights give the same bytes.
void launch_check_weights(hipStream_t s, const float* w, int64_t E, unsigned long long* bad);
void launch_build_alias(hipStream_t s, const int64_t* indptr, const int32_t* indices, const float* w, int32_t V, int64_t E, double* p, AliasEntry* table);
// k[m] = the column and ub[m] the keep-or-alias word of slot slot[m] of row row[m] of hop hop[m] at degree deg[m] under draw word word[m]
void launch_weighted_probe(hipStream_t s, const int32_t* row, const int32_t* hop, const int32_t* slot, const int32_t* deg, const uint32_t* word,
                           int32_t* k, uint32_t* ub, int32_t n);
// weighted sampling without replacement: u[m] and key[m] of column col[m] of row row[m] of hop hop[m] under draw word word[m] at weight w[m] > 0
void launch_shared_draw_probe(hipStream_t s, const int32_t* ids, const uint32_t* word, uint32_t* key, int32_t n);
// weighted shared-key sampling: u[m] and key[m] of neighbour id ids[m] under draw word word[m] at weight w[m] > 0
void launch_weighted_shared_probe(hipStream_t s, const int32_t* ids, const uint32_t* word, const float* w, uint32_t* u, double* key, int32_t n);
void launch_weighted_distinct_probe(hipStream_t s, const int32_t* row, const int32_t* hop, const int32_t* col, const uint32_t* word, const float* w,
                                    uint32_t* u, double* key, int32_t n);
void launch_find_feat(hipStream_t s, const int32_t* sampled_ids, int32_t* cache_offset, const int32_t* nc,
                      int32_t op_id, const int32_t* feat_map, int32_t bound);
void launch_find_topo(hipStream_t s, const int32_t* input_ids, int8_t* part_index, int32_t* part_offset,
                      int32_t batch_size, const int8_t* topo_owner, const int32_t* topo_row);
struct GatherArgs {
    const float* table;                       // V x F rows: the "cpu_float_attrs" of the reference
    // clique caches (Global_Float_Feature_Cache, the reference's float** cache_float_attrs): device table of
    // Kg x nchunks chunk pointers (a shard is a ChunkList); shard row r lives in chunk r >> chunk_shift
    const float* const* shard_tab;
    int32_t chunk_shift, nchunks;
    const int32_t* feat_map;                  // int32[V] global slot or -1; null = no cache
    const float** row_ptr;                    // scratch [rows]: address of each row's source (own shard / peer shard / backing
                                              // table / null), resolved by a lookup pass in front of the gather; null: resolve
                                              // inside the gather (no cache)
    int32_t cache_capacity;                   // rows per GPU
    int32_t F;
    int32_t table_pitch, shard_pitch;         // floats between two rows of the backing table / of a shard chunk (0: F, dense).
                                              // HBM copies we own are laid out with a 128-byte-aligned pitch when F * 4 is not
                                              // a multiple of 128 (F = 100: 512 bytes), so that every row read starts on a line
    int32_t total_num_nodes;
    const int32_t* sampled_ids;
    const int32_t* nc;
    float* dst;
    int32_t off_idx, size_idx;                // nc[] words of (offset, size), legion_idx_*; off_idx < 0 => offset 0
    int32_t dst_rows;                         // capacity of dst in rows (<= 0: unbounded)
    int32_t* rows_seen;                       // host-mapped word: the launch leaves its actual row count here (may be null)
    int32_t* hit_stats;                       // host-mapped {hits, rows}: the lookup pass of a SAMPLED batch adds its counts (may be null)
    int32_t rows_hint;                        // row count of an earlier launch of this kind (0: unknown)
    bool table_on_host;                       // the backing table is pinned host memory (misses cross PCIe)
    bool row_ptr_ready;                       // row_ptr was filled by the caller (exchange plan): skip the lookup pass
};
void launch_gather(hipStream_t s, const GatherArgs& a, int32_t rows_bound);
// Edge features (gather.hip "S5, edge features"): out[e, :] = table[edge_ids[e], :] for the COO edges e of hop `hop` of the pipe's batch
// (hop 0: all of them, [0, legion_batch_edges)), the range read from ec on the device and clamped to ids_cap; an id outside [0, E) stores zeros.
struct EdgeGatherArgs {
    const float* table;       // the graph's float32 [E, dim], dense, on this GPU
    int64_t E;
    int32_t dim;
    const int64_t* edge_ids;  // the pipe's, as k_edge_ids left them
    const int32_t* ec;        // the pipe's edge counters
    int32_t hop, hops;        // 1..hops, or 0 = every hop
    float* out;               // the pipe's edge_feat, float32 [ids_cap, dim]
    int32_t ids_cap;          // rows of edge_ids and of out
};
// chunks a row of `dim` floats is gathered in (16-byte chunks where dim % 4 == 0, else floats): what the 32-bit flat work space is counted in
constexpr int32_t edge_gather_chunks(int32_t dim) { return dim % 4 == 0 ? dim / 4 : dim; }
void launch_gather_edges(hipStream_t s, const EdgeGatherArgs& a, int32_t edges_bound);
// Target-edge exclusion (lp_exclude.hip, lp_exclude.h): the pair table of a batch's k target pairs, behind k_seed, and the marking pass over
// every COO edge of the batch, behind the last hop.  Everything here but the counters' layout belongs to the batch's pipe.
struct LpPairsArgs {
    const int32_t* ids;       // the pipe's sampled_ids: [0, 2 k) are the src and pos thirds, as k_seed left them
    const int32_t* nc;        // the pipe's node counters: the level-0 size is read on the device
    uint64_t* pairs;          // uint64[cap], the pipe's lp_pairs
    int32_t* excluded;        // int32[kLpExcludedWords], the pipe's lp_excluded: zeroed here
    int32_t k, cap;
};
void launch_lp_pairs(hipStream_t s, const LpPairsArgs& a);
struct LpKeepArgs {
    const int32_t *ids, *src_off, *dst_off, *nc, *ec;   // the pipe's batch
    const uint64_t* pairs;    // as k_lp_pairs left it; not read when !active
    uint8_t* keep;            // uint8[ids_cap], the pipe's edge_keep
    int32_t* excluded;        // the pipe's lp_excluded
    int32_t k, cap, hops, ids_cap;
    bool active;              // k_lp_pairs ran for this batch (a training batch); false: every edge is kept and the counts are zeroed here
};
constexpr int kLpExcludedWords = 8;
void launch_lp_edge_keep(hipStream_t s, const LpKeepArgs& a, int32_t edges_bound);
// Aggregated last hop (gather.hip "S5, aggregated last hop"): the neighbour sums of the last hop's runs_bound (static bound) input
// slots, from the draws in cand[slot * f + j], into rows [legion_first_block_dst(nc, hops), + runs) of a.dst.  a.sampled_ids / a.row_ptr are not read.
// wdraw (normalised sums): the weight of every draw by slot, as launch_agg_norm_weights left it; null = plain sums.
void launch_gather_sum(hipStream_t s, const GatherArgs& a, const int32_t* cand, int32_t cand_cap, const int32_t* ec, int32_t hops,
                       int32_t f, int32_t runs_bound, const float* wdraw = nullptr);
// Normalised last hop (gather.hip "S5, normalised last hop"): out_deg[p] = out-degree of batch position p inside block 1 (all edges of
// the batch), and wdraw[slot] = 1 / sqrt(max(out_deg[position of the slot's draw], 1)) for every slot of the last hop with a draw.
// Everything here belongs to the batch's pipe.
struct AggNormArgs {
    const int32_t* nc;
    const int32_t* ec;
    int32_t hops, f;
    const int32_t* cand;     // the last hop's draws
    int32_t cand_cap;        // elements of cand and of wdraw
    const int32_t* src_off;  // the pipe's COO sources (agg_src_off)
    int32_t ids_cap;         // elements of src_off and of out_deg
    int32_t* out_deg;
    int32_t* chunk_cnt;      // int32[kMaxChunks]: draws per chunk of slots
    float* wdraw;
};
void launch_agg_norm_weights(hipStream_t s, const AggNormArgs& a, int32_t slots_bound, int32_t edges_bound);
// Edge-weighted last hop (gather.hip "S5, edge-weighted last hop"): wdraw[slot] = edge_w[edge of the slot's draw] for every slot of the last hop
// with a draw, edge_w as k_edge_ids left it behind the last hop.  Everything here belongs to the batch's pipe.
struct AggEdgeWeightArgs {
    const int32_t* nc;
    const int32_t* ec;
    int32_t hops, f;
    const int32_t* cand;     // the last hop's draws
    int32_t cand_cap;        // elements of cand and of wdraw
    const float* edge_w;     // the pipe's edge weights, by COO edge
    int32_t ids_cap;         // elements of edge_w
    int32_t* chunk_cnt;      // int32[kMaxChunks]: draws per chunk of slots
    float* wdraw;
};
void launch_agg_edge_weights(hipStream_t s, const AggEdgeWeightArgs& a, int32_t slots_bound);
// words of GPUMemoryPool::rows_seen: [l] = level-l gather, then one per launch kind below
constexpr int kRowsSeenAll = LEGION_MAX_HOPS + 1;      // all rows of the batch (get_feature_kernel_all)
constexpr int kRowsSeenAggIn = LEGION_MAX_HOPS + 2;    // rows of the levels < H (get_feature_kernel_agg)
constexpr int kRowsSeenAggRuns = LEGION_MAX_HOPS + 3;  // input slots of the last hop (get_feature_kernel_agg)
constexpr int kRowsSeenWords = LEGION_MAX_HOPS + 4;
// owner-computes exchange variant of the gather (gather.hip "S5, owner-computes"): counts = int32[2 * kMaxParts] scratch
void launch_exchange_plan(hipStream_t s, const GatherArgs& g, int32_t me, int32_t Kg, int32_t* slot, int32_t* counts,
                          int32_t* req_row, int32_t* req_dst, int32_t rows_bound);
void launch_exchange_rows(hipStream_t s, bool scatter, const float* const* shard_chunks, int32_t chunk_shift, const int32_t* list,
                          int32_t n, int32_t F, int32_t shard_pitch, const float* in, float* out, int32_t out_rows);
void launch_hotness(hipStream_t s, const int32_t* ids, const int32_t* nc, int32_t hops, unsigned long long* access,
                    int32_t* max_ids, int32_t bound);
void launch_rng_probe(hipStream_t s, const int32_t* idx, const int32_t* deg, int32_t* k, int32_t n);
void launch_distinct_probe(hipStream_t s, const int32_t* row, const int32_t* hop, const int32_t* deg, int32_t f, int32_t* pos, int32_t n);
// the seeded counterparts (w = the batch's draw word) and perm(0 .. n - 1) of a round
void launch_seeded_rng_probe(hipStream_t s, uint32_t w, const int32_t* idx, const int32_t* deg, int32_t* k, int32_t n);
void launch_seeded_distinct_probe(hipStream_t s, uint32_t w, const int32_t* row, const int32_t* hop, const int32_t* deg, int32_t f, int32_t* pos, int32_t n);
void launch_perm_probe(hipStream_t s, uint32_t ks, int32_t n, int32_t* out);
// drawn link-prediction thirds under draw word w: rho[i] = the positive's position in a row of degree deg[i] (-1: deg <= 0), neg[i] on [0, V)
void launch_lp_draw_probe(hipStream_t s, uint32_t w, const int32_t* src, const int32_t* deg, int32_t V, int32_t* rho, int32_t* neg, int32_t n);
// cache construction helpers
void launch_aggregate_access(hipStream_t s, unsigned long long* agg, const unsigned long long* add, int32_t n);
void launch_iota(hipStream_t s, int32_t* out, int32_t n);
void launch_build_feat_map(hipStream_t s, int32_t* feat_map, const int32_t* QF, int32_t capacity, int32_t Kg, int32_t V);
void launch_build_topo_map(hipStream_t s, int8_t* owner, int32_t* row, const int32_t* QT, int32_t capacity, int32_t Kg,
                           int32_t Ki, int32_t V);
void launch_fill_i32(hipStream_t s, int32_t* p, int32_t v, int64_t n);
void launch_fill_i8(hipStream_t s, int8_t* p, int8_t v, int64_t n);
void launch_feat_fill_up(hipStream_t s, int32_t row0, int32_t rows, int32_t F, int32_t chunk_pitch, int32_t table_pitch, float* chunk,
                         const float* table, const int32_t* QF, int32_t Kg, int32_t Ki, int32_t V);
void launch_copy_rows_pitched(hipStream_t s, float* dst, int32_t dst_pitch, const float* src, int32_t src_pitch, int32_t F, int64_t rows);
void launch_neighbor_count(hipStream_t s, const int32_t* QT, int32_t Kg, int32_t Ki, int32_t capacity, int32_t V,
                           const int64_t* indptr, int64_t* count_out);
void launch_topo_fill_up(hipStream_t s, const int32_t* QT, int32_t Kg, int32_t Ki, int32_t capacity, int32_t V,
                         const int64_t* indptr, const int32_t* indices, const int64_t* frag_indptr,
                         int32_t* const* frag_chunks, int32_t edge_shift);
// ends[q] = end offset of the last row that starts before (q+1) << edge_shift   (q < nch - 1)
void launch_chunk_ends(hipStream_t s, const int64_t* frag_indptr, int32_t capacity, int32_t edge_shift, int32_t nch, int64_t* ends);
void launch_edge_mem(hipStream_t s, const int32_t* order, uint64_t* edge_mem, int32_t V, const int64_t* indptr);
void launch_topo_transactions(hipStream_t s, const int32_t* order, const uint64_t* hot, uint64_t* out, int32_t V, const int64_t* indptr);
void sort_by_hotness_desc(hipStream_t s, unsigned long long* keys, int32_t* ids, int32_t n);
void inclusive_scan_u64(hipStream_t s, const uint64_t* in, uint64_t* out, int32_t n);
void inclusive_scan_i64(hipStream_t s, const int64_t* in, int64_t* out, int32_t n);

} // namespace legion

// ---- the opaque handle types (host mirrors of the reference classes) ------------------------------
struct PeerExchange;               // peer_exchange.cpp: staging of the bulk-copy (hipMemcpyPeerAsync) gather
struct GPUMemoryPool {
    int32_t pipeline_depth = LEGION_PIPELINE_DEPTH;
    int32_t current_pipe = 0, iter = 0, mode = 0, op_id = 0;
    int32_t device_id = -1;           // logical GPU this pool serves (set by batch_generator_kernel)
    // scratch owned by the pool when AllocateScratch() was used
    bool owns_scratch = false;
    int32_t V = 0, batch_size = 0, hops = 0, num_ids = 0;
    int32_t fanout[LEGION_MAX_HOPS] = {0};
    int32_t max_slots = 0, max_tiles = 0;
    int32_t feature_rows = 0;         // capacity of the feature buffers in rows (0 = unbounded)
    legion::pos_t* pos_map = nullptr; // pos_t[V], see sampler.hip "position table"
    uint32_t batch_serial = 0;        // batches started on this pool; epoch = 0xFFFFFFFF - serial
    legion::BatchCtl* ctl = nullptr;  // device copy of (batch cursor, epoch): what the kernels read
    // Feedback for sizing the gather launches without a host round trip: pinned, device-mapped words the gather
    // kernels write their actual row count to ([l] = level-l gather, [LEGION_MAX_HOPS + 1] = all rows of the batch);
    // the host reads whatever an earlier batch left there.
    int32_t* rows_seen = nullptr;      // host view
    int32_t* rows_seen_dev = nullptr;  // device view of the same words
    bool capturing = false;           // between Begin/EndBatchCapture: launchers record a self-driven batch
    bool ctl_synced = false;          // ctl holds (ctl_counter, epoch of the NEXT batch): a batch graph can run as is
    int32_t ctl_counter = 0;
    int32_t* cand = nullptr;
    // The serving modes the pool is in: set through pool_apply_modes only (the public setters change one field each), read by the launchers.
    legion::ServeModes modes;
    // What one launcher of a batch leaves for the next: reset by batch_generator_kernel, stored by a recording, restored by a replay
    struct Progress {
        int32_t sampled_hop = 0;      // hops of the current batch that GPU_Random_Sampling has queued (0 behind batch_generator_kernel)
        bool sampled_presc = false;   // ... as pre-sampling hops
        uint32_t levels_gathered = 0; // bit l: get_feature_kernel gathered level l of the current batch
        int32_t edge_id_hop = 0;      // hops 1..edge_id_hop of the current batch left their edge ids (k_edge_ids is queued behind each of them)
        bool edge_feat_gathered = false;   // get_edge_feature_kernel(_all) gathered edge rows of the current batch (-> Pipe::edge_feat_filled)
        bool lp_pairs_built = false;  // k_lp_pairs is queued behind the current batch's k_seed: a training batch under modes.lp_exclude
        bool lp_marked = false;       // k_lp_edge_keep is queued behind the current batch's last hop (-> Pipe::lp_marked)
    } progress;
    // Everything that exists once per pipe.  own[]: the device buffers the POOL owns per pipe, one row of pool_pipe_buffers() each (below) --
    // allocated when a mode that wants them is set, kept until the scratch is released, null before.  cand_pipe: the aggregated last hop parks
    // its draws in the PIPE's buffer, because k_gather_sum reads them on the gather stream while hop 1 of the next batch already overwrites
    // `cand` on the sampler stream.  The normalised sums rank them through agg_out_deg / agg_wdraw / agg_chunk_cnt; the edge-weighted sums use
    // the last two in the same way and no degrees.  edge_ids / edge_w: the batch's, read back by callers.  edge_feat: float32 [num_ids,
    // modes.edge_feat_dim], the batch's gathered edge rows (GPUMemoryPool_SetEdgeFeatures), read back by callers.  lp_pairs / edge_keep /
    // lp_excluded: the target pairs' table, the keep byte of every COO edge and the counts of the zeros (GPUMemoryPool_SetLpExclude); the last
    // two are read back by callers.
    enum PipeBuf { kCandPipe, kAggOutDeg, kAggWdraw, kAggChunkCnt, kEdgeIds, kEdgeW, kEdgeFeat, kLpPairs, kEdgeKeep, kLpExcluded, kPipeBufs };
    struct Pipe {
        float* float_features = nullptr;   // the seven buffers the caller registered (IPC buffers)
        int32_t *labels = nullptr, *node_counter = nullptr, *edge_counter = nullptr, *sampled_ids = nullptr, *agg_src_off = nullptr, *agg_dst_off = nullptr;
        void* own[kPipeBufs] = {};
        bool edge_w_filled = false;        // the pipe's last batch ran over retained weights (GetEdgeWeightBuffer is null otherwise)
        bool edge_feat_filled = false;     // the pipe's last batch had its edge rows gathered (GetEdgeFeatureBuffer is null otherwise)
        bool lp_marked = false;            // the pipe's last batch ran the marking launch (GetEdgeKeepBuffer / GetLpExcludedBuffer are null otherwise)
        template <typename T> T* buf(PipeBuf b) const { return (T*)own[b]; }
    };
    std::vector<Pipe> pipes;               // pipeline_depth of them from the constructor on, never resized
    Pipe& pipe() { return pipes[current_pipe]; }
    const Pipe& pipe() const { return pipes[current_pipe]; }
    // Seeded sampling (modes.seeded / modes.seed, GPUMemoryPool_BeginRound): the training batches read the round's shuffled copy of the
    // training list (shuf_ids / shuf_labels, filled by k_shuffle_seeds in BeginRound; allocated there on first use, never inside a capture).
    // shuf_src: the seed set's list the copy was made of; shuf_valid: it holds the permutation of (seed, round).  shuf_file_order: BeginRound
    // was told to leave the training list in file order (lists served verbatim, link-prediction thirds) -- the draws are still seeded.
    uint32_t round = 0;
    int32_t* shuf_ids = nullptr;
    int32_t* shuf_labels = nullptr;
    int32_t shuf_cap = 0, shuf_n = 0;
    const int32_t* shuf_src = nullptr;
    bool shuf_valid = false, shuf_file_order = false;
    bool seed_reads_shuffle = false;  // the last batch_generator_kernel (the recording's, inside a capture) read the shuffled copy
    // Drawn link-prediction thirds (modes.lp_draw = k, GPUMemoryPool_SetLpDraw): the graph the positives are read from -- kept here because
    // batch_generator_kernel has the reference's signature, without a graph.  Under the mode BeginRound shuffles whole triples into the same copy.
    GPUGraphStorage* lp_graph = nullptr;
    // Edge ids (modes.edge_ids, GPUMemoryPool_SetEdgeIds): max_slots words, one buffer (written by k_sample, read by k_edge_ids of the same
    // hop); allocated when the mode is switched on, kept until the scratch is released
    int32_t* cols = nullptr;
    int32_t edge_feat_alloc_dim = 0;  // the row width the pipes' edge_feat buffers are allocated for (0: none); another dim reallocates them
    uint32_t edge_feat_gen = 0;       // ... and counts every such (re)allocation and release: a batch graph that writes them replays only under the count it recorded
    // Target-edge exclusion (modes.lp_exclude, GPUMemoryPool_SetLpExclude): the table capacity the pipes' lp_pairs are allocated for (0: none;
    // a k of another capacity reallocates them), and the count of such (re)allocations and releases, by the rule of edge_feat_gen
    int32_t lp_alloc_cap = 0;
    uint32_t lp_gen = 0;
    int32_t* aux2[2] = {nullptr, nullptr}; // slot states, one buffer per hop parity (hop h uses aux2[h & 1])
    int32_t aux_ready_hop = 0, aux_ready_count = 0; // the launch before prepared aux2[hop & 1] for this fan-out
    int32_t* tile_edge = nullptr;
    int32_t* tile_node = nullptr;
    int2* tile_pre = nullptr;
    int2* chunk_tot = nullptr;
    legion::HopState* hop_state = nullptr;
    int32_t* cache_search_buffer = nullptr;
    const float** row_ptr = nullptr;  // [num_ids] row source addresses of the running gather (cached configurations)
    PeerExchange* peer_exchange = nullptr; // created by the first legion_peer_exchange_gather of this pool
    int32_t* agg_src_ids = nullptr;
    int8_t* tmp_part_ind = nullptr;
    int32_t* tmp_part_off = nullptr;
    // host-side launch bounds (no device round trips)
    int32_t bound_n = 0;        // upper bound of the next hop's input count
    int32_t bound_nodes = 0;    // upper bound of nodes discovered so far
    int32_t level_bound[LEGION_MAX_HOPS + 1] = {0};
    explicit GPUMemoryPool(int32_t depth);
};
namespace legion {
// The pool's modes := wanted, once for every mode.  Refused in who's name: a null pool, a pool that is being captured (a recording keeps
// its modes).  Refused as GPUMemoryPool_SetAggNorm: an unknown norm, and a norm on a pool that does not aggregate the last hop -- unless the
// pool holds that norm already (it stays set while the aggregated mode is off).  Refused in who's name, whichever setter comes second: the
// edge-weighted sums (agg_edge_weight) without the aggregated mode -- unless the pool holds the flag already --, without edge ids, or together
// with a norm; and the edge features (edge_feat_dim) without edge ids, at a negative width, or at a width whose per-pipe buffer overflows or
// whose flat work space (num_ids * edge_gather_chunks) reaches 2^31.  Refused as GPUMemoryPool_SetLpDraw: a negative triple count,
// and a positive one on a pool without a graph (lp_graph).  Allocates the aggregated modes' per-pipe buffers when the
// pool owns scratch (call it under the scratch's device); another seed invalidates the shuffled copy, another seeded state the graph cursor.
bool pool_apply_modes(GPUMemoryPool* p, const ServeModes& wanted, const char* who);
// The pool's two buffer tables (memory_pool.cpp, where the rules are written down): the scratch it owns once, and the buffers it owns per pipe,
// one row for every Pipe::own[which].  wanted: the pool's modes ask for it now; listed: GPUMemoryPool_ScratchInfo names it
struct ScratchBuffer { void** slot; size_t bytes; const char* name; int32_t kind, elem_bytes, lifetime; };
__attribute__((visibility("hidden"))) std::vector<ScratchBuffer> pool_scratch(GPUMemoryPool* p);
struct PipeBuffer { GPUMemoryPool::PipeBuf which; size_t bytes; bool wanted, listed; const char* name; int32_t kind, elem_bytes, lifetime; };
__attribute__((visibility("hidden"))) std::array<PipeBuffer, GPUMemoryPool::kPipeBufs> pool_pipe_buffers(const GPUMemoryPool* p);
}

struct GPUGraphStorage {
    int32_t partition_count = 0;
    int32_t node_num = 0;
    int64_t edge_num = 0, cache_edge_num = 0;
    int64_t* csr_node_index_cpu = nullptr;   // device-visible pointer of the whole CSR (slot [P])
    int32_t* csr_dst_node_ids_cpu = nullptr;
    // HBM replicas of the whole CSR, one per logical GPU that has one (GPUGraphStorage_ReplicateToDevices)
    std::vector<int64_t*> replica_indptr;
    std::vector<int32_t*> replica_indices;
    // Weighted sampler mode (GPUGraphStorage_SetEdgeWeights): the alias table of the whole CSR per logical GPU, device memory, one copy per
    // physical device like the replicas; empty / null = no weights are set
    std::vector<legion::AliasEntry*> alias;
    // Weighted sampling without replacement reads the weights themselves: with retain_weights set (GPUGraphStorage_RetainEdgeWeights, before
    // SetEdgeWeights) the float32[E] device copy the table was built from stays next to the table, shared per physical device in the same
    // way; empty / null = not retained (the copy is freed after the build, as it always was)
    std::vector<float*> weights;
    bool retain_weights = false;
    // Edge features (GPUGraphStorage_SetEdgeFeatures): float32 [E, edge_feat_dim], dense, row e beside indices[e], device memory, one copy per
    // physical device by the rule of `weights`; empty / null = no table (edge_feat_dim == 0)
    std::vector<float*> edge_feat;
    int32_t edge_feat_dim = 0;
    int32_t csr_location = LEGION_LOC_HOST_PINNED;
    bool owns_csr = false;
    // CSR fragment of one logical GPU (device memory on that GPU's physical device).  Both arrays are chunk lists
    // (ChunkList, like the feature shards).  indptr chunk q: entries [q<<row_shift, min(rows, (q+1)<<row_shift)] (one entry of
    // overlap, so ip[r] and ip[r+1] come from the same chunk).  indices chunk q: every row whose first edge offset o
    // satisfies o >> edge_shift == q, whole, at element o & mask (the chunk is as long as its last row needs).
    struct Fragment {
        int32_t rows = 0;
        int64_t edges = 0;
        legion::ChunkList<int64_t> ip;       // both imported, or neither
        legion::ChunkList<int32_t> ix;
        bool complete = false;               // every chunk present (built locally, or all chunks imported)
    };
    std::vector<Fragment> frag;
    int32_t row_shift = 27, edge_shift = 28;
    // which fragments logical GPU d may read (its clique): view[d][p]
    std::vector<std::vector<bool>> view;
    // device-side chunk-pointer tables per local viewer (P*ip_nch indptr pointers, then P*ix_nch indices pointers)
    std::vector<void**> d_frag_tab;
    int32_t ip_nch = 1, ix_nch = 1;
};

struct GPUNodeStorage {
    int32_t partition_count = 0, total_num_nodes = 0, float_attr_len = 0;
    float* float_attrs = nullptr;     // device-visible V x F table
    int32_t float_attr_pitch = 0;     // floats between two rows of float_attrs (>= float_attr_len)
    std::vector<float*> replica_attrs; // HBM replicas per logical GPU (GPUNodeStorage_ReplicateToDevices)
    int32_t replica_pitch = 0;        // ... of the replicas (legion_row_pitch)
    int32_t features_location = LEGION_LOC_HOST_PINNED;
    bool owns_features = false;
    struct SeedSet { int32_t num = 0; int32_t* ids = nullptr; int32_t* labels = nullptr; };   // device copies
    std::vector<SeedSet> seeds[legion::kModes];    // by mode, per partition
    // the set of `mode` on partition p; an empty one (no lists, size 0) for any other mode or partition
    const SeedSet& seed_set(int32_t mode, int32_t p) const
    {
        static const SeedSet none;
        return mode >= 0 && mode < legion::kModes && p >= 0 && p < (int32_t)seeds[mode].size() ? seeds[mode][p] : none;
    }
};

struct CacheController {              // PreSCCacheController, GPUCache.cu:239-500
    int32_t device_idx = 0, device_count = 1, total_num_nodes = 0, train_step = 0;
    unsigned long long* node_access_time = nullptr;
    unsigned long long* edge_access_time = nullptr;
    int32_t iter = 0, max_ids = 0;
    int32_t* d_max_ids = nullptr;     // device-side running max of nc[LEGION_NC_TOTAL]
    int32_t node_capacity = 0, edge_capacity = 0;
    // direct-mapped replacements of the three BGHT maps (GPUCache.cu:315-321)
    int32_t* feat_map = nullptr;      // node_map_:       id -> global cache slot | -1
    int8_t* topo_owner = nullptr;     // edge_index_map_: id -> owner logical GPU | -1
    int32_t* topo_row = nullptr;      // edge_offset_map_: id -> row in owner's fragment | -1
    int32_t* d_global_count = nullptr;
    // Feature-cache hit rate (GPUCache.cu:130-147,414-425: counted every 500th batch, printed at the last level).
    // Two pinned, device-mapped {hits, rows} slots: sampling k counts into slot k % 2 while the host prints what
    // sampling k - 1 left in the other one -- no device-to-host copy, no synchronisation.
    int32_t find_iter = 0;
    int32_t* hit_stats = nullptr;      // host view, 2 x {hits, rows}
    int32_t* hit_stats_dev = nullptr;  // device view
    hipEvent_t hit_ev[2] = {nullptr, nullptr}; // recorded behind the last counting launch of the sampling that used slot k
    bool hit_ev_armed[2] = {false, false};
    int32_t hit_samples = 0;           // samplings started
    double last_hit_rate = -1.0;       // what the last print showed
};

struct GPUCache {
    int32_t device_count = 0;
    std::vector<CacheController*> ctl;
    std::vector<int32_t*> QF, QT;                    // per clique, on the clique's first GPU
    std::vector<unsigned long long*> AF, AT;
    int Kc = 1, Kg = 1;
    std::vector<int32_t> node_capacity, edge_capacity;   // per clique
    std::vector<double> alpha;
    int64_t cache_memory = 0;
    int32_t int_attr_len = 0, float_attr_len = 0, train_step = 0;
    std::vector<legion::ChunkList<float>> shards;    // per logical GPU: the shard's chunk allocations
    std::vector<float**> d_shard_tab;                // per LOCAL logical GPU: device table [Kg x nchunks]
    std::vector<int32_t> chunk_shift, nchunks;       // per clique
    int32_t shard_pitch = 0;                         // floats between two rows of a shard chunk (legion_row_pitch(F))
    bool is_presc = true;
    bool capacity_forced = false;
    int32_t forced_node_capacity = 0, forced_edge_capacity = 0;
};
