// sampler.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the mini-batch hot path: the seed launch and the sampler's three
// passes per hop.  (The gathers and the exchange are gather.hip, the one-off construction kernels build_kernels.hip.)
//
// Reference semantics restated (liayan/Legion-1, src/):
//   S1 batch_generator                Kernels.cu:68-96      -> k_seed
//   S2 update_counter                 Kernels.cu:112-150    -> folded into k_seed / k_write (last tile)
//   S3 kernel_random_sampler_2        Kernels.cu:342-448    -> k_sample + k_mark + k_write
//   S3' kernel_pre_sampler_optimized  Kernels.cu:468-564    -> k_sample<.., RowSource::Presc, ..>
//   S4 construct_graph                Kernels.cu:450-463    -> k_write (both sides)
//   S5 zero_copy_with_aggregated_cache Kernels.cu:662-702   -> k_gather (+ k_row_ptrs in front of a cached gather): gather.hip
//   S6 FindFeat/FindTopo (BGHT find)  GPUCache.cu:387-461   -> direct-mapped int32/int8[V] tables: gather.hip, build_kernels.hip
//   S7 ClearPosMap / HotnessMeasure   Kernels.cu:750-756, GPUCache.cu:227-235 -> no kernel (table epochs) / k_hotness: build_kernels.hip
//
// Design (DESIGN.md has the long form):
//  * The reference's output ORDER depends on LDS/global atomicAdd races.  We produce the
//    canonical schedule (serial, slot-index ascending) deterministically: a hop is
//      k_sample : every slot draws its neighbour (same Thrust minstd arithmetic), parks it in
//                 cand[idx] and claims the node with atomicMin(pos[dst], PROVISIONAL|idx), so the
//                 LOWEST slot that touches a new node wins -- exactly the serial order.  Slot state
//                 aux[idx]: -1 claim pending / won, >= 0 the neighbour's known final position,
//                 <= -2 lost to slot -2-x.  Repeated draws of a row are settled in-wave; a claim that
//                 replaces a larger slot's claim writes that slot's state ("you lost to me");
//      k_mark   : streaming pass over the states: a slot still at -1 kept its claim = a new node; it gets its
//                 rank among the new nodes of its tile, the tile its count (no table probe); a workgroup runs a contiguous
//                 chunk of tiles and leaves each tile's (edges, new nodes) prefix inside the chunk + the chunk totals;
//      k_write  : every workgroup scans k_mark's <= 2048 chunk totals in LDS (no scan launch; + one 8-byte in-chunk prefix per tile),
//                 then ordered compaction (wave ballot + popcount prefix, one LDS exchange per tile)
//                 appends edges / new nodes at their canonical positions and both COO offsets -- an edge
//                 that lost its claim follows loser -> winner through the slot states and computes the
//                 winner's position from that tile's prefix + rank; it also sets the next hop's states
//                 to -1; the workgroup of the last tile applies update_counter (S2).
//    Three launches per hop (round 1: four), 11 per 3-hop batch with k_seed and the gather.  The three passes of a hop share one
//    tile size (template parameter TILE): kTile slots, or kTileNarrow on hops too small to fill the chip (internal.h).
//  * One u64[V] "position table" replaces accessed_map (bitmap) + position_map.  Entry =
//    (epoch << 32) | value, epoch = 0xFFFFFFFF - batch serial, so entries of older batches compare
//    GREATER than anything of the running batch: they are stale without ever being cleared (no
//    V/8-byte memset, no ClearPosMap scatter).  value: 0x80000000|idx = claimed in the running hop,
//    else the final index in sampled_ids.
//  * Row descriptors (start, degree) of a tile are fetched once per source row and staged in
//    LDS -- the reference re-reads both int64 indptr words in each of the `count` lanes.
//  * RNG: x = s_b * 48271^(idx+1) mod (2^31-1), s_b = 1 unless the pool is seeded (one more mul-mod per workgroup: the batch's s_b goes
//    into the workgroup's base power).  Per thread: one table lookup and one Mersenne
//    mul-mod per tile instead of Thrust's discard() chain of 2*log2(idx) 64-bit `%`.
//    The final fp64 divide/multiply/truncate is kept verbatim -- it is what makes k bit exact.
//  * All loop bounds come from device counters; launches are sized by static upper bounds, so
//    there is not a single device->host copy in the batch (the reference does 7).
#include "internal.h"
#include "draws.h"
#include "launch.h"
#include <array>
#include <mutex>

#include "audit_hooks.h"

namespace legion {

// ------------------------------------------------------------------------------------------------
// S1 + S2(op 0): seed batch
// ------------------------------------------------------------------------------------------------
// The positive of a drawn link-prediction triple (lp_rho, draws.h): one neighbour of src, read where k_sample would read that row (the owner's fragment when the topology map names one, else
// the whole CSR; fragment rows are copies in CSR order), degree as k_sample computes it; src itself for an empty row or a negative entry.
// The row addressing below restates k_sample's ("owner lookup, chunk tables, int32 degree") rather than sharing a helper with it, on
// purpose: k_sample interleaves those loads with its tile's other work and its instantiations are kept instruction for
// instruction.  Whoever changes the fragment layout changes both; the cached-topology test compares this copy with the uncached statement.
__device__ inline int32_t lp_pos(const CsrTables& c, uint32_t w, uint32_t i, int32_t src)
{
    const int64_t* ip = c.indptr + src;
    const int32_t* rowp;
    const int8_t owner = c.topo_owner ? c.topo_owner[src] : (int8_t)-1;
    int64_t start;
    if (owner >= 0) {
        const int32_t row = c.topo_row[src];
        ip = c.frag_indptr[owner * c.ip_nch + (row >> c.row_shift)] + (row & ((1 << c.row_shift) - 1));
        start = ip[0];
        rowp = c.frag_indices[owner * c.ix_nch + (int32_t)(start >> c.edge_shift)] + (start & ((1ll << c.edge_shift) - 1));
    } else {
        start = ip[0];
        rowp = c.indices + start;
    }
    const int32_t d = (int32_t)(ip[1] - start);
    if (d <= 0) return src;
    const int32_t pos = rowp[lp_rho(w, i, src, d)];
    return pos < 0 ? src : pos;
}

// Kernel's `batch_size` is the launcher's clamped `size` -- the reference passes `size`
// (Kernels.cu:227), so the read offset is size*counter (restated, not "fixed").
// SELF (captured batch graphs): the batch cursor and the table epoch live in device memory (BatchCtl),
// advanced by k_advance at the end of every graph launch, so that the captured launch has no per-batch
// arguments.  Host-driven launches pass both as arguments and publish them for the kernels that follow, and with them the batch's
// draw word (seeded sampling: BatchCtl::draw, 0 with the mode off).  In training mode under a seed all_ids / all_labels are the pool's
// shuffled copy of the list (k_shuffle_seeds), read exactly as the file-order list is.
// LP (GPUMemoryPool_SetLpDraw, training batches only): the batch is 3 k slots, [src | pos | neg].  Every thread reads the source of its
// slot i = idx % k from the (shuffled) triple list; a thread of the second third then reads the row descriptor and one neighbour, a thread
// of the last third hashes.  No thread waits for another; what follows the id (claim loop, counters, slot states) is the default mode's.
// LP = false is the kernel as it was: `lp` is not read.
template <bool SELF, bool LP>
__global__ __launch_bounds__(kBlock) void k_seed(int32_t* __restrict__ batch_ids, int32_t* __restrict__ labels,
                                                 int32_t batch_size, int32_t size, int32_t counter,
                                                 const int32_t* __restrict__ all_ids,
                                                 const int32_t* __restrict__ all_labels, int32_t total_cap,
                                                 pos_t* __restrict__ pos_map, uint32_t epoch,
                                                 BatchCtl* __restrict__ ctl, int32_t* __restrict__ nc,
                                                 int32_t* __restrict__ ec, int32_t* __restrict__ aux_next,
                                                 int32_t f_next, int32_t aux_cap, uint32_t seeded, uint32_t draw_key, LpDrawArgs lp)
{
    int32_t idx = threadIdx.x + blockDim.x * blockIdx.x;
    if (SELF) {
        counter = ctl->counter;
        epoch = ctl->epoch;
        // Kernels.cu:224 on the device (int64: counter is not bounded by the host here)
        const int64_t done = (int64_t)batch_size * counter;
        size = (done + batch_size >= total_cap) ? (int32_t)max((int64_t)0, min((int64_t)batch_size, (int64_t)total_cap - done)) : batch_size;
    } else if (idx == 0) {
        ctl->counter = counter;
        ctl->epoch = epoch;
        ctl->draw = seeded_draw_word(seeded, draw_key, counter);
        ctl->seeded = seeded;
        ctl->draw_key = draw_key;
    }
    if (idx < size) {
        int32_t g = size * counter + idx;
        if (g >= total_cap) {
            batch_ids[idx] = -1;
            labels[idx] = -1;
        } else {
            int32_t src_id, label;
            if constexpr (LP) {
                const int32_t q = (idx >= lp.k) + (idx >= 2 * lp.k), i = idx - q * lp.k;   // third, slot; size == 3 k (the launcher checked)
                const int32_t gs = g - q * lp.k;                                          // the slot's entry of the src third
                const uint32_t w = SELF ? ctl->draw : seeded_draw_word(seeded, draw_key, counter);
                src_id = all_ids[gs];
                label = -1;
                if (q == 0) label = all_labels[gs];
                else if (q == 1) src_id = lp_pos(lp.csr, w, (uint32_t)i, src_id);
                else src_id = lp_neg(w, (uint32_t)i, src_id, lp.V);
            } else {
                src_id = all_ids[g % total_cap];
            }
            batch_ids[idx] = src_id;
            // position_map[src_id] = idx (Kernels.cu:92).  The reference assumes distinct seeds (:67); with
            // duplicates (link-prediction triples) its serial order lets the LAST occurrence win, so do the
            // same deterministically: the largest idx of the running epoch survives.
            const pos_t mine = pos_entry(epoch, (uint32_t)idx);
            pos_t cur = pos_map[src_id];
            while ((uint32_t)(cur >> kPosShift) != epoch || cur < mine) {
                const pos_t seen = atomicCAS(pos_map + src_id, cur, mine);
                if (seen == cur) break;
                cur = seen;
            }
            if constexpr (LP) labels[idx] = label;
            else labels[idx] = all_labels[g % total_cap];
        }
    }
    if (idx < LEGION_COUNTER_WORDS) { // cudaMemsetAsync(counters) + update_counter(op 0), Kernels.cu:220-221,118-127
        constexpr int seeds = legion_idx_level_size(0);
        int32_t nv = 0;
        if (idx == LEGION_NC_TOTAL || idx == LEGION_NC_NEXT_INPUTS || idx == seeds) nv = size;
        nc[idx] = nv;
        ec[idx] = 0;
    }
    // slot states of hop 1 start as "claim pending" (-1), see k_sample
    const int64_t n_init = min((int64_t)max(size, 0) * f_next, (int64_t)aux_cap);
    for (int64_t i = idx; i < n_init; i += (int64_t)gridDim.x * blockDim.x) aux_next[i] = -1;
}
// fallback when a hop's fan-out differs from what the previous launch prepared the slot states for
__global__ void k_fill_aux(const int32_t* __restrict__ nc, int32_t count, int32_t* __restrict__ aux, int32_t aux_cap)
{
    const int64_t n = min((int64_t)nc[LEGION_NC_NEXT_INPUTS] * count, (int64_t)aux_cap);
    for (int64_t i = threadIdx.x + (int64_t)blockDim.x * blockIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) aux[i] = -1;
}
__global__ void k_set_cursor(BatchCtl* ctl, int32_t counter, uint32_t epoch, uint32_t seeded, uint32_t draw_key)
{
    ctl->counter = counter; ctl->epoch = epoch;
    ctl->draw = seeded_draw_word(seeded, draw_key, counter); ctl->seeded = seeded; ctl->draw_key = draw_key;
}
// end of a captured batch: next batch, next (smaller) epoch, the next batch's draw word
__global__ void k_advance(BatchCtl* ctl)
{
    const int32_t counter = ctl->counter + 1;
    ctl->counter = counter; ctl->epoch -= 1;
    ctl->draw = seeded_draw_word(ctl->seeded, ctl->draw_key, counter);
}

// Seeded sampling: the round's shuffled copy of a training list, one thread per list index.  k_seed reads the copy exactly as it reads the
// file-order list; the cycle walk of seeded_perm runs here, once per epoch, and nowhere else.
__global__ __launch_bounds__(kBlock) void k_shuffle_seeds(const int32_t* __restrict__ ids, const int32_t* __restrict__ labels, int32_t n, uint32_t ks,
                                                          int32_t* __restrict__ out_ids, int32_t* __restrict__ out_labels)
{
    const int32_t g = threadIdx.x + blockDim.x * blockIdx.x;
    if (g >= n) return;
    const uint32_t p = seeded_perm((uint32_t)g, (uint32_t)n, ks);   // < n
    out_ids[g] = ids[p];
    out_labels[g] = labels[p];
}

// Drawn link-prediction thirds: the round's copy of a [src | pos | neg] list of batches of 3 k, one thread per list index.  Triple t =
// b k + i (batch b, slot i) takes the place of triple perm(t) on [0, n / 3): a triple moves as a whole, each third to its own third.
__global__ __launch_bounds__(kBlock) void k_shuffle_triples(const int32_t* __restrict__ ids, const int32_t* __restrict__ labels, int32_t n, int32_t k, uint32_t ks,
                                                            int32_t* __restrict__ out_ids, int32_t* __restrict__ out_labels)
{
    const int32_t g = threadIdx.x + blockDim.x * blockIdx.x;
    if (g >= n) return;
    const int32_t b = g / (3 * k), r = g - b * 3 * k, q = r / k, i = r - q * k;
    const uint32_t t = seeded_perm((uint32_t)(b * k + i), (uint32_t)(n / 3), ks);   // < n / 3
    const int32_t from = (int32_t)(t / (uint32_t)k) * 3 * k + q * k + (int32_t)(t % (uint32_t)k);   // < n
    out_ids[g] = ids[from];
    out_labels[g] = labels[from];
}

// S7: ClearPosMap (Kernels.cu:750-756) has no kernel here: position-table entries carry the batch epoch
// in their upper 32 bits, so entries of older batches are simply stale (see the table format below).

// ------------------------------------------------------------------------------------------------
// S3: sampler, pass 1 -- draw + claim
// ------------------------------------------------------------------------------------------------
struct SampleArgs {
    CsrTables csr;
    const int32_t* sampled_ids;
    const int32_t* agg_src_ids;
    const int32_t* nc;
    const int32_t* ec;
    pos_t* pos_map;
    int32_t* cand;
    int32_t* aux;
    int32_t* tile_edge;
    // One word for two pointers no instantiation reads together (like the tables at the end, and for the same reason): the hotness counters
    // are read from RowSource::Presc only, the slot's column is stored under COLS only, and COLS is never instantiated with Presc.
    union {
        unsigned long long* edge_access_time;   // Presc only
        int32_t* cols;                          // COLS only (GPUMemoryPool_SetEdgeIds): cols[idx] = the column of slot idx's draw inside its row
    };
    const BatchCtl* ctl;       // table epoch of the running batch
    const uint32_t* pow_tab;   // pow_tab[m] = 48271^(m+1), m < kTile (a launch with a smaller tile reads its first TILE entries)
    uint32_t a_tile;           // 48271^TILE
    uint32_t a_step;           // 48271^(TILE * gridDim.x)
    FastDiv fdiv;              // / count
    int32_t count;
    int32_t op_id;
    int32_t window;            // lanes to look back for a repeated draw of the same row: min(count - 1, 8)
    int32_t prefilter_from_op; // first op_id whose claims are preceded by the pre-filter load (4: hop 2; hop 1 never)
    // One table per weighted rule, in one word: growing the struct would move the hidden kernel arguments behind it, and with them
    // one load of every instantiation.
    union {
        const AliasEntry* alias;   // Weighted only: the whole CSR's alias table, entry e beside csr.indices[e] (null under the other rules)
        const float* weights;      // the rules that read weights (WeightedDistinct, WeightedShared): the graph's retained edge weights, w[e] beside csr.indices[e]; the alias table is not read
    };
};

// One slot's probe + claim on the position table.  Returns the slot's state: -1 = claim pending / won, >= 0 = the neighbour's known final
// position, <= -2 = lost to slot -2 - x.
__device__ inline int32_t claim_slot(const SampleArgs& a, uint32_t epoch, int32_t dst, int32_t idx)
{
    // claim: lowest idx wins.  Entries of older batches have a larger epoch field, i.e. compare
    // greater: unseen.  A stale (larger) pre-filter read only costs a redundant atomic.
    const pos_t prov0 = pos_entry(epoch, kProvisional);
    const pos_t mine = prov0 | (pos_t)(uint32_t)idx;
    // (plain loads: a non-temporal hint on this pre-filter load costs +11 % of k_sample, on the neighbour load
    // nothing, profiles/r02_sampler_experiments.md)
    // hop 1: nearly every neighbour is new, so the pre-filter load would only add a dependent round trip in front
    // of the claim -- go straight to the atomic (it returns the exact entry either way)
    pos_t cur = (a.op_id < a.prefilter_from_op) ? ~(pos_t)0 : a.pos_map[dst];
    if (cur > mine) {
        const pos_t old = atomicMin(a.pos_map + dst, mine);
        if (old > mine) {
            // the table holds this slot's claim now.  If it replaced a claim of this hop (a larger
            // slot that got there first), that slot has lost for good: tell it who beat it.  Its own
            // thread left aux at -1 (pending) and never writes it again, so this is the only store.
            if ((uint32_t)(old >> kPosShift) == epoch) a.aux[(uint32_t)old & kPosValueMask] = -2 - idx;
            cur = mine;
        } else {
            cur = old; // a smaller entry arrived between the load and the atomic: exact value
        }
    }
    // final positions are only written by earlier launches: if we see one it is exact
    if (cur < prov0) return (int32_t)((uint32_t)cur & kPosValueMask);
    // a smaller claim of this hop is in the table: this slot has lost for good (claims only
    // decrease).  Point at that slot; if it loses later too, its own aux points further, and
    // k_write follows the chain to the winner.
    if (cur < mine) return -2 - (int32_t)((uint32_t)cur & kPosValueMask);
    return -1;
}

// An instantiation is k_sample<TILE, SRC, RULE, COLS>: where a row is read (RowSource), what a slot draws by (DrawRule), and whether the
// slot's column is handed on.  sample_variant_exists (internal.h) says which of them there are; the dispatch table behind the kernels is
// built from it.  Branches that belong to one rule test RULE; branches that several rules share test the rule's fact (kDrawRuleFacts).
// SRC, the row source.  Whole: indptr / indices of the whole CSR.  Presc (S3', a pre-sampling hop): the whole CSR, and every draw counts in
// edge_access_time[src], the topology hotness.  Fragments: the owner's fragment where the topology map names one (FindTopo fused), else the
// whole CSR; a fragment row is the whole row's copy in CSR order.  Not under a rule whose table lies beside the whole CSR (whole_csr).
// RULE, the draw rule:
//  Stream (the default, the reference's draws): the slot's position in its row comes from the minstd stream, x[s].
//  Distinct (GPUMemoryPool_SetSampleDistinct): the position comes from the row's distinct picks instead.  The hash is pure, so the workgroup
//   stages distinct_u of EVERY slot of the tile's rows (rows that straddle a tile edge included: both tiles compute the whole row) in LDS
//   beside the row descriptors (s_pick: every rule that stages picks has it, and the fan-out bound that goes with it), one lane per row of
//   degree > f resolves the row's picks in place, and after one more barrier every slot reads its own.  Everything behind the position is
//   the stream rule's code.
//  Weighted (GPUMemoryPool_SetSampling(pool, 2), INTEGRATION.md "Weighted sampling"), the alias rule: the slot draws a column of its row and
//   keeps the column's neighbour or takes the column's alias (Walker's method over the graph's alias table, k_build_alias).  Both hashes are
//   the slot's own, so nothing is staged beyond the row descriptors, and the alias entry and the column's neighbour are two loads off the
//   staged row start whose addresses do not depend on each other's result: the slot's dependent chain is as long as the stream rule's.
//   Whole CSR only: the table lies beside the whole CSR's indices, the fragments have none.  The one rule whose pick is not a column.
//  WeightedDistinct (GPUMemoryPool_SetWeightedDistinct on top of the weighted kind, INTEGRATION.md "Weighted sampling without replacement"):
//   the row's picks are its f eligible columns of smallest exponential key, staged in s_pick like the distinct rule's -- but one WAVE
//   resolves a row, its lanes striding over the row's retained weights (weighted_distinct_resolve, draws.h), since a single lane would walk
//   a hub's weights alone.  The row's staged degree becomes min(eligible columns, f); reads the weights, not the alias table; whole CSR only.
//  Shared (GPUMemoryPool_SetSharedDraws on top of the distinct kind, INTEGRATION.md "Shared-key sampling"): the row's picks are its f columns
//   of smallest NODE key, a hash of the neighbour's id and the batch's draw word alone, so rows that see the same neighbours pick the same
//   ones.  Staged in s_pick and read by the slots exactly like the distinct rule's; one WAVE resolves a row of degree > f, its lanes striding
//   over the row's ids (shared_resolve, draws.h).  The rule reads nothing but the row itself, through s_row[r]: every row source, no table.
//  WeightedShared (GPUMemoryPool_SetSharedDraws on top of the weighted kind with GPUMemoryPool_SetWeightedDistinct, INTEGRATION.md "Weighted
//   shared-key sampling"): WeightedDistinct with one difference, the uniform under a column's exponential key is the hash of the column's
//   NEIGHBOUR ID and the batch's draw word (weighted_distinct_resolve<true>: it loads the row's ids through s_row[r] beside its weights).
// COLS (GPUMemoryPool_SetEdgeIds, INTEGRATION.md "Edge ids"): the slot's column -- the position inside its row that the rule picked, the one
// place it is known -- is parked in cols[idx] beside cand[idx]; k_edge_ids turns it into the edge's position in the whole CSR.  A fragment
// row is the whole row's copy, so the column means the same there.  Not from Presc (a pre-sampling batch hands nothing over) and not under
// the alias rule (the draw may take the alias neighbour, whose id the table holds and whose column it does not).  COLS = false is the
// kernel as it was, instruction for instruction (profiles/edge_ids.md): `cols` is not read.
template <int TILE, RowSource SRC, DrawRule RULE, bool COLS = false>
__global__ __launch_bounds__(kBlock) void k_sample(SampleArgs a)
{
    static_assert(sample_variant_exists(SRC, RULE, COLS), "no such variant: internal.h says why (and cols shares edge_access_time's word with the pre-sampling counters)");
    __shared__ const int32_t* s_row[TILE + 2]; // pointer to the first neighbour of the staged row
    __shared__ int32_t s_deg[TILE + 2];
    __shared__ int32_t s_src[TILE + 2];
    __shared__ int32_t s_cnt[kBlock / 64];
    // the tile's rows hold at most TILE + 2 (f - 1) slots: the first row may begin f - 1 slots in front of the tile, the last end f - 1 behind it
    __shared__ int32_t s_pick[draw_rule_facts(RULE).stages_picks() ? TILE + 2 * kDistinctMaxFanout : 1];

    const int32_t N = a.nc[LEGION_NC_NEXT_INPUTS];
    const int32_t f = a.count;
    const int32_t total = N * f; // int32 like the reference (Kernels.cu:375)
    const int32_t* __restrict__ input = (a.op_id == 2) ? a.sampled_ids : a.agg_src_ids + a.ec[LEGION_EC_INPUT_OFF];
    const int32_t n_tiles = (total + TILE - 1) / TILE;
    const int tid = threadIdx.x;
    const uint32_t epoch = a.ctl->epoch;
    const uint32_t draw = a.ctl->draw;   // the batch's draw word (seeded sampling), same line as the epoch; 0 = mode off

    if ((int32_t)blockIdx.x >= n_tiles) return;

    // per-thread RNG state: x[s] = s_b * 48271^(tile*TILE + tid + 256*s + 1) (the distinct and the weighted mode draw from the hash: no stream)
    uint32_t x[TILE / kBlock];
    if constexpr (RULE == DrawRule::Stream) {
        // uniform per workgroup; the seeded stream is the unseeded one times the batch's s_b (1 with the mode off: mulmod31(b, 1) == b)
        uint32_t base = mulmod31(powmod31(a.a_tile, (uint64_t)blockIdx.x), seeded_stream_seed(draw));
#pragma unroll
        for (int s = 0; s < TILE / kBlock; s++) x[s] = mulmod31(base, a.pow_tab[tid + kBlock * s]);
    }

    for (int32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int32_t tile_start = tile * TILE;
        const int32_t tile_end = min(tile_start + TILE, total);
        const int32_t i0 = (int32_t)fdiv((uint32_t)tile_start, a.fdiv);
        const int32_t i_last = (int32_t)fdiv((uint32_t)(tile_end - 1), a.fdiv);
        const int32_t nrows = i_last - i0 + 1;

        // stage the row descriptors of this tile in LDS (one global fetch per source row)
        for (int32_t r = tid; r < nrows; r += kBlock) {
            const int32_t src = input[i0 + r];
            const int32_t* rowp = nullptr;
            int32_t deg = -1;
            if (src >= 0) {
                const int64_t* ip = a.csr.indptr + src;
                const int32_t* ix = a.csr.indices;
                int8_t owner = -1;
                if (SRC == RowSource::Fragments) owner = a.csr.topo_owner[src]; // FindTopo fused (GPUCache.cu:434-443)
                if (owner >= 0) {   // cached row: chunk tables of the owner's fragment (local HBM or xGMI peer)
                    const int32_t row = a.csr.topo_row[src];
                    ip = a.csr.frag_indptr[owner * a.csr.ip_nch + (row >> a.csr.row_shift)] + (row & ((1 << a.csr.row_shift) - 1));
                    const int64_t start = ip[0];
                    ix = a.csr.frag_indices[owner * a.csr.ix_nch + (int32_t)(start >> a.csr.edge_shift)];
                    rowp = ix + (start & ((1ll << a.csr.edge_shift) - 1));
                    deg = (int32_t)(ip[1] - start); // int32 truncation as in Kernels.cu:393,396
                } else {
                    const int64_t start = ip[0];
                    rowp = ix + start;
                    deg = (int32_t)(ip[1] - start);
                }
            }
            s_row[r] = rowp;
            s_deg[r] = deg;
            s_src[r] = src;
        }
        if constexpr (RULE == DrawRule::Distinct) {
            const uint32_t hop = (uint32_t)a.op_id >> 1;
            for (int32_t p = tid; p < nrows * f; p += kBlock) {
                const uint32_t rr = fdiv((uint32_t)p, a.fdiv);
                s_pick[p] = (int32_t)distinct_u(distinct_key((uint32_t)i0 + rr, hop, draw), (uint32_t)p - rr * (uint32_t)f);
            }
        }
        __syncthreads();
        if constexpr (RULE == DrawRule::Distinct) {
            for (int32_t r = tid; r < nrows; r += kBlock)
                if (s_deg[r] > f) distinct_resolve(s_pick + r * f, s_deg[r], f);
            __syncthreads();
        }
        if constexpr (RULE == DrawRule::Shared) {
            const uint32_t salt = shared_salt(draw);
            for (int32_t r = wave_id(); r < nrows; r += kBlock / 64) {   // one wave per row: r and everything read through it is wave-uniform
                const int32_t d = s_deg[r];
                if (d > f) shared_resolve(s_pick + r * f, s_row[r], d, f, salt);
            }
            __syncthreads();
        }
        if constexpr (draw_rule_facts(RULE).reads_weights) {
            const uint32_t hop = (uint32_t)a.op_id >> 1;
            for (int32_t r = wave_id(); r < nrows; r += kBlock / 64) {   // one wave per row: r and everything read through it is wave-uniform
                const int32_t d = s_deg[r];
                if (d <= 0) continue;
                int32_t got;
                if constexpr (RULE == DrawRule::WeightedShared) got = weighted_distinct_resolve<true>(s_pick + r * f, a.weights + (s_row[r] - a.csr.indices), s_row[r], d, f, weighted_shared_salt(draw));
                else got = weighted_distinct_resolve<false>(s_pick + r * f, a.weights + (s_row[r] - a.csr.indices), nullptr, d, f,
                                                            weighted_distinct_key((uint32_t)(i0 + r), hop, draw));
                if (lane_id() == 0) s_deg[r] = got;   // what the slot test below reads: min(eligible columns, f)
            }
            __syncthreads();
        }

        int32_t cnt = 0;
#pragma unroll
        for (int s = 0; s < TILE / kBlock; s++) {
            const int32_t idx = tile_start + tid + kBlock * s;
            int32_t dst = -1, known = -1, j = 0, r = 0;
            [[maybe_unused]] int32_t col = 0;
            if (idx < tile_end) {
                const uint32_t i = fdiv((uint32_t)idx, a.fdiv);
                j = idx - (int32_t)i * f;
                r = (int32_t)i - i0;
                const int32_t deg = s_deg[r];
                if (j < deg) { // deg == -1 for padded (-1) sources; Kernels.cu:385,399
                    if constexpr (COLS) {   // the rule's pick, named; the loads below are the ones of COLS = false
                        if constexpr (draw_rule_facts(RULE).reads_weights) col = s_pick[r * f + j];
                        else if constexpr (draw_rule_facts(RULE).stages_picks()) col = deg <= f ? j : s_pick[r * f + j];
                        else col = sample_index(x[s], deg);
                        dst = s_row[r][col];
                    }
                    else if constexpr (draw_rule_facts(RULE).reads_weights) dst = s_row[r][s_pick[r * f + j]];
                    else if constexpr (draw_rule_facts(RULE).stages_picks()) dst = s_row[r][deg <= f ? j : s_pick[r * f + j]];
                    else if constexpr (RULE == DrawRule::Weighted) {
                        const uint32_t key = weighted_key(i, (uint32_t)a.op_id >> 1, draw);
                        const int32_t* col = s_row[r] + weighted_column(key, (uint32_t)j, deg);
                        const AliasEntry e = a.alias[col - a.csr.indices];   // beside the neighbour load, not behind it
                        const int32_t own = *col;
                        dst = weighted_ub(key, (uint32_t)j) < e.thr ? own : e.alias_id;
                    }
                    else dst = s_row[r][sample_index(x[s], deg)];
                    if (dst < 0) dst = -1;
                }
            }
            // Draws are with replacement, so the f slots of a row repeat neighbours (f = 5 of ~14: every 7th
            // slot).  The slots of a row sit in adjacent lanes: a lane that finds its neighbour in an earlier
            // lane of the same row has lost to it for good -- no table probe, no claim, and k_mark skips it too.
            int32_t dup = 0;
            for (int d = 1; d <= a.window; d++) { // uniform trip count, executed by the whole wave
                const int32_t o = __shfl_up(dst, d);
                if (d <= j && d <= lane_id() && o == dst) dup = d; // keeps the earliest match: short chains
            }
            if (dst >= 0) {
                if (SRC == RowSource::Presc) atomicAdd(a.edge_access_time + s_src[r], 1ull); // Kernels.cu:525
                if (dup) known = -2 - (idx - dup);
                else known = claim_slot(a, epoch, dst, idx);
                cnt++;
            }
            if (idx < tile_end) {
                a.cand[idx] = dst;
                if constexpr (COLS) a.cols[idx] = col;   // read by k_edge_ids for a slot with a draw only
                // aux[idx] was initialised to -1 ("claim pending") by the previous launch.  A pending slot must not
                // store here: the slot that replaces its claim writes aux[idx] from another XCD, and two L2s
                // holding different dirty bytes for one address would be written back in no defined order.
                if (dst < 0) a.aux[idx] = 0;            // no edge: never read as an edge, not counted as a winner
                else if (known != -1) a.aux[idx] = known;
            }
        }
        // tile edge count
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
        if (lane_id() == 0) s_cnt[wave_id()] = cnt;
        __syncthreads();
        if (tid == 0) {
            int32_t t = 0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; w++) t += s_cnt[w];
            a.tile_edge[tile] = t;
        }
        if constexpr (RULE == DrawRule::Stream) {
#pragma unroll
            for (int s = 0; s < TILE / kBlock; s++) x[s] = mulmod31(x[s], a.a_step);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// S3 pass 2 -- rank the winners inside their tile, count new nodes per tile
// ------------------------------------------------------------------------------------------------
// A slot whose state is still -1 after k_sample kept its claim: it discovered a new node.  Its state becomes
// "winner, r-th new node of this tile" (enc_win): with the per-tile counts that is the node's final position,
// computable by ANY workgroup of k_write -- which is what lets k_write resolve the edges that lost their claim
// itself (round 1 needed a fourth launch per hop, k_resolve, for that).
constexpr int32_t kWinBase = 0x40000000;   // loser states are -2 - slot with slot < 2^30; winner ranks sit below them

__device__ inline int32_t enc_win(int32_t r) { return -2 - (kWinBase + r); }
__device__ inline bool is_win(int32_t v) { return v <= -2 - kWinBase; }
__device__ inline int32_t win_rank(int32_t v) { return -2 - v - kWinBase; }

// Tile prefixes without a scan launch and without every workgroup of k_write reading every tile count: k_mark gives each of its
// workgroups a CONTIGUOUS chunk of T = ceil(tiles / workgroups) tiles, so a workgroup knows the (edges, new nodes) counted in front of each of
// its tiles INSIDE its chunk (tile_pre) and the chunk's totals (chunk_tot); k_write scans the <= kMaxChunks chunk totals in LDS (8-16 KB of
// shared reads per workgroup instead of every tile count: 35-70 KB at 4-9 k tiles, re-read by all 1536 workgroups at once -- one such prefix
// build cost 6.8 / 16.3 us per launch at the papers100M / products hop 3, profiles/r04_sampler.md) and adds tile_pre[t] of any tile it needs.
// kMaxChunks (internal.h) >= the largest k_mark grid (256 CUs x 8 workgroups); GPUMemoryPool_AllocateScratch sizes chunk_tot with it.
template <int TILE>
__global__ __launch_bounds__(kBlock) void k_mark(const int32_t* __restrict__ nc, const int32_t* __restrict__ ec,
                                                 int32_t count, int32_t* __restrict__ aux, const int32_t* __restrict__ tile_edge,
                                                 int32_t* __restrict__ tile_node, int2* __restrict__ tile_pre,
                                                 int2* __restrict__ chunk_tot, HopState* __restrict__ hs)
{
    constexpr int S = TILE / kBlock, W = kBlock / 64;
    __shared__ int32_t s_c[S * W];
    const int32_t total = nc[LEGION_NC_NEXT_INPUTS] * count;
    const int32_t n_tiles = (total + TILE - 1) / TILE;
    const int lane = lane_id(), wave = wave_id();
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // hop-start snapshot of the counters: k_write's last tile applies update_counter in place, so
        // its other workgroups must not read the live nc/ec
        HopState h;
        h.edge_base = ec[LEGION_EC_TOTAL]; h.node_base = nc[LEGION_NC_TOTAL]; h.n_edges = 0; h.n_nodes = 0;
        h.in_off = ec[LEGION_EC_INPUT_OFF]; h.n_in = nc[LEGION_NC_NEXT_INPUTS]; h.slots = total; h.pad = 0;
        *hs = h;
    }
    const int32_t T = (n_tiles + (int32_t)gridDim.x - 1) / (int32_t)gridDim.x;     // tiles per chunk (k_write derives the same T)
    const int32_t t0 = (int32_t)blockIdx.x * T, t1 = min(t0 + T, n_tiles);
    if (t0 >= n_tiles) return;
    // the slot states of the NEXT tile of this workgroup are fetched before the current one is ranked: the loads overlap the
    // two barriers and the stores of the current tile (a workgroup runs 1-5 tiles; the pass is a chain of short latencies)
    int32_t nxt[S];
#pragma unroll
    for (int s = 0; s < S; s++) {
        const int64_t idx = (int64_t)t0 * TILE + threadIdx.x + kBlock * s;
        nxt[s] = idx < total ? aux[idx] : 0;
    }
    int32_t te_next = threadIdx.x == 0 ? tile_edge[t0] : 0, run_e = 0, run_n = 0;   // thread 0 keeps the chunk's running sums
    for (int32_t tile = t0; tile < t1; tile++) {
        bool win[S];
        int32_t rk[S];
        const int32_t te = te_next;
#pragma unroll
        for (int s = 0; s < S; s++) {
            const int32_t idx = tile * TILE + threadIdx.x + kBlock * s;
            win[s] = idx < total && nxt[s] == -1;
        }
        {
            const int64_t nt = (int64_t)tile + 1;
#pragma unroll
            for (int s = 0; s < S; s++) {
                const int64_t idx = nt * TILE + threadIdx.x + kBlock * s;
                nxt[s] = (nt < t1 && idx < total) ? aux[idx] : 0;
            }
            if (threadIdx.x == 0 && nt < t1) te_next = tile_edge[nt];
        }
#pragma unroll
        for (int s = 0; s < S; s++) {
            const unsigned long long b = __ballot(win[s]);
            rk[s] = __popcll(b & lt);
            if (lane == 0) s_c[s * W + wave] = __popcll(b);
        }
        __syncthreads();
        int32_t run = 0, before[S];
#pragma unroll
        for (int q = 0; q < S * W; q++) { // slot order inside a tile: s-major, then wave, then lane
#pragma unroll
            for (int s = 0; s < S; s++)
                if (q == s * W + wave) before[s] = run;
            run += s_c[q];
        }
#pragma unroll
        for (int s = 0; s < S; s++)
            if (win[s]) aux[tile * TILE + threadIdx.x + kBlock * s] = enc_win(before[s] + rk[s]);
        if (threadIdx.x == 0) {
            tile_node[tile] = run;
            tile_pre[tile] = make_int2(run_e, run_n);      // in front of this tile inside its chunk
            run_e += te; run_n += run;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) chunk_tot[blockIdx.x] = make_int2(run_e, run_n);
}

// ------------------------------------------------------------------------------------------------
// S2: update_counter (Kernels.cu:128-149) behind hop hh, which found level hh (legion_batch_layout.h draws the words)
// ------------------------------------------------------------------------------------------------
__device__ inline void apply_update_counter(int32_t* nc, int32_t* ec, int32_t op_id, int32_t hops, int32_t n_nodes,
                                            int32_t n_edges)
{
    const int32_t hh = op_id / 2;
    const int off = legion_idx_level_offset(hh), size = legion_idx_level_size(hh);
    nc[LEGION_NC_TOTAL] += n_nodes;
    // nodes through level hh - 1, whose words lie one pair in front (addressed from level hh's: k_write keeps one base address)
    nc[off] = nc[off - LEGION_LEVEL_WORDS] + nc[size - LEGION_LEVEL_WORDS];
    nc[size] = n_nodes;
    if (hh == hops) nc[legion_idx_nodes_through(hh)] = nc[off] + nc[size];
    nc[LEGION_NC_HOP_NEW] = 0;
    nc[LEGION_NC_NEXT_INPUTS] = n_edges;
    const int32_t before = hh == 1 ? hh : hh - 1;        // edges through hop hh - 1; hop 1 reads its own word, which k_seed zeroed
    ec[legion_idx_edges_through(hh)] = ec[legion_idx_edges_through(before)] + n_edges;
    ec[LEGION_EC_INPUT_OFF] = ec[LEGION_EC_TOTAL];
    ec[LEGION_EC_TOTAL] += n_edges;
    ec[LEGION_EC_HOP] = 0;
}

// ------------------------------------------------------------------------------------------------
// S3 pass 3 + S4 -- ordered compaction: edges, new nodes, both COO offsets; next hop's slot states
// ------------------------------------------------------------------------------------------------
struct WriteArgs {
    HopState* hs;
    int32_t* nc;
    int32_t* ec;
    int32_t hops;
    const int32_t* cand;
    const int32_t* aux;     // slot states after k_mark: >= 0 known position, winner rank (enc_win), -2 - <slot it lost to>
    const int32_t* tile_edge;
    const int32_t* tile_node;
    int32_t* sampled_ids;
    int32_t* agg_src_ids;
    int32_t* agg_src_off;
    int32_t* agg_dst_off;
    pos_t* pos_map;
    FastDiv fdiv;
    int32_t op_id;
    const BatchCtl* ctl;
    int32_t last_hop;       // positions of the nodes found in the last hop are never looked up through the table
    const int2* tile_pre;   // k_mark: (edges, new nodes) in front of a tile inside its chunk
    const int2* chunk_tot;  // k_mark: totals of chunk c = tiles [c * T, (c + 1) * T)
    int32_t mark_grid;      // workgroups of k_mark: T = ceil(tiles / mark_grid)
    int32_t* aux_next;      // slot states of the next hop (the other buffer), set to "claim pending" here
    int32_t next_count;     // fan-out of the next hop (0: none)
    int32_t aux_cap;
    int32_t ids_cap;        // elements of sampled_ids / agg_src_ids / agg_*_off (GPUMemoryPool::num_ids): bound of every store below
    int32_t V;              // entries of pos_map
};

// Every store of k_write is addressed through the tile prefix (s_chunk[] + tile_pre[]) that k_mark left behind.  With a correct
// k_mark the offsets are below the buffers' capacity by construction (num_ids = the sum of the static per-hop bounds); an experiment
// that skips or breaks the prefix build writes through uninitialised offsets -- round 4's timing-only variant did, and hung its run
// (profiles/r04_sampler.md).  The bound check makes such a variant drop the store instead of running away; it is one unsigned compare
// per store in a kernel that waits for memory (+0.3-0.6 us per launch: profiles/r05_sampler.md, r05_ab_bounded_stores.log).
// (LEGION_STORE_OK: draws.h, the normalised last hop's passes bound their stores the same way.)

template <int TILE>
__global__ __launch_bounds__(kBlock) void k_write(WriteArgs a)
{
    constexpr int S = TILE / kBlock, W = kBlock / 64;
    // (edges, new nodes) counted in front of a tile = exclusive prefix over the chunk totals of k_mark, built once per workgroup in
    // LDS (<= kMaxChunks entries: one coalesced round of loads), + tile_pre[t] (one 8-byte read, issued next to the other loads of
    // the tile or of the losing edge that needs it).  No scan launch, no inter-workgroup hand-off (device-scope fences cost an L2
    // write-back + invalidate per XCD: profiles/r01_gather_sweep.md).
    __shared__ int2 s_chunk[kMaxChunks];
    __shared__ int32_t s_e[S * W];
    __shared__ int2 s_scan[W];
    __shared__ uint32_t s_div_t[3];
    constexpr int PER = kMaxChunks / kBlock;                        // consecutive chunks per thread
    const int32_t q0 = (int32_t)threadIdx.x * PER;
    // The hop's size (hs->slots) is one round trip away and everything below is addressed through it.  What the workgroup's FIRST tile and
    // the chunk scan read does not need it: the addresses are inside their allocations whatever the hop's size (chunk_tot has kMaxChunks
    // entries; blockIdx.x < the tiles the per-tile scratch is sized for; slots are checked against aux_cap), so these loads go out beside
    // the one of hs and are masked once it is known: two dependent round trips less in front of the stores, -1.1 / -0.7 / -2.0 us at the
    // headline's hops.  (Hop 1's seed ids fetched here as well, in front of their pos_map probe: +-0 / +0.3 / +0.5 us, not kept --
    // profiles/narrow_hops.md.)
    int2 v[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) v[u] = a.chunk_tot[q0 + u];
    int32_t c[S], so[S];
#pragma unroll
    for (int s = 0; s < S; s++) {
        const int64_t idx = (int64_t)blockIdx.x * TILE + threadIdx.x + kBlock * s;
        c[s] = idx < a.aux_cap ? a.cand[idx] : -1;
        so[s] = idx < a.aux_cap ? a.aux[idx] : 0;
    }
    int2 own = a.tile_pre[blockIdx.x];
    int32_t tile_e = a.tile_edge[blockIdx.x];
    const HopState h = *a.hs;
    const uint32_t epoch = a.ctl->epoch;
    const int32_t total = h.slots;
    const int32_t n_tiles = (total + TILE - 1) / TILE;
    const int lane = lane_id(), wave = wave_id();
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (n_tiles == 0) { // empty hop: only the counters move
        if (blockIdx.x == 0 && threadIdx.x == 0) apply_update_counter(a.nc, a.ec, a.op_id, a.hops, 0, 0);
        return;
    }
    if ((int32_t)blockIdx.x >= n_tiles) return;
    const int32_t T = (n_tiles + a.mark_grid - 1) / a.mark_grid;   // tiles per chunk, as k_mark derived it
    if (threadIdx.x == 0) {                                        // one 64-bit divide per workgroup (T is device-side: no host round trip)
        const FastDiv f((uint32_t)T);
        s_div_t[0] = f.d; s_div_t[1] = f.m; s_div_t[2] = f.s;
    }
    const int32_t n_chunks = (n_tiles + T - 1) / T;                // <= mark_grid <= kMaxChunks
    {
        int32_t se = 0, sn = 0;
#pragma unroll
        for (int u = 0; u < PER; u++) {
            if (q0 + u >= n_chunks) v[u] = make_int2(0, 0);
            se += v[u].x; sn += v[u].y;
        }
        int32_t ie = se, in = sn;
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t ue = __shfl_up(ie, o), un = __shfl_up(in, o);
            if (lane >= o) { ie += ue; in += un; }
        }
        if (lane == 63) s_scan[wave] = make_int2(ie, in);
        __syncthreads();
        int32_t run_e = ie - se, run_n = in - sn;
#pragma unroll
        for (int w = 0; w < W; w++)
            if (w < wave) { run_e += s_scan[w].x; run_n += s_scan[w].y; }
#pragma unroll
        for (int u = 0; u < PER; u++) {
            if (q0 + u < n_chunks) s_chunk[q0 + u] = make_int2(run_e, run_n);
            run_e += v[u].x; run_n += v[u].y;
        }
        __syncthreads();
    }
    FastDiv div_t;
    div_t.d = s_div_t[0]; div_t.m = s_div_t[1]; div_t.s = s_div_t[2];
    // new nodes in front of tile t (what an edge that lost its claim needs of its winner's tile); `pre` = tile_pre[t]
    auto nodes_before = [&](int32_t t, int32_t pre_n_in_chunk) { return s_chunk[fdiv((uint32_t)t, div_t)].y + pre_n_in_chunk; };

    for (int32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const bool first = tile == (int32_t)blockIdx.x;   // its loads were issued at the top
        if (!first) { own = a.tile_pre[tile]; tile_e = a.tile_edge[tile]; }
        const int2 own_chunk = s_chunk[fdiv((uint32_t)tile, div_t)];
        const int32_t pre_e = own_chunk.x + own.x, pre_n = own_chunk.y + own.y;
        const int32_t ebase = h.edge_base + pre_e;
        const int32_t nbase = h.node_base + pre_n;
        // ---- loads first, all S slots of the thread in flight together (nothing below this block reads global memory) ----
        int32_t dpos[S], w[S], re[S], wpre[S];
        const int32_t* __restrict__ pre_n_of = reinterpret_cast<const int32_t*>(a.tile_pre) + 1;   // tile_pre[t].y at [2 * t]
#pragma unroll
        for (int s = 0; s < S; s++) {
            const int32_t idx = tile * TILE + threadIdx.x + kBlock * s;
            if (!first) {
                c[s] = (idx < total) ? a.cand[idx] : -1;
                so[s] = (idx < total) ? a.aux[idx] : 0;
            } else if (idx >= total) { c[s] = -1; so[s] = 0; }
        }
#pragma unroll
        for (int s = 0; s < S; s++) {
            dpos[s] = 0; w[s] = -1;
            if (c[s] == -1) continue;
            const int32_t idx = tile * TILE + threadIdx.x + kBlock * s;
            // dst-side offset = position of the slot's source node; for hops > 1 the sources are the
            // previous hop's edge endpoints, whose positions are that hop's src-side offsets: same value
            // as position_map[src] (construct_graph, Kernels.cu:457-461) without the random read.
            const int32_t i = (int32_t)fdiv((uint32_t)idx, a.fdiv);
            // hop 1: the seed's position.  That is i unless the seed list holds duplicates (link-prediction
            // triples), where the reference's position_map keeps the last occurrence -- read it (<= B*f probes).
            dpos[s] = (a.op_id == 2) ? (int32_t)((uint32_t)a.pos_map[a.sampled_ids[i]] & kPosValueMask) : a.agg_src_off[h.in_off + i];
            // lost the claim: first link of loser -> (earlier loser ->)* winner or known node
            // (with the in-chunk node prefix of that slot's tile, should it turn out to be the winner: same round trip)
            wpre[s] = 0;
            if (so[s] < -1 && !is_win(so[s])) { w[s] = -2 - so[s]; so[s] = a.aux[w[s]]; wpre[s] = pre_n_of[2 * (w[s] / TILE)]; }
        }
#pragma unroll
        for (int s = 0; s < S; s++) // longer chains are rare: follow them one slot at a time
            while (w[s] >= 0 && so[s] < -1 && !is_win(so[s])) { w[s] = -2 - so[s]; so[s] = a.aux[w[s]]; wpre[s] = pre_n_of[2 * (w[s] / TILE)]; }
#pragma unroll
        for (int s = 0; s < S; s++) {
            const unsigned long long be = __ballot(c[s] != -1);
            re[s] = __popcll(be & lt);
            if (lane == 0) s_e[s * W + wave] = __popcll(be);
        }
        __syncthreads();
        if (tile == n_tiles - 1 && threadIdx.x == 0) { // hop totals: update_counter (S2)
            const int32_t n_edges = pre_e + tile_e, n_nodes = pre_n + a.tile_node[tile];
            a.hs->n_edges = n_edges;
            a.hs->n_nodes = n_nodes;
            apply_update_counter(a.nc, a.ec, a.op_id, a.hops, n_nodes, n_edges);
        }
        // ---- stores ----
#pragma unroll
        for (int s = 0; s < S; s++) {
            if (c[s] == -1) continue;
            int32_t pe = 0;
            for (int q = 0; q < s * W + wave; q++) pe += s_e[q];
            const int32_t dst = c[s];
            const int32_t e = ebase + pe + re[s];
            if (!LEGION_STORE_OK(e, a.ids_cap)) continue;
            if (!a.last_hop) a.agg_src_ids[e] = dst;   // the next hop's input list; nothing reads it after the last hop
            a.agg_dst_off[e] = dpos[s];
            // src-side offset (construct_graph, Kernels.cu:456-460) = position of the sampled neighbour
            int32_t p = so[s];
            if (w[s] >= 0) {         // an edge that lost its claim
                if (p < -1)         // ... to a new node: the winner's position from ITS tile's prefix and its rank
                    p = h.node_base + nodes_before(w[s] / TILE, wpre[s]) + win_rank(p);
            } else if (is_win(p)) {  // this slot discovered the node: k_mark ranked it inside the tile
                p = nbase + win_rank(p);
                if (LEGION_STORE_OK(p, a.ids_cap)) a.sampled_ids[p] = dst;
                // the scattered table store is only needed when a later hop may look the node up by id
                if (!a.last_hop && LEGION_STORE_OK(dst, a.V)) a.pos_map[dst] = pos_entry(epoch, (uint32_t)p);
            }
            a.agg_src_off[e] = p;
        }
        // The next hop expands this tile's edges into slots [e * f', (e + 1) * f'): their states (the other aux
        // buffer, last read two launches ago) start as "claim pending"
        if (a.next_count > 0) {
            const int64_t lo = min((int64_t)pre_e * a.next_count, (int64_t)a.aux_cap);
            const int64_t hi = min((int64_t)(pre_e + tile_e) * a.next_count, (int64_t)a.aux_cap);
            for (int64_t q = lo + threadIdx.x; q < hi; q += kBlock) a.aux_next[q] = -1;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// Edge ids (GPUMemoryPool_SetEdgeIds): slot -> edge, once more, behind k_write
// ------------------------------------------------------------------------------------------------
// edge_ids[e] = indptr[src] + cols[slot] for the COO edge e that k_write made of `slot`: one edge per slot with a draw (cand != -1), in
// ascending slot order, behind the edges of the earlier hops.  The prefix is re-derived from what k_mark left, as k_write derives it and as
// k_draw_weights (gather.hip) re-derives the last hop's: the <= kMaxChunks chunk totals scanned per workgroup in LDS, tile_pre[tile] on
// top, wave ballots and popcount prefixes inside the tile -- no scan launch, no device-scope hand-off, no per-element atomic.  The launch
// sits on the sampler stream directly behind the hop's k_write, in front of the next hop: cand (cand_pipe on an aggregated last hop), cols,
// tile_pre, chunk_tot and hop_state are still this hop's.  The live counters are NOT: k_write's last tile applied update_counter, so the
// hop's sizes and offsets come from the snapshot in hop_state.  indptr is the WHOLE CSR's, whatever the hop drew from.  Nothing here
// depends on what edge_ids / edge_w held: every edge of the hop is stored, nothing else is.
struct EdgeIdArgs {
    const HopState* hs;
    const int32_t* cand;
    const int32_t* cols;
    const int2* tile_pre;
    const int2* chunk_tot;
    const int32_t* sampled_ids;
    const int32_t* agg_src_ids;
    const int64_t* indptr;     // whole CSR
    const float* weights;      // WEIGHTS only: the graph's retained weights, w[e] beside indices[e]
    int64_t* edge_ids;
    float* edge_w;             // WEIGHTS only
    int64_t E;                 // entries of the whole CSR: bound of the weight probe
    FastDiv fdiv;              // / fan-out
    int32_t op_id;
    int32_t mark_grid;         // workgroups of the hop's k_mark: T = ceil(tiles / mark_grid)
    int32_t slots_cap;         // elements of cand / cols
    int32_t ids_cap;           // elements of edge_ids / edge_w, sampled_ids and agg_src_ids
};

template <int TILE, bool WEIGHTS>
__global__ __launch_bounds__(kBlock) void k_edge_ids(EdgeIdArgs a)
{
    constexpr int S = TILE / kBlock, W = kBlock / 64, PER = kMaxChunks / kBlock;
    __shared__ int32_t s_chunk[kMaxChunks];   // edges in front of chunk c of the hop
    __shared__ int32_t s_scan[W];
    __shared__ int32_t s_e[S * W];
    const int lane = lane_id(), wave = wave_id();
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int32_t q0 = (int32_t)threadIdx.x * PER;
    int32_t v[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) v[u] = a.chunk_tot[q0 + u].x;   // kMaxChunks entries are allocated; masked below
    const HopState h = *a.hs;
    const int32_t total = min(h.slots, a.slots_cap);
    const int32_t n_tiles = (total + TILE - 1) / TILE;
    if ((int32_t)blockIdx.x >= n_tiles) return;
    const int32_t T = (n_tiles + a.mark_grid - 1) / a.mark_grid;   // tiles per chunk, as k_mark derived it
    const int32_t n_chunks = (n_tiles + T - 1) / T;                // <= mark_grid <= kMaxChunks
    {
        int32_t se = 0;
#pragma unroll
        for (int u = 0; u < PER; u++) {
            if (q0 + u >= n_chunks) v[u] = 0;
            se += v[u];
        }
        int32_t ie = se;
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t ue = __shfl_up(ie, o);
            if (lane >= o) ie += ue;
        }
        if (lane == 63) s_scan[wave] = ie;
        __syncthreads();
        int32_t run = ie - se;
#pragma unroll
        for (int w = 0; w < W; w++)
            if (w < wave) run += s_scan[w];
#pragma unroll
        for (int u = 0; u < PER; u++) {
            if (q0 + u < n_chunks) s_chunk[q0 + u] = run;
            run += v[u];
        }
        __syncthreads();
    }
    const int32_t* __restrict__ input = (a.op_id == 2) ? a.sampled_ids : a.agg_src_ids + h.in_off;
    for (int32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int32_t ebase = h.edge_base + s_chunk[tile / T] + a.tile_pre[tile].x;
        int32_t col[S], src[S], re[S];
        bool draw[S];
#pragma unroll
        for (int s = 0; s < S; s++) {
            const int32_t idx = tile * TILE + threadIdx.x + kBlock * s;
            draw[s] = idx < total && a.cand[idx] != -1;
            col[s] = 0; src[s] = -1;
            if (draw[s]) {
                col[s] = a.cols[idx];
                const int32_t i = (int32_t)fdiv((uint32_t)idx, a.fdiv);
                if (i < h.n_in && LEGION_STORE_OK((a.op_id == 2 ? 0 : h.in_off) + i, a.ids_cap)) src[s] = input[i];
            }
        }
#pragma unroll
        for (int s = 0; s < S; s++) {
            const unsigned long long be = __ballot(draw[s]);
            re[s] = __popcll(be & lt);
            if (lane == 0) s_e[s * W + wave] = __popcll(be);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < S; s++) {
            if (!draw[s] || src[s] < 0) continue;
            int32_t pe = 0;
            for (int q = 0; q < s * W + wave; q++) pe += s_e[q];   // slot order inside a tile: s-major, then wave, then lane
            const int32_t e = ebase + pe + re[s];
            if (!LEGION_STORE_OK(e, a.ids_cap)) continue;
            const int64_t eid = a.indptr[src[s]] + col[s];
            a.edge_ids[e] = eid;
            if constexpr (WEIGHTS) a.edge_w[e] = (unsigned long long)eid < (unsigned long long)a.E ? a.weights[eid] : 0.0f;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// host side: launch wrappers
// ------------------------------------------------------------------------------------------------
// compute units of the current device, asked once per process (launch.h's grid_for sizes every grid by it)
int sampler_cu_count()
{
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess)
            cus = p.multiProcessorCount;
        if (cus <= 0) cus = 256;
    }
    return cus;
}

// 48271^(m+1) table for m < kTile, one copy per physical device
static uint32_t* pow_table()
{
    static uint32_t* tabs[64] = {nullptr};
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    if (!tabs[dev]) {
        std::vector<uint32_t> h(kTile);
        uint32_t x = 1;
        for (int m = 0; m < kTile; m++) { x = mulmod31(x, kA); h[m] = x; }
        HIP_CHECK(hipMalloc(&tabs[dev], kTile * sizeof(uint32_t)));
        HIP_CHECK(hipMemcpy(tabs[dev], h.data(), kTile * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    LEGION_AUDIT_SHARE(tabs[dev], current_logical_device());   // one table per PHYSICAL device, whichever logical GPUs map to it
    return tabs[dev];
}

void launch_seed(hipStream_t s, const SeedArgs& a, bool self_driven)
{
    const int32_t bound = self_driven ? a.batch_size : a.size;
    int blocks = bound > 0 ? (bound - 1) / kBlock + 1 : 1;
    // the audit names an argument by its expression: the pointers under k_seed's parameter names
    int32_t *batch_ids = a.batch_ids, *labels = a.labels, *nc = a.nc, *ec = a.ec, *aux_next = a.aux_next;
    const int32_t *all_ids = a.all_ids, *all_labels = a.all_labels;
    pos_t* pos_map = a.pos_map; BatchCtl* ctl = a.ctl;
    LEGION_AUDIT_LAUNCH(s, "k_seed", LEGION_AW(batch_ids), LEGION_AW(labels), LEGION_AW(pos_map), LEGION_AW(ctl), LEGION_AW(nc), LEGION_AW(ec), LEGION_AW(aux_next), LEGION_AL(all_ids), LEGION_AL(all_labels));
    const LpDrawArgs lp = a.lp ? *a.lp : LpDrawArgs{};
    auto* k = a.lp ? (self_driven ? k_seed<true, true> : k_seed<false, true>) : (self_driven ? k_seed<true, false> : k_seed<false, false>);
    k<<<blocks, kBlock, 0, s>>>(batch_ids, labels, a.batch_size, a.size, a.counter, all_ids, all_labels, a.total_cap, pos_map, a.epoch, ctl, nc, ec, aux_next, a.f_next, a.aux_cap, a.seeded, a.draw_key, lp);
    HIP_CHECK_LAST();
}
void launch_set_cursor(hipStream_t s, BatchCtl* ctl, int32_t counter, uint32_t epoch, uint32_t seeded, uint32_t draw_key)
{
    LEGION_AUDIT_LAUNCH(s, "k_set_cursor", LEGION_AW(ctl));
    k_set_cursor<<<1, 1, 0, s>>>(ctl, counter, epoch, seeded, draw_key);
    HIP_CHECK_LAST();
}
void launch_shuffle_seeds(hipStream_t s, const int32_t* ids, const int32_t* labels, int32_t n, uint32_t ks, int32_t* out_ids, int32_t* out_labels)
{
    if (n <= 0) return;
    LEGION_AUDIT_LAUNCH(s, "k_shuffle_seeds", LEGION_AW(out_ids), LEGION_AW(out_labels), LEGION_AL(ids), LEGION_AL(labels));
    k_shuffle_seeds<<<(n + kBlock - 1) / kBlock, kBlock, 0, s>>>(ids, labels, n, ks, out_ids, out_labels);
    HIP_CHECK_LAST();
}
void launch_shuffle_triples(hipStream_t s, const int32_t* ids, const int32_t* labels, int32_t n, int32_t k, uint32_t ks, int32_t* out_ids, int32_t* out_labels)
{
    if (n <= 0 || k <= 0 || n % (3 * k) != 0) return;   // the callers refuse such a list by name
    LEGION_AUDIT_LAUNCH(s, "k_shuffle_triples", LEGION_AW(out_ids), LEGION_AW(out_labels), LEGION_AL(ids), LEGION_AL(labels));
    k_shuffle_triples<<<(n + kBlock - 1) / kBlock, kBlock, 0, s>>>(ids, labels, n, k, ks, out_ids, out_labels);
    HIP_CHECK_LAST();
}
void launch_advance(hipStream_t s, BatchCtl* ctl)
{
    LEGION_AUDIT_LAUNCH(s, "k_advance", LEGION_AW(ctl));
    k_advance<<<1, 1, 0, s>>>(ctl);
    HIP_CHECK_LAST();
}
void warm_static_tables() { (void)pow_table(); (void)sampler_cu_count(); }

// The k_sample instantiations of a tile, by (row source, rule, columns): entry sample_variant_index(..) is the variant where
// sample_variant_exists says there is one -- taking its address here is what instantiates it -- and null where there is none.
constexpr int sample_variant_index(RowSource src, DrawRule rule, bool cols) { return ((int)src * kDrawRules + (int)rule) * 2 + (cols ? 1 : 0); }
template <int TILE, RowSource SRC, DrawRule RULE, bool COLS>
constexpr auto sample_variant() -> void (*)(SampleArgs)
{
    if constexpr (sample_variant_exists(SRC, RULE, COLS)) return k_sample<TILE, SRC, RULE, COLS>;
    else return nullptr;
}
template <int TILE, int... I>
constexpr std::array<void (*)(SampleArgs), sizeof...(I)> sample_variants(std::integer_sequence<int, I...>) { return {{sample_variant<TILE, (RowSource)(I / 2 / kDrawRules), (DrawRule)(I / 2 % kDrawRules), I % 2 != 0>()...}}; }

template <int TILE>
static void launch_sample_hop_t(hipStream_t s, const CsrTables& csr, const SamplerBuffers& b, int32_t count, int32_t op_id,
                       int32_t hops, int32_t slots_bound, RowSource src, const DrawTables& draw, const EdgeIdOut* eo)
{
    const int max_tiles = (slots_bound + TILE - 1) / TILE;
    // Workgroups per CU of the persistent tile loops.  The memory system is saturated by the scattered probes long before the CUs
    // are full: 4 workgroups (16 waves) per CU beat 8 by 2-4 % on hop 3 at every shape and tie on the small hops; 3 lose on hop 2
    // (same-box sweep, profiles/r04_sampler.md).
    // The narrow hops are the opposite case, chains of dependent round trips walked by too few waves: one tile per workgroup as far as
    // the k_mark chunk table allows (8 per CU; running hop 2 of the headline narrow at 4 or 8 per CU lost: profiles/narrow_hops.md).
    constexpr int wg_per_cu = TILE == kTile ? 4 : 8;
    const int grid = std::min(grid_for(max_tiles, 1, wg_per_cu), kMaxChunks);   // one chunk of tiles per k_mark workgroup (see k_mark)
    if (!b.aux_prepared) { // the previous launch prepared the slot states for another fan-out (or there was none)
        LEGION_AUDIT_LAUNCH(s, "k_fill_aux", LEGION_AW(b.aux), LEGION_AL(b.nc));
        k_fill_aux<<<grid_for(slots_bound, kBlock * 4), kBlock, 0, s>>>(b.nc, count, b.aux, b.aux_cap);
        HIP_CHECK_LAST();
    }
    SampleArgs a;
    a.csr = csr;
    a.sampled_ids = b.sampled_ids; a.agg_src_ids = b.agg_src_ids; a.nc = b.nc; a.ec = b.ec;
    a.pos_map = b.pos_map; a.cand = b.cand; a.aux = b.aux; a.tile_edge = b.tile_edge;
    if (eo) a.cols = eo->cols;   // no columns from a pre-sampling hop (sample_variant_exists): the word is free
    else a.edge_access_time = b.edge_access_time;
    a.ctl = b.ctl;
    a.pow_tab = pow_table();
    a.a_tile = powmod31(kA, TILE);
    a.a_step = powmod31(kA, (uint64_t)TILE * (uint64_t)grid);
    a.fdiv = FastDiv((uint32_t)count);
    a.count = count; a.op_id = op_id;
    a.window = std::min(count - 1, 8);
    a.prefilter_from_op = 4;   // hop 1 goes straight to the atomic (see k_sample; moving the boundary lost: profiles/r04_sampler.md)
    if (draw_rule_facts(draw.rule).reads_weights) a.weights = draw.weights;
    else a.alias = draw.rule == DrawRule::Weighted ? draw.alias : nullptr;
    // the whole CSR may be a peer's / the host's table; the fragment chunk tables, the id -> (owner, row) maps and every buffer of the pool are this GPU's
    LEGION_AUDIT_LAUNCH(s, "k_sample", LEGION_AW(a.pos_map), LEGION_AW(a.cand), LEGION_AW(a.aux), LEGION_AW(a.tile_edge), LEGION_AW(a.edge_access_time), LEGION_AL(a.sampled_ids), LEGION_AL(a.agg_src_ids), LEGION_AL(a.nc), LEGION_AL(a.ec), LEGION_AL(a.ctl), LEGION_AL(a.pow_tab), LEGION_AL(csr.frag_indptr), LEGION_AL(csr.frag_indices), LEGION_AL(csr.topo_owner), LEGION_AL(csr.topo_row), LEGION_AR(csr.indptr), LEGION_AR(csr.indices), LEGION_AL(a.alias));
    static constexpr auto variants = sample_variants<TILE>(std::make_integer_sequence<int, kRowSources * kDrawRules * 2>());
    variants[sample_variant_index(src, draw.rule, eo != nullptr)]<<<grid, kBlock, 0, s>>>(a);   // launch_sample_hop saw that it exists
    HIP_CHECK_LAST();
    LEGION_AUDIT_LAUNCH(s, "k_mark", LEGION_AW(b.aux), LEGION_AW(b.tile_node), LEGION_AW(b.tile_pre), LEGION_AW(b.chunk_tot), LEGION_AW(b.hop_state), LEGION_AL(b.nc), LEGION_AL(b.ec), LEGION_AL(b.tile_edge));
    k_mark<TILE><<<grid, kBlock, 0, s>>>(b.nc, b.ec, count, b.aux, b.tile_edge, b.tile_node, b.tile_pre, b.chunk_tot, b.hop_state);
    HIP_CHECK_LAST();
    WriteArgs w;
    w.hs = b.hop_state; w.nc = b.nc; w.ec = b.ec; w.hops = hops; w.cand = b.cand; w.aux = b.aux; w.ctl = b.ctl; w.tile_edge = b.tile_edge; w.tile_node = b.tile_node;
    w.sampled_ids = b.sampled_ids; w.agg_src_ids = b.agg_src_ids; w.agg_src_off = b.agg_src_off;
    w.agg_dst_off = b.agg_dst_off; w.pos_map = b.pos_map; w.fdiv = a.fdiv; w.op_id = op_id; w.last_hop = (op_id / 2 == hops) ? 1 : 0;
    w.aux_next = b.aux_next; w.next_count = b.next_count; w.aux_cap = b.aux_cap; w.ids_cap = b.ids_cap; w.V = b.V;
    w.tile_pre = b.tile_pre; w.chunk_tot = b.chunk_tot; w.mark_grid = grid;
    // 17 KB of static LDS (the chunk prefix): 8 workgroups per CU
    const int wgrid = grid_for(max_tiles, 1, 8);
    LEGION_AUDIT_LAUNCH(s, "k_write", LEGION_AW(w.hs), LEGION_AW(w.nc), LEGION_AW(w.ec), LEGION_AW(w.sampled_ids), LEGION_AW(w.agg_src_ids), LEGION_AW(w.agg_src_off), LEGION_AW(w.agg_dst_off), LEGION_AW(w.pos_map), LEGION_AW(w.aux_next), LEGION_AL(w.cand), LEGION_AL(w.aux), LEGION_AL(w.tile_edge), LEGION_AL(w.tile_node), LEGION_AL(w.tile_pre), LEGION_AL(w.chunk_tot), LEGION_AL(w.ctl));
    k_write<TILE><<<wgrid, kBlock, 0, s>>>(w);
    HIP_CHECK_LAST();
    if (!eo) return;
    EdgeIdArgs e;
    e.hs = b.hop_state; e.cand = b.cand; e.cols = eo->cols; e.tile_pre = b.tile_pre; e.chunk_tot = b.chunk_tot;
    e.sampled_ids = b.sampled_ids; e.agg_src_ids = b.agg_src_ids; e.indptr = eo->indptr; e.weights = eo->weights;
    e.edge_ids = eo->edge_ids; e.edge_w = eo->edge_w; e.E = eo->E; e.fdiv = a.fdiv; e.op_id = op_id; e.mark_grid = grid;
    e.slots_cap = std::min(slots_bound, b.aux_cap); e.ids_cap = b.ids_cap;
    // the whole CSR's indptr may be a peer's / the host's table, the weights are this GPU's copy; 8 KB of static LDS: the grid of k_write
    LEGION_AUDIT_LAUNCH(s, "k_edge_ids", LEGION_AW(e.edge_ids), LEGION_AW(e.edge_w), LEGION_AL(e.hs), LEGION_AL(e.cand), LEGION_AL(e.cols), LEGION_AL(e.tile_pre), LEGION_AL(e.chunk_tot), LEGION_AL(e.sampled_ids), LEGION_AL(e.agg_src_ids), LEGION_AR(e.indptr), LEGION_AL(e.weights));
    if (e.weights && e.edge_w) k_edge_ids<TILE, true><<<wgrid, kBlock, 0, s>>>(e);
    else k_edge_ids<TILE, false><<<wgrid, kBlock, 0, s>>>(e);
    HIP_CHECK_LAST();
}

void launch_sample_hop(hipStream_t s, const CsrTables& csr, const SamplerBuffers& b, int32_t count, int32_t op_id,
                       int32_t hops, int32_t slots_bound, bool is_presc, const DrawTables& draw, const EdgeIdOut* eo)
{
    if (count <= 0 || slots_bound <= 0) { LEGION_ARG_ERROR("GPU_Random_Sampling: empty hop"); return; }
    const RowSource src = is_presc ? RowSource::Presc : csr.topo_owner ? RowSource::Fragments : RowSource::Whole;
    // what a caller of the C ABI can get wrong, in the order it always was refused in: edge ids (GPUMemoryPool_SetEdgeIds) under the rule whose
    // pick is no column, edge ids without the pool's buffers, a whole-CSR rule without its table (launchers.cpp resolved rule and tables from
    // the same modes: a kernel never receives a null table, nor fragments without one), a fan-out above the rule's bound
    if (eo && !draw_rule_facts(draw.rule).picks_column) { LEGION_ARG_ERROR("GPU_Random_Sampling: edge ids (GPUMemoryPool_SetEdgeIds) under weighted sampling with replacement (GPUMemoryPool_SetSampling(pool, 2) without GPUMemoryPool_SetWeightedDistinct): the alias table holds the alias neighbour's id, not its column"); return; }
    if (eo && (!eo->cols || !eo->edge_ids || !eo->indptr)) { LEGION_ARG_ERROR("GPU_Random_Sampling: edge ids (GPUMemoryPool_SetEdgeIds) without the pool's column and edge-id buffers"); return; }
    const void* table = draw_rule_facts(draw.rule).reads_weights ? (const void*)draw.weights : (const void*)draw.alias;
    if (draw_rule_facts(draw.rule).whole_csr && (!table || src == RowSource::Fragments)) { LEGION_ARG_ERROR("GPU_Random_Sampling: weighted sampling (GPUMemoryPool_SetSampling) draws from the whole CSR's alias table: the graph has none (GPUGraphStorage_SetEdgeWeights)"); return; }
    if (draw_rule_facts(draw.rule).max_fanout && count > draw_rule_facts(draw.rule).max_fanout) { LEGION_ARG_ERROR(draw_rule_facts(draw.rule).fanout_refusal); return; }
    // ... and what none of them can: the dispatch table has no kernel for the rest (GPU_Random_Sampling leaves eo null for a pre-sampling hop)
    if (!sample_variant_exists(src, draw.rule, eo != nullptr)) { LEGION_ARG_ERROR("launch_sample_hop: no k_sample variant for this row source, draw rule and column hand-over"); return; }
    // one tile size for the three passes of the hop, from its static slot bound (internal.h: kNarrowSlots)
    if (sampler_tile_of(slots_bound) == kTileNarrow) launch_sample_hop_t<kTileNarrow>(s, csr, b, count, op_id, hops, slots_bound, src, draw, eo);
    else launch_sample_hop_t<kTile>(s, csr, b, count, op_id, hops, slots_bound, src, draw, eo);
}

} // namespace legion
