"""What tests/test_gpu_deep_tiles.py and tests/test_deep_tiles_cpu.py share (a helper module, not collected by pytest): one weighted graph
of 600 000 nodes, a two-hop shape whose second hop has several tiles per workgroup in every launch of the sampler, and the arithmetic that
says so.

A sampler hop is k_sample, k_mark, k_write and, with edge ids on, k_edge_ids (launch_sample_hop_t, csrc/sampler.hip).  With G = the grid of
k_sample and k_mark, a hop of `tiles` tiles runs
  k_sample     tile, tile + G, tile + 2 G, ... per workgroup: the staged row descriptors and picks are rewritten per tile
  k_mark       a chunk of T = ceil(tiles / G) CONSECUTIVE tiles per workgroup: tile_pre is non-zero from a chunk's second tile on, and
               n_chunks = ceil(tiles / T) < G
  k_write,     tile, tile + 8 CUs, ... per workgroup: the reload path behind the first tile, s_chunk[tile / T], and the winner of a loser
  k_edge_ids   in another chunk
Every other shape of the suite outside the BASELINE-shape tests (the reference's rule only) has T == 1 and one tile per workgroup.  Here
batch 0's hop 2 has about 20 x CUs tiles (T = 6, two to three tiles per k_write workgroup, five to six per k_sample workgroup) and the
short last batch's about 6.7 x CUs (T = 2, one tile per k_write workgroup): regime() is that arithmetic, B follows the device's CU count.

The aggregated last hop's slot -> edge prefix (k_draw_weights, k_draw_edge_weights: csrc/gather.hip) runs over its own chunks of the same
slots: weight_chunks() is that arithmetic -- ten or eleven steps of 256 slots per workgroup in batch 0, four in the short batch, whose last
chunks are empty; every other shape of the suite has chunks of one step.

Every statement is eidref.run_batch (the alias rule, which hands no edge ids over: weightedref.run_batch); nothing here restates a rule."""
import numpy as np

import drawrulecases as D
import eidref
import weightedref

RULES = ("stream", "distinct", "weighted", "wdistinct", "shared", "wshared")
# how capi.Engine.run_batch is told the rule
ENGINE_ARGS = dict(eidref.ENGINE_ARGS, weighted=D.ENGINE_ARGS["weighted"])
COUNTERS = (0, 1)                                   # the first batch and the last, which is short (a third of a batch)

TILE = 1024                                         # kTile (csrc/internal.h): the slots of a tile of a hop above NARROW_SLOTS
NARROW_SLOTS = D.NARROW_SLOTS                       # kNarrowSlots (csrc/internal.h)
MAX_CHUNKS = 2048                                   # kMaxChunks (csrc/internal.h): the clamp of k_sample's and k_mark's grid
SAMPLE_WG_PER_CU = 4                                # wg_per_cu at the wide tile (launch_sample_hop_t, csrc/sampler.hip): k_sample's and k_mark's grid
WRITE_WG_PER_CU = 8                                 # grid_for(max_tiles, 1, 8) (launch_sample_hop_t, csrc/sampler.hip): k_write's and k_edge_ids' grid
ALIAS_HUB_DEGREE = 256                              # kAliasHubDegree (csrc/internal.h)
CUS = 256                                           # the MI355X's compute units: what the CPU test works the regimes out at

V, F = 600000, 4
FAN = [16, 16]
EMPTY, HUB, ALL_ZERO, HOLES = 0, 1, 2, 3            # rows made by hand: degree 0, 300, 30 with every weight 0, 40 with two -1 holes
HAND_MADE = (EMPTY, HUB, ALL_ZERO, HOLES)
HOLE_COLUMNS = (3, 33)
# The seed of the graph's random part.  The rules without replacement by weight are compared bit for bit only on rows whose cut is no near
# tie (wdistinctref: the f-th and the (f + 1)-th key within 2^-40); this seed leaves no such row in any batch the GPU test runs, which
# tests/test_deep_tiles_cpu.py asserts.  The first of 0, 1, 2, ... that does.
GRAPH_SEED = 0


def graph(seed=GRAPH_SEED):
    """dict(indptr, indices, w, labels, feats): 600 000 nodes of 16..48 random neighbours, so that every row fills the fan-out of 16 and the
    slot counts are nearly exact; rows 0..3 by hand; one entry in a hundred names a hand-made row, so that those rows are inputs of hop 2 all
    over its slot range; weights are 0 (one in ten) or 1..16."""
    rng = np.random.RandomState(7000 + seed)
    deg = rng.randint(16, 49, size=V)
    deg[:4] = [0, 300, 30, 40]
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    indices = rng.randint(0, V, size=E).astype(np.int32)
    to_hand_made = rng.rand(E) < 0.01
    indices[to_hand_made] = rng.randint(0, 4, size=int(to_hand_made.sum()))
    w = np.where(rng.rand(E) < 0.1, 0, rng.randint(1, 17, size=E)).astype(np.float32)
    w[indptr[ALL_ZERO]:indptr[ALL_ZERO + 1]] = 0.0
    for c in HOLE_COLUMNS:
        indices[indptr[HOLES] + c], w[indptr[HOLES] + c] = -1, 16.0
    labels = rng.randint(0, 9, size=V).astype(np.int32)
    feats = np.random.RandomState(1).rand(V, F).astype(np.float32)
    return dict(indptr=indptr, indices=indices, w=w, labels=labels, feats=feats)


def batch_size(cus=CUS):
    """5 x (8 x CUs) tiles of hop-2 slots, and a little: batch 0 is above 16 x CUs tiles with T = 6, the last batch (a third) between
    4 x CUs and 8 x CUs with T = 2.  20 500 at 256 CUs."""
    return (5 * WRITE_WG_PER_CU * cus * TILE) // (2 * FAN[0] * FAN[1]) + 20


def seed_list(cus=CUS):
    """B + B / 3 seeds: the hand-made rows first, the others random"""
    B = batch_size(cus)
    return np.concatenate([np.arange(4), np.random.RandomState(2).randint(0, V, size=B + B // 3 - 4)]).astype(np.int32)


def slots_bound(hop, cus=CUS):
    """the static slot bound of hop 1 or 2 (seeds x fan-outs so far): what launch_sample_hop sizes the hop's tile and grids by"""
    return batch_size(cus) * int(np.prod(FAN[:hop]))


def hop2_slots(res):
    """the slots of hop 2 of a batch (a statement's or the engine's): its inputs are hop 1's edges, ec[3]"""
    return int(res["ec"][3]) * FAN[1]


def regime(slots, cus, bound=None):
    """(tiles, T, n_chunks, tiles per k_write workgroup) of a wide-tile hop of `slots` slots whose static bound is `bound` slots (default:
    the hop is full), as launch_sample_hop_t, k_mark and k_write derive them; the last is the largest over the workgroups."""
    up = lambda a, b: -(-int(a) // int(b))
    assert slots > 0 and (bound is None or NARROW_SLOTS < bound >= slots)
    tiles = up(slots, TILE)
    max_tiles = tiles if bound is None else up(bound, TILE)
    grid = min(max_tiles, SAMPLE_WG_PER_CU * cus, MAX_CHUNKS)
    T = up(tiles, grid)
    return tiles, T, up(tiles, T), up(tiles, min(max_tiles, WRITE_WG_PER_CU * cus))


def assert_regimes(slots0, slots1, cus):
    """what the shape exists for, of batch 0's and the last batch's hop-2 slots on `cus` compute units"""
    bound = slots_bound(2, cus)
    assert slots_bound(1, cus) > NARROW_SLOTS                       # hop 1 runs the wide tile too
    tiles, T, n_chunks, per_write = regime(slots0, cus, bound)
    assert tiles > 16 * cus and T >= 3 and n_chunks <= MAX_CHUNKS and per_write >= 2, (tiles, T, n_chunks, per_write)
    tiles, T, n_chunks, per_write = regime(slots1, cus, bound)
    assert 4 * cus < tiles <= 8 * cus and T == 2 and n_chunks <= MAX_CHUNKS and per_write == 1, (tiles, T, n_chunks, per_write)


BLOCK = 256                                         # kBlock (csrc/internal.h): the slots a workgroup of the slot -> edge passes takes per step
WEIGHT_WG_PER_CU = 8                                # grid_for's default (csrc/launch.h): launch_agg_norm_weights' and launch_agg_edge_weights' grid


def weight_chunks(slots, bound, cus):
    """(chunk_len, non_empty_chunks, grid) of the slot -> edge prefix of an aggregated last hop of `slots` slots whose static bound is `bound`
    slots, as launch_agg_edge_weights / launch_agg_norm_weights (the grid: one workgroup per 256 slots of the bound, at most 8 per compute
    unit and kMaxChunks) and agg_norm_chunk_len (the slots over the grid, rounded up to 256) derive them (csrc/gather.hip).  A workgroup takes
    chunk_len / 256 steps of its loop; the chunks from non_empty_chunks on have lo == hi == slots."""
    up = lambda a, b: -(-int(a) // int(b))
    assert 0 < slots <= bound
    grid = min(MAX_CHUNKS, up(bound, BLOCK), WEIGHT_WG_PER_CU * cus)
    chunk_len = up(up(slots, grid), BLOCK) * BLOCK
    return chunk_len, up(slots, chunk_len), grid


def assert_weight_regimes(slots0, slots1, cus):
    """what the edge-weighted case of this shape exists for: in both batches a workgroup of k_draw_edge_weights takes at least two steps (the
    carry of the rank from one step to the next, the barrier behind a step), and the short batch leaves whole chunks empty"""
    bound = slots_bound(2, cus)
    for slots in (slots0, slots1):
        chunk_len, filled, grid = weight_chunks(slots, bound, cus)
        assert chunk_len >= 2 * BLOCK and 1 < filled <= grid, (slots, chunk_len, filled, grid)
    chunk_len, filled, grid = weight_chunks(slots1, bound, cus)
    assert filled < grid, (slots1, chunk_len, filled, grid)


def statement(g, rule, counter, alias=None, ties=None, cus=CUS):
    """The rule's batch `counter`, unseeded (draw word 0), at the batch size of `cus` compute units.  alias: (thr, alias_id), the graph's
    alias table, which the weighted rule reads; ties: a list that receives the near-tie rows of the rules without replacement by weight."""
    B, seeds = batch_size(cus), seed_list(cus)
    lab = g["labels"][seeds]
    if rule == "weighted":
        return weightedref.run_batch(weightedref.Table(g["indptr"], g["indices"], *alias), g["feats"], seeds, lab, B, counter, FAN)
    return eidref.run_batch(g, rule, seeds, lab, B, counter, FAN, ties=ties)
