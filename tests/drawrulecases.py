"""What tests/test_gpu_draw_rules.py and tests/test_draw_rules_cpu.py share (a helper module, not collected by pytest): one small weighted
graph, the two batch shapes that select the sampler's two tiles, and each draw rule's existing NumPy statement behind one signature.

The four rules are what `sampling` and `weighted_distinct` say together (DrawRule, csrc/internal.h): stream = the reference's draws with
replacement, distinct, weighted, wdistinct = weighted without replacement.  Every statement is distinctref.run_batch with the rule's
`draw`; nothing here restates a rule.  Where the rows are read is k_sample's other parameter (RowSource, csrc/internal.h): plain = Whole,
presc = Presc, partitioned = Fragments; a (rule, kind) pair below is k_sample<TILE, SRC, RULE> of either tile."""
import numpy as np

import distinctref
import seededref
import wdistinctref
import weightedref

RULES = ("stream", "distinct", "weighted", "wdistinct")
# how capi.Engine.run_batch is told the rule
ENGINE_ARGS = dict(stream=dict(sample="replace"), distinct=dict(sample="distinct"), weighted=dict(sample="weighted"),
                   wdistinct=dict(sample="weighted", weighted_distinct=True))
WHOLE_CSR_ONLY = ("weighted", "wdistinct")          # the rules whose table lies beside the whole CSR: no partitioned sampler
# (rule, where the rows are read): every combination of these rules that there is (sample_variant_exists), the k_sample<TILE, SRC, RULE> of one tile
COMBOS = [(r, k) for r in RULES for k in ("plain", "presc", "partitioned") if not (k == "partitioned" and r in WHOLE_CSR_ONLY)]

NARROW_SLOTS, MAX_FANOUT = 256 * 1024, 64           # kNarrowSlots, kDistinctMaxFanout (csrc/internal.h)
# tile -> (batch size, fan-outs): the smallest shapes that select each tile.  Wide: 4097 x 64 = 262 208 slots, the first batch size whose
# hop is above kNarrowSlots at the distinct rules' largest fan-out.
SHAPES = dict(narrow=(64, [5, 4]), wide=(4097, [64]))
assert all(B * f <= NARROW_SLOTS for B, f in [(64, 5), (64 * 5, 4)]) and 4096 * 64 == NARROW_SLOTS < 4097 * 64
COUNTERS = (0, 1)                                   # the first batch and the last, which is short

V, F = 3000, 4
EMPTY, LONG, ALL_ZERO, HUB, HOLES = 0, 1, 2, 3, 4   # rows made by hand: degree 0, 129 (> 64), 30 with every weight 0, 300, 40 with two -1 holes
# The seed of the graph's random part.  Weighted sampling without replacement is compared bit for bit only on rows whose cut is no near
# tie (wdistinctref: the f-th and the (f + 1)-th key within 2^-40); this seed leaves no such row in any batch the GPU test runs, which
# tests/test_draw_rules_cpu.py asserts.  Found by trying 0, 1, 2, ... in order.
GRAPH_SEED = 0


def graph(seed=GRAPH_SEED):
    """dict(indptr, indices, w, labels, feats): 3000 nodes of 0..70 random neighbours (multi-edges throughout), rows 0..4 by hand;
    weights are 0 (one in five) or 1..16."""
    rng = np.random.RandomState(1000 + seed)
    deg = rng.randint(0, 71, size=V)
    deg[:5] = [0, 129, 30, 300, 40]
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    indices = rng.randint(0, V, size=E).astype(np.int32)
    w = np.where(rng.rand(E) < 0.2, 0, rng.randint(1, 17, size=E)).astype(np.float32)
    w[indptr[ALL_ZERO]:indptr[ALL_ZERO + 1]] = 0.0
    for c in (3, 33):
        indices[indptr[HOLES] + c], w[indptr[HOLES] + c] = -1, 16.0
    labels = rng.randint(0, 9, size=V).astype(np.int32)
    feats = np.random.RandomState(1).rand(V, F).astype(np.float32)
    return dict(indptr=indptr, indices=indices, w=w, labels=labels, feats=feats)


def seed_list(tile):
    """B + B / 3 seeds: the hand-made rows first, the others random with repeats (the wide list is longer than the graph)."""
    B = SHAPES[tile][0]
    return np.concatenate([np.arange(5), np.random.RandomState(2).randint(0, V, size=B + B // 3 - 5)]).astype(np.int32)


def statement(g, rule, tile, counter, alias=None, ties=None):
    """The rule's batch `counter` of the tile's shape, unseeded (draw word 0).  alias: (thr, alias_id), the graph's alias table, which the
    weighted rule reads; ties: a list that receives wdistinct's near-tie rows."""
    B, fan = SHAPES[tile]
    seeds = seed_list(tile)
    lab = g["labels"][seeds]
    if rule == "weighted":
        return weightedref.run_batch(weightedref.Table(g["indptr"], g["indices"], *alias), g["feats"], seeds, lab, B, counter, fan)
    if rule == "wdistinct":
        return wdistinctref.run_batch(wdistinctref.Weights(g["indptr"], g["indices"], g["w"]), g["feats"], seeds, lab, B, counter, fan, ties=ties)
    draw = seededref.replace_positions(0) if rule == "stream" else distinctref.positions
    return distinctref.run_batch(g["indptr"], g["indices"], g["feats"], seeds, lab, B, counter, fan, draw=draw)
