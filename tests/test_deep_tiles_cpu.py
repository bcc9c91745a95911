"""What tests/test_gpu_deep_tiles.py relies on, proved without a device at 256 compute units (tests/deepcases.py): the near-tie cap of the
rules without replacement by weight is zero on its batches, its two batches lie in the two regimes it exists for (several tiles per
workgroup in k_sample, k_mark, k_write and k_edge_ids; T = 2 with one tile per k_write workgroup), and the statements really hold what
the kernels do differently there -- the hand-made rows as inputs of a workgroup's second or later tile, draws, new nodes and repeated
neighbours beyond k_write's first round of tiles, and losers whose winner lies in another k_mark chunk."""
import numpy as np
import pytest

import deepcases as X
import eidref as R


@pytest.fixture(scope="module")
def g():
    return X.graph()


@pytest.fixture(scope="module")
def batches(g):
    """every (rule that needs no device-built table, counter) once, with its near-tie rows"""
    out = {}
    for rule in R.RULES:
        for it in X.COUNTERS:
            ties = []
            out[(rule, it)] = (X.statement(g, rule, it, ties=ties), ties)
    return out


def test_the_graph_is_the_one_described(g):
    deg = np.diff(g["indptr"])
    row = lambda v: slice(int(g["indptr"][v]), int(g["indptr"][v + 1]))
    assert deg[:4].tolist() == [0, 300, 30, 40] and deg[X.HUB] > X.ALIAS_HUB_DEGREE and deg[X.HUB] > 64
    assert deg[4:].min() == 16 and deg[4:].max() == 48              # every other row fills the fan-out
    assert (g["w"][row(X.ALL_ZERO)] == 0).all()
    holes = np.nonzero(g["indices"][row(X.HOLES)] == -1)[0]
    assert holes.tolist() == list(X.HOLE_COLUMNS) and (g["w"][row(X.HOLES)][holes] == 16).all()
    assert (g["indices"] == -1).sum() == 2 and g["indices"].max() < X.V
    share = np.isin(g["indices"], X.HAND_MADE).mean()
    assert 0.009 < share < 0.011                                    # one entry in a hundred names a hand-made row
    seeds = X.seed_list()
    B = X.batch_size()
    assert B == 20500 and len(seeds) == B + B // 3 and seeds[:4].tolist() == [0, 1, 2, 3]


def test_no_near_tie_in_the_weighted_batches(batches):
    """the cap on near-tie rows is zero (deepcases.GRAPH_SEED)"""
    for rule in ("wdistinct", "wshared"):
        for it in X.COUNTERS:
            assert batches[(rule, it)][1] == [], (rule, it)


@pytest.mark.parametrize("rule", R.RULES)
def test_both_batches_lie_in_their_regime(batches, rule):
    X.assert_regimes(X.hop2_slots(batches[(rule, 0)][0]), X.hop2_slots(batches[(rule, 1)][0]), X.CUS)
    for it in X.COUNTERS:
        res = batches[(rule, it)][0]
        assert X.hop2_slots(res) == len(res["draws"][1])


def test_the_alias_rule_lies_in_the_same_regimes(g):
    """The alias rule's statement needs the table the device built.  Its slot counts do not: with replacement every slot of a seed whose
    weights do not all vanish draws a column, and only a draw of HOLES' two -1 entries is no edge -- so hop 1 has between 16 x (such seeds
    that are not HOLES) and 16 x (such seeds) edges, and regime() is monotonic in the slots."""
    seeds, B = X.seed_list(), X.batch_size()
    wsum = np.add.reduceat(np.append(g["w"], 0).astype(np.float64), g["indptr"][:-1])
    wsum[np.diff(g["indptr"]) == 0] = 0
    bounds = []
    for it in X.COUNTERS:
        mine = R.batch_seeds(seeds, B, it)
        live = wsum[mine] > 0
        bounds.append((int((live & (mine != X.HOLES)).sum()), int(live.sum())))
    for pick in (0, 1):
        X.assert_regimes(bounds[0][pick] * X.FAN[0] * X.FAN[1], bounds[1][pick] * X.FAN[0] * X.FAN[1], X.CUS)


def claims(res):
    """of hop 2: (slot, drawn id, first slot of hop 2 that drew the id, whether the id is a new node of hop 2), one entry per edge"""
    draws = res["draws"][1].astype(np.int64)
    slot = np.nonzero(draws >= 0)[0]
    ids = draws[slot]
    before = np.zeros(X.V, bool)
    before[res["ids"][:int(res["nc"][7])]] = True                   # nc[7]: the nodes through hop 1
    first = np.full(X.V, -1, np.int64)
    u, at = np.unique(ids, return_index=True)                       # slot is ascending: the first occurrence is the first slot
    first[u] = slot[at]
    return slot, ids, first[ids], ~before[ids]


@pytest.mark.parametrize("rule", R.RULES)
def test_the_statement_reaches_the_later_tiles(batches, rule):
    res = batches[(rule, 0)][0]
    f = X.FAN[1]
    tiles, T, n_chunks, per_write = X.regime(X.hop2_slots(res), X.CUS, X.slots_bound(2))
    inputs = res["draw_counts"][1][0]
    second_round = X.SAMPLE_WG_PER_CU * X.CUS * X.TILE              # the first slot of a k_sample workgroup's second tile
    for v in X.HAND_MADE:
        at = np.nonzero(inputs == v)[0] * f
        assert (at >= second_round).any(), v
    slot, ids, first, new = claims(res)
    assert len(slot) == int(res["ec"][4] - res["ec"][3])
    deep = slot // X.TILE >= X.WRITE_WG_PER_CU * X.CUS              # a k_write / k_edge_ids workgroup's second or later tile
    assert deep.any()                                               # draws
    assert (deep & new & (first == slot)).any()                     # new nodes
    assert (deep & (~new | (first < slot))).any()                   # repeated neighbours: known before the hop, or lost to an earlier slot
    lost = new & (first < slot)
    other_chunk = lost & (first // X.TILE // T != slot // X.TILE // T)
    assert other_chunk.sum() > 0                                    # nodes_before(w / TILE, wpre) through another chunk's s_chunk entry
    assert (lost & ~other_chunk & (first // X.TILE != slot // X.TILE)).any()   # ... and through tile_pre inside the loser's own chunk
    # the new nodes of hop 2, in the order of their first slots, are the batch's ids behind hop 1's
    won = new & (first == slot)
    assert np.array_equal(ids[won], res["ids"][int(res["nc"][7]):])


def test_the_edge_weighted_prefix_takes_several_steps_per_chunk(batches):
    """k_draw_edge_weights at 256 compute units (tests/test_gpu_deep_tiles.py::test_edge_weighted_last_hop_over_five_million_slots): the grid is
    min(kMaxChunks, ceil(5 248 000 / 256), 8 x 256) = 2048 workgroups, so batch 0's 5.2 million slots make chunks of 2560 or 2816 slots -- ten or
    eleven steps of the kernel's loop -- and the short batch's 1.7 million chunks of 1024, four steps, with the last chunks empty.  Every
    shape of tests/test_gpu_agg_edge_weight.py has chunks of exactly 256 slots: one step."""
    assert X.weight_chunks(1280, 1280, X.CUS) == (256, 5, 5) and X.weight_chunks(4097 * 64, 4097 * 64, X.CUS) == (256, 1025, 1025)
    bound = X.slots_bound(2)
    assert bound == 20500 * 256 and X.weight_chunks(bound, bound, X.CUS) == (2816, 1864, 2048)
    s0, s1 = (X.hop2_slots(batches[("distinct", it)][0]) for it in X.COUNTERS)
    X.assert_weight_regimes(s0, s1, X.CUS)
    len0, filled0, grid0 = X.weight_chunks(s0, bound, X.CUS)
    len1, filled1, grid1 = X.weight_chunks(s1, bound, X.CUS)
    assert grid0 == grid1 == 2048 and len0 in (2560, 2816) and len1 == 1024 and filled1 < 2048
    assert len0 * (filled0 - 1) < s0 <= len0 * filled0 and len1 * (filled1 - 1) < s1 <= len1 * filled1
