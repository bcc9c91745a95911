"""Every draw rule and the edge-id pass on a hop of several tiles per workgroup (tests/deepcases.py has the shape and its arithmetic; the
rest of the suite reaches such hops under the reference's rule only).  Hop 2 of batch 0 has about 20 x CUs wide tiles, hop 2 of the short
last batch about 6.7 x CUs.  What a failure of a case here points at, beyond what the same comparison at drawrulecases.SHAPES covers:

  k_sample<.., RULE, COLS>   a workgroup's second and later tile (tile += gridDim.x): s_row / s_deg / s_src and, under the rules that stage
                             picks, s_pick are staged again; s_deg is rewritten in place under the rules that read weights.  The hand-made
                             rows (degree 0, a hub, all weights 0, holes) are inputs of such tiles.
  k_mark                     T = 6 (5 under the rules by weight) and T = 2 tiles per chunk: the prefetch of the next tile, tile_pre != 0
                             from a chunk's second tile on, n_chunks < the grid.
  k_write                    the reload of a workgroup's second and third tile, s_chunk[tile / T] through the device-built FastDiv, and
                             nodes_before() of a loser whose winner lies in another chunk.  A wrong src_off / ids / nc at indices of batch
                             0 only, from tile 8 x CUs on: the reload; throughout: the chunk prefix.
  k_edge_ids                 its own copy of the chunk prefix and of the tile loop: edge_ids / edge_w wrong where src_off is right.
  k_draw_weights             the slot -> edge prefix of the aggregated last hop over the same chunks, from cand_pipe.
  k_draw_edge_weights        its own copy of that prefix for the edge-weighted sums: chunks of ten or eleven steps of 256 slots (four in the
                             short batch, whose last chunks are empty), where every other shape of the suite has chunks of one step.  A wrong
                             nbr_sum from a chunk's second step on (slot % chunk_len >= 256): the rank carried from step to step.

deepcases.regime() gives the tile, chunk (tile // T) and workgroup stride (4 x CUs for k_sample and k_mark, 8 x CUs for k_write and
k_edge_ids) of a differing index: slot = index of the hop's draw, tile = slot // 1024.  Every comparison is array_equal, weights by bit
pattern; the statements (tests/eidref.py, tests/weightedref.py) are computed once per (rule, counter) and shared.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import deepcases as X
import eidref as R
import scratchpoison as P
from aggcases import assert_sum_bits
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import expected_sums
from edgeaggref import expected_nbr_sum_edge
from eidref import assert_edge_ids, bits
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return X.graph()


class Engines:
    """The whole-CSR engine of this module (one logical GPU, weights retained), built on first use and closed with the module, and the
    statements at the batch size of the device's CU count."""

    def __init__(self, K, g):
        self.K, self.g, self.cus, self.eng, self.want = K, g, int(K.lib().legion_sampler_cu_count()), None, {}

    def engine(self, G, **kw):
        B, seeds, g = X.batch_size(self.cus), X.seed_list(self.cus), self.g
        return make_engine(self.K, (X.V, X.F, g["indptr"], g["indices"], g["feats"]), B, X.FAN, G=G, seeds=dict(train=[(seeds, g["labels"][seeds])] * G),
                           edge_weights=g["w"], retain_edge_weights=True, cache_memory=int(X.V * X.F * 4 * 0.15), train_step=2, **kw)

    def whole(self):
        if self.eng is None:
            self.eng = self.engine(1)
        return self.eng

    def statement(self, rule, counter):
        """computed once per (rule, counter) and shared, never changed"""
        key = (rule, counter)
        if key not in self.want:
            ties = []
            alias = self.whole().alias_rows(0) if rule == "weighted" else None      # the table the device built: any valid table is a statement
            self.want[key] = X.statement(self.g, rule, counter, alias=alias, ties=ties, cus=self.cus)
            assert ties == []                                                       # test_deep_tiles_cpu.py: the cap on near-tie rows is zero
        return self.want[key]

    def close(self):
        if self.eng is not None:
            self.eng.close()


@pytest.fixture(scope="module")
def engines(K, g):
    e = Engines(K, g)
    yield e
    e.close()


def test_the_shape_follows_the_device(K, engines):
    """B comes from the device's CU count, and both regimes hold there for the rule with the most and the rule with the fewest slots"""
    assert X.batch_size(engines.cus) == (5 * 8 * engines.cus * 1024) // (2 * 16 * 16) + 20
    for rule in ("shared", "wdistinct"):
        X.assert_regimes(X.hop2_slots(engines.statement(rule, 0)), X.hop2_slots(engines.statement(rule, 1)), engines.cus)


@pytest.mark.parametrize("rule", X.RULES)
def test_every_rule_beyond_one_tile_per_workgroup(K, engines, rule):
    """k_sample<kTile, Whole, RULE, no columns>, k_mark and k_write: nc, ec, ids, labels and both COO arrays of batch 0 (T >= 3, two to
    three tiles per k_write workgroup, five to six per k_sample workgroup) and of the short last batch (T = 2) equal the rule's statement,
    and the batches the device ran lie in those regimes by its own counters and CU count."""
    eng = engines.whole()
    slots = []
    for it in X.COUNTERS:
        want = engines.statement(rule, it)
        eng.run_batch(0, it, **X.ENGINE_ARGS[rule])
        got = eng.result(0, with_features=False)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        assert "edge_ids" not in got
        slots.append(X.hop2_slots(got))
    X.assert_regimes(slots[0], slots[1], engines.cus)


@pytest.mark.parametrize("rule", R.RULES)
def test_edge_ids_beyond_one_tile_per_workgroup(K, engines, rule):
    """k_sample<.., COLS> and k_edge_ids: the ids and the bits of w[edge_ids] of batch 0, the last batch and batch 0 once more equal the
    statement.  k_edge_ids re-derives the edge prefix from chunk_tot and tile_pre with its own code; between the three batches the chunk
    table shrinks from T >= 3 to T = 2 and grows back, so a chunk total or tile_pre left over from the other regime would show."""
    eng = engines.whole()
    slots = {}
    for it in (0, 1, 0):
        eng.run_batch(0, it, edge_ids=True, **R.ENGINE_ARGS[rule])
        assert K.lib().GPUMemoryPool_GetEdgeIds(eng.pools[0]) == 1
        got = eng.result(0, with_features=False)
        assert_edge_ids(engines.statement(rule, it), got)
        slots[it] = X.hop2_slots(got)
    X.assert_regimes(slots[0], slots[1], engines.cus)


def test_presampling_and_fragments(K, engines, g):
    """k_sample<kTile, Presc, Distinct> and k_sample<kTile, Fragments, .., COLS> on the same hops, one two-GPU clique: the pre-sampling batches
    under the distinct rule equal the statement and add its draws per row to edge_access_time (the atomics of a workgroup's later tiles
    included); then the shared and the stream rule draw batch 0 from the fragments with edge ids, which stay positions in the WHOLE CSR."""
    L = K.lib()
    eng = engines.engine(2)
    try:
        for dev in range(2):
            L.SetGPUDevice(dev)
            hot = lambda: K.read_dev(L.GPUCache_GetEdgeAccessedMap(eng.cache, dev), np.uint64, X.V)
            before, acc = hot(), np.zeros(X.V, np.uint64)
            for it in X.COUNTERS:
                want = engines.statement("distinct", it)
                eng.run_batch(dev, it, is_presc=True, sample="distinct")
                assert_batch_equal(want, eng.result(dev, with_features=False), keys=KEYS_NO_FEATURES)
                for inp, cnt in want["draw_counts"]:
                    np.add.at(acc, inp[inp >= 0], cnt[inp >= 0].astype(np.uint64))
            assert acc.sum() > 0 and np.array_equal(hot() - before, acc)
        eng.build_cache(cache_agg_mode=1, node_capacity=X.V // 8, edge_capacity=X.V // 3, train_step=2)
        assert L.GPUCache_Kg(eng.cache) == 2 and all(L.GPUGraphStorage_FragmentRows(eng.graph, dev) == X.V // 3 for dev in range(2))
        for rule in ("shared", "stream"):
            eng.run_batch(0, 0, edge_ids=True, **R.ENGINE_ARGS[rule])
            assert_edge_ids(engines.statement(rule, 0), eng.result(0, with_features=False))
    finally:
        L.legion_clear_error()
        eng.close()


@pytest.mark.parametrize("fill", ["ones", "random"])
def test_a_deep_hop_leaves_nothing_in_the_scratch(K, engines, fill):
    """tile_pre, chunk_tot and cols of a T >= 3 hop, and every other hop- and batch-lifetime buffer, filled with wrong but safe values
    between two runs of batch 0 under the weighted rule without replacement, edge ids on: the second run is the first and the statement's.
    A kernel that reads a chunk total or a tile prefix beyond what this hop's k_mark wrote would take the poison."""
    eng = engines.whole()
    want = engines.statement("wdistinct", 0)
    eng.run_batch(0, 0, edge_ids=True, **R.ENGINE_ARGS["wdistinct"])
    first = eng.result(0, with_features=False)
    done = P.poison_pool(K, eng, np.random.RandomState(3), fill, lifetimes=("hop", "batch"), tile=P.TILE_WIDE, avoid=want["ids"], slots=X.hop2_slots(want))
    assert {"tile_pre", "chunk_tot", "cols", "cand", "tile_edge", "tile_node", "edge_ids", "edge_w"} <= set(done)
    assert not np.array_equal(eng.result(0, with_features=False)["edge_ids"], first["edge_ids"])      # the poison is where the batch is read from
    eng.run_batch(0, 0, edge_ids=True, **R.ENGINE_ARGS["wdistinct"])
    again = eng.result(0, with_features=False)
    assert_edge_ids(first, again)
    assert_edge_ids(want, again)


def test_aggregated_last_hop_over_five_million_slots(K, engines):
    """k_draw_weights and k_gather_sum behind a T >= 3 hop whose draws lie in cand_pipe: the distinct rule's batch 0 handed over as normalised
    neighbour sums, edge ids off and on.  The ids equal the statement, the sums and the rows are bit-equal between the two runs and equal
    the statement of the sums over this batch (distinctcases.expected_sums: tests/gcnref.py's, with a run's draws counted from the batch --
    the graph has holes, and gcnref recounts those from the reference's draws)."""
    eng = engines.whole()
    want = engines.statement("distinct", 0)
    eng.run_batch(0, 0, agg_last_hop=True, agg_norm="both", **R.ENGINE_ARGS["distinct"])
    off = eng.result(0)
    assert_batch_equal(want, off, keys=KEYS_NO_FEATURES)
    assert "edge_ids" not in off
    eng.run_batch(0, 0, agg_last_hop=True, agg_norm="both", edge_ids=True, **R.ENGINE_ARGS["distinct"])
    on = eng.result(0)
    assert_edge_ids(want, on)
    assert on["nbr_sum"].size > 0 and np.array_equal(bits(off["nbr_sum"]), bits(on["nbr_sum"])) and np.array_equal(bits(off["features"]), bits(on["features"]))
    n_in, N, S, d = expected_sums(want, X.FAN, True)
    assert N * X.FAN[1] == X.hop2_slots(want) and on["features"].shape == (n_in, X.F) and on["nbr_sum"].shape == S.shape
    assert np.array_equal(on["out_deg"], d) and np.array_equal(off["out_deg"], d)
    assert np.array_equal(bits(on["features"]), bits(want["features"][:n_in]))
    assert np.array_equal(bits(on["nbr_sum"]), bits(S))


def test_edge_weighted_last_hop_over_five_million_slots(K, engines):
    """k_draw_edge_weights<count> and k_draw_edge_weights behind a T >= 3 hop: the distinct rule's batch 0 and its short last batch handed over
    as neighbour sums scaled by each draw's edge weight.  The grid is min(kMaxChunks, ceil(bound / 256), 8 x CUs) workgroups and a chunk the
    slots over the grid rounded up to 256 (deepcases.weight_chunks, from the device's own counters and CU count): here every workgroup takes
    several steps of its loop, carrying the rank of its slots from one step to the next, and the short batch leaves the last chunks empty --
    tests/test_gpu_agg_edge_weight.py's shapes have chunks of exactly one step.  The batch and its ids equal the statement (tests/eidref.py),
    the sums have the bits of tests/edgeaggref.py's."""
    eng = engines.whole()
    slots = []
    for it in X.COUNTERS:
        want = engines.statement("distinct", it)
        eng.run_batch(0, it, agg_last_hop=True, edge_ids=True, agg_edge_weight=True, **R.ENGINE_ARGS["distinct"])
        assert K.lib().GPUMemoryPool_GetAggEdgeWeight(eng.pools[0]) == 1
        got = eng.result(0)
        assert_edge_ids(want, got)
        n_in, N, _, S = expected_nbr_sum_edge(want, engines.g["indptr"], engines.g["indices"], X.FAN)
        assert N * X.FAN[1] == X.hop2_slots(got) and got["features"].shape == (n_in, X.F) and got["nbr_sum"].shape == S.shape
        assert np.array_equal(bits(got["features"]), bits(want["features"][:n_in]))
        assert not np.isnan(S).any() and (want["edge_w"] == 0).any()
        assert_sum_bits("edge-weighted, batch %d" % it, got["nbr_sum"], S)
        slots.append(X.hop2_slots(got))
    X.assert_weight_regimes(slots[0], slots[1], engines.cus)
    print("weight_chunks at %d CUs: %s, %s" % (engines.cus, X.weight_chunks(slots[0], X.slots_bound(2, engines.cus), engines.cus),
                                               X.weight_chunks(slots[1], X.slots_bound(2, engines.cus), engines.cus)))
