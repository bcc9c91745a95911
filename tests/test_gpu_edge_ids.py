"""The edge-id mode on the GPU (GPUMemoryPool_SetEdgeIds: k_sample<.., COLS> + k_edge_ids, INTEGRATION.md "Edge ids") against the NumPy
statement of tests/eidref.py: every rule that hands ids over on both tiles and both counters, whole CSR and the clique's fragments, seeded
batches, the aggregated last hop, recorded graphs, two pipes, poisoned scratch and the refusals.  Every comparison is array_equal; weights
by bit pattern.  Shapes and graph: tests/drawrulecases.py (wsharedcases.rule_graph() is the same graph).  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import drawrulecases as D
import eidref as R
import scratchpoison as P
from conftest import BATCH_KEYS, assert_batch_equal
from eidref import assert_edge_ids, bits
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

SEED = 7                                            # wsharedcases.SEED: its CPU test covers the seeded wshared batches of round 0
EDGE_BUFFERS = ("cols", "edge_ids", "edge_w")


@pytest.fixture(scope="module")
def g():
    return D.graph()


class Engines:
    """The engines of this module, built on first use and closed with it (tests/test_gpu_draw_rules.py builds them the same way): whole(tile)
    one logical GPU over the whole CSR, clique(tile) two logical GPUs behind a filled cache with CSR fragments.  Both retain the weights."""

    def __init__(self, K, g):
        self.K, self.g, self.made, self.want = K, g, {}, {}

    def _engine(self, tile, G, **kw):
        B, fan = D.SHAPES[tile]
        seeds = D.seed_list(tile)
        g = self.g
        return make_engine(self.K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, fan, G=G, seeds=dict(train=[(seeds, g["labels"][seeds])] * G),
                           edge_weights=g["w"], retain_edge_weights=True, cache_memory=int(D.V * D.F * 4 * 0.15), train_step=2, **kw)

    def whole(self, tile):
        if ("whole", tile) not in self.made:
            self.made[("whole", tile)] = self._engine(tile, 1)
        return self.made[("whole", tile)]

    def clique(self, tile):
        if ("clique", tile) not in self.made:
            L = self.K.lib()
            eng = self.made[("clique", tile)] = self._engine(tile, 2)
            for dev in range(2):
                for it in D.COUNTERS:
                    eng.run_batch(dev, it, is_presc=True)
            eng.build_cache(cache_agg_mode=1, node_capacity=D.V // 8, edge_capacity=D.V // 3, train_step=2)
            assert L.GPUCache_Kg(eng.cache) == 2 and all(L.GPUGraphStorage_FragmentRows(eng.graph, dev) == D.V // 3 for dev in range(2))
        return self.made[("clique", tile)]

    def statement(self, rule, tile, counter, seed=None, round=0):
        """computed once per batch and shared, never changed"""
        key = (rule, tile, counter, seed, round)
        if key not in self.want:
            B, fan = D.SHAPES[tile]
            seeds = D.seed_list(tile)
            ties = []
            self.want[key] = R.run_batch(self.g, rule, seeds, self.g["labels"][seeds], B, counter, fan, seed=seed, round=round, ties=ties)
            assert ties == []               # the cap on near-tie rows is zero (test_draw_rules_cpu.py, test_weighted_shared_cpu.py, test_edge_ids_cpu.py)
        return self.want[key]

    def close(self):
        for eng in self.made.values():
            eng.close()


@pytest.fixture(scope="module")
def engines(K, g):
    e = Engines(K, g)
    yield e
    e.close()


COMBOS = [(r, "whole") for r in R.RULES] + [(r, "partitioned") for r in R.PARTITIONED_RULES]


@pytest.mark.parametrize("tile", list(D.SHAPES))
@pytest.mark.parametrize("rule,kind", COMBOS, ids=["%s-%s" % c for c in COMBOS])
def test_ids_and_weights_equal_the_statement(K, engines, rule, kind, tile):
    """The first and the (short) last batch of either tile: edge_ids is the statement's, edge_w has the bits of w[edge_ids], and the batch
    around them is the rule's.  A partitioned hop draws from fragment rows; the ids are still positions in the WHOLE CSR."""
    eng = engines.clique(tile) if kind == "partitioned" else engines.whole(tile)
    for it in D.COUNTERS:
        eng.run_batch(0, it, edge_ids=True, **R.ENGINE_ARGS[rule])
        assert K.lib().GPUMemoryPool_GetEdgeIds(eng.pools[0]) == 1
        assert_edge_ids(engines.statement(rule, tile, it), eng.result(0, with_features=False))


@pytest.mark.parametrize("rule", ["stream", "distinct", "shared"])
def test_seeded_batches(K, engines, rule):
    """seed 7, rounds 0 and 1: the ids are the statement's under the batch's draw word, over the round's shuffled list"""
    eng = engines.whole("narrow")
    for rnd in (0, 1):
        for it in D.COUNTERS:
            eng.run_batch(0, it, edge_ids=True, seed=SEED, round=rnd, **R.ENGINE_ARGS[rule])
            assert_edge_ids(engines.statement(rule, "narrow", it, seed=SEED, round=rnd), eng.result(0, with_features=False))


def test_seeded_weighted_shared_batch(K, engines):
    """the seeded wshared batches whose near-tie cap tests/test_weighted_shared_cpu.py proves: seed 7, round 0"""
    eng = engines.whole("narrow")
    for it in D.COUNTERS:
        eng.run_batch(0, it, edge_ids=True, seed=SEED, round=0, **R.ENGINE_ARGS["wshared"])
        assert_edge_ids(engines.statement("wshared", "narrow", it, seed=SEED), eng.result(0, with_features=False))


@pytest.mark.parametrize("rule", R.RULES)
def test_the_existing_outputs_do_not_move(K, engines, rule):
    """nc, ec, ids, labels, both COO arrays and the features of a batch with the mode on are those of the same batch with it off"""
    eng = engines.whole("narrow")
    eng.run_batch(0, 0, **R.ENGINE_ARGS[rule])
    off = eng.result(0)
    assert "edge_ids" not in off and K.lib().GPUMemoryPool_GetEdgeIds(eng.pools[0]) == 0
    eng.run_batch(0, 0, edge_ids=True, **R.ENGINE_ARGS[rule])
    on = eng.result(0)
    assert_batch_equal(off, on, keys=BATCH_KEYS)
    assert len(on["edge_ids"]) == len(on["src_off"])


@pytest.mark.parametrize("rule", ["stream", "distinct"])
def test_aggregated_last_hop(K, engines, rule):
    """the last hop's draws lie in cand_pipe: the ids still match, and the neighbour sums are those of the batch without the mode"""
    eng = engines.whole("narrow")
    eng.run_batch(0, 0, agg_last_hop=True, **R.ENGINE_ARGS[rule])
    off = eng.result(0)
    eng.run_batch(0, 0, agg_last_hop=True, edge_ids=True, **R.ENGINE_ARGS[rule])
    on = eng.result(0)
    assert_edge_ids(engines.statement(rule, "narrow", 0), on)
    assert on["nbr_sum"].size > 0 and np.array_equal(bits(off["nbr_sum"]), bits(on["nbr_sum"])) and np.array_equal(bits(off["features"]), bits(on["features"]))


def test_recorded_graph_and_its_refusals(K, g):
    """capture_batch(edge_ids=True) replays for both counters like run_batch; a graph replays only in the state it was recorded in"""
    L = K.lib()
    B, fan = D.SHAPES["narrow"]
    seeds = D.seed_list("narrow")
    eng = make_engine(K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, fan, seeds=dict(train=[(seeds, g["labels"][seeds])]),
                      edge_weights=g["w"], retain_edge_weights=True)
    try:
        L.GPUCache_SetPreSc(eng.cache, 0)
        graph = eng.capture_batch(0, edge_ids=True, sample="distinct")
        for it in D.COUNTERS:
            eng.run_graph(graph, it)
            replayed = eng.result(0)
            eng.run_batch(0, it, edge_ids=True, sample="distinct")
            driven = eng.result(0)
            assert_batch_equal(replayed, driven)
            assert np.array_equal(replayed["edge_ids"], driven["edge_ids"]) and np.array_equal(bits(replayed["edge_w"]), bits(driven["edge_w"]))
            want = R.run_batch(g, "distinct", seeds, g["labels"][seeds], B, it, fan)
            assert_edge_ids(want, replayed)
        L.GPUMemoryPool_SetEdgeIds(eng.pools[0], 0)
        with pytest.raises(RuntimeError, match=r"LegionBatchGraph_Launch: the graph was recorded with edge ids \(GPUMemoryPool_SetEdgeIds\) and the pool has the mode off now"):
            eng.run_graph(graph, 0)
        plain = eng.capture_batch(0, sample="distinct")
        eng.run_graph(plain, 0)
        L.GPUMemoryPool_SetEdgeIds(eng.pools[0], 1)
        with pytest.raises(RuntimeError, match=r"LegionBatchGraph_Launch: the graph was recorded without edge ids and the pool has the mode on now \(GPUMemoryPool_SetEdgeIds\)"):
            eng.run_graph(plain, 0)
        eng.run_graph(graph, 1)                     # back in its state: it replays
        assert np.array_equal(eng.result(0, edge_ids=True)["edge_ids"], R.run_batch(g, "distinct", seeds, g["labels"][seeds], B, 1, fan)["edge_ids"])
    finally:
        L.legion_clear_error()
        eng.close()


def test_two_pipes_keep_their_own_ids(K, engines, g):
    """batch 0 into pipe 0, batch 1 into pipe 1: pipe 0 still holds batch 0's ids and weights"""
    eng = engines._engine("narrow", 1, pipeline_depth=2)
    try:
        eng.run_batch(0, 0, pipe=0, edge_ids=True)
        eng.run_batch(0, 1, pipe=1, edge_ids=True)
        assert_edge_ids(engines.statement("stream", "narrow", 0), eng.result(0, pipe=0, with_features=False))
        assert_edge_ids(engines.statement("stream", "narrow", 1), eng.result(0, pipe=1, with_features=False))
    finally:
        eng.close()


@pytest.mark.parametrize("tile", list(D.SHAPES))
@pytest.mark.parametrize("fill", P.FILLS)
def test_the_result_does_not_depend_on_what_the_scratch_held(K, engines, tile, fill):
    """cols, edge_ids and edge_w filled through GPUMemoryPool_ScratchInfo with wrong but safe values between two runs of one batch"""
    eng = engines.whole(tile)
    rule = "wdistinct" if tile == "narrow" else "stream"
    eng.run_batch(0, 0, edge_ids=True, **R.ENGINE_ARGS[rule])
    first = eng.result(0, with_features=False)
    listed = {b["name"]: b for b in K.pool_scratch(eng.pools[0], 0)}
    assert [(listed[n]["lifetime"], listed[n]["per_pipe"], listed[n]["elem_bytes"]) for n in EDGE_BUFFERS] == [("hop", False, 4), ("batch", True, 8), ("batch", True, 4)]
    done = P.poison_pool(K, eng, np.random.RandomState(3), fill, lifetimes=("hop", "batch"), names=EDGE_BUFFERS, tile=P.TILE_NARROW if tile == "narrow" else P.TILE_WIDE)
    assert sorted(done) == sorted(EDGE_BUFFERS)
    poisoned = eng.result(0, with_features=False)
    assert not np.array_equal(poisoned["edge_ids"], first["edge_ids"])          # the poison is where the batch is read from
    eng.run_batch(0, 0, edge_ids=True, **R.ENGINE_ARGS[rule])
    again = eng.result(0, with_features=False)
    assert_edge_ids(first, again)
    assert_edge_ids(engines.statement(rule, tile, 0), again)


def test_a_pool_that_never_saw_the_mode_lists_and_holds_nothing_of_it(K, g):
    L = K.lib()
    seeds = D.seed_list("narrow")
    eng = make_engine(K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), 64, [5, 4], seeds=dict(train=[(seeds, g["labels"][seeds])]))
    try:
        eng.run_batch(0, 0)
        assert [b["name"] for b in K.pool_scratch(eng.pools[0], 0)] == [t[0] for t in P.EXPECTED_TABLE]
        assert L.GPUMemoryPool_GetEdgeIds(eng.pools[0]) == 0 and not L.GPUMemoryPool_GetEdgeIdBuffer(eng.pools[0]) and not L.GPUMemoryPool_GetEdgeWeightBuffer(eng.pools[0])
        K.check()
    finally:
        eng.close()


def test_refusals_are_sticky_errors_by_name(K, g):
    """argument checks, all made before any launch: a null pool, the alias rule under the mode (either order), a switch during capture; and
    a graph without retained weights has no weight buffer while its ids are served"""
    L = K.lib()
    err = lambda: (L.legion_last_error() or b"").decode()
    B, fan = D.SHAPES["narrow"]
    seeds = D.seed_list("narrow")
    arrays = (D.V, D.F, g["indptr"], g["indices"], g["feats"])
    L.legion_clear_error()
    L.GPUMemoryPool_SetEdgeIds(None, 1)
    assert "GPUMemoryPool_SetEdgeIds: null pool" in err()
    L.legion_clear_error()
    assert L.GPUMemoryPool_GetEdgeIds(None) == 0 and not err()
    for getter in ("GPUMemoryPool_GetEdgeIdBuffer", "GPUMemoryPool_GetEdgeWeightBuffer"):
        assert not getattr(L, getter)(None)
        assert getter + ": null pool" in err()
        L.legion_clear_error()
    eng = make_engine(K, arrays, B, fan, seeds=dict(train=[(seeds, g["labels"][seeds])]), edge_weights=g["w"], retain_edge_weights=True)
    try:
        pool = eng.pools[0]
        alias = r"the alias table holds the alias neighbour's id, not its column"
        with pytest.raises(RuntimeError, match=r"GPUMemoryPool_SetEdgeIds: edge ids \(GPUMemoryPool_SetEdgeIds\) cannot be handed over under weighted sampling with replacement.*" + alias):
            eng.run_batch(0, 0, sample="weighted", edge_ids=True)
        assert L.GPUMemoryPool_GetEdgeIds(pool) == 0 and L.GPUMemoryPool_GetSampling(pool) == 2
        eng.run_batch(0, 0, sample="weighted", weighted_distinct=True, edge_ids=True)       # with the flag the weighted kind hands ids over
        L.GPUMemoryPool_SetWeightedDistinct(pool, 0)                                        # ... and the flag cannot leave under the mode
        assert "GPUMemoryPool_SetWeightedDistinct: edge ids" in err() and L.GPUMemoryPool_GetWeightedDistinct(pool) == 1
        L.legion_clear_error()
        eng.run_batch(0, 0, edge_ids=True)
        L.GPUMemoryPool_SetSampling(pool, 2)                                                # the kind without the flag: the alias rule
        assert "GPUMemoryPool_SetSampling: edge ids" in err() and L.GPUMemoryPool_GetSampling(pool) == 0 and L.GPUMemoryPool_GetEdgeIds(pool) == 1
        L.legion_clear_error()
        L.GPUCache_SetPreSc(eng.cache, 0)
        stream = L.d_stream_create()
        assert L.GPUMemoryPool_BeginBatchCapture(pool, stream) == 0
        L.GPUMemoryPool_SetEdgeIds(pool, 0)
        assert "GPUMemoryPool_SetEdgeIds: the pool is being captured" in err() and L.GPUMemoryPool_GetEdgeIds(pool) == 1
        L.legion_clear_error()
        eng.run_batch(0, 0, stream=stream, sync=False, gather=False, plan=False, edge_ids=True)
        graph = L.GPUMemoryPool_EndBatchCapture(pool, stream)
        K.check()
        assert graph
        L.LegionBatchGraph_Delete(graph)
        L.d_stream_destroy(stream)
    finally:
        L.legion_clear_error()
        eng.close()
    bare = make_engine(K, arrays, B, fan, seeds=dict(train=[(seeds, g["labels"][seeds])]))
    try:
        bare.run_batch(0, 0, edge_ids=True)
        got = bare.result(0, with_features=False)
        assert not L.GPUMemoryPool_GetEdgeWeightBuffer(bare.pools[0]) and not err()
        assert_edge_ids(R.run_batch(g, "stream", seeds, g["labels"][seeds], B, 0, fan), got, weights=False)
    finally:
        L.legion_clear_error()
        bare.close()
