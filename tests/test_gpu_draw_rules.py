"""The sampler's host-side launch path on the GPU (csrc/launchers.cpp, launch_sample_hop and launch_seed in csrc/sampler.hip): every reachable
(draw rule, pre-sampling, partitioned) combination on both tiles against the rule's NumPy statement, the seed launch host-driven against
captured, and both rules' fan-out bound.  Every batch check is array_equal.  Shapes, graph and statements: tests/drawrulecases.py.  Run with
`pytest -m gpu`."""
import numpy as np
import pytest

import drawrulecases as D
import lpref as P
import seededref
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import random_graph
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return D.graph()


class Engines:
    """The engines of this module, built on first use and closed with it.  whole(tile): one logical GPU with a cache controller (plain and
    pre-sampling hops: the whole CSR); clique(tile): two logical GPUs behind a filled cache with CSR fragments, built the way
    test_presampling_counts_and_partitioned_fragments builds it, both serving the same seed list."""

    def __init__(self, K, g):
        self.K, self.g, self.made, self.want = K, g, {}, {}

    def _engine(self, tile, G):
        B, fan = D.SHAPES[tile]
        seeds = D.seed_list(tile)
        g = self.g
        return make_engine(self.K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, fan, G=G, seeds=dict(train=[(seeds, g["labels"][seeds])] * G),
                           edge_weights=g["w"], retain_edge_weights=True, cache_memory=int(D.V * D.F * 4 * 0.15), train_step=2)

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
            assert L.GPUCache_Kg(eng.cache) == 2 and L.GPUCache_EdgeCapacity(eng.cache, 0) == D.V // 3
            assert all(L.GPUGraphStorage_FragmentRows(eng.graph, dev) == D.V // 3 for dev in range(2))
        return self.made[("clique", tile)]

    def statement(self, rule, tile, counter):
        """computed once per (rule, tile, counter) and shared by the three combinations of the rule"""
        key = (rule, tile, counter)
        if key not in self.want:
            ties = []
            alias = self.whole(tile).alias_rows(0) if rule == "weighted" else None      # the table the device built: any valid table is a statement
            self.want[key] = D.statement(self.g, rule, tile, counter, alias=alias, ties=ties)
            assert ties == []                                                           # test_draw_rules_cpu.py: the cap is zero rows
        return self.want[key]

    def close(self):
        for eng in self.made.values():
            eng.close()


@pytest.fixture(scope="module")
def engines(K, g):
    e = Engines(K, g)
    yield e
    e.close()


@pytest.mark.parametrize("tile", list(D.SHAPES))
@pytest.mark.parametrize("rule,kind", D.COMBOS, ids=["%s-%s" % c for c in D.COMBOS])
def test_every_rule_and_table_kind_on_both_tiles(K, engines, rule, kind, tile):
    """The first and the (short) last batch: nc, ec, ids, labels and both COO arrays equal the rule's statement.  A pre-sampling hop
    adds the statement's draws per row to edge_access_time; a partitioned hop reads fragment rows, which are the same rows."""
    L = K.lib()
    presc = kind == "presc"
    eng = engines.clique(tile) if kind == "partitioned" else engines.whole(tile)
    L.SetGPUDevice(0)
    hot = lambda: K.read_dev(L.GPUCache_GetEdgeAccessedMap(eng.cache, 0), np.uint64, D.V)
    before, acc = hot(), np.zeros(D.V, np.uint64)
    for it in D.COUNTERS:
        want = engines.statement(rule, tile, it)
        eng.run_batch(0, it, is_presc=presc, **D.ENGINE_ARGS[rule])
        assert L.GPUMemoryPool_GetSampling(eng.pools[0]) == dict(stream=0, distinct=1, weighted=2, wdistinct=2)[rule]
        assert L.GPUMemoryPool_GetWeightedDistinct(eng.pools[0]) == int(rule == "wdistinct")
        assert_batch_equal(want, eng.result(0, with_features=False), keys=KEYS_NO_FEATURES)
        for inp, cnt in want["draw_counts"]:
            np.add.at(acc, inp[inp >= 0], cnt[inp >= 0].astype(np.uint64))
    assert acc.sum() > 0 and np.array_equal(hot() - before, acc if presc else np.zeros(D.V, np.uint64))


def test_the_shapes_select_both_tiles_and_the_rows_are_there(g):
    """what the cases above rely on: the hand-made rows are seeds of batch 0 of either shape, and the statements see them"""
    deg = np.diff(g["indptr"])
    row = lambda v: slice(int(g["indptr"][v]), int(g["indptr"][v + 1]))
    assert deg[D.EMPTY] == 0 and deg[D.LONG] > D.MAX_FANOUT and deg[D.HUB] > D.MAX_FANOUT
    assert deg[D.ALL_ZERO] > 0 and (g["w"][row(D.ALL_ZERO)] == 0).all() and (g["indices"][row(D.HOLES)] == -1).sum() == 2
    for tile, (B, fan) in D.SHAPES.items():
        seeds = D.seed_list(tile)
        assert seeds[:5].tolist() == [0, 1, 2, 3, 4] and B < len(seeds) < 2 * B
        assert (B * fan[0] <= D.NARROW_SLOTS) == (tile == "narrow")


@pytest.mark.parametrize("lp", [False, True], ids=["lp_draw-off", "lp_draw-on"])
def test_seed_launch_host_driven_equals_captured(K, lp):
    """k_seed through launch_seed's two branches: the batch a recorded graph replays at a counter is the host-driven batch of that counter
    -- first, middle and last (padded with its first triple, or short) -- and both are the statement's.  Seeded, so that the draw word travels both ways; with
    drawn link-prediction thirds (k = 22) and without."""
    k, fan, S = 22, [5, 4], 4242
    V, F, B = 500, 6, 3 * k
    indptr, indices, _ = random_graph(1, V, holes=True)
    feats = np.random.RandomState(1).rand(V, F).astype(np.float32)
    Ls = P.toy_list(indptr, V, k, 5)                         # five batches of [src | pos | neg] thirds, the last one padded
    Lab = (np.arange(len(Ls)) % 1000).astype(np.int32)
    if not lp:
        Ls, Lab = Ls[:-7], Lab[:-7]                          # a short last batch: the size is clamped on the host / on the device
    kw = dict(seed=S, round=1, lp_draw=k if lp else 0)
    st = P.Statement(indptr, indices, feats, B, fan, S) if lp else seededref.Statement(indptr, indices, feats, B, fan, S)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(Ls, Lab)]))
    K.lib().GPUCache_SetPreSc(eng.cache, 0)
    graph = eng.capture_batch(0, **kw)
    assert len(Ls) == 5 * B - (0 if lp else 7)
    for counter in (0, 2, 4):
        eng.run_graph(graph, counter)
        replayed = eng.result(0)
        eng.run_batch(0, counter, **kw)
        driven = eng.result(0)
        assert_batch_equal(replayed, driven)
        assert_batch_equal(st.run_batch(Ls, Lab, counter, round=1), driven)
    eng.close()


def test_both_rule_bounds_refuse_a_count_of_65_and_launch_nothing(K, g):
    """Distinct and weighted-without-replacement take a fan-out of at most 64: GPU_Random_Sampling refuses 65 by each rule's own text, and
    the batch is as the seed launch left it.  The other two rules run the same hop."""
    L = K.lib()
    seeds = D.seed_list("narrow")
    eng = make_engine(K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), 64, [65], seeds=dict(train=[(seeds, g["labels"][seeds])]),
                      edge_weights=g["w"], retain_edge_weights=True)
    pool = eng.pools[0]
    texts = {(1, 0): "GPU_Random_Sampling: distinct sampling (GPUMemoryPool_SetSampleDistinct) takes a fan-out of at most 64: k_sample stages the picks of a tile's rows in static LDS",
             (2, 1): "GPU_Random_Sampling: weighted sampling without replacement (GPUMemoryPool_SetWeightedDistinct) takes a fan-out of at most 64: "
                     "k_sample keeps a row's best picks one per lane and stages them in static LDS"}
    for (kind, flag), text in texts.items():
        L.GPUMemoryPool_SetSampling(pool, kind)
        L.GPUMemoryPool_SetWeightedDistinct(pool, flag)
        L.batch_generator_kernel(None, eng.noder, eng.cache, pool, 64, 0, 0, 0, K.TRAINMODE)
        L.d_stream_sync(None)
        K.check()
        seeded = eng.result(0, with_features=False)
        L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, 65, 2, 0)
        msg = (L.legion_last_error() or b"").decode()
        assert text in msg, msg
        L.legion_clear_error()
        L.d_stream_sync(None)
        assert_batch_equal(seeded, eng.result(0, with_features=False), keys=KEYS_NO_FEATURES)      # no hop ran: counters and buffers untouched
        assert int(seeded["ec"].sum()) == 0
    for sample in ("replace", "weighted"):
        eng.run_batch(0, 0, sample=sample)
        assert int(eng.result(0, with_features=False)["ec"].sum()) > 0
    eng.close()
