"""The edge-feature mode on the GPU (GPUMemoryPool_SetEdgeFeatures: k_gather_edges behind get_edge_feature_kernel / _all, INTEGRATION.md "Edge
features") against the NumPy statement of tests/efref.py, edge_feat[e, :] = X[edge_ids[e], :]: every row width at which the kernel takes
another path, both launchers, the clique's fragments, a grid that loops, a poisoned output buffer, two pipes, a table indexed beyond 2^31
floats, recorded graphs, the gather on a second stream beside the next batch's sampler, and the refusals.  Every comparison is by bit
pattern.  Graph and shapes: tests/drawrulecases.py (multi-edges, zero-degree rows, holes).  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import drawrulecases as D
import scratchpoison as P
from conftest import assert_batch_equal
from efref import assert_edge_feat, bits
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 4, 20, 64)        # a scalar row; an odd width (rows not 8-byte aligned); one float4 chunk; C = 5, no power of two; 16 chunks
RULES = dict(stream=dict(sample="replace"), distinct=dict(sample="distinct"))
# launch_gather_edges' grid rule (csrc/gather.hip): one workgroup per BLOCK * U items of the static bound, at most BLOCKS_PER_CU per compute unit
BLOCK, U, BLOCKS_PER_CU = 256, 2, 8


@pytest.fixture(scope="module")
def g():
    return D.graph()


def table(g, dim):
    """the synthetic table of the toy graph: every value names its row and its column"""
    import legion1_amd.synth as S
    return S.edge_features(0, len(g["indices"]), dim)


class Engines:
    """One engine per (kind, dim), built on first use and closed with the module; the tables are computed once and never changed."""

    def __init__(self, K, g):
        self.K, self.g, self.made, self.X = K, g, {}, {}

    def table(self, dim):
        if dim not in self.X:
            self.X[dim] = table(self.g, dim)
        return self.X[dim]

    def make(self, dim, tile="narrow", G=1, B=None, fan=None, **kw):
        b, f = D.SHAPES[tile]
        seeds = D.seed_list(tile)
        g = self.g
        return make_engine(self.K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B or b, fan or f, G=G, seeds=dict(train=[(seeds, g["labels"][seeds])] * G),
                           edge_features=self.table(dim) if dim else None, **kw)

    def whole(self, dim):
        if ("whole", dim) not in self.made:
            self.made[("whole", dim)] = self.make(dim)
        return self.made[("whole", dim)]

    def clique(self, dim):
        """two logical GPUs behind a filled cache: the hops draw from the clique's CSR fragments"""
        if ("clique", dim) not in self.made:
            L = self.K.lib()
            eng = self.made[("clique", dim)] = self.make(dim, G=2, cache_memory=int(D.V * D.F * 4 * 0.15), train_step=2)
            for dev in range(2):
                for it in D.COUNTERS:
                    eng.run_batch(dev, it, is_presc=True)
            eng.build_cache(cache_agg_mode=1, node_capacity=D.V // 8, edge_capacity=D.V // 3, train_step=2)
            assert L.GPUCache_Kg(eng.cache) == 2 and all(L.GPUGraphStorage_FragmentRows(eng.graph, dev) == D.V // 3 for dev in range(2))
        return self.made[("clique", dim)]

    def close(self):
        for eng in self.made.values():
            eng.close()


@pytest.fixture(scope="module")
def engines(K, g):
    e = Engines(K, g)
    yield e
    e.close()


def feat_buffer(K, eng, pipe=0):
    """(device pointer, bytes) of the pipe's edge_feat buffer as GPUMemoryPool_ScratchInfo lists it"""
    b = {b["name"]: b for b in K.pool_scratch(eng.pools[0], pipe)}["edge_feat"]
    assert (b["kind"], b["elem_bytes"], b["lifetime"], b["per_pipe"]) == ("float", 4, "batch", True) and b["ptr"]
    assert b["bytes"] == eng.num_ids * eng.edge_feature_dim * 4
    return b["ptr"], b["bytes"]


# ---- row widths, rules, both launchers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("dim", DIMS)
def test_rows_equal_the_statement_at_every_width(K, engines, dim, rule):
    """Two hops over the toy graph, the first and the (short) last batch, gathered hop by hop: under `stream` repeated draws give the same
    table row twice; the table copy the graph holds is the one it was given."""
    eng, X = engines.whole(dim), engines.table(dim)
    assert eng.edge_feature_dim == dim and K.lib().GPUGraphStorage_GetEdgeFeatureDim(eng.graph) == dim
    assert np.array_equal(bits(eng.edge_feature_rows(0, 1000, 300)), bits(X[1000:1300]))
    for it in D.COUNTERS:
        eng.run_batch(0, it, edge_ids=True, edge_features=True, **RULES[rule])
        got = eng.result(0, with_features=False)
        assert K.lib().GPUMemoryPool_GetEdgeFeatures(eng.pools[0]) == dim and len(got["edge_ids"]) > 300
        assert_edge_feat(X, got)
        if rule == "stream":
            assert len(np.unique(got["edge_ids"])) < len(got["edge_ids"])          # some row is gathered twice


@pytest.mark.parametrize("dim", (3, 20))
def test_per_hop_launches_and_the_one_launch_give_identical_bytes(K, engines, dim):
    """get_edge_feature_kernel behind each hop against get_edge_feature_kernel_all behind the last: the whole buffer, not just the batch's part"""
    eng, X = engines.whole(dim), engines.table(dim)
    eng.run_batch(0, 0, edge_ids=True, edge_features=True)           # the mode is on: the buffer exists
    ptr, nbytes = feat_buffer(K, eng)
    whole = {}
    for per_level in (True, False):
        K.lib().d_memset_async(ptr, 0, nbytes, None)
        K.lib().d_stream_sync(None)
        eng.run_batch(0, 0, edge_ids=True, edge_features=True, per_level=per_level)
        assert_edge_feat(X, eng.result(0, with_features=False))
        whole[per_level] = K.read_dev(ptr, np.uint32, nbytes // 4)
    assert np.array_equal(whole[True], whole[False]) and whole[True].any()


def test_fragment_hops_gather_whole_csr_rows(K, engines):
    """a partitioned hop draws from fragment rows; the ids, and with them the table rows, are positions in the WHOLE CSR"""
    eng, X = engines.clique(20), engines.table(20)
    for it in D.COUNTERS:
        eng.run_batch(0, it, edge_ids=True, edge_features=True, sample="distinct")
        assert_edge_feat(X, eng.result(0, with_features=False))


def test_every_lane_takes_several_trips_of_the_persistent_loop(K, engines, g):
    """1024 seeds x [16, 9] at dim = 64 (C = 16 chunks), one launch over all edges.  The launcher's grid is min(ceil(bound * C / (256 * U)),
    8 * CUs) workgroups, U = 2 items per lane and trip: on a 256-CU part 2048 workgroups = 1 048 576 items per trip, so every lane takes two
    trips from 2 097 152 items = 131 072 edges on; the batch has about 159 000 (asserted against the device's CU count below)."""
    L = K.lib()
    dim, B, fan = 64, 1024, [16, 9]
    eng, X = engines.make(dim, tile="wide", B=B, fan=fan), engines.table(dim)
    try:
        eng.run_batch(0, 0, edge_ids=True, edge_features=True, per_level=False)
        got = eng.result(0, with_features=False)
        C, bound = dim // 4, B * fan[0] + B * fan[0] * fan[1]
        grid = min(-(-bound * C // (BLOCK * U)), BLOCKS_PER_CU * L.legion_sampler_cu_count())
        assert len(got["edge_ids"]) * C >= 2 * grid * BLOCK * U, (len(got["edge_ids"]), grid)
        assert_edge_feat(X, got)
    finally:
        eng.close()


# ---- stores nothing else, reads nothing stale --------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (3, 20))
def test_the_buffer_behind_the_batch_is_untouched_and_the_rows_do_not_depend_on_what_it_held(K, engines, dim):
    L = K.lib()
    eng, X = engines.whole(dim), engines.table(dim)
    eng.run_batch(0, 1, edge_ids=True, edge_features=True)           # the mode is on: the buffer exists
    ptr, nbytes = feat_buffer(K, eng)
    rows = {}
    for fill in (0, P.NAN_BITS):
        pattern = np.full(nbytes // 4, fill, np.uint32)
        L.d_copy_h_2_d(ptr, pattern.ctypes.data, nbytes)
        eng.run_batch(0, 1, edge_ids=True, edge_features=True)
        got = eng.result(0, with_features=False)
        n = len(got["edge_ids"]) * dim
        whole = K.read_dev(ptr, np.uint32, nbytes // 4)
        assert 0 < n < len(whole) and (whole[n:] == fill).all()      # everything behind n_edges * dim is still the pattern
        assert_edge_feat(X, got)
        rows[fill] = whole[:n]
    assert np.array_equal(rows[0], rows[P.NAN_BITS])


def test_two_pipes_keep_their_own_rows(K, engines):
    """batch 0 into pipe 0, batch 1 into pipe 1: pipe 0 still holds batch 0's rows"""
    eng, X = engines.make(20, pipeline_depth=2), engines.table(20)
    try:
        eng.run_batch(0, 0, pipe=0, edge_ids=True, edge_features=True)
        first = eng.result(0, pipe=0, with_features=False)
        eng.run_batch(0, 1, pipe=1, edge_ids=True, edge_features=True)
        again = eng.result(0, pipe=0, with_features=False)
        assert_edge_feat(X, again)
        assert_edge_feat(X, eng.result(0, pipe=1, with_features=False))
        assert np.array_equal(first["edge_ids"], again["edge_ids"]) and np.array_equal(bits(first["edge_feat"]), bits(again["edge_feat"]))
        eng.run_batch(0, 0, pipe=1, edge_ids=True)                   # a batch without the gather: pipe 1 hands nothing out, pipe 0 still does
        L = K.lib()
        L.GPUMemoryPool_SetCurrentPipe(eng.pools[0], 1)
        assert not L.GPUMemoryPool_GetEdgeFeatureBuffer(eng.pools[0])
        assert "edge_feat" not in eng.result(0, pipe=1, with_features=False)
    finally:
        eng.close()


# ---- 64-bit addressing -------------------------------------------------------------------------------------------------------
def test_rows_beyond_two_to_the_31_floats(K):
    """dim = 64 over E = 4096 x 8200 = 33 587 200 > 2^25 edges: the table is 8.6 GB, filled on the device by legion_synth_edge_features and
    never held on the host.  The batch's seeds are the last 64 rows; rows 4093..4095 lie wholly beyond 2^25 edges = 2^31 floats (4093 x 8200
    = 33 562 600 > 2^25), so their 15 draws of hop 1 -- and max(edge_ids) x dim, asserted -- address the table past 2^31 floats; the rows
    are checked against the closed form."""
    import legion1_amd.synth as S
    L = K.lib()
    dim, V, deg = 64, 4096, 8200
    E = V * deg
    assert E > 1 << 25 and (V - 3) * deg >= 1 << 25
    indptr = np.arange(V + 1, dtype=np.int64) * deg
    indices = np.random.RandomState(5).randint(0, V, size=E).astype(np.int32)
    seeds = np.arange(V - 64, V, dtype=np.int32)
    L.SetGPUDevice(0)
    raw = K.DevBuf(E * dim * 4)
    eng = None
    try:
        L.legion_synth_edge_features(None, raw.ptr, 0, E, dim)
        L.d_stream_sync(None)
        K.check()
        eng = K.Engine(indptr, indices, np.zeros((V, 1), np.float32), V, 1, dict(train=[(seeds, np.zeros(len(seeds), np.int32))]), 64, [5, 4],
                       edge_features=raw.ptr, edge_feature_dim=dim)
        raw.free()                                                   # the graph holds its own copy
        assert np.array_equal(bits(eng.edge_feature_rows(0, E - 3, 3)), bits(S.edge_features(E - 3, 3, dim)))
        eng.run_batch(0, 0, edge_ids=True, edge_features=True, gather=False, per_level=False)
        got = eng.result(0, with_features=False)
        assert int(got["edge_ids"].max()) * dim >= 1 << 31 and len(got["edge_ids"]) == 64 * 5 + 64 * 5 * 4
        assert (got["edge_ids"][:320] * dim >= 1 << 31).sum() >= 15 # every draw of the last three seeds
        want = S.edge_features_at(got["edge_ids"], dim)
        assert np.array_equal(bits(want), bits(got["edge_feat"]))
    finally:
        L.legion_clear_error()
        raw.free()
        if eng is not None:
            eng.close()


# ---- recorded graphs ---------------------------------------------------------------------------------------------------------
def test_recorded_graph_and_its_refusals(K, engines):
    """capture_batch(edge_features=True) replays for both counters, twice, like run_batch; a graph replays only at the width it was recorded
    at, and not into a buffer the pool has reallocated since"""
    L = K.lib()
    eng, X = engines.make(20), engines.table(20)
    try:
        pool = eng.pools[0]
        L.GPUCache_SetPreSc(eng.cache, 0)
        graph = eng.capture_batch(0, edge_ids=True, edge_features=True, sample="distinct")
        assert not L.GPUMemoryPool_GetEdgeFeatureBuffer(pool)        # recorded, not run: nothing was gathered yet
        for it in D.COUNTERS + D.COUNTERS:
            eng.run_graph(graph, it)
            replayed = eng.result(0)
            eng.run_batch(0, it, edge_ids=True, edge_features=True, sample="distinct")
            driven = eng.result(0)
            assert_batch_equal(replayed, driven)
            assert_edge_feat(X, replayed)
            assert np.array_equal(replayed["edge_ids"], driven["edge_ids"]) and np.array_equal(bits(replayed["edge_feat"]), bits(driven["edge_feat"]))
        L.GPUMemoryPool_SetEdgeFeatures(pool, 0)
        with pytest.raises(RuntimeError, match=r"LegionBatchGraph_Launch: the graph was recorded gathering edge features \(GPUMemoryPool_SetEdgeFeatures\) and the pool is at another row width"):
            eng.run_graph(graph, 0)
        plain = eng.capture_batch(0, edge_ids=True, sample="distinct")
        eng.run_graph(plain, 0)
        L.GPUMemoryPool_SetEdgeFeatures(pool, 20)
        K.check()
        with pytest.raises(RuntimeError, match=r"LegionBatchGraph_Launch: the graph was recorded without edge features and the pool gathers them now"):
            eng.run_graph(plain, 0)
        eng.run_graph(graph, 1)                                      # back at its width, the buffer kept: it replays
        assert_edge_feat(X, eng.result(0, edge_features=True))
        L.GPUMemoryPool_SetEdgeFeatures(pool, 8)                     # another width: refused by the rule ...
        K.check()
        with pytest.raises(RuntimeError, match=r"the pool is at another row width"):
            eng.run_graph(graph, 0)
        L.GPUMemoryPool_SetEdgeFeatures(pool, 20)                    # ... and back at 20 the buffer is a new allocation
        K.check()
        with pytest.raises(RuntimeError, match=r"LegionBatchGraph_Launch: the graph writes an edge-feature buffer the pool has reallocated since"):
            eng.run_graph(graph, 0)
    finally:
        L.legion_clear_error()
        eng.close()


# ---- beside the next batch's sampler ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (3, 20))
def test_edge_rows_gathered_beside_the_next_batchs_sampler(K, engines, g, dim):
    """k_gather_edges reads only the batch's pipe and the table, so it can run beside the next batch's sampler.  Depth 2, the schedule of
    tests/test_gpu_agg_edge_weight.py::test_overlapped_two_stream_schedule_and_the_graphs_refusals: batch i + 1 is sampled (a recorded
    LegionBatchGraph per pipe) on one stream while get_edge_feature_kernel_all of batch i runs on the other, behind an event.  The sampler of
    batch i + 1 overwrites the pool's draw buffer, columns and slot states and sets the pool's per-batch host state meanwhile.  So that the
    rows read back are the second stream's, the pipe's buffer is filled with NaN words on that stream in front of its gather (the recorded
    batch gathers once itself).  dim 3: the scalar kernel; dim 20: the 16-byte one."""
    import eidref
    L = K.lib()
    eng, X = engines.make(dim, pipeline_depth=2), engines.table(dim)
    B, fan = D.SHAPES["narrow"]
    seeds = D.seed_list("narrow")
    s_samp, s_gath = L.d_stream_create(), L.d_stream_create()
    try:
        L.GPUCache_SetPreSc(eng.cache, 0)
        pool = eng.pools[0]
        ev_sampled, ev_gathered = [L.d_event_create(), L.d_event_create()], [L.d_event_create(), L.d_event_create()]
        used = [False, False]
        graphs = [eng.capture_batch(0, gather=False, pipe=q, stream=s_samp, sample="distinct", edge_ids=True, edge_features=True) for q in (0, 1)]
        assert L.GPUMemoryPool_GetEdgeFeatures(pool) == dim and L.GPUMemoryPool_GetEdgeIds(pool) == 1
        bufs = [feat_buffer(K, eng, q) for q in (0, 1)]
        assert bufs[0][0] != bufs[1][0]
        want = {it: eidref.run_batch(g, "distinct", seeds, g["labels"][seeds], B, it, fan) for it in D.COUNTERS}

        def enqueue(i, counter):
            q = i % 2
            L.GPUMemoryPool_SetCurrentPipe(pool, q)
            L.GPUMemoryPool_SetCurrentMode(pool, K.TRAINMODE)
            if used[q]:
                L.d_stream_wait_event(s_samp, ev_gathered[q])
            eng.run_graph(graphs[q], counter, sync=False)
            L.d_event_record(ev_sampled[q], s_samp)
            L.d_stream_wait_event(s_gath, ev_sampled[q])
            L.d_memset_async(bufs[q][0], 0xFF, bufs[q][1], s_gath)
            L.get_edge_feature_kernel_all(s_gath, eng.graph, pool, 0)
            L.d_event_record(ev_gathered[q], s_gath)
            used[q] = True

        counters = [0, 1, 1, 0, 1, 0]
        enqueue(0, counters[0])
        for i, it in enumerate(counters):
            if i + 1 < len(counters):
                enqueue(i + 1, counters[i + 1])          # batch i + 1 is sampled while batch i's edge rows are still being gathered
            L.d_stream_sync(s_samp)
            L.d_stream_sync(s_gath)
            K.check()
            got = eng.result(0, pipe=i % 2, with_features=False, edge_ids=True, edge_features=True)
            eidref.assert_edge_ids(want[it], got, weights=False)
            assert_edge_feat(X, got)
            n = len(got["edge_ids"]) * dim
            rest = K.read_dev(bufs[i % 2][0], np.uint32, bufs[i % 2][1] // 4)[n:]
            assert len(rest) and (rest == 0xFFFFFFFF).all()              # ... and behind the batch's rows the second stream's fill is untouched
    finally:
        L.legion_clear_error()
        eng.close()
        for s in (s_samp, s_gath):
            L.d_stream_destroy(s)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_launcher_and_setter_refusals_are_sticky_errors_by_name(K, engines, g):
    """argument checks, all made before any launch"""
    L = K.lib()

    def err():
        msg = (L.legion_last_error() or b"").decode()
        L.legion_clear_error()
        return msg

    bare = engines.make(0)                                           # a graph without a table
    try:
        pool = bare.pools[0]
        bare.run_batch(0, 0, edge_ids=True)
        L.get_edge_feature_kernel(None, bare.graph, pool, 0, 2)
        assert "get_edge_feature_kernel: the pool does not gather edge features (GPUMemoryPool_SetEdgeFeatures)" in err()
        L.GPUMemoryPool_SetEdgeFeatures(pool, 4)
        K.check()
        L.get_edge_feature_kernel(None, bare.graph, pool, 0, 2)
        assert "get_edge_feature_kernel: the graph holds no edge-feature table on this GPU (GPUGraphStorage_SetEdgeFeatures)" in err()
        L.get_edge_feature_kernel_all(None, bare.graph, pool, 0)
        assert "get_edge_feature_kernel_all: the graph holds no edge-feature table on this GPU" in err()
        bare.set_edge_features(table(g, 3))
        L.get_edge_feature_kernel(None, bare.graph, pool, 0, 2)
        assert "get_edge_feature_kernel: the graph's edge-feature table has rows of 3 floats, the pool gathers rows of 4" in err()
        for op in (0, 1, 3, 6, -2):                                  # two hops: 2 and 4 are the sampling ops
            L.get_edge_feature_kernel(None, bare.graph, pool, 0, op)
            assert "get_edge_feature_kernel: op_id must be 2,4,..,2*hops" in err(), op
        L.GPUMemoryPool_SetEdgeFeatures(pool, 3)
        K.check()
        L.get_edge_feature_kernel(None, bare.graph, pool, 0, 2)      # now everything fits: it gathers
        L.d_stream_sync(None)
        K.check()
        assert L.GPUMemoryPool_GetEdgeFeatureBuffer(pool)
        # a pipe whose batch left no edge ids: pre-sampling, sampled with the ids off, a hop not sampled yet
        L.GPUMemoryPool_SetEdgeFeatures(pool, 0)
        bare.run_batch(0, 0, is_presc=True, edge_ids=True)
        L.GPUMemoryPool_SetEdgeFeatures(pool, 3)
        L.get_edge_feature_kernel_all(None, bare.graph, pool, 0)
        assert "get_edge_feature_kernel_all: the current pipe's batch left no edge ids for this hop" in err() and not L.GPUMemoryPool_GetEdgeFeatureBuffer(pool)
        L.GPUMemoryPool_SetEdgeFeatures(pool, 0)
        bare.run_batch(0, 0)
        L.GPUMemoryPool_SetEdgeIds(pool, 1)
        L.GPUMemoryPool_SetEdgeFeatures(pool, 3)
        K.check()
        L.get_edge_feature_kernel(None, bare.graph, pool, 0, 2)
        assert "get_edge_feature_kernel: the current pipe's batch left no edge ids for this hop" in err()
        L.batch_generator_kernel(None, bare.noder, bare.cache, pool, 64, 0, 0, 0, K.TRAINMODE)
        L.GPU_Random_Sampling(None, bare.graph, bare.cache, pool, 5, 2, 0)
        L.get_edge_feature_kernel(None, bare.graph, pool, 0, 4)      # hop 2 is not sampled yet; hop 1 is
        assert "get_edge_feature_kernel: the current pipe's batch left no edge ids for this hop" in err()
        L.get_edge_feature_kernel(None, bare.graph, pool, 0, 2)
        L.d_stream_sync(None)
        K.check()
        # the setter: a width whose flat work space reaches 2^31, the mode during a capture, the table's own refusals
        L.GPUMemoryPool_SetEdgeFeatures(pool, (1 << 31) - 1)
        assert "GPUMemoryPool_SetEdgeFeatures: edge features (GPUMemoryPool_SetEdgeFeatures): NumIds * chunks per row reaches 2^31 work items" in err()
        assert L.GPUMemoryPool_GetEdgeFeatures(pool) == 3
        stream = L.d_stream_create()
        L.GPUCache_SetPreSc(bare.cache, 0)
        assert L.GPUMemoryPool_BeginBatchCapture(pool, stream) == 0
        L.GPUMemoryPool_SetEdgeFeatures(pool, 0)
        assert "GPUMemoryPool_SetEdgeFeatures: the pool is being captured" in err() and L.GPUMemoryPool_GetEdgeFeatures(pool) == 3
        bare.run_batch(0, 0, stream=stream, sync=False, gather=False, plan=False, edge_ids=True, edge_features=True)
        graph = L.GPUMemoryPool_EndBatchCapture(pool, stream)
        K.check()
        assert graph
        L.LegionBatchGraph_Delete(graph)
        L.d_stream_destroy(stream)
        x = np.zeros(4, np.float32)
        assert L.GPUGraphStorage_SetEdgeFeatures(bare.graph, x.ctypes.data, 0, K.LOC_HOST_PAGEABLE) == -1
        assert "GPUGraphStorage_SetEdgeFeatures: dim must be at least 1" in err()
        huge = L.NewGPUMemoryGraphStorage()                          # a graph that says it has 2^40 edges: E * dim * 4 overflows before anything is touched
        info = K.LegionBuildInfo()
        info.partition_count, info.total_num_nodes, info.total_edge_num = 1, bare.V, 1 << 40
        info.csr_node_index, info.csr_dst_node_ids, info.csr_location = bare.indptr_ptr, bare.indices_ptr, K.LOC_DEVICE
        L.GPUGraphStorage_Build(huge, C.byref(info))
        K.check()
        assert L.GPUGraphStorage_SetEdgeFeatures(huge, x.ctypes.data, (1 << 31) - 1, K.LOC_HOST_PAGEABLE) == -1
        assert "GPUGraphStorage_SetEdgeFeatures: the table's size, E * dim * 4 bytes, overflows" in err() and L.GPUGraphStorage_GetEdgeFeatureDim(huge) == 0
        L.GPUGraphStorage_Delete(huge)
        assert L.GPUGraphStorage_SetEdgeFeatures(None, x.ctypes.data, 3, K.LOC_HOST_PAGEABLE) == -1
        assert "GPUGraphStorage_SetEdgeFeatures: null graph, or GPUGraphStorage_Build was not called" in err()
        assert L.GPUGraphStorage_GetEdgeFeatureDim(bare.graph) == 3 and L.GPUGraphStorage_GetEdgeFeatureDim(None) == 0      # the refused replacements kept the table
        assert np.array_equal(bits(bare.edge_feature_rows(0, 5, 7)), bits(table(g, 3)[5:12]))
        bare.set_edge_features(None)
        assert L.GPUGraphStorage_GetEdgeFeatureDim(bare.graph) == 0
    finally:
        L.legion_clear_error()
        bare.close()


def test_a_pool_that_never_saw_the_mode_lists_and_holds_nothing_of_it(K, engines):
    L = K.lib()
    eng = engines.make(0)
    try:
        eng.run_batch(0, 0)
        assert [b["name"] for b in K.pool_scratch(eng.pools[0], 0)] == [t[0] for t in P.EXPECTED_TABLE]
        eng.run_batch(0, 0, edge_ids=True)
        names = [b["name"] for b in K.pool_scratch(eng.pools[0], 0)]
        assert "edge_feat" not in names and "edge_ids" in names      # the edge-id mode alone lists what it lists today
        assert L.GPUMemoryPool_GetEdgeFeatures(eng.pools[0]) == 0 and not L.GPUMemoryPool_GetEdgeFeatureBuffer(eng.pools[0])
        K.check()
    finally:
        eng.close()
