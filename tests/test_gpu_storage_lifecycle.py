"""The life cycle of what the three storages own (csrc/graph_storage.cpp, node_storage.cpp, memory_pool.cpp): a pool that is re-sized, a pool
that is finalised twice and allocated again, the one-copy-per-physical-device rule of the replicas and the alias table with two logical GPUs
on one device, and the device's free memory over whole build / close cycles.  Every batch comparison is array_equal against the same batch
from a fresh engine of that shape.  One process, one GPU.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

from conftest import BATCH_KEYS, assert_batch_equal
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)
from legion1_amd import layout

pytestmark = pytest.mark.gpu

AGG_KEYS = ("nc", "ec", "ids", "labels", "src_off", "dst_off", "features", "nbr_sum", "out_deg")
SMALL, LARGE = (8, [3, 2]), (64, [5, 4, 3])      # one tile and one chunk against 15 tiles of the narrow kind; 2 hops against 3


def random_graph(V, F, max_deg, seed):
    rng = np.random.RandomState(seed)
    deg = rng.randint(0, max_deg + 1, size=V)
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.randint(0, V, size=int(indptr[-1])).astype(np.int32)
    feats = rng.rand(V, F).astype(np.float32)
    labels = rng.randint(0, 9, size=V).astype(np.int32)
    seeds = rng.permutation(V)[:200].astype(np.int32)
    return dict(V=V, F=F, indptr=indptr, indices=indices, feats=feats, labels=labels, seeds=seeds, E=int(indptr[-1]))


@pytest.fixture(scope="module")
def graph():
    return random_graph(3000, 8, 40, 11)


def engine(K, g, B, fan, G=1, **kw):
    return make_engine(K, (g["V"], g["F"], g["indptr"], g["indices"], g["feats"]), B, fan, G=G,
                       seeds=dict(train=[(g["seeds"], g["labels"][g["seeds"]])] * G), **kw)


def two_batches(eng, dev=0):
    """one plain batch, then one aggregated and normalised one (which leaves both modes set on the pool)"""
    eng.run_batch(dev, 0)
    plain = eng.result(dev)
    eng.run_batch(dev, 1, agg_last_hop=True, agg_norm="both")
    return plain, eng.result(dev)


def allocate_scratch(K, eng, B, fan, dev=0):
    """GPUMemoryPool_AllocateScratch on the engine's EXISTING pool, then output buffers of the new NumIds registered the way Engine does it"""
    L, pool = K.lib(), eng.pools[dev]
    L.SetGPUDevice(dev)
    eng.fanout, eng.hops, eng.batch_size = np.asarray(fan, dtype=np.int32), len(fan), int(B)
    L.GPUMemoryPool_AllocateScratch(pool, eng.V, eng.batch_size, eng.fanout.ctypes.data, eng.hops)
    K.check()
    n = eng.num_ids = L.GPUMemoryPool_NumIds(pool)
    for b in eng.out[dev][0].values():
        if b is not None:
            b.free()
    o = eng.out[dev][0] = dict(ids=K.DevBuf(n * 4), labels=K.DevBuf(eng.batch_size * 4), src=K.DevBuf(n * 4), dst=K.DevBuf(n * 4),
                               nc=K.DevBuf(layout.COUNTER_BYTES), ec=K.DevBuf(layout.COUNTER_BYTES), feat=None)
    for name, key in (("SampledIds", "ids"), ("Labels", "labels"), ("AggSrcOf", "src"), ("AggDstOf", "dst"), ("NodeCounter", "nc"), ("EdgeCounter", "ec")):
        getattr(L, "GPUMemoryPool_Set" + name)(pool, o[key].ptr, 0)
    eng.alloc_features()
    eng._seed_state = {}      # the pool's shuffled copy went with its scratch


@pytest.fixture(scope="module")
def fresh(K, graph):
    """the two batches from a fresh pool of either shape (computed once, never changed)"""
    out = {}
    for B, fan in (SMALL, LARGE):
        eng = engine(K, graph, B, fan)
        out[B] = two_batches(eng)
        eng.close()
    return out


# ---------------------------------------------------------------------------------------------------
# 1. re-size
# ---------------------------------------------------------------------------------------------------
def test_a_resized_pool_serves_what_a_fresh_pool_of_that_shape_serves(K, graph, fresh):
    L = K.lib()
    eng = engine(K, graph, *SMALL)
    L.GPUMemoryPool_SetAggLastHop(eng.pools[0], 1)
    L.GPUMemoryPool_SetAggNorm(eng.pools[0], 1)
    K.check()
    for B, fan in (SMALL, LARGE, SMALL):
        allocate_scratch(K, eng, B, fan)
        assert L.GPUMemoryPool_GetAggLastHop(eng.pools[0]) == 1 and L.GPUMemoryPool_GetAggNorm(eng.pools[0]) == 1
        assert L.GPUMemoryPool_GetAggOutDeg(eng.pools[0]), (B, fan)
        assert L.GPUMemoryPool_NumIds(eng.pools[0]) == B * (1 + int(np.cumprod(fan).sum()))
        plain, agg = two_batches(eng)
        assert_batch_equal(fresh[B][0], plain, BATCH_KEYS)
        assert_batch_equal(fresh[B][1], agg, AGG_KEYS)
        assert L.GPUMemoryPool_GetAggOutDeg(eng.pools[0])
        K.check()
    eng.close()
    K.check()


# ---------------------------------------------------------------------------------------------------
# 2. Finalize
# ---------------------------------------------------------------------------------------------------
def test_a_finalised_pool_refuses_batches_and_serves_again_once_allocated(K, graph):
    L = K.lib()
    B, fan = SMALL
    ref_eng = engine(K, graph, B, fan)
    ref_eng.run_batch(0, 0, seed=7)
    ref = ref_eng.result(0)
    ref_eng.close()

    eng = engine(K, graph, B, fan)
    eng.run_batch(0, 0, seed=7)      # the pool holds a shuffled copy when it is finalised
    pool = eng.pools[0]
    L.GPUMemoryPool_Finalize(pool)
    L.GPUMemoryPool_Finalize(pool)
    K.check()

    def refused(who, call):
        L.legion_clear_error()
        call()
        said = (L.legion_last_error() or b"").decode()
        L.legion_clear_error()
        assert (who + ": GPUMemoryPool_AllocateScratch was not called") in said, (who, said)

    L.SetGPUDevice(0)
    refused("batch_generator_kernel", lambda: L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE))
    refused("GPU_Random_Sampling", lambda: L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, int(fan[0]), 2, 0))
    refused("get_feature_kernel_all", lambda: L.get_feature_kernel_all(None, eng.cache, eng.noder, pool, 0, 1))
    L.GPUMemoryPool_SetSampleSeed(pool, 1, 7)
    K.check()

    def begin_round():
        assert L.GPUMemoryPool_BeginRound(None, pool, eng.noder, 0, 0) == -1
    refused("GPUMemoryPool_BeginRound", begin_round)

    allocate_scratch(K, eng, B, fan)
    eng.run_batch(0, 0, seed=7)
    assert_batch_equal(ref, eng.result(0), BATCH_KEYS)
    eng.close()      # GPUMemoryPool_Delete
    K.check()


# ---------------------------------------------------------------------------------------------------
# 3. one copy per physical device, shared by its logical GPUs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [100, 128], ids=["pitched", "dense"])
def test_two_logical_gpus_of_one_device_share_every_copy(K, F):
    L = K.lib()
    for dev in (0, 1):
        L.legion_set_device_map(dev, 0)
    g = random_graph(3000, F, 40, 12)
    V, E = g["V"], g["E"]
    B, fan = 32, [5, 3]
    host = dict(csr_location=K.LOC_HOST_PINNED, features_location=K.LOC_HOST_PINNED)
    plain_eng = engine(K, g, B, fan, G=2, **host)      # never replicates: every read goes to the pinned tables
    plain_eng.run_batch(0, 0)
    ref = plain_eng.result(0)
    plain_eng.close()

    eng = engine(K, g, B, fan, G=2, retain_edge_weights=True, **host)
    assert L.legion_row_pitch(F) == (128 if F == 100 else F)
    for _ in range(2):      # the second call finds every replica in place
        assert L.GPUGraphStorage_ReplicateToDevices(eng.graph) == (V + 1) * 8 + E * 4
        assert L.GPUNodeStorage_ReplicateToDevices(eng.noder) == V * L.legion_row_pitch(F) * 4
        K.check()
    for dev in (0, 1):
        eng.run_batch(dev, 0)
        assert_batch_equal(ref, eng.result(dev), BATCH_KEYS)

    w = np.random.RandomState(3).uniform(0.01, 4.0, size=E).astype(np.float32)
    w[::7] = 0.0
    eng.set_edge_weights(w)
    assert eng.has_edge_weights() and eng.has_retained_edge_weights()
    thr, alias = eng.alias_rows(0)
    thr1, alias1 = eng.alias_rows(1)
    assert np.array_equal(thr, thr1) and np.array_equal(alias, alias1)
    w_bad = w.copy()
    w_bad[[5, E - 3]] = -1.0, float("nan")
    with pytest.raises(RuntimeError, match=r"GPUGraphStorage_SetEdgeWeights: 2 of %d edge weights are negative, NaN or infinite: weights must be finite "
                                            r"and >= 0 \(the earlier table, if any, stays\)" % E):
        eng.set_edge_weights(w_bad)
    assert eng.has_edge_weights() and eng.has_retained_edge_weights()
    for dev in (0, 1):
        again = eng.alias_rows(dev)
        assert np.array_equal(thr, again[0]) and np.array_equal(alias, again[1]), dev
    for kw in (dict(sample="weighted"), dict(sample="weighted", weighted_distinct=True)):
        got = []
        for dev in (0, 1):
            eng.run_batch(dev, 0, **kw)
            got.append(eng.result(dev))
        assert layout.batch_edges(got[0]["ec"], len(fan)) > 0
        assert_batch_equal(got[0], got[1], BATCH_KEYS)      # one table, one draw rule: the two logical GPUs agree
    eng.set_edge_weights(None)
    assert not eng.has_edge_weights() and not eng.has_retained_edge_weights()
    eng.close()
    K.check()


# ---------------------------------------------------------------------------------------------------
# 4. nothing left behind
# ---------------------------------------------------------------------------------------------------
def test_build_and_close_cycles_leave_the_device_memory_where_it_was(K):
    """V = 2^20, F = 4, 4 edges per node, tables in pinned host memory: indptr 8 MiB, indices 16 MiB, features 16 MiB (their replica, at
    the line-aligned pitch of 32 floats, 128 MiB), position table 8 MiB, alias table 32 MiB, retained weights 16 MiB.  A single one of
    them leaked once per cycle costs >= 3 x 8 MiB over the three measured cycles; the bound is 4 MiB (allocator granularity and the
    runtime's own pools are far below it).  The cycle then runs once more inside the measured window with the aggregated last hop, the
    norm and edge ids on, on a pool of 2 048 x [32, 32] (2 097 152 slots, 2 164 736 ids; the 64 seeds make a small batch of it): cand_pipe,
    agg_out_deg, agg_wdraw and edge_w are 8 MiB and more per pipe, edge_ids 16 MiB and cols 8 MiB, so that one of them leaked in that one
    cycle is above the same bound (agg_chunk_cnt, 8 KiB, is below it: the list tests of tests/test_gpu_pool_pipes.py see it go)."""
    import torch
    L = K.lib()
    V, F, D = 1 << 20, 4, 4
    rng = np.random.RandomState(4)
    indptr = np.arange(V + 1, dtype=np.int64) * D
    indices = rng.randint(0, V, size=V * D).astype(np.int32)
    feats = rng.rand(V, F).astype(np.float32)
    w = rng.uniform(0.5, 2.0, size=V * D).astype(np.float32)
    seeds = np.arange(64, dtype=np.int32)
    labels = np.zeros(64, np.int32)

    def cycle(B=32, fan=(3, 2), **modes):
        eng = make_engine(K, (V, F, indptr, indices, feats), B, list(fan), seeds=dict(train=[(seeds, labels)]), retain_edge_weights=True,
                          csr_location=K.LOC_HOST_PINNED, features_location=K.LOC_HOST_PINNED)
        assert L.GPUGraphStorage_ReplicateToDevices(eng.graph) == (V + 1) * 8 + V * D * 4
        assert L.GPUNodeStorage_ReplicateToDevices(eng.noder) == V * L.legion_row_pitch(F) * 4
        eng.set_edge_weights(w)
        eng.run_batch(0, 0, sample="weighted", weighted_distinct=True, **modes)
        assert layout.batch_edges(eng.result(0)["ec"], 2) > 0
        if modes:
            assert {b["name"]: b["bytes"] for b in K.pool_scratch(eng.pools[0]) if b["per_pipe"] and b["ptr"]} == dict(
                cand_pipe=8 << 20, agg_out_deg=2164736 * 4, agg_wdraw=8 << 20, agg_chunk_cnt=8192, edge_ids=2164736 * 8, edge_w=2164736 * 4)
        eng.close()
        K.check()

    modes = dict(B=2048, fan=(32, 32), agg_last_hop=True, agg_norm="both", edge_ids=True)
    cycle()      # warm-up: whatever the runtime keeps for itself it has now
    cycle(**modes)
    L.SetGPUDevice(0)
    L.d_stream_sync(None)
    free_before = torch.cuda.mem_get_info(0)[0]
    for _ in range(3):
        cycle()
    cycle(**modes)
    L.SetGPUDevice(0)
    L.d_stream_sync(None)
    free_after = torch.cuda.mem_get_info(0)[0]
    print("free device memory: %d bytes before, %d after four cycles (%d lost)" % (free_before, free_after, free_before - free_after))
    assert free_before - free_after <= 4 << 20, (free_before, free_after)
