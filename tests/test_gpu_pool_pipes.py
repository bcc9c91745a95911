"""The memory pool's per-pipe record (GPUMemoryPool::Pipe) and its table of per-pipe buffers (pool_pipe_buffers, csrc/memory_pool.cpp) on a
pool that owns scratch: what is allocated when, what survives a mode switched off, what Finalize and AllocateScratch do to the list, and
that two pipes never see each other's buffers.  The presence literals were recorded from the library before the per-pipe vectors became one
record and one table; every batch comparison is array_equal (floats by bit pattern) against the NumPy statements of tests/eidref.py,
tests/edgeaggref.py and tests/gcnref.py.  Graph and shape: tests/drawrulecases.py, narrow (64 x [5, 4]).  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import drawrulecases as D
import eidref as R
import poolpipes as W
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from edgeaggref import expected_nbr_sum_edge
from eidref import assert_edge_ids, bits
from gcnref import expected_nbr_sum_norm
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

B, FAN = D.SHAPES["narrow"]
EDGE_ON = dict(agg_last_hop=True, edge_ids=True, agg_edge_weight=True)
NORM_ON = dict(agg_last_hop=True, agg_norm="both")

# what AllocateScratch allocates whatever the modes are
BASE = {"pos_map", "cand", "aux2[0]", "aux2[1]", "tile_edge", "tile_node", "tile_pre", "chunk_tot", "hop_state", "cache_search_buffer", "row_ptr",
        "agg_src_ids", "tmp_part_ind", "tmp_part_off", "ctl"}
EDGE = {"cols", "edge_ids", "edge_w"}
# the listed buffers with a pointer behind each step of poolpipes.STEPS: a buffer is there once any state since AllocateScratch wanted it
PRESENT = {
    "fresh": BASE,
    "edge ids on": BASE | EDGE,
    "edge ids off": BASE | EDGE,
    "aggregated last hop": BASE | EDGE | {"cand_pipe"},
    "norm": BASE | EDGE | {"cand_pipe", "agg_out_deg", "agg_wdraw", "agg_chunk_cnt"},
    "edge-weighted sums": BASE | EDGE | {"cand_pipe", "agg_out_deg", "agg_wdraw", "agg_chunk_cnt"},
    "everything off": BASE | EDGE | {"cand_pipe", "agg_out_deg", "agg_wdraw", "agg_chunk_cnt"},
}
# ... and behind AllocateScratch on a pool in the edge-weighted sums' modes: exactly what they want -- the degrees are the norm's
PRESENT_EDGE_WEIGHTED = BASE | EDGE | {"cand_pipe", "agg_wdraw", "agg_chunk_cnt"}
NEVER_SAW_EDGE_IDS = ["pos_map", "cand", "aux2[0]", "aux2[1]", "tile_edge", "tile_node", "tile_pre", "chunk_tot", "hop_state", "cache_search_buffer", "row_ptr",
                      "agg_src_ids", "tmp_part_ind", "tmp_part_off", "cand_pipe", "agg_out_deg", "agg_wdraw", "agg_chunk_cnt", "ctl"]
WITH_EDGE_IDS = ["pos_map", "cand", "aux2[0]", "aux2[1]", "tile_edge", "tile_node", "tile_pre", "chunk_tot", "hop_state", "cache_search_buffer", "row_ptr",
                 "agg_src_ids", "tmp_part_ind", "tmp_part_off", "cols", "cand_pipe", "agg_out_deg", "agg_wdraw", "agg_chunk_cnt", "edge_ids", "edge_w", "ctl"]


@pytest.fixture(scope="module")
def g():
    return D.graph()


@pytest.fixture(scope="module")
def want(g):
    """counter -> (the eidref batch of the reference's draws, its edge-weighted sums, its normalised sums and block out-degrees): computed
    once, shared, never changed"""
    seeds = D.seed_list("narrow")
    out = {}
    for counter in D.COUNTERS:
        ref = R.run_batch(g, "stream", seeds, g["labels"][seeds], B, counter, FAN)
        _, _, _, S_norm, d = expected_nbr_sum_norm(ref, g["indptr"], g["indices"], FAN)
        out[counter] = (ref, expected_nbr_sum_edge(ref, g["indptr"], g["indices"], FAN), S_norm, d)
    return out


def engine(K, g):
    seeds = D.seed_list("narrow")
    return make_engine(K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, FAN, seeds=dict(train=[(seeds, g["labels"][seeds])]),
                       edge_weights=g["w"], retain_edge_weights=True, pipeline_depth=2)


def assert_edge_weighted(name, want, got):
    ref, (n_in, N, _, S), _, _ = want
    assert_edge_ids(ref, got)                              # the batch word for word, edge_ids, edge_w by bit pattern
    assert N > 0 and got["features"].shape == (n_in, D.F) and np.array_equal(bits(got["features"]), bits(ref["features"][:n_in])), name
    assert got["nbr_sum"].shape == S.shape and not np.isnan(S).any() and np.array_equal(bits(got["nbr_sum"]), bits(S)), name


def assert_normalised(name, want, got):
    ref, (n_in, N, _, _), S, d = want
    assert_batch_equal(ref, got, keys=KEYS_NO_FEATURES)
    assert got["out_deg"].dtype == np.int32 and np.array_equal(got["out_deg"], d), name
    assert np.array_equal(bits(got["features"]), bits(ref["features"][:n_in])), name
    assert got["nbr_sum"].shape == S.shape and not np.isnan(S).any() and np.array_equal(bits(got["nbr_sum"]), bits(S)), name


def pointers(K, pool):
    """({(name, pipe or None): pointer} of every listed buffer with one, the two pipes' name lists)"""
    there, names = {}, []
    for pipe in (0, 1):
        rows, ptrs = W.listed(K, pool, pipe)
        names.append([r[0] for r in rows])
        for r in rows:
            if ptrs[r[0]]:
                key = (r[0], pipe if r[4] else None)
                assert there.setdefault(key, ptrs[r[0]]) == ptrs[r[0]], key          # what is not per pipe is one buffer in both lists
    return there, names


def test_the_modes_life_cycle_on_a_pool_that_owns_scratch(K, g, want):
    L = K.lib()
    eng = engine(K, g)
    pool = eng.pools[0]
    L.SetGPUDevice(0)
    try:
        seen = {}
        for step in W.walk(K, pool):
            there, names = pointers(K, pool)
            for pipe in (0, 1):
                assert {n for n, q in there if q in (None, pipe)} == PRESENT[step], (step, pipe)
                assert names[pipe] == (WITH_EDGE_IDS if step != "fresh" else NEVER_SAW_EDGE_IDS), (step, pipe)   # cols remembers the mode until the scratch goes
            assert len(set(there.values())) == len(there), step                      # no two entries share a pointer, across both pipes
            assert all(there[k] == v for k, v in seen.items()), step                 # once there, a pointer keeps its value
            seen = there
        assert {q for n, q in seen if n in ("cand_pipe", "edge_ids", "edge_w", "agg_out_deg", "agg_wdraw", "agg_chunk_cnt")} == {0, 1}

        L.GPUMemoryPool_Finalize(pool)                                               # every mode is off: the list of a pool that never saw edge ids
        K.check()
        there, names = pointers(K, pool)
        assert there == {} and names == [NEVER_SAW_EDGE_IDS] * 2
        for q in (0, 1):
            L.GPUMemoryPool_SetCurrentPipe(pool, q)
            assert not L.GPUMemoryPool_GetEdgeIdBuffer(pool) and not L.GPUMemoryPool_GetEdgeWeightBuffer(pool) and not L.GPUMemoryPool_GetAggOutDeg(pool)
        for setter in ("GPUMemoryPool_SetAggLastHop", "GPUMemoryPool_SetEdgeIds", "GPUMemoryPool_SetAggEdgeWeight"):   # without scratch: nothing is allocated
            getattr(L, setter)(pool, 1)
            K.check()
        there, names = pointers(K, pool)
        assert there == {} and names == [WITH_EDGE_IDS] * 2

        L.GPUMemoryPool_AllocateScratch(pool, eng.V, eng.batch_size, eng.fanout.ctypes.data, eng.hops)
        K.check()
        there, names = pointers(K, pool)
        for pipe in (0, 1):
            assert {n for n, q in there if q in (None, pipe)} == PRESENT_EDGE_WEIGHTED, pipe
        assert names == [WITH_EDGE_IDS] * 2 and len(set(there.values())) == len(there)
        for q in (0, 1):                                                             # no batch has run: no weights to hand over yet, and no degrees ever
            L.GPUMemoryPool_SetCurrentPipe(pool, q)
            assert L.GPUMemoryPool_GetEdgeIdBuffer(pool) == there[("edge_ids", q)]
            assert not L.GPUMemoryPool_GetEdgeWeightBuffer(pool) and not L.GPUMemoryPool_GetAggOutDeg(pool)

        eng.run_batch(0, 0, **EDGE_ON)
        assert_edge_weighted("behind Finalize and AllocateScratch", want[0], eng.result(0))
        assert pointers(K, pool)[0] == there                                         # the batch allocated nothing
        L.GPUMemoryPool_SetCurrentPipe(pool, 0)
        assert L.GPUMemoryPool_GetEdgeWeightBuffer(pool) == there[("edge_w", 0)]
        L.GPUMemoryPool_SetCurrentPipe(pool, 1)
        assert not L.GPUMemoryPool_GetEdgeWeightBuffer(pool)                         # pipe 1 has run no batch
    finally:
        L.legion_clear_error()
        eng.close()
    K.check()


@pytest.mark.parametrize("modes", ["edge_weighted", "normalised"])
def test_two_pipes_keep_their_own_batches(K, g, want, modes):
    """batch 0 on pipe 0, then batch 1 on pipe 1, then pipe 0 is read back: every per-pipe buffer the modes use is in the comparison -- the
    draws and their weights through the sums, agg_out_deg, edge_ids and edge_w as they are handed over"""
    eng = engine(K, g)
    try:
        kw, check = (EDGE_ON, assert_edge_weighted) if modes == "edge_weighted" else (NORM_ON, assert_normalised)
        for pipe, counter in ((0, 0), (1, 1)):
            eng.run_batch(0, counter, pipe=pipe, **kw)
        assert not np.array_equal(want[0][0]["ids"], want[1][0]["ids"])              # two different batches
        for pipe, counter in ((0, 0), (1, 1), (0, 0)):
            check("pipe %d" % pipe, want[counter], eng.result(0, pipe=pipe))
    finally:
        eng.close()
    K.check()
