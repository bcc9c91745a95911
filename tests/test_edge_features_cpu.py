"""Edge features (INTEGRATION.md "Edge features": GPUMemoryPool_SetEdgeFeatures, GPUGraphStorage_SetEdgeFeatures), the parts that need no GPU.

The EXPECTED VALUE of the mode is the NumPy statement of tests/efref.py, `X[edge_ids]`.  This file checks what stands around it: the pool's
setter and getter through the library on a pool without scratch -- every refusal by its text with the pool's modes unmoved --, what
GPUMemoryPool_ScratchInfo lists with the mode on and on a pool that never saw it, the synthetic table's closed form, the Engine's own
argument checks, and that the header and capi agree on the new symbols.

Two pool refusals are asserted in tests/test_gpu_edge_features.py, because they need a pool with scratch: the switch during a capture, and a
width whose flat work space (NumIds * chunks per row) reaches 2^31.  One is asserted nowhere, because no pool can reach it: "NumIds * dim * 4
overflows" (int64) needs NumIds * dim >= 2^61, with dim < 2^31 that is NumIds >= 2^30, and a pool gets its NumIds from
GPUMemoryPool_AllocateScratch alone, which at that size allocates more than 40 GB of scratch (a pool without scratch has NumIds = 0).  The
branch stands in front of the 2^31 check so that the product it guards is never formed wrapped."""
import inspect
import os
import re

import numpy as np
import pytest

import scratchpoison as P
from conftest import ROOT

NEW_SYMBOLS = ("GPUGraphStorage_SetEdgeFeatures", "GPUGraphStorage_GetEdgeFeatureDim", "GPUGraphStorage_CopyEdgeFeatureRows", "GPUMemoryPool_SetEdgeFeatures",
               "GPUMemoryPool_GetEdgeFeatures", "GPUMemoryPool_GetEdgeFeatureBuffer", "get_edge_feature_kernel", "get_edge_feature_kernel_all",
               "legion_synth_edge_features")
NEEDS_IDS = "%s: edge features (GPUMemoryPool_SetEdgeFeatures) need edge ids (GPUMemoryPool_SetEdgeIds first, and not off while the mode is on)"
NEGATIVE = "GPUMemoryPool_SetEdgeFeatures: negative edge-feature width (0 = off, dim > 0 = float32 [edges, dim] per batch)"
EDGE_ID_ROWS = [("cols", "count", 4, "hop", False), ("edge_ids", "count_pair", 8, "batch", True), ("edge_w", "float", 4, "batch", True)]


@pytest.fixture
def pool_lib():
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    L.legion_clear_error()
    pool = L.NewGPUMemoryPool(2)
    yield K, L, pool
    L.legion_clear_error()
    L.GPUMemoryPool_Delete(pool)


def modes(L, pool):
    """(edge ids, edge-feature width, aggregated, edge-weighted sums, sampling kind)"""
    return (L.GPUMemoryPool_GetEdgeIds(pool), L.GPUMemoryPool_GetEdgeFeatures(pool), L.GPUMemoryPool_GetAggLastHop(pool), L.GPUMemoryPool_GetAggEdgeWeight(pool),
            L.GPUMemoryPool_GetSampling(pool))


def last_error(L):
    msg = (L.legion_last_error() or b"").decode()
    L.legion_clear_error()
    return msg


def listed(K, pool, pipe=0):
    return [(b["name"], b["kind"], b["elem_bytes"], b["lifetime"], b["per_pipe"]) for b in K.pool_scratch(pool, pipe)]


# ---- the pool's mode ----------------------------------------------------------------------------------------------------
def test_the_getter_returns_what_was_set_and_a_null_pool_is_refused(pool_lib):
    K, L, pool = pool_lib
    assert modes(L, pool) == (0, 0, 0, 0, 0) and L.GPUMemoryPool_GetEdgeFeatures(None) == 0 and not L.legion_last_error()
    L.GPUMemoryPool_SetEdgeFeatures(None, 4)
    assert last_error(L).count("GPUMemoryPool_SetEdgeFeatures: null pool") == 1
    assert not L.GPUMemoryPool_GetEdgeFeatureBuffer(None)
    assert last_error(L).count("GPUMemoryPool_GetEdgeFeatureBuffer: null pool") == 1
    L.GPUMemoryPool_SetEdgeIds(pool, 1)
    for dim in (4, 0, 1, 3, 64, 64, 0, 0):
        L.GPUMemoryPool_SetEdgeFeatures(pool, dim)
        assert not L.legion_last_error() and modes(L, pool) == (1, dim, 0, 0, 0), dim
        assert not L.GPUMemoryPool_GetEdgeFeatureBuffer(pool) and not L.legion_last_error()      # nothing was gathered: no buffer is handed out
    L.GPUMemoryPool_SetEdgeIds(pool, 0)
    L.GPUMemoryPool_SetEdgeFeatures(pool, 0)                                                    # off is acceptable anywhere
    assert not L.legion_last_error() and modes(L, pool) == (0, 0, 0, 0, 0)


def test_every_refusal_by_its_message_with_the_modes_unmoved(pool_lib):
    K, L, pool = pool_lib
    who = "GPUMemoryPool_SetEdgeFeatures"
    L.GPUMemoryPool_SetEdgeFeatures(pool, 4)                        # the mode without edge ids
    assert last_error(L).count(NEEDS_IDS % who) == 1 and modes(L, pool) == (0, 0, 0, 0, 0)
    L.GPUMemoryPool_SetEdgeFeatures(pool, -1)                       # a negative width, with and without edge ids
    assert last_error(L).count(NEGATIVE) == 1 and modes(L, pool) == (0, 0, 0, 0, 0)
    L.GPUMemoryPool_SetEdgeIds(pool, 1)
    L.GPUMemoryPool_SetEdgeFeatures(pool, -(1 << 31))
    assert last_error(L).count(NEGATIVE) == 1 and modes(L, pool) == (1, 0, 0, 0, 0)
    L.GPUMemoryPool_SetEdgeFeatures(pool, 20)
    assert not L.legion_last_error() and modes(L, pool) == (1, 20, 0, 0, 0)
    L.GPUMemoryPool_SetEdgeFeatures(pool, -5)                       # ... and over a mode that is on: the width stays
    assert last_error(L).count(NEGATIVE) == 1 and modes(L, pool) == (1, 20, 0, 0, 0)
    L.GPUMemoryPool_SetEdgeIds(pool, 0)                             # edge ids cannot leave under the mode: the id setter comes second
    assert last_error(L).count(NEEDS_IDS % "GPUMemoryPool_SetEdgeIds") == 1 and modes(L, pool) == (1, 20, 0, 0, 0)
    L.GPUMemoryPool_SetSampling(pool, 2)                            # the alias rule hands no ids and therefore no rows: the edge-id mode's own refusal
    assert "GPUMemoryPool_SetSampling: edge ids (GPUMemoryPool_SetEdgeIds) cannot be handed over under weighted sampling with replacement" in last_error(L)
    assert modes(L, pool) == (1, 20, 0, 0, 0)
    for setter, arg in (("SetSampleDistinct", 1), ("SetAggLastHop", 1), ("SetAggEdgeWeight", 1), ("SetSharedDraws", 1)):      # every other mode leaves it alone
        getattr(L, "GPUMemoryPool_" + setter)(pool, arg)
    L.GPUMemoryPool_SetSampleSeed(pool, 1, 3)
    assert not L.legion_last_error() and modes(L, pool) == (1, 20, 1, 1, 1)
    L.GPUMemoryPool_SetEdgeFeatures(pool, 0)
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 0)
    L.GPUMemoryPool_SetEdgeIds(pool, 0)                             # with the mode off the ids may go
    assert not L.legion_last_error() and modes(L, pool) == (0, 0, 1, 0, 1)


# ---- GPUMemoryPool_ScratchInfo ----------------------------------------------------------------------------------------------
def test_scratch_info_lists_edge_feat_while_the_mode_is_on_and_todays_rows_otherwise(pool_lib):
    """a pool without a device allocates nothing, so it lists the mode's buffer exactly while the mode is on"""
    K, L, pool = pool_lib
    today = [tuple(t) for t in P.EXPECTED_TABLE]
    assert listed(K, pool) == today                                 # never in any of the modes
    L.GPUMemoryPool_SetEdgeIds(pool, 1)
    hop_scratch = [t for t in today if not t[4] and t[0] != "ctl"]  # cols behind the scratch, the two per-pipe rows behind the others, ctl last
    with_ids = hop_scratch + [EDGE_ID_ROWS[0]] + [t for t in today if t[4]] + EDGE_ID_ROWS[1:] + [today[-1]]
    assert listed(K, pool) == with_ids                              # the edge-id mode alone: exactly what it lists today
    L.GPUMemoryPool_SetEdgeFeatures(pool, 20)
    row = ("edge_feat", "float", 4, "batch", True)
    for pipe in (0, 1):
        assert listed(K, pool, pipe) == with_ids[:-1] + [row, today[-1]]
    L.GPUMemoryPool_SetEdgeFeatures(pool, 0)
    assert listed(K, pool) == with_ids
    L.GPUMemoryPool_SetEdgeIds(pool, 0)
    assert listed(K, pool) == today and not L.legion_last_error()
    assert row[1] in P.KINDS and "edge_feat" not in [t[0] for t in P.EXPECTED_TABLE]


# ---- the synthetic table ------------------------------------------------------------------------------------------------------
def test_synth_edge_features_is_a_pure_closed_form_of_row_and_column():
    import legion1_amd.synth as S
    a = S.edge_features(0, 4096, 20)
    assert a.dtype == np.float32 and a.shape == (4096, 20)
    assert np.array_equal(a, S.edge_features(0, 4096, 20))                                  # pure
    assert np.array_equal(a[100:300], S.edge_features(100, 200, 20))                        # a function of the position, not of the range asked for
    assert np.array_equal(a[:, :3], S.edge_features(0, 4096, 3))                            # ... and of the column, not of the width
    assert np.array_equal(S.edge_features_at([7, 7, 4095, 0], 20), a[[7, 7, 4095, 0]])
    assert (a == np.floor(a)).all() and a.min() >= 0 and a.max() < 2 ** 24                  # integers below 2^24: exact in float32
    assert len(np.unique(a[:, 0])) > 4000 and len(np.unique(a[0])) == 20                    # differs across e and across c
    assert (a[1:] != a[:-1]).all(axis=1).sum() > 4000 and (a[:, 1:] != a[:, :-1]).all()
    big = S.edge_features((1 << 32) - 2, 4, 4)                                              # positions beyond 2^32 mix their high word
    assert not np.array_equal(big[2:], S.edge_features(0, 2, 4)) and (big < 2 ** 24).all()


# ---- the Engine's argument checks and the public surface ----------------------------------------------------------------------
def test_the_engine_refuses_the_mode_without_what_it_rests_on():
    """capi.Engine's own argument checks (ValueError, as for agg_edge_weight) are made before the library is called: no engine is needed"""
    import legion1_amd.capi as K
    probe = K.Engine.__new__(K.Engine)
    probe.edge_feature_dim = 4
    with pytest.raises(ValueError, match="edge_features=True needs edge_ids=True"):
        probe._set_modes(0, False, None, "replace", None, 0, None, edge_ids=False, edge_features=True)
    probe.edge_feature_dim = 0
    with pytest.raises(ValueError, match=r"edge_features=True needs the Engine's edge-feature table"):
        probe._set_modes(0, False, None, "replace", None, 0, None, edge_ids=True, edge_features=True)
    probe.E = 10
    with pytest.raises(ValueError, match="a device pointer needs edge_feature_dim >= 1"):
        probe.set_edge_features(12345)
    for bad in (np.zeros((9, 4), np.float32), np.zeros(40, np.float32), np.zeros((10, 4, 1), np.float32)):
        with pytest.raises(ValueError, match=r"edge_features: float32 \[E, dim\] with one row per CSR entry \(10\)"):
            probe.set_edge_features(bad, None if bad.ndim != 3 else 3)


def test_header_and_capi_agree_on_the_new_symbols():
    import legion1_amd.capi as K
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in K._SIGS and hasattr(K.lib(), name), name
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)               # the declarations, without the comments that name the calls
    n_args = {name: len(re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code).group(1).split(",")) for name in NEW_SYMBOLS}
    assert n_args == {name: len(K._SIGS[name][1]) for name in NEW_SYMBOLS}
    for fn in (K.Engine.run_batch, K.Engine.capture_batch):
        assert inspect.signature(fn).parameters["edge_features"].default is False
    for arg in ("edge_features", "edge_feature_dim"):
        assert inspect.signature(K.Engine.__init__).parameters[arg].default is None
    assert "k_gather_edges" in open(os.path.join(ROOT, "legion-1_amd", "csrc", "gather.hip")).read()
