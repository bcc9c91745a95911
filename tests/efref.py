"""The edge-feature mode (GPUMemoryPool_SetEdgeFeatures, INTEGRATION.md "Edge features") as a NumPy statement, shared by the CPU and the GPU
tests.  A helper module, not collected by pytest.

    edge_feat[e, :] = X[edge_ids[e], :]      for the batch's COO edge e, X the graph's float32 [E, dim] table in CSR order

and nothing else: edge_ids themselves are held to tests/eidref.py by tests/test_gpu_edge_ids.py."""
import numpy as np


def expected_edge_feat(X, edge_ids):
    X = np.asarray(X, dtype=np.float32)
    assert X.ndim == 2
    return X[np.asarray(edge_ids, dtype=np.int64)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_edge_feat(X, got):
    """the engine's batch `got` (capi.Engine.result()) against the statement over its own edge ids: shape, dtype, and every bit"""
    want = expected_edge_feat(X, got["edge_ids"])
    assert got["edge_feat"].dtype == np.float32 and got["edge_feat"].shape == want.shape == (len(got["src_off"]), X.shape[1])
    if not np.array_equal(bits(want), bits(got["edge_feat"])):
        bad = np.nonzero((bits(want) != bits(got["edge_feat"])).any(axis=1))[0]
        raise AssertionError("edge_feat: %d of %d rows differ, first at edges %s (ids %s): %s vs %s" % (
            len(bad), len(want), bad[:3], got["edge_ids"][bad[:3]], want[bad[:3]], got["edge_feat"][bad[:3]]))
