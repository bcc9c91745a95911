"""The edge-id mode (GPUMemoryPool_SetEdgeIds, INTEGRATION.md "Edge ids") as a NumPy statement, shared by the CPU and the GPU tests.  A
helper module, not collected by pytest.

    edge_ids[e] = indptr[src] + p      for the batch's COO edge e, drawn by input row `src` of its hop at neighbour position p
    edge_w[e]   = w[edge_ids[e]]

No rule is restated here: distinctref.run_batch takes every rule's positions from a callable, and this module wraps that callable so that
it also records the [N, f] positions of each hop.  The edges of a hop are its slots with a draw in row-major (ascending slot) order, behind
the edges of the earlier hops -- exactly where src_off / dst_off have them."""
import numpy as np

import distinctref
import seededref
import sharedref
import wdistinctref
import wsharedref
from weightedref import batch_seeds

RULES = ("stream", "distinct", "wdistinct", "shared", "wshared")          # the alias rule ("weighted") hands no ids over
WITHOUT_REPLACEMENT = ("distinct", "wdistinct", "shared", "wshared")
# how capi.Engine.run_batch is told the rule
ENGINE_ARGS = dict(stream=dict(sample="replace"), distinct=dict(sample="distinct"), wdistinct=dict(sample="weighted", weighted_distinct=True),
                   shared=dict(sample="distinct", shared_draws=True), wshared=dict(sample="weighted", weighted_distinct=True, shared_draws=True))
PARTITIONED_RULES = ("stream", "distinct", "shared")                      # the rules that read the clique's fragments


def recording(draw, log):
    """`draw` with the positions of every hop appended to `log`"""
    def wrapped(rows, hop, deg, f):
        p = draw(rows, hop, deg, f)
        log.append(np.array(p, dtype=np.int64, copy=True))
        return p
    return wrapped


def rule_draw(rule, g, first_inputs, W=0, ties=None):
    """The rule's positions callable for ONE run_batch call under draw word W.  g: dict(indptr, indices, w)."""
    if rule == "stream":
        return seededref.replace_positions(W)
    if rule == "distinct":
        return seededref.distinct_positions(W) if W else distinctref.positions
    if rule == "shared":
        return sharedref.shared_positions(g["indptr"], g["indices"], first_inputs, W)
    graph = wdistinctref.Weights(g["indptr"], g["indices"], g["w"])
    if rule == "wdistinct":
        return wdistinctref.wd_positions(graph, first_inputs, W, ties)
    assert rule == "wshared", rule
    return wsharedref.ws_positions(graph, first_inputs, W, ties)


def run_batch(g, rule, all_ids, all_labels, batch_size, counter, fanout, seed=None, round=0, ties=None, feats=None):
    """distinctref.run_batch's batch of the rule -- unseeded under draw word 0, else under seededref's draw word over the round's shuffled
    list -- with two more keys: edge_ids int64 [n_edges] and edge_w float32 [n_edges].  ties: a list that receives the near-tie rows of the
    rules without replacement by weight."""
    indptr = np.asarray(g["indptr"], dtype=np.int64)
    W = 0
    if seed is not None:
        W = seededref.W(seed, round, counter)
        all_ids, all_labels = seededref.shuffled(all_ids, all_labels, seed, round)
    if feats is None:
        feats = g["feats"] if "feats" in g else np.zeros((len(indptr) - 1, 1), np.float32)
    log = []
    draw = recording(rule_draw(rule, g, batch_seeds(all_ids, batch_size, counter), W, ties), log)
    res = distinctref.run_batch(indptr, g["indices"], feats, all_ids, all_labels, batch_size, counter, fanout, draw=draw)
    assert len(log) == len(fanout)
    eids = []
    for h, p in enumerate(log):
        inp = np.asarray(res["draw_counts"][h][0], dtype=np.int64)
        has = res["draws"][h].reshape(p.shape) >= 0
        eids.append((indptr[np.where(inp >= 0, inp, 0)][:, None] + p)[has])          # row-major = ascending slot
    res["edge_ids"] = np.concatenate(eids).astype(np.int64) if eids else np.zeros(0, np.int64)
    res["edge_w"] = np.asarray(g["w"], dtype=np.float32)[res["edge_ids"]]
    res["positions"] = log
    return res


# ---- a served batch against the statement ----------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_edge_ids(want, got, weights=True):
    """the engine's batch `got` with its edge ids against run_batch's `want`: the batch word for word, the ids, and the weights by bit pattern"""
    from conftest import KEYS_NO_FEATURES, assert_batch_equal
    assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
    assert got["edge_ids"].dtype == np.int64
    assert_batch_equal(want, got, keys=("edge_ids",))               # names the first differing edges
    if weights:
        assert_batch_equal(dict(edge_w=bits(want["edge_w"])), dict(edge_w=bits(got["edge_w"])), keys=("edge_w",))
    else:
        assert "edge_w" not in got
