"""Target-edge exclusion on the GPU (GPUMemoryPool_SetLpExclude: k_lp_pairs behind the seed kernel, k_lp_edge_keep behind the last hop),
through the C ABI, against the NumPy statement of tests/lpexref.py.  Everything is integer: every check is array_equal.  The inputs are
those tests/test_lp_exclude_cpu.py proves to hold, at every hop, an excluded edge, a kept edge between two seeds and an edge beyond the
seeds.  Run with `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest

import lpexref as X
import seededref
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu


def assert_marks(got, k, H, *others):
    """the batch's marks equal the statement applied to the batch itself, and to every other statement of the same batch"""
    assert got["edge_keep"].dtype == np.uint8 and got["lp_excluded"].dtype == np.int32 and len(got["lp_excluded"]) == 8
    for b in (got,) + others:
        keep, cnt = X.keep(b, k, H)
        assert np.array_equal(got["edge_keep"], keep), "edge_keep: %d of %d differ" % (int((got["edge_keep"] != keep).sum()), len(keep))
        assert np.array_equal(got["lp_excluded"], cnt), (got["lp_excluded"], cnt)
    return got["lp_excluded"]


def toy_engine(K, k, fan, L, Lab, **kw):
    g = X.graph()
    return make_engine(K, (len(g[0]) - 1, g[2].shape[1], g[0], g[1], g[2]), 3 * k, fan, seeds=dict(train=[(L, Lab)]), **kw)


# ---------------------------------------------------------------------------------------------------
# 1. against the statement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_marks_equal_the_statement_and_nothing_else_moves(K, case):
    """k = 1, 22 (B = 66: past a wave) and 86 (B = 258: past 256); drawn thirds under both samplers and verbatim thirds; three batches.  The
    batch with the mode on is the statement's batch and, bit for bit, the batch with the mode off."""
    k, fan = case["k"], case["fan"]
    H = len(fan)
    st, L, Lab = X.statement(case, X.graph())
    eng = toy_engine(K, k, fan, L, Lab)
    args = X.engine_args(case)
    for counter in X.COUNTERS:
        eng.run_batch(0, counter, per_level=bool(counter & 1), lp_exclude=k, **args)
        got = eng.result(0)
        want = st.run_batch(L, Lab, counter)
        assert_batch_equal(want, got)
        cnt = assert_marks(got, k, H, want)
        assert (cnt[1:H + 1] > 0).all() and K.lib().GPUMemoryPool_GetLpExclude(eng.pools[0]) == k
        eng.run_batch(0, counter, per_level=bool(counter & 1), **args)
        off = eng.result(0)
        assert "edge_keep" not in off and K.lib().GPUMemoryPool_GetLpExclude(eng.pools[0]) == 0
        assert_batch_equal(off, got)
        K.lib().GPUMemoryPool_SetCurrentPipe(eng.pools[0], 0)
        assert not K.lib().GPUMemoryPool_GetEdgeKeepBuffer(eng.pools[0]) and not K.lib().GPUMemoryPool_GetLpExcludedBuffer(eng.pools[0])
    eng.close()


def test_the_alias_rule_needs_no_edge_ids(K):
    """sample="weighted": the one rule that hands no edge ids over marks its edges like every other"""
    k, fan = 22, [5, 4, 3]
    g = X.graph()
    case = dict(k=k, fan=fan, thirds="verbatim", S=1)
    L, Lab = X.case_list(case, g)
    w = (1.0 + np.arange(len(g[1])) % 7).astype(np.float32)
    eng = toy_engine(K, k, fan, L, Lab, edge_weights=w)
    for counter in (0, 2):
        eng.run_batch(0, counter, sample="weighted", lp_exclude=k)
        got = eng.result(0)
        cnt = assert_marks(got, k, len(fan))
        assert (cnt[1:4] > 0).all()
        eng.run_batch(0, counter, sample="weighted")
        assert_batch_equal(eng.result(0), got)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 2. more pairs than a workgroup has lanes, more edges than the grid covers in one trip
# ---------------------------------------------------------------------------------------------------
def test_every_workgroup_loops_and_the_pair_build_spans_several_trips(K):
    """k = 1366 (B = 4098, cap = 8192: k_lp_pairs' 256 lanes insert in six trips) with fan-outs {32, 32}.  k_lp_edge_keep's grid rule,
    restated: one workgroup per 256 lanes x 4 edges of the pool's NumIds, at most 4 per compute unit -- the batch must hold at least twice
    the edges one trip of that grid covers.  A row hands over each neighbour once, so the fan-outs alone do not make the edges: the toy
    graph is built with 24 partners a node (rows of about 54 entries), which gives some four million.  The sampler's own statement of four
    million edges takes seconds and is other tests' business: the marks are held against the statement on the batch the GPU returned."""
    k, fan = 1366, [32, 32]
    g = X.toy_graph(partners=24)
    L = X.triple_list(g[0], g[1], k, 1, seed=9)
    Lab = np.zeros(len(L), np.int32)
    eng = K.Engine(g[0], g[1], g[2], len(g[0]) - 1, g[2].shape[1], dict(train=[(L, Lab)]), 3 * k, fan)
    lib = K.lib()
    one_trip = min((eng.num_ids + 1023) // 1024, 4 * lib.legion_sampler_cu_count()) * 1024
    eng.run_batch(0, 0, gather=False, lp_exclude=k)
    got = eng.result(0, with_features=False)
    n_edges = int(got["ec"][2 + len(fan)])
    assert X.pair_cap(k) == 8192 and k > 256 and n_edges >= 2 * one_trip, (n_edges, one_trip)
    cnt = assert_marks(got, k, len(fan))
    assert (cnt[1:3] > 0).all() and int((got["edge_keep"] == 0).sum()) == cnt[0]
    eng.run_batch(0, 0, gather=False)
    assert_batch_equal(eng.result(0, with_features=False), got, keys=KEYS_NO_FEATURES)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 3. the collision case
# ---------------------------------------------------------------------------------------------------
def test_long_probe_chains_across_the_tables_end(K):
    """tests/lpexref.collision_case (proved on the CPU): ten target pairs with one first slot, three from the table's end, and a pair of two
    seeds that is no target and walks the whole chain.  Rows of at most 4 entries under distinct draws of fan-out 4: every crafted edge is
    in the batch."""
    c = X.collision_case()
    k, fan = c["k"], [4, 4]
    Lab = np.zeros(len(c["list"]), np.int32)
    V = len(c["indptr"]) - 1
    eng = make_engine(K, (V, 4, c["indptr"], c["indices"], c["feats"]), 3 * k, fan, seeds=dict(train=[(c["list"], Lab)]))
    st = seededref.Statement(c["indptr"], c["indices"], c["feats"], 3 * k, fan, None, "distinct", shuffle=False)
    eng.run_batch(0, 0, sample="distinct", lp_exclude=k)
    got = eng.result(0)
    want = st.run_batch(c["list"], Lab, 0)
    assert_batch_equal(want, got)
    assert_marks(got, k, len(fan), want)
    u, v = got["ids"][got["dst_off"]].astype(np.int64), got["ids"][got["src_off"]].astype(np.int64)
    keys = X.pair_keys(u, v)
    for a, b in c["pairs"]:                                         # both directions of every target pair, at both hops
        at = keys == X.pair_keys([a], [b])[0]
        assert at.sum() >= 4 and not got["edge_keep"][at].any() and {(a, b), (b, a)} <= set(zip(u[at].tolist(), v[at].tolist()))
    at = keys == X.pair_keys([c["probe"][0]], [c["probe"][1]])[0]
    assert at.sum() >= 2 and got["edge_keep"][at].all()             # the pair that walks the chain and finds nothing
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 4. odd triples in a padded last batch
# ---------------------------------------------------------------------------------------------------
def odd_list(kind, g, k):
    """two batches of 3 k, the last one padded with its first triple (as lpref.toy_list pads), with one oddity in it"""
    indptr, indices = g[0], g[1]
    V = len(indptr) - 1
    L = X.triple_list(indptr, indices, k, 2, seed=40).reshape(2, 3, k)
    real = k - k // 3
    L[1, :, real:] = L[1, :, :1]                                    # the padding: the first triple, again and again
    if kind == "repeated":
        L[1, :, 5] = L[1, :, 2]
    elif kind == "both_orders":
        L[1, 0, 5], L[1, 1, 5] = L[1, 1, 2], L[1, 0, 2]
    else:
        assert kind == "empty_row"
        L[1, 0, 5] = L[1, 1, 5] = V - 1                             # the isolated node: its positive is itself
    return L.reshape(-1).astype(np.int32)


@pytest.mark.parametrize("kind", ["repeated", "both_orders", "empty_row"])
def test_odd_triples_in_a_padded_last_batch(K, kind):
    """A triple repeated inside a batch, (s, p) and (p, s) in one batch, a source whose row is empty.  (A list with a -1 id in one of its
    thirds is not run: the seed kernel indexes the position table by every list entry it is given, so such a list is outside what
    batch_generator_kernel takes, with the mode or without.  That k_lp_pairs and the statement skip a triple with a negative id is
    held on the CPU, tests/test_lp_exclude_cpu.py.)"""
    k, fan = 22, [5, 4, 3]
    g = X.graph()
    L = odd_list(kind, g, k)
    Lab = (np.arange(len(L)) % 1000).astype(np.int32)
    st = seededref.Statement(g[0], g[1], g[2], 3 * k, fan, None, "distinct", shuffle=False)
    eng = toy_engine(K, k, fan, L, Lab)
    eng.run_batch(0, 1, sample="distinct", lp_exclude=k)
    got = eng.result(0)
    want = st.run_batch(L, Lab, 1)
    assert_batch_equal(want, got)
    cnt = assert_marks(got, k, len(fan), want)
    src, pos = got["ids"][:k], got["ids"][k:2 * k]
    assert cnt[0] > 0 and len(X.targets(got["ids"], k)) == k
    assert len(np.unique(X.targets(got["ids"], k))) < k             # the padding repeats a pair
    if kind == "both_orders":
        assert (src[5], pos[5]) == (pos[2], src[2]) and src[2] != pos[2]
    if kind == "empty_row":
        assert src[5] == pos[5] == len(g[0]) - 2
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 5. the scratch rule, two pipes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["random", "zero", "ones"])
def test_the_marks_do_not_depend_on_what_the_buffers_held(K, fill):
    """lp_pairs, edge_keep and lp_excluded of both pipes filled with random bytes, zeros or 0xFF in front of the batch: the marks are the
    statement's, and edge_keep behind the batch's edges holds exactly what was filled in."""
    case = X.CASES[3 * 2 + 1]                                       # k = 22, {5, 4, 3}, drawn, distinct
    k, fan = case["k"], case["fan"]
    st, L, Lab = X.statement(case, X.graph())
    eng = toy_engine(K, k, fan, L, Lab, pipeline_depth=2)
    lib, pool = K.lib(), eng.pools[0]
    args = X.engine_args(case)
    eng.run_batch(0, 0, lp_exclude=k, **args)                       # the mode is on: the buffers exist
    rng = np.random.RandomState(7)
    filled = {}
    for pipe in (0, 1):
        for b in K.pool_scratch(pool, pipe):
            if b["name"] in ("lp_pairs", "edge_keep", "lp_excluded"):
                assert b["ptr"] and b["per_pipe"] and b["lifetime"] == "batch"
                a = rng.randint(0, 256, size=b["bytes"]).astype(np.uint8) if fill == "random" else np.full(b["bytes"], 0 if fill == "zero" else 0xFF, np.uint8)
                lib.d_copy_h_2_d(b["ptr"], a.ctypes.data, a.nbytes)
                filled[(pipe, b["name"])] = (b["ptr"], a)
    assert len(filled) == 6
    for pipe, counter in ((0, 1), (1, 2)):
        eng.run_batch(0, counter, pipe=pipe, lp_exclude=k, **args)
        got = eng.result(0, pipe=pipe)
        want = st.run_batch(L, Lab, counter)
        assert_batch_equal(want, got)
        assert_marks(got, k, len(fan), want)
        ptr, a = filled[(pipe, "edge_keep")]
        n = len(got["edge_keep"])
        assert len(a) == eng.num_ids and np.array_equal(K.read_dev(ptr, np.uint8, len(a))[n:], a[n:])
    eng.close()


def test_two_pipes_keep_their_own_marks(K):
    case = X.CASES[3 * 2]                                           # k = 22, {5, 4, 3}, drawn, replace
    k, fan = case["k"], case["fan"]
    st, L, Lab = X.statement(case, X.graph())
    eng = toy_engine(K, k, fan, L, Lab, pipeline_depth=2)
    args = X.engine_args(case)
    eng.run_batch(0, 0, pipe=0, lp_exclude=k, **args)
    eng.run_batch(0, 1, pipe=1, lp_exclude=k, **args)
    marks = []
    for pipe in (0, 1):
        got = eng.result(0, pipe=pipe)
        assert_batch_equal(st.run_batch(L, Lab, pipe), got)
        assert_marks(got, k, len(fan))
        marks.append(got["edge_keep"])
    assert not np.array_equal(marks[0], marks[1])
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 6. a recorded batch graph
# ---------------------------------------------------------------------------------------------------
def test_a_recorded_batch_replays_and_is_refused_in_the_other_state(K):
    case = X.CASES[3 * 2]
    k, fan, S = case["k"], case["fan"], case["S"]
    g = X.graph()
    st, L, Lab = X.statement(case, g)
    eng = toy_engine(K, k, fan, L, Lab)
    lib, pool = K.lib(), eng.pools[0]
    args = X.engine_args(case)
    rec = eng.capture_batch(0, lp_exclude=k, **args)
    for rnd, counters in ((0, (0, 2, 1)), (1, (1,))):               # three counters, out of order, and a new round: no new recording
        for counter in counters:
            eng.run_graph(rec, counter, round=rnd)
            got = eng.result(0)
            want = st.run_batch(L, Lab, counter, round=rnd)
            assert_batch_equal(want, got)
            assert_marks(got, k, len(fan), want)
    eng.run_graph(rec, 0, round=0)
    lib.GPUMemoryPool_SetLpExclude(pool, 0)
    with pytest.raises(RuntimeError, match=r"LegionBatchGraph_Launch: the graph was recorded with target-edge exclusion \(GPUMemoryPool_SetLpExclude\)"):
        eng.run_graph(rec, 0)
    off = eng.capture_batch(0, **args)
    lib.GPUMemoryPool_SetLpExclude(pool, k)
    with pytest.raises(RuntimeError, match=r"LegionBatchGraph_Launch: the graph was recorded without target-edge exclusion"):
        eng.run_graph(off, 0)
    lib.GPUMemoryPool_SetLpDraw(pool, 0, None)
    lib.GPUMemoryPool_SetLpExclude(pool, 4 * k)                     # a k of another capacity, and (below) back: the table is reallocated twice
    lib.GPUMemoryPool_SetLpExclude(pool, 0)
    K.check()
    eng._seed_state.pop(0, None)
    eng.run_batch(0, 2, lp_exclude=k, **args)                       # host-driven: the same batch
    got = eng.result(0)
    assert_batch_equal(st.run_batch(L, Lab, 2), got)
    assert_marks(got, k, len(fan))
    with pytest.raises(RuntimeError, match="LegionBatchGraph_Launch: the graph uses a pair table of target-edge exclusion the pool has reallocated since"):
        eng.run_graph(rec, 0)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 7. other modes of batch, two logical GPUs
# ---------------------------------------------------------------------------------------------------
def test_a_validation_batch_keeps_every_edge(K):
    k, fan = 22, [5, 4, 3]
    g = X.graph()
    case = dict(k=k, fan=fan, thirds="verbatim", S=1)
    L, Lab = X.case_list(case, g)
    V = len(g[0]) - 1
    eng = make_engine(K, (V, g[2].shape[1], g[0], g[1], g[2]), 3 * k, fan, seeds=dict(train=[(L, Lab)], valid=[(L, Lab)]))
    eng.run_batch(0, 0, mode=K.VALIDMODE, lp_exclude=k)
    got = eng.result(0)
    assert X.keep(got, k, len(fan))[1][0] > 0                       # as a training batch it would have marks
    assert len(got["edge_keep"]) == got["ec"][2 + len(fan)] > 0 and got["edge_keep"].all() and not got["lp_excluded"].any()
    eng.run_batch(0, 0, mode=K.TRAINMODE, lp_exclude=k)             # ... and has them, on the same pool
    assert assert_marks(eng.result(0), k, len(fan))[0] > 0
    eng.close()


def test_two_logical_gpus_under_the_device_audit(K):
    """G = 2 logical GPUs in one process: both pools mark their own batches; the launches' written arguments are their own GPU's memory
    (the audit's violations fail the test through conftest's fixture, and are counted here)."""
    k, fan = 22, [5, 4]
    g = X.graph()
    lib = K.lib()
    assert lib.legion_audit_enabled()
    lists = [X.triple_list(g[0], g[1], k, 2, seed=60 + d) for d in range(2)]
    labs = [np.zeros(len(x), np.int32) for x in lists]
    V = len(g[0]) - 1
    eng = make_engine(K, (V, g[2].shape[1], g[0], g[1], g[2]), 3 * k, fan, G=2, seeds=dict(train=list(zip(lists, labs))))
    before = (ctypes.c_int64 * 4)()
    lib.legion_audit_counts(before)
    for dev in (0, 1, 0):
        for counter in (0, 1):
            eng.run_batch(dev, counter, sample="distinct", lp_exclude=k)
            got = eng.result(dev)
            want = seededref.Statement(g[0], g[1], g[2], 3 * k, fan, None, "distinct", shuffle=False).run_batch(lists[dev], labs[dev], counter)
            assert_batch_equal(want, got)
            assert assert_marks(got, k, len(fan), want)[0] > 0
    after = (ctypes.c_int64 * 4)()
    lib.legion_audit_counts(after)
    assert after[0] > before[0] and after[1] == before[1] == 0      # checks were made, 0 violations
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 8. the refusals that need a pool with scratch
# ---------------------------------------------------------------------------------------------------
def test_refusals_of_the_generator_and_during_a_capture(K):
    k, fan = 22, [5, 4]
    g = X.graph()
    case = dict(k=k, fan=fan, thirds="verbatim", S=1)
    L, Lab = X.case_list(case, g)
    eng = toy_engine(K, k, fan, L, Lab)
    lib, pool = K.lib(), eng.pools[0]

    def refused(words, fn):
        lib.legion_clear_error()
        fn()
        msg = (lib.legion_last_error() or b"").decode()
        assert all(msg.count(w) == 1 for w in words), (words, msg)
        lib.legion_clear_error()

    gen = lambda bs: lib.batch_generator_kernel(None, eng.noder, eng.cache, pool, bs, 0, 0, 0, K.TRAINMODE)  # noqa: E731
    eng.run_batch(0, 0, lp_exclude=k)
    refused(("batch_generator_kernel", "GPUMemoryPool_SetLpExclude", "the batch size must be three times"), lambda: gen(3 * k - 3))
    lib.GPUMemoryPool_SetLpExclude(pool, 20)                        # 3 batches of 66 seeds: 198 is no multiple of 3 * 20
    refused(("batch_generator_kernel", "GPUMemoryPool_SetLpExclude", "not a multiple of the batch of 3 k"), lambda: gen(60))
    lib.GPUMemoryPool_SetLpExclude(pool, k)
    st = lib.d_stream_create()
    assert lib.GPUMemoryPool_BeginBatchCapture(pool, st) == 0
    refused(("GPUMemoryPool_SetLpExclude: the pool is being captured",), lambda: lib.GPUMemoryPool_SetLpExclude(pool, 0))
    refused(("GPUMemoryPool_SetLpExclude: the pool is being captured",), lambda: lib.GPUMemoryPool_SetLpExclude(pool, 5))
    eng.run_batch(0, 0, stream=st, sync=False, lp_exclude=k)
    rec = lib.GPUMemoryPool_EndBatchCapture(pool, st)
    K.check()
    assert rec and lib.GPUMemoryPool_GetLpExclude(pool) == k
    eng._graphs.append(rec)
    eng.run_batch(0, 1, lp_exclude=k)
    assert assert_marks(eng.result(0), k, len(fan))[0] > 0
    eng.close()
    lib.d_stream_destroy(st)
