"""Weighted sampling without replacement on the GPU (GPUMemoryPool_SetWeightedDistinct on top of the weighted kind / LEGION_SAMPLING=weighted
LEGION_WEIGHTED_DISTINCT=1: k_sample<.., DrawRule::WeightedDistinct> over the graph's retained edge weights), through the C ABI and served, against
the NumPy statement of tests/wdistinctref.py.  Every batch check is array_equal on nc, ec, ids, labels, both COO arrays and the feature
rows, and on the draws the last hop parked -- after asserting that no row of the compared batches is a near tie (wdistinctref: the cap is
zero rows).  Run with `pytest -m gpu`."""
import subprocess

import numpy as np
import pytest

import wdistinctref as R
import weightedref as Wt
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import Statement as DistinctStatement, expected_sums
from harness import K, OUT, SERVER, assert_served_record, child_env, ipc_namespace, make_engine, replay_served, serve_sets, served  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

WORKLOAD, SCALE, B = "products", 0.004, 512
WD = dict(sample="weighted", weighted_distinct=True)


def assert_bits(name, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %d words differ" % (name, int((a != b).sum()))


def last_hop_draws(K, eng, want, dev=0):
    """the draws the last hop parked in the pool's candidate buffer against the statement's"""
    L = K.lib()
    L.SetGPUDevice(dev)
    ref = want["draws"][-1]
    got = K.read_dev(L.GPUMemoryPool_GetCandidateBuffer(eng.pools[dev]), np.int32, len(ref))
    assert np.array_equal(got, ref), "parked draws: %d of %d differ" % (int((got != ref).sum()), len(ref))


# ---------------------------------------------------------------------------------------------------
# graphs and their weights
# ---------------------------------------------------------------------------------------------------
SPECIAL = [0, 1, 2, 4, 5, 6, 24, 25, 26, 63, 64, 65, 129, 300, 3000, 30, 129, 300, 300, 300, 61]
HOLES, HUB, ALL_ZERO, ONE_WEIGHT, THREE_WEIGHTS, TWENTY_WEIGHTS, LATE_HEAVY, WIDE_RANGE = 12, 14, 15, 16, 17, 18, 19, 20


def hand_made_graph():
    """1500 nodes.  Rows 0..20 by hand: the degrees d = 0, 1, f - 1, f, f + 1 of every fan-out of the tests (1, 5, 25, 64), 129 and 300
    (three and five chunks of 64 columns), a hub of 3000, an all-zero row of 30, rows of 129 / 300 / 300 columns of which 1 / 3 / 20 carry
    weight (m <= f < d), a row of 300 whose heavy columns are its last 44 (the last chunk), a row of weights from 1e-30 to 1e30; the others
    0..40 neighbours.  Weights are the synth: source's alphabet, 0 (one in five) or 1..16.  Random neighbours: multi-edges throughout, forty
    columns of the hub hold one id; row 12 has -1 holes with weight."""
    rng = np.random.RandomState(77)
    V = 1500
    deg = rng.randint(0, 41, size=V)
    deg[:len(SPECIAL)] = SPECIAL
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    indices = rng.randint(0, V, size=E).astype(np.int32)
    w = np.where(rng.rand(E) < 0.2, 0, rng.randint(1, 17, size=E)).astype(np.float32)
    row = lambda v: slice(int(indptr[v]), int(indptr[v + 1]))
    w[row(1)] = 1.0
    w[row(ALL_ZERO)] = 0.0
    for v, cols in ((ONE_WEIGHT, [7]), (THREE_WEIGHTS, [0, 64, 128]), (TWENTY_WEIGHTS, list(range(3, 300, 15)))):
        w[row(v)] = 0.0
        w[indptr[v] + np.array(cols)] = 2.0
    w[row(LATE_HEAVY)] = 1.0
    w[indptr[LATE_HEAVY] + 256:indptr[LATE_HEAVY] + 300] = 1e6
    w[row(WIDE_RANGE)] = (10.0 ** np.linspace(-30, 30, 61)).astype(np.float32)
    indices[indptr[HUB] + 100:indptr[HUB] + 140] = indices[indptr[HUB] + 5]      # forty columns of the hub hold one id
    indices[indptr[HOLES] + 3], indices[indptr[HOLES] + 70] = -1, -1
    w[indptr[HOLES] + 3], w[indptr[HOLES] + 70] = 16.0, 16.0
    labels = rng.randint(0, 9, size=V).astype(np.int32)
    return V, indptr, indices, w, labels


@pytest.fixture(scope="module")
def hand():
    V, indptr, indices, w, labels = hand_made_graph()
    F = 4
    feats = np.random.RandomState(1).rand(V, F).astype(np.float32)
    n = len(SPECIAL)
    seeds = np.concatenate([np.arange(n), n + np.random.RandomState(2).permutation(V - n)[:353]]).astype(np.int32)   # the special rows once, in batch 0
    return dict(V=V, F=F, indptr=indptr, indices=indices, w=w, labels=labels, feats=feats, seeds=seeds, graph=R.Weights(indptr, indices, w))


def hand_engine(K, g, fan, Bh=128, **kw):
    kw.setdefault("retain_edge_weights", True)
    return make_engine(K, (g["V"], g["F"], g["indptr"], g["indices"], g["feats"]), Bh, fan, seeds=dict(train=[(g["seeds"], g["labels"][g["seeds"]])]),
                       edge_weights=g["w"], **kw)


@pytest.fixture(scope="module")
def prod(synth):
    """the products graph at scale 0.004 with the synth: source's weights"""
    spec = synth.spec_for(WORKLOAD, scale=SCALE)
    ds = synth.generate(spec)
    w = synth.edge_weights(ds.E)
    return dict(ds=ds, spec=spec, w=w, graph=R.Weights(ds.indptr, ds.indices, w))


def prod_engine(K, prod, fan, **kw):
    kw.setdefault("retain_edge_weights", True)
    return make_engine(K, prod["ds"], B, fan, edge_weights=prod["w"], **kw)


# ---------------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------------
def test_probe_matches_the_statement(K):
    """u_c exact; key_c within 4 ulp of NumPy's (the two logs are each within about 1 ulp, the rest is correctly rounded)."""
    L = K.lib()
    rng = np.random.RandomState(5)
    n = 8192
    rows = rng.randint(0, 2 ** 31 - 1, size=n)
    hops = rng.randint(1, 9, size=n)
    cols = np.concatenate([rng.randint(0, 5000, size=n - 64), np.full(32, 0), np.full(32, 2 ** 31 - 2)])
    word = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64)
    word[:64], word[64:128] = 0, 0xFFFFFFFF
    w = (10.0 ** rng.uniform(-3, 3, size=n)).astype(np.float32)
    w[128:1024] = rng.randint(1, 17, size=896)
    w[1024:1280], w[1280:1536] = np.float32(1e-45), np.finfo(np.float32).max          # the smallest subnormal, FLT_MAX
    assert w[1024] > 0 and (w > 0).all()
    bufs = [K.DevBuf.from_numpy(np.ascontiguousarray(x, dtype=np.int32)) for x in (rows, hops, cols)]
    bufs += [K.DevBuf.from_numpy(word.astype(np.uint32)), K.DevBuf.from_numpy(w)]
    u_out, key_out = K.DevBuf(n * 4), K.DevBuf(n * 8)
    L.legion_weighted_distinct_probe(None, *[b.ptr for b in bufs], u_out.ptr, key_out.ptr, n)
    L.d_stream_sync(None)
    K.check()
    u, key = u_out.to_numpy(np.uint32, n), key_out.to_numpy(np.float64, n)
    for b in bufs + [u_out, key_out]:
        b.free()
    want_u, want_key = R.column_keys(rows, hops, cols, w, word)
    assert np.array_equal(u, want_u)
    ulps = np.abs(key - want_key) / np.spacing(want_key)
    print("key: largest distance %.1f ulp, %d of %d bit-equal" % (ulps.max(), int((key == want_key).sum()), n))
    assert np.isfinite(key).all() and (key > 0).all() and ulps.max() <= 4.0


# ---------------------------------------------------------------------------------------------------
# whole batches through the C ABI
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan", [[1, 1, 1], [5, 5], [25, 5, 5], [64, 64], [5, 25, 25], [64, 64, 1]])
def test_hand_made_rows_equal_the_statement(K, hand, fan):
    """Every special row is a seed of batch 0; the last batch is short (padded -1 sources).  128 seeds: {64, 64} bounds hop 2 by 524 288
    slots and {5, 25, 25} / {64, 64, 1} hop 3 by 400 000 / 524 288, which run the 1024-slot tiles at f = 64, 25 and 1; everything else
    runs the 256-slot ones.  5 and 25 divide neither tile, so rows straddle tile and wave edges."""
    g = hand
    st = R.Statement(g["graph"], g["feats"], 128, fan)
    lab = g["labels"][g["seeds"]]
    last = (len(g["seeds"]) - 1) // 128
    assert len(g["seeds"]) % 128 != 0
    eng = hand_engine(K, g, fan)
    assert eng.has_retained_edge_weights()
    for it in (0, last):
        want = st.run_batch(g["seeds"], lab, it)
        assert st.ties == []
        eng.run_batch(0, it, per_level=bool(it), **WD)
        assert K.lib().GPUMemoryPool_GetSampling(eng.pools[0]) == 2 and K.lib().GPUMemoryPool_GetWeightedDistinct(eng.pools[0]) == 1
        got = eng.result(0)
        assert_batch_equal(want, got)
        last_hop_draws(K, eng, want)
        if it == 0:
            f = fan[0]
            first = want["draws"][0].reshape(-1, f)
            row = lambda v: g["indices"][int(g["indptr"][v]):int(g["indptr"][v + 1])]
            assert (first[0] == -1).all() and (first[ALL_ZERO] == -1).all()
            assert first[ONE_WEIGHT].tolist() == [int(row(ONE_WEIGHT)[7])] + [-1] * (f - 1)
            three = [int(row(THREE_WEIGHTS)[c]) for c in (0, 64, 128)]
            assert first[THREE_WEIGHTS].tolist() == three + [-1] * (f - 3) if f >= 3 else first[THREE_WEIGHTS][0] in three
            heavy = set(row(LATE_HEAVY)[256:].tolist())
            assert sum(int(x) in heavy for x in first[LATE_HEAVY]) >= min(f, 44) - 1          # light columns weigh 10^-6 of a heavy one
    eng.close()


@pytest.mark.parametrize("fan", [[7], [25, 10], [25, 10, 5]])
def test_batches_equal_the_statement(K, prod, fan):
    """First and (short) last batch.  {25, 10, 5} from 512 seeds: hop 3 is bounded by 640 000 slots and runs the 1024-slot tiles, the hops
    before it the 256-slot ones."""
    ds = prod["ds"]
    lab = ds.labels[ds.train]
    st = R.Statement(prod["graph"], ds.features, B, fan)
    eng = prod_engine(K, prod, fan)
    last = (len(ds.train) - 1) // B
    assert last >= 1 and len(ds.train) % B != 0
    for it in (0, last):
        want = st.run_batch(ds.train, lab, it)
        assert st.ties == []
        eng.run_batch(0, it, per_level=bool(it), **WD)
        assert_batch_equal(want, eng.result(0))
        last_hop_draws(K, eng, want)
        if it == 0:
            assert (want["draws"][-1] == -1).any() and int(want["ec"][2 + len(fan)]) > 0
            for h, f in enumerate(fan):                                   # no row draws a neighbour column twice: counts never exceed f
                assert int(want["draw_counts"][h][1].max()) <= f
    eng.close()


def test_seeded_rounds_differ(K, prod):
    ds, fan, seed = prod["ds"], [10, 5], 0xC0FFEE
    lab = ds.labels[ds.train]
    st = R.Statement(prod["graph"], ds.features, B, fan, seed=seed)
    eng = prod_engine(K, prod, fan)
    seen = []
    for rnd in (0, 1):
        for it in (0, 1):
            want = st.run_batch(ds.train, lab, it, round=rnd)
            assert st.ties == []
            eng.run_batch(0, it, seed=seed, round=rnd, **WD)
            assert_batch_equal(want, eng.result(0))
            last_hop_draws(K, eng, want)
            seen.append(want)
    assert not np.array_equal(seen[0]["ids"], seen[2]["ids"]) and not np.array_equal(seen[0]["draws"][0], seen[2]["draws"][0])
    plain = R.Statement(prod["graph"], ds.features, B, fan)
    unseeded = plain.run_batch(ds.train, lab, 0)
    assert plain.ties == []
    eng.run_batch(0, 0, **WD)
    assert_batch_equal(unseeded, eng.result(0))
    assert not np.array_equal(unseeded["draws"][0], seen[0]["draws"][0])
    eng.close()


# ---------------------------------------------------------------------------------------------------
# composition
# ---------------------------------------------------------------------------------------------------
def test_presampling_counts_the_statements_draws(K, prod):
    ds, fan = prod["ds"], [10, 5]
    V, F = ds.spec.V, ds.spec.F
    L = K.lib()
    lab = ds.labels[ds.train]
    st = R.Statement(prod["graph"], ds.features, B, fan)
    eng = prod_engine(K, prod, fan, cache_memory=int(V * F * 4 * 0.15), train_step=2)
    acc = np.zeros(V, np.uint64)
    for it in range(2):
        eng.run_batch(0, it, is_presc=True, **WD)
        want = st.run_batch(ds.train, lab, it)
        assert st.ties == []
        assert_batch_equal(want, eng.result(0, with_features=False), keys=KEYS_NO_FEATURES)
        for inp, cnt in want["draw_counts"]:
            np.add.at(acc, inp[inp >= 0], cnt[inp >= 0].astype(np.uint64))
    L.SetGPUDevice(0)
    assert np.array_equal(K.read_dev(L.GPUCache_GetEdgeAccessedMap(eng.cache, 0), np.uint64, V), acc)
    # behind a cache with CSR fragments the sampler still reads the whole CSR, beside which the weights lie; the cached gather serves the rows
    eng.build_cache(cache_agg_mode=0, node_capacity=V // 8, edge_capacity=V // 3, train_step=2)
    assert L.GPUGraphStorage_FragmentRows(eng.graph, 0) > 0
    for it in (0, 1):
        eng.run_batch(0, it, per_level=bool(it), **WD)
        assert_batch_equal(st.run_batch(ds.train, lab, it), eng.result(0))
    eng.close()


def test_aggregated_hand_offs_on_top(K, prod):
    ds, fan = prod["ds"], [10, 5]
    lab = ds.labels[ds.train]
    st = R.Statement(prod["graph"], ds.features, B, fan)
    eng = prod_engine(K, prod, fan)
    want = st.run_batch(ds.train, lab, 0)
    assert st.ties == []
    for norm in (False, True):
        eng.run_batch(0, 0, agg_last_hop=True, agg_norm="both" if norm else None, per_level=norm, **WD)
        got = eng.result(0)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        n_in, N, S, d = expected_sums(want, fan, norm)
        assert N > 0 and got["features"].shape[0] == n_in
        assert_bits("features", got["features"], want["features"][:n_in])
        assert_bits("nbr_sum", got["nbr_sum"], S)
        if norm:
            assert np.array_equal(got["out_deg"], d)
    eng.close()


def test_batch_graph_replay_on_both_pipes_and_a_flipped_flag_is_refused(K, prod):
    ds, fan = prod["ds"], [10, 5, 3]
    L = K.lib()
    lab = ds.labels[ds.train]
    st = R.Statement(prod["graph"], ds.features, B, fan)
    eng = prod_engine(K, prod, fan, pipeline_depth=2)
    L.GPUCache_SetPreSc(eng.cache, 0)
    graphs = [eng.capture_batch(0, pipe=q, per_level=(q == 0), **WD) for q in (0, 1)]
    assert L.GPUMemoryPool_GetSampling(eng.pools[0]) == 2 and L.GPUMemoryPool_GetWeightedDistinct(eng.pools[0]) == 1
    last = (len(ds.train) - 1) // B
    for n, it in enumerate((0, 1, last, 0)):
        q = n % 2
        want = st.run_batch(ds.train, lab, it)
        assert st.ties == []
        eng.run_graph(graphs[q], it)
        assert_batch_equal(want, eng.result(0, pipe=q))
        eng.run_batch(0, it, pipe=q, **WD)                            # the plain run of the same batch
        assert_batch_equal(want, eng.result(0, pipe=q))
    # a graph recorded in one state of the flag does not launch in the other
    L.GPUMemoryPool_SetWeightedDistinct(eng.pools[0], 0)
    with pytest.raises(RuntimeError, match="recorded with weighted sampling without replacement"):
        eng.run_graph(graphs[0], 0)
    L.legion_clear_error()
    plain = eng.capture_batch(0, pipe=0, sample="weighted")
    L.GPUMemoryPool_SetWeightedDistinct(eng.pools[0], 1)
    with pytest.raises(RuntimeError, match="recorded without weighted sampling without replacement"):
        eng.run_graph(plain, 0)
    L.legion_clear_error()
    eng.run_graph(graphs[1], 1)                                       # back in its own state: replays
    assert_batch_equal(st.run_batch(ds.train, lab, 1), eng.result(0, pipe=1))
    eng.close()


def test_switching_kinds_on_one_pool(K, oracle, prod):
    """replace -> weighted -> weighted without replacement -> distinct -> ...: each batch equals its own reference."""
    ds, fan = prod["ds"], [10, 5]
    lab = ds.labels[ds.train]
    eng = prod_engine(K, prod, fan)
    thr, alias = eng.alias_rows(0)
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    wd = R.Statement(prod["graph"], ds.features, B, fan)
    refs = dict(replace=orc, weighted=Wt.Statement(Wt.Table(ds.indptr, ds.indices, thr, alias), ds.features, B, fan), wd=wd,
                distinct=DistinctStatement(ds.indptr, ds.indices, ds.features, B, fan))
    for it, kind in enumerate(("replace", "weighted", "wd", "distinct", "wd", "weighted", "replace")):
        if kind == "wd":
            eng.run_batch(0, it % 2, **WD)
        else:
            eng.run_batch(0, it % 2, sample=kind)
        assert K.lib().GPUMemoryPool_GetSampling(eng.pools[0]) == dict(replace=0, distinct=1, weighted=2, wd=2)[kind]
        assert K.lib().GPUMemoryPool_GetWeightedDistinct(eng.pools[0]) == int(kind == "wd")
        assert_batch_equal(refs[kind].run_batch(ds.train, lab, it % 2), eng.result(0))
    assert wd.ties == []
    eng.close()


def test_two_logical_gpus_and_dropped_weights(K, hand):
    g, fan = hand, [5, 5]
    sets = dict(train=[(g["seeds"][:100], g["labels"][g["seeds"][:100]])] * 2)
    eng = make_engine(K, (g["V"], g["F"], g["indptr"], g["indices"], g["feats"]), 64, fan, G=2, seeds=sets, edge_weights=g["w"], retain_edge_weights=True)
    st = R.Statement(g["graph"], g["feats"], 64, fan)
    want = st.run_batch(g["seeds"][:100], g["labels"][g["seeds"][:100]], 0)
    assert st.ties == []
    for dev in (0, 1):
        eng.run_batch(dev, 0, **WD)
        assert_batch_equal(want, eng.result(dev))
    eng.set_edge_weights(None)                                           # dropping the table drops the copy
    assert not eng.has_edge_weights() and not eng.has_retained_edge_weights()
    eng.set_edge_weights(g["w"])
    assert eng.has_retained_edge_weights()
    eng.run_batch(0, 0, **WD)
    assert_batch_equal(want, eng.result(0))
    eng.close()


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_a_graph_without_retained_weights_is_refused(K, prod):
    ds, fan = prod["ds"], [10, 5]
    L = K.lib()
    eng = prod_engine(K, prod, fan, retain_edge_weights=False)     # a table, but the weights were not kept
    pool = eng.pools[0]
    assert eng.has_edge_weights() and not eng.has_retained_edge_weights()
    with pytest.raises(ValueError, match="needs the weights kept on the device"):
        eng.run_batch(0, 0, **WD)
    with pytest.raises(ValueError, match="needs the weights kept on the device"):
        eng.capture_batch(0, **WD)
    with pytest.raises(ValueError, match="needs sample='weighted'"):
        eng.run_batch(0, 0, sample="distinct", weighted_distinct=True)
    # ... and by the library itself: through the launcher
    L.GPUMemoryPool_SetSampling(pool, 2)
    L.GPUMemoryPool_SetWeightedDistinct(pool, 1)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
    L.legion_clear_error()
    L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, 10, 2, 0)
    msg = (L.legion_last_error() or b"").decode()
    assert "GPU_Random_Sampling: weighted sampling without replacement (GPUMemoryPool_SetWeightedDistinct)" in msg and "GPUGraphStorage_RetainEdgeWeights" in msg, msg
    L.legion_clear_error()
    L.d_stream_sync(None)
    # ... and through a capture: the recording fails by the same name
    L.GPUCache_SetPreSc(eng.cache, 0)
    s = L.d_stream_create()
    assert L.GPUMemoryPool_BeginBatchCapture(pool, s) == 0
    L.batch_generator_kernel(s, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
    L.GPU_Random_Sampling(s, eng.graph, eng.cache, pool, 10, 2, 0)
    msg = (L.legion_last_error() or b"").decode()
    assert "without retained edge weights" in msg, msg
    assert not L.GPUMemoryPool_EndBatchCapture(pool, s)
    L.legion_clear_error()
    L.GPUMemoryPool_SetWeightedDistinct(pool, 0)
    ref = Wt.Statement(Wt.Table(ds.indptr, ds.indices, *eng.alias_rows(0)), ds.features, B, fan).run_batch(ds.train, ds.labels[ds.train], 0)
    eng.run_batch(0, 0, sample="weighted")                              # the engine stays usable: the plain weighted kind needs no weights
    assert_batch_equal(ref, eng.result(0))
    K.check()
    L.d_stream_destroy(s)
    eng.close()


def test_a_fan_out_of_65_is_refused(K, hand):
    g = hand
    L = K.lib()
    eng = hand_engine(K, g, [65], Bh=64)
    pool = eng.pools[0]
    L.GPUMemoryPool_SetSampling(pool, 2)
    L.GPUMemoryPool_SetWeightedDistinct(pool, 1)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, 64, 0, 0, 0, K.TRAINMODE)
    L.legion_clear_error()
    L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, 65, 2, 0)
    msg = (L.legion_last_error() or b"").decode()
    assert "GPU_Random_Sampling: weighted sampling without replacement (GPUMemoryPool_SetWeightedDistinct) takes a fan-out of at most 64" in msg, msg
    L.legion_clear_error()
    L.d_stream_sync(None)
    want = Wt.Statement(Wt.Table(g["indptr"], g["indices"], *eng.alias_rows(0)), g["feats"], 64, [65]).run_batch(g["seeds"], g["labels"][g["seeds"]], 0)
    eng.run_batch(0, 0, sample="weighted")                              # plain weighted keeps accepting 65
    assert_batch_equal(want, eng.result(0))
    assert L.GPUMemoryPool_GetWeightedDistinct(pool) == 0
    eng.close()


# ---------------------------------------------------------------------------------------------------
# served: the `legion` binary under LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["0", "1"])
def test_server_binary_serves_weighted_distinct_batches(tmp_path, synth, oracle, prod, graph):
    """A synth: source: the server generates the weights on the device (legion_synth_edge_weights == synth.edge_weights), builds its table
    of them and keeps them; the statement replays the schedule."""
    ds, spec, fan, epochs = prod["ds"], prod["spec"], [10, 5], 2
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    meta_line = "synth:%s:%r %d %d %d %d %d %d %d %d %d 0" % (WORKLOAD, SCALE, B, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, 1 << 40, epochs)
    env = dict(LEGION_SAMPLING="weighted", LEGION_WEIGHTED_DISTINCT="1", LEGION_BATCH_GRAPH=graph)
    with served(tmp_path, meta_line, fan, env=env) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    text = srv.log_text()
    assert got["sampling"] == "weighted"                                # the flag is not published: a trainer reads the kind
    assert "Sampling: weighted by edge weight, without replacement" in text and "LEGION_WEIGHTED_DISTINCT=1)" in text
    assert "Edge weights: alias table built in HBM" in text and "Edge weights: kept in HBM beside the table" in text
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B, n_valid=n_valid, n_test=n_test)
    st = R.Statement(prod["graph"], ds.features, B, fan)
    assert got["hops"] == len(fan) and steps[1] > 0 and steps[2] > 0
    for rec, ref, mode, local in replay_served(got, st, sets, ds.labels, steps, epochs, bs):
        assert_served_record(rec, ref, len(fan))
    assert st.ties == []


def test_boot_without_the_weighted_kind_is_refused(tmp_path, synth, prod):
    ds, spec = prod["ds"], prod["spec"]
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write("synth:%s:%r %d %d %d %d %d %d %d %d 1 0" % (WORKLOAD, SCALE, B, spec.V, ds.E, spec.F, spec.n_train, 0, 0, 1 << 40))
    for sampling in (None, "distinct"):
        cenv = child_env(ipc_namespace("wdboot"), LEGION_SAMPLING=sampling, LEGION_WEIGHTED_DISTINCT="1", LEGION_BATCH_GRAPH=None, LEGION_AGG_LAST_HOP=None,
                         LEGION_AGG_NORM=None, LEGION_SAMPLING_SEED=None, LEGION_LP_DRAW=None)
        r = subprocess.run([SERVER, "1", "0", "10,5", meta], env=cenv, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
        said = r.stdout + r.stderr
        assert r.returncode == 1 and "Server_Initialize: LEGION_WEIGHTED_DISTINCT=1 needs LEGION_SAMPLING=weighted" in said, said[-2000:]
