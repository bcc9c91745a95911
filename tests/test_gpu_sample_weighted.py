"""The weighted sampler mode on the GPU (GPUMemoryPool_SetSampling(pool, 2) / LEGION_SAMPLING=weighted: k_sample<.., DrawRule::Weighted> over the alias
table k_build_alias made of GPUGraphStorage_SetEdgeWeights' weights), through the C ABI and served, against the NumPy statement of
tests/weightedref.py fed with the LIBRARY'S OWN table -- which tests/weightedref.py's check_table holds to the weights first.  Every batch
check is array_equal on nc, ec, ids, labels, both COO arrays and the feature rows, and on the draws the last hop parked.  Run with
`pytest -m gpu`."""
import subprocess

import numpy as np
import pytest

import weightedref as Wt
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import Statement as DistinctStatement, expected_sums
from harness import K, OUT, SERVER, assert_served_record, child_env, ipc_namespace, make_engine, replay_served, serve_sets, served  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

WORKLOAD, SCALE, B = "products", 0.004, 512


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
# graphs, their weights, and the library's tables (built once)
# ---------------------------------------------------------------------------------------------------
def hand_made_graph():
    """1500 nodes.  Rows 0..13 by hand: degrees 0, 1, 2, 63, 64, 65, 255, 256, 257 (one lane per row up to 256 neighbours, a wave above), a
    hub of 5000, an all-zero row, a row with a single non-zero weight, a row of equal weights, a row of weights from 1e-30 to 1e30; the
    others 0..40 neighbours with weights 0 (one in five) or 1e-2 .. 1e2.  Random neighbours: multi-edges throughout; one -1 hole with weight."""
    rng = np.random.RandomState(77)
    V = 1500
    deg = rng.randint(0, 41, size=V)
    deg[:14] = [0, 1, 2, 63, 64, 65, 255, 256, 257, 5000, 30, 20, 16, 61]
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    indices = rng.randint(0, V, size=E).astype(np.int32)
    w = np.where(rng.rand(E) < 0.2, 0.0, 10.0 ** rng.uniform(-2, 2, size=E)).astype(np.float32)
    row = lambda v: slice(int(indptr[v]), int(indptr[v + 1]))
    w[row(1)] = 1.0
    w[row(10)] = 0.0                                            # all-zero row
    w[row(11)] = 0.0
    w[indptr[11] + 7] = 0.5                                     # a single non-zero weight
    w[row(12)] = 3.0                                            # equal weights
    w[row(13)] = (10.0 ** np.linspace(-30, 30, 61)).astype(np.float32)
    indices[indptr[9] + 100:indptr[9] + 140] = indices[indptr[9] + 5]      # forty columns of the hub hold one id
    indices[indptr[5] + 3] = -1                                 # a hole
    w[indptr[5] + 3] = 4.0
    labels = rng.randint(0, 9, size=V).astype(np.int32)
    return V, indptr, indices, w, labels


SINGLE_ROW = 11


@pytest.fixture(scope="module")
def hand(K):
    V, indptr, indices, w, labels = hand_made_graph()
    F = 4
    feats = np.random.RandomState(1).rand(V, F).astype(np.float32)
    seeds = np.concatenate([np.arange(14), 14 + np.random.RandomState(2).permutation(V - 14)[:360]]).astype(np.int32)   # the special rows once, in batch 0
    eng = make_engine(K, (V, F, indptr, indices, feats), 128, [7, 3], seeds=dict(train=[(seeds, labels[seeds])]), edge_weights=w)
    thr, alias = eng.alias_rows(0)
    yield dict(V=V, F=F, indptr=indptr, indices=indices, w=w, labels=labels, feats=feats, seeds=seeds, eng=eng, thr=thr, alias=alias,
               table=Wt.Table(indptr, indices, thr, alias))
    eng.close()


@pytest.fixture(scope="module")
def prod(K, synth):
    """the products graph at scale 0.004 with the synth: source's weights, and the table the library builds of them"""
    spec = synth.spec_for(WORKLOAD, scale=SCALE)
    ds = synth.generate(spec)
    w = synth.edge_weights(ds.E)
    eng = make_engine(K, ds, B, [2], edge_weights=w)
    thr, alias = eng.alias_rows(0)
    eng.close()
    return dict(ds=ds, spec=spec, w=w, thr=thr, alias=alias, table=Wt.Table(ds.indptr, ds.indices, thr, alias))


def prod_engine(K, prod, fan, **kw):
    return make_engine(K, prod["ds"], B, fan, edge_weights=prod["w"], **kw)


# ---------------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------------
def test_probe_matches_the_statement(K):
    L = K.lib()
    rng = np.random.RandomState(5)
    n = 4096
    rows = rng.randint(0, 2 ** 31 - 1, size=n)
    hops = rng.randint(1, 9, size=n)
    slots = rng.randint(0, 64, size=n)
    deg = np.concatenate([rng.randint(1, 200, size=n - 96), np.full(32, 1), np.full(32, 2 ** 31 - 1), rng.randint(2 ** 20, 2 ** 31 - 1, size=32)])
    word = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64)
    word[:64], word[64:128] = 0, 0xFFFFFFFF
    word[-96:-80], word[-64:-48] = 0, 0xFFFFFFFF                                    # ... and at d = 1 and d = 2^31 - 1 too
    bufs = [K.DevBuf.from_numpy(np.ascontiguousarray(x, dtype=np.int32)) for x in (rows, hops, slots, deg)]
    bufs.append(K.DevBuf.from_numpy(word.astype(np.uint32)))
    k_out, ub_out = K.DevBuf(n * 4), K.DevBuf(n * 4)
    L.legion_weighted_probe(None, *[b.ptr for b in bufs], k_out.ptr, ub_out.ptr, n)
    L.d_stream_sync(None)
    K.check()
    k, ub = k_out.to_numpy(np.int32, n), ub_out.to_numpy(np.uint32, n)
    for b in bufs + [k_out, ub_out]:
        b.free()
    want_k, want_ub = Wt.slot_draw(rows, hops, slots, deg, word)
    assert np.array_equal(k.astype(np.int64), want_k) and np.array_equal(ub, want_ub)
    assert (k[deg == 1] == 0).all() and (k >= 0).all() and (k.astype(np.int64) < deg).all() and k[deg == 2 ** 31 - 1].max() > 2 ** 28


# ---------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------
def test_table_of_the_hand_made_graph(K, hand):
    L = K.lib()
    g = hand
    indptr, indices, w, thr, alias = g["indptr"], g["indices"], g["w"], g["thr"], g["alias"]
    worst = Wt.check_table(indptr, indices, w, thr, alias)
    print("largest |P - share| of the library's table: %.3g (bound %.3g)" % (worst, Wt.P_BOUND))
    row = lambda v: slice(int(indptr[v]), int(indptr[v + 1]))
    assert (thr[row(10)] == 0).all() and (alias[row(10)] == -1).all()                                  # the all-zero row
    only = int(indices[indptr[SINGLE_ROW] + 7])
    assert (alias[row(SINGLE_ROW)] == only).all() and (np.delete(thr[row(SINGLE_ROW)], 7) == 0).all()  # every draw of this row is that neighbour
    assert (thr[row(12)] == 0xFFFFFFFF).all() and np.array_equal(alias[row(12)], indices[row(12)])     # equal weights: every column keeps itself
    eng = g["eng"]
    assert eng.has_edge_weights()
    eng.set_edge_weights(w)                                                                             # built twice: the same bytes
    thr2, alias2 = eng.alias_rows(0)
    assert np.array_equal(thr, thr2) and np.array_equal(alias, alias2)
    part = eng.alias_rows(0, e0=int(indptr[9]) + 17, n=1000)
    assert np.array_equal(part[0], thr[int(indptr[9]) + 17:][:1000]) and np.array_equal(part[1], alias[int(indptr[9]) + 17:][:1000])
    # refused tables name the cause and leave the earlier table in place
    for bad in (-1.0, float("nan"), float("inf")):
        w_bad = w.copy()
        w_bad[[3, int(indptr[9]) + 4000]] = bad
        with pytest.raises(RuntimeError, match=r"GPUGraphStorage_SetEdgeWeights: 2 of %d edge weights are negative, NaN or infinite" % len(w)):
            eng.set_edge_weights(w_bad)
        assert eng.has_edge_weights()
        thr3, alias3 = eng.alias_rows(0)
        assert np.array_equal(thr, thr3) and np.array_equal(alias, alias3)
    L.legion_clear_error()
    assert L.GPUGraphStorage_CopyAliasRows(eng.graph, 0, len(w) - 1, 2, thr3.ctypes.data, alias3.ctypes.data) == -1
    assert b"entries outside" in (L.legion_last_error() or b"")
    L.legion_clear_error()


def test_two_logical_gpus_hold_identical_tables_and_a_dropped_table_is_gone(K, hand):
    g = hand
    eng = make_engine(K, (g["V"], g["F"], g["indptr"], g["indices"], g["feats"]), 64, [3], G=2,
                      seeds=dict(train=[(g["seeds"][:100], g["labels"][g["seeds"][:100]])] * 2), edge_weights=g["w"])
    for dev in (0, 1):
        thr, alias = eng.alias_rows(dev)
        assert np.array_equal(thr, g["thr"]) and np.array_equal(alias, g["alias"]), dev
    eng.set_edge_weights(None)
    assert not eng.has_edge_weights()
    with pytest.raises(RuntimeError, match="holds no alias table"):
        eng.alias_rows(0)
    with pytest.raises(ValueError, match="needs the Engine's edge_weights"):
        eng.run_batch(0, 0, sample="weighted")
    eng.close()


def test_table_of_the_synth_graph(K, prod):
    ds, w = prod["ds"], prod["w"]
    worst = Wt.check_table(ds.indptr, ds.indices, w, prod["thr"], prod["alias"])
    deg = np.diff(ds.indptr)
    print("largest |P - share|: %.3g; degrees %d..%d" % (worst, deg.min(), deg.max()))
    assert deg.max() > 256 and deg.min() <= 256                                    # both builders ran
    eng = prod_engine(K, prod, [2], G=2)
    for dev in (0, 1):
        thr, alias = eng.alias_rows(dev)
        assert np.array_equal(thr, prod["thr"]) and np.array_equal(alias, prod["alias"]), dev
    eng.close()


# ---------------------------------------------------------------------------------------------------
# whole batches through the C ABI
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan", [[7], [25, 10], [25, 10, 5]])
def test_batches_equal_the_statement(K, prod, fan):
    """First and (short) last batch.  {25, 10, 5} from 512 seeds: hop 3 is bounded by 640 000 slots and runs the 1024-slot tiles, the hops
    before it the 256-slot ones; 7 and 25 divide neither, so rows straddle tile and wave edges."""
    ds = prod["ds"]
    lab = ds.labels[ds.train]
    st = Wt.Statement(prod["table"], ds.features, B, fan)
    eng = prod_engine(K, prod, fan)
    last = (len(ds.train) - 1) // B
    assert last >= 1 and len(ds.train) % B != 0
    for it in (0, last):
        want = st.run_batch(ds.train, lab, it)
        eng.run_batch(0, it, sample="weighted", per_level=bool(it))
        assert K.lib().GPUMemoryPool_GetSampling(eng.pools[0]) == 2 and K.lib().GPUMemoryPool_GetSampleDistinct(eng.pools[0]) == 0
        assert_batch_equal(want, eng.result(0))
        last_hop_draws(K, eng, want)
        if it == 0:
            assert (want["draws"][-1] == -1).any() and int(want["ec"][2 + len(fan)]) > 0          # rows without weight give no edge
            if len(fan) == 3:
                assert B * 25 * 10 * 5 > 256 * 1024 >= B * 25 * 10
    eng.close()


def test_the_hand_made_graph_and_the_row_with_a_single_weight(K, hand):
    """Every special row is a seed of batch 0.  Every draw of the single-weight row is its one weighted neighbour; the all-zero row, the row of
    degree 0 and the padded sources of the short last batch draw nothing."""
    g = hand
    eng, fan = g["eng"], [7, 3]
    st = Wt.Statement(g["table"], g["feats"], 128, fan)
    lab = g["labels"][g["seeds"]]
    last = (len(g["seeds"]) - 1) // 128
    for it in (0, 1, last):
        want = st.run_batch(g["seeds"], lab, it)
        eng.run_batch(0, it, sample="weighted")
        got = eng.result(0)
        assert_batch_equal(want, got)
        last_hop_draws(K, eng, want)
        if it == 0:
            first = want["draws"][0].reshape(-1, 7)
            only = int(g["indices"][g["indptr"][SINGLE_ROW] + 7])
            assert first[SINGLE_ROW].tolist() == [only] * 7 and (first[10] == -1).all() and (first[0] == -1).all()
            src, dst = got["ids"][got["src_off"]], got["ids"][got["dst_off"]]
            e1 = int(got["ec"][3])
            assert (src[:e1][dst[:e1] == SINGLE_ROW] == only).all() and (dst[:e1] == SINGLE_ROW).sum() == 7
    eng.run_batch(0, 0)                                                 # back to the default kind
    assert K.lib().GPUMemoryPool_GetSampling(eng.pools[0]) == 0


def test_seeded_rounds_differ(K, prod):
    ds, fan, seed = prod["ds"], [10, 5], 0xC0FFEE
    lab = ds.labels[ds.train]
    st = Wt.Statement(prod["table"], ds.features, B, fan, seed=seed)
    eng = prod_engine(K, prod, fan)
    seen = []
    for rnd in (0, 1):
        for it in (0, 1):
            want = st.run_batch(ds.train, lab, it, round=rnd)
            eng.run_batch(0, it, sample="weighted", seed=seed, round=rnd)
            assert_batch_equal(want, eng.result(0))
            last_hop_draws(K, eng, want)
            seen.append(want)
    assert not np.array_equal(seen[0]["ids"], seen[2]["ids"]) and not np.array_equal(seen[0]["draws"][0], seen[2]["draws"][0])
    unseeded = Wt.Statement(prod["table"], ds.features, B, fan).run_batch(ds.train, lab, 0)
    eng.run_batch(0, 0, sample="weighted")
    assert_batch_equal(unseeded, eng.result(0))
    assert not np.array_equal(unseeded["draws"][0], seen[0]["draws"][0])
    eng.close()


def test_presampling_counts_the_statements_draws(K, prod):
    ds, fan = prod["ds"], [10, 5]
    V, F = ds.spec.V, ds.spec.F
    L = K.lib()
    lab = ds.labels[ds.train]
    st = Wt.Statement(prod["table"], ds.features, B, fan)
    eng = prod_engine(K, prod, fan, cache_memory=int(V * F * 4 * 0.15), train_step=2)
    acc = np.zeros(V, np.uint64)
    for it in range(2):
        eng.run_batch(0, it, is_presc=True, sample="weighted")
        want = st.run_batch(ds.train, lab, it)
        assert_batch_equal(want, eng.result(0, with_features=False), keys=KEYS_NO_FEATURES)
        for inp, cnt in want["draw_counts"]:
            np.add.at(acc, inp[inp >= 0], cnt[inp >= 0].astype(np.uint64))
    L.SetGPUDevice(0)
    assert np.array_equal(K.read_dev(L.GPUCache_GetEdgeAccessedMap(eng.cache, 0), np.uint64, V), acc)
    # behind a cache with CSR fragments the weighted sampler still reads the whole CSR; the cached gather serves the rows
    eng.build_cache(cache_agg_mode=0, node_capacity=V // 8, edge_capacity=V // 3, train_step=2)
    assert L.GPUGraphStorage_FragmentRows(eng.graph, 0) > 0
    for it in (0, 1):
        eng.run_batch(0, it, sample="weighted", per_level=bool(it))
        assert_batch_equal(st.run_batch(ds.train, lab, it), eng.result(0))
    eng.close()


def test_batch_graph_replay_on_both_pipes(K, prod):
    ds, fan = prod["ds"], [10, 5, 3]
    L = K.lib()
    lab = ds.labels[ds.train]
    st = Wt.Statement(prod["table"], ds.features, B, fan)
    eng = prod_engine(K, prod, fan, pipeline_depth=2)
    L.GPUCache_SetPreSc(eng.cache, 0)
    graphs = [eng.capture_batch(0, pipe=q, sample="weighted", per_level=(q == 0)) for q in (0, 1)]
    assert L.GPUMemoryPool_GetSampling(eng.pools[0]) == 2
    last = (len(ds.train) - 1) // B
    for n, it in enumerate((0, 1, last, 0)):
        q = n % 2
        eng.run_graph(graphs[q], it)
        assert_batch_equal(st.run_batch(ds.train, lab, it), eng.result(0, pipe=q))
    eng.close()


def test_aggregated_hand_offs_on_top(K, prod):
    ds, fan = prod["ds"], [10, 5]
    lab = ds.labels[ds.train]
    st = Wt.Statement(prod["table"], ds.features, B, fan)
    eng = prod_engine(K, prod, fan)
    want = st.run_batch(ds.train, lab, 0)
    for norm in (False, True):
        eng.run_batch(0, 0, sample="weighted", agg_last_hop=True, agg_norm="both" if norm else None, per_level=norm)
        got = eng.result(0)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        n_in, N, S, d = expected_sums(want, fan, norm)
        assert N > 0 and got["features"].shape[0] == n_in
        assert_bits("features", got["features"], want["features"][:n_in])
        assert_bits("nbr_sum", got["nbr_sum"], S)
        if norm:
            assert np.array_equal(got["out_deg"], d)
    eng.close()


def test_switching_kinds_on_one_pool(K, oracle, prod):
    """replace -> weighted -> distinct -> replace: each batch equals its own reference."""
    ds, fan = prod["ds"], [10, 5]
    lab = ds.labels[ds.train]
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    refs = dict(replace=orc, weighted=Wt.Statement(prod["table"], ds.features, B, fan),
                distinct=DistinctStatement(ds.indptr, ds.indices, ds.features, B, fan))
    eng = prod_engine(K, prod, fan)
    for it, kind in enumerate(("replace", "weighted", "distinct", "replace", "weighted")):
        eng.run_batch(0, it % 2, sample=kind)
        assert K.lib().GPUMemoryPool_GetSampling(eng.pools[0]) == ("replace", "distinct", "weighted").index(kind)
        assert_batch_equal(refs[kind].run_batch(ds.train, lab, it % 2), eng.result(0))
    eng.close()


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_a_weighted_pool_over_a_graph_without_weights_is_refused(K, prod):
    ds, fan = prod["ds"], [10, 5]
    L = K.lib()
    eng = make_engine(K, ds, B, fan)                              # no edge_weights
    pool = eng.pools[0]
    with pytest.raises(ValueError, match="needs the Engine's edge_weights"):
        eng.run_batch(0, 0, sample="weighted")
    with pytest.raises(ValueError, match="needs the Engine's edge_weights"):
        eng.capture_batch(0, sample="weighted")
    with pytest.raises(ValueError):
        eng.run_batch(0, 0, sample="heavy")
    # ... and by the library itself: through the launcher
    L.GPUMemoryPool_SetSampling(pool, 2)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
    L.legion_clear_error()
    L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, 10, 2, 0)
    msg = (L.legion_last_error() or b"").decode()
    assert "GPU_Random_Sampling: weighted sampling" in msg and "GPUGraphStorage_SetEdgeWeights" in msg, msg
    L.legion_clear_error()
    L.d_stream_sync(None)
    # ... and through a capture: the recording fails by the same name
    L.GPUCache_SetPreSc(eng.cache, 0)
    st = L.d_stream_create()
    assert L.GPUMemoryPool_BeginBatchCapture(pool, st) == 0
    L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
    L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, 10, 2, 0)
    msg = (L.legion_last_error() or b"").decode()
    assert "GPU_Random_Sampling: weighted sampling" in msg, msg
    assert not L.GPUMemoryPool_EndBatchCapture(pool, st)
    L.legion_clear_error()
    L.GPUMemoryPool_SetSampling(pool, 3)
    assert b"unknown sampling kind" in (L.legion_last_error() or b"")
    L.legion_clear_error()
    L.GPUMemoryPool_SetSampling(pool, 0)
    eng.run_batch(0, 0)                                           # the engine stays usable
    K.check()
    L.d_stream_destroy(st)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# served: the `legion` binary under LEGION_SAMPLING=weighted
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,cache", [("0", False), ("1", False), ("1", True)])
def test_server_binary_serves_weighted_batches(tmp_path, synth, oracle, prod, graph, cache):
    """A synth: source: the server generates the weights on the device (legion_synth_edge_weights == synth.edge_weights) and builds its
    table of them; the statement replays the schedule with the table THIS process' library built of the same weights (held to them by
    check_table in test_table_of_the_synth_graph).  With LEGION_SYNTH_CACHE=1 the feature cache and the CSR fragments are built and the
    sampler still reads the whole CSR."""
    ds, spec, fan, epochs = prod["ds"], prod["spec"], [10, 5], 2
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    budget = int(spec.V * spec.F * 4 * 0.2) if cache else 1 << 40
    meta_line = "synth:%s:%r %d %d %d %d %d %d %d %d %d 0" % (WORKLOAD, SCALE, B, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, budget, epochs)
    env = dict(LEGION_SAMPLING="weighted", LEGION_BATCH_GRAPH=graph, LEGION_SYNTH_CACHE="1" if cache else None)
    with served(tmp_path, meta_line, fan, env=env) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    text = srv.log_text()
    assert got["sampling"] == "weighted" and "Sampling: weighted by edge weight" in text and "(LEGION_SAMPLING=weighted)" in text
    assert "Edge weights: alias table built in HBM" in text and ("cache built on top" in text) == cache
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B, n_valid=n_valid, n_test=n_test)
    st = Wt.Statement(prod["table"], ds.features, B, fan)
    assert got["hops"] == len(fan) and steps[1] > 0 and steps[2] > 0
    for rec, ref, mode, local in replay_served(got, st, sets, ds.labels, steps, epochs, bs):
        assert_served_record(rec, ref, len(fan))


def test_served_from_files(tmp_path, synth, oracle, prod):
    """A dataset directory: without edge_weights the boot is refused by name with exit code 1; with the file the batches are the statement's."""
    ds, spec, fan, epochs = prod["ds"], prod["spec"], [10, 5], 1
    data = tmp_path / "data"
    synth.write_legion_files(ds, str(data))
    meta_line = synth.meta_config_line(ds, str(data), B, 1 << 40, epochs, 0)
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write(meta_line)
    cenv = child_env(ipc_namespace("wboot"), LEGION_SAMPLING="weighted", LEGION_BATCH_GRAPH=None, LEGION_AGG_LAST_HOP=None, LEGION_AGG_NORM=None,
                     LEGION_SAMPLING_SEED=None, LEGION_LP_DRAW=None)
    r = subprocess.run([SERVER, "1", "0", "10,5", meta], env=cenv, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    said = r.stdout + r.stderr
    assert r.returncode == 1 and "Server_Initialize: LEGION_SAMPLING=weighted needs" in said and "edge_weights" in said and "missing or short" in said, said[-2000:]
    prod["w"][:100].astype("<f4").tofile(str(data / "edge_weights"))                     # short
    r = subprocess.run([SERVER, "1", "0", "10,5", meta], env=cenv, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 1 and "missing or short" in r.stdout + r.stderr, (r.stdout + r.stderr)[-2000:]
    prod["w"].astype("<f4").tofile(str(data / "edge_weights"))
    with served(tmp_path, meta_line, fan, env=dict(LEGION_SAMPLING="weighted", LEGION_BATCH_GRAPH=None)) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    assert got["sampling"] == "weighted"
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B)
    st = Wt.Statement(prod["table"], ds.features, B, fan)
    for rec, ref, mode, local in replay_served(got, st, sets, ds.labels, steps, epochs, bs):
        assert_served_record(rec, ref, len(fan))
