"""The distinct-draw sampler mode on the GPU (GPUMemoryPool_SetSampleDistinct / LEGION_SAMPLING=distinct: k_sample<.., DrawRule::Distinct>), through the
C ABI and served, against the NumPy statement of tests/distinctref.py.  Every batch check is array_equal on nc, ec, ids, labels, both COO
arrays and the feature rows; the aggregated hand-offs on top are held bit for bit against tests/aggref.py / tests/gcnref.py fed with the
statement's batch.  Run with `pytest -m gpu`."""
import subprocess

import numpy as np
import pytest

import distinctref as D
from aggref import expected_nbr_sum
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import Statement, random_graph
from gcnref import expected_nbr_sum_norm
from harness import K, OUT, SERVER, assert_served_record, child_env, ipc_namespace, make_engine, replay_served, serve_sets, served  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

H_GRID = (1, 2, 3, 4)
F_GRID = (1, 2, 5, 10, 25, 64)


def d_grid(f):
    return (f + 1, f + 2, 2 * f, 3 * f + 1, 10 * f + 3, 1000 + f)


def assert_bits(name, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %d words differ" % (name, int((a != b).sum()))


def probe(K, rows, hops, deg, f):
    L = K.lib()
    bufs = [K.DevBuf.from_numpy(np.ascontiguousarray(x, dtype=np.int32)) for x in (rows, hops, deg)]
    out = K.DevBuf(len(rows) * f * 4)
    L.legion_distinct_probe(None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, f, out.ptr, len(rows))
    L.d_stream_sync(None)
    K.check()
    got = out.to_numpy(np.int32, len(rows) * f).reshape(len(rows), f)
    for b in bufs + [out]:
        b.free()
    return got


# ---------------------------------------------------------------------------------------------------
# the probe: k_sample's device functions against the statement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", F_GRID)
def test_probe_matches_the_statement_over_the_grid(K, f):
    n = 4000
    for row0 in (0, 3000000):
        rows = np.arange(row0, row0 + n, dtype=np.int64)
        for h in H_GRID:
            for d in d_grid(f):
                got = probe(K, rows, np.full(n, h), np.full(n, d), f)
                assert np.array_equal(got, D.positions(rows, h, np.full(n, d), f)), (h, f, d, row0)


@pytest.mark.parametrize("f", [1, 3, 5, 25, 40, 64])
def test_probe_matches_the_statement_on_random_rows(K, f):
    rng = np.random.RandomState(100 + f)
    n = 50000
    rows = rng.randint(0, 2 ** 31 - 1, size=n).astype(np.int64)
    hops = rng.randint(1, 9, size=n)
    deg = np.concatenate([rng.randint(-1, 4 * f + 3, size=n - 2000), rng.randint(f + 1, 2 ** 31 - 1, size=1990),
                          np.full(10, 2 ** 31 - 1)]).astype(np.int64)
    got = probe(K, rows, hops, deg, f)
    want = D.positions(rows, hops, deg, f)
    assert np.array_equal(got, want)
    assert (got[deg <= 0] == -1).all() and (got[deg > f] >= 0).all()
    assert probe(K, [199999], [1], [2000000000], 5).tolist() == [[1067425008, 1935742059, 137284816, 1563980815, 1023845666]]
    assert probe(K, [12345], [3], [1000], 25)[0, :8].tolist() == [85, 698, 268, 619, 680, 723, 544, 143]


# ---------------------------------------------------------------------------------------------------
# whole batches through the C ABI
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan,B", [([1], 203), ([40], 100), ([64], 64), ([7, 1], 203), ([25, 10], 128), ([25, 10, 5], 64), ([5, 4, 3], 203),
                                   ([40, 3], 90), ([1, 1, 1, 1], 50), ([3, 64], 40)])
def test_toy_graphs(K, fan, B):
    """H = 1..4, fan-outs 1, 40 (above half a wave, rows straddle every tile edge), 64 and the BASELINE triples on graphs with holes, rows of
    degree 0, d <= f, d > f and hubs; first, middle and short last batch; a seed list that repeats seeds."""
    for seed in (0, 1):
        V, F = 500, 6
        indptr, indices, labels = random_graph(seed, V, holes=True)
        feats = np.random.RandomState(seed).rand(V, F).astype(np.float32)
        seeds = np.random.RandomState(seed + 9).permutation(V)[:203].astype(np.int32)
        if seed:
            seeds[7] = seeds[3]
        lab = labels[seeds]
        st = Statement(indptr, indices, feats, B, fan)
        eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(seeds, lab)]))
        for counter in range(min(4, (len(seeds) + B - 1) // B)):
            eng.run_batch(0, counter, sample="distinct", per_level=bool(counter & 1))
            assert K.lib().GPUMemoryPool_GetSampleDistinct(eng.pools[0]) == 1
            assert_batch_equal(st.run_batch(seeds, lab, counter), eng.result(0))
        eng.close()


def test_synthetic_datasets_and_the_mode_switched_on_and_off(K, oracle, small_ds):
    """The generator's graph (multi-edges, skewed degrees).  Between the distinct batches the default mode gives the oracle's batch bit for
    bit: the default draws are untouched by the switch."""
    ds = small_ds
    B = 300
    for fan in ([10, 5], [25, 10, 5], [10, 5, 3]):
        orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
        st = Statement(ds.indptr, ds.indices, ds.features, B, fan)
        lab = ds.labels[ds.train]
        eng = make_engine(K, ds, B, fan)
        last = (len(ds.train) - 1) // B
        for it in (0, 2, last):
            eng.run_batch(0, it)
            assert K.lib().GPUMemoryPool_GetSampleDistinct(eng.pools[0]) == 0
            ref = orc.run_batch(ds.train, lab, it)
            assert_batch_equal(ref, eng.result(0))
            eng.run_batch(0, it, sample="distinct")
            want = st.run_batch(ds.train, lab, it)
            assert_batch_equal(want, eng.result(0))
            assert int(want["nc"][5 + 2 * len(fan)]) != int(ref["nc"][5 + 2 * len(fan)])      # another sampling, not the same batch
        eng.run_batch(0, 1)
        assert_batch_equal(orc.run_batch(ds.train, lab, 1), eng.result(0))
        eng.close()


def test_large_graph_both_tile_sizes(K):
    """1.2 M nodes, {25, 10, 5} from 4000 seeds: hop 1 (100 k slots) runs the 256-slot tiles, hops 2 and 3 (up to 1 M and 5 M slots, far
    beyond 256 Ki) the 1024-slot tiles; 25 and 10 and 5 do not divide either tile, so rows straddle tile and wave edges throughout."""
    V, F, B, fan = 1200000, 4, 4000, [25, 10, 5]
    indptr, indices, labels = random_graph(11, V, max_deg=40, hubs=50, hub_deg=5000)
    feats = np.random.RandomState(1).rand(V, F).astype(np.float32)
    seeds = np.random.RandomState(2).permutation(V)[:2 * B + 77].astype(np.int32)
    lab = labels[seeds]
    st = Statement(indptr, indices, feats, B, fan)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(seeds, lab)]))
    for counter in (0, 1, 2):
        want = st.run_batch(seeds, lab, counter)
        eng.run_batch(0, counter, sample="distinct")
        assert_batch_equal(want, eng.result(0))
        if counter < 2:
            assert len(want["draws"][2]) > 256 * 1024 and len(want["draws"][0]) <= 256 * 1024
    eng.close()


def test_no_pair_repeats_on_a_graph_without_multi_edges(K):
    """Every (input slot, neighbour id) pair of a hop occurs once, and a row of degree d gives min(d, f) edges: read from the GPU's own COO."""
    V, F, B, fan = 3000, 4, 256, [10, 5, 3]
    indptr, indices, labels = random_graph(5, V, max_deg=30, hubs=3, hub_deg=400, simple=True)
    deg = np.diff(indptr)
    feats = np.zeros((V, F), np.float32)
    seeds = np.random.RandomState(3).permutation(V)[:B].astype(np.int32)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(seeds, labels[seeds])]))
    eng.run_batch(0, 0, sample="distinct")
    got = eng.result(0)
    want = D.run_batch(indptr, indices, feats, seeds, labels[seeds], B, 0, fan)
    assert_batch_equal(want, got)
    ids, ec = got["ids"], got["ec"]
    for h, f in enumerate(fan, start=1):
        e0, e1 = (0 if h == 1 else int(ec[1 + h])), int(ec[2 + h])
        src, dst = ids[got["src_off"][e0:e1]], ids[got["dst_off"][e0:e1]]
        inp, cnt = want["draw_counts"][h - 1]
        assert np.array_equal(cnt, np.minimum(deg[inp], f)) and int(cnt.sum()) == e1 - e0
        slot = np.repeat(np.arange(len(inp)), cnt)                   # the input slot of every edge: edges are in slot order
        assert np.array_equal(dst, inp[slot])
        pairs = slot.astype(np.int64) * V + src
        assert len(np.unique(pairs)) == len(pairs), "hop %d repeats a neighbour of an input slot" % h
    eng.close()


def test_batch_graph_replay(K, small_ds):
    """The distinct batch recorded as one hipGraph per pipe and replayed over several batches; the recording keeps its mode."""
    ds = small_ds
    B, fan = 200, [10, 5, 3]
    L = K.lib()
    lab = ds.labels[ds.train]
    st = Statement(ds.indptr, ds.indices, ds.features, B, fan)
    eng = make_engine(K, ds, B, fan, pipeline_depth=2)
    L.GPUCache_SetPreSc(eng.cache, 0)
    graphs = [eng.capture_batch(0, pipe=q, sample="distinct", per_level=(q == 0)) for q in (0, 1)]
    assert L.GPUMemoryPool_GetSampleDistinct(eng.pools[0]) == 1
    last = (len(ds.train) - 1) // B
    for n, it in enumerate((0, 1, 2, 5, last, 0)):
        q = n % 2
        eng.run_graph(graphs[q], it)
        assert_batch_equal(st.run_batch(ds.train, lab, it), eng.result(0, pipe=q))
    eng.close()


def test_presampling_counts_and_partitioned_fragments(K, oracle, small_ds):
    """G = 2 clique.  The pre-sampling batches run the distinct draws: edge_access_time equals the statement's per-row draw counts.  Then a
    cache with CSR fragments and feature shards: the partitioned sampler (a fragment row is the same row) and the cached gather give the
    statement's batch."""
    ds = small_ds
    V, F = ds.spec.V, ds.spec.F
    L = K.lib()
    B, fan, G = 300, [10, 5], 2
    parts = oracle.split_seeds(ds.train, G)
    eng = make_engine(K, ds, B, fan, G=G, cache_memory=int(V * F * 4 * 0.15), train_step=2)
    st = Statement(ds.indptr, ds.indices, ds.features, B, fan)
    for g in range(G):
        acc = np.zeros(V, np.uint64)
        for it in range(2):
            eng.run_batch(g, it, is_presc=True, sample="distinct")
            want = st.run_batch(parts[g], ds.labels[parts[g]], it)
            assert_batch_equal(want, eng.result(g, with_features=False), keys=KEYS_NO_FEATURES)
            for inp, cnt in want["draw_counts"]:
                np.add.at(acc, inp[inp >= 0], cnt[inp >= 0].astype(np.uint64))
        L.SetGPUDevice(g)
        assert np.array_equal(K.read_dev(L.GPUCache_GetEdgeAccessedMap(eng.cache, g), np.uint64, V), acc)
    eng.build_cache(cache_agg_mode=1, node_capacity=V // 8, edge_capacity=V // 3, train_step=2)
    assert L.GPUCache_Kg(eng.cache) == G and L.GPUCache_EdgeCapacity(eng.cache, 0) == V // 3
    for g in range(G):
        L.SetGPUDevice(g)
        assert L.GPUGraphStorage_FragmentRows(eng.graph, g) == V // 3
        for it in (0, 1, 3):
            eng.run_batch(g, it, sample="distinct", per_level=(it != 1))
            assert_batch_equal(st.run_batch(parts[g], ds.labels[parts[g]], it), eng.result(g))
    eng.close()


@pytest.mark.parametrize("fan", [[10], [10, 5], [25, 10, 5]])
def test_aggregated_hand_offs_on_top(K, small_ds, fan):
    """LEGION_AGG_LAST_HOP's sums and LEGION_AGG_NORM's normalised sums over distinct draws: the per-pipe draw buffer holds the distinct
    draws, so nbr_sum / S_w equal aggref / gcnref fed with the statement's batch, bit for bit."""
    ds = small_ds
    B = 300
    lab = ds.labels[ds.train]
    st = Statement(ds.indptr, ds.indices, ds.features, B, fan)
    eng = make_engine(K, ds, B, fan)
    for it in (0, 3):
        want = st.run_batch(ds.train, lab, it)
        eng.run_batch(0, it, sample="distinct", agg_last_hop=True, per_level=(it == 0))
        got = eng.result(0)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        n_in, N, run_dst, S = expected_nbr_sum(want, ds.indptr, ds.indices, fan)
        assert N > 0 and got["features"].shape[0] == n_in
        assert_bits("features", got["features"], want["features"][:n_in])
        assert_bits("nbr_sum", got["nbr_sum"], S)
        eng.run_batch(0, it, sample="distinct", agg_last_hop=True, agg_norm="both", per_level=(it != 0))
        got = eng.result(0)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        n_in, N, run_dst, Sw, d = expected_nbr_sum_norm(want, ds.indptr, ds.indices, fan)
        assert np.array_equal(got["out_deg"], d)
        assert_bits("features", got["features"], want["features"][:n_in])
        assert_bits("nbr_sum (normalised)", got["nbr_sum"], Sw)
    eng.close()


def test_refusals(K, oracle, small_ds):
    """A fan-out above 64 in the distinct mode and a switch while the pool is being captured are sticky errors that name the cause; the
    engine refuses an unknown mode; the default mode still takes f = 65 and the engine stays usable."""
    ds = small_ds
    L = K.lib()
    B, fan = 64, [65, 2]
    lab = ds.labels[ds.train]
    eng = make_engine(K, ds, B, fan)
    pool = eng.pools[0]

    def refused(words, fn):
        L.legion_clear_error()
        fn()
        msg = (L.legion_last_error() or b"").decode()
        assert all(w in msg for w in words), (words, msg)
        L.legion_clear_error()

    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    eng.run_batch(0, 0)                                                    # f = 65 with replacement: served as ever
    assert_batch_equal(orc.run_batch(ds.train, lab, 0), eng.result(0))
    L.GPUMemoryPool_SetSampleDistinct(pool, 1)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
    refused(("GPU_Random_Sampling", "distinct", "at most 64"), lambda: L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, 65, 2, 0))
    L.d_stream_sync(None)
    L.GPUMemoryPool_SetSampleDistinct(pool, 0)
    L.GPUCache_SetPreSc(eng.cache, 0)
    st = L.d_stream_create()
    assert L.GPUMemoryPool_BeginBatchCapture(pool, st) == 0
    refused(("GPUMemoryPool_SetSampleDistinct: the pool is being captured",), lambda: L.GPUMemoryPool_SetSampleDistinct(pool, 1))
    eng.run_batch(0, 0, stream=st, sync=False)
    g = L.GPUMemoryPool_EndBatchCapture(pool, st)
    K.check()
    assert g and L.GPUMemoryPool_GetSampleDistinct(pool) == 0
    eng._graphs.append(g)
    with pytest.raises(ValueError):
        eng.run_batch(0, 0, sample="unique")
    with pytest.raises(ValueError):
        eng.capture_batch(0, sample="")
    refused(("legion_distinct_probe", "1 to 64"), lambda: L.legion_distinct_probe(None, None, None, None, 65, None, 1))
    eng.run_graph((g, st, 0), 1)
    assert_batch_equal(orc.run_batch(ds.train, lab, 1), eng.result(0))
    eng.close()
    L.d_stream_destroy(st)


# ---------------------------------------------------------------------------------------------------
# served: the `legion` binary with LEGION_SAMPLING
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan,graph,cache", [([10, 5], "0", False), ([25, 10, 5], "1", False), ([10, 5], "1", True), ([40], "0", False)])
def test_server_binary_serves_distinct_batches(tmp_path, synth, oracle, fan, graph, cache):
    """LEGION_SAMPLING=distinct, plain op loop and LEGION_BATCH_GRAPH=1, and behind LEGION_SYNTH_CACHE=1 (pre-sampling epoch, cost model,
    partitioned sampler, cached gather): a fresh trainer process reads sampling() == "distinct" and every batch of the schedule (train +
    valid + test steps, two epochs) equals the statement replayed over the served schedule."""
    workload, scale, B, epochs = "products", 0.004, 512, 2
    spec = synth.spec_for(workload, scale=scale)
    ds = synth.generate(spec)
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    budget = int(spec.V * spec.F * 4 * 0.2) if cache else 1 << 40
    meta_line = "synth:%s:%r %d %d %d %d %d %d %d %d %d 0" % (workload, scale, B, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, budget, epochs)
    env = dict(LEGION_SAMPLING="distinct", LEGION_BATCH_GRAPH=graph, LEGION_SYNTH_CACHE="1" if cache else None)
    with served(tmp_path, meta_line, fan, env=env) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    text = srv.log_text()
    assert got["sampling"] == "distinct" and "Sampling: distinct neighbours" in text and "(LEGION_SAMPLING=distinct)" in text
    assert ("cache built on top" in text) == cache
    H = len(fan)
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B, n_valid=n_valid, n_test=n_test)
    st = Statement(ds.indptr, ds.indices, ds.features, B, fan)
    assert got["hops"] == H and steps[1] > 0 and steps[2] > 0
    for rec, ref, mode, local in replay_served(got, st, sets, ds.labels, steps, epochs, bs):
        assert_served_record(rec, ref, H)


@pytest.mark.parametrize("value", [None, "replace"])
def test_server_default_is_replace(tmp_path, synth, oracle, value):
    """Unset and `replace`: the oracle's batches, sampling() == "replace", and the runner logs the mode once."""
    workload, scale, B, epochs, fan = "products", 0.004, 512, 1, [10, 5]
    spec = synth.spec_for(workload, scale=scale)
    ds = synth.generate(spec)
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    meta_line = "synth:%s:%r %d %d %d %d %d %d %d %d %d 0" % (workload, scale, B, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, 1 << 40, epochs)
    with served(tmp_path, meta_line, fan, env=dict(LEGION_SAMPLING=value)) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    text = srv.log_text()
    assert got["sampling"] == "replace" and text.count("Sampling: with replacement") == 1
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B, n_valid=n_valid, n_test=n_test)
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, spec.V, spec.F, B, fan)
    for rec, ref, mode, local in replay_served(got, orc, sets, ds.labels, steps, epochs, bs):
        assert_served_record(rec, ref, len(fan))


@pytest.mark.parametrize("value", ["unique", "1", "Distinct"])
def test_boot_refuses_an_unknown_sampling_mode(tmp_path, synth, value):
    """The `legion` binary refuses a LEGION_SAMPLING it does not know by name, at boot, before it reads the dataset: exit code 1."""
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write(synth.meta_config_line(ds, str(tmp_path / "nowhere") + "/", 512, 1 << 40, 1, 0))
    cenv = child_env(ipc_namespace("boot"), LEGION_SAMPLING=value, LEGION_BATCH_GRAPH=None, LEGION_AGG_LAST_HOP=None, LEGION_AGG_NORM=None)
    r = subprocess.run([SERVER, "1", "0", "10,5", meta], env=cenv, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    said = r.stdout + r.stderr
    assert r.returncode == 1 and "Server_Initialize:" in said and "LEGION_SAMPLING=%s is not a known sampling mode" % value in said, said[-2000:]
    assert "`replace`" in said and "`distinct`" in said
