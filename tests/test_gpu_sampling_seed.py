"""Seeded sampling on the GPU (GPUMemoryPool_SetSampleSeed / GPUMemoryPool_BeginRound / LEGION_SAMPLING_SEED: the seeded k_sample, k_seed
on the round's shuffled list, k_shuffle_seeds), through the C ABI and served, against the NumPy statement of tests/seededref.py.  Every
batch check is array_equal on nc, ec, ids, labels, both COO arrays and the feature rows.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import seededref as R
from aggref import expected_nbr_sum
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import random_graph
from gcnref import expected_nbr_sum_norm
from harness import K, OUT, assert_served_record, make_engine, replay_served, serve_sets, served  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

S_GRID = (0, 1, 12345, 0xFFFFFFFF)
R_GRID = (0, 1, 7)
C_GRID = (0, 1, 40)
F_GRID = (1, 2, 5, 10, 25, 64)
N_LIST = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 203, 256, 257, 1000, 4097, 65537, 100003)
NARROW_SLOTS = 256 * 1024      # kNarrowSlots (csrc/internal.h)


def d_grid(f):
    return (f + 1, f + 2, 2 * f, 3 * f + 1, 10 * f + 3, 1000 + f)


def assert_bits(name, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %d words differ" % (name, int((a != b).sum()))


def dev_call(K, fn, arrays, n_out):
    """fn(*device copies of `arrays`, out) -> int32 [n_out]"""
    L = K.lib()
    bufs = [K.DevBuf.from_numpy(np.ascontiguousarray(x, dtype=np.int32)) for x in arrays]
    out = K.DevBuf(n_out * 4)
    fn([b.ptr for b in bufs], out.ptr)
    L.d_stream_sync(None)
    K.check()
    got = out.to_numpy(np.int32, n_out)
    for b in bufs + [out]:
        b.free()
    return got


# ---------------------------------------------------------------------------------------------------
# the probes: the kernels' device functions against the statement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", S_GRID)
def test_replace_probe_matches_the_statement(K, S):
    L = K.lib()
    rng = np.random.RandomState(S % 1000)
    n = 3000
    idx = np.concatenate([[0, 1, 2, 999999, 2 ** 31 - 2, 2 ** 31 - 3, 2 ** 30], rng.randint(0, 2 ** 31 - 1, size=n - 7)]).astype(np.int64)
    deg = np.concatenate([[1000] * 4, [1, 2 ** 31 - 1, 7], rng.randint(1, 5000, size=n - 1007), rng.randint(1, 2 ** 31 - 1, size=1000)]).astype(np.int64)
    for r in R_GRID:
        for c in C_GRID:
            got = dev_call(K, lambda p, out: L.legion_seeded_rng_probe(None, S, r, c, p[0], p[1], out, n), (idx, deg), n)
            assert np.array_equal(got, R.replace_index(idx, deg, R.W(S, r, c))), (S, r, c)
    got = dev_call(K, lambda p, out: L.legion_seeded_rng_probe(None, 12345, 3, 2, p[0], p[1], out, 4), ([0, 1, 2, 999999], [1000] * 4), 4)
    assert got.tolist() == [130, 473, 774, 996]


@pytest.mark.parametrize("f", F_GRID)
def test_distinct_probe_matches_the_statement(K, f):
    L = K.lib()
    n = 600
    rng = np.random.RandomState(f)
    rows = np.concatenate([np.arange(200), np.arange(3000000, 3000200), rng.randint(0, 2 ** 31 - 1, size=200)]).astype(np.int64)
    hops = rng.randint(1, 5, size=n)
    deg = np.concatenate([np.resize(np.array(d_grid(f)), 500), rng.randint(-1, f + 1, size=90), rng.randint(f + 1, 2 ** 31 - 1, size=9), [2 ** 31 - 1]]).astype(np.int64)
    for S in S_GRID:
        for r in R_GRID:
            for c in C_GRID:
                got = dev_call(K, lambda p, out: L.legion_seeded_distinct_probe(None, S, r, c, p[0], p[1], p[2], f, out, n), (rows, hops, deg), n * f)
                assert np.array_equal(got.reshape(n, f), R.distinct_positions(R.W(S, r, c))(rows, hops, deg, f)), (S, r, c, f)
    if f == 5:
        got = dev_call(K, lambda p, out: L.legion_seeded_distinct_probe(None, 12345, 3, 2, p[0], p[1], p[2], 5, out, 2), ([0, 199999], [1, 1], [6, 2000000000]), 10)
        assert got.tolist() == [1, 0, 3, 4, 2, 213940653, 337251786, 41287048, 39838029, 1676941256]


@pytest.mark.parametrize("S", S_GRID)
def test_perm_probe_matches_the_statement(K, S):
    L = K.lib()
    for r in R_GRID:
        for n in N_LIST:
            got = dev_call(K, lambda p, out: L.legion_perm_probe(None, S, r, n, out), (), n)
            assert np.array_equal(got, R.perm(n, R.Ks(S, r))), (S, r, n)
    got = dev_call(K, lambda p, out: L.legion_perm_probe(None, 12345, 3, 203, out), (), 203)
    assert got[:8].tolist() == [97, 64, 43, 85, 38, 200, 142, 99]


# ---------------------------------------------------------------------------------------------------
# whole batches through the C ABI
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", ["replace", "distinct"])
@pytest.mark.parametrize("fan", [[1], [40], [7, 1], [25, 10], [25, 10, 5], [5, 4, 3]], ids=lambda f: "-".join(map(str, f)))
def test_toy_graphs(K, fan, sample):
    """V = 500 with holes, rows of degree 0 and hubs, one repeated seed; rounds 0, 1, 7; first, middle and short last batch; per-level and
    single gathers; both sampler modes."""
    V, F, B, S = 500, 6, 64, 12345
    indptr, indices, labels = random_graph(1, V, holes=True)
    feats = np.random.RandomState(1).rand(V, F).astype(np.float32)
    seeds = np.random.RandomState(10).permutation(V)[:203].astype(np.int32)
    seeds[7] = seeds[3]
    lab = labels[seeds]
    st = R.Statement(indptr, indices, feats, B, fan, S, sample)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(seeds, lab)]))
    seen = []
    for rnd in R_GRID:
        for counter in (0, 2, 3):
            eng.run_batch(0, counter, sample=sample, per_level=bool((counter + rnd) & 1), seed=S, round=rnd)
            want = st.run_batch(seeds, lab, counter, round=rnd)
            assert_batch_equal(want, eng.result(0))
            seen.append(want["ids"][:8].tolist())
    assert len(set(map(tuple, seen))) == len(seen)          # every (round, counter) is another batch
    eng.close()


def test_seed_zero_is_a_seed_and_the_mode_off_is_untouched(K, oracle, small_ds):
    """Seed 0 under the mode gives another batch than the mode off; between seeded batches (both sampler modes) an unseeded run_batch gives
    the oracle's batch bit for bit."""
    ds = small_ds
    B, fan = 300, [10, 5, 3]
    lab = ds.labels[ds.train]
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    eng = make_engine(K, ds, B, fan)
    seed = C.c_uint32(1)
    for it in (0, 2):
        eng.run_batch(0, it, seed=0, round=0)
        assert K.lib().GPUMemoryPool_GetSampleSeed(eng.pools[0], C.byref(seed)) == 1 and seed.value == 0
        got0 = eng.result(0)
        assert_batch_equal(R.Statement(ds.indptr, ds.indices, ds.features, B, fan, 0).run_batch(ds.train, lab, it), got0)
        eng.run_batch(0, it)
        assert K.lib().GPUMemoryPool_GetSampleSeed(eng.pools[0], None) == 0
        ref = orc.run_batch(ds.train, lab, it)
        assert_batch_equal(ref, eng.result(0))
        assert not np.array_equal(ref["ids"][:B], got0["ids"][:B]) and not np.array_equal(ref["nc"], got0["nc"])
        eng.run_batch(0, it, sample="distinct", seed=0xFFFFFFFF, round=2)
        assert_batch_equal(R.Statement(ds.indptr, ds.indices, ds.features, B, fan, 0xFFFFFFFF, "distinct").run_batch(ds.train, lab, it, round=2), eng.result(0))
        eng.run_batch(0, it + 1)
        assert_batch_equal(orc.run_batch(ds.train, lab, it + 1), eng.result(0))
    eng.close()


def dense_graph(seed, V, lo, hi):
    """every row has lo..hi neighbours and no holes: every slot with j < degree draws"""
    rng = np.random.RandomState(seed)
    deg = rng.randint(lo, hi + 1, size=V)
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.randint(0, V, size=int(indptr[-1])).astype(np.int32)
    return indptr, indices, rng.randint(0, 7, size=V).astype(np.int32)


@pytest.mark.parametrize("case", ["narrow-at-the-bound", "wide-just-above", "second-tile"])
def test_tile_shapes(K, case):
    """One hop's static slot bound exactly at kNarrowSlots (256-slot tiles) and one seed above it (1024-slot tiles), both sampler modes;
    and a hop of more than 4 x CU count x 1024 slots, where a workgroup runs a second tile and the stream's seed factor rides the a_step
    product (with-replacement mode; the CU count is read from the device)."""
    cus = K.lib().legion_sampler_cu_count()
    assert 32 <= cus <= 1024
    V, F, S = 2000, 4, 12345
    if case == "second-tile":
        fan = [25, 20]
        B = (4 * cus * 1024) // (fan[0] * fan[1]) + 100
        indptr, indices, labels = dense_graph(3, V, 25, 60)
        modes = ("replace",)
    else:
        fan, B = [32], 8192 + (case == "wide-just-above")
        indptr, indices, labels = random_graph(2, V, max_deg=70, holes=True)
        modes = ("replace", "distinct")
        assert (B * fan[0] <= NARROW_SLOTS) == (case == "narrow-at-the-bound")
    feats = np.random.RandomState(1).rand(V, F).astype(np.float32)
    seeds = np.random.RandomState(2).randint(0, V, size=B + B // 3).astype(np.int32)
    lab = labels[seeds]
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(seeds, lab)]))
    for sample in modes:
        st = R.Statement(indptr, indices, feats, B, fan, S, sample)
        for counter, rnd in ((0, 1), (1, 1)):
            want = st.run_batch(seeds, lab, counter, round=rnd)
            if case == "second-tile" and counter == 0:
                assert len(want["draws"][1]) > 4 * cus * 1024 and int(want["ec"][2 + 2] - want["ec"][2 + 1]) > 4 * cus * 1024
            eng.run_batch(0, counter, sample=sample, seed=S, round=rnd)
            assert_batch_equal(want, eng.result(0))
    eng.close()


def test_presampling_counts_and_partitioned_fragments(K, oracle, small_ds):
    """G = 2 clique.  Pre-sampling batches under a seed: edge_access_time equals the statement's draw counts.  Then a cache with CSR
    fragments and feature shards: the partitioned sampler and the cached gather give the uncached statement's batch."""
    ds = small_ds
    V, F = ds.spec.V, ds.spec.F
    L = K.lib()
    B, fan, G, S = 300, [10, 5], 2, 777
    parts = oracle.split_seeds(ds.train, G)
    eng = make_engine(K, ds, B, fan, G=G, cache_memory=int(V * F * 4 * 0.15), train_step=2)
    st = R.Statement(ds.indptr, ds.indices, ds.features, B, fan, S)
    for g in range(G):
        acc = np.zeros(V, np.uint64)
        for it in range(2):
            eng.run_batch(g, it, is_presc=True, seed=S, round=0)
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
        for it, rnd, sample in ((0, 0, "replace"), (1, 1, "replace"), (3, 1, "distinct")):
            eng.run_batch(g, it, sample=sample, per_level=(it != 1), seed=S, round=rnd)
            want = R.Statement(ds.indptr, ds.indices, ds.features, B, fan, S, sample).run_batch(parts[g], ds.labels[parts[g]], it, round=rnd)
            assert_batch_equal(want, eng.result(g))
    eng.close()


def test_batch_graph_replay_and_round_change(K, small_ds):
    """A seeded batch recorded as one hipGraph per pipe: replayed over iters 0..3 it gives the host-driven batches; a round change between
    replays needs no new recording (only k_set_cursor runs); so does another seed."""
    ds = small_ds
    B, fan, S = 200, [10, 5, 3], 4242
    L = K.lib()
    lab = ds.labels[ds.train]
    eng = make_engine(K, ds, B, fan, pipeline_depth=2)
    L.GPUCache_SetPreSc(eng.cache, 0)
    for sample in ("replace", "distinct"):
        st = R.Statement(ds.indptr, ds.indices, ds.features, B, fan, S, sample)
        graphs = [eng.capture_batch(0, pipe=q, sample=sample, per_level=(q == 0), seed=S, round=0) for q in (0, 1)]
        for it in range(4):
            q = it % 2
            eng.run_graph(graphs[q], it)
            got = eng.result(0, pipe=q)
            assert_batch_equal(st.run_batch(ds.train, lab, it), got)
            eng.run_batch(0, it, pipe=q, sample=sample, seed=S, round=0)      # host-driven
            assert_batch_equal(got, eng.result(0, pipe=q))
        for n, (it, rnd) in enumerate(((0, 1), (1, 1), (2, 1), (2, 7), (0, 0))):
            q = n % 2
            eng.run_graph(graphs[q], it, round=rnd)
            assert_batch_equal(st.run_batch(ds.train, lab, it, round=rnd), eng.result(0, pipe=q))
        eng.run_graph(graphs[0], 1, seed=S + 1, round=2)
        assert_batch_equal(R.Statement(ds.indptr, ds.indices, ds.features, B, fan, S + 1, sample).run_batch(ds.train, lab, 1, round=2), eng.result(0, pipe=0))
    eng.close()


def test_refusals(K, oracle, small_ds):
    """A graph recorded unseeded is refused under a seed and the other way round; SetSampleSeed and BeginRound inside a capture, and a
    training batch under a seed without BeginRound, are refused -- all by name; the engine stays usable."""
    ds = small_ds
    L = K.lib()
    B, fan, S = 100, [5, 3], 9
    lab = ds.labels[ds.train]
    eng = make_engine(K, ds, B, fan)
    pool = eng.pools[0]
    L.GPUCache_SetPreSc(eng.cache, 0)

    def refused(words, fn):
        L.legion_clear_error()
        fn()
        msg = (L.legion_last_error() or b"").decode()
        assert all(w in msg for w in words), (words, msg)
        L.legion_clear_error()

    plain = eng.capture_batch(0)
    seeded = eng.capture_batch(0, seed=S, round=1)
    eng.run_graph(seeded, 2)
    assert_batch_equal(R.Statement(ds.indptr, ds.indices, ds.features, B, fan, S).run_batch(ds.train, lab, 2, round=1), eng.result(0))
    with pytest.raises(RuntimeError, match="LegionBatchGraph_Launch: the graph was recorded unseeded and the pool is seeded now"):
        eng.run_graph(plain, 0)
    with pytest.raises(RuntimeError, match="LegionBatchGraph_Launch: the graph was recorded under a seed"):
        eng.run_graph(seeded, 0, seed=None)
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    eng.run_graph(plain, 1)
    assert_batch_equal(orc.run_batch(ds.train, lab, 1), eng.result(0))
    # inside a capture
    eng.run_batch(0, 0)                                 # unseeded, round 0: the state the recording below runs in
    st = L.d_stream_create()
    assert L.GPUMemoryPool_BeginBatchCapture(pool, st) == 0
    refused(("GPUMemoryPool_SetSampleSeed: the pool is being captured",), lambda: L.GPUMemoryPool_SetSampleSeed(pool, 1, 5))
    refused(("GPUMemoryPool_BeginRound: the pool is being captured",), lambda: L.GPUMemoryPool_BeginRound(st, pool, eng.noder, 0, 1))
    eng.run_batch(0, 0, stream=st, sync=False)
    g = L.GPUMemoryPool_EndBatchCapture(pool, st)
    K.check()
    assert g and L.GPUMemoryPool_GetSampleSeed(pool, None) == 0
    eng._graphs.append(g)
    # a training batch under a seed without its round's shuffled list; validation batches need none
    L.GPUMemoryPool_SetSampleSeed(pool, 1, 5)
    eng._seed_state.pop(0, None)
    refused(("batch_generator_kernel", "GPUMemoryPool_BeginRound"), lambda: L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE))
    assert L.GPUMemoryPool_BeginRound(None, pool, eng.noder, 0, 0) == 0
    L.GPUMemoryPool_SetSampleSeed(pool, 1, 6)          # another seed: the copy holds seed 5's permutation
    refused(("batch_generator_kernel", "GPUMemoryPool_BeginRound"), lambda: L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE))
    L.d_stream_sync(None)
    eng.run_batch(0, 1, seed=6, round=0)
    assert_batch_equal(R.Statement(ds.indptr, ds.indices, ds.features, B, fan, 6).run_batch(ds.train, lab, 1), eng.result(0))
    eng.run_batch(0, 1)
    assert_batch_equal(orc.run_batch(ds.train, lab, 1), eng.result(0))
    eng.close()
    L.d_stream_destroy(st)


@pytest.mark.parametrize("sample", ["replace", "distinct"])
def test_aggregated_hand_offs_on_top(K, small_ds, sample):
    """Neighbour sums and normalised sums of a seeded batch: bit for bit aggref / gcnref fed with the statement's batch."""
    ds = small_ds
    B, fan, S = 300, [10, 5], 31337
    lab = ds.labels[ds.train]
    st = R.Statement(ds.indptr, ds.indices, ds.features, B, fan, S, sample)
    eng = make_engine(K, ds, B, fan)
    for it, rnd in ((0, 0), (3, 2)):
        want = st.run_batch(ds.train, lab, it, round=rnd)
        eng.run_batch(0, it, sample=sample, agg_last_hop=True, per_level=(it == 0), seed=S, round=rnd)
        got = eng.result(0)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        n_in, N, run_dst, Ssum = expected_nbr_sum(want, ds.indptr, ds.indices, fan)
        assert N > 0 and got["features"].shape[0] == n_in
        assert_bits("features", got["features"], want["features"][:n_in])
        assert_bits("nbr_sum", got["nbr_sum"], Ssum)
        eng.run_batch(0, it, sample=sample, agg_last_hop=True, agg_norm="both", per_level=(it != 0), seed=S, round=rnd)
        got = eng.result(0)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        n_in, N, run_dst, Sw, d = expected_nbr_sum_norm(want, ds.indptr, ds.indices, fan)
        assert np.array_equal(got["out_deg"], d)
        assert_bits("nbr_sum (normalised)", got["nbr_sum"], Sw)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# served: the `legion` binary with LEGION_SAMPLING_SEED
# ---------------------------------------------------------------------------------------------------
def published_rows(st, sets, bs, steps, num_ids_bound):
    """feature_rows as Runner_InitializeFeaturesBuffer sizes them: 1.2 x the largest batch of the pre-sampling epoch (round 0's training
    batches), scaled by the seed ratio when the evaluation batch is the larger one, clamped to the static bound."""
    ids = sets[0]
    lab = np.zeros(len(ids), np.int32)
    largest = max(int(st.run_batch(ids, lab, c, mode=0, batch_size=bs[0], round=0)["nc"][5 + 2 * len(st.fan)]) for c in range(steps[0]))
    rows = int(largest * 1.2)
    ev = max(bs[1], bs[2])
    if ev > st.B:
        rows = int(rows * ev / st.B)
    return min(rows, num_ids_bound)


@pytest.mark.parametrize("graph,G,sample", [("0", 1, "replace"), ("1", 1, "replace"), ("1", 1, "distinct"), ("0", 2, "replace")])
def test_server_binary_serves_seeded_batches(tmp_path, synth, oracle, graph, G, sample):
    """LEGION_SAMPLING_SEED=12345, two epochs plus validation and test: every record equals the statement's batch of (mode, local,
    round = b // (train + valid steps)); epoch 0 and epoch 1 differ; the full training batches of an epoch are disjoint; the statement
    itself shows that no batch outgrows the feature rows the server publishes."""
    import oracle as O
    workload, scale, B, epochs, fan, S = "products", 0.004, 96, 2, [10, 5], 12345     # 786 training seeds: 8 steps on one GPU, 4 each on two
    spec = synth.spec_for(workload, scale=scale)
    ds = synth.generate(spec)
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    meta_line = "synth:%s:%r %d %d %d %d %d %d %d %d %d 0" % (workload, scale, B, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, 1 << 40, epochs)
    env = dict(LEGION_SAMPLING_SEED=S, LEGION_BATCH_GRAPH=graph, LEGION_SAMPLING=sample)
    with served(tmp_path, meta_line, fan, G=G, env=env) as srv:
        gots = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    text = srv.log_text()
    assert text.count("Sampling seed: 12345 (LEGION_SAMPLING_SEED)") == G and "Feature buffer too small" not in text
    sets, steps, bs = serve_sets(oracle, ds, B, G, n_valid=n_valid, n_test=n_test)
    H = len(fan)
    assert steps[0] >= 3 and steps[1] > 0 and steps[2] > 0
    for g, got in enumerate(gots):
        assert got["sampling_seed"] == S and got["sampling"] == sample and got["hops"] == H
        st = R.Statement(ds.indptr, ds.indices, ds.features, B, fan, S, sample)
        pool_b = max(B, bs[g][1], bs[g][2])
        rows = published_rows(st, sets[g], bs[g], steps, pool_b * (1 + fan[0] + fan[0] * fan[1]))
        assert len(got["batches"]) == O.max_step(steps, epochs)
        train = {}
        for rec in got["batches"]:
            mode, local = O.schedule(steps, epochs, rec["b"])
            rnd = rec["b"] // (steps[0] + steps[1])
            ids = sets[g][mode]
            ref = st.run_batch(ids, ds.labels[ids], local, mode=mode, batch_size=bs[g][mode], round=rnd)
            assert int(ref["nc"][5 + 2 * H]) <= rows, (rec["b"], int(ref["nc"][5 + 2 * H]), rows)      # the shape condition, from the statement alone
            assert_served_record(rec, ref, H)
            if mode == 0:
                train[(rnd, local)] = rec
            elif mode == 2:
                assert rnd >= epochs
        for local in range(steps[0]):
            assert train[(0, local)]["seeds"] != train[(1, local)]["seeds"] and train[(0, local)]["ids"] != train[(1, local)]["ids"]
        for rnd in range(epochs):
            full = [train[(rnd, c)]["seeds"] for c in range(steps[0]) if len(train[(rnd, c)]["seeds"]) == bs[g][0]]
            flat = np.concatenate(full)
            assert len(full) >= 2 and len(np.unique(flat)) == len(flat) and np.isin(flat, sets[g][0]).all()


def test_unseeded_server_says_none(tmp_path, synth, oracle):
    """Without the variable: sampling_seed() is None, nothing is logged about a seed, and the batches are the oracle's."""
    workload, scale, B, epochs, fan = "products", 0.004, 512, 1, [10, 5]
    spec = synth.spec_for(workload, scale=scale)
    ds = synth.generate(spec)
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    meta_line = "synth:%s:%r %d %d %d %d %d %d %d %d %d 0" % (workload, scale, B, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, 1 << 40, epochs)
    with served(tmp_path, meta_line, fan, env=dict(LEGION_SAMPLING_SEED=None)) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    assert got["sampling_seed"] is None and "Sampling seed" not in srv.log_text()
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B, n_valid=n_valid, n_test=n_test)
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, spec.V, spec.F, B, fan)
    for rec, ref, mode, local in replay_served(got, orc, sets, ds.labels, steps, epochs, bs):
        assert_served_record(rec, ref, len(fan))


def test_link_prediction_lists_stay_in_file_order(tmp_path, synth, oracle):
    """Meta flag 2: the [src | pos | neg] lists are served verbatim -- the runner says so once -- and their draws are seeded."""
    import oracle as O
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    B, fan, epochs, S = 510, [10, 5], 2, 12345
    meta_line = "synth:products:0.004 %d %d %d %d %d 100 60 0 %d 2" % (B, spec.V, ds.E, spec.F, spec.n_train, epochs)
    with served(tmp_path, meta_line, fan, env=dict(LEGION_SAMPLING_SEED=hex(S))) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    text = srv.log_text()
    assert text.count("the training lists are served verbatim (meta flag 2): not shuffled") == 1 and got["sampling_seed"] == S
    lists = [synth.lp_trainingset(ds, len(ds.train), B, rank=0, world=1)]
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B, 1, train=lists, n_valid=100, n_test=60)
    st = R.Statement(ds.indptr, ds.indices, ds.features, B, fan, S, shuffle=False)
    plain = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, spec.V, spec.F, B, fan)
    for rec in got["batches"]:
        mode, local = O.schedule(steps, epochs, rec["b"])
        ids = sets[mode]
        ref = st.run_batch(ids, ds.labels[ids], local, mode=mode, batch_size=bs[mode], round=rec["b"] // (steps[0] + steps[1]))
        assert_served_record(rec, ref, len(fan))
        if mode == 0:
            assert rec["seeds"] == plain.run_batch(ids, ds.labels[ids], local, mode=mode, batch_size=bs[mode])["ids"][:len(rec["seeds"])].tolist()
