"""Aggregated last hop on the GPU (get_feature_kernel_agg / k_gather_sum), through the C ABI, against the CPU oracle's DEFAULT-mode
batch and the NumPy statement of tests/aggref.py: nc, ec, ids, labels and both COO arrays word for word, feature rows
[0, n_in) bit-equal, the neighbour sums bit-equal (array_equal on the uint32 view).  Run with `pytest -m gpu`.

The served path: the `legion` binary with LEGION_AGG_LAST_HOP=1 and a fresh trainer process on ipc_service.get_next_aggregated."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from aggref import expected_nbr_sum, last_hop_runs
from conftest import KEYS_NO_FEATURES, ROOT, assert_batch_equal, sha
from harness import K, OUT, Children, attached_client, child_env, in_process_runner, make_engine, replay_served, serve_sets, served, wait_for_text  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu


def assert_agg_batch(ref, got, indptr, indices, fan, x=None):
    """`got` (aggregated mode) against the default-mode reference batch `ref`.  Returns (n_in, N, cnt)."""
    assert_batch_equal(ref, got, keys=KEYS_NO_FEATURES)
    n_in, N, run_dst, S = expected_nbr_sum(ref, indptr, indices, fan, x=x)
    feats = np.asarray(ref["features"] if x is None else x, dtype=np.float32)
    assert got["features"].shape == (n_in, feats.shape[1]) and got["nbr_sum"].shape == S.shape, (got["features"].shape, got["nbr_sum"].shape, S.shape)
    assert np.array_equal(got["features"].view(np.uint32), feats[:n_in].view(np.uint32))
    a, b = got["nbr_sum"].view(np.uint32), S.view(np.uint32)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError("nbr_sum: %d words differ, first at %s: %r vs %r" % (len(bad), bad[:3].tolist(), got["nbr_sum"][tuple(bad[0])], S[tuple(bad[0])]))
    return n_in, N, last_hop_runs(ref, indptr, indices, fan)[3]


@pytest.mark.parametrize("F", [128, 100, 36, 7])
@pytest.mark.parametrize("fan", [[10], [10, 5], [10, 5, 3]])
def test_parity_hops_and_feature_widths(K, oracle, synth, fan, F):
    """H = 1, 2, 3; F = 128 (float4, whole lines), 100 (float4, pitched replica: 128 floats per row), 36 (float4, 9 lanes per row,
    pitched), 7 (scalar path, pitched); first batch, a middle one and the short last batch; the levels < H gathered per level behind
    their hops (first batch) or inside the aggregated call (the others)."""
    L = K.lib()
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    V = spec.V
    feats = np.random.RandomState(F).standard_normal((V, F)).astype(np.float32)
    pitch = L.legion_row_pitch(F)
    table = np.full((V, pitch), np.float32(-777.0))      # poison in the pad floats: must never reach a sum
    table[:, :F] = feats
    B = 300
    train = ds.train[:2 * B + 41]
    lab = ds.labels[train]
    orc = oracle.OracleRunner(ds.indptr, ds.indices, feats, V, F, B, fan)
    eng = K.Engine(ds.indptr, ds.indices, table.reshape(-1), V, F, dict(train=[(train, lab)]), B, fan, features_pitch=pitch if pitch > F else 0)
    eng.alloc_features()
    for it in (0, 1, 2):
        ref = orc.run_batch(train, lab, it)
        eng.run_batch(0, it, agg_last_hop=True, per_level=(it == 0))
        n_in, N, cnt = assert_agg_batch(ref, eng.result(0), ds.indptr, ds.indices, fan)
        assert N > 0 and n_in > 0
    assert int(ref["nc"][4]) == 41                        # the last one was the short batch
    # and the default mode on the same engine afterwards: untouched
    eng.run_batch(0, 1)
    assert_batch_equal(orc.run_batch(train, lab, 1), eng.result(0))
    eng.close()


def holes_graph(seed, V=500):
    """degree-0 rows, -1 neighbour entries, degree < fan-out, a few hubs (the shape of test_random_graphs_with_holes)"""
    rng = np.random.RandomState(seed)
    deg = rng.randint(0, 12, size=V)
    deg[rng.randint(0, V, 5)] = 300
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.randint(-1, V, size=int(indptr[-1])).astype(np.int32)
    labels = rng.randint(0, 9, size=V).astype(np.int32)
    seeds = rng.permutation(V)[:203].astype(np.int32)
    return indptr, indices, labels, seeds


@pytest.mark.parametrize("seed", [0, 1])
def test_graphs_with_holes_and_short_rows(K, oracle, seed):
    V, F = 500, 7 + seed                                  # 7: scalar path, 8: float4 path
    indptr, indices, labels, seeds = holes_graph(seed, V)
    feats = np.random.RandomState(100 + seed).rand(V, F).astype(np.float32)
    feats[::17] = np.float32(-0.0)                        # 0.0f + (-0.0f) = +0.0f: the sum starts from +0.0
    empty_runs = 0
    for fan, B in (([3, 2], 50), ([5, 4, 3], 64), ([25, 10], 203), ([1, 1, 1, 1], 7), ([2], 1), ([6], 64), ([2, 2, 2, 2, 2], 7)):
        orc = oracle.OracleRunner(indptr, indices, feats, V, F, B, fan)
        eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(seeds, labels[seeds])]))
        for counter in range(min(4, (len(seeds) + B - 1) // B)):
            ref = orc.run_batch(seeds, labels[seeds], counter)
            eng.run_batch(0, counter, agg_last_hop=True, per_level=bool(counter & 1))
            n_in, N, cnt = assert_agg_batch(ref, eng.result(0), indptr, indices, fan)
            empty_runs += int((cnt == 0).sum())
        eng.close()
    assert empty_runs > 0                                 # degree-0 inputs / all-hole draws: stored rows of +0.0 were compared


def test_stale_rows_and_the_end_of_the_buffer(K, oracle):
    """A large batch, then a short one on the same pipe: rows of runs without draws are +0.0 (stored, not left over from the large
    batch), and rows [n_in + N, ...) are never written."""
    V, F = 500, 8
    indptr, indices, labels, seeds = holes_graph(5, V)
    feats = (np.random.RandomState(9).rand(V, F) + 1.0).astype(np.float32)      # no zero in the table: a zero row is a stored one
    B, fan = 100, [5, 3]
    seeds = seeds[:2 * B + 9]
    orc = oracle.OracleRunner(indptr, indices, feats, V, F, B, fan)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(seeds, labels[seeds])]))
    L = K.lib()
    feat = eng.out[0][0]["feat"]
    eng.run_batch(0, 0, agg_last_hop=True)
    big = eng.result(0)
    poison = np.float32(np.frombuffer(b"\xa5\xa5\xa5\xa5", np.float32)[0])
    for it in (0, 2):                                     # the full batch again over a poisoned buffer, then the short last one
        L.d_memset_async(feat.ptr, 0xA5, feat.nbytes, None)
        L.d_stream_sync(None)
        ref = orc.run_batch(seeds, labels[seeds], it)
        eng.run_batch(0, it, agg_last_hop=True)
        got = eng.result(0)
        n_in, N, cnt = assert_agg_batch(ref, got, indptr, indices, fan)
        assert (cnt == 0).any() and not got["nbr_sum"][cnt == 0].view(np.uint32).any()
        rest = feat.to_numpy(np.float32, (eng.feature_rows - n_in - N) * F, offset_bytes=(n_in + N) * F * 4)
        assert (rest.view(np.uint32) == poison.view(np.uint32)).all()
    assert n_in + N < big["features"].shape[0] + big["nbr_sum"].shape[0]
    eng.close()


def test_feature_sources_host_table_cache_and_clique(K, oracle, small_ds, monkeypatch):
    """The sums read the source k_gather would read: a pinned-host table, a Kg = 1 cache built from a pre-sampling epoch, a
    G = 2 logical clique with in-kernel peer reads; LEGION_PEER_GATHER=exchange + the mode is refused, naming both."""
    ds = small_ds
    V, F = ds.spec.V, ds.spec.F
    L = K.lib()
    B, fan = 300, [10, 5]
    # pinned host tables
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, V, F, B, fan)
    eng = make_engine(K, ds, B, fan, csr_location=K.LOC_HOST_PINNED, features_location=K.LOC_HOST_PINNED)
    for it in (0, 3):
        eng.run_batch(0, it, agg_last_hop=True, per_level=(it == 0))
        assert_agg_batch(orc.run_batch(ds.train, ds.labels[ds.train], it), eng.result(0), ds.indptr, ds.indices, fan)
    eng.close()
    # caches: G logical GPUs on one device, Kg = G
    for G, mode in ((1, 0), (2, 1)):
        parts = oracle.split_seeds(ds.train, G)
        eng = make_engine(K, ds, B, fan, G=G, cache_memory=int(V * F * 4 * 0.15), train_step=2)
        for g in range(G):
            for it in range(2):
                eng.run_batch(g, it, is_presc=True)
        eng.build_cache(cache_agg_mode=mode, node_capacity=V // 8, edge_capacity=0, train_step=2)
        assert L.GPUCache_Kg(eng.cache) == G and L.GPUCache_NodeCapacity(eng.cache, 0) == V // 8
        for g in range(G):
            orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, V, F, B, fan, partition_count=G)
            L.SetGPUDevice(g)
            fmap = K.read_dev(L.GPUCache_GetFeatureMap(eng.cache, g), np.int32, V)
            for it in (0, 1):
                ref = orc.run_batch(parts[g], ds.labels[parts[g]], it)
                eng.run_batch(g, it, agg_last_hop=True, per_level=(it == 0))
                assert_agg_batch(ref, eng.result(g), ds.indptr, ds.indices, fan)
                slot = fmap[ref["ids"][int(ref["nc"][3 + 2 * len(fan)]):]]         # the last hop's new nodes: hits and misses were summed
                assert (slot >= 0).any() and (slot < 0).any()
                if G == 2:
                    assert ((slot >= 0) & (slot // (V // 8) != g)).any()          # ... and rows of the peer's shard
        if G == 2:
            monkeypatch.setenv("LEGION_PEER_GATHER", "exchange")
            with pytest.raises(RuntimeError) as ex:
                eng.run_batch(0, 0, agg_last_hop=True)
            assert "LEGION_PEER_GATHER=exchange" in str(ex.value) and "aggregated last hop (GPUMemoryPool_SetAggLastHop)" in str(ex.value)
            monkeypatch.delenv("LEGION_PEER_GATHER")
            eng.run_batch(0, 1, agg_last_hop=True)        # still usable
            assert_agg_batch(oracle.OracleRunner(ds.indptr, ds.indices, ds.features, V, F, B, fan, partition_count=G).run_batch(parts[0], ds.labels[parts[0]], 1),
                             eng.result(0), ds.indptr, ds.indices, fan)
        eng.close()


def test_launcher_refusals(K, oracle, small_ds):
    ds = small_ds
    B, fan = 300, [10, 5]
    L = K.lib()
    eng = make_engine(K, ds, B, fan)
    pool = eng.pools[0]

    def refused(text, fn):
        L.legion_clear_error()
        fn()
        msg = (L.legion_last_error() or b"").decode()
        assert text in msg, (text, msg)
        L.legion_clear_error()

    agg = lambda: L.get_feature_kernel_agg(None, eng.cache, eng.noder, pool, 0, 1)      # noqa: E731
    eng.run_batch(0, 0)
    refused("does not aggregate the last hop", agg)
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    assert L.GPUMemoryPool_GetAggLastHop(pool) == 1
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
    refused("before the last hop", agg)
    L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, fan[0], 2, 0)
    refused("before the last hop", agg)
    L.d_stream_sync(None)
    for q in range(eng.depth):
        L.GPUMemoryPool_SetFloatFeatures(pool, None, q)
    eng.run_batch(0, 0, gather=False)
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    refused("feature buffer of the current pipe is not set", agg)
    for q in range(eng.depth):
        L.GPUMemoryPool_SetFloatFeatures(pool, eng.out[0][q]["feat"].ptr, q)
    # and the engine still produces the expected batch in both modes
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    ref = orc.run_batch(ds.train, ds.labels[ds.train], 2)
    eng.run_batch(0, 2, agg_last_hop=True)
    assert_agg_batch(ref, eng.result(0), ds.indptr, ds.indices, fan)
    eng.run_batch(0, 2)
    assert_batch_equal(ref, eng.result(0))
    eng.close()


@pytest.mark.parametrize("graph", [False, True])
def test_overlapped_two_stream_schedule_aggregated(K, oracle, small_ds, graph):
    """Depth 2: batch i + 1 is sampled on one stream while batch i is summed on the other (the schedule of
    test_overlapped_two_stream_schedule), 10 consecutive batches, each equal to its serial result.  Hop 1 of batch i + 1 overwrites
    the pool's one draw buffer while k_gather_sum of batch i may still run: this is the test that fails if the last hop's draws are
    not kept per pipe.  graph=True: the sampler side replayed as a recorded hipGraph per pipe, the sums by a plain launch behind it."""
    ds = small_ds
    B, fan = 200, [10, 5, 3]
    H = len(fan)
    n = 10
    assert (n - 1) * B < len(ds.train) <= n * B         # ten batches, the last one short
    L = K.lib()
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    eng = make_engine(K, ds, B, fan, pipeline_depth=2)
    L.GPUCache_SetPreSc(eng.cache, 0)
    pool = eng.pools[0]
    s_samp, s_gath = L.d_stream_create(), L.d_stream_create()
    ev_sampled = [L.d_event_create(), L.d_event_create()]
    ev_gathered = [L.d_event_create(), L.d_event_create()]
    used = [False, False]
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    graphs = [eng.capture_batch(0, gather=False, pipe=q, stream=s_samp, agg_last_hop=True) for q in (0, 1)] if graph else None   # the sampler side only
    assert L.GPUMemoryPool_GetAggLastHop(pool) == 1

    def enqueue(i):
        q = i % 2
        L.GPUMemoryPool_SetCurrentPipe(pool, q)
        L.GPUMemoryPool_SetCurrentMode(pool, K.TRAINMODE)
        if used[q]:
            L.d_stream_wait_event(s_samp, ev_gathered[q])
        if graph:
            eng.run_graph(graphs[q], i, sync=False)
        else:
            L.batch_generator_kernel(s_samp, eng.noder, eng.cache, pool, B, i, 0, 0, K.TRAINMODE)
            for h in range(H):
                L.GPU_Random_Sampling(s_samp, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
        L.d_event_record(ev_sampled[q], s_samp)
        L.d_stream_wait_event(s_gath, ev_sampled[q])
        L.get_feature_kernel_agg(s_gath, eng.cache, eng.noder, pool, 0, 1)
        L.d_event_record(ev_gathered[q], s_gath)
        used[q] = True

    enqueue(0)
    for i in range(n):
        if i + 1 < n:
            enqueue(i + 1)          # batch i + 1 is sampled while batch i is still being summed
        L.d_stream_sync(s_samp)
        L.d_stream_sync(s_gath)
        K.check()
        assert_agg_batch(orc.run_batch(ds.train, ds.labels[ds.train], i), eng.result(0, pipe=i % 2, aggregated=True), ds.indptr, ds.indices, fan)
    eng.close()
    for s in (s_samp, s_gath):
        L.d_stream_destroy(s)


def test_whole_batch_as_one_graph(K, oracle, small_ds):
    """The aggregated batch recorded as ONE hipGraph per pipe (sampler, per-level gathers of the levels < H, sums) and replayed."""
    ds = small_ds
    B, fan = 200, [10, 5]
    L = K.lib()
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    eng = make_engine(K, ds, B, fan, pipeline_depth=2)
    L.GPUCache_SetPreSc(eng.cache, 0)
    graphs = [eng.capture_batch(0, pipe=q, agg_last_hop=True, per_level=(q == 0)) for q in (0, 1)]
    last = (len(ds.train) - 1) // B
    for n, it in enumerate((0, 1, 2, 5, last, 0)):
        q = n % 2
        eng.run_graph(graphs[q], it)
        assert_agg_batch(orc.run_batch(ds.train, ds.labels[ds.train], it), eng.result(0, pipe=q), ds.indptr, ds.indices, fan)
    eng.close()


def test_full_papers100m_shape(K, oracle, synth):
    """One BASELINE shape at size (papers100M, {25, 10, 5}, 8000 seeds, three batches): the rows * F and buffer arithmetic where
    n_in + N is in the millions.  Sampling against the (OpenMP) oracle on a host copy of the CSR; the expected sums from the oracle's
    batch and the generator's feature rows."""
    import torch
    sys_bench = __import__("bench")
    L = K.lib()
    fan = [25, 10, 5]
    spec = synth.spec_for("papers100M")
    dev = torch.device("cuda", 0)
    indptr, indices, feats, E = sys_bench.build_graph_on_gpu(K, spec, dev, pitch=0)
    B = 8000
    tr = torch.empty(spec.n_train, dtype=torch.int32, device=dev)
    L.legion_synth_seed_ids(None, tr.data_ptr(), 0, spec.n_train, spec.V, spec.M2, spec.C2, 1, 0)
    lab = torch.empty(spec.V, dtype=torch.int32, device=dev)
    L.legion_synth_labels(None, lab.data_ptr(), 0, spec.V, spec.classes)
    torch.cuda.synchronize()
    my_lab = lab[tr.long()].contiguous()
    seeds = dict(train=[((tr.data_ptr(), spec.n_train), (my_lab.data_ptr(), spec.n_train))])
    eng = K.Engine(indptr.data_ptr(), indices.data_ptr(), feats.data_ptr(), spec.V, spec.F, seeds, B, fan, E=E)
    eng.alloc_features()
    h_indptr, h_indices = indptr.cpu().numpy(), indices.cpu().numpy()
    orc = oracle.OracleRunner(h_indptr, h_indices, None, spec.V, spec.F, B, fan, with_features=False)
    h_tr, h_lab = tr.cpu().numpy(), my_lab.cpu().numpy()
    for it in (0, 1, 7):
        ref = orc.run_batch(h_tr, h_lab, it, gather=False, omp=True)
        x = np.concatenate([synth.features(spec, ref["ids"][i:i + 200000]) for i in range(0, len(ref["ids"]), 200000)])
        eng.run_batch(0, it, agg_last_hop=True, per_level=(it != 1))
        n_in, N, cnt = assert_agg_batch(ref, eng.result(0), h_indptr, h_indices, fan, x=x)
        assert N > 500000 and n_in > 100000
    eng.close()


def test_sums_behind_a_replayed_sampler_graph_do_not_inherit_the_previous_batch(K, oracle, small_ds):
    """get_feature_kernel_agg decides from the pool's per-batch host state whether the levels < H were gathered per level.  A replayed
    sampler-only graph must bring the state of ITS recording, not leave that of the plain batch before it: plain aggregated batches with
    per-level gathers alternate with sampler-graph replays + get_feature_kernel_agg over a poisoned buffer -- rows [0, n_in) of the
    replayed batch must be gathered by that call; and a pre-sampling batch in front of a replay does not make the call refuse."""
    ds = small_ds
    B, fan = 200, [10, 5]
    L = K.lib()
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    eng = make_engine(K, ds, B, fan, cache_memory=int(ds.spec.V * ds.spec.F * 4 * 0.15))
    L.GPUCache_SetPreSc(eng.cache, 0)
    st = L.d_stream_create()
    g = eng.capture_batch(0, gather=False, stream=st, agg_last_hop=True)        # the sampler side only
    feat = eng.out[0][0]["feat"]
    for it, before in ((3, "plain"), (1, "plain"), (4, "presc")):
        if before == "plain":
            eng.run_batch(0, it + 1, agg_last_hop=True, per_level=True, stream=st)     # leaves "every level < H gathered" behind
        else:
            eng.run_batch(0, it + 1, is_presc=True, stream=st)
            L.GPUMemoryPool_SetAggLastHop(eng.pools[0], 1)
        L.d_memset_async(feat.ptr, 0xA5, feat.nbytes, st)
        eng.run_graph(g, it, sync=False)
        L.get_feature_kernel_agg(st, eng.cache, eng.noder, eng.pools[0], 0, 1)
        L.d_stream_sync(st)
        K.check()
        assert_agg_batch(orc.run_batch(ds.train, ds.labels[ds.train], it), eng.result(0, aggregated=True), ds.indptr, ds.indices, fan)
    eng.close()
    L.d_stream_destroy(st)


def test_rows_times_chunks_beyond_int32_is_refused(K):
    """(row, chunk) work items are addressed with 31 bits: a pool whose levels can hold 2^31 / C rows or more is refused by name through
    get_feature_kernel_agg (sticky error, nothing launched).  H = 1, F = 4096 (C = 1024 float4 chunks per row), 2^21 seeds: 2^31 items."""
    V, F, B = 64, 4096, 1 << 21
    indptr = np.arange(V + 1, dtype=np.int64)
    indices = np.arange(V, dtype=np.int32)[::-1].copy()
    seeds = np.zeros(B, np.int32)
    eng = K.Engine(indptr, indices, np.zeros((V, F), np.float32), V, F, dict(train=[(seeds, seeds)]), B, [1])
    eng.alloc_features(rows=16)
    with pytest.raises(RuntimeError, match=r"rows\*F exceeds 2\^31 work items"):
        eng.run_batch(0, 0, agg_last_hop=True, per_level=False)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# served: the `legion` binary -> ipc_service.get_next_aggregated
# ---------------------------------------------------------------------------------------------------
# (the cases that leave LEGION_RUNNER_GATHER at auto keep the ids they had before the parameter)
@pytest.mark.parametrize("fan,graph,gather", [
    pytest.param([10, 5], "0", "auto", id="fan0-0"), pytest.param([5, 4, 3], "0", "auto", id="fan1-0"),
    pytest.param([10, 5], "1", "auto", id="fan2-1"), pytest.param([6], "0", "auto", id="fan3-0"),
    pytest.param([10, 5], "0", "level", id="fan0-0-level"), pytest.param([10, 5], "0", "all", id="fan0-0-all")])
def test_server_binary_serves_aggregated_batches(tmp_path, synth, oracle, fan, graph, gather):
    """LEGION_AGG_LAST_HOP=1: a fresh trainer process sees aggregated() == True, get_next raises there, and every batch of the schedule
    (train + valid + test steps, two epochs) through get_next_aggregated equals the oracle's default batch + the NumPy statement.
    graph = 1: the runner's LEGION_BATCH_GRAPH=1 path (sampler graph on stream 0, the sums by a plain call on stream 1 while the next
    batch's graph overwrites the shared draw buffer).  gather = level / all: LEGION_RUNNER_GATHER pinned, so that both ways of the levels
    below the last are served -- gathered per level in front of the sums, or inside get_feature_kernel_agg -- whichever `auto` picks here."""
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    data = str(tmp_path / "ds") + "/"
    synth.write_legion_files(ds, data)
    B, epochs = 512, 2
    env = dict(LEGION_BATCH_GRAPH=graph, LEGION_AGG_LAST_HOP="1", **({} if gather == "auto" else dict(LEGION_RUNNER_GATHER=gather)))
    with served(tmp_path, synth.meta_config_line(ds, data, B, 1 << 40, epochs, 0), fan, env=env) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["agg", spec.F, epochs, OUT])
        srv.finish()
    H = len(fan)
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B)
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, spec.V, spec.F, B, fan)
    assert got["hops"] == H and steps[1] > 0 and steps[2] > 0
    for rec, ref, mode, local in replay_served(got, orc, sets, ds.labels, steps, epochs, bs):
        n_in, N, run_dst, S = expected_nbr_sum(ref, ds.indptr, ds.indices, fan)
        assert (rec["n"], rec["n_in"], rec["runs"]) == (int(ref["nc"][5 + 2 * H]), n_in, N)
        assert rec["edges"] == [int(ref["ec"][2 + (H - k + 1)]) for k in range(1, H + 1)]
        assert rec["ids"] == sha(ref["ids"]) and rec["labels"] == sha(ref["labels"]) and rec["src"] == sha(ref["src_off"]) and rec["dst"] == sha(ref["dst_off"])
        assert rec["features"] == sha(ref["features"][:n_in]) and rec["nbr_sum"] == sha(S), rec["b"]
    assert "Hand-off: the last hop as neighbour sums" in srv.log_text()


def test_plain_server_refuses_get_next_aggregated_and_a_short_buffer_is_named(K, small_ds, tmp_path, capfd, monkeypatch):
    """An in-process runner (the pattern of test_a_batch_larger_than_the_feature_buffer_...).  (a) Without LEGION_AGG_LAST_HOP a trainer's
    get_next_aggregated raises, naming the switch.  (b) With it: after one good batch the published row capacity is shrunk below n_in + N:
    the trainer refuses the batch and the server names it as rows of features + neighbour sums and counts it."""
    ds = small_ds
    B, fan = 300, [10, 5]
    for agg in (False, True):
        if agg:
            monkeypatch.setenv("LEGION_AGG_LAST_HOP", "1")
        else:
            monkeypatch.delenv("LEGION_AGG_LAST_HOP", raising=False)
        # two pre-sampling batches: the buffer is sized for max(n_in + N)
        with in_process_runner(K, ds, B, fan, "agg%d" % agg, presc_batches=2) as r, Children() as children:
            L, env, runner, rp = r.L, r.env, r.runner, r.rp
            assert L.IPCEnv_GetAggLastHop(env) == int(agg)
            cenv = child_env(r.ns)
            if not agg:
                code = ("import sys, torch; sys.path.insert(0, %r); import ipc_service; torch.cuda.set_device(0); ipc_service.initialize()\n"
                        "assert ipc_service.aggregated() is False\n"
                        "try:\n    ipc_service.get_next_aggregated(%d); sys.exit(7)\n"
                        "except RuntimeError as e:\n    sys.exit(0 if 'LEGION_AGG_LAST_HOP=1' in str(e) and 'does not aggregate' in str(e) else 5)\n"
                        % (os.path.join(ROOT, "legion-1_amd", "ipc_service"), ds.spec.F))
                res = subprocess.run([sys.executable, "-c", code], env=cenv, capture_output=True, text=True, timeout=240)
                assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
                continue
            pool = L.Runner_GetMemoryPool(runner)
            small_rows = 100
            log = str(tmp_path / "client.log")
            client = attached_client(children, "ipc_client_modes.py", ["agg", ds.spec.F, "refuse", "feature buffer holds %d rows" % small_rows], cenv, log)
            rp.global_batch_id = 0
            L.Runner_RunOnce(runner, C.byref(rp))
            rp.global_batch_id = 1
            L.Runner_RunOnce(runner, C.byref(rp))          # batch 0 handed over: complete
            K.check()
            wait_for_text(log, "BATCH", client, 240, 0.05)
            assert L.Runner_ShortBatches(runner) == 0
            L.GPUMemoryPool_SetFeatureRows(pool, small_rows)
            L.IPCEnv_SetFeatureRows(env, 0, small_rows)
            rp.global_batch_id = 2
            L.Runner_RunOnce(runner, C.byref(rp))          # hands batch 1 over: n_in + N rows no longer fit
            K.check()
            rc = client.wait(timeout=120)
            text = open(log).read()
            assert rc == 0 and "RAISED after 1 good batches" in text and "rows (features + neighbour sums)" in text, text[-3000:]
            assert L.Runner_ShortBatches(runner) == 1
    said = capfd.readouterr().out
    assert "Feature buffer too small: a batch has" in said and "rows (features + neighbour sums), the buffer holds 100 rows" in said, said[-1500:]
