"""Normalised last hop on the GPU (GPUMemoryPool_SetAggNorm: k_agg_norm_prep / k_block_out_deg / k_draw_weights in front of the weighted
k_gather_sum), through the C ABI, against the CPU oracle's DEFAULT-mode batch and the NumPy statement of tests/gcnref.py.  Every check is
array_equal: out_deg against bincount, the normalised sums bit for bit (uint32 view), feature rows [0, n_in) and nc, ec, ids, labels
and both COO arrays word for word.  Run with `pytest -m gpu`.

The served path: the `legion` binary with LEGION_AGG_LAST_HOP=1 LEGION_AGG_NORM=both and a fresh trainer process on
ipc_service.get_next_aggregated_norm."""
import os
import subprocess
import sys

import numpy as np
import pytest

from aggref import expected_nbr_sum
from conftest import KEYS_NO_FEATURES, ROOT, assert_batch_equal, sha
from gcnref import expected_nbr_sum_norm
from harness import K, OUT, SERVER, child_env, ipc_namespace, make_engine, replay_served, serve_sets, served  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu


def assert_bits(name, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d words differ, first at %s: %r vs %r" % (name, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def assert_norm_batch(ref, got, indptr, indices, fan, x=None):
    """`got` (normalised mode) against the default-mode reference batch `ref`.  Returns (n_in, N, d)."""
    assert_batch_equal(ref, got, keys=KEYS_NO_FEATURES)
    n_in, N, run_dst, S, d = expected_nbr_sum_norm(ref, indptr, indices, fan, x=x)
    feats = np.asarray(ref["features"] if x is None else x, dtype=np.float32)
    assert got["out_deg"].dtype == np.int32 and np.array_equal(got["out_deg"], d), "out_deg"
    assert got["features"].shape == (n_in, feats.shape[1])
    assert_bits("features", got["features"], feats[:n_in])
    assert_bits("nbr_sum", got["nbr_sum"], S)
    return n_in, N, d


def assert_plain_agg_batch(ref, got, indptr, indices, fan):
    """the plain aggregated mode (tests/aggref.py), for the batches around a normalised one"""
    assert_batch_equal(ref, got, keys=KEYS_NO_FEATURES)
    n_in, N, run_dst, S = expected_nbr_sum(ref, indptr, indices, fan)
    assert "out_deg" not in got
    assert_bits("features", got["features"], np.asarray(ref["features"])[:n_in])
    assert_bits("nbr_sum", got["nbr_sum"], S)


@pytest.mark.parametrize("F", [128, 100, 36, 7])
@pytest.mark.parametrize("fan", [[10], [10, 5], [10, 5, 3]])
def test_parity_hops_and_feature_widths(K, oracle, synth, fan, F):
    """H = 1, 2, 3; F = 128 (float4, whole lines), 100 and 36 (float4, pitched replica), 7 (scalar path, pitched); first batch, a middle one
    and the short last batch; the levels < H gathered per level (first batch) or inside the aggregated call.  On the same engine the plain
    aggregated mode before and after a normalised batch still gives aggref's sums bit for bit, and the default mode its rows."""
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
    eng.run_batch(0, 1, agg_last_hop=True)
    assert_plain_agg_batch(orc.run_batch(train, lab, 1), eng.result(0), ds.indptr, ds.indices, fan)
    weighted = 0
    for it in (0, 1, 2):
        ref = orc.run_batch(train, lab, it)
        eng.run_batch(0, it, agg_last_hop=True, agg_norm="both", per_level=(it == 0))
        assert L.GPUMemoryPool_GetAggNorm(eng.pools[0]) == 1
        n_in, N, d = assert_norm_batch(ref, eng.result(0), ds.indptr, ds.indices, fan)
        assert N > 0 and n_in > 0
        weighted += int((d > 1).sum())
    assert int(ref["nc"][4]) == 41 and weighted > 0       # the last one was the short batch; some weights were not 1
    eng.run_batch(0, 1, agg_last_hop=True)                # the plain sums again, then the default mode: untouched
    assert L.GPUMemoryPool_GetAggNorm(eng.pools[0]) == 0
    assert_plain_agg_batch(orc.run_batch(train, lab, 1), eng.result(0), ds.indptr, ds.indices, fan)
    eng.run_batch(0, 1)
    assert_batch_equal(orc.run_batch(train, lab, 1), eng.result(0))
    eng.close()


def holes_graph(seed, V=500):
    """degree-0 rows, -1 neighbour entries, degree < fan-out, a few hubs (the shape of test_gpu_agg_last_hop.py's)"""
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
    """Slots without a draw inside and at the end of a run: the slot -> edge prefix counts exactly the slots k_write turned into edges."""
    V, F = 500, 7 + seed                                  # 7: scalar path, 8: float4 path
    indptr, indices, labels, seeds = holes_graph(seed, V)
    feats = np.random.RandomState(100 + seed).rand(V, F).astype(np.float32)
    feats[::17] = np.float32(-0.0)                        # 0.0f + w * (-0.0f) = +0.0f: the sum starts from +0.0
    hubs = 0
    for fan, B in (([3, 2], 50), ([5, 4, 3], 64), ([25, 10], 203), ([1, 1, 1, 1], 7), ([2], 1), ([6], 64)):
        orc = oracle.OracleRunner(indptr, indices, feats, V, F, B, fan)
        eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(seeds, labels[seeds])]))
        for counter in range(min(4, (len(seeds) + B - 1) // B)):
            ref = orc.run_batch(seeds, labels[seeds], counter)
            eng.run_batch(0, counter, agg_last_hop=True, agg_norm="both", per_level=bool(counter & 1))
            n_in, N, d = assert_norm_batch(ref, eng.result(0), indptr, indices, fan)
            hubs = max(hubs, int(d.max()))
        eng.close()
    assert hubs > 1                                       # some weights were not 1


def test_short_feature_buffer_and_stale_rows(K, oracle):
    """(a) A buffer poisoned in front of the batch: rows [n_in + N, ...) are never written and runs without draws are stored +0.0.
    (b) The published capacity cut below n_in + N: the rows below it are the expected ones, nothing at or beyond it is written."""
    V, F = 500, 8
    indptr, indices, labels, seeds = holes_graph(5, V)
    feats = (np.random.RandomState(9).rand(V, F) + 1.0).astype(np.float32)
    B, fan = 100, [5, 3]
    seeds = seeds[:2 * B + 9]
    orc = oracle.OracleRunner(indptr, indices, feats, V, F, B, fan)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(seeds, labels[seeds])]))
    L = K.lib()
    feat = eng.out[0][0]["feat"]
    full_rows = eng.feature_rows
    poison = np.frombuffer(b"\xa5\xa5\xa5\xa5", np.uint32)[0]
    for it, cut in ((0, None), (2, None), (0, 7)):
        ref = orc.run_batch(seeds, labels[seeds], it)
        n_in, N, run_dst, S, d = expected_nbr_sum_norm(ref, indptr, indices, fan)
        cap = full_rows if cut is None else n_in + N - cut
        assert n_in < cap <= full_rows
        L.GPUMemoryPool_SetFeatureRows(eng.pools[0], cap)
        eng.feature_rows = cap
        L.d_memset_async(feat.ptr, 0xA5, feat.nbytes, None)
        L.d_stream_sync(None)
        eng.run_batch(0, it, agg_last_hop=True, agg_norm="both")
        got = eng.result(0)
        assert_batch_equal(ref, got, keys=KEYS_NO_FEATURES)
        assert np.array_equal(got["out_deg"], d)
        rows = min(n_in + N, cap) - n_in
        assert_bits("features", got["features"], np.asarray(ref["features"])[:n_in])
        assert_bits("nbr_sum", got["nbr_sum"], S[:rows])
        rest = feat.to_numpy(np.uint32, (full_rows - n_in - rows) * F, offset_bytes=(n_in + rows) * F * 4)
        assert (rest == poison).all()
        if cut is None:
            empty = ~S.view(np.uint32).any(axis=1)
            assert empty.any() and not got["nbr_sum"][empty].view(np.uint32).any()
    eng.close()


def test_feature_sources_host_table_cache_and_clique(K, oracle, small_ds):
    """The weighted sums read the source the plain ones read: a pinned-host table, a Kg = 1 cache built from a pre-sampling epoch, a
    G = 2 logical clique with in-kernel peer reads."""
    ds = small_ds
    V, F = ds.spec.V, ds.spec.F
    L = K.lib()
    B, fan = 300, [10, 5]
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, V, F, B, fan)
    eng = make_engine(K, ds, B, fan, csr_location=K.LOC_HOST_PINNED, features_location=K.LOC_HOST_PINNED)
    for it in (0, 3):
        eng.run_batch(0, it, agg_last_hop=True, agg_norm="both", per_level=(it == 0))
        assert_norm_batch(orc.run_batch(ds.train, ds.labels[ds.train], it), eng.result(0), ds.indptr, ds.indices, fan)
    eng.close()
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
                eng.run_batch(g, it, agg_last_hop=True, agg_norm="both", per_level=(it == 0))
                assert_norm_batch(ref, eng.result(g), ds.indptr, ds.indices, fan)
                slot = fmap[ref["ids"][int(ref["nc"][3 + 2 * len(fan)]):]]         # the last hop's new nodes: hits and misses were summed
                assert (slot >= 0).any() and (slot < 0).any()
                if G == 2:
                    assert ((slot >= 0) & (slot // (V // 8) != g)).any()          # ... and rows of the peer's shard
        eng.close()


def test_launcher_refusals(K, oracle, small_ds, monkeypatch):
    """GPUMemoryPool_SetAggNorm: refused by name without the aggregated mode, with an unknown norm and while capturing; and every
    refusal of get_feature_kernel_agg holds in the normalised mode (before the last hop, no feature buffer, the exchange gather)."""
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
    refused("GPUMemoryPool_SetAggNorm: the pool does not aggregate the last hop", lambda: L.GPUMemoryPool_SetAggNorm(pool, 1))
    assert L.GPUMemoryPool_GetAggNorm(pool) == 0 and not L.GPUMemoryPool_GetAggOutDeg(pool)
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    refused("GPUMemoryPool_SetAggNorm: unknown norm", lambda: L.GPUMemoryPool_SetAggNorm(pool, 3))
    L.GPUMemoryPool_SetAggNorm(pool, 1)
    K.check()
    assert L.GPUMemoryPool_GetAggNorm(pool) == 1 and L.GPUMemoryPool_GetAggOutDeg(pool)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
    refused("before the last hop", agg)
    L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, fan[0], 2, 0)
    refused("before the last hop", agg)
    L.d_stream_sync(None)
    L.GPUCache_SetPreSc(eng.cache, 0)
    st = L.d_stream_create()
    assert L.GPUMemoryPool_BeginBatchCapture(pool, st) == 0
    refused("GPUMemoryPool_SetAggNorm: the pool is being captured", lambda: L.GPUMemoryPool_SetAggNorm(pool, 0))
    eng.run_batch(0, 0, stream=st, sync=False, agg_last_hop=True, agg_norm="both")
    g = L.GPUMemoryPool_EndBatchCapture(pool, st)
    K.check()
    assert g and L.GPUMemoryPool_GetAggNorm(pool) == 1
    eng._graphs.append(g)
    for q in range(eng.depth):
        L.GPUMemoryPool_SetFloatFeatures(pool, None, q)
    eng.run_batch(0, 0, gather=False, agg_last_hop=True, agg_norm="both")
    refused("feature buffer of the current pipe is not set", agg)
    for q in range(eng.depth):
        L.GPUMemoryPool_SetFloatFeatures(pool, eng.out[0][q]["feat"].ptr, q)
    monkeypatch.setenv("LEGION_PEER_GATHER", "exchange")
    refused("LEGION_PEER_GATHER=exchange cannot serve the aggregated last hop", agg)
    monkeypatch.delenv("LEGION_PEER_GATHER")
    with pytest.raises(ValueError):
        eng.run_batch(0, 0, agg_norm="both")               # the engine's own: only together with agg_last_hop
    with pytest.raises(ValueError):
        eng.run_batch(0, 0, agg_last_hop=True, agg_norm="left")
    # and the engine still produces the expected batch in all three modes, the recorded graph included
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    ref = orc.run_batch(ds.train, ds.labels[ds.train], 2)
    eng.run_batch(0, 2, agg_last_hop=True, agg_norm="both")
    assert_norm_batch(ref, eng.result(0), ds.indptr, ds.indices, fan)
    eng.run_batch(0, 2, agg_last_hop=True)
    assert_plain_agg_batch(ref, eng.result(0), ds.indptr, ds.indices, fan)
    eng.run_batch(0, 2)
    assert_batch_equal(ref, eng.result(0))
    eng.close()
    L.d_stream_destroy(st)


@pytest.mark.parametrize("graph", [False, True])
def test_overlapped_two_stream_schedule_normalised(K, oracle, small_ds, graph):
    """Depth 2: batch i + 1 is sampled on one stream while batch i's degrees, weights and sums run on the other, 10 consecutive batches,
    each equal to its serial result.  The sampler of batch i + 1 overwrites the pool's draw buffer, slot states, tile prefixes and the
    position table meanwhile: this is the test that fails if the new passes read anything but the pipe's own draws, COO and counters.
    graph=True: the sampler side replayed as a recorded hipGraph per pipe."""
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
    L.GPUMemoryPool_SetAggNorm(pool, 1)
    graphs = [eng.capture_batch(0, gather=False, pipe=q, stream=s_samp, agg_last_hop=True, agg_norm="both") for q in (0, 1)] if graph else None
    assert L.GPUMemoryPool_GetAggLastHop(pool) == 1 and L.GPUMemoryPool_GetAggNorm(pool) == 1

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
        got = eng.result(0, pipe=i % 2, aggregated=True, normalised=True)
        assert_norm_batch(orc.run_batch(ds.train, ds.labels[ds.train], i), got, ds.indptr, ds.indices, fan)
    eng.close()
    for s in (s_samp, s_gath):
        L.d_stream_destroy(s)


def test_whole_batch_as_one_graph(K, oracle, small_ds):
    """The normalised batch recorded as ONE hipGraph per pipe (sampler, gathers of the levels < H, the three passes, the sums) and replayed."""
    ds = small_ds
    B, fan = 200, [10, 5]
    L = K.lib()
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    eng = make_engine(K, ds, B, fan, pipeline_depth=2)
    L.GPUCache_SetPreSc(eng.cache, 0)
    graphs = [eng.capture_batch(0, pipe=q, agg_last_hop=True, agg_norm="both", per_level=(q == 0)) for q in (0, 1)]
    last = (len(ds.train) - 1) // B
    for n, it in enumerate((0, 1, 2, 5, last, 0)):
        q = n % 2
        eng.run_graph(graphs[q], it)
        assert_norm_batch(orc.run_batch(ds.train, ds.labels[ds.train], it), eng.result(0, pipe=q), ds.indptr, ds.indices, fan)
    eng.close()


def test_link_prediction_duplicate_seeds_one_hop(K, oracle, synth, small_ds):
    """H = 1 over [src | pos | neg] seed thirds with duplicates inside a batch: one run per seed SLOT, the duplicates' edges name the seed's
    last occurrence (the reference's position_map), and the out-degrees count positions, not slots."""
    ds = small_ds
    B, fan = 96, [5]
    seeds = synth.lp_trainingset(ds, 300, B, seed=3)
    seeds[5] = seeds[40]
    seeds[B + 7] = seeds[B + 8]
    seeds[2 * B + 1] = seeds[2 * B + 90]
    lab = ds.labels[seeds]
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, ds.spec.V, ds.spec.F, B, fan)
    eng = make_engine(K, ds, B, fan, seeds=dict(train=[(seeds, lab)]))
    for counter in range(3):
        ref = orc.run_batch(seeds, lab, counter)
        eng.run_batch(0, counter, agg_last_hop=True, agg_norm="both", per_level=bool(counter & 1))
        assert_norm_batch(ref, eng.result(0), ds.indptr, ds.indices, fan)
    eng.close()


def test_full_papers100m_shape(K, oracle, synth):
    """papers100M, {25, 10, 5}, 8000 seeds, two batches at full shape: millions of slots through the chunked slot -> edge prefix (every
    chunk of the 2048 in use), millions of degree atomics, hub positions.  Sampling against the (OpenMP) oracle on a host copy of the
    CSR; the expected sums from the oracle's batch and the generator's feature rows."""
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
    for it in (0, 1):
        ref = orc.run_batch(h_tr, h_lab, it, gather=False, omp=True)
        x = np.concatenate([synth.features(spec, ref["ids"][i:i + 200000]) for i in range(0, len(ref["ids"]), 200000)])
        eng.run_batch(0, it, agg_last_hop=True, agg_norm="both", per_level=(it != 1))
        n_in, N, d = assert_norm_batch(ref, eng.result(0), h_indptr, h_indices, fan, x=x)
        assert N > 500000 and n_in > 100000 and int(d.max()) > 1
        print("papers100M batch %d: n %d, edges %d, largest out-degree %d" % (it, len(d), int(d.sum()), int(d.max())))
    eng.close()


# ---------------------------------------------------------------------------------------------------
# served: the `legion` binary -> ipc_service.get_next_aggregated_norm
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan,graph", [([10, 5], "0"), ([10, 5], "1"), ([5, 4, 3], "1"), ([6], "0")])
def test_server_binary_serves_normalised_batches(tmp_path, synth, oracle, fan, graph):
    """LEGION_AGG_LAST_HOP=1 LEGION_AGG_NORM=both: a fresh trainer process sees aggregate_norm() == 1, get_next and get_next_aggregated
    raise there, and every batch of the schedule (train + valid + test steps, two epochs) through get_next_aggregated_norm equals the
    oracle's default batch + the NumPy statement; the degrees the trainer counts from its COO are the statement's.  graph = 1: the
    runner's LEGION_BATCH_GRAPH=1 path."""
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    data = str(tmp_path / "ds") + "/"
    synth.write_legion_files(ds, data)
    B, epochs = 512, 2
    env = dict(LEGION_BATCH_GRAPH=graph, LEGION_AGG_LAST_HOP="1", LEGION_AGG_NORM="both")
    with served(tmp_path, synth.meta_config_line(ds, data, B, 1 << 40, epochs, 0), fan, env=env) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["norm", spec.F, epochs, OUT])
        srv.finish()
    H = len(fan)
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B)
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, spec.V, spec.F, B, fan)
    assert got["hops"] == H and steps[1] > 0 and steps[2] > 0
    for rec, ref, mode, local in replay_served(got, orc, sets, ds.labels, steps, epochs, bs):
        n_in, N, run_dst, S, d = expected_nbr_sum_norm(ref, ds.indptr, ds.indices, fan)
        assert (rec["n"], rec["n_in"], rec["runs"]) == (int(ref["nc"][5 + 2 * H]), n_in, N)
        assert rec["edges"] == [int(ref["ec"][2 + (H - k + 1)]) for k in range(1, H + 1)]
        assert rec["ids"] == sha(ref["ids"]) and rec["labels"] == sha(ref["labels"]) and rec["src"] == sha(ref["src_off"]) and rec["dst"] == sha(ref["dst_off"])
        assert rec["features"] == sha(ref["features"][:n_in]) and rec["nbr_sum"] == sha(S) and rec["out_deg"] == sha(d), rec["b"]
    text = srv.log_text()
    assert "Hand-off: the last hop as neighbour sums" in text and "normalised by out-degree^-1/2 inside block 1 (LEGION_AGG_NORM=both)" in text


def test_torch_gcn_trainer_trains_on_normalised_batches(tmp_path, synth):
    """examples/legion_sage_torch.py --model gcn --aggregated (first layer GraphConvBothFused over get_next_aggregated_norm) against the server
    binary with LEGION_AGG_LAST_HOP=1 LEGION_AGG_NORM=both: every epoch reports, and the loss is finite and falls -- the criterion
    test_gpu_ipc.py applies to GraphConvBoth on the default hand-off (GraphConv has no self term)."""
    spec = synth.spec_for("products", scale=0.02)
    ds = synth.generate(spec)
    ds.features[np.arange(spec.V), ds.labels % spec.F] += 3.0
    data = str(tmp_path / "ds") + "/"
    synth.write_legion_files(ds, data)
    B, epochs, fan = 512, 4, [10, 5]
    path = os.pathsep.join([os.path.join(ROOT, "legion-1_amd", "ipc_service"), os.environ.get("PYTHONPATH", "")])
    env = dict(LEGION_BATCH_GRAPH="1", LEGION_AGG_LAST_HOP="1", LEGION_AGG_NORM="both", PYTHONPATH=path)
    with served(tmp_path, synth.meta_config_line(ds, data, B, 1 << 40, epochs, 0), fan, env=env) as srv:
        said = srv.run_one([sys.executable, os.path.join(ROOT, "examples", "legion_sage_torch.py"), "--features_num", str(spec.F),
                            "--class_num", str(spec.classes), "--hidden_dim", "64", "--learning_rate", "0.01", "--drop_rate", "0.1",
                            "--epoch", str(epochs), "--model", "gcn", "--aggregated", "--seed", "0"], timeout=400)
        srv.finish()
    lines = [l for l in said.splitlines() if l.startswith("Epoch:")]
    assert len(lines) == epochs and "Accuracy on test data:" in said, said
    losses = [float(l.split("Train Loss:")[1].split(",")[0]) for l in lines]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], said


@pytest.mark.parametrize("env,words", [
    (dict(LEGION_AGG_NORM="both"), ("LEGION_AGG_NORM=both needs LEGION_AGG_LAST_HOP=1",)),
    (dict(LEGION_AGG_NORM="both", LEGION_AGG_LAST_HOP="0"), ("LEGION_AGG_NORM=both needs LEGION_AGG_LAST_HOP=1",)),
    (dict(LEGION_AGG_NORM="right", LEGION_AGG_LAST_HOP="1"), ("LEGION_AGG_NORM=right is not a known norm", "`both`")),
    (dict(LEGION_AGG_NORM="1", LEGION_AGG_LAST_HOP="1"), ("LEGION_AGG_NORM=1 is not a known norm",)),
])
def test_boot_refusals(tmp_path, synth, env, words):
    """The `legion` binary refuses a LEGION_AGG_NORM it cannot serve by name, at boot, before it reads the dataset: exit code 1."""
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write(synth.meta_config_line(ds, str(tmp_path / "nowhere") + "/", 512, 1 << 40, 1, 0))
    cenv = child_env(ipc_namespace("boot"), **dict(dict(LEGION_AGG_LAST_HOP=None, LEGION_BATCH_GRAPH=None), **env))
    r = subprocess.run([SERVER, "1", "0", "10,5", meta], env=cenv, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    said = r.stdout + r.stderr
    assert r.returncode == 1 and "Server_Initialize:" in said and all(w in said for w in words), said[-2000:]
    assert "System is ready for serving" not in said
