"""The distinct-draw sampler mode (k_sample<TILE, SRC, DrawRule::Distinct>) where the suite's stress tests had never seen it: on both
sides of the tile switch, in the wide pre-sampling and the wide partitioned instantiations behind a chunked cache, at chosen degrees around
the take-all / Floyd boundary inside whole batches, switched per batch together with the hand-off mode and recorded batch graphs, served
with the aggregated hand-offs, and refused at boot with a fan-out it cannot run.  Run with `pytest -m gpu`.

The expected batch is tests/distinctref.py's for a distinct batch and the CPU oracle's for a replace batch, compared with
conftest.assert_batch_equal on every key; aggregated results are held bit for bit against tests/aggref.py / tests/gcnref.py fed with that
batch (part D's distinct batches on graphs with holes: distinctcases.expected_sums, the same statement with a run's draws counted from the
batch -- aggref recounts them as the default mode would draw).  Every input is built by tests/distinctcases.py and held to its purpose on the CPU by tests/test_distinct_cases_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import distinctcases as X
import distinctref as D
from aggref import expected_nbr_sum
from conftest import KEYS_NO_FEATURES, assert_batch_equal, sha
from gcnref import expected_nbr_sum_norm
from harness import K, OUT, SERVER, assert_served_record, child_env, ipc_namespace, make_engine, replay_served, serve_sets, served  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu


def assert_bits(name, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %d words differ" % (name, int((a != b).sum()))


def set_env(monkeypatch, **values):
    for name, val in values.items():
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))


# ---------------------------------------------------------------------------------------------------
# A. the tile switch
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def switch_graph():
    return X.switch_graph()


@pytest.mark.parametrize("B,fan,tiles,straddling", X.SWITCH_CASES, ids=["%d-%s" % (c[0], "-".join(map(str, c[1]))) for c in X.SWITCH_CASES])
def test_distinct_batches_do_not_depend_on_the_tile_of_a_hop(K, oracle, switch_graph, B, fan, tiles, straddling):
    """Hop bounds on either side of kNarrowSlots with fan-outs that do not divide a tile (25, 63, 3: rows of d > f lie across the edges of
    the tile the hop runs, counted on the CPU) and the one that does (64): two full batches, the short last one and the first again in the
    distinct mode, and one replace batch in between against the oracle."""
    g = switch_graph
    assert X.hop_tiles(B, fan) == tiles
    seeds = X.switch_seeds(g, B, fan)
    lab = g["labels"][seeds]
    st = X.Statement(g["indptr"], g["indices"], g["feats"], B, fan)
    orc = oracle.OracleRunner(g["indptr"], g["indices"], g["feats"], g["V"], g["F"], B, fan)
    eng = make_engine(K, (g["V"], g["F"], g["indptr"], g["indices"], g["feats"]), B, fan, seeds=dict(train=[(seeds, lab)]))
    want = {}
    for n, counter in enumerate(X.SWITCH_BATCHES):
        if counter not in want:
            want[counter] = st.run_batch(seeds, lab, counter)
        eng.run_batch(0, counter, sample="distinct", per_level=bool(n & 1))
        assert_batch_equal(want[counter], eng.result(0))
        assert want[counter]["ec"][2 + len(fan)] > 0
        if n == 1:
            eng.run_batch(0, counter)
            assert_batch_equal(orc.run_batch(seeds, lab, counter), eng.result(0))
    eng.close()


# ---------------------------------------------------------------------------------------------------
# B. wide pre-sampling and wide partitioned hops
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_bytes,peer,lookup", [(None, None, "fused"), (None, "exchange", "pass"), (40000, None, "pass"), (40000, "exchange", "fused")])
def test_wide_presampling_and_partitioned_hops(K, monkeypatch, chunk_bytes, peer, lookup):
    """{25, 10} from 1049 seeds per logical GPU, G = 2 clique on one device: hop 2's bound is 262 250 slots, so its pre-sampling batches run
    k_sample<1024, RowSource::Presc, DrawRule::Distinct> and, behind the cache, k_sample<1024, RowSource::Fragments, DrawRule::Distinct>.  The pre-sampling batches are the
    statement's and edge_access_time its draw counts; then CSR fragments and feature shards in one chunk each or (chunk_bytes) in several;
    peer rows by in-kernel loads or through the exchange; FindFeat as a lookup pass or fused into the gather."""
    L = K.lib()
    set_env(monkeypatch, LEGION_SHARD_CHUNK_BYTES=chunk_bytes, LEGION_PEER_GATHER=peer, LEGION_CACHE_HIT_PERIOD="1" if lookup == "pass" else None)
    g = X.clique_case()
    V, F, B, fan, G = g["V"], g["F"], X.CLIQUE_B, X.CLIQUE_FAN, X.CLIQUE_G
    parts = g["parts"]
    eng = make_engine(K, (V, F, g["indptr"], g["indices"], g["feats"]), B, fan, G=G, seeds=dict(train=[(p, g["labels"][p]) for p in parts]),
                      cache_memory=64 << 20, train_step=2)
    st = X.Statement(g["indptr"], g["indices"], g["feats"], B, fan)
    for m in range(G):
        acc = np.zeros(V, np.uint64)
        for it in range(2):
            eng.run_batch(m, it, is_presc=True, sample="distinct")
            want = st.run_batch(parts[m], g["labels"][parts[m]], it)
            assert_batch_equal(want, eng.result(m, with_features=False), keys=KEYS_NO_FEATURES)
            assert len(want["draws"][1]) > 128 * 1024
            for inp, cnt in want["draw_counts"]:
                np.add.at(acc, inp[inp >= 0], cnt[inp >= 0].astype(np.uint64))
        L.SetGPUDevice(m)
        assert np.array_equal(K.read_dev(L.GPUCache_GetEdgeAccessedMap(eng.cache, m), np.uint64, V), acc)
    eng.build_cache(cache_agg_mode=1, node_capacity=V // 8, edge_capacity=V // 3, train_step=2)
    assert L.GPUCache_Kg(eng.cache) == G and L.GPUCache_EdgeCapacity(eng.cache, 0) == V // 3 and L.GPUCache_NodeCapacity(eng.cache, 0) == V // 8
    for m in range(G):
        L.SetGPUDevice(m)
        assert L.GPUGraphStorage_FragmentRows(eng.graph, m) == V // 3
        counts = [L.GPUGraphStorage_FragmentChunkCount(eng.graph, m, w) for w in (0, 1)] + [L.GPUCache_ShardChunkCount(eng.cache, m)]
        assert all(c > 1 for c in counts) if chunk_bytes else counts == [1, 1, 1], counts
        fmap = K.read_dev(L.GPUCache_GetFeatureMap(eng.cache, m), np.int32, V)
        for it, per_level in ((0, True), (1, False), (2, True)):
            want = st.run_batch(parts[m], g["labels"][parts[m]], it)
            eng.run_batch(m, it, sample="distinct", per_level=per_level)
            assert_batch_equal(want, eng.result(m))
            slot = fmap[want["ids"]]
            assert (slot >= 0).any() and (slot < 0).any() and ((slot >= 0) & (slot // (V // 8) != m)).any()      # hits, misses, rows of the peer's shard
    eng.close()


def test_wide_hops_from_pinned_host_tables(K):
    """the same shape, G = 1, with the CSR and the feature table in pinned host memory"""
    g = X.clique_case()
    V, F, B, fan = g["V"], g["F"], X.CLIQUE_B, X.CLIQUE_FAN
    p = g["parts"][0]
    lab = g["labels"][p]
    st = X.Statement(g["indptr"], g["indices"], g["feats"], B, fan)
    eng = make_engine(K, (V, F, g["indptr"], g["indices"], g["feats"]), B, fan, seeds=dict(train=[(p, lab)]),
                      csr_location=K.LOC_HOST_PINNED, features_location=K.LOC_HOST_PINNED)
    for it, per_level in ((0, True), (2, False)):
        eng.run_batch(0, it, sample="distinct", per_level=per_level)
        assert_batch_equal(st.run_batch(p, lab, it), eng.result(0))
    eng.close()


# ---------------------------------------------------------------------------------------------------
# C. the degree ladder inside whole batches
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", X.LADDER_F)
def test_degree_ladder_inside_whole_batches(K, f):
    """Rows of degree 0, 1, f - 1, f, f + 1, f + 2, 2 f, 255, 256, 257, 65 535, 65 536, 65 537 and 2^20 + 3 on a graph without multi-edges: as
    the seeds (H = 1) and as the neighbours of the seeds (H = 2, fan-outs {2, f}: the same rows in hop 2's input list).  The batch is the
    statement's; and from the GPU's own COO: min(d, f) edges per row, no (slot, neighbour) pair twice, CSR order for d <= f."""
    g = X.ladder_graph(f)
    V, indptr, indices = g["V"], g["indptr"], g["indices"]
    deg = np.diff(indptr)
    for fan, seeds in (([f], g["seeds1"]), ([2, f], g["seeds2"])):
        B = len(seeds)
        lab = g["labels"][seeds]
        eng = make_engine(K, (V, 1, indptr, indices, g["feats"]), B, fan, seeds=dict(train=[(seeds, lab)]))
        eng.run_batch(0, 0, sample="distinct", per_level=(len(fan) == 1))
        got = eng.result(0)
        want = D.run_batch(indptr, indices, g["feats"], seeds, lab, B, 0, fan)
        assert_batch_equal(want, got)
        ids, ec = got["ids"], got["ec"]
        for h, fh in enumerate(fan, start=1):
            e0, e1 = (0 if h == 1 else int(ec[1 + h])), int(ec[2 + h])
            src, dst = ids[got["src_off"][e0:e1]], ids[got["dst_off"][e0:e1]]
            inp = seeds if h == 1 else ids[got["src_off"][(0 if h == 2 else int(ec[h])):e0]]        # the hop's input list: what the hop before it drew
            cnt = np.minimum(deg[inp], fh)
            assert int(cnt.sum()) == e1 - e0, (h, int(cnt.sum()), e1 - e0)
            slot = np.repeat(np.arange(len(inp)), cnt)                   # the input slot of every edge: edges are in slot order
            assert np.array_equal(dst, inp[slot])
            pairs = slot.astype(np.int64) * V + src
            assert len(np.unique(pairs)) == len(pairs), "hop %d repeats a neighbour of an input slot" % h
            start = np.cumsum(cnt) - cnt
            for m in np.nonzero((deg[inp] <= fh) & (deg[inp] > 0))[0]:
                assert np.array_equal(src[start[m]:start[m] + cnt[m]], indices[indptr[inp[m]]:indptr[inp[m] + 1]]), (h, m)
        assert np.array_equal(want["draw_counts"][-1][0], np.arange(14)) and deg[:14].tolist() == g["want"]
        eng.close()


# ---------------------------------------------------------------------------------------------------
# D. randomised differential: sampling mode x hand-off mode x pipe x per_level x plan x recorded graphs
# ---------------------------------------------------------------------------------------------------
def padded(L, table):
    """(what the engine gets, features_pitch): rows at the 128-byte-aligned pitch with poison in the pad floats; (the table, 0) where the dense
    rows already are whole lines"""
    V, F = table.shape
    pitch = L.legion_row_pitch(F)
    if pitch == F:
        return table, 0
    wide = np.full((V, pitch), np.float32(-777.0))
    wide[:, :F] = table
    return wide.reshape(-1), pitch


def check_step(name, s, ref, got, g, fan):
    """one batch of sampling mode s["sample"] and hand-off s["hand_off"] against `ref`, the statement's (distinct) or the oracle's (replace)"""
    hand_off = s.get("hand_off", "default")
    assert (ref["ids"] >= 0).all()
    if hand_off == "default":
        assert "nbr_sum" not in got and "out_deg" not in got
        assert_batch_equal(ref, got, keys=KEYS_NO_FEATURES)
        assert_bits(name + ": features", got["features"], ref["features"])
        return
    assert_batch_equal(ref, got, keys=KEYS_NO_FEATURES)
    norm = hand_off == "norm"
    if s["sample"] == "distinct":
        n_in, N, S, d = X.expected_sums(ref, fan, norm)
    elif norm:
        n_in, N, _, S, d = expected_nbr_sum_norm(ref, g["indptr"], g["indices"], fan)
    else:
        (n_in, N, _, S), d = expected_nbr_sum(ref, g["indptr"], g["indices"], fan), None
    assert got["features"].shape == (n_in, g["table"].shape[1]) and got["nbr_sum"].shape == S.shape, (name, got["features"].shape, got["nbr_sum"].shape, S.shape)
    assert_bits(name + ": features", got["features"], ref["features"][:n_in])
    if norm:
        assert np.array_equal(got["out_deg"], d), name + ": out_deg"
    else:
        assert "out_deg" not in got
    assert_bits(name + ": nbr_sum", got["nbr_sum"], S)


@pytest.mark.parametrize("seed", range(int(os.environ.get("LEGION_STRESS_DISTINCT_N", "16"))))
def test_randomised_distinct_differential(K, oracle, seed):
    """Random graphs (hubs, isolated nodes, -1 entries, self loops, repeated seeds), V, F, H = 1..4, fan-outs 1..11 before a last fan-out in
    {1, 2, 7, 8, 9, 25, 40, 64}, padded pitch, device or pinned-host table and CSR, one or two pipes; on one engine a sequence of batches whose
    sampling mode, hand-off mode, per_level, plan, pipe and counter are drawn per batch: all six (sampling, hand-off) states, both sampling
    switches with the hand-off kept and changed, the short last batch followed by batch 0 on the same pipe.  One batch graph per sampling
    mode is recorded before the sequence and replayed twice, each time directly behind a run_batch of the OTHER mode on the same pool: the
    replay gives its recorded mode's batch and the run_batch behind it its own.  The configuration is printed: pytest shows it on failure."""
    L = K.lib()
    cfg, g, seq = X.random_config(seed)
    print("seed %d -> %s" % (seed, cfg))
    for s in seq:
        print("   ", s)
    V, F, fan, B = cfg["V"], cfg["F"], cfg["fan"], cfg["B"]
    seeds, lab = g["seeds"], g["labels"][g["seeds"]]
    feats, pitch = padded(L, g["table"]) if cfg["pitched"] else (g["table"], 0)
    orc = oracle.OracleRunner(g["indptr"], g["indices"], g["table"], V, F, B, fan)
    st = X.Statement(g["indptr"], g["indices"], g["table"], B, fan)
    refs = {}

    def ref_of(sample, counter):
        if (sample, counter) not in refs:
            refs[(sample, counter)] = (st if sample == "distinct" else orc).run_batch(seeds, lab, counter)
        return refs[(sample, counter)]

    eng = make_engine(K, (V, F, g["indptr"], g["indices"], feats), B, fan, seeds=dict(train=[(seeds, lab)]), features_pitch=pitch,
                      features_location=K.LOC_HOST_PINNED if cfg["host_table"] else K.LOC_DEVICE,
                      csr_location=K.LOC_HOST_PINNED if cfg["host_csr"] else K.LOC_DEVICE, pipeline_depth=cfg["pipeline_depth"])
    L.GPUCache_SetPreSc(eng.cache, 0)
    graphs = {m: eng.capture_batch(0, pipe=c["pipe"], per_level=c["per_level"], sample=m) for m, c in cfg["graphs"].items()}
    for i, s in enumerate(seq):
        name = "step %d %s" % (i, s)
        ref = ref_of(s["sample"], s["counter"])
        if s.get("replay"):
            pipe = cfg["graphs"][s["sample"]]["pipe"]
            eng.run_graph(graphs[s["sample"]], s["counter"])
            check_step(name, s, ref, eng.result(0, pipe=pipe, aggregated=False, normalised=False), g, fan)
        else:
            eng.run_batch(0, s["counter"], per_level=s["per_level"], plan=s["plan"], pipe=s["pipe"], sample=s["sample"], **X.HAND_OFFS[s["hand_off"]])
            check_step(name, s, ref, eng.result(0, pipe=s["pipe"]), g, fan)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# E. served: LEGION_SAMPLING=distinct with the aggregated hand-offs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan,graph,norm", [([10, 5], "0", None), ([25, 10, 5], "1", None), ([10, 5], "1", "both")])
def test_server_binary_serves_distinct_aggregated_batches(tmp_path, synth, oracle, fan, graph, norm):
    """LEGION_SAMPLING=distinct LEGION_AGG_LAST_HOP=1 (and LEGION_AGG_NORM=both): the feature buffer is sized from max(n_in + N) of a
    pre-sampling epoch that draws distinct neighbours itself.  A fresh trainer reads sampling() == "distinct", and every record of two epochs
    (train + valid + test steps) equals the statement's batch and the sums' statement over it; no batch was short of buffer rows."""
    workload, scale, B, epochs = "products", 0.004, 512, 2
    spec = synth.spec_for(workload, scale=scale)
    ds = synth.generate(spec)
    assert not (ds.indices < 0).any()                   # aggref / gcnref count a run's draws as min(d, f): right for a distinct batch without holes
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    meta_line = "synth:%s:%r %d %d %d %d %d %d %d %d %d 0" % (workload, scale, B, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, 1 << 40, epochs)
    env = dict(LEGION_SAMPLING="distinct", LEGION_AGG_LAST_HOP="1", LEGION_AGG_NORM=norm, LEGION_BATCH_GRAPH=graph, LEGION_SYNTH_CACHE=None)
    with served(tmp_path, meta_line, fan, env=env) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["norm" if norm else "agg", spec.F, epochs, OUT])
        srv.finish()
    text = srv.log_text()
    assert got["sampling"] == "distinct" and "(LEGION_SAMPLING=distinct)" in text and "Hand-off: the last hop as neighbour sums" in text
    assert ("(LEGION_AGG_NORM=both)" in text) == bool(norm) and "Feature buffer too small" not in text
    H = len(fan)
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B, n_valid=n_valid, n_test=n_test)
    st = X.Statement(ds.indptr, ds.indices, ds.features, B, fan)
    assert got["hops"] == H and steps[1] > 0 and steps[2] > 0
    for rec, ref, mode, local in replay_served(got, st, sets, ds.labels, steps, epochs, bs):
        if norm:
            n_in, N, run_dst, S, d = expected_nbr_sum_norm(ref, ds.indptr, ds.indices, fan)
            assert rec["out_deg"] == sha(d), rec["b"]
        else:
            n_in, N, run_dst, S = expected_nbr_sum(ref, ds.indptr, ds.indices, fan)
        assert (rec["n"], rec["n_in"], rec["runs"]) == (int(ref["nc"][5 + 2 * H]), n_in, N)
        assert_served_record(rec, ref, H, keys=("n", "edges", "ids", "labels", "src", "dst"))
        assert rec["features"] == sha(ref["features"][:n_in]) and rec["nbr_sum"] == sha(S), rec["b"]


# ---------------------------------------------------------------------------------------------------
# F. boot: a fan-out the distinct mode cannot run
# ---------------------------------------------------------------------------------------------------
def test_boot_refuses_distinct_sampling_with_a_fan_out_above_64(tmp_path, synth):
    """LEGION_SAMPLING=distinct with fan-outs 65,2: refused by name at boot, exit code 1, before the dataset is read -- not batch by batch by
    the launcher, the pre-sampling epoch first."""
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write(synth.meta_config_line(ds, str(tmp_path / "nowhere") + "/", 512, 1 << 40, 1, 0))
    cenv = child_env(ipc_namespace("boot"), LEGION_SAMPLING="distinct", LEGION_BATCH_GRAPH=None, LEGION_AGG_LAST_HOP=None, LEGION_AGG_NORM=None)
    r = subprocess.run([SERVER, "1", "0", "65,2", meta], env=cenv, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    said = r.stdout + r.stderr
    assert r.returncode == 1 and "Server_Initialize:" in said and "LEGION_SAMPLING=distinct" in said and "at most 64" in said, said[-2000:]
    assert "hop 1 has 65" in said and "Finish Reading All Files" not in said and "dataset file(s) missing" not in said, said[-2000:]


def test_default_sampling_still_serves_a_fan_out_of_65(tmp_path, synth, oracle):
    """the same server with 65,2 and the default mode: the oracle's batches"""
    workload, scale, B, epochs, fan = "products", 0.004, 512, 1, [65, 2]
    spec = synth.spec_for(workload, scale=scale)
    ds = synth.generate(spec)
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    meta_line = "synth:%s:%r %d %d %d %d %d %d %d %d %d 0" % (workload, scale, B, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, 1 << 40, epochs)
    with served(tmp_path, meta_line, fan, env=dict(LEGION_SAMPLING=None, LEGION_AGG_LAST_HOP=None, LEGION_AGG_NORM=None)) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    assert got["sampling"] == "replace"
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B, n_valid=n_valid, n_test=n_test)
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, spec.V, spec.F, B, fan)
    for rec, ref, mode, local in replay_served(got, orc, sets, ds.labels, steps, epochs, bs):
        assert_served_record(rec, ref, len(fan))
