"""Edge ids and weights as a trainer receives them (LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1: the pool's per-pipe buffers exported through the
"<name>_ext2" object, ipc_service.get_edge_ids() / get_edge_weights()), the served edge-weighted sums (LEGION_AGG_EDGE_WEIGHT=1) and the
published serving modes, through the `legion` binary, against the NumPy statement of tests/eidref.py replayed over the served schedule.
Every comparison is by SHA-256 of the bytes or array_equal; sums by bit pattern (aggcases.assert_sum_bits).  Two graphs: the weighted graph
of tests/drawrulecases.py written as dataset files (64 x [5, 4] and one [5, 4, 3] run: three training batches per epoch, so both pipes are
reused; validation batches of 301 and 300, the short one; a test batch of 100), and synth:products at the scale and batch size
tests/test_gpu_weighted_distinct.py serves, whose schedule has no near-tie row.  Run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import drawrulecases as D
import eidref as R
import seededref
from aggcases import assert_sum_bits
from conftest import sha
from distinctref import run_batch as plain_run_batch
from edgeaggref import expected_nbr_sum_edge
from eidref import bits
from harness import OUT, assert_served_record, replay_served, serve_sets, served
from weightedref import batch_seeds

pytestmark = pytest.mark.gpu

B, FAN, EPOCHS, SEED = D.SHAPES["narrow"][0], D.SHAPES["narrow"][1], 2, 7
OFF = dict(LEGION_AGG_LAST_HOP=None, LEGION_AGG_NORM=None, LEGION_SAMPLING=None, LEGION_SAMPLING_SEED=None, LEGION_LP_DRAW=None, LEGION_WEIGHTED_DISTINCT=None,
           LEGION_SHARED_DRAWS=None, LEGION_EDGE_IDS=None, LEGION_EDGE_WEIGHTS=None, LEGION_AGG_EDGE_WEIGHT=None, LEGION_BATCH_GRAPH=None)
# rule -> (the sampling variables of its server, the seed)
RULES = dict(stream=(dict(LEGION_SAMPLING="replace"), None),
             distinct=(dict(LEGION_SAMPLING="distinct", LEGION_SAMPLING_SEED=SEED), SEED),
             wdistinct=(dict(LEGION_SAMPLING="weighted", LEGION_WEIGHTED_DISTINCT="1"), None),
             shared=(dict(LEGION_SAMPLING="distinct", LEGION_SHARED_DRAWS="1", LEGION_SAMPLING_SEED=SEED), SEED))
NOT_SERVED = "ipc_service.get_edge_%s: the server does not serve edge ids (start it with LEGION_EDGE_IDS=1%s)"
NO_WEIGHTS = "ipc_service.get_edge_weights: the server does not serve edge weights (start it with LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1)"
EDGE_SERVER = "LEGION_AGG_LAST_HOP=1 LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1 LEGION_AGG_EDGE_WEIGHT=1"
NOT_EDGE = "ipc_service.get_next_aggregated_edge_weight: the server does not scale the neighbour sums by edge weight (start it with " + EDGE_SERVER + ") -- call "
IS_EDGE = (": the server scales the neighbour sums by each edge's weight (LEGION_AGG_EDGE_WEIGHT=1): every row of the sums is w_e x the neighbour's features -- "
           "call get_next_aggregated_edge_weight")


class EdgeStatement:
    """eidref.run_batch behind the oracle runner's signature (harness.replay_served), the round of a record from its index as
    tests/test_gpu_shared_draws.py's ByRound has it.  Under a seed only the training list is shuffled (seededref.run_batch), which
    eidref.run_batch does for every list: the other modes' batches are put together here from the same parts.  .ties: the near-tie rows."""

    def __init__(self, g, rule, batch, fan, seed, got, steps):
        self.g, self.rule, self.B, self.fan, self.seed, self.ties = g, rule, batch, list(fan), seed, []
        self.rounds = iter([rec["b"] // (steps[0] + steps[1]) for rec in got["batches"]])

    def run_batch(self, ids, lab, counter, mode=0, batch_size=None, round=None):
        rnd = next(self.rounds) if round is None else round
        bs = self.B if batch_size is None else batch_size
        if self.seed is None or mode == seededref.TRAINMODE:
            return R.run_batch(self.g, self.rule, ids, lab, bs, counter, self.fan, seed=self.seed, round=rnd, ties=self.ties)
        g, log = self.g, []
        indptr = np.asarray(g["indptr"], dtype=np.int64)
        draw = R.recording(R.rule_draw(self.rule, g, batch_seeds(ids, bs, counter), seededref.W(self.seed, rnd, counter), self.ties), log)
        res = plain_run_batch(indptr, g["indices"], g["feats"], ids, lab, bs, counter, self.fan, draw=draw)
        eids = []
        for h, p in enumerate(log):
            inp = np.asarray(res["draw_counts"][h][0], dtype=np.int64)
            eids.append((indptr[np.where(inp >= 0, inp, 0)][:, None] + p)[res["draws"][h].reshape(p.shape) >= 0])
        res["edge_ids"] = np.concatenate(eids).astype(np.int64)
        res["edge_w"] = np.asarray(g["w"], dtype=np.float32)[res["edge_ids"]]
        return res


@pytest.fixture(scope="module")
def case(synth, tmp_path_factory):
    """the drawrulecases graph as a dataset directory with its edge_weights file"""
    g = D.graph()
    rng = np.random.RandomState(11)
    train = np.concatenate([np.arange(5), rng.randint(0, D.V, size=3 * B + 20 - 5)]).astype(np.int32)      # the hand-made rows in batch 0; (n - 1) // 64 = 3 steps
    valid, test = rng.randint(0, D.V, size=601).astype(np.int32), rng.randint(0, D.V, size=100).astype(np.int32)
    spec = synth.SynthSpec("drawrules", D.V, D.F, float(g["indptr"][-1]) / D.V, len(train), len(valid), len(test))
    ds = synth.Dataset(spec, g["indptr"], g["indices"], g["feats"], g["labels"], train, valid, test)
    data = str(tmp_path_factory.mktemp("drawrules"))
    synth.write_legion_files(ds, data)
    g["w"].astype("<f4").tofile(os.path.join(data, "edge_weights"))
    return dict(g=g, ds=ds, data=data, F=D.F, meta=synth.meta_config_line(ds, data, B, 1 << 40, EPOCHS, 0))


@pytest.fixture(scope="module")
def prod(synth):
    """synth:products at scale 0.004, batch 512, fan-outs [10, 5] (tests/test_gpu_weighted_distinct.py's served shape)"""
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    g = dict(indptr=ds.indptr, indices=ds.indices, w=synth.edge_weights(ds.E), feats=ds.features, labels=ds.labels)
    line = "synth:products:%r %d %d %d %d %d %d %d %d %d 0" % (0.004, 512, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, 1 << 40, EPOCHS)
    return dict(g=g, ds=ds, F=spec.F, B=512, fan=[10, 5], n_valid=n_valid, n_test=n_test, meta=line)


_mode_off = {}


def records_with_the_mode_off(tmp_path_factory, what, meta_line, fan, F, env):
    """tests/ipc_client_modes.py's records of the same server without the edge variables: once per (graph, rule, fan-outs), shared, never changed"""
    key = (what, tuple(fan))
    if key not in _mode_off:
        with served(tmp_path_factory.mktemp("off"), meta_line, fan, env=dict(OFF, **env)) as srv:
            _mode_off[key], = srv.run_clients("ipc_client_modes.py", ["plain", F, EPOCHS, OUT])
            srv.finish()
        assert not [f for f in os.listdir("/dev/shm") if srv.env["LEGION_IPC_NAMESPACE"] in f]
    return _mode_off[key]


def check_raw_batch(npz, g, weights):
    """batch 0 as the client dumped it: every edge id lies in its input row's CSR range and names the neighbour the edge leads to"""
    raw = np.load(npz)
    ids, src, dst, eid = (raw[k].astype(np.int64) for k in ("ids", "src", "dst", "edge_ids"))
    assert raw["edge_ids"].dtype == np.int64 and len(eid) == len(src) == len(dst) > 0
    indptr, u = np.asarray(g["indptr"], dtype=np.int64), ids[dst]
    assert ((indptr[u] <= eid) & (eid < indptr[u + 1])).all()
    assert np.array_equal(np.asarray(g["indices"])[eid], ids[src])
    if weights:
        assert np.array_equal(bits(raw["edge_w"]), bits(np.asarray(g["w"], dtype=np.float32)[eid]))
    else:
        assert "edge_w" not in raw.files


def assert_edges_of_record(rec, ref, hops, weights):
    """per block: the ids, and the weights by bit pattern, of the block's prefix of the statement's edges"""
    assert_served_record(rec, ref, hops)
    for k, n in enumerate(rec["edges"]):
        assert rec["eid"][k] == sha(ref["edge_ids"][:n]), "batch %d block %d: edge ids" % (rec["b"], k + 1)
        if weights:
            assert rec["ew"][k] == sha(bits(ref["edge_w"][:n])), "batch %d block %d: edge weights" % (rec["b"], k + 1)
    assert ("ew" in rec) == weights and len(ref["edge_ids"]) == rec["edges"][0]


def serve_and_replay(tmp_path, tmp_path_factory, oracle, what, src, rule, fan, graph, edge_weights=True, batch=B, n_valid=None, n_test=None):
    """One server of the rule with the edge variables on, one ipc_client_edges.py trainer, the whole schedule against the statement; returns
    (the trainer's output, the server's log)."""
    env, seed = RULES[rule]
    on = dict(env, LEGION_EDGE_IDS="1", LEGION_EDGE_WEIGHTS="1" if edge_weights and rule != "wdistinct" else None, LEGION_BATCH_GRAPH=graph)
    with served(tmp_path, src["meta"], fan, env=dict(OFF, **on)) as srv:
        ext2 = [f for f in os.listdir("/dev/shm") if f == srv.env["LEGION_IPC_NAMESPACE"] + "simpleIPCshm_ext2"]       # there once the server is ready
        got, = srv.run_clients("ipc_client_edges.py", ["plain", src["F"], EPOCHS, OUT])
        srv.finish()
    assert len(ext2) == 1 and not [f for f in os.listdir("/dev/shm") if srv.env["LEGION_IPC_NAMESPACE"] in f]
    weights = edge_weights or rule == "wdistinct"
    ds, g, H = src["ds"], src["g"], len(fan)
    (sets,), steps, (bs,) = serve_sets(oracle, ds, batch, n_valid=n_valid, n_test=n_test)
    assert got["hops"] == H and steps[0] >= (3 if what == "files" else 1) and steps[1] > 0 and steps[2] > 0     # the dataset files: both pipes are reused within an epoch
    assert got["modes"] == dict(lp_draw=0, weighted_distinct=rule == "wdistinct", shared_draws=rule == "shared", edge_ids=True, edge_weights=weights, agg_edge_weight=False)
    st = EdgeStatement(g, rule, batch, fan, seed, got, steps)
    for rec, ref, mode, local in replay_served(got, st, sets, ds.labels, steps, EPOCHS, bs):
        assert_edges_of_record(rec, ref, H, weights)
    assert st.ties == []                                    # the cap on near-tie rows is zero
    check_raw_batch(str(tmp_path / "client0.json.npz"), g, weights)
    # nothing the plain trainer records moves when the mode is switched on
    off = records_with_the_mode_off(tmp_path_factory, (what, rule), src["meta"], fan, src["F"], env)
    assert off["steps"] == got["steps"] and len(off["batches"]) == len(got["batches"]) and (off["sampling"], off["sampling_seed"]) == (got["sampling"], got["sampling_seed"])
    for a, b in zip(off["batches"], got["batches"]):
        assert a == {k: b[k] for k in a}, "batch %d: the served batch moved with the edge variables" % a["b"]
    r = got["refused"]
    assert "no batch yet" in r["get_edge_ids_before"] and "no batch yet" in r["get_edge_ids_after_synchronize"]
    assert r["get_next_aggregated_edge_weight"] == NOT_EDGE + "get_next"
    return got, srv.log_text()


@pytest.mark.parametrize("graph", ["0", "1"])
@pytest.mark.parametrize("rule", list(RULES))
def test_served_ids_and_weights_equal_the_statement(tmp_path, tmp_path_factory, oracle, case, rule, graph):
    """Every batch of two epochs, validation and test batches included, under each rule that hands ids over: with replacement plus
    LEGION_EDGE_WEIGHTS=1, distinct under a seed, weighted without replacement (the weights are retained without the variable), shared keys."""
    got, log = serve_and_replay(tmp_path, tmp_path_factory, oracle, "files", case, rule, FAN, graph)
    assert "Hand-off: every sampled edge's position in the whole CSR" in log and "Hand-off: every sampled edge's weight beside its id" in log
    assert ("(LEGION_EDGE_WEIGHTS=1)" in log) == (rule != "wdistinct")
    assert got["sampling"] == dict(stream="replace", distinct="distinct", wdistinct="weighted", shared="distinct")[rule]


def test_three_hops_serve_three_prefixes(tmp_path, tmp_path_factory, oracle, case):
    got, _ = serve_and_replay(tmp_path, tmp_path_factory, oracle, "files", case, "stream", FAN + [3], "0")
    assert all(len(set(rec["edges"])) == 3 and rec["edges"] == sorted(rec["edges"], reverse=True) for rec in got["batches"])      # three blocks, three lengths


@pytest.mark.parametrize("graph", ["0", "1"])
def test_served_from_the_synth_source(tmp_path, tmp_path_factory, oracle, prod, graph):
    """synth:products, weighted sampling without replacement: the server generates the weights on the device and retains them"""
    got, _ = serve_and_replay(tmp_path, tmp_path_factory, oracle, "synth", prod, "wdistinct", prod["fan"], graph, batch=prod["B"], n_valid=prod["n_valid"], n_test=prod["n_test"])
    assert got["modes"]["weighted_distinct"] is True and got["sampling"] == "weighted"


@pytest.mark.parametrize("rule", ["stream", "distinct"])
def test_ids_without_weights(tmp_path, tmp_path_factory, oracle, case, rule):
    """Without LEGION_EDGE_WEIGHTS the graph retains nothing under these kinds: edge_weights() is False, get_edge_weights() raises by name,
    and the ids are served all the same."""
    got, log = serve_and_replay(tmp_path, tmp_path_factory, oracle, "files", case, rule, FAN, "0", edge_weights=False)
    assert got["modes"]["edge_weights"] is False and got["refused"]["get_edge_weights"] == NO_WEIGHTS == got["refused"]["get_edge_weights_before"]
    assert "every sampled edge's weight" not in log and "Edge weights:" not in log


@pytest.mark.parametrize("graph", ["0", "1"])
def test_served_edge_weighted_sums(tmp_path, oracle, case, graph):
    """LEGION_AGG_LAST_HOP=1 LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1 LEGION_AGG_EDGE_WEIGHT=1: the sums by bit pattern against
    edgeaggref.expected_nbr_sum_edge, x_in word for word, the ids and weights of every hop alongside; the other calls refuse by name."""
    g, ds, H = case["g"], case["ds"], len(FAN)
    env = dict(OFF, LEGION_AGG_LAST_HOP="1", LEGION_EDGE_IDS="1", LEGION_EDGE_WEIGHTS="1", LEGION_AGG_EDGE_WEIGHT="1", LEGION_BATCH_GRAPH=graph)
    with served(tmp_path, case["meta"], FAN, env=env) as srv:
        got, = srv.run_clients("ipc_client_edges.py", ["edge", D.F, EPOCHS, OUT])
        srv.finish()
    assert "Hand-off: the sums scaled by each edge's weight (LEGION_AGG_EDGE_WEIGHT=1)" in srv.log_text() and "Feature buffer too small" not in srv.log_text()
    assert got["modes"] == dict(lp_draw=0, weighted_distinct=False, shared_draws=False, edge_ids=True, edge_weights=True, agg_edge_weight=True)
    assert got["refused"]["get_next"] == "ipc_service.get_next" + IS_EDGE and got["refused"]["get_next_aggregated"] == "ipc_service.get_next_aggregated" + IS_EDGE
    assert got["refused"]["get_next_aggregated_norm"] == "ipc_service.get_next_aggregated_norm" + IS_EDGE
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B)
    st = EdgeStatement(g, "stream", B, FAN, None, got, steps)
    raw = np.load(str(tmp_path / "client0.json.npz"))
    for rec, ref, mode, local in replay_served(got, st, sets, ds.labels, steps, EPOCHS, bs):
        n_in, N, run_dst, S = expected_nbr_sum_edge(ref, g["indptr"], g["indices"], FAN)
        assert_served_record(rec, ref, H, keys=("n", "sizes", "edges", "ids", "labels", "src", "dst"))
        assert (rec["n_in"], rec["runs"]) == (n_in, N) and N > 0
        assert np.array_equal(bits(raw["x_in_%d" % rec["b"]]), bits(ref["features"][:n_in]))
        assert_sum_bits("nbr_sum of batch %d" % rec["b"], raw["nbr_sum_%d" % rec["b"]], S)
        for k, n in enumerate(rec["edges"]):                 # the hops < H are block 2's prefix: their weights are what GraphConvEdgeWeight reads
            assert rec["eid"][k] == sha(ref["edge_ids"][:n]) and rec["ew"][k] == sha(bits(ref["edge_w"][:n]))
    check_raw_batch(str(tmp_path / "client0.json.npz"), g, True)


def test_wrong_call_on_servers_that_do_not_scale_the_sums(tmp_path, case):
    """get_next_aggregated_edge_weight on an aggregating and on a normalising server names the call to make instead"""
    for norm, call in ((None, "get_next_aggregated"), ("both", "get_next_aggregated_norm")):
        with served(tmp_path, case["meta"], FAN, env=dict(OFF, LEGION_AGG_LAST_HOP="1", LEGION_AGG_NORM=norm)) as srv:
            got, = srv.run_clients("ipc_client_edges.py", ["norm" if norm else "agg", D.F, EPOCHS, OUT])
            srv.finish()
        assert got["refused"]["get_next_aggregated_edge_weight"] == NOT_EDGE + call
        assert got["refused"]["get_edge_ids"] == NOT_SERVED % ("ids", "") and got["refused"]["get_edge_weights"] == NOT_SERVED % ("weights", " LEGION_EDGE_WEIGHTS=1")


def test_two_logical_gpus_receive_their_own_buffers(tmp_path, oracle, case):
    """G = 2 in one server: each trainer's ids and weights are those of its own device's schedule"""
    g, ds, H, G = case["g"], case["ds"], len(FAN), 2
    env = dict(OFF, LEGION_SAMPLING="distinct", LEGION_EDGE_IDS="1", LEGION_EDGE_WEIGHTS="1")
    with served(tmp_path, case["meta"], FAN, G=G, env=env) as srv:
        gots = srv.run_clients("ipc_client_edges.py", ["plain", D.F, EPOCHS, OUT])
        srv.finish()
    assert srv.log_text().count("Hand-off: every sampled edge's position in the whole CSR") == G
    sets, steps, bs = serve_sets(oracle, ds, B, G)
    assert steps[0] >= 1 and not np.array_equal(sets[0][0], sets[1][0])
    for dev, got in enumerate(gots):
        st = EdgeStatement(g, "distinct", B, FAN, None, got, steps)
        for rec, ref, mode, local in replay_served(got, st, sets[dev], ds.labels, steps, EPOCHS, bs[dev]):
            assert_edges_of_record(rec, ref, H, True)
        check_raw_batch(str(tmp_path / ("client%d.json.npz" % dev)), g, True)
    assert gots[0]["batches"][0]["eid"] != gots[1]["batches"][0]["eid"]


def test_published_words(tmp_path, synth):
    """lp_draw() is the triples per batch on a server that draws the thirds (tests/test_gpu_lp_draw.py's kind); on a plain server every word
    is off and no `_ext2` exists.  weighted_distinct() and shared_draws() on their servers: test_served_ids_and_weights_equal_the_statement."""
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    batch, fan, S = 510, [10, 5], 12345
    line = "synth:products:0.004 %d %d %d %d %d 100 60 0 1 2" % (batch, spec.V, ds.E, spec.F, spec.n_train)
    with served(tmp_path, line, fan, env=dict(OFF, LEGION_SAMPLING_SEED=S, LEGION_LP_DRAW=1)) as srv:
        assert srv.env["LEGION_IPC_NAMESPACE"] + "simpleIPCshm_ext2" in os.listdir("/dev/shm")
        got, = srv.run_clients("ipc_client_edges.py", ["plain", spec.F, 1, OUT])
        srv.finish()
    assert got["modes"] == dict(lp_draw=batch // 3, weighted_distinct=False, shared_draws=False, edge_ids=False, edge_weights=False, agg_edge_weight=False)
    plain = "synth:products:0.004 %d %d %d %d %d 100 60 %d 1 0" % (512, spec.V, ds.E, spec.F, spec.n_train, 1 << 40)
    with served(tmp_path, plain, fan, env=OFF) as srv:
        ns = srv.env["LEGION_IPC_NAMESPACE"]
        names = sorted(f for f in os.listdir("/dev/shm") if ns in f)
        got, = srv.run_clients("ipc_client_edges.py", ["plain", spec.F, 1, OUT])
        srv.finish()
    assert got["modes"] == dict(lp_draw=0, weighted_distinct=False, shared_draws=False, edge_ids=False, edge_weights=False, agg_edge_weight=False)
    assert names == sorted([ns + "simpleIPCshm", ns + "simpleIPCshm_ext"] + ["sem." + ns + "sem_%s_0_%d" % (rw, q) for rw in "rw" for q in (0, 1)]), names
    assert got["refused"]["get_edge_ids"] == NOT_SERVED % ("ids", "")


def test_a_client_refuses_a_server_that_says_edge_ids_but_registered_no_buffers():
    """An env of this process with every hand-off buffer of GPU 0 registered and the `edge_ids` word on, but no edge buffers: a trainer
    must not run on a null edge buffer, so legion_ipc_client_open refuses it by name; with the word off the same env is attached to."""
    import ctypes as C
    import subprocess
    import sys

    from conftest import ROOT
    from harness import child_env, ipc_namespace, load_library
    K = load_library()
    L, ns = K.lib(), ipc_namespace("noreg")
    client = ("import sys, ctypes as C; sys.path.insert(0, %r)\nimport legion1_amd.capi as K\nL = K.lib(); L.legion_set_error_mode(K.ERR_RETURN)\n"
              "c = L.legion_ipc_client_open(0)\nprint('OPENED' if c else 'REFUSED', (L.legion_last_error() or b'').decode())\n"
              "if c: L.legion_ipc_client_close(C.c_void_p(c))\n") % ROOT
    L.legion_ipc_set_namespace(ns.encode())
    e = None
    try:
        e = L.NewIPCEnv(1)
        info = K.LegionBuildInfo()
        info.partition_count, info.epoch, info.raw_batch_size = 1, 1, 64
        sizes = [np.array([x], np.int32) for x in (200, 100, 50)]
        info.training_set_num, info.validation_set_num, info.testing_set_num = (a.ctypes.data for a in sizes)
        L.IPCEnv_Coordinate(e, C.byref(info))
        L.IPCEnv_InitializeSamplesBuffer(e, 64, 1000, D.F, 0, 2)
        L.IPCEnv_InitializeFeaturesBuffer(e, 64, 1000, D.F, 0, 2)
        K.check()
        for word, want in ((1, "legion_ipc_client_open: the server serves edge ids (LEGION_EDGE_IDS=1) but registered no edge buffers for GPU 0 (IPCEnv_RegisterEdgeBuffers;"), (0, "OPENED")):
            L.IPCEnv_SetEdgeIds(e, word)
            r = subprocess.run([sys.executable, "-c", client], env=child_env(ns), capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and want in r.stdout and [ln.split(" ")[0] for ln in r.stdout.splitlines() if ln.startswith(("REFUSED", "OPENED"))] == ["REFUSED" if word else "OPENED"], r.stdout[-1500:] + r.stderr[-1500:]
    finally:
        if e:
            L.IPCEnv_Finalize(e)
        L.legion_clear_error()
        L.legion_ipc_set_namespace(b"")
    assert not [f for f in os.listdir("/dev/shm") if ns in f]
