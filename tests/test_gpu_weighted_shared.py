"""Weighted shared-key sampling on the GPU (GPUMemoryPool_SetSharedDraws on top of the weighted kind with GPUMemoryPool_SetWeightedDistinct /
LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1 LEGION_SHARED_DRAWS=1: k_sample<.., DrawRule::WeightedShared> and
weighted_distinct_resolve<true>, csrc/draws.h), through the C ABI and served, against the NumPy statement of tests/wsharedref.py.  Every
check is array_equal -- nc, ec, ids, labels, both COO arrays, the feature rows, the draws every hop parked and, under pre-sampling,
edge_access_time -- except the probe's fp64 key, which is held within 4 ulp.  Every compared batch is first asserted free of near ties
(wsharedref: the cap is zero rows; tests/test_weighted_shared_cpu.py asserts the same without a device).  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import drawrulecases as D
import seededref
import sharedref
import wdistinctref
import weightedref as Wt
import wsharedcases as C
import wsharedref as R
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import expected_sums
from harness import K, OUT, assert_served_record, make_engine, replay_served, serve_sets, served  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

WS = dict(sample="weighted", weighted_distinct=True, shared_draws=True)


def assert_bits(name, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %d words differ" % (name, int((a != b).sum()))


def assert_rule(K, pool):
    L = K.lib()
    assert (L.GPUMemoryPool_GetSampling(pool), L.GPUMemoryPool_GetWeightedDistinct(pool), L.GPUMemoryPool_GetSharedDraws(pool)) == (2, 1, 1)


def run_hop_by_hop(K, eng, counter, want, presc=False, dev=0, seed=None, round=0):
    """The sampler side of batch `counter` under the rule, driven launcher by launcher as Engine.run_batch drives it, with the draws every
    hop parked in the pool's candidate buffer held against the statement's behind each hop.  Returns the batch (no features)."""
    L, pool = K.lib(), eng.pools[dev]
    eng._set_modes(dev, False, None, "weighted", seed, round, None, is_presc=presc, weighted_distinct=True, shared_draws=True)
    assert_rule(K, pool)
    L.GPUMemoryPool_SetCurrentPipe(pool, 0)
    L.GPUMemoryPool_SetCurrentMode(pool, K.TRAINMODE)
    L.GPUMemoryPool_SetIter(pool, counter)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, eng.batch_size, counter, dev, dev, K.TRAINMODE)
    for h, f in enumerate(eng.fanout.tolist()):
        L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, f, 2 * h + 2, int(presc))
        L.d_stream_sync(None)
        K.check()
        ref = want["draws"][h]
        got = K.read_dev(L.GPUMemoryPool_GetCandidateBuffer(pool), np.int32, len(ref))
        assert np.array_equal(got, ref), "hop %d, parked draws: %d of %d differ" % (h + 1, int((got != ref).sum()), len(ref))
    return eng.result(dev, with_features=False)


def statement_batch(st, seeds, lab, it):
    """the statement's batch, after asserting that none of its rows is a near tie"""
    want = st.run_batch(seeds, lab, it)
    assert st.ties == []
    return want


# ---------------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------------
def test_probe_matches_the_statement(K):
    """4096 ids -- 0, V - 1, -1, INT32_MIN and MAX, runs of ids that differ in one bit -- at weights 1e-45 (the smallest subnormal), FLT_MAX,
    the integers 1..16 and 10^-3..10^3, under draw word 0 and two seeded ones.  u exact; key within 4 ulp of NumPy's: the two logs are
    each within about 1 ulp, the rest of the key is correctly rounded (the bound of the probe test of weighted sampling without
    replacement, whose key function this is)."""
    L = K.lib()
    n, V = 4096, D.V
    rng = np.random.RandomState(6)
    ids = rng.randint(-2 ** 31, 2 ** 31 - 1, size=n, dtype=np.int64).astype(np.int32)
    ids[:6] = [0, V - 1, -1, -2 ** 31, 2 ** 31 - 1, 1]
    bits = (np.uint32(1) << np.arange(32, dtype=np.uint32)).view(np.int32)
    ids[64:96] = bits                                                   # one bit each
    ids[96:128] = np.int32(123456789) ^ bits                            # one bit off a common id
    ids[128:2048] = rng.randint(0, V, size=1920)
    w = (10.0 ** rng.uniform(-3, 3, size=n)).astype(np.float32)
    w[128:1024] = rng.randint(1, 17, size=896)
    w[1024:1280], w[1280:1536] = np.float32(1e-45), np.finfo(np.float32).max
    assert w[1024] > 0 and (w > 0).all()
    words = (0, seededref.W(7, 0, 0), seededref.W(0xC0FFEE, 3, 11))
    assert words[1] != 0 and words[2] != 0 and words[1] != words[2]
    mixed = np.array(words, np.uint32)[np.arange(n) % 3]               # one launch more, a word per element
    ids_buf, w_buf, u_buf, key_buf = K.DevBuf.from_numpy(ids), K.DevBuf.from_numpy(w), K.DevBuf(n * 4), K.DevBuf(n * 8)
    seen = []
    for word in [np.full(n, W, np.uint32) for W in words] + [mixed]:
        word_buf = K.DevBuf.from_numpy(word)
        L.legion_weighted_shared_probe(None, ids_buf.ptr, word_buf.ptr, w_buf.ptr, u_buf.ptr, key_buf.ptr, n)
        L.d_stream_sync(None)
        K.check()
        u, key = u_buf.to_numpy(np.uint32, n), key_buf.to_numpy(np.float64, n)
        word_buf.free()
        want_u, want_key = R.node_keys(ids, w, word.astype(np.int64))
        assert np.array_equal(u, want_u)
        assert len(np.unique(u)) == len(np.unique(ids)) or word is mixed    # a bijection under one word: distinct ids, distinct hashes
        ulps = np.abs(key - want_key) / np.spacing(want_key)
        print("key: largest distance %.1f ulp, %d of %d bit-equal" % (ulps.max(), int((key == want_key).sum()), n))
        assert np.isfinite(key).all() and (key > 0).all() and ulps.max() <= 4.0
        seen.append(u)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert not np.array_equal(seen[0], sharedref.node_keys(ids, 0))     # the salt is re-tagged: not the uniform rule's node keys
    for b in (ids_buf, w_buf, u_buf, key_buf):
        b.free()


# ---------------------------------------------------------------------------------------------------
# whole batches on drawrulecases.graph(): both tiles, plain and pre-sampling, draw word 0 and seed 7
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    return C.rule_graph()


class Engines:
    """The engines of this module on drawrulecases.graph(), built on first use and closed with it: one logical GPU with a cache controller
    and the graph's retained weights per tile.  statement(tile, seed, counter): computed once, near ties asserted absent."""

    def __init__(self, K, g):
        self.K, self.g, self.made, self.want = K, g, {}, {}

    def whole(self, tile):
        if tile not in self.made:
            B, fan = D.SHAPES[tile]
            seeds, g = D.seed_list(tile), self.g
            self.made[tile] = make_engine(self.K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, fan, seeds=dict(train=[(seeds, g["labels"][seeds])]),
                                          edge_weights=g["w"], retain_edge_weights=True, cache_memory=int(D.V * D.F * 4 * 0.15), train_step=2)
        return self.made[tile]

    def statement(self, tile, seed, counter):
        key = (tile, seed, counter)
        if key not in self.want:
            B, fan = D.SHAPES[tile]
            seeds, g = D.seed_list(tile), self.g
            self.want[key] = statement_batch(R.Statement(g["graph"], g["feats"], B, fan, seed=seed), seeds, g["labels"][seeds], counter)
        return self.want[key]

    def close(self):
        for eng in self.made.values():
            eng.close()


@pytest.fixture(scope="module")
def engines(K, g):
    e = Engines(K, g)
    yield e
    e.close()


@pytest.mark.parametrize("tile", list(D.SHAPES))
@pytest.mark.parametrize("seed", C.WORDS, ids=["word0", "seed7"])
@pytest.mark.parametrize("kind", ["plain", "presc"])
def test_batches_on_both_tiles_plain_and_presampling(K, engines, kind, seed, tile):
    """Rows of degree 0, 129 and 300, an all-zero row (m = 0 < d) and a row of 40 with weighted -1 holes among the seeds, zero weights (so
    m <= f < d occurs) and multi-edges throughout; wide: f - 1 is lane 63.  The first and the (short) last batch, hop by hop: the parked
    draws of every hop, then nc, ec, ids, labels and both COO arrays.  A pre-sampling batch adds the statement's draws per row to
    edge_access_time, any other nothing; a plain batch is run once more through Engine.run_batch for its feature rows."""
    L = K.lib()
    presc = kind == "presc"
    eng = engines.whole(tile)
    L.SetGPUDevice(0)
    hot = lambda: K.read_dev(L.GPUCache_GetEdgeAccessedMap(eng.cache, 0), np.uint64, D.V)
    before, acc = hot(), np.zeros(D.V, np.uint64)
    for it in D.COUNTERS:
        want = engines.statement(tile, seed, it)
        got = run_hop_by_hop(K, eng, it, want, presc=presc, seed=seed)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        for inp, cnt in want["draw_counts"]:
            np.add.at(acc, inp[inp >= 0], cnt[inp >= 0].astype(np.uint64))
        if not presc:
            eng.run_batch(0, it, per_level=bool(it), seed=seed, **WS)
            assert_batch_equal(want, eng.result(0))
    assert acc.sum() > 0 and np.array_equal(hot() - before, acc if presc else np.zeros(D.V, np.uint64))
    if tile == "narrow" and kind == "plain" and seed is None:             # what the case relies on
        first = engines.statement(tile, None, 0)["draws"][0].reshape(-1, D.SHAPES[tile][1][0])
        assert (first[D.EMPTY] == -1).all() and (first[D.ALL_ZERO] == -1).all() and (first[D.LONG] >= 0).all() and (first[D.HUB] >= 0).all()
        other = wdistinctref.run_batch(engines.g["graph"], engines.g["feats"], D.seed_list(tile), engines.g["labels"][D.seed_list(tile)], D.SHAPES[tile][0], 0, D.SHAPES[tile][1])
        assert not np.array_equal(other["draws"][0], engines.statement(tile, None, 0)["draws"][0])      # not the per-column rule's draws


# ---------------------------------------------------------------------------------------------------
# the graph made by hand (wsharedcases.hand_made_graph)
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    return C.hand_made_graph(C.HAND_SEED)


def hand_engine(K, g, fan, Bh=C.HB, **kw):
    kw.setdefault("retain_edge_weights", True)
    return make_engine(K, (g["V"], g["F"], g["indptr"], g["indices"], g["feats"]), Bh, fan, seeds=dict(train=[(g["seeds"], g["labels"][g["seeds"]])]),
                       edge_weights=g["w"], **kw)


@pytest.mark.parametrize("fan", C.FANS, ids=lambda f: "-".join(map(str, f)))
def test_hand_made_rows_equal_the_statement(K, hand, fan):
    """Every special row is a seed of batch 0; the last batch is short.  Degrees 0, 1, f - 1, f, f + 1 of every fan-out, 129 and 300, a hub
    of 3000 with forty equal columns of one node (exact ties at the cut) and forty of another at different weights, rows with m <= f < d, a
    row whose heavy columns are its last chunk, weights from 1e-30 to 1e30, weighted -1 holes.  Draw word 0 and seed 7."""
    g = hand
    lab = g["labels"][g["seeds"]]
    eng = hand_engine(K, g, fan)
    assert eng.has_retained_edge_weights()
    row = lambda v: g["indices"][int(g["indptr"][v]):int(g["indptr"][v + 1])]
    for seed in C.WORDS:
        st = R.Statement(g["graph"], g["feats"], C.HB, fan, seed=seed)
        for it in C.hand_counters(g):
            want = statement_batch(st, g["seeds"], lab, it)
            got = run_hop_by_hop(K, eng, it, want, seed=seed)
            assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
            eng.run_batch(0, it, per_level=bool(it), seed=seed, **WS)
            assert_batch_equal(want, eng.result(0))
            if it == 0 and seed is None:
                f = fan[0]
                first = want["draws"][0].reshape(-1, f)
                assert (first[0] == -1).all() and (first[C.ALL_ZERO] == -1).all()
                assert first[C.ONE_WEIGHT].tolist() == [int(row(C.ONE_WEIGHT)[7])] + [-1] * (f - 1)
                three = [int(row(C.THREE_WEIGHTS)[c]) for c in (0, 64, 128)]
                assert first[C.THREE_WEIGHTS].tolist() == three + [-1] * (f - 3) if f >= 3 else first[C.THREE_WEIGHTS][0] in three
    eng.close()


# ---------------------------------------------------------------------------------------------------
# composition
# ---------------------------------------------------------------------------------------------------
def narrow_engine(K, g, **kw):
    B, fan = D.SHAPES["narrow"]
    seeds = D.seed_list("narrow")
    kw.setdefault("retain_edge_weights", True)
    return make_engine(K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, kw.pop("fan", fan), seeds=dict(train=[(seeds, g["labels"][seeds])]), edge_weights=g["w"], **kw)


def test_aggregated_hand_offs_on_top(K, g, engines):
    """The plain and the normalised aggregated hand-off over the statement's draws (distinctcases.expected_sums), bit for bit."""
    B, fan = D.SHAPES["narrow"]
    want = engines.statement("narrow", C.SEED, 0)
    eng = narrow_engine(K, g)
    for norm in (False, True):
        eng.run_batch(0, 0, agg_last_hop=True, agg_norm="both" if norm else None, per_level=norm, seed=C.SEED, **WS)
        got = eng.result(0)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        n_in, N, S, d = expected_sums(want, fan, norm)
        assert N > 0 and got["features"].shape[0] == n_in
        assert_bits("features", got["features"], want["features"][:n_in])
        assert_bits("nbr_sum", got["nbr_sum"], S)
        if norm:
            assert np.array_equal(got["out_deg"], d)
    eng.close()


def test_batch_graph_replay_on_both_pipes_and_either_flipped_flag_is_refused(K, g, engines):
    L = K.lib()
    seeds = D.seed_list("narrow")
    lab = g["labels"][seeds]
    eng = narrow_engine(K, g, pipeline_depth=2)
    pool = eng.pools[0]
    L.GPUCache_SetPreSc(eng.cache, 0)
    graphs = [eng.capture_batch(0, pipe=q, per_level=(q == 0), seed=C.SEED, **WS) for q in (0, 1)]
    assert_rule(K, pool)
    for n, it in enumerate((0, 1, 0)):
        q = n % 2
        want = engines.statement("narrow", C.SEED, it)
        eng.run_graph(graphs[q], it)
        assert_batch_equal(want, eng.result(0, pipe=q))
        eng.run_batch(0, it, pipe=q, seed=C.SEED, **WS)                  # the plain run of the same batch
        assert_batch_equal(want, eng.result(0, pipe=q))
    # a graph recorded under the rule does not launch with either flag off ...
    L.GPUMemoryPool_SetSharedDraws(pool, 0)
    with pytest.raises(RuntimeError, match="recorded with shared-key sampling"):
        eng.run_graph(graphs[0], 0)
    L.legion_clear_error()
    L.GPUMemoryPool_SetSharedDraws(pool, 1)
    L.GPUMemoryPool_SetWeightedDistinct(pool, 0)
    with pytest.raises(RuntimeError, match="recorded with weighted sampling without replacement"):
        eng.run_graph(graphs[0], 0)
    L.legion_clear_error()
    # ... nor one recorded under a neighbouring rule with the flag on
    wd = eng.capture_batch(0, pipe=0, seed=C.SEED, sample="weighted", weighted_distinct=True)
    L.GPUMemoryPool_SetSharedDraws(pool, 1)
    with pytest.raises(RuntimeError, match="recorded without shared-key sampling"):
        eng.run_graph(wd, 0)
    L.legion_clear_error()
    eng.run_graph(graphs[1], 1)                                            # back in its own state: replays
    assert_batch_equal(engines.statement("narrow", C.SEED, 1), eng.result(0, pipe=1))
    eng.close()


def test_switching_rules_on_one_pool(K, g, engines):
    """weighted -> weighted without replacement -> weighted shared-key -> shared-key -> replace, and back: each batch equals its own statement."""
    B, fan = D.SHAPES["narrow"]
    seeds = D.seed_list("narrow")
    lab = g["labels"][seeds]
    L = K.lib()
    eng = narrow_engine(K, g)
    a = (g["indptr"], g["indices"], g["feats"], B, fan)
    refs = dict(weighted=Wt.Statement(Wt.Table(g["indptr"], g["indices"], *eng.alias_rows(0)), g["feats"], B, fan), wd=wdistinctref.Statement(g["graph"], g["feats"], B, fan),
                ws=R.Statement(g["graph"], g["feats"], B, fan), shared=sharedref.Statement(*a))
    args = dict(weighted=dict(sample="weighted"), wd=dict(sample="weighted", weighted_distinct=True), ws=WS, shared=dict(sample="distinct", shared_draws=True),
                replace=dict(sample="replace"))
    state = dict(weighted=(2, 0, 0), wd=(2, 1, 0), ws=(2, 1, 1), shared=(1, 0, 1), replace=(0, 0, 0))
    for n, kind in enumerate(("weighted", "wd", "ws", "shared", "replace", "ws", "wd", "ws")):
        it = n % 2
        eng.run_batch(0, it, **args[kind])
        pool = eng.pools[0]
        assert (L.GPUMemoryPool_GetSampling(pool), L.GPUMemoryPool_GetWeightedDistinct(pool), L.GPUMemoryPool_GetSharedDraws(pool)) == state[kind]
        want = D.statement(g, "stream", "narrow", it) if kind == "replace" else refs[kind].run_batch(seeds, lab, it)
        assert_batch_equal(want, eng.result(0))
    assert refs["wd"].ties == [] and refs["ws"].ties == []
    eng.close()


def test_behind_a_cache_with_csr_fragments_the_rule_still_reads_the_whole_csr(K, g, engines):
    """Whole CSR only: the weights lie beside the whole CSR's indices, the fragments have none.  The launcher hands a whole-CSR rule the
    whole CSR's tables whatever the cache holds (launch_sample_hop's refusal of fragment tables under such a rule guards that and cannot
    be reached through the C ABI), so behind a filled clique cache with fragments the batch is still the statement's."""
    L = K.lib()
    B, fan = D.SHAPES["narrow"]
    seeds = D.seed_list("narrow")
    eng = make_engine(K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, fan, G=2, seeds=dict(train=[(seeds, g["labels"][seeds])] * 2),
                      edge_weights=g["w"], retain_edge_weights=True, cache_memory=int(D.V * D.F * 4 * 0.15), train_step=2)
    for dev in range(2):
        for it in D.COUNTERS:
            eng.run_batch(dev, it, is_presc=True, **WS)
    eng.build_cache(cache_agg_mode=1, node_capacity=D.V // 8, edge_capacity=D.V // 3, train_step=2)
    assert L.GPUCache_Kg(eng.cache) == 2 and all(L.GPUGraphStorage_FragmentRows(eng.graph, dev) == D.V // 3 for dev in range(2))
    for dev in range(2):
        for it in D.COUNTERS:
            eng.run_batch(dev, it, per_level=bool(it), **WS)
            assert_batch_equal(engines.statement("narrow", None, it), eng.result(dev))
    eng.close()


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_a_graph_without_retained_weights_is_refused(K, g):
    L = K.lib()
    B = D.SHAPES["narrow"][0]
    eng = narrow_engine(K, g, retain_edge_weights=False)                 # a table, but the weights were not kept
    pool = eng.pools[0]
    assert eng.has_edge_weights() and not eng.has_retained_edge_weights()
    with pytest.raises(ValueError, match="needs the weights kept on the device"):
        eng.run_batch(0, 0, **WS)
    with pytest.raises(ValueError, match="shared_draws=True needs sample='distinct'"):
        eng.run_batch(0, 0, sample="weighted", shared_draws=True)
    # ... and by the library itself, through the launcher: the refusal of weighted sampling without replacement, whose table this is
    L.GPUMemoryPool_SetSampling(pool, 2)
    L.GPUMemoryPool_SetWeightedDistinct(pool, 1)
    L.GPUMemoryPool_SetSharedDraws(pool, 1)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
    L.legion_clear_error()
    L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, 5, 2, 0)
    msg = (L.legion_last_error() or b"").decode()
    assert "GPU_Random_Sampling: weighted sampling without replacement (GPUMemoryPool_SetWeightedDistinct) over a graph without retained edge weights" in msg and "GPUGraphStorage_RetainEdgeWeights" in msg, msg
    L.legion_clear_error()
    L.d_stream_sync(None)
    # shared_draws without weighted_distinct under the weighted kind stays the plain weighted rule, which needs no weights
    L.GPUMemoryPool_SetWeightedDistinct(pool, 0)
    seeds = D.seed_list("narrow")
    ref = Wt.Statement(Wt.Table(g["indptr"], g["indices"], *eng.alias_rows(0)), g["feats"], B, D.SHAPES["narrow"][1]).run_batch(seeds, g["labels"][seeds], 0)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
    for h, f in enumerate(D.SHAPES["narrow"][1]):
        L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, f, 2 * h + 2, 0)
    L.d_stream_sync(None)
    K.check()
    assert L.GPUMemoryPool_GetSharedDraws(pool) == 1
    assert_batch_equal(ref, eng.result(0, with_features=False), keys=KEYS_NO_FEATURES)
    eng.close()


def test_a_fan_out_of_65_is_refused_by_the_rules_name(K, g):
    L = K.lib()
    eng = narrow_engine(K, g, fan=[65])
    pool = eng.pools[0]
    L.GPUMemoryPool_SetSampling(pool, 2)
    L.GPUMemoryPool_SetWeightedDistinct(pool, 1)
    L.GPUMemoryPool_SetSharedDraws(pool, 1)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, 64, 0, 0, 0, K.TRAINMODE)
    L.d_stream_sync(None)
    K.check()
    seeded = eng.result(0, with_features=False)
    L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, 65, 2, 0)
    msg = (L.legion_last_error() or b"").decode()
    assert ("GPU_Random_Sampling: weighted shared-key sampling (GPUMemoryPool_SetWeightedDistinct + GPUMemoryPool_SetSharedDraws) takes a fan-out of at most 64: "
            "k_sample keeps a row's best picks one per lane and stages them in static LDS") in msg, msg
    L.legion_clear_error()
    L.d_stream_sync(None)
    assert_batch_equal(seeded, eng.result(0, with_features=False), keys=KEYS_NO_FEATURES)     # no hop ran
    assert int(seeded["ec"].sum()) == 0
    eng.run_batch(0, 0, sample="weighted")                                # plain weighted keeps accepting 65
    assert int(eng.result(0, with_features=False)["ec"].sum()) > 0
    eng.close()


# ---------------------------------------------------------------------------------------------------
# served: the `legion` binary under LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1 LEGION_SHARED_DRAWS=1 LEGION_SAMPLING_SEED=7
# ---------------------------------------------------------------------------------------------------
class ByRound:
    """The statement behind harness.replay_served, which asks for (ids, labels, local, mode, batch size) in the order of the trainer's
    records: the round of record b is b // (training + validation steps)."""

    def __init__(self, st, got, steps):
        self.st, self.rounds = st, iter([rec["b"] // (steps[0] + steps[1]) for rec in got["batches"]])

    def run_batch(self, ids, lab, counter, mode=0, batch_size=None):
        return self.st.run_batch(ids, lab, counter, mode=mode, batch_size=batch_size, round=next(self.rounds))


def test_server_binary_serves_weighted_shared_key_batches(tmp_path, synth, oracle):
    """A synth: source: the server generates the weights on the device (synth.edge_weights), builds its table of them and keeps them; the
    statement replays the schedule, round by round."""
    workload, scale, B, epochs, fan, S = "products", 0.004, 96, 2, [10, 5], C.SEED
    spec = synth.spec_for(workload, scale=scale)
    ds = synth.generate(spec)
    graph = R.Weights(ds.indptr, ds.indices, synth.edge_weights(ds.E))
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    meta_line = "synth:%s:%r %d %d %d %d %d %d %d %d %d 0" % (workload, scale, B, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, 1 << 40, epochs)
    env = dict(LEGION_SAMPLING="weighted", LEGION_WEIGHTED_DISTINCT="1", LEGION_SHARED_DRAWS="1", LEGION_SAMPLING_SEED=S)
    with served(tmp_path, meta_line, fan, env=env) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    text = srv.log_text()
    assert got["sampling"] == "weighted" and got["sampling_seed"] == S     # the flags are not published: a trainer reads the kind
    assert "Sampling: weighted by edge weight, without replacement, by a key of the neighbour node" in text
    assert "LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1 LEGION_SHARED_DRAWS=1)" in text
    assert "Edge weights: alias table built in HBM" in text and "Edge weights: kept in HBM beside the table" in text
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B, n_valid=n_valid, n_test=n_test)
    plain = R.Statement(graph, ds.features, B, fan, seed=S)
    st = ByRound(plain, got, steps)
    assert got["hops"] == len(fan) and steps[0] >= 3 and steps[1] > 0 and steps[2] > 0
    for rec, ref, mode, local in replay_served(got, st, sets, ds.labels, steps, epochs, bs):
        assert_served_record(rec, ref, len(fan))
    assert plain.ties == []
