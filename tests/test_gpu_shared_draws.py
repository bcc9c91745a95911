"""Shared-key sampling on the GPU (GPUMemoryPool_SetSharedDraws on top of the distinct kind / LEGION_SAMPLING=distinct LEGION_SHARED_DRAWS=1:
k_sample<.., DrawRule::Shared> and shared_resolve, csrc/draws.h), through the C ABI and served, against the NumPy statement of
tests/sharedref.py.  Every check is array_equal: nc, ec, ids, labels, both COO arrays, the feature rows, the draws every hop parked and,
under pre-sampling, edge_access_time -- every value is an integer or a copied float, so no tolerance applies and no row is left out.
Run with `pytest -m gpu`."""
import numpy as np
import pytest

import drawrulecases as D
import seededref
import sharedref as R
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import expected_sums
from harness import K, OUT, assert_served_record, make_engine, replay_served, serve_sets, served  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

SD = dict(sample="distinct", shared_draws=True)


def assert_bits(name, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %d words differ" % (name, int((a != b).sum()))


def run_hop_by_hop(K, eng, counter, want, presc=False, dev=0, seed=None, round=0):
    """The sampler side of batch `counter` under the flag, driven launcher by launcher as Engine.run_batch drives it, with the draws every
    hop parked in the pool's candidate buffer held against the statement's behind each hop.  Returns the batch (no features)."""
    L, pool = K.lib(), eng.pools[dev]
    eng._set_modes(dev, False, None, "distinct", seed, round, None, is_presc=presc, shared_draws=True)
    assert L.GPUMemoryPool_GetSampling(pool) == 1 and L.GPUMemoryPool_GetSharedDraws(pool) == 1      # "distinct", with the flag on top
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


# ---------------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------------
def test_probe_matches_the_statement(K):
    """4096 ids -- 0, V - 1, -1, INT32_MIN and MAX, runs of ids that differ in one bit -- under draw word 0 and two seeded ones."""
    L = K.lib()
    n, V = 4096, D.V
    rng = np.random.RandomState(6)
    ids = rng.randint(-2 ** 31, 2 ** 31 - 1, size=n, dtype=np.int64).astype(np.int32)
    ids[:6] = [0, V - 1, -1, -2 ** 31, 2 ** 31 - 1, 1]
    bits = (np.uint32(1) << np.arange(32, dtype=np.uint32)).view(np.int32)
    ids[64:96] = bits                                                   # one bit each
    ids[96:128] = np.int32(123456789) ^ bits                            # one bit off a common id
    ids[128:2048] = rng.randint(0, V, size=1920)
    words = (0, seededref.W(7, 0, 0), seededref.W(0xC0FFEE, 3, 11))
    assert words[1] != 0 and words[2] != 0 and words[1] != words[2]
    ids_buf, key_buf = K.DevBuf.from_numpy(ids), K.DevBuf(n * 4)
    seen = []
    for W in words:
        word_buf = K.DevBuf.from_numpy(np.full(n, W, np.uint32))
        L.legion_shared_draw_probe(None, ids_buf.ptr, word_buf.ptr, key_buf.ptr, n)
        L.d_stream_sync(None)
        K.check()
        key = key_buf.to_numpy(np.uint32, n)
        word_buf.free()
        assert np.array_equal(key, R.node_keys(ids, W))
        assert len(np.unique(key)) == len(np.unique(ids))                # a bijection: distinct ids, distinct keys
        seen.append(key)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    # one launch, a word per element
    mixed = np.array(words, np.uint32)[np.arange(n) % 3]
    word_buf = K.DevBuf.from_numpy(mixed)
    L.legion_shared_draw_probe(None, ids_buf.ptr, word_buf.ptr, key_buf.ptr, n)
    L.d_stream_sync(None)
    K.check()
    assert np.array_equal(key_buf.to_numpy(np.uint32, n), R.node_keys(ids, mixed.astype(np.int64)))
    for b in (ids_buf, key_buf, word_buf):
        b.free()


# ---------------------------------------------------------------------------------------------------
# whole batches: plain, pre-sampling, partitioned; both tiles
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    return D.graph()


class Engines:
    """The engines of this module, built on first use and closed with it, the way tests/test_gpu_draw_rules.py builds them: whole(tile) --
    one logical GPU with a cache controller (plain and pre-sampling hops: the whole CSR); clique(tile) -- Kg = 2 on one device behind a
    filled cache with tiny CSR fragments, both logical GPUs serving the same seed list.  statement(tile, counter): computed once."""

    def __init__(self, K, g):
        self.K, self.g, self.made, self.want = K, g, {}, {}

    def _engine(self, tile, G):
        B, fan = D.SHAPES[tile]
        seeds = D.seed_list(tile)
        g = self.g
        return make_engine(self.K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, fan, G=G, seeds=dict(train=[(seeds, g["labels"][seeds])] * G),
                           cache_memory=int(D.V * D.F * 4 * 0.15), train_step=2)

    def whole(self, tile):
        if ("whole", tile) not in self.made:
            self.made[("whole", tile)] = self._engine(tile, 1)
        return self.made[("whole", tile)]

    def clique(self, tile):
        if ("clique", tile) not in self.made:
            L = self.K.lib()
            eng = self.made[("clique", tile)] = self._engine(tile, 2)
            for dev in range(2):
                for it in D.COUNTERS:
                    eng.run_batch(dev, it, is_presc=True)
            eng.build_cache(cache_agg_mode=1, node_capacity=D.V // 8, edge_capacity=D.V // 3, train_step=2)
            assert L.GPUCache_Kg(eng.cache) == 2 and L.GPUCache_EdgeCapacity(eng.cache, 0) == D.V // 3
            assert all(L.GPUGraphStorage_FragmentRows(eng.graph, dev) == D.V // 3 for dev in range(2))
        return self.made[("clique", tile)]

    def statement(self, tile, counter):
        if (tile, counter) not in self.want:
            B, fan = D.SHAPES[tile]
            seeds, g = D.seed_list(tile), self.g
            self.want[(tile, counter)] = R.run_batch(g["indptr"], g["indices"], g["feats"], seeds, g["labels"][seeds], B, counter, fan)
        return self.want[(tile, counter)]

    def close(self):
        for eng in self.made.values():
            eng.close()


@pytest.fixture(scope="module")
def engines(K, g):
    e = Engines(K, g)
    yield e
    e.close()


@pytest.mark.parametrize("tile", list(D.SHAPES))
@pytest.mark.parametrize("kind", ["plain", "presc", "partitioned"])
def test_batches_on_both_tiles_plain_presampling_and_partitioned(K, engines, kind, tile):
    """drawrulecases.graph(): rows of degree 0, 129, 300 and 40 with holes among the seeds, multi-edges throughout.  The first and the
    (short) last batch, hop by hop: the parked draws of every hop, then nc, ec, ids, labels and both COO arrays.  A pre-sampling batch
    adds the statement's draws per row to edge_access_time, any other nothing; a plain or partitioned batch is run once more through
    Engine.run_batch for its feature rows."""
    L = K.lib()
    presc = kind == "presc"
    eng = engines.clique(tile) if kind == "partitioned" else engines.whole(tile)
    L.SetGPUDevice(0)
    hot = lambda: K.read_dev(L.GPUCache_GetEdgeAccessedMap(eng.cache, 0), np.uint64, D.V)
    before, acc = hot(), np.zeros(D.V, np.uint64)
    for it in D.COUNTERS:
        want = engines.statement(tile, it)
        got = run_hop_by_hop(K, eng, it, want, presc=presc)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        for inp, cnt in want["draw_counts"]:
            np.add.at(acc, inp[inp >= 0], cnt[inp >= 0].astype(np.uint64))
        if not presc:
            eng.run_batch(0, it, per_level=bool(it), **SD)
            assert_batch_equal(want, eng.result(0))
    assert acc.sum() > 0 and np.array_equal(hot() - before, acc if presc else np.zeros(D.V, np.uint64))
    if tile == "narrow" and kind == "plain":                                # what the case relies on: long rows are cut, and rows agree
        first = engines.statement(tile, 0)["draws"][0].reshape(-1, D.SHAPES[tile][1][0])
        assert (first[D.EMPTY] == -1).all() and (first[D.LONG] >= 0).all() and (first[D.HUB] >= 0).all()


# ---------------------------------------------------------------------------------------------------
# a small graph made for the resolve
# ---------------------------------------------------------------------------------------------------
RV = 6000
LATE = 320          # the row whose smallest keys sit in its last chunk: five chunks of 64


def resolve_graph(f):
    """Nodes 0..9 by hand, all seeds of batch 0: degree f, f + 1, 63, 64, 65, 128, 129 and 4000 (one, one, two, three and 63 chunks of 64
    lanes; whole and ragged last chunks), a row of 200 copies of one id (every key ties: the column decides), and a row of 320 distinct
    ids whose 64 smallest keys under draw word 0 sit in its last chunk, columns 256..319, in descending key order (each of them enters
    the best list at its front).  The others: 0..70 random neighbours, multi-edges and -1 holes."""
    rng = np.random.RandomState(4000 + f)
    deg = rng.randint(0, 71, size=RV)
    deg[:10] = [f, f + 1, 63, 64, 65, 128, 129, 4000, 200, LATE]
    indptr = np.zeros(RV + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.randint(0, RV, size=int(indptr[-1])).astype(np.int32)
    indices[rng.rand(len(indices)) < 0.02] = -1
    for v in range(8):                                                     # the hand-made rows hold no hole: min(d, f) edges each
        sl = slice(int(indptr[v]), int(indptr[v + 1]))
        indices[sl] = np.where(indices[sl] < 0, v, indices[sl])
    indices[indptr[8]:indptr[9]] = 4242
    ids = rng.choice(RV, size=LATE, replace=False).astype(np.int32)
    ids = ids[np.argsort(R.node_keys(ids, 0), kind="stable")]              # ascending key
    late = np.concatenate([rng.permutation(ids[64:]), ids[:64][::-1]])     # the 64 smallest last, the smallest of all in the last column
    indices[indptr[9]:indptr[10]] = late
    labels = rng.randint(0, 9, size=RV).astype(np.int32)
    feats = np.random.RandomState(1).rand(RV, 3).astype(np.float32)
    seeds = np.concatenate([np.arange(10), 10 + rng.permutation(RV - 10)[:33]]).astype(np.int32)
    return dict(indptr=indptr, indices=indices, labels=labels, feats=feats, seeds=seeds)


@pytest.mark.parametrize("f", [1, 5, 64])
def test_rows_made_for_the_resolve(K, f):
    """Two hops of fan-out f from 32 seeds, batch 0 (the hand-made rows) and the short batch 1, unseeded and under a draw word."""
    g = resolve_graph(f)
    B, fan = 32, [f, f]
    lab = g["labels"][g["seeds"]]
    st0 = R.Statement(g["indptr"], g["indices"], g["feats"], B, fan)
    row = lambda v: g["indices"][int(g["indptr"][v]):int(g["indptr"][v + 1])]
    first = st0.run_batch(g["seeds"], lab, 0)["draws"][0].reshape(-1, f)
    assert first[9].tolist() == row(9)[LATE - f:].tolist()                  # the f smallest keys: the last f columns
    assert (first[8] == 4242).all() and first[0].tolist() == row(0).tolist()
    assert [(first[v] >= 0).sum() for v in range(10)] == [min(len(row(v)), f) for v in range(10)]     # the hand-made rows hold no hole
    eng = make_engine(K, (RV, 3, g["indptr"], g["indices"], g["feats"]), B, fan, seeds=dict(train=[(g["seeds"], lab)]))
    for seed in (None, 99):
        st = R.Statement(g["indptr"], g["indices"], g["feats"], B, fan, seed=seed)
        for it in (0, 1):
            want = st.run_batch(g["seeds"], lab, it)
            got = run_hop_by_hop(K, eng, it, want, seed=seed)
            assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
            eng.run_batch(0, it, seed=seed, **SD)
            assert_batch_equal(want, eng.result(0))
    eng.close()


# ---------------------------------------------------------------------------------------------------
# seeded, recorded, refused
# ---------------------------------------------------------------------------------------------------
def test_seeded_rounds_and_a_batch_graph_replayed_across_rounds(K, g):
    """Two rounds x two batches under a seed against Statement(seed=...), host-driven and replayed from ONE recording (the draw word and
    the shuffled list travel through the pool's cursor, not through the graph).  A graph recorded with the flag does not launch with it off,
    and the other way round; a switch inside a capture and a fan-out of 65 are refused by name."""
    L = K.lib()
    B, fan, S = 64, [5, 4], 0xC0FFEE
    seeds = D.seed_list("narrow")
    lab = g["labels"][seeds]
    st = R.Statement(g["indptr"], g["indices"], g["feats"], B, fan, seed=S)
    eng = make_engine(K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, fan, seeds=dict(train=[(seeds, lab)]))
    pool = eng.pools[0]
    L.GPUCache_SetPreSc(eng.cache, 0)
    graph = eng.capture_batch(0, seed=S, round=0, **SD)
    assert L.GPUMemoryPool_GetSampling(pool) == 1 and L.GPUMemoryPool_GetSharedDraws(pool) == 1
    seen = {}
    for rnd in (0, 1):
        for it in (0, 1):
            want = seen[(rnd, it)] = st.run_batch(seeds, lab, it, round=rnd)
            eng.run_graph(graph, it, round=rnd)
            assert_batch_equal(want, eng.result(0))
            eng.run_batch(0, it, seed=S, round=rnd, **SD)                  # host-driven
            assert_batch_equal(want, eng.result(0))
    assert not np.array_equal(seen[(0, 0)]["draws"][0], seen[(1, 0)]["draws"][0]) and not np.array_equal(seen[(0, 0)]["ids"], seen[(0, 1)]["ids"])
    # the other state of the flag
    L.GPUMemoryPool_SetSharedDraws(pool, 0)
    with pytest.raises(RuntimeError, match="recorded with shared-key sampling"):
        eng.run_graph(graph, 0)
    L.legion_clear_error()
    plain = eng.capture_batch(0, sample="distinct", seed=S, round=1)
    L.GPUMemoryPool_SetSharedDraws(pool, 1)
    with pytest.raises(RuntimeError, match="recorded without shared-key sampling"):
        eng.run_graph(plain, 0)
    L.legion_clear_error()
    eng.run_graph(graph, 1)                                                # back in its own state: replays
    assert_batch_equal(seen[(1, 1)], eng.result(0))
    # a switch while the pool is being captured
    s = L.d_stream_create()
    assert L.GPUMemoryPool_BeginBatchCapture(pool, s) == 0
    L.GPUMemoryPool_SetSharedDraws(pool, 0)
    msg = (L.legion_last_error() or b"").decode()
    assert "GPUMemoryPool_SetSharedDraws: the pool is being captured" in msg, msg
    L.legion_clear_error()
    empty = L.GPUMemoryPool_EndBatchCapture(pool, s)
    assert empty and L.GPUMemoryPool_GetSharedDraws(pool) == 1
    L.LegionBatchGraph_Delete(empty)
    K.check()
    L.d_stream_destroy(s)
    eng.close()


def test_a_fan_out_of_65_is_refused_under_the_flag_only(K, g):
    L = K.lib()
    seeds = D.seed_list("narrow")
    eng = make_engine(K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), 64, [65], seeds=dict(train=[(seeds, g["labels"][seeds])]))
    pool = eng.pools[0]
    L.GPUMemoryPool_SetSampling(pool, 1)
    L.GPUMemoryPool_SetSharedDraws(pool, 1)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, 64, 0, 0, 0, K.TRAINMODE)
    L.d_stream_sync(None)
    K.check()
    seeded = eng.result(0, with_features=False)
    L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, 65, 2, 0)
    msg = (L.legion_last_error() or b"").decode()
    assert ("GPU_Random_Sampling: shared-key sampling (GPUMemoryPool_SetSharedDraws) takes a fan-out of at most 64: k_sample keeps a row's best picks "
            "one per lane and stages them in static LDS") in msg, msg
    L.legion_clear_error()
    L.d_stream_sync(None)
    assert_batch_equal(seeded, eng.result(0, with_features=False), keys=KEYS_NO_FEATURES)     # no hop ran
    assert int(seeded["ec"].sum()) == 0
    L.GPUMemoryPool_SetSampling(pool, 0)                                   # the flag is remembered and acts only at kind 1: 65 runs
    assert L.GPUMemoryPool_GetSharedDraws(pool) == 1
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, 64, 0, 0, 0, K.TRAINMODE)
    L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, 65, 2, 0)
    L.d_stream_sync(None)
    K.check()
    assert int(eng.result(0, with_features=False)["ec"].sum()) > 0
    eng.close()


# ---------------------------------------------------------------------------------------------------
# composition
# ---------------------------------------------------------------------------------------------------
def test_aggregated_hand_offs_on_top(K, synth):
    """The plain and the normalised aggregated hand-off over the statement's draws (tests/aggref.py and tests/gcnref.py through
    distinctcases.expected_sums), bit for bit."""
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    B, fan = 512, [10, 5]
    lab = ds.labels[ds.train]
    want = R.Statement(ds.indptr, ds.indices, ds.features, B, fan).run_batch(ds.train, lab, 0)
    eng = make_engine(K, ds, B, fan)
    for norm in (False, True):
        eng.run_batch(0, 0, agg_last_hop=True, agg_norm="both" if norm else None, per_level=norm, **SD)
        got = eng.result(0)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        n_in, N, S, d = expected_sums(want, fan, norm)
        assert N > 0 and got["features"].shape[0] == n_in
        assert_bits("features", got["features"], want["features"][:n_in])
        assert_bits("nbr_sum", got["nbr_sum"], S)
        if norm:
            assert np.array_equal(got["out_deg"], d)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# served: the `legion` binary under LEGION_SAMPLING=distinct LEGION_SHARED_DRAWS=1 LEGION_SAMPLING_SEED=7
# ---------------------------------------------------------------------------------------------------
class ByRound:
    """The statement behind harness.replay_served, which asks for (ids, labels, local, mode, batch size) in the order of the trainer's
    records: the round of record b is b // (training + validation steps)."""

    def __init__(self, st, got, steps):
        self.st, self.rounds = st, iter([rec["b"] // (steps[0] + steps[1]) for rec in got["batches"]])

    def run_batch(self, ids, lab, counter, mode=0, batch_size=None):
        return self.st.run_batch(ids, lab, counter, mode=mode, batch_size=batch_size, round=next(self.rounds))


def test_server_binary_serves_shared_key_batches(tmp_path, synth, oracle):
    workload, scale, B, epochs, fan, S = "products", 0.004, 96, 2, [10, 5], 7
    spec = synth.spec_for(workload, scale=scale)
    ds = synth.generate(spec)
    n_valid, n_test = min(700, spec.n_valid), min(300, spec.n_test)
    meta_line = "synth:%s:%r %d %d %d %d %d %d %d %d %d 0" % (workload, scale, B, spec.V, ds.E, spec.F, spec.n_train, n_valid, n_test, 1 << 40, epochs)
    env = dict(LEGION_SAMPLING="distinct", LEGION_SHARED_DRAWS="1", LEGION_SAMPLING_SEED=S)
    with served(tmp_path, meta_line, fan, env=env) as srv:
        got, = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    text = srv.log_text()
    assert got["sampling"] == "distinct" and got["sampling_seed"] == S       # the flag is not published: a trainer reads the kind
    assert "by a key of the neighbour node" in text and "LEGION_SHARED_DRAWS=1)" in text
    (sets,), steps, (bs,) = serve_sets(oracle, ds, B, n_valid=n_valid, n_test=n_test)
    st = ByRound(R.Statement(ds.indptr, ds.indices, ds.features, B, fan, seed=S), got, steps)
    assert got["hops"] == len(fan) and steps[0] >= 3 and steps[1] > 0 and steps[2] > 0
    for rec, ref, mode, local in replay_served(got, st, sets, ds.labels, steps, epochs, bs):
        assert_served_record(rec, ref, len(fan))
