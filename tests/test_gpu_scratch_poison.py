"""A batch must not depend on what the pool's scratch held.  Every buffer GPUMemoryPool_ScratchInfo lists as dead -- between batches, and
for the hop-lifetime ones between the ops of a batch -- the position table and the engine's own output buffers are filled with wrong
but safe values (tests/scratchpoison.py), and every batch is then compared word for word with the oracle or the rule's NumPy statement,
never with an unpoisoned run of the library.  Features are included.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import scratchpoison as P
import wsharedcases
from aggref import expected_nbr_sum, last_hop_runs
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import random_graph
from gcnref import expected_nbr_sum_norm
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

TILE_OF = dict(narrow=P.TILE_NARROW, wide=P.TILE_WIDE)


# ---- driving a batch op by op, as capi.Engine.run_batch does, with a hook between the ops ------------------------------------------
def drive(K, eng, counter, batch_size=None, dev=0, pipe=0, per_level=True, hook=None, agg_last_hop=False, agg_norm=None, sample="replace",
          weighted_distinct=False, shared_draws=False):
    """hook("sampled", h): behind the seed launch (h = 0) and behind hop h; hook("gather", l): in front of every gather op"""
    L, pool, H = K.lib(), eng.pools[dev], eng.hops
    agg, norm = eng._set_modes(dev, agg_last_hop, agg_norm, sample, None, 0, None, weighted_distinct=weighted_distinct, shared_draws=shared_draws)
    eng._agg[(dev, pipe)], eng._norm[(dev, pipe)] = agg, norm
    hook = hook or (lambda kind, n: None)
    L.GPUMemoryPool_SetCurrentPipe(pool, pipe)
    L.GPUMemoryPool_SetCurrentMode(pool, K.TRAINMODE)
    L.GPUMemoryPool_SetIter(pool, counter)
    L.batch_generator_kernel(None, eng.noder, eng.cache, pool, eng.batch_size if batch_size is None else batch_size, counter, dev, dev, K.TRAINMODE)
    hook("sampled", 0)
    if per_level:
        hook("gather", 0)
        L.get_feature_kernel(None, eng.cache, eng.noder, pool, dev, 1, 1)
    for h in range(1, H + 1):
        L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, int(eng.fanout[h - 1]), 2 * h, 0)
        hook("sampled", h)
        if per_level and not (agg and h == H):
            hook("gather", h)
            L.get_feature_kernel(None, eng.cache, eng.noder, pool, dev, 2 * h + 1, 1)
    if agg:
        hook("gather", H)
        L.get_feature_kernel_agg(None, eng.cache, eng.noder, pool, dev, 1)
    elif not per_level:
        hook("gather", H)
        L.get_feature_kernel_all(None, eng.cache, eng.noder, pool, dev, 1)
    L.make_update_plan(None, eng.graph, eng.cache, pool, dev, K.TRAINMODE)
    L.update_cache(None, eng.cache, eng.noder, pool, dev, K.TRAINMODE)
    L.d_stream_sync(None)
    K.check()


def hop_slots(want, fan):
    """the slots of the batch's largest hop, from its counters"""
    n, out = int(want["nc"][4]), 1
    for h, f in enumerate(fan, 1):
        out = max(out, n * int(f))
        n = int(want["ec"][2 + h]) - (int(want["ec"][1 + h]) if h > 1 else 0)
    return out


def poison_all(K, eng, rng, fill, want, fan, tile, decoy, dev=0, pipes=(0,), cache_slots=1, stream=None):
    """in front of a batch: every hop- and batch-lifetime buffer, the table, and the output buffers of the pipes"""
    kw = dict(avoid=want["ids"], decoy=decoy, slots=hop_slots(want, fan), tile=tile, cache_slots=cache_slots)
    done = P.poison_pool(K, eng, rng, fill, dev=dev, pipes=pipes, stream=stream, **kw)
    for q in pipes:
        P.poison_outputs(K, eng, rng, fill, dev=dev, pipe=q, stream=stream, avoid=want["ids"])
    return done


def between_ops(K, eng, rng, fill, want, fan, tile, decoy, dev=0, cache_slots=1):
    """the hook of drive(): behind sampler op h the hop-lifetime buffers and the slot states that op consumed (aux2[h & 1]: the launcher
    gives hop h that buffer and has it prepare the other), in front of a gather op the gather's own scratch"""
    kw = dict(avoid=want["ids"], decoy=decoy, slots=hop_slots(want, fan), tile=tile, cache_slots=cache_slots, dev=dev)

    def hook(kind, n):
        if kind == "sampled":
            P.poison_pool(K, eng, rng, fill, lifetimes=("hop",), **kw)
            P.poison_pool(K, eng, rng, fill, lifetimes=("batch",), names=("aux2[%d]" % (n & 1),), **kw)
        else:
            P.poison_pool(K, eng, rng, fill, lifetimes=("batch",), names=P.GATHER_SCRATCH, **kw)
    return hook


# ---- the engines and statements of (a), (b), (d): one pool per tile, shared, so that the rules follow each other on it too ----------
@pytest.fixture(scope="module")
def g():
    return wsharedcases.rule_graph()


class Shared:
    def __init__(self, K, g, oracle):
        self.K, self.g, self.oracle, self.eng, self.decoys, self.want, self.st = K, g, oracle, {}, {}, {}, {}

    def engine(self, tile):
        if tile not in self.eng:
            B, fan = P.SHAPES[tile]
            seeds, g = P.seed_list(tile), self.g
            V, F = len(g["indptr"]) - 1, g["feats"].shape[1]
            self.eng[tile] = make_engine(self.K, (V, F, g["indptr"], g["indices"], g["feats"]), B, fan, seeds=dict(train=[(seeds, g["labels"][seeds])]),
                                         edge_weights=g["w"], retain_edge_weights=True, pipeline_depth=2)
            self.decoys[tile] = P.Decoy(self.K, V, F)
        return self.eng[tile], self.decoys[tile]

    def statement(self, rule, tile, counter, bs):
        """computed once per batch and shared by the tests that compare it; a weighted rule without replacement: no near tie (the cap is zero)"""
        key = (rule, tile, counter, bs)
        if key not in self.want:
            if (rule, tile) not in self.st:
                alias = self.engine(tile)[0].alias_rows(0) if rule == "weighted" else None      # the table the device built: any valid table is a statement
                self.st[(rule, tile)] = P.statement(rule, self.g, tile, alias=alias, oracle=self.oracle)
            st, seeds = self.st[(rule, tile)], P.seed_list(tile)
            self.want[key] = st.run_batch(seeds, self.g["labels"][seeds], counter, batch_size=bs)
            assert getattr(st, "ties", []) == []
        return self.want[key]

    def close(self):
        for e in self.eng.values():
            e.close()
        for d in self.decoys.values():
            d.free()


@pytest.fixture(scope="module")
def shared(K, g, oracle):
    s = Shared(K, g, oracle)
    yield s
    s.close()


def assert_listed(done):
    """every buffer of the pool that a batch of this mode could read was poisoned: nothing was silently left out of the list"""
    missing = {t[0] for t in P.EXPECTED_TABLE if t[3] != "state" and not t[4]} - set(done)
    assert not missing, missing


def test_the_poison_is_on_the_device(K, shared):
    """what the helper generated is what every listed buffer, both pipes' mode buffers included, holds afterwards: read back word for word"""
    eng, decoy = shared.engine("narrow")
    fan = P.SHAPES["narrow"][1]
    want = shared.statement("replace", "narrow", 0, None)
    drive(K, eng, 0, agg_last_hop=True, agg_norm="both")               # the per-pipe buffers of both aggregated modes exist from here on
    for fill in P.FILLS:
        written = []
        kw = dict(avoid=want["ids"], decoy=decoy, slots=hop_slots(want, fan), tile=P.TILE_NARROW)
        done = P.poison_pool(K, eng, np.random.RandomState(1), fill, pipes=(0, 1), written=written, **kw)
        assert sorted(done) == sorted([t[0] for t in P.EXPECTED_TABLE if t[3] != "state"] + [t[0] for t in P.EXPECTED_TABLE if t[4]])
        for name, ptr, a in written:
            assert np.array_equal(K.read_dev(ptr, np.uint8, a.nbytes), np.frombuffer(a.tobytes(), np.uint8)), (fill, name)
        assert len({ptr for _, ptr, _ in written}) == len(written)    # no buffer twice: each pipe's own


# ---- a. between batches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", list(P.SHAPES))
@pytest.mark.parametrize("rule", P.RULES)
def test_between_batches(K, shared, rule, tile):
    """A full batch, one seed, a seed without neighbours (every later hop is k_write's n_tiles == 0 path), the full batch again and the
    short last batch on one pool, a different fill in front of each."""
    eng, decoy = shared.engine(tile)
    fan = P.SHAPES[tile][1]
    rng = np.random.RandomState(P.RULES.index(rule) * 2 + (tile == "wide"))
    for n, (counter, bs, fill) in enumerate(P.SEQUENCE):
        want = shared.statement(rule, tile, counter, bs)
        assert_listed(poison_all(K, eng, rng, fill, want, fan, TILE_OF[tile], decoy, pipes=(0, 1)))
        drive(K, eng, counter, batch_size=bs, per_level=bool(n & 1), **P.ENGINE_ARGS[rule])
        assert_batch_equal(want, eng.result(0))
    empty = shared.statement(rule, tile, 0, 1)
    assert int(empty["nc"][4]) == 1 and int(empty["ec"][2 + len(fan)]) == 0          # the seed of degree 0: no edge in any hop


def dense_graph(V, lo, hi):
    """every row but node 0 has lo..hi neighbours and no holes: every slot draws, so the batch fills its static bound; node 0 has none"""
    rng = np.random.RandomState(3)
    deg = rng.randint(lo, hi + 1, size=V)
    deg[0] = 0
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    return indptr, rng.randint(1, V, size=int(indptr[-1])).astype(np.int32), rng.randint(0, 7, size=V).astype(np.int32)


def test_between_batches_with_several_tiles_per_chunk(K, oracle):
    """The reference's draws at a bound where a k_mark workgroup runs T > 1 tiles (launch_sample_hop_t: at most 4 workgroups per compute
    unit and kMaxChunks = 2048 of them, 1024 slots each), so tile_pre holds in-chunk prefixes that are not zero."""
    cus = K.lib().legion_sampler_cu_count()
    fan, V, F = [25, 20], 2000, 4
    B = (4 * cus * 1024) // (fan[0] * fan[1]) + 100
    grid = min(4 * cus, 2048)
    tiles = (B * fan[0] * fan[1] + 1023) // 1024
    assert B * fan[0] * fan[1] > P.NARROW_SLOTS and (tiles + grid - 1) // grid > 1                   # T > 1 from the bound and the CU count
    indptr, indices, labels = dense_graph(V, 25, 60)
    feats = np.random.RandomState(1).rand(V, F).astype(np.float32)
    seeds = np.concatenate([[0, 1], np.random.RandomState(2).randint(1, V, size=B + B // 3 - 2)]).astype(np.int32)
    lab = labels[seeds]
    orc = oracle.OracleRunner(indptr, indices, feats, V, F, B, fan)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(seeds, lab)]))
    decoy = P.Decoy(K, V, F)
    rng = np.random.RandomState(77)
    for n, (counter, bs, fill) in enumerate(P.SEQUENCE):
        want = orc.run_batch(seeds, lab, counter, batch_size=bs)
        if n == 0:
            assert ((hop_slots(want, fan) + 1023) // 1024 + grid - 1) // grid > 1                  # ... and from the batch that ran
        assert_listed(poison_all(K, eng, rng, fill, want, fan, P.TILE_WIDE, decoy))
        drive(K, eng, counter, batch_size=bs, per_level=bool(n & 1))
        assert_batch_equal(want, eng.result(0))
    decoy.free()
    eng.close()


# ---- b. between ops -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", list(P.SHAPES))
@pytest.mark.parametrize("rule", ["replace", "wshared"])
def test_between_ops(K, shared, rule, tile):
    """The same sequence with the hop-lifetime buffers (and the slot states an op consumed) poisoned again behind every sampler op, and
    the gather's scratch in front of every gather op."""
    eng, decoy = shared.engine(tile)
    fan = P.SHAPES[tile][1]
    rng = np.random.RandomState(100 + P.RULES.index(rule) * 2 + (tile == "wide"))
    for n, (counter, bs, fill) in enumerate(P.SEQUENCE):
        want = shared.statement(rule, tile, counter, bs)
        poison_all(K, eng, rng, fill, want, fan, TILE_OF[tile], decoy)
        drive(K, eng, counter, batch_size=bs, per_level=not (n & 1), hook=between_ops(K, eng, rng, P.FILLS[(n + 1) % 3], want, fan, TILE_OF[tile], decoy),
              **P.ENGINE_ARGS[rule])
        assert_batch_equal(want, eng.result(0))


# ---- d. aggregated hand-offs ----------------------------------------------------------------------------------------------------------
def assert_bits(name, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d words differ, first at %s: %r vs %r" % (name, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def assert_sums(ref, got, g, fan, norm):
    """the aggregated batch `got` against the default-mode statement's batch: aggref's sums, or gcnref's with the block's out-degrees"""
    assert_batch_equal(ref, got, keys=KEYS_NO_FEATURES)
    if norm:
        n_in, N, _, S, d = expected_nbr_sum_norm(ref, g["indptr"], g["indices"], fan)
        assert np.array_equal(got["out_deg"], d)
    else:
        n_in, N, _, S = expected_nbr_sum(ref, g["indptr"], g["indices"], fan)
    assert_bits("features", got["features"], np.asarray(ref["features"])[:n_in])
    assert_bits("nbr_sum", got["nbr_sum"], S)
    cnt = last_hop_runs(ref, g["indptr"], g["indices"], fan)[3]
    assert not got["nbr_sum"][cnt == 0].view(np.uint32).any()          # a run without draws is a stored row of +0.0
    return cnt


@pytest.mark.parametrize("tile", list(P.SHAPES))
@pytest.mark.parametrize("norm", [False, True], ids=["sums", "normalised"])
def test_aggregated_hand_offs(K, shared, g, norm, tile):
    """cand_pipe, agg_out_deg, agg_wdraw and agg_chunk_cnt of both pipes poisoned with everything else in front of every batch; the
    batches alternate between the pipes."""
    eng, decoy = shared.engine(tile)
    fan = P.SHAPES[tile][1]
    rng = np.random.RandomState(200 + 2 * norm + (tile == "wide"))
    empty_runs = 0
    for n, (counter, bs, fill) in enumerate(P.SEQUENCE + P.SEQUENCE[:1]):
        want = shared.statement("replace", tile, counter, bs)
        q = n & 1
        done = poison_all(K, eng, rng, fill, want, fan, TILE_OF[tile], decoy, pipes=(0, 1))
        if n:                                                          # the modes' buffers exist from the first aggregated batch on
            assert {"cand_pipe"} | ({"agg_out_deg", "agg_wdraw", "agg_chunk_cnt"} if norm else set()) <= set(done)
        drive(K, eng, counter, batch_size=bs, pipe=q, per_level=bool(n & 2), agg_last_hop=True, agg_norm="both" if norm else None)
        empty_runs += int((assert_sums(want, eng.result(0, pipe=q), g, fan, norm) == 0).sum())
    assert empty_runs > 0


# ---- e. batch graphs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["replace", "distinct"])
def test_recorded_batches_replayed_over_poison(K, oracle, g, rule):
    """One recorded batch per pipe, replayed for the iterations 0..3 (the last one short) with everything poisoned between the replays"""
    B, fan = P.SHAPES["narrow"]
    V, F = len(g["indptr"]) - 1, g["feats"].shape[1]
    seeds = np.concatenate([np.arange(5), np.random.RandomState(4).randint(0, V, size=3 * B + B // 3 - 5)]).astype(np.int32)
    lab = g["labels"][seeds]
    st = P.statement(rule, g, "narrow", oracle=oracle)
    eng = make_engine(K, (V, F, g["indptr"], g["indices"], g["feats"]), B, fan, seeds=dict(train=[(seeds, lab)]), pipeline_depth=2)
    K.lib().GPUCache_SetPreSc(eng.cache, 0)
    decoy = P.Decoy(K, V, F)
    graphs = [eng.capture_batch(0, pipe=q, per_level=(q == 0), **P.ENGINE_ARGS[rule]) for q in (0, 1)]
    rng = np.random.RandomState(300 + (rule == "distinct"))
    for q in (0, 1):
        for it in range(4):
            want = st.run_batch(seeds, lab, it)
            poison_all(K, eng, rng, P.FILLS[(it + q) % 3], want, fan, P.TILE_NARROW, decoy, pipes=(0, 1), stream=graphs[q][1])     # the stream the graph replays on
            eng.run_graph(graphs[q], it)
            assert_batch_equal(want, eng.result(0, pipe=q))
    assert int(want["nc"][4]) == B // 3                                # the last one was the short batch
    decoy.free()
    eng.close()


# ---- c. / f. the cached clique ----------------------------------------------------------------------------------------------------------
def build_clique(K, oracle, V, F, indptr, indices, feats, labels, B, fan, parts, cap_n, cap_e, steps=2):
    """A G = 2 clique with forced capacities, the way test_randomised_clique_cache_differential builds it, and the oracle's runners with
    the same caches: pre-sampling batches on both, the oracle's ranking, its id -> slot maps and fragments."""
    G = 2
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, G=G, seeds=dict(train=[(p, labels[p]) for p in parts]), train_step=steps)
    orcs = [oracle.OracleRunner(indptr, indices, feats, V, F, B, fan, partition_count=G) for _ in range(G)]
    for d in range(G):
        for it in range(steps):
            eng.run_batch(d, it, is_presc=True)
            orcs[d].run_batch(parts[d], labels[parts[d]], it, is_presc=True)
    eng.build_cache(cache_agg_mode=1, node_capacity=cap_n, edge_capacity=cap_e, train_step=steps)
    L = K.lib()
    assert L.GPUCache_Kg(eng.cache) == G and L.GPUCache_NodeCapacity(eng.cache, 0) == cap_n and L.GPUCache_EdgeCapacity(eng.cache, 0) == cap_e
    _, QF = oracle.candidate_selection([o.node_access_time for o in orcs], V)
    _, QT = oracle.candidate_selection([o.edge_access_time for o in orcs], V)
    for o in orcs:
        o.set_feature_cache(QF, cap_n, G)
        if cap_e > 0:
            o.set_topo_cache(QT, cap_e, G, 0)
    return eng, orcs


def hit_counters(K, eng, dev):
    n_hit, n_rows = C.c_int32(0), C.c_int32(0)
    K.lib().GPUCache_FeatureCacheHitRate(eng.cache, dev, C.byref(n_hit), C.byref(n_rows))
    return n_hit.value, n_rows.value


@pytest.mark.parametrize("peers", ["in-kernel", "exchange"])
@pytest.mark.parametrize("lookup", ["pass", "fused"])
def test_caches_and_lookups(K, oracle, g, monkeypatch, lookup, peers):
    """Feature shards in several chunks and CSR fragments; FindFeat as its own pass (every batch hit-sampled) or inside the gather; the
    peers' rows by in-kernel loads or through the exchange.  The sequence on both members; the pass still counts the oracle's hits."""
    monkeypatch.setenv("LEGION_SHARD_CHUNK_BYTES", "20000")
    for name, on, val in (("LEGION_CACHE_HIT_PERIOD", lookup == "pass", "1"), ("LEGION_PEER_GATHER", peers == "exchange", "exchange")):
        monkeypatch.setenv(name, val) if on else monkeypatch.delenv(name, raising=False)
    B, fan = P.SHAPES["narrow"]
    V, F = len(g["indptr"]) - 1, g["feats"].shape[1]
    parts = [P.seed_list("narrow"), np.concatenate([np.arange(5), np.random.RandomState(9).randint(0, V, size=B + B // 3 - 5)]).astype(np.int32)]
    cap_n, cap_e = V // 6, V // 8
    eng, orcs = build_clique(K, oracle, V, F, g["indptr"], g["indices"], g["feats"], g["labels"], B, fan, parts, cap_n, cap_e)
    assert K.lib().GPUCache_ShardChunkCount(eng.cache, 0) > 1
    decoys = []
    for d in (0, 1):
        K.lib().SetGPUDevice(d)
        decoys.append(P.Decoy(K, V, F))
    rng = np.random.RandomState(400 + 2 * (lookup == "pass") + (peers == "exchange"))
    for d in (0, 1):
        for n, (counter, bs, fill) in enumerate(P.SEQUENCE):
            want = orcs[d].run_batch(parts[d], g["labels"][parts[d]], counter, batch_size=bs)
            poison_all(K, eng, rng, fill, want, fan, P.TILE_NARROW, decoys[d], dev=d, cache_slots=2 * cap_n)
            drive(K, eng, counter, batch_size=bs, dev=d, per_level=bool(n & 1))
            got = eng.result(d)
            assert_batch_equal(want, got)
            if lookup == "pass" and peers == "in-kernel":
                hit = orcs[d].node_map[got["ids"][got["ids"] >= 0]] >= 0
                assert hit_counters(K, eng, d) == (int(hit.sum()), len(got["ids"]))
        slot = orcs[d].node_map[got["ids"]]
        assert ((slot >= 0) & (slot // cap_n != d)).any() and (slot < 0).any()       # peer rows and misses were gathered
    for d in (0, 1):
        K.lib().SetGPUDevice(d)
        decoys[d].free()
    eng.close()


# ---- f. undersized grids ----------------------------------------------------------------------------------------------------------------
def est_rows(hint, bound):
    """csrc/launch.h"""
    return min(bound, hint + hint // 4 + 1024) if hint > 0 else bound


@pytest.mark.parametrize("F", [4, 7, 100])
def test_undersized_grids(K, oracle, monkeypatch, F):
    """A batch of one seed sizes the next launch of every gather-like kernel (est_rows: the hint + 25 % + 1024), then a full batch of at
    least eight times that many rows runs on those grids, then one seed again on the full batch's: the uncached gather, the lookup pass,
    the fused lookup, the exchange plan at G = 2 and k_gather_sum (its runs), every one through get_feature_kernel_all / _agg."""
    V, B, fan = 40000, 1024, [5, 4, 3]
    indptr, indices, labels = random_graph(11, V, holes=True)
    feats = np.random.RandomState(F).standard_normal((V, F)).astype(np.float32)
    hub = int(np.argmax(np.diff(indptr)))
    rs = np.random.RandomState(12)
    parts = [np.concatenate([[hub], rs.permutation(V)[:B + B // 3]]).astype(np.int32) for _ in range(2)]
    bound = B * (1 + 5 + 20 + 60)
    order = ((0, 1), (0, None), (0, 1))                                # one seed (the hub), the full batch, one seed
    plain = oracle.OracleRunner(indptr, indices, feats, V, F, B, fan)
    small, full = (plain.run_batch(parts[0], labels[parts[0]], c, batch_size=bs) for c, bs in order[:2])
    rows = lambda w: int(w["nc"][0])                                   # what get_feature_kernel_all gathers
    runs = lambda w: int(w["ec"][2 + 2] - w["ec"][2 + 1])              # hop 2's edges = the last hop's input slots: what k_gather_sum walks
    assert rows(full) >= 8 * est_rows(rows(small), bound) and runs(full) >= 8 * est_rows(runs(small), B * 5 * 4)
    rng = np.random.RandomState(500 + F)

    def walk(eng, refs, devs, name, **kw):
        decoy = {}
        for d in devs:
            K.lib().SetGPUDevice(d)
            decoy[d] = P.Decoy(K, V, K.lib().legion_row_pitch(F))
            for n, (c, bs) in enumerate(order):
                want = refs[d].run_batch(parts[d], labels[parts[d]], c, batch_size=bs)
                poison_all(K, eng, rng, P.FILLS[n], want, fan, P.TILE_NARROW, decoy[d], dev=d, cache_slots=kw.get("cache_slots", 1))
                drive(K, eng, c, batch_size=bs, dev=d, per_level=False, agg_last_hop=name == "sums")
                if name == "sums":
                    n_in, N, _, S = expected_nbr_sum(want, indptr, indices, fan)
                    got = eng.result(d)
                    assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
                    assert_bits("features", got["features"], want["features"][:n_in])
                    assert_bits("nbr_sum", got["nbr_sum"], S)
                else:
                    assert_batch_equal(want, eng.result(d))
            K.lib().SetGPUDevice(d)
            decoy[d].free()

    for name in ("LEGION_CACHE_HIT_PERIOD", "LEGION_PEER_GATHER"):
        monkeypatch.delenv(name, raising=False)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(parts[0], labels[parts[0]])]))
    walk(eng, [plain], (0,), "uncached")
    walk(eng, [plain], (0,), "sums")
    eng.close()
    cap_n = V // 5
    eng, orcs = build_clique(K, oracle, V, F, indptr, indices, feats, labels, B, fan, parts, cap_n, 0)
    walk(eng, orcs, (0,), "fused", cache_slots=2 * cap_n)              # (the first batch behind the cache build is hit-sampled: the pass)
    monkeypatch.setenv("LEGION_CACHE_HIT_PERIOD", "1")
    walk(eng, orcs, (1,), "pass", cache_slots=2 * cap_n)
    monkeypatch.delenv("LEGION_CACHE_HIT_PERIOD")
    monkeypatch.setenv("LEGION_PEER_GATHER", "exchange")
    walk(eng, orcs, (0, 1), "exchange", cache_slots=2 * cap_n)
    eng.close()
