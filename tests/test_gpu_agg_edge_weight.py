"""The edge-weighted last hop on the GPU (GPUMemoryPool_SetAggEdgeWeight: k_draw_edge_weights in front of k_gather_sum<.., WT>, INTEGRATION.md
"Edge-weighted sums") against the NumPy statement of tests/edgeaggref.py over the batches of tests/eidref.py.  Sums are compared by bit
pattern; the rest of the batch is the edge-id mode's.  Shapes and graph: tests/drawrulecases.py.  Run with `pytest -m gpu`.

How many chunks of the slot -> edge prefix a shape spans (launch_agg_norm_weights' grid rule, which launch_agg_edge_weights shares: one
workgroup per 256 slots of the hop's static bound, at most 8 per compute unit and kMaxChunks = 2048; a chunk is the slot count over the
grid, rounded up to 256):
  narrow  64 x [5, 4]: the last hop's bound is 64 x 5 runs x 4 = 1 280 slots -> 5 chunks of 256
  wide    4 097 x [64]: 262 208 slots -> 1 025 workgroups (below 8 x 256 compute units), chunks of 256, the last one of 64 slots"""
import ctypes as C
import ctypes.util
import types

import numpy as np
import pytest

import drawrulecases as D
import eidref as R
import scratchpoison as P
from aggcases import assert_sum_bits
from conftest import assert_batch_equal
from edgeaggref import expected_nbr_sum_edge
from eidref import assert_edge_ids, bits
from harness import K, in_process_runner, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

SEED = 7
K_BLOCK, K_MAX_CHUNKS, WGS_PER_CU = 256, 2048, 8            # kBlock, kMaxChunks (csrc/internal.h), grid_for's default (csrc/launch.h)
WDRAW_BUFFERS = ("cand_pipe", "agg_wdraw", "agg_chunk_cnt")
ON = dict(agg_last_hop=True, edge_ids=True, agg_edge_weight=True)
PLAIN = dict(agg_last_hop=True, edge_ids=True)
EVERYTHING_ELSE = ("nc", "ec", "ids", "labels", "src_off", "dst_off", "features", "edge_ids")


def chunks_of(tile, cus):
    B, fan = D.SHAPES[tile]
    slots = B * int(np.prod(fan))                          # level_bound[H - 1] * fan-out of the last hop
    return min(K_MAX_CHUNKS, -(-slots // K_BLOCK), cus * WGS_PER_CU)


def test_the_shapes_span_several_chunks():
    assert [chunks_of(t, 256) for t in ("narrow", "wide")] == [5, 1025]


@pytest.fixture(scope="module")
def g():
    return D.graph()


class Engines:
    """The engines of this module, built on first use and closed with it (tests/test_gpu_edge_ids.py builds them the same way): whole(tile) one
    logical GPU over the whole CSR, clique(tile) two logical GPUs behind a filled cache with CSR fragments.  Both retain the weights."""

    def __init__(self, K, g):
        self.K, self.g, self.made, self.want = K, g, {}, {}

    def _engine(self, tile, G, **kw):
        B, fan = D.SHAPES[tile]
        seeds = D.seed_list(tile)
        g = self.g
        return make_engine(self.K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, fan, G=G, seeds=dict(train=[(seeds, g["labels"][seeds])] * G),
                           edge_weights=g["w"], retain_edge_weights=True, cache_memory=int(D.V * D.F * 4 * 0.15), train_step=2, **kw)

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
            assert L.GPUCache_Kg(eng.cache) == 2 and all(L.GPUGraphStorage_FragmentRows(eng.graph, dev) == D.V // 3 for dev in range(2))
        return self.made[("clique", tile)]

    def statement(self, rule, tile, counter, seed=None, round=0):
        """(the eidref batch, (n_in, N, run_dst, S_e)): computed once per batch and shared, never changed"""
        key = (rule, tile, counter, seed, round)
        if key not in self.want:
            B, fan = D.SHAPES[tile]
            seeds = D.seed_list(tile)
            ties = []
            ref = R.run_batch(self.g, rule, seeds, self.g["labels"][seeds], B, counter, fan, seed=seed, round=round, ties=ties)
            assert ties == []               # the cap on near-tie rows is zero (test_draw_rules_cpu.py, test_weighted_shared_cpu.py, test_edge_ids_cpu.py)
            self.want[key] = (ref, expected_nbr_sum_edge(ref, self.g["indptr"], self.g["indices"], fan))
        return self.want[key]

    def close(self):
        for eng in self.made.values():
            eng.close()


@pytest.fixture(scope="module")
def engines(K, g):
    e = Engines(K, g)
    yield e
    e.close()


def assert_edge_weighted(name, want, got):
    """the engine's batch `got` against (the eidref batch, its S_e): the batch and its edge ids word for word, the weights and the rows of the
    levels < H by bit pattern, and the sums by bit pattern -- only a NaN of the statement accepts any NaN (aggcases.assert_sum_bits)"""
    ref, (n_in, N, _, S) = want
    assert_edge_ids(ref, got)
    assert got["features"].shape == (n_in, ref["features"].shape[1]) and np.array_equal(bits(got["features"]), bits(ref["features"][:n_in])), name
    assert got["nbr_sum"].shape == S.shape and N > 0, (name, got["nbr_sum"].shape, S.shape)
    assert_sum_bits(name, got["nbr_sum"], S)


COMBOS = [(r, t) for t in D.SHAPES for r in R.RULES]


@pytest.mark.parametrize("rule,tile", COMBOS, ids=["%s-%s" % c for c in COMBOS])
def test_sums_equal_the_statement_on_the_whole_csr(K, engines, rule, tile):
    """both tiles, the first and the (short) last batch, every rule that hands ids over: nbr_sum has the bits of S_e"""
    eng = engines.whole(tile)
    for it in D.COUNTERS:
        eng.run_batch(0, it, **ON, **R.ENGINE_ARGS[rule])
        assert K.lib().GPUMemoryPool_GetAggEdgeWeight(eng.pools[0]) == 1
        want = engines.statement(rule, tile, it)
        assert not np.isnan(want[1][3]).any() and (want[0]["edge_w"] == 0).any() == (rule in ("stream", "distinct", "shared"))
        assert_edge_weighted("%s %s %d" % (rule, tile, it), want, eng.result(0))


@pytest.mark.parametrize("rule", R.PARTITIONED_RULES)
def test_sums_equal_the_statement_on_the_clique(K, engines, rule):
    """two logical GPUs behind a filled cache: the rows come from the shards and the backing table, the draws from fragment rows, the weights
    from the whole CSR"""
    eng = engines.clique("narrow")
    for it in D.COUNTERS:
        eng.run_batch(0, it, **ON, **R.ENGINE_ARGS[rule])
        assert_edge_weighted("%s clique %d" % (rule, it), engines.statement(rule, "narrow", it), eng.result(0))


@pytest.mark.parametrize("rule", ["stream", "distinct", "wshared"])
def test_seeded_batches(K, engines, rule):
    """seed 7, rounds 0 and 1: the sums are the statement's under the batch's draw word, over the round's shuffled list"""
    eng = engines.whole("narrow")
    for rnd in (0, 1):
        for it in D.COUNTERS:
            eng.run_batch(0, it, seed=SEED, round=rnd, **ON, **R.ENGINE_ARGS[rule])
            assert_edge_weighted("%s seeded %d %d" % (rule, rnd, it), engines.statement(rule, "narrow", it, seed=SEED, round=rnd), eng.result(0))


@pytest.mark.parametrize("rule", ["stream", "wdistinct"])
def test_nothing_else_moves(K, g, rule):
    """with the flag on against the plain aggregated batch with edge ids, everything except nbr_sum is array-equal; and a pool whose flag was
    never set, and one whose flag was switched off again, hand over the same plain batch and hold what they held"""
    L = K.lib()
    B, fan = D.SHAPES["narrow"]
    seeds = D.seed_list("narrow")
    eng = make_engine(K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), B, fan, seeds=dict(train=[(seeds, g["labels"][seeds])]),
                      edge_weights=g["w"], retain_edge_weights=True)
    try:
        eng.run_batch(0, 0, **PLAIN, **R.ENGINE_ARGS[rule])
        before = eng.result(0)
        listed = {b["name"]: b for b in K.pool_scratch(eng.pools[0], 0)}
        assert listed["cand_pipe"]["ptr"] and not listed["agg_wdraw"]["ptr"] and not listed["agg_chunk_cnt"]["ptr"] and not listed["agg_out_deg"]["ptr"]
        eng.run_batch(0, 0, **ON, **R.ENGINE_ARGS[rule])
        on = eng.result(0)
        listed = {b["name"]: b for b in K.pool_scratch(eng.pools[0], 0)}
        assert listed["agg_wdraw"]["ptr"] and listed["agg_chunk_cnt"]["ptr"] and not listed["agg_out_deg"]["ptr"]      # the degrees are the norm's
        assert_batch_equal(before, on, keys=EVERYTHING_ELSE)
        assert np.array_equal(bits(before["edge_w"]), bits(on["edge_w"])) and np.array_equal(bits(before["features"]), bits(on["features"]))
        assert on["nbr_sum"].shape == before["nbr_sum"].shape and not np.array_equal(bits(on["nbr_sum"]), bits(before["nbr_sum"]))
        eng.run_batch(0, 0, **PLAIN, **R.ENGINE_ARGS[rule])
        after = eng.result(0)
        assert L.GPUMemoryPool_GetAggEdgeWeight(eng.pools[0]) == 0
        assert_batch_equal(before, after, keys=EVERYTHING_ELSE)
        assert np.array_equal(bits(before["nbr_sum"]), bits(after["nbr_sum"])) and np.array_equal(bits(before["edge_w"]), bits(after["edge_w"]))
    finally:
        L.legion_clear_error()
        eng.close()


# ---- adversarial numerics on a hand-made graph --------------------------------------------------------------
ADV_W = np.array([0.0, 1.0, 0.5, 2.0 ** -24, 3e38], np.float32)
ADV_X = np.array([1.5, 1e-40, -1e-40, 1.2e-38, -2e-38, 3e38, -3e38, 2.0, np.inf, -np.inf, np.nan, 0.0, -0.0, -7.25, 2.0 ** -126, 3.0 ** -20], np.float32)


ADV_V, ADV_FULL = 32, 26


def adversarial_graph(F):
    """32 rows.  Row r < 26 sees nodes r, r + 1, .. r + 4 (mod 26) under the weights 0, 1, 0.5, 2^-24, 3e38 in this order, so each of those nodes
    meets every weight; rows 26 .. 31 see two nodes under 0.5 and 2^-24, so that a subnormal product survives into a sum.  Element (n, c) of
    the table is special value (3 n + 5 c) mod 16 -- subnormals, values whose product with 0.5 or 2^-24 goes subnormal, values that overflow
    under 3e38 or inside a run, both infinities, NaN and both zeros in every column"""
    V, f = ADV_V, 5
    deg = np.array([f] * ADV_FULL + [2] * (V - ADV_FULL))
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    full = ((np.arange(ADV_FULL)[:, None] + np.arange(f)[None, :]) % ADV_FULL).astype(np.int32).reshape(-1)
    short = np.stack([3 * np.arange(V - ADV_FULL) + 1, 5 * np.arange(V - ADV_FULL) + 2], 1).astype(np.int32).reshape(-1)
    indices = np.concatenate([full, short])
    w = np.concatenate([np.tile(ADV_W, ADV_FULL), np.tile(ADV_W[2:4], V - ADV_FULL)])
    n, c = np.meshgrid(np.arange(V), np.arange(F), indexing="ij")
    feats = ADV_X[(3 * n + 5 * c) % len(ADV_X)]
    assert len(set(map(tuple, np.stack([full, bits(w[:len(full)])], 1).tolist()))) == ADV_FULL * f            # every (node, weight) pair once
    return dict(indptr=indptr, indices=indices, w=w, feats=np.ascontiguousarray(feats, np.float32), labels=np.zeros(V, np.int32))


@pytest.mark.parametrize("rule", ["stream", "distinct"])
@pytest.mark.parametrize("F", [3, 8])
def test_adversarial_numerics(K, F, rule):
    """F = 3 takes the scalar path, F = 8 the 16-byte one.  Bits are compared; only the payload and sign of a RESULT NaN are left open"""
    a = adversarial_graph(F)
    V, fan = ADV_V, [5]
    seeds = np.arange(V, dtype=np.int32)
    ref = R.run_batch(a, rule, seeds, a["labels"], V, 0, fan)
    want = (ref, expected_nbr_sum_edge(ref, a["indptr"], a["indices"], fan))
    S = want[1][3]
    sub = lambda v: ((bits(v) & 0x7F800000) == 0) & ((bits(v) & 0x007FFFFF) != 0)
    assert np.isnan(S).any() and np.isinf(S).any() and sub(S).any() and (~np.isnan(S)).mean() > 0.3 and not (bits(S) == 0x80000000).any()
    eng = make_engine(K, (V, F, a["indptr"], a["indices"], a["feats"]), V, fan, seeds=dict(train=[(seeds, a["labels"])]), edge_weights=a["w"], retain_edge_weights=True)
    try:
        eng.run_batch(0, 0, **ON, **R.ENGINE_ARGS[rule])
        got = eng.result(0)
        assert_edge_ids(ref, got)
        assert_sum_bits("adversarial F=%d %s" % (F, rule), got["nbr_sum"], S)
    finally:
        K.lib().legion_clear_error()
        eng.close()


# ---- two pipes, two streams, recorded graphs ------------------------------------------------------------------
def test_overlapped_two_stream_schedule_and_the_graphs_refusals(K, engines, g):
    """Depth 2: batch i + 1 is sampled (a recorded LegionBatchGraph per pipe) on one stream while batch i's weights and sums run on the other.
    The sampler of batch i + 1 overwrites the pool's draw buffer, columns and slot states meanwhile: the new pass reads the pipe's own draws,
    counters and edge_w.  A graph replays only in the state of the flag it was recorded in."""
    L = K.lib()
    eng = engines._engine("narrow", 1, pipeline_depth=2)
    try:
        L.GPUCache_SetPreSc(eng.cache, 0)
        pool = eng.pools[0]
        s_samp, s_gath = L.d_stream_create(), L.d_stream_create()
        ev_sampled, ev_gathered = [L.d_event_create(), L.d_event_create()], [L.d_event_create(), L.d_event_create()]
        used = [False, False]
        graphs = [eng.capture_batch(0, gather=False, pipe=q, stream=s_samp, sample="distinct", **ON) for q in (0, 1)]
        assert L.GPUMemoryPool_GetAggEdgeWeight(pool) == 1 and L.GPUMemoryPool_GetEdgeIds(pool) == 1

        def enqueue(i, counter):
            q = i % 2
            L.GPUMemoryPool_SetCurrentPipe(pool, q)
            L.GPUMemoryPool_SetCurrentMode(pool, K.TRAINMODE)
            if used[q]:
                L.d_stream_wait_event(s_samp, ev_gathered[q])
            eng.run_graph(graphs[q], counter, sync=False)
            L.d_event_record(ev_sampled[q], s_samp)
            L.d_stream_wait_event(s_gath, ev_sampled[q])
            L.get_feature_kernel_agg(s_gath, eng.cache, eng.noder, pool, 0, 1)
            L.d_event_record(ev_gathered[q], s_gath)
            used[q] = True

        counters = [0, 1, 1, 0, 1, 0]
        enqueue(0, counters[0])
        for i, it in enumerate(counters):
            if i + 1 < len(counters):
                enqueue(i + 1, counters[i + 1])          # batch i + 1 is sampled while batch i is still being summed
            L.d_stream_sync(s_samp)
            L.d_stream_sync(s_gath)
            K.check()
            assert_edge_weighted("overlapped %d" % i, engines.statement("distinct", "narrow", it), eng.result(0, pipe=i % 2, aggregated=True, edge_ids=True))
        whole = eng.capture_batch(0, pipe=0, stream=s_samp, sample="distinct", **ON)         # and the whole batch, sums included, as one graph
        for it in D.COUNTERS:
            eng.run_graph(whole, it)
            assert_edge_weighted("one graph %d" % it, engines.statement("distinct", "narrow", it), eng.result(0, pipe=0))
        L.GPUMemoryPool_SetAggEdgeWeight(pool, 0)
        with pytest.raises(RuntimeError, match=r"LegionBatchGraph_Launch: the graph was recorded with edge-weighted sums \(GPUMemoryPool_SetAggEdgeWeight\) and the pool has the flag off now"):
            eng.run_graph(whole, 0)
        plain = eng.capture_batch(0, pipe=0, stream=s_samp, sample="distinct", **PLAIN)
        eng.run_graph(plain, 0)
        L.GPUMemoryPool_SetAggEdgeWeight(pool, 1)
        with pytest.raises(RuntimeError, match=r"LegionBatchGraph_Launch: the graph was recorded without edge-weighted sums and the pool has the flag on now \(GPUMemoryPool_SetAggEdgeWeight\)"):
            eng.run_graph(plain, 0)
        eng.run_graph(whole, 1)                             # back in its state: it replays
        assert_edge_weighted("one graph again", engines.statement("distinct", "narrow", 1), eng.result(0, pipe=0, aggregated=True, edge_ids=True))
    finally:
        L.legion_clear_error()
        eng.close()
        for s in (s_samp, s_gath):
            L.d_stream_destroy(s)


# ---- poisoned scratch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", list(D.SHAPES))
@pytest.mark.parametrize("fill", P.FILLS)
def test_the_result_does_not_depend_on_what_the_scratch_held(K, engines, tile, fill):
    """every hop- and batch-lifetime buffer of the pool -- the pipe's draws, agg_wdraw and the chunk counts included -- filled through
    GPUMemoryPool_ScratchInfo with wrong but safe values between two runs of one batch"""
    eng = engines.whole(tile)
    rule = "wdistinct" if tile == "narrow" else "stream"
    eng.run_batch(0, 0, **ON, **R.ENGINE_ARGS[rule])
    first = eng.result(0)
    listed = {b["name"]: b for b in K.pool_scratch(eng.pools[0], 0)}
    assert [(listed[n]["lifetime"], listed[n]["per_pipe"], listed[n]["elem_bytes"]) for n in WDRAW_BUFFERS] == [("batch", True, 4)] * 3
    done = P.poison_pool(K, eng, np.random.RandomState(5), fill, lifetimes=("hop", "batch"), avoid=first["ids"], tile=P.TILE_NARROW if tile == "narrow" else P.TILE_WIDE)
    assert set(WDRAW_BUFFERS) | {"cols", "edge_ids", "edge_w", "cand"} <= set(done) and "agg_out_deg" not in done
    eng.run_batch(0, 0, **ON, **R.ENGINE_ARGS[rule])
    again = eng.result(0)
    assert np.array_equal(bits(first["nbr_sum"]), bits(again["nbr_sum"]))
    assert_edge_weighted("poisoned %s %s" % (tile, fill), engines.statement(rule, tile, 0), again)


# ---- the in-process runner -----------------------------------------------------------------------------------------------
def test_the_in_process_runner_hands_over_the_same_rows(K, g, monkeypatch):
    """LEGION_AGG_LAST_HOP=1, and GPUMemoryPool_SetEdgeIds plus the new setter on Runner_GetMemoryPool: one batch per pipe through
    Runner_RunOnce equals the engine's -- no trainer attached, the pipes' buffers are read where the runner registered them"""
    monkeypatch.setenv("LEGION_AGG_LAST_HOP", "1")
    for var in ("LEGION_AGG_NORM", "LEGION_SAMPLING", "LEGION_SAMPLING_SEED", "LEGION_BATCH_GRAPH", "LEGION_RUNNER_GATHER", "LEGION_PEER_GATHER"):
        monkeypatch.delenv(var, raising=False)
    B, fan = D.SHAPES["narrow"]
    H = len(fan)
    # 2 B + 1 seeds, the hand-made rows first: the runner serves (n - 1) // B = 2 full training batches, one per pipe
    seeds = np.concatenate([np.arange(5), np.random.RandomState(4).randint(0, D.V, size=2 * B + 1 - 5)]).astype(np.int32)
    ds = types.SimpleNamespace(spec=types.SimpleNamespace(V=D.V, F=D.F), indptr=g["indptr"], indices=g["indices"], features=g["feats"], labels=g["labels"], train=seeds)
    want = []
    for it in (0, 1):
        ref = R.run_batch(g, "stream", seeds, g["labels"][seeds], B, it, fan)
        want.append((ref, expected_nbr_sum_edge(ref, g["indptr"], g["indices"], fan)))
    libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6", use_errno=True)
    libc.sem_open.restype = C.c_void_p
    libc.sem_open.argtypes = [C.c_char_p, C.c_int]
    libc.sem_post.argtypes = libc.sem_close.argtypes = [C.c_void_p]
    with in_process_runner(K, ds, B, fan, "ew", presc_batches=2) as r:
        L, env, runner, rp = r.L, r.env, r.runner, r.rp
        assert L.IPCEnv_GetAggLastHop(env) == 1
        L.GPUGraphStorage_RetainEdgeWeights(r.eng.graph, 1)
        r.eng.set_edge_weights(g["w"])
        pool = L.Runner_GetMemoryPool(runner)
        L.GPUMemoryPool_SetEdgeIds(pool, 1)
        L.GPUMemoryPool_SetAggEdgeWeight(pool, 1)
        K.check()
        assert L.GPUMemoryPool_GetAggLastHop(pool) == 1 and L.GPUMemoryPool_GetAggEdgeWeight(pool) == 1
        sems = [libc.sem_open(("/%ssem_r_0_%d" % (r.ns, q)).encode(), 0) for q in (0, 1)]
        assert all(sems)
        for q in (0, 1):
            libc.sem_post(sems[q])                         # the trainer's "pipe q is free"
        for b in (0, 1):                                   # batch b is queued and batch b - 1, once complete, handed over
            rp.global_batch_id = b
            L.Runner_RunOnce(runner, C.byref(rp))
            K.check()
        libc.sem_post(sems[1])                             # Runner_Finalize waits for batch 1, hands it over and then for the pipe behind the current one
        L.Runner_Finalize(runner, C.byref(rp))
        K.check()
        for s in sems:
            libc.sem_close(s)
        for q, (ref, (n_in, N, _, S)) in enumerate(want):
            nc = K.read_dev(L.IPCEnv_GetNodeCounter(env, 0, q), np.int32, len(ref["nc"]))
            ec = K.read_dev(L.IPCEnv_GetEdgeCounter(env, 0, q), np.int32, len(ref["ec"]))
            assert np.array_equal(nc, ref["nc"]) and np.array_equal(ec, ref["ec"]), q
            E = int(ec[2 + H])
            assert np.array_equal(K.read_dev(L.IPCEnv_GetAggSrc(env, 0, q), np.int32, E), ref["src_off"])
            rows = K.read_dev(L.IPCEnv_GetFloatFeatures(env, 0, q), np.float32, (n_in + N) * D.F).reshape(n_in + N, D.F)
            assert np.array_equal(bits(rows[:n_in]), bits(ref["features"][:n_in])), q
            assert_sum_bits("runner pipe %d" % q, rows[n_in:], S)


# ---- refusals on the GPU: argument errors caught on the host, nothing launched behind them ---------------------------------------
def test_refusals_launch_nothing(K, g):
    L = K.lib()
    B, fan = D.SHAPES["narrow"]
    seeds = D.seed_list("narrow")
    arrays = (D.V, D.F, g["indptr"], g["indices"], g["feats"])

    def checks():
        c = (C.c_int64 * 4)()
        L.legion_audit_counts(c)
        return c[0]

    def refused(text, fn):
        L.d_stream_sync(None)
        L.legion_clear_error()
        before = checks()
        fn()
        msg = (L.legion_last_error() or b"").decode()
        assert text in msg, (text, msg)
        assert checks() == before                           # every launch is an audited one: none was made
        L.legion_clear_error()

    bare = make_engine(K, arrays, B, fan, seeds=dict(train=[(seeds, g["labels"][seeds])]), edge_weights=g["w"])      # weights, not retained
    try:
        pool = bare.pools[0]
        agg = lambda: L.get_feature_kernel_agg(None, bare.cache, bare.noder, pool, 0, 1)      # noqa: E731
        bare.run_batch(0, 0, gather=False, **ON)            # the setters accept: what the graph retains shows per batch
        assert L.GPUMemoryPool_GetAggEdgeWeight(pool) == 1 and not L.GPUMemoryPool_GetEdgeWeightBuffer(pool)
        refused("get_feature_kernel_agg: edge-weighted sums (GPUMemoryPool_SetAggEdgeWeight) over a batch without edge weights: the graph does not retain its weights "
                "(GPUGraphStorage_RetainEdgeWeights", agg)
    finally:
        L.legion_clear_error()
        bare.close()
    eng = make_engine(K, arrays, B, fan, seeds=dict(train=[(seeds, g["labels"][seeds])]), edge_weights=g["w"], retain_edge_weights=True)
    try:
        pool = eng.pools[0]
        agg = lambda: L.get_feature_kernel_agg(None, eng.cache, eng.noder, pool, 0, 1)        # noqa: E731
        eng.run_batch(0, 0, **ON)
        L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
        refused("get_feature_kernel_agg: called before the last hop's GPU_Random_Sampling", agg)
        L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, fan[0], 2, 0)
        refused("get_feature_kernel_agg: called before the last hop's GPU_Random_Sampling", agg)
        L.batch_generator_kernel(None, eng.noder, eng.cache, pool, B, 0, 0, 0, K.TRAINMODE)
        for h in range(len(fan)):
            L.GPU_Random_Sampling(None, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 1)     # a pre-sampling batch
        refused("get_feature_kernel_agg: a pre-sampling batch gathers nothing", agg)
        with pytest.raises(ValueError, match="agg_edge_weight needs agg_last_hop=True, edge_ids=True"):
            eng.run_batch(0, 0, agg_last_hop=True, agg_edge_weight=True)
        with pytest.raises(ValueError, match="agg_edge_weight and agg_norm together"):
            eng.run_batch(0, 0, agg_norm="both", **ON)
        want_ref = R.run_batch(g, "stream", seeds, g["labels"][seeds], B, 1, fan)
        eng.run_batch(0, 1, **ON)                            # and the engine still hands over the expected batch
        assert_edge_weighted("after the refusals", (want_ref, expected_nbr_sum_edge(want_ref, g["indptr"], g["indices"], fan)), eng.result(0))
    finally:
        L.legion_clear_error()
        eng.close()
