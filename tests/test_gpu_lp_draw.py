"""Drawn link-prediction thirds on the GPU (GPUMemoryPool_SetLpDraw / LEGION_LP_DRAW: k_seed<.., LP>, k_shuffle_triples), through the C ABI
and served, against the NumPy statement of tests/lpref.py.  Every batch check is array_equal on nc, ec, ids, labels, both COO arrays and
the feature rows.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import lpref as P
from aggref import expected_nbr_sum
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import random_graph
from gcnref import expected_nbr_sum_norm
from harness import K, OUT, assert_served_record, make_engine, serve_sets, served  # noqa: F401  (K: the module-scoped library fixture)
from seededref import W

pytestmark = pytest.mark.gpu

S_GRID = (0, 1, 12345, 0xFFFFFFFF)
R_GRID = (0, 1, 7)
C_GRID = (0, 1, 40)
DEG_GRID = (-1, 0, 1, 2, 7, 2 ** 31 - 1)
V_GRID = (1, 2, 500, 2 ** 31 - 1)


def assert_bits(name, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %d words differ" % (name, int((a != b).sum()))


def probe(K, S, r, c, src, deg, V):
    L = K.lib()
    n = len(src)
    bufs = [K.DevBuf.from_numpy(np.ascontiguousarray(x, dtype=np.int32)) for x in (src, deg)] + [K.DevBuf(n * 4), K.DevBuf(n * 4)]
    L.legion_lp_draw_probe(None, S, r, c, bufs[0].ptr, bufs[1].ptr, V, bufs[2].ptr, bufs[3].ptr, n)
    L.d_stream_sync(None)
    K.check()
    got = bufs[2].to_numpy(np.int32, n), bufs[3].to_numpy(np.int32, n)
    for b in bufs:
        b.free()
    return got


# ---------------------------------------------------------------------------------------------------
# 1. the probe: the seed kernel's device functions against the statement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", S_GRID)
def test_probe_matches_the_statement(K, S):
    n = 3000
    rng = np.random.RandomState(S % 1000)
    src = np.concatenate([[0, 0, 5], rng.randint(0, 2 ** 31 - 1, size=n - 3)]).astype(np.int64)
    deg = np.concatenate([[1000, 1000, 1], np.resize(np.array(DEG_GRID), 600), rng.randint(1, 5000, size=n - 1603), rng.randint(1, 2 ** 31 - 1, size=1000)]).astype(np.int64)
    src[21], deg[21], src[2666], deg[2666] = 499, 7, 111059955, 2 ** 31 - 1
    for a, r in enumerate(R_GRID):
        for b, c in enumerate(C_GRID):
            for V in (V_GRID[(a + b) % 4], V_GRID[(a + b + 2) % 4]):
                rho, neg = probe(K, S, r, c, src, deg, V)
                w = W(S, r, c)
                assert np.array_equal(rho, P.rho(w, np.arange(n), src, deg)), (S, r, c)
                assert np.array_equal(neg, P.neg(w, np.arange(n), src, V)), (S, r, c, V)
                assert ((neg >= 0) & (neg < V)).all() and (rho[deg <= 0] == -1).all() and (rho[deg > 0] < deg[deg > 0]).all()
    if S == 12345:      # the known answers of INTEGRATION.md
        rho, neg = probe(K, 12345, 3, 2, src, deg, 500)
        assert rho[[0, 1, 21, 2666]].tolist() == [121, 995, 5, 1052666731] and neg[[0, 1]].tolist() == [153, 453]
        assert int(probe(K, 12345, 3, 2, src, deg, 111059956)[1][21]) == 52733101 and int(probe(K, 12345, 3, 2, src, deg, 2 ** 31 - 1)[1][2666]) == 393912042
        assert [int(x[0]) for x in probe(K, 12345, 3, 2, [5], [1], 1)] == [0, 0]
    if S == 0:
        assert [int(x[0]) for x in probe(K, 0, 0, 0, [0], [10], 10)] == [4, 7]


# ---------------------------------------------------------------------------------------------------
# 2. - 3. whole batches through the C ABI
# ---------------------------------------------------------------------------------------------------
def toy(k, batches=5, holes=True):
    V, F = 500, 6
    indptr, indices, _ = random_graph(1, V, holes=holes)
    feats = np.random.RandomState(1).rand(V, F).astype(np.float32)
    L = P.toy_list(indptr, V, k, batches)
    Lab = (np.arange(len(L)) % 1000).astype(np.int32)        # a label per list entry
    return V, F, indptr, indices, feats, L, Lab


@pytest.mark.parametrize("sample", ["replace", "distinct"])
@pytest.mark.parametrize("fan", [[1], [25, 10], [5, 4, 3]], ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("k", [22, 171])
def test_toy_graph_batches(K, k, fan, sample):
    """V = 500 with holes, empty rows and hubs, one repeated source; 5 batches of 3 k, the last one padded (T = 110 at k = 22: the
    permutation cycle-walks); rounds 0, 1, 7; first, middle and last batch, and the batch that holds the empty-row source; per-level and
    single gathers; both sampler modes."""
    S = 12345
    V, F, indptr, indices, feats, Ls, Lab = toy(k)
    B = 3 * k
    st = P.Statement(indptr, indices, feats, B, fan, S, sample)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(Ls, Lab)]))
    empty = int(np.nonzero(np.diff(indptr) == 0)[0][0])
    seen, pos_is_src = [], 0
    for rnd in R_GRID:
        ids, _ = st.drawn(Ls, Lab, rnd)
        where = [c for c in range(5) if empty in ids[c * B:c * B + k]]
        for counter in sorted(set([0, 2, 4] + where[:1])):
            eng.run_batch(0, counter, sample=sample, per_level=bool((counter + rnd) & 1), seed=S, round=rnd, lp_draw=k)
            want = st.run_batch(Ls, Lab, counter, round=rnd)
            got = eng.result(0)
            assert_batch_equal(want, got)
            assert (got["labels"][k:] == -1).all() and (got["labels"][:k] >= 0).all()
            src, pos = got["ids"][:k], got["ids"][k:2 * k]
            pos_is_src += int(((src == empty) & (pos == empty)).sum())
            seen.append(tuple(got["ids"][:B].tolist()))
    assert len(set(seen)) == len(seen)          # every (round, counter) is another batch
    assert pos_is_src >= len(R_GRID)            # the empty-row source draws itself
    assert K.lib().GPUMemoryPool_GetLpDraw(eng.pools[0]) == k
    eng.close()


def test_file_order_keeps_the_src_thirds_and_draws_afresh(K):
    """BeginRound(noder = NULL) under the mode: the src thirds are the file's, in list order; pos and neg are drawn per batch and round."""
    k, fan, S = 22, [5, 4, 3], 777
    V, F, indptr, indices, feats, Ls, Lab = toy(k)
    B = 3 * k
    L = K.lib()
    st = P.Statement(indptr, indices, feats, B, fan, S, shuffle=False)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(Ls, Lab)]))
    drawn = {}
    for rnd in (0, 1):
        eng.run_batch(0, 0, seed=S, round=rnd, lp_draw=k)                        # the engine begins the round with the list: shuffled
        assert L.GPUMemoryPool_BeginRound(None, eng.pools[0], None, 0, rnd) == 0
        for counter in (0, 3, 4):
            eng.run_batch(0, counter, seed=S, round=rnd, lp_draw=k)
            got = eng.result(0)
            assert_batch_equal(st.run_batch(Ls, Lab, counter, round=rnd), got)
            assert np.array_equal(got["ids"][:k], Ls[counter * B:counter * B + k]) and np.array_equal(got["labels"][:k], Lab[counter * B:counter * B + k])
            drawn[(rnd, counter)] = got["ids"][k:B].tolist()
        eng._seed_state.pop(0, None)                                            # the next round begins through the engine again
    assert len(set(map(tuple, drawn.values()))) == len(drawn)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 4. captured graphs
# ---------------------------------------------------------------------------------------------------
def test_batch_graph_replays_across_rounds_and_seeds(K):
    """One recording: counters 0..4, two rounds and another seed without re-recording equal the statement; a graph recorded in the other
    lp_draw state is refused by name, both ways round."""
    k, fan, S = 171, [5, 4, 3], 4242
    V, F, indptr, indices, feats, Ls, Lab = toy(k)
    B = 3 * k
    L = K.lib()
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(Ls, Lab)]))
    L.GPUCache_SetPreSc(eng.cache, 0)
    st = P.Statement(indptr, indices, feats, B, fan, S)
    g = eng.capture_batch(0, seed=S, round=0, lp_draw=k)
    for rnd in (0, 1):
        for counter in range(5):
            eng.run_graph(g, counter, round=rnd)
            assert_batch_equal(st.run_batch(Ls, Lab, counter, round=rnd), eng.result(0))
    eng.run_graph(g, 3, round=0)                  # out of order: the cursor is reset
    assert_batch_equal(st.run_batch(Ls, Lab, 3, round=0), eng.result(0))
    eng.run_graph(g, 1, seed=S + 1, round=2)
    assert_batch_equal(P.Statement(indptr, indices, feats, B, fan, S + 1).run_batch(Ls, Lab, 1, round=2), eng.result(0))
    eng.run_batch(0, 1, seed=S + 1, round=2, lp_draw=k)                          # host-driven: the same batch
    assert_batch_equal(P.Statement(indptr, indices, feats, B, fan, S + 1).run_batch(Ls, Lab, 1, round=2), eng.result(0))
    off = eng.capture_batch(0, seed=S, round=0)                                 # seeded, the mode off
    with pytest.raises(RuntimeError, match="LegionBatchGraph_Launch: the graph was recorded with drawn link-prediction thirds"):
        eng.run_graph(g, 0)
    with pytest.raises(RuntimeError, match="LegionBatchGraph_Launch: the graph was recorded without drawn link-prediction thirds"):
        eng.run_graph(off, 0, lp_draw=k)
    L.legion_clear_error()
    eng.run_graph(g, 2)
    assert_batch_equal(st.run_batch(Ls, Lab, 2, round=0), eng.result(0))
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 5. the positives' rows behind a topology cache
# ---------------------------------------------------------------------------------------------------
def test_positives_come_from_fragments_and_from_the_whole_csr(K, synth, small_ds, monkeypatch):
    """A clique of Kg = 2 logical GPUs on one device with a filled topology cache: the batches of both GPUs equal the uncached statement;
    on either GPU src rows are served from the peer's fragment, from the own one and from the whole CSR (the fragments hold the
    hottest eighth of the rows: the sources of the pre-sampled batches, not those of a later round)."""
    monkeypatch.setenv("LEGION_SHARD_CHUNK_BYTES", str(1 << 20))
    ds = small_ds
    V, F = ds.spec.V, ds.spec.F
    L = K.lib()
    k, fan, G, S = 100, [10, 5], 2, 777
    B = 3 * k
    lists = [synth.lp_trainingset(ds, 800, B, rank=g, world=G) for g in range(G)]
    labs = [ds.labels[l] for l in lists]
    assert all(len(l) >= 3 * B and len(l) % B == 0 for l in lists)
    eng = make_engine(K, ds, B, fan, G=G, seeds=dict(train=list(zip(lists, labs))), cache_memory=int(V * F * 4 * 0.15), train_step=2)
    st = P.Statement(ds.indptr, ds.indices, ds.features, B, fan, S)
    for g in range(G):
        for it in range(2):
            eng.run_batch(g, it, is_presc=True, seed=S, round=0, lp_draw=k)
            assert_batch_equal(st.run_batch(lists[g], labs[g], it), eng.result(g, with_features=False), keys=KEYS_NO_FEATURES)
    cap = V // 16
    eng.build_cache(cache_agg_mode=1, node_capacity=V // 8, edge_capacity=cap, train_step=2)
    assert L.GPUCache_Kg(eng.cache) == G and L.GPUCache_EdgeCapacity(eng.cache, 0) == cap
    L.SetGPUDevice(0)
    QT = K.read_dev(L.GPUCache_GetQT(eng.cache, 0), np.int32, V)
    owner = np.full(V, -1, np.int64)
    owner[QT[:G * cap]] = np.arange(G * cap) % G
    for g in range(G):
        L.SetGPUDevice(g)
        assert L.GPUGraphStorage_FragmentRows(eng.graph, g) == cap
        served_by = []
        for it, rnd, sample in ((0, 0, "replace"), (1, 1, "replace"), (2, 1, "distinct")):
            eng.run_batch(g, it, sample=sample, per_level=(it != 1), seed=S, round=rnd, lp_draw=k)
            want = P.Statement(ds.indptr, ds.indices, ds.features, B, fan, S, sample).run_batch(lists[g], labs[g], it, round=rnd)
            assert_batch_equal(want, eng.result(g))
            served_by.append(owner[want["ids"][:k]])
        o = np.concatenate(served_by)
        print("GPU %d: src rows from the peer's fragment %d, the own %d, the whole CSR %d" % (g, (o == 1 - g).sum(), (o == g).sum(), (o < 0).sum()))
        assert (o == 1 - g).any() and (o == g).any() and (o < 0).any()
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 6. the aggregated hand-offs on top
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan", [[7], [10, 5]], ids=lambda f: "H%d" % len(f))
def test_aggregated_hand_offs_on_top(K, fan):
    """Neighbour sums and normalised sums of a drawn batch: bit for bit aggref / gcnref fed with the statement's batch.  The duplicate
    seeds of a triple batch keep one run per slot.  (The graph has no holes: aggref recomputes the draws of a graph with holes from the
    unseeded stream.)"""
    k, S = 171, 31337
    V, F, indptr, indices, feats, Ls, Lab = toy(k, holes=False)
    B = 3 * k
    st = P.Statement(indptr, indices, feats, B, fan, S)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(Ls, Lab)]))
    for it, rnd in ((0, 0), (3, 2)):
        want = st.run_batch(Ls, Lab, it, round=rnd)
        assert len(np.unique(want["ids"][:B])) < B
        eng.run_batch(0, it, agg_last_hop=True, per_level=(it == 0), seed=S, round=rnd, lp_draw=k)
        got = eng.result(0)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        n_in, N, run_dst, Ssum = expected_nbr_sum(want, indptr, indices, fan)
        assert N > 0 and got["features"].shape[0] == n_in and (len(fan) > 1 or N == B)
        assert_bits("features", got["features"], want["features"][:n_in])
        assert_bits("nbr_sum", got["nbr_sum"], Ssum)
        eng.run_batch(0, it, agg_last_hop=True, agg_norm="both", per_level=(it != 0), seed=S, round=rnd, lp_draw=k)
        got = eng.result(0)
        assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
        n_in, N, run_dst, Sw, d = expected_nbr_sum_norm(want, indptr, indices, fan)
        assert np.array_equal(got["out_deg"], d)
        assert_bits("nbr_sum (normalised)", got["nbr_sum"], Sw)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 7. the mode off
# ---------------------------------------------------------------------------------------------------
def test_mode_off_is_untouched(K, oracle):
    """Between two drawn batches an unseeded run_batch on the same engine gives the oracle's batch bit for bit: all three thirds from the
    file."""
    k, fan, S = 171, [10, 5, 3], 9
    V, F, indptr, indices, feats, Ls, Lab = toy(k)
    B = 3 * k
    orc = oracle.OracleRunner(indptr, indices, feats, V, F, B, fan)
    st = P.Statement(indptr, indices, feats, B, fan, S)
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(Ls, Lab)]))
    for it in (0, 4):
        eng.run_batch(0, it, seed=S, round=1, lp_draw=k)
        drawn = eng.result(0)
        assert_batch_equal(st.run_batch(Ls, Lab, it, round=1), drawn)
        eng.run_batch(0, it)
        assert K.lib().GPUMemoryPool_GetLpDraw(eng.pools[0]) == 0
        ref = orc.run_batch(Ls, Lab, it)
        assert_batch_equal(ref, eng.result(0))
        assert np.array_equal(ref["ids"][:B], Ls[it * B:(it + 1) * B]) and not np.array_equal(ref["ids"][:B], drawn["ids"][:B])
        eng.run_batch(0, it, sample="distinct", seed=S, round=2, lp_draw=k)
        assert_batch_equal(P.Statement(indptr, indices, feats, B, fan, S, "distinct").run_batch(Ls, Lab, it, round=2), eng.result(0))
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals(K):
    """B != 3 k, a list that is no multiple of 3 k (batch_generator_kernel and BeginRound), no seed, a switch while capturing: each once,
    by name, and the pool's modes unchanged; the engine stays usable."""
    k, fan, S = 22, [5, 3], 9
    V, F, indptr, indices, feats, Ls, Lab = toy(k)
    B = 3 * k
    L = K.lib()
    eng = make_engine(K, (V, F, indptr, indices, feats), B, fan, seeds=dict(train=[(Ls, Lab)]))
    pool = eng.pools[0]
    L.GPUCache_SetPreSc(eng.cache, 0)

    def refused(words, fn):
        L.legion_clear_error()
        before = (L.GPUMemoryPool_GetLpDraw(pool), L.GPUMemoryPool_GetSampleSeed(pool, None), L.GPUMemoryPool_GetSampleDistinct(pool))
        fn()
        msg = (L.legion_last_error() or b"").decode()
        assert all(msg.count(w) == 1 for w in words), (words, msg)
        L.legion_clear_error()
        assert before == (L.GPUMemoryPool_GetLpDraw(pool), L.GPUMemoryPool_GetSampleSeed(pool, None), L.GPUMemoryPool_GetSampleDistinct(pool))

    gen = lambda bs: L.batch_generator_kernel(None, eng.noder, eng.cache, pool, bs, 0, 0, 0, K.TRAINMODE)  # noqa: E731
    eng.run_batch(0, 0, seed=S, round=0, lp_draw=k)
    refused(("batch_generator_kernel", "GPUMemoryPool_SetLpDraw", "the batch size must be three times"), lambda: gen(B - 3))
    L.GPUMemoryPool_SetLpDraw(pool, 20, eng.graph)                                 # 5 batches of 66 seeds: 330 is no multiple of 3 * 20
    refused(("GPUMemoryPool_BeginRound", "GPUMemoryPool_SetLpDraw", "not a multiple of the batch of 3 k"), lambda: L.GPUMemoryPool_BeginRound(None, pool, eng.noder, 0, 0))
    assert L.GPUMemoryPool_BeginRound(None, pool, None, 0, 0) == 0                 # file order: nothing to shuffle, the generator looks itself
    refused(("batch_generator_kernel", "GPUMemoryPool_SetLpDraw", "not a multiple of the batch of 3 k"), lambda: gen(60))
    L.GPUMemoryPool_SetLpDraw(pool, k, eng.graph)
    assert L.GPUMemoryPool_BeginRound(None, pool, eng.noder, 0, 0) == 0
    L.GPUMemoryPool_SetSampleSeed(pool, 0, 0)
    refused(("batch_generator_kernel", "GPUMemoryPool_SetSampleSeed", "GPUMemoryPool_SetLpDraw"), lambda: gen(B))
    L.GPUMemoryPool_SetSampleSeed(pool, 1, S)
    eng._seed_state.pop(0, None)
    refused(("batch_generator_kernel", "GPUMemoryPool_BeginRound"), lambda: gen(B))             # the existing rule, unchanged
    eng.run_batch(0, 1, seed=S, round=0, lp_draw=k)
    st = L.d_stream_create()
    assert L.GPUMemoryPool_BeginBatchCapture(pool, st) == 0
    refused(("GPUMemoryPool_SetLpDraw: the pool is being captured",), lambda: L.GPUMemoryPool_SetLpDraw(pool, 0, None))
    refused(("GPUMemoryPool_SetLpDraw: the pool is being captured",), lambda: L.GPUMemoryPool_SetLpDraw(pool, 5, eng.graph))
    eng.run_batch(0, 0, stream=st, sync=False, seed=S, round=0, lp_draw=k)
    g = L.GPUMemoryPool_EndBatchCapture(pool, st)
    K.check()
    assert g and L.GPUMemoryPool_GetLpDraw(pool) == k
    eng._graphs.append(g)
    eng.run_batch(0, 2, seed=S, round=0, lp_draw=k)
    assert_batch_equal(P.Statement(indptr, indices, feats, B, fan, S).run_batch(Ls, Lab, 2), eng.result(0))
    eng.close()
    L.d_stream_destroy(st)


# ---------------------------------------------------------------------------------------------------
# 9. served: the `legion` binary with LEGION_LP_DRAW=1
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,G", [("0", 1), ("1", 1), ("0", 2)])
def test_server_binary_serves_drawn_thirds(tmp_path, synth, oracle, graph, G):
    """synth:products:0.004, B = 510, meta flag 2, two epochs: every record equals the statement's batch of (mode, local, round); the src
    thirds are GPU g's (src % G == g); the two epochs' training batches differ; the mode is logged once per GPU in place of the
    "served verbatim" line."""
    import oracle as O
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    B, fan, epochs, S = 510, [10, 5], 2, 12345
    k, H = B // 3, len(fan)
    meta_line = "synth:products:0.004 %d %d %d %d %d 100 60 0 %d 2" % (B, spec.V, ds.E, spec.F, spec.n_train, epochs)
    with served(tmp_path, meta_line, fan, G=G, env=dict(LEGION_SAMPLING_SEED=S, LEGION_LP_DRAW=1, LEGION_BATCH_GRAPH=graph)) as srv:
        gots = srv.run_clients("ipc_client_modes.py", ["plain", spec.F, epochs, OUT])
        srv.finish()
    text = srv.log_text()
    assert text.count("Drawn link-prediction thirds: %d triples per batch (LEGION_LP_DRAW=1)" % k) == G and "served verbatim" not in text
    assert "Feature buffer too small" not in text
    lists = [synth.lp_trainingset(ds, len(ds.train), B, rank=g, world=G) for g in range(G)]
    sets, steps, bs = serve_sets(oracle, ds, B, G, train=lists, n_valid=100, n_test=60)
    assert steps[0] >= 2
    for g, got in enumerate(gots):
        assert got["sampling_seed"] == S and len(got["batches"]) == O.max_step(steps, epochs)
        st = P.Statement(ds.indptr, ds.indices, ds.features, B, fan, S)
        train = {}
        for rec in got["batches"]:
            mode, local = O.schedule(steps, epochs, rec["b"])
            rnd = rec["b"] // (steps[0] + steps[1])
            ids = sets[g][mode]
            ref = st.run_batch(ids, ds.labels[ids], local, mode=mode, batch_size=bs[g][mode], round=rnd)
            assert_served_record(rec, ref, H)
            if mode == 0:
                src = np.asarray(rec["seeds"][:k])
                assert len(rec["seeds"]) == B and (src % G == g).all()
                train[(rnd, local)] = rec
        locals_ = sorted(c for r, c in train if r == 0)
        assert len(locals_) >= 2
        for local in locals_:
            assert train[(0, local)]["seeds"] != train[(1, local)]["seeds"] and train[(0, local)]["ids"] != train[(1, local)]["ids"]
