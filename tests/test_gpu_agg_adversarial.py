"""Adversarial numerics and a randomised differential for the aggregated hand-off (k_gather_sum, k_agg_norm_prep, k_block_out_deg,
k_draw_weights, get_feature_kernel_agg with and without GPUMemoryPool_SetAggNorm), through the C ABI, against the CPU oracle's DEFAULT-mode
batch and the NumPy statements of tests/aggref.py and tests/gcnref.py.  Run with `pytest -m gpu`.

The rules, for every batch of every test here (check_batch):
  * nc, ec, ids, labels and both COO arrays: word for word (conftest.KEYS_NO_FEATURES);
  * feature rows -- all n rows in the default mode, rows [0, n_in) in both aggregated modes -- are COPIES: uint32 equality with table[ids];
  * out_deg (normalised mode): equal to np.bincount over the batch's src_off;
  * the sums: aggcases.assert_sum_bits.  Where the statement is NaN the GPU's value must be a NaN -- payload and sign of a RESULT NaN are not
    part of the contract (IEEE 754 leaves them open, and x86 and the GPU choose differently) -- and everywhere else the uint32 words are equal,
    signs of zero and of infinity included.  Before the GPU's sums are looked at, the statement alone must pass aggcases.statement_caps: at
    most 5 % of its elements NaN, no -0.0 word.
tests/test_agg_numerics_cpu.py proves on the CPU that these inputs hold every class of special result and tell every mutant of
aggcases.MUTANTS from the statement."""
import os

import numpy as np
import pytest

import aggcases as A
from aggref import expected_nbr_sum
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from gcnref import expected_nbr_sum_norm
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

MODES = dict(default={}, plain=dict(agg_last_hop=True), norm=dict(agg_last_hop=True, agg_norm="both"))


def padded(L, table):
    """(what the engine gets, features_pitch): rows at the 128-byte-aligned pitch with poison in the pad floats, which must never reach a
    row or a sum; (the table itself, 0) where the dense rows already are whole lines"""
    V, F = table.shape
    pitch = L.legion_row_pitch(F)
    if pitch == F:
        return table, 0
    wide = np.full((V, pitch), np.float32(-777.0))
    wide[:, :F] = table
    return wide.reshape(-1), pitch


def check_batch(name, mode, ref, got, table, indptr, indices, fan, sums=True):
    """One batch of `mode` against the oracle's default-mode batch `ref` under the module's rules.  sums=False: everything but the sums
    (a table the NaN cap cannot hold on).  Returns (n_in, N, d) in the aggregated modes."""
    assert_batch_equal(ref, got, keys=KEYS_NO_FEATURES)
    assert (ref["ids"] >= 0).all()
    x = table[ref["ids"]]
    if mode == "default":
        assert "nbr_sum" not in got and "out_deg" not in got
        A.assert_words_equal(name + ": features", got["features"], x)
        return None
    with np.errstate(all="ignore"):
        if mode == "norm":
            n_in, N, _, S, d = expected_nbr_sum_norm(ref, indptr, indices, fan, x=x)
        else:
            (n_in, N, _, S), d = expected_nbr_sum(ref, indptr, indices, fan, x=x), None
    if sums:
        A.statement_caps(name, S)                   # on the statement alone
    assert got["features"].shape == (n_in, table.shape[1]) and got["nbr_sum"].shape == S.shape, (name, got["features"].shape, got["nbr_sum"].shape)
    A.assert_words_equal(name + ": features", got["features"], x[:n_in])
    if mode == "norm":
        assert got["out_deg"].dtype == np.int32 and np.array_equal(got["out_deg"], d), name + ": out_deg"
    else:
        assert "out_deg" not in got
    if sums:
        A.assert_sum_bits(name + ": nbr_sum", got["nbr_sum"], S)
    return n_in, N, d


# ---------------------------------------------------------------------------------------------------
# 1. special values through the sums
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan", A.CASE_FANS, ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("F", [8, 128, 7, 36])
def test_special_values_through_the_sums(K, oracle, F, fan):
    """The adversarial table -- wide-range normals, subnormals, +-3e38 rows that overflow inside a run, +-inf, quiet and signalling NaNs,
    -0.0 rows -- through the plain and the normalised sums: F = 8 and 128 on the 16-byte path, F = 7 (scalar path) and 36 at the padded pitch
    with poison in the pad; H = 1, 2, 3 with last fan-outs 3, 10, 25; two full batches and the short last one.  These are the batches
    tests/test_agg_numerics_cpu.py::test_class_coverage_and_caps counts the result classes of."""
    L = K.lib()
    c = A.adversarial_case(A.CASE_V, F, A.CASE_SEED, n_seeds=A.CASE_SEEDS)
    seeds, lab = c["seeds"], c["labels"][c["seeds"]]
    feats, pitch = padded(L, c["table"]) if F in (7, 36) else (c["table"], 0)          # 8 and 128: dense rows
    assert (pitch > F) == (F in (7, 36))
    orc = oracle.OracleRunner(c["indptr"], c["indices"], c["table"], c["V"], F, A.CASE_B, fan)
    eng = make_engine(K, (c["V"], F, c["indptr"], c["indices"], feats), A.CASE_B, fan, seeds=dict(train=[(seeds, lab)]), features_pitch=pitch)
    for it in A.CASE_BATCHES:
        ref = orc.run_batch(seeds, lab, it)
        for mode in ("plain", "norm"):
            eng.run_batch(0, it, per_level=(it != 1), **MODES[mode])
            n_in, N, d = check_batch("batch %d %s" % (it, mode), mode, ref, eng.result(0), c["table"], c["indptr"], c["indices"], fan)
            assert N > 0 and n_in > 0
    assert int(ref["nc"][4]) == A.CASE_SEEDS - 2 * A.CASE_B         # the last one was the short batch
    eng.run_batch(0, 0)                                             # and the default mode behind them: its rows, NaN payloads included
    check_batch("default", "default", orc.run_batch(seeds, lab, 0), eng.result(0), c["table"], c["indptr"], c["indices"], fan)
    eng.close()


@pytest.mark.parametrize("source", ["pinned_host", "cache"])
def test_special_values_from_the_host_table_and_the_cache(K, oracle, source):
    """The same table read from pinned host memory, and through a Kg = 1 cache built from a pre-sampling epoch: the sums then add rows of
    the cache (hits) and of the backing table (misses)."""
    L = K.lib()
    F, fan = 8, [4, 10]
    c = A.adversarial_case(A.CASE_V, F, A.CASE_SEED, n_seeds=A.CASE_SEEDS)
    V, seeds, lab = c["V"], c["seeds"], c["labels"][c["seeds"]]
    orc = oracle.OracleRunner(c["indptr"], c["indices"], c["table"], V, F, A.CASE_B, fan)
    kw = dict(features_location=K.LOC_HOST_PINNED, csr_location=K.LOC_HOST_PINNED) if source == "pinned_host" else dict(cache_memory=int(V * F * 4 * 0.15), train_step=2)
    eng = make_engine(K, (V, F, c["indptr"], c["indices"], c["table"]), A.CASE_B, fan, seeds=dict(train=[(seeds, lab)]), **kw)
    fmap = None
    if source == "cache":
        for it in range(2):
            eng.run_batch(0, it, is_presc=True)
        eng.build_cache(cache_agg_mode=0, node_capacity=V // 8, edge_capacity=0, train_step=2)
        assert L.GPUCache_Kg(eng.cache) == 1 and L.GPUCache_NodeCapacity(eng.cache, 0) == V // 8
        fmap = K.read_dev(L.GPUCache_GetFeatureMap(eng.cache, 0), np.int32, V)
    for it in (0, 2):
        ref = orc.run_batch(seeds, lab, it)
        for mode in ("plain", "norm"):
            eng.run_batch(0, it, per_level=(it == 0), **MODES[mode])
            check_batch("%s batch %d %s" % (source, it, mode), mode, ref, eng.result(0), c["table"], c["indptr"], c["indices"], fan)
        if fmap is not None:
            slot = fmap[ref["ids"][int(ref["nc"][3 + 2 * len(fan)]):]]         # the last hop's new nodes: hits and misses were summed
            assert (slot >= 0).any() and (slot < 0).any()
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 2. bit-transparent gathers
# ---------------------------------------------------------------------------------------------------
def bit_case(F, n_seeds=A.CASE_SEEDS):
    """the graph of the shared case under a table of random words"""
    c = A.adversarial_case(A.CASE_V, F, A.CASE_SEED, n_seeds=n_seeds)
    c["table"] = A.bit_pattern_features(c["V"], F, 40 + F)
    words = c["table"].view(np.uint32)
    assert np.isnan(c["table"]).any() and (((words & 0x7F800000) == 0) & ((words & 0x007FFFFF) != 0)).any()     # NaNs and subnormals are in it
    return c


@pytest.mark.parametrize("F,pitched", [(F, p) for F in (1, 7, 36, 100, 128) for p in (False, True) if not (p and F == 128)])     # 128 floats are whole lines
def test_gathers_move_every_bit_pattern(K, oracle, F, pitched):
    """Uniform random 32-bit words as features -- NaNs of every payload, signalling ones included, subnormals, infinities, both zeros:
    every gathered row equals table[ids] as uint32, per level (k_gather behind each hop) and in one launch (k_row_ptrs), dense rows and
    the padded pitch, and rows [0, n_in) of both aggregated modes likewise.  (The sums of this table are not compared: a quarter of a
    percent of its words are NaNs, so nearly every run of 10 draws over F columns would be one, and the NaN cap says such a comparison
    proves nothing.)"""
    L = K.lib()
    assert not pitched or L.legion_row_pitch(F) > F
    c = bit_case(F)
    fan = [5, 3]
    seeds, lab = c["seeds"], c["labels"][c["seeds"]]
    feats, pitch = padded(L, c["table"]) if pitched else (c["table"], 0)
    orc = oracle.OracleRunner(c["indptr"], c["indices"], c["table"], c["V"], F, A.CASE_B, fan)
    eng = make_engine(K, (c["V"], F, c["indptr"], c["indices"], feats), A.CASE_B, fan, seeds=dict(train=[(seeds, lab)]), features_pitch=pitch)
    for it, per_level in ((0, True), (1, False), (2, True), (2, False)):
        ref = orc.run_batch(seeds, lab, it)
        eng.run_batch(0, it, per_level=per_level)
        check_batch("batch %d per_level %s" % (it, per_level), "default", ref, eng.result(0), c["table"], c["indptr"], c["indices"], fan)
        for mode in ("plain", "norm"):
            eng.run_batch(0, it, per_level=per_level, **MODES[mode])
            check_batch("batch %d %s" % (it, mode), mode, ref, eng.result(0), c["table"], c["indptr"], c["indices"], fan, sums=False)
    eng.close()


@pytest.mark.parametrize("pitched", [False, True])
def test_gathers_move_every_bit_pattern_from_the_host_table(K, oracle, pitched):
    """... from a table in pinned host memory, dense and at the padded pitch (F = 36)"""
    L = K.lib()
    F, fan = 36, [5, 3]
    c = bit_case(F)
    seeds, lab = c["seeds"], c["labels"][c["seeds"]]
    feats, pitch = padded(L, c["table"]) if pitched else (c["table"], 0)
    orc = oracle.OracleRunner(c["indptr"], c["indices"], c["table"], c["V"], F, A.CASE_B, fan)
    eng = make_engine(K, (c["V"], F, c["indptr"], c["indices"], feats), A.CASE_B, fan, seeds=dict(train=[(seeds, lab)]), features_pitch=pitch,
                      features_location=K.LOC_HOST_PINNED)
    for it, per_level in ((0, True), (2, False)):
        ref = orc.run_batch(seeds, lab, it)
        eng.run_batch(0, it, per_level=per_level)
        check_batch("batch %d" % it, "default", ref, eng.result(0), c["table"], c["indptr"], c["indices"], fan)
        eng.run_batch(0, it, per_level=per_level, **MODES["norm"])
        check_batch("batch %d norm" % it, "norm", ref, eng.result(0), c["table"], c["indptr"], c["indices"], fan, sums=False)
    eng.close()


@pytest.mark.parametrize("G,lookup,peer", [(1, "pass", None), (1, "fused", None), (2, "fused", "in_kernel"), (2, "pass", "exchange")])
def test_gathers_move_every_bit_pattern_through_the_cache(K, oracle, monkeypatch, G, lookup, peer):
    """... through the unified cache: Kg = 1 with FindFeat as a lookup pass (LEGION_CACHE_HIT_PERIOD=1: k_gather_lookup's sampled form) and fused
    into the gather; a G = 2 logical clique whose peer shard is read in-kernel, and the same clique with LEGION_PEER_GATHER=exchange (the
    peers' rows arrive through the bulk-copy exchange).  Hits, misses and (G = 2) rows of the peer's shard all occur."""
    L = K.lib()
    F, fan = 36, [5, 3]
    c = bit_case(F, n_seeds=1300)
    V = c["V"]
    for name, val in (("LEGION_CACHE_HIT_PERIOD", "1" if lookup == "pass" else None), ("LEGION_PEER_GATHER", "exchange" if peer == "exchange" else None),
                      ("LEGION_SHARD_CHUNK_BYTES", None)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    parts = oracle.split_seeds(c["seeds"], G)
    eng = make_engine(K, (V, F, c["indptr"], c["indices"], c["table"]), A.CASE_B, fan, G=G, seeds=dict(train=[(p, c["labels"][p]) for p in parts]),
                      cache_memory=int(V * F * 4 * 0.3), train_step=2)
    for g in range(G):
        for it in range(2):
            eng.run_batch(g, it, is_presc=True)
    eng.build_cache(cache_agg_mode=G - 1, node_capacity=V // 8, edge_capacity=0, train_step=2)
    assert L.GPUCache_Kg(eng.cache) == G and L.GPUCache_NodeCapacity(eng.cache, 0) == V // 8
    for g in range(G):
        orc = oracle.OracleRunner(c["indptr"], c["indices"], c["table"], V, F, A.CASE_B, fan, partition_count=G)
        L.SetGPUDevice(g)
        fmap = K.read_dev(L.GPUCache_GetFeatureMap(eng.cache, g), np.int32, V)
        for it, per_level in ((0, True), (1, False)):
            ref = orc.run_batch(parts[g], c["labels"][parts[g]], it)
            eng.run_batch(g, it, per_level=per_level)
            check_batch("gpu %d batch %d" % (g, it), "default", ref, eng.result(g), c["table"], c["indptr"], c["indices"], fan)
            slot = fmap[ref["ids"]]
            assert (slot >= 0).any() and (slot < 0).any()
            if G == 2:
                assert ((slot >= 0) & (slot // (V // 8) != g)).any()
            if peer != "exchange":                    # the exchange gather does not serve the aggregated modes (refused by name)
                eng.run_batch(g, it, per_level=per_level, **MODES["plain"])
                check_batch("gpu %d batch %d plain" % (g, it), "plain", ref, eng.result(g), c["table"], c["indptr"], c["indices"], fan, sums=False)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 3. out-degree and weights on star graphs
# ---------------------------------------------------------------------------------------------------
def star_features(V, F=4):
    return np.random.RandomState(V).standard_normal((V, F)).astype(np.float32)      # normal rows: the weight is the only thing under test


@pytest.mark.parametrize("E", A.STAR_E)
@pytest.mark.parametrize("hops", [1, 2])
def test_star_edge_counts_around_the_wave_and_workgroup_size(K, oracle, hops, E):
    """Block 1 has exactly E edges, E on every side of 64 and 256 (k_block_out_deg's first lane beyond E, its last lane, its last thread):
    batch 0 sends every last-hop edge to one position, batch 1 alternates between two.  out_deg == bincount, weighted sums bit-equal."""
    g = A.star_edge_case(E, hops)
    V, fan, B = g["V"], g["fan"], g["B"]
    feats = star_features(V)
    lab = np.zeros(len(g["seeds"]), np.int32)
    orc = oracle.OracleRunner(g["indptr"], g["indices"], feats, V, feats.shape[1], B, fan)
    eng = make_engine(K, (V, feats.shape[1], g["indptr"], g["indices"], feats), B, fan, seeds=dict(train=[(g["seeds"], lab)]))
    for counter in (0, 1):
        ref = orc.run_batch(g["seeds"], lab, counter)
        assert int(ref["ec"][2 + hops]) == E
        eng.run_batch(0, counter, per_level=bool(counter), **MODES["norm"])
        n_in, N, d = check_batch("E %d batch %d" % (E, counter), "norm", ref, eng.result(0), feats, g["indptr"], g["indices"], fan)
        assert int(d.sum()) == E and {int(v): int(d[i]) for i, v in enumerate(ref["ids"]) if d[i]} == {k: v for k, v in g["want"][counter].items() if v}
    eng.close()


@pytest.mark.parametrize("arrangement", ["grouped", "round_robin"])
@pytest.mark.parametrize("hops", [1, 2])
def test_star_degrees_cover_one_to_1024_and_fifty_thousand(K, oracle, hops, arrangement):
    """Chosen out-degrees: every integer of [1, 1024] and 52 500 (one position receives all B * f last-hop edges of a batch), a self-targeting
    input, fan-out 25.  grouped: src_off holds one run of d equal positions per target -- runs of 3 x 256 and more, runs that begin and end
    in lanes 63 / 0 / 1 and threads 255 / 0 / 1 (asserted in tests/test_agg_numerics_cpu.py on these very graphs).  round_robin: the same
    inputs, the batch's targets taking turns.  The coverage is asserted on the reference's degrees; the GPU's must equal them, and every
    weighted sum the statement's bit for bit -- 242 of these degrees have a weight that a once-rounded 1 / sqrt(d) gets wrong."""
    f, B = 25, 2100
    g = A.star_graph(A.coverage_batches(f, B, np.random.RandomState(4)), f, B, arrangement, hops=hops, self_target=7, seed=9)
    V, fan = g["V"], g["fan"]
    feats = star_features(V)
    lab = np.zeros(len(g["seeds"]), np.int32)
    orc = oracle.OracleRunner(g["indptr"], g["indices"], feats, V, feats.shape[1], B, fan)
    eng = make_engine(K, (V, feats.shape[1], g["indptr"], g["indices"], feats), B, fan, seeds=dict(train=[(g["seeds"], lab)]))
    seen, longest = set(), 0
    for counter in range(len(g["want"])):
        ref = orc.run_batch(g["seeds"], lab, counter)
        eng.run_batch(0, counter, per_level=bool(counter & 1), **MODES["norm"])
        n_in, N, d = check_batch("batch %d" % counter, "norm", ref, eng.result(0), feats, g["indptr"], g["indices"], fan)
        seen |= set(d.tolist())
        longest = max(longest, int(A.equal_runs(ref["src_off"])[1].max()))
    assert set(range(1, 1025)) <= seen and max(seen) >= 50000 and longest >= 3 * 256, (len(seen), max(seen), longest)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 4. randomised differential of the three modes on one engine
# ---------------------------------------------------------------------------------------------------
LAST_FANS = (1, 2, 7, 8, 9, 15, 16, 17, 25, 40)          # around k_gather_sum's unroll of 8
MODE_CYCLE = ("default", "plain", "norm", "plain", "default", "norm")     # walked once around from any start: every switch, in both directions


def random_config(seed):
    """seed -> (configuration, graph + table, the sequence of batches).  Pure NumPy: what a failure prints, and what can be replayed without a GPU."""
    rng = np.random.RandomState(9000 + seed)
    V = int(rng.choice([33, 200, 1500, 6000]))
    F = int(rng.choice([1, 2, 3, 4, 5, 8, 20, 36, 64, 100]))
    deg = rng.geometric(0.25, size=V) - 1                  # test_gpu_parity.py::test_randomised_differential's recipe: isolated nodes, hubs,
    hubs = rng.randint(0, V, size=max(1, V // 100))        # skewed neighbours, -1 entries, self loops, repeated seeds
    deg[hubs] = rng.randint(50, 400, size=len(hubs))
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    nbr = np.where(rng.rand(int(indptr[-1])) < 0.5, rng.choice(hubs, size=int(indptr[-1])), rng.randint(0, V, size=int(indptr[-1])))
    nbr[rng.rand(len(nbr)) < 0.02] = -1
    indices = nbr.astype(np.int32)
    labels = rng.randint(0, 7, size=V).astype(np.int32)
    hops = int(rng.randint(1, 5))
    fan = [int(rng.randint(1, 12)) for _ in range(hops - 1)] + [int(rng.choice(LAST_FANS))]
    width = int(np.prod(fan[:-1]))                         # runs per seed, at most: the NumPy statement is kept to a few thousand runs
    n_seeds = int(rng.randint(5, max(6, min(V, 900))))
    B = int(rng.randint(2, max(2, min(n_seeds - 1, 4000 // width)) + 1))
    if n_seeds % B == 0:
        n_seeds -= 1                                       # the last batch is short
    seeds = rng.randint(0, V, size=n_seeds).astype(np.int32)
    n_batches = (n_seeds + B - 1) // B
    adversarial = bool(rng.randint(2))
    if adversarial:
        # non-finite rows at a share that keeps the expected NaN share of the sums near 2 %: a run of f draws meets one with probability
        # <= f * share, and it spoils cols of the F columns
        cols = len(set(A.special_columns(F)))
        share = min(0.025, 0.02 * F / (cols * fan[-1]))
        table = A.adversarial_features(V, F, 500 + seed, keep_out=hubs, nonfinite=share)[0]
    else:
        table = rng.standard_normal((V, F)).astype(np.float32)
    cfg = dict(seed=seed, V=V, F=F, fan=fan, B=B, n_seeds=n_seeds, adversarial=adversarial, pitched=bool(rng.randint(2)), host_table=bool(rng.randint(2)),
               pipeline_depth=int(rng.randint(1, 3)))
    start = int(rng.randint(len(MODE_CYCLE)))
    seq = [dict(counter=int(rng.randint(n_batches)), mode=MODE_CYCLE[(start + i) % len(MODE_CYCLE)]) for i in range(len(MODE_CYCLE) + 1)]
    # the short last batch, then batch 0 in the same mode on the same pipe: the launch-size feedback (rows_hint) of that pipe is smaller than the batch
    mode, pipe = MODE_CYCLE[int(rng.randint(3))], int(rng.randint(cfg["pipeline_depth"]))
    seq += [dict(counter=n_batches - 1, mode=mode, pipe=pipe), dict(counter=0, mode=mode, pipe=pipe)]
    for s in seq:
        s.setdefault("pipe", int(rng.randint(cfg["pipeline_depth"])))
        s.update(per_level=bool(rng.randint(2)), plan=bool(rng.randint(2)))
    modes = [s["mode"] for s in seq]
    assert set(modes) == set(MODES) and {(a, b) for a, b in zip(modes, modes[1:]) if a != b} >= {(a, b) for a in MODES for b in MODES if a != b}
    assert n_batches >= 2 and n_seeds % B and len(seq) >= 6
    return cfg, dict(indptr=indptr, indices=indices, labels=labels, seeds=seeds, table=table), seq


@pytest.mark.parametrize("seed", range(int(os.environ.get("LEGION_STRESS_AGG_N", "16"))))
def test_randomised_aggregated_differential(K, oracle, seed):
    """Random graphs (hubs, isolated nodes, -1 entries, repeated seeds), V, F in {1, 2, 3, 4, 5, 8, 20, 36, 64, 100}, H = 1..4 with fan-outs
    1..11 before the last hop and a last fan-out around the unroll of 8, batch size, padded pitch, device or pinned-host table, adversarial or
    normal features, one or two pipes; on one engine nine batches whose mode (default / plain sums / normalised), per_level, plan and pipe
    are drawn per batch: every mode, every switch between two modes in both directions, and the short last batch followed by batch 0 on the
    same pipe.  Every batch in full under the module's rules.  The configuration is printed: pytest shows it when the test fails."""
    L = K.lib()
    cfg, g, seq = random_config(seed)
    print("seed %d -> %s" % (seed, cfg))
    for s in seq:
        print("   ", s)
    V, F, fan, B = cfg["V"], cfg["F"], cfg["fan"], cfg["B"]
    seeds, lab = g["seeds"], g["labels"][g["seeds"]]
    feats, pitch = padded(L, g["table"]) if cfg["pitched"] else (g["table"], 0)
    orc = oracle.OracleRunner(g["indptr"], g["indices"], g["table"], V, F, B, fan)
    eng = make_engine(K, (V, F, g["indptr"], g["indices"], feats), B, fan, seeds=dict(train=[(seeds, lab)]), features_pitch=pitch,
                      features_location=K.LOC_HOST_PINNED if cfg["host_table"] else K.LOC_DEVICE, pipeline_depth=cfg["pipeline_depth"])
    for i, s in enumerate(seq):
        ref = orc.run_batch(seeds, lab, s["counter"])
        eng.run_batch(0, s["counter"], per_level=s["per_level"], plan=s["plan"], pipe=s["pipe"], **MODES[s["mode"]])
        check_batch("step %d %s" % (i, s), s["mode"], ref, eng.result(0, pipe=s["pipe"]), g["table"], g["indptr"], g["indices"], fan)
    eng.close()
