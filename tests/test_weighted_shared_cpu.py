"""Weighted shared-key sampling (LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1 LEGION_SHARED_DRAWS=1, INTEGRATION.md "Weighted
shared-key sampling"), the parts that need no GPU: the statement of tests/wsharedref.py against a plain-Python restatement, the properties
that make it what it is (per row it is weighted sampling without replacement; rows that list the same neighbours at the same weights agree;
a batch reaches far fewer nodes than under per-column keys), the near ties of every batch the GPU tests compare, the environment parser
through the `legion` binary's boot, the pool's flags without a device, the C ABI's new name and the Engine's argument check."""
import math
import os
import subprocess

import numpy as np
import pytest

import distinctref as D
import drawrulecases as DR
import wdistinctref as WD
import wsharedcases as C
import wsharedref as R
from conftest import ROOT
from distinctref import mix32_scalar

SERVER = os.path.join(ROOT, "legion-1_amd", "csrc", "legion")
MODE_VARS = ("LEGION_AGG_LAST_HOP", "LEGION_AGG_NORM", "LEGION_SAMPLING", "LEGION_SAMPLING_SEED", "LEGION_LP_DRAW", "LEGION_WEIGHTED_DISTINCT",
             "LEGION_SHARED_DRAWS")


def scalar_picks(nbr, w_row, f, W=0):
    """the statement once more, per row in plain Python: sort by (key, column), take f, sort by column"""
    Ksw = mix32_scalar(mix32_scalar((W & 0xFFFFFFFF) ^ 0x165667B1) ^ 0x27D4EB2F)
    keyed = []
    for c, (x, wt) in enumerate(zip(nbr, w_row)):
        if wt > 0:
            u = mix32_scalar((int(x) & 0xFFFFFFFF) ^ Ksw)
            keyed.append((-math.log((u + 0.5) * 2.0 ** -32) / float(wt), c))
    keyed.sort()
    return sorted(c for _, c in keyed[:f])


def random_rows(seed, n):
    """(nbr, weights, f, W): d in 1..400, f in {1, 5, 10, 25, 64}, ids from a small alphabet (multi-edges throughout) or the whole int32
    range, one entry in ten a hole (-1), the weight alphabet 0..16 (so a node's duplicates come at equal and at unequal weights)"""
    rng = np.random.RandomState(seed)
    for _ in range(n):
        d = int(rng.randint(1, 401))
        small = rng.rand() < 0.5
        nbr = rng.randint(0, 40, size=d) if small else rng.randint(-2 ** 31, 2 ** 31 - 1, size=d, dtype=np.int64)
        nbr = np.where(rng.rand(d) < 0.1, -1, nbr).astype(np.int32)
        w = rng.randint(0, 17, size=d).astype(np.float32)
        if rng.rand() < 0.1:
            w[:] = 0
        if rng.rand() < 0.2:
            w[rng.rand(d) < 0.9] = 0                                     # few eligible columns: m <= f < d occurs
        yield nbr, w, int(rng.choice([1, 5, 10, 25, 64])), int(rng.randint(0, 2 ** 32, dtype=np.uint64))


# ---- the statement ------------------------------------------------------------------------------------
def test_statement_agrees_with_a_plain_loop_on_random_rows():
    n = seen_small = seen_cut = seen_zero = seen_exact = 0
    for nbr, w, f, W in random_rows(13, 200):
        picks, gap, exact = R.row_picks(nbr, w, f, W)
        elig = np.nonzero(w > 0)[0]
        m = len(elig)
        assert picks.tolist() == scalar_picks(nbr.tolist(), w.tolist(), f, W), (len(nbr), f, W)
        assert len(picks) == min(m, f) and (np.diff(picks) > 0).all() and np.isin(picks, elig).all()
        assert gap >= R.TIE_MARGIN                                       # an exact tie reports inf: it is no near tie
        if m <= f:
            assert picks.tolist() == elig.tolist() and gap == np.inf and not exact
            seen_small += m > 0 and len(w) > f
            seen_zero += m == 0
        else:
            seen_cut += 1
            seen_exact += exact
        n += 1
    assert n == 200 and seen_small > 3 and seen_cut > 80 and seen_zero > 5 and seen_exact > 3


def test_a_row_with_duplicate_ids_of_equal_and_of_unequal_weight():
    """Columns 0..5 hold node 9 at weight 4: six bit-equal keys, taken in column order.  Columns 6..8 hold node 9 at weights 1, 2, 64: the
    same uniform, keys in the inverse order of the weights.  So node 9's columns rank 8 (weight 64), then 0..5, then 7, then 6."""
    nbr = np.array([9] * 9 + [11, 12, 13], np.int32)
    w = np.array([4] * 6 + [1, 2, 64] + [1e-30] * 3, np.float32)          # the other nodes never enter before node 9 is used up
    for W in (0, 5, 0xDEADBEEF):
        for f, want in ((1, [8]), (3, [0, 1, 8]), (7, [0, 1, 2, 3, 4, 5, 8]), (8, [0, 1, 2, 3, 4, 5, 7, 8]), (9, list(range(9)))):
            picks, gap, exact = R.row_picks(nbr, w, f, W)
            assert picks.tolist() == want == scalar_picks(nbr.tolist(), w.tolist(), f, W)
            assert exact == (f == 3)                                       # of these, only f = 3 cuts between two of the six equal columns
            assert gap >= R.TIE_MARGIN
    u, key = R.node_keys(nbr[:9], w[:9], 0)
    assert len(set(u.tolist())) == 1 and len(set(key[:6].tolist())) == 1 and key[8] < key[0] < key[7] < key[6]
    assert R.node_keys(np.array([-1], np.int32), np.float32(1), 0)[0].tolist() == [mix32_scalar(0xFFFFFFFF ^ R.salt(0))]   # a hole: its bit pattern


def test_inclusion_frequencies_on_distinct_ids_are_weighted_sampling_without_replacement():
    """d = 8 distinct ids, f = 3, weights {1, 1, 2, 2, 4, 4, 8, 0} over 20 000 draw words: the inclusion counts of the seven eligible columns
    against the exact successive-sampling probabilities (wdistinctref.inclusion_probabilities: a plain recursion, exact at this size) by
    the statistic sum (o - e)^2 / e under distinctref.chi2_cap.  A column's count is binomial(N, p), so its term has mean 1 - p and the sum
    has mean d' - f = 4 over the d' = 7 eligible columns; the counts sum to f N, so the quadratic form has at most 6 non-zero directions:
    the cap is the chi-square quantile at 6 degrees of freedom, whose mean is above the statistic's."""
    d, f, N = 8, 3, 20000
    nbr = np.random.RandomState(4).choice(100000, size=d, replace=False).astype(np.int32)
    w = np.array([1, 1, 2, 2, 4, 4, 8, 0], np.float32)
    p = WD.inclusion_probabilities(w, f)
    assert abs(sum(p) - f) < 1e-12 and p[7] == 0.0
    words = np.arange(N, dtype=np.int64) * 2654435761 % (1 << 32)
    _, key = R.node_keys(np.broadcast_to(nbr, (N, d)), np.broadcast_to(w, (N, d)), words[:, None])
    taken = np.argsort(key, axis=1, kind="stable")[:, :f]
    assert sorted(taken[17].tolist()) == R.row_picks(nbr, w, f, int(words[17]))[0].tolist()      # the same rule as the statement's
    counts = np.bincount(taken.reshape(-1), minlength=d)
    e = N * np.array(p[:7])
    chi2 = float(((counts[:7] - e) ** 2 / e).sum())
    print("inclusion counts", counts.tolist(), "expected", [round(x, 1) for x in e], "chi2 = %.2f, cap %.2f" % (chi2, D.chi2_cap(6)))
    assert counts[7] == 0 and chi2 <= D.chi2_cap(6)


def test_rows_that_list_the_same_neighbours_at_the_same_weights_agree():
    rng = np.random.RandomState(8)
    for f, W in ((5, 0), (10, 77), (64, 0xDEADBEEF)):
        nbr = rng.choice(5000, size=150, replace=False).astype(np.int32)
        w = rng.randint(1, 17, size=150).astype(np.float32)
        perm = rng.permutation(150)
        a, b = R.row_picks(nbr, w, f, W)[0], R.row_picks(nbr[perm], w[perm], f, W)[0]
        assert len(a) == f and sorted(nbr[a].tolist()) == sorted(nbr[perm][b].tolist())
        assert sorted(nbr[a].tolist()) != sorted(nbr[R.row_picks(nbr, w, f, W + 1)[0]].tolist())     # the draw word does enter
        # ... which the per-column rule does not do: there the hash belongs to the column and the row
        c, d = WD.row_picks(3, 1, w, f, W)[0], WD.row_picks(3, 1, w[perm], f, W)[0]
        assert sorted(nbr[c].tolist()) != sorted(nbr[perm][d].tolist())


def test_the_point_of_the_mode_fewer_nodes_for_the_same_edges():
    """products @ 0.05, B = 1000, {25, 10, 5}, the synth: source's weights, seed 7, batches 0 and 3: at most 0.70 of the unique nodes of
    weighted sampling without replacement (the trial statement gave 0.632 and 0.641, for the same number of edges to within 0.3 %).  The
    bound is a condition on the statement -- one key per node and batch --, not a speed claim."""
    import legion1_amd.synth as S
    spec = S.spec_for("products", scale=0.05)
    ds = S.generate(spec, with_features=False)
    g = R.Weights(ds.indptr, ds.indices, S.edge_weights(ds.E))
    zero = np.zeros((spec.V, 1), np.float32)
    B, fan = 1000, [25, 10, 5]
    lab = np.zeros(len(ds.train), np.int32)
    a_st, b_st = WD.Statement(g, zero, B, fan, seed=7), R.Statement(g, zero, B, fan, seed=7)
    for counter in (0, 3):
        a, b = a_st.run_batch(ds.train, lab, counter), b_st.run_batch(ds.train, lab, counter)
        na, nb = int(a["nc"][5 + 2 * 3]), int(b["nc"][5 + 2 * 3])
        ea, eb = int(a["ec"][2 + 3]), int(b["ec"][2 + 3])
        print("batch %d: per-column keys %d nodes, node keys %d nodes (%.3f), edges %d / %d (%.4f)" % (counter, na, nb, nb / na, ea, eb, eb / ea))
        assert ea > 0 and eb > 0
        assert nb <= 0.70 * na


# ---- near ties of the batches the GPU tests compare bit for bit ------------------------------------------
def test_no_near_tie_in_any_batch_the_gpu_tests_run_and_exact_ties_occur():
    """drawrulecases.graph() at both tiles, counters 0 and 1, draw word 0 and seed 7: no near tie (the GPU tests' cap is zero rows).  Cuts
    between two columns of one node at one weight are there -- bit-equal keys on both sides, settled by the column -- and are not counted."""
    g = C.rule_graph()
    exact = 0
    for tile, (B, fan) in DR.SHAPES.items():
        seeds = DR.seed_list(tile)
        for seed in C.WORDS:
            near, found = C.cuts(g, seeds, B, fan, DR.COUNTERS, seed)
            assert near == [], (tile, seed, near)
            if seed is None:                                                # the module-level forms say the same under one draw word
                assert R.near_ties(g["graph"], seeds, B, DR.COUNTERS, fan) == [] and R.exact_ties(g["graph"], seeds, B, DR.COUNTERS, fan) == found
            print(tile, seed, "exact ties:", found)
            exact += len(found)
    assert exact >= 1


def test_the_hand_made_graphs_seed_is_the_first_without_a_near_tie():
    """wsharedcases.HAND_SEED: the first of 0, 1, 2, ... whose graph leaves no near tie in any batch the GPU test runs on it; the hub's forty
    equal columns put exact ties at the cut."""
    first = next(s for s in range(C.HAND_SEED + 1) if C.hand_near_ties(C.hand_made_graph(s)) == [])
    assert first == C.HAND_SEED
    g = C.hand_made_graph(C.HAND_SEED)
    hub_exact = [t for seed in C.WORDS for t in C.cuts(g, g["seeds"], C.HB, [25, 5, 5], (0,), seed)[1] if t[1:] == (1, C.HUB)]
    assert hub_exact, "the hub's cut at f = 25 is meant to fall among the forty equal columns"
    # ... and node MIXED's forty columns of different weights are picked more than once
    for fan in ([25, 5, 5], [64, 64]):
        ids = R.Statement(g["graph"], g["feats"], C.HB, fan).run_batch(g["seeds"], g["labels"][g["seeds"]], 0)["draws"][0].reshape(-1, fan[0])
        print(fan, "hub: TWIN x %d, MIXED x %d" % ((ids[C.HUB] == C.TWIN).sum(), (ids[C.HUB] == C.MIXED).sum()))
    assert (ids[C.HUB] == C.MIXED).sum() >= 2


def test_no_near_tie_in_the_served_batches(synth, oracle):
    """What tests/test_gpu_weighted_shared.py serves: products @ 0.004, B = 96, {10, 5}, seed 7, two epochs.  Every batch of every list in
    both rounds (the schedule runs a subset of them): no near tie."""
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec, with_features=False)
    B, fan = 96, [10, 5]
    st = R.Statement(R.Weights(ds.indptr, ds.indices, synth.edge_weights(ds.E)), np.zeros((spec.V, 1), np.float32), B, fan, seed=C.SEED)
    va, te = oracle.split_seeds(ds.valid[:min(700, spec.n_valid)], 1), oracle.split_seeds(ds.test[:min(300, spec.n_test)], 1)
    steps, tb, vb, sb = oracle.coordinate([len(ds.train)], [len(va[0])], [len(te[0])], B)
    n = 0
    for rnd in (0, 1):
        for mode, ids, bs in ((0, ds.train, tb[0]), (1, va[0], vb[0]), (2, te[0], sb[0])):
            for it in range(int(steps[mode])):
                st.run_batch(ids, ds.labels[ids], it, mode=mode, batch_size=int(bs), round=rnd)
                n += 1
    print("%d batches, exact ties %d" % (n, len(st.exact)))
    assert n >= 6 and st.ties == []


# ---- parser and boot ----------------------------------------------------------------------------------
ACCEPTED = "Server_Initialize: the synth: dataset path names no known workload / scale"
NEEDS_KIND = "Server_Initialize: LEGION_SHARED_DRAWS=1 needs LEGION_SAMPLING=distinct: the flag keys the distinct draws by the neighbour node"
NEEDS_SEED = ("Server_Initialize: LEGION_SHARED_DRAWS=1 needs LEGION_SAMPLING_SEED: the node keys come from the batch's draw word, and without a seed "
              "every batch of every epoch would prefer the same nodes")


@pytest.mark.parametrize("sampling,wd,seed,flag,fanout,said", [
    ("weighted", "1", "7", "1", "25,10", ACCEPTED),
    ("weighted", "1", "0", "1", "64,2", ACCEPTED),                       # seed 0 is a seed
    ("weighted", "1", None, "0", "10,5", ACCEPTED),
    ("weighted", "1", None, "1", "10,5", NEEDS_SEED),
    ("weighted", None, "7", "1", "10,5", NEEDS_KIND),                    # the flag acts under the weighted kind only on top of LEGION_WEIGHTED_DISTINCT
    ("weighted", "0", "7", "1", "10,5", NEEDS_KIND),
    ("distinct", "1", "7", "1", "10,5", "Server_Initialize: LEGION_WEIGHTED_DISTINCT=1 needs LEGION_SAMPLING=weighted"),
    ("weighted", "1", "7", "2", "10,5", "Server_Initialize: LEGION_SHARED_DRAWS=2 is not a known setting"),
    ("weighted", "1", "7", "1", "65,2", "Server_Initialize: LEGION_WEIGHTED_DISTINCT=1 LEGION_SHARED_DRAWS=1 takes fan-outs of at most 64, hop 1 has 65: k_sample keeps a "
                                        "row's best picks one per lane and stages them in static LDS"),
    ("weighted", "1", "7", "1", "10,70", "Server_Initialize: LEGION_WEIGHTED_DISTINCT=1 LEGION_SHARED_DRAWS=1 takes fan-outs of at most 64, hop 2 has 70"),
])
def test_boot_parses_the_triple(tmp_path, sampling, wd, seed, flag, fanout, said):
    """serve_modes_from_env and serve_modes_fit_fanout through the server's boot.  Every refusal comes before a device is touched: this
    machine has none, and the accepted settings get as far as the synth: source."""
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write("synth:nosuchworkload 512 1000 0 16 100 0 0 %d 1 0\n" % (1 << 30))
    env = {k: v for k, v in os.environ.items() if k not in MODE_VARS}
    env.update(LEGION_IPC_NAMESPACE="cpuws%d_" % os.getpid())
    for name, value in (("LEGION_SAMPLING", sampling), ("LEGION_WEIGHTED_DISTINCT", wd), ("LEGION_SAMPLING_SEED", seed), ("LEGION_SHARED_DRAWS", flag)):
        if value is not None:
            env[name] = value
    r = subprocess.run([SERVER, "1", "0", fanout, meta], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 1 and said in out, out[-2000:]


# ---- the pool's flags, without a device ---------------------------------------------------------------
def test_pool_flags_round_trip_without_a_gpu():
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    pool = L.NewGPUMemoryPool(2)

    def err():
        msg = (L.legion_last_error() or b"").decode()
        L.legion_clear_error()
        return msg
    try:
        L.GPUMemoryPool_SetSampling(pool, 2)
        for wd in (0, 1):
            for sd in (0, 1):                                               # the rule is the three together: no new field, no fourth kind
                L.GPUMemoryPool_SetWeightedDistinct(pool, wd)
                L.GPUMemoryPool_SetSharedDraws(pool, sd)
                assert not err()
                assert (L.GPUMemoryPool_GetSampling(pool), L.GPUMemoryPool_GetWeightedDistinct(pool), L.GPUMemoryPool_GetSharedDraws(pool)) == (2, wd, sd)
                assert L.GPUMemoryPool_GetSampleDistinct(pool) == 0
        for kind in (0, 1, 2):                                               # both flags are remembered across kinds
            L.GPUMemoryPool_SetSampling(pool, kind)
            assert not err() and (L.GPUMemoryPool_GetSampling(pool), L.GPUMemoryPool_GetWeightedDistinct(pool), L.GPUMemoryPool_GetSharedDraws(pool)) == (kind, 1, 1)
        L.legion_weighted_shared_probe(None, None, None, None, None, None, 4)
        assert "legion_weighted_shared_probe: null array" in err()
        L.legion_weighted_shared_probe(None, None, None, None, None, None, 0)  # nothing to do: no device is touched
        assert not err()
    finally:
        L.legion_clear_error()
        L.GPUMemoryPool_Delete(pool)


def test_capi_table_and_header_name_the_probe():
    import legion1_amd.capi as K
    L = K.lib()
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    assert "legion_weighted_shared_probe" in K._SIGS and "legion_weighted_shared_probe(" in header and L.legion_weighted_shared_probe


def test_engine_takes_the_flag_on_top_of_weighted_distinct_only():
    import legion1_amd.capi as K
    eng = K.Engine.__new__(K.Engine)            # no device: _set_modes validates its arguments first
    with pytest.raises(ValueError, match="shared_draws=True needs sample='distinct'"):
        eng._set_modes(0, False, None, "weighted", None, 0, None, shared_draws=True)
    with pytest.raises(ValueError, match="weighted_distinct=True needs sample='weighted'"):
        eng._set_modes(0, False, None, "distinct", None, 0, None, weighted_distinct=True, shared_draws=True)
    # the triple passes the flag checks: the next refusal is about the Engine's tables, which this stand-in says it lacks
    eng.has_edge_weights = lambda: False
    with pytest.raises(ValueError, match="sample='weighted' needs the Engine's edge_weights"):
        eng._set_modes(0, False, None, "weighted", None, 0, None, weighted_distinct=True, shared_draws=True)
    eng.has_edge_weights, eng.has_retained_edge_weights = (lambda: True), (lambda: False)
    with pytest.raises(ValueError, match="weighted_distinct=True needs the weights kept on the device"):
        eng._set_modes(0, False, None, "weighted", None, 0, None, weighted_distinct=True, shared_draws=True)
