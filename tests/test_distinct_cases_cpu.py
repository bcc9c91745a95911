"""Every input of tests/test_gpu_distinct_cross.py is generated here first and held to its purpose before a GPU looks at it: the switch cases
lie on the intended side of kNarrowSlots and hold the rows the distinct mode is about across the edges of the tile they run; the randomised
configurations are never trivially take-all and walk every (sampling, hand-off) state and switch; every mutant draw of tests/distinctcases.py
is told from the statement by a new switch case at the tile that case runs; the ladder graph has the degrees it names."""
import numpy as np
import pytest

import distinctcases as X
import distinctref as D
from aggref import expected_nbr_sum
from conftest import assert_batch_equal
from gcnref import expected_nbr_sum_norm


def differs(want, got):
    try:
        assert_batch_equal(want, got)
    except AssertionError:
        return True
    return False


# ---- the helper itself -------------------------------------------------------------------------------------
def test_floyd_with_every_switch_off_is_the_statement():
    rng = np.random.RandomState(1)
    for f in (1, 2, 3, 25, 63, 64):
        n = 3000
        rows = rng.randint(0, 2 ** 31 - 1, size=n).astype(np.int64)
        hop = rng.randint(1, 5, size=n)
        deg = np.concatenate([rng.randint(-1, 3 * f + 2, size=n - 100), rng.randint(f + 1, 2 ** 31 - 1, size=100)]).astype(np.int64)
        want = D.positions(rows, hop, deg, f)
        assert np.array_equal(X.floyd(rows, hop, deg, f), want)
        assert np.array_equal(X.floyd(rows, hop, deg, f, restart=np.full(n, f)), want)      # a restart behind the row is none
        # every mutant of the table is the statement on rows it is not about: d < f for all of them
        small = deg < f
        for name in X.MUTANTS:
            got = X.mutant_draw(name, 4, [f])(np.arange(n), 1, deg, f)
            assert np.array_equal(got[small], D.positions(np.arange(n), 1, deg, f)[small]), name
        tiles = X.hop_tiles(4, [f])
        assert np.array_equal(X.mutant_key_in_tile(tiles, 1024)(rows, 1, deg, f), D.positions(rows, 1, deg, f))      # that hop runs the 256-slot tile
        assert np.array_equal(X.mutant_restart_at_edge(tiles, 1024)(rows, 1, deg, f), D.positions(rows, 1, deg, f))


def test_mutants_do_what_their_names_say():
    f = 5
    rows, deg = np.arange(400, dtype=np.int64), np.full(400, 9, dtype=np.int64)
    want = D.positions(rows, 1, deg, f)
    # 1: rows of tile 0 keep their key (i0 = 0), rows behind it do not; a row on the edge (slots 255 | 256: row 51) is split between two keys
    got = X.mutant_key_in_tile([256])(rows, 1, deg, f)
    assert np.array_equal(got[:51], want[:51]) and got[51, 0] == want[51, 0] and not np.array_equal(got[52:], want[52:])
    assert np.array_equal(got[52:102], D.positions(rows[52:102] - 51, 1, deg[52:102], f))     # tile 1 begins inside row 51: i0 = 51
    # 2: only rows on a tile edge can differ, and only in slots behind the edge
    many = np.arange(4000, dtype=np.int64)
    got = X.mutant_restart_at_edge([256])(many, 1, np.full(4000, 6), f)
    w6 = D.positions(many, 1, np.full(4000, 6), f)
    on_edge = X.crossing(4000, f, 256)
    assert np.array_equal(got[~on_edge], w6[~on_edge]) and on_edge.sum() == 78 - 78 // 5      # 78 tile edges; every fifth falls between two rows
    for m in np.nonzero(on_edge)[0]:
        c = 256 - (m * f) % 256
        assert np.array_equal(got[m, :c], w6[m, :c])
    assert any(len(set(r)) < f for r in got[on_edge].tolist())                            # a restart repeats a neighbour sooner or later
    # 3: Floyd at d == f is the identity whatever the key (an equivalent mutant); 3b: a row of d == f + 1 never takes its last neighbour
    rng = np.random.RandomState(3)
    for ff in (1, 2, 5, 25, 63, 64):
        keys = rng.randint(0, 2 ** 31 - 1, size=20000).astype(np.int64)
        d_all = rng.randint(-1, 3 * ff, size=20000)
        d_all[:5000] = ff
        for h in (1, 4):
            assert np.array_equal(X.mutant_take_all_below_f(keys, h, d_all, ff), D.positions(keys, h, d_all, ff))
    got = X.mutant_take_all_up_to_f1(rows, 1, np.full(400, f + 1), f)
    assert (got == np.arange(f)).all() and (D.positions(rows, 1, np.full(400, f + 1), f) == f).any()
    assert np.array_equal(X.mutant_take_all_up_to_f1(rows, 1, deg, f), want)
    # 4: repeats survive
    got = X.mutant_raw_compare(rows, 1, np.full(400, 6), f)
    assert any(len(set(r)) < f for r in got.tolist())
    # 5: the same picks at every hop
    assert np.array_equal(X.mutant_no_hop(rows, 1, deg, f), X.mutant_no_hop(rows, 3, deg, f)) and not np.array_equal(X.mutant_no_hop(rows, 1, deg, f), want)


def test_hop_tiles():
    assert X.hop_tiles(8192, [32]) == [256] and X.hop_tiles(8193, [32]) == [1024]
    assert X.hop_tiles(1024, [16, 16, 2]) == [256, 256, 1024] and X.hop_tiles(1, [1, 1, 1, 1]) == [256] * 4
    assert X.hop_bounds(1049, [25, 10]) == [26225, 262250]


# ---- A: the switch cases ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def switch():
    """the graph and, per case, (seeds, the statement's batches 0, 1 and 2): computed once, read by every test below"""
    g = X.switch_graph()
    out = {}
    for B, fan, tiles, straddling in X.SWITCH_CASES:
        seeds = X.switch_seeds(g, B, fan)
        lab = g["labels"][seeds]
        out[(B, tuple(fan))] = (seeds, [D.run_batch(g["indptr"], g["indices"], g["feats"], seeds, lab, B, it, fan) for it in (0, 1, 2)])
    return g, out


def test_switch_bounds_fall_on_the_intended_side():
    for B, fan, tiles, straddling in X.SWITCH_CASES:
        assert X.hop_tiles(B, fan) == tiles, (B, fan)
    bound = {(B, tuple(fan)): X.hop_bounds(B, fan)[-1] for B, fan, _, _ in X.SWITCH_CASES}
    assert bound[(10485, (25,))] == 262125 and bound[(10486, (25,))] == 262150 and bound[(4161, (63,))] == 262143 and bound[(4162, (63,))] == 262206
    assert bound[(87381, (3,))] == X.NARROW_SLOTS - 1 and bound[(87382, (3,))] == X.NARROW_SLOTS + 2 and bound[(1049, (25, 10))] == 262250
    assert bound[(4096, (64,))] == X.NARROW_SLOTS and bound[(4097, (64,))] == X.NARROW_SLOTS + 64


@pytest.mark.parametrize("B,fan,tiles,straddling", X.SWITCH_CASES)
def test_switch_cases_hold_the_rows_they_are_about(switch, B, fan, tiles, straddling):
    g, cases = switch
    seeds, batches = cases[(B, tuple(fan))]
    assert len(seeds) == 2 * B + B // 3
    for it, want in enumerate(batches):
        cov = X.coverage(want, g["indptr"], fan, B)
        print("B %d fan %s batch %d:" % (B, fan, it), cov)
        assert [c["tile"] for c in cov] == tiles
        for h in straddling:          # >= 50 in the full batches; the short one has a third of the tile edges
            assert cov[h - 1]["big_cross_tile"] >= (50 if it < 2 else 1), (it, cov[h - 1])
            assert cov[h - 1]["big_cross_wave"] >= cov[h - 1]["big_cross_tile"]             # a tile edge is a wave edge
        assert sum(c["eq_f"] for c in cov) > 0 and sum(c["eq_f1"] for c in cov) > 0
        assert sum(c["none"] for c in cov) > 0 and sum(c["small"] for c in cov) > 0 and sum(c["holes"] for c in cov) > 0
        if fan == [64]:
            assert cov[0]["big_cross_tile"] == 0 and cov[0]["big_cross_wave"] == 0 and cov[0]["big"] > 50
    assert int(batches[2]["nc"][4]) == B // 3                                           # the short one
    assert len(set(seeds[:B].tolist())) < B                                                 # seeds repeat inside a batch


def test_clique_case_runs_a_wide_second_hop():
    g = X.clique_case()
    assert g["V"] <= 60000 and X.hop_tiles(X.CLIQUE_B, X.CLIQUE_FAN) == [256, 1024]
    assert not set(g["parts"][0].tolist()) & set(g["parts"][1].tolist())
    for p in g["parts"]:
        want = D.run_batch(g["indptr"], g["indices"], g["feats"], p, g["labels"][p], X.CLIQUE_B, 0, X.CLIQUE_FAN)
        cov = X.coverage(want, g["indptr"], X.CLIQUE_FAN, X.CLIQUE_B)
        assert cov[1]["big_cross_tile"] >= 50 and cov[1]["eq_f"] > 0 and cov[1]["eq_f1"] > 0 and cov[1]["slots"] > 128 * 1024, cov


# ---- D: the randomised configurations -----------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(16))
def test_randomised_configurations(seed):
    cfg, g, seq = X.random_config(seed)
    print(cfg)
    assert X.nontrivial_hops(cfg, g), "the generator redraws a configuration whose distinct batch is trivially the take-all batch"
    cfg2, g2, seq2 = X.random_config(seed)
    assert cfg2 == cfg and seq2 == seq and all(np.array_equal(g[k], g2[k]) for k in g)      # a failure can be replayed from its seed
    runs = [s for s in seq if not s.get("replay")]
    states = [(s["sample"], s["hand_off"]) for s in runs]
    assert set(states) == {(s, m) for s in ("replace", "distinct") for m in X.HAND_OFFS}
    switches = {(a[0], b[0], a[1] == b[1]) for a, b in zip(states, states[1:]) if a[0] != b[0]}
    assert switches == {(a, b, kept) for a, b in (("replace", "distinct"), ("distinct", "replace")) for kept in (True, False)}
    n_batches = (cfg["n_seeds"] + cfg["B"] - 1) // cfg["B"]
    assert cfg["n_seeds"] % cfg["B"] and n_batches >= 2
    a, b = runs[-2], runs[-1]
    assert a["counter"] == n_batches - 1 and b["counter"] == 0 and a["pipe"] == b["pipe"] and (a["sample"], a["hand_off"]) == (b["sample"], b["hand_off"])
    assert seq[-2] is a and seq[-1] is b
    # the replays: two per recorded graph, each directly behind a run_batch of the other sampling mode and in front of another run_batch
    for mode in ("replace", "distinct"):
        at = [i for i, s in enumerate(seq) if s.get("replay") and s["sample"] == mode]
        assert len(at) == 2
        for i in at:
            assert i > 0 and not seq[i - 1].get("replay") and seq[i - 1]["sample"] != mode and not seq[i + 1].get("replay")
    assert all(0 <= s["counter"] < n_batches and (s.get("replay") or 0 <= s["pipe"] < cfg["pipeline_depth"]) for s in seq)
    assert 1 <= len(cfg["fan"]) <= 4 and cfg["fan"][-1] in X.LAST_FANS and all(1 <= f <= 11 for f in cfg["fan"][:-1])


def test_randomised_configurations_cover_the_drawn_dimensions():
    cfgs = [X.random_config(seed)[0] for seed in range(16)]
    assert {c["pitched"] for c in cfgs} == {False, True} and {c["host_table"] for c in cfgs} == {False, True} and {c["host_csr"] for c in cfgs} == {False, True}
    assert {c["pipeline_depth"] for c in cfgs} == {1, 2} and len({len(c["fan"]) for c in cfgs}) >= 3 and len({c["V"] for c in cfgs}) >= 3


def test_expected_sums_are_aggrefs_and_gcnrefs():
    """distinctcases.expected_sums against tests/aggref.py and tests/gcnref.py fed with the statement's batch, bit for bit, where those can
    count a run's draws from the graph: graphs without holes (H = 1 with repeated seeds included)."""
    for seed, fan, B in ((0, [5], 60), (1, [4, 7], 50), (2, [3, 2, 25], 40), (3, [64], 30), (4, [2, 1], 64)):
        V = 400
        indptr, indices, labels = X.random_graph(seed, V, max_deg=30)
        feats = np.random.RandomState(seed).standard_normal((V, 3)).astype(np.float32)
        seeds = np.random.RandomState(seed + 50).randint(0, V, size=2 * B + 7).astype(np.int32)
        for it in (0, 2):
            want = D.run_batch(indptr, indices, feats, seeds, labels[seeds], B, it, fan)
            n_in, N, _, S = expected_nbr_sum(want, indptr, indices, fan)
            got = X.expected_sums(want, fan, norm=False)
            assert got[:2] == (n_in, N) and got[3] is None and np.array_equal(got[2].view(np.uint32), S.view(np.uint32))
            n_in, N, _, Sw, d = expected_nbr_sum_norm(want, indptr, indices, fan)
            got = X.expected_sums(want, fan, norm=True)
            assert got[:2] == (n_in, N) and np.array_equal(got[3], d) and np.array_equal(got[2].view(np.uint32), Sw.view(np.uint32))
            assert N > 0 and np.abs(S).sum() > 0


# ---- C: the ladder --------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", X.LADDER_F)
def test_ladder_graph(f):
    g = X.ladder_graph(f)
    deg = np.diff(g["indptr"])
    want = [0, 1, f - 1, f, f + 1, f + 2, 2 * f, 255, 256, 257, 65535, 65536, 65537, 2 ** 20 + 3]
    assert g["want"] == want and deg[:14].tolist() == want and g["indptr"][-1] == len(g["indices"]) and g["F"] == 1
    assert (g["indices"] >= 0).all() and g["indices"].max() < g["V"]
    for k in range(21):
        row = g["indices"][g["indptr"][k]:g["indptr"][k + 1]]
        assert len(np.unique(row)) == len(row), "row %d has a multi-edge" % k
    assert deg[21:].sum() == 0 and g["seeds1"].tolist() == list(range(14))
    # H = 2: fan-out 2 over seeds of degree 2 takes both neighbours in CSR order, so hop 2's input list is the ladder
    b = D.run_batch(g["indptr"], g["indices"], g["feats"], g["seeds2"], g["labels"][g["seeds2"]], len(g["seeds2"]), 0, [2, f])
    inp, cnt = b["draw_counts"][1]
    assert inp.tolist() == list(range(14)) and cnt.tolist() == [min(d, f) for d in want]
    b1 = D.run_batch(g["indptr"], g["indices"], g["feats"], g["seeds1"], g["labels"][g["seeds1"]], 14, 0, [f])
    assert b1["draw_counts"][0][1].tolist() == cnt.tolist() and int(b1["ec"][3]) == int(cnt.sum())


# ---- the mutant table -----------------------------------------------------------------------------------
def former_inputs():
    """what tests/test_gpu_sample_distinct.py feeds whole batches with: test_toy_graphs' twenty (graph, fan-outs) pairs, every batch of
    each, and test_large_graph_both_tile_sizes' batch 0"""
    toy = []
    for fan, B in [([1], 203), ([40], 100), ([64], 64), ([7, 1], 203), ([25, 10], 128), ([25, 10, 5], 64), ([5, 4, 3], 203), ([40, 3], 90), ([1, 1, 1, 1], 50), ([3, 64], 40)]:
        for seed in (0, 1):
            V, F = 500, 6
            indptr, indices, labels = X.random_graph(seed, V, holes=True)
            feats = np.random.RandomState(seed).rand(V, F).astype(np.float32)
            seeds = np.random.RandomState(seed + 9).permutation(V)[:203].astype(np.int32)
            if seed:
                seeds[7] = seeds[3]
            for counter in range(min(4, (len(seeds) + B - 1) // B)):
                toy.append((indptr, indices, feats, seeds, labels[seeds], B, counter, fan))
    V, F, B, fan = 1200000, 4, 4000, [25, 10, 5]
    indptr, indices, labels = X.random_graph(11, V, max_deg=40, hubs=50, hub_deg=5000)
    feats = np.zeros((V, F), np.float32)                     # the rows are copies: the draws decide
    seeds = np.random.RandomState(2).permutation(V)[:2 * B + 77].astype(np.int32)
    return dict(toy=toy, large=[(indptr, indices, feats, seeds, labels[seeds], B, 0, fan)])


def kills(inputs, name, statements):
    """does the mutant's batch differ from the statement's on one of `inputs` (run_batch argument tuples)?"""
    for k, a in enumerate(inputs):
        if k not in statements:
            statements[k] = D.run_batch(*a)
        if differs(statements[k], D.run_batch(*a, draw=X.mutant_draw(name, a[5], a[7]))):
            return True
    return False


def test_mutant_table(switch):
    """Every mutant draw against the statement under assert_batch_equal, over the former whole-batch inputs and over the new switch cases
    (batch 0 of each).  Every mutant must be killed by a new switch case, the tiled ones at the tile that case runs: "key in tile, 1024" is
    the statement on every hop that runs the 256-slot tile.  The table is printed (CHANGELOG.md holds it as found)."""
    g, cases = switch
    sets = former_inputs()
    for B, fan, tiles, straddling in X.SWITCH_CASES:
        seeds, batches = cases[(B, tuple(fan))]
        sets["B %d %s" % (B, fan)] = [(g["indptr"], g["indices"], g["feats"], seeds, g["labels"][seeds], B, 0, fan)]
    table = {}
    for col, inputs in sets.items():
        statements = {}
        for name in X.MUTANTS:
            table[(name, col)] = kills(inputs, name, statements)
    cols = list(sets)
    print("%-24s %s" % ("mutant", " | ".join(cols)))
    for name in X.MUTANTS:
        print("%-24s %s" % (name, " | ".join(("killed" if table[(name, c)] else "-").center(len(c)) for c in cols)))
    new = cols[2:]
    for name in X.MUTANTS:
        if name in X.EQUIVALENT:          # Floyd at d == f is take-all (distinctcases.mutant_take_all_below_f): nothing can tell it, and nothing does
            assert not any(table[(name, c)] for c in cols), name
        else:
            assert any(table[(name, c)] for c in new), "no new switch case tells %r from the statement" % name
    # a tiled mutant is the statement wherever its tile does not run: the kills above are at the tile the case runs
    for B, fan, tiles, straddling in X.SWITCH_CASES:
        for T in (256, 1024):
            if T not in tiles:
                assert not table[("key in tile, %d" % T, "B %d %s" % (B, fan))] and not table[("restart at edge, %d" % T, "B %d %s" % (B, fan))]
    # the restart needs rows across a tile edge: where none crosses (f = 64) it cannot be seen, where >= 50 cross it is
    for B, fan, tiles, straddling in X.SWITCH_CASES:
        col = "B %d %s" % (B, fan)
        assert any(table[("restart at edge, %d" % T, col)] for T in (256, 1024)) == bool(straddling), col
