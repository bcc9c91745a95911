"""What tests/test_gpu_mode_walk.py relies on, proved without a device (tests/modewalk.py): valid() accepts what the existing GPU tests run
and rejects what the library documents as refused; no statement a default walk can ask for has a near-tie row, so the cap is zero; the
composed statement with a single mode on IS that mode's statement; and the default walks contain every transition the walk exists for --
a condition on the walks, not a measurement of them."""
import os

import numpy as np
import pytest

import drawrulecases as D
import eidref as R
import modewalk as M
import weightedref
from distinctcases import expected_sums
from edgeaggref import expected_nbr_sum_edge
from efref import expected_edge_feat
from eidref import bits

WALKS = int(os.environ.get("LEGION_STRESS_WALK_N", str(M.DEFAULT_WALKS)))
PLAIN_VECTOR = M.Vector(rule="stream", seed=None, round=0, edge_ids=False, edge_features=False, agg="none", presc=False, per_level=True, pipe=0, counter=0,
                        driver="run_batch")
DIM = 3


@pytest.fixture(scope="module")
def g():
    return D.graph()


@pytest.fixture(scope="module")
def X(g):
    import legion1_amd.synth as S
    return S.edge_features(0, len(g["indices"]), DIM)


@pytest.fixture(scope="module")
def alias(g):
    """a valid alias table of the graph (Vose's algorithm on the host; the GPU test takes the table the device built: any valid table is a statement)"""
    return weightedref.build_table(g["indptr"], g["indices"], g["w"])


@pytest.fixture(scope="module")
def cache():
    return {}


def vector_of(rule, is_presc=False, **kw):
    """the vector of a run_batch call as the GPU tests write it: a rule and capi.Engine.run_batch's keyword arguments"""
    agg = "none"
    if kw.get("agg_last_hop"):
        agg = "edge_weight" if kw.get("agg_edge_weight") else "norm" if kw.get("agg_norm") else "sums"
    v = PLAIN_VECTOR._replace(rule=rule, edge_ids=bool(kw.get("edge_ids")), edge_features=bool(kw.get("edge_features")), agg=agg, presc=is_presc,
                              seed=kw.get("seed"), round=kw.get("round", 0))
    told = M.engine_args(v)
    assert all(told[k] == x for k, x in dict(kw, **M.ENGINE_ARGS[rule]).items()), (v, told, kw)     # the vector tells the engine what the test told it
    return v


# ---- validity --------------------------------------------------------------------------------------------------------------------
def test_the_rules_are_told_to_the_engine_as_the_existing_tests_tell_them():
    assert all(M.ENGINE_ARGS[r] == R.ENGINE_ARGS[r] for r in R.RULES) and M.ENGINE_ARGS[M.ALIAS] == D.ENGINE_ARGS["weighted"]
    assert M.ENGINE_ARGS["shared"] == dict(sample="distinct", shared_draws=True)
    assert M.ENGINE_ARGS["wshared"] == dict(sample="weighted", weighted_distinct=True, shared_draws=True)
    assert set(M.RULES) == set(R.RULES) | set(D.RULES) and M.rules_of("clique") == M.rules_of("exchange") == R.PARTITIONED_RULES


def test_valid_accepts_every_combination_the_existing_gpu_tests_run():
    import test_gpu_agg_edge_weight as EW
    import test_gpu_edge_ids as EID
    ran = []
    for rule, kind in EID.COMBOS:                                    # tests/test_gpu_edge_ids.py: every rule of eidref.ENGINE_ARGS with ids on
        ran.append((vector_of(rule, edge_ids=True), "clique" if kind == "partitioned" else "whole"))
    assert {r for r, _ in EID.COMBOS} == set(R.ENGINE_ARGS)
    for rule, kind in D.COMBOS:                                      # tests/test_gpu_draw_rules.py: plain, pre-sampling and partitioned hops
        ran.append((vector_of(rule, is_presc=kind == "presc"), "clique" if kind == "partitioned" else "whole"))
    for rule in R.RULES:                                             # tests/test_gpu_agg_edge_weight.py: ON and PLAIN under every rule with ids, seeded too
        for kw in (EW.ON, EW.PLAIN):
            ran.append((vector_of(rule, **kw), "whole"))
            ran.append((vector_of(rule, seed=M.SEED, round=1, **kw), "whole"))
    for rule in R.PARTITIONED_RULES:
        ran.append((vector_of(rule, **EW.ON), "clique"))
    ran.append((vector_of("distinct", agg_last_hop=True, agg_norm="both", edge_ids=True), "whole"))      # tests/test_gpu_deep_tiles.py
    ran.append((vector_of("distinct", edge_ids=True, edge_features=True), "clique"))                      # tests/test_gpu_edge_features.py
    assert len(ran) > 40
    for v, kind in ran:
        assert M.valid(v, kind) is None, (v, kind, M.valid(v, kind))
        for driver in M.DRIVERS:
            for pipe in (0, 1):
                for per_level in (False, True):
                    w = v._replace(driver=driver, pipe=pipe, per_level=per_level, counter=1)
                    assert (M.valid(w, kind) is None) == (not (v.presc and driver == "replay")), w


def test_valid_rejects_each_documented_refusal():
    ok = PLAIN_VECTOR._replace(edge_ids=True)
    assert M.valid(ok) is None
    assert "edge_features needs edge_ids" in M.valid(PLAIN_VECTOR._replace(edge_features=True))
    assert "refused under the alias rule" in M.valid(ok._replace(rule=M.ALIAS))
    assert "refused under the alias rule" in M.valid(ok._replace(rule=M.ALIAS, agg="edge_weight"))
    assert "agg_edge_weight needs edge_ids" in M.valid(PLAIN_VECTOR._replace(agg="edge_weight"))
    assert M.valid(ok._replace(agg="edge_weight")) is None
    for v in (ok._replace(agg=a) for a in M.AGGS):                   # a norm and the edge-weighted sums exclude each other: agg is ONE value
        told = M.engine_args(v)
        assert not (told.get("agg_norm") and told.get("agg_edge_weight")) and bool(told.get("agg_last_hop")) == (v.agg != "none")
    for rule in M.RULES:
        assert (M.valid(PLAIN_VECTOR._replace(rule=rule), "clique") is None) == (rule in R.PARTITIONED_RULES)
        assert M.valid(PLAIN_VECTOR._replace(rule=rule), "whole") is None
    assert "capture_batch records no pre-sampling batch" in M.valid(PLAIN_VECTOR._replace(presc=True, driver="replay"))
    for agg in M.AGGS[1:]:
        assert "exchange refuses the aggregated last hop" in M.valid(ok._replace(agg=agg), "exchange")
    assert M.valid(ok, "exchange") is None
    for bad in (dict(rule="lp_draw"), dict(seed=8), dict(seed=None, round=1), dict(round=2, seed=M.SEED), dict(pipe=2), dict(counter=2), dict(agg="both"), dict(driver="served")):
        assert M.valid(PLAIN_VECTOR._replace(**bad)) is not None, bad


def test_a_presampling_batch_hands_over_no_ids_no_rows_and_no_sums():
    everything = PLAIN_VECTOR._replace(edge_ids=True, edge_features=True, agg="edge_weight")
    assert M.hands_over(everything) == ("features", "nbr_sum", "edge_ids", "edge_w", "edge_feat")
    assert M.hands_over(everything._replace(agg="norm")) == ("features", "nbr_sum", "out_deg", "edge_ids", "edge_w", "edge_feat")
    assert M.hands_over(PLAIN_VECTOR) == ("features",)
    assert M.valid(everything._replace(presc=True)) is None and M.hands_over(everything._replace(presc=True)) == ()


# ---- near ties -------------------------------------------------------------------------------------------------------------------
def test_no_statement_a_walk_can_ask_for_has_a_near_tie_row(g, cache):
    """30 statements: every rule with a statement of its own on the host x both counters x unseeded, (7, 0), (7, 1).  The cap is zero."""
    n = 0
    for rule in R.RULES:
        for it in D.COUNTERS:
            for seed, rnd in M.SEEDINGS:
                res, ties = M.batch_statement(g, rule, it, seed, rnd, cache=cache)
                assert ties == [], (rule, it, seed, rnd, ties)
                assert int(res["ec"][2 + len(M.FAN)]) > 300
                n += 1
    assert n == 30
    asked = {(v.rule, v.seed, v.round) for kind in M.KINDS for s in range(WALKS) for v in M.walk(s, kind=kind)}
    assert asked <= {(r, s, rnd) for r in M.RULES for s, rnd in M.SEEDINGS}


# ---- composition -----------------------------------------------------------------------------------------------------------------
def same_batch(a, b):
    assert set(a) == set(b)
    for k in ("nc", "ec", "ids", "labels", "src_off", "dst_off", "edge_ids"):
        if k in a:
            assert np.array_equal(a[k], b[k]), k
    for k in ("features", "edge_w"):
        if k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("rule", R.RULES)
def test_with_no_mode_on_the_statement_is_the_rules_batch(g, X, cache, rule):
    seeds = D.seed_list(M.TILE)
    for it in D.COUNTERS:
        for seed, rnd in M.SEEDINGS:
            v = PLAIN_VECTOR._replace(rule=rule, counter=it, seed=seed, round=rnd)
            want = M.statement(g, X, v, cache=cache)
            assert sorted(want) == ["batch", "ties"]
            same_batch(want["batch"], R.run_batch(g, rule, seeds, g["labels"][seeds], M.B, it, M.FAN, seed=seed, round=rnd))
            assert M.statement(g, X, v._replace(pipe=1, per_level=False, driver="replay"), cache=cache)["batch"] is want["batch"]      # computed once, shared
            assert sorted(M.statement(g, X, v._replace(presc=True, edge_ids=True, agg="sums"), cache=cache)) == ["batch", "ties"]


def test_the_alias_rules_statement_is_drawrulecases(g, X, alias, cache):
    for it in D.COUNTERS:
        v = PLAIN_VECTOR._replace(rule=M.ALIAS, counter=it)
        same_batch(M.statement(g, X, v, alias=alias, cache=cache)["batch"], D.statement(g, "weighted", M.TILE, it, alias=alias))
        seeded = M.statement(g, X, v._replace(seed=M.SEED, round=1), alias=alias, cache=cache)["batch"]
        assert not np.array_equal(seeded["labels"], D.statement(g, "weighted", M.TILE, it, alias=alias)["labels"])      # the round's shuffled list


@pytest.mark.parametrize("rule", ["stream", "wdistinct", "shared"])
def test_each_mode_alone_is_its_own_statement(g, X, cache, rule):
    for it in D.COUNTERS:
        base = PLAIN_VECTOR._replace(rule=rule, counter=it)
        batch = M.statement(g, X, base, cache=cache)["batch"]
        for agg in ("sums", "norm"):
            want = M.statement(g, X, base._replace(agg=agg), cache=cache)
            n_in, N, S, d = expected_sums(batch, M.FAN, agg == "norm")
            assert sorted(want) == sorted(["batch", "ties", "n_in", "nbr_sum"] + (["out_deg"] if agg == "norm" else []))
            assert want["batch"] is batch and want["n_in"] == n_in and N > 0 and np.array_equal(bits(want["nbr_sum"]), bits(S))
            assert agg == "sums" or np.array_equal(want["out_deg"], d)
        want = M.statement(g, X, base._replace(agg="edge_weight", edge_ids=True), cache=cache)
        n_in, N, _, S = expected_nbr_sum_edge(batch, g["indptr"], g["indices"], M.FAN)
        assert sorted(want) == ["batch", "n_in", "nbr_sum", "ties"] and want["n_in"] == n_in and np.array_equal(bits(want["nbr_sum"]), bits(S))
        assert not np.array_equal(bits(S), bits(expected_sums(batch, M.FAN, False)[2]))                 # the three hand-offs are three statements
        want = M.statement(g, X, base._replace(edge_ids=True, edge_features=True), cache=cache)
        assert sorted(want) == ["batch", "edge_feat", "ties"] and want["edge_feat"].shape == (len(batch["src_off"]), DIM)
        assert np.array_equal(bits(want["edge_feat"]), bits(expected_edge_feat(X, batch["edge_ids"])))


# ---- the walk --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", M.KINDS)
def test_a_walk_is_deterministic_and_every_step_is_valid(kind):
    for s in range(WALKS):
        w = M.walk(s, kind=kind)
        assert w == M.walk(s, kind=kind) and len(w) == M.STEPS and all(M.valid(v, kind) is None for v in w)
        assert all(type(x) in (str, int, bool, type(None)) for v in w for x in v)
    assert M.walk(0) != M.walk(1)


@pytest.mark.parametrize("kind", M.KINDS)
def test_the_default_walks_cover_what_the_walk_exists_for(kind):
    """The condition: every rule; every ordered pair of hand-offs as consecutive steps on one pipe; edge features off -> on -> off; edge
    ids on -> off -> on; seeded -> unseeded and back, both ways; a pre-sampling step directly before a step with edge features; a replay
    directly after a run_batch of another vector.  (The exchange engine hands over rows only: no hand-off pairs there.)  Stated over the
    default seeds, whatever $LEGION_STRESS_WALK_N says."""
    cov = M.coverage([M.walk(s, kind=kind) for s in range(M.DEFAULT_WALKS)])
    assert M.missing(cov, kind) == []
    assert kind == "exchange" or len(cov["agg_pairs"]) == len(M.AGGS) ** 2
    assert M.missing(M.coverage([M.walk(0, 4, kind)]), kind) != []                                      # the condition can fail: four steps do not hold it


# ---- the comparison and the diagnosis, against an engine made of statements --------------------------------------------------------
class StatementEngine:
    """capi.Engine's run_batch / capture_batch / run_graph / result / close answered from the statements: what a correct engine hands over.
    leak: a function (previous vector or None, vector, result dict) that spoils a result the way a state leak would."""

    def __init__(self, g, X, cache, leak=None):
        self.g, self.X, self.cache, self.leak, self.pipes, self.prev, self.closed = g, X, cache, leak, {}, None, False

    def _serve(self, dev, v):
        want = M.statement(self.g, self.X, v, cache=self.cache)
        got = {k: np.array(want["batch"][k]) for k in ("nc", "ec", "ids", "labels", "src_off", "dst_off")}
        handed = M.hands_over(v)
        if "features" in handed:
            got["features"] = np.array(want["batch"]["features"][:want["n_in"]] if v.agg != "none" else want["batch"]["features"])
        for k in ("nbr_sum", "out_deg", "edge_feat"):
            if k in handed:
                got[k] = np.array(want[k])
        for k in ("edge_ids", "edge_w"):
            if k in handed:
                got[k] = np.array(want["batch"][k])
        if self.leak is not None:
            self.leak(self.prev, v, got)
        self.pipes[(dev, v.pipe)], self.prev = got, v

    def run_batch(self, dev, counter, is_presc=False, **kw):
        rule = [r for r in M.RULES if all(kw.get(k, False) == x for k, x in dict(dict(sample="replace", weighted_distinct=False, shared_draws=False), **M.ENGINE_ARGS[r]).items())]
        assert len(rule) == 1, kw
        v = vector_of(rule[0], is_presc=is_presc, **{k: x for k, x in kw.items() if k not in ("pipe", "per_level", "sample", "weighted_distinct", "shared_draws")})
        self._serve(dev, v._replace(pipe=kw["pipe"], per_level=kw["per_level"], counter=counter))

    def capture_batch(self, dev, **kw):
        return (dev, kw)

    def run_graph(self, handle, counter):
        self.run_batch(handle[0], counter, **handle[1])

    def result(self, dev=0, pipe=0, with_features=True):
        got = dict(self.pipes[(dev, pipe)])
        if not with_features:
            got.pop("features", None)
        return got

    def close(self):
        self.closed = True


def test_compare_tells_every_key_a_vector_hands_over(g, X, cache):
    v = PLAIN_VECTOR._replace(rule="distinct", edge_ids=True, edge_features=True, agg="norm")
    eng = StatementEngine(g, X, cache)
    want = {0: M.statement(g, X, v, cache=cache)}
    M.assert_step(eng, v, want)
    good = eng.result(0, 0)
    assert sorted(good) == sorted(("nc", "ec", "ids", "labels", "src_off", "dst_off") + M.hands_over(v))
    for k in good:
        bad = dict(good)
        bad[k] = good[k].copy()
        flat = bad[k].reshape(-1).view(np.uint32 if bad[k].dtype == np.float32 else bad[k].dtype)
        flat[len(flat) // 2] ^= 1                                    # one bit of one word
        with pytest.raises(AssertionError):
            M.compare(v, want[0], bad, k)
        if k in M.OPTIONAL_KEYS:
            with pytest.raises(AssertionError, match="result\\(\\) lacks %r" % k):
                M.compare(v, want[0], {x: y for x, y in good.items() if x != k}, k)
    plain = M.statement(g, X, PLAIN_VECTOR, cache=cache)
    eng.run_batch(0, 0, **M.engine_args(PLAIN_VECTOR))
    with pytest.raises(AssertionError, match="result\\(\\) holds 'edge_ids'"):
        M.compare(PLAIN_VECTOR, plain, dict(eng.result(0, 0), edge_ids=good["edge_ids"]), "stale key")


def test_a_whole_walk_on_an_engine_made_of_statements_and_both_findings(g, X, alias, cache):
    """every default walk of the whole-CSR kind passes on an engine that hands over the statements -- the driver, the replays and the second
    read of the other pipe agree with statement() --; a leak behind a particular previous step is reported as state, with the seed, the step
    and the previous vector; a combination that is wrong on any engine as the combination itself; and an error that is no mismatch is not
    followed by a fresh engine"""
    st = lambda v: M.statement(g, X, v, alias=alias, cache=cache)      # noqa: E731
    cache.update({(M.ALIAS, it, s, r): M.batch_statement(g, M.ALIAS, it, s, r, alias=alias) for it in D.COUNTERS for s, r in M.SEEDINGS})
    built = []

    def fresh(leak=None):
        built.append(StatementEngine(g, X, cache, leak))
        return built[-1]

    eng, held = StatementEngine(g, X, cache), {}
    for s in range(WALKS):
        M.run_walk(eng, M.walk(s), st, fresh, held=held, label="walk %d" % s)
    assert built == [] and sorted(held) == [(0, 0), (0, 1)]
    w = M.walk(3)
    i = next(i for i in range(1, len(w)) if w[i].edge_ids and not w[i].presc and w[i - 1].agg != "none" and not w[i - 1].presc)

    def stale_weights(prev, v, got):                                 # edge_w of a step behind an aggregated one keeps a word of the batch before
        if prev is not None and prev.agg != "none" and not prev.presc and "edge_w" in got:
            got["edge_w"][0] += 1
    with pytest.raises(AssertionError) as ex:
        M.run_walk(StatementEngine(g, X, cache, stale_weights), w, st, fresh, label="walk 3")
    msg = str(ex.value)
    assert "walk 3, step %d, device 0: fresh engine agrees: state left by the previous step" % i in msg and str(w[i]) in msg and str(w[i - 1]) in msg and "edge_w" in msg
    assert len(built) == 1 and built[0].closed

    def wrong_ids(prev, v, got):                                     # wrong whatever came before
        if "edge_ids" in got:
            got["edge_ids"][-1] += 1
    j = next(j for j in range(len(w)) if w[j].edge_ids and not w[j].presc)
    with pytest.raises(AssertionError, match="walk 3, step %d, device 0: fresh engine differs too: the combination itself" % j):
        M.run_walk(StatementEngine(g, X, cache, wrong_ids), w, st, lambda: fresh(wrong_ids), label="walk 3")
    assert len(built) == 2 and built[1].closed

    def fault(prev, v, got):
        raise RuntimeError("an illegal memory access was encountered")
    with pytest.raises(RuntimeError):
        M.run_walk(StatementEngine(g, X, cache, fault), w, st, fresh, label="walk 3")
    assert len(built) == 2                                           # nothing more was started
