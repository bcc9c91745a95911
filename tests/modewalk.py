"""A seeded walk over combinations of the pool's serving modes on ONE long-lived pool (tests/test_gpu_mode_walk.py runs it on the GPU,
tests/test_mode_walk_cpu.py proves on the CPU what it relies on).  A helper module like drawrulecases.py, not collected by pytest.

Every pull request that added a mode tested it against its NumPy statement and beside a few hand-picked neighbours.  This module runs
arbitrary sequences instead: every run_batch re-sets the pool's modes, the setters allocate per-pipe buffers lazily, progress flags gate
the launchers and the launch-size feedback survives from one mode to the next, so a leak shows as a step that differs from its statement
although the same step alone on a fresh engine does not.

  the lattice     Vector: rule, seed / round, edge_ids, edge_features, agg, presc, per_level, pipe, counter, driver.  valid() states the
                  rules the library documents (capi.Engine.run_batch's docstring), none of them read off the code under test.
  the statement   statement() restates no rule: eidref.run_batch (the alias rule: drawrulecases.statement over the alias rows the device
                  built) composed with distinctcases.expected_sums, edgeaggref.expected_nbr_sum_edge and efref.expected_edge_feat.
  the walk        walk(seed, steps): a deterministic list of valid vectors, each a partial re-draw of the one before it, so that most
                  steps change a few modes and keep the others.  assert_step() runs one and compares everything the vector hands over.

lp_draw stays out of the lattice: it needs a [src | pos | neg] training list, and with it another engine than the one every other mode
shares.  Graph, shape and seed list are drawrulecases.graph(), SHAPES["narrow"] (64 x [5, 4]) and seed_list("narrow"); every comparison is
array_equal, floats by bit pattern."""
import collections

import numpy as np

import drawrulecases as D
import eidref as R
import weightedref
from aggcases import assert_sum_bits
from distinctcases import expected_sums
from edgeaggref import expected_nbr_sum_edge
from efref import expected_edge_feat
from eidref import bits

TILE = "narrow"
B, FAN = D.SHAPES[TILE]
SEED = 7                                            # the seed of the seeded steps (wsharedcases.SEED, tests/test_gpu_edge_ids.py)
ALIAS = "weighted"                                  # the alias rule: weighted draws with replacement, which hand no edge ids over
RULES = R.RULES + (ALIAS,)
ENGINE_ARGS = dict(R.ENGINE_ARGS, weighted=D.ENGINE_ARGS[ALIAS])
AGGS = ("none", "sums", "norm", "edge_weight")      # the hand-off of the last hop: rows, plain sums, norm="both", sums scaled by edge_w
DRIVERS = ("run_batch", "replay")                   # replay: capture_batch, then run_graph for both counters
KINDS = ("whole", "clique", "exchange")             # the engine a walk runs on: whole CSR; fragments behind a filled cache; ... with LEGION_PEER_GATHER=exchange
SEEDINGS = ((None, 0), (SEED, 0), (SEED, 1))
STEPS = 24                                          # the steps of a default walk: coverage() holds over DEFAULT_WALKS seeds on every kind (at 16 the clique's walks miss two transitions)
DEFAULT_WALKS = 16                                  # the sibling stress tests' default; $LEGION_STRESS_WALK_N overrides it

Vector = collections.namedtuple("Vector", "rule seed round edge_ids edge_features agg presc per_level pipe counter driver")
OPTIONAL_KEYS = ("nbr_sum", "out_deg", "edge_ids", "edge_w", "edge_feat")


def rules_of(kind):
    """the rules an engine kind takes: partitioned engines read the clique's fragments, which only these rules' samplers do"""
    return RULES if kind == "whole" else R.PARTITIONED_RULES


def valid(v, kind="whole"):
    """None if the library documents the combination as one it serves on an engine of `kind`, else the reason it does not"""
    if v.rule not in RULES or v.agg not in AGGS or v.driver not in DRIVERS or v.pipe not in (0, 1) or v.counter not in D.COUNTERS:
        return "outside the lattice"
    if (v.seed, v.round) not in SEEDINGS:
        return "seed: None (round 0) or %d (round 0 or 1)" % SEED
    if v.rule not in rules_of(kind):
        return "partitioned engines take %s only" % (R.PARTITIONED_RULES,)
    if v.edge_features and not v.edge_ids:
        return "edge_features needs edge_ids: a row is gathered by the id the edge-id mode hands over"
    if v.edge_ids and v.rule == ALIAS:
        return "edge_ids is refused under the alias rule: the alias table holds the alias neighbour's id, not its column"
    if v.agg == "edge_weight" and not v.edge_ids:
        return "agg_edge_weight needs edge_ids: the sums are scaled by the edge_w that mode hands over"
    if v.presc and v.driver == "replay":
        return "a recorded graph is a training batch: capture_batch records no pre-sampling batch"
    if kind == "exchange" and v.agg != "none":
        return "LEGION_PEER_GATHER=exchange refuses the aggregated last hop: the exchange moves rows, not sums"
    return None


def hands_over(v):
    """The keys of Engine.result() a step leaves, beyond nc, ec, ids, labels and the COO arrays.  A pre-sampling batch hands over no rows, no
    sums and no ids, whatever its modes say; norm="both" excludes the edge-weighted sums by the lattice itself (agg is one value)."""
    if v.presc:
        return ()
    keys = ["features"]
    if v.agg != "none":
        keys.append("nbr_sum")
    if v.agg == "norm":
        keys.append("out_deg")
    if v.edge_ids:
        keys += ["edge_ids", "edge_w"]
    if v.edge_features:
        keys.append("edge_feat")
    return tuple(keys)


def engine_args(v):
    """how capi.Engine.run_batch / capture_batch are told the vector (without the counter, the driver and is_presc)"""
    kw = dict(ENGINE_ARGS[v.rule], seed=v.seed, round=v.round, edge_ids=v.edge_ids, edge_features=v.edge_features, per_level=v.per_level, pipe=v.pipe)
    if v.agg != "none":
        kw.update(agg_last_hop=True)
    if v.agg == "norm":
        kw.update(agg_norm="both")
    if v.agg == "edge_weight":
        kw.update(agg_edge_weight=True)
    return kw


# ---- the composed statement ------------------------------------------------------------------------------------------------------
def batch_statement(g, rule, counter, seed=None, round=0, alias=None, cache=None):
    """(the rule's batch, its near-tie rows), cached in `cache` by (rule, counter, seed, round): eidref.run_batch, and for the alias rule
    drawrulecases.statement (seeded: the same weightedref.run_batch behind weightedref.Statement's draw word and shuffled list)."""
    key = (rule, counter, seed, round)
    if cache is not None and key in cache:
        return cache[key]
    seeds, ties = D.seed_list(TILE), []
    lab = g["labels"][seeds]
    if rule != ALIAS:
        res = R.run_batch(g, rule, seeds, lab, B, counter, FAN, seed=seed, round=round, ties=ties)
    elif seed is None:
        res = D.statement(g, ALIAS, TILE, counter, alias=alias)
    else:
        res = weightedref.Statement(weightedref.Table(g["indptr"], g["indices"], *alias), g["feats"], B, FAN, seed=seed).run_batch(seeds, lab, counter, round=round)
    if cache is not None:
        cache[key] = (res, ties)
    return res, ties


def statement(g, X, v, alias=None, cache=None):
    """What the step `v` hands over, as a dict: batch (the rule's batch: nc, ec, ids, labels, COO, features, and edge_ids / edge_w where the
    rule has them), ties, and for the modes that are on n_in, nbr_sum, out_deg and edge_feat.  X: the engine's edge-feature table (None:
    no step gathers edge rows); alias: (thr, alias_id) for the alias rule; cache: a dict the caller keeps between calls."""
    batch, ties = batch_statement(g, v.rule, v.counter, v.seed, v.round, alias=alias, cache=cache)
    want = dict(batch=batch, ties=ties)
    if v.presc:
        return want
    key = (v.rule, v.counter, v.seed, v.round, v.agg)
    if v.agg != "none":
        if cache is not None and key in cache:
            sums = cache[key]
        else:
            if v.agg == "edge_weight":
                n_in, _, _, S = expected_nbr_sum_edge(batch, g["indptr"], g["indices"], FAN)
                sums = dict(n_in=n_in, nbr_sum=S)
            else:
                n_in, _, S, d = expected_sums(batch, FAN, v.agg == "norm")
                sums = dict(n_in=n_in, nbr_sum=S)
                if v.agg == "norm":
                    sums["out_deg"] = d
            if cache is not None:
                cache[key] = sums
        want.update(sums)
    if v.edge_features:
        want["edge_feat"] = expected_edge_feat(X, batch["edge_ids"])
    return want


# ---- the walk --------------------------------------------------------------------------------------------------------------------
def _draw(rng, prev, kind):
    """a vector: every field of `prev` is kept with probability 0.6 (None: all are drawn), then the fields that depend on others are
    brought into the lattice in the order the rules name them, without drawing anything again"""
    keep = (lambda: False) if prev is None else (lambda: rng.rand() < 0.6)
    rules = rules_of(kind)
    f = {}
    f["rule"] = prev.rule if keep() else rules[rng.randint(len(rules))]
    f["seed"], f["round"] = (prev.seed, prev.round) if keep() else SEEDINGS[rng.randint(len(SEEDINGS))]
    f["agg"] = prev.agg if keep() else AGGS[rng.randint(len(AGGS))]
    f["edge_ids"] = prev.edge_ids if keep() else bool(rng.randint(2))
    f["edge_features"] = prev.edge_features if keep() else bool(rng.randint(2))
    f["presc"] = False if keep() else bool(rng.rand() < 0.2)
    f["per_level"] = prev.per_level if keep() else bool(rng.randint(2))
    f["pipe"] = prev.pipe if keep() else int(rng.randint(2))
    f["counter"] = int(rng.randint(2))
    f["driver"] = DRIVERS[int(rng.rand() < 0.25)]
    if kind == "exchange":
        f["agg"] = "none"
    if f["rule"] == ALIAS:
        f["edge_ids"] = False
        if f["agg"] == "edge_weight":
            f["agg"] = "sums"
    if f["agg"] == "edge_weight":
        f["edge_ids"] = True
    if not f["edge_ids"]:
        f["edge_features"] = False
    if f["driver"] == "replay":
        f["presc"] = False
    return Vector(**f)


def walk(seed, steps=STEPS, kind="whole"):
    """`steps` valid vectors from np.random.RandomState(seed): the same list on every machine"""
    rng = np.random.RandomState(seed)
    out, prev = [], None
    while len(out) < steps:
        v = _draw(rng, prev, kind)
        assert valid(v, kind) is None, (v, valid(v, kind))
        out.append(v)
        prev = v
    return out


def coverage(walks):
    """What the walks contain, as sets and flags (tests/test_mode_walk_cpu.py states the condition over them).  A transition is a pair of
    CONSECUTIVE steps of one walk; the hand-off pairs count only between two steps on the same pipe that both hand sums or rows over."""
    c = dict(rules=set(), agg_pairs=set(), ef_off_on_off=False, eid_on_off_on=False, seeded_unseeded_seeded=False, unseeded_seeded_unseeded=False,
             presc_then_edge_features=False, replay_after_another_run_batch=False)
    for w in walks:
        c["rules"] |= {v.rule for v in w}
        for a, b in zip(w, w[1:]):
            if a.pipe == b.pipe and not a.presc and not b.presc:
                c["agg_pairs"].add((a.agg, b.agg))
            c["presc_then_edge_features"] |= a.presc and b.edge_features and not b.presc
            c["replay_after_another_run_batch"] |= a.driver == "run_batch" and b.driver == "replay" and a._replace(driver="replay") != b
        for a, b, d in zip(w, w[1:], w[2:]):
            ef = tuple(v.edge_features and not v.presc for v in (a, b, d))
            eid = tuple(v.edge_ids and not v.presc for v in (a, b, d))
            sd = tuple(v.seed is not None for v in (a, b, d))
            c["ef_off_on_off"] |= ef == (False, True, False)
            c["eid_on_off_on"] |= eid == (True, False, True)
            c["seeded_unseeded_seeded"] |= sd == (True, False, True)
            c["unseeded_seeded_unseeded"] |= sd == (False, True, False)
    return c


def missing(cov, kind="whole"):
    """what coverage() of the walks of an engine kind lacks of the condition: [] when it holds"""
    out = ["rule " + r for r in rules_of(kind) if r not in cov["rules"]]
    if kind != "exchange":
        out += ["hand-offs %s -> %s" % p for p in ((a, b) for a in AGGS for b in AGGS) if p not in cov["agg_pairs"]]
    out += [k for k, v in cov.items() if v is False]
    return out


# ---- one step against its statement ----------------------------------------------------------------------------------------------
def compare(v, want, got, where):
    """the engine's batch `got` against statement()'s `want`: everything the vector hands over, and none of the keys it does not"""
    from conftest import KEYS_NO_FEATURES, assert_batch_equal
    batch = want["batch"]
    assert want["ties"] == [], (where, want["ties"])                # the cap on near-tie rows is zero (tests/test_mode_walk_cpu.py)
    assert_batch_equal(batch, got, keys=KEYS_NO_FEATURES)
    handed = hands_over(v)
    for k in OPTIONAL_KEYS:
        assert (k in got) == (k in handed), "%s: result() %s %r (has %s)" % (where, "lacks" if k in handed else "holds", k, sorted(got))
    if v.presc:
        return
    F = batch["features"].shape[1]
    if v.agg == "none":
        assert got["features"].shape == batch["features"].shape, (where, got["features"].shape, batch["features"].shape)
        assert_batch_equal(dict(features=bits(batch["features"])), dict(features=bits(got["features"])), keys=("features",))
    else:
        n_in, S = want["n_in"], want["nbr_sum"]
        assert got["features"].shape == (n_in, F) and got["nbr_sum"].shape == S.shape, (where, got["features"].shape, got["nbr_sum"].shape, n_in, S.shape)
        assert_batch_equal(dict(features=bits(batch["features"][:n_in])), dict(features=bits(got["features"])), keys=("features",))
        assert_sum_bits(where, got["nbr_sum"], S)
    if v.agg == "norm":
        assert_batch_equal(dict(out_deg=want["out_deg"]), got, keys=("out_deg",))
    if v.edge_ids:
        assert got["edge_ids"].dtype == np.int64
        assert_batch_equal(batch, got, keys=("edge_ids",))
        assert_batch_equal(dict(edge_w=bits(batch["edge_w"])), dict(edge_w=bits(got["edge_w"])), keys=("edge_w",))
    if v.edge_features:
        assert got["edge_feat"].dtype == np.float32 and got["edge_feat"].shape == want["edge_feat"].shape, (where, got["edge_feat"].shape)
        assert_batch_equal(dict(edge_feat=bits(want["edge_feat"])), dict(edge_feat=bits(got["edge_feat"])), keys=("edge_feat",))


def assert_step(eng, v, want, dev=0):
    """Run the step on logical GPU `dev` of `eng` and compare it.  want: {counter: statement(.., v at that counter)} -- a run_batch step
    needs the vector's counter, a replay step both: it records with capture_batch, replays the other counter and then the vector's own,
    which is the batch the pipe holds afterwards."""
    kw = engine_args(v)
    if v.driver == "run_batch":
        eng.run_batch(dev, v.counter, is_presc=v.presc, **kw)
        compare(v, want[v.counter], eng.result(dev, pipe=v.pipe, with_features=not v.presc), "run_batch")
        return
    graph = eng.capture_batch(dev, **kw)
    for it in (1 - v.counter, v.counter):
        eng.run_graph(graph, it)
        compare(v._replace(counter=it), want[it], eng.result(dev, pipe=v.pipe), "replay of counter %d" % it)


def assert_pipe_still_holds(eng, dev, pipe, held):
    """the batch a pipe was left with by the last step that wrote it, read once more behind a step on the other pipe"""
    v, want = held
    compare(v, want, eng.result(dev, pipe=pipe, with_features=not v.presc), "pipe %d, read again behind a step on pipe %d" % (pipe, 1 - pipe))


def run_walk(eng, vectors, statement_of, fresh, dev=0, held=None, label=""):
    """Every step of `vectors` on `eng` through assert_step, and behind every step the OTHER pipe once more against the statement of the
    last step that wrote it.  statement_of(v): the composed statement; held: {(dev, pipe): (vector, statement)} kept between walks on one
    engine.  On a mismatch -- an AssertionError, never an error the library or the runtime raised: behind a fault nothing more is started
    -- `fresh()` builds a new engine, the one vector runs alone on it, and the message names the label, the step, the previous vector and
    which of the two it was.  Nothing is run a second time on the engine that failed."""
    held = {} if held is None else held
    for i, v in enumerate(vectors):
        want = {it: statement_of(v._replace(counter=it)) for it in ((0, 1) if v.driver == "replay" else (v.counter,))}
        try:
            assert_step(eng, v, want, dev)
            held[(dev, v.pipe)] = (v._replace(driver="run_batch"), want[v.counter])
            if (dev, 1 - v.pipe) in held:
                assert_pipe_still_holds(eng, dev, 1 - v.pipe, held[(dev, 1 - v.pipe)])
        except AssertionError as ex:
            other = fresh()
            try:
                assert_step(other, v, want, dev)
                finding = "fresh engine agrees: state left by the previous step"
            except AssertionError as again:
                finding = "fresh engine differs too: the combination itself (%s)" % str(again)[:300]
            finally:
                other.close()
            raise AssertionError("%s, step %d, device %d: %s\n  vector   %s\n  previous %s\n  %s" % (label, i, dev, finding, v, vectors[i - 1] if i else None, ex)) from ex
    return held
