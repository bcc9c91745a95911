"""The adversarial inputs of tests/aggcases.py, proven on the CPU: what tests/test_gpu_agg_adversarial.py sends through the GPU is not vacuous.

Everything here runs on the C oracle's DEFAULT-mode batches and the NumPy statements of tests/aggref.py / tests/gcnref.py.  The batches are
the ones the GPU test `test_special_values_through_the_sums` uses (the same adversarial_case, fan-outs and batch size), so the class
coverage, the two caps and the mutant table are statements about that test's inputs."""
import numpy as np
import pytest

import aggcases as A
from gcnref import block_out_degree

CASE_V, CASE_SEED, CASE_B, CASE_SEEDS, CASE_FANS, CASE_BATCHES = A.CASE_V, A.CASE_SEED, A.CASE_B, A.CASE_SEEDS, A.CASE_FANS, A.CASE_BATCHES


def case_batches(oracle, F, fan, table=None):
    """(case, [(ref, x)]) of the shared case: x = table[ids], the rows by batch position"""
    c = A.adversarial_case(CASE_V, F, CASE_SEED, n_seeds=CASE_SEEDS)
    table = c["table"] if table is None else table
    orc = oracle.OracleRunner(c["indptr"], c["indices"], table, c["V"], F, CASE_B, fan)
    out = []
    for it in CASE_BATCHES:
        ref = orc.run_batch(c["seeds"], c["labels"][c["seeds"]], it)
        assert (ref["ids"] >= 0).all()
        A.assert_words_equal("the oracle's own gather", ref["features"], table[ref["ids"]])       # the oracle copies rows word for word
        out.append((ref, table[ref["ids"]]))
    return c, out


def test_host_keeps_subnormals():
    """A library that switches the host to flush-to-zero (some do, through the MXCSR of the thread that loads them) would silently turn
    the reference into the flush-to-zero mutant.  Checked again at the end of every test below that relies on it."""
    assert np.float32(1e-39) * np.float32(0.5) != 0
    assert np.float32(1e-39) + np.float32(1e-39) == np.float32(2e-39)
    a = np.full(64, 1e-39, np.float32)                       # the vector paths NumPy's array arithmetic takes
    assert ((a * np.float32(0.5)) != 0).all() and ((a + a) != 0).all()


def test_adversarial_table_has_every_class_in_its_place():
    for F in (1, 2, 7, 8, 36, 128):
        hubs = np.arange(0, 4000, 97)
        t, cls = A.adversarial_features(4000, F, 5, keep_out=hubs)
        c_inf, c_nan = A.special_columns(F)
        count = np.bincount(cls, minlength=len(A.CLASSES))
        assert (count > 0).all(), dict(zip(A.CLASSES, count))
        assert 0.015 < (count[A.INF] + count[A.NAN]) / 4000 < 0.035                 # about 2.5 % of the rows are non-finite
        assert set(cls[hubs].tolist()) <= {A.WIDE, A.SUBNORMAL}                       # no hub in a special class
        finite = np.isfinite(t)
        assert finite[~np.isin(cls, (A.INF, A.NAN))].all()
        other = np.ones(F, bool)
        other[[c_inf, c_nan]] = False
        assert finite[:, other].all()                                                 # non-finite values in two columns only
        assert np.isinf(t[cls == A.INF, c_inf]).all() and {-np.inf, np.inf} <= set(t[cls == A.INF, c_inf].tolist())
        w = t.view(np.uint32)[cls == A.NAN, c_nan]
        assert np.isnan(t[cls == A.NAN, c_nan]).all() and (w & 0x00400000).any() and not (w & 0x00400000).all()   # quiet and signalling
        sub = t[cls == A.SUBNORMAL]
        assert ((sub != 0) & (np.abs(sub) < A.TINY)).mean() > 0.5
        assert (np.abs(t[cls == A.BIG]) == A.BIG_VALUE).all() and (t[cls == A.NEGZERO].view(np.uint32) == 0x80000000).all()
        assert np.float32(A.BIG_VALUE) + np.float32(A.BIG_VALUE) == np.inf
        t2, cls2 = A.adversarial_features(4000, F, 5, keep_out=hubs)
        assert np.array_equal(t.view(np.uint32), t2.view(np.uint32)) and np.array_equal(cls, cls2)
    b = A.bit_pattern_features(5000, 8, 3)
    assert b.dtype == np.float32 and np.isnan(b).any() and ((b != 0) & (np.abs(b) < A.TINY)).any()
    words = b.view(np.uint32)
    assert ((words & 0x7FC00000) == 0x7F800000).any() and ((words >> 31) == 1).mean() > 0.4           # signalling NaNs or infinities; both signs


def test_assert_sum_bits_fails_where_it_must():
    want = np.array([[0.0, -np.inf, np.nan, 1.5, 1e-40]], np.float32)
    A.assert_sum_bits("same", want.copy(), want)
    other_nan = want.copy()
    other_nan.view(np.uint32)[0, 2] = 0xFFC01234                                  # another payload, another sign: still a NaN
    A.assert_sum_bits("payload", other_nan, want)
    for col, value in ((0, -0.0), (1, np.inf), (2, 1.0), (2, np.inf), (3, np.nan), (4, 0.0), (3, np.float32(1.5000001))):
        bad = want.copy()
        bad[0, col] = value
        with pytest.raises(AssertionError):
            A.assert_sum_bits("col %d" % col, bad, want)
    with pytest.raises(AssertionError):
        A.statement_caps("-0.0", np.array([1.0, -0.0], np.float32))
    with pytest.raises(AssertionError):
        A.statement_caps("NaN", np.array([np.nan] + [1.0] * 18, np.float32))      # 5.3 %
    assert A.statement_caps("ok", np.array([np.nan] + [1.0] * 19, np.float32)) == 0.05
    with pytest.raises(AssertionError):
        A.assert_words_equal("zero", np.array([0.0], np.float32), np.array([-0.0], np.float32))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fan", CASE_FANS, ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("F", [8, 128, 7, 36])
def test_class_coverage_and_caps(oracle, F, fan, weighted):
    """On the batches the GPU test uses, the statement holds at least one element of every class of aggcases.RESULT_CLASSES -- a subnormal
    result, an infinity by overflow of finite inputs, an infinity from an infinite input, a NaN from a NaN input, a NaN from inf - inf --
    and stays under the NaN cap without a -0.0 word."""
    c, batches = case_batches(oracle, F, fan)
    seen = dict.fromkeys(A.RESULT_CLASSES, 0)
    shares = []
    for ref, x in batches:
        S = A.statement(ref, c["indptr"], c["indices"], fan, x=x, weighted=weighted)
        shares.append(A.statement_caps("fan %s" % fan, S))
        for k, v in A.result_classes(ref, c["indptr"], c["indices"], fan, S, x=x).items():
            seen[k] += v
    print("F %d fan %s %s: NaN share %s, %s" % (F, fan, "weighted" if weighted else "plain", ["%.2f %%" % (100 * s) for s in shares], seen))
    assert all(v > 0 for v in seen.values()), seen
    assert np.float32(1e-39) * np.float32(0.5) != 0


ONE_CLASS_TABLES = ("normal", "wide", "subnormal", "big", "negzero", "adversarial")


def kill_table(oracle, F, fan):
    """{(mutant, form): {table: killed}} on the shared case: `normal` is the standard_normal table the former tests use, the four one-class
    tables hold rows of one finite class only, `adversarial` is the GPU test's table."""
    c = A.adversarial_case(CASE_V, F, CASE_SEED, n_seeds=CASE_SEEDS)
    tables = dict(normal=np.random.RandomState(F).standard_normal((CASE_V, F)).astype(np.float32), adversarial=c["table"])
    for name in ("wide", "subnormal", "big", "negzero"):
        tables[name] = A.adversarial_features(CASE_V, F, CASE_SEED + 1, only=name)[0]
    out = {}
    for tname in ONE_CLASS_TABLES:
        _, batches = case_batches(oracle, F, fan, table=tables[tname])
        for weighted in (False, True):
            form = "weighted" if weighted else "plain"
            wants = [A.statement(ref, c["indptr"], c["indices"], fan, x=x, weighted=weighted) for ref, x in batches]
            for mname, (fn, forms) in A.MUTANTS.items():
                if form not in forms:
                    continue
                killed = any(A.differs(mname, fn(ref, c["indptr"], c["indices"], fan, x=x, weighted=weighted), want)
                             for (ref, x), want in zip(batches, wants))
                out.setdefault((mname, form), {})[tname] = killed
    return out


@pytest.mark.parametrize("fan", [[10], [4, 10], [3, 2, 3], [3, 25]], ids=lambda f: "-".join(map(str, f)))
def test_every_mutant_is_killed_by_the_new_inputs(oracle, fan):
    """Every wrong implementation of aggcases.MUTANTS differs from the statement under assert_sum_bits on the adversarial table, in both
    forms it applies to (`fma` and `rsq` are the statement itself without weights).  Which class does it:
      reversed, pairwise, float64, fma   by any table whose adds or products round: normal, wide and the adversarial one; NOT by a table of
                                         -0.0 rows (every sum is +0.0) -- and float64 accumulation is also what keeps a run of +-3e38 finite
      pairwise                           likewise, at a last fan-out >= 4 only: a tree over three terms IS (a + b) + c
      rsq                                by any table with nonzero finite rows (the weights differ, so the first product does)
      ftz                                NOT by the standard_normal table of the former tests, nor by wide / big / -0.0 rows: only the
                                         subnormal rows, alone or inside the adversarial table, tell it from the statement."""
    F = 8
    table = kill_table(oracle, F, fan)
    print("fan %s, F %d: mutant (form) -> killed by" % (fan, F))
    for (m, form), row in sorted(table.items()):
        print("  %-9s %-8s %s" % (m, form, "  ".join("%s:%s" % (t, "yes" if row[t] else "no") for t in ONE_CLASS_TABLES)))
    if fan[-1] < 4:
        assert not any(any(table.pop(("pairwise", form)).values()) for form in ("plain", "weighted"))
    for key, row in table.items():
        assert row["adversarial"], (key, row)
        assert not row["negzero"], (key, row)
    for form in ("plain", "weighted"):
        ftz = table[("ftz", form)]
        assert not ftz["normal"] and not ftz["wide"] and not ftz["big"], ftz        # the documented gap: the former inputs cannot see it
        assert ftz["subnormal"] and ftz["adversarial"], ftz
        for m in ("reversed", "pairwise", "float64"):
            if (m, form) not in table:
                continue
            assert table[(m, form)]["normal"] and table[(m, form)]["wide"], (m, form, table[(m, form)])
    assert table[("fma", "weighted")]["normal"] and table[("rsq", "weighted")]["normal"]
    assert np.float32(1e-39) * np.float32(0.5) != 0


def test_once_rounded_weight_differs_where_the_star_test_looks():
    """w = fl(1 / fl(sqrt(d))) (two roundings: the contract) against fl(1 / sqrt(d)) rounded once (what an rsq-style instruction
    approximates): they differ for 242 of the d in [1, 1024] -- every one of which the star test realises -- and 15 047 of [1, 65535]."""
    def count(hi):
        d = np.arange(1, hi + 1)
        twice = np.float32(1) / np.sqrt(d.astype(np.float32))
        once = (1.0 / np.sqrt(d.astype(np.float64))).astype(np.float32)
        assert twice.dtype == np.float32
        return int((twice != once).sum())
    assert count(1024) == 242 and count(65535) == 15047


STAR_E, star_edge_case = A.STAR_E, A.star_edge_case


def check_star_batch(oracle_runner, g, counter, feats):
    """realised == intended: returns (ref, d)"""
    ref = oracle_runner.run_batch(g["seeds"], np.zeros(len(g["seeds"]), np.int32), counter)
    d, _ = block_out_degree(ref, g["fan"])
    want = g["want"][counter]
    intended = np.array([want.get(int(v), 0) for v in ref["ids"]], np.int64)
    assert np.array_equal(d, intended), (counter, np.flatnonzero(d != intended)[:5])
    assert set(want) <= set(ref["ids"].tolist())
    return ref, d


@pytest.mark.parametrize("hops", [1, 2])
def test_star_graph_realises_the_intended_degrees(oracle, hops):
    """Through the oracle: every batch position's out-degree is the intended one, for the edge-count cases (E is the batch's edge count,
    the grouped batch is one run, the round-robin batch has no two equal neighbours) and for the coverage graph in both arrangements
    (every d in [1, 1024], one d >= 50 000, a self-targeting input, runs that start and end on every side of a wave and a workgroup edge)."""
    for E in STAR_E:
        g = star_edge_case(E, hops)
        feats = np.zeros((g["V"], 1), np.float32)
        orc = oracle.OracleRunner(g["indptr"], g["indices"], feats, g["V"], 1, g["B"], g["fan"])
        for counter in (0, 1):
            ref, d = check_star_batch(orc, g, counter, feats)
            assert int(ref["ec"][2 + hops]) == E and int(d.sum()) == E
            last = ref["src_off"][(g["B"] if hops == 2 else 0):]
            _, length = A.equal_runs(last)
            if counter == 0:
                assert len(length) <= 1 and (hops == 2 or int(d.max()) == E)          # one position receives every last-hop edge
            else:
                assert (length == 1).all()
    f, B = 25, 2100
    for arrangement in ("grouped", "round_robin"):
        g = A.star_graph(A.coverage_batches(f, B, np.random.RandomState(4)), f, B, arrangement, hops=hops, self_target=7, seed=9)
        feats = np.zeros((g["V"], 1), np.float32)
        orc = oracle.OracleRunner(g["indptr"], g["indices"], feats, g["V"], 1, B, g["fan"])
        seen, longest, starts, ends, lengths = set(), 0, set(), set(), []
        for counter in range(len(g["want"])):
            ref, d = check_star_batch(orc, g, counter, feats)
            seen |= set(d.tolist())
            start, length = A.equal_runs(ref["src_off"])
            longest = max(longest, int(length.max()))
            lengths.append(length)
            big = length >= 64
            starts |= set((start[big] % 256).tolist())
            ends |= set(((start[big] + length[big]) % 256).tolist())
        assert set(range(1, 1025)) <= seen and max(seen) >= 50000, (len(seen), max(seen))
        assert any(v in g["want"][0] for v in g["seeds"][:B].tolist()) == (hops == 1)      # the self-targeting input (a middle at H = 2)
        if arrangement == "grouped":
            # long runs begin and end in the last lane of a wave, the first, the second -- and the same around thread 255 -> 0
            edge = {63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 0, 1}
            assert longest >= B * f and edge <= starts and edge <= ends, (longest, sorted(edge - starts), sorted(edge - ends))
        else:
            # the all-to-one batch is one run in either arrangement; in every other batch a run is one input's draws (<= f edges) until
            # only the batch's largest target has inputs left
            assert longest == B * f and np.median(np.concatenate(lengths[:-1])) <= f and (np.concatenate(lengths[:-1]) <= f).mean() > 0.9


def test_vectorised_draw_index_is_pyrefs():
    """aggref.sample_indices (what recounts the draws of a graph with -1 entries) against pyref.sample_index, value by value"""
    import pyref
    from aggref import sample_indices
    rs = np.random.RandomState(2)
    idx = np.concatenate([np.arange(0, 300), rs.randint(0, 1 << 31, size=700, dtype=np.int64), [(1 << 31) - 2, (1 << 31) - 3]])
    deg = np.concatenate([rs.randint(1, 50, size=500), rs.randint(1, 1 << 22, size=len(idx) - 500)])
    assert sample_indices(idx, deg).tolist() == [pyref.sample_index(int(i), int(d)) for i, d in zip(idx, deg)]
