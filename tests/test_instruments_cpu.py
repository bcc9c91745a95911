"""What tests/test_gpu_instruments.py and tests/test_gpu_synth_windows.py rest on, proved without a GPU (tests/instrumentcases.py).

Three statements, one rule: the NumPy statements of legion-1_amd/synth.py -- the GPU tests' reference -- equal an exact-integer restatement
at every window, for three dataset specs, and the neighbour rule also equals the oracle's C statement at every skew.  A truncating kernel
would be seen: a window above 2^32 differs from the window at the same index modulo 2^32 in most entries.  The case tables reach what
their names say: ragged last steps, several loop iterations, the word sum's grid cap, every n_tail.  And the three instruments are
declared in capi.py with the header's signatures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import instrumentcases as IC
from conftest import ROOT


@pytest.fixture(scope="module", params=IC.SPECS, ids=lambda p: "%s@%g" % p)
def spec(request, synth):
    return synth.spec_for(*request.param)


def both_ends(a):
    return [(k, a[k]) for r in IC.exact_slices(len(a)) for k in r]


# ---- three statements, one rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e0", IC.WINDOWS)
def test_numpy_neighbours_weights_and_edge_features_equal_the_integer_rules(spec, synth, e0):
    n = IC.WINDOW_N
    nbr = synth.neighbors(spec, e0, e0 + n)
    assert nbr.dtype == np.int32 and nbr.shape == (n,) and nbr.min() >= 0 and nbr.max() < spec.V
    for k, got in both_ends(nbr):
        assert int(got) == IC.neighbor(e0 + k, spec.V, spec.M, spec.C), (e0, k)
    w = synth.edge_weights(e0 + n, e0)
    assert w.dtype == np.float32 and w.shape == (n,)
    for k, got in both_ends(w):
        assert float(got) == IC.edge_weight(e0 + k), (e0, k)
    for dim in IC.EDGE_DIMS:
        ef = synth.edge_features(e0, n, dim)
        assert ef.dtype == np.float32 and ef.shape == (n, dim)
        for k, row in both_ends(ef):
            assert [float(x) for x in row] == [IC.edge_feature(e0 + k, c) for c in range(dim)], (e0, k, dim)


@pytest.mark.parametrize("start", IC.WINDOWS)
@pytest.mark.parametrize("F", IC.FEATURE_WIDTHS)
def test_numpy_features_equal_the_integer_rule(synth, start, F):
    """rows, not elements: the window starts at the row that holds absolute element `start`"""
    spec = synth.spec_for("papers100M", F=F)
    v0 = IC.feature_v0(start, F)
    assert v0 * F <= start < (v0 + 1) * F
    got = synth.features(spec, np.arange(v0, v0 + IC.WINDOW_N, dtype=np.int64))
    assert got.dtype == np.float32 and got.shape == (IC.WINDOW_N, F)
    for r, row in both_ends(got):
        for c in sorted({0, F // 2, F - 1}):
            want = IC.feature(v0 + r, c, F)
            assert isinstance(want, np.float32) and row[c] == want and -0.5 <= want < 0.5, (start, F, r, c)
    k = (got.astype(np.float64) + 0.5) * 2.0 ** 24                                      # exact by construction: 24-bit integers behind the scaling
    assert np.array_equal(k, np.floor(k)) and k.min() >= 0 and k.max() < 2 ** 24


def test_numpy_labels_seed_ids_and_degrees_equal_the_integer_rules(spec, synth):
    n = IC.WINDOW_N
    for v0 in IC.node_windows(spec.V):
        assert 0 <= v0 and v0 + n <= spec.V < 2 ** 31                                   # the kernels take v0 and n as int32
        ids = np.arange(v0, v0 + n, dtype=np.int64)
        for k, got in both_ends(synth.labels(spec, ids)):
            assert int(got) == IC.label(v0 + k, spec.classes), (v0, k)
        for k, got in both_ends(synth.degrees(spec, v0, v0 + n)):
            assert int(got) == IC.degree(v0 + k, spec.ladder), (v0, k)
        sid = synth.seed_ids(spec, v0, v0 + n)
        assert sid.min() >= 0 and sid.max() < spec.V
        for k, got in both_ends(sid):
            assert int(got) == IC.seed_id(v0 + k, spec.V, spec.M2, spec.C2), (v0, k)
    assert IC.degree(0, spec.ladder) >= 1 and len(spec.ladder) == IC.NBUCKET + 2


def test_strided_seed_lists_are_slices_of_the_plain_list(synth):
    """the reference expression of the GPU test, stated once against the integer rule: entry k is seed i0 + phase + k * stride"""
    spec, n = synth.spec_for("uk-union"), 500
    for stride, phase in IC.SEED_STRIDES:
        for i0 in (0, spec.n_train - n):
            got = synth.seed_ids(spec, i0, i0 + phase + n * stride)[phase::stride]
            assert len(got) == n
            for k in (0, 1, n // 2, n - 1):
                assert int(got[k]) == IC.seed_id(i0 + phase + k * stride, spec.V, spec.M2, spec.C2), (stride, phase, i0, k)
    assert {s for s, _ in IC.SEED_STRIDES} == {1, 2, 3, 8} and all({0, 1, s - 1} == {p for t, p in IC.SEED_STRIDES if t == s} for s in (1, 2, 3, 8))


def sg_neighbors(oracle, e0, n, spec, skew):
    out = np.empty(n, np.int32)
    oracle.lib().sg_neighbors(out.ctypes.data_as(C.c_void_p), C.c_int64(e0), C.c_int64(n), C.c_uint32(spec.V), C.c_uint32(spec.M), C.c_uint32(spec.C),
                              C.c_uint32(skew))
    return out


@pytest.mark.parametrize("e0", IC.WINDOWS)
def test_the_integer_neighbour_rule_equals_the_oracle_at_every_skew(spec, synth, oracle, e0):
    n = IC.WINDOW_N
    at_205 = sg_neighbors(oracle, e0, n, spec, 205)
    assert np.array_equal(at_205, synth.neighbors(spec, e0, e0 + n))
    for skew in IC.SKEWS:
        got = at_205 if skew == 205 else sg_neighbors(oracle, e0, n, spec, skew)
        for k, g in both_ends(got):
            assert int(g) == IC.neighbor(e0 + k, spec.V, spec.M, spec.C, skew), (e0, k, skew)
    assert not np.array_equal(sg_neighbors(oracle, e0, n, spec, 0), sg_neighbors(oracle, e0, n, spec, 256))       # the skew does something
    assert not np.array_equal(sg_neighbors(oracle, e0, n, spec, 255), sg_neighbors(oracle, e0, n, spec, 256))     # ... up to its last step


# ---- a truncating kernel would be seen --------------------------------------------------------------------------------------------------------
def test_windows_above_2_32_differ_from_their_index_modulo_2_32(spec, synth):
    """a condition on the INPUTS: a kernel that drops the high word of the index computes the right-hand side, so the two sides have to differ"""
    n, high = IC.WINDOW_N, [w for w in IC.WINDOWS if w >= 2 ** 32]
    assert len(high) == 3 and any(w < 2 ** 32 < w + n for w in IC.WINDOWS)             # and one window crosses 2^32 inside
    for e0 in high:
        lo = e0 % 2 ** 32
        frac = dict(neighbors=np.mean(synth.neighbors(spec, e0, e0 + n) != synth.neighbors(spec, lo, lo + n)),
                    edge_weights=np.mean(synth.edge_weights(e0 + n, e0) != synth.edge_weights(lo + n, lo)))
        for dim in IC.EDGE_DIMS:
            frac["edge_features %d" % dim] = np.mean(synth.edge_features(e0, n, dim) != synth.edge_features(lo, n, dim))
        assert all(f > 0.5 for f in frac.values()), (e0, frac)
    for start in high:                                                                  # the feature table's element index passes 2^32 too (papers100M: V * F = 1.4e10)
        for F in IC.FEATURE_WIDTHS:
            f_spec, v0 = synth.spec_for("papers100M", F=F), IC.feature_v0(start, F)
            lo = v0 - 2 ** 32 // F if 2 ** 32 % F == 0 else None                        # rows whose element index is 2^32 less exist only where F divides 2^32
            if lo is not None:
                assert np.mean(synth.features(f_spec, np.arange(v0, v0 + 200)) != synth.features(f_spec, np.arange(lo, lo + 200))) > 0.5


# ---- the case tables ------------------------------------------------------------------------------------------------------------------------------
def test_the_windows_and_the_long_run_are_the_stated_ones():
    assert IC.WINDOWS == (0, 2 ** 31 - 300, 2 ** 32 - 300, 2 ** 32 + 12345, 2 ** 33 - 7, 2 ** 40 - 50)
    assert IC.WINDOW_N == 3000 and IC.EXACT_N == 200 and IC.LONG_N == 4096 * 256 + 4097
    lanes = 4096 * 256                                                                  # big_grid's cap: every lane of the full grid takes a first step,
    assert IC.LONG_N > lanes + 1 and (IC.LONG_N - lanes) % 256 != 0                     # some take a second one, and the last workgroup that does is ragged
    assert -(-IC.LONG_N // 256) > 4096                                                  # ... because the grid really is capped at this size
    assert 8 * IC.LONG_N + 4096 < IC.MAX_BUFFER                                         # an int64 output of one call stays far below the buffer limit
    assert max(IC.WINDOWS) + IC.LONG_N < 2 ** 63


@pytest.mark.parametrize("unroll", IC.COPY_UNROLLS)
def test_every_copy_size_exercises_what_its_name_says(unroll):
    cases = {c.name: c for c in IC.copy_sizes(unroll)}
    assert len(cases) == len(IC.copy_sizes(unroll)) == 16
    plan = {name: IC.copy_plan(c, unroll) for name, c in cases.items()}
    step = 256 * unroll
    assert [plan[k]["n"] for k in ("one chunk", "block - 1", "block", "block + 1", "step - 1", "step", "step + 1", "three steps ragged")] == \
        [1, 255, 256, 257, step - 1, step, step + 1, 3 * step + 77]
    for name, p in plan.items():
        assert 16 * p["n"] + p["rem"] == cases[name].nbytes <= 16 * (6 * 256 * 8 + 77) + 12 and p["grid"] >= 1
        if cases[name].grid == 0:
            assert p["iters"] == 1 and p["grid"] == -(-p["n"] // step), name            # grid <= 0: one iteration per lane, the last workgroup ragged or full
    assert plan["step"]["last"] == step and plan["step"]["grid"] == 1                   # exactly one full workgroup step: no guard fails
    assert plan["step - 1"]["grid"] == 1 and plan["step + 1"]["grid"] == 2              # one chunk short of it, and one chunk into a second workgroup
    assert plan["three steps ragged"]["grid"] == 4 and plan["three steps ragged"]["n"] % step == 77
    g3, g1 = plan["grid 3 loops"], plan["grid 1 loops"]
    assert g3["grid"] == 3 and g3["iters"] == 3 and g3["last"] == 77                    # two full trips of every workgroup, then 77 chunks: a ragged last step
    assert g1["grid"] == 1 and g1["iters"] == 6 and g1["last"] == 1                     # five full trips, then one chunk
    for r in (4, 8, 12):
        for base in ("one chunk", "three steps ragged"):
            p = plan["%s + %d bytes" % (base, r)]
            assert p["rem"] == r and p["n"] == plan[base]["n"]
    assert all(p["rem"] == 0 for name, p in plan.items() if "bytes" not in name)


@pytest.mark.parametrize("unroll", IC.COPY_UNROLLS)
def test_the_index_plan_covers_every_chunk_once_and_two_wrong_plans_do_not(unroll):
    """k_copy_f4's index arithmetic restated (instrumentcases.copy_touched): at these sizes both plans store every chunk exactly once; a CONTIG
    plan whose lane distance is the whole grid, and a store guard one chunk short, each miss chunks at some size -- so the GPU comparison at
    the same sizes can tell them from the kernel"""
    seen_wide, seen_short = False, True
    for case in IC.copy_sizes(unroll):
        p = IC.copy_plan(case, unroll)
        for contig in IC.COPY_CONTIGS:
            assert (IC.copy_touched(p["n"], p["grid"], unroll, contig) == 1).all(), (case, contig)
            short = IC.copy_touched(p["n"], p["grid"], unroll, contig, guard_slack=1)
            seen_short &= short[-1] == 0 and (short[:-1] == 1).all()
        wide = IC.copy_touched(p["n"], p["grid"], unroll, 1, contig_step=p["grid"] * 256)
        seen_wide |= not (wide == 1).all()
        if unroll == 1 or p["grid"] == 1:
            assert (wide == 1).all()                                                    # where that wrong plan IS the right one
    assert seen_short and seen_wide == (unroll > 1)


def test_the_sum_sizes_reach_every_loop_every_tail_and_the_grid_cap():
    assert IC.SUM_SIZES == (4, 8, 12, 16, 20, 28, 16368, 16380, 16384, 16388, 16400, 16 * 4099 + 8, 16 * (2048 * 1024 + 5 * 1024 + 3) + 12)
    plans = [IC.sum_plan(b) for b in IC.SUM_SIZES]
    assert all(b % 4 == 0 and 0 < b <= IC.MAX_BUFFER for b in IC.SUM_SIZES)
    assert {p["n_tail"] for p in plans} == {0, 1, 2, 3}
    assert {p["n_tail"] for p in plans if p["n16"] == 0} == {1, 2, 3}                   # nothing but a tail: the one workgroup's lanes read only tail words
    assert [p["grid"] for p in plans[:9]] == [1] * 9 and plans[10]["grid"] == 2         # 1024 chunks fill one workgroup, 1025 start a second
    assert any(p["unrolled"] >= 1 and p["rest"] >= 1 for p in plans)                    # the 4x-unrolled loop and the remainder loop in one call
    assert any(p["unrolled"] >= 1 and p["rest"] == 0 for p in plans) and any(p["unrolled"] == 0 and p["rest"] >= 1 for p in plans)
    capped = [p for p in plans if p["uncapped"] > IC.SUM_GRID_CAP]
    assert len(capped) == 1 and capped[0]["grid"] == IC.SUM_GRID_CAP == 2048 and capped[0]["n_tail"] == 3 and capped[0]["unrolled"] >= 1 and capped[0]["rest"] >= 1
    assert IC.sum_plan(16 * 1024 * 2048)["grid"] == 2048 and IC.sum_plan(16 * 1024 * 2047)["grid"] == 2047


def test_the_pattern_names_positions_and_the_sum_reference_carries():
    a = IC.pattern(70000, 0x5EED)
    assert a.dtype == np.uint32 and [int(x) for x in a[:50]] == [IC.mix32(i ^ 0x5EED) for i in range(50)]
    assert int(a[69999]) == IC.mix32(69999 ^ 0x5EED) and len(np.unique(a)) == len(a)    # mix32 is a bijection: no two positions hold the same word
    assert not np.array_equal(a[:1000], IC.pattern(1000, 0x5EEE))
    sentinel_word = IC.SENTINEL * 0x01010101
    assert sentinel_word not in a and not (a.view(np.uint8) == IC.SENTINEL).reshape(-1, 16).all(axis=1).any()    # no chunk of it looks like an untouched destination
    assert IC.word_sum(a) == sum(int(x) for x in a) % 2 ** 64 and IC.word_sum(a) > 2 ** 32
    ones = np.full(5, 0xFFFFFFFF, np.uint32)
    assert IC.word_sum(ones) == 5 * 0xFFFFFFFF and IC.word_sum(np.zeros(0, np.uint32)) == 0
    n_big = IC.SUM_SIZES[-1] // 4
    assert n_big * 0xFFFFFFFF < 2 ** 64 and (2 ** 64 - 5 + n_big * 0xFFFFFFFF) % 2 ** 64 < n_big * 0xFFFFFFFF    # the preloaded accumulator really wraps


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------------
C_TYPES = {"void*": C.c_void_p, "const void*": C.c_void_p, "uint64_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32}
INSTRUMENTS = {"legion_copy_f4": "void", "legion_copy_f4_cfg": "int", "legion_sum_words": "void"}


def test_header_and_capi_agree_on_the_instruments():
    import legion1_amd.capi as K
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)               # the declarations, without the comments that name the calls
    for name, ret in INSTRUMENTS.items():
        m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m and m.group(1) == ret, name
        args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(2).split(",")]       # drop each parameter's name
        res, sig = K._SIGS[name]
        assert res == (None if ret == "void" else C.c_int), name
        assert sig == [C_TYPES[a] for a in args], (name, args)
        assert hasattr(K.lib(), name), name
    assert "bytes % 16" in re.search(r"/\*((?:(?!\*/).)*)\*/\s*int legion_copy_f4_cfg", header, flags=re.S).group(1)     # the ragged-byte rule is a stated contract
