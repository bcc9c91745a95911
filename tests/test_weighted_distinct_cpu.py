"""Weighted sampling without replacement (LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1, INTEGRATION.md "Weighted sampling without
replacement"), the parts that need no GPU: the statement of tests/wdistinctref.py against itself and against the exact successive-sampling
probabilities, the environment parser through the `legion` binary's boot, the pool's flag and the graph's retain switch without a
device, the launcher's flag, the C ABI's new names and the Engine's argument check."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import wdistinctref as R
from conftest import ROOT
from distinctref import mix32_scalar

SERVER = os.path.join(ROOT, "legion-1_amd", "csrc", "legion")
MODE_VARS = ("LEGION_AGG_LAST_HOP", "LEGION_AGG_NORM", "LEGION_SAMPLING", "LEGION_SAMPLING_SEED", "LEGION_LP_DRAW", "LEGION_WEIGHTED_DISTINCT")


def scalar_picks(i, h, w_row, f, W=0):
    """the statement once more, in plain Python floats and ints"""
    K = mix32_scalar(mix32_scalar(((i + R.GOLDEN * h) & R.M32) ^ W) ^ R.WD_TAG)
    keyed = []
    for c, x in enumerate(w_row):
        if x > 0:
            u = mix32_scalar(K ^ ((R.STEP * (c + 1)) & R.M32))
            keyed.append((-math.log((u + 0.5) * 2.0 ** -32) / float(x), c))
    keyed.sort()
    return sorted(c for _, c in keyed[:f])


def random_rows(seed, n):
    """(i, h, weights, f, W) with d in 1..400, f in {1, 5, 10, 25, 64} and the synth: source's weight alphabet 0..16"""
    rng = np.random.RandomState(seed)
    for _ in range(n):
        d = int(rng.randint(1, 401))
        w = rng.randint(0, 17, size=d).astype(np.float32)
        if rng.rand() < 0.1:
            w[:] = 0
        if rng.rand() < 0.2:
            w[rng.rand(d) < 0.9] = 0                                     # few eligible columns: m <= f < d occurs
        yield int(rng.randint(0, 2 ** 31 - 1)), int(rng.randint(1, 4)), w, int(rng.choice([1, 5, 10, 25, 64])), int(rng.randint(0, 2 ** 32, dtype=np.uint64))


# ---- the statement ------------------------------------------------------------------------------------
def test_statement_properties_on_random_rows():
    seen_small = seen_cut = seen_zero = 0
    for i, h, w, f, W in random_rows(11, 1500):
        picks, gap = R.row_picks(i, h, w, f, W)
        elig = np.nonzero(w > 0)[0]
        m = len(elig)
        assert gap >= R.TIE_MARGIN                                       # the cap on near ties is zero rows
        assert len(picks) == min(m, f) and (np.diff(picks) > 0).all()    # min(m, f) many, distinct, ascending
        assert np.isin(picks, elig).all()                                # a zero-weight column is never picked
        assert picks.tolist() == scalar_picks(i, h, w.tolist(), f, W)
        if m <= f:
            assert picks.tolist() == elig.tolist() and gap == np.inf     # exactly the eligible columns
            seen_small += m > 0 and len(w) > f
            seen_zero += m == 0
        else:
            seen_cut += 1
    assert seen_small > 20 and seen_cut > 500 and seen_zero > 50


def test_the_draw_word_and_the_row_change_the_picks():
    w = np.random.RandomState(3).randint(1, 17, size=120).astype(np.float32)
    base = R.row_picks(7, 1, w, 10, 0)[0].tolist()
    assert base == R.row_picks(7, 1, w, 10, 0)[0].tolist()
    assert base != R.row_picks(7, 1, w, 10, 12345)[0].tolist()
    assert base != R.row_picks(8, 1, w, 10, 0)[0].tolist() and base != R.row_picks(7, 2, w, 10, 0)[0].tolist()


def test_extreme_weights_keep_finite_keys():
    tiny, huge = np.float32(1e-45), np.finfo(np.float32).max             # the smallest subnormal, FLT_MAX
    assert tiny > 0
    u, key = R.column_keys(np.arange(4096), 1, np.arange(4096) % 7, np.where(np.arange(4096) % 2, tiny, huge), 0)
    assert np.isfinite(key).all() and (key > 0).all()
    assert R.row_picks(0, 1, [tiny, huge, tiny], 1)[0].tolist() == [1]  # FLT_MAX against 1e-45: never the subnormal


def test_inclusion_frequencies_follow_successive_sampling():
    """One row, w = (1, 2, 3, 4, 0), f = 2, over 2^16 row indices: every empirical inclusion frequency within 6 binomial standard
    deviations sqrt(p (1 - p) / N) of the exact successive-sampling probability."""
    w = np.array([1, 2, 3, 4, 0], np.float32)
    N = 1 << 16
    p = R.inclusion_probabilities(w, 2)
    assert [round(x, 4) for x in p] == [0.2345, 0.4413, 0.6083, 0.7159, 0.0]
    pos, gap = R.positions(np.arange(N), 1, np.zeros(N, np.int64), np.full(N, 5), 2, w)
    assert (gap >= R.TIE_MARGIN).all() and ((pos >= 0).sum(axis=1) == 2).all()
    for c in range(5):
        freq = float((pos == c).any(axis=1).mean())
        sd = math.sqrt(p[c] * (1 - p[c]) / N)
        z = (freq - p[c]) / sd if sd else 0.0
        print("column %d: %.4f against %.4f, z = %+.2f" % (c, freq, p[c], z))
        assert freq == 0.0 if p[c] == 0.0 else abs(z) <= 6.0


def small_graph(seed=0, V=300):
    rng = np.random.RandomState(seed)
    deg = rng.randint(0, 41, size=V)
    deg[5], deg[6] = 700, 9
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    indices = rng.randint(-1, V, size=E).astype(np.int32)
    w = rng.randint(0, 17, size=E).astype(np.float32)
    for v in rng.choice(np.nonzero(deg > 0)[0], 12, replace=False):
        w[indptr[v]:indptr[v + 1]] = 0.0
    return indptr, indices, w


def test_whole_batches_draw_distinct_weighted_columns():
    indptr, indices, w = small_graph()
    V = len(indptr) - 1
    g = R.Weights(indptr, indices, w)
    feats = np.random.RandomState(2).rand(V, 3).astype(np.float32)
    labels = np.arange(V, dtype=np.int32) % 7
    seeds = np.random.RandomState(3).permutation(V)[:150].astype(np.int32)
    fan = [7, 5, 3]
    assert R.near_ties(g, seeds, 64, (0, 1, 2), fan) == [] and R.near_ties(g, seeds, 64, (0,), fan, 12345) == []
    for counter, word in ((0, 0), (1, 0), (2, 0), (0, 12345)):
        b = R.run_batch(g, feats, seeds, labels[seeds], 64, counter, fan, word)
        for h, f in enumerate(fan):
            inp, cnt = b["draw_counts"][h]
            for node, n in zip(inp.tolist(), cnt.tolist()):
                if node >= 0:
                    sl = slice(int(indptr[node]), int(indptr[node + 1]))
                    assert n <= min(f, int(((w[sl] > 0) & (indices[sl] >= 0)).sum()))   # a hole is eligible but gives no edge
        assert int(b["ec"][2 + 3]) == sum(int(c.sum()) for _, c in b["draw_counts"]) > 0
    a, c = R.run_batch(g, feats, seeds, labels[seeds], 64, 0, fan, 0), R.run_batch(g, feats, seeds, labels[seeds], 64, 0, fan, 12345)
    assert not np.array_equal(a["draws"][0], c["draws"][0])


# ---- parser and boot ----------------------------------------------------------------------------------
ACCEPTED = "Server_Initialize: the synth: dataset path names no known workload / scale"
NEEDS = "Server_Initialize: LEGION_WEIGHTED_DISTINCT=1 needs LEGION_SAMPLING=weighted"


@pytest.mark.parametrize("sampling,flag,fanout,said", [
    ("weighted", None, "65,2", ACCEPTED),                                # plain weighted keeps accepting 65
    ("weighted", "", "65,2", ACCEPTED),
    ("weighted", "0", "65,2", ACCEPTED),
    ("weighted", "1", "64,2", ACCEPTED),
    (None, "0", "10,5", ACCEPTED),
    ("weighted", "2", "10,5", "Server_Initialize: LEGION_WEIGHTED_DISTINCT=2 is not a known setting: `1` (weighted draws without replacement: distinct columns per row, by edge weight), `0` or unset"),
    ("weighted", "on", "10,5", "Server_Initialize: LEGION_WEIGHTED_DISTINCT=on is not a known setting"),
    (None, "1", "10,5", NEEDS),
    ("distinct", "1", "10,5", NEEDS),
    ("replace", "1", "10,5", NEEDS),
    ("weighted", "1", "65,2", "Server_Initialize: LEGION_WEIGHTED_DISTINCT=1 takes fan-outs of at most 64, hop 1 has 65"),
    ("weighted", "1", "10,70", "Server_Initialize: LEGION_WEIGHTED_DISTINCT=1 takes fan-outs of at most 64, hop 2 has 70"),
])
def test_boot_parses_the_flag(tmp_path, sampling, flag, fanout, said):
    """Every refusal comes before a device is touched: this machine has none, and the accepted settings get as far as the synth: source."""
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write("synth:nosuchworkload 512 1000 0 16 100 0 0 %d 1 0\n" % (1 << 30))
    env = {k: v for k, v in os.environ.items() if k not in MODE_VARS}
    env.update(LEGION_IPC_NAMESPACE="cpuwd%d_" % os.getpid())
    if sampling is not None:
        env["LEGION_SAMPLING"] = sampling
    if flag is not None:
        env["LEGION_WEIGHTED_DISTINCT"] = flag
    r = subprocess.run([SERVER, "1", "0", fanout, meta], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 1 and said in out, out[-2000:]


# ---- the pool's flag and the graph's switch, without a device --------------------------------------------
def test_pool_flag_round_trip_without_a_gpu():
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    pool = L.NewGPUMemoryPool(2)

    def err():
        msg = (L.legion_last_error() or b"").decode()
        L.legion_clear_error()
        return msg
    try:
        assert L.GPUMemoryPool_GetWeightedDistinct(pool) == 0 and L.GPUMemoryPool_GetWeightedDistinct(None) == 0
        L.GPUMemoryPool_SetSampling(pool, 2)
        for on, want in ((1, 1), (0, 0), (7, 1)):
            L.GPUMemoryPool_SetWeightedDistinct(pool, on)
            assert not err() and L.GPUMemoryPool_GetWeightedDistinct(pool) == want
            assert L.GPUMemoryPool_GetSampling(pool) == 2 and L.GPUMemoryPool_GetSampleDistinct(pool) == 0    # a flag, not a fourth kind
        for kind in (0, 1, 2):                                               # the flag is remembered across kinds
            L.GPUMemoryPool_SetSampling(pool, kind)
            assert not err() and L.GPUMemoryPool_GetSampling(pool) == kind and L.GPUMemoryPool_GetWeightedDistinct(pool) == 1
        L.GPUMemoryPool_SetSampling(pool, 0)
        L.GPUMemoryPool_SetWeightedDistinct(pool, 0)                         # ... and may be set under any kind
        L.GPUMemoryPool_SetWeightedDistinct(pool, 1)
        assert not err() and L.GPUMemoryPool_GetSampling(pool) == 0 and L.GPUMemoryPool_GetWeightedDistinct(pool) == 1
        L.GPUMemoryPool_SetSampling(pool, 3)                                 # still no fourth kind
        assert "GPUMemoryPool_SetSampling: unknown sampling kind (0 = replace, 1 = distinct, 2 = weighted)" in err()
        L.GPUMemoryPool_SetWeightedDistinct(None, 1)
        assert "GPUMemoryPool_SetWeightedDistinct: null pool" in err()
        # the graph's side refuses null and unbuilt handles by name and touches no device
        assert L.GPUGraphStorage_RetainEdgeWeights(None, 1) == -1 and "GPUGraphStorage_RetainEdgeWeights: null graph" in err()
        assert L.GPUGraphStorage_HasRetainedEdgeWeights(None) == 0
        g = L.NewGPUMemoryGraphStorage()
        assert L.GPUGraphStorage_HasRetainedEdgeWeights(g) == 0
        assert L.GPUGraphStorage_RetainEdgeWeights(g, 1) == -1 and "GPUGraphStorage_Build was not called" in err()
        L.GPUGraphStorage_Delete(g)
    finally:
        L.legion_clear_error()
        L.GPUMemoryPool_Delete(pool)


# ---- launcher and Python surface ----------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["--weighted-distinct", "--weighted_distinct", None])
def test_launch_server_passes_the_flag_on(tmp_path, flag):
    work = tmp_path / "pkg"
    (work / "csrc").mkdir(parents=True)
    (work / "launch_server.py").write_text(open(os.path.join(ROOT, "legion-1_amd", "launch_server.py")).read())
    stand_in = work / "csrc" / "legion"
    stand_in.write_text("#!/bin/sh\necho \"SAMPLING=[${LEGION_SAMPLING}] WD=[${LEGION_WEIGHTED_DISTINCT}]\"\n")
    stand_in.chmod(0o755)
    env = {k: v for k, v in os.environ.items() if k not in MODE_VARS}
    r = subprocess.run([sys.executable, str(work / "launch_server.py"), "--dataset", "PR", "--gpu_number", "1", "--sampling", "weighted"] + ([flag] if flag else []),
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=60)
    assert "SAMPLING=[weighted] WD=[%s]" % ("1" if flag else "") in r.stdout, r.stdout + r.stderr


def test_capi_table_and_header_name_the_new_symbols():
    import legion1_amd.capi as K
    L = K.lib()
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    for name in ("GPUGraphStorage_RetainEdgeWeights", "GPUGraphStorage_HasRetainedEdgeWeights", "GPUMemoryPool_SetWeightedDistinct",
                 "GPUMemoryPool_GetWeightedDistinct", "legion_weighted_distinct_probe"):
        assert name in K._SIGS and name + "(" in header and getattr(L, name)


def test_engine_refuses_the_flag_without_the_weighted_kind_before_it_touches_anything():
    import legion1_amd.capi as K
    eng = K.Engine.__new__(K.Engine)            # no device: _set_modes validates its arguments first
    for sample in ("replace", "distinct"):
        with pytest.raises(ValueError, match="weighted_distinct=True needs sample='weighted'"):
            eng._set_modes(0, False, None, sample, None, 0, None, weighted_distinct=True)
    with pytest.raises(ValueError, match="'replace', 'distinct' or 'weighted'"):
        eng._set_modes(0, False, None, "heavy", None, 0, None, weighted_distinct=True)
