"""Shared-key sampling (LEGION_SAMPLING=distinct LEGION_SHARED_DRAWS=1, INTEGRATION.md "Shared-key sampling"), the parts that need no GPU:
the statement of tests/sharedref.py against a plain-Python restatement, the properties that make it what it is (a row's picks depend on
its neighbour ids and the batch alone; every column is equally likely; rows that overlap agree, so a batch reaches far fewer nodes for the
same edges), the environment parser through the `legion` binary's boot, the pool's flag without a device, the launcher's flag, the C
ABI's new names and the Engine's argument check."""
import os
import subprocess
import sys

import numpy as np
import pytest

import distinctref as D
import sharedref as R
from conftest import ROOT
from distinctref import mix32_scalar

SERVER = os.path.join(ROOT, "legion-1_amd", "csrc", "legion")
MODE_VARS = ("LEGION_AGG_LAST_HOP", "LEGION_AGG_NORM", "LEGION_SAMPLING", "LEGION_SAMPLING_SEED", "LEGION_LP_DRAW", "LEGION_WEIGHTED_DISTINCT",
             "LEGION_SHARED_DRAWS")


def scalar_picks(nbr, f, W=0):
    """the statement once more, in plain Python ints"""
    d = len(nbr)
    if d <= f:
        return list(range(d))
    Ks = mix32_scalar((W & 0xFFFFFFFF) ^ 0x165667B1)
    keyed = sorted((mix32_scalar((int(x) & 0xFFFFFFFF) ^ Ks), c) for c, x in enumerate(nbr))
    return sorted(c for _, c in keyed[:f])


def random_rows(seed, f_of=(1, 5, 10, 25, 64)):
    """(nbr, f, W): every f with every degree of {0, 1, f - 1, f, f + 1, 64, 65, 129, 300}, ids from a small alphabet (multi-edges
    throughout) or the whole int32 range, one entry in ten a hole (-1)"""
    rng = np.random.RandomState(seed)
    for f in f_of:
        for d in sorted({0, 1, f - 1, f, f + 1, 64, 65, 129, 300}):
            for small in (True, False):
                nbr = rng.randint(0, 40, size=d) if small else rng.randint(-2 ** 31, 2 ** 31 - 1, size=d, dtype=np.int64)
                nbr = np.where(rng.rand(d) < 0.1, -1, nbr).astype(np.int32)
                yield nbr, f, int(rng.randint(0, 2 ** 32, dtype=np.uint64)) if small else 0


# ---- the statement ------------------------------------------------------------------------------------
def test_scalar_statement_agrees_with_the_vectorised_one():
    n = cut = ties = 0
    for nbr, f, W in random_rows(5):
        picks = R.row_picks(nbr, f, W)
        assert picks.tolist() == scalar_picks(nbr.tolist(), f, W), (len(nbr), f, W)
        assert len(picks) == min(len(nbr), f) and (np.diff(picks) > 0).all()          # min(d, f) many, distinct, ascending
        n += 1
        cut += len(nbr) > f
        ties += len(nbr) > f and len(set(nbr.tolist())) < len(nbr)
    assert n == 82 and cut == 46 and ties > 15                                        # 41 (f, d) pairs: at f = 1 and f = 64 the degree sets overlap


def test_a_multi_edge_ties_on_the_key_and_the_column_decides():
    assert R.row_picks(np.full(200, 77, np.int32), 5, 9).tolist() == [0, 1, 2, 3, 4]
    assert R.node_keys(np.array([-1, 0, 2999], np.int32), 0).tolist() == [mix32_scalar(x ^ mix32_scalar(0x165667B1)) for x in (0xFFFFFFFF, 0, 2999)]


def test_permuted_neighbour_lists_pick_the_same_ids_whatever_the_row_or_the_hop():
    """The key belongs to the neighbour: two rows whose lists are permutations of each other take the same id SET, and neither the row's
    index in the input list nor the hop enters (the draw is not even told the row: positions() has no such argument; here through whole
    batches, where the same node is a source at different rows of different hops)."""
    rng = np.random.RandomState(8)
    for f, W in ((5, 0), (10, 77), (64, 0xDEADBEEF)):
        nbr = rng.choice(5000, size=150, replace=False).astype(np.int32)
        perm = rng.permutation(150)
        a, b = R.row_picks(nbr, f, W), R.row_picks(nbr[perm], f, W)
        assert sorted(nbr[a].tolist()) == sorted(nbr[perm][b].tolist())
        assert sorted(nbr[a].tolist()) != sorted(nbr[R.row_picks(nbr, f, W + 1)].tolist())   # the draw word does enter
    # whole batches: every source node's picked id set is one set per batch, at whichever rows and hops it stands
    V = 400
    deg = rng.randint(0, 30, size=V)
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.randint(0, V, size=int(indptr[-1])).astype(np.int32)
    seeds = rng.permutation(V)[:60].astype(np.int32)
    fan = [4, 4, 4]
    b = R.run_batch(indptr, indices, np.zeros((V, 1), np.float32), seeds, seeds, 60, 0, fan, W=3)
    picked, seen_twice = {}, 0
    for h in range(3):
        inp = b["draw_counts"][h][0]
        draws = b["draws"][h].reshape(len(inp), fan[h])
        for v, row in zip(inp.tolist(), draws.tolist()):
            got = sorted(x for x in row if x >= 0)
            seen_twice += v in picked
            assert picked.setdefault(v, got) == got
    assert seen_twice > 100


def test_every_column_is_equally_likely():
    """One row of 12 distinct ids at f = 5 over 20 000 draw words: the inclusion counts of the columns against f / d by chi-square.  The
    twelve counts sum to f N and a draw's indicators are exchangeable (variance p (1 - p), covariance p ((f - 1) / (d - 1) - p), p = f / d),
    so the statistic sum (o - e)^2 / (e (d - f) / (d - 1)) is chi-square with d - 1 degrees of freedom: Pearson's, with the
    finite-population factor of a fixed-size sample without replacement."""
    d, f, N = 12, 5, 20000
    nbr = np.random.RandomState(4).choice(100000, size=d, replace=False).astype(np.int32)
    words = np.arange(N, dtype=np.int64) * 2654435761 % (1 << 32)
    keys = R.node_keys(np.broadcast_to(nbr, (N, d)), words[:, None])
    taken = np.argsort(keys, axis=1, kind="stable")[:, :f]
    assert sorted(taken[17].tolist()) == R.row_picks(nbr, f, int(words[17])).tolist()      # the same rule as the statement's
    counts = np.bincount(taken.reshape(-1), minlength=d)
    e = N * f / d
    chi2 = float(((counts - e) ** 2).sum() / (e * (d - f) / (d - 1)))
    print("inclusion counts", counts.tolist(), "expected %.1f, chi2 = %.2f, cap %.2f" % (e, chi2, D.chi2_cap(d - 1)))
    assert chi2 <= D.chi2_cap(d - 1)


def test_the_point_of_the_mode_fewer_nodes_for_the_same_edges():
    """products @ 0.25, B = 2000, {25, 10, 5}, batches 0 and 3: the shared-key batch has exactly the distinct batch's number of edges
    (min(d, f) per row either way -- the synthetic graph has no holes) and at most 0.52 of its nodes.  A per-hop or per-row key lands at
    0.58 or above: the bound is a condition on the statement (one key per node and batch), not a speed claim."""
    import legion1_amd.synth as S
    spec = S.spec_for("products", scale=0.25)
    ds = S.generate(spec, with_features=False)
    zero = np.zeros((spec.V, 1), np.float32)
    B, fan = 2000, [25, 10, 5]
    lab = np.zeros(len(ds.train), np.int32)
    for counter in (0, 3):
        a = D.run_batch(ds.indptr, ds.indices, zero, ds.train, lab, B, counter, fan)
        b = R.run_batch(ds.indptr, ds.indices, zero, ds.train, lab, B, counter, fan)
        na, nb = int(a["nc"][5 + 2 * 3]), int(b["nc"][5 + 2 * 3])
        ea, eb = int(a["ec"][2 + 3]), int(b["ec"][2 + 3])
        print("batch %d: distinct %d nodes, shared key %d nodes (%.3f), edges %d / %d" % (counter, na, nb, nb / na, ea, eb))
        assert ea == eb > 0
        assert nb <= 0.52 * na


# ---- parser and boot ----------------------------------------------------------------------------------
ACCEPTED = "Server_Initialize: the synth: dataset path names no known workload / scale"
NEEDS_KIND = "Server_Initialize: LEGION_SHARED_DRAWS=1 needs LEGION_SAMPLING=distinct: the flag keys the distinct draws by the neighbour node"
NEEDS_SEED = ("Server_Initialize: LEGION_SHARED_DRAWS=1 needs LEGION_SAMPLING_SEED: the node keys come from the batch's draw word, and without a seed "
              "every batch of every epoch would prefer the same nodes")


@pytest.mark.parametrize("sampling,seed,flag,fanout,said", [
    ("distinct", "7", "1", "25,10", ACCEPTED),
    ("distinct", "0", "1", "64,2", ACCEPTED),                            # seed 0 is a seed
    ("distinct", None, None, "10,5", ACCEPTED),
    ("distinct", None, "", "10,5", ACCEPTED),
    ("distinct", None, "0", "10,5", ACCEPTED),
    (None, None, "0", "10,5", ACCEPTED),
    ("distinct", None, "1", "10,5", NEEDS_SEED),
    (None, "7", "1", "10,5", NEEDS_KIND),
    ("replace", "7", "1", "10,5", NEEDS_KIND),
    ("weighted", "7", "1", "10,5", NEEDS_KIND),
    ("distinct", "7", "2", "10,5", "Server_Initialize: LEGION_SHARED_DRAWS=2 is not a known setting: `1` (distinct draws by a key of the neighbour node: rows that see "
                                   "the same neighbours pick the same ones), `0` or unset"),
    ("distinct", "7", "on", "10,5", "Server_Initialize: LEGION_SHARED_DRAWS=on is not a known setting"),
    ("distinct", "7", "1", "65,2", "Server_Initialize: LEGION_SHARED_DRAWS=1 takes fan-outs of at most 64, hop 1 has 65: k_sample keeps a row's best picks one per lane "
                                   "and stages them in static LDS"),
    ("distinct", "7", "1", "10,70", "Server_Initialize: LEGION_SHARED_DRAWS=1 takes fan-outs of at most 64, hop 2 has 70"),
])
def test_boot_parses_the_flag(tmp_path, sampling, seed, flag, fanout, said):
    """serve_modes_from_env and serve_modes_fit_fanout through the server's boot.  Every refusal comes before a device is touched: this
    machine has none, and the accepted settings get as far as the synth: source."""
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write("synth:nosuchworkload 512 1000 0 16 100 0 0 %d 1 0\n" % (1 << 30))
    env = {k: v for k, v in os.environ.items() if k not in MODE_VARS}
    env.update(LEGION_IPC_NAMESPACE="cpusd%d_" % os.getpid())
    for name, value in (("LEGION_SAMPLING", sampling), ("LEGION_SAMPLING_SEED", seed), ("LEGION_SHARED_DRAWS", flag)):
        if value is not None:
            env[name] = value
    r = subprocess.run([SERVER, "1", "0", fanout, meta], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 1 and said in out, out[-2000:]


# ---- the pool's flag, without a device ----------------------------------------------------------------
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
        assert L.GPUMemoryPool_GetSharedDraws(pool) == 0 and L.GPUMemoryPool_GetSharedDraws(None) == 0
        L.GPUMemoryPool_SetSampling(pool, 1)
        for on, want in ((1, 1), (0, 0), (7, 1)):
            L.GPUMemoryPool_SetSharedDraws(pool, on)
            assert not err() and L.GPUMemoryPool_GetSharedDraws(pool) == want
            assert L.GPUMemoryPool_GetSampling(pool) == 1 and L.GPUMemoryPool_GetSampleDistinct(pool) == 1    # a flag, not a fourth kind: still "distinct"
            assert L.GPUMemoryPool_GetWeightedDistinct(pool) == 0
        for kind in (0, 1, 2):                                               # the flag is remembered across kinds
            L.GPUMemoryPool_SetSampling(pool, kind)
            assert not err() and L.GPUMemoryPool_GetSampling(pool) == kind and L.GPUMemoryPool_GetSharedDraws(pool) == 1
        L.GPUMemoryPool_SetSampling(pool, 0)
        L.GPUMemoryPool_SetSharedDraws(pool, 0)                              # ... and may be set under any kind
        L.GPUMemoryPool_SetSharedDraws(pool, 1)
        assert not err() and L.GPUMemoryPool_GetSampling(pool) == 0 and L.GPUMemoryPool_GetSharedDraws(pool) == 1
        L.GPUMemoryPool_SetSampling(pool, 3)                                 # still no fourth kind
        assert "GPUMemoryPool_SetSampling: unknown sampling kind (0 = replace, 1 = distinct, 2 = weighted)" in err()
        L.GPUMemoryPool_SetSharedDraws(None, 1)
        assert "GPUMemoryPool_SetSharedDraws: null pool" in err()
        L.legion_shared_draw_probe(None, None, None, None, 4)
        assert "legion_shared_draw_probe: null array" in err()
    finally:
        L.legion_clear_error()
        L.GPUMemoryPool_Delete(pool)


# ---- launcher and Python surface ----------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["--shared-draws", "--shared_draws", None])
def test_launch_server_passes_the_flag_on(tmp_path, flag):
    work = tmp_path / "pkg"
    (work / "csrc").mkdir(parents=True)
    (work / "launch_server.py").write_text(open(os.path.join(ROOT, "legion-1_amd", "launch_server.py")).read())
    stand_in = work / "csrc" / "legion"
    stand_in.write_text("#!/bin/sh\necho \"SAMPLING=[${LEGION_SAMPLING}] SEED=[${LEGION_SAMPLING_SEED}] SD=[${LEGION_SHARED_DRAWS}]\"\n")
    stand_in.chmod(0o755)
    env = {k: v for k, v in os.environ.items() if k not in MODE_VARS}
    r = subprocess.run([sys.executable, str(work / "launch_server.py"), "--dataset", "PR", "--gpu_number", "1", "--sampling", "distinct", "--sampling_seed", "7"]
                       + ([flag] if flag else []), cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=60)
    assert "SAMPLING=[distinct] SEED=[7] SD=[%s]" % ("1" if flag else "") in r.stdout, r.stdout + r.stderr


def test_capi_table_and_header_name_the_new_symbols():
    import legion1_amd.capi as K
    L = K.lib()
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    for name in ("GPUMemoryPool_SetSharedDraws", "GPUMemoryPool_GetSharedDraws", "legion_shared_draw_probe"):
        assert name in K._SIGS and name + "(" in header and getattr(L, name)


def test_engine_refuses_the_flag_without_the_distinct_kind_before_it_touches_anything():
    import legion1_amd.capi as K
    eng = K.Engine.__new__(K.Engine)            # no device: _set_modes validates its arguments first
    for sample in ("replace", "weighted"):
        with pytest.raises(ValueError, match="shared_draws=True needs sample='distinct'"):
            eng._set_modes(0, False, None, sample, None, 0, None, shared_draws=True)
