"""Drawn link-prediction thirds (GPUMemoryPool_SetLpDraw / LEGION_LP_DRAW, INTEGRATION.md "Drawn link-prediction thirds"), the parts that
need no GPU: the NumPy statement of tests/lpref.py against its known answers and its own properties, the boot of the `legion` binary under
LEGION_LP_DRAW, and the pool's setter on a pool without scratch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lpref as P
from conftest import ROOT
from distinctcases import random_graph
from seededref import Ks, W, perm

SERVER = os.path.join(ROOT, "legion-1_amd", "csrc", "legion")
# what the boot says when the modes were accepted: the meta line names a synth: workload that does not exist, which Server_Initialize
# refuses right behind the modes and before any device is touched
ACCEPTED = "Server_Initialize: the synth: dataset path names no known workload / scale"
MODE_VARS = ("LEGION_AGG_LAST_HOP", "LEGION_AGG_NORM", "LEGION_SAMPLING", "LEGION_SAMPLING_SEED", "LEGION_LP_DRAW")


# ---------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------
def test_known_answers():
    w = W(12345, 3, 2)
    assert w == 0xd66bf856 and P.keys(w) == (0xf622a3ef, 0xf89d4487)
    for (i, src, d), want in (((0, 0, 1000), 121), ((1, 0, 1000), 995), ((21, 499, 7), 5), ((2666, 111059955, 2 ** 31 - 1), 1052666731), ((0, 5, 1), 0)):
        assert int(P.rho(w, [i], [src], [d])[0]) == want, (i, src, d)
    for (i, src, V), want in (((0, 0, 500), 153), ((1, 0, 500), 453), ((21, 499, 111059956), 52733101), ((2666, 111059955, 2 ** 31 - 1), 393912042), ((0, 5, 1), 0)):
        assert int(P.neg(w, [i], [src], V)[0]) == want, (i, src, V)
    w = W(0, 0, 0)
    assert w == 0x77bb992c and P.keys(w) == (0x049153fc, 0xc8677817)
    assert int(P.rho(w, [0], [0], [10])[0]) == 4 and int(P.neg(w, [0], [0], 10)[0]) == 7
    assert P.rho(w, [0, 1, 2], [3, 4, 5], [0, -1, -2 ** 31]).tolist() == [-1, -1, -1]
    assert perm(110, Ks(12345, 3))[:8].tolist() == [97, 64, 43, 85, 38, 66, 104, 99]


@pytest.mark.parametrize("k", [22, 171])
def test_drawn_list_properties(k):
    V = 500
    indptr, indices, labels = random_graph(1, V, holes=True)
    L = P.toy_list(indptr, V, k, 5)
    Lab = np.arange(len(L), dtype=np.int32)                  # a label per list entry: shows which entry a slot came from
    n, T = len(L), len(L) // 3
    file_src = L.reshape(-1, 3, k)[:, 0, :].reshape(-1)
    lists = {}
    for r in (0, 1):
        ids, lab = P.drawn_list(indptr, indices, L, Lab, k, V, 12345, r)
        lists[r] = ids
        b = ids.reshape(-1, 3, k)
        src, pos, neg = b[:, 0, :].reshape(-1), b[:, 1, :].reshape(-1), b[:, 2, :].reshape(-1)
        assert np.array_equal(np.sort(src), np.sort(file_src))                      # a permutation of the file's triples' sources
        sl, _ = P.triple_shuffled(L, Lab, k, 12345, r)
        assert np.array_equal(np.sort(sl.reshape(-1, 3, k), axis=None), np.sort(L)) and np.array_equal(sl.reshape(-1, 3, k)[:, 0, :].reshape(-1), src)
        tl = P.triple_perm_index(n, k, 12345, r).reshape(-1, 3, k)                   # a triple moves as a whole
        assert np.array_equal(tl[:, 1, :] - tl[:, 0, :], np.full((n // (3 * k), k), k)) and np.array_equal(tl[:, 2, :] - tl[:, 0, :], np.full((n // (3 * k), k), 2 * k))
        assert len(np.unique(tl[:, 0, :])) == T
        lb = lab.reshape(-1, 3, k)
        assert (lb[:, 1:, :] == -1).all() and np.array_equal(L[lb[:, 0, :].reshape(-1)], src)
        empty = 0
        for s, p in zip(src.tolist(), pos.tolist()):
            row = indices[indptr[s]:indptr[s + 1]]
            assert p in row[row >= 0] or p == s
            empty += len(row) == 0 and p == s
        assert empty >= 1
        assert ((neg >= 0) & (neg < V)).all()
    assert not np.array_equal(lists[0], lists[1])
    b0 = lists[0].reshape(-1, 3, k)
    assert not np.array_equal(b0[0, 2], b0[1, 2]) and not np.array_equal(b0[0], b0[1])
    ids_fo, _ = P.drawn_list(indptr, indices, L, Lab, k, V, 12345, 0, shuffle=False)
    assert np.array_equal(ids_fo.reshape(-1, 3, k)[:, 0, :].reshape(-1), file_src)


@pytest.mark.parametrize("seed", [(12345, 3, 2), (0, 0, 0), (0xFFFFFFFF, 7, 40)], ids=lambda s: "%x-%d-%d" % s)
def test_uniformity(seed):
    """30 000 negatives into V = 10 bins and 30 000 positions at d = 7: every bin within 5 sigma of the binomial expectation."""
    n = 30000
    w = W(*seed)
    i = np.arange(n)
    src = np.random.RandomState(3).randint(0, 2 ** 31 - 1, size=n)
    worst = 0.0
    for got, bins in ((P.neg(w, i, src, 10), 10), (P.rho(w, i, src, np.full(n, 7)), 7)):
        cnt = np.bincount(got, minlength=bins)
        assert len(cnt) == bins
        p = 1.0 / bins
        z = np.abs(cnt - n * p) / np.sqrt(n * p * (1 - p))
        worst = max(worst, float(z.max()))
    print("largest deviation: %.2f sigma" % worst)
    assert worst <= 5.0


# ---------------------------------------------------------------------------------------------------
# the boot
# ---------------------------------------------------------------------------------------------------
LP_META = "synth:nosuchworkload %d 1000 0 16 100 0 0 %d 1 %d\n"
NEEDS_SEED = "Server_Initialize: LEGION_LP_DRAW=1 needs LEGION_SAMPLING_SEED: the thirds are drawn from the batch's draw word"
UNKNOWN = "Server_Initialize: LEGION_LP_DRAW=%s is not a known setting: `1` (the pos and neg thirds of link-prediction batches are drawn per batch), `0` or unset"
BOOTS = [
    (510, 2, dict(LEGION_LP_DRAW="1", LEGION_SAMPLING_SEED="12345"), None),
    (510, 2, dict(LEGION_LP_DRAW="0"), None), (512, 0, dict(LEGION_LP_DRAW=""), None), (512, 0, dict(LEGION_LP_DRAW="0", LEGION_SAMPLING_SEED="1"), None),
    (510, 2, dict(LEGION_LP_DRAW="1"), NEEDS_SEED),
    (510, 2, dict(LEGION_LP_DRAW="2", LEGION_SAMPLING_SEED="12345"), UNKNOWN % "2"),
    (510, 2, dict(LEGION_LP_DRAW="yes", LEGION_SAMPLING_SEED="12345"), UNKNOWN % "yes"),
    (510, 0, dict(LEGION_LP_DRAW="1", LEGION_SAMPLING_SEED="12345"), "Server_Initialize: LEGION_LP_DRAW=1 needs link-prediction training lists (meta flag 2: [src | pos | neg] thirds per batch)"),
    (512, 2, dict(LEGION_LP_DRAW="1", LEGION_SAMPLING_SEED="12345"), "Server_Initialize: LEGION_LP_DRAW=1 needs a batch size divisible by 3 ([src | pos | neg] thirds), the meta line has 512"),
]


@pytest.mark.parametrize("B,flag,env_vars,refusal", [pytest.param(*c, id="%d-%d-" % c[:2] + ",".join("%s=%s" % (k[7:], v) for k, v in c[2].items())) for c in BOOTS])
def test_boot_parses_lp_draw(tmp_path, B, flag, env_vars, refusal):
    """The `legion` binary's boot: exit code 1 and exactly one Server_Initialize refusal -- the one the table names, or, for an accepted
    setting, that of the check behind the modes (the meta line names a synth: workload that does not exist).  No device is touched."""
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write(LP_META % (B, 1 << 30, flag))
    env = {k: v for k, v in os.environ.items() if k not in MODE_VARS}
    env.update(env_vars, LEGION_IPC_NAMESPACE="cpulp%d_" % os.getpid())
    r = subprocess.run([SERVER, "1", "0", "10,5", meta], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    said = r.stdout + r.stderr
    assert r.returncode == 1 and (refusal or ACCEPTED) in said, said[-2000:]
    assert len(set(re.findall(r"Server_Initialize: .*", said))) == 1, said[-2000:]


def test_launch_server_sets_the_variable(tmp_path):
    """launch_server.py --lp_draw: LEGION_LP_DRAW=1 reaches the server process (a stand-in that prints it), beside the seed it needs;
    without the flag the caller's environment passes through."""
    work = tmp_path / "pkg"
    (work / "csrc").mkdir(parents=True)
    (work / "launch_server.py").write_text(open(os.path.join(ROOT, "legion-1_amd", "launch_server.py")).read())
    stand_in = work / "csrc" / "legion"
    stand_in.write_text("#!/bin/sh\necho \"LP=[${LEGION_LP_DRAW}] SEED=[${LEGION_SAMPLING_SEED}]\"\n")
    stand_in.chmod(0o755)
    env = {k: v for k, v in os.environ.items() if k not in MODE_VARS}

    def run(*flags, **more):
        return subprocess.run([sys.executable, str(work / "launch_server.py"), "--dataset", "PR", "--gpu_number", "1"] + list(flags),
                              cwd=str(tmp_path), env=dict(env, **more), capture_output=True, text=True, timeout=60)

    assert "LP=[1] SEED=[12345]" in run("--lp_draw", "--sampling_seed", "12345").stdout
    assert "LP=[1] SEED=[]" in run("--lp_draw", LEGION_LP_DRAW="0").stdout          # the flag wins; the server refuses the missing seed
    assert "LP=[] SEED=[7]" in run("--sampling_seed", "7").stdout
    assert "LP=[] SEED=[]" in run().stdout
    assert "LP=[0] SEED=[]" in run(LEGION_LP_DRAW="0").stdout
    r = run("--help")
    assert r.returncode == 0 and "--lp_draw" in r.stdout and "LEGION_LP_DRAW=1" in r.stdout


# ---------------------------------------------------------------------------------------------------
# the pool's setter (no scratch: no device is touched)
# ---------------------------------------------------------------------------------------------------
@pytest.fixture
def pool_lib():
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    pool = L.NewGPUMemoryPool(2)            # no scratch: no setter touches a device
    yield L, pool
    L.legion_clear_error()
    L.GPUMemoryPool_Delete(pool)


def pool_modes(L, pool):
    """The five mode values that are not lp_draw."""
    seed = C.c_uint32(99)
    on = L.GPUMemoryPool_GetSampleSeed(pool, C.byref(seed))
    return (L.GPUMemoryPool_GetAggLastHop(pool), L.GPUMemoryPool_GetAggNorm(pool), L.GPUMemoryPool_GetSampleDistinct(pool), on, seed.value)


def last_error(L):
    msg = (L.legion_last_error() or b"").decode()
    L.legion_clear_error()
    return msg


def test_get_equals_set_and_the_other_modes_do_not_move(pool_lib):
    L, pool = pool_lib
    graph = L.NewGPUMemoryGraphStorage()
    try:
        L.GPUMemoryPool_SetSampleSeed(pool, 1, 77)
        L.GPUMemoryPool_SetSampleDistinct(pool, 1)
        others = pool_modes(L, pool)
        assert others == (0, 0, 1, 1, 77) and L.GPUMemoryPool_GetLpDraw(pool) == 0 and L.GPUMemoryPool_GetLpDraw(None) == 0
        for k in (170, 1, 0, 2666, 0):
            L.GPUMemoryPool_SetLpDraw(pool, k, graph)
            assert not L.legion_last_error(), last_error(L)
            assert L.GPUMemoryPool_GetLpDraw(pool) == k and pool_modes(L, pool) == others
        L.GPUMemoryPool_SetLpDraw(pool, 22, graph)
        L.GPUMemoryPool_SetLpDraw(None, 5, graph)
        assert last_error(L).count("GPUMemoryPool_SetLpDraw: null pool") == 1
        L.GPUMemoryPool_SetLpDraw(pool, 5, None)
        assert last_error(L).count("GPUMemoryPool_SetLpDraw: null graph") == 1
        L.GPUMemoryPool_SetLpDraw(pool, -1, graph)
        assert last_error(L).count("GPUMemoryPool_SetLpDraw: negative triples per batch") == 1
        assert L.GPUMemoryPool_GetLpDraw(pool) == 22 and pool_modes(L, pool) == others      # a refusal leaves the pool as it was
        L.GPUMemoryPool_SetAggLastHop(pool, 1)                                             # ... and the other setters leave lp_draw alone
        L.GPUMemoryPool_SetSampleSeed(pool, 1, 78)
        assert not L.legion_last_error() and L.GPUMemoryPool_GetLpDraw(pool) == 22
        L.GPUMemoryPool_SetLpDraw(pool, 0, None)                                            # off needs no graph
        assert not L.legion_last_error() and L.GPUMemoryPool_GetLpDraw(pool) == 0
    finally:
        L.legion_clear_error()
        L.GPUGraphStorage_Delete(graph)
