"""The distinct-draw sampler mode on the CPU: the NumPy statement of tests/distinctref.py against its scalar twin, the known answers, the
properties a sampler without replacement must have, the bookkeeping against tests/pyref.py, and the uniformity of the positions."""
import os
import subprocess
import sys

import numpy as np
import pytest

import distinctref as D
import pyref
from conftest import ROOT
from harness import device_free_server

H_GRID = (1, 2, 3, 4)
F_GRID = (1, 2, 5, 10, 25, 64)


def d_grid(f):
    return (f + 1, f + 2, 2 * f, 3 * f + 1, 10 * f + 3, 1000 + f)


def test_mix32_known_answers():
    assert D.mix32_scalar(1) == 0x688990c0
    assert D.mix32_scalar(0x9E3779B9) == 0x01fce552
    assert D.mix32([1, 0x9E3779B9]).tolist() == [0x688990c0, 0x01fce552]


def test_picks_known_answers():
    assert D.picks_scalar(0, 1, 6, 5) == [0, 2, 3, 4, 5]
    assert D.picks_scalar(12345, 3, 1000, 25)[:8] == [85, 698, 268, 619, 680, 723, 544, 143]
    assert D.picks_scalar(199999, 1, 2000000000, 5) == [1067425008, 1935742059, 137284816, 1563980815, 1023845666]
    assert D.positions([0], 1, [6], 5).tolist() == [[0, 2, 3, 4, 5]]
    assert D.positions([12345], 3, [1000], 25)[0, :8].tolist() == [85, 698, 268, 619, 680, 723, 544, 143]
    assert D.positions([199999], 1, [2000000000], 5).tolist() == [[1067425008, 1935742059, 137284816, 1563980815, 1023845666]]


def test_vectorised_equals_scalar():
    rng = np.random.RandomState(7)
    for f in (1, 2, 3, 5, 10, 25, 40, 64):
        n = 400
        rows = rng.randint(0, 2 ** 31 - 1, size=n).astype(np.int64)
        hop = rng.randint(1, 5, size=n)
        deg = np.concatenate([rng.randint(-1, 3 * f + 2, size=n - 40), rng.randint(f + 1, 2 ** 31 - 1, size=40)]).astype(np.int64)
        got = D.positions(rows, hop, deg, f)
        for m in range(n):
            assert got[m].tolist() == D.picks_scalar(int(rows[m]), int(hop[m]), int(deg[m]), f), (f, m, rows[m], hop[m], deg[m])
        one = D.positions(rows, 3, deg, f)                      # a scalar hop broadcasts
        assert one[5].tolist() == D.picks_scalar(int(rows[5]), 3, int(deg[5]), f)


@pytest.mark.parametrize("f", F_GRID + (3, 40))
def test_positions_are_distinct_and_in_range(f):
    rng = np.random.RandomState(f)
    n = 20000
    rows = np.arange(n, dtype=np.int64) + rng.randint(0, 1 << 20)
    for h in H_GRID:
        deg = rng.choice(np.array(d_grid(f) + (f + 3, 7 * f, 2 ** 31 - 1)), size=n).astype(np.int64)
        p = D.positions(rows, h, deg, f)
        assert p.shape == (n, f) and (p >= 0).all() and (p < deg[:, None]).all()
        s = np.sort(p, axis=1)
        assert (s[:, 1:] != s[:, :-1]).all()


@pytest.mark.parametrize("f", (1, 2, 5, 25, 64))
def test_small_degrees_take_every_neighbour_once_in_csr_order(f):
    rows = np.arange(3 * (f + 2), dtype=np.int64)
    deg = np.tile(np.arange(-1, f + 1, dtype=np.int64), 3)
    for h in H_GRID:
        p = D.positions(rows, h, deg, f)
        for m in range(len(rows)):
            d = max(int(deg[m]), 0)
            assert p[m].tolist() == list(range(d)) + [-1] * (f - d)


def test_edge_cases():
    # f = 1: one position, any of the d
    p = D.positions(np.arange(50000), 2, np.full(50000, 7), 1)
    assert set(p[:, 0].tolist()) == set(range(7))
    # d = f + 1: exactly one neighbour is left out, and every one of them is left out for some row
    for f in (1, 5, 64):
        p = D.positions(np.arange(40000), 1, np.full(40000, f + 1), f)
        left = (f + 1) * f // 2 - p.sum(axis=1)
        assert ((left >= 0) & (left <= f)).all() and set(left.tolist()) == set(range(f + 1))
        assert (np.sort(p, axis=1)[:, 1:] != np.sort(p, axis=1)[:, :-1]).all()
    # f = 64, the largest fan-out of the mode
    p = D.positions(np.arange(3000), 4, np.full(3000, 100), 64)
    assert all(len(set(r)) == 64 for r in p.tolist()) and p.max() == 99 and p.min() == 0
    # d near 2^31: no overflow, the positions stay int32 neighbour positions
    big = np.array([2 ** 31 - 1, 2 ** 31 - 2, 2 ** 31 - 65, 2000000000], dtype=np.int64)
    for f in (1, 5, 64):
        p = D.positions(np.arange(4) + 199999, 1, big, f)
        assert (p >= 0).all() and (p < big[:, None]).all() and p.max() > 2 ** 30
        for m in range(4):
            assert p[m].tolist() == D.picks_scalar(199999 + m, 1, int(big[m]), f)


def small_graph(seed, V=300, holes=True):
    rng = np.random.RandomState(seed)
    deg = rng.randint(0, 12, size=V)
    deg[rng.randint(0, V, 4)] = 90
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.randint(-1 if holes else 0, V, size=int(indptr[-1])).astype(np.int32)
    labels = rng.randint(0, 9, size=V).astype(np.int32)
    feats = rng.rand(V, 5).astype(np.float32)
    seeds = rng.permutation(V)[:97].astype(np.int32)
    return indptr, indices, feats, labels, seeds


@pytest.mark.parametrize("seed", [0, 1])
def test_bookkeeping_is_pyrefs(seed):
    """With the draw function swapped for the default mode's, the whole-batch statement IS pyref.run_batch: the new bookkeeping is the old one."""
    indptr, indices, feats, labels, seeds = small_graph(seed)
    dup = np.concatenate([seeds[:20], seeds[5:15]])             # a seed list that repeats seeds inside a batch
    for fan, B, ids in (([3, 2], 40, seeds), ([5, 4, 3], 50, seeds), ([4], 30, dup), ([2, 2, 2, 2], 7, seeds), ([6, 3], 97, seeds)):
        lab = labels[ids]
        for counter in range(min(3, (len(ids) + B - 1) // B)):
            want = pyref.run_batch(indptr, indices, feats, ids, lab, B, counter, fan)
            got = D.run_batch(indptr, indices, feats, ids, lab, B, counter, fan, draw=D.pyref_positions)
            for k in want:
                assert np.array_equal(want[k], got[k]) and want[k].dtype == got[k].dtype, (fan, counter, k)


def test_whole_batch_draws_distinct_neighbours():
    """On a graph without multi-edges and holes every (input slot, neighbour id) pair of a hop occurs once, and a row gives min(d, f) edges."""
    V = 400
    rng = np.random.RandomState(3)
    deg = rng.randint(0, 30, size=V)
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = np.concatenate([rng.permutation(V)[:d] for d in deg]).astype(np.int32)
    feats, labels = rng.rand(V, 3).astype(np.float32), rng.randint(0, 5, size=V).astype(np.int32)
    seeds = rng.permutation(V)[:64].astype(np.int32)
    fan = [10, 5, 3]
    b = D.run_batch(indptr, indices, feats, seeds, labels[seeds], 64, 0, fan)
    for h, f in enumerate(fan):
        dr = b["draws"][h].reshape(-1, f)
        inp, cnt = b["draw_counts"][h]
        assert np.array_equal(cnt, np.minimum(deg[inp], f))
        for row, c in zip(dr.tolist(), cnt.tolist()):
            assert len(set(row[:c])) == c and all(x == -1 for x in row[c:])
    assert b["ec"][2 + 3] == sum(int(c.sum()) for _, c in b["draw_counts"])


@pytest.mark.parametrize("row0", [0, 3000000])
@pytest.mark.parametrize("f", F_GRID)
def test_uniformity(f, row0):
    """Per case (h, f, d), 200 000 rows: X = sum (c_k - e)^2 / e * (d - 1) / (d - f) over the position counts c_k, e = n f / d, is chi-square
    with d - 1 degrees of freedom under exchangeable sampling without replacement; it must not exceed the quantile at 1 - 1e-6."""
    n = 200000
    rows = np.arange(row0, row0 + n, dtype=np.int64)
    worst = 0.0
    for h in H_GRID:
        for d in d_grid(f):
            p = D.positions(rows, h, np.full(n, d, dtype=np.int64), f)
            c = np.bincount(p.reshape(-1), minlength=d).astype(np.float64)
            assert len(c) == d
            e = n * f / d
            X = float(((c - e) ** 2 / e).sum() * (d - 1) / (d - f))
            cap = D.chi2_cap(d - 1)
            worst = max(worst, X / cap)
            print("h=%d f=%d d=%d rows %d..: X = %.2f, cap %.2f" % (h, f, d, row0, X, cap))
            assert X <= cap, (h, f, d, row0, X, cap)
    print("f=%d rows %d..: largest X / cap = %.3f" % (f, row0, worst))


# ---- the switch through the layers that need no GPU ------------------------------------------------
def test_capi_table_and_header_name_the_new_symbols():
    import legion1_amd.capi as K
    L = K.lib()
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    for name in ("GPUMemoryPool_SetSampleDistinct", "GPUMemoryPool_GetSampleDistinct", "IPCEnv_SetSampling", "IPCEnv_GetSampling",
                 "legion_ipc_client_sampling", "legion_distinct_probe"):
        assert name in K._SIGS and name + "(" in header and getattr(L, name)


def test_pool_switch_without_a_gpu():
    """The mode lives in the pool: off by default, set and read back without a device (nothing is allocated); a null pool is refused by name."""
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    pool = L.NewGPUMemoryPool(2)
    try:
        assert L.GPUMemoryPool_GetSampleDistinct(pool) == 0
        for on, want in ((1, 1), (0, 0), (7, 1), (0, 0)):
            L.GPUMemoryPool_SetSampleDistinct(pool, on)
            assert not L.legion_last_error() and L.GPUMemoryPool_GetSampleDistinct(pool) == want
        L.GPUMemoryPool_SetSampleDistinct(None, 1)
        assert "GPUMemoryPool_SetSampleDistinct: null pool" in (L.legion_last_error() or b"").decode()
        assert L.GPUMemoryPool_GetSampleDistinct(None) == 0
    finally:
        L.legion_clear_error()
        L.GPUMemoryPool_Delete(pool)


def test_sampling_word_round_trip_without_a_gpu():
    """The word behind agg_norm in the "<name>_ext" object, with the device-free IPC env: a server sets it, a client process reads it (0
    from a server that never set it) and every older word it reads is where it was; in the mapped object the three words are neighbours,
    agg_last_hop, agg_norm, sampling; ipc_service.sampling() names the mode."""
    ns = "cpuipc_samp%d_" % os.getpid()
    pre, _ = device_free_server(ns, 3, "")
    client = pre + ("sys.path.insert(0, %r)\nimport legion1_amd.capi as K\nL = K.lib(); L.legion_set_error_mode(K.ERR_RETURN)\n"
                    "c = C.c_void_p(L.legion_ipc_client_open(0)); K.check(); assert c.value\n"
                    "s = (C.c_int32 * 3)(); L.legion_ipc_client_steps(c, s)\n"
                    "print('CLIENT', L.legion_ipc_client_sampling(c), L.legion_ipc_client_agg_norm(c), L.legion_ipc_client_agg_last_hop(c), "
                    "L.legion_ipc_client_hops(c), L.legion_ipc_client_feature_rows(c), list(s)); L.legion_ipc_client_close(c)\n"
                    "import torch, ipc_service\nipc_service.initialize(); print('SERVICE', ipc_service.sampling()); ipc_service.finalize()\n"
                    ) % os.path.join(ROOT, "legion-1_amd", "ipc_service")
    body = ("assert L.IPCEnv_GetSampling(e) == 0\n"
            "L.IPCEnv_SetFeatureRows(e, 0, 4321)\n"
            "ext = [f for f in os.listdir('/dev/shm') if %r in f and f.endswith('_ext')]; assert len(ext) == 1, ext\n"
            "words = lambda: np.fromfile('/dev/shm/' + ext[0], dtype=np.int32)\n"
            "where = {}\n"
            "for name, setter in (('agg', L.IPCEnv_SetAggLastHop), ('norm', L.IPCEnv_SetAggNorm), ('sampling', L.IPCEnv_SetSampling)):\n"
            "    w0 = words(); setter(e, 1); w1 = words(); setter(e, 0)\n"
            "    changed = np.nonzero(w0 != w1)[0]; assert len(changed) == 1 and w1[changed[0]] == 1, (name, changed)\n"
            "    where[name] = int(changed[0])\n"
            "assert where['norm'] == where['agg'] + 1 and where['sampling'] == where['norm'] + 1, where\n"
            "for agg, norm, samp in ((0, 0, 0), (0, 0, 1), (1, 1, 1), (1, 0, 1), (1, 1, 0)):\n"
            "    L.IPCEnv_SetAggLastHop(e, agg); L.IPCEnv_SetAggNorm(e, norm); L.IPCEnv_SetSampling(e, samp)\n"
            "    assert (L.IPCEnv_GetSampling(e), L.IPCEnv_GetAggNorm(e), L.IPCEnv_GetAggLastHop(e)) == (samp, norm, agg)\n"
            "    r = subprocess.run([sys.executable, '-c', %r], capture_output=True, text=True, timeout=120)\n"
            "    print(r.stdout.strip(), r.stderr[-500:]); assert 'CLIENT %%d %%d %%d 3 4321 [7, 2, 1]' %% (samp, norm, agg) in r.stdout\n"
            "    assert 'SERVICE ' + ('distinct' if samp else 'replace') in r.stdout\n") % (ns, client)
    _, server = device_free_server(ns, 3, body)
    r = subprocess.run([sys.executable, "-c", server], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SERVER_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert not [f for f in os.listdir("/dev/shm") if ns in f]


def test_launch_server_sets_the_variable_for_the_child(tmp_path):
    """launch_server.py --sampling distinct: LEGION_SAMPLING reaches the server process (a stand-in that prints it); without the flag the
    caller's environment passes through; another value is refused by the argument parser."""
    work = tmp_path / "pkg"
    (work / "csrc").mkdir(parents=True)
    src = open(os.path.join(ROOT, "legion-1_amd", "launch_server.py")).read()
    (work / "launch_server.py").write_text(src)
    stand_in = work / "csrc" / "legion"
    stand_in.write_text("#!/bin/sh\necho \"SAMPLING=[${LEGION_SAMPLING}]\"\n")
    stand_in.chmod(0o755)
    env = {k: v for k, v in os.environ.items() if k != "LEGION_SAMPLING"}

    def run(*flags, **more):
        return subprocess.run([sys.executable, str(work / "launch_server.py"), "--dataset", "PR", "--gpu_number", "1"] + list(flags),
                              cwd=str(tmp_path), env=dict(env, **more), capture_output=True, text=True, timeout=60)

    assert "SAMPLING=[distinct]" in run("--sampling", "distinct").stdout
    assert "SAMPLING=[replace]" in run("--sampling", "replace", LEGION_SAMPLING="distinct").stdout
    assert "SAMPLING=[]" in run().stdout
    assert "SAMPLING=[distinct]" in run(LEGION_SAMPLING="distinct").stdout
    r = run("--sampling", "unique")
    assert r.returncode != 0 and "invalid choice" in r.stderr
