"""The weighted sampler mode (LEGION_SAMPLING=weighted, INTEGRATION.md "Weighted sampling"), the parts that need no GPU: the statement of
tests/weightedref.py against itself (what a valid alias table is, and that the statement's draws follow the weights), the environment
parser through the `legion` binary's boot, the launcher's flag, the pool's sampling kind and the trainer's word on a device-free IPC env,
the C ABI's new names, and the synth: source's edge weights."""
import os
import subprocess
import sys

import numpy as np
import pytest

import distinctref as D
import weightedref as Wt
from conftest import ROOT
from harness import device_free_server

SERVER = os.path.join(ROOT, "legion-1_amd", "csrc", "legion")


def graph_with_weights(seed=0, V=300):
    """rows of degree 0..40 and a hub, multi-edges, holes; about one weight in six is 0, the rest span 1e-3 .. 1e3; all-zero rows; one row of
    equal weights and one with a single non-zero weight"""
    rng = np.random.RandomState(seed)
    deg = rng.randint(0, 41, size=V)
    deg[5], deg[6], deg[7] = 700, 9, 12
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    indices = rng.randint(-1, V, size=E).astype(np.int32)
    w = np.where(rng.rand(E) < 1 / 6, 0.0, 10.0 ** rng.uniform(-3, 3, size=E)).astype(np.float32)
    for v in rng.choice(np.nonzero(deg > 0)[0], 12, replace=False):
        w[indptr[v]:indptr[v + 1]] = 0.0
    w[indptr[6]:indptr[7]] = 2.5
    w[indptr[7]:indptr[8]] = 0.0
    w[indptr[7] + 4] = 3.0
    return indptr, indices, w


# ---- what a valid table is ---------------------------------------------------------------------------
def test_check_table_accepts_the_python_builder_and_rejects_five_corruptions():
    indptr, indices, w = graph_with_weights()
    thr, alias = Wt.build_table(indptr, indices, w)
    worst = Wt.check_table(indptr, indices, w, thr, alias)
    print("largest |P - share| of the Python builder's table: %.3g (bound %.3g)" % (worst, Wt.P_BOUND))
    deg = np.diff(indptr)
    Wrow = np.add.reduceat(np.concatenate([w.astype(np.float64), [0.0]]), np.minimum(indptr[:-1], len(w)))
    live = [v for v in range(len(deg)) if deg[v] >= 5 and Wrow[v] > 0 and w[indptr[v]:indptr[v + 1]].min() == 0 and v not in (5, 6, 7)]
    assert live

    def rejected(words, thr2, alias2):
        with pytest.raises(AssertionError) as ex:
            Wt.check_table(indptr, indices, w, thr2, alias2)
        assert all(x in str(ex.value) for x in words), (words, str(ex.value))

    # 1. a threshold off by 2^8: 2^8 / (d 2^32) of row 5's 700 columns is 8.5e-11 < 2^-30, so take a short row, where it is 2^-24 / d
    v = next(u for u in live if deg[u] <= 16)
    k = next(c for c in range(indptr[v], indptr[v + 1]) if 1 << 8 <= thr[c] < Wt.TWO32 - (1 << 9) and alias[c] != indices[c])
    t2 = thr.copy(); t2[k] += 1 << 8
    rejected(("row %d," % v, "its share of the weight"), t2, alias)
    # 2. an alias id outside the row
    a2 = alias.copy()
    outside = next(i for i in range(len(deg)) if i not in set(indices[indptr[v]:indptr[v + 1]].tolist()))
    k = next(c for c in range(indptr[v], indptr[v + 1]) if thr[c] < Wt.TWO32 - 1)
    a2[k] = outside
    rejected(("aliases id %d" % outside, "no neighbour of the row"), thr, a2)
    # 3. mass given to an id whose columns all weigh 0
    ids_v, w_v = indices[indptr[v]:indptr[v + 1]], w[indptr[v]:indptr[v + 1]]
    ghost = next(int(i) for i in ids_v if w_v[ids_v == i].sum() == 0)
    k = indptr[v] + int(np.nonzero(ids_v == ghost)[0][0])
    t3 = thr.copy(); t3[k] = 1
    rejected(("whose columns all weigh 0",), t3, alias)
    # 4. two rows swapped (same degree, different neighbours)
    u1, u2 = next((a, b) for a in live for b in live if a < b and deg[a] == deg[b])
    t4, a4 = thr.copy(), alias.copy()
    for arr in (t4, a4):
        tmp = arr[indptr[u1]:indptr[u1 + 1]].copy()
        arr[indptr[u1]:indptr[u1 + 1]] = arr[indptr[u2]:indptr[u2 + 1]]
        arr[indptr[u2]:indptr[u2 + 1]] = tmp
    with pytest.raises(AssertionError):
        Wt.check_table(indptr, indices, w, t4, a4)
    # 5. an all-zero row that is not the sentinel
    z = next(u for u in range(len(deg)) if deg[u] > 0 and Wrow[u] == 0)
    t5, a5 = thr.copy(), alias.copy()
    t5[indptr[z]], a5[indptr[z]] = Wt.TWO32 - 1, indices[indptr[z]]
    rejected(("all-zero row %d" % z, "not {0, -1}"), t5, a5)
    # ... and the sentinel in a row that has weight
    t6, a6 = thr.copy(), alias.copy()
    t6[indptr[6]:indptr[7]], a6[indptr[6]:indptr[7]] = 0, -1
    if -1 not in indices[indptr[6]:indptr[7]]:
        with pytest.raises(AssertionError):
            Wt.check_table(indptr, indices, w, t6, a6)


def test_python_builder_special_rows():
    assert Wt.vose_row([4, 5, 6], [0, 0, 0]) == ([0, 0, 0], [-1, -1, -1])
    assert Wt.vose_row([4, 5, 6], [2, 2, 2]) == ([Wt.TWO32 - 1] * 3, [4, 5, 6])                # equal weights: every column keeps itself
    thr, alias = Wt.vose_row([4, 5, 6, 7], [0, 0, 3, 0])
    assert thr == [0, 0, Wt.TWO32 - 1, 0] and alias == [6, 6, 6, 6]                            # a single weight: every draw is that neighbour
    assert Wt.vose_row([], []) == ([], [])
    thr, alias = Wt.vose_row([9], [1e-30])
    assert thr == [Wt.TWO32 - 1] and alias == [9]


# ---- the statement's draws follow the weights ------------------------------------------------------------
N_DRAWS = 1 << 21       # 2 M draws per row (the least the check allows is 50 000): the 1 : 1e6 neighbour is expected twice, not 0.05 times


@pytest.mark.parametrize("name,weights", [("0..15", list(range(16))), ("1,0,1e6", [1.0, 0.0, 1e6]), ("64 equal", [1.0] * 64)])
@pytest.mark.parametrize("word", [0, 0x9E3779B9])
def test_chi_square_of_the_statements_draws(name, weights, word):
    """One row, ids 100 .. 100 + d - 1.  The draws are hashes of (row of the input list, hop, slot, draw word): 2^21 of them over 2^17 rows,
    hops 1..4 and slots 0..3.  A neighbour of weight 0 is never drawn; the counts of the others stay below the chi-square quantile at
    1 - 1e-6.  The GPU equals the statement bit for bit (tests/test_gpu_sample_weighted.py), so this is the kernel's distribution too."""
    d = len(weights)
    ids = np.arange(100, 100 + d)
    thr, alias = Wt.vose_row(ids, weights)
    n = N_DRAWS
    m = np.arange(n, dtype=np.int64)
    got = Wt.draw_ids(ids, thr, alias, m >> 4, 1 + ((m >> 2) & 3), m & 3, word)
    c = np.bincount(got - 100, minlength=d).astype(np.float64)
    assert len(c) == d and c.sum() == n
    wt = np.asarray(weights, dtype=np.float64)
    assert (c[wt == 0] == 0).all()
    e = n * wt[wt > 0] / wt.sum()
    X = float(((c[wt > 0] - e) ** 2 / e).sum())
    dof = int((wt > 0).sum()) - 1
    cap = D.chi2_cap(dof)
    print("%s, W = %#x: X = %.2f on %d degrees of freedom, cap %.2f; counts %s" % (name, word, X, dof, cap, c[:16].astype(np.int64).tolist()))
    assert X <= cap, (name, X, cap)


def test_slot_draw_known_answers():
    """(k, ub) of a few tuples, from the arithmetic written out with plain Python integers."""
    def scalar(i, h, j, d, w):
        K = D.mix32_scalar(D.mix32_scalar(((i + D.GOLDEN * h) & D.M32) ^ w) ^ Wt.WEIGHTED_TAG)
        uc = D.mix32_scalar(K ^ ((D.STEP * (2 * j + 1)) & D.M32))
        ub = D.mix32_scalar(K ^ ((D.STEP * (2 * j + 2)) & D.M32))
        return (uc * d) >> 32, ub
    cases = [(0, 1, 0, 1, 0), (7, 2, 3, 2, 0), (123456, 3, 24, 2 ** 31 - 1, 0xFFFFFFFF), (2 ** 31 - 1, 8, 63, 1000, 0xDEADBEEF), (5, 1, 0, 17, 1)]
    k, ub = Wt.slot_draw(*[np.array(x) for x in zip(*cases)][:4], w=np.array([c[4] for c in cases]))
    for m, c in enumerate(cases):
        assert (int(k[m]), int(ub[m])) == scalar(*c), c
        assert 0 <= int(k[m]) < c[3]


def test_whole_batches_of_the_statement_draw_only_weighted_neighbours():
    """weightedref.run_batch on the graph above: every edge of the batch is a (source, neighbour) pair of positive weight, a row without
    weight gives no edge, and the parked draws are the edges' sources in slot order."""
    indptr, indices, w = graph_with_weights(1)
    V = len(indptr) - 1
    thr, alias = Wt.build_table(indptr, indices, w)
    table = Wt.Table(indptr, indices, thr, alias)
    feats = np.random.RandomState(2).rand(V, 3).astype(np.float32)
    labels = np.arange(V, dtype=np.int32) % 7
    seeds = np.random.RandomState(3).permutation(V)[:150].astype(np.int32)
    rowof = np.repeat(np.arange(V), np.diff(indptr))
    good = set(zip(rowof[w > 0].tolist(), indices[w > 0].tolist()))
    fan = [7, 5, 3]
    for counter, word in ((0, 0), (1, 0), (2, 0), (0, 12345)):
        b = Wt.run_batch(table, feats, seeds, labels[seeds], 64, counter, fan, word)
        for h, f in enumerate(fan):
            inp, cnt = b["draw_counts"][h]
            dr = b["draws"][h].reshape(-1, f)
            for node, row in zip(inp.tolist(), dr.tolist()):
                assert all(x == -1 or (node, x) in good for x in row)
        assert int(b["ec"][2 + 3]) == sum(int(c.sum()) for _, c in b["draw_counts"]) > 0
    a, c = Wt.run_batch(table, feats, seeds, labels[seeds], 64, 0, fan, 0), Wt.run_batch(table, feats, seeds, labels[seeds], 64, 0, fan, 12345)
    assert not np.array_equal(a["draws"][0], c["draws"][0])


# ---- parser and boot -----------------------------------------------------------------------------------
ACCEPTED = "Server_Initialize: the synth: dataset path names no known workload / scale"


@pytest.mark.parametrize("value,refusal", [
    ("weighted", None),
    ("Weighted", "Server_Initialize: LEGION_SAMPLING=Weighted is not a known sampling mode: `replace` (the default: draws with replacement) or `distinct` "
                 "(min(degree, fan-out) distinct neighbours per row), or `weighted` (draws with replacement in proportion to the edge weights)")])
def test_boot_parses_weighted(tmp_path, value, refusal):
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write("synth:nosuchworkload 512 1000 0 16 100 0 0 %d 1 0\n" % (1 << 30))
    env = {k: v for k, v in os.environ.items() if k not in ("LEGION_AGG_LAST_HOP", "LEGION_AGG_NORM", "LEGION_SAMPLING", "LEGION_SAMPLING_SEED", "LEGION_LP_DRAW")}
    env.update(LEGION_SAMPLING=value, LEGION_IPC_NAMESPACE="cpuwt%d_" % os.getpid())
    r = subprocess.run([SERVER, "1", "0", "65,2", meta], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)   # 65: the fan-out bound is the distinct mode's alone
    said = r.stdout + r.stderr
    assert r.returncode == 1 and (refusal or ACCEPTED) in said, said[-2000:]


def test_launch_server_passes_weighted_on(tmp_path):
    work = tmp_path / "pkg"
    (work / "csrc").mkdir(parents=True)
    (work / "launch_server.py").write_text(open(os.path.join(ROOT, "legion-1_amd", "launch_server.py")).read())
    stand_in = work / "csrc" / "legion"
    stand_in.write_text("#!/bin/sh\necho \"SAMPLING=[${LEGION_SAMPLING}]\"\n")
    stand_in.chmod(0o755)
    env = {k: v for k, v in os.environ.items() if k != "LEGION_SAMPLING"}
    r = subprocess.run([sys.executable, str(work / "launch_server.py"), "--dataset", "PR", "--gpu_number", "1", "--sampling", "weighted"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=60)
    assert "SAMPLING=[weighted]" in r.stdout, r.stdout + r.stderr


# ---- the pool's sampling kind, without a device -----------------------------------------------------------
def test_pool_sampling_kind_without_a_gpu():
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    pool = L.NewGPUMemoryPool(2)

    def err():
        msg = (L.legion_last_error() or b"").decode()
        L.legion_clear_error()
        return msg
    try:
        assert L.GPUMemoryPool_GetSampling(pool) == 0 and L.GPUMemoryPool_GetSampling(None) == 0
        for kind in (0, 1, 2, 1, 0, 2):
            L.GPUMemoryPool_SetSampling(pool, kind)
            assert not err() and L.GPUMemoryPool_GetSampling(pool) == kind and L.GPUMemoryPool_GetSampleDistinct(pool) == int(kind == 1)
        for kind in (3, -1):
            L.GPUMemoryPool_SetSampling(pool, kind)
            assert "GPUMemoryPool_SetSampling: unknown sampling kind (0 = replace, 1 = distinct, 2 = weighted)" in err()
            assert L.GPUMemoryPool_GetSampling(pool) == 2
        L.GPUMemoryPool_SetSampleDistinct(pool, 7)                      # any non-zero argument: distinct
        assert not err() and L.GPUMemoryPool_GetSampling(pool) == 1 and L.GPUMemoryPool_GetSampleDistinct(pool) == 1
        L.GPUMemoryPool_SetSampling(pool, 2)
        L.GPUMemoryPool_SetSampleDistinct(pool, 0)                      # "not distinct" is the default kind, whatever the pool was in
        assert not err() and L.GPUMemoryPool_GetSampling(pool) == 0
        L.GPUMemoryPool_SetSampling(None, 2)
        assert "GPUMemoryPool_SetSampling: null pool" in err()
        # the graph's side refuses null handles by name and touches no device
        assert L.GPUGraphStorage_SetEdgeWeights(None, None, 0) == -1 and "GPUGraphStorage_SetEdgeWeights: null graph" in err()
        assert L.GPUGraphStorage_HasEdgeWeights(None) == 0
        assert L.GPUGraphStorage_CopyAliasRows(None, 0, 0, 1, None, None) == -1 and "GPUGraphStorage_CopyAliasRows" in err()
        g = L.NewGPUMemoryGraphStorage()
        assert L.GPUGraphStorage_HasEdgeWeights(g) == 0
        assert L.GPUGraphStorage_SetEdgeWeights(g, None, 0) == -1 and "GPUGraphStorage_Build was not called" in err()
        L.GPUGraphStorage_Delete(g)
    finally:
        L.legion_clear_error()
        L.GPUMemoryPool_Delete(pool)


def test_sampling_word_takes_2_and_nothing_else_moves():
    """IPCEnv_SetSampling(2) on the device-free IPC env: the "<name>_ext" object stays 2152 bytes, only int32 word 535 changes, to 2; a
    client reads 2 and ipc_service.sampling() says "weighted"; any other non-zero value is still 1 ("distinct")."""
    ns = "cpuipc_wt%d_" % os.getpid()
    pre, _ = device_free_server(ns, 2, "")
    client = pre + ("sys.path.insert(0, %r)\nimport legion1_amd.capi as K\nL = K.lib(); L.legion_set_error_mode(K.ERR_RETURN)\n"
                    "c = C.c_void_p(L.legion_ipc_client_open(0)); K.check(); assert c.value\n"
                    "print('CLIENT', L.legion_ipc_client_sampling(c)); L.legion_ipc_client_close(c)\n"
                    "import torch, ipc_service\nipc_service.initialize(); print('SERVICE', ipc_service.sampling()); ipc_service.finalize()\n"
                    ) % os.path.join(ROOT, "legion-1_amd", "ipc_service")
    body = ("ext = [f for f in os.listdir('/dev/shm') if %r in f and f.endswith('_ext')]; assert len(ext) == 1, ext\n"
            "assert os.path.getsize('/dev/shm/' + ext[0]) == 2152\n"
            "words = lambda: np.fromfile('/dev/shm/' + ext[0], dtype=np.int32)\n"
            "w0 = words(); L.IPCEnv_SetSampling(e, 2); w1 = words()\n"
            "assert np.nonzero(w0 != w1)[0].tolist() == [535] and w1[535] == 2 and L.IPCEnv_GetSampling(e) == 2\n"
            "for value, name in ((2, 'weighted'), (1, 'distinct'), (7, 'distinct'), (0, 'replace'), (2, 'weighted')):\n"
            "    L.IPCEnv_SetSampling(e, value); stored = 2 if value == 2 else int(value != 0)\n"
            "    assert L.IPCEnv_GetSampling(e) == stored and words()[535] == stored and len(words()) * 4 == 2152\n"
            "    r = subprocess.run([sys.executable, '-c', %r], capture_output=True, text=True, timeout=120)\n"
            "    print(r.stdout.strip(), r.stderr[-500:]); assert 'CLIENT %%d' %% stored in r.stdout and 'SERVICE ' + name in r.stdout\n") % (ns, client)
    _, server = device_free_server(ns, 2, body)
    r = subprocess.run([sys.executable, "-c", server], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SERVER_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert not [f for f in os.listdir("/dev/shm") if ns in f]


def test_capi_table_and_header_name_the_new_symbols():
    import legion1_amd.capi as K
    L = K.lib()
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    for name in ("GPUMemoryPool_SetSampling", "GPUMemoryPool_GetSampling", "GPUGraphStorage_SetEdgeWeights", "GPUGraphStorage_HasEdgeWeights",
                 "GPUGraphStorage_CopyAliasRows", "legion_weighted_probe", "legion_synth_edge_weights"):
        assert name in K._SIGS and name + "(" in header and getattr(L, name)


def test_engine_refuses_an_unknown_sampling_name_before_it_touches_anything():
    import legion1_amd.capi as K
    eng = K.Engine.__new__(K.Engine)            # no device: _set_modes validates its arguments first
    for bad in ("unique", "", "Weighted", None):
        with pytest.raises(ValueError, match="'replace', 'distinct' or 'weighted'"):
            eng._set_modes(0, False, None, bad, None, 0, None)


# ---- the synth: source's weights ---------------------------------------------------------------------------
def test_synth_edge_weights_known_answers():
    import legion1_amd.synth as S
    w = S.edge_weights(100000)
    assert w.dtype == np.float32 and len(w) == 100000
    assert set(np.unique(w).tolist()) == set(float(x) for x in range(17))                   # 0 and every integer of 1..16
    assert abs((w == 0).mean() - (1 - (15 / 16) ** 2)) < 0.01                                # 0.121: about one in eight
    assert np.array_equal(S.edge_weights(100000, 99000), w[99000:])                         # a closed form of the position
    def scalar(e):
        h, hb = S.sm64_int(S.S_WGT + e), S.sm64_int(S.S_WGT_BLOCK + (e >> 6))
        return float(1 + ((h >> 4) & 15)) if (h & 15) and (hb & 15) else 0.0
    for e in list(range(200)) + [12345, 99999]:
        assert float(w[e]) == scalar(e), e
    blocks = w[:96000].reshape(-1, 64)
    assert 40 < int((blocks == 0).all(axis=1).sum()) < 160                                   # about one block in sixteen is all zero
    # on the products graph of the tests: zero-weight columns and all-zero rows both occur
    spec = S.spec_for("products", scale=0.004)
    ds = S.generate(spec, with_features=False)
    w = S.edge_weights(ds.E)
    rows = np.add.reduceat(np.concatenate([w, [0.0]]), np.minimum(ds.indptr[:-1], ds.E))
    deg = np.diff(ds.indptr)
    assert ((rows == 0) & (deg > 0)).sum() > 0 and (w == 0).sum() > ds.E // 10
