"""Normalised last hop (INTEGRATION.md "Normalised sums": LEGION_AGG_LAST_HOP=1 LEGION_AGG_NORM=both), the parts that need no GPU.

The EXPECTED VALUE of the mode is the NumPy statement of tests/gcnref.py (`expected_nbr_sum_norm`), computed from a DEFAULT-mode batch of a
reference implementation (tests/pyref.py here, the C oracle in tests/test_gpu_agg_norm.py) and the input graph -- never from the code
under test.  This file checks the statement's own premises on toy batches, the trainer-side formula (GraphConvBothFused) against
GraphConvBoth on the default batch, the mode word of the "<name>_ext" object, the refusals and the public surface."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pyref
from aggref import cum_edges, expected_nbr_sum, last_hop_runs
from conftest import ROOT
from harness import device_free_server
from gcnref import block_out_degree, expected_nbr_sum_norm


def toy_graph(seed, V=90, F=6, holes=True):
    """the toy graphs of test_agg_last_hop_cpu.py: degree-0 rows, hubs, -1 neighbours, rows of -0.0"""
    rs = np.random.RandomState(seed)
    deg = rs.randint(0, 9, size=V)
    deg[rs.randint(0, V, 3)] = 40
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rs.randint(-1 if holes else 0, V, size=int(indptr[-1])).astype(np.int32)
    feats = rs.standard_normal((V, F)).astype(np.float32)
    feats[rs.randint(0, V, 4)] = np.float32(-0.0)
    labels = rs.randint(0, 5, size=V).astype(np.int32)
    seeds = rs.permutation(V)[:37].astype(np.int32)
    return indptr, indices, feats, labels, seeds


TOY_CASES = [([4], 16), ([3, 2], 16), ([5, 4, 3], 16), ([2, 2, 2], 37), ([25, 10], 9)]


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("fan,B", TOY_CASES)
def test_expected_value_statement_holds_on_toy_batches(fan, B, holes):
    """d counts every edge of block 1 once; w is 1 exactly where d <= 1 and the two-rounding 1 / sqrt elsewhere; the vectorised S_w equals
    the literal per-run loop in np.float32 scalars (product rounded, then the add) bit for bit; a run without draws is +0.0; and a
    run whose draws all weigh 1 is the row of aggref's plain statement."""
    indptr, indices, feats, labels, seeds = toy_graph(len(fan) * 10 + B, holes=holes)
    H = len(fan)
    seen_weighted = False
    for counter in range((len(seeds) + B - 1) // B):
        ref = pyref.run_batch(indptr, indices, feats, seeds, labels[seeds], B, counter, fan)
        n_in, N, run_dst, S, d = expected_nbr_sum_norm(ref, indptr, indices, fan)
        d2, w = block_out_degree(ref, fan)
        n, E = int(ref["nc"][5 + 2 * H]), cum_edges(ref["ec"], H)
        assert np.array_equal(d, d2) and d.dtype == np.int32 and d.shape == (n,) and int(d.sum()) == E
        for p in range(n):
            assert w[p] == np.float32(1.0) / np.float32(np.sqrt(np.float32(max(int(d[p]), 1))))
        assert (w[d <= 1] == np.float32(1)).all() and (w[d > 1] < 1).all()
        seen_weighted |= bool((d > 1).any())
        e = cum_edges(ref["ec"], H - 1)
        _, _, _, cnt = last_hop_runs(ref, indptr, indices, fan)
        x = ref["features"]
        for i in range(N):
            acc = np.zeros(feats.shape[1], np.float32)
            for _ in range(int(cnt[i])):
                p = int(ref["src_off"][e])
                acc = acc + np.array([np.float32(w[p]) * np.float32(v) for v in x[p]], np.float32)
                e += 1
            assert np.array_equal(acc.view(np.uint32), S[i].view(np.uint32)), (counter, i)
        assert e == E
        assert not np.signbit(S[cnt == 0]).any() and not S[cnt == 0].view(np.uint32).any()
        # a run whose draws all have weight 1 is the plain statement's row, bit for bit
        _, _, _, plain = expected_nbr_sum(ref, indptr, indices, fan)
        start = np.cumsum(cnt) - cnt + cum_edges(ref["ec"], H - 1)
        unit = np.array([bool((w[ref["src_off"][start[i]:start[i] + cnt[i]]] == 1).all()) for i in range(N)], bool)
        assert plain.shape == S.shape and np.array_equal(plain[unit].view(np.uint32), S[unit].view(np.uint32))
        assert unit.all() or not np.array_equal(plain, S)
    assert seen_weighted


@pytest.mark.parametrize("fan,B", TOY_CASES)
def test_graph_conv_both_fused_matches_graph_conv_both(fan, B):
    """examples/legion_sage_torch.py: GraphConvBothFused on the normalised batch against GraphConvBoth on the default batch, same weights,
    torch on the CPU.  The bound is derived, with u = 2^-24:
      * per term.  Default: t = fl(x * r), r = torch's rsqrt(d).  Served: t' = fl(w * x), w = fl(1 / fl(sqrt(d))): two correct roundings,
        |w / d^-1/2 - 1| <= (1 + u) / (1 - u) - 1 =: e_w.  torch's rsqrt is measured against float64 (e_t: the reference's own error).
        |t - t'| <= |x| d^-1/2 ((1 + e_t)(1 + u) - (1 - e_w)(1 - u)) =: D_term.  The hops < H use r on both sides: identical terms.
      * per destination.  Both add k = indeg terms in some order: each is within k u sum|its terms| of its exact sum, and the exact sums
        differ by at most D = sum D_term: |agg - agg'| <= 2 k u (M + D) + D, M = sum |t|.
      * behind the common factor in_deg^-1/2 and the linear map: that bound through |W|, plus the roundings both sides do alike (the
        scaling, a matrix product of F terms, the bias add): (F + 4) u of the magnitudes involved, once per side."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("legion_sage_torch", os.path.join(ROOT, "examples", "legion_sage_torch.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    indptr, indices, feats, labels, seeds = toy_graph(11 + len(fan), holes=True)
    H = len(fan)
    ref = pyref.run_batch(indptr, indices, feats, seeds, labels[seeds], B, 0, fan)
    n_in, N, run_dst, S, d = expected_nbr_sum_norm(ref, indptr, indices, fan)
    x = torch.from_numpy(ref["features"])
    F, out_f = x.shape[1], 5
    n = int(ref["nc"][5 + 2 * H])
    edges = [cum_edges(ref["ec"], H - k) for k in range(H)]            # edges of block k + 1
    e_in = cum_edges(ref["ec"], H - 1)
    src = torch.from_numpy(ref["src_off"][:edges[0]].astype(np.int64))
    dst = torch.from_numpy(ref["dst_off"][:edges[0]].astype(np.int64))
    torch.manual_seed(3)
    plain, fused = ex.GraphConvBoth(F, out_f), ex.GraphConvBothFused(F, out_f)
    fused.load_state_dict(plain.state_dict())
    with torch.no_grad():
        a = plain((src, dst, n, n_in), x)
        block = ex.fused_first_block(src, dst, n, n_in, edges, torch.from_numpy(S))
        assert torch.equal(block[5], torch.from_numpy(run_dst)) and block[4] == e_in
        b = fused(block, x[:n_in])
        u = 2.0 ** -24
        dd = torch.from_numpy(d.clip(1).astype(np.float64))
        exact = dd.rsqrt()
        e_t = float(((torch.from_numpy(d.clip(1).astype(np.float32)).rsqrt().double() - exact).abs() / exact).max())
        e_w = (1 + u) / (1 - u) - 1
        term = x.abs().double() * exact.unsqueeze(1)                     # |x| d^-1/2 by position
        last = torch.arange(edges[0]) >= e_in
        D_term = term.index_select(0, src) * ((1 + e_t) * (1 + u) - (1 - e_w) * (1 - u)) * last.unsqueeze(1)
        k = torch.bincount(dst, minlength=n_in).double().unsqueeze(1)
        M = torch.zeros(n_in, F, dtype=torch.float64).index_add_(0, dst, term.index_select(0, src) * (1 + e_t) * (1 + u))
        D = torch.zeros(n_in, F, dtype=torch.float64).index_add_(0, dst, D_term)
        r_in = k.clamp(min=1).float().rsqrt().double()                   # the factor both sides apply: torch's own fp32 value
        W = plain.fc.weight.abs().double()
        bound = ((2.0 * k * u * (M + D) + D) * r_in) @ W.T
        shared = (F + 4) * u * (((M + D) * r_in) @ W.T + plain.fc.bias.abs().double())
        err = (a.double() - b.double()).abs()
    assert a.shape == b.shape == (n_in, out_f)
    assert bool((err <= bound + 2 * shared).all()), float((err - bound - 2 * shared).max())
    assert float(err.max()) < 1e-3 * float(a.abs().max())             # and the bound is not what lets a wrong formula through


def test_public_surface_carries_the_new_names():
    import inspect
    import legion1_amd.capi as K
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    for name in ("GPUMemoryPool_SetAggNorm", "GPUMemoryPool_GetAggNorm", "GPUMemoryPool_GetAggOutDeg", "IPCEnv_SetAggNorm", "IPCEnv_GetAggNorm",
                 "legion_ipc_client_agg_norm"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in K._SIGS, name
    for fn in (K.Engine.run_batch, K.Engine.capture_batch):
        assert inspect.signature(fn).parameters["agg_norm"].default is None
    kernels = open(os.path.join(ROOT, "legion-1_amd", "csrc", "gather.hip")).read()
    for name in ("k_block_out_deg", "k_draw_weights", "k_agg_norm_prep", "fp contract(off)"):
        assert name in kernels, name
    sys.path.insert(0, os.path.join(ROOT, "legion-1_amd", "ipc_service"))
    import torch  # noqa: F401  (the extension links libtorch)
    import ipc_service
    for name in ("aggregate_norm", "get_next_aggregated_norm", "get_next_aggregated", "aggregated", "get_next"):
        assert callable(getattr(ipc_service, name)), name
    sig = ipc_service.get_next_aggregated_norm.__doc__.splitlines()[0]
    assert sig.count("arg") == 1 and "list[torch.Tensor]" in sig.replace("List", "list"), sig      # (feature_dim) -> tensors, like get_next
    assert "-> int" in ipc_service.aggregate_norm.__doc__.splitlines()[0]


def test_set_agg_norm_is_refused_by_name_without_the_aggregated_mode():
    """GPUMemoryPool_SetAggNorm on a pool without scratch (no device is touched): refused by name while the pool does not aggregate the
    last hop, accepted behind GPUMemoryPool_SetAggLastHop, an unknown norm refused, and switching the aggregated mode keeps its behaviour."""
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    L.legion_clear_error()
    pool = L.NewGPUMemoryPool(2)
    try:
        assert L.GPUMemoryPool_GetAggNorm(pool) == 0 and not L.GPUMemoryPool_GetAggOutDeg(pool)
        L.GPUMemoryPool_SetAggNorm(pool, 1)
        msg = (L.legion_last_error() or b"").decode()
        assert "GPUMemoryPool_SetAggNorm" in msg and "does not aggregate the last hop" in msg and "GPUMemoryPool_SetAggLastHop" in msg, msg
        L.legion_clear_error()
        assert L.GPUMemoryPool_GetAggNorm(pool) == 0
        L.GPUMemoryPool_SetAggNorm(pool, 0)                             # "none" is always acceptable
        assert not L.legion_last_error()
        L.GPUMemoryPool_SetAggLastHop(pool, 1)
        assert not L.legion_last_error() and L.GPUMemoryPool_GetAggLastHop(pool) == 1
        L.GPUMemoryPool_SetAggNorm(pool, 1)
        assert not L.legion_last_error() and L.GPUMemoryPool_GetAggNorm(pool) == 1
        L.GPUMemoryPool_SetAggNorm(pool, 2)
        msg = (L.legion_last_error() or b"").decode()
        assert "GPUMemoryPool_SetAggNorm: unknown norm" in msg, msg
        L.legion_clear_error()
        assert L.GPUMemoryPool_GetAggNorm(pool) == 1
        L.GPUMemoryPool_SetAggLastHop(pool, 0)
        assert not L.legion_last_error() and L.GPUMemoryPool_GetAggLastHop(pool) == 0
    finally:
        L.legion_clear_error()
        L.GPUMemoryPool_Delete(pool)


# 32-bit word indices of the mode words in the "<name>_ext" object and its size, as the build that first had all five laid them out (byte
# offsets 2132 .. 2148 of 2152): peers of other builds map the same object, so the words never move.
EXT_WORDS = dict(agg_last_hop=533, agg_norm=534, sampling=535, sampling_seeded=536, sampling_seed=537)
EXT_BYTES = 2152


def test_ext_word_round_trip_without_a_gpu():
    """The norm word of the "<name>_ext" object, with the device-free IPC env: a server that sets it, a client process
    that reads it (0 from a server that never set it); every older field the client reads -- the aggregated word, hops, steps, the row
    capacity -- is where it was, whatever the new word holds.  And the mapped object diffed word by word around every IPCEnv_Set* of a
    mode: each call changes exactly the word(s) at the absolute positions above, to the value given, and no other; the size never changes."""
    ns = "cpuipc_norm%d_" % os.getpid()
    pre, _ = device_free_server(ns, 3, "")
    client = pre + ("import legion1_amd.capi as K\nL = K.lib(); L.legion_set_error_mode(K.ERR_RETURN)\n"
                    "c = C.c_void_p(L.legion_ipc_client_open(0)); K.check(); assert c.value\n"
                    "s = (C.c_int32 * 3)(); L.legion_ipc_client_steps(c, s)\n"
                    "print('CLIENT', L.legion_ipc_client_agg_norm(c), L.legion_ipc_client_agg_last_hop(c), L.legion_ipc_client_hops(c), "
                    "L.legion_ipc_client_feature_rows(c), list(s)); L.legion_ipc_client_close(c)\n")
    body = ("assert L.IPCEnv_GetAggNorm(e) == 0 and L.IPCEnv_GetAggLastHop(e) == 0\n"
            "ext = [f for f in os.listdir('/dev/shm') if %r in f and f.endswith('_ext')]; assert len(ext) == 1, ext\n"
            "words = lambda: np.fromfile('/dev/shm/' + ext[0], dtype=np.uint32)\n"
            "W = %r; assert not words()[W['agg_last_hop']:].any()\n"
            "def changes(call, *args):\n"
            "    w0 = words(); call(e, *args); w1 = words(); assert len(w0) * 4 == len(w1) * 4 == os.path.getsize('/dev/shm/' + ext[0]) == %d\n"
            "    return {int(i): int(w1[i]) for i in np.nonzero(w0 != w1)[0]}\n"
            "assert changes(L.IPCEnv_SetAggLastHop, 1) == {W['agg_last_hop']: 1} and changes(L.IPCEnv_SetAggNorm, 1) == {W['agg_norm']: 1}\n"
            "assert changes(L.IPCEnv_SetSampling, 1) == {W['sampling']: 1}\n"
            "assert changes(L.IPCEnv_SetSamplingSeed, 1, 0xDEADBEEF) == {W['sampling_seeded']: 1, W['sampling_seed']: 0xDEADBEEF}\n"
            "assert changes(L.IPCEnv_SetSamplingSeed, 1, 7) == {W['sampling_seed']: 7}\n"
            "assert changes(L.IPCEnv_SetSamplingSeed, 0, 7) == {W['sampling_seeded']: 0, W['sampling_seed']: 0}\n"
            "assert changes(L.IPCEnv_SetSampling, 0) == {W['sampling']: 0} and changes(L.IPCEnv_SetAggNorm, 0) == {W['agg_norm']: 0}\n"
            "assert changes(L.IPCEnv_SetAggLastHop, 0) == {W['agg_last_hop']: 0}\n"
            "assert changes(L.IPCEnv_SetAggLastHop, 0) == {} and changes(L.IPCEnv_SetSamplingSeed, 0, 9) == {}\n"
            "L.IPCEnv_SetFeatureRows(e, 0, 4321)\n"
            "for agg, norm in ((0, 0), (1, 0), (1, 1), (0, 1), (1, 0)):\n"
            "    L.IPCEnv_SetAggLastHop(e, agg); L.IPCEnv_SetAggNorm(e, norm)\n"
            "    assert L.IPCEnv_GetAggNorm(e) == norm and L.IPCEnv_GetAggLastHop(e) == agg\n"
            "    r = subprocess.run([sys.executable, '-c', %r], capture_output=True, text=True, timeout=60)\n"
            "    print(r.stdout.strip(), r.stderr[-500:]); assert 'CLIENT %%d %%d 3 4321 [7, 2, 1]' %% (norm, agg) in r.stdout\n") % (ns, EXT_WORDS, EXT_BYTES, client)
    _, server = device_free_server(ns, 3, body)
    r = subprocess.run([sys.executable, "-c", server], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "SERVER_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert not [f for f in os.listdir("/dev/shm") if ns in f]


def test_ipc_service_refuses_the_wrong_call_for_the_servers_norm_without_a_gpu():
    """get_next_aggregated on a normalising server raises, naming LEGION_AGG_NORM and the right call; get_next_aggregated_norm on a server
    that aggregates without normalising, and on one that does not aggregate at all, raises too, naming the switch and the right call
    -- all before they wait for a batch (device-free IPC env); aggregate_norm() says which."""
    ns = "cpuipc_normsvc%d_" % os.getpid()
    pre, _ = device_free_server(ns, 2, "")
    client = pre + ("sys.path.insert(0, %r)\nimport torch, ipc_service\nipc_service.initialize()\n"
                    "agg, norm = ipc_service.aggregated(), ipc_service.aggregate_norm()\n"
                    "assert isinstance(norm, int)\n"
                    "bad, good_name = (ipc_service.get_next_aggregated, 'get_next_aggregated_norm') if norm else "
                    "(ipc_service.get_next_aggregated_norm, 'get_next_aggregated' if agg else 'get_next')\n"
                    "try:\n    bad(16); print('NOT REFUSED')\n"
                    "except RuntimeError as e:\n    print('REFUSED', int(agg), norm, ('LEGION_AGG_NORM' in str(e)) and str(e).split('call ')[-1].split()[0] == good_name)\n"
                    "ipc_service.finalize()\n") % os.path.join(ROOT, "legion-1_amd", "ipc_service")
    body = ("for agg, norm in ((1, 1), (1, 0), (0, 0)):\n"
            "    L.IPCEnv_SetAggLastHop(e, agg); L.IPCEnv_SetAggNorm(e, norm)\n"
            "    r = subprocess.run([sys.executable, '-c', %r], capture_output=True, text=True, timeout=120)\n"
            "    print(r.stdout.strip(), r.stderr[-800:]); assert 'REFUSED %%d %%d True' %% (agg, norm) in r.stdout\n") % client
    _, server = device_free_server(ns, 2, body)
    r = subprocess.run([sys.executable, "-c", server], capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "SERVER_OK" in r.stdout, r.stdout[-2500:] + r.stderr[-2000:]
