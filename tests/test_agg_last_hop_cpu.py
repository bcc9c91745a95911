"""Aggregated last hop (INTEGRATION.md "Aggregated last hop"), the parts that need no GPU.

The EXPECTED VALUE of the mode is the NumPy statement of tests/aggref.py (`expected_nbr_sum`), computed from a DEFAULT-mode batch of a reference
implementation (tests/pyref.py here, the C oracle in tests/test_gpu_agg_last_hop.py) and the input graph -- never from the code under
test.  This file checks the statement's own premises on toy batches, the trainer-side formula that folds the sums into nodes against the
default first-layer aggregate, and that the public surface carries the new names."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pyref
from aggref import cum_edges, expected_nbr_sum, last_hop_runs
from conftest import ROOT


# ---------------------------------------------------------------------------------------------------
def toy_graph(seed, V=90, F=6, holes=True):
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
    """Counter formulas for n_in and N, the last hop's COO slice = the runs in order, sum(cnt) = its edge count (asserted inside
    expected_nbr_sum), for full and short batches; and the vectorised sum equals the literal per-run loop bit for bit."""
    indptr, indices, feats, labels, seeds = toy_graph(len(fan) * 10 + B, holes=holes)
    H, f = len(fan), fan[-1]
    for counter in range((len(seeds) + B - 1) // B):
        ref = pyref.run_batch(indptr, indices, feats, seeds, labels[seeds], B, counter, fan)
        n_in, N, run_dst, S = expected_nbr_sum(ref, indptr, indices, fan)
        nc = ref["nc"]
        assert n_in == sum(int(nc[4 + 2 * l]) for l in range(H)) and n_in + int(nc[4 + 2 * H]) == int(nc[5 + 2 * H])
        assert (run_dst < n_in).all() and S.shape == (N, feats.shape[1])
        # the literal statement, run by run
        e = cum_edges(ref["ec"], H - 1)
        _, _, _, cnt = last_hop_runs(ref, indptr, indices, fan)
        for i in range(N):
            acc = np.zeros(feats.shape[1], np.float32)
            for _ in range(int(cnt[i])):
                acc = acc + ref["features"][ref["src_off"][e]]
                e += 1
            assert np.array_equal(acc.view(np.uint32), S[i].view(np.uint32)), (counter, i)
        assert e == cum_edges(ref["ec"], H)
        assert not np.signbit(S[cnt == 0]).any()         # a run without draws is +0.0


@pytest.mark.parametrize("fan,B", TOY_CASES)
def test_folding_the_run_sums_reproduces_the_default_first_layer_aggregate(fan, B):
    """The trainer's first layer in the new mode (two index_add_ lines: the edges of the hops < H over x_in, and the run sums over
    run_dst) against the default mode's (index_select / index_add_ over every edge of block 1), in torch on the CPU.  Both add the
    same k = indeg fp32 terms per destination in a different order; each ordering is within (k - 1) roundings of the exact sum, every
    partial sum is bounded by sum|terms|, so |a - b| <= 2 k 2^-24 sum|terms| per element -- derived, not tuned."""
    import torch
    indptr, indices, feats, labels, seeds = toy_graph(7 + len(fan), holes=True)
    H = len(fan)
    ref = pyref.run_batch(indptr, indices, feats, seeds, labels[seeds], B, 0, fan)
    n_in, N, run_dst, S = expected_nbr_sum(ref, indptr, indices, fan)
    x = torch.from_numpy(ref["features"])
    F = x.shape[1]
    e_in, e_all = cum_edges(ref["ec"], H - 1), cum_edges(ref["ec"], H)
    src = torch.from_numpy(ref["src_off"][:e_all].astype(np.int64))
    dst = torch.from_numpy(ref["dst_off"][:e_all].astype(np.int64))
    default = torch.zeros(n_in, F).index_add_(0, dst, x.index_select(0, src))
    assert e_in == 0 or int(src[:e_in].max()) < n_in           # block 2 only reads rows the mode still hands over
    fused = torch.zeros(n_in, F).index_add_(0, dst[:e_in], x[:n_in].index_select(0, src[:e_in]))
    fused += torch.zeros(n_in, F).index_add_(0, torch.from_numpy(run_dst), torch.from_numpy(S))
    k = torch.bincount(dst, minlength=n_in).to(torch.float64).unsqueeze(1)
    mag = torch.zeros(n_in, F, dtype=torch.float64).index_add_(0, dst, x.index_select(0, src).abs().double())
    bound = 2.0 * k * 2.0 ** -24 * mag
    err = (default.double() - fused.double()).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    assert int(torch.bincount(dst, minlength=n_in).sum()) == e_all


def test_public_surface_carries_the_new_names():
    import legion1_amd.capi as K
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    for name in ("get_feature_kernel_agg", "GPUMemoryPool_SetAggLastHop", "GPUMemoryPool_GetAggLastHop"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in K._SIGS, name
    import inspect
    assert "agg_last_hop" in inspect.signature(K.Engine.run_batch).parameters
    assert "agg_last_hop" in inspect.signature(K.Engine.capture_batch).parameters
    assert "k_gather_sum" in open(os.path.join(ROOT, "legion-1_amd", "csrc", "gather.hip")).read()
    for name in ("IPCEnv_SetAggLastHop", "IPCEnv_GetAggLastHop", "legion_ipc_client_agg_last_hop"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in K._SIGS, name
    import sys
    sys.path.insert(0, os.path.join(ROOT, "legion-1_amd", "ipc_service"))
    import torch  # noqa: F401  (the extension links libtorch)
    import ipc_service
    for name in ("aggregated", "get_next_aggregated", "get_next", "get_block_size", "get_steps", "initialize", "synchronize", "finalize"):
        assert callable(getattr(ipc_service, name)), name
    sig = ipc_service.get_next_aggregated.__doc__.splitlines()[0]
    assert sig.count("arg") == 1 and "list[torch.Tensor]" in sig.replace("List", "list"), sig      # (feature_dim) -> tensors, like get_next


@pytest.mark.parametrize("fan,B", TOY_CASES)
def test_sage_mean_fused_matches_sage_mean(fan, B):
    """examples/legion_sage_torch.py: the fused first layer on an aggregated batch against SageMean on the default batch, same weights,
    torch on the CPU.  Before the division both add the same k = indeg fp32 terms per destination in a different order:
    |a - b| <= 2 k 2^-24 sum|terms| per element of the aggregate (see the test above); behind the division by clamp(deg, 1) and the linear
    map W_neigh that bound becomes sum_c |W[o, c]| * bound[c] / deg, plus the roundings of the shared part (the division, the two
    matrix products of <= F terms and two adds: (F + 4) 2^-24 of the magnitudes involved)."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("legion_sage_torch", os.path.join(ROOT, "examples", "legion_sage_torch.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    indptr, indices, feats, labels, seeds = toy_graph(11 + len(fan), holes=True)
    H = len(fan)
    ref = pyref.run_batch(indptr, indices, feats, seeds, labels[seeds], B, 0, fan)
    n_in, N, run_dst, S = expected_nbr_sum(ref, indptr, indices, fan)
    x = torch.from_numpy(ref["features"])
    F, out_f = x.shape[1], 5
    n = int(ref["nc"][5 + 2 * H])
    edges = [cum_edges(ref["ec"], H - k) for k in range(H)]            # edges of block k + 1
    src = torch.from_numpy(ref["src_off"][:edges[0]].astype(np.int64))
    dst = torch.from_numpy(ref["dst_off"][:edges[0]].astype(np.int64))
    torch.manual_seed(3)
    plain, fused = ex.SageMean(F, out_f), ex.SageMeanFused(F, out_f)
    fused.load_state_dict(plain.state_dict())
    with torch.no_grad():
        a = plain((src, dst, n, n_in), x)
        block = ex.fused_first_block(src, dst, n, n_in, edges, torch.from_numpy(S))
        assert torch.equal(block[5], torch.from_numpy(run_dst)) and block[4] == cum_edges(ref["ec"], H - 1)
        b = fused(block, x[:n_in])
        u = 2.0 ** -24
        k = torch.bincount(dst, minlength=n_in).double().unsqueeze(1)
        mag = torch.zeros(n_in, F, dtype=torch.float64).index_add_(0, dst, x.index_select(0, src).abs().double())
        deg = k.clamp(min=1)
        W = plain.fc_neigh.weight.abs().double()
        bound = (2.0 * k * u * mag / deg) @ W.T                          # the reordered sums, through the division and W_neigh
        shared = (F + 4) * u * ((mag / deg) @ W.T + x[:n_in].abs().double() @ plain.fc_self.weight.abs().double().T + plain.bias.abs().double())
        err = (a.double() - b.double()).abs()
    assert a.shape == b.shape == (n_in, out_f)
    assert bool((err <= bound + 2 * shared).all()), float((err - bound - 2 * shared).max())


def test_ext_flag_round_trip_without_a_gpu():
    """The mode word behind the older fields of the "<name>_ext" object, with the device-free IPC env: a server that sets it, a client
    process that reads it (and 0 from a server that does not); the older fields the client reads (hops, steps) are where they were."""
    ns = "cpuipc_agg%d_" % os.getpid()
    pre = ("import os, sys, ctypes as C; sys.path.insert(0, %r)\n"
           "os.environ['LEGION_IPC_NO_DEVICE'] = '1'; os.environ['LEGION_IPC_NAMESPACE'] = %r\n"
           "import legion1_amd.capi as K\n"
           "L = K.lib(); L.legion_set_error_mode(K.ERR_RETURN)\n") % (ROOT, ns)
    client = pre + ("c = C.c_void_p(L.legion_ipc_client_open(0)); K.check(); assert c.value\n"
                    "s = (C.c_int32 * 3)(); L.legion_ipc_client_steps(c, s)\n"
                    "print('CLIENT', L.legion_ipc_client_agg_last_hop(c), L.legion_ipc_client_hops(c), list(s)); L.legion_ipc_client_close(c)\n")
    server = pre + ("import numpy as np, subprocess\n"
                    "e = L.NewIPCEnv(1)\n"
                    "info = K.LegionBuildInfo(); info.partition_count = 1; info.epoch = 1; info.raw_batch_size = 500\n"
                    "tr, va, te = (np.array([x], np.int32) for x in (3601, 700, 300))\n"
                    "info.training_set_num, info.validation_set_num, info.testing_set_num = tr.ctypes.data, va.ctypes.data, te.ctypes.data\n"
                    "L.IPCEnv_Coordinate(e, C.byref(info)); L.IPCEnv_InitializeSamplesBuffer(e, 500, 1000, 16, 0, 2); L.IPCEnv_SetHops(e, 3); K.check()\n"
                    "assert L.IPCEnv_GetAggLastHop(e) == 0\n"
                    "for on in (0, 1, 0, 7):\n"
                    "    L.IPCEnv_SetAggLastHop(e, on); assert L.IPCEnv_GetAggLastHop(e) == int(on != 0)\n"
                    "    r = subprocess.run([sys.executable, '-c', %r], capture_output=True, text=True, timeout=60)\n"
                    "    print(r.stdout.strip(), r.stderr[-500:]); assert 'CLIENT %%d 3 [7, 2, 1]' %% int(on != 0) in r.stdout\n"
                    "L.IPCEnv_Finalize(e); print('SERVER_OK')\n") % client
    r = subprocess.run([sys.executable, "-c", server], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "SERVER_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert not [f for f in os.listdir("/dev/shm") if ns in f]


def test_ipc_service_refuses_the_wrong_call_for_the_servers_mode_without_a_gpu():
    """ipc_service.get_next on an aggregated server and get_next_aggregated on a plain one raise, naming the mode, before they wait for a
    batch -- with the device-free IPC env (no hand-off buffers, zero handle slots)."""
    ns = "cpuipc_aggsvc%d_" % os.getpid()
    pre = ("import os, sys, ctypes as C; sys.path.insert(0, %r)\n"
           "os.environ['LEGION_IPC_NO_DEVICE'] = '1'; os.environ['LEGION_IPC_NAMESPACE'] = %r\n") % (ROOT, ns)
    client = pre + ("sys.path.insert(0, %r)\nimport torch, ipc_service\nipc_service.initialize()\n"
                    "agg = ipc_service.aggregated()\n"
                    "bad, good_name = (ipc_service.get_next, 'get_next_aggregated') if agg else (ipc_service.get_next_aggregated, 'get_next')\n"
                    "try:\n    bad(16); print('NOT REFUSED')\n"
                    "except RuntimeError as e:\n    print('REFUSED', int(agg), ('LEGION_AGG_LAST_HOP=1' in str(e)) and ('call ' + good_name) in str(e))\n"
                    "ipc_service.finalize()\n") % os.path.join(ROOT, "legion-1_amd", "ipc_service")
    server = pre + ("import numpy as np, subprocess\nimport legion1_amd.capi as K\nL = K.lib(); L.legion_set_error_mode(K.ERR_RETURN)\n"
                    "e = L.NewIPCEnv(1)\n"
                    "info = K.LegionBuildInfo(); info.partition_count = 1; info.epoch = 1; info.raw_batch_size = 500\n"
                    "tr, va, te = (np.array([x], np.int32) for x in (3601, 700, 300))\n"
                    "info.training_set_num, info.validation_set_num, info.testing_set_num = tr.ctypes.data, va.ctypes.data, te.ctypes.data\n"
                    "L.IPCEnv_Coordinate(e, C.byref(info)); L.IPCEnv_InitializeSamplesBuffer(e, 500, 1000, 16, 0, 2); L.IPCEnv_SetHops(e, 2); K.check()\n"
                    "for on in (1, 0):\n"
                    "    L.IPCEnv_SetAggLastHop(e, on)\n"
                    "    r = subprocess.run([sys.executable, '-c', %r], capture_output=True, text=True, timeout=120)\n"
                    "    print(r.stdout.strip(), r.stderr[-800:]); assert 'REFUSED %%d True' %% on in r.stdout\n"
                    "L.IPCEnv_Finalize(e); print('SERVER_OK')\n") % client
    r = subprocess.run([sys.executable, "-c", server], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SERVER_OK" in r.stdout, r.stdout[-2500:] + r.stderr[-2000:]
