"""The serving modes as one value (ServeModes, csrc/internal.h; DESIGN.md "Where a serving mode lives"), the parts that need no GPU: the
environment parser and the fan-out bound through the `legion` binary's boot, the pool's setters on a pool without scratch, and the merged
trainer-side client's refusal of a server in another hand-off than the test expects."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from harness import device_free_server

SERVER = os.path.join(ROOT, "legion-1_amd", "csrc", "legion")
MODE_VARS = ("LEGION_AGG_LAST_HOP", "LEGION_AGG_NORM", "LEGION_SAMPLING", "LEGION_SAMPLING_SEED")
# what the boot says when the modes were accepted: the meta line names a synth: workload that does not exist, which Server_Initialize
# refuses right behind the modes and before any device is touched
ACCEPTED = "Server_Initialize: the synth: dataset path names no known workload / scale"
NORM_NEEDS_AGG = "Server_Initialize: LEGION_AGG_NORM=both needs LEGION_AGG_LAST_HOP=1: only the last hop's neighbour sums are normalised"


# (fan-outs, the four variables, the refusal -- None: the boot goes on to the next check).  Every refusal text is the whole message.
NOT_A_SEED = "Server_Initialize: LEGION_SAMPLING_SEED=%s is not a sampling seed: a decimal or 0x hex integer in [0, 2^32), or unset (the same batches every epoch)"
BOOTS = [("64,5", env, None) for env in (
    {}, dict(LEGION_AGG_LAST_HOP="", LEGION_AGG_NORM="", LEGION_SAMPLING="", LEGION_SAMPLING_SEED=""),
    dict(LEGION_AGG_LAST_HOP="0"), dict(LEGION_AGG_LAST_HOP="1"), dict(LEGION_AGG_LAST_HOP="yes"),
    dict(LEGION_AGG_LAST_HOP="1", LEGION_AGG_NORM="both"), dict(LEGION_AGG_LAST_HOP="2", LEGION_AGG_NORM="both"),
    dict(LEGION_SAMPLING="replace"), dict(LEGION_SAMPLING="distinct"),
    dict(LEGION_SAMPLING_SEED="0"), dict(LEGION_SAMPLING_SEED="4294967295"), dict(LEGION_SAMPLING_SEED="0xDEADBEEF"), dict(LEGION_SAMPLING_SEED="0Xff"),
    dict(LEGION_AGG_LAST_HOP="1", LEGION_AGG_NORM="both", LEGION_SAMPLING="distinct", LEGION_SAMPLING_SEED="12345"))] + [
    ("65,2", dict(LEGION_SAMPLING="replace"), None),                                        # the bound is the distinct mode's alone
    ("10,5", dict(LEGION_AGG_NORM="left"), "Server_Initialize: LEGION_AGG_NORM=left is not a known norm: `both` (GraphConv norm='both', out-degree rsqrt inside block 1) or unset"),
    ("10,5", dict(LEGION_AGG_NORM="both"), NORM_NEEDS_AGG),
    ("10,5", dict(LEGION_AGG_NORM="both", LEGION_AGG_LAST_HOP="0"), NORM_NEEDS_AGG),
    ("10,5", dict(LEGION_AGG_NORM="both", LEGION_AGG_LAST_HOP="on"), NORM_NEEDS_AGG),          # atoi: non-numeric reads as off
    ("10,5", dict(LEGION_SAMPLING="unique"), "Server_Initialize: LEGION_SAMPLING=unique is not a known sampling mode: `replace` (the default: draws with replacement) or "
                                             "`distinct` (min(degree, fan-out) distinct neighbours per row)"),
    ("10,5", dict(LEGION_SAMPLING_SEED="-1"), NOT_A_SEED % "-1"), ("10,5", dict(LEGION_SAMPLING_SEED="4294967296"), NOT_A_SEED % "4294967296"),
    ("10,5", dict(LEGION_SAMPLING_SEED="0x"), NOT_A_SEED % "0x"), ("10,5", dict(LEGION_SAMPLING_SEED="12z"), NOT_A_SEED % "12z"),
    ("65,2", dict(LEGION_SAMPLING="distinct"), "Server_Initialize: LEGION_SAMPLING=distinct takes fan-outs of at most 64, hop 1 has 65: k_sample stages the picks of a "
                                               "tile's rows in static LDS"),
    ("10,5,65", dict(LEGION_SAMPLING="distinct", LEGION_AGG_LAST_HOP="1"), "Server_Initialize: LEGION_SAMPLING=distinct takes fan-outs of at most 64, hop 3 has 65: "),
    # the order the refusals are tested in: norm, sampling, seed, fan-out
    ("65,2", dict(LEGION_AGG_NORM="x", LEGION_SAMPLING="y", LEGION_SAMPLING_SEED="z"), "Server_Initialize: LEGION_AGG_NORM=x is not a known norm"),
    ("65,2", dict(LEGION_SAMPLING="y", LEGION_SAMPLING_SEED="z"), "Server_Initialize: LEGION_SAMPLING=y is not a known sampling mode"),
    ("65,2", dict(LEGION_SAMPLING="distinct", LEGION_SAMPLING_SEED="z"), NOT_A_SEED % "z"),
]


@pytest.mark.parametrize("fan,env_vars,refusal", [pytest.param(*c, id=c[0] + "-" + (",".join("%s=%s" % (k[7:], v) for k, v in c[1].items()) or "unset")) for c in BOOTS])
def test_boot_parses_the_four_variables(tmp_path, fan, env_vars, refusal):
    """The `legion` binary's boot: exit code 1 and exactly one Server_Initialize refusal -- the one the table names, or, for unset, empty and
    every valid value, that of the check behind the modes."""
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write("synth:nosuchworkload 512 1000 0 16 100 0 0 %d 1 0\n" % (1 << 30))
    env = {k: v for k, v in os.environ.items() if k not in MODE_VARS}
    env.update(env_vars, LEGION_IPC_NAMESPACE="cpumodes%d_" % os.getpid())
    r = subprocess.run([SERVER, "1", "0", fan, meta], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    said = r.stdout + r.stderr
    assert r.returncode == 1 and (refusal or ACCEPTED) in said, said[-2000:]
    assert len(set(re.findall(r"Server_Initialize: .*", said))) == 1, said[-2000:]


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
    seed = C.c_uint32(99)
    on = L.GPUMemoryPool_GetSampleSeed(pool, C.byref(seed))
    return (L.GPUMemoryPool_GetAggLastHop(pool), L.GPUMemoryPool_GetAggNorm(pool), L.GPUMemoryPool_GetSampleDistinct(pool), on, seed.value)


def last_error(L):
    msg = (L.legion_last_error() or b"").decode()
    L.legion_clear_error()
    return msg


def test_every_getter_returns_what_was_set_and_nothing_else_moves(pool_lib):
    L, pool = pool_lib
    want = [0, 0, 0, 0, 0]
    assert pool_modes(L, pool) == tuple(want) == pool_modes(L, None)
    for name, args, changed in (("SetSampleDistinct", (1,), {2: 1}), ("SetSampleSeed", (1, 0), {3: 1, 4: 0}), ("SetAggLastHop", (5,), {0: 1}),
                                ("SetAggNorm", (1,), {1: 1}), ("SetSampleSeed", (7, 0xFFFFFFFF), {3: 1, 4: 0xFFFFFFFF}), ("SetSampleDistinct", (0,), {2: 0}),
                                ("SetSampleSeed", (0, 5), {3: 0, 4: 5}), ("SetAggNorm", (0,), {1: 0}), ("SetSampleDistinct", (-3,), {2: 1}),
                                ("SetAggLastHop", (0,), {0: 0})):
        getattr(L, "GPUMemoryPool_" + name)(pool, *args)
        assert not L.legion_last_error(), (name, last_error(L))
        want = [changed.get(i, v) for i, v in enumerate(want)]
        assert pool_modes(L, pool) == tuple(want), (name, args)
        getattr(L, "GPUMemoryPool_" + name)(None, *args)
        assert last_error(L).count("GPUMemoryPool_%s: null pool" % name) == 1 and pool_modes(L, pool) == tuple(want), name


def test_norm_needs_the_aggregated_mode_and_survives_it_being_switched_off_and_on(pool_lib):
    L, pool = pool_lib
    L.GPUMemoryPool_SetAggNorm(pool, 1)
    msg = last_error(L)
    assert msg.count("GPUMemoryPool_SetAggNorm: the pool does not aggregate the last hop (GPUMemoryPool_SetAggLastHop first): only neighbour sums are normalised") == 1, msg
    assert pool_modes(L, pool) == (0, 0, 0, 0, 0)
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    L.GPUMemoryPool_SetAggNorm(pool, 1)
    assert not L.legion_last_error() and pool_modes(L, pool)[:2] == (1, 1)
    L.GPUMemoryPool_SetAggNorm(pool, 2)
    assert "GPUMemoryPool_SetAggNorm: unknown norm (0 = none, 1 = out-degree rsqrt)" in last_error(L) and pool_modes(L, pool)[:2] == (1, 1)
    L.GPUMemoryPool_SetAggLastHop(pool, 0)                   # leaves the norm in place ...
    assert not L.legion_last_error() and pool_modes(L, pool)[:2] == (0, 1)
    L.GPUMemoryPool_SetSampleDistinct(pool, 1)               # ... and so does every other setter while the aggregated mode is off
    L.GPUMemoryPool_SetSampleSeed(pool, 1, 3)
    assert not L.legion_last_error() and pool_modes(L, pool) == (0, 1, 1, 1, 3)
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    assert not L.legion_last_error() and pool_modes(L, pool) == (1, 1, 1, 1, 3)
    L.GPUMemoryPool_SetAggLastHop(pool, 0)
    L.GPUMemoryPool_SetAggNorm(pool, 0)
    L.GPUMemoryPool_SetAggNorm(pool, 1)                      # once dropped it cannot be asked for again without the aggregated mode
    assert "GPUMemoryPool_SetAggNorm: the pool does not aggregate the last hop" in last_error(L) and pool_modes(L, pool)[:2] == (0, 0)


def test_the_merged_client_exits_non_zero_on_a_server_in_another_hand_off():
    """tests/ipc_client_modes.py picks its get_next* by the server's own word, after checking the hand-off the test expects against it.  Device-free
    IPC env, a server in each hand-off, the check in a process of its own: exit code 9 and both names for another hand-off, 0 for the server's."""
    ns = "cpuipc_modes%d_" % os.getpid()
    pre, _ = device_free_server(ns, 2, "")
    client = pre + ("sys.path.insert(0, %r)\nimport ipc_client_modes as M\nM.ipc_service.initialize()\n"
                    "print('HAND_OFF', M.expect_hand_off(sys.argv[1]))\n") % os.path.join(ROOT, "tests")
    body = ("for agg, norm, said, expected in ((0, 0, 'plain', 'agg'), (1, 1, 'norm', 'agg'), (1, 0, 'agg', 'norm'), (1, 0, 'agg', 'agg')):\n"
            "    L.IPCEnv_SetAggLastHop(e, agg); L.IPCEnv_SetAggNorm(e, norm)\n"
            "    r = subprocess.run([sys.executable, '-c', %r, expected], capture_output=True, text=True, timeout=120)\n"
            "    print(r.returncode, r.stdout.strip(), r.stderr[-800:])\n"
            "    if said == expected:\n"
            "        assert r.returncode == 0 and 'HAND_OFF ' + said in r.stdout\n"
            "    else:\n"
            "        assert r.returncode == 9 and 'HAND_OFF' not in r.stdout and \"the server's hand-off is %%r, the test expects %%r\" %% (said, expected) in r.stdout\n") % client
    _, server = device_free_server(ns, 2, body)
    r = subprocess.run([sys.executable, "-c", server], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SERVER_OK" in r.stdout, r.stdout[-2500:] + r.stderr[-2000:]
    assert not [f for f in os.listdir("/dev/shm") if ns in f]
