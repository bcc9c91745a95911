"""Served edge ids / weights and the published serving modes (INTEGRATION.md "Edge ids"), the parts that need no GPU: the
three new variables through the `legion` binary's boot, the layout of the third shm object "<name>_ext2" on the device-free IPC env, the
trainer module without a server, the launcher's flags and the example's edge-weight layers."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from harness import device_free_server
from test_example_layers import _block, _load

SERVER = os.path.join(ROOT, "legion-1_amd", "csrc", "legion")
MODE_VARS = ("LEGION_AGG_LAST_HOP", "LEGION_AGG_NORM", "LEGION_SAMPLING", "LEGION_SAMPLING_SEED", "LEGION_LP_DRAW", "LEGION_WEIGHTED_DISTINCT",
             "LEGION_SHARED_DRAWS", "LEGION_EDGE_IDS", "LEGION_EDGE_WEIGHTS", "LEGION_AGG_EDGE_WEIGHT")
# what the boot says when the modes were accepted (tests/test_serve_modes_cpu.py): the refusal right behind them, before any device is touched
ACCEPTED = "Server_Initialize: the synth: dataset path names no known workload / scale"
UNKNOWN = "Server_Initialize: %s=%s is not a known setting: `1` ("
ALIAS = ("Server_Initialize: LEGION_EDGE_IDS=1 cannot be served under LEGION_SAMPLING=weighted without LEGION_WEIGHTED_DISTINCT=1: the alias table holds the alias "
         "neighbour's id, not its column")
NEEDS_IDS = "Server_Initialize: LEGION_EDGE_WEIGHTS=1 needs LEGION_EDGE_IDS=1: an edge's weight is served beside its id"
NEEDS_AGG, NEEDS_EID, NEEDS_W, NO_NORM = ("needs LEGION_AGG_LAST_HOP=1", "needs LEGION_EDGE_IDS=1", "needs retained edge weights (LEGION_EDGE_WEIGHTS=1, or "
                                          "LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1)", "must not be combined with LEGION_AGG_NORM")


def _e(**kw):
    return {"LEGION_" + k: v for k, v in kw.items()}


FULL = _e(AGG_LAST_HOP="1", EDGE_IDS="1", EDGE_WEIGHTS="1", AGG_EDGE_WEIGHT="1")
WD = _e(SAMPLING="weighted", WEIGHTED_DISTINCT="1")
# (the variables, what the refusal must contain -- () = accepted --, what it must not contain)
BOOTS = [(env, (), ()) for env in (
    _e(EDGE_IDS="", EDGE_WEIGHTS="", AGG_EDGE_WEIGHT=""), _e(EDGE_IDS="0", EDGE_WEIGHTS="0", AGG_EDGE_WEIGHT="0"),
    _e(EDGE_IDS="1"), _e(EDGE_IDS="1", EDGE_WEIGHTS="0"), _e(EDGE_IDS="1", EDGE_WEIGHTS="1"), _e(EDGE_IDS="1", SAMPLING="distinct"),
    _e(EDGE_IDS="1", EDGE_WEIGHTS="1", SAMPLING="distinct", SAMPLING_SEED="7", SHARED_DRAWS="1"),
    dict(WD, LEGION_EDGE_IDS="1"), dict(WD, LEGION_EDGE_IDS="1", LEGION_EDGE_WEIGHTS="1"), _e(EDGE_IDS="1", EDGE_WEIGHTS="1", AGG_LAST_HOP="1"),
    FULL, dict(FULL, LEGION_SAMPLING="distinct"), dict(WD, LEGION_AGG_LAST_HOP="1", LEGION_EDGE_IDS="1", LEGION_AGG_EDGE_WEIGHT="1"),
    dict(FULL, LEGION_AGG_EDGE_WEIGHT="0", LEGION_AGG_NORM="both"))] + [
    (_e(EDGE_IDS="yes"), (UNKNOWN % ("LEGION_EDGE_IDS", "yes"),), ()), (_e(EDGE_IDS="2"), (UNKNOWN % ("LEGION_EDGE_IDS", "2"),), ()),
    (_e(EDGE_IDS="1", SAMPLING="weighted"), (ALIAS,), ()), (_e(EDGE_IDS="1", SAMPLING="weighted", WEIGHTED_DISTINCT="0"), (ALIAS,), ()),
    (_e(EDGE_IDS="1", EDGE_WEIGHTS="on"), (UNKNOWN % ("LEGION_EDGE_WEIGHTS", "on"),), ()),
    (_e(EDGE_WEIGHTS="1"), (NEEDS_IDS,), ()), (dict(WD, LEGION_EDGE_WEIGHTS="1"), (NEEDS_IDS,), ()), (_e(EDGE_WEIGHTS="1", EDGE_IDS="0"), (NEEDS_IDS,), ()),
    (dict(FULL, LEGION_AGG_EDGE_WEIGHT="both"), (UNKNOWN % ("LEGION_AGG_EDGE_WEIGHT", "both"),), ()),
    # every missing condition is named, and only the missing ones
    (_e(AGG_EDGE_WEIGHT="1"), ("Server_Initialize: LEGION_AGG_EDGE_WEIGHT=1 ", NEEDS_AGG, NEEDS_EID, NEEDS_W), (NO_NORM,)),
    (dict(FULL, LEGION_AGG_LAST_HOP="0"), ("Server_Initialize: LEGION_AGG_EDGE_WEIGHT=1 ", NEEDS_AGG), (NEEDS_EID, NEEDS_W, NO_NORM)),
    (dict(FULL, LEGION_EDGE_WEIGHTS="0"), ("Server_Initialize: LEGION_AGG_EDGE_WEIGHT=1 ", NEEDS_W), (NEEDS_AGG, NEEDS_EID, NO_NORM)),
    (_e(AGG_LAST_HOP="1", AGG_EDGE_WEIGHT="1"), ("Server_Initialize: LEGION_AGG_EDGE_WEIGHT=1 ", NEEDS_EID, NEEDS_W), (NEEDS_AGG, NO_NORM)),
    (dict(FULL, LEGION_AGG_NORM="both"), ("Server_Initialize: LEGION_AGG_EDGE_WEIGHT=1 ", NO_NORM), (NEEDS_AGG, NEEDS_EID, NEEDS_W)),
    (dict(WD, LEGION_AGG_LAST_HOP="1", LEGION_AGG_NORM="both", LEGION_AGG_EDGE_WEIGHT="1"), ("Server_Initialize: LEGION_AGG_EDGE_WEIGHT=1 ", NEEDS_EID, NO_NORM), (NEEDS_AGG, NEEDS_W)),
    # the order: edge ids, edge weights, edge-weighted sums
    (_e(EDGE_IDS="x", EDGE_WEIGHTS="y", AGG_EDGE_WEIGHT="z"), (UNKNOWN % ("LEGION_EDGE_IDS", "x"),), ()),
    (_e(EDGE_IDS="1", EDGE_WEIGHTS="y", AGG_EDGE_WEIGHT="z"), (UNKNOWN % ("LEGION_EDGE_WEIGHTS", "y"),), ()),
]


@pytest.mark.parametrize("env_vars,refusal,absent", [pytest.param(*c, id=",".join("%s=%s" % (k[7:], v) for k, v in c[0].items())) for c in BOOTS])
def test_boot_parses_the_three_edge_variables(tmp_path, env_vars, refusal, absent):
    """The `legion` binary's boot: exit code 1 and exactly one Server_Initialize refusal before any device call -- the one the table names,
    or, for every accepted combination, that of the check behind the modes."""
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write("synth:nosuchworkload 512 1000 0 16 100 0 0 %d 1 0\n" % (1 << 30))
    env = {k: v for k, v in os.environ.items() if k not in MODE_VARS}
    env.update(env_vars, LEGION_IPC_NAMESPACE="cpuedges%d_" % os.getpid())
    r = subprocess.run([SERVER, "1", "0", "5,4", meta], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    said = r.stdout + r.stderr
    lines = set(re.findall(r"Server_Initialize: .*", said))
    assert r.returncode == 1 and len(lines) == 1, said[-2000:]
    line, = lines
    for text in refusal or (ACCEPTED,):
        assert text in line, (text, line)
    for text in absent:
        assert text not in line, (text, line)
    assert "Finish Reading" not in said        # refused at boot: nothing was read, no device touched


# ---- the layout of "<name>_ext2" -------------------------------------------------------------------
EXT2_BYTES = 108 + 8 * 2 * 2 * 64
WORDS = ("LpDraw", "WeightedDistinct", "SharedDraws", "EdgeIds", "EdgeWeights", "AggEdgeWeight")     # in the order of the words, at byte 52 + 4 i
CLIENT_WORDS = ("lp_draw", "weighted_distinct", "shared_draws", "edge_ids", "edge_weights", "agg_edge_weight")
# in a device-free server process: the names of the namespace, the six words and the _ext object as the files hold them
_LOOK = ("import struct, hashlib\n"
         "ns = os.environ['LEGION_IPC_NAMESPACE']\n"
         "def left(): return sorted(f for f in os.listdir('/dev/shm') if ns in f)\n"
         "PLAIN = sorted([ns + 'simpleIPCshm', ns + 'simpleIPCshm_ext'] + ['sem.' + ns + 'sem_%%s_0_%%d' %% (rw, q) for rw in 'rw' for q in (0, 1)])\n"
         "def raw2(): return open('/dev/shm/' + ns + 'simpleIPCshm_ext2', 'rb').read()\n"
         "def words(): return list(struct.unpack_from('<6i', raw2(), 52))\n"
         "def ext_file(): return open('/dev/shm/' + ns + 'simpleIPCshm_ext', 'rb').read()\n"
         "GET = [getattr(L, 'IPCEnv_Get' + n) for n in %r]; SET = [getattr(L, 'IPCEnv_Set' + n) for n in %r]\n") % (WORDS, WORDS)


def _run_server(ns, body, hops=2):
    _, server = device_free_server(ns, hops, _LOOK + body)
    try:
        r = subprocess.run([sys.executable, "-c", server], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "SERVER_OK" in r.stdout, r.stdout[-2500:] + r.stderr[-2500:]
        assert not [f for f in os.listdir("/dev/shm") if ns in f]                # IPCEnv_Finalize left nothing behind
        return r.stdout
    finally:
        for f in os.listdir("/dev/shm"):
            if ns in f:
                os.unlink(os.path.join("/dev/shm", f))


def test_a_server_with_every_word_off_leaves_exactly_todays_names():
    """Setting every word to 0, and reading every word, creates nothing: the slab, `_ext` and the 2 x 2 semaphores."""
    _run_server("cpuext2_off%d_" % os.getpid(),
                "assert left() == PLAIN, left()\n"
                "for s in SET: s(e, 0)\n"
                "assert [g(e) for g in GET] == [0] * 6 and L.IPCEnv_GetEdgeElems(e, 0) == 0; K.check()\n"
                "assert left() == PLAIN, left()\n"
                "assert len(ext_file()) == 2152\n")


@pytest.mark.parametrize("i", range(6), ids=WORDS)
def test_any_one_word_on_adds_the_pinned_ext2_and_changes_exactly_its_word(i):
    """The first setter of a word that is on creates `_ext2` of the pinned size (magic, the writer's size, the tie to the slab); each
    setter then changes exactly its word at the pinned position, and `_ext` keeps its 2152 bytes and every word it had."""
    _run_server("cpuext2_on%d_%d_" % (i, os.getpid()),
                ("i = %d\n" % i) +
                "L.IPCEnv_SetAggLastHop(e, 1); L.IPCEnv_SetSampling(e, 2); L.IPCEnv_SetSamplingSeed(e, 1, 77)\n"
                "before = ext_file(); assert len(before) == 2152\n"
                "SET[i](e, 5 if i == 0 else 1)\n"
                "assert left() == sorted(PLAIN + [ns + 'simpleIPCshm_ext2']), left()\n"
                "raw = raw2(); assert len(raw) == %d\n" % EXT2_BYTES +
                "magic, size, s0, s1, s2 = struct.unpack_from('<2I3i', raw, 0)\n"
                "assert (magic, size, [s0, s1, s2]) == (0x4C474E32, %d, [7, 2, 1]), (hex(magic), size, s0, s1, s2)\n" % EXT2_BYTES +
                "assert raw[20:52] == before[2100:2132] and raw[20:24] != bytes(4)      # the handle checksums of _ext: the tie to the slab\n"
                "want = [0] * 6; want[i] = 5 if i == 0 else 1\n"
                "assert words() == want and [g(e) for g in GET] == want, (words(), want)\n"
                "assert raw[76:] == bytes(len(raw) - 76)                                 # no edge buffers registered\n"
                "for j in range(6):\n"
                "    for v in ((3, 0) if j == 0 else (1, 0, -4)):\n"
                "        SET[j](e, v); want[j] = v if j == 0 else int(v != 0)\n"
                "        assert words() == want and [g(e) for g in GET] == want, (j, v, words(), want)\n"
                "        want[j] = 0; SET[j](e, 0)\n"
                "SET[0](e, -2); assert words()[0] == 0                                   # a negative k is off\n"
                "assert ext_file() == before; K.check()\n")


def test_registered_edge_buffers_publish_their_elements_and_no_handle_without_a_device():
    """IPCEnv_RegisterEdgeBuffers on the device-free env: edge_elems of the device at its pinned position, the handle slots stay zero, the
    object appears although every mode word is off; bad arguments are refused by name and change nothing."""
    _run_server("cpuext2_reg%d_" % os.getpid(),
                "L.IPCEnv_RegisterEdgeBuffers(e, 0, 0, None, None, 1234); L.IPCEnv_RegisterEdgeBuffers(e, 0, 1, None, None, 1234); K.check()\n"
                "raw = raw2(); assert len(raw) == %d and words() == [0] * 6\n" % EXT2_BYTES +
                "assert list(struct.unpack_from('<8i', raw, 76)) == [1234] + [0] * 7 and raw[108:] == bytes(8 * 2 * 2 * 64)\n"
                "assert L.IPCEnv_GetEdgeElems(e, 0) == 1234 and L.IPCEnv_GetEdgeElems(e, 1) == 0 and L.IPCEnv_GetEdgeElems(e, -1) == 0\n"
                "for bad in ((1, 0, 10), (0, 2, 10), (0, 0, 0)):\n"
                "    L.IPCEnv_RegisterEdgeBuffers(e, bad[0], bad[1], None, None, bad[2])\n"
                "    assert b'IPCEnv_RegisterEdgeBuffers: bad arguments' in (L.legion_last_error() or b''); L.legion_clear_error()\n"
                "assert raw2() == raw\n")


def _client_script(pre):
    """a trainer process: the six words through the C client and through ipc_service"""
    return pre + ("import legion1_amd.capi as K\nL = K.lib(); L.legion_set_error_mode(K.ERR_RETURN)\n"
                  "c = C.c_void_p(L.legion_ipc_client_open(0)); K.check(); assert c.value\n"
                  "print('C_WORDS', [getattr(L, 'legion_ipc_client_' + n)(c) for n in %r], L.legion_ipc_client_edge_elems(c),\n"
                  "      bool(L.legion_ipc_client_edge_buffer(c, 0)), bool(L.legion_ipc_client_edge_buffer(c, 1)), L.legion_ipc_client_hops(c))\n"
                  "L.legion_ipc_client_close(c)\n"
                  "sys.path.insert(0, %r)\nimport torch, ipc_service as S\nS.initialize()\n"
                  "print('PY_WORDS', [S.lp_draw(), S.weighted_distinct(), S.shared_draws(), S.edge_ids(), S.edge_weights(), S.aggregate_edge_weight()], S.sampling())\n"
                  "for f in (S.get_edge_ids, S.get_edge_weights):\n"
                  "    try:\n"
                  "        f(); print('NOT REFUSED')\n"
                  "    except RuntimeError as ex:\n"
                  "        print('REFUSED', str(ex).splitlines()[0])\n"
                  "S.finalize()\n") % (CLIENT_WORDS, os.path.join(ROOT, "legion-1_amd", "ipc_service"))


def test_a_client_process_reads_all_six_values_and_zeros_without_the_object():
    """A trainer process against a server with every word on (lp_draw = 341), then one word each, then none: through legion_ipc_client_*
    and through ipc_service.  `sampling()` stays "weighted" on a weighted-distinct server.  Before the first batch get_edge_ids() and
    get_edge_weights() raise by name; on a server that does not serve them they name the variables to start it with."""
    ns = "cpuext2_cl%d_" % os.getpid()
    pre, _ = device_free_server(ns, 3, "")
    out = _run_server(ns, ("client = %r\n" % _client_script(pre)) +
                      "def trainer():\n"
                      "    r = subprocess.run([sys.executable, '-c', client], capture_output=True, text=True, timeout=120)\n"
                      "    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]\n"
                      "    print(r.stdout, flush=True)\n"
                      "print('== none'); trainer(); assert left() == PLAIN\n"
                      "L.IPCEnv_SetSampling(e, 2)\n"
                      "for j, s in enumerate(SET): s(e, 341 if j == 0 else 1)\n"
                      "L.IPCEnv_RegisterEdgeBuffers(e, 0, 0, None, None, 99); L.IPCEnv_RegisterEdgeBuffers(e, 0, 1, None, None, 99)\n"
                      "print('== all'); trainer()\n"
                      "for j, s in enumerate(SET): s(e, 0)\n"
                      "SET[3](e, 1); print('== ids'); trainer()\n", hops=3)
    none, every, ids = (out.split("== " + k)[1].split("==")[0] for k in ("none", "all", "ids"))
    assert "C_WORDS [0, 0, 0, 0, 0, 0] 0 False False 3" in none and "PY_WORDS [0, False, False, False, False, False] replace" in none, none
    assert none.count("REFUSED") == 2 and "NOT REFUSED" not in none, none
    assert "REFUSED ipc_service.get_edge_ids: the server does not serve edge ids (start it with LEGION_EDGE_IDS=1)" in none, none
    assert "REFUSED ipc_service.get_edge_weights: the server does not serve edge ids (start it with LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1)" in none, none
    assert "C_WORDS [341, 1, 1, 1, 1, 1] 99 False False 3" in every and "PY_WORDS [341, True, True, True, True, True] weighted" in every, every
    assert every.count("REFUSED") == 2 and "NOT REFUSED" not in every, every
    assert "REFUSED ipc_service.get_edge_ids: no batch yet" in every and "REFUSED ipc_service.get_edge_weights: no batch yet" in every, every
    assert "C_WORDS [0, 0, 0, 1, 0, 0] 99" in ids and "PY_WORDS [0, False, False, True, False, False] weighted" in ids, ids
    assert "REFUSED ipc_service.get_edge_weights: the server does not serve edge weights (start it with LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1)" in ids, ids


def test_a_stale_ext2_is_ignored_removed_by_a_fresh_server_and_by_unlink_namespace():
    """A killed server's `_ext2` (a) under a slab another server re-created with other step counts: a client ignores it, every word reads 0;
    (b) under a fresh plain server of this build: NewIPCEnv removed it, the names are today's; (c) legion_ipc_unlink_namespace removes it."""
    ns = "cpuext2_stale%d_" % os.getpid()
    pre, full = device_free_server(ns, 2, "")
    killed = full.replace("L.IPCEnv_Finalize(e); print('SERVER_OK')\n", "") + "L.IPCEnv_SetEdgeIds(e, 1); L.IPCEnv_SetLpDraw(e, 9); K.check(); print('READY', flush=True); os._exit(0)\n"
    client = pre + ("import legion1_amd.capi as K\nL = K.lib(); L.legion_set_error_mode(K.ERR_RETURN)\n"
                    "c = C.c_void_p(L.legion_ipc_client_open(0)); K.check(); assert c.value\n"
                    "print('WORDS', [getattr(L, 'legion_ipc_client_' + n)(c) for n in %r], flush=True); os._exit(0)\n") % (CLIENT_WORDS,)
    run = lambda code: subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    names = lambda: sorted(f for f in os.listdir("/dev/shm") if ns in f)
    try:
        r = run(killed)
        assert r.returncode == 0 and "READY" in r.stdout, r.stdout + r.stderr[-2000:]
        assert ns + "simpleIPCshm_ext2" in names() and len(names()) == 3 + 4, names()
        assert "WORDS [9, 0, 0, 1, 0, 0]" in run(client).stdout                                  # against the live slab it is honoured
        with open("/dev/shm/" + ns + "simpleIPCshm", "r+b") as f:                               # (a) another server's slab: other step counts
            f.write((11).to_bytes(4, "little") + (3).to_bytes(4, "little") + (2).to_bytes(4, "little"))
        assert "WORDS [0, 0, 0, 0, 0, 0]" in run(client).stdout
        # (b) a fresh plain server of the namespace inherits nothing
        out = _run_server_keep(ns, "assert left() == PLAIN, left()\nassert [g(e) for g in GET] == [0] * 6\n")
        assert "SERVER_OK" in out
        # (c) a killed server again, then the clean-up call
        r = run(killed)
        assert "READY" in r.stdout and ns + "simpleIPCshm_ext2" in names()
        r = run(pre + "import legion1_amd.capi as K\nK.lib().legion_ipc_unlink_namespace(%r.encode(), 8); print('UNLINKED')\n" % ns)
        assert "UNLINKED" in r.stdout and names() == [], (r.stdout + r.stderr[-1500:], names())
    finally:
        for f in os.listdir("/dev/shm"):
            if ns in f:
                os.unlink(os.path.join("/dev/shm", f))


def _run_server_keep(ns, body):
    _, server = device_free_server(ns, 2, _LOOK + body)
    r = subprocess.run([sys.executable, "-c", server], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    assert not [f for f in os.listdir("/dev/shm") if ns in f]
    return r.stdout


# ---- the trainer module, the launcher, the example -------------------------------------------------
def test_the_new_ipc_service_functions_need_initialize():
    sys.path.insert(0, os.path.join(ROOT, "legion-1_amd", "ipc_service"))
    import ipc_service
    calls = [(getattr(ipc_service, n), ()) for n in ("lp_draw", "weighted_distinct", "shared_draws", "edge_ids", "edge_weights", "aggregate_edge_weight",
                                                     "get_edge_ids", "get_edge_weights")] + [(ipc_service.get_next_aggregated_edge_weight, (16,))]
    for fn, args in calls:
        with pytest.raises(RuntimeError, match=r"ipc_service\.initialize\(\) was not called"):
            fn(*args)


def test_the_launcher_maps_the_three_flags_and_its_default_line_is_unchanged(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("launch_server", os.path.join(ROOT, "legion-1_amd", "launch_server.py"))
    ls = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ls)
    monkeypatch.chdir(tmp_path)
    for v in MODE_VARS:
        monkeypatch.delenv(v, raising=False)
    started = []
    monkeypatch.setattr(ls.subprocess, "call", lambda cmd, env: started.append((cmd, {k: v for k, v in env.items() if k in MODE_VARS})) or 0)
    base = ["--dataset", "PR", "--gpu_number", "1"]
    for flags, want in (([], {}), (["--edge_ids"], _e(EDGE_IDS="1")), (["--edge-ids", "--edge-weights"], _e(EDGE_IDS="1", EDGE_WEIGHTS="1")),
                        (["--edge_ids", "--edge_weights", "--agg_edge_weight"], _e(EDGE_IDS="1", EDGE_WEIGHTS="1", AGG_EDGE_WEIGHT="1")),
                        (["--agg-edge-weight"], _e(AGG_EDGE_WEIGHT="1"))):
        assert ls.main(base + flags) == 0
        assert started[-1][1] == want, (flags, started[-1][1])
        assert started[-1][0] == started[0][0]                      # the command line is the default's whatever the flags
    cmd = started[0][0]
    assert cmd[0].endswith(os.path.join("csrc", "legion")) and cmd[1:4] == ["1", "0", "25,10"] and cmd[4] == os.path.abspath("meta_config") and len(cmd) == 5


def _weighted(block, n_src, n_dst, seed):
    """edge weights for a block of test_example_layers._block and the dense A_w they make (duplicate edges add up), float64"""
    src, dst = block[0], block[1]
    w = torch.rand(src.shape[0], generator=torch.Generator().manual_seed(seed), dtype=torch.float64) + 0.25
    A = torch.zeros(n_dst, n_src, dtype=torch.float64).index_put_((dst, src), w, accumulate=True)
    return w, A


def test_graphconv_edge_weight_matches_dense_definition():
    m = _load()
    block, _, h = _block(seed=5)
    w, A_w = _weighted(block, block[2], block[3], 6)
    layer = m.GraphConvEdgeWeight(16, 8).double()
    assert torch.allclose(layer(block + (w,), h), layer.fc(A_w @ h), atol=1e-12)
    assert not torch.allclose(layer(block + (torch.ones_like(w),), h), layer.fc(A_w @ h), atol=1e-3)      # the weights are read


def test_fused_edge_weight_layer_given_exact_sums_equals_the_unfused_layer():
    """A block whose first e_in edges have sources among the dst nodes (the hops < H) and whose other edges come in runs of `fan` per input
    slot (the last hop): the fused layer over x_in and the exact per-slot sums sum_e w_e h[src_e] equals the unfused layer over every row."""
    m = _load()
    g = torch.Generator().manual_seed(11)
    n_dst, n_src, e_in, slots, fan = 20, 50, 60, 30, 3
    src = torch.cat([torch.randint(0, n_dst, (e_in,), generator=g), torch.randint(n_dst, n_src, (slots * fan,), generator=g)])
    run_dst = torch.randint(0, n_dst, (slots,), generator=g)
    dst = torch.cat([torch.randint(0, n_dst, (e_in,), generator=g), run_dst.repeat_interleave(fan)])
    h = torch.randn(n_src, 16, generator=g, dtype=torch.float64)
    w = torch.rand(src.shape[0], generator=g, dtype=torch.float64) + 0.25
    sums = (h[src[e_in:]] * w[e_in:, None]).view(slots, fan, 16).sum(1)
    plain, fused = m.GraphConvEdgeWeight(16, 8).double(), m.GraphConvEdgeWeightFused(16, 8).double()
    fused.load_state_dict(plain.state_dict())
    want = plain((src, dst, n_src, n_dst, w), h)
    got = fused((src, dst, n_src, n_dst, e_in, run_dst, sums, w), h[:n_dst])
    assert torch.allclose(got, want, atol=1e-12)
