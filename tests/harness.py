"""What the GPU tests share (a plain helper module like props.py and pyref.py, not collected by pytest), in layers that stay usable on their own.
processes: SERVER, ipc_namespace, child_env, wait_for_text, Children, and on top of them served() -- one `legion` server, a trainer per GPU;
replay: serve_sets, replay_served, assert_served_record -- every served record against the oracle's batch of the same schedule slot;
in-process: K, make_engine, in_process_runner, attached_client -- a Runner of this process with a trainer process attached.
Nothing here retries: a process that exits non-zero or misses its deadline fails the test once, with the tail of its log."""
import contextlib
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys
import time
import types

import numpy as np
import pytest

from conftest import ROOT, note_server_audit, sha

TESTS = os.path.join(ROOT, "tests")
SERVER = os.path.join(ROOT, "legion-1_amd", "csrc", "legion")
READY = "System is ready for serving"


# ---- processes -----------------------------------------------------------------------------------
# The library builds its names from the namespace: "/<ns>sem_r_<dev>_<pipe>" (sem_name(), csrc/ipc_shm.cpp; POSIX: at most NAME_MAX - 4 =
# 251 characters) and the abstract socket "<ns>legion_vmm_<dev>_<pipe>", which vmm_sock_addr() (csrc/ipc_vmm.cpp) cuts SILENTLY to 106 bytes -- the tighter
# bound: with two digits each for device and pipe the suffix is 16 characters, so beyond 90 the per-pipe names would collide.
NS_MAX = 106 - len("legion_vmm_99_99")
_ns_counter = itertools.count()


def ipc_namespace(tag):
    """A namespace no other call of this session returns (pid + a process-wide counter), and no other session's process either."""
    ns = "t%d_%d_%s_" % (os.getpid(), next(_ns_counter), tag)
    assert len(ns) <= NS_MAX and "/" not in ns, ns
    return ns


def child_env(ns, **extra):
    """The environment of a server or trainer process of namespace `ns`; a value of None removes the variable."""
    env = dict(os.environ, LEGION_IPC_NAMESPACE=ns, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k, v in extra.items():
        if v is None:
            env.pop(k, None)
        else:
            env[k] = str(v)
    return env


def log_tail(path, n=3000):
    """The last n characters of a log (n = None: all of it); "" while the file does not exist."""
    if not os.path.exists(path):
        return ""
    with open(path, errors="ignore") as f:
        text = f.read()
    return text if n is None else text[-n:]


def wait_for_text(path, word, procs, timeout, poll):
    """Poll the file until `word` is in it.  A watched process that exits first fails the test; at the deadline the watched processes are
    killed and the test fails.  Both name the file's tail."""
    procs = [procs] if isinstance(procs, subprocess.Popen) else list(procs)
    t0 = time.time()
    while True:
        exited = [p for p in procs if p.poll() is not None]         # looked at BEFORE the read: its last words are in the file by then
        if word in log_tail(path, None):
            return
        if exited:
            raise AssertionError("exit code %s before %r appeared in %s:\n%s" % ([p.returncode for p in exited], word, path, log_tail(path)))
        if time.time() - t0 >= timeout:
            for p in procs:
                p.kill()
                p.wait()
            raise AssertionError("no %r in %s after %g s:\n%s" % (word, path, timeout, log_tail(path)))
        time.sleep(poll)


class Children:
    """Owns every process a test starts.  Leaving the block -- return, assertion, timeout, KeyboardInterrupt -- kills the ones still alive
    and closes their pipes; log files are closed as soon as the child holds them."""

    def __init__(self):
        self.procs = []

    def start(self, argv, log=None, err_log=None, **popen_kw):
        """log: stdout (and stderr, unless err_log names a file of its own) go to this file."""
        files = [open(p, "w") for p in (log, err_log) if p]
        try:
            if files:
                popen_kw.update(stdout=files[0], stderr=files[-1] if err_log else subprocess.STDOUT)
            p = subprocess.Popen([str(a) for a in argv], **popen_kw)
        finally:
            for f in files:
                f.close()
        self.procs.append(p)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.procs:
            if p.poll() is None:
                p.kill()
        for p in self.procs:
            p.wait()
            for pipe in (p.stdout, p.stderr):
                if pipe is not None:
                    pipe.close()
        return False


def audit_clean(log_text, gpus=1):
    """$LEGION_DEVICE_AUDIT=1 (tests/conftest.py): the server's summary line -- checks ran, none failed, and the server attributed every stream,
    allocation and launch to a logical GPU (returns the parsed counts; None when the audit is off)."""
    if os.environ.get("LEGION_DEVICE_AUDIT") != "1":
        return None
    m = re.search(r"Device audit: (\d+) checks, (\d+) violations, (\d+) unattributed, (\d+) launches with peer arguments", log_text)
    assert m, log_text[-1500:]
    checks, bad, unattributed, peer = (int(x) for x in m.groups())
    assert checks > 100 * gpus and bad == 0 and unattributed == 0, (m.group(0), log_text[-1500:])
    counts = dict(checks=checks, violations=bad, unattributed=unattributed, peer_launches=peer)
    note_server_audit(counts)
    return counts


def device_free_server(ns, hops, body):
    """(preamble, script) of a server process on the device-free IPC env ($LEGION_IPC_NO_DEVICE=1: the CPU tests of the "<name>_ext" words):
    one GPU, 3601 / 700 / 300 seeds at batch 500 -> steps [7, 2, 1]; `body` runs with L, the env `e`, np, C and subprocess in scope."""
    pre = ("import os, sys, ctypes as C; sys.path.insert(0, %r)\n"
           "os.environ['LEGION_IPC_NO_DEVICE'] = '1'; os.environ['LEGION_IPC_NAMESPACE'] = %r\n") % (ROOT, ns)
    return pre, pre + ("import numpy as np, subprocess\nimport legion1_amd.capi as K\nL = K.lib(); L.legion_set_error_mode(K.ERR_RETURN)\n"
                       "e = L.NewIPCEnv(1)\n"
                       "info = K.LegionBuildInfo(); info.partition_count = 1; info.epoch = 1; info.raw_batch_size = 500\n"
                       "tr, va, te = (np.array([x], np.int32) for x in (3601, 700, 300))\n"
                       "info.training_set_num, info.validation_set_num, info.testing_set_num = tr.ctypes.data, va.ctypes.data, te.ctypes.data\n"
                       "L.IPCEnv_Coordinate(e, C.byref(info)); L.IPCEnv_InitializeSamplesBuffer(e, 500, 1000, 16, 0, 2); L.IPCEnv_SetHops(e, %d); K.check()\n"
                       % hops) + body + "L.IPCEnv_Finalize(e); print('SERVER_OK')\n"


OUT = object()      # in run_clients' args: where the trainer's output path goes (tmp_path / client<g>.json)


class Served:
    """Handle of served(): the running server, its namespace and environment, its log."""

    def __init__(self, children, tmp_path, G, env):
        self.children, self.tmp_path, self.G, self.env = children, tmp_path, G, env
        self.log = str(tmp_path / "server.log")
        self.server = None

    def log_text(self):
        return log_tail(self.log, None)

    def run_clients(self, script, args, client_env=None, timeout=300):
        """tests/<script>, one process per GPU (LEGION_IPC_DEVICE=g, `client_env` on top of the server's environment), all running at
        once; each must exit 0.  Returns the JSON each wrote to the path that stands for OUT in `args`."""
        outs = [str(self.tmp_path / ("client%d.json" % g)) for g in range(self.G)]
        procs = [self.children.start([sys.executable, os.path.join(TESTS, script)] + [outs[g] if a is OUT else a for a in args],
                                     env=dict(self.env, LEGION_IPC_DEVICE=str(g), **(client_env or {})),
                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for g in range(self.G)]
        for g, p in enumerate(procs):
            said, _ = p.communicate(timeout=timeout)
            assert p.returncode == 0, "trainer %d: exit code %d\n%s\nserver:\n%s" % (g, p.returncode, said[-3000:], log_tail(self.log, 1500))
        return [json.load(open(o)) for o in outs]

    def run_one(self, argv, timeout):
        """One trainer process of another kind (examples/legion_sage_torch.py) in the server's environment; must exit 0.  Returns its stdout."""
        p = self.children.start(argv, env=self.env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        out, err = p.communicate(timeout=timeout)
        assert p.returncode == 0, out[-2000:] + err[-3000:]
        return out

    def finish(self, wait=60, audit_gpus="all"):
        """The server ends by itself with exit code 0 and, unless audit_gpus is None, a clean device-audit line with more than
        100 checks per GPU (default: all G); returns the audit counts."""
        self.server.wait(timeout=wait)
        assert self.server.returncode == 0, log_tail(self.log)
        if audit_gpus is not None:
            return audit_clean(self.log_text(), self.G if audit_gpus == "all" else audit_gpus)


@contextlib.contextmanager
def served(tmp_path, meta_line, fan, G=1, agg_mode=0, env=None, ready_timeout=240, server=(SERVER,)):
    """`legion G agg_mode fan meta_config` in tmp_path under a namespace of its own, `env` on top of child_env(); yields once the server is
    ready.  At most G + 1 processes exist at a time.  server: the argv prefix (the harness's own CPU tests put a stand-in there)."""
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write(meta_line)
    with Children() as children:
        h = Served(children, tmp_path, G, child_env(ipc_namespace("s"), **(env or {})))
        h.server = children.start(list(server) + [G, agg_mode, ",".join(map(str, fan)), meta], log=h.log, env=h.env, cwd=str(tmp_path))
        wait_for_text(h.log, READY, h.server, ready_timeout, 0.2)
        yield h


# ---- replay: the served schedule on the oracle ---------------------------------------------------
def serve_sets(oracle, ds, B, G=1, train=None, n_valid=None, n_test=None, part=None):
    """What a G-GPU server with batch size B serves from `ds`: per GPU its {mode: seed ids}, the step counts, per GPU its {mode: batch size}.
    train: per-GPU training lists served verbatim (meta flag 2); part: the partition file's owner array (meta flag 1); n_valid /
    n_test: the meta line takes the first n ids of each range.  Otherwise the tid % G split."""
    tr = train if train is not None else oracle.split_seeds(ds.train, G, part, int(part is not None))
    va, te = oracle.split_seeds(ds.valid[:n_valid], G), oracle.split_seeds(ds.test[:n_test], G)
    steps, tb, vb, sb = oracle.coordinate([len(p) for p in tr], [len(p) for p in va], [len(p) for p in te], B)
    return ([{0: tr[g], 1: va[g], 2: te[g]} for g in range(G)], steps, [{0: int(tb[g]), 1: int(vb[g]), 2: int(sb[g])} for g in range(G)])


def replay_served(got, orc, sets, labels, steps, epochs, batch_sizes):
    """One trainer's records against the schedule: as many as oracle.max_step says, and for each (rec, ref, mode, local) with ref the
    oracle's batch of that slot.  sets / batch_sizes: {mode: ...} of this trainer's GPU; labels: by node id."""
    import oracle
    assert len(got["batches"]) == oracle.max_step(steps, epochs), (len(got["batches"]), oracle.max_step(steps, epochs))
    for rec in got["batches"]:
        mode, local = oracle.schedule(steps, epochs, rec["b"])
        ids = sets[mode]
        yield rec, orc.run_batch(ids, labels[ids], local, mode=mode, batch_size=batch_sizes[mode]), mode, local


SERVED_KEYS = ("n", "sizes", "edges", "ids", "features", "labels", "src", "dst")        # what tests/ipc_client.py records per batch


def assert_served_record(rec, ref, hops, keys=SERVED_KEYS):
    """A trainer's record of one batch against the oracle's batch `ref`: counts word for word, buffers by SHA-256.  Like
    conftest.assert_batch_equal, a key the record does not carry is a failure -- a caller that means to leave one out passes `keys=`
    without it."""
    H, nc, ec = hops, ref["nc"], ref["ec"]
    want = dict(n=lambda: int(nc[5 + 2 * H]),
                sizes=lambda: [int(x) for k in range(1, H + 1) for x in (nc[5 + 2 * (H - k + 1)], nc[5 + 2 * (H - k)])],
                edges=lambda: [int(ec[2 + (H - k + 1)]) for k in range(1, H + 1)],
                ids=lambda: sha(ref["ids"]), features=lambda: sha(ref["features"]), labels=lambda: sha(ref["labels"]),
                src=lambda: sha(ref["src_off"]), dst=lambda: sha(ref["dst_off"]))
    for k in keys:
        assert k in rec, "batch %s: the record has no %r (has %s)" % (rec.get("b"), k, sorted(rec))
        w = want[k]()
        assert rec[k] == w, "batch %s: %s is %r, the oracle says %r" % (rec.get("b"), k, rec[k], w)


# ---- in-process: the library of this process -----------------------------------------------------
def load_library():
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    L.SetGPUDevice(0)
    return K


@pytest.fixture(scope="module")
def K():
    return load_library()


def make_engine(K, ds_or_arrays, B, fan, G=1, seeds=None, **kw):
    if hasattr(ds_or_arrays, "spec"):
        ds = ds_or_arrays
        V, F, indptr, indices, feats = ds.spec.V, ds.spec.F, ds.indptr, ds.indices, ds.features
        if seeds is None:
            import oracle as O
            parts = O.split_seeds(ds.train, G)
            seeds = dict(train=[(p, ds.labels[p]) for p in parts])
    else:
        V, F, indptr, indices, feats = ds_or_arrays
    eng = K.Engine(indptr, indices, feats, V, F, seeds, B, fan, G=G, **kw)
    eng.alloc_features()
    return eng


@contextlib.contextmanager
def in_process_runner(K, ds, B, fan, tag, features_buffer=True, presc_batches=0):
    """A one-GPU Runner of THIS process behind an IPCEnv under a namespace of its own, ready to Runner_RunOnce: yields .L, .ns, .eng, .env,
    .runner, .rp.  Whatever was created is released on every way out, newest first and each step whether or not the one before it
    failed: stream sync, Runner_Delete, IPCEnv_Finalize, eng.close(), legion_clear_error, the process-wide namespace back to ""."""
    L = K.lib()
    r = types.SimpleNamespace(L=L, ns=ipc_namespace(tag))
    with contextlib.ExitStack() as undo:
        L.legion_ipc_set_namespace(r.ns.encode())
        undo.callback(L.legion_ipc_set_namespace, b"")
        undo.callback(L.legion_clear_error)
        r.eng = make_engine(K, ds, B, fan)
        undo.callback(r.eng.close)
        r.env = L.NewIPCEnv(1)
        undo.callback(L.IPCEnv_Finalize, r.env)
        L.IPCEnv_Coordinate(r.env, C.byref(r.eng.info))
        r.fan = np.asarray(fan, dtype=np.int32)         # rp.fanout points into it
        rp = r.rp = K.RunnerParams()
        rp.device_id, rp.fanout, rp.hops = 0, r.fan.ctypes.data, len(fan)
        rp.cache, rp.graph, rp.noder, rp.env, rp.global_batch_id, rp.in_memory = r.eng.cache, r.eng.graph, r.eng.noder, r.env, 0, 1
        r.runner = L.NewGPURunner()
        undo.callback(L.Runner_Delete, r.runner)
        undo.callback(L.d_stream_sync, None)
        L.Runner_Initialize(r.runner, C.byref(rp))
        for b in range(presc_batches):                  # a pre-sampling epoch: the feature buffer is sized from its largest batch
            rp.global_batch_id = b
            L.Runner_RunPreSc(r.runner, C.byref(rp))
        if features_buffer:
            L.Runner_InitializeFeaturesBuffer(r.runner, C.byref(rp))
        L.GPUCache_SetPreSc(r.eng.cache, 0)
        K.check()
        yield r


def attached_client(children, script, args, env, log_path):
    """Start tests/<script> as the trainer of an in-process runner (output in log_path) and wait until it says ATTACHED."""
    p = children.start([sys.executable, os.path.join(TESTS, script)] + list(args), log=log_path, env=env)
    wait_for_text(log_path, "ATTACHED", p, 240, 0.1)
    return p
