"""tests/harness.py stands between a failing server and the rest of the GPU suite, so its own behaviour is tested here, without a GPU:
the `legion` binary and the trainers are replaced by a few lines of Python (no legion1_amd, no torch), the served records by the
oracle's own batches."""
import copy
import json
import subprocess
import sys
import time

import pytest

import harness
from conftest import sha
from harness import OUT, Children, assert_served_record, child_env, ipc_namespace, replay_served, serve_sets, served, wait_for_text

SLEEPER = [sys.executable, "-c", "import time; time.sleep(120)"]


def stand_in(code):
    return (sys.executable, "-c", code)


def server_code(exit_code, then="time.sleep(120)"):
    return stand_in("import sys, time; print('Train Steps: 3'); print(%r, flush=True); %s; print('stand-in leaves'); sys.exit(%d)" % (harness.READY, then, exit_code))


# ---- wait_for_text ---------------------------------------------------------------------------------
def test_wait_for_text_returns_when_the_word_appears(tmp_path):
    log = str(tmp_path / "log")
    with Children() as ch:
        p = ch.start(stand_in("import time; time.sleep(0.3); print('now ATTACHED', flush=True); time.sleep(120)"), log=log)
        wait_for_text(log, "ATTACHED", p, 30, 0.05)
        assert p.poll() is None
    assert p.poll() is not None


def test_wait_for_text_names_the_log_when_the_process_exits_first(tmp_path):
    log = str(tmp_path / "log")
    with Children() as ch:
        p = ch.start(stand_in("import sys; print('out of memory, giving up'); sys.exit(2)"), log=log)
        with pytest.raises(AssertionError, match="out of memory, giving up") as ex:
            wait_for_text(log, "ready", [p], 30, 0.05)
        assert "[2]" in str(ex.value)


def test_wait_for_text_kills_at_the_deadline(tmp_path):
    log = str(tmp_path / "log")
    with Children() as ch:
        p = ch.start(stand_in("import time; print('still loading', flush=True); time.sleep(120)"), log=log)
        t0 = time.time()
        with pytest.raises(AssertionError, match="still loading"):
            wait_for_text(log, "ready", p, 1.5, 0.05)
        assert 1.5 <= time.time() - t0 < 20 and p.poll() is not None


# ---- Children / served -----------------------------------------------------------------------------
def test_children_kills_on_every_way_out(tmp_path):
    for exc in (AssertionError, subprocess.TimeoutExpired, KeyboardInterrupt):
        with pytest.raises(exc):
            with Children() as ch:
                a, b = ch.start(SLEEPER), ch.start(SLEEPER, log=str(tmp_path / "b.log"))
                raise exc("x", 1) if exc is subprocess.TimeoutExpired else exc("x")
        assert a.poll() is not None and b.poll() is not None


def test_a_failing_body_leaves_no_server_and_no_client(tmp_path):
    with pytest.raises(ZeroDivisionError):
        with served(tmp_path, "meta line", [10, 5], server=server_code(0)) as srv:
            client = srv.children.start(SLEEPER, env=srv.env)
            assert srv.server.poll() is None and client.poll() is None
            1 / 0
    assert srv.server.poll() is not None and client.poll() is not None


def test_served_passes_the_command_line_and_one_environment_per_gpu(tmp_path):
    code = ("import json, os, sys; print(%r, flush=True)\n"
            "json.dump(dict(argv=sys.argv[1:], ns=os.environ['LEGION_IPC_NAMESPACE'], legacy=os.environ['HSA_ENABLE_IPC_MODE_LEGACY'],\n"
            "               x=os.environ.get('X')), open('server.json', 'w'))\n") % harness.READY
    script = tmp_path / "client.py"
    script.write_text("import json, os, sys\n"
                      "json.dump(dict(args=sys.argv[1:], g=os.environ['LEGION_IPC_DEVICE'], ns=os.environ['LEGION_IPC_NAMESPACE'],\n"
                      "               x=os.environ['X'], y=os.environ['Y']), open(sys.argv[2], 'w'))\n")
    with served(tmp_path, "the meta line", [5, 4, 3], G=2, agg_mode=1, env={"X": "1"}, server=stand_in(code)) as srv:
        got = srv.run_clients(str(script), [100, OUT, "tail"], client_env={"Y": "2"})
        assert srv.finish(audit_gpus=None) is None
    said = json.load(open(tmp_path / "server.json"))
    assert said["argv"] == ["2", "1", "5,4,3", str(tmp_path / "meta_config")] and open(tmp_path / "meta_config").read() == "the meta line"
    assert said["legacy"] == "0" and said["x"] == "1"
    assert [r["g"] for r in got] == ["0", "1"] and all(r["ns"] == said["ns"] and (r["x"], r["y"]) == ("1", "2") for r in got)
    assert [r["args"] for r in got] == [["100", str(tmp_path / ("client%d.json" % g)), "tail"] for g in range(2)]
    assert harness.READY in srv.log_text()


def test_a_server_that_exits_3_fails_finish_with_its_log(tmp_path):
    with served(tmp_path, "meta", [10], server=server_code(3, then="time.sleep(0.2)")) as srv:
        with pytest.raises(AssertionError, match="stand-in leaves"):
            srv.finish(audit_gpus=None)
    assert srv.server.returncode == 3


def test_a_client_that_exits_non_zero_fails_once_and_the_server_is_killed(tmp_path):
    script = tmp_path / "client.py"
    script.write_text("import sys; print('no such pipe'); sys.exit(5)\n")
    with pytest.raises(AssertionError, match="no such pipe"):
        with served(tmp_path, "meta", [10], server=server_code(0)) as srv:
            srv.run_clients(str(script), [OUT])
    assert srv.server.poll() is not None


def test_finish_reads_the_audit_line(tmp_path, monkeypatch):
    monkeypatch.setenv("LEGION_DEVICE_AUDIT", "1")
    monkeypatch.setattr(harness, "note_server_audit", lambda counts: None)      # a stand-in's line is no evidence for the terminal summary
    line = "Device audit: 201 checks, 0 violations, 0 unattributed, 7 launches with peer arguments"
    with served(tmp_path, "meta", [10], G=2, server=server_code(0, then="print(%r)" % line)) as srv:
        assert srv.finish() == dict(checks=201, violations=0, unattributed=0, peer_launches=7)      # more than 100 checks per GPU
        srv.G = 3
        with pytest.raises(AssertionError):
            srv.finish()
        assert srv.finish(audit_gpus=2)["checks"] == 201


def test_namespaces_are_distinct_and_short_enough(monkeypatch):
    names = [ipc_namespace("agg1") for _ in range(1000)]
    assert len(set(names)) == 1000
    # the bounds harness.NS_MAX states: vmm_sock_addr() cuts "<ns>legion_vmm_<dev>_<pipe>" to 106 bytes, a semaphore name holds NAME_MAX - 4 characters
    assert harness.NS_MAX == 90
    for ns in names:
        assert len(ns + "legion_vmm_99_99") <= 106 and len("/" + ns + "sem_r_99_99") <= 255 - 4
    with pytest.raises(AssertionError):
        ipc_namespace("x" * 90)
    monkeypatch.setenv("LEGION_LOG", "stderr")
    env = child_env("ns_", LEGION_LOG=None, LEGION_TABLES="host", N=3)
    assert "LEGION_LOG" not in env and (env["LEGION_IPC_NAMESPACE"], env["HSA_ENABLE_IPC_MODE_LEGACY"], env["LEGION_TABLES"], env["N"]) == ("ns_", "0", "host", "3")


# ---- replay ----------------------------------------------------------------------------------------
def test_replay_of_the_oracles_own_batches_passes_and_every_change_fails(synth, oracle):
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    B, fan, epochs, H = 128, [10, 5], 2, 2
    sets, steps, bs = serve_sets(oracle, ds, B)
    assert steps.tolist() == [6, 1, 18] and oracle.max_step(steps, epochs) == 32
    orc = oracle.OracleRunner(ds.indptr, ds.indices, ds.features, spec.V, spec.F, max(bs[0].values()), fan)    # evaluation batches are larger than B
    recs, modes = [], set()
    for b in range(32):     # the field layout of tests/ipc_client.py, H = 2
        mode, local = oracle.schedule(steps, epochs, b)
        modes.add(mode)
        ids = sets[0][mode]
        ref = orc.run_batch(ids, ds.labels[ids], local, mode=mode, batch_size=bs[0][mode])
        nc, ec = ref["nc"], ref["ec"]
        recs.append(dict(b=b, n=int(nc[9]), sizes=[int(nc[9]), int(nc[7]), int(nc[7]), int(nc[5])], edges=[int(ec[4]), int(ec[3])], ids=sha(ref["ids"]),
                         features=sha(ref["features"]), labels=sha(ref["labels"]), src=sha(ref["src_off"]), dst=sha(ref["dst_off"])))
    assert modes == {0, 1, 2}
    good = dict(steps=steps.tolist(), hops=H, batches=recs)

    def replay(got, steps=steps, **kw):
        return len([assert_served_record(rec, ref, H, **kw) for rec, ref, mode, local in replay_served(got, orc, sets[0], ds.labels, steps, epochs, bs[0])])

    def changed(b, drop=None, **fields):
        batches = copy.deepcopy(recs)
        batches[b].update(fields)
        batches[b].pop(drop, None)
        return dict(good, batches=batches)

    assert replay(good) == 32
    d = recs[20]["features"]
    with pytest.raises(AssertionError, match="batch 20: features"):
        replay(changed(20, features=d[:17] + ("0" if d[17] != "0" else "1") + d[18:]))
    with pytest.raises(AssertionError, match="batch 7: n is"):
        replay(changed(7, n=recs[7]["n"] + 1))
    with pytest.raises(AssertionError):
        replay(dict(good, batches=recs[:-1]))
    with pytest.raises(AssertionError, match="no 'labels'"):
        replay(changed(3, drop="labels"))
    assert replay(changed(3, drop="labels"), keys=tuple(k for k in harness.SERVED_KEYS if k != "labels")) == 32      # ... unless the caller says so
    other = serve_sets(oracle, ds, 256)[1]
    assert other.tolist() != steps.tolist()
    with pytest.raises(AssertionError):
        replay(good, steps=other)
