"""The logical-device audit (csrc/audit.h, $LEGION_DEVICE_AUDIT=1 -- on for every GPU test, tests/conftest.py).

The clique paths (Kg = 2 / 4 / 8), the one-process server over several GPUs and the peer exchange all run here with every logical
GPU mapped onto the box's ONE device, where a stream, allocation or launch made under the wrong device works anyway.  Under the
audit each of them carries the logical GPU it was created under and is checked on use; these tests show that the checks really run
(counts), that the multi-GPU paths are clean under them, and -- the negative controls -- that the mistakes the audit exists for are
caught: scratch allocated under the wrong GPU, a stream used under another GPU, an event recorded across GPUs, a table in a GPU's
memory that nobody enabled peer access to.  Reference behaviour being protected: one thread per GPU under cudaSetDevice(own)
(Server.cu:87-95,119-127), all-pairs peer access (GPUGraphStore.cu:145-168), shards and fragments on their owner
(GPU_Memory_Graph_Storage.cu:98-133, GPUCache.cu:769-826)."""
import ctypes as C

import numpy as np
import pytest

from conftest import KEYS_NO_FEATURES, assert_batch_equal
from harness import load_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    K = load_library()
    if not K.lib().legion_audit_enabled():
        pytest.skip("LEGION_DEVICE_AUDIT is off")
    return K


def counts(L):
    c = (C.c_int64 * 4)()
    L.legion_audit_counts(c)
    return dict(checks=c[0], violations=c[1], unattributed=c[2], peer_launches=c[3])


def messages(L):
    return [L.legion_audit_message(i).decode() for i in range(L.legion_audit_message_count())]


def expect_violation(K, pattern):
    """The audit recorded a violation matching `pattern`, and it is the sticky error of this thread; both are cleared."""
    L = K.lib()
    c, msgs = counts(L), messages(L)
    err = L.legion_last_error().decode()
    L.legion_audit_reset()
    L.legion_clear_error()
    assert c["violations"] >= 1 and any(pattern in m for m in msgs), (c, msgs)
    assert "device audit" in err, err
    return msgs


def clique_engine(K, oracle, synth, G, mode, cap_n=400, cap_e=300):
    spec = synth.spec_for("products", scale=0.004)
    ds = synth.generate(spec)
    parts = oracle.split_seeds(ds.train, G)
    B, fan = 32, [5, 4, 3]          # 786 training ids over up to 8 GPUs: two full batches per GPU
    steps = 2
    seeds = dict(train=[(p, ds.labels[p]) for p in parts])
    eng = K.Engine(ds.indptr, ds.indices, ds.features, spec.V, spec.F, seeds, B, fan, G=G, train_step=steps)
    eng.alloc_features()
    orcs = [oracle.OracleRunner(ds.indptr, ds.indices, ds.features, spec.V, spec.F, B, fan, partition_count=G) for _ in range(G)]
    for g in range(G):
        for it in range(steps):
            eng.run_batch(g, it, is_presc=True)
            assert_batch_equal(orcs[g].run_batch(parts[g], ds.labels[parts[g]], it, is_presc=True), eng.result(g, with_features=False), keys=KEYS_NO_FEATURES)
    eng.build_cache(cache_agg_mode=mode, node_capacity=cap_n, edge_capacity=cap_e, train_step=steps)
    return eng, ds, parts


@pytest.mark.parametrize("G,mode", [(2, 1), (4, 2), (8, 3)])
def test_clique_paths_are_clean_and_really_checked(K, oracle, synth, G, mode, monkeypatch):
    """Pre-sampling on G logical GPUs, ranking, cost-free fill-up of a Kg = G clique cache + CSR fragments, cached batches on every
    GPU with in-kernel peer reads and with the bulk-copy exchange: thousands of checks, no violation, nothing unattributed -- and the
    launches that read a peer's table are counted as such."""
    L = K.lib()
    L.legion_audit_reset()
    eng, ds, parts = clique_engine(K, oracle, synth, G, mode)
    for peer_gather in (None, "exchange"):
        if peer_gather:
            monkeypatch.setenv("LEGION_PEER_GATHER", peer_gather)
        for g in range(G):
            eng.run_batch(g, 0, per_level=(g % 2 == 0))
    K.check()
    c = counts(L)
    eng.close()
    assert c["violations"] == 0 and c["checks"] > 100 * G, (c, messages(L))
    assert c["unattributed"] == 0, c          # every stream / allocation / launch of the run had a logical GPU
    assert c["peer_launches"] > 0, c          # GPUs > 0 read the shared CSR / feature table of GPU 0 and the clique's rankings as peers


def test_scratch_pool_under_the_wrong_gpu_is_caught(K, oracle, synth):
    """The mistake VERDICT r05 names: a memory pool whose scratch was allocated while another GPU was current.  On one physical device
    it works; on a node its kernels would write a peer's memory (or fault).  The audit refuses the first launch."""
    L = K.lib()
    L.legion_audit_reset()
    eng, ds, parts = clique_engine(K, oracle, synth, 2, 1)
    L.SetGPUDevice(0)
    L.GPUMemoryPool_SetCurrentPipe(eng.pools[1], 0)
    # GPU 1's pool (allocated under SetGPUDevice(1)) driven as GPU 0
    L.batch_generator_kernel(None, eng.noder, eng.cache, eng.pools[1], 32, 0, 0, 0, K.TRAINMODE)
    L.d_stream_sync(None)
    msgs = expect_violation(K, "scratch of the memory pool: expected memory of logical GPU 0, got memory of logical GPU 1")
    assert any("k_seed: argument pos_map is memory of logical GPU 1" in m and "WRITTEN from logical GPU 0" in m for m in msgs), msgs
    eng.close()


def test_stream_and_event_of_another_gpu_are_caught(K):
    L = K.lib()
    L.legion_audit_reset()
    L.SetGPUDevice(1)
    s1, e1 = L.d_stream_create(), L.d_event_create()
    buf1 = K.DevBuf(4096)
    L.SetGPUDevice(0)
    s0 = L.d_stream_create()
    buf0 = K.DevBuf(4096)
    L.d_memset_async(buf0.ptr, 0, 4096, s1)                     # GPU 1's stream used while GPU 0 is current
    expect_violation(K, "hipMemsetAsync: stream of logical GPU 1")
    L.d_event_record(e1, s0)                                    # GPU 1's event on GPU 0's stream: hipErrorInvalidHandle on two devices
    expect_violation(K, "hipEventRecord: event of logical GPU 1")
    L.d_memset_async(buf0.ptr, 0, 4096, s0)                     # the legal forms stay silent
    L.d_stream_sync(s0)
    K.check()
    assert counts(L)["violations"] == 0
    L.SetGPUDevice(1)
    L.d_stream_destroy(s1); L.d_event_destroy(e1); buf1.free()
    L.SetGPUDevice(0)
    L.d_stream_destroy(s0); buf0.free()


def test_peer_memory_without_recorded_access_is_caught(K):
    """A kernel argument in another logical GPU's memory is legal only where the all-pairs enable of GPUGraphStorage_Build recorded
    peer access between the two (GPUGraphStore.cu:145-168).  Logical GPU 40 is in nobody's partition table."""
    L = K.lib()
    L.legion_audit_reset()
    L.legion_set_device_map(40, 0)
    L.SetGPUDevice(40)
    src = K.DevBuf.from_numpy(np.arange(4096, dtype=np.float32))
    L.SetGPUDevice(0)
    dst = K.DevBuf(4096 * 4)
    L.legion_copy_f4(None, dst.ptr, src.ptr, 4096 * 4)
    L.d_stream_sync(None)
    expect_violation(K, "k_copy_f4: argument src is memory of logical GPU 40")
    L.legion_copy_f4(None, src.ptr, dst.ptr, 4096 * 4)          # ... and nothing of this library may WRITE into another GPU's memory
    L.d_stream_sync(None)
    expect_violation(K, "k_copy_f4: argument dst is memory of logical GPU 40")
    L.SetGPUDevice(40)
    src.free()
    L.SetGPUDevice(0)
    dst.free()


def test_a_set_device_behind_the_librarys_back_is_caught(K):
    """HIP's own current device must be the physical device of the thread's logical GPU: a hipSetDevice that bypasses SetGPUDevice /
    DeviceGuard (another library, a forgotten restore) is reported at the next call.  One physical device: map logical GPU 1 onto a
    device id HIP is not on."""
    L = K.lib()
    L.legion_audit_reset()
    L.legion_set_device_map(41, 0)
    L.SetGPUDevice(41)
    L.legion_set_device_map(41, 5)          # from now on logical GPU 41 claims physical device 5, while HIP stays on 0
    b = L.d_alloc_space(256)
    expect_violation(K, "but HIP's current device is 0")
    L.legion_set_device_map(41, 0)
    L.d_free_space(b)
    L.SetGPUDevice(0)
