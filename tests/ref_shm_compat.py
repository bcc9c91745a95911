"""The reference's shm helper against the product's hand-off slab -- in both directions, without a GPU ($LEGION_IPC_NO_DEVICE=1).  Run by
tests/test_ref_shm_compat.py in a process of its own.   python tests/ref_shm_compat.py <namespace> <ref|standin>

Two implementations of the helper's sharedMemoryCreate / sharedMemoryClose play the reference's part:
  ref      its OWN code: oracle/_ref/libhelper_multiprocess_ref.so, compiled by `make -C oracle ref` from the reference tree where that tree
           exists (git-ignored, never part of this repository)
  standin  StandInHelper below -- what that code does, in Python: shm_open(O_RDWR | O_CREAT, 0777) + ftruncate(size) + mmap(MAP_SHARED).
           tests/golden/ref_shm_helper.json holds what the REAL helper did in observe()'s cases (object sizes, modes, bytes kept or cut;
           `python oracle/make_golden_ref_shm.py` where the library exists), and the stand-in must do exactly the same: the checks below run
           on every checkout.

What the reference does with the slab (and nothing else is exercised here): both its server (CUDA_IPC_Service.cu:43-51) and its trainer
extension (ipc_cuda_kernel.cu:44-51) call sharedMemoryCreate("simpleIPCshm", sizeof(shmStruct) = 7180): shm_open(O_RDWR | O_CREAT) +
ftruncate(7180) + mmap; the server zeroes it and writes steps[3] and the 8 x 2 x 7 IPC handles; the trainer reads them."""
import ctypes as C
import hashlib
import mmap
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF_SLAB = 12 + 8 * 2 * 7 * 64          # sizeof(shmStruct) of the reference: int32 steps[3] + cudaIpcMemHandle_t[8][2][7]
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libhelper_multiprocess_ref.so")


class ShmInfo(C.Structure):             # sharedMemoryInfo (helper_multiprocess.h): addr, size, shmFd
    _fields_ = [("addr", C.c_void_p), ("size", C.c_size_t), ("fd", C.c_int)]


class StandInHelper:
    """sharedMemoryCreate / sharedMemoryClose on POSIX shared memory (/dev/shm), same signatures as the library's: create(name, size,
    byref(ShmInfo)) -> 0 or errno, close(byref(ShmInfo))."""

    def __init__(self):
        self.maps = {}

    def create(self, name, size, info_ref):
        si = info_ref._obj
        si.size = size
        try:
            fd = os.open("/dev/shm/" + name.decode(), os.O_RDWR | os.O_CREAT | os.O_NOFOLLOW | os.O_CLOEXEC, 0o777)
        except OSError as ex:
            return ex.errno
        si.fd = fd
        os.ftruncate(fd, size)
        m = mmap.mmap(fd, size, mmap.MAP_SHARED, mmap.PROT_READ | mmap.PROT_WRITE)
        anchor = C.c_char.from_buffer(m)
        si.addr = C.addressof(anchor)
        self.maps[si.addr] = (m, anchor)
        return 0

    def close(self, info_ref):
        si = info_ref._obj
        m, anchor = self.maps.pop(si.addr)
        del anchor
        m.close()
        os.close(si.fd)


def helper(kind):
    """(create, close) of the reference's helper: its own library (kind "ref") or the stand-in."""
    if kind == "standin":
        h = StandInHelper()
        return h.create, h.close
    ref = C.CDLL(REF_LIB)
    create, close = ref._Z18sharedMemoryCreatePKcmP19sharedMemoryInfo_st, ref._Z17sharedMemoryCloseP19sharedMemoryInfo_st
    create.argtypes, create.restype = [C.c_char_p, C.c_size_t, C.POINTER(ShmInfo)], C.c_int
    close.argtypes = [C.POINTER(ShmInfo)]
    return create, close


def observe(kind, ns):
    """What the helper does to a shared object, case by case: no object yet, one of its own size with data in it, a longer one, a shorter one;
    then a write through its mapping.  Returns JSON-able facts (the golden file records the library's)."""
    create, close = helper(kind)
    name = ns + "probe"
    path = "/dev/shm/" + name
    pattern = bytes((7 * i + 3) & 0xFF for i in range(REF_SLAB + 4096))
    out = {}
    old = os.umask(0o022)
    try:
        for case, before in (("absent", None), ("same_size", pattern[:REF_SLAB]), ("longer", pattern), ("shorter", pattern[:12])):
            if before is not None:
                with open(path, "wb") as f:
                    f.write(before)
            si = ShmInfo()
            rc = create(name.encode(), REF_SLAB, C.byref(si))
            st = os.stat(path)
            with open(path, "rb") as f:
                data = f.read()
            mapped = C.string_at(si.addr, REF_SLAB)
            out[case] = {"rc": rc, "size": st.st_size, "mode": oct(st.st_mode & 0o777), "mapping_is_the_object": mapped == data[:REF_SLAB],
                         "sha256": hashlib.sha256(data).hexdigest()}
            if case == "shorter":       # a write through the mapping reaches the object
                (C.c_int32 * 3).from_address(si.addr)[:] = [1388, 196, 196]
                with open(path, "rb") as f:
                    out["write_through"] = {"head": f.read(12).hex()}
            close(C.byref(si))
            os.unlink(path)
    finally:
        os.umask(old)
        if os.path.exists(path):
            os.unlink(path)
    return out


def main(ns, kind):
    os.environ["LEGION_IPC_NO_DEVICE"] = "1"
    os.environ["LEGION_IPC_NAMESPACE"] = ns
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    create, close = helper(kind)
    name = (ns + "simpleIPCshm").encode()                 # the reference's literal name behind the test's namespace prefix
    path = "/dev/shm/" + name.decode()

    # ---- 1. OUR server's slab, then the REFERENCE trainer's open (sharedMemoryCreate: it ftruncate()s the object to ITS size) ----
    e = C.c_void_p(L.NewIPCEnv(8))
    info = K.LegionBuildInfo()
    nums = [(C.c_int32 * 8)(*[4001 + i for i in range(8)]), (C.c_int32 * 8)(*[600] * 8), (C.c_int32 * 8)(*[100] * 8)]
    info.partition_count, info.epoch, info.raw_batch_size = 8, 3, 500
    info.training_set_num, info.validation_set_num, info.testing_set_num = [C.cast(a, C.c_void_p) for a in nums]
    L.IPCEnv_Coordinate(e, C.byref(info))
    for d in range(8):
        L.IPCEnv_InitializeSamplesBuffer(e, 500, 1000, 16, d, 2)
    L.IPCEnv_SetHops(e, 3)
    K.check()
    assert os.stat(path).st_size == REF_SLAB, "the shared object must be exactly the reference's struct"
    si = ShmInfo()
    assert create(name, REF_SLAB, C.byref(si)) == 0 and si.addr
    assert os.stat(path).st_size == REF_SLAB                                  # its ftruncate changed nothing
    steps = (C.c_int32 * 3).from_address(si.addr)
    assert list(steps) == [8, 2, 1], list(steps)                              # (4001 - 1) // 500, (600 - 1) // 512 + 1, (100 - 1) // 512 + 1
    table = (C.c_ubyte * (8 * 2 * 7 * 64)).from_address(si.addr + 12)         # the handle table sits where the reference reads it
    assert not any(table)                                                     # (no device: every slot zero)
    # what rounds 1-4 appended behind the struct now lives in its own object: the reference's ftruncate cannot cut it off.
    # The server keeps writing its extension words for EVERY device and a client of ours keeps reading them:
    for d in range(8):
        for p in range(2):
            L.IPCEnv_SetMirror(e, d, p, 100 * d + p + 1, 7)
    os.environ["LEGION_IPC_DEVICE"] = "7"
    c = C.c_void_p(L.legion_ipc_client_open(-1))
    K.check()
    assert L.legion_ipc_client_hops(c) == 3
    L.IPCEnv_IPCPost(e, 7, 0)
    L.legion_ipc_client_wait(c)
    nc, ec = (C.c_int32 * 16)(), (C.c_int32 * 16)()
    L.legion_ipc_client_read_counters(c, nc, ec)
    assert list(nc) == [701] * 16 and list(ec) == [7] * 16
    L.legion_ipc_client_close(c)
    close(C.byref(si))
    L.IPCEnv_Finalize(e)
    K.check()
    assert not os.path.exists(path) and not os.path.exists(path + "_ext")

    # ---- 2. the REFERENCE server's slab (created, zeroed and filled the way CUDA_IPC_Service.cu:44-51,130-133 does), then OUR client ----
    si = ShmInfo()
    assert create(name, REF_SLAB, C.byref(si)) == 0
    C.memset(si.addr, 0, REF_SLAB)
    (C.c_int32 * 3).from_address(si.addr)[:] = [1388, 196, 196]
    os.environ["LEGION_IPC_DEVICE"] = "2"
    c = C.c_void_p(L.legion_ipc_client_open(-1))
    K.check()
    assert c.value
    got = (C.c_int32 * 3)()
    L.legion_ipc_client_steps(c, got)
    assert list(got) == [1388, 196, 196]
    assert L.legion_ipc_client_hops(c) == 2 and L.legion_ipc_client_feature_rows(c) == 0      # no extension object: the reference's 2-hop layout
    assert os.stat(path).st_size == REF_SLAB and not os.path.exists(path + "_ext")            # our client neither grew the slab nor created the extension
    L.legion_ipc_client_close(c)
    close(C.byref(si))
    for f in os.listdir("/dev/shm"):
        if ns in f:
            os.unlink(os.path.join("/dev/shm", f))
    print("REF_SHM_COMPAT_OK")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
