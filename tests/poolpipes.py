"""The memory pool's mode life cycle (a helper module, not collected by pytest): the setter sequence tests/test_scratch_poison_cpu.py walks on a
pool that never saw a device and tests/test_gpu_pool_pipes.py walks on one that owns scratch.  Both hold GPUMemoryPool_ScratchInfo's list at
every step to literals recorded from the library BEFORE the per-pipe buffers became one record per pipe and one table: they state what that
change had to keep."""

# (step, [(setter, argument)]): the pool's modes after a step are those of all steps so far.  The edge-weighted sums need the aggregated mode
# and edge ids and no norm, and are switched off before either.
STEPS = (
    ("fresh", []),
    ("edge ids on", [("GPUMemoryPool_SetEdgeIds", 1)]),
    ("edge ids off", [("GPUMemoryPool_SetEdgeIds", 0)]),
    ("aggregated last hop", [("GPUMemoryPool_SetAggLastHop", 1)]),
    ("norm", [("GPUMemoryPool_SetAggNorm", 1)]),
    ("edge-weighted sums", [("GPUMemoryPool_SetAggNorm", 0), ("GPUMemoryPool_SetEdgeIds", 1), ("GPUMemoryPool_SetAggEdgeWeight", 1)]),
    ("everything off", [("GPUMemoryPool_SetAggEdgeWeight", 0), ("GPUMemoryPool_SetEdgeIds", 0), ("GPUMemoryPool_SetAggLastHop", 0)]),
)


def walk(K, pool, steps=STEPS):
    """apply `steps` to `pool` one after the other; yields each step's name once its setters have run without leaving an error"""
    L = K.lib()
    for name, calls in steps:
        for setter, arg in calls:
            getattr(L, setter)(pool, arg)
            assert not L.legion_last_error(), (name, setter, L.legion_last_error())
        yield name


def listed(K, pool, pipe):
    """GPUMemoryPool_ScratchInfo's list for `pipe`: [(name, kind, element bytes, lifetime, per pipe, bytes)] and {name: pointer or None}"""
    got = K.pool_scratch(pool, pipe)
    assert len({b["name"] for b in got}) == len(got)
    return [(b["name"], b["kind"], b["elem_bytes"], b["lifetime"], b["per_pipe"], b["bytes"]) for b in got], {b["name"]: b["ptr"] for b in got}
