"""Poison for the memory pool's scratch (a helper module, not collected by pytest): what tests/test_gpu_scratch_poison.py writes into every
buffer GPUMemoryPool_ScratchInfo lists as dead, and the rules tests/test_scratch_poison_cpu.py holds the generator to.

The design rule: a kernel that wrongly consumes a poisoned word computes a WRONG BATCH and never forms a wild address or an endless loop.
So every value is one the buffer could legitimately hold at another time:
  id              node ids in [0, limit) that are not the running batch's (all of [0, limit) when the batch holds every node), and -1
  slot_state      -1 (claim pending) and -2 - s ("lost to slot s") with s < i, the word's own index, and s inside the hop's slot range: a
                  chain of poisoned states strictly descends, so following it ends
  count(_pair)    values in [0, tile], mostly 1, whose sum over the whole buffer stays below `budget` (the pool's num_ids / 4): no prefix of
                  them reaches the capacity of the batch's buffers
  device_pointer  NULL, or the address of a row of a decoy buffer the test owns (rows of NAN_BITS)
  float           NAN_BITS, a quiet NaN with a payload no arithmetic produces
  table_entry     (e << 32) | v with the epoch e in (the running batch's, kEpochTop]; v arbitrary: provisional claims, positions inside
                  the batch, anything
and two uniform fills, all-zero and all-0xFF, for every kind but device pointers (a pattern byte is no address) and, for all-zero, but
the table: a zero entry has epoch 0, BELOW every running epoch, which by the table's rule is a live entry of the running batch, not a
stale one -- the table's all-0xFF fill is what GPUMemoryPool_AllocateScratch writes."""
import numpy as np

NAN_BITS = 0x7FC5CA7E                       # quiet NaN, payload 0x5CA7E
EPOCH_TOP, PROVISIONAL, POS_MASK = 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF      # kEpochTop, kProvisional, kPosValueMask (csrc/internal.h)
TILE_NARROW, TILE_WIDE = 256, 1024          # kTileNarrow, kTile
FILLS = ("random", "zero", "ones")          # "ones": every byte 0xFF
KINDS = ("id", "slot_state", "count", "count_pair", "device_pointer", "float", "table_entry")
# GPUMemoryPool_ScratchInfo's list, literally: a buffer added to the pool fails tests/test_scratch_poison_cpu.py until it has a lifetime here
EXPECTED_TABLE = [
    ("pos_map", "table_entry", 8, "table", False),
    ("cand", "id", 4, "hop", False),
    ("aux2[0]", "slot_state", 4, "batch", False),
    ("aux2[1]", "slot_state", 4, "batch", False),
    ("tile_edge", "count", 4, "hop", False),
    ("tile_node", "count", 4, "hop", False),
    ("tile_pre", "count_pair", 8, "hop", False),
    ("chunk_tot", "count_pair", 8, "hop", False),
    ("hop_state", "count", 4, "hop", False),
    ("cache_search_buffer", "id", 4, "batch", False),
    ("row_ptr", "device_pointer", 8, "batch", False),
    ("agg_src_ids", "id", 4, "batch", False),
    ("tmp_part_ind", "id", 1, "batch", False),
    ("tmp_part_off", "id", 4, "batch", False),
    ("cand_pipe", "id", 4, "batch", True),
    ("agg_out_deg", "count", 4, "batch", True),
    ("agg_wdraw", "float", 4, "batch", True),
    ("agg_chunk_cnt", "count", 4, "batch", True),
    ("ctl", "count", 4, "state", False),
]
GATHER_SCRATCH = ("row_ptr", "cache_search_buffer", "tmp_part_ind", "tmp_part_off")     # dead in front of every gather op of a batch


class Decoy:
    """V rows of `pitch` floats of NAN_BITS on the current device: where a poisoned row pointer points."""

    def __init__(self, K, V, pitch):
        self.V, self.pitch = int(V), int(pitch)
        self.buf = K.DevBuf.from_numpy(np.full(self.V * self.pitch, NAN_BITS, np.uint32))

    def rows(self, r):
        return np.uint64(self.buf.ptr) + np.asarray(r, dtype=np.uint64) * np.uint64(4 * self.pitch)

    def free(self):
        self.buf.free()


def _counts(n, rng, tile, budget):
    """n counts in [0, tile] whose sum is at most budget: ones wherever the budget allows, a few larger values from what is left"""
    out = np.zeros(n, np.int32)
    budget = max(int(budget), 0)
    ones = min(n, budget // 2)
    out[rng.permutation(n)[:ones]] = 1
    left = budget - ones
    for i in rng.randint(0, max(n, 1), size=min(8, n)):
        v = int(rng.randint(0, tile + 1))
        if v - int(out[i]) <= left:
            left -= v - int(out[i])
            out[i] = v
    return out


def generate(kind, nbytes, elem_bytes, rng, fill="random", limit=1, avoid=(), slots=1, tile=TILE_NARROW, budget=0, epoch=0, decoy=None):
    """The poison of one buffer: a C-contiguous array of exactly nbytes bytes.  limit: ids are below it (V; the clique's cache slots for
    cache_search_buffer); avoid: the running batch's ids; slots: the hop's slot range; epoch: the epoch the next batch runs under."""
    assert kind in KINDS and fill in FILLS and nbytes % elem_bytes == 0
    n = nbytes // elem_bytes
    if kind == "device_pointer":                              # never a pattern byte, whatever the fill
        assert elem_bytes == 8
        out = np.zeros(n, np.uint64)
        if decoy is not None:
            out = np.where(rng.rand(n) < 0.25, np.uint64(0), decoy.rows(rng.randint(0, decoy.V, size=n))).astype(np.uint64)
        return out
    if fill == "ones" or (fill == "zero" and kind != "table_entry"):
        return np.full(nbytes, 0xFF if fill == "ones" else 0, np.uint8)
    if kind == "id":
        dtype = {1: np.int8, 4: np.int32}[elem_bytes]
        limit = min(int(limit), 127) if elem_bytes == 1 else int(limit)
        pool = np.setdiff1d(np.arange(limit, dtype=np.int64), np.asarray(avoid, dtype=np.int64))
        if len(pool) == 0:
            pool = np.arange(max(limit, 1), dtype=np.int64)
        out = pool[rng.randint(0, len(pool), size=n)]
        out[rng.rand(n) < 0.25] = -1
        return out.astype(dtype)
    if kind == "slot_state":
        i = np.arange(n, dtype=np.int64)
        s = (i // 2) % max(int(slots), 1)                     # s < i for every i >= 1, and inside the hop's slot range
        out = np.where((i == 0) | (rng.rand(n) < 0.34), -1, -2 - s)
        return out.astype(np.int32)
    if kind == "count":
        return _counts(n, rng, tile, budget)
    if kind == "count_pair":
        return np.stack([_counts(n, rng, tile, budget), _counts(n, rng, tile, budget)], axis=1).astype(np.int32)
    if kind == "float":
        return np.full(n, NAN_BITS, np.uint32)
    assert kind == "table_entry" and elem_bytes == 8 and 0 <= epoch < EPOCH_TOP
    e = np.uint64(epoch + 1) + (rng.randint(0, 1 << 62, size=n).astype(np.uint64) % np.uint64(EPOCH_TOP - epoch))
    which = rng.randint(0, 3, size=n)
    v = np.where(which == 0, PROVISIONAL | rng.randint(0, max(int(slots), 1), size=n),          # a claim of a running hop
                 np.where(which == 1, rng.randint(0, max(int(budget) * 4, 1), size=n),           # a final-looking position inside the batch
                          rng.randint(0, 1 << 32, size=n))).astype(np.uint64)                    # anything
    return (e << np.uint64(32)) | v


def next_epoch(K, pool):
    """the table epoch the pool's NEXT batch runs under (batch_generator_kernel / LegionBatchGraph_Launch: kEpochTop - the new serial)"""
    return EPOCH_TOP - (int(K.lib().GPUMemoryPool_GetBatchSerial(pool)) + 1)


def _write(K, stream, jobs):
    """[(device pointer, array)] on `stream`, behind everything it holds and finished before the arrays go away"""
    L = K.lib()
    L.d_stream_sync(stream)
    for ptr, a in jobs:
        assert a.flags["C_CONTIGUOUS"]
        if a.nbytes:
            L.d_copy_async(ptr, a.ctypes.data, a.nbytes, stream)
    L.d_stream_sync(stream)
    K.check()


def poison_pool(K, eng, rng, fill="random", dev=0, pipes=(0,), stream=None, lifetimes=("hop", "batch", "table"), names=None, avoid=(),
                decoy=None, slots=None, tile=TILE_NARROW, cache_slots=1, written=None):
    """Fill every listed buffer of eng.pools[dev] whose lifetime is in `lifetimes` (and whose name is in `names`, when given) with the
    poison of its kind.  Synchronises `stream` before it writes and writes on it.  Returns the names written; `written`: a list that
    receives (name, device pointer, the array written)."""
    L, pool = K.lib(), eng.pools[dev]
    L.SetGPUDevice(dev)
    n_ids = int(L.GPUMemoryPool_NumIds(pool))
    jobs, done, seen = [], [], set()
    for pipe in pipes:
        for b in K.pool_scratch(pool, pipe):
            if b["lifetime"] not in lifetimes or b["lifetime"] == "state" or not b["ptr"] or (names is not None and b["name"] not in names):
                continue
            if (b["name"], b["ptr"]) in seen:
                continue
            seen.add((b["name"], b["ptr"]))
            hop_slots = b["bytes"] // 4 if slots is None else slots
            a = generate(b["kind"], b["bytes"], b["elem_bytes"], rng, fill, limit=cache_slots if b["name"] == "cache_search_buffer" else eng.V, avoid=avoid,
                         slots=max(1, min(int(hop_slots), b["bytes"] // 4)), tile=tile, budget=n_ids // 4, epoch=next_epoch(K, pool), decoy=decoy)
            assert a.nbytes == b["bytes"], (b["name"], a.nbytes, b["bytes"])
            jobs.append((b["ptr"], a))
            done.append(b["name"])
            if written is not None:
                written.append((b["name"], b["ptr"], a))
    _write(K, stream, jobs)
    return done


def poison_outputs(K, eng, rng, fill="random", dev=0, pipe=0, stream=None, avoid=()):
    """The engine's own output buffers of (dev, pipe) -- ids, labels, both COO arrays, the feature / neighbour-sum rows -- under the same
    rules: ids as ids, offsets as positions below num_ids, rows as NAN_BITS.  The counters are not touched: k_seed stores all of them."""
    K.lib().SetGPUDevice(dev)
    o = eng.out[dev][pipe]
    jobs = []
    for key, kind, limit in (("ids", "id", eng.V), ("labels", "id", 64), ("src", "id", eng.num_ids), ("dst", "id", eng.num_ids)):
        jobs.append((o[key].ptr, generate(kind, o[key].nbytes, 4, rng, fill, limit=limit, avoid=avoid if key == "ids" else ())))
    if o["feat"] is not None:
        jobs.append((o["feat"].ptr, generate("float", o["feat"].nbytes, 4, rng, fill)))
    _write(K, stream, jobs)


# ---- the shapes and batches of tests/test_gpu_scratch_poison.py, shared with the CPU test that proves the near-tie cap on them ---------
RULES = ("replace", "distinct", "weighted", "wdistinct", "shared", "wshared")
ENGINE_ARGS = dict(replace=dict(sample="replace"), distinct=dict(sample="distinct"), weighted=dict(sample="weighted"),
                   wdistinct=dict(sample="weighted", weighted_distinct=True), shared=dict(sample="distinct", shared_draws=True),
                   wshared=dict(sample="weighted", weighted_distinct=True, shared_draws=True))
NARROW_SLOTS = 256 * 1024                   # kNarrowSlots
# narrow: every hop runs the 256-slot tile; wide: hop 2 is bounded by 1024 x 16 x 17 = 278 528 slots, the smallest two-hop bound above kNarrowSlots with fan-outs
# on both sides of a power of two
SHAPES = dict(narrow=(64, [5, 4, 3]), wide=(1024, [16, 17]))
assert 64 * 5 * 4 * 3 <= NARROW_SLOTS < 1024 * 16 * 17
EMPTY, LONG = 0, 1                          # drawrulecases' hand-made rows: node 0 has no neighbour, node 1 has 129
# (counter, batch size or None = the pool's, fill): a full batch, one seed (node LONG: list entry 1), a seed of degree 0 (node EMPTY: list
# entry 0; hop 1 finds no edge and every later hop is k_write's n_tiles == 0 path), the full batch again, the short last batch
SEQUENCE = ((0, None, "random"), (1, 1, "ones"), (0, 1, "zero"), (0, None, "random"), (1, None, "ones"))


def seed_list(tile):
    """drawrulecases.seed_list's recipe at this module's batch sizes: the hand-made rows first, B + B / 3 seeds in all"""
    B = SHAPES[tile][0]
    return np.concatenate([np.arange(5), np.random.RandomState(2).randint(0, 3000, size=B + B // 3 - 5)]).astype(np.int32)


def statement(rule, g, tile, alias=None, oracle=None):
    """The rule's statement behind run_batch(ids, lab, counter, batch_size=): the C oracle for the reference's draws when given (else
    seededref's NumPy statement of them), the rule's NumPy statement otherwise.  g: wsharedcases.rule_graph(); alias: the engine's alias
    table (the weighted rule reads it).  A statement of a rule without replacement by weight collects its near ties in .ties."""
    import seededref, sharedref, wdistinctref, weightedref, wsharedref
    B, fan = SHAPES[tile]
    a = (g["indptr"], g["indices"], g["feats"])
    if rule == "replace":
        return oracle.OracleRunner(*a, len(g["indptr"]) - 1, g["feats"].shape[1], B, fan) if oracle is not None else seededref.Statement(*a, B, fan, None)
    if rule == "distinct":
        return seededref.Statement(*a, B, fan, None, "distinct")
    if rule == "weighted":
        return weightedref.Statement(weightedref.Table(g["indptr"], g["indices"], *alias), g["feats"], B, fan)
    if rule == "shared":
        return sharedref.Statement(*a, B, fan)
    return (wdistinctref if rule == "wdistinct" else wsharedref).Statement(g["graph"], g["feats"], B, fan)
