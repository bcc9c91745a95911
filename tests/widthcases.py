"""Inputs of tests/test_gpu_gather_widths.py and tests/test_gpu_exchange_plan.py -- the row gathers at every row width, across wave and
row edges -- with what proves on the CPU that they reach what they are meant to reach (tests/test_gather_widths_cpu.py): one small graph,
a feature table whose every element names its own (node, column), a comparison that says which element arrived instead, the table of
widths, the lane arithmetic of the flat work space as plain integers, and the cached configurations with the floors their batches have
to meet.  Pure NumPy over the oracle's batches; a helper module, not collected by pytest."""
import collections
import functools

import numpy as np

V, B, FAN = 600, 24, [3, 2]
N_SEEDS = 2 * B + 8                # batch 0, the middle batch 1 and the short last batch 2 (8 seeds)
BATCHES = (0, 1, 2)
ROWS_MAX = B * (1 + 3 + 6)         # 240 rows: under est_rows' 1024-row floor (csrc/launch.h), so every grid covers its batch at once
PRESC_STEPS = 2                    # pre-sampling batches per member in front of a cache build
POISON = 0xFFFFFFFF                # what d_memset_async(.., 0xFF, ..) leaves in every word
MAX_DEVICE = 8                     # LEGION_MAX_DEVICE (include/legion_amd.h): legion_exchange_plan's counts are int32[2 * MAX_DEVICE]
WAVE, BLOCK = 64, 256


# ---- the graph --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph():
    """degrees 0..12 from a fixed RandomState, one hub of 60 neighbours that a tenth of all edges point at, a few -1 holes, multi-edges
    (neighbours are drawn with repetition); labels 0..6"""
    rng = np.random.RandomState(20260)
    deg = rng.randint(0, 13, size=V)
    hub = 17
    deg[hub] = 60
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    nbr = np.where(rng.rand(E) < 0.1, hub, rng.randint(0, V, size=E))
    nbr[rng.rand(E) < 0.02] = -1
    labels = rng.randint(0, 7, size=V).astype(np.int32)
    return dict(indptr=indptr, indices=nbr.astype(np.int32), labels=labels, hub=hub)


def seed_lists(G):
    """one training list per clique member: N_SEEDS distinct nodes with at least one neighbour, the hub among member 0's first batch"""
    g = graph()
    rng = np.random.RandomState(31 + G)
    pool = rng.permutation(np.nonzero(np.diff(g["indptr"]) > 0)[0])
    parts = [pool[k * N_SEEDS:(k + 1) * N_SEEDS].astype(np.int32) for k in range(G)]
    if g["hub"] not in parts[0][:B]:
        parts[0][3] = g["hub"]
    return parts


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
WORD0, COLS = 0x3F000000, 2048     # word = WORD0 + v * COLS + c: floats in [0.5, 1), pairwise distinct for v < 1024, c < 2048


@functools.lru_cache(maxsize=None)
def table(F):
    assert V <= 1024 and F <= COLS
    w = (WORD0 + np.arange(V, dtype=np.uint32)[:, None] * COLS + np.arange(F, dtype=np.uint32)[None, :]).astype(np.uint32)
    t = np.ascontiguousarray(w).view(np.float32)
    t.setflags(write=False)
    return t


def decode(word):
    """(v, c) of a table word, None for anything else"""
    d = int(word) - WORD0
    return (d // COLS, d % COLS) if 0 <= d < 1024 * COLS else None


def expected_rows(F, ids):
    """table(F)[ids], a row of +0.0 for an id < 0"""
    ids = np.asarray(ids, dtype=np.int64)
    out = table(F)[np.where(ids >= 0, ids, 0)].copy()
    out[ids < 0] = 0
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint32 else a.view(np.uint32)


def _says(word, with_chunk):
    vc = decode(word)
    if vc is None:
        return "0x%08X, not a table word" % int(word) + (" (poison)" if int(word) == POISON else "")
    return "node %d's column %d%s" % (vc[0], vc[1], " (chunk %d)" % (vc[1] // 4) if with_chunk else "")


def assert_rows(name, got, want):
    """`got` against `want` as uint32 [rows, F].  A failure names the first wrong (row, column), what was expected there, which table
    element arrived instead, and how many 16-byte chunks differ."""
    a, b = bits(got), bits(want)
    assert a.shape == b.shape and a.ndim == 2, "%s: shape %s, expected %s" % (name, a.shape, b.shape)
    if np.array_equal(a, b):
        return
    F = a.shape[1]
    bad = a != b
    r, c = (int(x) for x in np.argwhere(bad)[0])
    chunks = int(np.add.reduceat(bad, np.arange(0, F, 4), axis=1).astype(bool).sum())
    raise AssertionError("%s: row %d column %d (chunk %d) holds %s; expected %s; %d words in %d 16-byte chunks of %d rows differ" % (
        name, r, c, c // 4, _says(a[r, c], True), _says(b[r, c], False) if b[r, c] else "+0.0", int(bad.sum()), chunks, int(bad.any(axis=1).sum())))


# ---- the widths ---------------------------------------------------------------------------------------------------------------------------
Width = collections.namedtuple("Width", "F path C forced reason")


def path_of(F, aligned=True):
    """rows_are_vec4 (csrc/launch.h): the 16-byte path when F % 4 == 0 and both the table and the destination are 16-byte aligned"""
    return "vec" if F % 4 == 0 and aligned else "scalar"


def chunks_per_row(F, aligned=True):
    return F // 4 if path_of(F, aligned) == "vec" else F


def row_pitch(F):
    """legion_row_pitch restated: the next multiple of 32 floats (a whole number of 128-byte lines)"""
    return (F + 31) // 32 * 32


WIDTHS = [
    Width(4, "vec", 1, False, "C = 1: ch is always 0, 64 rows per wave"),
    Width(8, "vec", 2, False, "C = 2"),
    Width(12, "vec", 3, False, "C = 3: the smallest C that does not divide a wave"),
    Width(100, "vec", 25, False, "a workload's width: pitched replica and shards"),
    Width(128, "vec", 32, False, "a workload's width: two rows per wave"),
    Width(252, "vec", 63, False, "one chunk under a wave"),
    Width(256, "vec", 64, False, "a row is exactly a wave"),
    Width(260, "vec", 65, False, "one chunk over a wave"),
    Width(516, "vec", 129, False, "a row spans three waves"),
    Width(1028, "vec", 257, False, "a row is wider than a 256-lane workgroup"),
    Width(1, "scalar", 1, False, "C = 1"),
    Width(2, "scalar", 2, False, "C = 2"),
    Width(3, "scalar", 3, False, "C = 3"),
    Width(7, "scalar", 7, False, "the suite's scalar width"),
    Width(63, "scalar", 63, False, "one float under a wave"),
    Width(65, "scalar", 65, False, "one float over a wave"),
    Width(127, "scalar", 127, False, "one float under two waves"),
    Width(129, "scalar", 129, False, "one float over two waves: a row spans three"),
    Width(257, "scalar", 257, False, "wider than a workgroup"),
    Width(64, "scalar", 64, True, "destination 4 bytes off alignment: the scalar path at a row of exactly a wave"),
    Width(256, "scalar", 256, True, "destination 4 bytes off alignment: one row per workgroup"),
]
ALIGNED = [w for w in WIDTHS if not w.forced]
FORCED = [w for w in WIDTHS if w.forced]


def width_id(w):
    return "F%d-%s%s-C%d" % (w.F, "forced-" if w.forced else "", w.path, w.C)


# ---- the flat work space ------------------------------------------------------------------------------------------------------------------
def work_space_facts(rows, C):
    """Item q = r * C + ch of a launch over `rows` rows of C chunks, 64 consecutive items per wave.  Counts of: rows that begin in one wave
    and end in another; waves whose first item is not chunk 0 of its row (k_gather_lookup's `first < 0`: the lead lane is clamped to lane
    0); waves that hold more than one row's lead lane; rows that span three or more waves."""
    rows, C = int(rows), int(C)
    total = rows * C
    first = np.arange(rows, dtype=np.int64) * C
    w0, w1 = first // WAVE, (first + C - 1) // WAVE
    base = np.arange(0, total, WAVE, dtype=np.int64)
    last = np.minimum(base + WAVE, total) - 1
    return dict(straddling_rows=int((w0 != w1).sum()), clamped_waves=int((base % C != 0).sum()),
                multi_lead_waves=int((base // C != last // C).sum()), three_wave_rows=int((w1 - w0 >= 2).sum()))


def claimed_facts(w):
    """the facts the reason column of WIDTHS claims for a width: each must be non-zero for every batch used"""
    out = []
    if WAVE % w.C:
        out.append("straddling_rows")
    if w.C > WAVE:
        out.append("clamped_waves")
    if w.C >= 129:
        out.append("three_wave_rows")
    if w.C < WAVE:
        out.append("multi_lead_waves")
    return out


# ---- the reference's batches ----------------------------------------------------------------------------------------------------------------
def plain_runner(oracle, F):
    g = graph()
    return oracle.OracleRunner(g["indptr"], g["indices"], table(F), V, F, B, FAN)


def plain_batches(oracle, F):
    """{counter: the oracle's batch} of member 0's list, uncached"""
    g, orc, seeds = graph(), plain_runner(oracle, F), seed_lists(1)[0]
    return {it: orc.run_batch(seeds, g["labels"][seeds], it) for it in BATCHES}


# Forced node capacities per clique size (rows per member), chosen on the CPU until every batch of BATCHES on every member meets FLOOR:
# tests/test_gather_widths_cpu.py asserts it, the GPU tests assert it again from the same helper.
CAPACITY = {1: 150, 2: 110, 4: 70}
FLOOR = 10                         # hits in the member's own shard, misses, and rows in every peer's shard, per batch
PAIR_FLOOR = 3                     # Kg = 4: rows of every (requester, owner) pair in at least one of PLAN_BATCHES
PLAN_BATCHES = (0, 1)
PLAN_WIDTHS = (7, 100, 260)        # scalar, pitched vec, C = 65
CHUNK_ROWS = 16                    # rows per shard chunk the tests ask for: a capacity of 70 is five chunks


def shard_chunk_bytes(F):
    """$LEGION_SHARD_CHUNK_BYTES for CHUNK_ROWS rows per chunk at this width (chunk_shift, csrc/chunks.cpp: the largest power of two of
    pitched rows that fits)"""
    return row_pitch(F) * 4 * CHUNK_ROWS


def clique_oracles(oracle, F, Kg):
    """The oracle's side of a Kg-member clique with CAPACITY[Kg] rows per member: PRESC_STEPS pre-sampling batches per member, the
    ranking, the id -> slot map and the shards' rows.  Returns (runners, seed lists)."""
    g, parts = graph(), seed_lists(Kg)
    orcs = [oracle.OracleRunner(g["indptr"], g["indices"], table(F), V, F, B, FAN, partition_count=Kg) for _ in range(Kg)]
    for d in range(Kg):
        for it in range(PRESC_STEPS):
            orcs[d].run_batch(parts[d], g["labels"][parts[d]], it, is_presc=True)
    _, QF = oracle.candidate_selection([o.node_access_time for o in orcs], V)
    for o in orcs:
        o.set_feature_cache(QF, CAPACITY[Kg], Kg)
    return orcs, parts


def owners_of(orc, ids, Kg):
    """(slot, owner) per batch row: the oracle's cache slot (< 0: a miss or a -1 id) and the clique member whose shard holds it (-1: none)"""
    ids = np.asarray(ids, dtype=np.int64)
    slot = np.where(ids >= 0, orc.node_map[np.where(ids >= 0, ids, 0)], -1).astype(np.int64)
    return slot, np.where(slot >= 0, slot // CAPACITY[Kg], -1)


def cache_counts(orc, ids, me, Kg):
    """dict(own, miss, peers=[rows in member j's shard, 0 for me], hits, rows) of a batch on member `me`"""
    ids = np.asarray(ids)
    slot, owner = owners_of(orc, ids, Kg)
    peers = [int((owner == j).sum()) if j != me else 0 for j in range(Kg)]
    return dict(own=int((owner == me).sum()), miss=int(((slot < 0) & (ids >= 0)).sum()), peers=peers, hits=int((slot >= 0).sum()), rows=len(ids))


def assert_floors(orc, ids, me, Kg, what=""):
    c = cache_counts(orc, ids, me, Kg)
    assert c["own"] >= FLOOR and c["miss"] >= FLOOR and all(n >= FLOOR for j, n in enumerate(c["peers"]) if j != me), (what, me, Kg, c)
    return c


def quiet_seeds(orc):
    """a validation list whose batch asks no peer for anything: nodes without neighbours that the clique does not cache (the batch is its
    seeds, every one a miss)"""
    g = graph()
    quiet = np.nonzero((np.diff(g["indptr"]) == 0) & (orc.node_map < 0))[0].astype(np.int32)
    return quiet[:B]


def expected_plan(orc, ids, me, Kg):
    """legion_exchange_plan's contract over a batch's ids: (counts[Kg], per owner the sorted (req_row, req_dst) pairs)"""
    slot, owner = owners_of(orc, ids, Kg)
    cap = CAPACITY[Kg]
    counts, pairs = [], []
    for j in range(Kg):
        r = np.nonzero(owner == j)[0] if j != me else np.zeros(0, np.int64)
        counts.append(len(r))
        pairs.append(sorted(zip((slot[r] - j * cap).tolist(), r.tolist())))
    return counts, pairs
