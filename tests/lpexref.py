"""Target-edge exclusion (GPUMemoryPool_SetLpExclude, INTEGRATION.md "Target-edge exclusion") as a NumPy statement, shared by the CPU and
the GPU tests.  A helper module, not collected by pytest.

  the target pairs of a batch of B = 3 k seeds: {ids[i], ids[k + i]}, i < k, both ids >= 0
  edge e < batch_edges:  u = ids[dst_off[e]], v = ids[src_off[e]];  edge_keep[e] = 0 iff {u, v} is a target pair (unordered), else 1
  lp_excluded[h] = zeros among hop h's edges (1 <= h <= H), lp_excluded[0] their sum, the other words of int32[8] are 0
  a batch whose level-0 size is not 3 k keeps every edge

The statement looks every edge up, wherever its offsets lie: that the kernel may skip the edges with an offset >= B is what it proves.
The pair table of the kernels (uint64[cap], cap the smallest power of two >= max(4 k, 64), linear probing from pair_slot) is restated here
too, for the known answers and for the collision case."""
import numpy as np

from distinctref import M32, mix32_scalar

EMPTY = (1 << 64) - 1


def pair_cap(k):
    cap = 64
    while cap < 4 * int(k):
        cap *= 2
    return cap


def pair_slot(lo, hi, cap):
    """mix32(lo ^ mix32(hi)) & (cap - 1), plain Python ints; lo <= hi"""
    return mix32_scalar((int(lo) & M32) ^ mix32_scalar(int(hi) & M32)) & (int(cap) - 1)


def pair_keys(u, v):
    """uint64 [n]: (min << 32) | max"""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    return (np.minimum(u, v).astype(np.uint64) << np.uint64(32)) | np.maximum(u, v).astype(np.uint64)


def targets(ids, k):
    """uint64 [<= k]: the keys of the batch's valid target pairs"""
    a, b = np.asarray(ids[:k], dtype=np.int64), np.asarray(ids[k:2 * k], dtype=np.int64)
    ok = (a >= 0) & (b >= 0)
    return pair_keys(a[ok], b[ok])


def keep(batch, k, H):
    """(edge_keep uint8 [E], lp_excluded int32 [8]) of a batch dict(nc, ec, ids, src_off, dst_off)"""
    nc, ec, ids = np.asarray(batch["nc"]), np.asarray(batch["ec"]), np.asarray(batch["ids"], dtype=np.int64)
    E = int(ec[2 + H])
    out, cnt = np.ones(E, np.uint8), np.zeros(8, np.int32)
    if int(nc[4]) != 3 * k or E == 0:
        return out, cnt
    u, v = ids[np.asarray(batch["dst_off"][:E], dtype=np.int64)], ids[np.asarray(batch["src_off"][:E], dtype=np.int64)]
    hit = (u >= 0) & (v >= 0) & np.isin(pair_keys(np.maximum(u, 0), np.maximum(v, 0)), targets(ids, k))
    out[hit] = 0
    for h in range(1, H + 1):
        lo = 0 if h == 1 else int(ec[2 + h - 1])
        cnt[h] = int(hit[lo:int(ec[2 + h])].sum())
    cnt[0] = int(hit.sum())
    return out, cnt


def hop_census(batch, k, H):
    """per hop h = 1..H: (excluded, kept with both offsets < B, edges with an offset >= B, excluded with an offset >= B)"""
    ec, B = np.asarray(batch["ec"]), 3 * k
    kp, _ = keep(batch, k, H)
    E = len(kp)
    s, d = np.asarray(batch["src_off"][:E]), np.asarray(batch["dst_off"][:E])
    low = (s < B) & (d < B)
    out = []
    for h in range(1, H + 1):
        r = slice(0 if h == 1 else int(ec[2 + h - 1]), int(ec[2 + h]))
        out.append((int((kp[r] == 0).sum()), int(((kp[r] == 1) & low[r]).sum()), int((~low[r]).sum()), int(((kp[r] == 0) & ~low[r]).sum())))
    return out


# ---- the toy graph and its lists -----------------------------------------------------------------------
CORE = 4


def toy_graph(V=300, seed=3, core_links=1, partners=3):
    """A symmetric graph with multi-edges and self-loops: nodes [0, CORE) form a complete core with two self-loops each, one doubled edge
    and core_links edges each to the outside (short rows in which a batch of ONE triple re-finds its pair and its own seeds at every hop);
    the others have `partners` random partners each and are as often a partner (about six entries a row, some doubled, a few self-loops);
    node V - 1 is isolated.  Returns (indptr int64, indices int32, features float32 [V, 4])."""
    rng = np.random.RandomState(seed)
    pairs = [(a, b) for a in range(CORE) for b in range(a + 1, CORE)] + [(0, 1)]
    loops = 2 * list(range(CORE)) + rng.randint(CORE, V - 1, size=V // 12).tolist()
    for a in range(CORE):
        pairs += [(a, int(b)) for b in rng.randint(CORE, V - 1, size=core_links)]
    for a in range(CORE, V - 1):
        for b in rng.randint(CORE, V - 1, size=partners):
            if int(b) != a:
                pairs.append((a, int(b)))
                if rng.rand() < 0.15:
                    pairs.append((a, int(b)))                     # a multi-edge
    src = np.array([p[0] for p in pairs] + [p[1] for p in pairs] + loops, dtype=np.int64)
    dst = np.array([p[1] for p in pairs] + [p[0] for p in pairs] + loops, dtype=np.int64)
    order = np.lexsort((rng.rand(len(src)), src))                 # rows in node order, columns shuffled inside a row
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(src, minlength=V))
    feats = np.random.RandomState(seed + 1).rand(V, 4).astype(np.float32)
    return indptr, dst[order].astype(np.int32), feats


def is_symmetric(indptr, indices):
    V = len(indptr) - 1
    src = np.repeat(np.arange(V, dtype=np.int64), np.diff(indptr))
    a = np.sort(src * V + indices)
    return np.array_equal(a, np.sort(indices.astype(np.int64) * V + src))


def triple_list(indptr, indices, k, batches, seed, core=False):
    """A [src | pos | neg] list of `batches` batches of 3 k: pos is a neighbour of src (src itself for an empty row), neg is uniform --
    core: sources and negatives from the core, so that a batch of one triple has seed-seed edges."""
    rng = np.random.RandomState(seed)
    V = len(indptr) - 1
    n = batches * k
    src = rng.randint(0, CORE, size=n) if core else (rng.permutation(V)[:n] if n <= V else rng.randint(0, V, size=n))
    deg = np.diff(indptr)[src]
    pos = np.where(deg > 0, indices[np.minimum(indptr[src] + (rng.rand(n) * deg).astype(np.int64), len(indices) - 1)], src)
    neg = rng.randint(0, CORE, size=n) if core else rng.randint(0, V, size=n)
    out = np.empty(3 * n, np.int32)
    for b in range(batches):
        r = slice(b * k, (b + 1) * k)
        out[b * 3 * k:(b + 1) * 3 * k] = np.concatenate([src[r], pos[r], neg[r]])
    return out


# ---- the pair table, simulated ---------------------------------------------------------------------------
def build_table(keys, cap):
    """The table after inserting `keys` (uint64) in this order, and every key's chain depth (occupied slots walked before its own)"""
    tab = np.full(cap, EMPTY, dtype=np.uint64)
    depth = {}
    for key in (int(x) for x in keys):
        slot, d = pair_slot(key >> 32, key & M32, cap), 0
        while int(tab[slot]) not in (EMPTY, key):
            slot, d = (slot + 1) & (cap - 1), d + 1
        tab[slot] = key
        depth.setdefault(key, d)
    return tab, depth


def lookup_walk(tab, key):
    """(found, occupied slots walked before the answer) of a lookup"""
    cap, key = len(tab), int(key)
    slot, d = pair_slot(key >> 32, key & M32, cap), 0
    while d < cap:
        t = int(tab[slot])
        if t == key:
            return True, d
        if t == EMPTY:
            return False, d
        slot, d = (slot + 1) & (cap - 1), d + 1
    return False, d


def colliding_pairs(V, cap, slot):
    """every pair lo < hi < V whose first slot is `slot`"""
    return [(lo, hi) for hi in range(V) for lo in range(hi) if pair_slot(lo, hi, cap) == slot]


def collision_case(V=300, k=16, chain=10, seed=0):
    """A batch of k triples, verbatim, on a graph made for it: `chain` target pairs of 2 * chain distinct nodes whose first slot is cap - 3
    (their probe chain wraps past the table's end), the other triples' pairs in first slots [16, 40), and one pair of two seeds of
    DIFFERENT target pairs, no target itself, whose first slot is cap - 3 or cap - 2: its lookup walks the chain to the empty slot behind
    it.  Every pair is an edge of the graph, in both directions; every row has at most 4 entries, so a distinct hop of fan-out >= 4 takes
    them all.  Returns dict(indptr, indices, feats, list, k, cap, pairs, probe)."""
    cap = pair_cap(k)
    head = cap - 3
    rng = np.random.RandomState(seed)
    pool = colliding_pairs(V - 1, cap, head)
    while True:
        rng.shuffle(pool)
        chosen, used = [], set()
        for lo, hi in pool:
            if lo not in used and hi not in used:
                chosen.append((lo, hi))
                used |= {lo, hi}
            if len(chosen) == chain:
                break
        seeds = sorted(used)
        probes = [(a, b) for i, a in enumerate(seeds) for b in seeds[i + 1:] if (a, b) not in chosen and pair_slot(a, b, cap) in (head, head + 1)]
        if len(chosen) == chain and probes:
            break
    fill = []
    for hi in range(V - 1):
        for lo in range(hi):
            if len(fill) < k - chain and lo not in used and hi not in used and 16 <= pair_slot(lo, hi, cap) < 40:
                fill.append((lo, hi))
                used |= {lo, hi}
    pairs = chosen + fill
    assert len(pairs) == k
    outside = [v for v in range(V - 1) if v not in used]
    edges = pairs + [probes[0]] + [(a, outside[i % len(outside)]) for i, a in enumerate(sorted(used))]      # one neighbour that is no seed, for every seed
    src = np.array([e[0] for e in edges] + [e[1] for e in edges], dtype=np.int64)
    dst = np.array([e[1] for e in edges] + [e[0] for e in edges], dtype=np.int64)
    order = np.argsort(src, kind="stable")
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(src, minlength=V))
    L = np.array([p[0] for p in pairs] + [p[1] for p in pairs] + [outside[-1 - i] for i in range(k)], dtype=np.int32)
    return dict(indptr=indptr, indices=dst[order].astype(np.int32), feats=np.random.RandomState(1).rand(V, 4).astype(np.float32), list=L, k=k, cap=cap,
                pairs=pairs, probe=probes[0], head=head, chain=chain)


# ---- the batches of tests/test_gpu_lp_exclude.py, shared with the CPU test that proves they exercise every kind of edge ----------------
# thirds: "replace" / "distinct" = drawn under seed S with that sampler (lp_draw = k), "verbatim" = the list's own thirds, unseeded.  The
# seeds of the k = 1 cases were searched for: one triple must re-find its pair and one of its own seeds at every hop of three batches.
COUNTERS = (0, 1, 2)
FANS = ([5, 4, 3], [5, 4])
CASES = [dict(k=k, fan=fan, thirds=t, S={(1, "replace"): 10, (1, "distinct"): 3}.get((k, t), 1))
         for k in (1, 22, 86) for fan in FANS for t in ("replace", "distinct", "verbatim")]


def case_id(case):
    return "k%d-%s-%s" % (case["k"], "-".join(map(str, case["fan"])), case["thirds"])


_graph = []


def graph():
    if not _graph:
        _graph.append(toy_graph())
    return _graph[0]


def case_list(case, g):
    """(list, labels): three batches of 3 k; k = 1 takes its triples from the core"""
    L = triple_list(g[0], g[1], case["k"], len(COUNTERS), seed=case["k"], core=case["k"] == 1)
    return L, (np.arange(len(L)) % 1000).astype(np.int32)


def engine_args(case):
    """what Engine.run_batch takes for the case, the mode itself aside"""
    if case["thirds"] == "verbatim":
        return dict(sample="replace")
    return dict(sample=case["thirds"], seed=case["S"], lp_draw=case["k"])


def statement(case, g):
    """(the sampler's statement of the case, list, labels)"""
    import lpref
    import seededref
    B = 3 * case["k"]
    L, Lab = case_list(case, g)
    if case["thirds"] == "verbatim":
        return seededref.Statement(g[0], g[1], g[2], B, case["fan"], None, "replace", shuffle=False), L, Lab
    return lpref.Statement(g[0], g[1], g[2], B, case["fan"], case["S"], case["thirds"]), L, Lab
