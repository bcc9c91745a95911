"""Inputs of tests/test_gpu_distinct_cross.py -- the distinct-draw sampler mode across both sampler tiles, caches and mode switches -- with
what proves on the CPU that they reach what they are meant to reach (tests/test_distinct_cases_cpu.py): graph and case builders, the tile a
hop runs, the coverage of a batch counted from the statement's batch alone, and the mutant draws that a good input must tell from
tests/distinctref.py.  Pure NumPy; a helper module, not collected by pytest."""
import numpy as np

import distinctref as D

NARROW_SLOTS = 256 * 1024      # kNarrowSlots (csrc/internal.h): a hop whose static slot bound is at most this runs the 256-slot tile
TILE_NARROW, TILE_WIDE = 256, 1024


class Statement:
    """tests/distinctref.py behind the oracle runner's run_batch signature (harness.replay_served)."""

    def __init__(self, indptr, indices, feats, B, fan):
        self.a, self.B, self.fan = (indptr, indices, feats), B, list(fan)

    def run_batch(self, ids, lab, counter, mode=0, batch_size=None):
        return D.run_batch(*self.a, ids, lab, self.B if batch_size is None else batch_size, counter, self.fan)


def random_graph(seed, V, max_deg=40, hubs=5, hub_deg=300, holes=False, simple=False):
    """degrees 0..max_deg around the fan-outs of the tests (rows with d <= f and d > f) and a few hubs; simple: no multi-edges"""
    rng = np.random.RandomState(seed)
    deg = rng.randint(0, max_deg + 1, size=V)
    deg[rng.randint(0, V, hubs)] = min(hub_deg, V)
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    if simple:
        indices = np.concatenate([rng.permutation(V)[:d] for d in deg]).astype(np.int32)
    else:
        indices = rng.randint(-1 if holes else 0, V, size=int(indptr[-1])).astype(np.int32)
    labels = rng.randint(0, 9, size=V).astype(np.int32)
    return indptr, indices, labels


# ---- tiles and coverage ----------------------------------------------------------------------------
def hop_bounds(B, fan):
    out, cur = [], int(B)
    for f in fan:
        cur *= int(f)
        out.append(cur)
    return out


def hop_tiles(B, fan):
    """the tile every hop's three passes run: from the hop's STATIC slot bound B * f1 * .. * fh, whatever the batch holds (sampler_tile_of)"""
    return [TILE_NARROW if b <= NARROW_SLOTS else TILE_WIDE for b in hop_bounds(B, fan)]


def row_degrees(inp, indptr):
    """the int32 degree the sampler sees for every entry of a hop's input list; -1 for a -1 entry"""
    inp, indptr = np.asarray(inp, dtype=np.int64), np.asarray(indptr)
    s = np.where(inp >= 0, inp, 0)
    return np.where(inp >= 0, (indptr[s + 1] - indptr[s]).astype(np.int32).astype(np.int64), -1)


def crossing(n_rows, f, edge):
    """bool [n_rows]: the f slots of row i, [i f, i f + f), lie on both sides of a multiple of `edge`"""
    first = np.arange(n_rows, dtype=np.int64) * f
    return first // edge != (first + f - 1) // edge


def coverage(want, indptr, fan, B):
    """Per hop of a distinctref.run_batch result: slots and tile; rows with d > f, d == f, d == f + 1, d <= 0; holes drawn (slots whose
    draw met a -1 neighbour); rows with d > f whose slots cross an edge of the hop's tile; rows with d > f that cross a 64-lane edge."""
    tiles, out = hop_tiles(B, fan), []
    for h, f in enumerate(fan):
        inp, cnt = want["draw_counts"][h]
        deg = row_degrees(inp, indptr)
        big = deg > f
        out.append(dict(hop=h + 1, f=int(f), rows=len(inp), slots=len(inp) * int(f), tile=tiles[h], big=int(big.sum()), eq_f=int((deg == f).sum()),
                        eq_f1=int((deg == f + 1).sum()), none=int((deg <= 0).sum()), small=int(((deg > 0) & (deg <= f)).sum()),
                        holes=int(np.minimum(deg.clip(0), f).sum() - np.asarray(cnt).sum()),
                        big_cross_tile=int((big & crossing(len(inp), f, tiles[h])).sum()), big_cross_wave=int((big & crossing(len(inp), f, 64)).sum())))
    return out


# ---- the mutants: subtly wrong samplers as draw functions of distinctref.run_batch --------------------
def floyd(keyrows, hop, deg, f, use_hop=True, floyd_above=None, raw_compare=False, restart=None):
    """distinctref.positions with the places a kernel can go wrong as switches (all off: the statement, held to it by the CPU tests).
    keyrows: what enters the row key in place of the row's index; use_hop=False: the hop does not; floyd_above: rows of d > floyd_above
    run Floyd's algorithm, the others take their first min(d, f) neighbours (the statement: f); raw_compare: a pick is looked for among the hashes u[0..t) as int32 instead of the
    picks; restart[m] = c: pick t >= c is looked for among the picks [c, t) only."""
    keyrows, deg = np.asarray(keyrows, dtype=np.int64), np.asarray(deg, dtype=np.int64)
    hop = np.broadcast_to(np.asarray(hop, dtype=np.int64), keyrows.shape)
    f = int(f)
    j = np.arange(f, dtype=np.int64)
    out = np.where(j[None, :] < deg[:, None], j[None, :], -1)
    big = np.nonzero(deg > (f if floyd_above is None else floyd_above))[0]
    if len(big) == 0:
        return out
    d = deg[big]
    K = D.mix32(((keyrows[big] + (D.GOLDEN * hop[big] if use_hop else 0)) & D.M32).astype(np.uint32))
    pick, raw = np.empty((len(big), f), np.int64), np.empty((len(big), f), np.int64)
    for t in range(f):
        J = d - f + t
        u = D.mix32(K ^ np.uint32((D.STEP * (t + 1)) & D.M32))
        r = ((u.astype(np.uint64) * (J + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        eq = (raw if raw_compare else pick)[:, :t] == r[:, None]
        if restart is not None:
            c = np.asarray(restart, dtype=np.int64)[big]
            eq &= j[None, :t] >= np.where(t >= c, c, 0)[:, None]
        pick[:, t] = np.where(eq.any(axis=1), J, r)
        raw[:, t] = u.view(np.int32)
    out[big] = pick
    return out


def _tile_of_hop(tiles, only, hop):
    """the tile of hop `hop` if the mutant lives in that instantiation (only = None: in both), else None: the hop runs the statement"""
    t = tiles[int(np.asarray(hop).reshape(-1)[0]) - 1]
    return t if only in (None, t) else None


def mutant_key_in_tile(tiles, only=None):
    """1. the row key is taken from the row's index inside its tile (r = i - i0) instead of the hop's input list; a row on a tile edge is
    computed by both tiles, each with its own r, and every slot reads the picks of the tile it lies in"""
    def draw(rows, hop, deg, f):
        T = _tile_of_hop(tiles, only, hop)
        if T is None:
            return D.positions(rows, hop, deg, f)
        rows = np.asarray(rows, dtype=np.int64)
        first = rows * f
        tile_a, tile_b = first // T, (first + f - 1) // T
        pa = floyd(rows - (tile_a * T) // f, hop, deg, f)
        pb = floyd(rows - (tile_b * T) // f, hop, deg, f)
        slot_tile = (first[:, None] + np.arange(f)[None, :]) // T
        return np.where(slot_tile == tile_a[:, None], pa, pb)
    return draw


def mutant_restart_at_edge(tiles, only=None):
    """2. Floyd restarts at a tile edge: the slots of a row behind the edge compare only with picks behind it"""
    def draw(rows, hop, deg, f):
        T = _tile_of_hop(tiles, only, hop)
        if T is None:
            return D.positions(rows, hop, deg, f)
        rows = np.asarray(rows, dtype=np.int64)
        first = rows * f
        edge = (first // T + 1) * T                         # the first slot of the next tile
        return floyd(rows, hop, deg, f, restart=np.where(edge < first + f, edge - first, f))
    return draw


def mutant_take_all_below_f(rows, hop, deg, f):
    """3. take-all only for d < f: a row of d == f runs Floyd.  An EQUIVALENT mutant: at d == f pick t is drawn from [0, t] and replaced by
    J = t when it is among the picks before it, so by induction pick t = t -- Floyd's algorithm at d == f IS take-all in CSR order, and no
    input tells the two apart (tests/test_distinct_cases_cpu.py proves it over every key).  The boundary that can be told is the next one:"""
    return floyd(rows, hop, deg, f, floyd_above=f - 1)


def mutant_take_all_up_to_f1(rows, hop, deg, f):
    """3b. take-all up to d == f + 1: such a row takes its first f neighbours and never its last"""
    return floyd(rows, hop, deg, f, floyd_above=f + 1)


def mutant_raw_compare(rows, hop, deg, f):
    """4. picks are compared with the unresolved hashes instead of the resolved picks: a repeated position is not replaced"""
    return floyd(rows, hop, deg, f, raw_compare=True)


def mutant_no_hop(rows, hop, deg, f):
    """5. the hop is left out of the key"""
    return floyd(rows, hop, deg, f, use_hop=False)


MUTANTS = ("key in tile, 256", "key in tile, 1024", "restart at edge, 256", "restart at edge, 1024", "take-all below f", "take-all up to f + 1",
           "raw compare", "no hop in key")
EQUIVALENT = ("take-all below f",)        # mutants that no input can tell from the statement (see mutant_take_all_below_f)


def mutant_draw(name, B, fan):
    """the draw function of a mutant of MUTANTS for a batch of B seeds and these fan-outs (the tiled ones need every hop's tile)"""
    tiles = hop_tiles(B, fan)
    if name.startswith("key in tile"):
        return mutant_key_in_tile(tiles, int(name.split(", ")[1]))
    if name.startswith("restart at edge"):
        return mutant_restart_at_edge(tiles, int(name.split(", ")[1]))
    return {"take-all below f": mutant_take_all_below_f, "take-all up to f + 1": mutant_take_all_up_to_f1, "raw compare": mutant_raw_compare, "no hop in key": mutant_no_hop}[name]


# ---- A: the tile switch --------------------------------------------------------------------------------
def switch_graph(seed=4242, V=60000, F=8):
    """tests/test_gpu_narrow_hops.py's recipe: geometric degrees (mean 24) with hubs of 50-400 neighbours, half of all edges pointing at a
    hub, isolated nodes and -1 entries"""
    rng = np.random.RandomState(seed)
    deg = rng.geometric(0.04, size=V) - 1
    hubs = rng.randint(0, V, size=V // 100)
    deg[hubs] = rng.randint(50, 400, size=len(hubs))
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    nbr = np.where(rng.rand(E) < 0.5, rng.choice(hubs, size=E), rng.randint(0, V, size=E))
    nbr[rng.rand(E) < 0.02] = -1
    feats = rng.rand(V, F).astype(np.float32)
    labels = rng.randint(0, 7, size=V).astype(np.int32)
    return dict(V=V, F=F, indptr=indptr, indices=nbr.astype(np.int32), feats=feats, labels=labels)


# (batch, fan-outs, the tile of every hop, the hops (1-based) that must hold >= 50 rows of d > f across an edge of their own tile)
SWITCH_CASES = [
    (10485, [25], [256], [1]),                  # 262 125 slots: the last bound before the switch
    (10486, [25], [1024], [1]),                 # 262 150
    (4161, [63], [256], [1]),                   # 262 143
    (4162, [63], [1024], [1]),                  # 262 206: a row covers almost a whole wave; the largest pick staging
    (87381, [3], [256], [1]),                   # 262 143: rows of three slots
    (87382, [3], [1024], [1]),                  # 262 146
    (1049, [25, 10], [256, 1024], [1, 2]),      # hop 2: 262 250 -- a narrow hop feeding a wide one
    (8000, [25, 3, 2], [256, 1024, 1024], [1, 2]),   # the headline's hop 1, then wide hops (f = 2 divides the tile: no row crosses)
    (4096, [64], [256], []),                    # the maximal fan-out on either side of the switch: 64 divides both tiles, by design
    (4097, [64], [1024], []),
]
SWITCH_BATCHES = (0, 1, 2, 0)                   # two full batches, the short last one, and the first again


def switch_seeds(g, B, fan):
    """2 B + B / 3 seeds drawn with repetition, half of them among the nodes of degree > f1 and one in twenty among those of degree f1 or
    f1 + 1: the rows the distinct mode is about fill hop 1 whatever the fan-out, and the boundary degrees occur in every batch"""
    rng = np.random.RandomState(B + len(fan))
    deg, f = np.diff(g["indptr"]), int(fan[0])
    n = 2 * B + B // 3
    big, edge = np.nonzero(deg > f)[0], np.nonzero((deg == f) | (deg == f + 1))[0]
    u = rng.rand(n)
    seeds = np.where(u < 0.5, rng.choice(big, size=n), np.where(u < 0.55, rng.choice(edge, size=n), rng.randint(0, g["V"], size=n)))
    return seeds.astype(np.int32)


# ---- B: the cached clique at the smallest shape with wide hops ---------------------------------------------
CLIQUE_B, CLIQUE_FAN, CLIQUE_G = 1049, [25, 10], 2          # hop 2: 262 250 slots, the wide tile


def clique_case():
    """the switch recipe under another seed, and one seed list per logical GPU: two full batches and a short one each, without repetition"""
    g = switch_graph(seed=777)
    rng = np.random.RandomState(778)
    perm = rng.permutation(g["V"])
    n = 2 * CLIQUE_B + CLIQUE_B // 3
    g["parts"] = [perm[k * n:(k + 1) * n].astype(np.int32) for k in range(CLIQUE_G)]
    return g


# ---- C: the degree ladder --------------------------------------------------------------------------------
LADDER_F = (1, 2, 25, 63, 64)
LADDER_HUB = (1 << 20) + 3


def ladder_degrees(f):
    return [0, 1, f - 1, f, f + 1, f + 2, 2 * f, 255, 256, 257, 65535, 65536, 65537, LADDER_HUB]


def ladder_graph(f):
    """A simple graph (no multi-edges, no holes, F = 1): node k < 14 has degree ladder_degrees(f)[k]; nodes 14..20 have two neighbours each,
    the ladder nodes 2 k and 2 k + 1 in that order; every other node has none.  H = 1: the ladder nodes are the seeds.  H = 2 with fan-outs
    {2, f}: nodes 14..20 are, and hop 2's input list is the ladder in order."""
    rng = np.random.RandomState(1000 + f)
    want = ladder_degrees(f)
    V = LADDER_HUB + 64
    n = len(want)
    deg = np.zeros(V, np.int64)
    deg[:n] = want
    deg[n:n + n // 2] = 2
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    rows = [rng.permutation(V)[:d] for d in want]   # d distinct ids in no order
    rows += [np.array([2 * k, 2 * k + 1]) for k in range(n // 2)]
    indices = np.concatenate(rows).astype(np.int32)
    feats = rng.rand(V, 1).astype(np.float32)
    labels = (np.arange(V) % 5).astype(np.int32)
    return dict(V=V, F=1, f=f, indptr=indptr, indices=indices, feats=feats, labels=labels, want=want,
                seeds1=np.arange(n, dtype=np.int32), seeds2=np.arange(n, n + n // 2, dtype=np.int32))


# ---- D: randomised configurations ----------------------------------------------------------------------------
HAND_OFFS = dict(default={}, plain=dict(agg_last_hop=True), norm=dict(agg_last_hop=True, agg_norm="both"))
LAST_FANS = (1, 2, 7, 8, 9, 25, 40, 64)
# walked once around from any start, under any renaming of the hand-offs: all six (sampling, hand-off) states, replace -> distinct and
# distinct -> replace with the hand-off kept (0 -> 1, 3 -> 4) and with the hand-off changed (2 -> 3, 4 -> 5; 1 -> 2, 5 -> 0)
STATE_CYCLE = (("replace", 0), ("distinct", 0), ("replace", 1), ("distinct", 2), ("replace", 2), ("distinct", 1))


def _draw_config(rng):
    V = int(rng.choice([33, 200, 1500, 6000]))
    F = int(rng.choice([1, 3, 4, 8, 36, 100]))
    deg = rng.geometric(0.25, size=V) - 1                  # tests/test_gpu_agg_adversarial.py's recipe: isolated nodes, hubs, skewed
    hubs = rng.randint(0, V, size=max(1, V // 100))        # neighbours, -1 entries, self loops, repeated seeds
    deg[hubs] = rng.randint(50, 400, size=len(hubs))
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    nbr = np.where(rng.rand(E) < 0.5, rng.choice(hubs, size=E), rng.randint(0, V, size=E))
    nbr[rng.rand(E) < 0.02] = -1
    hops = int(rng.randint(1, 5))
    fan = [int(rng.randint(1, 12)) for _ in range(hops - 1)] + [int(rng.choice(LAST_FANS))]
    width = int(np.prod(fan[:-1]))                         # the NumPy statements are kept to a few thousand last-hop rows
    n_seeds = int(rng.randint(5, max(6, min(V, 900))))
    B = int(rng.randint(2, max(2, min(n_seeds - 1, 4000 // width)) + 1))
    if n_seeds % B == 0:
        n_seeds -= 1                                       # the last batch is short
    seeds = rng.randint(0, V, size=n_seeds).astype(np.int32)
    cfg = dict(V=V, F=F, fan=fan, B=B, n_seeds=n_seeds, pitched=bool(rng.randint(2)), host_table=bool(rng.randint(2)), host_csr=bool(rng.randint(2)),
               pipeline_depth=int(rng.randint(1, 3)))
    g = dict(indptr=indptr, indices=nbr.astype(np.int32), labels=rng.randint(0, 7, size=V).astype(np.int32), seeds=seeds,
             table=rng.standard_normal((V, F)).astype(np.float32))
    return cfg, g


def nontrivial_hops(cfg, g, counter=0):
    """the hops of a batch where the distinct mode is neither all Floyd nor all take-all: >= 20 % of the hop's input rows at d > f and
    >= 5 % at 0 < d <= f"""
    want = D.run_batch(g["indptr"], g["indices"], g["table"], g["seeds"], g["labels"][g["seeds"]], cfg["B"], counter, cfg["fan"])
    return [c["hop"] for c in coverage(want, g["indptr"], cfg["fan"], cfg["B"]) if c["rows"] and c["big"] >= 0.2 * c["rows"] and c["small"] >= 0.05 * c["rows"]]


def random_config(seed):
    """seed -> (configuration, graph + table, the sequence of steps).  A drawn configuration whose batch 0 has no non-trivial hop is drawn
    again (cfg["attempt"] counts).  A step is a run_batch (sample, hand_off, counter, pipe, per_level, plan) or the replay of the batch
    graph recorded in `sample` mode before the sequence (replay=True: counter only), placed directly behind a run_batch of the other mode."""
    attempt = 0
    while True:
        rng = np.random.RandomState(7000 + seed + 1000 * attempt)
        cfg, g = _draw_config(rng)
        if nontrivial_hops(cfg, g):
            break
        attempt += 1
    cfg.update(seed=seed, attempt=attempt)
    n_batches = (cfg["n_seeds"] + cfg["B"] - 1) // cfg["B"]
    names = [list(HAND_OFFS)[k] for k in rng.permutation(3)]
    start = int(rng.randint(len(STATE_CYCLE)))
    walk = [STATE_CYCLE[(start + i) % len(STATE_CYCLE)] for i in range(len(STATE_CYCLE) + 1)]
    seq = [dict(sample=s, hand_off=names[m], counter=int(rng.randint(n_batches))) for s, m in walk]
    # the short last batch, then batch 0 in the same state on the same pipe: that pipe's launch-size feedback is smaller than the batch
    s, m = STATE_CYCLE[int(rng.randint(len(STATE_CYCLE)))]
    pipe = int(rng.randint(cfg["pipeline_depth"]))
    seq += [dict(sample=s, hand_off=names[m], counter=n_batches - 1, pipe=pipe), dict(sample=s, hand_off=names[m], counter=0, pipe=pipe)]
    for st in seq:
        st.setdefault("pipe", int(rng.randint(cfg["pipeline_depth"])))
        st.update(per_level=bool(rng.randint(2)), plan=bool(rng.randint(2)))
    cfg["graphs"] = {s: dict(pipe=int(rng.randint(cfg["pipeline_depth"])), per_level=bool(rng.randint(2))) for s in ("replace", "distinct")}
    # two replays per recorded graph, each directly behind a run_batch of the other sampling mode (inside the walk: the closing pair stays adjacent)
    after = {}
    for s in ("replace", "distinct"):
        other = [i for i in range(len(walk)) if seq[i]["sample"] != s and i not in after]
        for i in rng.choice(other, size=2, replace=False):
            after[int(i)] = dict(replay=True, sample=s, counter=int(rng.randint(n_batches)))
    out = []
    for i, st in enumerate(seq):
        out.append(st)
        if i in after:
            out.append(after[i])
    return cfg, g, out


def expected_sums(want, fan, norm):
    """The sums of an aggregated hand-off over the statement's batch `want`, in np.float32 and edge order: tests/aggref.py's statement (norm:
    tests/gcnref.py's) with the draws of a run COUNTED FROM THE BATCH (draw_counts) -- aggref recounts them from the graph, and where the graph
    has holes by recomputing the default mode's draws, which a distinct batch did not make.  On graphs without holes the three agree bit for
    bit (tests/test_distinct_cases_cpu.py).  Returns (n_in, N, S, d): d = the out-degrees inside block 1 (norm) or None."""
    H, f = len(fan), int(fan[-1])
    nc, ec = want["nc"], want["ec"]
    n, n_in = int(nc[5 + 2 * H]), int(nc[3 + 2 * H])
    cnt = np.asarray(want["draw_counts"][H - 1][1], dtype=np.int64)
    N = len(cnt)
    e0, e1 = (0 if H == 1 else int(ec[1 + H])), int(ec[2 + H])
    src = np.asarray(want["src_off"][e0:e1], dtype=np.int64)
    assert int(cnt.sum()) == e1 - e0
    x = np.asarray(want["features"], dtype=np.float32)
    d = w = None
    if norm:
        d = np.bincount(np.asarray(want["src_off"][:e1], dtype=np.int64), minlength=n).astype(np.int32)
        w = np.float32(1) / np.sqrt(d.clip(1).astype(np.float32))
    start = np.cumsum(cnt) - cnt
    S = np.zeros((N, x.shape[1]), np.float32)
    for j in range(f):
        m = cnt > j
        if m.any():
            p = src[start[m] + j]
            S[m] = S[m] + (w[p][:, None] * x[p] if norm else x[p])
    return n_in, N, S, d
