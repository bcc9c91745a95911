"""Adversarial inputs for the aggregated last hop (tests/test_agg_numerics_cpu.py proves them on the CPU, tests/test_gpu_agg_adversarial.py
runs them on the GPU).  A helper module like aggref.py and gcnref.py, not collected by pytest.

  adversarial_features   a float32 table of named row classes: the values fp32 adds and products go wrong on
  bit_pattern_features   uniform random 32-bit words viewed as float32: what a gather must move without looking at
  assert_sum_bits        the comparison rule for sums, and statement_caps: what keeps that rule from hiding a failure
  MUTANTS                wrong implementations of the sums in NumPy: what the inputs must be able to tell from the statement
  adversarial_case       a random graph with hubs + the table + nodes whose neighbours are all of one special class
  star_graph             graphs whose block out-degrees are chosen, not drawn
"""
import numpy as np

from aggref import cum_edges, expected_nbr_sum, last_hop_runs
from gcnref import block_out_degree, expected_nbr_sum_norm

CLASSES = ("wide", "subnormal", "big", "inf", "nan", "negzero")
WIDE, SUBNORMAL, BIG, INF, NAN, NEGZERO = range(6)
BIG_VALUE = np.float32(3e38)                     # two equal-signed draws overflow: 6e38 > FLT_MAX = 3.4028e38
TINY = np.finfo(np.float32).tiny                 # 2^-126: the smallest normal
NAN_CAP = 0.05                                   # at most this share of a statement's elements may be NaN (statement_caps)


def special_columns(F):
    """(column of the +-inf entries, column of the NaN entries): two fixed columns, so that at F >= 4 at least half of every sum stays finite"""
    return 0, min(1, F - 1)


def adversarial_features(V, F, seed, keep_out=(), nonfinite=0.025, only=None):
    """(table float32 [V, F], cls int8 [V]): row v is of class CLASSES[cls[v]].
      wide       standard_normal * 2^k, k uniform in [-12, 12] per element: adds that lose low bits in both directions
      subnormal  standard_normal * 2^(-130 + k), k uniform in [-15, 5] per element: subnormal operands, sums and products
      big        +-3e38 in every column, one sign per row: two equal-signed draws overflow inside a run
      inf        a wide row with +inf or -inf in column special_columns(F)[0]
      nan        a wide row with a NaN in column special_columns(F)[1]: quiet and signalling, either sign, random payloads
      negzero    -0.0 in every column
    `nonfinite`: the share of inf + nan rows (half each); big rows 3 %, negzero 4 %, subnormal 30 %, the rest wide.  keep_out: node ids
    (hubs) that must be wide or subnormal, so that no large share of a batch's runs draws a non-finite row.  only: a class name -- every
    row of that one class (the tables that show which class kills which mutant)."""
    rs = np.random.RandomState(seed)
    u = rs.rand(V)
    edges = np.cumsum([0.30, 0.03, nonfinite / 2, nonfinite / 2, 0.04])
    cls = np.full(V, WIDE, np.int8)
    for c, lo, hi in zip((SUBNORMAL, BIG, INF, NAN, NEGZERO), np.concatenate([[0.0], edges[:-1]]), edges):
        cls[(u >= lo) & (u < hi)] = c
    keep_out = np.asarray(keep_out, dtype=np.int64)
    if len(keep_out):
        cls[keep_out] = np.where(cls[keep_out] == SUBNORMAL, SUBNORMAL, WIDE)
    special = np.flatnonzero((cls == INF) | (cls == NAN))
    cls[special[int(round(nonfinite * V)):]] = WIDE      # never more than the share asked for, however the draw fell
    if only is not None:
        cls[:] = CLASSES.index(only)
    wide = (rs.standard_normal((V, F)) * np.exp2(rs.randint(-12, 13, size=(V, F)))).astype(np.float32)
    sub = (rs.standard_normal((V, F)) * np.exp2(-130.0 + rs.randint(-15, 6, size=(V, F)))).astype(np.float32)
    sign = np.where(rs.rand(V) < 0.5, np.float32(-1), np.float32(1))
    table = wide.copy()
    table[cls == SUBNORMAL] = sub[cls == SUBNORMAL]
    table[cls == BIG] = (sign[:, None] * BIG_VALUE)[cls == BIG]
    table[cls == NEGZERO] = np.float32(-0.0)
    c_inf, c_nan = special_columns(F)
    table[cls == INF, c_inf] = (sign * np.float32(np.inf))[cls == INF]
    # NaN words: exponent all ones, payload != 0; bit 22 set = quiet, clear = signalling.  Written as words: no arithmetic touches them.
    payload = rs.randint(1, 1 << 22, size=V).astype(np.uint32)
    quiet = (rs.rand(V) < 0.5).astype(np.uint32) << np.uint32(22)
    word = np.uint32(0x7F800000) | quiet | payload | ((sign < 0).astype(np.uint32) << np.uint32(31))
    bits = table.view(np.uint32)
    bits[cls == NAN, c_nan] = word[cls == NAN]
    assert np.isnan(table[cls == NAN, c_nan]).all() and table.dtype == np.float32
    return table, cls


def bit_pattern_features(V, F, seed):
    """uniform random uint32 words viewed as float32 [V, F]: NaNs of every payload, subnormals, both zeros, infinities"""
    return np.random.RandomState(seed).randint(0, 1 << 32, size=(V, F), dtype=np.uint64).astype(np.uint32).view(np.float32)


def assert_words_equal(name, got, want):
    """plain uint32 equality of two float32 arrays: the rule for COPIED rows"""
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d words differ, first at %s: %#010x vs %#010x" % (name, len(bad), bad[:3].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))


def assert_sum_bits(name, got, want):
    """The rule for SUMS.  Where `want` is NaN, `got` must be a NaN: payload and sign of a result NaN are not part of the contract (IEEE 754
    leaves them open; x86 SSE returns the first operand's payload quietened or the default NaN 0xFFC00000, the GPU its own default), so a
    NumPy statement cannot pin them.  Everywhere else the uint32 words must be equal: signs of zero and of infinity count."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    nan = np.isnan(want)
    if not np.isnan(got[nan]).all():
        bad = np.argwhere(nan & ~np.isnan(got))
        raise AssertionError("%s: %d elements are not NaN where the statement is, first at %s: %r" % (name, len(bad), bad[:3].tolist(), got[tuple(bad[0])]))
    a, b = got.view(np.uint32), want.view(np.uint32)
    diff = (a != b) & ~nan
    if diff.any():
        bad = np.argwhere(diff)
        i = tuple(bad[0])
        raise AssertionError("%s: %d words differ, first at %s: %r (%#010x) vs %r (%#010x)" % (name, len(bad), bad[:3].tolist(), got[i], a[i], want[i], b[i]))


def statement_caps(name, S):
    """What keeps assert_sum_bits honest, asserted on the NumPy statement ALONE before anything is compared with it: at most NAN_CAP of its
    elements are NaN (a NaN accepts any NaN), and none is -0.0 (a sum that starts from +0.0 cannot end there: x + (-x) = +0.0 and
    +0.0 + (-0.0) = +0.0 in round-to-nearest).  Returns the NaN share."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    share = float(np.isnan(S).mean()) if S.size else 0.0
    assert share <= NAN_CAP, "%s: %.2f %% of the statement's elements are NaN (cap %.0f %%)" % (name, 100 * share, 100 * NAN_CAP)
    assert not (S.view(np.uint32) == np.uint32(0x80000000)).any(), "%s: the statement holds a -0.0" % name
    return share


# ---- the statement and its mutants -------------------------------------------------------------------------------------------------
def statement(ref, indptr, indices, fan, x=None, weighted=False):
    """S of the plain (tests/aggref.py) or the normalised (tests/gcnref.py) statement, as the mutants return theirs"""
    with np.errstate(all="ignore"):
        return (expected_nbr_sum_norm(ref, indptr, indices, fan, x=x)[3] if weighted else expected_nbr_sum(ref, indptr, indices, fan, x=x)[3])


def _runs(ref, indptr, indices, fan, x):
    x = np.asarray(ref["features"] if x is None else x, dtype=np.float32)
    H, f = len(fan), int(fan[-1])
    n_in, N, run_dst, cnt = last_hop_runs(ref, indptr, indices, fan)
    e0, e1 = cum_edges(ref["ec"], H - 1), cum_edges(ref["ec"], H)
    src = np.asarray(ref["src_off"][e0:e1], dtype=np.int64)
    return x, f, N, cnt, src, np.cumsum(cnt) - cnt


def _once_rounded_weights(ref, fan):
    d, _ = block_out_degree(ref, fan)
    return (1.0 / np.sqrt(d.clip(1).astype(np.float64))).astype(np.float32)


def _flush(a):
    """flush-to-zero of float32 values: a subnormal becomes a zero of its sign"""
    a = np.asarray(a, dtype=np.float32)
    return np.where((np.abs(a) < TINY) & (a != 0), np.copysign(np.float32(0), a), a).astype(np.float32)


def _sequential(ref, indptr, indices, fan, x, weighted, order="slot", single_rounding=False, wide_acc=False, ftz=False, once=False):
    x, f, N, cnt, src, start = _runs(ref, indptr, indices, fan, x)
    w = (_once_rounded_weights(ref, fan) if once else block_out_degree(ref, fan)[1]) if weighted else None
    if ftz:
        x = _flush(x)
    acc = np.zeros((N, x.shape[1]), dtype=np.float64 if wide_acc else np.float32)
    with np.errstate(all="ignore"):
        for k in range(f):
            m = cnt > k
            if not m.any():
                continue
            p = src[start[m] + (k if order == "slot" else cnt[m] - 1 - k)]
            if single_rounding and weighted:          # fl(w * x + acc): the product is exact in float64 (24 + 24 bits)
                acc[m] = (w[p][:, None].astype(np.float64) * x[p].astype(np.float64) + acc[m].astype(np.float64)).astype(np.float32)
                continue
            term = w[p][:, None] * x[p] if weighted else x[p]
            assert term.dtype == np.float32
            if ftz:
                term = _flush(term)
            acc[m] = acc[m] + term
            if ftz:
                acc[m] = _flush(acc[m])
        return acc.astype(np.float32)


def _pairwise(ref, indptr, indices, fan, x=None, weighted=False):
    """the draws of a run added as a balanced tree, then + 0.0f"""
    x, f, N, cnt, src, start = _runs(ref, indptr, indices, fan, x)
    w = block_out_degree(ref, fan)[1] if weighted else None
    T = np.zeros((N, f, x.shape[1]), np.float32)
    have = np.arange(f)[None, :] < cnt[:, None]
    with np.errstate(all="ignore"):
        for j in range(f):
            m = cnt > j
            p = src[start[m] + j]
            T[m, j] = w[p][:, None] * x[p] if weighted else x[p]
        while T.shape[1] > 1:
            if T.shape[1] & 1:
                T = np.concatenate([T, np.zeros((N, 1, T.shape[2]), np.float32)], axis=1)
                have = np.concatenate([have, np.zeros((N, 1), bool)], axis=1)
            a, b, hb = T[:, 0::2], T[:, 1::2], have[:, 1::2]
            T = np.where(hb[:, :, None], a + b, a)         # the draws are a prefix of the slots here: a right operand implies a left one
            have = have[:, 0::2]
        return np.where(have[:, 0, None], np.float32(0) + T[:, 0], np.float32(0)).astype(np.float32)


MUTANTS = {
    # name: (function over (ref, indptr, indices, fan, x=None, weighted=False) -> S, the forms it differs in)
    "reversed":  (lambda *a, x=None, weighted=False: _sequential(*a, x, weighted, order="reversed"), ("plain", "weighted")),
    "pairwise":  (_pairwise, ("plain", "weighted")),
    "fma":       (lambda *a, x=None, weighted=False: _sequential(*a, x, weighted, single_rounding=True), ("weighted",)),
    "float64":   (lambda *a, x=None, weighted=False: _sequential(*a, x, weighted, wide_acc=True), ("plain", "weighted")),
    "ftz":       (lambda *a, x=None, weighted=False: _sequential(*a, x, weighted, ftz=True), ("plain", "weighted")),
    "rsq":       (lambda *a, x=None, weighted=False: _sequential(*a, x, weighted, once=True), ("weighted",)),
}


def differs(name, got, want):
    """does assert_sum_bits tell `got` from `want`"""
    try:
        assert_sum_bits(name, got, want)
    except AssertionError:
        return True
    return False


def run_input_flags(ref, indptr, indices, fan, x=None):
    """(inf_in, nan_in) bool [N, F]: whether any draw of the run holds an infinity / a NaN in that column"""
    x, f, N, cnt, src, start = _runs(ref, indptr, indices, fan, x)
    inf_in, nan_in = np.zeros((N, x.shape[1]), bool), np.zeros((N, x.shape[1]), bool)
    for j in range(f):
        m = cnt > j
        p = src[start[m] + j]
        inf_in[m] |= np.isinf(x[p])
        nan_in[m] |= np.isnan(x[p])
    return inf_in, nan_in


RESULT_CLASSES = ("subnormal result", "inf by overflow", "inf from an inf input", "NaN from a NaN input", "NaN from inf - inf")


def result_classes(ref, indptr, indices, fan, S, x=None):
    """how many elements of the statement S are of each of RESULT_CLASSES"""
    inf_in, nan_in = run_input_flags(ref, indptr, indices, fan, x)
    fin = ~inf_in & ~nan_in
    return {"subnormal result": int(((S != 0) & (np.abs(S) < TINY)).sum()),
            "inf by overflow": int((np.isinf(S) & fin).sum()),
            "inf from an inf input": int((np.isinf(S) & inf_in & ~nan_in).sum()),
            "NaN from a NaN input": int((np.isnan(S) & nan_in).sum()),
            "NaN from inf - inf": int((np.isnan(S) & ~nan_in).sum())}


# ---- graphs -------------------------------------------------------------------------------------------------------------------------
MIXERS = ("infmix", "infone", "bigpos", "bigneg", "nanmix", "submix")


def adversarial_case(V, F, seed, n_seeds=900, nonfinite=0.025):
    """A random graph with hubs (no -1 entries: holes are the randomised tests' business), the adversarial table with the hubs kept out of
    the special classes, and 4 "mixer" nodes per kind of MIXERS whose 30 neighbours all come from one pool -- inf rows of both signs, inf
    rows of one sign + wide rows, big rows of one sign, NaN rows + wide rows, subnormal rows -- so that every result class occurs at every
    fan-out >= 2 by construction and not by luck.  5 % of all neighbour entries and every 13th seed name a mixer: they are inputs of the last
    hop at every H.  Returns a dict: V, F, indptr, indices, labels, seeds, table, cls, hubs, mixers."""
    rs = np.random.RandomState(seed)
    deg = rs.geometric(0.2, size=V) - 1
    hubs = rs.choice(V, size=max(1, V // 100), replace=False)
    deg[hubs] = rs.randint(50, 300, size=len(hubs))
    table, cls = adversarial_features(V, F, seed + 1, keep_out=hubs, nonfinite=nonfinite)
    plain = np.setdiff1d(np.flatnonzero(cls == WIDE), hubs)
    mixers = rs.choice(plain, size=4 * len(MIXERS), replace=False)
    deg[mixers] = 30
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    u = rs.rand(E)
    nbr = np.where(u < 0.4, rs.choice(hubs, size=E), rs.randint(0, V, size=E))
    nbr = np.where(u > 0.95, rs.choice(mixers, size=E), nbr)
    c_inf = special_columns(F)[0]
    pos = table[:, c_inf] > 0
    pools = dict(infmix=np.flatnonzero(cls == INF),
                 infone=np.concatenate([np.flatnonzero((cls == INF) & pos), plain[:20]]),
                 bigpos=np.flatnonzero((cls == BIG) & (table[:, 0] > 0)), bigneg=np.flatnonzero((cls == BIG) & (table[:, 0] < 0)),
                 nanmix=np.concatenate([np.flatnonzero(cls == NAN), plain[20:40]]), submix=np.flatnonzero(cls == SUBNORMAL))
    for i, m in enumerate(mixers):
        pool = pools[MIXERS[i % len(MIXERS)]]
        assert len(pool) >= 2, (MIXERS[i % len(MIXERS)], "V is too small for this class share")
        nbr[indptr[m]:indptr[m + 1]] = rs.choice(pool, size=30)
    seeds = rs.permutation(np.setdiff1d(np.arange(V), mixers))[:n_seeds].astype(np.int32)
    at = np.arange(0, len(seeds), 13)                 # no seed twice within 13 * 24 = 312 neighbouring seeds: aggref's plain statement has no
    seeds[at] = mixers[np.arange(len(at)) % len(mixers)]      # rule for a seed that repeats inside a batch (gcnref's has; tested elsewhere)
    return dict(V=V, F=F, indptr=indptr, indices=nbr.astype(np.int32), labels=rs.randint(0, 9, size=V).astype(np.int32), seeds=seeds,
                table=table, cls=cls, hubs=hubs, mixers=mixers)


def star_graph(batches, f, B, arrangement, hops=1, idle=0, self_target=0, seed=0):
    """A graph whose block out-degrees are chosen.  Every adjacency entry of an input node s is the same target t_s, so whatever index the
    sampler's RNG draws, the neighbour is t_s; deg_s lies in 1..f, so s contributes min(deg_s, f) = deg_s edges that all name t_s, and
    d[position of t] = the sum of deg_s over the inputs of the batch that name t.

    batches: per batch the list of intended degrees, one target each.  A degree d takes d // f inputs of degree f and one of degree
    d % f.  Every batch is filled up to exactly B inputs: `idle` inputs of degree 0 (an edge count that the others cannot reach), then one
    more target that takes the remaining inputs at degree f.  self_target > 0: the first batch also holds one input whose neighbours
    are all itself, with that degree (<= f): the one case where a target is also an input.  Otherwise targets are never inputs.
    arrangement "grouped": the inputs of a target are neighbours, src_off holds one run of d equal positions per target;
                "round_robin": the batch's targets take turns, no two neighbouring INPUTS name the same target while more than one target
                has inputs left (at f = 1 no two neighbouring edges are equal).
    hops = 1: the inputs are the seeds.  hops = 2: every seed has one neighbour of its own (a "middle" node, degree-1 hop, fan-out 2) and the
    middles are the inputs, in seed order; every middle's position then counts its hop-1 edge as well.
    Node ids are shuffled by `seed`.  Returns a dict: V, indptr, indices, seeds (len(batches) * B of them, batch k = counter k), fan, and
    want: per batch {node id: intended out-degree} of every node with one -- all other positions of the batch have d = 0."""
    arrangements = [arrangement] * len(batches) if isinstance(arrangement, str) else list(arrangement)     # one for all, or one per batch
    assert len(arrangements) == len(batches) and set(arrangements) <= {"grouped", "round_robin"} and hops in (1, 2) and 0 <= self_target <= f
    adj, inputs_of_batch, want = [], [], []           # adj[node] = (target node, degree), by provisional node number

    def node(target, degree):
        adj.append((target, degree))
        return len(adj) - 1

    for k, degrees in enumerate(batches):
        groups, w = [], {}
        for d in list(degrees):
            t = node(None, 0)
            groups.append([node(t, f) for _ in range(d // f)] + ([node(t, d % f)] if d % f else []))
            w[t] = d
        if k == 0 and self_target:
            s = node(None, 0)
            adj[s] = (s, self_target)
            groups.append([s])
            w[s] = self_target
        used = sum(len(g) for g in groups) + idle
        assert used <= B, "batch %d needs %d inputs, B is %d" % (k, used, B)
        if used < B:
            t = node(None, 0)
            groups.append([node(t, f) for _ in range(B - used)])
            w[t] = (B - used) * f
        if arrangements[k] == "grouped":
            order = [s for g in groups for s in g]
        else:
            order, depth = [], 0
            while len(order) < sum(len(g) for g in groups):
                order += [g[depth] for g in groups if len(g) > depth]
                depth += 1
        order += [node(None, 0) for _ in range(idle)]
        assert len(order) == B
        if hops == 2:
            for s in order:
                w[s] = w.get(s, 0) + 1                # the hop-1 edge names the middle
        inputs_of_batch.append(order)
        want.append(w)
    seeds = []
    for order in inputs_of_batch:
        seeds += [node(s, 1) for s in order] if hops == 2 else order
    V = len(adj)
    new = np.random.RandomState(seed).permutation(V)   # provisional number -> node id
    deg = np.zeros(V, np.int64)
    tgt = np.zeros(V, np.int64)
    for i, (t, dg) in enumerate(adj):
        deg[new[i]], tgt[new[i]] = dg, (new[t] if t is not None else 0)
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = np.repeat(tgt, deg).astype(np.int32)
    return dict(V=V, indptr=indptr, indices=indices, seeds=new[np.asarray(seeds)].astype(np.int32), fan=([2, f] if hops == 2 else [f]),
                want=[{int(new[t]): d for t, d in w.items()} for w in want], B=B)


# the shape tests/test_gpu_agg_adversarial.py::test_special_values_through_the_sums runs and tests/test_agg_numerics_cpu.py proves: adversarial_case(
# CASE_V, F, CASE_SEED, n_seeds=CASE_SEEDS), batch size CASE_B, these fan-outs (last ones 3, 10, 25 at H = 1, 2, 3) and these batches (2 is short: 41 seeds)
CASE_V, CASE_SEED, CASE_B, CASE_SEEDS = 3000, 11, 300, 641
CASE_FANS = ([3], [10], [25], [5, 3], [4, 10], [3, 25], [3, 2, 3], [3, 2, 10], [2, 2, 25])
CASE_BATCHES = (0, 1, 2)

STAR_E = (1, 63, 64, 65, 255, 256, 257, 511, 513)


def star_edge_case(E, hops):
    """the star graph of one edge count E of block 1, last fan-out 1: batch 0 grouped (one position receives every last-hop edge), batch 1
    round-robin over two targets (no two neighbouring last-hop edges are equal)"""
    if hops == 1:
        return star_graph([[E], [E - E // 2] + ([E // 2] if E > 1 else [])], 1, E, ("grouped", "round_robin"), seed=E)
    B = (E + 1) // 2                                  # E = B hop-1 edges + (E - B) last-hop edges; B - (E - B) inputs stay without a draw
    k = E - B
    return star_graph([[k] if k else [], ([k - k // 2] + ([k // 2] if k > 1 else [])) if k else []], 1, B, ("grouped", "round_robin"), hops=2, idle=B - k, seed=E)


def equal_runs(a):
    """(start, length) of the maximal runs of equal neighbouring values"""
    a = np.asarray(a)
    if len(a) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    start = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1]]))
    return start, np.diff(np.concatenate([start, [len(a)]]))


def coverage_batches(f, B, rs):
    """Per batch the intended degrees such that every integer of [1, 1024] is some target's degree, in a shuffled order, packed greedily
    into batches of at most B inputs (star_graph fills each up), and one last batch whose B inputs all name one target: d = B * f."""
    batches, cur, used = [], [], 0
    for d in rs.permutation(np.arange(1, 1025)).tolist():
        need = -(-d // f)
        if used + need > B:
            batches.append(cur)
            cur, used = [], 0
        cur.append(d)
        used += need
    batches.append(cur)
    batches.append([])                                # star_graph's filler takes all B inputs
    return batches
