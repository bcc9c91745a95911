"""Weighted sampling without replacement (GPUMemoryPool_SetWeightedDistinct on top of the weighted kind / LEGION_SAMPLING=weighted
LEGION_WEIGHTED_DISTINCT=1, INTEGRATION.md "Weighted sampling without replacement") as a NumPy statement, shared by the CPU and the GPU
tests.  A helper module, not collected by pytest.

For hop h (1-based, op_id / 2), row i of that hop's input list with source node v, degree d (the int32 indptr difference), start =
indptr[v], fan-out f <= 64 and the batch's draw word W (0 unseeded), in the notation of tests/distinctref.py:

  K      = mix32(mix32((i + 0x9E3779B9 * h) ^ W) ^ 0x27D4EB2F)
  u_c    = mix32(K ^ (0x85EBCA6B * (c + 1)))          c in [0, d)            -- distinct_u(K, c): one hash per COLUMN
  x_c    = (float64(u_c) + 0.5) * 2^-32                                      -- exact, in (0, 1)
  key_c  = -log(x_c) / float64(w[start + c])          if w > 0               -- fp64 log, fp64 divide
  eligible columns: w[start + c] > 0;  m = their number
  m <= f : the picks are all eligible columns
  m >  f : the picks are the f eligible columns with the smallest (key_c, c)
  slot j < min(m, f) takes the j-th pick in ASCENDING COLUMN order; slot j >= min(m, f) (or source -1): no draw

Everything behind the position is the default mode's bookkeeping: run_batch() is distinctref.run_batch with a `draw` that returns these
positions.  The picks depend on the selected SET alone, so only the boundary between the f-th and the (f + 1)-th key can depend on the last
bit of a log: near_ties() names the rows where the two lie within 2^-40 of each other (relative).  The device log and NumPy's are each
within about 1 ulp (2^-52) and everything else in the key is correctly rounded, so 2^-40 is more than 2^10 times what the two can differ
by; such rows are the only ones a bit-compare may leave out, and the tests' cap on them is zero."""
import numpy as np

import distinctref as D
from distinctref import GOLDEN, M32, STEP, mix32
from weightedref import batch_seeds

WD_TAG = 0x27D4EB2F
TIE_MARGIN = 2.0 ** -40
MAX_FANOUT = 64


def column_keys(rows, hop, cols, w, W=0):
    """(u uint32, key float64), both of the broadcast shape: the hash and the key of column cols of row rows of hop hop at weight w under
    draw word W; key = +inf where w is not > 0."""
    rows, hop, cols, W, w = np.broadcast_arrays(*[np.asarray(x, dtype=np.int64) for x in (rows, hop, cols, W)], np.asarray(w, dtype=np.float32))
    shape = rows.shape
    K = mix32(mix32(((rows + GOLDEN * hop) & M32).astype(np.uint32) ^ W.astype(np.uint32)) ^ np.uint32(WD_TAG))
    u = mix32(K ^ ((STEP * (cols + 1)) & M32).astype(np.uint32).reshape(K.shape)).reshape(shape)
    x = (u.astype(np.float64) + 0.5) * 2.0 ** -32
    w64 = w.astype(np.float64)
    ok = w64 > 0
    key = np.where(ok, -np.log(x) / np.where(ok, w64, 1.0), np.inf)
    return u, key


def row_picks(i, h, w_row, f, W=0):
    """(picks, gap): the ascending columns row i of hop h takes of a row with weights w_row, and the relative distance of its f-th and
    (f + 1)-th key (inf when m <= f: nothing is cut)."""
    w_row = np.asarray(w_row, dtype=np.float32)
    pos, gap = _positions_block(np.array([i]), h, np.zeros(1, np.int64), np.array([len(w_row)]), int(f), W, w_row)
    return pos[0][pos[0] >= 0], float(gap[0])


def _positions_block(rows, hop, start, deg, f, W, w):
    """(pos int64 [n, f], gap float64 [n]) of n rows of degree >= 1, as one padded [n, max degree] block."""
    n, width = len(rows), int(deg.max())
    c = np.arange(width, dtype=np.int64)
    valid = c[None, :] < deg[:, None]
    ww = np.where(valid, w[np.where(valid, start[:, None] + c[None, :], 0)], np.float32(0))
    _, key = column_keys(rows[:, None], hop, c[None, :], ww, W)
    order = np.argsort(key, axis=1, kind="stable")                      # (key, column): a stable sort of the columns in ascending order
    m = (ww > 0).sum(axis=1)
    take = np.minimum(m, f)
    if width < f:
        order = np.concatenate([order, np.zeros((n, f - width), np.int64)], axis=1)
    j = np.arange(f, dtype=np.int64)
    big = np.iinfo(np.int64).max
    sel = np.sort(np.where(j[None, :] < take[:, None], order[:, :f], big), axis=1)
    pos = np.where(sel == big, -1, sel)
    gap = np.full(n, np.inf)
    cut = np.nonzero(m > f)[0]
    if len(cut):
        skey = np.take_along_axis(key[cut], order[cut][:, f - 1:f + 1], axis=1)
        gap[cut] = (skey[:, 1] - skey[:, 0]) / skey[:, 1]
    return pos, gap


def positions(rows, hop, start, deg, f, w, W=0):
    """(pos int64 [n, f], gap float64 [n]): the column slot j of row rows[m] takes (-1 = no draw) in a row of deg[m] columns whose weights
    begin at w[start[m]], and the row's relative key gap at the cut.  Rows are worked in blocks of similar degree."""
    rows, start, deg = (np.asarray(x, dtype=np.int64) for x in (rows, start, deg))
    f = int(f)
    assert 1 <= f <= MAX_FANOUT
    w = np.asarray(w, dtype=np.float32)
    pos, gap = np.full((len(rows), f), -1, dtype=np.int64), np.full(len(rows), np.inf)
    live = deg > 0
    bucket = np.where(live, np.ceil(np.log2(np.maximum(deg, 1))).astype(np.int64), -1)
    for b in np.unique(bucket[live]):
        at = np.nonzero(bucket == b)[0]
        step = max(1, (1 << 22) >> int(b))                               # blocks of at most ~4 M columns
        for lo in range(0, len(at), step):
            sl = at[lo:lo + step]
            pos[sl], gap[sl] = _positions_block(rows[sl], hop, start[sl], deg[sl], f, W, w)
    return pos, gap


class Weights:
    """A graph with its edge weights (float32[E], in indices order)."""

    def __init__(self, indptr, indices, w):
        self.indptr, self.indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices)
        self.w = np.asarray(w, dtype=np.float32)
        assert len(self.w) == int(self.indptr[-1])


def wd_positions(graph, first_inputs, W=0, ties=None):
    """A `draw` for ONE distinctref.run_batch call: the closure keeps the input list of the hop it is asked for, as
    weightedref.weighted_positions does.  ties: a list that receives (hop, row) of every row whose cut is a near tie."""
    state = dict(inp=np.asarray(first_inputs, dtype=np.int64), hop=1)

    def draw(rows, hop, deg, f):
        inp = state["inp"]
        assert int(hop) == state["hop"] and len(inp) == len(rows), (hop, state["hop"], len(inp), len(rows))
        rows, deg = np.asarray(rows, dtype=np.int64), np.asarray(deg, dtype=np.int64)
        node = np.where(inp >= 0, inp, 0)
        start = graph.indptr[node]
        pos, gap = positions(rows, int(hop), start, np.where(inp >= 0, deg, -1), f, graph.w, W)
        if ties is not None:
            ties.extend((int(hop), int(r)) for r in rows[gap < TIE_MARGIN])
        has = pos >= 0
        dst = np.where(has, graph.indices[np.where(has, start[:, None] + pos, 0)].astype(np.int64), -1)
        state["inp"], state["hop"] = dst[dst >= 0], state["hop"] + 1        # row-major = ascending slot
        return pos
    return draw


def run_batch(graph, feats, all_ids, all_labels, batch_size, counter, fanout, W=0, ties=None):
    """Batch `counter` of the list all_ids under draw word W."""
    draw = wd_positions(graph, batch_seeds(all_ids, batch_size, counter), W, ties)
    return D.run_batch(graph.indptr, graph.indices, feats, all_ids, all_labels, batch_size, counter, fanout, draw=draw)


def near_ties(graph, all_ids, batch_size, counters, fanout, W=0):
    """[(counter, hop, row)] of the rows of the batches `counters` whose f-th and (f + 1)-th keys differ by less than 2^-40 relative.  W: one
    draw word, or a function of the counter."""
    out = []
    zero = np.zeros((len(graph.indptr) - 1, 1), np.float32)
    for it in counters:
        ties = []
        run_batch(graph, zero, all_ids, np.zeros(len(all_ids), np.int64), batch_size, it, fanout, W(it) if callable(W) else W, ties)
        out.extend((int(it), h, r) for h, r in ties)
    return out


class Statement:
    """run_batch behind the oracle runner's signature (harness.replay_served); seed=None: unseeded, else tests/seededref.py's draw word
    and shuffled training list.  .ties collects (hop, row) of every near tie of every batch it ran."""

    def __init__(self, graph, feats, B, fan, seed=None, shuffle=True):
        self.graph, self.feats, self.B, self.fan, self.seed, self.shuffle = graph, feats, B, list(fan), seed, shuffle
        self.ties = []

    def run_batch(self, ids, lab, counter, mode=0, batch_size=None, round=0):
        W = 0
        if self.seed is not None:
            import seededref
            W = seededref.W(self.seed, round, counter)
            if mode == seededref.TRAINMODE and self.shuffle:
                ids, lab = seededref.shuffled(ids, lab, self.seed, round)
        return run_batch(self.graph, self.feats, ids, lab, self.B if batch_size is None else batch_size, counter, self.fan, W, self.ties)


def inclusion_probabilities(w, f):
    """Exact inclusion probabilities of successive sampling of f of len(w) items in proportion to w (plain recursion: small inputs only)."""
    w = [float(x) for x in w]
    out = [0.0] * len(w)

    def walk(left, picked, p, total):
        if left == 0 or total <= 0.0:
            return
        for k, x in enumerate(w):
            if k in picked or x <= 0.0:
                continue
            q = p * x / total
            out[k] += q
            walk(left - 1, picked | {k}, q, total - x)
    walk(int(f), frozenset(), 1.0, sum(w))
    return out
