"""Weighted shared-key sampling (GPUMemoryPool_SetSharedDraws on top of the weighted kind with GPUMemoryPool_SetWeightedDistinct /
LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1 LEGION_SHARED_DRAWS=1, INTEGRATION.md "Weighted shared-key sampling") as a NumPy
statement, shared by the CPU and the GPU tests.  A helper module, not collected by pytest.

For a row with source node v, start = indptr[v], degree d (the int32 indptr difference), fan-out f <= 64 and the batch's draw word W (0
unseeded), in the notation of tests/wdistinctref.py and tests/sharedref.py:

  Ksw    = mix32(mix32(W ^ 0x165667B1) ^ 0x27D4EB2F)                         -- sharedref.salt(W), re-tagged: no row, no hop
  u_c    = mix32(uint32(indices[start + c]) ^ Ksw)    c in [0, d)            -- one hash per NEIGHBOUR NODE (the id's bit pattern, -1 holes included)
  x_c    = (float64(u_c) + 0.5) * 2^-32                                      -- exact, in (0, 1)
  key_c  = -log(x_c) / float64(w[start + c])          if w > 0               -- fp64 log, fp64 divide: wdistinctref's key as it is
  eligible columns: w[start + c] > 0;  m = their number
  m <= f : the picks are all eligible columns
  m >  f : the picks are the f eligible columns with the smallest (key_c, c)
  slot j < min(m, f) takes the j-th pick in ASCENDING COLUMN order; slot j >= min(m, f) (or source -1): no draw

Everything behind the position is the default mode's bookkeeping: run_batch() is distinctref.run_batch with a `draw` that returns these
positions, the arrangement of wdistinctref.wd_positions.  The picks depend on the selected SET alone, so only the cut between the f-th and
the (f + 1)-th key can depend on the last bit of a log: near_ties() names the rows where the two lie within 2^-40 of each other (relative),
by wdistinctref's margin and reasoning.  One case is new: two columns with the same neighbour id and the same weight bits have BIT-EQUAL
keys on the device and here alike (the same u, the same w, the same operations), and the column settles them exactly.  Such a cut is an
exact tie, not a near one: near_ties() leaves it out and exact_ties() names it."""
import numpy as np

import distinctref as D
from distinctref import M32, mix32, mix32_scalar
from sharedref import SALT_TAG
from wdistinctref import MAX_FANOUT, TIE_MARGIN, WD_TAG, Weights  # noqa: F401  (Weights: the graph type of this statement too)
from weightedref import batch_seeds


def salt(W=0):
    return mix32_scalar(mix32_scalar((int(W) & M32) ^ SALT_TAG) ^ WD_TAG)


def node_keys(ids, w, W=0):
    """(u uint32, key float64), both of the broadcast shape: the hash of neighbour id ids (int32 bit patterns) under draw word W and its key
    at weight w; key = +inf where w is not > 0."""
    ids, W, w = np.broadcast_arrays(np.asarray(ids, dtype=np.int64), np.asarray(W, dtype=np.int64), np.asarray(w, dtype=np.float32))
    shape = ids.shape
    ks = mix32(mix32((W.reshape(-1) & M32).astype(np.uint32) ^ np.uint32(SALT_TAG)) ^ np.uint32(WD_TAG))
    u = mix32(ids.reshape(-1).astype(np.int32).view(np.uint32) ^ ks).reshape(shape)
    x = (u.astype(np.float64) + 0.5) * 2.0 ** -32
    w64 = w.astype(np.float64)
    ok = w64 > 0
    key = np.where(ok, -np.log(x) / np.where(ok, w64, 1.0), np.inf)
    return u, key


def row_picks(nbr, w_row, f, W=0):
    """(picks, gap, exact): the ascending columns a row with neighbour list nbr and weights w_row takes, the relative distance of its f-th
    and (f + 1)-th key (inf when m <= f: nothing is cut, and when the cut is an exact tie), and whether the cut is an exact tie."""
    nbr, w_row = np.asarray(nbr, dtype=np.int32), np.asarray(w_row, dtype=np.float32)
    assert len(nbr) == len(w_row)
    if len(nbr) == 0:
        return np.zeros(0, np.int64), np.inf, False
    pos, gap, exact = _positions_block(np.zeros(1, np.int64), np.array([len(nbr)]), int(f), W, w_row, nbr)
    return pos[0][pos[0] >= 0], float(gap[0]), bool(exact[0])


def _positions_block(start, deg, f, W, w, indices):
    """(pos int64 [n, f], gap float64 [n], exact bool [n]) of n rows of degree >= 1, as one padded [n, max degree] block."""
    n, width = len(start), int(deg.max())
    c = np.arange(width, dtype=np.int64)
    valid = c[None, :] < deg[:, None]
    at = np.where(valid, start[:, None] + c[None, :], 0)
    ww = np.where(valid, w[at], np.float32(0))
    ids = np.where(valid, indices[at], 0).astype(np.int32)
    _, key = node_keys(ids, ww, W)
    order = np.argsort(key, axis=1, kind="stable")                      # (key, column): a stable sort of the columns in ascending order
    m = (ww > 0).sum(axis=1)
    take = np.minimum(m, f)
    if width < f:
        order = np.concatenate([order, np.zeros((n, f - width), np.int64)], axis=1)
    j = np.arange(f, dtype=np.int64)
    big = np.iinfo(np.int64).max
    sel = np.sort(np.where(j[None, :] < take[:, None], order[:, :f], big), axis=1)
    pos = np.where(sel == big, -1, sel)
    gap, exact = np.full(n, np.inf), np.zeros(n, bool)
    cut = np.nonzero(m > f)[0]
    if len(cut):
        two = order[cut][:, f - 1:f + 1]                                   # the columns on both sides of the cut
        skey = np.take_along_axis(key[cut], two, axis=1)
        sid, sw = np.take_along_axis(ids[cut], two, axis=1), np.take_along_axis(ww[cut], two, axis=1).view(np.uint32)
        same = (sid[:, 0] == sid[:, 1]) & (sw[:, 0] == sw[:, 1])         # the same node at the same weight bits: bit-equal keys on both sides
        assert (skey[same, 0] == skey[same, 1]).all()
        gap[cut] = np.where(same, np.inf, (skey[:, 1] - skey[:, 0]) / skey[:, 1])
        exact[cut] = same
    return pos, gap, exact


def positions(start, deg, f, indices, w, W=0):
    """(pos int64 [n, f], gap float64 [n], exact bool [n]): the column slot j of a row of deg[m] columns beginning at indices[start[m]] /
    w[start[m]] takes (-1 = no draw), the row's relative key gap at the cut and whether the cut is an exact tie.  Rows are worked in blocks
    of similar degree."""
    start, deg = np.asarray(start, dtype=np.int64), np.asarray(deg, dtype=np.int64)
    f = int(f)
    assert 1 <= f <= MAX_FANOUT
    indices, w = np.asarray(indices), np.asarray(w, dtype=np.float32)
    pos, gap, exact = np.full((len(start), f), -1, dtype=np.int64), np.full(len(start), np.inf), np.zeros(len(start), bool)
    live = deg > 0
    bucket = np.where(live, np.ceil(np.log2(np.maximum(deg, 1))).astype(np.int64), -1)
    for b in np.unique(bucket[live]):
        at = np.nonzero(bucket == b)[0]
        step = max(1, (1 << 22) >> int(b))                               # blocks of at most ~4 M columns
        for lo in range(0, len(at), step):
            sl = at[lo:lo + step]
            pos[sl], gap[sl], exact[sl] = _positions_block(start[sl], deg[sl], f, W, w, indices)
    return pos, gap, exact


def ws_positions(graph, first_inputs, W=0, ties=None, exact=None):
    """A `draw` for ONE distinctref.run_batch call: the closure keeps the input list of the hop it is asked for, as
    wdistinctref.wd_positions does.  ties / exact: lists that receive (hop, row) of every row whose cut is a near tie / an exact tie."""
    state = dict(inp=np.asarray(first_inputs, dtype=np.int64), hop=1)

    def draw(rows, hop, deg, f):
        inp = state["inp"]
        assert int(hop) == state["hop"] and len(inp) == len(rows), (hop, state["hop"], len(inp), len(rows))
        rows, deg = np.asarray(rows, dtype=np.int64), np.asarray(deg, dtype=np.int64)
        start = graph.indptr[np.where(inp >= 0, inp, 0)]
        pos, gap, ex = positions(start, np.where(inp >= 0, deg, -1), f, graph.indices, graph.w, W)
        if ties is not None:
            ties.extend((int(hop), int(r)) for r in rows[gap < TIE_MARGIN])
        if exact is not None:
            exact.extend((int(hop), int(r)) for r in rows[ex])
        has = pos >= 0
        dst = np.where(has, graph.indices[np.where(has, start[:, None] + pos, 0)].astype(np.int64), -1)
        state["inp"], state["hop"] = dst[dst >= 0], state["hop"] + 1        # row-major = ascending slot
        return pos
    return draw


def run_batch(graph, feats, all_ids, all_labels, batch_size, counter, fanout, W=0, ties=None, exact=None):
    """Batch `counter` of the list all_ids under draw word W."""
    draw = ws_positions(graph, batch_seeds(all_ids, batch_size, counter), W, ties, exact)
    return D.run_batch(graph.indptr, graph.indices, feats, all_ids, all_labels, batch_size, counter, fanout, draw=draw)


def _cuts(graph, all_ids, batch_size, counters, fanout, W, which):
    out = []
    zero = np.zeros((len(graph.indptr) - 1, 1), np.float32)
    for it in counters:
        found = []
        run_batch(graph, zero, all_ids, np.zeros(len(all_ids), np.int64), batch_size, it, fanout, W(it) if callable(W) else W, **{which: found})
        out.extend((int(it), h, r) for h, r in found)
    return out


def near_ties(graph, all_ids, batch_size, counters, fanout, W=0):
    """[(counter, hop, row)] of the rows of the batches `counters` whose f-th and (f + 1)-th keys differ by less than 2^-40 relative and are
    not the bit-equal keys of one node at one weight.  W: one draw word, or a function of the counter."""
    return _cuts(graph, all_ids, batch_size, counters, fanout, W, "ties")


def exact_ties(graph, all_ids, batch_size, counters, fanout, W=0):
    """[(counter, hop, row)] of the rows whose cut falls between two columns of one node at one weight: settled by the column, exactly"""
    return _cuts(graph, all_ids, batch_size, counters, fanout, W, "exact")


class Statement:
    """run_batch behind the oracle runner's signature (harness.replay_served); seed=None: unseeded, else tests/seededref.py's draw word
    and shuffled training list.  .ties / .exact collect (hop, row) of every near / exact tie of every batch it ran."""

    def __init__(self, graph, feats, B, fan, seed=None, shuffle=True):
        self.graph, self.feats, self.B, self.fan, self.seed, self.shuffle = graph, feats, B, list(fan), seed, shuffle
        self.ties, self.exact = [], []

    def run_batch(self, ids, lab, counter, mode=0, batch_size=None, round=0):
        W = 0
        if self.seed is not None:
            import seededref
            W = seededref.W(self.seed, round, counter)
            if mode == seededref.TRAINMODE and self.shuffle:
                ids, lab = seededref.shuffled(ids, lab, self.seed, round)
        return run_batch(self.graph, self.feats, ids, lab, self.B if batch_size is None else batch_size, counter, self.fan, W, self.ties, self.exact)
