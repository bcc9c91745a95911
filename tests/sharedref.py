"""Shared-key sampling (GPUMemoryPool_SetSharedDraws on top of the distinct kind / LEGION_SAMPLING=distinct LEGION_SHARED_DRAWS=1,
INTEGRATION.md "Shared-key sampling") as a NumPy statement, shared by the CPU and the GPU tests.  A helper module, not collected by pytest.

For hop h, row i of the hop's input list with source node v, degree d (the int32 indptr difference), nbr[c] = indices[indptr[v] + c],
fan-out f <= 64 and the batch's draw word W (0 unseeded), in the notation of tests/distinctref.py, all uint32 with wrap-around:

  Ks     = mix32(W ^ 0x165667B1)                               -- the batch's node-key salt: no hop, no row
  key_c  = mix32(uint32(nbr[c]) ^ Ks)          c in [0, d)     -- a function of the NEIGHBOUR ID and the batch only
  d <= f : the picks are all columns (no key is formed)
  d >  f : the picks are the f columns of smallest (key_c, c), compared lexicographically
  slot j < min(d, f) takes the j-th pick in ASCENDING COLUMN order; slot j >= min(d, f) (or source -1): no draw

mix32 is a bijection, so only equal ids (multi-edges) tie and the column settles those; a negative entry is keyed by its bit pattern and,
when picked, is "no edge" by the dst < 0 rule like everywhere.  Everything behind the position is the default mode's bookkeeping:
run_batch() is distinctref.run_batch with a `draw` that returns these positions.  Every value is an integer: the GPU is compared bit for
bit, no row is left out."""
import numpy as np

import distinctref as D
from distinctref import M32, mix32, mix32_scalar
from weightedref import batch_seeds

SALT_TAG = 0x165667B1
MAX_FANOUT = 64


def salt(W=0):
    return mix32_scalar((int(W) & M32) ^ SALT_TAG)


def node_keys(ids, W=0):
    """uint32, the shape of ids: the node key of every id (int32 bit patterns) under draw word W (a scalar or an array of ids' shape)."""
    ids = np.asarray(ids)
    Wa = np.broadcast_to(np.asarray(W, dtype=np.int64) & M32, ids.shape).astype(np.uint32)
    ks = mix32(Wa.reshape(-1) ^ np.uint32(SALT_TAG))
    return mix32(ids.astype(np.int32).view(np.uint32).reshape(-1) ^ ks).reshape(ids.shape)


def row_picks(nbr, f, W=0):
    """the ascending columns a row with neighbour list nbr takes at fan-out f"""
    nbr = np.asarray(nbr, dtype=np.int32)
    pos = positions(np.zeros(1, np.int64), np.array([len(nbr)]), int(f), nbr, W)[0]
    return pos[pos >= 0]


def _positions_block(start, deg, f, indices, W):
    """int64 [n, f] of n rows of degree > f, as one padded [n, max degree] block of packed (key << 32 | column) words"""
    width = int(deg.max())
    c = np.arange(width, dtype=np.int64)
    valid = c[None, :] < deg[:, None]
    nbr = indices[np.where(valid, start[:, None] + c[None, :], 0)]
    packed = (node_keys(nbr, W).astype(np.uint64) << np.uint64(32)) | c[None, :].astype(np.uint64)
    packed = np.where(valid, packed, np.uint64(0xFFFFFFFFFFFFFFFF))
    best = np.partition(packed, f - 1, axis=1)[:, :f]                   # the f smallest words, in any order
    return np.sort((best & np.uint64(M32)).astype(np.int64), axis=1)


def positions(start, deg, f, indices, W=0):
    """int64 [n, f]: the column slot j of a row of deg[m] columns beginning at indices[start[m]] takes; -1 = no draw.  Rows are worked in
    blocks of similar degree."""
    start, deg = np.asarray(start, dtype=np.int64), np.asarray(deg, dtype=np.int64)
    f = int(f)
    assert 1 <= f <= MAX_FANOUT
    indices = np.asarray(indices)
    j = np.arange(f, dtype=np.int64)
    pos = np.where(j[None, :] < deg[:, None], j[None, :], -1)                # d <= f (and, overwritten below, d > f)
    big = deg > f
    bucket = np.where(big, np.ceil(np.log2(np.maximum(deg, 1))).astype(np.int64), -1)
    for b in np.unique(bucket[big]):
        at = np.nonzero(bucket == b)[0]
        step = max(1, (1 << 22) >> int(b))                                  # blocks of at most ~4 M columns
        for lo in range(0, len(at), step):
            sl = at[lo:lo + step]
            pos[sl] = _positions_block(start[sl], deg[sl], f, indices, W)
    return pos


def shared_positions(indptr, indices, first_inputs, W=0):
    """A `draw` for ONE distinctref.run_batch call: the closure keeps the input list of the hop it is asked for, as
    wdistinctref.wd_positions does (the keys belong to the neighbours, which the hop's sources name)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices)
    state = dict(inp=np.asarray(first_inputs, dtype=np.int64), hop=1)

    def draw(rows, hop, deg, f):
        inp = state["inp"]
        assert int(hop) == state["hop"] and len(inp) == len(rows), (hop, state["hop"], len(inp), len(rows))
        deg = np.asarray(deg, dtype=np.int64)
        start = indptr[np.where(inp >= 0, inp, 0)]
        pos = positions(start, np.where(inp >= 0, deg, -1), f, indices, W)
        has = pos >= 0
        dst = np.where(has, indices[np.where(has, start[:, None] + pos, 0)].astype(np.int64), -1)
        state["inp"], state["hop"] = dst[dst >= 0], state["hop"] + 1        # row-major = ascending slot
        return pos
    return draw


def run_batch(indptr, indices, feats, all_ids, all_labels, batch_size, counter, fanout, W=0):
    """Batch `counter` of the list all_ids under draw word W."""
    draw = shared_positions(indptr, indices, batch_seeds(all_ids, batch_size, counter), W)
    return D.run_batch(indptr, indices, feats, all_ids, all_labels, batch_size, counter, fanout, draw=draw)


class Statement:
    """run_batch behind the oracle runner's signature (harness.replay_served); seed=None: unseeded (draw word 0), else tests/seededref.py's
    draw word and shuffled training list."""

    def __init__(self, indptr, indices, feats, B, fan, seed=None, shuffle=True):
        self.a, self.B, self.fan, self.seed, self.shuffle = (indptr, indices, feats), B, list(fan), seed, shuffle

    def run_batch(self, ids, lab, counter, mode=0, batch_size=None, round=0):
        W = 0
        if self.seed is not None:
            import seededref
            W = seededref.W(self.seed, round, counter)
            if mode == seededref.TRAINMODE and self.shuffle:
                ids, lab = seededref.shuffled(ids, lab, self.seed, round)
        return run_batch(*self.a, ids, lab, self.B if batch_size is None else batch_size, counter, self.fan, W)
