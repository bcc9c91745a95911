"""The weighted sampler mode (GPUMemoryPool_SetSampling(pool, 2) / LEGION_SAMPLING=weighted, INTEGRATION.md "Weighted sampling") as a NumPy
statement, shared by the CPU and the GPU tests.  A helper module, not collected by pytest.

The graph carries an alias table: one entry {uint32 thr, int32 alias_id} per CSR entry.  For hop h (1-based, op_id / 2), row i of that
hop's input list, slot j, degree d (the int32 indptr difference) and the batch's draw word W (0 unseeded), all uint32 with wrap-around
except the one 64-bit product, in the notation of tests/distinctref.py:

  slot j >= d (or source -1)   no draw
  K  = mix32(mix32((i + 0x9E3779B9 * h) ^ W) ^ 0xC2B2AE35)
  uc = mix32(K ^ (0x85EBCA6B * (2j + 1)));  ub = mix32(K ^ (0x85EBCA6B * (2j + 2)))          -- distinct_u(K, 2j), distinct_u(K, 2j + 1)
  k  = (uint64(uc) * d) >> 32
  e  = alias[start + k]
  dst = indices[start + k] if ub < e.thr else e.alias_id

Everything behind dst is the default mode's bookkeeping: run_batch() is distinctref.run_batch with a `draw` that returns a column whose
neighbour is dst (k itself, or the first column of the row that holds alias_id, or -1 for a negative alias_id: no edge).

build_table() is Vose's algorithm in plain Python (fp64 residuals); check_table() states what ANY valid table is, whoever built it."""
import numpy as np

import distinctref as D
from distinctref import GOLDEN, M32, STEP, mix32

WEIGHTED_TAG = 0xC2B2AE35
TWO32 = 1 << 32
P_BOUND = 2.0 ** -30        # |P(id) - w(id) / W|: 2^-32 of threshold quantisation per id, < 2^-40 of fp64 residual arithmetic for d <= 2^16, 4 x margin


# ---- one slot's draw -------------------------------------------------------------------------------
def slot_draw(rows, hop, slot, deg, w=0):
    """(k int64 [n], ub uint32 [n]): the column and the keep-or-alias word of slot slot[m] of row rows[m] of hop hop[m] at degree deg[m] > 0
    under draw word w (scalar or [n])."""
    rows, slot, deg = (np.asarray(x, dtype=np.int64) for x in (rows, slot, deg))
    hop = np.broadcast_to(np.asarray(hop, dtype=np.int64), rows.shape)
    w = np.broadcast_to(np.asarray(w, dtype=np.int64), rows.shape).astype(np.uint32)
    K = mix32(mix32(((rows + GOLDEN * hop) & M32).astype(np.uint32) ^ w) ^ np.uint32(WEIGHTED_TAG))
    uc = mix32(K ^ ((STEP * (2 * slot + 1)) & M32).astype(np.uint32))
    ub = mix32(K ^ ((STEP * (2 * slot + 2)) & M32).astype(np.uint32))
    k = ((uc.astype(np.uint64) * deg.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    return k, ub


def draw_ids(ids, thr, alias_id, rows, hop, slot, w=0):
    """The neighbour ids the slots draw from ONE row (ids / thr / alias_id: its d columns)."""
    ids, thr, alias_id = np.asarray(ids), np.asarray(thr, dtype=np.uint32), np.asarray(alias_id)
    k, ub = slot_draw(rows, hop, slot, np.full(len(np.asarray(rows)), len(ids)), w)
    return np.where(ub < thr[k], ids[k], alias_id[k])


# ---- the table -------------------------------------------------------------------------------------
def vose_row(ids, w):
    """(thr, alias_id) lists of one row: Vose's algorithm with fp64 residuals, small and large columns taken in column order.  A column
    that ends up keeping itself stores {2^32 - 1, own id}; an all-zero row is {0, -1} throughout."""
    d = len(ids)
    W = 0.0
    for x in w:
        W += float(x)
    if d == 0:
        return [], []
    if not W > 0.0:
        return [0] * d, [-1] * d
    p = [float(x) * d / W for x in w]
    thr, alias = [TWO32 - 1] * d, [int(i) for i in ids]
    small = [k for k in range(d) if p[k] < 1.0][::-1]
    large = [k for k in range(d) if p[k] >= 1.0][::-1]
    while small and large:
        s, l = small.pop(), large[-1]
        thr[s] = min(int(p[s] * TWO32), TWO32 - 1)
        alias[s] = int(ids[l])
        p[l] = (p[l] + p[s]) - 1.0
        if p[l] < 1.0 and len(large) > 1:       # the last large column stays the alias of every small one left
            small.append(large.pop())
    return thr, alias


def build_table(indptr, indices, w):
    """(thr uint32 [E], alias_id int32 [E]) by vose_row over every row."""
    indptr = np.asarray(indptr)
    E = int(indptr[-1])
    thr, alias = np.zeros(E, np.uint32), np.zeros(E, np.int32)
    for v in range(len(indptr) - 1):
        a, b = int(indptr[v]), int(indptr[v + 1])
        if b > a:
            t, al = vose_row(indices[a:b], w[a:b])
            thr[a:b], alias[a:b] = t, al
    return thr, alias


def _pair_keys(rowof, ids):
    return rowof.astype(np.int64) * TWO32 + (np.asarray(ids).astype(np.int64) + (1 << 31))


def check_table(indptr, indices, w, thr, alias_id):
    """Assert that (thr, alias_id) is a valid alias table of the weights w on the CSR, per row:
    - every alias_id is an id of the row -- or every entry is {0, -1}, exactly when the row's weights sum to 0;
    - P(id) = sum over the row's columns of [own id: thr ; aliased to id: 2^32 - thr] / (d 2^32) is exactly 0 for an id whose columns all
      weigh 0, and within 2^-30 of the id's share of the row's weight (fp64) otherwise.
    Returns the largest |P - share| seen."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices)
    w64 = np.asarray(w, dtype=np.float64)
    thr, alias_id = np.asarray(thr, dtype=np.uint32).astype(np.int64), np.asarray(alias_id).astype(np.int64)
    V, E = len(indptr) - 1, int(indptr[-1])
    assert len(indices) >= E and len(w64) == E and len(thr) == E and len(alias_id) == E
    indices = indices[:E]
    deg = np.diff(indptr)
    rowof = np.repeat(np.arange(V, dtype=np.int64), deg)
    Wrow = np.zeros(V, np.float64)
    np.add.at(Wrow, rowof, w64)
    zero_row = (Wrow == 0.0)[rowof]
    sentinel = (thr == 0) & (alias_id == -1)
    bad = np.nonzero(zero_row & ~sentinel)[0]
    assert len(bad) == 0, "entry %d of all-zero row %d is {%d, %d}, not {0, -1}" % (bad[0], rowof[bad[0]], thr[bad[0]], alias_id[bad[0]]) if len(bad) else ""
    live = ~zero_row
    # in a row with weight, a {0, -1} entry is legitimate only if -1 is an id of the row: covered by the membership test below
    own = _pair_keys(rowof[live], indices[live])
    ali = _pair_keys(rowof[live], alias_id[live])
    keys, inv_own = np.unique(own, return_inverse=True)
    at = np.searchsorted(keys, ali)
    member = (at < len(keys)) & (keys[np.minimum(at, max(len(keys) - 1, 0))] == ali) if len(keys) else np.zeros(len(ali), bool)
    miss = np.nonzero(~member)[0]
    if len(miss):
        e = np.nonzero(live)[0][miss[0]]
        raise AssertionError("entry %d of row %d aliases id %d, which is no neighbour of the row" % (e, rowof[e], alias_id[e]))
    num = np.zeros(len(keys), np.uint64)                         # sums stay below d 2^32 < 2^64
    np.add.at(num, inv_own, thr[live].astype(np.uint64))
    np.add.at(num, at, (TWO32 - thr[live]).astype(np.uint64))
    wsum = np.zeros(len(keys), np.float64)
    np.add.at(wsum, inv_own, w64[live])
    key_row = keys // TWO32
    share = wsum / Wrow[key_row]
    P = num.astype(np.float64) / (deg[key_row].astype(np.float64) * float(TWO32))
    ghost = np.nonzero((wsum == 0.0) & (num != 0))[0]
    assert len(ghost) == 0, "row %d gives id %d, whose columns all weigh 0, %d / (d 2^32) of its draws" % (
        key_row[ghost[0]], keys[ghost[0]] % TWO32 - (1 << 31), num[ghost[0]]) if len(ghost) else ""
    err = np.abs(P - share)
    worst = int(np.argmax(err)) if len(err) else 0
    assert len(err) == 0 or err[worst] <= P_BOUND, "row %d, id %d: P = %.12g, its share of the weight is %.12g (off by %.3g > 2^-30)" % (
        key_row[worst], keys[worst] % TWO32 - (1 << 31), P[worst], share[worst], err[worst])
    return float(err.max()) if len(err) else 0.0


# ---- the whole batch -------------------------------------------------------------------------------
class Table:
    """A graph with its alias table, and where the first column of (row, id) lies."""

    def __init__(self, indptr, indices, thr, alias_id):
        self.indptr, self.indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices)
        self.thr, self.alias_id = np.asarray(thr, dtype=np.uint32), np.asarray(alias_id, dtype=np.int32)
        V, E = len(self.indptr) - 1, int(self.indptr[-1])
        rowof = np.repeat(np.arange(V, dtype=np.int64), np.diff(self.indptr))
        col = np.arange(E, dtype=np.int64) - self.indptr[rowof]
        keys = _pair_keys(rowof, self.indices[:E])
        order = np.lexsort((col, keys))
        self._keys, self._cols = keys[order], col[order]

    def first_column(self, node, ids):
        """the first column of row `node` that holds id `ids` (both [n]); the id must be in the row"""
        q = _pair_keys(np.asarray(node, dtype=np.int64), ids)
        at = np.searchsorted(self._keys, q, side="left")
        assert (self._keys[np.minimum(at, len(self._keys) - 1)] == q).all(), "an alias id is no neighbour of its row"
        return self._cols[at]


def batch_seeds(all_ids, batch_size, counter):
    """hop 1's input list as distinctref.run_batch forms it"""
    total_cap = len(all_ids)
    size = (total_cap - batch_size * counter) if batch_size * (counter + 1) >= total_cap else batch_size
    size = max(size, 0)
    g = size * counter + np.arange(size, dtype=np.int64)
    return np.where(g < total_cap, np.asarray(all_ids, dtype=np.int64)[g % max(total_cap, 1)], -1) if size else np.zeros(0, np.int64)


def weighted_positions(table, first_inputs, w=0):
    """A `draw` for ONE distinctref.run_batch call: the closure keeps the input list of the hop it is asked for -- hop 1's is
    first_inputs, a later hop's the neighbours its own answer to the hop before gave, in slot order (what run_batch appends to agg_src)."""
    state = dict(inp=np.asarray(first_inputs, dtype=np.int64), hop=1)

    def draw(rows, hop, deg, f):
        inp = state["inp"]
        assert int(hop) == state["hop"] and len(inp) == len(rows), (hop, state["hop"], len(inp), len(rows))
        rows, deg, f = np.asarray(rows, dtype=np.int64), np.asarray(deg, dtype=np.int64), int(f)
        node = np.where(inp >= 0, inp, 0)
        start = table.indptr[node]
        j = np.arange(f, dtype=np.int64)
        has = j[None, :] < deg[:, None]
        shape = has.shape
        k, ub = slot_draw(np.repeat(rows, f), hop, np.tile(j, len(rows)), np.where(has, deg[:, None], 1).reshape(-1), w)
        k, ub = k.reshape(shape), ub.reshape(shape)
        e = np.where(has, start[:, None] + k, 0)
        keep = ub < table.thr[e]
        a = table.alias_id[e].astype(np.int64)
        pos = np.where(keep, k, -1)
        look = has & ~keep & (a >= 0)
        if look.any():
            pos[look] = table.first_column(np.broadcast_to(node[:, None], shape)[look], a[look])
        pos = np.where(has, pos, -1)
        dst = np.where(pos >= 0, table.indices[np.where(pos >= 0, start[:, None] + pos, 0)].astype(np.int64), -1)
        state["inp"], state["hop"] = dst[dst >= 0], state["hop"] + 1        # row-major = ascending slot
        return pos
    return draw


def run_batch(table, feats, all_ids, all_labels, batch_size, counter, fanout, w=0):
    """The weighted batch `counter` of the list all_ids under draw word w."""
    draw = weighted_positions(table, batch_seeds(all_ids, batch_size, counter), w)
    return D.run_batch(table.indptr, table.indices, feats, all_ids, all_labels, batch_size, counter, fanout, draw=draw)


class Statement:
    """run_batch behind the oracle runner's signature (harness.replay_served); seed=None: unseeded, else tests/seededref.py's draw word
    and shuffled training list."""

    def __init__(self, table, feats, B, fan, seed=None, shuffle=True):
        self.table, self.feats, self.B, self.fan, self.seed, self.shuffle = table, feats, B, list(fan), seed, shuffle

    def run_batch(self, ids, lab, counter, mode=0, batch_size=None, round=0):
        w = 0
        if self.seed is not None:
            import seededref
            w = seededref.W(self.seed, round, counter)
            if mode == seededref.TRAINMODE and self.shuffle:
                ids, lab = seededref.shuffled(ids, lab, self.seed, round)
        return run_batch(self.table, self.feats, ids, lab, self.B if batch_size is None else batch_size, counter, self.fan, w)
