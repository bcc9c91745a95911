"""Seeded sampling (GPUMemoryPool_SetSampleSeed / LEGION_SAMPLING_SEED, INTEGRATION.md "Seeded sampling") as a NumPy statement, shared by
the CPU and the GPU tests.  A helper module, not collected by pytest.

All arithmetic is uint32 with wrap-around unless said otherwise; mix32 is distinctref's.  S = the seed, r = the round, c = the iter
(batch_generator_kernel's `counter`):

  Ks = mix32(mix32(S ^ 0x53485546) ^ r)                       the shuffle key of the round
  W  = mix32(mix32(mix32(S ^ 0x44524157) ^ r) ^ c)            the draw word of the batch

  shuffle (training lists): perm on [0, n).  n <= 1: identity.  Else b = bit_length(n - 1) rounded up to even, h = b / 2, m = (1 << h) - 1;
    x = g; repeat { L = x >> h, R = x & m; four rounds q = 0..3: (L, R) = (R, L ^ (mix32(R ^ mix32(Ks + q * 0x9E3779B9)) & m));
    x = (L << h) | R } until x < n.  The seed at list index g of round r is ids[perm(g)].
  replace:  s_b = 1 + W % 2147483646;  x(idx) = s_b * 48271^(idx + 1) mod (2^31 - 1);  position = pyref.sample_index's fp64 arithmetic on x
  distinct: the row key becomes K = mix32((i + 0x9E3779B9 * h) ^ W); everything behind it is distinctref's.

Mode off (seed=None below): s_b = 1, W = 0, identity perm."""
import numpy as np

import distinctref
from distinctref import GOLDEN, M32, STEP, mix32, mix32_scalar

M31 = 2147483647
SHUFFLE_TAG, DRAW_TAG = 0x53485546, 0x44524157
TRAINMODE = 0


# ---- keys (plain Python ints) --------------------------------------------------------------------
def Ks(S, r):
    S, r = int(S), int(r)
    return mix32_scalar(mix32_scalar((S ^ SHUFFLE_TAG) & M32) ^ (r & M32))


def W(S, r, c):
    S, r, c = int(S), int(r), int(c)
    return mix32_scalar(mix32_scalar(mix32_scalar((S ^ DRAW_TAG) & M32) ^ (r & M32)) ^ (c & M32))


def s_b(w):
    return 1 + (int(w) & M32) % 2147483646


# ---- the shuffle -----------------------------------------------------------------------------------
def perm_scalar(g, n, ks):
    if n <= 1:
        return g
    b = (n - 1).bit_length()
    b += b & 1
    h = b // 2
    m = (1 << h) - 1
    rk = [mix32_scalar((ks + q * GOLDEN) & M32) for q in range(4)]
    x = g
    while True:
        L, R = x >> h, x & m
        for q in range(4):
            L, R = R, L ^ (mix32_scalar(R ^ rk[q]) & m)
        x = (L << h) | R
        if x < n:
            return x


def perm(n, ks):
    """int64 [n]: perm(0 .. n - 1), vectorised (the cycle walk repeats on the entries still outside [0, n))."""
    n = int(n)
    if n <= 1:
        return np.arange(n, dtype=np.int64)
    b = (n - 1).bit_length()
    b += b & 1
    h = np.uint32(b // 2)
    m = np.uint32((1 << (b // 2)) - 1)
    rk = [np.uint32(mix32_scalar((ks + q * GOLDEN) & M32)) for q in range(4)]
    x = np.arange(n, dtype=np.uint32)
    todo = np.arange(n)
    while len(todo):
        v = x[todo]
        L, R = v >> h, v & m
        for q in range(4):
            L, R = R, L ^ (mix32(R ^ rk[q]) & m)
        v = (L << h) | R
        x[todo] = v
        todo = todo[v >= n]
    return x.astype(np.int64)


# ---- draws -----------------------------------------------------------------------------------------
def _mulmod31(a, b):
    return (a * b) % np.uint64(M31)          # both < 2^31: the product fits uint64


def minstd_values(idx, sb=1):
    """uint64 [n]: sb * 48271^(idx + 1) mod (2^31 - 1) by repeated squaring on whole arrays."""
    e = np.asarray(idx, dtype=np.uint64) + np.uint64(1)
    res = np.full(e.shape, int(sb) % M31, dtype=np.uint64)
    base = np.uint64(48271)
    while e.any():
        odd = (e & np.uint64(1)).astype(bool)
        res = np.where(odd, _mulmod31(res, base), res)
        base = _mulmod31(base, base)
        e = e >> np.uint64(1)
    return res


def replace_index(idx, deg, w=0):
    """int64 [n]: the neighbour position slot idx draws at degree deg under draw word w (fp64 exactly as thrust's uniform_int_distribution)."""
    x = minstd_values(idx, s_b(w))
    r = (x - np.uint64(1)).astype(np.float64) / np.float64(2147483646.0)
    return (r * np.asarray(deg, dtype=np.float64) + np.float64(0.0)).astype(np.int64)


def replace_positions(w):
    """A `draw` for distinctref.run_batch: the with-replacement stream seeded by draw word w (w = 0: the reference's)."""
    def draw(rows, hop, deg, f):
        rows = np.asarray(rows, dtype=np.int64)
        deg = np.asarray(deg, dtype=np.int64)
        j = np.arange(int(f), dtype=np.int64)
        idx = rows[:, None] * int(f) + j[None, :]
        has = j[None, :] < deg[:, None]
        k = replace_index(idx.reshape(-1), np.where(has, deg[:, None], 1).reshape(-1), w).reshape(idx.shape)
        return np.where(has, k, -1)
    return draw


def picks_scalar(i, h, d, f, w=0):
    if d <= f:
        return [j if j < d else -1 for j in range(f)]
    K = mix32_scalar(((i + GOLDEN * h) & M32) ^ w)
    pick = []
    for t in range(f):
        J = d - f + t
        u = mix32_scalar(K ^ ((STEP * (t + 1)) & M32))
        r = (u * (J + 1)) >> 32
        pick.append(J if r in pick else r)
    return pick


def distinct_positions(w):
    """A `draw` for distinctref.run_batch: distinctref.positions with w XORed into the row key."""
    def draw(rows, hop, deg, f):
        rows = np.asarray(rows, dtype=np.int64)
        deg = np.asarray(deg, dtype=np.int64)
        hop = np.broadcast_to(np.asarray(hop, dtype=np.int64), rows.shape)
        f = int(f)
        j = np.arange(f, dtype=np.int64)
        out = np.where(j[None, :] < deg[:, None], j[None, :], -1)
        big = np.nonzero(deg > f)[0]
        if len(big):
            d = deg[big]
            K = mix32(((rows[big] + GOLDEN * hop[big]) & M32).astype(np.uint32) ^ np.uint32(w))
            pick = np.empty((len(big), f), dtype=np.int64)
            for t in range(f):
                J = d - f + t
                u = mix32(K ^ np.uint32((STEP * (t + 1)) & M32))
                r = ((u.astype(np.uint64) * (J + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
                hit = (pick[:, :t] == r[:, None]).any(axis=1) if t else np.zeros(len(big), bool)
                pick[:, t] = np.where(hit, J, r)
            out[big] = pick
        return out
    return draw


# ---- the whole batch -------------------------------------------------------------------------------
def shuffled(all_ids, all_labels, seed, rnd):
    p = perm(len(all_ids), Ks(seed, rnd))
    return np.asarray(all_ids)[p], np.asarray(all_labels)[p]


def run_batch(indptr, indices, feats, all_ids, all_labels, batch_size, counter, fanout, sample="replace", seed=None, round=0,
              mode=TRAINMODE, shuffle=True):
    """The batch (seed, round, counter) of `mode`'s list all_ids: distinctref.run_batch fed with the seeded draw and, for a training list,
    the round's shuffled list.  seed=None: the mode off."""
    w = 0 if seed is None else W(seed, round, counter)
    if seed is not None and mode == TRAINMODE and shuffle:
        all_ids, all_labels = shuffled(all_ids, all_labels, seed, round)
    draw = distinct_positions(w) if sample == "distinct" else replace_positions(w)
    return distinctref.run_batch(indptr, indices, feats, all_ids, all_labels, batch_size, counter, fanout, draw=draw)


class Statement:
    """run_batch behind the oracle runner's signature (harness.replay_served), for one seed and sampler mode; `round` per call.
    shuffle=False: training lists served verbatim (meta flag 2)."""

    def __init__(self, indptr, indices, feats, B, fan, seed, sample="replace", shuffle=True):
        self.a, self.B, self.fan, self.seed, self.sample, self.shuffle = (indptr, indices, feats), B, list(fan), seed, sample, shuffle

    def run_batch(self, ids, lab, counter, mode=TRAINMODE, batch_size=None, round=0):
        return run_batch(*self.a, ids, lab, self.B if batch_size is None else batch_size, counter, self.fan, sample=self.sample,
                         seed=self.seed, round=round, mode=mode, shuffle=self.shuffle)
