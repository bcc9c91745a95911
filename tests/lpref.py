"""Drawn link-prediction thirds (GPUMemoryPool_SetLpDraw / LEGION_LP_DRAW, INTEGRATION.md "Drawn link-prediction thirds") as a NumPy
statement, shared by the CPU and the GPU tests.  A helper module, not collected by pytest.

All arithmetic is uint32 with wrap-around except the two 64-bit products; mix32, W, Ks and perm are seededref's.  The training list L
(labels Lab) is laid out in batches of 3 k, [src | pos | neg]; list index g = b * 3k + q * k + i is batch b, third q, slot i; triple
t = b * k + i; T = len(L) / 3.

  triple shuffle:  L'[g] = L[(t' // k) * 3k + q * k + t' % k],  t' = perm(t) on [0, T) under Ks(S, r); Lab' likewise
  keys of batch c: Kp = mix32(W ^ 0x4C50504F), Kn = mix32(W ^ 0x4C504E45),  W = W(S, r, c)
  slot i:          src = L'[c * 3k + i];  u(K) = mix32(mix32(K ^ (0x85EBCA6B * (i + 1))) ^ src)
    pos: d = int32(indptr[src + 1] - indptr[src]); d <= 0: src; else rho = (u(Kp) * d) >> 32, pos = indices[indptr[src] + rho], src if pos < 0
    neg: (u(Kn) * V) >> 32
  the batch: ids [src | pos | neg], labels Lab' on the src third and -1 on the drawn slots; everything behind is the seeded statement's
  on these 3 k seeds."""
import numpy as np

import seededref
from distinctref import M32, STEP, mix32, mix32_scalar
from seededref import Ks, W, perm

POS_TAG, NEG_TAG = 0x4C50504F, 0x4C504E45
TRAINMODE = 0


def keys(w):
    """(Kp, Kn) of a batch with draw word w, plain Python ints"""
    w = int(w) & M32
    return mix32_scalar(w ^ POS_TAG), mix32_scalar(w ^ NEG_TAG)


def u(key, i, src):
    """uint32 [n]: the slot's hash under `key` (Kp or Kn): distinctref's u(key, slot) with the source folded in"""
    i = np.asarray(i, dtype=np.int64)
    step = ((STEP * (i + 1)) & M32).astype(np.uint32)
    return mix32(mix32(np.uint32(key) ^ step) ^ (np.asarray(src, dtype=np.int64) & M32).astype(np.uint32))


def _scale(h, n):
    return ((h.astype(np.uint64) * (np.asarray(n, dtype=np.int64) & M32).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def rho(w, i, src, d):
    """int64 [n]: the positive's position in a row of degree d (-1 where d <= 0: the source itself)"""
    d = np.asarray(d, dtype=np.int64)
    return np.where(d > 0, _scale(u(keys(w)[0], i, src), np.maximum(d, 0)), -1)


def neg(w, i, src, V):
    """int64 [n]: the negative, on [0, V)"""
    return _scale(u(keys(w)[1], i, src), V)


def triple_perm_index(n, k, S, r):
    """int64 [n]: the list index L'[g] is read from"""
    n, k = int(n), int(k)
    assert k > 0 and n % (3 * k) == 0
    g = np.arange(n, dtype=np.int64)
    b, rem = g // (3 * k), g % (3 * k)
    q, i = rem // k, rem % k
    t = perm(n // 3, Ks(S, r))[b * k + i]
    return (t // k) * 3 * k + q * k + t % k


def triple_shuffled(L, Lab, k, S, r):
    idx = triple_perm_index(len(L), k, S, r)
    return np.asarray(L)[idx], np.asarray(Lab)[idx]


def draw_batch(indptr, indices, src, w, V):
    """(pos, neg) int64 [k] of a batch whose src third is `src`"""
    src = np.asarray(src, dtype=np.int64)
    i = np.arange(len(src), dtype=np.int64)
    start = np.asarray(indptr)[src]
    d = (np.asarray(indptr)[src + 1] - start).astype(np.int32).astype(np.int64)      # int32 truncation, as k_sample's
    p = rho(w, i, src, d)
    nb = np.asarray(indices)[np.where(p >= 0, start + p, 0)].astype(np.int64) if len(indices) else np.full(len(src), -1, np.int64)
    pos = np.where((p >= 0) & (nb >= 0), nb, src)
    return pos, neg(w, i, src, V)


def drawn_list(indptr, indices, L, Lab, k, V, S, r, shuffle=True):
    """The whole round's list: the triple-shuffled src thirds (file order with shuffle=False) with every batch's pos and neg thirds drawn,
    labels -1 on the drawn slots."""
    L, Lab = np.asarray(L), np.asarray(Lab)
    k = int(k)
    assert k > 0 and len(L) % (3 * k) == 0
    ids, lab = triple_shuffled(L, Lab, k, S, r) if shuffle else (L.copy(), Lab.copy())
    ids, lab = ids.astype(np.int32), lab.astype(np.int32)
    for c in range(len(L) // (3 * k)):
        o = c * 3 * k
        pos, ng = draw_batch(indptr, indices, ids[o:o + k], W(S, r, c), V)
        ids[o + k:o + 2 * k], ids[o + 2 * k:o + 3 * k] = pos, ng
        lab[o + k:o + 3 * k] = -1
    return ids, lab


def toy_list(indptr, V, k, batches, seed=5):
    """A [src | pos | neg] list of `batches` batches of 3 k whose last batch is padded with its first triple, as the generator pads; one
    source repeated, one source with an empty row.  The file's own pos / neg thirds (src + 1, src + 2) are never served under the mode."""
    rng = np.random.RandomState(seed)
    T = batches * k - k // 3                                 # real triples: the last batch is short
    src = rng.permutation(V)[:T].astype(np.int32) if T <= V else rng.randint(0, V, size=T).astype(np.int32)
    src[1] = np.nonzero(np.diff(indptr) == 0)[0][0]
    src[7] = src[3]
    out = np.empty(batches * 3 * k, np.int32)
    for b in range(batches):
        s = src[b * k:(b + 1) * k]
        s = np.concatenate([s, np.full(k - len(s), s[0], np.int32)])
        out[b * 3 * k:(b + 1) * 3 * k] = np.concatenate([s, (s + 1) % V, (s + 2) % V])
    return out


class Statement:
    """seededref.Statement's signature (harness.replay_served): a training batch is seededref.run_batch(..., shuffle=False) on the round's
    drawn list, k = B / 3; validation and test batches are the seeded statement's.  shuffle=False: BeginRound(noder = NULL), the src thirds
    in file order."""

    def __init__(self, indptr, indices, feats, B, fan, seed, sample="replace", shuffle=True):
        assert B % 3 == 0
        self.a, self.B, self.fan, self.seed, self.sample, self.shuffle = (indptr, indices, feats), B, list(fan), seed, sample, shuffle
        self.V = len(indptr) - 1
        self._lists = {}

    def drawn(self, ids, lab, round=0):
        key = (int(round), hash(np.asarray(ids).tobytes()), hash(np.asarray(lab).tobytes()))
        if key not in self._lists:
            self._lists[key] = drawn_list(self.a[0], self.a[1], ids, lab, self.B // 3, self.V, self.seed, round, shuffle=self.shuffle)
        return self._lists[key]

    def run_batch(self, ids, lab, counter, mode=TRAINMODE, batch_size=None, round=0):
        bs = self.B if batch_size is None else batch_size
        if mode == TRAINMODE:
            assert bs == self.B
            ids, lab = self.drawn(ids, lab, round)
        return seededref.run_batch(*self.a, ids, lab, bs, counter, self.fan, sample=self.sample, seed=self.seed, round=round, mode=mode,
                                   shuffle=False)
