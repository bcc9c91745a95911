"""What tests/test_gpu_weighted_shared.py and tests/test_weighted_shared_cpu.py share (a helper module, not collected by pytest): the small
graph made for the weighted shared-key resolve, the batches the GPU test runs on it and on drawrulecases.graph(), and the draw words of
those batches.  The CPU test asserts that none of these batches holds a near tie (wsharedref: the cap is zero rows) and that exact ties --
one node at one weight on both sides of the cut -- do occur; the GPU test compares every one of them bit for bit."""
import numpy as np

import drawrulecases as D
import wsharedref as R

# ---- the batches on drawrulecases.graph(): both tiles, counters 0 and 1, draw word 0 and seed 7 (round 0) -----------------------------
SEED = 7
WORDS = (None, SEED)                                # unseeded (draw word 0 through the C ABI) and seeded


def cuts(g, seeds, B, fan, counters, seed):
    """(near ties, exact ties) as [(counter, hop, row)] of the batches `counters` of the training list `seeds` as an Engine or a server runs
    them: unseeded under draw word 0, seeded (round 0) under seededref's draw word over the round's shuffled list"""
    near, exact = [], []
    lab = g["labels"][seeds]
    for it in counters:
        st = R.Statement(g["graph"], np.zeros((len(g["indptr"]) - 1, 1), np.float32), B, fan, seed=seed)
        st.run_batch(seeds, lab, it)
        near.extend((it,) + t for t in st.ties)
        exact.extend((it,) + t for t in st.exact)
    return near, exact


# ---- the graph made by hand -----------------------------------------------------------------------------------------------------------
FANS = ([1, 1, 1], [25, 5, 5], [64, 64])
HB = 128                                            # its batch size: {64, 64} bounds hop 2 by 524 288 slots, the 1024-slot tiles
SPECIAL = [0, 1, 2, 4, 5, 6, 24, 25, 26, 63, 64, 65, 129, 300, 3000, 30, 129, 300, 300, 300, 61]
HOLES, HUB, ALL_ZERO, ONE_WEIGHT, THREE_WEIGHTS, TWENTY_WEIGHTS, LATE_HEAVY, WIDE_RANGE = 12, 14, 15, 16, 17, 18, 19, 20
HV = 1500
TWIN, TWIN_AT, MIXED, MIXED_AT = 77, 100, 78, 200  # the hub's two runs of forty columns that hold one id each


def hand_made_graph(seed):
    """1500 nodes.  Rows 0..20 by hand: the degrees d = 0, 1, f - 1, f, f + 1 of every fan-out of the tests (1, 5, 25, 64), 129 and 300
    (three and five chunks of 64 columns), a hub of 3000, an all-zero row of 30, rows of 129 / 300 / 300 columns of which 1 / 3 / 20 carry
    weight (m <= f < d), a row of 300 whose heavy columns are its last 44 (the last chunk only), a row of weights from 1e-30 to 1e30; the
    others 0..40 neighbours.  Weights: 0 (one in five) or 1..16.  Random neighbours, so multi-edges throughout.  The hub holds node TWIN in
    forty columns of ONE weight, 4096 times the heaviest other: forty bit-equal keys in front of nearly every other, which the cut falls
    among at every fan-out below 40 (exact ties); and node MIXED in forty columns of weights 64, 128, .. 2560: one uniform, forty different keys, several of
    which may be picked.  Row HOLES has -1 holes with weight.  seed: of the random part."""
    rng = np.random.RandomState(7700 + seed)
    deg = rng.randint(0, 41, size=HV)
    deg[:len(SPECIAL)] = SPECIAL
    indptr = np.zeros(HV + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    indices = rng.randint(0, HV, size=E).astype(np.int32)
    w = np.where(rng.rand(E) < 0.2, 0, rng.randint(1, 17, size=E)).astype(np.float32)
    row = lambda v: slice(int(indptr[v]), int(indptr[v + 1]))
    w[row(1)] = 1.0
    w[row(ALL_ZERO)] = 0.0
    for v, cols in ((ONE_WEIGHT, [7]), (THREE_WEIGHTS, [0, 64, 128]), (TWENTY_WEIGHTS, list(range(3, 300, 15)))):
        w[row(v)] = 0.0
        w[indptr[v] + np.array(cols)] = 2.0
    w[row(LATE_HEAVY)] = 1.0
    w[indptr[LATE_HEAVY] + 256:indptr[LATE_HEAVY] + 300] = 1e6
    w[row(WIDE_RANGE)] = (10.0 ** np.linspace(-30, 30, 61)).astype(np.float32)
    hub = int(indptr[HUB])
    indices[hub + TWIN_AT:hub + TWIN_AT + 40], w[hub + TWIN_AT:hub + TWIN_AT + 40] = TWIN, 65536.0
    indices[hub + MIXED_AT:hub + MIXED_AT + 40], w[hub + MIXED_AT:hub + MIXED_AT + 40] = MIXED, 64.0 * np.arange(1, 41, dtype=np.float32)
    indices[indptr[HOLES] + 3], indices[indptr[HOLES] + 70] = -1, -1
    w[indptr[HOLES] + 3], w[indptr[HOLES] + 70] = 16.0, 16.0
    labels = rng.randint(0, 9, size=HV).astype(np.int32)
    n = len(SPECIAL)
    seeds = np.concatenate([np.arange(n), n + np.random.RandomState(2).permutation(HV - n)[:353]]).astype(np.int32)   # the special rows once, in batch 0
    feats = np.random.RandomState(1).rand(HV, 4).astype(np.float32)
    return dict(V=HV, F=4, indptr=indptr, indices=indices, w=w, labels=labels, feats=feats, seeds=seeds, graph=R.Weights(indptr, indices, w))


def hand_counters(g):
    """the first batch (every special row) and the last, which is short"""
    assert len(g["seeds"]) % HB != 0
    return (0, (len(g["seeds"]) - 1) // HB)


def hand_near_ties(g):
    """every near tie of every batch the GPU test runs on the hand-made graph"""
    return [(tuple(fan), seed) + t for fan in FANS for seed in WORDS for t in cuts(g, g["seeds"], HB, fan, hand_counters(g), seed)[0]]


# The seed of the hand-made graph's random part, chosen as drawrulecases.GRAPH_SEED was: the first of 0, 1, 2, ... that leaves no near tie
# in any batch the GPU test runs, which tests/test_weighted_shared_cpu.py asserts.
HAND_SEED = 0


def rule_graph():
    """drawrulecases.graph() as the statement's graph type, with its arrays"""
    g = D.graph()
    return dict(g, graph=R.Weights(g["indptr"], g["indices"], g["w"]))
