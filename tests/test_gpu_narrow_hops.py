"""The sampler picks the tile of a hop's three passes (k_sample, k_mark, k_write) from the hop's static slot bound, batch x fan-outs so
far: at most kNarrowSlots = 256 Ki slots -> 256-slot tiles, one slot per thread; above -> 1024-slot tiles (csrc/internal.h).  The RNG
stream, the claims and every rank are indexed by slot, so a batch must not depend on which tile a hop ran.

Parity cases in the style of tests/test_gpu_full_shape.py -- every buffer of every batch word for word against the oracle -- with hop
bounds on either side of the switch: exactly at it, one seed above it, narrow hops followed by wide ones, and the switch inside a batch.
The small shapes of the other parity tests all run narrow tiles only, the full shapes wide tiles on every hop but the first."""
import numpy as np
import pytest

from conftest import assert_batch_equal
from harness import K  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu

NARROW_SLOTS = 256 * 1024      # kNarrowSlots (csrc/internal.h)


@pytest.fixture(scope="module")
def graph():
    """60 k nodes, geometric degrees with hubs of 50-400 neighbours, half of all edges pointing at a hub (many claims of one node inside a
    hop: replaced claims and loser -> winner chains across tiles), isolated nodes and -1 entries."""
    rng = np.random.RandomState(4242)
    V, F = 60000, 8
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
    return V, F, indptr, nbr.astype(np.int32), feats, labels


def hop_bounds(B, fan):
    out, cur = [], B
    for f in fan:
        cur *= f
        out.append(cur)
    return out


# (batch, fan-outs, which hops run narrow tiles, seeds drawn with repetition)
CASES = [
    (8192, [32], [True], False),                     # exactly kNarrowSlots: the last bound that runs narrow
    (8193, [32], [False], False),                    # one seed more: wide
    (4096, [64], [True], True),                      # the same bound from a fan-out above most degrees (padded slots), repeated seeds
    (4097, [64], [False], True),
    (8192, [32, 3], [True, False], False),           # narrow hop feeding a wide one
    (1024, [16, 16, 2], [True, True, False], True),  # hop 2 exactly at the bound, hop 3 above it
    (4096, [64, 1], [True, True], False),            # two narrow hops at the bound
    (8000, [25, 3, 2], [True, False, False], False), # hop 1 of the headline shape, then wide hops
]


@pytest.mark.parametrize("B,fan,narrow,repeated", CASES)
def test_batches_do_not_depend_on_the_tile_of_a_hop(K, oracle, graph, B, fan, narrow, repeated):
    V, F, indptr, indices, feats, labels = graph
    assert [b <= NARROW_SLOTS for b in hop_bounds(B, fan)] == narrow
    rng = np.random.RandomState(B + len(fan))
    n_seeds = 2 * B + B // 3                                          # two full batches and a short one
    seeds = (rng.randint(0, V, size=n_seeds) if repeated else rng.permutation(V)[:n_seeds]).astype(np.int32)
    lab = labels[seeds]
    orc = oracle.OracleRunner(indptr, indices, feats, V, F, B, fan)
    eng = K.Engine(indptr, indices, feats, V, F, dict(train=[(seeds, lab)]), B, fan)
    eng.alloc_features()
    for counter in (0, 1, 2, 0):
        ref = orc.run_batch(seeds, lab, counter)
        eng.run_batch(0, counter)
        assert_batch_equal(ref, eng.result(0))
        assert ref["ec"][2 + len(fan)] > 0
    eng.close()
