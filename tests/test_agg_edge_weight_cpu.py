"""Edge-weighted last hop (INTEGRATION.md "Edge-weighted sums": GPUMemoryPool_SetAggEdgeWeight), the parts that need no GPU.

The EXPECTED VALUE of the mode is the NumPy statement of tests/edgeaggref.py (`expected_nbr_sum_edge`) over an eidref.run_batch batch -- never
the code under test.  This file checks the statement's own premises, the trainer's first layer (the fused formula against the edge-wise one
on default batches of tests/drawrulecases.py) and the setter and getter through the library on a pool without scratch: every refusal by its
message with the pool's modes unmoved, the flag surviving the aggregated mode being switched off and on, a null pool."""
import inspect
import os
import re

import numpy as np
import pytest

import drawrulecases as D
import eidref as R
from aggref import cum_edges, expected_nbr_sum
from conftest import ROOT
from edgeaggref import expected_nbr_sum_edge, last_hop_slots


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def g():
    return D.graph()


@pytest.mark.parametrize("tile", list(D.SHAPES))
def test_unit_weights_give_the_plain_statement_bit_for_bit(g, tile):
    """with every weight 1.0 the product is the row itself: S_e is aggref.expected_nbr_sum of the same (default-mode) batch"""
    B, fan = D.SHAPES[tile]
    seeds = D.seed_list(tile)
    ones = dict(g, w=np.ones_like(g["w"]))
    for it in D.COUNTERS:
        ref = R.run_batch(ones, "stream", seeds, g["labels"][seeds], B, it, fan)
        n_in, N, run_dst, S = expected_nbr_sum_edge(ref, g["indptr"], g["indices"], fan)
        p_in, P, p_dst, plain = expected_nbr_sum(ref, g["indptr"], g["indices"], fan)
        assert (n_in, N) == (p_in, P) and N > 0 and np.array_equal(run_dst, p_dst)
        assert S.dtype == np.float32 and np.array_equal(bits(S), bits(plain)) and plain.any()


def test_the_statement_is_the_literal_loop_and_zero_weight_runs_are_plus_zero(g):
    """one hop over the hand-made rows: the vectorised S_e equals the per-run loop in np.float32 scalars (product rounded, then the add); the
    run of the row whose 30 weights are all 0 has draws and sums to +0.0, like the run without draws"""
    fan, B = [4], 64
    seeds = D.seed_list("narrow")
    ref = R.run_batch(g, "stream", seeds, g["labels"][seeds], B, 0, fan)
    n_in, N, run_dst, S = expected_nbr_sum_edge(ref, g["indptr"], g["indices"], fan)
    _, _, _, has, edge = last_hop_slots(ref, g["indptr"], fan)
    assert N == B and list(ref["ids"][:5]) == [D.EMPTY, D.LONG, D.ALL_ZERO, D.HUB, D.HOLES]
    x, e = ref["features"], 0
    for i in range(N):
        acc = np.zeros(D.F, np.float32)
        for j in range(fan[0]):
            if has[i, j]:
                assert edge[i, j] == e
                acc = acc + np.array([np.float32(ref["edge_w"][e]) * np.float32(v) for v in x[ref["src_off"][e]]], np.float32)
                e += 1
        assert np.array_equal(bits(acc), bits(S[i])), i
    assert e == cum_edges(ref["ec"], 1)
    assert has[D.ALL_ZERO].all() and not has[D.EMPTY].any()
    assert not bits(S[D.ALL_ZERO]).any() and not bits(S[D.EMPTY]).any()
    assert (ref["edge_w"] == 0).any() and (ref["edge_w"] > 1).any() and S.any()


@pytest.mark.parametrize("tile", list(D.SHAPES))
def test_the_trainers_fused_first_layer_matches_the_edge_wise_one(g, tile):
    """agg = index_add_(dst_b2, ew_b2[:, None] * x_in[src_b2]) + index_add_(run_dst, S_e) on the served batch against index_add_ of
    ew * x[src] over all of block 1 on the default batch, torch on the CPU.  The bound is derived, with u = 2^-24:
      * per term.  Both sides form t = fl(ew * x) from the same two float32 values with one correct rounding: the terms are identical.
      * per destination v of k(v) terms.  Each side adds those k terms (and exact zeros: index_add_'s start, the +0.0 a run starts from) in an
        order of its own -- edge order there; here slot order inside a run of at most f draws, then the runs, then the edges of the hops < H
        and one add of the two partial results.  A term passes through at most k roundings on either side, so each sum is within g(k) M of
        the exact one, g(k) = k u / (1 - k u), M = sum |t| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: the bound
        holds for any order of the adds).  So |agg - agg'| <= 2 g(k(v)) M(v).
      k(v) <= (runs of v) * f + (edges of the hops < H into v); it is counted from the batch."""
    import torch
    B, fan = D.SHAPES[tile]
    H, f = len(fan), fan[-1]
    seeds = D.seed_list(tile)
    u = 2.0 ** -24
    for it in D.COUNTERS:
        ref = R.run_batch(g, "stream", seeds, g["labels"][seeds], B, it, fan)
        n_in, N, run_dst, S = expected_nbr_sum_edge(ref, g["indptr"], g["indices"], fan)
        e_in, E = cum_edges(ref["ec"], H - 1), cum_edges(ref["ec"], H)
        x = torch.from_numpy(ref["features"])
        src, dst = torch.from_numpy(ref["src_off"][:E].astype(np.int64)), torch.from_numpy(ref["dst_off"][:E].astype(np.int64))
        ew = torch.from_numpy(ref["edge_w"][:E])
        assert int(dst.max()) < n_in and E > e_in
        terms = ew[:, None] * x[src]                                                        # float32: the edge-wise trainer's messages
        edge_wise = torch.zeros(n_in, D.F).index_add_(0, dst, terms)
        x_in = x[:n_in]                                                                     # what the aggregated hand-off serves
        assert e_in == 0 or int(src[:e_in].max()) < n_in
        # where a run's sum goes: the dst_off of its edges.  That is run_dst, except that a seed list which repeats a seed inside a batch (the
        # wide list does) names the seed's LAST occurrence in every edge of its slots (tests/aggref.py has the same rule)
        _, _, _, has, edge = last_hop_slots(ref, g["indptr"], fan)
        one = np.where(has.any(axis=1), edge.max(axis=1), e_in)                             # any edge of the run
        run_node = torch.from_numpy(np.where(has.any(axis=1), ref["dst_off"][one], run_dst).astype(np.int64))
        assert H == 1 or np.array_equal(run_node.numpy(), run_dst)
        fused = torch.zeros(n_in, D.F).index_add_(0, dst[:e_in], ew[:e_in, None] * x_in[src[:e_in]]) + \
            torch.zeros(n_in, D.F).index_add_(0, run_node, torch.from_numpy(S))
        k = torch.bincount(dst, minlength=n_in).double()
        runs_of = torch.bincount(run_node, minlength=n_in).double()
        below = torch.bincount(dst[:e_in], minlength=n_in).double()
        assert bool((k <= runs_of * f + below).all())
        M = torch.zeros(n_in, D.F, dtype=torch.float64).index_add_(0, dst, terms.double().abs())
        gk = (k * u / (1 - k * u)).unsqueeze(1)
        err = (edge_wise.double() - fused.double()).abs()
        assert bool((err <= 2 * gk * M).all()), float((err - 2 * gk * M).max())
        assert float(err.max()) < 1e-4 * float(edge_wise.abs().max()) and float(edge_wise.abs().max()) > 1     # the bound lets no wrong formula through
        plain = torch.zeros(n_in, D.F).index_add_(0, dst, x[src])
        assert float((plain - edge_wise).abs().max()) > 1                                   # ... and the weights matter on this graph


def test_public_surface_carries_the_new_names():
    import legion1_amd.capi as K
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    for name in ("GPUMemoryPool_SetAggEdgeWeight", "GPUMemoryPool_GetAggEdgeWeight"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in K._SIGS, name
    for fn in (K.Engine.run_batch, K.Engine.capture_batch):
        assert inspect.signature(fn).parameters["agg_edge_weight"].default is False
    kernels = open(os.path.join(ROOT, "legion-1_amd", "csrc", "gather.hip")).read()
    assert "k_draw_edge_weights" in kernels


# ---- the setter and the getter on a pool without scratch: no setter touches a device ----------------------------------
@pytest.fixture
def pool_lib():
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    L.legion_clear_error()
    pool = L.NewGPUMemoryPool(2)
    yield L, pool
    L.legion_clear_error()
    L.GPUMemoryPool_Delete(pool)


def modes(L, pool):
    """(aggregated, norm, edge ids, edge-weighted sums, sampling kind, weighted_distinct)"""
    return (L.GPUMemoryPool_GetAggLastHop(pool), L.GPUMemoryPool_GetAggNorm(pool), L.GPUMemoryPool_GetEdgeIds(pool), L.GPUMemoryPool_GetAggEdgeWeight(pool),
            L.GPUMemoryPool_GetSampling(pool), L.GPUMemoryPool_GetWeightedDistinct(pool))


def last_error(L):
    msg = (L.legion_last_error() or b"").decode()
    L.legion_clear_error()
    return msg


NEEDS_AGG = "%s: edge-weighted sums (GPUMemoryPool_SetAggEdgeWeight) on a pool that does not aggregate the last hop (GPUMemoryPool_SetAggLastHop first)"
NEEDS_IDS = "%s: edge-weighted sums (GPUMemoryPool_SetAggEdgeWeight) need edge ids (GPUMemoryPool_SetEdgeIds first, and not off while the flag is on)"
NO_NORM = "%s: edge-weighted sums (GPUMemoryPool_SetAggEdgeWeight) together with a norm (GPUMemoryPool_SetAggNorm)"


def test_the_getter_returns_what_was_set_and_a_null_pool_is_refused(pool_lib):
    L, pool = pool_lib
    assert modes(L, pool) == (0, 0, 0, 0, 0, 0) and L.GPUMemoryPool_GetAggEdgeWeight(None) == 0 and not L.legion_last_error()
    L.GPUMemoryPool_SetAggEdgeWeight(None, 1)
    assert last_error(L).count("GPUMemoryPool_SetAggEdgeWeight: null pool") == 1
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    L.GPUMemoryPool_SetEdgeIds(pool, 1)
    for on, want in ((1, 1), (0, 0), (-7, 1), (1, 1), (0, 0), (0, 0)):
        L.GPUMemoryPool_SetAggEdgeWeight(pool, on)
        assert not L.legion_last_error() and modes(L, pool) == (1, 0, 1, want, 0, 0), on
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 0)                      # off is acceptable anywhere
    L.GPUMemoryPool_SetEdgeIds(pool, 0)
    L.GPUMemoryPool_SetAggLastHop(pool, 0)
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 0)
    assert not L.legion_last_error() and modes(L, pool) == (0, 0, 0, 0, 0, 0)


def test_every_refusal_by_its_message_with_the_modes_unmoved(pool_lib):
    L, pool = pool_lib
    who = "GPUMemoryPool_SetAggEdgeWeight"
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 1)                      # neither the aggregated mode nor edge ids: the aggregated mode is named first
    assert last_error(L).count(NEEDS_AGG % who) == 1 and modes(L, pool) == (0, 0, 0, 0, 0, 0)
    L.GPUMemoryPool_SetEdgeIds(pool, 1)
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 1)                      # edge ids alone
    assert last_error(L).count(NEEDS_AGG % who) == 1 and modes(L, pool) == (0, 0, 1, 0, 0, 0)
    L.GPUMemoryPool_SetEdgeIds(pool, 0)
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 1)                      # the aggregated mode alone
    assert last_error(L).count(NEEDS_IDS % who) == 1 and modes(L, pool) == (1, 0, 0, 0, 0, 0)
    L.GPUMemoryPool_SetEdgeIds(pool, 1)
    L.GPUMemoryPool_SetAggNorm(pool, 1)
    assert not L.legion_last_error() and modes(L, pool) == (1, 1, 1, 0, 0, 0)
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 1)                      # behind a norm: the flag comes second
    assert last_error(L).count(NO_NORM % who) == 1 and modes(L, pool) == (1, 1, 1, 0, 0, 0)
    L.GPUMemoryPool_SetAggNorm(pool, 0)
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 1)
    assert not L.legion_last_error() and modes(L, pool) == (1, 0, 1, 1, 0, 0)
    L.GPUMemoryPool_SetAggNorm(pool, 1)                            # in front of a norm: the norm comes second
    assert last_error(L).count(NO_NORM % "GPUMemoryPool_SetAggNorm") == 1 and modes(L, pool) == (1, 0, 1, 1, 0, 0)
    L.GPUMemoryPool_SetAggNorm(pool, 2)                            # and value 2 of the norm is no way in
    assert "GPUMemoryPool_SetAggNorm: unknown norm (0 = none, 1 = out-degree rsqrt)" in last_error(L) and modes(L, pool) == (1, 0, 1, 1, 0, 0)
    L.GPUMemoryPool_SetEdgeIds(pool, 0)                            # edge ids cannot leave under the flag
    assert last_error(L).count(NEEDS_IDS % "GPUMemoryPool_SetEdgeIds") == 1 and modes(L, pool) == (1, 0, 1, 1, 0, 0)
    L.GPUMemoryPool_SetSampling(pool, 2)                           # the alias rule hands no ids and therefore no sums: the edge-id mode's own refusal
    assert "GPUMemoryPool_SetSampling: edge ids (GPUMemoryPool_SetEdgeIds) cannot be handed over under weighted sampling with replacement" in last_error(L)
    assert modes(L, pool) == (1, 0, 1, 1, 0, 0)
    L.GPUMemoryPool_SetWeightedDistinct(pool, 1)                   # every rule that hands ids over takes the flag
    L.GPUMemoryPool_SetSampling(pool, 2)
    L.GPUMemoryPool_SetSharedDraws(pool, 1)
    L.GPUMemoryPool_SetSampling(pool, 1)
    assert not L.legion_last_error() and modes(L, pool) == (1, 0, 1, 1, 1, 1)


def test_the_flag_survives_the_aggregated_mode_being_switched_off_and_on(pool_lib):
    L, pool = pool_lib
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    L.GPUMemoryPool_SetEdgeIds(pool, 1)
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 1)
    L.GPUMemoryPool_SetAggLastHop(pool, 0)                         # leaves the flag in place ...
    assert not L.legion_last_error() and modes(L, pool) == (0, 0, 1, 1, 0, 0)
    L.GPUMemoryPool_SetSampleDistinct(pool, 1)                     # ... and so does every other setter while the aggregated mode is off
    L.GPUMemoryPool_SetSampleSeed(pool, 1, 3)
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 1)                      # asking for what the pool holds is no change
    assert not L.legion_last_error() and modes(L, pool) == (0, 0, 1, 1, 1, 0)
    L.GPUMemoryPool_SetEdgeIds(pool, 0)                            # remembered or acting, the flag keeps the edge ids
    assert last_error(L).count(NEEDS_IDS % "GPUMemoryPool_SetEdgeIds") == 1 and modes(L, pool) == (0, 0, 1, 1, 1, 0)
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    assert not L.legion_last_error() and modes(L, pool) == (1, 0, 1, 1, 1, 0)
    L.GPUMemoryPool_SetAggLastHop(pool, 0)
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 0)
    L.GPUMemoryPool_SetAggEdgeWeight(pool, 1)                      # once dropped it cannot be asked for again without the aggregated mode
    assert last_error(L).count(NEEDS_AGG % "GPUMemoryPool_SetAggEdgeWeight") == 1 and modes(L, pool) == (0, 0, 1, 0, 1, 0)


def test_the_engine_refuses_the_flag_without_what_it_rests_on():
    """capi.Engine's own argument checks (ValueError, as for agg_norm) are made before the library is called: no engine is needed to see them"""
    import legion1_amd.capi as K
    probe = K.Engine.__new__(K.Engine)
    for kw in (dict(agg=False, edge_ids=True), dict(agg=True, edge_ids=False), dict(agg=False, edge_ids=False)):
        with pytest.raises(ValueError, match="agg_edge_weight needs agg_last_hop=True, edge_ids=True"):
            probe._set_modes(0, kw["agg"], None, "replace", None, 0, None, edge_ids=kw["edge_ids"], agg_edge_weight=True)
    with pytest.raises(ValueError, match="agg_edge_weight and agg_norm together are not in this build"):
        probe._set_modes(0, True, "both", "replace", None, 0, None, edge_ids=True, agg_edge_weight=True)
