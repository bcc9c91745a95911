"""Target-edge exclusion (INTEGRATION.md "Target-edge exclusion": GPUMemoryPool_SetLpExclude), the parts that need no GPU.

The EXPECTED VALUE of the mode is the NumPy statement of tests/lpexref.py.  This file checks what stands around it: the pair table's slot
function through the library against its Python restatement and the documented known answers; the pool's setter on a pool without scratch
-- every refusal by its text with the pool's modes unmoved --; what GPUMemoryPool_ScratchInfo lists before, under and after the mode; that
the inputs of tests/test_gpu_lp_exclude.py exercise what they are meant to (every hop of every batch has an excluded edge, a kept edge
between two seeds and an edge beyond the seeds, and no excluded edge lies beyond the seeds); and the collision case's construction.

Three refusals need a pool with scratch and are asserted in tests/test_gpu_lp_exclude.py: the switch during a capture and the two of
batch_generator_kernel."""
import inspect
import os
import re

import numpy as np
import pytest

import lpexref as X
import scratchpoison as P
from conftest import ROOT

C = X          # the GPU test's cases live beside the statement

NEW_SYMBOLS = ("GPUMemoryPool_SetLpExclude", "GPUMemoryPool_GetLpExclude", "GPUMemoryPool_GetEdgeKeepBuffer", "GPUMemoryPool_GetLpExcludedBuffer",
               "legion_lp_pair_slot")
# INTEGRATION.md "Target-edge exclusion": (lo, hi, cap) -> first slot
KNOWN_SLOTS = {(0, 1, 64): 53, (12, 345, 8192): 3949, (7, 2 ** 31 - 1, 1 << 20): 849294, (2 ** 31 - 1, 2 ** 31 - 1, 1 << 20): 978592}
LP_ROWS = [("lp_pairs", "count_pair", 8, "batch", True), ("edge_keep", "id", 1, "batch", True), ("lp_excluded", "count", 4, "batch", True)]


@pytest.fixture
def pool_lib():
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    L.legion_clear_error()
    pool = L.NewGPUMemoryPool(2)
    yield K, L, pool
    L.legion_clear_error()
    L.GPUMemoryPool_Delete(pool)


def modes(L, pool):
    """(lp_exclude, lp_draw, aggregated, sampling kind)"""
    return (L.GPUMemoryPool_GetLpExclude(pool), L.GPUMemoryPool_GetLpDraw(pool), L.GPUMemoryPool_GetAggLastHop(pool), L.GPUMemoryPool_GetSampling(pool))


def last_error(L):
    msg = (L.legion_last_error() or b"").decode()
    L.legion_clear_error()
    return msg


def listed(K, pool, pipe=0):
    return [(b["name"], b["kind"], b["elem_bytes"], b["lifetime"], b["per_pipe"]) for b in K.pool_scratch(pool, pipe)]


# ---- the slot function ------------------------------------------------------------------------------------------------------------
def test_the_slot_function_equals_its_restatement_and_the_known_answers():
    import legion1_amd.capi as K
    L = K.lib()
    for (lo, hi, cap), want in KNOWN_SLOTS.items():
        assert L.legion_lp_pair_slot(lo, hi, cap) == want == X.pair_slot(lo, hi, cap), (lo, hi, cap)
    rng = np.random.RandomState(11)
    edge = [0, 1, 2, 63, 64, 2 ** 31 - 2, 2 ** 31 - 1]
    cases = [(a, b) for a in edge for b in edge if a <= b] + [tuple(sorted(p)) for p in rng.randint(0, 2 ** 31 - 1, size=(400, 2)).tolist()]
    for cap in (64, 128, 8192, 1 << 20):
        for lo, hi in cases:
            got = L.legion_lp_pair_slot(lo, hi, cap)
            assert got == X.pair_slot(lo, hi, cap) and 0 <= got < cap, (lo, hi, cap)
    assert len({X.pair_slot(lo, hi, 1 << 20) for lo, hi in cases}) > 400                # it spreads
    assert [X.pair_cap(k) for k in (1, 16, 17, 22, 86, 1366, 2666, 7998)] == [64, 64, 128, 128, 512, 8192, 16384, 32768]
    keys = X.pair_keys([5, 9, 0, 7], [9, 5, 0, 2 ** 31 - 1])
    assert keys.tolist() == [(5 << 32) | 9, (5 << 32) | 9, 0, (7 << 32) | (2 ** 31 - 1)] and X.EMPTY not in keys.tolist()


# ---- the pool's mode -----------------------------------------------------------------------------------------------------------------
def test_the_getter_returns_what_was_set_and_no_buffer_is_handed_out(pool_lib):
    K, L, pool = pool_lib
    assert modes(L, pool) == (0, 0, 0, 0) and L.GPUMemoryPool_GetLpExclude(None) == 0 and not L.legion_last_error()
    for k in (22, 0, 1, 86, 86, 1366, 0, 0):
        L.GPUMemoryPool_SetLpExclude(pool, k)
        assert not L.legion_last_error() and modes(L, pool) == (k, 0, 0, 0), k
        assert not L.GPUMemoryPool_GetEdgeKeepBuffer(pool) and not L.GPUMemoryPool_GetLpExcludedBuffer(pool) and not L.legion_last_error()
    for getter in ("GPUMemoryPool_GetEdgeKeepBuffer", "GPUMemoryPool_GetLpExcludedBuffer"):
        assert not getattr(L, getter)(None)
        assert last_error(L).count(getter + ": null pool") == 1


def test_every_refusal_by_its_message_with_the_modes_unmoved(pool_lib):
    K, L, pool = pool_lib
    L.GPUMemoryPool_SetLpExclude(None, 4)
    assert last_error(L).count("GPUMemoryPool_SetLpExclude: null pool") == 1
    negative = "GPUMemoryPool_SetLpExclude: negative triples per batch for target-edge exclusion"
    L.GPUMemoryPool_SetLpExclude(pool, -1)
    assert last_error(L).count(negative) == 1 and modes(L, pool) == (0, 0, 0, 0)
    L.GPUMemoryPool_SetLpExclude(pool, 22)
    L.GPUMemoryPool_SetLpExclude(pool, -(1 << 31))                  # ... and over a mode that is on: the k stays
    assert last_error(L).count(negative) == 1 and modes(L, pool) == (22, 0, 0, 0)
    # drawn thirds of another k, whichever setter comes second
    other = "%s: target-edge exclusion (GPUMemoryPool_SetLpExclude) and drawn link-prediction thirds (GPUMemoryPool_SetLpDraw) with different triples per batch"
    graph = L.NewGPUMemoryGraphStorage()
    L.GPUMemoryPool_SetLpDraw(pool, 23, graph)
    assert last_error(L).count(other % "GPUMemoryPool_SetLpDraw") == 1 and modes(L, pool) == (22, 0, 0, 0)
    L.GPUMemoryPool_SetLpDraw(pool, 22, graph)                      # the same k: both describe the same batch
    assert not L.legion_last_error() and modes(L, pool) == (22, 22, 0, 0)
    L.GPUMemoryPool_SetLpExclude(pool, 21)
    assert last_error(L).count(other % "GPUMemoryPool_SetLpExclude") == 1 and modes(L, pool) == (22, 22, 0, 0)
    L.GPUMemoryPool_SetLpExclude(pool, 0)
    L.GPUMemoryPool_SetLpExclude(pool, 22)                          # off and on again at the thirds' k
    L.GPUMemoryPool_SetLpDraw(pool, 0, None)
    assert not L.legion_last_error() and modes(L, pool) == (22, 0, 0, 0)
    # the aggregated last hop, whichever setter comes second
    agg = "%s: target-edge exclusion (GPUMemoryPool_SetLpExclude) together with the aggregated last hop (GPUMemoryPool_SetAggLastHop): the neighbour sums would contain the excluded draws"
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    assert last_error(L).count(agg % "GPUMemoryPool_SetAggLastHop") == 1 and modes(L, pool) == (22, 0, 0, 0)
    L.GPUMemoryPool_SetLpExclude(pool, 0)
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    L.GPUMemoryPool_SetLpExclude(pool, 22)
    assert last_error(L).count(agg % "GPUMemoryPool_SetLpExclude") == 1 and modes(L, pool) == (0, 0, 1, 0)
    L.GPUMemoryPool_SetAggLastHop(pool, 0)
    L.GPUMemoryPool_SetLpExclude(pool, 22)
    for setter, arg in (("SetSampleDistinct", 1), ("SetSharedDraws", 1), ("SetEdgeIds", 1)):      # every other mode leaves it alone
        getattr(L, "GPUMemoryPool_" + setter)(pool, arg)
    L.GPUMemoryPool_SetSampling(pool, 2)                            # the alias rule: the mode needs no edge ids
    assert "GPUMemoryPool_SetSampling: edge ids" in last_error(L)   # (the edge-id mode's own refusal)
    L.GPUMemoryPool_SetEdgeIds(pool, 0)
    L.GPUMemoryPool_SetSampling(pool, 2)
    assert not L.legion_last_error() and modes(L, pool) == (22, 0, 0, 2)
    L.GPUGraphStorage_Delete(graph)


def test_the_engine_switches_the_mode_off_in_front_of_what_refuses_it():
    """capi.Engine._set_modes: lp_exclude defaults to 0 everywhere, and run_batch / capture_batch / result carry the argument"""
    import legion1_amd.capi as K
    for fn in (K.Engine.run_batch, K.Engine.capture_batch, K.Engine._set_modes):
        assert inspect.signature(fn).parameters["lp_exclude"].default == 0
    assert inspect.signature(K.Engine.result).parameters["lp_exclude"].default is None


# ---- GPUMemoryPool_ScratchInfo ------------------------------------------------------------------------------------------------------------
def test_scratch_info_lists_the_three_buffers_while_the_mode_is_on_and_todays_rows_otherwise(pool_lib):
    """a pool without a device allocates nothing, so it lists the mode's buffers exactly while the mode is on -- at the capacity of its k"""
    K, L, pool = pool_lib
    today = [tuple(t) for t in P.EXPECTED_TABLE]
    assert listed(K, pool) == today                                 # never in the mode
    L.GPUMemoryPool_SetLpExclude(pool, 22)
    for pipe in (0, 1):
        assert listed(K, pool, pipe) == today[:-1] + LP_ROWS + [today[-1]]
    size = lambda: {b["name"]: b["bytes"] for b in K.pool_scratch(pool)}      # noqa: E731
    assert size()["lp_pairs"] == 8 * 128 and size()["lp_excluded"] == 32 and size()["edge_keep"] == L.GPUMemoryPool_NumIds(pool)
    L.GPUMemoryPool_SetLpExclude(pool, 30)                          # the same capacity
    assert size()["lp_pairs"] == 8 * 128
    L.GPUMemoryPool_SetLpExclude(pool, 1366)                        # another one
    assert size()["lp_pairs"] == 8 * 8192 and listed(K, pool) == today[:-1] + LP_ROWS + [today[-1]]
    L.GPUMemoryPool_SetEdgeIds(pool, 1)                             # behind the edge-id rows
    names = [t[0] for t in listed(K, pool)]
    assert names[-6:] == ["edge_ids", "edge_w", "lp_pairs", "edge_keep", "lp_excluded", "ctl"]
    L.GPUMemoryPool_SetEdgeIds(pool, 0)
    L.GPUMemoryPool_SetLpExclude(pool, 0)
    assert listed(K, pool) == today and not L.legion_last_error()
    assert all(r[1] in P.KINDS for r in LP_ROWS) and not set(r[0] for r in LP_ROWS) & set(t[0] for t in P.EXPECTED_TABLE)


# ---- the statement on the GPU test's inputs -------------------------------------------------------------------------------------------------
def test_the_statement_on_hand_made_edges():
    """both directions, every multi-edge, a pair {s, s} matches self-loops of s only, a -1 id is no pair, another level-0 size keeps everything"""
    k, H = 3, 1
    ids = np.array([5, 7, -1, 6, 7, 9, 100, 101, 102, 6, 8], np.int32)      # the pairs {5, 6} and {7, 7}; (-1, 9) is none.  Position 9 holds 6 once more:
    # no batch does that, and the statement, which knows nothing of positions, looks the edge up all the same
    nc = np.zeros(16, np.int32)
    nc[4] = 9
    src = np.array([3, 0, 3, 1, 1, 0, 10, 5, 2, 9], np.int32)              # ids: 6 5 6 7 7 5 8 9 -1 6
    dst = np.array([0, 3, 0, 1, 0, 0, 0, 2, 5, 0], np.int32)               # ids: 5 6 5 7 5 5 5 -1 9 5
    ec = np.zeros(16, np.int32)
    ec[3] = len(src)
    b = dict(nc=nc, ec=ec, ids=ids, src_off=src, dst_off=dst)
    kp, cnt = X.keep(b, k, H)
    assert kp.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 0] and cnt.tolist() == [5, 5, 0, 0, 0, 0, 0, 0]
    nc[4] = 8
    kp, cnt = X.keep(b, k, H)
    assert kp.all() and not cnt.any()


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_every_hop_of_every_gpu_batch_exercises_the_three_kinds_of_edge(case):
    g = C.graph()
    st, L, Lab = C.statement(case, g)
    k, H = case["k"], len(case["fan"])
    for counter in C.COUNTERS:
        batch = st.run_batch(L, Lab, counter)
        census = X.hop_census(batch, k, H)
        for h, (excluded, kept_low, high, excluded_high) in enumerate(census, 1):
            assert excluded >= 1 and kept_low >= 1 and high >= 1 and excluded_high == 0, (counter, h, census)
        kp, cnt = X.keep(batch, k, H)
        assert cnt[0] == (kp == 0).sum() == sum(c[0] for c in census) and not cnt[H + 1:].any()


def test_the_toy_graph_is_what_the_tests_need():
    indptr, indices, feats = C.graph()
    V = len(indptr) - 1
    src = np.repeat(np.arange(V), np.diff(indptr))
    assert X.is_symmetric(indptr, indices) and indptr[V] == indptr[V - 1] and (np.diff(indptr)[:V - 1] > 0).all()      # symmetric, one isolated node
    assert (src == indices).sum() >= 8 and len(np.unique(src * V + indices)) < len(indices)                           # self-loops and multi-edges


# ---- the collision case ---------------------------------------------------------------------------------------------------------------------
def test_the_collision_case_is_what_it_claims():
    c = X.collision_case()
    k, cap, head = c["k"], c["cap"], c["head"]
    assert cap == X.pair_cap(k) == 64 and head == cap - 3
    chain = c["pairs"][:c["chain"]]
    assert len(chain) >= 9 and all(X.pair_slot(lo, hi, cap) == head for lo, hi in chain)
    assert len({v for p in c["pairs"] for v in p}) == 2 * k and np.diff(c["indptr"]).max() <= 4
    keys = X.pair_keys([p[0] for p in c["pairs"]], [p[1] for p in c["pairs"]])
    assert np.array_equal(np.sort(keys), np.sort(X.targets(c["list"], k)))
    seeds = set(c["list"][:2 * k].tolist())
    probe = c["probe"]
    assert probe[0] in seeds and probe[1] in seeds and tuple(probe) not in c["pairs"]
    pk = int(X.pair_keys([probe[0]], [probe[1]])[0])
    for order in (np.arange(k), np.arange(k)[::-1], np.random.RandomState(4).permutation(k)):      # the inserts race: whatever their order
        tab, depth = X.build_table(keys[order], cap)
        run = [(head + j) & (cap - 1) for j in range(len(chain))]
        assert all(int(tab[s]) != X.EMPTY for s in run) and int(tab[(head + len(chain)) & (cap - 1)]) == X.EMPTY
        assert 0 in run and cap - 1 in run                                                           # the chain wraps past the table's end
        assert max(depth[int(x)] for x in keys[:len(chain)]) >= 8
        found, walked = X.lookup_walk(tab, pk)
        assert not found and walked >= 8
        assert all(X.lookup_walk(tab, int(x))[0] for x in keys)
    # the crafted edges are in the graph, in both directions
    indptr, indices = c["indptr"], c["indices"]
    for a, b in c["pairs"] + [probe]:
        assert b in indices[indptr[a]:indptr[a + 1]] and a in indices[indptr[b]:indptr[b + 1]]


def test_header_and_capi_agree_on_the_new_symbols():
    import legion1_amd.capi as K
    header = open(os.path.join(ROOT, "include", "legion_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in K._SIGS and hasattr(K.lib(), name), name
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    n_args = {name: len(re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code).group(1).split(",")) for name in NEW_SYMBOLS}
    assert n_args == {name: len(K._SIGS[name][1]) for name in NEW_SYMBOLS}
    kernels = open(os.path.join(ROOT, "legion-1_amd", "csrc", "lp_exclude.hip")).read()
    assert "k_lp_pairs" in kernels and "k_lp_edge_keep" in kernels
