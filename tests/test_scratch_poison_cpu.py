"""tests/scratchpoison.py held to its rules for every kind, GPUMemoryPool_ScratchInfo's list against a literal copy (fresh, and through the
modes' life cycle of tests/poolpipes.py), and the near-tie cap
of zero rows on the exact batches tests/test_gpu_scratch_poison.py compares for the two weighted rules without replacement.  No device."""
import ctypes as C

import numpy as np
import pytest

import poolpipes as W
import scratchpoison as P
import wsharedcases


class FakeDecoy:
    V, pitch, base = 50, 8, 0x7000_0000_0000

    def rows(self, r):
        return np.uint64(self.base) + np.asarray(r, dtype=np.uint64) * np.uint64(4 * self.pitch)


def test_the_enumerator_lists_every_buffer_with_a_lifetime():
    """A pool that never saw a device: the list is host state.  Names, kinds, element sizes, lifetimes and per-pipe flags are the literal
    table; every pipe of the pool reports it; a pipe the pool does not have, a negative index and null arguments are refused."""
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    pool = L.NewGPUMemoryPool(2)
    try:
        for pipe in (0, 1):
            got = K.pool_scratch(pool, pipe)
            assert [(b["name"], b["kind"], b["elem_bytes"], b["lifetime"], b["per_pipe"]) for b in got] == P.EXPECTED_TABLE
            assert all(b["ptr"] is None for b in got)                       # nothing is allocated yet
        assert len({t[0] for t in P.EXPECTED_TABLE}) == len(P.EXPECTED_TABLE)
        assert [t[0] for t in P.EXPECTED_TABLE if t[3] == "state"] == ["ctl"] and [t[0] for t in P.EXPECTED_TABLE if t[3] == "table"] == ["pos_map"]
        info = K.LegionScratchInfo()
        assert L.GPUMemoryPool_ScratchInfo(pool, len(P.EXPECTED_TABLE), 0, C.byref(info)) == 1      # past the end: no error
        assert not L.legion_last_error()
        for args in ((pool, 0, 2, C.byref(info)), (pool, -1, 0, C.byref(info)), (pool, 0, 0, None), (None, 0, 0, C.byref(info))):
            assert L.GPUMemoryPool_ScratchInfo(*args) == -1
            assert b"GPUMemoryPool_ScratchInfo" in (L.legion_last_error() or b"")
            L.legion_clear_error()
    finally:
        L.legion_clear_error()
        L.GPUMemoryPool_Delete(pool)


# GPUMemoryPool_ScratchInfo's list of a pool that never saw a device, with its bytes (V, num_ids, max_slots and max_tiles are all 0), recorded
# from the library before the per-pipe buffers became one table: while the edge-id mode is off ...
LISTED = [
    ("pos_map", "table_entry", 8, "table", False, 0),
    ("cand", "id", 4, "hop", False, 0),
    ("aux2[0]", "slot_state", 4, "batch", False, 0),
    ("aux2[1]", "slot_state", 4, "batch", False, 0),
    ("tile_edge", "count", 4, "hop", False, 4),
    ("tile_node", "count", 4, "hop", False, 4),
    ("tile_pre", "count_pair", 8, "hop", False, 8),
    ("chunk_tot", "count_pair", 8, "hop", False, 16384),
    ("hop_state", "count", 4, "hop", False, 32),
    ("cache_search_buffer", "id", 4, "batch", False, 0),
    ("row_ptr", "device_pointer", 8, "batch", False, 0),
    ("agg_src_ids", "id", 4, "batch", False, 0),
    ("tmp_part_ind", "id", 1, "batch", False, 0),
    ("tmp_part_off", "id", 4, "batch", False, 0),
    ("cand_pipe", "id", 4, "batch", True, 0),
    ("agg_out_deg", "count", 4, "batch", True, 0),
    ("agg_wdraw", "float", 4, "batch", True, 0),
    ("agg_chunk_cnt", "count", 4, "batch", True, 8192),
    ("ctl", "count", 4, "state", False, 20),
]
# ... and while it is on: cols behind tmp_part_off, edge_ids and edge_w behind agg_chunk_cnt
LISTED_EDGE_IDS = [
    ("pos_map", "table_entry", 8, "table", False, 0),
    ("cand", "id", 4, "hop", False, 0),
    ("aux2[0]", "slot_state", 4, "batch", False, 0),
    ("aux2[1]", "slot_state", 4, "batch", False, 0),
    ("tile_edge", "count", 4, "hop", False, 4),
    ("tile_node", "count", 4, "hop", False, 4),
    ("tile_pre", "count_pair", 8, "hop", False, 8),
    ("chunk_tot", "count_pair", 8, "hop", False, 16384),
    ("hop_state", "count", 4, "hop", False, 32),
    ("cache_search_buffer", "id", 4, "batch", False, 0),
    ("row_ptr", "device_pointer", 8, "batch", False, 0),
    ("agg_src_ids", "id", 4, "batch", False, 0),
    ("tmp_part_ind", "id", 1, "batch", False, 0),
    ("tmp_part_off", "id", 4, "batch", False, 0),
    ("cols", "count", 4, "hop", False, 0),
    ("cand_pipe", "id", 4, "batch", True, 0),
    ("agg_out_deg", "count", 4, "batch", True, 0),
    ("agg_wdraw", "float", 4, "batch", True, 0),
    ("agg_chunk_cnt", "count", 4, "batch", True, 8192),
    ("edge_ids", "count_pair", 8, "batch", True, 0),
    ("edge_w", "float", 4, "batch", True, 0),
    ("ctl", "count", 4, "state", False, 20),
]
LISTED_AT = {"fresh": LISTED, "edge ids on": LISTED_EDGE_IDS, "edge ids off": LISTED, "aggregated last hop": LISTED, "norm": LISTED,
             "edge-weighted sums": LISTED_EDGE_IDS, "everything off": LISTED}


def test_the_list_through_the_modes_life_cycle_without_a_device():
    """A pool of depth 2 that never saw a device allocates nothing, whatever mode is set: every pointer stays null, and the list is the literal
    table except while the edge-id mode is on -- without cols there is nothing that remembers the mode once it is off again.  No setter
    leaves an error (poolpipes.walk asserts it behind each)."""
    import legion1_amd.capi as K
    L = K.lib()
    L.legion_set_error_mode(K.ERR_RETURN)
    assert [t[:5] for t in LISTED] == P.EXPECTED_TABLE and [s[0] for s in W.STEPS] == list(LISTED_AT)
    pool = L.NewGPUMemoryPool(2)
    try:
        for step in W.walk(K, pool):
            for pipe in (0, 1):
                rows, ptrs = W.listed(K, pool, pipe)
                assert rows == LISTED_AT[step], (step, pipe)
                assert all(v is None for v in ptrs.values()), (step, pipe, ptrs)
            assert not L.legion_last_error()
    finally:
        L.legion_clear_error()
        L.GPUMemoryPool_Delete(pool)


@pytest.mark.parametrize("fill", P.FILLS)
@pytest.mark.parametrize("kind,elem", sorted({(t[1], t[2]) for t in P.EXPECTED_TABLE}))      # every (kind, element size) the pool holds
def test_every_kind_keeps_the_safe_fill_rules(kind, elem, fill):
    rng = np.random.RandomState(5)
    n, V, slots, tile, budget, epoch = 4099, 3000, 1500, 256, 700, P.EPOCH_TOP - 9
    avoid = np.arange(0, V, 2)
    a = P.generate(kind, n * elem, elem, rng, fill, limit=V, avoid=avoid, slots=slots, tile=tile, budget=budget, epoch=epoch, decoy=FakeDecoy())
    assert a.nbytes == n * elem and a.flags["C_CONTIGUOUS"]
    raw = np.frombuffer(a.tobytes(), np.uint8)
    if kind == "device_pointer":                              # NULL or the start of a decoy row, whatever the fill
        p = a.astype(np.uint64)
        off = (p[p != 0] - np.uint64(FakeDecoy.base)).astype(np.int64)
        assert (p == 0).any() and (p != 0).any() and (off % (4 * FakeDecoy.pitch) == 0).all() and (off // (4 * FakeDecoy.pitch) < FakeDecoy.V).all() and (off >= 0).all()
        assert not np.isin(raw.view(np.uint64), [0xFFFFFFFFFFFFFFFF, 0xA5A5A5A5A5A5A5A5]).any()
        assert not P.generate(kind, 64, 8, rng, fill).any()   # without a decoy: NULL only
        return
    if fill == "ones":
        assert (raw == 0xFF).all()
        return
    if fill == "zero" and kind != "table_entry":
        assert not raw.any()
        return
    if kind == "id":
        v = a.astype(np.int64)
        top = min(V, 127) if elem == 1 else V
        assert ((v == -1) | ((v >= 0) & (v < top))).all() and (v == -1).any() and (v >= 0).any()
        assert not np.isin(v[v >= 0], avoid).any()            # none of the batch's ids
        all_in = P.generate("id", 400, 4, rng, limit=10, avoid=np.arange(10))
        assert ((all_in >= -1) & (all_in < 10)).all()         # a batch that holds every node: any id
    elif kind == "slot_state":
        v, i = a.astype(np.int64), np.arange(n)
        lost = v != -1
        assert v[0] == -1 and (v == -1).sum() > n // 5 and lost.sum() > n // 2
        s = -2 - v[lost]
        assert (s >= 0).all() and (s < slots).all() and (s < i[lost]).all()       # inside the hop, and every chain descends
        assert (v > -2 - 0x40000000).all()                                        # no winner rank (enc_win): a loser's link only
    elif kind in ("count", "count_pair"):
        v = a.reshape(n, -1).astype(np.int64)
        assert (v >= 0).all() and (v <= tile).all() and (v.sum(axis=0) <= budget).all() and (v.sum(axis=0) >= budget // 2).all()
        assert (v.max(axis=0) > 1).all() or budget < 4
    elif kind == "float":
        assert (a.view(np.uint32) == P.NAN_BITS).all() and np.isnan(a.view(np.float32)).all()
    else:
        e, v = (a >> np.uint64(32)).astype(np.int64), (a & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert (e > epoch).all() and (e <= P.EPOCH_TOP).all() and len(np.unique(e)) > 3
        assert (v & P.PROVISIONAL).astype(bool).any() and (v < budget * 4).any() and (v > P.PROVISIONAL).any()


def test_table_entries_right_behind_the_first_batch_have_one_epoch():
    """the first batch of a pool runs under kEpochTop - 1: the only stale epoch is kEpochTop itself"""
    a = P.generate("table_entry", 800, 8, np.random.RandomState(1), epoch=P.EPOCH_TOP - 1)
    assert ((a >> np.uint64(32)) == P.EPOCH_TOP).all()


def test_the_sequence_reaches_what_it_is_meant_to():
    """list entry 0 has no neighbour, entry 1 has more than either shape's first fan-out; the wide shape's hop 2 is the wide tile's"""
    g = wsharedcases.rule_graph()
    deg = np.diff(g["indptr"])
    for tile, (B, fan) in P.SHAPES.items():
        seeds = P.seed_list(tile)
        assert seeds[0] == P.EMPTY and deg[P.EMPTY] == 0 and seeds[1] == P.LONG and deg[P.LONG] > max(fan)
        assert B < len(seeds) < 2 * B
        bound = B * int(np.prod(fan[:2]))
        assert (bound > P.NARROW_SLOTS) == (tile == "wide")
    assert [s[1] for s in P.SEQUENCE] == [None, 1, 1, None, None] and len({s[2] for s in P.SEQUENCE}) == len(P.FILLS)


@pytest.mark.parametrize("tile", list(P.SHAPES))
@pytest.mark.parametrize("rule", ["wdistinct", "wshared"])
def test_no_near_tie_in_any_compared_batch(rule, tile):
    """the cap is zero rows: weighted draws without replacement are compared bit for bit on every row of every batch of the sequence"""
    g = wsharedcases.rule_graph()
    st = P.statement(rule, dict(g, feats=np.zeros((len(g["indptr"]) - 1, 1), np.float32)), tile)
    seeds = P.seed_list(tile)
    for counter, bs in dict.fromkeys(s[:2] for s in P.SEQUENCE):
        st.run_batch(seeds, g["labels"][seeds], counter, batch_size=bs)
    assert st.ties == []
