"""The edge-id statement (tests/eidref.py) against itself on drawrulecases.graph(), for every rule that hands ids over, both tiles' shapes
and both counters: an id names an edge of the right row with the right neighbour, the rules without replacement give a row distinct ids,
no id points at a hole -- and the graph holds rows whose picks include two columns of ONE neighbour, so a consumer (or a kernel) that
searched the row for the neighbour's id instead of keeping the column would be caught.  No device."""
import numpy as np
import pytest

import drawrulecases as D
import eidref as R


@pytest.fixture(scope="module")
def g():
    return D.graph()


@pytest.fixture(scope="module")
def batches(g):
    """every (rule, tile, counter) once"""
    out = {}
    for rule in R.RULES:
        for tile, (B, fan) in D.SHAPES.items():
            seeds = D.seed_list(tile)
            for it in D.COUNTERS:
                out[(rule, tile, it)] = R.run_batch(g, rule, seeds, g["labels"][seeds], B, it, fan)
    return out


def hop_rows(res):
    """per hop: (the edge range of the hop, the input row of each of its edges)"""
    out, e0 = [], 0
    for h, p in enumerate(res["positions"]):
        has = res["draws"][h].reshape(p.shape) >= 0
        n = int(has.sum())
        out.append((slice(e0, e0 + n), np.repeat(np.arange(len(p)), has.sum(axis=1))))
        e0 += n
    assert e0 == len(res["edge_ids"]) == len(res["src_off"])
    return out


@pytest.mark.parametrize("it", D.COUNTERS)
@pytest.mark.parametrize("tile", list(D.SHAPES))
@pytest.mark.parametrize("rule", R.RULES)
def test_an_id_names_the_edge_it_was_drawn_from(g, batches, rule, tile, it):
    res = batches[(rule, tile, it)]
    eid, ids = res["edge_ids"], res["ids"].astype(np.int64)
    assert len(eid) > 0 and eid.dtype == np.int64
    assert np.array_equal(g["indices"][eid], ids[res["src_off"]])                   # the neighbour the edge names
    u = ids[res["dst_off"]]
    assert ((g["indptr"][u] <= eid) & (eid < g["indptr"][u + 1])).all()            # inside the row of the edge's source
    assert (g["indices"][eid] != -1).all()                                          # never a hole
    assert res["edge_w"].dtype == np.float32 and np.array_equal(res["edge_w"].view(np.uint32), g["w"][eid].view(np.uint32))
    if rule in R.WITHOUT_REPLACEMENT:
        for sl, rows in hop_rows(res):
            pair = np.stack([rows, eid[sl]], axis=1)
            assert len(np.unique(pair, axis=0)) == len(pair)                        # distinct columns per (hop, input slot)
    if rule in ("wdistinct", "wshared"):
        assert (res["edge_w"] > 0).all()                                            # a column of weight 0 is never picked


@pytest.mark.parametrize("rule", R.RULES)
def test_the_holes_row_is_drawn_from_and_gives_no_hole(g, batches, rule):
    """row HOLES is a seed of batch 0 of either shape: its slots that hit a hole are no edge, the others name columns that are none"""
    for tile in D.SHAPES:
        res = batches[(rule, tile, 0)]
        sl, rows = hop_rows(res)[0]
        mine = res["edge_ids"][sl][rows == D.HOLES]
        lo, hi = int(g["indptr"][D.HOLES]), int(g["indptr"][D.HOLES + 1])
        assert ((mine >= lo) & (mine < hi)).all() and not np.isin(mine - lo, (3, 33)).any()
        p = res["positions"][0][D.HOLES]
        assert (p >= 0).sum() >= len(mine) > 0


def test_some_row_picks_two_columns_of_one_neighbour(g, batches):
    """Multi-edges: under a rule without replacement some (hop, row) holds two DIFFERENT ids whose neighbour is the same node.  Searching the
    row for the neighbour would give both edges one id."""
    found = 0
    for rule in R.WITHOUT_REPLACEMENT:
        for tile in D.SHAPES:
            res = batches[(rule, tile, 0)]
            for sl, rows in hop_rows(res):
                eid = res["edge_ids"][sl]
                pair = np.stack([rows, g["indices"][eid].astype(np.int64)], axis=1)
                found += len(pair) - len(np.unique(pair, axis=0))
                assert len(np.unique(np.stack([rows, eid], axis=1), axis=0)) == len(eid)
        assert found > 0, rule


def test_no_near_tie_in_the_weighted_batches(g):
    """the cap on near-tie rows is zero for wdistinct on these shapes (GRAPH_SEED; tests/test_draw_rules_cpu.py asserts the same)"""
    for tile, (B, fan) in D.SHAPES.items():
        seeds = D.seed_list(tile)
        for it in D.COUNTERS:
            ties = []
            R.run_batch(g, "wdistinct", seeds, g["labels"][seeds], B, it, fan, ties=ties)
            assert ties == []


def test_the_statement_is_the_rules_own_batch(g):
    """recording the positions changes nothing: the batch is the one drawrulecases' statement gives"""
    for rule in ("stream", "distinct", "wdistinct"):
        want = D.statement(g, rule, "narrow", 1)
        B, fan = D.SHAPES["narrow"]
        seeds = D.seed_list("narrow")
        got = R.run_batch(g, rule, seeds, g["labels"][seeds], B, 1, fan)
        for k in ("nc", "ec", "ids", "labels", "src_off", "dst_off"):
            assert np.array_equal(want[k], got[k]), (rule, k)
