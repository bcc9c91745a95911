"""What tests/widthcases.py claims, proven without a GPU: every width takes the path and the chunk count its table row states, the table's
words name their element, the oracle's batches put rows across the wave and workgroup edges the reason column speaks of, the cached
configurations meet their floors at the forced capacities, and assert_rows tells the ways a lane-to-row mapping goes wrong apart."""
import numpy as np
import pytest

import widthcases as W


@pytest.fixture(scope="module")
def rows_per_batch(oracle):
    """rows of the batches every gather test uses: a batch's structure does not depend on the row width"""
    return {it: len(w["ids"]) for it, w in W.plain_batches(oracle, 4).items()}


def test_the_batches_are_a_first_a_middle_and_a_short_last_one(oracle, rows_per_batch):
    seeds = W.seed_lists(1)[0]
    assert len(seeds) == W.N_SEEDS == 2 * W.B + 8 and len(set(seeds.tolist())) == len(seeds)
    want = W.plain_batches(oracle, 4)
    assert [int(want[it]["nc"][4]) for it in W.BATCHES] == [W.B, W.B, 8]
    assert all(40 <= n <= W.ROWS_MAX < 1024 for n in rows_per_batch.values()), rows_per_batch
    g = W.graph()
    deg = np.diff(g["indptr"])
    assert deg.min() == 0 and deg[g["hub"]] == deg.max() == 60 and (g["indices"] < 0).sum() >= 5
    assert any(len(set(g["indices"][a:b].tolist())) < b - a for a, b in zip(g["indptr"][:-1], g["indptr"][1:]))       # multi-edges
    assert g["hub"] in want[0]["ids"][:W.B]


def test_widths_cover_the_listed_chunk_counts():
    assert sorted(w.C for w in W.ALIGNED if w.path == "vec") == [1, 2, 3, 25, 32, 63, 64, 65, 129, 257]
    assert sorted(w.C for w in W.ALIGNED if w.path == "scalar") == [1, 2, 3, 7, 63, 65, 127, 129, 257]
    assert [(w.F, w.C) for w in W.FORCED] == [(64, 64), (256, 256)]
    assert len({W.width_id(w) for w in W.WIDTHS}) == len(W.WIDTHS)


@pytest.mark.parametrize("w", W.WIDTHS, ids=W.width_id)
def test_path_chunks_and_pitch_follow_from_the_width(w):
    import legion1_amd.capi as K
    assert W.path_of(w.F, aligned=not w.forced) == w.path and W.chunks_per_row(w.F, aligned=not w.forced) == w.C
    if w.forced:
        assert w.F % 4 == 0 and W.path_of(w.F) == "vec"            # only the destination's alignment sends it down the scalar path
    pitch = W.row_pitch(w.F)
    assert pitch >= w.F and pitch % 32 == 0 and pitch - w.F < 32
    assert K.lib().legion_row_pitch(w.F) == pitch
    assert W.shard_chunk_bytes(w.F) == pitch * 4 * W.CHUNK_ROWS


@pytest.mark.parametrize("w", W.ALIGNED, ids=W.width_id)
def test_table_words_name_their_element(w):
    t = W.bits(W.table(w.F))
    assert t.shape == (W.V, w.F) and len(np.unique(t)) == t.size
    f = W.table(w.F)
    assert np.isfinite(f).all() and (f >= 0.5).all() and (f < 1.0).all()
    for v in (0, W.V - 1):
        for c in (0, w.F - 1):
            assert W.decode(t[v, c]) == (v, c)
    assert W.decode(W.POISON) is None and W.decode(0) is None and W.decode(W.WORD0 - 1) is None


def test_one_table_is_a_prefix_of_the_next():
    """the same (node, column) is the same word at every width: a row that arrives from another width's table would still decode"""
    assert np.array_equal(W.bits(W.table(1028))[:, :100], W.bits(W.table(100)))


def test_work_space_facts_on_hand_counted_cases():
    assert W.work_space_facts(4, 64) == dict(straddling_rows=0, clamped_waves=0, multi_lead_waves=0, three_wave_rows=0)
    assert W.work_space_facts(64, 1) == dict(straddling_rows=0, clamped_waves=0, multi_lead_waves=1, three_wave_rows=0)
    # C = 65, 3 rows: items 0..194 in waves 0..3; row 0 = [0, 65) ends in wave 1, row 1 = [65, 130) in waves 1..2, row 2 = [130, 195) in 2..3:
    # waves 1..3 begin inside a row, waves 1 and 2 hold two rows each
    assert W.work_space_facts(3, 65) == dict(straddling_rows=3, clamped_waves=3, multi_lead_waves=2, three_wave_rows=0)
    # C = 129, 2 rows: row 0 = [0, 129) waves 0..2, row 1 = [129, 258) waves 2..4; waves 1..4 begin inside a row; wave 2 holds row 1's lead
    assert W.work_space_facts(2, 129) == dict(straddling_rows=2, clamped_waves=4, multi_lead_waves=1, three_wave_rows=2)
    # C = 256: every row is one workgroup of four waves, three of which start inside it
    assert W.work_space_facts(2, 256) == dict(straddling_rows=2, clamped_waves=6, multi_lead_waves=0, three_wave_rows=2)


@pytest.mark.parametrize("w", W.WIDTHS, ids=W.width_id)
def test_every_batch_reaches_what_the_reason_claims(rows_per_batch, w):
    claims = W.claimed_facts(w)
    assert ("straddling_rows" in claims) == (64 % w.C != 0) and ("clamped_waves" in claims) == (w.C > 64) and ("three_wave_rows" in claims) == (w.C >= 129)
    for it, rows in rows_per_batch.items():
        facts = W.work_space_facts(rows, w.C)
        for name in claims:
            assert facts[name] > 0, (it, rows, w, name, facts)
        if w.C > W.BLOCK:
            assert rows * w.C > 2 * W.BLOCK                        # more than one workgroup, every row across a workgroup edge or two


@pytest.mark.parametrize("Kg", [1, 2])
def test_cached_batches_meet_the_floors(oracle, Kg):
    """at the forced capacities: at least FLOOR rows in the member's own shard, FLOOR misses and FLOOR rows in every peer's shard, for
    every member and every batch used; the shards are several chunks at every width"""
    g = W.graph()
    orcs, parts = W.clique_oracles(oracle, 4, Kg)
    for me in range(Kg):
        for it in W.BATCHES:
            want = orcs[me].run_batch(parts[me], g["labels"][parts[me]], it)
            c = W.assert_floors(orcs[me], want["ids"], me, Kg, what="batch %d" % it)
            assert c["own"] + sum(c["peers"]) == c["hits"] and c["hits"] + c["miss"] + int((want["ids"] < 0).sum()) == c["rows"]
    assert (W.CAPACITY[Kg] - 1) // W.CHUNK_ROWS + 1 >= 3


def test_the_map_does_not_depend_on_the_width(oracle):
    a, _ = W.clique_oracles(oracle, 4, 2)
    b, _ = W.clique_oracles(oracle, 257, 2)
    assert np.array_equal(a[0].node_map, b[1].node_map)
    slot = np.nonzero(b[0].node_map == W.CAPACITY[2] + 5)[0]
    assert len(slot) == 1 and np.array_equal(W.bits(b[0].caches[1][5]), W.bits(W.table(257)[slot[0]]))


def test_the_plan_case_asks_every_owner_of_every_requester(oracle):
    Kg = 4
    g = W.graph()
    orcs, parts = W.clique_oracles(oracle, 7, Kg)
    best = np.zeros((Kg, Kg), np.int64)
    for me in range(Kg):
        for it in W.PLAN_BATCHES:
            want = orcs[me].run_batch(parts[me], g["labels"][parts[me]], it)
            counts, pairs = W.expected_plan(orcs[me], want["ids"], me, Kg)
            assert counts[me] == 0 and [len(p) for p in pairs] == counts
            dst = [r for p in pairs for _, r in p]
            assert len(set(dst)) == len(dst) and all(0 <= row < W.CAPACITY[Kg] for p in pairs for row, _ in p)
            best[me] = np.maximum(best[me], counts)
    assert all(best[me, j] >= W.PAIR_FLOOR for me in range(Kg) for j in range(Kg) if j != me), best
    assert (W.CAPACITY[Kg] - 1) // W.CHUNK_ROWS + 1 >= 3
    quiet = W.quiet_seeds(orcs[0])
    assert len(quiet) == W.B
    for me in range(Kg):
        want = orcs[me].run_batch(quiet, g["labels"][quiet], 0, mode=1)
        assert np.array_equal(want["ids"], quiet)                  # no neighbours: the batch is its seeds
        assert W.expected_plan(orcs[me], want["ids"], me, Kg)[0] == [0] * Kg


# ---- assert_rows: each way a lane-to-row mapping goes wrong fails, and the message points at it ------------------------------------------------
IDS = np.array([5, 112, 37, 599, 0, 240], dtype=np.int32)


def failure(got, want):
    with pytest.raises(AssertionError) as ex:
        W.assert_rows("rows", got, want)
    return str(ex.value)


@pytest.mark.parametrize("F", [260, 7])
def test_assert_rows_passes_on_equal_rows_and_says_what_arrived(F):
    want = W.expected_rows(F, IDS)
    W.assert_rows("rows", want.copy(), want)
    W.assert_rows("rows", W.bits(want).copy(), want)
    ch = 4 if F == 7 else 64                                        # column of the chunk that goes wrong: chunk 1, or chunk 16 (the second wave of the row)
    # one 16-byte chunk replaced by the same chunk of the neighbouring row
    got = want.copy()
    got[2, ch:ch + 4] = want[1, ch:ch + 4]
    msg = failure(got, want)
    assert "row 2 column %d (chunk %d) holds node 112's column %d" % (ch, ch // 4, ch) in msg and "expected node 37's column %d" % ch in msg
    assert "1 16-byte chunks of 1 rows" in msg
    # one chunk left as poison
    got = W.bits(want).copy()
    got[3, ch:ch + 4] = W.POISON
    msg = failure(got, want)
    assert "row 3 column %d" % ch in msg and "not a table word (poison)" in msg and "expected node 599's column %d" % ch in msg
    # two rows swapped
    got = want.copy()
    got[[1, 4]] = want[[4, 1]]
    msg = failure(got, want)
    assert "row 1 column 0 (chunk 0) holds node 0's column 0" in msg and "expected node 112's column 0" in msg
    assert "%d 16-byte chunks of 2 rows" % (2 * ((F + 3) // 4)) in msg
    # chunk 0 of a row repeated in every chunk
    got = want.copy()
    got[5] = np.tile(want[5, :4], F // 4 + 1)[:F]
    msg = failure(got, want)
    assert "row 5 column 4 (chunk 1) holds node 240's column 0 (chunk 0)" in msg and "expected node 240's column 4" in msg
    assert "%d 16-byte chunks of 1 rows" % ((F + 3) // 4 - 1) in msg


def test_assert_rows_on_zero_rows_stale_words_and_shapes():
    want = W.expected_rows(8, np.array([3, -1, 9], dtype=np.int32))
    assert not W.bits(want)[1].any() and W.decode(W.bits(want)[2, 7]) == (9, 7)
    got = want.copy()
    got[1] = want[0]                                               # a stale row where a -1 id has none
    msg = failure(got, want)
    assert "row 1 column 0 (chunk 0) holds node 3's column 0" in msg and "expected +0.0" in msg
    got = W.bits(want).copy()
    got[0, 3] = 0x7FC00000
    assert "row 0 column 3 (chunk 0) holds 0x7FC00000, not a table word" in failure(got, want)
    with pytest.raises(AssertionError, match="shape"):
        W.assert_rows("rows", want[:2], want)
