"""Row gathers at every row width of tests/widthcases.py's WIDTHS, across wave, row and workgroup edges.  Item q of a gather-like launch
is (row, chunk) = (q / C, q % C) with C = F / 4 on the 16-byte path and C = F on the scalar one (rows_are_vec4, csrc/launch.h); the
test ids name the kernel instances a width pins:
  uncached dense / padded           k_gather<v4f | float> over a dense and a pitched table
  host-pinned                       k_gather over the host mapping; behind a G = 1 cache: k_row_ptrs in front of k_gather
  cached G = 1, fused / pass        k_gather_lookup<v4f | float>; k_row_ptrs + k_gather with the hit counters
  clique G = 2, fused / pass        ... with rows of the peer's shard, and k_feat_fill_up's shards read back
  clique G = 2, exchange            k_exch_count, k_exch_fill, k_exch_rows serve and scatter
  sums, plain / normalised          k_gather_sum<.., false | true>, uncached and on the clique
  forced scalar                     the float instances at F % 4 == 0, the destination 4 bytes off 16-byte alignment
Every case: batch 0, the middle batch and the short last batch, each per level (launches at off > 0) and in one launch, into a poisoned
buffer; rows and sums bit for bit against table(F)[ids] and the NumPy statements; the words behind the last row keep the poison.  The
table's words name their (node, column), so a failure reads "row 37 column 256 (chunk 64) holds node 112's column 0".  No width is
refused by the library: each is served.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import widthcases as W
from aggref import expected_nbr_sum
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from gcnref import expected_nbr_sum_norm
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

ENV = ("LEGION_SHARD_CHUNK_BYTES", "LEGION_CACHE_HIT_PERIOD", "LEGION_PEER_GATHER")
widths = pytest.mark.parametrize("w", W.ALIGNED, ids=W.width_id)


def set_env(monkeypatch, F, lookup="fused", peers="in-kernel"):
    """shards of CHUNK_ROWS rows per chunk at this width; FindFeat as its own pass (every batch hit-sampled) or inside the gather; the
    peers' rows by in-kernel loads or through the exchange"""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("LEGION_SHARD_CHUNK_BYTES", str(W.shard_chunk_bytes(F)))
    if lookup == "pass":
        monkeypatch.setenv("LEGION_CACHE_HIT_PERIOD", "1")
    if peers == "exchange":
        monkeypatch.setenv("LEGION_PEER_GATHER", "exchange")


# ---- the references: computed once per (width, clique size), shared and left unchanged ------------------------------------------------------
class Refs:
    def __init__(self, oracle):
        self.oracle, self._plain, self._clique, self._sums = oracle, {}, {}, {}

    def plain(self, F):
        """{counter: batch} of the uncached runner"""
        if F not in self._plain:
            self._plain[F] = W.plain_batches(self.oracle, F)
        return self._plain[F]

    def clique(self, F, Kg):
        """(runners, seed lists, {(member, counter): batch}) of the cached configuration; every batch meets the floors"""
        if (F, Kg) not in self._clique:
            g = W.graph()
            orcs, parts = W.clique_oracles(self.oracle, F, Kg)
            wants = {(d, it): orcs[d].run_batch(parts[d], g["labels"][parts[d]], it) for d in range(Kg) for it in W.BATCHES}
            for (d, it), want in wants.items():
                W.assert_floors(orcs[d], want["ids"], d, Kg, what="batch %d" % it)
            self._clique[(F, Kg)] = (orcs, parts, wants)
        return self._clique[(F, Kg)]

    def sums(self, key, want, norm):
        """(n_in, N, S, d) of the existing statements (tests/aggref.py, tests/gcnref.py) over a default-mode batch"""
        if (key, norm) not in self._sums:
            g = W.graph()
            if norm:
                n_in, N, _, S, d = expected_nbr_sum_norm(want, g["indptr"], g["indices"], W.FAN)
            else:
                (n_in, N, _, S), d = expected_nbr_sum(want, g["indptr"], g["indices"], W.FAN), None
            self._sums[(key, norm)] = (n_in, N, S, d)
        return self._sums[(key, norm)]


@pytest.fixture(scope="module")
def refs(oracle):
    return Refs(oracle)


# ---- engines ----------------------------------------------------------------------------------------------------------------------------------
def plain_engine(K, F, feats=None, **kw):
    g, seeds = W.graph(), W.seed_lists(1)[0]
    feats = W.table(F) if feats is None else feats
    return make_engine(K, (W.V, F, g["indptr"], g["indices"], feats), W.B, W.FAN, seeds=dict(train=[(seeds, g["labels"][seeds])]), **kw)


def cached_engine(K, refs, F, Kg, **kw):
    """A clique of Kg members in this process with CAPACITY[Kg] rows each, the way build_clique of tests/test_gpu_scratch_poison.py builds
    it: the pre-sampling batches of the oracle's runners, the forced capacity, and then the oracle's map on every member."""
    L, g = K.lib(), W.graph()
    orcs, parts, wants = refs.clique(F, Kg)
    eng = make_engine(K, (W.V, F, g["indptr"], g["indices"], W.table(F)), W.B, W.FAN, G=Kg, seeds=dict(train=[(p, g["labels"][p]) for p in parts]),
                      train_step=W.PRESC_STEPS, **kw)
    for d in range(Kg):
        for it in range(W.PRESC_STEPS):
            eng.run_batch(d, it, is_presc=True)
    eng.build_cache(cache_agg_mode={1: 0, 2: 1, 4: 2}[Kg], node_capacity=W.CAPACITY[Kg], edge_capacity=0, train_step=W.PRESC_STEPS)
    assert L.GPUCache_Kg(eng.cache) == Kg and L.GPUCache_NodeCapacity(eng.cache, 0) == W.CAPACITY[Kg]
    assert L.GPUCache_ShardChunkRows(eng.cache, 0) == W.CHUNK_ROWS and L.GPUCache_ShardChunkCount(eng.cache, 0) >= 3
    assert L.GPUCache_ShardPitch(eng.cache) == W.row_pitch(F)
    for d in range(Kg):
        L.SetGPUDevice(d)
        assert np.array_equal(K.read_dev(L.GPUCache_GetFeatureMap(eng.cache, d), np.int32, W.V), orcs[d].node_map)
    return eng, orcs, wants


def hit_counters(K, eng, dev):
    n_hit, n_rows = C.c_int32(0), C.c_int32(0)
    K.lib().GPUCache_FeatureCacheHitRate(eng.cache, dev, C.byref(n_hit), C.byref(n_rows))
    return n_hit.value, n_rows.value


# ---- one batch into a poisoned buffer ---------------------------------------------------------------------------------------------------------
def poison(K, eng, dev):
    buf = eng.out[dev][0]["feat"]
    K.lib().SetGPUDevice(dev)
    K.lib().d_memset_async(buf.ptr, 0xFF, buf.nbytes, None)
    return buf


def check_copies(K, eng, F, name, want, dev=0, **kw):
    """the batch `want` gathered into the poisoned buffer: everything but the rows word for word, the rows against table(F)[ids], poison
    behind the batch's last row; returns the batch's ids"""
    buf = poison(K, eng, dev)
    eng.run_batch(dev, **kw)
    assert_batch_equal(want, eng.result(dev, with_features=False), keys=KEYS_NO_FEATURES)
    words = buf.to_numpy(np.uint32, eng.num_ids * F)
    n = len(want["ids"])
    assert 0 < n < eng.num_ids
    W.assert_rows(name, words[:n * F].reshape(n, F), W.expected_rows(F, want["ids"]))
    assert np.array_equal(W.bits(want["features"]), W.bits(W.expected_rows(F, want["ids"])))       # the oracle copied the same rows
    assert (words[n * F:] == W.POISON).all(), "%s: %d words behind row %d were written" % (name, int((words[n * F:] != W.POISON).sum()), n)
    return want["ids"]


def walk_copies(K, eng, F, name, wants, dev=0, after=None):
    """batch 0, the middle batch and the short last batch, each per level and in one launch"""
    for it in W.BATCHES:
        for per_level in (True, False):
            what = "%s, batch %d, %s" % (name, it, "per level" if per_level else "one launch")
            ids = check_copies(K, eng, F, what, wants[it], dev=dev, counter=it, per_level=per_level)
            if after:
                after(what, ids)


def check_sums(K, eng, refs, F, name, key, want, norm, dev=0, **kw):
    """the aggregated batch: rows [0, n_in) against table(F)[ids], the sums behind them against the statement, poison behind the last sum"""
    n_in, N, S, d = refs.sums(key, want, norm)
    buf = poison(K, eng, dev)
    eng.run_batch(dev, agg_last_hop=True, agg_norm="both" if norm else None, **kw)
    got = eng.result(dev, with_features=False)
    assert_batch_equal(want, got, keys=KEYS_NO_FEATURES)
    words = buf.to_numpy(np.uint32, eng.num_ids * F)
    assert 0 < n_in and 0 < N and n_in + N < eng.num_ids
    W.assert_rows(name + ", first rows", words[:n_in * F].reshape(n_in, F), W.expected_rows(F, want["ids"][:n_in]))
    W.assert_rows(name + ", sums", words[n_in * F:(n_in + N) * F].reshape(N, F), S)
    assert (words[(n_in + N) * F:] == W.POISON).all(), "%s: words behind sum %d were written" % (name, N)
    if norm:
        K.lib().GPUMemoryPool_SetCurrentPipe(eng.pools[dev], 0)
        assert np.array_equal(K.read_dev(K.lib().GPUMemoryPool_GetAggOutDeg(eng.pools[dev]), np.int32, len(want["ids"])), d)


def walk_sums(K, eng, refs, F, name, key, wants, norm, dev=0):
    for it in W.BATCHES:
        for per_level in (True, False):
            what = "%s, batch %d, %s" % (name, it, "per level" if per_level else "one launch")
            check_sums(K, eng, refs, F, what, key + (it,), wants[it], norm, dev=dev, counter=it, per_level=per_level)


# ---- uncached -------------------------------------------------------------------------------------------------------------------------------------
@widths
def test_uncached_dense_table(K, refs, monkeypatch, w):
    """k_gather over a dense device table"""
    set_env(monkeypatch, w.F)
    eng = plain_engine(K, w.F)
    try:
        walk_copies(K, eng, w.F, "uncached, dense", refs.plain(w.F))
    finally:
        K.lib().legion_clear_error()
        eng.close()


@widths
def test_uncached_padded_table(K, refs, monkeypatch, w):
    """k_gather over a device table whose rows are legion_row_pitch(F) floats apart (a width that is whole 128-byte lines already: one
    more line apart); the pad floats hold a value that must never arrive"""
    set_env(monkeypatch, w.F)
    pitch = W.row_pitch(w.F) if W.row_pitch(w.F) > w.F else w.F + 32
    assert K.lib().legion_row_pitch(w.F) == W.row_pitch(w.F) and pitch > w.F and (w.F % 4 or pitch % 4 == 0)
    padded = np.full((W.V, pitch), np.float32(-777.0))
    padded[:, :w.F] = W.table(w.F)
    eng = plain_engine(K, w.F, feats=padded.reshape(-1), features_pitch=pitch)
    try:
        walk_copies(K, eng, w.F, "uncached, pitch %d" % pitch, refs.plain(w.F))
    finally:
        K.lib().legion_clear_error()
        eng.close()


@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "behind-a-cache"])
@widths
def test_host_pinned_table(K, refs, monkeypatch, w, cached):
    """the table in pinned host memory, read through the GPU's host mapping: k_gather alone, and behind a G = 1 cache the lookup pass in
    front of it (a host table never takes the fused lookup) with hits from the shard and misses over the mapping"""
    set_env(monkeypatch, w.F)
    if cached:
        eng, orcs, wants = cached_engine(K, refs, w.F, 1, features_location=K.LOC_HOST_PINNED)
        wants = {it: wants[(0, it)] for it in W.BATCHES}
    else:
        eng, wants = plain_engine(K, w.F, features_location=K.LOC_HOST_PINNED), refs.plain(w.F)
    try:
        walk_copies(K, eng, w.F, "host-pinned table" + (", cached" if cached else ""), wants)
    finally:
        K.lib().legion_clear_error()
        eng.close()


# ---- cached, G = 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookup", ["fused", "pass"])
@widths
def test_cached_one_gpu(K, refs, monkeypatch, w, lookup):
    """a forced capacity of CAPACITY[1] rows in several chunks: k_gather_lookup (the first gathered batch behind a cache build is a pass
    batch, so one runs first), or every batch through k_row_ptrs + k_gather with the hit counters equal to the oracle's"""
    set_env(monkeypatch, w.F, lookup=lookup)
    eng, orcs, wants = cached_engine(K, refs, w.F, 1)
    try:
        eng.run_batch(0, 0)

        def counters(what, ids):
            assert hit_counters(K, eng, 0) == (int((orcs[0].node_map[ids[ids >= 0]] >= 0).sum()), len(ids)), what

        walk_copies(K, eng, w.F, "G = 1, %s lookup" % lookup, {it: wants[(0, it)] for it in W.BATCHES}, after=counters if lookup == "pass" else None)
    finally:
        K.lib().legion_clear_error()
        eng.close()


# ---- cached, the G = 2 clique ---------------------------------------------------------------------------------------------------------------------
def assert_shards(K, eng, orcs, F, Kg):
    """k_feat_fill_up at this width: every member's shard, chunk by chunk, holds the oracle's cache rows in its first F floats per row and
    zeros in the pad floats"""
    L = K.lib()
    pitch, cr, cap = L.GPUCache_ShardPitch(eng.cache), L.GPUCache_ShardChunkRows(eng.cache, 0), W.CAPACITY[Kg]
    for j in range(Kg):
        L.SetGPUDevice(j)
        for q in range(L.GPUCache_ShardChunkCount(eng.cache, j)):
            rows = min(cr, cap - q * cr)
            chunk = K.read_dev(L.GPUCache_GetShardChunk(eng.cache, j, q), np.uint32, rows * pitch).reshape(rows, pitch)
            W.assert_rows("shard of member %d, chunk %d" % (j, q), chunk[:, :F], orcs[0].caches[j][q * cr:q * cr + rows])
            assert not chunk[:, F:].any(), "shard of member %d, chunk %d: pad floats are not zero" % (j, q)
        assert q * cr + rows == cap


@pytest.mark.parametrize("way", ["fused", "pass", "exchange"])
@widths
def test_cached_clique(K, refs, monkeypatch, w, way):
    """both members of a G = 2 clique: the peer's rows by in-kernel loads with the fused lookup or the lookup pass, or through
    LEGION_PEER_GATHER=exchange (plan, serve, scatter); the shards read back"""
    set_env(monkeypatch, w.F, lookup="pass" if way == "pass" else "fused", peers="exchange" if way == "exchange" else "in-kernel")
    eng, orcs, wants = cached_engine(K, refs, w.F, 2)
    try:
        assert_shards(K, eng, orcs, w.F, 2)
        for d in (0, 1):
            eng.run_batch(d, 0)

            def counters(what, ids, d=d):
                assert hit_counters(K, eng, d) == (int((orcs[d].node_map[ids[ids >= 0]] >= 0).sum()), len(ids)), what

            walk_copies(K, eng, w.F, "G = 2 member %d, %s" % (d, way), {it: wants[(d, it)] for it in W.BATCHES}, dev=d, after=counters if way == "pass" else None)
    finally:
        K.lib().legion_clear_error()
        eng.close()


# ---- the aggregated last hop ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True], ids=["sums", "normalised"])
@pytest.mark.parametrize("where", ["uncached", "clique"])
@widths
def test_aggregated_last_hop(K, refs, monkeypatch, w, where, norm):
    """k_gather_sum without and with weights: the first rows bit-equal to the table's, the sums bit-equal to the existing statements
    (fp32 adds in draw order: exact for the table's arbitrary floats too) -- uncached, and on both members of the G = 2 clique with
    in-kernel peer reads"""
    set_env(monkeypatch, w.F)
    if where == "clique":
        eng, orcs, wants = cached_engine(K, refs, w.F, 2)
        devs = (0, 1)
    else:
        eng, wants, devs = plain_engine(K, w.F), {(0, it): b for it, b in refs.plain(w.F).items()}, (0,)
    try:
        for d in devs:
            walk_sums(K, eng, refs, w.F, "%s member %d, %s" % (where, d, "normalised sums" if norm else "plain sums"), (w.F, where, d),
                      {it: wants[(d, it)] for it in W.BATCHES}, norm, dev=d)
    finally:
        K.lib().legion_clear_error()
        eng.close()


# ---- the scalar path at F % 4 == 0 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["uncached", "cached-fused", "cached-pass", "plain-sums"])
@pytest.mark.parametrize("w", W.FORCED, ids=W.width_id)
def test_destination_four_bytes_off_alignment(K, refs, monkeypatch, w, config):
    """The destination is an allocation's base + 4 bytes (GPUMemoryPool_SetFloatFeatures), so rows_are_vec4 sends every row kernel down
    its float instance at C = F: C = 64 is a row per wave, C = 256 a row per workgroup.  Rows bit-equal to the aligned run of the same
    engine and to the statement; the 4 bytes in front and everything behind the batch's rows keep the poison."""
    L, F = K.lib(), w.F
    agg = config == "plain-sums"
    set_env(monkeypatch, F, lookup="pass" if config == "cached-pass" else "fused")
    if config.startswith("cached"):
        eng, orcs, wants = cached_engine(K, refs, F, 1)
        wants = {it: wants[(0, it)] for it in W.BATCHES}
        eng.run_batch(0, 0)
    else:
        eng, wants = plain_engine(K, F), refs.plain(F)
    words = (eng.num_ids + 1) * F
    spare = K.DevBuf(words * 4)
    try:
        for it in W.BATCHES:
            for per_level in (True, False):
                name = "%s at base + 4, batch %d, %s" % (config, it, "per level" if per_level else "one launch")
                want = wants[it]
                kw = dict(counter=it, per_level=per_level, agg_last_hop=agg)
                if agg:
                    n_in, N, S, _ = refs.sums((F, "forced", it), want, False)
                    r, expect = n_in + N, np.concatenate([W.bits(W.expected_rows(F, want["ids"][:n_in])), W.bits(S)])
                else:
                    r, expect = len(want["ids"]), W.bits(W.expected_rows(F, want["ids"]))
                buf = poison(K, eng, 0)
                eng.run_batch(0, **kw)
                aligned = buf.to_numpy(np.uint32, r * F).reshape(r, F)
                W.assert_rows(name + " (the aligned run)", aligned, expect)
                L.d_memset_async(spare.ptr, 0xFF, spare.nbytes, None)
                L.GPUMemoryPool_SetFloatFeatures(eng.pools[0], spare.ptr + 4, 0)
                K.check()
                try:
                    eng.run_batch(0, **kw)
                    assert_batch_equal(want, eng.result(0, with_features=False), keys=KEYS_NO_FEATURES)
                    got = spare.to_numpy(np.uint32, words)
                finally:
                    L.GPUMemoryPool_SetFloatFeatures(eng.pools[0], eng.out[0][0]["feat"].ptr, 0)
                    L.d_stream_sync(None)
                rows = got[1:1 + r * F].reshape(r, F)
                W.assert_rows(name, rows, expect)
                assert np.array_equal(rows, aligned), name
                assert got[0] == W.POISON and (got[1 + r * F:] == W.POISON).all() and len(got[1 + r * F:]) >= F - 1, name
                if config == "cached-pass":
                    ids = want["ids"]
                    assert hit_counters(K, eng, 0) == (int((orcs[0].node_map[ids[ids >= 0]] >= 0).sum()), len(ids)), name
    finally:
        L.legion_clear_error()
        spare.free()
        eng.close()
