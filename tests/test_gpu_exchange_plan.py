"""legion_exchange_plan's documented contract (include/legion_amd.h), through the C ABI in one process and without torch, on a Kg = 4 clique
with forced capacities and shards in several chunks: counts[j] is the number of batch rows cached on clique member j; the request lists
are contiguous per owner, owner-major; req_row is the row inside the owner's shard and req_dst the batch row; nothing is written behind
the last request.  The order inside one owner's list comes from atomics and is unspecified, so every owner's slice is compared as a
sorted list of pairs.  Then the rest of the protocol by hand -- local, per owner serve and copy back, scatter -- must leave
table(F)[ids] in the poisoned feature buffer.  Widths: F = 7 (scalar), 100 (pitched 16-byte rows) and 260 (C = 65).  Inputs and their
floors: tests/widthcases.py, proven on the CPU by tests/test_gather_widths_cpu.py.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import widthcases as W
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

KG = 4
LIST_POISON = -0x01010102          # int32 of the bytes FE FE FE FE: no row of a shard and no row of a batch


class Clique:
    """the engine, the oracle's runners, and per member the plan's three device buffers"""

    def __init__(self, K, oracle, F):
        L, g = K.lib(), W.graph()
        self.K, self.L, self.F = K, L, F
        self.orcs, self.parts = W.clique_oracles(oracle, F, KG)
        self.quiet = W.quiet_seeds(self.orcs[0])
        seeds = dict(train=[(p, g["labels"][p]) for p in self.parts], valid=[(self.quiet, g["labels"][self.quiet])] * KG)
        self.eng = eng = make_engine(K, (W.V, F, g["indptr"], g["indices"], W.table(F)), W.B, W.FAN, G=KG, seeds=seeds, train_step=W.PRESC_STEPS)
        for d in range(KG):
            for it in range(W.PRESC_STEPS):
                eng.run_batch(d, it, is_presc=True)
        eng.build_cache(cache_agg_mode=2, node_capacity=W.CAPACITY[KG], edge_capacity=0, train_step=W.PRESC_STEPS)
        assert L.GPUCache_Kg(eng.cache) == KG and L.GPUCache_NodeCapacity(eng.cache, 0) == W.CAPACITY[KG]
        assert L.GPUCache_ShardChunkRows(eng.cache, 0) == W.CHUNK_ROWS and L.GPUCache_ShardChunkCount(eng.cache, 0) >= 3
        self.bufs = []
        for d in range(KG):
            L.SetGPUDevice(d)
            assert np.array_equal(K.read_dev(L.GPUCache_GetFeatureMap(eng.cache, d), np.int32, W.V), self.orcs[d].node_map)
            self.bufs.append(dict(req_row=K.DevBuf(eng.num_ids * 4), req_dst=K.DevBuf(eng.num_ids * 4), counts=K.DevBuf(2 * W.MAX_DEVICE * 4)))

    def plan(self, me, counter, mode=0):
        """sample the batch on member `me` without gathering, poison both lists and the feature buffer, plan: (counts[Kg], req_row, req_dst)"""
        L, eng, b = self.L, self.eng, self.bufs[me]
        eng.run_batch(me, counter, mode=mode, gather=False)
        L.SetGPUDevice(me)
        L.GPUMemoryPool_SetCurrentPipe(eng.pools[me], 0)
        feat = eng.out[me][0]["feat"]
        L.d_memset_async(feat.ptr, 0xFF, feat.nbytes, None)
        for name in ("req_row", "req_dst"):
            L.d_memset_async(b[name].ptr, 0xFE, b[name].nbytes, None)
        assert L.legion_exchange_plan(None, eng.cache, eng.noder, eng.pools[me], me, b["req_row"].ptr, b["req_dst"].ptr, b["counts"].ptr) == 0
        L.d_stream_sync(None)
        self.K.check()
        return (b["counts"].to_numpy(np.int32, KG).tolist(), b["req_row"].to_numpy(np.int32, eng.num_ids), b["req_dst"].to_numpy(np.int32, eng.num_ids))

    def close(self):
        for d, b in enumerate(self.bufs):
            self.L.SetGPUDevice(d)
            for x in b.values():
                x.free()
        self.L.legion_clear_error()
        self.eng.close()


@pytest.fixture(params=W.PLAN_WIDTHS, ids=lambda F: "F%d-%s-C%d" % (F, W.path_of(F), W.chunks_per_row(F)))
def clique(request, K, oracle, monkeypatch):
    F = request.param
    for name in ("LEGION_CACHE_HIT_PERIOD", "LEGION_PEER_GATHER"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("LEGION_SHARD_CHUNK_BYTES", str(W.shard_chunk_bytes(F)))
    c = Clique(K, oracle, F)
    yield c
    c.close()


def assert_plan(c, me, want, counts, req_row, req_dst):
    """the contract, owner by owner; returns the total number of requests"""
    exp_counts, exp_pairs = W.expected_plan(c.orcs[me], want["ids"], me, KG)
    assert counts == exp_counts and counts[me] == 0, (me, counts, exp_counts)
    at = 0
    for j in range(KG):
        got = sorted(zip(req_row[at:at + counts[j]].tolist(), req_dst[at:at + counts[j]].tolist()))
        assert got == exp_pairs[j], "requester %d, owner %d: the slice at %d is not the set of this owner's rows" % (me, j, at)
        at += counts[j]
    assert len(set(req_dst[:at].tolist())) == at                                   # every batch row is asked for once
    assert (req_row[at:] == LIST_POISON).all() and (req_dst[at:] == LIST_POISON).all()   # nothing behind the last request
    return at


def test_plan_lists_and_the_protocol_by_hand(K, clique):
    """every member as the requester, two batches: the plan's lists against the oracle's map, every owner's served rows against the
    oracle's cache rows, and after local + scatter the whole batch against table(F)[ids]"""
    c, L, eng, F = clique, K.lib(), clique.eng, clique.F
    g = W.graph()
    best = np.zeros((KG, KG), np.int64)
    for me in range(KG):
        for it in W.PLAN_BATCHES:
            name = "requester %d, batch %d" % (me, it)
            want = c.orcs[me].run_batch(c.parts[me], g["labels"][c.parts[me]], it)
            counts, req_row, req_dst = c.plan(me, it)
            assert_batch_equal(want, eng.result(me, with_features=False), keys=KEYS_NO_FEATURES)
            total = assert_plan(c, me, want, counts, req_row, req_dst)
            best[me] = np.maximum(best[me], counts)
            assert L.legion_exchange_local(None, eng.cache, eng.noder, eng.pools[me], me) == 0
            L.d_stream_sync(None)
            K.check()
            at = 0
            for j in range(KG):
                n = counts[j]
                if n == 0:
                    continue
                L.SetGPUDevice(j)                                                  # the owner: the list over, its rows into a send buffer, the rows back
                lst, out = K.DevBuf.from_numpy(req_row[at:at + n]), K.DevBuf(n * F * 4)
                L.legion_exchange_serve(None, eng.cache, j, lst.ptr, n, out.ptr)
                L.d_stream_sync(None)
                K.check()
                served = out.to_numpy(np.uint32, n * F).reshape(n, F)
                lst.free()
                out.free()
                W.assert_rows(name + ", rows served by owner %d" % j, served, c.orcs[me].caches[j][req_row[at:at + n]])
                L.SetGPUDevice(me)                                                 # the requester: the owner's rows to their place
                rows, dst = K.DevBuf.from_numpy(served), K.DevBuf.from_numpy(req_dst[at:at + n])
                L.GPUMemoryPool_SetCurrentPipe(eng.pools[me], 0)
                L.legion_exchange_scatter(None, eng.pools[me], rows.ptr, dst.ptr, n, F)
                L.d_stream_sync(None)
                K.check()
                rows.free()
                dst.free()
                at += n
            assert at == total
            L.SetGPUDevice(me)
            words = eng.out[me][0]["feat"].to_numpy(np.uint32, eng.num_ids * F)
            n = len(want["ids"])
            W.assert_rows(name + ", the batch", words[:n * F].reshape(n, F), W.expected_rows(F, want["ids"]))
            assert (words[n * F:] == W.POISON).all(), name
    assert all(best[me, j] >= W.PAIR_FLOOR for me in range(KG) for j in range(KG) if j != me), best


def test_a_batch_without_peer_rows_and_empty_lists(K, clique):
    """a validation batch of nodes without neighbours that nobody caches: all counts 0 and both lists untouched, and the local gather
    alone completes the batch; legion_exchange_serve and legion_exchange_scatter with n = 0 leave everything untouched"""
    c, L, eng, F = clique, K.lib(), clique.eng, clique.F
    g = W.graph()
    for me in (0, KG - 1):
        want = c.orcs[me].run_batch(c.quiet, g["labels"][c.quiet], 0, mode=1)
        assert np.array_equal(want["ids"], c.quiet) and W.expected_plan(c.orcs[me], want["ids"], me, KG)[0] == [0] * KG
        counts, req_row, req_dst = c.plan(me, 0, mode=1)
        assert_batch_equal(want, eng.result(me, with_features=False), keys=KEYS_NO_FEATURES)
        assert counts == [0] * KG and assert_plan(c, me, want, counts, req_row, req_dst) == 0
        # n = 0: neither the owner's send buffer nor the requester's feature buffer is touched, with or without pointers
        out = K.DevBuf(F * 4)
        L.d_memset_async(out.ptr, 0xFF, out.nbytes, None)
        L.legion_exchange_serve(None, eng.cache, me, c.bufs[me]["req_row"].ptr, 0, out.ptr)
        L.legion_exchange_serve(None, eng.cache, me, None, 0, None)
        L.legion_exchange_scatter(None, eng.pools[me], out.ptr, c.bufs[me]["req_dst"].ptr, 0, F)
        L.legion_exchange_scatter(None, eng.pools[me], None, None, 0, F)
        L.d_stream_sync(None)
        K.check()
        assert (out.to_numpy(np.uint32, F) == W.POISON).all()
        out.free()
        feat = eng.out[me][0]["feat"]
        assert (feat.to_numpy(np.uint32, eng.num_ids * F) == W.POISON).all()
        assert L.legion_exchange_local(None, eng.cache, eng.noder, eng.pools[me], me) == 0
        L.d_stream_sync(None)
        K.check()
        words = feat.to_numpy(np.uint32, eng.num_ids * F)
        n = len(want["ids"])
        W.assert_rows("requester %d, the quiet batch" % me, words[:n * F].reshape(n, F), W.expected_rows(F, want["ids"]))
        assert (words[n * F:] == W.POISON).all()
