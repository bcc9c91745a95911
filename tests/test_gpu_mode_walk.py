"""Seeded walks over combinations of the serving modes on long-lived pools (tests/modewalk.py has the lattice, the composed statement and the
walk; tests/test_mode_walk_cpu.py proves the walks' coverage and the zero cap on near-tie rows), and the row kernels' scalar path behind a
destination that is not 16-byte aligned.

Every walk runs on three engines that live as long as the module, so that a step meets whatever the steps -- and the walks -- before it left
in the pool: buffers the setters allocated lazily, progress flags, the launch-size feedback, recorded graphs.
  whole      one logical GPU over the whole CSR: every rule.  Edge rows of 3 floats (k_gather_edges' scalar path).
  clique     two logical GPUs behind a filled cache with CSR fragments: the partitioned rules.  Edge rows of 20 floats (the 16-byte path).
             The walks alternate between the two logical GPUs, and between the fused lookup and the lookup pass (LEGION_CACHE_HIT_PERIOD=1).
  exchange   such a clique under LEGION_PEER_GATHER=exchange: the vectors without an aggregated hand-off, which the exchange refuses by name.
A step that differs from its statement is run once more, alone, on a fresh engine: the failure says whether the combination itself is wrong
or the state the previous step left.  Every comparison is array_equal, floats by bit pattern.  Run with `pytest -m gpu`."""
import os
import time

import numpy as np
import pytest

import drawrulecases as D
import eidref as R
import modewalk as M
from aggcases import assert_sum_bits
from conftest import KEYS_NO_FEATURES, assert_batch_equal
from distinctcases import expected_sums
from eidref import bits
from harness import K, make_engine  # noqa: F401  (K: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

WALKS = int(os.environ.get("LEGION_STRESS_WALK_N", str(M.DEFAULT_WALKS)))
DIMS = dict(whole=3, clique=20, exchange=4)         # the scalar path; C = 5 chunks of 16 bytes; one chunk
POISON = 0xA5A5A5A5


@pytest.fixture(scope="module")
def g():
    return D.graph()


def filled_clique(K, eng, V):
    """two logical GPUs: a pre-sampling epoch each, then the cache with CSR fragments (tests/test_gpu_edge_ids.py builds it the same way)"""
    L = K.lib()
    for dev in range(2):
        for it in D.COUNTERS:
            eng.run_batch(dev, it, is_presc=True)
    eng.build_cache(cache_agg_mode=1, node_capacity=V // 8, edge_capacity=V // 3, train_step=2)
    assert L.GPUCache_Kg(eng.cache) == 2 and all(L.GPUGraphStorage_FragmentRows(eng.graph, dev) == V // 3 for dev in range(2))
    return eng


class Engines:
    """One engine per kind, built on first use and closed with the module; the tables, the alias rows and the statements are computed once
    and never changed.  held[kind]: what every pipe of the kind's engine was last left with."""

    def __init__(self, K, g):
        self.K, self.g, self.made, self.X, self.want, self.rows = K, g, {}, {}, {}, None
        self.held = {kind: {} for kind in M.KINDS}

    def table(self, dim):
        if dim not in self.X:
            import legion1_amd.synth as S
            self.X[dim] = S.edge_features(0, len(self.g["indices"]), dim)
        return self.X[dim]

    def build(self, kind):
        g, G = self.g, 1 if kind == "whole" else 2
        seeds = D.seed_list(M.TILE)
        eng = make_engine(self.K, (D.V, D.F, g["indptr"], g["indices"], g["feats"]), M.B, M.FAN, G=G, seeds=dict(train=[(seeds, g["labels"][seeds])] * G),
                          edge_weights=g["w"], retain_edge_weights=True, cache_memory=int(D.V * D.F * 4 * 0.15), train_step=2, pipeline_depth=2,
                          edge_features=self.table(DIMS[kind]))
        if G == 2:
            return filled_clique(self.K, eng, D.V)
        self.K.lib().GPUCache_SetPreSc(eng.cache, 0)        # no cache follows: the planner of a recorded batch counts no hotness
        return eng

    def get(self, kind):
        if kind not in self.made:
            self.made[kind] = self.build(kind)
        return self.made[kind]

    def alias(self):
        if self.rows is None:
            self.rows = self.get("whole").alias_rows(0)     # the table the device built: any valid table is a statement
        return self.rows

    def statement_of(self, kind):
        X = self.table(DIMS[kind])
        return lambda v: M.statement(self.g, X, v, alias=self.alias() if v.rule == M.ALIAS else None, cache=self.want)

    def close(self):
        for eng in self.made.values():
            eng.close()


@pytest.fixture(scope="module")
def engines(K, g):
    e = Engines(K, g)
    yield e
    K.lib().legion_clear_error()
    e.close()


def set_env(mp, kind, lookup_pass=False):
    for var in ("LEGION_PEER_GATHER", "LEGION_CACHE_HIT_PERIOD"):
        mp.delenv(var, raising=False)
    if kind == "exchange":
        mp.setenv("LEGION_PEER_GATHER", "exchange")
    if lookup_pass:
        mp.setenv("LEGION_CACHE_HIT_PERIOD", "1")


@pytest.mark.parametrize("n", range(WALKS))
def test_a_walk_over_the_serving_modes_on_every_engine_kind(K, engines, monkeypatch, n):
    """walk n (modewalk.walk(n, kind=...): 24 steps) on the whole-CSR engine, on the clique -- logical GPU n % 2, the lookup pass in walks
    2 and 3 of every four -- and on the clique under the exchange.  Behind every step the other pipe is read once more."""
    for kind in M.KINDS:
        dev = 0 if kind == "whole" else n % 2
        with monkeypatch.context() as mp:
            set_env(mp, kind, lookup_pass=kind == "clique" and n % 4 >= 2)
            eng = engines.get(kind)
            t0 = time.perf_counter()
            try:
                M.run_walk(eng, M.walk(n, kind=kind), engines.statement_of(kind), lambda: engines.build(kind), dev=dev, held=engines.held[kind],
                           label="walk %d on the %s engine" % (n, kind))
            except BaseException:
                engines.held[kind].clear()                  # what the pipes hold behind a failed step is not stated
                K.lib().legion_clear_error()
                raise
            print("walk %d, %s: %.3f s" % (n, kind, time.perf_counter() - t0))


def test_the_exchange_refuses_the_aggregated_hand_off_by_name_and_the_next_step_runs(K, engines, monkeypatch):
    eng = engines.get("exchange")
    set_env(monkeypatch, "exchange")
    with pytest.raises(RuntimeError) as ex:
        eng.run_batch(0, 0, agg_last_hop=True, sample="distinct")
    assert "LEGION_PEER_GATHER=exchange" in str(ex.value) and "aggregated last hop (GPUMemoryPool_SetAggLastHop)" in str(ex.value)
    engines.held["exchange"].pop((0, 0), None)              # pipe 0 holds a sampled batch without its rows
    nxt = M.Vector(rule="distinct", seed=None, round=0, edge_ids=True, edge_features=True, agg="none", presc=False, per_level=True, pipe=0, counter=1, driver="run_batch")
    M.run_walk(eng, [nxt, nxt._replace(pipe=1, counter=0, driver="replay")], engines.statement_of("exchange"), lambda: engines.build("exchange"),
               held=engines.held["exchange"], label="behind the exchange's refusal")


# ---- the scalar fallback of rows_are_vec4 ----------------------------------------------------------------------------------------------
def test_rows_at_a_destination_four_bytes_off_alignment(K, g, monkeypatch):
    """The row kernels take their 16-byte path only when F % 4 == 0 and both the table and the destination are 16-byte aligned (rows_are_vec4,
    csrc/launch.h); every other test reaches the scalar kernels through F % 4 != 0.  The destination is the caller's
    (GPUMemoryPool_SetFloatFeatures): here it is an allocation's base + 4 bytes at F = 8.  Batch 0 through the uncached gather, the cached
    gather of the clique's logical GPU 0 in both lookups, and get_feature_kernel_agg with plain sums: the rows read from base + 4 are
    bit-equal to the aligned run and to the statement, and the 4 bytes in front and everything behind the batch's rows -- the spare row's
    tail included -- keep the poison.  Neither the setter nor a launcher refuses such a pointer: it is served."""
    L = K.lib()
    F = 8
    set_env(monkeypatch, "whole")
    g8 = dict(g, feats=np.random.RandomState(11).rand(D.V, F).astype(np.float32))
    seeds = D.seed_list(M.TILE)
    lab = g["labels"][seeds]
    want = R.run_batch(g8, "stream", seeds, lab, M.B, 0, M.FAN)
    n_in, N, S, _ = expected_sums(want, M.FAN, False)
    n = len(want["ids"])
    assert want["features"].shape == (n, F) and 0 < n_in < n and N > 0

    def build(G):
        eng = make_engine(K, (D.V, F, g["indptr"], g["indices"], g8["feats"]), M.B, M.FAN, G=G, seeds=dict(train=[(seeds, lab)] * G),
                          cache_memory=int(D.V * F * 4 * 0.15) if G == 2 else 0, train_step=2)
        return filled_clique(K, eng, D.V) if G == 2 else eng

    def check_rows(name, rows, agg):
        if agg:
            assert np.array_equal(bits(rows[:n_in]), bits(want["features"][:n_in])), name
            assert_sum_bits(name, rows[n_in:], S)
        else:
            assert np.array_equal(bits(rows), bits(want["features"])), name

    def off_by_four(eng, name, agg, aligned, **kw):
        """one batch into base + 4: (the rows, bit-compared with `aligned` and the statement); the words around them keep the poison"""
        words = (eng.num_ids + 1) * F
        spare = K.DevBuf(words * 4)
        try:
            fill = np.full(words, POISON, np.uint32)
            L.d_copy_h_2_d(spare.ptr, fill.ctypes.data, fill.nbytes)
            L.GPUMemoryPool_SetFloatFeatures(eng.pools[0], spare.ptr + 4, 0)
            K.check()
            eng.run_batch(0, 0, **kw)
            assert_batch_equal(want, eng.result(0, with_features=False), keys=KEYS_NO_FEATURES)
            got = spare.to_numpy(np.uint32, words)
            r = (n_in + N) if agg else n
            rows = got[1:1 + r * F].view(np.float32).reshape(r, F)
            check_rows(name, rows, agg)
            assert np.array_equal(bits(rows), bits(aligned)), name
            assert got[0] == POISON and (got[1 + r * F:] == POISON).all() and len(got[1 + r * F:]) >= F - 1, name
        finally:
            L.GPUMemoryPool_SetFloatFeatures(eng.pools[0], eng.out[0][0]["feat"].ptr, 0)
            L.d_stream_sync(None)
            spare.free()

    whole = build(1)
    try:
        for agg, kw in ((False, {}), (True, dict(agg_last_hop=True))):
            whole.run_batch(0, 0, **kw)
            res = whole.result(0)
            aligned = np.concatenate([res["features"], res["nbr_sum"]]) if agg else res["features"]
            check_rows("aligned", aligned, agg)
            off_by_four(whole, "uncached gather" if not agg else "plain sums", agg, aligned, **kw)
    finally:
        L.legion_clear_error()
        whole.close()
    clique = build(2)
    try:
        for _ in range(2):                                  # the first gathered batch of a cache is a lookup-pass batch, the second a fused one
            clique.run_batch(0, 0)
            aligned = clique.result(0)["features"]
            check_rows("aligned, cached", aligned, False)
        fmap = K.read_dev(L.GPUCache_GetFeatureMap(clique.cache, 0), np.int32, D.V)[want["ids"]]
        assert (fmap >= 0).any() and (fmap < 0).any() and ((fmap >= 0) & (fmap // (D.V // 8) != 0)).any()      # hits, misses, rows of the peer's shard
        off_by_four(clique, "cached gather, fused lookup", False, aligned)
        monkeypatch.setenv("LEGION_CACHE_HIT_PERIOD", "1")
        off_by_four(clique, "cached gather, lookup pass", False, aligned)
    finally:
        L.legion_clear_error()
        clique.close()
