"""The generator kernels of csrc/synth.hip away from index 0 (inputs: tests/instrumentcases.py; the references' own proof:
tests/test_instruments_cpu.py).

Each generated value is a closed form of its absolute index, so a window of a few thousand entries that starts at a large e0 tests the
arithmetic of entry 2^32 of a full-size table (uk-union: E = 5.5e9; papers100M: V * F = 1.4e10) in milliseconds.  The reference is the
NumPy statement of legion-1_amd/synth.py, which the CPU test ties to exact integers at the same windows; skews other than 205 use the
integer rule itself.  Every kernel also runs once over LONG_N entries, where lanes take a second grid-stride step with a ragged tail.
Every output lies in a sentinel-filled buffer with a guard behind its last element; all comparisons are by bit pattern."""
import dataclasses
import functools

import numpy as np
import pytest

import instrumentcases as IC
from harness import K  # noqa: F401  (the module's library fixture)

pytestmark = pytest.mark.gpu

N, G = IC.WINDOW_N, IC.GUARD_BYTES
TOP = max(IC.WINDOWS)
SENTINEL_WORD = IC.SENTINEL * 0x01010101


@pytest.fixture(scope="module")
def out(K):
    """one output buffer for the module: the largest call writes LONG_N int64, or LONG_N rows of pitch 2"""
    buf = K.DevBuf(8 * IC.LONG_N + G)
    assert buf.nbytes <= IC.MAX_BUFFER
    yield buf
    buf.free()


def generate(K, out, nbytes, call):
    """Fill [0, nbytes + guard) with the sentinel, run `call(pointer)`, and hand back the nbytes as uint32 words; the guard must be untouched."""
    L = K.lib()
    assert 0 <= nbytes and nbytes % 4 == 0 and nbytes + G <= out.nbytes
    L.d_memset_async(out.ptr, IC.SENTINEL, nbytes + G, None)
    call(out.ptr)
    L.d_stream_sync(None)
    K.check()
    raw = out.to_numpy(np.uint8, nbytes + G)
    touched = np.nonzero(raw[nbytes:] != IC.SENTINEL)[0]
    assert len(touched) == 0, "%d guard bytes behind the output were written, first at +%d" % (len(touched), touched[0])
    return raw[:nbytes].view(np.uint32)


def words(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def assert_same(got_words, want, what):
    want = np.ascontiguousarray(want)
    got = got_words.view(want.dtype).reshape(want.shape)
    if not np.array_equal(words(got), words(want)):
        bad = np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]
        unwritten = int((got_words == SENTINEL_WORD).sum())
        raise AssertionError("%s: %d of %d entries differ (%d words still hold the sentinel), first at %s: %s, expected %s"
                             % (what, len(bad), len(want), unwritten, bad[:5].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist()))


@functools.lru_cache(maxsize=None)
def spec_of(name, scale=1.0):
    import legion1_amd.synth as S
    return S.spec_for(name, scale)


@functools.lru_cache(maxsize=None)
def neighbours_by_the_integer_rule(name, scale, e0, skew):
    s = spec_of(name, scale)
    return np.array([IC.neighbor(e0 + k, s.V, s.M, s.C, skew) for k in range(N)], dtype=np.int32)


# ---- edges: windows up to 2^40 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e0", IC.WINDOWS)
@pytest.mark.parametrize("name,scale", [("uk-union", 1.0), ("products", 0.01)])
def test_neighbours_at_every_window_and_skew(K, synth, out, name, scale, e0):
    L, s = K.lib(), spec_of(name, scale)
    for skew in IC.SKEWS:
        want = synth.neighbors(s, e0, e0 + N) if skew == 205 else neighbours_by_the_integer_rule(name, scale, e0, skew)
        got = generate(K, out, 4 * N, lambda p: L.legion_synth_neighbors_skew(None, p, e0, N, s.V, s.M, s.C, skew))
        assert_same(got, want, "k_synth_neighbors %s e0 = %d skew %d" % (s.name, e0, skew))
    got = generate(K, out, 4 * N, lambda p: L.legion_synth_neighbors(None, p, e0, N, s.V, s.M, s.C))      # the spec'd skew through its own entry point
    assert_same(got, synth.neighbors(s, e0, e0 + N), "legion_synth_neighbors %s e0 = %d" % (s.name, e0))


@pytest.mark.parametrize("e0", IC.WINDOWS)
def test_edge_weights_at_every_window(K, synth, out, e0):
    L = K.lib()
    got = generate(K, out, 4 * N, lambda p: L.legion_synth_edge_weights(None, p, e0, N))
    assert_same(got, synth.edge_weights(e0 + N, e0), "k_synth_edge_weights e0 = %d" % e0)


@pytest.mark.parametrize("e0", IC.WINDOWS)
@pytest.mark.parametrize("dim", IC.EDGE_DIMS)
def test_edge_features_at_every_window(K, synth, out, dim, e0):
    L = K.lib()
    got = generate(K, out, 4 * N * dim, lambda p: L.legion_synth_edge_features(None, p, e0, N, dim))
    assert_same(got, synth.edge_features(e0, N, dim), "k_synth_edge_features e0 = %d dim %d" % (e0, dim))


# ---- node features: rows whose element index reaches the windows ----------------------------------------------------------------------------------
def pitched(rows, pitch):
    """float32 [n, F] rows as the uint32 words of a [n, pitch] buffer whose pad floats hold the sentinel"""
    full = np.full((rows.shape[0], pitch), SENTINEL_WORD, dtype=np.uint32)
    full[:, :rows.shape[1]] = rows.view(np.uint32)
    return full


@pytest.mark.parametrize("start", IC.WINDOWS)
@pytest.mark.parametrize("F", IC.FEATURE_WIDTHS)
def test_features_dense_and_pitched_at_every_window(K, synth, out, F, start):
    L = K.lib()
    s, v0 = dataclasses.replace(spec_of("papers100M"), F=F), IC.feature_v0(start, F)
    want = synth.features(s, np.arange(v0, v0 + N, dtype=np.int64))
    got = generate(K, out, 4 * N * F, lambda p: L.legion_synth_features(None, p, v0, N, F))
    assert_same(got, want, "legion_synth_features F = %d v0 = %d" % (F, v0))
    pitches = sorted({F, F + 1, L.legion_row_pitch(F)})
    assert pitches[0] == F and len(pitches) >= 2
    for pitch in pitches:
        got = generate(K, out, 4 * N * pitch, lambda p: L.legion_synth_features_pitched(None, p, v0, N, F, pitch))
        assert_same(got, pitched(want, pitch), "legion_synth_features_pitched F = %d pitch %d v0 = %d (pad floats keep the sentinel)" % (F, pitch, v0))


def test_a_pitch_below_the_width_is_refused_and_writes_nothing(K, out):
    L = K.lib()
    for F, pitch in ((7, 6), (100, 99), (128, 0), (2, -1)):
        L.d_memset_async(out.ptr, IC.SENTINEL, 4 * 64 * F + G, None)
        L.legion_synth_features_pitched(None, out.ptr, 5, 64, F, pitch)
        L.d_stream_sync(None)
        msg = (L.legion_last_error() or b"").decode()
        L.legion_clear_error()
        assert msg.count("legion_synth_features_pitched: pitch < F") == 1, (F, pitch, msg)
        assert (out.to_numpy(np.uint8, 4 * 64 * F + G) == IC.SENTINEL).all(), (F, pitch)


# ---- per-node kernels: int32 ids below V ------------------------------------------------------------------------------------------------------------
def test_degrees_labels_and_seed_ids_at_the_ends_of_the_table(K, synth, out):
    L, s = K.lib(), spec_of("uk-union")
    lad = np.ascontiguousarray(s.ladder, dtype=np.int32)
    for v0 in IC.node_windows(s.V):
        assert v0 + N <= s.V
        got = generate(K, out, 8 * N, lambda p: L.legion_synth_degrees(None, p, v0, N, lad.ctypes.data))
        assert_same(got, synth.degrees(s, v0, v0 + N), "k_synth_degrees v0 = %d" % v0)
        got = generate(K, out, 4 * N, lambda p: L.legion_synth_labels(None, p, v0, N, s.classes))
        assert_same(got, synth.labels(s, np.arange(v0, v0 + N, dtype=np.int64)), "k_synth_labels v0 = %d" % v0)
        got = generate(K, out, 4 * N, lambda p: L.legion_synth_seed_ids(None, p, v0, N, s.V, s.M2, s.C2, 1, 0))
        assert_same(got, synth.seed_ids(s, v0, v0 + N), "k_synth_seed_ids i0 = %d" % v0)


@pytest.mark.parametrize("stride,phase", IC.SEED_STRIDES)
def test_strided_seed_lists(K, synth, out, stride, phase):
    """the tid % G split of the permutation-ordered list: entry k is seed i0 + phase + k * stride"""
    L, s = K.lib(), spec_of("uk-union")
    for i0 in (0, s.n_train - N):
        want = synth.seed_ids(s, i0, i0 + phase + N * stride)[phase::stride]
        assert len(want) == N
        got = generate(K, out, 4 * N, lambda p: L.legion_synth_seed_ids(None, p, i0, N, s.V, s.M2, s.C2, stride, phase))
        assert_same(got, want, "k_synth_seed_ids i0 = %d stride %d phase %d" % (i0, stride, phase))


# ---- the second grid-stride step ------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_over_more_entries_than_the_capped_grid_has_lanes(K, synth, out):
    """LONG_N entries at each kernel's highest window: 4097 lanes take a second step; dim = 1 and F = 1 so that the element count crosses the grid"""
    L, s, n = K.lib(), spec_of("uk-union"), IC.LONG_N
    assert n > 4096 * 256
    got = generate(K, out, 4 * n, lambda p: L.legion_synth_neighbors_skew(None, p, TOP, n, s.V, s.M, s.C, 205))
    assert_same(got, synth.neighbors(s, TOP, TOP + n), "k_synth_neighbors over LONG_N")
    got = generate(K, out, 4 * n, lambda p: L.legion_synth_edge_weights(None, p, TOP, n))
    assert_same(got, synth.edge_weights(TOP + n, TOP), "k_synth_edge_weights over LONG_N")
    got = generate(K, out, 4 * n, lambda p: L.legion_synth_edge_features(None, p, TOP, n, 1))
    assert_same(got, synth.edge_features(TOP, n, 1), "k_synth_edge_features over LONG_N")
    f1 = dataclasses.replace(spec_of("papers100M"), F=1)
    want = synth.features(f1, np.arange(TOP, TOP + n, dtype=np.int64))
    got = generate(K, out, 4 * n, lambda p: L.legion_synth_features(None, p, TOP, n, 1))
    assert_same(got, want, "k_synth_features over LONG_N")
    got = generate(K, out, 8 * n, lambda p: L.legion_synth_features_pitched(None, p, TOP, n, 1, 2))
    assert_same(got, pitched(want, 2), "k_synth_features over LONG_N at pitch 2")
    v0 = s.V - n
    lad = np.ascontiguousarray(s.ladder, dtype=np.int32)
    got = generate(K, out, 8 * n, lambda p: L.legion_synth_degrees(None, p, v0, n, lad.ctypes.data))
    assert_same(got, synth.degrees(s, v0, s.V), "k_synth_degrees over LONG_N")
    got = generate(K, out, 4 * n, lambda p: L.legion_synth_labels(None, p, v0, n, s.classes))
    assert_same(got, synth.labels(s, np.arange(v0, s.V, dtype=np.int64)), "k_synth_labels over LONG_N")
    got = generate(K, out, 4 * n, lambda p: L.legion_synth_seed_ids(None, p, v0, n, s.V, s.M2, s.C2, 1, 0))
    assert_same(got, synth.seed_ids(s, v0, s.V), "k_synth_seed_ids over LONG_N")
    i0 = s.n_train - 3 * n - 2
    got = generate(K, out, 4 * n, lambda p: L.legion_synth_seed_ids(None, p, i0, n, s.V, s.M2, s.C2, 3, 2))
    assert_same(got, synth.seed_ids(s, i0, i0 + 2 + 3 * n)[2::3], "k_synth_seed_ids over LONG_N, stride 3 phase 2")


# ---- nothing to generate ----------------------------------------------------------------------------------------------------------------------------------
def test_n_of_zero_or_less_writes_nothing(K, out):
    L, s = K.lib(), spec_of("uk-union")
    lad = np.ascontiguousarray(s.ladder, dtype=np.int32)
    for n in (0, -1, -(1 << 31)):
        calls = (lambda p: L.legion_synth_degrees(None, p, 0, n, lad.ctypes.data),
                 lambda p: L.legion_synth_neighbors_skew(None, p, TOP, n, s.V, s.M, s.C, 205),
                 lambda p: L.legion_synth_neighbors(None, p, TOP, n, s.V, s.M, s.C),
                 lambda p: L.legion_synth_features(None, p, TOP, n, 7),
                 lambda p: L.legion_synth_features_pitched(None, p, TOP, n, 7, 8),
                 lambda p: L.legion_synth_labels(None, p, 0, n, s.classes),
                 lambda p: L.legion_synth_edge_weights(None, p, TOP, n),
                 lambda p: L.legion_synth_edge_features(None, p, TOP, n, 3),
                 lambda p: L.legion_synth_seed_ids(None, p, 0, n, s.V, s.M2, s.C2, 2, 1))
        for k, call in enumerate(calls):
            L.d_memset_async(out.ptr, IC.SENTINEL, 2 * G, None)
            call(out.ptr)
            L.d_stream_sync(None)
            K.check()
            assert (out.to_numpy(np.uint8, 2 * G) == IC.SENTINEL).all(), (n, k)
