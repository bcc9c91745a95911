"""The benchmark's two instruments against NumPy (inputs and references: tests/instrumentcases.py; their properties: tests/test_instruments_cpu.py).

legion_copy_f4 / legion_copy_f4_cfg: bench.py times this copy between two uninitialised buffers and prints the rate as the measured HBM
ceiling; a variant that skipped chunks would report a better one.  Here every one of the 32 variants copies a position-dependent pattern
into the interior of a sentinel-filled buffer, at sizes around the workgroup step, with explicit grids whose lanes loop, and at byte counts
that are no multiple of 16: the copied range equals the source word for word, everything else keeps the sentinel, the source is unchanged.
No misaligned or foreign pointer is ever passed: the copy does not check its pointers.

legion_sum_words: the reading consumer of bench.py's `served` legs and its checksum.  Sizes with every n_tail, through the 4x-unrolled loop,
the remainder loop and past the grid cap; the carry out of 32 bits (all-ones words), the wrap-around of *acc, three adjacent accumulators,
two streams, and the refusals, which launch nothing."""
import numpy as np
import pytest

import instrumentcases as IC
from harness import K  # noqa: F401  (the module's library fixture)

pytestmark = pytest.mark.gpu

G = IC.GUARD_BYTES
COPY_MAX = 16 * (6 * IC.COPY_BLOCK * 8 + 77) + 16          # the largest copy_sizes() entry, rounded up to a chunk
SUM_MAX = (IC.SUM_SIZES[-1] + 15) // 16 * 16


def last_error(L):
    msg = (L.legion_last_error() or b"").decode()
    L.legion_clear_error()
    return msg


# ---- the copy ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def copy_bufs(K):
    """the source (the pattern) and a destination with GUARD_BYTES in front of and behind the largest copy"""
    words = IC.pattern(COPY_MAX // 4, 0xC0B1)
    words.setflags(write=False)
    src, dst = K.DevBuf.from_numpy(words), K.DevBuf(G + COPY_MAX + G)
    assert src.ptr % 16 == 0 and dst.ptr % 16 == 0
    yield K.lib(), words, src, dst
    src.free()
    dst.free()


def fill_dst(L, dst):
    L.d_memset_async(dst.ptr, IC.SENTINEL, dst.nbytes, None)


def assert_copied(K, bufs, nbytes, what):
    """dst[G : G + 16 * (nbytes // 16)) holds the source's words, every other byte of dst the sentinel, and the source is what it was"""
    L, words, src, dst = bufs
    L.d_stream_sync(None)
    K.check()
    n = nbytes // 16
    got = dst.to_numpy(np.uint8, dst.nbytes)
    body = got[G:G + 16 * n].view(np.uint32).reshape(-1, 4)
    want = words[:4 * n].reshape(-1, 4)
    bad = np.nonzero((body != want).any(axis=1))[0]
    if len(bad):
        kept = int((body[bad].view(np.uint8) == IC.SENTINEL).all(axis=1).sum())
        raise AssertionError("%s: %d of %d chunks differ from the source (%d of them still hold the sentinel), first at %s" % (what, len(bad), n, kept, bad[:8].tolist()))
    assert (got[:G] == IC.SENTINEL).all(), "%s: the guard in front of the copy was written" % what
    behind = np.nonzero(got[G + 16 * n:] != IC.SENTINEL)[0]
    assert len(behind) == 0, "%s: %d bytes behind the last whole chunk were written, first at +%d (bytes %% 16 = %d)" % (what, len(behind), behind[0], nbytes % 16)
    assert np.array_equal(src.to_numpy(np.uint32, len(words)), words), "%s: the source changed" % what


@pytest.mark.parametrize("unroll,nt,contig", IC.COPY_VARIANTS)
def test_every_copy_variant_copies_every_chunk_and_nothing_else(K, copy_bufs, unroll, nt, contig):
    L, words, src, dst = copy_bufs
    for case in IC.copy_sizes(unroll):
        assert case.nbytes <= COPY_MAX
        fill_dst(L, dst)
        rc = L.legion_copy_f4_cfg(None, dst.ptr + G, src.ptr, case.nbytes, case.grid, unroll, nt, contig)
        assert rc == 0, case
        assert_copied(K, copy_bufs, case.nbytes, "k_copy_f4<%d, %d, %d> %s (grid %d, %d bytes)" % (unroll, nt, contig, case.name, case.grid, case.nbytes))


def test_the_default_copy_is_a_whole_copy_too(K, copy_bufs):
    """legion_copy_f4, the call bench.py's measure_copy times"""
    L, words, src, dst = copy_bufs
    unroll = IC.COPY_DEFAULT[0]
    for case in [c for c in IC.copy_sizes(unroll) if c.grid == 0] + [IC.CopyCase("largest", 0, COPY_MAX)]:
        fill_dst(L, dst)
        L.legion_copy_f4(None, dst.ptr + G, src.ptr, case.nbytes)
        assert_copied(K, copy_bufs, case.nbytes, "legion_copy_f4 %s (%d bytes)" % (case.name, case.nbytes))


def test_the_copy_runs_on_a_created_stream(K, copy_bufs):
    L, words, src, dst = copy_bufs
    fill_dst(L, dst)
    L.d_stream_sync(None)
    s = L.d_stream_create()
    try:
        assert L.legion_copy_f4_cfg(s, dst.ptr + G, src.ptr, 16 * 1801, 2, 4, 3, 1) == 0
        L.d_stream_sync(s)
        assert_copied(K, copy_bufs, 16 * 1801, "k_copy_f4<4, 3, 1> on a created stream")
    finally:
        L.d_stream_destroy(s)


def test_a_copy_of_less_than_a_chunk_is_a_no_op(K, copy_bufs):
    L, words, src, dst = copy_bufs
    fill_dst(L, dst)
    for nbytes in (0, -1, -16, -(1 << 40), 4, 12, 15):
        for variant in (IC.COPY_DEFAULT, (8, 0, 1)):
            assert L.legion_copy_f4_cfg(None, dst.ptr + G, src.ptr, nbytes, 0, *variant) == 0 and not L.legion_last_error(), nbytes
        L.legion_copy_f4(None, dst.ptr + G, src.ptr, nbytes)
    assert_copied(K, copy_bufs, 0, "bytes < 16")


@pytest.mark.parametrize("unroll,nt,contig", IC.COPY_BAD_VARIANTS)
def test_an_unknown_copy_variant_is_refused_and_writes_nothing(K, copy_bufs, unroll, nt, contig):
    L, words, src, dst = copy_bufs
    fill_dst(L, dst)
    for grid in (0, 2):
        assert L.legion_copy_f4_cfg(None, dst.ptr + G, src.ptr, 16 * 600, grid, unroll, nt, contig) == -1
        assert last_error(L).count("legion_copy_f4_cfg: no such variant") == 1
    assert_copied(K, copy_bufs, 0, "variant (%d, %d, %d)" % (unroll, nt, contig))
    assert L.legion_copy_f4_cfg(None, dst.ptr + G, src.ptr, 0, 0, unroll, nt, contig) == 0 and not L.legion_last_error()     # nothing to copy: nothing to refuse


# ---- the word sum -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sum_bufs(K):
    """the summed buffer (the largest size, 16 bytes to spare) and four u64 accumulators"""
    assert SUM_MAX + 16 <= IC.MAX_BUFFER
    src, acc = K.DevBuf(SUM_MAX + 16), K.DevBuf(32)
    assert src.ptr % 16 == 0 and acc.ptr % 8 == 0
    yield K.lib(), src, acc
    src.free()
    acc.free()


@pytest.fixture(scope="module")
def big_pattern():
    words = IC.pattern(SUM_MAX // 4 + 4, 0x5A11)
    words.setflags(write=False)
    return words


def set_acc(L, acc, *values):
    a = np.array(list(values) + [0] * (4 - len(values)), dtype=np.uint64)
    L.d_copy_h_2_d(acc.ptr, a.ctypes.data, 32)


def get_acc(K, L, acc, stream=None):
    L.d_stream_sync(stream)
    K.check()
    return [int(x) for x in acc.to_numpy(np.uint64, 4)]


@pytest.mark.parametrize("nbytes", IC.SUM_SIZES)
def test_the_word_sum_equals_numpy(K, sum_bufs, big_pattern, nbytes):
    L, src, acc = sum_bufs
    n, top = nbytes // 4, 2 ** 64 - 5
    # all-ones words: every addition carries out of 32 bits -- inside a lane, across a wave's shuffles and in the workgroup's partial sums
    L.d_memset_async(src.ptr, 0xFF, SUM_MAX + 16, None)
    set_acc(L, acc, 0)
    L.legion_sum_words(None, src.ptr, nbytes, acc.ptr)
    assert get_acc(K, L, acc) == [n * 0xFFFFFFFF, 0, 0, 0]
    # all-zero words leave *acc as it was
    L.d_memset_async(src.ptr, 0, nbytes, None)
    set_acc(L, acc, 0x0123456789ABCDEF, 1, 2, 3)
    L.legion_sum_words(None, src.ptr, nbytes, acc.ptr)
    assert get_acc(K, L, acc) == [0x0123456789ABCDEF, 1, 2, 3]
    # the pattern: only [0, nbytes) is it, the words behind are still all ones, so a sum that reads past its end is wrong
    words = big_pattern[:n]
    ref = IC.word_sum(words)
    L.d_copy_h_2_d(src.ptr, words.ctypes.data, nbytes)
    set_acc(L, acc, 0)
    L.legion_sum_words(None, src.ptr, nbytes, acc.ptr)
    assert get_acc(K, L, acc) == [ref, 0, 0, 0]
    # *acc accumulates, modulo 2^64
    set_acc(L, acc, top)
    L.legion_sum_words(None, src.ptr, nbytes, acc.ptr)
    assert get_acc(K, L, acc) == [(top + ref) % 2 ** 64, 0, 0, 0]
    L.legion_sum_words(None, src.ptr, nbytes, acc.ptr)
    assert get_acc(K, L, acc) == [(top + 2 * ref) % 2 ** 64, 0, 0, 0]
    # three calls into three adjacent accumulators, as bench.py's reading consumer makes them: each holds its own sum
    half, rest = n // 2 * 4, nbytes - 16
    set_acc(L, acc, 7, 11, 13, 17)
    L.legion_sum_words(None, src.ptr, nbytes, acc.ptr)
    L.legion_sum_words(None, src.ptr, half, acc.ptr + 8)               # half = 0 for a single word: a no-op
    L.legion_sum_words(None, src.ptr + 16, rest, acc.ptr + 16)         # rest <= 0 below 20 bytes: a no-op
    assert get_acc(K, L, acc) == [7 + ref, 11 + IC.word_sum(words[:half // 4]), 13 + IC.word_sum(words[4:]), 17]
    # a created stream and the null stream give the same value
    s = L.d_stream_create()
    try:
        set_acc(L, acc, 0, 0)
        L.d_stream_sync(None)
        L.legion_sum_words(s, src.ptr, nbytes, acc.ptr)
        L.d_stream_sync(s)
        L.legion_sum_words(None, src.ptr, nbytes, acc.ptr + 8)
        assert get_acc(K, L, acc, s) == [ref, ref, 0, 0]
    finally:
        L.d_stream_destroy(s)


def test_the_word_sum_refuses_bad_arguments_before_any_launch(K, sum_bufs):
    L, src, acc = sum_bufs
    L.d_memset_async(src.ptr, 0xFF, 4096, None)
    kept = [99, 98, 97, 96]
    set_acc(L, acc, *kept)
    refusal = "legion_sum_words: src must be 16-byte aligned, bytes a multiple of 4"
    for what, args in (("src + 4", (src.ptr + 4, 16, acc.ptr)), ("src + 8", (src.ptr + 8, 1024, acc.ptr)), ("src + 1", (src.ptr + 1, 16, acc.ptr)),
                       ("6 bytes", (src.ptr, 6, acc.ptr)), ("1023 bytes", (src.ptr, 1023, acc.ptr)), ("17 bytes", (src.ptr, 17, acc.ptr)),
                       ("null src", (None, 16, acc.ptr)), ("null acc", (src.ptr, 16, None)), ("both null", (None, 1024, None))):
        L.legion_sum_words(None, *args)
        assert last_error(L).count(refusal) == 1, what
        assert get_acc(K, L, acc) == kept, what
    for nbytes in (0, -4, -3, -(1 << 40)):                                     # nothing to read: no error, whatever the other arguments are
        for args in ((src.ptr, nbytes, acc.ptr), (src.ptr + 4, nbytes, acc.ptr), (None, nbytes, None)):
            L.legion_sum_words(None, *args)
            assert not L.legion_last_error(), (nbytes, args)
    assert get_acc(K, L, acc) == kept
    L.legion_sum_words(None, src.ptr, 4096, acc.ptr)                           # and the next good call works
    assert get_acc(K, L, acc) == [99 + 1024 * 0xFFFFFFFF, 98, 97, 96]
