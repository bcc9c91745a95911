"""Inputs and references of tests/test_gpu_instruments.py and tests/test_gpu_synth_windows.py -- the benchmark's instruments (the streaming
copy behind the measured HBM ceiling, the word sum behind `value_served`) and the generator kernels every dataset is made of -- with what
tests/test_instruments_cpu.py proves about them without a GPU.

Three statements of each generator rule exist: csrc/synth.hip (HIP), legion-1_amd/synth.py (NumPy) and, below, plain Python `int`
arithmetic with explicit masks (no NumPy, so nothing can wrap or be truncated unnoticed).  The CPU test ties NumPy to the integers at every
window; the GPU tests compare the kernels with NumPy.  Everything is bit-exact: integers, or float32 values that are exact by
construction.  No tolerance appears anywhere.  A helper module, not collected by pytest."""
import collections

import numpy as np

M32, M64 = (1 << 32) - 1, (1 << 64) - 1

# ---- the generator's rules as exact integers (spec: the docstring of legion-1_amd/synth.py; constants restated, not imported) --------------
GEN_SEED = 0x1E610
S_DEG, S_NBR, S_FEAT, S_LAB = ((GEN_SEED << 32) ^ t for t in (0x0DE6, 0x0EB2, 0xFEA7, 0x1AB1))
S_WGT, S_WGT_BLOCK = (GEN_SEED << 32) ^ 0x3E16, (GEN_SEED << 32) ^ 0xB3E16
NBUCKET = 24
EDGE_FEAT_TAG, GOLDEN32 = 0x45464541, 0x9E3779B9


def sm64(z):
    """splitmix64's finaliser of z + the golden increment, modulo 2^64"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def neighbor(e, V, M, C, skew=205):
    """the neighbour id of CSR entry e: `skew` of 256 entries take the cubed (Zipf-like) variate, the others the uniform one"""
    h = sm64((S_NBR + e) & M64)
    a = h >> 32
    x = a
    if (h & 0xFF) < skew:
        x = (((((a * a) & M64) >> 32) * a) & M64) >> 32
    r = ((x * V) & M64) >> 32
    return ((r * M + C) & M64) % V


def edge_weight(e):
    """0 when the low four bits of the entry's hash or of the hash of its block of 64 entries are 0, else 1 + the entry's next four bits"""
    h, hb = sm64((S_WGT + e) & M64), sm64((S_WGT_BLOCK + (e >> 6)) & M64)
    return 1 + ((h >> 4) & 15) if (h & 15) and (hb & 15) else 0


def mix32(z):
    z &= M32
    z = ((z ^ (z >> 16)) * 0x7FEB352D) & M32
    z = ((z ^ (z >> 15)) * 0x846CA68B) & M32
    return z ^ (z >> 16)


def edge_feature(e, c):
    """the top 24 bits of a 32-bit mix of the entry's position -- low word AND high word -- and the column"""
    row = mix32((e & M32) ^ mix32(((e >> 32) & M32) ^ EDGE_FEAT_TAG))
    return mix32((row + c * GOLDEN32) & M32) >> 8


def label(v, classes):
    return sm64((S_LAB + v) & M64) % classes


def seed_id(i, V, M2, C2):
    return ((i * M2 + C2) & M64) % V


def degree(v, ladder):
    """bucket = leading zeros of the hash's top 24 bits (24 when they are all zero), degree = the ladder's step + the low word modulo its span"""
    h = sm64((S_DEG + v) & M64)
    top = h >> 40
    b = 24 - top.bit_length()
    lo, hi = int(ladder[b]), int(ladder[b + 1])
    return lo + (h & M32) % (hi - lo)


def feature(v, c, F):
    """element (v, c) of the feature table: the hash's top 24 bits times 2^-24, minus 0.5 -- every step exact in float32"""
    k = sm64((S_FEAT + v * F + c) & M64) >> 40
    return np.float32(k) * np.float32(2.0 ** -24) - np.float32(0.5)


# ---- windows: a closed form of the absolute index is tested at a large index by a short window that starts there ----------------------------
WINDOWS = (0, 2 ** 31 - 300, 2 ** 32 - 300, 2 ** 32 + 12345, 2 ** 33 - 7, 2 ** 40 - 50)
WINDOW_N = 3000                     # entries per window in a NumPy comparison
EXACT_N = 200                       # the exact-integer restatement checks the first and the last EXACT_N entries of a window
LONG_N = 4096 * 256 + 4097          # big_grid (csrc/synth.hip) caps at 4096 x 256 lanes: a second grid-stride step for one lane more than the first 4096, i.e. a ragged tail
SKEWS = (0, 1, 205, 255, 256)
EDGE_DIMS = (1, 3, 64)
FEATURE_WIDTHS = (1, 7, 100, 128)
SPECS = (("uk-union", 1.0), ("papers100M", 1.0), ("products", 0.01))
SEED_STRIDES = tuple((s, p) for s in (1, 2, 3, 8) for p in sorted({0, 1, s - 1}))        # (stride, phase): list i0 + phase + k * stride


def exact_slices(n=WINDOW_N):
    """the index ranges of a window of n entries that the integer restatement checks"""
    return (range(0, min(EXACT_N, n)), range(max(n - EXACT_N, 0), n))


def node_windows(V, n=WINDOW_N):
    """first ids of the degree / label / seed-id windows of a table of V nodes"""
    return (0, 12345, V - n)


def feature_v0(start, F):
    """the row whose elements contain absolute element `start`: v0 * F <= start < (v0 + 1) * F"""
    return start // F


# ---- the copy's cases -------------------------------------------------------------------------------------------------------------------------
COPY_BLOCK = 256                    # __launch_bounds__(256): lanes per workgroup of k_copy_f4
COPY_UNROLLS, COPY_NTS, COPY_CONTIGS = (1, 2, 4, 8), (0, 1, 2, 3), (0, 1)
COPY_VARIANTS = tuple((u, nt, c) for u in COPY_UNROLLS for nt in COPY_NTS for c in COPY_CONTIGS)
COPY_DEFAULT = (1, 3, 0)            # legion_copy_f4: one chunk per lane, non-temporal loads and stores, grid-strided
COPY_BAD_VARIANTS = ((3, 0, 0), (1, 4, 0), (1, 0, 2), (0, 3, 0), (1, -1, 0), (16, 3, 1))      # unroll 0: the derived grid would divide by it
GUARD_BYTES = 4096
SENTINEL = 0xA5                     # destination fill and guards; the pattern below never produces a buffer of it
CopyCase = collections.namedtuple("CopyCase", "name grid nbytes")


def copy_sizes(unroll):
    """the sizes (grid, bytes) a variant of `unroll` chunks per lane is run at; a workgroup's step is 256 * unroll chunks"""
    step = COPY_BLOCK * unroll
    cases = [CopyCase(name, 0, 16 * n) for name, n in (("one chunk", 1), ("block - 1", 255), ("block", 256), ("block + 1", 257), ("step - 1", step - 1),
                                                       ("step", step), ("step + 1", step + 1), ("three steps ragged", 3 * step + 77))]
    cases += [CopyCase("grid 3 loops", 3, 16 * (2 * 3 * step + 77)), CopyCase("grid 1 loops", 1, 16 * (5 * step + 1))]
    cases += [CopyCase("%s + %d bytes" % (name, r), 0, 16 * n + r) for name, n in (("one chunk", 1), ("three steps ragged", 3 * step + 77)) for r in (4, 8, 12)]
    return cases


def copy_plan(case, unroll):
    """what legion_copy_f4_cfg makes of a case: chunks n, bytes left over, workgroups, iterations of the lane loop, chunks in the last step"""
    n, step = case.nbytes // 16, COPY_BLOCK * unroll
    grid = case.grid if case.grid > 0 else -(-n // step)
    per_iter = grid * step
    return dict(n=n, rem=case.nbytes % 16, grid=grid, iters=-(-n // per_iter), last=n - (-(-n // per_iter) - 1) * per_iter, per_iter=per_iter, step=step)


def copy_touched(n, grid, unroll, contig, contig_step=None, guard_slack=0):
    """how often k_copy_f4<unroll, ., contig> stores each of n chunks, as plain index arithmetic over (workgroup, lane, iteration, u).
    contig_step / guard_slack restate two wrong kernels: the CONTIG distance between a lane's chunks, and a store guard of `< n - slack`."""
    hits = np.zeros(n, np.int64)
    lanes = np.arange(COPY_BLOCK, dtype=np.int64)
    step = (COPY_BLOCK if contig_step is None else contig_step) if contig else grid * COPY_BLOCK
    stride = grid * COPY_BLOCK * unroll
    for b in range(grid):
        i = b * COPY_BLOCK * unroll + lanes if contig else lanes + COPY_BLOCK * b
        while (i < n).any():
            live = i[i < n]
            for u in range(unroll):
                at = live + u * step
                np.add.at(hits, at[at < n - guard_slack], 1)
            i = i + stride
    return hits


# ---- the word sum's cases -----------------------------------------------------------------------------------------------------------------------
SUM_GRID_CAP, SUM_CHUNKS_PER_GROUP = 2048, 1024        # legion_sum_words: min(max(ceil(n16 / 1024), 1), 2048) workgroups of 256 lanes
SUM_SIZES = (4, 8, 12, 16, 20, 28,
             16 * 1023, 16 * 1023 + 12, 16 * 1024, 16 * 1024 + 4, 16 * 1025,
             16 * (4 * 1024 + 3) + 8,
             16 * (2048 * 1024 + 5 * 1024 + 3) + 12)
MAX_BUFFER = 64 << 20


def sum_plan(nbytes):
    """what legion_sum_words makes of a size: 16-byte chunks, trailing words, workgroups, and per lane 0 of workgroup 0 the trips of the
    4x-unrolled loop and of the remainder loop"""
    n16, n_tail = nbytes // 16, (nbytes % 16) // 4
    grid = min(max(-(-n16 // SUM_CHUNKS_PER_GROUP), 1), SUM_GRID_CAP)
    stride, i, unrolled, rest = grid * 256, 0, 0, 0
    while i + 3 * stride < n16:
        i, unrolled = i + 4 * stride, unrolled + 1
    while i < n16:
        i, rest = i + stride, rest + 1
    return dict(n16=n16, n_tail=n_tail, grid=grid, uncapped=-(-n16 // SUM_CHUNKS_PER_GROUP), unrolled=unrolled, rest=rest)


# ---- the fill pattern and the sum's reference -----------------------------------------------------------------------------------------------------
def mix32_np(z):
    z = np.asarray(z, dtype=np.uint32)
    z = (z ^ (z >> np.uint32(16))) * np.uint32(0x7FEB352D)
    z = (z ^ (z >> np.uint32(15))) * np.uint32(0x846CA68B)
    return z ^ (z >> np.uint32(16))


def pattern(n_words, tag):
    """uint32[n_words], word i = mix32(i ^ tag): a function of the position, so a chunk that lands in the wrong place is visible"""
    return mix32_np(np.arange(n_words, dtype=np.uint32) ^ np.uint32(tag))


def word_sum(words):
    """the sum of 32-bit words modulo 2^64"""
    words = np.asarray(words)
    assert words.dtype == np.uint32
    return int(words.astype(np.uint64).sum(dtype=np.uint64)) & M64
