"""The EXPECTED VALUE of the aggregated last hop as a NumPy statement over a DEFAULT-mode batch of a reference implementation and the
input graph (tests/test_agg_last_hop_cpu.py says why), shared by the CPU and the GPU tests.  A helper module, not collected by pytest."""
import numpy as np

import pyref


def cum_edges(ec, h):
    """edges of hops 1..h of a batch (apply_update_counter's layout: ec[2 + h] is cumulative; ec[2] is not a total)"""
    return 0 if h == 0 else int(ec[2 + h])


def sample_indices(idx, deg):
    """pyref.sample_index over arrays: 48271^(idx + 1) mod (2^31 - 1) by square-and-multiply in uint64 (every product < 2^62), then the
    same IEEE double arithmetic.  tests/test_agg_numerics_cpu.py holds it against pyref.sample_index."""
    idx, deg = np.asarray(idx, dtype=np.int64), np.asarray(deg, dtype=np.int64)
    M = np.uint64(pyref.M31)
    e = (idx + 1).astype(np.uint64)
    x, b = np.ones(idx.shape, np.uint64), np.full(idx.shape, 48271, np.uint64)
    while e.any():
        x = np.where(e & np.uint64(1), x * b % M, x)
        b = b * b % M
        e = e >> np.uint64(1)
    r = (x.astype(np.int64) - 1).astype(np.float64) / np.float64(2147483646.0)
    return (r * deg.astype(np.float64) + np.float64(0.0)).astype(np.int64)


def last_hop_runs(ref, indptr, indices, fanout):
    """(n_in, N, run_dst, cnt) of a default-mode batch: rows before the last hop, the last hop's input slots ("runs"), the batch
    position of every run's input node, and the draws of every run recomputed from the graph -- min(deg, f) for a valid input
    node, 0 for a -1; where the graph has holes (-1 neighbours) every draw is recomputed and the holes are left out."""
    nc, ec = np.asarray(ref["nc"]), np.asarray(ref["ec"])
    H, f = len(fanout), int(fanout[-1])
    ids = np.asarray(ref["ids"])
    n_in = int(nc[3 + 2 * H])
    if H == 1:
        N = int(nc[4])
        run_dst = np.arange(N, dtype=np.int64)
    else:
        e0, e1 = cum_edges(ec, H - 2), cum_edges(ec, H - 1)
        run_dst = np.asarray(ref["src_off"][e0:e1], dtype=np.int64)
        N = e1 - e0
    # the formula the device and the trainer use for N
    assert N == (int(nc[4]) if H == 1 else int(ec[3]) if H == 2 else int(ec[1 + H] - ec[H]))
    L = ids[run_dst] if N else np.zeros(0, np.int32)
    valid = L >= 0
    Ls = np.where(valid, L, 0).astype(np.int64)
    row0 = np.asarray(indptr)[Ls]
    deg = np.asarray(indptr)[Ls + 1] - row0
    cnt = np.where(valid, np.minimum(deg, f), 0).astype(np.int64)
    if (np.asarray(indices) < 0).any():
        run = np.repeat(np.arange(N, dtype=np.int64), cnt)              # one entry per draw: its run, its slot j inside the run
        j = np.arange(len(run), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        hit = np.asarray(indices)[row0[run] + sample_indices(run * f + j, deg[run])] >= 0
        cnt = np.bincount(run[hit], minlength=N).astype(np.int64)
    return n_in, N, run_dst, cnt


def expected_nbr_sum(ref, indptr, indices, fanout, x=None):
    """S[i, :] = ((0.0f + x[c(i, j0)]) + x[c(i, j1)]) + ... in np.float32, edge order.  x: the reference's feature rows by batch
    position (default: ref["features"]).  Vectorised over the runs without changing the order of any run's adds: step j adds the
    j-th draw of every run that has one."""
    x = np.asarray(ref["features"] if x is None else x, dtype=np.float32)
    ec = np.asarray(ref["ec"])
    H, f = len(fanout), int(fanout[-1])
    n_in, N, run_dst, cnt = last_hop_runs(ref, indptr, indices, fanout)
    e0, e1 = cum_edges(ec, H - 1), cum_edges(ec, H)
    src, dst = np.asarray(ref["src_off"][e0:e1], dtype=np.int64), np.asarray(ref["dst_off"][e0:e1], dtype=np.int64)
    # self-checks of the statement: the last hop's COO slice is exactly the runs, in order
    assert int(cnt.sum()) == e1 - e0, (int(cnt.sum()), e1 - e0)
    # At H = 1 a seed list may repeat a seed inside a batch: the runs stay one per seed SLOT, and the edges of a slot name the seed's position,
    # which is its last occurrence (the reference's position_map; tests/gcnref.py has the same rule)
    run_node = run_dst
    if H == 1 and N:
        ids = np.asarray(ref["ids"][:N])
        last = {}
        for i, v in enumerate(ids.tolist()):
            last[v] = i
        run_node = np.array([last[v] for v in ids.tolist()], dtype=np.int64)
    assert np.array_equal(dst, np.repeat(run_node, cnt))
    start = np.cumsum(cnt) - cnt
    S = np.zeros((N, x.shape[1]), dtype=np.float32)
    for j in range(f):
        m = cnt > j
        if m.any():
            S[m] = S[m] + x[src[start[m] + j]]
    return n_in, N, run_dst, S
