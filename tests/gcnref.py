"""The EXPECTED VALUE of the normalised last hop (INTEGRATION.md "Normalised sums") as a NumPy statement in np.float32 over a DEFAULT-mode
batch of a reference implementation and the input graph, shared by the CPU and the GPU tests.  A helper module, not collected by pytest.

  d[p]      = #{ e < E : src_off[e] == p }                      out-degree of batch position p inside block 1 (np.bincount)
  w[p]      = fl32(1 / fl32(sqrt(float32(max(d[p], 1)))))       IEEE sqrt and divide, each correctly rounded (NumPy's are)
  S_w[i, :] = ((+0.0f + fl32(w[p0] * x[c0])) + fl32(w[p1] * x[c1])) + ...    the draws of run i in slot order; product rounded, then the add
"""
import numpy as np

from aggref import cum_edges, last_hop_runs


def block_out_degree(ref, fanout):
    """(d, w) of a default-mode batch: int32 [n] and float32 [n], n = nc[5 + 2H]; all E = ec[2 + H] edges of block 1 are counted."""
    H = len(fanout)
    n, E = int(ref["nc"][5 + 2 * H]), cum_edges(ref["ec"], H)
    src = np.asarray(ref["src_off"][:E], dtype=np.int64)
    assert len(src) == E and (E == 0 or (0 <= src.min() and src.max() < n))
    d = np.bincount(src, minlength=n).astype(np.int32)
    w = np.float32(1) / np.sqrt(d.clip(1).astype(np.float32))
    assert d.shape == (n,) and w.dtype == np.float32
    return d, w


def expected_nbr_sum_norm(ref, indptr, indices, fanout, x=None):
    """(n_in, N, run_dst, S_w, d).  x: the reference's feature rows by batch position (default: ref["features"]).  Vectorised over the
    runs like aggref.expected_nbr_sum, without changing the order of any run's adds: step j adds the j-th weighted draw of every run
    that has one; the product is a float32 array (rounded) before the add sees it."""
    x = np.asarray(ref["features"] if x is None else x, dtype=np.float32)
    H, f = len(fanout), int(fanout[-1])
    n_in, N, run_dst, cnt = last_hop_runs(ref, indptr, indices, fanout)
    d, w = block_out_degree(ref, fanout)
    e0, e1 = cum_edges(ref["ec"], H - 1), cum_edges(ref["ec"], H)
    src, dst = np.asarray(ref["src_off"][e0:e1], dtype=np.int64), np.asarray(ref["dst_off"][e0:e1], dtype=np.int64)
    assert int(cnt.sum()) == e1 - e0, (int(cnt.sum()), e1 - e0)
    # the last hop's COO slice is exactly the runs, in order.  At H = 1 a seed list may hold duplicates (link-prediction triples): the runs
    # stay one per seed SLOT, and the edges of a slot name the seed's position, which is its last occurrence (the reference's position_map)
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
            p = src[start[m] + j]
            prod = w[p][:, None] * x[p]                  # float32 * float32 -> float32: one rounding
            assert prod.dtype == np.float32
            S[m] = S[m] + prod                            # ... and the add its own
    return n_in, N, run_dst, S, d
