"""The EXPECTED VALUE of the edge-weighted last hop (INTEGRATION.md "Edge-weighted sums", GPUMemoryPool_SetAggEdgeWeight) as a NumPy statement
in np.float32 over an eidref.run_batch batch, shared by the CPU and the GPU tests.  A helper module, not collected by pytest.

  e(i, j)   = the COO edge of the j-th draw of run i: (edges of the hops < H) + (slots with a draw in front of it, in slot order)
  S_e[i, :] = ((+0.0f + fl32(edge_w[e(i, j0)] * x[c(i, j0)])) + fl32(edge_w[e(i, j1)] * x[c(i, j1)])) + ...    ascending slot; product rounded,
                                                                                                               then the add
The draws come from the batch itself (ref["draws"]: what every slot parked), not from a rule's count of them: the rules by weight draw
min(columns of weight > 0, fan-out) per row, the others min(degree, fan-out)."""
import numpy as np

from aggref import cum_edges


def last_hop_slots(ref, indptr, fanout):
    """(n_in, N, run_dst, has, edge): rows before the last hop, its input slots ("runs"), the batch position of every run's input node, which
    of the [N, f] slots hold a draw and the COO edge of each that does (-1 elsewhere)."""
    nc, ec = np.asarray(ref["nc"]), np.asarray(ref["ec"])
    H, f = len(fanout), int(fanout[-1])
    n_in = int(nc[3 + 2 * H])
    if H == 1:
        N = int(nc[4])
        run_dst = np.arange(N, dtype=np.int64)
    else:
        run_dst = np.asarray(ref["src_off"][cum_edges(ec, H - 2):cum_edges(ec, H - 1)], dtype=np.int64)
        N = len(run_dst)
    parked = np.asarray(ref["draws"][H - 1]).reshape(N, f)
    has = parked >= 0
    e_in, E = cum_edges(ec, H - 1), cum_edges(ec, H)
    assert int(has.sum()) == E - e_in, (int(has.sum()), E - e_in)
    edge = np.where(has, e_in + (np.cumsum(has.reshape(-1)).reshape(N, f) - has), -1).astype(np.int64)
    # self-checks of the invariant the statement rests on: edge e(i, j) leads to the node slot (i, j) parked, out of run i's input row
    src = np.asarray(ref["src_off"][:E], dtype=np.int64)
    assert np.array_equal(np.asarray(ref["ids"])[src[edge[has]]], parked[has])
    row = np.asarray(ref["ids"], dtype=np.int64)[run_dst] if N else np.zeros(0, np.int64)
    lo, hi = np.asarray(indptr)[np.where(row >= 0, row, 0)], np.asarray(indptr)[np.where(row >= 0, row, 0) + 1]
    eid = np.asarray(ref["edge_ids"], dtype=np.int64)
    run_of = np.repeat(np.arange(N), has.sum(axis=1))
    assert ((lo[run_of] <= eid[e_in:E]) & (eid[e_in:E] < hi[run_of])).all()
    return n_in, N, run_dst, has, edge


def expected_nbr_sum_edge(ref, indptr, indices, fanout, x=None):
    """(n_in, N, run_dst, S_e).  ref: an eidref.run_batch batch (draws, edge_ids, edge_w); x: the feature rows by batch position (default:
    ref["features"]).  Vectorised over the runs without changing the order of any run's adds: step j adds the weighted draw of slot j of every
    run that has one; the product is a float32 array (rounded) before the add sees it."""
    x = np.asarray(ref["features"] if x is None else x, dtype=np.float32)
    f = int(fanout[-1])
    n_in, N, run_dst, has, edge = last_hop_slots(ref, indptr, fanout)
    src = np.asarray(ref["src_off"], dtype=np.int64)
    ew = np.asarray(ref["edge_w"])
    assert ew.dtype == np.float32
    S = np.zeros((N, x.shape[1]), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for j in range(f):
            m = has[:, j]
            if m.any():
                e = edge[m, j]
                prod = ew[e][:, None] * x[src[e]]             # float32 * float32 -> float32: one rounding
                assert prod.dtype == np.float32
                S[m] = S[m] + prod                             # ... and the add its own
    return n_in, N, run_dst, S
