"""The distinct-draw sampler mode (GPUMemoryPool_SetSampleDistinct / LEGION_SAMPLING=distinct, INTEGRATION.md "Sampling without
replacement") as a NumPy statement, shared by the CPU and the GPU tests.  A helper module, not collected by pytest.

For hop h (1-based, op_id / 2), row i of that hop's input list (slot idx = i * f + j), degree d (the int32 indptr difference) and fan-out f:

  slot j >= d      no draw
  d <= f           slot j < d takes neighbour position j
  d >  f           Floyd's algorithm on hashed randoms, all uint32 with wrap-around except the one 64-bit product:
                     mix32(z): z ^= z >> 16; z *= 0x7feb352d; z ^= z >> 15; z *= 0x846ca68b; z ^= z >> 16
                     K = mix32(i + 0x9E3779B9 * h)
                     t = 0 .. f-1:  J = d - f + t;  u = mix32(K ^ (0x85EBCA6B * (t + 1)));  r = (uint64(u) * (J + 1)) >> 32
                                    pick[t] = J if r is among pick[0..t-1] else r
                   slot j takes neighbour position pick[j]

Everything behind the position is the default mode's bookkeeping (tests/pyref.py): the dst < 0 rule, first occurrence by ascending slot,
the counters, both COO arrays.  run_batch() restates that bookkeeping vectorised (a few million slots per batch are practical) with the
draw function as a parameter, so that the same code fed with pyref.sample_index must reproduce pyref.run_batch."""
import numpy as np

M32 = 0xFFFFFFFF
GOLDEN, STEP = 0x9E3779B9, 0x85EBCA6B


# ---- scalar, plain Python ints -------------------------------------------------------------------
def mix32_scalar(z):
    z &= M32
    z ^= z >> 16
    z = (z * 0x7feb352d) & M32
    z ^= z >> 15
    z = (z * 0x846ca68b) & M32
    z ^= z >> 16
    return z


def picks_scalar(i, h, d, f):
    """The positions of the slots 0..f-1 of row i of hop h; -1 = no draw."""
    if d <= f:
        return [j if j < d else -1 for j in range(f)]
    K = mix32_scalar(i + GOLDEN * h)
    pick = []
    for t in range(f):
        J = d - f + t
        u = mix32_scalar(K ^ ((STEP * (t + 1)) & M32))
        r = (u * (J + 1)) >> 32
        pick.append(J if r in pick else r)
    return pick


# ---- vectorised ----------------------------------------------------------------------------------
def mix32(z):
    z = np.array(z, dtype=np.uint32, copy=True, ndmin=1)
    z ^= z >> np.uint32(16)
    z *= np.uint32(0x7feb352d)           # uint32 arrays wrap
    z ^= z >> np.uint32(15)
    z *= np.uint32(0x846ca68b)
    z ^= z >> np.uint32(16)
    return z


def positions(rows, hop, deg, f):
    """int64 [n, f]: the position slot j of row rows[m] of hop hop (scalar or [n]) takes at degree deg[m]; -1 = no draw."""
    rows = np.asarray(rows, dtype=np.int64)
    deg = np.asarray(deg, dtype=np.int64)
    hop = np.broadcast_to(np.asarray(hop, dtype=np.int64), rows.shape)
    n, f = len(rows), int(f)
    j = np.arange(f, dtype=np.int64)
    out = np.where(j[None, :] < deg[:, None], j[None, :], -1)            # d <= f (and, overwritten below, d > f)
    big = np.nonzero(deg > f)[0]
    if len(big):
        d = deg[big]
        K = mix32(((rows[big] + GOLDEN * hop[big]) & M32).astype(np.uint32))
        pick = np.empty((len(big), f), dtype=np.int64)
        for t in range(f):
            J = d - f + t
            u = mix32(K ^ np.uint32((STEP * (t + 1)) & M32))
            r = ((u.astype(np.uint64) * (J + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
            hit = (pick[:, :t] == r[:, None]).any(axis=1) if t else np.zeros(len(big), bool)
            pick[:, t] = np.where(hit, J, r)
        out[big] = pick
    return out


def pyref_positions(rows, hop, deg, f):
    """The default mode's draws in the same shape (pyref.sample_index per slot, slot index = row * f + j): run_batch(draw=pyref_positions)
    must be pyref.run_batch."""
    import pyref
    out = np.full((len(rows), f), -1, dtype=np.int64)
    for m, (i, d) in enumerate(zip(np.asarray(rows).tolist(), np.asarray(deg).tolist())):
        for j in range(min(max(d, 0), f)):
            out[m, j] = pyref.sample_index(i * f + j, d)
    return out


# ---- the whole batch -----------------------------------------------------------------------------
def run_batch(indptr, indices, feats, all_ids, all_labels, batch_size, counter, fanout, draw=positions):
    """pyref.run_batch's batch with the neighbour position of a slot taken from `draw`.  Returns nc, ec, ids, labels, src_off, dst_off,
    features as pyref does, and draws: per hop the int32 [N * f] neighbour id every slot parked (-1 = no draw / a hole), and
    draw_counts: per hop (input node ids [N], draws per row [N]) -- what pre-sampling adds to edge_access_time."""
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    V, H, total_cap = len(indptr) - 1, len(fanout), len(all_ids)
    nc, ec = [0] * 16, [0] * 16
    size = (total_cap - batch_size * counter) if batch_size * (counter + 1) >= total_cap else batch_size
    size = max(size, 0)
    g = size * counter + np.arange(size, dtype=np.int64)
    ok = g < total_cap
    ids = np.where(ok, np.asarray(all_ids, dtype=np.int64)[g % max(total_cap, 1)], -1) if size else np.zeros(0, np.int64)
    labels = np.where(ok, np.asarray(all_labels, dtype=np.int64)[g % max(total_cap, 1)], -1) if size else np.zeros(0, np.int64)
    pos = np.full(V, -1, dtype=np.int64)                     # position_map of this batch; a repeated seed keeps its LAST occurrence
    live = np.nonzero(ids >= 0)[0]
    u, first_rev = np.unique(ids[live][::-1], return_index=True)
    pos[u] = live[::-1][first_rev]
    nc[0] = size; nc[2] = size; nc[3] = 0; nc[4] = size
    agg_src = np.zeros(0, np.int64)
    src_off, dst_off, draws, draw_counts = [], [], [], []
    for h in range(1, H + 1):
        f, N = int(fanout[h - 1]), nc[2]
        inp = ids[:N] if h == 1 else agg_src[ec[2]:ec[2] + N]
        valid = inp >= 0
        s = np.where(valid, inp, 0)
        start = indptr[s].astype(np.int64)
        deg = np.where(valid, (indptr[s + 1] - indptr[s]).astype(np.int32).astype(np.int64), -1)
        p = draw(np.arange(N, dtype=np.int64), h, deg, f)                   # [N, f]
        has = p >= 0
        dst = np.where(has, indices[np.where(has, start[:, None] + p, 0)].astype(np.int64), -1)
        has &= dst >= 0                                                     # a hole (-1 neighbour) is no edge
        dst = np.where(has, dst, -1)
        draws.append(dst.reshape(-1).astype(np.int32))
        draw_counts.append((inp.copy(), has.sum(axis=1)))
        e_src = dst[has]                                                    # row-major = ascending slot
        e_dst = np.repeat(inp, has.sum(axis=1))
        fresh = e_src[pos[e_src] < 0]
        _, first = np.unique(fresh, return_index=True)
        new_nodes = fresh[np.sort(first)]                                   # first occurrence by ascending slot
        pos[new_nodes] = nc[0] + np.arange(len(new_nodes), dtype=np.int64)
        ids = np.concatenate([ids, new_nodes])
        agg_src = np.concatenate([agg_src, e_src])
        src_off.append(pos[e_src]); dst_off.append(pos[e_dst])
        nc[1], ec[1] = len(new_nodes), len(e_src)
        nc[0] += nc[1]
        nc[3 + 2 * h] = nc[1 + 2 * h] + nc[2 + 2 * h]
        nc[4 + 2 * h] = nc[1]
        if h == H:
            nc[5 + 2 * h] = nc[3 + 2 * h] + nc[4 + 2 * h]
        nc[1] = 0
        nc[2] = ec[1]
        ec[2 + h] = ec[0] + ec[1]
        ec[2] = ec[0]
        ec[0] += ec[1]
        ec[1] = 0
    n = nc[5 + 2 * H]
    ids = ids[:n]
    feats = np.asarray(feats)
    out_feat = np.zeros((n, feats.shape[1]), dtype=np.float32)
    keep = ids >= 0
    out_feat[keep] = feats[ids[keep] % V]
    cat = lambda parts: (np.concatenate(parts) if parts else np.zeros(0, np.int64)).astype(np.int32)
    return dict(nc=np.array(nc, np.int32), ec=np.array(ec, np.int32), ids=ids.astype(np.int32), labels=labels.astype(np.int32),
                src_off=cat(src_off), dst_off=cat(dst_off), features=out_feat, draws=draws, draw_counts=draw_counts)


def chi2_cap(dof, p_tail=1e-6):
    """The chi-square quantile at 1 - p_tail: scipy's, else Wilson-Hilferty with z = 4.7534 (p_tail = 1e-6 only), which sits above the exact
    quantile at small degrees of freedom."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - p_tail, dof))
    except ImportError:
        assert p_tail == 1e-6
        z = 4.7534
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * (2.0 / (9.0 * dof)) ** 0.5) ** 3
