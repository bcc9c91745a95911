"""Trainer-side process of the served-edges tests: tests/ipc_client_modes.py's records of every batch -- the same keys, so the two can be held
against each other -- plus what a server with LEGION_EDGE_IDS=1 hands over beside them and the serving modes it publishes.  <hand-off> is what the
test expects of the server: plain | agg | norm as in ipc_client_modes.py, edge = LEGION_AGG_EDGE_WEIGHT=1 (get_next_aggregated_edge_weight).
usage: ipc_client_edges.py <hand-off> <feature_dim> <epochs> <out.json>
Writes out.json (modes, the refusals' texts, one record per batch: per block the SHA-256 of its edge ids and of its edge weights' bytes) and
out.json.npz: batch 0 raw (ids, src, dst, edge_ids, edge_w) and, in the edge hand-off, every batch's x_in and neighbour sums."""
import json
import sys

import numpy as np
import torch

from ipc_client_modes import ipc_service, sha

CALLS = dict(plain="get_next", agg="get_next_aggregated", norm="get_next_aggregated_norm", edge="get_next_aggregated_edge_weight")


def refusal(call, *args):
    """the first line of what the call raises; None when it returns"""
    try:
        call(*args)
    except RuntimeError as e:
        return str(e).splitlines()[0]
    return None


def main():
    expected, feat_dim, epochs, out_path = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    torch.cuda.set_device(0)
    ipc_service.initialize()
    print("ATTACHED", flush=True)
    modes = dict(lp_draw=ipc_service.lp_draw(), weighted_distinct=ipc_service.weighted_distinct(), shared_draws=ipc_service.shared_draws(),
                 edge_ids=ipc_service.edge_ids(), edge_weights=ipc_service.edge_weights(), agg_edge_weight=ipc_service.aggregate_edge_weight())
    hand_off = "edge" if modes["agg_edge_weight"] else ("norm" if ipc_service.aggregate_norm() else "agg") if ipc_service.aggregated() else "plain"
    if hand_off != expected:
        print("the server's hand-off is %r, the test expects %r" % (hand_off, expected), flush=True)
        sys.exit(9)
    aggregated = hand_off != "plain"
    refused = {name: refusal(getattr(ipc_service, name), feat_dim) for h, name in CALLS.items() if h != hand_off}     # every wrong call, before any batch
    refused["get_edge_ids_before"] = refusal(ipc_service.get_edge_ids)
    refused["get_edge_weights_before"] = refusal(ipc_service.get_edge_weights)
    get_next = getattr(ipc_service, CALLS[hand_off])
    hops = ipc_service.get_hops()
    train_steps, valid_steps, test_steps = ipc_service.get_steps()
    recs, raw = [], {}
    for b in range((train_steps + valid_steps) * epochs + test_steps):
        t = get_next(feat_dim)
        sizes = ipc_service.get_block_size()
        assert len(t) == 3 + 2 * hops + int(aggregated)
        ids, feats, labels = t[:3]
        rec = dict(b=b, n=int(ids.shape[0]), sizes=list(sizes), edges=[int(t[3 + 2 * k].numel()) for k in range(hops)])
        if aggregated:
            nbr_sum = t[-1]
            assert feats.shape == (sizes[1], feat_dim) and nbr_sum.shape[1] == feat_dim and nbr_sum.dtype == torch.float32
            rec.update(n_in=int(feats.shape[0]), runs=int(nbr_sum.shape[0]))
        else:
            assert feats.shape == (ids.shape[0], feat_dim)
        torch.cuda.synchronize()
        rec.update(ids=sha(ids), features=sha(feats), labels=sha(labels), src=sha(t[3]), dst=sha(t[4]), seeds=ids[:labels.shape[0]].cpu().tolist(),
                   out_deg=sha(torch.bincount(t[3].long(), minlength=int(ids.shape[0])).int()))
        if aggregated:
            rec["nbr_sum"] = sha(nbr_sum)
        if modes["edge_ids"]:
            eid = ipc_service.get_edge_ids()
            assert len(eid) == hops and all(e.dtype == torch.int64 and e.is_cuda and e.dim() == 1 for e in eid)
            assert [int(e.numel()) for e in eid] == rec["edges"] and len({e.data_ptr() for e in eid}) == 1      # prefixes of one buffer, like src / dst
            rec["eid"] = [sha(e) for e in eid]
            if modes["edge_weights"]:
                ew = ipc_service.get_edge_weights()
                assert len(ew) == hops and all(w.dtype == torch.float32 and w.is_cuda for w in ew) and [int(w.numel()) for w in ew] == rec["edges"]
                rec["ew"] = [sha(w) for w in ew]
            elif b == 0:
                refused["get_edge_weights"] = refusal(ipc_service.get_edge_weights)
            if b == 0:
                raw.update(ids=ids.cpu().numpy(), src=t[3].cpu().numpy(), dst=t[4].cpu().numpy(), edge_ids=eid[0].cpu().numpy())
                if modes["edge_weights"]:
                    raw["edge_w"] = ew[0].cpu().numpy()
        elif b == 0:
            refused["get_edge_ids"] = refusal(ipc_service.get_edge_ids)
            refused["get_edge_weights"] = refusal(ipc_service.get_edge_weights)
        if hand_off == "edge":
            raw["x_in_%d" % b], raw["nbr_sum_%d" % b] = feats.cpu().numpy(), nbr_sum.cpu().numpy()
        recs.append(rec)
        ipc_service.synchronize()
        if b == 0 and modes["edge_ids"]:
            refused["get_edge_ids_after_synchronize"] = refusal(ipc_service.get_edge_ids)                       # the views were valid until synchronize()
    sampling, seed = ipc_service.sampling(), ipc_service.sampling_seed()
    ipc_service.finalize()
    np.savez(out_path + ".npz", **raw)
    with open(out_path, "w") as f:
        json.dump(dict(steps=[train_steps, valid_steps, test_steps], hops=hops, hand_off=hand_off, sampling=sampling, sampling_seed=seed, modes=modes,
                       refused=refused, batches=recs), f)


if __name__ == "__main__":
    main()
