"""Trainer-side process of the normalised hand-off tests: attaches through `ipc_service` to a server that runs with LEGION_AGG_LAST_HOP=1
LEGION_AGG_NORM=both.
usage: ipc_client_agg_norm.py <feature_dim> <epochs> <out.json>     every batch of the schedule through get_next_aggregated_norm, one record each"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legion-1_amd", "ipc_service"))
import ipc_service  # noqa: E402


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def main():
    feat_dim, epochs, out_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    torch.cuda.set_device(0)
    ipc_service.initialize()
    print("ATTACHED", flush=True)
    assert ipc_service.aggregated() is True and ipc_service.aggregate_norm() == 1
    for wrong, words in ((ipc_service.get_next, ("neighbour sums", "get_next_aggregated")),
                         (ipc_service.get_next_aggregated, ("LEGION_AGG_NORM=both", "get_next_aggregated_norm"))):
        try:
            wrong(feat_dim)
            raise SystemExit("%s did not refuse a normalising server" % wrong.__name__)
        except RuntimeError as e:
            assert all(w in str(e) for w in words), str(e)
    hops = ipc_service.get_hops()
    sampling = ipc_service.sampling()
    train_steps, valid_steps, test_steps = ipc_service.get_steps()
    recs = []
    for b in range((train_steps + valid_steps) * epochs + test_steps):
        t = ipc_service.get_next_aggregated_norm(feat_dim)
        sizes = ipc_service.get_block_size()
        assert len(t) == 3 + 2 * hops + 1
        ids, x_in, labels, nbr_sum = t[0], t[1], t[2], t[-1]
        assert x_in.shape == (sizes[1], feat_dim) and nbr_sum.shape[1] == feat_dim and nbr_sum.dtype == torch.float32
        assert nbr_sum.data_ptr() == x_in.data_ptr() + x_in.numel() * 4          # the same buffer, behind the n_in feature rows
        torch.cuda.synchronize()
        recs.append(dict(b=b, n=int(ids.shape[0]), n_in=int(x_in.shape[0]), runs=int(nbr_sum.shape[0]), sizes=list(sizes), ids=sha(ids), features=sha(x_in),
                         labels=sha(labels), edges=[int(t[3 + 2 * k].numel()) for k in range(hops)], src=sha(t[3]), dst=sha(t[4]), nbr_sum=sha(nbr_sum),
                         out_deg=sha(torch.bincount(t[3].long(), minlength=int(ids.shape[0])).int())))   # what the trainer counts itself
        ipc_service.synchronize()
    ipc_service.finalize()
    with open(out_path, "w") as f:
        json.dump(dict(steps=[train_steps, valid_steps, test_steps], hops=hops, sampling=sampling, batches=recs), f)


if __name__ == "__main__":
    main()
