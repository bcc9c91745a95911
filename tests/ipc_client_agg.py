"""Trainer-side process of the aggregated hand-off tests: attaches through `ipc_service` to a server that runs with LEGION_AGG_LAST_HOP=1.
usage: ipc_client_agg.py <feature_dim> <epochs> <out.json>          every batch of the schedule through get_next_aggregated, one record each
       ipc_client_agg.py <feature_dim> refuse "<error text>"        consume until get_next_aggregated raises; exit 0 = that text after one good batch"""
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
    feat_dim = int(sys.argv[1])
    torch.cuda.set_device(0)
    ipc_service.initialize()
    print("ATTACHED", flush=True)
    assert ipc_service.aggregated() is True
    try:
        ipc_service.get_next(feat_dim)
        raise SystemExit("get_next did not refuse an aggregated server")
    except RuntimeError as e:
        assert "neighbour sums" in str(e) and "get_next_aggregated" in str(e), str(e)
    hops = ipc_service.get_hops()
    sampling = ipc_service.sampling()
    if sys.argv[2] == "refuse":
        good = 0
        try:
            for _ in range(3):
                out = ipc_service.get_next_aggregated(feat_dim)
                good += 1
                print("BATCH", [tuple(t.shape) for t in out], flush=True)
                ipc_service.synchronize()
        except RuntimeError as e:
            print("RAISED after %d good batches:" % good, str(e).splitlines()[0], flush=True)
            ipc_service.finalize()
            sys.exit(0 if (sys.argv[3] in str(e) and good == 1) else 5)
        sys.exit(7)
    epochs, out_path = int(sys.argv[2]), sys.argv[3]
    train_steps, valid_steps, test_steps = ipc_service.get_steps()
    recs = []
    for b in range((train_steps + valid_steps) * epochs + test_steps):
        t = ipc_service.get_next_aggregated(feat_dim)
        sizes = ipc_service.get_block_size()
        assert len(t) == 3 + 2 * hops + 1
        ids, x_in, labels, nbr_sum = t[0], t[1], t[2], t[-1]
        assert x_in.shape == (sizes[1], feat_dim) and nbr_sum.shape[1] == feat_dim and nbr_sum.dtype == torch.float32
        assert nbr_sum.data_ptr() == x_in.data_ptr() + x_in.numel() * 4          # the same buffer, behind the n_in feature rows
        torch.cuda.synchronize()
        recs.append(dict(b=b, n=int(ids.shape[0]), n_in=int(x_in.shape[0]), runs=int(nbr_sum.shape[0]), sizes=list(sizes), ids=sha(ids), features=sha(x_in),
                         labels=sha(labels), edges=[int(t[3 + 2 * k].numel()) for k in range(hops)], src=sha(t[3]), dst=sha(t[4]), nbr_sum=sha(nbr_sum)))
        ipc_service.synchronize()
    ipc_service.finalize()
    with open(out_path, "w") as f:
        json.dump(dict(steps=[train_steps, valid_steps, test_steps], hops=hops, sampling=sampling, batches=recs), f)


if __name__ == "__main__":
    main()
