"""Trainer-side process of the seeded-sampling tests: tests/ipc_client_sampling.py's loop on a server started with (or without)
LEGION_SAMPLING_SEED, plus what ipc_service.sampling_seed() said and the seed part of every batch.
usage: ipc_client_seed.py <feature_dim> <epochs> <out.json>"""
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
    feat_dim, epochs, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    torch.cuda.set_device(0)
    ipc_service.initialize()
    print("ATTACHED", flush=True)
    seed, sampling = ipc_service.sampling_seed(), ipc_service.sampling()
    train_steps, valid_steps, test_steps = ipc_service.get_steps()
    hops = ipc_service.get_hops()
    recs = []
    for b in range((train_steps + valid_steps) * epochs + test_steps):
        tensors = ipc_service.get_next(feat_dim)
        sizes = ipc_service.get_block_size()
        ids, feats, labels = tensors[:3]
        blocks = tensors[3:]
        assert len(blocks) == 2 * hops and feats.shape == (ids.shape[0], feat_dim)
        torch.cuda.synchronize()
        recs.append(dict(b=b, n=int(ids.shape[0]), sizes=list(sizes), ids=sha(ids), features=sha(feats), labels=sha(labels),
                         edges=[int(blocks[2 * k].numel()) for k in range(hops)], src=sha(blocks[0]), dst=sha(blocks[1]),
                         seeds=ids[:labels.shape[0]].cpu().tolist()))
        ipc_service.synchronize()
    ipc_service.finalize()
    with open(out, "w") as f:
        json.dump(dict(steps=[train_steps, valid_steps, test_steps], hops=hops, sampling=sampling, sampling_seed=seed, batches=recs), f)


if __name__ == "__main__":
    main()
