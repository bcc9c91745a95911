"""Trainer-side process of the serving-mode tests: attaches through `ipc_service` to a server in any hand-off, sampling mode and seeding, and
reads every batch through the get_next* of the hand-off the SERVER says it is in.  <hand-off> is what the test expects of the server (plain |
agg: LEGION_AGG_LAST_HOP=1 | norm: ... LEGION_AGG_NORM=both): a server that says otherwise ends the client with exit code 9 before any batch.
usage: ipc_client_modes.py <hand-off> <feature_dim> <epochs> <out.json>     every batch of the schedule, one record each
       ipc_client_modes.py <hand-off> <feature_dim> refuse "<error text>"   consume until the call raises; exit 0 = that text after one good batch"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legion-1_amd", "ipc_service"))
import ipc_service  # noqa: E402

# hand-off -> (the call that reads its batches, the other calls with the words their refusal carries on such a server)
HAND_OFFS = {
    "plain": ("get_next", ()),
    "agg": ("get_next_aggregated", (("get_next", ("neighbour sums", "get_next_aggregated")),)),
    "norm": ("get_next_aggregated_norm", (("get_next", ("neighbour sums", "get_next_aggregated")),
                                          ("get_next_aggregated", ("LEGION_AGG_NORM=both", "get_next_aggregated_norm")))),
}


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def expect_hand_off(expected):
    """The hand-off the attached server says it is in; exit code 9 when the test expects another (selecting the call by the server's own
    word must not hide a server that booted in the wrong mode)."""
    hand_off = ("norm" if ipc_service.aggregate_norm() else "agg") if ipc_service.aggregated() else "plain"
    if hand_off != expected:
        print("the server's hand-off is %r, the test expects %r" % (hand_off, expected), flush=True)
        sys.exit(9)
    return hand_off


def main():
    feat_dim = int(sys.argv[2])
    torch.cuda.set_device(0)
    ipc_service.initialize()
    print("ATTACHED", flush=True)
    hand_off = expect_hand_off(sys.argv[1])
    aggregated = hand_off != "plain"
    assert ipc_service.aggregated() is aggregated and ipc_service.aggregate_norm() == int(hand_off == "norm")
    call, wrong_calls = HAND_OFFS[hand_off]
    get_next = getattr(ipc_service, call)
    for wrong, words in wrong_calls:
        try:
            getattr(ipc_service, wrong)(feat_dim)
            raise SystemExit("%s did not refuse a server in the %s hand-off" % (wrong, hand_off))
        except RuntimeError as e:
            assert all(w in str(e) for w in words), str(e)
    hops = ipc_service.get_hops()
    sampling, seed = ipc_service.sampling(), ipc_service.sampling_seed()
    if sys.argv[3] == "refuse":
        good = 0
        try:
            for _ in range(3):
                out = get_next(feat_dim)
                good += 1
                print("BATCH", [tuple(t.shape) for t in out], flush=True)
                ipc_service.synchronize()
        except RuntimeError as e:
            print("RAISED after %d good batches:" % good, str(e).splitlines()[0], flush=True)
            ipc_service.finalize()
            sys.exit(0 if (sys.argv[4] in str(e) and good == 1) else 5)
        sys.exit(7)
    epochs, out_path = int(sys.argv[3]), sys.argv[4]
    train_steps, valid_steps, test_steps = ipc_service.get_steps()
    recs = []
    for b in range((train_steps + valid_steps) * epochs + test_steps):
        t = get_next(feat_dim)
        sizes = ipc_service.get_block_size()
        assert len(t) == 3 + 2 * hops + int(aggregated)
        ids, feats, labels = t[:3]
        rec = dict(b=b, n=int(ids.shape[0]), sizes=list(sizes), edges=[int(t[3 + 2 * k].numel()) for k in range(hops)])
        if aggregated:
            nbr_sum = t[-1]
            assert feats.shape == (sizes[1], feat_dim) and nbr_sum.shape[1] == feat_dim and nbr_sum.dtype == torch.float32
            assert nbr_sum.data_ptr() == feats.data_ptr() + feats.numel() * 4          # the same buffer, behind the n_in feature rows
            rec.update(n_in=int(feats.shape[0]), runs=int(nbr_sum.shape[0]))
        else:
            assert feats.shape == (ids.shape[0], feat_dim)
        torch.cuda.synchronize()
        rec.update(ids=sha(ids), features=sha(feats), labels=sha(labels), src=sha(t[3]), dst=sha(t[4]), seeds=ids[:labels.shape[0]].cpu().tolist(),
                   out_deg=sha(torch.bincount(t[3].long(), minlength=int(ids.shape[0])).int()))   # what the trainer counts itself
        recs.append(dict(rec, nbr_sum=sha(nbr_sum)) if aggregated else rec)
        ipc_service.synchronize()
    ipc_service.finalize()
    with open(out_path, "w") as f:
        json.dump(dict(steps=[train_steps, valid_steps, test_steps], hops=hops, hand_off=hand_off, sampling=sampling, sampling_seed=seed, batches=recs), f)


if __name__ == "__main__":
    main()
