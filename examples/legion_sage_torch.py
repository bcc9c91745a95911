#!/usr/bin/env python3
"""GraphSAGE / GCN trainer on top of the sampling server, plain PyTorch (no DGL).

Consumes mini-batches from the `legion` server through `ipc_service` exactly like the reference trainer
(pytorch_extension/legion_graphsage.py:72-172): one process per GPU, `ipc_service.get_next(F)` ->
[ids, features, labels, (src, dst) x H], `get_block_size()` -> (num_src, num_dst) x H, `synchronize()` hands the
buffers back.  The reference builds DGL blocks + `SAGEConv(..., 'mean')`; dgl is not installable here, so the mean
aggregator is written with index_add_ -- the same arithmetic on the same COO blocks (duplicate edges, which sampling
with replacement produces, count twice as in DGL).  Works for any number of hops the server samples.

`--task lp` is the link-prediction variant (pytorch_extension/lp_sage.py:72-97): every training batch is laid out as
three equal thirds [src | pos | neg] (a `trainingset` file written by `legion1_amd.synth.lp_trainingset`), the loss is
-logsigmoid(<h_src, h_pos>) - logsigmoid(-<h_src, h_neg>); validation / test batches are only drained.

    LEGION_TABLES=auto legion-1_amd/csrc/legion 1 0 25,10 meta_config &          # or launch_server.py
    PYTHONPATH=legion-1_amd/ipc_service python examples/legion_sage_torch.py --features_num 100 --class_num 47
"""
import argparse
import os
import time

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
import torch.nn.functional as Func
from torch.nn.parallel import DistributedDataParallel as DDP


class SageMean(nn.Module):
    """h_dst = W_self h_dst + W_neigh mean_{(s,d) in block} h_s + b.  The dst nodes of a block are the first
    num_dst src nodes (sampled_ids lists the seeds first, then the new nodes hop by hop)."""

    def __init__(self, in_feats, out_feats):
        super().__init__()
        self.fc_self = nn.Linear(in_feats, out_feats, bias=False)
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_feats))

    def forward(self, block, h):
        src, dst, num_src, num_dst = block
        assert h.shape[0] == num_src
        agg = torch.zeros(num_dst, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, dst, h.index_select(0, src))
        deg = torch.zeros(num_dst, dtype=h.dtype, device=h.device).index_add_(0, dst, torch.ones_like(dst, dtype=h.dtype))
        agg = agg / deg.clamp(min=1).unsqueeze(1)
        return self.fc_self(h[:num_dst]) + self.fc_neigh(agg) + self.bias


class SageMeanFused(SageMean):
    """First layer behind a server that hands the last hop over as neighbour sums (LEGION_AGG_LAST_HOP=1, ipc_service.get_next_aggregated;
    INTEGRATION.md "Aggregated last hop").  h = x_in[n_in, F]: only the nodes found before the last hop have feature rows.  The edges of
    the hops < H (the first e_in of block 1: all their sources < n_in) are aggregated as SageMean does; the last hop arrives as one row
    of sums per input slot, S[N, F], to be added into node run_dst[i].  Same parameters as SageMean, same result up to fp32 summation order."""

    def forward(self, block, h):
        src, dst, num_src, num_dst, e_in, run_dst, nbr_sum = block
        assert h.shape[0] == num_dst
        agg = torch.zeros(num_dst, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, dst[:e_in], h.index_select(0, src[:e_in]))
        agg += torch.zeros(num_dst, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, run_dst, nbr_sum)
        deg = torch.zeros(num_dst, dtype=h.dtype, device=h.device).index_add_(0, dst, torch.ones_like(dst, dtype=h.dtype))
        agg = agg / deg.clamp(min=1).unsqueeze(1)
        return self.fc_self(h) + self.fc_neigh(agg) + self.bias


def fused_first_block(src, dst, num_src, num_dst, edges_per_block, nbr_sum):
    """Block 1 of an aggregated batch for SageMeanFused.  edges_per_block[k] = edges of block k + 1 (hops 1..H-k): block 2 holds the edges
    of the hops < H, and the destination node of input slot i of the last hop is the source of hop-(H-1) edge i (slot i itself at H = 1)."""
    H = len(edges_per_block)
    e_in = edges_per_block[1] if H >= 2 else 0
    e_prev = edges_per_block[2] if H >= 3 else 0
    run_dst = src[e_prev:e_in] if H >= 2 else torch.arange(nbr_sum.shape[0], device=src.device)
    return (src, dst, num_src, num_dst, e_in, run_dst, nbr_sum)


class GraphConvBoth(nn.Module):
    """DGL GraphConv(norm='both', allow_zero_in_degree=True) as legion_gcn.py:80-87 uses it:
    h_dst = sum_{(s,d)} h_s / sqrt(outdeg_s * indeg_d) W + b, degrees counted inside the block and clamped to >= 1."""

    def __init__(self, in_feats, out_feats):
        super().__init__()
        self.fc = nn.Linear(in_feats, out_feats, bias=True)

    def forward(self, block, h):
        src, dst, num_src, num_dst = block
        one = torch.ones_like(src, dtype=h.dtype)
        out_deg = torch.zeros(num_src, dtype=h.dtype, device=h.device).index_add_(0, src, one).clamp(min=1)
        in_deg = torch.zeros(num_dst, dtype=h.dtype, device=h.device).index_add_(0, dst, one).clamp(min=1)
        m = (h * out_deg.rsqrt().unsqueeze(1)).index_select(0, src)
        agg = torch.zeros(num_dst, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, dst, m)
        return self.fc(agg * in_deg.rsqrt().unsqueeze(1))


class GraphConvBothFused(GraphConvBoth):
    """First layer behind a server that hands the last hop over as out-degree-normalised neighbour sums (LEGION_AGG_LAST_HOP=1
    LEGION_AGG_NORM=both, ipc_service.get_next_aggregated_norm; INTEGRATION.md "Normalised sums").  h = x_in[n_in, F].  Both degrees are
    counted from the COO the trainer gets anyway (4-byte work per edge); the edges of the hops < H (the first e_in of block 1, all their
    sources < n_in) are scaled and aggregated as GraphConvBoth does; the last hop arrives as S_w[N, F], its rows already scaled by
    out_deg^-1/2 and summed per input slot, to be added into node run_dst[i].  Same parameters as GraphConvBoth, same result up to fp32
    summation order."""

    def forward(self, block, h):
        src, dst, num_src, num_dst, e_in, run_dst, nbr_sum = block
        assert h.shape[0] == num_dst
        one = torch.ones_like(src, dtype=h.dtype)
        out_deg = torch.zeros(num_src, dtype=h.dtype, device=h.device).index_add_(0, src, one).clamp(min=1)
        in_deg = torch.zeros(num_dst, dtype=h.dtype, device=h.device).index_add_(0, dst, one).clamp(min=1)
        m = (h * out_deg[:num_dst].rsqrt().unsqueeze(1)).index_select(0, src[:e_in])
        agg = torch.zeros(num_dst, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, dst[:e_in], m)
        agg += torch.zeros(num_dst, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, run_dst, nbr_sum)
        return self.fc(agg * in_deg.rsqrt().unsqueeze(1))


class GraphConvEdgeWeight(nn.Module):
    """DGL GraphConv(norm='none', allow_zero_in_degree=True) with edge_weight=w, PyG GCNConv(normalize=False) with edge_weight:
    h_dst = (sum_{e = (s,d)} w_e h_s) W + b.  block = (src, dst, num_src, num_dst, w), w[e] the weight of COO edge e as the server hands
    it over (LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1, ipc_service.get_edge_weights(); INTEGRATION.md "Edge ids"); duplicate edges count twice."""

    def __init__(self, in_feats, out_feats):
        super().__init__()
        self.fc = nn.Linear(in_feats, out_feats, bias=True)

    def forward(self, block, h):
        src, dst, num_src, num_dst, w = block
        assert h.shape[0] == num_src and w.shape[0] == src.shape[0]
        m = h.index_select(0, src) * w.to(h.dtype).unsqueeze(1)
        return self.fc(torch.zeros(num_dst, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, dst, m))


class GraphConvEdgeWeightFused(GraphConvEdgeWeight):
    """First layer behind a server that hands the last hop over as edge-weighted neighbour sums (LEGION_AGG_EDGE_WEIGHT=1,
    ipc_service.get_next_aggregated_edge_weight; INTEGRATION.md "Edge-weighted sums").  h = x_in[n_in, F].  The edges of the hops < H (the
    first e_in of block 1) are scaled by their served weights and aggregated as GraphConvEdgeWeight does; the last hop arrives as one row
    per input slot, sum_e w_e x[src_e], to be added into node run_dst[i].  Same parameters, same result up to fp32 summation order."""

    def forward(self, block, h):
        src, dst, num_src, num_dst, e_in, run_dst, nbr_sum, w = block
        assert h.shape[0] == num_dst
        m = h.index_select(0, src[:e_in]) * w[:e_in].to(h.dtype).unsqueeze(1)
        agg = torch.zeros(num_dst, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, dst[:e_in], m)
        agg += torch.zeros(num_dst, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, run_dst, nbr_sum)
        return self.fc(agg)


class SAGE(nn.Module):
    def __init__(self, in_feats, n_hidden, n_classes, n_layers, dropout, conv=SageMean, first=None):
        super().__init__()
        dims = [in_feats] + [n_hidden] * (n_layers - 1) + [n_classes]
        self.layers = nn.ModuleList((first if first is not None and i == 0 else conv)(dims[i], dims[i + 1]) for i in range(n_layers))
        self.dropout = nn.Dropout(dropout)

    def forward(self, blocks, x):
        h = x
        for l, (layer, block) in enumerate(zip(self.layers, blocks)):
            h = layer(block, h)
            if l != len(self.layers) - 1:
                h = self.dropout(Func.relu(h))
        return h


def getter(ipc_service, aggregated, norm, edge_weight=False):
    """the ipc_service call for the server's hand-off mode: rows, neighbour sums, or the sums normalised by out-degree or scaled by edge weight"""
    if aggregated and edge_weight:
        return ipc_service.get_next_aggregated_edge_weight
    return ipc_service.get_next_aggregated_norm if aggregated and norm else ipc_service.get_next_aggregated if aggregated else ipc_service.get_next


def next_batch(ipc_service, feat_len, hops, aggregated=False, norm=0, edge_weight=False):
    """edge_weight: every block carries its edges' served weights (ipc_service.get_edge_weights(): block k's is a view of the same length
    as its src / dst); behind an aggregating server block 1 takes the served edge-weighted sums for the last hop."""
    out = getter(ipc_service, aggregated, norm, edge_weight)(feat_len)   # zero-copy views of server-owned device memory
    sizes = ipc_service.get_block_size()
    features, labels = out[1], out[2]
    blocks = [(out[3 + 2 * k].long(), out[4 + 2 * k].long(), sizes[2 * k], sizes[2 * k + 1]) for k in range(hops)]
    edges = [len(b[0]) for b in blocks]
    if aggregated:                                  # features = x_in[n_in, F]; out[-1] = the last hop's neighbour sums per input slot
        blocks[0] = fused_first_block(*blocks[0], edges, out[3 + 2 * hops])
    if edge_weight:
        blocks = [b + (w,) for b, w in zip(blocks, ipc_service.get_edge_weights())]
    return features, labels.long(), blocks


def worker(rank, world, args):
    import ipc_service
    torch.cuda.set_device(rank)
    device = torch.device("cuda", rank)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "12355")
        dist.init_process_group("nccl", rank=rank, world_size=world)   # RCCL on ROCm
    ipc_service.initialize()
    train_steps, valid_steps, test_steps = ipc_service.get_steps()
    hops = ipc_service.get_hops() if hasattr(ipc_service, "get_hops") else 2
    if rank == 0:   # how the server's sampler draws (LEGION_SAMPLING): "replace" like the reference, or "distinct" neighbours per row
        seed = ipc_service.sampling_seed() if hasattr(ipc_service, "sampling_seed") else None
        print("Server sampling mode: %s, %s" % (ipc_service.sampling() if hasattr(ipc_service, "sampling") else "replace",
                                                "the same batches every epoch (no LEGION_SAMPLING_SEED)" if seed is None else "seed %d: fresh draws per batch, reshuffled per epoch" % seed), flush=True)
    served_agg = bool(ipc_service.aggregated()) if hasattr(ipc_service, "aggregated") else False
    if served_agg != bool(args.aggregated):
        raise SystemExit("--aggregated must match the server: it %s the last hop (LEGION_AGG_LAST_HOP)" % ("aggregates" if served_agg else "does not aggregate"))
    served_norm = int(ipc_service.aggregate_norm()) if hasattr(ipc_service, "aggregate_norm") else 0
    if served_agg and not args.edge_weight and (served_norm != 0) != (args.model == "gcn"):      # the sums must be the ones the first layer adds up
        raise SystemExit("--model %s --aggregated needs a server that %s the neighbour sums (LEGION_AGG_NORM%s): GraphConvBoth adds rows scaled by "
                         "out-degree^-1/2, SageMean the rows themselves" % (args.model, "normalises" if args.model == "gcn" else "does not normalise",
                                                                          "=both" if args.model == "gcn" else " unset"))
    fused = (GraphConvBothFused if args.model == "gcn" else SageMeanFused) if served_agg else None
    conv = GraphConvBoth if args.model == "gcn" else SageMean
    served_ew = bool(ipc_service.aggregate_edge_weight()) if hasattr(ipc_service, "aggregate_edge_weight") else False
    if args.edge_weight:                 # sum_e w_e h[src_e] per dst: the weights of blocks 2..H are the served edge_w, block 1 takes the served sums
        if not (hasattr(ipc_service, "edge_weights") and ipc_service.edge_weights()):
            raise SystemExit("--edge_weight needs a server that serves edge weights (LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1)")
        if served_agg and not served_ew:
            raise SystemExit("--edge_weight --aggregated needs a server whose neighbour sums are scaled by edge weight (LEGION_AGG_EDGE_WEIGHT=1)")
        conv, fused = GraphConvEdgeWeight, GraphConvEdgeWeightFused if served_agg else None
    elif served_ew:
        raise SystemExit("the server scales its neighbour sums by edge weight (LEGION_AGG_EDGE_WEIGHT=1): run with --edge_weight --aggregated")
    model = SAGE(args.features_num, args.hidden_dim, args.class_num, hops, args.drop_rate, conv=conv, first=fused).to(device)
    if world > 1:
        model = DDP(model, device_ids=[rank])
    opt = torch.optim.Adam(model.parameters(), lr=args.learning_rate)
    loss_fn = nn.CrossEntropyLoss()

    def evaluate(steps):
        hit = tot = 0
        model.eval()
        with torch.no_grad():
            for _ in range(steps):
                x, y, blocks = next_batch(ipc_service, args.features_num, hops, served_agg, served_norm, args.edge_weight)
                ok = y >= 0                                  # -1 padded seeds of a short batch
                pred = model(blocks, x).argmax(1)
                hit += int((pred[ok] == y[ok]).sum())
                tot += int(ok.sum())
                torch.cuda.synchronize()
                ipc_service.synchronize()
        if world > 1:
            t = torch.tensor([hit, tot], device=device)
            dist.all_reduce(t)
            hit, tot = int(t[0]), int(t[1])
        return hit / max(tot, 1)

    def drain(steps):
        for _ in range(steps):
            getter(ipc_service, served_agg, served_norm, args.edge_weight)(args.features_num)
            ipc_service.synchronize()
        return float("nan")

    def lp_loss(h):                                          # lp_sage.py:87-90
        out, pos_out, neg_out = h.split(h.size(0) // 3, dim=0)
        return -Func.logsigmoid((out * pos_out).sum(-1)).mean() - Func.logsigmoid(-(out * neg_out).sum(-1)).mean()

    if args.task == "lp":
        evaluate = drain
    for epoch in range(args.epoch):
        model.train()
        t0, last = time.time(), float("nan")
        for _ in range(train_steps):
            x, y, blocks = next_batch(ipc_service, args.features_num, hops, served_agg, served_norm, args.edge_weight)
            loss = lp_loss(model(blocks, x)) if args.task == "lp" else loss_fn(model(blocks, x), y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            ipc_service.synchronize()                        # the server may refill this pipe now
            last = float(loss)
        cost = time.time() - t0
        acc = evaluate(valid_steps)
        if rank == 0:
            print("Epoch:{}, Cost:{:.3f} s, Train Loss:{:.4f}, Val Acc: {:.4f}".format(epoch, cost, last, acc), flush=True)
    acc = evaluate(test_steps)
    if rank == 0:
        print("Accuracy on test data: {:.4f}".format(acc), flush=True)
    ipc_service.finalize()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    ap = argparse.ArgumentParser("Train GraphSAGE on batches of the Legion server (plain PyTorch).")
    ap.add_argument("--model", default="sage", choices=["sage", "gcn"], help="legion_graphsage.py | legion_gcn.py layer")
    ap.add_argument("--task", default="nc", choices=["nc", "lp"], help="node classification | link prediction (lp_sage.py)")
    ap.add_argument("--class_num", type=int, default=47, help="nc: classes; lp: embedding width")
    ap.add_argument("--features_num", type=int, default=100)
    ap.add_argument("--hidden_dim", type=int, default=256)
    ap.add_argument("--drop_rate", type=float, default=0.5)
    ap.add_argument("--learning_rate", type=float, default=0.003)
    ap.add_argument("--epoch", type=int, default=100, help="must equal the epoch count in the server's meta_config")
    ap.add_argument("--gpu_num", type=int, default=1)
    ap.add_argument("--seed", type=int, default=None, help="torch.manual_seed (weights, dropout)")
    ap.add_argument("--aggregated", action="store_true", help="the server runs with LEGION_AGG_LAST_HOP=1: first layer = SageMeanFused over get_next_aggregated; "
                                                              "with --model gcn the server also runs with LEGION_AGG_NORM=both: GraphConvBothFused over get_next_aggregated_norm")
    ap.add_argument("--edge_weight", action="store_true", help="the server runs with LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1: every layer is GraphConvEdgeWeight "
                                                               "(sum_e w_e h[src_e] per dst) over get_edge_weights(); with --aggregated the server also runs with "
                                                               "LEGION_AGG_EDGE_WEIGHT=1: first layer = GraphConvEdgeWeightFused over get_next_aggregated_edge_weight")
    a = ap.parse_args()
    if a.gpu_num == 1:
        worker(0, 1, a)
    else:
        mp.spawn(worker, args=(a.gpu_num, a), nprocs=a.gpu_num, join=True)
