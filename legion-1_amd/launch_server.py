#!/usr/bin/env python3
"""Launcher of the sampling server with the reference launcher's command line (legion_server.py:72-85):

    python launch_server.py --dataset_path /data --dataset PA --gpu_number 8 --cache_memory 38000000000 --epoch 10

It writes the same one-line ``meta_config`` (legion_server.py:58-59:
``path batch V E F n_train n_valid n_test cache_bytes epochs partition_flag``) into the working directory and
starts ``csrc/legion <gpu_number> <cache_agg_mode> <fanouts>`` (the reference: ``./src/legion G mode``,
legion_server.py:69).  Unlike the reference, ``--nbrs_num`` is honoured (the reference hard-codes 25,10 in
Server.cu:68-69 and never forwards the flag).
"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

# dataset facts the reference launcher carries (legion_server.py:6-53): directory, V, E, F, train/valid/test sizes
DATASETS = {
    "PR": ("products", 2449029, 123718280, 100, 196615, 39323, 2213091),
    "PA": ("paper100M", 111059956, 1615685872, 128, 11105995, 100000, 100000),
    "CO": ("com-friendster", 65608366, 1806067135, 256, 6560836, 100000, 100000),
    "UKS": ("ukunion", 133633040, 5507679822, 256, 13363304, 100000, 100000),
    "UKL": ("uk2014", 787801471, 47284178505, 128, 78780147, 100000, 100000),
    "CL": ("clueweb", 955207488, 42574107469, 128, 95520748, 100000, 100000),
}


def cache_agg_mode(gpu_number: int, usenvlink: int) -> int:
    """legion_server.py:61-68: pairs of GPUs form a clique when the fast interconnect is used."""
    return 1 if (usenvlink == 1 and gpu_number >= 2) else 0


def meta_line(args) -> str:
    name, V, E, F, n_train, n_valid, n_test = DATASETS[args.dataset]
    path = args.dataset_path + "/" + name + "/"
    return "{} {} {} {} {} {} {} {} {} {} {}".format(path, args.train_batch_size, V, E, F, n_train, n_valid, n_test,
                                                    args.cache_memory, args.epoch, 2 if args.seed_lists else 1 - args.usenvlink)


def main(argv=None):
    ap = argparse.ArgumentParser("Legion server (MI355X build).")
    ap.add_argument("--dataset_path", type=str, default="/home/atc-artifacts-user/datasets")
    ap.add_argument("--dataset", type=str, default="PA", choices=sorted(DATASETS))
    ap.add_argument("--train_batch_size", type=int, default=8000)
    ap.add_argument("--hops_num", type=int, default=2)
    ap.add_argument("--nbrs_num", type=str, default="25,10", help="fan-out per hop, e.g. 25,10,5")
    ap.add_argument("--gpu_number", type=int, default=1)
    ap.add_argument("--epoch", type=int, default=10)
    ap.add_argument("--cache_memory", type=int, default=38000000000)
    ap.add_argument("--usenvlink", type=int, default=1, help="1: cliques over the GPU interconnect (xGMI)")
    ap.add_argument("--seed_lists", action="store_true", help="extension (link prediction on several GPUs): every GPU g serves its own "
                    "pre-partitioned list trainingset_<G>_<g> verbatim (meta_config flag 2) instead of a split of `trainingset`")
    ap.add_argument("--sampling", type=str, default=None, choices=["replace", "distinct", "weighted"], help="extension: how a row draws its neighbours "
                    "(LEGION_SAMPLING for the server): replace = with replacement like the reference (the default), distinct = "
                    "min(degree, fan-out) distinct neighbours per row, weighted = with replacement in proportion to the dataset's edge_weights file")
    ap.add_argument("--sampling_seed", type=int, default=None, help="extension: a 32-bit seed (LEGION_SAMPLING_SEED for the server): every batch "
                    "draws afresh and the training list is reshuffled every epoch; without it every epoch is the same epoch, like the reference's")
    ap.add_argument("--lp_draw", action="store_true", help="extension (LEGION_LP_DRAW=1 for the server; needs --seed_lists and --sampling_seed): "
                    "the [src | pos | neg] triples are reshuffled every epoch and every batch draws its pos and neg thirds afresh")
    ap.add_argument("--weighted-distinct", "--weighted_distinct", dest="weighted_distinct", action="store_true", help="extension "
                    "(LEGION_WEIGHTED_DISTINCT=1 for the server; needs --sampling weighted): the weighted draws are without replacement, "
                    "min(neighbours of weight > 0, fan-out) distinct neighbours per row; the server keeps the weights in HBM beside the alias table")
    ap.add_argument("--shared-draws", "--shared_draws", dest="shared_draws", action="store_true", help="extension "
                    "(LEGION_SHARED_DRAWS=1 for the server; needs --sampling distinct and --sampling_seed): the distinct draws are keyed by the "
                    "neighbour node, so rows that see the same neighbours pick the same ones and a batch reaches fewer unique nodes; also on top of "
                    "--sampling weighted --weighted-distinct: the weighted draws without replacement take one uniform per neighbour node")
    ap.add_argument("--edge-ids", "--edge_ids", dest="edge_ids", action="store_true", help="extension (LEGION_EDGE_IDS=1 for the server): every "
                    "sampled edge's position in the dataset's edge_dst is served beside the blocks (ipc_service.get_edge_ids(); DGL's edata[dgl.EID], "
                    "PyG's e_id); not under --sampling weighted without --weighted-distinct")
    ap.add_argument("--edge-weights", "--edge_weights", dest="edge_weights", action="store_true", help="extension (LEGION_EDGE_WEIGHTS=1 for the "
                    "server; needs --edge-ids): the server keeps the dataset's edge_weights in HBM under every sampling kind and serves every "
                    "sampled edge's weight (ipc_service.get_edge_weights())")
    ap.add_argument("--agg-edge-weight", "--agg_edge_weight", dest="agg_edge_weight", action="store_true", help="extension "
                    "(LEGION_AGG_EDGE_WEIGHT=1 for the server; needs LEGION_AGG_LAST_HOP=1, --edge-ids and --edge-weights): the last hop's "
                    "neighbour sums scale every row by its edge's weight (ipc_service.get_next_aggregated_edge_weight())")
    ap.add_argument("--dry_run", action="store_true", help="write meta_config and print the command only")
    args = ap.parse_args(argv)
    fan = [int(x) for x in args.nbrs_num.replace("[", "").replace("]", "").split(",") if x.strip()]
    with open("meta_config", "w") as f:
        f.write(meta_line(args))
    cmd = [os.path.join(HERE, "csrc", "legion"), str(args.gpu_number), str(cache_agg_mode(args.gpu_number, args.usenvlink)),
           ",".join(map(str, fan)), os.path.abspath("meta_config")]
    if args.dry_run:
        print(" ".join(cmd))
        return 0
    env = dict(os.environ)
    if args.sampling is not None:
        env["LEGION_SAMPLING"] = args.sampling
    if args.sampling_seed is not None:
        env["LEGION_SAMPLING_SEED"] = str(args.sampling_seed)
    if args.lp_draw:
        env["LEGION_LP_DRAW"] = "1"
    if args.weighted_distinct:
        env["LEGION_WEIGHTED_DISTINCT"] = "1"
    if args.shared_draws:
        env["LEGION_SHARED_DRAWS"] = "1"
    if args.edge_ids:
        env["LEGION_EDGE_IDS"] = "1"
    if args.edge_weights:
        env["LEGION_EDGE_WEIGHTS"] = "1"
    if args.agg_edge_weight:
        env["LEGION_AGG_EDGE_WEIGHT"] = "1"
    return subprocess.call(cmd, env=env)


if __name__ == "__main__":
    sys.exit(main())
