#!/usr/bin/env python3
"""Throughput of the `legion` server process as a trainer sees it: a null consumer (wait -> read counters -> post), or with
--consumer aggregate a PyTorch consumer that computes the first layer's mean aggregate in both hand-off modes (rows / neighbour sums),
--consumer aggregate-gcn the same for GraphConv(norm='both')'s first-layer aggregate (rows / out-degree-normalised neighbour sums),
--consumer edges a PyTorch consumer that reads block 1's COO and, where the server serves them, its edge ids and weights,
drains every batch of the schedule through the C-ABI IPC client, for the two RunOnce variants of the runner:

    (default)                  enqueue batch i, then wait for batch i-1 and post it (sampler i || gathers i-1)
    LEGION_BATCH_GRAPH=1       the sampler side as a recorded hipGraph, the rows gathered by one plain launch on stream 1 behind it
(the reference's synchronous loop and the whole-batch graphs lost at every shape: profiles/r01_server_loop.md, r04_graph_trace.md)

    python examples/serve_bench.py [--workload products --scale 0.3 --batch 8000 --fanout 25,10 --epochs 3]
--edge-ids serves every variant three times -- as it is, with LEGION_EDGE_IDS=1, with LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1 -- for the cost
of the served edge buffers (profiles/served_edges.md), under the null consumer or --consumer edges.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def consume(epochs, hops):
    import legion1_amd.capi as K
    from legion1_amd import layout
    lib = K.lib()
    lib.legion_ipc_client_open.restype = C.c_void_p
    c = C.c_void_p(lib.legion_ipc_client_open(-1))
    steps = (C.c_int32 * 3)()
    lib.legion_ipc_client_steps(c, steps)
    total = (steps[0] + steps[1]) * epochs + steps[2]
    nc, ec = (C.c_int32 * layout.COUNTER_WORDS)(), (C.c_int32 * layout.COUNTER_WORDS)()
    edges = 0
    t0 = time.perf_counter()
    for _ in range(total):
        lib.legion_ipc_client_wait(c)
        lib.legion_ipc_client_read_counters(c, nc, ec)
        edges += layout.batch_edges(ec, hops)
        lib.legion_ipc_client_post(c)
    dt = time.perf_counter() - t0
    lib.legion_ipc_client_close(c)
    print(total, dt, edges)


def consume_aggregating(epochs, feat_dim):
    """A consumer that computes what the first GNN layer of a mean aggregator computes from a served batch -- the mean aggregate [n_in, F] --
    in whichever mode the server hands over: by index_select / index_add_ over every edge of block 1 (default), or from the rows of the
    hops < H plus the last hop's neighbour sums (LEGION_AGG_LAST_HOP=1).  Both modes are timed producing the same tensor."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "legion-1_amd", "ipc_service"))
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import ipc_service
    from legion_sage_torch import fused_first_block
    torch.cuda.set_device(0)
    ipc_service.initialize()
    steps = ipc_service.get_steps()
    hops, agg_mode = ipc_service.get_hops(), ipc_service.aggregated()
    total = (steps[0] + steps[1]) * epochs + steps[2]
    edges, check = 0, 0.0
    t0 = time.perf_counter()
    for _ in range(total):
        out = (ipc_service.get_next_aggregated if agg_mode else ipc_service.get_next)(feat_dim)
        sizes = ipc_service.get_block_size()
        x, src, dst, n_in = out[1], out[3].long(), out[4].long(), sizes[1]
        if agg_mode:
            _, _, _, _, e_in, run_dst, nbr_sum = fused_first_block(src, dst, sizes[0], n_in, [out[3 + 2 * k].numel() for k in range(hops)], out[3 + 2 * hops])
            agg = torch.zeros(n_in, feat_dim, device=x.device).index_add_(0, dst[:e_in], x.index_select(0, src[:e_in]))
            agg += torch.zeros(n_in, feat_dim, device=x.device).index_add_(0, run_dst.long(), nbr_sum)
        else:
            agg = torch.zeros(n_in, feat_dim, device=x.device).index_add_(0, dst, x.index_select(0, src))
        deg = torch.bincount(dst, minlength=n_in).clamp(min=1).unsqueeze(1)
        agg = agg / deg
        edges += int(src.numel())
        torch.cuda.synchronize()
        ipc_service.synchronize()
    dt = time.perf_counter() - t0
    check = float(agg.double().sum())            # the last batch's aggregate: the two modes agree to fp32 summation order
    ipc_service.finalize()
    print("last-batch aggregate sum %.6f (%s)" % (check, "aggregated" if agg_mode else "default"))
    print(total, dt, edges)


def consume_aggregating_gcn(epochs, feat_dim):
    """consume_aggregating for GraphConv(norm='both'): the first layer's aggregate [n_in, F] in front of its linear map,
    sum_{(s,d)} x_s / sqrt(outdeg_s) / sqrt(indeg_d), degrees counted inside block 1 -- from every row of the batch (default), or from the
    rows of the hops < H plus the last hop's normalised sums (LEGION_AGG_LAST_HOP=1 LEGION_AGG_NORM=both).  Both count the degrees from
    the COO; both are timed producing the same tensor."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "legion-1_amd", "ipc_service"))
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import ipc_service
    from legion_sage_torch import fused_first_block
    torch.cuda.set_device(0)
    ipc_service.initialize()
    steps = ipc_service.get_steps()
    hops, agg_mode = ipc_service.get_hops(), ipc_service.aggregated()
    if agg_mode and not ipc_service.aggregate_norm():
        raise SystemExit("--consumer aggregate-gcn: the server aggregates the last hop without LEGION_AGG_NORM=both")
    total = (steps[0] + steps[1]) * epochs + steps[2]
    edges = 0
    t0 = time.perf_counter()
    for _ in range(total):
        out = (ipc_service.get_next_aggregated_norm if agg_mode else ipc_service.get_next)(feat_dim)
        sizes = ipc_service.get_block_size()
        x, src, dst, n, n_in = out[1], out[3].long(), out[4].long(), sizes[0], sizes[1]
        out_w = torch.bincount(src, minlength=n).clamp(min=1).to(x.dtype).rsqrt().unsqueeze(1)
        in_w = torch.bincount(dst, minlength=n_in).clamp(min=1).to(x.dtype).rsqrt().unsqueeze(1)
        if agg_mode:
            _, _, _, _, e_in, run_dst, nbr_sum = fused_first_block(src, dst, n, n_in, [out[3 + 2 * k].numel() for k in range(hops)], out[3 + 2 * hops])
            agg = torch.zeros(n_in, feat_dim, device=x.device).index_add_(0, dst[:e_in], (x * out_w[:n_in]).index_select(0, src[:e_in]))
            agg += torch.zeros(n_in, feat_dim, device=x.device).index_add_(0, run_dst.long(), nbr_sum)
        else:
            agg = torch.zeros(n_in, feat_dim, device=x.device).index_add_(0, dst, (x * out_w).index_select(0, src))
        agg = agg * in_w
        edges += int(src.numel())
        torch.cuda.synchronize()
        ipc_service.synchronize()
    dt = time.perf_counter() - t0
    check = float(agg.double().sum())            # the last batch's aggregate: the two modes agree to fp32 summation order
    ipc_service.finalize()
    print("last-batch GraphConv aggregate sum %.6f (%s)" % (check, "normalised sums" if agg_mode else "default"))
    print(total, dt, edges)


def consume_edges(epochs, feat_dim):
    """A consumer that reads every edge of block 1 once: the sums of src and dst in every mode and, where the server serves them
    (LEGION_EDGE_IDS=1, LEGION_EDGE_WEIGHTS=1), of the edge ids and the edge weights -- one pass over each served buffer per batch."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "legion-1_amd", "ipc_service"))
    import ipc_service
    torch.cuda.set_device(0)
    ipc_service.initialize()
    steps = ipc_service.get_steps()
    ids_on, w_on = ipc_service.edge_ids(), ipc_service.edge_weights()
    total = (steps[0] + steps[1]) * epochs + steps[2]
    edges = 0
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    t0 = time.perf_counter()
    for _ in range(total):
        out = ipc_service.get_next(feat_dim)
        acc[0] += out[3].sum()
        acc[1] += out[4].sum()
        if ids_on:
            acc[2] += ipc_service.get_edge_ids()[0].sum()
        if w_on:
            acc[3] += ipc_service.get_edge_weights()[0].sum()
        edges += int(out[3].numel())
        torch.cuda.synchronize()
        ipc_service.synchronize()
    dt = time.perf_counter() - t0
    ipc_service.finalize()
    print("sums of src, dst, edge ids, edge weights: %s (edge ids %s, weights %s)" % (acc.tolist(), "served" if ids_on else "off", "served" if w_on else "off"))
    print(total, dt, edges)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--consume", type=int, default=0, help="internal: run the null consumer for this many epochs")
    ap.add_argument("--workload", default="products")
    ap.add_argument("--scale", type=float, default=0.3)
    ap.add_argument("--batch", type=int, default=8000)
    ap.add_argument("--fanout", default="25,10")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--variants", default="all", help="comma list of: pipelined,graph + gather")
    ap.add_argument("--consumer", default="null", choices=["null", "aggregate", "aggregate-gcn", "edges"],
                    help="null: wait -> read counters -> post.  aggregate: a PyTorch consumer that computes the first layer's mean aggregate [n_in, F] "
                         "of every batch; each variant is then served twice, default hand-off and LEGION_AGG_LAST_HOP=1.  aggregate-gcn: the same for "
                         "GraphConv(norm='both')'s aggregate, default hand-off and LEGION_AGG_LAST_HOP=1 LEGION_AGG_NORM=both")
    ap.add_argument("--edge-ids", action="store_true", help="serve every variant three times: as it is, with LEGION_EDGE_IDS=1, and with LEGION_EDGE_IDS=1 "
                    "LEGION_EDGE_WEIGHTS=1 (consumers null and edges; --source files gets an edge_weights file of the synth: source's weights)")
    ap.add_argument("--features", type=int, default=0, help="internal: feature width for --consume with --consumer aggregate")
    ap.add_argument("--full-eval", action="store_true", help="keep the full validation / test sets (512-seed batches)")
    ap.add_argument("--source", default="files", choices=["files", "synth"],
                    help="files: write the dataset in Legion's raw layout and let the server read it (GPUGraphStore.cu:254-325).  synth: the server generates "
                         "the same tables in its own HBM (meta_config dataset path `synth:<workload>:<scale>`) -- the only way to serve the papers100M / uk-union shapes")
    a = ap.parse_args()
    if a.consume:
        if a.consumer == "aggregate-gcn":
            return consume_aggregating_gcn(a.consume, a.features)
        if a.consumer == "edges":
            return consume_edges(a.consume, a.features)
        return consume_aggregating(a.consume, a.features) if a.consumer == "aggregate" else consume(a.consume, len(a.fanout.split(",")))
    import legion1_amd.synth as S
    if a.source == "synth":
        spec = S.spec_for(a.workload, scale=a.scale)
        n_eval = min(512, spec.n_valid, spec.n_test) if not a.full_eval else None
        tmp = tempfile.mkdtemp(prefix="legion_serve_")
        meta = os.path.join(tmp, "meta_config")
        with open(meta, "w") as f:
            f.write("synth:%s:%r %d %d 0 %d %d %d %d 0 %d 0" % (a.workload, a.scale, a.batch, spec.V, spec.F, spec.n_train,
                                                             n_eval or spec.n_valid, n_eval or spec.n_test, a.epochs))
        return serve_variants(a, tmp, meta, spec.F)
    ds = S.generate(S.spec_for(a.workload, scale=a.scale))
    if not a.full_eval:   # keep the schedule dominated by full training batches: one validation / test batch each
        import dataclasses
        ds.valid, ds.test = ds.valid[:512], ds.test[:512]
        ds.spec = dataclasses.replace(ds.spec, n_valid=len(ds.valid), n_test=len(ds.test))
    tmp = tempfile.mkdtemp(prefix="legion_serve_")
    data = os.path.join(tmp, "ds") + "/"
    S.write_legion_files(ds, data)
    if a.edge_ids:
        S.edge_weights(ds.E).astype("<f4").tofile(os.path.join(data, "edge_weights"))
    meta = os.path.join(tmp, "meta_config")
    with open(meta, "w") as f:
        f.write(S.meta_config_line(ds, data, a.batch, 1 << 40, a.epochs, 0))
    return serve_variants(a, tmp, meta, ds.spec.F)


def serve_variants(a, tmp, meta, F):
    server = os.path.join(ROOT, "legion-1_amd", "csrc", "legion")
    variants = [("pipelined", {}), ("graph + gather", {"LEGION_BATCH_GRAPH": "1"}), ("pipelined", {}), ("graph + gather", {"LEGION_BATCH_GRAPH": "1"})]
    if a.variants != "all":
        variants = [v for v in variants[:2] if v[0] in a.variants.split(",")]
    if a.consumer == "aggregate":    # every variant in both hand-off modes, alternating
        variants = [(n + m, dict(e, **x)) for n, e in variants for m, x in ((", rows", {}), (", neighbour sums", {"LEGION_AGG_LAST_HOP": "1"}))]
    if a.consumer == "aggregate-gcn":
        variants = [(n + m, dict(e, **x)) for n, e in variants for m, x in ((", rows", {}), (", normalised sums", {"LEGION_AGG_LAST_HOP": "1", "LEGION_AGG_NORM": "both"}))]
    if a.edge_ids:                   # every variant with the mode off, with the ids, with ids and weights, alternating
        variants = [(n + m, dict(e, **x)) for n, e in variants for m, x in ((", edge ids off", {}), (", edge ids", {"LEGION_EDGE_IDS": "1"}),
                                                                            (", edge ids + weights", {"LEGION_EDGE_IDS": "1", "LEGION_EDGE_WEIGHTS": "1"}))]
    for name, extra in variants:
        ns = "sb%d_%s%s%s%s%s_" % (os.getpid(), name[:3], extra.get("LEGION_BATCH_GRAPH", ""), extra.get("LEGION_AGG_LAST_HOP", ""), extra.get("LEGION_EDGE_IDS", ""), extra.get("LEGION_EDGE_WEIGHTS", ""))
        env = dict(os.environ, LEGION_IPC_NAMESPACE=ns, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
        log = open(os.path.join(tmp, "server_%s.log" % name[:3]), "w")
        proc = subprocess.Popen([server, "1", "0", a.fanout, meta], stdout=log, stderr=subprocess.STDOUT, env=env, cwd=tmp)
        while "System is ready for serving" not in open(log.name).read():
            if proc.poll() is not None:
                raise SystemExit("server died:\n" + open(log.name).read()[-2000:])
            time.sleep(0.2)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--consume", str(a.epochs), "--fanout", a.fanout, "--consumer", a.consumer, "--features", str(F)],
                             env=env, capture_output=True, text=True, timeout=600)   # one consumer process per server
        if out.returncode != 0:
            raise SystemExit(out.stdout[-2000:] + out.stderr[-2000:])
        total, dt, edges = out.stdout.strip().splitlines()[-1].split()
        total, dt, edges = int(total), float(dt), int(edges)
        proc.wait(timeout=60)
        if a.consumer != "null":
            print("    " + out.stdout.strip().splitlines()[-2], flush=True)
        print("%-32s %5d batches  %.3f ms/batch  %.2f G edges/s" % (name, total, dt / total * 1e3, edges / dt / 1e9), flush=True)


if __name__ == "__main__":
    main()
