"""What the edge-weighted last hop (GPUMemoryPool_SetAggEdgeWeight) costs, and its new kernel beside its yardstick: the same batches as plain
aggregated batches with edge ids, with the flag, and with normalised sums (GPUMemoryPool_SetAggNorm: k_draw_weights ranks the same slots
and takes one more dependent load), the three modes alternating batch by batch inside one process, through the launchers of this process
-- not bench.py.  products or papers100M {25,10,5}, 8000 seeds, the reference's draws, CSR, features and synthetic retained edge weights
resident in HBM.

  python3 profiles/edge_agg.py run <workload> <label> [--batches 24] [--warmup 3]
      device events around the whole batch (seed launch .. get_feature_kernel_agg) and around get_feature_kernel_agg alone: per mode the
      median [min, max] ms, as one JSON line.
  rocprofv3 --kernel-trace -d DIR -- python3 profiles/edge_agg.py run <workload> <label>
  python3 profiles/edge_agg.py table DIR
      the kernels of get_feature_kernel_agg in that run: median [min, max] us of both passes of k_draw_edge_weights, of k_agg_norm_prep,
      k_block_out_deg and k_draw_weights, and of k_gather_sum by instantiation."""
import argparse, collections, csv, glob, json, os, re, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("plain", "edge", "norm")


def table(trace_dir):
    f = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    per = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        m = re.search(r"legion::(k_draw_edge_weights<\w+>|k_agg_norm_prep|k_block_out_deg|k_draw_weights|k_gather_sum<[^>]*>)", r["Kernel_Name"])
        if m:
            per[m.group(1).replace(" ", "")].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    print("| kernel | launches counted | median us | min | max |\n|---|---|---|---|---|")
    for name in sorted(per):
        d = [t for _, t in sorted(per[name])][len(per[name]) // 4:]                     # the first quarter is warm-up
        print("| `%s` | %d | %.1f | %.1f | %.1f |" % (name, len(d), statistics.median(d), min(d), max(d)))


def run(a):
    import numpy as np, torch
    import legion1_amd.capi as K, legion1_amd.synth as S
    from legion1_amd import layout
    import bench
    L = K.lib(); L.SetGPUDevice(0)
    fan = [25, 10, 5]; H = 3; B = 8000
    spec = S.spec_for(a.workload); dev = torch.device("cuda", 0)
    pitch = L.legion_row_pitch(spec.F) if spec.F % 32 else 0
    indptr, indices, feats, E = bench.build_graph_on_gpu(K, spec, dev, pitch=pitch)
    tr = torch.empty(spec.n_train, dtype=torch.int32, device=dev)
    L.legion_synth_seed_ids(None, tr.data_ptr(), 0, spec.n_train, spec.V, spec.M2, spec.C2, 1, 0)
    lab = torch.zeros(spec.n_train, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng = K.Engine(indptr.data_ptr(), indices.data_ptr(), feats.data_ptr(), spec.V, spec.F,
                   dict(train=[((tr.data_ptr(), spec.n_train), (lab.data_ptr(), spec.n_train))]), B, fan, E=E, features_pitch=pitch,
                   retain_edge_weights=True)
    w = torch.empty(E, dtype=torch.float32, device=dev)
    L.legion_synth_edge_weights(None, w.data_ptr(), 0, E)
    torch.cuda.synchronize()
    L.GPUGraphStorage_SetEdgeWeights(eng.graph, w.data_ptr(), K.LOC_DEVICE)
    K.check()
    del w
    eng.alloc_features()
    pool = eng.pools[0]; st = L.d_stream_create(); ev = [L.d_event_create() for _ in range(3)]
    steps = spec.n_train // B
    L.GPUMemoryPool_SetAggLastHop(pool, 1)
    L.GPUMemoryPool_SetEdgeIds(pool, 1)
    K.check()

    def one(it, mode):
        L.GPUMemoryPool_SetAggEdgeWeight(pool, 0); L.GPUMemoryPool_SetAggNorm(pool, int(mode == "norm")); L.GPUMemoryPool_SetAggEdgeWeight(pool, int(mode == "edge"))
        L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
        L.d_event_record(ev[0], st)
        L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)
        L.get_feature_kernel(st, eng.cache, eng.noder, pool, 0, 1, 1)
        for h in range(H):
            L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
            if h < H - 1: L.get_feature_kernel(st, eng.cache, eng.noder, pool, 0, 2 * h + 3, 1)
        L.d_event_record(ev[1], st)
        L.get_feature_kernel_agg(st, eng.cache, eng.noder, pool, 0, 1)
        L.d_event_record(ev[2], st); L.d_stream_sync(st); K.check()
        return [L.d_event_elapsed_ms(ev[0], ev[2]), L.d_event_elapsed_ms(ev[1], ev[2])]

    for it in range(a.warmup):
        for m in MODES: one(it % steps, m)
    rows = {m: [] for m in MODES}
    for it in range(a.warmup, a.warmup + a.batches):
        k = it % len(MODES)
        for m in MODES[k:] + MODES[:k]:                      # the order inside a triple rotates too
            rows[m].append(one(it % steps, m))
    nc = eng.out[0][0]["nc"].to_numpy(np.int32, layout.COUNTER_WORDS); ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
    stat = lambda v: dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4))
    out = dict(label=a.label, workload=a.workload, V=int(spec.V), E=int(E), F=int(spec.F), B=B, fanout=fan, batches=a.batches, warmup=a.warmup,
               last_batch=dict(n_in=layout.first_block_dst(nc, H), runs=layout.hop_inputs(nc, ec, H), slots=layout.hop_inputs(nc, ec, H) * fan[-1],
                               last_hop_edges=layout.hop_edges_end(ec, H) - layout.hop_edges_begin(ec, H)))
    for m in MODES:
        r = np.array(rows[m], dtype=np.float64)
        out[m] = dict(batch_ms=stat(r[:, 0]), agg_call_ms=stat(r[:, 1]))
    out["edge_minus_plain_batch_ms"] = stat([e[0] - p[0] for p, e in zip(rows["plain"], rows["edge"])])
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("workload", choices=["products", "papers100M"])
    r.add_argument("label")
    r.add_argument("--batches", type=int, default=24)
    r.add_argument("--warmup", type=int, default=3)
    t = sub.add_parser("table")
    t.add_argument("trace_dir")
    a = ap.parse_args()
    table(a.trace_dir) if a.cmd == "table" else run(a)
