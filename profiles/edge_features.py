"""What get_edge_feature_kernel (k_gather_edges, GPUMemoryPool_SetEdgeFeatures) takes per hop, beside k_gather on the same box: products or
papers100M {25,10,5}, 8000 seeds, the reference's draws, CSR, node features and the edge table resident in HBM, through the launchers of this
process -- not bench.py.

  python3 profiles/edge_features.py <workload> <label> [--dims 4,16,64] [--batches 16] [--warmup 3]
      phase 1: the node gather of every batch (get_feature_kernel_all, HIP events) and a streaming float4 copy, for the fraction of peak;
      phase 2, per row width: the table is generated on the device (legion_synth_edge_features), every batch runs its hops and, behind each,
      get_edge_feature_kernel between two HIP events.  Per hop: median [min, max] us, edges, algorithmic bytes (8 + 8 dim per edge: the id, the
      row in, the row out) over the event time.  A width whose table and its copy do not fit the device is skipped and says so.  One JSON line.
The library is the one $LEGION_LIB names (a variant build), else the shipped one."""
import argparse, json, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(a):
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
    seeds = dict(train=[((tr.data_ptr(), spec.n_train), (lab.data_ptr(), spec.n_train))])
    steps = spec.n_train // B
    st = L.d_stream_create(); ev = [L.d_event_create() for _ in range(2 * H + 2)]
    stat = lambda v: dict(median=round(float(np.median(v)), 2), min=round(float(min(v)), 2), max=round(float(max(v)), 2))
    out = dict(label=a.label, workload=a.workload, V=int(spec.V), E=int(E), F=int(spec.F), B=B, fanout=fan, batches=a.batches, warmup=a.warmup,
               lib=os.environ.get("LEGION_LIB", "shipped"), cus=int(L.legion_sampler_cu_count()))

    def sample(eng, it):
        pool = eng.pools[0]
        L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
        L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)

    # ---- phase 1: k_gather and the copy, on the engine that holds the node features ----
    eng = K.Engine(indptr.data_ptr(), indices.data_ptr(), feats.data_ptr(), spec.V, spec.F, seeds, B, fan, E=E, features_pitch=pitch)
    eng.alloc_features()
    rows = []
    for it in range(a.warmup + a.batches):
        sample(eng, it % steps)
        for h in range(H):
            L.GPU_Random_Sampling(st, eng.graph, eng.cache, eng.pools[0], fan[h], 2 * h + 2, 0)
        L.d_event_record(ev[0], st)
        L.get_feature_kernel_all(st, eng.cache, eng.noder, eng.pools[0], 0, 1)
        L.d_event_record(ev[1], st); L.d_stream_sync(st); K.check()
        nc = eng.out[0][0]["nc"].to_numpy(np.int32, layout.COUNTER_WORDS)
        if it >= a.warmup:
            rows.append((L.d_event_elapsed_ms(ev[0], ev[1]) * 1e3, layout.batch_nodes(nc, H)))
    r = np.array(rows)
    gbps = float(np.median(r[:, 1] * (8 * spec.F + 8) / (r[:, 0] * 1e-6) / 1e9))
    out["k_gather"] = dict(us=stat(r[:, 0]), rows=int(r[:, 1].mean()), bytes_per_row=8 * spec.F + 8, GBps=round(gbps, 1))
    eng.close()
    del feats
    torch.cuda.empty_cache()
    out["copy_GBps"] = bench.measure_copy(types.SimpleNamespace(L=L, dev=dev))
    out["k_gather"]["frac_of_copy"] = round(gbps / out["copy_GBps"], 3)
    out["k_gather"]["frac_of_8TBps"] = round(gbps / 8000.0, 3)

    # ---- phase 2: the edge gather per row width, on an engine without node features (the table needs the room) ----
    tiny = torch.zeros(spec.V, dtype=torch.float32, device=dev)
    eng = K.Engine(indptr.data_ptr(), indices.data_ptr(), tiny.data_ptr(), spec.V, 1, seeds, B, fan, E=E)
    pool = eng.pools[0]
    L.GPUMemoryPool_SetEdgeIds(pool, 1); K.check()
    out["dims"] = {}
    for dim in a.dims:
        free, _ = torch.cuda.mem_get_info(dev)
        need = 2 * E * dim * 4 + eng.num_ids * dim * 4
        if need > free * 0.95:
            out["dims"][str(dim)] = dict(skipped="the table and its copy take %.0f GB, %.0f GB are free" % (need / 1e9, free / 1e9))
            continue
        table = torch.empty(E * dim, dtype=torch.float32, device=dev)
        L.legion_synth_edge_features(None, table.data_ptr(), 0, E, dim)
        torch.cuda.synchronize()
        eng.set_edge_features(table.data_ptr(), dim)
        del table
        torch.cuda.empty_cache()
        L.GPUMemoryPool_SetEdgeFeatures(pool, dim); K.check()
        rows = []
        for it in range(a.warmup + a.batches):
            sample(eng, it % steps)
            for h in range(H):
                L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
                L.d_event_record(ev[2 * h], st)
                L.get_edge_feature_kernel(st, eng.graph, pool, 0, 2 * h + 2)
                L.d_event_record(ev[2 * h + 1], st)
            L.d_stream_sync(st); K.check()
            ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
            if it >= a.warmup:
                rows.append([L.d_event_elapsed_ms(ev[2 * h], ev[2 * h + 1]) * 1e3 for h in range(H)] +
                            [layout.edges_through(ec, h + 1) - layout.edges_through(ec, h) for h in range(H)])
        r = np.array(rows, dtype=np.float64)
        hops = []
        for h in range(H):
            us, edges = r[:, h], r[:, H + h]
            g = float(np.median(edges * (8 + 8 * dim) / (us * 1e-6) / 1e9))
            hops.append(dict(us=stat(us), edges=int(edges.mean()), bytes_per_edge=8 + 8 * dim, GBps=round(g, 1), frac_of_copy=round(g / out["copy_GBps"], 3),
                             ns_per_edge=round(float(np.median(us / edges)) * 1e3, 4)))
        out["dims"][str(dim)] = dict(table_GB=round(E * dim * 4 / 1e9, 2), hops=hops)
        L.GPUMemoryPool_SetEdgeFeatures(pool, 0)
        eng.set_edge_features(None)
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", choices=["products", "papers100M"])
    ap.add_argument("label")
    ap.add_argument("--dims", type=lambda s: [int(x) for x in s.split(",")], default=[4, 16, 64])
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    main(ap.parse_args())
