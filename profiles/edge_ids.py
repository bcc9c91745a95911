"""What the edge-id mode (GPUMemoryPool_SetEdgeIds) costs: the same batches with the mode off and on, alternating batch by batch inside one
process, through the launchers of this process -- not bench.py.  products or papers100M {25,10,5}, 8000 seeds, the reference's draws, CSR
and features resident in HBM.

  python3 profiles/edge_ids.py run <workload> <label> [--batches 24] [--warmup 3] [--weights]
      device events around the seed launch, each hop's GPU_Random_Sampling (k_sample + k_mark + k_write, + k_edge_ids under the mode) and
      the gather of all levels: per mode the median [min, max] ms of each call and of the batch, as one JSON line.  --weights: the graph
      retains synthetic edge weights, so k_edge_ids<.., true> also stores edge_w.
  rocprofv3 --kernel-trace -d DIR -- python3 profiles/edge_ids.py run <workload> <label>
  python3 profiles/edge_ids.py table DIR
      the kernels of that run per mode and hop (a k_seed starts a batch, its k-th k_sample is hop k; a batch whose k_sample carries COLS
      ran with the mode on): median us of k_sample, k_mark, k_write and k_edge_ids."""
import argparse, collections, csv, glob, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(trace_dir):
    f = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    seq = []
    for r in csv.DictReader(open(f)):
        n = r["Kernel_Name"]
        if "legion::k_" not in n:
            continue
        short = n.split("legion::")[1].split("<")[0].split("(")[0]
        if short not in ("k_seed", "k_sample", "k_mark", "k_write", "k_edge_ids"):
            continue
        cols = short == "k_sample" and n.split("<")[1].split(">")[0].replace(" ", "").split(",")[6:7] == ["true"]
        seq.append((int(r["Start_Timestamp"]), short, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, cols))
    seq.sort()
    batches, cur = [], None
    for t, n, d, cols in seq:
        if n == "k_seed":
            cur = dict(on=False, hop=0, rows=[])
            batches.append(cur)
            continue
        if cur is None:
            continue
        if n == "k_sample":
            cur["hop"] += 1
            cur["on"] |= cols
        cur["rows"].append((n, cur["hop"], d))
    per = collections.defaultdict(list)
    for b in batches[len(batches) // 4:]:                 # the first quarter is warm-up
        for n, hop, d in b["rows"]:
            per[("on" if b["on"] else "off", n, hop)].append(d)
    print("| mode | kernel | hop 1 | hop 2 | hop 3 |\n|---|---|---|---|---|")
    for mode in ("off", "on"):
        for n in ("k_sample", "k_mark", "k_write", "k_edge_ids"):
            cells = ["%.1f" % statistics.median(per[(mode, n, h)]) if per.get((mode, n, h)) else "-" for h in (1, 2, 3)]
            if cells != ["-"] * 3:
                print("| %s | `%s` | %s |" % (mode, n, " | ".join(cells)))
    print("\nmedian us over %d batches per mode" % (len(batches) - len(batches) // 4 >> 1))


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
                   retain_edge_weights=a.weights)
    if a.weights:
        w = torch.empty(E, dtype=torch.float32, device=dev)
        L.legion_synth_edge_weights(None, w.data_ptr(), 0, E)
        torch.cuda.synchronize()
        L.GPUGraphStorage_SetEdgeWeights(eng.graph, w.data_ptr(), K.LOC_DEVICE)
        K.check()
        del w
    eng.alloc_features()
    pool = eng.pools[0]; st = L.d_stream_create(); ev = [L.d_event_create() for _ in range(H + 3)]
    steps = spec.n_train // B

    def one(it, on):
        L.GPUMemoryPool_SetEdgeIds(pool, int(on))
        L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
        L.d_event_record(ev[0], st)
        L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)
        L.d_event_record(ev[1], st)
        for h in range(H):
            L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
            L.d_event_record(ev[2 + h], st)
        L.get_feature_kernel_all(st, eng.cache, eng.noder, pool, 0, 1)
        L.d_event_record(ev[H + 2], st); L.d_stream_sync(st); K.check()
        ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
        t = [L.d_event_elapsed_ms(ev[i], ev[i + 1]) for i in range(H + 2)]
        return [L.d_event_elapsed_ms(ev[0], ev[H + 2])] + t + [layout.batch_edges(ec, H)]

    modes = (False, True)
    for it in range(a.warmup):
        for m in modes: one(it % steps, m)
    rows = {m: [] for m in modes}
    for it in range(a.warmup, a.warmup + a.batches):
        for m in (modes if it % 2 == 0 else modes[::-1]):       # the order inside a pair alternates too
            rows[m].append(one(it % steps, m))
    stat = lambda v: dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4))
    out = dict(label=a.label, workload=a.workload, V=int(spec.V), E=int(E), B=B, fanout=fan, batches=a.batches, warmup=a.warmup, weights=bool(a.weights))
    for m in modes:
        r = np.array(rows[m], dtype=np.float64)
        out["on" if m else "off"] = dict(batch_ms=stat(r[:, 0]), seed_ms=stat(r[:, 1]), hop_ms=[stat(r[:, 2 + h]) for h in range(H)],
                                         gather_ms=stat(r[:, H + 2]), edges=int(r[:, H + 3].mean()))
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
    r.add_argument("--weights", action="store_true")
    t = sub.add_parser("table")
    t.add_argument("trace_dir")
    a = ap.parse_args()
    table(a.trace_dir) if a.cmd == "table" else run(a)
