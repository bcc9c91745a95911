"""What target-edge exclusion (GPUMemoryPool_SetLpExclude) costs: the same link-prediction batches with the mode off and on, alternating
batch by batch inside one process, through the launchers of this process -- not bench.py.  products or papers100M {25,10,5}, B = 7998
(k = 2666 triples, the pos and neg thirds drawn per batch under a seed), the reference's draws, CSR and features resident in HBM.

  python3 profiles/lp_exclude.py run <workload> <label> [--batches 24] [--warmup 3]
      device events around batch_generator_kernel (k_seed, + k_lp_pairs under the mode) and each hop's GPU_Random_Sampling (the last one
      + k_lp_edge_keep under the mode): per mode the median [min, max] ms of each call, the batch's edges and lp_excluded[0..H] of the
      last timed batch, as one JSON line."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(a):
    import numpy as np, torch
    import legion1_amd.capi as K, legion1_amd.synth as S
    from legion1_amd import layout
    import bench
    L = K.lib(); L.SetGPUDevice(0)
    fan = [25, 10, 5]; H = 3; k = 2666; B = 3 * k; seed = 12345
    spec = S.spec_for(a.workload); dev = torch.device("cuda", 0)
    pitch = L.legion_row_pitch(spec.F) if spec.F % 32 else 0
    indptr, indices, feats, E = bench.build_graph_on_gpu(K, spec, dev, pitch=pitch)
    n = spec.n_train // B * B                                       # whole batches of [src | pos | neg]; only the src thirds are read
    tr = torch.empty(n, dtype=torch.int32, device=dev)
    L.legion_synth_seed_ids(None, tr.data_ptr(), 0, n, spec.V, spec.M2, spec.C2, 1, 0)
    lab = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng = K.Engine(indptr.data_ptr(), indices.data_ptr(), feats.data_ptr(), spec.V, spec.F,
                   dict(train=[((tr.data_ptr(), n), (lab.data_ptr(), n))]), B, fan, E=E, features_pitch=pitch)
    pool = eng.pools[0]; st = L.d_stream_create(); ev = [L.d_event_create() for _ in range(H + 2)]
    steps = n // B
    eng._set_seed(0, seed, 0, st, k)                                # seeded, lp_draw = k, the round begun on the batches' stream

    def one(it, on):
        L.GPUMemoryPool_SetLpExclude(pool, k if on else 0)
        L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
        L.d_event_record(ev[0], st)
        L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)
        L.d_event_record(ev[1], st)
        for h in range(H):
            L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
            L.d_event_record(ev[2 + h], st)
        L.d_stream_sync(st); K.check()
        ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
        cnt = K.read_dev(L.GPUMemoryPool_GetLpExcludedBuffer(pool), np.int32, 8) if on else np.zeros(8, np.int32)
        return [L.d_event_elapsed_ms(ev[i], ev[i + 1]) for i in range(H + 1)] + [layout.batch_edges(ec, H)], cnt

    modes = (False, True)
    for it in range(a.warmup):
        for m in modes: one(it % steps, m)
    rows, cnts = {m: [] for m in modes}, {}
    for it in range(a.warmup, a.warmup + a.batches):
        for m in (modes if it % 2 == 0 else modes[::-1]):       # the order inside a pair alternates too
            r, cnts[m] = one(it % steps, m)
            rows[m].append(r)
    stat = lambda v: dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4))
    out = dict(label=a.label, workload=a.workload, V=int(spec.V), E=int(E), B=B, k=k, fanout=fan, batches=a.batches, warmup=a.warmup)
    for m in modes:
        r = np.array(rows[m], dtype=np.float64)
        out["on" if m else "off"] = dict(seed_ms=stat(r[:, 0]), hop_ms=[stat(r[:, 1 + h]) for h in range(H)], edges=int(r[:, H + 1].mean()),
                                         lp_excluded=cnts[m][:H + 1].tolist())
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
    run(ap.parse_args())
