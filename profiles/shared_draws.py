"""Batch times (device events) under `distinct` and under shared-key sampling (GPUMemoryPool_SetSharedDraws on top of the distinct kind),
same seeds, the modes alternating batch by batch inside one process: the seed launch, one GPU_Random_Sampling per hop (k_sample + k_mark
+ k_write) and one gather of all levels (get_feature_kernel_all), through the launchers of this process -- not bench.py.  products or
papers100M {25,10,5}, 8000 seeds, CSR and features resident in HBM.  Per mode: ms per batch, sampler ms (seed launch + hops) and gather
ms as median [min, max] over the timed batches, and the nodes and edges of a batch.  `--modes distinct` runs on a tree that has no flag
yet (the baseline leg at the parent commit).
Usage: python3 profiles/shared_draws.py <workload> <label> [--batches 24] [--warmup 3] [--modes distinct,shared] [--seed 7]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import legion1_amd.capi as K, legion1_amd.synth as S
from legion1_amd import layout
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload", choices=["products", "papers100M"])
ap.add_argument("label")
ap.add_argument("--batches", type=int, default=24)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--modes", default="distinct,shared")
ap.add_argument("--seed", type=int, default=7, help="the pool's sampling seed: every batch draws under its own word, as a served epoch does")
a = ap.parse_args()
modes = a.modes.split(",")
assert a.batches >= 20 and set(modes) <= {"distinct", "shared"}
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
               dict(train=[((tr.data_ptr(), spec.n_train), (lab.data_ptr(), spec.n_train))]), B, fan, E=E, features_pitch=pitch)
eng.alloc_features()
pool = eng.pools[0]; st = L.d_stream_create(); ev = [L.d_event_create() for _ in range(3)]
steps = spec.n_train // B                     # full batches of the list
L.GPUMemoryPool_SetSampling(pool, 1)
L.GPUMemoryPool_SetSampleSeed(pool, 1, a.seed)
L.GPUMemoryPool_BeginRound(st, pool, eng.noder, 0, 0)
L.d_stream_sync(st); K.check()
def one(it, mode):
    if "shared" in modes:
        L.GPUMemoryPool_SetSharedDraws(pool, int(mode == "shared"))
    L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
    L.d_event_record(ev[0], st)
    L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)
    for h in range(H):
        L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
    L.d_event_record(ev[1], st)
    L.get_feature_kernel_all(st, eng.cache, eng.noder, pool, 0, 1)
    L.d_event_record(ev[2], st); L.d_stream_sync(st); K.check()
    nc = eng.out[0][0]["nc"].to_numpy(np.int32, layout.COUNTER_WORDS); ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
    s, g = L.d_event_elapsed_ms(ev[0], ev[1]), L.d_event_elapsed_ms(ev[1], ev[2])
    return s + g, s, g, layout.batch_nodes(nc, H), layout.batch_edges(ec, H)
for it in range(a.warmup):
    for m in modes: one(it % steps, m)
rows = {m: [] for m in modes}
for it in range(a.warmup, a.warmup + a.batches):
    for m in modes: rows[m].append(one(it % steps, m))
stat = lambda v: dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3), max=round(float(max(v)), 3))
out = dict(label=a.label, workload=a.workload, V=int(spec.V), E=int(E), B=B, fanout=fan, batches=a.batches, warmup=a.warmup, seed=a.seed)
for m in modes:
    r = np.array(rows[m], dtype=np.float64)
    out[m] = dict(batch_ms=stat(r[:, 0]), sampler_ms=stat(r[:, 1]), gather_ms=stat(r[:, 2]), nodes=int(r[:, 3].mean()), edges=int(r[:, 4].mean()))
print(json.dumps(out))
eng.close()
