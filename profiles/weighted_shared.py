"""Call times (device events) under weighted sampling without replacement and under weighted shared-key sampling (GPUMemoryPool_SetSharedDraws
on top of it), same seeds, the states alternating batch by batch inside one process: per hop one GPU_Random_Sampling call (k_sample +
k_mark + k_write), then one gather of all levels (get_feature_kernel_all); per batch the edges and the unique nodes.  products or
papers100M {25,10,5}, 8000 seeds, CSR and features resident in HBM, the synth: source's edge weights retained on the device, pool seeded.
`--states weighted_distinct` runs on a tree that has no such rule yet (the baseline leg at the parent commit).
Usage: python3 profiles/weighted_shared.py <workload> <label> [--batches 24] [--warmup 3] [--states weighted_distinct,weighted_shared] [--seed 7]"""
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
ap.add_argument("--states", default="weighted_distinct,weighted_shared")
ap.add_argument("--seed", type=int, default=7, help="the pool's sampling seed: every batch draws under its own word, as a served epoch does")
a = ap.parse_args()
states = a.states.split(",")
assert a.batches >= 20 and set(states) <= {"weighted_distinct", "weighted_shared"}
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
w = torch.empty(E, dtype=torch.float32, device=dev)
L.legion_synth_edge_weights(None, w.data_ptr(), 0, E)
torch.cuda.synchronize()
assert L.GPUGraphStorage_RetainEdgeWeights(eng.graph, 1) == 0
rc = L.GPUGraphStorage_SetEdgeWeights(eng.graph, w.data_ptr(), K.LOC_DEVICE)
K.check(); assert rc == 0 and L.GPUGraphStorage_HasRetainedEdgeWeights(eng.graph) == 1
del w
pool = eng.pools[0]; st = L.d_stream_create(); ev = [L.d_event_create() for _ in range(H + 2)]
steps = spec.n_train // B                     # full batches of the list
L.GPUMemoryPool_SetSampling(pool, 2)
L.GPUMemoryPool_SetWeightedDistinct(pool, 1)
L.GPUMemoryPool_SetSampleSeed(pool, 1, a.seed)
L.GPUMemoryPool_BeginRound(st, pool, eng.noder, 0, 0)
L.d_stream_sync(st); K.check()
def one(it, state):
    if "weighted_shared" in states:
        L.GPUMemoryPool_SetSharedDraws(pool, int(state == "weighted_shared"))
    L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
    L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)
    L.d_stream_sync(st)
    for h in range(H):
        L.d_event_record(ev[h], st)
        L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
    L.d_event_record(ev[H], st)
    L.get_feature_kernel_all(st, eng.cache, eng.noder, pool, 0, 1)
    L.d_event_record(ev[H + 1], st); L.d_stream_sync(st); K.check()
    nc = eng.out[0][0]["nc"].to_numpy(np.int32, layout.COUNTER_WORDS); ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
    return [L.d_event_elapsed_ms(ev[h], ev[h + 1]) * 1e3 for h in range(H + 1)] + [layout.batch_nodes(nc, H), layout.batch_edges(ec, H)]
for it in range(a.warmup):
    for m in states: one(it % steps, m)
rows = {m: [] for m in states}
for it in range(a.warmup, a.warmup + a.batches):
    for m in states: rows[m].append(one(it % steps, m))
stat = lambda v: dict(median=round(float(np.median(v)), 1), min=round(float(min(v)), 1), max=round(float(max(v)), 1))
out = dict(label=a.label, workload=a.workload, V=int(spec.V), E=int(E), B=B, fanout=fan, batches=a.batches, warmup=a.warmup, seed=a.seed)
for m in states:
    r = np.array(rows[m], dtype=np.float64)
    out[m] = {"hop%d_us" % (h + 1): stat(r[:, h]) for h in range(H)}
    out[m].update(gather_us=stat(r[:, H]), nodes=int(r[:, H + 1].mean()), edges=int(r[:, H + 2].mean()))
print(json.dumps(out))
eng.close()
