"""Call times (device events) of the sampler hops in the default and the weighted sampling kind, same seeds, alternating inside one
process: per hop one GPU_Random_Sampling call (k_sample + k_mark + k_write); per batch the edges and the unique nodes.  papers100M or
products {25,10,5}, 8000 seeds, the synth: source's edge weights (legion_synth_edge_weights).  Also the build time of the alias table
(GPUGraphStorage_SetEdgeWeights, weights already on the device: check, build and the scratch's allocation) and its footprint.
Copied into a checkout without the weighted mode (the parent commit's) it times the default mode alone: the comparison base; with a
fourth argument `replace-only` the change does the same.
Usage: python3 profiles/sample_weighted_call_times.py <workload> <label> [batches] [replace-only]"""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import legion1_amd.capi as K, legion1_amd.synth as S
from legion1_amd import layout
import bench
workload, label = sys.argv[1], sys.argv[2]
batches = int(sys.argv[3]) if len(sys.argv) > 3 else 12
L = K.lib(); L.SetGPUDevice(0)
has_weighted = "GPUMemoryPool_SetSampling" in K._SIGS and sys.argv[4:5] != ["replace-only"]
fan = [25, 10, 5]; H = 3; B = 8000
spec = S.spec_for(workload); dev = torch.device("cuda", 0)
pitch = L.legion_row_pitch(spec.F) if spec.F % 32 else 0
indptr, indices, feats, E = bench.build_graph_on_gpu(K, spec, dev, pitch=pitch)
tr = torch.empty(spec.n_train, dtype=torch.int32, device=dev)
L.legion_synth_seed_ids(None, tr.data_ptr(), 0, spec.n_train, spec.V, spec.M2, spec.C2, 1, 0)
lab = torch.zeros(spec.n_train, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
eng = K.Engine(indptr.data_ptr(), indices.data_ptr(), feats.data_ptr(), spec.V, spec.F,
               dict(train=[((tr.data_ptr(), spec.n_train), (lab.data_ptr(), spec.n_train))]), B, fan, E=E, features_pitch=pitch)
eng.alloc_features()
build_s = []
if has_weighted:
    w = torch.empty(E, dtype=torch.float32, device=dev)
    L.legion_synth_edge_weights(None, w.data_ptr(), 0, E)
    torch.cuda.synchronize()
    for _ in range(2):                                   # the second build replaces the first: the same work
        t0 = time.perf_counter()
        rc = L.GPUGraphStorage_SetEdgeWeights(eng.graph, w.data_ptr(), K.LOC_DEVICE)
        build_s.append(round(time.perf_counter() - t0, 4))
        K.check(); assert rc == 0
    del w
pool = eng.pools[0]; st = L.d_stream_create(); ev = [L.d_event_create() for _ in range(H + 1)]
def one(it, weighted):
    if has_weighted: L.GPUMemoryPool_SetSampling(pool, 2 if weighted else 0)
    L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
    L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)
    L.d_stream_sync(st)
    for h in range(H):
        L.d_event_record(ev[h], st)
        L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
    L.d_event_record(ev[H], st); L.d_stream_sync(st); K.check()
    nc = eng.out[0][0]["nc"].to_numpy(np.int32, layout.COUNTER_WORDS); ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
    return [L.d_event_elapsed_ms(ev[h], ev[h + 1]) * 1e3 for h in range(H)], layout.batch_edges(ec, H), layout.batch_nodes(nc, H)
modes = (False, True) if has_weighted else (False,)
for it in range(3):
    for m in modes: one(it, m)
t = {m: [] for m in modes}; edges = {m: [] for m in modes}; nodes = {m: [] for m in modes}
for it in range(3, 3 + batches):
    for m in modes:
        us, e, n = one(it, m)
        t[m].append(us); edges[m].append(e); nodes[m].append(n)
stat = lambda v: dict(median=round(float(np.median(v)), 2), min=round(float(min(v)), 2), max=round(float(max(v)), 2))
def summary(m):
    a = np.array(t[m])
    d = {"hop%d_us" % (h + 1): stat(a[:, h]) for h in range(H)}
    d["edges"] = int(np.mean(edges[m])); d["nodes"] = int(np.mean(nodes[m]))
    return d
out = dict(label=label, workload=workload, E=int(E), batches=batches, replace=summary(False))
if has_weighted:
    out["weighted"] = summary(True); out["alias_build_s"] = build_s; out["alias_table_bytes"] = 8 * int(E)
print(json.dumps(out))
eng.close()
