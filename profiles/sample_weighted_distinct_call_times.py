"""Call times (device events) of the sampler hops in four sampling states -- replace, distinct, weighted, weighted without replacement
(GPUMemoryPool_SetWeightedDistinct) --, same seeds, alternating inside one process: per hop one GPU_Random_Sampling call (k_sample +
k_mark + k_write); per batch the edges and the unique nodes.  papers100M or products {25,10,5}, 8000 seeds, the synth: source's edge
weights (legion_synth_edge_weights), retained on the device (GPUGraphStorage_RetainEdgeWeights).  Also the time of
GPUGraphStorage_SetEdgeWeights with the weights kept, and the two footprints.
Usage: python3 profiles/sample_weighted_distinct_call_times.py <workload> <label> [batches]"""
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
w = torch.empty(E, dtype=torch.float32, device=dev)
L.legion_synth_edge_weights(None, w.data_ptr(), 0, E)
torch.cuda.synchronize()
assert L.GPUGraphStorage_RetainEdgeWeights(eng.graph, 1) == 0
t0 = time.perf_counter()
rc = L.GPUGraphStorage_SetEdgeWeights(eng.graph, w.data_ptr(), K.LOC_DEVICE)
build_s = round(time.perf_counter() - t0, 4)
K.check(); assert rc == 0 and L.GPUGraphStorage_HasRetainedEdgeWeights(eng.graph) == 1
del w
pool = eng.pools[0]; st = L.d_stream_create(); ev = [L.d_event_create() for _ in range(H + 1)]
STATES = dict(replace=(0, 0), distinct=(1, 0), weighted=(2, 0), weighted_distinct=(2, 1))
def one(it, state):
    kind, flag = STATES[state]
    L.GPUMemoryPool_SetSampling(pool, kind); L.GPUMemoryPool_SetWeightedDistinct(pool, flag)
    L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
    L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)
    L.d_stream_sync(st)
    for h in range(H):
        L.d_event_record(ev[h], st)
        L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
    L.d_event_record(ev[H], st); L.d_stream_sync(st); K.check()
    nc = eng.out[0][0]["nc"].to_numpy(np.int32, layout.COUNTER_WORDS); ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
    return [L.d_event_elapsed_ms(ev[h], ev[h + 1]) * 1e3 for h in range(H)], layout.batch_edges(ec, H), layout.batch_nodes(nc, H)
for it in range(3):
    for m in STATES: one(it, m)
t = {m: [] for m in STATES}; edges = {m: [] for m in STATES}; nodes = {m: [] for m in STATES}
for it in range(3, 3 + batches):
    for m in STATES:
        us, e, n = one(it, m)
        t[m].append(us); edges[m].append(e); nodes[m].append(n)
stat = lambda v: dict(median=round(float(np.median(v)), 2), min=round(float(min(v)), 2), max=round(float(max(v)), 2))
def summary(m):
    a = np.array(t[m])
    d = {"hop%d_us" % (h + 1): stat(a[:, h]) for h in range(H)}
    d["edges"] = int(np.mean(edges[m])); d["nodes"] = int(np.mean(nodes[m]))
    return d
out = dict(label=label, workload=workload, E=int(E), batches=batches, set_edge_weights_retained_s=build_s, alias_table_bytes=8 * int(E),
           retained_weight_bytes=4 * int(E))
for m in STATES:
    out[m] = summary(m)
print(json.dumps(out))
eng.close()
