"""Call time (device events around ONE get_feature_kernel_agg call, the levels < H gathered before it) of the plain neighbour sums and of
the normalised sums (GPUMemoryPool_SetAggNorm: three small passes + the weighted k_gather_sum), same batches, alternating; papers100M or
products {25,10,5}, 8000 seeds.  Copied into a checkout without the normalised mode (the parent commit's) it times the plain sums alone:
the comparison base.
Usage: python3 profiles/agg_norm_call_times.py <workload> <label>"""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import legion1_amd.capi as K, legion1_amd.synth as S
from legion1_amd import layout
import bench
workload, label = sys.argv[1], sys.argv[2]
L = K.lib(); L.SetGPUDevice(0)
has_norm = "GPUMemoryPool_SetAggNorm" in K._SIGS
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
pool = eng.pools[0]; st = L.d_stream_create(); e0, e1 = L.d_event_create(), L.d_event_create()
L.GPUMemoryPool_SetAggLastHop(pool, 1)
def one(it, norm):
    if has_norm: L.GPUMemoryPool_SetAggNorm(pool, int(norm))
    L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
    L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)
    L.get_feature_kernel(st, eng.cache, eng.noder, pool, 0, 1, 1)
    for h in range(H):
        L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
        if h < H - 1: L.get_feature_kernel(st, eng.cache, eng.noder, pool, 0, 2 * h + 3, 1)
    L.d_stream_sync(st)
    L.d_event_record(e0, st)
    L.get_feature_kernel_agg(st, eng.cache, eng.noder, pool, 0, 1)
    L.d_event_record(e1, st); L.d_stream_sync(st); K.check()
    return L.d_event_elapsed_ms(e0, e1) * 1e3
modes = (False, True) if has_norm else (False,)
for it in range(3):
    for m in modes: one(it, m)
t = {m: [] for m in modes}; shapes = []
for it in range(3, 15):
    for m in modes: t[m].append(one(it, m))
    nc = eng.out[0][0]["nc"].to_numpy(np.int32, layout.COUNTER_WORDS); ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
    shapes.append(dict(n=layout.batch_nodes(nc, H), n_in=layout.first_block_dst(nc, H), N=layout.hop_inputs(nc, ec, H), E=layout.batch_edges(ec, H), E_H=layout.hop_edges_end(ec, H) - layout.hop_edges_begin(ec, H)))
m = {k: int(np.mean([s[k] for s in shapes])) for k in shapes[0]}
stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
out = dict(label=label, workload=workload, F=spec.F, mean_shape=m, plain_sums_us=stat(t[False]))
if has_norm:
    out["normalised_sums_us"] = stat(t[True])
    out["paired_difference_us"] = stat([b - a for a, b in zip(t[False], t[True])])
print(json.dumps(out))
eng.close()
