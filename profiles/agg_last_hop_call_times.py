"""Call time (device events around ONE launcher call) of the last level's gather in the default mode and of k_gather_sum in the aggregated
mode, same batches, alternating; papers100M or products {25,10,5}, 8000 seeds.  Usage: python3 profiles/agg_last_hop_call_times.py <workload> <label>   (LEGION_LIB selects a variant build)"""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import legion1_amd.capi as K, legion1_amd.synth as S
from legion1_amd import layout
import bench
workload, label = sys.argv[1], sys.argv[2]
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
pool = eng.pools[0]; st = L.d_stream_create(); e0, e1 = L.d_event_create(), L.d_event_create()
def one(it, agg):
    L.GPUMemoryPool_SetAggLastHop(pool, int(agg))
    L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
    L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)
    L.get_feature_kernel(st, eng.cache, eng.noder, pool, 0, 1, 1)
    for h in range(H):
        L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
        if h < H - 1: L.get_feature_kernel(st, eng.cache, eng.noder, pool, 0, 2 * h + 3, 1)
    L.d_stream_sync(st)
    L.d_event_record(e0, st)
    if agg: L.get_feature_kernel_agg(st, eng.cache, eng.noder, pool, 0, 1)
    else: L.get_feature_kernel(st, eng.cache, eng.noder, pool, 0, 2 * H + 1, 1)
    L.d_event_record(e1, st); L.d_stream_sync(st); K.check()
    return L.d_event_elapsed_ms(e0, e1) * 1e3
for it in range(3): one(it, False); one(it, True)
t = {False: [], True: []}; shapes = []
for it in range(3, 15):
    for agg in (False, True): t[agg].append(one(it, agg))
    nc = eng.out[0][0]["nc"].to_numpy(np.int32, layout.COUNTER_WORDS); ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
    shapes.append(dict(n=layout.batch_nodes(nc, H), n_in=layout.first_block_dst(nc, H), N=layout.hop_inputs(nc, ec, H), E_H=layout.hop_edges_end(ec, H) - layout.hop_edges_begin(ec, H)))
m = {k: int(np.mean([s[k] for s in shapes])) for k in shapes[0]}
F = spec.F
print(json.dumps(dict(label=label, workload=workload, F=F, mean_shape=m,
    last_level_gather_us=dict(median=float(np.median(t[False])), min=float(min(t[False])), max=float(max(t[False]))),
    gather_sum_us=dict(median=float(np.median(t[True])), min=float(min(t[True])), max=float(max(t[True]))),
    gather_bytes=8 * F * (m["n"] - m["n_in"]), gather_sum_bytes=4 * F * (m["E_H"] + m["N"]) + 4 * m["N"] * 5)))
eng.close()
