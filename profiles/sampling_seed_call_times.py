"""Call times (device events) of the sampler hops and of the gather with seeded sampling off and on, alternating per batch on one engine:
per hop one GPU_Random_Sampling call (k_sample + k_mark + k_write), then get_feature_kernel_all; and GPUMemoryPool_BeginRound
(k_shuffle_seeds over the workload's training list) timed the same way, one call per round.  papers100M or products {25,10,5}, 8000 seeds.
The seeded batches read the shuffled list and draw other neighbours, so their edges and unique nodes are reported beside the times.
Under `rocprofv3 --kernel-trace --stats` k_shuffle_seeds and the k_sample instantiations separate by name; `seeded-only` / `off-only` as the
fourth argument runs one mode alone for such a trace.
Usage: python3 profiles/sampling_seed_call_times.py <workload> <label> [batches] [seeded-only|off-only] [replace|distinct]"""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import legion1_amd.capi as K, legion1_amd.synth as S
from legion1_amd import layout
import bench
workload, label = sys.argv[1], sys.argv[2]
batches = int(sys.argv[3]) if len(sys.argv) > 3 else 12
only = sys.argv[4] if len(sys.argv) > 4 else "both"
distinct = sys.argv[5:6] == ["distinct"]
L = K.lib(); L.SetGPUDevice(0)
fan = [25, 10, 5]; H = 3; B = 8000; SEED = 12345
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
pool = eng.pools[0]; st = L.d_stream_create(); ev = [L.d_event_create() for _ in range(H + 2)]
L.GPUMemoryPool_SetSampleDistinct(pool, int(distinct))
def begin_round(rnd):
    L.GPUMemoryPool_SetSampleSeed(pool, 1, SEED)
    L.d_event_record(ev[0], st)
    L.GPUMemoryPool_BeginRound(st, pool, eng.noder, 0, rnd)
    L.d_event_record(ev[1], st); L.d_stream_sync(st); K.check()
    return L.d_event_elapsed_ms(ev[0], ev[1]) * 1e3
def one(it, seeded):
    L.GPUMemoryPool_SetSampleSeed(pool, int(seeded), SEED)       # the round's shuffled copy stays valid: same seed
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
    return [L.d_event_elapsed_ms(ev[h], ev[h + 1]) * 1e3 for h in range(H + 1)], layout.batch_edges(ec, H), layout.batch_nodes(nc, H)
modes = {"both": (False, True), "seeded-only": (True,), "off-only": (False,)}[only]
shuffle_us = [begin_round(r) for r in range(6)] if True in modes else []
begin_round(0) if True in modes else None
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
    d["gather_us"] = stat(a[:, H]); d["edges"] = int(np.mean(edges[m])); d["nodes"] = int(np.mean(nodes[m]))
    return d
out = dict(label=label, workload=workload, sample="distinct" if distinct else "replace", F=spec.F, batches=batches, n_train=spec.n_train)
if False in modes: out["off"] = summary(False)
if True in modes: out["seeded"] = summary(True); out["begin_round_us"] = [round(x, 2) for x in shuffle_us]
print(json.dumps(out))
eng.close()
