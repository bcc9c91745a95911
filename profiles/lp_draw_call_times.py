"""Call times (device events) of batch_generator_kernel -- one k_seed launch -- with drawn link-prediction thirds off and on, alternating in
blocks of eight batches on one engine (one BeginRound per block: the mode changed), at the `lp` leg's shape: papers100M (or products) {25,10,5}, B = 7998, the [src | pos | neg] list of
legion_synth_lp_seeds.  Off is the seeded mode with the list in file order (k_seed<false, false>), on is k_seed<false, true> on the
triple-shuffled list.  Also GPUMemoryPool_BeginRound under the mode (k_shuffle_triples over the whole list), one call per round, and the
hops and the gather behind either batch, whose edges and nodes are reported beside the times (the drawn batches are other batches).
Usage: python3 profiles/lp_draw_call_times.py <workload> <label> [batches]"""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import legion1_amd.capi as K, legion1_amd.synth as S
from legion1_amd import layout
import bench
workload, label = sys.argv[1], sys.argv[2]
batches = int(sys.argv[3]) if len(sys.argv) > 3 else 24
L = K.lib(); L.SetGPUDevice(0)
fan = [25, 10, 5]; H = 3; B = 7998; k = B // 3; SEED = 12345
spec = S.spec_for(workload); dev = torch.device("cuda", 0)
pitch = L.legion_row_pitch(spec.F) if spec.F % 32 else 0
indptr, indices, feats, E = bench.build_graph_on_gpu(K, spec, dev, pitch=pitch)
tr = torch.empty(spec.n_train, dtype=torch.int32, device=dev)
L.legion_synth_seed_ids(None, tr.data_ptr(), 0, spec.n_train, spec.V, spec.M2, spec.C2, 1, 0)
tno = torch.arange(spec.n_train, dtype=torch.int64, device=dev)
n = (spec.n_train + k - 1) // k * B
seeds = torch.empty(n, dtype=torch.int32, device=dev)
L.legion_synth_lp_seeds(None, seeds.data_ptr(), tr.data_ptr(), tno.data_ptr(), spec.n_train, B, indptr.data_ptr(), indices.data_ptr(), spec.V, 1)
lab = torch.zeros(n, dtype=torch.int32, device=dev)
torch.cuda.synchronize(); K.check()
eng = K.Engine(indptr.data_ptr(), indices.data_ptr(), feats.data_ptr(), spec.V, spec.F,
               dict(train=[((seeds.data_ptr(), n), (lab.data_ptr(), n))]), B, fan, E=E, features_pitch=pitch)
eng.alloc_features()
pool = eng.pools[0]; st = L.d_stream_create(); ev = [L.d_event_create() for _ in range(H + 3)]
L.GPUMemoryPool_SetSampleSeed(pool, 1, SEED)
def begin_round(rnd, on):
    L.GPUMemoryPool_SetLpDraw(pool, k if on else 0, eng.graph if on else None)
    L.d_event_record(ev[0], st)
    L.GPUMemoryPool_BeginRound(st, pool, eng.noder if on else None, 0, rnd)      # off: the list is served verbatim, nothing is launched
    L.d_event_record(ev[1], st); L.d_stream_sync(st); K.check()
    return L.d_event_elapsed_ms(ev[0], ev[1]) * 1e3
def one(it):
    L.GPUMemoryPool_SetCurrentPipe(pool, 0); L.GPUMemoryPool_SetCurrentMode(pool, 0); L.GPUMemoryPool_SetIter(pool, it)
    L.d_event_record(ev[0], st)
    L.batch_generator_kernel(st, eng.noder, eng.cache, pool, B, it, 0, 0, 0)
    for h in range(H):
        L.d_event_record(ev[1 + h], st)
        L.GPU_Random_Sampling(st, eng.graph, eng.cache, pool, fan[h], 2 * h + 2, 0)
    L.d_event_record(ev[1 + H], st)
    L.get_feature_kernel_all(st, eng.cache, eng.noder, pool, 0, 1)
    L.d_event_record(ev[2 + H], st); L.d_stream_sync(st); K.check()
    nc = eng.out[0][0]["nc"].to_numpy(np.int32, layout.COUNTER_WORDS); ec = eng.out[0][0]["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
    return [L.d_event_elapsed_ms(ev[h], ev[h + 1]) * 1e3 for h in range(H + 2)], layout.batch_edges(ec, H), layout.batch_nodes(nc, H)
shuffle_us = [begin_round(r, True) for r in range(6)]
BLOCK = 8
t = {m: [] for m in (False, True)}; edges = {m: [] for m in t}; nodes = {m: [] for m in t}
for m in (False, True):                                   # warm-up: both instantiations, untimed
    begin_round(0, m)
    for it in range(3): one(it)
for first in range(3, 3 + batches, BLOCK):
    for m in (False, True):
        begin_round(0, m)
        for it in range(first, min(first + BLOCK, 3 + batches)):
            us, e, nn = one(it)
            t[m].append(us); edges[m].append(e); nodes[m].append(nn)
stat = lambda v: dict(median=round(float(np.median(v)), 2), min=round(float(min(v)), 2), max=round(float(max(v)), 2))
def summary(m):
    a = np.array(t[m])
    d = {"batch_generator_us": stat(a[:, 0])}
    d.update({"hop%d_us" % (h + 1): stat(a[:, 1 + h]) for h in range(H)})
    d["gather_us"] = stat(a[:, 1 + H]); d["edges"] = int(np.mean(edges[m])); d["nodes"] = int(np.mean(nodes[m]))
    return d
print(json.dumps(dict(label=label, workload=workload, F=spec.F, B=B, k=k, batches=batches, list_len=n, off=summary(False), lp_draw=summary(True),
                      begin_round_us=[round(x, 2) for x in shuffle_us])))
eng.close()
