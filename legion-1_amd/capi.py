"""ctypes binding of the C ABI (include/legion_amd.h -> csrc/liblegion_amd.so).

This is the host-side mirror used by tests and bench.py.  It contains no compute
and no fallback: if the HIP library is missing, importing :func:`lib` raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import layout

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB_PATH = os.path.join(_HERE, "csrc", "liblegion_amd.so")


def lib_path() -> str:
    """The library this process loads: csrc/liblegion_amd.so, or the ABSOLUTE path in $LEGION_LIB -- a variant build of an experiment
    (profiles/ab_kernels.sh) or the host-sanitizer build (make -C legion-1_amd/csrc asan-host).  Experiments point at their variant
    through this and never overwrite the shipped library (round 4 swapped it in place: a killed run left an invalid library behind)."""
    p = os.environ.get("LEGION_LIB")
    if not p:
        return DEFAULT_LIB_PATH
    if not os.path.isabs(p):
        raise RuntimeError(f"LEGION_LIB={p!r}: an absolute path is required (a relative one would depend on the working directory of every child process)")
    return p


LIB_PATH = DEFAULT_LIB_PATH      # kept for callers that print it; lib() resolves lib_path() when it loads
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "legion_amd.h")

TRAINMODE, VALIDMODE, TESTMODE = 0, 1, 2
LOC_HOST_PINNED, LOC_DEVICE, LOC_HOST_PAGEABLE = 0, 1, 2
ERR_EXIT, ERR_RETURN = 0, 1

_lib = None

vp, i32, i64, u32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_double


class LegionBuildInfo(C.Structure):
    _fields_ = [
        ("partition_count", i32),
        ("training_set_num", vp), ("training_set_ids", vp), ("training_labels", vp),
        ("validation_set_num", vp), ("validation_set_ids", vp), ("validation_labels", vp),
        ("testing_set_num", vp), ("testing_set_ids", vp), ("testing_labels", vp),
        ("total_num_nodes", i32), ("float_attr_len", i32),
        ("host_float_attrs", vp), ("features_location", i32),
        ("csr_node_index", vp), ("csr_dst_node_ids", vp), ("csr_location", i32),
        ("total_edge_num", i64), ("cache_edge_num", i64),
        ("epoch", i32), ("raw_batch_size", i32),
        ("float_attr_pitch", i32),
    ]


class LegionSynthSpec(C.Structure):
    _fields_ = [("V", i32), ("F", i32), ("classes", i32), ("n_train", i32), ("n_valid", i32), ("n_test", i32),
                ("M", u32), ("C", u32), ("M2", u32), ("C2", u32), ("ladder", i32 * 26), ("mean_degree", f64)]


class OpParams(C.Structure):
    _fields_ = [("device_id", C.c_int), ("stream", vp), ("event", vp), ("memorypool", vp), ("cache", vp),
                ("graph", vp), ("noder", vp), ("env", vp), ("neighbor_count", C.c_int), ("is_presc", C.c_int),
                ("in_memory", C.c_int)]


class RunnerParams(C.Structure):
    _fields_ = [("device_id", C.c_int), ("fanout", vp), ("hops", i32), ("cache", vp), ("graph", vp), ("noder", vp),
                ("env", vp), ("global_batch_id", C.c_int), ("in_memory", C.c_int)]


# (name, restype, argtypes) for everything that does not return void / take only ints+pointers
_SIGS = {
    "legion_version": (C.c_char_p, []),
    "legion_last_error": (C.c_char_p, []),
    "legion_set_error_mode": (None, [C.c_int]),
    "legion_set_device_map": (None, [i32, i32]),
    "legion_physical_device": (i32, [i32]),
    "legion_row_pitch": (i32, [i32]),
    "legion_shard_pitch": (i32, [i32, i64, i64]),
    "GPUCache_HitSamplingDone": (None, [vp, i32, vp]),
    "legion_set_remote_device": (None, [i32, C.c_int]),
    "legion_is_remote_device": (C.c_int, [i32]),
    "legion_audit_enabled": (C.c_int, []),
    "legion_audit_counts": (None, [vp]),
    "legion_audit_message_count": (i32, []),
    "legion_audit_message": (C.c_char_p, [i32]),
    "legion_audit_reset": (None, []),
    "legion_audit_report": (i64, []),
    "legion_audit_alias": (C.c_int, [i32, i32]),
    "d_alloc_space": (vp, [i64]),
    "d_free_space": (None, [vp]),
    "host_alloc_space64": (vp, [i64]),
    "host_free_space": (None, [vp]),
    "d_copy_h_2_d": (None, [vp, vp, i64]),
    "d_copy_d_2_h": (None, [vp, vp, i64]),
    "d_stream_sync": (None, [vp]),
    "d_stream_create": (vp, []),
    "d_stream_create_cu_mask": (vp, [vp, i32]),
    "d_stream_create_priority": (vp, [i32]),
    "d_stream_destroy": (None, [vp]),
    "d_copy_async": (None, [vp, vp, i64, vp]),
    "d_memset_async": (None, [vp, C.c_int, i64, vp]),
    "d_event_create": (vp, []),
    "d_event_destroy": (None, [vp]),
    "d_event_record": (None, [vp, vp]),
    "d_stream_wait_event": (None, [vp, vp]),
    "d_event_elapsed_ms": (C.c_float, [vp, vp]),
    "SetGPUDevice": (None, [i32]),
    "GetGPUDevice": (i32, []),
    "NewGPUMemoryGraphStorage": (vp, []),
    "GPUGraphStorage_Build": (None, [vp, vp]),
    "GPUGraphStorage_GraphCache": (None, [vp, vp, i32, i32, i32]),
    "GPUGraphStorage_ReplicateToDevices": (i64, [vp]),
    "GPUNodeStorage_ReplicateToDevices": (i64, [vp]),
    "GPUGraphStorage_Finalize": (None, [vp]),
    "GPUGraphStorage_Delete": (None, [vp]),
    "GPUGraphStorage_GetFragmentIndex": (vp, [vp, i32, i32]),
    "GPUGraphStorage_ExportFragment": (C.c_int, [vp, i32, vp, vp, vp]),
    "GPUGraphStorage_ImportFragment": (C.c_int, [vp, i32, i32, vp, vp, i32]),
    "GPUGraphStorage_GetFragmentMatrix": (vp, [vp, i32, i32]),
    "GPUMemoryPool_BeginBatchCapture": (C.c_int, [vp, vp]),
    "GPUMemoryPool_EndBatchCapture": (vp, [vp, vp]),
    "LegionBatchGraph_Launch": (C.c_int, [vp, vp, i32]),
    "LegionBatchGraph_Delete": (None, [vp]),
    "GPUGraphStorage_FragmentRows": (i32, [vp, i32]),
    "GPUGraphStorage_FragmentEdges": (C.c_int64, [vp, i32]),
    "GPUGraphStorage_FragmentChunkCount": (i32, [vp, i32, i32]),
    "GPUGraphStorage_FragmentChunkSpan": (C.c_int64, [vp, i32]),
    "GPUGraphStorage_GetFragmentChunk": (vp, [vp, i32, i32, i32]),
    "GPUGraphStorage_ExportFragmentChunk": (C.c_int, [vp, i32, i32, i32, vp]),
    "GPUGraphStorage_ImportFragmentChunk": (C.c_int, [vp, i32, i32, i32, i32, vp, i32, C.c_int64]),
    "NewGPUMemoryNodeStorage": (vp, []),
    "GPUNodeStorage_Build": (None, [vp, vp]),
    "GPUNodeStorage_Delete": (None, [vp]),
    "GPUNodeStorage_TrainingSetSize": (i32, [vp, i32]),
    "NewGPUMemoryPool": (vp, [i32]),
    "GPUMemoryPool_AllocateScratch": (None, [vp, i32, i32, vp, i32]),
    "GPUMemoryPool_NumIds": (i32, [vp]),
    "GPUMemoryPool_SetSampledIds": (None, [vp, vp, i32]),
    "GPUMemoryPool_SetFloatFeatures": (None, [vp, vp, i32]),
    "GPUMemoryPool_SetLabels": (None, [vp, vp, i32]),
    "GPUMemoryPool_SetAggSrcOf": (None, [vp, vp, i32]),
    "GPUMemoryPool_SetAggDstOf": (None, [vp, vp, i32]),
    "GPUMemoryPool_SetNodeCounter": (None, [vp, vp, i32]),
    "GPUMemoryPool_SetEdgeCounter": (None, [vp, vp, i32]),
    "GPUMemoryPool_SetFeatureRows": (None, [vp, i32]),
    "GPUMemoryPool_SetCurrentPipe": (None, [vp, i32]),
    "GPUMemoryPool_SetCurrentMode": (None, [vp, i32]),
    "GPUMemoryPool_SetIter": (None, [vp, i32]),
    "GPUMemoryPool_GetPositionMap": (vp, [vp]),
    "GPUMemoryPool_GetBatchSerial": (u32, [vp]),
    "GPUMemoryPool_SetBatchSerial": (None, [vp, u32]),
    "GPUMemoryPool_GetAggSrcId": (vp, [vp]),
    "GPUMemoryPool_GetCacheSearchBuffer": (vp, [vp]),
    "GPUMemoryPool_GetTmpPartIdx": (vp, [vp]),
    "GPUMemoryPool_GetTmpPartOff": (vp, [vp]),
    "GPUMemoryPool_Finalize": (None, [vp]),
    "GPUMemoryPool_Delete": (None, [vp]),
    "NewGPUCache": (vp, []),
    "GPUCache_Initialize": (None, [vp, i64, i32, i32, i32, i32]),
    "GPUCache_InitializeCacheController": (None, [vp, i32, i32]),
    "GPUCache_NodeCapacity": (i32, [vp, i32]),
    "GPUCache_EdgeCapacity": (i32, [vp, i32]),
    "GPUCache_FindFeat": (None, [vp, vp, vp, vp, i32, vp, i32]),
    "GPUCache_FindTopo": (None, [vp, vp, vp, vp, i32, i32, vp, i32]),
    "GPUCache_CandidateSelection": (None, [vp, C.c_int, vp, vp]),
    "GPUCache_CostModel": (None, [vp, C.c_int, vp, vp, vp, i32]),
    "GPUCache_SetCapacity": (None, [vp, i32, i32]),
    "GPUCache_SetPreSc": (None, [vp, C.c_int]),
    "GPUCache_FillUp": (None, [vp, C.c_int, vp, vp]),
    "GPUCache_MaxIdNum": (i32, [vp, i32]),
    "GPUCache_Float_Feature_Cache": (vp, [vp, i32]),
    "GPUCache_ExportFeatureShard": (C.c_int, [vp, i32, vp]),
    "GPUCache_ImportFeatureShard": (C.c_int, [vp, i32, vp]),
    "GPUCache_ShardChunkCount": (i32, [vp, i32]),
    "GPUCache_ShardChunkRows": (i32, [vp, i32]),
    "GPUCache_ShardPitch": (i32, [vp]),
    "GPUCache_GetShardChunk": (vp, [vp, i32, i32]),
    "GPUCache_ShardGeometry": (C.c_int, [vp, i32, vp]),
    "GPUCache_CheckShardGeometry": (C.c_int, [vp, i32, vp]),
    "GPUCache_ExportFeatureShardChunk": (C.c_int, [vp, i32, i32, vp]),
    "GPUCache_ImportFeatureShardChunk": (C.c_int, [vp, i32, i32, vp]),
    "GPUCache_HitSampling": (vp, [vp, i32, C.c_int, C.c_int]),
    "GPUCache_FeatureCacheHitRate": (f64, [vp, i32, vp, vp]),
    "GPUCache_GetNodeAccessedMap": (vp, [vp, i32]),
    "GPUCache_GetEdgeAccessedMap": (vp, [vp, i32]),
    "GPUCache_GetFeatureMap": (vp, [vp, i32]),
    "GPUCache_GetQF": (vp, [vp, i32]),
    "GPUCache_GetQT": (vp, [vp, i32]),
    "GPUCache_Kg": (i32, [vp]),
    "GPUCache_Kc": (i32, [vp]),
    "GPUCache_Alpha": (f64, [vp, i32]),
    "GPUCache_Delete": (None, [vp]),
    "batch_generator_kernel": (None, [vp, vp, vp, vp, i32, i32, i32, i32, i32]),
    "GPU_Random_Sampling": (None, [vp, vp, vp, vp, i32, i32, C.c_int]),
    "get_feature_kernel": (None, [vp, vp, vp, vp, i32, i32, C.c_int]),
    "get_feature_kernel_all": (None, [vp, vp, vp, vp, i32, C.c_int]),
    "get_feature_kernel_agg": (None, [vp, vp, vp, vp, i32, C.c_int]),
    "GPUMemoryPool_SetAggLastHop": (None, [vp, C.c_int]),
    "GPUMemoryPool_GetAggLastHop": (C.c_int, [vp]),
    "GPUMemoryPool_SetAggNorm": (None, [vp, C.c_int]),
    "GPUMemoryPool_GetAggNorm": (C.c_int, [vp]),
    "GPUMemoryPool_GetAggOutDeg": (vp, [vp]),
    "GPUMemoryPool_SetSampleDistinct": (None, [vp, C.c_int]),
    "GPUMemoryPool_GetSampleDistinct": (C.c_int, [vp]),
    "GPUMemoryPool_SetSampling": (None, [vp, C.c_int]),
    "GPUMemoryPool_GetSampling": (C.c_int, [vp]),
    "GPUGraphStorage_SetEdgeWeights": (C.c_int, [vp, vp, i32]),
    "GPUGraphStorage_HasEdgeWeights": (C.c_int, [vp]),
    "GPUGraphStorage_RetainEdgeWeights": (C.c_int, [vp, C.c_int]),
    "GPUGraphStorage_HasRetainedEdgeWeights": (C.c_int, [vp]),
    "GPUMemoryPool_SetWeightedDistinct": (None, [vp, C.c_int]),
    "GPUMemoryPool_GetWeightedDistinct": (C.c_int, [vp]),
    "GPUMemoryPool_SetSharedDraws": (None, [vp, C.c_int]),
    "GPUMemoryPool_GetSharedDraws": (C.c_int, [vp]),
    "GPUMemoryPool_SetEdgeIds": (None, [vp, C.c_int]),
    "GPUMemoryPool_GetEdgeIds": (C.c_int, [vp]),
    "GPUMemoryPool_SetAggEdgeWeight": (None, [vp, C.c_int]),
    "GPUMemoryPool_GetAggEdgeWeight": (C.c_int, [vp]),
    "GPUMemoryPool_GetEdgeIdBuffer": (vp, [vp]),
    "GPUMemoryPool_GetEdgeWeightBuffer": (vp, [vp]),
    "GPUGraphStorage_CopyAliasRows": (C.c_int, [vp, i32, i64, i64, vp, vp]),
    "GPUGraphStorage_SetEdgeFeatures": (C.c_int, [vp, vp, i32, i32]),
    "GPUGraphStorage_GetEdgeFeatureDim": (i32, [vp]),
    "GPUGraphStorage_CopyEdgeFeatureRows": (C.c_int, [vp, i32, i64, i64, vp]),
    "GPUMemoryPool_SetEdgeFeatures": (None, [vp, i32]),
    "GPUMemoryPool_GetEdgeFeatures": (i32, [vp]),
    "GPUMemoryPool_GetEdgeFeatureBuffer": (vp, [vp]),
    "get_edge_feature_kernel": (None, [vp, vp, vp, i32, i32]),
    "get_edge_feature_kernel_all": (None, [vp, vp, vp, i32]),
    "GPUMemoryPool_SetSampleSeed": (None, [vp, C.c_int, u32]),
    "GPUMemoryPool_GetSampleSeed": (C.c_int, [vp, vp]),
    "GPUMemoryPool_BeginRound": (C.c_int, [vp, vp, vp, i32, i32]),
    "GPUMemoryPool_SetLpDraw": (None, [vp, i32, vp]),
    "GPUMemoryPool_GetLpDraw": (i32, [vp]),
    "GPUMemoryPool_SetLpExclude": (None, [vp, i32]),
    "GPUMemoryPool_GetLpExclude": (i32, [vp]),
    "GPUMemoryPool_GetEdgeKeepBuffer": (vp, [vp]),
    "GPUMemoryPool_GetLpExcludedBuffer": (vp, [vp]),
    "legion_lp_pair_slot": (u32, [u32, u32, u32]),
    "GPUMemoryPool_GetRound": (i32, [vp]),
    "legion_exchange_plan": (C.c_int, [vp, vp, vp, vp, i32, vp, vp, vp]),
    "legion_exchange_local": (C.c_int, [vp, vp, vp, vp, i32]),
    "legion_exchange_serve": (None, [vp, vp, i32, vp, i32, vp]),
    "legion_exchange_scatter": (None, [vp, vp, vp, vp, i32, i32]),
    "legion_peer_exchange_gather": (C.c_int, [vp, vp, vp, vp, i32]),
    "legion_peer_exchange_stats": (None, [vp, vp]),
    "GPUMemoryPool_ReleasePeerExchange": (None, [vp]),
    "make_update_plan": (None, [vp, vp, vp, vp, i32, i32]),
    "update_cache": (None, [vp, vp, vp, vp, i32, i32]),
    "NewBatchGenerator": (vp, [C.c_int]), "NewRandomSampler": (vp, [C.c_int]), "NewFeatureExtractor": (vp, [C.c_int]),
    "NewCachePlanner": (vp, [C.c_int]), "NewCacheUpdater": (vp, [C.c_int]),
    "Operator_run": (None, [vp, vp]), "Operator_Delete": (None, [vp]),
    "NewIPCEnv": (vp, [i32]),
    "IPCEnv_MirrorCounters": (None, [vp, i32, i32, vp]),
    "IPCEnv_SetMirror": (None, [vp, i32, i32, i32, i32]),
    "IPCEnv_SlabPinned": (C.c_int, [vp]),
    "IPCEnv_Coordinate": (None, [vp, vp]),
    "IPCEnv_GetMaxStep": (i32, [vp]),
    "IPCEnv_InitializeSamplesBuffer": (None, [vp, i32, i32, i32, i32, i32]),
    "IPCEnv_InitializeFeaturesBuffer": (None, [vp, i32, i32, i32, i32, i32]),
    "IPCEnv_GetRawBatchsize": (i32, [vp]),
    "IPCEnv_GetLocalBatchId": (i32, [vp, i32]),
    "IPCEnv_GetCurrentBatchsize": (i32, [vp, i32, i32]),
    "IPCEnv_GetCurrentMode": (i32, [vp, i32]),
    "IPCEnv_GetIds": (vp, [vp, i32, i32]), "IPCEnv_GetFloatFeatures": (vp, [vp, i32, i32]),
    "IPCEnv_GetLabels": (vp, [vp, i32, i32]), "IPCEnv_GetAggSrc": (vp, [vp, i32, i32]),
    "IPCEnv_GetAggDst": (vp, [vp, i32, i32]), "IPCEnv_GetNodeCounter": (vp, [vp, i32, i32]),
    "IPCEnv_GetEdgeCounter": (vp, [vp, i32, i32]),
    "IPCEnv_IPCPost": (None, [vp, i32, i32]), "IPCEnv_IPCWait": (None, [vp, i32, i32]),
    "IPCEnv_IPCTryWait": (C.c_int, [vp, i32, i32, i32]),
    "IPCEnv_HandoffSpinUs": (C.c_int, []),
    "IPCEnv_Finalize": (None, [vp]), "IPCEnv_GetTrainStep": (i32, [vp]), "IPCEnv_SetHops": (None, [vp, i32]),
    "legion_ipc_set_namespace": (None, [C.c_char_p]),
    "legion_ipc_unlink_namespace": (None, [C.c_char_p, i32]),
    "IPCEnv_MirroredNodeCounter": (i32, [vp, i32, i32, i32]),
    "IPCEnv_SetFeatureRows": (None, [vp, i32, i32]),
    "IPCEnv_SetAggLastHop": (None, [vp, i32]), "IPCEnv_GetAggLastHop": (i32, [vp]), "legion_ipc_client_agg_last_hop": (i32, [vp]),
    "IPCEnv_SetAggNorm": (None, [vp, i32]), "IPCEnv_GetAggNorm": (i32, [vp]), "legion_ipc_client_agg_norm": (i32, [vp]),
    "IPCEnv_SetSampling": (None, [vp, i32]), "IPCEnv_GetSampling": (i32, [vp]), "legion_ipc_client_sampling": (i32, [vp]),
    "IPCEnv_SetSamplingSeed": (None, [vp, i32, u32]), "IPCEnv_GetSamplingSeed": (i32, [vp, vp]), "legion_ipc_client_sampling_seed": (i32, [vp, vp]),
    # the words of the "<name>_ext2" object (created only when one of them is on) and the served edge buffers
    "IPCEnv_SetLpDraw": (None, [vp, i32]), "IPCEnv_GetLpDraw": (i32, [vp]), "legion_ipc_client_lp_draw": (i32, [vp]),
    "IPCEnv_SetWeightedDistinct": (None, [vp, i32]), "IPCEnv_GetWeightedDistinct": (i32, [vp]), "legion_ipc_client_weighted_distinct": (i32, [vp]),
    "IPCEnv_SetSharedDraws": (None, [vp, i32]), "IPCEnv_GetSharedDraws": (i32, [vp]), "legion_ipc_client_shared_draws": (i32, [vp]),
    "IPCEnv_SetEdgeIds": (None, [vp, i32]), "IPCEnv_GetEdgeIds": (i32, [vp]), "legion_ipc_client_edge_ids": (i32, [vp]),
    "IPCEnv_SetEdgeWeights": (None, [vp, i32]), "IPCEnv_GetEdgeWeights": (i32, [vp]), "legion_ipc_client_edge_weights": (i32, [vp]),
    "IPCEnv_SetAggEdgeWeight": (None, [vp, i32]), "IPCEnv_GetAggEdgeWeight": (i32, [vp]), "legion_ipc_client_agg_edge_weight": (i32, [vp]),
    "IPCEnv_RegisterEdgeBuffers": (None, [vp, i32, i32, vp, vp, i32]), "IPCEnv_GetEdgeElems": (i32, [vp, i32]),
    "legion_ipc_client_edge_buffer": (vp, [vp, i32]), "legion_ipc_client_edge_elems": (i32, [vp]),
    "legion_ipc_client_open": (vp, [i32]), "legion_ipc_client_wait": (None, [vp]),
    "legion_ipc_client_post": (None, [vp]), "legion_ipc_client_post_nosync": (None, [vp]), "legion_ipc_client_buffer": (vp, [vp, i32]),
    "legion_ipc_client_steps": (None, [vp, vp]), "legion_ipc_client_hops": (i32, [vp]), "legion_ipc_client_feature_rows": (i32, [vp]),
    "legion_ipc_client_read_counters": (None, [vp, vp, vp]), "legion_ipc_client_close": (None, [vp]),
    "legion_runner_gather_estimate": (C.c_int, [i32, f64, f64, vp, vp]),
    "NewGPURunner": (vp, []), "Runner_Initialize": (None, [vp, vp]),
    "Runner_InitializeFeaturesBuffer": (None, [vp, vp]), "Runner_RunPreSc": (None, [vp, vp]),
    "Runner_RunOnce": (None, [vp, vp]), "Runner_Finalize": (None, [vp, vp]), "Runner_GetMemoryPool": (vp, [vp]), "Runner_ShortBatches": (i64, [vp]),
    "Runner_Delete": (None, [vp]),
    "NewGPUServer": (vp, []), "Server_SetFanout": (None, [vp, vp, i32]),
    "Server_SetMetaConfigPath": (None, [vp, C.c_char_p]), "Server_Initialize": (None, [vp, C.c_int]),
    "Server_PreSc": (None, [vp, C.c_int]), "Server_Run": (None, [vp]), "Server_Finalize": (None, [vp]),
    "Server_Delete": (None, [vp]),
    "legion_synth_degrees": (None, [vp, vp, i32, i32, vp]),
    "legion_synth_neighbors": (None, [vp, vp, i64, i64, i32, u32, u32]),
    "legion_synth_neighbors_skew": (None, [vp, vp, i64, i64, i32, u32, u32, i32]),
    "legion_synth_lp_seeds": (None, [vp, vp, vp, vp, i64, i32, vp, vp, i32, u32]),
    "legion_synth_features": (None, [vp, vp, i64, i64, i32]),
    "legion_synth_features_pitched": (None, [vp, vp, i64, i64, i32, i32]),
    "legion_synth_labels": (None, [vp, vp, i32, i32, i32]),
    "legion_synth_edge_weights": (None, [vp, vp, i64, i64]),
    "legion_synth_edge_features": (None, [vp, vp, i64, i64, i32]),
    "legion_synth_seed_ids": (None, [vp, vp, i64, i64, i32, u32, u32, i32, i32]),
    "legion_synth_spec": (C.c_int, [C.c_char_p, f64, vp]),
    "legion_synth_label_host": (i32, [i32, i32]),
    "legion_synth_seed_id_host": (i32, [i64, i32, u32, u32]),
    "legion_copy_f4": (None, [vp, vp, vp, i64]),
    "legion_sum_words": (None, [vp, vp, i64, vp]),
    "GPUMemoryPool_GetCandidateBuffer": (vp, [vp]),
    "legion_copy_f4_cfg": (C.c_int, [vp, vp, vp, i64, i32, i32, i32, i32]),
    "legion_rng_probe": (None, [vp, vp, vp, vp, i32]),
    "legion_distinct_probe": (None, [vp, vp, vp, vp, i32, vp, i32]),
    "legion_seeded_rng_probe": (None, [vp, u32, i32, i32, vp, vp, vp, i32]),
    "legion_seeded_distinct_probe": (None, [vp, u32, i32, i32, vp, vp, vp, i32, vp, i32]),
    "legion_perm_probe": (None, [vp, u32, i32, i32, vp]),
    "legion_weighted_probe": (None, [vp, vp, vp, vp, vp, vp, vp, vp, i32]),
    "legion_weighted_distinct_probe": (None, [vp, vp, vp, vp, vp, vp, vp, vp, i32]),
    "legion_shared_draw_probe": (None, [vp, vp, vp, vp, i32]),
    "legion_weighted_shared_probe": (None, [vp, vp, vp, vp, vp, vp, i32]),
    "legion_lp_draw_probe": (None, [vp, u32, i32, i32, vp, vp, i32, vp, vp, i32]),
    "legion_seeded_draw_word": (u32, [u32, i32, i32]),
    "legion_seeded_shuffle_key": (u32, [u32, i32]),
    "legion_sampler_cu_count": (i32, []),
    "GPUMemoryPool_ScratchInfo": (C.c_int, [vp, i32, i32, vp]),
}

# GPUMemoryPool_ScratchInfo (include/legion_amd.h: LEGION_SCRATCH_*): what an element of a pool buffer is, and when its contents are dead
SCRATCH_KINDS = ("id", "slot_state", "count", "count_pair", "device_pointer", "float", "table_entry")
SCRATCH_LIFETIMES = ("hop", "batch", "table", "state")


class LegionScratchInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ptr", vp), ("bytes", i64), ("kind", i32), ("elem_bytes", i32), ("lifetime", i32), ("per_pipe", i32)]


def pool_scratch(pool, pipe=0):
    """The pool's device buffers as GPUMemoryPool_ScratchInfo lists them for `pipe`: [dict(name, ptr, bytes, kind, elem_bytes, lifetime,
    per_pipe)], kind and lifetime as the words of SCRATCH_KINDS / SCRATCH_LIFETIMES; ptr is None while a buffer is not allocated."""
    out, info = [], LegionScratchInfo()
    while True:
        r = lib().GPUMemoryPool_ScratchInfo(pool, len(out), int(pipe), C.byref(info))
        if r == 1:
            return out
        if r != 0:
            check()
            raise RuntimeError("GPUMemoryPool_ScratchInfo failed")
        out.append(dict(name=info.name.decode(), ptr=info.ptr, bytes=int(info.bytes), kind=SCRATCH_KINDS[info.kind], elem_bytes=int(info.elem_bytes),
                        lifetime=SCRATCH_LIFETIMES[info.lifetime], per_pipe=bool(info.per_pipe)))


def lib():
    """The loaded HIP library.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `make -C legion-1_amd/csrc` "
                               "(or __graft_entry__.build()); there is no CPU fallback")
        _lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS.items():
            fn = getattr(_lib, name)
            fn.restype = res
            fn.argtypes = args
    return _lib


def check():
    """Raise if the library recorded a (sticky) error."""
    msg = lib().legion_last_error()
    if msg:
        text = msg.decode()
        lib().legion_clear_error()
        raise RuntimeError(text)


# ------------------------------------------------------------------------------------------------------
# small device-memory helpers (raw hipMalloc through the C ABI; no torch needed)
# ------------------------------------------------------------------------------------------------------
class DevBuf:
    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.ptr = lib().d_alloc_space(max(self.nbytes, 16))
        check()

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DevBuf":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        if a.nbytes:
            lib().d_copy_h_2_d(b.ptr, a.ctypes.data, a.nbytes)
        b.dtype, b.shape = a.dtype, a.shape
        return b

    def to_numpy(self, dtype, count: int, offset_bytes: int = 0) -> np.ndarray:
        out = np.empty(int(count), dtype=dtype)
        if out.nbytes:
            lib().d_copy_d_2_h(out.ctypes.data, self.ptr + offset_bytes, out.nbytes)
        return out

    def free(self):
        if self.ptr:
            lib().d_free_space(self.ptr)
            self.ptr = None


def read_dev(ptr: int, dtype, count: int) -> np.ndarray:
    out = np.empty(int(count), dtype=dtype)
    if out.nbytes:
        lib().d_copy_d_2_h(out.ctypes.data, ptr, out.nbytes)
    return out


def _ptr_array(ptrs):
    arr = (vp * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr


class Engine:
    """Host-side assembly of the reference objects for G logical GPUs (one process), the way
    GPUGraphStore::Initialze + GPURunner::Initialize do it (GPUGraphStore.cu:429-470,
    Server.cu:169-271), but driven from arrays instead of files.  Output buffers are raw device
    allocations (or externally supplied pointers) -- no IPC involved.

    ``indptr`` / ``indices`` / ``features`` may be numpy arrays (copied to the chosen location)
    or integer device pointers (``*_location`` = LOC_DEVICE).  ``edge_weights``: float32[E], one weight per CSR entry
    (GPUGraphStorage_SetEdgeWeights: the graph's alias table, what sample="weighted" draws from); set_edge_weights() replaces or drops it.
    ``retain_edge_weights=True`` (GPUGraphStorage_RetainEdgeWeights): every table build keeps the weights on the device beside the
    table, which run_batch(sample="weighted", weighted_distinct=True) reads.
    ``edge_features``: float32 [E, dim], one row per CSR entry (GPUGraphStorage_SetEdgeFeatures), what run_batch(edge_ids=True,
    edge_features=True) gathers by edge id; a numpy array, or an integer device pointer together with ``edge_feature_dim``.
    set_edge_features() replaces or drops it.
    """

    def __init__(self, indptr, indices, features, V, F, seeds, batch_size, fanout, G=1,
                 csr_location=LOC_DEVICE, features_location=LOC_DEVICE, cache_memory=0, train_step=1, epoch=1,
                 pipeline_depth=1, E=None, local_devs=None, features_pitch=0, edge_weights=None, retain_edge_weights=False,
                 edge_features=None, edge_feature_dim=None):
        L = lib()
        # one process per GPU: the other members of the clique are remote (legion_set_remote_device)
        self.local_devs = list(range(int(G))) if local_devs is None else list(local_devs)
        for g in range(int(G)):
            L.legion_set_remote_device(g, 0 if g in self.local_devs else 1)
        self.L, self.G, self.V, self.F = L, int(G), int(V), int(F)
        L.SetGPUDevice(self.local_devs[0])      # the shared tables below live on the first local GPU
        self.fanout = np.asarray(fanout, dtype=np.int32)
        self.hops = len(self.fanout)
        self.batch_size = int(batch_size)
        self._keep = []
        self._owned = []

        def place(arr, location, dtype):
            if isinstance(arr, (int, np.integer)):
                return int(arr)
            arr = np.ascontiguousarray(arr, dtype=dtype)
            if location == LOC_DEVICE:
                b = DevBuf.from_numpy(arr)
                self._owned.append(b)
                return b.ptr
            p = L.host_alloc_space64(max(arr.nbytes, 16))
            C.memmove(p, arr.ctypes.data, arr.nbytes)
            self._owned.append(("host", p))
            return p

        self.E = int(E if E is not None else (indptr[-1] if not isinstance(indptr, (int, np.integer)) else 0))
        self.indptr_ptr = place(indptr, csr_location, np.int64)
        self.indices_ptr = place(indices, csr_location, np.int32)
        self.features_ptr = place(features, features_location, np.float32) if features is not None else None

        # seeds: dict(train=[(ids, labels)] * G, valid=..., test=...) with numpy arrays or (ptr, n) pairs
        info = LegionBuildInfo()
        info.partition_count = self.G
        for key, pre in (("train", "training"), ("valid", "validation"), ("test", "testing")):
            sets = seeds.get(key)
            if sets is None:
                sets = [(np.zeros(0, np.int32), np.zeros(0, np.int32))] * self.G
            nums = np.zeros(self.G, dtype=np.int32)
            idp, lbp = [], []
            for g, (ids, labs) in enumerate(sets):
                if isinstance(ids, tuple):          # (device_ptr, n)
                    nums[g] = ids[1]
                    idp.append(ids[0])
                    lbp.append(labs[0])
                else:
                    ids = np.ascontiguousarray(ids, dtype=np.int32)
                    labs = np.ascontiguousarray(labs, dtype=np.int32)
                    self._keep += [ids, labs]
                    nums[g] = len(ids)
                    idp.append(ids.ctypes.data)
                    lbp.append(labs.ctypes.data)
            ida, lba = _ptr_array(idp), _ptr_array(lbp)
            self._keep += [nums, ida, lba]
            setattr(info, pre + "_set_num", nums.ctypes.data)
            setattr(info, pre + "_set_ids", C.cast(ida, vp))
            setattr(info, pre + "_labels", C.cast(lba, vp))
            setattr(self, key + "_num", nums)
        info.total_num_nodes, info.float_attr_len = self.V, self.F
        info.host_float_attrs, info.features_location = self.features_ptr, features_location
        info.float_attr_pitch = int(features_pitch)        # 0 = dense rows; > F: the table was built with padded rows
        info.csr_node_index, info.csr_dst_node_ids, info.csr_location = self.indptr_ptr, self.indices_ptr, csr_location
        info.total_edge_num, info.cache_edge_num = self.E, 0
        info.epoch, info.raw_batch_size = epoch, self.batch_size
        self.info = info

        self.graph = L.NewGPUMemoryGraphStorage()
        L.GPUGraphStorage_Build(self.graph, C.byref(info))
        self.noder = L.NewGPUMemoryNodeStorage()
        L.GPUNodeStorage_Build(self.noder, C.byref(info))
        self.cache = L.NewGPUCache()
        L.GPUCache_Initialize(self.cache, int(cache_memory), 0, self.F, int(train_step), self.G)
        check()
        if retain_edge_weights:
            L.GPUGraphStorage_RetainEdgeWeights(self.graph, 1)
            check()
        if edge_weights is not None:
            self.set_edge_weights(edge_weights)
        self.edge_feature_dim = 0
        if edge_features is not None:
            self.set_edge_features(edge_features, edge_feature_dim)
        elif edge_feature_dim is not None:
            raise ValueError("edge_feature_dim without edge_features: the width belongs to a table")
        self.depth = int(pipeline_depth)
        self.pools, self.out = [None] * self.G, [None] * self.G
        for g in self.local_devs:
            L.SetGPUDevice(g)
            L.GPUCache_InitializeCacheController(self.cache, g, self.V)
            pool = L.NewGPUMemoryPool(self.depth)
            L.GPUMemoryPool_AllocateScratch(pool, self.V, self.batch_size, self.fanout.ctypes.data, self.hops)
            check()
            n = L.GPUMemoryPool_NumIds(pool)
            self.num_ids = n
            pipes = []
            for q in range(self.depth):
                o = dict(ids=DevBuf(n * 4), labels=DevBuf(self.batch_size * 4), src=DevBuf(n * 4), dst=DevBuf(n * 4),
                         nc=DevBuf(layout.COUNTER_BYTES), ec=DevBuf(layout.COUNTER_BYTES), feat=None)
                L.GPUMemoryPool_SetSampledIds(pool, o["ids"].ptr, q)
                L.GPUMemoryPool_SetLabels(pool, o["labels"].ptr, q)
                L.GPUMemoryPool_SetAggSrcOf(pool, o["src"].ptr, q)
                L.GPUMemoryPool_SetAggDstOf(pool, o["dst"].ptr, q)
                L.GPUMemoryPool_SetNodeCounter(pool, o["nc"].ptr, q)
                L.GPUMemoryPool_SetEdgeCounter(pool, o["ec"].ptr, q)
                pipes.append(o)
            self.pools[g] = pool
            self.out[g] = pipes
        self.streams = [None] * self.G
        self._graphs = []
        self._agg = {}      # (dev, pipe) -> the pipe's last batch was handed over aggregated (run_batch(agg_last_hop=True))
        self._seed_state = {}   # dev -> (seed or None, round) the pool was last put into (run_batch / capture_batch / run_graph)
        self._norm = {}     # (dev, pipe) -> ... with normalised sums (run_batch(agg_norm="both"))
        self._eid = {}      # (dev, pipe) -> the pipe's last batch left its edge ids (run_batch(edge_ids=True))
        self._lpx = {}      # (dev, pipe) -> the pipe's last batch had its target edges marked (run_batch(lp_exclude=k))
        self._efeat = {}    # (dev, pipe) -> the row width the pipe's last batch had its edge rows gathered at (run_batch(edge_features=True)), 0: not
        check()

    # ---- weighted sampling: the graph's alias table ------------------------------------------------------
    def set_edge_weights(self, w):
        """float32[E] weights in `indices` order -> the graph's alias table (replacing an earlier one); None drops it.  A refused table
        (a negative, NaN or infinite weight) raises and leaves the earlier one in place."""
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float32)
            if len(w) != self.E:
                raise ValueError("edge_weights: one float32 per CSR entry (%d), got %d" % (self.E, len(w)))
        self.L.GPUGraphStorage_SetEdgeWeights(self.graph, None if w is None else w.ctypes.data, LOC_HOST_PAGEABLE)
        check()

    # ---- edge features: the graph's per-edge table --------------------------------------------------------
    def set_edge_features(self, x, dim=None, location=None):
        """float32 [E, dim] rows in `indices` order -> the graph's edge-feature table (replacing an earlier one); None drops it.  x: a numpy
        array (dim is its second axis; a flat array needs dim) or an integer device pointer with dim (location: LOC_DEVICE)."""
        if x is None:
            self.L.GPUGraphStorage_SetEdgeFeatures(self.graph, None, 0, LOC_HOST_PAGEABLE)
            check()
            self.edge_feature_dim = 0
            return
        if isinstance(x, (int, np.integer)):
            if dim is None or int(dim) < 1:
                raise ValueError("edge_features: a device pointer needs edge_feature_dim >= 1")
            ptr, dim, location = int(x), int(dim), LOC_DEVICE if location is None else location
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            if x.ndim == 2 and dim is None:
                dim = x.shape[1]
            if dim is None or int(dim) < 1 or x.size != self.E * int(dim) or (x.ndim == 2 and x.shape != (self.E, int(dim))):
                raise ValueError("edge_features: float32 [E, dim] with one row per CSR entry (%d), got shape %s and dim %s" % (self.E, x.shape, dim))
            ptr, dim, location = x.ctypes.data, int(dim), LOC_HOST_PAGEABLE
        self.L.GPUGraphStorage_SetEdgeFeatures(self.graph, ptr, dim, location)
        check()
        self.edge_feature_dim = int(self.L.GPUGraphStorage_GetEdgeFeatureDim(self.graph))

    def edge_feature_rows(self, dev=0, e0=0, n=None):
        """float32 [n, dim]: rows [e0, e0 + n) of logical GPU dev's edge-feature table."""
        n = self.E - e0 if n is None else int(n)
        out = np.empty((n, self.edge_feature_dim), np.float32)
        self.L.GPUGraphStorage_CopyEdgeFeatureRows(self.graph, dev, int(e0), n, out.ctypes.data)
        check()
        return out

    def has_edge_weights(self):
        return bool(self.L.GPUGraphStorage_HasEdgeWeights(self.graph))

    def has_retained_edge_weights(self):
        return bool(self.L.GPUGraphStorage_HasRetainedEdgeWeights(self.graph))

    def alias_rows(self, dev=0, e0=0, n=None):
        """(thr uint32[n], alias_id int32[n]): entries [e0, e0 + n) of logical GPU dev's alias table."""
        n = self.E - e0 if n is None else int(n)
        thr, alias = np.empty(n, np.uint32), np.empty(n, np.int32)
        self.L.GPUGraphStorage_CopyAliasRows(self.graph, dev, int(e0), n, thr.ctypes.data, alias.ctypes.data)
        check()
        return thr, alias

    # ---- feature buffers ------------------------------------------------------------------------------
    def alloc_features(self, rows=None):
        rows = self.num_ids if rows is None else int(rows)
        for g in self.local_devs:
            self.L.SetGPUDevice(g)
            for q in range(self.depth):
                b = DevBuf(rows * self.F * 4)
                self.out[g][q]["feat"] = b
                self.L.GPUMemoryPool_SetFloatFeatures(self.pools[g], b.ptr, q)
            self.L.GPUMemoryPool_SetFeatureRows(self.pools[g], rows)
        self.feature_rows = rows
        check()

    # ---- one batch through the reference's launcher API -----------------------------------------------------
    def run_batch(self, dev=0, counter=0, mode=TRAINMODE, is_presc=False, gather=True, plan=True, pipe=0,
                  batch_size=None, per_level=True, stream=None, sync=True, agg_last_hop=False, agg_norm=None, sample="replace",
                  seed=None, round=0, lp_draw=0, weighted_distinct=False, shared_draws=False, edge_ids=False, agg_edge_weight=False,
                  edge_features=False, lp_exclude=0):
        """lp_exclude: 0, or k > 0 (GPUMemoryPool_SetLpExclude): a training batch of 3 k seeds [src | pos | neg] additionally leaves edge_keep[e] = 0
        for every COO edge that joins a target pair {ids[i], ids[k + i]}, either direction, and 1 for every other, with the zeros per hop in
        lp_excluded (INTEGRATION.md "Target-edge exclusion"); result() then returns `edge_keep` uint8 [n_edges] and `lp_excluded` int32[8].  A
        batch of another mode keeps every edge; a pre-sampling batch marks nothing.  Refused by the library together with agg_last_hop and with an
        lp_draw of another k.  Set on every call like `lp_draw`.
        edge_features (GPUMemoryPool_SetEdgeFeatures, only with edge_ids=True on an Engine with an edge-feature table): the batch additionally
        leaves edge_feat[e, :] = X[edge_ids[e], :] in the pipe's buffer -- gathered per hop (get_edge_feature_kernel) where the node rows are
        gathered per level, else in one launch behind the last hop (get_edge_feature_kernel_all); result() then returns `edge_feat` float32
        [n_edges, dim].  A pre-sampling batch gathers nothing.  Set on every call like `edge_ids`.
        agg_edge_weight (GPUMemoryPool_SetAggEdgeWeight, only with agg_last_hop=True, edge_ids=True and without agg_norm, on an
        Engine(retain_edge_weights=True)): `nbr_sum` holds the sums with every row scaled by its draw's edge weight, S_e of INTEGRATION.md
        "Edge-weighted sums".  Set on every call like `agg_norm`.
        edge_ids (GPUMemoryPool_SetEdgeIds): the batch additionally leaves every COO edge's position in the whole CSR in the pipe's buffer, and
        its weight on an Engine(retain_edge_weights=True); result() then returns `edge_ids` int64 [n_edges] (and `edge_w` float32 [n_edges]).
        Refused by the library under sample="weighted" without weighted_distinct; a pre-sampling batch hands nothing over.  Set on every call
        like `sample`.
        shared_draws (GPUMemoryPool_SetSharedDraws, only with sample="distinct"): the distinct draws are keyed by the neighbour node, so rows
        that see the same neighbours pick the same ones; seed=None draws under word 0 (the same node keys in every batch).  Set on every call
        like `sample`.  Also allowed with sample="weighted", weighted_distinct=True: the weighted draws without replacement take their
        uniforms per neighbour node (INTEGRATION.md "Weighted shared-key sampling").
        weighted_distinct (GPUMemoryPool_SetWeightedDistinct, only with sample="weighted" on an Engine(retain_edge_weights=True)): the
        weighted draws are without replacement -- min(columns of weight > 0, fan-out) distinct columns per row, by exponential keys.  Set on
        every call like `sample`.
        lp_draw: 0, or k > 0 (GPUMemoryPool_SetLpDraw, only under a seed): a training batch is 3 k seeds [src | pos | neg], the src third
        from the round's triple-shuffled training list, pos and neg drawn for this batch.  Set on every call like `seed`; a change re-runs
        GPUMemoryPool_BeginRound.
        seed: None (the reference's draws: the same batch every epoch) or a uint32 (GPUMemoryPool_SetSampleSeed: the batch's draws come
        from W(seed, round, counter) and a training batch reads the round's shuffled list); round: the epoch the batch belongs to.  Like
        `sample`, both SET the pool's state on every call, and GPUMemoryPool_BeginRound runs when the seed, the round or the device's
        training list changed.
        sample: "replace" (the reference's draws with replacement) or "distinct" (GPUMemoryPool_SetSampleDistinct: min(degree, fan-out)
        distinct neighbours per row, pre-sampling batches included) or "weighted" (GPUMemoryPool_SetSampling(pool, 2): with replacement, in
        proportion to the Engine's edge_weights; refused without them).  Like agg_last_hop and agg_norm, the argument SETS the pool's mode on
        every call: a mode switched on through GPUMemoryPool_SetSampleDistinct directly is switched back by a run_batch() without sample="distinct".
        agg_last_hop: the aggregated hand-off (get_feature_kernel_agg) -- feature rows of the levels < H (per level behind each hop,
        or all of them inside that call with per_level=False) and the last hop as neighbour sums; result() then returns
        `features` [n_in, F] and `nbr_sum` [N, F].  agg_norm="both" (only with agg_last_hop): the sums weighted by out-degree^-1/2 inside
        block 1 (GPUMemoryPool_SetAggNorm); result() additionally returns `out_deg` int32 [n]."""
        L, pool = self.L, self.pools[dev]
        # a pre-sampling batch aggregates nothing; gather=False: the sampler side of an aggregated batch (the last hop's draws kept per pipe)
        agg, norm = self._set_modes(dev, agg_last_hop, agg_norm, sample, seed, round, stream, is_presc=is_presc, lp_draw=lp_draw, weighted_distinct=weighted_distinct,
                                     shared_draws=shared_draws, edge_ids=edge_ids, agg_edge_weight=agg_edge_weight, edge_features=edge_features, lp_exclude=lp_exclude)
        self._lpx[(dev, pipe)] = bool(lp_exclude) and not is_presc
        efeat = bool(edge_features) and not is_presc
        ef_per_hop = efeat and gather and per_level
        self._eid[(dev, pipe)] = bool(edge_ids) and not is_presc
        self._efeat[(dev, pipe)] = self.edge_feature_dim if efeat else 0
        self._agg[(dev, pipe)] = agg and gather
        self._norm[(dev, pipe)] = norm and gather
        L.GPUMemoryPool_SetCurrentPipe(pool, pipe)
        L.GPUMemoryPool_SetCurrentMode(pool, mode)
        L.GPUMemoryPool_SetIter(pool, counter)
        bs = self.batch_size if batch_size is None else batch_size
        L.batch_generator_kernel(stream, self.noder, self.cache, pool, bs, counter, dev, dev, mode)
        if gather and not is_presc and per_level:
            L.get_feature_kernel(stream, self.cache, self.noder, pool, dev, 1, 1)
        for h in range(self.hops):
            L.GPU_Random_Sampling(stream, self.graph, self.cache, pool, int(self.fanout[h]), 2 * h + 2, int(is_presc))
            if ef_per_hop:
                L.get_edge_feature_kernel(stream, self.graph, pool, dev, 2 * h + 2)
            if gather and not is_presc and per_level and not (agg and h == self.hops - 1):
                L.get_feature_kernel(stream, self.cache, self.noder, pool, dev, 2 * h + 3, 1)
        if agg and gather:
            L.get_feature_kernel_agg(stream, self.cache, self.noder, pool, dev, 1)
        elif gather and not is_presc and not per_level:
            L.get_feature_kernel_all(stream, self.cache, self.noder, pool, dev, 1)
        if efeat and not ef_per_hop:
            L.get_edge_feature_kernel_all(stream, self.graph, pool, dev)
        if plan:
            L.make_update_plan(stream, self.graph, self.cache, pool, dev, mode)
            L.update_cache(stream, self.cache, self.noder, pool, dev, mode)
        if sync:
            L.d_stream_sync(stream)
            check()

    def _set_modes(self, dev, agg, norm, sample, seed, round, stream, is_presc=False, lp_draw=0, weighted_distinct=False, shared_draws=False, edge_ids=False,
                   agg_edge_weight=False, edge_features=False, lp_exclude=0):
        """The pool's serving modes := the arguments of run_batch / capture_batch, validated; the library is only called for what differs
        (inside a capture nothing does: capture_batch set everything before Begin).  Returns (aggregated, normalised) as set."""
        if norm not in (None, "both"):
            raise ValueError("agg_norm: None or 'both'")
        if norm and not agg:
            raise ValueError("agg_norm needs agg_last_hop=True: only the last hop's neighbour sums are normalised")
        if agg_edge_weight and not (agg and edge_ids):
            raise ValueError("agg_edge_weight needs agg_last_hop=True, edge_ids=True: the last hop's neighbour sums are scaled by the edge_w the edge-id mode hands over")
        if agg_edge_weight and norm:
            raise ValueError("agg_edge_weight and agg_norm together are not in this build: GraphConv(norm='both', edge_weight=) rounds twice per product")
        if edge_features and not edge_ids:
            raise ValueError("edge_features=True needs edge_ids=True: a row is gathered by the id the edge-id mode hands over")
        if edge_features and not self.edge_feature_dim:
            raise ValueError("edge_features=True needs the Engine's edge-feature table (Engine(edge_features=...) or set_edge_features())")
        if sample not in ("replace", "distinct", "weighted"):
            raise ValueError("sample: 'replace', 'distinct' or 'weighted'")
        if weighted_distinct and sample != "weighted":
            raise ValueError("weighted_distinct=True needs sample='weighted': the flag turns the weighted draws into draws without replacement")
        if shared_draws and sample != "distinct" and not (sample == "weighted" and weighted_distinct):
            raise ValueError("shared_draws=True needs sample='distinct': the flag keys the distinct draws by the neighbour node")
        if sample == "weighted" and not self.has_edge_weights():
            raise ValueError("sample='weighted' needs the Engine's edge_weights (Engine(edge_weights=...) or set_edge_weights())")
        if weighted_distinct and not self.has_retained_edge_weights():
            raise ValueError("weighted_distinct=True needs the weights kept on the device: Engine(..., edge_weights=..., retain_edge_weights=True)")
        L, pool = self.L, self.pools[dev]
        L.SetGPUDevice(dev)
        agg = bool(agg) and not is_presc
        norm = int(agg and norm == "both")
        # edge ids are refused together with the alias rule, whichever is set second: off in front of a change of the draw rule, on (again) behind it
        rule = (("replace", "distinct", "weighted").index(sample), int(bool(weighted_distinct)))
        # the edge-weighted sums sit on top of the aggregated mode and of edge ids, and exclude a norm: off in front of everything they depend on, on behind it
        ew = int(bool(agg_edge_weight) and agg)
        # target-edge exclusion is refused together with the aggregated last hop and with drawn thirds of another k: off (or at its new k) in front of both
        # (a pre-sampling batch marks nothing)
        lpx = 0 if is_presc else int(lp_exclude)
        if L.GPUMemoryPool_GetLpExclude(pool) != lpx and (agg or lpx == 0 or (L.GPUMemoryPool_GetLpDraw(pool) not in (0, lpx))):
            L.GPUMemoryPool_SetLpExclude(pool, 0)
        eid_off = L.GPUMemoryPool_GetEdgeIds(pool) and (not edge_ids or rule != (L.GPUMemoryPool_GetSampling(pool), L.GPUMemoryPool_GetWeightedDistinct(pool)))
        if L.GPUMemoryPool_GetAggEdgeWeight(pool) and (not ew or eid_off):
            L.GPUMemoryPool_SetAggEdgeWeight(pool, 0)
        # edge features sit on top of edge ids: off in front of them, on (at the table's width; a pre-sampling batch gathers nothing) behind them
        ef = self.edge_feature_dim if edge_features and not is_presc else 0
        if L.GPUMemoryPool_GetEdgeFeatures(pool) and (not ef or eid_off):
            L.GPUMemoryPool_SetEdgeFeatures(pool, 0)
        if eid_off:
            L.GPUMemoryPool_SetEdgeIds(pool, 0)
        for mode, want in (("Sampling", ("replace", "distinct", "weighted").index(sample)), ("WeightedDistinct", int(bool(weighted_distinct))), ("SharedDraws", int(bool(shared_draws))), ("AggLastHop", int(agg)), ("AggNorm", norm)):   # the last two allocate
            if getattr(L, "GPUMemoryPool_Get" + mode)(pool) != want:
                getattr(L, "GPUMemoryPool_Set" + mode)(pool, want)
        if L.GPUMemoryPool_GetEdgeIds(pool) != int(bool(edge_ids)):   # allocates on the first switch on
            L.GPUMemoryPool_SetEdgeIds(pool, int(bool(edge_ids)))
            check()
        if L.GPUMemoryPool_GetAggEdgeWeight(pool) != ew:   # allocates where the norm has not
            L.GPUMemoryPool_SetAggEdgeWeight(pool, ew)
            check()
        if L.GPUMemoryPool_GetEdgeFeatures(pool) != ef:   # allocates on the first switch on, reallocates at another width
            L.GPUMemoryPool_SetEdgeFeatures(pool, ef)
            check()
        self._set_seed(dev, seed, round, stream, lp_draw)
        if L.GPUMemoryPool_GetLpExclude(pool) != lpx:   # allocates on the first switch on, reallocates the pair table at another capacity
            L.GPUMemoryPool_SetLpExclude(pool, lpx)
            check()
        return agg, bool(norm)

    def _set_seed(self, dev, seed, round, stream, lp_draw=0):
        """The pool's seeded state := (seed, round, lp_draw); BeginRound on `stream` when any of them changed (not callable inside a capture:
        there the state is what capture_batch set before Begin)."""
        L, pool = self.L, self.pools[dev]
        want = (None if seed is None else int(seed) & 0xFFFFFFFF, int(round), int(lp_draw))
        if self._seed_state.get(dev, (None, 0, 0)) == want:
            return
        L.GPUMemoryPool_SetSampleSeed(pool, int(seed is not None), want[0] or 0)
        if L.GPUMemoryPool_GetLpDraw(pool) != want[2]:
            L.GPUMemoryPool_SetLpDraw(pool, want[2], self.graph)
        L.GPUMemoryPool_BeginRound(stream, pool, self.noder, dev, want[1])
        check()
        self._seed_state[dev] = want

    # ---- the same batch recorded once as a hipGraph (one launch per batch) ---------------------------------------
    def capture_batch(self, dev=0, mode=TRAINMODE, gather=True, plan=True, pipe=0, batch_size=None, per_level=True,
                      stream=None, agg_last_hop=False, agg_norm=None, sample="replace", seed=None, round=0, lp_draw=0, weighted_distinct=False, shared_draws=False,
                      edge_ids=False, agg_edge_weight=False, edge_features=False, lp_exclude=0):
        """Record run_batch(dev, <any counter>, mode, ...) on `stream`; returns the graph handle for run_graph().  A graph recorded with a
        seed replays only while the pool is seeded (and the other way round); the seed's value and the round may change between replays:
        run_graph(..., seed=, round=).  lp_draw: as run_batch; a graph replays only in the lp_draw state it was recorded in, and
        only in the weighted_distinct, the shared_draws, the edge_ids, the agg_edge_weight and the lp_exclude state, and at the edge-feature
        width, it was recorded in."""
        L = self.L
        L.SetGPUDevice(dev)
        if stream is None:
            if self.streams[dev] is None:
                self.streams[dev] = L.d_stream_create()
            stream = self.streams[dev]
        # a recording keeps its modes, and setting them allocates (the aggregated modes' buffers, the shuffled copy): not between Begin and End
        self._set_modes(dev, agg_last_hop, agg_norm, sample, seed, round, stream, lp_draw=lp_draw, weighted_distinct=weighted_distinct, shared_draws=shared_draws,
                        edge_ids=edge_ids, agg_edge_weight=agg_edge_weight, edge_features=edge_features, lp_exclude=lp_exclude)
        if L.GPUMemoryPool_BeginBatchCapture(self.pools[dev], stream) != 0:
            check()
            raise RuntimeError("BeginBatchCapture failed")
        self.run_batch(dev, 0, mode=mode, gather=gather, plan=plan, pipe=pipe, batch_size=batch_size, per_level=per_level,
                       stream=stream, sync=False, agg_last_hop=agg_last_hop, agg_norm=agg_norm, sample=sample, seed=seed, round=round, lp_draw=lp_draw,
                       weighted_distinct=weighted_distinct, shared_draws=shared_draws, edge_ids=edge_ids, agg_edge_weight=agg_edge_weight,
                       edge_features=edge_features, lp_exclude=lp_exclude)
        g = L.GPUMemoryPool_EndBatchCapture(self.pools[dev], stream)
        check()
        if not g:
            raise RuntimeError("EndBatchCapture failed")
        self._graphs.append(g)
        return (g, stream, dev)

    def run_graph(self, handle, counter, sync=True, seed=False, round=None, lp_draw=None):
        """seed / round / lp_draw: leave the pool's seeded state as it is (the defaults), or set it first like run_batch does (seed=None:
        unseeded)."""
        g, stream, dev = handle
        self.L.SetGPUDevice(dev)
        if seed is not False or round is not None or lp_draw is not None:
            cur = self._seed_state.get(dev, (None, 0, 0))
            self._set_seed(dev, cur[0] if seed is False else seed, cur[1] if round is None else round, stream, cur[2] if lp_draw is None else lp_draw)
        if self.L.LegionBatchGraph_Launch(g, stream, int(counter)) != 0:
            check()
            raise RuntimeError("LegionBatchGraph_Launch failed")
        if sync:
            self.L.d_stream_sync(stream)
            check()

    def result(self, dev=0, pipe=0, with_features=True, aggregated=None, normalised=None, edge_ids=None, edge_features=None, lp_exclude=None):
        """lp_exclude: whether the pipe's edge marks are read (`edge_keep` uint8 [n_edges], `lp_excluded` int32[8]) -- None: as run_batch /
        capture_batch on this engine left it.
        edge_features: whether the pipe's gathered edge rows are read (`edge_feat` float32 [n_edges, dim]) -- None: as run_batch /
        capture_batch on this engine left it; True: at the width of the engine's table.
        edge_ids: whether the pipe's edge ids are read (`edge_ids`, and `edge_w` where the batch ran over retained weights) -- None: as
        run_batch / capture_batch on this engine left it.
        aggregated: how to read the pipe's feature buffer -- None: as run_batch / capture_batch on this engine left it; True / False
        for a caller that drove the launchers itself.  normalised: likewise, whether the pipe's block out-degrees are read (`out_deg`)."""
        if aggregated is None:
            aggregated = self._agg.get((dev, pipe), False)
        if normalised is None:
            normalised = self._norm.get((dev, pipe), False)
        o = self.out[dev][pipe]
        self.L.SetGPUDevice(dev)
        nc = o["nc"].to_numpy(np.int32, layout.COUNTER_WORDS)
        ec = o["ec"].to_numpy(np.int32, layout.COUNTER_WORDS)
        H = self.hops
        n_nodes, n_edges = layout.batch_nodes(nc, H), layout.batch_edges(ec, H)
        res = dict(nc=nc, ec=ec, ids=o["ids"].to_numpy(np.int32, n_nodes), labels=o["labels"].to_numpy(np.int32, layout.level_size(nc, 0)),
                   src_off=o["src"].to_numpy(np.int32, n_edges), dst_off=o["dst"].to_numpy(np.int32, n_edges))
        if self._eid.get((dev, pipe), False) if edge_ids is None else edge_ids:
            self.L.GPUMemoryPool_SetCurrentPipe(self.pools[dev], pipe)
            eid, ew = self.L.GPUMemoryPool_GetEdgeIdBuffer(self.pools[dev]), self.L.GPUMemoryPool_GetEdgeWeightBuffer(self.pools[dev])
            check()
            if not eid:
                raise RuntimeError("result(edge_ids=True): the pool has no edge-id buffer (GPUMemoryPool_SetEdgeIds was never on)")
            res["edge_ids"] = read_dev(eid, np.int64, n_edges)
            if ew:
                res["edge_w"] = read_dev(ew, np.float32, n_edges)
        if self._lpx.get((dev, pipe), False) if lp_exclude is None else lp_exclude:
            self.L.GPUMemoryPool_SetCurrentPipe(self.pools[dev], pipe)
            keep, cnt = self.L.GPUMemoryPool_GetEdgeKeepBuffer(self.pools[dev]), self.L.GPUMemoryPool_GetLpExcludedBuffer(self.pools[dev])
            check()
            if not keep or not cnt:
                raise RuntimeError("result(): the pipe's last batch did not run the marking launch (GPUMemoryPool_GetEdgeKeepBuffer is null)")
            res["edge_keep"] = read_dev(keep, np.uint8, n_edges)
            res["lp_excluded"] = read_dev(cnt, np.int32, 8)
        dim = self._efeat.get((dev, pipe), 0) if edge_features is None else (self.edge_feature_dim if edge_features else 0)
        if dim:
            self.L.GPUMemoryPool_SetCurrentPipe(self.pools[dev], pipe)
            ef = self.L.GPUMemoryPool_GetEdgeFeatureBuffer(self.pools[dev])
            check()
            if not ef:
                raise RuntimeError("result(): the pipe's last batch had no edge rows gathered (GPUMemoryPool_GetEdgeFeatureBuffer is null)")
            res["edge_feat"] = read_dev(ef, np.float32, n_edges * dim).reshape(n_edges, dim)
        if with_features and o["feat"] is not None and aggregated:
            # aggregated hand-off: rows [0, n_in) are features, rows [n_in, n_in + N) the last hop's neighbour sums per input slot
            n_in, runs = layout.first_block_dst(nc, H), layout.hop_inputs(nc, ec, H)
            cap = getattr(self, "feature_rows", n_in + runs)
            r_in = min(n_in, cap)
            r_sum = max(0, min(n_in + runs, cap) - n_in)
            buf = o["feat"].to_numpy(np.float32, (r_in + r_sum) * self.F).reshape(r_in + r_sum, self.F)
            res["features"], res["nbr_sum"] = buf[:r_in], buf[r_in:]
            if normalised:
                self.L.GPUMemoryPool_SetCurrentPipe(self.pools[dev], pipe)
                res["out_deg"] = read_dev(self.L.GPUMemoryPool_GetAggOutDeg(self.pools[dev]), np.int32, n_nodes)
        elif with_features and o["feat"] is not None:
            rows = min(n_nodes, getattr(self, "feature_rows", n_nodes))
            res["features"] = o["feat"].to_numpy(np.float32, rows * self.F).reshape(rows, self.F)
        return res

    # ---- cache pipeline (Server::PreSc, Server.cu:83-114) ----------------------------------------------------------
    def build_cache(self, cache_agg_mode=0, counters=None, node_capacity=None, edge_capacity=None, train_step=1):
        L = self.L
        L.GPUCache_CandidateSelection(self.cache, cache_agg_mode, self.noder, self.graph)
        if node_capacity is not None:
            L.GPUCache_SetCapacity(self.cache, int(node_capacity), int(edge_capacity))
        cp = None
        if counters is not None:
            counters = np.ascontiguousarray(counters, dtype=np.uint64)
            cp = counters.ctypes.data
        L.GPUCache_CostModel(self.cache, cache_agg_mode, self.noder, self.graph, cp, int(train_step))
        L.GPUCache_FillUp(self.cache, cache_agg_mode, self.noder, self.graph)
        check()

    # ---- one process per GPU: exchange the clique's cache shards / CSR fragments over HIP IPC -----------------
    def export_shards(self, dev):
        """(feature_chunk_handles, indptr_chunk_handles, indices_chunk_handles, (fragment_rows, fragment_edges), shard geometry) of a
        LOCAL clique member; every handle is a 64-byte HIP IPC handle of one chunk allocation; the geometry -- (pitch, rows per
        chunk, chunks, rows) the shard was built with -- travels with the handles and is checked by the importer."""
        L = self.L
        fh = []
        geom = None
        if L.GPUCache_Float_Feature_Cache(self.cache, dev):
            g4 = (i32 * 4)()
            if L.GPUCache_ShardGeometry(self.cache, dev, g4) == 0:
                geom = tuple(g4)
            for q in range(L.GPUCache_ShardChunkCount(self.cache, dev)):
                b = C.create_string_buffer(64)
                if L.GPUCache_ExportFeatureShardChunk(self.cache, dev, q, b) != 0:
                    break
                fh.append(b.raw)
        th = [[], []]
        rows, edges = L.GPUGraphStorage_FragmentRows(self.graph, dev), L.GPUGraphStorage_FragmentEdges(self.graph, dev)
        if rows > 0:
            for which in (0, 1):
                for q in range(L.GPUGraphStorage_FragmentChunkCount(self.graph, dev, which)):
                    b = C.create_string_buffer(64)
                    if L.GPUGraphStorage_ExportFragmentChunk(self.graph, dev, which, q, b) != 0:
                        break
                    th[which].append(b.raw)
        check()
        have_t = rows > 0 and th[0] and th[1]
        return (fh if fh else None, th[0] if have_t else None, th[1] if have_t else None, (rows, edges), geom)

    def import_shards(self, owner_dev, handles, viewer_devs=None):
        """Open a REMOTE member's shards so that the local members read them in-kernel (xGMI peer loads)."""
        L = self.L
        fh, ih, xh, (rows, edges) = handles[:4]
        geom = handles[4] if len(handles) > 4 else None
        if fh is not None:
            if geom is not None and L.GPUCache_CheckShardGeometry(self.cache, owner_dev, (i32 * 4)(*geom)) != 0:
                check()      # raises: the exporter's pitch / chunk geometry is not what this process derived
            for q, h in enumerate(fh):
                L.GPUCache_ImportFeatureShardChunk(self.cache, owner_dev, q, h)
        if ih is not None:
            for v in (self.local_devs if viewer_devs is None else viewer_devs):
                for which, hs in ((0, ih), (1, xh)):
                    for q, h in enumerate(hs):
                        L.GPUGraphStorage_ImportFragmentChunk(self.graph, owner_dev, v, which, q, h, rows, edges)
        check()

    def close(self):
        L = self.L
        for g in self._graphs:
            L.LegionBatchGraph_Delete(g)
        self._graphs = []
        for d, st in enumerate(self.streams):
            if st is not None:
                L.SetGPUDevice(d)
                L.d_stream_destroy(st)
        self.streams = [None] * self.G
        for g, pool in enumerate(self.pools):
            if pool is None:
                continue
            L.SetGPUDevice(g)
            L.GPUMemoryPool_Delete(pool)
            for pipes in self.out[g]:
                for b in pipes.values():
                    if b is not None:
                        b.free()
        L.GPUCache_Delete(self.cache)
        L.GPUGraphStorage_Delete(self.graph)
        L.GPUNodeStorage_Delete(self.noder)
        for b in self._owned:
            if isinstance(b, tuple):
                L.host_free_space(b[1])
            else:
                b.free()
        self.pools, self.out, self._owned = [], [], []
