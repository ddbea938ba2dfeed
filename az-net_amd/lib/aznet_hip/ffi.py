"""ctypes binding of libaznet_hip.so (include/aznet_hip.h).

This is the only way the Python host code reaches the GPU path, and there is no
fallback: if the shared library is missing or no gfx950 device is visible, the
constructors raise.  NumPy owns every host buffer; torch (when used) owns the
feature map and hands over a raw device pointer.
"""
import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libaznet_hip.so")

AZ_MAX_LEVELS = 16
AZ_NUM_SUBREG = 11
AZ_OK = 0
AZ_BATCH_MAX = 32          # include/aznet_hip.h
AZ_PYRAMID_MAX = 8         # include/aznet_hip.h
AZ_SKIP_MAX_SRC = 3        # include/aznet_hip.h
AZ_SKIP_CHUNK = 128        # include/aznet_hip.h
AZ_TRAIN_FP32, AZ_TRAIN_BF16 = 0, 1       # include/aznet_hip.h
AZ_NMS_HARD, AZ_NMS_LINEAR, AZ_NMS_GAUSSIAN = 0, 1, 2      # include/aznet_hip.h
AZ_SOFT_NMS_MAX = 4096     # include/aznet_hip.h
NMS_METHODS = {"hard": AZ_NMS_HARD, "linear": AZ_NMS_LINEAR, "gaussian": AZ_NMS_GAUSSIAN}
AZ_ERR_INVALID, AZ_ERR_HIP, AZ_ERR_CAPACITY, AZ_ERR_STATE, AZ_ERR_NO_DEVICE = -1, -2, -3, -4, -5
_ERR_NAMES = {-1: "AZ_ERR_INVALID", -2: "AZ_ERR_HIP", -3: "AZ_ERR_CAPACITY", -4: "AZ_ERR_STATE",
              -5: "AZ_ERR_NO_DEVICE"}

# every symbol include/aznet_hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "az_version", "az_create", "az_destroy", "az_last_error", "az_set_limits", "az_load_head",
    "az_set_feature_map_dev", "az_set_feature_map_host", "az_propose", "az_propose_launch",
    "az_propose_fetch", "az_last_candidates", "az_divide_region", "az_sift_dup", "az_roi_dedup",
    "az_roi_pool", "az_head_forward", "az_decode_filter", "az_topk", "az_topk_radix", "az_nms", "az_set_profiling",
    "az_last_kernel_times", "az_stream", "az_load_det_head", "az_det_forward", "az_detect",
    "az_set_gemm_mode", "az_last_anchors", "az_tune_begin", "az_tune_end", "az_tune_kth_largest",
    "az_tune_top", "az_tune_push", "az_bbox_overlaps", "az_recall_match", "az_image_blob_size",
    "az_image_blob_host", "az_image_blob_dev", "az_nms_batched", "az_set_graphs",
    "az_set_feature_map_dev_async", "az_result_record_layout", "az_propose_stage_result_dev",
    "az_propose_launch_on", "az_set_feature_map_dev_nhwc", "az_set_pass_costs", "az_get_pass_costs",
    "az_measure_box", "az_image_blob_dev_on", "az_set_lanes", "az_next_stream", "az_last_stream",
    "az_rccl_unique_id", "az_rccl_init", "az_gather_records", "az_rccl_destroy", "az_comm_stream",
    "az_bias_relu", "az_bias_relu_pool", "az_batch_launch", "az_batch_fetch", "az_batch_next_stream",
    "az_batch_stage_results_dev", "az_batch_fetch_all", "az_batch_launch_shapes", "az_abi_sizes",
    "az_detect_batch", "az_voc_eval", "az_rank_unit", "az_coco_eval", "az_diag_eval",
    "az_set_feature_pyramid_dev_nhwc", "az_roi_dedup_pyramid", "az_roi_pool_pyramid", "az_propose_pyramid",
    "az_detect_pyramid",
    "az_load_skip_front", "az_set_skip_maps_dev_nhwc", "az_detect_skip", "az_det_forward_skip", "az_skip_pool",
    "az_skip_conv",
    "az_zoom_labels", "az_train_ex_rois", "az_train_adj_targets", "az_train_target_stats",
    "az_solver_create", "az_solver_destroy", "az_solver_load", "az_solver_read", "az_solver_set_hyper", "az_solver_step",
    "az_solver_update", "az_sgd_update", "az_solver_forward_test", "az_solver_fetch", "az_solver_gemm_unit",
    "az_det_targets", "az_det_target_stats",
    "az_det_solver_create", "az_det_solver_destroy", "az_det_solver_load", "az_det_solver_read", "az_det_solver_set_hyper",
    "az_det_solver_step", "az_det_solver_update", "az_det_solver_forward_test", "az_det_solver_fetch",
    "az_det_solver_attach_skip", "az_det_solver_load_skip", "az_det_solver_read_skip", "az_det_solver_set_skip_hyper",
    "az_det_solver_step_skip", "az_det_solver_forward_test_skip", "az_skip_pool_bwd_unit",
    "az_solver_set_precision", "az_det_solver_set_precision", "az_solver_gemm_unit_prec",
    "az_solver_set_accumulate", "az_det_solver_set_accumulate", "az_solver_load_history", "az_det_solver_load_history",
    "az_det_solver_load_skip_history",
    "az_det_solver_mine", "az_det_solver_mine_skip",
    "az_soft_nms_batched", "az_box_vote_batched",
    "az_load_det_head_lowrank", "az_lowrank_gemm_unit", "az_lowrank_split",
    "az_load_head_lowrank", "az_az_lowrank_split",
    "az_detect_iter", "az_detect_iter_skip",
    "az_det_diag_eval", "az_coco_diag_eval",
]
AZ_ITER_LOC_MAX_ROUNDS = 8  # include/aznet_hip.h
AZ_ITER_LOC_MAX_ROWS = 4096  # include/aznet_hip.h (az_detect_iter: az_topk's largest k)
AZ_LOWRANK_MAX = 2048      # include/aznet_hip.h


class AzParams(ctypes.Structure):
    _fields_ = [("im_h", ctypes.c_int32), ("im_w", ctypes.c_int32), ("scale", ctypes.c_double),
                ("Tz", ctypes.c_double), ("Tc", ctypes.c_double), ("dedup", ctypes.c_double),
                ("eps", ctypes.c_double), ("min_side", ctypes.c_double),
                ("batch_size", ctypes.c_int32), ("num_proposals", ctypes.c_int32),
                ("fixed_num", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AzStats(ctypes.Structure):
    _fields_ = [("n_proposals", ctypes.c_int32), ("num_eval", ctypes.c_int32),
                ("depth", ctypes.c_int32), ("n_levels", ctypes.c_int32),
                ("n_candidates", ctypes.c_int32),
                ("level_regions", ctypes.c_int32 * AZ_MAX_LEVELS),
                ("level_unique", ctypes.c_int32 * AZ_MAX_LEVELS),
                ("level_zoomed", ctypes.c_int32 * AZ_MAX_LEVELS),
                ("spec_rows", ctypes.c_int32), ("root_deferred", ctypes.c_int32),
                ("static_plan", ctypes.c_int32), ("n_passes", ctypes.c_int32),
                ("pass_rows", ctypes.c_int32 * AZ_MAX_LEVELS),
                ("search_form", ctypes.c_int32), ("n_reruns", ctypes.c_int32),
                ("pass_levels", ctypes.c_int32 * AZ_MAX_LEVELS)]


AZ_TRAIN_MAX_REGIONS = 16    # include/aznet_hip.h


class AzTrainParams(ctypes.Structure):
    _fields_ = [("min_side", ctypes.c_double), ("zoom_err_prob", ctypes.c_double), ("emb_obj_thresh", ctypes.c_double),
                ("emb_reg_thresh", ctypes.c_double), ("adj_thresh", ctypes.c_double), ("eps", ctypes.c_double),
                ("train_rep", ctypes.c_int32), ("n_addregions", ctypes.c_int32), ("n_subregion", ctypes.c_int32),
                ("reserved", ctypes.c_int32),
                ("addregions", (ctypes.c_double * 4) * AZ_TRAIN_MAX_REGIONS),
                ("subregion", (ctypes.c_double * 4) * AZ_TRAIN_MAX_REGIONS)]


def make_train_params(tp):
    """az_train_params from a dict (az_data_layer.roidb.train_params) or an AzTrainParams."""
    if isinstance(tp, AzTrainParams):
        return tp
    p = AzTrainParams()
    for k in ("min_side", "zoom_err_prob", "emb_obj_thresh", "emb_reg_thresh", "adj_thresh", "eps"):
        setattr(p, k, float(tp[k]))
    p.train_rep = int(tp["train_rep"])
    for name, cnt in (("addregions", "n_addregions"), ("subregion", "n_subregion")):
        rows = tp[name]
        if not 1 <= len(rows) <= AZ_TRAIN_MAX_REGIONS:
            raise AzError(AZ_ERR_INVALID, "%s: 1..%d rows" % (name, AZ_TRAIN_MAX_REGIONS))
        setattr(p, cnt, len(rows))
        for i, r in enumerate(rows):
            for q in range(4):
                getattr(p, name)[i][q] = float(r[q])
    return p


SEARCH_FORMS = {0: "level_loop", 1: "pair_speculation", 2: "whole_tree_pass", 3: "closure_pass", 4: "one_pass_plan",
                5: "batch_level_loop"}


class AzError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "%s (%d): %s" % (_ERR_NAMES.get(code, "AZ_ERR"), code, msg))
        self.code = code


_lib = None


def load_library(path=None):
    """Load libaznet_hip.so and declare prototypes.  Fails loudly when it is absent:
    build it with `python -c 'import __graft_entry__ as g; g.build()'` or
    `make -C az-net_amd/csrc`."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("AZNET_HIP_LIB") or LIB_PATH      # (AZNET_HIP_LIB: an A/B build of the library, measurements)
    if not os.path.exists(p):
        raise ImportError("libaznet_hip.so not found at %s -- the HIP extension is required "
                          "(no CPU fallback); run make -C az-net_amd/csrc" % p)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 and must be the
    # first to load it -- if this library pulls in /opt/rocm's copy first, torch later finds
    # "No HIP GPUs".  The host side uses torch for device memory / streams anyway.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = ctypes.CDLL(p)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    ip, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    cip = ctypes.POINTER(ctypes.c_int)
    L.az_version.restype = ctypes.c_char_p
    L.az_version.argtypes = []
    L.az_create.argtypes = [ci, ctypes.POINTER(vp)]
    L.az_destroy.argtypes = [vp]
    L.az_last_error.restype = ctypes.c_char_p
    L.az_last_error.argtypes = [vp]
    L.az_set_limits.argtypes = [vp, ci, ci]
    L.az_set_gemm_mode.argtypes = [vp, ci]
    L.az_load_head.argtypes = [vp, ci, ci, ci, ci] + [fp] * 12
    L.az_set_feature_map_dev.argtypes = [vp, vp, ci, ci, ci]
    L.az_set_feature_map_host.argtypes = [vp, fp, ci, ci, ci]
    L.az_set_feature_map_dev_async.argtypes = [vp, vp, ci, ci, ci]
    szp = ctypes.POINTER(ctypes.c_size_t)
    L.az_result_record_layout.argtypes = [ci, szp, szp, szp, szp]
    L.az_propose_stage_result_dev.argtypes = [vp, vp, ctypes.c_size_t]
    L.az_propose.argtypes = [vp, ctypes.POINTER(AzParams), dp, fp, ci, cip, ctypes.POINTER(AzStats)]
    L.az_propose_launch.argtypes = [vp, ctypes.POINTER(AzParams)]
    L.az_propose_launch_on.argtypes = [vp, ctypes.POINTER(AzParams), vp, ci, ci, ci, ci]
    L.az_set_feature_map_dev_nhwc.argtypes = [vp, vp, ci, ci, ci]
    L.az_propose_fetch.argtypes = [vp, dp, fp, ci, cip, ctypes.POINTER(AzStats)]
    L.az_last_candidates.argtypes = [vp, dp, fp, ci, cip]
    L.az_divide_region.argtypes = [vp, dp, ci, cd, dp, ci, cip]
    L.az_sift_dup.argtypes = [vp, dp, ci, cd, dp, ci, cip]
    L.az_roi_dedup.argtypes = [vp, dp, ci, cd, cd, ci, fp, ip, ip, cip]
    L.az_roi_pool.argtypes = [vp, fp, ci, fp]
    L.az_head_forward.argtypes = [vp, fp, ci, fp, fp, fp]
    L.az_decode_filter.argtypes = [vp, dp, fp, fp, ci, ci, ci, cd, cd, dp, fp, ci, cip]
    L.az_topk.argtypes = [vp, fp, ci, ci, ip, cip]
    L.az_topk_radix.argtypes = [vp, fp, ci, ci, ip, cip]
    L.az_nms.argtypes = [vp, fp, ci, cd, i64p, cip]
    L.az_nms_batched.argtypes = [vp, fp, ip, ci, cd, i64p, ip]
    L.az_soft_nms_batched.argtypes = [vp, fp, ip, ci, ci, cd, cd, cd, i64p, fp, ip]
    L.az_box_vote_batched.argtypes = [vp, fp, ip, ci, i64p, ip, cd, fp]
    L.az_load_det_head.argtypes = [vp, ci, ci, ci, ci] + [fp] * 8
    L.az_load_det_head_lowrank.argtypes = [vp, ci, ci, ci, ci, ci, ci] + [fp] * 10
    L.az_lowrank_gemm_unit.argtypes = [vp, fp, fp, fp, ci, ci, ci, ci, fp]
    L.az_lowrank_split.argtypes = [ci, ci]
    L.az_load_head_lowrank.argtypes = [vp, ci, ci, ci, ci, ci] + [fp] * 13
    L.az_az_lowrank_split.argtypes = [ci, ci]
    L.az_det_forward.argtypes = [vp, fp, ci, fp, fp]
    L.az_detect.argtypes = [vp, dp, ci, cd, cd, ci, ci, ci, cd, fp, dp]
    L.az_set_feature_pyramid_dev_nhwc.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), ci, ci, ci, ci]
    L.az_roi_dedup_pyramid.argtypes = [vp, dp, ci, dp, ci, cd, ci, fp, ip, ip, cip]
    L.az_roi_pool_pyramid.argtypes = [vp, fp, ci, fp]
    L.az_propose_pyramid.argtypes = [vp, ctypes.POINTER(AzParams), dp, ci, dp, fp, ci, cip, ctypes.POINTER(AzStats)]
    L.az_detect_pyramid.argtypes = [vp, dp, ci, dp, ci, cd, ci, ci, ci, cd, fp, dp]
    L.az_load_skip_front.argtypes = [vp, ci, cip, fp, cd, cd, ci, fp, fp]
    L.az_set_skip_maps_dev_nhwc.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_void_p), cip, cip, cip]
    L.az_detect_skip.argtypes = [vp, dp, ci, cd, cd, ci, ci, ci, cd, fp, dp]
    L.az_detect_iter.argtypes = [vp, dp, ci, cd, cd, ci, ci, ci, cd, ci, cd, ci, fp, dp, ip, ip, fp, dp, ip]
    L.az_detect_iter_skip.argtypes = L.az_detect_iter.argtypes
    L.az_det_forward_skip.argtypes = [vp, fp, ci, fp, fp]
    L.az_skip_pool.argtypes = [vp, fp, ci, ci, fp]
    L.az_skip_conv.argtypes = [vp, fp, ci, fp]
    L.az_detect_batch.argtypes = [vp, ci, ctypes.POINTER(vp), ci, ip, ip, dp, ip, dp, ip, cd, ci, cd, fp, dp]
    L.az_set_profiling.argtypes = [vp, ci]
    L.az_set_graphs.argtypes = [vp, ci]
    L.az_last_kernel_times.argtypes = [vp, ctypes.c_char_p, fp, ip, ci, cip]
    L.az_stream.restype = vp
    L.az_stream.argtypes = [vp]
    L.az_set_pass_costs.argtypes = [vp, ci, ip, dp]
    L.az_get_pass_costs.argtypes = [vp, ip, dp, ci, cip]
    L.az_measure_box.argtypes = [vp, dp, dp]
    L.az_set_lanes.argtypes = [vp, ci]
    L.az_rccl_unique_id.argtypes = [vp, ctypes.c_size_t]
    L.az_rccl_init.argtypes = [vp, vp, ctypes.c_size_t, ci, ci]
    L.az_gather_records.argtypes = [vp, vp, vp, ctypes.c_size_t]
    L.az_rccl_destroy.argtypes = [vp]
    L.az_comm_stream.restype = vp
    L.az_comm_stream.argtypes = [vp]
    L.az_next_stream.restype = vp
    L.az_next_stream.argtypes = [vp]
    L.az_last_stream.restype = vp
    L.az_last_stream.argtypes = [vp]
    L.az_batch_next_stream.restype = vp
    L.az_batch_next_stream.argtypes = [vp]
    L.az_batch_launch.argtypes = [vp, ci, ctypes.POINTER(AzParams), ctypes.POINTER(vp), ci, ci, ci]
    L.az_batch_fetch.argtypes = [vp, ci, dp, fp, ci, cip, ctypes.POINTER(AzStats)]
    L.az_batch_launch_shapes.argtypes = [vp, ci, ctypes.POINTER(AzParams), ctypes.POINTER(vp), ci, cip, cip]
    L.az_batch_stage_results_dev.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t]
    L.az_batch_fetch_all.argtypes = [vp, dp, fp, ci, cip, ctypes.POINTER(AzStats)]
    ll, llp = ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    L.az_last_anchors.argtypes = [vp, dp, fp, ci, cip]
    L.az_tune_begin.argtypes = [vp, ll]
    L.az_tune_end.argtypes = [vp]
    L.az_tune_kth_largest.argtypes = [vp, ll, fp, llp]
    L.az_tune_top.argtypes = [vp, ll, fp, ll, llp]
    L.az_tune_push.argtypes = [vp, fp, ll]
    L.az_bbox_overlaps.argtypes = [vp, dp, ci, dp, ci, dp]
    L.az_recall_match.argtypes = [vp, ci, dp, ip, dp, ip, dp]
    L.az_voc_eval.argtypes = [vp, ci, ci, dp, dp, ip, dp, u8p, ip, cd, ci, ctypes.POINTER(ctypes.c_int8), dp, dp,
                              ctypes.POINTER(ctypes.c_int64), dp, dp]
    L.az_rank_unit.argtypes = [vp, ci, ci, dp, ip, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.az_coco_eval.argtypes = [vp, ci, ci, dp, dp, ip, dp, dp, u8p, ip, dp, dp, dp, ip, ctypes.POINTER(ctypes.c_int8)]
    tpp = ctypes.POINTER(AzTrainParams)
    L.az_diag_eval.argtypes = [vp, ci, dp, fp, ip, ip, ctypes.c_longlong, dp, ip, ctypes.c_longlong, dp, ip,
                               ctypes.c_longlong, cd, cd, cd, cd, ip, ci, dp, u8p, ctypes.POINTER(ctypes.c_int64), dp, ip, ip,
                               ip, ctypes.POINTER(ctypes.c_int64), fp]
    i64p = ctypes.POINTER(ctypes.c_int64)
    L.az_det_diag_eval.argtypes = [vp, ci, ci, dp, dp, ip, dp, u8p, ip, cd, cd, ci, ip, dp, ci, ctypes.POINTER(ctypes.c_int8),
                                   dp, ip, dp, ip, u8p, ip, i64p, i64p, i64p, i64p, dp, fp]
    L.az_coco_diag_eval.argtypes = [vp, ci, ci, dp, dp, ip, dp, dp, u8p, ip, cd, ip, dp, ip, dp, ip, ctypes.POINTER(ctypes.c_int8),
                                    u8p, ip, i64p, i64p, i64p, dp, dp, fp]
    L.az_zoom_labels.argtypes = [vp, dp, ci, dp, ci, cd, cd, u8p]
    L.az_train_ex_rois.argtypes = [vp, tpp, ci, ip, dp, ip, dp, ll, fp, u8p, ip, ci, llp, llp]
    L.az_train_adj_targets.argtypes = [vp, tpp, ci, fp, ip, fp, ip, dp, ip, ci]
    L.az_train_target_stats.argtypes = [vp, ci, cd, dp, ll, dp, dp, ci]
    u64 = ctypes.c_uint64
    L.az_solver_create.argtypes = [vp, ci, ci, ci, ci, ci, u64, ctypes.POINTER(vp)]
    L.az_solver_destroy.argtypes = [vp]
    L.az_solver_load.argtypes = [vp] + [fp] * 12
    L.az_solver_read.argtypes = [vp] + [fp] * 12
    L.az_solver_set_hyper.argtypes = [vp, fp, fp, fp]
    L.az_solver_step.argtypes = [vp, vp, ci, ci, ci, ci, fp, ci, fp, fp, fp, fp, u64, ll, fp, dp, vp]
    L.az_solver_update.argtypes = [vp, cd, cd, cd, cd]
    L.az_sgd_update.argtypes = [vp, vp, vp, vp, ll, cd, cd, cd, cd]
    L.az_solver_forward_test.argtypes = [vp, vp, ci, ci, ci, ci, fp, ci, fp, fp, fp]
    L.az_solver_fetch.argtypes = [vp, ctypes.c_char_p, vp, ll, llp]
    L.az_solver_gemm_unit.argtypes = [vp, ci, fp, fp, fp, ci, ci, ci]
    L.az_solver_gemm_unit_prec.argtypes = [vp, ci, ci, fp, fp, fp, ci, ci, ci]
    L.az_solver_set_precision.argtypes = [vp, ci]
    L.az_det_solver_set_precision.argtypes = [vp, ci]
    L.az_solver_set_accumulate.argtypes = [vp, ci]
    L.az_det_solver_set_accumulate.argtypes = [vp, ci]
    L.az_solver_load_history.argtypes = [vp] + [fp] * 12
    L.az_det_solver_load_history.argtypes = [vp] + [fp] * 8
    L.az_det_solver_load_skip_history.argtypes = [vp, fp, fp]
    L.az_det_targets.argtypes = [vp, ci, fp, ip, fp, ip, ip, cd, cd, cd, fp, dp]
    L.az_det_target_stats.argtypes = [vp, ci, fp, ip, ci, cd, ci, dp, dp, dp]
    L.az_det_solver_create.argtypes = [vp, ci, ci, ci, ci, ci, u64, ctypes.POINTER(vp)]
    L.az_det_solver_destroy.argtypes = [vp]
    L.az_det_solver_load.argtypes = [vp] + [fp] * 8
    L.az_det_solver_read.argtypes = [vp] + [fp] * 8
    L.az_det_solver_set_hyper.argtypes = [vp, fp, fp, fp]
    L.az_det_solver_step.argtypes = [vp, vp, ci, ci, ci, ci, fp, ci, fp, fp, fp, u64, ll, fp, dp, vp]
    L.az_det_solver_update.argtypes = [vp, cd, cd, cd, cd]
    L.az_det_solver_forward_test.argtypes = [vp, vp, ci, ci, ci, ci, fp, ci, fp, fp]
    L.az_det_solver_fetch.argtypes = [vp, ctypes.c_char_p, vp, ll, llp]
    vpp = ctypes.POINTER(vp)
    L.az_det_solver_attach_skip.argtypes = [vp, ci, cip, fp, cd, cd, u64]
    L.az_det_solver_load_skip.argtypes = [vp, fp, fp]
    L.az_det_solver_read_skip.argtypes = [vp, fp, fp]
    L.az_det_solver_set_skip_hyper.argtypes = [vp, fp, fp]
    L.az_det_solver_step_skip.argtypes = [vp, ci, cip, vpp, cip, cip, ci, ci, fp, ci, fp, fp, fp, u64, ll, fp, dp, vpp]
    L.az_det_solver_forward_test_skip.argtypes = [vp, ci, cip, vpp, cip, cip, ci, ci, fp, ci, fp, fp]
    L.az_skip_pool_bwd_unit.argtypes = [vp, ci, cip, fp, vpp, cip, cip, ci, ci, fp, ci, fp, fp, ip, vpp]
    L.az_det_solver_mine.argtypes = [vp, vp, ci, ci, ci, ci, fp, ci, fp, fp, cd, ci, ip, ip, fp]
    L.az_det_solver_mine_skip.argtypes = [vp, ci, cip, vpp, cip, cip, ci, ci, fp, ci, fp, fp, cd, ci, ip, ip, fp]
    L.az_image_blob_size.argtypes = [ci, ci, cd, cip, cip]
    L.az_image_blob_host.argtypes = [vp, u8p, ci, ci, fp, cd, fp, ci, ci]
    L.az_image_blob_dev.argtypes = [vp, u8p, ci, ci, fp, cd, vp, ci, ci]
    L.az_image_blob_dev_on.argtypes = [vp, u8p, ci, ci, fp, cd, vp, ci, ci, vp]
    L.az_bias_relu.argtypes = [vp, vp, vp, ci, ctypes.c_longlong, ci]
    L.az_bias_relu_pool.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci]
    for name in SYMBOLS:
        if name not in ("az_version", "az_last_error", "az_stream", "az_next_stream", "az_last_stream", "az_comm_stream",
                        "az_batch_next_stream"):
            getattr(L, name).restype = ci
    # the structs this module hands across the boundary have the library's layout (every fetch clears sizeof(az_stats) bytes
    # of the caller's block: a binding built for another header must not get that far)
    L.az_abi_sizes.argtypes = []
    sizes = int(L.az_abi_sizes())
    if (sizes & 0xffff, (sizes >> 16) & 0xffff) != (ctypes.sizeof(AzParams), ctypes.sizeof(AzStats)):
        raise AzError(AZ_ERR_INVALID, "libaznet_hip.so %s has sizeof(az_params, az_stats) = (%d, %d), this binding (%d, %d): "
                      "rebuild az-net_amd/csrc" % (L.az_version().decode(), sizes & 0xffff, (sizes >> 16) & 0xffff,
                                                  ctypes.sizeof(AzParams), ctypes.sizeof(AzStats)))
    if path is None:
        _lib = L
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _scales(scales):
    """The scales of an image pyramid as the ABI takes them: contiguous f64."""
    return _f64(np.asarray(scales, dtype=np.float64).reshape(-1))


def _p(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def is_lowrank_head(head):
    """A detection-head dict that carries truncated-SVD factors (L6 / U6 and / or L7 / U7)."""
    return isinstance(head, dict) and any(k in head for k in ("L6", "U6", "L7", "U7"))


def lowrank_split(K, r):
    """az_lowrank_split: the number of K chunks of an L stage [., K] x [K, r] -- host arithmetic, no GPU needed."""
    n = int(load_library().az_lowrank_split(int(K), int(r)))
    if n < 1:
        raise AzError(n, "az_lowrank_split(%d, %d)" % (K, r))
    return n


def az_lowrank_split(K, r):
    """az_az_lowrank_split: the number of K chunks of the AZ head's L stage [., K] x [K, r] -- host arithmetic, no GPU
    needed."""
    n = int(load_library().az_az_lowrank_split(int(K), int(r)))
    if n < 1:
        raise AzError(n, "az_az_lowrank_split(%d, %d)" % (K, r))
    return n


def coco_diag_means(prec_fix):
    """What coco_diag_eval adds to az_coco_diag_eval's curves prec_fix [8,10,101,K] on the host: ap_fix [K,10,8], the mean
    over recThrs of the entries > -1 (NaN where none), and stats_fix [8,3], AP / AP50 / AP75 per variant by COCOeval
    summarize's expression np.mean(s[s > -1]) over s [T,R,K] (-1 where none)."""
    p = np.ascontiguousarray(prec_fix, np.float64)
    K = p.shape[3]
    q = np.ascontiguousarray(p.transpose(3, 1, 0, 2))    # [K,10,8,101]: a curve is all -1 or has no -1, but for a caller's own array
    ok = q > -1
    every, some = ok.all(-1), ok.any(-1)
    with np.errstate(invalid="ignore"):
        ap = np.where(every, q.mean(-1), np.nan) if K else np.zeros((0, 10, 8))
    for k, t, v in zip(*np.nonzero(some & ~every)):
        ap[k, t, v] = np.mean(q[k, t, v][ok[k, t, v]])
    stats = np.zeros((8, 3))
    for v in range(8):
        for j, s in enumerate((p[v], p[v, 0:1], p[v, 5:6])):
            stats[v, j] = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    return {"ap_fix": ap, "stats_fix": stats}


class AzContext(object):
    """One GPU's search context (az_ctx).  Not thread-safe; one per process/GPU."""

    def __init__(self, device=0, max_regions=None, max_candidates=None, gemm_mode=None):
        """gemm_mode: 0 fp32 MFMA (default); 2 = int6 on the 16-bit matrix cores with fp32 operands as two
        fp16 terms (3 MFMAs per product, ~2^-21); 3 = as three bf16 terms (6 MFMAs, all 24 mantissa bits)
        (az_set_gemm_mode); None reads the AZ_GEMM_MODE environment variable (default 0)."""
        self.L = load_library()
        h = ctypes.c_void_p()
        rc = self.L.az_create(int(device), ctypes.byref(h))
        if rc != AZ_OK:
            raise AzError(rc, "az_create(device=%d) failed: a gfx950 GPU is required, there is no "
                              "CPU fallback" % device)
        self.h = h
        self.device = int(device)
        self.dims = None
        self.skip_dims = None          # the loaded skip front's sizes (load_skip_front)
        self.feat_shape = None
        self._feat_keepalive = None
        if max_regions is not None:
            self._chk(self.L.az_set_limits(self.h, int(max_regions),
                                           int(max_candidates or max_regions * AZ_NUM_SUBREG)))
        if gemm_mode is None:
            gemm_mode = int(os.environ.get("AZ_GEMM_MODE", "0"))
        if int(gemm_mode) not in (0, 2, 3):
            self.close()
            raise ValueError("gemm_mode must be 0 (fp32 MFMA), 2 (two fp16 terms) or 3 (three bf16 terms), got %r" % (gemm_mode,))
        self.gemm_mode = int(gemm_mode)
        if self.gemm_mode:
            self._chk(self.L.az_set_gemm_mode(self.h, self.gemm_mode))
        self.max_regions = max_regions or 16384
        self.max_candidates = max_candidates or self.max_regions * AZ_NUM_SUBREG

    def _chk(self, rc):
        if rc != AZ_OK:
            raise AzError(rc, self.L.az_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.az_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup --------------------------------------------------------------------
    def load_head(self, head):
        """head: dict of Caffe-layout fp32 arrays W6,b6,W71,b71,W72,b72,Was,bas,Wab,bab,Wz,bz.  A head that carries
        truncated-SVD factors of int6 (L6 / U6: compress.compress_az_head, caffemodel.az_head_from_layers of a compressed
        file) goes through load_head_lowrank."""
        if isinstance(head, dict) and ("L6" in head or "U6" in head):
            return self.load_head_lowrank(head)
        W6 = _f32(head["W6"])
        n6, K6 = W6.shape
        assert K6 % 49 == 0
        C = K6 // 49
        n71, n72 = head["W71"].shape[0], head["W72"].shape[0]
        assert head["W71"].shape == (n71, n6) and head["W72"].shape == (n72, n6)
        assert head["Was"].shape == (11, n71) and head["Wab"].shape == (44, n71)
        assert head["Wz"].shape == (1, n72)
        arrs = [W6] + [_f32(head[k]) for k in ("b6", "W71", "b71", "W72", "b72", "Was", "bas", "Wab",
                                                 "bab", "Wz", "bz")]
        self._chk(self.L.az_load_head(self.h, C, n6, n71, n72, *[_p(a, ctypes.c_float) for a in arrs]))
        self.dims = dict(C=C, n6=n6, n71=n71, n72=n72, K6=K6)

    def load_head_lowrank(self, head):
        """az_load_head_lowrank.  head: as load_head's, with int6 given as L6 [r6, C*49], U6 [n6, r6], b6 instead of W6, b6."""
        if "L6" not in head or "U6" not in head:
            raise ValueError("a low-rank AZ head needs both L6 and U6")
        if "W6" in head:
            raise ValueError("a low-rank AZ head carries L6 and U6 in W6's place, not beside it")
        L6, U6 = _f32(head["L6"]), _f32(head["U6"])
        if L6.ndim != 2 or U6.ndim != 2 or U6.shape[1] != L6.shape[0]:
            raise ValueError("L6 %s and U6 %s do not chain" % (L6.shape, U6.shape))
        (r6, K6), n6 = L6.shape, U6.shape[0]
        assert K6 % 49 == 0
        C = K6 // 49
        n71, n72 = head["W71"].shape[0], head["W72"].shape[0]
        assert head["W71"].shape == (n71, n6) and head["W72"].shape == (n72, n6)
        assert head["Was"].shape == (11, n71) and head["Wab"].shape == (44, n71)
        assert head["Wz"].shape == (1, n72)
        arrs = [L6, U6] + [_f32(head[k]) for k in ("b6", "W71", "b71", "W72", "b72", "Was", "bas", "Wab",
                                                     "bab", "Wz", "bz")]
        assert arrs[2].size == n6
        self._chk(self.L.az_load_head_lowrank(self.h, C, n6, n71, n72, r6, *[_p(a, ctypes.c_float) for a in arrs]))
        self.dims = dict(C=C, n6=n6, n71=n71, n72=n72, K6=K6, r6=r6)

    def set_feature_map(self, fmap, wait=True, producer_done=False):
        """fmap: [1,C,H,W] or [C,H,W]; a NumPy array (copied to HBM) or a CUDA torch tensor
        (borrowed: its data_ptr is handed to the library, the tensor is kept alive here).
        The ctx stream is not torch's: torch's current stream is synchronised first, so a map the
        backbone is still writing is never read early.  wait=False (torch tensors only) skips the
        closing synchronisation of the ctx stream (az_set_feature_map_dev_async): the tensor then
        has to stay untouched until the next propose/propose_fetch returns.  producer_done=True (torch tensors): the caller
        knows the map is complete (e.g. a search that read it has been fetched): torch's stream is not synchronised."""
        if isinstance(fmap, np.ndarray):
            a = _f32(fmap)
            if a.ndim == 4:
                assert a.shape[0] == 1
                a = a[0]
            C, H, W = a.shape
            self._chk(self.L.az_set_feature_map_host(self.h, _p(a, ctypes.c_float), C, H, W))
            self._feat_keepalive = None
        else:   # torch tensor on this device
            t, cl = self._torch_map(fmap)
            C, H, W = (int(x) for x in t.shape)
            import torch
            if not producer_done:
                torch.cuda.current_stream(t.device).synchronize()     # producer (backbone) done
            fn = self.L.az_set_feature_map_dev_nhwc if cl else (
                self.L.az_set_feature_map_dev if wait else self.L.az_set_feature_map_dev_async)
            self._chk(fn(self.h, ctypes.c_void_p(t.data_ptr()), C, H, W))
            self._feat_keepalive = fmap
        self.feat_shape = (C, H, W)

    def _torch_map(self, fmap):
        """(tensor [C,H,W] view, channels_last?) of a CUDA conv5_3 tensor: NCHW-contiguous maps are transposed into
        ctx memory by the library, torch.channels_last ones ([1,C,H,W] stored [H][W][C]) are borrowed as they are."""
        import torch
        t = fmap
        assert t.is_cuda and str(t.dtype) == "torch.float32" and t.device.index == self.device, \
            "feature map must be a float32 CUDA tensor on this context's GPU"
        if t.dim() == 4:
            assert t.shape[0] == 1
            if t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous():
                return t[0], True
            t = t[0]
        assert t.is_contiguous()
        return t, False

    # ---- hot path -----------------------------------------------------------------
    @staticmethod
    def make_params(im_h, im_w, scale, Tz, num_proposals=300, fixed_num=True, Tc=0.05,
                    dedup=1. / 16., eps=1e-14, min_side=10, batch_size=10000, speculate=True, fused=True,
                    tune=False, radix_select=False, fused_levels=True, static_tree=True, pair_spec=None, full_spec=None,
                    early_end=True):
        """speculate=False evaluates levels 1-3 one by one instead of in one pass (same bits,
        slower); fused=False keeps the geometry of those levels as separate launches;
        fused_levels=False does the same for the levels after them (az_level.hip).  All
        exist for tests and measurements.  tune=True selects the tuner's variant of the search
        (lib/detect/tune.py:256-316) and keeps the anchor history (last_anchors).  radix_select=True
        does the final top-k with the single-workgroup radix select (same result, for tests).
        static_tree=False: with Tz <= 0 (every zoom test passes, the tree depends on the image shape only) still
        walk the tree level by level instead of forwarding all levels' rois in one head pass (same bits).
        pair_spec: None = let the context decide from its previous search whether a level's head pass also carries the
        rows of ALL children of its regions (so that the next level needs no pass); False = never; True = at every
        eligible level (same bits in all three).
        full_spec: None = let the context decide from its previous search of this image shape whether the search's ONE
        head pass evaluates the rows of the shape's full tree, every level finding its outputs by RoIPool window (pays
        for dense trees: after a full tree the full tree's rows, otherwise the closure rows); False = never; True = the
        full tree's rows whenever the shape allows; "closure" = the closure rows whenever the shape allows -- every region
        any pruning of the tree can produce, so no Tz can miss a window (same bits in all four).
        early_end=False: enqueue every level even when the context's previous search of the shape ended early (by default
        such a search is enqueued only up to the level where that one ended, and run again in full if this tree goes on;
        same bits)."""
        return AzParams(int(im_h), int(im_w), float(scale), float(Tz), float(Tc), float(dedup),
                        float(eps), float(min_side), int(batch_size), int(num_proposals),
                        1 if fixed_num else 0,
                        (0 if speculate else 1) | (0 if fused else 2) | (4 if tune else 0) |
                        (8 if radix_select else 0) | (0 if fused_levels else 16) | (0 if static_tree else 32) |
                        (0 if pair_spec is None else (128 if pair_spec else 64)) |
                        (0 if full_spec is None else ((512 | 1024) if full_spec == "closure" else (512 if full_spec else 256))) |
                        (0 if early_end else 4096))

    def _search_result(self, call, cap, want_scores, want_stats):
        """One search's result: call(boxes, scores, cap, n, stats) fills the buffers allocated here (ctypes arguments);
        returns boxes [n,4] f64, with scores [n] f32 and / or the AzStats when asked."""
        boxes = np.empty((max(cap, 1), 4), dtype=np.float64)
        scores = np.empty((max(cap, 1),), dtype=np.float32)
        n = ctypes.c_int(0)
        st = AzStats()
        self._chk(call(_p(boxes, ctypes.c_double), _p(scores, ctypes.c_float), cap, ctypes.byref(n), ctypes.byref(st)))
        out = [boxes[:n.value].copy()]
        if want_scores:
            out.append(scores[:n.value].copy())
        if want_stats:
            out.append(st)
        return out[0] if len(out) == 1 else tuple(out)

    def propose(self, params, want_scores=False, want_stats=False):
        cap = params.num_proposals if params.fixed_num else self.max_candidates
        return self._search_result(lambda *out: self.L.az_propose(self.h, ctypes.byref(params), *out), cap, want_scores,
                                   want_stats)

    # ---- multi-scale test pyramids (cfg.TEST.SCALES with several entries) --------------------------------------------
    def set_feature_pyramid(self, maps, producer_done=False):
        """maps: the S conv5_3 maps of one padded image blob (_get_image_blob of a pyramid), CUDA float32 tensors
        [1,C,H,W] in torch.channels_last memory (or [H][W][C] views), all of one size; borrowed (kept alive here) as
        set_feature_map borrows a channel-last map.  Level 0 also becomes the context's single map."""
        import torch
        maps = list(maps)
        if not 1 <= len(maps) <= AZ_PYRAMID_MAX:
            raise ValueError("a pyramid has 1 to %d levels, got %d" % (AZ_PYRAMID_MAX, len(maps)))
        views = []
        for m in maps:
            t, cl = self._torch_map(m)
            if not cl:
                raise ValueError("pyramid maps must be channels_last CUDA tensors (the layout RoIPool reads)")
            views.append(t)
        shapes = {tuple(int(x) for x in t.shape) for t in views}
        if len(shapes) != 1:
            raise ValueError("the maps of a pyramid must all have one (padded) size, got %s" % sorted(shapes))
        C, H, W = shapes.pop()
        if not producer_done:
            torch.cuda.current_stream(views[0].device).synchronize()
        tab = (ctypes.c_void_p * len(views))(*[t.data_ptr() for t in views])
        self._chk(self.L.az_set_feature_pyramid_dev_nhwc(self.h, tab, len(views), C, H, W))
        self._feat_keepalive = maps
        self.feat_shape = (C, H, W)
        self.pyramid_levels = len(views)

    def roi_dedup_pyramid(self, boxes, scales, dedup=1. / 16., batch_size=10000):
        """_get_rois_blob over a pyramid + np.unique per batch_size chunk: (rois [P,5] f32 with the level in column 0,
        index [U], inverse [P])."""
        sc = _scales(scales)
        return self._roi_dedup(self.L.az_roi_dedup_pyramid, (_p(sc, ctypes.c_double), sc.size), boxes, dedup, batch_size)

    def roi_pool_pyramid(self, rois):
        return self._roi_pool(self.L.az_roi_pool_pyramid, rois)

    def propose_pyramid(self, params, scales, want_scores=False, want_stats=False):
        """propose() over the pyramid set (az_propose_pyramid: the plain level loop); params.scale is ignored."""
        sc = _scales(scales)
        cap = params.num_proposals if params.fixed_num else self.max_candidates
        return self._search_result(
            lambda *out: self.L.az_propose_pyramid(self.h, ctypes.byref(params), _p(sc, ctypes.c_double), sc.size, *out),
            cap, want_scores, want_stats)

    def detect_pyramid(self, boxes, scales, im_h, im_w, dedup=1. / 16., batch_size=10000, eps=1e-14):
        """detect() over the pyramid set (az_detect_pyramid)."""
        sc = _scales(scales)
        return self._detect(self.L.az_detect_pyramid, (_p(sc, ctypes.c_double), sc.size), boxes, im_h, im_w, dedup,
                            batch_size, eps)

    def _ext(self, handle):
        """torch view of one of the context's HIP streams (by raw handle)."""
        import torch
        cache = self.__dict__.setdefault("_ext_streams", {})
        s = cache.get(int(handle))
        if s is None:
            s = cache[int(handle)] = torch.cuda.ExternalStream(int(handle), device=torch.device("cuda", self.device))
        return s

    def wait_event(self, event, params=None):
        """Make the stream the NEXT launched search runs on wait (on the device, no host synchronisation) for a
        torch.cuda.Event -- e.g. the one recorded behind the backbone's last kernel on torch's stream.  params: the
        parameters that search will be launched with -- searches that cannot be queued (a data-dependent proposal count, the
        tuner's variant) always run on the context's first lane, whatever lane is next in turn (az_capi.hip: next_lane)."""
        first_lane = params is not None and (not params.fixed_num or (params.reserved & 4))
        h = self.L.az_stream(self.h) if first_lane else self.L.az_next_stream(self.h)
        self._ext(h).wait_event(event)

    def set_lanes(self, lanes):
        """2: queued searches take turns between two streams of this context, so consecutive images overlap on the GPU
        (az_set_lanes); 1: one stream (the default)."""
        self._chk(self.L.az_set_lanes(self.h, int(lanes)))
        self.lanes = int(lanes)

    def record_event(self):
        """A torch.cuda.Event recorded now on the stream of the search launched last: behind that search."""
        return self._ext(self.L.az_last_stream(self.h)).record_event()

    def propose_launch(self, params, fmap=None, producer_done=False, producer_event=None):
        """fmap (a CUDA torch tensor [1,C,H,W] / [C,H,W] on this GPU): hand the image's map over in the same call
        (az_propose_launch_on); it must stay untouched until propose_fetch returns.  producer_done=True skips the
        synchronisation of torch's current stream (the caller knows the map is complete); producer_event (a
        torch.cuda.Event recorded behind the map's producer) orders the search behind it ON THE DEVICE instead, so the
        host can go on and enqueue the next image's backbone while this search runs.
        Up to three searches per lane may be launched before the first is fetched (fixed proposal count): the host then enqueues
        the next image's launch sequence while the GPU still works on the current one -- same stream, the searches do not
        overlap on the GPU; propose_fetch returns them oldest first."""
        self._last_params = params
        if not hasattr(self, "_queued"):
            self._queued = []
        if fmap is None:
            self._chk(self.L.az_propose_launch(self.h, ctypes.byref(params)))
            self._queued.append(params)
            return
        # (the layout checks of a tensor are remembered per tensor object: between two searches the GPU waits for
        #  exactly this host code)
        ck = getattr(self, "_map_cache", None)
        if ck is None:
            ck = self._map_cache = {}
        ent = ck.get(id(fmap))
        ptr = fmap.data_ptr()
        if ent is None or ent[0] != ptr or ent[5]() is not fmap:
            import weakref
            t, cl = self._torch_map(fmap)
            C, H, W = (int(x) for x in t.shape)
            if len(ck) > 64:
                ck.clear()
            ent = ck[id(fmap)] = (ptr, C, H, W, 1 if cl else 0, weakref.ref(fmap), t.device)
        _, C, H, W, cl, _, dev = ent
        if producer_event is not None:
            self.wait_event(producer_event, params)
        elif not producer_done:
            import torch
            torch.cuda.current_stream(dev).synchronize()
        self._chk(self.L.az_propose_launch_on(self.h, ctypes.byref(params), ctypes.c_void_p(ptr), C, H, W, cl))
        self._queued.append(params)
        # (up to six searches may be queued -- three per lane: their maps stay referenced until they are long fetched)
        import collections
        self.__dict__.setdefault("_feat_keep", collections.deque(maxlen=10)).append(fmap)
        self._feat_keepalive = fmap
        self.feat_shape = (C, H, W)

    # ---- a batch of images in lockstep (az_batch_launch) ------------------------------------------------------------
    def batch_launch(self, params, fmaps, producer_done=False, producer_event=None):
        """The images of consecutive iterations of the dataset loop (lib/detect/test.py:508-513), all of ONE shape, searched
        together: every level's rois of all of them in one head pass (az_batch_launch).  fmaps: CUDA tensors [1,C,H,W] /
        [C,H,W] on this GPU, one per image (torch.channels_last ones are read where they lie, others are converted by torch);
        they must stay untouched until the batch's last batch_fetch.  producer_done / producer_event as propose_launch.
        Results: batch_fetch(i), i = 0 .. len(fmaps)-1 in order; each is what propose gives for that image alone.
        params may also be a LIST of AzParams, one per image: the images of the batch then have shapes of their own
        (az_batch_launch_shapes; they must walk the same number of levels and share num_proposals, eps, min_side, flags)."""
        import torch
        maps, ptrs, shape, hw = [], [], None, []
        converted = False
        # (the layout checks of a tensor are remembered per tensor object, as propose_launch does: a batch of 32 maps is
        #  otherwise ~0.3 ms of Python)
        ck = self.__dict__.setdefault("_bmap_cache", {})
        for f in fmaps:
            ent = ck.get(id(f))
            ptr = f.data_ptr()
            if ent is None or ent[0] != ptr or ent[2]() is not f:
                import weakref
                t = f if f.dim() == 4 else f[None]
                assert t.is_cuda and t.dtype == torch.float32 and t.device.index == self.device and t.shape[0] == 1
                if not t.is_contiguous(memory_format=torch.channels_last):
                    t = t.contiguous(memory_format=torch.channels_last)
                    converted = True
                    ent = None                       # (a converted copy is made again every time: the source may have changed)
                else:
                    # (only the checks' outcome is remembered, never the tensor or a view of it: an entry must not keep a
                    #  conv map alive -- a dataset loop hands over a fresh tensor per image; entries whose tensor has died
                    #  are dropped as soon as a few have gathered)
                    if len(ck) >= 64:
                        for k in [k for k, e in ck.items() if e[2]() is None]:
                            del ck[k]
                        if len(ck) >= 256:
                            ck.clear()
                    ent = ck[id(f)] = (ptr, tuple(int(x) for x in t.shape[1:]), weakref.ref(f))
                chw = tuple(int(x) for x in t.shape[1:])
            else:
                t, chw = (f if f.dim() == 4 else f[None]), ent[1]
            per_image = isinstance(params, (list, tuple))
            assert per_image or shape in (None, chw), "the maps of a batch have one shape (or pass one AzParams per image)"
            assert shape is None or shape[0] == chw[0]
            shape = chw
            maps.append(t)
            ptrs.append(t.data_ptr())
            hw.append(chw[1:])
        C, H, W = shape
        dev = maps[0].device
        if producer_event is not None and not converted:
            self._ext(self.L.az_batch_next_stream(self.h)).wait_event(producer_event)
        elif converted or not producer_done:
            torch.cuda.current_stream(dev).synchronize()
        arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
        self._batch_stream = self._ext(self.L.az_batch_next_stream(self.h))       # (the stream this batch runs on)
        if isinstance(params, (list, tuple)):
            assert len(params) == len(ptrs)
            pa = (AzParams * len(ptrs))(*params)
            Hs = (ctypes.c_int * len(ptrs))(*[h for h, _ in hw])
            Ws = (ctypes.c_int * len(ptrs))(*[w for _, w in hw])
            self._chk(self.L.az_batch_launch_shapes(self.h, len(ptrs), pa, arr, C, Hs, Ws))
            params = params[0]
        else:
            self._chk(self.L.az_batch_launch(self.h, len(ptrs), ctypes.byref(params), arr, C, H, W))
        import collections
        q = self.__dict__.setdefault("_batches", collections.deque())
        q.append((params, maps))
        self.feat_shape = (C, H, W)

    def batch_stage_results(self, dst_ptr, pitch_bytes, cap_bytes):
        """Right behind batch_launch: the batch's result records to dst_ptr + i * pitch_bytes (a raw device pointer, e.g. rows
        of the RCCL send buffer), device to device; image i's is complete when batch_fetch(i) returns."""
        self._chk(self.L.az_batch_stage_results_dev(self.h, ctypes.c_void_p(int(dst_ptr)), int(pitch_bytes), int(cap_bytes)))

    def batch_fetch_all(self, want_scores=False, want_stats=False):
        """Every image of the oldest unfetched batch in one call (az_batch_fetch_all): a list of what batch_fetch(i) returns."""
        if not getattr(self, "_batches", None):
            raise AzError(-4, "batch_fetch_all without batch_launch")
        params, maps = self._batches[0]
        n, cap = len(maps), params.num_proposals
        boxes = np.empty((n, cap, 4), dtype=np.float64)
        scores = np.empty((n, cap), dtype=np.float32)
        cnt = (ctypes.c_int * n)()
        st = (AzStats * n)()
        try:
            self._chk(self.L.az_batch_fetch_all(self.h, _p(boxes, ctypes.c_double), _p(scores, ctypes.c_float), cap, cnt, st))
        finally:
            self._batches.popleft()
        out = []
        for i in range(n):
            r = [boxes[i, :cnt[i]].copy()]
            if want_scores:
                r.append(scores[i, :cnt[i]].copy())
            if want_stats:
                r.append(st[i])
            out.append(r[0] if len(r) == 1 else tuple(r))
        return out

    def batch_drain(self):
        """Collect and drop every batch still in flight (after an error in the caller's loop: the context is usable again)."""
        while getattr(self, "_batches", None):
            try:
                self.batch_fetch_all()
            except AzError:
                pass

    def batch_record_event(self):
        """A torch.cuda.Event recorded now on the stream of the batch launched last: behind that batch."""
        return self._batch_stream.record_event()

    def batch_fetch(self, i, want_scores=False, want_stats=False):
        if not getattr(self, "_batches", None):
            raise AzError(-4, "batch_fetch without batch_launch")
        params, maps = self._batches[0]
        try:
            return self._search_result(lambda *out: self.L.az_batch_fetch(self.h, int(i), *out), params.num_proposals,
                                       want_scores, want_stats)
        finally:
            if i == len(maps) - 1:
                self._batches.popleft()

    def propose_fetch(self, want_scores=False, want_stats=False):
        params = self._queued.pop(0) if getattr(self, "_queued", None) else self._last_params
        cap = params.num_proposals if params.fixed_num else self.max_candidates
        return self._search_result(lambda *out: self.L.az_propose_fetch(self.h, *out), cap, want_scores, want_stats)

    @staticmethod
    def result_record_layout(num_proposals):
        """(bytes, n_offset, boxes_offset, scores_offset) of the device-resident result record of a
        fixed-count search (az_result_record_layout)."""
        L = load_library()
        v = [ctypes.c_size_t(0) for _ in range(4)]
        rc = L.az_result_record_layout(int(num_proposals), *[ctypes.byref(x) for x in v])
        if rc != AZ_OK:
            raise AzError(rc, "az_result_record_layout(%r)" % (num_proposals,))
        return tuple(int(x.value) for x in v)

    # ---- the exchange step, natively (one ncclAllGather on the ctx stream) ---------------------------------------------
    @staticmethod
    def rccl_unique_id():
        """128 bytes (made on rank 0, handed to the other ranks by the launcher) for rccl_init."""
        L = load_library()
        buf = ctypes.create_string_buffer(128)
        rc = L.az_rccl_unique_id(buf, 128)
        if rc != AZ_OK:
            raise AzError(rc, "az_rccl_unique_id: no usable librccl.so in this process")
        return bytes(buf.raw)

    def rccl_init(self, uid, nranks, rank):
        assert len(uid) == 128
        self._chk(self.L.az_rccl_init(self.h, ctypes.create_string_buffer(uid, 128), 128, int(nranks), int(rank)))

    def gather_records(self, send_ptr, recv_ptr, bytes_per_rank):
        """ncclAllGather of this rank's staged records (az_gather_records): enqueued on the ctx stream."""
        self._chk(self.L.az_gather_records(self.h, ctypes.c_void_p(int(send_ptr)), ctypes.c_void_p(int(recv_ptr)),
                                           int(bytes_per_rank)))

    def rccl_destroy(self):
        self._chk(self.L.az_rccl_destroy(self.h))

    def comm_stream(self):
        """torch view of the stream az_gather_records runs on (exists after rccl_init)."""
        return self._ext(self.L.az_comm_stream(self.h))

    def stage_result(self, dst_ptr, cap_bytes):
        """Between propose_launch and propose_fetch: enqueue a device-to-device copy of the result
        record to `dst_ptr` (a raw device pointer, e.g. a slot of the RCCL send buffer)."""
        self._chk(self.L.az_propose_stage_result_dev(self.h, ctypes.c_void_p(int(dst_ptr)), int(cap_bytes)))

    def last_candidates(self):
        cap = self.max_candidates
        boxes = np.empty((cap, 4), dtype=np.float64)
        scores = np.empty((cap,), dtype=np.float32)
        n = ctypes.c_int(0)
        self._chk(self.L.az_last_candidates(self.h, _p(boxes, ctypes.c_double), _p(scores, ctypes.c_float),
                                            cap, ctypes.byref(n)))
        return boxes[:n.value].copy(), scores[:n.value].copy()

    # ---- unit entry points ----------------------------------------------------------
    def divide_region(self, regions, min_side=10.0):
        regions = _f64(regions).reshape(-1, 4)
        cap = max(16, 12 * regions.shape[0] + 64)
        out = np.empty((cap, 4), dtype=np.float64)
        n = ctypes.c_int(0)
        rc = self.L.az_divide_region(self.h, _p(regions, ctypes.c_double), regions.shape[0], float(min_side),
                                     _p(out, ctypes.c_double), cap, ctypes.byref(n))
        if rc == AZ_ERR_CAPACITY and n.value > cap:
            cap = n.value
            out = np.empty((cap, 4), dtype=np.float64)
            rc = self.L.az_divide_region(self.h, _p(regions, ctypes.c_double), regions.shape[0],
                                         float(min_side), _p(out, ctypes.c_double), cap, ctypes.byref(n))
        self._chk(rc)
        return out[:n.value].copy()

    def sift_dup(self, regions, min_side=10.0):
        regions = _f64(regions).reshape(-1, 4)
        cap = max(1, regions.shape[0])
        out = np.empty((cap, 4), dtype=np.float64)
        n = ctypes.c_int(0)
        self._chk(self.L.az_sift_dup(self.h, _p(regions, ctypes.c_double), regions.shape[0], float(min_side),
                                     _p(out, ctypes.c_double), cap, ctypes.byref(n)))
        return out[:n.value].copy()

    def roi_dedup(self, boxes, scale, dedup=1. / 16., batch_size=10000):
        return self._roi_dedup(self.L.az_roi_dedup, (float(scale),), boxes, dedup, batch_size)

    def _roi_dedup(self, fn, proj, boxes, dedup, batch_size):
        """az_roi_dedup / az_roi_dedup_pyramid (fn), proj: the arguments that name the scale or the pyramid."""
        boxes = _f64(boxes).reshape(-1, 4)
        P = boxes.shape[0]
        rois = np.empty((max(P, 1), 5), dtype=np.float32)
        index = np.empty((max(P, 1),), dtype=np.int32)
        inv = np.empty((max(P, 1),), dtype=np.int32)
        n = ctypes.c_int(0)
        self._chk(fn(self.h, _p(boxes, ctypes.c_double), P, *proj, float(dedup), int(batch_size), _p(rois, ctypes.c_float),
                     _p(index, ctypes.c_int32), _p(inv, ctypes.c_int32), ctypes.byref(n)))
        return rois[:P].copy(), index[:n.value].copy(), inv[:P].copy()

    def roi_pool(self, rois):
        return self._roi_pool(self.L.az_roi_pool, rois)

    def _roi_pool(self, fn, rois):
        rois = _f32(rois).reshape(-1, 5)
        R = rois.shape[0]
        out = np.empty((max(R, 1), self.dims["K6"]), dtype=np.float32)
        self._chk(fn(self.h, _p(rois, ctypes.c_float), R, _p(out, ctypes.c_float)))
        return out[:R]

    def head_forward(self, rois):
        rois = _f32(rois).reshape(-1, 5)
        R = rois.shape[0]
        z = np.empty((max(R, 1), 1), dtype=np.float32)
        p = np.empty((max(R, 1), AZ_NUM_SUBREG), dtype=np.float32)
        d = np.empty((max(R, 1), 4 * AZ_NUM_SUBREG), dtype=np.float32)
        self._chk(self.L.az_head_forward(self.h, _p(rois, ctypes.c_float), R, _p(z, ctypes.c_float),
                                         _p(p, ctypes.c_float), _p(d, ctypes.c_float)))
        return z[:R], p[:R], d[:R]

    def decode_filter(self, anchors, deltas, scores, im_h, im_w, eps=1e-14, min_side=10.0):
        anchors = _f64(anchors).reshape(-1, 4)
        R = anchors.shape[0]
        deltas = _f32(deltas).reshape(R, 4 * AZ_NUM_SUBREG)
        scores = _f32(scores).reshape(R, AZ_NUM_SUBREG)
        cap = max(1, R * AZ_NUM_SUBREG)
        ob = np.empty((cap, 4), dtype=np.float64)
        os_ = np.empty((cap,), dtype=np.float32)
        n = ctypes.c_int(0)
        self._chk(self.L.az_decode_filter(self.h, _p(anchors, ctypes.c_double), _p(deltas, ctypes.c_float),
                                          _p(scores, ctypes.c_float), R, int(im_h), int(im_w), float(eps),
                                          float(min_side), _p(ob, ctypes.c_double), _p(os_, ctypes.c_float),
                                          cap, ctypes.byref(n)))
        return ob[:n.value].copy(), os_[:n.value].copy()

    def topk(self, scores, k, radix=False):
        """radix=True: az_topk_radix, the single-workgroup radix select at every size (same result, for tests)."""
        scores = _f32(scores).ravel()
        idx = np.empty((max(1, min(k, scores.shape[0])),), dtype=np.int32)
        n = ctypes.c_int(0)
        fn = self.L.az_topk_radix if radix else self.L.az_topk
        self._chk(fn(self.h, _p(scores, ctypes.c_float), scores.shape[0], int(k), _p(idx, ctypes.c_int32), ctypes.byref(n)))
        return idx[:n.value].copy()

    def topk_radix(self, scores, k):
        return self.topk(scores, k, radix=True)

    def nms(self, dets, thresh):
        dets = _f32(dets).reshape(-1, 5)
        N = dets.shape[0]
        keep = np.empty((max(N, 1),), dtype=np.int64)
        n = ctypes.c_int(0)
        self._chk(self.L.az_nms(self.h, _p(dets, ctypes.c_float), N, float(thresh), _p(keep, ctypes.c_int64),
                                ctypes.byref(n)))
        return keep[:n.value].copy()

    # ---- Fast R-CNN head on the shared map -----------------------------------------------
    def nms_batched(self, dets_list, thresh):
        """NMS of many independent box sets ([n_g,5] float32 each) in one call -> list of keep index
        arrays (what apply_nms, lib/detect/test.py:467-484, needs per class per image)."""
        n = len(dets_list)
        off = np.zeros(n + 1, dtype=np.int32)
        for g, d in enumerate(dets_list):
            off[g + 1] = off[g] + d.shape[0]
        allb = _f32(np.vstack([np.zeros((0, 5), np.float32)] + [np.asarray(d, dtype=np.float32).reshape(-1, 5)
                                                                   for d in dets_list]))
        keep = np.zeros(max(int(off[n]), 1), dtype=np.int64)
        nk = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self.L.az_nms_batched(self.h, _p(allb, ctypes.c_float), _p(off, ctypes.c_int32), n, float(thresh),
                                        _p(keep, ctypes.c_int64), _p(nk, ctypes.c_int32)))
        return [keep[off[g]:off[g] + nk[g]].copy() for g in range(n)]

    @staticmethod
    def _groups(dets_list):
        """(offsets int32 [n + 1], all rows float32 [total, 5]) of a list of [n_g, 5] box sets."""
        n = len(dets_list)
        off = np.zeros(n + 1, dtype=np.int32)
        for g, d in enumerate(dets_list):
            off[g + 1] = off[g] + np.asarray(d).reshape(-1, 5).shape[0]
        allb = _f32(np.vstack([np.zeros((0, 5), np.float32)] + [np.asarray(d, dtype=np.float32).reshape(-1, 5)
                                                                   for d in dets_list]))
        return off, allb

    def soft_nms_batched(self, dets_list, method, thresh, sigma=0.5, min_score=0.001):
        """Soft-NMS (az_soft_nms_batched) of many independent box sets ([n_g,5] float32 each) in one call.  method: 'hard',
        'linear', 'gaussian' or an AZ_NMS_* value.  Returns a list of (keep int64 [nk], scores float32 [nk]): the picked
        indices in pick order and their scores when they were picked."""
        n = len(dets_list)
        off, allb = self._groups(dets_list)
        if isinstance(method, str):
            if method not in NMS_METHODS:
                raise ValueError("NMS method %r: 'hard', 'linear' or 'gaussian'" % (method,))
            method = NMS_METHODS[method]
        keep = np.zeros(max(int(off[n]), 1), dtype=np.int64)
        sc = np.zeros(max(int(off[n]), 1), dtype=np.float32)
        nk = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self.L.az_soft_nms_batched(self.h, _p(allb, ctypes.c_float), _p(off, ctypes.c_int32), n, int(method),
                                             float(thresh), float(sigma), float(min_score), _p(keep, ctypes.c_int64),
                                             _p(sc, ctypes.c_float), _p(nk, ctypes.c_int32)))
        return [(keep[off[g]:off[g] + nk[g]].copy(), sc[off[g]:off[g] + nk[g]].copy()) for g in range(n)]

    def box_vote_batched(self, dets_list, keeps, vote_thresh):
        """Box voting (az_box_vote_batched): dets_list the ORIGINAL box sets, keeps one index array per set (from nms_batched
        or soft_nms_batched).  Returns a list of [nk, 4] float32 arrays: the voted box of every kept box, in keep order."""
        n = len(dets_list)
        if len(keeps) != n:
            raise AzError(AZ_ERR_INVALID, "box_vote_batched: one keep list per box set")
        off, allb = self._groups(dets_list)
        keep = np.zeros(max(int(off[n]), 1), dtype=np.int64)
        nk = np.zeros(max(n, 1), dtype=np.int32)
        lists = [np.asarray(k, dtype=np.int64).ravel() for k in keeps]
        lens = np.array([k.size for k in lists], dtype=np.int64)
        long = np.flatnonzero(lens > np.diff(off))
        if long.size:
            raise AzError(AZ_ERR_INVALID, "box_vote_batched: keep list %d is longer than its box set" % long[0])
        if n:
            flat = np.concatenate(lists)
            # list g goes to keep[off[g] ...]: its elements' positions in `flat`, moved by off[g] - (where list g starts in flat)
            keep[np.arange(flat.size) + np.repeat(off[:n] - (np.cumsum(lens) - lens), lens)] = flat
            nk[:n] = lens
        out = np.zeros((max(int(off[n]), 1), 4), dtype=np.float32)
        self._chk(self.L.az_box_vote_batched(self.h, _p(allb, ctypes.c_float), _p(off, ctypes.c_int32), n,
                                             _p(keep, ctypes.c_int64), _p(nk, ctypes.c_int32), float(vote_thresh),
                                             _p(out, ctypes.c_float)))
        return [out[off[g]:off[g] + nk[g]].copy() for g in range(n)]

    def load_det_head(self, head):
        """head: dict of Caffe-layout fp32 arrays W6,b6 (fc6), W7,b7 (fc7), Wc,bc (cls_score),
        Wb,bb (bbox_pred).  A head that carries truncated-SVD factors (L6 / U6 and / or L7 / U7: aznet_hip.compress,
        caffemodel.det_head_from_layers of a compressed file) goes through load_det_head_lowrank."""
        if is_lowrank_head(head):
            return self.load_det_head_lowrank(head)
        W6 = _f32(head["W6"])
        n6, K6 = W6.shape
        assert K6 % 49 == 0
        C = K6 // 49
        n7 = head["W7"].shape[0]
        ncls = head["Wc"].shape[0]
        assert head["W7"].shape == (n7, n6) and head["Wc"].shape == (ncls, n7) and head["Wb"].shape == (4 * ncls, n7)
        arrs = [W6] + [_f32(head[k]) for k in ("b6", "W7", "b7", "Wc", "bc", "Wb", "bb")]
        self._chk(self.L.az_load_det_head(self.h, C, n6, n7, ncls, *[_p(a, ctypes.c_float) for a in arrs]))
        self.det_dims = dict(C=C, n6=n6, n7=n7, ncls=ncls)
        if self.skip_dims is not None and self.skip_dims["Cout"] != C:
            self.skip_dims = None      # (az_load_det_head dropped the front: it folds to the head's C)

    def load_det_head_lowrank(self, head):
        """az_load_det_head_lowrank.  head: as load_det_head's, with fc6 given as L6 [r6, C*49], U6 [n6, r6], b6 instead of
        W6, b6 and / or fc7 as L7 [r7, n6], U7 [n7, r7], b7 instead of W7, b7 (a layer given as W stays at full rank)."""
        def layer(i):
            if ("L%d" % i in head) != ("U%d" % i in head):
                raise ValueError("a low-rank head needs both L%d and U%d" % (i, i))
            if "L%d" % i in head:
                Lf, U = _f32(head["L%d" % i]), _f32(head["U%d" % i])
                if Lf.ndim != 2 or U.ndim != 2 or U.shape[1] != Lf.shape[0]:
                    raise ValueError("L%d %s and U%d %s do not chain" % (i, Lf.shape, i, U.shape))
                return Lf, U, Lf.shape[0], U.shape[0], Lf.shape[1]
            W = _f32(head["W%d" % i])
            return None, W, 0, W.shape[0], W.shape[1]
        L6, U6, r6, n6, K6 = layer(6)
        L7, U7, r7, n7, in7 = layer(7)
        assert K6 % 49 == 0
        C = K6 // 49
        ncls = head["Wc"].shape[0]
        assert in7 == n6 and head["Wc"].shape == (ncls, n7) and head["Wb"].shape == (4 * ncls, n7)
        b6, b7, Wc, bc, Wb, bb = [_f32(head[k]) for k in ("b6", "b7", "Wc", "bc", "Wb", "bb")]
        assert b6.size == n6 and b7.size == n7
        pf = lambda a: _p(a, ctypes.c_float) if a is not None else None
        self._chk(self.L.az_load_det_head_lowrank(self.h, C, n6, n7, ncls, r6, r7, pf(L6), pf(U6), pf(b6), pf(L7), pf(U7),
                                                  pf(b7), pf(Wc), pf(bc), pf(Wb), pf(bb)))
        self.det_dims = dict(C=C, n6=n6, n7=n7, ncls=ncls, r6=r6, r7=r7)
        if self.skip_dims is not None and self.skip_dims["Cout"] != C:
            self.skip_dims = None      # (the load dropped the front: it folds to the head's C)

    def lowrank_gemm_unit(self, X, W, b, relu=True, M=None):
        """az_lowrank_gemm_unit (tests): the U-stage kernel alone -> act(X[:M] . W^T + b), [M, N] float32."""
        X, W, b = _f32(X), _f32(W), _f32(b).reshape(-1)
        K = X.shape[1] if X.ndim == 2 else 0
        M = X.shape[0] if M is None else int(M)
        N = W.shape[0]
        if X.ndim != 2 or W.ndim != 2 or W.shape[1] != K or b.size != N or M > X.shape[0]:
            raise AzError(AZ_ERR_INVALID, "lowrank_gemm_unit: X [M, K], W [N, K], b [N]")
        Y = np.zeros((max(M, 1), N), dtype=np.float32)
        self._chk(self.L.az_lowrank_gemm_unit(self.h, _p(X, ctypes.c_float), _p(W, ctypes.c_float), _p(b, ctypes.c_float),
                                              M, N, K, 1 if relu else 0, _p(Y, ctypes.c_float)))
        return Y[:M]

    def _det_forward(self, fn, rois):
        """az_det_forward / az_det_forward_skip (fn): the head alone on rois [R, 5]."""
        rois = _f32(rois).reshape(-1, 5)
        R = rois.shape[0]
        nc = self.det_dims["ncls"]
        p = np.empty((max(R, 1), nc), dtype=np.float32)
        b = np.empty((max(R, 1), 4 * nc), dtype=np.float32)
        self._chk(fn(self.h, _p(rois, ctypes.c_float), R, _p(p, ctypes.c_float), _p(b, ctypes.c_float)))
        return p[:R], b[:R]

    def det_forward(self, rois):
        return self._det_forward(self.L.az_det_forward, rois)

    def detect(self, boxes, scale, im_h, im_w, dedup=1. / 16., batch_size=10000, eps=1e-14):
        return self._detect(self.L.az_detect, (float(scale),), boxes, im_h, im_w, dedup, batch_size, eps)

    def _det_out(self, P):
        """The detections of P boxes as the az_detect* entries write them: (scores [P, ncls] f32, boxes [P, 4 ncls] f64)."""
        nc = self.det_dims["ncls"]
        return np.empty((max(P, 1), nc), dtype=np.float32), np.empty((max(P, 1), 4 * nc), dtype=np.float64)

    def _detect(self, fn, proj, boxes, im_h, im_w, dedup, batch_size, eps):
        """az_detect / az_detect_skip / az_detect_pyramid (fn), proj: the arguments that name the scale or the pyramid."""
        boxes = _f64(boxes).reshape(-1, 4)
        P = boxes.shape[0]
        s, b = self._det_out(P)
        self._chk(fn(self.h, _p(boxes, ctypes.c_double), P, *proj, float(dedup), int(batch_size), int(im_h), int(im_w),
                     float(eps), _p(s, ctypes.c_float), _p(b, ctypes.c_double)))
        return s[:P], b[:P]

    # ---- the skip-connection detector (az_skip.hip) -------------------------------------------
    def load_skip_front(self, front):
        """front: dict with Cs (channels of each source), scales (their ROIPooling spatial_scale), Wp [Cout, sum Cs] or
        Caffe's [Cout, sum Cs, 1, 1] and bp [Cout] (conv_pool5), and optionally gain (scale5: 1000) and eps (the GRN
        layers': 1e-10), as synth.make_skip_front / caffemodel.skip_front_from_layers return it.  Needs load_det_head."""
        Cs = np.ascontiguousarray(front["Cs"], dtype=np.intc).reshape(-1)
        sc = _f32(front["scales"]).reshape(-1)
        assert Cs.shape[0] == sc.shape[0]
        Wp = _f32(front["Wp"])
        Wp = Wp.reshape(Wp.shape[0], -1)
        bp = _f32(front["bp"]).reshape(-1)
        Cout = Wp.shape[0]
        assert Wp.shape == (Cout, int(Cs.sum())) and bp.shape == (Cout,), (Wp.shape, bp.shape, Cs)
        self._chk(self.L.az_load_skip_front(self.h, int(Cs.shape[0]), _p(Cs, ctypes.c_int), _p(sc, ctypes.c_float),
                                            float(front.get("gain", 1000.0)), float(front.get("eps", 1e-10)), int(Cout),
                                            _p(Wp, ctypes.c_float), _p(bp, ctypes.c_float)))
        self.skip_dims = dict(Cs=[int(x) for x in Cs], sumC=int(Cs.sum()), Cout=int(Cout))

    def _need_front(self, who):
        """The entries that size their buffers by the front: without one, the ABI's own refusal."""
        if self.skip_dims is None:
            raise AzError(AZ_ERR_STATE, "%s: az_load_skip_front has not been called" % who)

    def set_skip_maps(self, maps, producer_done=False):
        """maps: one float32 CUDA tensor per source of the loaded front, in its order ([1,C,H,W] or [C,H,W]); borrowed
        (kept alive here).  A map that is not torch.channels_last is copied into that layout first.  torch's current
        stream is synchronised unless producer_done."""
        import torch
        self._need_front("set_skip_maps")
        ts = []
        for m in maps:
            assert m.is_cuda and m.dtype == torch.float32 and m.device.index == self.device, \
                "skip maps must be float32 CUDA tensors on this context's GPU"
            if m.dim() == 3:
                m = m[None]
            assert m.dim() == 4 and m.shape[0] == 1
            # (NHWC memory whatever the strides of size-1 dimensions say)
            ts.append(m.permute(0, 2, 3, 1).contiguous())
        if not producer_done:
            torch.cuda.current_stream(ts[0].device).synchronize()
        n = len(ts)
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        Hs = np.array([t.shape[1] for t in ts], dtype=np.intc)
        Ws = np.array([t.shape[2] for t in ts], dtype=np.intc)
        Cs = np.array([t.shape[3] for t in ts], dtype=np.intc)
        self._chk(self.L.az_set_skip_maps_dev_nhwc(self.h, n, ptrs, _p(Cs, ctypes.c_int), _p(Hs, ctypes.c_int),
                                                   _p(Ws, ctypes.c_int)))
        self._skip_keepalive = ts
        if int(Cs[-1]) == self.skip_dims["Cout"]:          # (the context's ordinary map as well: az_set_skip_maps_dev_nhwc)
            self._feat_keepalive = ts[-1]
            self.feat_shape = (int(Cs[-1]), int(Hs[-1]), int(Ws[-1]))

    def detect_skip(self, boxes, scale, im_h, im_w, dedup=1. / 16., batch_size=10000, eps=1e-14):
        return self._detect(self.L.az_detect_skip, (float(scale),), boxes, im_h, im_w, dedup, batch_size, eps)

    def detect_iter(self, boxes, scale, im_h, im_w, rounds, min_score, max_rows, dedup=1. / 16., batch_size=10000, eps=1e-14,
                    skip=False):
        """az_detect_iter (skip: az_detect_iter_skip): iterative box localisation.  Returns (scores [P, ncls], boxes
        [P, 4 ncls], extra); extra is a dict of the later rounds' rows, round after round: cls, src (int32), round (int32: 2,
        3, ...), score (float32), box ([., 4] float64), and count (int32 [rounds - 1]: the rows of each round)."""
        boxes = _f64(boxes).reshape(-1, 4)
        P = boxes.shape[0]
        rounds, max_rows = int(rounds), int(max_rows)
        # (sized only for arguments the entry accepts: anything else it refuses before it touches a buffer)
        ok = 1 <= rounds <= AZ_ITER_LOC_MAX_ROUNDS and 1 <= max_rows <= AZ_ITER_LOC_MAX_ROWS
        cap = max((rounds - 1) * max_rows, 1) if ok else 1
        s, b = self._det_out(P)
        cls = np.empty(cap, dtype=np.int32)
        src = np.empty(cap, dtype=np.int32)
        sc = np.empty(cap, dtype=np.float32)
        bx = np.empty((cap, 4), dtype=np.float64)
        cnt = np.zeros(max(rounds - 1, 1) if ok else 1, dtype=np.int32)
        fn = self.L.az_detect_iter_skip if skip else self.L.az_detect_iter
        self._chk(fn(self.h, _p(boxes, ctypes.c_double), P, float(scale), float(dedup), int(batch_size), int(im_h), int(im_w),
                     float(eps), rounds, float(min_score), max_rows, _p(s, ctypes.c_float), _p(b, ctypes.c_double),
                     _p(cls, ctypes.c_int32), _p(src, ctypes.c_int32), _p(sc, ctypes.c_float), _p(bx, ctypes.c_double),
                     _p(cnt, ctypes.c_int32)))
        cnt = cnt[:rounds - 1]
        n = int(cnt.sum())
        extra = dict(cls=cls[:n], src=src[:n], round=np.repeat(np.arange(2, rounds + 1, dtype=np.int32), cnt), score=sc[:n],
                     box=bx[:n], count=cnt)
        return s[:P], b[:P], extra

    def det_forward_skip(self, rois):
        return self._det_forward(self.L.az_det_forward_skip, rois)

    def skip_pool(self, rois, normalise=True):
        """concat5 of the rois, [R*49, sum Cs] (row = roi * 49 + bin): the raw ROIPooling maxima (normalise=False) or
        the normalised, scaled rows the 1x1 convolution reads."""
        self._need_front("skip_pool")
        rois = _f32(rois).reshape(-1, 5)
        R = rois.shape[0]
        out = np.empty((max(R, 1) * 49, self.skip_dims["sumC"]), dtype=np.float32)
        self._chk(self.L.az_skip_pool(self.h, _p(rois, ctypes.c_float), R, 1 if normalise else 0, _p(out, ctypes.c_float)))
        return out[:R * 49]

    def skip_conv(self, cat):
        """conv_pool5 + relu_pool of host rows [rows, sum Cs] -> [rows, Cout]."""
        self._need_front("skip_conv")
        cat = _f32(cat).reshape(-1, self.skip_dims["sumC"])
        rows = cat.shape[0]
        out = np.empty((max(rows, 1), self.skip_dims["Cout"]), dtype=np.float32)
        self._chk(self.L.az_skip_conv(self.h, _p(cat, ctypes.c_float), rows, _p(out, ctypes.c_float)))
        return out[:rows]

    def detect_batch(self, maps, boxes_list, scales, im_shapes, dedup=1. / 16., batch_size=10000, eps=1e-14):
        """detect() for several images at once (az_detect_batch): maps[i] is image i's conv5_3, a float32 CUDA tensor on
        this GPU ([1,C,H,W] / [C,H,W]; channels_last ones are read in place, others are converted on torch's current
        stream), boxes_list[i] its proposals [P_i,4], scales[i] / im_shapes[i] its scale and (h, w, ...).  Returns
        [(scores f32 [P_i,K], boxes f64 [P_i,4K])], each bit for bit what detect() returns for that image alone.  Up to
        AZ_BATCH_MAX images go to one call; an image with more boxes than the region capacity is run in pieces that
        start at a multiple of batch_size (dedup is per chunk, so the bits stay the same)."""
        import torch
        n = len(boxes_list)
        assert len(maps) == n and len(scales) == n and len(im_shapes) == n
        nc = self.det_dims["ncls"]
        C = self.det_dims["C"]
        boxes_list = [_f64(b).reshape(-1, 4) for b in boxes_list]
        piece = (self.max_regions // int(batch_size)) * int(batch_size)
        # (item = one call row: image index, first box, box count)
        items = []
        for i, b in enumerate(boxes_list):
            P = b.shape[0]
            if P <= self.max_regions:
                items.append((i, 0, P))
            elif piece <= 0:
                raise AzError(AZ_ERR_CAPACITY, "detect_batch: batch_size %d exceeds the region capacity %d"
                              % (batch_size, self.max_regions))
            else:
                items.extend((i, s0, min(piece, P - s0)) for s0 in range(0, P, piece))
        views = {}
        for i, m in enumerate(maps):
            if boxes_list[i].shape[0] == 0:
                continue
            if isinstance(m, np.ndarray):
                m = torch.from_numpy(_f32(m)).to("cuda:%d" % self.device)
            t = m if m.dim() == 4 else m.unsqueeze(0)
            assert t.is_cuda and t.dtype == torch.float32 and t.shape[0] == 1 and t.device.index == self.device, \
                "maps must be float32 CUDA tensors on this context's GPU"
            if not t.is_contiguous(memory_format=torch.channels_last):
                t = t.contiguous(memory_format=torch.channels_last)
            views[i] = t
        if views:
            torch.cuda.current_stream(self.device).synchronize()           # (the maps are complete)
        outs = [(np.empty((b.shape[0], nc), np.float32), np.empty((b.shape[0], 4 * nc), np.float64)) for b in boxes_list]
        for k0 in range(0, len(items), AZ_BATCH_MAX):
            grp = items[k0:k0 + AZ_BATCH_MAX]
            m = len(grp)
            ptrs = (ctypes.c_void_p * m)()
            Hs = np.zeros(m, np.int32)
            Ws = np.zeros(m, np.int32)
            off = np.zeros(m + 1, np.int32)
            sc = np.zeros(m, np.float64)
            hw = np.zeros((m, 2), np.int32)
            for k, (i, s0, P) in enumerate(grp):
                off[k + 1] = off[k] + P
                sc[k] = float(scales[i])
                hw[k] = (int(im_shapes[i][0]), int(im_shapes[i][1]))
                if P:
                    t = views[i]
                    ptrs[k] = t.data_ptr()
                    Hs[k], Ws[k] = int(t.shape[2]), int(t.shape[3])
                    if int(t.shape[1]) != C:
                        raise AzError(AZ_ERR_INVALID, "detect_batch: map %d has %d channels, the detection head %d"
                                      % (i, int(t.shape[1]), C))
            B = np.ascontiguousarray(np.concatenate([boxes_list[i][s0:s0 + P] for i, s0, P in grp])
                                     if off[m] else np.zeros((1, 4)), dtype=np.float64)
            S = np.empty((max(int(off[m]), 1), nc), np.float32)
            D = np.empty((max(int(off[m]), 1), 4 * nc), np.float64)
            self._chk(self.L.az_detect_batch(
                self.h, m, ptrs, C, _p(Hs, ctypes.c_int32), _p(Ws, ctypes.c_int32), _p(B, ctypes.c_double),
                _p(off, ctypes.c_int32), _p(sc, ctypes.c_double), _p(hw, ctypes.c_int32), float(dedup), int(batch_size),
                float(eps), _p(S, ctypes.c_float), _p(D, ctypes.c_double)))
            for k, (i, s0, P) in enumerate(grp):
                outs[i][0][s0:s0 + P] = S[off[k]:off[k + 1]]
                outs[i][1][s0:s0 + P] = D[off[k]:off[k + 1]]
        return outs

    # ---- tuner ------------------------------------------------------------------------
    def last_anchors(self):
        """(regions [n,4] f64, zoom [n] f32) of the last tuner-variant search (Bhis, tune.py:303)."""
        cap = 2 * self.max_regions
        regions = np.empty((cap, 4), dtype=np.float64)
        zoom = np.empty((cap,), dtype=np.float32)
        n = ctypes.c_int(0)
        self._chk(self.L.az_last_anchors(self.h, _p(regions, ctypes.c_double), _p(zoom, ctypes.c_float), cap,
                                         ctypes.byref(n)))
        return regions[:n.value].copy(), zoom[:n.value].copy()

    def tune_begin(self, capacity):
        self._chk(self.L.az_tune_begin(self.h, int(capacity)))

    def tune_end(self):
        self._chk(self.L.az_tune_end(self.h))

    def tune_kth_largest(self, k):
        """(k-th largest pooled zoom score as float, number of pooled scores); -inf when <= k."""
        v = ctypes.c_float(0)
        n = ctypes.c_longlong(0)
        self._chk(self.L.az_tune_kth_largest(self.h, int(k), ctypes.byref(v), ctypes.byref(n)))
        return float(v.value), int(n.value)

    def tune_top(self, k):
        cap = int(k) + 65536
        while True:
            out = np.empty((cap,), dtype=np.float32)
            n = ctypes.c_longlong(0)
            rc = self.L.az_tune_top(self.h, int(k), _p(out, ctypes.c_float), cap, ctypes.byref(n))
            if rc == AZ_ERR_CAPACITY and n.value > cap:
                cap = int(n.value)
                continue
            self._chk(rc)
            return out[:n.value].copy()

    def tune_push(self, scores):
        a = _f32(scores).ravel()
        self._chk(self.L.az_tune_push(self.h, _p(a, ctypes.c_float), a.size))

    # ---- recall evaluation -------------------------------------------------------------
    def bbox_overlaps(self, boxes, query_boxes):
        b = _f64(boxes).reshape(-1, 4)
        q = _f64(query_boxes).reshape(-1, 4)
        out = np.zeros((b.shape[0], q.shape[0]), dtype=np.float64)
        self._chk(self.L.az_bbox_overlaps(self.h, _p(b, ctypes.c_double), b.shape[0], _p(q, ctypes.c_double),
                                          q.shape[0], _p(out, ctypes.c_double)))
        return out

    def recall_match(self, boxes_list, gt_list):
        """Per-image greedy matching of imdb.evaluate_recall for lists of [n_i,4] candidate and
        [k_i,4] ground-truth boxes -> concatenated gt overlaps (image order, then pick order)."""
        assert len(boxes_list) == len(gt_list)
        n = len(boxes_list)
        boff = np.zeros(n + 1, dtype=np.int32)
        goff = np.zeros(n + 1, dtype=np.int32)
        for i in range(n):
            boff[i + 1] = boff[i] + boxes_list[i].shape[0]
            goff[i + 1] = goff[i] + gt_list[i].shape[0]
        b = _f64(np.vstack([np.zeros((0, 4))] + [x.reshape(-1, 4) for x in boxes_list]))
        g = _f64(np.vstack([np.zeros((0, 4))] + [x.reshape(-1, 4) for x in gt_list]))
        out = np.zeros((int(goff[n]),), dtype=np.float64)
        self._chk(self.L.az_recall_match(self.h, n, _p(b, ctypes.c_double), _p(boff, ctypes.c_int32),
                                         _p(g, ctypes.c_double), _p(goff, ctypes.c_int32), _p(out, ctypes.c_double)))
        return out

    # ---- training data layer (lib/az_data_layer/roidb.py) ------------------------------------
    def zoom_labels(self, rois, gt, max_area_ratio, min_obj):
        """_compute_zoom_labels (roidb.py:313-341): bool [R]."""
        r = _f64(rois).reshape(-1, 4)
        g = _f64(gt).reshape(-1, 4)
        out = np.zeros((r.shape[0],), dtype=np.uint8)
        self._chk(self.L.az_zoom_labels(self.h, _p(r, ctypes.c_double), r.shape[0], _p(g, ctypes.c_double), g.shape[0],
                                        float(max_area_ratio), float(min_obj), _p(out, ctypes.c_uint8)))
        return out.astype(bool)

    @staticmethod
    def _offsets(arrays):
        off = np.zeros(len(arrays) + 1, dtype=np.int32)
        if len(arrays):
            off[1:] = np.cumsum([a.shape[0] for a in arrays])
        return off

    def train_ex_rois(self, tp, sizes, gt_list, noise, cap=None):
        """az_train_ex_rois: example regions and zoom labels of len(sizes) images, consuming `noise` (uniform doubles)
        as one stream.  Returns (ex_boxes f32 [E,4], zoom u8 [E], ex_off int32 [n+1], noise_used int64 [n]).
        Raises AzError(AZ_ERR_CAPACITY) with `.needed` = the doubles needed where the noise ran out; with an explicit
        `cap` that is too small, the same with `.needed_cap` (cap=None grows the buffer and calls again)."""
        p = make_train_params(tp)
        n = len(sizes)
        sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(-1, 2))
        gts = [_f64(g).reshape(-1, 4) for g in gt_list]
        assert len(gts) == n
        goff = self._offsets(gts)
        g = _f64(np.vstack([np.zeros((0, 4))] + gts))
        nz = _f64(noise).ravel()
        grow = cap is None
        cap = int(cap) if cap is not None else max(1024, 8192 * n)
        while True:
            ex = np.zeros((cap, 4), dtype=np.float32)
            zoom = np.zeros((cap,), dtype=np.uint8)
            eoff = np.zeros(n + 1, dtype=np.int32)
            used = np.zeros(max(n, 1), dtype=np.int64)
            need = np.zeros(2, dtype=np.int64)
            rc = self.L.az_train_ex_rois(self.h, ctypes.byref(p), n, _p(sz, ctypes.c_int32), _p(g, ctypes.c_double),
                                         _p(goff, ctypes.c_int32), _p(nz, ctypes.c_double), nz.size,
                                         _p(ex, ctypes.c_float), _p(zoom, ctypes.c_uint8), _p(eoff, ctypes.c_int32), cap,
                                         _p(used, ctypes.c_longlong), _p(need, ctypes.c_longlong))
            if rc == AZ_ERR_CAPACITY and (need[0] or need[1]):
                if need[1] and grow:
                    cap = int(need[1])
                    continue
                e = AzError(rc, self.L.az_last_error(self.h).decode())
                if need[0]:
                    e.needed = int(need[0])
                else:
                    e.needed_cap = int(need[1])
                raise e
            self._chk(rc)
            E = int(eoff[n])
            return ex[:E], zoom[:E], eoff, used[:n]

    def train_adj_targets(self, tp, ex_boxes, ex_off, gt_list, cap=None):
        """az_train_adj_targets: ex_boxes f32 [E,4] with ex_off [n+1], gt_list of n f32 [.,4] arrays ->
        (targets f64 [T,7] un-normalised, tgt_off int32 [n+1]).  An explicit `cap` that is too small raises
        AzError(AZ_ERR_CAPACITY) with `.needed_cap`."""
        p = make_train_params(tp)
        ex = _f32(ex_boxes).reshape(-1, 4)
        eoff = np.ascontiguousarray(ex_off, dtype=np.int32).ravel()
        n = eoff.size - 1
        gts = [_f32(g).reshape(-1, 4) for g in gt_list]
        assert len(gts) == n and int(eoff[n]) == ex.shape[0]
        goff = self._offsets(gts)
        g = _f32(np.vstack([np.zeros((0, 4), np.float32)] + gts))
        grow = cap is None
        cap = int(cap) if cap is not None else max(1024, ex.shape[0])
        while True:
            t = np.zeros((cap, 7), dtype=np.float64)
            toff = np.zeros(n + 1, dtype=np.int32)
            rc = self.L.az_train_adj_targets(self.h, ctypes.byref(p), n, _p(ex, ctypes.c_float), _p(eoff, ctypes.c_int32),
                                             _p(g, ctypes.c_float), _p(goff, ctypes.c_int32), _p(t, ctypes.c_double),
                                             _p(toff, ctypes.c_int32), cap)
            if rc == AZ_ERR_CAPACITY and int(toff[n]) > cap:
                if grow:
                    cap = int(toff[n])
                    continue
                e = AzError(rc, self.L.az_last_error(self.h).decode())
                e.needed_cap = int(toff[n])
                raise e
            self._chk(rc)
            return t[:int(toff[n])], toff

    def train_target_stats(self, n_sub, eps, targets, normalise=True):
        """az_train_target_stats over targets f64 [T,7] (C-contiguous; normalised IN PLACE when asked) ->
        (means [n_sub,4], stds [n_sub,4])."""
        assert targets.dtype == np.float64 and targets.flags["C_CONTIGUOUS"] and (targets.ndim == 2 and targets.shape[1] == 7)
        means = np.zeros((int(n_sub), 4), dtype=np.float64)
        stds = np.zeros((int(n_sub), 4), dtype=np.float64)
        self._chk(self.L.az_train_target_stats(self.h, int(n_sub), float(eps), _p(targets, ctypes.c_double),
                                               targets.shape[0], _p(means, ctypes.c_double), _p(stds, ctypes.c_double),
                                               1 if normalise else 0))
        return means, stds

    def det_targets(self, ex_boxes, ex_off, gt_list, label_list, bbox_thresh, bg_thresh_lo, eps):
        """az_det_targets: ex_boxes f32 [E,4] with ex_off [n+1], gt_list of n f32 [.,4] arrays and label_list of n integer
        arrays -> (targets f32 [E,5] un-normalised, max_overlaps f64 [E])."""
        ex = _f32(ex_boxes).reshape(-1, 4)
        eoff = np.ascontiguousarray(ex_off, dtype=np.int32).ravel()
        n = eoff.size - 1
        gts = [_f32(g).reshape(-1, 4) for g in gt_list]
        labs = [np.asarray(l).astype(np.int32).ravel() for l in label_list]
        assert len(gts) == n and len(labs) == n and int(eoff[n]) == ex.shape[0]
        assert all(g.shape[0] == l.size for g, l in zip(gts, labs))
        goff = self._offsets(gts)
        g = _f32(np.vstack([np.zeros((0, 4), np.float32)] + gts))
        lab = np.ascontiguousarray(np.concatenate([np.zeros(0, np.int32)] + labs), dtype=np.int32)
        t = np.zeros((ex.shape[0], 5), dtype=np.float32)
        mo = np.zeros(ex.shape[0], dtype=np.float64)
        self._chk(self.L.az_det_targets(self.h, n, _p(ex, ctypes.c_float), _p(eoff, ctypes.c_int32), _p(g, ctypes.c_float),
                                        _p(lab, ctypes.c_int32), _p(goff, ctypes.c_int32), float(bbox_thresh), float(bg_thresh_lo),
                                        float(eps), _p(t, ctypes.c_float), _p(mo, ctypes.c_double)))
        return t, mo

    def det_target_stats(self, targets, ex_off, num_classes, eps, normalise=True):
        """az_det_target_stats over targets f32 [E,5] (C-contiguous; normalised IN PLACE when asked) with ex_off [n+1] ->
        (counts [num_classes], means [num_classes,4], stds [num_classes,4])."""
        assert targets.dtype == np.float32 and targets.flags["C_CONTIGUOUS"] and (targets.ndim == 2 and targets.shape[1] == 5)
        eoff = np.ascontiguousarray(ex_off, dtype=np.int32).ravel()
        assert int(eoff[-1]) == targets.shape[0]
        K = int(num_classes)
        counts = np.zeros(K, dtype=np.float64)
        means = np.zeros((K, 4), dtype=np.float64)
        stds = np.zeros((K, 4), dtype=np.float64)
        self._chk(self.L.az_det_target_stats(self.h, eoff.size - 1, _p(targets, ctypes.c_float), _p(eoff, ctypes.c_int32), K, float(eps),
                                             1 if normalise else 0, _p(counts, ctypes.c_double), _p(means, ctypes.c_double),
                                             _p(stds, ctypes.c_double)))
        return counts, means, stds

    # ---- detection evaluation (imdb.evaluate_detections, VOC) -------------------------------
    def voc_eval(self, n_classes, n_images, det_box, det_conf, det_off, gt_box, gt_difficult, gt_off,
                 min_overlap=0.5, metric_07=True, want_curves=True):
        """az_voc_eval: VOCevaldet + xVOCap for every class at once.  Segment
        s = c*n_images + i owns det_box[det_off[s]:det_off[s+1]] ([D,4] 1-based, results-file
        values) with det_conf, and gt_box[gt_off[s]:gt_off[s+1]] ([G,4] 1-based) with gt_difficult.
        Returns a dict: npos [C] int64, ap [C], ap_auc [C]; with want_curves also match [D] int8
        (input order: 1 TP, -1 FP, 0 ignored) and rec / prec [D] (each class's rank order)."""
        bx = _f64(det_box).reshape(-1, 4)
        cf = _f64(det_conf).ravel()
        doff = np.ascontiguousarray(det_off, dtype=np.int32).ravel()
        gb = _f64(gt_box).reshape(-1, 4)
        gd = np.ascontiguousarray(gt_difficult, dtype=np.uint8).ravel()
        goff = np.ascontiguousarray(gt_off, dtype=np.int32).ravel()
        nseg = int(n_classes) * int(n_images)
        if doff.size != nseg + 1 or goff.size != nseg + 1:
            raise AzError(AZ_ERR_INVALID, "voc_eval: offsets need n_classes*n_images+1 entries")
        D, G = int(doff[-1]), int(goff[-1])
        if bx.shape[0] != D or cf.size != D or gb.shape[0] != G or gd.size != G:
            raise AzError(AZ_ERR_INVALID, "voc_eval: array sizes disagree with the offsets")
        out = {"npos": np.zeros(n_classes, np.int64), "ap": np.zeros(n_classes, np.float64),
               "ap_auc": np.zeros(n_classes, np.float64)}
        mp = rp = pp = None
        if want_curves:
            out["match"] = np.zeros(D, np.int8)
            out["rec"] = np.zeros(D, np.float64)
            out["prec"] = np.zeros(D, np.float64)
            mp = _p(out["match"], ctypes.c_int8)
            rp, pp = _p(out["rec"], ctypes.c_double), _p(out["prec"], ctypes.c_double)
        self._chk(self.L.az_voc_eval(self.h, int(n_classes), int(n_images), _p(bx, ctypes.c_double),
                                     _p(cf, ctypes.c_double), _p(doff, ctypes.c_int32), _p(gb, ctypes.c_double),
                                     _p(gd, ctypes.c_uint8), _p(goff, ctypes.c_int32), float(min_overlap),
                                     1 if metric_07 else 0, mp, rp, pp, _p(out["npos"], ctypes.c_int64),
                                     _p(out["ap"], ctypes.c_double), _p(out["ap_auc"], ctypes.c_double)))
        return out

    def rank_unit(self, n_classes, n_images, score, det_off):
        """az_rank_unit (tests): the evaluations' shared ranking alone -> (by_seg, by_class), uint32 [D] each."""
        sc = _f64(score).ravel()
        doff = np.ascontiguousarray(det_off, dtype=np.int32).ravel()
        if doff.size != int(n_classes) * int(n_images) + 1 or sc.size != int(doff[-1]):
            raise AzError(AZ_ERR_INVALID, "rank_unit: array sizes disagree with the offsets")
        by_seg, by_class = np.zeros(sc.size, np.uint32), np.zeros(sc.size, np.uint32)
        self._chk(self.L.az_rank_unit(self.h, int(n_classes), int(n_images), _p(sc, ctypes.c_double), _p(doff, ctypes.c_int32),
                                      _p(by_seg, ctypes.c_uint32), _p(by_class, ctypes.c_uint32)))
        return by_seg, by_class

    def coco_eval(self, n_classes, n_images, det_box, det_score, det_off, gt_box, gt_area, gt_crowd, gt_off,
                  want_matches=False):
        """az_coco_eval: COCOeval evaluate + accumulate + summarize, iouType 'bbox' (DESIGN §1c), for every category
        at once.  Segment s = k*n_images + i owns det_box[det_off[s]:det_off[s+1]] ([D,4] xywh, file order) with
        det_score, and gt_box[gt_off[s]:gt_off[s+1]] ([G,4] xywh) with gt_area and gt_crowd.  Returns a dict:
        precision [10,101,K,4,3], recall [10,K,4,3], stats [12]; with want_matches also dt_match [4,10,D] int32 (the
        matched box's position in its segment, -1 none) and dt_ignore [4,10,D] int8 (-1: past the first 100)."""
        bx = _f64(det_box).reshape(-1, 4)
        sc = _f64(det_score).ravel()
        doff = np.ascontiguousarray(det_off, dtype=np.int32).ravel()
        gb = _f64(gt_box).reshape(-1, 4)
        ga = _f64(gt_area).ravel()
        gc = np.ascontiguousarray(gt_crowd, dtype=np.uint8).ravel()
        goff = np.ascontiguousarray(gt_off, dtype=np.int32).ravel()
        K = int(n_classes)
        nseg = K * int(n_images)
        if doff.size != nseg + 1 or goff.size != nseg + 1:
            raise AzError(AZ_ERR_INVALID, "coco_eval: offsets need n_classes*n_images+1 entries")
        D, G = int(doff[-1]), int(goff[-1])
        if bx.shape[0] != D or sc.size != D or gb.shape[0] != G or ga.size != G or gc.size != G:
            raise AzError(AZ_ERR_INVALID, "coco_eval: array sizes disagree with the offsets")
        out = {"precision": np.zeros((10, 101, K, 4, 3)), "recall": np.zeros((10, K, 4, 3)), "stats": np.zeros(12)}
        mp = ip_ = None
        if want_matches:
            out["dt_match"] = np.zeros((4, 10, D), np.int32)
            out["dt_ignore"] = np.zeros((4, 10, D), np.int8)
            mp, ip_ = _p(out["dt_match"], ctypes.c_int32), _p(out["dt_ignore"], ctypes.c_int8)
        self._chk(self.L.az_coco_eval(self.h, K, int(n_images), _p(bx, ctypes.c_double), _p(sc, ctypes.c_double),
                                      _p(doff, ctypes.c_int32), _p(gb, ctypes.c_double), _p(ga, ctypes.c_double),
                                      _p(gc, ctypes.c_uint8), _p(goff, ctypes.c_int32),
                                      _p(out["precision"], ctypes.c_double), _p(out["recall"], ctypes.c_double),
                                      _p(out["stats"], ctypes.c_double), mp, ip_))
        return out

    # ---- proposal diagnosis (what tune.py:368-419 records AZ_results.mat for) ----------------
    def diag_eval(self, anchors_list, zoom_list, level_list, gt_list, props_list, tz, emb_reg_thresh, emb_obj_thresh,
                  iou_thresh=0.5, cuts=(10, 50, 100, 300, 1000, 2000), area_edges=(32 ** 2, 96 ** 2), want_kernel_ms=False):
        """az_diag_eval ("Proposal diagnosis") for a whole image set at once: per image [m_i,4] anchors with their zoom scores
        (f32) and search levels, [k_i,4] objects and [n_i,4] proposals in rank order.  Returns a dict: anchor_label [A]
        u8, level_table [AZ_MAX_LEVELS,4] int64 (anchors, zoomed, labelled, both), best_iou [G] f64, best_rank /
        first_hit / deepest_level [G] int32, recall_table [len(cuts)+1,4] int64 (all / small / medium / large; the
        last row counts every object), the three offset arrays, and with want_kernel_ms the kernels' device time."""
        n = len(anchors_list)
        assert len(zoom_list) == n and len(level_list) == n and len(gt_list) == n and len(props_list) == n
        aoff, goff, poff = self._offsets(anchors_list), self._offsets(gt_list), self._offsets(props_list)
        a = _f64(np.vstack([np.zeros((0, 4))] + [np.asarray(x).reshape(-1, 4) for x in anchors_list]))
        g = _f64(np.vstack([np.zeros((0, 4))] + [np.asarray(x).reshape(-1, 4) for x in gt_list]))
        p = _f64(np.vstack([np.zeros((0, 4))] + [np.asarray(x).reshape(-1, 4) for x in props_list]))
        z = _f32(np.concatenate([np.zeros(0, np.float32)] + [np.asarray(x, dtype=np.float32).ravel() for x in zoom_list]))
        lv = np.ascontiguousarray(np.concatenate([np.zeros(0, np.int32)] + [np.asarray(x).ravel() for x in level_list]),
                                  dtype=np.int32)
        if z.size != a.shape[0] or lv.size != a.shape[0]:
            raise AzError(AZ_ERR_INVALID, "diag_eval: zoom scores / levels disagree with the anchors")
        return self.diag_eval_packed(a, z, lv, aoff, g, goff, p, poff, tz, emb_reg_thresh, emb_obj_thresh, iou_thresh, cuts,
                                     area_edges, want_kernel_ms=want_kernel_ms)

    def diag_eval_packed(self, anchors, zoom, level, anc_off, gt, gt_off, props, prop_off, tz, emb_reg_thresh,
                         emb_obj_thresh, iou_thresh, cuts, area_edges, want_kernel_ms=False, counts=None, out=None):
        """az_diag_eval on arrays that are packed already (what diag_eval builds).  counts: (n_anchors, n_gt, n_props)
        when they are not to be taken from the arrays; out: a dict of preallocated outputs to fill instead of new ones."""
        a, g, p = _f64(anchors).reshape(-1, 4), _f64(gt).reshape(-1, 4), _f64(props).reshape(-1, 4)
        z = _f32(zoom).ravel()
        lv = np.ascontiguousarray(level, dtype=np.int32).ravel()
        aoff, goff, poff = (np.ascontiguousarray(o, dtype=np.int32).ravel() for o in (anc_off, gt_off, prop_off))
        n = aoff.size - 1
        if n < 0 or goff.size != n + 1 or poff.size != n + 1:
            raise AzError(AZ_ERR_INVALID, "diag_eval: the three offset arrays need n_images+1 entries each")
        A, G, P = counts if counts is not None else (a.shape[0], g.shape[0], p.shape[0])
        ct = np.ascontiguousarray(cuts, dtype=np.int32).ravel()
        ed = _f64(area_edges).ravel()
        if ed.size != 2:
            raise AzError(AZ_ERR_INVALID, "diag_eval: area_edges needs two entries")
        if out is None:
            out = {"anchor_label": np.zeros(a.shape[0], np.uint8), "level_table": np.zeros((AZ_MAX_LEVELS, 4), np.int64),
                   "best_iou": np.zeros(g.shape[0], np.float64), "best_rank": np.zeros(g.shape[0], np.int32),
                   "first_hit": np.zeros(g.shape[0], np.int32), "deepest_level": np.zeros(g.shape[0], np.int32),
                   "recall_table": np.zeros((ct.size + 1, 4), np.int64)}
        ms = ctypes.c_float(0.0)
        self._chk(self.L.az_diag_eval(
            self.h, n, _p(a, ctypes.c_double), _p(z, ctypes.c_float), _p(lv, ctypes.c_int32), _p(aoff, ctypes.c_int32), int(A),
            _p(g, ctypes.c_double), _p(goff, ctypes.c_int32), int(G), _p(p, ctypes.c_double), _p(poff, ctypes.c_int32), int(P),
            float(tz), float(emb_reg_thresh), float(emb_obj_thresh), float(iou_thresh), _p(ct, ctypes.c_int32), ct.size,
            _p(ed, ctypes.c_double), _p(out["anchor_label"], ctypes.c_uint8), _p(out["level_table"], ctypes.c_int64),
            _p(out["best_iou"], ctypes.c_double), _p(out["best_rank"], ctypes.c_int32), _p(out["first_hit"], ctypes.c_int32),
            _p(out["deepest_level"], ctypes.c_int32), _p(out["recall_table"], ctypes.c_int64),
            ctypes.byref(ms) if want_kernel_ms else None))
        out.update(anc_off=aoff, gt_off=goff, prop_off=poff, cuts=ct.copy())
        if want_kernel_ms:
            out["kernel_ms"] = float(ms.value)
        return out

    # ---- detection diagnosis (Hoiem et al. 2012 / TIDE 2020 on az_voc_eval's layout) ---------
    def det_diag_eval(self, n_classes, n_images, det_box, det_conf, det_off, gt_box, gt_difficult, gt_off,
                      min_overlap=0.5, bg_overlap=0.1, metric_07=True, class_group=None, cuts=(), want_kernel_ms=False):
        """az_det_diag_eval ("Detection diagnosis") on voc_eval's arguments, plus bg_overlap, class_group
        [C] int32 (None: every class its own group) and cuts (finite, ascending multiples of npos, at most 16).  Returns a
        dict: per detection in input order type [D] int8 (0 IGN, 1 TP, 2 DUP, 3 LOC, 4 SIM, 5 OTH, 6 BG), ov_same /
        ov_other [D] f64, arg_same / other_class [D] int32, loc_fixed [D] u8; gt_claim [G] int32; per class type_table
        [C,7], miss [C], fp_at [C,len(cuts),7], npos [C] int64 and ap_fix [C,8]; with want_kernel_ms the kernels'
        device time."""
        bx = _f64(det_box).reshape(-1, 4)
        cf = _f64(det_conf).ravel()
        doff = np.ascontiguousarray(det_off, dtype=np.int32).ravel()
        gb = _f64(gt_box).reshape(-1, 4)
        gd = np.ascontiguousarray(gt_difficult, dtype=np.uint8).ravel()
        goff = np.ascontiguousarray(gt_off, dtype=np.int32).ravel()
        C = int(n_classes)
        nseg = C * int(n_images)
        if doff.size != nseg + 1 or goff.size != nseg + 1:
            raise AzError(AZ_ERR_INVALID, "det_diag_eval: offsets need n_classes*n_images+1 entries")
        D, G = int(doff[-1]), int(goff[-1])
        if bx.shape[0] != D or cf.size != D or gb.shape[0] != G or gd.size != G:
            raise AzError(AZ_ERR_INVALID, "det_diag_eval: array sizes disagree with the offsets")
        grp = None
        if class_group is not None:
            grp = np.ascontiguousarray(class_group, dtype=np.int32).ravel()
            if grp.size != C:
                raise AzError(AZ_ERR_INVALID, "det_diag_eval: class_group needs n_classes entries")
        ct = _f64(cuts).ravel()
        if not np.isfinite(ct).all():
            raise AzError(AZ_ERR_INVALID, "det_diag_eval: the cuts must be finite")
        out = {"type": np.zeros(D, np.int8), "ov_same": np.zeros(D), "arg_same": np.zeros(D, np.int32),
               "ov_other": np.zeros(D), "other_class": np.zeros(D, np.int32), "loc_fixed": np.zeros(D, np.uint8),
               "gt_claim": np.zeros(G, np.int32), "type_table": np.zeros((C, 7), np.int64), "miss": np.zeros(C, np.int64),
               "fp_at": np.zeros((C, ct.size, 7), np.int64), "npos": np.zeros(C, np.int64), "ap_fix": np.zeros((C, 8))}
        ms = ctypes.c_float(0.0)
        i64 = ctypes.c_int64
        self._chk(self.L.az_det_diag_eval(
            self.h, C, int(n_images), _p(bx, ctypes.c_double), _p(cf, ctypes.c_double), _p(doff, ctypes.c_int32),
            _p(gb, ctypes.c_double), _p(gd, ctypes.c_uint8), _p(goff, ctypes.c_int32), float(min_overlap), float(bg_overlap),
            1 if metric_07 else 0, None if grp is None else _p(grp, ctypes.c_int32), _p(ct, ctypes.c_double), ct.size,
            _p(out["type"], ctypes.c_int8), _p(out["ov_same"], ctypes.c_double), _p(out["arg_same"], ctypes.c_int32),
            _p(out["ov_other"], ctypes.c_double), _p(out["other_class"], ctypes.c_int32), _p(out["loc_fixed"], ctypes.c_uint8),
            _p(out["gt_claim"], ctypes.c_int32), _p(out["type_table"], i64), _p(out["miss"], i64), _p(out["fp_at"], i64),
            _p(out["npos"], i64), _p(out["ap_fix"], ctypes.c_double), ctypes.byref(ms) if want_kernel_ms else None))
        out["cuts"] = ct.copy()
        if want_kernel_ms:
            out["kernel_ms"] = float(ms.value)
        return out

    def coco_diag_eval(self, n_classes, n_images, det_box, det_score, det_off, gt_box, gt_area, gt_crowd, gt_off,
                       bg_overlap=0.1, class_group=None, want_kernel_ms=False):
        """az_coco_diag_eval ("Detection diagnosis, COCO protocol") on coco_eval's arguments, plus bg_overlap
        (in [0, 0.5]) and class_group [K] int32 (None: every class its own group); area range all, maxDets 100, the ten
        thresholds.  Returns a dict: per detection in input order ov_same / ov_other [D] f64, arg_same / other_class [D]
        int32, type [10,D] int8 (-1 past the segment's first 100, 0 IGN, 1 TP, 2 DUP, 3 LOC, 4 SIM, 5 OTH, 6 BG),
        loc_fixed [10,D] u8; gt_claim [10,G] int32; per class npos [K], type_table [K,10,7], miss [K,10] int64; the
        curves prec_fix [8,10,101,K] and recall_fix [8,10,K] (variant 0 is coco_eval's precision[:, :, :, 0, 2]); and
        from them ap_fix [K,10,8] (the mean over recThrs of the entries > -1, NaN where none) and stats_fix [8,3]
        (AP, AP50, AP75 per variant by summarize's np.mean(s[s > -1]), -1 where none); with want_kernel_ms the
        kernels' device time."""
        bx = _f64(det_box).reshape(-1, 4)
        sc = _f64(det_score).ravel()
        doff = np.ascontiguousarray(det_off, dtype=np.int32).ravel()
        gb = _f64(gt_box).reshape(-1, 4)
        ga = _f64(gt_area).ravel()
        gc = np.ascontiguousarray(gt_crowd, dtype=np.uint8).ravel()
        goff = np.ascontiguousarray(gt_off, dtype=np.int32).ravel()
        K = int(n_classes)
        nseg = K * int(n_images)
        if doff.size != nseg + 1 or goff.size != nseg + 1:
            raise AzError(AZ_ERR_INVALID, "coco_diag_eval: offsets need n_classes*n_images+1 entries")
        D, G = int(doff[-1]), int(goff[-1])
        if bx.shape[0] != D or sc.size != D or gb.shape[0] != G or ga.size != G or gc.size != G:
            raise AzError(AZ_ERR_INVALID, "coco_diag_eval: array sizes disagree with the offsets")
        grp = None
        if class_group is not None:
            grp = np.ascontiguousarray(class_group, dtype=np.int32).ravel()
            if grp.size != K:
                raise AzError(AZ_ERR_INVALID, "coco_diag_eval: class_group needs n_classes entries")
        out = {"ov_same": np.zeros(D), "arg_same": np.zeros(D, np.int32), "ov_other": np.zeros(D),
               "other_class": np.zeros(D, np.int32), "type": np.zeros((10, D), np.int8), "loc_fixed": np.zeros((10, D), np.uint8),
               "gt_claim": np.zeros((10, G), np.int32), "npos": np.zeros(K, np.int64), "type_table": np.zeros((K, 10, 7), np.int64),
               "miss": np.zeros((K, 10), np.int64), "prec_fix": np.zeros((8, 10, 101, K)), "recall_fix": np.zeros((8, 10, K))}
        ms = ctypes.c_float(0.0)
        i64 = ctypes.c_int64
        self._chk(self.L.az_coco_diag_eval(
            self.h, K, int(n_images), _p(bx, ctypes.c_double), _p(sc, ctypes.c_double), _p(doff, ctypes.c_int32),
            _p(gb, ctypes.c_double), _p(ga, ctypes.c_double), _p(gc, ctypes.c_uint8), _p(goff, ctypes.c_int32),
            float(bg_overlap), None if grp is None else _p(grp, ctypes.c_int32), _p(out["ov_same"], ctypes.c_double),
            _p(out["arg_same"], ctypes.c_int32), _p(out["ov_other"], ctypes.c_double), _p(out["other_class"], ctypes.c_int32),
            _p(out["type"], ctypes.c_int8), _p(out["loc_fixed"], ctypes.c_uint8), _p(out["gt_claim"], ctypes.c_int32),
            _p(out["npos"], i64), _p(out["type_table"], i64), _p(out["miss"], i64), _p(out["prec_fix"], ctypes.c_double),
            _p(out["recall_fix"], ctypes.c_double), ctypes.byref(ms) if want_kernel_ms else None))
        out.update(coco_diag_means(out["prec_fix"]))
        if want_kernel_ms:
            out["kernel_ms"] = float(ms.value)
        return out

    # ---- image front-end ---------------------------------------------------------------
    def image_blob_size(self, h, w, scale):
        oh, ow = ctypes.c_int(0), ctypes.c_int(0)
        rc = self.L.az_image_blob_size(int(h), int(w), float(scale), ctypes.byref(oh), ctypes.byref(ow))
        if rc != AZ_OK:
            raise AzError(rc, "az_image_blob_size: bad arguments")
        return oh.value, ow.value

    def image_blob(self, im, means, scale, out=None, stream=None):
        """uint8 BGR HWC image -> [1,3,oh,ow] f32 blob (mean-subtracted, cv2-style bilinear).
        out: None -> NumPy array; a CUDA torch tensor of the right shape -> filled in place.
        stream (with a tensor `out`): a raw hipStream_t handle, e.g. torch.cuda.current_stream().cuda_stream -- upload and
        kernel are only ENQUEUED there (az_image_blob_dev_on), ordered with whatever that stream runs next."""
        im = np.ascontiguousarray(im, dtype=np.uint8)
        assert im.ndim == 3 and im.shape[2] == 3
        h, w = im.shape[:2]
        oh, ow = self.image_blob_size(h, w, scale)
        m = _f32(np.asarray(means).ravel())
        assert m.size == 3
        if out is None:
            blob = np.empty((1, 3, oh, ow), dtype=np.float32)
            self._chk(self.L.az_image_blob_host(self.h, _p(im, ctypes.c_uint8), h, w, _p(m, ctypes.c_float),
                                                float(scale), _p(blob, ctypes.c_float), oh, ow))
            return blob
        assert tuple(out.shape[-3:]) == (3, oh, ow) and out.is_contiguous() and out.is_cuda
        if stream is not None:
            # (torch's default stream has the handle 0, which az_image_blob_dev_on reads as "the ctx stream": the default
            #  stream is named explicitly -- hipStreamLegacy, (hipStream_t)1 -- or the upload and the front-end kernel would
            #  run on another stream than the backbone that reads the blob)
            sh = int(stream) or 1
            self._chk(self.L.az_image_blob_dev_on(self.h, _p(im, ctypes.c_uint8), h, w, _p(m, ctypes.c_float), float(scale),
                                                  ctypes.c_void_p(out.data_ptr()), oh, ow, ctypes.c_void_p(sh)))
            return out
        self._chk(self.L.az_image_blob_dev(self.h, _p(im, ctypes.c_uint8), h, w, _p(m, ctypes.c_float),
                                           float(scale), ctypes.c_void_p(out.data_ptr()), oh, ow))
        return out

    # ---- measurement -----------------------------------------------------------------
    def set_profiling(self, mode):
        """mode bits: 1 = fc GEMM launches only, 2 = every launch group, 4 = accumulate across
        calls until read; 0 = off."""
        self._chk(self.L.az_set_profiling(self.h, int(mode)))

    def set_graphs(self, on):
        """Replay the search's launch sequence as a hipGraph (same results, less host time)."""
        self._chk(self.L.az_set_graphs(self.h, 1 if on else 0))

    # the round-3 profile's figures for the full head on one MI355X box: what tests pin the form choice to
    REFERENCE_PASS_COSTS = ((40, 142.0), (704, 1096.0))

    def set_pass_costs(self, table=None):
        """table: ((rows, us), ...) ascending, 2..6 points -- the cost of one head pass the context chooses the search
        form by (az_set_pass_costs); None / () = measure on the device at the next launch (the default)."""
        t = list(table or ())
        rows = np.ascontiguousarray([r for r, _ in t], dtype=np.int32)
        us = np.ascontiguousarray([u for _, u in t], dtype=np.float64)
        self._chk(self.L.az_set_pass_costs(self.h, len(t), _p(rows, ctypes.c_int32) if t else None,
                                           _p(us, ctypes.c_double) if t else None))

    def pass_costs(self):
        """((rows, us), ...) in use; () before the first launch of a context that measures its own."""
        rows = np.zeros(8, dtype=np.int32)
        us = np.zeros(8, dtype=np.float64)
        n = ctypes.c_int(0)
        self._chk(self.L.az_get_pass_costs(self.h, _p(rows, ctypes.c_int32), _p(us, ctypes.c_double), 8, ctypes.byref(n)))
        return tuple((int(rows[i]), float(us[i])) for i in range(n.value))

    def measure_box(self):
        """(fp32 MFMA TFLOP/s this box sustains in a register-only loop, TB/s of a 1 GiB float4 copy) -- az_measure_box."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        self._chk(self.L.az_measure_box(self.h, ctypes.byref(a), ctypes.byref(b)))
        return float(a.value), float(b.value)

    def last_kernel_times(self, cap=65536):
        names = ctypes.create_string_buffer(32 * cap)
        ms = np.zeros(cap, dtype=np.float32)
        lv = np.zeros(cap, dtype=np.int32)
        n = ctypes.c_int(0)
        self._chk(self.L.az_last_kernel_times(self.h, names, _p(ms, ctypes.c_float), _p(lv, ctypes.c_int32),
                                              cap, ctypes.byref(n)))
        out = []
        for i in range(min(n.value, cap)):
            nm = names.raw[32 * i:32 * i + 32].split(b"\0", 1)[0].decode()
            out.append((nm, int(lv[i]), float(ms[i])))
        return out

    def stream_handle(self):
        return self.L.az_stream(self.h)


_default_ctx = None


HEAD_KEYS = ("W6", "b6", "W71", "b71", "W72", "b72", "Was", "bas", "Wab", "bab", "Wz", "bz")


def dropout_mask(seed, iteration, layer, n, ratio=0.5):
    """The NumPy form of the trainer's dropout mask (include/aznet_hip.h, az_solver_step): keep flags (uint8) of the elements
    0 .. n-1 of layer 0 / 1 / 2 (int6, int7_1, int7_2) at (seed, iteration).  The trainer holds the ratio as a float32
    and thresholds at (unsigned)((double)ratio_f32 * 2^24): the ratio is rounded to float32 here first (0.3 -> 5033165)."""
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    G = 0x9E3779B97F4A7C15
    key = mix((mix((mix((int(seed) + G) & M) + int(iteration)) & M) + int(layer)) & M)
    with np.errstate(over="ignore"):
        z = np.uint64(key) + np.uint64(G) * (np.arange(n, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)) >= np.uint64(int(float(np.float32(ratio)) * 16777216.0))).astype(np.uint8)


def sgd_update_numpy(w, g, hist, rate, momentum, decay, clip_scale):
    """The NumPy form of az_sgd_update / az_solver_update for one blob (float32, one rounding per operation; rate and decay
    already carry lr_mult / decay_mult): returns (w, hist) after the step."""
    f = np.float32
    gg = g.astype(f) * f(clip_scale)
    gg = gg + f(decay) * w
    h = f(momentum) * hist + f(rate) * gg
    return w - h, h


def bf16_round(x):
    """x (float32) with every element rounded to the nearest bfloat16, ties to even, as float32: what AZ_TRAIN_BF16 does to
    the operands of a matrix product.  Overflow goes to inf; NaN stays NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)).view(np.float32)
    return np.where(np.isnan(x), x, r).astype(np.float32)


class _Trainer(object):
    """What the two trainers behind conv5_3 share: the handle, the parameters and hyper-parameters, the map / roi arguments
    of a pass, `update` and the debug `fetch`.  A subclass names its C prefix, its parameters in the ABI's order, how many
    dropout ratios it has and which saved tensors are not float32, sets `dims` and calls `_create`."""
    _C = None               # "az_solver" / "az_det_solver"
    KEYS = ()
    _NDROP = 0
    _U8, _I32, _F64 = (), ("argmax",), ()
    _ROWS49 = ()            # saved tensors whose rows are (roi, bin)
    _FLAT = ()              # saved tensors that are not one row per row of the last pass: returned as they come

    def _fn(self, name):
        return getattr(self.L, self._C + "_" + name)

    def _create(self, ctx, sizes, max_rois, seed, head):
        self.ctx, self.L = ctx, ctx.L
        h = ctypes.c_void_p()
        ctx._chk(self._fn("create")(ctx.h, *([int(x) for x in sizes] + [int(max_rois), int(seed) & ((1 << 64) - 1), ctypes.byref(h)])))
        self.h = h
        self.max_rois = int(max_rois)
        self.last_rows = 0
        if head is not None:
            self.load(head)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self._fn("destroy")(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, head):
        """head: {name: Caffe-layout array} for any subset of KEYS."""
        shp = self._shapes()
        arrs = [_f32(head[k]).reshape(shp[k]) if k in head else None for k in self.KEYS]
        self.ctx._chk(self._fn("load")(self.h, *[_p(a, ctypes.c_float) if a is not None else None for a in arrs]))

    def read(self):
        shp = self._shapes()
        out = {k: np.empty(shp[k], dtype=np.float32) for k in self.KEYS}
        self.ctx._chk(self._fn("read")(self.h, *[_p(out[k], ctypes.c_float) for k in self.KEYS]))
        return out

    def set_hyper(self, lr_mult=None, decay_mult=None, dropout_ratio=None):
        arrs = [None if v is None else _f32(v).reshape(n)
                for v, n in ((lr_mult, len(self.KEYS)), (decay_mult, len(self.KEYS)), (dropout_ratio, self._NDROP))]
        self.ctx._chk(self._fn("set_hyper")(self.h, *[None if a is None else _p(a, ctypes.c_float) for a in arrs]))

    def set_precision(self, precision):
        """AZ_TRAIN_FP32 (0) or AZ_TRAIN_BF16 (1): the operands of every matrix product from the next step on (*_set_precision)."""
        self.ctx._chk(self._fn("set_precision")(self.h, int(precision)))

    def set_accumulate(self, on):
        """0: a step overwrites the parameter gradients (the default); 1: every following step adds to them, one float32
        add per element (*_set_accumulate; Caffe's iter_size)."""
        self.ctx._chk(self._fn("set_accumulate")(self.h, int(on)))

    def load_history(self, hist):
        """hist: {name: Caffe-layout array} of momentum history for any subset of KEYS; the rest keeps what it holds."""
        shp = self._shapes()
        arrs = [_f32(hist[k]).reshape(shp[k]) if k in hist else None for k in self.KEYS]
        self.ctx._chk(self._fn("load_history")(self.h, *[_p(a, ctypes.c_float) if a is not None else None for a in arrs]))

    def read_history(self):
        """The momentum history of every parameter in KEYS, shaped as `read` shapes the weights."""
        return {k: self.fetch("h_" + k) for k in self.KEYS}

    def _map(self, conv):
        """(pointer, N, H, W, channels_last) of a float32 CUDA tensor [N,C,H,W] in either memory format."""
        import torch
        assert conv.is_cuda and conv.dtype == torch.float32 and conv.dim() == 4 and conv.shape[1] == self.dims["C"]
        N, _, H, W = (int(x) for x in conv.shape)
        if conv.is_contiguous():
            cl = 0
        elif conv.is_contiguous(memory_format=torch.channels_last):
            cl = 1
        else:
            raise AzError(AZ_ERR_INVALID, "conv5_3 must be contiguous or channels_last")
        return ctypes.c_void_p(conv.data_ptr()), N, H, W, cl

    def _pass_args(self, conv, rois, dmap=None):
        """The leading arguments of *_step / *_forward_test (map, rois [R,5], R), the rois array that backs them, and the
        pointer of dmap (None, or a CUDA tensor of conv's shape and memory format); waits for conv's stream."""
        import torch
        ptr, N, H, W, cl = self._map(conv)
        rois = _f32(rois).reshape(-1, 5)
        dptr = None
        if dmap is not None:
            assert dmap.is_cuda and dmap.dtype == conv.dtype and dmap.shape == conv.shape and dmap.stride() == conv.stride()
            dptr = ctypes.c_void_p(dmap.data_ptr())
        torch.cuda.current_stream(conv.device).synchronize()
        return (ptr, N, H, W, cl, _p(rois, ctypes.c_float), rois.shape[0]), rois, dptr

    def _step(self, fn, lead, targets, seed, iteration, nloss, dptr):
        """fn(handle, lead ..., targets ..., seed, iteration, losses, sumsq, dptr): (losses f32 [nloss], sum of squares)."""
        losses = np.zeros(nloss, dtype=np.float32)
        sq = ctypes.c_double(0.0)
        f = ctypes.c_float
        self.ctx._chk(fn(self.h, *(list(lead) + [_p(t, f) for t in targets] +
                                   [int(seed) & ((1 << 64) - 1), int(iteration), _p(losses, f), ctypes.byref(sq), dptr])))
        self.last_rows = lead[-1]
        return losses, float(sq.value)

    def _forward(self, fn, lead, outs):
        """fn(handle, lead ..., outs ...): the filled float32 arrays `outs`."""
        self.ctx._chk(fn(self.h, *(list(lead) + [_p(o, ctypes.c_float) for o in outs])))
        self.last_rows = lead[-1]
        return outs

    def update(self, rate, momentum, weight_decay, clip_scale=1.0):
        self.ctx._chk(self._fn("update")(self.h, float(rate), float(momentum), float(weight_decay), float(clip_scale)))

    def fetch(self, name):
        """A saved tensor of the last pass by name (*_fetch), shaped."""
        fn = self._fn("fetch")
        n = ctypes.c_longlong(0)
        self.ctx._chk(fn(self.h, name.encode(), None, 0, ctypes.byref(n)))
        dt = (np.uint8 if name in self._U8 else np.int32 if name in self._I32 else np.float64 if name in self._F64 else np.float32)
        out = np.empty(n.value // np.dtype(dt).itemsize, dtype=dt)
        self.ctx._chk(fn(self.h, name.encode(), out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        if name in self._FLAT:
            return out
        shp = self._shapes()
        if len(name) > 2 and name[1] == "_" and name[2:] in shp:
            return out.reshape(shp[name[2:]])
        rows = self.last_rows * (49 if name in self._ROWS49 else 1)
        return out.reshape(rows, -1) if rows else out


class AzSolver(_Trainer):
    """The AZ-net trainer behind conv5_3 (az_solver_*): fp32 master weights, gradients and momentum history of the head in
    HBM; one `step` is forward + backward of a minibatch, `update` Caffe's SGD step."""
    _C, KEYS, _NDROP, _U8 = "az_solver", HEAD_KEYS, 3, ("mask6", "mask71", "mask72")

    def __init__(self, ctx, C, n6, n71, n72, max_rois=256, seed=0, head=None):
        self.dims = dict(C=int(C), n6=int(n6), n71=int(n71), n72=int(n72), K6=int(C) * 49)
        self._create(ctx, (C, n6, n71, n72), max_rois, seed, head)

    def _shapes(self):
        d = self.dims
        return {"W6": (d["n6"], d["K6"]), "b6": (d["n6"],), "W71": (d["n71"], d["n6"]), "b71": (d["n71"],),
                "W72": (d["n72"], d["n6"]), "b72": (d["n72"],), "Was": (11, d["n71"]), "bas": (11,),
                "Wab": (44, d["n71"]), "bab": (44,), "Wz": (1, d["n72"]), "bz": (1,)}

    def step(self, conv, rois, adj_labels, adj_targets, adj_loss_weights, zoom_labels, seed, iteration, dmap=None):
        """Forward + backward of one minibatch.  conv: CUDA tensor [N,C,H,W]; dmap: None or a CUDA tensor of conv's shape and
        memory format that receives d loss / d conv5_3.  Returns (losses [zoom, adj, bbox] f32, sum of squares of the head's
        gradients)."""
        lead, _rois, dptr = self._pass_args(conv, rois, dmap)
        R = lead[-1]
        targets = (_f32(adj_labels).reshape(R, 11), _f32(adj_targets).reshape(R, 44), _f32(adj_loss_weights).reshape(R, 44),
                   _f32(zoom_labels).reshape(R))
        return self._step(self.L.az_solver_step, lead, targets, seed, iteration, 3, dptr)

    def forward_test(self, conv, rois):
        """TEST-phase forward (dropout off): raw (zoom_score [R], adj_score [R,11], adj_bbox [R,44])."""
        lead, _rois, _ = self._pass_args(conv, rois)
        R = lead[-1]
        return self._forward(self.L.az_solver_forward_test, lead,
                             (np.empty(R, np.float32), np.empty((R, 11), np.float32), np.empty((R, 44), np.float32)))


DET_MAX_ROIS = 4096                                          # az_det_solver_create's limit on max_rois
DET_HEAD_KEYS = ("W6", "b6", "W7", "b7", "Wc", "bc", "Wb", "bb")
SKIP_KEYS = ("Wp", "bp")                                     # conv_pool5 of an attached skip front


class AzDetSolver(_Trainer):
    """The detection-net trainer behind conv5_3 (az_det_solver_*): fc6 -> fc7 -> {cls_score, bbox_pred} with fp32 master
    weights, gradients and momentum history in HBM; `step` is forward + backward of a minibatch, `update` Caffe's SGD step."""
    _C, KEYS, _NDROP, _U8 = "az_det_solver", DET_HEAD_KEYS, 2, ("mask6", "mask7")
    _I32, _F64 = ("argmax", "skip_argmax", "mine_keep", "mine_nkeep"), ("skip_factor",)
    _ROWS49 = ("cat", "skip_argmax", "skip_factor", "d_y", "d_cat", "d_raw")
    _FLAT = ("mine_loss", "mine_loss_cls", "mine_loss_bbox", "mine_keep", "mine_nkeep")     # of the last mining pass: [R], [N]

    def __init__(self, ctx, C, n6, n7, num_classes, max_rois=256, seed=0, head=None):
        self.dims = dict(C=int(C), n6=int(n6), n7=int(n7), ncls=int(num_classes), K6=int(C) * 49)
        self._create(ctx, (C, n6, n7, num_classes), max_rois, seed, head)

    def _shapes(self):
        d = self.dims
        shp = {"W6": (d["n6"], d["K6"]), "b6": (d["n6"],), "W7": (d["n7"], d["n6"]), "b7": (d["n7"],),
               "Wc": (d["ncls"], d["n7"]), "bc": (d["ncls"],), "Wb": (4 * d["ncls"], d["n7"]), "bb": (4 * d["ncls"],)}
        shp.update(self._skip_shapes())
        return shp

    def _targets(self, R, labels, bbox_targets, bbox_loss_weights):
        nb = 4 * self.dims["ncls"]
        return _f32(labels).reshape(R), _f32(bbox_targets).reshape(R, nb), _f32(bbox_loss_weights).reshape(R, nb)

    def _outs(self, R):
        K = self.dims["ncls"]
        return np.empty((R, K), np.float32), np.empty((R, 4 * K), np.float32)

    def step(self, conv, rois, labels, bbox_targets, bbox_loss_weights, seed, iteration, dmap=None):
        """Forward + backward of one minibatch.  conv: CUDA tensor [N,C,H,W]; dmap: None or a CUDA tensor of conv's shape and
        memory format that receives d loss / d conv5_3.  Returns (losses [cls, bbox] f32, sum of squares of the head's
        gradients)."""
        lead, _rois, dptr = self._pass_args(conv, rois, dmap)
        targets = self._targets(lead[-1], labels, bbox_targets, bbox_loss_weights)
        return self._step(self.L.az_det_solver_step, lead, targets, seed, iteration, 2, dptr)

    def forward_test(self, conv, rois):
        """TEST-phase forward (dropout off): (cls_prob [R, ncls], raw bbox_pred [R, 4 ncls])."""
        lead, _rois, _ = self._pass_args(conv, rois)
        return self._forward(self.L.az_det_solver_forward_test, lead, self._outs(lead[-1]))

    # ---- online hard-example mining (az_det_solver_mine*) ----
    def _mine(self, fn, lead, labels, targets, nms_thresh, per_image, want_losses):
        N, R = (lead[1] if fn is self.L.az_det_solver_mine else lead[5]), lead[-1]
        labels = _f32(labels).reshape(R)
        targets = None if targets is None else _f32(targets).reshape(R, 4)
        per_image = int(per_image)
        sel = np.full((N, max(per_image, 0)), -1, dtype=np.int32)
        n_sel = np.zeros(N, dtype=np.int32)
        loss = np.empty(R, np.float32) if want_losses else None
        f, i32 = ctypes.c_float, ctypes.c_int32
        self.last_rows = R                     # (a refused call has run no pass: fetch then answers for the pass before it)
        self.ctx._chk(fn(self.h, *(list(lead) + [_p(labels, f), None if targets is None else _p(targets, f), float(nms_thresh),
                                                 per_image, _p(sel, i32), _p(n_sel, i32), None if loss is None else _p(loss, f)])))
        return np.concatenate([sel[i, :n_sel[i]] for i in range(N)]) if N else sel.reshape(-1), n_sel, loss

    def mine(self, conv, rois, labels, targets, nms_thresh, per_image, want_losses=False):
        """One hard-example mining pass (az_det_solver_mine): TEST-phase forward over all pool rows, a loss per row, per-image
        NMS with the loss as score.  rois [R,5] with a non-decreasing image index; labels [R]; targets [R,4] (the rows' own
        class's deltas) or None.  Returns (sel int32 [sum n_sel]: the chosen rows image by image in descending loss, n_sel
        int32 [N], the row losses f32 [R] or None)."""
        lead, _rois, _ = self._pass_args(conv, rois)
        return self._mine(self.L.az_det_solver_mine, lead, labels, targets, nms_thresh, per_image, want_losses)

    def mine_skip(self, maps, rois, labels, targets, nms_thresh, per_image, want_losses=False):
        """`mine` behind the skip front (az_det_solver_mine_skip)."""
        lead, _keep, _ = self._skip_args(maps, rois)
        return self._mine(self.L.az_det_solver_mine_skip, lead, labels, targets, nms_thresh, per_image, want_losses)

    # ---- the skip-connection front (az_det_solver_*_skip) ----
    def attach_skip(self, Cs, scales, gain=1000.0, eps=1e-10, seed=0, front=None):
        """Put roi_pool3/4/5 + GRN + concat + scale + conv_pool5 in front of fc6 (az_det_solver_attach_skip); front:
        {"Wp", "bp"} to load at once."""
        Cs = np.ascontiguousarray(Cs, dtype=np.intc)
        sc = _f32(scales).reshape(-1)
        if Cs.size != sc.size:
            raise AzError(AZ_ERR_INVALID, "attach_skip: one spatial_scale per source")
        self.ctx._chk(self.L.az_det_solver_attach_skip(self.h, int(Cs.size), _p(Cs, ctypes.c_int), _p(sc, ctypes.c_float), float(gain),
                                                       float(eps), int(seed) & ((1 << 64) - 1)))
        self.skip = dict(Cs=tuple(int(c) for c in Cs), scales=tuple(float(x) for x in sc), gain=float(gain), eps=float(eps),
                         sumC=int(Cs.sum()))
        if front is not None:
            self.load_skip(front)

    def _skip_shapes(self):
        sk = getattr(self, "skip", None)
        return {} if sk is None else {"Wp": (self.dims["C"], sk["sumC"]), "bp": (self.dims["C"],)}

    def load_skip(self, front):
        shp = self._skip_shapes()
        arrs = [_f32(front[k]).reshape(shp[k]) if k in front and k in shp else None for k in SKIP_KEYS]
        self.ctx._chk(self.L.az_det_solver_load_skip(self.h, *[_p(a, ctypes.c_float) if a is not None else None for a in arrs]))

    def read_skip(self):
        shp = self._skip_shapes()
        out = {k: np.empty(shp.get(k, (0,)), dtype=np.float32) for k in SKIP_KEYS}
        self.ctx._chk(self.L.az_det_solver_read_skip(self.h, *[_p(out[k], ctypes.c_float) for k in SKIP_KEYS]))
        return out

    def load_skip_history(self, hist):
        shp = self._skip_shapes()
        arrs = [_f32(hist[k]).reshape(shp[k]) if k in hist and k in shp else None for k in SKIP_KEYS]
        self.ctx._chk(self.L.az_det_solver_load_skip_history(self.h, *[_p(a, ctypes.c_float) if a is not None else None for a in arrs]))

    def read_skip_history(self):
        if getattr(self, "skip", None) is None:
            raise AzError(AZ_ERR_STATE, "read_skip_history: no skip front attached")
        return {k: self.fetch("h_" + k) for k in SKIP_KEYS}

    def set_skip_hyper(self, lr_mult=None, decay_mult=None):
        a = None if lr_mult is None else _f32(lr_mult).reshape(2)
        b = None if decay_mult is None else _f32(decay_mult).reshape(2)
        f = ctypes.c_float
        self.ctx._chk(self.L.az_det_solver_set_skip_hyper(self.h, None if a is None else _p(a, f), None if b is None else _p(b, f)))

    def _maps(self, maps, dmaps=None):
        """The argument arrays of n maps [N, C_i, H_i, W_i] (float32 CUDA tensors, all in one memory format)."""
        import torch
        maps = list(maps)
        if not maps:
            raise AzError(AZ_ERR_INVALID, "no maps")
        n = len(maps)
        N = int(maps[0].shape[0])
        for m in maps:
            if not (m.is_cuda and m.dtype == torch.float32 and m.dim() == 4 and int(m.shape[0]) == N):
                raise AzError(AZ_ERR_INVALID, "the maps must be float32 CUDA tensors [N, C, H, W] of one batch size")
        if all(m.is_contiguous() for m in maps):
            cl = 0
        elif all(m.is_contiguous(memory_format=torch.channels_last) for m in maps):
            cl = 1
        else:
            raise AzError(AZ_ERR_INVALID, "the maps must all be contiguous or all channels_last")
        Cs = np.asarray([m.shape[1] for m in maps], dtype=np.intc)
        Hs = np.asarray([m.shape[2] for m in maps], dtype=np.intc)
        Ws = np.asarray([m.shape[3] for m in maps], dtype=np.intc)
        ptrs = (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps])
        dptrs = None
        if dmaps is not None:
            dmaps = list(dmaps)
            if len(dmaps) != n:
                raise AzError(AZ_ERR_INVALID, "dmaps: one entry (or None) per map")
            for d, m in zip(dmaps, maps):
                if d is not None:
                    if not (d.is_cuda and d.dtype == m.dtype and d.shape == m.shape and d.stride() == m.stride()):
                        raise AzError(AZ_ERR_INVALID, "dmaps: every buffer must have its map's device, dtype, shape and strides")
            dptrs = (ctypes.c_void_p * n)(*[None if d is None else d.data_ptr() for d in dmaps])
        torch.cuda.current_stream(maps[0].device).synchronize()
        return n, Cs, ptrs, Hs, Ws, N, cl, dptrs

    def _skip_args(self, maps, rois, dmaps=None):
        """The leading arguments of *_step_skip / *_forward_test_skip, the arrays that back them, and dmaps' pointers."""
        n, Cs, ptrs, Hs, Ws, N, cl, dptrs = self._maps(maps, dmaps)
        rois = _f32(rois).reshape(-1, 5)
        f, ci = ctypes.c_float, ctypes.c_int
        return (n, _p(Cs, ci), ptrs, _p(Hs, ci), _p(Ws, ci), N, cl, _p(rois, f), rois.shape[0]), (Cs, Hs, Ws, rois), dptrs

    def step_skip(self, maps, rois, labels, bbox_targets, bbox_loss_weights, seed, iteration, dmaps=None):
        """Forward + backward of one minibatch through the skip front and the head.  maps: CUDA tensors [N, C_i, H_i, W_i] in
        concat order; dmaps: None, or a list with, per map, None or a tensor of the map's shape and memory format that
        receives d loss / d map.  Returns (losses [cls, bbox] f32, sum of squares of all ten gradients)."""
        lead, _keep, dptrs = self._skip_args(maps, rois, dmaps)
        targets = self._targets(lead[-1], labels, bbox_targets, bbox_loss_weights)
        return self._step(self.L.az_det_solver_step_skip, lead, targets, seed, iteration, 2, dptrs)

    def forward_test_skip(self, maps, rois):
        """TEST-phase forward of the skip net: (cls_prob [R, ncls], raw bbox_pred [R, 4 ncls])."""
        lead, _keep, _ = self._skip_args(maps, rois)
        return self._forward(self.L.az_det_solver_forward_test_skip, lead, self._outs(lead[-1]))


def skip_pool_bwd_unit(ctx, maps, scales, rois, d_raw=None, channels_last=False, want=None):
    """az_skip_pool_bwd_unit: roi_pool3/4/5 with arg-max on host maps [N, C_i, H_i, W_i] (NumPy, NCHW order; with
    channels_last they are handed over -- and the gradients taken back -- in NHWC memory order) and the gather of d_raw
    [R*49, sum C].  want: per map, whether its gradient is asked for (default: all, when d_raw is given).  Returns
    (pooled [R*49, sum C] f32, argmax [R*49, sum C] int32, [d map_i or None])."""
    maps = [_f32(m) for m in maps]
    n = len(maps)
    N = maps[0].shape[0]
    Cs = np.asarray([m.shape[1] for m in maps], dtype=np.intc)
    Hs = np.asarray([m.shape[2] for m in maps], dtype=np.intc)
    Ws = np.asarray([m.shape[3] for m in maps], dtype=np.intc)
    sc = _f32(scales).reshape(n)
    dev = [np.ascontiguousarray(m.transpose(0, 2, 3, 1)) if channels_last else m for m in maps]
    rois = _f32(rois).reshape(-1, 5)
    R, sumC = rois.shape[0], int(Cs.sum())
    pooled = np.empty((R * 49, sumC), np.float32)
    arg = np.empty((R * 49, sumC), np.int32)
    f, ci = ctypes.c_float, ctypes.c_int
    ptrs = (ctypes.c_void_p * n)(*[m.ctypes.data for m in dev])
    dr, douts, dptrs = None, [None] * n, None
    if d_raw is not None:
        dr = _f32(d_raw).reshape(R * 49, sumC)
        want = [True] * n if want is None else list(want)
        douts = [np.empty_like(m) if w else None for m, w in zip(dev, want)]
        dptrs = (ctypes.c_void_p * n)(*[None if d is None else d.ctypes.data for d in douts])
    ctx._chk(ctx.L.az_skip_pool_bwd_unit(ctx.h, n, _p(Cs, ci), _p(sc, f), ptrs, _p(Hs, ci), _p(Ws, ci), int(N), 1 if channels_last else 0,
                                         _p(rois, f), R, None if dr is None else _p(dr, f), _p(pooled, f),
                                         arg.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dptrs))
    if channels_last:
        douts = [None if d is None else np.ascontiguousarray(d.transpose(0, 3, 1, 2)) for d in douts]
    return pooled, arg, douts


def sgd_update(ctx, w, g, hist, rate, momentum, decay, clip_scale=1.0):
    """az_sgd_update on three contiguous float32 CUDA tensors of one size (w and hist are updated in place)."""
    import torch
    for t in (w, g, hist):
        assert t.is_cuda and t.dtype == torch.float32 and t.numel() == w.numel()
        assert t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)
    assert g.stride() == w.stride() and hist.stride() == w.stride()
    torch.cuda.current_stream(w.device).synchronize()
    ctx._chk(ctx.L.az_sgd_update(ctx.h, ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(g.data_ptr()),
                                 ctypes.c_void_p(hist.data_ptr()), int(w.numel()), float(rate), float(momentum), float(decay),
                                 float(clip_scale)))


def gemm_unit(ctx, form, a, b, precision=0):
    """One product of the trainer's GEMM kernel (az_solver_gemm_unit_prec): form 0 a[M,K] b[N,K]^T, 1 a[M,K] b[K,N],
    2 a[K,M]^T b[K,N]; precision AZ_TRAIN_FP32 or AZ_TRAIN_BF16."""
    a, b = _f32(a), _f32(b)
    if form == 0:
        (M, K), N = a.shape, b.shape[0]
    elif form == 1:
        (M, K), N = a.shape, b.shape[1]
    else:
        (K, M), N = a.shape, b.shape[1]
    d = np.empty((M, N), dtype=np.float32)
    f = ctypes.c_float
    ctx._chk(ctx.L.az_solver_gemm_unit_prec(ctx.h, int(form), int(precision), _p(a, f), _p(b, f), _p(d, f), M, N, K))
    return d


def bias_relu_(y, bias):
    """In place on a CUDA fp32 tensor y [1,C,H,W] (contiguous or channels_last): y = max(y + bias[c], 0) in one launch on
    torch's current stream (az_bias_relu).  Returns y."""
    import torch
    L = load_library()
    C, H, W = int(y.shape[1]), int(y.shape[2]), int(y.shape[3])
    cl = y.is_contiguous(memory_format=torch.channels_last) and not (y.is_contiguous() and C > 1 and H * W > 1)
    if not cl and not y.is_contiguous():
        raise ValueError("bias_relu_: the tensor must be contiguous or channels_last")
    rc = L.az_bias_relu(ctypes.c_void_p(torch.cuda.current_stream(y.device).cuda_stream), ctypes.c_void_p(y.data_ptr()),
                        ctypes.c_void_p(bias.data_ptr()), C, H * W, 1 if cl else 0)
    if rc != AZ_OK:
        raise AzError(rc, "az_bias_relu")
    return y


def bias_relu_pool(y, bias):
    """y [1,C,H,W] CUDA fp32 (contiguous or channels_last) -> max_pool2d(relu(y + bias), 2, 2, ceil_mode=True) as a new tensor
    of the same memory format, one launch on torch's current stream (az_bias_relu_pool)."""
    import torch
    L = load_library()
    C, H, W = int(y.shape[1]), int(y.shape[2]), int(y.shape[3])
    cl = y.is_contiguous(memory_format=torch.channels_last) and not (y.is_contiguous() and C > 1 and H * W > 1)
    if not cl and not y.is_contiguous():
        raise ValueError("bias_relu_pool: the tensor must be contiguous or channels_last")
    out = torch.empty((1, C, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=y.device,
                      memory_format=torch.channels_last if cl else torch.contiguous_format)
    rc = L.az_bias_relu_pool(ctypes.c_void_p(torch.cuda.current_stream(y.device).cuda_stream), ctypes.c_void_p(y.data_ptr()),
                             ctypes.c_void_p(bias.data_ptr()), ctypes.c_void_p(out.data_ptr()), C, H, W, 1 if cl else 0)
    if rc != AZ_OK:
        raise AzError(rc, "az_bias_relu_pool")
    return out


def _rank_device():
    """This process's GPU: torch's current device when torch has one, else LOCAL_RANK, else 0 --
    one process per GPU, so the drop-in helpers must not all land on GPU 0."""
    try:
        import torch
        if torch.cuda.is_available():
            return int(torch.cuda.current_device())
    except Exception:
        pass
    return int(os.environ.get("LOCAL_RANK", "0"))


def set_default_context(ctx):
    """Make `ctx` (the context of this rank's HipAZNet) the one the drop-in modules use."""
    global _default_ctx
    _default_ctx = ctx
    return ctx


def default_context(device=None):
    """Process-wide context used by the drop-in modules (utils.cython_div / cython_nms / cython_bbox,
    apply_nms): the rank's own net's context when one exists (HipAZNet registers itself), otherwise a
    context created on this rank's GPU."""
    global _default_ctx
    if _default_ctx is None or getattr(_default_ctx, "h", None) is None:
        _default_ctx = AzContext(_rank_device() if device is None else device)
    return _default_ctx
