"""ctypes binding of include/yolact_hip.h (the C ABI of libyolact_hip.so)."""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None

OK, EINVAL, EHIP, ENOMEM, EWEIGHTS, ESTATE, EDIVERGE, EOVERFLOW = 0, -1, -2, -3, -4, -5, -6, -7
COMPAT_STRICT, COMPAT_SANE = 0, 1
TOUR_MAX = 6   # YH_TOUR_MAX
SCENE_STREAMS_MAX = 64   # YH_SCENE_STREAMS_MAX


class YhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"yolact_hip error {code}: {msg}")
        self.code = code


PRECISION_F16, PRECISION_FP8 = 0, 1

# yh_tuning (include/yolact_hip_debug.h): per-handle measurement / test knobs, -1 = the library's default; the reserved
# slots that follow them are not named here, so tune= cannot set them
TUNING_FIELDS = ("plan_cus", "chsplit", "upfuse", "ablate", "op_tile", "op_kslices", "tfl_dot", "tfl_graph", "tailfork", "dsfuse",
                 "headfork_maxb", "protofuse", "chain", "tfl_fuse", "tfl_group", "op_xgap", "op_tanh_from")


class Tuning(C.Structure):
    _fields_ = [(f, C.c_int32) for f in TUNING_FIELDS] + [("reserved", C.c_int32 * 15)]

    @classmethod
    def of(cls, **kw):
        t = cls()
        C.memset(C.byref(t), 0xFF, C.sizeof(t))
        for k, v in kw.items():
            assert k in TUNING_FIELDS, k
            setattr(t, k, int(v))
        return t

    def as_dict(self):
        return {f: getattr(self, f) for f in TUNING_FIELDS}


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("backbone", C.c_int32),
                ("input_size", C.c_int32), ("max_batch", C.c_int32), ("num_classes", C.c_int32),
                ("top_k", C.c_int32), ("max_dets", C.c_int32), ("conf_thresh", C.c_float),
                ("nms_thresh", C.c_float), ("use_graph", C.c_int32), ("debug_tensors", C.c_int32),
                ("precision", C.c_int32), ("fp8_f16_layers", C.c_int32), ("fp8_per_tensor", C.c_int32), ("reserved", C.c_int32 * 4), ("tune", Tuning)]


class TensorInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("kind", C.c_int32), ("ndims", C.c_int32), ("dims", C.c_int32 * 4),
                ("scale", C.c_float), ("zero_point", C.c_int32)]


class Detection(C.Structure):
    _fields_ = [("class_id", C.c_int32), ("prior", C.c_int32), ("score", C.c_float), ("box", C.c_float * 4)]


class TflDetectConfig(C.Structure):
    """yh_tfl_detect_config (include/yolact_hip.h)."""
    _fields_ = [("outputs", C.c_int32 * 4), ("top_k", C.c_int32), ("max_dets", C.c_int32), ("conf_thresh", C.c_float),
                ("nms_thresh", C.c_float), ("max_images", C.c_int32), ("reserved", C.c_int32 * 4)]


def lib_path():
    return os.path.join(_PKG, "lib", "libyolact_hip.so")


# every symbol include/yolact_hip.h declares: (name, restype, argtypes)
_vp, _i, _f, _sz = C.c_void_p, C.c_int32, C.c_float, C.c_size_t
SYMBOLS = [
    ("yh_version", C.c_char_p, []),
    ("yh_default_config", None, [C.POINTER(Config)]),
    ("yh_create", _i, [C.POINTER(Config), C.POINTER(_vp)]),
    ("yh_destroy", None, [_vp]),
    ("yh_set_tuning", _i, [_vp, C.POINTER(Tuning)]),
    ("yh_get_tuning", _i, [_vp, C.POINTER(Tuning)]),
    ("yh_last_error", C.c_char_p, [_vp]),
    ("yh_weights_nbytes", _sz, [_vp]),
    ("yh_weights_device_ptr", _vp, [_vp]),
    ("yh_weights_generate", _i, [_vp, C.c_uint64, _vp, _sz]),
    ("yh_load_weights_host", _i, [_vp, _vp, _sz]),
    ("yh_load_weights_device", _i, [_vp, _vp, _sz]),
    ("yh_fp8_calibrate", _i, [_vp]),
    ("yh_fp8_layer_count", _i, [_vp]),
    ("yh_fp8_layer_info", _i, [_vp, _i, C.POINTER(C.c_char_p), C.POINTER(_f)]),
    ("yh_fp8_set_layer_scale", _i, [_vp, _i, _f]),
    ("yh_fp8_layer_channels", _i, [_vp, _i]),
    ("yh_fp8_layer_channel_scales", _i, [_vp, _i, _vp, _i]),
    ("yh_fp8_set_layer_channel_scales", _i, [_vp, _i, _vp, _i]),
    ("yh_group_broadcast_weights", _i, [C.POINTER(_vp), _i, _i]),
    ("yh_rccl_unique_id", _i, [_vp]),
    ("yh_rank_broadcast_weights", _i, [_vp, _vp, _i, _i, _i]),
    ("yh_group_create", _i, [C.POINTER(Config), C.POINTER(_i), _i, C.POINTER(_vp)]),
    ("yh_group_destroy", None, [_vp]),
    ("yh_group_last_error", C.c_char_p, [_vp]),
    ("yh_group_size", _i, [_vp]),
    ("yh_group_member", _vp, [_vp, _i]),
    ("yh_group_load_weights_host", _i, [_vp, _vp, _sz]),
    ("yh_group_replicate_weights", _i, [_vp]),
    ("yh_group_weights_replication", C.c_char_p, [_vp]),
    ("yh_group_fp8_calibrate", _i, [_vp]),
    ("yh_group_evaluate", _i, [_vp, _vp, _i, _i]),
    ("yh_group_evaluate_device", _i, [_vp, C.POINTER(_vp), C.POINTER(_i), _i]),
    ("yh_group_prepare", _i, [_vp, _i, _i]),
    ("yh_group_sync", _i, [_vp]),
    ("yh_group_read_detections", _i, [_vp, _i, C.POINTER(_i), _vp, _i, _vp, _sz]),
    ("yh_group_frame_owner", _i, [_vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    ("yh_input_dims", _i, [_vp, C.POINTER(_i * 4)]),
    ("yh_set_input_u8", _i, [_vp, _vp, _i]),
    ("yh_set_input_u8_device", _i, [_vp, _vp, _i]),
    ("yh_invoke", _i, [_vp]),
    ("yh_prepare", _i, [_vp, _i, _i]),
    ("yh_sync", _i, [_vp]),
    ("yh_output_count", _i, [_vp]),
    ("yh_output_info", _i, [_vp, _i, C.POINTER(TensorInfo)]),
    ("yh_output_read_f32", _i, [_vp, _i, _vp, _sz]),
    ("yh_output_device_ptr", _vp, [_vp, _i]),
    ("yh_evaluate", _i, [_vp]),
    ("yh_read_detections", _i, [_vp, _i, C.POINTER(_i), _vp, _i, _vp, _sz]),
    ("yh_proto_dims", _i, [_vp, C.POINTER(_i * 2)]),
    ("yh_num_priors", _i, [_vp]),
    ("yh_read_priors", _i, [_vp, _vp, _sz]),
    ("yh_classify_frame_u32", _i, [_vp, _vp, _i, _i, _i]),
    ("yh_postprocess_cells", _i, [_vp, _vp, _i, _vp, _i]),
    ("yh_resize_triangle_rgb8", _i, [_vp, _vp, _i, _i, _vp, _i, _i]),
    ("yh_profile_launch_count", _i, [_vp, _i]),
    ("yh_profile_run", _i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("yh_time_steps", _i, [_vp, _i, _i, C.POINTER(_f)]),
    ("yh_flops_per_frame", C.c_double, [_vp]),
    ("yh_tfl_validate", _i, [_vp, _sz, C.POINTER(_i), C.POINTER(_i), C.c_char_p, _sz]),
    ("yh_tfl_create", _i, [_vp, _sz, _i, C.POINTER(_vp)]),
    ("yh_tfl_create_tuned", _i, [_vp, _sz, _i, C.POINTER(Tuning), C.POINTER(_vp)]),
    ("yh_tfl_create_batch", _i, [_vp, _sz, _i, _i, C.POINTER(_vp)]),
    ("yh_tfl_create_batch_tuned", _i, [_vp, _sz, _i, _i, C.POINTER(Tuning), C.POINTER(_vp)]),
    ("yh_tfl_destroy", None, [_vp]),
    ("yh_tfl_last_error", C.c_char_p, [_vp]),
    ("yh_tfl_input_info", _i, [_vp, C.POINTER(TensorInfo)]),
    ("yh_tfl_output_count", _i, [_vp]),
    ("yh_tfl_output_info", _i, [_vp, _i, C.POINTER(TensorInfo)]),
    ("yh_tfl_set_batch", _i, [_vp, _i]),
    ("yh_tfl_set_input", _i, [_vp, _vp, _sz]),
    ("yh_tfl_invoke", _i, [_vp]),
    ("yh_tfl_output_read", _i, [_vp, _i, _vp, _sz]),
    ("yh_tfl_tensor_count", _i, [_vp]),
    ("yh_tfl_plan_info", _i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    ("yh_tfl_direct_forms", _i, [C.POINTER(_i), _i]),
    ("yh_tfl_op_info", _i, [_vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    ("yh_tfl_op_quant", _i, [_vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    ("yh_tfl_tensor_read", _i, [_vp, _i, _vp, _sz]),
    ("yh_tfl_classify_frame_u32", _i, [_vp, _vp, _i, _i, _i]),
    ("yh_tfl_classify_batch_u32", _i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    ("yh_tfl_classify_batch_device_frames", _vp, [_vp]),
    ("yh_scene_create", _i, [_i, _i, _i, C.POINTER(_vp)]),
    ("yh_scene_destroy", None, [_vp]),
    ("yh_scene_last_error", C.c_char_p, [_vp]),
    ("yh_scene_append", _i, [_vp, _vp, _vp, _i]),
    ("yh_scene_append_classified", _i, [_vp, _vp, _vp, _i, _i]),
    ("yh_scene_read", _i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    ("yh_scene_time", _i, [_vp, _i, C.POINTER(_f)]),
    ("yh_scene_plan", _i, [_vp, _vp, _i, _i, _i]),
    ("yh_scene_plan_conn", _i, [_vp, _vp, _i, _i, _i, _i]),
    ("yh_scene_plan_read", _i, [_vp, _vp, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    ("yh_scene_set_fields", _i, [_vp, _vp, _vp, _vp]),
    ("yh_scene_plan_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_i), C.POINTER(_i)]),
    ("yh_scene_plan_tour", _i, [_vp, _vp, _i, _i, _i]),
    ("yh_scene_plan_tour_conn", _i, [_vp, _vp, _i, _i, _i, _i]),
    ("yh_scene_tour_read", _i, [_vp, C.POINTER(_i), _vp, _vp, _vp, C.POINTER(_f), _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    ("yh_scene_tour_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_i), C.POINTER(_i)]),
    ("yh_scene_plan_turn", _i, [_vp, _vp, _i, _i, _i, _i, _f]),
    ("yh_scene_turn_read", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    ("yh_scene_turn_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_i), C.POINTER(_i)]),
    ("yh_scene_plan_turn_tour", _i, [_vp, _vp, _i, _i, _i, _i, _f]),
    ("yh_scene_turn_tour_read", _i, [_vp, C.POINTER(_i), _vp, _vp, _vp, _vp, C.POINTER(_f), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    ("yh_scene_turn_tour_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_i), C.POINTER(_i)]),
    ("yh_scene_append_memory", _i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i]),
    ("yh_scene_memory_read", _i, [_vp, _vp, _vp]),
    ("yh_scene_memory_reset", _i, [_vp]),
    ("yh_scene_memory_time", _i, [_vp, _i, C.POINTER(_f)]),
    ("yh_scene_append_memory_search", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i]),
    ("yh_scene_motion_read", _i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    ("yh_scene_memory_search_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_f)]),
    ("yh_scene_op_register", _i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    ("yh_scene_append_memory_search_norm", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i]),
    ("yh_scene_motion_norm_read", _i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    ("yh_scene_memory_search_norm_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_f)]),
    ("yh_scene_op_register_norm", _i, [_vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("yh_scene_append_memory_pyramid", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _i]),
    ("yh_scene_pyramid_read", _i, [_vp, _i, _vp, _vp, _vp]),
    ("yh_scene_memory_pyramid_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_f)]),
    ("yh_scene_op_pyramid", _i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("yh_scene_append_memory_pyramid_norm", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    ("yh_scene_pyramid_norm_read", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("yh_scene_memory_pyramid_norm_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_f)]),
    ("yh_scene_op_pyramid_norm", _i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    ("yh_scene_batch_create", _i, [_i, _i, _i, _i, C.POINTER(_vp)]),
    ("yh_scene_batch_destroy", None, [_vp]),
    ("yh_scene_batch_last_error", C.c_char_p, [_vp]),
    ("yh_scene_batch_stage", _i, [_vp, _i, _vp, _vp, _i]),
    ("yh_scene_batch_stage_frames", _i, [_vp, _i, _i, _vp, _vp, _i]),
    ("yh_scene_batch_append", _i, [_vp, _i, _i]),
    ("yh_scene_batch_read", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    ("yh_scene_batch_plan", _i, [_vp, _vp, _i, _vp, _i, _vp]),
    ("yh_scene_batch_plan_read", _i, [_vp, _i, _vp, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    ("yh_scene_batch_time", _i, [_vp, _i, C.POINTER(_f)]),
    ("yh_scene_batch_plan_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_i), C.POINTER(_i)]),
    ("yh_scene_batch_set_fields", _i, [_vp, _i, _vp, _vp, _vp]),
    ("yh_scene_batch_append_memory", _i, [_vp, _i, _vp, _vp, _vp, _i, _i]),
    ("yh_scene_batch_memory_read", _i, [_vp, _i, _vp, _vp]),
    ("yh_scene_batch_memory_frame_balls", _i, [_vp, _i, _vp]),
    ("yh_scene_batch_memory_reset", _i, [_vp, _i]),
    ("yh_scene_batch_memory_time", _i, [_vp, _i, C.POINTER(_f)]),
    ("yh_scene_batch_append_memory_search", _i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i]),
    ("yh_scene_batch_motion_read", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    ("yh_scene_batch_memory_search_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_f)]),
    ("yh_scene_batch_append_memory_pyramid", _i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i]),
    ("yh_scene_batch_pyramid_read", _i, [_vp, _i, _i, _vp, _vp, _vp]),
    ("yh_scene_batch_memory_pyramid_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_f)]),
    ("yh_scene_batch_append_memory_search_norm", _i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i]),
    ("yh_scene_batch_motion_norm_read", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    ("yh_scene_batch_memory_search_norm_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_f)]),
    ("yh_scene_batch_append_memory_pyramid_norm", _i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    ("yh_scene_batch_pyramid_norm_read", _i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("yh_scene_batch_memory_pyramid_norm_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_f)]),
    ("yh_scene_batch_plan_turn", _i, [_vp, _vp, _i, _vp, _vp, _f, _vp]),
    ("yh_scene_batch_turn_read", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    ("yh_scene_batch_turn_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_i), C.POINTER(_i)]),
    ("yh_scene_batch_plan_turn_tour", _i, [_vp, _vp, _i, _vp, _vp, _f, _vp]),
    ("yh_scene_batch_turn_tour_read", _i, [_vp, _i, C.POINTER(_i), _vp, _vp, _vp, _vp, C.POINTER(_f), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    ("yh_scene_batch_turn_tour_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_i), C.POINTER(_i)]),
    ("yh_scene_batch_plan_tour", _i, [_vp, _vp, _i, _vp, _i, _vp]),
    ("yh_scene_batch_tour_read", _i, [_vp, _i, C.POINTER(_i), _vp, _vp, _vp, C.POINTER(_f), _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    ("yh_scene_batch_tour_time", _i, [_vp, _i, C.POINTER(_f), C.POINTER(_i), C.POINTER(_i)]),
    ("yh_classify_device_frame", _vp, [_vp]),
    ("yh_classify_batch_u32", _i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    ("yh_classify_batch_device_frames", _vp, [_vp]),
    ("yh_instance_frame", _i, [_vp, _i, _i, _i, _vp, _f, _vp]),
    ("yh_instance_device_frame", _vp, [_vp]),
    ("yh_instance_read", _i, [_vp, C.POINTER(_i), _vp, _i]),
    ("yh_instance_batch", _i, [_vp, _i, _i, _i, _i, _vp, _f, _vp]),
    ("yh_instance_batch_device_frames", _vp, [_vp]),
    ("yh_instance_batch_read", _i, [_vp, _i, C.POINTER(_i), _vp, _i]),
    ("yh_instance_track", _i, [_vp, _i, _i, _i, _vp, _f, _i, _i, _vp]),
    ("yh_instance_tracks_read", _i, [_vp, C.POINTER(_i), _vp, _i]),
    ("yh_instance_track_reset", _i, [_vp]),
    ("yh_instance_track_batch", _i, [_vp, _i, _i, _i, _i, _vp, _f, _i, _i, _vp, _vp]),
    ("yh_instance_track_batch_read", _i, [_vp, _i, C.POINTER(_i), _vp, _i]),
    ("yh_instance_track_reset_stream", _i, [_vp, _i]),
    ("yh_debug_read_tensor", _i, [_vp, C.c_char_p, _vp, _sz, C.POINTER(_i * 4)]),
    ("yh_debug_read_tensor_frame", _i, [_vp, C.c_char_p, _i, _vp, _sz, C.POINTER(_i * 4)]),
    ("yh_debug_read_tensor_e4m3", _i, [_vp, C.c_char_p, _i, _vp, _sz, C.POINTER(_i * 4)]),
    ("yh_debug_fp8_weights", _i, [_vp, _i, _vp, _vp, C.POINTER(_i * 2)]),
    ("yh_debug_last_conv_launches", _i, [_vp]),
    ("yh_debug_last_conv_forms", _i, [_vp, _vp, _i]),
    ("yh_conv_forms", _i, [_vp, _i]),
    ("yh_debug_alloc_map", _i, [_vp, C.c_char_p, _sz]),
    ("yh_debug_setup_audit", _i, [C.POINTER(C.c_int64 * 4)]),
    ("yh_debug_rccl_shared_device", _i, [_i]),
    ("yh_debug_rccl_library", _i, [C.c_char_p]),
    ("yh_debug_set_cu_mask", _i, [_vp, _vp, _i]),
    ("yh_debug_run_phase", _i, [_vp, _i, _i, C.POINTER(_f)]),
    ("yh_debug_graph_nodes", _i, [_vp, _i, C.c_char_p, _sz]),
    ("yh_debug_guard_selfcheck", _i, [_vp, _i]),
    ("yh_debug_act_paint", _i, [_vp, _i]),
    ("yh_debug_act_check", _i, [_vp, _i, C.c_char_p, _sz]),
    ("yh_op_stem_pool_f16", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("yh_op_stem_pool_rgb8", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("yh_op_quantize_e4m3", _i, [_vp, _vp, _sz, C.c_float, _vp]),
    ("yh_op_absmax_channels_f16", _i, [_vp, _vp, C.c_int64, _i, _vp]),
    ("yh_op_conv2d_fp8", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    ("yh_op_conv2d_levels_fp8", _i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    ("yh_op_conv2d_resup_f16", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _i, _i, _vp]),
    ("yh_op_conv2d_tail_f16", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    ("yh_op_conv2d_tail_fp8", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    ("yh_op_conv2d_dual_f16", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp]),
    ("yh_op_bneck_f16", _i, [_vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("yh_op_conv2d_levels_f16", _i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp]),
    ("yh_op_conv2d_f16", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    ("yh_op_bilinear_f16", _i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    ("yh_op_maxpool3x3s2_f16", _i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    ("yh_op_detect", _i, [_vp, _vp, _vp, _vp, _vp, _i]),
    ("yh_op_instance_frame", _i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _f, _vp, _vp, _i, C.POINTER(_i)]),
    ("yh_op_instance_track", _i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _f, _i, _i, _vp, _vp, _i, C.POINTER(_i)]),
    ("yh_op_instance_batch", _i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _f, _vp]),
    ("yh_op_instance_track_batch", _i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _f, _i, _i, _vp, _vp]),
    ("yh_op_classify_pre_batch", _i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    ("yh_op_classify_post_batch", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    ("yh_tfl_default_detect_config", None, [_vp]),
    ("yh_tfl_detect_setup", _i, [_vp, _vp, _vp, _i]),
    ("yh_tfl_evaluate", _i, [_vp]),
    ("yh_tfl_detect", _i, [_vp]),
    ("yh_tfl_read_detections", _i, [_vp, _i, C.POINTER(_i), _vp, _i, _vp, _sz]),
    ("yh_tfl_proto_dims", _i, [_vp, C.POINTER(_i * 2)]),
    ("yh_tfl_detections_device", _vp, [_vp]),
    ("yh_tfl_detection_counts_device", _vp, [_vp]),
    ("yh_tfl_masks_device", _vp, [_vp]),
    ("yh_tfl_detect_stage_times", _i, [_vp, _i, C.POINTER(_f * 4)]),
    ("yh_tfl_op_detect", _i, [_vp, _i, _i, _i, _i, _i] + [_vp, _i, _f, _i] * 4 + [_vp, _i, _i, _f, _f]),
    ("yh_tfl_instance_batch", _i, [_vp, _i, _i, _i, _i, _vp, _f, _vp]),
    ("yh_tfl_instance_frames", _i, [_vp, _i, _i, _i, _i, _vp, _f, _vp]),
    ("yh_tfl_instance_device_frames", _vp, [_vp]),
    ("yh_tfl_instance_read", _i, [_vp, _i, C.POINTER(_i), _vp, _i]),
    ("yh_tfl_instance_row_width", _i, [_vp]),
    ("yh_tfl_op_instance_frames", _i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _f, _vp]),
]


def load_library():
    """Loads libyolact_hip.so. Raises (never falls back) if it has not been built."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "(there is no CPU fallback for the HIP kernel library)")
        L = C.CDLL(path)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)  # AttributeError if the ABI symbol is absent
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def version():
    return load_library().yh_version().decode()


# ConvForm (csrc/yh_internal.h, exported as YH_FORM_* by include/yolact_hip_debug.h): index = the form's number. "REDUCE" is no form of
# the table: Engine.last_conv_forms lists splitk_reduce_f16 as (-1, "REDUCE").
CONV_FORMS = ("PLAIN", "K3", "SPLITK", "ML", "ML_SPLITK", "DUAL", "DUAL_SPLITK", "RESUP", "TAIL", "LIN")
CONV_FORM_NAMES = CONV_FORMS + ("REDUCE",)


def conv_forms():
    """yh_conv_forms: the compiled table of conv kernel instances, one dict(tile, tch, tm, fp8, forms) per tile - forms = the names
    (CONV_FORMS) of the forms the tile is instantiated in. Needs no GPU."""
    L = load_library()
    n = L.yh_conv_forms(None, 0)
    rows = np.zeros((n, 5), np.int32)
    assert L.yh_conv_forms(_p(rows), n) == n
    assert not (rows[:, 4] >> len(CONV_FORMS)).any(), "a form bit this binding has no name for"
    return [dict(tile=int(r[0]), tch=int(r[1]), tm=int(r[2]), fp8=bool(r[3]), forms=tuple(f for i, f in enumerate(CONV_FORMS) if r[4] >> i & 1))
            for r in rows]


def setup_audit():
    """yh_debug_setup_audit: process-wide counters of the setup discipline -
    dict(setups, worker_jobs, overlaps, in_flight); `overlaps` must stay 0."""
    L = load_library()
    a = (C.c_int64 * 4)()
    rc = L.yh_debug_setup_audit(C.byref(a))
    if rc != OK:
        raise YhError(rc, "yh_debug_setup_audit")
    return dict(setups=a[0], worker_jobs=a[1], overlaps=a[2], in_flight=a[3])


def rccl_unique_id():
    """ncclGetUniqueId through the library (128 bytes) for yh_rank_broadcast_weights."""
    L = load_library()
    buf = C.create_string_buffer(128)
    rc = L.yh_rccl_unique_id(buf)
    if rc != OK:
        raise YhError(rc, L.yh_last_error(None).decode())
    return buf.raw


def group_broadcast_weights(engines, root=0):
    """One process, one Engine per GPU: RCCL broadcast of engines[root]'s weights to the others."""
    L = load_library()
    arr = (C.c_void_p * len(engines))(*[e.h for e in engines])
    rc = L.yh_group_broadcast_weights(arr, len(engines), root)
    if rc != OK:
        raise YhError(rc, L.yh_last_error(engines[root].h).decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f16_bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float16)).view(np.uint16)


def _bits_f32(b, shape):
    return b.view(np.float16).astype(np.float32).reshape(shape)


class Engine:
    """RAII wrapper of one yh_engine handle."""

    def __init__(self, input_size=550, backbone=50, max_batch=1, num_classes=81, top_k=200, max_dets=100,
                 conf_thresh=0.05, nms_thresh=0.5, use_graph=True, device=0, debug_tensors=False, precision=PRECISION_F16,
                 tune=None, fp8_f16_layers=0, fp8_per_tensor=False):
        self.L = load_library()
        cfg = Config()
        self.L.yh_default_config(C.byref(cfg))
        cfg.device, cfg.backbone, cfg.input_size, cfg.max_batch = device, backbone, input_size, max_batch
        cfg.num_classes, cfg.top_k, cfg.max_dets = num_classes, top_k, max_dets
        cfg.conf_thresh, cfg.nms_thresh, cfg.use_graph = conf_thresh, nms_thresh, 1 if use_graph else 0
        cfg.debug_tensors = 1 if debug_tensors else 0
        cfg.precision = precision
        cfg.fp8_f16_layers = fp8_f16_layers
        cfg.fp8_per_tensor = 1 if fp8_per_tensor else 0
        if tune:
            cfg.tune = Tuning.of(**tune)
        self._tune = dict(tune or {})
        self.cfg = cfg
        h = C.c_void_p()
        rc = self.L.yh_create(C.byref(cfg), C.byref(h))
        if rc != OK:
            raise YhError(rc, self.L.yh_last_error(None).decode())
        self.h = h
        self.S, self.C, self.max_batch = input_size, num_classes, max_batch
        self.P = self.L.yh_num_priors(self.h)
        d = (C.c_int32 * 2)()
        self.L.yh_proto_dims(self.h, C.byref(d))
        self.hp, self.wp = d[0], d[1]
        self.n = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.yh_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            raise YhError(rc, self.L.yh_last_error(self.h).decode())

    # ---- tuning (per handle; the library reads no environment variable)
    def set_tuning(self, **kw):
        """Replaces the run-time tuning fields; fields not named keep what this wrapper last set."""
        self._tune.update(kw)
        t = Tuning.of(**self._tune)
        self._chk(self.L.yh_set_tuning(self.h, C.byref(t)))

    def reset_tuning(self, *names):
        for k in names:
            self._tune.pop(k, None)
        t = Tuning.of(**self._tune)
        self._chk(self.L.yh_set_tuning(self.h, C.byref(t)))

    def tuning(self):
        t = Tuning()
        self._chk(self.L.yh_get_tuning(self.h, C.byref(t)))
        return t.as_dict()

    # ---- weights
    def weights_nbytes(self):
        return self.L.yh_weights_nbytes(self.h)

    def generate_weights(self, seed=1):
        blob = np.zeros(self.weights_nbytes(), np.uint8)
        self._chk(self.L.yh_weights_generate(self.h, seed, _p(blob), blob.size))
        return blob

    def load_weights(self, blob):
        blob = np.ascontiguousarray(blob, np.uint8)
        self._chk(self.L.yh_load_weights_host(self.h, _p(blob), blob.size))

    def weights_device_ptr(self):
        return self.L.yh_weights_device_ptr(self.h)

    def load_weights_device(self, dev_ptr, nbytes):
        self._chk(self.L.yh_load_weights_device(self.h, C.c_void_p(dev_ptr), nbytes))

    # ---- fp8 precision (configs[4])
    def fp8_calibrate(self):
        """Sets every fp8 input tensor's scale from the f16 forward of the frames last set."""
        self._chk(self.L.yh_fp8_calibrate(self.h))

    def fp8_layers(self):
        """[(conv name, activation scale)] of the convolutions that read E4M3 operands, in execution order."""
        out = []
        for i in range(self.L.yh_fp8_layer_count(self.h)):
            name, sc = C.c_char_p(), C.c_float()
            self._chk(self.L.yh_fp8_layer_info(self.h, i, C.byref(name), C.byref(sc)))
            out.append((name.value.decode(), sc.value))
        return out

    def fp8_set_layer_scale(self, i, scale):
        """One number: the same scale in every channel of layer i's input tensor; an array: one per channel."""
        if np.ndim(scale) == 0:
            self._chk(self.L.yh_fp8_set_layer_scale(self.h, i, C.c_float(scale)))
        else:
            v = np.ascontiguousarray(scale, np.float32)
            self._chk(self.L.yh_fp8_set_layer_channel_scales(self.h, i, _p(v), int(v.size)))

    def fp8_channel_scales(self):
        """[(conv name, per-input-channel activation scales as an f32 array)] of the E4M3 convolutions, in execution order -
        what the oracle's fp8 forward mode is given (oracle.Net.set_fp8) and what a host stores with the model."""
        out = []
        for i, (name, _) in enumerate(self.fp8_layers()):
            nc = self.L.yh_fp8_layer_channels(self.h, i)
            if nc < 1:
                raise YhError(nc, "yh_fp8_layer_channels")
            v = np.empty(nc, np.float32)
            self._chk(self.L.yh_fp8_layer_channel_scales(self.h, i, _p(v), nc))
            out.append((name, v))
        return out

    def rank_broadcast_weights(self, id_bytes, rank, nranks, root=0):
        """One process per GPU: RCCL broadcast of the root rank's weights (id_bytes from rccl_unique_id on one rank)."""
        buf = C.create_string_buffer(bytes(id_bytes), 128)
        self._chk(self.L.yh_rank_broadcast_weights(self.h, buf, rank, nranks, root))

    # ---- interpreter-shaped surface
    def input_dims(self):
        d = (C.c_int32 * 4)()
        self._chk(self.L.yh_input_dims(self.h, C.byref(d)))
        return tuple(d)

    def set_input(self, rgb):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        n = rgb.shape[0]
        assert rgb.shape == (n, self.S, self.S, 3), rgb.shape
        self._chk(self.L.yh_set_input_u8(self.h, _p(rgb), n))
        self.n = n

    def set_input_device(self, dev_ptr, n):
        self._chk(self.L.yh_set_input_u8_device(self.h, C.c_void_p(dev_ptr), n))
        self.n = n

    def invoke(self):
        self._chk(self.L.yh_invoke(self.h))

    def evaluate(self):
        self._chk(self.L.yh_evaluate(self.h))

    def set_cu_mask(self, n_cus, total=256, offset=0):
        """Study hook: the handle's compute streams on CUs offset .. offset + n_cus - 1 of `total` (yh_debug_set_cu_mask)."""
        words = (total + 31) // 32
        m = (C.c_uint32 * words)()
        for i in range(offset, offset + n_cus):
            m[i // 32] |= 1 << (i % 32)
        self._chk(self.L.yh_debug_set_cu_mask(self.h, C.cast(m, C.c_void_p), words))

    def run_phase(self, phase, reps=1):
        """Study hook: device ms of `reps` runs of one phase of the forward (yh_debug_run_phase)."""
        ms = C.c_float()
        self._chk(self.L.yh_debug_run_phase(self.h, phase, reps, C.byref(ms)))
        return ms.value

    def prepare(self, n, with_tail=True):
        """yh_prepare: capture the step for n frames now, on this thread (allocate_tensors() at its proper time)."""
        self._chk(self.L.yh_prepare(self.h, n, 1 if with_tail else 0))

    def sync(self):
        self._chk(self.L.yh_sync(self.h))

    def output_count(self):
        return self.L.yh_output_count(self.h)

    def output_info(self, i):
        ti = TensorInfo()
        self._chk(self.L.yh_output_info(self.h, i, C.byref(ti)))
        return dict(name=ti.name.decode(), kind=ti.kind, dims=tuple(ti.dims[:ti.ndims]), scale=ti.scale,
                    zero_point=ti.zero_point)

    def output(self, i):
        info = self.output_info(i)
        out = np.empty(info["dims"], np.float32)
        self._chk(self.L.yh_output_read_f32(self.h, i, _p(out), out.size))
        return out

    def priors(self):
        out = np.empty((self.P, 4), np.float32)
        self._chk(self.L.yh_read_priors(self.h, _p(out), out.size))
        return out

    def detections(self, frame, want_masks=True):
        nd = C.c_int32()
        dets = (Detection * self.cfg.max_dets)()
        masks = np.zeros((self.cfg.max_dets, self.hp, self.wp), np.uint8) if want_masks else None
        self._chk(self.L.yh_read_detections(self.h, frame, C.byref(nd), C.cast(dets, C.c_void_p), self.cfg.max_dets,
                                            _p(masks) if want_masks else None, masks.size if want_masks else 0))
        out = [dict(class_id=d.class_id, prior=d.prior, score=d.score, box=tuple(d.box)) for d in dets[:nd.value]]
        return out, (masks[:nd.value] if want_masks else None)

    def flops_per_frame(self):
        return self.L.yh_flops_per_frame(self.h)

    # ---- instance frame (DESIGN.md §11 "Instance frame")
    def _class_map(self, class_map):
        if class_map is None:
            return None
        cm = np.ascontiguousarray(class_map, np.uint8)
        assert cm.shape == (self.cfg.num_classes - 1,), "class_map: one value per foreground class"
        return cm

    def instance_frame(self, frame, width, height, class_map=None, min_score=0.0, read=True):
        """yh_instance_frame: the detections of frame `frame` of the last evaluate painted into a height x width uint32 frame of
        class << 24 | id << 16 on the device (instance_device_frame; the table: instances). class_map: uint8 [num_classes - 1] with
        values 0..3, None: the reference's model (foreground 0, 1, 2 -> 1, 2, 3). read=False leaves the frame on the device."""
        cm = self._class_map(class_map)
        out = np.zeros((height, width), np.uint32) if read else None
        self._chk(self.L.yh_instance_frame(self.h, frame, width, height, _p(cm) if cm is not None else None, C.c_float(min_score),
                                           _p(out) if read else None))
        return out

    def instance_device_frame(self):
        """Device pointer of the last instance frame (for Scene.append_classified(..., mode=COMPAT_SANE)); None before one."""
        return self.L.yh_instance_device_frame(self.h)

    def instances(self):
        """The last instance frame's table: int32 [m][4] = (detection rank, output class, id, pixels won)."""
        n = C.c_int32()
        self._chk(self.L.yh_instance_read(self.h, C.byref(n), None, 0))
        t = np.zeros((n.value, 4), np.int32)
        self._chk(self.L.yh_instance_read(self.h, C.byref(n), _p(t), n.value))
        return t

    def op_instance_frame(self, masks, class_ids, scores, width, height, class_map=None, min_score=0.0):
        """yh_op_instance_frame: the instance frame's kernels on caller-provided masks uint8 [n][hp][wp], class ids and scores in
        rank order. Returns (frame uint32 [height][width], table int32 [m][4])."""
        masks = np.ascontiguousarray(masks, np.uint8)
        n, hp, wp = masks.shape
        ids = np.ascontiguousarray(class_ids, np.int32).reshape(n)
        sc = np.ascontiguousarray(scores, np.float32).reshape(n)
        cm = self._class_map(class_map)
        out = np.zeros((height, width), np.uint32)
        table = np.zeros((self.cfg.max_dets, 4), np.int32)
        m = C.c_int32()
        self._chk(self.L.yh_op_instance_frame(self.h, _p(masks), _p(ids), _p(sc), n, hp, wp, width, height,
                                              _p(cm) if cm is not None else None, C.c_float(min_score), _p(out), _p(table),
                                              len(table), C.byref(m)))
        return out, table[:m.value].copy()

    # ---- instance batch (DESIGN.md §11 "Instance batch")
    def instance_batch(self, first, n, width, height, class_map=None, min_score=0.0, read=True):
        """yh_instance_batch: frames first .. first + n - 1 of the last evaluate painted in one pair of launches; frame b equals
        instance_frame(first + b, ...). Returns uint32 [n][height][width], or None with read=False (the frames stay on the device:
        instance_batch_device_frames; the tables: instances_of)."""
        cm = self._class_map(class_map)
        out = np.zeros((max(n, 0), height, width), np.uint32) if read else None
        self._chk(self.L.yh_instance_batch(self.h, first, n, width, height, _p(cm) if cm is not None else None, C.c_float(min_score),
                                           _p(out) if read else None))
        return out

    def instance_batch_device_frames(self):
        """Device pointer of the last batch's frames [n][height][width] (for SceneBatch.stage_frames); None before one."""
        return self.L.yh_instance_batch_device_frames(self.h)

    def instances_of(self, b):
        """The instance table of frame b of the last batch: int32 [m][4] = (detection rank, output class, id, pixels won)."""
        n = C.c_int32()
        self._chk(self.L.yh_instance_batch_read(self.h, b, C.byref(n), None, 0))
        t = np.zeros((n.value, 4), np.int32)
        self._chk(self.L.yh_instance_batch_read(self.h, b, C.byref(n), _p(t), n.value))
        return t

    def op_instance_batch(self, masks, class_ids, scores, counts, width, height, class_map=None, min_score=0.0):
        """yh_op_instance_batch: the batch's kernels on caller-provided masks uint8 [n_frames][n_dets][hp][wp], class ids and scores
        [n_frames][n_dets] in rank order per frame, counts [n_frames]. Returns (frames uint32 [n_frames][height][width], the list of
        the frames' tables)."""
        masks = np.ascontiguousarray(masks, np.uint8)
        nf, nd, hp, wp = masks.shape
        ids = np.ascontiguousarray(class_ids, np.int32).reshape(nf, nd)
        sc = np.ascontiguousarray(scores, np.float32).reshape(nf, nd)
        cnt = np.ascontiguousarray(counts, np.int32).reshape(nf)
        cm = self._class_map(class_map)
        out = np.zeros((nf, height, width), np.uint32)
        self._chk(self.L.yh_op_instance_batch(self.h, _p(masks), _p(ids), _p(sc), _p(cnt), nf, nd, hp, wp, width, height,
                                              _p(cm) if cm is not None else None, C.c_float(min_score), _p(out)))
        return out, [self.instances_of(b) for b in range(nf)]

    # ---- instance tracks (DESIGN.md §11 "Instance tracks")
    @staticmethod
    def _permille(min_iou):
        return int(round(float(min_iou) * 1000.0))

    def instance_track(self, frame, width, height, class_map=None, min_score=0.0, min_iou=0.3, max_age=2, read=True):
        """yh_instance_track: instance_frame with ids that persist - the detections are matched to the handle's tracker by mask
        overlap (IoU >= min_iou, rounded to per-mille), a track that is not seen lives max_age further calls. The instance table
        (instances) carries the track ids; the tracker itself: tracks."""
        cm = self._class_map(class_map)
        out = np.zeros((height, width), np.uint32) if read else None
        self._chk(self.L.yh_instance_track(self.h, frame, width, height, _p(cm) if cm is not None else None, C.c_float(min_score),
                                           self._permille(min_iou), int(max_age), _p(out) if read else None))
        return out

    def tracks(self):
        """The tracker after the last tracked call: int32 [m][6] = (slot, output class, id, age, area, rank or -1)."""
        n = C.c_int32()
        self._chk(self.L.yh_instance_tracks_read(self.h, C.byref(n), None, 0))
        t = np.zeros((n.value, 6), np.int32)
        self._chk(self.L.yh_instance_tracks_read(self.h, C.byref(n), _p(t), n.value))
        return t

    def track_reset(self, stream=0):
        """yh_instance_track_reset_stream: an empty tracker for one stream of the bank (0: instance_track's), None: for all."""
        self._chk(self.L.yh_instance_track_reset_stream(self.h, -1 if stream is None else int(stream)))

    def op_instance_track(self, masks, class_ids, scores, width, height, class_map=None, min_score=0.0, min_iou=0.3, max_age=2):
        """yh_op_instance_track: a tracked call on caller-provided masks uint8 [n][hp][wp], class ids and scores in rank order;
        successive calls form the sequence. Returns (frame uint32 [height][width], instance table int32 [m][4])."""
        masks = np.ascontiguousarray(masks, np.uint8)
        n, hp, wp = masks.shape
        ids = np.ascontiguousarray(class_ids, np.int32).reshape(n)
        sc = np.ascontiguousarray(scores, np.float32).reshape(n)
        cm = self._class_map(class_map)
        out = np.zeros((height, width), np.uint32)
        table = np.zeros((self.cfg.max_dets, 4), np.int32)
        m = C.c_int32()
        self._chk(self.L.yh_op_instance_track(self.h, _p(masks), _p(ids), _p(sc), n, hp, wp, width, height,
                                              _p(cm) if cm is not None else None, C.c_float(min_score), self._permille(min_iou),
                                              int(max_age), _p(out), _p(table), len(table), C.byref(m)))
        return out, table[:m.value].copy()

    # ---- instance track batch (DESIGN.md §11 "Instance track batch")
    @staticmethod
    def _streams(streams, n):
        if streams is None:
            return None
        st = np.ascontiguousarray(streams, np.int32)
        assert st.shape == (n,), "streams: one value per frame"
        return st

    def instance_track_batch(self, first, n, width, height, class_map=None, min_score=0.0, min_iou=0.3, max_age=2, streams=None,
                             read=True):
        """yh_instance_track_batch: frames first .. first + n - 1 of the last evaluate tracked with one wait; frame b is what
        instance_track(first + b, ...) gives on the tracker of streams[b] (None: all on stream 0, instance_track's), the calls made
        in batch order. A tracked batch is an instance batch: returns uint32 [n][height][width], or None with read=False
        (instance_batch_device_frames; the tables: instances_of; the trackers: tracks_of)."""
        cm = self._class_map(class_map)
        st = self._streams(streams, n)
        out = np.zeros((max(n, 0), height, width), np.uint32) if read else None
        self._chk(self.L.yh_instance_track_batch(self.h, first, n, width, height, _p(cm) if cm is not None else None,
                                                 C.c_float(min_score), self._permille(min_iou), int(max_age),
                                                 _p(st) if st is not None else None, _p(out) if read else None))
        return out

    def tracks_of(self, b):
        """The tracker of frame b's stream right after frame b of the last tracked batch: int32 [m][6] = (slot, output class, id,
        age, area, rank or -1)."""
        n = C.c_int32()
        self._chk(self.L.yh_instance_track_batch_read(self.h, b, C.byref(n), None, 0))
        t = np.zeros((n.value, 6), np.int32)
        self._chk(self.L.yh_instance_track_batch_read(self.h, b, C.byref(n), _p(t), n.value))
        return t

    def op_instance_track_batch(self, masks, class_ids, scores, counts, width, height, class_map=None, min_score=0.0, min_iou=0.3,
                                max_age=2, streams=None):
        """yh_op_instance_track_batch: a tracked batch on caller-provided masks uint8 [n_frames][n_dets][hp][wp], class ids and scores
        [n_frames][n_dets] in rank order per frame, counts [n_frames], against the handle's bank of trackers. Returns (frames uint32
        [n_frames][height][width], the list of the frames' instance tables, the list of their track tables)."""
        masks = np.ascontiguousarray(masks, np.uint8)
        nf, nd, hp, wp = masks.shape
        ids = np.ascontiguousarray(class_ids, np.int32).reshape(nf, nd)
        sc = np.ascontiguousarray(scores, np.float32).reshape(nf, nd)
        cnt = np.ascontiguousarray(counts, np.int32).reshape(nf)
        cm = self._class_map(class_map)
        st = self._streams(streams, nf)
        out = np.zeros((nf, height, width), np.uint32)
        self._chk(self.L.yh_op_instance_track_batch(self.h, _p(masks), _p(ids), _p(sc), _p(cnt), nf, nd, hp, wp, width, height,
                                                    _p(cm) if cm is not None else None, C.c_float(min_score), self._permille(min_iou),
                                                    int(max_age), _p(st) if st is not None else None, _p(out)))
        return out, [self.instances_of(b) for b in range(nf)], [self.tracks_of(b) for b in range(nf)]

    # ---- reference-compat path
    def classify_device_frame(self):
        """Device pointer of the frame the last classify_frame produced (for Scene.append_classified)."""
        return self.L.yh_classify_device_frame(self.h)

    def classify_frame(self, frame_u32, width, height, mode=COMPAT_STRICT):
        """In place on a C-contiguous uint32 array of width*height packed pixels."""
        assert frame_u32.dtype == np.uint32 and frame_u32.flags.c_contiguous and frame_u32.size == width * height
        self._chk(self.L.yh_classify_frame_u32(self.h, _p(frame_u32), width, height, mode))

    def classify_batch(self, frames_u32=None, frames_dev_ptr=None, n=None, width=640, height=480, mode=COMPAT_STRICT, out=True):
        """yh_classify_batch_u32: classify on n frames as one step of 2n tiles (DESIGN.md §11 "Classify batch"). frames_u32: uint32
        [n][height][width] on the host (n defaults to its first dimension), or frames_dev_ptr: a device pointer to the same layout
        with n given. out: True (a new array), False (nothing is copied back) or the uint32 array to write, which may be frames_u32
        itself. Returns (frames uint32 [n][height][width], or None with out=False; diverged int32 [n]). On YH_EDIVERGE the
        YhError carries the flags as .diverged. The device copy: classify_batch_device_frames."""
        assert (frames_u32 is None) != (frames_dev_ptr is None), "give frames_u32 or frames_dev_ptr"
        if frames_u32 is not None:
            src = np.ascontiguousarray(frames_u32, np.uint32)
            if n is None:
                n = src.shape[0]
            assert src.size >= max(int(n), 0) * width * height, (src.shape, n, width, height)
            ptr, on_dev = _p(src), 0
        else:
            assert n is not None, "frames_dev_ptr needs n"
            ptr, on_dev = C.c_void_p(frames_dev_ptr), 1
        if isinstance(out, np.ndarray):   # the array to write (it may be frames_u32 itself: in place)
            assert out.dtype == np.uint32 and out.flags.c_contiguous and out.size == int(n) * width * height
            res = out
        else:
            res = np.zeros((max(int(n), 0), height, width), np.uint32) if out else None
        div = np.zeros(max(int(n), 1), np.int32)
        try:
            self._chk(self.L.yh_classify_batch_u32(self.h, ptr, on_dev, int(n), width, height, mode,
                                                   _p(res) if res is not None else None, _p(div)))
        except YhError as e:
            e.diverged = div[:max(int(n), 0)].copy()
            raise
        return res, div[:int(n)]

    def classify_batch_device_frames(self):
        """Device pointer of the last classify_batch's frames [n][height][width] (None before a batch or after a failed one): what
        SceneBatch.stage_frames(frames_dev_ptr=...) takes."""
        return self.L.yh_classify_batch_device_frames(self.h)

    def op_classify_pre_batch(self, frames_u32, width, height):
        """yh_op_classify_pre_batch: the batch's pre kernel alone on uint32 [n][height][width]. Returns (tiles uint8 [2n][S][S][3],
        form: 0 the LDS form, 1 the fallback)."""
        src = np.ascontiguousarray(frames_u32, np.uint32)
        n = src.size // (width * height)
        assert src.size == n * width * height
        tiles = np.zeros((2 * n, self.S, self.S, 3), np.uint8)
        form = C.c_int32(-1)
        self._chk(self.L.yh_op_classify_pre_batch(self.h, _p(src), n, width, height, _p(tiles), C.byref(form)))
        return tiles, form.value

    def op_classify_post_batch(self, cells, width, height, mode=COMPAT_STRICT, out=None):
        """yh_op_classify_post_batch: cells_postprocess and the batch's post kernel on float32 [2n][cells][C] logits. Returns
        (frames uint32 [n][height][width], diverged int32 [n]); `out`, if given, is the array written (left untouched on
        YH_EDIVERGE, where the YhError carries the flags as .diverged)."""
        cells = np.ascontiguousarray(cells, np.float32)
        n = cells.shape[0] // 2
        res = out if out is not None else np.zeros((n, height, width), np.uint32)
        assert res.dtype == np.uint32 and res.flags.c_contiguous and res.size == n * width * height
        div = np.zeros(max(n, 1), np.int32)
        try:
            self._chk(self.L.yh_op_classify_post_batch(self.h, _p(cells), n, width, height, mode, _p(res), _p(div)))
        except YhError as e:
            e.diverged = div[:n].copy()
            raise
        return res, div[:n]

    def postprocess_cells(self, cells, mode=COMPAT_STRICT):
        cells = np.ascontiguousarray(cells, np.float32)
        n = cells.shape[0]
        out = np.zeros((n, self.S, self.S), np.uint32)
        self._chk(self.L.yh_postprocess_cells(self.h, _p(cells), n, _p(out), mode))
        return out

    def resize_triangle(self, src, dw, dh):
        src = np.ascontiguousarray(src, np.uint8)
        sh, sw = src.shape[:2]
        out = np.empty((dh, dw, 3), np.uint8)
        self._chk(self.L.yh_resize_triangle_rgb8(self.h, _p(src), sw, sh, _p(out), dw, dh))
        return out

    def tensor(self, name):
        """Named intermediate of the last forward as f32 NHWC (test hook)."""
        d = (C.c_int32 * 4)()
        self._chk(self.L.yh_debug_read_tensor(self.h, name.encode(), None, 0, C.byref(d)))
        out = np.empty(tuple(d), np.float32)
        self._chk(self.L.yh_debug_read_tensor(self.h, name.encode(), _p(out), out.size, C.byref(d)))
        return out

    def tensor_frame(self, name, frame):
        """One frame of a named intermediate as f32 [h][w][c] (test hook)."""
        d = (C.c_int32 * 4)()
        self._chk(self.L.yh_debug_read_tensor_frame(self.h, name.encode(), frame, None, 0, C.byref(d)))
        out = np.empty(tuple(d)[1:], np.float32)
        self._chk(self.L.yh_debug_read_tensor_frame(self.h, name.encode(), frame, _p(out), out.size, C.byref(d)))
        return out

    def tensor_e4m3(self, name, frame):
        """One frame of a named intermediate's E4M3 twin as raw codes, uint8 [h][w][c] (test hook; YhError ESTATE where the fp8 plan
        does not write that form)."""
        d = (C.c_int32 * 4)()
        self._chk(self.L.yh_debug_read_tensor_e4m3(self.h, name.encode(), frame, None, 0, C.byref(d)))
        out = np.empty(tuple(d)[1:], np.uint8)
        self._chk(self.L.yh_debug_read_tensor_e4m3(self.h, name.encode(), frame, _p(out), out.size, C.byref(d)))
        return out

    def fp8_weights(self, layer_index):
        """(codes uint8 [cout][k*k*cin], s_w f32 [cout]) of E4M3 layer layer_index as its kernel reads them (test hook)."""
        d = (C.c_int32 * 2)()
        self._chk(self.L.yh_debug_fp8_weights(self.h, layer_index, None, None, C.byref(d)))
        codes, sw = np.empty((d[0], d[1]), np.uint8), np.empty(d[0], np.float32)
        self._chk(self.L.yh_debug_fp8_weights(self.h, layer_index, _p(codes), _p(sw), C.byref(d)))
        return codes, sw

    # ---- measurement hooks
    def profile(self, with_tail=True, reps=5):
        nl = self.L.yh_profile_launch_count(self.h, 1 if with_tail else 0)
        ms = np.zeros(nl, np.float32)
        fl = np.zeros(nl, np.float64)
        by = np.zeros(nl, np.float64)
        names = (C.c_char_p * nl)()
        self._chk(self.L.yh_profile_run(self.h, 1 if with_tail else 0, reps, _p(ms), _p(fl), _p(by), C.cast(names, C.c_void_p)))
        return [dict(name=names[i].decode(), ms=float(ms[i]), flops=float(fl[i]), bytes=float(by[i])) for i in range(nl)]

    def time_steps(self, steps, with_tail=True):
        ms = C.c_float()
        self._chk(self.L.yh_time_steps(self.h, 1 if with_tail else 0, steps, C.byref(ms)))
        return ms.value

    def alloc_map(self):
        """Audit hook: one text line per buffer of the handle (base, end, size, offsets inside their 2 MiB pages)."""
        buf = C.create_string_buffer(1 << 20)
        self._chk(self.L.yh_debug_alloc_map(self.h, buf, len(buf)))
        return buf.value.decode()

    def graph_nodes(self, with_tail=True):
        """Audit hook: the captured step for the current batch size, one sorted text line per graph node."""
        buf = C.create_string_buffer(1 << 20)
        self._chk(self.L.yh_debug_graph_nodes(self.h, 1 if with_tail else 0, buf, len(buf)))
        return buf.value.decode()

    def guard_selfcheck(self, where):
        """The single-op entry points' guard check on a staged output with one guard byte changed (where 1 .. 4; 0: none): raises
        YhError(EOVERFLOW) naming the output, the side and the byte; no kernel runs."""
        self._chk(self.L.yh_debug_guard_selfcheck(self.h, where))

    def act_paint(self, first_image):
        """0xFF into images first_image .. max_batch - 1 of every activation allocation (and E4M3 twin)."""
        self._chk(self.L.yh_debug_act_paint(self.h, first_image))

    def act_check(self, first_image):
        """The painted images are still 0xFF and every allocation's 256 trailing bytes zero, or YhError(EOVERFLOW) whose `offenders`
        lists up to nine changed bytes, one line each."""
        buf = C.create_string_buffer(1 << 14)
        rc = self.L.yh_debug_act_check(self.h, first_image, buf, len(buf))
        if rc != OK:
            err = YhError(rc, self.L.yh_last_error(self.h).decode())
            err.offenders = buf.value.decode().splitlines()
            raise err

    def last_conv_launches(self):
        return self.L.yh_debug_last_conv_launches(self.h)

    def last_conv_forms(self):
        """The kernels the last single-op conv call launched, in order: [(tile id, form name)]; a split-K call ends with (-1, "REDUCE")."""
        n = self.L.yh_debug_last_conv_forms(self.h, None, 0)
        pairs = np.zeros((max(n, 1), 2), np.int32)
        self.L.yh_debug_last_conv_forms(self.h, _p(pairs), n)
        return [(int(t), CONV_FORM_NAMES[f]) for t, f in pairs[:n]]

    # ---- single ops (tests)
    def op_conv2d(self, x, w, bias, stride=1, pad=0, residual=None, act=0):
        n, hh, ww, cin = x.shape
        cout, kh, kw, _ = w.shape
        ho, wo = (hh + 2 * pad - kh) // stride + 1, (ww + 2 * pad - kw) // stride + 1
        xb, wb = _f16_bits(x), _f16_bits(w)
        bias = np.ascontiguousarray(bias, np.float32)
        rb = _f16_bits(residual) if residual is not None else None
        y = np.zeros((n, ho, wo, cout), np.uint16)
        self._chk(self.L.yh_op_conv2d_f16(self.h, _p(xb), n, hh, ww, cin, _p(wb), _p(bias), cout, kh, kw, stride, pad,
                                          _p(rb) if rb is not None else None, act, _p(y)))
        return _bits_f32(y, y.shape)

    def op_bilinear(self, x, ho, wo):
        n, hh, ww, c = x.shape
        xb = _f16_bits(x)
        y = np.zeros((n, ho, wo, c), np.uint16)
        self._chk(self.L.yh_op_bilinear_f16(self.h, _p(xb), n, hh, ww, c, ho, wo, _p(y)))
        return _bits_f32(y, y.shape)

    def op_maxpool(self, x):
        n, hh, ww, c = x.shape
        ho, wo = (hh + 2 - 3) // 2 + 1, (ww + 2 - 3) // 2 + 1
        xb = _f16_bits(x)
        y = np.zeros((n, ho, wo, c), np.uint16)
        self._chk(self.L.yh_op_maxpool3x3s2_f16(self.h, _p(xb), n, hh, ww, c, _p(y)))
        return _bits_f32(y, y.shape)

    def op_conv2d_dual(self, x1, x2, stride2, w, bias, act=0):
        """The two-source 1x1 conv: x1 [n][ho][wo][c1], x2 [n][h2][w2][c2] read at stride2, w [cout][c1 + c2] -> [n][ho][wo][cout] f32."""
        n, ho, wo, c1 = x1.shape
        _, h2, w2, c2 = x2.shape
        cout = w.shape[0]
        assert w.shape[1] == c1 + c2
        x1b, x2b, wb = _f16_bits(x1), _f16_bits(x2), _f16_bits(w)
        bias = np.ascontiguousarray(bias, np.float32)
        y = np.zeros((n, ho, wo, cout), np.uint16)
        self._chk(self.L.yh_op_conv2d_dual_f16(self.h, _p(x1b), n, ho, wo, c1, _p(x2b), h2, w2, c2, stride2, _p(wb), _p(bias), cout, act, _p(y)))
        return y.view(np.float16).astype(np.float32)

    def op_bneck(self, planes, tile_m, a, w3, bias3, w2=None, bias2=None, stride=1, res=None, x2=None, stride2=1, w1n=None, bias1n=None,
                 want_a_next=None, inv_scale=None):
        """One launch of csrc/bneck.hip (yh_op_bneck_f16): a [n][H][W][planes], w2 [planes][3][3][planes], w3 [4 planes][planes (+ 64)],
        res [n][P][Q][4 planes] or x2 [n][H2][W2][64] at stride2, w1n [planes][4 planes]; planes 256: a is b, inv_scale [256] asks for the
        E4M3 codes of a'. want_a_next (default: w1n given) asks for a' as f16. -> dict(y [n][P][Q][4 planes] f32, a_next f32 or None,
        a_next8 uint8 or None)."""
        n, hh, ww, _ = a.shape
        P, Q = (hh, ww) if planes == 256 else ((hh - 1) // stride + 1, (ww - 1) // stride + 1)
        f = lambda v: None if v is None else _f16_bits(v)
        g = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
        q = lambda v: None if v is None else _p(v)
        ab, w2b, w3b, rb, x2b, w1b = f(a), f(w2), f(w3), f(res), f(x2), f(w1n)
        b2, b3, b1, inv = g(bias2), g(bias3), g(bias1n), g(inv_scale)
        if want_a_next is None:
            want_a_next = w1n is not None
        y = np.zeros((n, P, Q, 4 * planes), np.uint16)
        an = np.zeros((n, P, Q, planes), np.uint16) if want_a_next else None
        a8 = np.zeros((n, P, Q, planes), np.uint8) if inv is not None else None
        h2, w2w = (x2.shape[1], x2.shape[2]) if x2 is not None else (0, 0)
        self._chk(self.L.yh_op_bneck_f16(self.h, planes, tile_m, q(ab), n, hh, ww, q(w2b), q(b2), stride, q(w3b), q(b3), q(rb), q(x2b), h2, w2w,
                                         stride2, q(w1b), q(b1), q(y), q(an), q(a8), q(inv)))
        return dict(y=_bits_f32(y, y.shape), a_next=None if an is None else _bits_f32(an, an.shape), a_next8=a8)

    def op_conv2d_levels(self, x, level_sizes, w, bias, act=0):
        """x [n][cells][cin] with cells = sum(s*s for s in level_sizes); w [cout][k][k][cin] -> [n][cells][cout] f32."""
        n, cells, cin = x.shape
        cout, k = w.shape[0], w.shape[1]
        ls = np.ascontiguousarray(level_sizes, np.int32)
        assert cells == int((ls.astype(np.int64) ** 2).sum())
        xb, wb = _f16_bits(x), _f16_bits(w)
        bias = np.ascontiguousarray(bias, np.float32)
        y = np.zeros((n, cells, cout), np.uint16)
        self._chk(self.L.yh_op_conv2d_levels_f16(self.h, _p(xb), n, _p(ls), len(ls), cin, _p(wb), _p(bias), cout, k, act, _p(y)))
        return y.view(np.float16).astype(np.float32)

    def op_stem_pool(self, x, w, bias, want_stem=True):
        """x [n][S][S][3], w [64][7][7][3] (f16-representable f32) -> (stem or None, pool) as f32 NHWC."""
        n, S = x.shape[0], x.shape[1]
        so = (S + 6 - 7) // 2 + 1
        po = (so + 2 - 3) // 2 + 1
        xb, wb = _f16_bits(x), _f16_bits(w)
        bias = np.ascontiguousarray(bias, np.float32)
        stem = np.zeros((n, so, so, 64), np.uint16) if want_stem else None
        pool = np.zeros((n, po, po, 64), np.uint16)
        self._chk(self.L.yh_op_stem_pool_f16(self.h, _p(xb), n, S, _p(wb), _p(bias), _p(stem) if want_stem else None, _p(pool)))
        f = lambda a: a.view(np.float16).astype(np.float32)
        return (f(stem) if want_stem else None), f(pool)

    def op_stem_pool_rgb8(self, rgb, w, bias, want_stem=True):
        """rgb [n][S][S][3] uint8 (preprocessing fused into the kernel) -> (stem or None, pool) as f32 NHWC."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        n, S = rgb.shape[0], rgb.shape[1]
        so = (S + 6 - 7) // 2 + 1
        po = (so + 2 - 3) // 2 + 1
        wb = _f16_bits(w)
        bias = np.ascontiguousarray(bias, np.float32)
        stem = np.zeros((n, so, so, 64), np.uint16) if want_stem else None
        pool = np.zeros((n, po, po, 64), np.uint16)
        self._chk(self.L.yh_op_stem_pool_rgb8(self.h, _p(rgb), n, S, _p(wb), _p(bias), _p(stem) if want_stem else None, _p(pool)))
        f = lambda a: a.view(np.float16).astype(np.float32)
        return (f(stem) if want_stem else None), f(pool)

    def op_conv2d_fp8(self, x_codes, w_codes, scale, bias, stride=1, pad=0, residual=None, act=0, reps=0):
        """x_codes [n][h][w][cin] / w_codes [cout][k][k][cin]: uint8 E4M3 codes -> (y f32 NHWC, ms per launch or None)."""
        n, hh, ww, cin = x_codes.shape
        cout, k = w_codes.shape[0], w_codes.shape[1]
        ho, wo = (hh + 2 * pad - k) // stride + 1, (ww + 2 * pad - k) // stride + 1
        xc, wc = np.ascontiguousarray(x_codes, np.uint8), np.ascontiguousarray(w_codes, np.uint8)
        sc, bs = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(bias, np.float32)
        rb = _f16_bits(residual) if residual is not None else None
        y = np.zeros((n, ho, wo, cout), np.uint16)
        ms = C.c_float(0)
        self._chk(self.L.yh_op_conv2d_fp8(self.h, _p(xc), n, hh, ww, cin, _p(wc), _p(sc), _p(bs), cout, k, stride, pad,
                                          _p(rb) if rb is not None else None, act, _p(y), reps, C.byref(ms) if reps else None))
        return y.view(np.float16).astype(np.float32), (ms.value if reps else None)

    def op_conv2d_levels_fp8(self, x_codes, level_sizes, w_codes, scale, bias, act=0):
        """op_conv2d_levels with E4M3 codes: x_codes [n][cells][cin], w_codes [cout][k][k][cin] uint8 -> [n][cells][cout] f32."""
        n, cells, cin = x_codes.shape
        cout, k = w_codes.shape[0], w_codes.shape[1]
        ls = np.ascontiguousarray(level_sizes, np.int32)
        assert cells == int((ls.astype(np.int64) ** 2).sum())
        xc, wc = np.ascontiguousarray(x_codes, np.uint8), np.ascontiguousarray(w_codes, np.uint8)
        sc, bs = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(bias, np.float32)
        y = np.zeros((n, cells, cout), np.uint16)
        self._chk(self.L.yh_op_conv2d_levels_fp8(self.h, _p(xc), n, _p(ls), len(ls), cin, _p(wc), _p(sc), _p(bs), cout, k, act, _p(y)))
        return y.view(np.float16).astype(np.float32)

    def op_conv2d_resup(self, x, w, bias, res_lo, act=0):
        """The FPN lateral: x [n][P][Q][cin], w [cout][cin] (or [cout][1][1][cin]), res_lo [n][rh][rw][cout] resized to P x Q in the
        conv's epilogue and added -> [n][P][Q][cout] f32."""
        n, P, Q, cin = x.shape
        cout = w.shape[0]
        _, rh, rw, rc = res_lo.shape
        assert rc == cout and w.size == cout * cin and res_lo.shape[0] == n
        xb, wb, rb = _f16_bits(x), _f16_bits(w), _f16_bits(res_lo)
        bias = np.ascontiguousarray(bias, np.float32)
        y = np.zeros((n, P, Q, cout), np.uint16)
        self._chk(self.L.yh_op_conv2d_resup_f16(self.h, _p(xb), n, P, Q, cin, _p(wb), _p(bias), cout, _p(rb), rh, rw, act, _p(y)))
        return _bits_f32(y, y.shape)

    def op_conv2d_tail(self, x, w, bias, w2, bias2, act=1, scale=None):
        """A k x k 'same' conv to 256 channels with the 1x1 conv to 32 channels in its epilogue: x [n][h][w][cin], w [cout][k][k][cin],
        w2 [32][256] -> y2 [n][h][w][32] f32. scale given: x and w are uint8 E4M3 codes (the fp8 tile)."""
        n, hh, ww, cin = x.shape
        cout, k = w.shape[0], w.shape[1]
        w2b = _f16_bits(w2)
        assert w2b.size == 32 * 256
        bias, bias2 = np.ascontiguousarray(bias, np.float32), np.ascontiguousarray(bias2, np.float32)
        y2 = np.zeros((n, hh, ww, 32), np.uint16)
        if scale is None:
            xb, wb = _f16_bits(x), _f16_bits(w)
            self._chk(self.L.yh_op_conv2d_tail_f16(self.h, _p(xb), n, hh, ww, cin, _p(wb), _p(bias), cout, k, act, _p(w2b), _p(bias2), _p(y2)))
        else:
            xc, wc = np.ascontiguousarray(x, np.uint8), np.ascontiguousarray(w, np.uint8)
            sc = np.ascontiguousarray(scale, np.float32)
            self._chk(self.L.yh_op_conv2d_tail_fp8(self.h, _p(xc), n, hh, ww, cin, _p(wc), _p(sc), _p(bias), cout, k, act, _p(w2b), _p(bias2),
                                                   _p(y2)))
        return _bits_f32(y2, y2.shape)

    def op_quantize_e4m3(self, x_f16_bits, inv_scale=1.0):
        """x: uint16 array of f16 bit patterns -> uint8 e4m3 codes of x * inv_scale."""
        xb = np.ascontiguousarray(x_f16_bits, np.uint16)
        y = np.zeros(xb.shape, np.uint8)
        self._chk(self.L.yh_op_quantize_e4m3(self.h, _p(xb), xb.size, C.c_float(inv_scale), _p(y)))
        return y

    def op_absmax_channels_f16(self, x_f16_bits):
        """x: uint16 [rows][C] of f16 bit patterns -> uint32 [C], the bit patterns of max_r |x[r][c]| as f32 (the calibration's kernel)."""
        xb = np.ascontiguousarray(x_f16_bits, np.uint16)
        rows, c = xb.shape
        out = np.zeros(c, np.uint32)
        self._chk(self.L.yh_op_absmax_channels_f16(self.h, _p(xb), rows, c, _p(out)))
        return out

    def op_detect(self, loc, conf, mask, proto):
        n = loc.shape[0]
        lb, cb, mb, pb = _f16_bits(loc), _f16_bits(conf), _f16_bits(mask), _f16_bits(proto)
        self._chk(self.L.yh_op_detect(self.h, _p(lb), _p(cb), _p(mb), _p(pb), n))
        self.n = n


class Group:
    """RAII wrapper of yh_group: one process, one engine per device (devices may repeat), frames sharded in contiguous blocks."""

    def __init__(self, devices, **engine_kw):
        self.L = load_library()
        cfg = Config()
        self.L.yh_default_config(C.byref(cfg))
        kw = dict(input_size=550, backbone=50, max_batch=1, num_classes=81, top_k=200, max_dets=100, conf_thresh=0.05, nms_thresh=0.5,
                  use_graph=True, debug_tensors=False, precision=PRECISION_F16, tune=None, fp8_f16_layers=0, fp8_per_tensor=False)
        unknown = set(engine_kw) - set(kw)
        if unknown:
            raise TypeError(f"Group: unknown engine keyword(s) {sorted(unknown)}")
        kw.update(engine_kw)
        cfg.backbone, cfg.input_size, cfg.max_batch = kw["backbone"], kw["input_size"], kw["max_batch"]
        cfg.num_classes, cfg.top_k, cfg.max_dets = kw["num_classes"], kw["top_k"], kw["max_dets"]
        cfg.conf_thresh, cfg.nms_thresh, cfg.use_graph = kw["conf_thresh"], kw["nms_thresh"], 1 if kw["use_graph"] else 0
        cfg.debug_tensors, cfg.precision = (1 if kw["debug_tensors"] else 0), kw["precision"]
        cfg.fp8_f16_layers, cfg.fp8_per_tensor = kw["fp8_f16_layers"], (1 if kw["fp8_per_tensor"] else 0)
        if kw["tune"]:
            cfg.tune = Tuning.of(**kw["tune"])
        devs = (C.c_int32 * len(devices))(*devices)
        g = C.c_void_p()
        rc = self.L.yh_group_create(C.byref(cfg), devs, len(devices), C.byref(g))
        if rc != OK:
            raise YhError(rc, self.L.yh_group_last_error(None).decode())
        self.g, self.cfg, self.n, self.S, self.max_batch = g, cfg, len(devices), kw["input_size"], kw["max_batch"]
        self.members = []
        for i in range(self.n):                 # non-owning Engine views of the members (the group owns the handles)
            e = Engine.__new__(Engine)
            e.L, e.cfg, e.h, e._tune = self.L, cfg, C.c_void_p(self.L.yh_group_member(self.g, i)), {}
            e.S, e.C, e.max_batch, e.n = kw["input_size"], kw["num_classes"], kw["max_batch"], 0
            e.P = self.L.yh_num_priors(e.h)
            d = (C.c_int32 * 2)()
            self.L.yh_proto_dims(e.h, C.byref(d))
            e.hp, e.wp = d[0], d[1]
            e.close = lambda: None              # never yh_destroy a member
            self.members.append(e)
        self.hp, self.wp = self.members[0].hp, self.members[0].wp

    def close(self):
        if getattr(self, "g", None):
            for e in self.members:
                e.h = None
            self.L.yh_group_destroy(self.g)
            self.g = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            raise YhError(rc, self.L.yh_group_last_error(self.g).decode())

    def load_weights(self, blob):
        blob = np.ascontiguousarray(blob, np.uint8)
        self._chk(self.L.yh_group_load_weights_host(self.g, _p(blob), blob.size))

    def replicate_weights(self):
        self._chk(self.L.yh_group_replicate_weights(self.g))

    def weights_replication(self):
        return self.L.yh_group_weights_replication(self.g).decode()

    def fp8_calibrate(self):
        self._chk(self.L.yh_group_fp8_calibrate(self.g))

    def evaluate(self, frames, with_tail=True):
        frames = np.ascontiguousarray(frames, np.uint8)
        n = frames.shape[0]
        assert frames.shape == (n, self.S, self.S, 3), frames.shape
        self._chk(self.L.yh_group_evaluate(self.g, _p(frames), n, 1 if with_tail else 0))
        self.total = n

    def prepare(self, n_frames, with_tail=True):
        """yh_group_prepare: capture every member's step for a call with n_frames frames, serially on this thread."""
        self._chk(self.L.yh_group_prepare(self.g, n_frames, 1 if with_tail else 0))

    def evaluate_device(self, dev_ptrs, counts, with_tail=True):
        ptrs = (C.c_void_p * self.n)(*[C.c_void_p(p) for p in dev_ptrs])
        cnt = (C.c_int32 * self.n)(*counts)
        self._chk(self.L.yh_group_evaluate_device(self.g, ptrs, cnt, 1 if with_tail else 0))
        self.total = int(sum(counts))

    def sync(self):
        self._chk(self.L.yh_group_sync(self.g))

    def frame_owner(self, frame):
        m, l = C.c_int32(), C.c_int32()
        self._chk(self.L.yh_group_frame_owner(self.g, frame, C.byref(m), C.byref(l)))
        return m.value, l.value

    def detections(self, frame, want_masks=True):
        nd = C.c_int32()
        dets = (Detection * self.cfg.max_dets)()
        masks = np.zeros((self.cfg.max_dets, self.hp, self.wp), np.uint8) if want_masks else None
        self._chk(self.L.yh_group_read_detections(self.g, frame, C.byref(nd), C.cast(dets, C.c_void_p), self.cfg.max_dets,
                                                  _p(masks) if want_masks else None, masks.size if want_masks else 0))
        out = [dict(class_id=d.class_id, prior=d.prior, score=d.score, box=tuple(d.box)) for d in dets[:nd.value]]
        return out, (masks[:nd.value] if want_masks else None)


def scene_motion(dx=0.0, dy=0.0, dtheta=0.0, pivot=None, size=(640, 480)):
    """(gather_q16, carry_q16) for Scene.append_memory, as two lists of six ints, from what the robot did between two frames as the
    map saw it: carry takes a previous-map pixel p to the current-map pixel R(dtheta) (p - pivot) + pivot + (dx, dy) - x to the right,
    y down, dtheta in radians turning x towards y -, gather is its inverse. pivot: the robot's own pixel; None: the start pixel
    (W * 5 / 8, H - 1) of a frame of `size` = (W, H). Coefficients are int(round(v * 65536)). A convenience: where the motion comes
    from (odometry) is the caller's business, and any twelve integers are valid."""
    import math
    px, py = ((size[0] * 5) // 8, size[1] - 1) if pivot is None else pivot
    c, s = math.cos(dtheta), math.sin(dtheta)
    tx, ty = px - c * px + s * py + dx, py - s * px - c * py + dy           # carry: p' = R p + t
    carry = (c, -s, tx, s, c, ty)
    gather = (c, s, -(c * tx + s * ty), -s, c, s * tx - c * ty)             # p = R^T (p' - t)
    q = lambda v: [int(round(x * 65536)) for x in v]
    return q(gather), q(carry)


def scene_motion_candidates(prior=(0.0, 0.0, 0.0), dtheta_step=0.01, n_side=2, pivot=None, size=(640, 480)):
    """(gathers, carries) for Scene.append_memory_search: 2 n_side + 1 rows of six ints each, built with scene_motion. Row 0 is the
    prior (dx, dy, dtheta); rows 1, 2, 3, 4, .. turn it by +1, -1, +2, -2, .. steps of dtheta_step about the pivot. A convenience:
    any rows that pass the call's int32 conditions are valid candidates."""
    dx, dy, dtheta = prior
    steps = [0] + [s * j for j in range(1, n_side + 1) for s in (1, -1)]
    rows = [scene_motion(dx, dy, dtheta + s * dtheta_step, pivot, size) for s in steps]
    return [g for g, _ in rows], [c for _, c in rows]


SCENE_IDENTITY_Q16 = (65536, 0, 0, 0, 65536, 0)


_SCENE_OUTPUTS = ("map", "world", "conn0", "conn1", "balls")   # in the argument order of yh_scene_read / yh_scene_batch_read


def _scene_outputs(W, H, which):
    """Host arrays for the outputs named in `which` (None: all of them)."""
    which = _SCENE_OUTPUTS if which is None else tuple(which)
    if not which or any(k not in _SCENE_OUTPUTS for k in which):
        raise ValueError(f"which: need some of {_SCENE_OUTPUTS}, got {which}")
    shapes = dict(map=((H, W), np.uint32), world=((H, W, 4), np.float32), conn0=((H, W, 4), np.float32), conn1=((H, W, 4), np.float32),
                  balls=((100, 4), np.float32))
    return {k: np.zeros(*shapes[k]) for k in _SCENE_OUTPUTS if k in which}


class Scene:
    """RAII wrapper of yh_scene: append_scene's two compute dispatches (src/scene.rs:147-331) on the GPU."""

    def __init__(self, width=640, height=480, device=0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.yh_scene_create(device, width, height, C.byref(h))
        if rc != OK:
            raise YhError(rc, self.L.yh_scene_last_error(None).decode())
        self.h, self.W, self.H = h, width, height

    def close(self):
        if getattr(self, "h", None):
            self.L.yh_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            raise YhError(rc, self.L.yh_scene_last_error(self.h).decode())

    def append(self, depth, cls_id, mode=COMPAT_STRICT):
        depth = np.ascontiguousarray(depth, np.uint16)
        cls_id = np.ascontiguousarray(cls_id, np.uint8)
        assert depth.shape == (self.H, self.W) and cls_id.shape == (self.H, self.W, 2)
        self._chk(self.L.yh_scene_append(self.h, _p(depth), _p(cls_id), mode))

    def append_classified(self, depth, frame_u32=None, frame_dev_ptr=None, mode=COMPAT_STRICT):
        depth = np.ascontiguousarray(depth, np.uint16)
        assert depth.shape == (self.H, self.W)
        if frame_dev_ptr is not None:
            self._chk(self.L.yh_scene_append_classified(self.h, _p(depth), C.c_void_p(frame_dev_ptr), 1, mode))
        else:
            f = np.ascontiguousarray(frame_u32, np.uint32)
            assert f.size == self.W * self.H
            self._chk(self.L.yh_scene_append_classified(self.h, _p(depth), _p(f), 0, mode))

    def read(self, which=None):
        """The last frame's outputs; `which` names the ones wanted (default: all five) - the others are not copied (yh_scene_read takes nulls)."""
        out = _scene_outputs(self.W, self.H, which)
        self._chk(self.L.yh_scene_read(self.h, *(_p(out[k]) if k in out else None for k in _SCENE_OUTPUTS)))
        return out

    def time(self, reps=20):
        ms = C.c_float()
        self._chk(self.L.yh_scene_time(self.h, reps, C.byref(ms)))
        return ms.value

    def append_memory(self, depth, frame_u32=None, frame_dev_ptr=None, cls_id=None, motion=None, keep=224, ball_max_age=30):
        """A frame fused into the handle's memory (DESIGN.md §11 "Scene memory"): the frame as append_classified(.., COMPAT_SANE) takes
        it - or cls_id, (class, id) bytes [h][w][2], packed here - and motion = (gather_q16, carry_q16), six ints each (scene_motion);
        None: the identity. keep 0 .. 256: how much of a remembered height survives a frame, in 256ths."""
        depth = np.ascontiguousarray(depth, np.uint16)
        assert depth.shape == (self.H, self.W)
        g, c = (SCENE_IDENTITY_Q16, SCENE_IDENTITY_Q16) if motion is None else motion
        g, c = np.array(g, np.int32), np.array(c, np.int32)   # (a value outside int32 raises here)
        assert g.shape == (6,) and c.shape == (6,)
        if frame_dev_ptr is not None:
            self._chk(self.L.yh_scene_append_memory(self.h, _p(depth), C.c_void_p(frame_dev_ptr), 1, _p(g), _p(c), keep, ball_max_age))
            return
        f = SceneBatch.pack(cls_id) if cls_id is not None else np.ascontiguousarray(frame_u32, np.uint32)
        assert f.size == self.W * self.H
        self._chk(self.L.yh_scene_append_memory(self.h, _p(depth), _p(f), 0, _p(g), _p(c), keep, ball_max_age))

    def read_memory(self):
        """The memory as the last memory append left it: map u32 [h][w], balls i32 [100][4] = (x, y, count, age); zeros while empty."""
        out = dict(map=np.zeros((self.H, self.W), np.uint32), balls=np.zeros((100, 4), np.int32))
        self._chk(self.L.yh_scene_memory_read(self.h, _p(out["map"]), _p(out["balls"])))
        return out

    def memory_reset(self):
        self._chk(self.L.yh_scene_memory_reset(self.h))

    def memory_time(self, reps=20):
        ms = C.c_float()
        self._chk(self.L.yh_scene_memory_time(self.h, reps, C.byref(ms)))
        return ms.value

    def append_memory_search(self, depth, frame_u32=None, frame_dev_ptr=None, cls_id=None, candidates=None, radius=4, keep=224, ball_max_age=30):
        """append_memory with the motion found on the device (DESIGN.md §11 "Scene memory: registration"): candidates =
        (gathers, carries), n_rot rows of six ints each, row 0 the prior (scene_motion_candidates); None: the identity alone. Every
        row is tried with every whole-pixel shift of up to `radius` (0 .. 8) either way; read_motion tells which won."""
        depth = np.ascontiguousarray(depth, np.uint16)
        assert depth.shape == (self.H, self.W)
        g, c = ([SCENE_IDENTITY_Q16], [SCENE_IDENTITY_Q16]) if candidates is None else candidates
        g, c = np.ascontiguousarray(np.array(g, np.int32)), np.ascontiguousarray(np.array(c, np.int32))   # (a value outside int32 raises here)
        assert g.ndim == 2 and g.shape[1] == 6 and c.shape == g.shape
        if frame_dev_ptr is not None:
            self._chk(self.L.yh_scene_append_memory_search(self.h, _p(depth), C.c_void_p(frame_dev_ptr), 1, len(g), _p(g), _p(c), radius, keep, ball_max_age))
            self._search = (len(g), radius)
            return
        f = SceneBatch.pack(cls_id) if cls_id is not None else np.ascontiguousarray(frame_u32, np.uint32)
        assert f.size == self.W * self.H
        self._chk(self.L.yh_scene_append_memory_search(self.h, _p(depth), _p(f), 0, len(g), _p(g), _p(c), radius, keep, ball_max_age))
        self._search = (len(g), radius)

    def read_motion(self, scores=False):
        """What the last append_memory_search chose: gather and carry i32 [6], chosen = (k, u, v), score u64 [3] = (S chosen, S of the
        prior, sum_n) and, if asked for, scores u64 [n_rot][2 radius + 1][2 radius + 1], indexed [k][v + radius][u + radius]."""
        out = dict(gather=np.zeros(6, np.int32), carry=np.zeros(6, np.int32), chosen=np.zeros(3, np.int32), score=np.zeros(3, np.uint64))
        table = None
        if scores and getattr(self, "_search", None):
            n_rot, radius = self._search
            table = np.zeros((n_rot, 2 * radius + 1, 2 * radius + 1), np.uint64)
        self._chk(self.L.yh_scene_motion_read(self.h, _p(out["gather"]), _p(out["carry"]), _p(out["chosen"]), _p(out["score"]), _p(table) if table is not None else None))
        if scores:
            out["scores"] = table
        return out

    def op_register(self, n, m, gathers, radius):
        """Test hook (yh_scene_op_register): the registration kernels alone on stamps n and memory m, u32 [h][w]; gathers [n_rot][6].
        Returns (scores u64 [n_rot][2 radius + 1][2 radius + 1], chosen (k, u, v), sum_n); commits nothing."""
        n, m = np.ascontiguousarray(n, np.uint32), np.ascontiguousarray(m, np.uint32)
        assert n.shape == (self.H, self.W) and m.shape == (self.H, self.W)
        g = np.ascontiguousarray(np.array(gathers, np.int32))
        assert g.ndim == 2 and g.shape[1] == 6
        ok = 1 <= len(g) <= 16 and 0 <= radius <= 8   # (otherwise the library refuses before it writes anything)
        scores = np.zeros((len(g), 2 * radius + 1, 2 * radius + 1) if ok else (1,), np.uint64)
        chosen, sum_n = np.zeros(3, np.int32), C.c_uint64()
        self._chk(self.L.yh_scene_op_register(self.h, _p(n), _p(m), len(g), _p(g), radius, _p(scores), _p(chosen), C.byref(sum_n)))
        return scores, tuple(int(v) for v in chosen), sum_n.value

    def memory_search_time(self, reps=20):
        """(ms per frame, ms of the registration alone) of the last append_memory_search, replayed; commits nothing."""
        ms, ms_search = C.c_float(), C.c_float()
        self._chk(self.L.yh_scene_memory_search_time(self.h, reps, C.byref(ms), C.byref(ms_search)))
        return ms.value, ms_search.value

    def append_memory_search_norm(self, depth, frame_u32=None, frame_dev_ptr=None, cls_id=None, candidates=None, radius=4, min_inside=None, keep=224,
                                  ball_max_age=30):
        """append_memory_search with the choice made by the normalised score S / (T - S) over the pixels both maps cover (DESIGN.md §11
        "Scene memory: normalised registration"), for dense maps. candidates and radius as there; min_inside: how many frame pixels
        a candidate must keep inside the frame to qualify, 1 .. W H; None: W H // 4. read_motion works as after append_memory_search,
        read_motion_norm returns the rest."""
        depth = np.ascontiguousarray(depth, np.uint16)
        assert depth.shape == (self.H, self.W)
        g, c = ([SCENE_IDENTITY_Q16], [SCENE_IDENTITY_Q16]) if candidates is None else candidates
        g, c = np.ascontiguousarray(np.array(g, np.int32)), np.ascontiguousarray(np.array(c, np.int32))   # (a value outside int32 raises here)
        assert g.ndim == 2 and g.shape[1] == 6 and c.shape == g.shape
        if min_inside is None:
            min_inside = (self.W * self.H) // 4
        if frame_dev_ptr is not None:
            f, on_device = C.c_void_p(frame_dev_ptr), 1
        else:
            keepalive = SceneBatch.pack(cls_id) if cls_id is not None else np.ascontiguousarray(frame_u32, np.uint32)
            assert keepalive.size == self.W * self.H
            f, on_device = _p(keepalive), 0
        self._chk(self.L.yh_scene_append_memory_search_norm(self.h, _p(depth), f, on_device, len(g), _p(g), _p(c), radius, min_inside, keep, ball_max_age))
        self._search = (len(g), radius)
        self._norm_levels = False

    def read_motion_norm(self):
        """What the last append_memory_search_norm saw beside read_motion's: totals (T) and inside (C), u64 [n_rot][2 radius + 1]
        [2 radius + 1] laid out as read_motion's scores, chosen_stc and prior_stc u64 [3] = (S, T, C) of the choice and of (0, 0, 0),
        and qualified: False if no candidate qualified. After append_memory_pyramid_norm: chosen_stc, prior_stc and qualified alone
        (read_pyramid_norm has the levels' tables)."""
        n_rot, radius = getattr(self, "_search", None) or (1, 0)
        shape = (n_rot, 2 * radius + 1, 2 * radius + 1)
        out = dict(chosen_stc=np.zeros(3, np.uint64), prior_stc=np.zeros(3, np.uint64))
        if not getattr(self, "_norm_levels", False):
            out.update(totals=np.zeros(shape, np.uint64), inside=np.zeros(shape, np.uint64))
        q = C.c_int32()
        t, i = (_p(out[k]) if k in out else None for k in ("totals", "inside"))
        self._chk(self.L.yh_scene_motion_norm_read(self.h, t, i, _p(out["chosen_stc"]), _p(out["prior_stc"]), C.byref(q)))
        out["qualified"] = bool(q.value)
        return out

    def op_register_norm(self, n, m, gathers, radius, min_inside):
        """Test hook (yh_scene_op_register_norm): the normalised registration's kernels alone on stamps n and memory m, u32 [h][w];
        gathers [n_rot][6]. Returns dict(scores, totals, inside: u64 [n_rot][2 radius + 1][2 radius + 1], chosen (k, u, v), qualified,
        sum_n); commits nothing."""
        n, m = np.ascontiguousarray(n, np.uint32), np.ascontiguousarray(m, np.uint32)
        assert n.shape == (self.H, self.W) and m.shape == (self.H, self.W)
        g = np.ascontiguousarray(np.array(gathers, np.int32))
        assert g.ndim == 2 and g.shape[1] == 6
        ok = 1 <= len(g) <= 16 and 0 <= radius <= 8   # (otherwise the library refuses before it writes anything)
        shape = (len(g), 2 * radius + 1, 2 * radius + 1) if ok else (1,)
        out = dict(scores=np.zeros(shape, np.uint64), totals=np.zeros(shape, np.uint64), inside=np.zeros(shape, np.uint64))
        chosen, q, sum_n = np.zeros(3, np.int32), C.c_int32(), C.c_uint64()
        self._chk(self.L.yh_scene_op_register_norm(self.h, _p(n), _p(m), len(g), _p(g), radius, min_inside, _p(out["scores"]), _p(out["totals"]), _p(out["inside"]),
                                                   _p(chosen), C.byref(q), C.byref(sum_n)))
        out.update(chosen=tuple(int(v) for v in chosen), qualified=bool(q.value), sum_n=sum_n.value)
        return out

    def memory_search_norm_time(self, reps=20):
        """(ms per frame, ms of the registration alone) of the last append_memory_search_norm, replayed; commits nothing."""
        ms, ms_search = C.c_float(), C.c_float()
        self._chk(self.L.yh_scene_memory_search_norm_time(self.h, reps, C.byref(ms), C.byref(ms_search)))
        return ms.value, ms_search.value

    def append_memory_pyramid(self, depth, frame_u32=None, frame_dev_ptr=None, cls_id=None, candidates=None, levels=3, radius=8, refine=1, keep=224,
                              ball_max_age=30):
        """append_memory_search with the candidates searched coarse to fine (DESIGN.md §11 "Scene memory: pyramid registration"):
        candidates as there, at most 15 rows. Every row is scored on `levels` (1 .. 3) max-pooled levels of both maps: `radius`
        (0 .. 8) either way at the coarsest, `refine` (0 .. 8) around twice the shift found above at each finer one; at full size
        "row 0, no shift" joins. read_motion tells which won (its table is read_pyramid's), read_pyramid the levels' tables."""
        depth = np.ascontiguousarray(depth, np.uint16)
        assert depth.shape == (self.H, self.W)
        g, c = ([SCENE_IDENTITY_Q16], [SCENE_IDENTITY_Q16]) if candidates is None else candidates
        g, c = np.ascontiguousarray(np.array(g, np.int32)), np.ascontiguousarray(np.array(c, np.int32))   # (a value outside int32 raises here)
        assert g.ndim == 2 and g.shape[1] == 6 and c.shape == g.shape
        if frame_dev_ptr is not None:
            f, on_device = C.c_void_p(frame_dev_ptr), 1
        else:
            keepalive = SceneBatch.pack(cls_id) if cls_id is not None else np.ascontiguousarray(frame_u32, np.uint32)
            assert keepalive.size == self.W * self.H
            f, on_device = _p(keepalive), 0
        self._chk(self.L.yh_scene_append_memory_pyramid(self.h, _p(depth), f, on_device, len(g), _p(g), _p(c), levels, radius, refine, keep, ball_max_age))
        self._pyramid = (len(g), levels, radius, refine)
        self._search = (len(g) + 1, refine)   # (read_motion(scores=True) is refused after this append: it names read_pyramid)

    def read_pyramid(self, level):
        """Level `level` (0 .. levels) of the last append_memory_pyramid: centres i32 [hyp][2], the centre each hypothesis was scored
        around; scores u64 [hyp][2 p + 1][2 p + 1] indexed [hyp][V - centre_y + p][U - centre_x + p], p = radius at the top level,
        refine below, hyp = n_rot (n_rot + 1 at level 0: the last is "row 0, no shift"); sum_n of the level's stamps."""
        n_rot, levels, radius, refine = getattr(self, "_pyramid", None) or (1, 0, 0, 0)
        ok = 0 <= level <= levels                # (otherwise the library refuses before it writes anything)
        p, hyp = (radius if level == levels else refine), n_rot + (1 if level == 0 else 0)
        out = dict(centres=np.zeros((hyp, 2), np.int32), scores=np.zeros((hyp, 2 * p + 1, 2 * p + 1), np.uint64))
        sum_n = C.c_uint64()
        self._chk(self.L.yh_scene_pyramid_read(self.h, level, _p(out["centres"]) if ok else None, _p(out["scores"]) if ok else None, C.byref(sum_n)))
        out["sum_n"] = sum_n.value
        return out

    def op_pyramid(self, n, m, gathers, levels, radius, refine):
        """Test hook (yh_scene_op_pyramid): the pyramid registration alone on stamps n and memory m, u32 [h][w]; gathers [n_rot][6].
        Returns dict(chosen (k, u, v), score u64 [3], pyr_n and pyr_m: lists of the pooled levels 1 .. levels, and centres, scores,
        lists over levels 0 .. levels laid out as read_pyramid's); commits nothing."""
        n, m = np.ascontiguousarray(n, np.uint32), np.ascontiguousarray(m, np.uint32)
        assert n.shape == (self.H, self.W) and m.shape == (self.H, self.W)
        g = np.ascontiguousarray(np.array(gathers, np.int32))
        assert g.ndim == 2 and g.shape[1] == 6
        ok = 1 <= len(g) <= 15 and 1 <= levels <= 3 and 0 <= radius <= 8 and 0 <= refine <= 8   # (otherwise the library refuses before it writes anything)
        dims, hs, ps = [], [], []
        for lv in range((levels if ok else 0) + 1):
            dims.append((-(-self.H >> lv), -(-self.W >> lv)))
            hs.append(len(g) + (1 if lv == 0 else 0)); ps.append(2 * (radius if lv == levels else refine) + 1)
        words = sum(h * w for h, w in dims[1:])
        pyr_n, pyr_m = np.zeros(max(words, 1), np.uint32), np.zeros(max(words, 1), np.uint32)
        centres, scores = np.zeros((sum(hs), 2), np.int32), np.zeros(sum(h * p * p for h, p in zip(hs, ps)), np.uint64)
        chosen, score = np.zeros(3, np.int32), np.zeros(3, np.uint64)
        self._chk(self.L.yh_scene_op_pyramid(self.h, _p(n), _p(m), len(g), _p(g), levels, radius, refine, _p(chosen), _p(score), _p(pyr_n), _p(pyr_m),
                                             _p(centres), _p(scores)))
        out = dict(chosen=tuple(int(v) for v in chosen), score=score, pyr_n=[], pyr_m=[], centres=[], scores=[])
        o = 0
        for h, w in dims[1:]:
            out["pyr_n"].append(pyr_n[o:o + h * w].reshape(h, w)); out["pyr_m"].append(pyr_m[o:o + h * w].reshape(h, w))
            o += h * w
        oc = os_ = 0
        for h, p in zip(hs, ps):
            out["centres"].append(centres[oc:oc + h]); out["scores"].append(scores[os_:os_ + h * p * p].reshape(h, p, p))
            oc += h; os_ += h * p * p
        return out

    def memory_pyramid_time(self, reps=20):
        """(ms per frame, ms of the registration alone) of the last append_memory_pyramid, replayed; commits nothing."""
        ms, ms_search = C.c_float(), C.c_float()
        self._chk(self.L.yh_scene_memory_pyramid_time(self.h, reps, C.byref(ms), C.byref(ms_search)))
        return ms.value, ms_search.value

    def append_memory_pyramid_norm(self, depth, frame_u32=None, frame_dev_ptr=None, cls_id=None, candidates=None, levels=3, radius=8, refine=1, min_inside=None,
                                   keep=224, ball_max_age=30):
        """append_memory_pyramid with every level, and the choice, decided by the normalised score S / (T - S) of
        append_memory_search_norm (DESIGN.md §11 "Scene memory: normalised pyramid registration"): the pyramid's reach on dense maps.
        candidates, levels, radius and refine as append_memory_pyramid; min_inside as append_memory_search_norm (None: W H // 4), carried
        to level l as (min_inside + 4^l - 1) >> 2 l. read_motion and read_pyramid work as after append_memory_pyramid, read_motion_norm
        returns chosen_stc, prior_stc and qualified, read_pyramid_norm the levels' three tables and flags."""
        depth = np.ascontiguousarray(depth, np.uint16)
        assert depth.shape == (self.H, self.W)
        g, c = ([SCENE_IDENTITY_Q16], [SCENE_IDENTITY_Q16]) if candidates is None else candidates
        g, c = np.ascontiguousarray(np.array(g, np.int32)), np.ascontiguousarray(np.array(c, np.int32))   # (a value outside int32 raises here)
        assert g.ndim == 2 and g.shape[1] == 6 and c.shape == g.shape
        if min_inside is None:
            min_inside = (self.W * self.H) // 4
        if frame_dev_ptr is not None:
            f, on_device = C.c_void_p(frame_dev_ptr), 1
        else:
            keepalive = SceneBatch.pack(cls_id) if cls_id is not None else np.ascontiguousarray(frame_u32, np.uint32)
            assert keepalive.size == self.W * self.H
            f, on_device = _p(keepalive), 0
        self._chk(self.L.yh_scene_append_memory_pyramid_norm(self.h, _p(depth), f, on_device, len(g), _p(g), _p(c), levels, radius, refine, min_inside, keep,
                                                             ball_max_age))
        self._pyramid = (len(g), levels, radius, refine)
        self._search = (len(g) + 1, refine)   # (read_motion(scores=True) is refused after this append: it names read_pyramid)
        self._norm_levels = True              # (read_motion_norm asks for no tables: they are read_pyramid_norm's)

    def read_pyramid_norm(self, level):
        """Level `level` (0 .. levels) of the last append_memory_pyramid_norm: centres, scores (S) and sum_n as read_pyramid returns
        them, totals (T) and inside (C) laid out as scores, min_inside: the level's threshold, qualified i32 [hyp]: whether any entry
        of the hypothesis qualified."""
        n_rot, levels, radius, refine = getattr(self, "_pyramid", None) or (1, 0, 0, 0)
        ok = 0 <= level <= levels                # (otherwise the library refuses before it writes anything)
        p, hyp = (radius if level == levels else refine), n_rot + (1 if level == 0 else 0)
        shape = (hyp, 2 * p + 1, 2 * p + 1)
        out = dict(centres=np.zeros((hyp, 2), np.int32), scores=np.zeros(shape, np.uint64), totals=np.zeros(shape, np.uint64), inside=np.zeros(shape, np.uint64),
                   qualified=np.zeros(hyp, np.int32))
        sum_n, need = C.c_uint64(), C.c_int32()
        a = [_p(out[k]) if ok else None for k in ("centres", "scores", "totals", "inside")]
        self._chk(self.L.yh_scene_pyramid_norm_read(self.h, level, a[0], a[1], a[2], a[3], C.byref(sum_n), C.byref(need), _p(out["qualified"]) if ok else None))
        out.update(sum_n=sum_n.value, min_inside=need.value)
        return out

    def op_pyramid_norm(self, n, m, gathers, levels, radius, refine, min_inside):
        """Test hook (yh_scene_op_pyramid_norm): the normalised pyramid registration alone on stamps n and memory m, u32 [h][w];
        gathers [n_rot][6]. Returns op_pyramid's dict (scores: the S tables) with totals, inside (lists over levels, laid out as
        scores), flags (list over levels of i32 [hyp]: whether any entry of the hypothesis qualified), chosen_stc u64 [3] = (S, T, C)
        of the choice and qualified; commits nothing."""
        n, m = np.ascontiguousarray(n, np.uint32), np.ascontiguousarray(m, np.uint32)
        assert n.shape == (self.H, self.W) and m.shape == (self.H, self.W)
        g = np.ascontiguousarray(np.array(gathers, np.int32))
        assert g.ndim == 2 and g.shape[1] == 6
        ok = 1 <= len(g) <= 15 and 1 <= levels <= 3 and 0 <= radius <= 8 and 0 <= refine <= 8   # (otherwise the library refuses before it writes anything)
        dims, hs, ps = [], [], []
        for lv in range((levels if ok else 0) + 1):
            dims.append((-(-self.H >> lv), -(-self.W >> lv)))
            hs.append(len(g) + (1 if lv == 0 else 0)); ps.append(2 * (radius if lv == levels else refine) + 1)
        words = sum(h * w for h, w in dims[1:])
        pyr_n, pyr_m = np.zeros(max(words, 1), np.uint32), np.zeros(max(words, 1), np.uint32)
        nt = sum(h * p * p for h, p in zip(hs, ps))
        centres, scores, totals, inside = np.zeros((sum(hs), 2), np.int32), np.zeros(nt, np.uint64), np.zeros(nt, np.uint64), np.zeros(nt, np.uint64)
        chosen, score, flags, stc = np.zeros(3, np.int32), np.zeros(3, np.uint64), np.zeros(sum(hs) + 1, np.int32), np.zeros(3, np.uint64)
        self._chk(self.L.yh_scene_op_pyramid_norm(self.h, _p(n), _p(m), len(g), _p(g), levels, radius, refine, _p(chosen), _p(score), _p(pyr_n), _p(pyr_m),
                                                  _p(centres), _p(scores), min_inside, _p(totals), _p(inside), _p(flags), _p(stc)))
        out = dict(chosen=tuple(int(v) for v in chosen), score=score, pyr_n=[], pyr_m=[], centres=[], scores=[], totals=[], inside=[], flags=[],
                   chosen_stc=stc, qualified=bool(flags[-1]))
        o = 0
        for h, w in dims[1:]:
            out["pyr_n"].append(pyr_n[o:o + h * w].reshape(h, w)); out["pyr_m"].append(pyr_m[o:o + h * w].reshape(h, w))
            o += h * w
        oc = os_ = 0
        for h, p in zip(hs, ps):
            out["centres"].append(centres[oc:oc + h]); out["flags"].append(flags[oc:oc + h])
            for key, tab in (("scores", scores), ("totals", totals), ("inside", inside)):
                out[key].append(tab[os_:os_ + h * p * p].reshape(h, p, p))
            oc += h; os_ += h * p * p
        return out

    def memory_pyramid_norm_time(self, reps=20):
        """(ms per frame, ms of the registration alone) of the last append_memory_pyramid_norm, replayed; commits nothing."""
        ms, ms_search = C.c_float(), C.c_float()
        self._chk(self.L.yh_scene_memory_pyramid_norm_time(self.h, reps, C.byref(ms), C.byref(ms_search)))
        return ms.value, ms_search.value

    def plan(self, targets=None, n_targets=3, start=None, connectivity=4):
        """modify_path (src/path.rs:25-120) on the last appended frame. targets: (x, y) pixels, or None: the first n_targets balls
        (balls[..3], path.rs:37). start: the robot's pixel (x, y); None: the reference's START_NODE, (400, 479), at 640x480 only.
        connectivity: 4, or 8 to use the scene's diagonal lengths too (DESIGN.md §11 "Diagonals")."""
        if start is None:
            if (self.W, self.H) != (640, 480):
                raise ValueError("start=None is the reference's START_NODE at 640x480; give the start for other sizes")
            start = (400, 479)
        if targets is None:
            self._chk(self.L.yh_scene_plan_conn(self.h, None, n_targets, start[0], start[1], connectivity))
        else:
            t = np.ascontiguousarray(targets, np.int32).reshape(-1, 2)
            self._chk(self.L.yh_scene_plan_conn(self.h, _p(t), len(t), start[0], start[1], connectivity))

    def read_plan(self, fields=True):
        """The last plan: path int32 [L][2] (x, y) from the start to a target, directions f32 [L - 1][2] (magnitude, rotation), and
        with fields=True cost f32 [H][W] and next int32 [H][W] (linear index of the successor, -1 at targets)."""
        n = C.c_int32()
        self._chk(self.L.yh_scene_plan_read(self.h, None, None, None, None, 0, C.byref(n)))
        out = dict(path=np.zeros((n.value, 2), np.int32))
        dirs = np.zeros((n.value, 2), np.float32)
        if fields:
            out["cost"] = np.zeros((self.H, self.W), np.float32)
            out["next"] = np.zeros((self.H, self.W), np.int32)
        self._chk(self.L.yh_scene_plan_read(self.h, _p(out["cost"]) if fields else None, _p(out["next"]) if fields else None,
                                            _p(out["path"]), _p(dirs), n.value, C.byref(n)))
        out["directions"] = dirs[:max(n.value - 1, 0)]
        return out

    def set_fields(self, map, conn0, conn1):
        """Test hook: host fields as if a SANE frame had produced them (layouts of read())."""
        m = np.ascontiguousarray(map, np.uint32)
        c0, c1 = np.ascontiguousarray(conn0, np.float32), np.ascontiguousarray(conn1, np.float32)
        assert m.shape == (self.H, self.W) and c0.shape == (self.H, self.W, 4) and c1.shape == (self.H, self.W, 4)
        self._chk(self.L.yh_scene_set_fields(self.h, _p(m), _p(c0), _p(c1)))

    def plan_time(self, reps=20):
        """Replays the last plan: dict(ms_per_plan, rounds, tile_runs)."""
        ms, r, t = C.c_float(), C.c_int32(), C.c_int32()
        self._chk(self.L.yh_scene_plan_time(self.h, reps, C.byref(ms), C.byref(r), C.byref(t)))
        return dict(ms_per_plan=ms.value, rounds=r.value, tile_runs=t.value)

    def plan_tour(self, targets=None, n_targets=3, start=None, connectivity=4):
        """The tour (DESIGN.md §11 "Tour"): one cost field per target solved in the same launches, the visiting order of least
        total cost and the joined route. targets, n_targets (at most TOUR_MAX, distinct), start and connectivity as plan()."""
        if start is None:
            if (self.W, self.H) != (640, 480):
                raise ValueError("start=None is the reference's START_NODE at 640x480; give the start for other sizes")
            start = (400, 479)
        if targets is None:
            self._chk(self.L.yh_scene_plan_tour_conn(self.h, None, n_targets, start[0], start[1], connectivity))
        else:
            t = np.ascontiguousarray(targets, np.int32).reshape(-1, 2)
            self._chk(self.L.yh_scene_plan_tour_conn(self.h, _p(t), len(t), start[0], start[1], connectivity))

    def read_tour(self, fields=False):
        """The last tour: targets int32 [K][2], order int32 [K] (indices into targets), legs f32 [K + 1][K] (row 0 from the start,
        row 1 + a from target a; column b = to target b), total f32, path int32 [L][2], directions f32 [L - 1][2], leg_ends int32 [K]
        (index in path where each leg ends); with fields=True also cost f32 [K][H][W], next int32 [K][H][W], label uint8 [H][W]."""
        k, n, total = C.c_int32(), C.c_int32(), C.c_float()
        self._chk(self.L.yh_scene_tour_read(self.h, C.byref(k), None, None, None, None, None, None, None, None, None, None, 0, C.byref(n)))
        K = k.value
        out = dict(targets=np.zeros((K, 2), np.int32), order=np.zeros(K, np.int32), legs=np.zeros((K + 1, K), np.float32),
                   path=np.zeros((n.value, 2), np.int32), leg_ends=np.zeros(K, np.int32))
        dirs = np.zeros((n.value, 2), np.float32)
        if fields:
            out["cost"] = np.zeros((K, self.H, self.W), np.float32)
            out["next"] = np.zeros((K, self.H, self.W), np.int32)
            out["label"] = np.zeros((self.H, self.W), np.uint8)
        f = lambda name: _p(out[name]) if fields else None
        self._chk(self.L.yh_scene_tour_read(self.h, C.byref(k), _p(out["targets"]), _p(out["order"]), _p(out["legs"]), C.byref(total),
                                            f("cost"), f("next"), f("label"), _p(out["path"]), _p(dirs), _p(out["leg_ends"]), n.value, C.byref(n)))
        out["total"] = np.float32(total.value)
        out["directions"] = dirs[:max(n.value - 1, 0)]
        return out

    def tour_time(self, reps=20):
        """Replays the last tour: dict(ms_per_tour, rounds, tile_runs)."""
        ms, r, t = C.c_float(), C.c_int32(), C.c_int32()
        self._chk(self.L.yh_scene_tour_time(self.h, reps, C.byref(ms), C.byref(r), C.byref(t)))
        return dict(ms_per_tour=ms.value, rounds=r.value, tile_runs=t.value)


    def plan_turn(self, targets=None, n_targets=3, start=None, heading=6, turn_price=2.0):
        """The turn-aware plan (DESIGN.md §11 "Turns"): the 8-connected planner over states (pixel, heading) with turn_price per
        45 degrees turned in place. targets, n_targets, start as plan(); heading: the start heading 0 .. 7 (0 right, clockwise on
        the image; 6, the default, is up: the camera looks up the bird's-eye map from START_NODE)."""
        if start is None:
            if (self.W, self.H) != (640, 480):
                raise ValueError("start=None is the reference's START_NODE at 640x480; give the start for other sizes")
            start = (400, 479)
        if targets is None:
            self._chk(self.L.yh_scene_plan_turn(self.h, None, n_targets, start[0], start[1], heading, turn_price))
        else:
            t = np.ascontiguousarray(targets, np.int32).reshape(-1, 2)
            self._chk(self.L.yh_scene_plan_turn(self.h, _p(t), len(t), start[0], start[1], heading, turn_price))

    def read_turn(self, fields=True):
        """The last turn plan: path int32 [L][2], directions f32 [L - 1][2] (magnitude, rotation), turns int32 [L - 1] (signed
        45-degree steps made before each drive), and with fields=True cost f32 [8][H][W] and act uint8 [8][H][W] (0 drive, 1 turn
        to h - 1, 2 turn to h + 1, 255 at targets)."""
        n = C.c_int32()
        self._chk(self.L.yh_scene_turn_read(self.h, None, None, None, None, None, 0, C.byref(n)))
        out = dict(path=np.zeros((n.value, 2), np.int32))
        dirs, turns = np.zeros((n.value, 2), np.float32), np.zeros(n.value, np.int32)
        if fields:
            out["cost"] = np.zeros((8, self.H, self.W), np.float32)
            out["act"] = np.zeros((8, self.H, self.W), np.uint8)
        self._chk(self.L.yh_scene_turn_read(self.h, _p(out["cost"]) if fields else None, _p(out["act"]) if fields else None,
                                            _p(out["path"]), _p(dirs), _p(turns), n.value, C.byref(n)))
        out["directions"] = dirs[:max(n.value - 1, 0)]
        out["turns"] = turns[:max(n.value - 1, 0)]
        return out

    def turn_time(self, reps=20):
        """Replays the last turn plan: dict(ms_per_plan, rounds, tile_runs)."""
        ms, r, t = C.c_float(), C.c_int32(), C.c_int32()
        self._chk(self.L.yh_scene_turn_time(self.h, reps, C.byref(ms), C.byref(r), C.byref(t)))
        return dict(ms_per_plan=ms.value, rounds=r.value, tile_runs=t.value)

    def plan_turn_tour(self, targets=None, n_targets=3, start=None, heading=6, turn_price=2.0):
        """The turn-aware tour (DESIGN.md §11 "Turn tour"): one turn-plan field per target solved in the same launches, the visiting
        order of least total cost with every leg starting in the heading the leg before arrived with, and the joined route.
        targets, n_targets (at most TOUR_MAX, distinct) and start as plan_tour(); heading and turn_price as plan_turn()."""
        if start is None:
            if (self.W, self.H) != (640, 480):
                raise ValueError("start=None is the reference's START_NODE at 640x480; give the start for other sizes")
            start = (400, 479)
        if targets is None:
            self._chk(self.L.yh_scene_plan_turn_tour(self.h, None, n_targets, start[0], start[1], heading, turn_price))
        else:
            t = np.ascontiguousarray(targets, np.int32).reshape(-1, 2)
            self._chk(self.L.yh_scene_plan_turn_tour(self.h, _p(t), len(t), start[0], start[1], heading, turn_price))

    def read_turn_tour(self, fields=True):
        """The last turn tour: targets int32 [K][2], order int32 [K], legs f32 [1 + 8K][K] and arrive uint8 [1 + 8K][K] (row 0 the
        start state, row 1 + 8a + h the state (target a, heading h); column b = to target b: the cost, the heading on arrival),
        total f32, leg_headings int32 [K], path int32 [L][2], directions f32 [L - 1][2], turns int32 [L - 1], leg_ends int32 [K];
        with fields=True also cost f32 [K][8][H][W], act uint8 [K][8][H][W], label uint8 [8][H][W]."""
        k, n, total = C.c_int32(), C.c_int32(), C.c_float()
        self._chk(self.L.yh_scene_turn_tour_read(self.h, C.byref(k), None, None, None, None, None, None, None, None, None, None, None, None, None, 0, C.byref(n)))
        K = k.value
        out = dict(targets=np.zeros((K, 2), np.int32), order=np.zeros(K, np.int32), legs=np.zeros((1 + 8 * K, K), np.float32),
                   arrive=np.zeros((1 + 8 * K, K), np.uint8), leg_headings=np.zeros(K, np.int32), path=np.zeros((n.value, 2), np.int32),
                   leg_ends=np.zeros(K, np.int32))
        dirs, turns = np.zeros((n.value, 2), np.float32), np.zeros(n.value, np.int32)
        if fields:
            out["cost"] = np.zeros((K, 8, self.H, self.W), np.float32)
            out["act"] = np.zeros((K, 8, self.H, self.W), np.uint8)
            out["label"] = np.zeros((8, self.H, self.W), np.uint8)
        f = lambda name: _p(out[name]) if fields else None
        self._chk(self.L.yh_scene_turn_tour_read(self.h, C.byref(k), _p(out["targets"]), _p(out["order"]), _p(out["legs"]), _p(out["arrive"]), C.byref(total),
                                                 _p(out["leg_headings"]), f("cost"), f("act"), f("label"), _p(out["path"]), _p(dirs), _p(turns),
                                                 _p(out["leg_ends"]), n.value, C.byref(n)))
        out["total"] = np.float32(total.value)
        out["directions"] = dirs[:max(n.value - 1, 0)]
        out["turns"] = turns[:max(n.value - 1, 0)]
        return out

    def turn_tour_time(self, reps=20):
        """Replays the last turn tour: dict(ms_per_tour, rounds, tile_runs)."""
        ms, r, t = C.c_float(), C.c_int32(), C.c_int32()
        self._chk(self.L.yh_scene_turn_tour_time(self.h, reps, C.byref(ms), C.byref(r), C.byref(t)))
        return dict(ms_per_tour=ms.value, rounds=r.value, tile_runs=t.value)


class SceneBatch:
    """RAII wrapper of yh_scene_batch: N frames appended and planned in one set of launches; frame b equals a Scene fed that frame alone."""

    def __init__(self, width=640, height=480, max_frames=8, device=0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.yh_scene_batch_create(device, width, height, max_frames, C.byref(h))
        if rc != OK:
            raise YhError(rc, self.L.yh_scene_batch_last_error(None).decode())
        self.h, self.W, self.H, self.max_frames, self.n = h, width, height, max_frames, 0

    def close(self):
        if getattr(self, "h", None):
            self.L.yh_scene_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            raise YhError(rc, self.L.yh_scene_batch_last_error(self.h).decode())

    @staticmethod
    def pack(cls_id):
        """A (class, id) byte image [h][w][2] as the packed u32 frame both compat modes read the same: class << 24 | id << 16 | id << 8 | class."""
        ci = np.ascontiguousarray(cls_id, np.uint8).astype(np.uint32)
        return np.ascontiguousarray(ci[..., 0] << 24 | ci[..., 1] << 16 | ci[..., 1] << 8 | ci[..., 0])

    def stage(self, slot, depth, frame_u32=None, frame_dev_ptr=None, cls_id=None):
        """One frame into slot `slot`: depth u16 [h][w] and one of frame_u32 (host, packed), frame_dev_ptr (device, packed) or cls_id
        ((class, id) bytes [h][w][2], packed here). The sources are free again on return."""
        depth = np.ascontiguousarray(depth, np.uint16)
        assert depth.shape == (self.H, self.W)
        if frame_dev_ptr is not None:
            self._chk(self.L.yh_scene_batch_stage(self.h, slot, _p(depth), C.c_void_p(frame_dev_ptr), 1))
            return
        f = self.pack(cls_id) if cls_id is not None else np.ascontiguousarray(frame_u32, np.uint32)
        assert f.size == self.W * self.H
        self._chk(self.L.yh_scene_batch_stage(self.h, slot, _p(depth), _p(f), 0))

    def stage_frames(self, first_slot, depths, frames_u32=None, frames_dev_ptr=None):
        """n frames into slots first_slot .. first_slot + n - 1 in one call: depths u16 [n][h][w] and one of frames_u32 (host, packed
        [n][h][w]) or frames_dev_ptr (device, packed [n][h][w]: Engine.instance_batch_device_frames). The sources are free again on return."""
        depths = np.ascontiguousarray(depths, np.uint16)
        if depths.ndim != 3 or depths.shape[1:] != (self.H, self.W):
            raise ValueError(f"depths: need [n][{self.H}][{self.W}], got {depths.shape}")
        n = depths.shape[0]
        if (frames_u32 is None) == (frames_dev_ptr is None):
            raise ValueError("give exactly one of frames_u32 and frames_dev_ptr")
        if frames_dev_ptr is not None:
            if not frames_dev_ptr:
                raise ValueError("frames_dev_ptr is null")
            self._chk(self.L.yh_scene_batch_stage_frames(self.h, first_slot, n, _p(depths), C.c_void_p(frames_dev_ptr), 1))
            return
        f = np.ascontiguousarray(frames_u32, np.uint32)
        if f.size != n * self.W * self.H:
            raise ValueError(f"frames_u32: need {n} frames of {self.H} x {self.W}, got {f.shape}")
        self._chk(self.L.yh_scene_batch_stage_frames(self.h, first_slot, n, _p(depths), _p(f), 0))

    def append(self, n, mode=COMPAT_STRICT):
        self._chk(self.L.yh_scene_batch_append(self.h, n, mode))
        self.n, self._fields = n, False

    def read(self, b, which=None):
        """Frame b's outputs; `which` as in Scene.read (yh_scene_batch_read takes nulls as well)."""
        out = _scene_outputs(self.W, self.H, which)
        self._chk(self.L.yh_scene_batch_read(self.h, b, *(_p(out[k]) if k in out else None for k in _SCENE_OUTPUTS)))
        return out

    def plan(self, targets=None, n_targets=3, starts=None, connectivity=4):
        """Plans every frame of the last append (Scene.plan per frame, in shared launches). targets: [n][k] (x, y) pixels, or None:
        each frame's first n_targets balls. starts: [n] (x, y); None: the reference's START_NODE per frame, at 640x480 only.
        Returns the status list: OK, or ESTATE for a frame without a usable ball (it has no plan)."""
        n = self.n
        if starts is None:
            if (self.W, self.H) != (640, 480):
                raise ValueError("starts=None is the reference's START_NODE at 640x480; give the starts for other sizes")
            starts = [(400, 479)] * n
        s = np.ascontiguousarray(starts, np.int32).reshape(-1, 2)
        assert len(s) == n
        status = np.zeros(max(n, 1), np.int32)
        if targets is None:
            self._chk(self.L.yh_scene_batch_plan(self.h, None, n_targets, _p(s), connectivity, _p(status)))
        else:
            t = np.ascontiguousarray(targets, np.int32)
            assert t.ndim == 3 and t.shape[0] == n and t.shape[2] == 2
            self._chk(self.L.yh_scene_batch_plan(self.h, _p(t), t.shape[1], _p(s), connectivity, _p(status)))
        return [int(v) for v in status[:n]]

    def read_plan(self, b, fields=True):
        """Frame b of the last plan, as Scene.read_plan."""
        n = C.c_int32()
        self._chk(self.L.yh_scene_batch_plan_read(self.h, b, None, None, None, None, 0, C.byref(n)))
        out = dict(path=np.zeros((n.value, 2), np.int32))
        dirs = np.zeros((n.value, 2), np.float32)
        if fields:
            out["cost"] = np.zeros((self.H, self.W), np.float32)
            out["next"] = np.zeros((self.H, self.W), np.int32)
        self._chk(self.L.yh_scene_batch_plan_read(self.h, b, _p(out["cost"]) if fields else None, _p(out["next"]) if fields else None,
                                                  _p(out["path"]), _p(dirs), n.value, C.byref(n)))
        out["directions"] = dirs[:max(n.value - 1, 0)]
        return out

    def append_memory(self, n, motions=None, streams=None, keep=224, ball_max_age=30):
        """Slots 0 .. n - 1 as staged, fused into the memories of their camera streams (DESIGN.md §11 "Scene batch: memory"): frame b is
        Scene.append_memory on the memory of streams[b] (0 .. SCENE_STREAMS_MAX - 1; None: all on stream 0), the calls made in batch
        order. motions: n (gather_q16, carry_q16) pairs as scene_motion returns them; None: the identity for every frame. keep and
        ball_max_age are one value per call."""
        if motions is None:
            motions = [(SCENE_IDENTITY_Q16, SCENE_IDENTITY_Q16)] * max(n, 0)
        g = np.array([m[0] for m in motions], np.int32).reshape(-1, 6)   # (a value outside int32 raises here)
        c = np.array([m[1] for m in motions], np.int32).reshape(-1, 6)
        assert len(g) == len(c) == max(n, 0), "motions: one (gather, carry) pair per frame"
        st = Engine._streams(streams, n)
        self._chk(self.L.yh_scene_batch_append_memory(self.h, n, _p(st) if st is not None else None, _p(g), _p(c), keep, ball_max_age))
        self.n, self._fields = n, False

    def append_memory_search(self, n, candidates=None, streams=None, radius=4, keep=224, ball_max_age=30):
        """append_memory with every frame's motion found on the device (DESIGN.md §11 "Scene batch: registration"): frame b is
        Scene.append_memory_search on the memory of streams[b], the calls made in batch order, so a stream's later frame is scored
        against what its earlier frame has just fused. candidates: n (gathers, carries) pairs, the same number of rows of six ints
        each, row 0 the frame's prior (scene_motion_candidates); None: the identity alone for every frame. radius, keep and
        ball_max_age are one value per call; read_motion(b) tells what frame b chose."""
        if candidates is None:
            candidates = [([SCENE_IDENTITY_Q16], [SCENE_IDENTITY_Q16])] * max(n, 0)
        g = np.ascontiguousarray(np.array([m[0] for m in candidates], np.int32))   # (a value outside int32 raises here)
        c = np.ascontiguousarray(np.array([m[1] for m in candidates], np.int32))
        assert len(candidates) == max(n, 0), "candidates: one (gathers, carries) pair per frame"
        assert n <= 0 or (g.ndim == 3 and g.shape[2] == 6 and c.shape == g.shape), "candidates: the same number of rows of six ints for every frame"
        n_rot = g.shape[1] if g.ndim == 3 else 0
        st = Engine._streams(streams, n)
        self._chk(self.L.yh_scene_batch_append_memory_search(self.h, n, _p(st) if st is not None else None, n_rot, _p(g), _p(c), radius, keep, ball_max_age))
        self.n, self._fields, self._search = n, False, (n_rot, radius)

    def append_memory_pyramid(self, n, candidates=None, streams=None, levels=3, radius=8, refine=1, keep=224, ball_max_age=30):
        """append_memory_search with every frame's candidates searched coarse to fine (DESIGN.md §11 "Scene batch: pyramid
        registration"): frame b is Scene.append_memory_pyramid on the memory of streams[b], the calls made in batch order, so a
        stream's later frame is registered against what its earlier frame has just fused. candidates as append_memory_search takes
        them, at most 15 rows a frame; None: the identity alone. levels, radius, refine, keep and ball_max_age are one value per call;
        read_motion(b) tells what frame b chose, read_pyramid(b, level) its levels' tables."""
        if candidates is None:
            candidates = [([SCENE_IDENTITY_Q16], [SCENE_IDENTITY_Q16])] * max(n, 0)
        g = np.ascontiguousarray(np.array([m[0] for m in candidates], np.int32))   # (a value outside int32 raises here)
        c = np.ascontiguousarray(np.array([m[1] for m in candidates], np.int32))
        assert len(candidates) == max(n, 0), "candidates: one (gathers, carries) pair per frame"
        assert n <= 0 or (g.ndim == 3 and g.shape[2] == 6 and c.shape == g.shape), "candidates: the same number of rows of six ints for every frame"
        n_rot = g.shape[1] if g.ndim == 3 else 0
        st = Engine._streams(streams, n)
        self._chk(self.L.yh_scene_batch_append_memory_pyramid(self.h, n, _p(st) if st is not None else None, n_rot, _p(g), _p(c), levels, radius, refine, keep,
                                                              ball_max_age))
        self.n, self._fields, self._pyramid = n, False, (n_rot, levels, radius, refine)
        self._search = (n_rot + 1, refine)   # (read_motion(scores=True) is refused after this append: it names read_pyramid)

    def read_pyramid(self, frame, level):
        """Level `level` (0 .. levels) of what the last append_memory_pyramid did for frame `frame`: the dict Scene.read_pyramid
        returns (centres, scores, sum_n)."""
        n_rot, levels, radius, refine = getattr(self, "_pyramid", None) or (1, 0, 0, 0)
        ok = 0 <= level <= levels                # (otherwise the library refuses before it writes anything)
        p, hyp = (radius if level == levels else refine), n_rot + (1 if level == 0 else 0)
        out = dict(centres=np.zeros((hyp, 2), np.int32), scores=np.zeros((hyp, 2 * p + 1, 2 * p + 1), np.uint64))
        sum_n = C.c_uint64()
        self._chk(self.L.yh_scene_batch_pyramid_read(self.h, frame, level, _p(out["centres"]) if ok else None, _p(out["scores"]) if ok else None, C.byref(sum_n)))
        out["sum_n"] = sum_n.value
        return out

    def memory_pyramid_time(self, reps=20):
        """(ms per batch, ms of the registration launches alone) of the last append_memory_pyramid, replayed; commits nothing."""
        ms, ms_search = C.c_float(), C.c_float()
        self._chk(self.L.yh_scene_batch_memory_pyramid_time(self.h, reps, C.byref(ms), C.byref(ms_search)))
        return ms.value, ms_search.value

    def read_motion(self, frame, scores=False):
        """What the last append_memory_search or append_memory_pyramid chose for frame `frame`: the dict Scene.read_motion returns
        (after a pyramid append scores=True is refused: read_pyramid has the tables)."""
        out = dict(gather=np.zeros(6, np.int32), carry=np.zeros(6, np.int32), chosen=np.zeros(3, np.int32), score=np.zeros(3, np.uint64))
        table = None
        if scores and getattr(self, "_search", None):
            n_rot, radius = self._search
            table = np.zeros((n_rot, 2 * radius + 1, 2 * radius + 1), np.uint64)
        self._chk(self.L.yh_scene_batch_motion_read(self.h, frame, _p(out["gather"]), _p(out["carry"]), _p(out["chosen"]), _p(out["score"]),
                                                    _p(table) if table is not None else None))
        if scores:
            out["scores"] = table
        return out

    def memory_search_time(self, reps=20):
        """(ms per batch, ms of the registration launches alone) of the last append_memory_search, replayed; commits nothing."""
        ms, ms_search = C.c_float(), C.c_float()
        self._chk(self.L.yh_scene_batch_memory_search_time(self.h, reps, C.byref(ms), C.byref(ms_search)))
        return ms.value, ms_search.value

    def _candidates(self, n, candidates):
        """(gathers, carries, n_rot) of n (gathers, carries) pairs as the batched searching appends take them; None: the identity alone."""
        if candidates is None:
            candidates = [([SCENE_IDENTITY_Q16], [SCENE_IDENTITY_Q16])] * max(n, 0)
        g = np.ascontiguousarray(np.array([m[0] for m in candidates], np.int32))   # (a value outside int32 raises here)
        c = np.ascontiguousarray(np.array([m[1] for m in candidates], np.int32))
        assert len(candidates) == max(n, 0), "candidates: one (gathers, carries) pair per frame"
        assert n <= 0 or (g.ndim == 3 and g.shape[2] == 6 and c.shape == g.shape), "candidates: the same number of rows of six ints for every frame"
        return g, c, (g.shape[1] if g.ndim == 3 else 0)

    def append_memory_search_norm(self, n, candidates=None, streams=None, radius=4, min_inside=None, keep=224, ball_max_age=30):
        """append_memory_search with every frame's choice made by the normalised score (DESIGN.md §11 "Scene batch: normalised
        registration"), for dense maps: frame b is Scene.append_memory_search_norm on the memory of streams[b], the calls made in
        batch order. candidates, streams and radius as append_memory_search; min_inside: how many frame pixels a candidate must keep
        inside the frame to qualify, 1 .. W H, one value per call; None: W H // 4. read_motion(b) works as after append_memory_search
        (its scores are the S table), read_motion_norm(b) returns the rest."""
        g, c, n_rot = self._candidates(n, candidates)
        if min_inside is None:
            min_inside = (self.W * self.H) // 4
        st = Engine._streams(streams, n)
        self._chk(self.L.yh_scene_batch_append_memory_search_norm(self.h, n, _p(st) if st is not None else None, n_rot, _p(g), _p(c), radius, min_inside, keep,
                                                                  ball_max_age))
        self.n, self._fields, self._search, self._norm_levels = n, False, (n_rot, radius), False

    def read_motion_norm(self, frame):
        """What the last append_memory_search_norm saw for frame `frame` beside read_motion's: the dict Scene.read_motion_norm returns
        (after append_memory_pyramid_norm: chosen_stc, prior_stc and qualified alone; read_pyramid_norm has the levels' tables)."""
        n_rot, radius = getattr(self, "_search", None) or (1, 0)
        shape = (n_rot, 2 * radius + 1, 2 * radius + 1)
        out = dict(chosen_stc=np.zeros(3, np.uint64), prior_stc=np.zeros(3, np.uint64))
        if not getattr(self, "_norm_levels", False):
            out.update(totals=np.zeros(shape, np.uint64), inside=np.zeros(shape, np.uint64))
        q = C.c_int32()
        t, i = (_p(out[k]) if k in out else None for k in ("totals", "inside"))
        self._chk(self.L.yh_scene_batch_motion_norm_read(self.h, frame, t, i, _p(out["chosen_stc"]), _p(out["prior_stc"]), C.byref(q)))
        out["qualified"] = bool(q.value)
        return out

    def memory_search_norm_time(self, reps=20):
        """(ms per batch, ms of the registration launches alone) of the last append_memory_search_norm, replayed; commits nothing."""
        ms, ms_search = C.c_float(), C.c_float()
        self._chk(self.L.yh_scene_batch_memory_search_norm_time(self.h, reps, C.byref(ms), C.byref(ms_search)))
        return ms.value, ms_search.value

    def append_memory_pyramid_norm(self, n, candidates=None, streams=None, levels=3, radius=8, refine=1, min_inside=None, keep=224, ball_max_age=30):
        """append_memory_pyramid with every level, and the choice, decided by the normalised score (DESIGN.md §11 "Scene batch:
        normalised pyramid registration"): frame b is Scene.append_memory_pyramid_norm on the memory of streams[b], the calls made
        in batch order. candidates, streams, levels, radius and refine as append_memory_pyramid; min_inside as
        append_memory_search_norm. read_motion(b) and read_pyramid(b, level) work as after append_memory_pyramid, read_motion_norm(b)
        returns chosen_stc, prior_stc and qualified, read_pyramid_norm(b, level) the levels' three tables and flags."""
        g, c, n_rot = self._candidates(n, candidates)
        if min_inside is None:
            min_inside = (self.W * self.H) // 4
        st = Engine._streams(streams, n)
        self._chk(self.L.yh_scene_batch_append_memory_pyramid_norm(self.h, n, _p(st) if st is not None else None, n_rot, _p(g), _p(c), levels, radius, refine,
                                                                   min_inside, keep, ball_max_age))
        self.n, self._fields, self._pyramid = n, False, (n_rot, levels, radius, refine)
        self._search = (n_rot + 1, refine)   # (read_motion(scores=True) is refused after this append: it names read_pyramid)
        self._norm_levels = True             # (read_motion_norm asks for no tables: they are read_pyramid_norm's)

    def read_pyramid_norm(self, frame, level):
        """Level `level` (0 .. levels) of what the last append_memory_pyramid_norm did for frame `frame`: the dict
        Scene.read_pyramid_norm returns (centres, scores, totals, inside, sum_n, min_inside, qualified)."""
        n_rot, levels, radius, refine = getattr(self, "_pyramid", None) or (1, 0, 0, 0)
        ok = 0 <= level <= levels                # (otherwise the library refuses before it writes anything)
        p, hyp = (radius if level == levels else refine), n_rot + (1 if level == 0 else 0)
        shape = (hyp, 2 * p + 1, 2 * p + 1)
        out = dict(centres=np.zeros((hyp, 2), np.int32), scores=np.zeros(shape, np.uint64), totals=np.zeros(shape, np.uint64), inside=np.zeros(shape, np.uint64),
                   qualified=np.zeros(hyp, np.int32))
        sum_n, need = C.c_uint64(), C.c_int32()
        a = [_p(out[k]) if ok else None for k in ("centres", "scores", "totals", "inside")]
        self._chk(self.L.yh_scene_batch_pyramid_norm_read(self.h, frame, level, a[0], a[1], a[2], a[3], C.byref(sum_n), C.byref(need),
                                                          _p(out["qualified"]) if ok else None))
        out.update(sum_n=sum_n.value, min_inside=need.value)
        return out

    def memory_pyramid_norm_time(self, reps=20):
        """(ms per batch, ms of the registration launches alone) of the last append_memory_pyramid_norm, replayed; commits nothing."""
        ms, ms_search = C.c_float(), C.c_float()
        self._chk(self.L.yh_scene_batch_memory_pyramid_norm_time(self.h, reps, C.byref(ms), C.byref(ms_search)))
        return ms.value, ms_search.value

    def read_memory(self, stream=0):
        """The memory of one stream: map u32 [h][w], balls i32 [100][4] = (x, y, count, age); zeros while empty."""
        out = dict(map=np.zeros((self.H, self.W), np.uint32), balls=np.zeros((100, 4), np.int32))
        self._chk(self.L.yh_scene_batch_memory_read(self.h, stream, _p(out["map"]), _p(out["balls"])))
        return out

    def read_frame_memory_balls(self, frame):
        """The ball table of frame `frame`'s stream right after that frame of the last memory append: i32 [100][4]."""
        out = np.zeros((100, 4), np.int32)
        self._chk(self.L.yh_scene_batch_memory_frame_balls(self.h, frame, _p(out)))
        return out

    def memory_reset(self, stream=-1):
        """Empties the memory of one stream; -1: of all."""
        self._chk(self.L.yh_scene_batch_memory_reset(self.h, stream))

    def memory_time(self, reps=20):
        """Replays the last memory append from the state it started from (nothing is committed): ms per batch."""
        ms = C.c_float()
        self._chk(self.L.yh_scene_batch_memory_time(self.h, reps, C.byref(ms)))
        return ms.value

    def time(self, reps=20):
        """Replays the last append: ms per batch."""
        ms = C.c_float()
        self._chk(self.L.yh_scene_batch_time(self.h, reps, C.byref(ms)))
        return ms.value

    def plan_time(self, reps=20):
        """Replays the last plan: dict(ms_per_batch, rounds, tile_runs)."""
        ms, r, t = C.c_float(), C.c_int32(), C.c_int32()
        self._chk(self.L.yh_scene_batch_plan_time(self.h, reps, C.byref(ms), C.byref(r), C.byref(t)))
        return dict(ms_per_batch=ms.value, rounds=r.value, tile_runs=t.value)

    def plan_tour(self, targets=None, n_targets=3, starts=None, connectivity=4):
        """The tour (Scene.plan_tour) of every frame of the last append in shared solver rounds. targets: [n][k] (x, y) pixels, k at
        most TOUR_MAX and distinct within a frame, or None: each frame's first n_targets balls (a ball on an earlier ball's pixel
        dropped, so frames may have fewer). starts and connectivity as plan().
        Returns the status list: OK, or ESTATE for a frame without a usable ball (it has no tour)."""
        n = self.n
        if starts is None:
            if (self.W, self.H) != (640, 480):
                raise ValueError("starts=None is the reference's START_NODE at 640x480; give the starts for other sizes")
            starts = [(400, 479)] * n
        s = np.ascontiguousarray(starts, np.int32).reshape(-1, 2)
        assert len(s) == n
        status = np.zeros(max(n, 1), np.int32)
        if targets is None:
            self._chk(self.L.yh_scene_batch_plan_tour(self.h, None, n_targets, _p(s), connectivity, _p(status)))
        else:
            t = np.ascontiguousarray(targets, np.int32)
            assert t.ndim == 3 and t.shape[0] == n and t.shape[2] == 2
            self._chk(self.L.yh_scene_batch_plan_tour(self.h, _p(t), t.shape[1], _p(s), connectivity, _p(status)))
        return [int(v) for v in status[:n]]

    def read_tour(self, b, fields=False):
        """Frame b of the last tour, as Scene.read_tour."""
        k, n, total = C.c_int32(), C.c_int32(), C.c_float()
        self._chk(self.L.yh_scene_batch_tour_read(self.h, b, C.byref(k), None, None, None, None, None, None, None, None, None, None, 0, C.byref(n)))
        K = k.value
        out = dict(targets=np.zeros((K, 2), np.int32), order=np.zeros(K, np.int32), legs=np.zeros((K + 1, K), np.float32),
                   path=np.zeros((n.value, 2), np.int32), leg_ends=np.zeros(K, np.int32))
        dirs = np.zeros((n.value, 2), np.float32)
        if fields:
            out["cost"] = np.zeros((K, self.H, self.W), np.float32)
            out["next"] = np.zeros((K, self.H, self.W), np.int32)
            out["label"] = np.zeros((self.H, self.W), np.uint8)
        f = lambda name: _p(out[name]) if fields else None
        self._chk(self.L.yh_scene_batch_tour_read(self.h, b, C.byref(k), _p(out["targets"]), _p(out["order"]), _p(out["legs"]), C.byref(total),
                                                  f("cost"), f("next"), f("label"), _p(out["path"]), _p(dirs), _p(out["leg_ends"]), n.value, C.byref(n)))
        out["total"] = np.float32(total.value)
        out["directions"] = dirs[:max(n.value - 1, 0)]
        return out

    def tour_time(self, reps=20):
        """Replays the last tour: dict(ms_per_batch, rounds, tile_runs)."""
        ms, r, t = C.c_float(), C.c_int32(), C.c_int32()
        self._chk(self.L.yh_scene_batch_tour_time(self.h, reps, C.byref(ms), C.byref(r), C.byref(t)))
        return dict(ms_per_batch=ms.value, rounds=r.value, tile_runs=t.value)

    def plan_turn(self, targets=None, n_targets=3, starts=None, headings=6, turn_price=2.0):
        """The turn-aware plan (Scene.plan_turn) of every frame of the last append in shared solver rounds. targets, n_targets,
        starts as plan(); headings: the start heading 0 .. 7, one int for all frames or a list of n; turn_price: one per call.
        Returns the status list: OK, or ESTATE for a frame without a usable ball (it has no turn plan)."""
        n = self.n
        if starts is None:
            if (self.W, self.H) != (640, 480):
                raise ValueError("starts=None is the reference's START_NODE at 640x480; give the starts for other sizes")
            starts = [(400, 479)] * n
        s = np.ascontiguousarray(starts, np.int32).reshape(-1, 2)
        hd = np.full(max(n, 1), headings, np.int32) if np.isscalar(headings) else np.ascontiguousarray(headings, np.int32).reshape(-1)
        assert len(s) == n and len(hd) >= n
        status = np.zeros(max(n, 1), np.int32)
        if targets is None:
            self._chk(self.L.yh_scene_batch_plan_turn(self.h, None, n_targets, _p(s), _p(hd), turn_price, _p(status)))
        else:
            t = np.ascontiguousarray(targets, np.int32)
            assert t.ndim == 3 and t.shape[0] == n and t.shape[2] == 2
            self._chk(self.L.yh_scene_batch_plan_turn(self.h, _p(t), t.shape[1], _p(s), _p(hd), turn_price, _p(status)))
        return [int(v) for v in status[:n]]

    def read_turn(self, b, fields=True):
        """Frame b of the last turn plan, as Scene.read_turn."""
        n = C.c_int32()
        self._chk(self.L.yh_scene_batch_turn_read(self.h, b, None, None, None, None, None, 0, C.byref(n)))
        out = dict(path=np.zeros((n.value, 2), np.int32))
        dirs, turns = np.zeros((n.value, 2), np.float32), np.zeros(n.value, np.int32)
        if fields:
            out["cost"] = np.zeros((8, self.H, self.W), np.float32)
            out["act"] = np.zeros((8, self.H, self.W), np.uint8)
        self._chk(self.L.yh_scene_batch_turn_read(self.h, b, _p(out["cost"]) if fields else None, _p(out["act"]) if fields else None,
                                                  _p(out["path"]), _p(dirs), _p(turns), n.value, C.byref(n)))
        out["directions"] = dirs[:max(n.value - 1, 0)]
        out["turns"] = turns[:max(n.value - 1, 0)]
        return out

    def turn_time(self, reps=20):
        """Replays the last turn plan: dict(ms_per_batch, rounds, tile_runs)."""
        ms, r, t = C.c_float(), C.c_int32(), C.c_int32()
        self._chk(self.L.yh_scene_batch_turn_time(self.h, reps, C.byref(ms), C.byref(r), C.byref(t)))
        return dict(ms_per_batch=ms.value, rounds=r.value, tile_runs=t.value)

    def plan_turn_tour(self, targets=None, n_targets=3, starts=None, headings=6, turn_price=2.0):
        """The turn-aware tour (Scene.plan_turn_tour) of every frame of the last append in shared solver rounds. targets: [n][k]
        (x, y) pixels, k at most TOUR_MAX and distinct within a frame, or None: each frame's first n_targets balls (a ball on an
        earlier ball's pixel dropped, so frames may have fewer). starts, headings and turn_price as plan_turn().
        Returns the status list: OK, or ESTATE for a frame without a usable ball (it has no turn tour)."""
        n = self.n
        if starts is None:
            if (self.W, self.H) != (640, 480):
                raise ValueError("starts=None is the reference's START_NODE at 640x480; give the starts for other sizes")
            starts = [(400, 479)] * n
        s = np.ascontiguousarray(starts, np.int32).reshape(-1, 2)
        hd = np.full(max(n, 1), headings, np.int32) if np.isscalar(headings) else np.ascontiguousarray(headings, np.int32).reshape(-1)
        assert len(s) == n and len(hd) >= n
        status = np.zeros(max(n, 1), np.int32)
        if targets is None:
            self._chk(self.L.yh_scene_batch_plan_turn_tour(self.h, None, n_targets, _p(s), _p(hd), turn_price, _p(status)))
        else:
            t = np.ascontiguousarray(targets, np.int32)
            assert t.ndim == 3 and t.shape[0] == n and t.shape[2] == 2
            self._chk(self.L.yh_scene_batch_plan_turn_tour(self.h, _p(t), t.shape[1], _p(s), _p(hd), turn_price, _p(status)))
        return [int(v) for v in status[:n]]

    def read_turn_tour(self, b, fields=True):
        """Frame b of the last turn tour, as Scene.read_turn_tour."""
        k, n, total = C.c_int32(), C.c_int32(), C.c_float()
        self._chk(self.L.yh_scene_batch_turn_tour_read(self.h, b, C.byref(k), None, None, None, None, None, None, None, None, None, None, None, None, None, 0, C.byref(n)))
        K = k.value
        out = dict(targets=np.zeros((K, 2), np.int32), order=np.zeros(K, np.int32), legs=np.zeros((1 + 8 * K, K), np.float32),
                   arrive=np.zeros((1 + 8 * K, K), np.uint8), leg_headings=np.zeros(K, np.int32), path=np.zeros((n.value, 2), np.int32),
                   leg_ends=np.zeros(K, np.int32))
        dirs, turns = np.zeros((n.value, 2), np.float32), np.zeros(n.value, np.int32)
        if fields:
            out["cost"] = np.zeros((K, 8, self.H, self.W), np.float32)
            out["act"] = np.zeros((K, 8, self.H, self.W), np.uint8)
            out["label"] = np.zeros((8, self.H, self.W), np.uint8)
        f = lambda name: _p(out[name]) if fields else None
        self._chk(self.L.yh_scene_batch_turn_tour_read(self.h, b, C.byref(k), _p(out["targets"]), _p(out["order"]), _p(out["legs"]), _p(out["arrive"]),
                                                       C.byref(total), _p(out["leg_headings"]), f("cost"), f("act"), f("label"), _p(out["path"]), _p(dirs),
                                                       _p(turns), _p(out["leg_ends"]), n.value, C.byref(n)))
        out["total"] = np.float32(total.value)
        out["directions"] = dirs[:max(n.value - 1, 0)]
        out["turns"] = turns[:max(n.value - 1, 0)]
        return out

    def turn_tour_time(self, reps=20):
        """Replays the last turn tour: dict(ms_per_batch, rounds, tile_runs)."""
        ms, r, t = C.c_float(), C.c_int32(), C.c_int32()
        self._chk(self.L.yh_scene_batch_turn_tour_time(self.h, reps, C.byref(ms), C.byref(r), C.byref(t)))
        return dict(ms_per_batch=ms.value, rounds=r.value, tile_runs=t.value)

    def set_fields(self, b, map, conn0, conn1):
        """Test hook: host fields for frame b as if a SANE frame had produced them (layouts of read())."""
        m = np.ascontiguousarray(map, np.uint32)
        c0, c1 = np.ascontiguousarray(conn0, np.float32), np.ascontiguousarray(conn1, np.float32)
        assert m.shape == (self.H, self.W) and c0.shape == (self.H, self.W, 4) and c1.shape == (self.H, self.W, 4)
        first = not getattr(self, "_fields", False)
        self._chk(self.L.yh_scene_batch_set_fields(self.h, b, _p(m), _p(c0), _p(c1)))
        self.n = b + 1 if first else max(self.n, b + 1)
        self._fields = True


def serialize_path(directions, created_secs):
    """Path::serialize (src/path.rs:17-21), byte for byte: `created` as big-endian u64 seconds since the epoch, then every
    (magnitude, rotation) pair as two big-endian f32 - what the reference answers to GetPath (path.rs:167-169)."""
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 2)
    return int(created_secs).to_bytes(8, "big") + d.astype(">f4").tobytes()


def tfl_validate(model_bytes):
    """Parse-only check of a .tflite buffer (no GPU): returns (ok, n_tensors, n_ops, message)."""
    L = load_library()
    nt, no = C.c_int32(), C.c_int32()
    err = C.create_string_buffer(512)
    rc = L.yh_tfl_validate(model_bytes, len(model_bytes), C.byref(nt), C.byref(no), err, 512)
    return rc == OK, nt.value, no.value, err.value.decode()


_KIND_NP = {1: np.float32, 3: np.uint8, 2: np.int32, 9: np.int8}
TFL_MAX_IMAGES = 512   # YH_TFL_MAX_IMAGES

# YH_TFL_FAM_* (include/yolact_hip_debug.h), by value
TFL_FAMILIES = ("conv_scalar", "conv_px8", "conv_dot1", "conv_dot4", "conv_i8_lds", "conv_i8_direct", "dw_scalar", "dw_c4",
                "add", "requant", "quantize_f32", "dequantize", "lut", "pad", "resize", "concat", "copy")


def tfl_priors(level_sizes, input_size, aspect_ratios=(1.0, 0.5, 2.0), base_scale=24.0):
    """YOLACT priors [P][4] (cx, cy, w, h; float32) for square feature levels of level_sizes cells at a square input of input_size
    pixels: level l carries anchors of base_scale * 2^l pixels at a 550-pixel input, one per aspect ratio, square (YOLACT's
    use_square_anchors) - the engine's prior table (Engine.priors()) in its arithmetic and order: level, row, column, anchor. A
    .tflite file holds no priors, so TfliteEngine.detect_setup takes these."""
    f = np.float32
    S = f(input_size)
    out = []
    for l, n in enumerate(level_sizes):
        scale = f(f(base_scale * 2.0 ** l) * S) / f(550.0)
        wv = np.array([f(f(scale * np.sqrt(f(a))) / S) for a in aspect_ratios], f)
        c = (np.arange(n, dtype=f) + f(0.5)) / f(n)
        q = np.empty((n, n, len(aspect_ratios), 4), f)
        q[..., 0] = c[None, :, None]
        q[..., 1] = c[:, None, None]
        q[..., 2] = wv[None, None, :]
        q[..., 3] = wv[None, None, :]
        out.append(q.reshape(-1, 4))
    return np.ascontiguousarray(np.concatenate(out, 0))


def tfl_direct_forms():
    """yh_tfl_direct_forms: the rows (D, once, KK) of the register-fed int8 convolution's table of forms (no GPU)."""
    L = load_library()
    n = L.yh_tfl_direct_forms(None, 0)
    rows = (_i * (3 * n))()
    L.yh_tfl_direct_forms(rows, n)
    return [(rows[3 * i], bool(rows[3 * i + 1]), rows[3 * i + 2]) for i in range(n)]


class TfliteEngine:
    """RAII wrapper of yh_tfl: the reference's own model family (MobileNetV2-style .tflite), uint8 per-tensor quantised or int8
    with per-tensor / per-channel weight scales and uint8 / float32 edges."""

    def __init__(self, model_bytes, device=0, tune=None, max_images=2):
        """max_images: images per invoke the handle has room for (yh_tfl_create_batch: 1 .. TFL_MAX_IMAGES; classify_batch on n frames
        needs 2n)."""
        self.L = load_library()
        h = C.c_void_p()
        t = Tuning.of(**(tune or {}))
        rc = self.L.yh_tfl_create_batch_tuned(model_bytes, len(model_bytes), device, int(max_images), C.byref(t), C.byref(h))
        if rc != OK:
            raise YhError(rc, self.L.yh_tfl_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.yh_tfl_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            raise YhError(rc, self.L.yh_tfl_last_error(self.h).decode())

    @staticmethod
    def _info(ti):
        return dict(name=ti.name.decode(), kind=ti.kind, dims=tuple(ti.dims[:ti.ndims]), scale=ti.scale, zero_point=ti.zero_point)

    def input_info(self):
        ti = TensorInfo()
        self._chk(self.L.yh_tfl_input_info(self.h, C.byref(ti)))
        return self._info(ti)

    def output_count(self):
        return self.L.yh_tfl_output_count(self.h)

    def output_info(self, i):
        ti = TensorInfo()
        self._chk(self.L.yh_tfl_output_info(self.h, i, C.byref(ti)))
        return self._info(ti)

    def set_batch(self, n):
        """1 .. max_images images per invoke (the two tiles of a frame as one pass); inputs / outputs / tensors then carry n images."""
        self._chk(self.L.yh_tfl_set_batch(self.h, n))
        self.nb = n

    def set_input(self, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.yh_tfl_set_input(self.h, _p(arr), arr.nbytes))

    def invoke(self):
        self._chk(self.L.yh_tfl_invoke(self.h))

    def output(self, i):
        info = self.output_info(i)
        nb = getattr(self, "nb", 1)
        out = np.empty(((nb,) + tuple(info["dims"])) if nb > 1 else info["dims"], _KIND_NP[info["kind"]])
        self._chk(self.L.yh_tfl_output_read(self.h, i, _p(out), out.nbytes))
        return out

    def plan_summary(self):
        """Launches per invoke of the prepared plan, CONV_2D launches and how many of those run on the int8 matrix pipes."""
        a, b, c = _i(), _i(), _i()
        self._chk(self.L.yh_tfl_plan_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(launches_per_invoke=a.value, conv2d_launches=b.value, conv2d_on_int8_mfma=c.value)

    def op_info(self, op):
        """yh_tfl_op_info: dict(family = a name of TFL_FAMILIES or None, row = the table-of-forms row or -1, grouped, folded) of
        operator `op` (file order) for the image count of the next invoke."""
        f, r, g, d = _i(), _i(), _i(), _i()
        self._chk(self.L.yh_tfl_op_info(self.h, op, C.byref(f), C.byref(r), C.byref(g), C.byref(d)))
        return dict(family=TFL_FAMILIES[f.value] if f.value >= 0 else None, row=r.value, grouped=bool(g.value), folded=bool(d.value))

    def op_quant(self, op):
        """yh_tfl_op_quant: dict(signed = the operator's output is int8 (True), uint8 (False) or another type (None); per_channel =
        it is an int8 convolution whose weights carry one scale per output channel)."""
        a, b = _i(), _i()
        self._chk(self.L.yh_tfl_op_quant(self.h, op, C.byref(a), C.byref(b)))
        return dict(signed=None if a.value < 0 else bool(a.value), per_channel=bool(b.value))

    def tensor(self, index, shape, dtype):
        nb = getattr(self, "nb", 1)
        out = np.empty(((nb,) + tuple(shape)) if nb > 1 else shape, dtype)
        self._chk(self.L.yh_tfl_tensor_read(self.h, index, _p(out), out.nbytes))
        return out

    def classify_frame(self, frame_u32, width, height, mode=COMPAT_STRICT):
        assert frame_u32.dtype == np.uint32 and frame_u32.flags.c_contiguous and frame_u32.size == width * height
        self._chk(self.L.yh_tfl_classify_frame_u32(self.h, _p(frame_u32), width, height, mode))

    def classify_batch(self, frames_u32=None, frames_dev_ptr=None, n=None, width=640, height=480, mode=COMPAT_STRICT, out=None,
                       read=True):
        """yh_tfl_classify_batch_u32: classify on n frames as one invoke of 2n images (DESIGN.md §11 "TFLite classify batch"; the
        handle needs max_images >= 2n). frames_u32: uint32 [n][height][width] on the host (n defaults to its first dimension), or
        frames_dev_ptr: a device pointer to the same layout with n given. out: the uint32 array to write, which may be frames_u32
        itself; None: a new array, or with read=False nothing is copied back. Returns (frames uint32 [n][height][width] or None;
        diverged int32 [n]), like Engine.classify_batch. On YH_EDIVERGE the YhError carries the flags as .diverged. The device
        copy: classify_batch_device_frames."""
        assert (frames_u32 is None) != (frames_dev_ptr is None), "give frames_u32 or frames_dev_ptr"
        if frames_u32 is not None:
            src = np.ascontiguousarray(frames_u32, np.uint32)
            if n is None:
                n = src.shape[0]
            assert src.size >= max(int(n), 0) * width * height, (src.shape, n, width, height)
            ptr, on_dev = _p(src), 0
        else:
            assert n is not None, "frames_dev_ptr needs n"
            ptr, on_dev = C.c_void_p(frames_dev_ptr), 1
        if out is not None:   # the array to write (it may be frames_u32 itself: in place)
            assert out.dtype == np.uint32 and out.flags.c_contiguous and out.size == int(n) * width * height
            res = out
        else:
            res = np.zeros((max(int(n), 0), height, width), np.uint32) if read else None
        div = np.zeros(max(int(n), 1), np.int32)
        try:
            self._chk(self.L.yh_tfl_classify_batch_u32(self.h, ptr, on_dev, int(n), width, height, mode,
                                                       _p(res) if res is not None else None, _p(div)))
        except YhError as e:
            e.diverged = div[:max(int(n), 0)].copy()
            raise
        return res, div[:int(n)]

    def classify_batch_device_frames(self):
        """Device pointer of the last classify_batch's frames [n][height][width] (None before a batch or after a failed one): what
        SceneBatch.stage_frames(frames_dev_ptr=...) takes."""
        return self.L.yh_tfl_classify_batch_device_frames(self.h)

    # ---- detections on the model's own outputs (DESIGN.md §11 "TFLite detections")
    def detect_setup(self, priors, **cfg):
        """yh_tfl_detect_setup: binds the detection tail to four of the model's outputs. priors: float32 [P][4] cx, cy, w, h
        (tfl_priors). cfg: outputs=(loc, conf, mask, proto) indices into the model's outputs (0, 1, 2, 3), top_k=200, max_dets=100,
        conf_thresh=0.05, nms_thresh=0.5, max_images=0 (the handle's): the images the workspaces are sized for - the candidate
        lists alone take max_images * (C - 1) * P * 8 bytes."""
        c = TflDetectConfig()
        self.L.yh_tfl_default_detect_config(C.byref(c))
        for k, v in cfg.items():
            if k == "outputs":
                c.outputs[:] = [int(x) for x in v]
            elif k == "reserved":
                c.reserved[:] = [int(x) for x in v]
            else:
                assert hasattr(c, k), k
                setattr(c, k, v)
        pr = np.ascontiguousarray(priors, np.float32)
        assert pr.ndim == 2 and pr.shape[1] == 4, pr.shape
        self._chk(self.L.yh_tfl_detect_setup(self.h, C.byref(c), _p(pr), pr.shape[0]))
        self._det_cfg = c

    def evaluate(self):
        """yh_tfl_evaluate: invoke + the tail on every image of the batch (asynchronous; detections() waits)."""
        self._chk(self.L.yh_tfl_evaluate(self.h))
        self._det_geo = None

    def detect(self):
        """yh_tfl_detect: the tail alone on the outputs of the last invoke / classify call."""
        self._chk(self.L.yh_tfl_detect(self.h))
        self._det_geo = None

    def detect_stage_times(self, reps=20):
        """yh_tfl_detect_stage_times: mean ms of each of the tail's four launches on the last invoke's outputs, timed by events."""
        ms = (_f * 4)()
        self._chk(self.L.yh_tfl_detect_stage_times(self.h, reps, C.byref(ms)))
        self._det_geo = None
        return list(ms)

    def proto_dims(self):
        d = (_i * 2)()
        self._chk(self.L.yh_tfl_proto_dims(self.h, C.byref(d)))
        return d[0], d[1]

    def _read_detections(self, image, max_dets, hp, wp, want_masks):
        nd = C.c_int32()
        dets = (Detection * max_dets)()
        masks = np.zeros((max_dets, hp, wp), np.uint8) if want_masks else None
        self._chk(self.L.yh_tfl_read_detections(self.h, image, C.byref(nd), C.cast(dets, C.c_void_p), max_dets,
                                                _p(masks) if want_masks else None, masks.size if want_masks else 0))
        out = [dict(class_id=d.class_id, prior=d.prior, score=d.score, box=tuple(d.box)) for d in dets[:nd.value]]
        return out, (masks[:nd.value] if want_masks else None)

    def detections(self, image, want_masks=True):
        """yh_tfl_read_detections for image `image` of the last evaluate / detect / op_detect: (list of dict(class_id, prior, score,
        box), masks uint8 [nd][hp][wp] or None), as Engine.detections."""
        geo = getattr(self, "_det_geo", None)   # (op_detect's geometry while its results are the current ones)
        if geo is None and getattr(self, "_det_cfg", None) is None:   # no setup, no op_detect: the library's own answer (YH_ESTATE)
            nd = C.c_int32()
            self._chk(self.L.yh_tfl_read_detections(self.h, image, C.byref(nd), None, 0, None, 0))
        if geo is None:
            hp, wp = self.proto_dims()
            geo = (self._det_cfg.max_dets, hp, wp)
        return self._read_detections(image, geo[0], geo[1], geo[2], want_masks)

    def op_detect(self, loc, conf, mask, proto, priors, quant=None, top_k=200, max_dets=100, conf_thresh=0.05, nms_thresh=0.5):
        """yh_tfl_op_detect: the tail on caller-provided tensors, no model involved. loc [n][P][4], conf [n][P][C], mask [n][P][32],
        proto [n][hp][wp][32], each uint8, int8 or float32; quant: dict role -> (scale, zero_point) for the quantised ones. The
        results are read with detections()."""
        arrs, args = [], []
        for name, a in (("loc", loc), ("conf", conf), ("mask", mask), ("proto", proto)):
            a = np.ascontiguousarray(a)
            kind = {np.dtype(np.uint8): 3, np.dtype(np.int8): 9, np.dtype(np.float32): 1}[a.dtype]
            sc, zp = (quant or {}).get(name, (1.0, 0))
            arrs.append(a)
            args += [_p(a), kind, float(sc), int(zp)]
        n, P, Cc = arrs[1].shape
        hp, wp = arrs[3].shape[1:3]
        assert arrs[0].shape == (n, P, 4) and arrs[2].shape == (n, P, 32) and arrs[3].shape == (n, hp, wp, 32)
        pr = np.ascontiguousarray(priors, np.float32)
        assert pr.shape == (P, 4)
        self._det_geo = None
        self._chk(self.L.yh_tfl_op_detect(self.h, n, P, Cc, hp, wp, *args, _p(pr), top_k, max_dets, conf_thresh, nms_thresh))
        self._det_geo = (max_dets, hp, wp)

    # ---- instance frames from the setup's detections (DESIGN.md §11 "TFLite instance frames")
    def _inst_class_map(self, class_map, ncls=None):
        if class_map is None:
            return None
        cm = np.ascontiguousarray(class_map, np.uint8)
        if ncls is None:   # the setup's C - 1, from the conf output bound by detect_setup
            assert getattr(self, "_det_cfg", None) is not None, "class_map needs detect_setup"
            ncls = self.output_info(self._det_cfg.outputs[1])["dims"][-1] - 1
        assert cm.shape == (ncls,), "class_map: one value per foreground class"
        return cm

    def instance_batch(self, first, n, width, height, class_map=None, min_score=0.0, read=True):
        """yh_tfl_instance_batch: images first .. first + n - 1 of the last evaluate / detect, each painted as Engine.instance_batch
        paints a frame. Returns uint32 [n][height][width], or None with read=False (the frames stay on the device:
        instance_device_frames; the tables, rows of 4: instances_of)."""
        cm = self._inst_class_map(class_map)
        out = np.zeros((max(n, 0), height, width), np.uint32) if read else None
        self._chk(self.L.yh_tfl_instance_batch(self.h, first, n, width, height, _p(cm) if cm is not None else None, C.c_float(min_score),
                                               _p(out) if read else None))
        return out

    def instance_frames(self, first, n, width, height, class_map=None, min_score=0.0, read=True):
        """yh_tfl_instance_frames: camera frames first .. first + n - 1, frame b painted from images 2b (the left tile) and 2b + 1
        of the last tail - what detect() after classify_batch leaves. Returns uint32 [n][height][width], or None with read=False
        (instance_device_frames; the tables, rows of 5 = (tile, rank, class, id, pixels): instances_of)."""
        cm = self._inst_class_map(class_map)
        out = np.zeros((max(n, 0), height, width), np.uint32) if read else None
        self._chk(self.L.yh_tfl_instance_frames(self.h, first, n, width, height, _p(cm) if cm is not None else None, C.c_float(min_score),
                                                _p(out) if read else None))
        return out

    def instance_device_frames(self):
        """Device pointer of the last instance batch's frames [n][height][width] (None before a batch or after a failed one): what
        SceneBatch.stage_frames(frames_dev_ptr=...) takes."""
        return self.L.yh_tfl_instance_device_frames(self.h)

    def instances_of(self, i):
        """The instance table of image / frame i of the last batch: int32 [m][4] = (rank, output class, id, pixels won) after
        instance_batch, int32 [m][5] = (tile, rank within the tile, output class, id, pixels won) after instance_frames."""
        n = C.c_int32()
        self._chk(self.L.yh_tfl_instance_read(self.h, i, C.byref(n), None, 0))
        w = self.L.yh_tfl_instance_row_width(self.h)
        t = np.zeros((n.value, w), np.int32)
        self._chk(self.L.yh_tfl_instance_read(self.h, i, C.byref(n), _p(t), n.value))
        return t

    def op_instance_frames(self, masks, class_ids, scores, counts, width, height, class_map=None, min_score=0.0):
        """yh_tfl_op_instance_frames: instance_frames' kernels on caller-provided masks uint8 [2n][n_dets][hp][wp], class ids and
        scores [2n][n_dets] in rank order per image, counts [2n]; image 2b is the left tile of frame b. class_map: up to 80 values
        (the rest 0). Returns (frames uint32 [n][height][width], the list of the frames' tables)."""
        masks = np.ascontiguousarray(masks, np.uint8)
        ni, nd, hp, wp = masks.shape
        assert ni % 2 == 0, "two images per camera frame"
        ids = np.ascontiguousarray(class_ids, np.int32).reshape(ni, nd)
        sc = np.ascontiguousarray(scores, np.float32).reshape(ni, nd)
        cnt = np.ascontiguousarray(counts, np.int32).reshape(ni)
        cm = None
        if class_map is not None:
            given = np.ascontiguousarray(class_map, np.uint8).reshape(-1)
            assert given.size <= 80, "class_map: at most 80 foreground classes"
            cm = np.zeros(80, np.uint8)
            cm[:given.size] = given
        out = np.zeros((ni // 2, height, width), np.uint32)
        self._chk(self.L.yh_tfl_op_instance_frames(self.h, _p(masks), _p(ids), _p(sc), _p(cnt), ni // 2, nd, hp, wp, width, height,
                                                   _p(cm) if cm is not None else None, C.c_float(min_score), _p(out)))
        return out, [self.instances_of(b) for b in range(ni // 2)]
