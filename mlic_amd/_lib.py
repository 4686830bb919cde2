"""ctypes binding of libmlic_hip.so (C ABI in include/mlic_hip.h).

The library is built in-tree (`python -m mlic_amd.build` or __graft_entry__.build()).  There is no
fallback: if the shared object is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MLIC_HIP_LIB", os.path.join(_HERE, "libmlic_hip.so"))

_lock = threading.Lock()
_lib = None


class MlicError(RuntimeError):
    pass


class ContainerInfo(C.Structure):
    """mlic_container_info (include/mlic_hip.h)."""
    _fields_ = [("H", C.c_uint32), ("W", C.c_uint32), ("hz", C.c_uint32), ("wz", C.c_uint32), ("level", C.c_int32),
                ("reserved", C.c_int32), ("y_off", C.c_uint64), ("y_len", C.c_uint64), ("z_off", C.c_uint64),
                ("z_len", C.c_uint64)]


class ContainerRoiInfo(C.Structure):
    """mlic_container_roi_info (include/mlic_hip.h)."""
    _fields_ = [("file", ContainerInfo), ("map_off", C.c_uint64), ("map_len", C.c_uint64)]


class ContainerTiledInfo(C.Structure):
    """mlic_container_tiled_info (include/mlic_hip.h)."""
    _fields_ = [("H", C.c_uint32), ("W", C.c_uint32), ("T", C.c_uint32), ("V", C.c_uint32), ("ny", C.c_uint32),
                ("nx", C.c_uint32), ("vbr", C.c_int32), ("reserved", C.c_int32), ("table_off", C.c_uint64),
                ("payload_off", C.c_uint64), ("payload_len", C.c_uint64)]


class ContainerScaledInfo(C.Structure):
    """mlic_container_scaled_info (include/mlic_hip.h)."""
    _fields_ = [("H", C.c_uint32), ("W", C.c_uint32), ("filter", C.c_int32), ("vbr", C.c_int32),
                ("inner_off", C.c_uint64), ("inner_len", C.c_uint64), ("inner", ContainerInfo)]


class ContainerResidualInfo(C.Structure):
    """mlic_container_residual_info (include/mlic_hip.h)."""
    _fields_ = [("H", C.c_uint32), ("W", C.c_uint32), ("tau", C.c_int32), ("vbr", C.c_int32), ("digest", C.c_uint64),
                ("m", C.c_uint8 * 24), ("freq_off", C.c_uint64 * 24), ("inner_off", C.c_uint64),
                ("inner_len", C.c_uint64), ("res_off", C.c_uint64), ("res_len", C.c_uint64), ("inner", ContainerInfo)]


class ContainerResidualSegInfo(C.Structure):
    """mlic_container_residual_seg_info (include/mlic_hip.h)."""
    _fields_ = [("H", C.c_uint32), ("W", C.c_uint32), ("tau", C.c_int32), ("vbr", C.c_int32), ("digest", C.c_uint64),
                ("m", C.c_uint8 * 24), ("freq_off", C.c_uint64 * 24), ("seg_len", C.c_uint32), ("n_seg", C.c_uint32),
                ("inner_off", C.c_uint64), ("inner_len", C.c_uint64), ("res_off", C.c_uint64), ("res_len", C.c_uint64),
                ("index_off", C.c_uint64), ("data_off", C.c_uint64), ("data_len", C.c_uint64), ("inner", ContainerInfo)]


class ContainerResidualDeepInfo(C.Structure):
    """mlic_container_residual_deep_info (include/mlic_hip.h)."""
    _fields_ = [("H", C.c_uint32), ("W", C.c_uint32), ("tau", C.c_int32), ("vbr", C.c_int32), ("digest", C.c_uint64),
                ("m", C.c_uint8 * 24), ("freq_off", C.c_uint64 * 24), ("seg_len", C.c_uint32), ("n_seg", C.c_uint32),
                ("inner_off", C.c_uint64), ("inner_len", C.c_uint64), ("res_off", C.c_uint64), ("res_len", C.c_uint64),
                ("index_off", C.c_uint64), ("data_off", C.c_uint64), ("data_len", C.c_uint64), ("depth", C.c_int32),
                ("shift", C.c_int32), ("lo_off", C.c_uint64), ("lo_len", C.c_uint64), ("inner", ContainerInfo)]


class ContainerResidualYuvInfo(C.Structure):
    """mlic_container_residual_yuv_info (include/mlic_hip.h)."""
    _fields_ = [("H", C.c_uint32), ("W", C.c_uint32), ("tau", C.c_int32), ("vbr", C.c_int32), ("digest", C.c_uint64),
                ("m", C.c_uint8 * 24), ("freq_off", C.c_uint64 * 24), ("seg_len", C.c_uint32), ("n_seg", C.c_uint32),
                ("inner_off", C.c_uint64), ("inner_len", C.c_uint64), ("res_off", C.c_uint64), ("res_len", C.c_uint64),
                ("index_off", C.c_uint64), ("data_off", C.c_uint64), ("data_len", C.c_uint64), ("depth", C.c_int32),
                ("shift", C.c_int32), ("lo_off", C.c_uint64), ("lo_len", C.c_uint64), ("sub_x", C.c_int32),
                ("sub_y", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32), ("site_x", C.c_int32),
                ("inner", ContainerInfo)]


class ContainerLayeredInfo(C.Structure):
    """mlic_container_layered_info (include/mlic_hip.h)."""
    _fields_ = [("H", C.c_uint32), ("W", C.c_uint32), ("hz", C.c_uint32), ("wz", C.c_uint32), ("level", C.c_int32),
                ("S", C.c_uint32), ("layers_present", C.c_uint32), ("z_off", C.c_uint64), ("z_len", C.c_uint64),
                ("layer_off", C.c_uint64 * 32), ("layer_len", C.c_uint64 * 32)]


class YuvDesc(C.Structure):
    """mlic_yuv_desc (include/mlic_hip.h)."""
    _fields_ = [("sub_x", C.c_int32), ("sub_y", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32),
                ("site_x", C.c_int32), ("reserved", C.c_int32 * 3)]


class QuantDesc(C.Structure):
    """mlic_quant_desc (include/mlic_hip.h)."""
    _fields_ = [("y", C.c_void_p), ("y_bs", C.c_int64), ("params", C.c_void_p), ("params_bs", C.c_int64),
                ("params_a", C.c_void_p), ("params_a_bs", C.c_int64), ("yh", C.c_void_p), ("yh_bs", C.c_int64),
                ("lik", C.c_void_p), ("lik_bs", C.c_int64), ("sym", C.c_void_p), ("idx", C.c_void_p),
                ("sym16", C.c_void_p), ("idx8", C.c_void_p), ("ovf", C.c_void_p), ("nlim", C.c_int32),
                ("ntable", C.c_int32), ("table", C.c_void_p), ("phase", C.c_int32), ("vbr", C.c_int32),
                ("sc", C.c_void_p), ("rs", C.c_void_p), ("scp", C.c_void_p), ("rsp", C.c_void_p),
                ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


def _sig(lib):
    p, i, i64, f, sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
    P = C.POINTER
    lib.mlic_last_error.restype = C.c_char_p
    lib.mlic_version.restype = C.c_char_p
    sigs = {
        "mlic_create": [C.c_char_p, i, P(C.c_char_p), P(p), P(i64), P(i), p, P(p)],
        "mlic_destroy": [p],
        "mlic_forward": [p, p, p, i, i, i, p, p, p, f],
        "mlic_forward_v": [p, p, p, i, i, i, p, p, p, p],
        "mlic_compress_v": [p, p, p, i, i, i, p],
        "mlic_decompress_v": [p, p, P(p), P(sz), P(p), P(sz), i, i, i, p, p],
        "mlic_set_entropy_tables": [p, p, p, p, i, i, p, p, p, i, i],
        "mlic_compress": [p, p, p, i, i, i, f],
        "mlic_encoded_size": [p, i, P(sz), P(sz)],
        "mlic_encoded_copy": [p, i, p, p],
        "mlic_encoded_streams": [p, i, P(i64), P(i64), p, p, p],
        "mlic_decompress": [p, p, P(p), P(sz), P(p), P(sz), i, i, i, p, f],
        "mlic_run_module": [p, p, C.c_char_p, i, p, p, i, i, i, i, p],
        "mlic_workspace_bytes": [p, P(sz), P(sz)],
        "mlic_local_attn_mask": [p, p, i, i],
        "mlic_set_profiling": [p, i],
        "mlic_set_lanes": [p, i],
        "mlic_set_priority_base": [p, i],
        "mlic_set_precision": [p, i],
        "mlic_set_synthesis_precision": [p, i],
        "mlic_set_poison": [p, i],
        "mlic_set_kernel_option": [C.c_char_p, i],
        "mlic_get_kernel_option": [C.c_char_p, P(i)],
        "mlic_ab_families": [P(i)],
        "mlic_batch_stream": [p, i, i, p, sz, P(sz)],
        "mlic_decompress_batch_stream": [p, p, p, sz, P(p), P(sz), i, i, i, p, p],
        "mlic_range_fallbacks": [p, P(i64), P(i64), P(i64), i],
        "mlic_profile_layers": [p, p, sz, P(sz)],
        "mlic_bench_conv": [i, i, i, i, i, i, i, i, i, i, P(C.c_double), P(C.c_double)],
        "mlic_profile_read": [p, i, P(i64), P(C.c_double), P(C.c_double), P(C.c_double)],
        "mlic_profile_categories": [P(i)],
        "mlic_host_stats": [p, P(C.c_double), P(C.c_double), P(C.c_double), i],
        "mlic_profile_category_name": [i, p, sz],
        "mlic_conv_run": [p, i, p, p, p, p, i, i, i, i, i, i, i, i, p, p],
        "mlic_conv_choice": [i, i, i, i, i, i, i, i, P(i)],
        "mlic_dw_run": [p, p, p, p, p, i, i, i, i, i, i],
        "mlic_dwpw_run": [p, p, p, p, p, p, p, i, i, i, i, i, i, p],
        "mlic_local_attn_run": [p, i, p, p, p, p, i, i, i, i, f],
        "mlic_local_attn_packed_run": [p, p, p, p, p, i, i, i, f],
        "mlic_local_attn_packed_half_run": [p, p, p, p, p, i, i, i, f, i],
        "mlic_linatt_splits": [i, P(i)],
        "mlic_linear_attention_run": [p, p, p, p, p, p, i, i, i, i, i, i, i, i],
        "mlic_linatt_pack_run": [p, p, p, p, i, i, i, i, i, i, i],
        "mlic_ln_channels_run": [p, p, p, p, p, i, i, i],
        "mlic_taps_gather_run": [p, p, p, p, i, i, i],
        "mlic_quant_phase_run": [p, P(QuantDesc)],
        "mlic_phase_indexes_run": [p, P(QuantDesc)],
        "mlic_phase_dequant_run": [p, P(QuantDesc)],
        "mlic_phase_fill_run": [p, P(QuantDesc)],
        "mlic_layer_streams": [p, i, P(p), P(sz), i, P(i)],
        "mlic_decompress_prefix": [p, p, P(p), P(sz), i, P(p), P(sz), i, i, i, i, i, p, p],
        "mlic_container_layered_bytes": [sz, P(sz), i, i, P(sz)],
        "mlic_container_write_layered": [C.c_uint32, C.c_uint32, i, C.c_uint32, C.c_uint32, p, sz, P(p), P(sz), i, p,
                                         sz, P(sz)],
        "mlic_container_parse_layered": [p, sz, i, C.c_uint64, i, P(ContainerLayeredInfo)],
        "mlic_recip_plane_run": [p, p, p, i64],
        "mlic_eb_forward_run": [p] * 20 + [i, i, i, i],
        "mlic_eb_dequant_run": [p, p, p, p, i, i, i, i],
        "mlic_ckbd_mask_run": [p, p, i64, p, i64, i, i, i, i, i],
        "mlic_image_sq_err_u8": [p, p, p, i, i64, p],
        "mlic_ms_ssim_scratch_bytes": [i, i, i, i, P(sz)],
        "mlic_image_ms_ssim_u8": [p, p, P(i64), p, P(i64), i, i, i, i, p, sz, p, p],
        "mlic_lpips_create": [i, P(C.c_char_p), P(p), P(i64), P(i), p, P(p)],
        "mlic_lpips_destroy": [p],
        "mlic_lpips_set_precision": [p, i],
        "mlic_lpips_scratch_bytes": [i, i, i, P(sz)],
        "mlic_image_lpips_u8": [p, p, p, P(i64), p, P(i64), i, i, i, p, sz, p, p],
        "mlic_lpips_range_fallbacks": [p, P(i64), i],
        "mlic_lpips_profile": [p, i, P(C.c_double)],
        "mlic_dists_create": [i, P(C.c_char_p), P(p), P(i64), P(i), p, P(p)],
        "mlic_dists_destroy": [p],
        "mlic_dists_set_precision": [p, i],
        "mlic_dists_scratch_bytes": [i, i, i, P(sz)],
        "mlic_image_dists_u8": [p, p, p, P(i64), p, P(i64), i, i, i, p, sz, p, p],
        "mlic_dists_range_fallbacks": [p, P(i64), i],
        "mlic_dists_profile": [p, i, P(C.c_double)],
        "mlic_image_ingest_u8": [p, p, P(i64), i, i, i, p, i, i],
        "mlic_image_egress_u8": [p, p, P(i64), i, i, i, p, P(i64), p, P(i64), p],
        "mlic_image_blur3_pad": [p, p, p, i, i, i, i, i, p, p],
        "mlic_container_bytes": [sz, sz, i, P(sz)],
        "mlic_container_write": [C.c_uint32, C.c_uint32, i, C.c_uint32, C.c_uint32, p, sz, p, sz, p, sz, P(sz)],
        "mlic_container_parse": [p, sz, i, i, C.c_uint64, P(ContainerInfo)],
        "mlic_forward_g": [p, p, p, i, i, i, p, p, p, p],
        "mlic_compress_g": [p, p, p, i, i, i, p],
        "mlic_decompress_g": [p, p, P(p), P(sz), P(p), P(sz), i, i, i, p, p],
        "mlic_image_roi_levels_u8": [p, p, P(i64), i, i, i, i, i, p],
        "mlic_roi_gain_plane": [p, p, i, i, i, P(f), i, p],
        "mlic_image_sq_err_roi_u8": [p, p, P(i64), p, P(i64), p, P(i64), i, i, i, p],
        "mlic_rate_map_run": [p, p, i64, p, i64, i, i, i, i, i, i, p, p, p, p],
        "mlic_image_sq_err_blocks_u8": [p, p, P(i64), p, P(i64), i, i, i, i, p],
        "mlic_image_heat_u8": [p, p, i, i, i, i, C.c_double, C.c_double, i, i, i, p, P(i64), p, P(i64), i],
        "mlic_container_write_roi": [C.c_uint32, C.c_uint32, i, C.c_uint32, C.c_uint32, p, sz, p, sz, p, p, sz, P(sz)],
        "mlic_container_parse_roi": [p, sz, i, C.c_uint64, P(ContainerRoiInfo), p, sz],
        "mlic_tile_grid": [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint32), P(C.c_uint32), p, sz],
        "mlic_image_tile_blend_u8": [p, p, p, i, i, i, i, i, i, i, i, p, P(i64), p, P(i64), p],
        "mlic_container_write_tiled": [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, i, p, p, sz, p, sz, P(sz)],
        "mlic_container_parse_tiled": [p, sz, C.c_uint64, P(ContainerTiledInfo)],
        "mlic_container_tiled_tile": [p, sz, P(ContainerTiledInfo), C.c_uint64, P(C.c_uint64), P(C.c_uint64)],
        "mlic_encode_image_u8": [p, p, p, P(i64), i, i, f, i, p, sz, P(sz)],
        "mlic_encode_image_u8_budget": [p, p, p, P(i64), i, i, f, i, C.c_double, i, p, sz, P(sz), P(i)],
        "mlic_decode_image_u8": [p, p, p, sz, i, C.c_uint64, p, p, P(i64), sz, P(i), P(i), P(i)],
        "mlic_resample_table": [i, i, i, p, p, p, i, P(i)],
        "mlic_image_ingest_u8_scaled": [p, p, P(i64), i, i, i, i, i, i, p, i, i],
        "mlic_image_egress_u8_scaled": [p, p, P(i64), i, i, i, i, i, i, p, P(i64), p, P(i64), p],
        "mlic_container_write_scaled": [C.c_uint32, C.c_uint32, i, i, p, sz, p, sz, P(sz)],
        "mlic_container_parse_scaled": [p, sz, i, C.c_uint64, P(ContainerScaledInfo)],
        "mlic_encode_image_u8_scaled": [p, p, p, P(i64), i, i, i, i, i, f, i, p, sz, P(sz)],
        "mlic_image_residual_front_u8": [p, p, P(i64), p, P(i64), i, i, i, i, p, p, p, p, p, p],
        "mlic_image_residual_apply_u8": [p, p, P(i64), p, i, i, i, i, p, P(i64), p, P(i64), p, p],
        "mlic_residual_tables": [p, p, p, p, p, p],
        "mlic_container_write_residual": [C.c_uint32, C.c_uint32, i, i, C.c_uint64, p, p, p, sz, p, sz, p, sz, P(sz)],
        "mlic_container_parse_residual": [p, sz, i, C.c_uint64, P(ContainerResidualInfo)],
        "mlic_residual_segments_scratch_bytes": [i, i64, P(sz)],
        "mlic_residual_encode_segments": [p, p, p, i, i, i, p, p, i, i64, p, sz, p, p, p, sz, p],
        "mlic_residual_decode_segments": [p, p, sz, p, p, p, i, i, i, p, p, i, i64, p, p, sz, p],
        "mlic_residual_encode_segments_host": [p, p, i, i, i, p, p, i, i64, p, sz, p, p],
        "mlic_residual_decode_segments_host": [p, sz, p, p, p, i, i, i, p, p, i, i64, p],
        "mlic_container_write_residual_seg": [C.c_uint32, C.c_uint32, i, i, C.c_uint64, p, p, C.c_uint32, C.c_uint32, p,
                                              p, sz, p, sz, p, sz, P(sz)],
        "mlic_container_parse_residual_seg": [p, sz, i, C.c_uint64, P(ContainerResidualSegInfo)],
        "mlic_image_residual_front_u16": [p, p, P(i64), p, P(i64), i, i, i, i, i, i, p, p, p, p, p, p, p, p, p],
        "mlic_image_residual_stats_u16": [p, p, P(i64), p, P(i64), i, i, i, i, i, p, p],
        "mlic_image_residual_apply_u16": [p, p, P(i64), p, p, i, i, i, i, i, i, p, P(i64), p, P(i64), p, p, p],
        "mlic_residual_shift": [i, C.c_uint64, C.c_uint32, C.c_uint64, P(i)],
        "mlic_container_write_residual_deep": [C.c_uint32, C.c_uint32, i, i, i, i, C.c_uint64, p, p, C.c_uint32,
                                               C.c_uint32, p, p, sz, p, sz, p, sz, p, sz, P(sz)],
        "mlic_container_parse_residual_deep": [p, sz, i, C.c_uint64, P(ContainerResidualDeepInfo)],
        "mlic_decode_image_u8_sized": [p, p, p, sz, i, C.c_uint64, p, i, i, i, p, P(i64), sz, P(i), P(i), P(i), P(i),
                                       P(i)],
        "mlic_image_ingest_yuv8": [p, p, P(i64), p, P(i64), p, P(i64), P(YuvDesc), i, i, i, p, i, i],
        "mlic_image_egress_yuv8": [p, p, P(i64), i, i, i, P(YuvDesc), p, P(i64), p, P(i64), p, P(i64), p, P(i64), p,
                                   P(i64), p, P(i64), p],
        "mlic_encode_image_yuv8": [p, p, p, P(i64), p, P(i64), p, P(i64), P(YuvDesc), i, i, f, i, p, sz, P(sz)],
        "mlic_decode_image_yuv8": [p, p, p, sz, i, C.c_uint64, p, P(YuvDesc), p, P(i64), sz, p, P(i64), sz, p, P(i64),
                                   sz, P(i), P(i), P(i)],
        "mlic_image_ingest_u16": [p, p, P(i64), i, i, i, i, i, p, i, i],
        "mlic_image_egress_u16": [p, p, P(i64), i, i, i, i, i, p, P(i64), p, P(i64), p],
        "mlic_image_ingest_yuv16": [p, p, P(i64), p, P(i64), p, P(i64), P(YuvDesc), i, i, i, i, i, p, i, i],
        "mlic_image_egress_yuv16": [p, p, P(i64), i, i, i, P(YuvDesc), i, i, p, P(i64), p, P(i64), p, P(i64), p,
                                    P(i64), p, P(i64), p, P(i64), p],
        "mlic_encode_image_yuv16": [p, p, p, P(i64), p, P(i64), p, P(i64), P(YuvDesc), i, i, i, i, f, i, p, sz, P(sz)],
        "mlic_decode_image_yuv16": [p, p, p, sz, i, C.c_uint64, p, P(YuvDesc), i, i, p, P(i64), sz, p, P(i64), sz, p,
                                    P(i64), sz, P(i), P(i), P(i)],
        "mlic_residual_segments_scratch_bytes_n": [i, i64, i, P(sz)],
        "mlic_residual_encode_segments_n": [p, p, p, i, i64, p, p, i, i64, p, sz, p, p, p, sz, p],
        "mlic_residual_decode_segments_n": [p, p, sz, p, p, p, i, i64, p, p, i, i64, p, p, sz, p],
        "mlic_residual_encode_segments_host_n": [p, p, i, i64, p, p, i, i64, p, sz, p, p],
        "mlic_residual_decode_segments_host_n": [p, sz, p, p, p, i, i64, p, p, i, i64, p],
        "mlic_image_residual_front_yuv8": [p] + [p, P(i64)] * 6 + [P(YuvDesc), i, i, i, i, i] + [p] * 9,
        "mlic_image_residual_stats_yuv8": [p] + [p, P(i64)] * 6 + [P(YuvDesc), i, i, i, i, p, p],
        "mlic_image_residual_apply_yuv8": [p] + [p, P(i64)] * 3 + [p, p, P(YuvDesc), i, i, i, i, i] +
                                          [p, P(i64)] * 6 + [p, p, p],
        "mlic_image_residual_front_yuv16": [p] + [p, P(i64)] * 6 + [P(YuvDesc), i, i, i, i, i, i, i] + [p] * 9,
        "mlic_image_residual_stats_yuv16": [p] + [p, P(i64)] * 6 + [P(YuvDesc), i, i, i, i, i, i, p, p],
        "mlic_image_residual_apply_yuv16": [p] + [p, P(i64)] * 3 + [p, p, P(YuvDesc), i, i, i, i, i, i, i] +
                                           [p, P(i64)] * 6 + [p, p, p],
        "mlic_residual_yuv_samples": [i, i, i, i, P(C.c_uint64)],
        "mlic_residual_yuv_plane_words": [i, i, i, i, i, P(C.c_uint64)],
        "mlic_container_write_residual_yuv": [C.c_uint32, C.c_uint32, i, i, i, i, i, i, i, i, i, C.c_uint64, p, p,
                                              C.c_uint32, C.c_uint32, p, p, sz, p, sz, p, sz, p, sz, P(sz)],
        "mlic_container_parse_residual_yuv": [p, sz, i, C.c_uint64, P(ContainerResidualYuvInfo)],
        "mlic_neglog2_sum": [p, p, i, i64, p],
        "mlic_gaussian_likelihood": [p, p, p, p, i64, f, p],
        "mlic_scale_indexes": [p, p, i64, p, i, p],
        "mlic_encoded_bits": [p, i, P(C.c_double), P(C.c_double)],
        "mlic_pmf_to_quantized_cdf": [p, i, i, p],
        "mlic_rans_encode": [p, p, i64, p, p, p, i, i, p, sz, P(sz)],
        "mlic_rans_decode": [p, sz, p, i64, p, p, p, i, i, p],
        "mlic_rans_decode_narrow": [p, sz, p, i64, i, p, p, p, i, i, p, P(i)],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    return lib


def _check_build_record():
    """The in-tree library must be the build of the sources in the tree (mlic_amd/build.py record)."""
    import json
    from . import build as _build
    if os.environ.get("MLIC_HIP_LIB"):
        return  # an explicitly chosen library (A/B builds): the caller vouches for it
    rec_path = _build.RECORD
    if not os.path.exists(rec_path):
        raise MlicError(f"{rec_path} missing: rebuild with `python -m mlic_amd.build` (records the sources the "
                        f"library was built from)")
    with open(rec_path) as f:
        rec = json.load(f)
    if rec.get("sources_sha256") != _build.source_digest():
        raise MlicError("libmlic_hip.so was built from other sources than the ones in this tree (stale build): "
                        "rebuild with `python -m mlic_amd.build`")


def lib():
    """The loaded library (raises if it was not built, or was built from other sources)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise MlicError(f"libmlic_hip.so not found at {LIB_PATH}: build it with "
                                f"`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
            _check_build_record()
            _lib = _sig(C.CDLL(LIB_PATH))
    return _lib


def poison() -> bool:
    """$MLIC_POISON=1 (test switch): the executor NaN-fills its workspace blocks on allocation and the
    Python layer NaN-fills the output tensors it hands to the library, so any element a kernel does
    not write, or any read of memory its producer never wrote, shows up as NaN."""
    return os.environ.get("MLIC_POISON", "0") not in ("", "0")


def ab_families() -> bool:
    """True when the loaded library holds the A/B-only kernel families (make AB=1)."""
    v = C.c_int()
    call("mlic_ab_families", C.byref(v))
    return bool(v.value)


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().mlic_last_error().decode(errors="replace")
        raise MlicError(f"{what}: {msg}" if what else msg)


def call(name: str, *args):
    check(getattr(lib(), name)(*args), name)
