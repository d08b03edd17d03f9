"""ctypes binding of ``libstereo_match_amd.so`` (C-ABI: include/stereo_match_amd.h).

The product path has NO CPU fallback: if the in-tree HIP library is missing,
``load()`` raises ``ImportError`` with the build command.  Nothing here
imports ``oracle/``.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# STEREO_MATCH_AMD_LIB: alternative build of the same library (kernel experiments only)
LIB_PATH = os.environ.get("STEREO_MATCH_AMD_LIB") or os.path.join(_HERE, "libstereo_match_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "stereo_match_amd.h")

SM_OK, SM_E_ARG, SM_E_HIP, SM_E_UNSUPPORTED = 0, -1, -2, -4
SM_E_DATA = -5
SM_COST_SGBM, SM_COST_CENSUS, SM_COST_VOLUME = 0, 1, 2
SM_MODE_SGBM, SM_MODE_HH = 5, 8
TIMING_ONLY = 0x40000000  # include/stereo_match_amd.h SM_TIMING_ONLY
STAGES = ("cost", "paths", "wta", "median", "total", "wls", "speckle", "horizontal", "sweep", "sweep_wta", "h2d",
          "d2h", "fallback", "call")


class SmParams(ctypes.Structure):
    """Mirror of ``struct sm_params`` (field order must match the header)."""
    _fields_ = [(n, ctypes.c_int) for n in (
        "min_disparity", "num_disparities", "block_size", "P1", "P2",
        "disp12_max_diff", "uniqueness_ratio", "pre_filter_cap",
        "speckle_window_size", "speckle_range", "cost_kind", "mode")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SmWlsParams(ctypes.Structure):
    """Mirror of ``struct sm_wls_params``."""
    _fields_ = [("lambda_", ctypes.c_double), ("sigma_color", ctypes.c_double)] + [
        (n, ctypes.c_int) for n in (
            "lrc_thresh", "depth_discontinuity_radius", "use_confidence", "min_disp", "left_offset",
            "right_offset", "top_offset", "bottom_offset", "num_iter")] + [
        ("lambda_attenuation", ctypes.c_float), ("roll_off", ctypes.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SmBmParams(ctypes.Structure):
    """Mirror of ``struct sm_bm_params``."""
    _fields_ = [(n, ctypes.c_int) for n in (
        "min_disparity", "num_disparities", "block_size", "pre_filter_type", "pre_filter_size",
        "pre_filter_cap", "texture_threshold", "uniqueness_ratio", "speckle_window_size", "speckle_range",
        "disp12_max_diff")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SmRectifyCam(ctypes.Structure):
    """Mirror of ``struct sm_rectify_cam``: K and iR row-major 3x3, dist = (k1, k2, p1, p2, k3)."""
    _fields_ = [("K", ctypes.c_double * 9), ("dist", ctypes.c_double * 5), ("iR", ctypes.c_double * 9)]


class SmCloudParams(ctypes.Structure):
    """Mirror of ``struct sm_cloud_params`` (point-cloud mask and options)."""
    _fields_ = [("lo", ctypes.c_double), ("hi", ctypes.c_double), ("lo_mode", ctypes.c_int),
                ("has_hi", ctypes.c_int), ("zero_nonfinite", ctypes.c_int), ("handle_missing", ctypes.c_int)]


SM_CLOUD_LO_NONE, SM_CLOUD_LO_VALUE, SM_CLOUD_LO_MIN = 0, 1, 2


class SmPngParams(ctypes.Structure):
    """Mirror of ``struct sm_png_params`` (PNG source kind, filter and disparity conversion)."""
    _fields_ = [(n, ctypes.c_int) for n in (
        "src_kind", "channels", "keep_channel_order", "filter", "disp_mode", "has_bounds", "lo", "hi")]


class SmPngDecParams(ctypes.Structure):
    """Mirror of ``struct sm_pngdec_params`` (PNG input: output kind, imread flags, disparity
    conversion, the files' geometry and limits)."""
    _fields_ = [("out_kind", ctypes.c_int), ("flags", ctypes.c_int), ("keep_channel_order", ctypes.c_int),
                ("disp_mode", ctypes.c_int), ("invalid_i16", ctypes.c_int), ("invalid_f32", ctypes.c_float),
                ("file_channels", ctypes.c_int), ("file_depth", ctypes.c_int), ("max_chunks", ctypes.c_int),
                ("max_file_bytes", ctypes.c_uint64)]


class SmJpegDecParams(ctypes.Structure):
    """Mirror of ``struct sm_jpegdec_params`` (JPEG input: imread flags, the files' geometry, the
    batch's file-size bound and device descriptors)."""
    _fields_ = [("flags", ctypes.c_int), ("keep_channel_order", ctypes.c_int), ("file_channels", ctypes.c_int),
                ("subsampling", ctypes.c_int), ("max_file_bytes", ctypes.c_uint64), ("d_desc", ctypes.c_void_p)]


class SmMcsgmParams(ctypes.Structure):
    """Mirror of ``struct sm_mcsgm_params`` (MC-CNN's stereo method: SGM penalties, bilateral filter)."""
    _fields_ = [(n, ctypes.c_float) for n in ("pi1", "pi2", "sgm_q1", "sgm_q2", "sgm_v", "sgm_d")] + [
        ("sgm_i", ctypes.c_int), ("blur_sigma", ctypes.c_float), ("blur_t", ctypes.c_float)]


class SmMcsgmStages(ctypes.Structure):
    """Mirror of ``struct sm_mcsgm_stages``: where the maps between the steps go (0: not wanted)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("wta_left", "wta_right", "status", "filled", "subpixel", "median")]


class SmMccbcaParams(ctypes.Structure):
    """Mirror of ``struct sm_mccbca_params`` (cross-based cost aggregation: arm length and threshold,
    iterations before and after the semi-global matching)."""
    _fields_ = [("l1", ctypes.c_int), ("tau1", ctypes.c_float), ("i1", ctypes.c_int), ("i2", ctypes.c_int)]


MCSGM_STAGES = tuple(n for n, _ in SmMcsgmStages._fields_)
MCSGM_INT_STAGES = MCSGM_STAGES[:4]  # int32 maps; the other two are float32

SM_PNG_SEG = 32768
SM_PNGDEC_CAP = 32768
SM_PNGDEC_U8, SM_PNGDEC_U16, SM_PNGDEC_DISP_I16, SM_PNGDEC_DISP_F32 = 0, 1, 2, 3
SM_PNG_SRC_U8, SM_PNG_SRC_U16, SM_PNG_SRC_DISP_I16, SM_PNG_SRC_DISP_F32 = 0, 1, 2, 3
SM_PNG_DISP_KITTI, SM_PNG_DISP_LINEAR_U8 = 0, 1
PLY_MAX_ROW = 157  # bytes of the longest row '%f %f %f %d %d %d ' + newline

ABI_VERSION = 3  # include/stereo_match_amd.h SM_ABI_VERSION this binding is written against

_c = ctypes
_SIGS = {
    "sm_version": (_c.c_char_p, []),
    "sm_abi_version": (_c.c_int, []),
    "sm_create": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_void_p)]),
    "sm_destroy": (None, [_c.c_void_p]),
    "sm_set_stream": (_c.c_int, [_c.c_void_p, _c.c_void_p]),
    "sm_reset_stream": (_c.c_int, [_c.c_void_p]),
    "sm_compute": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                              _c.POINTER(SmParams), _c.c_void_p, _c.c_void_p]),
    "sm_compute_wta_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t,
                                               _c.c_int, _c.c_int, _c.c_int, _c.POINTER(SmParams), _c.c_void_p,
                                               _c.c_void_p]),
    "sm_compute_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                     _c.POINTER(SmParams), _c.c_void_p]),
    "sm_compute_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t,
                                           _c.c_int, _c.c_int, _c.c_int, _c.POINTER(SmParams), _c.c_void_p]),
    "sm_compute_cn": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                 _c.POINTER(SmParams), _c.c_void_p]),
    "sm_compute_batch_device_cn": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t,
                                              _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(SmParams),
                                              _c.c_void_p]),
    "sm_aggregate_cost_f32": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                         _c.POINTER(SmParams), _c.c_float, _c.c_float, _c.c_void_p]),
    "sm_aggregate_cost_f32_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int,
                                                _c.c_int, _c.c_int, _c.POINTER(SmParams), _c.c_float,
                                                _c.c_float, _c.c_void_p]),
    "sm_wls_default_params": (_c.c_int, [_c.POINTER(SmParams), _c.POINTER(SmWlsParams)]),
    "sm_wls_filter": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                 _c.POINTER(SmWlsParams), _c.c_void_p]),
    "sm_wls_filter_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int,
                                              _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(SmWlsParams),
                                              _c.c_void_p]),
    "sm_compute_disparity": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                        _c.POINTER(SmParams), _c.POINTER(SmWlsParams), _c.c_void_p, _c.c_void_p]),
    "sm_compute_disparity_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t,
                                                     _c.c_int, _c.c_int, _c.c_int, _c.POINTER(SmParams),
                                                     _c.POINTER(SmWlsParams), _c.c_void_p, _c.c_void_p,
                                                     _c.c_void_p]),
    "sm_filter_speckles": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "sm_filter_speckles_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                             _c.c_int, _c.c_int]),
    "sm_reproject_image_to_3d": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                            _c.c_void_p, _c.c_int, _c.c_void_p]),
    "sm_reproject_image_to_3d_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                                   _c.c_void_p, _c.c_int, _c.c_void_p]),
    "sm_rectify_map": (_c.c_int, [_c.c_void_p, _c.POINTER(SmRectifyCam), _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "sm_rectify_map_device": (_c.c_int, [_c.c_void_p, _c.POINTER(SmRectifyCam), _c.c_int, _c.c_int, _c.c_void_p,
                                         _c.c_void_p]),
    "sm_remap_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                               _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "sm_remap_u8_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                            _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                            _c.c_void_p, _c.c_void_p]),
    "sm_bgr2gray_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_bgr2gray_u8_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                               _c.c_int, _c.c_void_p]),
    "sm_nlm_denoise_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_int,
                                     _c.c_int, _c.c_void_p]),
    "sm_nlm_denoise_u8_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                                  _c.c_int, _c.c_float, _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_nlm_weight_table": (_c.c_int, [_c.c_float, _c.c_int, _c.c_int, _c.c_void_p, _c.POINTER(_c.c_int),
                                       _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "sm_gauss2d_f64": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int,
                                  _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "sm_gauss2d_f64_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                               _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p,
                                               _c.c_size_t, _c.c_int]),
    "sm_image_measure_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int,
                                       _c.c_void_p, _c.c_int, _c.c_double, _c.c_void_p]),
    "sm_image_measure_u8_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                                    _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int,
                                                    _c.c_double, _c.c_void_p]),
    "sm_pyr_down_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_pyr_down_u8_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                               _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_int]),
    "sm_cloud_extract_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_int,
                                                 _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                                 _c.POINTER(SmCloudParams), _c.c_size_t, _c.c_void_p, _c.c_void_p,
                                                 _c.c_void_p]),
    "sm_cloud_extract": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                    _c.c_void_p, _c.POINTER(SmCloudParams), _c.c_size_t, _c.c_void_p, _c.c_void_p,
                                    _c.POINTER(_c.c_int64)]),
    "sm_ply_format_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_size_t, _c.c_void_p,
                                        _c.c_void_p]),
    "sm_ply_format_host": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_size_t, _c.c_void_p,
                                      _c.POINTER(_c.c_uint64)]),
    "sm_cloud_ply_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_int,
                                             _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.POINTER(SmCloudParams),
                                             _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "sm_cloud_ply": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                _c.c_void_p, _c.POINTER(SmCloudParams), _c.c_size_t, _c.c_void_p,
                                _c.POINTER(_c.c_int64), _c.POINTER(_c.c_uint64)]),
    "sm_png_bound": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "sm_png_encode_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_size_t, _c.c_int, _c.c_int,
                                              _c.c_int, _c.POINTER(SmPngParams), _c.c_size_t, _c.c_void_p,
                                              _c.c_void_p]),
    "sm_png_encode": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.POINTER(SmPngParams),
                                 _c.c_size_t, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    "sm_png_encode_host": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.POINTER(SmPngParams),
                                      _c.c_size_t, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    "sm_png_info": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                               _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "sm_png_decode_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                              _c.c_int, _c.POINTER(SmPngDecParams), _c.c_void_p, _c.c_size_t,
                                              _c.c_size_t, _c.c_void_p]),
    "sm_png_decode": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.POINTER(SmPngDecParams), _c.c_void_p,
                                 _c.c_size_t, _c.POINTER(_c.c_int)]),
    "sm_png_decode_host": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(SmPngDecParams), _c.c_void_p, _c.c_size_t,
                                      _c.POINTER(_c.c_int)]),
    "sm_png_decode_stats": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "sm_pngdec_status_message": (_c.c_char_p, [_c.c_int]),
    "sm_pngdec_status_code": (_c.c_int, [_c.c_int]),
    "sm_jpeg_info": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                                _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "sm_jpeg_desc_bytes": (_c.c_size_t, []),
    "sm_jpeg_parse": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.POINTER(_c.c_int)]),
    "sm_jpeg_decode_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                               _c.c_int, _c.POINTER(SmJpegDecParams), _c.c_void_p, _c.c_size_t,
                                               _c.c_size_t, _c.c_void_p]),
    "sm_jpeg_decode": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.POINTER(SmJpegDecParams), _c.c_void_p,
                                  _c.c_size_t, _c.POINTER(_c.c_int)]),
    "sm_jpeg_decode_host": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(SmJpegDecParams), _c.c_void_p, _c.c_size_t,
                                       _c.POINTER(_c.c_int)]),
    "sm_jpeg_decode_stats": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "sm_jpegdec_status_message": (_c.c_char_p, [_c.c_int]),
    "sm_jpegdec_status_code": (_c.c_int, [_c.c_int]),
    "sm_mccnn_set_weights": (_c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p)]),
    "sm_mccnn_features_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                            _c.c_size_t, _c.c_void_p]),
    "sm_mccnn_join_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int, _c.c_void_p]),
    "sm_mccnn_volume_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int,
                                          _c.c_int, _c.c_size_t, _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_mccnn_features": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_mccnn_join": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                 _c.c_int, _c.c_void_p]),
    "sm_mccnn_volume": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                   _c.c_int, _c.c_void_p]),
    "sm_mccnn_features_host": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p), _c.c_void_p,
                                          _c.c_int, _c.c_size_t, _c.c_int, _c.c_int, _c.c_size_t, _c.c_void_p]),
    "sm_mccnn_join_host": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                      _c.c_void_p]),
    "sm_mcacc_set_weights": (_c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p), _c.c_int,
                                        _c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p)]),
    "sm_mcacc_features_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                            _c.c_size_t, _c.c_void_p]),
    "sm_mcacc_join_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_mcacc_volume_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int,
                                          _c.c_int, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_mcacc_features": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_mcacc_join": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                 _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_mcacc_volume": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                   _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_mcacc_features_host": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p), _c.c_void_p,
                                          _c.c_int, _c.c_size_t, _c.c_int, _c.c_int, _c.c_size_t, _c.c_void_p]),
    "sm_mcacc_join_host": (_c.c_int, [_c.c_int, _c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p), _c.c_void_p,
                                      _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                      _c.c_void_p]),
    "sm_mcacc_sigmoid_host": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "sm_mcacc_set_precision": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "sm_mcacc_join_host_bf16": (_c.c_int, [_c.c_int, _c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p),
                                           _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _c.c_int, _c.c_void_p]),
    "sm_mcacc_bf16_host": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "sm_mcsgm_default_params": (_c.c_int, [_c.POINTER(SmMcsgmParams)]),
    "sm_mcsgm_aggregate_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t,
                                             _c.c_int, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                             _c.POINTER(SmMcsgmParams), _c.c_void_p]),
    "sm_mcsgm_disparity_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t,
                                             _c.c_int, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                             _c.POINTER(SmMcsgmParams), _c.c_void_p, _c.POINTER(SmMcsgmStages)]),
    "sm_mcsgm_aggregate": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                      _c.c_int, _c.c_int, _c.POINTER(SmMcsgmParams), _c.c_void_p]),
    "sm_mcsgm_disparity": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                      _c.c_int, _c.c_int, _c.POINTER(SmMcsgmParams), _c.c_void_p,
                                      _c.POINTER(SmMcsgmStages)]),
    "sm_mcsgm_aggregate_host": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int,
                                           _c.c_int, _c.c_size_t, _c.c_int, _c.c_int, _c.POINTER(SmMcsgmParams),
                                           _c.c_void_p]),
    "sm_mcsgm_disparity_host": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int,
                                           _c.c_int, _c.c_size_t, _c.c_int, _c.c_int, _c.POINTER(SmMcsgmParams),
                                           _c.c_void_p, _c.POINTER(SmMcsgmStages)]),
    "sm_mccbca_default_params": (_c.c_int, [_c.POINTER(SmMccbcaParams)]),
    "sm_mccbca_arms_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int, _c.c_size_t,
                                         _c.POINTER(SmMccbcaParams), _c.c_void_p]),
    "sm_mccbca_aggregate_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t,
                                              _c.c_int, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int,
                                              _c.POINTER(SmMccbcaParams), _c.c_int, _c.c_void_p]),
    "sm_mccbca_arms": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(SmMccbcaParams),
                                  _c.c_void_p]),
    "sm_mccbca_aggregate": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_int, _c.c_int, _c.POINTER(SmMccbcaParams), _c.c_int, _c.c_void_p]),
    "sm_mccbca_arms_host": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int, _c.c_int, _c.c_size_t,
                                       _c.POINTER(SmMccbcaParams), _c.c_void_p]),
    "sm_mccbca_aggregate_host": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int,
                                            _c.c_int, _c.c_size_t, _c.c_int, _c.c_int, _c.POINTER(SmMccbcaParams),
                                            _c.c_int, _c.c_void_p]),
    "sm_bm_default_params": (_c.c_int, [_c.c_int, _c.c_int, _c.POINTER(SmBmParams)]),
    "sm_bm_right_matcher_params": (_c.c_int, [_c.POINTER(SmBmParams), _c.POINTER(SmBmParams)]),
    "sm_bm_compute": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                 _c.POINTER(SmBmParams), _c.c_void_p]),
    "sm_bm_compute_batch_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t,
                                              _c.c_int, _c.c_int, _c.c_int, _c.POINTER(SmBmParams), _c.c_void_p]),
    "sm_compute_batch": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.POINTER(_c.c_void_p),
                                    _c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int, _c.POINTER(SmParams),
                                    _c.c_void_p]),
    "sm_right_matcher_params": (_c.c_int, [_c.POINTER(SmParams), _c.POINTER(SmParams)]),
    "sm_synchronize": (_c.c_int, [_c.c_void_p]),
    "sm_get_counters": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_longlong)]),
    "sm_get_counter": (_c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(_c.c_longlong)]),
    "sm_set_cu_mask": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint32), _c.c_int]),
    "sm_set_timing": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "sm_get_timing": (_c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_longlong),
                                 _c.POINTER(_c.c_longlong)]),
    "sm_reset_timing": (_c.c_int, [_c.c_void_p]),
    "sm_set_debug_flags": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "sm_set_tuning": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int]),
    "sm_debug_fetch": (_c.c_longlong, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t]),
    "sm_last_error": (_c.c_char_p, [_c.c_void_p]),
}

_lib = None
_lock = threading.Lock()


def wls_default_params(left: SmParams) -> SmWlsParams:
    """sm_wls_default_params: the filter createDisparityWLSFilter(left) builds."""
    out = SmWlsParams()
    rc = load().sm_wls_default_params(ctypes.byref(left), ctypes.byref(out))
    if rc != SM_OK:
        _raise(rc, None)
    return out


def ply_format_host(verts: np.ndarray, colors: np.ndarray, capacity: int = None) -> np.ndarray:
    """sm_ply_format_host: the PLY body of float32 verts [N, 3] and uint8 colors [N, 3] as a uint8
    array, formatted on the CPU by the row function the GPU kernels use.  Needs no context and no
    device.  ``capacity`` (default: the exact size, asked for first) bounds the output buffer; a
    body that does not fit is a ValueError and nothing is written."""
    lib = load()
    v = np.ascontiguousarray(verts)
    c = np.ascontiguousarray(colors)
    if v.dtype != np.float32 or c.dtype != np.uint8 or v.ndim != 2 or v.shape[1] != 3 or c.shape != v.shape:
        raise ValueError("ply_format_host: float32 verts [N, 3] and uint8 colors [N, 3]")
    n = v.shape[0]
    nb = ctypes.c_uint64()
    if capacity is None:
        rc = lib.sm_ply_format_host(v.ctypes.data, c.ctypes.data, n, 0, None, ctypes.byref(nb))
        if nb.value == 0:
            if rc != SM_OK:
                _raise(rc, None)
            return np.empty(0, np.uint8)
        capacity = nb.value
    out = np.empty(int(capacity), np.uint8)
    rc = lib.sm_ply_format_host(v.ctypes.data, c.ctypes.data, n, out.size, out.ctypes.data if out.size else None,
                                ctypes.byref(nb))
    if rc != SM_OK:
        _raise(rc, None)
    return out[:nb.value]


def png_file_geometry(prm: "SmPngParams"):
    """(channels, depth) of the file an image with these parameters makes."""
    if prm.src_kind == SM_PNG_SRC_U8:
        return prm.channels, 8
    if prm.src_kind == SM_PNG_SRC_U16:
        return 1, 16
    return 1, (8 if prm.disp_mode == SM_PNG_DISP_LINEAR_U8 else 16)


def png_encode_host(img: np.ndarray, prm: "SmPngParams", capacity: int = None) -> np.ndarray:
    """sm_png_encode_host: the PNG file of a 2-D (or [H, W, 3]) array as a uint8 array, encoded on
    the CPU by the functions the GPU kernels run.  Needs no context and no device.  ``capacity``
    (default: sm_png_bound) bounds the output buffer; a file that does not fit is a ValueError."""
    lib = load()
    H, W = img.shape[:2]
    if capacity is None:
        capacity = lib.sm_png_bound(H, W, *png_file_geometry(prm))
    out = np.empty(int(capacity), np.uint8)
    nb = ctypes.c_uint64()
    rc = lib.sm_png_encode_host(img.ctypes.data, img.strides[0] if img.size else 0, H, W, ctypes.byref(prm), out.size,
                                out.ctypes.data if out.size else None, ctypes.byref(nb))
    if rc != SM_OK:
        _raise(rc, None)
    return out[:nb.value]


def png_info(buf):
    """sm_png_info: (H, W, channels, depth) of a PNG file held in a bytes-like object.  Host only."""
    b = np.frombuffer(buf, np.uint8)
    v = [ctypes.c_int() for _ in range(4)]
    rc = load().sm_png_info(b.ctypes.data if b.size else np.zeros(1, np.uint8).ctypes.data, b.size, *[ctypes.byref(x) for x in v])
    if rc != SM_OK:
        _raise(rc, None)
    return tuple(x.value for x in v)


def png_decode_stats(ctx=None):
    """sm_png_decode_stats: (parallel, serial) images of the last decode call of this context, or
    (ctx None) of this thread's last sm_png_decode_host."""
    a, b = ctypes.c_int(), ctypes.c_int()
    rc = load().sm_png_decode_stats(ctx, ctypes.byref(a), ctypes.byref(b))
    if rc != SM_OK:
        _raise(rc, ctx)
    return a.value, b.value


def png_decode_host(buf, prm: "SmPngDecParams", out: np.ndarray):
    """sm_png_decode_host into ``out`` (rows ``out.strides[0]`` apart), decoded on the CPU by the
    functions the GPU kernels run.  Needs no context and no device."""
    b = np.frombuffer(buf, np.uint8)
    rc = load().sm_png_decode_host(b.ctypes.data, b.size, ctypes.byref(prm), out.ctypes.data, out.strides[0], None)
    if rc != SM_OK:
        _raise(rc, None)
    return out


def _file_ptr(b: np.ndarray) -> int:
    return b.ctypes.data if b.size else np.zeros(1, np.uint8).ctypes.data


def jpeg_info(buf):
    """sm_jpeg_info: (H, W, channels, subsampling) of a JPEG file held in a bytes-like object;
    subsampling 0 (gray), 444, 422 or 420.  Host only."""
    b = np.frombuffer(buf, np.uint8)
    v = [ctypes.c_int() for _ in range(4)]
    rc = load().sm_jpeg_info(_file_ptr(b), b.size, *[ctypes.byref(x) for x in v])
    if rc != SM_OK:
        _raise(rc, None)
    return tuple(x.value for x in v)


def jpeg_parse(buf) -> np.ndarray:
    """sm_jpeg_parse: the descriptor the device decodes a file from, as a uint8 array.  Host only."""
    lib = load()
    b = np.frombuffer(buf, np.uint8)
    desc = np.zeros(lib.sm_jpeg_desc_bytes(), np.uint8)
    rc = lib.sm_jpeg_parse(_file_ptr(b), b.size, desc.ctypes.data, None)
    if rc != SM_OK:
        _raise(rc, None)
    return desc


def jpeg_desc_info(desc: np.ndarray):
    """(H, W, channels, subsampling) from a descriptor of :func:`jpeg_parse` (the leading words of
    csrc/sm_jpegdec.hpp's JdDesc: status, W, H, components, luma factors h and v)."""
    _, W, H, nc, hs, vs = (int(x) for x in desc[:24].view(np.int32))
    return H, W, nc, (0 if nc == 1 else 444 if hs == 1 else 422 if vs == 1 else 420)


def jpeg_decode_stats(ctx=None):
    """sm_jpeg_decode_stats: (sub-sequences, synchronisation rounds) of the last decode call of this
    context, or (ctx None) of this thread's last sm_jpeg_decode_host."""
    a, b = ctypes.c_int(), ctypes.c_int()
    rc = load().sm_jpeg_decode_stats(ctx, ctypes.byref(a), ctypes.byref(b))
    if rc != SM_OK:
        _raise(rc, ctx)
    return a.value, b.value


def jpeg_decode_host(buf, prm: "SmJpegDecParams", out: np.ndarray):
    """sm_jpeg_decode_host into ``out`` (rows ``out.strides[0]`` apart): the plain serial decoder on
    the CPU, built from the functions the GPU kernels run.  Needs no context and no device."""
    b = np.frombuffer(buf, np.uint8)
    rc = load().sm_jpeg_decode_host(_file_ptr(b), b.size, ctypes.byref(prm), out.ctypes.data, out.strides[0], None)
    if rc != SM_OK:
        _raise(rc, None)
    return out


def _ptr_array(arrays):
    """A C array of the arrays' data pointers (float32, contiguous; the caller keeps them alive)."""
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def mccnn_features_host(weights, biases, gray: np.ndarray, image_stride: int, row_stride: int, n: int, H: int, W: int):
    """sm_mccnn_features_host: the CPU twin's feature maps [n, H, W, 64] of n gray images inside
    ``gray`` (a uint8 array; images / rows ``image_stride`` / ``row_stride`` bytes apart)."""
    feat = np.empty((n, H, W, 64), np.float32)
    rc = load().sm_mccnn_features_host(len(weights), _ptr_array(weights), _ptr_array(biases), gray.ctypes.data, n,
                                       image_stride, H, W, row_stride, feat.ctypes.data)
    if rc != SM_OK:
        _raise(rc, None)
    return feat


def mccnn_join_host(fa: np.ndarray, fb: np.ndarray, D: int, min_disparity: int) -> np.ndarray:
    """sm_mccnn_join_host: the CPU twin's volume [n, D, H, W] of feature maps [n, H, W, 64]."""
    n, H, W = fa.shape[:3]
    vol = np.empty((n, D, H, W), np.float32)
    rc = load().sm_mccnn_join_host(fa.ctypes.data, fb.ctypes.data, n, H, W, D, min_disparity, vol.ctypes.data)
    if rc != SM_OK:
        _raise(rc, None)
    return vol


def mcacc_features_host(weights, biases, gray: np.ndarray, image_stride: int, row_stride: int, n: int, H: int, W: int):
    """sm_mcacc_features_host: the CPU twin's feature maps [n, H, W, 112] of n gray images inside
    ``gray`` (a uint8 array; images / rows ``image_stride`` / ``row_stride`` bytes apart)."""
    feat = np.empty((n, H, W, 112), np.float32)
    rc = load().sm_mcacc_features_host(len(weights), _ptr_array(weights), _ptr_array(biases), gray.ctypes.data, n,
                                       image_stride, H, W, row_stride, feat.ctypes.data)
    if rc != SM_OK:
        _raise(rc, None)
    return feat


SM_MCACC_F32, SM_MCACC_BF16 = 0, 1
MCACC_PRECISIONS = {"f32": SM_MCACC_F32, "bf16": SM_MCACC_BF16}


def mcacc_join_host(fc_w, fc_b, fa: np.ndarray, fb: np.ndarray, D: int, min_disparity: int, a_is_left: bool,
                    raw: bool, precision: str = "f32") -> np.ndarray:
    """sm_mcacc_join_host (``precision="bf16"``: sm_mcacc_join_host_bf16): the CPU twin's volume
    [n, D, H, W] of feature maps [n, H, W, 112]."""
    n, H, W = fa.shape[:3]
    vol = np.empty((n, D, H, W), np.float32)
    fn = load().sm_mcacc_join_host_bf16 if MCACC_PRECISIONS[precision] == SM_MCACC_BF16 else load().sm_mcacc_join_host
    rc = fn(len(fc_w) - 1, fc_w[0].shape[0], _ptr_array(fc_w), _ptr_array(fc_b), fa.ctypes.data, fb.ctypes.data, n, H, W,
            D, min_disparity, int(bool(a_is_left)), int(bool(raw)), vol.ctypes.data)
    if rc != SM_OK:
        _raise(rc, None)
    return vol


def mcacc_bf16_host(x: np.ndarray) -> np.ndarray:
    """sm_mcacc_bf16_host: the bfloat16 bit patterns (uint16) of a float32 array, the rounding of
    ``precision="bf16"``."""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape, np.uint16)
    rc = load().sm_mcacc_bf16_host(x.ctypes.data, x.size, out.ctypes.data)
    if rc != SM_OK:
        _raise(rc, None)
    return out


def mcacc_sigmoid_host(z: np.ndarray) -> np.ndarray:
    """sm_mcacc_sigmoid_host: the scorer's sigmoid of a contiguous float32 array."""
    z = np.ascontiguousarray(z, np.float32)
    s = np.empty_like(z)
    rc = load().sm_mcacc_sigmoid_host(z.ctypes.data, z.size, s.ctypes.data)
    if rc != SM_OK:
        _raise(rc, None)
    return s


def mcsgm_stage_arrays(n: int, H: int, W: int):
    """Empty numpy maps for every member of ``sm_mcsgm_stages`` and the struct that points at them."""
    maps = {k: np.empty((n, H, W), np.int32 if k in MCSGM_INT_STAGES else np.float32) for k in MCSGM_STAGES}
    return maps, SmMcsgmStages(*[maps[k].ctypes.data for k in MCSGM_STAGES])


def mcsgm_aggregate_host(vol: np.ndarray, a: np.ndarray, b: np.ndarray, image_stride: int, row_stride: int,
                         min_disparity: int, prm: "SmMcsgmParams") -> np.ndarray:
    """sm_mcsgm_aggregate_host: the CPU twin's aggregated volume of ``vol`` [n, D, H, W] (float32,
    contiguous) and the n images inside ``a`` / ``b`` (uint8; one geometry for both)."""
    n, D, H, W = vol.shape
    agg = np.empty_like(vol)
    rc = load().sm_mcsgm_aggregate_host(vol.ctypes.data, a.ctypes.data, b.ctypes.data, n, image_stride, H, W, row_stride,
                                        D, min_disparity, ctypes.byref(prm), agg.ctypes.data)
    if rc != SM_OK:
        _raise(rc, None)
    return agg


def mcsgm_disparity_host(agg_l: np.ndarray, agg_r: np.ndarray, a: np.ndarray, image_stride: int, row_stride: int,
                         min_disparity: int, prm: "SmMcsgmParams", stages: bool):
    """sm_mcsgm_disparity_host: (disparity [n, H, W] float32, dict of the stage maps or None)."""
    n, D, H, W = agg_l.shape
    disp = np.empty((n, H, W), np.float32)
    maps, st = mcsgm_stage_arrays(n, H, W) if stages else (None, None)
    rc = load().sm_mcsgm_disparity_host(agg_l.ctypes.data, agg_r.ctypes.data, a.ctypes.data, n, image_stride, H, W,
                                        row_stride, D, min_disparity, ctypes.byref(prm), disp.ctypes.data,
                                        ctypes.byref(st) if stages else None)
    if rc != SM_OK:
        _raise(rc, None)
    return disp, maps


def mccbca_arms_host(img: np.ndarray, image_stride: int, row_stride: int, prm: "SmMccbcaParams") -> np.ndarray:
    """sm_mccbca_arms_host: uint8 [n, 4, H, W] (left, right, up, down) of the n images inside ``img``
    (uint8 [n, H, W] of any row and image stride)."""
    n, H, W = img.shape
    arms = np.empty((n, 4, H, W), np.uint8)
    rc = load().sm_mccbca_arms_host(img.ctypes.data, n, image_stride, H, W, row_stride, ctypes.byref(prm), arms.ctypes.data)
    if rc != SM_OK:
        _raise(rc, None)
    return arms


def mccbca_aggregate_host(vol: np.ndarray, a: np.ndarray, b: np.ndarray, image_stride: int, row_stride: int,
                          min_disparity: int, prm: "SmMccbcaParams", iterations: int) -> np.ndarray:
    """sm_mccbca_aggregate_host: the CPU twin's cross-based aggregation of ``vol`` [n, D, H, W] (float32,
    contiguous) and the n images inside ``a`` / ``b`` (uint8; one geometry for both)."""
    n, D, H, W = vol.shape
    agg = np.empty_like(vol)
    rc = load().sm_mccbca_aggregate_host(vol.ctypes.data, a.ctypes.data, b.ctypes.data, n, image_stride, H, W, row_stride,
                                         D, min_disparity, ctypes.byref(prm), iterations, agg.ctypes.data)
    if rc != SM_OK:
        _raise(rc, None)
    return agg


def volume_scale(scale) -> float:
    """The C-ABI's scale argument for an external cost volume: "auto" -> 0.0 (the window derived
    per pair on the device), else the explicit float (NaN is refused: it would quantise every
    cell to NaN; the C-ABI itself treats NaN like 0)."""
    if isinstance(scale, str):
        if scale != "auto":
            raise ValueError(f"scale must be a number or 'auto', not {scale!r}")
        return 0.0
    if scale is None:
        raise ValueError("scale=None is ambiguous: pass 'auto' for the per-pair window or a number")
    s = float(scale)
    if s != s:
        raise ValueError("scale is NaN: pass 'auto' for the per-pair window")
    return s


def header_symbols(path: str = HEADER_PATH):
    """Function names declared in include/stereo_match_amd.h."""
    with open(path) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w\s\*]*?\b(sm_\w+)\s*\(", text, flags=re.M)))


def _init_torch_hip_first():
    """torch wheels bundle their own libamdhip64; our library links ROCm's.
    Both runtimes can live in one process, but on the MI355X boxes torch's
    reports "No HIP GPUs are available" if ROCm's was initialised first.  So
    when torch is installed, bring its runtime up before ours (device
    enumeration only; no context is created on any device)."""
    try:
        import torch
    except Exception:  # torch absent: nothing to order
        return
    try:
        if getattr(torch.version, "hip", None):
            torch.cuda.is_available()
    except Exception:
        pass


def load():
    """Load the HIP library (fails loudly if it has not been built)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C stereo_match_amd/csrc` "
                "(or python -c 'import __graft_entry__ as g; g.build()'). "
                "There is no CPU fallback.")
        _init_torch_hip_first()
        lib = ctypes.CDLL(LIB_PATH)
        # the version check comes before any other symbol is bound: a library built for an
        # older ABI may lack symbols this binding declares (AttributeError otherwise)
        if not hasattr(lib, "sm_abi_version"):
            raise ImportError(f"{LIB_PATH} predates the versioned C-ABI (no sm_abi_version), this binding needs "
                              f"version {ABI_VERSION}: rebuild it with `make -C stereo_match_amd/csrc`")
        lib.sm_abi_version.restype = ctypes.c_int
        lib.sm_abi_version.argtypes = []
        abi = lib.sm_abi_version()
        if abi != ABI_VERSION:
            raise ImportError(f"{LIB_PATH} has C-ABI version {abi}, this binding needs {ABI_VERSION}: rebuild it "
                              "with `make -C stereo_match_amd/csrc`")
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name, None)
            if fn is None:
                raise ImportError(f"{LIB_PATH} (C-ABI {abi}) does not export {name}: rebuild it with "
                                  "`make -C stereo_match_amd/csrc`")
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


class SmError(RuntimeError):
    """Raised for SM_E_HIP / SM_E_UNSUPPORTED (OpenCV would raise cv2.error)."""

    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


def _raise(code: int, ctx):
    lib = load()
    msg = (lib.sm_last_error(ctx) or b"").decode(errors="replace")
    if code == SM_E_ARG:
        raise ValueError(msg)
    raise SmError(code, msg)


class Engine:
    """One sm_ctx bound to one HIP device (not thread-safe; one per thread)."""

    def __init__(self, device: int = 0):
        lib = load()
        h = ctypes.c_void_p()
        rc = lib.sm_create(int(device), ctypes.byref(h))
        if rc != SM_OK:
            _raise(rc, None)
        self._lib = lib
        self.ctx = h
        self.device = device

    def close(self):
        if getattr(self, "ctx", None):
            self._lib.sm_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != SM_OK:
            _raise(rc, self.ctx)

    def set_stream(self, stream_handle):
        """Enqueue on this hipStream_t handle (0 = the null stream, e.g. torch's
        default stream); None = back to the context's own stream."""
        if stream_handle is None:
            self._check(self._lib.sm_reset_stream(self.ctx))
        else:
            self._check(self._lib.sm_set_stream(self.ctx, ctypes.c_void_p(int(stream_handle))))

    # -- host arrays -------------------------------------------------------
    def compute(self, left: np.ndarray, right: np.ndarray, params: SmParams) -> np.ndarray:
        """uint8 [H, W] gray or [H, W, 3] BGR pairs -> int16 [H, W] disparity x16."""
        left = np.ascontiguousarray(left)
        right = np.ascontiguousarray(right)
        H, W = left.shape[:2]
        cn = 1 if left.ndim == 2 else left.shape[2]
        out = np.empty((H, W), np.int16)
        self._check(self._lib.sm_compute_cn(self.ctx, left.ctypes.data, right.ctypes.data, H, W, W * cn, cn,
                                            ctypes.byref(params), out.ctypes.data))
        return out

    def compute_wta(self, left: np.ndarray, right: np.ndarray, params: SmParams):
        """Gray pair -> (int16 [H, W] disparity x16, int16 [H, W] integer WTA index): the
        index is OpenCV's bestDisp in [0, D) where the uniqueness test passes, -1 elsewhere,
        before the sub-pixel step, the LR check and the median (sm_compute's wta_out)."""
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        if left.ndim != 2:
            raise ValueError("compute_wta takes gray [H, W] images")
        H, W = left.shape
        out = np.empty((H, W), np.int16)
        wta = np.empty((H, W), np.int16)
        self._check(self._lib.sm_compute(self.ctx, left.ctypes.data, right.ctypes.data, H, W, W,
                                         ctypes.byref(params), out.ctypes.data, wta.ctypes.data))
        return out, wta

    # -- device pointers (e.g. torch tensors' data_ptr()) -------------------
    def compute_wta_batch_device(self, d_left: int, d_right: int, npairs: int, pair_stride: int, H: int, W: int,
                                 stride: int, params: SmParams, d_out: int, d_wta: int):
        self._check(self._lib.sm_compute_wta_batch_device(
            self.ctx, ctypes.c_void_p(d_left), ctypes.c_void_p(d_right), npairs, pair_stride, H, W, stride,
            ctypes.byref(params), ctypes.c_void_p(d_out), ctypes.c_void_p(d_wta)))

    def compute_device(self, d_left: int, d_right: int, H: int, W: int, stride: int, params: SmParams,
                       d_out: int):
        self._check(self._lib.sm_compute_device(self.ctx, ctypes.c_void_p(d_left), ctypes.c_void_p(d_right),
                                                H, W, stride, ctypes.byref(params), ctypes.c_void_p(d_out)))

    def compute_batch_device(self, d_left: int, d_right: int, npairs: int, pair_stride: int, H: int, W: int,
                             stride: int, params: SmParams, d_out: int, channels: int = 1):
        self._check(self._lib.sm_compute_batch_device_cn(
            self.ctx, ctypes.c_void_p(d_left), ctypes.c_void_p(d_right), npairs, pair_stride, H, W, stride,
            channels, ctypes.byref(params), ctypes.c_void_p(d_out)))

    # -- external cost volume (mc-cnn) ----------------------------------------
    def aggregate_cost_f32(self, vol: np.ndarray, params: SmParams, offset: float = 0.0,
                           scale=1.0) -> np.ndarray:
        """SGM over a float32 d-major cost volume [D][H][W] (or [1][D][H][W]).  scale "auto"
        (opt-in): the quantisation window from the volume's own finite range, per pair
        (include/stereo_match_amd.h: scale 0 at the C-ABI); default: the explicit window
        offset 0, scale 1."""
        scale = volume_scale(scale)
        v = np.ascontiguousarray(vol, np.float32)
        if v.ndim == 4:
            if v.shape[0] != 1:
                raise ValueError("expected a (1, D, H, W) volume")
            v = v[0]
        if v.ndim != 3:
            raise ValueError("expected a (D, H, W) float32 volume")
        D, H, W = v.shape
        out = np.empty((H, W), np.int16)
        self._check(self._lib.sm_aggregate_cost_f32(self.ctx, v.ctypes.data, D, H, W, ctypes.byref(params),
                                                    float(offset), float(scale), out.ctypes.data))
        return out

    def aggregate_cost_f32_device(self, d_cost: int, npairs: int, pair_stride_elems: int, D: int, H: int,
                                  W: int, params: SmParams, offset: float, scale, d_out: int):
        self._check(self._lib.sm_aggregate_cost_f32_device(
            self.ctx, ctypes.c_void_p(d_cost), npairs, pair_stride_elems, D, H, W, ctypes.byref(params),
            float(offset), volume_scale(scale), ctypes.c_void_p(d_out)))

    # -- WLS post-filter --------------------------------------------------------
    def wls_filter(self, displ: np.ndarray, guide: np.ndarray, dispr, params: "SmWlsParams") -> np.ndarray:
        displ = np.ascontiguousarray(displ, np.int16)
        guide = np.ascontiguousarray(guide, np.uint8)
        H, W = displ.shape
        if guide.shape != (H, W):
            raise ValueError("guide must be a gray (uint8) image of the disparity map's size")
        ptr_r = None
        if dispr is not None:
            dispr = np.ascontiguousarray(dispr, np.int16)
            if dispr.shape != (H, W):
                raise ValueError("right disparity map must match the left one")
            ptr_r = dispr.ctypes.data
        out = np.empty((H, W), np.int16)
        self._check(self._lib.sm_wls_filter(self.ctx, displ.ctypes.data, ptr_r, guide.ctypes.data, W, H, W,
                                            ctypes.byref(params), out.ctypes.data))
        return out

    def wls_filter_batch_device(self, d_displ: int, d_dispr, d_guide: int, npairs: int, guide_pair_stride: int,
                                guide_stride: int, H: int, W: int, params: "SmWlsParams", d_out: int):
        self._check(self._lib.sm_wls_filter_batch_device(
            self.ctx, ctypes.c_void_p(d_displ), ctypes.c_void_p(d_dispr or 0) if d_dispr else None,
            ctypes.c_void_p(d_guide), npairs, guide_pair_stride, guide_stride, H, W, ctypes.byref(params),
            ctypes.c_void_p(d_out)))

    def compute_disparity(self, left: np.ndarray, right: np.ndarray, params: SmParams, wls: "SmWlsParams"):
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        H, W = left.shape
        displ = np.empty((H, W), np.int16)
        filt = np.empty((H, W), np.int16)
        self._check(self._lib.sm_compute_disparity(self.ctx, left.ctypes.data, right.ctypes.data, H, W, W,
                                                   ctypes.byref(params), ctypes.byref(wls), displ.ctypes.data,
                                                   filt.ctypes.data))
        return displ, filt

    def compute_disparity_batch_device(self, d_left: int, d_right: int, npairs: int, pair_stride: int, H: int,
                                       W: int, stride: int, params: SmParams, wls: "SmWlsParams", d_displ: int,
                                       d_dispr: int, d_filtered: int):
        self._check(self._lib.sm_compute_disparity_batch_device(
            self.ctx, ctypes.c_void_p(d_left), ctypes.c_void_p(d_right), npairs, pair_stride, H, W, stride,
            ctypes.byref(params), ctypes.byref(wls), ctypes.c_void_p(d_displ), ctypes.c_void_p(d_dispr),
            ctypes.c_void_p(d_filtered)))

    # -- speckle filter -------------------------------------------------------
    def filter_speckles(self, img: np.ndarray, new_val: int, max_speckle_size: int, max_diff: int) -> np.ndarray:
        """cv::filterSpeckles on a copy of an int16 map (returns the filtered map)."""
        out = np.array(img, dtype=np.int16, order="C", copy=True)
        if out.ndim != 2:
            raise ValueError("expected a 2-D int16 map")
        H, W = out.shape
        self._check(self._lib.sm_filter_speckles(self.ctx, out.ctypes.data, H, W, int(new_val),
                                                 int(max_speckle_size), int(max_diff)))
        return out

    def filter_speckles_device(self, d_img: int, nimg: int, H: int, W: int, new_val: int, max_speckle_size: int,
                               max_diff: int):
        self._check(self._lib.sm_filter_speckles_device(self.ctx, ctypes.c_void_p(d_img), nimg, H, W, int(new_val),
                                                        int(max_speckle_size), int(max_diff)))

    # -- 3-D reprojection ---------------------------------------------------------
    def reproject(self, disp: np.ndarray, Q: np.ndarray, handle_missing: bool = False) -> np.ndarray:
        d = np.ascontiguousarray(disp)
        kind = {np.dtype(np.int16): 0, np.dtype(np.float32): 1}.get(d.dtype)
        if kind is None or d.ndim != 2:
            raise ValueError("disparity must be a 2-D int16 or float32 array")
        Qd = np.ascontiguousarray(np.asarray(Q, np.float64).reshape(16))
        H, W = d.shape
        out = np.empty((H, W, 3), np.float32)
        self._check(self._lib.sm_reproject_image_to_3d(self.ctx, d.ctypes.data, kind, H, W, Qd.ctypes.data,
                                                       int(bool(handle_missing)), out.ctypes.data))
        return out

    def reproject_device(self, d_disp: int, kind: int, nimg: int, H: int, W: int, Q: np.ndarray,
                         handle_missing: bool, d_xyz: int):
        Qd = np.ascontiguousarray(np.asarray(Q, np.float64).reshape(16))
        self._check(self._lib.sm_reproject_image_to_3d_device(self.ctx, ctypes.c_void_p(d_disp), kind, nimg, H, W,
                                                              Qd.ctypes.data, int(bool(handle_missing)),
                                                              ctypes.c_void_p(d_xyz)))

    # -- rectification front end ------------------------------------------------------
    def rectify_map(self, cam: "SmRectifyCam", H: int, W: int):
        """initUndistortRectifyMap: float32 (mapx, mapy), each [H, W]."""
        mapx = np.empty((max(H, 0), max(W, 0)), np.float32)
        mapy = np.empty_like(mapx)
        self._check(self._lib.sm_rectify_map(self.ctx, ctypes.byref(cam), H, W, mapx.ctypes.data, mapy.ctypes.data))
        return mapx, mapy

    def rectify_map_device(self, cam: "SmRectifyCam", H: int, W: int, d_mapx: int, d_mapy: int):
        self._check(self._lib.sm_rectify_map_device(self.ctx, ctypes.byref(cam), H, W, ctypes.c_void_p(d_mapx),
                                                    ctypes.c_void_p(d_mapy)))

    def remap(self, src: np.ndarray, mapx: np.ndarray, mapy: np.ndarray, want_dst: bool = True,
              want_gray: bool = False):
        """remap(INTER_LINEAR) of a uint8 [h, w] or [h, w, 3] image (any row stride, pixels
        contiguous) through float32 maps [H, W]: (dst or None, gray or None)."""
        if src.dtype != np.uint8 or src.ndim not in (2, 3):
            raise ValueError("remap: src must be a uint8 [h, w] or [h, w, c] array")
        cn = 1 if src.ndim == 2 else src.shape[2]
        if src.size and (src.strides[1] != cn or (src.ndim == 3 and src.strides[2] != 1) or src.strides[0] < 0):
            src = np.ascontiguousarray(src)
        mapx = np.ascontiguousarray(mapx, np.float32)
        mapy = np.ascontiguousarray(mapy, np.float32)
        if mapx.ndim != 2 or mapx.shape != mapy.shape:
            raise ValueError("remap: mapx and mapy must be float32 [H, W] arrays of one shape")
        H, W = mapx.shape
        dst = np.empty((H, W) if src.ndim == 2 else (H, W, cn), np.uint8) if want_dst else None
        gray = np.empty((H, W), np.uint8) if want_gray else None
        self._check(self._lib.sm_remap_u8(
            self.ctx, src.ctypes.data, src.shape[0], src.shape[1], src.strides[0] if src.size else 0, cn,
            mapx.ctypes.data, mapy.ctypes.data, H, W, dst.ctypes.data if want_dst else None,
            gray.ctypes.data if want_gray else None))
        return dst, gray

    def remap_batch_device(self, d_src: int, nimg: int, img_stride: int, srcH: int, srcW: int, src_stride: int,
                           channels: int, d_mapx: int, d_mapy: int, H: int, W: int, d_dst, d_gray):
        self._check(self._lib.sm_remap_u8_batch_device(
            self.ctx, ctypes.c_void_p(d_src), nimg, img_stride, srcH, srcW, src_stride, channels,
            ctypes.c_void_p(d_mapx), ctypes.c_void_p(d_mapy), H, W, ctypes.c_void_p(d_dst) if d_dst else None,
            ctypes.c_void_p(d_gray) if d_gray else None))

    def bgr2gray(self, src: np.ndarray) -> np.ndarray:
        """cvtColor(COLOR_BGR2GRAY) of a uint8 [H, W, 3] image."""
        if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
            raise ValueError("bgr2gray: src must be a uint8 [H, W, 3] array")
        src = np.ascontiguousarray(src)
        H, W = src.shape[:2]
        gray = np.empty((H, W), np.uint8)
        self._check(self._lib.sm_bgr2gray_u8(self.ctx, src.ctypes.data, H, W, 3 * W, gray.ctypes.data))
        return gray

    def bgr2gray_batch_device(self, d_src: int, nimg: int, img_stride: int, H: int, W: int, src_stride: int,
                              d_gray: int):
        self._check(self._lib.sm_bgr2gray_u8_batch_device(self.ctx, ctypes.c_void_p(d_src), nimg, img_stride, H, W,
                                                          src_stride, ctypes.c_void_p(d_gray)))

    # -- point clouds ------------------------------------------------------
    def cloud_extract(self, disp: np.ndarray, kind: int, bgr: np.ndarray, Q: np.ndarray, prm: "SmCloudParams"):
        """sm_cloud_extract on a C-contiguous [H, W] map and a uint8 [H, W, 3] image whose pixels
        are contiguous (any row stride): (verts float32 [N, 3], colors uint8 [N, 3] RGB)."""
        H, W = disp.shape
        Qd = np.ascontiguousarray(np.asarray(Q, np.float64).reshape(16))
        verts = np.empty((H * W, 3), np.float32)
        colors = np.empty((H * W, 3), np.uint8)
        n = ctypes.c_int64()
        self._check(self._lib.sm_cloud_extract(self.ctx, disp.ctypes.data, kind, bgr.ctypes.data, bgr.strides[0], H, W,
                                               Qd.ctypes.data, ctypes.byref(prm), H * W, verts.ctypes.data,
                                               colors.ctypes.data, ctypes.byref(n)))
        return verts[:n.value].copy(), colors[:n.value].copy()

    def cloud_extract_batch_device(self, d_disp: int, kind: int, d_bgr: int, img_stride: int, bgr_stride: int,
                                   nimg: int, H: int, W: int, Q: np.ndarray, prm: "SmCloudParams", capacity_rows: int,
                                   d_verts: int, d_colors: int, d_counts: int):
        Qd = np.ascontiguousarray(np.asarray(Q, np.float64).reshape(16))
        self._check(self._lib.sm_cloud_extract_batch_device(
            self.ctx, ctypes.c_void_p(d_disp), kind, ctypes.c_void_p(d_bgr), img_stride, bgr_stride, nimg, H, W,
            Qd.ctypes.data, ctypes.byref(prm), capacity_rows, ctypes.c_void_p(d_verts) if d_verts else None,
            ctypes.c_void_p(d_colors) if d_colors else None, ctypes.c_void_p(d_counts) if d_counts else None))

    def ply_format_device(self, d_verts: int, d_colors: int, n: int, capacity_bytes: int, d_out: int, d_nbytes: int):
        self._check(self._lib.sm_ply_format_device(
            self.ctx, ctypes.c_void_p(d_verts) if d_verts else None, ctypes.c_void_p(d_colors) if d_colors else None, n,
            capacity_bytes, ctypes.c_void_p(d_out) if d_out else None, ctypes.c_void_p(d_nbytes) if d_nbytes else None))

    def cloud_ply_batch_device(self, d_disp: int, kind: int, d_bgr: int, img_stride: int, bgr_stride: int, nimg: int,
                               H: int, W: int, Q: np.ndarray, prm: "SmCloudParams", capacity_bytes: int, d_out: int,
                               d_counts: int, d_nbytes: int):
        Qd = np.ascontiguousarray(np.asarray(Q, np.float64).reshape(16))
        self._check(self._lib.sm_cloud_ply_batch_device(
            self.ctx, ctypes.c_void_p(d_disp), kind, ctypes.c_void_p(d_bgr), img_stride, bgr_stride, nimg, H, W,
            Qd.ctypes.data, ctypes.byref(prm), capacity_bytes, ctypes.c_void_p(d_out) if d_out else None,
            ctypes.c_void_p(d_counts) if d_counts else None, ctypes.c_void_p(d_nbytes) if d_nbytes else None))

    def cloud_ply(self, disp: np.ndarray, kind: int, bgr: np.ndarray, Q: np.ndarray, prm: "SmCloudParams"):
        """sm_cloud_ply: (PLY body as a uint8 array, N).  The buffer handed to the library is sized
        for the longest possible rows; only the pages the body reaches are ever touched."""
        H, W = disp.shape
        Qd = np.ascontiguousarray(np.asarray(Q, np.float64).reshape(16))
        out = np.empty(H * W * PLY_MAX_ROW, np.uint8)
        n, nb = ctypes.c_int64(), ctypes.c_uint64()
        self._check(self._lib.sm_cloud_ply(self.ctx, disp.ctypes.data, kind, bgr.ctypes.data, bgr.strides[0], H, W,
                                           Qd.ctypes.data, ctypes.byref(prm), out.size, out.ctypes.data,
                                           ctypes.byref(n), ctypes.byref(nb)))
        return out[:nb.value], n.value

    # -- fastNlMeansDenoising -------------------------------------------------------------
    def png_encode(self, img: np.ndarray, prm: "SmPngParams") -> np.ndarray:
        """sm_png_encode: the PNG file of a host array as a uint8 array (encoded on the device)."""
        H, W = img.shape[:2]
        out = np.empty(self._lib.sm_png_bound(H, W, *png_file_geometry(prm)), np.uint8)
        nb = ctypes.c_uint64()
        self._check(self._lib.sm_png_encode(self.ctx, img.ctypes.data, img.strides[0] if img.size else 0, H, W,
                                            ctypes.byref(prm), out.size, out.ctypes.data if out.size else None,
                                            ctypes.byref(nb)))
        return out[:nb.value]

    def png_decode(self, buf, prm: "SmPngDecParams", out: np.ndarray) -> np.ndarray:
        """sm_png_decode: one file in host memory into the host array ``out`` (decoded on the device)."""
        b = np.frombuffer(buf, np.uint8)
        self._check(self._lib.sm_png_decode(self.ctx, b.ctypes.data, b.size, ctypes.byref(prm), out.ctypes.data,
                                            out.strides[0], None))
        return out

    def png_decode_batch_device(self, d_files: int, d_offsets: int, d_sizes: int, nimg: int, H: int, W: int,
                                prm: "SmPngDecParams", d_out: int, img_stride: int, row_stride: int, d_status: int):
        self._check(self._lib.sm_png_decode_batch_device(self.ctx, d_files, d_offsets, d_sizes, nimg, H, W,
                                                         ctypes.byref(prm), d_out, img_stride, row_stride, d_status))

    def jpeg_decode(self, buf, prm: "SmJpegDecParams", out: np.ndarray) -> np.ndarray:
        """sm_jpeg_decode: one file in host memory into the host array ``out`` (decoded on the device)."""
        b = np.frombuffer(buf, np.uint8)
        self._check(self._lib.sm_jpeg_decode(self.ctx, _file_ptr(b), b.size, ctypes.byref(prm), out.ctypes.data,
                                             out.strides[0], None))
        return out

    def jpeg_decode_batch_device(self, d_files: int, d_offsets: int, d_sizes: int, nimg: int, H: int, W: int,
                                 prm: "SmJpegDecParams", d_out: int, img_stride: int, row_stride: int, d_status: int):
        self._check(self._lib.sm_jpeg_decode_batch_device(self.ctx, d_files, d_offsets, d_sizes, nimg, H, W,
                                                          ctypes.byref(prm), d_out, img_stride, row_stride, d_status))

    def jpeg_decode_stats(self):
        """(sub-sequences, synchronisation rounds) of this context's last JPEG decode call."""
        return jpeg_decode_stats(self.ctx)

    def png_decode_stats(self):
        """(parallel, serial): the inflate paths of the images of the last decode call."""
        return png_decode_stats(self.ctx)

    def png_encode_batch_device(self, d_img: int, img_stride: int, row_stride: int, nimg: int, H: int, W: int,
                                prm: "SmPngParams", capacity_bytes: int, d_out: int, d_nbytes: int):
        self._check(self._lib.sm_png_encode_batch_device(
            self.ctx, ctypes.c_void_p(d_img), img_stride, row_stride, nimg, H, W, ctypes.byref(prm), capacity_bytes,
            ctypes.c_void_p(d_out or None), ctypes.c_void_p(d_nbytes or None)))

    def mccnn_set_weights(self, weights, biases):
        """sm_mccnn_set_weights: float32 arrays w0 [64,1,3,3], w1.. [64,64,3,3] and b0.. [64]."""
        self._check(self._lib.sm_mccnn_set_weights(self.ctx, len(weights), _ptr_array(weights), _ptr_array(biases)))

    def mccnn_features(self, gray: np.ndarray) -> np.ndarray:
        """sm_mccnn_features: contiguous uint8 [n, H, W] -> float32 [n, H, W, 64]."""
        n, H, W = gray.shape
        feat = np.empty((n, H, W, 64), np.float32)
        self._check(self._lib.sm_mccnn_features(self.ctx, gray.ctypes.data, n, H, W, feat.ctypes.data))
        return feat

    def mccnn_join(self, fa: np.ndarray, fb: np.ndarray, D: int, min_disparity: int) -> np.ndarray:
        """sm_mccnn_join: feature maps [n, H, W, 64] -> the volume [n, D, H, W]."""
        n, H, W = fa.shape[:3]
        vol = np.empty((n, D, H, W), np.float32)
        self._check(self._lib.sm_mccnn_join(self.ctx, fa.ctypes.data, fb.ctypes.data, n, H, W, D, min_disparity,
                                            vol.ctypes.data))
        return vol

    def mccnn_volume(self, a: np.ndarray, b: np.ndarray, D: int, min_disparity: int) -> np.ndarray:
        """sm_mccnn_volume: contiguous uint8 [n, H, W] images -> the volume [n, D, H, W]."""
        n, H, W = a.shape
        vol = np.empty((n, D, H, W), np.float32)
        self._check(self._lib.sm_mccnn_volume(self.ctx, a.ctypes.data, b.ctypes.data, n, H, W, D, min_disparity,
                                              vol.ctypes.data))
        return vol

    def mcacc_set_weights(self, conv_w, conv_b, fc_w, fc_b):
        """sm_mcacc_set_weights: float32 arrays w0 [112,1,3,3], w1.. [112,112,3,3], b [112]; fw0 [U,224],
        fw1.. [U,U], the last [1,U]; fb [U], the last [1]."""
        self._check(self._lib.sm_mcacc_set_weights(self.ctx, len(conv_w), _ptr_array(conv_w), _ptr_array(conv_b),
                                                   len(fc_w) - 1, fc_w[0].shape[0], _ptr_array(fc_w), _ptr_array(fc_b)))

    def mcacc_set_precision(self, precision: str):
        """sm_mcacc_set_precision: "f32" or "bf16", for the joins and volumes that follow."""
        if precision not in MCACC_PRECISIONS:
            raise ValueError(f"precision {precision!r}: 'f32' or 'bf16'")
        self._check(self._lib.sm_mcacc_set_precision(self.ctx, MCACC_PRECISIONS[precision]))

    def mcacc_features(self, gray: np.ndarray) -> np.ndarray:
        """sm_mcacc_features: contiguous uint8 [n, H, W] -> float32 [n, H, W, 112]."""
        n, H, W = gray.shape
        feat = np.empty((n, H, W, 112), np.float32)
        self._check(self._lib.sm_mcacc_features(self.ctx, gray.ctypes.data, n, H, W, feat.ctypes.data))
        return feat

    def mcacc_join(self, fa: np.ndarray, fb: np.ndarray, D: int, min_disparity: int, a_is_left: bool, raw: bool) -> np.ndarray:
        """sm_mcacc_join: feature maps [n, H, W, 112] -> the volume [n, D, H, W]."""
        n, H, W = fa.shape[:3]
        vol = np.empty((n, D, H, W), np.float32)
        self._check(self._lib.sm_mcacc_join(self.ctx, fa.ctypes.data, fb.ctypes.data, n, H, W, D, min_disparity,
                                            int(bool(a_is_left)), int(bool(raw)), vol.ctypes.data))
        return vol

    def mcacc_volume(self, a: np.ndarray, b: np.ndarray, D: int, min_disparity: int, a_is_left: bool, raw: bool) -> np.ndarray:
        """sm_mcacc_volume: contiguous uint8 [n, H, W] images -> the volume [n, D, H, W]."""
        n, H, W = a.shape
        vol = np.empty((n, D, H, W), np.float32)
        self._check(self._lib.sm_mcacc_volume(self.ctx, a.ctypes.data, b.ctypes.data, n, H, W, D, min_disparity,
                                              int(bool(a_is_left)), int(bool(raw)), vol.ctypes.data))
        return vol

    def mcacc_features_device(self, d_gray: int, n: int, image_stride: int, H: int, W: int, row_stride: int, d_feat: int):
        self._check(self._lib.sm_mcacc_features_device(self.ctx, d_gray, n, image_stride, H, W, row_stride, d_feat))

    def mcacc_join_device(self, d_fa: int, d_fb: int, n: int, H: int, W: int, D: int, min_disparity: int, a_is_left: bool,
                          raw: bool, d_vol: int):
        self._check(self._lib.sm_mcacc_join_device(self.ctx, d_fa, d_fb, n, H, W, D, min_disparity, int(bool(a_is_left)),
                                                   int(bool(raw)), d_vol))

    def mcacc_volume_device(self, d_a: int, d_b: int, n: int, image_stride: int, H: int, W: int, row_stride: int,
                            D: int, min_disparity: int, a_is_left: bool, raw: bool, d_vol: int):
        self._check(self._lib.sm_mcacc_volume_device(self.ctx, d_a, d_b, n, image_stride, H, W, row_stride, D,
                                                     min_disparity, int(bool(a_is_left)), int(bool(raw)), d_vol))

    def mccnn_features_device(self, d_gray: int, n: int, image_stride: int, H: int, W: int, row_stride: int, d_feat: int):
        self._check(self._lib.sm_mccnn_features_device(self.ctx, d_gray, n, image_stride, H, W, row_stride, d_feat))

    def mccnn_join_device(self, d_fa: int, d_fb: int, n: int, H: int, W: int, D: int, min_disparity: int, d_vol: int):
        self._check(self._lib.sm_mccnn_join_device(self.ctx, d_fa, d_fb, n, H, W, D, min_disparity, d_vol))

    def mccnn_volume_device(self, d_a: int, d_b: int, n: int, image_stride: int, H: int, W: int, row_stride: int,
                            D: int, min_disparity: int, d_vol: int):
        self._check(self._lib.sm_mccnn_volume_device(self.ctx, d_a, d_b, n, image_stride, H, W, row_stride, D,
                                                     min_disparity, d_vol))

    def mcsgm_aggregate(self, vol: np.ndarray, a: np.ndarray, b: np.ndarray, min_disparity: int,
                        prm: "SmMcsgmParams") -> np.ndarray:
        """sm_mcsgm_aggregate: contiguous float32 [n, D, H, W] and uint8 [n, H, W] images."""
        n, D, H, W = vol.shape
        agg = np.empty_like(vol)
        self._check(self._lib.sm_mcsgm_aggregate(self.ctx, vol.ctypes.data, a.ctypes.data, b.ctypes.data, n, H, W, D,
                                                 min_disparity, ctypes.byref(prm), agg.ctypes.data))
        return agg

    def mcsgm_disparity(self, agg_l: np.ndarray, agg_r: np.ndarray, a: np.ndarray, min_disparity: int,
                        prm: "SmMcsgmParams", stages: bool):
        """sm_mcsgm_disparity: (disparity [n, H, W] float32, dict of the stage maps or None)."""
        n, D, H, W = agg_l.shape
        disp = np.empty((n, H, W), np.float32)
        maps, st = mcsgm_stage_arrays(n, H, W) if stages else (None, None)
        self._check(self._lib.sm_mcsgm_disparity(self.ctx, agg_l.ctypes.data, agg_r.ctypes.data, a.ctypes.data, n, H, W, D,
                                                 min_disparity, ctypes.byref(prm), disp.ctypes.data,
                                                 ctypes.byref(st) if stages else None))
        return disp, maps

    def mcsgm_aggregate_device(self, d_vol: int, d_a: int, d_b: int, n: int, image_stride: int, H: int, W: int,
                               row_stride: int, D: int, min_disparity: int, prm: "SmMcsgmParams", d_agg: int):
        self._check(self._lib.sm_mcsgm_aggregate_device(self.ctx, d_vol, d_a, d_b, n, image_stride, H, W, row_stride, D,
                                                        min_disparity, ctypes.byref(prm), d_agg))

    def mcsgm_disparity_device(self, d_agg_l: int, d_agg_r: int, d_a: int, n: int, image_stride: int, H: int, W: int,
                               row_stride: int, D: int, min_disparity: int, prm: "SmMcsgmParams", d_disp: int,
                               stages: "SmMcsgmStages" = None):
        self._check(self._lib.sm_mcsgm_disparity_device(self.ctx, d_agg_l, d_agg_r, d_a, n, image_stride, H, W, row_stride,
                                                        D, min_disparity, ctypes.byref(prm), d_disp,
                                                        ctypes.byref(stages) if stages is not None else None))

    def mccbca_arms(self, img: np.ndarray, prm: "SmMccbcaParams") -> np.ndarray:
        """sm_mccbca_arms: contiguous uint8 [n, H, W] -> uint8 [n, 4, H, W] (left, right, up, down)."""
        n, H, W = img.shape
        arms = np.empty((n, 4, H, W), np.uint8)
        self._check(self._lib.sm_mccbca_arms(self.ctx, img.ctypes.data, n, H, W, ctypes.byref(prm), arms.ctypes.data))
        return arms

    def mccbca_aggregate(self, vol: np.ndarray, a: np.ndarray, b: np.ndarray, min_disparity: int,
                         prm: "SmMccbcaParams", iterations: int) -> np.ndarray:
        """sm_mccbca_aggregate: contiguous float32 [n, D, H, W] and uint8 [n, H, W] images."""
        n, D, H, W = vol.shape
        agg = np.empty_like(vol)
        self._check(self._lib.sm_mccbca_aggregate(self.ctx, vol.ctypes.data, a.ctypes.data, b.ctypes.data, n, H, W, D,
                                                  min_disparity, ctypes.byref(prm), iterations, agg.ctypes.data))
        return agg

    def mccbca_arms_device(self, d_gray: int, n: int, image_stride: int, H: int, W: int, row_stride: int,
                           prm: "SmMccbcaParams", d_arms: int):
        self._check(self._lib.sm_mccbca_arms_device(self.ctx, d_gray, n, image_stride, H, W, row_stride, ctypes.byref(prm),
                                                    d_arms))

    def mccbca_aggregate_device(self, d_vol: int, d_a: int, d_b: int, n: int, image_stride: int, H: int, W: int,
                                row_stride: int, D: int, min_disparity: int, prm: "SmMccbcaParams", iterations: int,
                                d_agg: int):
        self._check(self._lib.sm_mccbca_aggregate_device(self.ctx, d_vol, d_a, d_b, n, image_stride, H, W, row_stride, D,
                                                         min_disparity, ctypes.byref(prm), iterations, d_agg))

    def nlm_denoise(self, src: np.ndarray, h: float, template_window: int, search_window: int,
                    dst: np.ndarray = None) -> np.ndarray:
        """fastNlMeansDenoising of a uint8 [H, W] image (any row stride, pixels contiguous);
        ``dst`` (uint8 [H, W], C-contiguous) is filled and returned when given."""
        if not isinstance(src, np.ndarray) or src.dtype != np.uint8 or src.ndim != 2:
            raise ValueError("nlm_denoise: src must be a uint8 [H, W] array")
        if src.size and (src.strides[1] != 1 or src.strides[0] < src.shape[1]):
            src = np.ascontiguousarray(src)
        H, W = src.shape
        if dst is None:
            dst = np.empty((H, W), np.uint8)
        elif (not isinstance(dst, np.ndarray) or dst.dtype != np.uint8 or dst.shape != (H, W)
              or not dst.flags.c_contiguous or not dst.flags.writeable):
            raise ValueError(f"nlm_denoise: dst must be a writeable C-contiguous uint8 [{H}, {W}] array")
        self._check(self._lib.sm_nlm_denoise_u8(self.ctx, src.ctypes.data if src.size else None, H, W,
                                                src.strides[0] if src.size else W, float(h), int(template_window),
                                                int(search_window), dst.ctypes.data if dst.size else None))
        return dst

    def nlm_denoise_batch_device(self, d_src: int, nimg: int, img_stride: int, H: int, W: int, src_stride: int,
                                 h: float, template_window: int, search_window: int, d_dst: int):
        self._check(self._lib.sm_nlm_denoise_u8_batch_device(
            self.ctx, ctypes.c_void_p(d_src), nimg, img_stride, H, W, src_stride, float(h), int(template_window),
            int(search_window), ctypes.c_void_p(d_dst)))

    def nlm_weight_table(self, h: float, template_window: int, search_window: int):
        """(tab int32 [n], fpm, shift): the weight table nlm_denoise uses (sm_nlm_weight_table)."""
        n, fpm, shift = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        args = (float(h), int(template_window), int(search_window))
        rc = self._lib.sm_nlm_weight_table(*args, None, ctypes.byref(n), ctypes.byref(fpm), ctypes.byref(shift))
        if rc != SM_OK:
            _raise(rc, None)  # a context-free call: the message is the thread's
        tab = np.empty(n.value, np.int32)
        rc = self._lib.sm_nlm_weight_table(*args, tab.ctypes.data, ctypes.byref(n), ctypes.byref(fpm),
                                           ctypes.byref(shift))
        if rc != SM_OK:
            _raise(rc, None)
        return tab, fpm.value, shift.value

    # -- gaussian_filter, image_measure, pyrDown ---------------------------
    @staticmethod
    def _half_kernel(w):
        """(array kept alive, pointer or None, r) of a half kernel w[0..r] (None: identity)."""
        if w is None:
            return None, None, 0
        w = np.ascontiguousarray(w, np.float64)
        if w.ndim != 1 or w.size < 1:
            raise ValueError("a half kernel is a 1-D float64 array w[0..r], centre first")
        return w, w.ctypes.data, w.size - 1

    def gauss2d(self, src: np.ndarray, wy, wx) -> np.ndarray:
        """sm_gauss2d_f64 of a float64 [H, W] or [N, H, W] array (any row and image stride,
        pixels contiguous) with the half kernels ``wy`` (axis 0) and ``wx`` (axis 1)."""
        if not isinstance(src, np.ndarray) or src.dtype != np.float64 or src.ndim not in (2, 3):
            raise ValueError("gauss2d: src must be a float64 [H, W] or [N, H, W] array")
        a = src if src.ndim == 3 else src[None]
        n, H, W = a.shape
        ok = a.size == 0 or (a.strides[2] == 8 and a.strides[1] % 8 == 0 and a.strides[1] >= 8 * W and
                             (n == 1 or (a.strides[0] % 8 == 0 and a.strides[0] >= (H - 1) * a.strides[1] + 8 * W)))
        if not ok:
            a = np.ascontiguousarray(a)
        ky, py, ry = self._half_kernel(wy)
        kx, px, rx = self._half_kernel(wx)
        out = np.empty((n, H, W), np.float64)
        self._check(self._lib.sm_gauss2d_f64(self.ctx, a.ctypes.data if a.size else None, n,
                                             a.strides[0] // 8 if n > 1 else 0, H, W, a.strides[1] // 8 if a.size else W,
                                             py, ry, px, rx, out.ctypes.data if out.size else None))
        return out if src.ndim == 3 else out[0]

    def gauss2d_batch_device(self, d_src: int, nimg: int, src_img_stride: int, H: int, W: int, src_stride: int, wy, wx,
                             d_dst: int, dst_img_stride: int, dst_stride: int):
        """Strides count doubles."""
        ky, py, ry = self._half_kernel(wy)
        kx, px, rx = self._half_kernel(wx)
        self._check(self._lib.sm_gauss2d_f64_batch_device(
            self.ctx, ctypes.c_void_p(d_src), nimg, src_img_stride, H, W, src_stride, py, ry, px, rx,
            ctypes.c_void_p(d_dst), dst_img_stride, dst_stride))

    def image_measure(self, bgr: np.ndarray, w1, w2, alpha: float) -> np.ndarray:
        """sm_image_measure_u8 of a uint8 [H, W, 3] image: float64 [H, W]."""
        if not isinstance(bgr, np.ndarray) or bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3:
            raise ValueError("image_measure: the image must be a uint8 [H, W, 3] array")
        bgr = np.ascontiguousarray(bgr)
        H, W = bgr.shape[:2]
        k1, p1, r1 = self._half_kernel(w1)
        k2, p2, r2 = self._half_kernel(w2)
        out = np.empty((H, W), np.float64)
        self._check(self._lib.sm_image_measure_u8(self.ctx, bgr.ctypes.data if bgr.size else None, H, W, 3 * W, p1, r1,
                                                  p2, r2, float(alpha), out.ctypes.data if out.size else None))
        return out

    def image_measure_batch_device(self, d_bgr: int, nimg: int, img_stride: int, H: int, W: int, src_stride: int, w1,
                                   w2, alpha: float, d_dst: int):
        k1, p1, r1 = self._half_kernel(w1)
        k2, p2, r2 = self._half_kernel(w2)
        self._check(self._lib.sm_image_measure_u8_batch_device(
            self.ctx, ctypes.c_void_p(d_bgr), nimg, img_stride, H, W, src_stride, p1, r1, p2, r2, float(alpha),
            ctypes.c_void_p(d_dst)))

    def pyr_down(self, src: np.ndarray) -> np.ndarray:
        """sm_pyr_down_u8 of a uint8 [H, W] or [H, W, 3] image (any row stride, pixels contiguous)."""
        if not isinstance(src, np.ndarray) or src.dtype != np.uint8 or src.ndim not in (2, 3):
            raise ValueError("pyr_down: src must be a uint8 [H, W] or [H, W, 3] array")
        cn = 1 if src.ndim == 2 else src.shape[2]
        H, W = src.shape[:2]
        if src.size and (src.strides[1] != cn or (src.ndim == 3 and src.strides[2] != 1) or src.strides[0] < W * cn):
            src = np.ascontiguousarray(src)
        dH, dW = (H + 1) // 2, (W + 1) // 2
        out = np.empty((dH, dW) if src.ndim == 2 else (dH, dW, cn), np.uint8)
        self._check(self._lib.sm_pyr_down_u8(self.ctx, src.ctypes.data if src.size else None, H, W,
                                             src.strides[0] if src.size else W * cn, cn,
                                             out.ctypes.data if out.size else None))
        return out

    def pyr_down_batch_device(self, d_src: int, nimg: int, src_img_stride: int, H: int, W: int, src_stride: int,
                              channels: int, d_dst: int, dst_img_stride: int, dst_stride: int):
        """Strides count bytes."""
        self._check(self._lib.sm_pyr_down_u8_batch_device(
            self.ctx, ctypes.c_void_p(d_src), nimg, src_img_stride, H, W, src_stride, channels, ctypes.c_void_p(d_dst),
            dst_img_stride, dst_stride))

    # -- StereoBM -------------------------------------------------------------------
    def bm_compute(self, left: np.ndarray, right: np.ndarray, params: "SmBmParams") -> np.ndarray:
        left = np.ascontiguousarray(left)
        right = np.ascontiguousarray(right)
        H, W = left.shape
        out = np.empty((H, W), np.int16)
        self._check(self._lib.sm_bm_compute(self.ctx, left.ctypes.data, right.ctypes.data, H, W, W,
                                            ctypes.byref(params), out.ctypes.data))
        return out

    def bm_compute_batch_device(self, d_left: int, d_right: int, npairs: int, pair_stride: int, H: int, W: int,
                                stride: int, params: "SmBmParams", d_out: int):
        self._check(self._lib.sm_bm_compute_batch_device(
            self.ctx, ctypes.c_void_p(d_left), ctypes.c_void_p(d_right), npairs, pair_stride, H, W, stride,
            ctypes.byref(params), ctypes.c_void_p(d_out)))

    def synchronize(self):
        self._check(self._lib.sm_synchronize(self.ctx))

    COUNTERS = ("sweep_fallbacks", "ew_repairs", "volume_clamped", "volume_nan", "line_groups",
                "ew_open", "band_repairs", "band_open", "band_groups", "line_strips")  # SM_COUNTER_*

    def counters(self) -> dict:
        """Counters since the engine was created (include/stereo_match_amd.h SM_COUNTER_*):
        sweep_fallbacks (launch groups the guarded fallback recomputed), ew_repairs (in-sweep
        E/W strip segments the patch pass recomputed), volume_clamped / volume_nan (external
        cost-volume cells clamped by the quantisation window / NaN), line_groups (launch groups
        whose E/W paths ran inside the down sweep), ew_open (of the ew_repairs, segments whose
        recomputation had not met the speculative values by the strip's end), band_repairs /
        band_open / band_groups (the row-band engine's repaired chains, chains that crossed a
        boundary, launch groups), line_strips (strips x pairs of the line_groups)."""
        out = {}
        n = ctypes.c_longlong()
        for i, name in enumerate(self.COUNTERS):
            self._check(self._lib.sm_get_counter(self.ctx, i, ctypes.byref(n)))
            out[name] = n.value
        return out

    def set_cu_mask(self, cus):
        """Restrict the context's streams to the CU indices in ``cus`` (None: all)."""
        if cus is None:
            self._check(self._lib.sm_set_cu_mask(self.ctx, None, 0))
            return
        nwords = (max(cus) // 32 + 1) if cus else 1
        words = (ctypes.c_uint32 * nwords)()
        for c in cus:
            words[c // 32] |= 1 << (c % 32)
        self._check(self._lib.sm_set_cu_mask(self.ctx, words, nwords))

    # -- timing ---------------------------------------------------------------
    def set_timing(self, on, stages=None):
        """on: every stage; with ``stages`` (names from STAGES) only those stages
        record events (each timed stage delays the stream a little)."""
        v = int(bool(on))
        if on and stages is not None:
            v = TIMING_ONLY
            for name in stages:
                v |= 1 << STAGES.index(name)
        self._check(self._lib.sm_set_timing(self.ctx, v))

    def reset_timing(self):
        self._check(self._lib.sm_reset_timing(self.ctx))

    def timing(self) -> dict:
        """{stage: (total_ms, launches, pairs)}"""
        out = {}
        for i, name in enumerate(STAGES):
            ms = ctypes.c_double()
            n = ctypes.c_longlong()
            np_ = ctypes.c_longlong()
            self._check(self._lib.sm_get_timing(self.ctx, i, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(np_)))
            out[name] = (ms.value, n.value, np_.value)
        return out

    # -- debug ------------------------------------------------------------------
    def set_debug_flags(self, flags: int):
        """Timing ablations only (results become wrong); 0 = normal."""
        self._check(self._lib.sm_set_debug_flags(self.ctx, int(flags)))

    TUNE_EW_LANES, TUNE_SWEEP_NCW, TUNE_EW_WAVES, TUNE_EW_PRIO, TUNE_EW_WARMUP, TUNE_SWEEP_LINES = 1, 2, 3, 4, 5, 6
    TUNE_EW_GUESS = 7
    TUNE_BANDS, TUNE_BAND_WARMUP, TUNE_BAND_GUESS, TUNE_COST_WGS, TUNE_LR_STAGGER, TUNE_SWEEP_XCD = 8, 9, 10, 11, 12, 13
    TUNE_PLY_STAGE = 14
    TUNE_EW_START = 15
    TUNE_EW_PATCH = 16
    TUNE_HOP_EPOCH = 17
    TUNE_MCACC_CHUNK = 18

    def set_tuning(self, key: int, value: int):
        """Launch-shape knob (include/stereo_match_amd.h sm_set_tuning); 0 = automatic."""
        self._check(self._lib.sm_set_tuning(self.ctx, int(key), int(value)))

    def debug_fetch(self, what: int) -> bytes:
        n = self._lib.sm_debug_fetch(self.ctx, what, None, 0)
        if n < 0:
            _raise(int(n), self.ctx)
        buf = (ctypes.c_char * max(int(n), 1))()
        r = self._lib.sm_debug_fetch(self.ctx, what, buf, int(n))
        if r < 0:
            _raise(int(r), self.ctx)
        return bytes(buf)[:int(n)]


def right_matcher_params(p: SmParams) -> SmParams:
    lib = load()
    out = SmParams()
    rc = lib.sm_right_matcher_params(ctypes.byref(p), ctypes.byref(out))
    if rc != SM_OK:
        _raise(rc, None)
    return out


def compute_batch(engines, lefts, rights, params: SmParams) -> np.ndarray:
    """sm_compute_batch over several Engines (one per device): host pairs in,
    int16 [n, H, W] out; pairs sharded contiguously across the engines."""
    lib = load()
    n = len(lefts)
    if n != len(rights):
        raise ValueError("lefts and rights differ in length")
    if n == 0:
        return np.empty((0, 0, 0), np.int16)
    L = [np.ascontiguousarray(a, np.uint8) for a in lefts]
    R = [np.ascontiguousarray(b, np.uint8) for b in rights]
    H, W = L[0].shape
    if any(a.shape != (H, W) for a in L + R):
        raise ValueError("all images must have the same shape")
    out = np.empty((n, H, W), np.int16)
    ctxs = (ctypes.c_void_p * len(engines))(*[e.ctx for e in engines])
    lp = (ctypes.c_void_p * n)(*[a.ctypes.data for a in L])
    rp = (ctypes.c_void_p * n)(*[b.ctypes.data for b in R])
    rc = lib.sm_compute_batch(ctxs, len(engines), lp, rp, n, H, W, ctypes.byref(params), out.ctypes.data)
    if rc != SM_OK:
        _raise(rc, None)
    return out


_engines: dict = {}


def engine(device: int = 0) -> Engine:
    """Per-(thread, device) cached engine."""
    key = (threading.get_ident(), device)
    e = _engines.get(key)
    if e is None:
        e = _engines[key] = Engine(device)
    return e
