"""ctypes binding of the C ABI in include/md2hot.h (libmd2hot.so).

There is deliberately no fallback: if the library is missing or fails to load,
`lib()` raises.  The library must be loaded after `import torch` so that its
libamdhip64.so.7 dependency resolves to the HIP runtime torch already loaded.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

from .build import LIB_PATH as _BUILT_LIB
from .build import source_hash

# MD2_LIB overrides the library path (A/B runs of alternative builds: their build id
# is not checked against the tree)
LIB_PATH = os.environ.get("MD2_LIB", _BUILT_LIB)

MAX_SCALES = 4
MAX_SRC = 3
ABI_VERSION = 24

NO_SSIM = 1 << 0
AVG_REPROJECTION = 1 << 1
NO_AUTOMASK = 1 << 2
V1_MULTISCALE = 1 << 3
T_PER_SCALE = 1 << 4
PREDICTIVE_MASK = 1 << 5

_vp = ctypes.c_void_p


class Desc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("num_src", ctypes.c_int32), ("num_scales", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("min_depth", ctypes.c_float), ("max_depth", ctypes.c_float),
                ("disparity_smoothness", ctypes.c_float), ("disp_dtype", ctypes.c_uint32),
                ("seed", ctypes.c_uint64)]


class Tensors(ctypes.Structure):
    _fields_ = [("disp", _vp * MAX_SCALES),
                ("color", (_vp * (1 + MAX_SRC)) * MAX_SCALES),
                ("K", _vp * MAX_SCALES),
                ("inv_K", _vp * MAX_SCALES),
                ("T", _vp),
                ("noise", _vp),
                ("seed_ptr", _vp),
                ("mask", _vp),
                ("src8", _vp)]


_lock = threading.Lock()
_lib = None

EXPORTS = ["md2_abi_version", "md2_last_error", "md2_workspace_bytes", "md2_select_bytes",
           "md2_photometric_fwd", "md2_photometric_bwd", "md2_generate_images", "md2_tiebreak_noise",
           "md2_timing_begin", "md2_timing_end", "md2_timing_calls", "md2_decoder_pad_fwd", "md2_decoder_pad_bwd",
           "md2_decoder_pad_workspace_bytes", "md2_adam_step", "md2_adam_step_dev", "md2_adam_hyper", "md2_adam_apply_dev", "md2_encoder_input",
           "md2_pose_fwd", "md2_pose_bwd", "md2_aug_plan_create", "md2_aug_plan_destroy", "md2_aug_run",
           "md2_bn_workspace_bytes", "md2_bn_fwd", "md2_bn_bwd", "md2_maxpool3s2_fwd", "md2_maxpool3s2_bwd",
           "md2_disp_head_workspace_bytes", "md2_disp_head_fwd", "md2_disp_head_bwd",
           "md2_stem_wgrad_workspace_bytes", "md2_stem_wgrad", "md2_stem_fwd", "md2_conv_col2im", "md2_bias_act_fwd", "md2_bias_act_bwd",
           "md2_bias_act_workspace_bytes", "md2_maxpool3s2_bwd_add", "md2_bn_bwd_multi",
           "md2_conv_fwd", "md2_conv_workspace_bytes", "md2_conv_split_weights",
           "md2_conv_dgrad", "md2_conv_wgrad", "md2_conv_direct", "md2_conv_wgrad_direct",
           "md2_conv_wgrad_direct_workspace_bytes", "md2_conv_split_weights_multi", "md2_bn_fwd_mask",
           "md2_bn_bwd_mask", "md2_build_id", "md2_maxpool3s2_bwd_multi", "md2_decoder_pad_bwd2", "md2_aug_run2",
           "md2_conv_bf16_weights", "md2_conv_bf16_weights_multi",
           "md2_depth_eval", "md2_depth_eval_workspace_bytes",
           "md2_velo_project", "md2_velo_project_workspace_bytes",
           "md2_pose_ate", "md2_pose_ate_workspace_bytes",
           "md2_disp_colorize", "md2_disp_colorize_workspace_bytes",
           "md2_bn_pool_fwd_supported", "md2_bn_pool_fwd", "md2_bn_bwd_reduce_mask", "md2_bn_coef_offset",
           "md2_stem_wgrad_bn_supported", "md2_stem_wgrad_bn",
           "md2_aug_plan_create_mixed", "md2_aug_run_mixed",
           "md2_depth_export16", "md2_depth_export16_check",
           "md2_jpeg_workspace_bytes", "md2_jpeg_check", "md2_jpeg_plan_create", "md2_jpeg_plan_destroy",
           "md2_jpeg_run",
           "md2_jpeg_index_bytes", "md2_jpeg_index", "md2_jpeg_check_indexed", "md2_jpeg_run_indexed",
           "md2_jpeg_encode_bound", "md2_jpeg_encode_workspace_bytes", "md2_jpeg_encode_check", "md2_jpeg_encode",
           "md2_png_workspace_bytes", "md2_png_check", "md2_png_run",
           "md2_png_index_bytes", "md2_png_indexed_workspace_bytes", "md2_png_index", "md2_png_check_indexed",
           "md2_png_run_indexed",
           "md2_png_encode_bound", "md2_png_encode_workspace_bytes", "md2_png_encode_check", "md2_png_encode",
           "md2_log_panel_tile_blocks", "md2_log_panel_check", "md2_log_panel_workspace_bytes", "md2_log_panel",
           "md2_depth_points", "md2_depth_points_workspace_bytes"]

DTYPE_F32 = 0    # md2_desc.disp_dtype
DTYPE_BF16 = 1
PAD_ELU = 1 << 0
PAD_UPSAMPLE = 1 << 1
PAD_NHWC = 1 << 2
PAD_BF16 = 1 << 3


class PadDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32),
                ("width", ctypes.c_int32), ("skip_channels", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class AugDesc(ctypes.Structure):
    _fields_ = [("items", ctypes.c_int32), ("frames", ctypes.c_int32), ("in_height", ctypes.c_int32),
                ("in_width", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("num_scales", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AugItem(ctypes.Structure):
    _fields_ = [("flip", ctypes.c_uint8), ("color_aug", ctypes.c_uint8), ("hue_shift", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8), ("order", ctypes.c_uint8 * 4), ("brightness", ctypes.c_float),
                ("contrast", ctypes.c_float), ("saturation", ctypes.c_float)]


BN_RELU = 1 << 0
BN_RESIDUAL = 1 << 1
BN_BF16 = 1 << 2


class BnDesc(ctypes.Structure):
    _fields_ = [("pixels", ctypes.c_int64), ("channels", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("eps", ctypes.c_float), ("momentum", ctypes.c_float), ("groups", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


POOL_BF16 = 1 << 0


CONV_NO_SPLIT = 1 << 1
CONV_TILE_N32 = 1 << 2
CONV_TILE_N64 = 1 << 3
CONV_TILE_N128 = 1 << 4
CONV_X6 = 1 << 5
CONV_BM256 = 1 << 6
CONV_PRESPLIT = 1 << 7
CONV_PATCH = 1 << 8
CONV_S2_ONE = 1 << 9
CONV_WS = 1 << 10
CONV_BF16 = 1 << 11   # ABI 22: bf16 operands (autocast convolutions, config C5)


class ConvDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("in_channels", ctypes.c_int32), ("out_channels", ctypes.c_int32), ("kernel_h", ctypes.c_int32),
                ("kernel_w", ctypes.c_int32), ("stride", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("flags", ctypes.c_uint32)]


class WsplitEntry(ctypes.Structure):
    """include/md2hot.h md2_wsplit_entry (one weight of md2_conv_split_weights_multi)."""
    _fields_ = [("weight", _vp), ("planes_fwd", _vp), ("planes_dgrad", _vp), ("co", ctypes.c_int32),
                ("kt", ctypes.c_int32), ("ci", ctypes.c_int32), ("block0", ctypes.c_int32), ("planes_col", _vp)]


class PoolDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32),
                ("width", ctypes.c_int32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32)]


HEAD_WEIGHT_CL = 1 << 0
HEAD_BF16 = 1 << 1   # ABI 23: bf16 padded input / its gradient


class HeadDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32),
                ("width", ctypes.c_int32), ("flags", ctypes.c_uint32)]


STEM_WEIGHT_CL = 1 << 0
STEM_BF16 = 1 << 1   # ABI 23: md2_stem_wgrad on bf16 x / grad_y
STEM_PREFETCH = 1 << 2   # the fp32 weight gradient's prefetching form for this call (MD2_STEM_PF32=1: every call)


class StemDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32),
                ("width", ctypes.c_int32), ("flags", ctypes.c_uint32)]


BIAS_ACT_RELU = 1 << 0


class BiasActDesc(ctypes.Structure):
    _fields_ = [("pixels", ctypes.c_int64), ("channels", ctypes.c_int32), ("flags", ctypes.c_uint32)]


# ABI 24: md2_depth_eval (csrc/eval.hip)
EVAL_POST_PROCESS = 1 << 0
EVAL_RESIZE_DEPTH = 1 << 1
EVAL_GT_RANGE = 1 << 2
EVAL_MEDIAN_SCALE = 1 << 3
EVAL_MEDIAN_LOWER = 1 << 4
EVAL_POOL_BATCH = 1 << 5
EVAL_OUT = 10   # floats per population


class EvalDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("gt_height", ctypes.c_int32), ("gt_width", ctypes.c_int32),
                ("crop_y0", ctypes.c_int32), ("crop_y1", ctypes.c_int32), ("crop_x0", ctypes.c_int32),
                ("crop_x1", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("min_depth", ctypes.c_double), ("max_depth", ctypes.c_double),
                ("eval_min", ctypes.c_float), ("eval_max", ctypes.c_float),
                ("scale_factor", ctypes.c_double)]


# md2_velo_project (csrc/velo.hip): new symbols under ABI 24, no version bump
VELO_VEL_DEPTH = 1 << 0


class VeloDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("total_points", ctypes.c_int64), ("reserved", ctypes.c_int32 * 2)]


# md2_pose_ate (csrc/traj.hip): new symbols under ABI 24, no version bump
class PoseAteDesc(ctypes.Structure):
    _fields_ = [("sequences", ctypes.c_int32), ("track_length", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("reserved0", ctypes.c_int32), ("total_frames", ctypes.c_int64), ("reserved", ctypes.c_int64)]


# md2_disp_colorize (csrc/viz.hip): new symbols under ABI 24, no version bump
class VizDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("in_height", ctypes.c_int32), ("in_width", ctypes.c_int32),
                ("out_height", ctypes.c_int32), ("out_width", ctypes.c_int32), ("percentile", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32)]


# md2_depth_export16 (csrc/eval.hip): a new symbol under ABI 24, no version bump
DEPTH16_POST_PROCESS = 1 << 0


class Depth16Desc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("in_height", ctypes.c_int32), ("in_width", ctypes.c_int32),
                ("out_height", ctypes.c_int32), ("out_width", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("min_depth", ctypes.c_double), ("max_depth", ctypes.c_double), ("scale_factor", ctypes.c_double),
                ("clip_max", ctypes.c_double), ("quant", ctypes.c_double), ("reserved", ctypes.c_int64)]


# md2_jpeg_run (csrc/jpeg.hip): new symbols under ABI 24, no version bump
JPEG_444, JPEG_422, JPEG_420 = 0, 1, 2
JPEG_ST_BLOCKS, JPEG_ST_CODE, JPEG_ST_END = 1, 2, 4
JPEG_ST_INDEX = 8        # md2_jpeg_run_indexed: the stored index does not fit the stream
JPEG_QUANT_BYTES = 128   # one bank.quant table: 64 uint16, natural order
JPEG_HUFF_BYTES = 272    # one bank.huff table: counts[16], values[256]


class JpegImage(ctypes.Structure):
    _fields_ = [("stream_offset", ctypes.c_uint64), ("out_offset", ctypes.c_uint64),
                ("stream_bytes", ctypes.c_uint32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("sampling", ctypes.c_int32), ("quant", ctypes.c_uint8 * 3), ("dc", ctypes.c_uint8 * 3),
                ("ac", ctypes.c_uint8 * 3), ("reserved", ctypes.c_uint8 * 7)]


class JpegBank(ctypes.Structure):
    _fields_ = [("quant", _vp), ("huff", _vp), ("num_quant", ctypes.c_int32), ("num_huff", ctypes.c_int32)]


# md2_jpeg_encode (csrc/jpegenc.hip): new symbols under ABI 24, no version bump
JPEGENC_ST_SPACE = 1     # the stream does not fit its output range
JPEGENC_BLOCK_BYTES = 208   # md2_jpeg_encode_bound per block of the scan


class JpegEncImage(ctypes.Structure):
    _fields_ = [("in_offset", ctypes.c_uint64), ("out_offset", ctypes.c_uint64), ("out_capacity", ctypes.c_uint32),
                ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("sampling", ctypes.c_int32),
                ("quant", ctypes.c_uint8 * 2), ("reserved", ctypes.c_uint8 * 6)]


# md2_png_run (csrc/png.hip): new symbols under ABI 24, no version bump
PNG_ST_BLOCK, PNG_ST_CODE, PNG_ST_END, PNG_ST_DIST, PNG_ST_FILTER, PNG_ST_ADLER = 1, 2, 4, 8, 16, 32
PNG_ST_INDEX = 64   # md2_png_run_indexed: the index does not fit the stream
PNG_INDEX_HEADER_BYTES, PNG_INDEX_ENTRY_BYTES = 16, 24   # the index layout (include/md2hot.h)


class PngImage(ctypes.Structure):
    _fields_ = [("height", ctypes.c_int32), ("width", ctypes.c_int32), ("out_offset", ctypes.c_uint64),
                ("stream_offset", ctypes.c_uint64), ("stream_bytes", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


# md2_png_encode (csrc/pngenc.hip): new symbols under ABI 24, no version bump
PNGENC_RGB8, PNGENC_GRAY16 = 0, 1
PNGENC_ST_SPACE = 1      # the stream does not fit its output range


class PngEncImage(ctypes.Structure):
    _fields_ = [("in_offset", ctypes.c_uint64), ("out_offset", ctypes.c_uint64), ("ws_offset", ctypes.c_uint64),
                ("out_capacity", ctypes.c_uint32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("kind", ctypes.c_int32), ("segment_bytes", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


# md2_log_panel (csrc/md2hot.hip): new symbols under ABI 24, no version bump
LOG_COLOR, LOG_WARP, LOG_DISP, LOG_MAP = 0, 1, 2, 3
LOG_MAX_ITEMS = 4
LOG_MAX_TILES = 1024


class LogTile(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("item", ctypes.c_int32), ("scale", ctypes.c_int32),
                ("frame", ctypes.c_int32), ("y", ctypes.c_int32), ("x", ctypes.c_int32), ("h", ctypes.c_int32),
                ("w", ctypes.c_int32), ("src", _vp), ("block0", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class LogDesc(ctypes.Structure):
    _fields_ = [("hot", Desc), ("items", ctypes.c_int32), ("sheet_h", ctypes.c_int32), ("sheet_w", ctypes.c_int32),
                ("num_tiles", ctypes.c_int32)]


# md2_depth_points (csrc/points.hip): new symbols under ABI 24, no version bump
POINTS_DEPTH_INPUT = 1 << 0
POINTS_WORLD = 1 << 1
POINTS_RECORD_BYTES = 15


class PointsDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("disp_a", ctypes.c_float), ("disp_b", ctypes.c_float),
                ("depth_scale", ctypes.c_float), ("near", ctypes.c_float), ("far", ctypes.c_float),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


def _declare(L):
    L.md2_depth_points_workspace_bytes.restype = ctypes.c_size_t
    L.md2_depth_points_workspace_bytes.argtypes = [ctypes.POINTER(PointsDesc)]
    L.md2_depth_points.restype = ctypes.c_int
    L.md2_depth_points.argtypes = [ctypes.POINTER(PointsDesc)] + [_vp] * 5 + [ctypes.c_size_t] + [_vp] * 3
    L.md2_log_panel_tile_blocks.restype = ctypes.c_int
    L.md2_log_panel_tile_blocks.argtypes = [ctypes.POINTER(LogTile)]
    L.md2_log_panel_check.restype = ctypes.c_int
    L.md2_log_panel_check.argtypes = [ctypes.POINTER(LogDesc), ctypes.POINTER(LogTile), ctypes.POINTER(Tensors)]
    L.md2_log_panel_workspace_bytes.restype = ctypes.c_size_t
    L.md2_log_panel_workspace_bytes.argtypes = [ctypes.POINTER(LogDesc)]
    L.md2_log_panel.restype = ctypes.c_int
    L.md2_log_panel.argtypes = [ctypes.POINTER(LogDesc), ctypes.POINTER(Tensors), _vp, ctypes.c_int, _vp, _vp, _vp]
    L.md2_jpeg_workspace_bytes.restype = ctypes.c_size_t
    L.md2_jpeg_workspace_bytes.argtypes = [ctypes.POINTER(JpegImage), ctypes.c_int]
    L.md2_jpeg_check.restype = ctypes.c_int
    L.md2_jpeg_check.argtypes = [ctypes.POINTER(JpegImage), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_uint64, ctypes.c_uint64]
    L.md2_jpeg_plan_create.restype = _vp
    L.md2_jpeg_plan_create.argtypes = [ctypes.c_int, ctypes.c_size_t]
    L.md2_jpeg_plan_destroy.restype = None
    L.md2_jpeg_plan_destroy.argtypes = [_vp]
    L.md2_jpeg_run.restype = ctypes.c_int
    L.md2_jpeg_run.argtypes = [_vp, _vp, ctypes.c_uint64, ctypes.POINTER(JpegImage), ctypes.c_int,
                               ctypes.POINTER(JpegBank), _vp, ctypes.c_uint64, _vp, _vp]
    L.md2_jpeg_index_bytes.restype = ctypes.c_size_t
    L.md2_jpeg_index_bytes.argtypes = [ctypes.c_uint32]
    L.md2_jpeg_index.restype = ctypes.c_int
    L.md2_jpeg_index.argtypes = [_vp, _vp, ctypes.c_uint64, ctypes.POINTER(JpegImage), ctypes.POINTER(ctypes.c_uint64),
                                 ctypes.c_int, ctypes.POINTER(JpegBank), _vp, ctypes.c_uint64, _vp, _vp]
    L.md2_jpeg_check_indexed.restype = ctypes.c_int
    L.md2_jpeg_check_indexed.argtypes = [ctypes.POINTER(JpegImage), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64]
    L.md2_jpeg_run_indexed.restype = ctypes.c_int
    L.md2_jpeg_run_indexed.argtypes = [_vp, _vp, ctypes.c_uint64, ctypes.POINTER(JpegImage),
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.POINTER(JpegBank), _vp,
                                       ctypes.c_uint64, _vp, _vp]
    L.md2_jpeg_encode_bound.restype = ctypes.c_size_t
    L.md2_jpeg_encode_bound.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.md2_jpeg_encode_workspace_bytes.restype = ctypes.c_size_t
    L.md2_jpeg_encode_workspace_bytes.argtypes = [ctypes.POINTER(JpegEncImage), ctypes.c_int]
    L.md2_jpeg_encode_check.restype = ctypes.c_int
    L.md2_jpeg_encode_check.argtypes = [ctypes.POINTER(JpegEncImage), ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                        ctypes.c_uint64]
    L.md2_jpeg_encode.restype = ctypes.c_int
    L.md2_jpeg_encode.argtypes = [_vp, ctypes.c_uint64, ctypes.POINTER(JpegEncImage), _vp, ctypes.c_int, _vp,
                                  ctypes.c_int, _vp, ctypes.c_uint64, _vp, ctypes.c_size_t, _vp, _vp, _vp]
    L.md2_png_workspace_bytes.restype = ctypes.c_size_t
    L.md2_png_workspace_bytes.argtypes = [ctypes.POINTER(PngImage), ctypes.c_int]
    L.md2_png_check.restype = ctypes.c_int
    L.md2_png_check.argtypes = [ctypes.POINTER(PngImage), ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64]
    L.md2_png_run.restype = ctypes.c_int
    L.md2_png_run.argtypes = [_vp, ctypes.c_uint64, ctypes.POINTER(PngImage), _vp, ctypes.c_int, _vp, ctypes.c_size_t,
                              _vp, ctypes.c_uint64, _vp, _vp]
    _u64p = ctypes.POINTER(ctypes.c_uint64)
    L.md2_png_index_bytes.restype = ctypes.c_size_t
    L.md2_png_index_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.md2_png_indexed_workspace_bytes.restype = ctypes.c_size_t
    L.md2_png_indexed_workspace_bytes.argtypes = [ctypes.POINTER(PngImage), ctypes.c_int, ctypes.c_int]
    L.md2_png_index.restype = ctypes.c_int
    L.md2_png_index.argtypes = [_vp, ctypes.c_uint64, ctypes.POINTER(PngImage), _vp, ctypes.c_int, ctypes.c_int, _vp,
                                ctypes.c_uint64, _u64p, _vp, _vp, _vp]
    L.md2_png_check_indexed.restype = ctypes.c_int
    L.md2_png_check_indexed.argtypes = [ctypes.POINTER(PngImage), _u64p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                        ctypes.c_uint64]
    L.md2_png_run_indexed.restype = ctypes.c_int
    L.md2_png_run_indexed.argtypes = [_vp, ctypes.c_uint64, ctypes.POINTER(PngImage), _vp, _u64p, _vp, ctypes.c_int,
                                      ctypes.c_int, _vp, ctypes.c_size_t, _vp, ctypes.c_uint64, _vp, _vp]
    L.md2_png_encode_bound.restype = ctypes.c_size_t
    L.md2_png_encode_bound.argtypes = [ctypes.c_int] * 4
    L.md2_png_encode_workspace_bytes.restype = ctypes.c_size_t
    L.md2_png_encode_workspace_bytes.argtypes = [ctypes.POINTER(PngEncImage), ctypes.c_int]
    L.md2_png_encode_check.restype = ctypes.c_int
    L.md2_png_encode_check.argtypes = [ctypes.POINTER(PngEncImage), ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64]
    L.md2_png_encode.restype = ctypes.c_int
    L.md2_png_encode.argtypes = [_vp, ctypes.c_uint64, ctypes.POINTER(PngEncImage), _vp, ctypes.c_int, _vp,
                                 ctypes.c_size_t, _vp, ctypes.c_uint64, _vp, _vp, _vp]
    L.md2_depth_export16.restype = ctypes.c_int
    L.md2_depth_export16.argtypes = [ctypes.POINTER(Depth16Desc)] + [_vp] * 4
    L.md2_depth_export16_check.restype = ctypes.c_int
    L.md2_depth_export16_check.argtypes = [ctypes.POINTER(Depth16Desc)]
    # the stem's fused BatchNorm passes: new symbols under ABI 24, no version bump
    L.md2_bn_pool_fwd_supported.restype = ctypes.c_int
    L.md2_bn_pool_fwd_supported.argtypes = [ctypes.POINTER(BnDesc), ctypes.c_int, ctypes.c_int]
    L.md2_bn_pool_fwd.restype = ctypes.c_int
    L.md2_bn_pool_fwd.argtypes = [ctypes.POINTER(BnDesc), ctypes.c_int, ctypes.c_int] + [_vp] * 13
    L.md2_bn_bwd_reduce_mask.restype = ctypes.c_int
    L.md2_bn_bwd_reduce_mask.argtypes = [ctypes.POINTER(BnDesc)] + [_vp] * 10
    L.md2_bn_coef_offset.restype = ctypes.c_size_t
    L.md2_bn_coef_offset.argtypes = [ctypes.POINTER(BnDesc)]
    L.md2_stem_wgrad_bn_supported.restype = ctypes.c_int
    L.md2_stem_wgrad_bn_supported.argtypes = [ctypes.POINTER(StemDesc)]
    L.md2_stem_wgrad_bn.restype = ctypes.c_int
    L.md2_stem_wgrad_bn.argtypes = [ctypes.POINTER(StemDesc)] + [_vp] * 6 + [ctypes.c_int] + [_vp] * 3
    L.md2_disp_colorize_workspace_bytes.restype = ctypes.c_size_t
    L.md2_disp_colorize_workspace_bytes.argtypes = [ctypes.POINTER(VizDesc)]
    L.md2_disp_colorize.restype = ctypes.c_int
    L.md2_disp_colorize.argtypes = [ctypes.POINTER(VizDesc)] + [_vp] * 6
    L.md2_pose_ate_workspace_bytes.restype = ctypes.c_size_t
    L.md2_pose_ate_workspace_bytes.argtypes = [ctypes.POINTER(PoseAteDesc)]
    L.md2_pose_ate.restype = ctypes.c_int
    L.md2_pose_ate.argtypes = [ctypes.POINTER(PoseAteDesc)] + [_vp] * 7
    L.md2_velo_project_workspace_bytes.restype = ctypes.c_size_t
    L.md2_velo_project_workspace_bytes.argtypes = [ctypes.POINTER(VeloDesc)]
    L.md2_velo_project.restype = ctypes.c_int
    L.md2_velo_project.argtypes = [ctypes.POINTER(VeloDesc)] + [_vp] * 6
    L.md2_depth_eval_workspace_bytes.restype = ctypes.c_size_t
    L.md2_depth_eval_workspace_bytes.argtypes = [ctypes.POINTER(EvalDesc)]
    L.md2_depth_eval.restype = ctypes.c_int
    L.md2_depth_eval.argtypes = [ctypes.POINTER(EvalDesc)] + [_vp] * 6
    L.md2_bias_act_fwd.restype = ctypes.c_int
    L.md2_bias_act_fwd.argtypes = [ctypes.POINTER(BiasActDesc)] + [_vp] * 4
    L.md2_bias_act_bwd.restype = ctypes.c_int
    L.md2_bias_act_bwd.argtypes = [ctypes.POINTER(BiasActDesc)] + [_vp] * 6
    L.md2_bias_act_workspace_bytes.restype = ctypes.c_size_t
    L.md2_bias_act_workspace_bytes.argtypes = [ctypes.POINTER(BiasActDesc)]
    L.md2_conv_fwd.restype = ctypes.c_int
    L.md2_conv_fwd.argtypes = [ctypes.POINTER(ConvDesc)] + [_vp] * 5
    L.md2_conv_dgrad.restype = ctypes.c_int
    L.md2_conv_dgrad.argtypes = [ctypes.POINTER(ConvDesc)] + [_vp] * 5
    L.md2_conv_wgrad.restype = ctypes.c_int
    L.md2_conv_wgrad.argtypes = [ctypes.POINTER(ConvDesc)] + [_vp] * 5
    L.md2_conv_split_weights.restype = ctypes.c_int
    L.md2_conv_direct.restype = ctypes.c_int
    L.md2_conv_direct.argtypes = [ctypes.POINTER(ConvDesc)] + [_vp] * 4
    L.md2_conv_wgrad_direct.restype = ctypes.c_int
    L.md2_conv_wgrad_direct.argtypes = [ctypes.POINTER(ConvDesc)] + [_vp] * 5
    L.md2_conv_wgrad_direct_workspace_bytes.restype = ctypes.c_size_t
    L.md2_conv_wgrad_direct_workspace_bytes.argtypes = [ctypes.POINTER(ConvDesc)]
    L.md2_conv_split_weights.argtypes = [ctypes.POINTER(ConvDesc)] + [_vp] * 4
    L.md2_conv_split_weights_multi.restype = ctypes.c_int
    L.md2_conv_split_weights_multi.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp]
    L.md2_conv_bf16_weights.restype = ctypes.c_int
    L.md2_conv_bf16_weights.argtypes = [ctypes.POINTER(ConvDesc)] + [_vp] * 4
    L.md2_conv_bf16_weights_multi.restype = ctypes.c_int
    L.md2_conv_bf16_weights_multi.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp]
    L.md2_conv_workspace_bytes.restype = ctypes.c_size_t
    L.md2_conv_workspace_bytes.argtypes = [ctypes.POINTER(ConvDesc)]
    L.md2_stem_wgrad_workspace_bytes.restype = ctypes.c_size_t
    L.md2_stem_wgrad_workspace_bytes.argtypes = [ctypes.POINTER(StemDesc)]
    L.md2_stem_wgrad.restype = ctypes.c_int
    L.md2_stem_wgrad.argtypes = [ctypes.POINTER(StemDesc)] + [_vp] * 5
    L.md2_stem_fwd.restype = ctypes.c_int
    L.md2_conv_col2im.restype = ctypes.c_int
    L.md2_conv_col2im.argtypes = [ctypes.POINTER(ConvDesc)] + [_vp] * 3
    L.md2_stem_fwd.argtypes = [ctypes.POINTER(StemDesc)] + [_vp] * 4
    L.md2_disp_head_workspace_bytes.restype = ctypes.c_size_t
    L.md2_disp_head_workspace_bytes.argtypes = [ctypes.POINTER(HeadDesc)]
    L.md2_disp_head_fwd.restype = ctypes.c_int
    L.md2_disp_head_fwd.argtypes = [ctypes.POINTER(HeadDesc)] + [_vp] * 5
    L.md2_disp_head_bwd.restype = ctypes.c_int
    L.md2_disp_head_bwd.argtypes = [ctypes.POINTER(HeadDesc)] + [_vp] * 9
    L.md2_abi_version.restype = ctypes.c_int
    L.md2_abi_version.argtypes = []
    L.md2_build_id.restype = ctypes.c_char_p
    L.md2_build_id.argtypes = []
    L.md2_last_error.restype = ctypes.c_char_p
    L.md2_last_error.argtypes = []
    L.md2_workspace_bytes.restype = ctypes.c_size_t
    L.md2_workspace_bytes.argtypes = [ctypes.POINTER(Desc)]
    L.md2_select_bytes.restype = ctypes.c_size_t
    L.md2_select_bytes.argtypes = [ctypes.POINTER(Desc)]
    L.md2_photometric_fwd.restype = ctypes.c_int
    L.md2_photometric_fwd.argtypes = [ctypes.POINTER(Desc), ctypes.POINTER(Tensors), _vp, _vp, _vp, _vp]
    L.md2_photometric_bwd.restype = ctypes.c_int
    L.md2_photometric_bwd.argtypes = [ctypes.POINTER(Desc), ctypes.POINTER(Tensors), _vp, _vp,
                                      ctypes.POINTER(_vp), _vp, _vp, _vp, _vp]
    L.md2_generate_images.restype = ctypes.c_int
    L.md2_generate_images.argtypes = [ctypes.POINTER(Desc), ctypes.POINTER(Tensors),
                                      ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp]
    L.md2_tiebreak_noise.restype = ctypes.c_int
    L.md2_tiebreak_noise.argtypes = [ctypes.POINTER(Desc), _vp, ctypes.c_int, _vp, _vp]
    L.md2_decoder_pad_fwd.restype = ctypes.c_int
    L.md2_decoder_pad_fwd.argtypes = [ctypes.POINTER(PadDesc), _vp, _vp, _vp, _vp, _vp]
    L.md2_decoder_pad_bwd.restype = ctypes.c_int
    L.md2_decoder_pad_bwd.argtypes = [ctypes.POINTER(PadDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    L.md2_decoder_pad_bwd2.restype = ctypes.c_int
    L.md2_decoder_pad_bwd2.argtypes = [ctypes.POINTER(PadDesc)] + [_vp] * 9
    L.md2_encoder_input.restype = ctypes.c_int
    L.md2_encoder_input.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                    ctypes.c_float, ctypes.c_float, _vp, _vp]
    L.md2_adam_step.restype = ctypes.c_int
    L.md2_adam_step.argtypes = [_vp, _vp, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                ctypes.c_double, ctypes.c_int, _vp]
    L.md2_adam_step_dev.restype = ctypes.c_int
    L.md2_adam_step_dev.argtypes = [_vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_double, _vp, _vp, _vp]
    L.md2_adam_hyper.restype = ctypes.c_int
    L.md2_adam_hyper.argtypes = [_vp, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp]
    L.md2_adam_apply_dev.restype = ctypes.c_int
    L.md2_adam_apply_dev.argtypes = [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_double, _vp, _vp]
    L.md2_decoder_pad_workspace_bytes.restype = ctypes.c_size_t
    L.md2_decoder_pad_workspace_bytes.argtypes = [ctypes.POINTER(PadDesc)]
    L.md2_pose_fwd.restype = ctypes.c_int
    L.md2_pose_fwd.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, _vp, _vp, _vp, _vp]
    L.md2_pose_bwd.restype = ctypes.c_int
    L.md2_pose_bwd.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]
    L.md2_aug_plan_create.restype = _vp
    L.md2_aug_plan_create.argtypes = [ctypes.POINTER(AugDesc)]
    L.md2_aug_plan_destroy.restype = None
    L.md2_aug_plan_destroy.argtypes = [_vp]
    L.md2_aug_run.restype = ctypes.c_int
    L.md2_aug_run.argtypes = [_vp, _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp]
    L.md2_aug_run2.restype = ctypes.c_int
    L.md2_aug_run2.argtypes = [_vp, _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp]
    L.md2_aug_plan_create_mixed.restype = _vp
    L.md2_aug_plan_create_mixed.argtypes = [ctypes.POINTER(AugDesc), ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    L.md2_aug_run_mixed.restype = ctypes.c_int
    L.md2_aug_run_mixed.argtypes = [_vp, _vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int32),
                                    ctypes.POINTER(ctypes.c_uint64), _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                    _vp, _vp]
    L.md2_bn_workspace_bytes.restype = ctypes.c_size_t
    L.md2_bn_workspace_bytes.argtypes = [ctypes.POINTER(BnDesc)]
    L.md2_bn_fwd.restype = ctypes.c_int
    L.md2_bn_fwd.argtypes = [ctypes.POINTER(BnDesc)] + [_vp] * 11
    L.md2_bn_bwd.restype = ctypes.c_int
    L.md2_bn_bwd.argtypes = [ctypes.POINTER(BnDesc)] + [_vp] * 12
    L.md2_maxpool3s2_fwd.restype = ctypes.c_int
    L.md2_maxpool3s2_fwd.argtypes = [ctypes.POINTER(PoolDesc), _vp, _vp, _vp, _vp]
    L.md2_maxpool3s2_bwd.restype = ctypes.c_int
    L.md2_maxpool3s2_bwd.argtypes = [ctypes.POINTER(PoolDesc), _vp, _vp, _vp, _vp]
    L.md2_bn_bwd_multi.restype = ctypes.c_int
    L.md2_bn_bwd_multi.argtypes = [ctypes.POINTER(BnDesc)] + [_vp] * 14
    L.md2_bn_fwd_mask.restype = ctypes.c_int
    L.md2_bn_fwd_mask.argtypes = [ctypes.POINTER(BnDesc)] + [_vp] * 12
    L.md2_bn_bwd_mask.restype = ctypes.c_int
    L.md2_bn_bwd_mask.argtypes = [ctypes.POINTER(BnDesc)] + [_vp] * 14
    L.md2_maxpool3s2_bwd_add.restype = ctypes.c_int
    L.md2_maxpool3s2_bwd_add.argtypes = [ctypes.POINTER(PoolDesc)] + [_vp] * 5
    L.md2_maxpool3s2_bwd_multi.restype = ctypes.c_int
    L.md2_maxpool3s2_bwd_multi.argtypes = [ctypes.POINTER(PoolDesc)] + [_vp] * 6
    L.md2_timing_begin.restype = ctypes.c_int
    L.md2_timing_begin.argtypes = [ctypes.c_int]
    L.md2_timing_calls.restype = ctypes.c_int
    L.md2_timing_calls.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    L.md2_timing_end.restype = ctypes.c_int
    L.md2_timing_end.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                 ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]


def lib():
    """The loaded library; raises RuntimeError if it is not built or not loadable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_PATH} is not built. Build it with `python -m monodepth2_amd.build` "
                    "(hipcc --offload-arch=gfx950); there is no CPU fallback.")
            L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
            _declare(L)
            v = L.md2_abi_version()
            if v != ABI_VERSION:
                raise RuntimeError(f"libmd2hot ABI {v} != expected {ABI_VERSION}")
            if LIB_PATH == _BUILT_LIB:
                got, want = L.md2_build_id().decode(), source_hash()
                if got != want:
                    raise RuntimeError(
                        f"{LIB_PATH} was built from other sources (build id {got}, tree {want}): "
                        "rebuild it with `python -m monodepth2_amd.build`")
            _lib = L
    return _lib


def stream(device) -> int:
    """The raw hipStream_t of `device`'s current stream (what torch.cuda.current_stream(
    device).cuda_stream returns, without building a Stream object: ~10x cheaper on the
    host, and this is called for every kernel the step launches)."""
    idx = device.index if isinstance(device, torch.device) else device
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if idx is None else idx)


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().md2_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")


class KernelTimer:
    """Context manager around md2_timing_begin/end: average photo-kernel durations."""

    def __init__(self, max_launches: int = 4096):
        self.max_launches = max_launches
        self.fwd_ms = self.bwd_ms = 0.0
        self.n_fwd = self.n_bwd = 0

    def __enter__(self):
        check(lib().md2_timing_begin(self.max_launches), "md2_timing_begin")
        return self

    def __exit__(self, *exc):
        f, b = ctypes.c_double(), ctypes.c_double()
        nf, nb = ctypes.c_int(), ctypes.c_int()
        check(lib().md2_timing_end(ctypes.byref(f), ctypes.byref(nf), ctypes.byref(b), ctypes.byref(nb)),
              "md2_timing_end")
        self.fwd_ms, self.n_fwd, self.bwd_ms, self.n_bwd = f.value, nf.value, b.value, nb.value
        check(lib().md2_timing_calls(ctypes.byref(f), ctypes.byref(nf), ctypes.byref(b), ctypes.byref(nb)),
              "md2_timing_calls")
        self.fwd_call_ms, self.n_fwd_call, self.bwd_call_ms, self.n_bwd_call = f.value, nf.value, b.value, nb.value
        return False
