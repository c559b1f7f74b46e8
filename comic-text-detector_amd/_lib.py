"""ctypes binding of libctd_hip.so (C ABI in include/ctd_hip.h).

The product path has NO CPU fallback: if the HIP library is missing, or cannot
be loaded, importing a symbol from here raises.  `build()` compiles it in-tree.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libctd_hip.so")
SELFTEST_PATH = os.path.join(_HERE, "ctd_selftest")

# ---- constants mirrored from include/ctd_hip.h -------------------------------
ABI_VERSION = 10
OK = 0
PREC_F32, PREC_F16, PREC_F32S = 0, 1, 2
ACT = {"none": 0, "silu": 1, "leaky": 2, "relu": 3, "sigmoid": 4}
IN_NCHW_F32, IN_NHWC_U8 = 0, 1
(OP_INPUT, OP_CONV, OP_CONVT, OP_MAXPOOL, OP_AVGPOOL2, OP_DETECT, OP_EXPORT, OP_STEM, OP_SEG_FINAL,
 OP_DB_UP) = range(1, 11)
OUT_MASK, OUT_LINES = 0, 1
REGION_OK, REGION_DEGENERATE, REGION_MAX_SIDE, REGION_TILE = 0, 1, 32766, 1024
REGION_U8, REGION_F16, REGION_F32 = 0, 1, 2
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1
COLOR_OK, COLOR_EMPTY, COLOR_NO_MASK, COLOR_NO_CONTRAST, COLOR_TOO_LARGE = range(5)
COLOR_MAX_PIXELS, COLOR_MAX_COORD = 1 << 24, 1 << 29
ERASE_PLAIN, ERASE_TEXTURED, ERASE_NO_RING, ERASE_NO_MASK, ERASE_EMPTY, ERASE_TOO_LARGE = range(6)
ERASE_MAX_PIXELS, ERASE_MAX_COORD, ERASE_MAX_GROW, ERASE_MAX_RING = 1 << 24, 1 << 29, 8, 16
ERASE_TILE_W, ERASE_TILE_H = 64, 32
BALLOON_OK, BALLOON_NOT_PLAIN, BALLOON_TOO_LARGE = range(3)
BALLOON_MAX_WORDS, BALLOON_MAX_REACH, BALLOON_MIN_REACH_MIN, BALLOON_MAX_REACH_MIN = 8192, 32, 8, 1024
BALLOON_CUT_LEFT, BALLOON_CUT_TOP, BALLOON_CUT_RIGHT, BALLOON_CUT_BOTTOM = 1, 2, 4, 8
BALLOON_FOOTPRINT, FOOTPRINT_MAX_PAD, FOOTPRINT_DEFAULT_PAD = 256, 16, 4
BALLOON_TILTED = 512
FILL_OK, FILL_NO_HOLE, FILL_NO_KNOWN = range(3)
FILL_MAX_SIDE, FILL_TILE = 8192, 64
TEXTURE_OK, TEXTURE_NO_HOLE, TEXTURE_NO_SOURCE = range(3)
TEXTURE_PATCH, TEXTURE_MAX_RADIUS, TEXTURE_MAX_SIDE, TEXTURE_TILE = 7, 127, 8192, 64
LAYOUT_OK, LAYOUT_NO_REGION, LAYOUT_EMPTY = range(3)
LAYOUT_MAX_INSET = 16
FIT_OK, FIT_NO_REGION, FIT_NO_TEXT, FIT_NO_ANCHOR, FIT_NO_FIT = range(5)
FIT_MAX_CANDS, FIT_MAX_LINES, FIT_MAX_GLYPHS = 16, 32, 4096
TYPESET_MAX_SIDE, TYPESET_MAX_RADIUS, TYPESET_TILE_W, TYPESET_TILE_H = 8192, 12, 64, 32
TYPESET_OK, TYPESET_EMPTY, TYPESET_OUTSIDE = range(3)          # typeset.typeset_tables' status column (not part of the ABI)
RASTER_MAX_SIDE, RASTER_MAX_SCALE = 1024, 1 << 22
RASTER_OK, RASTER_EMPTY, RASTER_REFUSED = range(3)
# the shape of the raster launch (csrc/kernels.h RS_*; not part of the ABI, no result depends on it): pixel rows a band, pixel
# columns a chunk, segments a staging pass, workgroups a job.  The tests put sizes on both sides of each.
RASTER_BAND_H, RASTER_CHUNK_W, RASTER_SEG_CHUNK, RASTER_BANDS_Y = 4, 128, 32, 8


class CtdTensor(C.Structure):
    _fields_ = [("channels", C.c_int32), ("log2_down", C.c_int32), ("dtype", C.c_int32)]


class CtdOp(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("src0", C.c_int32), ("src0_coff", C.c_int32), ("src0_c", C.c_int32), ("src0_up", C.c_int32),
        ("src1", C.c_int32), ("src1_coff", C.c_int32), ("src1_c", C.c_int32), ("src1_up", C.c_int32),
        ("res", C.c_int32), ("res_coff", C.c_int32),
        ("dst", C.c_int32), ("dst_coff", C.c_int32),
        ("cout", C.c_int32),
        ("k", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
        ("act", C.c_int32),
        ("w_off", C.c_int64), ("b_off", C.c_int64),
        ("aux", C.c_int32 * 8),
        ("faux", C.c_float * 8),
    ]


class CtdTailPage(C.Structure):
    _fields_ = [("img_dev", C.c_void_p), ("im_h", C.c_int32), ("im_w", C.c_int32), ("dw", C.c_int32), ("dh", C.c_int32)]


class CtdTailParams(C.Structure):
    _fields_ = [("conf_thresh", C.c_float), ("nms_thresh", C.c_float), ("box_thresh", C.c_float),
                ("max_candidates", C.c_int32), ("unclip_ratio", C.c_double), ("refine", C.c_int32),
                ("refine_mode", C.c_int32), ("keep_undetected_mask", C.c_int32), ("pad_", C.c_int32)]


class CtdBlk(C.Structure):
    _fields_ = [("xyxy", C.c_int32 * 4), ("language", C.c_int32), ("vertical", C.c_int32), ("angle", C.c_int32),
                ("font_is_float", C.c_int32), ("font_size", C.c_double), ("vec", C.c_double * 2), ("norm", C.c_double),
                ("weight", C.c_double), ("merged", C.c_int32), ("line_off", C.c_int32), ("n_lines", C.c_int32),
                ("dist_off", C.c_int32), ("n_dist", C.c_int32), ("pad_", C.c_int32)]


class CtdTraceWin(C.Structure):
    _fields_ = [("page", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("pass_", C.c_int32), ("path", C.c_int32), ("n_cand", C.c_int32), ("hist", C.c_uint32 * 1024),
                ("rules", C.c_int32 * 18), ("cand_rule", C.c_int32 * 4), ("cand_invert", C.c_int32 * 4),
                ("sums", C.c_uint64 * 6), ("cand_dist", C.c_uint64 * 4)]


class CtdRegionJob(C.Structure):
    _fields_ = [("page_dev", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("pitch", C.c_int32),
                ("Minv", C.c_double * 9), ("w", C.c_int32), ("h", C.c_int32), ("rotate", C.c_int32), ("pad_", C.c_int32),
                ("out_off", C.c_int64)]


class CtdRegionBatchJob(C.Structure):
    _fields_ = [("warp", CtdRegionJob), ("slot", C.c_int32), ("rows", C.c_int32), ("Wk", C.c_int32), ("cut", C.c_int32)]


class CtdColorJob(C.Structure):
    _fields_ = [("page_dev", C.c_void_p), ("mask_dev", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32),
                ("mask_pitch", C.c_int32), ("quad", C.c_int32 * 8)]


class CtdLineColor(C.Structure):
    _fields_ = [("n_fg", C.c_int64), ("s_fg", C.c_int64 * 3), ("n_bg", C.c_int64), ("s_bg", C.c_int64 * 3),
                ("g_on", C.c_int64), ("g_off", C.c_int64), ("n_on", C.c_int32), ("n_off", C.c_int32), ("status", C.c_int32),
                ("fg", C.c_uint8 * 3), ("bg", C.c_uint8 * 3), ("pad_", C.c_uint8 * 6)]


class CtdEraseJob(C.Structure):
    _fields_ = [("page", C.c_int32), ("xyxy", C.c_int32 * 4), ("pad_", C.c_int32 * 3)]


class CtdErasePage(C.Structure):
    _fields_ = [("page_dev", C.c_void_p), ("mask_dev", C.c_void_p), ("out_dev", C.c_void_p), ("rest_dev", C.c_void_p),
                ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32), ("mask_pitch", C.c_int32), ("out_pitch", C.c_int32),
                ("rest_pitch", C.c_int32), ("block0", C.c_int32), ("n_blocks", C.c_int32), ("tile0", C.c_int32),
                ("pad_", C.c_int32)]


class CtdEraseParams(C.Structure):
    _fields_ = [("grow", C.c_int32), ("ring", C.c_int32), ("tol", C.c_int32), ("min_ring", C.c_int32), ("n_tiles", C.c_int32),
                ("pad_", C.c_int32 * 3)]


class CtdEraseRow(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_fill", C.c_int32), ("n_ring", C.c_int32), ("cnt", C.c_int32 * 3),
                ("med", C.c_uint8 * 3), ("pad_", C.c_uint8 * 5)]


class CtdBalloonJob(C.Structure):
    _fields_ = [("page", C.c_int32), ("xyxy", C.c_int32 * 4), ("erase_row", C.c_int32), ("word0", C.c_int64)]


class CtdBalloonParams(C.Structure):
    _fields_ = [("grow", C.c_int32), ("tol", C.c_int32), ("reach", C.c_int32), ("reach_min", C.c_int32), ("max_words", C.c_int32),
                ("pad_", C.c_int32 * 3)]


class CtdBalloonRow(C.Structure):
    _fields_ = [("status", C.c_int32), ("area", C.c_int32), ("bbox", C.c_int32 * 4), ("flags", C.c_int32), ("n_seed", C.c_int32),
                ("sum_x", C.c_int64), ("sum_y", C.c_int64)]


class CtdFootprintParams(C.Structure):
    _fields_ = [("grow", C.c_int32), ("pad", C.c_int32), ("reach", C.c_int32), ("reach_min", C.c_int32), ("max_words", C.c_int32),
                ("pad_", C.c_int32 * 3)]


class CtdTiltJob(C.Structure):
    _fields_ = [("win", C.c_int32 * 4), ("ax", C.c_int32), ("ay", C.c_int32), ("c", C.c_int32), ("s", C.c_int32),
                ("W", C.c_int32), ("H", C.c_int32), ("word0", C.c_int64)]


class CtdTiltParams(C.Structure):
    _fields_ = [("max_words", C.c_int32), ("pad_", C.c_int32 * 3)]


class CtdLayoutJob(C.Structure):
    _fields_ = [("win", C.c_int32 * 4), ("ax", C.c_int32), ("ay", C.c_int32), ("word0", C.c_int64)]


class CtdLayoutParams(C.Structure):
    _fields_ = [("inset", C.c_int32), ("max_words", C.c_int32), ("n_rows", C.c_int32), ("pad_", C.c_int32)]


class CtdLayoutRow(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_inner", C.c_int32), ("area", C.c_int32), ("rect", C.c_int32 * 4),
                ("a_area", C.c_int32), ("a_rect", C.c_int32 * 4)]


class CtdFitJob(C.Structure):
    _fields_ = [("n_glyphs", C.c_int32), ("n_cands", C.c_int32), ("cand0", C.c_int32), ("pad_", C.c_int32), ("break0", C.c_int64)]


class CtdFitCand(C.Structure):
    _fields_ = [("line", C.c_int32), ("gap", C.c_int32), ("cum0", C.c_int64)]


class CtdFitParams(C.Structure):
    _fields_ = [("inset", C.c_int32), ("max_words", C.c_int32), ("n_rows", C.c_int32), ("n_cands", C.c_int32),
                ("n_cum", C.c_int64), ("n_breaks", C.c_int64)]


class CtdFitLine(C.Structure):
    _fields_ = [("start", C.c_int32), ("x1", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("length", C.c_int32)]


class CtdFitRow(C.Structure):
    _fields_ = [("status", C.c_int32), ("cand", C.c_int32), ("n_lines", C.c_int32), ("n_inner", C.c_int32),
                ("lines", CtdFitLine * 32)]


class CtdFitBalance(C.Structure):
    _fields_ = [("balanced", C.c_int32), ("pad_", C.c_int32), ("cost", C.c_int64)]


class CtdTypesetPage(C.Structure):
    _fields_ = [("page_dev", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int64)]


class CtdTypesetLayer(C.Structure):
    _fields_ = [("cov0", C.c_int64), ("page", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("cov_pitch", C.c_int32), ("clip", C.c_int32 * 4), ("fill", C.c_uint8 * 3), ("stroke", C.c_uint8 * 3),
                ("radius", C.c_uint8), ("pad_", C.c_uint8)]


class CtdTypesetTile(C.Structure):
    _fields_ = [("page", C.c_int32), ("tx", C.c_int32), ("ty", C.c_int32), ("first", C.c_int32)]


class CtdTypesetParams(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("n_pages", C.c_int32), ("n_tiles", C.c_int32), ("n_entries", C.c_int32),
                ("cov_bytes", C.c_int64), ("pad_", C.c_int64)]


class CtdTypesetRow(C.Structure):
    _fields_ = [("n_fill", C.c_int32), ("n_stroke", C.c_int32)]


class CtdGlyphLayer(C.Structure):
    _fields_ = [("page", C.c_int32), ("clip", C.c_int32 * 4), ("fill", C.c_uint8 * 3), ("stroke", C.c_uint8 * 3),
                ("radius", C.c_uint8), ("pad_", C.c_uint8), ("pad2_", C.c_int32)]


class CtdTiltLayer(C.Structure):
    _fields_ = [("page", C.c_int32), ("clip", C.c_int32 * 4), ("fill", C.c_uint8 * 3), ("stroke", C.c_uint8 * 3),
                ("radius", C.c_uint8), ("pad_", C.c_uint8), ("ax", C.c_int32), ("ay", C.c_int32), ("c", C.c_int32),
                ("s", C.c_int32), ("pad2_", C.c_int32)]


class CtdGlyphPlace(C.Structure):
    _fields_ = [("layer", C.c_int32), ("glyph", C.c_int32), ("x", C.c_int32), ("y", C.c_int32)]


class CtdGlyphRecord(C.Structure):
    _fields_ = [("off", C.c_int64), ("w", C.c_int32), ("h", C.c_int32)]


class CtdGlyphParams(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("n_pages", C.c_int32), ("n_tiles", C.c_int32), ("n_entries", C.c_int32),
                ("n_places", C.c_int32), ("n_glyphs", C.c_int32), ("atlas_bytes", C.c_int64)]


class CtdRasterJob(C.Structure):
    _fields_ = [("off", C.c_int64), ("w", C.c_int32), ("h", C.c_int32), ("bx", C.c_int32), ("by", C.c_int32),
                ("seg_first", C.c_int32), ("seg_count", C.c_int32), ("scale", C.c_int32), ("pad_", C.c_int32)]


class CtdFillPage(C.Structure):
    _fields_ = [("page_dev", C.c_void_p), ("hole_dev", C.c_void_p), ("out_dev", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32),
                ("pitch", C.c_int32), ("hole_pitch", C.c_int32), ("out_pitch", C.c_int32), ("tile0", C.c_int32),
                ("lvl0", C.c_int64)]


class CtdFillParams(C.Structure):
    _fields_ = [("n_tiles", C.c_int32), ("pad_", C.c_int32 * 7)]


class CtdFillRow(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_hole", C.c_int32), ("levels", C.c_int32), ("top", C.c_uint8 * 3),
                ("pad_", C.c_uint8 * 17)]


class CtdTexturePage(C.Structure):
    _fields_ = [("page_dev", C.c_void_p), ("hole_dev", C.c_void_p), ("init_dev", C.c_void_p), ("out_dev", C.c_void_p),
                ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32), ("hole_pitch", C.c_int32), ("init_pitch", C.c_int32),
                ("out_pitch", C.c_int32), ("tile0", C.c_int32), ("pad_", C.c_int32), ("fld0", C.c_int64), ("cls0", C.c_int64)]


class CtdTextureParams(C.Structure):
    _fields_ = [("n_tiles", C.c_int32), ("radius", C.c_int32), ("n_em", C.c_int32), ("n_sweep", C.c_int32), ("n_init", C.c_int32),
                ("seed", C.c_uint32), ("scratch_bytes", C.c_int64)]


class CtdTextureRow(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_hole", C.c_int32), ("n_target", C.c_int32), ("n_source", C.c_int32),
                ("n_unmatched", C.c_int32), ("pad_", C.c_int32 * 3)]


# every symbol include/ctd_hip.h declares: (restype, argtypes)
_vp, _i32, _i64, _f = C.c_void_p, C.c_int32, C.c_int64, C.c_float
SYMBOLS = {
    "ctd_engine_create": (_i32, [C.POINTER(_vp), C.POINTER(CtdTensor), _i32, C.POINTER(CtdOp), _i32,
                                 C.POINTER(C.c_float), _i64, _i32, _i32]),
    "ctd_engine_destroy": (None, [_vp]),
    "ctd_engine_blks_shape": (_i32, [_vp, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "ctd_engine_forward": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctd_engine_n_ops": (_i32, [_vp]),
    "ctd_engine_op_work": (_i32, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i32)]),
    "ctd_engine_op_kernel": (_i32, [_vp, _i32, C.c_char_p, _i32]),
    "ctd_engine_profile": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                  C.POINTER(C.c_float)]),
    "ctd_engine_read_tensor": (_i32, [_vp, _i32, C.POINTER(C.c_float), _i64]),
    "ctd_engine_workspace_bytes": (_i64, [_vp]),
    "ctd_engine_arena_generation": (_i32, [_vp]),
    "ctd_tuning_set": (_i32, [C.c_char_p, C.c_int64]),
    "ctd_tuning_get": (_i32, [C.c_char_p, C.POINTER(C.c_int64)]),
    "ctd_nms_workspace_bytes": (C.c_size_t, [_i32, _i32]),
    "ctd_nms": (_i32, [_vp, _i32, _i32, _i32, _f, _f, _i32, _i32, _f, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ctd_db_step": (_i32, [_vp, _i32, _i32, _i32, _f, _vp, _vp, _f, _vp]),
    "ctd_ccl_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "ctd_ccl": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, C.c_size_t, _vp]),
    "ctd_ccl_dual": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, C.c_size_t, _vp]),
    "ctd_resize_linear_u8": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp]),
    "ctd_region_transforms": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_double, _vp, _vp, _vp, _vp]),
    "ctd_warp_regions": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp]),
    "ctd_warp_region_batches": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "ctd_line_colors": (_i32, [_vp, _i32, _vp, _vp]),
    "ctd_erase_text": (_i32, [_vp, _i32, _vp, _i32, C.POINTER(CtdEraseParams), _vp, _vp]),
    "ctd_balloon_regions": (_i32, [_vp, _i32, _vp, _i32, _vp, C.POINTER(CtdBalloonParams), _vp, _vp, _vp]),
    "ctd_balloon_footprints": (_i32, [_vp, _i32, _vp, _i32, _vp, C.POINTER(CtdFootprintParams), _vp, _vp, _vp]),
    "ctd_balloon_tilt": (_i32, [_vp, _i32, _vp, _vp, C.POINTER(CtdTiltParams), _vp, _vp, _vp]),
    "ctd_layout_boxes": (_i32, [_vp, _i32, _vp, _vp, C.POINTER(CtdLayoutParams), _vp, _vp]),
    "ctd_layout_fit": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(CtdFitParams), _vp, _vp]),
    "ctd_layout_fit_work_bytes": (C.c_int64, [_vp, _i32]),
    "ctd_layout_fit_balanced": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(CtdFitParams), _vp, _vp, _vp, C.c_int64,
                                       _vp]),
    "ctd_typeset": (_i32, [_vp, _vp, _vp, _vp, _vp, C.POINTER(CtdTypesetParams), _vp, _vp]),
    "ctd_typeset_glyphs": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(CtdGlyphParams), _vp, _vp]),
    "ctd_typeset_tilted": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(CtdGlyphParams), _vp, _vp]),
    "ctd_rasterise_glyphs": (_i32, [_vp, _i64, _vp, _i32, _vp, _i64, _vp, _vp]),
    "ctd_fill_rest": (_i32, [_vp, _i32, C.POINTER(CtdFillParams), _vp, _vp, _vp]),
    "ctd_texture_fill": (_i32, [_vp, _i32, C.POINTER(CtdTextureParams), _vp, _vp, _vp]),
    "ctd_db_boxes": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, _vp, _vp, C.POINTER(_i32)]),
    "ctd_tail_create": (_i32, [C.POINTER(_vp), _i32]),
    "ctd_tail_destroy": (None, [_vp]),
    "ctd_tail_stream": (_vp, [_vp]),
    "ctd_tail_run": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _i64, _vp, C.POINTER(CtdTailPage),
                            C.POINTER(CtdTailParams), _vp, _vp, _vp]),
    "ctd_tail_timings": (_i32, [_vp, C.POINTER(C.c_double)]),
    "ctd_tail_refine_paths": (_i32, [_vp, C.POINTER(_i32)]),
    "ctd_tail_db_boxes": (_i32, [_vp, _i32, _i32, _i32, _vp, _i64, _vp, _i32, C.c_double]),
    "ctd_tail_refine": (_i32, [_vp, _i32, C.POINTER(CtdTailPage), _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "ctd_tail_page_counts": (_i32, [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32),
                                    C.POINTER(_i32)]),
    "ctd_tail_page_fetch": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctd_tail_batch_counts": (_i32, [_vp, _vp]),
    "ctd_tail_batch_fetch": (_i32, [_vp, _vp, _vp, _vp]),
    "ctd_tail_pack_records": (_i32, [_vp, _i32, _i32, _vp]),
    "ctd_tail_set_threads": (_i32, [_vp, _i32]),
    "ctd_tail_set_trace": (_i32, [_vp, _i32]),
    "ctd_tail_trace_counts": (_i32, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "ctd_tail_trace_windows": (_i32, [_vp, _vp]),
    "ctd_tail_trace_lds_launches": (_i32, [_vp, C.POINTER(_i32), _vp]),
    "ctd_tail_trace_db_sizes": (_i32, [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "ctd_tail_trace_db_fetch": (_i32, [_vp, _i32, _vp, _vp]),
    "ctd_db_boxes_compact": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _i32, C.c_double, _vp, _vp, C.POINTER(_i32)]),
    "ctd_topk_colors": (_i32, [_vp, _vp]),
    "ctd_otsu_from_hist": (_i32, [_vp]),
    "ctd_inrange_bounds": (None, [C.c_double, C.c_double, C.POINTER(_i32), C.POINTER(_i32)]),
    "ctd_group_output": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32,
                                C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "ctd_host_gather": (_i32, [_vp, _vp, _vp, _i32, _i32]),
    "ctd_last_error": (C.c_char_p, []),
    "ctd_abi_version": (_i32, []),
    "ctd_device_info": (_i32, [_i32, C.c_char_p, C.POINTER(_i32), C.POINTER(_i64)]),
}


class CtdError(RuntimeError):
    pass


def build(verbose: bool = False) -> None:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    import sys
    r = subprocess.run(["make", "-C", src, "-j8", f"PYTHON={sys.executable}"], capture_output=True, text=True)
    if r.returncode != 0:
        raise CtdError("building libctd_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout[-2000:])


_lib = None


def lib() -> C.CDLL:
    """Loads libctd_hip.so (loudly failing if absent) and types every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise CtdError(f"{LIB_PATH} is missing: the HIP extension was not built "
                       "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
                       "There is no CPU fallback for the product path.")
    # torch ships its own libamdhip64.so (same SONAME as /opt/rocm's).  Import it
    # first so the process has ONE HIP runtime: streams and device pointers made by
    # torch are then valid in this library.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)       # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if L.ctd_abi_version() != ABI_VERSION:
        raise CtdError("libctd_hip.so ABI version mismatch; rebuild")
    _lib = L
    _apply_env_tuning(L)
    return L


# The library reads no environment variables; dispatch knobs go through `ctd_tuning_set`.  For A/B runs of unchanged
# scripts the host side applies CTD_TUNING="key=value,key=value" once at load time (and the older per-knob names).
_LEGACY_ENV = {"CTD_FUSE": "fuse", "CTD_NO_REUSE": "no_reuse", "CTD_F32_MFMA": "f32_mfma", "CTD_HALO_PAIR": "halo_pair",
               "CTD_HALO_MIN_PATCHES": "halo_min_patches", "CTD_DBUP_MFMA": "db_up_mfma", "CTD_SEGFINAL_MFMA": "seg_final_mfma"}


def _apply_env_tuning(L) -> None:
    items = []
    for env, key in _LEGACY_ENV.items():
        if env in os.environ:
            v = os.environ[env]
            items.append((key, 1 if (env == "CTD_NO_REUSE" and not v.lstrip("-").isdigit()) else int(v)))
    for part in os.environ.get("CTD_TUNING", "").split(","):
        if "=" in part:
            k, v = part.split("=", 1)
            items.append((k.strip(), int(v)))
    for k, v in items:
        if L.ctd_tuning_set(k.encode(), v) != OK:
            raise CtdError(f"unknown tuning key {k!r} (CTD_TUNING / legacy environment knob)")


def check(rc: int, what: str = "") -> None:
    if rc != OK:
        msg = lib().ctd_last_error().decode("utf8", "replace")
        raise CtdError(f"{what} failed (rc={rc}): {msg}")


def tuning_get(key: str) -> int:
    """The value the library holds for a tuning key (the rows of csrc/tuning.def)."""
    v = C.c_int64()
    check(lib().ctd_tuning_get(key.encode(), C.byref(v)), f"ctd_tuning_get({key!r})")
    return v.value


@contextlib.contextmanager
def tuning(keys=None, **more):
    """`with tuning(halo_min_patches=1, fuse=0):` (or a dict) -- sets the keys in the order given and, on the way out, puts
    back what each one held on the way in, last set first, also when the body raises.  What was there is read from the
    library, so a value that CTD_TUNING set at load time survives.  Every key is read before any is set: an unknown one
    raises CtdError with nothing changed."""
    keys = {**(keys or {}), **more}
    held = [(k, tuning_get(k)) for k in keys]
    done = []
    try:
        for (k, old), v in zip(held, keys.values()):
            check(lib().ctd_tuning_set(k.encode(), int(v)), f"ctd_tuning_set({k!r})")
            done.append((k, old))
        yield
    finally:
        for k, old in reversed(done):
            check(lib().ctd_tuning_set(k.encode(), old), f"ctd_tuning_set({k!r})")
