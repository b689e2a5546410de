"""ctypes binding of include/fr_raster.h (libfr_raster.so).

Loading fails loudly: there is no Python / CPU implementation to fall back to."""
from __future__ import annotations

import ctypes as C
import os

FR_WINDING_I16, FR_GRAY_DEBUG, FR_MASK_NONZERO, FR_COVERAGE_U8, FR_SDF_U8 = 0, 1, 2, 3, 4
FR_SAMPLE_CORNER, FR_SAMPLE_CENTER = 0, 1
FR_FILL_CONSISTENT = 1           # crossing-rule flag of the _ex entry points (include/fr_raster.h)
FR_TEXT_SRGB, FR_TEXT_BGRA = 8, 4  # flags of fr_text_plan_create_rgba only: linear-light blending, B G R A output
FR_TEXT_LOAD = 32                  # fr_text_plan_create_rgba only: draw over the pixels already in the output
FR_TEXT_CACHE = 128                # the upright and _ex text plans: each distinct glyph image made once per render, same bytes
FR_TEXT_OVER = 256                 # the RGBA text plans: source-over alpha (a premultiplied output) instead of alpha replaced
FR_TEXT_CACHE_AFFINE = 512         # the matrix-form text plans: FR_TEXT_CACHE keyed by (glyph, pen fractions, bits of m), same bytes
FR_LAYER_SRGB = 1              # the flag space of the fr_layer_over / _shadow / _rects / _paint calls: work in linear light
FR_LCD_BGR = 2                     # fr_layer_lcd alone, beside FR_LAYER_SRGB: memory byte b takes sub-pixel 2 - b
FR_LCD_TAPS = 5                    # the length of fr_layer_lcd's filter
FR_MASK_PLANE, FR_MASK_ERASE = 4, 8    # fr_layer_mask alone: the mask is a plane of bytes; no layer, the destination is erased
# fr_layer_blend's modes; FR_BLEND_MODES is their number
(FR_BLEND_MULTIPLY, FR_BLEND_SCREEN, FR_BLEND_OVERLAY, FR_BLEND_DARKEN, FR_BLEND_LIGHTEN, FR_BLEND_HARD_LIGHT, FR_BLEND_DIFFERENCE, FR_BLEND_EXCLUSION,
 FR_BLEND_PLUS, FR_BLEND_MODES) = range(10)
FR_OUTLINE_GROW, FR_OUTLINE_RING, FR_OUTLINE_INNER, FR_OUTLINE_SHRINK = 0, 1, 2, 3      # fr_layer_outline_params.kind
FR_OUTLINE_MAX_RADIUS = 256        # fr_layer_outline_params.radius, in 1/16 pixel
FR_GRADIENT_LINEAR, FR_GRADIENT_RADIAL = 0, 1                   # fr_layer_paint_params.kind
FR_SPREAD_PAD, FR_SPREAD_REPEAT, FR_SPREAD_REFLECT = 0, 1, 2    # fr_layer_paint_params.spread
FR_GRADIENT_MAX_STOPS = 8
FR_DECOR_UNDERLINE, FR_DECOR_STRIKEOUT, FR_DECOR_LINE_BOX = 0, 1, 2    # the kinds of fr_text_decoration

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path() -> str:
    # FR_RASTER_LIB: experiment builds only (make ablate4 / make variant); the product is libfr_raster.so
    return os.environ.get("FR_RASTER_LIB") or os.path.join(_HERE, "libfr_raster.so")


class FrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"fr_raster error {code}: {msg}")
        self.code = code


class Job(C.Structure):          # == fr_job
    _fields_ = [("glyph", C.c_uint32), ("min_x", C.c_int32), ("max_y", C.c_int32),
                ("w", C.c_uint32), ("h", C.c_uint32), ("out_x", C.c_uint32), ("out_y", C.c_uint32),
                ("scale", C.c_float)]


class RasterParams(C.Structure):  # == fr_raster_params
    _fields_ = [("mode", C.c_int32), ("samples_per_axis", C.c_int32), ("sample_phase", C.c_int32),
                ("reserved", C.c_int32)]


class GlyphPlace(C.Structure):   # == fr_glyph_place
    _fields_ = [("glyph", C.c_uint32), ("pen_x64", C.c_int32), ("pen_y", C.c_int32)]


class GlyphPlaceEx(C.Structure):  # == fr_glyph_place_ex
    _fields_ = [("glyph", C.c_uint32), ("pen_x64", C.c_int32), ("pen_y64", C.c_int32), ("scale", C.c_float),
                ("slant", C.c_float)]


class GlyphPlaceAffine(C.Structure):  # == fr_glyph_place_affine
    _fields_ = [("glyph", C.c_uint32), ("pen_x64", C.c_int32), ("pen_y64", C.c_int32), ("m", C.c_float * 4)]


class TextRun(C.Structure):      # == fr_text_run
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("out_x", C.c_uint32), ("out_y", C.c_uint32), ("scale", C.c_float)]


class LayerBlit(C.Structure):    # == fr_layer_blit
    _fields_ = [("src_x", C.c_uint32), ("src_y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("opacity", C.c_uint32)]


class LayerMaskBlit(C.Structure):    # == fr_layer_mask_blit
    _fields_ = [("src_x", C.c_uint32), ("src_y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("mask_x", C.c_uint32), ("mask_y", C.c_uint32),
                ("opacity", C.c_uint32), ("invert", C.c_uint32)]


class LcdBlit(C.Structure):      # == fr_lcd_blit
    _fields_ = [("src_x", C.c_uint32), ("src_y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("rgba", C.c_uint8 * 4)]


class LayerShadowParams(C.Structure):    # == fr_layer_shadow_params
    _fields_ = [("src_x", C.c_uint32), ("src_y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("dst_x", C.c_uint32), ("dst_y", C.c_uint32), ("dst_w", C.c_uint32), ("dst_h", C.c_uint32),
                ("dx", C.c_int32), ("dy", C.c_int32), ("spread", C.c_uint32), ("blur_radius", C.c_uint32),
                ("blur_passes", C.c_uint32), ("rgba", C.c_uint8 * 4)]


class LayerOutlineParams(C.Structure):   # == fr_layer_outline_params
    _fields_ = [("src_x", C.c_uint32), ("src_y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("dst_x", C.c_uint32), ("dst_y", C.c_uint32), ("dst_w", C.c_uint32), ("dst_h", C.c_uint32),
                ("dx", C.c_int32), ("dy", C.c_int32), ("radius", C.c_uint32), ("kind", C.c_uint32), ("rgba", C.c_uint8 * 4)]


class LayerWarpBlit(C.Structure):    # == fr_layer_warp_blit (72 bytes)
    _fields_ = [("src_x", C.c_uint32), ("src_y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("dst_w", C.c_uint32), ("dst_h", C.c_uint32),
                ("u0", C.c_int64), ("v0", C.c_int64), ("ux", C.c_int32), ("uy", C.c_int32), ("vx", C.c_int32), ("vy", C.c_int32),
                ("opacity", C.c_uint32), ("reserved", C.c_uint32)]


class LayerRect(C.Structure):    # == fr_layer_rect
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("rgba", C.c_uint8 * 4)]


class GradientStop(C.Structure):  # == fr_gradient_stop
    _fields_ = [("offset", C.c_uint32), ("rgba", C.c_uint8 * 4)]


class LayerPaintParams(C.Structure):     # == fr_layer_paint_params
    _fields_ = [("src_x", C.c_uint32), ("src_y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("kind", C.c_uint32), ("spread", C.c_uint32),
                ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
                ("n_stops", C.c_uint32), ("stops", GradientStop * FR_GRADIENT_MAX_STOPS)]


class FontLine(C.Structure):     # == fr_font_line
    _fields_ = [("ascender", C.c_int16), ("descender", C.c_int16), ("line_gap", C.c_int16),
                ("underline_position", C.c_int16), ("underline_thickness", C.c_int16),
                ("strikeout_size", C.c_int16), ("strikeout_position", C.c_int16), ("present", C.c_uint16)]


# every symbol include/fr_raster.h declares: (name, restype, argtypes)
_P = C.c_void_p
_I16P, _U32P, _U8P = C.POINTER(C.c_int16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
SYMBOLS = [
    ("fr_abi_version", C.c_int, []),
    ("fr_last_error", C.c_char_p, []),
    ("fr_build_id", C.c_char_p, []),
    ("fr_ctx_create", C.c_int, [C.c_int, _P, C.POINTER(_P)]),
    ("fr_ctx_destroy", None, [_P]),
    ("fr_ctx_sync", C.c_int, [_P]),
    ("fr_ctx_set_option", C.c_int, [_P, C.c_char_p, C.c_int64]),
    ("fr_glyphset_create", C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(_P)]),
    ("fr_glyphset_destroy", None, [_P]),
    ("fr_glyphset_prepare", C.c_int, [_P]),
    ("fr_glyphset_stats", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("fr_glyphset_set_boxes", C.c_int, [_P, _P]),
    ("fr_plan_create", C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(RasterParams), C.POINTER(_P)]),
    ("fr_plan_create_ex", C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(RasterParams), C.c_uint32, C.POINTER(_P)]),
    ("fr_plan_destroy", None, [_P]),
    ("fr_plan_render", C.c_int, [_P, _P, C.c_size_t, C.c_size_t]),
    ("fr_plan_render_timed", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.POINTER(C.c_float)]),
    ("fr_plan_pixels", C.c_uint64, [_P]),
    ("fr_plan_stats", C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("fr_plan_describe", C.c_int, [_P, C.c_char_p, C.c_size_t]),
    ("fr_text_plan_create", C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(RasterParams), C.c_uint32,
                                      C.POINTER(_P)]),
    ("fr_text_plan_create_rgba", C.c_int, [_P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.POINTER(RasterParams),
                                           C.c_uint32, C.POINTER(_P)]),
    ("fr_text_plan_create_ex", C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(RasterParams), C.c_uint32,
                                         C.POINTER(_P)]),
    ("fr_text_plan_create_rgba_ex", C.c_int, [_P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.POINTER(RasterParams),
                                              C.c_uint32, C.POINTER(_P)]),
    ("fr_text_plan_create_affine", C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(RasterParams), C.c_uint32,
                                             C.POINTER(_P)]),
    ("fr_text_plan_create_rgba_affine", C.c_int, [_P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.POINTER(RasterParams),
                                                  C.c_uint32, C.POINTER(_P)]),
    ("fr_allgather_bands", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("fr_gather_bands", C.c_int, [_P, _P, _P, C.c_size_t, C.c_int]),
    ("fr_render_batch", C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(RasterParams), _P, C.c_size_t, C.c_size_t]),
    ("fr_render_batch_ex", C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(RasterParams), C.c_uint32, _P, C.c_size_t, C.c_size_t]),
    ("fr_render_glyph_dims", C.c_int, [_P, C.c_uint16, C.c_uint16, _P, _P, C.POINTER(C.c_uint16),
                                       C.POINTER(C.c_uint16), C.POINTER(C.c_float)]),
    ("fr_render_glyph", C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint16, C.c_uint16, C.c_int32, _P]),
    ("fr_render_glyph_ex", C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint16, C.c_uint16, C.c_int32, C.c_uint32, _P]),
    ("fr_glyph_info_init", C.c_int, [_P, _P, _P, C.c_uint32, _P, _P]),
    ("fr_winding_in_glyph", C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, _P]),
    ("fr_winding_lattice", C.c_int, [_P, _P, _P, C.c_uint32, _P, _P]),
    ("fr_glyph_debug_render", C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint8, _P]),
    ("fr_atlas_layout", C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint16, C.c_uint32, C.c_uint32, C.c_uint32,
                                  _P, _P, C.POINTER(C.c_uint32)]),
    ("fr_atlas_layout_glyph_dims", C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint16, C.c_uint32, C.c_uint32, _P,
                                             C.POINTER(C.c_uint32)]),
    ("fr_exact_lattice", C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, _P]),
    ("fr_exact_coverage", C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, _P]),
    ("fr_font_open", C.c_int, [_P, C.c_size_t, C.c_uint32, C.POINTER(_P)]),
    ("fr_font_close", None, [_P]),
    ("fr_font_info", C.c_int, [_P, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_int)]),
    ("fr_font_char_to_glyph", C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint16)]),
    ("fr_font_glyph_advance", C.c_int, [_P, C.c_uint16, C.POINTER(C.c_int16)]),
    ("fr_text_layout", C.c_int, [_P, _P, C.c_uint32, C.c_uint16, _P, _P, C.POINTER(C.c_int32)]),
    ("fr_font_line_metrics", C.c_int, [_P, C.POINTER(FontLine)]),
    ("fr_text_decoration", C.c_int, [_P, C.c_uint16, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("fr_font_glyph_measure", C.c_int, [_P, C.c_uint16, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _P]),
    ("fr_font_glyph_fill", C.c_int, [_P, C.c_uint16, _P, _P]),
    ("fr_qoi_bound", C.c_size_t, [C.c_uint32, C.c_uint32]),
    ("fr_qoi_encode_rgb", C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fr_qoi_encode_gray", C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fr_qoi_encode_rgba", C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fr_srgb_decode", C.c_int, [_P, C.c_size_t, _P]),
    ("fr_srgb_encode", C.c_int, [_P, C.c_size_t, _P]),
    ("fr_rgba_unpremultiply", C.c_int, [_P, C.c_size_t, C.c_int]),
    ("fr_layer_over", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, _P, C.c_uint32, C.c_uint32]),
    ("fr_layer_unpremultiply", C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int]),
    ("fr_layer_shadow", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.POINTER(LayerShadowParams), C.c_uint32]),
    ("fr_layer_outline", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.POINTER(LayerOutlineParams), C.c_uint32]),
    ("fr_layer_rects", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_uint32, C.c_uint32]),
    ("fr_layer_paint", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.POINTER(LayerPaintParams), C.c_uint32]),
    ("fr_layer_lcd", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, _P, C.c_uint32, C.POINTER(C.c_uint16), C.c_uint32]),
    ("fr_layer_mask", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, _P, C.c_uint32, C.c_uint32]),
    ("fr_layer_warp", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, _P, C.c_uint32, C.c_uint32]),
    ("fr_layer_blend", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, _P, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("fr_selftest_sqrt", C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    ("fr_selftest_division", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("fr_selftest_row_cuts", C.c_int, [_P, _P, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    ("fr_selftest_cand_records", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), _P]),
]

_lib = None


def _preload_hip_runtime() -> None:
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own
    libamdhip64.so.7; if this library pulled in /opt/rocm's copy first, a later
    `import torch` would bring a second runtime into the process (observed: "No HIP GPUs
    are available" + a crash at exit).  So when torch is installed, its runtime is loaded
    first and libfr_raster.so binds to it by SONAME.  FR_HIP_RUNTIME=system skips this
    (pure C / Zig hosts never see torch and use /opt/rocm's runtime via RUNPATH)."""
    if os.environ.get("FR_HIP_RUNTIME", "") == "system":
        return
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load_library() -> C.CDLL:
    """dlopen libfr_raster.so (built by __graft_entry__.build()); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback.")
    _preload_hip_runtime()
    lib = C.CDLL(path)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise FrError(rc, load_library().fr_last_error().decode("utf-8", "replace"))


def ptr(a):
    """numpy array -> void* (array must stay alive across the call)"""
    return a.ctypes.data_as(C.c_void_p)
