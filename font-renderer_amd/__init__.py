"""font-renderer_amd — MI355X-native glyph rasterizer (host-side mirror).

Python mirror of the reference's host interface for ONE path
(/root/reference/src/tools/render_glyph.zig + the Glyph/Image types either side of
it), sitting on the C ABI of include/fr_raster.h (libfr_raster.so, hand-written HIP
for gfx950).  There is no CPU path in this package: every compute call goes through
the shared library and raises if it (or a GPU) is missing.
"""
from .glyph import Box, Contour, FontInformation, Glyph, GlyphSet  # noqa: F401
from .image import RGB, RGBA, Gray, GlyphDebug, Winding  # noqa: F401
from ._lib import (  # noqa: F401
    FR_COVERAGE_U8, FR_DECOR_LINE_BOX, FR_DECOR_STRIKEOUT, FR_DECOR_UNDERLINE, FR_FILL_CONSISTENT, FR_SDF_U8, FR_GRAY_DEBUG, FR_MASK_NONZERO, FR_SAMPLE_CENTER, FR_SAMPLE_CORNER,
    FR_GRADIENT_LINEAR, FR_GRADIENT_MAX_STOPS, FR_GRADIENT_RADIAL, FR_SPREAD_PAD, FR_SPREAD_REFLECT, FR_SPREAD_REPEAT,
    FR_BLEND_DARKEN, FR_BLEND_DIFFERENCE, FR_BLEND_EXCLUSION, FR_BLEND_HARD_LIGHT, FR_BLEND_LIGHTEN, FR_BLEND_MODES, FR_BLEND_MULTIPLY, FR_BLEND_OVERLAY, FR_BLEND_PLUS, FR_BLEND_SCREEN,
    FR_OUTLINE_GROW, FR_OUTLINE_INNER, FR_OUTLINE_MAX_RADIUS, FR_OUTLINE_RING, FR_OUTLINE_SHRINK,
    FR_LAYER_SRGB, FR_LCD_BGR, FR_LCD_TAPS, FR_MASK_ERASE, FR_MASK_PLANE, FR_TEXT_BGRA, FR_TEXT_CACHE, FR_TEXT_CACHE_AFFINE, FR_TEXT_LOAD, FR_TEXT_OVER, FR_TEXT_SRGB, FR_WINDING_I16, FrError, GlyphPlace, GlyphPlaceAffine, GlyphPlaceEx,
    FontLine, GradientStop, Job, LayerBlit, LayerMaskBlit, LayerOutlineParams, LayerPaintParams, LayerRect, LayerShadowParams, LayerWarpBlit, LcdBlit, TextRun, lib_path, load_library,
)
from .device import Context  # noqa: F401
from .layer import (  # noqa: F401
    layer_blend, layer_lcd, layer_mask, layer_outline, layer_over, layer_paint, layer_rects, layer_shadow, layer_unpremultiply, layer_warp, make_blits, make_gradient_linear, make_gradient_radial,
    make_lcd_blits, make_mask_blits, make_rects, make_warp_blits, warp_from_matrix,
)
from .render_glyph import (  # noqa: F401
    GlyphInfo, Plan, TextPlan, TextPlanRGBA, DeviceGlyphSet, make_places, make_places_affine, make_places_ex, make_runs, renderGlyph,
    render_glyph_dims,
    windingInGlyph, winding_lattice, exact_lattice, exact_coverage, glyph_debug_render, build_id, srgb_to_linear16,
    linear16_to_srgb,
)
from .font import Font  # noqa: F401
from .text import (  # noqa: F401
    decoration_rects, draw_text_lcd, draw_text_rgba, instance_cell, instance_cell_affine, instance_cell_ex, lcd_line, placed_line, render_spans, render_spans_rgba, render_text,
    render_text_lcd, render_text_rgba, render_text_rgba_rotated, render_text_rotated, render_text_view, rotated_line, span_line, view_line,
)
