"""Host-side mirror of /root/reference/src/tools/render_glyph.zig on the C ABI.

Same names and argument meaning as the reference: renderGlyph(glyph, font_info,
font_size) -> Image.Gray (:11), GlyphInfo.init (:110), windingInGlyph (:160).  The
arithmetic runs in libfr_raster.so (HIP, gfx950); nothing is computed in Python."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from .glyph import FontInformation, Glyph, GlyphSet
from .image import RGB, Gray, Winding


def _flat(glyph: Glyph):
    gs = GlyphSet([glyph])
    return gs.points_xy, gs.contour_start, len(gs.contour_start) - 1


class Context:
    """fr_ctx.  stream: a hipStream_t handle (int) to launch on, e.g.
    torch.cuda.current_stream().cuda_stream, or None for a private stream."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._lib = L.load_library()
        h = C.c_void_p()
        L.check(self._lib.fr_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(h)))
        self._h = h
        self.device = device

    def set_option(self, key: str, value: int) -> None:
        L.check(self._lib.fr_ctx_set_option(self._h, key.encode(), value))

    def sync(self) -> None:
        L.check(self._lib.fr_ctx_sync(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.fr_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class DeviceGlyphSet:
    """fr_glyphset: points in HBM + root records (precompute kernel run at creation)."""

    def __init__(self, ctx: Context, gs: GlyphSet):
        self.ctx, self.host = ctx, gs
        h = C.c_void_p()
        L.check(ctx._lib.fr_glyphset_create(ctx._h, L.ptr(gs.points_xy), L.ptr(gs.contour_start), gs.n_contours,
                                            L.ptr(gs.glyph_start), len(gs), C.byref(h)))
        self._h = h
        boxes = np.ascontiguousarray(gs.boxes, np.int16)               # Glyph.box: what text plans size their cells from
        L.check(ctx._lib.fr_glyphset_set_boxes(self._h, L.ptr(boxes)))

    def prepare(self) -> None:
        L.check(self.ctx._lib.fr_glyphset_prepare(self._h))

    def stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        L.check(self.ctx._lib.fr_glyphset_stats(self._h, C.byref(a), C.byref(b)))
        return {"segments": a.value, "records": b.value}

    def selftest_row_cuts(self, jobs: np.ndarray, samples_per_axis: int = 1, sample_phase: int = L.FR_SAMPLE_CORNER):
        """fr_selftest_row_cuts over the cells of `jobs`: the set's row cuts against the acceptance expression at every
        sample row -> (pairs compared, mismatches, (job, candidate, row) of the first mismatch)"""
        assert jobs.dtype.itemsize == 32
        jobs = np.ascontiguousarray(jobs)
        pairs, bad = C.c_uint64(), C.c_uint64()
        first = (C.c_uint32 * 3)()
        L.check(self.ctx._lib.fr_selftest_row_cuts(self._h, L.ptr(jobs), len(jobs), samples_per_axis, sample_phase,
                                                   C.byref(pairs), C.byref(bad), first))
        return pairs.value, bad.value, tuple(first)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.ctx._lib.fr_glyphset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_jobs(rows: Sequence) -> np.ndarray:
    """rows of (glyph, min_x, max_y, w, h, out_x, out_y, scale) -> fr_job array"""
    dt = np.dtype([("glyph", "<u4"), ("min_x", "<i4"), ("max_y", "<i4"), ("w", "<u4"), ("h", "<u4"),
                   ("out_x", "<u4"), ("out_y", "<u4"), ("scale", "<f4")])
    a = np.zeros(len(rows), dt)
    for i, r in enumerate(rows):
        a[i] = tuple(r)
    return a


class Plan:
    """fr_plan: a job table resident on the device.  flags: FR_FILL_CONSISTENT or 0 (the reference's crossing rule)."""

    def __init__(self, dgs: DeviceGlyphSet, jobs: np.ndarray, mode: int, samples_per_axis: int = 1,
                 sample_phase: int = L.FR_SAMPLE_CORNER, flags: int = 0):
        assert jobs.dtype.itemsize == 32
        self.ctx, self.dgs, self.mode = dgs.ctx, dgs, mode
        self.params = L.RasterParams(mode, samples_per_axis, sample_phase, 0)
        jobs = np.ascontiguousarray(jobs)
        h = C.c_void_p()
        L.check(self.ctx._lib.fr_plan_create_ex(self.ctx._h, dgs._h, L.ptr(jobs), len(jobs), C.byref(self.params), flags,
                                                C.byref(h)))
        self._h = h
        self.n_jobs = len(jobs)

    @property
    def pixels(self) -> int:
        return int(self.ctx._lib.fr_plan_pixels(self._h))

    def stats(self) -> dict:
        """how the jobs are split between the two render kernels (decided per job)"""
        a, b = C.c_uint32(), C.c_uint32()
        L.check(self.ctx._lib.fr_plan_stats(self._h, C.byref(a), C.byref(b)))
        return {"jobs_cov4": a.value, "jobs_general": b.value}

    def describe(self) -> str:
        """the kernel instances one render launches, as rocprofv3 names them, with job counts"""
        buf = C.create_string_buffer(1024)
        L.check(self.ctx._lib.fr_plan_describe(self._h, buf, len(buf)))
        return buf.value.decode()

    def render(self, out_dev_ptr: int, out_stride: int, out_rows: int) -> None:
        """asynchronous on the context's stream; out_dev_ptr is a DEVICE address"""
        L.check(self.ctx._lib.fr_plan_render(self._h, C.c_void_p(out_dev_ptr), out_stride, out_rows))

    def render_timed(self, out_dev_ptr: int, out_stride: int, out_rows: int) -> float:
        ms = C.c_float()
        L.check(self.ctx._lib.fr_plan_render_timed(self._h, C.c_void_p(out_dev_ptr), out_stride, out_rows, C.byref(ms)))
        return ms.value

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.ctx._lib.fr_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PLACE_DTYPE = np.dtype([("glyph", "<u4"), ("pen_x64", "<i4"), ("pen_y", "<i4")])
PLACE_EX_DTYPE = np.dtype([("glyph", "<u4"), ("pen_x64", "<i4"), ("pen_y64", "<i4"), ("scale", "<f4"), ("slant", "<f4")])
PLACE_AFFINE_DTYPE = np.dtype([("glyph", "<u4"), ("pen_x64", "<i4"), ("pen_y64", "<i4"), ("m", "<f4", (4,))])
RUN_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4"), ("w", "<u4"), ("h", "<u4"), ("out_x", "<u4"), ("out_y", "<u4"),
                      ("scale", "<f4")])


def make_places(rows: Sequence) -> np.ndarray:
    """rows of (glyph, pen_x64, pen_y) -> fr_glyph_place array"""
    return np.array([tuple(r) for r in rows], PLACE_DTYPE)


def make_places_ex(rows: Sequence) -> np.ndarray:
    """rows of (glyph, pen_x64, pen_y64, scale, slant) -> fr_glyph_place_ex array (scale 0: the run's; slant 0: upright)"""
    return np.array([tuple(r) for r in rows], PLACE_EX_DTYPE)


def make_places_affine(rows: Sequence) -> np.ndarray:
    """rows of (glyph, pen_x64, pen_y64, xx, xy, yx, yy) -> fr_glyph_place_affine array: the font-unit point (x, y), y up, is
    drawn xx*x + xy*y pixels right of and yx*x + yy*y pixels above the pen"""
    out = np.zeros(len(rows), PLACE_AFFINE_DTYPE)
    for k, r in enumerate(rows):
        out[k] = (r[0], r[1], r[2], tuple(r[3:7]))
    return out


def _places(places) -> tuple:
    """a placement array of any of the three dtypes -> (C-contiguous array, the suffix of its entry points)"""
    dt = getattr(places, "dtype", None)
    if dt == PLACE_AFFINE_DTYPE:
        return np.ascontiguousarray(places, PLACE_AFFINE_DTYPE), "_affine"
    ex = dt == PLACE_EX_DTYPE
    return np.ascontiguousarray(places, PLACE_EX_DTYPE if ex else PLACE_DTYPE), "_ex" if ex else ""


def make_runs(rows: Sequence) -> np.ndarray:
    """rows of (first, count, w, h, out_x, out_y, scale) -> fr_text_run array"""
    return np.array([tuple(r) for r in rows], RUN_DTYPE)


class TextPlan(Plan):
    """fr_text_plan_create: glyph placements and the runs that composite them (include/fr_raster.h).  An ordinary
    fr_plan: render / render_timed / describe / stats / pixels / close as Plan.  mode: FR_COVERAGE_U8 (n in {1, 2, 4})
    or FR_MASK_NONZERO (n = 1).  places of PLACE_EX_DTYPE (make_places_ex) go through fr_text_plan_create_ex, places of
    PLACE_AFFINE_DTYPE (make_places_affine) through fr_text_plan_create_affine."""

    def __init__(self, dgs: DeviceGlyphSet, places: np.ndarray, runs: np.ndarray, mode: int = L.FR_COVERAGE_U8,
                 samples_per_axis: int = 4, sample_phase: int = L.FR_SAMPLE_CENTER, flags: int = 0):
        places, ex = _places(places)
        runs = np.ascontiguousarray(runs, RUN_DTYPE)
        self.ctx, self.dgs, self.mode = dgs.ctx, dgs, mode
        self.params = L.RasterParams(mode, samples_per_axis, sample_phase, 0)
        h = C.c_void_p()
        create = getattr(self.ctx._lib, "fr_text_plan_create" + ex)
        L.check(create(self.ctx._h, dgs._h, L.ptr(places), len(places), L.ptr(runs), len(runs), C.byref(self.params), flags, C.byref(h)))
        self._h = h
        self.n_places, self.n_runs = len(places), len(runs)


def _colors(rows, n: int, what: str) -> np.ndarray:
    """n RGBA colours -> (n, 4) u8, C-contiguous"""
    c = np.ascontiguousarray(np.asarray(rows, np.uint8).reshape(-1, 4)) if n else np.zeros((0, 4), np.uint8)
    if c.shape != (n, 4):
        raise ValueError(f"{what}: expected {n} RGBA colours, got shape {np.shape(rows)}")
    return c


class TextPlanRGBA(Plan):
    """fr_text_plan_create_rgba: a text plan whose placements carry colours (n_places x 4 u8, R G B A) blended per sample
    in placement order over each run's clear colour (n_runs x 4 u8); renders RGBA pixels (4 bytes each, 4-byte aligned
    output; strides and rows count pixels).  FR_COVERAGE_U8 only, n in {1, 2, 4}.  With FR_TEXT_LOAD in `flags` the
    samples start at the pixels already in the output instead, and run_clear_rgba may be None (it is ignored).  places of
    PLACE_EX_DTYPE (make_places_ex) go through fr_text_plan_create_rgba_ex, places of PLACE_AFFINE_DTYPE
    (make_places_affine) through fr_text_plan_create_rgba_affine."""

    def __init__(self, dgs: DeviceGlyphSet, places: np.ndarray, place_rgba, runs: np.ndarray, run_clear_rgba,
                 samples_per_axis: int = 4, sample_phase: int = L.FR_SAMPLE_CENTER, flags: int = 0):
        places, ex = _places(places)
        runs = np.ascontiguousarray(runs, RUN_DTYPE)
        pc = _colors(place_rgba, len(places), "place_rgba")
        rc = None if run_clear_rgba is None else _colors(run_clear_rgba, len(runs), "run_clear_rgba")     # (None: NULL)
        self.ctx, self.dgs, self.mode = dgs.ctx, dgs, L.FR_COVERAGE_U8
        self.params = L.RasterParams(L.FR_COVERAGE_U8, samples_per_axis, sample_phase, 0)
        h = C.c_void_p()
        create = getattr(self.ctx._lib, "fr_text_plan_create_rgba" + ex)
        L.check(create(self.ctx._h, dgs._h, L.ptr(places), L.ptr(pc), len(places), L.ptr(runs), None if rc is None else L.ptr(rc),
                       len(runs), C.byref(self.params), flags, C.byref(h)))
        self._h = h
        self.n_places, self.n_runs = len(places), len(runs)


BLIT_DTYPE = np.dtype([("src_x", "<u4"), ("src_y", "<u4"), ("w", "<u4"), ("h", "<u4"), ("dst_x", "<i4"), ("dst_y", "<i4"),
                       ("opacity", "<u4")])


def make_blits(rows: Sequence) -> np.ndarray:
    """rows of (src_x, src_y, w, h, dst_x, dst_y, opacity) -> fr_layer_blit array"""
    return np.array([tuple(r) for r in rows], BLIT_DTYPE)


def layer_over(ctx: Context, src_ptr: int, src_stride_px: int, src_rows: int, dst_ptr: int, dst_stride_px: int, dst_rows: int,
               blits, srgb: bool = False, flags: int = 0) -> None:
    """fr_layer_over: rectangles of the premultiplied layer at device address src_ptr composited over the premultiplied
    image at dst_ptr (both 4 bytes per pixel, alpha last; strides and rows in pixels), asynchronous on the context's
    stream.  blits: an fr_layer_blit array (make_blits) or None.  srgb: FR_LAYER_SRGB, composite in linear light."""
    n = 0 if blits is None else len(blits)
    b = None if blits is None else np.ascontiguousarray(blits, BLIT_DTYPE)
    L.check(ctx._lib.fr_layer_over(ctx._h, C.c_void_p(src_ptr), src_stride_px, src_rows, C.c_void_p(dst_ptr), dst_stride_px,
                                   dst_rows, None if b is None else L.ptr(b), n, flags | (L.FR_LAYER_SRGB if srgb else 0)))


RECT_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("rgba", "u1", (4,))])


def make_rects(rows: Sequence) -> np.ndarray:
    """rows of (x0, y0, x1, y1, (R, G, B, A)), the edges in 1/64 pixel -> fr_layer_rect array"""
    return np.array([(int(r[0]), int(r[1]), int(r[2]), int(r[3]), tuple(int(v) for v in r[4])) for r in rows], RECT_DTYPE)


def layer_rects(ctx: Context, dst_ptr: int, dst_stride_px: int, dst_rows: int, rects, srgb: bool = False, flags: int = 0) -> None:
    """fr_layer_rects: anti-aliased rectangles, each in one straight colour, composited in order over the premultiplied
    image at device address dst_ptr (4 bytes per pixel, alpha last; stride and rows in pixels), asynchronous on the
    context's stream.  rects: an fr_layer_rect array (make_rects) or None.  srgb: FR_LAYER_SRGB, composite in linear light."""
    n = 0 if rects is None else len(rects)
    r = None if rects is None else np.ascontiguousarray(rects, RECT_DTYPE)
    L.check(ctx._lib.fr_layer_rects(ctx._h, C.c_void_p(dst_ptr), dst_stride_px, dst_rows, None if r is None else L.ptr(r), n,
                                    flags | (L.FR_LAYER_SRGB if srgb else 0)))


def layer_unpremultiply(ctx: Context, ptr: int, stride_px: int, w: int, h: int, srgb: bool = False) -> None:
    """fr_layer_unpremultiply: the w x h window at device address ptr of an image with rows of stride_px pixels from
    premultiplied to straight alpha, in place, asynchronous on the context's stream"""
    L.check(ctx._lib.fr_layer_unpremultiply(ctx._h, C.c_void_p(ptr), stride_px, w, h, 1 if srgb else 0))


def layer_shadow(ctx: Context, src_ptr: int, src_stride_px: int, src_rows: int, dst_ptr: int, dst_stride_px: int, dst_rows: int,
                 window, rect, offset=(0, 0), spread: int = 0, blur_radius: int = 0, blur_passes: int = 0,
                 rgba=(0, 0, 0, 255), srgb: bool = False, flags: int = 0) -> None:
    """fr_layer_shadow: the alpha of the window (src_x, src_y, w, h) of the premultiplied layer at device address src_ptr,
    spread by a square maximum of radius `spread`, blurred by `blur_passes` box passes of radius `blur_radius`, moved by
    offset = (dx, dy) whole pixels and tinted with the straight colour rgba, written as a premultiplied R G B A layer over
    every pixel of rect = (dst_x, dst_y, dst_w, dst_h) of the image at dst_ptr (strides and rows in pixels); asynchronous
    on the context's stream.  srgb: FR_LAYER_SRGB, the colour bytes as an srgb=True render writes them.  window or rect
    None passes a NULL parameter block (refused)."""
    p = None
    if window is not None and rect is not None:
        p = L.LayerShadowParams(*[int(v) for v in window], *[int(v) for v in rect], int(offset[0]), int(offset[1]), int(spread),
                                int(blur_radius), int(blur_passes), (C.c_uint8 * 4)(*[int(v) for v in rgba]))
    L.check(ctx._lib.fr_layer_shadow(ctx._h, C.c_void_p(src_ptr), src_stride_px, src_rows, C.c_void_p(dst_ptr), dst_stride_px, dst_rows,
                                     None if p is None else C.byref(p), flags | (L.FR_LAYER_SRGB if srgb else 0)))


def render_batch(dgs: DeviceGlyphSet, jobs: np.ndarray, mode: int, out: np.ndarray, samples_per_axis: int = 1,
                 sample_phase: int = L.FR_SAMPLE_CORNER, flags: int = 0) -> np.ndarray:
    """fr_render_batch into a HOST array `out` (2-D, u8 or i16 for FR_WINDING_I16)."""
    want = np.int16 if mode == L.FR_WINDING_I16 else np.uint8
    assert out.dtype == want and out.ndim == 2 and out.flags.c_contiguous
    prm = L.RasterParams(mode, samples_per_axis, sample_phase, 0)
    jobs = np.ascontiguousarray(jobs)
    L.check(dgs.ctx._lib.fr_render_batch_ex(dgs.ctx._h, dgs._h, L.ptr(jobs), len(jobs), C.byref(prm), flags, L.ptr(out),
                                            out.shape[1], out.shape[0]))
    return out


def render_glyph_dims(box, units_per_em: int, font_size: int):
    """render_glyph.zig:13-19 -> (min_corner, max_corner, width, height, scale)"""
    lib = L.load_library()
    b = np.asarray(box, np.int16)
    mn, mx = np.zeros(2, np.int16), np.zeros(2, np.int16)
    w, h, s = C.c_uint16(), C.c_uint16(), C.c_float()
    L.check(lib.fr_render_glyph_dims(L.ptr(b), units_per_em, font_size, L.ptr(mn), L.ptr(mx), C.byref(w), C.byref(h), C.byref(s)))
    return (int(mn[0]), int(mn[1])), (int(mx[0]), int(mx[1])), w.value, h.value, s.value


def srgb_to_linear16(values) -> np.ndarray:
    """fr_srgb_decode: 8-bit sRGB values -> 16-bit linear light (u16, same shape), as FR_TEXT_SRGB plans decode them"""
    a = np.ascontiguousarray(values, np.uint8)
    out = np.empty(a.shape, np.uint16)
    L.check(L.load_library().fr_srgb_decode(L.ptr(a), a.size, L.ptr(out)))
    return out


def linear16_to_srgb(values) -> np.ndarray:
    """fr_srgb_encode: 16-bit linear light -> 8-bit sRGB (u8, same shape), rounded to nearest in the encoded domain"""
    a = np.asarray(values)
    if a.size and (a.min() < 0 or a.max() > 65535):
        raise ValueError("linear16_to_srgb: values outside [0, 65535]")
    a = np.ascontiguousarray(a, np.uint16)
    out = np.empty(a.shape, np.uint8)
    L.check(L.load_library().fr_srgb_encode(L.ptr(a), a.size, L.ptr(out)))
    return out


def renderGlyph(glyph: Glyph, font_info: FontInformation, font_size: int, *, ctx: Optional[Context] = None,
                mode: int = L.FR_GRAY_DEBUG, flags: int = 0) -> Gray:
    """render_glyph.zig:11 — `pub fn renderGlyph(glyph, font_info, font_size) !Image.Gray`."""
    ctx = ctx or default_context()
    _, _, w, h, _ = render_glyph_dims(glyph.box.as_array(), font_info.units_per_em, font_size)
    im = Gray.init(w, h)                                                     # :22
    pts, cstart, nc = _flat(glyph)
    box = glyph.box.as_array()
    L.check(ctx._lib.fr_render_glyph_ex(ctx._h, L.ptr(pts), L.ptr(cstart), nc, L.ptr(box), font_info.units_per_em,
                                        font_size, mode, flags, L.ptr(im.data)))
    return im


def renderGlyphWinding(glyph: Glyph, font_info: FontInformation, font_size: int, *, ctx: Optional[Context] = None,
                       scaler: int = 50, overflow_color: int = 150, flags: int = 0) -> Winding:
    """same grid as renderGlyph, raw i16 windings into an Image.Winding (Image.zig:85-130)"""
    ctx = ctx or default_context()
    _, _, w, h, _ = render_glyph_dims(glyph.box.as_array(), font_info.units_per_em, font_size)
    im = Winding.init(w, h, scaler, overflow_color)
    pts, cstart, nc = _flat(glyph)
    box = glyph.box.as_array()
    L.check(ctx._lib.fr_render_glyph_ex(ctx._h, L.ptr(pts), L.ptr(cstart), nc, L.ptr(box), font_info.units_per_em,
                                        font_size, L.FR_WINDING_I16, flags, L.ptr(im.data)))
    return im


class GlyphInfo:
    """render_glyph.zig:76-155.  contours[c] = list of (curve_type, include_p0)."""
    CURVE_TYPES = ("x_axis", "balance", "up_stright", "up_normal", "up_u", "up_inv_u",
                   "down_stright", "down_normal", "down_inv_u", "down_u")        # :84-95 enum order

    def __init__(self, curve_type: np.ndarray, include_p0: np.ndarray, curves_per_contour: Sequence[int]):
        self.curve_type, self.include_p0 = curve_type, include_p0
        self.contours, o = [], 0
        for n in curves_per_contour:
            self.contours.append(list(zip(curve_type[o:o + n].tolist(), include_p0[o:o + n].astype(bool).tolist())))
            o += n

    @staticmethod
    def init(glyph: Glyph, *, ctx: Optional[Context] = None) -> "GlyphInfo":    # :110
        ctx = ctx or default_context()
        pts, cstart, nc = _flat(glyph)
        n = glyph.curve_count
        ct, ip = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        L.check(ctx._lib.fr_glyph_info_init(ctx._h, L.ptr(pts), L.ptr(cstart), nc, L.ptr(ct), L.ptr(ip)))
        return GlyphInfo(ct[:n], ip[:n], [c.curve_count for c in glyph.contours])

    def deinit(self) -> None:                                                    # :148
        self.contours = []


def windingInGlyph(glyph: Glyph, glyph_info: Optional[GlyphInfo], point, *, ctx: Optional[Context] = None):
    """render_glyph.zig:160.  `point` is one (x, y) or an (n, 2) int16 array; glyph_info is
    recomputed on the device (it is a pure function of the glyph) and only type-checked here."""
    ctx = ctx or default_context()
    q = np.ascontiguousarray(point, np.int16).reshape(-1, 2)
    pts, cstart, nc = _flat(glyph)
    out = np.zeros(len(q), np.int16)
    L.check(ctx._lib.fr_winding_in_glyph(ctx._h, L.ptr(pts), L.ptr(cstart), nc, L.ptr(q), len(q), L.ptr(out)))
    return int(out[0]) if np.ndim(point) == 1 else out


def winding_lattice(glyph: Glyph, *, ctx: Optional[Context] = None) -> np.ndarray:
    """the lattice of Image.GlyphDebug.render (Image.zig:220-240): (H, W) int16"""
    ctx = ctx or default_context()
    pts, cstart, nc = _flat(glyph)
    box = glyph.box.as_array()
    W, H = int(box[2]) - int(box[0]) + 3, int(box[3]) - int(box[1]) + 3
    out = np.zeros((H, W), np.int16)
    L.check(ctx._lib.fr_winding_lattice(ctx._h, L.ptr(pts), L.ptr(cstart), nc, L.ptr(box), L.ptr(out)))
    return out


def exact_lattice(glyph: Glyph, K: int, x0: int, y0: int, w: int, h: int, *, ctx: Optional[Context] = None) -> np.ndarray:
    """SURVEY §8 f-3 (build-defined): GlyphInfo.init + windingInGlyph (render_glyph.zig:110-300) on the
    glyph scaled by K, at the integer points (x0 + i, y0 - j) of the scaled glyph: (h, w) int16"""
    ctx = ctx or default_context()
    pts, cstart, nc = _flat(glyph)
    out = np.zeros((h, w), np.int16)
    L.check(ctx._lib.fr_exact_lattice(ctx._h, L.ptr(pts), L.ptr(cstart), nc, K, x0, y0, w, h, L.ptr(out)))
    return out


def exact_coverage(glyph: Glyph, K: int, x0: int, y0: int, w_px: int, h_px: int, n: int, *,
                   ctx: Optional[Context] = None) -> np.ndarray:
    """n x n lattice points per pixel of exact_lattice -> round_half_up(255 * inside / n^2): (h_px, w_px) u8"""
    ctx = ctx or default_context()
    pts, cstart, nc = _flat(glyph)
    out = np.zeros((h_px, w_px), np.uint8)
    L.check(ctx._lib.fr_exact_coverage(ctx._h, L.ptr(pts), L.ptr(cstart), nc, K, x0, y0, w_px, h_px, n, L.ptr(out)))
    return out


def glyph_debug_render(glyph: Glyph, winding_scale: int, *, ctx: Optional[Context] = None) -> RGB:
    """Image.GlyphDebug.render (Image.zig:220-240) through fr_glyph_debug_render: the exact-integer lattice
    coloured by setWindingLinear (:192-200) with the glyph's points marked (:202-218)"""
    ctx = ctx or default_context()
    pts, cs, nc = _flat(glyph)
    box = glyph.box.as_array()
    W, H = int(box[2]) - int(box[0]) + 3, int(box[3]) - int(box[1]) + 3
    out = np.zeros((H * W, 3), np.uint8)
    L.check(ctx._lib.fr_glyph_debug_render(ctx._h, L.ptr(pts), L.ptr(cs), nc, L.ptr(box), winding_scale, L.ptr(out)))
    return RGB(W, H, out)


def build_id() -> str:
    return L.load_library().fr_build_id().decode()
