"""Host-side mirror of /root/reference/src/tools/render_glyph.zig on the C ABI.

Same names and argument meaning as the reference: renderGlyph(glyph, font_info,
font_size) -> Image.Gray (:11), GlyphInfo.init (:110), windingInGlyph (:160).  The
arithmetic runs in libfr_raster.so (HIP, gfx950); nothing is computed in Python."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from .device import Context, Handle, default_context
from .glyph import FontInformation, Glyph, GlyphSet
from .image import RGB, GlyphDebug, Gray, Winding
# Kept names, not a second home: the layer calls are defined in layer.py only.  They were public attributes of this
# module, and code outside this tree's current tests and tools (the suite of the commit before layer.py existed among
# it) calls render_glyph.layer_* and render_glyph.make_blits / make_rects; dropping the names breaks those callers.
from .layer import BLIT_DTYPE, RECT_DTYPE, layer_over, layer_rects, layer_shadow, layer_unpremultiply, make_blits, make_rects  # noqa: F401


def _flat(glyph: Glyph):
    gs = GlyphSet([glyph])
    return gs.points_xy, gs.contour_start, len(gs.contour_start) - 1


class DeviceGlyphSet(Handle):
    """fr_glyphset: points in HBM + root records (precompute kernel run at creation)."""

    def __init__(self, ctx: Context, gs: GlyphSet):
        self.ctx, self.host = ctx, gs
        self._open(ctx._lib.fr_glyphset_destroy, ctx._lib.fr_glyphset_create, ctx._h, L.ptr(gs.points_xy),
                   L.ptr(gs.contour_start), gs.n_contours, L.ptr(gs.glyph_start), len(gs))
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

    def selftest_cand_records(self):
        """fr_selftest_cand_records: the set's candidate table against records and cuts rebuilt from the control points
        -> (live candidates, mismatching slots, (glyph, slot) of the first mismatch, live candidates per glyph)"""
        live, bad = C.c_uint64(), C.c_uint64()
        first = (C.c_uint32 * 2)()
        per_glyph = np.zeros(max(len(self.host), 1), np.uint32)
        L.check(self.ctx._lib.fr_selftest_cand_records(self._h, C.byref(live), C.byref(bad), first, L.ptr(per_glyph)))
        return live.value, bad.value, tuple(first), per_glyph[:len(self.host)]


# the tables of the C ABI as numpy sees them: derived from the ctypes structures of _lib, which mirror include/fr_raster.h
JOB_DTYPE = np.dtype(L.Job)
PLACE_DTYPE = np.dtype(L.GlyphPlace)
PLACE_EX_DTYPE = np.dtype(L.GlyphPlaceEx)
PLACE_AFFINE_DTYPE = np.dtype(L.GlyphPlaceAffine)
RUN_DTYPE = np.dtype(L.TextRun)


def make_jobs(rows: Sequence) -> np.ndarray:
    """rows of (glyph, min_x, max_y, w, h, out_x, out_y, scale) -> fr_job array"""
    a = np.zeros(len(rows), JOB_DTYPE)
    for i, r in enumerate(rows):
        a[i] = tuple(r)
    return a


class Plan(Handle):
    """fr_plan: a job table resident on the device.  flags: FR_FILL_CONSISTENT or 0 (the reference's crossing rule)."""

    def __init__(self, dgs: DeviceGlyphSet, jobs: np.ndarray, mode: int, samples_per_axis: int = 1,
                 sample_phase: int = L.FR_SAMPLE_CORNER, flags: int = 0):
        assert jobs.dtype.itemsize == 32
        jobs = np.ascontiguousarray(jobs)
        self._create(dgs, mode, samples_per_axis, sample_phase, flags, "fr_plan_create_ex", L.ptr(jobs), len(jobs))
        self.n_jobs = len(jobs)

    def _create(self, dgs: DeviceGlyphSet, mode: int, samples_per_axis: int, sample_phase: int, flags: int, entry: str, *table):
        """what every plan is made by: entry(ctx, glyph set, *table, &params, flags, &plan)"""
        self.ctx, self.dgs, self.mode = dgs.ctx, dgs, mode
        self.params = L.RasterParams(mode, samples_per_axis, sample_phase, 0)
        lib = self.ctx._lib
        self._open(lib.fr_plan_destroy, getattr(lib, entry), self.ctx._h, dgs._h, *table, C.byref(self.params), flags)

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
        self._create(dgs, mode, samples_per_axis, sample_phase, flags, "fr_text_plan_create" + ex,
                     L.ptr(places), len(places), L.ptr(runs), len(runs))
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
        self._create(dgs, L.FR_COVERAGE_U8, samples_per_axis, sample_phase, flags, "fr_text_plan_create_rgba" + ex,
                     L.ptr(places), L.ptr(pc), len(places), L.ptr(runs), None if rc is None else L.ptr(rc), len(runs))
        self.n_places, self.n_runs = len(places), len(runs)


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
    return GlyphDebug.render(glyph, winding_scale, ctx=ctx).rgb


def build_id() -> str:
    return L.load_library().fr_build_id().decode()
