#!/usr/bin/env python3
"""Mints tests/golden/host_rules.json: the lines host/host_rules_selftest prints, made from a built libfr_raster.so through
ctypes — the library as it was BEFORE the host arithmetic moved into csrc/fr_host_rules.cpp, so that the golden file
records what the entry points answered then.  No device is needed: fr_render_glyph_dims, both atlas layouts, the sRGB
conversions and fr_rgba_unpremultiply never touch one, and check_k answers through fr_exact_lattice before the context
is looked at (a NULL context: "ctx is NULL" means the lattice passed).

The case tables are those of host/host_rules_selftest.cpp, restated.  check_params, check_flags, check_job and the arena
layout are not reachable in a library without a device: their lines are taken from the self-test given with --selftest
(tests/test_host_rules.py restates those rules on its own).

    tools/mint_host_rules.py --lib OLD/libfr_raster.so --selftest font-renderer_amd/host/host_rules_selftest > tests/golden/host_rules.json
"""
import argparse
import ctypes as C
import json
import struct
import subprocess
import sys

import numpy as np

JOB = np.dtype([("glyph", "<u4"), ("min_x", "<i4"), ("max_y", "<i4"), ("w", "<u4"), ("h", "<u4"), ("out_x", "<u4"), ("out_y", "<u4"), ("scale", "<f4")])


def fnv(b):
    b = bytes(b)
    h = 0xCBF29CE484222325
    for x in b:
        h = ((h ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return "#%d:%016x" % (len(b), h)


def job_text(j):
    return "%d,%d,%d,%d,%d,%d,%d,%08x" % (j["glyph"], j["min_x"], j["max_y"], j["w"], j["h"], j["out_x"], j["out_y"], struct.unpack("<I", struct.pack("<f", j["scale"]))[0])


def glyphs(n, upm1, tall=False):
    i = np.arange(n, dtype=np.int64)
    if tall:
        boxes = np.tile(np.array([0, 0, 10, 32765], np.int16), (n, 1))
    else:
        boxes = np.stack([-(i * 37 % 200), -(i * 91 % 300), 100 + i * 53 % 900, 200 + i * 29 % 1200], 1).astype(np.int16)
    upm = np.array([upm1], np.uint16) if upm1 else (1000 + (i % 3) * 512).astype(np.uint16)
    return np.ascontiguousarray(boxes), upm


DIMS = [
    ("fraction", (-3, -7, 1001, 1503), 2048, 64), ("tiny", (10, 20, 30, 40), 65535, 1), ("point", (0, 0, 0, 0), 1, 65535),
    ("negative", (-900, -800, -100, -50), 1000, 333), ("w32767", (0, 0, 32766, 10), 1, 1), ("w32768", (0, 0, 32767, 10), 1, 1),
    ("h32767", (0, -32766, 10, 0), 1, 1), ("h32768", (0, -32767, 10, 0), 1, 1), ("min-32768", (-32768, -5, -2, 5), 1, 1),
    ("min-32768wide", (-32768, -5, -1, 5), 1, 1), ("hi32767", (32760, 0, 32767, 10), 1, 1), ("scaled-hi-in", (0, 0, 16383, 100), 1, 2),
    ("scaled-hi-out", (0, 0, 16384, 100), 1, 2), ("scaled-hi-y-out", (0, 0, 100, 16384), 1, 2), ("scaled-lo-in", (-16384, 0, -16000, 10), 1, 2),
    ("scaled-lo-out", (-16385, 0, -16000, 10), 1, 2), ("scaled-lo-y-out", (0, -16385, 10, -16000), 1, 2), ("upm0", (0, 0, 10, 10), 0, 10),
    ("size0", (0, 0, 10, 10), 10, 0),
]
# name, n, first, upm1, n_upm, size, cell, cols, rows_per_page, boxes, jobs, upm
CELLS = [
    ("one-page", 10, 5, 2048, 1, 64, 64, 4, 0, 1, 1, 1), ("pages-upm-per-glyph", 23, 0, 0, 23, 48, 32, 5, 2, 1, 1, 1),
    ("page-exact", 12, 100, 1000, 1, 20, 16, 3, 2, 1, 1, 1), ("one-glyph-upm-both", 1, 7, 0, 1, 64, 128, 1, 1, 1, 1, 1),
    ("empty", 0, 0, 1000, 1, 64, 64, 4, 0, 0, 0, 1), ("null-boxes", 3, 0, 1000, 1, 64, 64, 4, 0, 0, 1, 1),
    ("null-jobs", 3, 0, 1000, 1, 64, 64, 4, 0, 1, 0, 1), ("null-upm", 3, 0, 1000, 1, 64, 64, 4, 0, 1, 1, 0),
    ("n-upm-2-of-5", 5, 0, 0, 2, 64, 64, 4, 0, 1, 1, 1), ("cell-0", 3, 0, 1000, 1, 64, 0, 4, 0, 1, 1, 1),
    ("cols-0", 3, 0, 1000, 1, 64, 64, 0, 0, 1, 1, 1), ("size-0", 3, 0, 1000, 1, 0, 64, 4, 0, 1, 1, 1),
    ("too-wide", 3, 0, 1000, 1, 64, 65536, 65536, 0, 1, 1, 1), ("widest", 3, 0, 1000, 1, 64, 65535, 65537, 0, 1, 1, 1),
    ("too-tall", 3, 0, 1000, 1, 64, 0x80000000, 1, 0, 1, 1, 1), ("tallest", 2, 0, 1000, 1, 64, 0x80000000, 1, 0, 1, 1, 1),
    ("tall-paged", 5, 0, 1000, 1, 64, 0x80000000, 1, 2, 1, 1, 1),
]
# name, n, first, upm1, n_upm, size, atlas_w, align, boxes, jobs, upm, tall
SHELVES = [
    ("wrap", 20, 0, 1000, 1, 100, 300, 1, 1, 1, 1, 0), ("align-16-upm-per-glyph", 20, 3, 0, 20, 64, 256, 16, 1, 1, 1, 0),
    ("align-0", 5, 0, 2048, 1, 200, 4096, 0, 1, 1, 1, 0), ("align-7-tight", 9, 0, 1000, 1, 50, 60, 7, 1, 1, 1, 0),
    ("one-glyph-upm-both", 1, 9, 0, 1, 64, 64, 1, 1, 1, 1, 0), ("empty", 0, 0, 1000, 1, 64, 64, 1, 0, 0, 1, 0),
    ("null-boxes", 3, 0, 1000, 1, 64, 640, 1, 0, 1, 1, 0), ("null-jobs", 3, 0, 1000, 1, 64, 640, 1, 1, 0, 1, 0),
    ("null-upm", 3, 0, 1000, 1, 64, 640, 1, 1, 1, 0, 0), ("n-upm-2-of-5", 5, 0, 0, 2, 64, 640, 1, 1, 1, 1, 0),
    ("atlas-w-0", 3, 0, 1000, 1, 64, 0, 1, 1, 1, 1, 0), ("size-0", 3, 0, 1000, 1, 0, 640, 1, 1, 1, 1, 0),
    ("glyph-too-wide", 3, 0, 1000, 1, 64, 4, 1, 1, 1, 1, 0), ("box-leaves-i16", 3, 0, 1, 1, 65535, 640, 1, 1, 1, 1, 0),
    ("tallest", 131080, 0, 1, 1, 1, 11, 1, 1, 1, 1, 1), ("too-tall", 131081, 0, 1, 1, 1, 11, 1, 1, 1, 1, 1),
]
M = 1 << 20
KS = [
    ("K-0", 0, 0, 0, 4, 4), ("K-1", 1, 0, 0, 4, 4), ("K-8", 8, 0, 0, 4, 4), ("K-9", 9, 0, 0, 4, 4),
    ("w-max", 1, -M, 0, M, 4), ("w-over", 1, -M, 0, M + 1, 4), ("h-max", 1, 0, M, 4, M), ("h-over", 1, 0, M, 4, M + 1),
    ("x0-min", 1, -M, 0, 4, 4), ("x0-under", 1, -M - 1, 0, 4, 4), ("x1-max", 1, M - 4, 0, 4, 4), ("x1-over", 1, M - 3, 0, 4, 4),
    ("y0-max", 1, 0, M, 4, 4), ("y0-over", 1, 0, M + 1, 4, 4), ("y1-min", 1, 0, -M + 4, 4, 4), ("y1-under", 1, 0, -M + 3, 4, 4),
    ("empty", 3, 0, 0, 0, 0),
]


def mint(lib):
    lib.fr_last_error.restype = C.c_char_p
    out = []
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def line(name, rc, fields):
        out.append("%s rc=%d %s" % (name, rc, "err=" + lib.fr_last_error().decode() if rc else fields))

    def dims(box, upm, size, width=True, scale=True):
        b = np.array(box, np.int16) if box is not None else None
        mn, mx, w, h, s = np.zeros(2, np.int16), np.zeros(2, np.int16), C.c_uint16(0), C.c_uint16(0), C.c_float(0)
        rc = lib.fr_render_glyph_dims(p(b), C.c_uint16(upm), C.c_uint16(size), p(mn), p(mx), C.byref(w) if width else None, C.byref(h),
                                      C.byref(s) if scale else None)
        return rc, mn, mx, w.value, h.value, struct.unpack("<I", struct.pack("<f", s.value))[0]

    for name, box, upm, size in DIMS:
        rc, mn, mx, w, h, bits = dims(box, upm, size)
        line("dims/" + name, rc, "min=%d,%d max=%d,%d size=%dx%d scale=%08x" % (mn[0], mn[1], mx[0], mx[1], w, h, bits))
    line("dims/null-box", dims(None, 10, 10, scale=False)[0], "")
    line("dims/null-width", dims((0, 0, 10, 10), 10, 10, width=False, scale=False)[0], "")
    rc, _, _, w, h, _ = dims((0, 0, 10, 10), 10, 10, scale=False)
    line("dims/without-scale", rc, "size=%dx%d" % (w, h))

    def cells(n, first, upm, n_upm, size, cell, cols, rpp, boxes, jobs, pages=True):
        page, n_pages = np.zeros(n, np.uint32), C.c_uint32(0)
        rc = lib.fr_atlas_layout(p(boxes), C.c_uint32(n), C.c_uint32(first), p(upm), C.c_uint32(n_upm), C.c_uint16(size), C.c_uint32(cell),
                                 C.c_uint32(cols), C.c_uint32(rpp), p(jobs), p(page) if pages else None, C.byref(n_pages) if pages else None)
        return rc, page, n_pages.value

    for name, n, first, upm1, n_upm, size, cell, cols, rpp, hb, hj, hu in CELLS:
        boxes, upm = glyphs(n, upm1)
        if upm1 == 0 and n_upm < n:
            upm = upm[:n_upm].copy()
        jobs = np.zeros(n, JOB)
        rc, page, n_pages = cells(n, first, upm if hu else None, n_upm, size, cell, cols, rpp, boxes if hb else None, jobs if hj else None)
        line("cells/" + name, rc, "n=%d jobs=%s last=%s page_of=%s pages=%d" % (n, fnv(jobs.tobytes()), job_text(jobs[-1]) if n else "-", fnv(page.tobytes()), n_pages))
    boxes, upm = glyphs(4, 0)
    upm[2] = 0
    jobs = np.zeros(4, JOB)
    line("cells/upm-0-at-2", cells(4, 0, upm, 4, 64, 64, 4, 0, boxes, jobs, pages=False)[0], "")
    upm[2] = 1000
    line("cells/no-page-outputs", cells(4, 0, upm, 4, 64, 64, 4, 0, boxes, jobs, pages=False)[0], "jobs=%s" % fnv(jobs.tobytes()))

    def shelves(n, first, upm, n_upm, size, atlas_w, align, boxes, jobs, height=True):
        atlas_h = C.c_uint32(0)
        rc = lib.fr_atlas_layout_glyph_dims(p(boxes), C.c_uint32(n), C.c_uint32(first), p(upm), C.c_uint32(n_upm), C.c_uint16(size),
                                            C.c_uint32(atlas_w), C.c_uint32(align), p(jobs), C.byref(atlas_h) if height else None)
        return rc, atlas_h.value

    for name, n, first, upm1, n_upm, size, atlas_w, align, hb, hj, hu, tall in SHELVES:
        boxes, upm = glyphs(n, upm1, bool(tall))
        if upm1 == 0 and n_upm < n:
            upm = upm[:n_upm].copy()
        jobs = np.zeros(n, JOB)
        rc, atlas_h = shelves(n, first, upm if hu else None, n_upm, size, atlas_w, align, boxes if hb else None, jobs if hj else None)
        line("shelves/" + name, rc, "n=%d jobs=%s last=%s atlas_h=%d" % (n, fnv(jobs.tobytes()), job_text(jobs[-1]) if n else "-", atlas_h))
    boxes, upm = glyphs(4, 0)
    upm[2] = 0
    jobs = np.zeros(4, JOB)
    line("shelves/upm-0-at-2", shelves(4, 0, upm, 4, 64, 640, 1, boxes, jobs, height=False)[0], "")
    upm[2] = 1000
    line("shelves/no-height-output", shelves(4, 0, upm, 4, 64, 640, 1, boxes, jobs, height=False)[0], "jobs=%s" % fnv(jobs.tobytes()))

    codes, lin, back = np.arange(256, dtype=np.uint8), np.zeros(256, np.uint16), np.zeros(256, np.uint8)
    rc = lib.fr_srgb_decode(p(codes), C.c_size_t(256), p(lin))
    line("srgb/decode-all-codes", rc, "first=%d last=%d table=%s" % (lin[0], lin[255], fnv(lin.tobytes())))
    rc = lib.fr_srgb_encode(p(lin), C.c_size_t(256), p(back))
    line("srgb/encode-decoded", rc, "same=%d" % int(np.array_equal(back, codes)))
    allv, enc = np.arange(65536, dtype=np.uint16), np.zeros(65536, np.uint8)
    rc = lib.fr_srgb_encode(p(allv), C.c_size_t(65536), p(enc))
    line("srgb/encode-all-values", rc, "first=%d last=%d table=%s" % (enc[0], enc[65535], fnv(enc.tobytes())))
    line("srgb/decode-null", lib.fr_srgb_decode(None, C.c_size_t(1), p(lin)), "")
    line("srgb/encode-null", lib.fr_srgb_encode(p(allv), C.c_size_t(1), None), "")
    line("srgb/decode-nothing", lib.fr_srgb_decode(None, C.c_size_t(0), None), "ok")
    line("srgb/encode-nothing", lib.fr_srgb_encode(None, C.c_size_t(0), None), "ok")
    for srgb in (0, 1):
        a, c = np.divmod(np.arange(65536, dtype=np.uint32), 256)
        px = np.ascontiguousarray(np.stack([c, 255 - c, c ^ 0x55, a], 1).astype(np.uint8))
        rc = lib.fr_rgba_unpremultiply(p(px), C.c_size_t(65536), C.c_int(srgb))
        line("unpremultiply/%s-all-pairs" % ("srgb" if srgb else "linear"), rc, "image=%s" % fnv(px.tobytes()))
    line("unpremultiply/null", lib.fr_rgba_unpremultiply(None, C.c_size_t(1), C.c_int(0)), "")
    line("unpremultiply/nothing", lib.fr_rgba_unpremultiply(None, C.c_size_t(0), C.c_int(1)), "ok")

    for name, K, x0, y0, w, h in KS:
        rc = lib.fr_exact_lattice(None, None, None, C.c_uint32(0), C.c_uint32(K), C.c_int32(x0), C.c_int32(y0), C.c_uint32(w), C.c_uint32(h), None)
        if rc == -1 and lib.fr_last_error() == b"ctx is NULL":
            rc = 0                      # check_k passed; the context is what it looked at next
        line("check_k/" + name, rc, "ok")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True)
    ap.add_argument("--selftest", required=True)
    a = ap.parse_args()
    minted = dict(l.split(" ", 1) for l in mint(C.CDLL(a.lib)))
    own = dict(l.split(" ", 1) for l in subprocess.run([a.selftest], capture_output=True, text=True, check=True).stdout.splitlines())
    missing = [k for k in minted if k not in own]
    assert not missing, "cases the self-test does not print: %s" % missing
    unreachable = ("check_params/", "check_flags/", "check_job/", "scale_in_range", "arena/")
    lines = {}
    for k, v in own.items():                # the self-test's order
        if k in minted:
            lines[k] = minted[k]
        else:
            assert k.startswith(unreachable), k
            lines[k] = v
    json.dump(lines, sys.stdout, indent=0)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
