"""CPU twin of sRGB text plans (fr_text_plan_create_rgba with FR_TEXT_SRGB / FR_TEXT_BGRA, include/fr_raster.h, DESIGN.md
section 5), written from the definition and not from the kernel or the generated header: the tables come from the
IEC 61966-2-1 decode f in binary64, the per-instance non-zero tests from tests/text_rgba_ref.instance_hits.  Every
sub-sample of a run starts at its clear colour; the instances are applied in placement order, each to the samples where
its winding is non-zero, by c' = E((D[C.c] * A + D[c] * (255 - A) + 127) div 255) for R G B and a' = A; each colour
channel of a pixel is then E((sum of D over its n x n samples + n^2 / 2) div n^2), alpha (sum + n^2 / 2) div n^2.
FR_TEXT_BGRA swaps bytes 0 and 2 of every output pixel."""
import math

import numpy as np

import text_rgba_ref


def decode(c: float) -> float:
    return c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4


def _tables():
    D = np.array([math.floor(65535.0 * decode(v / 255.0) + 0.5) for v in range(256)], np.int64)
    T = np.array([math.ceil(65535.0 * decode((k - 0.5) / 255.0)) for k in range(1, 256)], np.int64)     # T[1 .. 255]
    E = np.searchsorted(T, np.arange(65536), side="right").astype(np.int64)     # #{k : L >= T[k]}
    return D, T, E


D, T, E = _tables()


def encode(L):
    """E(L) for L in [0, 65535] (array or int)"""
    return E[np.asarray(L, np.int64)]


def blend(dst, c):
    """the definition's update of sRGB RGBA samples dst (..., 4) int64 by the colour c = (R, G, B, A)"""
    a = int(c[3])
    out = np.empty_like(dst)
    for ch in range(3):
        out[..., ch] = encode((int(D[int(c[ch])]) * a + D[dst[..., ch]] * (255 - a) + 127) // 255)
    out[..., 3] = a
    return out


def run_samples(gs, places, place_rgba, run, clear, n=1, center=False, fill=False):
    """-> (h n, w n, 4) int64: every sub-sample's sRGB RGBA after the run's instances, in placement order"""
    w, h = int(run["w"]), int(run["h"])
    smp = np.empty((h * n, w * n, 4), np.int64)
    smp[:] = np.asarray(clear, np.int64)
    for k, y0, x0, hit in text_rgba_ref.instance_hits(gs, places, run, n, center, fill):
        view = smp[y0 * n:y0 * n + hit.shape[0], x0 * n:x0 * n + hit.shape[1]]
        view[hit] = blend(view[hit], place_rgba[k])
    return smp


def resolve(smp, n):
    """E((sum of D over each pixel's n x n samples + n^2/2) div n^2) for R G B, the rounded mean for alpha -> (h, w, 4) u8"""
    h, w = smp.shape[0] // n, smp.shape[1] // n
    lin = smp.copy()
    lin[..., :3] = D[smp[..., :3]]
    s = lin.reshape(h, n, w, n, 4).sum(axis=(1, 3))
    q = (s + n * n // 2) // (n * n)
    q[..., :3] = encode(q[..., :3])
    return q.astype(np.uint8)


def bgra(img):
    """R G B A pixels -> B G R A"""
    return img[..., [2, 1, 0, 3]]


def render_run(gs, places, place_rgba, run, clear, n=1, center=False, fill=False, bgr=False):
    img = resolve(run_samples(gs, places, place_rgba, run, clear, n, center, fill), n)
    return bgra(img) if bgr else img


def render_runs(gs, places, place_rgba, runs, run_clear, out, n=1, center=False, fill=False, which=None, bgr=False):
    """every run (or the runs `which`) into the (rows, cols, 4) u8 array `out`, as an sRGB text plan writes it"""
    for r in (range(len(runs)) if which is None else which):
        run = runs[r]
        img = render_run(gs, places, place_rgba, run, run_clear[r], n, center, fill, bgr)
        oy, ox = int(run["out_y"]), int(run["out_x"])
        out[oy:oy + img.shape[0], ox:ox + img.shape[1]] = img
    return out
