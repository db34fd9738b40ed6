"""A model of an unsmoothed bitmap fill -- the surface pattern with cairo_pattern_set_filter(CAIRO_FILTER_NEAREST) -- as cairo 1.16
hands it to pixman 0.40 and as pixman fetches it, in Python integers and numpy: DESIGN.md, "Unsmoothed bitmap fills".  It shares no
code with csrc; the matrices and the 16.16 transform are tests/spread_model.py's, the extends tests/pad_model.py's (texels).

    the fetch     with f = (fx, fy) the 16.16 position of a pixel centre, the ONE texel ((fx - 1) >> 16, (fy - 1) >> 16): pixman_fixed_e
                  back where the bilinear sample goes half a texel back.  At every scale: there is no convolution.
    texel edges   so a sample exactly on a texel edge (f & 0xffff == 0) reads the texel to the left of / above the edge.  floor(f)
                  -- floor_many below, the rule this must not be confused with -- reads the other one.
    the cut       an EXTEND_NONE fill is bounded by its source (_cairo_pattern_get_extents): the bitmap's rectangle padded by 0.004
                  source pixels per side, mapped to device space and rounded to the nearest pixel edge on both axes whatever the scale
                  (cut_rect).  CAIRO_FILTER_GOOD pads by half a source pixel on an axis it magnifies and rounds out on the others
                  (cut_rect(..., nearest=False): what the frame builder always did).  A repeating or padded fill is unbounded.

source() gives the source pixels (premultiplied 0xAARRGGBB) of a pixel-aligned box filled on a clear surface: what the frame holds
(tests/test_nearest_model.py holds that, and the cut, against libcairo).
"""
import math

import numpy as np

import pad_model as pm
import spread_model as sm

NONE, REPEAT, PAD = pm.NONE, pm.REPEAT, pm.PAD
GOOD, NEAREST = 0, 1                        # swfr_fill_style::filter, swfr_style::filter
CAIRO_FILTER = {GOOD: 1, NEAREST: 3}        # cairo_filter_t
premultiply, rgba_bytes = pm.premultiply, pm.rgba_bytes


# ---------------------------------------------------------------------------------------------------------------- the fetch
def nearest_many(bitmap, fx, fy, extend):
    """the pixels at the int64 arrays of 16.16 positions (fx, fy)"""
    fx, fy = np.asarray(fx, np.int64), np.asarray(fy, np.int64)
    return pm.texels(bitmap, (fx - 1) >> 16, (fy - 1) >> 16, extend).astype(np.uint32)


def floor_many(bitmap, fx, fy, extend):
    """the WRONG rule, for the generator's gate: floor(f), which takes the texel to the right of / below an edge"""
    fx, fy = np.asarray(fx, np.int64), np.asarray(fy, np.int64)
    return pm.texels(bitmap, fx >> 16, fy >> 16, extend).astype(np.uint32)


def positions(m, rect, anchor=None):
    """the 16.16 positions (fx, fy) of the pixel centres of the rectangle (x0, y0, x1, y1); `anchor`: the operation's rectangle"""
    (bx, by), ((m00, m01), (m10, m11)) = sm.to_pixman(m, anchor or rect)
    px, py = np.meshgrid(np.arange(rect[0], rect[2], dtype=np.int64), np.arange(rect[1], rect[3], dtype=np.int64))
    return bx + px * m00 + py * m01, by + px * m10 + py * m11


def source_pixels(m, bitmap, rect, extend, anchor=None, fetch=nearest_many):
    fx, fy = positions(m, rect, anchor)
    return fetch(bitmap, fx, fy, extend)


# ---------------------------------------------------------------------------------------------------------------- the cut
def _lround(v):
    return int(math.floor(v + 0.5))


def cut_rect(m, width, height, nearest=True, is_vector=False):
    """the device-space rectangle (x0, y0, x1, y1) an EXTEND_NONE fill of a width x height bitmap is cut to; m: the pattern matrix
    (device -> pattern space); None where m is singular.  is_vector: _cairo_pattern_get_extents' rule for a vector target -- an axis
    that rounds to nothing is given one pixel -- which is what a cairo_recording_surface, the probe of tests/test_nearest_model.py, is;
    an image surface, what the frames are drawn on, is none: there such a fill draws nothing"""
    sx0, sy0, sx1, sy1 = 0.0, 0.0, float(width), float(height)
    if nearest:
        sx0, sy0, sx1, sy1 = sx0 - 0.004, sy0 - 0.004, sx1 + 0.004, sy1 + 0.004
        round_x = round_y = True
    else:
        round_x, round_y = math.hypot(m[0], m[1]) < 1.0, math.hypot(m[2], m[3]) < 1.0
        if round_x:
            sx0, sx1 = sx0 - 0.5, sx1 + 0.5
        if round_y:
            sy0, sy1 = sy0 - 0.5, sy1 + 0.5
    im = sm.invert(m)
    if im is None:
        return None
    pts = [sm.apply(im, x, y) for x in (sx0, sx1) for y in (sy0, sy1)]
    x0, x1 = min(p[0] for p in pts), max(p[0] for p in pts)
    y0, y1 = min(p[1] for p in pts), max(p[1] for p in pts)
    if not round_x:
        x0, x1 = x0 - 0.5, x1 + 0.5
    if not round_y:
        y0, y1 = y0 - 0.5, y1 + 0.5
    ix0, iy0, ix1, iy1 = _lround(x0), _lround(y0), _lround(x1), _lround(y1)
    if is_vector:
        ix1, iy1 = ix1 + (ix1 == ix0 and x0 != x1), iy1 + (iy1 == iy0 and y0 != y1)
    return ix0, iy0, ix1, iy1


def intersect(a, b):
    r = (max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3]))
    return r if r[0] < r[2] and r[1] < r[3] else None


# ---------------------------------------------------------------------------------------------------------------- a box on a clear frame
def source(matrices, bitmap, rect, extend=NONE, fetch=nearest_many):
    """the source pixels of a pixel-aligned box (x0, y0, x1, y1) with an unsmoothed fill: {"rect": the operation's rectangle -- the box,
    under EXTEND_NONE cut to the bitmap's -- or None where nothing is drawn, "pixels": (h, w) 0xAARRGGBB of that rectangle,
    "placements": how many of its samples read a texel inside and outside the bitmap}.  matrices: swf-tree matrices, outermost first,
    the fill's own last; None for a singular one"""
    m = sm.pattern_matrix(matrices)
    if m is None:
        return None
    h, w = bitmap.shape
    op = intersect(rect, cut_rect(m, w, h)) if extend == NONE else tuple(rect)
    if op is None:
        return {"rect": None, "pixels": None, "placements": {"inside": 0, "outside": 0}}
    fx, fy = positions(m, op)
    x, y = (fx - 1) >> 16, (fy - 1) >> 16
    inside = int(((x >= 0) & (x < w) & (y >= 0) & (y < h)).sum())
    return {"rect": op, "pixels": fetch(bitmap, fx, fy, extend), "placements": {"inside": inside, "outside": x.size - inside}}


def frame(matrices, bitmap, rect, extend, width, height, fetch=nearest_many):
    """(the (height, width, 4) RGBA frame a clear surface holds after the box, source()'s result)"""
    out = np.zeros((height, width, 4), np.uint8)
    src = source(matrices, bitmap, rect, extend, fetch)
    if src is not None and src["rect"] is not None:
        x0, y0, x1, y1 = src["rect"]
        out[y0:y1, x0:x1] = rgba_bytes(src["pixels"])
    return out, src
