"""A model of a bitmap fill's source pixel as cairo 1.16 hands the surface pattern to pixman 0.40 and as pixman fetches it, in Python
integers and numpy -- DESIGN.md, "Padded bitmap fills".  It shares no code with csrc; the matrices and the 16.16 transform are
tests/spread_model.py's (pattern_matrix, to_pixman: a surface pattern and a gradient go the same way to pixman).

    filter        _cairo_pattern_analyze_filter for CAIRO_FILTER_GOOD: bilinear unless an axis is minified below 0.75, then
                  create_separable_convolution's box (x) tent kernel per axis, 2^bits phases, 16.16 weights (filter_of)
    position      the 16.16 position of a pixel centre; bilinear: half a texel back, 7-bit weights; convolution: the middle of the
                  closest phase, the taps from its left-most one
    extend        what a tap outside the bitmap reads: NONE transparent black, REPEAT the coordinate modulo the size, PAD the
                  coordinate clamped -- per axis, so past a corner it is the corner texel

source() gives the source pixels (premultiplied 0xAARRGGBB) of a rectangle; where that rectangle is a pixel-aligned box filled on a
clear surface, they are what the frame holds (tests/test_pad_model.py holds that against libcairo).
"""
import math

import numpy as np

import spread_model as sm

NONE, REPEAT, PAD = 0, 1, 2                 # swfr_style::extend of a bitmap style (cairo_extend_t: NONE 0, REPEAT 1, PAD 3)
CAIRO_EXTEND = {NONE: 0, REPEAT: 1, PAD: 3}


def premultiply(rgba_straight):
    """(h, w, 4) straight RGBA bytes -> (h, w) premultiplied 0xAARRGGBB, as putImageData does it: c * a / 255, truncated"""
    s = np.asarray(rgba_straight).astype(np.uint32)
    a = s[..., 3]
    return (a << 24) | ((s[..., 0] * a // 255) << 16) | ((s[..., 1] * a // 255) << 8) | (s[..., 2] * a // 255)


def rgba_bytes(argb):
    """(h, w) 0xAARRGGBB -> (h, w, 4) bytes R, G, B, A: the layout of the frames the tests compare"""
    a = np.asarray(argb, np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], -1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the filter
def _use_bilinear(x, y, t):
    h = x * x + y * y                       # a row of the device -> pattern matrix
    if h < 1.0 / (0.75 * 0.75):
        return True
    # exactly 1/2, axis-parallel, at an integer offset: the box filter is then a bilinear sample (24.8 comparisons)
    return 3.99 < h < 4.01 and round(x * y * 256.0) == 0 and (round(t * 256.0) & 255) == 0


def _kernel(x, r):
    return max(0.0, min(min(r, 1.0), min((r + 1) / 2 - x, (r + 1) / 2 + x)))


def _axis(r):
    """(taps, bits, [phase][tap] 16.16 weights) of one axis minified r times"""
    width = 2 if r < 1.0 else int(math.ceil(r + 1))
    bits = 0
    while width > 1 and r * (1 << bits) <= 128.0:
        bits += 1
    table = []
    for i in range(1 << bits):
        frac = (i + .5) / (1 << bits)
        x1 = math.ceil(frac - width / 2.0 - 0.5) - frac + 0.5
        w = [int(_kernel(x1 + j, r) * 65536.0) for j in range(width)]
        total = 1 / sum(_kernel(x1 + j, r) for j in range(width))
        w = [int(v * total) for v in w]
        w[width // 2] += 65536 - sum(w)
        table.append(w)
    return width, bits, table


def filter_of(m):
    """None for the bilinear sample, else ((cw, xbits, x table), (ch, ybits, y table)); m: the pattern matrix (xx, yx, xy, yy, x0, y0)"""
    xx, yx, xy, yy, x0, y0 = m
    if _use_bilinear(xx, xy, x0) and _use_bilinear(yx, yy, y0):
        return None
    dx, dy = min(math.hypot(xx, xy), 16.0), min(math.hypot(yx, yy), 16.0)
    return _axis(1.0 if dx < 1.0 / 0.75 else dx), _axis(1.0 if dy < 1.0 / 0.75 else dy)


# ---------------------------------------------------------------------------------------------------------------- the fetch
def texel(bitmap, x, y, extend):
    h, w = bitmap.shape
    if extend == REPEAT:
        x, y = x % w, y % h
    elif extend == PAD:
        x, y = min(max(x, 0), w - 1), min(max(y, 0), h - 1)
    elif not (0 <= x < w and 0 <= y < h):
        return 0
    return int(bitmap[y, x])


def bilinear(bitmap, fx, fy, extend):
    """the pixel at the 16.16 position (fx, fy): pixman's bilinear interpolation with 7-bit weights"""
    bx, by = fx - 0x8000, fy - 0x8000
    x0, y0, wx, wy = bx >> 16, by >> 16, (bx >> 9) & 0x7f, (by >> 9) & 0x7f
    c = [texel(bitmap, x0 + (k & 1), y0 + (k >> 1), extend) for k in range(4)]
    w = [(128 - wx) * (128 - wy), wx * (128 - wy), (128 - wx) * wy, wx * wy]
    out = 0
    for sh in (0, 8, 16, 24):
        out |= ((sum(((c[k] >> sh) & 255) * w[k] for k in range(4)) >> 14) & 255) << sh
    return out


def convolution(bitmap, fx, fy, flt, extend):
    """pixman's bits_image_fetch_pixel_separable_convolution at the 16.16 position (fx, fy)"""
    (cw, xbits, xt), (ch, ybits, yt) = flt
    xsh, ysh = 16 - xbits, 16 - ybits
    x = (fx & ~((1 << xsh) - 1)) + ((1 << xsh) >> 1)
    y = (fy & ~((1 << ysh) - 1)) + ((1 << ysh) >> 1)
    xw, yw = xt[(x & 0xffff) >> xsh], yt[(y & 0xffff) >> ysh]
    x1, y1 = (x - 1 - (((cw << 16) - 65536) >> 1)) >> 16, (y - 1 - (((ch << 16) - 65536) >> 1)) >> 16
    acc = [0, 0, 0, 0]
    for i in range(ch):
        if not yw[i]:
            continue
        for j in range(cw):
            if not xw[j]:
                continue
            p = texel(bitmap, x1 + j, y1 + i, extend)
            f = (yw[i] * xw[j] + 0x8000) >> 16
            for k, sh in enumerate((0, 8, 16, 24)):
                acc[k] += ((p >> sh) & 255) * f
    out = 0
    for k, sh in enumerate((0, 8, 16, 24)):
        out |= min(max((acc[k] + 0x8000) >> 16, 0), 255) << sh
    return out


# ---------------------------------------------------------------------------------------------------------------- the fetch, on arrays
def texels(bitmap, x, y, extend):
    """texel() for int64 arrays of coordinates -> uint32"""
    h, w = bitmap.shape
    if extend == REPEAT:
        return bitmap[y % h, x % w]
    if extend == PAD:
        return bitmap[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
    ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    return np.where(ok, bitmap[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0).astype(np.uint32)


def bilinear_many(bitmap, fx, fy, extend):
    """bilinear() for int64 arrays of 16.16 positions (tests/test_shaded_frame_model.py holds the two equal)"""
    fx, fy = np.asarray(fx, np.int64), np.asarray(fy, np.int64)
    bx, by = fx - 0x8000, fy - 0x8000
    x0, y0, wx, wy = bx >> 16, by >> 16, (bx >> 9) & 0x7f, (by >> 9) & 0x7f
    c = [texels(bitmap, x0 + (k & 1), y0 + (k >> 1), extend).astype(np.int64) for k in range(4)]
    w = [(128 - wx) * (128 - wy), wx * (128 - wy), (128 - wx) * wy, wx * wy]
    out = np.zeros(fx.shape, np.int64)
    for sh in (0, 8, 16, 24):
        out |= ((sum(((c[k] >> sh) & 255) * w[k] for k in range(4)) >> 14) & 255) << sh
    return out.astype(np.uint32)


def convolution_many(bitmap, fx, fy, flt, extend):
    """convolution() for int64 arrays of 16.16 positions"""
    fx, fy = np.asarray(fx, np.int64), np.asarray(fy, np.int64)
    (cw, xbits, xt), (ch, ybits, yt) = flt
    xsh, ysh = 16 - xbits, 16 - ybits
    x = (fx & ~((1 << xsh) - 1)) + ((1 << xsh) >> 1)
    y = (fy & ~((1 << ysh) - 1)) + ((1 << ysh) >> 1)
    xw, yw = np.array(xt, np.int64)[(x & 0xffff) >> xsh], np.array(yt, np.int64)[(y & 0xffff) >> ysh]      # [..., tap]
    x1, y1 = (x - 1 - (((cw << 16) - 65536) >> 1)) >> 16, (y - 1 - (((ch << 16) - 65536) >> 1)) >> 16
    acc = [np.zeros(fx.shape, np.int64) for _ in range(4)]
    for i in range(ch):
        for j in range(cw):
            on = (yw[..., i] != 0) & (xw[..., j] != 0)
            if not on.any():
                continue
            p = texels(bitmap, x1 + j, y1 + i, extend).astype(np.int64)
            f = np.where(on, (yw[..., i] * xw[..., j] + 0x8000) >> 16, 0)
            for k, sh in enumerate((0, 8, 16, 24)):
                acc[k] += ((p >> sh) & 255) * f
    out = np.zeros(fx.shape, np.int64)
    for k, sh in enumerate((0, 8, 16, 24)):
        out |= np.clip((acc[k] + 0x8000) >> 16, 0, 255) << sh
    return out.astype(np.uint32)


def source_pixels(m, bitmap, rect, extend, anchor=None):
    """the source pixels (premultiplied 0xAARRGGBB) of the rectangle (x0, y0, x1, y1) for the pattern matrix m; `anchor`: the
    operation's rectangle where that is another (the rectangle cut to the frame is what is asked for)"""
    (bx, by), ((m00, m01), (m10, m11)) = sm.to_pixman(m, anchor or rect)
    px, py = np.meshgrid(np.arange(rect[0], rect[2], dtype=np.int64), np.arange(rect[1], rect[3], dtype=np.int64))
    fx, fy = bx + px * m00 + py * m01, by + px * m10 + py * m11
    flt = filter_of(m)
    return bilinear_many(bitmap, fx, fy, extend) if flt is None else convolution_many(bitmap, fx, fy, flt, extend)


def placement(bitmap, fx, fy, flt):
    """where a sample's taps lie: "inside" (every tap in the bitmap), "outside" (none) or "rim" -- taps of weight zero not counted"""
    h, w = bitmap.shape
    if flt is None:
        bx, by = fx - 0x8000, fy - 0x8000
        xs = [(bx >> 16) + k for k in (0, 1) if (128 - ((bx >> 9) & 0x7f), (bx >> 9) & 0x7f)[k]]
        ys = [(by >> 16) + k for k in (0, 1) if (128 - ((by >> 9) & 0x7f), (by >> 9) & 0x7f)[k]]
    else:
        (cw, xbits, xt), (ch, ybits, yt) = flt
        xsh, ysh = 16 - xbits, 16 - ybits
        x = (fx & ~((1 << xsh) - 1)) + ((1 << xsh) >> 1)
        y = (fy & ~((1 << ysh) - 1)) + ((1 << ysh) >> 1)
        x1, y1 = (x - 1 - (((cw << 16) - 65536) >> 1)) >> 16, (y - 1 - (((ch << 16) - 65536) >> 1)) >> 16
        xs = [x1 + j for j in range(cw) if xt[(x & 0xffff) >> xsh][j]]
        ys = [y1 + i for i in range(ch) if yt[(y & 0xffff) >> ysh][i]]
    inside = [0 <= x < w and 0 <= y < h for x in xs for y in ys]
    return "inside" if all(inside) else ("rim" if any(inside) else "outside")


def source(matrices, bitmap, rect, extend=PAD):
    """the source pixels of the operation's rectangle (x0, y0, x1, y1): {"pixels": (h, w) 0xAARRGGBB, "bilinear": the filter chosen,
    "placements": how many samples lie inside, on the rim of and outside the bitmap}.  matrices: swf-tree matrices, outermost first,
    the fill's own last; None for a singular one (nothing is painted)"""
    m = sm.pattern_matrix(matrices)
    if m is None:
        return None
    flt = filter_of(m)
    (bx, by), ((m00, m01), (m10, m11)) = sm.to_pixman(m, rect)
    x0, y0, x1, y1 = rect
    out = np.zeros((y1 - y0, x1 - x0), np.uint32)
    places = {"inside": 0, "rim": 0, "outside": 0}
    for py in range(y0, y1):
        for px in range(x0, x1):
            fx, fy = bx + px * m00 + py * m01, by + px * m10 + py * m11
            out[py - y0, px - x0] = bilinear(bitmap, fx, fy, extend) if flt is None else convolution(bitmap, fx, fy, flt, extend)
            places[placement(bitmap, fx, fy, flt)] += 1
    return {"pixels": out, "bilinear": flt is None, "placements": places}
