"""The convolution of a filtered layer ("Convolution filters") in numpy, and the same through pixman 0.40 itself.

A kernel is `height` rows of `width` taps, each dimension 1..7, every tap a signed 16.16 integer, sum |tap| <= 8 388 607.  Over an image
of premultiplied pixels, any channel order (every channel, alpha included, is treated alike):

    S = sum_j sum_i tap[j][i] * c(x - width // 2 + i, y - height // 2 + j) + 0x8000
    out(x, y) = 255 if S < 0 else min(255, S >> 16)

with a tap outside the image reading 0: what pixman computes for PIXMAN_FILTER_CONVOLUTION with these taps (pixman-bits-image.c,
bits_image_fetch_pixel_convolution with accum_32 / reduce_32: the taps' products summed in UNSIGNED 32-bit integers, 0x8000 added,
divided by 65536, clipped to 0..255 -- a negative sum is a number of 2^31 or more there and clips to 255, not to 0; the live library
decides, and this is what it does) composited with SRC from an image of EXTEND_NONE.  The window sits where blur_model's box sits.  tests/test_convolution_model.py holds convolve() against
pixman_convolve() byte for byte.

A "convolution" value is a dict with "taps" (rows of 16.16 integers) or with "matrix" (rows of numbers) and an optional "divisor"
(absent: 1): tap = floor(m * 65536 / divisor + 0.5).  In a filter list it is the entry {"convolution": value}; apply(), cairo_apply() and
as_dicts() dispatch: such an entry goes to the rule here, everything else to inner_model (and through it to filter_model and
shadow_model) unchanged.
"""
import ctypes
import math

import numpy as np

import blur_model
import filter_model
import inner_model

MAX_DIM = 7
MAX_ABS_SUM = 8388607
MAX_FILTERS = filter_model.MAX_FILTERS


def taps_of(value):
    """the rows of 16.16 integer taps of a "convolution" value"""
    assert isinstance(value, dict) and ("taps" in value) != ("matrix" in value), value
    if "taps" in value:
        assert "divisor" not in value
        rows = [[int(t) for t in row] for row in value["taps"]]
    else:
        div = value.get("divisor", 1)
        rows = [[int(math.floor(float(m) * 65536.0 / float(div) + 0.5)) for m in row] for row in value["matrix"]]
    assert 1 <= len(rows) <= MAX_DIM and 1 <= len(rows[0]) <= MAX_DIM and all(len(r) == len(rows[0]) for r in rows), value
    return rows


def in_range(rows):
    return sum(abs(t) for r in rows for t in r) <= MAX_ABS_SUM


def as_dict(value):
    """the value as Renderer.built_filters() reports it: its taps"""
    return {"taps": taps_of(value)}


def convolve(img, value):
    """the convolution of an HxWxC (or HxW) uint8 image with a "convolution" value"""
    rows = taps_of(value)
    assert in_range(rows), "the kernel is beyond the bound: refused, never wrapped"
    kh, kw = len(rows), len(rows[0])
    a = np.asarray(img, dtype=np.uint8)
    flat = a.ndim == 2
    if flat:
        a = a[..., None]
    h, w = a.shape[:2]
    ax, ay = kw // 2, kh // 2
    padded = np.zeros((h + kh - 1, w + kw - 1, a.shape[2]), np.int64)
    padded[ay:ay + h, ax:ax + w] = a
    acc = np.full(a.shape, 0x8000, np.int64)
    for j in range(kh):
        for i in range(kw):
            if rows[j][i]:
                acc += rows[j][i] * padded[j:j + h, i:i + w]
    assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31, "the 32-bit sum is exact inside the bound"
    out = np.where(acc < 0, 255, np.minimum(255, acc >> 16)).astype(np.uint8)      # (pixman's unsigned sums: negative clips at the top)
    return np.ascontiguousarray(out[..., 0] if flat else out)


def pixman_convolve(words, value):
    """the convolution of an HxW uint32 image of ARGB words, by pixman: one pixman_image_composite32(SRC) from an image carrying the
    filter (as blur_model.pixman_pass)"""
    lib = blur_model.pixman()
    rows = taps_of(value)
    kh, kw = len(rows), len(rows[0])
    h, wd = words.shape
    src = np.ascontiguousarray(words, dtype=np.uint32)
    dst = np.zeros_like(src)
    flat = [t for r in rows for t in r]
    params = (ctypes.c_int32 * (2 + len(flat)))(kw << 16, kh << 16, *flat)
    si = lib.pixman_image_create_bits(blur_model.PIXMAN_a8r8g8b8, wd, h, src.ctypes.data, wd * 4)
    di = lib.pixman_image_create_bits(blur_model.PIXMAN_a8r8g8b8, wd, h, dst.ctypes.data, wd * 4)
    try:
        assert lib.pixman_image_set_filter(si, blur_model.PIXMAN_FILTER_CONVOLUTION, ctypes.cast(params, ctypes.c_void_p), 2 + len(flat))
        lib.pixman_image_composite32(blur_model.PIXMAN_OP_SRC, si, None, di, 0, 0, 0, 0, 0, 0, wd, h)
    finally:
        lib.pixman_image_unref(si)
        lib.pixman_image_unref(di)
    return dst


# ---- the list model
def kind_of(entry):
    """("blur" | "shadow" | "convolution", its value) of one entry"""
    assert isinstance(entry, dict) and len(entry) == 1, entry
    (kind, value), = entry.items()
    assert kind in ("blur", "shadow", "convolution"), entry
    return kind, value


def as_dicts(filters):
    """the list with every key of every entry filled in: what Renderer.built_filters() reports"""
    return [{"convolution": as_dict(kind_of(e)[1])} if kind_of(e)[0] == "convolution" else inner_model.as_dicts([e])[0] for e in filters]


def apply(img, filters, order="rgba"):
    """R_n of an HxWx4 uint8 premultiplied group image whose bytes are in `order` (the rule here is blind to it; shadow_model.shadow)"""
    assert 1 <= len(filters) <= MAX_FILTERS
    out = np.ascontiguousarray(img, dtype=np.uint8)
    for entry in filters:
        kind, value = kind_of(entry)
        out = convolve(out, value) if kind == "convolution" else inner_model.apply(out, [entry], order)
    return out


def cairo_apply(words, filters):
    """R_n of an HxW uint32 image of premultiplied ARGB words, every step by libcairo and pixman"""
    assert 1 <= len(filters) <= MAX_FILTERS
    out = np.ascontiguousarray(words, dtype=np.uint32).copy()
    for entry in filters:
        kind, value = kind_of(entry)
        out = pixman_convolve(out, value) if kind == "convolution" else inner_model.cairo_apply(out, [entry])
    return out


def convolution(value=None, **kw):
    return {"convolution": dict(value or {}, **kw)}


# ---- the kernels the scenes, goldens and device tests share
SHARPEN = {"matrix": [[0, -1, 0], [-1, 5, -1], [0, -1, 0]]}
EMBOSS = {"matrix": [[-2, -1, 0], [-1, 1, 1], [0, 1, 2]]}
EDGE = {"matrix": [[-1, -1, -1], [-1, 8, -1], [-1, -1, -1]]}                 # (tap sum 0)
BOX3 = {"matrix": [[1, 1, 1]] * 3, "divisor": 9}
GAUSS5 = {"matrix": [[1, 4, 6, 4, 1], [4, 16, 24, 16, 4], [6, 24, 36, 24, 6], [4, 16, 24, 16, 4], [1, 4, 6, 4, 1]], "divisor": 256}
MOTION_7X1 = {"matrix": [[1, 1, 1, 1, 1, 1, 1]], "divisor": 7}
MOTION_1X7 = {"matrix": [[1]] * 7, "divisor": 7}
EVEN_2X2 = {"matrix": [[1, 2], [3, -1]], "divisor": 5}
EVEN_4X6 = {"matrix": [[1, 0, -1, 2], [0, 2, 1, 0], [-1, 1, 3, 1], [2, 0, 1, -1], [0, 1, 0, 1], [1, -1, 2, 0]], "divisor": 16}
IDENTITY = {"taps": [[65536]]}
NAMED = {"sharpen": SHARPEN, "emboss": EMBOSS, "edge": EDGE, "box3": BOX3, "gauss5": GAUSS5, "motion_7x1": MOTION_7X1, "motion_1x7": MOTION_1X7,
         "even_2x2": EVEN_2X2, "even_4x6": EVEN_4X6}


def random_kernel(rng, kw, kh, kind="signed"):
    """a kw x kh "convolution" value of random taps: "signed" (some of them zero), "bound" (sum |tap| exactly MAX_ABS_SUM), "negative" (every
    tap below zero), "zero" (every tap zero), "sparse" (most taps zero)"""
    n = kw * kh
    if kind == "zero":
        t = np.zeros(n, np.int64)
    elif kind == "bound":
        mag = rng.integers(1, 1 << 20, n).astype(np.int64)
        mag = mag * MAX_ABS_SUM // int(mag.sum())
        mag[0] += MAX_ABS_SUM - int(mag.sum())
        t = mag * rng.choice([-1, 1], n)
        assert int(np.abs(t).sum()) == MAX_ABS_SUM
    elif kind == "negative":
        t = -rng.integers(1, 3 * 65536 // n + 2, n).astype(np.int64)
    else:
        t = rng.integers(-2 * 65536, 2 * 65536 + 1, n).astype(np.int64)
        t[rng.random(n) < (0.75 if kind == "sparse" else 0.2)] = 0
    return {"taps": [[int(v) for v in t[j * kw:(j + 1) * kw]] for j in range(kh)]}
