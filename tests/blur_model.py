"""The box blur of a blurred layer ("Blurred layers") in numpy, and the same through pixman 0.40 itself.

One 1-D pass of box width w (1..255) over an image of premultiplied pixels, any channel order (every channel, alpha included, is
treated alike): w = 1 is the identity; otherwise, with f = (65536 + w // 2) // w and S the plain sum of a channel's bytes over the
window [x - w // 2, x - w // 2 + w - 1], a tap outside the image reading 0,

    out = min(255, (f * S + 0x8000) >> 16)

which is what pixman computes for PIXMAN_FILTER_CONVOLUTION with w equal taps of f (pixman-bits-image.c,
bits_image_fetch_pixel_convolution: the taps' products summed in 16.16, 0x8000 added, >> 16, clipped to 0..255) composited with SRC
from an image of EXTEND_NONE.  A blur (bx, by, passes) is `passes` times a horizontal pass of width max(1, bx), then a vertical pass
of width max(1, by).  tests/test_blur_model.py holds box_pass against pixman_blur byte for byte.
"""
import ctypes
import ctypes.util

import numpy as np


def box_pass(img, w, axis):
    """one pass of box width w along `axis` (1: horizontal, 0: vertical) of an HxWxC uint8 image"""
    w = int(w)
    if not 1 <= w <= 255:
        raise ValueError("box width must be 1..255")
    if w == 1:
        return img.copy()
    f = (65536 + w // 2) // w
    a = np.moveaxis(img.astype(np.int64), axis, 0)
    n = a.shape[0]
    c = np.concatenate([np.zeros((1,) + a.shape[1:], np.int64), np.cumsum(a, axis=0)], axis=0)      # c[i] = sum of a[:i]
    lo = np.clip(np.arange(n) - w // 2, 0, n)
    hi = np.clip(np.arange(n) - w // 2 + w, 0, n)
    s = c[hi] - c[lo]
    out = np.minimum(255, (f * s + 0x8000) >> 16).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def blur(img, bx, by, passes=1):
    """the blur (bx, by, passes) of an HxWxC uint8 image"""
    out = img.copy()
    for _ in range(int(passes)):
        out = box_pass(out, max(1, int(bx)), 1)
        out = box_pass(out, max(1, int(by)), 0)
    return out


# ---- pixman itself (the yardstick): one pixman_image_composite32(SRC) per pass from an image carrying the convolution filter
PIXMAN_a8r8g8b8 = 0x20028888
PIXMAN_OP_SRC = 1
PIXMAN_FILTER_CONVOLUTION = 5
_pixman = None


def pixman():
    """libpixman-1 through ctypes, or None when the machine has none"""
    global _pixman
    if _pixman is None:
        name = ctypes.util.find_library("pixman-1")
        try:
            lib = ctypes.CDLL(name) if name else False
        except OSError:
            lib = False
        if lib:
            P, I = ctypes.c_void_p, ctypes.c_int
            lib.pixman_image_create_bits.restype, lib.pixman_image_create_bits.argtypes = P, [I, I, I, P, I]
            lib.pixman_image_set_filter.restype, lib.pixman_image_set_filter.argtypes = I, [P, I, P, I]
            lib.pixman_image_composite32.restype = None
            lib.pixman_image_composite32.argtypes = [I, P, P, P] + [ctypes.c_int32] * 8
            lib.pixman_image_unref.restype, lib.pixman_image_unref.argtypes = I, [P]
            lib.pixman_version_string.restype = ctypes.c_char_p
        _pixman = lib
    return _pixman or None


def pixman_pass(words, w, axis):
    """one pass of box width w over an HxW uint32 image of ARGB words, by pixman"""
    lib = pixman()
    if w == 1:
        return words.copy()
    h, wd = words.shape
    src = np.ascontiguousarray(words, dtype=np.uint32)
    dst = np.zeros_like(src)
    f = (65536 + w // 2) // w
    kw, kh = (w, 1) if axis == 1 else (1, w)
    params = (ctypes.c_int32 * (2 + w))(kw << 16, kh << 16, *([f] * w))
    si = lib.pixman_image_create_bits(PIXMAN_a8r8g8b8, wd, h, src.ctypes.data, wd * 4)
    di = lib.pixman_image_create_bits(PIXMAN_a8r8g8b8, wd, h, dst.ctypes.data, wd * 4)
    try:
        assert lib.pixman_image_set_filter(si, PIXMAN_FILTER_CONVOLUTION, ctypes.cast(params, ctypes.c_void_p), 2 + w)
        lib.pixman_image_composite32(PIXMAN_OP_SRC, si, None, di, 0, 0, 0, 0, 0, 0, wd, h)
    finally:
        lib.pixman_image_unref(si)
        lib.pixman_image_unref(di)
    return dst


def pixman_blur(words, bx, by, passes=1):
    """the blur (bx, by, passes) of an HxW uint32 image of premultiplied ARGB words, pass by pass through pixman"""
    out = np.ascontiguousarray(words, dtype=np.uint32).copy()
    for _ in range(int(passes)):
        out = pixman_pass(out, max(1, int(bx)), 1)
        out = pixman_pass(out, max(1, int(by)), 0)
    return out


def words_to_bytes(words):
    """HxW ARGB words -> HxWx4 bytes (b, g, r, a: the little-endian order in memory; the blur treats every channel alike)"""
    return np.ascontiguousarray(words, dtype="<u4").view(np.uint8).reshape(words.shape + (4,))


def bytes_to_words(img):
    return np.ascontiguousarray(img, dtype=np.uint8).view("<u4").reshape(img.shape[:2])


def random_premultiplied(rng, h, w):
    """HxW premultiplied ARGB words: random colours under random alphas, with an opaque run and a clear run in every other row"""
    a = rng.integers(0, 256, (h, w)).astype(np.uint32)
    for y in range(0, h, 2):
        x0 = int(rng.integers(0, w))
        a[y, x0:x0 + max(1, w // 3)] = 255
        x1 = int(rng.integers(0, w))
        a[y, x1:x1 + max(1, w // 4)] = 0
    ch = [(rng.integers(0, 256, (h, w)).astype(np.uint32) * a + 127) // 255 for _ in range(3)]
    return (a << 24) | (ch[0] << 16) | (ch[1] << 8) | ch[2]
