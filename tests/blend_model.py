"""The blend-mode rule ("Blend modes") in numpy: what one path leaves in a pixel under each of the eight operators.

    result = combine_<operator>(s, d),   s = mul_un8(c, cov) per channel

with c the premultiplied source pixel, cov the path's 8-bit coverage of the pixel, d the premultiplied destination -- pixman's
unified combiners.  Channels last, any order (the alpha channel is index 3).  tests/test_blend_model.py checks it against libcairo.
"""
import numpy as np

MODES = {"multiply": 3, "screen": 4, "lighten": 5, "darken": 6, "difference": 7, "add": 8, "overlay": 13, "hardlight": 14}
REFUSED = {"layer": 2, "subtract": 9, "invert": 10, "alpha": 11, "erase": 12}
# swfr_path::lerp >> 8 (swfr.h SWFR_OP_*)
OPERATORS = {"over": 0, "multiply": 1, "screen": 2, "lighten": 3, "darken": 4, "difference": 5, "add": 6, "overlay": 7, "hardlight": 8}
# cairo_operator_t
CAIRO_OPERATORS = {"normal": 2, "multiply": 14, "screen": 15, "overlay": 16, "darken": 17, "lighten": 18, "hardlight": 21,
                   "difference": 23, "add": 12}


def _i(x):
    return np.asarray(x).astype(np.int64)


def div1(x):
    x = _i(x) + 0x80
    return (x + (x >> 8)) >> 8


def mul_un8(x, a):
    return div1(_i(x) * _i(a))


def source_pixel(r8, g8, b8, a8):
    """cairo_set_source_rgba(r/255, g/255, b/255, a/255) as an 8-bit premultiplied pixel (R, G, B, A): doubles, 16-bit shorts, >> 8"""
    r, g, b, a = (np.asarray(v, np.float64) / 255.0 for v in (r8, g8, b8, a8))

    def sh(v):
        return ((v * 65535.0 + 0.5).astype(np.int64) & 0xffff) >> 8
    return np.stack([sh(r * a), sh(g * a), sh(b * a), sh(a)], -1).astype(np.uint8)


def lerp_source(c, cov, d):
    """Cairo's SOURCE with a coverage mask (0x7f rounding): what OVER and ADD become on a still-clear surface"""
    c, d, a = _i(c), _i(d), _i(cov)[..., None]

    def m(x, f):
        t = x * f + 0x7f
        return (t + (t >> 8)) >> 8
    return np.minimum(m(c, a) + m(d, 255 - a), 255).astype(np.uint8)


def blend(mode, c, cov, d):
    """(..., 4) uint8: the pixel after a path of source pixel `c` (..., 4) and coverage `cov` (...) is blended into `d` (..., 4)"""
    s = mul_un8(c, _i(cov)[..., None])
    d = _i(d)
    sa, da = s[..., 3:4], d[..., 3:4]
    if mode == "normal":
        out = np.minimum(mul_un8(d, 255 - sa) + s, 255)
    elif mode == "add":
        out = np.minimum(d + s, 255)
    elif mode == "multiply":
        out = np.minimum(mul_un8(d, s) + np.minimum(mul_un8(s, 255 - da) + mul_un8(d, 255 - sa), 255), 255)
    else:
        if mode == "screen":
            b = s * da + d * sa - s * d
        elif mode == "darken":
            b = np.minimum(s * da, d * sa)
        elif mode == "lighten":
            b = np.maximum(s * da, d * sa)
        elif mode == "difference":
            b = np.abs(d * sa - s * da)
        elif mode == "overlay":
            b = np.where(2 * d < da, 2 * s * d, sa * da - 2 * (da - d) * (sa - s))
        elif mode == "hardlight":
            b = np.where(2 * s < sa, 2 * s * d, sa * da - 2 * (da - d) * (sa - s))
        else:
            raise ValueError(mode)
        out = div1(np.clip((255 - sa) * d + (255 - da) * s + b, 0, 65025))
        out[..., 3:4] = div1(np.clip(255 * da + 255 * sa - sa * da, 0, 65025))
    return out.astype(np.uint8)
