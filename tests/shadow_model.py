"""The shadow of a shadowed layer ("Shadowed layers") in numpy, over tests/blur_model.py's box blur, and the same through
libcairo 1.16 + pixman 0.40 themselves: the literal call sequence the rule is defined by.

A shadow is a dict with every key optional but "color": {"color": (r, g, b, a) straight bytes, "dx", "dy" whole pixels (0), "x", "y" the box
(0), "passes" (1), "strength" 1..255 (1), "hide_object", "knockout" (False)} -- the "shadow" value of the Python mirror.  From the group
surface G (premultiplied):

    2. S(x, y)  = Ga(x - dx, y - dy) in the alpha channel, 0 outside the image; the colour channels 0
    3. S        = blur(S, x, y, passes)
    4. Ta       = min(255, strength * Sa)
    5. Tc       = mul_un8(cp, Ta) per channel, cp = premultiplied_pixel(color)
    6. R        = Tc (hide_object) | mul_un8(Tc, 255 - Ga) (knockout) | G + mul_un8(Tc, 255 - Ga), saturating (neither)

tests/test_shadow_model.py holds shadow() against cairo_shadow() byte for byte.
"""
import ctypes

import numpy as np

import blur_model

KEYS = ("color", "dx", "dy", "x", "y", "passes", "strength", "hide_object", "knockout")


def values(sh):
    """(color, dx, dy, x, y, passes, strength, hide_object, knockout) with the defaults filled in"""
    assert not set(sh) - set(KEYS), sh
    return (tuple(int(c) for c in sh["color"]), int(sh.get("dx", 0)), int(sh.get("dy", 0)), int(sh.get("x", 0)), int(sh.get("y", 0)),
            int(sh.get("passes", 1)), int(sh.get("strength", 1)), bool(sh.get("hide_object", False)), bool(sh.get("knockout", False)))


def as_dict(sh):
    """the shadow with every key: what Renderer.built_layers() reports"""
    return dict(zip(KEYS, values(sh)))


# the cases the model is held against libcairo with, and the kernels against the model (tests/test_shadow_model.py, tests/test_shadow_gpu.py)
STRENGTHS = (1, 2, 3, 255)
COLORS = {"opaque": (200, 30, 90, 255), "translucent": (20, 160, 255, 117), "clear": (255, 255, 255, 0)}
FLAGS = {"over": {}, "hide": {"hide_object": True}, "knockout": {"knockout": True}}


def offsets(w, h):
    """no shift, two in-frame shifts, everything shifted out, one pixel left"""
    return ((0, 0), (3, -2), (-5, 4), (w, 0), (-(w - 1), h - 1))


def premultiplied_pixel(color):
    """(r, g, b, a) premultiplied bytes of cairo_set_source_rgba(r / 255, g / 255, b / 255, a / 255): cairo's _cairo_color_compute_shorts
    (each of r * a, g * a, b * a, a in doubles, times 65535 plus a half, to 16 bits) and the >> 8 of its pixman solid image"""
    r, g, b, a = (c / 255.0 for c in color)

    def short(v):
        return (int(v * 65535.0 + 0.5) & 0xffff) >> 8
    return short(r * a), short(g * a), short(b * a), short(a)


def mul_un8(x, a):
    """pixman's MUL_UN8 on int64 arrays: (t + (t >> 8)) >> 8 with t = x * a + 0x80"""
    t = x * a + 0x80
    return (t + (t >> 8)) >> 8


def shifted_alpha(alpha, dx, dy):
    """S's alpha of step 2: alpha(x - dx, y - dy), 0 outside"""
    h, w = alpha.shape
    out = np.zeros_like(alpha)
    if abs(dx) < w and abs(dy) < h:
        out[max(0, dy):min(h, h + dy), max(0, dx):min(w, w + dx)] = alpha[max(0, -dy):min(h, h - dy), max(0, -dx):min(w, w - dx)]
    return out


def shadow(img, sh, order="rgba"):
    """the final surface R of an HxWx4 uint8 premultiplied group image whose bytes are in `order` ("rgba": a frame as read back; "bgra":
    the bytes of ARGB words); alpha is byte 3 in both"""
    color, dx, dy, bx, by, passes, strength, hide, knockout = values(sh)
    assert not (hide and knockout)
    r, g, b, a = premultiplied_pixel(color)
    cp = np.array((r, g, b, a) if order == "rgba" else (b, g, r, a), np.int64)
    s = shifted_alpha(img[..., 3], dx, dy)
    s = blur_model.blur(s[..., None], bx, by, passes)[..., 0]
    ta = np.minimum(255, strength * s.astype(np.int64))
    tc = mul_un8(cp[None, None, :], ta[..., None])
    if hide:
        return tc.astype(np.uint8)
    under = mul_un8(tc, 255 - img[..., 3:].astype(np.int64))
    if knockout:
        return under.astype(np.uint8)
    return np.minimum(255, img.astype(np.int64) + under).astype(np.uint8)


# ---- libcairo + pixman (the yardstick): the rule's call sequence on image surfaces
CAIRO_FORMAT_ARGB32 = 0
CAIRO_OPERATOR_OVER, CAIRO_OPERATOR_DEST_OUT, CAIRO_OPERATOR_ADD = 2, 9, 12
_cairo = None


def cairo():
    """libcairo through ctypes with the signatures cairo_shadow needs"""
    global _cairo
    if _cairo is None:
        from oracle import cairo_backend as cb
        lib = cb._load()
        P, D, I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
        for fn, res, args in (("cairo_mask_surface", None, [P, P, D, D]), ("cairo_set_source_surface", None, [P, P, D, D]), ("cairo_paint", None, [P]),
                              ("cairo_surface_status", I, [P])):
            f = getattr(lib, fn)
            f.restype, f.argtypes = res, args
        _cairo = lib
    return _cairo


class _Surface:
    """an ARGB32 image surface over a numpy array of words, with a context"""

    def __init__(self, lib, words):
        self.lib = lib
        self.words = np.ascontiguousarray(words, dtype=np.uint32).copy()
        h, w = self.words.shape
        self.surf = lib.cairo_image_surface_create_for_data(self.words.ctypes.data, CAIRO_FORMAT_ARGB32, w, h, w * 4)
        assert lib.cairo_surface_status(self.surf) == 0
        self.cr = lib.cairo_create(self.surf)

    def flush(self):
        self.lib.cairo_surface_flush(self.surf)
        return self.words

    def close(self):
        self.lib.cairo_destroy(self.cr)
        self.lib.cairo_surface_destroy(self.surf)


def cairo_shadow(words, sh):
    """the final surface R of an HxW uint32 image of premultiplied ARGB words, by libcairo and pixman: steps 2 to 6 as the calls the rule
    names, every surface of the image's size"""
    lib = cairo()
    color, dx, dy, bx, by, passes, strength, hide, knockout = values(sh)
    assert not (hide and knockout)
    clear = np.zeros_like(np.asarray(words, dtype=np.uint32))
    G, S, T, Tc = _Surface(lib, words), _Surface(lib, clear), _Surface(lib, clear), _Surface(lib, clear)
    try:
        # 2. the alpha surface
        lib.cairo_set_source_rgba(S.cr, 0.0, 0.0, 0.0, 1.0)
        lib.cairo_mask_surface(S.cr, G.surf, float(dx), float(dy))
        # 3. the blur, on the surface's own words
        view = S.flush()
        view[:] = blur_model.pixman_blur(view.copy(), bx, by, passes)
        lib.cairo_surface_mark_dirty(S.surf)
        # 4. the strength: n ADD paints
        lib.cairo_set_operator(T.cr, CAIRO_OPERATOR_ADD)
        for _ in range(strength):
            lib.cairo_set_source_surface(T.cr, S.surf, 0.0, 0.0)
            lib.cairo_paint(T.cr)
        T.flush()
        # 5. the tint
        r, g, b, a = color
        lib.cairo_set_source_rgba(Tc.cr, r / 255.0, g / 255.0, b / 255.0, a / 255.0)
        lib.cairo_mask_surface(Tc.cr, T.surf, 0.0, 0.0)
        # 6. the group over it, out of it, or not at all
        if not hide:
            lib.cairo_set_operator(Tc.cr, CAIRO_OPERATOR_DEST_OUT if knockout else CAIRO_OPERATOR_OVER)
            lib.cairo_set_source_surface(Tc.cr, G.surf, 0.0, 0.0)
            lib.cairo_paint(Tc.cr)
        assert lib.cairo_status(Tc.cr) == 0 and lib.cairo_status(T.cr) == 0 and lib.cairo_status(S.cr) == 0
        return Tc.flush().copy()
    finally:
        for s in (Tc, T, S, G):
            s.close()
