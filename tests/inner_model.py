"""The inner shadow of a shadowed layer ("Inner shadows") in numpy, over tests/blur_model.py's box blur and tests/shadow_model.py's
helpers, and the same through libcairo 1.16 + pixman 0.40 themselves: the literal call sequence the rule is defined by.

An inner shadow is a shadow_model shadow with one more key, "inner": True; "hide_object" is not offered with it.  From the group surface G
(premultiplied):

    2'. S(x, y) = 255 - Ga(x - dx, y - dy) in the alpha channel, 255 where that pixel lies outside the image; the colour channels 0
    3.  S       = blur(S, x, y, passes)
    4.  Ta      = min(255, strength * Sa)
    5.  Tc      = mul_un8(cp, Ta) per channel, cp = premultiplied_pixel(color)
    6'. R       = mul_un8(Tc, Ga) (knockout) | mul_un8(Tc, Ga) + mul_un8(G, 255 - Tca), saturating (not)

shadow(), apply(), cairo_apply() and as_dict() dispatch: a dict with a true "inner" goes to the rule here, everything else to
shadow_model and filter_model unchanged.  tests/test_inner_model.py holds inner_shadow() against cairo_inner_shadow() byte for byte.
"""
import numpy as np

import blur_model
import filter_model
import shadow_model
from shadow_model import mul_un8, premultiplied_pixel

CAIRO_OPERATOR_ATOP, CAIRO_OPERATOR_DEST_IN = 5, 8
MAX_FILTERS = filter_model.MAX_FILTERS


def is_inner(sh):
    return bool(sh.get("inner", False))


def outer_of(sh):
    """the shadow without its "inner" key: what shadow_model's helpers take"""
    return {k: v for k, v in sh.items() if k != "inner"}


def values(sh):
    """shadow_model.values of an inner shadow, which hides no object"""
    assert is_inner(sh) and isinstance(sh["inner"], (bool, np.bool_)), sh
    v = shadow_model.values(outer_of(sh))
    assert not v[7], "an inner shadow has no hide_object"
    return v


def as_dict(sh):
    """the shadow with every key, "inner" only where it is set: what Renderer.built_layers() reports"""
    d = shadow_model.as_dict(outer_of(sh))
    if is_inner(sh):
        d["inner"] = True
    return d


def as_dicts(filters):
    """filter_model.as_dicts with as_dict above for the shadows"""
    out = []
    for entry in filters:
        kind, value = filter_model.kind_of(entry)
        out.append({"shadow": as_dict(value)} if kind == "shadow" else filter_model.as_dicts([entry])[0])
    return out


def inverse_alpha(alpha, dx, dy):
    """S's alpha of step 2': 255 - alpha(x - dx, y - dy), 255 outside"""
    return (255 - shadow_model.shifted_alpha(alpha, dx, dy).astype(np.int64)).astype(np.uint8)


def inner_shadow(img, sh, order="rgba"):
    """the final surface R of an HxWx4 uint8 premultiplied group image whose bytes are in `order` (shadow_model.shadow)"""
    color, dx, dy, bx, by, passes, strength, _, knockout = values(sh)
    r, g, b, a = premultiplied_pixel(color)
    cp = np.array((r, g, b, a) if order == "rgba" else (b, g, r, a), np.int64)
    s = inverse_alpha(img[..., 3], dx, dy)
    s = blur_model.blur(s[..., None], bx, by, passes)[..., 0]
    ta = np.minimum(255, strength * s.astype(np.int64))
    tc = mul_un8(cp[None, None, :], ta[..., None])
    inside = mul_un8(tc, img[..., 3:].astype(np.int64))
    if knockout:
        return inside.astype(np.uint8)
    return np.minimum(255, inside + mul_un8(img.astype(np.int64), 255 - tc[..., 3:])).astype(np.uint8)


def shadow(img, sh, order="rgba"):
    return inner_shadow(img, sh, order) if is_inner(sh) else shadow_model.shadow(img, outer_of(sh), order)


def apply(img, filters, order="rgba"):
    """filter_model.apply with the inner rule for the entries that ask for it"""
    assert 1 <= len(filters) <= MAX_FILTERS
    out = np.ascontiguousarray(img, dtype=np.uint8)
    for entry in filters:
        kind, value = filter_model.kind_of(entry)
        out = inner_shadow(out, value, order) if kind == "shadow" and is_inner(value) else filter_model.apply(out, [entry], order)
    return out


# ---- libcairo + pixman (the yardstick)
def cairo():
    """shadow_model.cairo(): its signatures (cairo_paint, cairo_mask_surface, cairo_set_source_surface) and the backend's own
    (cairo_set_operator, cairo_set_source_rgba) are all the sequence below calls"""
    return shadow_model.cairo()


def cairo_inverse_alpha(words, dx, dy):
    """step 2' alone: the surface S of an HxW uint32 image of premultiplied ARGB words"""
    lib = cairo()
    G, S = shadow_model._Surface(lib, words), shadow_model._Surface(lib, np.zeros_like(np.asarray(words, dtype=np.uint32)))
    try:
        _inverse_alpha_calls(lib, S, G, dx, dy)
        assert lib.cairo_status(S.cr) == 0
        return S.flush().copy()
    finally:
        S.close(), G.close()


def _inverse_alpha_calls(lib, S, G, dx, dy):
    lib.cairo_set_source_rgba(S.cr, 0.0, 0.0, 0.0, 1.0)
    lib.cairo_paint(S.cr)
    lib.cairo_set_operator(S.cr, shadow_model.CAIRO_OPERATOR_DEST_OUT)
    lib.cairo_mask_surface(S.cr, G.surf, float(dx), float(dy))


def cairo_inner_shadow(words, sh):
    """the final surface R of an HxW uint32 image of premultiplied ARGB words, by libcairo and pixman: steps 2' to 6' as the calls the
    rule names, every surface of the image's size"""
    lib = cairo()
    color, dx, dy, bx, by, passes, strength, _, knockout = values(sh)
    clear = np.zeros_like(np.asarray(words, dtype=np.uint32))
    Sf = shadow_model._Surface
    G, S, T, Tc, R = Sf(lib, words), Sf(lib, clear), Sf(lib, clear), Sf(lib, clear), Sf(lib, words)
    try:
        # 2'. the inverse alpha surface
        _inverse_alpha_calls(lib, S, G, dx, dy)
        # 3. the blur, on the surface's own words
        view = S.flush()
        view[:] = blur_model.pixman_blur(view.copy(), bx, by, passes)
        lib.cairo_surface_mark_dirty(S.surf)
        # 4. the strength: n ADD paints
        lib.cairo_set_operator(T.cr, shadow_model.CAIRO_OPERATOR_ADD)
        for _ in range(strength):
            lib.cairo_set_source_surface(T.cr, S.surf, 0.0, 0.0)
            lib.cairo_paint(T.cr)
        T.flush()
        # 5. the tint
        r, g, b, a = color
        lib.cairo_set_source_rgba(Tc.cr, r / 255.0, g / 255.0, b / 255.0, a / 255.0)
        lib.cairo_mask_surface(Tc.cr, T.surf, 0.0, 0.0)
        # 6'. the tint atop the group, or the tint inside the group alone
        if knockout:
            lib.cairo_set_operator(Tc.cr, CAIRO_OPERATOR_DEST_IN)
            lib.cairo_set_source_surface(Tc.cr, G.surf, 0.0, 0.0)
            lib.cairo_paint(Tc.cr)
            out = Tc
        else:
            Tc.flush()
            lib.cairo_set_operator(R.cr, CAIRO_OPERATOR_ATOP)
            lib.cairo_set_source_surface(R.cr, Tc.surf, 0.0, 0.0)
            lib.cairo_paint(R.cr)
            out = R
        assert lib.cairo_status(R.cr) == 0 and lib.cairo_status(Tc.cr) == 0 and lib.cairo_status(T.cr) == 0 and lib.cairo_status(S.cr) == 0
        return out.flush().copy()
    finally:
        for s in (R, Tc, T, S, G):
            s.close()


def cairo_shadow(words, sh):
    return cairo_inner_shadow(words, sh) if is_inner(sh) else shadow_model.cairo_shadow(words, outer_of(sh))


def cairo_apply(words, filters):
    """R_n of an HxW uint32 image of premultiplied ARGB words, every step by libcairo and pixman"""
    assert 1 <= len(filters) <= MAX_FILTERS
    out = np.ascontiguousarray(words, dtype=np.uint32).copy()
    for entry in filters:
        kind, value = filter_model.kind_of(entry)
        out = cairo_inner_shadow(out, value) if kind == "shadow" and is_inner(value) else filter_model.cairo_apply(out, [entry])
    return out
