"""Convolution-filter scenes ("Convolution filters"), built from the pieces of tests/filter_scenes.py and tests/inner_scenes.py,
and their reference from libcairo + pixman: InnerReplay with, around every object whose "filters" holds a {"convolution": ...} entry,

    cairo_push_group; the object; R_0 = cairo_pop_group; every entry in turn on that surface as the literal call sequence of its rule
    (convolution_model.cairo_apply: one pixman_image_composite32(SRC) from an image carrying the convolution filter for such an entry,
    the other kinds as before); cairo_set_source(the last result); cairo_set_operator(the mode of "layer", absent: OVER); cairo_paint

Every other object is InnerReplay's.  An object that also carries "mask" or "opacity" gets its filters first: those wrappers go around
the filtered layer and take the mode.  tools/make_convolution_goldens.py writes goldens() to tests/golden/cairo_convolution_*.npz
(premultiplied RGBA; key = scene name); the tests rebuild the scenes from here, so a golden file holds pixels only.  Every scene is at
most 96 x 64.  A scene's "group" is the filtered object without its filters, alone on a clear frame: the golden tool makes the filtered
surface of it, to see that the sharpen, emboss and edge scenes do hold pixels whose colour exceeds their alpha.
"""
import ctypes

import numpy as np

import blend_model as bm
import blend_scenes as bs
import blur_scenes as bl
import convolution_model as cm
import filter_model as fm
import filter_scenes as fsc
import inner_scenes as isc
import layer_scenes as ls
import mask_scenes as ms
from blend_scenes import _rect, _shape
from blur_scenes import OUTER_KEYS, _scene
from filter_scenes import _filtered
from layer_scenes import _pair
from shadow_scenes import DROP, GLOW

golden_path = bs.golden_path
W, H = bl.W, bl.H
Cv = cm.convolution


def _has_convolution(obj):
    return bool(obj.get("filters")) and any("convolution" in e for e in obj["filters"])


class ConvolutionReplay(isc.InnerReplay):
    """InnerReplay whose filter lists may hold convolutions: see the module's docstring"""

    def _draw(self, obj):
        if not _has_convolution(obj):
            return super()._draw(obj)
        assert obj.get("blur") is None and obj.get("shadow") is None
        if any(obj.get(k) is not None for k in OUTER_KEYS):
            outer = {"type": "container", "children": [{k: v for k, v in obj.items() if k not in OUTER_KEYS + ("layer",)}]}
            outer.update({k: obj[k] for k in OUTER_KEYS + ("layer",) if obj.get(k) is not None})
            return super()._draw(outer)
        be = self.be
        lib, cr = be.lib, be.cr
        P, I = ctypes.c_void_p, ctypes.c_int
        for fn, res, args in (("cairo_push_group", None, [P]), ("cairo_pop_group", P, [P]), ("cairo_set_source", None, [P, P]), ("cairo_paint", None, [P]),
                              ("cairo_pattern_destroy", None, [P]), ("cairo_pattern_get_surface", I, [P, ctypes.POINTER(P)]),
                              ("cairo_image_surface_get_width", I, [P]), ("cairo_image_surface_get_height", I, [P])):
            f = getattr(lib, fn)
            f.restype, f.argtypes = res, args
        lib.cairo_push_group(cr)
        try:
            super()._draw({k: v for k, v in obj.items() if k not in ("filters", "layer")})
        finally:
            group = lib.cairo_pop_group(cr)
        surf = P()
        assert lib.cairo_pattern_get_surface(group, ctypes.byref(surf)) == 0
        lib.cairo_surface_flush(surf)
        w, h, stride = lib.cairo_image_surface_get_width(surf), lib.cairo_image_surface_get_height(surf), lib.cairo_image_surface_get_stride(surf)
        assert (w, h) == (be.w, be.h) and stride == w * 4, "the group's surface is the frame's size"
        data = lib.cairo_image_surface_get_data(surf)
        view = np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_uint32)), shape=(h, w))
        view[:] = cm.cairo_apply(view.copy(), obj["filters"])        # R_n takes the group surface's place
        lib.cairo_surface_mark_dirty(surf)
        be.save()
        lib.cairo_set_source(cr, group)
        lib.cairo_set_operator(cr, bm.CAIRO_OPERATORS[ls.layer_mode_name(obj.get("layer") or True)])
        lib.cairo_paint(cr)
        be.restore()
        lib.cairo_pattern_destroy(group)


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a convolution scene through libcairo and pixman"""
    from oracle import cairo_backend as cb
    be = cb.CairoBackend(sc["width"], sc["height"])
    try:
        if aliased:
            f = be.lib.cairo_set_antialias
            f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int]
            f(be.cr, bs.CAIRO_ANTIALIAS_NONE)
        if sc.get("even_odd"):
            be.set_fill_rule(True)
        low = ms._lowering(sc.get("bitmaps", []))
        stage = low.lower(sc["stage"])
        rp = ConvolutionReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in low.extra.items():
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


without_filters = fsc.without_filters
without_last = fsc.without_last


# ---- pieces
def _opaque_pair():
    """_pair's shapes, opaque, and a translucent bar across them"""
    return [_shape([(8.3, 4.2), (58.6, 12.7), (20.2, 40.4)], (230, 40, 90, 255)), _shape([(30.1, 3.4), (61.2, 30.9), (12.5, 36.3)], (40, 200, 120, 255)),
            _rect(22, 18, 50.5, 44.25, (20, 60, 240, 120))]


def _off_frame():
    """an object running off the left and the bottom of the frame"""
    return [_shape([(-20.5, 10.2), (40.6, 20.7), (30.2, H + 15.4), (-10.1, H + 4.0)], (240, 160, 30, 210)), _rect(-5, 30, 25.5, H + 9, (30, 90, 200, 255))]


def _scene_of(ground, kids, filters, mode=None, **kw):
    sc = _scene(ground + [_filtered(kids, filters, mode, **kw)])
    sc["group"] = (list(kids), [dict(e) for e in filters])
    return sc


def kernel_scenes():
    """every named kernel alone over a translucent ground: the framebuffer instance"""
    ground = bs._grounds(W, H)["translucent"]
    return {name: _scene_of(ground, _pair(), [Cv(value)]) for name, value in sorted(cm.NAMED.items())}


def structure_scenes():
    g = bs._grounds(W, H)
    tr, op = g["translucent"], g["opaque"]
    out = {}
    out["sharpen_opaque_content"] = _scene_of(tr, _opaque_pair(), [Cv(cm.SHARPEN)])
    out["emboss_off_two_sides"] = _scene_of(tr, _off_frame(), [Cv(cm.EMBOSS)])
    out["edge_over_clear"] = _scene_of(g["clear"], _pair(), [Cv(cm.EDGE)])
    for mode, value in (("multiply", cm.SHARPEN), ("difference", cm.EMBOSS), ("add", cm.EDGE), ("overlay", cm.GAUSS5)):
        out["%s_opaque_ground" % mode] = _scene_of(op, _pair(), [Cv(value)], mode)
    out["sharpen_under_mask"] = _scene_of(tr, _pair(), [Cv(cm.SHARPEN)], mask=[_shape([(10, 5), (66, 12), (30, 48)], (0, 0, 0, 200))])
    out["emboss_under_opacity"] = _scene_of(tr, _pair(), [Cv(cm.EMBOSS)], "screen", opacity=170)
    out["blur_then_sharpen"] = _scene_of(tr, _pair(), [fsc.BLUR_ODD, Cv(cm.SHARPEN)])
    out["sharpen_then_blur"] = _scene_of(tr, _pair(), [Cv(cm.SHARPEN), fsc.BLUR_EVEN])
    out["drop_then_edge"] = _scene_of(tr, _pair(), [fm.shadow(DROP), Cv(cm.EDGE)])
    out["edge_then_drop"] = _scene_of(tr, _pair(), [Cv(cm.EDGE), fm.shadow(DROP)])
    out["sharpen_then_inner_glow"] = _scene_of(tr, _pair(), [Cv(cm.SHARPEN), {"shadow": dict(GLOW, inner=True)}])
    out["two_in_a_row_and_a_knockout_glow"] = _scene_of(tr, _pair(), [Cv(cm.EVEN_2X2), Cv(cm.MOTION_1X7), fm.shadow(GLOW, knockout=True), Cv(cm.BOX3)])
    return out


def aliased_scenes():
    g = bs._grounds(W, H)
    return {"sharpen": _scene_of(g["translucent"], _pair(), [Cv(cm.SHARPEN)]),
            "even_4x6_multiply": _scene_of(g["opaque"], _pair(), [Cv(cm.EVEN_4X6)], "multiply"),
            "blur_then_emboss": _scene_of(g["translucent"], _pair(), [fsc.BLUR_EVEN, Cv(cm.EMBOSS)])}


# the scenes whose filtered surface must hold pixels whose colour exceeds their alpha
ABOVE_ALPHA = ("sharpen", "emboss", "edge")


def files():
    """golden file name -> (scenes, aliased)"""
    return {"cairo_convolution_kernels": (kernel_scenes, False), "cairo_convolution_structure": (structure_scenes, False),
            "cairo_convolution_aliased": (aliased_scenes, True)}


def goldens():
    return {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())} for fname, (make, aliased) in files().items()}
