"""Shadowed-layer scenes ("Shadowed layers"), built from the pieces of tests/blur_scenes.py, and their reference from libcairo +
pixman: BlurReplay with, around every object that carries "shadow",

    cairo_push_group; the object; G = cairo_pop_group; steps 2 to 6 of the rule on G's surface as the literal call sequence
    (tests/shadow_model.py, cairo_shadow: cairo_mask_surface, pixman's convolution, ADD paints, cairo_mask_surface, an OVER or DEST_OUT
    paint of G); cairo_set_source(the final surface); cairo_set_operator(the mode of "layer", absent: OVER); cairo_paint

An object that also carries "mask" or "opacity" gets its shadow first: those wrappers go around the shadowed layer and take the mode.
tools/make_shadow_goldens.py writes goldens() to tests/golden/cairo_shadow_*.npz (premultiplied RGBA; key = scene name); the tests rebuild
the scenes from here, so a golden file holds pixels only.  Every scene is at most 96 x 64.
"""
import ctypes

import numpy as np

import blend_model as bm
import blend_scenes as bs
import blur_scenes as bl
import layer_scenes as ls
import mask_scenes as ms
import scenarios
import shadow_model as sm
from blend_scenes import _rect, _shape, _with_ground
from blur_scenes import OUTER_KEYS, _blurred, _scene
from layer_scenes import _pair

golden_path = bs.golden_path
W, H = bl.W, bl.H


class ShadowReplay(bl.BlurReplay):
    """BlurReplay whose objects may carry "shadow" (a dict as tests/shadow_model.py takes it): see the module's docstring"""

    def _draw(self, obj):
        if obj.get("shadow") is None:
            return super()._draw(obj)
        assert obj.get("blur") is None, "a filter list is ordered; this pair of keys is not"
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
            super()._draw({k: v for k, v in obj.items() if k not in ("shadow", "layer")})
        finally:
            group = lib.cairo_pop_group(cr)
        surf = P()
        assert lib.cairo_pattern_get_surface(group, ctypes.byref(surf)) == 0
        lib.cairo_surface_flush(surf)
        w, h, stride = lib.cairo_image_surface_get_width(surf), lib.cairo_image_surface_get_height(surf), lib.cairo_image_surface_get_stride(surf)
        assert (w, h) == (be.w, be.h) and stride == w * 4, "the group's surface is the frame's size"
        data = lib.cairo_image_surface_get_data(surf)
        view = np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_uint32)), shape=(h, w))
        view[:] = sm.cairo_shadow(view.copy(), obj["shadow"])       # the final surface R takes the group surface's place
        lib.cairo_surface_mark_dirty(surf)
        be.save()
        lib.cairo_set_source(cr, group)
        lib.cairo_set_operator(cr, bm.CAIRO_OPERATORS[ls.layer_mode_name(obj.get("layer") or True)])
        lib.cairo_paint(cr)
        be.restore()
        lib.cairo_pattern_destroy(group)


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a shadow scene through libcairo and pixman"""
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
        rp = ShadowReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in low.extra.items():
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


def without_shadow(obj):
    """the same tree with every "shadow" replaced by a plain layer of the same mode"""
    if isinstance(obj, list):
        return [without_shadow(o) for o in obj]
    out = {k: v for k, v in obj.items() if k != "shadow"}
    if "shadow" in obj and not any(obj.get(k) is not None for k in OUTER_KEYS):
        out["layer"] = obj.get("layer") or True
    if "children" in out:
        out["children"] = without_shadow(out["children"])
    if out.get("mask") is not None:
        out["mask"] = without_shadow(out["mask"])
    return out


# ---- pieces
DROP = {"color": (10, 20, 60, 200), "dx": 4, "dy": 3, "x": 5, "y": 5}
GLOW = {"color": (255, 220, 40, 255), "x": 6, "y": 6, "strength": 2}


def _shadowed(kids, shadow, mode=None, **kw):
    obj = {"type": "container", "children": list(kids), "shadow": dict(shadow), **kw}
    if mode is not None:
        obj["layer"] = mode
    return obj


OPERATORS = bl.OPERATORS
VARIANTS = {"odd_3": dict(DROP, x=3, y=3), "even_2": dict(DROP, x=2, y=2), "even_4x6": dict(DROP, x=4, y=6), "passes3": dict(DROP, x=3, y=2, passes=3),
            "x_only": dict(DROP, x=7, y=0), "box_1x1": dict(DROP, x=1, y=1), "partly_out": dict(DROP, dx=-30, dy=25),
            "strength_1": dict(GLOW, strength=1), "strength_3": dict(GLOW, strength=3), "strength_255": dict(GLOW, strength=255, color=(0, 200, 90, 90)),
            "wider_than_frame": dict(GLOW, x=255, y=255, strength=40)}


def operator_scenes():
    """a drop shadow and a glow x normal and two operators x {clear, opaque, translucent} ground, around overlapping translucent children"""
    out = {}
    for kind, sh in (("drop", DROP), ("glow", GLOW)):
        for mode in OPERATORS:
            for gname, ground in bs._grounds(W, H).items():
                out["%s_%s_%s" % (kind, mode, gname)] = _scene(ground + [_shadowed(_pair(), sh, mode)])
    return out


def structure_scenes():
    """odd and even boxes, an offset that pushes the shadow partly and wholly out of the frame, strengths, content that touches all four
    frame edges; hide and knockout twins; with "mask", "opacity" and both; inside a layer, a layer inside; two shadowed layers and a
    blurred one in one frame"""
    out = {}
    ground = bs._grounds(W, H)["translucent"]
    for name, sh in VARIANTS.items():
        out["shadow_" + name] = _scene(ground + [_shadowed(_pair(), sh)])
    edges = [_rect(-6, -6, W + 6, 9, (40, 90, 200, 140)), _rect(-6, H - 7, W + 6, H + 6, (200, 90, 40, 255)),
             _shape([(-4.5, 10.2), (W + 3.3, -2.1), (W * 0.6, H + 5.5)], (230, 40, 90, 200))]
    out["frame_edges"] = _scene([_shadowed(edges, dict(DROP, dx=-5, dy=6, x=6, y=4))])
    out["frame_edges_over_ground"] = _scene(bs._grounds(W, H)["opaque"] + [_shadowed(edges, dict(GLOW, x=9, y=4, passes=2), "multiply")])
    for kind, sh in (("drop", DROP), ("glow", dict(GLOW, strength=3))):
        for gname in ("clear", "translucent"):
            g = bs._grounds(W, H)[gname]
            out["hide_%s_%s" % (kind, gname)] = _scene(g + [_shadowed(_pair(), dict(sh, hide_object=True))])
            out["knockout_%s_%s" % (kind, gname)] = _scene(g + [_shadowed(_pair(), dict(sh, knockout=True))])
    out["knockout_screen_opaque"] = _scene(bs._grounds(W, H)["opaque"] + [_shadowed(_pair(), dict(GLOW, knockout=True), "screen")])
    out["hide_screen_opaque"] = _scene(bs._grounds(W, H)["opaque"] + [_shadowed(_pair(), dict(GLOW, hide_object=True), "screen")])
    tri = [_shape([(10, 5), (66, 12), (30, 48)], (0, 0, 0, 200))]
    out["shadow_and_opacity"] = _scene(ground + [_shadowed(_pair(), DROP, "screen", opacity=180)])
    out["shadow_and_mask"] = _scene(ground + [_shadowed(_pair(), GLOW, mask=tri)])
    out["shadow_mask_opacity"] = _scene(ground + [_shadowed(_pair(), dict(DROP, passes=2), "multiply", opacity=200, mask=[_rect(12, 8, 60, 40, (0, 0, 0, 230))])])
    out["inside_faded"] = _scene(ground + [{"type": "container", "opacity": 140, "children": [_rect(4, 4, 30, 20, (250, 240, 30, 255)), _shadowed(_pair(), DROP)]}])
    out["inside_mask"] = _scene(ground + [{"type": "container", "mask": tri, "children": [_shadowed(_pair(), GLOW), _rect(40, 30, 70, 50, (20, 200, 60, 180))]}])
    out["shadow_inside_layer"] = _scene(ground + [ls._layer("screen", [_rect(2, 30, 40, 50, (10, 180, 220, 160)), _shadowed(_pair(), DROP, "multiply")])])
    out["layer_inside_shadow"] = _scene(ground + [_shadowed([ls._layer("multiply", _pair()), _rect(2, 30, 40, 50, (10, 180, 220, 160))], DROP)])
    out["two_shadows_and_a_blur"] = _scene(ground + [_shadowed(_pair(-6, -3), DROP), _blurred([_shape([(20, 4), (50, 9), (36, 30)], (255, 255, 255, 120))], 4, 3),
                                                     _shadowed(_pair(8, 6), dict(GLOW, knockout=True), "screen")])
    out["matrix_outside"] = _scene(ground + [_shadowed(_pair(), DROP, matrix=scenarios._m(0.8, 0.9, 6, 3))])
    return out


def source_scenes():
    """a bitmap fill (repeating, over a solid) and a radial gradient inside the shadowed group: the scenarios of tests/scenarios.py scaled
    into a 96 x 64 frame, over a ground"""
    SC = scenarios.scenarios()
    out = {}
    for name, sh in (("bitmap_repeat_over_solid", dict(DROP, dx=6, dy=-4, x=5, y=4, passes=2)), ("gradient_radial", dict(GLOW, x=4, y=6))):
        sc = SC[name]
        k = min(96.0 / sc["width"], 64.0 / sc["height"])
        small = dict(sc, width=96, height=64)
        kids = [{"type": "container", "matrix": scenarios._m(k * 0.8, k * 0.8, 8, 6), "children": sc["stage"]["children"]}]
        out[name] = dict(small, exact=True, stage={"children": _with_ground(small) + [_shadowed(kids, sh)]})
    return out


def files():
    """golden file name -> (scenes, aliased)"""
    out = {}
    for aliased in (False, True):
        tag = "aliased_" if aliased else ""
        out["cairo_shadow_%soperators" % tag] = (operator_scenes, aliased)
        out["cairo_shadow_%sstructure" % tag] = (structure_scenes, aliased)
        out["cairo_shadow_%ssources" % tag] = (source_scenes, aliased)
    return out


def goldens():
    return {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())} for fname, (make, aliased) in files().items()}
