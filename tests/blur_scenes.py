"""Blurred-layer scenes ("Blurred layers"), built from tests/scenarios.py, tests/blend_scenes.py, tests/layer_scenes.py and
tests/mask_scenes.py pieces, and their reference from libcairo + pixman: FadeReplay with, around every object that carries "blur",

    cairo_push_group; the object; group = cairo_pop_group; the box blur on the group's surface -- one pixman_image_composite32(SRC) from an
    image carrying PIXMAN_FILTER_CONVOLUTION per axis and pass (tests/blur_model.py, pixman_blur); cairo_set_source(group);
    cairo_set_operator(the mode of "layer", absent: OVER); cairo_paint

An object that also carries "mask" or "opacity" is blurred first: those wrappers go around the blurred layer and take the mode.
tools/make_blur_goldens.py writes goldens() to tests/golden/cairo_blur_*.npz (premultiplied RGBA; key = scene name); the tests rebuild the
scenes from here, so a golden file holds pixels only.  Every scene is at most 96 x 64.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import blend_model as bm  # noqa: E402
import blend_scenes as bs  # noqa: E402
import blur_model  # noqa: E402
import fade_scenes as fs  # noqa: E402
import layer_scenes as ls  # noqa: E402
import mask_scenes as ms  # noqa: E402
import scenarios  # noqa: E402
from blend_scenes import _rect, _shape, _with_ground  # noqa: E402
from layer_scenes import _pair  # noqa: E402

golden_path = bs.golden_path
W, H = 72, 52
OUTER_KEYS = ("mask", "opacity")


def blur_of(obj):
    b = obj["blur"]
    return int(b.get("x", 0)), int(b.get("y", 0)), int(b.get("passes", 1))


class BlurReplay(fs.FadeReplay):
    """FadeReplay whose objects may carry "blur" ({"x", "y", "passes"}): see the module's docstring.  The operator in force around the
    object stays in force inside the group and is restored behind the paint."""

    def _draw(self, obj):
        if obj.get("blur") is None:
            return super()._draw(obj)
        if any(obj.get(k) is not None for k in OUTER_KEYS):
            # mask and fade apply to the blurred image: a plain container carries them (and the mode) around the blurred object
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
            super()._draw({k: v for k, v in obj.items() if k not in ("blur", "layer")})
        finally:
            group = lib.cairo_pop_group(cr)
        surf = P()
        assert lib.cairo_pattern_get_surface(group, ctypes.byref(surf)) == 0
        lib.cairo_surface_flush(surf)
        w, h, stride = lib.cairo_image_surface_get_width(surf), lib.cairo_image_surface_get_height(surf), lib.cairo_image_surface_get_stride(surf)
        assert (w, h) == (be.w, be.h) and stride == w * 4, "the group's surface is the frame's size"
        data = lib.cairo_image_surface_get_data(surf)
        view = np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_uint32)), shape=(h, w))
        view[:] = blur_model.pixman_blur(view.copy(), *blur_of(obj))
        lib.cairo_surface_mark_dirty(surf)
        be.save()
        lib.cairo_set_source(cr, group)
        lib.cairo_set_operator(cr, bm.CAIRO_OPERATORS[ls.layer_mode_name(obj.get("layer") or True)])
        lib.cairo_paint(cr)
        be.restore()
        lib.cairo_pattern_destroy(group)


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a blur scene through libcairo and pixman"""
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
        rp = BlurReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in low.extra.items():
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


def without_blur(obj):
    """the same tree with every "blur" replaced by a plain layer of the same mode"""
    if isinstance(obj, list):
        return [without_blur(o) for o in obj]
    out = {k: v for k, v in obj.items() if k != "blur"}
    if "blur" in obj and not any(obj.get(k) is not None for k in OUTER_KEYS):
        out["layer"] = obj.get("layer") or True
    if "children" in out:
        out["children"] = without_blur(out["children"])
    if out.get("mask") is not None:
        out["mask"] = without_blur(out["mask"])
    return out


# ---- pieces
def _blurred(kids, x, y, passes=1, mode=None, **kw):
    obj = {"type": "container", "children": list(kids), "blur": {"x": x, "y": y, "passes": passes}, **kw}
    if mode is not None:
        obj["layer"] = mode
    return obj


def _scene(kids, w=W, h=H, **kw):
    return dict(width=w, height=h, exact=True, stage={"children": list(kids)}, **kw)


OPERATORS = ("normal", "multiply", "screen")
BOXES = {"odd_3": (3, 3, 1), "even_2": (2, 2, 1), "even_4": (4, 4, 1), "odd_5": (5, 5, 1), "wide_8x3": (8, 3, 1), "tall_3x16": (3, 16, 1), "x_only_7": (7, 0, 1),
         "y_only_6": (0, 6, 1), "passes3_3x2": (3, 2, 3), "passes3_even_4": (4, 4, 3), "wider_than_frame": (255, 255, 1), "wider_x_100": (100, 1, 2)}


def operator_scenes():
    """normal and two operators x {clear, opaque, translucent} ground: a blurred group of overlapping translucent children"""
    out = {}
    for mode in OPERATORS:
        for gname, ground in bs._grounds(W, H).items():
            out["%s_%s" % (mode, gname)] = _scene(ground + [_blurred(_pair(), 3, 3, 1, mode)])
    return out


def box_scenes():
    """odd and even boxes, bx != by, one axis at 0, three passes, boxes wider than the frame; content that touches all four frame
    edges; a blurred layer inside a faded layer, inside a mask, and carrying both itself; two blurred layers in one frame"""
    out = {}
    ground = bs._grounds(W, H)["translucent"]
    for name, (x, y, passes) in BOXES.items():
        out["box_" + name] = _scene(ground + [_blurred(_pair(), x, y, passes)])
    edges = [_rect(-6, -6, W + 6, H + 6, (40, 90, 200, 140)), _shape([(-4.5, 10.2), (W + 3.3, -2.1), (W * 0.6, H + 5.5)], (230, 40, 90, 200))]
    out["frame_edges"] = _scene([_blurred(edges, 6, 6, 1)])
    out["frame_edges_over_ground"] = _scene(bs._grounds(W, H)["opaque"] + [_blurred(edges, 9, 4, 2, "multiply")])
    out["inside_faded"] = _scene(ground + [{"type": "container", "opacity": 140, "children": [_rect(4, 4, 30, 20, (250, 240, 30, 255)), _blurred(_pair(), 5, 5, 1)]}])
    out["inside_mask"] = _scene(ground + [{"type": "container", "mask": [_shape([(10, 5), (66, 12), (30, 48)], (0, 0, 0, 200))],
                                           "children": [_blurred(_pair(), 4, 7, 1), _rect(40, 30, 70, 50, (20, 200, 60, 180))]}])
    out["blur_and_opacity"] = _scene(ground + [_blurred(_pair(), 5, 3, 1, "screen", opacity=180)])
    out["blur_and_mask"] = _scene(ground + [_blurred(_pair(), 6, 6, 1, mask=[_shape([(10, 5), (66, 12), (30, 48)], (0, 0, 0, 255))])])
    out["blur_mask_opacity"] = _scene(ground + [_blurred(_pair(), 3, 8, 2, "multiply", opacity=200, mask=[_rect(12, 8, 60, 40, (0, 0, 0, 230))])])
    out["two_layers"] = _scene(ground + [_blurred(_pair(-6, -3), 5, 5, 1), _shape([(20, 4), (50, 9), (36, 30)], (255, 255, 255, 120)),
                                         _blurred(_pair(8, 6), 2, 9, 1, "screen")])
    out["layer_inside_blur"] = _scene(ground + [_blurred([ls._layer("multiply", _pair()), _rect(2, 30, 40, 50, (10, 180, 220, 160))], 4, 4, 1)])
    out["blur_inside_layer"] = _scene(ground + [ls._layer("screen", [_rect(2, 30, 40, 50, (10, 180, 220, 160)), _blurred(_pair(), 4, 4, 1, "multiply")])])
    out["matrix_outside"] = _scene(ground + [_blurred(_pair(), 6, 2, 1, matrix=scenarios._m(0.8, 0.9, 6, 3))])
    return out


def source_scenes():
    """a bitmap fill (repeating, over a solid) and a radial gradient inside the blurred group: the scenarios of tests/scenarios.py
    scaled into a 96 x 64 frame, over a ground"""
    SC = scenarios.scenarios()
    out = {}
    for name, blur in (("bitmap_repeat_over_solid", (5, 4, 2)), ("gradient_radial", (4, 6, 1))):
        sc = SC[name]
        k = min(96.0 / sc["width"], 64.0 / sc["height"])
        small = dict(sc, width=96, height=64)
        kids = [{"type": "container", "matrix": scenarios._m(k, k, 0, 0), "children": sc["stage"]["children"]}]
        out[name] = dict(small, exact=True, stage={"children": _with_ground(small) + [_blurred(kids, *blur)]})
    return out


def files():
    """golden file name -> (scenes, aliased)"""
    out = {}
    for aliased in (False, True):
        tag = "aliased_" if aliased else ""
        out["cairo_blur_%soperators" % tag] = (operator_scenes, aliased)
        out["cairo_blur_%sboxes" % tag] = (box_scenes, aliased)
        out["cairo_blur_%ssources" % tag] = (source_scenes, aliased)
    return out


def goldens():
    return {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())} for fname, (make, aliased) in files().items()}
