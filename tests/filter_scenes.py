"""Filter-list scenes ("Filter lists"), built from the pieces of tests/blur_scenes.py and tests/shadow_scenes.py, and their
reference from libcairo + pixman: ShadowReplay with, around every object that carries "filters" (a list of {"blur": ...} / {"shadow": ...}
entries, tests/filter_model.py),

    cairo_push_group; the object; R_0 = cairo_pop_group; every entry in turn on that surface as the literal call sequence of its rule
    (filter_model.cairo_apply: pixman's convolution for a blur, shadow_model.cairo_shadow for a shadow, each on the result before it);
    cairo_set_source(the last result); cairo_set_operator(the mode of "layer", absent: OVER); cairo_paint

An object that also carries "mask" or "opacity" gets its filters first: those wrappers go around the filtered layer and take the mode.
An empty list is no filter: the object is drawn as if it had no such key.  tools/make_filter_goldens.py writes goldens() to
tests/golden/cairo_filters_*.npz (premultiplied RGBA; key = scene name); the tests rebuild the scenes from here, so a golden file holds
pixels only.  Every scene is at most 96 x 64.
"""
import ctypes

import numpy as np

import blend_model as bm
import blend_scenes as bs
import blur_scenes as bl
import filter_model as fm
import layer_scenes as ls
import mask_scenes as ms
import scenarios
import shadow_scenes as ss
from blend_scenes import _rect, _shape, _with_ground
from blur_scenes import OUTER_KEYS, _blurred, _scene
from layer_scenes import _pair
from shadow_scenes import DROP, GLOW, _shadowed

golden_path = bs.golden_path
W, H = bl.W, bl.H


class FilterReplay(ss.ShadowReplay):
    """ShadowReplay whose objects may carry "filters": see the module's docstring"""

    def _draw(self, obj):
        if obj.get("filters") is None:
            return super()._draw(obj)
        assert obj.get("blur") is None and obj.get("shadow") is None, "the single keys have no place in the list's order"
        if not obj["filters"]:
            return super()._draw({k: v for k, v in obj.items() if k != "filters"})
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
        view[:] = fm.cairo_apply(view.copy(), obj["filters"])        # R_n takes the group surface's place
        lib.cairo_surface_mark_dirty(surf)
        be.save()
        lib.cairo_set_source(cr, group)
        lib.cairo_set_operator(cr, bm.CAIRO_OPERATORS[ls.layer_mode_name(obj.get("layer") or True)])
        lib.cairo_paint(cr)
        be.restore()
        lib.cairo_pattern_destroy(group)


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a filter scene through libcairo and pixman"""
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
        rp = FilterReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in low.extra.items():
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


def map_filters(obj, change):
    """the same tree with every non-empty "filters" list replaced by change(list); where that leaves no entry the object becomes a plain
    layer of the same mode (the outer wrappers of "mask" and "opacity" are layers already)"""
    if isinstance(obj, list):
        return [map_filters(o, change) for o in obj]
    out = dict(obj)
    if obj.get("filters"):
        rest = list(change(list(obj["filters"])))
        if rest:
            out["filters"] = rest
        else:
            del out["filters"]
            if not any(obj.get(k) is not None for k in OUTER_KEYS):
                out["layer"] = obj.get("layer") or True
    if "children" in out:
        out["children"] = map_filters(out["children"], change)
    if out.get("mask") is not None:
        out["mask"] = map_filters(out["mask"], change)
    return out


def without_filters(obj):
    return map_filters(obj, lambda f: [])


def without_last(obj):
    return map_filters(obj, lambda f: f[:-1])


def without_noops(obj):
    """without the entries that are a 1 x 1 blur"""
    return map_filters(obj, lambda f: [e for e in f if not ("blur" in e and fm.blur_of(e["blur"])[0] <= 1 and fm.blur_of(e["blur"])[1] <= 1)])


def as_filter_lists(obj):
    """the same tree with every "blur" and every "shadow" rewritten as a "filters" list of that one entry"""
    if isinstance(obj, list):
        return [as_filter_lists(o) for o in obj]
    out = {k: v for k, v in obj.items() if k not in ("blur", "shadow")}
    for key in ("blur", "shadow"):
        if obj.get(key) is not None:
            assert "filters" not in out
            out["filters"] = [{key: dict(obj[key])}]
    if "children" in out:
        out["children"] = as_filter_lists(out["children"])
    if out.get("mask") is not None:
        out["mask"] = as_filter_lists(out["mask"])
    return out


# ---- pieces.  The six entries the model and the kernels are held to in every ordered pair (tests/test_filters_model.py,
# tests/test_filters_gpu.py): a blur of two box steps and one of three, a glow, a drop shadow, a knockout glow, a hide-object drop shadow
BLUR_EVEN, BLUR_ODD = fm.blur(3, 4, 1), fm.blur(2, 0, 3)
ENTRIES = {"blur_even": BLUR_EVEN, "blur_odd": BLUR_ODD, "glow": fm.shadow(GLOW), "drop": fm.shadow(DROP), "kglow": fm.shadow(GLOW, knockout=True),
           "hdrop": fm.shadow(DROP, hide_object=True)}
E = ENTRIES
NOOP = fm.blur(1, 1, 1)
# a knockout glow, a 2 x 2 blur with two passes, a drop shadow, a 255 x 1 blur
CHAIN_OF_FOUR = [E["kglow"], fm.blur(2, 2, 2), E["drop"], fm.blur(255, 1, 1)]


def _filtered(kids, filters, mode=None, **kw):
    obj = {"type": "container", "children": list(kids), "filters": [dict(e) for e in filters], **kw}
    if mode is not None:
        obj["layer"] = mode
    return obj


OPERATORS = bl.OPERATORS
CHAINS = {"glow_drop": [E["glow"], E["drop"]], "blur_drop": [BLUR_EVEN, E["drop"]]}
# each of `order_a_b` has its twin `order_b_a`
ORDERS = {"glow": E["glow"], "drop": E["drop"], "blur": BLUR_EVEN, "kglow": E["kglow"]}
ORDER_PAIRS = (("glow", "drop"), ("blur", "drop"), ("kglow", "blur"))
# a blur of an odd and of an even number of box steps in first, middle and last place, a later shadow of an odd number, of none, and two
# odd blurs: every branch of the destination plan ("Filter lists")
PLACES = {"odd_first": [BLUR_ODD, E["drop"]], "even_first": [fm.blur(4, 6, 1), E["glow"]],
          "odd_middle": [E["glow"], BLUR_ODD, E["drop"]], "even_middle": [E["glow"], BLUR_EVEN, E["drop"]],
          "odd_last": [E["drop"], BLUR_ODD], "even_last": [E["drop"], BLUR_EVEN],
          "odd_odd": [BLUR_ODD, E["glow"], fm.blur(0, 5, 1)], "odd_then_even_then_odd": [fm.blur(3, 0, 1), BLUR_EVEN, BLUR_ODD, E["kglow"]],
          "later_shadow_odd": [BLUR_EVEN, fm.shadow(DROP, x=7, y=0)], "later_shadow_box_1x1": [BLUR_ODD, fm.shadow(DROP, x=1, y=1)],
          "first_shadow_odd": [fm.shadow(GLOW, x=0, y=5), E["drop"]]}


def operator_scenes():
    """glow then drop, and blur then drop x normal and two operators x {clear, opaque, translucent} ground"""
    out = {}
    for cname, chain in CHAINS.items():
        for mode in OPERATORS:
            for gname, ground in bs._grounds(W, H).items():
                out["%s_%s_%s" % (cname, mode, gname)] = _scene(ground + [_filtered(_pair(), chain, mode)])
    return out


def structure_scenes():
    out = {}
    ground = bs._grounds(W, H)["translucent"]
    for a, b in ORDER_PAIRS:
        out["order_%s_%s" % (a, b)] = _scene(ground + [_filtered(_pair(), [ORDERS[a], ORDERS[b]])])
        out["order_%s_%s" % (b, a)] = _scene(ground + [_filtered(_pair(), [ORDERS[b], ORDERS[a]])])
    out["chain_of_four"] = _scene(ground + [_filtered(_pair(), CHAIN_OF_FOUR)])
    out["hide_then_blur"] = _scene(ground + [_filtered(_pair(), [E["hdrop"], BLUR_EVEN])])
    for name, chain in PLACES.items():
        out["place_" + name] = _scene(ground + [_filtered(_pair(), chain)])
    out["partly_out_then_shadow"] = _scene(ground + [_filtered(_pair(), [fm.shadow(DROP, dx=-30, dy=25), E["glow"]])])
    out["noop_glow_drop"] = _scene(ground + [_filtered(_pair(), [E["glow"], NOOP, E["drop"]])])
    out["noop_blur_drop"] = _scene(ground + [_filtered(_pair(), [BLUR_ODD, fm.blur(1, 1, 2), E["drop"]], "screen")])
    tri = [_shape([(10, 5), (66, 12), (30, 48)], (0, 0, 0, 200))]
    out["filters_and_opacity"] = _scene(ground + [_filtered(_pair(), CHAINS["glow_drop"], "screen", opacity=180)])
    out["filters_and_mask"] = _scene(ground + [_filtered(_pair(), CHAINS["blur_drop"], mask=tri)])
    out["filters_mask_opacity"] = _scene(ground + [_filtered(_pair(), [E["drop"], BLUR_ODD], "multiply", opacity=200, mask=[_rect(12, 8, 60, 40, (0, 0, 0, 230))])])
    out["filters_inside_layer"] = _scene(ground + [ls._layer("screen", [_rect(2, 30, 40, 50, (10, 180, 220, 160)), _filtered(_pair(), CHAINS["glow_drop"], "multiply")])])
    out["layer_inside_filters"] = _scene(ground + [_filtered([ls._layer("multiply", _pair()), _rect(2, 30, 40, 50, (10, 180, 220, 160))], CHAINS["blur_drop"])])
    out["filtered_blurred_shadowed"] = _scene(ground + [_filtered(_pair(-6, -3), [E["kglow"], BLUR_ODD]),
                                                        _blurred([_shape([(20, 4), (50, 9), (36, 30)], (255, 255, 255, 120))], 4, 3),
                                                        _shadowed(_pair(8, 6), DROP, "screen")])
    out["matrix_outside"] = _scene(ground + [_filtered(_pair(), CHAINS["glow_drop"], matrix=scenarios._m(0.8, 0.9, 6, 3))])
    return out


def source_scenes():
    """a bitmap fill (repeating, over a solid) and a radial gradient inside the filtered group: the scenarios of tests/scenarios.py scaled
    into a 96 x 64 frame, over a ground"""
    SC = scenarios.scenarios()
    out = {}
    for name, chain in (("bitmap_repeat_over_solid", [fm.blur(3, 2, 2), fm.shadow(DROP, dx=6, dy=-4)]), ("gradient_radial", [E["glow"], fm.blur(2, 3, 1)])):
        sc = SC[name]
        k = min(96.0 / sc["width"], 64.0 / sc["height"])
        small = dict(sc, width=96, height=64)
        kids = [{"type": "container", "matrix": scenarios._m(k * 0.8, k * 0.8, 8, 6), "children": sc["stage"]["children"]}]
        out[name] = dict(small, exact=True, stage={"children": _with_ground(small) + [_filtered(kids, chain)]})
    return out


def files():
    """golden file name -> (scenes, aliased)"""
    out = {}
    for aliased in (False, True):
        tag = "aliased_" if aliased else ""
        out["cairo_filters_%soperators" % tag] = (operator_scenes, aliased)
        out["cairo_filters_%sstructure" % tag] = (structure_scenes, aliased)
        out["cairo_filters_%ssources" % tag] = (source_scenes, aliased)
    return out


def goldens():
    return {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())} for fname, (make, aliased) in files().items()}
