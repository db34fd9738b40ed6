"""Inner-shadow scenes ("Inner shadows"), built from the pieces of tests/shadow_scenes.py and tests/filter_scenes.py, and their
reference from libcairo + pixman: FilterReplay with, around every object whose "shadow" or whose "filters" carries "inner": True,

    cairo_push_group; the object; G = cairo_pop_group; the shadow's steps 2' to 6' (inner_model.cairo_inner_shadow) or every entry of the
    list in turn (inner_model.cairo_apply) on that surface as the literal call sequences; cairo_set_source(the last result);
    cairo_set_operator(the mode of "layer", absent: OVER); cairo_paint

Every other object is FilterReplay's.  An object that also carries "mask" or "opacity" gets its shadow first: those wrappers go around
the layer and take the mode.  tools/make_inner_goldens.py writes goldens() to tests/golden/cairo_inner_*.npz (premultiplied RGBA; key =
scene name); the tests rebuild the scenes from here, so a golden file holds pixels only.  Every scene is at most 96 x 64.
"""
import ctypes

import numpy as np

import blend_model as bm
import blend_scenes as bs
import blur_scenes as bl
import filter_model as fm
import filter_scenes as fsc
import inner_model as im
import layer_scenes as ls
import mask_scenes as ms
import scenarios
from blend_scenes import _rect, _shape, _with_ground
from blur_scenes import OUTER_KEYS, _scene
from filter_scenes import _filtered
from layer_scenes import _pair
from shadow_scenes import DROP, GLOW, _shadowed

golden_path = bs.golden_path
W, H = bl.W, bl.H


def _inner_list(obj):
    """the object's filters as a list when one of them is an inner shadow (a lone "shadow" is a list of one entry), else None"""
    if obj.get("shadow") is not None and im.is_inner(obj["shadow"]):
        return [{"shadow": obj["shadow"]}]
    if obj.get("filters") and any("shadow" in e and im.is_inner(e["shadow"]) for e in obj["filters"]):
        return list(obj["filters"])
    return None


class InnerReplay(fsc.FilterReplay):
    """FilterReplay whose shadows, alone or in a list, may carry "inner": see the module's docstring"""

    def _draw(self, obj):
        chain = _inner_list(obj)
        if chain is None:
            return super()._draw(obj)
        assert obj.get("blur") is None and (obj.get("shadow") is None or obj.get("filters") is None)
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
            super()._draw({k: v for k, v in obj.items() if k not in ("shadow", "filters", "layer")})
        finally:
            group = lib.cairo_pop_group(cr)
        surf = P()
        assert lib.cairo_pattern_get_surface(group, ctypes.byref(surf)) == 0
        lib.cairo_surface_flush(surf)
        w, h, stride = lib.cairo_image_surface_get_width(surf), lib.cairo_image_surface_get_height(surf), lib.cairo_image_surface_get_stride(surf)
        assert (w, h) == (be.w, be.h) and stride == w * 4, "the group's surface is the frame's size"
        data = lib.cairo_image_surface_get_data(surf)
        view = np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_uint32)), shape=(h, w))
        if obj.get("shadow") is not None:
            view[:] = im.cairo_inner_shadow(view.copy(), obj["shadow"])       # the final surface R takes the group surface's place
        else:
            view[:] = im.cairo_apply(view.copy(), chain)                      # ... or R_n
        lib.cairo_surface_mark_dirty(surf)
        be.save()
        lib.cairo_set_source(cr, group)
        lib.cairo_set_operator(cr, bm.CAIRO_OPERATORS[ls.layer_mode_name(obj.get("layer") or True)])
        lib.cairo_paint(cr)
        be.restore()
        lib.cairo_pattern_destroy(group)


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of an inner-shadow scene through libcairo and pixman"""
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
        rp = InnerReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in low.extra.items():
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


def map_shadows(obj, change):
    """the same tree with every shadow value, alone or in a list, replaced by change(value); change() returning None takes a lone shadow
    or the whole list away and leaves a plain layer of the same mode (the outer wrappers of "mask" and "opacity" are layers already)"""
    if isinstance(obj, list):
        return [map_shadows(o, change) for o in obj]
    out = dict(obj)
    gone = False
    if obj.get("shadow") is not None:
        new = change(dict(obj["shadow"]))
        if new is None:
            del out["shadow"]
            gone = True
        else:
            out["shadow"] = new
    if obj.get("filters"):
        new = [{"shadow": change(dict(e["shadow"]))} if "shadow" in e else e for e in obj["filters"]]
        if any("shadow" in e and e["shadow"] is None for e in new):
            del out["filters"]
            gone = True
        else:
            out["filters"] = new
    if gone and not any(obj.get(k) is not None for k in OUTER_KEYS):
        out["layer"] = obj.get("layer") or True
    if "children" in out:
        out["children"] = map_shadows(out["children"], change)
    if out.get("mask") is not None:
        out["mask"] = map_shadows(out["mask"], change)
    return out


def without_filters(obj):
    """every shadowed or filtered object that holds an inner shadow as a plain layer"""
    def plain(o):
        if isinstance(o, list):
            return [plain(x) for x in o]
        out = dict(o)
        if _inner_list(o) is not None:
            out.pop("shadow", None), out.pop("filters", None)
            if not any(o.get(k) is not None for k in OUTER_KEYS):
                out["layer"] = o.get("layer") or True
        if "children" in out:
            out["children"] = plain(out["children"])
        if out.get("mask") is not None:
            out["mask"] = plain(out["mask"])
        return out
    return plain(obj)


def flag_cleared(obj):
    """every inner shadow as the outer shadow of the same values"""
    return map_shadows(obj, im.outer_of)


# ---- pieces
INNER = dict(DROP, inner=True)                                   # an inner shadow: offset (4, 3), a 5 x 5 box
INNER_GLOW = dict(GLOW, inner=True)                              # an inner glow: no offset, a 6 x 6 box, strength 2
OPERATORS = ("normal", "multiply", "add")
KINDS = {"shadow": INNER, "glow": INNER_GLOW}
E = {"inner": fm.shadow(INNER), "iglow": fm.shadow(INNER_GLOW), "ikglow": fm.shadow(INNER_GLOW, knockout=True), "drop": fsc.ENTRIES["drop"],
     "blur": fsc.BLUR_EVEN, "blur_odd": fsc.BLUR_ODD}
# the inner entry before and after an outer drop shadow and after a blur (of an even and of an odd number of box steps: both buffers)
LISTS = {"inner_drop": [E["inner"], E["drop"]], "drop_inner": [E["drop"], E["inner"]], "blur_inner": [E["blur"], E["inner"]],
         "blur_odd_iglow": [E["blur_odd"], E["iglow"]], "drop_ikglow_blur": [E["drop"], E["ikglow"], E["blur"]],
         "chain_of_four": [E["inner"], fm.blur(2, 2, 2), E["drop"], E["ikglow"]]}


def operator_scenes():
    """an inner shadow and an inner glow x OVER, multiply and add x {clear, opaque, translucent} ground, around overlapping translucent
    children"""
    out = {}
    for kind, sh in KINDS.items():
        for mode in OPERATORS:
            for gname, ground in bs._grounds(W, H).items():
                out["%s_%s_%s" % (kind, mode, gname)] = _scene(ground + [_shadowed(_pair(), sh, mode)])
    return out


def structure_scenes():
    """knockout twins (knockout_X beside plain_X); an object that runs off the frame on two sides; an offset larger than the object, and
    one that shifts everything out; an opaque object; inside "mask" and inside "opacity", and carrying them; in lists"""
    out = {}
    ground = bs._grounds(W, H)["translucent"]
    for kind, sh in (("shadow", INNER), ("glow", dict(INNER_GLOW, strength=3))):
        for gname in ("clear", "translucent"):
            g = bs._grounds(W, H)[gname]
            out["plain_%s_%s" % (kind, gname)] = _scene(g + [_shadowed(_pair(), sh)])
            out["knockout_%s_%s" % (kind, gname)] = _scene(g + [_shadowed(_pair(), dict(sh, knockout=True))])
    out["plain_screen_opaque"] = _scene(bs._grounds(W, H)["opaque"] + [_shadowed(_pair(), INNER_GLOW, "screen")])
    out["knockout_screen_opaque"] = _scene(bs._grounds(W, H)["opaque"] + [_shadowed(_pair(), dict(INNER_GLOW, knockout=True), "screen")])
    # off the frame to the left and at the top: no inner shadow along those two frame edges
    corner = [_rect(-20, -14, 44.5, 30.25, (230, 200, 60, 255)), _shape([(-8, 20), (30, -6), (52, 41)], (40, 90, 200, 170))]
    out["off_frame_two_sides"] = _scene(ground + [_shadowed(corner, dict(INNER, dx=3, dy=3, x=7, y=7))])
    out["off_frame_two_sides_glow"] = _scene(ground + [_shadowed(corner, dict(INNER_GLOW, x=9, y=5, passes=2), "multiply")])
    small = [_rect(20, 14, 38, 30, (240, 240, 240, 255))]
    out["offset_larger_than_object"] = _scene(ground + [_shadowed(small, dict(INNER, dx=25, dy=-20, x=3, y=3))])
    out["everything_shifted_out"] = _scene(ground + [_shadowed(_pair(), dict(INNER, dx=-W, dy=0))])
    out["opaque_object"] = _scene(ground + [_shadowed(small + [_rect(30, 22, 60, 46, (30, 160, 90, 255))], dict(INNER, x=4, y=6, passes=2, strength=2))])
    out["strength_255"] = _scene(ground + [_shadowed(_pair(), dict(INNER_GLOW, strength=255, color=(0, 200, 90, 90)))])
    out["box_1x1"] = _scene(ground + [_shadowed(_pair(), dict(INNER, x=1, y=1))])
    out["wider_than_frame"] = _scene(ground + [_shadowed(_pair(), dict(INNER_GLOW, x=255, y=255, strength=40))])
    tri = [_shape([(10, 5), (66, 12), (30, 48)], (0, 0, 0, 200))]
    out["inner_and_opacity"] = _scene(ground + [_shadowed(_pair(), INNER, "multiply", opacity=180)])
    out["inner_and_mask"] = _scene(ground + [_shadowed(_pair(), INNER_GLOW, mask=tri)])
    out["inside_faded"] = _scene(ground + [{"type": "container", "opacity": 140, "children": [_rect(4, 4, 30, 20, (250, 240, 30, 255)), _shadowed(_pair(), INNER)]}])
    out["inside_mask"] = _scene(ground + [{"type": "container", "mask": tri, "children": [_shadowed(_pair(), INNER_GLOW), _rect(40, 30, 70, 50, (20, 200, 60, 180))]}])
    for name, chain in LISTS.items():
        out["list_" + name] = _scene(ground + [_filtered(_pair(), chain)])
    out["list_and_mask_opacity"] = _scene(ground + [_filtered(_pair(), LISTS["drop_inner"], "multiply", opacity=200, mask=[_rect(12, 8, 60, 40, (0, 0, 0, 230))])])
    out["two_inner_and_an_outer"] = _scene(ground + [_shadowed(_pair(-6, -3), INNER), _shadowed(_pair(8, 6), dict(INNER_GLOW, knockout=True), "add"),
                                                     _shadowed([_shape([(20, 4), (50, 9), (36, 30)], (255, 255, 255, 120))], DROP)])
    return out


def source_scenes():
    """a bitmap fill (repeating, over a solid) and a radial gradient inside the group: the scenarios of tests/scenarios.py scaled into a
    96 x 64 frame, over a ground"""
    SC = scenarios.scenarios()
    out = {}
    for name, sh in (("bitmap_repeat_over_solid", dict(INNER, dx=6, dy=-4, x=5, y=4, passes=2)), ("gradient_radial", dict(INNER_GLOW, x=4, y=6))):
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
        out["cairo_inner_%soperators" % tag] = (operator_scenes, aliased)
        out["cairo_inner_%sstructure" % tag] = (structure_scenes, aliased)
        out["cairo_inner_%ssources" % tag] = (source_scenes, aliased)
    return out


def goldens():
    return {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())} for fname, (make, aliased) in files().items()}
