"""Layer-opacity scenes ("Layer opacity"), built from tests/scenarios.py, tests/blend_scenes.py, tests/layer_scenes.py and
tests/mask_scenes.py pieces, and their libcairo reference: MaskReplay with, around every object that carries "opacity",

    cairo_push_group; the object (with its "mask", composited in normal mode, if it has one); cairo_pop_group_to_source;
    cairo_set_operator(the mode of "layer", absent: OVER); cairo_paint_with_alpha(opacity / 255.0)

tools/make_composite_goldens.py writes goldens() to tests/golden/cairo_fade_*.npz (premultiplied RGBA; key = scene name); the tests rebuild
the scenes from here, so a golden file holds pixels only.  Every scene is at most 128 x 64.
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import blend_model as bm  # noqa: E402
import blend_scenes as bs  # noqa: E402
import layer_scenes as ls  # noqa: E402
import mask_scenes as ms  # noqa: E402
import scenarios  # noqa: E402
from blend_scenes import _rect, _shape  # noqa: E402
from layer_scenes import _layer, _pair  # noqa: E402
from mask_scenes import TRANSLUCENT_MASK, _masked, _scaled, _scene  # noqa: E402

MODES = ls.MODES                             # the nine operators a faded layer can be composited with ("normal": OVER)
LINEAR_BOUND = ls.LINEAR_BOUND               # (mul_un8 by the opacity has slope <= 1: tests/test_layer_gpu.py's bound carries over)
OPACITIES = (1, 128, 254)
golden_path = bs.golden_path
W, H = ms.W, ms.H


class FadeReplay(ms.MaskReplay):
    """MaskReplay whose objects may carry "opacity" (0..255): see the module's docstring.  The operator in force around the object
    stays in force inside the group and is restored behind the paint."""

    def _draw(self, obj):
        opacity = obj.get("opacity")
        if opacity is None:
            return super()._draw(obj)
        be = self.be
        lib, cr = be.lib, be.cr
        for fn, args in (("cairo_push_group", []), ("cairo_pop_group_to_source", []), ("cairo_paint_with_alpha", [ctypes.c_double])):
            f = getattr(lib, fn)
            f.restype, f.argtypes = None, [ctypes.c_void_p] + args
        lib.cairo_push_group(cr)
        try:
            super()._draw({k: v for k, v in obj.items() if k not in ("opacity", "layer")})
        finally:
            lib.cairo_pop_group_to_source(cr)
            be.save()
            lib.cairo_set_operator(cr, bm.CAIRO_OPERATORS[ls.layer_mode_name(obj.get("layer") or True)])
            lib.cairo_paint_with_alpha(cr, int(opacity) / 255.0)
            be.restore()


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a fade scene through libcairo"""
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
        rp = FadeReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in low.extra.items():
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


def without_opacity(obj):
    """the same tree with every "opacity" key dropped"""
    if isinstance(obj, list):
        return [without_opacity(o) for o in obj]
    out = {k: v for k, v in obj.items() if k != "opacity"}
    if "children" in out:
        out["children"] = without_opacity(out["children"])
    if out.get("mask") is not None:
        out["mask"] = without_opacity(out["mask"])
    return out


# ---- pieces
def _faded(mode, opacity, kids, **kw):
    obj = {"type": "container", "children": list(kids), "opacity": opacity, **kw}
    if mode is not None:
        obj["layer"] = mode
    return obj


def alpha_multiplier(opacity):
    """the colour transform a caller without layer opacity would reach for: alpha mult opacity / 255 in 8.8, per definition"""
    import make_cxform_goldens as mk
    return mk.cxform(mult=(256, 256, 256, (opacity * 256 + 127) // 255), add=(0, 0, 0, 0))


def operator_scenes():
    """every operator x opacity {1, 128, 254} over an opaque and a translucent ground, and opacity 128 over a clear one: overlapping
    translucent children faded as one image"""
    out = {}
    for mode in MODES:
        for gname, ground in bs._grounds(W, H).items():
            for opacity in OPACITIES if gname != "clear" else (128,):
                out["%s_%03d_%s" % (mode, opacity, gname)] = _scene(ground + [_faded(mode, opacity, _pair())])
    return out


def source_scenes():
    """gradient and bitmap members, strokes, "opacity" on a shape and on a morph shape, opacity 255 and 0, and the scene that tells
    "as a whole" from "per definition" """
    out = {}
    SC = scenarios.scenarios()
    ground = bs._with_ground(dict(width=128, height=64))
    for name, s, exact in (("gradient_radial", 0.5, True), ("gradient_focal", 0.5, True), ("gradient_linear_ext", 0.5, False),
                           ("bitmap_minified_rotated", 0.6, True), ("bitmap_repeat_over_solid", 0.5, True), ("stroke_curves", 0.5, True)):
        content, bitmaps = _scaled(name, s, 20, 1)
        kw = dict(bitmaps=bitmaps) if bitmaps else {}
        out["%s_normal_128" % name] = _scene(ground + [_faded(None, 128, [content] + _pair(60, 10))], 128, 64, exact, **kw)
        out["%s_multiply_200" % name] = _scene(ground + [_faded("multiply", 200, [content] + _pair(60, 10))], 128, 64, exact, **kw)
    # overlapping children under one alpha: faded as a whole the overlaps do not show through; a colour transform with the same alpha
    # multiplier fades every definition on its own (whole_not_per_definition differs from per_definition: the generator checks it)
    out["whole_not_per_definition"] = _scene(bs._grounds(W, H)["opaque"] + [_faded("layer", 128, _pair())])
    out["per_definition"] = _scene(bs._grounds(W, H)["opaque"] + [{"type": "container", "color_transform": alpha_multiplier(128), "children": _pair()}])
    # "opacity" on a shape (its matrix inside the group) and on a morph shape, with a mode
    tri = _shape([(8.3, 4.2), (58.6, 12.7), (20.2, 40.4)], (230, 40, 90, 150), matrix=scenarios._m(1, 1, 100, -60), opacity=90, layer="screen")
    out["shape_with_opacity"] = _scene(bs._grounds(W, H)["translucent"] + [tri])
    morph = SC["morph_round_stroke_090"]
    out["morph_with_opacity"] = _scene(bs._with_ground(morph)[:1] + [dict(morph["stage"]["children"][0], opacity=77, layer="hardlight")], 128, 64)
    # opacity 255 is the plain layer, opacity 0 draws nothing
    out["opacity_255"] = _scene(bs._grounds(W, H)["translucent"] + [_faded("difference", 255, _pair())])
    out["opacity_000"] = _scene(bs._grounds(W, H)["translucent"] + [_faded("difference", 0, _pair()), _shape([(2, 30), (40, 35), (9, 46)], (9, 200, 200, 99))])
    return out


CLEAR_STATE = ("empty_first", "clear_fill", "clear_fill_multiply", "offframe_whole", "painted")
CLEAR_STATE_OPACITIES = (0, 128)
SPECK = ls.SPECK


def _clear_state_kids(kind):
    """the children of a faded group that changes no pixel (`painted`: at opacity 0 only)"""
    clear_fill = _shape([(2, 2), (60, 5), (30, 44)], (255, 255, 255, 0))
    return {"empty_first": [], "clear_fill": [clear_fill], "clear_fill_multiply": [dict(clear_fill, blend_mode="multiply")],
            "offframe_whole": _pair(80, 10), "painted": _pair()}[kind]


def stays_clear(kind, mode, opacity):
    """fade_model.parent_stays_clear for the clear-state scenes"""
    import fade_model
    return fade_model.parent_stays_clear(mode, kind not in ("clear_fill_multiply", "painted"), opacity)


def structure_scenes():
    """what the walk, the culling and the clear-surface bookkeeping have to get right"""
    import make_cxform_goldens as mk
    out = {}
    ground = bs._grounds(W, H)["opaque"]
    tr = bs._grounds(W, H)["translucent"]
    tint = mk.cxform(mult=(256, 200, 128, 160), add=(0, 20, 60, 0))
    follow = ls.structure_scenes(["normal"])["empty_first_normal"]["stage"]["children"][1:]
    # faded groups nested four deep, the operators and opacities differing from level to level; with plain layers between
    kids = _pair(4, 3)
    for lvl, (mode, opacity) in enumerate((("screen", 200), ("multiply", 128), ("add", 60), ("normal", 230))):
        kids = [_shape([(3 + 5 * lvl, 3), (50, 8 + 4 * lvl), (10, 40 - 3 * lvl)], (20 + 60 * lvl, 90, 250 - 50 * lvl, 140)), _faded(mode, opacity, kids),
                _rect(40 - 6 * lvl, 30, 62, 46 - 2 * lvl, (250, 250 - 70 * lvl, 20, 120))]
    out["nested4"] = _scene(ground + kids[1:2])
    out["faded_in_layers"] = _scene(ground + [_layer("multiply", [_shape([(3, 3), (50, 8), (10, 40)], (20, 90, 250, 140)),
                                                                 _layer("add", [_rect(30, 4, 60, 30, (200, 20, 20, 100)), _faded("overlay", 99, _pair())])])])
    out["layer_in_faded"] = _scene(ground + [_faded("difference", 150, [_layer("screen", _pair()), _rect(30, 4, 60, 30, (200, 20, 20, 100))])])
    # faded around masked: "opacity" and "mask" on one object (type 13 around type 11 in normal mode), and nested by hand
    out["opacity_and_mask"] = _scene(ground + [_masked("hardlight", _pair(), TRANSLUCENT_MASK, opacity=140)])
    out["opacity_and_mask_normal"] = _scene(tr + [_masked(None, _pair(), TRANSLUCENT_MASK, opacity=1)])
    out["faded_around_masked"] = _scene(ground + [_faded("lighten", 180, [_shape([(3, 3), (50, 8), (10, 40)], (20, 90, 250, 140)), _masked("screen", _pair(), TRANSLUCENT_MASK)])])
    out["faded_in_content"] = _scene(ground + [_masked("darken", [_faded("add", 120, _pair()), _rect(40, 30, 62, 46, (250, 250, 20, 120))], TRANSLUCENT_MASK)])
    out["faded_in_mask"] = _scene(ground + [_masked("normal", _pair(), [_rect(30, 4, 60, 30, (200, 20, 20, 100)), _faded("multiply", 100, TRANSLUCENT_MASK)])])
    # "blend_mode" in force inside the group; colour transforms around and on the object (they recolour the definitions inside)
    out["blend_inside"] = _scene(ground + [{"type": "container", "blend_mode": "hardlight", "children": [
        _faded("add", 128, _pair() + [dict(_rect(10, 10, 40, 40, (0, 0, 0, 128)), blend_mode="multiply")])]}])
    out["blend_on_object"] = _scene(ground + [_faded("normal", 128, _pair(), blend_mode="multiply")])
    out["cxform_around"] = _scene(ground + [{"type": "container", "color_transform": tint, "children": [_faded("screen", 128, _pair())]}])
    out["cxform_on_object"] = _scene(ground + [_faded("screen", 128, _pair(), color_transform=tint)])
    # opaque full-strip covers inside a faded group hide nothing outside -- and, faded, are no covers; an opaque cover above hides the group
    out["cover_inside"] = _scene([_rect(0, 0, 128, 48, (30, 160, 90, 255)), _rect(64, 16, 128, 32, (200, 60, 30, 255)),
                                  _faded("multiply", 128, [_rect(0, 0, 128, 48, (60, 50, 20, 255)), _shape([(5, 3), (120, 10), (90, 45)], (250, 200, 40, 200))]),
                                  _faded("normal", 254, [_rect(64, 0, 128, 48, (60, 50, 120, 255))])], 128, 48)
    out["cover_above"] = _scene([_rect(0, 0, 128, 48, (30, 160, 90, 255)), _faded("add", 128, _pair()),
                                 _rect(0, 0, 64, 48, (10, 20, 30, 255)), _shape([(50, 2), (126, 20), (60, 46)], (255, 255, 255, 90))], 128, 48)
    # a group that covers many strips of which its members touch few; groups partly and wholly off the frame
    out["sparse"] = _scene([_shape([(3, 60), (125, 2), (127, 62)], (90, 160, 30, 210)),
                            _faded("screen", 128, [_shape([(2, 2), (19, 3), (4, 19)], (250, 20, 40, 180)), _shape([(100, 40), (127, 45), (110, 63)], (20, 40, 250, 180)),
                                                   _rect(60, 28, 75, 37, (1, 1, 1, 200))])], 128, 64)
    out["offframe_part"] = _scene([_shape([(2, 2), (60, 5), (30, 44)], (90, 160, 30, 210)), _faded("overlay", 128, _pair(30, 20)), _faded("normal", 77, _pair(-25, -22))])
    # ---- the clear-surface bookkeeping: what the faded group leaves of the parent's "still clear" state shows in the rounding of the
    #      translucent triangles behind it (a SOURCE lerp's 0x7f or OVER's 0x80)
    for mode in MODES:
        for kind in CLEAR_STATE:
            for opacity in CLEAR_STATE_OPACITIES if kind != "painted" else (0,):
                out["%s_%03d_%s" % (kind, opacity, mode)] = _scene([_faded(mode, opacity, _clear_state_kids(kind))] + follow)
    return out


def wrong_rule_scenes():
    """For the clear-state scenes: name -> (the same pixels by other means, the rule it must NOT be confused with).  The faded group
    changes no pixel, so the scene without it is the rule "the parent stays clear", and the scene with an opaque speck in a corner the
    triangles do not touch -- the speck painted into the expected image too -- the rule "the parent counts as drawn"."""
    out = {}
    for name, s in structure_scenes().items():
        head, _, mode = name.rpartition("_")
        kind, _, opacity = head.rpartition("_")
        if kind in CLEAR_STATE:
            kids = s["stage"]["children"]
            drawn = dict(s, stage={"children": [dict(SPECK)] + kids[1:]}, speck=True)
            clear = dict(s, stage={"children": kids[1:]})
            out[name] = (clear, drawn) if stays_clear(kind, mode, int(opacity)) else (drawn, clear)
    return out


def files():
    """golden file name -> (scenes, aliased)"""
    out = {}
    for aliased in (False, True):
        a = "aliased_" if aliased else ""
        out["cairo_fade_%ssources" % a] = (source_scenes, aliased)
        out["cairo_fade_%soperators" % a] = (operator_scenes, aliased)
        out["cairo_fade_%sstructure" % a] = (structure_scenes, aliased)
    return out


def solid_scenes():
    """(file name, scene name, scene, aliased) of every golden scene whose styles are all solid: what tests/frame_model.py can draw"""
    for fname, (make, aliased) in sorted(files().items()):
        for name, sc in sorted(make().items()):
            if not sc.get("bitmaps") and "gradient" not in name:
                yield fname, name, sc, aliased


def goldens():
    return {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())} for fname, (make, aliased) in files().items()}


# ---- random trees
def _levels(obj):
    """the levels of SWFR_MAX_LAYER_DEPTH the object's subtree needs: "opacity" takes one (and stands in for "layer"), a "mask" two
    (with or without "layer"), a "layer" alone one"""
    own = (1 if obj.get("opacity") is not None else 0) + (2 if obj.get("mask") is not None else 0)
    if own == 0 and obj.get("layer") not in (None, False):
        own = 1
    below = [_levels(c) for c in obj.get("children", [])] + [_levels(c) for c in obj.get("mask") or []]
    return own + max(below, default=0)


def rand_faded_scene(rng, **kw):
    """mask_scenes.rand_masked_scene -- random composited trees with layers, blend modes, colour transforms and masks -- with "opacity"
    put at random on containers, layers, masked objects and shapes, in the tree and in the mask lists, wherever the depth limit allows:
    mostly 1..254, now and then 0 and 255"""
    import layer_model as lm
    sc = ms.rand_masked_scene(rng, **kw)
    kids = sc["stage"]["children"]

    def opacity():
        r = int(rng.integers(0, 10))
        return 0 if r == 0 else (255 if r == 1 else int(rng.integers(1, 255)))

    def visit(obj):
        if rng.integers(0, 3) == 0:
            obj["opacity"] = opacity()
            if max(_levels(k) for k in kids) > lm.MAX_DEPTH:
                del obj["opacity"]
            elif "layer" not in obj and rng.integers(0, 2) == 0:
                obj["layer"] = MODES[int(rng.integers(0, 9))]
        for c in obj.get("children", []):
            visit(c)
        if obj.get("mask"):
            obj["mask"] = [dict(c) for c in obj["mask"]]             # (mask members are shared with the tree: copies get keys of their own)
            for c in obj["mask"]:
                if c["type"] == "shape":
                    visit(c)
    for k in kids:
        visit(k)
    return sc
