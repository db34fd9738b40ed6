"""Masked-layer scenes ("Masked layers"), built from tests/scenarios.py, tests/blend_scenes.py and tests/layer_scenes.py
pieces, and their libcairo reference: LayerReplay with, around every object that carries "mask",

    cairo_push_group; the object; content = cairo_pop_group; cairo_push_group; the mask list; mask = cairo_pop_group;
    cairo_set_source(content); cairo_set_operator(the mode of "layer", absent: OVER); cairo_mask(mask)

the mask list drawn in the parent's space, outside the object's own matrix, colour transform and blend mode.
tools/make_composite_goldens.py writes goldens() to tests/golden/cairo_mask_*.npz (premultiplied RGBA; key = scene name); the tests rebuild
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
import scenarios  # noqa: E402
from blend_scenes import _rect, _shape  # noqa: E402
from layer_scenes import _layer, _pair  # noqa: E402
from scenarios import _m  # noqa: E402

MODES = ls.MODES                             # the nine operators a masked layer can be composited with ("normal": OVER)
LINEAR_BOUND = ls.LINEAR_BOUND
golden_path = bs.golden_path
W, H = 64, 48


class MaskReplay(ls.LayerReplay):
    """LayerReplay whose objects may carry "mask" (a list of display objects): see the module's docstring.  The operator in force
    around the object stays in force inside both groups and is restored behind the cairo_mask."""

    def _draw(self, obj):
        mask = obj.get("mask")
        if mask is None:
            return super()._draw(obj)
        be = self.be
        lib, cr = be.lib, be.cr
        P = ctypes.c_void_p
        for fn, res, args in (("cairo_push_group", None, [P]), ("cairo_pop_group", P, [P]), ("cairo_set_source", None, [P, P]),
                              ("cairo_mask", None, [P, P]), ("cairo_pattern_destroy", None, [P])):
            f = getattr(lib, fn)
            f.restype, f.argtypes = res, args
        lib.cairo_push_group(cr)
        try:
            ls.LayerReplay._draw(self, {k: v for k, v in obj.items() if k not in ("mask", "layer")})
        finally:
            content = lib.cairo_pop_group(cr)
        lib.cairo_push_group(cr)
        try:
            for m in mask:
                self._draw(m)
        finally:
            mpat = lib.cairo_pop_group(cr)
        be.save()
        lib.cairo_set_source(cr, content)
        lib.cairo_set_operator(cr, bm.CAIRO_OPERATORS[ls.layer_mode_name(obj.get("layer") or True)])
        lib.cairo_mask(cr, mpat)
        be.restore()
        lib.cairo_pattern_destroy(mpat)
        lib.cairo_pattern_destroy(content)


def _lowering(bitmaps):
    """tools/make_cxform_goldens.py's Lowering, which also lowers the "mask" lists: under the transforms AROUND the object, not its own"""
    import make_cxform_goldens as mk

    class MaskLowering(mk.Lowering):
        def _object(self, obj, lut):
            out = super()._object(obj, lut)
            if obj.get("mask") is not None:
                out["mask"] = [self._object(c, lut) for c in obj["mask"]]
            return out
    return MaskLowering(bitmaps)


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a mask scene through libcairo"""
    from oracle import cairo_backend as cb
    be = cb.CairoBackend(sc["width"], sc["height"])
    try:
        if aliased:
            f = be.lib.cairo_set_antialias
            f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int]
            f(be.cr, bs.CAIRO_ANTIALIAS_NONE)
        if sc.get("even_odd"):
            be.set_fill_rule(True)
        low = _lowering(sc.get("bitmaps", []))
        stage = low.lower(sc["stage"])
        rp = MaskReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in low.extra.items():
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


def without_masks(obj):
    """the same tree with every "mask" key dropped"""
    if isinstance(obj, list):
        return [without_masks(o) for o in obj]
    out = {k: v for k, v in obj.items() if k != "mask"}
    if "children" in out:
        out["children"] = without_masks(out["children"])
    return out


# ---- pieces
def _masked(mode, kids, mask, **kw):
    obj = {"type": "container", "children": list(kids), "mask": list(mask), **kw}
    if mode is not None:
        obj["layer"] = mode
    return obj


def _scene(kids, w=W, h=H, exact=True, **kw):
    return dict(width=w, height=h, exact=exact, stage={"children": list(kids)}, **kw)


QUAD = [(12.4, 6.3), (56.2, 9.8), (50.7, 40.1), (15.6, 43.6)]
SOLID_MASK = [_shape(QUAD, (10, 200, 90, 255))]                                   # opaque: the mask's colour plays no part
TRANSLUCENT_MASK = [_shape(QUAD, (250, 20, 20, 140)), _shape([(5.5, 20.2), (60.3, 14.9), (33.1, 46.6)], (0, 0, 0, 77))]   # alpha 140, 77, and their OVER


def _scaled(name, s, tx=0.0, ty=0.0, only=None):
    """the children of a tests/scenarios.py scene inside a container that scales them by `s` and moves them by (tx, ty) pixels"""
    sc = scenarios.scenarios()[name]
    kids = sc["stage"]["children"]
    return {"type": "container", "matrix": _m(s, s, round(tx * 20), round(ty * 20)), "children": kids if only is None else [kids[only]]}, sc.get("bitmaps", [])


def _gradient_mask(tx=0.0, ty=0.0):
    """a radial gradient whose alpha runs 255 -> 60 -> 200 (tests/scenarios.py, gradient_alpha_over), about 60 x 52 pixels"""
    return [_scaled("gradient_alpha_over", 0.5, tx, ty, only=1)[0]]


def source_scenes():
    """solid, gradient and bitmap content under solid and gradient masks; a translucent mask; the geometry-only mask by way of a colour
    transform; strokes in the mask; "mask" on a shape and on a morph shape"""
    import make_cxform_goldens as mk
    out = {}
    for gname, ground in bs._grounds(W, H).items():
        out["solid_solidmask_%s" % gname] = _scene(ground + [_masked(None, _pair(), SOLID_MASK)])
        out["solid_translucentmask_%s" % gname] = _scene(ground + [_masked(None, _pair(), TRANSLUCENT_MASK)])
    ground = bs._with_ground(dict(width=128, height=64))
    out["solid_gradientmask"] = _scene(ground + [_masked(None, _pair(3, 2), _gradient_mask(2, 1))], 128, 64)
    for name, s, exact in (("gradient_radial", 0.5, True), ("gradient_focal", 0.5, True), ("gradient_linear_ext", 0.5, False),
                           ("bitmap_minified_rotated", 0.6, True), ("bitmap_repeat_over_solid", 0.5, True)):
        content, bitmaps = _scaled(name, s, 20, 1)
        kw = dict(bitmaps=bitmaps) if bitmaps else {}
        out["%s_solidmask" % name] = _scene(ground + [_masked(None, [content], [_shape([(22, 4), (90, 2), (84, 60), (30, 50)], (1, 2, 3, 255))])], 128, 64, exact, **kw)
        out["%s_gradientmask" % name] = _scene(ground + [_masked(None, [content], _gradient_mask(24, 3))], 128, 64, exact, **kw)
    # Flash's clip-depth mask, geometry only: the mask under a colour transform with alpha mult 0, add 255 (strokes count here)
    opaque = mk.cxform(mult=(256, 256, 256, 0), add=(0, 0, 0, 255))
    stroked = {"type": "shape", "definition": scenarios._poly_shape([(round(x * 20), round(y * 20)) for x, y in QUAD], {"type": "solid", "color": scenarios._rgba(9, 9, 9, 40)},
                                                                     line=scenarios._rgba(200, 0, 0, 90), line_width=80)}
    out["geometry_only_mask"] = _scene(bs._grounds(W, H)["opaque"] + [_masked(None, _pair(), [{"type": "container", "color_transform": opaque, "children": [stroked]}])])
    out["stroked_mask"] = _scene(bs._grounds(W, H)["opaque"] + [_masked(None, _pair(), [stroked])])
    # "mask" on a shape (its matrix moves the shape, not the mask) and on a morph shape, with a mode
    SC = scenarios.scenarios()
    tri = _shape([(8.3, 4.2), (58.6, 12.7), (20.2, 40.4)], (230, 40, 90, 150), matrix=_m(1, 1, 100, -60), mask=TRANSLUCENT_MASK, layer="screen")
    out["shape_with_mask"] = _scene(bs._grounds(W, H)["translucent"] + [tri])
    morph = SC["morph_round_stroke_090"]
    out["morph_with_mask"] = _scene(bs._with_ground(morph)[:1] + [dict(morph["stage"]["children"][0], mask=[_shape([(20, 10), (120, 20), (90, 80), (30, 70)], (0, 0, 0, 180))], layer="multiply")],
                                    128, 64)
    return out


def operator_scenes():
    """every operator x {clear, opaque, translucent} ground: overlapping translucent children through a translucent mask"""
    out = {}
    for mode in MODES:
        for gname, ground in bs._grounds(W, H).items():
            out["%s_%s" % (mode, gname)] = _scene(ground + [_masked(mode, _pair(), TRANSLUCENT_MASK)])
    return out


CLEAR_STATE = ("both_clear", "content_clear", "mask_clear", "mask_outside", "both_drawn_zero", "content_drawn_zero")
SPECK = ls.SPECK


def _clear_state_halves(kind):
    """(content, mask) of a masked group that changes no pixel: still-clear halves hold nothing, or a clear source under OVER (which
    leaves a surface clear); a half that was "drawn on" with every pixel zero holds a clear source under multiply"""
    clear_fill = _shape([(2, 2), (60, 5), (30, 44)], (255, 255, 255, 0))
    zero = dict(clear_fill, blend_mode="multiply")
    paint = _shape([(2, 2), (60, 5), (30, 44)], (90, 160, 30, 210))
    return {"both_clear": ([clear_fill], []), "content_clear": ([], [paint]), "mask_clear": ([paint], [clear_fill]),
            "mask_outside": ([paint], _pair(80, 10)), "both_drawn_zero": ([zero], [zero]), "content_drawn_zero": ([zero], [paint])}[kind]


def stays_clear(kind, mode):
    """mask_model.nothing_to_do for the clear-state scenes"""
    import mask_model
    content_clear = kind in ("both_clear", "content_clear")
    mask_clear = kind in ("both_clear", "mask_clear", "mask_outside")
    return mask_model.nothing_to_do(mode, content_clear, mask_clear)


def structure_scenes():
    """what the walk, the culling and the clear-surface bookkeeping have to get right"""
    import make_cxform_goldens as mk
    out = {}
    ground = bs._grounds(W, H)["opaque"]
    tr = bs._grounds(W, H)["translucent"]
    fade = mk.cxform(mult=(256, 200, 128, 160), add=(0, 20, 60, 0))
    follow = ls.structure_scenes(["normal"])["empty_first_normal"]["stage"]["children"][1:]
    # a mask partly and wholly off the frame, one that misses the content, content off the frame
    out["mask_offframe_part"] = _scene(ground + [_masked("normal", _pair(), [_shape([(30, -20), (90, 10), (50, 30)], (0, 0, 0, 200))]),
                                                 _masked("hardlight", _pair(), [_shape([(-20, 20), (25, 30), (10, 70)], (0, 0, 0, 220))])])
    out["mask_offframe_whole"] = _scene(ground + [_masked("multiply", _pair(), _pair(80, 10)), _shape([(2, 30), (40, 35), (9, 46)], (9, 200, 200, 99))])
    out["mask_misses_content"] = _scene(ground + [_masked("screen", [_rect(4, 4, 24.5, 20.25, (250, 0, 0, 200))], [_rect(34, 26, 60.5, 44.25, (0, 0, 0, 255))]),
                                                  _masked("difference", [_rect(4, 30, 30, 40, (0, 250, 0, 200))], [_rect(20, 26, 60.5, 44.25, (0, 0, 0, 150))])])
    out["content_offframe"] = _scene(tr + [_masked("add", _pair(80, 10), SOLID_MASK), _masked("overlay", _pair(-25, -22), TRANSLUCENT_MASK)])
    # masked inside masked (four levels), in the content half and in the mask half
    inner = _masked("screen", _pair(4, 3), [_shape([(20, 8), (60, 20), (28, 44)], (0, 0, 0, 170))])
    out["masked_in_content"] = _scene(ground + [_masked("lighten", [_shape([(3, 3), (50, 8), (10, 40)], (20, 90, 250, 140)), inner, _rect(40, 30, 62, 46, (250, 250, 20, 120))], TRANSLUCENT_MASK)])
    out["masked_in_mask"] = _scene(ground + [_masked("darken", _pair(), [_shape([(3, 3), (50, 8), (10, 40)], (20, 90, 250, 140)), inner])])
    # a masked group inside two plain layers; a plain layer inside each half
    out["masked_in_two_layers"] = _scene(ground + [_layer("multiply", [_shape([(3, 3), (50, 8), (10, 40)], (20, 90, 250, 140)),
                                                                      _layer("add", [_rect(30, 4, 60, 30, (200, 20, 20, 100)), _masked("overlay", _pair(), TRANSLUCENT_MASK)])])])
    out["layer_in_content"] = _scene(ground + [_masked("difference", [_layer("screen", _pair()), _rect(30, 4, 60, 30, (200, 20, 20, 100))], TRANSLUCENT_MASK)])
    out["layer_in_mask"] = _scene(ground + [_masked("normal", _pair(), [_rect(30, 4, 60, 30, (200, 20, 20, 100)), _layer("multiply", TRANSLUCENT_MASK)])])
    # "blend_mode" in force inside both halves (each path against its own group's pixels); colour transforms around and inside
    out["blend_inside"] = _scene(ground + [{"type": "container", "blend_mode": "hardlight", "children": [
        _masked("add", _pair(), TRANSLUCENT_MASK + [dict(_rect(10, 10, 40, 40, (0, 0, 0, 128)), blend_mode="multiply")])]}])
    out["blend_on_object"] = _scene(ground + [_masked("normal", _pair(), TRANSLUCENT_MASK, blend_mode="multiply")])
    out["cxform_around"] = _scene(ground + [{"type": "container", "color_transform": fade, "children": [_masked("screen", _pair(), TRANSLUCENT_MASK)]}])
    out["cxform_on_object"] = _scene(ground + [_masked("screen", _pair(), TRANSLUCENT_MASK, color_transform=fade)])
    # opaque full-strip covers inside either half hide nothing outside; an opaque cover above hides the group
    out["cover_inside"] = _scene([_rect(0, 0, 128, 48, (30, 160, 90, 255)), _rect(64, 16, 128, 32, (200, 60, 30, 255)),
                                  _masked("multiply", [_rect(0, 0, 128, 48, (60, 50, 20, 255)), _shape([(5, 3), (120, 10), (90, 45)], (250, 200, 40, 200))],
                                          [_rect(0, 0, 128, 48, (9, 9, 9, 255)), dict(_rect(0, 8, 128, 24, (0, 0, 0, 255)), blend_mode="difference")]),
                                  _masked("normal", [_rect(0, 0, 128, 48, (60, 50, 120, 255))], [_rect(64, 0, 128, 48, (9, 9, 9, 255)), _shape([(5, 3), (120, 10), (90, 45)], (250, 200, 40, 200))])], 128, 48)
    out["cover_above"] = _scene([_rect(0, 0, 128, 48, (30, 160, 90, 255)), _masked("add", _pair(), TRANSLUCENT_MASK),
                                 _rect(0, 0, 64, 48, (10, 20, 30, 255)), _shape([(50, 2), (126, 20), (60, 46)], (255, 255, 255, 90))], 128, 48)
    # a group that covers many strips of which each half touches few, and not the same ones
    out["sparse"] = _scene([_shape([(3, 60), (125, 2), (127, 62)], (90, 160, 30, 210)),
                            _masked("screen", [_shape([(2, 2), (19, 3), (4, 19)], (250, 20, 40, 180)), _shape([(100, 40), (127, 45), (110, 63)], (20, 40, 250, 180)), _rect(60, 28, 75, 37, (1, 1, 1, 200))],
                                    [_shape([(1, 1), (12, 3), (4, 12)], (0, 0, 0, 180)), _shape([(66, 30), (71, 31), (64, 37)], (0, 0, 0, 120)), _shape([(60, 2), (70, 3), (64, 9)], (0, 0, 0, 255))])], 128, 64)
    # ---- the clear-surface bookkeeping: what the masked group leaves of the parent's "still clear" state shows in the rounding of the
    #      translucent triangles behind it (a SOURCE lerp's 0x7f or OVER's 0x80)
    for mode in MODES:
        for kind in CLEAR_STATE:
            content, mask = _clear_state_halves(kind)
            out["%s_%s" % (kind, mode)] = _scene([_masked(mode, content, mask)] + follow)
    return out


def wrong_rule_scenes():
    """For the clear-state scenes: name -> (the same pixels by other means, the rule it must NOT be confused with).  The masked group
    changes no pixel, so the scene without it is the rule "the parent stays clear", and the scene with an opaque speck in a corner the
    triangles do not touch -- the speck painted into the expected image too -- the rule "the parent counts as drawn"."""
    out = {}
    for name, s in structure_scenes().items():
        kind, _, mode = name.rpartition("_")
        if kind in CLEAR_STATE:
            kids = s["stage"]["children"]
            drawn = dict(s, stage={"children": [dict(SPECK)] + kids[1:]}, speck=True)
            clear = dict(s, stage={"children": kids[1:]})
            out[name] = (clear, drawn) if stays_clear(kind, mode) else (drawn, clear)
    return out


def files():
    """golden file name -> (scenes, aliased)"""
    out = {}
    for aliased in (False, True):
        a = "aliased_" if aliased else ""
        out["cairo_mask_%ssources" % a] = (source_scenes, aliased)
        out["cairo_mask_%soperators" % a] = (operator_scenes, aliased)
        out["cairo_mask_%sstructure" % a] = (structure_scenes, aliased)
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
    """the levels of SWFR_MAX_LAYER_DEPTH the object's subtree needs: a "mask" takes two (with or without "layer"), a "layer" one"""
    own = 2 if obj.get("mask") is not None else (1 if obj.get("layer") not in (None, False) else 0)
    below = [_levels(c) for c in obj.get("children", [])] + [_levels(c) for c in obj.get("mask") or []]
    return own + max(below, default=0)


def rand_masked_scene(rng, **kw):
    """composite_scenes.rand_composited_scene with "mask" lists put at random on containers, layers and shapes wherever the depth limit
    allows: masks of one to three shapes taken from the tree (their own keys kept: blend modes, layers, colour transforms), now and
    then a masked group of its own, an empty list, a mask moved off the frame; masked groups inside masked groups in both halves."""
    import copy
    import composite_scenes as cs
    import layer_model as lm
    sc = cs.rand_composited_scene(rng, **kw)
    pool = []

    def collect(obj):
        if obj["type"] == "shape":
            pool.append(obj)
        for c in obj.get("children", []):
            collect(c)
    for k in sc["stage"]["children"]:
        collect(k)

    def mask_list(room):
        r = int(rng.integers(0, 12))
        if r == 0:
            return []
        picks = [copy.copy(pool[int(rng.integers(0, len(pool)))]) for _ in range(int(rng.integers(1, 4)))]
        picks = [p if _levels(p) <= room else {k: v for k, v in p.items() if k != "layer"} for p in picks]
        if r == 1:
            return [{"type": "container", "matrix": _m(1, 1, (sc["width"] + 60) * 20, 0), "children": picks}]
        if r < 4 and room >= 2:
            return [picks[0], {"type": "container", "children": picks[1:] or picks, "mask": [copy.copy(pool[int(rng.integers(0, len(pool)))])], "layer": MODES[int(rng.integers(0, 9))]}]
        return picks

    def visit(obj, used):
        if obj.get("mask") is None and rng.integers(0, 4) == 0:
            below = max([_levels(c) for c in obj.get("children", [])], default=0)
            if used + 2 + below <= lm.MAX_DEPTH:
                m = [c for c in mask_list(lm.MAX_DEPTH - used - 2)]
                m = [c if _levels(c) <= lm.MAX_DEPTH - used - 2 else {k: v for k, v in c.items() if k not in ("layer", "mask")} for c in m]
                obj["mask"] = m
                if rng.integers(0, 3) == 0 and "layer" not in obj:
                    obj["layer"] = MODES[int(rng.integers(0, 9))]
        own = 2 if obj.get("mask") is not None else (1 if obj.get("layer") not in (None, False) else 0)
        for c in obj.get("children", []):
            visit(c, used + own)
    kids = [copy.deepcopy(k) for k in sc["stage"]["children"]]      # (definitions are shared by identity in the pool: deep copies of the tree only)
    for k in kids:
        visit(k, 0)
    return dict(sc, stage={"children": kids})
