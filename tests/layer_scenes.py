"""Isolated-layer scenes ("Isolated layers"), built from tests/scenarios.py and tests/blend_scenes.py pieces, and their
libcairo reference: BlendReplay with cairo_push_group / cairo_pop_group_to_source / cairo_set_operator / cairo_paint around every object
that carries "layer".  tools/make_composite_goldens.py writes goldens() to tests/golden/cairo_layer_*.npz (premultiplied RGBA; key = scene
name); the tests rebuild the scenes from here, so a golden file holds pixels only.
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
import scenarios  # noqa: E402
from blend_scenes import _rect, _shape, _with_ground  # noqa: E402
from scenarios import _m  # noqa: E402

MODES = ["normal"] + sorted(bm.MODES)        # the nine operators a layer can be composited with ("normal": OVER)
LINEAR_BOUND = bs.LINEAR_BOUND               # the same derivation: +-1 LSB in the source, operator slope <= 2, one rounding
S1_CROPS = bs.S1_CROPS
S1_GROUP = 4                                 # neighbouring stars per layer in the 4K frame
golden_path = bs.golden_path
s1_arrays = bs.s1_arrays


def layer_mode_name(layer):
    """the operator name of a "layer" value (True / "normal" / "layer" / 0..2: OVER)"""
    if layer is True:
        return "normal"
    if isinstance(layer, str):
        name = layer.lower()
        return "normal" if name == "layer" else name
    return {v: k for k, v in bm.MODES.items()}.get(int(layer), "normal")


class LayerReplay(bs.BlendReplay):
    """BlendReplay whose objects may carry "layer": the object (its matrix, blend mode and all) is drawn into a group and the group
    painted with the operator of the layer's mode.  The operator in force around the layer stays in force inside it (cairo_push_group
    keeps the graphics state) and is restored behind the paint."""

    def _draw(self, obj):
        layer = obj.get("layer")
        if layer is None or layer is False:
            return super()._draw(obj)
        be = self.be
        lib, cr = be.lib, be.cr
        for fn in ("cairo_push_group", "cairo_pop_group_to_source", "cairo_paint"):
            f = getattr(lib, fn)
            f.restype, f.argtypes = None, [ctypes.c_void_p]
        lib.cairo_push_group(cr)
        try:
            super()._draw({k: v for k, v in obj.items() if k != "layer"})
        finally:
            lib.cairo_pop_group_to_source(cr)
            be.save()
            lib.cairo_set_operator(cr, bm.CAIRO_OPERATORS[layer_mode_name(layer)])
            lib.cairo_paint(cr)
            be.restore()


def cairo_render(sc, aliased=False, replay=LayerReplay):
    """premultiplied RGBA of a layer scene through libcairo (colour transforms by way of their lowering, tools/make_cxform_goldens.py)"""
    from oracle import cairo_backend as cb
    import make_cxform_goldens as mk
    be = cb.CairoBackend(sc["width"], sc["height"])
    try:
        if aliased:
            f = be.lib.cairo_set_antialias
            f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int]
            f(be.cr, bs.CAIRO_ANTIALIAS_NONE)
        if sc.get("even_odd"):
            be.set_fill_rule(True)
        low = mk.Lowering(sc.get("bitmaps", []))
        stage = low.lower(sc["stage"])
        rp = replay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in low.extra.items():
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


def without_layers(obj):
    """the same tree with every "layer" key dropped: today's per-path rule"""
    if isinstance(obj, list):
        return [without_layers(o) for o in obj]
    out = {k: v for k, v in obj.items() if k != "layer"}
    if "children" in out:
        out["children"] = without_layers(out["children"])
    return out


def _layer(mode, kids, **kw):
    return {"type": "container", "layer": mode, "children": list(kids), **kw}


def _pair(dx=0.0, dy=0.0):
    """two overlapping translucent triangles and a rectangle across both"""
    return [_shape([(8.3 + dx, 4.2 + dy), (58.6 + dx, 12.7 + dy), (20.2 + dx, 40.4 + dy)], (230, 40, 90, 150)),
            _shape([(30.1 + dx, 3.4 + dy), (61.2 + dx, 30.9 + dy), (12.5 + dx, 36.3 + dy)], (40, 200, 120, 119)),
            _rect(22 + dx, 18 + dy, 50.5 + dx, 44.25 + dy, (20, 60, 240, 200))]


def overlap_scenes():
    """every operator x {clear, opaque, translucent} ground: a layer of overlapping translucent children"""
    out = {}
    W, H = 72, 52
    for mode in MODES:
        for gname, ground in bs._grounds(W, H).items():
            out["%s_%s" % (mode, gname)] = dict(width=W, height=H, exact=True, stage={"children": ground + [_layer(mode, _pair())]})
    return out


def source_scenes(mode):
    """one operator: strokes over their own fills (miter, and round as a morph shape), gradients and bitmaps inside a layer, over an
    opaque and a translucent ground"""
    SC = scenarios.scenarios()
    out = {}
    for name, exact in (("stroke_curves", True), ("stroke_rectilinear_loop_scaled", True), ("morph_round_stroke_090", True),
                        ("gradient_radial", True), ("gradient_linear_ext", False), ("bitmap_magnified", True), ("bitmap_repeat_over_solid", True)):
        sc = SC[name]
        out["%s_%s" % (mode, name)] = dict(sc, exact=exact, stage={"children": _with_ground(sc) + [_layer(mode, sc["stage"]["children"])]})
    # a shape and a morph shape that are layers themselves (the "layer" key on the object, its matrix inside the group)
    sc = SC["stroke_curves"]
    out["%s_shape_layer" % mode] = dict(sc, exact=True, stage={"children": _with_ground(sc) + [dict(k, layer=mode) for k in sc["stage"]["children"]]})
    sc = SC["morph_round_stroke_255"]
    out["%s_morph_layer" % mode] = dict(sc, exact=True, stage={"children": _with_ground(sc) + [dict(k, layer=mode) for k in sc["stage"]["children"]]})
    return out


CLEAR_STATE = ("empty_first", "clear_fill", "clear_fill_multiply", "offframe_whole")


SPECK = _rect(63, 47, 64, 48, (0, 0, 0, 255))       # one opaque pixel in the corner of a 64 x 48 frame


def structure_scenes(modes=None):
    """what the walk, the culling and the clear-surface bookkeeping have to get right, per operator (`modes`: those operators only)"""
    modes = MODES if modes is None else modes
    import make_cxform_goldens as mk
    SC = scenarios.scenarios()
    out = {}
    W, H = 100, 100
    stack = SC["translucent_stack"]["stage"]["children"]
    ground = _with_ground(dict(width=W, height=H))
    fade = mk.cxform(mult=(256, 200, 128, 160), add=(0, 20, 60, 0))
    # (triangles whose pixels tell a SOURCE lerp's 0x7f rounding from OVER's 0x80: most do in a few pixels, some in none --
    #  tools/make_composite_goldens.py checks these with libcairo)
    follow = [_shape([(14.6, 7.3), (2.2, 44.1), (41.6, 29.3)], (84, 23, 95, 196)), _shape([(60.4, 43.4), (41.1, 33.1), (9.9, 2.8)], (31, 64, 179, 128))]
    for mode in modes:
        other = "hardlight" if mode != "hardlight" else "darken"
        # "blend_mode" paths inside a layer (each against the layer's own pixels), and a layer inside a "blend_mode" container
        out["blend_inside_%s" % mode] = dict(width=W, height=H, exact=True, stage={"children": ground + [
            _layer(mode, [stack[0], {"type": "container", "blend_mode": other, "children": stack[1:]},
                          dict(_shape([(10, 60), (70, 50), (40, 95)], (250, 250, 250, 200)), blend_mode="multiply")], matrix=_m(0.95, 0.95, 40, 30))]})
        out["layer_in_blend_%s" % mode] = dict(width=W, height=H, exact=True, stage={"children": ground + [
            {"type": "container", "blend_mode": other, "children": [stack[0], _layer(mode, stack[1:]), _shape([(5, 5), (60, 15), (20, 50)], (255, 30, 200, 230))]}]})
        out["layer_and_blend_%s" % mode] = dict(width=W, height=H, exact=True, stage={"children": ground + [
            {"type": "container", "layer": mode, "blend_mode": other, "children": stack}]})
        # layers nested 2, 3 and 4 deep, the operators differing from level to level
        for depth in (2, 3, 4):
            kids = _pair(10, 30)
            for lvl in range(depth - 1):
                m2 = MODES[(MODES.index(mode) + 2 * lvl + 1) % len(MODES)]
                kids = [_shape([(15 + 9 * lvl, 8), (90, 20 + 11 * lvl), (35, 80 - 6 * lvl)], (250 - 60 * lvl, 90 + 50 * lvl, 30 + 40 * lvl, 170)),
                        _layer(m2, kids), _rect(60 - 8 * lvl, 40, 92, 70 + 7 * lvl, (10 + 70 * lvl, 200, 160, 140))]
            out["nested%d_%s" % (depth, mode)] = dict(width=W, height=H, exact=True, stage={"children": ground + [_layer(mode, kids)]})
        # a colour transform inside and outside a layer (it recolours the definitions: the same pixels)
        out["cxform_outside_%s" % mode] = dict(width=W, height=H, exact=True, stage={"children": ground + [
            {"type": "container", "layer": mode, "color_transform": fade, "children": stack}]})
        out["cxform_inside_%s" % mode] = dict(width=W, height=H, exact=True, stage={"children": ground + [
            _layer(mode, [{"type": "container", "color_transform": fade, "children": stack}])]})
        # an opaque full-strip cover inside a group over an opaque ground: nothing outside the group may be culled
        out["cover_inside_%s" % mode] = dict(width=192, height=48, exact=True, stage={"children": [
            _rect(0, 0, 192, 48, (30, 160, 90, 255)), _rect(64, 16, 128, 32, (200, 60, 30, 255)),
            _layer(mode, [_rect(0, 0, 192, 48, (60, 50, 20, 255)), _shape([(5, 3), (180, 10), (90, 45)], (250, 200, 40, 200))]),
            _layer(mode, [_shape([(-10, -10), (300, -10), (300, 100), (-10, 100)], (30, 20, 70, 200)), _rect(64, 0, 128, 48, (9, 9, 9, 255))])]})
        # an opaque cover above a group hides it
        out["cover_above_%s" % mode] = dict(width=192, height=48, exact=True, stage={"children": [
            _rect(0, 0, 192, 48, (30, 160, 90, 255)), _layer(mode, [_shape([(5, 3), (180, 10), (90, 45)], (250, 200, 40, 200)), _rect(30, 8, 150, 40, (1, 2, 3, 99))]),
            _rect(0, 0, 128, 48, (10, 20, 30, 255)), _shape([(100, 2), (190, 20), (120, 46)], (255, 255, 255, 90))]})
        # a group that covers many strips of which its members touch few
        out["sparse_%s" % mode] = dict(width=256, height=64, exact=True, stage={"children": [
            _shape([(3, 60), (250, 2), (254, 62)], (90, 160, 30, 210)),
            _layer(mode, [_shape([(2, 2), (9, 3), (4, 9)], (250, 20, 40, 180)), _shape([(246, 52), (255, 55), (249, 63)], (20, 40, 250, 180)),
                          _shape([(120, 30), (131, 31), (124, 37)], (240, 240, 20, 120))])]})
        # a group partly and wholly off the frame
        out["offframe_part_%s" % mode] = dict(width=64, height=48, exact=True, stage={"children": [
            _shape([(2, 2), (60, 5), (30, 44)], (90, 160, 30, 210)), _layer(mode, _pair(30, 20)), _layer(mode, _pair(-25, -22))]})
        out["offframe_whole_%s" % mode] = dict(width=64, height=48, exact=True, stage={"children": [_layer(mode, _pair(80, 10))] + follow})
        # ---- the clear-surface bookkeeping: what the group leaves of the parent's "still clear" state shows in the rounding of the
        #      translucent triangles behind it (a SOURCE lerp's 0x7f or OVER's 0x80)
        out["empty_first_%s" % mode] = dict(width=64, height=48, exact=True, stage={"children": [_layer(mode, [])] + follow})
        out["clear_fill_%s" % mode] = dict(width=64, height=48, exact=True, stage={"children": [
            _layer(mode, [_shape([(2, 2), (60, 5), (30, 44)], (255, 255, 255, 0))])] + follow})
        out["clear_fill_multiply_%s" % mode] = dict(width=64, height=48, exact=True, stage={"children": [
            _layer(mode, [dict(_shape([(2, 2), (60, 5), (30, 44)], (255, 255, 255, 0)), blend_mode="multiply")])] + follow})
    # one translucent path alone in an OVER group over a ground: lerp then OVER, not OVER alone -- a layer is never a no-op
    for k, (tri, colour) in enumerate(() if "normal" not in modes else ((((24.7, 94.9), (83.9, 88.9), (38.9, 23.6)), (100, 220, 156, 191)),
                                        (((19.9, 54.6), (86.2, 28.7), (36.6, 98.3)), (250, 12, 202, 91)),
                                        (((2.9, 6.4), (97.7, 73.3), (91.3, 61.4)), (220, 203, 179, 41)))):
        out["single_over_%d" % k] = dict(width=W, height=H, exact=True, stage={"children": ground + [_layer("normal", [_shape(list(tri), colour)])]})
    return out


def wrong_rule_scenes():
    """For the scenes whose point is the bookkeeping: name -> (the same pixels by other means or None, the rule it must NOT be confused
    with).  tools/make_composite_goldens.py checks with libcairo that the first renders the same pixels and the second differs in at least
    one.  A clear-state scene's group changes no pixel, so the scene without it is the rule "the parent stays clear", and the scene
    with an opaque speck in a corner the triangles do not touch -- the speck painted into the expected image too -- the rule "the
    parent counts as drawn".  The parent stays clear behind a still-clear group under OVER and ADD only; the group holding a clear
    fill under multiply was drawn on.  single_over without its layer is the plain path."""
    sc = structure_scenes()
    out = {}
    for name, s in sc.items():
        kind, mode = name.rsplit("_", 1)
        if kind in CLEAR_STATE:
            kids = s["stage"]["children"]
            drawn = dict(s, stage={"children": [dict(SPECK)] + kids[1:]}, speck=True)
            clear = dict(s, stage={"children": kids[1:]})
            stays_clear = kind != "clear_fill_multiply" and mode in ("normal", "add")
            out[name] = (clear, drawn) if stays_clear else (drawn, clear)
        elif kind == "single_over":
            out[name] = (None, dict(s, stage={"children": without_layers(s["stage"]["children"])}))
    return out


def s1_stage():
    """S1 (the 4K benchmark scene) with its stars in layers of S1_GROUP neighbours, the nine operators in turn"""
    from swf_renderer_amd import api, synth
    pts, cols = synth.scene(**synth.S1)
    stage = api.stars_to_stage(pts, cols)
    kids = stage["children"]
    groups = [_layer(MODES[(i // S1_GROUP) % len(MODES)], kids[i:i + S1_GROUP]) for i in range(0, len(kids), S1_GROUP)]
    return dict(width=synth.S1["width"], height=synth.S1["height"], exact=True, stage=dict(stage, children=groups))


def files():
    """golden file name -> (scenes, aliased)"""
    out = {"cairo_layer_overlap": (overlap_scenes, False), "cairo_layer_aliased_overlap": (overlap_scenes, True)}
    for aliased in (False, True):
        for mode in MODES:
            out["cairo_layer_%ssources_%s" % ("aliased_" if aliased else "", mode)] = ((lambda mode=mode: source_scenes(mode)), aliased)
            out["cairo_layer_%sstructure_%s" % ("aliased_" if aliased else "", mode)] = ((lambda mode=mode: structure_scenes([mode])), aliased)
    return out


def goldens(with_s1=True):
    out = {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())} for fname, (make, aliased) in files().items()}
    if with_s1:
        out["cairo_layer_s1_crops"] = s1_arrays(cairo_render(s1_stage()))
    return out
