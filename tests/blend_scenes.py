"""Blend-mode scenes ("Blend modes"), built from tests/scenarios.py pieces, and their libcairo reference: CanvasReplay with
cairo_set_operator around every object that carries a "blend_mode" -- what CanvasRenderer would do if it set
ctx.globalCompositeOperation before drawing the object.  tools/make_composite_goldens.py writes goldens() to
tests/golden/cairo_blend_*.npz (premultiplied RGBA; key = scene name); the tests rebuild the scenes from here, so a golden file holds
pixels only.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import canvas_replay as cr  # noqa: E402
import blend_model as bm  # noqa: E402
import scenarios  # noqa: E402
from scenarios import _m, _poly_shape, _rgba  # noqa: E402

GOLD = os.path.join(HERE, "golden")
MODES = sorted(bm.MODES)
LINEAR_BOUND = 3                       # LSB: linear gradients are the +-1 LSB extension; the modes have slope up to 2 in s, plus one rounding
S1_CROPS = ((0, 0), (2432, 768), (1792, 1024), (3584, 1904), (960, 320))
CAIRO_ANTIALIAS_NONE = 1


def golden_path(fname):
    return os.path.join(GOLD, fname + ".npz")


class BlendReplay(cr.CanvasReplay):
    """CanvasReplay whose objects may carry "blend_mode": the Cairo operator of the mode is set (inside a save / restore) around the
    object, so it holds for every path below it until an inner object sets another; "normal" restores OVER."""

    def _draw(self, obj):
        mode = obj.get("blend_mode")
        if mode is None:
            return super()._draw(obj)
        name = mode.lower() if isinstance(mode, str) else {v: k for k, v in dict(bm.MODES, normal=1).items()}[max(int(mode), 1)]
        be = self.be
        be.save()
        try:
            be.lib.cairo_set_operator(be.cr, bm.CAIRO_OPERATORS[name])
            super()._draw({k: v for k, v in obj.items() if k != "blend_mode"})
        finally:
            be.restore()


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a blend scene through libcairo (colour transforms by way of their lowering, tools/make_cxform_goldens.py)"""
    import ctypes
    from oracle import cairo_backend as cb
    import make_cxform_goldens as mk
    be = cb.CairoBackend(sc["width"], sc["height"])
    try:
        if aliased:
            f = be.lib.cairo_set_antialias
            f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int]
            f(be.cr, CAIRO_ANTIALIAS_NONE)
        if sc.get("even_odd"):
            be.set_fill_rule(True)
        low = mk.Lowering(sc.get("bitmaps", []))
        stage = low.lower(sc["stage"])
        rp = BlendReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in low.extra.items():
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


# ---- pieces
def _shape(pts_px, colour, **kw):
    return {"type": "shape", "definition": _poly_shape([(round(x * 20), round(y * 20)) for x, y in pts_px], {"type": "solid", "color": _rgba(*colour)}), **kw}


def _rect(x0, y0, x1, y1, colour, **kw):
    return _shape([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], colour, **kw)


def _grounds(w, h):
    """what lies below the blended paths: nothing (the surface is still clear), an opaque and a translucent quadrilateral that leave
    a margin of the frame clear, so that every blended shape crosses covered and clear pixels"""
    quad = [(3.3, 2.6), (w - 2.2, 4.1), (w - 5.4, h - 3.2), (1.7, h - 6.3)]
    return {"clear": [], "opaque": [_shape(quad, (200, 120, 40, 255))], "translucent": [_shape(quad, (60, 140, 220, 150))]}


def solid_scenes():
    """every mode x {opaque, alpha 119, alpha 1} solid x {clear, opaque, translucent} ground: a slanted triangle, a pixel-aligned and an
    unaligned rectangle per colour.  Over the clear ground the first triangle is the frame's FIRST paint (add: a SOURCE lerp), the
    rest are later ones"""
    out = {}
    W, H = 96, 72
    for mode in MODES:
        for gname, ground in _grounds(W, H).items():
            kids = []
            for k, a in enumerate((255, 119, 1)):
                x = 4 + 31 * k
                col = (230 - 60 * k, 40 + 70 * k, 90 + 50 * k, a)
                kids += [_shape([(x + 1.3, 1.2), (x + 27.6, 9.7), (x + 8.2, 30.4)], col),
                         _rect(x + 2, 34, x + 22, 50, col),
                         _rect(x + 3.37, 52.21, x + 24.62, 69.45, col),
                         _rect(x + 12, 44, x + 29, 60, (col[0], 255 - col[1], col[2], a))]       # (overlaps the two before it)
            out["%s_%s" % (mode, gname)] = dict(width=W, height=H, exact=True, stage={"children": ground + [
                {"type": "container", "blend_mode": mode, "children": kids}]})
    return out


def _with_ground(sc):
    w, h = sc["width"], sc["height"]
    ground = [_shape([(w * 0.05, h * 0.1), (w * 0.7, h * 0.02), (w * 0.6, h * 0.8), (w * 0.1, h * 0.95)], (220, 200, 60, 255)),
              _shape([(w * 0.4, h * 0.3), (w * 0.97, h * 0.2), (w * 0.9, h * 0.97), (w * 0.5, h * 0.7)], (40, 90, 200, 140))]
    return ground


def source_scenes(mode):
    """one mode over an opaque and a translucent ground: strokes over their own fills (miter and, as a morph shape at two ratios, round),
    radial, focal and linear gradients, bitmaps (repeat / no-repeat, magnified / minified)"""
    SC = scenarios.scenarios()
    out = {}

    def blended(name, which=None, ground=True, exact=True):
        sc = SC[name]
        kids = list(sc["stage"]["children"])
        which = range(len(kids)) if which is None else which
        for i in which:
            kids[i] = dict(kids[i], blend_mode=mode)
        o = dict(sc, stage={"children": (_with_ground(sc) if ground else []) + kids}, exact=exact)
        out["%s_%s" % (mode, name)] = o

    blended("stroke_curves")                                   # a stroke over its own fill
    blended("stroke_rectilinear_loop_scaled")                  # box paths: a translucent box stroke over its own translucent fill
    blended("morph_round_stroke_090")                          # round caps and joins, translucent, over the shape's own fills
    blended("morph_round_stroke_255")
    blended("morph_color_030", which=[1], ground=False)        # interpolated colours
    blended("gradient_radial")
    blended("gradient_focal")
    blended("gradient_alpha_over", which=[1], ground=False)    # translucent stops over an opaque shape and clear pixels
    blended("gradient_linear_ext", exact=False)
    blended("bitmap_magnified")
    blended("bitmap_no_repeat_magnified", which=[0])           # the bitmap first (add: a lerp), the translucent solid OVER it
    blended("bitmap_no_repeat_minified", which=[1])
    blended("bitmap_repeat_over_solid", which=[1])
    blended("bitmap_minified_rotated")
    return out


def structure_scenes():
    """what the walk and the culling have to get right"""
    import make_cxform_goldens as mk
    SC = scenarios.scenarios()
    out = {}
    W, H = 100, 100
    stack = SC["translucent_stack"]["stage"]["children"]
    ground = _with_ground(dict(width=W, height=H))
    fade = mk.cxform(mult=(256, 200, 128, 160), add=(0, 20, 60, 0))
    for mode in ("multiply", "overlay", "add", "difference", "screen"):
        # a blended container with overlapping children (no group isolation: each path on its own)
        out["container_%s" % mode] = dict(width=W, height=H, exact=True, stage={"children": ground + [
            {"type": "container", "blend_mode": mode, "matrix": _m(0.95, 0.95, 40, 30), "children": stack}]})
        # the blend wrapper outside and inside a colour transform: the same pixels
        out["cxform_outside_%s" % mode] = dict(width=W, height=H, exact=True, stage={"children": ground + [
            {"type": "container", "blend_mode": mode, "color_transform": fade, "children": stack}]})
        out["cxform_inside_%s" % mode] = dict(width=W, height=H, exact=True, stage={"children": ground + [
            {"type": "container", "color_transform": fade, "children": [{"type": "container", "blend_mode": mode, "children": stack}]}]})
        # nested modes: the innermost wins, an inner normal restores OVER
        out["nested_%s" % mode] = dict(width=W, height=H, exact=True, stage={"children": ground + [
            {"type": "container", "blend_mode": mode, "children": [
                stack[0],
                {"type": "container", "blend_mode": "normal", "children": [_shape([(10, 60), (70, 50), (40, 95)], (250, 250, 250, 200))]},
                {"type": "container", "blend_mode": "hardlight" if mode != "hardlight" else "darken", "children": [
                    _shape([(55, 5), (95, 30), (60, 70)], (20, 220, 120, 180)),
                    dict(_rect(20, 20, 50, 45, (255, 255, 0, 255)), blend_mode=0)]},
                _shape([(5, 5), (60, 15), (20, 50)], (255, 30, 200, 230))]}]})
        # a blended path that fully covers an opaque one below it, strip for strip: nothing may be culled
        out["cover_below_%s" % mode] = dict(width=192, height=48, exact=True, stage={"children": [
            _rect(0, 0, 192, 48, (30, 160, 90, 255)), _rect(64, 16, 128, 32, (200, 60, 30, 255)),
            dict(_rect(0, 0, 192, 48, (60, 50, 20, 255)), blend_mode=mode),           # (dark enough for ADD not to saturate)
            dict(_shape([(-10, -10), (300, -10), (300, 100), (-10, 100)], (30, 20, 70, 255)), blend_mode=mode)]})
        # an opaque cover above blended paths: it hides them
        out["cover_above_%s" % mode] = dict(width=192, height=48, exact=True, stage={"children": [
            _rect(0, 0, 192, 48, (30, 160, 90, 255)),
            dict(_shape([(5, 3), (180, 10), (90, 45)], (250, 200, 40, 200)), blend_mode=mode),
            _rect(0, 0, 128, 48, (10, 20, 30, 255)), _shape([(100, 2), (190, 20), (120, 46)], (255, 255, 255, 90))]})
        # a clear source under an operator other than ADD is an operation all the same: the translucent fill behind it is no longer
        # the surface's first paint (OVER's 0x80 rounding, not the SOURCE lerp's 0x7f)
        out["clear_source_first_%s" % mode] = dict(width=64, height=48, exact=True, stage={"children": [
            dict(_shape([(2, 2), (60, 5), (30, 44)], (255, 255, 255, 0)), blend_mode=mode),
            _shape([(4, 40), (20, 3), (61, 30)], (200, 100, 50, 119)), _shape([(1, 1), (40, 20), (5, 30)], (20, 100, 250, 77))]})
    return out


def s1_stage():
    """S1 (the 4K benchmark scene) with every third star blended, the modes in turn"""
    from swf_renderer_amd import api, synth
    pts, cols = synth.scene(**synth.S1)
    stage = api.stars_to_stage(pts, cols)
    for i, kid in enumerate(stage["children"]):
        if i % 3 == 2:
            kid["blend_mode"] = MODES[(i // 3) % len(MODES)]
    return dict(width=synth.S1["width"], height=synth.S1["height"], exact=True, stage=stage)


def files():
    """golden file name -> (scenes, aliased)"""
    out = {"cairo_blend_solids": (solid_scenes, False), "cairo_blend_structure": (structure_scenes, False),
           "cairo_blend_aliased_solids": (solid_scenes, True), "cairo_blend_aliased_structure": (structure_scenes, True)}
    for mode in MODES:
        out["cairo_blend_sources_" + mode] = ((lambda mode=mode: source_scenes(mode)), False)
    for mode in MODES:
        out["cairo_blend_aliased_sources_" + mode] = ((lambda mode=mode: source_scenes(mode)), True)
    return out


def s1_arrays(img):
    out = {"sha256": np.frombuffer(hashlib.sha256(np.ascontiguousarray(img).tobytes()).digest(), np.uint8).copy()}
    for x, y in S1_CROPS:
        out["%d_%d" % (x, y)] = img[y:y + 256, x:x + 256].copy()
    return out


def goldens(with_s1=True):
    out = {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())} for fname, (make, aliased) in files().items()}
    if with_s1:
        out["cairo_blend_s1_crops"] = s1_arrays(cairo_render(s1_stage()))
        out["cairo_blend_aliased_s1_crops"] = s1_arrays(cairo_render(s1_stage(), aliased=True))
    return out
