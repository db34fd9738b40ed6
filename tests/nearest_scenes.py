"""Unsmoothed bitmap fill scenes ("Unsmoothed bitmap fills") and their libcairo reference: tests/pad_scenes.py's PadReplay
-- so that "pad", "blend_mode", "layer", "mask" and "opacity" mean what they mean in the other families -- over a backend that sets
cairo_pattern_set_filter(CAIRO_FILTER_NEAREST) (cairo_filter_t 3) on the surface pattern of a fill that carries "filter": "nearest".

tools/make_nearest_goldens.py writes goldens() to tests/golden/cairo_nearest_*.npz (premultiplied RGBA; key = scene name); the tests
rebuild the scenes from here, so a golden file holds pixels only.  Frames are 96 x 48 and 300 x 40 (five tile columns, three
tile-rows).

The bitmaps: tests/pad_scenes.py's 1 x 1, 2 x 2, 3 x 5 and 8 x 8 and a 6 x 3, every texel its own colour; 1 x 7 and 7 x 1 (one texel
wide / high: what a relaxed "strictly inside" test of the transposed fetch would get wrong); and one 80 x 24, neighbouring texels
of different colours, large enough that a whole wavefront's 64 samples lie strictly inside it at 1:1 and at 3 x (the fast path of the
transposed fetch) while the neighbouring strips straddle its rim (the general routine).

A morph shape's fills are solid by the format's decoder (a bitmap fill there is refused, with or without a filter), so the morph
scene is a morph shape composited over a nearest fill.

The `cxform` files stay out of files() for the reason tests/pad_scenes.py gives: variant textures belong to the handle that walked
the stage.
"""
import ctypes
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import blend_scenes as bs  # noqa: E402
import mask_scenes as ms  # noqa: E402
import pad_scenes as ps  # noqa: E402
from pad_scenes import _at, _box, _quad, _shape  # noqa: E402
from scenarios import _m, _poly_shape, _rgba  # noqa: E402

LINEAR_BOUND = ps.LINEAR_BOUND               # (no scene here has a linear gradient: everything is exact)
golden_path = bs.golden_path
W, H = ps.W, ps.H
EXTENDS = ps.EXTENDS
CAIRO_FILTER_NEAREST = 3                     # cairo_filter_t


# ---- the libcairo reference
def _backend(width, height):
    from oracle import cairo_backend as cb

    class NearestBackend(cb.CairoBackend):
        """CairoBackend whose surface patterns get cairo_pattern_set_extend(self.extend) and cairo_pattern_set_filter(self.filter)
        where those are set"""
        extend = None
        filter = None

        def set_fill_pattern(self, bitmap, repeat):
            super().set_fill_pattern(bitmap, repeat)
            extend = self._fill[2] if self.extend is None else self.extend
            self._fill = self._fill[:2] + (extend, self.filter)

        def _apply_source(self, src):
            super()._apply_source(src)
            if src[0] == "pattern" and len(src) > 3 and src[3] is not None:
                self.lib.cairo_pattern_set_filter(src[1], src[3])
    return NearestBackend(width, height)


class NearestReplay(ps.PadReplay):
    """PadReplay that hands an unsmoothed fill's filter to the backend before the path is drawn.  The decoded path keeps the fill's
    "smoothed" as it stands in the tag, so for_cairo() writes "nearest" there for a fill that carries that filter."""

    def _draw_path(self, path):
        self.be.filter = CAIRO_FILTER_NEAREST if path.get("fill", {}).get("smoothed") == "nearest" else None
        return super()._draw_path(path)


def is_nearest(fill):
    return fill.get("filter") in ("nearest", 1) and not isinstance(fill.get("filter"), bool)


def for_cairo(obj):
    """pad_scenes.for_cairo, and every bitmap fill with "filter": "nearest" (or 1) says "smoothed": "nearest" (what NearestReplay reads)"""
    if isinstance(obj, list):
        return [for_cairo(o) for o in obj]
    if isinstance(obj, dict):
        out = {k: for_cairo(v) for k, v in obj.items()}
        if out.get("type") == "bitmap":
            if out.get("pad"):
                assert not out.get("repeating")
                out["repeating"] = "pad"
            if is_nearest(out):
                out["smoothed"] = "nearest"
        return out
    return obj


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a scene through libcairo; sc["raw_bitmaps"]: id -> (width, height, straight RGBA bytes)"""
    be = _backend(sc["width"], sc["height"])
    try:
        if aliased:
            f = be.lib.cairo_set_antialias
            f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int]
            f(be.cr, bs.CAIRO_ANTIALIAS_NONE)
        low = ms._lowering(sc.get("bitmaps", []))
        stage = low.lower(for_cairo(sc["stage"]))
        rp = NearestReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in list(low.extra.items()) + list(sc.get("raw_bitmaps", {}).items()):
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


def with_filter(obj, value):
    """the same tree with the filter of every bitmap fill replaced: "good", "nearest", 0, 1, or None for no key at all"""
    if isinstance(obj, list):
        return [with_filter(o, value) for o in obj]
    if isinstance(obj, dict):
        out = {k: with_filter(v, value) for k, v in obj.items() if not (k == "filter" and obj.get("type") == "bitmap")}
        if out.get("type") == "bitmap" and value is not None:
            out["filter"] = value
        return out
    return obj


with_extend = ps.with_extend                 # (keeps "filter": it drops and sets "pad" and "repeating" alone)


# ---- pieces
SIZES = {**ps.SIZES, 15: (1, 7), 16: (7, 1), 17: (80, 24), 18: (6, 3)}              # bitmap id -> (width, height)


def _tag(bid):
    """a DefineBitmap (image/x-swf-bmp, format 3).  Up to 256 texels: every texel a colour of its own; the 80 x 24 one: 256 colours, no
    texel the colour of a neighbour (the index steps by 3 along a row and by 89 down a column, modulo 256)"""
    w, h = SIZES[bid]
    n = min(w * h, 256)
    rng = np.random.default_rng(100 + bid)
    table, seen = np.zeros((n, 3), np.uint8), set()
    for k in range(n):
        while True:
            c = tuple(int(v) for v in rng.integers(0, 256, 3))
            if c not in seen:
                break
        seen.add(c)
        table[k] = c
    padded = w + (-w) % 4
    idx = np.zeros((h, padded), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    idx[:, :w] = (np.arange(w * h).reshape(h, w) if w * h <= 256 else (3 * xx + 89 * yy) % 256)
    data = bytes([3, w & 255, w >> 8, h & 255, h >> 8, n - 1]) + zlib.compress(table.tobytes() + idx.tobytes())
    return {"type": "define-bitmap", "id": bid, "width": w, "height": h, "media_type": "image/x-swf-bmp", "data": data.hex()}


BITMAPS = ps.BITMAPS + [_tag(bid) for bid in sorted(SIZES) if bid not in ps.SIZES]


def _fill(bid, matrix, extend="none", filter="nearest"):
    f = {"type": "bitmap", "bitmap_id": bid, "repeating": extend == "repeat", "smoothed": False, "matrix": matrix}
    if extend == "pad":
        f["pad"] = True
    if filter is not None:
        f["filter"] = filter
    return f


def _scene(kids, w=W, h=H, **kw):
    return dict(width=w, height=h, exact=True, bitmaps=BITMAPS, stage={"children": kids}, **kw)


GROUND = ps.GROUND
_whole = lambda fill, **kw: _shape(_quad(2, 1, 94, 47), fill, **kw)
_rot = lambda k, t, x, y: _m(20 * k * np.cos(t), 20 * k * np.cos(t), round(20 * x), round(20 * y), 20 * k * np.sin(t), -20 * k * np.sin(t))


# ---- the groups
def extend_scenes(extend):
    """one edge rule: 3 x and 7.3 x magnified, 1:1 at a fractional offset, 0.45 x and 0.3 x minified (where CAIRO_FILTER_GOOD convolves),
    rotated (magnified and minified) -- slanted quadrilaterals that reach past the bitmap on every side; the small bitmaps, the ones a
    texel wide / high among them; the 80 x 24 bitmap at 1:1 and 3 x (a whole wavefront strictly inside, its neighbours on the rim)"""
    out = {}
    f = lambda bid, matrix: _fill(bid, matrix, extend)
    out["magnified_3"] = _scene([_whole(f(14, _at(3, 3, 30.3, 10.6)))])
    out["magnified_7_3"] = _scene([_whole(f(13, _at(7.3, 7.3, 34.9, 4.9)))])
    out["one_to_one_fractional"] = _scene([_whole(f(14, _at(1, 1, 40.35, 18.6))), _shape(_box(3, 3, 30, 20), f(17, _at(1, 1, -20.45, -1.7)))])
    out["minified_045"] = _scene([_whole(f(17, _at(0.45, 0.45, 30.2, 17.3)))])
    out["minified_03"] = _scene([_whole(f(17, _at(0.3, 0.3, 36.6, 20.4)))])
    out["minified_mixed"] = _scene([_whole(f(14, _at(0.5, 3.0, 44.3, 10.7)))])
    out["rotated"] = _scene([_whole(f(13, _rot(4, 0.6, 45, 15)))])
    out["rotated_minified"] = _scene([_whole(f(17, _rot(0.55, 0.6, 30, 12)))])
    out["mirrored"] = _scene([_whole(f(13, _at(-3.25, 4.5, 52.6, 11.1)))])
    out["small_bitmaps"] = _scene([_shape(_quad(1, 1, 24, 47), f(11, _at(5, 5, 10.4, 20.9))), _shape(_quad(25, 1, 48, 47), f(12, _at(3.25, 3.25, 33.7, 20.2))),
                                   _shape(_quad(49, 1, 72, 47), f(15, _at(4.5, 3.5, 58.3, 12.6))), _shape(_quad(73, 1, 95, 47), f(16, _at(1.75, 6.5, 78.2, 20.4)))])
    out["thin_minified"] = _scene([_shape(_quad(1, 1, 47, 47), f(15, _at(0.6, 0.4, 22.3, 21.6))), _shape(_quad(49, 1, 95, 47), f(16, _at(0.4, 0.7, 70.2, 23.4)))])
    # 80 x 24 at 1:1 from (-3.6, 5.3): the strip of columns 0 .. 63, rows 8 .. 23 lies strictly inside; columns 64 .. 95 cross the rim
    out["large_1"] = _scene([_shape(_box(0, 0, 96, 48), f(17, _at(1, 1, -3.6, 5.3)))])
    # at 3 x from (-40.5, -10.5) it covers the frame (240 x 72 pixels): every strip inside; from (20.4, 6.6) on the wide frame its rim
    # crosses the strips of columns 0 .. 63 and 256 .. 299
    out["large_3"] = _scene([_shape(_quad(0, 0, 96, 48), f(17, _at(3, 3, -40.5, -10.5)))])
    out["large_3_wide"] = _scene([_shape(_quad(3, 1, 297, 39), f(17, _at(3, 3, 20.4, -6.6)))], 300, 40)
    return out


def edge_boxes():
    """the texel-edge fills: a pixel-aligned box over the 6 x 3 bitmap whose every sample lies exactly on a texel edge on both axes --
    1:1 with the translation at an odd half pixel, 2 x at (30, 10) twips modulo 40 / 20, 0.5 x at (10, 10) twips -- per edge rule.
    -> name -> dict(matrix, rect, extend): a box on a clear frame, so tests/nearest_model.py says what the frame holds"""
    out = {}
    for extend in EXTENDS:
        out["edge_1_%s" % extend] = dict(matrix=_m(20, 20, 20 * 40 + 10, 20 * 20 + 10), rect=(34, 17, 52, 25), extend=extend)
        out["edge_2_%s" % extend] = dict(matrix=_m(40, 40, 20 * 40 + 30, 20 * 20 + 10), rect=(36, 18, 54, 26), extend=extend)
        out["edge_05_%s" % extend] = dict(matrix=_m(10, 10, 20 * 40 + 10, 20 * 20 + 10), rect=(34, 17, 52, 25), extend=extend)
    return out


EDGE_BITMAP = 18


def edge_scenes():
    return {name: _scene([_shape(_box(*b["rect"]), _fill(EDGE_BITMAP, b["matrix"], b["extend"]))]) for name, b in edge_boxes().items()}


def _pair(extend="none"):
    """a magnified and a minified nearest fill side by side, both reaching past their bitmaps"""
    return [_shape(_quad(2, 1, 50, 47), _fill(13, _at(3.5, 3.5, 20.3, 14.6), extend)), _shape(_quad(46, 3, 94, 45), _fill(17, _at(0.45, 0.3, 52.2, 20.9), extend))]


def shape_scenes():
    """a triangle and a stroked shape with a nearest fill, antialiased rows crossing the cut; a nearest and a good fill of one bitmap in
    one frame (per edge rule); a morph shape over a nearest fill; shapes that fit their bitmap exactly; coverage 255 everywhere"""
    import scenarios
    out = {}
    out["triangle"] = _scene(GROUND + [_shape([(5.5, 3.2), (90.3, 8.9), (38.1, 45.6)], _fill(14, _at(6.5, 3.75, 22.4, 9.3)))])
    stroked = {"type": "shape", "definition": _poly_shape([(round(20 * x), round(20 * y)) for x, y in _quad(8, 5, 88, 43)], _fill(13, _at(9.25, 5.5, 30.6, 9.8)),
                                                          line=_rgba(20, 30, 200, 180), line_width=70)}
    out["stroked"] = _scene(GROUND + [stroked])
    for extend in EXTENDS:
        out["nearest_beside_good_%s" % extend] = _scene([_shape(_quad(1, 2, 47, 46), _fill(13, _at(4.5, 4.5, 17.4, 12.7), extend)),
                                                         _shape(_quad(49, 2, 95, 46), _fill(13, _at(4.5, 4.5, 65.4, 12.7), extend, filter="good"))])
    msc = scenarios.scenarios()["morph_color_030"]
    morph = msc["stage"]["children"][1]
    k = 0.9 * min(W / msc["width"], H / msc["height"])
    out["morph_over_nearest"] = _scene([_whole(_fill(14, _at(5.5, 5.5, 20.3, 2.6), "repeat")),
                                        dict(morph, matrix=_m(k, k, round(k * morph["matrix"]["translate_x"]) + 60, round(k * morph["matrix"]["translate_y"]) + 40))])
    out["fitted"] = _scene([_shape(_box(x, y, x + k * SIZES[bid][0], y + k * SIZES[bid][1]), _fill(bid, _at(k, k, x, y)))
                            for bid, k, x, y in ((14, 3, 2, 3), (13, 2.5, 30.35, 2.6), (12, 7.75, 44.2, 3.4), (11, 7.75, 64, 4), (15, 4, 76.5, 5.5), (16, 3, 3.25, 36.5))])
    out["full_coverage"] = _scene([_shape(_box(0, 0, 96, 48), _fill(13, _at(9, 6, 34, 9), "pad"))])
    return out


def structure_scenes():
    """the nearest pair under "blend_mode", "layer", "mask" and "opacity"; and the 300 x 40 frame of the two-band routes"""
    out = {}
    pair = _pair("pad")
    out["blend_mode"] = _scene(GROUND + [dict(p, blend_mode="multiply") for p in _pair("repeat")])
    out["layer"] = _scene(GROUND + [{"type": "container", "layer": "screen", "children": _pair("none") + [bs._rect(30, 8, 70, 30, (200, 20, 20, 100))]}])
    out["mask"] = _scene(GROUND + [{"type": "container", "children": pair, "mask": [bs._shape([(12.4, 6.3), (86.2, 9.8), (80.7, 40.1), (15.6, 43.6)], (10, 200, 90, 200))]}])
    out["opacity"] = _scene(GROUND + [{"type": "container", "opacity": 150, "children": pair + [bs._rect(30, 8, 70, 30, (200, 20, 20, 100))]}])
    out["wide"] = _scene([_shape(_quad(3, 1, 297, 39), _fill(14, _at(6.5, 3.25, 120.4, 6.6))), _shape(_quad(200, 4, 290, 36), _fill(13, _at(0.4, 0.4, 240.4, 18.6), "repeat"))], 300, 40)
    return out


def cxform_scenes():
    """the nearest pair under colour transforms -- variant textures: the texels are recoloured, the addressing stays -- one of which
    makes every texel translucent"""
    import make_cxform_goldens as mk
    out = {}
    tint = mk.cxform(mult=(256, 200, 128, 256), add=(0, 20, 60, 0))
    veil = mk.cxform(mult=(256, 230, 256, 150), add=(0, 0, 10, 0))
    out["cxform_tint"] = _scene(GROUND + [{"type": "container", "color_transform": tint, "children": _pair("none")}])
    out["cxform_translucent"] = _scene(GROUND + [{"type": "container", "color_transform": veil, "children": _pair("pad")}])
    out["cxform_translucent_repeat"] = _scene(GROUND + [{"type": "container", "color_transform": veil, "children": _pair("repeat")}])
    return out


GROUPS = dict({e: (lambda e=e: extend_scenes(e)) for e in EXTENDS}, edges=edge_scenes, shapes=shape_scenes, structure=structure_scenes)
CXFORM_GROUPS = {"cxform": cxform_scenes}
MINIFIED = ("minified_045", "minified_03", "minified_mixed", "rotated_minified", "thin_minified")       # (where CAIRO_FILTER_GOOD convolves)


def all_scenes():
    out = {}
    for group, make in list(GROUPS.items()) + list(CXFORM_GROUPS.items()):
        out.update({"%s/%s" % (group, name): sc for name, sc in make().items()})
    return out


def _files(groups):
    return {"cairo_nearest_%s%s" % ("aliased_" if aliased else "", group): (make, aliased) for aliased in (False, True) for group, make in groups.items()}


def files():
    """golden file name -> (scenes, aliased): what every device route must reproduce byte for byte"""
    return _files(GROUPS)


def cxform_files():
    """the same for the colour-transformed scenes (the module's docstring: not in files())"""
    return _files(CXFORM_GROUPS)


def goldens():
    return {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())}
            for fname, (make, aliased) in dict(files(), **cxform_files()).items()}


# ---- random single boxes (tests/test_nearest_model.py against libcairo, tests/test_nearest_gpu.py against the model)
FW, FH = ps.FW, ps.FH


def random_box_case(rng, extend, minified=None):
    """pad_scenes.random_box_case with the edge rule `extend` and the nearest filter on its fill"""
    case = ps.random_box_case(rng, minified)
    sc = case["scene"]
    case["scene"] = dict(sc, stage=with_filter(with_extend(sc["stage"], extend), "nearest"))
    case["minified"] = min(np.hypot(case["model"]["matrices"][0]["scale_x"], case["model"]["matrices"][0]["rotate_skew0"]),
                           np.hypot(case["model"]["matrices"][0]["scale_y"], case["model"]["matrices"][0]["rotate_skew1"])) < 0.75 * 20 * 65536
    return case
